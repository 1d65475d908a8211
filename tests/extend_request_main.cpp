// The verdict of sns_stability_arnoldi_extend (csrc/sns_policy.h: policy::check_arnoldi_extend_args behind the stability family's
// rows, asked as SREQ_ARNOLDI or SREQ_ARNOLDI_LEFT) on its own, for tests/test_host_krylov_schur.py; built like
// tests/request_main.cpp.  stdin holds one question per line:
//   LEFT DIM PARTITIONED TT VL BF EV FACETS TRACTION BACKFLOW M SHIFT BREAKDOWN_REL K
// stdout the verdict of each: the error code, a tab, the message tail, a tab, then the same pair for the plain Arnoldi request of
// that side with the same m, shift and breakdown_rel.  First line: SREQ_COUNT, SREQ_KINDS, STABILITY_M_MIN, STABILITY_M_MAX.
// Exit code 2: a malformed question.
#include <cstdio>
#include <cstdlib>

#include "sns_policy.h"

int main() {
    using namespace sns::policy;
    std::printf("%d %d %d %d\n", (int)SREQ_COUNT, (int)SREQ_KINDS, STABILITY_M_MIN, STABILITY_M_MAX);
    int left, dim, b[8], m, k;
    char shift[64], brel[64];
    while (std::scanf("%d", &left) == 1) {
        if (std::scanf("%d %d %d %d %d %d %d %d %d %d %63s %63s %d", &dim, b, b + 1, b + 2, b + 3, b + 4, b + 5, b + 6, b + 7, &m, shift,
                       brel, &k) != 13)
            return 2;
        if (left != 0 && left != 1) return 2;
        const HandleFacts f{dim, b[0] != 0, b[1] != 0, b[2] != 0, b[3] != 0, b[4] != 0, b[5] != 0, b[6] != 0, b[7] != 0};
        const StabilityRequest request = left ? SREQ_ARNOLDI_LEFT : SREQ_ARNOLDI;
        const ArnoldiArgs a{m, std::strtod(shift, nullptr), std::strtod(brel, nullptr)};
        const Verdict v = check_stability_extend_request(request, f, a, k);
        const Verdict p = check_stability_request(request, f, a);
        std::printf("%d\t%s\t%d\t%s\n", v.error, v.tail, p.error, p.tail);
    }
    return 0;
}
