// The verdicts of the complex-shift entry points (csrc/sns_policy.h: policy::check_shifted_args behind the stability family's rows
// asked as SREQ_ARNOLDI or SREQ_ARNOLDI_LEFT for sns_stability_arnoldi_shifted; policy::check_shifted_coefficient behind the rows
// asked as SREQ_MASS_APPLY[_TRANSPOSE] for sns_shifted_apply and sns_shifted_solve) on their own, for
// tests/test_host_complex_shift.py; built like tests/request_main.cpp.  stdin holds one question per line:
//   P LEFT DIM PARTITIONED TT VL BF EV FACETS TRACTION BACKFLOW M K SHIFT_RE SHIFT_IM PC_SHIFT BREAKDOWN_REL      the process
//   O LEFT DIM PARTITIONED TT VL BF EV FACETS TRACTION BACKFLOW C_RE C_IM                                          the operator
// stdout the verdict of each: the error code, a tab, the message tail.  First line: SREQ_COUNT, SREQ_KINDS, STABILITY_M_MIN,
// STABILITY_M_MAX.  Exit code 2: a malformed question.
#include <cstdio>
#include <cstdlib>

#include "sns_policy.h"

int main() {
    using namespace sns::policy;
    std::printf("%d %d %d %d\n", (int)SREQ_COUNT, (int)SREQ_KINDS, STABILITY_M_MIN, STABILITY_M_MAX);
    char kind[8];
    while (std::scanf("%7s", kind) == 1) {
        int left, dim, b[8];
        if (std::scanf("%d %d %d %d %d %d %d %d %d %d", &left, &dim, b, b + 1, b + 2, b + 3, b + 4, b + 5, b + 6, b + 7) != 10) return 2;
        if ((left != 0 && left != 1) || kind[1] != 0) return 2;
        const HandleFacts f{dim, b[0] != 0, b[1] != 0, b[2] != 0, b[3] != 0, b[4] != 0, b[5] != 0, b[6] != 0, b[7] != 0};
        Verdict v;
        if (kind[0] == 'P') {
            int m, k;
            char t[4][64];
            if (std::scanf("%d %d %63s %63s %63s %63s", &m, &k, t[0], t[1], t[2], t[3]) != 6) return 2;
            const ShiftedArgs a{m, k, std::strtod(t[0], nullptr), std::strtod(t[1], nullptr), std::strtod(t[2], nullptr),
                                std::strtod(t[3], nullptr)};
            v = check_stability_shifted_request(left ? SREQ_ARNOLDI_LEFT : SREQ_ARNOLDI, f, a);
        } else if (kind[0] == 'O') {
            char t[2][64];
            if (std::scanf("%63s %63s", t[0], t[1]) != 2) return 2;
            v = check_shifted_operator_request(left ? SREQ_MASS_APPLY_TRANSPOSE : SREQ_MASS_APPLY, f, std::strtod(t[0], nullptr),
                                               std::strtod(t[1], nullptr));
        } else {
            return 2;
        }
        std::printf("%d\t%s\n", v.error, v.tail);
    }
    return 0;
}
