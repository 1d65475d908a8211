// What a handle allows of the left-hand stability entry points (csrc/sns_policy.h: policy::check_stability_request with the
// kinds SREQ_MASS_APPLY_TRANSPOSE and SREQ_ARNOLDI_LEFT) on its own, for
// tests/test_host_left_modes.py::test_left_request_rules.  stdin holds one question per line:
//   REQUEST DIM PARTITIONED TT VL M SHIFT BREAKDOWN_REL         (REQUEST: 0 the transposed mass pass, 1 the left Arnoldi process;
//                                                                SHIFT and BREAKDOWN_REL as strtod reads them: nan, inf, -inf too)
// stdout two verdicts per question, tab separated: the left-hand kind's error code and message tail, then the right-hand kind's
// (SREQ_MASS_APPLY / SREQ_ARNOLDI).  First line: SREQ_COUNT, SREQ_MASS_APPLY_TRANSPOSE, SREQ_ARNOLDI_LEFT, SREQ_KINDS.
#include <cstdio>
#include <cstdlib>

#include "sns_policy.h"

int main() {
    using namespace sns::policy;
    std::printf("%d %d %d %d\n", (int)SREQ_COUNT, (int)SREQ_MASS_APPLY_TRANSPOSE, (int)SREQ_ARNOLDI_LEFT, (int)SREQ_KINDS);
    int req, dim, part, tt, vl, m;
    char s1[64], s2[64];
    while (std::scanf("%d %d %d %d %d %d %63s %63s", &req, &dim, &part, &tt, &vl, &m, s1, s2) == 8) {
        const StabilityFacts f{dim, part != 0, tt != 0, vl != 0};
        const ArnoldiArgs a{m, std::strtod(s1, nullptr), std::strtod(s2, nullptr)};
        const FormVerdict l = check_stability_request(req == 0 ? SREQ_MASS_APPLY_TRANSPOSE : SREQ_ARNOLDI_LEFT, f, a);
        const FormVerdict r = check_stability_request(req == 0 ? SREQ_MASS_APPLY : SREQ_ARNOLDI, f, a);
        std::printf("%d\t%s\t%d\t%s\n", l.error, l.tail, r.error, r.tail);
    }
    return 0;
}
