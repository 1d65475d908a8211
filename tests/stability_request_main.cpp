// What a handle allows of the stability analysis (csrc/sns_policy.h: policy::check_stability_request) on its own, for
// tests/test_host_stability.py::test_stability_request_rules.  stdin holds one question per line:
//   REQUEST DIM PARTITIONED TT VL M SHIFT BREAKDOWN_REL         (SHIFT and BREAKDOWN_REL as strtod reads them: nan, inf, -inf too)
// stdout the verdict of each: the error code, a tab, the message tail.  First line: SREQ_COUNT, STABILITY_M_MIN, STABILITY_M_MAX.
#include <cstdio>
#include <cstdlib>

#include "sns_policy.h"

int main() {
    using namespace sns::policy;
    std::printf("%d %d %d\n", (int)SREQ_COUNT, STABILITY_M_MIN, STABILITY_M_MAX);
    int req, dim, part, tt, vl, m;
    char s1[64], s2[64];
    while (std::scanf("%d %d %d %d %d %d %63s %63s", &req, &dim, &part, &tt, &vl, &m, s1, s2) == 8) {
        const FormVerdict v = check_stability_request((StabilityRequest)req, {dim, part != 0, tt != 0, vl != 0},
                                                      {m, std::strtod(s1, nullptr), std::strtod(s2, nullptr)});
        std::printf("%d\t%s\n", v.error, v.tail);
    }
    return 0;
}
