// What a handle allows of the Hessian pass (csrc/sns_policy.h: policy::check_state_gradient_request) on its own, for
// tests/test_host_hessian.py::test_request_rules.  stdin holds one question per line:
//   DIM PARTITIONED TT VL BF EV TRACTION BACKFLOW C_JAC C_MASS      (the coefficients as strtod reads them: nan, inf, -inf too)
// stdout one verdict per question, tab separated: the error code and the message tail.  First line: SREQ_COUNT and SREQ_KINDS,
// which the new function leaves as they were.
#include <cstdio>
#include <cstdlib>

#include "sns_policy.h"

int main() {
    using namespace sns::policy;
    std::printf("%d %d\n", (int)SREQ_COUNT, (int)SREQ_KINDS);
    int dim, part, tt, vl, bf, ev, tr, bk;
    char s1[64], s2[64];
    while (std::scanf("%d %d %d %d %d %d %d %d %63s %63s", &dim, &part, &tt, &vl, &bf, &ev, &tr, &bk, s1, s2) == 10) {
        const StateGradientFacts f{dim, part != 0, tt != 0, vl != 0, bf != 0, ev != 0, tr != 0, bk != 0};
        const FormVerdict v = check_state_gradient_request(f, std::strtod(s1, nullptr), std::strtod(s2, nullptr));
        std::printf("%d\t%s\n", v.error, v.tail);
    }
    return 0;
}
