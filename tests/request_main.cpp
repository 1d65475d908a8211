// What a handle's state allows (csrc/sns_policy.h: the one rule table behind policy::check_form_request, check_boundary_request,
// check_stability_request and check_state_gradient_request) on its own, for the five request tests (tests/request_gate.py).
// stdin holds one question per line:
//   FAMILY REQUEST DIM PARTITIONED TT VL BF EV FACETS TRACTION BACKFLOW [arguments]
// FAMILY: f the form requests, b the boundary setters, s the stability analysis (arguments M SHIFT BREAKDOWN_REL), g the Hessian
// pass (REQUEST 0; arguments C_JAC C_MASS); REQUEST: the value in the family's enum; the real arguments as strtod reads them
// (nan, inf, -inf too).  stdout the verdict of each: the error code, a tab, the message tail -- and for the left-hand kinds of
// the stability analysis, after another tab, the right-hand kind's verdict in the same form.
// First line: REQ_COUNT BREQ_COUNT SREQ_COUNT SREQ_KINDS STABILITY_M_MIN STABILITY_M_MAX.  Exit code 2: a malformed question.
#include <cstdio>
#include <cstdlib>

#include "sns_policy.h"

int main() {
    using namespace sns::policy;
    std::printf("%d %d %d %d %d %d\n", (int)REQ_COUNT, (int)BREQ_COUNT, (int)SREQ_COUNT, (int)SREQ_KINDS, STABILITY_M_MIN, STABILITY_M_MAX);
    char family;
    int req, dim, b[8];
    while (std::scanf(" %c", &family) == 1) {
        if (std::scanf("%d %d %d %d %d %d %d %d %d %d", &req, &dim, b, b + 1, b + 2, b + 3, b + 4, b + 5, b + 6, b + 7) != 10) return 2;
        const HandleFacts f{dim, b[0] != 0, b[1] != 0, b[2] != 0, b[3] != 0, b[4] != 0, b[5] != 0, b[6] != 0, b[7] != 0};
        char s1[64], s2[64];
        Verdict v;
        if (family == 'f' && req >= 0 && req < REQ_COUNT) {
            v = check_form_request((FormRequest)req, f);
        } else if (family == 'b' && req >= 0 && req < BREQ_COUNT) {
            v = check_boundary_request((BoundaryRequest)req, f);
        } else if (family == 's' && req >= 0 && req < SREQ_KINDS) {
            int m;
            if (std::scanf("%d %63s %63s", &m, s1, s2) != 3) return 2;
            const ArnoldiArgs a{m, std::strtod(s1, nullptr), std::strtod(s2, nullptr)};
            v = check_stability_request((StabilityRequest)req, f, a);
            if (req >= SREQ_COUNT) {
                const Verdict r = check_stability_request((StabilityRequest)(req - SREQ_COUNT), f, a);
                std::printf("%d\t%s\t%d\t%s\n", v.error, v.tail, r.error, r.tail);
                continue;
            }
        } else if (family == 'g' && req == 0) {
            if (std::scanf("%63s %63s", s1, s2) != 2) return 2;
            v = check_state_gradient_request(f, std::strtod(s1, nullptr), std::strtod(s2, nullptr));
        } else {
            return 2;
        }
        std::printf("%d\t%s\n", v.error, v.tail);
    }
    return 0;
}
