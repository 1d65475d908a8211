// The request family of the resolvent analysis (csrc/sns_policy.h: FAMILY_RESOLVENT behind policy::check_resolvent_energy_request
// and policy::check_resolvent_lanczos_request) on its own, for tests/test_host_resolvent.py; built like tests/request_main.cpp.
// stdin holds one question per line:
//   REQUEST DIM PARTITIONED TT VL BF EV FACETS TRACTION BACKFLOW N OMEGA BREAKDOWN_REL ALIASED
// REQUEST: the value in policy::ResolventRequest.  RREQ_ENERGY: N = parts and ALIASED = x_dev == y_dev of sns_energy_apply (OMEGA
// and BREAKDOWN_REL are read and ignored; sns_lumped_volumes asks with parts = 1, not aliased).  RREQ_LANCZOS: N = m, OMEGA,
// BREAKDOWN_REL and ALIASED = V_dev is the state or a weight, of sns_resolvent_lanczos.  stdout the verdict of each: the error
// code, a tab, the message tail.  First line: RREQ_COUNT, FAMILY_RESOLVENT, FAMILY_RAW_JACOBIAN.  Exit code 2: a malformed question.
#include <cstdio>

#include "sns_policy.h"

int main() {
    using namespace sns::policy;
    std::printf("%d %d %d\n", (int)RREQ_COUNT, (int)FAMILY_RESOLVENT, (int)FAMILY_RAW_JACOBIAN);
    int req, dim, b[8], n, aliased;
    double omega, rel;
    while (std::scanf("%d", &req) == 1) {
        if (std::scanf("%d %d %d %d %d %d %d %d %d %d %lf %lf %d", &dim, b, b + 1, b + 2, b + 3, b + 4, b + 5, b + 6, b + 7, &n, &omega, &rel,
                       &aliased) != 13)
            return 2;
        if (req < 0 || req >= RREQ_COUNT) return 2;
        const HandleFacts f{dim, b[0] != 0, b[1] != 0, b[2] != 0, b[3] != 0, b[4] != 0, b[5] != 0, b[6] != 0, b[7] != 0};
        const Verdict v = req == RREQ_ENERGY ? check_resolvent_energy_request(f, {n, aliased != 0})
                                             : check_resolvent_lanczos_request(f, {n, omega, rel, aliased != 0});
        std::printf("%d\t%s\n", v.error, v.tail);
    }
    return 0;
}
