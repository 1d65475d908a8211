// The request family of the raw Jacobian (csrc/sns_policy.h: FAMILY_RAW_JACOBIAN behind policy::check_raw_jacobian_request) on its
// own, for tests/test_host_rawjac.py; built like tests/request_main.cpp.  stdin holds one question per line:
//   REQUEST DIM PARTITIONED TT VL BF EV FACETS TRACTION BACKFLOW FORM ALIASED VARIANT
// REQUEST: the value in policy::RawJacobianRequest; FORM ALIASED VARIANT: the arguments of sns_raw_jacobian_apply (the form id,
// x_dev == y_dev, a perturbed form variant set), read and ignored for the other request.  stdout the verdict of each: the error
// code, a tab, the message tail.  First line: JREQ_COUNT, FAMILY_RAW_JACOBIAN, FAMILY_STATE_GRADIENT.  Exit code 2: a malformed
// question.
#include <cstdio>

#include "sns_policy.h"

int main() {
    using namespace sns::policy;
    std::printf("%d %d %d\n", (int)JREQ_COUNT, (int)FAMILY_RAW_JACOBIAN, (int)FAMILY_STATE_GRADIENT);
    int req, dim, b[8], form, aliased, variant;
    while (std::scanf("%d", &req) == 1) {
        if (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %d", &dim, b, b + 1, b + 2, b + 3, b + 4, b + 5, b + 6, b + 7, &form, &aliased,
                       &variant) != 12)
            return 2;
        if (req < 0 || req >= JREQ_COUNT) return 2;
        const HandleFacts f{dim, b[0] != 0, b[1] != 0, b[2] != 0, b[3] != 0, b[4] != 0, b[5] != 0, b[6] != 0, b[7] != 0};
        const Verdict v = check_raw_jacobian_request((RawJacobianRequest)req, f, {form, aliased != 0, variant != 0});
        std::printf("%d\t%s\n", v.error, v.tail);
    }
    return 0;
}
