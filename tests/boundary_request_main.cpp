// What a handle allows of the boundary terms (csrc/sns_policy.h: policy::check_boundary_request, and the rule
// policy::check_form_request gained for the shape gradient) on its own, for tests/test_host_boundary.py::test_boundary_request_table.
// stdin holds one question per line:
//   b REQUEST DIM PARTITIONED HAS_FACETS                          a boundary request
//   f REQUEST DIM PARTITIONED TT VL BF EV BOUNDARY_FLOW           a form request with the seventh fact
// stdout the verdict of each: the error code, a tab, the message tail.  First line: BREQ_COUNT.
#include <cstdio>

#include "sns_policy.h"

int main() {
    using namespace sns::policy;
    char kind;
    std::printf("%d\n", (int)BREQ_COUNT);
    while (std::scanf(" %c", &kind) == 1) {
        FormVerdict v;
        if (kind == 'b') {
            int req, dim, part, facets;
            if (std::scanf("%d %d %d %d", &req, &dim, &part, &facets) != 4) return 2;
            v = check_boundary_request((BoundaryRequest)req, {dim, part != 0, facets != 0});
        } else if (kind == 'f') {
            int req, dim, part, tt, vl, bf, ev, bnd;
            if (std::scanf("%d %d %d %d %d %d %d %d", &req, &dim, &part, &tt, &vl, &bf, &ev, &bnd) != 8) return 2;
            v = check_form_request((FormRequest)req, {dim, part != 0, tt != 0, vl != 0, bf != 0, ev != 0, bnd != 0});
        } else {
            return 2;
        }
        std::printf("%d\t%s\n", v.error, v.tail);
    }
    return 0;
}
