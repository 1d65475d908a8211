// What a handle's form state allows (csrc/sns_policy.h: policy::check_form_request) on its own, for
// tests/test_host.py::test_form_request_table: stdin holds one question per line (request dim partitioned tt_on vl_on bf_on ev_on),
// stdout the verdict of each: the error code, a tab, the message tail.
#include <cstdio>

#include "sns_policy.h"

int main() {
    int req, dim, part, tt, vl, bf, ev;
    std::printf("%d\n", (int)sns::policy::REQ_COUNT);
    while (std::scanf("%d %d %d %d %d %d %d", &req, &dim, &part, &tt, &vl, &bf, &ev) == 7) {
        const sns::policy::FormVerdict v = sns::policy::check_form_request(
            (sns::policy::FormRequest)req, {dim, part != 0, tt != 0, vl != 0, bf != 0, ev != 0});
        std::printf("%d\t%s\n", v.error, v.tail);
    }
    return 0;
}
