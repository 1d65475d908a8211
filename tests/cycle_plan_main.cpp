// The cycle's plan (csrc/sns_policy.h: policy::plan_cycle) on its own, for tests/test_host.py: argv[1] holds the raw sns_options,
// stdin the Facts (see test_host.py::plan_of), stdout one line per level and one line of handle-wide fields.
#include <cstdio>
#include <vector>

#include "sns_policy.h"

int main(int argc, char** argv) {
    sns_options o;
    FILE* fo = argc > 1 ? std::fopen(argv[1], "rb") : nullptr;
    if (!fo || std::fread(&o, sizeof(o), 1, fo) != 1) return 2;
    std::fclose(fo);
    sns::policy::Facts f;
    int nl = 0, windows = 0, last = 0, fits = 0, team_overlap = 0;
    long long l1 = 0;
    if (std::scanf("%d %d %d %lld %d %d %d %d", &f.nranks, &f.rep_level, &nl, &l1, &windows, &last, &fits, &team_overlap) != 8) return 3;
    f.rows_global_l1 = l1;
    f.windows = windows != 0;
    f.last = (sns::policy::CoarsestKind)last;
    f.rep_gather_fits = fits != 0;
    f.team_overlap = team_overlap != 0;
    auto read64 = [&](std::vector<int64_t>& v) { for (int l = 0; l < nl; ++l) { long long x = 0; if (std::scanf("%lld", &x) != 1) return false; v.push_back(x); } return true; };
    auto read8 = [&](std::vector<uint8_t>& v) { for (int l = 0; l < nl; ++l) { int x = 0; if (std::scanf("%d", &x) != 1) return false; v.push_back((uint8_t)x); } return true; };
    if (!read64(f.rows) || !read64(f.max_owned) || !read8(f.has_blocks) || !read8(f.has_ap) || !read8(f.has_ap_rep) || !read8(f.win_capable)) return 4;
    const sns::policy::CyclePlan p = sns::policy::plan_cycle(o, f);
    for (const auto& q : p.level)
        std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", q.kind, q.cycled, q.blocks, q.nu, q.pre, q.post, q.exact, q.windows,
                    q.sx, q.px, q.fused_post, q.fused_restrict, q.fuses_next_first, q.lp_fmt, q.start_odd);
    std::printf("%d %d %d %d %d\n", p.fine_windows, p.fine_tails_unused, p.rep_gather_first, p.graph_level, p.fuse_puts);
    return 0;
}
