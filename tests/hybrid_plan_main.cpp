// The fine level's row of the cycle's plan (csrc/sns_policy.h: policy::plan_cycle) with the hybrid aggregation's fact, for
// tests/test_host_hybrid_aggregation.py: argv[1] holds the raw sns_options, argv[2] nranks, argv[3] whether level 0 was re-matched
// (-1: the fact left at its default), argv[4..] the global rows per level; stdout one line per level (kind blocks pre post).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sns_policy.h"

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    sns_options o;
    FILE* fo = std::fopen(argv[1], "rb");
    if (!fo || std::fread(&o, sizeof(o), 1, fo) != 1) return 2;
    std::fclose(fo);
    sns::policy::Facts f;
    f.nranks = std::atoi(argv[2]);
    const int rematched = std::atoi(argv[3]);
    if (rematched >= 0) f.fine_rematched = rematched != 0;
    for (int a = 4; a < argc; ++a) f.rows.push_back(std::atoll(argv[a]));
    const size_t nl = f.rows.size();
    f.rows_global_l1 = nl > 1 ? f.rows[1] : 0;
    f.max_owned.assign(nl, 0);
    for (size_t l = 0; l < nl; ++l) f.max_owned[l] = (f.rows[l] + f.nranks - 1) / f.nranks;
    f.has_blocks.assign(nl, 1);
    f.has_blocks[nl - 1] = 0;
    f.has_ap.assign(nl, 1);
    f.has_ap[nl - 1] = 0;
    f.has_ap_rep.assign(nl, 0);
    f.win_capable.assign(nl, 0);
    f.last = sns::policy::coarsest_kind(o, f.rows[nl - 1]);
    const sns::policy::CyclePlan p = sns::policy::plan_cycle(o, f);
    for (const auto& q : p.level) std::printf("%d %d %d %d\n", q.kind, q.blocks, q.pre, q.post);
    return 0;
}
