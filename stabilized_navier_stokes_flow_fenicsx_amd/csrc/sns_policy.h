// The policy of the AMG hierarchy in ONE place (round 5): every size threshold and every sweep schedule --
// which levels take aggregate blocks, how many sweeps a level runs before and after its coarse-grid correction, where the
// hierarchy ends and how its last level is solved, which level a partitioned run replicates from, which levels run as a
// hipGraph.  Pure host code over (options, a few global counts): no HIP, no handle, so that the table can be unit-tested on the
// CPU (sns_host_cycle_policy, tests/test_host.py) and every rank of a partitioned run answers alike by construction.
// The handle-side predicates of csrc/sns_cycle.hip / sns_setup.hip gather the facts and ask here; the numbers live nowhere else.
// In the same idiom, at the end: the route of an assembly (plan_assembly, tests/assembly_plan_main.cpp), what a handle's state
// allows of every entry point that can refuse (HandleFacts and the one table RULES, tests/request_main.cpp), which operator is
// a new one (OperatorKey, tests/operator_key_main.cpp), the damping of a
// level's smoother (LevelDamping, tests/damping_policy_main.cpp), what a kernel of a solve hands to a later one (Handoff,
// tests/handoff_main.cpp), what a solve and a set-up may leave out of their fixed cost (plan_step, tests/step_plan_main.cpp), when
// the Krylov and Newton loops stop and which step the line search tries next (LineSearch, tests/newton_policy_main.cpp), the
// Givens least-squares problem of the two FGMRES loops (GivensLsq, tests/givens_lsq_main.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <type_traits>
#include <vector>

#include "sns.h"

namespace sns {
namespace policy {

// ---- hierarchy shape -----------------------------------------------------------------------------------------------------------
// rows at or below which a level >= 1 ends the hierarchy (it is solved directly): the dense level of round 4 (amg_dense_rows,
// capped at 4096 rows = a 16 k x 16 k inverse) or the one-workgroup inverse of rounds 1-3 (amg_coarse_size)
inline int coarsest_rows(const sns_options& o) { return std::max(o.amg_coarse_size, std::min(o.amg_dense_rows, 4096)); }
// the one-workgroup inverse with partial pivoting takes at most this many nodes
inline int small_inverse_rows(const sns_options& o) { return std::max(o.amg_coarse_size, 40); }
enum CoarsestKind { COARSEST_SMALL_INVERSE = 0, COARSEST_BLOCKED_INVERSE = 1, COARSEST_SWEEPS = 2 };
inline CoarsestKind coarsest_kind(const sns_options& o, int64_t rows) {
    if (rows <= small_inverse_rows(o)) return COARSEST_SMALL_INVERSE;
    if (rows <= o.amg_dense_rows) return COARSEST_BLOCKED_INVERSE;
    return COARSEST_SWEEPS;                              // amg_max_levels reached with a large last level: 1 + 8 nodal sweeps
}
// a partitioned run replicates the hierarchy from the first level >= 1 with at most amg_replicate_rows GLOBAL rows (and more
// than the small inverse takes; `fits`: the replicated level fits the scratch vectors of every rank's fine level)
inline bool replicate_from(const sns_options& o, int level, int64_t rows_global, bool fits) {
    return level >= 1 && o.amg_replicate_rows > 0 && rows_global <= (int64_t)o.amg_replicate_rows &&
           rows_global > (int64_t)small_inverse_rows(o) && fits;
}
// without a replicated tail the distributed coarsest level is all-gathered into one dense system of at most this many dofs
constexpr int DISTRIBUTED_DENSE_MAX_DOFS = 640;
// first level (>= 1) with at most this many rows: it and everything below are launch-bound and run as ONE hipGraph
// (10 M tets: level 2, 36 k rows; level 1 has 218 k rows = 46 us per sweep)
constexpr int GRAPH_MAX_ROWS = 150000;

// ---- operator-strength aggregation of the fine level (amg_aggregation = 1, 2, 3) --------------------------------------------------
// s_ij = || D_i^-1/2 A_ij D_j^-1/2 ||_F of the first assembled operator (k_strength), symmetrised s_ij <- max(s_ij, s_ji); the
// edge (i, j) is strong when s_ij >= STRENGTH_THETA x the strongest coupling of i or of j.  The aggregates come from pairwise
// heavy-edge matching of the strong graph (1: sns_host.cpp aggregate_strength; 2: the same map on the device, sns_aggregate.hip).
constexpr double STRENGTH_THETA = 0.25;
// the aggregates must fit the 32 x 32 smoother blocks of csrc/sns_block.hip
constexpr int STRENGTH_MAX_AGG = 8;
// the hybrid (amg_aggregation = 3): an owned node is marked when its strongest coupling to another geometric aggregate exceeds
// HYBRID_KAPPA x the larger of its strongest coupling inside its own and its row's mean coupling (the mean alone for a singleton);
// the geometric aggregates holding a marked node are dissolved and re-matched by strength (sns_aggregate.hip).  The smallest
// candidate of {1.5, 2, 3, 4, 8} that marks no node on the structured and the body-centred Delaunay channels
// (profiles/proto_hybrid_aggregation.txt)
constexpr double HYBRID_KAPPA = 4.0;
// ... and when more than HYBRID_PHI of a handle's owned rows are marked, every aggregate is dissolved (the map of amg_aggregation
// = 2): re-matching only the dissolved aggregates of the jittered-cubic channel (2 % of its rows marked) needs more iterations
// than the geometric map (profiles/proto_hybrid_aggregation.txt, profiles/hybrid_aggregation.txt)
constexpr double HYBRID_PHI = 0.01;

// ---- smoother kind ---------------------------------------------------------------------------------------------------------------
// aggregate blocks on the FINE level: always with amg_block_smooth = 2 and with the aggregation by operator strength
// (amg_aggregation = 1 or 2: its aggregates are made to hold a sliver's nodes in one block -- with nodal blocks they gain nothing,
// scripts/proto_strength_aggregation.py); with the hybrid (3) when it re-matched level 0 on some rank (`rematched`, agreed over
// the ranks) -- otherwise its map is the geometric one and it smooths as 0 does; with 1 on a partitioned handle whose share of the
// fine level is at most amg_block_fine_rows rows per rank -- the latency-bound strong split
inline bool fine_blocks(const sns_options& o, int nranks, int64_t rows_global_fine, bool rematched = false) {
    if (o.amg_block_smooth >= 2 || o.amg_aggregation == 1 || o.amg_aggregation == 2) return true;
    if (o.amg_aggregation == 3 && rematched) return true;
    if (o.amg_block_smooth < 1 || o.amg_block_fine_rows <= 0) return false;
    if (nranks < 2 || rows_global_fine <= 0) return false;
    return rows_global_fine <= (int64_t)o.amg_block_fine_rows * nranks;
}
// ... on a level in general: the options allow it and the level is small enough per rank (amg_block_max_rows, 0 = no limit;
// `sharing` = ranks the level's rows are spread over: 1 for a serial or replicated level)
inline bool blocks_allowed(const sns_options& o, int64_t rows_global, int sharing) {
    if (o.amg_block_smooth <= 0 || o.amg_f32_matrix == 0 || o.pc_type != SNS_PC_AMG) return false;
    return !(o.amg_block_max_rows > 0 && rows_global > (int64_t)o.amg_block_max_rows * std::max(1, sharing));
}

// ---- sweep schedule -------------------------------------------------------------------------------------------------------------
// extra sweeps on level 2 and below for LARGE problems (amg_nu_scale_with_size): the plain-aggregation V-cycle loses convergence
// with its depth and on a big mesh those levels cost next to nothing (profiles/r3_deep_sweeps.txt: 81 M tets 73 / 82 -> 53 / 57
// iterations).  depth_equiv: the depth as rounds 1-3 counted it; small_aggregates: the first coarsening keeps more than one row in
// six, i.e. an unstructured mesh (config 4u: 71 -> 58 iterations per Newton step with the first tier).
struct ExtraSweeps { int l2 = 0, deep = 0; };
inline ExtraSweeps extra_sweeps(const sns_options& o, int64_t rows_global_fine, int depth_equiv, bool small_aggregates) {
    ExtraSweeps e;
    if (!o.amg_nu_scale_with_size) return e;
    if (rows_global_fine >= 20000000) { e.l2 = 6; e.deep = 10; }               // 192 M tets: 63 / 71 -> 55 / 66, -10 % time
    else if (rows_global_fine >= 8000000) { e.l2 = 4; e.deep = 6; }
    else if (rows_global_fine >= 2500000 || (depth_equiv >= 7 && small_aggregates)) { e.l2 = 2; e.deep = 2; }
    return e;
}
// depth of the hierarchy as rounds 1-3 counted it: a hierarchy that ends in the dense level of round 4 would have gone on for
// ~log5(rows / amg_coarse_size) more levels
inline int depth_equivalent(const sns_options& o, int nlevels_smoothed_and_last, bool last_blocked_inverse, int64_t last_rows) {
    int n = nlevels_smoothed_and_last;
    if (last_blocked_inverse && last_rows > o.amg_coarse_size)
        n += (int)std::ceil(std::log((double)last_rows / std::max(1, o.amg_coarse_size)) / std::log(5.0));
    return n;
}
// sweeps per half cycle of level `ll` (its number in the hierarchy as coarsened: the replicated copy is not a new level).
// Nodal blocks: the fine level is the expensive one (1 sweep); levels 1 and 2 are cheap and are where plain aggregation needs
// the smoothing (4 and 6); levels >= 3 are launch-bound (2).  Aggregate blocks: one sweep is worth about two nodal sweeps.
inline int half_cycle_sweeps(const sns_options& o, int ll, bool blocks, const ExtraSweeps& e) {
    if (blocks && ll >= 1) {
        if (ll >= 3) return std::max(1, o.amg_bnu_deep) + (e.deep + 1) / 2;
        if (ll == 2) return std::max(1, o.amg_bnu_l2) + (e.l2 + 1) / 2;
        return std::max(1, o.amg_bnu_l2);
    }
    int nu = std::max(1, o.amg_nu);
    if (ll >= 3 && o.amg_nu_deep > 0) nu = o.amg_nu_deep + e.deep;
    else if (ll == 2 && o.amg_nu_l2 > 0) nu = o.amg_nu_l2 + e.l2;
    else if (ll >= 1 && o.amg_nu_coarse > 0) nu = o.amg_nu_coarse;
    return nu;
}
// sweeps before / after the coarse-grid correction (the first pre-sweep is w S b from the zero guess).  Level 1: asymmetric --
// post-smoothing is the more valuable half under a piecewise-constant prolongation: 1 + amg_bnu_l1 with aggregate blocks,
// 1 + (nu + 2) with nodal blocks -- UNLESS its sweeps are rank-local (a partitioned level whose sweeps do not see the neighbours'
// iterate: nu + nu there, 1 + 6 costs 8-11 % more iterations).  A PARTITIONED level 1 with exact global sweeps (exact_partitioned)
// runs one post-sweep more, 1 + (amg_bnu_l1 + 1): its rows per rank are few, a sweep costs ~11 us, and the 4- / 8-way split of the
// 10 M-tet duct needs 91 / 89 instead of 98 / 95 iterations for it (profiles/r5_l1_schedules.txt; 4 + 4 rank-local: 91 / 97).
// amg_nu_l1_pre / _post fix the counts.
struct Sweeps { int pre = 1, post = 1; };
inline Sweeps pre_post_sweeps(const sns_options& o, int ll, bool blocks, bool rank_local_sweeps, int nu, bool exact_partitioned = false) {
    Sweeps s;
    s.pre = s.post = nu;
    if (ll == 1) {
        if (blocks) {
            if (!rank_local_sweeps) { s.pre = 1; s.post = std::max(1, o.amg_bnu_l1) + (exact_partitioned ? 1 : 0); }
        } else if (o.amg_nu_l1_pre == 0 && o.amg_nu_l1_post == 0 && !rank_local_sweeps && nu >= 2) {
            s.pre = 1;
            s.post = nu + 2;
        }
        if (o.amg_nu_l1_pre > 0) s.pre = o.amg_nu_l1_pre;
        if (o.amg_nu_l1_post > 0) s.post = o.amg_nu_l1_post;
    }
    return s;
}

// ---- the plan: what a hierarchy of the given structure runs ----------------------------------------------------------------------
// Facts: the hierarchy's structure as built.  rows[l]: GLOBAL rows of level l as held (a replicated level: its rows; its size is the
// level count); rep_level: first replicated level (0: none; the level before it is only the source of the copy and is not cycled);
// windows: the transport reads ghost entries from receive windows (peer / team); has_blocks[l]: the level's aggregates have at most
// 8 members (its smoother blocks exist); has_ap[l]: M = A P exists (the fused post-sweep); has_ap_rep[l]: M's columns in the ids of
// the replicated level below.  Agreed over the ranks by the caller: win_capable[l] -- every rank's plan of the level receives in
// order straight into its window; max_owned[l] -- the most owned rows any rank holds on the level.  last: how the last level is
// solved.  rep_gather_fits: a rank's piece of the replicated right-hand side fits the all-gather staging area.  fine_rematched:
// the hybrid aggregation (amg_aggregation = 3) re-matched level-0 nodes on some rank.  team_overlap / fuse_puts: the switches
// SNS_TEAM_OVERLAP / SNS_NO_CARRIED_PUT (not options).
struct Facts {
    int nranks = 1, rep_level = 0;
    std::vector<int64_t> rows, max_owned;
    std::vector<uint8_t> has_blocks, has_ap, has_ap_rep, win_capable;
    int64_t rows_global_l1 = 0;
    bool windows = false, rep_gather_fits = false, fine_rematched = false;
    CoarsestKind last = COARSEST_SWEEPS;
    bool team_overlap = false, fuse_puts = true;
};

// One level's row of the plan.  kind: SNS_LEVEL_* of include/sns.h; cycled = 0: only the source of the replicated copy; blocks: the
// aggregate blocks smooth it; nu: sweeps per half cycle (half_cycle_sweeps); pre / post: sweeps before / after the coarse-grid correction (the
// first pre-sweep is w S b from the zero guess); exact: exact global sweeps over the windows (amg_exact_sweeps); windows: the window
// form of the cycle (vcycle_windows); sx: every sweep exchanges ghost values (amg_sweep_exchange_rows); px: one exchange after the
// coarse-grid correction makes the single post-sweep the exact global one (amg_post_exchange); fused_post: coarse-grid correction +
// first post-sweep over M = A P; fused_restrict: residual + restriction (+ next first sweep) in one launch (amg_fuse_restrict);
// fuses_next_first: the restriction from this level also does the next level's first sweep; lp_fmt: the low-precision matrix copy
// the smoother reads (0 none, 1 fp32, 2 fp16); start_odd: (pre - 1 + post) odd -- the cycle starts in the ping-pong buffer, so that
// the result lands in x.
struct LevelPlan {
    int kind = SNS_LEVEL_NODAL_BLOCKS, cycled = 1, blocks = 0, nu = 0, pre = 0, post = 0;
    int exact = 0, windows = 0, sx = 0, px = 0, fused_post = 0, fused_restrict = 0, fuses_next_first = 0, lp_fmt = 0, start_odd = 0;
    bool ghost_sweeps() const { return sx || px || exact; }      // the level's sweeps see the neighbours' values
    bool operator==(const LevelPlan& o) const {
        return kind == o.kind && cycled == o.cycled && blocks == o.blocks && nu == o.nu && pre == o.pre && post == o.post &&
               exact == o.exact && windows == o.windows && sx == o.sx && px == o.px && fused_post == o.fused_post &&
               fused_restrict == o.fused_restrict && fuses_next_first == o.fuses_next_first && lp_fmt == o.lp_fmt &&
               start_odd == o.start_odd;
    }
};
// fine_windows: the level-0 passes (operator applications included) read their ghost entries straight from the receive window;
// fine_tails_unused: the partitioned fine level's cycle never reads a ghost tail as zero (no internal buffer, no copy);
// rep_gather_first: both halves of the replicated tail's all-gather ride in solver kernels; graph_level: first level of the hipGraph
// (0: none); fuse_puts: kernels carry the put of the vector they produce
struct CyclePlan {
    std::vector<LevelPlan> level;
    int fine_windows = 0, fine_tails_unused = 0, rep_gather_first = 0, graph_level = 0, fuse_puts = 0;
};

inline CyclePlan plan_cycle(const sns_options& o, const Facts& f) {
    CyclePlan p;
    const int nl = (int)f.rows.size();
    if (nl == 0) return p;
    p.level.resize((size_t)nl);
    const int last = nl - 1, R = f.rep_level;
    const bool part = f.nranks > 1;
    const bool amg = o.pc_type == SNS_PC_AMG;
    const bool win = part && f.windows && o.halo_windows && !f.team_overlap;
    auto partitioned = [&](int l) { return part && !(R > 0 && l >= R); };
    auto fact = [](const std::vector<uint8_t>& v, int l) { return l >= 0 && (size_t)l < v.size() && v[(size_t)l] != 0; };
    const bool small_agg = f.rows_global_l1 > 0 && (double)f.rows[0] < 6.0 * (double)f.rows_global_l1;
    const ExtraSweeps e = extra_sweeps(o, f.rows[0], depth_equivalent(o, nl - (R > 0 ? 1 : 0), f.last == COARSEST_BLOCKED_INVERSE && nl > 1,
                                                                      f.rows[last]), small_agg);
    for (int l = 0; l < nl; ++l) {                          // what a level is and how it is smoothed
        LevelPlan& q = p.level[(size_t)l];
        const bool solved_last = l == last && nl > 1;
        const bool rep_src = R > 0 && l == R - 1;
        const int ll = (R > 0 && l >= R) ? l - 1 : l;      // the replicated copy is not a new level
        q.cycled = rep_src ? 0 : 1;
        q.blocks = !solved_last && !rep_src && fact(f.has_blocks, l) && (l > 0 || fine_blocks(o, f.nranks, f.rows[0], f.fine_rematched)) &&
                   blocks_allowed(o, f.rows[(size_t)l], partitioned(l) ? f.nranks : 1);
        if (solved_last) {
            q.kind = f.last == COARSEST_BLOCKED_INVERSE ? SNS_LEVEL_DIRECT_BLOCKED : f.last == COARSEST_SMALL_INVERSE ? SNS_LEVEL_DIRECT
                                                                                                                      : SNS_LEVEL_SWEEPS_ONLY;
            if (part && R == 0 && f.last != COARSEST_SWEEPS) q.kind = SNS_LEVEL_DIRECT;     // the all-gathered dense system
        } else {
            q.kind = q.blocks ? SNS_LEVEL_AGGREGATE_BLOCKS : SNS_LEVEL_NODAL_BLOCKS;
        }
        const bool direct = q.kind == SNS_LEVEL_DIRECT || q.kind == SNS_LEVEL_DIRECT_BLOCKED;
        q.lp_fmt = (amg && !direct && !rep_src) ? (o.amg_f32_matrix == 2 ? 2 : o.amg_f32_matrix ? 1 : 0) : 0;
        q.nu = half_cycle_sweeps(o, ll, q.blocks, e);
        // (the most owned rows of any rank: a level's ranks all fall on the same side of the threshold)
        q.sx = partitioned(l) && o.amg_sweep_exchange_rows > 0 && (size_t)l < f.max_owned.size() &&
               f.max_owned[(size_t)l] <= (int64_t)o.amg_sweep_exchange_rows;
        q.px = partitioned(l) && !q.sx && o.amg_post_exchange && q.nu == 1 && (l == 0 || !q.blocks);
    }
    for (int l = 0; l < nl; ++l) {                          // exact global sweeps: the window form of a level >= 1
        LevelPlan& q = p.level[(size_t)l];
        const bool rep_src_next = R > 0 && l + 1 == R - 1;  // (xc straight from the replicated solution)
        q.exact = win && o.amg_exact_sweeps && amg && l >= 1 && l + 1 < nl && !(R > 0 && l >= R - 1) && !q.sx && q.blocks &&
                  fact(f.has_ap, l) && o.amg_fused_post && o.amg_fuse_restrict != 0 && fact(f.win_capable, l) &&
                  (rep_src_next ? fact(f.has_ap_rep, l) : fact(f.win_capable, l + 1));
    }
    for (int l = 0; l < nl; ++l) {                          // the sweep counts and what is fused into what
        LevelPlan& q = p.level[(size_t)l];
        const int ll = (R > 0 && l >= R) ? l - 1 : l;
        if (l + 1 < nl || nl == 1) {
            // rank-local sweeps: any level of a partitioned handle (the rule of rounds 2-4) unless its sweeps are the exact global ones
            const Sweeps s = pre_post_sweeps(o, ll, q.blocks, part && !q.exact, q.nu, q.exact != 0);
            q.pre = s.pre;
            q.post = s.post;
        }
        q.start_odd = (q.pre + q.post > 0) && ((q.pre - 1 + q.post) & 1);
        q.fused_post = l + 1 < nl && o.amg_fused_post && fact(f.has_ap, l) && q.lp_fmt != 0 && q.post >= 1 && !q.sx &&
                       (!partitioned(l) || (l == 0 && q.px && q.nu == 1));
        q.fused_restrict = (l >= 1 || (o.amg_fuse_restrict >= 2 && !partitioned(l))) && o.amg_fuse_restrict != 0 && q.lp_fmt != 0;
        // the next level's first sweep is the plain rank-local w S bc of a smoothed level: not the dense coarsest level, not the
        // level whose cycle is the all-gather into the replicated tail (nor that tail's first level), not a level whose sweeps
        // exchange ghost values
        const int c = l + 1;
        if (c + 1 < nl && !(R > 0 && (c == R - 1 || l == R - 1))) {
            const LevelPlan& C = p.level[(size_t)c];
            q.fuses_next_first = !C.sx && (C.blocks || C.lp_fmt != 0);
        }
    }
    p.fine_tails_unused = nl >= 2 && partitioned(0) && R != 1 && p.level[0].fused_post;
    p.fine_windows = win && fact(f.win_capable, 0);
    p.level[0].windows = p.fine_windows && p.fine_tails_unused && fact(f.win_capable, 1);
    for (int l = 1; l < nl; ++l) p.level[(size_t)l].windows = p.level[(size_t)l].exact;
    p.rep_gather_first = win && R >= 3 && p.level[(size_t)R - 2].exact && p.level[(size_t)R].blocks && f.rep_gather_fits;
    if (part) {
        p.graph_level = R;                                  // only the replicated tail is free of exchanges
    } else {
        for (int l = 1; l < nl && !p.graph_level; ++l)
            if (f.rows[(size_t)l] <= (int64_t)GRAPH_MAX_ROWS) p.graph_level = l;
    }
    p.fuse_puts = f.fuse_puts;
    return p;
}

// ---- cycle hand-offs (csrc/sns_cycle.hip, sns_krylov.hip; the contract is in DESIGN.md, "Cycle hand-offs") --------------------------
// Who does level l's first sweep z = w S b: the level's own cycle, the restriction of the level above (its plan's
// fuses_next_first), the gather into the replicated tail (rep_gather_first), or nobody -- the last level is solved, the source of
// the replicated copy is not cycled.  rep_level: first replicated level (0: none).  That the Krylov kernel in front of pc_apply
// did the FINE level's is a run-time fact of the rank (Handoff::krylov_first), asked where the answer here is the level itself.
enum FirstSweepOwner { FIRST_SWEEP_NOBODY = 0, FIRST_SWEEP_LEVEL = 1, FIRST_SWEEP_RESTRICTION = 2, FIRST_SWEEP_GATHER = 3 };
inline FirstSweepOwner first_sweep_owner(const CyclePlan& p, int rep_level, int l) {
    if (l < 0 || l + 1 >= (int)p.level.size() || (rep_level > 0 && l == rep_level - 1)) return FIRST_SWEEP_NOBODY;
    if (l > 0 && p.level[(size_t)l - 1].fuses_next_first) return FIRST_SWEEP_RESTRICTION;
    if (rep_level > 0 && l == rep_level && p.rep_gather_first) return FIRST_SWEEP_GATHER;
    return FIRST_SWEEP_LEVEL;
}
// the buffer a level's cycle starts in: after pre - 1 + post ping-pong swaps the result sits in x
template <class T>
inline T* cycle_start(const LevelPlan& q, T* x, T* pong) { return q.start_odd ? pong : x; }

// What one kernel of a solve hands to a later one across function boundaries, and the rule of the carried puts.  A kernel that
// produces vector v of level l may carry the put half of v's halo exchange (PutDst): that advances the plan's round and flips the
// parity of its receive window, so the next exchange of exactly v on that plan must wait for the carried put (comm_put_carried)
// and must not put again.  Hence: a put is carried only where a consumer is promised; every carried put is taken by exactly one
// exchange of that vector on that level; nothing but the promised result of pc_apply outlives the call.  Only the transitions
// below write the members; each returns whether it was legal, and an illegal one leaves the state as it was (begin_solve and
// end_pc_apply always leave it clean).  Vectors are names: compared, never dereferenced.
// A replayed hipGraph runs no host code.  On a partitioned handle the graph covers the replicated tail, which has no windows,
// and a serial handle has none at all: nothing here is moved by a level at or below plan.graph_level -- enter_level moves state
// for level 0 alone, and no put is ever recorded or asked for on a level without the window form.
struct Handoff {
    bool krylov_first = false;               // the Krylov kernel that wrote pc_apply's input did the fine level's first sweep
    bool op_promised = false;                // the caller of pc_apply promises an operator application of the result
    std::vector<const void*> put;            // put[l]: the vector whose put on level l's plan is carried and not yet taken

    int outstanding() const {                // first level with a carried put nobody has taken (-1: none)
        for (size_t l = 0; l < put.size(); ++l)
            if (put[l]) return (int)l;
        return -1;
    }
    // a solve begins (krylov): nothing may be outstanding; *level (optional): the level that was
    bool begin_solve(int* level = nullptr) {
        const int bad = outstanding();
        if (level) *level = bad;
        krylov_first = op_promised = false;
        put.clear();
        return bad < 0;
    }
    // the Krylov kernel did the fine level's first sweep into v, the buffer its cycle starts in (carried: with the put of v)
    bool krylov_did_first_sweep(const void* v, bool carried) {
        if (carried && !put_carried(0, v)) return false;
        krylov_first = true;
        return true;
    }
    void promise_operator() { op_promised = true; }
    // level l's cycle is entered: did the Krylov kernel do its first sweep?  (forgotten; the put that sweep carried stays
    // recorded against its vector until the first exchange of the cycle takes it)
    bool enter_level(int l) {
        if (l != 0) return false;
        const bool done = krylov_first;
        krylov_first = false;
        return done;
    }
    // a kernel of level l carried the put of the vector v it wrote: a sweep of l's cycle, the restriction above l that wrote
    // l's first sweep, the last kernel of l's cycle (v its result, leaving the level).  One at a time per level
    bool put_carried(int l, const void* v) {
        if (l < 0 || !v) return false;
        if ((size_t)l >= put.size()) put.resize((size_t)l + 1, nullptr);
        if (put[(size_t)l]) return false;
        put[(size_t)l] = v;
        return true;
    }
    // THE consumption point, asked by every exchange over a window: is the put of v on level l's plan done already?  *done is
    // true at most once per carried put.  Illegal while the put of another vector of the level is outstanding
    bool take_put(int l, const void* v, bool* done) {
        *done = false;
        if (l < 0 || (size_t)l >= put.size() || !put[(size_t)l]) return l >= 0;
        if (put[(size_t)l] != v) return false;
        put[(size_t)l] = nullptr;
        *done = true;
        return true;
    }
    // pc_apply(., z) ends: keeps the carried put of the fine level's result, and only where that is z, the operator application
    // was promised and the call succeeded.  Anything else outstanding after a successful call is illegal (*level: where);
    // after a failed one it is dropped -- a solve that ended in an error must not leak a hand-off
    bool end_pc_apply(bool ok, const void* z, int* level = nullptr) {
        const void* keep = (ok && op_promised && !put.empty() && put[0] == z) ? z : nullptr;
        if (keep) put[0] = nullptr;
        const int bad = ok ? outstanding() : -1;
        if (level) *level = bad;
        krylov_first = op_promised = false;
        put.clear();
        if (keep) put.push_back(keep);
        return bad < 0;
    }
};

// ---- the route of an assembly (csrc/sns_assemble.hip; the table is in DESIGN.md) ------------------------------------------------------
// Facts: the call (form; state, matrix, residual asked for) and the handle (dim, opt.assembly_fused, a perturbed form variant, a
// mesh with cells).  Whether w violates its Dirichlet data is learnt on the device: where bc_check says so the driver counts the
// violations and asks again with the answer (`violated` is not read otherwise).
struct AssemblyFacts {
    int dim = 3, form = SNS_FORM_NS;
    bool has_w = false, want_matrix = false, has_F = false, fused = false, variant = false, cells = false;
};
enum AssemblyRoute { ROUTE_FUSED_STOKES = 0, ROUTE_FUSED_NS = 1, ROUTE_STAGED = 2, ROUTE_STOKES_2D = 3, ROUTE_NS_2D = 4 };
// element pass: none, the staged element kernel (16 cells per workgroup), the one-lane-per-cell residual kernel; state: w as
// given, the Dirichlet data extended by zero, w with the data imposed
enum ElementKernel { ELEMENT_NONE = 0, ELEMENT_STAGED = 1, ELEMENT_RESIDUAL = 2 };
enum AssemblyState { STATE_W = 0, STATE_GEXT = 1, STATE_SNAPPED = 2 };
// error != SNS_OK: refused with `message`.  The launches in the driver's order: the owner-lane passes offdiag / diag (diag writes
// F too), the element pass (store_K: with matrices; Fe_out: with residuals), the two gathers, the lifting pass, the Dirichlet
// rows of a 2-D Stokes residual; matrix: the fine operator is rewritten.
struct AssemblyPlan {
    int error = SNS_OK;
    const char* message = "";
    AssemblyRoute route = ROUTE_STAGED;
    AssemblyState state = STATE_W;
    ElementKernel element = ELEMENT_NONE;
    bool bc_check = false, offdiag = false, diag = false, store_K = false, Fe_out = false, gather_matrix = false,
         gather_residual = false, lift = false, bc_residual = false, matrix = false;
};

inline AssemblyPlan plan_assembly(const AssemblyFacts& f, bool violated = true) {
    AssemblyPlan p;
    auto refuse = [&](const char* why) { p.error = SNS_E_ARG; p.message = why; return p; };
    if (f.form != SNS_FORM_STOKES && f.form != SNS_FORM_NS) return refuse("bad form");
    const bool ns = f.form == SNS_FORM_NS;
    if (ns && !f.has_w) return refuse("NS form needs a state vector");
    p.matrix = f.want_matrix;
    if (f.dim == 2) {                                       // always the owner-lane passes; fused and variant do not apply
        if (!f.cells) return refuse("empty mesh");
        p.route = ns ? ROUTE_NS_2D : ROUTE_STOKES_2D;
        p.offdiag = f.want_matrix;
        p.diag = f.want_matrix || (!ns && f.has_F);
        if (ns) {
            p.bc_check = f.has_F;
            p.element = f.want_matrix ? ELEMENT_NONE : ELEMENT_RESIDUAL;
            p.Fe_out = p.gather_residual = !f.want_matrix;
            p.lift = f.has_F && violated;
        } else {
            p.state = f.has_w ? STATE_SNAPPED : STATE_GEXT;
            p.bc_residual = f.has_w && f.has_F;
        }
        return p;
    }
    // (a perturbed form exists in the staged element kernel only: Jacobian AND residual go through it; with try_fused && !has_F
    // the check's answer is not used: kept as it was)
    const bool try_fused = f.want_matrix && f.fused && ns && f.cells && !f.variant;
    p.bc_check = ns && f.cells && ((!f.want_matrix && f.has_F) || try_fused);
    const bool fast_residual = p.bc_check && !violated && !f.variant;
    if (try_fused || (!ns && !f.has_w && f.want_matrix && f.fused && f.cells)) {
        p.route = ns ? ROUTE_FUSED_NS : ROUTE_FUSED_STOKES;
        p.state = ns ? STATE_W : STATE_GEXT;
        p.offdiag = p.diag = true;
        p.lift = ns && f.has_F && !fast_residual;
        return p;
    }
    p.element = fast_residual ? ELEMENT_RESIDUAL : f.cells ? ELEMENT_STAGED : ELEMENT_NONE;
    p.store_K = p.element == ELEMENT_STAGED && f.want_matrix;
    p.Fe_out = p.element == ELEMENT_RESIDUAL || (p.element == ELEMENT_STAGED && f.has_F);
    p.gather_matrix = f.want_matrix;
    p.gather_residual = f.has_F;
    return p;
}

// ---- what a handle's state allows (asked by the entry points of csrc/sns_api.hip; the table is in DESIGN.md, "Form state") ----------
// Facts: the handle (dim, a communicator attached), the switches of the 3-D NS form that are on -- time term, viscosity law, body
// force, viscosity field --, whether boundary facets are set, and a traction / a backflow coefficient set on facets that exist
// ("a boundary flow term is on" is either of the two: HAS_BOUNDARY_FLOW).  Built from a handle in one place (facts_of,
// csrc/sns_ctx.h) for every family of requests; a family reads the facts its rows name and no other.
struct HandleFacts {
    int dim = 3;
    bool partitioned = false, tt_on = false, vl_on = false, bf_on = false, ev_on = false;
    bool has_facets = false, traction_on = false, backflow_on = false;
};
enum FactBit {
    IS_NOT_3D = 1, IS_PARTITIONED = 2, HAS_TIME_TERM = 4, HAS_LAW = 8, HAS_FORCE = 16, HAS_FIELD = 32, NO_FACETS = 64, HAS_TRACTION = 128,
    HAS_BACKFLOW = 256, HAS_BOUNDARY_FLOW = HAS_TRACTION | HAS_BACKFLOW
};
// The families: the setters and passes of the 3-D NS form; the three setters of the facet terms (csrc/sns_boundary.hip); the
// stability analysis (csrc/sns_stability.hip) -- SREQ_COUNT is the number of right-hand kinds, SREQ_KINDS counts all: the
// left-hand kinds (sns_mass_apply_transpose, sns_stability_arnoldi_left) follow the right-hand ones and are refused exactly as
// those are --; the Hessian pass (sns_jacobian_state_gradient, csrc/sns_hessian.hip), one request; the raw Jacobian
// (sns_raw_jacobian_apply) and the Dirichlet values of a live handle (sns_set_dirichlet_values), two requests; the resolvent
// analysis (csrc/sns_resolvent.hip), two requests: the passes that touch no form (sns_energy_apply, sns_lumped_volumes) and the
// process (sns_resolvent_lanczos).
enum Family { FAMILY_FORM = 0, FAMILY_BOUNDARY, FAMILY_STABILITY, FAMILY_STATE_GRADIENT, FAMILY_RAW_JACOBIAN, FAMILY_RESOLVENT };
enum FormRequest {
    REQ_SET_TIME_TERM = 0, REQ_CLEAR_TIME_TERM, REQ_SET_CARREAU, REQ_SET_NEWTONIAN, REQ_SET_FIELD /* set or clear: force, viscosity, mixture */,
    REQ_TIME_STEP, REQ_SHAPE_GRADIENT, REQ_RECOVER_GRADIENT, REQ_ERROR_INDICATOR, REQ_SCALAR /* system or solve */,
    REQ_ELEMENT_VISCOSITY /* the query */, REQ_FORM_VARIANT, REQ_COUNT
};
enum BoundaryRequest { BREQ_SET_FACETS = 0, BREQ_SET_FLOW, BREQ_SET_SCALAR, BREQ_COUNT };
enum StabilityRequest { SREQ_MASS_APPLY = 0, SREQ_ARNOLDI, SREQ_COUNT, SREQ_MASS_APPLY_TRANSPOSE = SREQ_COUNT, SREQ_ARNOLDI_LEFT, SREQ_KINDS };
constexpr int GREQ_STATE_GRADIENT = 0;
enum RawJacobianRequest { JREQ_APPLY = 0, JREQ_SET_DIRICHLET, JREQ_COUNT };
enum ResolventRequest { RREQ_ENERGY = 0 /* the energy pass, the lumped volumes */, RREQ_LANCZOS, RREQ_COUNT };
// error != SNS_OK: refused; the entry point's message is its name, ": " and `tail`
struct Verdict {
    int error = SNS_OK;
    const char* tail = "";
};
// A request is refused by its first row with one of `any_of` true; in every family the SNS_E_ARG rows (the dimension) stand
// before the SNS_E_STATE rows.  Asymmetries kept as they grew: a Newtonian law is refused under a time term though
// it sets nothing, and allowed under a force or a field; CLEARING a field is refused while a law is set; the shape gradient
// and the two recovery requests never ask for the dimension; setting or clearing facets never needs facets; the mass pass
// ignores a time term (B is taken at theta = 0 and u_t = 0 whatever the handle's history) while the Arnoldi process sets its
// own; the Hessian pass allows a viscosity field (the viscous term stays linear in u) and a traction alone (constant in w), and
// refuses a body force (J then depends on f through dM/dw(w, -f): a second contraction that is not built) and a backflow
// coefficient (that term is quadratic in u; its Hessian is not built); the raw-Jacobian pass serves 2-D handles and every
// switch of the form (its blocks are the assembly's own) and refuses only a backflow coefficient, whose share of J0 lives in
// the boundary pass and is not built matrix-free; a traction alone is constant in w; the energy pass and the lumped volumes
// read the mesh and the mask alone, so a law or a time term does not refuse them, while the resolvent process is refused where
// the Arnoldi process is, in its words.
struct Rule {
    Family family;
    int request;
    unsigned any_of;
    int code;
    const char* tail;
};
constexpr Rule RULES[] = {
    {FAMILY_FORM, REQ_SET_TIME_TERM, IS_NOT_3D, SNS_E_ARG, "3-D handles only"},
    {FAMILY_FORM, REQ_SET_TIME_TERM, IS_PARTITIONED, SNS_E_STATE, "not with a communicator attached (partitioned time stepping is not built)"},
    {FAMILY_FORM, REQ_SET_TIME_TERM, HAS_LAW, SNS_E_STATE, "not with a viscosity law set (the transient form has no law)"},
    {FAMILY_FORM, REQ_CLEAR_TIME_TERM, IS_NOT_3D, SNS_E_ARG, "3-D handles only"},
    {FAMILY_FORM, REQ_CLEAR_TIME_TERM, IS_PARTITIONED, SNS_E_STATE, "not with a communicator attached (partitioned time stepping is not built)"},
    {FAMILY_FORM, REQ_SET_CARREAU, IS_NOT_3D, SNS_E_ARG, "3-D handles only"},
    {FAMILY_FORM, REQ_SET_CARREAU, IS_PARTITIONED, SNS_E_STATE, "not with a communicator attached (partitioned handles have no law)"},
    {FAMILY_FORM, REQ_SET_CARREAU, HAS_TIME_TERM, SNS_E_STATE, "not with a time term set (the transient form has no law)"},
    {FAMILY_FORM, REQ_SET_CARREAU, HAS_FORCE | HAS_FIELD, SNS_E_STATE, "not with a body force or a viscosity field set"},
    {FAMILY_FORM, REQ_SET_NEWTONIAN, IS_NOT_3D, SNS_E_ARG, "3-D handles only"},
    {FAMILY_FORM, REQ_SET_NEWTONIAN, IS_PARTITIONED, SNS_E_STATE, "not with a communicator attached (partitioned handles have no law)"},
    {FAMILY_FORM, REQ_SET_NEWTONIAN, HAS_TIME_TERM, SNS_E_STATE, "not with a time term set (the transient form has no law)"},
    {FAMILY_FORM, REQ_SET_FIELD, IS_NOT_3D, SNS_E_ARG, "3-D handles only"},
    {FAMILY_FORM, REQ_SET_FIELD, IS_PARTITIONED, SNS_E_STATE, "not with a communicator attached (partitioned handles have no external fields)"},
    {FAMILY_FORM, REQ_SET_FIELD, HAS_LAW, SNS_E_STATE, "not with a viscosity law set"},
    {FAMILY_FORM, REQ_TIME_STEP, IS_NOT_3D, SNS_E_ARG, "3-D handles only"},
    {FAMILY_FORM, REQ_TIME_STEP, IS_PARTITIONED, SNS_E_STATE, "not with a communicator attached (partitioned time stepping is not built)"},
    {FAMILY_FORM, REQ_TIME_STEP, HAS_LAW, SNS_E_STATE, "not with a viscosity law set (the transient form has no law)"},
    {FAMILY_FORM, REQ_SHAPE_GRADIENT, IS_PARTITIONED, SNS_E_STATE, "not with a communicator attached (partitioned shape gradients are not built)"},
    {FAMILY_FORM, REQ_SHAPE_GRADIENT, HAS_LAW, SNS_E_STATE, "not with a viscosity law set (the mesh derivative of nu_e is not built)"},
    {FAMILY_FORM, REQ_SHAPE_GRADIENT, HAS_FORCE | HAS_FIELD, SNS_E_STATE,
     "not with a body force or a viscosity field set (the mesh derivative is not built with them)"},
    {FAMILY_FORM, REQ_SHAPE_GRADIENT, HAS_BOUNDARY_FLOW, SNS_E_STATE,
     "not with a boundary traction or backflow term set (the mesh derivative of the facet terms is not built)"},
    {FAMILY_FORM, REQ_RECOVER_GRADIENT, IS_PARTITIONED, SNS_E_STATE, "not with a communicator attached (partitioned gradient recovery is not built)"},
    {FAMILY_FORM, REQ_ERROR_INDICATOR, IS_PARTITIONED, SNS_E_STATE,
     "not with a communicator attached (a partitioned indicator needs a halo exchange of G)"},
    {FAMILY_FORM, REQ_SCALAR, IS_NOT_3D, SNS_E_ARG, "3-D handles only"},
    {FAMILY_FORM, REQ_SCALAR, IS_PARTITIONED, SNS_E_STATE, "not with a communicator attached (partitioned scalar transport is not built)"},
    {FAMILY_FORM, REQ_ELEMENT_VISCOSITY, IS_NOT_3D, SNS_E_ARG, "3-D handles only"},
    {FAMILY_FORM, REQ_FORM_VARIANT, IS_NOT_3D, SNS_E_ARG, "3-D handles only"},

    {FAMILY_BOUNDARY, BREQ_SET_FACETS, IS_NOT_3D, SNS_E_ARG, "3-D handles only"},
    {FAMILY_BOUNDARY, BREQ_SET_FACETS, IS_PARTITIONED, SNS_E_STATE, "not with a communicator attached (partitioned boundary terms are not built)"},
    {FAMILY_BOUNDARY, BREQ_SET_FLOW, IS_NOT_3D, SNS_E_ARG, "3-D handles only"},
    {FAMILY_BOUNDARY, BREQ_SET_FLOW, IS_PARTITIONED, SNS_E_STATE, "not with a communicator attached (partitioned boundary terms are not built)"},
    {FAMILY_BOUNDARY, BREQ_SET_FLOW, NO_FACETS, SNS_E_STATE, "set the boundary facets first (sns_set_boundary_facets)"},
    {FAMILY_BOUNDARY, BREQ_SET_SCALAR, IS_NOT_3D, SNS_E_ARG, "3-D handles only"},
    {FAMILY_BOUNDARY, BREQ_SET_SCALAR, IS_PARTITIONED, SNS_E_STATE, "not with a communicator attached (partitioned boundary terms are not built)"},
    {FAMILY_BOUNDARY, BREQ_SET_SCALAR, NO_FACETS, SNS_E_STATE, "set the boundary facets first (sns_set_boundary_facets)"},

    {FAMILY_STABILITY, SREQ_MASS_APPLY, IS_NOT_3D, SNS_E_ARG, "3-D handles only"},
    {FAMILY_STABILITY, SREQ_MASS_APPLY, IS_PARTITIONED, SNS_E_STATE, "not with a communicator attached (partitioned stability analysis is not built)"},
    {FAMILY_STABILITY, SREQ_MASS_APPLY, HAS_LAW, SNS_E_STATE, "not with a viscosity law set (the mass operator of the law's form is not built)"},
    {FAMILY_STABILITY, SREQ_ARNOLDI, IS_NOT_3D, SNS_E_ARG, "3-D handles only"},
    {FAMILY_STABILITY, SREQ_ARNOLDI, IS_PARTITIONED, SNS_E_STATE, "not with a communicator attached (partitioned stability analysis is not built)"},
    {FAMILY_STABILITY, SREQ_ARNOLDI, HAS_LAW, SNS_E_STATE, "not with a viscosity law set (the mass operator of the law's form is not built)"},
    {FAMILY_STABILITY, SREQ_ARNOLDI, HAS_TIME_TERM, SNS_E_STATE, "not with a time term set (the analysis sets its own and clears it)"},

    {FAMILY_STATE_GRADIENT, GREQ_STATE_GRADIENT, IS_NOT_3D, SNS_E_ARG, "3-D handles only"},
    {FAMILY_STATE_GRADIENT, GREQ_STATE_GRADIENT, IS_PARTITIONED, SNS_E_STATE, "not with a communicator attached (the partitioned Hessian pass is not built)"},
    {FAMILY_STATE_GRADIENT, GREQ_STATE_GRADIENT, HAS_LAW, SNS_E_STATE, "not with a viscosity law set (the second derivative of nu_e is not built)"},
    {FAMILY_STATE_GRADIENT, GREQ_STATE_GRADIENT, HAS_TIME_TERM, SNS_E_STATE, "not with a time term set (the pass is taken on the steady form)"},
    {FAMILY_STATE_GRADIENT, GREQ_STATE_GRADIENT, HAS_FORCE, SNS_E_STATE,
     "not with a body force set (J depends on f through the stabilisation's weighting: that contraction is not built)"},
    {FAMILY_STATE_GRADIENT, GREQ_STATE_GRADIENT, HAS_BACKFLOW, SNS_E_STATE,
     "not with a backflow coefficient set (the Hessian of the backflow term is not built)"},

    {FAMILY_RAW_JACOBIAN, JREQ_APPLY, IS_PARTITIONED, SNS_E_STATE, "not with a communicator attached (the partitioned raw-Jacobian pass is not built)"},
    {FAMILY_RAW_JACOBIAN, JREQ_APPLY, HAS_BACKFLOW, SNS_E_STATE,
     "not with a backflow coefficient set (the backflow term's share of the raw Jacobian is not built)"},
    {FAMILY_RAW_JACOBIAN, JREQ_SET_DIRICHLET, IS_PARTITIONED, SNS_E_STATE,
     "not with a communicator attached (partitioned handles keep the Dirichlet values they were created with)"},

    {FAMILY_RESOLVENT, RREQ_ENERGY, IS_NOT_3D, SNS_E_ARG, "3-D handles only"},
    {FAMILY_RESOLVENT, RREQ_ENERGY, IS_PARTITIONED, SNS_E_STATE, "not with a communicator attached (partitioned stability analysis is not built)"},
    {FAMILY_RESOLVENT, RREQ_LANCZOS, IS_NOT_3D, SNS_E_ARG, "3-D handles only"},
    {FAMILY_RESOLVENT, RREQ_LANCZOS, IS_PARTITIONED, SNS_E_STATE, "not with a communicator attached (partitioned stability analysis is not built)"},
    {FAMILY_RESOLVENT, RREQ_LANCZOS, HAS_LAW, SNS_E_STATE, "not with a viscosity law set (the mass operator of the law's form is not built)"},
    {FAMILY_RESOLVENT, RREQ_LANCZOS, HAS_TIME_TERM, SNS_E_STATE, "not with a time term set (the analysis sets its own and clears it)"},
};

// The one lookup.  An entry point's own value checks stand between the family's SNS_E_ARG rows and its SNS_E_STATE rows:
// ROWS_ARG / ROWS_STATE ask for the verdict only where it is of that kind, so that a call with two things wrong reports what it
// always reported.
enum Rows { ROWS_ALL = 0, ROWS_ARG = SNS_E_ARG, ROWS_STATE = SNS_E_STATE };
inline Verdict check_request(Family family, int request, const HandleFacts& f, Rows rows = ROWS_ALL) {
    if (family == FAMILY_STABILITY && request >= SREQ_COUNT) request -= SREQ_COUNT;      // the left-hand kinds: the right-hand rows
    const unsigned facts = (f.dim != 3) * IS_NOT_3D | f.partitioned * IS_PARTITIONED | f.tt_on * HAS_TIME_TERM | f.vl_on * HAS_LAW |
                           f.bf_on * HAS_FORCE | f.ev_on * HAS_FIELD | (!f.has_facets) * NO_FACETS | f.traction_on * HAS_TRACTION |
                           f.backflow_on * HAS_BACKFLOW;
    for (const Rule& r : RULES)
        if (r.family == family && r.request == request && (facts & r.any_of))
            return (rows == ROWS_ALL || r.code == rows) ? Verdict{r.code, r.tail} : Verdict{};
    return {};
}
// ... and with the verdict of the call's own arguments in its place
inline Verdict check_request(Family family, int request, const HandleFacts& f, const Verdict& arguments) {
    Verdict v = check_request(family, request, f, ROWS_ARG);
    if (v.error == SNS_OK) v = arguments;
    if (v.error == SNS_OK) v = check_request(family, request, f, ROWS_STATE);
    return v;
}

// The arguments of the Arnoldi process: m in [2, 64], a finite shift >= 0 and breakdown_rel in (0, 1)
constexpr int STABILITY_M_MIN = 2, STABILITY_M_MAX = 64;
struct ArnoldiArgs {
    int m = STABILITY_M_MAX;
    double shift = 0.0, breakdown_rel = 1e-6;
};
inline Verdict check_arnoldi_args(const ArnoldiArgs& a) {
    if (a.m < STABILITY_M_MIN || a.m > STABILITY_M_MAX) return {SNS_E_ARG, "m must lie in [2, 64]"};
    if (!(a.shift >= 0.0) || !(a.shift <= 1.7976931348623157e308)) return {SNS_E_ARG, "the shift must be finite and >= 0"};
    if (!(a.breakdown_rel > 0.0) || !(a.breakdown_rel < 1.0)) return {SNS_E_ARG, "breakdown_rel must lie in (0, 1)"};
    return {};
}
// ... and of its continuation from column k (sns_stability_arnoldi_extend): those, then k in [1, m - 1].  The call is asked
// as SREQ_ARNOLDI / SREQ_ARNOLDI_LEFT: it is refused where they are, and has no kind of its own
inline Verdict check_arnoldi_extend_args(const ArnoldiArgs& a, int k) {
    const Verdict v = check_arnoldi_args(a);
    if (v.error != SNS_OK) return v;
    if (k < 1 || k > a.m - 1) return {SNS_E_ARG, "k must lie in [1, m - 1]"};
    return {};
}
// ... and of the process with a complex or negative shift s = shift_re + i shift_im on top of the assembled J + pc_shift B
// (sns_stability_arnoldi_shifted; k = 0 a fresh process, k >= 1 a continuation): m, k in [0, m - 1], finite shift parts, a
// finite pc_shift >= 0, breakdown_rel.  Asked as SREQ_ARNOLDI / SREQ_ARNOLDI_LEFT, like the continuation
struct ShiftedArgs {
    int m = STABILITY_M_MAX, k = 0;
    double shift_re = 0.0, shift_im = 0.0, pc_shift = 0.0, breakdown_rel = 1e-6;
};
inline Verdict check_shifted_args(const ShiftedArgs& a) {
    auto finite = [](double v) { return v - v == 0.0; };
    if (a.m < STABILITY_M_MIN || a.m > STABILITY_M_MAX) return {SNS_E_ARG, "m must lie in [2, 64]"};
    if (a.k < 0 || a.k > a.m - 1) return {SNS_E_ARG, "k must lie in [0, m - 1]"};
    if (!finite(a.shift_re) || !finite(a.shift_im)) return {SNS_E_ARG, "both parts of the shift must be finite"};
    if (!finite(a.pc_shift) || !(a.pc_shift >= 0.0)) return {SNS_E_ARG, "pc_shift must be finite and >= 0"};
    if (!(a.breakdown_rel > 0.0) || !(a.breakdown_rel < 1.0)) return {SNS_E_ARG, "breakdown_rel must lie in (0, 1)"};
    return {};
}
// ... and the coefficient of the complex operator A + c B (sns_shifted_apply, sns_shifted_solve: asked as SREQ_MASS_APPLY[_TRANSPOSE])
inline Verdict check_shifted_coefficient(double c_re, double c_im) {
    if (!(c_re - c_re == 0.0) || !(c_im - c_im == 0.0)) return {SNS_E_ARG, "both parts of c must be finite"};
    return {};
}
// ... and the coefficients of the Hessian pass
inline Verdict check_state_gradient_args(double c_jac, double c_mass) {
    if (!(c_jac - c_jac == 0.0) || !(c_mass - c_mass == 0.0)) return {SNS_E_ARG, "the coefficients must be finite"};
    return {};
}

// ... and the arguments of the raw-Jacobian pass: the NS form, distinct vectors, the reference's constants (the block code
// holds no others: a perturbed form variant is the call's own verdict, not a fact of the table)
struct RawJacobianArgs {
    int form = SNS_FORM_NS;
    bool aliased = false, variant = false;
};
inline Verdict check_raw_jacobian_args(const RawJacobianArgs& a) {
    if (a.form == SNS_FORM_STOKES) return {SNS_E_ARG, "the Stokes forms are not supported"};
    if (a.form != SNS_FORM_NS) return {SNS_E_ARG, "bad form"};
    if (a.aliased) return {SNS_E_ARG, "x and y must not be the same vector"};
    if (a.variant) return {SNS_E_STATE, "not with a perturbed form variant set (the pass holds the reference's constants only)"};
    return {};
}

// ... and the arguments of the resolvent family.  The energy pass: parts in {1, 2}, distinct vectors (the lumped volumes have
// no argument to check: the default).  The process: m in [2, 64], a finite omega, breakdown_rel in (0, 1), and a basis that is
// neither the state nor a weight vector
struct EnergyArgs {
    int parts = 1;
    bool aliased = false;
};
inline Verdict check_energy_args(const EnergyArgs& a) {
    if (a.parts != 1 && a.parts != 2) return {SNS_E_ARG, "parts must be 1 or 2"};
    if (a.aliased) return {SNS_E_ARG, "x and y must not be the same vector"};
    return {};
}
struct ResolventArgs {
    int m = STABILITY_M_MAX;
    double omega = 0.0, breakdown_rel = 1e-6;
    bool aliased = false;
};
inline Verdict check_resolvent_args(const ResolventArgs& a) {
    if (a.m < STABILITY_M_MIN || a.m > STABILITY_M_MAX) return {SNS_E_ARG, "m must lie in [2, 64]"};
    if (!(a.omega - a.omega == 0.0)) return {SNS_E_ARG, "omega must be finite"};
    if (!(a.breakdown_rel > 0.0) || !(a.breakdown_rel < 1.0)) return {SNS_E_ARG, "breakdown_rel must lie in (0, 1)"};
    if (a.aliased) return {SNS_E_ARG, "V must not be the state or a weight vector"};
    return {};
}

// The families as the host tests ask them (tests/request_main.cpp; the raw Jacobian's: tests/rawjac_request_main.cpp; the
// resolvent's: tests/resolvent_request_main.cpp)
inline Verdict check_form_request(FormRequest request, const HandleFacts& f) { return check_request(FAMILY_FORM, request, f); }
inline Verdict check_boundary_request(BoundaryRequest request, const HandleFacts& f) { return check_request(FAMILY_BOUNDARY, request, f); }
inline Verdict check_stability_request(StabilityRequest request, const HandleFacts& f, const ArnoldiArgs& a = {}) {
    const bool arnoldi = request == SREQ_ARNOLDI || request == SREQ_ARNOLDI_LEFT;
    return check_request(FAMILY_STABILITY, request, f, arnoldi ? check_arnoldi_args(a) : Verdict{});
}
// (tests/extend_request_main.cpp) request: SREQ_ARNOLDI or SREQ_ARNOLDI_LEFT
inline Verdict check_stability_extend_request(StabilityRequest request, const HandleFacts& f, const ArnoldiArgs& a, int k) {
    return check_request(FAMILY_STABILITY, request, f, check_arnoldi_extend_args(a, k));
}
// (tests/shifted_request_main.cpp) the process: SREQ_ARNOLDI or SREQ_ARNOLDI_LEFT; the operator: SREQ_MASS_APPLY[_TRANSPOSE]
inline Verdict check_stability_shifted_request(StabilityRequest request, const HandleFacts& f, const ShiftedArgs& a) {
    return check_request(FAMILY_STABILITY, request, f, check_shifted_args(a));
}
inline Verdict check_shifted_operator_request(StabilityRequest request, const HandleFacts& f, double c_re, double c_im) {
    return check_request(FAMILY_STABILITY, request, f, check_shifted_coefficient(c_re, c_im));
}
inline Verdict check_state_gradient_request(const HandleFacts& f, double c_jac = 1.0, double c_mass = 0.0) {
    return check_request(FAMILY_STATE_GRADIENT, GREQ_STATE_GRADIENT, f, check_state_gradient_args(c_jac, c_mass));
}
inline Verdict check_raw_jacobian_request(RawJacobianRequest request, const HandleFacts& f, const RawJacobianArgs& a = {}) {
    return check_request(FAMILY_RAW_JACOBIAN, request, f, request == JREQ_APPLY ? check_raw_jacobian_args(a) : Verdict{});
}

inline Verdict check_resolvent_energy_request(const HandleFacts& f, const EnergyArgs& a = {}) {
    return check_request(FAMILY_RESOLVENT, RREQ_ENERGY, f, check_energy_args(a));
}
inline Verdict check_resolvent_lanczos_request(const HandleFacts& f, const ResolventArgs& a = {}) {
    return check_request(FAMILY_RESOLVENT, RREQ_LANCZOS, f, check_resolvent_args(a));
}

// ---- which operator is it? (the spectral estimates of csrc/sns_damping.hip; the cases are in DESIGN.md) -----------------------------
// What the fine operator's values depend on beside the state: the form's share (FormKey: time term, viscosity law, and a counter
// that moves whenever the viscosity field is written or cleared, another that moves whenever a boundary coefficient -- the
// backflow beta, the Robin alpha -- is written or cleared) and the call's (the form id, the Reynolds number, the six
// parameters of a scalar assembly, whether the values were transposed since).  The handle keeps the key of the operator in
// levels[0].vals and the key of the operator the levels' estimates were taken on; a set-up takes them again iff the two differ.
struct FormKey {
    double sigma = 0.0, theta = 0.0;
    bool law_on = false;
    double lambda = 0.0, n = 1.0, r = 0.0;
    uint64_t nu_generation = 0;
    uint64_t boundary_generation = 0;
    bool operator==(const FormKey& o) const {
        return sigma == o.sigma && theta == o.theta && law_on == o.law_on && lambda == o.lambda && n == o.n && r == o.r &&
               nu_generation == o.nu_generation && boundary_generation == o.boundary_generation;
    }
};
struct OperatorKey {
    int form = -1;                                          // (no operator: equal to no assembled one)
    double reynolds = 0.0;
    bool transposed = false;
    FormKey f;
    double scalar[6] = {0, 0, 0, 0, 0, 0};                  // kappa[4], sigma, theta of the last scalar assembly (kept by the flow assemblies)
    bool operator==(const OperatorKey& o) const {
        return form == o.form && reynolds == o.reynolds && transposed == o.transposed && f == o.f &&
               std::equal(scalar, scalar + 6, o.scalar);
    }
};
// an assembly of `form` rewrote the operator (scalar_par: the parameters of a scalar assembly, null for a flow assembly)
inline void stamp_operator(OperatorKey& k, int form, double reynolds, const FormKey& f, const double* scalar_par = nullptr) {
    k.form = form;
    k.reynolds = reynolds;
    k.transposed = false;
    k.f = f;
    if (scalar_par) std::copy(scalar_par, scalar_par + 6, k.scalar);
}
// (r3_estimates: SNS_R3_SPECTRAL_ESTIMATE, the every-fourth-set-up cadence alone)
inline bool new_operator(const OperatorKey& matrix, const OperatorKey& estimated, bool r3_estimates) {
    return !r3_estimates && !(matrix == estimated);
}

// ---- smoother damping (the transitions are in csrc/sns_damping.hip; the rule is in DESIGN.md, "Damping state") ---------------------
// A level's damped block-Jacobi sweep x += w S (b - A x) and what its w was derived from: |lambda|max of S A (0: no estimate),
// the stability limit of the dominant Ritz values (0: not estimated), the damping that passed the growth check at the last
// fresh estimate (0: none).  The handle adds the factor of the retries (damping_backoff) and the count of set-ups (pc_setups).
struct LevelDamping {
    double omega = 0.8, lambda_max = 0.0, omega_checked = 0.0, ritz_limit = 0.0;
};
constexpr int ESTIMATE_EVERY = 4;                          // the spectrum moves little between the Jacobians of one Newton sequence
constexpr double LAMBDA_CAP = 4.0 / 3.0;                   // w <= 4 / (3 |lambda|max), the smoothing-optimal damping
constexpr int COMPOUNDING_SWEEPS = 3;                      // sweeps per cycle from which a level compounds an amplified mode
constexpr double GROWTH_BOUND = 0.9;                       // a sweep must contract the dominant mode by >= 10 % ...
constexpr double GROWTH_STEP = GROWTH_BOUND;               // ... and every trial that does not scales the damping by as much,
constexpr int GROWTH_TRIALS = 6;                           // this many times at the most
constexpr double RETRY_FACTOR = 0.7, RETRY_FLOOR = 0.4;    // a retry scales every damping; none is offered at or below the floor

// the estimates of a level are taken at this set-up: it has none, every ESTIMATE_EVERY-th set-up, a new operator
inline bool estimates_due(bool has_estimate, int pc_setups, bool new_operator) {
    return !has_estimate || pc_setups % ESTIMATE_EVERY == 0 || new_operator;
}
// levels that run COMPOUNDING_SWEEPS or more sweeps per cycle and are not the last: the Ritz limit (amg_ritz_limit) and the growth check
inline bool takes_growth_check(bool not_last, int sweeps_per_cycle) { return not_last && sweeps_per_cycle >= COMPOUNDING_SWEEPS; }
inline bool takes_ritz_limit(const sns_options& o, bool not_last, int sweeps_per_cycle) {
    return o.amg_ritz_limit && takes_growth_check(not_last, sweeps_per_cycle);
}
// the damping before the growth check: amg_omega, capped by |lambda|max where there is an estimate and by the Ritz limit where
// the level takes one, each times the factor of the retries
inline double capped_damping(double amg_omega, double backoff, double lambda_max, bool ritz, double ritz_limit) {
    double w = amg_omega * backoff;
    if (lambda_max > 0.0) w = std::min(amg_omega, LAMBDA_CAP / lambda_max) * backoff;
    if (ritz && ritz_limit > 0.0) w = std::min(w, ritz_limit * backoff);
    return w;
}
// the growth check: `growth(w, &g)` measures the growth per sweep of the dominant mode under w (an error code: passed on)
template <class Growth>
inline int checked_damping(double& w, Growth&& growth) {
    for (int trial = 0; trial < GROWTH_TRIALS; ++trial) {
        double g = 0.0;
        if (const int rc = growth(w, &g)) return rc;
        if (g < GROWTH_BOUND) break;
        w *= GROWTH_STEP;
    }
    return SNS_OK;
}
// between fresh estimates a level stays at or below the damping that passed
inline double held_damping(double w, double omega_checked) { return omega_checked > 0.0 ? std::min(w, omega_checked) : w; }
// the retry of a failed solve: which reasons, whether one is offered, and what it does to the factor and to a level -- the
// stored values are scaled in place, not derived again from the factor (two retries: (w 0.7) 0.7, not w 0.49)
inline bool retryable(int reason) {
    return reason == SNS_KSP_DIVERGED_BREAKDOWN || reason == SNS_KSP_DIVERGED_NANORINF || reason == SNS_KSP_STALLED;
}
inline bool retry_offered(const sns_options& o, double backoff) {
    return o.pc_type == SNS_PC_AMG && o.amg_retry_damping != 0 && backoff > RETRY_FLOOR;
}
inline void back_off(double& backoff) { backoff *= RETRY_FACTOR; }
inline void back_off(LevelDamping& d) {
    d.omega *= RETRY_FACTOR;
    if (d.omega_checked > 0.0) d.omega_checked *= RETRY_FACTOR;
}
// an options call: every estimate is taken and verified again (omega itself is rewritten by the next set-up)
inline void forget_estimates(LevelDamping& d) { d.lambda_max = d.omega_checked = d.ritz_limit = 0.0; }

// ---- the fixed cost of a linear solve (csrc/sns_krylov.hip, sns_cycle.hip; DESIGN.md, "The fixed cost of a solve") ----------------
// Work a BiCGStab solve queues that its result does not need, and where it may be left out: on a SERIAL handle only -- a
// partitioned one keeps its schedule, its hand-offs are pinned as they are.  Facts: the ranks of the handle; the Krylov method
// and the preconditioner; fine_plain_cycle -- the preconditioner's fine level runs the plain form of the cycle and has a level
// below it (vcycle, not vcycle_windows, not the replicated tail, not a single level); zero_guess_vouched -- the caller zeroed
// the guess itself on the solve's stream; estimates_due -- a level takes its spectral estimates at this set-up (asked by the
// set-up alone); plain_step -- the switch SNS_PLAIN_STEP (not an option), today's schedule whatever else.
struct StepFacts {
    int nranks = 1, ksp_type = SNS_KSP_BICGSTAB, pc_type = SNS_PC_AMG;
    bool fine_plain_cycle = false, zero_guess_vouched = false, estimates_due = true, plain_step = false;
};
// skip_zero_guess_residual: r0 is a copy of b, no operator pass.  export_ax: the pass behind the reported true residual is
// A x into the caller's buffer (the residual is b minus that), where the caller asks for it.  staged_speculation: the
// speculative half iteration is queued in two stages around the host's look at the residual -- the x / r / p update and the
// head of the preconditioner before, the rest after and only if the iteration goes on.  split_cycle: that head is the fine
// level's cycle through the restriction (else the whole application: it is cheap, or cannot be cut).  setup_two_streams: the
// set-up's latency-bound chain -- the Galerkin products down the levels, the last level's inverse -- runs on a stream of its own
// beside the levels' bandwidth-bound passes; not while estimates are taken, which solve on the levels as they are refreshed
struct StepPlan {
    bool skip_zero_guess_residual = false, export_ax = false, staged_speculation = false, split_cycle = false,
         setup_two_streams = false;
    bool operator==(const StepPlan& o) const {
        return skip_zero_guess_residual == o.skip_zero_guess_residual && export_ax == o.export_ax &&
               staged_speculation == o.staged_speculation && split_cycle == o.split_cycle && setup_two_streams == o.setup_two_streams;
    }
};
inline StepPlan plan_step(const StepFacts& f) {
    StepPlan p;
    if (f.nranks != 1 || f.plain_step || f.ksp_type != SNS_KSP_BICGSTAB) return p;
    p.skip_zero_guess_residual = f.zero_guess_vouched;
    p.export_ax = true;
    // under the AMG preconditioner only what can be cut is staged: a cycle of another form runs whole, as it always did
    p.split_cycle = f.pc_type == SNS_PC_AMG && f.fine_plain_cycle;
    p.staged_speculation = f.pc_type != SNS_PC_AMG || p.split_cycle;
    p.setup_two_streams = f.pc_type == SNS_PC_AMG && !f.estimates_due;
    return p;
}

// ---- the nonlinear drivers (csrc/sns_solve.hip; the contract is in DESIGN.md, "Nonlinear drivers") ----------------------------------
// The stopping rules of the Krylov methods and of the Newton loop, and the reference's bt line search (cubic backtracking), as
// arithmetic on a handful of doubles: the drivers launch and measure, the answers come from here.
// a residual norm at or below tol = max(ksp_rtol ||b||, ksp_atol) ends a linear solve; which of the two it met is the reason
inline int ksp_converged(double rn, double tol, double atol) {
    if (!(rn <= tol)) return 0;
    return rn <= atol ? SNS_KSP_CONVERGED_ATOL : SNS_KSP_CONVERGED_RTOL;
}
// the Newton loop before its first step (f = ||F|| of the guess) and after step `it` (f0: the norm at the start; step_norm =
// lambda ||y||; x_norm = ||w|| after the step).  0: go on.  The iteration limit comes last and is asked BEFORE the next
// Jacobian is assembled: no Jacobian after the last iteration
inline int snes_start(double f, const sns_options& o) {
    if (!(f == f)) return SNS_SNES_DIVERGED_FNORM_NAN;
    if (f < o.snes_atol) return SNS_SNES_CONVERGED_FNORM_ABS;
    return o.snes_max_it <= 0 ? SNS_SNES_DIVERGED_MAX_IT : 0;
}
inline int snes_after_step(double f, double f0, double step_norm, double x_norm, int it, const sns_options& o) {
    if (f < o.snes_atol) return SNS_SNES_CONVERGED_FNORM_ABS;
    if (f <= o.snes_rtol * f0) return SNS_SNES_CONVERGED_FNORM_RELATIVE;
    if (step_norm < o.snes_stol * x_norm) return SNS_SNES_CONVERGED_SNORM_RELATIVE;
    return it >= o.snes_max_it ? SNS_SNES_DIVERGED_MAX_IT : 0;
}
// The line search along x - lambda y.  f: ||F|| at the current state; initslope: F . (J y) as measured -- made a descent slope
// here (a positive one is negated, zero becomes -1).  lambda() is the step to try, the first is 1; offer(gn) takes ||F|| at that
// trial.  A trial is accepted by sufficient decrease (ls_alpha); after the first rejection the next step minimises the
// quadratic through f, the slope and the trial, after every later one the cubic through the last two trials, each kept within
// [0.1, 0.5] of the step before.  ls_max_it trials follow the first.  A NaN at the first trial and a non-finite norm at a
// later one end the search with FAIL_NAN (no later trial could be accepted).  No device access, no handle.
constexpr double ls_alpha = 1e-4;
constexpr int ls_max_it = 40;
struct LineSearch {
    enum Answer { ACCEPT = 0, TRY_AGAIN, FAIL_LINE_SEARCH, FAIL_NAN };
    LineSearch(double f_, double initslope) : f(f_), slope(initslope > 0 ? -initslope : initslope) {
        if (slope == 0) slope = -1.0;
    }
    double lambda() const { return lam; }
    Answer offer(double gn) {
        const bool first = trials++ == 0;
        if (0.5 * gn * gn <= 0.5 * f * f + lam * ls_alpha * slope) return ACCEPT;
        if (first ? !(gn == gn) : !std::isfinite(gn)) return FAIL_NAN;
        if (trials > ls_max_it) return FAIL_LINE_SEARCH;
        double lamtemp;
        if (first) {
            lamtemp = -slope / (gn * gn - f * f - 2.0 * lam * slope);
        } else {
            const double t1 = 0.5 * (gn * gn - f * f) - lam * slope;
            const double t2 = 0.5 * (gprev * gprev - f * f) - lamprev * slope;
            const double a = (t1 / (lam * lam) - t2 / (lamprev * lamprev)) / (lam - lamprev);
            const double bq = (-lamprev * t1 / (lam * lam) + lam * t2 / (lamprev * lamprev)) / (lam - lamprev);
            const double d = std::max(bq * bq - 3 * a * slope, 0.0);
            lamtemp = (a == 0) ? -slope / (2.0 * bq) : (-bq + std::sqrt(d)) / (3.0 * a);
        }
        lamprev = lam;
        gprev = gn;
        lam = std::min(std::max(lamtemp, 0.1 * lam), 0.5 * lam);
        return TRY_AGAIN;
    }

   private:
    double f, slope, lam = 1.0, lamprev = 1.0, gprev = 0.0;
    int trials = 0;
};

// ---- the least-squares problem of FGMRES (csrc/sns_krylov.hip: fgmres, T = double; csrc/sns_shifted.hip: cfgmres, T =
// std::complex<double>; tests/givens_lsq_main.cpp) ------------------------------------------------------------------------------------
// min |beta e1 - H y| over a cycle of at most m columns by Givens rotations [cs, sn; -conj(sn), cs] with cs real.  restart(beta)
// opens a cycle; push_column(j, h, wn) takes column j -- its j + 1 Gram-Schmidt coefficients and the norm wn >= 0 of what was
// left --, applies the earlier rotations, forms the new one and returns the residual estimate |g[j + 1]|; solve(j) is the
// minimiser over the first j columns.  H is stored by columns of m + 1.  The two types differ in the new rotation alone, and
// each keeps its own formula: the real one is not the complex one at zero imaginary part, the two do not round alike.
// No device access, no handle.
inline double givens_conj(double v) { return v; }
inline std::complex<double> givens_conj(const std::complex<double>& v) { return std::conj(v); }
template <class T>
struct GivensLsq {
    int m;
    std::vector<T> H, sn, g, y;
    std::vector<double> cs;
    explicit GivensLsq(int m_) : m(m_), H((size_t)(m_ + 1) * m_, T(0.0)), sn(m_), g(m_ + 1), y(m_), cs(m_) {}
    void restart(double beta) {
        std::fill(g.begin(), g.end(), T(0.0));
        g[0] = beta;
    }
    double push_column(int j, const T* h, double wn) {
        T* Hj = &H[(size_t)j * (m + 1)];
        for (int k = 0; k <= j; ++k) Hj[k] = h[k];
        Hj[j + 1] = wn;
        for (int k = 0; k < j; ++k) {                      // previous rotations
            const T t0 = cs[k] * Hj[k] + sn[k] * Hj[k + 1];
            Hj[k + 1] = -givens_conj(sn[k]) * Hj[k] + cs[k] * Hj[k + 1];
            Hj[k] = t0;
        }
        if constexpr (std::is_same<T, double>::value) {
            const double den = std::hypot(Hj[j], wn);
            cs[j] = den > 0 ? Hj[j] / den : 1.0;
            sn[j] = den > 0 ? wn / den : 0.0;
            Hj[j] = den;
        } else {
            const double aa = std::abs(Hj[j]), den = std::hypot(aa, wn);
            if (den > 0.0 && aa > 0.0) {
                cs[j] = aa / den;
                sn[j] = (Hj[j] / aa) * (wn / den);
                Hj[j] = Hj[j] * (den / aa);
            } else {
                cs[j] = den > 0.0 ? 0.0 : 1.0;
                sn[j] = den > 0.0 ? 1.0 : 0.0;
                Hj[j] = wn;
            }
        }
        Hj[j + 1] = 0.0;
        g[j + 1] = -givens_conj(sn[j]) * g[j];
        g[j] = cs[j] * g[j];
        return std::abs(g[j + 1]);
    }
    const std::vector<T>& solve(int j) {                   // y = H^-1 g over the leading j columns
        for (int k = j - 1; k >= 0; --k) {
            T sacc = g[k];
            for (int q = k + 1; q < j; ++q) sacc -= H[(size_t)q * (m + 1) + k] * y[q];
            y[k] = sacc / H[(size_t)k * (m + 1) + k];
        }
        return y;
    }
};

}  // namespace policy
}  // namespace sns
