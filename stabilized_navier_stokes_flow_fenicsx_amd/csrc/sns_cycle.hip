// The V-cycle (serial, partitioned over RCCL, partitioned over the window transports), the hipGraph of its launch-bound tail,
// and the preconditioner / operator applications the Krylov methods call.
// (shared internals in csrc/sns_ctx.h)
#include "sns_ctx.h"

namespace sns {

// Coarse part of the cycle (the graph level and below) as ONE hipGraph launch.  Captured on a private
// stream (the caller's stream may be the legacy default stream, which cannot be captured), re-captured when
// the per-level damping or the plan of the levels it covers changed.  Distributed runs capture the replicated tail only (the
// exchanges above it are host-driven).  Any capture failure disables the graph for good.
int coarse_cycle(sns_ctx* h, int l, const double* b, double* x) {
    const int gl = h->plan.graph_level;
    if (gl <= 0 || l != gl || h->graph_disabled || (int)h->levels.size() <= gl + 1) return vcycle(h, l, b, x);
    // signature: the graph level, whether its first sweeps are done outside the graph, every omega, the plan rows from the level
    // above the graph down
    std::vector<double> sig = {(double)gl, (double)h->plan.rep_gather_first};
    for (auto& L : h->levels) sig.push_back(L.damping.omega);
    const std::vector<policy::LevelPlan> rows(h->plan.level.begin() + (gl - 1), h->plan.level.end());
    if (!h->coarse_graph || sig != h->graph_sig || rows != h->graph_rows) {
        h->coarse_graph.reset();
        if (!h->cap_stream && hipStreamCreateWithFlags(h->cap_stream.put(), hipStreamNonBlocking) != hipSuccess) {
            h->graph_disabled = true;
            return vcycle(h, l, b, x);
        }
        HIP_TRY(hipStreamSynchronize(h->stream));          // capture must not race with pending work on the buffers
        hipStream_t user = h->stream;
        hipGraph_t graph = nullptr;
        bool ok = hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (ok) {
            h->stream = h->cap_stream;
            const int rc = vcycle(h, l, b, x);
            h->stream = user;
            ok = (hipStreamEndCapture(h->cap_stream, &graph) == hipSuccess) && rc == SNS_OK && graph;
        }
        hipGraphExec_t exec = nullptr;
        if (ok) ok = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
        if (graph) (void)hipGraphDestroy(graph);
        if (!ok) {
            (void)hipGetLastError();
            h->graph_disabled = true;
            return vcycle(h, l, b, x);
        }
        *h->coarse_graph.put() = exec;
        h->graph_sig = sig;
        h->graph_rows = rows;
    }
    HIP_TRY(hipGraphLaunch(h->coarse_graph, h->stream));
    return SNS_OK;
}


// ---- the stages both forms of the cycle launch ----------------------------------------------------------------------------------

// Where level l's coarse-grid problem lives.  rep_src: the level below is only the source of the replicated tail -- its right-hand
// side is restricted straight into the all-gather's send buffer, and the correction is prolongated straight from this rank's rows
// of the replicated solution (no copies)
struct CoarseVectors {
    bool rep_src;
    double* cb;
    const double* cx;
};
static CoarseVectors coarse_vectors(sns_ctx* h, int l) {
    Level& C = h->levels[l + 1];
    const bool rep_src = h->rep_level > 0 && l + 1 == h->rep_level - 1;
    if (!rep_src) return {false, C.b, C.x};
    return {true, h->rep_bsend, h->levels[h->rep_level].x + 4 * (size_t)h->rep_off};
}

// Restriction of level l's residual into the coarse right-hand side cb, with the coarse level's first sweep (into the buffer its
// cycle starts from) where the plan fuses it.  fused: the residual b - A x is computed in the same launch (k_resid_restrict), else
// L.r holds it (k_restrict_blk onto the coarse level's aggregate blocks, k_restrict).  gs: the ghost entries of x from this receive
// window (the window form); agp / pd: the all-gather piece / the put the launch carries
static void launch_restrict(sns_ctx* h, int l, bool fused, const double* x, const double* b, double* cb, const GhostSrc* gs = nullptr,
                            const AgPut& agp = AgPut(), const PutDst& pd = PutDst()) {
    const Level& L = h->levels[l];
    const Level& C = h->levels[l + 1];
    const policy::LevelPlan& Q = h->plan.level[(size_t)l];
    const policy::LevelPlan& QC = h->plan.level[(size_t)l + 1];
    const bool fuse = policy::first_sweep_owner(h->plan, h->rep_level, l + 1) == policy::FIRST_SWEEP_RESTRICTION;
    const float* dc = fuse ? C.dinv32 : nullptr;
    double* zc = fuse ? cycle_start(h, l + 1, C.x) : nullptr;   // (the coarse cycle is called with x = C.x)
    if (fused) {
        // mode of the coarse level's first sweep: 0 none, 1 nodal D^-1, 2 its aggregate blocks (walked in THEIR order)
        const int mode = !fuse ? 0 : (QC.blocks ? 2 : 1);
        const int32_t* slots = mode == 2 ? C.blk_rows : nullptr;
        const int32_t n_slots = mode == 2 ? 8 * C.n_blk : C.n_owned;
        const unsigned grid = (unsigned)((n_slots + 7) / 8);
        if (l == 0) time_begin(h, SPMV_B_MINUS_AX);                      // (bench.py's per-launch accounting of the fine-level passes)
        with_fmt(Q.lp_fmt, [&](auto F) {
            dispatch<2, 1, 0>(mode, [&](auto M) {
                dispatch<1, 0>(gs != nullptr, [&](auto G) {
                    const LpMat A = lp_mat<F>(L);
                    hipLaunchKernelGGL((k_resid_restrict<F, M, G>), dim3(grid), dim3(256), 0, h->stream, C.n_owned, n_slots, slots,
                                       L.m_ptr, L.m_idx, L.free_mask, L.rowptr, L.colind, A.vals, A.scale, x, b, L.r, cb, dc,
                                       (const void*)C.binv32, C.damping.omega, zc, gs ? *gs : GhostSrc(), agp, pd);
                });
            });
        });
        if (l == 0) time_end(h);
    } else if (fuse && QC.blocks) {
        const int32_t ns = 8 * C.n_blk;
        with_fmt(C.binv_fmt, [&](auto F) {
            hipLaunchKernelGGL((k_restrict_blk<F>), dim3((unsigned)((ns + 63) / 64)), dim3(256), 0, h->stream, ns, C.blk_rows, L.m_ptr,
                               L.m_idx, L.free_mask, L.r, cb, (const void*)C.binv32, C.damping.omega, zc, pd);
        });
    } else {
        hipLaunchKernelGGL(k_restrict, dim3((unsigned)((4 * (int64_t)C.n_owned + 255) / 256)), dim3(256), 0, h->stream,
                           C.n_owned, L.m_ptr, L.m_idx, L.free_mask, L.r, cb, dc, C.damping.omega, zc);
    }
}

// Fused coarse-grid correction + first post-smoothing sweep of level l over M = A P: y = (x + P xc) + w S (r - M xc), r the
// residual restricted before (k_bpost on the aggregate blocks, else k_post_lp).  xc_own: this rank's rows of the coarse solution,
// apc: M's column ids, gc: the window form's source of the ghost aggregates' part of xc (k_bpost reads it where it has a window), pd:
// the put the launch carries.  Level 0 is timed as mode 4
static void launch_post(sns_ctx* h, int l, const double* xc, const double* xc_own, const int32_t* apc, const double* x, double* y,
                        const GhostSrc* gc = nullptr, const PutDst& pd = PutDst()) {
    const Level& L = h->levels[l];
    const policy::LevelPlan& Q = h->plan.level[(size_t)l];
    const int32_t rows = L.n_owned;
    const GhostSrc g = gc ? *gc : GhostSrc();
    if (l == 0) time_begin(h, 4);
    with_fmt(Q.lp_fmt, [&](auto F) {
        const LpMat M = ap_mat<F>(L);
        if (Q.blocks) {
            const int32_t ns = 8 * L.n_blk;
            dispatch<1, 0>(g.win[0] != nullptr, [&](auto G) {
                hipLaunchKernelGGL((k_bpost<F, G>), dim3((unsigned)((ns + 63) / 64)), dim3(256), 0, h->stream, ns, L.blk_rows,
                                   L.ap_rowptr, apc, M.vals, M.scale, (const void*)L.binv32, xc, xc_own, x, (const double*)L.r,
                                   L.damping.omega, L.agg, L.free_mask, y, g, pd);
            });
        } else {
            // (nodal blocks: FINE 1 the fine level, 0 a coarse one, 2 the fine level of the window form)
            dispatch<2, 1, 0>(gc ? 2 : l == 0 ? 1 : 0, [&](auto FINE) {
                hipLaunchKernelGGL((k_post_lp<F, FINE>), dim3((rows + 63) / 64), dim3(256), 0, h->stream, rows, L.ap_rowptr, apc,
                                   M.vals, M.scale, xc, x, (const double*)L.r, L.dinv32, L.damping.omega, L.agg, L.free_mask, y, g);
            });
        }
    });
    if (l == 0) time_end(h);
}


// The V-cycle of a PARTITIONED level over a window transport (peer windows / the in-process team; round 5).  Every exchange is one
// put launch (comm_put) and the pass behind it reads the ghost entries from the level's receive window, its boundary waves waiting
// for the neighbours themselves: no staging copy, no unpack, no split pass.  Level 0: first sweep | put, residual | restriction
// (+ level 1's first sweep) | coarse | put of level 1's solution, fused correction + post-sweep.  Level >= 1 (plan exact): the
// single-GPU schedule with exact global sweeps -- [put, sweep]* | put, residual + restriction (+ next first sweep) in one launch |
// coarse | fused correction + first post-sweep (the coarse solution read straight from the replicated tail where that is the next
// level, else after a put of it) | [put, sweep]*.
int vcycle_windows(sns_ctx* h, int l, const double* b, double* x) {
    Level& L = h->levels[l];
    Level& C = h->levels[l + 1];
    Comm* c = h->comm.get();
    const Plan& P = c->plans[l];
    const policy::LevelPlan& Q = h->plan.level[(size_t)l];
    const policy::LevelPlan& QC = h->plan.level[(size_t)l + 1];
    const int32_t rows = L.n_owned;
    const double om = L.damping.omega;
    const int nu_pre = Q.pre, nu_post = Q.post;
    double* cur = cycle_start(h, l, x);
    double* oth = (cur == x) ? h->levels[l].pong : x;
    // The put of every exchange of this level's iterate rides in the kernel that PRODUCES the iterate (PutDst) where that is an
    // aggregate-block kernel: `carry` records it with the hand-off state, window_put -- every exchange -- asks there
    const bool blk = Q.blocks != 0;
    const PutDst pdl = (h->plan.fuse_puts && blk && rows > 0) ? comm_put_dst(c, P) : PutDst();
    const GhostSrc gs = comm_ghost_src(c, P);
    auto carry = [&](const PutDst& pd, int lv, const double* v) -> int {
        return pd.sr_ptr ? handoff_legal(h->handoff.put_carried(lv, v), "a second carried put before the first was taken", lv) : SNS_OK;
    };
    const bool by_krylov = h->handoff.enter_level(l);
    if (!by_krylov && rows > 0 && policy::first_sweep_owner(h->plan, h->rep_level, l) == policy::FIRST_SWEEP_LEVEL) {
        PutDst pd1 = pdl;
        launch_first_sweep(h, Q, L, rows, b, om, cur, &pd1);
        SNS_TRY(carry(pd1, l, cur));
    }
    for (int s = 1; s < nu_pre; ++s) {                     // (level >= 1 only: the fine level runs one sweep per half cycle)
        SNS_TRY(window_put(h, l, cur));
        if (rows > 0 && blk) {
            launch_sweep(h, Q, L, rows, cur, oth, b, om, &gs, pdl);
            SNS_TRY(carry(pdl, l, oth));
        }
        std::swap(cur, oth);
    }
    const auto [rep_src, cb, cx] = coarse_vectors(h, l);
    const bool fuse = policy::first_sweep_owner(h->plan, h->rep_level, l + 1) == policy::FIRST_SWEEP_RESTRICTION;
    // residual (+ restriction): the true residual needs the neighbours' iterate
    SNS_TRY(window_put(h, l, cur));
    // (the next level's first sweep, written by the restriction, is exchanged first thing in its cycle: put from here)
    const PutDst pdc = (h->plan.fuse_puts && fuse && QC.blocks && !rep_src && QC.windows && C.n_owned > 0 &&
                        (l == 0 || rows > 0))
                           ? comm_put_dst(c, c->plans[l + 1]) : PutDst();
    if (l == 0) {
        Split s3;
        s3.mode = SPLIT_WINDOW;
        s3.gs = gs;
        if (rows > 0) launch_pc_spmv<SPMV_B_MINUS_AX>(h, L, Q.lp_fmt, rows, cur, L.r, b, 0.0, s3);
        if (C.n_owned > 0) launch_restrict(h, l, false, nullptr, nullptr, cb, nullptr, AgPut(), pdc);
    } else if (rows > 0 && C.n_owned > 0) {
        // (the level below is the source of the replicated tail: the restricted right-hand side goes straight into every rank's
        // all-gather staging area, the tail's first sweep waits for it -- rep_gather_first)
        const AgPut agp = (rep_src && h->plan.rep_gather_first) ? comm_ag_put(c, 4 * (int64_t)h->rep_maxn) : AgPut();
        launch_restrict(h, l, true, cur, b, cb, &gs, agp, pdc);
    }
    SNS_TRY(carry(pdc, l + 1, cycle_start(h, l + 1, C.x)));
    SNS_TRY(coarse_cycle(h, l + 1, cb, rep_src ? nullptr : C.x));
    // fused coarse-grid correction + first post-smoothing sweep over M = A P; the ghost aggregates' part of the coarse solution:
    // level >= 1 above the replicated tail reads every entry from the replicated solution (M's columns renumbered into its ids,
    // ap_colind_rep), else one put of the coarse level's solution and the window behind it
    GhostSrc gc;
    const double* xc = cx;
    const int32_t* apc = L.ap_colind;
    if (rep_src && l >= 1) {
        xc = h->levels[h->rep_level].x;
        apc = L.ap_colind_rep;
    } else {
        SNS_TRY(window_put(h, l + 1, cx));                           // (the level below may have put its result with its last kernel)
        gc = comm_ghost_src(c, c->plans[l + 1]);
    }
    // this level's result is exchanged next by the level above (its correction reads it) or, the fine level's, by the operator
    // application the caller of pc_apply has promised: the last kernel of the cycle puts it
    const bool last_puts = pdl.sr_ptr && (l == 0 ? h->handoff.op_promised : h->plan.level[(size_t)l - 1].windows != 0);
    if (rows > 0) {                                        // (nodal blocks: the fine level only, see the plan's exact)
        const PutDst pd = (nu_post > 1 || last_puts) ? pdl : PutDst();
        launch_post(h, l, xc, cx, apc, cur, oth, &gc, pd);
        SNS_TRY(carry(pd, l, oth));
    }
    std::swap(cur, oth);
    for (int s = 1; s < nu_post; ++s) {
        SNS_TRY(window_put(h, l, cur));
        if (rows > 0 && blk) {
            const PutDst pd = (s + 1 < nu_post || last_puts) ? pdl : PutDst();
            launch_sweep(h, Q, L, rows, cur, oth, b, om, &gs, pd);
            SNS_TRY(carry(pd, l, oth));
        }
        std::swap(cur, oth);
    }
    // cur == x by construction of the start buffer: where the last kernel carried its put, the level is left with it recorded
    return SNS_OK;
}


// The level above the replicated tail (l = rep_level - 1): all-gather the right-hand side, cycle the replicated tail, keep my rows
// of the result
static int enter_replicated_tail(sns_ctx* h, int l, const double* b, double* x) {
    const int32_t rows = h->levels[l].n_owned;
    Level& C = h->levels[h->rep_level];
    if (rows > 0 && b != h->rep_bsend)                   // (vcycle of the level above restricts straight into rep_bsend)
        HIP_TRY(hipMemcpyAsync(h->rep_bsend, b, 4 * (size_t)rows * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    Comm* cm = h->comm.get();
    if (policy::first_sweep_owner(h->plan, h->rep_level, h->rep_level) == policy::FIRST_SWEEP_GATHER) {
        // both halves of the all-gather ride in solver kernels: the residual + restriction of the level above has stored this
        // rank's piece into every rank's staging area, the first sweep of the replicated level waits for the pieces itself
        SNS_TRY(peer_check(cm));
        SNS_TRY(comm_host_barrier(cm, h->stream));
        const int32_t ns = 8 * C.n_blk;
        double* zc = cycle_start(h, h->rep_level, C.x);
        with_fmt(C.binv_fmt, [&](auto F) {
            hipLaunchKernelGGL((k_bfirst_gather<F>), dim3((unsigned)((ns + 63) / 64)), dim3(256), 0, h->stream, ns, C.blk_rows,
                               (const void*)C.binv32, C.damping.omega, zc, C.b, h->rep_rowmap, comm_ag_get(cm));
        });
    } else if (cm->windows() && h->opt.halo_windows && h->rep_doff &&
        (size_t)4 * h->rep_maxn * (size_t)cm->nranks <= cm->peer->ag_doubles) {
        // (every rank's rows land where the replicated level keeps them: no gather kernel behind the all-gather)
        SNS_TRY(comm_allgatherv(cm, h->rep_bsend, C.b, 4 * h->rep_maxn, h->rep_doff, h->rep_dcnt, h->stream));
    } else {
        SNS_TRY(comm_allgather(cm, h->rep_bsend, h->rep_brecv, 4 * h->rep_maxn, h->stream));
        hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)((4 * (int64_t)h->rep_NG + 255) / 256)), dim3(256), 0, h->stream,
                           h->rep_NG, h->rep_rowmap, h->rep_brecv, C.b);
    }
    SNS_TRY(coarse_cycle(h, h->rep_level, C.b, C.x));
    if (rows > 0 && x)                                   // (x == nullptr: the caller reads its rows of C.x in place)
        HIP_TRY(hipMemcpyAsync(x, C.x + 4 * (size_t)h->rep_off, 4 * (size_t)rows * sizeof(double),
                               hipMemcpyDeviceToDevice, h->stream));
    return SNS_OK;
}

// The last level: the all-gathered global dense inverse, the dense inverse, its fp32 copy from the blocked Gauss-Jordan
// elimination, or -- too large for a dense solve -- a fixed number of Jacobi sweeps (still a linear operator)
static int solve_last_level(sns_ctx* h, int l, const double* b, double* x) {
    Level& L = h->levels[l];
    const int32_t rows = L.n_owned;
    if (h->cg_N > 0) {
        const int N = h->cg_N, mr = 4 * h->cg_maxn;
        HIP_TRY(hipMemsetAsync(h->cg_send, 0, mr * sizeof(double), h->stream));
        if (rows > 0)
            HIP_TRY(hipMemcpyAsync(h->cg_send, b, 4 * (size_t)rows * sizeof(double), hipMemcpyDeviceToDevice,
                                   h->stream));
        SNS_TRY(comm_allgather(h->comm.get(), h->cg_send, h->cg_recv, mr, h->stream));
        if (rows > 0)
            hipLaunchKernelGGL(k_dense_matvec, dim3((4 * rows + 3) / 4), dim3(256), 0, h->stream, N,
                               h->cg_full + (size_t)h->comm->rank * mr * N, h->cg_recv, x, 4 * rows);
        return SNS_OK;
    }
    if (L.dense_inv) {
        const int N = 4 * L.n;
        hipLaunchKernelGGL(k_dense_matvec, dim3((N + 3) / 4), dim3(256), 0, h->stream, N, L.dense_inv, b, x, N);
        return SNS_OK;
    }
    if (L.dense_x32) {
        const int N = 4 * L.n;
        hipLaunchKernelGGL(k_dense_matvec32, dim3((N + 3) / 4), dim3(256), 0, h->stream, N, L.dense_np, L.dense_x32, b, x);
        return SNS_OK;
    }
    double* cur = x;
    double* oth = h->levels[l].pong;
    if (rows == 0) return SNS_OK;
    hipLaunchKernelGGL(k_bjacobi, dim3((unsigned)((4 * (int64_t)rows + 255) / 256)), dim3(256), 0, h->stream, rows, L.dinv, b,
                       L.damping.omega, cur);
    for (int s = 0; s < 8; ++s) {       // even count: result ends in x
        launch_pc_spmv<SPMV_JACOBI>(h, L, h->plan.level[(size_t)l].lp_fmt, rows, cur, oth, b, L.damping.omega);
        std::swap(cur, oth);
    }
    return SNS_OK;
}


// The plain form of the cycle on a level with a level below it, in two halves: the head runs through the restriction of the
// residual into the coarse right-hand side (with the next level's first sweep where the plan fuses it), the tail is the coarse
// cycle and everything behind it.  cur / oth: the ping-pong buffers as the head leaves them.  vcycle runs one behind the other;
// pc_apply_begin / pc_apply_finish cut the fine level's between them
static int vcycle_head(sns_ctx* h, int l, const double* b, double* x, double** cur_out, double** oth_out) {
    const policy::LevelPlan& Q = h->plan.level[(size_t)l];
    Level& L = h->levels[l];
    Level& C = h->levels[l + 1];
    const int32_t rows = L.n_owned;
    const double om = L.damping.omega;
    const int nu_pre = Q.pre;
    double* cur = cycle_start(h, l, x);
    double* oth = (cur == x) ? h->levels[l].pong : x;
    // distributed: on levels with few rows per rank the sweeps see the neighbours' current iterate (one small
    // exchange per sweep); on the big levels they stay rank-local (ghost values zero) and only the residual is exact
    const bool sx = Q.sx != 0;
    // ... and the sweeps AFTER the coarse-grid correction take the neighbours' corrected iterate as (frozen) ghost
    // values: with zero ghosts they would see the whole correction as a residual along the partition interfaces
    const bool px = Q.px != 0;
    const size_t ghost4 = 4 * (size_t)(L.n - rows);
    const bool tails_unused = (l == 0) && h->plan.fine_tails_unused;
    if (px && ghost4 > 0 && !tails_unused) {
        HIP_TRY(hipMemsetAsync(cur + 4 * (size_t)rows, 0, ghost4 * sizeof(double), h->stream));
        HIP_TRY(hipMemsetAsync(oth + 4 * (size_t)rows, 0, ghost4 * sizeof(double), h->stream));
    }
    // first sweep from a zero guess: z = omega D^-1 b, with the D^-1 copy the other sweeps of this level read (unless the Krylov
    // kernel, the restriction of the level above or the gather into the replicated tail has done it)
    const bool by_krylov = h->handoff.enter_level(l);
    if (!by_krylov && rows > 0 && policy::first_sweep_owner(h->plan, h->rep_level, l) == policy::FIRST_SWEEP_LEVEL)
        launch_first_sweep(h, Q, L, rows, b, om, cur);
    for (int s = 1; s < nu_pre; ++s) {
        if (sx) SNS_TRY(exchange_level(h, l, cur));
        launch_sweep(h, Q, L, rows, cur, oth, b, om);
        std::swap(cur, oth);
    }
    // Below the fine level the residual and the restriction (+ the next level's first sweep) are ONE launch (k_resid_restrict):
    // `xres` is then the vector the residual reads and the pass itself is issued with the restriction further down.
    // (amg_fuse_restrict = 2: a single-GPU fine level as well -- its residual kernel is the tuned k_spmv_lp, kept by default)
    const bool rr_fused = Q.fused_restrict && rows > 0 && C.n_owned > 0;
    const double* xres = cur;
    if (sx) {
        SNS_TRY(exchange_level(h, l, cur));
        if (!rr_fused) launch_pc_spmv<SPMV_B_MINUS_AX>(h, L, Q.lp_fmt, rows, cur, L.r, b, 0.0);
    } else if (L.xg && tails_unused) {
        // (fine level, fused post-sweep: the halo lands in the iterate's own ghost tail, no copy into the exchange vector)
        SNS_TRY(exchange_and_spmv<SPMV_B_MINUS_AX>(h, cur, cur, L.r, b, 0.0, nullptr, true));
    } else if (L.xg) {      // true residual needs the neighbours' iterate
        HIP_TRY(hipMemcpyAsync(L.xg, cur, 4 * (size_t)rows * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        if (l == 0) {
            SNS_TRY(exchange_and_spmv<SPMV_B_MINUS_AX>(h, L.xg, L.xg, L.r, b, 0.0, nullptr, true));
        } else {
            SNS_TRY(exchange_level(h, l, L.xg));
            xres = L.xg;
            if (!rr_fused) launch_pc_spmv<SPMV_B_MINUS_AX>(h, L, Q.lp_fmt, rows, L.xg, L.r, b, 0.0);
        }
    } else if (!rr_fused) {
        launch_pc_spmv<SPMV_B_MINUS_AX>(h, L, Q.lp_fmt, rows, cur, L.r, b, 0.0);
    }
    if (C.n_owned > 0) launch_restrict(h, l, rr_fused, xres, b, coarse_vectors(h, l).cb);
    *cur_out = cur;
    *oth_out = oth;
    return SNS_OK;
}

static int vcycle_tail(sns_ctx* h, int l, const double* b, double* cur, double* oth) {
    const policy::LevelPlan& Q = h->plan.level[(size_t)l];
    Level& L = h->levels[l];
    Level& C = h->levels[l + 1];
    const int32_t rows = L.n_owned;
    const double om = L.damping.omega;
    const int nu = Q.nu, nu_post = Q.post;
    const bool sx = Q.sx != 0, px = Q.px != 0;
    const size_t ghost4 = 4 * (size_t)(L.n - rows);
    const auto [rep_src, cb, cx] = coarse_vectors(h, l);
    SNS_TRY(coarse_cycle(h, l + 1, cb, rep_src ? nullptr : C.x));
    int s_first = 0;
    // Fused coarse-grid correction + first post-smoothing sweep (k_post_lp): z = (cur + P xc) + om Dinv (r - M xc) with
    // M = A P and r the residual restricted above -- the sweep reads M (0.37x the blocks of A on the fine level) instead
    // of A and the prolongation kernel disappears.  Serial levels always; a distributed fine level when its single
    // post-sweep is the exact global one (px): the ghost aggregates' corrections arrive by ONE level-(l+1) exchange
    // instead of the level-l halo of the corrected iterate.
    const bool fused_post = Q.fused_post != 0;
    if (fused_post) {
        const double* xc = cx;
        if (L.xg) {                                    // distributed fine level: xc incl. the neighbours' aggregates
            if (C.n_owned > 0)
                HIP_TRY(hipMemcpyAsync(C.xg, cx, 4 * (size_t)C.n_owned * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
            SNS_TRY(exchange_level(h, l + 1, C.xg));
            xc = C.xg;
        }
        if (rows > 0) launch_post(h, l, xc, xc, L.ap_colind, cur, oth);
        std::swap(cur, oth);
        s_first = 1;
    } else if (rows > 0) {
        hipLaunchKernelGGL(k_prolong_add, dim3((unsigned)((4 * (int64_t)rows + 255) / 256)), dim3(256), 0, h->stream, rows, L.agg,
                           L.free_mask, cx, cur);
    }
    if (fused_post) {
        // (the post-sweep is done; a partitioned fine level got its neighbours' corrections through xc)
    } else if (px && l == 0 && nu == 1) {
        // the single post-smoothing sweep of the fine level with the neighbours' corrected iterate: halo of `cur`
        // overlapped with the interior rows of the sweep
        SNS_TRY(exchange_and_spmv<SPMV_JACOBI>(h, cur, cur, oth, b, om, nullptr, true));
        std::swap(cur, oth);
        s_first = 1;
    } else if (px) {
        SNS_TRY(exchange_level(h, l, cur));
        if (ghost4 > 0 && nu > 1)
            HIP_TRY(hipMemcpyAsync(oth + 4 * (size_t)rows, cur + 4 * (size_t)rows, ghost4 * sizeof(double),
                                   hipMemcpyDeviceToDevice, h->stream));
    }
    for (int s = s_first; s < nu_post; ++s) {
        if (sx) SNS_TRY(exchange_level(h, l, cur));
        launch_sweep(h, Q, L, rows, cur, oth, b, om);
        std::swap(cur, oth);
    }
    // cur == x by construction of the start buffer
    return SNS_OK;
}

// V-cycle on level l: x <- approx A_l^-1 b  (x overwritten; zero initial guess)
int vcycle(sns_ctx* h, int l, const double* b, double* x) {
    if (h->rep_level > 0 && l == h->rep_level - 1) return enter_replicated_tail(h, l, b, x);
    if (l + 1 == (int)h->levels.size()) return solve_last_level(h, l, b, x);
    if (h->plan.level[(size_t)l].windows) return vcycle_windows(h, l, b, x);
    double *cur, *oth;
    SNS_TRY(vcycle_head(h, l, b, x, &cur, &oth));
    return vcycle_tail(h, l, b, cur, oth);
}


static int pc_apply_inner(sns_ctx* h, const double* r, double* z);
// (what the Krylov kernel in front handed over is consumed by the cycle this call runs and by nothing else; of the cycle's own
// hand-offs only the promised put of z outlives the call: policy::Handoff::end_pc_apply, on every way out)
int pc_apply(sns_ctx* h, const double* r, double* z) {
    const int rc = pc_apply_inner(h, r, z);
    int level = -1;
    const bool legal = h->handoff.end_pc_apply(rc == SNS_OK, z, &level);
    return rc != SNS_OK ? rc : handoff_legal(legal, "pc_apply ends with a carried put nobody took", level);
}

static int pc_apply_inner(sns_ctx* h, const double* r, double* z) {
    const int64_t nd = nred_of(h);
    switch (h->opt.pc_type) {
        case SNS_PC_NONE:
            HIP_TRY(hipMemcpyAsync(z, r, nd * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
            return SNS_OK;
        case SNS_PC_BJACOBI:
            hipLaunchKernelGGL(k_bjacobi, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, h->stream, h->n_owned,
                               h->levels[0].dinv, r, 1.0, z);
            return SNS_OK;
        case SNS_PC_AMG: {
            // distributed: the per-rank V-cycle must see ZERO ghost values on level 0 (block-Jacobi across ranks, like PETSc's
            // parallel default bjacobi): where z's ghost tail could be read, cycle in an internal buffer whose tail is never
            // written and copy the owned part out
            double* x = fine_cycle_vector(h, z);
            SNS_TRY(vcycle(h, 0, r, x));
            if (x != z) HIP_TRY(hipMemcpyAsync(z, x, nd * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
            return SNS_OK;
        }
    }
    set_error("bad pc_type");
    return SNS_E_ARG;
}

// whether the fine level of the AMG preconditioner runs the plain form of the cycle with a level below it: the form
// pc_apply_begin can cut behind the restriction
static bool fine_plain_cycle(const sns_ctx* h) {
    return h->opt.pc_type == SNS_PC_AMG && h->pc_ready && h->levels.size() >= 2 && h->plan.level.size() == h->levels.size() &&
           h->rep_level != 1 && !h->plan.level[0].windows;
}

// the facts of policy::plan_step gathered from the handle -- asked by the solve driver and by the set-up, nowhere else
policy::StepPlan step_plan(const sns_ctx* h, bool zero_guess_vouched, bool estimates_due) {
    policy::StepFacts f;
    f.nranks = h->comm ? std::max(2, h->comm->nranks) : 1;      // (a communicator attached: partitioned, whatever its size)
    f.ksp_type = h->opt.ksp_type;
    f.pc_type = h->opt.pc_type;
    f.fine_plain_cycle = fine_plain_cycle(h);
    f.zero_guess_vouched = zero_guess_vouched;
    f.estimates_due = estimates_due;
    f.plain_step = h->plain_step;
    return policy::plan_step(f);
}

// pc_apply in two stages.  The hand-off transitions keep their order -- enter_level in the head, end_pc_apply when the
// application ends, in finish or, for an application nobody will read, in abandon (as after a failed pc_apply: whatever the
// Krylov kernel in front handed over is dropped with it)
int pc_apply_begin(sns_ctx* h, const double* r, double* z, bool split) {
    if (h->pc_pending.open) { set_error("pc_apply_begin: the application before was not finished"); return SNS_E_STATE; }
    if (!split || !fine_plain_cycle(h)) {
        SNS_TRY(pc_apply(h, r, z));
        h->pc_pending = {};
        h->pc_pending.open = true;
        return SNS_OK;
    }
    sns_ctx::PendingCycle pc;
    pc.open = pc.cut = true;
    pc.b = r;
    pc.z = z;
    pc.x = fine_cycle_vector(h, z);
    const int rc = vcycle_head(h, 0, r, pc.x, &pc.cur, &pc.oth);
    if (rc != SNS_OK) {
        (void)h->handoff.end_pc_apply(false, z);
        return rc;
    }
    h->pc_pending = pc;
    return SNS_OK;
}

int pc_apply_finish(sns_ctx* h) {
    const sns_ctx::PendingCycle pc = h->pc_pending;
    h->pc_pending = {};
    if (!pc.open) { set_error("pc_apply_finish without pc_apply_begin"); return SNS_E_STATE; }
    if (!pc.cut) return SNS_OK;
    int rc = vcycle_tail(h, 0, pc.b, pc.cur, pc.oth);
    if (rc == SNS_OK && pc.x != pc.z) {
        if (hipMemcpyAsync(pc.z, pc.x, nred_of(h) * sizeof(double), hipMemcpyDeviceToDevice, h->stream) != hipSuccess) {
            set_error("pc_apply_finish: hipMemcpyAsync failed");
            rc = SNS_E_HIP;
        }
    }
    int level = -1;
    const bool legal = h->handoff.end_pc_apply(rc == SNS_OK, pc.z, &level);
    return rc != SNS_OK ? rc : handoff_legal(legal, "pc_apply ends with a carried put nobody took", level);
}

void pc_apply_abandon(sns_ctx* h) {
    const sns_ctx::PendingCycle pc = h->pc_pending;
    h->pc_pending = {};
    if (pc.open && pc.cut) (void)h->handoff.end_pc_apply(false, pc.z);
}


// operator apply with halo exchange (x must have room for the ghost tail)
int op_apply(sns_ctx* h, double* x, double* y) {
    SNS_TRY(exchange_and_spmv<SPMV_AX>(h, x, x, y, nullptr, 0.0, nullptr, false));
    h->tm.spmv_calls++;
    return SNS_OK;
}

// y = A x with the per-workgroup partial sums of <dotw, y> left in h->partial (BiCGStab's <rhat, A M p>)
int op_apply_dot(sns_ctx* h, double* x, double* y, const double* dotw) {
    SNS_TRY(exchange_and_spmv<SPMV_AX_DOT>(h, x, x, y, nullptr, 0.0, dotw, false));
    h->tm.spmv_calls++;
    return SNS_OK;
}

int op_residual(sns_ctx* h, double* x, const double* b, double* r) {
    SNS_TRY(exchange_and_spmv<SPMV_B_MINUS_AX>(h, x, x, r, b, 0.0, nullptr, false));
    h->tm.spmv_calls++;
    return SNS_OK;
}


}  // namespace sns
