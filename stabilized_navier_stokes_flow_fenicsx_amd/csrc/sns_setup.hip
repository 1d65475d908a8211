// Setup side of the C-ABI layer: the symbolic AMG hierarchy (aggregation, halo plans per level, replicated tail), the numeric
// setup of the preconditioner as a list of stages and the workspace vectors.  (The smoother damping: csrc/sns_damping.hip.)
// (shared internals in csrc/sns_ctx.h)
#include "sns_ctx.h"

namespace sns {

int alloc_level_vectors(Level& L) {
    const size_t nd = 4 * (size_t)L.n;
    SNS_TRY(L.x.alloc(nd));
    SNS_TRY(L.b.alloc(nd));
    SNS_TRY(L.r.alloc(nd));
    HIP_TRY(hipMemset(L.x, 0, nd * sizeof(double)));
    HIP_TRY(hipMemset(L.b, 0, nd * sizeof(double)));
    HIP_TRY(hipMemset(L.r, 0, nd * sizeof(double)));
    return SNS_OK;
}


int upload_pattern(Level& L, const HostPattern& P, hipStream_t s) {
    L.n = P.n;
    L.nnzb = P.nnzb;
    SNS_TRY(L.rowptr.upload(P.rowptr));
    SNS_TRY(L.colind.upload(P.colind));
    SNS_TRY(L.diag.upload(P.diag));
    SNS_TRY(L.vals.alloc((size_t)P.nnzb * 16));
    SNS_TRY(L.dinv.alloc((size_t)P.n * 16));
    SNS_TRY(L.slot_row.alloc((size_t)P.nnzb));
    hipLaunchKernelGGL(k_fill_slot_row, dim3((P.n + 255) / 256), dim3(256), 0, s, P.n, L.rowptr, L.slot_row);
    return SNS_OK;
}


// global sums of a few host doubles (collective; identity without a communicator)
int global_sum(sns_ctx* h, double* v, int count) {
    Comm* c = h->comm.get();
    if (!c || !c->active() || c->nranks <= 1) return SNS_OK;
    HIP_TRY(hipMemcpy(h->d_scal + 64, v, count * sizeof(double), hipMemcpyHostToDevice));
    SNS_TRY(comm_allreduce_sum(c, h->d_scal + 64, count, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    SNS_TRY(peer_check(c));
    HIP_TRY(hipMemcpy(v, h->d_scal + 64, count * sizeof(double), hipMemcpyDeviceToHost));
    return SNS_OK;
}


// host-side all-gather of `mine` (same length on every rank) through the communicator
int host_allgather(sns_ctx* h, const std::vector<double>& mine, std::vector<double>& all) {
    Comm* c = h->comm.get();
    const size_t len = mine.size();
    DevBuf<double> ds, dr;
    SNS_TRY(ds.alloc(len));
    SNS_TRY(dr.alloc(len * c->nranks));
    HIP_TRY(hipMemcpy(ds, mine.data(), len * sizeof(double), hipMemcpyHostToDevice));
    SNS_TRY(comm_allgather(c, ds, dr, (int)len, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    SNS_TRY(peer_check(c));
    all.resize(len * c->nranks);
    HIP_TRY(hipMemcpy(all.data(), dr, all.size() * sizeof(double), hipMemcpyDeviceToHost));
    return SNS_OK;
}


// Every link of a halo plan must be posted by BOTH ends with matching counts -- rank a sends s nodes to b <=> b receives s nodes
// from a, zero included: comm_exchange posts no ncclSend / ncclRecv for an empty direction, so the peer must not post the matching
// call either.  An asymmetric plan deadlocks RCCL where the team transport only reports an error, so every level's plan is checked
// when it is made (hierarchy build, collective): one all-gather of 2 * nranks counts per rank, and every rank reaches the same
// verdict from the same table, i.e. a bad plan ends the run on all ranks instead of hanging some of them.
int check_plan_symmetry(sns_ctx* h, const Plan& p, int level) {
    Comm* c = h->comm.get();
    if (!c || !c->active() || c->nranks <= 1) return SNS_OK;
    const int nr = c->nranks;
    std::vector<double> mine((size_t)2 * nr, 0.0), all;
    bool bad_peer = p.send_ptr.size() != p.nbr.size() + 1 || p.recv_ptr.size() != p.nbr.size() + 1;
    for (size_t k = 0; k < p.nbr.size() && !bad_peer; ++k) {
        const int peer = p.nbr[k];
        if (peer < 0 || peer >= nr || peer == c->rank) { bad_peer = true; break; }
        mine[(size_t)peer] += (double)(p.send_ptr[k + 1] - p.send_ptr[k]);
        mine[(size_t)nr + peer] += (double)(p.recv_ptr[k + 1] - p.recv_ptr[k]);
    }
    if (bad_peer) mine[(size_t)c->rank] = -1.0;                 // (a rank never sends to itself: the slot doubles as the error flag)
    SNS_TRY(host_allgather(h, mine, all));
    for (int a = 0; a < nr; ++a) {
        if (all[(size_t)a * 2 * nr + a] != 0.0) {
            set_error("halo plan of level " + std::to_string(level) + ": rank " + std::to_string(a) + " lists an invalid neighbour");
            return SNS_E_COMM;
        }
        for (int b = 0; b < nr; ++b) {
            const double sent = all[(size_t)a * 2 * nr + b], expected = all[(size_t)b * 2 * nr + nr + a];
            if (sent != expected) {
                set_error("halo plan of level " + std::to_string(level) + " is asymmetric: rank " + std::to_string(a) + " sends " +
                          std::to_string((long long)sent) + " nodes to rank " + std::to_string(b) + ", which expects " +
                          std::to_string((long long)expected));
                return SNS_E_COMM;
            }
        }
    }
    return SNS_OK;
}


// peer transport: wire an uploaded plan to the neighbours' windows (collective, like check_plan_symmetry before it)
int connect_plan(sns_ctx* h, Plan& p) {
    Comm* c = h->comm.get();
    if (!c || !c->peer) return SNS_OK;
    PlanOffers t;
    const int rc = peer_plan_offer(c, p, t);
    if (rc != SNS_OK) t.mine.assign((size_t)3 * c->nranks + 1, -2.0);  // (still take part in the all-gather: the peers must not hang)
    SNS_TRY(host_allgather(h, t.mine, t.all));
    if (rc != SNS_OK) return rc;
    for (double v : t.all)
        if (v == -2.0) { set_error("peer transport: a rank could not place the plan in its window"); return SNS_E_COMM; }
    return peer_plan_connect(c, p, t);
}


// Append a level with the pattern P (rows [0, n_owned) owned; n_global: its rows over all ranks): operator arrays, work vectors,
// the ping-pong buffer and, with_xg, the exchanged copy of the iterate.  pong and xg hold 4 * max(1, n) doubles on every path
// (a partitioned level of a rank with no row and no ghost on it used to get one double where the replicated tail gave four).
// The only place that appends to h->levels after level 0; a std::deque: no reference to a finer level moves.
static int append_level(sns_ctx* h, const HostPattern& P, int32_t n_owned, int64_t n_global, bool with_xg) {
    h->levels.emplace_back();
    Level& C = h->levels.back();
    SNS_TRY(upload_pattern(C, P, h->stream));
    C.n_owned = n_owned;
    C.n_global = n_global;
    SNS_TRY(alloc_level_vectors(C));
    const size_t nd = 4 * (size_t)std::max(1, C.n);
    SNS_TRY(C.pong.alloc(nd));
    HIP_TRY(hipMemset(C.pong, 0, nd * sizeof(double)));
    if (with_xg) {
        SNS_TRY(C.xg.alloc(nd));
        HIP_TRY(hipMemset(C.xg, 0, nd * sizeof(double)));
    }
    return SNS_OK;
}


int upload_block_rows(sns_ctx* h, int l, Level& L, const std::vector<int32_t>& m_ptr, const std::vector<int32_t>& m_idx,
                      int32_t nc_owned) {
    const int mode = h->opt.amg_block_smooth;
    if (mode <= 0 || nc_owned < 0) return SNS_OK;
    // (the fine level: runs before the hierarchy's plan exists; global counts only, every rank answers alike)
    const Comm* c = h->comm.get();
    if (l == 0 && !policy::fine_blocks(h->opt, (c && c->active()) ? c->nranks : 1, h->n_global_fine, h->fine_rematched)) return SNS_OK;
    // blocks = aggregates; an aggregate of more than 8 nodes (a leftover node joined a full neighbour) is split in member order
    std::vector<int32_t> rows, of((size_t)std::max(1, L.n), -1);
    rows.reserve((size_t)8 * std::max(1, nc_owned));
    int32_t nb = 0;
    for (int32_t G = 0; G < nc_owned; ++G) {
        const int32_t k0 = m_ptr[(size_t)G], k1 = m_ptr[(size_t)G + 1];
        for (int32_t k = k0; k < k1; k += 8) {
            for (int32_t q = 0; q < 8; ++q) {
                const int32_t node = (k + q < k1) ? m_idx[(size_t)k + q] : -1;
                rows.push_back(node);
                if (node >= 0) of[(size_t)node] = nb;
            }
            ++nb;
        }
    }
    if (rows.empty()) rows.assign(8, -1);
    L.n_blk = nb;
    SNS_TRY(L.blk_rows.upload(rows));
    SNS_TRY(L.blk_of.upload(of));
    return SNS_OK;
}

// symbolic part of M = A P of a level (fused first post-smoothing sweep, k_post_lp): pattern + gather lists -> device
// (a rank WITHOUT owned rows uploads the empty pattern all the same: whether a level takes the fused post-sweep -- one level-(l+1)
// exchange -- or the prolongation + level-l halo is decided from these arrays, and every rank must take the same branch)
int upload_ap(sns_ctx* h, Level& L, const HostPattern& fine, int32_t n_rows, const std::vector<int32_t>& agg_all) {
    if (n_rows < 0) n_rows = 0;
    HostAP M;
    try {
        build_ap_pattern(fine, n_rows, agg_all, M);
    } catch (const std::exception& e) {
        set_error(e.what());
        return SNS_E_MESH;
    }
    L.ap_nnz = M.nnz;
    SNS_TRY(L.ap_rowptr.upload(M.rowptr));
    SNS_TRY(L.ap_colind.upload(M.colind));
    SNS_TRY(L.ap_ptr.upload(M.ap_ptr));
    SNS_TRY(L.ap_idx.upload(M.ap_idx));
    SNS_TRY(L.ap_nib.upload(M.nib));
    return SNS_OK;
}


// The coarsest level's direct solve: <= max(amg_coarse_size, 40) nodes take the one-workgroup inverse with partial pivoting of
// rounds 1-3, up to amg_dense_rows nodes the blocked Gauss-Jordan inverse on the matrix cores (csrc/sns_dense.hip); a larger
// last level (amg_max_levels reached) is smoothed.
int alloc_coarsest_solver(sns_ctx* h, Level& last) {
    const sns_options& o = h->opt;
    const policy::CoarsestKind ck = policy::coarsest_kind(o, last.n);
    if (ck == policy::COARSEST_SMALL_INVERSE) {
        const size_t N = 4 * (size_t)last.n;
        SNS_TRY(last.dense_inv.alloc(N * N));
        SNS_TRY(h->d_piv.alloc(N));
    } else if (ck == policy::COARSEST_BLOCKED_INVERSE) {
        const int Np = (4 * last.n + 63) / 64 * 64;
        last.dense_np = Np;
        SNS_TRY(last.dense_gj.alloc((size_t)Np * Np));
        SNS_TRY(last.dense_work.alloc(dense_gj_work_doubles(Np)));
        SNS_TRY(last.dense_x32.alloc((size_t)Np * Np));
    }
    return SNS_OK;
}

// ... and of a hierarchy that ends partitioned: the global dense inverse, replicated on every rank (rank r's node i -> padded id
// r * maxn + i; `ghosts`: the owners of the last level's ghost nodes).  Collective: one global sum.  Too large: smoothed.
static int alloc_distributed_coarsest_solver(sns_ctx* h, Level& last, const GhostIds& ghosts) {
    const Comm* c = h->comm.get();
    std::vector<double> cnt(c->nranks, 0.0);
    cnt[c->rank] = (double)last.n_owned;
    SNS_TRY(global_sum(h, cnt.data(), c->nranks));
    int maxn = 0;
    h->cg_counts.resize(c->nranks);
    for (int r = 0; r < c->nranks; ++r) { h->cg_counts[r] = (int)cnt[r]; maxn = std::max(maxn, (int)cnt[r]); }
    const int N = 4 * c->nranks * std::max(1, maxn);
    if (N > policy::DISTRIBUTED_DENSE_MAX_DOFS) return SNS_OK;
    h->cg_maxn = std::max(1, maxn);
    h->cg_N = N;
    std::vector<int32_t> cmap((size_t)last.n, 0);
    for (int32_t i = 0; i < last.n_owned; ++i) cmap[i] = c->rank * h->cg_maxn + i;
    for (size_t q = 0; q < ghosts.own.size(); ++q) cmap[(size_t)last.n_owned + q] = ghosts.own[q] * h->cg_maxn + ghosts.gid[q];
    SNS_TRY(h->cg_colmap.upload(cmap));
    SNS_TRY(h->cg_rows.alloc((size_t)4 * h->cg_maxn * N));
    SNS_TRY(h->cg_full.alloc((size_t)N * N));
    SNS_TRY(h->cg_send.alloc((size_t)4 * h->cg_maxn));
    SNS_TRY(h->cg_recv.alloc((size_t)N));
    SNS_TRY(h->d_piv.alloc((size_t)N));
    return SNS_OK;
}


// ---- the stages of the symbolic build: build_hierarchy and build_replicated_tail below call them in this order ------------------
// The level being coarsened, carried from one step to the next and owned by the build: its local pattern (owned rows, then
// empty ghost rows), its nodes' coordinates (coarse levels: the aggregates' centroids; empty: none, as in 2-D) and the owners of
// its ghost nodes.
struct Front {
    HostPattern cur;
    int32_t n_owned = 0;
    std::vector<double> pts;
    GhostIds ghosts;
    const double* points() const { return pts.size() == (size_t)3 * cur.n ? pts.data() : nullptr; }
};

static int agg_size(const sns_options& o) { return std::min(255, std::max(2, o.amg_agg_size)); }

// One coarsening step on the device: the transfer arrays of level l (pattern `f.cur`) from its aggregation A, its smoother blocks
// and M = A P, then the coarse level appended (append_level).  Beside level 0 these two functions are the only place that fills or
// appends a Level.  What differs between the callers is said by them:
//   n_global  the coarse level's rows over all ranks (a replicated level: its own rows);
//   with_ap   M = A P for the fused post-sweep: every level of a serial hierarchy and of the replicated tail; of the partitioned
//             levels the fine one (its single post-sweep is the exact global sweep, the coarse ones smooth rank-locally) and, on
//             the window transports, all of them (the exact-sweep cycle takes the fused post-sweep too);
//   with_xg   the coarse level is partitioned: it exchanges halos.
static int add_next_level(sns_ctx* h, int l, const Front& f, const HostAggregation& A, int64_t n_global, bool with_ap, bool with_xg) {
    Level& L = h->levels[l];
    L.nc = A.nc;
    SNS_TRY(L.agg.upload(A.agg));
    SNS_TRY(L.m_ptr.upload(A.m_ptr));
    SNS_TRY(L.m_idx.upload(A.m_idx));
    SNS_TRY(L.r_ptr.upload(A.r_ptr));
    SNS_TRY(L.r_idx.upload(A.r_idx));
    SNS_TRY(upload_block_rows(h, l, L, A.m_ptr, A.m_idx, A.nc));
    if (with_ap) SNS_TRY(upload_ap(h, L, f.cur, f.n_owned, A.agg));
    return append_level(h, A.coarse, A.nc, n_global, with_xg);
}

// carry the front forward: the coarse pattern, its nodes (the aggregates' centroids) and the owners of its ghosts
static void advance(Front& f, HostAggregation& A, GhostIds&& ghosts) {
    const double* pts = f.points();
    f.pts = pts ? aggregate_centroids(pts, f.cur.n, A.agg, A.coarse.n) : std::vector<double>();
    f.cur = std::move(A.coarse);
    f.n_owned = A.nc;
    f.ghosts = std::move(ghosts);
}

// the ranks' shares of the source level (collective: one global sum of 2 * nranks counts)
static int agree_replicated_layout(sns_ctx* h, const Front& f, ReplicatedLayout& lay) {
    const Comm* c = h->comm.get();
    const int nr = c->nranks;
    std::vector<double> cnt((size_t)2 * nr, 0.0);
    cnt[c->rank] = (double)f.n_owned;
    cnt[nr + c->rank] = (double)f.cur.rowptr[f.n_owned];
    SNS_TRY(global_sum(h, cnt.data(), 2 * nr));
    lay = replicated_layout(nr, cnt.data());
    return SNS_OK;
}

// the global pattern from every rank's rows (collective: one all-gather -- which a rank with a bad ghost record does not reach)
static int gather_replicated_pattern(sns_ctx* h, const Front& f, const ReplicatedLayout& lay, HostPattern& G,
                                     std::vector<int32_t>& valmap, std::vector<int32_t>& rowmap) {
    std::vector<double> mine, all;
    SNS_TRY(replicated_record(lay, h->comm->rank, f.cur, f.n_owned, f.ghosts, mine));
    SNS_TRY(host_allgather(h, mine, all));
    return replicated_pattern(lay, all, G, valmap, rowmap);
}

// What the cycle knows of the replicated level R, appended next.  Window transports: the right-hand sides go straight to their
// rows of it (comm_allgatherv: rep_doff / rep_dcnt), and the level above the source reads the coarse solution of its fused
// correction + post-sweep straight from the replicated solution: the columns of its M = A P (local ids of the source level:
// owned, then ghosts) in the replicated level's ids.
static int record_replicated_level(sns_ctx* h, int R, const Front& f, const ReplicatedLayout& lay) {
    const int nr = h->comm->nranks, me = h->comm->rank;
    h->rep_level = (int)h->levels.size();
    h->rep_maxn = lay.maxn;
    h->rep_maxnz = lay.maxnz;
    h->rep_NG = lay.NG;
    h->rep_off = (int32_t)lay.off[me];
    std::vector<int64_t> doff((size_t)nr), dcnt((size_t)nr);
    for (int r = 0; r < nr; ++r) { doff[(size_t)r] = 4 * lay.off[r]; dcnt[(size_t)r] = 4 * (int64_t)lay.rows[r]; }
    SNS_TRY(h->rep_doff.upload(doff));
    SNS_TRY(h->rep_dcnt.upload(dcnt));
    Level& A = h->levels[R - 1];
    // (a rank without rows on that level uploads the empty list all the same: the plan asks whether it exists on every rank)
    if (R < 2 || !A.ap_colind) return SNS_OK;
    std::vector<int32_t> col((size_t)A.ap_nnz);
    if (!col.empty()) HIP_TRY(hipMemcpy(col.data(), A.ap_colind, col.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (auto& j : col) {
        const int64_t g = replicated_id(lay, me, f.n_owned, f.ghosts, j);
        if (g < 0) { set_error("replicated tail: ghost aggregate without an owner record"); return SNS_E_STATE; }
        j = (int32_t)g;
    }
    return A.ap_colind_rep.upload(col);
}

// the buffers the numeric set-up and the cycle move the source level's values and right-hand sides through
static int alloc_replicated_transfer(sns_ctx* h, const ReplicatedLayout& lay, const std::vector<int32_t>& valmap,
                                     const std::vector<int32_t>& rowmap) {
    const size_t nr = (size_t)h->comm->nranks, maxn = (size_t)lay.maxn, maxnz = (size_t)lay.maxnz;
    SNS_TRY(h->rep_valmap.upload(valmap));
    SNS_TRY(h->rep_rowmap.upload(rowmap));
    SNS_TRY(h->rep_vsend.alloc(maxnz * 16));
    SNS_TRY(h->rep_vrecv.alloc(maxnz * 16 * nr));
    SNS_TRY(h->rep_bsend.alloc(maxn * 4));
    SNS_TRY(h->rep_brecv.alloc(maxn * 4 * nr));
    HIP_TRY(hipMemset(h->rep_vsend, 0, maxnz * 16 * sizeof(double)));
    HIP_TRY(hipMemset(h->rep_bsend, 0, maxn * 4 * sizeof(double)));
    return SNS_OK;
}

// the replicated level's node coordinates, all-gathered like its pattern, so that its aggregation sees shapes, not only numbers
// (collective: a global sum, and the all-gather where every rank has coordinates); empty: none
static int gather_replicated_points(sns_ctx* h, const Front& f, const ReplicatedLayout& lay, std::vector<double>& gpts) {
    gpts.clear();
    double have[1] = {f.points() ? 0.0 : 1.0};
    SNS_TRY(global_sum(h, have, 1));
    if (have[0] != 0.0) return SNS_OK;
    std::vector<double> pm((size_t)3 * lay.maxn, 0.0), pa;
    for (int32_t i = 0; i < f.n_owned; ++i)
        for (int k = 0; k < 3; ++k) pm[3 * (size_t)i + k] = f.pts[3 * (size_t)i + k];
    SNS_TRY(host_allgather(h, pm, pa));
    gpts.resize((size_t)3 * lay.NG);
    for (size_t r = 0; r < lay.rows.size(); ++r)
        for (int32_t i = 0; i < lay.rows[r]; ++i)
            for (int k = 0; k < 3; ++k) gpts[3 * ((size_t)lay.off[r] + i) + k] = pa[r * pm.size() + 3 * (size_t)i + k];
    return SNS_OK;
}

// Multi-GPU: from level R on, every rank holds the GLOBAL operator (values all-gathered at every numeric setup)
// and cycles the rest of the hierarchy redundantly: no exchanges below R, and the smoothing there is the exact
// global block-Jacobi instead of a rank-local one (thin partitions lose their convergence on the deep levels
// otherwise).  `src` is the front at level R, the source of the copy: levels[R + 1] becomes the replicated level.  Collective.
static int build_replicated_tail(sns_ctx* h, int R, const Front& src) {
    const sns_options& o = h->opt;
    ReplicatedLayout lay;
    SNS_TRY(agree_replicated_layout(h, src, lay));
    Front f;                                                  // the replicated level: every row owned, no ghosts
    std::vector<int32_t> valmap, rowmap;
    SNS_TRY(gather_replicated_pattern(h, src, lay, f.cur, valmap, rowmap));
    SNS_TRY(record_replicated_level(h, R, src, lay));
    SNS_TRY(append_level(h, f.cur, lay.NG, lay.NG, false));
    SNS_TRY(alloc_replicated_transfer(h, lay, valmap, rowmap));
    SNS_TRY(gather_replicated_points(h, src, lay, f.pts));
    f.n_owned = lay.NG;
    // plain serial aggregation below (identical on every rank: same input, deterministic code)
    for (int l = h->rep_level; (int)h->levels.size() < o.amg_max_levels + 1; ++l) {
        if (f.n_owned <= policy::coarsest_rows(o)) break;
        std::vector<int32_t> agg;
        int32_t nc = 0;
        aggregate_nodes(f.cur, f.n_owned, agg_size(o), agg, nc, f.points());
        if (nc >= f.n_owned || nc == 0) break;
        HostAggregation A;
        build_coarse_from_agg(f.cur, f.n_owned, agg, nc, nc, A);
        SNS_TRY(add_next_level(h, l, f, A, nc, true, false));
        advance(f, A, GhostIds());
    }
    SNS_TRY(alloc_coarsest_solver(h, h->levels.back()));
    h->tm.amg_levels = (int)h->levels.size() - 1;
    return SNS_OK;
}


// Level 0 aggregated by operator strength: the strength of the assembled fine operator (csrc/sns_strength.hip) and aggregate_strength
// over the owned nodes -- amg_aggregation = 1: the strength copied to the host and sns_host.cpp's matcher; 2: the same map built on
// the device (csrc/sns_aggregate.hip), only the map copied; 3: the geometric map of amg_aggregation = 0 (`pts`: the node
// coordinates or null, as 0 passes them), re-matched by strength on the device only where it cuts a dominant coupling
// (h->fine_rematched_local).  The fp32 strength and the device scratch are local.
static int aggregate_fine_by_strength(sns_ctx* h, const HostPattern& fine, const double* pts, std::vector<int32_t>& agg, int32_t& nc) {
    const Level& L = h->levels[0];
    if (!h->has_matrix) {
        set_error("amg_aggregation = " + std::to_string(h->opt.amg_aggregation) + ": the hierarchy is built from the assembled operator; assemble first");
        return SNS_E_STATE;
    }
    const int max_agg = std::min(h->opt.amg_agg_size, policy::STRENGTH_MAX_AGG);
    if (h->opt.amg_aggregation == 3) {
        std::vector<int32_t> g;
        int32_t ng = 0;
        aggregate_nodes(fine, h->n_owned, std::min(255, std::max(2, h->opt.amg_agg_size)), g, ng, pts);
        return aggregate_hybrid_device(h, max_agg, g, ng, agg, nc, h->fine_rematched_local);
    }
    if (h->opt.amg_aggregation == 2) return aggregate_strength_device(h, max_agg, agg, nc);
    DevBuf<float> s_dev;
    DevBuf<double> scale;
    SNS_TRY(s_dev.alloc((size_t)L.nnzb));
    SNS_TRY(scale.alloc(4 * (size_t)L.n));
    SNS_TRY(compute_strength(h, s_dev, scale));
    std::vector<float> s((size_t)L.nnzb);
    if (L.nnzb > 0 && hipMemcpyAsync(s.data(), s_dev, s.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream) != hipSuccess) {
        set_error("amg_aggregation = 1: copy of the strength to the host failed");
        return SNS_E_HIP;
    }
    if (hipStreamSynchronize(h->stream) != hipSuccess) { set_error("amg_aggregation = 1: strength kernel failed"); return SNS_E_HIP; }
    aggregate_strength(fine, h->n_owned, std::min(h->opt.amg_agg_size, policy::STRENGTH_MAX_AGG), s.data(), agg, nc);
    return SNS_OK;
}

// the front at the fine level, the fine rows over all ranks (collective: one global sum) and level 0's exchanged vector
static int start_front(sns_ctx* h, const HostPattern& fine, bool dist, Front& f) {
    f.cur = fine;
    f.n_owned = h->n_owned;
    f.pts = h->dim == 3 ? std::move(h->host_pts) : std::vector<double>();
    h->host_pts = std::vector<double>();
    h->fine_rematched_local = h->fine_rematched = false;
    double ng[1] = {(double)h->n_owned};
    SNS_TRY(global_sum(h, ng, 1));
    h->n_global_fine = (int64_t)ng[0];
    h->n_global_l1 = 0;
    Level& L0 = h->levels[0];
    L0.n_global = h->n_global_fine;
    if (dist && !L0.xg) {
        SNS_TRY(L0.xg.alloc(4 * (size_t)L0.n));
        HIP_TRY(hipMemset(L0.xg, 0, 4 * (size_t)L0.n * sizeof(double)));
    }
    return SNS_OK;
}

// partitioned, l >= 1, amg_replicate_rows > 0: do the ranks hand level l over to the replicated tail?  (collective: two global sums)
static int agree_replication(sns_ctx* h, bool dist, int l, int32_t n_owned, bool& replicate) {
    replicate = false;
    if (!(dist && l >= 1 && h->opt.amg_replicate_rows > 0)) return SNS_OK;
    double g[1] = {(double)n_owned};
    SNS_TRY(global_sum(h, g, 1));
    // the replicated level must fit the scratch vectors sized by the local fine level
    double fits[1] = {g[0] <= (double)h->n_owned ? 0.0 : 1.0};
    SNS_TRY(global_sum(h, fits, 1));
    replicate = policy::replicate_from(h->opt, l, (int64_t)g[0], fits[0] == 0.0);
    return SNS_OK;
}

// does any rank have more rows than a coarsest level may (collective: one global sum)?  Serial: level l >= 1 is solved directly
// as soon as the coarsest solver takes it
static int agree_more_levels(sns_ctx* h, bool dist, int l, int32_t n_owned, bool& more) {
    const sns_options& o = h->opt;
    const int per_rank_coarse = dist ? std::max(1, o.amg_coarse_size / h->comm->nranks) : o.amg_coarse_size;
    double flag[1] = {n_owned > per_rank_coarse ? 1.0 : 0.0};
    SNS_TRY(global_sum(h, flag, 1));
    more = flag[0] != 0.0 && !(!dist && l >= 1 && n_owned <= policy::coarsest_rows(o));
    return SNS_OK;
}

// aggregate the owned nodes of level l (agg: -1 at the ghost nodes) and agree on the outcome (collective: one global sum):
// nc_global aggregates over all ranks; progress: fewer than there were nodes, and not none
static int aggregate_level(sns_ctx* h, int l, const Front& f, std::vector<int32_t>& agg, int32_t& nc_owned, int64_t& nc_global,
                           bool& progress) {
    nc_owned = 0;
    if (l == 0 && h->opt.amg_aggregation >= 1) {
        SNS_TRY(aggregate_fine_by_strength(h, f.cur, f.points(), agg, nc_owned));
    } else {
        aggregate_nodes(f.cur, f.n_owned, agg_size(h->opt), agg, nc_owned, f.points());
    }
    if (l == 0) h->agg0 = agg;
    // (+ whether the hybrid re-matched level-0 nodes of some rank: the fine level's blocks are uploaded on every rank or none)
    double prog[3] = {(double)f.n_owned, (double)nc_owned, (l == 0 && h->fine_rematched_local) ? 1.0 : 0.0};
    SNS_TRY(global_sum(h, prog, 3));
    if (l == 0) h->fine_rematched = prog[2] > 0.0;
    nc_global = (int64_t)prog[1];
    progress = !(prog[1] >= prog[0] || prog[1] == 0.0);
    if (l == 0 && progress) h->n_global_l1 = nc_global;
    return SNS_OK;
}

// Partitioned levels: the aggregate of every ghost node on its owner, through level l's exchange (the ids ride in the first
// component of xg, which is left zero again), and from them the coarse level's halo lists, its ghosts' owners and the ghost
// entries of agg (coarse_halo_lists, csrc/sns_host.cpp).
static int exchange_aggregate_ids(sns_ctx* h, int l, const Front& f, int32_t nc_owned, std::vector<int32_t>& agg, Plan& cplan,
                                  GhostIds& cghosts, int32_t& nc_total) {
    Comm* c = h->comm.get();
    Level& L = h->levels[l];
    std::vector<double> ids((size_t)4 * f.cur.n, -1.0);
    for (int32_t i = 0; i < f.n_owned; ++i) ids[(size_t)4 * i] = (double)agg[i];
    HIP_TRY(hipMemcpy(L.xg, ids.data(), ids.size() * sizeof(double), hipMemcpyHostToDevice));
    SNS_TRY(comm_exchange(c, c->plans[l], L.xg, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(ids.data(), L.xg, ids.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(L.xg, 0, ids.size() * sizeof(double)));
    std::vector<int32_t> owner_agg((size_t)f.cur.n);
    for (int32_t i = 0; i < f.cur.n; ++i) owner_agg[(size_t)i] = (int32_t)ids[(size_t)4 * i];
    return coarse_halo_lists(c->plans[l], owner_agg, nc_owned, agg, cplan, cghosts, nc_total);
}

// the plan of the level just appended: checked, uploaded, wired to the neighbours' windows (collective: check_plan_symmetry's
// all-gather and, on the peer transport, connect_plan's) and handed to the communicator
static int attach_plan(sns_ctx* h, Plan& cplan, int level) {
    SNS_TRY(check_plan_symmetry(h, cplan, level));
    SNS_TRY(plan_upload(cplan));
    SNS_TRY(connect_plan(h, cplan));
    h->comm->plans.push_back(std::move(cplan));
    return SNS_OK;
}

// levels[0].empty_c: per aggregate of the fine level and component, the members a Dirichlet condition keeps out of the transfer
static int flag_empty_aggregates(sns_ctx* h) {
    Level& L = h->levels[0];
    SNS_TRY(L.empty_c.alloc(4 * (size_t)std::max(1, L.nc)));
    if (L.nc > 0)
        hipLaunchKernelGGL(k_empty_coarse, dim3((unsigned)((4 * (int64_t)L.nc + 255) / 256)), dim3(256), 0, h->stream, L.nc, L.m_ptr,
                           L.m_idx, L.free_mask, L.empty_c);
    return SNS_OK;
}

// Build the aggregation hierarchy (symbolic, once per mesh; collective over the ranks).
// Aggregates never cross ranks, but the Galerkin operators keep every cross-rank coupling:
// a ghost fine node's aggregate becomes a ghost coarse node, and each level gets its own
// halo plan derived from the finer one.  With one rank this is plain serial aggregation.
// Every rank walks the same stages and so the same collectives: each `break` and the hand-over are decided from agreed values.
int build_hierarchy(sns_ctx* h, const HostPattern& fine) {
    Comm* c = h->comm.get();
    const bool dist = c && c->active() && c->nranks > 1;
    Front f;
    SNS_TRY(start_front(h, fine, dist, f));
    for (int l = 0; l + 1 < h->opt.amg_max_levels; ++l) {
        bool replicate = false, more = false, progress = false;
        SNS_TRY(agree_replication(h, dist, l, f.n_owned, replicate));
        if (replicate) {
            SNS_TRY(build_replicated_tail(h, l, f));
            return plan_hierarchy(h);
        }
        SNS_TRY(agree_more_levels(h, dist, l, f.n_owned, more));
        if (!more) break;
        std::vector<int32_t> agg;
        int32_t nc_owned = 0;
        int64_t nc_global = 0;
        SNS_TRY(aggregate_level(h, l, f, agg, nc_owned, nc_global, progress));
        if (!progress) break;                                  // no progress anywhere
        int32_t nc_total = nc_owned;
        Plan cplan;
        GhostIds cghosts;                                      // ghost coarse nodes: owner rank, owner-local id
        if (dist) SNS_TRY(exchange_aggregate_ids(h, l, f, nc_owned, agg, cplan, cghosts, nc_total));
        HostAggregation A;
        build_coarse_from_agg(f.cur, f.n_owned, agg, nc_owned, nc_total, A);
        SNS_TRY(add_next_level(h, l, f, A, nc_global, !dist || l == 0 || c->windows(), dist));
        if (dist) SNS_TRY(attach_plan(h, cplan, l + 1));
        if (l == 0) SNS_TRY(flag_empty_aggregates(h));
        advance(f, A, std::move(cghosts));
    }
    Level& last = h->levels.back();
    if (h->levels.size() > 1) SNS_TRY(dist ? alloc_distributed_coarsest_solver(h, last, f.ghosts) : alloc_coarsest_solver(h, last));
    h->tm.amg_levels = (int)h->levels.size();
    return plan_hierarchy(h);
}


// The plan of the cycle for the hierarchy just built (collective, once per hierarchy): its structure, the two per-rank facts agreed
// over the ranks -- a level's plans receive in order straight into the windows on EVERY rank; the most owned rows of any rank --,
// the switches SNS_TEAM_OVERLAP / SNS_NO_CARRIED_PUT, then csrc/sns_policy.h.  Every rank runs the same cycle whatever its ghost numbering or share.
int plan_hierarchy(sns_ctx* h) {
    const Comm* c = h->comm.get();
    const int nl = (int)h->levels.size();
    policy::Facts& f = h->facts;
    f = policy::Facts();
    f.nranks = (c && c->active()) ? std::max(1, c->nranks) : 1;
    f.rep_level = h->rep_level;
    f.rows_global_l1 = h->n_global_l1;
    f.windows = c && c->windows();
    f.team_overlap = h->team_overlap;
    f.fuse_puts = std::getenv("SNS_NO_CARRIED_PUT") == nullptr;
    const Level& last = h->levels.back();
    f.last = last.dense_gj ? policy::COARSEST_BLOCKED_INVERSE
                           : (last.dense_inv || h->cg_N > 0) ? policy::COARSEST_SMALL_INVERSE : policy::COARSEST_SWEEPS;
    f.rep_gather_fits = h->rep_level > 0 && c && c->peer && h->levels[h->rep_level].n_blk > 0 &&
                        (size_t)4 * h->rep_maxn * (size_t)c->nranks <= c->peer->ag_doubles;
    // per level: window-capable, owned rows; last: the hybrid re-matched level-0 nodes of this rank
    std::vector<double> mine((size_t)2 * nl + 1), all;
    mine[(size_t)2 * nl] = h->fine_rematched_local ? 1.0 : 0.0;
    for (int l = 0; l < nl; ++l) {
        const Level& L = h->levels[l];
        f.rows.push_back(L.n_global);
        f.has_blocks.push_back(L.blk_rows != nullptr);
        f.has_ap.push_back(L.ap_rowptr != nullptr);
        f.has_ap_rep.push_back(L.ap_colind_rep != nullptr);
        const bool wc = c && (size_t)l < c->plans.size() && c->plans[l].identity_recv && c->plans[l].win_recv[0] != nullptr;
        mine[(size_t)l] = wc ? 1.0 : 0.0;
        mine[(size_t)nl + l] = (double)L.n_owned;
    }
    if (f.nranks > 1) SNS_TRY(host_allgather(h, mine, all));
    else all = mine;
    f.win_capable.assign((size_t)nl, 1);
    f.max_owned.assign((size_t)nl, 0);
    for (size_t r = 0; r < all.size() / mine.size(); ++r) {
        if (all[r * mine.size() + 2 * (size_t)nl] != 0.0) f.fine_rematched = true;
        for (int l = 0; l < nl; ++l) {
            if (all[r * mine.size() + l] == 0.0) f.win_capable[(size_t)l] = 0;
            f.max_owned[(size_t)l] = std::max(f.max_owned[(size_t)l], (int64_t)all[r * mine.size() + nl + l]);
        }
    }
    h->plan = policy::plan_cycle(h->opt, f);
    return SNS_OK;
}


// ---- the stages of the numeric set-up: what pc_setup refreshes per level, in the order it calls them -----------------------------
// the level above the replicated tail is only the source of the copy: all-gather my rows' blocks, scatter them into place
static int refresh_replicated_source(sns_ctx* h, const Level& L) {
    Level& C = h->levels[h->rep_level];
    if (L.nnzb > 0)
        HIP_TRY(hipMemcpyAsync(h->rep_vsend, L.vals, (size_t)L.nnzb * 16 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    SNS_TRY(comm_allgather(h->comm.get(), h->rep_vsend, h->rep_vrecv, (int)(h->rep_maxnz * 16), h->stream));
    const int64_t nsrc = h->rep_maxnz * h->comm->nranks;
    hipLaunchKernelGGL(k_scatter_blocks, dim3((unsigned)((nsrc * 8 + 255) / 256)), dim3(256), 0, h->stream, nsrc, h->rep_valmap,
                       h->rep_vrecv, C.vals);
    return SNS_OK;
}

// the smoother's inverses: the nodal D^-1 and, where the plan smooths with them, the aggregates' inverse diagonal blocks
static int refresh_smoother_inverses(sns_ctx* h, const policy::LevelPlan& P, Level& L) {
    const int32_t rows = L.n_owned;
    if (rows > 0) hipLaunchKernelGGL(k_dinv, dim3((rows + 255) / 256), dim3(256), 0, h->stream, rows, L.diag, L.vals, L.dinv);
    if (!P.blocks) return SNS_OK;
    // from the fp64 operator (what the nodal D^-1 is to the point smoother), in the format of the level's matrix copy (fp32, or
    // fp16 with row scales: half the bytes of a block sweep's extra stream)
    const int bf = h->opt.amg_f32_matrix == 2 ? 2 : 1;
    if (!L.binv32 || L.binv_fmt != bf) {
        SNS_TRY(L.binv32.alloc(binv_bytes_per_block(bf) * (size_t)std::max(1, L.n_blk)));
        L.binv_fmt = bf;
    }
    if (L.n_blk > 0)
        with_fmt(bf, [&](auto F) {
            hipLaunchKernelGGL((k_binv<F>), dim3((unsigned)((L.n_blk + 7) / 8)), dim3(256), 0, h->stream, L.n_blk, L.blk_rows,
                               L.blk_of, L.rowptr, L.colind, L.vals, L.binv32, h->d_sing);
        });
    return SNS_OK;
}

// the low-precision copies the smoother reads: D^-1 as fp32, the operator as fp16 (with the fp16 M = A P of a level that has
// one) or as fp32
static int refresh_low_precision_copies(sns_ctx* h, const policy::LevelPlan& P, Level& L, bool not_last) {
    if (P.lp_fmt == 0) return SNS_OK;
    const int32_t rows = L.n_owned;
    if (!L.dinv32) SNS_TRY(L.dinv32.alloc((size_t)16 * std::max(1, L.n)));
    if (rows > 0)
        hipLaunchKernelGGL(k_cvt_f32, dim3(vec_grid(16 * (int64_t)rows)), dim3(256), 0, h->stream, 16 * (int64_t)rows, L.dinv,
                           L.dinv32);
    if (h->opt.amg_f32_matrix == 2) {
        if (!L.vals16) {
            SNS_TRY(L.vals16.alloc(std::max<size_t>(1, (size_t)L.nnzb * 4) * sizeof(uint2)));
            SNS_TRY(L.scale16.alloc((size_t)4 * std::max(1, L.n)));
        }
        // ONE pass over the level's fp64 operator writes its fp16 copy and, where the level has one, the fp16 copy of
        // M = A P for the fused post-smoothing sweep (k_lp_copies16)
        const bool with_m = not_last && L.ap_rowptr && L.ap_nib && h->opt.amg_fused_post;
        if (with_m && !L.ap_vals16) {
            SNS_TRY(L.ap_vals16.alloc(std::max<size_t>(1, (size_t)L.ap_nnz * 4) * sizeof(uint2)));
            SNS_TRY(L.ap_scale16.alloc((size_t)4 * std::max(1, L.n)));
        }
        if (rows > 0) {
            const unsigned grid = (unsigned)((rows + 31) / 32);
            if (with_m)
                hipLaunchKernelGGL((k_lp_copies16<1>), dim3(grid), dim3(128), 0, h->stream, rows, L.rowptr, L.vals,
                                   (uint2*)L.vals16.get(), L.scale16, L.ap_rowptr, L.ap_colind, L.ap_ptr, L.ap_idx, L.ap_nib, L.agg,
                                   L.free_mask, (uint2*)L.ap_vals16.get(), L.ap_scale16);
            else
                hipLaunchKernelGGL((k_lp_copies16<0>), dim3(grid), dim3(128), 0, h->stream, rows, L.rowptr, L.vals,
                                   (uint2*)L.vals16.get(), L.scale16, (const int32_t*)nullptr, (const int32_t*)nullptr,
                                   (const int32_t*)nullptr, (const int32_t*)nullptr, (const uint64_t*)nullptr,
                                   (const int32_t*)nullptr, (const uint8_t*)nullptr, (uint2*)nullptr, (float*)nullptr);
        }
    }
    if (h->opt.amg_f32_matrix != 2) {
        if (!L.vals32) SNS_TRY(L.vals32.alloc((size_t)L.nnzb * 16));
        if (L.nnzb > 0)
            hipLaunchKernelGGL(k_cvt_f32, dim3(vec_grid(L.nnzb * 16)), dim3(256), 0, h->stream, L.nnzb * 16, L.vals, L.vals32);
    }
    return SNS_OK;
}

// numeric part of M = A P, straight into the level's low-precision format (no fp64 copy of M; fp16: written together with the
// fp16 copy of A above).  (Allocated on a rank without rows too: the plan asks for it on every rank.)
static int refresh_ap32(sns_ctx* h, const policy::LevelPlan& P, Level& L) {
    if (!(L.ap_rowptr && h->opt.amg_fused_post && P.lp_fmt == 1)) return SNS_OK;
    const int32_t rows = L.n_owned;
    if (!L.ap_vals32) SNS_TRY(L.ap_vals32.alloc((size_t)L.ap_nnz * 16));
    if (rows > 0)
        hipLaunchKernelGGL(k_ap_cvt32, dim3((unsigned)((4 * (int64_t)rows + 255) / 256)), dim3(256), 0, h->stream, rows,
                           L.ap_rowptr, L.ap_colind, L.ap_ptr, L.ap_idx, L.vals, L.agg, L.free_mask, (float4*)L.ap_vals32.get());
    return SNS_OK;
}

// the Galerkin product: the operator of level l + 1 from level l's
static void refresh_galerkin(sns_ctx* h, int l) {
    const Level& L = h->levels[l];
    Level& C = h->levels[l + 1];
    const int64_t nth = C.nnzb * 8;
    hipLaunchKernelGGL(k_galerkin, dim3((unsigned)((nth + 255) / 256)), dim3(256), 0, h->stream, C.nnzb, L.r_ptr, L.r_idx, L.vals,
                       C.slot_row, C.colind, (l == 0) ? L.empty_c.get() : (const uint8_t*)nullptr, L.m_ptr, C.vals);
}

// the last level's direct solve, whichever the hierarchy was built with (alloc_coarsest_solver, build_hierarchy); none: smoothed
static int refresh_coarsest_solver(sns_ctx* h, int l) {
    Level& L = h->levels[l];
    if (h->cg_N > 0) {
        // distributed coarsest level: my rows of the GLOBAL dense matrix -> all-gather -> replicated inverse
        const int N = h->cg_N, mr = 4 * h->cg_maxn;
        HIP_TRY(hipMemsetAsync(h->cg_rows, 0, (size_t)mr * N * sizeof(double), h->stream));
        const int64_t nth = L.nnzb * 16;
        if (nth > 0)
            hipLaunchKernelGGL(k_bsr_to_dense_map, dim3((unsigned)((nth + 255) / 256)), dim3(256), 0, h->stream, L.n_owned,
                               L.rowptr, L.colind, L.vals, h->cg_colmap, N, h->cg_rows);
        // padding rows (ranks with fewer nodes than maxn) get a unit diagonal
        hipLaunchKernelGGL(k_pad_identity, dim3(1), dim3(256), 0, h->stream, 4 * L.n_owned, mr, h->comm->rank * mr, N, h->cg_rows);
        SNS_TRY(comm_allgather(h->comm.get(), h->cg_rows, h->cg_full, mr * N, h->stream));
        hipLaunchKernelGGL(k_dense_inverse, dim3(1), dim3(1024), 0, h->stream, N, h->cg_full, h->d_piv, h->d_sing);
    } else if (L.dense_gj) {
        // blocked Gauss-Jordan inverse on the fp64 matrix cores, then its fp32 copy for the cycle's matvec
        const int N = 4 * L.n, Np = L.dense_np;
        HIP_TRY(hipMemsetAsync(L.dense_gj, 0, (size_t)Np * Np * sizeof(double), h->stream));
        const int64_t nth = L.nnzb * 16;
        hipLaunchKernelGGL(k_bsr_to_dense_ld, dim3((unsigned)((nth + 255) / 256)), dim3(256), 0, h->stream, L.nnzb, L.slot_row,
                           L.colind, L.vals, Np, L.dense_gj);
        if (Np > N) hipLaunchKernelGGL(k_dense_pad_diag, dim3((Np - N + 255) / 256), dim3(256), 0, h->stream, N, Np, L.dense_gj);
        // (the two-stream schedule of dense_gj_inverse is opt-in: measured, it is SLOWER -- 3.9 against 2.4 ms at N = 1900 --
        // because the bulk update's 900 workgroups fill the chip and the pivot chain's few workgroups queue behind them)
        if (!h->gj_stream && std::getenv("SNS_GJ_TWO_STREAMS") &&
            hipStreamCreateWithFlags(h->gj_stream.put(), hipStreamNonBlocking) != hipSuccess) h->gj_stream.reset();
        dense_gj_inverse(h->stream, h->gj_stream, Np, L.dense_gj, L.dense_work, h->d_sing);
        const int64_t nn = (int64_t)Np * Np;
        hipLaunchKernelGGL(k_dense_to_f32, dim3((unsigned)((nn / 4 + 255) / 256)), dim3(256), 0, h->stream, nn, L.dense_gj, L.dense_x32);
    } else if (L.dense_inv) {
        const int N = 4 * L.n;
        HIP_TRY(hipMemsetAsync(L.dense_inv, 0, (size_t)N * N * sizeof(double), h->stream));
        const int64_t nth = L.nnzb * 16;
        hipLaunchKernelGGL(k_bsr_to_dense, dim3((unsigned)((nth + 255) / 256)), dim3(256), 0, h->stream, L.n, L.rowptr, L.colind,
                           L.vals, L.dense_inv);
        hipLaunchKernelGGL(k_dense_inverse, dim3(1), dim3(1024), 0, h->stream, N, L.dense_inv, h->d_piv, h->d_sing);
    }
    return SNS_OK;
}

// The end of a set-up, the stream drained and the singularity flag `sing` fetched: the verdict on the dense inverses over all
// ranks, then the put groups of the peer transport.
static int conclude_setup(sns_ctx* h, int nl, bool check_sing, int sing) {
    if (check_sing) {
        // The aggregate blocks' inverses are rank-local: one rank alone returning an error here would leave the others in the
        // Krylov loop's collectives (an RCCL hang, a peer time-out).  The verdict is taken over all ranks.
        double bad[1] = {sing != 0 ? 1.0 : 0.0};
        SNS_TRY(global_sum(h, bad, 1));
        if (bad[0] != 0.0) {
            // (the elimination runs without pivoting across its 64 x 64 blocks: see csrc/sns_dense.hip for why that is safe on this
            // operator class; if it ever is not, say so instead of preconditioning with garbage -- there is no fallback hierarchy)
            HIP_TRY(hipMemset(h->d_sing, 0, sizeof(int)));
            set_error("AMG setup: a dense inverse (coarsest level or an aggregate block" +
                      std::string(sing != 0 ? "" : ", on another rank") + ") met a zero or non-finite pivot; set "
                      "amg_dense_rows = 0 / amg_block_smooth = 0");
            return SNS_E_STATE;
        }
    }
    if (h->comm && h->comm->peer && h->opt.pc_type == SNS_PC_AMG)
        for (int l = 0; l < nl && l < (int)h->comm->plans.size(); ++l) {
            const Level& L = h->levels[l];
            if (L.blk_rows && L.n_blk > 0 && L.binv32)        // the puts carried by this level's block kernels (comm_put_dst)
                SNS_TRY(comm_plan_put_groups(h->comm.get(), h->comm->plans[l], L.blk_rows, 8 * L.n_blk, h->stream));
        }
    return SNS_OK;
}


// the stream and the events of the two-stream set-up, made once per handle: non-blocking, at the greatest priority the device
// offers -- the chain's few workgroups must not queue behind the bulk passes' (what made SNS_GJ_TWO_STREAMS slower)
static int setup_chain_ready(sns_ctx* h, int nl) {
    if (!h->setup_stream) {
        int least = 0, greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(hipStreamCreateWithPriority(h->setup_stream.put(), hipStreamNonBlocking, greatest));
        HIP_TRY(hipEventCreateWithFlags(h->ev_setup_fork.put(), hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(h->ev_setup_join.put(), hipEventDisableTiming));
    }
    while ((int)h->ev_setup_level.size() < nl) {
        h->ev_setup_level.emplace_back();
        HIP_TRY(hipEventCreateWithFlags(h->ev_setup_level.back().put(), hipEventDisableTiming));
    }
    return SNS_OK;
}

// One stream: per level its smoother inverses, low-precision copies, damping, M = A P, then the Galerkin product into the next
// (the last level: its direct solve).  Two streams (policy::plan_step; no estimates due, so that the damping is host arithmetic):
// the chain -- every Galerkin product, the last level's solver -- on h->setup_stream, the rest on the handle's stream, a level
// >= 1 after the product that wrote its operator; joined before the singularity flag is read.
int pc_setup(sns_ctx* h) {
    if (!h->has_matrix) { set_error("pc_setup before a matrix was assembled"); return SNS_E_STATE; }
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    const int nl = (h->opt.pc_type == SNS_PC_AMG) ? (int)h->levels.size() : 1;
    bool any_block = false;
    const bool new_operator = policy::new_operator(h->matrix_key, h->est_key, h->r3_estimates);
    bool estimates_due = false;
    for (int l = 0; l < nl; ++l) estimates_due = estimates_due || damping_estimates_due(h, l, nl, new_operator);
    const bool two = step_plan(h, false, estimates_due).setup_two_streams;
    hipStream_t const user = h->stream;
    // (the chain's launches go through the same stage functions: they launch on h->stream)
    struct OnChain {
        sns_ctx* h;
        hipStream_t user;
        OnChain(sns_ctx* hh, bool two) : h(hh), user(hh->stream) { if (two) h->stream = h->setup_stream; }
        ~OnChain() { h->stream = user; }
    };
    if (two) {
        SNS_TRY(setup_chain_ready(h, nl));
        HIP_TRY(hipEventRecord(h->ev_setup_fork, user));
        HIP_TRY(hipStreamWaitEvent(h->setup_stream, h->ev_setup_fork, 0));
    }
    for (int l = 0; l < nl; ++l) {
        Level& L = h->levels[l];
        if (h->rep_level > 0 && l == h->rep_level - 1) {
            SNS_TRY(refresh_replicated_source(h, L));
            continue;
        }
        const policy::LevelPlan& P = h->plan.level[(size_t)l];
        const bool not_last = l + 1 < nl;
        if (two && l >= 1) HIP_TRY(hipStreamWaitEvent(user, h->ev_setup_level[(size_t)l], 0));
        SNS_TRY(refresh_smoother_inverses(h, P, L));
        if (P.blocks) any_block = true;
        SNS_TRY(refresh_low_precision_copies(h, P, L, not_last));
        SNS_TRY(damping_decide(h, l, nl, new_operator));
        if (not_last) {
            SNS_TRY(refresh_ap32(h, P, L));
            OnChain chain(h, two);
            refresh_galerkin(h, l);
            if (two) HIP_TRY(hipEventRecord(h->ev_setup_level[(size_t)l + 1], h->setup_stream));
        } else if (nl > 1) {
            OnChain chain(h, two);
            SNS_TRY(refresh_coarsest_solver(h, l));
        }
    }
    if (two) {
        HIP_TRY(hipEventRecord(h->ev_setup_join, h->setup_stream));
        HIP_TRY(hipStreamWaitEvent(user, h->ev_setup_join, 0));
    }
    if (const char* miss = plan_buffer_missing(h)) {
        set_error(std::string("AMG setup: the cycle's plan needs ") + miss + ", which the setup did not allocate");
        return SNS_E_STATE;
    }
    ++h->pc_setups;
    h->est_key = h->matrix_key;
    const bool check_sing = nl > 1 && (h->levels[nl - 1].dense_gj != nullptr || any_block);
    int* h_sing = reinterpret_cast<int*>(h->h_scal + 768);
    *h_sing = 0;
    if (check_sing) HIP_TRY(hipMemcpyAsync(h_sing, h->d_sing, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    h->tm.pc_setup_ms += ms;
    HIP_TRY(hipGetLastError());
    SNS_TRY(conclude_setup(h, nl, check_sing, *h_sing));
    h->pc_ready = true;
    return SNS_OK;
}


// The device buffers the cycle reads because its plan says so (nullptr: all there).  pc_setup allocates them from the same plan;
// after sns_set_options a changed plan may ask for one it has not made yet.
const char* plan_buffer_missing(const sns_ctx* h) {
    if (h->opt.pc_type != SNS_PC_AMG) return nullptr;
    for (size_t l = 0; l < h->plan.level.size() && l < h->levels.size(); ++l) {
        const policy::LevelPlan& P = h->plan.level[l];
        const Level& L = h->levels[l];
        if (P.blocks && (!L.binv32 || L.binv_fmt != (P.lp_fmt == 2 ? 2 : 1))) return "a level's aggregate-block inverses";
        if (P.lp_fmt != 0 && (!L.dinv32 || !(P.lp_fmt == 2 ? (const void*)L.vals16 : (const void*)L.vals32)))
            return "a level's low-precision matrix copy";
        if (P.fused_post && !(P.lp_fmt == 2 ? (const void*)L.ap_vals16 : (const void*)L.ap_vals32)) return "a level's M = A P";
    }
    return nullptr;
}


int get_vec(sns_ctx* h, size_t k, double** out) {
    while (h->kv.size() <= k) {
        DevBuf<double> p;
        SNS_TRY(p.alloc((size_t)ld_of(h)));
        HIP_TRY(hipMemset(p, 0, (size_t)ld_of(h) * sizeof(double)));
        h->kv.push_back(std::move(p));
    }
    *out = h->kv[k];
    return SNS_OK;
}

}  // namespace sns
