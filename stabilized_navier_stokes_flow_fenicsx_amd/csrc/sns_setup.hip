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


int upload_pattern(Level& L, const HostPattern& P, DevBuf<int32_t>& slot_row, hipStream_t s) {
    L.n = P.n;
    L.nnzb = P.nnzb;
    SNS_TRY(L.rowptr.upload(P.rowptr));
    SNS_TRY(L.colind.upload(P.colind));
    SNS_TRY(L.diag.upload(P.diag));
    SNS_TRY(L.vals.alloc((size_t)P.nnzb * 16));
    SNS_TRY(L.dinv.alloc((size_t)P.n * 16));
    SNS_TRY(slot_row.alloc((size_t)P.nnzb));
    hipLaunchKernelGGL(k_fill_slot_row, dim3((P.n + 255) / 256), dim3(256), 0, s, P.n, L.rowptr, slot_row);
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


int append_level(sns_ctx* h, const HostPattern& P, int32_t n_owned, bool with_xg) {
    h->levels.emplace_back();
    h->slot_row.emplace_back();
    h->empty_c.emplace_back();
    h->pong.emplace_back();
    Level& C = h->levels.back();
    SNS_TRY(upload_pattern(C, P, h->slot_row.back(), h->stream));
    C.n_owned = n_owned;
    C.n_global = n_owned;                        // (append_level serves the replicated tail: every rank holds all rows)
    SNS_TRY(alloc_level_vectors(C));
    SNS_TRY(h->pong.back().alloc(4 * (size_t)std::max(1, C.n)));
    HIP_TRY(hipMemset(h->pong.back(), 0, 4 * (size_t)std::max(1, C.n) * sizeof(double)));
    if (with_xg) {
        SNS_TRY(C.xg.alloc(4 * (size_t)std::max(1, C.n)));
        HIP_TRY(hipMemset(C.xg, 0, 4 * (size_t)std::max(1, C.n) * sizeof(double)));
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

// Multi-GPU: from level R on, every rank holds the GLOBAL operator (values all-gathered at every numeric setup)
// and cycles the rest of the hierarchy redundantly: no exchanges below R, and the smoothing there is the exact
// global block-Jacobi instead of a rank-local one (thin partitions lose their convergence on the deep levels
// otherwise).  `cur` is the local pattern of level R (owned rows, local column ids), collective over the ranks.
int build_replicated_tail(sns_ctx* h, int R, const HostPattern& cur, int32_t n_owned, const std::vector<double>& cur_pts) {
    const sns_options& o = h->opt;
    Comm* c = h->comm.get();
    const int nr = c->nranks, me = c->rank;
    std::vector<double> cnt((size_t)2 * nr, 0.0);
    cnt[me] = (double)n_owned;
    cnt[nr + me] = (double)cur.rowptr[n_owned];
    SNS_TRY(global_sum(h, cnt.data(), 2 * nr));
    std::vector<int64_t> off((size_t)nr + 1, 0);
    int32_t maxn = 1;
    int64_t maxnz = 1;
    for (int r = 0; r < nr; ++r) {
        off[r + 1] = off[r] + (int64_t)cnt[r];
        maxn = std::max(maxn, (int32_t)cnt[r]);
        maxnz = std::max(maxnz, (int64_t)cnt[nr + r]);
    }
    const int32_t NG = (int32_t)off[nr];
    const std::vector<int32_t>& g_own = h->ghost_own[R];
    const std::vector<int32_t>& g_gid = h->ghost_gid[R];
    // [0, maxn): row lengths; [maxn, maxn + maxnz): global column ids of my slots
    std::vector<double> mine((size_t)maxn + (size_t)maxnz, -1.0), all;
    for (int32_t i = 0; i < maxn; ++i) mine[i] = i < n_owned ? (double)(cur.rowptr[i + 1] - cur.rowptr[i]) : 0.0;
    for (int32_t sidx = 0; sidx < cur.rowptr[n_owned]; ++sidx) {
        const int32_t j = cur.colind[sidx];
        int64_t gj;
        if (j < n_owned) gj = off[me] + j;
        else {
            const size_t q = (size_t)(j - n_owned);
            if (q >= g_own.size()) { set_error("replicated tail: ghost column without an owner record"); return SNS_E_STATE; }
            gj = off[g_own[q]] + g_gid[q];
        }
        mine[(size_t)maxn + sidx] = (double)gj;
    }
    SNS_TRY(host_allgather(h, mine, all));
    HostPattern G;
    G.n = NG;
    G.rowptr.assign((size_t)NG + 1, 0);
    std::vector<int32_t> valmap((size_t)nr * maxnz, -1), rowmap((size_t)std::max(1, NG), 0);
    const size_t LEN = mine.size();
    for (int r = 0; r < nr; ++r)
        for (int32_t i = 0; i < (int32_t)cnt[r]; ++i) {
            G.rowptr[(size_t)off[r] + i + 1] = (int32_t)all[r * LEN + i];
            rowmap[(size_t)off[r] + i] = r * maxn + i;
        }
    for (int32_t g = 0; g < NG; ++g) G.rowptr[g + 1] += G.rowptr[g];
    G.nnzb = G.rowptr[NG];
    G.colind.resize((size_t)G.nnzb);
    G.diag.assign((size_t)NG, 0);
    std::vector<std::pair<int32_t, int32_t>> ent;
    for (int r = 0; r < nr; ++r) {
        int64_t src = 0;
        for (int32_t i = 0; i < (int32_t)cnt[r]; ++i) {
            const int32_t g = (int32_t)off[r] + i;
            const int32_t len = (int32_t)all[r * LEN + i];
            ent.clear();
            for (int32_t k = 0; k < len; ++k, ++src)
                ent.emplace_back((int32_t)all[r * LEN + maxn + src], (int32_t)(r * maxnz + src));
            std::sort(ent.begin(), ent.end());
            bool has_diag = false;
            for (int32_t k = 0; k < len; ++k) {
                const int32_t slot = G.rowptr[g] + k;
                if (ent[k].first < 0 || ent[k].first >= NG || (k > 0 && ent[k].first == ent[k - 1].first)) {
                    set_error("replicated tail: inconsistent global pattern");
                    return SNS_E_STATE;
                }
                G.colind[slot] = ent[k].first;
                valmap[ent[k].second] = slot;
                if (ent[k].first == g) { G.diag[g] = slot; has_diag = true; }
            }
            if (!has_diag) { set_error("replicated tail: row without a diagonal block"); return SNS_E_STATE; }
        }
    }
    h->rep_level = (int)h->levels.size();
    h->rep_maxn = maxn;
    h->rep_maxnz = maxnz;
    h->rep_NG = NG;
    h->rep_off = (int32_t)off[me];
    {
        // window transports: the right-hand sides go straight to their rows of the replicated level (comm_allgatherv) ...
        std::vector<int64_t> doff((size_t)nr), dcnt((size_t)nr);
        for (int r = 0; r < nr; ++r) { doff[(size_t)r] = 4 * off[r]; dcnt[(size_t)r] = 4 * (int64_t)cnt[r]; }
        SNS_TRY(h->rep_doff.upload(doff));
        SNS_TRY(h->rep_dcnt.upload(dcnt));
        // ... and the level above the source reads the coarse solution of its fused correction + post-sweep straight from the
        // replicated solution: the columns of its M = A P (local ids of level R: owned, then ghosts) in the replicated level's ids
        Level& A = h->levels[R - 1];
        // (a rank without rows on that level uploads the empty list all the same: the plan asks whether it exists on every rank)
        if (R >= 2 && A.ap_colind) {
            std::vector<int32_t> col((size_t)A.ap_nnz);
            if (!col.empty()) HIP_TRY(hipMemcpy(col.data(), A.ap_colind, col.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            for (auto& j : col) {
                if (j < n_owned) j = (int32_t)off[me] + j;
                else {
                    const size_t q = (size_t)(j - n_owned);
                    if (q >= g_own.size()) { set_error("replicated tail: ghost aggregate without an owner record"); return SNS_E_STATE; }
                    j = (int32_t)off[g_own[q]] + g_gid[q];
                }
            }
            SNS_TRY(A.ap_colind_rep.upload(col));
        }
    }
    SNS_TRY(append_level(h, G, NG, false));
    h->ghost_own.emplace_back();
    h->ghost_gid.emplace_back();
    SNS_TRY(h->rep_valmap.upload(valmap));
    SNS_TRY(h->rep_rowmap.upload(rowmap));
    SNS_TRY(h->rep_vsend.alloc((size_t)maxnz * 16));
    SNS_TRY(h->rep_vrecv.alloc((size_t)maxnz * 16 * nr));
    SNS_TRY(h->rep_bsend.alloc((size_t)maxn * 4));
    SNS_TRY(h->rep_brecv.alloc((size_t)maxn * 4 * nr));
    HIP_TRY(hipMemset(h->rep_vsend, 0, (size_t)maxnz * 16 * sizeof(double)));
    HIP_TRY(hipMemset(h->rep_bsend, 0, (size_t)maxn * 4 * sizeof(double)));
    // the replicated level's node coordinates (all-gathered like its pattern), so that its aggregation sees shapes, not only numbers
    std::vector<double> gpts;
    {
        double have[1] = {cur_pts.size() == (size_t)3 * cur.n ? 0.0 : 1.0};
        SNS_TRY(global_sum(h, have, 1));
        if (have[0] == 0.0) {
            std::vector<double> pm((size_t)3 * maxn, 0.0), pa;
            for (int32_t i = 0; i < n_owned; ++i)
                for (int k = 0; k < 3; ++k) pm[3 * (size_t)i + k] = cur_pts[3 * (size_t)i + k];
            SNS_TRY(host_allgather(h, pm, pa));
            gpts.resize((size_t)3 * NG);
            for (int r = 0; r < nr; ++r)
                for (int32_t i = 0; i < (int32_t)cnt[r]; ++i)
                    for (int k = 0; k < 3; ++k) gpts[3 * ((size_t)off[r] + i) + k] = pa[(size_t)r * pm.size() + 3 * (size_t)i + k];
        }
    }
    // plain serial aggregation below (identical on every rank: same input, deterministic code)
    HostPattern curp = std::move(G);
    int32_t n_own = NG;
    for (int l = h->rep_level; (int)h->levels.size() < o.amg_max_levels + 1; ++l) {
        if (n_own <= policy::coarsest_rows(o)) break;
        std::vector<int32_t> agg;
        int32_t nc = 0;
        aggregate_nodes(curp, n_own, std::min(255, std::max(2, o.amg_agg_size)), agg, nc,
                        gpts.size() == (size_t)3 * n_own ? gpts.data() : nullptr);
        if (nc >= n_own || nc == 0) break;
        if (gpts.size() == (size_t)3 * n_own) {              // the next level's nodes: the aggregates' centroids
            std::vector<double> cp((size_t)3 * nc, 0.0);
            std::vector<int32_t> cn((size_t)nc, 0);
            for (int32_t i = 0; i < n_own; ++i) {
                const int32_t I = agg[i];
                if (I < 0) continue;
                for (int k = 0; k < 3; ++k) cp[3 * (size_t)I + k] += gpts[3 * (size_t)i + k];
                ++cn[I];
            }
            for (int32_t I = 0; I < nc; ++I)
                if (cn[I]) for (int k = 0; k < 3; ++k) cp[3 * (size_t)I + k] /= cn[I];
            gpts = std::move(cp);
        }
        HostAggregation A;
        build_coarse_from_agg(curp, n_own, agg, nc, nc, A);
        {
            Level& L = h->levels[l];
            L.nc = nc;
            SNS_TRY(L.agg.upload(A.agg));
            SNS_TRY(L.m_ptr.upload(A.m_ptr));
            SNS_TRY(L.m_idx.upload(A.m_idx));
            SNS_TRY(L.r_ptr.upload(A.r_ptr));
            SNS_TRY(L.r_idx.upload(A.r_idx));
            SNS_TRY(upload_block_rows(h, l, L, A.m_ptr, A.m_idx, nc));
            SNS_TRY(upload_ap(h, L, curp, n_own, A.agg));
        }
        SNS_TRY(append_level(h, A.coarse, nc, false));
        h->ghost_own.emplace_back();
        h->ghost_gid.emplace_back();
        curp = std::move(A.coarse);
        n_own = nc;
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

// Build the aggregation hierarchy (symbolic, once per mesh; collective over the ranks).
// Aggregates never cross ranks, but the Galerkin operators keep every cross-rank coupling:
// a ghost fine node's aggregate becomes a ghost coarse node, and each level gets its own
// halo plan derived from the finer one.  With one rank this is plain serial aggregation.
int build_hierarchy(sns_ctx* h, const HostPattern& fine) {
    const sns_options& o = h->opt;
    Comm* c = h->comm.get();
    const bool dist = c && c->active() && c->nranks > 1;
    HostPattern cur = fine;
    int32_t n_owned = h->n_owned;
    std::vector<double> cur_pts = h->dim == 3 ? std::move(h->host_pts) : std::vector<double>();   // coordinates of `cur`'s nodes (coarse: centroids)
    h->host_pts = std::vector<double>();
    h->fine_rematched_local = h->fine_rematched = false;
    {
        double ng[1] = {(double)h->n_owned};
        SNS_TRY(global_sum(h, ng, 1));
        h->n_global_fine = (int64_t)ng[0];
        h->n_global_l1 = 0;
        h->levels[0].n_global = h->n_global_fine;
    }
    h->ghost_gid.assign(1, {});
    h->ghost_own.assign(1, {});
    const int per_rank_coarse = dist ? std::max(1, o.amg_coarse_size / c->nranks) : o.amg_coarse_size;
    if (dist && !h->levels[0].xg) {
        SNS_TRY(h->levels[0].xg.alloc(4 * (size_t)h->levels[0].n));
        HIP_TRY(hipMemset(h->levels[0].xg, 0, 4 * (size_t)h->levels[0].n * sizeof(double)));
    }
    for (int l = 0; l + 1 < o.amg_max_levels; ++l) {
        if (dist && l >= 1 && o.amg_replicate_rows > 0) {
            double g[1] = {(double)n_owned};
            SNS_TRY(global_sum(h, g, 1));
            // the replicated level must fit the scratch vectors sized by the local fine level
            double fits[1] = {g[0] <= (double)h->n_owned ? 0.0 : 1.0};
            SNS_TRY(global_sum(h, fits, 1));
            if (policy::replicate_from(o, l, (int64_t)g[0], fits[0] == 0.0)) {
                SNS_TRY(build_replicated_tail(h, l, cur, n_owned, cur_pts));
                return plan_hierarchy(h);
            }
        }
        double flag[1] = {n_owned > per_rank_coarse ? 1.0 : 0.0};
        SNS_TRY(global_sum(h, flag, 1));
        if (flag[0] == 0.0) break;
        if (!dist && l >= 1 && n_owned <= policy::coarsest_rows(o)) break;       // serial: this level is solved directly
        std::vector<int32_t> agg;
        int32_t nc_owned = 0;
        const double* pts = cur_pts.size() == (size_t)3 * cur.n ? cur_pts.data() : nullptr;
        if (l == 0 && o.amg_aggregation >= 1) {
            SNS_TRY(aggregate_fine_by_strength(h, cur, pts, agg, nc_owned));
        } else {
            aggregate_nodes(cur, n_owned, std::min(255, std::max(2, o.amg_agg_size)), agg, nc_owned, pts);
        }
        if (l == 0) h->agg0 = agg;
        // (+ whether the hybrid re-matched level-0 nodes of some rank: the fine level's blocks below are uploaded on every rank or none)
        double prog[3] = {(double)n_owned, (double)nc_owned, (l == 0 && h->fine_rematched_local) ? 1.0 : 0.0};
        SNS_TRY(global_sum(h, prog, 3));
        if (l == 0) h->fine_rematched = prog[2] > 0.0;
        if (prog[1] >= prog[0] || prog[1] == 0.0) break;      // no progress anywhere
        if (l == 0) h->n_global_l1 = (int64_t)prog[1];
        int32_t nc_total = nc_owned;
        Plan cplan;
        std::vector<int32_t> g_own, g_gid;                     // ghost coarse nodes: owner rank, owner-local id
        Level& L = h->levels[l];
        if (dist) {
            const Plan& p = c->plans[l];
            std::vector<double> ids((size_t)4 * cur.n, -1.0);
            for (int32_t i = 0; i < n_owned; ++i) ids[(size_t)4 * i] = (double)agg[i];
            HIP_TRY(hipMemcpy(L.xg, ids.data(), ids.size() * sizeof(double), hipMemcpyHostToDevice));
            SNS_TRY(comm_exchange(c, p, L.xg, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
            HIP_TRY(hipMemcpy(ids.data(), L.xg, ids.size() * sizeof(double), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemset(L.xg, 0, ids.size() * sizeof(double)));
            cplan.nbr = p.nbr;
            cplan.n_own = nc_owned;
            cplan.send_ptr.assign(1, 0);
            cplan.recv_ptr.assign(1, 0);
            for (size_t k = 0; k < p.nbr.size(); ++k) {
                std::vector<int32_t> u;
                for (int32_t q = p.recv_ptr[k]; q < p.recv_ptr[k + 1]; ++q) {
                    const int32_t rid = (int32_t)ids[(size_t)4 * p.h_recv_idx[q]];
                    if (rid < 0) { set_error("hierarchy: ghost node without an aggregate on its owner"); return SNS_E_COMM; }
                    u.push_back(rid);
                }
                std::sort(u.begin(), u.end());
                u.erase(std::unique(u.begin(), u.end()), u.end());
                for (int32_t q = p.recv_ptr[k]; q < p.recv_ptr[k + 1]; ++q) {
                    const int32_t gnode = p.h_recv_idx[q];
                    const int32_t rid = (int32_t)ids[(size_t)4 * gnode];
                    agg[gnode] = nc_total + (int32_t)(std::lower_bound(u.begin(), u.end(), rid) - u.begin());
                }
                for (size_t q = 0; q < u.size(); ++q) {
                    cplan.h_recv_idx.push_back(nc_total + (int32_t)q);
                    g_own.push_back(p.nbr[k]);
                    g_gid.push_back(u[q]);
                }
                nc_total += (int32_t)u.size();
                cplan.recv_ptr.push_back((int32_t)cplan.h_recv_idx.size());
                std::vector<int32_t> sset;
                for (int32_t q = p.send_ptr[k]; q < p.send_ptr[k + 1]; ++q) sset.push_back(agg[p.h_send_idx[q]]);
                std::sort(sset.begin(), sset.end());
                sset.erase(std::unique(sset.begin(), sset.end()), sset.end());
                cplan.h_send_idx.insert(cplan.h_send_idx.end(), sset.begin(), sset.end());
                cplan.send_ptr.push_back((int32_t)cplan.h_send_idx.size());
            }
        }
        HostAggregation A;
        build_coarse_from_agg(cur, n_owned, agg, nc_owned, nc_total, A);
        L.nc = nc_owned;
        SNS_TRY(L.agg.upload(A.agg));
        SNS_TRY(L.m_ptr.upload(A.m_ptr));
        SNS_TRY(L.m_idx.upload(A.m_idx));
        SNS_TRY(L.r_ptr.upload(A.r_ptr));
        SNS_TRY(L.r_idx.upload(A.r_idx));
        SNS_TRY(upload_block_rows(h, l, L, A.m_ptr, A.m_idx, nc_owned));
        // M = A P for the fused first post-smoothing sweep: every level of a serial hierarchy; in a partitioned one the fine
        // level only (its single post-sweep is the exact global sweep; the distributed coarse levels smooth rank-locally)
        // ... and, on the window transports, every partitioned level: the exact-sweep cycle (plan exact) takes the fused post-sweep too
        if (!dist || l == 0 || c->windows()) SNS_TRY(upload_ap(h, L, cur, n_owned, A.agg));
        h->levels.emplace_back();
        h->slot_row.emplace_back();
        h->empty_c.emplace_back();
        h->pong.emplace_back();
        Level& C = h->levels.back();
        if (&h->levels[l] != &L) { set_error("internal: level storage moved"); return SNS_E_STATE; }
        SNS_TRY(upload_pattern(C, A.coarse, h->slot_row.back(), h->stream));
        C.n_owned = nc_owned;
        C.n_global = (int64_t)prog[1];
        SNS_TRY(alloc_level_vectors(C));
        SNS_TRY(h->pong.back().alloc(4 * (size_t)C.n));
        HIP_TRY(hipMemset(h->pong.back(), 0, 4 * (size_t)C.n * sizeof(double)));
        if (dist) {
            SNS_TRY(C.xg.alloc(4 * (size_t)C.n));
            HIP_TRY(hipMemset(C.xg, 0, 4 * (size_t)C.n * sizeof(double)));
            SNS_TRY(check_plan_symmetry(h, cplan, l + 1));
            SNS_TRY(plan_upload(cplan));
            SNS_TRY(connect_plan(h, cplan));
            c->plans.push_back(std::move(cplan));
        }
        h->ghost_own.push_back(std::move(g_own));
        h->ghost_gid.push_back(std::move(g_gid));
        if (l == 0) {
            SNS_TRY(h->empty_c[0].alloc(4 * (size_t)std::max(1, nc_owned)));
            if (nc_owned > 0)
                hipLaunchKernelGGL(k_empty_coarse, dim3((unsigned)((4 * (int64_t)nc_owned + 255) / 256)), dim3(256), 0,
                                   h->stream, nc_owned, L.m_ptr, L.m_idx, L.free_mask, h->empty_c[0]);
        }
        if (cur_pts.size() == (size_t)3 * cur.n) {
            std::vector<double> cp((size_t)3 * nc_total, 0.0), cnt((size_t)nc_total, 0.0);
            for (int32_t i = 0; i < cur.n; ++i) {
                const int32_t I = A.agg[(size_t)i];
                if (I < 0) continue;
                for (int c3 = 0; c3 < 3; ++c3) cp[3 * (size_t)I + c3] += cur_pts[3 * (size_t)i + c3];
                cnt[(size_t)I] += 1.0;
            }
            for (int32_t I = 0; I < nc_total; ++I)
                if (cnt[(size_t)I] > 0.0) for (int c3 = 0; c3 < 3; ++c3) cp[3 * (size_t)I + c3] /= cnt[(size_t)I];
            cur_pts = std::move(cp);
        } else {
            cur_pts.clear();
        }
        cur = std::move(A.coarse);
        n_owned = nc_owned;
    }
    Level& last = h->levels.back();
    if (h->levels.size() > 1) {
        if (!dist) {
            SNS_TRY(alloc_coarsest_solver(h, last));
        } else {
            // global dense coarsest solve, replicated on every rank: rank r's node i -> padded id r*maxn + i
            std::vector<double> cnt(c->nranks, 0.0);
            cnt[c->rank] = (double)last.n_owned;
            SNS_TRY(global_sum(h, cnt.data(), c->nranks));
            int maxn = 0;
            h->cg_counts.resize(c->nranks);
            for (int r = 0; r < c->nranks; ++r) { h->cg_counts[r] = (int)cnt[r]; maxn = std::max(maxn, (int)cnt[r]); }
            const int N = 4 * c->nranks * std::max(1, maxn);
            if (N <= policy::DISTRIBUTED_DENSE_MAX_DOFS) {
                h->cg_maxn = std::max(1, maxn);
                h->cg_N = N;
                std::vector<int32_t> cmap((size_t)last.n, 0);
                for (int32_t i = 0; i < last.n_owned; ++i) cmap[i] = c->rank * h->cg_maxn + i;
                const auto& go = h->ghost_own.back();
                const auto& gg = h->ghost_gid.back();
                for (size_t q = 0; q < go.size(); ++q) cmap[(size_t)last.n_owned + q] = go[q] * h->cg_maxn + gg[q];
                SNS_TRY(h->cg_colmap.upload(cmap));
                SNS_TRY(h->cg_rows.alloc((size_t)4 * h->cg_maxn * N));
                SNS_TRY(h->cg_full.alloc((size_t)N * N));
                SNS_TRY(h->cg_send.alloc((size_t)4 * h->cg_maxn));
                SNS_TRY(h->cg_recv.alloc((size_t)N));
                SNS_TRY(h->d_piv.alloc((size_t)N));
            }
        }
    }
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
                       h->slot_row[l + 1], C.colind, (l == 0) ? h->empty_c[0] : (const uint8_t*)nullptr, L.m_ptr, C.vals);
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
        hipLaunchKernelGGL(k_bsr_to_dense_ld, dim3((unsigned)((nth + 255) / 256)), dim3(256), 0, h->stream, L.nnzb, h->slot_row[l],
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


int pc_setup(sns_ctx* h) {
    if (!h->has_matrix) { set_error("pc_setup before a matrix was assembled"); return SNS_E_STATE; }
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    const int nl = (h->opt.pc_type == SNS_PC_AMG) ? (int)h->levels.size() : 1;
    bool any_block = false;
    const bool new_operator = policy::new_operator(h->matrix_key, h->est_key, h->r3_estimates);
    for (int l = 0; l < nl; ++l) {
        Level& L = h->levels[l];
        if (h->rep_level > 0 && l == h->rep_level - 1) {
            SNS_TRY(refresh_replicated_source(h, L));
            continue;
        }
        const policy::LevelPlan& P = h->plan.level[(size_t)l];
        const bool not_last = l + 1 < nl;
        SNS_TRY(refresh_smoother_inverses(h, P, L));
        if (P.blocks) any_block = true;
        SNS_TRY(refresh_low_precision_copies(h, P, L, not_last));
        SNS_TRY(damping_decide(h, l, nl, new_operator));
        if (not_last) {
            SNS_TRY(refresh_ap32(h, P, L));
            refresh_galerkin(h, l);
        } else if (nl > 1) {
            SNS_TRY(refresh_coarsest_solver(h, l));
        }
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
