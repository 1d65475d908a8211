// The host index logic of the distributed hierarchy build (csrc/sns_host.cpp: aggregate_centroids, coarse_halo_lists,
// replicated_layout / _id / _record / _pattern) on N simulated ranks in one process: a Kuhn box with shuffled node numbering is
// split over the ranks, every rank gets its local pattern and halo lists, aggregates with aggregate_nodes, and the ghost nodes'
// aggregate ids travel by copying along the lists the way comm_exchange moves them (the k-th node sent is the k-th received).
// Checked per case, over two coarsening steps and a replication of every front:
//   * exact equality with the loops as they stood inline in build_hierarchy / build_replicated_tail before the functions
//     existed (the ref_* functions below are transcribed from that code);
//   * what the exchange relies on: per link the k-th aggregate sent is the k-th ghost received, counts match both ways, the
//     receive lists are n_own + q in order, and every ghost coarse node is the aggregate its fine members have on their owner;
//   * the replicated pattern: valmap a bijection of the non-padding gathered slots onto G's slots, columns sorted and unique,
//     diag at the diagonal, G equal to the union of the local rows relabelled directly;
//   * the error returns.
// Built with -fsanitize=address,undefined by tests/test_host.py; prints "ERROR ..." and exits 1 where a check fails.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "sns_internal.h"

static std::string g_err;
namespace sns { void set_error(const std::string& s) { g_err = s; } }
using namespace sns;

#define CHECK(cond, what)                                                             \
    do {                                                                              \
        if (!(cond)) { std::printf("ERROR line %d (%s): %s\n", __LINE__, what, #cond); return 1; } \
    } while (0)

struct Rank {                                    // a rank's front: the level it coarsens next
    HostPattern cur;
    int32_t n_owned = 0;
    std::vector<double> pts;                     // 3 per local node
    HaloLists p;
    GhostIds ghosts;
    std::vector<int32_t> agg;                    // this step's aggregate map
    int32_t nc_owned = 0;
};

// ---- the parent's loops, transcribed -------------------------------------------------------------------------------------------
// build_hierarchy, "if (dist) { ... }": ids = the exchanged vector (4 doubles per node, the id in the first)
static int ref_coarse_plan(const HaloLists& p, const std::vector<double>& ids, int32_t nc_owned, std::vector<int32_t>& agg,
                           HaloLists& cplan, std::vector<int32_t>& g_own, std::vector<int32_t>& g_gid, int32_t& nc_total) {
    nc_total = nc_owned;
    cplan.nbr = p.nbr;
    cplan.n_own = nc_owned;
    cplan.send_ptr.assign(1, 0);
    cplan.recv_ptr.assign(1, 0);
    for (size_t k = 0; k < p.nbr.size(); ++k) {
        std::vector<int32_t> u;
        for (int32_t q = p.recv_ptr[k]; q < p.recv_ptr[k + 1]; ++q) {
            const int32_t rid = (int32_t)ids[(size_t)4 * p.h_recv_idx[q]];
            if (rid < 0) return 1;
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
    return 0;
}

// build_hierarchy's centroid loop (counts in double) ...
static std::vector<double> ref_centroids_partitioned(const std::vector<double>& cur_pts, int32_t n, const std::vector<int32_t>& agg,
                                                     int32_t nc_total) {
    std::vector<double> cp((size_t)3 * nc_total, 0.0), cnt((size_t)nc_total, 0.0);
    for (int32_t i = 0; i < n; ++i) {
        const int32_t I = agg[(size_t)i];
        if (I < 0) continue;
        for (int c3 = 0; c3 < 3; ++c3) cp[3 * (size_t)I + c3] += cur_pts[3 * (size_t)i + c3];
        cnt[(size_t)I] += 1.0;
    }
    for (int32_t I = 0; I < nc_total; ++I)
        if (cnt[(size_t)I] > 0.0) for (int c3 = 0; c3 < 3; ++c3) cp[3 * (size_t)I + c3] /= cnt[(size_t)I];
    return cp;
}

// ... and build_replicated_tail's (counts in int32_t)
static std::vector<double> ref_centroids_replicated(const std::vector<double>& gpts, int32_t n_own, const std::vector<int32_t>& agg,
                                                    int32_t nc) {
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
    return cp;
}

struct RefLayout {
    std::vector<double> cnt;
    std::vector<int64_t> off;
    int32_t maxn = 1, NG = 0;
    int64_t maxnz = 1;
};

// build_replicated_tail: the counts (summed over the ranks) -> offsets and record sizes
static RefLayout ref_layout(int nr, const std::vector<double>& cnt) {
    RefLayout L;
    L.cnt = cnt;
    L.off.assign((size_t)nr + 1, 0);
    for (int r = 0; r < nr; ++r) {
        L.off[r + 1] = L.off[r] + (int64_t)cnt[r];
        L.maxn = std::max(L.maxn, (int32_t)cnt[r]);
        L.maxnz = std::max(L.maxnz, (int64_t)cnt[nr + r]);
    }
    L.NG = (int32_t)L.off[nr];
    return L;
}

// build_replicated_tail: a rank's record
static int ref_record(const RefLayout& L, int me, const HostPattern& cur, int32_t n_owned, const std::vector<int32_t>& g_own,
                      const std::vector<int32_t>& g_gid, std::vector<double>& mine) {
    const std::vector<int64_t>& off = L.off;
    const int32_t maxn = L.maxn;
    mine.assign((size_t)maxn + (size_t)L.maxnz, -1.0);
    for (int32_t i = 0; i < maxn; ++i) mine[i] = i < n_owned ? (double)(cur.rowptr[i + 1] - cur.rowptr[i]) : 0.0;
    for (int32_t sidx = 0; sidx < cur.rowptr[n_owned]; ++sidx) {
        const int32_t j = cur.colind[sidx];
        int64_t gj;
        if (j < n_owned) gj = off[me] + j;
        else {
            const size_t q = (size_t)(j - n_owned);
            if (q >= g_own.size()) return 1;
            gj = off[g_own[q]] + g_gid[q];
        }
        mine[(size_t)maxn + sidx] = (double)gj;
    }
    return 0;
}

// build_replicated_tail: the merge (1: "inconsistent global pattern", 2: "row without a diagonal block")
static int ref_pattern(int nr, const RefLayout& L, const std::vector<double>& all, HostPattern& G, std::vector<int32_t>& valmap,
                       std::vector<int32_t>& rowmap) {
    const std::vector<double>& cnt = L.cnt;
    const std::vector<int64_t>& off = L.off;
    const int32_t maxn = L.maxn, NG = L.NG;
    const int64_t maxnz = L.maxnz;
    G.n = NG;
    G.rowptr.assign((size_t)NG + 1, 0);
    valmap.assign((size_t)nr * maxnz, -1);
    rowmap.assign((size_t)std::max(1, NG), 0);
    const size_t LEN = (size_t)maxn + (size_t)maxnz;
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
                if (ent[k].first < 0 || ent[k].first >= NG || (k > 0 && ent[k].first == ent[k - 1].first)) return 1;
                G.colind[slot] = ent[k].first;
                valmap[ent[k].second] = slot;
                if (ent[k].first == g) { G.diag[g] = slot; has_diag = true; }
            }
            if (!has_diag) return 2;
        }
    }
    return 0;
}

// ---- the simulated ranks ---------------------------------------------------------------------------------------------------------
static bool same(const HaloLists& a, const HaloLists& b) {
    return a.nbr == b.nbr && a.send_ptr == b.send_ptr && a.recv_ptr == b.recv_ptr && a.h_send_idx == b.h_send_idx &&
           a.h_recv_idx == b.h_recv_idx && a.n_own == b.n_own;
}
static bool same(const HostPattern& a, const HostPattern& b) {
    return a.n == b.n && a.nnzb == b.nnzb && a.rowptr == b.rowptr && a.colind == b.colind && a.diag == b.diag;
}
static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}
static int link_of(const HaloLists& p, int peer) {
    for (size_t k = 0; k < p.nbr.size(); ++k)
        if (p.nbr[k] == peer) return (int)k;
    return -1;
}

// level 0: the ranks' shares of the global pattern GP under `owner` (local ids: owned nodes in ascending global id, then the
// ghosts by owner rank and global id; the send lists in the order the receiver lists its ghosts)
static void split_mesh(const HostPattern& GP, const std::vector<double>& gpts, const std::vector<int>& owner, int nr,
                       std::vector<Rank>& ranks) {
    const int32_t n = GP.n;
    std::vector<int32_t> local_of((size_t)n, -1);                // id of a node on its owner
    std::vector<std::vector<int32_t>> owned((size_t)nr), ghost((size_t)nr);
    for (int32_t g = 0; g < n; ++g) { local_of[(size_t)g] = (int32_t)owned[(size_t)owner[g]].size(); owned[(size_t)owner[g]].push_back(g); }
    ranks.assign((size_t)nr, Rank());
    for (int r = 0; r < nr; ++r) {
        Rank& R = ranks[(size_t)r];
        std::vector<int32_t>& gh = ghost[(size_t)r];
        for (int32_t g : owned[(size_t)r])
            for (int32_t k = GP.rowptr[g]; k < GP.rowptr[g + 1]; ++k)
                if (owner[GP.colind[k]] != r) gh.push_back(GP.colind[k]);
        std::sort(gh.begin(), gh.end(), [&](int32_t a, int32_t b) { return owner[a] != owner[b] ? owner[a] < owner[b] : a < b; });
        gh.erase(std::unique(gh.begin(), gh.end()), gh.end());
        R.n_owned = (int32_t)owned[(size_t)r].size();
        std::vector<int32_t> lid((size_t)n, -1);
        for (int32_t g : owned[(size_t)r]) lid[(size_t)g] = local_of[(size_t)g];
        R.p.n_own = R.n_owned;
        R.p.send_ptr.assign(1, 0);
        R.p.recv_ptr.assign(1, 0);
        for (size_t q = 0; q < gh.size(); ++q) {
            lid[(size_t)gh[q]] = R.n_owned + (int32_t)q;
            if (R.p.nbr.empty() || R.p.nbr.back() != owner[gh[q]]) {
                if (!R.p.nbr.empty()) R.p.recv_ptr.push_back((int32_t)q);
                R.p.nbr.push_back(owner[gh[q]]);
            }
            R.p.h_recv_idx.push_back(R.n_owned + (int32_t)q);
            R.ghosts.own.push_back(owner[gh[q]]);
            R.ghosts.gid.push_back(local_of[(size_t)gh[q]]);
        }
        if (!R.p.nbr.empty()) R.p.recv_ptr.push_back((int32_t)gh.size());
        HostPattern& P = R.cur;
        P.n = R.n_owned + (int32_t)gh.size();
        P.rowptr.assign((size_t)P.n + 1, 0);
        P.diag.assign((size_t)P.n, 0);
        for (int32_t i = 0; i < R.n_owned; ++i) {
            const int32_t g = owned[(size_t)r][(size_t)i];
            std::vector<int32_t> cols;
            for (int32_t k = GP.rowptr[g]; k < GP.rowptr[g + 1]; ++k) cols.push_back(lid[(size_t)GP.colind[k]]);
            std::sort(cols.begin(), cols.end());
            P.diag[(size_t)i] = (int32_t)P.colind.size() + (int32_t)(std::lower_bound(cols.begin(), cols.end(), i) - cols.begin());
            P.colind.insert(P.colind.end(), cols.begin(), cols.end());
            P.rowptr[(size_t)i + 1] = (int32_t)P.colind.size();
        }
        for (int32_t i = R.n_owned; i < P.n; ++i) P.rowptr[(size_t)i + 1] = P.rowptr[(size_t)i];
        P.nnzb = (int64_t)P.colind.size();
        R.pts.resize((size_t)3 * P.n);
        for (int32_t g = 0; g < n; ++g)
            if (lid[(size_t)g] >= 0) for (int c = 0; c < 3; ++c) R.pts[3 * (size_t)lid[(size_t)g] + c] = gpts[3 * (size_t)g + c];
    }
    for (int r = 0; r < nr; ++r) {                               // what r sends to s: s's ghosts owned by r, in s's order
        Rank& R = ranks[(size_t)r];
        for (int s : R.p.nbr) {
            for (int32_t g : ghost[(size_t)s])
                if (owner[g] == r) R.p.h_send_idx.push_back(local_of[(size_t)g]);
            R.p.send_ptr.push_back((int32_t)R.p.h_send_idx.size());
        }
    }
}

// the exchange, by copying: rank r's local vector of the owners' aggregate ids (-1 where nothing arrives)
static int exchange_ids(const std::vector<Rank>& ranks, int r, std::vector<int32_t>& owner_agg) {
    const Rank& R = ranks[(size_t)r];
    owner_agg.assign((size_t)R.cur.n, -1);
    for (size_t k = 0; k < R.p.nbr.size(); ++k) {
        const Rank& S = ranks[(size_t)R.p.nbr[k]];
        const int ks = link_of(S.p, r);
        CHECK(ks >= 0, "a link has two ends");
        const int32_t cnt = R.p.recv_ptr[k + 1] - R.p.recv_ptr[k];
        CHECK(cnt == S.p.send_ptr[(size_t)ks + 1] - S.p.send_ptr[(size_t)ks], "send and receive counts of a link");
        CHECK(cnt > 0 || R.p.send_ptr[k + 1] > R.p.send_ptr[k], "a link moves something");
        for (int32_t j = 0; j < cnt; ++j)
            owner_agg[(size_t)R.p.h_recv_idx[(size_t)R.p.recv_ptr[k] + j]] = S.agg[(size_t)S.p.h_send_idx[(size_t)S.p.send_ptr[(size_t)ks] + j]];
    }
    return 0;
}

// the replicated level of the ranks' fronts: the new functions against the transcription and the properties of the result
static int check_replication(const std::vector<Rank>& ranks, const char* what) {
    const int nr = (int)ranks.size();
    std::vector<double> cnt((size_t)2 * nr, 0.0);
    for (int r = 0; r < nr; ++r) {
        cnt[(size_t)r] = (double)ranks[(size_t)r].n_owned;
        cnt[(size_t)nr + r] = (double)ranks[(size_t)r].cur.rowptr[(size_t)ranks[(size_t)r].n_owned];
    }
    const ReplicatedLayout lay = replicated_layout(nr, cnt.data());
    const RefLayout ref = ref_layout(nr, cnt);
    CHECK(lay.off == ref.off && lay.maxn == ref.maxn && lay.maxnz == ref.maxnz && lay.NG == ref.NG, what);
    for (int r = 0; r < nr; ++r) CHECK(lay.rows[(size_t)r] == (int32_t)cnt[(size_t)r], what);
    std::vector<double> all, all_ref;
    for (int r = 0; r < nr; ++r) {
        const Rank& R = ranks[(size_t)r];
        std::vector<double> mine, mine_ref;
        CHECK(replicated_record(lay, r, R.cur, R.n_owned, R.ghosts, mine) == SNS_OK, what);
        CHECK(ref_record(ref, r, R.cur, R.n_owned, R.ghosts.own, R.ghosts.gid, mine_ref) == 0, what);
        CHECK(same_bits(mine, mine_ref) && mine.size() == lay.record(), what);
        all.insert(all.end(), mine.begin(), mine.end());
        // the id mapping alone, as the columns of M = A P take it (build_replicated_tail: "for (auto& j : col)")
        for (int32_t j = 0; j < R.cur.n; ++j) {
            const int32_t want = j < R.n_owned ? (int32_t)ref.off[(size_t)r] + j
                                               : (int32_t)ref.off[(size_t)R.ghosts.own[(size_t)(j - R.n_owned)]] + R.ghosts.gid[(size_t)(j - R.n_owned)];
            CHECK(replicated_id(lay, r, R.n_owned, R.ghosts, j) == (int64_t)want, what);
        }
        CHECK(replicated_id(lay, r, R.n_owned, R.ghosts, R.cur.n) == -1, "a column past the ghosts has no owner record");
    }
    HostPattern G, Gr;
    std::vector<int32_t> valmap, rowmap, valmap_r, rowmap_r;
    CHECK(replicated_pattern(lay, all, G, valmap, rowmap) == SNS_OK, what);
    CHECK(ref_pattern(nr, ref, all, Gr, valmap_r, rowmap_r) == 0, what);
    CHECK(same(G, Gr) && valmap == valmap_r && rowmap == rowmap_r, what);
    // valmap: a bijection of the non-padding gathered slots onto G's slots
    std::vector<char> hit((size_t)G.nnzb, 0);
    for (int r = 0; r < nr; ++r)
        for (int64_t s = 0; s < lay.maxnz; ++s) {
            const int32_t v = valmap[(size_t)(r * lay.maxnz + s)];
            const bool padding = s >= (int64_t)cnt[(size_t)nr + r];
            CHECK(padding ? v == -1 : (v >= 0 && v < G.nnzb && !hit[(size_t)v]++), "valmap is a bijection");
        }
    CHECK(std::count(hit.begin(), hit.end(), 1) == G.nnzb, "valmap is onto");
    // G directly: every rank's owned rows with their columns relabelled through the ghosts' (owner, owner-local id)
    CHECK(G.n == lay.NG && (int32_t)G.rowptr.size() == lay.NG + 1 && G.rowptr[0] == 0, what);
    for (int r = 0; r < nr; ++r) {
        const Rank& R = ranks[(size_t)r];
        for (int32_t i = 0; i < R.n_owned; ++i) {
            const int32_t g = (int32_t)lay.off[(size_t)r] + i;
            CHECK(rowmap[(size_t)g] == r * lay.maxn + i, "rowmap");
            std::vector<int32_t> cols;
            for (int32_t k = R.cur.rowptr[i]; k < R.cur.rowptr[i + 1]; ++k) {
                const int32_t j = R.cur.colind[(size_t)k];
                const int own = j < R.n_owned ? r : R.ghosts.own[(size_t)(j - R.n_owned)];
                cols.push_back((int32_t)lay.off[(size_t)own] + (j < R.n_owned ? j : R.ghosts.gid[(size_t)(j - R.n_owned)]));
            }
            std::sort(cols.begin(), cols.end());
            CHECK(std::adjacent_find(cols.begin(), cols.end()) == cols.end(), "columns unique");
            CHECK(G.rowptr[(size_t)g + 1] - G.rowptr[(size_t)g] == (int32_t)cols.size(), "row length");
            CHECK(std::equal(cols.begin(), cols.end(), G.colind.begin() + G.rowptr[(size_t)g]), "G is the relabelled union of the local rows");
            CHECK(G.diag[(size_t)g] >= G.rowptr[(size_t)g] && G.diag[(size_t)g] < G.rowptr[(size_t)g + 1] && G.colind[(size_t)G.diag[(size_t)g]] == g,
                  "diag points at the diagonal");
        }
    }
    return 0;
}

// one coarsening step of all ranks; `ranks` becomes the coarse front
static int coarsen(std::vector<Rank>& ranks, int level) {
    const int nr = (int)ranks.size();
    for (Rank& R : ranks) {
        R.nc_owned = 0;
        aggregate_nodes(R.cur, R.n_owned, 8, R.agg, R.nc_owned, R.pts.data());
        CHECK((int32_t)R.agg.size() == R.cur.n, "aggregate_nodes: one entry per local node");
    }
    std::vector<HaloLists> coarse((size_t)nr);
    std::vector<GhostIds> cghosts((size_t)nr);
    std::vector<std::vector<int32_t>> owned_agg((size_t)nr);
    for (int r = 0; r < nr; ++r) owned_agg[(size_t)r] = ranks[(size_t)r].agg;      // (before the ghost entries are filled in)
    std::vector<HostAggregation> A((size_t)nr);
    for (int r = 0; r < nr; ++r) {
        Rank& R = ranks[(size_t)r];
        std::vector<int32_t> owner_agg;
        if (exchange_ids(ranks, r, owner_agg)) return 1;
        // the exchanged vector as build_hierarchy held it
        std::vector<double> ids((size_t)4 * R.cur.n, -1.0);
        for (int32_t i = 0; i < R.cur.n; ++i) ids[(size_t)4 * i] = (double)(i < R.n_owned ? R.agg[(size_t)i] : owner_agg[(size_t)i]);
        std::vector<int32_t> agg_ref = R.agg, g_own, g_gid, agg_new = R.agg;
        HaloLists plan_ref;
        int32_t nct_ref = 0, nct = 0;
        CHECK(ref_coarse_plan(R.p, ids, R.nc_owned, agg_ref, plan_ref, g_own, g_gid, nct_ref) == 0, "transcription");
        CHECK(coarse_halo_lists(R.p, owner_agg, R.nc_owned, agg_new, coarse[(size_t)r], cghosts[(size_t)r], nct) == SNS_OK, "coarse_halo_lists");
        CHECK(same(coarse[(size_t)r], plan_ref) && agg_new == agg_ref && cghosts[(size_t)r].own == g_own && cghosts[(size_t)r].gid == g_gid &&
                  nct == nct_ref, "coarse lists equal the parent's");
        // the receive lists are n_own + q in order
        const HaloLists& c = coarse[(size_t)r];
        CHECK(c.n_own == R.nc_owned && (int32_t)c.h_recv_idx.size() == nct - R.nc_owned, "ghost count");
        for (size_t q = 0; q < c.h_recv_idx.size(); ++q) CHECK(c.h_recv_idx[q] == R.nc_owned + (int32_t)q, "receive list in order");
        // every ghost coarse node is the aggregate its fine members have on their owner
        for (int32_t j = R.n_owned; j < R.cur.n; ++j) {
            const size_t q = (size_t)(j - R.n_owned), Q = (size_t)(agg_new[(size_t)j] - R.nc_owned);
            CHECK(agg_new[(size_t)j] >= R.nc_owned && Q < g_own.size(), "ghost node has a ghost aggregate");
            CHECK(g_own[Q] == R.ghosts.own[q] && g_gid[Q] == owned_agg[(size_t)R.ghosts.own[q]][(size_t)R.ghosts.gid[q]], "ghost aggregate identity");
        }
        build_coarse_from_agg(R.cur, R.n_owned, agg_new, R.nc_owned, nct, A[(size_t)r]);
    }
    // per link: the k-th aggregate r sends to s is the k-th ghost s receives from r; the counts match both ways
    for (int r = 0; r < nr; ++r)
        for (size_t k = 0; k < coarse[(size_t)r].nbr.size(); ++k) {
            const int s = coarse[(size_t)r].nbr[k];
            const HaloLists &cr = coarse[(size_t)r], &cs = coarse[(size_t)s];
            const int ks = link_of(cs, r);
            CHECK(ks >= 0, "coarse link has two ends");
            const int32_t ns = cr.send_ptr[k + 1] - cr.send_ptr[k], nrv = cs.recv_ptr[(size_t)ks + 1] - cs.recv_ptr[(size_t)ks];
            CHECK(ns == nrv, "coarse send count == the peer's receive count");
            for (int32_t j = 0; j < ns; ++j) {
                const int32_t sent = cr.h_send_idx[(size_t)cr.send_ptr[k] + j];
                const size_t Q = (size_t)(cs.h_recv_idx[(size_t)cs.recv_ptr[(size_t)ks] + j] - cs.n_own);
                CHECK(sent >= 0 && sent < cr.n_own, "an owned aggregate is sent");
                CHECK(cghosts[(size_t)s].own[Q] == r && cghosts[(size_t)s].gid[Q] == sent, "k-th sent is the k-th received");
            }
        }
    int64_t nodes = 0, aggs = 0, ghosts = 0;
    for (int r = 0; r < nr; ++r) {
        Rank& R = ranks[(size_t)r];
        HostAggregation& a = A[(size_t)r];
        // centroids: bit for bit what either of the parent's loops gives
        const std::vector<double> cp = aggregate_centroids(R.pts.data(), R.cur.n, a.agg, a.coarse.n);
        CHECK(same_bits(cp, ref_centroids_partitioned(R.pts, R.cur.n, a.agg, a.coarse.n)), "centroids, the partitioned loop");
        if (R.cur.n == R.n_owned) CHECK(same_bits(cp, ref_centroids_replicated(R.pts, R.n_owned, a.agg, a.nc)), "centroids, the replicated loop");
        // (the replicated loop on the owned nodes alone: the same arithmetic with the count kept as an integer)
        std::vector<int32_t> own_only = a.agg;
        for (int32_t j = R.n_owned; j < R.cur.n; ++j) own_only[(size_t)j] = -1;
        CHECK(same_bits(aggregate_centroids(R.pts.data(), R.cur.n, own_only, a.nc), ref_centroids_replicated(R.pts, R.n_owned, own_only, a.nc)),
              "centroids, integer counts");
        nodes += R.n_owned; aggs += a.nc; ghosts += a.coarse.n - a.nc;
        R.pts = cp;
        R.cur = std::move(a.coarse);
        R.n_owned = a.nc;
        R.p = std::move(coarse[(size_t)r]);
        R.ghosts = std::move(cghosts[(size_t)r]);
    }
    std::printf("  level %d: %ld nodes -> %ld aggregates, %ld ghost aggregates over %d ranks\n", level, (long)nodes, (long)aggs, (long)ghosts, nr);
    return 0;
}

static int run_case(const char* name, const HostPattern& GP, const std::vector<double>& gpts, const std::vector<int>& owner, int nr,
                    size_t most_neighbours, int32_t fewest_rows) {
    std::printf("case %s\n", name);
    std::vector<Rank> ranks;
    split_mesh(GP, gpts, owner, nr, ranks);
    size_t nb = 0;
    int32_t rows = GP.n;
    for (const Rank& R : ranks) { nb = std::max(nb, R.p.nbr.size()); rows = std::min(rows, R.n_owned); }
    CHECK(nb == most_neighbours && (rows == 0) == (fewest_rows == 0), "the case is what its name says");
    for (int level = 0; level < 2; ++level) {
        if (check_replication(ranks, name)) return 1;
        if (coarsen(ranks, level)) return 1;
    }
    return check_replication(ranks, name);
}

// the error returns: code and text
static int check_errors(const HostPattern& GP, const std::vector<double>& gpts, const std::vector<int>& owner, int nr) {
    std::vector<Rank> ranks;
    split_mesh(GP, gpts, owner, nr, ranks);
    for (Rank& R : ranks) aggregate_nodes(R.cur, R.n_owned, 8, R.agg, R.nc_owned, R.pts.data());
    Rank& R = ranks[0];
    std::vector<int32_t> owner_agg;
    if (exchange_ids(ranks, 0, owner_agg)) return 1;
    CHECK(!R.p.h_recv_idx.empty(), "rank 0 has ghosts");
    owner_agg[(size_t)R.p.h_recv_idx.back()] = -1;               // the owner left this node out of every aggregate
    HaloLists c;
    GhostIds g;
    int32_t nct = 0;
    std::vector<int32_t> agg = R.agg;
    g_err.clear();
    CHECK(coarse_halo_lists(R.p, owner_agg, R.nc_owned, agg, c, g, nct) == SNS_E_COMM, "ghost without an aggregate: code");
    CHECK(g_err == "hierarchy: ghost node without an aggregate on its owner", "ghost without an aggregate: text");
    std::vector<double> cnt((size_t)2 * nr, 0.0);
    for (int r = 0; r < nr; ++r) { cnt[(size_t)r] = ranks[(size_t)r].n_owned; cnt[(size_t)nr + r] = ranks[(size_t)r].cur.rowptr[(size_t)ranks[(size_t)r].n_owned]; }
    const ReplicatedLayout lay = replicated_layout(nr, cnt.data());
    std::vector<double> all, mine;
    GhostIds cut = R.ghosts;                                     // a ghost column past the owner records
    cut.own.pop_back();
    cut.gid.pop_back();
    g_err.clear();
    CHECK(replicated_record(lay, 0, R.cur, R.n_owned, cut, mine) == SNS_E_STATE, "ghost column without an owner record: code");
    CHECK(g_err == "replicated tail: ghost column without an owner record", "ghost column without an owner record: text");
    for (int r = 0; r < nr; ++r) {
        CHECK(replicated_record(lay, r, ranks[(size_t)r].cur, ranks[(size_t)r].n_owned, ranks[(size_t)r].ghosts, mine) == SNS_OK, "records");
        all.insert(all.end(), mine.begin(), mine.end());
    }
    HostPattern G;
    std::vector<int32_t> valmap, rowmap;
    const RefLayout ref = ref_layout(nr, cnt);
    const size_t first = (size_t)lay.maxn;                       // rank 0's first slot: row 0 has at least two columns
    CHECK(all[0] >= 2.0, "row 0 has two blocks");
    std::vector<double> bad = all;
    bad[first + 1] = bad[first];                                 // the same column twice in a row
    g_err.clear();
    CHECK(replicated_pattern(lay, bad, G, valmap, rowmap) == SNS_E_STATE && g_err == "replicated tail: inconsistent global pattern", "duplicate column");
    CHECK(ref_pattern(nr, ref, bad, G, valmap, rowmap) == 1, "duplicate column, transcription");
    bad = all;
    bad[first] = (double)lay.NG;                                 // a column past the level
    g_err.clear();
    CHECK(replicated_pattern(lay, bad, G, valmap, rowmap) == SNS_E_STATE && g_err == "replicated tail: inconsistent global pattern", "column out of range");
    bad = all;                                                   // row 0 of rank 0 loses its diagonal (global id 0) to an unused column
    std::vector<char> used((size_t)lay.NG, 0);
    size_t at = 0;
    for (int32_t k = 0; k < (int32_t)all[0]; ++k) { used[(size_t)all[first + k]] = 1; if (all[first + k] == 0.0) at = first + (size_t)k; }
    CHECK(at >= first && all[at] == 0.0, "row 0 has its diagonal");
    const int32_t unused = (int32_t)(std::find(used.begin(), used.end(), 0) - used.begin());
    CHECK(unused < lay.NG, "a column row 0 does not have");
    bad[at] = (double)unused;
    g_err.clear();
    CHECK(replicated_pattern(lay, bad, G, valmap, rowmap) == SNS_E_STATE && g_err == "replicated tail: row without a diagonal block", "missing diagonal");
    CHECK(ref_pattern(nr, ref, bad, G, valmap, rowmap) == 2, "missing diagonal, transcription");
    std::printf("error returns: 5 checked\n");
    return 0;
}

int main() {
    // Kuhn box nx x ny x nz, its nodes renumbered by a random permutation
    const int nx = 12, ny = 6, nz = 5;
    const int sy = nz + 1, sx = (ny + 1) * (nz + 1), n = (nx + 1) * sx;
    const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    std::mt19937 rng(7);
    std::vector<int32_t> newid((size_t)n);
    for (int i = 0; i < n; ++i) newid[(size_t)i] = i;
    std::shuffle(newid.begin(), newid.end(), rng);
    std::vector<int32_t> tets;
    for (int i = 0; i < nx; ++i) for (int j = 0; j < ny; ++j) for (int k = 0; k < nz; ++k) {
        const int base = i * sx + j * sy + k;
        for (auto& p : perm) {
            int off[3] = {0, 0, 0};
            tets.push_back(newid[(size_t)base]);
            for (int s = 0; s < 3; ++s) { off[p[s]] = 1; tets.push_back(newid[(size_t)(base + off[0] * sx + off[1] * sy + off[2])]); }
        }
    }
    std::vector<double> pts((size_t)3 * n);
    std::vector<int> ix((size_t)n), iy((size_t)n);
    std::uniform_real_distribution<double> jitter(-0.1, 0.1);
    for (int i = 0; i <= nx; ++i) for (int j = 0; j <= ny; ++j) for (int k = 0; k <= nz; ++k) {
        const size_t g = (size_t)newid[(size_t)(i * sx + j * sy + k)];
        pts[3 * g] = i + jitter(rng); pts[3 * g + 1] = j + jitter(rng); pts[3 * g + 2] = k + jitter(rng);
        ix[g] = i; iy[g] = j;
    }
    HostPattern GP;
    HostAssemblyMaps M;
    build_pattern(n, (int64_t)tets.size() / 4, tets.data(), GP, M);
    std::printf("Kuhn box %d x %d x %d: %d nodes, %ld blocks\n", nx, ny, nz, n, (long)GP.nnzb);
    std::vector<int> owner((size_t)n);
    for (int nr = 2; nr <= 4; ++nr) {                            // x-slabs
        for (int g = 0; g < n; ++g) owner[(size_t)g] = std::min(nr - 1, ix[(size_t)g] * nr / (nx + 1));
        if (run_case(("x-slabs, " + std::to_string(nr) + " ranks").c_str(), GP, pts, owner, nr, nr > 2 ? 2 : 1, 1)) return 1;
    }
    for (int g = 0; g < n; ++g) owner[(size_t)g] = (ix[(size_t)g] > nx / 2 ? 1 : 0) + (iy[(size_t)g] > ny / 2 ? 2 : 0);
    if (run_case("2 x 2 blocks (corner ghosts)", GP, pts, owner, 4, 3, 1)) return 1;
    if (check_errors(GP, pts, owner, 4)) return 1;
    for (int g = 0; g < n; ++g) owner[(size_t)g] = ix[(size_t)g] > nx / 2 ? 2 : 0;      // rank 1 of 3 owns no row
    if (run_case("3 ranks, rank 1 without rows", GP, pts, owner, 3, 1, 0)) return 1;
    std::printf("hierarchy host logic: all cases passed\n");
    return 0;
}
