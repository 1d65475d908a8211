// Internal structures shared by the host setup code, the HIP kernels and the
// C-ABI layer.  Not installed; the public surface is include/sns.h.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "sns.h"
#include "sns_devbuf.h"
#include "sns_policy.h"

namespace sns {

// ---- host-side symbolic data (built once per mesh, sns_host.cpp) ------------
struct HostPattern {
    int32_t n = 0;                       // block rows (nodes)
    int64_t nnzb = 0;
    std::vector<int32_t> rowptr, colind; // BSR pattern, columns sorted per row
    std::vector<int32_t> diag;           // slot of the diagonal block of each row
};

struct HostAssemblyMaps {
    // node -> incident (tet*4 + a), tet order: gather list for the residual
    std::vector<int64_t> nt_ptr;         // n+1
    std::vector<int32_t> nt_idx;         // 4*E   (tet*4+a fits int32 up to 536M tets)
    // BSR slot -> contributing element blocks (tet*16 + a*4 + b), fixed order
    std::vector<int64_t> c_ptr;          // nnzb+1
    std::vector<int32_t> c_idx;          // 16*E  (tet*16+ab as an UNSIGNED 32-bit pattern: up to 268 M tets)
};

struct HostAggregation {
    int32_t nc = 0;
    std::vector<int32_t> agg;            // fine node -> aggregate
    std::vector<int32_t> m_ptr, m_idx;   // aggregate -> member fine nodes
    HostPattern coarse;                  // coarse BSR pattern
    std::vector<int64_t> r_ptr;          // coarse slot -> fine slots (RAP gather)
    std::vector<int32_t> r_idx;
};

struct HostAP {                          // pattern of M = A P (fine rows x coarse columns) + its gather lists
    int32_t n = 0;
    int64_t nnz = 0;
    std::vector<int32_t> rowptr, colind; // per fine row: the aggregates its columns fall into (sorted)
    std::vector<int32_t> slot_row;       // fine row of each M slot
    std::vector<int32_t> ap_ptr, ap_idx; // M slot -> fine slots summed into it
    std::vector<uint64_t> nib;           // the same relation per fine block of a row: nibble j = row-local M slot of block j (15: the column
                                         // takes no part); ~0 = the row has more than 16 blocks or more than 8 slots (k_lp_copies16's register path)
};
void build_ap_pattern(const HostPattern& F, int32_t n_rows, const std::vector<int32_t>& agg_all, HostAP& M);

void build_pattern(int32_t n_nodes, int64_t n_tets, const int32_t* tets, HostPattern& P,
                   HostAssemblyMaps& M, int npe = 4);

// the lists of the boundary pass (csrc/sns_boundary.hip), built once per sns_set_boundary_facets
struct HostFacetLists {
    std::vector<int32_t> facets;         // 3*nf, rewound: (x1 - x0) x (x2 - x0) points out of the owning tet
    std::vector<int32_t> rows;           // the boundary rows: nodes of listed facets, ascending
    std::vector<int32_t> row_ptr;        // rows+1
    std::vector<int32_t> row_fv;         // 3*nf: facet * 4 + local vertex, per row in ascending facet order
};
// throws std::runtime_error (nothing written) for a facet that is no face of its tet, is listed twice or has no area
void build_facet_lists(int32_t n_nodes, int64_t n_tets, const int32_t* tets, const double* pts, int32_t n_facets,
                       const int32_t* facets, const int64_t* facet_tets, HostFacetLists& L);
void build_aggregation(const HostPattern& fine, int max_agg, HostAggregation& A);
// same, but only nodes [0, n_active) take part (distributed level 0: owned nodes only)
void build_aggregation_active(const HostPattern& fine, int32_t n_active, int max_agg, HostAggregation& A);
void build_coarse_from_agg(const HostPattern& F, int32_t n_owned_fine, const std::vector<int32_t>& agg_all,
                           int32_t nc_owned, int32_t nc_total, HostAggregation& A);

// ---- host index logic of the distributed hierarchy build (sns_host.cpp; tests/hierarchy_host_main.cpp) ----------------------
// the host half of a level's halo plan (counts in nodes); Plan (csrc/sns_comm.h) adds the device half
struct HaloLists {
    std::vector<int> nbr;                        // neighbour ranks, same order on both sides of a link
    std::vector<int32_t> send_ptr, recv_ptr;     // per neighbour: its range of h_send_idx / h_recv_idx
    std::vector<int32_t> h_send_idx, h_recv_idx; // local nodes sent / ghost nodes received
    int32_t n_own = 0;                           // owned nodes of the level (the ghost nodes follow them)
};
// where a level's ghost nodes live: owner rank and owner-local id of ghost q (local node n_owned + q).  Owned by the build.
struct GhostIds {
    std::vector<int32_t> own, gid;
};
// the points of the coarse nodes: the centroids of the aggregates (members summed in node order, divided by their count)
std::vector<double> aggregate_centroids(const double* pts, int32_t n, const std::vector<int32_t>& agg, int32_t nc);
// The coarse level's halo lists from the finer level's `p` and `owner_agg` (per local node of the finer level; read at the ghost
// nodes: the aggregate of the node on its owner, as exchanged).  Per link the distinct aggregates in ascending owner id become
// the ghost coarse nodes nc_owned, nc_owned + 1, ... (agg's ghost entries are filled in with them) and the distinct aggregates
// of the nodes sent the send list: both ends of a link sort the same set of ids, so the k-th sent is the k-th received.
// SNS_E_COMM (text set) for a ghost node whose owner gave it no aggregate.
int coarse_halo_lists(const HaloLists& p, const std::vector<int32_t>& owner_agg, int32_t nc_owned, std::vector<int32_t>& agg,
                      HaloLists& coarse, GhostIds& ghosts, int32_t& nc_total);
// The replicated level: rank r's rows[r] owned rows of the source level become rows off[r] .. of the global pattern.  What
// every rank all-gathers is a record of maxn + maxnz doubles: [0, maxn) its row lengths, then the global column ids of its slots
// (-1: padding).
struct ReplicatedLayout {
    std::vector<int32_t> rows;                   // per rank
    std::vector<int64_t> off;                    // nranks + 1
    int32_t maxn = 1, NG = 0;
    int64_t maxnz = 1;
    size_t record() const { return (size_t)maxn + (size_t)maxnz; }
};
ReplicatedLayout replicated_layout(int nranks, const double* rows_then_slots /* 2 * nranks, summed over the ranks */);
// local column j of rank `me` (owned, or ghost q = j - n_owned) -> id in the replicated level; -1: a ghost without an owner record
int64_t replicated_id(const ReplicatedLayout& lay, int me, int32_t n_owned, const GhostIds& ghosts, int32_t j);
// rank `me`'s record; SNS_E_STATE (text set) for a ghost column without an owner record
int replicated_record(const ReplicatedLayout& lay, int me, const HostPattern& cur, int32_t n_owned, const GhostIds& ghosts,
                      std::vector<double>& mine);
// the global pattern G from the ranks' records `all`, with valmap [nranks * maxnz]: gathered slot -> slot of G (-1: padding)
// and rowmap [max(1, NG)]: row of G -> gathered row rank * maxn + i.  SNS_E_STATE (text set) for an inconsistent pattern
int replicated_pattern(const ReplicatedLayout& lay, const std::vector<double>& all, HostPattern& G, std::vector<int32_t>& valmap,
                       std::vector<int32_t>& rowmap);

// ---- device-side level of the operator hierarchy ----------------------------
// (move-only: every device array is owned by the level, csrc/sns_devbuf.h)
struct Level {
    int32_t n = 0;                       // local block rows (owned + ghost on level 0)
    int32_t n_owned = 0;                 // rows that are solved for (== n when serial)
    int64_t n_global = 0;                // rows of this level over all ranks (a replicated level: its own rows)
    int64_t nnzb = 0;
    DevBuf<int32_t> rowptr, colind, diag;
    DevBuf<double> vals;                 // nnzb*16, block row-major
    DevBuf<double> dinv;                 // n*16
    DevBuf<int32_t> slot_row;            // nnzb: block row of each slot
    DevBuf<float> vals32;                // fp32 copy of vals for the preconditioner passes (amg_f32_matrix)
    DevBuf<void> vals16;                 // fp16 copy, row-scaled (amg_f32_matrix = 2): 4 halfs per block row
    DevBuf<float> scale16;               // its scales, one per dof row
    DevBuf<float> dinv32;                // fp32 copy of dinv for the low-precision Jacobi sweeps
    // to the next coarser level
    int32_t nc = 0;
    DevBuf<int32_t> agg;                 // n
    DevBuf<int32_t> m_ptr, m_idx;
    DevBuf<int64_t> r_ptr;
    DevBuf<int32_t> r_idx;
    DevBuf<uint8_t> free_mask;           // 4*n: 1 where dof takes part in transfer (level 0: !bc), else all 1
    DevBuf<uint8_t> empty_c;             // 4*nc, the fine level only.  Held by level l, it flags the dofs of level l + 1 (the coarse
                                         // side): per aggregate and component, the members excluded from the transfer (k_empty_coarse)
    // M = A P of this level for the fused first post-smoothing sweep (k_post_lp): pattern + gather lists (symbolic, once),
    // values per numeric setup straight into the level's low-precision format (k_lp_copies16 / k_ap_cvt32)
    int64_t ap_nnz = 0;
    DevBuf<int32_t> ap_rowptr, ap_colind, ap_ptr, ap_idx;
    DevBuf<int32_t> ap_colind_rep;       // partitioned level right above the replicated tail's source: M's columns in the ids of the replicated level
    DevBuf<uint64_t> ap_nib;             // per row: nibble j = the row-local M slot of block j (15: none); ~0 = row too long for k_lp_copies16's registers
    DevBuf<float> ap_vals32;
    DevBuf<void> ap_vals16;
    DevBuf<float> ap_scale16;
    // aggregate-block Jacobi smoother (amg_block_smooth, csrc/sns_block.hip): member rows of every aggregate padded to 8 slots
    // (-1: none), built with the hierarchy; the aggregates' inverse diagonal blocks (fp32, 1024 floats each) per numeric setup
    DevBuf<int32_t> blk_rows;
    DevBuf<int32_t> blk_of;              // node -> its smoother block (-1: ghost node)
    int32_t n_blk = 0;                   // smoother blocks (= nc, plus one per aggregate of more than 8 nodes)
    DevBuf<void> binv32;                 // (fp32 blocks, or fp16 + row scales: the format of the level's matrix copy, binv_fmt)
    int binv_fmt = 0;
    // work vectors (4*n doubles)
    DevBuf<double> x, b, r;
    DevBuf<double> pong;                 // the smoother's ping-pong buffer
    DevBuf<double> xg;                   // distributed runs: copy of the iterate whose ghost tail is exchanged
    // coarsest level: dense inverse (4n x 4n), row-major
    DevBuf<double> dense_inv;
    // ... or, for a coarsest level of up to amg_dense_rows rows, the blocked Gauss-Jordan inverse (csrc/sns_dense.hip): the
    // Np x Np fp64 matrix the elimination works in (Np = 4n rounded up to a multiple of 64), its workspace, and the finished
    // inverse as fp32 (leading dimension Np) for the cycle's matvec
    int dense_np = 0;
    DevBuf<double> dense_gj, dense_work;
    DevBuf<float> dense_x32;
    // block-Jacobi damping actually used on this level (damping.omega) and the estimates behind it; written by the three
    // transitions of csrc/sns_damping.hip only
    policy::LevelDamping damping;
};

void aggregate_nodes(const HostPattern& F, int32_t n_active, int max_agg, std::vector<int32_t>& agg, int32_t& nc,
                     const double* pts = nullptr, int* which = nullptr);
// aggregation of nodes [0, n_active) by operator strength: `strength` = one value per block slot of F (k_strength); the aggregates
// have at most max_agg members, are connected in the strong graph and do not depend on the node numbering (ties aside)
void aggregate_strength(const HostPattern& F, int32_t n_active, int max_agg, const float* strength, std::vector<int32_t>& agg,
                        int32_t& nc);
void set_error(const std::string& s);
const std::string& last_error();               // the calling thread's text (sns_last_error)

}  // namespace sns
