// C-ABI layer (include/sns.h): handle life cycle, communicator attachment, the introspection getters and bench hooks, and the
// entry points of the hot path (residual / Jacobian / SpMV / preconditioner / Krylov / Stokes / Newton / ...), which check their
// arguments, ask the request gate and make one call into sns::.  There is no CPU compute path.  (The solve drivers live in
// csrc/sns_solve.hip, the setup, cycle and Krylov parts in csrc/sns_setup.hip, sns_damping.hip, sns_cycle.hip and sns_krylov.hip;
// shared internals in csrc/sns_ctx.h; the policy of the hierarchy, the gate and the drivers in csrc/sns_policy.h.)  The handle owns its
// device memory and HIP objects by type (csrc/sns_devbuf.h): sns_destroy is `delete h`, and a failing create frees what it made.
#include <atomic>

#include "sns_ctx.h"

namespace sns {
static thread_local std::string g_err;
void set_error(const std::string& s) { g_err = s; }
const std::string& last_error() { return g_err; }

// the allocator behind every DevBuf, and the bytes it has handed out and not got back (sns_live_device_bytes)
static std::atomic<int64_t> g_live_bytes{0};
int dev_malloc_bytes(void** p, size_t bytes) {
    *p = nullptr;
    HIP_TRY(hipMalloc(p, bytes));
    g_live_bytes += (int64_t)bytes;
    return SNS_OK;
}
void dev_free_bytes(void* p, size_t bytes) {
    (void)hipFree(p);
    g_live_bytes -= (int64_t)bytes;
}
int dev_upload_bytes(void* dst, const void* src, size_t bytes) {
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return SNS_OK;
}

}  // namespace sns

// ============================================================================
// C ABI
// ============================================================================
extern "C" {


void sns_default_options(sns_options* o) {
    o->reynolds = 1.0;
    o->ksp_type = SNS_KSP_BICGSTAB;
    o->pc_type = SNS_PC_AMG;
    o->ksp_rtol = 1e-8;
    o->ksp_atol = 1e-50;
    o->ksp_max_it = 10000;
    o->gmres_restart = 30;
    o->snes_rtol = 1e-8;
    o->snes_atol = 1e-8;
    o->snes_stol = 1e-8;
    o->snes_max_it = 30;
    o->amg_max_levels = 12;
    o->amg_coarse_size = 32;
    o->amg_agg_size = 8;
    o->amg_nu = 1;
    o->amg_omega = 0.8;
    o->monitor = 0;
    o->corrected_convection = 0;
    o->amg_f32_matrix = 2;
    o->amg_nu_coarse = 4;
    o->amg_nu_deep = 2;
    o->amg_nu_l2 = 6;
    o->assembly_fused = 1;
    o->amg_sweep_exchange_rows = 0;
    o->amg_replicate_rows = 65536;
    o->amg_post_exchange = 1;
    o->stokes_viscosity = 1.0;
    o->stokes_beta = 0.2;
    o->amg_nu_l1_pre = 0;
    o->amg_nu_l1_post = 0;
    o->amg_retry_damping = 1;
    o->amg_retry_stall_its = 100;
    o->halo_overlap = 1;
    o->amg_fused_post = 1;
    o->amg_nu_scale_with_size = 1;
    o->amg_dense_rows = 512;
    o->amg_block_smooth = 1;
    o->amg_bnu_l1 = 3;
    o->amg_bnu_l2 = 4;
    o->amg_bnu_deep = 2;
    o->amg_ritz_limit = 1;
    o->amg_block_max_rows = 0;
    o->amg_block_fine_rows = 600000;
    o->amg_fuse_restrict = 1;
    o->halo_windows = 1;
    o->amg_exact_sweeps = 1;
    o->amg_aggregation = 0;
}


const char* sns_last_error(void) { return g_err.c_str(); }

const char* sns_version(void) { return "sns 0.1 (gfx950)"; }

int sns_abi_version(void) { return SNS_ABI_VERSION; }

int64_t sns_live_device_bytes(void) { return g_live_bytes.load(); }

int64_t sns_options_size(void) { return (int64_t)sizeof(sns_options); }


// amg_aggregation: 0, 1, 2 or 3; 1 and 2 (the same map, built on the host / on the device) and 3 (the hybrid) on 3-D handles only
// (the strength kernel reads the 4 x 4 blocks of the P1-P1 tet operator) and with aggregates that fit the 32 x 32 smoother blocks
static int check_aggregation_option(int dim, const sns_options& o) {
    if (o.amg_aggregation == 0) return SNS_OK;
    if (o.amg_aggregation < 1 || o.amg_aggregation > 3 || dim != 3 || o.amg_agg_size > policy::STRENGTH_MAX_AGG) {
        set_error("amg_aggregation: 0, or 1, 2 or 3 on a 3-D handle with amg_agg_size <= 8");
        return SNS_E_ARG;
    }
    return SNS_OK;
}

// dim 3: points [n*3], cells [E*4];  dim 2: points [n*2], cells [E*3]
static int create_common(int dim, sns_handle* out, int32_t n_nodes, int64_t n_tets, const double* points_in,
                         const int32_t* cells_in, const uint8_t* bc_mask_in, const double* bc_val_in, int device,
                         const sns_options* opt) {
    if (!out || n_nodes <= 0 || n_tets < 0 || !points_in || !cells_in || !bc_mask_in || !bc_val_in) {
        set_error("sns_create: null or empty input");
        return SNS_E_ARG;
    }
    *out = nullptr;
    if (opt) SNS_TRY(check_aggregation_option(dim, *opt));
    const int npe = dim + 1;
    // host validation: vertex ids in range, non-degenerate cells (kernels divide by det J)
    for (int64_t t = 0; t < n_tets; ++t) {
        const int32_t* v = cells_in + npe * t;
        for (int a = 0; a < npe; ++a)
            if (v[a] < 0 || v[a] >= n_nodes) { set_error("cell vertex id out of range"); return SNS_E_MESH; }
        const double* x0 = points_in + dim * (int64_t)v[0];
        double J[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        for (int c = 0; c < dim; ++c)
            for (int i = 0; i < dim; ++i) J[i][c] = points_in[dim * (int64_t)v[c + 1] + i] - x0[i];
        const double det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) -
                           J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
                           J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
        if (!(std::fabs(det) > 0.0)) { set_error("degenerate cell " + std::to_string(t)); return SNS_E_MESH; }
    }
    // device layout is the 3-D one in both cases: points in a stride of 3, cells in a stride of 4 (a triangle repeats
    // its last vertex), 4 dofs per node; a 2-D handle constrains the unused z component to 0
    std::vector<double> pts3;
    std::vector<int32_t> cells4;
    std::vector<uint8_t> mask2;
    std::vector<double> val2;
    const double* points = points_in;
    const int32_t* tets = cells_in;
    const uint8_t* bc_mask = bc_mask_in;
    const double* bc_val = bc_val_in;
    if (dim == 2) {
        pts3.assign((size_t)3 * n_nodes, 0.0);
        for (int32_t i = 0; i < n_nodes; ++i) { pts3[3 * (size_t)i] = points_in[2 * (size_t)i]; pts3[3 * (size_t)i + 1] = points_in[2 * (size_t)i + 1]; }
        cells4.resize((size_t)4 * n_tets);
        for (int64_t t = 0; t < n_tets; ++t) {
            for (int a = 0; a < 3; ++a) cells4[4 * (size_t)t + a] = cells_in[3 * t + a];
            cells4[4 * (size_t)t + 3] = cells_in[3 * t + 2];
        }
        mask2.assign(bc_mask_in, bc_mask_in + (size_t)4 * n_nodes);
        val2.assign(bc_val_in, bc_val_in + (size_t)4 * n_nodes);
        for (int32_t i = 0; i < n_nodes; ++i) { mask2[4 * (size_t)i + 2] = 1; val2[4 * (size_t)i + 2] = 0.0; }
        points = pts3.data(); tets = cells4.data(); bc_mask = mask2.data(); bc_val = val2.data();
    }
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<sns_ctx> h(new sns_ctx);
    if (opt) h->opt = *opt; else sns_default_options(&h->opt);
    h->device = device;
    h->dim = dim;
    h->n = n_nodes;
    h->n_owned = n_nodes;
    h->E = n_tets;
    HostPattern P;
    HostAssemblyMaps M;
    try {
        build_pattern(n_nodes, n_tets, tets, P, M, npe);
    } catch (const std::exception& e) {
        set_error(e.what());
        return SNS_E_MESH;
    }
    SNS_TRY(h->tets.alloc((size_t)4 * n_tets));
    HIP_TRY(hipMemcpy(h->tets, tets, (size_t)4 * n_tets * sizeof(int32_t), hipMemcpyHostToDevice));
    SNS_TRY(h->pts.alloc((size_t)3 * n_nodes));
    HIP_TRY(hipMemcpy(h->pts, points, (size_t)3 * n_nodes * sizeof(double), hipMemcpyHostToDevice));
    SNS_TRY(h->bc_mask.alloc((size_t)4 * n_nodes));
    HIP_TRY(hipMemcpy(h->bc_mask, bc_mask, (size_t)4 * n_nodes, hipMemcpyHostToDevice));
    SNS_TRY(h->bc_val.alloc((size_t)4 * n_nodes));
    HIP_TRY(hipMemcpy(h->bc_val, bc_val, (size_t)4 * n_nodes * sizeof(double), hipMemcpyHostToDevice));
    {
        std::vector<double> ge((size_t)4 * n_nodes);
        for (size_t i = 0; i < ge.size(); ++i) ge[i] = bc_mask[i] ? bc_val[i] : 0.0;
        SNS_TRY(h->gext.upload(ge));
    }
    SNS_TRY(h->nt_ptr.upload(M.nt_ptr));
    SNS_TRY(h->nt_idx.upload(M.nt_idx));
    SNS_TRY(h->c_ptr.upload(M.c_ptr));
    SNS_TRY(h->c_idx.upload(M.c_idx));
    {
        // lane -> slot map of the scratch-free assembly: off-diagonal slots only, and inside every window of
        // 8192 consecutive slots ordered by descending contribution count, so that the lanes of a wave loop
        // the same number of times (edge valences differ: 4 or 6 tets on a Kuhn mesh) while their gathers
        // stay within the same neighbourhood of the mesh
        const int64_t nnzb = (int64_t)P.colind.size(), WIN = 8192;
        std::vector<int32_t> order;
        order.reserve((size_t)nnzb);
        std::vector<int32_t> row_of((size_t)nnzb);
        for (int32_t i = 0; i < P.n; ++i)
            for (int32_t q = P.rowptr[i]; q < P.rowptr[i + 1]; ++q) row_of[(size_t)q] = i;
        std::vector<std::vector<int32_t>> bucket;
        for (int64_t s0 = 0; s0 < nnzb; s0 += WIN) {
            const int64_t s1 = std::min(nnzb, s0 + WIN);
            for (auto& b : bucket) b.clear();
            for (int64_t q = s0; q < s1; ++q) {
                if (P.colind[(size_t)q] == row_of[(size_t)q]) continue;
                const size_t cnt = (size_t)(M.c_ptr[(size_t)q + 1] - M.c_ptr[(size_t)q]);
                if (bucket.size() <= cnt) bucket.resize(cnt + 1);
                bucket[cnt].push_back((int32_t)q);
            }
            for (size_t c = bucket.size(); c-- > 0;) order.insert(order.end(), bucket[c].begin(), bucket[c].end());
        }
        h->n_od = (int64_t)order.size();
        SNS_TRY(h->od_order.upload(order));
    }
    h->levels.emplace_back();
    SNS_TRY(upload_pattern(h->levels[0], P, nullptr));
    h->levels[0].n_owned = n_nodes;
    SNS_TRY(alloc_level_vectors(h->levels[0]));
    SNS_TRY(h->levels[0].pong.alloc(4 * (size_t)n_nodes));
    HIP_TRY(hipMemset(h->levels[0].pong, 0, 4 * (size_t)n_nodes * sizeof(double)));
    {   // free mask of level 0 = !bc
        std::vector<uint8_t> fm((size_t)4 * n_nodes);
        for (size_t i = 0; i < fm.size(); ++i) fm[i] = bc_mask[i] ? 0 : 1;
        SNS_TRY(h->levels[0].free_mask.upload(fm));
    }
    // per-block partial sums: vector kernels use <= 2048 blocks x <= 8 sums, the fused SpMV+dot one block per 32 rows
    SNS_TRY(h->partial.alloc(std::max<size_t>((size_t)65536 * 8, (size_t)n_nodes / 4 + 512)));
    SNS_TRY(h->partial2.alloc((size_t)4096 * 8));
    SNS_TRY(h->d_scal.alloc(256));
    SNS_TRY(h->d_sing.alloc(1));
    HIP_TRY(hipMemset(h->d_sing, 0, sizeof(int)));
    HIP_TRY(hipHostMalloc((void**)h->h_scal.put(), 1024 * sizeof(double), hipHostMallocDefault));
    HIP_TRY(hipEventCreate(h->ev0.put()));
    HIP_TRY(hipEventCreate(h->ev1.put()));
    // the hierarchy is built lazily (first pc_setup) so that sns_attach_comm can shrink n_owned first
    HIP_TRY(hipDeviceSynchronize());
    h->tm = sns_timings{};
    h->graph_disabled = std::getenv("SNS_NO_GRAPH") != nullptr;
    h->r3_estimates = std::getenv("SNS_R3_SPECTRAL_ESTIMATE") != nullptr;
    h->plain_step = std::getenv("SNS_PLAIN_STEP") != nullptr;
    h->pattern.reset(new HostPattern(std::move(P)));
    h->host_pts.assign(points, points + (size_t)3 * n_nodes);
    SNS_TRY(plan_hierarchy(h.get()));                     // (the fine level alone until the hierarchy is built)
    *out = h.release();
    return SNS_OK;
}


int sns_create(sns_handle* out, int32_t n_nodes, int64_t n_tets, const double* points, const int32_t* tets,
               const uint8_t* bc_mask, const double* bc_val, int device, const sns_options* opt) {
    return create_common(3, out, n_nodes, n_tets, points, tets, bc_mask, bc_val, device, opt);
}

int sns_create_2d(sns_handle* out, int32_t n_nodes, int64_t n_tris, const double* points, const int32_t* tris,
                  const uint8_t* bc_mask, const double* bc_val, int device, const sns_options* opt) {
    return create_common(2, out, n_nodes, n_tris, points, tris, bc_mask, bc_val, device, opt);
}


}  // extern "C"


namespace {

// A verdict of csrc/sns_policy.h as the error of the entry point `who`
int refused(const char* who, const policy::Verdict& v) {
    if (v.error != SNS_OK) set_error(std::string(who) + ": " + v.tail);
    return v.error;
}
// THE gate: the handle's answer to `request` of `family` (the table policy::RULES, asked with facts_of(h)).  A family's
// dimension row (SNS_E_ARG) stands among the argument checks of some entry points, its state rows (SNS_E_STATE) after them:
// ROWS_ARG / ROWS_STATE ask for one kind, so that a call with two things wrong reports what it always reported.
using policy::ROWS_ALL;
using policy::ROWS_ARG;
using policy::ROWS_STATE;
int allows(const sns_ctx* h, const char* who, policy::Family family, int request, policy::Rows rows = ROWS_ALL) {
    return refused(who, policy::check_request(family, request, facts_of(h), rows));
}

}  // namespace


extern "C" {


int sns_destroy(sns_handle h) {
    if (!h) return SNS_OK;
    delete h;                                             // (~sns_ctx, csrc/sns_ctx.h)
    return SNS_OK;
}


int sns_set_stream(sns_handle h, void* s) {
    if (!h) return SNS_E_ARG;
    h->stream = (hipStream_t)s;
    return SNS_OK;
}

int sns_set_options(sns_handle h, const sns_options* o) {
    if (!h || !o) return SNS_E_ARG;
    SNS_TRY(check_aggregation_option(h->dim, *o));
    const bool pc_changed = (o->pc_type != h->opt.pc_type) || (o->amg_f32_matrix != h->opt.amg_f32_matrix) ||
                            (o->amg_fused_post != h->opt.amg_fused_post) || (o->amg_block_smooth != h->opt.amg_block_smooth);
    const bool damping_changed = (o->amg_omega != h->opt.amg_omega);
    const bool sweep_exchange_changed = (o->amg_sweep_exchange_rows != h->opt.amg_sweep_exchange_rows) ||
                                        (o->amg_post_exchange != h->opt.amg_post_exchange) ||
                                        (o->amg_fused_post != h->opt.amg_fused_post) || (o->amg_f32_matrix != h->opt.amg_f32_matrix) ||
                                        (o->pc_type != h->opt.pc_type);
    h->opt = *o;
    damping_reset(h, DampingReset::AFTER_RETRY);      // a retry's stronger damping does not outlive an options call
    if (sweep_exchange_changed) {
        // rank-local sweeps rely on ghost tails that are never written (zero); sweeps with exchanges fill them
        HIP_TRY(hipStreamSynchronize(h->stream));
        for (size_t l = 0; l < h->levels.size(); ++l) {
            Level& L = h->levels[l];
            const size_t nb = 4 * (size_t)L.n * sizeof(double);
            if (L.x) HIP_TRY(hipMemset(L.x, 0, nb));
            if (L.pong) HIP_TRY(hipMemset(L.pong, 0, nb));
        }
    }
    h->plan = policy::plan_cycle(h->opt, h->facts);         // (the stored facts: no communication)
    if (pc_changed || damping_changed || plan_buffer_missing(h)) h->pc_ready = false;
    if (damping_changed || pc_changed) damping_reset(h, DampingReset::ESTIMATES);   // re-estimate and re-verify
    return SNS_OK;
}

int sns_set_form_variant(sns_handle h, double c_inverse, double lsic_scale, double pspg_sign, int one_point_quadrature) {
    if (!h) return SNS_E_ARG;
    SNS_TRY(allows(h, "sns_set_form_variant", policy::FAMILY_FORM, policy::REQ_FORM_VARIANT));
    return set_form_variant(h, c_inverse, lsic_scale, pspg_sign, one_point_quadrature);
}

int sns_get_options(sns_handle h, sns_options* o) {
    if (!h || !o) return SNS_E_ARG;
    *o = h->opt;
    return SNS_OK;
}

int sns_get_sizes(sns_handle h, int32_t* nl, int32_t* no, int64_t* nt, int64_t* nnzb) {
    if (!h) return SNS_E_ARG;
    if (nl) *nl = h->n;
    if (no) *no = h->n_owned;
    if (nt) *nt = h->E;
    if (nnzb) *nnzb = h->levels[0].nnzb;
    return SNS_OK;
}


int sns_comm_unique_id(char id_out[128]) {
    ncclUniqueId id;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    NCCL_TRY(ncclGetUniqueId(&id));
    std::memcpy(id_out, &id, 128);
    return SNS_OK;
}


static int attach_common(sns_handle h, int rank, int nranks, const char* uid, Team* team, Peer* peer, int32_t n_owned, int n_nbr,
                         const int32_t* nbr, const int32_t* send_ptr, const int32_t* send_idx,
                         const int32_t* recv_ptr, const int32_t* recv_idx) {
    if (!h || nranks < 1 || rank < 0 || rank >= nranks || n_owned < 0 || n_owned > h->n || n_nbr < 0 ||
        (n_nbr > 0 && (!nbr || !send_ptr || !recv_ptr))) {
        set_error("sns_attach_comm: bad arguments");
        return SNS_E_ARG;
    }
    if (h->has_matrix || !h->pattern) {
        set_error("sns_attach_comm must directly follow sns_create");
        return SNS_E_STATE;
    }
    HIP_TRY(hipSetDevice(h->device));
    h->comm.reset(new Comm);
    Comm& c = *h->comm;
    c.rank = rank;
    c.nranks = nranks;
    c.team = team;
    c.peer = peer;
    if (team) SNS_TRY(team_peer(team, h->device, rank, &c.peer));      // (the team runs the peer transport's kernels, sns_comm.h)
    if (uid) {
        ncclUniqueId id;
        std::memcpy(&id, uid, 128);
        NCCL_TRY(ncclCommInitRank(&c.nccl, nranks, id, rank));
    }   // uid == NULL and no team: local part only, the caller moves ghost values and reduces (tests)
    h->n_owned = n_owned;
    h->levels[0].n_owned = n_owned;
    c.plans.emplace_back();
    Plan& p = c.plans[0];
    p.n_own = n_owned;
    p.nbr.assign(nbr, nbr + n_nbr);
    if (n_nbr > 0) {
        p.send_ptr.assign(send_ptr, send_ptr + n_nbr + 1);
        p.recv_ptr.assign(recv_ptr, recv_ptr + n_nbr + 1);
    } else {
        p.send_ptr.assign(1, 0);
        p.recv_ptr.assign(1, 0);
    }
    const int32_t ns = p.n_send(), nr = p.n_recv();
    for (int32_t i = 0; i < ns; ++i)
        if (send_idx[i] < 0 || send_idx[i] >= n_owned) { set_error("send_idx outside owned range"); return SNS_E_ARG; }
    for (int32_t i = 0; i < nr; ++i)
        if (recv_idx[i] < n_owned || recv_idx[i] >= h->n) { set_error("recv_idx outside ghost range"); return SNS_E_ARG; }
    p.h_send_idx.assign(send_idx, send_idx + ns);
    p.h_recv_idx.assign(recv_idx, recv_idx + nr);
    SNS_TRY(plan_upload(p));
    {
        // owned rows that reference a ghost column: the only rows of a level-0 pass that must wait for the halo
        const HostPattern& P = *h->pattern;
        std::vector<int32_t> rows((size_t)std::max(1, n_owned), 0);
        std::vector<uint8_t> flag((size_t)std::max(1, n_owned), 0);
        int32_t nb = 0;
        SNS_TRY(sns_host_boundary_rows(n_owned, P.rowptr.data(), P.colind.data(), rows.data(), &nb));
        for (int32_t q = 0; q < nb; ++q) flag[rows[q]] = 1;
        h->n_bnd = nb;
        rows.resize((size_t)std::max(1, nb));
        SNS_TRY(h->bnd_rows.upload(rows));
        SNS_TRY(h->bnd_flag.upload(flag));
        h->no_overlap = std::getenv("SNS_NO_OVERLAP") != nullptr;
        h->team_overlap = std::getenv("SNS_TEAM_OVERLAP") != nullptr;
    }
    if (!c.active()) {
        // no transport: the per-rank hierarchy must not reference ghost dofs at all
        std::vector<uint8_t> fm((size_t)4 * h->n);
        HIP_TRY(hipMemcpy(fm.data(), h->levels[0].free_mask, fm.size(), hipMemcpyDeviceToHost));
        for (size_t i = (size_t)4 * n_owned; i < fm.size(); ++i) fm[i] = 0;
        HIP_TRY(hipMemcpy(h->levels[0].free_mask, fm.data(), fm.size(), hipMemcpyHostToDevice));
    }
    // first collective of the communicator: both ends of every link agree on its counts (the coarse levels' plans are
    // checked the same way when the hierarchy derives them)
    SNS_TRY(check_plan_symmetry(h, c.plans[0], 0));
    SNS_TRY(connect_plan(h, c.plans[0]));
    return plan_hierarchy(h);                            // (the fine level alone until the hierarchy is built)
}


int sns_attach_comm(sns_handle h, int rank, int nranks, const char uid[128], int32_t n_owned, int n_nbr,
                    const int32_t* nbr, const int32_t* send_ptr, const int32_t* send_idx, const int32_t* recv_ptr,
                    const int32_t* recv_idx) {
    return attach_common(h, rank, nranks, uid, nullptr, nullptr, n_owned, n_nbr, nbr, send_ptr, send_idx, recv_ptr, recv_idx);
}


int sns_team_create(int nranks, void** team_out) {
    if (nranks < 1 || !team_out) return SNS_E_ARG;
    *team_out = new Team(nranks);
    return SNS_OK;
}

int sns_team_destroy(void* team) {
    delete static_cast<Team*>(team);
    return SNS_OK;
}

int sns_attach_team(sns_handle h, void* team, int rank, int nranks, int32_t n_owned, int n_nbr, const int32_t* nbr,
                    const int32_t* send_ptr, const int32_t* send_idx, const int32_t* recv_ptr,
                    const int32_t* recv_idx) {
    if (!team || static_cast<Team*>(team)->n != nranks) { set_error("sns_attach_team: bad team"); return SNS_E_ARG; }
    return attach_common(h, rank, nranks, nullptr, static_cast<Team*>(team), nullptr, n_owned, n_nbr, nbr, send_ptr, send_idx,
                         recv_ptr, recv_idx);
}


int sns_peer_create(int device, int rank, int nranks, int64_t window_bytes, void** peer_out, char ipc_handle_out[64]) {
    if (!peer_out || window_bytes < 0) return SNS_E_ARG;
    Peer* p = nullptr;
    SNS_TRY(peer_create(device, rank, nranks, (size_t)window_bytes, &p, ipc_handle_out));
    *peer_out = p;
    return SNS_OK;
}

int sns_peer_connect(void* peer, const char* ipc_handles) { return peer_connect(static_cast<Peer*>(peer), ipc_handles); }

int sns_peer_disconnect(void* peer) { return peer_close_mappings(static_cast<Peer*>(peer)); }

int sns_peer_destroy(void* peer) { return peer_destroy(static_cast<Peer*>(peer)); }

int sns_peer_check_links(void* peer, int rounds) { return peer_check_links(static_cast<Peer*>(peer), rounds); }

int sns_peer_selftest(int device, int nranks, int halo_nodes, int reps, double us_out[3]) {
    return peer_selftest(device, nranks, halo_nodes, reps, us_out);
}

int sns_attach_peer(sns_handle h, void* peer, int32_t n_owned, int n_nbr, const int32_t* nbr, const int32_t* send_ptr,
                    const int32_t* send_idx, const int32_t* recv_ptr, const int32_t* recv_idx) {
    Peer* p = static_cast<Peer*>(peer);
    if (!p || !p->connected) { set_error("sns_attach_peer: the peer communicator is not connected"); return SNS_E_ARG; }
    if (h && h->device != p->device) { set_error("sns_attach_peer: handle and window live on different devices"); return SNS_E_ARG; }
    return attach_common(h, p->rank, p->nranks, nullptr, nullptr, p, n_owned, n_nbr, nbr, send_ptr, send_idx, recv_ptr, recv_idx);
}


int sns_residual(sns_handle h, int form, const double* w, double* F) {
    if (!h || !F) return SNS_E_ARG;
    return timed_assemble(h, form, w, F, false);
}

int sns_jacobian(sns_handle h, int form, const double* w, double* F) {
    if (!h) return SNS_E_ARG;
    return timed_assemble(h, form, w, F, true);
}

int sns_residual_moments(sns_handle h, int form, const double* w, const double* phi, double out[4]) {
    if (!h || !phi || !out) { set_error("sns_residual_moments: null handle or pointer"); return SNS_E_ARG; }
    if (form != SNS_FORM_STOKES && form != SNS_FORM_NS) { set_error("bad form"); return SNS_E_ARG; }
    if (form == SNS_FORM_NS && !w) { set_error("NS form needs a state vector"); return SNS_E_ARG; }
    if (h->E == 0) { set_error("empty mesh"); return SNS_E_ARG; }
    return residual_moments(h, form, w, phi, out);
}

int sns_residual_shape_gradient(sns_handle h, int form, const double* w, const double* lam, double* gX) {
    if (!h || !w || !lam || !gX) { set_error("sns_residual_shape_gradient: null handle or pointer"); return SNS_E_ARG; }
    if (form != SNS_FORM_NS) {
        set_error(form == SNS_FORM_STOKES ? "sns_residual_shape_gradient: the Stokes forms are not supported" : "bad form");
        return SNS_E_ARG;
    }
    SNS_TRY(allows(h, "sns_residual_shape_gradient", policy::FAMILY_FORM, policy::REQ_SHAPE_GRADIENT));
    return residual_shape_gradient(h, w, lam, gX);
}

int sns_recover_gradient(sns_handle h, const double* w, double* G, double* D) {
    if (!h || !w || (!G && !D)) { set_error("sns_recover_gradient: null handle, state or both outputs null"); return SNS_E_ARG; }
    SNS_TRY(allows(h, "sns_recover_gradient", policy::FAMILY_FORM, policy::REQ_RECOVER_GRADIENT));
    return recover_gradient(h, w, G, D);
}

int sns_error_indicator(sns_handle h, const double* w, const double* G, double* eta2, double* gnorm2) {
    if (!h || !w || !eta2) { set_error("sns_error_indicator: null handle, state or eta2"); return SNS_E_ARG; }
    SNS_TRY(allows(h, "sns_error_indicator", policy::FAMILY_FORM, policy::REQ_ERROR_INDICATOR));
    return error_indicator(h, w, G, eta2, gnorm2);
}

int sns_mass_apply(sns_handle h, const double* w, const double* x, double* y) {
    if (!h || !w || !x || !y) { set_error("sns_mass_apply: null handle or pointer"); return SNS_E_ARG; }
    SNS_TRY(allows(h, "sns_mass_apply", policy::FAMILY_STABILITY, policy::SREQ_MASS_APPLY));
    return mass_apply(h, w, x, y);
}

int sns_mass_apply_transpose(sns_handle h, const double* w, const double* z, double* y) {
    if (!h || !w || !z || !y) { set_error("sns_mass_apply_transpose: null handle or pointer"); return SNS_E_ARG; }
    SNS_TRY(allows(h, "sns_mass_apply_transpose", policy::FAMILY_STABILITY, policy::SREQ_MASS_APPLY_TRANSPOSE));
    return mass_apply_transpose(h, w, z, y);
}

int sns_jacobian_state_gradient(sns_handle h, const double* w, const double* x, const double* z, double c_jac, double c_mass,
                                double* g) {
    const char* who = "sns_jacobian_state_gradient";
    if (!h || !w || !x || !z || !g) { set_error("sns_jacobian_state_gradient: null handle or pointer"); return SNS_E_ARG; }
    SNS_TRY(allows(h, who, policy::FAMILY_STATE_GRADIENT, policy::GREQ_STATE_GRADIENT, ROWS_ARG));
    SNS_TRY(refused(who, policy::check_state_gradient_args(c_jac, c_mass)));
    SNS_TRY(allows(h, who, policy::FAMILY_STATE_GRADIENT, policy::GREQ_STATE_GRADIENT, ROWS_STATE));
    return jacobian_state_gradient(h, w, x, z, c_jac, c_mass, g);
}

int sns_jacobian_shape_gradient(sns_handle h, const double* w, const double* x, const double* z, double c_jac, double c_mass,
                                double* gX) {
    const char* who = "sns_jacobian_shape_gradient";
    if (!h || !w || !x || !z || !gX) { set_error("sns_jacobian_shape_gradient: null handle or pointer"); return SNS_E_ARG; }
    SNS_TRY(allows(h, who, policy::FAMILY_STATE_GRADIENT, policy::GREQ_STATE_GRADIENT, ROWS_ARG));
    SNS_TRY(refused(who, policy::check_state_gradient_args(c_jac, c_mass)));
    SNS_TRY(allows(h, who, policy::FAMILY_STATE_GRADIENT, policy::GREQ_STATE_GRADIENT, ROWS_STATE));
    return jacobian_shape_gradient(h, w, x, z, c_jac, c_mass, gX);
}

int sns_raw_jacobian_apply(sns_handle h, int form, const double* w, const double* x, int transposed, double* y) {
    const char* who = "sns_raw_jacobian_apply";
    if (!h || !w || !x || !y) { set_error("sns_raw_jacobian_apply: null handle or pointer"); return SNS_E_ARG; }
    SNS_TRY(allows(h, who, policy::FAMILY_RAW_JACOBIAN, policy::JREQ_APPLY, ROWS_ARG));
    SNS_TRY(refused(who, policy::check_raw_jacobian_args({form, x == y, !h->form.fv.is_default()})));
    SNS_TRY(allows(h, who, policy::FAMILY_RAW_JACOBIAN, policy::JREQ_APPLY, ROWS_STATE));
    return raw_jacobian_apply(h, w, x, transposed != 0, y);
}

// The values alone move: the mask, and with it the pattern, the free mask of the hierarchy and every assembled value, stay.
// bc_val and gext are the two buffers derived from the values; every kernel reads them at its launch, nothing caches them.
int sns_set_dirichlet_values(sns_handle h, const double* bc_val_host) {
    const char* who = "sns_set_dirichlet_values";
    if (!h || !bc_val_host) { set_error("sns_set_dirichlet_values: null handle or pointer"); return SNS_E_ARG; }
    SNS_TRY(allows(h, who, policy::FAMILY_RAW_JACOBIAN, policy::JREQ_SET_DIRICHLET));
    const size_t nd = (size_t)ld_of(h);
    std::vector<uint8_t> mask(nd);
    std::vector<double> val(nd), ge(nd);
    SNS_TRY(sync_stream(h));                                // (kernels queued before the call read the old values)
    HIP_TRY(hipMemcpy(mask.data(), h->bc_mask, nd, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(val.data(), h->bc_val, nd * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < nd; ++i) {
        if (mask[i]) {
            const double g = (h->dim == 2 && (i & 3) == 2) ? 0.0 : bc_val_host[i];      // the unused z component of a 2-D handle
            if (!(g - g == 0.0)) { set_error("sns_set_dirichlet_values: non-finite value on a constrained dof"); return SNS_E_ARG; }
            val[i] = g;
        }
        ge[i] = mask[i] ? val[i] : 0.0;
    }
    HIP_TRY(hipMemcpy(h->bc_val, val.data(), nd * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->gext, ge.data(), nd * sizeof(double), hipMemcpyHostToDevice));
    return SNS_OK;
}

// the checks of the Arnoldi entry points and the run (`who`: the name in front of the message; args: the outcome of the
// argument rule of the entry point, reported between the two halves of the state's rules; c: the shifted step's coefficient)
// The verdict is formed by the caller before the pointers are looked at: an argument rule reads scalars and dereferences nothing
static int arnoldi_checked(const char* who, sns_ctx* h, bool left, const policy::Verdict& args, const double* w, double shift, int k,
                           int m, double breakdown_rel, double* V, double* H, int* m_done, int* total_ksp_its, int* reason,
                           const double* c = nullptr) {
    if (!h || !w || !V || !H || !m_done || !total_ksp_its || !reason) {
        set_error(std::string(who) + ": null handle or pointer");
        return SNS_E_ARG;
    }
    const policy::StabilityRequest request = left ? policy::SREQ_ARNOLDI_LEFT : policy::SREQ_ARNOLDI;
    SNS_TRY(allows(h, who, policy::FAMILY_STABILITY, request, ROWS_ARG));
    SNS_TRY(refused(who, args));
    SNS_TRY(allows(h, who, policy::FAMILY_STABILITY, request, ROWS_STATE));
    return sns::stability_arnoldi(h, w, shift, left, k, m, breakdown_rel, V, H, m_done, total_ksp_its, reason, c);
}

int sns_stability_arnoldi(sns_handle h, const double* w, double shift, int m, double breakdown_rel, double* V, double* H, int* m_done,
                          int* total_ksp_its, int* reason) {
    return arnoldi_checked("sns_stability_arnoldi", h, false, policy::check_arnoldi_args({m, shift, breakdown_rel}), w, shift, 0, m,
                           breakdown_rel, V, H, m_done, total_ksp_its, reason);
}

int sns_stability_arnoldi_left(sns_handle h, const double* w, double shift, int m, double breakdown_rel, double* V, double* H,
                               int* m_done, int* total_ksp_its, int* reason) {
    return arnoldi_checked("sns_stability_arnoldi_left", h, true, policy::check_arnoldi_args({m, shift, breakdown_rel}), w, shift, 0, m,
                           breakdown_rel, V, H, m_done, total_ksp_its, reason);
}

int sns_stability_arnoldi_extend(sns_handle h, const double* w, double shift, int k, int m, double breakdown_rel, int left, double* V,
                                 double* H, int* m_done, int* total_ksp_its, int* reason) {
    return arnoldi_checked("sns_stability_arnoldi_extend", h, left != 0, policy::check_arnoldi_extend_args({m, shift, breakdown_rel}, k), w,
                           shift, k, m, breakdown_rel, V, H, m_done, total_ksp_its, reason);
}

int sns_stability_arnoldi_shifted(sns_handle h, const double* w, double shift_re, double shift_im, double pc_shift, int k, int m,
                                  double breakdown_rel, int left, double* V, double* H, int* m_done, int* total_ksp_its, int* reason) {
    const double c[2] = {shift_re - pc_shift, shift_im};   // J + s B = (J + pc_shift B) + c B
    return arnoldi_checked("sns_stability_arnoldi_shifted", h, left != 0,
                           policy::check_shifted_args({m, k, shift_re, shift_im, pc_shift, breakdown_rel}), w, pc_shift, k, m, breakdown_rel,
                           V, H, m_done, total_ksp_its, reason, c);
}

// the checks of the two calls on the complex operator A + c B (`who`: the name in front of the message)
static int shifted_operator_checked(const char* who, sns_ctx* h, bool pointers, double c_re, double c_im, int transpose) {
    if (!h || !pointers) { set_error(std::string(who) + ": null handle or pointer"); return SNS_E_ARG; }
    const policy::StabilityRequest request = transpose ? policy::SREQ_MASS_APPLY_TRANSPOSE : policy::SREQ_MASS_APPLY;
    SNS_TRY(allows(h, who, policy::FAMILY_STABILITY, request, ROWS_ARG));
    SNS_TRY(refused(who, policy::check_shifted_coefficient(c_re, c_im)));
    SNS_TRY(allows(h, who, policy::FAMILY_STABILITY, request, ROWS_STATE));
    if (!h->has_matrix) { set_error(std::string(who) + " before a matrix was assembled"); return SNS_E_STATE; }
    return SNS_OK;
}

int sns_shifted_apply(sns_handle h, const double* w, double c_re, double c_im, int transpose, const double* x, double* y) {
    SNS_TRY(shifted_operator_checked("sns_shifted_apply", h, w && x && y, c_re, c_im, transpose));
    return shifted_apply(h, w, c_re, c_im, transpose != 0, x, y);
}

int sns_shifted_solve(sns_handle h, const double* w, double c_re, double c_im, int transpose, const double* b, double* x, int* its,
                      int* reason, double* rnorm) {
    SNS_TRY(shifted_operator_checked("sns_shifted_solve", h, w && b && x && its && reason && rnorm, c_re, c_im, transpose));
    SNS_TRY(ensure_hierarchy(h));
    return shifted_solve(h, w, c_re, c_im, transpose != 0, b, x, its, reason, rnorm);
}

int sns_energy_apply(sns_handle h, const double* chi, int parts, const double* x, double* y) {
    const char* who = "sns_energy_apply";
    if (!h || !x || !y) { set_error("sns_energy_apply: null handle or pointer"); return SNS_E_ARG; }
    SNS_TRY(allows(h, who, policy::FAMILY_RESOLVENT, policy::RREQ_ENERGY, ROWS_ARG));
    SNS_TRY(refused(who, policy::check_energy_args({parts, x == y})));
    SNS_TRY(allows(h, who, policy::FAMILY_RESOLVENT, policy::RREQ_ENERGY, ROWS_STATE));
    return energy_apply(h, chi, parts, x, y);
}

int sns_lumped_volumes(sns_handle h, double* m) {
    if (!h || !m) { set_error("sns_lumped_volumes: null handle or pointer"); return SNS_E_ARG; }
    SNS_TRY(allows(h, "sns_lumped_volumes", policy::FAMILY_RESOLVENT, policy::RREQ_ENERGY));
    return lumped_volumes(h, m);
}

int sns_resolvent_lanczos(sns_handle h, const double* w, double omega, int m, double breakdown_rel, const double* chi_f,
                          const double* chi_q, double* V, double* H, int* m_done, int* total_ksp_its, int* reason) {
    const char* who = "sns_resolvent_lanczos";
    if (!h || !w || !V || !H || !m_done || !total_ksp_its || !reason) {
        set_error("sns_resolvent_lanczos: null handle or pointer");
        return SNS_E_ARG;
    }
    SNS_TRY(allows(h, who, policy::FAMILY_RESOLVENT, policy::RREQ_LANCZOS, ROWS_ARG));
    SNS_TRY(refused(who, policy::check_resolvent_args({m, omega, breakdown_rel, V == w || V == chi_f || V == chi_q})));
    SNS_TRY(allows(h, who, policy::FAMILY_RESOLVENT, policy::RREQ_LANCZOS, ROWS_STATE));
    return resolvent_lanczos(h, w, omega, m, breakdown_rel, chi_f, chi_q, V, H, m_done, total_ksp_its, reason);
}

int sns_basis_rotate(sns_handle h, int n_in, int n_out, const double* Q, double* V) {
    const char* who = "sns_basis_rotate";
    if (!h || !Q || !V) { set_error("sns_basis_rotate: null handle or pointer"); return SNS_E_ARG; }
    if (n_in < 1 || n_in > policy::STABILITY_M_MAX + 1) { set_error(std::string(who) + ": n_in must lie in [1, 65]"); return SNS_E_ARG; }
    if (n_out < 1 || n_out > n_in) { set_error(std::string(who) + ": n_out must lie in [1, n_in]"); return SNS_E_ARG; }
    for (int t = 0; t < n_in * n_out; ++t)
        if (!(Q[t] - Q[t] == 0.0)) { set_error(std::string(who) + ": non-finite entry of Q"); return SNS_E_ARG; }
    return basis_rotate(h, n_in, n_out, Q, V);
}

int sns_spmv(sns_handle h, const double* x, double* y) {
    if (!h || !x || !y) return SNS_E_ARG;
    if (!h->has_matrix) { set_error("spmv before a matrix was assembled"); return SNS_E_STATE; }
    SNS_TRY(op_apply(h, const_cast<double*>(x), y));
    return sync_stream(h);
}

int sns_pc_setup(sns_handle h) {
    if (!h) return SNS_E_ARG;
    SNS_TRY(ensure_hierarchy(h));
    return pc_setup(h);
}

int sns_pc_apply(sns_handle h, const double* r, double* z) {
    if (!h || !r || !z) return SNS_E_ARG;
    if (!h->pc_ready && h->opt.pc_type != SNS_PC_NONE) { set_error("pc_apply before pc_setup"); return SNS_E_STATE; }
    SNS_TRY(pc_apply(h, r, z));
    return sync_stream(h);
}

int sns_krylov_solve(sns_handle h, const double* b, double* x, int* its, int* reason, double* rnorm) {
    if (!h || !b || !x || !its || !reason || !rnorm) return SNS_E_ARG;
    SNS_TRY(ensure_hierarchy(h));
    return krylov(h, b, x, its, reason, rnorm);
}


int sns_transpose_operator(sns_handle h) {
    if (!h) return SNS_E_ARG;
    return transpose_operator(h);
}

int sns_operator_is_transposed(sns_handle h, int* flag) {
    if (!h || !flag) return SNS_E_ARG;
    *flag = h->transposed ? 1 : 0;
    return SNS_OK;
}

int sns_adjoint_solve(sns_handle h, const double* g, double* lam, int* its, int* reason, double* rnorm) {
    if (!h || !g || !lam || !its || !reason || !rnorm) return SNS_E_ARG;
    return adjoint_solve(h, g, lam, its, reason, rnorm);
}

int sns_stokes_solve(sns_handle h, double* U, int* ksp_its, int* reason, double* rnorm) {
    if (!h || !U || !ksp_its || !reason || !rnorm) return SNS_E_ARG;
    return stokes_solve(h, U, ksp_its, reason, rnorm);
}

// the checks of the two scalar-transport entry points (`who`: the name in front of the message)
static int scalar_check(const char* who, sns_ctx* h, const double* w, const double* kappa, double sigma, double theta,
                        const uint8_t* cmask, const double* cval, const void* out) {
    const std::string name(who);
    if (!h || !w || !kappa || !cmask || !cval || !out) { set_error(name + ": null handle or pointer"); return SNS_E_ARG; }
    SNS_TRY(allows(h, who, policy::FAMILY_FORM, policy::REQ_SCALAR, ROWS_ARG));
    for (int k = 0; k < 4; ++k)
        if (!(kappa[k] > 0.0) || !std::isfinite(kappa[k])) { set_error(name + ": every kappa must be finite and > 0"); return SNS_E_ARG; }
    if (!(sigma >= 0.0) || !std::isfinite(sigma) || !(theta >= 0.0) || !std::isfinite(theta)) {
        set_error(name + ": sigma and theta must be finite and >= 0");
        return SNS_E_ARG;
    }
    return allows(h, who, policy::FAMILY_FORM, policy::REQ_SCALAR, ROWS_STATE);
}

int sns_scalar_system(sns_handle h, const double* w_dev, const double kappa[4], double sigma, double theta, const double* src_dev,
                      const uint8_t* cmask_dev, const double* cval_dev, double* rhs_dev) {
    SNS_TRY(scalar_check("sns_scalar_system", h, w_dev, kappa, sigma, theta, cmask_dev, cval_dev, rhs_dev));
    return scalar_system(h, w_dev, kappa, sigma, theta, src_dev, cmask_dev, cval_dev, rhs_dev);
}

int sns_scalar_solve(sns_handle h, const double* w_dev, const double kappa[4], double sigma, double theta, const double* src_dev,
                     const uint8_t* cmask_dev, const double* cval_dev, double* c_dev, int* its, int* reason, double* rnorm) {
    SNS_TRY(scalar_check("sns_scalar_solve", h, w_dev, kappa, sigma, theta, cmask_dev, cval_dev, c_dev));
    if (!its || !reason || !rnorm) { set_error("sns_scalar_solve: null output"); return SNS_E_ARG; }
    return scalar_solve(h, w_dev, kappa, sigma, theta, src_dev, cmask_dev, cval_dev, c_dev, its, reason, rnorm);
}

int sns_newton_solve(sns_handle h, double* w, int* its_out, int* reason_out, int* total_ksp, double* hist,
                     int hist_cap) {
    if (!h || !w || !its_out || !reason_out) return SNS_E_ARG;
    return newton_run(h, w, its_out, reason_out, total_ksp, hist, hist_cap);
}

int sns_set_time_term(sns_handle h, double sigma, double theta, const double* d_dev) {
    if (!h) return SNS_E_ARG;
    const policy::FormRequest req = (sigma == 0.0 && theta == 0.0 && !d_dev) ? policy::REQ_CLEAR_TIME_TERM : policy::REQ_SET_TIME_TERM;
    SNS_TRY(allows(h, "sns_set_time_term", policy::FAMILY_FORM, req, ROWS_ARG));
    if (!(sigma >= 0.0) || !std::isfinite(sigma) || !(theta >= 0.0) || !std::isfinite(theta)) {
        set_error("sns_set_time_term: sigma and theta must be finite and >= 0");
        return SNS_E_ARG;
    }
    if (sigma > 0.0 && !d_dev) { set_error("sns_set_time_term: sigma > 0 needs a history vector"); return SNS_E_ARG; }
    SNS_TRY(allows(h, "sns_set_time_term", policy::FAMILY_FORM, req, ROWS_STATE));
    return set_time_term(h, sigma, theta, d_dev);
}

int sns_set_viscosity_law(sns_handle h, int law, double lambda, double n, double nu_inf_ratio) {
    if (!h) return SNS_E_ARG;
    const policy::FormRequest req = law == SNS_LAW_CARREAU ? policy::REQ_SET_CARREAU : policy::REQ_SET_NEWTONIAN;
    SNS_TRY(allows(h, "sns_set_viscosity_law", policy::FAMILY_FORM, req, ROWS_ARG));
    if (law != SNS_LAW_NEWTONIAN && law != SNS_LAW_CARREAU) { set_error("sns_set_viscosity_law: unknown law"); return SNS_E_ARG; }
    if (law == SNS_LAW_CARREAU) {
        if (!(lambda >= 0.0) || !std::isfinite(lambda)) { set_error("sns_set_viscosity_law: lambda must be finite and >= 0"); return SNS_E_ARG; }
        if (!(n > 0.0) || !std::isfinite(n)) { set_error("sns_set_viscosity_law: n must be finite and > 0"); return SNS_E_ARG; }
        if (!(nu_inf_ratio >= 0.0) || !std::isfinite(nu_inf_ratio)) {
            set_error("sns_set_viscosity_law: nu_inf_ratio must be finite and >= 0");
            return SNS_E_ARG;
        }
    }
    SNS_TRY(allows(h, "sns_set_viscosity_law", policy::FAMILY_FORM, req, ROWS_STATE));
    return set_viscosity_law(h, law == SNS_LAW_CARREAU, lambda, n, nu_inf_ratio);
}

int sns_element_viscosity(sns_handle h, const double* w, double* nu_dev, double* gamma_dot_dev) {
    if (!h || !w) { set_error("sns_element_viscosity: null handle or state"); return SNS_E_ARG; }
    SNS_TRY(allows(h, "sns_element_viscosity", policy::FAMILY_FORM, policy::REQ_ELEMENT_VISCOSITY));
    return element_viscosity(h, w, nu_dev, gamma_dot_dev);
}

// the three field setters (`who`: the name in front of the message)
static int field_request(const char* who, const sns_ctx* h) {
    if (!h) { set_error(std::string(who) + ": null handle"); return SNS_E_ARG; }
    return allows(h, who, policy::FAMILY_FORM, policy::REQ_SET_FIELD);
}

int sns_set_body_force(sns_handle h, const double* f_dev) {
    SNS_TRY(field_request("sns_set_body_force", h));
    return set_body_force(h, f_dev);
}

int sns_set_element_viscosity(sns_handle h, const double* nu_dev) {
    SNS_TRY(field_request("sns_set_element_viscosity", h));
    return set_element_viscosity(h, nu_dev);
}

int sns_set_mixture(sns_handle h, const double* m_dev, double log_viscosity_ratio, const double buoyancy[3]) {
    SNS_TRY(field_request("sns_set_mixture", h));
    if (!std::isfinite(log_viscosity_ratio)) { set_error("sns_set_mixture: the log viscosity ratio must be finite"); return SNS_E_ARG; }
    if (buoyancy && !(std::isfinite(buoyancy[0]) && std::isfinite(buoyancy[1]) && std::isfinite(buoyancy[2]))) {
        set_error("sns_set_mixture: the buoyancy must be finite");
        return SNS_E_ARG;
    }
    return set_mixture(h, m_dev, log_viscosity_ratio, buoyancy);
}

// the three setters of the boundary terms (`who`: the name in front of the message)
static int boundary_setter(const char* who, const sns_ctx* h, policy::BoundaryRequest request) {
    if (!h) { set_error(std::string(who) + ": null handle"); return SNS_E_ARG; }
    return allows(h, who, policy::FAMILY_BOUNDARY, request);
}

int sns_set_boundary_facets(sns_handle h, int32_t n_facets, const int32_t* facets_host, const int64_t* facet_tets_host) {
    SNS_TRY(boundary_setter("sns_set_boundary_facets", h, policy::BREQ_SET_FACETS));
    if (n_facets < 0 || n_facets > (INT32_MAX - 3) / 9 || (n_facets > 0 && (!facets_host || !facet_tets_host))) {
        set_error("sns_set_boundary_facets: bad facet count or null list");
        return SNS_E_ARG;
    }
    return set_boundary_facets(h, n_facets, facets_host, facet_tets_host);
}

int sns_set_boundary_flow(sns_handle h, const double* t_dev, const double* beta_dev) {
    SNS_TRY(boundary_setter("sns_set_boundary_flow", h, policy::BREQ_SET_FLOW));
    return set_boundary_flow(h, t_dev, beta_dev);
}

int sns_set_boundary_scalar(sns_handle h, const double* alpha_dev, const double* g_dev) {
    SNS_TRY(boundary_setter("sns_set_boundary_scalar", h, policy::BREQ_SET_SCALAR));
    return set_boundary_scalar(h, alpha_dev, g_dev);
}

int sns_time_step(sns_handle h, double* w, double* wprev, double dt, int order, double theta_coeff, int* its, int* reason,
                  int* ksp_its) {
    if (!h || !w || !its || !reason) return SNS_E_ARG;
    if (order != 1 && order != 2) { set_error("sns_time_step: order must be 1 or 2"); return SNS_E_ARG; }
    if (!(dt > 0.0) || !std::isfinite(dt)) { set_error("sns_time_step: dt must be positive"); return SNS_E_ARG; }
    if (order == 2 && !wprev) { set_error("sns_time_step: BDF2 needs the state before w"); return SNS_E_ARG; }
    SNS_TRY(allows(h, "sns_time_step", policy::FAMILY_FORM, policy::REQ_TIME_STEP, ROWS_ARG));
    if (!(theta_coeff >= 0.0) || !std::isfinite(theta_coeff)) { set_error("sns_time_step: theta_coeff must be finite and >= 0"); return SNS_E_ARG; }
    SNS_TRY(allows(h, "sns_time_step", policy::FAMILY_FORM, policy::REQ_TIME_STEP, ROWS_STATE));
    return time_step(h, w, wprev, dt, order, theta_coeff, its, reason, ksp_its);
}


int sns_get_bsr(sns_handle h, int32_t* n_rows, int64_t* nnzb, const int32_t** rowptr, const int32_t** colind,
                const double** vals) {
    if (!h) return SNS_E_ARG;
    const Level& L = h->levels[0];
    if (n_rows) *n_rows = L.n;
    if (nnzb) *nnzb = L.nnzb;
    if (rowptr) *rowptr = L.rowptr;
    if (colind) *colind = L.colind;
    if (vals) *vals = L.vals;
    return SNS_OK;
}

int sns_get_element_scratch(sns_handle h, const double** Ke, const double** Fe) {
    if (!h) return SNS_E_ARG;
    if (Ke) *Ke = h->Ke;
    if (Fe) *Fe = h->Fe;
    return SNS_OK;
}

int sns_export(sns_handle h, int what, void* dst, int64_t nbytes) {
    if (!h || !dst) return SNS_E_ARG;
    const Level& L = h->levels[0];
    const void* src = nullptr;
    int64_t need = 0;
    switch (what) {
        case SNS_EXPORT_ROWPTR: src = L.rowptr; need = ((int64_t)L.n + 1) * 4; break;
        case SNS_EXPORT_COLIND: src = L.colind; need = L.nnzb * 4; break;
        case SNS_EXPORT_VALS: src = L.vals; need = L.nnzb * 16 * 8; break;
        case SNS_EXPORT_KE: src = h->Ke; need = h->E * 256 * 8; break;
        case SNS_EXPORT_FE: src = h->Fe; need = h->E * 16 * 8; break;
        case SNS_EXPORT_STRENGTH: {
            if (!h->has_matrix) { set_error("sns_export: strength before a matrix was assembled"); return SNS_E_STATE; }
            if (nbytes != L.nnzb * 4) { set_error("sns_export: size mismatch, need " + std::to_string(L.nnzb * 4)); return SNS_E_ARG; }
            DevBuf<double> scale;
            SNS_TRY(scale.alloc(4 * (size_t)L.n));
            SNS_TRY(compute_strength(h, (float*)dst, scale));
            return sync_stream(h);
        }
        case SNS_EXPORT_AGG0: {
            if (h->agg0.empty()) { set_error("sns_export: aggregate map before the hierarchy was built"); return SNS_E_STATE; }
            if (nbytes != (int64_t)L.n * 4) { set_error("sns_export: size mismatch, need " + std::to_string((int64_t)L.n * 4)); return SNS_E_ARG; }
            HIP_TRY(hipMemcpyAsync(dst, h->agg0.data(), (size_t)nbytes, hipMemcpyHostToDevice, h->stream));
            return sync_stream(h);
        }
        default: set_error("sns_export: unknown array"); return SNS_E_ARG;
    }
    if (!src) { set_error("sns_export: array not produced yet"); return SNS_E_STATE; }
    if (need != nbytes) { set_error("sns_export: size mismatch, need " + std::to_string(need)); return SNS_E_ARG; }
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)need, hipMemcpyDeviceToDevice, h->stream));
    return sync_stream(h);
}

int sns_get_counters(sns_handle h, int64_t out[8]) {
    if (!h || !out) return SNS_E_ARG;
    out[0] = h->last_ctr[0];
    out[1] = h->last_ctr[1];
    out[2] = h->last_ctr[2];
    out[3] = h->tm.ksp_its;
    out[4] = h->ctr_retries;
    out[5] = (int64_t)std::llround(h->damping_backoff * 1e6);
    out[6] = h->last_first_reason;
    out[7] = h->levels[0].ap_nnz;
    return SNS_OK;
}

int sns_comm_info(sns_handle h, int32_t out[4]) {
    if (!h || !out) return SNS_E_ARG;
    out[0] = out[1] = out[3] = 0;
    out[2] = 1;
    const Comm* c = h->comm.get();
    if (!c) return SNS_OK;
    out[0] = c->nccl ? 1 : (c->team ? 2 : (c->peer ? 3 : 0));
    out[1] = c->rank;
    out[2] = c->nranks;
    if (c->nccl) {
        int cnt = 0;
        NCCL_TRY(ncclCommCount(c->nccl, &cnt));
        out[3] = cnt;
    }
    return SNS_OK;
}

int sns_get_hierarchy(sns_handle h, int32_t* nlevels, int64_t rows[16], int64_t blocks[16], int32_t sweeps[16], double omega[16]) {
    if (!h || !nlevels) return SNS_E_ARG;
    const int nl = (int)std::min<size_t>(16, h->levels.size());
    *nlevels = nl;
    for (int l = 0; l < nl; ++l) {
        const Level& L = h->levels[l];
        if (rows) rows[l] = L.n_owned;
        if (blocks) blocks[l] = L.nnzb;
        if (sweeps) sweeps[l] = l + 1 < (int)h->levels.size() ? h->plan.level[(size_t)l].nu : 0;   // the coarsest level is a dense inverse
        if (omega) omega[l] = L.damping.omega;
    }
    return SNS_OK;
}

int sns_dense_inverse(int device, int32_t N, const double* A, double* Ainv) {
    if (N <= 0 || !A || !Ainv) return SNS_E_ARG;
    HIP_TRY(hipSetDevice(device));
    const int Np = (N + 63) / 64 * 64;
    DevBuf<double> W, work;
    DevBuf<int> sing;
    Stream side, mainst;
    SNS_TRY(W.alloc((size_t)Np * Np));
    SNS_TRY(work.alloc(dense_gj_work_doubles(Np)));
    SNS_TRY(sing.alloc(1));
    HIP_TRY(hipMemset(sing, 0, sizeof(int)));
    HIP_TRY(hipMemset(W, 0, (size_t)Np * Np * sizeof(double)));
    HIP_TRY(hipMemcpy2D(W, (size_t)Np * sizeof(double), A, (size_t)N * sizeof(double), (size_t)N * sizeof(double), N,
                        hipMemcpyDeviceToDevice));
    if (Np > N) hipLaunchKernelGGL(k_dense_pad_diag, dim3((Np - N + 255) / 256), dim3(256), 0, nullptr, N, Np, W);
    if (std::getenv("SNS_GJ_TWO_STREAMS")) (void)hipStreamCreateWithFlags(side.put(), hipStreamNonBlocking);
    HIP_TRY(hipDeviceSynchronize());                      // (the null stream does not order a non-blocking side stream)
    HIP_TRY(hipStreamCreateWithFlags(mainst.put(), hipStreamNonBlocking));
    dense_gj_inverse(mainst, side, Np, W, work, sing);
    HIP_TRY(hipStreamSynchronize(mainst));
    if (side) HIP_TRY(hipStreamSynchronize(side));
    HIP_TRY(hipMemcpy2D(Ainv, (size_t)N * sizeof(double), W, (size_t)Np * sizeof(double), (size_t)N * sizeof(double), N,
                        hipMemcpyDeviceToDevice));
    int hs = 0;
    HIP_TRY(hipMemcpy(&hs, sing, sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipGetLastError());
    if (hs) { set_error("sns_dense_inverse: zero or non-finite pivot"); return SNS_E_STATE; }
    return SNS_OK;
}

int sns_get_cycle(sns_handle h, int32_t* nlevels, int32_t kind[16], int32_t nu_pre[16], int32_t nu_post[16]) {
    if (!h || !nlevels || !kind || !nu_pre || !nu_post) return SNS_E_ARG;
    const int nl = (int)std::min<size_t>(16, h->levels.size());
    *nlevels = nl;
    for (int l = 0; l < nl; ++l) {
        const policy::LevelPlan& P = h->plan.level[(size_t)l];
        kind[l] = P.kind;
        nu_pre[l] = P.pre;
        nu_post[l] = P.post;
    }
    return SNS_OK;
}

int sns_get_timings(sns_handle h, sns_timings* t) {
    if (!h || !t) return SNS_E_ARG;
    *t = h->tm;
    t->amg_levels = (int)h->levels.size() - (h->rep_level > 0 ? 1 : 0);
    return SNS_OK;
}

int sns_reset_timings(sns_handle h) {
    if (!h) return SNS_E_ARG;
    h->tm = sns_timings{};
    h->ctr_retries = 0;
    for (int i = 0; i < 8; ++i) { h->kt_ms[i] = 0; h->kt_calls[i] = 0; }
    return SNS_OK;
}

int sns_time_kernels(sns_handle h, int on) {
    if (!h) return SNS_E_ARG;
    h->time_kernels = on != 0;
    return SNS_OK;
}

int sns_get_kernel_times(sns_handle h, double ms_total[8], int64_t calls[8]) {
    if (!h || !ms_total || !calls) return SNS_E_ARG;
    for (int i = 0; i < 8; ++i) { ms_total[i] = h->kt_ms[i]; calls[i] = h->kt_calls[i]; }
    return SNS_OK;
}


int sns_bench_spmv(sns_handle h, const double* x, double* y, int reps, double* ms_avg) {
    if (!h || !x || !y || reps <= 0 || !ms_avg) return SNS_E_ARG;
    if (!h->has_matrix) { set_error("bench_spmv before a matrix was assembled"); return SNS_E_STATE; }
    launch_spmv<SPMV_AX>(h, h->levels[0], h->n_owned, x, y, nullptr, 0.0, nullptr);   // warm
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    for (int i = 0; i < reps; ++i) launch_spmv<SPMV_AX>(h, h->levels[0], h->n_owned, x, y, nullptr, 0.0, nullptr);
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    *ms_avg = ms / reps;
    HIP_TRY(hipGetLastError());
    return SNS_OK;
}

int sns_bench_assemble(sns_handle h, int form, const double* w, double* F, int reps, double* ms_avg) {
    if (!h || reps <= 0 || !ms_avg) return SNS_E_ARG;
    SNS_TRY(assemble(h, form, w, F, true));
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    for (int i = 0; i < reps; ++i) SNS_TRY(assemble(h, form, w, F, true));
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    *ms_avg = ms / reps;
    return SNS_OK;
}

int sns_bench_collective(sns_handle h, int which, int count, int reps, double* ms_avg) {
    if (!h || reps <= 0 || !ms_avg || count < 0) return SNS_E_ARG;
    Comm* c = h->comm.get();
    if (!c || !c->active()) { set_error("sns_bench_collective: no communicator attached"); return SNS_E_STATE; }
    DevBuf<double> snd, rcv;
    if (which == 0) {
        if (c->plans.empty() || !h->levels[0].xg) { set_error("sns_bench_collective: no level-0 halo plan"); return SNS_E_STATE; }
    } else if (which == 1) {
        if (count < 1 || count > 32) { set_error("sns_bench_collective: all-reduce of 1..32 doubles"); return SNS_E_ARG; }
        HIP_TRY(hipMemsetAsync(h->d_scal + 64, 0, 32 * sizeof(double), h->stream));
    } else if (which == 2) {
        SNS_TRY(snd.alloc((size_t)std::max(1, count)));
        SNS_TRY(rcv.alloc((size_t)std::max(1, count) * c->nranks));
        HIP_TRY(hipMemset(snd, 0, (size_t)std::max(1, count) * sizeof(double)));
    } else {
        return SNS_E_ARG;
    }
    auto one = [&]() -> int {
        if (which == 0) return comm_exchange(c, c->plans[0], h->levels[0].xg, h->stream);
        if (which == 1) return comm_allreduce_sum(c, h->d_scal + 64, count, h->stream);
        return comm_allgather(c, snd, rcv, count, h->stream);
    };
    int rc = SNS_OK;
    for (int i = 0; i < 5 && rc == SNS_OK; ++i) rc = one();
    if (rc == SNS_OK) {
        (void)hipEventRecord(h->ev0, h->stream);
        for (int i = 0; i < reps && rc == SNS_OK; ++i) rc = one();
        (void)hipEventRecord(h->ev1, h->stream);
    }
    (void)hipStreamSynchronize(h->stream);
    if (rc == SNS_OK) rc = peer_check(c);
    if (rc == SNS_OK) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, h->ev0, h->ev1) != hipSuccess) rc = SNS_E_HIP;
        *ms_avg = ms / reps;
    }
    if (which == 0) (void)hipMemset(h->levels[0].xg, 0, 4 * (size_t)h->levels[0].n * sizeof(double));   // (the cycle relies on zero ghosts there)
    return rc;
}


}  // extern "C"

