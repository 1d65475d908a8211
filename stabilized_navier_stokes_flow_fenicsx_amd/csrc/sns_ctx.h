// Shared internals of the C-ABI layer (csrc/sns_api.hip and the setup / cycle / Krylov / solve / ... translation units beside it): the
// context behind an sns_handle, the error helpers, the launch helpers of the level passes and the functions the translation
// units call across each other.  The context owns its device memory and HIP objects by type (csrc/sns_devbuf.h): there is no
// free list, ~sns_ctx releases everything.  Not installed; the public surface is include/sns.h.
#pragma once
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "sns_comm.h"
#include "sns_internal.h"
#include "sns_kernels.h"
#include "sns_policy.h"

namespace sns {

#define HIP_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) {                                                                           \
            set_error(std::string(#expr) + ": " + hipGetErrorString(_e) + " @" + __FILE__ + ":" +         \
                      std::to_string(__LINE__));                                                          \
            return SNS_E_HIP;                                                                             \
        }                                                                                                 \
    } while (0)

#define NCCL_TRY(expr)                                                                                    \
    do {                                                                                                  \
        ncclResult_t _e = (expr);                                                                         \
        if (_e != ncclSuccess) {                                                                          \
            set_error(std::string(#expr) + ": " + ncclGetErrorString(_e));                                \
            return SNS_E_COMM;                                                                            \
        }                                                                                                 \
    } while (0)

#define SNS_TRY(expr)                                                                                     \
    do {                                                                                                  \
        int _r = (expr);                                                                                  \
        if (_r != SNS_OK) return _r;                                                                      \
    } while (0)

}  // namespace sns

using namespace sns;

// internal id of the scalar-transport operator in sns_ctx::matrix_form and the operator keys (beside SNS_FORM_STOKES, SNS_FORM_NS
// and the two 2-D ids of csrc/sns_kernels.h); no public entry point takes it
#define SNS_FORM_SCALAR 4

// The state of the 3-D NS form beside the options: what the setters of csrc/sns_form.hip write and form_pass
// (csrc/sns_assemble.hip) hands to the kernels.  Which switches go together is the table policy::RULES.
struct FormState {
    FormVariant fv;                              // sns_set_form_variant (diagnostic; default = the reference's form)
    // sns_set_time_term: the transient form.  tt.d points at tt_d, the handle's copy of the history (4*n doubles, allocated at
    // the first set), or at tt_eff below; tt_on selects the TT instantiations of the NS assembly kernels
    TimeTerm tt;
    DevBuf<double> tt_d;
    DevBuf<double> tt_w0;                        // sns_time_step: the state on entry
    bool tt_on = false;
    // sns_set_viscosity_law: the generalised-Newtonian form; vl_on selects the VL instantiations (never with tt_on)
    ViscosityLaw vl;
    bool vl_on = false;
    // sns_set_body_force / sns_set_element_viscosity: the caller's f, the effective history tt_eff = d - f that tt.d points at
    // while a force is on (d = tt_d under a time term, 0 without; rewritten whenever d or f changes; all zero for a viscosity
    // field alone), and the per-cell nu_t behind tt.nu_t.  bf_on runs the TT instantiations, ev_on the EV ones (never with vl_on)
    DevBuf<double> bf_f, tt_eff, ev_nu;
    bool bf_on = false, ev_on = false;
    uint64_t ev_generation = 0;                  // moves whenever ev_nu is written or a field is cleared: another operator
    // the compile-time variant of the 3-D NS assembly kernels: 0 the reference's steady form, 1 TT (a time term or a body force,
    // which rides in the effective history), 2 VL (a law; never with the others), 3 EV (a field; contains the time term)
    int ns_variant() const { return ev_on ? 3 : (vl_on ? 2 : ((tt_on || bf_on) ? 1 : 0)); }
    uint64_t boundary_generation = 0;            // moves whenever a boundary coefficient (beta, alpha) is written or cleared
    policy::FormKey key() const {                // (of an operator assembled now)
        return {tt.sigma, tt.theta, vl_on, vl.lambda, vl.n, vl.r, ev_generation, boundary_generation};
    }
};

// The boundary terms (csrc/sns_boundary.hip): the facet lists of sns_set_boundary_facets and the data of sns_set_boundary_flow /
// sns_set_boundary_scalar, all in buffers the handle owns.  Nothing is allocated before the first set; nf == 0: no facets.
struct BoundaryState {
    int32_t nf = 0, nb = 0;                      // facets, boundary rows
    DevBuf<int32_t> facets;                      // [3 nf] rewound: (x1 - x0) x (x2 - x0) points out of the owning tet
    DevBuf<int32_t> rows, row_ptr, row_fv;       // [nb], [nb + 1], [3 nf]: per row its entries facet * 4 + vertex, facets ascending
    DevBuf<uint8_t> swapped;                     // [nf] the rewinding swapped vertices 1 and 2 (the callers' P1 data is brought into that order)
    DevBuf<int32_t> slot;                        // [9 nf] BSR slot of block (node a, node b) of a facet at 9 f + 3 a + b
    DevBuf<double> t, beta, alpha, g;            // [9 nf] traction, [nf], [4 nf], [12 nf], P1 data in the rewound vertex order; *_on: the term is set
    bool t_on = false, beta_on = false, alpha_on = false, g_on = false;
    DevBuf<double> rm;                           // [4 nb] sns_residual_moments: phi_i times the raw boundary residual of row i
    bool flow_on() const { return nf > 0 && (t_on || beta_on); }
    bool scalar_on() const { return nf > 0 && (alpha_on || g_on); }
};

struct sns_ctx {
    // Release order: ~sns_ctx waits for the device and destroys the graph exec and the streams; then the members go in reverse
    // order of declaration -- events and every buffer first, the communicator (declared first) last: its plans' window areas go
    // back through plan_free, the plans' arrays are freed, the RCCL communicator is destroyed (~Comm, csrc/sns_comm.hip).
    std::unique_ptr<Comm> comm;
    ~sns_ctx() {
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
        coarse_graph.reset();
        cap_stream.reset();
        gj_stream.reset();
        side_stream.reset();
        setup_stream.reset();
    }
    sns_options opt;
    int device = 0;
    hipStream_t stream = nullptr;                // (borrowed: the caller's, sns_set_stream)
    // mesh (dim 3: tets; dim 2: triangles in a stride-4 connectivity, z component a Dirichlet dof)
    int dim = 3;
    int32_t n = 0, n_owned = 0;
    int64_t n_global_fine = 0;                   // fine-level rows over all ranks (set when the hierarchy is built)
    int64_t n_global_l1 = 0;                     // level-1 rows over all ranks (the sweep schedule must be the same on every rank)
    int64_t E = 0;
    DevBuf<int32_t> tets;
    DevBuf<double> pts;
    DevBuf<uint8_t> bc_mask;
    DevBuf<double> bc_val;
    // assembly maps
    DevBuf<int64_t> nt_ptr, c_ptr;
    DevBuf<int32_t> nt_idx, c_idx;
    DevBuf<int32_t> od_order;          // off-diagonal slots, locally sorted by contribution count (scratch-free assembly)
    DevBuf<double> gext;               // Dirichlet data extended by zero (the state the Stokes lifting term is taken at)
    int64_t n_od = 0;
    DevBuf<double> Ke, Fe;
    // residual moments (sns_residual_moments): per-256-cell support counts / offsets, the compacted connectivity and its
    // element residuals (capacity rm_cap cells, grown on demand), and an all-zero Dirichlet mask for the staged element kernel
    DevBuf<int64_t> rm_off;
    DevBuf<int32_t> rm_cells;
    DevBuf<double> rm_Fe;
    int64_t rm_cap = 0;
    DevBuf<uint8_t> rm_nomask;
    // operator hierarchy; levels[0] is the assembled fine operator.  A deque: references to a level stay valid
    // while coarser levels are appended (a vector reallocation under a live Level& once handed a kernel dangling
    // pointers)
    std::deque<Level> levels;
    DevBuf<int> d_piv;
    DevBuf<int> d_sing;
    FormState form;                              // the switches of the 3-D NS form and their buffers (csrc/sns_form.hip)
    BoundaryState bnd;                           // the facet terms and their lists (csrc/sns_boundary.hip)
    DevBuf<double> rm_nu;                        // residual moments: nu_t of the compacted cells (capacity rm_cap)
    bool has_matrix = false, pc_ready = false;
    int pc_setups = 0;
    // hipGraph of the launch-bound coarse part of the V-cycle (levels >= graph_level; serial runs only)
    Stream cap_stream;
    Stream gj_stream;                            // second stream of the dense coarsest level's elimination (bulk updates beside the pivot chain)
    GraphExec coarse_graph;
    std::vector<double> graph_sig;                // (graph level, omega per level) the graph was captured with ...
    std::vector<policy::LevelPlan> graph_rows;    // ... and the plan rows it covers
    bool graph_disabled = false;
    int matrix_form = -1;
    bool transposed = false;                     // vals holds A^T (sns_transpose_operator); every assembly clears it
    DevBuf<int32_t> tr_partner;                  // [nnzb] slot (i, j) -> slot (j, i), built at the first transpose (csrc/sns_transpose.hip)
    // which operator vals holds, and which one the levels' spectral estimates were last taken on (policy::OperatorKey): a set-up
    // takes them again iff the two differ.  matrix_changed and transpose_operator write the first, pc_setup the second
    policy::OperatorKey matrix_key, est_key;
    // sns_scalar_system (csrc/sns_scalar.hip): matrix_form = SNS_FORM_SCALAR while the scalar operator is the handle's matrix
    DevBuf<uint8_t> sc_mask;                     // the scalars' Dirichlet mask of the last scalar assembly (4*n, allocated at the first)
    // reductions
    DevBuf<double> partial;                      // [max(65536*8, n/32)]
    DevBuf<double> partial2;                     // second stage of long reductions
    DevBuf<double> d_scal;                       // [256]
    PinnedDoubles h_scal;                        // pinned [256]
    // Krylov workspace
    std::vector<DevBuf<double>> kv;                   // allocated vectors (4*n each)
    DevBuf<double> gm_V;                         // (m+1) * ld
    DevBuf<double> gm_Z;                         // m * ld
    int gm_m = 0;
    DevBuf<double> d_h;                          // device Hessenberg column scratch [3*(m+2)]
    // Newton workspace
    DevBuf<double> nw_F, nw_y, nw_w, nw_t;
    sns_timings tm{};
    Event ev0, ev1, ev_it;
    // debug counters of the last Krylov solve (sns_get_counters): host syncs, all-reduces, halo exchanges
    int64_t ctr_host_syncs = 0, ctr_allreduce = 0, ctr_exchange = 0;
    int64_t last_ctr[3] = {0, 0, 0};                 // snapshot at the end of the last Krylov solve
    int bnd_dot_blocks = 0;
    int dot_partials = 0;                            // partial sums the last fused SpMV+dot pass left in h->partial
    // multi-GPU, level 0: owned rows with at least one ghost column (the only rows that must wait for the halo)
    DevBuf<int32_t> bnd_rows;
    DevBuf<uint8_t> bnd_flag;
    int32_t n_bnd = 0;
    Stream side_stream;
    Event ev_x, ev_side;
    // the set-up on two streams (policy::StepPlan::setup_two_streams): the stream of the coarse chain, created once at the
    // greatest priority; the events main -> chain (the operator is assembled), chain -> main per level (its operator is
    // written) and at the end
    Stream setup_stream;
    Event ev_setup_fork, ev_setup_join;
    std::vector<Event> ev_setup_level;
    bool no_overlap = false;
    bool team_overlap = false;                       // SNS_TEAM_OVERLAP: the team transport takes the two-stream path too (tests)
    DevBuf<double> arn_V;                             // Arnoldi basis of the damping estimate, 9 vectors of the largest level >= ... asked for
    // what one kernel of a solve hands to a later one: the fine level's first sweep done by the Krylov kernel, the puts carried by
    // the kernels that produced a vector (PutDst), the caller's promise of an operator application (policy::Handoff: its
    // transitions are the only writers; window_put below is where a carried put is taken)
    policy::Handoff handoff;
    bool r3_estimates = false;                       // SNS_R3_SPECTRAL_ESTIMATE (tests of the retry path): round 3's policy -- spectral
                                                     // estimates every 4th setup whatever the operator (first Jacobians on the Stokes estimate)
    bool plain_step = false;                         // SNS_PLAIN_STEP (tests, profiles): policy::plan_step answers with the schedule of
                                                     // the solve as it was -- every operator pass, the whole speculative half iteration
    // the preconditioner application pc_apply_begin has opened and pc_apply_finish / pc_apply_abandon has not closed yet: its
    // result vector and, where the fine level's cycle was cut behind the restriction, the cycle's vector and ping-pong buffers
    struct PendingCycle {
        bool open = false, cut = false;
        const double* b = nullptr;
        double *z = nullptr, *x = nullptr, *cur = nullptr, *oth = nullptr;
    } pc_pending;
    double damping_backoff = 1.0;                    // < 1 after a failed AMG-preconditioned solve: all level dampings scaled
                                                     // (damping_back_off, csrc/sns_damping.hip; back to 1 by damping_reset)
    int64_t ctr_retries = 0;                         // damping retries since sns_reset_timings
    int last_first_reason = 0;                       // reason of the FIRST attempt of the last solve (0 = no retry happened)
    // what the V-cycle runs (csrc/sns_policy.h): the hierarchy's structure, agreed over the ranks when it is built, and the plan the
    // options make of it (rebuilt by sns_set_options).  Every decision of the cycle reads plan.
    policy::Facts facts;
    policy::CyclePlan plan;
    // distributed coarsest level: global dense inverse, replicated on every rank
    int cg_maxn = 0;                              // padded owned coarsest nodes per rank
    int cg_N = 0;                                 // 4 * nranks * cg_maxn (0 = not used)
    std::vector<int> cg_counts;                   // owned coarsest nodes of every rank
    // multi-GPU: replicated tail of the hierarchy.  levels[rep_level - 1], the source, is the last partitioned level: it is not
    // cycled, and levels[rep_level] holds the same operator over ALL ranks' rows on every rank (its values all-gathered from
    // the source at every numeric setup); that copy and everything below it is cycled redundantly on every rank without any
    // exchange.  0 = none.
    int rep_level = 0;
    int32_t rep_maxn = 0, rep_NG = 0, rep_off = 0;
    int64_t rep_maxnz = 0;
    DevBuf<int32_t> rep_valmap;                   // [nranks*maxnz] gathered slot -> slot of the replicated level (-1: padding)
    DevBuf<int32_t> rep_rowmap;                   // [NG] row of the replicated level -> gathered row (rank*maxn + i)
    DevBuf<double> rep_vsend, rep_vrecv, rep_bsend, rep_brecv;
    DevBuf<int64_t> rep_doff, rep_dcnt;                 // [nranks] doubles: where rank r's right-hand side goes in the replicated level's b, and how much
    DevBuf<int32_t> cg_colmap;                    // local coarsest node -> global (padded) node id
    DevBuf<double> cg_rows, cg_full, cg_send, cg_recv;
    std::unique_ptr<HostPattern> pattern;      // kept until the (lazy) hierarchy build
    std::vector<double> host_pts;              // ... with the node coordinates (3 per node): the aggregation's strength filter on anisotropic meshes
    std::vector<int32_t> agg0;                 // the level-0 aggregate map as built (owned nodes; -1 elsewhere): SNS_EXPORT_AGG0
    bool fine_rematched_local = false;         // amg_aggregation = 3 re-matched level-0 nodes of this rank ...
    bool fine_rematched = false;               // ... of some rank (agreed over the ranks: the fine-level aggregate blocks)
    // optional per-launch timing of the fine-level SpMV family
    bool time_kernels = false;
    std::vector<std::array<Event, 2>> ev_pool;
    std::vector<int> ev_mode;
    size_t ev_used = 0;
    double kt_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};            // modes 0..3 = SpmvMode, 4 = fused post-sweep on M = A P
    int64_t kt_calls[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};


// ---- across the translation units ------------------------------------------------------------------------------------------------
namespace sns {
// csrc/sns_setup.hip: symbolic hierarchy, numeric setup of the preconditioner, workspace vectors
int alloc_level_vectors(Level& L);
int upload_pattern(Level& L, const HostPattern& P, hipStream_t s);
int global_sum(sns_ctx* h, double* v, int count);
int host_allgather(sns_ctx* h, const std::vector<double>& mine, std::vector<double>& all);
int check_plan_symmetry(sns_ctx* h, const Plan& p, int level);
int connect_plan(sns_ctx* h, Plan& p);
int plan_hierarchy(sns_ctx* h);
const char* plan_buffer_missing(const sns_ctx* h);
int build_hierarchy(sns_ctx* h, const HostPattern& fine);
int pc_setup(sns_ctx* h);
// csrc/sns_damping.hip: the three transitions of the damping state (Level::damping, damping_backoff) -- decide: level l of nl at
// a set-up, with the spectral estimates that are due; back off: after a retryable failure of a solve; reset: an options call
enum class DampingReset { AFTER_RETRY /* only where a retry scaled the dampings: the factor too, and pc_ready */, ESTIMATES };
int damping_decide(sns_ctx* h, int l, int nl, bool new_operator);
bool damping_estimates_due(const sns_ctx* h, int l, int nl, bool new_operator);   // (decide would launch estimators on level l)
void damping_back_off(sns_ctx* h);
void damping_reset(sns_ctx* h, DampingReset what);
// The workspace vectors h->kv (4*n doubles each, allocated in slot order up to the slot asked for).  VEC_SCRATCH serves the lifting's
// BC defect, the snapped 2-D Stokes state, sns_time_step's BDF history, the moments' zero state and the zero vector of the three
// spectral estimates.  What makes the sharing sound: every user writes the whole range it reads before reading it, and none
// relies on the contents across a call into assemble / the estimates / the moments.
enum VecSlot { VEC_KRYLOV = 0 /* .. 9, the Krylov methods */, VEC_ARNOLDI_IN = 12, VEC_SCRATCH = 13, VEC_SAVED_GUESS = 14 /* the retry */ };
int get_vec(sns_ctx* h, size_t k, double** out);
// csrc/sns_assemble.hip: the assembly driver over policy::plan_assembly, the residual moments on the same element pass.
// matrix_changed: the fine operator was rewritten by an assembly of `form` (scalar_par: a scalar assembly's kappa[4], sigma,
// theta) -- the one place that says so: has_matrix, transposed, matrix_form, and matrix_key stamped from h->form and h->opt
void matrix_changed(sns_ctx* h, int form, const double* scalar_par = nullptr);
int assemble(sns_ctx* h, int form, const double* w, double* F, bool want_matrix);
int timed_assemble(sns_ctx* h, int form, const double* w, double* F, bool want_matrix);
int residual_moments(sns_ctx* h, int form, const double* w, const double* phi, double out[4]);
// ... and the NS form's raw Jacobian applied matrix-free: y = J0(w) x, or J0(w)^T x (writes y alone; synchronises)
int raw_jacobian_apply(sns_ctx* h, const double* w, const double* x, bool transposed, double* y);
// csrc/sns_cycle.hip: the V-cycle, the preconditioner and operator applications
int vcycle(sns_ctx* h, int l, const double* b, double* x);
int coarse_cycle(sns_ctx* h, int l, const double* b, double* x);
int pc_apply(sns_ctx* h, const double* r, double* z);
// ... in two stages (policy::StepPlan::staged_speculation): begin queues the application up to the point where it can be cut --
// the fine level's cycle through its restriction where `split`, else all of it --, finish the rest; abandon drops an opened
// application whose result nobody will read, through the clean-up of a failed pc_apply
int pc_apply_begin(sns_ctx* h, const double* r, double* z, bool split);
int pc_apply_finish(sns_ctx* h);
void pc_apply_abandon(sns_ctx* h);
policy::StepPlan step_plan(const sns_ctx* h, bool zero_guess_vouched, bool estimates_due = true);
int op_apply(sns_ctx* h, double* x, double* y);
int op_apply_dot(sns_ctx* h, double* x, double* y, const double* dotw);
int op_residual(sns_ctx* h, double* x, const double* b, double* r);
// csrc/sns_krylov.hip: BiCGStab / TFQMR / FGMRES and the solve driver with the damping retry
// zero_guess: the caller zeroed x itself on the handle's stream; ax / ax_done: a buffer for A x of the returned iterate, and
// whether the method left it there (else the caller applies the operator itself)
int krylov(sns_ctx* h, const double* b, double* x, int* its, int* reason, double* rnorm, bool zero_guess = false, double* ax = nullptr,
           bool* ax_done = nullptr);
// ... and the frame of a solve: what opens one (`who`: the caller in "<who> before a matrix was assembled") and what closes it
int solve_open(sns_ctx* h, const char* who);
int solve_close(sns_ctx* h, int its);
// csrc/sns_solve.hip: the solve drivers behind the entry points (which have checked the arguments) and their shared pieces.
// ensure_hierarchy builds the lazy hierarchy (assembles_next: the caller assembles next, so an operator-based aggregation may
// wait); solve_and_snap is krylov plus the exact Dirichlet data `val` under `mask` after a converged solve; give_back returns the
// operator flipped and the time term set for one call.  newton_run works on whatever NS form the handle carries
int ensure_hierarchy(sns_ctx* h, bool assembles_next = false);
int ensure_newton_workspace(sns_ctx* h);
int solve_and_snap(sns_ctx* h, const double* b, double* x, const uint8_t* mask, const double* val, int* its, int* reason, double* rnorm,
                   bool zero_guess = false);
int give_back(sns_ctx* h, int rc, bool flipped, bool time_term);
int newton_run(sns_ctx* h, double* w, int* its, int* reason, int* total_ksp, double* hist, int hist_cap);
int stokes_solve(sns_ctx* h, double* U, int* ksp_its, int* reason, double* rnorm);
int time_step(sns_ctx* h, double* w, double* wprev, double dt, int order, double theta_coeff, int* its, int* reason, int* ksp_its);
int scalar_solve(sns_ctx* h, const double* w, const double kappa[4], double sigma, double theta, const double* src, const uint8_t* cmask,
                 const double* cval, double* c, int* its, int* reason, double* rnorm);
int adjoint_solve(sns_ctx* h, const double* g, double* lam, int* its, int* reason, double* rnorm);
int stability_arnoldi(sns_ctx* h, const double* w, double shift, bool left, int k, int m, double breakdown_rel, double* V, double* H,
                      int* m_done, int* total_ksp_its, int* reason, const double* c = nullptr);
// csrc/sns_strength.hip: the strength of the fine-level couplings (amg_aggregation = 1, SNS_EXPORT_STRENGTH)
int compute_strength(sns_ctx* h, float* out, double* scale);
// csrc/sns_transpose.hip: flip the fine operator between A and A^T in place
int transpose_operator(sns_ctx* h);
// csrc/sns_shape.hip: lam . dR_raw/dX of the NS form by one element pass (uses the element scratch Fe)
int residual_shape_gradient(sns_ctx* h, const double* w, const double* lam, double* gX);
// csrc/sns_recover.hip: the nodal gradient of the P1 state recovered by volume-weighted averaging (G and / or the derived
// fields D), and the Zienkiewicz-Zhu indicator per cell (G null: recovered into a temporary)
int recover_gradient(sns_ctx* h, const double* w, double* G, double* D);
int error_indicator(sns_ctx* h, const double* w, const double* G, double* eta2, double* gnorm2);
// csrc/sns_stability.hip: the mass passes y = B(w) x and y = B(w)^T z, and the shift-invert Arnoldi process (left: on
// (J + shift B)^-T B^T, with the transposed operator in the handle) from column k0 (0: a fresh process; >= 1: the caller's
// decomposition continued), and the in-place compression of its basis V[:, 0:n_out] <- V[:, 0:n_in] Q (Q on the host)
int mass_apply(sns_ctx* h, const double* w, const double* x, double* y);
int mass_apply_transpose(sns_ctx* h, const double* w, const double* z, double* y);
// ... queued on the handle's stream: y = B x (left: B^T x), and for planar complex x, y the pair pass y += c B x
void launch_mass(sns_ctx* h, bool left, const double* w, const double* x, double* y);
void launch_mass_pair(sns_ctx* h, bool left, const double* w, double c_re, double c_im, const double* x, double* y);
// c: null, or the complex coefficient (re, im) of the shifted step -- S = Re[(A + c B)^-1 B] with A the handle's matrix
int arnoldi_run(sns_ctx* h, const double* w, bool left, int k0, int m, double breakdown_rel, double* V, double* H, int* m_done,
                int* total_its, int* reason, const double* c = nullptr);
int basis_rotate(sns_ctx* h, int n_in, int n_out, const double* Q, double* V);
// csrc/sns_shifted.hip: the complex operator y = A x + c B(w) x (left: B^T; A is the handle's matrix as it stands) on planar
// complex vectors -- 4 n real parts, then 4 n imaginary parts -- and its solve by right-preconditioned complex FGMRES with the
// handle's options.  CfgmresWork: the solver's own buffers (basis, preconditioned basis, coefficients), kept by whoever solves
// more than once
struct CfgmresWork {
    DevBuf<double> V, Z, co;
    int m = 0;
    int reserve(sns_ctx* h);
};
int shifted_apply(sns_ctx* h, const double* w, double c_re, double c_im, bool left, const double* x, double* y);
int cfgmres(sns_ctx* h, const double* w, double c_re, double c_im, bool left, const double* b, double* x, int* its, int* reason,
            double* rnorm, CfgmresWork& ws);
int shifted_solve(sns_ctx* h, const double* w, double c_re, double c_im, bool left, const double* b, double* x, int* its, int* reason,
                  double* rnorm);
// csrc/sns_resolvent.hip: the energy pass y = D_chi M D_chi x (chi null: all ones; parts = 2: planar complex x, y), the lumped
// nodal volumes in the layout of a state vector, and the Hermitian Krylov process on
// T = S B^T (J + i omega B)^-H Q (J + i omega B)^-1 B S, which assembles J, flips it twice per step and leaves it untransposed
void launch_energy(sns_ctx* h, const double* chi, int parts, const double* x, double* y);
int energy_apply(sns_ctx* h, const double* chi, int parts, const double* x, double* y);
int lumped_volumes(sns_ctx* h, double* m);
int resolvent_lanczos(sns_ctx* h, const double* w, double omega, int m, double breakdown_rel, const double* chi_f, const double* chi_q,
                      double* V, double* H, int* m_done, int* total_its, int* reason);
// csrc/sns_hessian.hip: g = grad_w [ z~^T (c_jac J(w) + c_mass B(w)) x~ ] by one element pass (uses the element scratch Fe)
int jacobian_state_gradient(sns_ctx* h, const double* w, const double* x, const double* z, double c_jac, double c_mass, double* g);
int jacobian_shape_gradient(sns_ctx* h, const double* w, const double* x, const double* z, double c_jac, double c_mass, double* gX);
// csrc/sns_scalar.hip: the four-species transport operator into the fine level's vals and its right-hand side (synchronises)
int scalar_system(sns_ctx* h, const double* w, const double kappa[4], double sigma, double theta, const double* src,
                  const uint8_t* cmask, const double* cval, double* rhs);
// csrc/sns_form.hip: the setters of the form state h->form and the query behind sns_element_viscosity (checked by the entry points).
// refresh_history points tt.d at what the kernels read after d or f changed; support_nu gathers nu_t of the cells k_support_scatter keeps
int set_form_variant(sns_ctx* h, double c_inverse, double lsic_scale, double pspg_sign, int one_point_quadrature);
int set_time_term(sns_ctx* h, double sigma, double theta, const double* d);
int set_viscosity_law(sns_ctx* h, bool carreau, double lambda, double n, double nu_inf_ratio);
int element_viscosity(sns_ctx* h, const double* w, double* nu, double* gamma_dot);
int refresh_history(sns_ctx* h);
int set_body_force(sns_ctx* h, const double* f);
int set_element_viscosity(sns_ctx* h, const double* nu);
int set_mixture(sns_ctx* h, const double* m, double log_ratio, const double buoyancy[3]);
int support_nu(sns_ctx* h, const double* phi, int64_t nc);
// csrc/sns_boundary.hip: the setters of h->bnd (checked by the entry points) and the owner-computes pass over the boundary rows.
// boundary_flow adds the traction and backflow terms to F and / or vals (either may be null) after the volume passes;
// boundary_scalar the Robin terms to vals and rhs; boundary_moments sum_i phi_i (raw boundary residual of row i) to out[0..3]
int set_boundary_facets(sns_ctx* h, int32_t n_facets, const int32_t* facets_host, const int64_t* facet_tets_host);
int set_boundary_flow(sns_ctx* h, const double* t, const double* beta);
int set_boundary_scalar(sns_ctx* h, const double* alpha, const double* g);
int boundary_flow(sns_ctx* h, const double* w, double* F, double* vals);
int boundary_scalar(sns_ctx* h, const uint8_t* cmask, const double* cval, double* vals, double* rhs);
int boundary_moments(sns_ctx* h, const double* w, const double* phi, double out[4]);
// ... and the fine level's free mask (with the per-aggregate counts derived from it) set to the complement of a Dirichlet mask
int fine_free_mask(sns_ctx* h, const uint8_t* dirichlet_mask);
// csrc/sns_aggregate.hip: aggregate_strength's map of the owned nodes, built on the device (amg_aggregation = 2)
int aggregate_strength_device(sns_ctx* h, int max_agg, std::vector<int32_t>& agg, int32_t& nc);
// ... and the hybrid (amg_aggregation = 3): the geometric map g (ng aggregates) re-matched where it cuts a dominant coupling
int aggregate_hybrid_device(sns_ctx* h, int max_agg, const std::vector<int32_t>& g, int32_t ng, std::vector<int32_t>& agg, int32_t& nc,
                            bool& rematched);
int norm2(sns_ctx* h, const double* x, double* out);
int dot(sns_ctx* h, const double* x, const double* y, double* out);
}  // namespace sns

// ---- small helpers and launch helpers (internal linkage: every translation unit gets its own) -------------------------------
namespace {

inline int vec_grid(int64_t n) { return (int)std::min<int64_t>((n + 255) / 256, 2048); }

inline int64_t ld_of(const sns_ctx* h) { return 4 * (int64_t)h->n; }

inline int64_t nred_of(const sns_ctx* h) { return 4 * (int64_t)h->n_owned; }


inline int sync_stream(sns_ctx* h) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SNS_OK;
}

// the operator behind the preconditioner changed (a setter altered a value, the values were transposed): the next solve sets up
inline void pc_stale(sns_ctx* h) { h->pc_ready = false; }

// the facts every request rule of policy::RULES is asked with: the one place that reads them off a handle
inline policy::HandleFacts facts_of(const sns_ctx* h) {
    const FormState& S = h->form;
    const BoundaryState& B = h->bnd;
    return {h->dim, h->comm != nullptr, S.tt_on, S.vl_on, S.bf_on, S.ev_on, B.nf > 0, B.nf > 0 && B.t_on, B.nf > 0 && B.beta_on};
}


inline void time_begin(sns_ctx* h, int mode, hipStream_t st = nullptr) {
    if (!h->time_kernels) return;
    if (h->ev_used == h->ev_pool.size()) {
        h->ev_pool.emplace_back();
        (void)hipEventCreate(h->ev_pool.back()[0].put());
        (void)hipEventCreate(h->ev_pool.back()[1].put());
        h->ev_mode.push_back(0);
    }
    h->ev_mode[h->ev_used] = mode;
    (void)hipEventRecord(h->ev_pool[h->ev_used][0], st ? st : h->stream);
}

inline void time_end(sns_ctx* h, hipStream_t st = nullptr) {
    if (!h->time_kernels) return;
    (void)hipEventRecord(h->ev_pool[h->ev_used][1], st ? st : h->stream);
    ++h->ev_used;
}

// resolve recorded event pairs (stream must be idle)
inline void time_collect(sns_ctx* h) {
    for (size_t i = 0; i < h->ev_used; ++i) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, h->ev_pool[i][0], h->ev_pool[i][1]) == hipSuccess) {
            h->kt_ms[h->ev_mode[i]] += ms;
            h->kt_calls[h->ev_mode[i]]++;
        }
    }
    h->ev_used = 0;
}


// finish a two-stage reduction locally: partial[nblocks][nred] -> dst_dev[0..nred)
inline void reduce_local(sns_ctx* h, int nblocks, int nred, double* dst_dev) {
    if (nblocks > 8192 && nred <= 8) {
        // the fused SpMV+dot leaves one partial per 32 rows (54 k at 10 M tets): a single workgroup needs ~40 us
        // for that, 2048-wide chunks on many CUs first ~5 us
        const int nchunks = (nblocks + 2047) / 2048;
        if (nchunks <= 4096) {
            hipLaunchKernelGGL(k_reduce_chunks, dim3(nchunks, nred), dim3(256), 0, h->stream, nblocks, nred, h->partial,
                               h->partial2);
            hipLaunchKernelGGL(k_reduce_final, dim3(nred), dim3(256), 0, h->stream, nchunks, nred, h->partial2, dst_dev);
            return;
        }
    }
    hipLaunchKernelGGL(k_reduce_final, dim3(nred), dim3(256), 0, h->stream, nblocks, nred, h->partial, dst_dev);
}

// sum `count` device doubles over the ranks (no-op without a communicator)
inline int allreduce(sns_ctx* h, double* buf_dev, int count) {
    if (h->comm && h->comm->active()) ++h->ctr_allreduce;
    return comm_allreduce_sum(h->comm.get(), buf_dev, count, h->stream);
}

inline int reduce_to(sns_ctx* h, int nblocks, int nred, double* dst_dev);

// BiCGStab's two reductions with the scalar update they feed (WHICH 1: alpha, 2: omega & co, k_reduce_final_bicg): without a
// communicator the last reduction stage and the update are one launch; with one, the all-reduce sits between them
template <int WHICH>
int reduce_bicg(sns_ctx* h, int nblocks, double* red, double* sc) {
    constexpr int NRED = WHICH == 1 ? 1 : 5;
    Peer* pe = (h->comm && h->comm->active()) ? h->comm->peer : nullptr;
    if (h->comm && h->comm->active() && !pe) {
        SNS_TRY(reduce_to(h, nblocks, NRED, red));
        if (WHICH == 1) hipLaunchKernelGGL(k_bicg_alpha, dim3(1), dim3(64), 0, h->stream, sc, red);
        else hipLaunchKernelGGL(k_bicg_omega, dim3(1), dim3(64), 0, h->stream, sc, red);
        return SNS_OK;
    }
    const double* src = h->partial;
    int nb = nblocks;
    if (nblocks > 8192) {                        // (as reduce_local: 2048-wide chunks on many CUs first; one workgroup over 27 k
                                                 // partials -- the slab share -- was measured at 29 us against 4.6 + 4.8 for the two stages)
        const int nchunks = (nblocks + 2047) / 2048;
        if (nchunks <= 4096) {
            hipLaunchKernelGGL(k_reduce_chunks, dim3(nchunks, NRED), dim3(256), 0, h->stream, nblocks, NRED, h->partial, h->partial2);
            src = h->partial2;
            nb = nchunks;
        }
    }
    if (pe) {                                    // peer windows: the all-reduce rides inside the same single-workgroup launch
        SNS_TRY(peer_check(h->comm.get()));
        ++h->ctr_allreduce;
        if (pe->host_sync) {                     // team: reduce + contribute | host barrier | sum + scalar update
            hipLaunchKernelGGL((k_reduce_final_bicg_peer<WHICH>), dim3(1), dim3(256), 0, h->stream, nb, src, red, sc,
                               peer_allreduce_args(pe, 1));
            SNS_TRY(comm_host_barrier(h->comm.get(), h->stream));
            hipLaunchKernelGGL((k_reduce_final_bicg_peer<WHICH>), dim3(1), dim3(256), 0, h->stream, nb, src, red, sc,
                               peer_allreduce_args(pe, 2));
            return SNS_OK;
        }
        hipLaunchKernelGGL((k_reduce_final_bicg_peer<WHICH>), dim3(1), dim3(256), 0, h->stream, nb, src, red, sc,
                           peer_allreduce_args(pe, 0));
        return SNS_OK;
    }
    hipLaunchKernelGGL((k_reduce_final_bicg<WHICH>), dim3(1), dim3(256), 0, h->stream, nb, src, red, sc);
    return SNS_OK;
}

inline int reduce_to(sns_ctx* h, int nblocks, int nred, double* dst_dev) {
    reduce_local(h, nblocks, nred, dst_dev);
    return allreduce(h, dst_dev, nred);
}

// ... and bring `count` doubles starting at src_dev to the host (synchronises the stream)
inline int fetch(sns_ctx* h, const double* src_dev, int count, double* out) {
    HIP_TRY(hipMemcpyAsync(h->h_scal, src_dev, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    ++h->ctr_host_syncs;
    SNS_TRY(peer_check(h->comm.get()));          // (peer transport: a collective behind this result may have given up waiting)
    std::memcpy(out, h->h_scal, count * sizeof(double));
    return SNS_OK;
}


// One pass of classical Gram-Schmidt of w against nv columns of V (leading dimension ld), in chunks of 8: the loop FGMRES, the
// Arnoldi process of the damping estimate (csrc/sns_damping.hip) and the one of the stability analysis (csrc/sns_stability.hip)
// run twice per step.  coef[c0..c0+8) = the chunk's local sums of V^T w; then finish(), where the caller completes the sums over
// the ranks and may queue further sums of the w it still sees; then w -= V coef.  nd entries per vector, g = the grid of the sums.
// CPLX: the same pass of the complex FGMRES (csrc/sns_shifted.hip) on planar complex vectors -- nd entries per part, ld the
// distance of two columns --: V^H w by k_cdot8, 16 sums per chunk, the coefficients (re, im) interleaved.
// basis_axpy is the second half on its own, w += sign * V coef: the pass ends with it, a solver's x += Z y is it.
template <bool CPLX = false>
inline void basis_axpy(sns_ctx* h, int64_t nd, int g, int nv, const double* V, int64_t ld, const double* coef, double sign, double* w) {
    for (int c0 = 0; c0 < nv; c0 += 8) {
        const int cn = std::min(8, nv - c0);
        if constexpr (CPLX)
            hipLaunchKernelGGL(k_caxpy8, dim3(g), dim3(256), 0, h->stream, nd, cn, V + (size_t)c0 * ld, ld, coef + 2 * c0, sign, w);
        else
            hipLaunchKernelGGL(k_multi_axpy8, dim3(g), dim3(256), 0, h->stream, nd, cn, V + (size_t)c0 * ld, ld, coef + c0, sign, w,
                               (double*)nullptr);
    }
}

template <bool CPLX = false, class Finish>
inline int gram_schmidt_pass(sns_ctx* h, int64_t nd, int g, int nv, const double* V, int64_t ld, double* w, double* coef,
                             Finish&& finish) {
    for (int c0 = 0; c0 < nv; c0 += 8) {
        const int cn = std::min(8, nv - c0);
        hipLaunchKernelGGL(CPLX ? k_cdot8 : k_multi_dot8, dim3(g), dim3(256), 0, h->stream, nd, cn, V + (size_t)c0 * ld, ld, w, h->partial);
        reduce_local(h, g, CPLX ? 16 : 8, coef + (CPLX ? 2 : 1) * c0);
    }
    SNS_TRY(finish());
    basis_axpy<CPLX>(h, nd, g, nv, V, ld, coef, -1.0, w);
    return SNS_OK;
}


// fill the ghost tail of a level-l vector from the owning ranks
inline int exchange_level(sns_ctx* h, int l, double* x) {
    Comm* c = h->comm.get();
    if (!c || !c->active() || c->nranks <= 1 || (size_t)l >= c->plans.size()) return SNS_OK;
    ++h->ctr_exchange;
    return comm_exchange(c, c->plans[l], x, h->stream);
}

inline int halo_exchange(sns_ctx* h, double* x) { return exchange_level(h, 0, x); }

// an illegal transition of the hand-off state (policy::Handoff) ends the call: the protocol of the carried puts was broken
inline int handoff_legal(bool legal, const char* what, int level) {
    if (legal) return SNS_OK;
    set_error(std::string("cycle hand-off: ") + what + " on level " + std::to_string(level));
    return SNS_E_STATE;
}

// The put half of the exchange of level l's vector v over a window transport -- one exchange on the counter.  The one place
// that asks whether the kernel that produced v has carried the put already, and the one caller of comm_put_carried
inline int window_put(sns_ctx* h, int l, const double* v) {
    Comm* c = h->comm.get();
    ++h->ctr_exchange;
    bool done = false;
    SNS_TRY(handoff_legal(h->handoff.take_put(l, v, &done), "an exchange while the carried put of another vector is outstanding", l));
    return done ? comm_put_carried(c, c->plans[l], h->stream) : comm_put(c, c->plans[l], v, h->stream);
}

// the buffer level l's cycle on x starts in, and the vector pc_apply(., z) cycles the fine level in: a partitioned fine level
// must see zero ghost values, z's tail may hold halo data -- an internal buffer unless nothing reads a tail as zero
inline double* cycle_start(sns_ctx* h, int l, double* x) { return policy::cycle_start(h->plan.level[(size_t)l], x, (double*)h->levels[l].pong); }
inline double* fine_cycle_vector(sns_ctx* h, double* z) {
    return (h->n > h->n_owned && !h->plan.fine_tails_unused) ? (double*)h->levels[0].x : z;
}

// Per-launch timing of the level-0 SpMV family (bench.py roofline leg): event pairs are
// recorded around every fine-level launch while h->time_kernels is set and resolved after
// the solve has synchronised.


// Multi-GPU, level 0: a pass is over every row, over the interior rows only (rows with a ghost column, flagged in h->bnd_flag, are
// skipped), over the boundary rows listed in h->bnd_rows, or -- window transports (round 5) -- over every row in one launch, the
// ghost entries read straight from the receive window `gs`.  (The values are the kernels' SPLIT template arguments.)
enum SplitMode { SPLIT_EVERY_ROW = 0, SPLIT_INTERIOR = 1, SPLIT_BOUNDARY_LIST = 2, SPLIT_WINDOW = 3 };
struct Split {
    int mode = SPLIT_EVERY_ROW;
    hipStream_t stream = nullptr;       // nullptr = the handle's stream
    int partial_off = 0;
    GhostSrc gs;
};

// The format of a level's low-precision copies (amg_f32_matrix: 1 = fp32, 2 = fp16 with row scales; a plan's lp_fmt, a level's
// binv_fmt) as a compile-time constant.  dispatch: fn(Int<V>()) for the V of Vs equal to v, the last of Vs where none is
template <int V>
using Int = std::integral_constant<int, V>;

template <int V, int... Vs, class Fn>
inline void dispatch(int v, Fn&& fn) {
    if constexpr (sizeof...(Vs) == 0) fn(Int<V>());
    else if (v == V) fn(Int<V>());
    else dispatch<Vs...>(v, fn);
}

template <class Fn>
inline void with_fmt(int fmt, Fn&& fn) { dispatch<2, 1>(fmt, fn); }

// One level pass under a split: launch(FINE, SPLIT, stream) with the two as compile-time constants -- a coarse level always over
// every row -- and the per-launch timing of the fine level as `mode`: every launch but the boundary-list pass (the interior
// pass is the bulk of a split launch)
template <class Launch>
void launch_split(sns_ctx* h, const Level& L, int mode, const Split& sp, Launch&& launch) {
    hipStream_t st = sp.stream ? sp.stream : h->stream;
    if (&L != &h->levels[0]) { launch(Int<0>(), Int<SPLIT_EVERY_ROW>(), st); return; }
    if (sp.mode == SPLIT_BOUNDARY_LIST) { launch(Int<1>(), Int<SPLIT_BOUNDARY_LIST>(), st); return; }
    hipStream_t timed = (sp.mode == SPLIT_INTERIOR || sp.mode == SPLIT_WINDOW) ? st : nullptr;   // (every row: the handle's stream)
    time_begin(h, mode, timed);
    dispatch<SPLIT_INTERIOR, SPLIT_WINDOW, SPLIT_EVERY_ROW>(sp.mode, [&](auto S) { launch(Int<1>(), S, st); });
    time_end(h, timed);
}

// y = A_l x (or fused variants).  rows = number of block rows computed.
template <int MODE>
void launch_spmv(sns_ctx* h, const Level& L, int32_t rows, const double* x, double* y, const double* b,
                 double omega, const double* dotw, Split sp = Split()) {
    if (sp.mode == SPLIT_BOUNDARY_LIST) rows = h->n_bnd;
    const int grid = (rows + 31) / 32;
    if (grid == 0) return;
    launch_split(h, L, MODE, sp, [&](auto FINE, auto S, hipStream_t st) {
        if constexpr (FINE != 0 || MODE != SPMV_AX_DOT) {
            const bool part = S == SPLIT_INTERIOR || S == SPLIT_BOUNDARY_LIST;
            hipLaunchKernelGGL((k_spmv<MODE, FINE, FINE, S>), dim3(grid), dim3(256), 0, st, rows, L.rowptr, L.colind, L.vals, x, y,
                               b, L.dinv, omega, dotw, h->partial, S == SPLIT_BOUNDARY_LIST ? h->bnd_rows : (const int32_t*)nullptr,
                               S == SPLIT_INTERIOR ? h->bnd_flag : (const uint8_t*)nullptr, part ? sp.partial_off : 0,
                               S == SPLIT_WINDOW ? sp.gs : GhostSrc());
        }
    });
}


// a level's matrix copy in format F -- values and row scales (nullptr in fp32) -- and the same of M = A P (borrowed pointers)
struct LpMat {
    const void* vals;
    const float* scale;
};
template <int F>
inline LpMat lp_mat(const Level& L) { return F == 2 ? LpMat{L.vals16, L.scale16} : LpMat{L.vals32, nullptr}; }
template <int F>
inline LpMat ap_mat(const Level& L) { return F == 2 ? LpMat{L.ap_vals16, L.ap_scale16} : LpMat{L.ap_vals32, nullptr}; }


// Preconditioner passes (Jacobi sweep, residual) of the AMG cycle on the low-precision copy of the level matrix
template <int MODE, int FINE, int SPLIT, int FMT>
void launch_lp(sns_ctx* h, const Level& L, int32_t rows, hipStream_t st, const double* x, double* y, const double* b,
               double omega, const GhostSrc& gs = GhostSrc()) {
    const int grid = (rows + 63) / 64;
    if (grid == 0) return;
    hipLaunchKernelGGL((k_spmv_lp<MODE, FINE, SPLIT, FMT, 1>), dim3(grid), dim3(256), 0, st, rows, L.rowptr, L.colind,
                       lp_mat<FMT>(L).vals, L.scale16, x, y, b, L.dinv32, omega, SPLIT == 2 ? h->bnd_rows : (const int32_t*)nullptr,
                       SPLIT == 1 ? h->bnd_flag : (const uint8_t*)nullptr, gs);
}

// (fmt: the level's plan, lp_fmt; 0 = the fp64 operator)
template <int MODE>
void launch_pc_spmv(sns_ctx* h, const Level& L, int fmt, int32_t rows, const double* x, double* y, const double* b,
                    double omega, Split sp = Split()) {
    if (fmt == 0) {
        launch_spmv<MODE>(h, L, rows, x, y, b, omega, nullptr, sp);
        return;
    }
    with_fmt(fmt, [&](auto F) {
        launch_split(h, L, MODE, sp, [&](auto FINE, auto S, hipStream_t st) {
            launch_lp<MODE, FINE, S, F>(h, L, S == SPLIT_BOUNDARY_LIST ? h->n_bnd : rows, st, x, y, b, omega,
                                        S == SPLIT_WINDOW ? sp.gs : GhostSrc());
        });
    });
}


// Level-0 pass whose input needs a halo exchange first (multi-GPU): the exchange of xe's ghost tail runs on the
// handle's stream (every RCCL call stays on ONE stream, in program order) while the interior rows -- the rows
// without a ghost column, i.e. nearly all of them -- are computed on a second stream; the few boundary rows follow
// once the halo has been unpacked.  `pc` selects the preconditioner flavour of the kernel (fp32 matrix copy).
// Without a transport, with a single rank or with SNS_NO_OVERLAP set this is exchange + one full pass.
template <int MODE>
int exchange_and_spmv(sns_ctx* h, double* xe, const double* x, double* y, const double* b, double omega,
                      const double* dotw, bool pc) {
    Level& L = h->levels[0];
    const int32_t rows = h->n_owned;
    Comm* c = h->comm.get();
    const bool dist = c && c->active() && c->nranks > 1;
    h->bnd_dot_blocks = 0;
    auto pass = [&](Split sp) {
        if constexpr (MODE == SPMV_B_MINUS_AX || MODE == SPMV_JACOBI) {
            if (pc) { launch_pc_spmv<MODE>(h, L, h->plan.level[0].lp_fmt, rows, x, y, b, omega, sp); return; }
        }
        launch_spmv<MODE>(h, L, rows, x, y, b, omega, dotw, sp);
    };
    if (dist && h->plan.fine_windows && xe == x) {
        // window transports: ONE put launch; the pass reads the ghost entries from the receive window and its boundary waves
        // wait for the neighbours' flags themselves -- no unpack, no boundary launch, no second stream
        SNS_TRY(window_put(h, 0, xe));                   // (the cycle's last kernel may have put it)
        Split s3;
        s3.mode = SPLIT_WINDOW;
        s3.gs = comm_ghost_src(c, c->plans[0]);
        pass(s3);
        h->dot_partials = (rows + 31) / 32;              // (one per workgroup in this form of the pass)
        return SNS_OK;
    }
    h->dot_partials = 4 * ((rows + 31) / 32);            // one per wave ...

    if (!dist || !h->bnd_flag || h->no_overlap || !h->opt.halo_overlap) {
        SNS_TRY(halo_exchange(h, xe));
        pass(Split());
        return SNS_OK;
    }
    const int gs = (rows + 31) / 32;                 // partial sums exist in the fp64 AX_DOT pass only
    Split s1, s2;
    s1.mode = SPLIT_INTERIOR;
    s2.mode = SPLIT_BOUNDARY_LIST;
    s2.partial_off = gs;
    if (MODE == SPMV_AX_DOT) { h->bnd_dot_blocks = (h->n_bnd + 31) / 32; h->dot_partials += 4 * h->bnd_dot_blocks; }   // ... of both launches
    if (c->nccl || (c->peer && !c->team) || h->team_overlap) {
        // (team transport with SNS_TEAM_OVERLAP=1: the same two-stream choreography -- interior pass on the side
        // stream, event joins, per-launch timing events on that stream -- over the emulated exchange, so that the
        // stream dependencies of the production path are exercised on a 1-GPU box)
        if (!h->side_stream) {
            int lo = 0, hi = 0;
            (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
            HIP_TRY(hipStreamCreateWithPriority(h->side_stream.put(), hipStreamNonBlocking, lo));
            HIP_TRY(hipEventCreateWithFlags(h->ev_x.put(), hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(h->ev_side.put(), hipEventDisableTiming));
        }
        HIP_TRY(hipEventRecord(h->ev_x, h->stream));                 // x (owned part) is ready
        HIP_TRY(hipStreamWaitEvent(h->side_stream, h->ev_x, 0));
        s1.stream = h->side_stream;
        pass(s1);                                                    // interior rows, concurrent with the halo
        HIP_TRY(hipEventRecord(h->ev_side, h->side_stream));
        SNS_TRY(halo_exchange(h, xe));                               // pack, ncclSend/Recv group, unpack
        pass(s2);                                                    // boundary rows
        HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_side, 0));       // y complete for whatever comes next
    } else {
        // team transport (tests, default): the exchange synchronises the host anyway; same two passes, one stream
        SNS_TRY(halo_exchange(h, xe));
        pass(s1);
        pass(s2);
    }
    return SNS_OK;
}


// one smoothing sweep y = x + w S (b - A x) of a level: S = the aggregates' inverse blocks where its plan has blocks, else the
// nodal D^-1.  gs: the ghost entries of x come from this receive window (the window form of the cycle; blocks only); pd: the put
// the sweep carries
inline void launch_sweep(sns_ctx* h, const policy::LevelPlan& P, const Level& L, int32_t rows, const double* x, double* y,
                         const double* b, double omega, const GhostSrc* gs = nullptr, const PutDst& pd = PutDst()) {
    if (!P.blocks) {
        launch_pc_spmv<SPMV_JACOBI>(h, L, P.lp_fmt, rows, x, y, b, omega);
        return;
    }
    const int32_t ns = 8 * L.n_blk;
    const unsigned grid = (unsigned)((ns + 63) / 64);
    if (grid == 0) return;
    with_fmt(L.binv_fmt, [&](auto F) {
        dispatch<1, 0>(gs != nullptr, [&](auto G) {
            const LpMat A = lp_mat<F>(L);
            hipLaunchKernelGGL((k_bsweep<F, G>), dim3(grid), dim3(256), 0, h->stream, ns, L.blk_rows, L.rowptr, L.colind, A.vals,
                               A.scale, (const void*)L.binv32, x, y, b, omega, gs ? *gs : GhostSrc(), pd);
        });
    });
}

// first sweep of a cycle from the zero guess, z = w S b (omega = 1: S b alone, the spectral estimate's operator)
inline void launch_first_sweep(sns_ctx* h, const policy::LevelPlan& P, const Level& L, int32_t rows, const double* b, double omega,
                               double* z, PutDst* pd = nullptr) {
    if (rows <= 0) return;
    const int g4 = (int)((4 * (int64_t)rows + 255) / 256);
    if (P.blocks) {
        const int32_t ns = 8 * L.n_blk;
        with_fmt(L.binv_fmt, [&](auto F) {
            hipLaunchKernelGGL((k_bfirst<F>), dim3((unsigned)((ns + 63) / 64)), dim3(256), 0, h->stream, ns, L.blk_rows,
                               (const void*)L.binv32, b, omega, z, pd ? *pd : PutDst());
        });
        return;
    }
    if (pd) *pd = PutDst();                              // (the nodal first sweeps do not carry a put)
    if (P.lp_fmt != 0) hipLaunchKernelGGL(k_bjacobi32, dim3(g4), dim3(256), 0, h->stream, rows, L.dinv32, b, omega, z);
    else hipLaunchKernelGGL(k_bjacobi, dim3(g4), dim3(256), 0, h->stream, rows, L.dinv, b, omega, z);
}


}  // namespace
