// The damping of the levels' block-Jacobi smoothers in one place: the state is Level::damping (omega and the three estimates
// behind it, policy::LevelDamping) with sns_ctx::damping_backoff and sns_ctx::pc_setups; it changes through the three transitions
// at the end of this file -- damping_decide (pc_setup), damping_back_off (krylov's retry), damping_reset (sns_set_options) -- and
// nowhere else.  The rule itself is pure host code in csrc/sns_policy.h ("smoother damping", tests/damping_policy_main.cpp); here
// are the three estimators that feed it and the launches they need.  (shared internals in csrc/sns_ctx.h; DESIGN.md, "Damping state")
#include "sns_ctx.h"

namespace sns {

// |lambda|max of Dinv*A on level l by a few power iterations (device resident; one host sync).
// The damped block-Jacobi smoother x += w Dinv (b - A x) needs w*|lambda|max < 2; on the reference's
// operator the fixed w = 0.9 already diverges at 10 M tets, so w is capped per level at the smoothing-optimal 4/(3 |lambda|max).  (Measured cliff on the coarse
// levels of the 10 M-tet Jacobian: w = 0.80 converges in 45 iterations, w >= 0.82 overflows, although the
// dominant mode itself is still damped there -- the offending mode is not the one of largest modulus.)
static int estimate_lambda_max(sns_ctx* h, int l, double* out) {
    Level& L = h->levels[l];
    const policy::LevelPlan& P = h->plan.level[(size_t)l];
    const int32_t rows = L.n_owned;
    const int64_t nd = 4 * (int64_t)rows;
    const int g = vec_grid(nd), g4 = (int)((nd + 255) / 256);
    double* x = h->levels[l].pong;
    double* y = L.r;
    double* z = L.x;
    // deterministic start vector with all frequencies: x_i = 1 + (i*2654435761 mod 1024)/1024 via axpby on an iota is
    // overkill; use b of the last solve if any, else the diagonal-inverse row sums: simplest robust choice = all ones
    if (rows > 0) hipLaunchKernelGGL(k_fill_pattern, dim3(g), dim3(256), 0, h->stream, nd, x);
    double* zero = nullptr;
    if (P.lp_fmt != 0) {
        SNS_TRY(get_vec(h, VEC_SCRATCH, &zero));                  // level sizes never exceed the fine level
        if (nd > 0) HIP_TRY(hipMemsetAsync(zero, 0, nd * sizeof(double), h->stream));
    }
    double lam = 0.0;
    const int iters = 12;
    // distributed levels whose sweeps see exchanged ghost values are damped for the GLOBAL operator; purely
    // rank-local sweeps (ghost values zero) for the rank-local one
    const bool glob = P.ghost_sweeps();
    for (int it = 0; it < iters; ++it) {
        if (glob) SNS_TRY(exchange_level(h, l, x));
        // the spectrum of the matrix the sweeps actually read: with a low-precision copy y = 0 - A~ x (the sign does not
        // matter to ||Dinv A x||), half the bytes of the fp64 pass
        if (P.lp_fmt != 0 && zero) launch_pc_spmv<SPMV_B_MINUS_AX>(h, L, P.lp_fmt, rows, x, y, zero, 0.0);
        else launch_spmv<SPMV_AX>(h, L, rows, x, y, nullptr, 0.0, nullptr);
        if (rows > 0) {
            if (P.blocks) launch_first_sweep(h, P, L, rows, y, 1.0, z);      // the smoother's own blocks
            else hipLaunchKernelGGL(k_bjacobi, dim3(g4), dim3(256), 0, h->stream, rows, L.dinv, y, 1.0, z);
            hipLaunchKernelGGL(k_dot2, dim3(g), dim3(256), 0, h->stream, nd, x, z, h->partial);   // (x.z, z.z)
        }
        if (glob) SNS_TRY(reduce_to(h, g, 2, h->d_scal + 16 + 2 * it));
        else reduce_local(h, g, 2, h->d_scal + 16 + 2 * it);
        // normalise with the device-side norm: x = z / ||z||  (scale read on device)
        if (rows > 0)
            hipLaunchKernelGGL(k_scale_by_rsqrt, dim3(g), dim3(256), 0, h->stream, nd, h->d_scal + 16 + 2 * it + 1, z, x);
    }
    std::vector<double> v(2 * iters);
    SNS_TRY(fetch(h, h->d_scal + 16, 2 * iters, v.data()));
    // x was normalised each step, so ||z|| of the last steps estimates |lambda|max; take the max of the tail
    for (int it = iters - 3; it < iters; ++it) lam = std::max(lam, std::sqrt(v[2 * it + 1]));
    *out = lam;
    return SNS_OK;
}


// Stability limit of the smoother damping on level l from the dominant Ritz values of S A (S = the level's smoother blocks,
// nodal or aggregate): M = 8 Arnoldi steps from the deterministic start vector of the power iteration (classical Gram-Schmidt
// with one re-orthogonalisation, the FGMRES kernels; one host read per step), eigenvalues of the 8 x 8 Hessenberg matrix on the
// host (sns_host_hessenberg_eigs).  |1 - w theta| < 1 needs w < 2 Re(theta) / |theta|^2: *limit = the minimum over the Ritz
// values with |theta| >= 0.5 |theta|max (those a few Arnoldi steps have converged to).  The power iteration above sees the
// modulus only; on a convection-dominated coarse level the dominant eigenvalues are complex, and a level that runs 1 + 6
// sweeps amplifies a damping above the limit seven times per cycle (oracle/experiments/r4_damping.py).
static int arnoldi_ritz(sns_ctx* h, int l, double* theta_max, double* limit) {
    constexpr int M = 8;
    Level& L = h->levels[l];
    const policy::LevelPlan& P = h->plan.level[(size_t)l];
    const int32_t rows = L.n_owned;
    const int64_t nd = 4 * (int64_t)rows;
    *theta_max = 0.0;
    *limit = 1e30;
    // levels whose sweeps see exchanged ghost values (plan exact): the GLOBAL operator's Ritz values -- one exchange per Arnoldi
    // step, the dots summed over the ranks; collective, so every rank goes through it whatever its row count.  (Levels that
    // exchange per sweep by amg_sweep_exchange_rows / the fine level's single post-sweep: not estimated, as in round 4.)
    const bool glob = P.exact != 0;
    if (!glob && (rows <= 0 || P.ghost_sweeps())) return SNS_OK;
    const int g = std::max(1, vec_grid(nd));           // (a rank without rows on a collective level still launches: empty loops, zero partials)
    auto reduce = [&](int nred, double* dst) -> int {
        if (glob) return reduce_to(h, g, nred, dst);
        reduce_local(h, g, nred, dst);
        return SNS_OK;
    };
    if (h->arn_V.count() < (size_t)(M + 1) * nd) SNS_TRY(h->arn_V.alloc((size_t)(M + 1) * nd));
    double* V = h->arn_V;
    double* y = L.r;
    double* zero = nullptr;
    double* xin = nullptr;                              // the SpMV input needs the level's full length (ghost tail = 0)
    SNS_TRY(get_vec(h, VEC_SCRATCH, &zero));
    SNS_TRY(get_vec(h, VEC_ARNOLDI_IN, &xin));
    HIP_TRY(hipMemsetAsync(zero, 0, nd * sizeof(double), h->stream));
    HIP_TRY(hipMemsetAsync(xin, 0, 4 * (size_t)L.n * sizeof(double), h->stream));
    double* sc = h->d_scal + 192;                      // [0, 8) pass-1 coefficients, [8, 16) pass 2, [16, 18) (w.w, w.w)
    hipLaunchKernelGGL(k_fill_pattern, dim3(g), dim3(256), 0, h->stream, nd, V);
    hipLaunchKernelGGL(k_dot2, dim3(g), dim3(256), 0, h->stream, nd, V, V, h->partial);
    SNS_TRY(reduce(2, sc + 16));
    hipLaunchKernelGGL(k_scale_by_rsqrt, dim3(g), dim3(256), 0, h->stream, nd, sc + 17, V, V);
    std::vector<double> H((size_t)M * M, 0.0);
    const bool lp = P.lp_fmt != 0;
    int m_done = 0;
    for (int j = 0; j < M; ++j) {
        double* vj = V + (size_t)j * nd;
        double* w = V + (size_t)(j + 1) * nd;
        HIP_TRY(hipMemcpyAsync(xin, vj, nd * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        if (glob) SNS_TRY(exchange_level(h, l, xin));
        // y = -A~ v (the copy the sweeps read) resp. + A v; w = S A v
        if (lp) launch_pc_spmv<SPMV_B_MINUS_AX>(h, L, P.lp_fmt, rows, xin, y, zero, 0.0);
        else launch_spmv<SPMV_AX>(h, L, rows, xin, y, nullptr, 0.0, nullptr);
        launch_first_sweep(h, P, L, rows, y, lp ? -1.0 : 1.0, w);
        for (int pass = 0; pass < 2; ++pass)               // (M = 8: one chunk)
            SNS_TRY(gram_schmidt_pass(h, nd, g, j + 1, V, nd, w, sc + 8 * pass,
                                      [&]() -> int { return glob ? allreduce(h, sc + 8 * pass, 8) : SNS_OK; }));
        hipLaunchKernelGGL(k_dot2, dim3(g), dim3(256), 0, h->stream, nd, w, w, h->partial);
        SNS_TRY(reduce(2, sc + 16));
        double v[18];
        SNS_TRY(fetch(h, sc, 18, v));
        for (int k = 0; k <= j; ++k) H[(size_t)k * M + j] = v[k] + v[8 + k];
        m_done = j + 1;
        const double wn = std::sqrt(std::max(0.0, v[16]));
        if (!(wn > 1e-12) || j + 1 == M) break;        // invariant subspace (tiny levels) or done
        H[(size_t)(j + 1) * M + j] = wn;
        hipLaunchKernelGGL(k_scale_by_rsqrt, dim3(g), dim3(256), 0, h->stream, nd, sc + 17, w, w);
    }
    std::vector<double> Hm((size_t)m_done * m_done), re((size_t)m_done), im((size_t)m_done);
    for (int i = 0; i < m_done; ++i)
        for (int j = 0; j < m_done; ++j) Hm[(size_t)i * m_done + j] = H[(size_t)i * M + j];
    if (sns_host_hessenberg_eigs(m_done, Hm.data(), re.data(), im.data()) != SNS_OK) return SNS_OK;
    double tmax = 0.0;
    for (int i = 0; i < m_done; ++i) tmax = std::max(tmax, std::hypot(re[i], im[i]));
    double lim = 1e30;
    for (int i = 0; i < m_done; ++i) {
        const double a2 = re[i] * re[i] + im[i] * im[i];
        if (std::sqrt(a2) < 0.5 * tmax || !(a2 > 0.0)) continue;
        lim = std::min(lim, 2.0 * std::max(re[i], 0.0) / a2);
    }
    *theta_max = tmax;
    *limit = lim;
    return SNS_OK;
}


// Growth factor per sweep of the damped block-Jacobi iteration matrix G_w = I - w Dinv A on the
// dominant mode of Dinv A (left in the level's pong by estimate_lambda_max).  |lambda|max alone does not bound
// the stable damping of a NON-symmetric operator (|1 - w lambda| < 1 needs w < 2 Re(lambda)/|lambda|^2):
// on the 10 M-tet Jacobian w = 0.8 converges and w = 0.85 on the coarse levels breaks BiCGStab down.
static int jacobi_growth(sns_ctx* h, int l, double omega, double* growth) {
    Level& L = h->levels[l];
    const policy::LevelPlan& P = h->plan.level[(size_t)l];
    const int32_t rows = L.n_owned;
    const int64_t nd = 4 * (int64_t)rows;
    const int g = vec_grid(nd);
    double* x0 = h->levels[l].pong;
    double* xa = L.x;
    double* xb = L.r;
    double* zero = nullptr;
    SNS_TRY(get_vec(h, VEC_SCRATCH, &zero));                      // level sizes never exceed the fine level
    if (nd > 0) HIP_TRY(hipMemsetAsync(zero, 0, nd * sizeof(double), h->stream));
    // keep x0 intact (it seeds later trials): first sweep x0 -> xa, then ping-pong xa <-> xb
    const bool glob = P.ghost_sweeps();
    if (glob) SNS_TRY(exchange_level(h, l, x0));
    launch_sweep(h, P, L, rows, x0, xa, zero, omega);
    double* cur = xa;
    double* oth = xb;
    const int sweeps = 6;
    for (int s = 1; s < sweeps; ++s) {
        if (s == 2 || s == sweeps - 1) {
            if (rows > 0) hipLaunchKernelGGL(k_dot2, dim3(g), dim3(256), 0, h->stream, nd, cur, cur, h->partial);
            if (glob) SNS_TRY(reduce_to(h, g, 2, h->d_scal + 48 + (s == 2 ? 0 : 2)));
            else reduce_local(h, g, 2, h->d_scal + 48 + (s == 2 ? 0 : 2));
        }
        if (glob) SNS_TRY(exchange_level(h, l, cur));
        launch_sweep(h, P, L, rows, cur, oth, zero, omega);
        std::swap(cur, oth);
    }
    double v[4];
    SNS_TRY(fetch(h, h->d_scal + 48, 4, v));             // ||x_2||^2, ||x_{sweeps-1}||^2
    *growth = (v[0] > 0.0) ? std::pow(v[2] / v[0], 0.5 / (double)(sweeps - 1 - 2)) : 0.0;
    // scratch vectors: only [0, nd) was written; ghost tails stay untouched
    return SNS_OK;
}


// the last level where it is solved directly: no sweeps, no estimates
static bool level_solved(const sns_ctx* h, int l, int nl) {
    const policy::LevelPlan& P = h->plan.level[(size_t)l];
    return l + 1 == nl && nl > 1 && (P.kind == SNS_LEVEL_DIRECT || P.kind == SNS_LEVEL_DIRECT_BLOCKED);
}

// whether damping_decide takes estimates on level l at this set-up (where not, it is host arithmetic alone)
bool damping_estimates_due(const sns_ctx* h, int l, int nl, bool new_operator) {
    if (h->opt.pc_type != SNS_PC_AMG || level_solved(h, l, nl)) return false;
    return policy::estimates_due(h->levels[l].damping.lambda_max > 0.0, h->pc_setups, new_operator);
}


// Decide: the damping of level l (of the nl levels the preconditioner cycles) at a set-up -- the estimators that are due,
// then the rule of csrc/sns_policy.h.  The spectrum moves little between the Jacobians of one Newton sequence, so the estimates
// are taken every fourth set-up -- but not from the Stokes operator to a Jacobian (or to another Reynolds number): round 3 took
// the first three Jacobians' damping from the Stokes solve's estimate, which is what let level 1 of the jittered 120 x 30 x 30
// duct run at w = 0.72 where its own spectrum allows 0.48 (tests/test_gpu_parity.py::
// test_damping_backoff_rescues_a_failed_linear_solve).  Levels that run 3 or more sweeps per cycle take the stability limit of
// the dominant (complex) Ritz values as well, and the growth check of rounds 1-3 (back off until a sweep contracts the dominant
// mode by >= 10 %): a level with two sweeps per cycle (the fine level, V(1,1)) does not compound an amplified mode, and backing
// its damping off for the sake of a few complex outliers weakens the smoothing of everything else (jittered 120 x 30 x 30 duct,
// Re 200: 56 iterations this way, 82 with the check on every level, 85 without it; the option that switched between the three,
// amg_growth_check, was retired in round 5).
int damping_decide(sns_ctx* h, int l, int nl, bool new_operator) {
    const sns_options& o = h->opt;
    Level& L = h->levels[l];
    policy::LevelDamping& d = L.damping;
    const policy::LevelPlan& P = h->plan.level[(size_t)l];
    const int32_t rows = L.n_owned;
    if (o.pc_type != SNS_PC_AMG || level_solved(h, l, nl)) {
        d.omega = policy::capped_damping(o.amg_omega, h->damping_backoff, 0.0, false, 0.0);
        return SNS_OK;
    }
    const bool due = damping_estimates_due(h, l, nl, new_operator);
    // (collective when the level's sweeps use exchanged ghost values: every rank takes part, rows or not)
    if (due && (rows > 0 || P.ghost_sweeps())) SNS_TRY(estimate_lambda_max(h, l, &d.lambda_max));
    const double lam = d.lambda_max;
    const bool ritz = policy::takes_ritz_limit(o, l + 1 < nl, P.pre + P.post);
    if (ritz && due && (rows > 0 || P.exact)) {
        double tmax = 0.0, lim = 1e30;
        SNS_TRY(arnoldi_ritz(h, l, &tmax, &lim));
        d.ritz_limit = lim;
        if (o.monitor) std::printf("    AMG level %d: Ritz |theta|max %.4f, damping limit 2 Re/|theta|^2 = %.4f\n", l, tmax, lim);
    }
    d.omega = policy::capped_damping(o.amg_omega, h->damping_backoff, lam, ritz, d.ritz_limit);
    if (due && lam > 0.0 && policy::takes_growth_check(l + 1 < nl, P.pre + P.post)) {
        // verify the damping on the dominant mode (left in the level's pong by estimate_lambda_max)
        SNS_TRY(policy::checked_damping(d.omega, [&](double w, double* gr) {
            SNS_TRY(jacobi_growth(h, l, w, gr));
            if (o.monitor) std::printf("    AMG level %d: omega %.4f growth/sweep on dominant mode %.4f\n", l, w, *gr);
            return (int)SNS_OK;
        }));
        d.omega_checked = d.omega;
    } else if (due && lam > 0.0) {
        d.omega_checked = 0.0;
    } else {
        d.omega = policy::held_damping(d.omega, d.omega_checked);
    }
    if (o.monitor) std::printf("    AMG level %d: n %d |lambda|max(Dinv A) %.4f omega %.4f\n", l, rows, lam, d.omega);
    return SNS_OK;
}


// Back off: krylov() after a retryable failure -- the factor and every level's stored dampings, scaled in place.  The smaller
// damping is kept for the later Jacobians of the handle (damping_decide multiplies by the factor) until sns_set_options.
void damping_back_off(sns_ctx* h) {
    policy::back_off(h->damping_backoff);
    for (auto& L : h->levels) policy::back_off(L.damping);
}


// Reset: sns_set_options.  AFTER_RETRY -- a retry's stronger damping does not outlive an options call: where the factor is not
// 1 it returns to 1, every estimate is forgotten and the next solve sets up again; nothing otherwise.  ESTIMATES -- amg_omega or
// the kind of the preconditioner changed: every estimate is taken and verified again (the caller drops pc_ready).
void damping_reset(sns_ctx* h, DampingReset what) {
    if (what == DampingReset::AFTER_RETRY) {
        if (h->damping_backoff == 1.0) return;
        h->damping_backoff = 1.0;
        h->pc_ready = false;
    }
    for (auto& L : h->levels) policy::forget_estimates(L.damping);
}

}  // namespace sns
