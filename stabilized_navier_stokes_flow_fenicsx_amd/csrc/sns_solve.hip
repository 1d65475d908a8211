// The solve drivers behind the entry points of csrc/sns_api.hip, which has checked their arguments: the Stokes solve, the Newton
// loop with the reference's bt line search, the BDF step, the scalar and adjoint solves, the Arnoldi sequence, and the pieces
// they share.  Host code only: the drivers queue launches and copies and fetch norms; when a loop stops and which step the line
// search tries next is decided in csrc/sns_policy.h ("the nonlinear drivers").  (shared internals in csrc/sns_ctx.h)
#include "sns_ctx.h"

namespace sns {

// assembles_next: the caller (a solve driver) assembles next -- with amg_aggregation = 1, 2 or 3, which aggregates the fine level by the
// assembled operator, the hierarchy waits for that assembly (the driver calls here again once it is done); any other caller
// without an assembled operator gets SNS_E_STATE and the handle stays as it was
int ensure_hierarchy(sns_ctx* h, bool assembles_next) {
    if (!h->pattern) return SNS_OK;                       // already built
    if (h->opt.pc_type != SNS_PC_AMG) return SNS_OK;      // built when (if) AMG is first asked for
    if (h->opt.amg_aggregation >= 1 && !h->has_matrix) {
        if (assembles_next) return SNS_OK;
        set_error("amg_aggregation = " + std::to_string(h->opt.amg_aggregation) + ": the hierarchy is built from the assembled operator; assemble first");
        return SNS_E_STATE;
    }
    int rc = build_hierarchy(h, *h->pattern);
    h->pattern.reset();
    return rc;
}

// Handle state borrowed for one call and given back at its end (adjoint_solve, stability_arnoldi): the fine operator
// flipped in place (`flipped`) and a time term set for the call (`time_term`).  rc: the call's result so far.  After a solve
// that did not converge and after an argument or state error the handle gets the untransposed operator back, with the hierarchy
// marked stale, and the steady form; the first error keeps its text.  A HIP or transport error leaves the device state
// undefined: nothing more is queued.  (The Arnoldi entry points refuse partitioned handles, so SNS_E_COMM reaches here from
// adjoint_solve alone.)
int give_back(sns_ctx* h, int rc, bool flipped, bool time_term) {
    if (rc == SNS_E_HIP || rc == SNS_E_COMM || (!flipped && !time_term)) return rc;
    const std::string err = last_error();
    int rb = SNS_OK;
    if (flipped) {
        rb = transpose_operator(h);
        pc_stale(h);
    }
    if (time_term) {
        const int rt = set_time_term(h, 0.0, 0.0, nullptr);
        if (rb == SNS_OK) rb = rt;
    }
    if (rc != SNS_OK) { set_error(err); return rc; }
    return rb;
}

// the end of a linear solve whose Dirichlet rows are identity rows: the reference's ILU-preconditioned solve returns them
// exactly, a Krylov method under AMG only to its tolerance -- a converged solve hands back the exact data `val` under `mask`
// (zero_guess: the caller zeroed x itself on the handle's stream)
int solve_and_snap(sns_ctx* h, const double* b, double* x, const uint8_t* mask, const double* val, int* its, int* reason,
                   double* rnorm, bool zero_guess) {
    SNS_TRY(krylov(h, b, x, its, reason, rnorm, zero_guess));
    if (*reason <= 0) return SNS_OK;
    const int64_t nd = nred_of(h);
    hipLaunchKernelGGL(k_snap_bc, dim3(vec_grid(nd)), dim3(256), 0, h->stream, nd, mask, val, 1e300, x);
    return sync_stream(h);
}

// the four work vectors of the Stokes and Newton drivers (4*n doubles each, zeroed), allocated at the first solve
int ensure_newton_workspace(sns_ctx* h) {
    if (h->nw_t) return SNS_OK;
    const size_t ld = (size_t)ld_of(h);
    for (DevBuf<double>* v : {&h->nw_F, &h->nw_y, &h->nw_w, &h->nw_t}) SNS_TRY(v->alloc(ld));
    for (DevBuf<double>* v : {&h->nw_F, &h->nw_y, &h->nw_w, &h->nw_t}) HIP_TRY(hipMemset(*v, 0, ld * sizeof(double)));
    return SNS_OK;
}

int stokes_solve(sns_ctx* h, double* U, int* ksp_its, int* reason, double* rnorm) {
    SNS_TRY(ensure_hierarchy(h, true));
    const int64_t nd = nred_of(h);
    SNS_TRY(ensure_newton_workspace(h));
    // one Newton step of the linear problem from w = 0:  A U = -F(0),  F(0) = lifting, F_B = -g   (:198-214)
    SNS_TRY(timed_assemble(h, SNS_FORM_STOKES, nullptr, h->nw_F, true));
    SNS_TRY(ensure_hierarchy(h));
    hipLaunchKernelGGL(k_scale_copy, dim3(vec_grid(nd)), dim3(256), 0, h->stream, nd, -1.0, h->nw_F, h->nw_F);
    HIP_TRY(hipMemsetAsync(U, 0, nd * sizeof(double), h->stream));
    return solve_and_snap(h, h->nw_F, U, h->bc_mask, h->bc_val, ksp_its, reason, rnorm, true);
}

// The Newton loop (newtonls + bt of the reference, :255-272) on whatever NS form the handle carries: the steady form for
// sns_newton_solve, the transient form of the step for time_step.
int newton_run(sns_ctx* h, double* w, int* its_out, int* reason_out, int* total_ksp, double* hist, int hist_cap) {
    SNS_TRY(ensure_hierarchy(h, true));
    const sns_options& o = h->opt;
    const int64_t nd = nred_of(h), ld = ld_of(h);
    const int g = vec_grid(nd);
    SNS_TRY(ensure_newton_workspace(h));
    double *F = h->nw_F, *y = h->nw_y, *wn = h->nw_w, *Fn = h->nw_t;
    int ksp_total = 0, nh = 0;
    auto record = [&](double f) { if (hist && nh < hist_cap) hist[nh] = f; ++nh; };
    SNS_TRY(halo_exchange(h, w));
    SNS_TRY(timed_assemble(h, SNS_FORM_NS, w, F, true));
    SNS_TRY(ensure_hierarchy(h));
    double f, f0;
    SNS_TRY(norm2(h, F, &f));
    f0 = f;
    record(f);
    if (o.monitor) std::printf("  0 SNES Function norm %.12e\n", f);
    int reason = policy::snes_start(f, o), it = 0;
    while (!reason) {
        ++it;
        // J y = F
        HIP_TRY(hipMemsetAsync(y, 0, nd * sizeof(double), h->stream));
        int kits = 0, kreason = 0;
        double krn = 0;
        // (y was zeroed here, on the solve's stream; J y of the returned iterate comes back with it where the method has it)
        double* Jy = Fn;                                     // borrow
        bool have_Jy = false;
        SNS_TRY(krylov(h, F, y, &kits, &kreason, &krn, true, Jy, &have_Jy));
        ksp_total += kits;
        if (kreason < 0) { reason = SNS_SNES_DIVERGED_LINEAR_SOLVE; break; }
        // bt line search, x_new = x - lambda y
        double initslope;
        if (!have_Jy) SNS_TRY(op_apply(h, y, Jy));
        SNS_TRY(dot(h, F, Jy, &initslope));
        double ynorm;
        SNS_TRY(norm2(h, y, &ynorm));
        policy::LineSearch ls(f, initslope);
        policy::LineSearch::Answer answer;
        double gn = 0.0;
        do {
            HIP_TRY(hipMemcpyAsync(wn, w, nd * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
            hipLaunchKernelGGL(k_axpby, dim3(g), dim3(256), 0, h->stream, nd, -ls.lambda(), y, 1.0, wn);
            SNS_TRY(halo_exchange(h, wn));
            SNS_TRY(timed_assemble(h, SNS_FORM_NS, wn, Fn, false));
            SNS_TRY(norm2(h, Fn, &gn));
            answer = ls.offer(gn);
        } while (answer == policy::LineSearch::TRY_AGAIN);
        if (answer != policy::LineSearch::ACCEPT) {
            reason = answer == policy::LineSearch::FAIL_NAN ? SNS_SNES_DIVERGED_FNORM_NAN : SNS_SNES_DIVERGED_LINE_SEARCH;
            break;
        }
        const double lam = ls.lambda();
        HIP_TRY(hipMemcpyAsync(w, wn, ld * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        // Dirichlet dofs within round-off of their data become exact (no lifting term from here on, :65)
        hipLaunchKernelGGL(k_snap_bc, dim3(vec_grid(ld)), dim3(256), 0, h->stream, ld, h->bc_mask, h->bc_val, 1e-12, w);
        double xnorm;
        SNS_TRY(norm2(h, w, &xnorm));
        f = gn;
        record(f);
        if (o.monitor) std::printf("%3d SNES Function norm %.12e  (ksp its %d, lambda %.3g)\n", it, f, kits, lam);
        reason = policy::snes_after_step(f, f0, lam * ynorm, xnorm, it, o);
        if (reason) break;
        SNS_TRY(timed_assemble(h, SNS_FORM_NS, w, F, true));
    }
    *its_out = it;
    *reason_out = reason;
    if (total_ksp) *total_ksp = ksp_total;
    return SNS_OK;
}

int time_step(sns_ctx* h, double* w, double* wprev, double dt, int order, double theta_coeff, int* its, int* reason, int* ksp_its) {
    const int64_t ld = ld_of(h);
    const int g = vec_grid(ld);
    // BDF1: u_t = (u - u^n) / dt;  BDF2: u_t = (3 u - 4 u^n + u^(n-1)) / (2 dt).  d in a workspace vector (copied by
    // set_time_term), the entry state in a buffer of its own (a step that does not converge restores it)
    double *d = nullptr, *w0 = nullptr;
    SNS_TRY(get_vec(h, VEC_SCRATCH, &d));
    if (!h->form.tt_w0) SNS_TRY(h->form.tt_w0.alloc((size_t)ld));
    w0 = h->form.tt_w0;
    const double sigma = (order == 1 ? 1.0 : 1.5) / dt, theta = theta_coeff / (dt * dt);
    hipLaunchKernelGGL(k_scale_copy, dim3(g), dim3(256), 0, h->stream, ld, (order == 1 ? -1.0 : -2.0) / dt, w, d);
    if (order == 2) hipLaunchKernelGGL(k_axpby, dim3(g), dim3(256), 0, h->stream, ld, 0.5 / dt, wprev, 1.0, d);
    HIP_TRY(hipMemcpyAsync(w0, w, ld * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    // (a dt so small that the coefficients overflow: refused in the words of the setter, as it always was)
    if (!std::isfinite(sigma) || !std::isfinite(theta)) {
        set_error("sns_set_time_term: sigma and theta must be finite and >= 0");
        return SNS_E_ARG;
    }
    SNS_TRY(set_time_term(h, sigma, theta, d));
    const int rc = newton_run(h, w, its, reason, ksp_its, nullptr, 0);
    if (rc != SNS_OK) {                                   // the entry state also where the loop gave up with an error
        if (rc != SNS_E_HIP) (void)hipMemcpy(w, w0, ld * sizeof(double), hipMemcpyDeviceToDevice);
        return rc;
    }
    if (*reason > 0) {
        if (wprev) HIP_TRY(hipMemcpyAsync(wprev, w0, ld * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    } else {
        HIP_TRY(hipMemcpyAsync(w, w0, ld * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    }
    return sync_stream(h);
}

int scalar_solve(sns_ctx* h, const double* w, const double kappa[4], double sigma, double theta, const double* src, const uint8_t* cmask,
                 const double* cval, double* c, int* its, int* reason, double* rnorm) {
    SNS_TRY(ensure_hierarchy(h, true));
    SNS_TRY(ensure_newton_workspace(h));
    SNS_TRY(scalar_system(h, w, kappa, sigma, theta, src, cmask, cval, h->nw_F));
    SNS_TRY(ensure_hierarchy(h));
    return solve_and_snap(h, h->nw_F, c, cmask, cval, its, reason, rnorm);
}

int adjoint_solve(sns_ctx* h, const double* g, double* lam, int* its, int* reason, double* rnorm) {
    SNS_TRY(transpose_operator(h));                      // (SNS_E_STATE / SNS_E_MESH: nothing was modified)
    int rc = ensure_hierarchy(h);
    // the Dirichlet rows AND columns of A are unit rows: lam_B = g_B exactly, and a converged solve hands that back; the other
    // rows' residual does not see it.  (The mask of the operator that was transposed: the scalars' own while the scalar operator
    // is the handle's matrix)
    const uint8_t* mask = h->matrix_form == SNS_FORM_SCALAR ? h->sc_mask.get() : h->bc_mask.get();
    if (rc == SNS_OK) rc = solve_and_snap(h, g, lam, mask, g, its, reason, rnorm);
    return give_back(h, rc, true, false);                // back to A, after a solve that did not converge too
}

// left: the operator is flipped between the assembly and the set-up and given back afterwards, as adjoint_solve does.  k = 0: a
// fresh process; k >= 1 (sns_stability_arnoldi_extend): the caller's decomposition continued from column k.  c (sns_stability_
// arnoldi_shifted): the complex coefficient of the shifted step on top of the assembled J + shift B, which is then the matrix
// the preconditioner is built for
int stability_arnoldi(sns_ctx* h, const double* w, double shift, bool left, int k, int m, double breakdown_rel, double* V, double* H,
                      int* m_done, int* total_ksp_its, int* reason, const double* c) {
    // J + shift B = the assembly with u_t = shift (u - u(w)): sigma = shift, theta = 0, d = -shift u(w) (pressure slots unused)
    if (shift > 0.0) {
        double* d = nullptr;
        SNS_TRY(get_vec(h, VEC_SCRATCH, &d));
        const int64_t ld = ld_of(h);
        hipLaunchKernelGGL(k_scale_copy, dim3(vec_grid(ld)), dim3(256), 0, h->stream, ld, -shift, w, d);
        SNS_TRY(set_time_term(h, shift, 0.0, d));
    }
    int rc = timed_assemble(h, SNS_FORM_NS, w, nullptr, true);
    bool flipped = false;
    if (left && rc == SNS_OK) {
        rc = transpose_operator(h);                      // (SNS_E_STATE / SNS_E_MESH: nothing was modified)
        flipped = rc == SNS_OK;
    }
    if (rc == SNS_OK) rc = ensure_hierarchy(h);
    if (rc == SNS_OK) rc = arnoldi_run(h, w, left, k, m, breakdown_rel, V, H, m_done, total_ksp_its, reason, c);
    return give_back(h, rc, flipped, shift > 0.0);       // (the assembled matrix stays J + shift B)
}

}  // namespace sns
