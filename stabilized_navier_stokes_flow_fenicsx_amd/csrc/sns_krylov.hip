// Krylov methods on the device (BiCGStab with device-resident scalars, TFQMR, FGMRES) and the solve driver with the damping retry.
// (shared internals in csrc/sns_ctx.h)
#include "sns_ctx.h"

namespace sns {

int norm2(sns_ctx* h, const double* x, double* out) {
    const int64_t nd = nred_of(h);
    const int g = vec_grid(nd);
    hipLaunchKernelGGL(k_dot2, dim3(g), dim3(256), 0, h->stream, nd, x, x, h->partial);
    SNS_TRY(reduce_to(h, g, 2, h->d_scal));
    double v[2];
    SNS_TRY(fetch(h, h->d_scal, 2, v));
    *out = std::sqrt(v[0]);
    return SNS_OK;
}

int dot(sns_ctx* h, const double* x, const double* y, double* out) {
    const int64_t nd = nred_of(h);
    const int g = vec_grid(nd);
    hipLaunchKernelGGL(k_dot2, dim3(g), dim3(256), 0, h->stream, nd, x, y, h->partial);
    SNS_TRY(reduce_to(h, g, 2, h->d_scal));
    double v[2];
    SNS_TRY(fetch(h, h->d_scal, 2, v));
    *out = v[0];
    return SNS_OK;
}


// Can the Krylov kernel that writes the preconditioner's input also do the V-cycle's first fine-level sweep z = w D^-1 (input)
// (k_bicg_s_first / k_bicg_xrp_first: one dependent launch and one read of the input less per cycle)?  Returns the buffer the
// cycle of pc_apply(., zdst) starts from, or nullptr.  The fine level must own its first sweep (not where it is solved directly
// or is only the source of the replicated copy); n_owned, n_blk: a rank without rows or blocks launches nothing there
double* fused_first_sweep_target(sns_ctx* h, double* zdst) {
    if (h->opt.pc_type != SNS_PC_AMG || !h->pc_ready) return nullptr;
    if (policy::first_sweep_owner(h->plan, h->rep_level, 0) != policy::FIRST_SWEEP_LEVEL) return nullptr;
    const Level& L = h->levels[0];
    const policy::LevelPlan& P = h->plan.level[0];
    if (P.lp_fmt == 0 || L.n_owned <= 0) return nullptr;
    if (P.blocks && L.n_blk <= 0) return nullptr;                // (aggregate blocks: k_bfirst_bicg, see fused_vector_kernel)
    return cycle_start(h, 0, fine_cycle_vector(h, zdst));
}

// the put that kernel carries (k_bfirst_bicg): empty unless the fine level runs the window form of the cycle
static PutDst fine_first_put(const sns_ctx* h) {
    if (!h->plan.fuse_puts || !h->plan.level[0].windows) return PutDst();
    return comm_put_dst(h->comm.get(), h->comm->plans[0]);
}

// BiCGStab's vector update in front of the preconditioner application pc_apply(., zdst): OP 1 s = r - alpha v (k_bicg_s), OP 2 the
// x / r update with the next p (k_bicg_xrp).  Where fused_first_sweep_target allows it, the same launch does the cycle's first
// fine-level sweep: on the aggregate blocks (k_bfirst_bicg, carrying the put of the window form) or nodal
template <int OP>
static int bicg_update(sns_ctx* h, double* zdst, const double* sc, const double* ph, const double* sh, const double* t, const double* v,
                        double* x, double* r, double* p, double* s) {
    const int64_t nd = nred_of(h);
    const int g = vec_grid(nd);
    double* z1 = fused_first_sweep_target(h, zdst);
    if (!z1) {
        if (OP == 1) hipLaunchKernelGGL(k_bicg_s, dim3(g), dim3(256), 0, h->stream, nd, r, sc, v, s);
        else hipLaunchKernelGGL(k_bicg_xrp, dim3(g), dim3(256), 0, h->stream, nd, sc, ph, sh, s, t, v, x, r, p);
        return SNS_OK;
    }
    const Level& L0 = h->levels[0];
    PutDst pd0;
    if (h->plan.level[0].blocks) {
        const int32_t ns = 8 * L0.n_blk;
        pd0 = fine_first_put(h);
        with_fmt(L0.binv_fmt, [&](auto F) {
            hipLaunchKernelGGL((k_bfirst_bicg<F, OP>), dim3((unsigned)((ns + 63) / 64)), dim3(256), 0, h->stream, ns, L0.blk_rows,
                               (const void*)L0.binv32, L0.damping.omega, z1, sc, ph, sh, t, v, x, r, p, s, pd0);
        });
    } else if (OP == 1) {
        hipLaunchKernelGGL(k_bicg_s_first, dim3(g), dim3(256), 0, h->stream, nd, r, sc, v, s, L0.dinv32, L0.damping.omega, z1);
    } else {
        hipLaunchKernelGGL(k_bicg_xrp_first, dim3(g), dim3(256), 0, h->stream, nd, sc, ph, sh, s, t, v, x, r, p, L0.dinv32, L0.damping.omega,
                           z1);
    }
    return handoff_legal(h->handoff.krylov_did_first_sweep(z1, pd0.sr_ptr != nullptr), "a second carried put before the first was taken", 0);
}


// ---- BiCGStab (right-preconditioned; the recurrences of oracle/solve.py:bicgstab_bj) ----
// Latency-lean formulation: rho / alpha / omega / beta live on the device (sc[]), the vector kernels read them
// there, and the three reductions of the textbook iteration are two -- <rhat, v>, then ONE pass for
// (t.s, t.t, rhat.s, rhat.t, s.s), from which omega, the next rho and ||r||^2 follow (k_bicg_dots5).  The host
// reads (||r||^2, flags) once per iteration, asynchronously: the copy is enqueued, then the x/r update and the
// FIRST HALF of the next iteration (p, M p, A M p, <rhat, v>, alpha: none of it touches x or r) are enqueued
// behind it, and only then does the host wait for the copy's event -- the GPU never idles on the stopping test.
// Where the step plan stages that speculation (policy::plan_step: serial handles), only the update and the head of M p -- the
// fine level's cycle through its restriction -- are enqueued before the wait, the rest once the host knows that the iteration
// goes on: the queued head outlasts a host wake-up many times over, and a solve that ends throws the head away, not the half.
// A converged claim is confirmed by the explicitly computed ||r|| before the loop is left.
// The plan also says whether r0 = b - A x0 needs its operator pass (not from a guess the caller vouches to be zero: r0 = b) and
// whether the pass behind the reported true residual leaves A x in `ax` (*ax_done: it did), the residual being b minus that.
int bicgstab(sns_ctx* h, const double* b, double* x, int* its_out, int* reason_out, double* rnorm_out, int stall_window,
             const policy::StepPlan& plan, double* ax, bool* ax_done) {
    const sns_options& o = h->opt;
    const int64_t nd = nred_of(h);
    const int g = vec_grid(nd);
    double *r, *rhat, *p, *v, *s, *t, *ph, *sh;
    double** const vecs[] = {&r, &rhat, &p, &v, &s, &t, &ph, &sh};
    for (int k = 0; k < 8; ++k) SNS_TRY(get_vec(h, VEC_KRYLOV + k, vecs[k]));
    double* sc = h->d_scal + 128;                         // device scalar block of this solver
    double* red = h->d_scal + 144;                        // reduction results
    double* hpin = h->h_scal + 512;                       // pinned landing zone of (rr, flags)
    if (!h->ev_it) HIP_TRY(hipEventCreateWithFlags(h->ev_it.put(), hipEventDisableTiming));
    double bnorm, rn;
    SNS_TRY(norm2(h, b, &bnorm));
    if (plan.skip_zero_guess_residual) HIP_TRY(hipMemcpyAsync(r, b, nd * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    else SNS_TRY(op_residual(h, x, b, r));
    // ||r0||^2 stays on the device as the first rho (rhat = r0); the host needs it for the start-up test
    hipLaunchKernelGGL(k_dot2, dim3(g), dim3(256), 0, h->stream, nd, r, r, h->partial);
    SNS_TRY(reduce_to(h, g, 2, red));
    hipLaunchKernelGGL(k_bicg_init, dim3(1), dim3(64), 0, h->stream, sc, red);
    {
        double v0[2];
        SNS_TRY(fetch(h, red, 2, v0));
        rn = std::sqrt(v0[0]);
    }
    const double tol = std::max(o.ksp_rtol * bnorm, o.ksp_atol);
    if (o.monitor) std::printf("  0 KSP Residual norm %.12e\n", rn);
    int its = 0, reason = 0;
    if (!(rn == rn)) reason = SNS_KSP_DIVERGED_NANORINF;
    else reason = policy::ksp_converged(rn, tol, o.ksp_atol);
    if (!reason && o.ksp_max_it < 1) reason = SNS_KSP_DIVERGED_ITS;
    if (!reason) {
        HIP_TRY(hipMemcpyAsync(rhat, r, nd * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(hipMemsetAsync(p, 0, nd * sizeof(double), h->stream));
        HIP_TRY(hipMemsetAsync(v, 0, nd * sizeof(double), h->stream));
        // p, ph = M p, v = A ph, alpha -- in two stages: through the head of M p, and the rest
        auto first_half_begin = [&](bool p_done) -> int {
            if (!p_done) hipLaunchKernelGGL(k_bicg_p, dim3(g), dim3(256), 0, h->stream, nd, r, sc, v, p);
            h->handoff.promise_operator();
            return pc_apply_begin(h, p, ph, plan.split_cycle);
        };
        auto first_half_finish = [&]() -> int {
            SNS_TRY(pc_apply_finish(h));
            SNS_TRY(op_apply_dot(h, ph, v, rhat));        // v = A ph with the fused partial sums of <rhat, v>
            SNS_TRY(reduce_bicg<1>(h, h->dot_partials, red, sc));                  // alpha
            return SNS_OK;
        };
        // (an opened application is dropped on every way out of the loop that does not finish it)
        struct DropPending {
            sns_ctx* h;
            ~DropPending() { pc_apply_abandon(h); }
        } drop_pending{h};
        SNS_TRY(first_half_begin(false));
        SNS_TRY(first_half_finish());
        const double rn0 = rn;
        double best_rn = rn;
        int best_it = 0;
        for (its = 1;; ++its) {
            SNS_TRY(bicg_update<1>(h, sh, sc, nullptr, nullptr, nullptr, v, nullptr, r, nullptr, s));
            h->handoff.promise_operator();
            SNS_TRY(pc_apply(h, s, sh));
            SNS_TRY(op_apply(h, sh, t));
            hipLaunchKernelGGL(k_bicg_dots5, dim3(g), dim3(256), 0, h->stream, nd, s, t, rhat, h->partial);
            SNS_TRY(reduce_bicg<2>(h, g, red, sc));                       // omega, next rho / beta, ||r||^2, flags
            HIP_TRY(hipMemcpyAsync(hpin, sc + 4, 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipEventRecord(h->ev_it, h->stream));
            // speculative first half of the next iteration, enqueued BEFORE the host looks at this one's result; its p-update
            // rides on the x / r update (k_bicg_xrp).  Staged: its rest follows the look, below
            const bool spec = its < o.ksp_max_it;
            if (spec) {
                SNS_TRY(bicg_update<2>(h, ph, sc, ph, sh, t, v, x, r, p, s));
                SNS_TRY(first_half_begin(true));
                if (!plan.staged_speculation) SNS_TRY(first_half_finish());
            } else {
                hipLaunchKernelGGL(k_bicg_xr, dim3(g), dim3(256), 0, h->stream, nd, sc, ph, sh, s, t, x, r);
            }
            HIP_TRY(hipEventSynchronize(h->ev_it));
            ++h->ctr_host_syncs;
            SNS_TRY(peer_check(h->comm.get()));
            const double rr = hpin[0];
            const int flags = (int)hpin[1];
            rn = std::sqrt(rr);
            if (o.monitor) std::printf("%3d KSP Residual norm %.12e\n", its, rn);
            if ((flags & 1) || !(rn == rn) || std::isinf(rn)) { reason = SNS_KSP_DIVERGED_NANORINF; break; }
            if (rn <= tol) {
                // the three-term formula can lose digits when ||r|| << ||s||: confirm with the vector itself
                double rtrue;
                SNS_TRY(norm2(h, r, &rtrue));
                if ((reason = policy::ksp_converged(rtrue, tol, o.ksp_atol))) {
                    rn = rtrue;
                    break;
                }
            }
            if (flags & 2) { reason = SNS_KSP_DIVERGED_BREAKDOWN; break; }
            if (its >= o.ksp_max_it) { reason = SNS_KSP_DIVERGED_ITS; break; }
            // stagnation watch of the damping-retry feature (stall_window > 0 only on an attempt that can still be retried):
            // BiCGStab under an over-relaxed smoother often does not break down outright but wanders without ever getting
            // anywhere.  Only REAL stagnation ends the attempt: no new best residual at all for stall_window
            // iterations, or, after stall_window iterations, a best residual still at or above the initial one.  A solve
            // that converges slowly -- BiCGStab plateaus on convection-dominated Jacobians -- keeps setting new bests and is
            // left alone, like PETSc's bcgs would leave it.  The attempt's reason is SNS_KSP_STALLED (not a breakdown).
            if (rn < best_rn) { best_rn = rn; best_it = its; }
            if (stall_window > 0 && (its - best_it >= stall_window || (its >= stall_window && best_rn >= rn0))) {
                reason = SNS_KSP_STALLED;
                break;
            }
            if (flags & 4) { reason = SNS_KSP_DIVERGED_BREAKDOWN; ++its; break; }   // rho == 0 stops the NEXT iteration
            if (plan.staged_speculation) SNS_TRY(first_half_finish());             // the iteration goes on
        }
        pc_apply_abandon(h);
        // the stopping test runs on the RECURRENCE residual (as PETSc's bcgs does); what is reported is the true one,
        // ||b - A x|| of the returned iterate, from one more operator pass (0.5 ms of a 145-ms solve at 10 M tets)
        if (reason != SNS_KSP_DIVERGED_NANORINF) {
            if (plan.export_ax && ax) {
                // the same pass as A x, b - (A x) formed with the one rounding op_residual's epilogue has
                SNS_TRY(op_apply(h, x, ax));
                hipLaunchKernelGGL(k_axpbypcz, dim3(g), dim3(256), 0, h->stream, nd, 1.0, b, -1.0, ax, 0.0, t);
                *ax_done = true;
            } else {
                SNS_TRY(op_residual(h, x, b, t));
            }
            SNS_TRY(norm2(h, t, &rn));
        }
    }
    *its_out = its;
    *reason_out = reason;
    *rnorm_out = rn;
    return SNS_OK;
}


// ---- TFQMR (Freund 1993) on B = A M^-1: the reference's KSP type ('tfqmr', :77, :199, :282) ----
// Same recurrences as oracle/c/sns_oracle.c:orc_solve(method=1).  The quasi-residual bound
// tau*sqrt(m+1) drives the stopping test (as in PETSc); the true residual is reported at the end.
int tfqmr(sns_ctx* h, const double* b, double* x, int* its_out, int* reason_out, double* rnorm_out) {
    const sns_options& o = h->opt;
    const int64_t nd = nred_of(h);
    const int g = vec_grid(nd);
    double *w, *y1, *y2, *u1, *u2, *d, *v, *xh, *rt, *tmp;
    double** const vecs[] = {&w, &y1, &y2, &u1, &u2, &d, &v, &xh, &rt, &tmp};
    for (int k = 0; k < 10; ++k) SNS_TRY(get_vec(h, VEC_KRYLOV + k, vecs[k]));
    auto axpby = [&](double a, const double* xx, double bb, double* yy) {
        hipLaunchKernelGGL(k_axpby, dim3(g), dim3(256), 0, h->stream, nd, a, xx, bb, yy);
    };
    auto lin3 = [&](double a, const double* xx, double bb, const double* yy, double c, double* zz) {
        hipLaunchKernelGGL(k_axpbypcz, dim3(g), dim3(256), 0, h->stream, nd, a, xx, bb, yy, c, zz);
    };
    auto applyB = [&](const double* in, double* out) -> int {
        SNS_TRY(pc_apply(h, in, tmp));
        return op_apply(h, tmp, out);
    };
    double bnorm, rn;
    SNS_TRY(norm2(h, b, &bnorm));
    SNS_TRY(op_residual(h, x, b, w));
    SNS_TRY(norm2(h, w, &rn));
    const double tol = std::max(o.ksp_rtol * bnorm, o.ksp_atol);
    if (o.monitor) std::printf("  0 KSP Residual norm %.12e\n", rn);
    int its = 0, reason = 0;
    if (!(rn == rn)) reason = SNS_KSP_DIVERGED_NANORINF;
    else reason = policy::ksp_converged(rn, tol, o.ksp_atol);
    if (!reason) {
        HIP_TRY(hipMemcpyAsync(y1, w, nd * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(rt, w, nd * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        SNS_TRY(applyB(y1, v));
        HIP_TRY(hipMemcpyAsync(u1, v, nd * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(hipMemsetAsync(d, 0, nd * sizeof(double), h->stream));
        HIP_TRY(hipMemsetAsync(xh, 0, nd * sizeof(double), h->stream));
        double tau = rn, theta = 0.0, eta = 0.0, rho = rn * rn;
        bool done = false;
        for (its = 1; its <= o.ksp_max_it && !done; ++its) {
            double sigma;
            SNS_TRY(dot(h, rt, v, &sigma));
            if (sigma == 0.0 || rho == 0.0) { reason = SNS_KSP_DIVERGED_BREAKDOWN; break; }
            const double alpha = rho / sigma;
            lin3(1.0, y1, -alpha, v, 0.0, y2);
            SNS_TRY(applyB(y2, u2));
            for (int m = 0; m < 2; ++m) {
                const double* um = m == 0 ? u1 : u2;
                const double* ym = m == 0 ? y1 : y2;
                axpby(-alpha, um, 1.0, w);
                axpby(1.0, ym, theta * theta * eta / alpha, d);
                double wn;
                SNS_TRY(norm2(h, w, &wn));
                theta = wn / tau;
                const double c = 1.0 / std::sqrt(1.0 + theta * theta);
                tau = tau * theta * c;
                eta = c * c * alpha;
                axpby(eta, d, 1.0, xh);
                rn = tau * std::sqrt((double)(2 * its - 1 + m) + 1.0);
                if (o.monitor) std::printf("%3d.%d KSP Residual bound %.12e\n", its, m, rn);
                if (!(rn == rn)) { reason = SNS_KSP_DIVERGED_NANORINF; done = true; break; }
                if (rn <= tol) { done = true; break; }
            }
            if (done) break;
            double rho_new;
            SNS_TRY(dot(h, rt, w, &rho_new));
            const double beta = rho_new / rho;
            rho = rho_new;
            lin3(1.0, w, beta, y2, 0.0, y1);
            SNS_TRY(applyB(y1, u1));
            lin3(1.0, u1, beta, u2, beta * beta, v);
        }
        if (its > o.ksp_max_it) its = o.ksp_max_it;
        SNS_TRY(pc_apply(h, xh, tmp));
        axpby(1.0, tmp, 1.0, x);
        SNS_TRY(op_residual(h, x, b, w));
        SNS_TRY(norm2(h, w, &rn));
        if (!reason) {
            if (done) reason = policy::ksp_converged(rn, 10.0 * tol, o.ksp_atol);
            if (!reason) reason = SNS_KSP_DIVERGED_ITS;
        }
    }
    *its_out = its;
    *reason_out = reason;
    *rnorm_out = rn;
    return SNS_OK;
}


// ---- FGMRES(m), right preconditioning, classical Gram-Schmidt with one re-orthogonalisation ----
int fgmres(sns_ctx* h, const double* b, double* x, int* its_out, int* reason_out, double* rnorm_out) {
    const sns_options& o = h->opt;
    const int m = std::min(200, std::max(1, o.gmres_restart));
    const int64_t nd = nred_of(h), ld = ld_of(h);
    const int g = vec_grid(nd);
    if (h->gm_m != m) {
        SNS_TRY(h->gm_V.alloc((size_t)(m + 1) * ld));
        SNS_TRY(h->gm_Z.alloc((size_t)m * ld));
        SNS_TRY(h->d_h.alloc((size_t)2 * (m + 16)));
        HIP_TRY(hipMemset(h->gm_V, 0, (size_t)(m + 1) * ld * sizeof(double)));
        HIP_TRY(hipMemset(h->gm_Z, 0, (size_t)m * ld * sizeof(double)));
        h->gm_m = m;
    }
    double* V = h->gm_V;
    double* Z = h->gm_Z;
    const int S = m + 16;                 // stride of one coefficient block
    double* dh1 = h->d_h;                 // pass-1 coefficients [0, m+8)
    double* dh2 = h->d_h + S;             // pass-2 coefficients [0, m+8), then (w.w, w.w) at [m+8, m+10)
    policy::GivensLsq<double> lsq(m);
    std::vector<double> hcol(2 * (m + 16));
    double bnorm, rn;
    SNS_TRY(norm2(h, b, &bnorm));
    const double tol = std::max(o.ksp_rtol * bnorm, o.ksp_atol);
    int its = 0, reason = 0;
    double* r = V;                         // V[0] doubles as the residual vector
    SNS_TRY(op_residual(h, x, b, r));
    SNS_TRY(norm2(h, r, &rn));
    if (o.monitor) std::printf("  0 KSP Residual norm %.12e\n", rn);
    while (!reason) {
        if (!(rn == rn) || std::isinf(rn)) { reason = SNS_KSP_DIVERGED_NANORINF; break; }
        if ((reason = policy::ksp_converged(rn, tol, o.ksp_atol))) break;
        if (its >= o.ksp_max_it) { reason = SNS_KSP_DIVERGED_ITS; break; }
        hipLaunchKernelGGL(k_scale_copy, dim3(g), dim3(256), 0, h->stream, nd, 1.0 / rn, r, V);
        lsq.restart(rn);
        int j = 0;
        for (; j < m && its < o.ksp_max_it; ++j) {
            double* vj = V + (size_t)j * ld;
            double* zj = Z + (size_t)j * ld;
            double* w = V + (size_t)(j + 1) * ld;
            SNS_TRY(pc_apply(h, vj, zj));
            SNS_TRY(op_apply(h, zj, w));
            const int nv = j + 1;
            // CGS2 with TWO global reductions per iteration: pass 1 dots; pass 2 dots + (w.w), the new
            // norm follows from ||w - V h2||^2 = w.w - |h2|^2 (V orthonormal).
            for (int pass = 0; pass < 2; ++pass) {
                double* dh = pass == 0 ? dh1 : dh2;
                SNS_TRY(gram_schmidt_pass(h, nd, g, nv, V, ld, w, dh, [&]() -> int {
                    if (pass == 0) return allreduce(h, dh, nv);
                    hipLaunchKernelGGL(k_dot2, dim3(g), dim3(256), 0, h->stream, nd, w, w, h->partial);
                    reduce_local(h, g, 2, dh + (m + 8));          // k_dot2 emits (x.y, y.y): both are w.w here
                    return allreduce(h, dh, m + 10);
                }));
            }
            // one device->host transfer per iteration: h1[0..nv), h2[0..nv), w.w
            SNS_TRY(fetch(h, h->d_h, 2 * S, hcol.data()));
            double h2sq = 0.0;
            for (int k = 0; k < nv; ++k) {
                hcol[k] += hcol[S + k];                        // column j
                h2sq += hcol[S + k] * hcol[S + k];
            }
            const double ww = hcol[S + (m + 8)];
            double wn2 = ww - h2sq;
            double wn;
            if (!(wn2 > 1e-6 * ww)) SNS_TRY(norm2(h, w, &wn));   // heavy cancellation: measure it
            else wn = std::sqrt(wn2);
            if (wn > 0.0) hipLaunchKernelGGL(k_scale_copy, dim3(g), dim3(256), 0, h->stream, nd, 1.0 / wn, w, w);
            const double res = lsq.push_column(j, hcol.data(), wn);
            ++its;
            if (o.monitor) std::printf("%3d KSP Residual norm %.12e\n", its, res);
            if (res <= tol || wn == 0.0 || !(res == res)) { ++j; break; }
        }
        // y = H^-1 g ; x += Z y
        HIP_TRY(hipMemcpyAsync(dh1, lsq.solve(j).data(), j * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));             // (y is rewritten at the next restart)
        basis_axpy(h, nd, g, j, Z, ld, dh1, 1.0, x);
        SNS_TRY(op_residual(h, x, b, r));
        SNS_TRY(norm2(h, r, &rn));
    }
    *its_out = its;
    *reason_out = reason;
    *rnorm_out = rn;
    return SNS_OK;
}


// The frame of a linear solve, for krylov() and for cfgmres (csrc/sns_shifted.hip).  solve_open (`who` names the caller in the
// refusal): a matrix, the preconditioner set up if that is due, the hand-off state and the counters of a new solve, the clock
// started.  solve_close: the clock stopped and read behind a synchronise, the iterations and the kernel times booked
int solve_open(sns_ctx* h, const char* who) {
    if (!h->has_matrix) { set_error(std::string(who) + " before a matrix was assembled"); return SNS_E_STATE; }
    if (!h->pc_ready && h->opt.pc_type != SNS_PC_NONE) SNS_TRY(pc_setup(h));
    int stale = -1;
    SNS_TRY(handoff_legal(h->handoff.begin_solve(&stale), "a solve begins with a carried put nobody took", stale));
    h->pc_pending = {};
    h->ctr_host_syncs = h->ctr_allreduce = h->ctr_exchange = 0;
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    return SNS_OK;
}

int solve_close(sns_ctx* h, int its) {
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    h->tm.krylov_ms += ms;
    h->tm.ksp_its += its;
    time_collect(h);
    HIP_TRY(hipGetLastError());
    return SNS_OK;
}

int krylov(sns_ctx* h, const double* b, double* x, int* its, int* reason, double* rnorm, bool zero_guess, double* ax, bool* ax_done) {
    bool ax_unused = false;
    if (!ax_done) ax_done = &ax_unused;
    *ax_done = false;
    SNS_TRY(solve_open(h, "krylov_solve"));
    const policy::StepPlan plan = step_plan(h, zero_guess);
    // A solve that BREAKS DOWN (or produces NaN/Inf) under the AMG preconditioner is retried ONCE, from the same initial
    // guess, with every level's block-Jacobi damping backed off (damping_back_off, csrc/sns_damping.hip: policy::RETRY_FACTOR, no
    // retry at or below policy::RETRY_FLOOR; opt.amg_retry_damping, default on): the damping
    // estimate (|lambda|max of Dinv A + a growth check on the dominant mode) is not a bound for a non-symmetric
    // operator, and at cell Reynolds numbers of 5-10 a slightly over-relaxed smoother is what breaks BiCGStab down
    // (measured: jittered 648 k-tet duct, Re 200: auto damping fails after 218 iterations, 0.7 x converges).  A solve
    // that merely runs out of iterations (DIVERGED_ITS) is NOT retried: like PETSc, the reason is reported and that is
    // it.  Because BiCGStab under an over-relaxed smoother more often STAGNATES than breaks down (the same 648 k-tet case,
    // round 3: it wanders between 0.2 and 70 x ||b|| for as long as it is allowed to), the first attempt also ends -- as a
    // breakdown -- when its best residual has not halved for amg_retry_stall_its (100) iterations.  The smaller damping is kept for the later Jacobians of the handle until sns_set_options is called; the
    // retry count and the current factor are visible through sns_get_counters.  *its is the sum over both attempts
    // (<= 2 ksp_max_it).  Not in the reference; converging solves never see it.
    const bool can_retry = policy::retry_offered(h->opt, h->damping_backoff);
    double* x0 = nullptr;
    if (can_retry) {
        SNS_TRY(get_vec(h, VEC_SAVED_GUESS, &x0));
        HIP_TRY(hipMemcpyAsync(x0, x, nred_of(h) * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    }
    int its_total = 0;
    h->last_first_reason = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        int rc;
        *ax_done = false;
        // (the retry starts from the saved guess: a zero guess is the same zero vector again)
        if (h->opt.ksp_type == SNS_KSP_BICGSTAB)
            rc = bicgstab(h, b, x, its, reason, rnorm, (can_retry && attempt == 0) ? h->opt.amg_retry_stall_its : 0, plan, ax, ax_done);
        else if (h->opt.ksp_type == SNS_KSP_FGMRES) rc = fgmres(h, b, x, its, reason, rnorm);
        else if (h->opt.ksp_type == SNS_KSP_TFQMR) rc = tfqmr(h, b, x, its, reason, rnorm);
        else { set_error("bad ksp_type"); return SNS_E_ARG; }
        SNS_TRY(rc);
        its_total += *its;
        if (!policy::retryable(*reason) || !can_retry || attempt == 1) break;
        h->last_first_reason = *reason;
        ++h->ctr_retries;
        damping_back_off(h);
        if (h->opt.monitor)
            std::printf("  KSP failed (reason %d after %d iterations): retrying with the smoother damping scaled by %.2f\n",
                        *reason, *its, h->damping_backoff);
        HIP_TRY(hipMemcpyAsync(x, x0, nred_of(h) * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    }
    *its = its_total;
    h->last_ctr[0] = h->ctr_host_syncs; h->last_ctr[1] = h->ctr_allreduce; h->last_ctr[2] = h->ctr_exchange;
    SNS_TRY(halo_exchange(h, x));                          // leave the solution's ghost tail current
    return solve_close(h, *its);
}


}  // namespace sns
