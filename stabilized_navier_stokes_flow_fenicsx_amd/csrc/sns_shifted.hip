// Complex and negative shifts for the stability analysis (sns_shifted_apply, sns_shifted_solve, sns_stability_arnoldi_shifted; the
// Arnoldi process itself is arnoldi_run of csrc/sns_stability.hip).  Shift-invert with s = a + i b in real Arnoldi arithmetic
// (Parlett & Saad 1987): the process runs on S = Re[(J + s B)^-1 B], a real operator with the eigenvectors of the pencil, so the
// basis, the rotation, the truncation and everything downstream stay real.  What is complex is the inner system
//     (P + c B) y = b,      P = J + p B the real matrix the handle holds and preconditions (p >= 0),  c = s - p complex,
// with B applied matrix-free.  Complex device vectors are planar: the 4 n real parts, then the 4 n imaginary parts, each part in
// the layout of a state vector.
// This unit is host code: its kernels are the pair instantiation of the mass pass (launch_mass_pair: k_mass_pass<.., .., 2> of
// csrc/sns_stability.hip, y <- y + c B(w) x or c B(w)^T x in one pass, each part's sums those of the single-vector pass) and
// k_cdot8 / k_caxpy8 of csrc/sns_kernels.hip.
//   shifted_apply     y = A x + c B x with A whatever the handle holds: two operator passes fill y, the pair pass adds -- three
//                     launches (two where c = 0: the result is then the operator pass's, bit for bit).
//   cfgmres           right-preconditioned complex FGMRES(r) on that operator -- complex arithmetic, not the real method on doubled
//                     vectors, which needs 2.5 - 3.4 times the iterations on the test ducts --: the preconditioner is
//                     pc_apply on each part, the true residual is computed at every restart and at the end.  The handle's
//                     gmres_restart (the cap of fgmres), ksp_rtol / ksp_atol / ksp_max_it and the PETSc-numbered reasons; no
//                     damping retry.  What it shares with fgmres (csrc/sns_krylov.hip) it calls: the frame of a solve
//                     (solve_open / solve_close), classical Gram-Schmidt with one re-orthogonalisation in chunks of 8 and the
//                     update x += Z y (gram_schmidt_pass<true> / basis_axpy<true>, csrc/sns_ctx.h), the Givens least-squares
//                     problem on the host (policy::GivensLsq<std::complex<double>>, csrc/sns_policy.h).  The loop itself is its
//                     own: its buffers are CfgmresWork's, not the handle's, it reads the host once per iteration through its own
//                     buffer and reduces over no ranks -- the places where one loop for both would need a hook each.
#include <complex>

#include "sns_ctx.h"

namespace sns {
namespace {

// y = A x + c B x queued on the handle's stream (x is not written: op_apply takes it unqualified for the halo of partitioned
// handles, which do not come here)
int queue_shifted_apply(sns_ctx* h, const double* w, double c_re, double c_im, bool left, const double* x, double* y) {
    const int64_t ld = ld_of(h);
    SNS_TRY(op_apply(h, const_cast<double*>(x), y));
    SNS_TRY(op_apply(h, const_cast<double*>(x) + ld, y + ld));
    if (c_re != 0.0 || c_im != 0.0) launch_mass_pair(h, left, w, c_re, c_im, x, y);
    return SNS_OK;
}

}  // namespace

int shifted_apply(sns_ctx* h, const double* w, double c_re, double c_im, bool left, const double* x, double* y) {
    SNS_TRY(queue_shifted_apply(h, w, c_re, c_im, left, x, y));
    HIP_TRY(hipGetLastError());
    return sync_stream(h);
}

int CfgmresWork::reserve(sns_ctx* h) {
    const int r = std::min(200, std::max(1, h->opt.gmres_restart));
    const size_t n2 = 2 * (size_t)ld_of(h);
    if (r == m && V) return SNS_OK;
    SNS_TRY(V.alloc((size_t)(r + 1) * n2));
    SNS_TRY(Z.alloc((size_t)r * n2));
    SNS_TRY(co.alloc((size_t)4 * (r + 8) + 2));
    HIP_TRY(hipMemsetAsync(V, 0, (size_t)(r + 1) * n2 * sizeof(double), h->stream));
    HIP_TRY(hipMemsetAsync(Z, 0, (size_t)r * n2 * sizeof(double), h->stream));
    m = r;
    return SNS_OK;
}

// (A + c B) x = b by right-preconditioned complex FGMRES(m) from the guess in x; b, x planar complex.  *reason: the KSP reasons of
// the real solvers; *rnorm the true residual norm of the returned iterate
int cfgmres(sns_ctx* h, const double* w, double c_re, double c_im, bool left, const double* b, double* x, int* its_out, int* reason_out,
            double* rnorm_out, CfgmresWork& ws) {
    using cplx = std::complex<double>;
    *its_out = 0;
    *reason_out = 0;
    *rnorm_out = 0.0;
    SNS_TRY(solve_open(h, "shifted solve"));
    SNS_TRY(ws.reserve(h));
    const sns_options& o = h->opt;
    const int m = ws.m;
    const int64_t ld = ld_of(h), n2 = 2 * ld;
    const int g = std::max(1, vec_grid(ld)), g2 = std::max(1, vec_grid(n2));
    double* V = ws.V;
    double* Z = ws.Z;
    const int CS = 2 * (m + 8);                            // stride of one pass's coefficients: (re, im) per column, chunks of 8
    double* co = ws.co;                                    // pass 1, pass 2, then (w.w, w.w)
    policy::GivensLsq<cplx> lsq(m);
    std::vector<cplx> hcol(m);
    std::vector<double> hv((size_t)2 * CS + 2);
    auto read = [&](const double* src, int count) -> int {                      // the one host read of an iteration
        HIP_TRY(hipMemcpyAsync(hv.data(), src, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        ++h->ctr_host_syncs;
        return SNS_OK;
    };
    auto norm = [&](const double* v, double* out) -> int {
        hipLaunchKernelGGL(k_dot2, dim3(g2), dim3(256), 0, h->stream, n2, v, v, h->partial);
        reduce_local(h, g2, 2, co + 2 * CS);
        SNS_TRY(read(co + 2 * CS, 2));
        *out = std::sqrt(hv[0]);
        return SNS_OK;
    };
    double* r = V;                                         // V[0] doubles as the residual vector
    auto residual = [&](double* rn) -> int {
        SNS_TRY(queue_shifted_apply(h, w, c_re, c_im, left, x, r));
        hipLaunchKernelGGL(k_axpby, dim3(g2), dim3(256), 0, h->stream, n2, 1.0, b, -1.0, r);
        return norm(r, rn);
    };
    double bnorm, rn;
    SNS_TRY(norm(b, &bnorm));
    const double tol = std::max(o.ksp_rtol * bnorm, o.ksp_atol);
    int its = 0, reason = 0;
    SNS_TRY(residual(&rn));
    if (o.monitor) std::printf("  0 KSP Residual norm %.12e\n", rn);
    while (!reason) {
        if (!(rn == rn) || std::isinf(rn)) { reason = SNS_KSP_DIVERGED_NANORINF; break; }
        if ((reason = policy::ksp_converged(rn, tol, o.ksp_atol))) break;
        if (its >= o.ksp_max_it) { reason = SNS_KSP_DIVERGED_ITS; break; }
        hipLaunchKernelGGL(k_scale_copy, dim3(g2), dim3(256), 0, h->stream, n2, 1.0 / rn, r, V);
        lsq.restart(rn);
        int j = 0;
        for (; j < m && its < o.ksp_max_it; ++j) {
            double* vj = V + (size_t)j * n2;
            double* zj = Z + (size_t)j * n2;
            double* wj = V + (size_t)(j + 1) * n2;
            SNS_TRY(pc_apply(h, vj, zj));                  // the real preconditioner of P on each part
            SNS_TRY(pc_apply(h, vj + ld, zj + ld));
            SNS_TRY(queue_shifted_apply(h, w, c_re, c_im, left, zj, wj));
            const int nv = j + 1;
            // CGS2 as fgmres has it: pass 1 dots; pass 2 dots and w.w, the new norm from |w - V h2|^2 = w.w - |h2|^2
            for (int pass = 0; pass < 2; ++pass)
                SNS_TRY(gram_schmidt_pass<true>(h, ld, g, nv, V, n2, wj, co + pass * CS, [&]() -> int {
                    if (pass == 0) return SNS_OK;
                    hipLaunchKernelGGL(k_dot2, dim3(g2), dim3(256), 0, h->stream, n2, wj, wj, h->partial);
                    reduce_local(h, g2, 2, co + 2 * CS);
                    return SNS_OK;
                }));
            SNS_TRY(read(co, 2 * CS + 2));
            double h2sq = 0.0;
            for (int k = 0; k < nv; ++k) {
                const cplx h1(hv[2 * k], hv[2 * k + 1]), h2(hv[CS + 2 * k], hv[CS + 2 * k + 1]);
                hcol[k] = h1 + h2;                         // column j
                h2sq += std::norm(h2);
            }
            const double ww = hv[2 * CS];
            const double wn2 = ww - h2sq;
            double wn;
            if (!(wn2 > 1e-6 * ww)) SNS_TRY(norm(wj, &wn));   // heavy cancellation: measure it
            else wn = std::sqrt(wn2);
            if (wn > 0.0) hipLaunchKernelGGL(k_scale_copy, dim3(g2), dim3(256), 0, h->stream, n2, 1.0 / wn, wj, wj);
            const double res = lsq.push_column(j, hcol.data(), wn);
            ++its;
            if (o.monitor) std::printf("%3d KSP Residual norm %.12e\n", its, res);
            if (res <= tol || wn == 0.0 || !(res == res)) { ++j; break; }
        }
        // y = H^-1 g ; x += Z y (a std::complex array is its (re, im) pairs in order)
        HIP_TRY(hipMemcpyAsync(co, reinterpret_cast<const double*>(lsq.solve(j).data()), (size_t)2 * j * sizeof(double),
                               hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));             // (y is rewritten at the next restart)
        basis_axpy<true>(h, ld, g, j, Z, n2, co, 1.0, x);
        SNS_TRY(residual(&rn));                            // the true residual
    }
    *its_out = its;
    *reason_out = reason;
    *rnorm_out = rn;
    h->last_ctr[0] = h->ctr_host_syncs; h->last_ctr[1] = h->ctr_allreduce; h->last_ctr[2] = h->ctr_exchange;
    return solve_close(h, its);
}

// the entry point's solve: its own buffers, for this call
int shifted_solve(sns_ctx* h, const double* w, double c_re, double c_im, bool left, const double* b, double* x, int* its, int* reason,
                  double* rnorm) {
    CfgmresWork ws;
    return cfgmres(h, w, c_re, c_im, left, b, x, its, reason, rnorm, ws);
}

}  // namespace sns
