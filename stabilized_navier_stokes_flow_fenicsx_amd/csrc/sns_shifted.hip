// Complex and negative shifts for the stability analysis (sns_shifted_apply, sns_shifted_solve, sns_stability_arnoldi_shifted; the
// Arnoldi process itself is arnoldi_run of csrc/sns_stability.hip).  Shift-invert with s = a + i b in real Arnoldi arithmetic
// (Parlett & Saad 1987): the process runs on S = Re[(J + s B)^-1 B], a real operator with the eigenvectors of the pencil, so the
// basis, the rotation, the truncation and everything downstream stay real.  What is complex is the inner system
//     (P + c B) y = b,      P = J + p B the real matrix the handle holds and preconditions (p >= 0),  c = s - p complex,
// with B applied matrix-free.  Complex device vectors are planar: the 4 n real parts, then the 4 n imaginary parts, each part in
// the layout of a state vector.
//   k_mass_axpy_pair  y <- y + c B(w) x, or c B(w)^T x, for complex c, x, y in ONE pass over the node -> cell lists, in the shape
//                     of k_mass_apply / k_mass_apply_t (csrc/sns_stability.hip): 4 lanes per row, lane l the cells l, l + 4, ...;
//                     the geometry, u_q and tau_q are formed once per (row, cell) and serve both parts; each part's sums run in
//                     the order of the single-vector kernels, the group sum is (l0 + l1) + (l2 + l3), and the epilogue is
//                     y_re += c_re t_re - c_im t_im, y_im += c_re t_im + c_im t_re.  No atomics, no scratch, bitwise
//                     reproducible.  Rows of constrained dofs (and, transposed, pressure rows) get nothing: B is 0 there.
//                     Entries of x are masked as the single-vector kernels mask them.
//   shifted_apply     y = A x + c B x with A whatever the handle holds: two operator passes fill y, the pair pass adds -- three
//                     launches (two where c = 0: the result is then the operator pass's, bit for bit).
//   cfgmres           right-preconditioned complex FGMRES(r) on that operator -- complex arithmetic, not the real method on doubled
//                     vectors, which needs 2.5 - 3.4 times the iterations on the test ducts --: the preconditioner is
//                     pc_apply on each part, Gram-Schmidt is classical with one re-orthogonalisation in chunks of 8 (k_cdot8 /
//                     k_caxpy8, csrc/sns_kernels.hip), the Givens rotations are complex and live on the host, one host read per
//                     iteration; the true residual is computed at every restart and at the end.  The handle's gmres_restart (the
//                     cap of fgmres), ksp_rtol / ksp_atol / ksp_max_it and the PETSc-numbered reasons; no damping retry.
#include <complex>

#include "sns_ctx.h"

namespace sns {
namespace {

// one cell's share of row (node, local vertex a) for both parts: acc[p][0..2] momentum, acc[p][3] the PSPG row (mass_cell of
// csrc/sns_stability.hip with two x)
template <bool corrected>
__device__ __forceinline__ void mass_cell_pair(const int32_t* __restrict__ tets, const double* __restrict__ pts,
                                               const double* __restrict__ w, const double* __restrict__ xr, const double* __restrict__ xi,
                                               const uint8_t* __restrict__ bc_mask, int64_t t, int a, double nu, const FormVariant& fv,
                                               double acc[2][4]) {
    const int4 tv = *reinterpret_cast<const int4*>(tets + 4 * t);
    const int32_t nd[4] = {tv.x, tv.y, tv.z, tv.w};
    double X[4][3], U[4][3], Z[2][4][3];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int64_t o = 4 * (int64_t)nd[v];
        const double* pp = pts + 3 * (int64_t)nd[v];
        X[v][0] = pp[0]; X[v][1] = pp[1]; X[v][2] = pp[2];
        const double2 u01 = *reinterpret_cast<const double2*>(w + o);
        U[v][0] = u01.x; U[v][1] = u01.y; U[v][2] = w[o + 2];
        const uint32_t mk = *reinterpret_cast<const uint32_t*>(bc_mask + o);      // the node's 4 mask bytes
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const double* x = p == 0 ? xr : xi;
            const double2 x01 = *reinterpret_cast<const double2*>(x + o);
            Z[p][v][0] = (mk & 0xFFu) ? 0.0 : x01.x;
            Z[p][v][1] = (mk & 0xFF00u) ? 0.0 : x01.y;
            Z[p][v][2] = (mk & 0xFF0000u) ? 0.0 : x[o + 2];
        }
    }
    TetMetric T;
    tet_metric(X, T);
    const double wd = fabs(T.det) * (1.0 / 24.0);
    double ga[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) ga[j] = a == 0 ? T.g[0][j] : (a == 1 ? T.g[1][j] : (a == 2 ? T.g[2][j] : T.g[3][j]));
    double usum[3], zsum[2][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        usum[j] = fv.qa * (((U[0][j] + U[1][j]) + U[2][j]) + U[3][j]);
#pragma unroll
        for (int p = 0; p < 2; ++p) zsum[p][j] = fv.qa * (((Z[p][0][j] + Z[p][1][j]) + Z[p][2][j]) + Z[p][3][j]);
    }
    const double dq = fv.qb - fv.qa;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double u[3], Gu[3], uGu = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) u[j] = usum[j] + dq * U[q][j];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            Gu[i] = T.G[i][0] * u[0] + T.G[i][1] * u[1] + T.G[i][2] * u[2];
            uGu += u[i] * Gu[i];
        }
        const double tw = wd * supg_tau(0.0, uGu, fv.ci, nu, T.GG);
        const double pa = wd * (q == a ? fv.qb : fv.qa);
        const double cc = pa + tw * (u[0] * ga[0] + u[1] * ga[1] + u[2] * ga[2]);      // (corrected)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            double z[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) z[j] = zsum[p][j] + dq * Z[p][q][j];
            const double gz = ga[0] * z[0] + ga[1] * z[1] + ga[2] * z[2];
            if (corrected) {
#pragma unroll
                for (int i = 0; i < 3; ++i) acc[p][i] += cc * z[i];
            } else {
                const double c = tw * gz;
#pragma unroll
                for (int i = 0; i < 3; ++i) acc[p][i] += pa * z[i] + c * u[i];
            }
            acc[p][3] += (fv.pspg * tw) * gz;
        }
    }
}

// ... and of row (node, local vertex a) of B^T z for both parts: acc[p][0..2] (mass_cell_t of csrc/sns_stability.hip with two z)
template <bool corrected>
__device__ __forceinline__ void mass_cell_pair_t(const int32_t* __restrict__ tets, const double* __restrict__ pts,
                                                 const double* __restrict__ w, const double* __restrict__ zr, const double* __restrict__ zi,
                                                 const uint8_t* __restrict__ bc_mask, int64_t t, int a, double nu, const FormVariant& fv,
                                                 double acc[2][4]) {
    const int4 tv = *reinterpret_cast<const int4*>(tets + 4 * t);
    const int32_t nd[4] = {tv.x, tv.y, tv.z, tv.w};
    double X[4][3], U[4][3], Z[2][4][4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int64_t o = 4 * (int64_t)nd[v];
        const double* pp = pts + 3 * (int64_t)nd[v];
        X[v][0] = pp[0]; X[v][1] = pp[1]; X[v][2] = pp[2];
        const double2 u01 = *reinterpret_cast<const double2*>(w + o);
        U[v][0] = u01.x; U[v][1] = u01.y; U[v][2] = w[o + 2];
        const uint32_t mk = *reinterpret_cast<const uint32_t*>(bc_mask + o);      // the node's 4 mask bytes, the pressure's too
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const double* z = p == 0 ? zr : zi;
            const double2 z01 = *reinterpret_cast<const double2*>(z + o);
            const double2 z23 = *reinterpret_cast<const double2*>(z + o + 2);
            Z[p][v][0] = (mk & 0xFFu) ? 0.0 : z01.x;
            Z[p][v][1] = (mk & 0xFF00u) ? 0.0 : z01.y;
            Z[p][v][2] = (mk & 0xFF0000u) ? 0.0 : z23.x;
            Z[p][v][3] = (mk & 0xFF000000u) ? 0.0 : z23.y;
        }
    }
    TetMetric T;
    tet_metric(X, T);
    const double wd = fabs(T.det) * (1.0 / 24.0);
    const double dq = fv.qb - fv.qa;
    const double ms = wd * (2.0 * fv.qa * (fv.qa + fv.qb)), ma = wd * (dq * dq);
    double usum[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) usum[j] = fv.qa * (((U[0][j] + U[1][j]) + U[2][j]) + U[3][j]);
    double tu[3] = {0.0, 0.0, 0.0}, ts = 0.0;             // sum_q ta u_q, sum_q ta:  ta = w_q tau_q N_a(q)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double u[3], Gu[3], uGu = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) u[j] = usum[j] + dq * U[q][j];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            Gu[i] = T.G[i][0] * u[0] + T.G[i][1] * u[1] + T.G[i][2] * u[2];
            uGu += u[i] * Gu[i];
        }
        const double ta = (wd * supg_tau(0.0, uGu, fv.ci, nu, T.GG)) * (q == a ? fv.qb : fv.qa);
#pragma unroll
        for (int i = 0; i < 3; ++i) tu[i] += ta * u[i];
        ts += ta;
    }
    const double ps = fv.pspg * ts;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        // the Galerkin part in closed form, then grad z_c (constant on the cell) against sum_q ta u_q: the single-vector order
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double za = a == 0 ? Z[p][0][j] : (a == 1 ? Z[p][1][j] : (a == 2 ? Z[p][2][j] : Z[p][3][j]));
            acc[p][j] += ms * (((Z[p][0][j] + Z[p][1][j]) + Z[p][2][j]) + Z[p][3][j]) + ma * za;
        }
        double dz[4][3];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                dz[c][k] = ((T.g[0][k] * Z[p][0][c] + T.g[1][k] * Z[p][1][c]) + T.g[2][k] * Z[p][2][c]) + T.g[3][k] * Z[p][3][c];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double conv = corrected ? (tu[0] * dz[i][0] + tu[1] * dz[i][1]) + tu[2] * dz[i][2]
                                          : (tu[0] * dz[0][i] + tu[1] * dz[1][i]) + tu[2] * dz[2][i];
            acc[p][i] += conv + ps * dz[3][i];
        }
    }
}

// lane (i, l): cells l, l + 4, ... of row i for both parts of x (the imaginary part 4 n doubles behind the real one, in x and
// in y); then lane c adds c t to component c of both parts of y.  nu_t: the per-cell viscosity or null
template <bool corrected, bool transposed>
__global__ __launch_bounds__(256) void k_mass_axpy_pair(int32_t n, const int64_t* __restrict__ nt_ptr, const int32_t* __restrict__ nt_idx,
                                                        const int32_t* __restrict__ tets, const double* __restrict__ pts,
                                                        const double* __restrict__ w, const double* __restrict__ x,
                                                        const uint8_t* __restrict__ bc_mask, double nu, const double* __restrict__ nu_t,
                                                        FormVariant fv, double c_re, double c_im, double* __restrict__ y) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = gid >> 2;
    const int l = (int)(gid & 3);
    const int64_t ld = 4 * (int64_t)n;
    const bool live = i < n;                               // (all 4 lanes of a group agree; nobody leaves before the moves)
    const int64_t k1 = live ? nt_ptr[i + 1] : 0;
    double acc[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    for (int64_t k = (live ? nt_ptr[i] : 0) + l; k < k1; k += 4) {
        const int32_t id = nt_idx[k];                      // tet * 4 + local vertex
        const int64_t t = (int64_t)(id >> 2);
        const double nu_c = nu_t ? nu_t[t] : nu;
        if (transposed) mass_cell_pair_t<corrected>(tets, pts, w, x, x + ld, bc_mask, t, id & 3, nu_c, fv, acc);
        else mass_cell_pair<corrected>(tets, pts, w, x, x + ld, bc_mask, t, id & 3, nu_c, fv, acc);
    }
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int c = 0; c < (transposed ? 3 : 4); ++c) {
            acc[p][c] += __shfl_xor(acc[p][c], 1, 4);
            acc[p][c] += __shfl_xor(acc[p][c], 2, 4);
        }
    if (!live || (transposed && l == 3) || bc_mask[4 * i + l]) return;      // rows of B (of B^T: the pressure rows too) that are 0
    const double tr = l == 0 ? acc[0][0] : (l == 1 ? acc[0][1] : (l == 2 ? acc[0][2] : acc[0][3]));
    const double ti = l == 0 ? acc[1][0] : (l == 1 ? acc[1][1] : (l == 2 ? acc[1][2] : acc[1][3]));
    y[4 * i + l] += c_re * tr - c_im * ti;
    y[ld + 4 * i + l] += c_re * ti + c_im * tr;
}

// y += c B(w) x, or with `left` c B(w)^T x (planar complex x, y)
void launch_mass_pair(sns_ctx* h, bool left, const double* w, double c_re, double c_im, const double* x, double* y) {
    if (h->n == 0) return;
    const FormState& S = h->form;
    const dim3 grid((unsigned)((4 * (int64_t)h->n + 255) / 256));
    const double nu = 1.0 / h->opt.reynolds;
    const double* nu_t = S.ev_on ? S.ev_nu.get() : nullptr;
    dispatch<1, 0>(h->opt.corrected_convection != 0, [&](auto C) {
        if (left)
            hipLaunchKernelGGL((k_mass_axpy_pair<C() != 0, true>), grid, dim3(256), 0, h->stream, h->n, h->nt_ptr, h->nt_idx, h->tets,
                               h->pts, w, x, h->bc_mask, nu, nu_t, S.fv, c_re, c_im, y);
        else
            hipLaunchKernelGGL((k_mass_axpy_pair<C() != 0, false>), grid, dim3(256), 0, h->stream, h->n, h->nt_ptr, h->nt_idx, h->tets,
                               h->pts, w, x, h->bc_mask, nu, nu_t, S.fv, c_re, c_im, y);
    });
}

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
    // a solve opens as krylov() opens it
    if (!h->has_matrix) { set_error("shifted solve before a matrix was assembled"); return SNS_E_STATE; }
    if (!h->pc_ready && h->opt.pc_type != SNS_PC_NONE) SNS_TRY(pc_setup(h));
    int stale = -1;
    SNS_TRY(handoff_legal(h->handoff.begin_solve(&stale), "a solve begins with a carried put nobody took", stale));
    h->pc_pending = {};
    h->ctr_host_syncs = h->ctr_allreduce = h->ctr_exchange = 0;
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    SNS_TRY(ws.reserve(h));
    const sns_options& o = h->opt;
    const int m = ws.m;
    const int64_t ld = ld_of(h), n2 = 2 * ld;
    const int g = std::max(1, vec_grid(ld)), g2 = std::max(1, vec_grid(n2));
    double* V = ws.V;
    double* Z = ws.Z;
    const int CS = 2 * (m + 8);                            // stride of one pass's coefficients: (re, im) per column, chunks of 8
    double* co = ws.co;                                    // pass 1, pass 2, then (w.w, w.w)
    std::vector<cplx> H((size_t)(m + 1) * m), sn(m), gv(m + 1), y(m);
    std::vector<double> cs(m), hv((size_t)2 * CS + 2), yri((size_t)2 * m);
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
        std::fill(gv.begin(), gv.end(), cplx(0.0));
        gv[0] = rn;
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
            for (int pass = 0; pass < 2; ++pass) {
                double* dh = co + pass * CS;
                for (int c0 = 0; c0 < nv; c0 += 8) {
                    hipLaunchKernelGGL(k_cdot8, dim3(g), dim3(256), 0, h->stream, ld, std::min(8, nv - c0), V + (size_t)c0 * n2, n2, wj,
                                       h->partial);
                    reduce_local(h, g, 16, dh + 2 * c0);
                }
                if (pass == 1) {
                    hipLaunchKernelGGL(k_dot2, dim3(g2), dim3(256), 0, h->stream, n2, wj, wj, h->partial);
                    reduce_local(h, g2, 2, co + 2 * CS);
                }
                for (int c0 = 0; c0 < nv; c0 += 8)
                    hipLaunchKernelGGL(k_caxpy8, dim3(g), dim3(256), 0, h->stream, ld, std::min(8, nv - c0), V + (size_t)c0 * n2, n2,
                                       dh + 2 * c0, -1.0, wj);
            }
            SNS_TRY(read(co, 2 * CS + 2));
            cplx* Hj = &H[(size_t)j * (m + 1)];            // column j
            double h2sq = 0.0;
            for (int k = 0; k < nv; ++k) {
                const cplx h1(hv[2 * k], hv[2 * k + 1]), h2(hv[CS + 2 * k], hv[CS + 2 * k + 1]);
                Hj[k] = h1 + h2;
                h2sq += std::norm(h2);
            }
            const double ww = hv[2 * CS];
            const double wn2 = ww - h2sq;
            double wn;
            if (!(wn2 > 1e-6 * ww)) SNS_TRY(norm(wj, &wn));   // heavy cancellation: measure it
            else wn = std::sqrt(wn2);
            Hj[nv] = wn;
            if (wn > 0.0) hipLaunchKernelGGL(k_scale_copy, dim3(g2), dim3(256), 0, h->stream, n2, 1.0 / wn, wj, wj);
            // Givens rotations [cs, sn; -conj(sn), cs] with cs real
            for (int k = 0; k < j; ++k) {
                const cplx t0 = cs[k] * Hj[k] + sn[k] * Hj[k + 1];
                Hj[k + 1] = -std::conj(sn[k]) * Hj[k] + cs[k] * Hj[k + 1];
                Hj[k] = t0;
            }
            const double aa = std::abs(Hj[j]), den = std::hypot(aa, wn);
            if (den > 0.0 && aa > 0.0) {
                cs[j] = aa / den;
                sn[j] = (Hj[j] / aa) * (wn / den);
                Hj[j] = Hj[j] * (den / aa);
            } else {
                cs[j] = den > 0.0 ? 0.0 : 1.0;
                sn[j] = den > 0.0 ? 1.0 : 0.0;
                Hj[j] = wn;
            }
            Hj[j + 1] = 0.0;
            gv[j + 1] = -std::conj(sn[j]) * gv[j];
            gv[j] = cs[j] * gv[j];
            const double res = std::abs(gv[j + 1]);
            ++its;
            if (o.monitor) std::printf("%3d KSP Residual norm %.12e\n", its, res);
            if (res <= tol || wn == 0.0 || !(res == res)) { ++j; break; }
        }
        // y = H^-1 g ; x += Z y
        for (int k = j - 1; k >= 0; --k) {
            cplx sacc = gv[k];
            for (int q = k + 1; q < j; ++q) sacc -= H[(size_t)q * (m + 1) + k] * y[q];
            y[k] = sacc / H[(size_t)k * (m + 1) + k];
            yri[2 * k] = y[k].real();
            yri[2 * k + 1] = y[k].imag();
        }
        HIP_TRY(hipMemcpyAsync(co, yri.data(), (size_t)2 * j * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));             // (yri is rewritten at the next restart)
        for (int c0 = 0; c0 < j; c0 += 8)
            hipLaunchKernelGGL(k_caxpy8, dim3(g), dim3(256), 0, h->stream, ld, std::min(8, j - c0), Z + (size_t)c0 * n2, n2, co + 2 * c0,
                               1.0, x);
        SNS_TRY(residual(&rn));                            // the true residual
    }
    *its_out = its;
    *reason_out = reason;
    *rnorm_out = rn;
    h->last_ctr[0] = h->ctr_host_syncs; h->last_ctr[1] = h->ctr_allreduce; h->last_ctr[2] = h->ctr_exchange;
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

// the entry point's solve: its own buffers, for this call
int shifted_solve(sns_ctx* h, const double* w, double c_re, double c_im, bool left, const double* b, double* x, int* its, int* reason,
                  double* rnorm) {
    CfgmresWork ws;
    return cfgmres(h, w, c_re, c_im, left, b, x, its, reason, rnorm, ws);
}

}  // namespace sns
