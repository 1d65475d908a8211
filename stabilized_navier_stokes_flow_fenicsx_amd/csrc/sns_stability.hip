// Linear stability of a steady state w of the 3-D NS form (sns_mass_apply, sns_stability_arnoldi; the reference has no
// counterpart: its forms are steady and it never asks whether the state it returns is stable).  The linearised transient problem
// is B x_t + J x = 0 with J the steady Jacobian at w and B = dR/du_t the Petrov-Galerkin mass operator of the stabilised form,
//     B[(a,i),(b,j)] = sum_q w_q N_b (N_a + tau_q u_q.g_a) delta_ij      (corrected_convection; the reference's own SUPG test
//                                                                          function dot(u, grad v) gives tau_q u_i g_a[j] N_b)
//     B[(a,p),(b,j)] = pspg sum_q w_q tau_q N_b g_a[j]                    (no pressure columns),
// at theta = 0 and u_t = 0, with the points, tau, C_I, the PSPG sign and nu (constant or per cell) of the handle's form: by
// definition B = J(sigma = 1, d = -u) - J(sigma = 0) of the assembly, which is affine in sigma where u_t = 0.  The leading
// eigenvalues lambda of J x = -lambda B x follow from Arnoldi on S = (J + s B)^-1 B: theta Ritz value of S, lambda = s - 1/theta.
//   k_mass_pass    <corrected, transposed, NP>: the one kernel of the mass passes, matrix-free, owner-computes, one pass over the
//                  node -> cell lists: 4 lanes per row.  Lane l of a row takes the cells l, l + 4, ... of the row's list and forms
//                  all 4 components of that cell's share -- the geometry, u_q and tau_q are computed once per (row, cell), not
//                  once per component and not once per input vector -- and the 4 partial rows are summed inside the group,
//                  (l0 + l1) + (l2 + l3), before lane c takes component c.  No atomics, no element scratch, a fixed order:
//                  bitwise reproducible.  No second BSR operator is stored: B has J's pattern and would cost what J costs.
//                  NP = 1 (launch_mass): y = B(w) x, stored; constrained rows are 0, constrained and pressure entries of x
//                  are not read as values.
//                  NP = 2 (launch_mass_pair, for csrc/sns_shifted.hip): y <- y + c B(w) x for planar complex c, x, y -- the
//                  imaginary part 4 n doubles behind the real one.  The cell functions run every per-part statement for both
//                  parts inside unrolled loops over p, so each part's sums are the NP = 1 sums, statement for statement (the
//                  test holds the two together with torch.equal); the epilogue is y_re += c_re t_re - c_im t_im,
//                  y_im += c_re t_im + c_im t_re and writes nothing on the rows where B is 0.
//                  Every index into Z[NP][..] and acc[NP][4] is a compile-time constant after unrolling: no scratch.
//   transposed     y = B(w)^T z (mass_cell_t), the same pass for the left (adjoint) problem J^T z = -lambda B^T z: B^T is by
//                  definition the transpose of the B above.  On a cell grad z_c is constant (P1), so with pa = w_q N_a(q),
//                  ta = w_q tau_q N_a(q) row (a, i) is  sum_q pa z_i(q) + (sum_q ta u_q).grad z_i + pspg (sum_q ta) d_i z_p
//                  (corrected_convection; the reference's test function: the middle term is sum_j (sum_q ta u_q)_j d_i z_j),
//                  pressure rows are 0 (B has no pressure columns).  Unlike B x the pass reads the pressure entries of z (the
//                  PSPG rows of B); constrained entries of z, a constrained pressure dof included, are read as 0.
//                  THE ORDER OF ITS STATEMENTS IS PART OF THE KERNEL: grad z and the first sum in closed form (z is linear on
//                  the cell) for every part first, which leaves the quadrature loop with u and tau alone -- 16 NP entries of z
//                  are dead before it starts --, then the convective and PSPG terms.  gfx950 VGPRs, corrected / plain:
//                  NP = 1: B 118 / 120 (4 waves per SIMD), B^T 134 / 134 (3); NP = 2: B 156 / 160 (3), B^T 178 / 176 (2).
//                  With the loop before the per-part work the entries of both z live across it: 200 / 200 at NP = 2.
//                  Scratch 0 everywhere.
//   arnoldi_run    plain Arnoldi without restart on S: per step one mass pass, one Krylov solve from a zero guess with the
//                  handle's options and damping retry (krylov(), as it is), classical Gram-Schmidt with one re-orthogonalisation
//                  (gram_schmidt_pass, csrc/sns_ctx.h).  One host read per step.  With `left` the same process on
//                  S_L = (J + s B)^-T B^T: the mass pass is the transposed one, the operator the handle holds is the transposed
//                  one (the entry point flips it and flips it back); nothing else differs.  Its Ritz vectors z satisfy
//                  z^T J = -lambda z^T B; the matrices are real, the pairing is z^T B x unconjugated.
// The sensitivity of an eigenvalue to the base flow and to a steady forcing contracts the modes with the Hessian of the residual:
// csrc/sns_hessian.hip.
// Thick restart (Stewart's Krylov-Schur; sns_stability_arnoldi_extend, sns_basis_rotate): the ordered Schur form of H is taken on
// the host by the caller (solver.py: krylov_schur_truncate), the device does the two things that touch V:
//   k_basis_rotate V[:, 0:n_out] <- V[:, 0:n_in] Q in place, columns n_out .. n_in - 1 zeroed.  Rows are independent: one lane owns
//                  one dof, loads its n_in values into registers (a compile-time-indexed row of NMAX = 17, 33 or 65 doubles,
//                  coalesced per column across the wave), and only then forms and stores the n_out outputs -- no lane stores a
//                  column another output of its row still has to read, and no other lane reads its row.  Q sits in LDS (at
//                  most 65 x 65 doubles = 33.8 KB), read as a broadcast.  Every sum runs over the columns in ascending order:
//                  no atomics, bitwise reproducible.  One streaming pass: reads and writes n_in * ndof * 8 B each.
//   arnoldi_run    with a first column k0 >= 1 continues a Krylov decomposition S V_k = V_{k+1} H_k the caller holds: no start
//                  vector treatment, the leading (k0 + 1) x k0 block of H kept, steps j = k0 .. m - 1 as ever.  Gram-Schmidt runs
//                  against all j + 1 columns, so the columns of H are full above the subdiagonal and its row k0 is full.
// Complex and negative shifts (sns_stability_arnoldi_shifted): the operator and its solve are csrc/sns_shifted.hip, which has no
// device code of its own; here the NP = 2 pass above, and apply_S of arnoldi_run.
// Out of scope: explicit locking / deflation of converged pairs; selections other than "nearest the shift"; a C implementation of
// the ordered Schur form (C callers have the two device primitives and sns_host_hessenberg_eigs); of
// the sensitivities, base flows with a body force or a backflow term, forcing on Dirichlet nodes and the exact form of
// E = D_w[B^T z][x]; 2-D and partitioned handles; the Carreau law.
#include "sns_ctx.h"

namespace sns {
namespace {

// one cell's share of row (node, local vertex a) for each of the NP input vectors x + p ld: acc[p][0..2] momentum, acc[p][3] the
// PSPG row.  The geometry, u_q, tau_q, ga and cc are formed once and serve every part; every index into Z and acc is a
// compile-time constant once the loops over p are unrolled
template <bool corrected, int NP>
__device__ __forceinline__ void mass_cell(const int32_t* __restrict__ tets, const double* __restrict__ pts,
                                          const double* __restrict__ w, const double* __restrict__ x, int64_t ld,
                                          const uint8_t* __restrict__ bc_mask, int64_t t, int a, double nu, const FormVariant& fv,
                                          double acc[NP][4]) {
    const int4 tv = *reinterpret_cast<const int4*>(tets + 4 * t);
    const int32_t nd[4] = {tv.x, tv.y, tv.z, tv.w};
    double X[4][3], U[4][3], Z[NP][4][3];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int64_t o = 4 * (int64_t)nd[v];
        const double* pp = pts + 3 * (int64_t)nd[v];
        X[v][0] = pp[0]; X[v][1] = pp[1]; X[v][2] = pp[2];
        const double2 u01 = *reinterpret_cast<const double2*>(w + o);
        U[v][0] = u01.x; U[v][1] = u01.y; U[v][2] = w[o + 2];
        const uint32_t mk = *reinterpret_cast<const uint32_t*>(bc_mask + o);      // the node's 4 mask bytes
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const double* xp = x + p * ld + o;
            const double2 x01 = *reinterpret_cast<const double2*>(xp);
            Z[p][v][0] = (mk & 0xFFu) ? 0.0 : x01.x;
            Z[p][v][1] = (mk & 0xFF00u) ? 0.0 : x01.y;
            Z[p][v][2] = (mk & 0xFF0000u) ? 0.0 : xp[2];
        }
    }
    TetMetric T;
    tet_metric(X, T);
    const double wd = fabs(T.det) * (1.0 / 24.0);
    double ga[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) ga[j] = a == 0 ? T.g[0][j] : (a == 1 ? T.g[1][j] : (a == 2 ? T.g[2][j] : T.g[3][j]));
    double usum[3], zsum[NP][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        usum[j] = fv.qa * (((U[0][j] + U[1][j]) + U[2][j]) + U[3][j]);
#pragma unroll
        for (int p = 0; p < NP; ++p) zsum[p][j] = fv.qa * (((Z[p][0][j] + Z[p][1][j]) + Z[p][2][j]) + Z[p][3][j]);
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
        for (int p = 0; p < NP; ++p) {
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

// ... and of row (node, local vertex a) of B^T z for each of the NP vectors z + p ld: acc[p][0..2] (the pressure rows of B^T are
// 0).  The order of the statements is part of the kernel: grad z and the closed-form Galerkin part of EVERY part first, so that
// the entries of z are dead before the quadrature loop, which runs on u and tau alone, then the convective and PSPG terms.  With
// the loop first the 16 NP entries of z live across it (the header comment has the register counts)
template <bool corrected, int NP>
__device__ __forceinline__ void mass_cell_t(const int32_t* __restrict__ tets, const double* __restrict__ pts,
                                            const double* __restrict__ w, const double* __restrict__ z, int64_t ld,
                                            const uint8_t* __restrict__ bc_mask, int64_t t, int a, double nu, const FormVariant& fv,
                                            double acc[NP][4]) {
    const int4 tv = *reinterpret_cast<const int4*>(tets + 4 * t);
    const int32_t nd[4] = {tv.x, tv.y, tv.z, tv.w};
    double X[4][3], U[4][3], Z[NP][4][4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int64_t o = 4 * (int64_t)nd[v];
        const double* pp = pts + 3 * (int64_t)nd[v];
        X[v][0] = pp[0]; X[v][1] = pp[1]; X[v][2] = pp[2];
        const double2 u01 = *reinterpret_cast<const double2*>(w + o);
        U[v][0] = u01.x; U[v][1] = u01.y; U[v][2] = w[o + 2];
        const uint32_t mk = *reinterpret_cast<const uint32_t*>(bc_mask + o);      // the node's 4 mask bytes, the pressure's too
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const double* zp = z + p * ld + o;
            const double2 z01 = *reinterpret_cast<const double2*>(zp);
            const double2 z23 = *reinterpret_cast<const double2*>(zp + 2);
            Z[p][v][0] = (mk & 0xFFu) ? 0.0 : z01.x;
            Z[p][v][1] = (mk & 0xFF00u) ? 0.0 : z01.y;
            Z[p][v][2] = (mk & 0xFF0000u) ? 0.0 : z23.x;
            Z[p][v][3] = (mk & 0xFF000000u) ? 0.0 : z23.y;
        }
    }
    TetMetric T;
    tet_metric(X, T);
    const double wd = fabs(T.det) * (1.0 / 24.0);
    // grad z_c, constant on the cell: dz[p][c][k] = d_k z_c
    double dz[NP][4][3];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                dz[p][c][k] = ((T.g[0][k] * Z[p][0][c] + T.g[1][k] * Z[p][1][c]) + T.g[2][k] * Z[p][2][c]) + T.g[3][k] * Z[p][3][c];
    // the Galerkin part needs no quadrature loop: z is linear on the cell, so with S = sum_v Z[v] and na(q) = N_a(q),
    // sum_q na(q) z(q) = sum_q na(q) (qa S + dq Z[q]) = 2 qa (qa + qb) S + dq^2 Z[a]
    const double dq = fv.qb - fv.qa;
    const double ms = wd * (2.0 * fv.qa * (fv.qa + fv.qb)), ma = wd * (dq * dq);
    double usum[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        usum[j] = fv.qa * (((U[0][j] + U[1][j]) + U[2][j]) + U[3][j]);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const double za = a == 0 ? Z[p][0][j] : (a == 1 ? Z[p][1][j] : (a == 2 ? Z[p][2][j] : Z[p][3][j]));
            acc[p][j] += ms * (((Z[p][0][j] + Z[p][1][j]) + Z[p][2][j]) + Z[p][3][j]) + ma * za;
        }
    }
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
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double conv = corrected ? (tu[0] * dz[p][i][0] + tu[1] * dz[p][i][1]) + tu[2] * dz[p][i][2]
                                          : (tu[0] * dz[p][0][i] + tu[1] * dz[p][1][i]) + tu[2] * dz[p][2][i];
            acc[p][i] += conv + ps * dz[p][3][i];
        }
}

// lane (i, l): cells l, l + 4, ... of row i for each of the NP parts of x (part p sits 4 n doubles behind part p - 1, in x and in
// y); then lane c owns component c of the row.  NP = 1: it stores y[4 i + c], 0 on a constrained row and on the pressure row of
// B^T.  NP = 2: it adds c t to both parts of y, y_re += c_re t_re - c_im t_im, y_im += c_re t_im + c_im t_re, and writes nothing
// on those rows.  nu_t: the per-cell viscosity or null
template <bool corrected, bool transposed, int NP>
__global__ __launch_bounds__(256) void k_mass_pass(int32_t n, const int64_t* __restrict__ nt_ptr, const int32_t* __restrict__ nt_idx,
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
    double acc[NP][4] = {};
    for (int64_t k = (live ? nt_ptr[i] : 0) + l; k < k1; k += 4) {
        const int32_t id = nt_idx[k];                      // tet * 4 + local vertex
        const int64_t t = (int64_t)(id >> 2);
        const double nu_c = nu_t ? nu_t[t] : nu;
        if (transposed) mass_cell_t<corrected, NP>(tets, pts, w, x, ld, bc_mask, t, id & 3, nu_c, fv, acc);
        else mass_cell<corrected, NP>(tets, pts, w, x, ld, bc_mask, t, id & 3, nu_c, fv, acc);
    }
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int c = 0; c < (transposed ? 3 : 4); ++c) {
            acc[p][c] += __shfl_xor(acc[p][c], 1, 4);
            acc[p][c] += __shfl_xor(acc[p][c], 2, 4);
        }
    if (!live) return;
    const bool zero_row = (transposed && l == 3) || bc_mask[4 * i + l];        // rows of B (of B^T: the pressure rows too) that are 0
    double t[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) t[p] = l == 0 ? acc[p][0] : (l == 1 ? acc[p][1] : (l == 2 ? acc[p][2] : acc[p][3]));
    if constexpr (NP == 1) {
        y[4 * i + l] = zero_row ? 0.0 : t[0];
    } else {
        if (zero_row) return;
        // y_re += c_re t_re - c_im t_im, y_im += c_re t_im + c_im t_re with the rounding written out: c_im t_im is rounded and
        // fused into c_re t_re, c_re t_im is rounded and fused into c_im t_re.  Not a choice made here: it is what contraction
        // made of the plain expressions in the pair kernel this one replaced (read from its gfx950 assembly, v_mul_f64 then
        // v_fma_f64 / v_fmac_f64 on those operands).  Left to contraction the choice moved with the surrounding code -- in this
        // kernel the imaginary line came out the other way round, 1 ulp in the imaginary part of some 5 % of the rows
        y[4 * i + l] += fma(c_re, t[0], -(c_im * t[1]));
        y[ld + 4 * i + l] += fma(c_im, t[0], c_re * t[1]);
    }
}

__global__ __launch_bounds__(256) void k_zero_constrained(int64_t ndof, const uint8_t* __restrict__ bc_mask, double* __restrict__ x) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ndof; i += (int64_t)gridDim.x * blockDim.x)
        if (bc_mask[i]) x[i] = 0.0;
}

// V[:, 0:n_out] <- V[:, 0:n_in] Q, columns n_out .. n_in - 1 zeroed; Q: n_in x n_out, row major.  One lane per row; the row
// lives in registers (every index into `row` is a compile-time constant) before the first store.  n_in <= NMAX.
template <int NMAX>
__global__ __launch_bounds__(256) void k_basis_rotate(int64_t ld, int n_in, int n_out, const double* __restrict__ Q, double* V) {
    extern __shared__ double Qs[];
    for (int t = threadIdx.x; t < n_in * n_out; t += blockDim.x) Qs[t] = Q[t];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ld) return;
    double row[NMAX];
#pragma unroll
    for (int c = 0; c < NMAX; ++c) row[c] = c < n_in ? V[(size_t)c * ld + i] : 0.0;
    for (int j = 0; j < n_out; ++j) {
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < NMAX; ++c)
            if (c < n_in) acc += row[c] * Qs[c * n_out + j];
        V[(size_t)j * ld + i] = acc;
    }
    for (int j = n_out; j < n_in; ++j) V[(size_t)j * ld + i] = 0.0;
}

// one launch of k_mass_pass over the node -> cell lists with the handle's form
template <int NP>
void launch_mass_pass(sns_ctx* h, bool left, const double* w, const double* x, double c_re, double c_im, double* y) {
    if (h->n == 0) return;
    const FormState& S = h->form;
    const dim3 grid((unsigned)((4 * (int64_t)h->n + 255) / 256));
    const double nu = 1.0 / h->opt.reynolds;
    const double* nu_t = S.ev_on ? S.ev_nu.get() : nullptr;
    dispatch<3, 2, 1, 0>(2 * (h->opt.corrected_convection != 0) + left, [&](auto K) {
        constexpr int k = decltype(K)::value;
        hipLaunchKernelGGL((k_mass_pass<(k & 2) != 0, (k & 1) != 0, NP>), grid, dim3(256), 0, h->stream, h->n, h->nt_ptr, h->nt_idx,
                           h->tets, h->pts, w, x, h->bc_mask, nu, nu_t, S.fv, c_re, c_im, y);
    });
}

}  // namespace

// y = B(w) x, or with `left` y = B(w)^T x
void launch_mass(sns_ctx* h, bool left, const double* w, const double* x, double* y) { launch_mass_pass<1>(h, left, w, x, 0.0, 0.0, y); }

// y += c B(w) x, or with `left` c B(w)^T x (planar complex x, y)
void launch_mass_pair(sns_ctx* h, bool left, const double* w, double c_re, double c_im, const double* x, double* y) {
    launch_mass_pass<2>(h, left, w, x, c_re, c_im, y);
}

// handle, pointers and the form state were checked by the entry point
int mass_apply(sns_ctx* h, const double* w, const double* x, double* y) {
    launch_mass(h, false, w, x, y);
    HIP_TRY(hipGetLastError());
    return sync_stream(h);
}

int mass_apply_transpose(sns_ctx* h, const double* w, const double* z, double* y) {
    launch_mass(h, true, w, z, y);
    HIP_TRY(hipGetLastError());
    return sync_stream(h);
}

// V[:, 0:n_out] <- V[:, 0:n_in] Q in place over ld_of(h) rows (Q on the host, n_in x n_out, row major; checked by the entry
// point); columns n_out .. n_in - 1 are zeroed.  Synchronises.
int basis_rotate(sns_ctx* h, int n_in, int n_out, const double* Q, double* V) {
    const int64_t ld = ld_of(h);
    const size_t nq = (size_t)n_in * n_out;
    DevBuf<double> q;
    SNS_TRY(q.alloc(nq));
    HIP_TRY(hipMemcpyAsync(q, Q, nq * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (ld > 0) {
        const dim3 grid((unsigned)((ld + 255) / 256));
        const size_t lds = nq * sizeof(double);
        if (n_in <= 17) hipLaunchKernelGGL((k_basis_rotate<17>), grid, dim3(256), lds, h->stream, ld, n_in, n_out, q, V);
        else if (n_in <= 33) hipLaunchKernelGGL((k_basis_rotate<33>), grid, dim3(256), lds, h->stream, ld, n_in, n_out, q, V);
        else hipLaunchKernelGGL((k_basis_rotate<policy::STABILITY_M_MAX + 1>), grid, dim3(256), lds, h->stream, ld, n_in, n_out, q, V);
        HIP_TRY(hipGetLastError());
    }
    return sync_stream(h);                                 // (q and the caller's Q live until here)
}

// The Arnoldi process on S = (J + shift B)^-1 B; the operator J + shift B is assembled and the hierarchy exists (the entry
// point).  V: (m + 1) columns of 4*n doubles, column 0 the start vector; H: (m + 1) x m, row major, zero beyond m_done.
// *reason: 1 all m steps done, 2 breakdown (the Krylov space is invariant: m_done columns, H[m_done][m_done - 1] = 0 and the
// column of V behind them zero), < 0 the KSP reason of an inner solve that did not converge (m_done = the steps completed).
// left: the process on (J + shift B)^-T B^T -- the mass pass is the transposed one, and the entry point has flipped the operator.
// k0 >= 1: continue the decomposition S V_k0 = V_{k0+1} H_k0 the caller holds in columns 0 .. k0 of V and the leading
// (k0 + 1) x k0 block of H (kept; the rest of H is zeroed): no start vector treatment, steps j = k0 .. m - 1, m_done starts at k0.
// c: the shifted step (csrc/sns_shifted.hip) -- S = Re[(A + c B)^-1 B], A the matrix the handle holds: the right-hand side is
// B v + 0 i, the solve the complex one from a zero guess, w its real part; everything else is the process above.
int arnoldi_run(sns_ctx* h, const double* w, bool left, int k0, int m, double breakdown_rel, double* V, double* H, int* m_done,
                int* total_its, int* reason, const double* c) {
    const int64_t ld = ld_of(h);
    const int g = std::max(1, vec_grid(ld));
    constexpr int CS = policy::STABILITY_M_MAX + 8;        // stride of one coefficient block (chunks of 8)
    DevBuf<double> b, co;                                  // b = B v; co: pass-1 and pass-2 coefficients, then (w.w, .) before and after
    DevBuf<double> cy;                                     // the shifted step's complex solution (b then holds B v + 0 i)
    CfgmresWork cw;
    SNS_TRY(b.alloc((size_t)(c ? 2 : 1) * ld));
    SNS_TRY(co.alloc((size_t)2 * CS + 4));
    if (c) {
        SNS_TRY(cy.alloc((size_t)2 * ld));
        HIP_TRY(hipMemsetAsync(b + ld, 0, (size_t)ld * sizeof(double), h->stream));
    }
    for (int r = 0; r < m + 1; ++r)
        for (int c = 0; c < m; ++c)
            if (r > k0 || c >= k0) H[(size_t)r * m + c] = 0.0;
    *m_done = k0;
    *total_its = 0;
    *reason = 1;
    // w = S v, from a zero guess; false: the inner solve did not converge (*reason holds why)
    auto apply_S = [&](const double* v, double* out, bool* ok) -> int {
        launch_mass(h, left, w, v, b);
        int its = 0, kr = 0;
        double rn = 0.0;
        if (c) {
            HIP_TRY(hipMemsetAsync(cy, 0, (size_t)2 * ld * sizeof(double), h->stream));
            SNS_TRY(cfgmres(h, w, c[0], c[1], left, b, cy, &its, &kr, &rn, cw));
            HIP_TRY(hipMemcpyAsync(out, cy, (size_t)ld * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        } else {
            HIP_TRY(hipMemsetAsync(out, 0, (size_t)ld * sizeof(double), h->stream));
            SNS_TRY(krylov(h, b, out, &its, &kr, &rn, true));
        }
        *total_its += its;
        *ok = kr > 0;
        if (!*ok) *reason = kr;
        else hipLaunchKernelGGL(k_zero_constrained, dim3(g), dim3(256), 0, h->stream, ld, h->bc_mask, out);    // (identity rows: 0 up to the tolerance)
        return SNS_OK;
    };
    auto norm_sq = [&](const double* v, double* dst) {
        hipLaunchKernelGGL(k_dot2, dim3(g), dim3(256), 0, h->stream, ld, v, v, h->partial);
        reduce_local(h, g, 2, dst);
    };
    bool ok = true;
    double hv[2 * CS + 4];
    if (k0 == 0) {
        // the start vector: constrained dofs zeroed, one application of S (it leaves the null space of B), unit norm
        double* v1 = V + (size_t)ld;
        hipLaunchKernelGGL(k_zero_constrained, dim3(g), dim3(256), 0, h->stream, ld, h->bc_mask, V);
        SNS_TRY(apply_S(V, v1, &ok));
        if (!ok) {
            HIP_TRY(hipMemsetAsync(v1, 0, (size_t)m * ld * sizeof(double), h->stream));
            return sync_stream(h);
        }
        norm_sq(v1, co + 2 * CS);
        SNS_TRY(fetch(h, co + 2 * CS, 2, hv));
        const double n0 = std::sqrt(hv[0]);
        if (!(n0 > 0.0) || !std::isfinite(n0)) {           // S v = 0: the start vector lies in the null space of B
            *reason = 2;
            HIP_TRY(hipMemsetAsync(V, 0, (size_t)(m + 1) * ld * sizeof(double), h->stream));
            return sync_stream(h);
        }
        hipLaunchKernelGGL(k_scale_copy, dim3(g), dim3(256), 0, h->stream, ld, 1.0 / n0, v1, V);
    }
    for (int j = k0; j < m; ++j) {
        double* wj = V + (size_t)(j + 1) * ld;
        SNS_TRY(apply_S(V + (size_t)j * ld, wj, &ok));
        if (!ok) {
            HIP_TRY(hipMemsetAsync(wj, 0, (size_t)ld * sizeof(double), h->stream));
            break;
        }
        const int nv = j + 1;
        norm_sq(wj, co + 2 * CS);
        for (int pass = 0; pass < 2; ++pass)
            SNS_TRY(gram_schmidt_pass(h, ld, g, nv, V, ld, wj, co + pass * CS, []() -> int { return SNS_OK; }));
        norm_sq(wj, co + 2 * CS + 2);
        SNS_TRY(fetch(h, co, 2 * CS + 4, hv));
        for (int k = 0; k < nv; ++k) H[(size_t)k * m + j] = hv[k] + hv[CS + k];
        *m_done = nv;
        const double before = std::sqrt(hv[2 * CS]), after = std::sqrt(hv[2 * CS + 2]);
        if (!(after > breakdown_rel * before)) {           // (a NaN ends the process here too)
            *reason = 2;
            HIP_TRY(hipMemsetAsync(wj, 0, (size_t)ld * sizeof(double), h->stream));
            break;
        }
        H[(size_t)(j + 1) * m + j] = after;
        hipLaunchKernelGGL(k_scale_copy, dim3(g), dim3(256), 0, h->stream, ld, 1.0 / after, wj, wj);
    }
    // the columns of V the process never reached
    const int used = *m_done + 1;
    if (used < m + 1) HIP_TRY(hipMemsetAsync(V + (size_t)used * ld, 0, (size_t)(m + 1 - used) * ld * sizeof(double), h->stream));
    HIP_TRY(hipGetLastError());
    return sync_stream(h);
}

}  // namespace sns
