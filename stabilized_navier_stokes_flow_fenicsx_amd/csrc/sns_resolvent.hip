// Resolvent analysis of a steady state w of the 3-D NS form (sns_energy_apply, sns_lumped_volumes, sns_resolvent_lanczos; the
// reference has no counterpart).  The flow linearised at w answers a harmonic body force f exp(i omega t) with q exp(i omega t),
// q = R(omega) f, R = (J + i omega B)^-1 B (solver.harmonic_response).  The gains are the singular values of R with the response
// measured in kinetic energy, |q|^2 = q^H Q q, and the forcing in the lumped volume norm, |f|^2 = f^H M_L f:
//     Q = D_q M D_q    M the consistent P1 Galerkin mass matrix on the three velocity components, on a tet
//                      M_ab = |det J| (1 + delta_ab) / 120, pressure rows and columns 0; D_q an optional nodal weight
//     M_L              the lumped nodal volumes m_i = sum over the cells of i of |det J| / 24, on the velocity dofs
// With S = D_f M_L^-1/2 (real, diagonal; D_f an optional nodal weight of the forcing) and f = S g the squared gains are the
// eigenvalues of the Hermitian positive semi-definite
//     T = S B^T (J + i omega B)^-H Q (J + i omega B)^-1 B S,
// and |f|_ML = |g|_2 where D_f = 1.
//   k_energy_pass  <NP, LUMPED>: y = Q x, built as k_mass_pass (csrc/sns_stability.hip) is: matrix-free, owner-computes, one pass
//                  over the node -> cell lists, 4 lanes per row.  Lane l takes the cells l, l + 4, ... of the row's list; a cell's
//                  share of row (a, i) is |det|/120 chi_a (sum_b chi_b x_{b,i} + chi_a x_{a,i}); the 4 partial rows are summed in
//                  the group, (l0 + l1) + (l2 + l3), and lane c takes component c.  No atomics, no element scratch, a fixed
//                  order: bitwise reproducible.  Constrained entries of x are read as 0; constrained rows and pressure rows of y
//                  are 0.  The cell needs |det J| and four weights only: the determinant is formed here from the three edges,
//                  tet_metric (K, G, g) is not called.  Every product that feeds a sum is an explicit fma, so that contraction has
//                  no choice to make and
//                  NP = 2 (planar complex x, y: the imaginary part 4 n doubles behind the real one) sums each part statement
//                  for statement as NP = 1 does -- the test holds the two together with torch.equal.
//                  LUMPED: m_i into the three velocity slots of node i, 0 into the pressure slot; no mask, x and chi not read.
//                  gfx950 VGPRs (from the cross-compile's resource remarks; waves per SIMD): <1, false> 84 (5), <2, false> 117 (4),
//                  <1, true> 44 (8); k_forcing_scale 22 (8), k_velocity_mask 10 (8).  Scratch 0 everywhere.
//   k_forcing_scale both parts of a planar vector times S: chi_f,i / sqrt(m_i) on the velocity dofs, 0 on pressure and
//                  constrained dofs (and where a node has no cell).  Out of place or in place.
//   resolvent_lanczos  the Hermitian Krylov process on T without restart, modelled on arnoldi_run: per step S, the pair mass pass
//                  (c = 1) into a zeroed vector, the forward complex solve (cfgmres, c = (0, omega)) from a zero guess, the energy
//                  pass, the operator flipped in place and set up, the adjoint solve (cfgmres with `left`, c = (0, -omega):
//                  J^T - i omega B^T = (J + i omega B)^H, the matrices are real), the operator flipped back and set up, the
//                  transposed pair mass pass, S, then classical Gram-Schmidt with one re-orthogonalisation in the complex inner
//                  product (gram_schmidt_pass<true>) and the breakdown test by the norm ratio.  One host read per step besides the
//                  solves' own.  The two flips and set-ups per step are what the library has (no transposed SpMV exists); their
//                  share of a step is recorded in profiles/resolvent.txt.
// Out of scope: 2-D and partitioned handles, the Carreau law, restarts, other norms, forcing through Dirichlet data, gain
// sensitivities, transient growth.
#include "sns_ctx.h"

namespace sns {
namespace {

// lane (i, l): cells l, l + 4, ... of row i; then lane c owns component c of the row (lane 3: the pressure row, 0).  chi: the
// nodal weight or null (all ones).  x, y: NP parts, part p sits 4 n doubles behind part p - 1.
template <int NP, bool LUMPED>
__global__ __launch_bounds__(256) void k_energy_pass(int32_t n, const int64_t* __restrict__ nt_ptr, const int32_t* __restrict__ nt_idx,
                                                     const int32_t* __restrict__ tets, const double* __restrict__ pts,
                                                     const double* __restrict__ chi, const double* __restrict__ x,
                                                     const uint8_t* __restrict__ bc_mask, double* __restrict__ y) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = gid >> 2;
    const int l = (int)(gid & 3);
    const int64_t ld = 4 * (int64_t)n;
    const bool live = i < n;                               // (all 4 lanes of a group agree; nobody leaves before the moves)
    const int64_t k1 = live ? nt_ptr[i + 1] : 0;
    double acc[NP][3] = {};
    for (int64_t k = (live ? nt_ptr[i] : 0) + l; k < k1; k += 4) {
        const int32_t id = nt_idx[k];                      // tet * 4 + local vertex
        const int a = id & 3;
        const int4 tv = *reinterpret_cast<const int4*>(tets + 4 * (int64_t)(id >> 2));
        const int32_t nd[4] = {tv.x, tv.y, tv.z, tv.w};
        double X[4][3];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const double* pp = pts + 3 * (int64_t)nd[v];
            X[v][0] = pp[0]; X[v][1] = pp[1]; X[v][2] = pp[2];
        }
        double e[3][3];                                    // the edges from vertex 0; det J = e0 . (e1 x e2)
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int j = 0; j < 3; ++j) e[r][j] = X[r + 1][j] - X[0][j];
        const double c0 = fma(e[1][1], e[2][2], -(e[1][2] * e[2][1]));
        const double c1 = fma(e[1][2], e[2][0], -(e[1][0] * e[2][2]));
        const double c2 = fma(e[1][0], e[2][1], -(e[1][1] * e[2][0]));
        const double ad = fabs(fma(e[0][2], c2, fma(e[0][1], c1, e[0][0] * c0)));
        if constexpr (LUMPED) {
            acc[0][0] += ad * (1.0 / 24.0);
        } else {
            double ch[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) ch[v] = chi ? chi[nd[v]] : 1.0;
            const double ca = a == 0 ? ch[0] : (a == 1 ? ch[1] : (a == 2 ? ch[2] : ch[3]));
            const double wa = (ad * (1.0 / 120.0)) * ca;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                double Z[4][3];
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int64_t o = 4 * (int64_t)nd[v];
                    const uint32_t mk = *reinterpret_cast<const uint32_t*>(bc_mask + o);      // the node's 4 mask bytes
                    const double* xp = x + p * ld + o;
                    const double2 x01 = *reinterpret_cast<const double2*>(xp);
                    Z[v][0] = (mk & 0xFFu) ? 0.0 : x01.x;
                    Z[v][1] = (mk & 0xFF00u) ? 0.0 : x01.y;
                    Z[v][2] = (mk & 0xFF0000u) ? 0.0 : xp[2];
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double za = a == 0 ? Z[0][c] : (a == 1 ? Z[1][c] : (a == 2 ? Z[2][c] : Z[3][c]));
                    const double s = fma(ch[3], Z[3][c], fma(ch[2], Z[2][c], fma(ch[1], Z[1][c], ch[0] * Z[0][c])));
                    acc[p][c] = fma(wa, fma(ca, za, s), acc[p][c]);
                }
            }
        }
    }
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int c = 0; c < (LUMPED ? 1 : 3); ++c) {
            acc[p][c] += __shfl_xor(acc[p][c], 1, 4);
            acc[p][c] += __shfl_xor(acc[p][c], 2, 4);
        }
    if (!live) return;
    if constexpr (LUMPED) {
        y[4 * i + l] = l == 3 ? 0.0 : acc[0][0];
    } else {
        const bool zero_row = l == 3 || bc_mask[4 * i + l];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const double t = l == 0 ? acc[p][0] : (l == 1 ? acc[p][1] : acc[p][2]);
            y[p * ld + 4 * i + l] = zero_row ? 0.0 : t;
        }
    }
}

// y = S x on both parts of a planar vector (ld doubles per part): S = chi_f,i / sqrt(m_i) on the velocity dofs of node i, 0 on
// pressure and constrained dofs.  chi_f: null = all ones; ml: the lumped volumes as k_energy_pass<1, true> leaves them.  x may be y
__global__ __launch_bounds__(256) void k_forcing_scale(int64_t ld, const double* __restrict__ chi_f, const double* __restrict__ ml,
                                                       const uint8_t* __restrict__ bc_mask, const double* x, double* y) {
    for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < ld; d += (int64_t)gridDim.x * blockDim.x) {
        const double m = ml[d];
        double s = 0.0;
        if ((d & 3) != 3 && !bc_mask[d] && m > 0.0) s = (chi_f ? chi_f[d >> 2] : 1.0) / sqrt(m);
        const double xr = x[d], xi = x[ld + d];
        y[d] = s * xr;
        y[ld + d] = s * xi;
    }
}

// the start vector's mask: both parts 0 on pressure and constrained dofs
__global__ __launch_bounds__(256) void k_velocity_mask(int64_t ld, const uint8_t* __restrict__ bc_mask, double* x) {
    for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < ld; d += (int64_t)gridDim.x * blockDim.x)
        if ((d & 3) == 3 || bc_mask[d]) {
            x[d] = 0.0;
            x[ld + d] = 0.0;
        }
}

template <int NP, bool LUMPED>
void launch_energy_pass(sns_ctx* h, const double* chi, const double* x, double* y) {
    if (h->n == 0) return;
    const dim3 grid((unsigned)((4 * (int64_t)h->n + 255) / 256));
    hipLaunchKernelGGL((k_energy_pass<NP, LUMPED>), grid, dim3(256), 0, h->stream, h->n, h->nt_ptr, h->nt_idx, h->tets, h->pts, chi, x,
                       h->bc_mask, y);
}

}  // namespace

// y = D_chi M D_chi x queued on the handle's stream (parts = 2: planar complex x, y)
void launch_energy(sns_ctx* h, const double* chi, int parts, const double* x, double* y) {
    if (parts == 2) launch_energy_pass<2, false>(h, chi, x, y);
    else launch_energy_pass<1, false>(h, chi, x, y);
}

// handle, pointers and arguments were checked by the entry point
int energy_apply(sns_ctx* h, const double* chi, int parts, const double* x, double* y) {
    launch_energy(h, chi, parts, x, y);
    HIP_TRY(hipGetLastError());
    return sync_stream(h);
}

int lumped_volumes(sns_ctx* h, double* m) {
    launch_energy_pass<1, true>(h, nullptr, nullptr, m);
    HIP_TRY(hipGetLastError());
    return sync_stream(h);
}

// The Hermitian Krylov process on T = S B^T (J + i omega B)^-H Q (J + i omega B)^-1 B S (the header comment).  J is assembled here
// as the steady form (the entry point refused a time term) and set up.  V: (m + 1) planar complex columns of 2 * 4 n doubles,
// column 0 the start vector on entry (zeroed on pressure and constrained dofs and normalised here); H: (m + 1) x m complex, row
// major, (re, im) interleaved, T V_m = V_{m+1} H, zero beyond m_done.  *reason: 1 all m steps done, 2 breakdown (m_done columns,
// H[m_done][m_done - 1] = 0 and the column of V behind them zero; a start vector that the mask annihilates: m_done = 0), < 0 the
// KSP reason of an inner solve that did not converge (m_done = the steps completed).  On every return but SNS_E_HIP the handle
// holds J untransposed with its hierarchy set up and the steady form.
int resolvent_lanczos(sns_ctx* h, const double* w, double omega, int m, double breakdown_rel, const double* chi_f, const double* chi_q,
                      double* V, double* H, int* m_done, int* total_its, int* reason) {
    const int64_t ld = ld_of(h), n2 = 2 * ld;
    const int g = std::max(1, vec_grid(ld)), g2 = std::max(1, vec_grid(n2));
    constexpr int CS = 2 * (policy::STABILITY_M_MAX + 8);  // stride of one pass's coefficients: (re, im) per column, chunks of 8
    DevBuf<double> ml, a, b, co;                           // lumped volumes; the two work vectors; pass 1, pass 2, (w.w, .) before and after
    CfgmresWork cw;
    for (size_t t = 0; t < (size_t)2 * (m + 1) * m; ++t) H[t] = 0.0;
    *m_done = 0;
    *total_its = 0;
    *reason = 1;
    SNS_TRY(ml.alloc((size_t)ld));
    SNS_TRY(a.alloc((size_t)n2));
    SNS_TRY(b.alloc((size_t)n2));
    SNS_TRY(co.alloc((size_t)2 * CS + 4));
    SNS_TRY(timed_assemble(h, SNS_FORM_NS, w, nullptr, true));
    SNS_TRY(ensure_hierarchy(h));
    SNS_TRY(pc_setup(h));
    launch_energy_pass<1, true>(h, nullptr, nullptr, ml);
    bool flipped = false;
    // the operator flipped in place and set up for what it then is
    auto flip = [&]() -> int {
        SNS_TRY(transpose_operator(h));
        flipped = !flipped;
        return pc_setup(h);
    };
    // out = T v; false: an inner solve did not converge (*reason holds why; the operator is untransposed and set up again)
    auto apply_T = [&](const double* v, double* out, bool* ok) -> int {
        int its = 0, kr = 0;
        double rn = 0.0;
        hipLaunchKernelGGL(k_forcing_scale, dim3(g), dim3(256), 0, h->stream, ld, chi_f, ml, h->bc_mask, v, a);           // t = S v
        HIP_TRY(hipMemsetAsync(b, 0, (size_t)n2 * sizeof(double), h->stream));
        launch_mass_pair(h, false, w, 1.0, 0.0, a, b);                                                                    // b = B t
        HIP_TRY(hipMemsetAsync(a, 0, (size_t)n2 * sizeof(double), h->stream));
        SNS_TRY(cfgmres(h, w, 0.0, omega, false, b, a, &its, &kr, &rn, cw));                                              // (J + i omega B) q = b
        *total_its += its;
        *ok = kr > 0;
        if (!*ok) { *reason = kr; return SNS_OK; }
        launch_energy_pass<2, false>(h, chi_q, a, b);                                                                     // r = Q q
        SNS_TRY(flip());
        HIP_TRY(hipMemsetAsync(a, 0, (size_t)n2 * sizeof(double), h->stream));
        SNS_TRY(cfgmres(h, w, 0.0, -omega, true, b, a, &its, &kr, &rn, cw));                                              // (J + i omega B)^H y = r
        *total_its += its;
        SNS_TRY(flip());
        *ok = kr > 0;
        if (!*ok) { *reason = kr; return SNS_OK; }
        HIP_TRY(hipMemsetAsync(b, 0, (size_t)n2 * sizeof(double), h->stream));
        launch_mass_pair(h, true, w, 1.0, 0.0, a, b);                                                                     // B^T y
        hipLaunchKernelGGL(k_forcing_scale, dim3(g), dim3(256), 0, h->stream, ld, chi_f, ml, h->bc_mask, b, out);         // u = S B^T y
        return SNS_OK;
    };
    auto norm_sq = [&](const double* v, double* dst) {
        hipLaunchKernelGGL(k_dot2, dim3(g2), dim3(256), 0, h->stream, n2, v, v, h->partial);
        reduce_local(h, g2, 2, dst);
    };
    auto run = [&]() -> int {
        double hv[2 * CS + 4];
        // the start vector: pressure and constrained dofs zeroed, unit norm
        hipLaunchKernelGGL(k_velocity_mask, dim3(g), dim3(256), 0, h->stream, ld, h->bc_mask, V);
        norm_sq(V, co + 2 * CS);
        SNS_TRY(fetch(h, co + 2 * CS, 2, hv));
        const double n0 = std::sqrt(hv[0]);
        if (!(n0 > 0.0) || !std::isfinite(n0)) {
            *reason = 2;
            HIP_TRY(hipMemsetAsync(V, 0, (size_t)(m + 1) * n2 * sizeof(double), h->stream));
            return SNS_OK;
        }
        hipLaunchKernelGGL(k_scale_copy, dim3(g2), dim3(256), 0, h->stream, n2, 1.0 / n0, V, V);
        for (int j = 0; j < m; ++j) {
            double* wj = V + (size_t)(j + 1) * n2;
            bool ok = true;
            SNS_TRY(apply_T(V + (size_t)j * n2, wj, &ok));
            if (!ok) break;
            const int nv = j + 1;
            norm_sq(wj, co + 2 * CS);
            for (int pass = 0; pass < 2; ++pass)
                SNS_TRY(gram_schmidt_pass<true>(h, ld, g, nv, V, n2, wj, co + pass * CS, []() -> int { return SNS_OK; }));
            norm_sq(wj, co + 2 * CS + 2);
            SNS_TRY(fetch(h, co, 2 * CS + 4, hv));
            for (int k = 0; k < nv; ++k) {
                H[2 * ((size_t)k * m + j)] = hv[2 * k] + hv[CS + 2 * k];
                H[2 * ((size_t)k * m + j) + 1] = hv[2 * k + 1] + hv[CS + 2 * k + 1];
            }
            *m_done = nv;
            const double before = std::sqrt(hv[2 * CS]), after = std::sqrt(hv[2 * CS + 2]);
            if (!(after > breakdown_rel * before)) {       // (a NaN ends the process here too)
                *reason = 2;
                break;
            }
            H[2 * ((size_t)(j + 1) * m + j)] = after;
            hipLaunchKernelGGL(k_scale_copy, dim3(g2), dim3(256), 0, h->stream, n2, 1.0 / after, wj, wj);
        }
        // the columns of V the process never reached (after a breakdown or a failed solve: the one it was working on too)
        const int used = *reason == 2 ? *m_done : *m_done + 1;
        if (used < m + 1) HIP_TRY(hipMemsetAsync(V + (size_t)used * n2, 0, (size_t)(m + 1 - used) * n2 * sizeof(double), h->stream));
        HIP_TRY(hipGetLastError());
        return sync_stream(h);
    };
    int rc = run();
    if (rc != SNS_OK && rc != SNS_E_HIP && rc != SNS_E_COMM && flipped) {      // an error between the two flips of a step
        rc = give_back(h, rc, true, false);
        (void)pc_setup(h);
    }
    return rc;
}

}  // namespace sns
