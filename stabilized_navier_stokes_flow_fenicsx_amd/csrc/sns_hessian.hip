// The Hessian pass of the 3-D NS form (sns_jacobian_state_gradient; the reference has no counterpart): for real dof vectors x, z
// and real scalars c_J, c_B,
//     g_k = sum_ij z~_i x~_j d( c_J J_ij(w) + c_B B_ij(w) ) / d w_k     (k unconstrained; 0 on constrained dofs),
// J = dR_raw/dw the steady Jacobian of the handle's form (form variant, corrected_convection, nu constant or the per-cell
// nu_t held fixed), B the Petrov-Galerkin mass operator of sns_mass_apply, x~ and z~ the vectors with every constrained entry
// (all four mask bytes of a node) read as 0.  It is what the sensitivity of an eigenvalue to the base flow and to a steady
// forcing contract the left and the right mode with (solver.eigenvalue_base_flow_sensitivity, eigenvalue_forcing_sensitivity).
// Per cell the scalar phi_e = c_J d/d eps [z_e . R_e(W + eps x_e)] + c_B z_e . (R_e(W; d = x_u) - R_e(W)) is differentiated by
// hand, tangent then reverse mode (csrc/sns_hessian_cell.h, which tests/hessian_cell_main.cpp compiles on the host):
//   k_state_gradient<corrected>  one lane per tet, as k_shape_tet: the adjoints of u(q), grad u and grad p serve all four
//                                vertices, so a cell is visited once, not once per incident row; 16 values per tet go to the
//                                handle's element scratch in the residual's layout, Ge[16 t + 4 a + c]
//   k_gather_state_gradient      row (i, c) <- sum over the cells of node i of Ge[16 t + 4 a + c] in the fixed order of
//                                nt_ptr / nt_idx (8 ids, then their 8 entries, as k_gather_shape), constrained rows stored as 0
// No atomics, a fixed order: bitwise reproducible.  Nothing of the handle besides the element scratch is written.
// Not built: the second contraction a body force adds (J depends on f through dM/dw(w, -f)), the Hessian of the backflow term,
// a viscosity law, a time term, 2-D and partitioned handles (policy::check_state_gradient_request refuses them).
#include "sns_ctx.h"
#include "sns_hessian_cell.h"

namespace sns {
namespace {

template <bool corrected>
__global__ __launch_bounds__(256) void k_state_gradient(int64_t n_tets, const int32_t* __restrict__ tets, const double* __restrict__ pts,
                                                        const double* __restrict__ w, const double* __restrict__ x,
                                                        const double* __restrict__ z, const uint8_t* __restrict__ bc_mask, double nu,
                                                        const double* __restrict__ nu_t, FormVariant fv, double cj, double cb,
                                                        double* __restrict__ Ge) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tets) return;
    const int4 tv = *reinterpret_cast<const int4*>(tets + 4 * t);
    const int32_t nd[4] = {tv.x, tv.y, tv.z, tv.w};
    double X[4][3], W[4][4], Xd[4][4], Z[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int64_t o = 4 * (int64_t)nd[a];
        const double* pp = pts + 3 * (int64_t)nd[a];
        X[a][0] = pp[0]; X[a][1] = pp[1]; X[a][2] = pp[2];
        const double2 w01 = *reinterpret_cast<const double2*>(w + o), w23 = *reinterpret_cast<const double2*>(w + o + 2);
        W[a][0] = w01.x; W[a][1] = w01.y; W[a][2] = w23.x; W[a][3] = w23.y;
        const double2 x01 = *reinterpret_cast<const double2*>(x + o), x23 = *reinterpret_cast<const double2*>(x + o + 2);
        const double2 z01 = *reinterpret_cast<const double2*>(z + o), z23 = *reinterpret_cast<const double2*>(z + o + 2);
        const uint32_t mk = *reinterpret_cast<const uint32_t*>(bc_mask + o);      // the node's 4 mask bytes, the pressure's too
        const bool m0 = mk & 0xFFu, m1 = mk & 0xFF00u, m2 = mk & 0xFF0000u, m3 = mk & 0xFF000000u;
        Xd[a][0] = m0 ? 0.0 : x01.x; Xd[a][1] = m1 ? 0.0 : x01.y; Xd[a][2] = m2 ? 0.0 : x23.x; Xd[a][3] = m3 ? 0.0 : x23.y;
        Z[a][0] = m0 ? 0.0 : z01.x; Z[a][1] = m1 ? 0.0 : z01.y; Z[a][2] = m2 ? 0.0 : z23.x; Z[a][3] = m3 ? 0.0 : z23.y;
    }
    TetMetric T;
    tet_metric(X, T);
    const HessianForm f{fv.ci, fv.lsic, fv.pspg, fv.qa, fv.qb, nu_t ? nu_t[t] : nu};
    double o[4][4];
    state_gradient_cell<corrected>(T.g, T.G, T.trG, T.GG, fabs(T.det) * (1.0 / 24.0), W, Xd, Z, f, cj, cb, o);
    double2* out = reinterpret_cast<double2*>(Ge + 16 * t);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        out[2 * a] = make_double2(o[a][0], o[a][1]);
        out[2 * a + 1] = make_double2(o[a][2], o[a][3]);
    }
}

// lane (i, c): g[4 i + c] <- sum over the cells of node i of Ge[16 t + 4 a + c], in list order; constrained rows 0
__global__ __launch_bounds__(256) void k_gather_state_gradient(int32_t n_rows, const int64_t* __restrict__ nt_ptr,
                                                               const int32_t* __restrict__ nt_idx, const uint8_t* __restrict__ bc_mask,
                                                               const double* __restrict__ Ge, double* __restrict__ g) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = gid >> 2;
    const int c = (int)(gid & 3);
    if (i >= n_rows) return;
    double s = 0.0;
    const int64_t k1 = nt_ptr[i + 1];
    int64_t k = nt_ptr[i];
    for (; k + 7 < k1; k += 8) {
        int32_t id[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) id[q] = nt_idx[k + q];
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = Ge[(int64_t)id[q] * 4 + c];
#pragma unroll
        for (int q = 0; q < 8; ++q) s += v[q];
    }
    if (k < k1) {
        int32_t id[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) id[q] = (k + q < k1) ? nt_idx[k + q] : -1;
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = id[q] >= 0 ? Ge[(int64_t)id[q] * 4 + c] : 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (id[q] >= 0) s += v[q];
    }
    g[4 * i + c] = bc_mask[4 * i + c] ? 0.0 : s;
}

}  // namespace

// handle, pointers, coefficients and the form state were checked by the entry point
int jacobian_state_gradient(sns_ctx* h, const double* w, const double* x, const double* z, double c_jac, double c_mass, double* g) {
    if (h->E == 0 || h->n == 0) {
        if (h->n > 0) HIP_TRY(hipMemsetAsync(g, 0, (size_t)4 * h->n * sizeof(double), h->stream));
        return sync_stream(h);
    }
    if (!h->Fe) SNS_TRY(h->Fe.alloc((size_t)h->E * 16));
    const FormState& S = h->form;
    const double nu = 1.0 / h->opt.reynolds;
    const double* nu_t = S.ev_on ? S.ev_nu.get() : nullptr;
    const unsigned gc = (unsigned)((h->E + 255) / 256);
    dispatch<1, 0>(h->opt.corrected_convection != 0, [&](auto C) {
        hipLaunchKernelGGL((k_state_gradient<C() != 0>), dim3(gc), dim3(256), 0, h->stream, h->E, h->tets, h->pts, w, x, z, h->bc_mask,
                           nu, nu_t, S.fv, c_jac, c_mass, h->Fe);
    });
    const int64_t nth = 4 * (int64_t)h->n;
    hipLaunchKernelGGL(k_gather_state_gradient, dim3((unsigned)((nth + 255) / 256)), dim3(256), 0, h->stream, h->n, h->nt_ptr, h->nt_idx,
                       h->bc_mask, h->Fe, g);
    HIP_TRY(hipGetLastError());
    return sync_stream(h);
}

}  // namespace sns
