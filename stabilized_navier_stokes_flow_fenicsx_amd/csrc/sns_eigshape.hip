// The eigenvalue shape pass of the 3-D NS form (sns_jacobian_shape_gradient; the reference has no counterpart): for real dof
// vectors x, z and real scalars c_J, c_B,
//     gX[k][j] = d/dX[k][j] [ z~^T ( c_J J0(w; X) + c_B B(w; X) ) x~ ]        (n_nodes x 3),
// J0 = dR_raw/dw the steady Jacobian of the handle's form (form variant, corrected_convection, nu constant or the per-cell nu_t
// held fixed), B the Petrov-Galerkin mass operator of sns_mass_apply, x~ and z~ the vectors with every constrained entry (all
// four mask bytes of a node) read as 0; w, x~, z~ and the viscosity are held fixed.  It is the explicit part of the shape
// sensitivity of an eigenvalue (solver.eigenvalue_shape_sensitivity), beside sns_jacobian_state_gradient, which differentiates
// the same contraction in w.  Per cell the Hessian pass's scalar phi_e is differentiated in the 12 vertex coordinates by hand,
// tangent along x then reverse mode through K, G and |det J| (csrc/sns_eigshape_cell.h, which tests/eigshape_cell_main.cpp
// compiles on the host):
//   k_eigshape_tet<corrected>  one lane per tet, as k_shape_tet and k_state_gradient; 16 values per tet go to the handle's
//                              element scratch in the shape gradient's layout, Ge[16 t + 4 a + j], slot 3 zero
//   k_gather_shape             (csrc/sns_shape.hip) node <- sum over its cells in the fixed order of nt_ptr / nt_idx
// No atomics, a fixed order: bitwise reproducible.  Nothing of the handle besides the element scratch is written.
// Not built: the mesh derivative of the facet terms, a body force, a viscosity law or a time term inside the contraction, 2-D
// and partitioned handles (the request rows of the Hessian pass refuse them).
#include "sns_ctx.h"
#include "sns_eigshape_cell.h"

namespace sns {
namespace {

template <bool corrected>
__global__ __launch_bounds__(256) void k_eigshape_tet(int64_t n_tets, const int32_t* __restrict__ tets, const double* __restrict__ pts,
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
    double o[4][3];
    // a viscosity field switches the viscous term to the stress-divergence form (2 nu_t eps(u), grad v)
    eigshape_cell<corrected>(T.g, T.G, T.trG, T.GG, fabs(T.det) * (1.0 / 24.0), W, Xd, Z, f, nu_t != nullptr, cj, cb, o);
    double2* out = reinterpret_cast<double2*>(Ge + 16 * t);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        out[2 * a] = make_double2(o[a][0], o[a][1]);
        out[2 * a + 1] = make_double2(o[a][2], 0.0);
    }
}

}  // namespace

// handle, pointers, coefficients and the form state were checked by the entry point
int jacobian_shape_gradient(sns_ctx* h, const double* w, const double* x, const double* z, double c_jac, double c_mass, double* gX) {
    if (h->E == 0 || h->n == 0) {
        if (h->n > 0) HIP_TRY(hipMemsetAsync(gX, 0, (size_t)3 * h->n * sizeof(double), h->stream));
        return sync_stream(h);
    }
    if (!h->Fe) SNS_TRY(h->Fe.alloc((size_t)h->E * 16));
    const FormState& S = h->form;
    const double nu = 1.0 / h->opt.reynolds;
    const double* nu_t = S.ev_on ? S.ev_nu.get() : nullptr;
    const unsigned gc = (unsigned)((h->E + 255) / 256);
    dispatch<1, 0>(h->opt.corrected_convection != 0, [&](auto C) {
        hipLaunchKernelGGL((k_eigshape_tet<C() != 0>), dim3(gc), dim3(256), 0, h->stream, h->E, h->tets, h->pts, w, x, z, h->bc_mask,
                           nu, nu_t, S.fv, c_jac, c_mass, h->Fe);
    });
    const int64_t nth = 4 * (int64_t)h->n;
    hipLaunchKernelGGL(k_gather_shape, dim3((unsigned)((nth + 255) / 256)), dim3(256), 0, h->stream, h->n, h->nt_ptr, h->nt_idx,
                       h->Fe, gX);
    HIP_TRY(hipGetLastError());
    return sync_stream(h);
}

}  // namespace sns
