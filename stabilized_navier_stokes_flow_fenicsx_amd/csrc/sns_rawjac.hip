// The raw-Jacobian pass (sns_raw_jacobian_apply) in a translation unit of its own: instantiating it beside the assembly kernels
// moved the register allocation of two of them (k_fused_diag under the viscosity law), so csrc/sns_kernels.hip stays as it was
// and this unit takes the block code from csrc/sns_element.h.
#include "sns_element.h"

namespace sns {

// The raw Jacobian applied matrix-free (sns_raw_jacobian_apply): y = J0(w) x or, with `transposed`, y = J0(w)^T x, J0 = dR_raw/dw
// without the Dirichlet rule -- no mask anywhere, every row written.  The lifting pass k_fused_lift is its [free, B] block applied to
// g - w_B; this is the whole operator, in either direction.  Lane l of row i walks the cells l, l + 4, ... of the node -> cell
// list (entry = 4 tet + local vertex a) and forms, for every b, one 4 x 4 block: (a, b) contracted along its columns, or (b, a)
// contracted along its rows.  The direction is a run-time flag, uniform over the launch.  Quad sums in a fixed order, lane c
// stores y[4 i + c]: no atomics, no scratch, bitwise reproducible.
template <int FORM, bool corrected, bool TT, bool VL, bool EV>
__global__ __launch_bounds__(256) void k_raw_jacobian_apply(int32_t n_rows, const int64_t* __restrict__ nt_ptr,
                                                            const int32_t* __restrict__ nt_idx, const int32_t* __restrict__ tets,
                                                            const double* __restrict__ pts, const double* __restrict__ w,
                                                            const double* __restrict__ x, double nu, int transposed,
                                                            double* __restrict__ y, TimeTerm tt, ViscosityLaw vl) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t node = gid >> 2;
    const int q = (int)(gid & 3);
    const bool live = node < n_rows;                       // (all 4 lanes of a group agree; nobody leaves before the moves)
    double R[4] = {0.0, 0.0, 0.0, 0.0};
    if (live) {
        const int64_t k1 = nt_ptr[node + 1];
        for (int64_t k = nt_ptr[node] + q; k < k1; k += 4) {
            const int32_t id = nt_idx[k];
            const int a = id & 3;
            const int64_t t = (int64_t)(id >> 2);
            const int4 tv = *reinterpret_cast<const int4*>(tets + 4 * t);
            const int32_t nd[4] = {tv.x, tv.y, tv.z, tv.w};
            double nuc = nu;
            if constexpr (EV) nuc = tt.nu_t[t];
            constexpr int NPE = (FORM == SNS_FORM_UGN_2D || FORM == SNS_FORM_STOKES_2D) ? 3 : 4;
#pragma unroll 1
            for (int b = 0; b < NPE; ++b) {
                const double2* xp = reinterpret_cast<const double2*>(x + 4 * (int64_t)nd[b]);
                const double2 x01 = xp[0], x23 = xp[1];
                double blk[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) blk[e] = 0.0;
                block_accumulate<FORM, corrected, TT, VL, EV>(tv, pts, w, nuc, 0.0, transposed ? b : a, transposed ? a : b, false, blk,
                                                              nullptr, tt, vl);
                if (transposed) {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        R[c] += blk[c] * x01.x + blk[4 + c] * x01.y + blk[8 + c] * x23.x + blk[12 + c] * x23.y;
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        R[c] += blk[4 * c] * x01.x + blk[4 * c + 1] * x01.y + blk[4 * c + 2] * x23.x + blk[4 * c + 3] * x23.y;
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        double v = R[c];
        v += quad_perm<0xB1>(v);
        v += quad_perm<0x4E>(v);
        R[c] = v;
    }
    if (!live) return;
    y[4 * node + q] = q == 0 ? R[0] : (q == 1 ? R[1] : (q == 2 ? R[2] : R[3]));
}
#define SNS_INST_RAWJAC(FM, C, T, V, E)                                                                                 \
    template __global__ void k_raw_jacobian_apply<FM, C, T, V, E>(int32_t, const int64_t*, const int32_t*, const int32_t*, const double*, \
                                                                  const double*, const double*, double, int, double*, TimeTerm,        \
                                                                  ViscosityLaw);
SNS_INST_RAWJAC(SNS_FORM_NS, false, false, false, false)
SNS_INST_RAWJAC(SNS_FORM_NS, true, false, false, false)
SNS_INST_RAWJAC(SNS_FORM_UGN_2D, false, false, false, false)
SNS_INST_RAWJAC(SNS_FORM_NS, false, true, false, false)
SNS_INST_RAWJAC(SNS_FORM_NS, true, true, false, false)
SNS_INST_RAWJAC(SNS_FORM_NS, false, false, true, false)
SNS_INST_RAWJAC(SNS_FORM_NS, true, false, true, false)
SNS_INST_RAWJAC(SNS_FORM_NS, false, true, false, true)
SNS_INST_RAWJAC(SNS_FORM_NS, true, true, false, true)

}  // namespace sns
