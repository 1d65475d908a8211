// Scalar transport on the flow mesh (sns_scalar_system, sns_scalar_solve; the reference has no counterpart): four species
// c_0..c_3 in the node-blocked layout [c0, c1, c2, c3] of the flow state, carried by the P1 velocity u of a state w,
//     R_k(c; v) = int (sigma c + u.grad c - s_k)(v + tau_k u.grad v) + kappa_k grad c . grad v dx = 0,
//     tau_k = (theta + u.G u + C_I kappa_k^2 G:G)^(-1/2),   G = K^T K, C_I = 36,
// with tau_k taken at each point of the 4-point degree-2 rule every integral uses (the flow form's metric and rule).  Inside a
// P1 tet the Laplacian of c vanishes, so the strong residual is sigma c + u.grad c - s.  The species do not couple: the operator
// is blockdiag(A_0..A_3), every 4 x 4 BSR block of the handle's pattern is diagonal -- 16 doubles stored for 4 used -- and the
// pattern, the SpMV family, the hierarchy, the Krylov methods and the in-place transpose serve it as they are.
//   k_scalar_system  owner-computes, one pass, no element scratch: 4 lanes per row, lane = species k.  A lane walks the slots of
//                    its row (rowptr / colind) and every slot's contributions (c_ptr / c_idx: tet, a, b) in their fixed order,
//                    recomputes the cell's geometry and its entry (a, b) -- the geometry is shared by the 4 lanes of a row and
//                    comes from L1/L2 -- and stores its 32-byte row of the block: its diagonal entry and three explicit zeros, so
//                    the 4 lanes of a row write the 128 bytes of a block together and vals is overwritten in full.  The row's
//                    source integral (taken on the diagonal slot, whose contributions are the row's cells, once each) and its
//                    lifting sum stay in the lane; the right-hand side is stored at the end.
// Dirichlet data as the flow operator treats its own (oracle/assemble.py): rows and columns zeroed, diagonal one,
// b_i -= sum_{j in B} A0_ij g_j, b_B = g.  No atomics; the summation order is fixed, so results are bitwise reproducible.
#include "sns_ctx.h"

namespace sns {
namespace {

constexpr double SC_QA = 0.1381966011250105, SC_QB = 0.5854101966249685, SC_CI = 36.0;

struct ScalarParams {
    double kappa[4];
    double sigma, theta;
};

// THE element math of the form, used by every kernel of this file: entry (a, b) of species-k's element matrix of cell t,
//     A = sum_q w_q (sigma phi_b + u_q.g_b)(phi_a + tau_q u_q.g_a) + kappa |t| g_a.g_b,
// and, where want_src, the share of the nodal P1 source s (4 per node, component k) in row a,
//     S = sum_q w_q s(x_q) (phi_a + tau_q u_q.g_a).
// K[m][j] = d_j phi_{m+1} (phi_0 = 1 - sum), g_a = grad phi_a, w_q = |det J| / 24: cells of either orientation count with |det J|.
__device__ __forceinline__ void scalar_entry(const int32_t* __restrict__ tets, const double* __restrict__ pts,
                                             const double* __restrict__ w, const double* __restrict__ src, int k, int64_t t,
                                             int a, int b, double kappa, double sigma, double theta, bool want_src, double& A,
                                             double& S) {
    const int4 tv = *reinterpret_cast<const int4*>(tets + 4 * t);
    const int32_t nd[4] = {tv.x, tv.y, tv.z, tv.w};
    double X[4][3], U[4][3];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const double* pp = pts + 3 * (int64_t)nd[m];
        X[m][0] = pp[0]; X[m][1] = pp[1]; X[m][2] = pp[2];
        const double2 u01 = *reinterpret_cast<const double2*>(w + 4 * (int64_t)nd[m]);
        U[m][0] = u01.x; U[m][1] = u01.y; U[m][2] = w[4 * (int64_t)nd[m] + 2];
    }
    double J[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        J[i][0] = X[1][i] - X[0][i];
        J[i][1] = X[2][i] - X[0][i];
        J[i][2] = X[3][i] - X[0][i];
    }
    const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
    const double c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
    const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
    const double id = 1.0 / det;
    double K[3][3];
    K[0][0] = c00 * id; K[1][0] = c01 * id; K[2][0] = c02 * id;
    K[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id;
    K[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id;
    K[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * id;
    K[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * id;
    K[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id;
    K[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * id;
    const double wq = fabs(det) * (1.0 / 24.0);
    // G:G of G = K^T K (symmetric: the off-diagonal entries count twice)
    double GG = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) {
            const double g = K[0][i] * K[0][j] + K[1][i] * K[1][j] + K[2][i] * K[2][j];
            GG += (i == j ? 1.0 : 2.0) * g * g;
        }
    const double diff = SC_CI * kappa * kappa * GG + theta;
    // g_a . g_b by the rows of K (g_0 = -(row sum))
    double ga[3], gb[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double g0 = -(K[0][j] + K[1][j] + K[2][j]);
        ga[j] = a == 0 ? g0 : (a == 1 ? K[0][j] : (a == 2 ? K[1][j] : K[2][j]));
        gb[j] = b == 0 ? g0 : (b == 1 ? K[0][j] : (b == 2 ? K[1][j] : K[2][j]));
    }
    double usum[3], ssum = 0.0, sn[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 3; ++j) usum[j] = SC_QA * (((U[0][j] + U[1][j]) + U[2][j]) + U[3][j]);
    if (want_src) {
#pragma unroll
        for (int m = 0; m < 4; ++m) sn[m] = src[4 * (int64_t)nd[m] + k];
        ssum = SC_QA * (((sn[0] + sn[1]) + sn[2]) + sn[3]);
    }
    double acc = 0.0, sacc = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double u[3], Ku[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) u[j] = usum[j] + (SC_QB - SC_QA) * U[q][j];
#pragma unroll
        for (int m = 0; m < 3; ++m) Ku[m] = K[m][0] * u[0] + K[m][1] * u[1] + K[m][2] * u[2];
        const double uGu = Ku[0] * Ku[0] + Ku[1] * Ku[1] + Ku[2] * Ku[2];          // u.G u = |K u|^2
        const double tau = 1.0 / sqrt(uGu + diff);
        const double uga = u[0] * ga[0] + u[1] * ga[1] + u[2] * ga[2];
        const double ugb = u[0] * gb[0] + u[1] * gb[1] + u[2] * gb[2];
        const double pa = q == a ? SC_QB : SC_QA, pb = q == b ? SC_QB : SC_QA;
        const double test = pa + tau * uga;
        acc += (sigma * pb + ugb) * test;
        if (want_src) sacc += (ssum + (SC_QB - SC_QA) * sn[q]) * test;
    }
    A = wq * acc + kappa * (4.0 * wq) * (ga[0] * gb[0] + ga[1] * gb[1] + ga[2] * gb[2]);
    S = wq * sacc;
}

// lane (i, k): row i of species k.  vals[16 s + 4 k + 0..3] = e_k * (entry of slot s); rhs[4 i + k].
__global__ __launch_bounds__(256) void k_scalar_system(int32_t n_rows, const int32_t* __restrict__ rowptr,
                                                       const int32_t* __restrict__ colind, const int64_t* __restrict__ c_ptr,
                                                       const int32_t* __restrict__ c_idx, const int32_t* __restrict__ tets,
                                                       const double* __restrict__ pts, const double* __restrict__ w,
                                                       ScalarParams P, const double* __restrict__ src,
                                                       const uint8_t* __restrict__ cmask, const double* __restrict__ cval,
                                                       double* __restrict__ vals, double* __restrict__ rhs) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = gid >> 2;
    const int k = (int)(gid & 3);
    if (i >= n_rows) return;                               // (no cross-lane traffic in this kernel)
    const double kappa = k == 0 ? P.kappa[0] : (k == 1 ? P.kappa[1] : (k == 2 ? P.kappa[2] : P.kappa[3]));
    const bool mr = cmask[4 * i + k] != 0;
    double lift = 0.0, srow = 0.0;
    const int32_t s1 = rowptr[i + 1];
    for (int32_t s = rowptr[i]; s < s1; ++s) {
        const int32_t j = colind[s];
        const bool on_diag = j == (int32_t)i;
        const bool want_src = on_diag && src != nullptr;
        double acc = 0.0;
        const int64_t q1 = c_ptr[s + 1];
        for (int64_t q = c_ptr[s]; q < q1; ++q) {
            const uint32_t id = (uint32_t)c_idx[q];        // tet*16 + a*4 + b, unsigned (up to 268 M tets)
            double A, S;
            scalar_entry(tets, pts, w, src, k, (int64_t)(id >> 4), (int)((id >> 2) & 3), (int)(id & 3), kappa, P.sigma, P.theta,
                         want_src, A, S);
            acc += A;
            srow += S;
        }
        const bool mc = cmask[4 * (int64_t)j + k] != 0;
        if (mc && !mr) lift += acc * cval[4 * (int64_t)j + k];
        const double v = (mr || mc) ? (on_diag ? 1.0 : 0.0) : acc;
        double2* o = reinterpret_cast<double2*>(vals + 16 * (int64_t)s + 4 * k);
        o[0] = make_double2(k == 0 ? v : 0.0, k == 1 ? v : 0.0);
        o[1] = make_double2(k == 2 ? v : 0.0, k == 3 ? v : 0.0);
    }
    rhs[4 * i + k] = mr ? cval[4 * i + k] : srow - lift;
}

// free[i] = the dof takes part in the hierarchy's transfers = it is not a Dirichlet dof of the operator in the handle
__global__ __launch_bounds__(256) void k_free_from_mask(int64_t ndof, const uint8_t* __restrict__ mask, uint8_t* __restrict__ free_mask) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ndof; i += (int64_t)gridDim.x * blockDim.x)
        free_mask[i] = mask[i] ? 0 : 1;
}

}  // namespace

// The fine level's free mask follows the operator in the handle: the hierarchy's transfer operators leave out the Dirichlet dofs
// of THAT operator -- the scalars' while the scalar operator is the handle's matrix, the flow's again from the next flow assembly
// on (csrc/sns_assemble.hip).  The mask and the per-aggregate counts derived from it (levels[0].empty_c, once the hierarchy exists) are
// rewritten in place; everything else that depends on them is rebuilt by the set-up every assembly makes stale.  Handles
// without a communicator only (the ghost part of a partitioned handle's mask is not the complement of its Dirichlet mask).
int fine_free_mask(sns_ctx* h, const uint8_t* dirichlet_mask) {
    Level& L = h->levels[0];
    const int64_t ld = ld_of(h);
    hipLaunchKernelGGL(k_free_from_mask, dim3(vec_grid(ld)), dim3(256), 0, h->stream, ld, dirichlet_mask, L.free_mask.get());
    if (h->levels.size() > 1 && h->levels[0].empty_c) {
        const int32_t nc = h->levels[1].n_owned;
        if (nc > 0)
            hipLaunchKernelGGL(k_empty_coarse, dim3((unsigned)((4 * (int64_t)nc + 255) / 256)), dim3(256), 0, h->stream, nc, L.m_ptr,
                               L.m_idx, L.free_mask, L.empty_c);
    }
    HIP_TRY(hipGetLastError());
    return SNS_OK;
}

// handle, pointers, dimension, communicator and the coefficients were checked by the entry points
int scalar_system(sns_ctx* h, const double* w, const double kappa[4], double sigma, double theta, const double* src,
                  const uint8_t* cmask, const double* cval, double* rhs) {
    const size_t ld = (size_t)ld_of(h);
    // the handle's copy of the scalars' Dirichlet mask: sns_adjoint_solve hands back lam_B = g_B by the mask of the operator it
    // transposed, which is this one while the scalar operator is the handle's matrix
    if (!h->sc_mask) SNS_TRY(h->sc_mask.alloc(ld));
    HIP_TRY(hipMemcpyAsync(h->sc_mask, cmask, ld, hipMemcpyDeviceToDevice, h->stream));
    SNS_TRY(fine_free_mask(h, cmask));
    ScalarParams P;
    for (int k = 0; k < 4; ++k) P.kappa[k] = kappa[k];
    P.sigma = sigma;
    P.theta = theta;
    Level& L = h->levels[0];
    const unsigned grid = (unsigned)((4 * (int64_t)h->n + 255) / 256);
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    hipLaunchKernelGGL(k_scalar_system, dim3(grid), dim3(256), 0, h->stream, h->n, L.rowptr, L.colind, h->c_ptr, h->c_idx, h->tets,
                       h->pts, w, P, src, cmask, cval, L.vals, rhs);
    SNS_TRY(boundary_scalar(h, cmask, cval, L.vals, rhs));     // the Robin terms (csrc/sns_boundary.hip; nothing set: nothing launched)
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    const hipError_t e = hipGetLastError();
    const double par[6] = {kappa[0], kappa[1], kappa[2], kappa[3], sigma, theta};
    matrix_changed(h, SNS_FORM_SCALAR, par);               // (another set of parameters is another operator)
    const int rc = sync_stream(h);                         // (the caller may free its arrays)
    HIP_TRY(e);
    SNS_TRY(rc);
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    h->tm.assemble_ms += ms;
    return SNS_OK;
}

}  // namespace sns
