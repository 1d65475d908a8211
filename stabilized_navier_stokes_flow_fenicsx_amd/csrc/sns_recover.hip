// Gradient recovery of the P1 state (sns_recover_gradient, sns_error_indicator; the reference has no counterpart):
//     G_i[c][j] = ( sum_{t in cells(i)} |t| d_j w_c|_t ) / ( sum_{t in cells(i)} |t| ),   |t| = |det J| / d!
// the lumped-mass L2 projection of the piecewise-constant gradient onto P1, c in (u_x, u_y, u_z, p), and from its velocity
// rows the nodal vorticity, Q, shear rate and divergence, and per cell the Zienkiewicz-Zhu indicator
//     eta_t^2 = int_t |G_h(u) - grad u_h|_F^2 = |t| / ((d+1)(d+2)) ( sum_a |e_a|_F^2 + |sum_a e_a|_F^2 ),  e_a = G_{node a} - grad u_h|_t
// (exact: the integrand is the square of a P1 function).
//   k_recover<DIM>  owner-computes, one pass: 4 lanes per node, lane = component c, walk the node's cells in the fixed order
//                   of nt_ptr / nt_idx (8 ids at a time, the tail masked).  Every lane recomputes K = J^-1 and |det J| of the
//                   cell from pts -- the geometry is shared by the 4 lanes of a node and comes from L1/L2 -- and forms
//                   d_j w_c = sum_m (w_c[m+1] - w_c[0]) K[m][j].  The derived fields are combined inside the 4-lane group with
//                   cross-lane moves.  One kernel serves every combination of outputs (G and D are tested at run time), so
//                   D does not depend, bit for bit, on whether G is stored.
//   k_zz<DIM>       one lane per cell: its own gradient again, the 4 (3) nodal G rows of u, eta_t^2 and |t| |grad u_h|_F^2
// No atomics, no element scratch, nothing of the handle is written; the result is bitwise reproducible.
#include "sns_ctx.h"

namespace sns {

// vertices nd[0..DIM], K[m][j] = d_j phi_{m+1} (phi_0 = 1 - sum) and |t| of cell t; 2-D: K[.][2] = K[2][.] = 0
template <int DIM>
__device__ __forceinline__ void cell_geometry(const int32_t* __restrict__ tets, const double* __restrict__ pts, int64_t t,
                                              int32_t nd[4], double K[3][3], double& vol) {
    if constexpr (DIM == 3) {
        const int4 tv = *reinterpret_cast<const int4*>(tets + 4 * t);
        nd[0] = tv.x; nd[1] = tv.y; nd[2] = tv.z; nd[3] = tv.w;
        double X[4][3];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double* pp = pts + 3 * (int64_t)nd[a];
            X[a][0] = pp[0]; X[a][1] = pp[1]; X[a][2] = pp[2];
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
        K[0][0] = c00 * id; K[1][0] = c01 * id; K[2][0] = c02 * id;
        K[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id;
        K[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id;
        K[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * id;
        K[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * id;
        K[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id;
        K[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * id;
        vol = fabs(det) * (1.0 / 6.0);
    } else {
        nd[0] = tets[4 * t]; nd[1] = tets[4 * t + 1]; nd[2] = tets[4 * t + 2]; nd[3] = nd[0];
        double X[3][2];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double* pp = pts + 3 * (int64_t)nd[a];
            X[a][0] = pp[0]; X[a][1] = pp[1];
        }
        const double J00 = X[1][0] - X[0][0], J01 = X[2][0] - X[0][0];
        const double J10 = X[1][1] - X[0][1], J11 = X[2][1] - X[0][1];
        const double det = J00 * J11 - J01 * J10;
        const double id = 1.0 / det;
        K[0][0] = J11 * id;  K[0][1] = -J01 * id; K[0][2] = 0.0;
        K[1][0] = -J10 * id; K[1][1] = J00 * id;  K[1][2] = 0.0;
        K[2][0] = 0.0; K[2][1] = 0.0; K[2][2] = 0.0;
        vol = fabs(det) * 0.5;
    }
}

// the cell's constant gradient of dof component c: g[j] = sum_m (w_c[m+1] - w_c[0]) K[m][j]
template <int DIM>
__device__ __forceinline__ void cell_gradient(const double* __restrict__ w, const int32_t nd[4], const double K[3][3], int c,
                                              double g[3]) {
    const double w0 = w[4 * (int64_t)nd[0] + c];
    double dw[DIM];
#pragma unroll
    for (int m = 0; m < DIM; ++m) dw[m] = w[4 * (int64_t)nd[m + 1] + c] - w0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < DIM; ++m) s += dw[m] * K[m][j];
        g[j] = j < DIM ? s : 0.0;
    }
}

// lane (i, c): row c of G_i; then, inside the 4-lane group, the derived fields D[6 i + k] (lane c < 3 stores k = c and
// k = 3 + c).  G and / or D may be null.  The slots past the end of a list repeat the list's first cell, so that every load
// of the 8 can be issued before the first use, and are left out of the sums.
template <int DIM>
__global__ __launch_bounds__(256) void k_recover(int32_t n, const int64_t* __restrict__ nt_ptr,
                                                 const int32_t* __restrict__ nt_idx, const int32_t* __restrict__ tets,
                                                 const double* __restrict__ pts, const double* __restrict__ w,
                                                 double* __restrict__ G, double* __restrict__ D) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = gid >> 2;
    const int c = (int)(gid & 3);
    const bool live = i < n;                               // (all 4 lanes of a group agree; nobody leaves before the moves)
    int64_t k = live ? nt_ptr[i] : 0;
    const int64_t k1 = live ? nt_ptr[i + 1] : 0;
    double sw = 0.0, s[3] = {0.0, 0.0, 0.0};
    for (; k < k1; k += 8) {
        const int32_t first = nt_idx[k];
        int32_t id[8];
        bool on[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            on[q] = k + q < k1;
            id[q] = on[q] ? nt_idx[k + q] : first;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            int32_t nd[4];
            double K[3][3], vol, g[3];
            cell_geometry<DIM>(tets, pts, (int64_t)(id[q] >> 2), nd, K, vol);
            cell_gradient<DIM>(w, nd, K, c, g);
            if (on[q]) {
                sw += vol;
                s[0] += vol * g[0]; s[1] += vol * g[1]; s[2] += vol * g[2];
            }
        }
    }
    double r[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) r[j] = sw > 0.0 ? s[j] / sw : 0.0;
    if (live && G) {
        double* o = G + 12 * i + 3 * c;
        o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
    }
    if (!D) return;                                        // (uniform over the grid)
    double U[3][3];                                        // U[m][j] = d_j u_m
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int j = 0; j < 3; ++j) U[m][j] = __shfl(r[j], m, 4);
    const double om[3] = {U[2][1] - U[1][2], U[0][2] - U[2][0], U[1][0] - U[0][1]};
    const double s01 = 0.5 * (U[0][1] + U[1][0]), s02 = 0.5 * (U[0][2] + U[2][0]), s12 = 0.5 * (U[1][2] + U[2][1]);
    const double SS = U[0][0] * U[0][0] + U[1][1] * U[1][1] + U[2][2] * U[2][2] + 2.0 * (s01 * s01 + s02 * s02 + s12 * s12);
    const double OO = 0.5 * (om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);      // |Omega|_F^2 = |omega|^2 / 2
    const double hi[3] = {0.5 * (OO - SS), sqrt(2.0 * SS), U[0][0] + U[1][1] + U[2][2]};
    if (live && c < 3) {
        D[6 * i + c] = c == 0 ? om[0] : (c == 1 ? om[1] : om[2]);
        D[6 * i + 3 + c] = c == 0 ? hi[0] : (c == 1 ? hi[1] : hi[2]);
    }
}

// eta2[t] and, where asked for, gn2[t] = |t| |grad u_h|_F^2; G: the recovered gradient, 12 doubles per node
template <int DIM>
__global__ __launch_bounds__(256) void k_zz(int64_t n_cells, const int32_t* __restrict__ tets, const double* __restrict__ pts,
                                            const double* __restrict__ w, const double* __restrict__ G,
                                            double* __restrict__ eta2, double* __restrict__ gn2) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_cells) return;
    int32_t nd[4];
    double K[3][3], vol, gu[3][3];
    cell_geometry<DIM>(tets, pts, t, nd, K, vol);
    double gg = 0.0;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        cell_gradient<DIM>(w, nd, K, m, gu[m]);
        gg += gu[m][0] * gu[m][0] + gu[m][1] * gu[m][1] + gu[m][2] * gu[m][2];
    }
    double se[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ee = 0.0;
#pragma unroll
    for (int a = 0; a <= DIM; ++a) {
        const double* ga = G + 12 * (int64_t)nd[a];
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            const double e = ga[q] - gu[q / 3][q % 3];
            se[q] += e;
            ee += e * e;
        }
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) ee += se[q] * se[q];
    eta2[t] = vol * (1.0 / ((DIM + 1) * (DIM + 2))) * ee;
    if (gn2) gn2[t] = vol * gg;
}

static void launch_recover(sns_ctx* h, const double* w, double* G, double* D) {
    const int64_t nth = 4 * (int64_t)h->n;
    const dim3 grid((unsigned)((nth + 255) / 256));
    if (h->dim == 2)
        hipLaunchKernelGGL(k_recover<2>, grid, dim3(256), 0, h->stream, h->n, h->nt_ptr, h->nt_idx, h->tets, h->pts, w, G, D);
    else
        hipLaunchKernelGGL(k_recover<3>, grid, dim3(256), 0, h->stream, h->n, h->nt_ptr, h->nt_idx, h->tets, h->pts, w, G, D);
}

// pointers and the communicator were checked by the entry points
int recover_gradient(sns_ctx* h, const double* w, double* G, double* D) {
    if (h->n == 0) return sync_stream(h);
    launch_recover(h, w, G, D);
    HIP_TRY(hipGetLastError());
    return sync_stream(h);
}

int error_indicator(sns_ctx* h, const double* w, const double* G, double* eta2, double* gnorm2) {
    if (h->E == 0 || h->n == 0) return sync_stream(h);
    DevBuf<double> tmp;                                    // freed on every way out, after the stream has drained
    if (!G) {
        SNS_TRY(tmp.alloc((size_t)12 * h->n));
        launch_recover(h, w, tmp, nullptr);
        G = tmp;
    }
    const dim3 grid((unsigned)((h->E + 255) / 256));
    if (h->dim == 2)
        hipLaunchKernelGGL(k_zz<2>, grid, dim3(256), 0, h->stream, h->E, h->tets, h->pts, w, G, eta2, gnorm2);
    else
        hipLaunchKernelGGL(k_zz<3>, grid, dim3(256), 0, h->stream, h->E, h->tets, h->pts, w, G, eta2, gnorm2);
    const hipError_t e = hipGetLastError();
    const int rc = sync_stream(h);                         // (before tmp goes, also after a failed launch)
    HIP_TRY(e);
    return rc;
}

}  // namespace sns
