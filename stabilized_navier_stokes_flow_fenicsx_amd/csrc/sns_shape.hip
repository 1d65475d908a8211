// Shape gradient of the raw NS residual contracted with a dof vector (sns_residual_shape_gradient):
//     gX[k][j] = sum_i lam[i] * d R_raw(w; X)[i] / d X[k][j]
// With the P1 field (v, q) = lam restricted to a cell, the cell's contribution is ONE scalar
//     L_e(X_e) = |det J| / n! * sum_q [ (u.grad)u . v + nu grad u : grad v - p div v + q div u + tau res_M . m + c_LSIC div u div v ]
// (m = the SUPG/PSPG test direction), so the kernels never form a 16 x 12 matrix: they evaluate L_e like the residual
// kernels evaluate the residual and run reverse mode by hand through everything that carries geometry,
//     grad phi_a = rows of K = J^-1 (g_0 = -sum),  G = K^T K,  |det J|,  and in 2-D h^2 = the longest edge squared:
//   * the adjoints of grad u, grad p, grad v, grad q and of G are accumulated over the quadrature points,
//   * folded into Kb = dL/dK,  then  dK = -K dJ K  and  d|det| = |det| tr(K dJ)  give  Jb = -K^T Kb K^T |det|/n! + L_e K^T,
//   * the vertex gradients are the columns of Jb, vertex 0 takes minus their sum; in 2-D the two ends of the longest
//     edge get +-2 h2b (X_u - X_v) on top.
//   k_shape_tet<corrected, TT>  one lane per tet: the 3-D G-metric form with the handle's form variant (quadrature points,
//                               C_I, LSIC factor, PSPG sign) and, TT, the time term (u_t is nodal data: no geometry)
//   k_shape_tri                 one lane per triangle: the UGN form, each conditional differentiated on the branch it takes
//   k_gather_shape              node <- sum of the incident cells' vertex gradients in the fixed order of nt_ptr / nt_idx
// Per-cell results go to the handle's element scratch in the residual's layout, Ge[16 t + 4 a + j]; no atomics, so the
// result is bitwise reproducible.  Nothing of the handle besides that scratch is written.
#include "sns_ctx.h"

namespace sns {

template <bool corrected, bool TT>
__global__ __launch_bounds__(256) void k_shape_tet(int64_t n_tets, const int32_t* __restrict__ tets,
                                                   const double* __restrict__ pts, const double* __restrict__ w,
                                                   const double* __restrict__ lam, double nu, double* __restrict__ Ge,
                                                   FormVariant fv, TimeTerm tt) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tets) return;
    const int4 tv = *reinterpret_cast<const int4*>(tets + 4 * t);
    const int32_t nd[4] = {tv.x, tv.y, tv.z, tv.w};
    double X[4][3], W[4][4], V[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const double* pp = pts + 3 * (int64_t)nd[a];
        X[a][0] = pp[0]; X[a][1] = pp[1]; X[a][2] = pp[2];
        const double2* wp = reinterpret_cast<const double2*>(w + 4 * (int64_t)nd[a]);
        const double2 w0 = wp[0], w1 = wp[1];
        W[a][0] = w0.x; W[a][1] = w0.y; W[a][2] = w1.x; W[a][3] = w1.y;
        const double2* lp = reinterpret_cast<const double2*>(lam + 4 * (int64_t)nd[a]);
        const double2 l0 = lp[0], l1 = lp[1];
        V[a][0] = l0.x; V[a][1] = l0.y; V[a][2] = l1.x; V[a][3] = l1.y;
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
    double g[4][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        g[1][j] = K[0][j]; g[2][j] = K[1][j]; g[3][j] = K[2][j];
        g[0][j] = -(K[0][j] + K[1][j] + K[2][j]);
    }
    double G[3][3], trG = 0.0, GG = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            G[i][j] = K[0][i] * K[0][j] + K[1][i] * K[1][j] + K[2][i] * K[2][j];
            GG += G[i][j] * G[i][j];
            if (i == j) trG += G[i][j];
        }
    // gradients of the state (u, p) and of the test field (v, q) = lam on the cell
    double gu[3][3], gp[3], gv[3][3], gq[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        gp[j] = W[0][3] * g[0][j] + W[1][3] * g[1][j] + W[2][3] * g[2][j] + W[3][3] * g[3][j];
        gq[j] = V[0][3] * g[0][j] + V[1][3] * g[1][j] + V[2][3] * g[2][j] + V[3][3] * g[3][j];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            gu[i][j] = W[0][i] * g[0][j] + W[1][i] * g[1][j] + W[2][i] * g[2][j] + W[3][i] * g[3][j];
            gv[i][j] = V[0][i] * g[0][j] + V[1][i] * g[1][j] + V[2][i] * g[2][j] + V[3][i] * g[3][j];
        }
    }
    const double divu = gu[0][0] + gu[1][1] + gu[2][2];
    const double divv = gv[0][0] + gv[1][1] + gv[2][2];
    const double dd = divu * divv;
    double guv = 0.0;                                      // grad u : grad v
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) guv += gu[i][j] * gv[i][j];
    const double wd = fabs(det) * (1.0 / 24.0);
    double UT[TT ? 4 : 1][3];                              // nodal u_t = sigma u + d
    if constexpr (TT) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double* dp = tt.d + 4 * (int64_t)nd[a];
            const double2 d01 = *reinterpret_cast<const double2*>(dp);
            UT[a][0] = tt.sigma * W[a][0] + d01.x;
            UT[a][1] = tt.sigma * W[a][1] + d01.y;
            UT[a][2] = tt.sigma * W[a][2] + dp[2];
        }
    }
    // adjoints of grad u, grad p, grad v, grad q, G (symmetric) and the value L_e / wd; the viscous term is the same at
    // every point of the rule
    double gub[3][3], gpb[3], gvb[3][3], gqb[3], Gb[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        gpb[i] = 0.0; gqb[i] = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) { gub[i][j] = 4.0 * nu * gv[i][j]; gvb[i][j] = 4.0 * nu * gu[i][j]; Gb[i][j] = 0.0; }
    }
    double Lh = 4.0 * nu * guv, sb_sum = 0.0, trGb = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double u[3] = {0.0, 0.0, 0.0}, p = 0.0, vq[3] = {0.0, 0.0, 0.0}, qq = 0.0, ut[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double ph = (q == a) ? fv.qb : fv.qa;
            u[0] += ph * W[a][0]; u[1] += ph * W[a][1]; u[2] += ph * W[a][2]; p += ph * W[a][3];
            vq[0] += ph * V[a][0]; vq[1] += ph * V[a][1]; vq[2] += ph * V[a][2]; qq += ph * V[a][3];
            if constexpr (TT) { ut[0] += ph * UT[a][0]; ut[1] += ph * UT[a][1]; ut[2] += ph * UT[a][2]; }
        }
        double conv[3], r[3], m[3], uGu = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            uGu += u[i] * (G[i][0] * u[0] + G[i][1] * u[1] + G[i][2] * u[2]);
            conv[i] = gu[i][0] * u[0] + gu[i][1] * u[1] + gu[i][2] * u[2];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            // res_M and the direction it is tested with: (u.grad)v + pspg grad q, or the reference's dot(u, grad(.))
            r[j] = (corrected ? conv[j] : (gu[0][j] * u[0] + gu[1][j] * u[1] + gu[2][j] * u[2])) + gp[j] + ut[j];
            m[j] = (corrected ? (gv[j][0] * u[0] + gv[j][1] * u[1] + gv[j][2] * u[2])
                              : (gv[0][j] * u[0] + gv[1][j] * u[1] + gv[2][j] * u[2])) + fv.pspg * gq[j];
        }
        const double s = (TT ? tt.theta : 0.0) + uGu + fv.ci * nu * nu * GG;
        const double tau = 1.0 / sqrt(s);
        const double nuL = fv.lsic / (trG * tau);
        const double rm = r[0] * m[0] + r[1] * m[1] + r[2] * m[2];
        Lh += (conv[0] + ut[0]) * vq[0] + (conv[1] + ut[1]) * vq[1] + (conv[2] + ut[2]) * vq[2] - p * divv + qq * divu +
              tau * rm + nuL * dd;
        const double cu = qq + nuL * divv, cv = nuL * divu - p;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                gub[i][j] += vq[i] * u[j] + tau * (corrected ? m[i] * u[j] : u[i] * m[j]);
                gvb[i][j] += tau * (corrected ? r[i] * u[j] : u[i] * r[j]);
            }
            gub[i][i] += cu;
            gvb[i][i] += cv;
            gpb[i] += tau * m[i];
            gqb[i] += tau * fv.pspg * r[i];
        }
        // tau = s^-1/2, nu_LSIC = lsic s^1/2 / tr G
        const double sb = 0.5 * tau * tau * (nuL * dd - tau * rm);
        sb_sum += sb;
        trGb -= nuL * dd / trG;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) Gb[i][j] += sb * u[i] * u[j];
    }
    const double cg = 2.0 * fv.ci * nu * nu * sb_sum;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Gb[i][j] += cg * G[i][j];
        Gb[i][i] += trGb;
    }
    // adjoint of grad phi_a, then of K (g_0 = -(K_0 + K_1 + K_2), G = K^T K)
    double gb[4][3];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            gb[a][j] = W[a][0] * gub[0][j] + W[a][1] * gub[1][j] + W[a][2] * gub[2][j] + W[a][3] * gpb[j] +
                       V[a][0] * gvb[0][j] + V[a][1] * gvb[1][j] + V[a][2] * gvb[2][j] + V[a][3] * gqb[j];
    double Kb[3][3];
#pragma unroll
    for (int mm = 0; mm < 3; ++mm)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            Kb[mm][j] = gb[mm + 1][j] - gb[0][j] + 2.0 * (K[mm][0] * Gb[0][j] + K[mm][1] * Gb[1][j] + K[mm][2] * Gb[2][j]);
    double T[3][3];                                        // Kb K^T
#pragma unroll
    for (int mm = 0; mm < 3; ++mm)
#pragma unroll
        for (int n = 0; n < 3; ++n) T[mm][n] = Kb[mm][0] * K[n][0] + Kb[mm][1] * K[n][1] + Kb[mm][2] * K[n][2];
    const double Le = wd * Lh;
    double o[4][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double s0 = 0.0;
#pragma unroll
        for (int n = 0; n < 3; ++n) {
            const double jb = Le * K[n][i] - wd * (K[0][i] * T[0][n] + K[1][i] * T[1][n] + K[2][i] * T[2][n]);
            o[n + 1][i] = jb;
            s0 += jb;
        }
        o[0][i] = -s0;
    }
    double2* out = reinterpret_cast<double2*>(Ge + 16 * t);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        out[2 * a] = make_double2(o[a][0], o[a][1]);
        out[2 * a + 1] = make_double2(o[a][2], 0.0);
    }
}

// 2-D UGN form (LidDrivenNavierStokesFlow.py:123-143 == DFG_2D_Validation.py:141-163): the 3-point rule of dx(degree 2),
// the vertex that carries 2/3 is 0, 2, 1 for q = 0, 1, 2 (as k_residual_tri)
__global__ __launch_bounds__(256) void k_shape_tri(int64_t n_tris, const int32_t* __restrict__ tets,
                                                   const double* __restrict__ pts, const double* __restrict__ w,
                                                   const double* __restrict__ lam, double nu, double* __restrict__ Ge) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tris) return;
    const int4 tv = *reinterpret_cast<const int4*>(tets + 4 * t);
    const int32_t nd[3] = {tv.x, tv.y, tv.z};
    double X[3][2], W[3][3], V[3][3];                      // (ux, uy, p) of the state and of lam
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double* pp = pts + 3 * (int64_t)nd[a];
        X[a][0] = pp[0]; X[a][1] = pp[1];
        const double2* wp = reinterpret_cast<const double2*>(w + 4 * (int64_t)nd[a]);
        const double2 w0 = wp[0], w1 = wp[1];
        W[a][0] = w0.x; W[a][1] = w0.y; W[a][2] = w1.y;
        const double2* lp = reinterpret_cast<const double2*>(lam + 4 * (int64_t)nd[a]);
        const double2 l0 = lp[0], l1 = lp[1];
        V[a][0] = l0.x; V[a][1] = l0.y; V[a][2] = l1.y;
    }
    const double J00 = X[1][0] - X[0][0], J01 = X[2][0] - X[0][0];
    const double J10 = X[1][1] - X[0][1], J11 = X[2][1] - X[0][1];
    const double det = J00 * J11 - J01 * J10;
    const double id = 1.0 / det;
    double K[2][2];
    K[0][0] = J11 * id;  K[0][1] = -J01 * id;
    K[1][0] = -J10 * id; K[1][1] = J00 * id;
    double g[3][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        g[1][j] = K[0][j]; g[2][j] = K[1][j];
        g[0][j] = -(K[0][j] + K[1][j]);
    }
    const double wd = fabs(det) * (1.0 / 6.0);
    // CellDiameter^2 and the edge that carries it (the first of the order (0,1), (0,2), (1,2) on a tie)
    double h2 = 0.0;
    int eu = 1, ev = 0;
#pragma unroll
    for (int v = 0; v < 3; ++v)
#pragma unroll
        for (int u = v + 1; u < 3; ++u) {
            const double d0 = X[u][0] - X[v][0], d1 = X[u][1] - X[v][1];
            const double l2 = d0 * d0 + d1 * d1;
            if (l2 > h2) { h2 = l2; eu = u; ev = v; }
        }
    const double h = sqrt(h2);
    double gu[2][2], gp[2], gv[2][2], gq[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        gp[j] = W[0][2] * g[0][j] + W[1][2] * g[1][j] + W[2][2] * g[2][j];
        gq[j] = V[0][2] * g[0][j] + V[1][2] * g[1][j] + V[2][2] * g[2][j];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            gu[i][j] = W[0][i] * g[0][j] + W[1][i] * g[1][j] + W[2][i] * g[2][j];
            gv[i][j] = V[0][i] * g[0][j] + V[1][i] * g[1][j] + V[2][i] * g[2][j];
        }
    }
    const double divu = gu[0][0] + gu[1][1], divv = gv[0][0] + gv[1][1];
    const double dd = divu * divv;
    const double guv = gu[0][0] * gv[0][0] + gu[0][1] * gv[0][1] + gu[1][0] * gv[1][0] + gu[1][1] * gv[1][1];
    double gub[2][2], gpb[2] = {0.0, 0.0}, gvb[2][2], gqb[2] = {0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) { gub[i][j] = 3.0 * nu * gv[i][j]; gvb[i][j] = 3.0 * nu * gu[i][j]; }
    double Lh = 3.0 * nu * guv, h2b = 0.0;
    const double c4 = 4.0 / h2, i3 = 4.0 * nu / h2;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        double u[2] = {0.0, 0.0}, p = 0.0, vq[2] = {0.0, 0.0}, qq = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double ph = (a == ((3 - q) % 3)) ? 0.66666666666666663 : 0.16666666666666666;
            u[0] += ph * W[a][0]; u[1] += ph * W[a][1]; p += ph * W[a][2];
            vq[0] += ph * V[a][0]; vq[1] += ph * V[a][1]; qq += ph * V[a][2];
        }
        // tau_SUPG = (inv1 + (4 nu / h^2)^2)^-1/2, inv1 = |u| <= 1e-8 ? 0 : (2|u|/h)^2;  tau_LSIC = h/2 |u| z, z = Re_UGN <= 3 ?
        // Re_UGN / 3 : 1 -- and their derivatives with respect to h^2 on the branch taken
        const double uu = u[0] * u[0] + u[1] * u[1];
        const double un = sqrt(uu);
        const double inv1 = (un <= 1e-8) ? 0.0 : c4 * uu;
        const double tau = rsqrt(inv1 + i3 * i3);
        const double dtau = 0.5 * tau * tau * tau * (inv1 + 2.0 * i3 * i3) / h2;
        const double ReU = un * h / (2.0 * nu);
        double tauL, dtauL;
        if (ReU <= 3.0) {
            tauL = 0.5 * h * un * (ReU * 0.33333333333333333);
            dtauL = uu / (12.0 * nu);
        } else {
            tauL = 0.5 * h * un;
            dtauL = 0.25 * un / h;
        }
        double conv[2], r[2], m[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            conv[i] = gu[i][0] * u[0] + gu[i][1] * u[1];
            r[i] = conv[i] + gp[i];
            m[i] = gv[i][0] * u[0] + gv[i][1] * u[1] + gq[i];
        }
        const double rm = r[0] * m[0] + r[1] * m[1];
        Lh += conv[0] * vq[0] + conv[1] * vq[1] - p * divv + qq * divu + tau * rm + tauL * dd;
        h2b += dtau * rm + dtauL * dd;
        const double cu = qq + tauL * divv, cv = tauL * divu - p;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                gub[i][j] += (vq[i] + tau * m[i]) * u[j];
                gvb[i][j] += tau * r[i] * u[j];
            }
            gub[i][i] += cu;
            gvb[i][i] += cv;
            gpb[i] += tau * m[i];
            gqb[i] += tau * r[i];
        }
    }
    double gb[3][2];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            gb[a][j] = W[a][0] * gub[0][j] + W[a][1] * gub[1][j] + W[a][2] * gpb[j] +
                       V[a][0] * gvb[0][j] + V[a][1] * gvb[1][j] + V[a][2] * gqb[j];
    double T[2][2];                                        // Kb K^T,  Kb[m][j] = gb[m + 1][j] - gb[0][j]
#pragma unroll
    for (int mm = 0; mm < 2; ++mm)
#pragma unroll
        for (int n = 0; n < 2; ++n)
            T[mm][n] = (gb[mm + 1][0] - gb[0][0]) * K[n][0] + (gb[mm + 1][1] - gb[0][1]) * K[n][1];
    const double Le = wd * Lh;
    double o[3][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        double s0 = 0.0;
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const double jb = Le * K[n][i] - wd * (K[0][i] * T[0][n] + K[1][i] * T[1][n]);
            o[n + 1][i] = jb;
            s0 += jb;
        }
        o[0][i] = -s0;
    }
    // h^2 = |X_eu - X_ev|^2
    const double ch = 2.0 * wd * h2b;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const double e = ch * (X[eu][i] - X[ev][i]);
            if (a == eu) o[a][i] += e;
            if (a == ev) o[a][i] -= e;
        }
    double2* out = reinterpret_cast<double2*>(Ge + 16 * t);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        out[2 * a] = make_double2(o[a][0], o[a][1]);
        out[2 * a + 1] = make_double2(0.0, 0.0);
    }
    out[6] = make_double2(0.0, 0.0);
    out[7] = make_double2(0.0, 0.0);
}

// gX[3 i + j] <- sum over the cells of node i of Ge[16 t + 4 a + j], in list order (8 ids, then their 8 entries, as
// k_gather_residual); lane (i, j), the lanes j = 3 idle.  Declared in sns_kernels.h: the eigenvalue shape pass
// (csrc/sns_eigshape.hip) stages its cells in the same layout and launches this kernel too
__global__ __launch_bounds__(256) void k_gather_shape(int32_t n_rows, const int64_t* __restrict__ nt_ptr,
                                                      const int32_t* __restrict__ nt_idx, const double* __restrict__ Ge,
                                                      double* __restrict__ gX) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = gid >> 2;
    const int c = (int)(gid & 3);
    if (i >= n_rows || c == 3) return;
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
    gX[3 * i + c] = s;
}

// form, pointers and the communicator were checked by the entry point
int residual_shape_gradient(sns_ctx* h, const double* w, const double* lam, double* gX) {
    if (h->E == 0 || h->n == 0) {
        if (h->n > 0) HIP_TRY(hipMemsetAsync(gX, 0, (size_t)3 * h->n * sizeof(double), h->stream));
        return sync_stream(h);
    }
    if (!h->Fe) SNS_TRY(h->Fe.alloc((size_t)h->E * 16));
    const double nu = 1.0 / h->opt.reynolds;
    const unsigned gc = (unsigned)((h->E + 255) / 256);
    if (h->dim == 2)
        hipLaunchKernelGGL(k_shape_tri, dim3(gc), dim3(256), 0, h->stream, h->E, h->tets, h->pts, w, lam, nu, h->Fe);
    else
        dispatch<1, 0>(h->opt.corrected_convection != 0, [&](auto C) {
            dispatch<1, 0>(h->form.tt_on, [&](auto T) {
                hipLaunchKernelGGL((k_shape_tet<C() != 0, T() != 0>), dim3(gc), dim3(256), 0, h->stream, h->E, h->tets, h->pts, w,
                                   lam, nu, h->Fe, h->form.fv, h->form.tt);
            });
        });
    const int64_t nth = 4 * (int64_t)h->n;
    hipLaunchKernelGGL(k_gather_shape, dim3((unsigned)((nth + 255) / 256)), dim3(256), 0, h->stream, h->n, h->nt_ptr,
                       h->nt_idx, h->Fe, gX);
    HIP_TRY(hipGetLastError());
    return sync_stream(h);
}

}  // namespace sns
