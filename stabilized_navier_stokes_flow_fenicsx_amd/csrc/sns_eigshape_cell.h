// One cell of the eigenvalue shape pass (csrc/sns_eigshape.hip: k_eigshape_tet; tests/eigshape_cell_main.cpp compiles the same
// text on the host): the gradient with respect to the cell's 12 vertex coordinates of the Hessian pass's own scalar
//     phi_e(X_e) = c_J d/d eps [ z_e . R_e(W + eps x_e; X_e) ]_{eps = 0}  +  c_B z_e . ( R_e(W; d = x_u; X_e) - R_e(W; X_e) ),
// R_e the raw steady residual of the 3-D NS form on the cell, W, x_e and z_e held fixed.  The tangent along x is the one
// csrc/sns_hessian_cell.h forms; unlike there nothing drops out, because the terms linear in W still carry geometry.  With
// the P1 test field (v, q) = z_e, the direction (x_u, x_p) = x_e, res_M = r, its test direction m, rd and md their tangents,
// s = u.Gu + C_I nu^2 G:G, tau = s^-1/2, S = u.G x_q, taud = -tau^3 S and kappa = lsic / tr G, the integrand per point is
//     c_J [ v . (grad x_u u + grad u x_q) + nu grad x_u : grad v - x_p div v + q div x_u + taud r.m + tau (rd.m + r.md)
//           + kappa tau S div u div v + kappa div x_u div v / tau ]  +  c_B [ x_q . v + tau x_q . m ]
// (nu grad x_u : grad v reads 2 nu eps(x_u) : grad v in the stress-divergence form a viscosity field switches on).  Reverse
// mode through everything that carries geometry, as k_shape_tet (csrc/sns_shape.hip) does for lam . R_e:
//   * the adjoints of grad u, grad p, grad x_u, grad x_p, grad v, grad q, of G (kept symmetric), tr G (through kappa) and
//     G:G (through s) are accumulated over the quadrature points,
//   * folded into Kb = d phi / d K (grad phi_a = rows of K = J^-1, g_0 = -sum; G = K^T K),
//   * Jb = -K^T Kb K^T |det| / 24 + phi_e K^T; the vertex gradients are the columns of Jb, vertex 0 takes minus their sum.
// c_J and c_B enter as factors only, so doubling both doubles every bit of the result.
#pragma once

#include "sns_hessian_cell.h"

namespace sns {

// g[a] = grad phi_a, G = K^T K with tr G and G:G, wd = |det J| / 24 (tet_metric); W = (u, p), Xd = x~, Z = z~ per vertex
// (constrained entries 0); stress_div: the viscous term is (2 nu eps(u), grad v); out[a][j] = d phi_e / d X[a][j]
template <bool corrected>
SNS_CELL_FN void eigshape_cell(const double g[4][3], const double G[3][3], double trG, double GG, double wd, const double W[4][4],
                               const double Xd[4][4], const double Z[4][4], const HessianForm& f, bool stress_div, double cj,
                               double cb, double out[4][3]) {
    double gu[3][3], gp[3], gx[3][3], gxp[3], gv[3][3], gq[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        gp[j] = ((W[0][3] * g[0][j] + W[1][3] * g[1][j]) + W[2][3] * g[2][j]) + W[3][3] * g[3][j];
        gxp[j] = ((Xd[0][3] * g[0][j] + Xd[1][3] * g[1][j]) + Xd[2][3] * g[2][j]) + Xd[3][3] * g[3][j];
        gq[j] = ((Z[0][3] * g[0][j] + Z[1][3] * g[1][j]) + Z[2][3] * g[2][j]) + Z[3][3] * g[3][j];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            gu[i][j] = ((W[0][i] * g[0][j] + W[1][i] * g[1][j]) + W[2][i] * g[2][j]) + W[3][i] * g[3][j];
            gx[i][j] = ((Xd[0][i] * g[0][j] + Xd[1][i] * g[1][j]) + Xd[2][i] * g[2][j]) + Xd[3][i] * g[3][j];
            gv[i][j] = ((Z[0][i] * g[0][j] + Z[1][i] * g[1][j]) + Z[2][i] * g[2][j]) + Z[3][i] * g[3][j];
        }
    }
    const double divu = (gu[0][0] + gu[1][1]) + gu[2][2];
    const double divx = (gx[0][0] + gx[1][1]) + gx[2][2];
    const double divv = (gv[0][0] + gv[1][1]) + gv[2][2];
    const double kap = f.lsic / trG;
    const double dd = divu * divv, xd = divx * divv;
    const double c0 = f.ci * f.nu * f.nu * GG;
    double sums[4][4];                                     // qa * (sum over the vertices) of W, x~, z~ (rows 0..2) per slot
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        sums[0][c] = f.qa * (((W[0][c] + W[1][c]) + W[2][c]) + W[3][c]);
        sums[1][c] = f.qa * (((Xd[0][c] + Xd[1][c]) + Xd[2][c]) + Xd[3][c]);
        sums[2][c] = f.qa * (((Z[0][c] + Z[1][c]) + Z[2][c]) + Z[3][c]);
    }
    const double dq = f.qb - f.qa;
    // adjoints of the six gradients and of G; the viscous term is the same at every point of the rule
    double gub[3][3], gxb[3][3], gvb[3][3], gpb[3], gxpb[3], gqb[3], Gb[3][3];
    const double cv4 = cj * (4.0 * f.nu);
    double vis = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        gpb[i] = 0.0; gxpb[i] = 0.0; gqb[i] = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double sx = stress_div ? gx[i][j] + gx[j][i] : gx[i][j];
            const double sv = stress_div ? gv[i][j] + gv[j][i] : gv[i][j];
            vis += sx * gv[i][j];
            gub[i][j] = 0.0;
            gxb[i][j] = cv4 * sv;
            gvb[i][j] = cv4 * sx;
            Gb[i][j] = 0.0;
        }
    }
    double Phi = cv4 * vis, sb_sum = 0.0, kapb = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double u[3], xq[3], v[3], Gu[3], uGu = 0.0, S = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            u[j] = sums[0][j] + dq * W[q][j];
            xq[j] = sums[1][j] + dq * Xd[q][j];
            v[j] = sums[2][j] + dq * Z[q][j];
        }
        const double xp = sums[1][3] + dq * Xd[q][3], qq = sums[2][3] + dq * Z[q][3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            Gu[i] = (G[i][0] * u[0] + G[i][1] * u[1]) + G[i][2] * u[2];
            uGu += u[i] * Gu[i];
            S += Gu[i] * xq[i];
        }
        const double tau = 1.0 / sqrt(uGu + c0);
        const double t2 = tau * tau, t3 = t2 * tau;
        // r = res_M, m = its test direction, rd and md their tangents along x; ct = v . (grad x_u u + grad u x_q)
        double r[3], m[3], rd[3], md[3], ct = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            ct += v[j] * (((gx[j][0] * u[0] + gx[j][1] * u[1]) + gx[j][2] * u[2]) + ((gu[j][0] * xq[0] + gu[j][1] * xq[1]) + gu[j][2] * xq[2]));
            if (corrected) {
                r[j] = ((gu[j][0] * u[0] + gu[j][1] * u[1]) + gu[j][2] * u[2]) + gp[j];
                m[j] = ((gv[j][0] * u[0] + gv[j][1] * u[1]) + gv[j][2] * u[2]) + f.pspg * gq[j];
                rd[j] = (((gx[j][0] * u[0] + gx[j][1] * u[1]) + gx[j][2] * u[2]) +
                         ((gu[j][0] * xq[0] + gu[j][1] * xq[1]) + gu[j][2] * xq[2])) + gxp[j];
                md[j] = (gv[j][0] * xq[0] + gv[j][1] * xq[1]) + gv[j][2] * xq[2];
            } else {
                r[j] = ((gu[0][j] * u[0] + gu[1][j] * u[1]) + gu[2][j] * u[2]) + gp[j];
                m[j] = ((gv[0][j] * u[0] + gv[1][j] * u[1]) + gv[2][j] * u[2]) + f.pspg * gq[j];
                rd[j] = (((gx[0][j] * u[0] + gx[1][j] * u[1]) + gx[2][j] * u[2]) +
                         ((gu[0][j] * xq[0] + gu[1][j] * xq[1]) + gu[2][j] * xq[2])) + gxp[j];
                md[j] = (gv[0][j] * xq[0] + gv[1][j] * xq[1]) + gv[2][j] * xq[2];
            }
        }
        const double rm = (r[0] * m[0] + r[1] * m[1]) + r[2] * m[2];
        const double cross = ((rd[0] * m[0] + rd[1] * m[1]) + rd[2] * m[2]) + ((r[0] * md[0] + r[1] * md[1]) + r[2] * md[2]);
        const double xm = (xq[0] * m[0] + xq[1] * m[1]) + xq[2] * m[2];
        const double xv = (xq[0] * v[0] + xq[1] * v[1]) + xq[2] * v[2];
        const double taud = -t3 * S;
        const double kts = kap * (tau * S), kot = kap / tau;
        Phi += cj * ((((ct - xp * divv) + qq * divx) + (taud * rm + tau * cross)) + (kts * dd + kot * xd)) + cb * (xv + tau * xm);
        const double taub = cj * ((cross - 3.0 * t2 * S * rm) + kap * (S * dd - xd / t2)) + cb * xm;      // adjoint of tau
        const double Sb = cj * (kap * tau * dd - t3 * rm);                                                 // adjoint of S
        kapb += cj * ((tau * S) * dd + xd / tau);                                                          // adjoint of kappa
        const double sb = -0.5 * t3 * taub;                                                                // tau = s^-1/2
        sb_sum += sb;
        double rb[3], mb[3], rdb[3], mdb[3], vj[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            rb[j] = cj * (taud * m[j] + tau * md[j]);
            mb[j] = cj * (taud * r[j] + tau * rd[j]) + cb * (tau * xq[j]);
            rdb[j] = cj * (tau * m[j]);
            mdb[j] = cj * (tau * r[j]);
            vj[j] = cj * v[j];
            gpb[j] += rb[j];
            gxpb[j] += rdb[j];
            gqb[j] += f.pspg * mb[j];
        }
        const double du = cj * (kts * divv), dv = cj * ((kts * divu + kot * divx) - xp), dx = cj * (qq + kot * divv);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (corrected) {
                    gub[i][k] += (rb[i] * u[k] + rdb[i] * xq[k]) + vj[i] * xq[k];
                    gxb[i][k] += rdb[i] * u[k] + vj[i] * u[k];
                    gvb[i][k] += mb[i] * u[k] + mdb[i] * xq[k];
                } else {
                    gub[i][k] += (u[i] * rb[k] + xq[i] * rdb[k]) + vj[i] * xq[k];
                    gxb[i][k] += u[i] * rdb[k] + vj[i] * u[k];
                    gvb[i][k] += u[i] * mb[k] + xq[i] * mdb[k];
                }
                Gb[i][k] += sb * (u[i] * u[k]) + (0.5 * Sb) * (u[i] * xq[k] + u[k] * xq[i]);
            }
            gub[i][i] += du;
            gvb[i][i] += dv;
            gxb[i][i] += dx;
        }
    }
    // s = u.Gu + C_I nu^2 G:G and kappa = lsic / tr G
    const double cg = 2.0 * (f.ci * f.nu * f.nu) * sb_sum, trGb = -(kapb * kap) / trG;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Gb[i][j] += cg * G[i][j];
        Gb[i][i] += trGb;
    }
    // adjoint of grad phi_a, then of K = g[1..3] (g_0 = -(K_0 + K_1 + K_2), G = K^T K)
    double gb[4][3];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            gb[a][j] = ((((W[a][0] * gub[0][j] + W[a][1] * gub[1][j]) + W[a][2] * gub[2][j]) + W[a][3] * gpb[j]) +
                        (((Xd[a][0] * gxb[0][j] + Xd[a][1] * gxb[1][j]) + Xd[a][2] * gxb[2][j]) + Xd[a][3] * gxpb[j])) +
                       (((Z[a][0] * gvb[0][j] + Z[a][1] * gvb[1][j]) + Z[a][2] * gvb[2][j]) + Z[a][3] * gqb[j]);
    double Kb[3][3];
#pragma unroll
    for (int mm = 0; mm < 3; ++mm)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            Kb[mm][j] = (gb[mm + 1][j] - gb[0][j]) +
                        2.0 * ((g[mm + 1][0] * Gb[0][j] + g[mm + 1][1] * Gb[1][j]) + g[mm + 1][2] * Gb[2][j]);
    double T[3][3];                                        // Kb K^T
#pragma unroll
    for (int mm = 0; mm < 3; ++mm)
#pragma unroll
        for (int n = 0; n < 3; ++n)
            T[mm][n] = (Kb[mm][0] * g[n + 1][0] + Kb[mm][1] * g[n + 1][1]) + Kb[mm][2] * g[n + 1][2];
    const double Le = wd * Phi;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double s0 = 0.0;
#pragma unroll
        for (int n = 0; n < 3; ++n) {
            const double jb = Le * g[n + 1][i] - wd * ((g[1][i] * T[0][n] + g[2][i] * T[1][n]) + g[3][i] * T[2][n]);
            out[n + 1][i] = jb;
            s0 += jb;
        }
        out[0][i] = -s0;
    }
}

}  // namespace sns
