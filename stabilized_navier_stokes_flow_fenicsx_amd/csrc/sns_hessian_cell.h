// One cell of the Hessian pass (csrc/sns_hessian.hip: k_state_gradient; tests/hessian_cell_main.cpp compiles the same text on
// the host): the gradient with respect to the cell's 16 state values of
//     phi_e(W) = c_J d/d eps [ z_e . R_e(W + eps x_e) ]_{eps = 0}  +  c_B z_e . ( R_e(W; d = x_u) - R_e(W) ),
// R_e the raw steady residual of the 3-D NS form on the cell, x_e and z_e held fixed.  Tangent in the direction x, then reverse
// mode, by hand.  With the P1 test field (v, q) = z_e, res_M = r, the SUPG / PSPG test direction m, s = u.Gu + C_I nu^2 G:G,
// tau = s^-1/2, kappa = lsic / tr G (nu_LSIC = kappa / tau) and dotted quantities the tangents along x, the part of the
// integrand's tangent that depends on W is, per quadrature point,
//     v . (grad x_u u + grad u x_q)  +  taud r.m  +  tau (rd.m + r.md)  +  kappa tau S div u div v  +  kappa div x_u div v / tau,
//     S = u.G x_q,  taud = -tau^3 S,  rd = d r[x],  md = d m[x]
// (the viscous term is linear in u for a fixed nu or nu_t and drops out, and so does everything linear in p: the pressure enters
// through grad p in r alone).  Its reverse sweep needs
//     d tau / d u = -tau^3 Gu,   d S / d u = G x_q,   and r, m, rd linear in u, grad u, grad p,
// and leaves per point the adjoint of u(q) -- spread over the vertices with N_a(q) -- and, summed over the points, the adjoints
// of grad u and grad p, which are constant on the cell and serve all four vertices through grad phi_a.  The mass part is
//     tau(u) x_q . m(u):   adjoint of u(q) = -tau^3 (x_q . m) Gu + tau (d m / d u)^T x_q.
// c_J and c_B enter as factors only, so doubling both doubles every bit of the result.
#pragma once

#if defined(__HIPCC__)
#define SNS_CELL_FN __device__ __forceinline__
#else
#include <cmath>
#define SNS_CELL_FN inline
#endif

namespace sns {

struct HessianForm {
    double ci, lsic, pspg, qa, qb, nu;                     // the form variant and the cell's viscosity
};

// g[a] = grad phi_a, G = K^T K with tr G and G:G, wd = |det J| / 24 (tet_metric); W = (u, p), Xd = x~, Z = z~ per vertex
// (constrained entries 0); out[a][c] = d phi_e / d W[a][c]
template <bool corrected>
SNS_CELL_FN void state_gradient_cell(const double g[4][3], const double G[3][3], double trG, double GG, double wd,
                                     const double W[4][4], const double Xd[4][4], const double Z[4][4], const HessianForm& f,
                                     double cj, double cb, double out[4][4]) {
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
    const double kdd = kap * (divu * divv), kxd = kap * (divx * divv), kdv = kap * divv;
    const double c0 = f.ci * f.nu * f.nu * GG;
    double usum[3], xsum[3], vsum[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        usum[j] = f.qa * (((W[0][j] + W[1][j]) + W[2][j]) + W[3][j]);
        xsum[j] = f.qa * (((Xd[0][j] + Xd[1][j]) + Xd[2][j]) + Xd[3][j]);
        vsum[j] = f.qa * (((Z[0][j] + Z[1][j]) + Z[2][j]) + Z[3][j]);
    }
    const double dq = f.qb - f.qa;
    double gub[3][3], gpb[3] = {0.0, 0.0, 0.0}, ubs[3] = {0.0, 0.0, 0.0};     // adjoints of grad u, grad p; sum_q of u(q)'s
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) gub[i][j] = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double u[3], xq[3], v[3], Gu[3], Gx[3], uGu = 0.0, S = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            u[j] = usum[j] + dq * W[q][j];
            xq[j] = xsum[j] + dq * Xd[q][j];
            v[j] = vsum[j] + dq * Z[q][j];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            Gu[i] = (G[i][0] * u[0] + G[i][1] * u[1]) + G[i][2] * u[2];
            Gx[i] = (G[i][0] * xq[0] + G[i][1] * xq[1]) + G[i][2] * xq[2];
            uGu += u[i] * Gu[i];
            S += Gu[i] * xq[i];
        }
        const double tau = 1.0 / sqrt(uGu + c0);
        const double t2 = tau * tau, t3 = t2 * tau;
        // r = res_M, m = its test direction, rd and md their tangents along x
        double r[3], m[3], rd[3], md[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
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
        const double taud = -t3 * S;
        const double taub = (cross - 3.0 * t2 * S * rm) + (S * kdd - kxd / t2);    // adjoint of tau
        const double Sb = tau * kdd - t3 * rm;                                      // adjoint of S
        double rb[3], mb[3], rdb[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            rb[j] = taud * m[j] + tau * md[j];
            mb[j] = taud * r[j] + tau * rd[j];
            rdb[j] = tau * m[j];
            gpb[j] += rb[j];
        }
        const double ctau = -t3 * taub, bt = -t3 * xm;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double lin, mB;
            if (corrected) {
                lin = (gu[0][k] * rb[0] + gu[1][k] * rb[1]) + gu[2][k] * rb[2];
                lin += (gv[0][k] * mb[0] + gv[1][k] * mb[1]) + gv[2][k] * mb[2];
                lin += (gx[0][k] * rdb[0] + gx[1][k] * rdb[1]) + gx[2][k] * rdb[2];
                mB = (gv[0][k] * xq[0] + gv[1][k] * xq[1]) + gv[2][k] * xq[2];
            } else {
                lin = (gu[k][0] * rb[0] + gu[k][1] * rb[1]) + gu[k][2] * rb[2];
                lin += (gv[k][0] * mb[0] + gv[k][1] * mb[1]) + gv[k][2] * mb[2];
                lin += (gx[k][0] * rdb[0] + gx[k][1] * rdb[1]) + gx[k][2] * rdb[2];
                mB = (gv[k][0] * xq[0] + gv[k][1] * xq[1]) + gv[k][2] * xq[2];
            }
            lin += (gx[0][k] * v[0] + gx[1][k] * v[1]) + gx[2][k] * v[2];          // the Galerkin convection v . grad x_u u
            const double ub = cj * ((ctau * Gu[k] + Sb * Gx[k]) + lin) + cb * (bt * Gu[k] + tau * mB);
            ubs[k] += ub;
            out[q][k] = dq * ub;                                                    // N_a(q) = qa + dq delta_aq
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                gub[i][j] += corrected ? (rb[i] * u[j] + (rdb[i] + v[i]) * xq[j]) : ((u[i] * rb[j] + xq[i] * rdb[j]) + v[i] * xq[j]);
            gub[i][i] += (tau * S) * kdv;
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
            out[a][i] = wd * ((out[a][i] + f.qa * ubs[i]) + cj * ((g[a][0] * gub[i][0] + g[a][1] * gub[i][1]) + g[a][2] * gub[i][2]));
        out[a][3] = wd * (cj * ((g[a][0] * gpb[0] + g[a][1] * gpb[1]) + g[a][2] * gpb[2]));
    }
}

}  // namespace sns
