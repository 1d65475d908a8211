// The element code of the four forms, shared by the translation units that instantiate kernels over it: the staged element
// kernel k_element and the per-block code block_accumulate<FORM, ...> the owner-computes passes are made of (csrc/sns_kernels.hip:
// k_fused_offdiag / k_fused_diag / k_fused_lift; csrc/sns_rawjac.hip: k_raw_jacobian_apply).  The text stands in the order it
// always had in csrc/sns_kernels.hip, which includes it in its old place: that unit's token stream, and with it its device code,
// is what it was.  SNS_ELEMENT_INSTANTIATE (set by csrc/sns_kernels.hip alone) emits k_element's explicit instantiations where
// they always stood.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "sns_kernels.h"

namespace sns {

// ============================================================================
// K1: element kernel
// ============================================================================
// 16 lanes per tet: lane (a,b) owns the 4x4 block coupling local vertices a,b.
// One wave = 4 tets, one 256-thread workgroup = 16 tets.  Nodal coordinates and
// the nodal state are staged in LDS once per tet; lanes 0..3 of a tet compute
// the geometry and the per-quadrature-point scalars (tau, nu_LSIC, u_q, ...)
// into LDS, then all 16 lanes accumulate their block over the 4 points.  The
// 256 blocks of a workgroup are transposed through LDS so that every store
// instruction writes 1 KiB contiguous.
//
// Math: SURVEY.md Appendix A == oracle/element.py, restating
// NavierStokesChannelFlow.py:160-172 (Stokes) and :220-251 + :46 (NS + exact
// Gateaux derivative).

#define QA 0.1381966011250105
#define QB 0.5854101966249685

constexpr int EL_TPB = 256;
constexpr int EL_TETS = EL_TETS_PER_BLOCK;

struct TetLds {
    double X[12];
    double W[16];
    double GW[16];     // (g - w) on Dirichlet dofs, 0 elsewhere  -> lifting (:65)
    double g[12];      // grad phi_a  [a][j]
    double gu[9];      // grad u      [i][j]
    double guga[12];   // (grad u) g_a [a][i]
    double sc[4];      // wd = |detJ|/24, div u, tr G, h^2 (Stokes)
    double q[4][16];   // per point: u[3], p, tau, nuL, Gu[3], conv[3], s[4]
};

// ... with a time term (TT): the nodal history and the per-point u_t = sigma u + d
struct TetLdsT : TetLds {
    double D[12];      // d [a][i]
    double ut[4][3];
};

// ... with a viscosity law (VL): eps g_a per vertex and the tet's nu_e, d nu_e / d s, 4 C_I nu_e nu' G:G
struct TetLdsV : TetLds {
    double eg[12];     // (eps g_a) [a][i]
    double vs[3];
};

// ... with a viscosity field (EV): the time term's data, eps g_a per vertex and the tet's nu_t
struct TetLdsE : TetLdsT {
    double eg[12];     // (eps g_a) [a][i]
    double nue;
};

__device__ __forceinline__ double phi_q(int q, int a) { return q == a ? QB : QA; }

// s = 2 eps:eps (= gamma_dot^2) of a constant grad u, eps = sym(grad u)
__device__ __forceinline__ double shear_rate2(const double gu[3][3]) {
    const double a = gu[0][1] + gu[1][0], b = gu[0][2] + gu[2][0], c = gu[1][2] + gu[2][1];
    return 2.0 * (gu[0][0] * gu[0][0] + gu[1][1] * gu[1][1] + gu[2][2] * gu[2][2]) + a * a + b * b + c * c;
}
// (eps v)_i = 1/2 ((grad u) v + (grad u)^T v)_i
__device__ __forceinline__ void eps_apply(const double gu[3][3], const double v[3], double out[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
        out[i] = 0.5 * ((gu[i][0] + gu[0][i]) * v[0] + (gu[i][1] + gu[1][i]) * v[1] + (gu[i][2] + gu[2][i]) * v[2]);
}
// Carreau law on s: nu_e = nu0 (r + (1 - r) (1 + lambda^2 s)^((n-1)/2)) and dnu = d nu_e / d s.  No square root of s:
// smooth at rest.  n = 1 gives nu_e == nu0 in every bit (exp(0) = 1, r + (1 - r) rounds to 1).
__device__ __forceinline__ void carreau(const ViscosityLaw& vl, double nu0, double s, double& nu_e, double& dnu) {
    const double l2 = vl.lambda * vl.lambda;
    const double x = 1.0 + l2 * s;
    const double e = 0.5 * (vl.n - 1.0);
    const double pw = exp(e * log(x));
    nu_e = nu0 * (vl.r + (1.0 - vl.r) * pw);
    dnu = nu0 * (1.0 - vl.r) * e * l2 * (pw / x);
}

template <int FORM, bool corrected, bool TT, bool VL, bool EV>
__global__ __launch_bounds__(EL_TPB, 3) void k_element(int64_t n_tets, const int32_t* __restrict__ tets,
                                                    const double* __restrict__ pts,
                                                    const double* __restrict__ w,
                                                    const uint8_t* __restrict__ bc_mask,
                                                    const double* __restrict__ bc_val, double nu,
                                                    int store_K, double* __restrict__ Ke,
                                                    double* __restrict__ Fe, FormVariant fv, TimeTerm tt,
                                                    ViscosityLaw vl) {
    static_assert(!VL || (FORM == SNS_FORM_NS && !TT), "the viscosity law exists in the steady 3-D NS form only");
    static_assert(!EV || (FORM == SNS_FORM_NS && TT && !VL), "the viscosity field is a variant of the 3-D NS form with the time term");
    // staging data and the output transpose tile share LDS (the tile is written after a barrier
    // that retires every read of the staging data): 34.8 KB per workgroup -> 4 workgroups per CU
    using Lds = std::conditional_t<EV, TetLdsE, std::conditional_t<TT, TetLdsT, std::conditional_t<VL, TetLdsV, TetLds>>>;
    constexpr size_t SH_BYTES = sizeof(Lds) * EL_TETS, TILE_BYTES = sizeof(double) * EL_TPB * 17;
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[SH_BYTES > TILE_BYTES ? SH_BYTES : TILE_BYTES];
    Lds* sh = reinterpret_cast<Lds*>(lds_raw);
    double* tile = reinterpret_cast<double*>(lds_raw);

    const int tid = threadIdx.x;
    const int tl = tid >> 4;            // tet within workgroup
    const int l = tid & 15;             // lane within tet
    const int a = l >> 2, b = l & 3;
    const int64_t t = (int64_t)blockIdx.x * EL_TETS + tl;
    const bool live = t < n_tets;
    Lds& S = sh[tl];

    // ---- stage nodal data ----------------------------------------------------
    if (live) {
        const int32_t na = tets[4 * t + a];
        const int64_t dof = 4 * (int64_t)na + b;      // lane l <-> local dof 4a+c with c=b
        const double wv = w ? w[dof] : 0.0;
        S.W[l] = wv;
        S.GW[l] = bc_mask[dof] ? (bc_val[dof] - wv) : 0.0;
        if constexpr (TT) {
            if (b < 3) S.D[3 * a + b] = tt.d[dof];
        }
        if (l < 12) {
            const int32_t nv = tets[4 * t + l / 3];
            S.X[l] = pts[3 * (int64_t)nv + l % 3];
        }
    }
    __syncthreads();

    // ---- geometry + per-point scalars (lanes 0..3 = quadrature points) -------
    if (live && l < 4) {
        const int q = l;
        const double* X = S.X;
        double J[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            J[i][0] = X[3 + i] - X[i];
            J[i][1] = X[6 + i] - X[i];
            J[i][2] = X[9 + i] - X[i];
        }
        const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
        const double c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
        const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
        const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
        const double id = 1.0 / det;
        double K[3][3];                                   // K = J^-1
        K[0][0] = c00 * id;
        K[1][0] = c01 * id;
        K[2][0] = c02 * id;
        K[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id;
        K[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id;
        K[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * id;
        K[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * id;
        K[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id;
        K[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * id;
        double g[4][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            g[1][j] = K[0][j];
            g[2][j] = K[1][j];
            g[3][j] = K[2][j];
            g[0][j] = -(K[0][j] + K[1][j] + K[2][j]);
        }
        double G[3][3];                                   // G = K^T K   (:235)
        double trG = 0.0, GG = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                G[i][j] = K[0][i] * K[0][j] + K[1][i] * K[1][j] + K[2][i] * K[2][j];
                GG += G[i][j] * G[i][j];
                if (i == j) trG += G[i][j];
            }
        const double* W = S.W;
        double gu[3][3], gp[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            gp[j] = W[3] * g[0][j] + W[7] * g[1][j] + W[11] * g[2][j] + W[15] * g[3][j];
#pragma unroll
            for (int i = 0; i < 3; ++i)
                gu[i][j] = W[i] * g[0][j] + W[4 + i] * g[1][j] + W[8 + i] * g[2][j] + W[12 + i] * g[3][j];
        }
        const double divu = gu[0][0] + gu[1][1] + gu[2][2];
        double nu_t = nu;                                 // the tet's viscosity
        if constexpr (VL) {
            double dnu;
            carreau(vl, nu, shear_rate2(gu), nu_t, dnu);
            if (q == 0) {
#pragma unroll
                for (int aa = 0; aa < 4; ++aa) {
                    double e3[3];
                    eps_apply(gu, g[aa], e3);
                    S.eg[3 * aa] = e3[0]; S.eg[3 * aa + 1] = e3[1]; S.eg[3 * aa + 2] = e3[2];
                }
                S.vs[0] = nu_t;
                S.vs[1] = dnu;
                S.vs[2] = 4.0 * fv.ci * nu_t * dnu * GG;   // d(C_I nu_e^2 G:G)/2 = vs[2] (eps g_b) . du_b
            }
        }
        if constexpr (EV) {
            nu_t = tt.nu_t[t];
            if (q == 0) {
#pragma unroll
                for (int aa = 0; aa < 4; ++aa) {
                    double e3[3];
                    eps_apply(gu, g[aa], e3);
                    S.eg[3 * aa] = e3[0]; S.eg[3 * aa + 1] = e3[1]; S.eg[3 * aa + 2] = e3[2];
                }
                S.nue = nu_t;
            }
        }
        if (q == 0) {
#pragma unroll
            for (int aa = 0; aa < 4; ++aa)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    S.g[3 * aa + j] = g[aa][j];
                    // (grad u) g_a, or for the corrected form g_a^T (grad u) (the transpose contraction)
                    S.guga[3 * aa + j] = corrected
                        ? (g[aa][0] * gu[0][j] + g[aa][1] * gu[1][j] + g[aa][2] * gu[2][j])
                        : (gu[j][0] * g[aa][0] + gu[j][1] * g[aa][1] + gu[j][2] * g[aa][2]);
                }
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) S.gu[3 * i + j] = gu[i][j];
            double h2 = 0.0;                               // CellDiameter^2 (:168)
#pragma unroll
            for (int aa = 0; aa < 4; ++aa)
#pragma unroll
                for (int bb = aa + 1; bb < 4; ++bb) {
                    const double d0 = X[3 * aa] - X[3 * bb], d1 = X[3 * aa + 1] - X[3 * bb + 1],
                                 d2 = X[3 * aa + 2] - X[3 * bb + 2];
                    h2 = fmax(h2, d0 * d0 + d1 * d1 + d2 * d2);
                }
            S.sc[0] = fabs(det) * (1.0 / 24.0);
            S.sc[1] = divu;
            S.sc[2] = trG;
            S.sc[3] = h2;
        }
        if (FORM == SNS_FORM_NS) {
            double u[3], p = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) u[i] = 0.0;
#pragma unroll
            for (int aa = 0; aa < 4; ++aa) {
                const double ph = (q == aa) ? fv.qb : fv.qa;
#pragma unroll
                for (int i = 0; i < 3; ++i) u[i] += ph * W[4 * aa + i];
                p += ph * W[4 * aa + 3];
            }
            double Gu[3], conv[3], r[3];
            double uGu = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                Gu[i] = G[i][0] * u[0] + G[i][1] * u[1] + G[i][2] * u[2];
                uGu += u[i] * Gu[i];
                conv[i] = gu[i][0] * u[0] + gu[i][1] * u[1] + gu[i][2] * u[2];          // (u.grad)u :243
            }
#pragma unroll
            for (int j = 0; j < 3; ++j)                       // res_M :241  (reference: dot(u, grad(u)) = (grad u)^T u)
                r[j] = (corrected ? conv[j] : (gu[0][j] * u[0] + gu[1][j] * u[1] + gu[2][j] * u[2])) + gp[j];
            double theta = 0.0;
            if constexpr (TT) {
                // u_t = sigma u + d at the point, into res_M; theta under the root of tau
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    double dq = 0.0;
#pragma unroll
                    for (int aa = 0; aa < 4; ++aa) dq += ((q == aa) ? fv.qb : fv.qa) * S.D[3 * aa + i];
                    const double ut = tt.sigma * u[i] + dq;
                    S.ut[q][i] = ut;
                    r[i] += ut;
                }
                theta = tt.theta;
            }
            const double tau = 1.0 / sqrt(theta + uGu + fv.ci * nu_t * nu_t * GG);        // :237-238 (C_I = 36)
            const double nuL = fv.lsic / (trG * tau);                                    // :249
            double* Q = S.q[q];
            Q[0] = u[0]; Q[1] = u[1]; Q[2] = u[2]; Q[3] = p; Q[4] = tau; Q[5] = nuL;
            Q[6] = Gu[0]; Q[7] = Gu[1]; Q[8] = Gu[2];
            Q[9] = conv[0]; Q[10] = conv[1]; Q[11] = conv[2];
#pragma unroll
            for (int aa = 0; aa < 4; ++aa) Q[12 + aa] = r[0] * g[aa][0] + r[1] * g[aa][1] + r[2] * g[aa][2];
        }
    }
    __syncthreads();

    // ---- block (a,b): accumulate over quadrature points -----------------------
    double acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0;
    double Rl[4] = {0.0, 0.0, 0.0, 0.0};                 // residual of local node a (lanes with b==0 only, NS)
    // Jacobian blocks are needed when they are stored, or when this tet has a Dirichlet dof whose
    // value differs from g (lifting term A0[:,B](g - x_B), :65).  Residual-only evaluations of the
    // line search skip them otherwise.
    const unsigned long long lift_mask = __ballot(live && S.GW[l] != 0.0);
    const bool need_blocks = store_K || FORM == SNS_FORM_STOKES || ((lift_mask >> (threadIdx.x & 48)) & 0xFFFFull) != 0;
    if (live) {
        const double ga0 = S.g[3 * a], ga1 = S.g[3 * a + 1], ga2 = S.g[3 * a + 2];
        const double gb0 = S.g[3 * b], gb1 = S.g[3 * b + 1], gb2 = S.g[3 * b + 2];
        const double ga[3] = {ga0, ga1, ga2}, gb[3] = {gb0, gb1, gb2};
        const double gab = ga0 * gb0 + ga1 * gb1 + ga2 * gb2;
        const double wd = S.sc[0], divu = S.sc[1], trG = S.sc[2];
        // viscosity law: nu_e for nu, the viscous term 2 nu_e eps g_a, d tau and d nu_LSIC gain kb = 4 C_I nu_e nu' G:G eps g_b
        // (eps g_a and eps g_b stay in LDS: only kb lives across the quadrature loop)
        auto eg = [&](int k) -> double {
            if constexpr (VL || EV) return S.eg[k];
            else return 0.0;
        };
        double nu_t = nu, kb[3] = {0.0, 0.0, 0.0};
        if constexpr (VL) {
            nu_t = S.vs[0];
#pragma unroll
            for (int j = 0; j < 3; ++j) kb[j] = S.vs[2] * eg(3 * b + j);
        }
        if constexpr (EV) nu_t = S.nue;
        if (FORM == SNS_FORM_STOKES) {
            const double vol = 4.0 * wd;
            const double muT = 0.2 * S.sc[3];                                            // :169
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                acc[5 * i] = vol * gab;                     // (grad u, grad v)
                acc[4 * i + 3] = -wd * ga[i];               // -(p, div v)   int phi_b = vol/4 = wd
                acc[12 + i] = wd * gb[i];                   // +(div u, q)
            }
            acc[15] = muT * vol * gab;                      // mu_T (grad p, grad q)
        } else {
            const double* gum = S.gu;
            const double gg0 = S.guga[3 * a], gg1 = S.guga[3 * a + 1], gg2 = S.guga[3 * a + 2];
            const double guga_a[3] = {gg0, gg1, gg2};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double* Q = S.q[q];
                const double pa = (q == a) ? fv.qb : fv.qa, pb = (q == b) ? fv.qb : fv.qa;
                const double u[3] = {Q[0], Q[1], Q[2]};
                const double tau = Q[4], nuL = Q[5];
                const double Gu[3] = {Q[6], Q[7], Q[8]};
                const double sa = Q[12 + a];
                const double ugb = u[0] * gb0 + u[1] * gb1 + u[2] * gb2;
                const double uga = u[0] * ga0 + u[1] * ga1 + u[2] * ga2;
                // coefficient of delta_ij; convection phi_a (g_b.u); viscous; SUPG tau s_a phi_b
                // (corrected form: test function (u.grad)v = (u.g_a) e_i, so tau*(r.e_i) pieces differ, see below)
                double cu[3], cg[3];
                const double t3 = tau * tau * tau;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    double dtau = -t3 * pb * Gu[j];                               // d tau / d u_(b,j)
                    double dnuL = fv.lsic * (tau / trG) * pb * Gu[j];             // d nu_L
                    if constexpr (VL) {
                        dtau -= t3 * kb[j];
                        dnuL += fv.lsic * (tau / trG) * kb[j];
                    }
                    cg[j] = dnuL * divu + nuL * gb[j];
                    if (!corrected) {
                        // d(r.g_a) = u_j g_a.g_b + phi_b ((grad u) g_a)_j
                        cu[j] = dtau * sa + tau * (u[j] * gab + pb * guga_a[j]);
                        if constexpr (TT) cu[j] += tau * tt.sigma * pb * ga[j];      // d(u_t.g_a)
                    } else {
                        cu[j] = dtau;                                              // used differently below
                    }
                }
                if (!need_blocks) {
                } else if (!corrected) {
                    double A1 = pa * ugb + nu_t * gab + tau * sa * pb;
                    if constexpr (TT) A1 += tt.sigma * pa * pb;                       // mass
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
#pragma unroll
                        for (int j = 0; j < 3; ++j)
                            acc[4 * i + j] += pa * pb * gum[3 * i + j] + u[i] * cu[j] + ga[i] * cg[j];
                        acc[5 * i] += A1;
                        acc[4 * i + 3] += -pb * ga[i] + tau * u[i] * gab;        // J[(a,i),(b,p)]
                        acc[12 + i] += pa * gb[i] + fv.pspg * cu[i];             // J[(a,p),(b,j)]
                    }
                    acc[15] += fv.pspg * tau * gab;
                } else {
                    // corrected variant: res_M = (u.grad)u + grad p ; SUPG test = (u.grad)v + grad q
                    //   R[(a,i)] += tau (u.g_a) r_i ; R[(a,p)] += tau (r.g_a)
                    // with r = conv + gp: d r_i/d u_(b,j) = delta_ij (u.g_b) + phi_b gu[i][j]
                    const double r0 = Q[9] + 0.0, r1 = Q[10], r2 = Q[11];
                    // r (without grad p) is conv; s_a already holds r.g_a incl. grad p; recover r_i:
                    // S.q stores conv and s only, so rebuild r_i = conv_i + gp_i via gp = sum_a P_a g_a
                    double gp[3];
#pragma unroll
                    for (int j = 0; j < 3; ++j)
                        gp[j] = S.W[3] * S.g[j] + S.W[7] * S.g[3 + j] + S.W[11] * S.g[6 + j] + S.W[15] * S.g[9 + j];
                    double r[3] = {r0 + gp[0], r1 + gp[1], r2 + gp[2]};
                    double A1 = pa * ugb + nu_t * gab + tau * uga * ugb;
                    double mp = 0.0;                                                  // d(tau u_t.g_a) / d u_(b,i) / g_a[i]
                    if constexpr (TT) {
#pragma unroll
                        for (int i = 0; i < 3; ++i) r[i] += S.ut[q][i];
                        A1 += tt.sigma * pb * (pa + tau * uga);                       // mass + SUPG of u_t
                        mp = fv.pspg * tau * tt.sigma * pb;
                    }
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
#pragma unroll
                        for (int j = 0; j < 3; ++j)
                            acc[4 * i + j] += pa * pb * gum[3 * i + j]
                                + cu[j] * uga * r[i]                               // d tau
                                + tau * pb * ga[j] * r[i]                          // d (u.g_a)
                                + tau * uga * pb * gum[3 * i + j]                  // d r_i (phi_b gu_ij)
                                + ga[i] * cg[j];
                        acc[5 * i] += A1;
                        acc[4 * i + 3] += -pb * ga[i] + tau * uga * gb[i];       // d r_i / d p_b = g_b[i]
                        // continuity row: phi_a g_b[j] + d(tau r.g_a)
                        acc[12 + i] += pa * gb[i] + fv.pspg * (cu[i] * sa + tau * (ugb * ga[i] + pb * guga_a[i]));
                        if constexpr (TT) acc[12 + i] += mp * ga[i];
                    }
                    acc[15] += fv.pspg * tau * gab;
                }
                if (b == 0) {                               // residual of node a
                    const double p = Q[3];
                    if (!corrected) {
#pragma unroll
                        for (int i = 0; i < 3; ++i)
                            Rl[i] += Q[9 + i] * pa + ((VL || EV) ? 2.0 * nu_t * eg(3 * a + i) : nu * guga_a[i]) - p * ga[i] + tau * u[i] * sa +
                                     nuL * divu * ga[i];
                        if constexpr (TT) {
#pragma unroll
                            for (int i = 0; i < 3; ++i) Rl[i] += pa * S.ut[q][i];
                        }
                    } else {
                        double gp[3];
#pragma unroll
                        for (int j = 0; j < 3; ++j)
                            gp[j] = S.W[3] * S.g[j] + S.W[7] * S.g[3 + j] + S.W[11] * S.g[6 + j] + S.W[15] * S.g[9 + j];
                        // nu (grad u):(grad v) needs (grad u) g_a regardless of the variant
                        const double vg[3] = {gum[0] * ga0 + gum[1] * ga1 + gum[2] * ga2,
                                              gum[3] * ga0 + gum[4] * ga1 + gum[5] * ga2,
                                              gum[6] * ga0 + gum[7] * ga1 + gum[8] * ga2};
#pragma unroll
                        for (int i = 0; i < 3; ++i)
                            Rl[i] += Q[9 + i] * pa + ((VL || EV) ? 2.0 * nu_t * eg(3 * a + i) : nu * vg[i]) - p * ga[i] + tau * uga * (Q[9 + i] + gp[i]) +
                                     nuL * divu * ga[i];
                        if constexpr (TT) {
#pragma unroll
                            for (int i = 0; i < 3; ++i) Rl[i] += (pa + tau * uga) * S.ut[q][i];
                        }
                    }
                    Rl[3] += pa * divu + fv.pspg * tau * sa;
                }
            }
            if constexpr (VL) {
                // point-independent: the transpose half of 2 nu_e d eps, and the rank-one 2 (eps g_a) d nu_e^T
                if (need_blocks) {
                    const double c1 = 4.0 * nu_t, c2 = 32.0 * S.vs[1];
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const double ei = c2 * S.eg[3 * a + i], gi = c1 * gb[i];
#pragma unroll
                        for (int j = 0; j < 3; ++j) acc[4 * i + j] += gi * ga[j] + ei * S.eg[3 * b + j];
                    }
                }
            }
            if constexpr (EV) {
                // point-independent: the transpose half of 2 nu_t d eps (nu_t is held fixed: no rank-one part)
                if (need_blocks) {
                    const double c1 = 4.0 * nu_t;
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const double gi = c1 * gb[i];
#pragma unroll
                        for (int j = 0; j < 3; ++j) acc[4 * i + j] += gi * ga[j];
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] *= wd;
#pragma unroll
            for (int c = 0; c < 4; ++c) Rl[c] *= wd;
        }
    }

    // ---- element residual: Fe[a][c] = R[a][c] + sum_b block(a,b) * (g-w)_b   (lifting :65)
    // Stokes: R = sum_b block(a,b) * w_b (linear form), so the same reduction with (w + (g-w)).
    if (Fe) {
        double part[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            double s = 0.0;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const double xv = (FORM == SNS_FORM_STOKES) ? (S.W[4 * b + d] + S.GW[4 * b + d]) : S.GW[4 * b + d];
                s += acc[4 * c + d] * xv;
            }
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            part[c] = s + Rl[c];
        }
        if (live && b == 0) {
            double* o = Fe + (4 * t + a) * 4;
            o[0] = part[0]; o[1] = part[1]; o[2] = part[2]; o[3] = part[3];
        }
    }

    // ---- transpose 256 blocks through LDS, store 1 KiB per wave instruction ----
    if (store_K) {
        __syncthreads();                                    // all reads of the staging data are done
#pragma unroll
        for (int e = 0; e < 16; ++e) tile[tid * 17 + e] = acc[e];
        __syncthreads();
        const int64_t base = (int64_t)blockIdx.x * (EL_TETS * 256);
        const int64_t lim = n_tets * 256;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int idx = i * EL_TPB + tid;
            const int64_t gidx = base + idx;
            if (gidx < lim) Ke[gidx] = tile[(idx >> 4) * 17 + (idx & 15)];
        }
    }
}

#ifdef SNS_ELEMENT_INSTANTIATE
#define SNS_INST_ELEMENT(F, C, T, V, E)                                                                     \
    template __global__ void k_element<F, C, T, V, E>(int64_t, const int32_t*, const double*, const double*,      \
                                                   const uint8_t*, const double*, double, int, double*, double*, \
                                                   FormVariant, TimeTerm, ViscosityLaw);
SNS_INST_ELEMENT(SNS_FORM_STOKES, false, false, false, false)
SNS_INST_ELEMENT(SNS_FORM_NS, false, false, false, false)
SNS_INST_ELEMENT(SNS_FORM_NS, true, false, false, false)
SNS_INST_ELEMENT(SNS_FORM_NS, false, true, false, false)
SNS_INST_ELEMENT(SNS_FORM_NS, true, true, false, false)
SNS_INST_ELEMENT(SNS_FORM_NS, false, false, true, false)
SNS_INST_ELEMENT(SNS_FORM_NS, true, false, true, false)
SNS_INST_ELEMENT(SNS_FORM_NS, false, true, false, true)
SNS_INST_ELEMENT(SNS_FORM_NS, true, true, false, true)
#endif

// quad-permute a double with DPP moves (no LDS, no memory traffic); CTRL = quad_perm encoding
template <int CTRL>
__device__ __forceinline__ double quad_perm(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xF, 0xF, true);
    hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}

// ============================================================================
// K1 (scratch-free variant): every BSR block is produced by the lane(s) that own it.
// A lane walks the block's contribution list (tet, a, b) and recomputes the element
// block on the fly, so nothing is staged in HBM: no 2 KiB/tet scratch write, no gather pass,
// no atomics, fixed summation order (bitwise reproducible).  Costs ~2x the block flops of the
// staged kernel (geometry + per-point scalars are recomputed per contribution) and only applies
// when the state satisfies the Dirichlet data (no lifting term, :65), i.e. every Newton iterate
// after the first update; the staged k_element path handles the rest.
// ============================================================================
template <bool corrected, bool TT, bool VL, bool EV>
__device__ __forceinline__ void tet_block_accumulate(const int4 tv, const double* __restrict__ pts,
                                                     const double* __restrict__ w, double nu, int a, int b,
                                                     bool want_res, double acc[16], double Ra[4], const TimeTerm& tt,
                                                     const ViscosityLaw& vl) {
    const int32_t nd[4] = {tv.x, tv.y, tv.z, tv.w};
    double X[4][3], W[4][4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const double* pp = pts + 3 * (int64_t)nd[v];
        X[v][0] = pp[0]; X[v][1] = pp[1]; X[v][2] = pp[2];
        const double2* wp = reinterpret_cast<const double2*>(w + 4 * (int64_t)nd[v]);
        const double2 w0 = wp[0], w1 = wp[1];
        W[v][0] = w0.x; W[v][1] = w0.y; W[v][2] = w1.x; W[v][3] = w1.y;
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
    double gu[3][3], gp[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        gp[j] = W[0][3] * g[0][j] + W[1][3] * g[1][j] + W[2][3] * g[2][j] + W[3][3] * g[3][j];
#pragma unroll
        for (int i = 0; i < 3; ++i) gu[i][j] = W[0][i] * g[0][j] + W[1][i] * g[1][j] + W[2][i] * g[2][j] + W[3][i] * g[3][j];
    }
    const double divu = gu[0][0] + gu[1][1] + gu[2][2];
    const double wd = fabs(det) * (1.0 / 24.0);
    const double itrG = 1.0 / trG;
    // viscosity law: nu_e and nu' = d nu_e / d s once per contribution
    double nu_t = nu, dnu = 0.0;
    if constexpr (VL) carreau(vl, nu, shear_rate2(gu), nu_t, dnu);
    // the part of tau^-2 that does not depend on the point: theta (time term) + C_I nu^2 G:G
    const double m0 = (TT ? tt.theta : 0.0) + 36.0 * nu_t * nu_t * GG;
    // time term: the nodal u_t = sigma u + d once, interpolated per point below (one more 3-vector gather per vertex)
    double UT[TT ? 4 : 1][3];
    if constexpr (TT) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const double* dp = tt.d + 4 * (int64_t)nd[v];
            const double2 d01 = *reinterpret_cast<const double2*>(dp);
            UT[v][0] = tt.sigma * W[v][0] + d01.x;
            UT[v][1] = tt.sigma * W[v][1] + d01.y;
            UT[v][2] = tt.sigma * W[v][2] + dp[2];
        }
    }
    const double sg = TT ? tt.sigma : 0.0;
    // runtime-indexed rows of g: select with predication (keeps everything in registers)
    double ga[3], gb[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        ga[j] = a == 0 ? g[0][j] : (a == 1 ? g[1][j] : (a == 2 ? g[2][j] : g[3][j]));
        gb[j] = b == 0 ? g[0][j] : (b == 1 ? g[1][j] : (b == 2 ? g[2][j] : g[3][j]));
    }
    const double gab = ga[0] * gb[0] + ga[1] * gb[1] + ga[2] * gb[2];
    double guga[3], visc[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        visc[j] = gu[j][0] * ga[0] + gu[j][1] * ga[1] + gu[j][2] * ga[2];                   // (grad u) g_a
        guga[j] = corrected ? (ga[0] * gu[0][j] + ga[1] * gu[1][j] + ga[2] * gu[2][j]) : visc[j];
    }
    // law: eps g_a, and kb = 4 C_I nu_e nu' G:G eps g_b carrying d(nu_e) into d tau and d nu_LSIC; the viscous Galerkin
    // term 2 nu_e eps g_a replaces nu (grad u) g_a; its derivative's point-independent part goes in once, up front
    double kb[VL ? 3 : 1];
    if constexpr (VL) {
        double ea[3], eb[3];
        eps_apply(gu, ga, ea);
        eps_apply(gu, gb, eb);
        const double vol = 4.0 * wd, c1 = vol * nu_t, c2 = 8.0 * vol * dnu, kap = 4.0 * 36.0 * nu_t * dnu * GG;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[4 * i + j] += c1 * gb[i] * ga[j] + c2 * ea[i] * eb[j];
            visc[i] = 2.0 * ea[i];
            kb[i] = kap * eb[i];
        }
    }
    // viscosity field (nu = the cell's nu_t, handed over by the caller): 2 nu_t eps g_a likewise, nu_t held fixed
    if constexpr (EV) {
        double ea[3];
        eps_apply(gu, ga, ea);
        const double c1 = 4.0 * wd * nu_t;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[4 * i + j] += c1 * gb[i] * ga[j];
            visc[i] = 2.0 * ea[i];
        }
    }
    // the quadrature weight wd is folded into the per-point coefficients, so every term lands directly in the
    // caller's accumulators (no per-contribution block)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double u[3] = {0.0, 0.0, 0.0}, p = 0.0;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const double ph = phi_q(q, v);
            u[0] += ph * W[v][0]; u[1] += ph * W[v][1]; u[2] += ph * W[v][2]; p += ph * W[v][3];
        }
        const double pa = phi_q(q, a), pb = phi_q(q, b);
        double Gu[3], conv[3], r[3], uGu = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            Gu[i] = G[i][0] * u[0] + G[i][1] * u[1] + G[i][2] * u[2];
            uGu += u[i] * Gu[i];
            conv[i] = gu[i][0] * u[0] + gu[i][1] * u[1] + gu[i][2] * u[2];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j)
            r[j] = (corrected ? conv[j] : (gu[0][j] * u[0] + gu[1][j] * u[1] + gu[2][j] * u[2])) + gp[j];
        double ut[3] = {0.0, 0.0, 0.0};
        if constexpr (TT) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const double ph = phi_q(q, v);
                ut[0] += ph * UT[v][0]; ut[1] += ph * UT[v][1]; ut[2] += ph * UT[v][2];
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) r[j] += ut[j];           // res_M gains u_t
        }
        // tau = m^-1/2, nu_LSIC = 1/(trG tau) = m tau / trG: one rsqrt per point, no divisions
        const double mq = uGu + m0;
        const double tau = rsqrt(mq);
        const double nuL = mq * tau * itrG;
        const double sa = r[0] * ga[0] + r[1] * ga[1] + r[2] * ga[2];
        const double ugb = u[0] * gb[0] + u[1] * gb[1] + u[2] * gb[2];
        const double uga = u[0] * ga[0] + u[1] * ga[1] + u[2] * ga[2];
        const double tw = wd * tau;                            // weighted tau
        const double t3w = tw * tau * tau;
        const double wpb = wd * pb, wpa = wd * pa;
        double cu[3], cg[3];                                   // both carry the weight
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double dtau = -t3w * pb * Gu[j];
            double dnuL = (tw * itrG) * pb * Gu[j];
            if constexpr (VL) {
                dtau -= t3w * kb[j];
                dnuL += (tw * itrG) * kb[j];
            }
            cg[j] = dnuL * divu + (wd * nuL) * gb[j];
            cu[j] = corrected ? dtau : dtau * sa + tw * (u[j] * gab + pb * guga[j]);
            if constexpr (TT && !corrected) cu[j] += (tw * sg * pb) * ga[j];               // d(u_t.g_a)
        }
        if (!corrected) {
            double A1 = wpa * ugb + (wd * nu_t) * gab + tw * sa * pb;
            if constexpr (TT) A1 += sg * wpa * pb;                                         // mass
            const double ppw = wpa * pb, tgw = tw * gab;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[4 * i + j] += ppw * gu[i][j] + u[i] * cu[j] + ga[i] * cg[j];
                acc[5 * i] += A1;
                acc[4 * i + 3] += tgw * u[i] - wpb * ga[i];
                acc[12 + i] += wpa * gb[i] + cu[i];
            }
            acc[15] += tgw;
        } else {
            double A1 = wpa * ugb + (wd * nu_t) * gab + tw * uga * ugb;
            const double cgu = wpa * pb + tw * uga * pb;       // coefficient of gu[i][j]
            if constexpr (TT) A1 += sg * cgu;                   // mass + SUPG of u_t
            const double mp = TT ? tw * sg * pb : 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    acc[4 * i + j] += cgu * gu[i][j] + (cu[j] * uga + tw * pb * ga[j]) * r[i] + ga[i] * cg[j];
                acc[5 * i] += A1;
                acc[4 * i + 3] += tw * uga * gb[i] - wpb * ga[i];
                acc[12 + i] += wpa * gb[i] + cu[i] * sa + tw * (ugb * ga[i] + pb * guga[i]);
                if constexpr (TT) acc[12 + i] += mp * ga[i];
            }
            acc[15] += tw * gab;
        }
        if (want_res) {
#pragma unroll
            for (int i = 0; i < 3; ++i)
                Ra[i] += wpa * conv[i] + (wd * nu_t) * visc[i] - (wd * p) * ga[i] +
                         (corrected ? tw * uga * r[i] : tw * u[i] * sa) + (wd * nuL) * divu * ga[i];
            Ra[3] += wpa * divu + tw * sa;
            if constexpr (TT) {
#pragma unroll
                for (int i = 0; i < 3; ++i) Ra[i] += wpa * ut[i];
            }
        }
    }
}

// Stokes form (:160-172): block (a,b) of the constant element matrix and, for the diagonal kernel, row a of
// A0 w (w = the Dirichlet data extended by zero: the lifting term of the right-hand side, :65 with x = 0).
__device__ __forceinline__ void tet_block_accumulate_stokes(const int4 tv, const double* __restrict__ pts,
                                                            const double* __restrict__ w, int a, int b, bool want_res,
                                                            double acc[16], double Ra[4]) {
    const int32_t nd[4] = {tv.x, tv.y, tv.z, tv.w};
    double X[4][3];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const double* pp = pts + 3 * (int64_t)nd[v];
        X[v][0] = pp[0]; X[v][1] = pp[1]; X[v][2] = pp[2];
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
    double h2 = 0.0;                                   // CellDiameter^2 (:168): longest edge
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int u = v + 1; u < 4; ++u) {
            const double d0 = X[u][0] - X[v][0], d1 = X[u][1] - X[v][1], d2 = X[u][2] - X[v][2];
            h2 = fmax(h2, d0 * d0 + d1 * d1 + d2 * d2);
        }
    const double wd = fabs(det) * (1.0 / 24.0), vol = 4.0 * wd, muT = 0.2 * h2;       // :169
    double ga[3], gb[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        ga[j] = a == 0 ? g[0][j] : (a == 1 ? g[1][j] : (a == 2 ? g[2][j] : g[3][j]));
        gb[j] = b == 0 ? g[0][j] : (b == 1 ? g[1][j] : (b == 2 ? g[2][j] : g[3][j]));
    }
    const double gab = ga[0] * gb[0] + ga[1] * gb[1] + ga[2] * gb[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        acc[5 * i] += vol * gab;                        // (grad u, grad v)
        acc[4 * i + 3] += -wd * ga[i];                  // -(p, div v)
        acc[12 + i] += wd * gb[i];                      // +(div u, q)
    }
    acc[15] += muT * vol * gab;                         // mu_T (grad p, grad q)
    if (want_res) {
        double gu[3][3], gp[3], psum = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            gp[i] = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) gu[i][j] = 0.0;
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const double* wv = w + 4 * (int64_t)nd[v];
            psum += wv[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                gp[j] += wv[3] * g[v][j];
#pragma unroll
                for (int i = 0; i < 3; ++i) gu[i][j] += wv[i] * g[v][j];
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
            Ra[i] += vol * (gu[i][0] * ga[0] + gu[i][1] * ga[1] + gu[i][2] * ga[2]) - wd * ga[i] * psum;
        Ra[3] += wd * (gu[0][0] + gu[1][1] + gu[2][2]) + muT * vol * (gp[0] * ga[0] + gp[1] * ga[1] + gp[2] * ga[2]);
    }
}

// ============================================================================
// 2-D triangle P1-P1 variants (handle created by sns_create_2d).  Same node-blocked layout [ux,uy,uz,p]
// (uz is a homogeneous Dirichlet dof: identity row), tets[] holds 3 vertex ids per cell in a stride of 4.
//   * Stokes   nu_s (grad u, grad v) - (p, div v) + (div u, q) + beta h^2 (grad p, grad q)
//       DFG_2D_Validation.py:107-117 (nu_s = 1, beta = 0.2), LidDrivenNavierStokesFlow.py:96-109 (nu, 1/(12 nu))
//   * NS with the h-based Tezduyar UGN parameters, LidDrivenNavierStokesFlow.py:123-143 ==
//       DFG_2D_Validation.py:141-163:  tau_SUPG = (inv1 + (4 nu / h^2)^2)^-1/2, inv1 = |u| <= 1e-8 ? 0 : (2|u|/h)^2,
//       tau_LSIC = h/2 |u| z, z = Re_UGN <= 3 ? Re_UGN/3 : 1, Re_UGN = |u| h / (2 nu); convection and SUPG test
//       function are the consistent (u.grad)(.) there (dot(u, nabla_grad(.))), and the exact Gateaux derivative
//       differentiates both taus (each branch of the conditionals separately, as ufl.derivative does).
// dx(degree 2) on a triangle: 3-point rule (1/6,1/6), (1/6,2/3), (2/3,1/6), weights 1/6.
// ============================================================================
#define T13 0.33333333333333333
#define T16 0.16666666666666666
#define T23 0.66666666666666663

// phi_v at quadrature point q: the vertex that carries 2/3 is 0, 2, 1 for q = 0, 1, 2
__device__ __forceinline__ double phi_q2(int q, int v) { return v == ((3 - q) % 3) ? T23 : T16; }

struct TriGeom {
    double g[3][2];     // grad phi_v
    double wd;          // |det J| / 6  (= quadrature weight x |det J|)
    double h2;          // CellDiameter^2
};
__device__ __forceinline__ void tri_geometry(const int4 tv, const double* __restrict__ pts, TriGeom& T) {
    const int32_t nd[3] = {tv.x, tv.y, tv.z};
    double X[3][2];
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const double* pp = pts + 3 * (int64_t)nd[v];
        X[v][0] = pp[0]; X[v][1] = pp[1];
    }
    const double J00 = X[1][0] - X[0][0], J01 = X[2][0] - X[0][0];
    const double J10 = X[1][1] - X[0][1], J11 = X[2][1] - X[0][1];
    const double det = J00 * J11 - J01 * J10;
    const double id = 1.0 / det;
    // K = J^-1, K[k][j] = dX_k / dx_j ; grad phi_1 = K[0][:], grad phi_2 = K[1][:]
    T.g[1][0] = J11 * id;  T.g[1][1] = -J01 * id;
    T.g[2][0] = -J10 * id; T.g[2][1] = J00 * id;
    T.g[0][0] = -(T.g[1][0] + T.g[2][0]);
    T.g[0][1] = -(T.g[1][1] + T.g[2][1]);
    T.wd = fabs(det) * T16;
    double h2 = 0.0;
#pragma unroll
    for (int v = 0; v < 3; ++v)
#pragma unroll
        for (int u = v + 1; u < 3; ++u) {
            const double d0 = X[u][0] - X[v][0], d1 = X[u][1] - X[v][1];
            h2 = fmax(h2, d0 * d0 + d1 * d1);
        }
    T.h2 = h2;
}
__device__ __forceinline__ void tri_state(const int4 tv, const double* __restrict__ w, double W[3][3]) {
    const int32_t nd[3] = {tv.x, tv.y, tv.z};
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const double2* wp = reinterpret_cast<const double2*>(w + 4 * (int64_t)nd[v]);
        const double2 w0 = wp[0], w1 = wp[1];
        W[v][0] = w0.x; W[v][1] = w0.y; W[v][2] = w1.y;       // ux, uy, p
    }
}

// per-point UGN scalars at velocity u (h, h2 of the cell): tau_SUPG, tau_LSIC and the coefficients c with
// d tau = c_tau (u . du), d tau_LSIC = c_L (u . du)
__device__ __forceinline__ void ugn_taus(const double u[2], double h, double h2, double nu, double& tau, double& ctau,
                                         double& tauL, double& cL) {
    const double uu = u[0] * u[0] + u[1] * u[1];
    const double un = sqrt(uu);
    const bool slow = un <= 1e-8;                                  // conditional(le(u_norm, 1e-8), 0, .)
    const double c4 = 4.0 / h2;
    const double i3 = 4.0 * nu / h2;                               // 1 / tau_SUNG3
    const double m = (slow ? 0.0 : c4 * uu) + i3 * i3;
    tau = rsqrt(m);
    ctau = slow ? 0.0 : -tau * tau * tau * c4;
    const double ReU = un * h / (2.0 * nu);
    if (ReU <= 3.0) {                                              // z = Re_UGN / 3
        tauL = 0.5 * h * un * (ReU * T13);
        cL = h2 / (6.0 * nu);
    } else {                                                       // z = 1
        tauL = 0.5 * h * un;
        cL = 0.5 * h / un;
    }
}

__device__ __forceinline__ void tri_block_accumulate_ugn(const int4 tv, const double* __restrict__ pts,
                                                         const double* __restrict__ w, double nu, int a, int b,
                                                         bool want_res, double acc[16], double Ra[4]) {
    TriGeom T;
    tri_geometry(tv, pts, T);
    double W[3][3];
    tri_state(tv, w, W);
    double gu[2][2], gp[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        gp[j] = W[0][2] * T.g[0][j] + W[1][2] * T.g[1][j] + W[2][2] * T.g[2][j];
#pragma unroll
        for (int i = 0; i < 2; ++i) gu[i][j] = W[0][i] * T.g[0][j] + W[1][i] * T.g[1][j] + W[2][i] * T.g[2][j];
    }
    const double divu = gu[0][0] + gu[1][1];
    const double wd = T.wd, h2 = T.h2, h = sqrt(h2);
    double ga[2], gb[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        ga[j] = a == 0 ? T.g[0][j] : (a == 1 ? T.g[1][j] : T.g[2][j]);
        gb[j] = b == 0 ? T.g[0][j] : (b == 1 ? T.g[1][j] : T.g[2][j]);
    }
    const double gab = ga[0] * gb[0] + ga[1] * gb[1];
    const double visc[2] = {gu[0][0] * ga[0] + gu[0][1] * ga[1], gu[1][0] * ga[0] + gu[1][1] * ga[1]};   // (grad u) g_a
    const double guga[2] = {ga[0] * gu[0][0] + ga[1] * gu[1][0], ga[0] * gu[0][1] + ga[1] * gu[1][1]};   // g_a^T (grad u)
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        double u[2] = {0.0, 0.0}, p = 0.0;
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const double ph = phi_q2(q, v);
            u[0] += ph * W[v][0]; u[1] += ph * W[v][1]; p += ph * W[v][2];
        }
        const double pa = phi_q2(q, a), pb = phi_q2(q, b);
        double tau, ctau, tauL, cL;
        ugn_taus(u, h, h2, nu, tau, ctau, tauL, cL);
        const double conv[2] = {gu[0][0] * u[0] + gu[0][1] * u[1], gu[1][0] * u[0] + gu[1][1] * u[1]};   // (u.grad)u
        const double r[2] = {conv[0] + gp[0], conv[1] + gp[1]};                                         // res
        const double sa = r[0] * ga[0] + r[1] * ga[1];
        const double ugb = u[0] * gb[0] + u[1] * gb[1];
        const double uga = u[0] * ga[0] + u[1] * ga[1];
        const double tw = wd * tau, wpa = wd * pa, wpb = wd * pb;
        double cu[2], cg[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            cu[j] = wd * ctau * pb * u[j];                                     // weighted d tau / d u_(b,j)
            cg[j] = wd * (cL * pb * u[j] * divu + tauL * gb[j]);               // weighted d (tau_LSIC div u)
        }
        const double A1 = wpa * ugb + (wd * nu) * gab + tw * uga * ugb;
        const double cgu = wpa * pb + tw * uga * pb;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[4 * i + j] += cgu * gu[i][j] + (cu[j] * uga + tw * pb * ga[j]) * r[i] + ga[i] * cg[j];
            acc[5 * i] += A1;
            acc[4 * i + 3] += tw * uga * gb[i] - wpb * ga[i];
            acc[12 + i] += wpa * gb[i] + cu[i] * sa + tw * (ugb * ga[i] + pb * guga[i]);
        }
        acc[15] += tw * gab;
        if (want_res) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
                Ra[i] += wpa * conv[i] + (wd * nu) * visc[i] - (wd * p) * ga[i] + tw * uga * r[i] +
                         (wd * tauL) * divu * ga[i];
            Ra[3] += wpa * divu + tw * sa;
        }
    }
}

__device__ __forceinline__ void tri_block_accumulate_stokes(const int4 tv, const double* __restrict__ pts,
                                                            const double* __restrict__ w, double nu_s, double beta,
                                                            int a, int b, bool want_res, double acc[16], double Ra[4]) {
    TriGeom T;
    tri_geometry(tv, pts, T);
    const double wd = T.wd, vol = 3.0 * wd, muT = beta * T.h2;
    double ga[2], gb[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        ga[j] = a == 0 ? T.g[0][j] : (a == 1 ? T.g[1][j] : T.g[2][j]);
        gb[j] = b == 0 ? T.g[0][j] : (b == 1 ? T.g[1][j] : T.g[2][j]);
    }
    const double gab = ga[0] * gb[0] + ga[1] * gb[1];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        acc[5 * i] += nu_s * vol * gab;                 // nu_s (grad u, grad v)
        acc[4 * i + 3] += -wd * ga[i];                  // -(p, div v), int phi_b = vol / 3 = wd
        acc[12 + i] += wd * gb[i];                      // +(div u, q)
    }
    acc[15] += muT * vol * gab;
    if (want_res) {
        double W[3][3];
        tri_state(tv, w, W);
        double gu[2][2], gp[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            gp[j] = W[0][2] * T.g[0][j] + W[1][2] * T.g[1][j] + W[2][2] * T.g[2][j];
#pragma unroll
            for (int i = 0; i < 2; ++i) gu[i][j] = W[0][i] * T.g[0][j] + W[1][i] * T.g[1][j] + W[2][i] * T.g[2][j];
        }
        const double psum = W[0][2] + W[1][2] + W[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i) Ra[i] += nu_s * vol * (gu[i][0] * ga[0] + gu[i][1] * ga[1]) - wd * ga[i] * psum;
        Ra[3] += wd * (gu[0][0] + gu[1][1]) + muT * vol * (gp[0] * ga[0] + gp[1] * ga[1]);
    }
}

// one interface for the four forms (aux: Stokes 2-D pressure-stabilisation coefficient beta; nu: 1/Re, or the
// Stokes 2-D viscosity)
template <int FORM, bool corrected, bool TT, bool VL, bool EV>
__device__ __forceinline__ void block_accumulate(const int4 tv, const double* __restrict__ pts,
                                                 const double* __restrict__ w, double nu, double aux, int a, int b,
                                                 bool want_res, double acc[16], double Ra[4], const TimeTerm& tt,
                                                 const ViscosityLaw& vl) {
    static_assert(!TT || FORM == SNS_FORM_NS, "the time term exists in the 3-D NS form only");
    static_assert(!VL || (FORM == SNS_FORM_NS && !TT), "the viscosity law exists in the steady 3-D NS form only");
    static_assert(!EV || (FORM == SNS_FORM_NS && TT && !VL), "the viscosity field is a variant of the 3-D NS form with the time term");
    if constexpr (FORM == SNS_FORM_STOKES) tet_block_accumulate_stokes(tv, pts, w, a, b, want_res, acc, Ra);
    else if constexpr (FORM == SNS_FORM_NS) tet_block_accumulate<corrected, TT, VL, EV>(tv, pts, w, nu, a, b, want_res, acc, Ra, tt, vl);
    else if constexpr (FORM == SNS_FORM_STOKES_2D) tri_block_accumulate_stokes(tv, pts, w, nu, aux, a, b, want_res, acc, Ra);
    else tri_block_accumulate_ugn(tv, pts, w, nu, a, b, want_res, acc, Ra);
}
constexpr bool form_is_linear(int form) { return form == SNS_FORM_STOKES || form == SNS_FORM_STOKES_2D; }

}  // namespace sns
