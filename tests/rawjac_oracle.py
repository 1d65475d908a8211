"""CPU oracle of the raw Jacobian J0 = dR_raw/dw and of what is built on it (plain helper module of tests/test_host_rawjac.py and
tests/test_gpu_rawjac.py, not a conftest).

J0 is the unconstrained Jacobian the other oracles already return and then constrain: ``ns3d_oracle.raw`` for the 3-D NS form
with every form keyword (autograd of the literal form), ``oracle.forms2d.ugn_elements`` + ``_coo`` for the 2-D UGN form.  On
top: the exact discrete gradient of a functional with respect to the Dirichlet values, by sparse LU; the moments of the raw
residual (the residual-based force); a BDF loop whose Dirichlet values move with t.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

from oracle import forms2d as F2

import ns3d_oracle as NS


def raw_jacobian(points, tets, w, Re, **form):
    """J0(w) of the 3-D NS form as CSR (4 n x 4 n): no lifting, no Dirichlet rule.  form: the keywords of ``ns3d_oracle``."""
    return sp.csr_matrix(NS.raw(points, tets, w, Re, **form)[1])


def raw_residual(points, tets, w, Re, **form):
    return NS.raw(points, tets, w, Re, want_jac=False, **form)[0]


def raw_jacobian_2d(points, tris, w, nu):
    """J0(w) of the 2-D UGN form in the 4-dofs-per-node layout: the u_z rows and columns are empty."""
    _, Je = F2.ugn_elements(points, tris, w, nu)
    return sp.csr_matrix(F2._coo(tris, Je, 4 * len(points)))


def ugn_branches(points, tris, w, nu):
    """How many quadrature points of the state take each branch of the UGN form's conditionals: (at rest: |u| <= 1e-8,
    Re_UGN <= 3 with |u| > 1e-8, Re_UGN > 3), and the number of triangles whose three points are all at rest."""
    W = np.asarray(w, dtype=np.float64).reshape(-1, 4)
    rest = low = high = 0
    cells_at_rest = 0
    for t in np.asarray(tris):
        X = torch.as_tensor(np.asarray(points)[t][:, :2], dtype=torch.float64)
        _, _, h = F2._geometry(X)
        n_rest = 0
        for q in range(3):
            phi = F2._phi(torch.as_tensor(F2.QPTS[q], dtype=torch.float64)).numpy()
            un = float(np.linalg.norm(phi @ W[t][:, :2]))
            re = un * float(h) / (2.0 * nu)
            if un <= 1e-8:
                rest += 1
                n_rest += 1
            elif re <= 3.0:
                low += 1
            else:
                high += 1
        cells_at_rest += n_rest == 3
    return rest, low, high, cells_at_rest


def dirichlet_gradient(J0, mask, grad_J):
    """The exact discrete dJ/dg at a state that satisfies its data: grad_J[B] - J0[f,B]^T J_ff^-T grad_J[f] on the constrained
    dofs B, 0 on the free dofs f.  Returns (dJ/dg, lam): lam the adjoint vector of the constrained operator (lam_B = grad_J[B])."""
    B = np.asarray(mask).astype(bool)
    f = ~B
    J0 = sp.csr_matrix(J0)
    lam = np.zeros(len(B))
    lam[f] = spla.splu(sp.csc_matrix(J0[f][:, f].T)).solve(np.asarray(grad_J, dtype=np.float64)[f])
    lam[B] = np.asarray(grad_J)[B]
    out = np.zeros(len(B))
    out[B] = np.asarray(grad_J)[B] - J0[f][:, B].T @ lam[f]
    return out, lam


def moments(points, tets, w, Re, phi, **form):
    """sum_i phi_i R_raw(w)[4 i + c], c = 0..3 (sns_residual_moments); minus its first three entries is the reaction force."""
    return (raw_residual(points, tets, w, Re, **form).reshape(-1, 4) * np.asarray(phi)[:, None]).sum(axis=0)


def march_dirichlet(points, tets, mask, g_of_t, Re, w0, dt, n_steps, order, theta_coeff, **kw):
    """``ns3d_oracle.march`` with Dirichlet values that move: step n + 1 is taken with g((n + 1) dt).  Returns [w0, w1, ...]."""
    hist = [np.asarray(w0, dtype=np.float64).copy()]
    for n in range(n_steps):
        o = 1 if n == 0 else order
        x, _ = NS.step(points, tets, mask, g_of_t((n + 1) * dt), Re, hist[-1], hist[-2] if n > 0 else hist[-1], dt, o, theta_coeff, **kw)
        hist.append(x)
    return hist


def fd_band(J_of, delta):
    """Central differences D(delta), D(delta / 2) of s -> J_of(s) at 0, their Richardson value D* and the band of
    tests/test_gpu_adjoint.py: 4 |D(delta/2) - D(delta)| / 3 + 1e-7 |D*|.  Returns (D(delta), D(delta/2), D*, band)."""
    D = [(J_of(d) - J_of(-d)) / (2.0 * d) for d in (delta, 0.5 * delta)]
    Dstar = (4.0 * D[1] - D[0]) / 3.0
    return D[0], D[1], Dstar, 4.0 * abs(D[1] - D[0]) / 3.0 + 1e-7 * abs(Dstar)
