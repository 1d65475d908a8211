"""CPU oracle of the scalar-transport form (plain helper module of the scalar tests, not a conftest).

The reference transports nothing (it traces streamlines), so there is nothing to pin to: this is the literal restatement of the
form the library documents (include/sns.h, sns_scalar_system), written with explicit trial and test functions and batched over
tets.  For species k with the P1 velocity u of a state w:

    R_k(c; v) = int (sigma c + u.grad c - s_k)(v + tau_k u.grad v) + kappa_k grad c . grad v dx
    tau_k     = (theta + u.G u + C_I kappa_k^2 G:G)^(-1/2)       C_I = 36, G = K^T K (oracle/element.py)

with tau_k taken at each point of the 4-point degree-2 rule every integral uses.  On top: the global assembly of the four
species in the node-blocked layout [c0, c1, c2, c3] by the Dirichlet rule of ``oracle/assemble.py`` (rows and columns zeroed,
diagonal one, b -= A0[:, B] g, b_B = g), a sparse LU solve and the BDF recursion of ``solver.advance_scalars``.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import assemble as asm
from oracle import element as el

RULE2 = (el.PHI, np.full(4, el.QW))                 # (phi_a(x_q) [q, a], weights as fractions of |det J|)


def conical_rule(n: int = 5):
    """A rule on the reference tet exact to degree 2 n - 3 (collapsed Gauss-Legendre), in the format of ``RULE2``."""
    x, wx = np.polynomial.legendre.leggauss(n)
    x, wx = 0.5 * (x + 1.0), 0.5 * wx
    phi, wt = [], []
    for a, wa in zip(x, wx):
        for b, wb in zip(x, wx):
            for c, wc in zip(x, wx):
                X, Y, Z = a, b * (1.0 - a), c * (1.0 - a) * (1.0 - b)
                phi.append([1.0 - X - Y - Z, X, Y, Z])
                wt.append(wa * wb * wc * (1.0 - a) ** 2 * (1.0 - b))
    return np.array(phi), np.array(wt)


def element(X, U, kappa, sigma=0.0, theta=0.0, src=None, *, rule=RULE2, stabilised=True):
    """Element matrices A (E, 4, 4) [tet, test a, trial b] and source vectors S (E, 4) of ONE species.  X (E, 4, 3) vertices,
    U (E, 4, 3) nodal velocities, src (E, 4) nodal source or None.  ``stabilised=False``: the Galerkin part alone."""
    X, U = np.asarray(X, dtype=np.float64), np.asarray(U, dtype=np.float64)
    E = len(X)
    K, detJ, g = el.geometry(X)                                          # g[e, a, :] = grad phi_a
    G = np.einsum("eki,ekj->eij", K, K)
    GG = (G * G).sum(axis=(1, 2))
    A, S = np.zeros((E, 4, 4)), np.zeros((E, 4))
    PHI, WT = rule
    for phi, wt in zip(PHI, WT):
        dx = wt * detJ
        u = np.einsum("a,eai->ei", phi, U)
        tau = 1.0 / np.sqrt(theta + np.einsum("ei,eij,ej->e", u, G, u) + el.C_I * kappa * kappa * GG)
        if not stabilised:
            tau = np.zeros(E)
        s = np.zeros(E) if src is None else np.einsum("a,ea->e", phi, src)
        for a in range(4):                                               # test function v = phi_a
            v, gv = phi[a], g[:, a]
            test = v + tau * np.einsum("ei,ei->e", u, gv)
            S[:, a] += dx * s * test
            for b in range(4):                                           # trial function c = phi_b
                c, gc = phi[b], g[:, b]
                A[:, a, b] += dx * ((sigma * c + np.einsum("ei,ei->e", u, gc)) * test + kappa * np.einsum("ei,ei->e", gc, gv))
    return A, S


def raw(points, tets, w, kappa, sigma=0.0, theta=0.0, source=None):
    """Unconstrained operator A0 (CSR, 4 n x 4 n, block diagonal over the species) and source vector (4 n,).  kappa: four
    values; source: (n, 4) or None."""
    points, tets = np.asarray(points, dtype=np.float64), np.asarray(tets)
    n = len(points)
    U = np.asarray(w, dtype=np.float64).reshape(n, 4)[:, :3][tets]
    t64 = tets.astype(np.int64)
    rows, cols, vals = [], [], []
    b = np.zeros(4 * n)
    for k in range(4):
        src = None if source is None else np.asarray(source, dtype=np.float64).reshape(n, 4)[:, k][tets]
        A, S = element(points[tets], U, float(kappa[k]), sigma, theta, src)
        rows.append(np.repeat(4 * t64 + k, 4, axis=1).ravel())
        cols.append(np.tile(4 * t64 + k, (1, 4)).ravel())
        vals.append(A.reshape(-1))
        np.add.at(b, (4 * t64 + k).ravel(), S.reshape(-1))
    A0 = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(4 * n, 4 * n)).tocsr()
    return A0, b


def assemble(points, tets, w, kappa, cmask, cval, sigma=0.0, theta=0.0, source=None):
    """(A, b, A0): the constrained operator and right-hand side as sns_scalar_system leaves them, and the raw operator."""
    A0, b = raw(points, tets, w, kappa, sigma, theta, source)
    mask = np.asarray(cmask).ravel().astype(np.uint8)
    g = np.asarray(cval, dtype=np.float64).ravel()
    B = mask.astype(bool)
    b = b - A0[:, B] @ g[B]
    b[B] = g[B]
    return asm._apply_bc_matrix(A0, mask), b, A0


def solve(points, tets, w, kappa, cmask, cval, sigma=0.0, theta=0.0, source=None):
    """c (n, 4) by a sparse LU."""
    A, b, _ = assemble(points, tets, w, kappa, cmask, cval, sigma, theta, source)
    return spla.splu(A.tocsc()).solve(b).reshape(-1, 4)


def advance(points, tets, w, kappa, cmask, cval, c0, dt, n_steps, order=2, theta_coeff=4.0):
    """The BDF recursion of solver.advance_scalars (first step BDF1), one LU per step; c0 and the result (n, 4)."""
    c = np.asarray(c0, dtype=np.float64).reshape(-1, 4).copy()
    cprev = c.copy()
    for step in range(1, n_steps + 1):
        o = 1 if step == 1 else order
        hist = c / dt if o == 1 else (2.0 * c - 0.5 * cprev) / dt
        cn = solve(points, tets, w, kappa, cmask, cval, (1.0 if o == 1 else 1.5) / dt, theta_coeff / (dt * dt), hist)
        cprev, c = c, cn
    return c
