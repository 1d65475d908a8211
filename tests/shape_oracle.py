"""CPU oracle of the shape gradient lam . dR_raw/dX (plain helper module of the shape tests, not a conftest).

The project's CPU forms are differentiable in the vertex coordinates, so the oracle is autograd over them, with no closed
form shared with the HIP kernels:

    3-D  ``tests/ns3d_oracle.residual`` with X a tensor that requires grad (sigma = theta = 0, d = 0 is the
         steady form; ``forms_literal.VARIANT`` and ``corrected_convection`` apply as there),
    2-D  ``oracle.forms2d.ugn_residual_one`` under ``torch.func.jacrev(..., argnums=0)``.

A cell's contribution is d(lam_e . F_e)/dX_e; the global gradient scatter-adds it per node.  Dof vectors are the
product's: 4 per node [ux, uy, uz, p] (uz unused in 2-D); gradients are (n_nodes, 3) with a zero z column in 2-D.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import forms2d as F2

import ns3d_oracle as NS

_T = torch.float64
_C3 = [0, 1, 3]


# ---- 3-D -------------------------------------------------------------------------------------------------------------
def tet_cell_residuals(X, W, D, Re, sigma=0.0, theta=0.0, corrected_convection=False):
    """(E,16) element residuals as numpy; X (E,4,3), W (E,16), D (E,4,3)."""
    Wt = torch.as_tensor(np.asarray(W, dtype=np.float64), dtype=_T)
    return NS.residual(np.asarray(X, dtype=np.float64), Wt, Re, d=D, sigma=sigma, theta=theta,
                       corrected_convection=corrected_convection).numpy()


def tet_cell_gradients(X, W, Lam, D, Re, sigma=0.0, theta=0.0, corrected_convection=False):
    """(E,4,3): d(Lam_e . F_e)/dX_e of every tet by reverse mode through the oracle residual."""
    Xt = torch.as_tensor(np.asarray(X, dtype=np.float64), dtype=_T).clone().requires_grad_(True)
    Wt = torch.as_tensor(np.asarray(W, dtype=np.float64), dtype=_T)
    Lt = torch.as_tensor(np.asarray(Lam, dtype=np.float64), dtype=_T)
    F = NS.residual(Xt, Wt, Re, d=D, sigma=sigma, theta=theta, corrected_convection=corrected_convection)
    (g,) = torch.autograd.grad((F * Lt).sum(), Xt)          # a tet's residual depends on its own vertices only
    return g.numpy()


def _cells3(points, tets, w, lam, d):
    W4 = np.asarray(w, dtype=np.float64).reshape(-1, 4)
    L4 = np.asarray(lam, dtype=np.float64).reshape(-1, 4)
    D = np.zeros((len(points), 3)) if d is None else np.asarray(d, dtype=np.float64).reshape(-1, 4)[:, :3]
    return points[tets], W4[tets].reshape(len(tets), 16), L4[tets].reshape(len(tets), 16), D[tets]


def raw_residual_3d(points, tets, w, Re, d=None, sigma=0.0, theta=0.0, corrected_convection=False):
    """Unconstrained global residual (4 n,)."""
    X, W, _, D = _cells3(points, tets, w, w, d)
    Fe = tet_cell_residuals(X, W, D, Re, sigma, theta, corrected_convection)
    F = np.zeros(4 * len(points))
    np.add.at(F, (4 * tets.astype(np.int64)[:, :, None] + np.arange(4)[None, None, :]).ravel(), Fe.ravel())
    return F


def gradient_3d(points, tets, w, lam, Re, d=None, sigma=0.0, theta=0.0, corrected_convection=False):
    """(n,3): sum_e d(lam_e . F_e)/dX scatter-added per node."""
    X, W, L, D = _cells3(points, tets, w, lam, d)
    ge = tet_cell_gradients(X, W, L, D, Re, sigma, theta, corrected_convection)
    out = np.zeros((len(points), 3))
    np.add.at(out, tets.ravel(), ge.reshape(-1, 3))
    return out


# ---- 2-D -------------------------------------------------------------------------------------------------------------
def tri_cell_residuals(X, W, nu):
    """(E,9) UGN element residuals; X (E,3,2), W (E,9) = [ux,uy,p]*3."""
    f = torch.func.vmap(lambda x, w: F2.ugn_residual_one(x, w, nu))
    return f(torch.as_tensor(np.asarray(X, dtype=np.float64), dtype=_T),
             torch.as_tensor(np.asarray(W, dtype=np.float64), dtype=_T)).numpy()


def tri_cell_gradients(X, W, Lam, nu, chunk=20000):
    """(E,3,2): Lam_e . dF_e/dX_e with dF_e/dX_e = jacrev of ``ugn_residual_one`` in its first argument."""
    fj = torch.func.vmap(torch.func.jacrev(lambda x, w: F2.ugn_residual_one(x, w, nu), argnums=0))
    out = []
    for s in range(0, len(X), chunk):
        Jx = fj(torch.as_tensor(np.asarray(X[s:s + chunk], dtype=np.float64), dtype=_T),
                torch.as_tensor(np.asarray(W[s:s + chunk], dtype=np.float64), dtype=_T))           # (E,9,3,2)
        out.append(torch.einsum("ei,eiaj->eaj", torch.as_tensor(np.asarray(Lam[s:s + chunk], dtype=np.float64), dtype=_T),
                                Jx).numpy())
    return np.concatenate(out)


def _cells2(points, tris, w, lam):
    W4 = np.asarray(w, dtype=np.float64).reshape(-1, 4)
    L4 = np.asarray(lam, dtype=np.float64).reshape(-1, 4)
    return points[tris][:, :, :2], W4[tris][:, :, _C3].reshape(len(tris), 9), L4[tris][:, :, _C3].reshape(len(tris), 9)


def raw_residual_2d(points, tris, w, nu):
    X, W, _ = _cells2(points, tris, w, w)
    Fe = tri_cell_residuals(X, W, nu)
    F = np.zeros(4 * len(points))
    np.add.at(F, (4 * tris.astype(np.int64)[:, :, None] + np.array(_C3)[None, None, :]).ravel(), Fe.ravel())
    return F


def gradient_2d(points, tris, w, lam, nu):
    """(n,3) with a zero z column."""
    X, W, L = _cells2(points, tris, w, lam)
    ge = tri_cell_gradients(X, W, L, nu)
    out = np.zeros((len(points), 3))
    np.add.at(out[:, :2], tris.ravel(), ge.reshape(-1, 2))
    return out


# ---- random disconnected cells (every node belongs to one cell) --------------------------------------------------------
def radius_ratio(X):
    """dim * inradius / circumradius of simplices X (E, dim+1, dim): 1 for the regular simplex."""
    X = np.asarray(X, dtype=np.float64)
    dim = X.shape[2]
    A = X[:, 1:] - X[:, :1]
    vol = np.abs(np.linalg.det(A)) / (6.0 if dim == 3 else 2.0)
    # circumcentre: 2 A c = |a_i|^2
    c = np.linalg.solve(2.0 * A, (A * A).sum(axis=2)[:, :, None])[:, :, 0]
    R = np.linalg.norm(c, axis=1)
    area = 0.0
    for a in range(dim + 1):
        f = np.delete(X, a, axis=1)
        e = f[:, 1:] - f[:, :1]
        area = area + (0.5 * np.linalg.norm(np.cross(e[:, 0], e[:, 1]), axis=1) if dim == 3 else np.linalg.norm(e[:, 0], axis=1))
    return dim * (dim * vol / area) / R


def random_cells(n_cells, dim, seed, min_ratio=0.1):
    """``n_cells`` disconnected random simplices of radius ratio >= min_ratio: points (n_cells (dim+1), dim), cells
    (n_cells, dim+1) int32, state and lam as dof vectors (4 per node; uz = 0 in 2-D)."""
    rng = np.random.default_rng(seed)
    keep = []
    while sum(len(k) for k in keep) < n_cells:
        X = rng.uniform(0.0, 1.0, (4 * n_cells, dim + 1, dim))
        keep.append(X[radius_ratio(X) >= min_ratio])
    X = np.concatenate(keep)[:n_cells]                        # (the cells overlap in space; they share no node)
    pts = X.reshape(-1, dim)
    cells = np.arange(n_cells * (dim + 1), dtype=np.int32).reshape(n_cells, dim + 1)
    w = rng.standard_normal((len(pts), 4))
    lam = rng.standard_normal((len(pts), 4))
    if dim == 2:
        w[:, 2] = 0.0
        lam[:, 2] = 0.0
    return pts, cells, w.ravel(), lam.ravel()
