"""CPU oracle of the boundary terms (plain helper module of the boundary tests, not a conftest).

The reference has no facet integral, so there is nothing to pin to: this is the literal restatement of the forms the library
documents (include/sns.h, sns_set_boundary_flow / sns_set_boundary_scalar), written per facet in torch with the Jacobian by
autograd.  A boundary facet has vertices (i0, i1, i2), area |Gamma| and the outward unit normal n -- outward = away from the
fourth vertex of the tet that owns it.  The facets stay in the caller's vertex order here (the orientation is a sign on the
normal), so per-vertex data is indexed as the caller gave it.

    flow     R(w; v) += - int t.v ds - int beta (u.n)_- u.v ds          (u.n)_- = min(u.n, 0)
             t P1 per facet (F, 3, 3) [vertex][component]: exact by the facet mass matrix |Gamma|/12 (1 + delta_ab);
             beta (F,) by the 6-point degree-4 rule with positive weights (A1, W1, A2, W2 below, weights times |Gamma|)
    scalars  R_k(c; v) += int (alpha_k c_k - g_k) v ds                   alpha (F, 4), g P1 per facet (F, 3, 4)

On top: the drivers of ``ns3d_oracle`` with the flow terms as their ``extra=`` (the facet terms are part of the raw form: lifting
through their columns, rows of constrained dofs replaced), and ``scalar_oracle.raw`` with the Dirichlet rule of
``oracle/assemble.py`` for the scalars.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

from oracle import assemble as asm

import ns3d_oracle as NS
import scalar_oracle as SO

_T = torch.float64
A1, W1 = 0.445948490915965, 0.223381589678011
A2, W2 = 0.091576213509771, 0.109951743655322
QPTS = np.array([[1 - 2 * A1, A1, A1], [A1, 1 - 2 * A1, A1], [A1, A1, 1 - 2 * A1],
                 [1 - 2 * A2, A2, A2], [A2, 1 - 2 * A2, A2], [A2, A2, 1 - 2 * A2]])       # barycentric (phi_0, phi_1, phi_2)
QWTS = np.array([W1, W1, W1, W2, W2, W2])
MASS = (np.ones((3, 3)) + np.eye(3)) / 12.0                                                # facet mass matrix / |Gamma|


def facet_geometry(points, tets, facets, facet_tets):
    """(area (F,), n (F, 3)): n = the unit normal pointing away from the owner's fourth vertex."""
    points, facets = np.asarray(points, dtype=np.float64), np.asarray(facets, dtype=np.int64)
    tn = np.asarray(tets, dtype=np.int64)[np.asarray(facet_tets, dtype=np.int64)]
    P = points[facets]
    cr = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    opp = tn.sum(axis=1) - facets.sum(axis=1)
    cr = cr * np.sign(np.einsum("fi,fi->f", cr, P[:, 0] - points[opp]))[:, None]
    nrm = np.linalg.norm(cr, axis=1)
    return 0.5 * nrm, cr / nrm[:, None]


def flow_residual(area, n, U, t, beta):
    """(F, 9) facet residuals [vertex a][component c].  U (F, 3, 3) nodal velocities (torch fp64, may require grad); t (F, 3, 3)
    or None; beta (F,) or None."""
    area, n = torch.as_tensor(area, dtype=_T), torch.as_tensor(n, dtype=_T)
    R = torch.zeros(U.shape[0], 3, 3, dtype=_T)
    if t is not None:                                                    # - int t.v: v = phi_a e_c, t = sum_b t_b phi_b
        R = R - area[:, None, None] * torch.einsum("ab,fbc->fac", torch.as_tensor(MASS, dtype=_T), torch.as_tensor(np.array(t), dtype=_T))
    if beta is not None:
        beta = torch.as_tensor(beta, dtype=_T)
        for phi, wq in zip(QPTS, QWTS):
            phi = torch.as_tensor(phi, dtype=_T)
            u = torch.einsum("a,fac->fc", phi, U)
            un_minus = torch.clamp(torch.einsum("fc,fc->f", u, n), max=0.0)
            R = R - (beta * wq * area * un_minus)[:, None, None] * phi[None, :, None] * u[:, None, :]
    return R.reshape(-1, 9)


def flow_element(area, n, U, t, beta, want_jac=True):
    """numpy (R (F, 9), J (F, 9, 9) or None): J = dR/dU by autograd with t and beta held fixed -- the derivative of the branch
    each quadrature point takes."""
    Ut = torch.as_tensor(np.asarray(U, dtype=np.float64), dtype=_T).clone().requires_grad_(want_jac)
    R = flow_residual(area, n, Ut, t, beta)
    if not want_jac or not R.requires_grad:
        return R.detach().numpy(), (np.zeros((len(Ut), 9, 9)) if want_jac else None)
    seeds = torch.eye(9, dtype=_T)[:, None, :].expand(9, R.shape[0], 9)
    rows = torch.autograd.grad(R, Ut, grad_outputs=seeds, is_grads_batched=True)[0]
    return R.detach().numpy(), rows.reshape(9, -1, 9).permute(1, 0, 2).detach().numpy()


def _vel_dofs(facets):
    f = np.asarray(facets, dtype=np.int64)
    return (4 * f[:, :, None] + np.arange(3)[None, None, :]).reshape(len(f), 9)           # [vertex][component]


def flow_raw(points, tets, w, facets, facet_tets, t=None, beta=None, want_jac=True):
    """Unconstrained boundary residual (ndof,) and Jacobian (CSR or None) of the flow terms."""
    ndof = 4 * len(points)
    area, n = facet_geometry(points, tets, facets, facet_tets)
    dofs = _vel_dofs(facets)
    U = np.asarray(w, dtype=np.float64)[dofs].reshape(-1, 3, 3)
    Re, Je = flow_element(area, n, U, t, beta, want_jac)
    F = np.zeros(ndof)
    np.add.at(F, dofs.ravel(), Re.ravel())
    if not want_jac:
        return F, None
    rows = np.repeat(dofs, 9, axis=1).ravel()
    cols = np.tile(dofs, (1, 9)).ravel()
    return F, sp.coo_matrix((Je.ravel(), (rows, cols)), shape=(ndof, ndof)).tocsr()


def _facet_terms(points, tets, facets, facet_tets, kw):
    """Takes t= and beta= out of kw: the flow terms as the ``extra=`` of the shared drivers."""
    t, beta = kw.pop("t", None), kw.pop("beta", None)
    return lambda w, want_jac: flow_raw(points, tets, w, facets, facet_tets, t, beta, want_jac)


def raw(points, tets, w, Re, facets, facet_tets, **kw):
    """Volume (``ns3d_oracle.raw``, its keywords) plus boundary (t=, beta=): the raw residual and Jacobian of the whole form."""
    extra = _facet_terms(points, tets, facets, facet_tets, kw)
    return NS.raw(points, tets, w, Re, extra=extra, **kw)


def assemble(points, tets, w, Re, mask, g, facets, facet_tets, **kw):
    """(J, F) of ``ns3d_oracle.assemble``: the Dirichlet rule applied to the whole raw form."""
    extra = _facet_terms(points, tets, facets, facet_tets, kw)
    return NS.assemble(points, tets, w, Re, mask, g, extra=extra, **kw)


def newton(points, tets, mask, g, Re, w0, facets, facet_tets, **kw):
    """``ns3d_oracle.newton`` with the boundary terms.  Returns (w, its)."""
    extra = _facet_terms(points, tets, facets, facet_tets, kw)
    return NS.newton(points, tets, mask, g, Re, w0, extra=extra, **kw)


def step(points, tets, mask, g, Re, w, wprev, dt, order, theta_coeff, facets, facet_tets, **kw):
    """One implicit BDF step (``ns3d_oracle.step``) with the boundary terms.  Returns (w, its)."""
    extra = _facet_terms(points, tets, facets, facet_tets, kw)
    return NS.step(points, tets, mask, g, Re, w, wprev, dt, order, theta_coeff, extra=extra, **kw)


# ---- scalars --------------------------------------------------------------------------------------------------------------------
def scalar_raw(points, tets, facets, facet_tets, alpha=None, g=None):
    """(A (CSR, 4 n x 4 n, block diagonal over the species), b (4 n,)) of the facet terms: alpha M_Gamma and int g v.
    alpha (F, 4) or None, g (F, 3, 4) or None."""
    n4 = 4 * len(points)
    f = np.asarray(facets, dtype=np.int64)
    area, _ = facet_geometry(points, tets, f, facet_tets)
    M = area[:, None, None] * MASS[None]                                 # (F, 3, 3)
    b = np.zeros(n4)
    rows, cols, vals = [], [], []
    for k in range(4):
        dof = 4 * f + k                                                  # (F, 3)
        if g is not None:
            np.add.at(b, dof.ravel(), np.einsum("fab,fb->fa", M, np.asarray(g, dtype=np.float64)[:, :, k]).ravel())
        if alpha is not None:
            rows.append(np.repeat(dof, 3, axis=1).ravel())
            cols.append(np.tile(dof, (1, 3)).ravel())
            vals.append((np.asarray(alpha, dtype=np.float64)[:, k][:, None, None] * M).ravel())
    if not rows:
        return sp.csr_matrix((n4, n4)), b
    return sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n4, n4)).tocsr(), b


def scalar_assemble(points, tets, w, kappa, cmask, cval, facets, facet_tets, *, alpha=None, g=None, sigma=0.0, theta=0.0,
                    source=None):
    """(A, b) as sns_scalar_system leaves them with the facet terms set: the Dirichlet rule on the whole raw form."""
    A0, b = SO.raw(points, tets, w, kappa, sigma, theta, source)
    Ab, bb = scalar_raw(points, tets, facets, facet_tets, alpha, g)
    A0, b = (A0 + Ab).tocsr(), b + bb
    mask = np.asarray(cmask).ravel().astype(np.uint8)
    gv = np.asarray(cval, dtype=np.float64).ravel()
    B = mask.astype(bool)
    b = b - A0[:, B] @ gv[B]
    b[B] = gv[B]
    return asm._apply_bc_matrix(A0, mask), b


def scalar_solve(points, tets, w, kappa, cmask, cval, facets, facet_tets, **kw):
    """c (n, 4) by a sparse LU."""
    A, b = scalar_assemble(points, tets, w, kappa, cmask, cval, facets, facet_tets, **kw)
    return spla.splu(sp.csc_matrix(A)).solve(b).reshape(-1, 4)
