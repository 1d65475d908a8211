"""CPU oracle of the generalised-Newtonian (Carreau) 3-D NS form (plain helper module of the viscosity tests, not a conftest).

The reference has a constant nu = 1/Re in every form, so there is nothing to pin to: this is the literal restatement of the
form the library documents (include/sns.h, sns_set_viscosity_law), written term by term with explicit test functions like
``oracle/forms_literal.py`` and batched over tets, with the Jacobian by autograd.

    eps  = sym(grad u)                                   constant on a P1 tet
    s    = 2 eps:eps                                      (= gamma_dot^2; no square root, so smooth at rest)
    nu_e = nu0 (r + (1 - r)(1 + lambda^2 s)^((n-1)/2))    nu0 = 1/Re, r = nu_inf / nu0
    F   += (2 nu_e eps(u), grad v)                        in place of nu (grad u, grad v) (:244)
    res_M unchanged                                       div(2 nu_e eps(u)) = 0 inside a P1 element
    tau  = (u.Gu + C_I nu_e^2 G:G)^-1/2                   nu_LSIC = 1 / (tr G tau) with the same tau

lambda = 0 (or n = 1) is ``forms_literal.ns_residual_literal`` plus nu (grad u^T, grad v).  On top: global assembly with
the Dirichlet rule of ``oracle/assemble.py`` and Newton with a sparse LU.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

from oracle import assemble as asm
from oracle import forms_literal as FL

_T = torch.float64


def carreau(s, nu0, lam, n, r):
    """nu_e(s) of the law, s = 2 eps:eps (torch or numpy)."""
    return nu0 * (r + (1.0 - r) * (1.0 + lam ** 2 * s) ** (0.5 * (n - 1.0)))


def _geometry(X):
    X = torch.as_tensor(X, dtype=_T)
    J = torch.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 3] - X[:, 0]], dim=2)      # J[e,i,j] = dx_i/dX_j
    K = torch.linalg.inv(J)
    detJ = torch.abs(torch.linalg.det(J))
    gphi = torch.einsum("ak,ekj->eaj", torch.as_tensor(FL.GHAT, dtype=_T), K)              # d phi_a / d x_j
    G = torch.einsum("eki,ekj->eij", K, K)                                                  # :232-235
    return detJ, gphi, G


def shear_rate2(X, W):
    """s = 2 eps:eps per tet (torch); X (E,4,3), W (E,16)."""
    _, gphi, _ = _geometry(X)
    U = torch.as_tensor(W, dtype=_T).reshape(-1, 4, 4)[:, :, :3]
    grad_u = torch.einsum("eai,eaj->eij", U, gphi)
    eps = 0.5 * (grad_u + grad_u.transpose(1, 2))
    return 2.0 * torch.sum(eps * eps, dim=(1, 2))


def law_residual(X, W, Re, lam, n, r, *, corrected_convection=False):
    """(E,16) element residuals.  X (E,4,3) vertices, W (E,16) nodal [ux,uy,uz,p]*4 (torch fp64, may require grad).  The
    perturbations of ``forms_literal.VARIANT`` apply as there."""
    V = FL.VARIANT
    nu0 = 1.0 / Re
    detJ, gphi, G = _geometry(X)
    Wn = W.reshape(-1, 4, 4)
    U, P = Wn[:, :, :3], Wn[:, :, 3]
    grad_u = torch.einsum("eai,eaj->eij", U, gphi)                                          # du_i/dx_j
    div_u = grad_u[:, 0, 0] + grad_u[:, 1, 1] + grad_u[:, 2, 2]
    grad_p = torch.einsum("ea,eaj->ej", P, gphi)
    eps = 0.5 * (grad_u + grad_u.transpose(1, 2))
    s = 2.0 * torch.sum(eps * eps, dim=(1, 2))
    nu_e = carreau(s, nu0, lam, n, r)
    GG = torch.sum(G * G, dim=(1, 2))
    trG = G[:, 0, 0] + G[:, 1, 1] + G[:, 2, 2]
    I3 = torch.eye(3, dtype=_T)
    out = torch.zeros(W.shape[0], 16, dtype=_T)
    for q in range(4):
        xi = torch.as_tensor([0.25, 0.25, 0.25] if V["one_point"] else FL.QPTS[q], dtype=_T)
        phi = FL._phi(xi)
        u = torch.einsum("a,eai->ei", phi, U)
        p = torch.einsum("a,ea->e", phi, P)
        Gu = torch.einsum("eij,ej->ei", G, u)
        tau = 1.0 / torch.sqrt(torch.sum(u * Gu, dim=1) + V["ci"] * nu_e ** 2 * GG)
        conv = torch.einsum("eij,ej->ei", grad_u, u)                                        # (u.grad)u = u @ nabla_grad(u)
        if corrected_convection:
            res_M = conv + grad_p
        else:
            res_M = torch.einsum("ei,eij->ej", u, grad_u) + grad_p                          # dot(u, grad(u)) :241
        v_lsic = V["lsic"] / (trG * tau)
        wq = FL.QW[q] * detJ
        cols = []
        for a in range(4):
            for c in range(4):
                if c < 3:                                                                    # test (v, q) = (phi_a e_c, 0)
                    t = phi[a] * conv[:, c]                                                  # :243
                    t = t + 2.0 * nu_e * torch.einsum("ej,ej->e", eps[:, c, :], gphi[:, a, :])   # (2 nu_e eps(u), grad v)
                    t = t - p * gphi[:, a, c]                                                # :245
                    if corrected_convection:                                                 # (u.grad) v = (u.g_a) e_c
                        supg = torch.einsum("ej,ej->e", u, gphi[:, a, :])[:, None] * I3[c][None, :]
                    else:                                                                    # dot(u, grad(v)) = u_c g_a
                        supg = u[:, c][:, None] * gphi[:, a, :]
                    t = t + tau * torch.einsum("ej,ej->e", res_M, supg)                      # :247
                    t = t + v_lsic * gphi[:, a, c] * div_u                                   # :251
                else:                                                                        # test (0, phi_a)
                    t = phi[a] * div_u                                                       # :246
                    t = t + V["pspg"] * tau * torch.einsum("ej,ej->e", res_M, gphi[:, a, :])
                cols.append(wq * t)
        out = out + torch.stack(cols, dim=1)
    return out


def transpose_term(X, W, Re):
    """(E,16) element vector of nu (grad u^T, grad v): what the stress-divergence form adds to the reference's viscous term
    for a constant nu."""
    detJ, gphi, _ = _geometry(X)
    U = torch.as_tensor(W, dtype=_T).reshape(-1, 4, 4)[:, :, :3]
    grad_u = torch.einsum("eai,eaj->eij", U, gphi)
    out = torch.zeros(len(detJ), 4, 4, dtype=_T)
    out[:, :, :3] = (detJ / 6.0 / Re)[:, None, None] * torch.einsum("ejc,eaj->eac", grad_u, gphi)
    return out.reshape(-1, 16)


def element(X, W, Re, lam, n, r, *, corrected_convection=False, want_jac=True):
    """numpy (F (E,16), J (E,16,16) or None); J = dF/dW by reverse-mode autodiff."""
    Wt = torch.as_tensor(np.asarray(W, dtype=np.float64).reshape(len(X), 16), dtype=_T).clone().requires_grad_(want_jac)
    F = law_residual(X, Wt, Re, lam, n, r, corrected_convection=corrected_convection)
    if not want_jac:
        return F.detach().numpy(), None
    # element e depends on W[e] only: the gradient of sum_e F[e, i] is row i of every element Jacobian (16 cotangents, one batched pass)
    seeds = torch.eye(16, dtype=_T)[:, None, :].expand(16, F.shape[0], 16)
    rows = torch.autograd.grad(F, Wt, grad_outputs=seeds, is_grads_batched=True)[0]
    return F.detach().numpy(), rows.permute(1, 0, 2).detach().numpy()


def element_viscosity(points, tets, w, Re, lam, n, r):
    """numpy (nu_e, gamma_dot) per tet."""
    W = np.asarray(w, dtype=np.float64).reshape(-1, 4)
    s = shear_rate2(points[tets], W[tets].reshape(len(tets), 16))
    return carreau(s, 1.0 / Re, lam, n, r).numpy(), torch.sqrt(s).numpy()


def raw(points, tets, w, Re, lam, n, r, *, corrected_convection=False, want_jac=True):
    """Unconstrained global residual (ndof,) and Jacobian (CSR or None)."""
    ndof = 4 * len(points)
    W = np.asarray(w, dtype=np.float64).reshape(-1, 4)
    Fe, Je = element(points[tets], W[tets].reshape(len(tets), 16), Re, lam, n, r,
                     corrected_convection=corrected_convection, want_jac=want_jac)
    F = np.zeros(ndof)
    np.add.at(F, asm._dof_index(tets).ravel(), Fe.reshape(-1))
    return F, (asm._coo(tets, Je, ndof) if want_jac else None)


def assemble(points, tets, w, Re, lam, n, r, mask, g, **kw):
    """(J, F) with the Dirichlet rule of oracle/assemble.assemble_ns: lifting F += A0[:,B](g - w_B), F_B = w_B - g, rows
    and columns of constrained dofs zeroed, unit diagonal."""
    F, J0 = raw(points, tets, w, Re, lam, n, r, **kw)
    B = mask.astype(bool)
    F = F + J0[:, B] @ (g[B] - w[B])
    F[B] = w[B] - g[B]
    return asm._apply_bc_matrix(J0, mask), F


def newton(points, tets, mask, g, Re, lam, n, r, w0, *, tol=1e-12, max_it=40, **kw):
    """Newton with a sparse LU of the autograd Jacobian from the guess w0, until the update is below tol relative to the
    state.  Steps are damped by halving while the residual norm does not fall (plain backtracking)."""
    B = mask.astype(bool)
    x = np.asarray(w0, dtype=np.float64).copy()
    x[B] = g[B]
    for it in range(max_it):
        J, F = assemble(points, tets, x, Re, lam, n, r, mask, g, **kw)
        y = spla.splu(sp.csc_matrix(J)).solve(F)
        f0, step = np.linalg.norm(F), 1.0
        while step > 1e-3:
            Ft, _ = raw(points, tets, x - step * y, Re, lam, n, r, want_jac=False, **kw)
            Ft[B] = 0.0
            if np.linalg.norm(Ft) < f0:
                break
            step *= 0.5
        x = x - step * y
        if step == 1.0 and np.linalg.norm(y) <= tol * max(np.linalg.norm(x), 1e-300):
            return x, it + 1
    raise RuntimeError("oracle Newton did not converge")


def stokes_start(points, tets, mask, g):
    """The Stokes solution of oracle/assemble.py: the Newton start of the fixture's runs."""
    A, b = asm.assemble_stokes(points, tets, mask, g)
    return spla.splu(sp.csc_matrix(A)).solve(b)
