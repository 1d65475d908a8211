"""CPU oracle of the transient 3-D NS form (plain helper module of the transient tests, not a conftest).

The reference has no unsteady form, so there is nothing to pin to: this is the literal restatement of the form the
library documents (include/sns.h, sns_set_time_term), written term by term with explicit test functions like
``oracle/forms_literal.py`` and batched over tets, with the Jacobian by autograd.

    u_t = sigma u + d                                  (d: nodal history, P1 like u; held fixed in the derivative)
    F  += (u_t, v)                                      Galerkin mass term
    res_M <- res_M + u_t                                in the SUPG and the PSPG part of the test function
    tau = (theta + u.Gu + C_I nu^2 G:G)^-1/2            nu_LSIC = 1 / (tr G tau) with the same tau

sigma = 0, d = 0, theta = 0 is ``forms_literal.ns_residual_literal``.  On top: global assembly with the Dirichlet rule
of ``oracle/assemble.py`` and a BDF1 / BDF2 stepper (Newton with a sparse LU).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

from oracle import assemble as asm
from oracle import forms_literal as FL

_T = torch.float64


def transient_residual(X, W, D, Re, sigma, theta, *, corrected_convection=False):
    """(E,16) element residuals.  X (E,4,3) vertices, W (E,16) nodal [ux,uy,uz,p]*4 (torch fp64, may require grad),
    D (E,4,3) nodal history.  The perturbations of ``forms_literal.VARIANT`` apply as there."""
    X = torch.as_tensor(X, dtype=_T)
    D = torch.as_tensor(D, dtype=_T)
    V = FL.VARIANT
    nu = 1.0 / Re
    J = torch.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 3] - X[:, 0]], dim=2)      # J[e,i,j] = dx_i/dX_j
    K = torch.linalg.inv(J)
    detJ = torch.abs(torch.linalg.det(J))
    gphi = torch.einsum("ak,ekj->eaj", torch.as_tensor(FL.GHAT, dtype=_T), K)              # d phi_a / d x_j
    G = torch.einsum("eki,ekj->eij", K, K)                                                  # :232-235
    Wn = W.reshape(-1, 4, 4)
    U, P = Wn[:, :, :3], Wn[:, :, 3]
    Ut = sigma * U + D                                                                       # nodal u_t
    grad_u = torch.einsum("eai,eaj->eij", U, gphi)                                          # du_i/dx_j
    div_u = grad_u[:, 0, 0] + grad_u[:, 1, 1] + grad_u[:, 2, 2]
    grad_p = torch.einsum("ea,eaj->ej", P, gphi)
    GG = torch.sum(G * G, dim=(1, 2))
    trG = G[:, 0, 0] + G[:, 1, 1] + G[:, 2, 2]
    I3 = torch.eye(3, dtype=_T)
    out = torch.zeros(W.shape[0], 16, dtype=_T)
    for q in range(4):
        xi = torch.as_tensor([0.25, 0.25, 0.25] if V["one_point"] else FL.QPTS[q], dtype=_T)
        phi = FL._phi(xi)
        u = torch.einsum("a,eai->ei", phi, U)
        p = torch.einsum("a,ea->e", phi, P)
        u_t = torch.einsum("a,eai->ei", phi, Ut)
        Gu = torch.einsum("eij,ej->ei", G, u)
        tau = 1.0 / torch.sqrt(theta + torch.sum(u * Gu, dim=1) + V["ci"] * nu ** 2 * GG)
        conv = torch.einsum("eij,ej->ei", grad_u, u)                                        # (u.grad)u = u @ nabla_grad(u)
        if corrected_convection:
            res_M = u_t + conv + grad_p
        else:
            res_M = u_t + torch.einsum("ei,eij->ej", u, grad_u) + grad_p                    # dot(u, grad(u)) :241
        v_lsic = V["lsic"] / (trG * tau)
        wq = FL.QW[q] * detJ
        cols = []
        for a in range(4):
            for c in range(4):
                if c < 3:                                                                    # test (v, q) = (phi_a e_c, 0)
                    t = phi[a] * conv[:, c]                                                  # :243
                    t = t + nu * torch.einsum("ej,ej->e", grad_u[:, c, :], gphi[:, a, :])    # :244
                    t = t - p * gphi[:, a, c]                                                # :245
                    t = t + phi[a] * u_t[:, c]                                               # (u_t, v)
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


def element(X, W, D, Re, sigma, theta, *, corrected_convection=False, want_jac=True):
    """numpy (F (E,16), J (E,16,16) or None); J = dF/dW by reverse-mode autodiff with D held fixed."""
    Wt = torch.as_tensor(np.asarray(W, dtype=np.float64).reshape(len(X), 16), dtype=_T).clone().requires_grad_(want_jac)
    F = transient_residual(X, Wt, D, Re, sigma, theta, corrected_convection=corrected_convection)
    if not want_jac:
        return F.detach().numpy(), None
    # element e depends on W[e] only: the gradient of sum_e F[e, i] is row i of every element Jacobian (16 cotangents, one batched pass)
    seeds = torch.eye(16, dtype=_T)[:, None, :].expand(16, F.shape[0], 16)
    rows = torch.autograd.grad(F, Wt, grad_outputs=seeds, is_grads_batched=True)[0]
    return F.detach().numpy(), rows.permute(1, 0, 2).detach().numpy()


def raw(points, tets, w, d, Re, sigma, theta, *, corrected_convection=False, want_jac=True):
    """Unconstrained global residual (ndof,) and Jacobian (CSR or None).  d: (ndof,) history, pressure slots ignored."""
    ndof = 4 * len(points)
    W = np.asarray(w, dtype=np.float64).reshape(-1, 4)
    Dn = np.asarray(d, dtype=np.float64).reshape(-1, 4)[:, :3]
    Fe, Je = element(points[tets], W[tets].reshape(len(tets), 16), Dn[tets], Re, sigma, theta,
                     corrected_convection=corrected_convection, want_jac=want_jac)
    F = np.zeros(ndof)
    np.add.at(F, asm._dof_index(tets).ravel(), Fe.reshape(-1))
    return F, (asm._coo(tets, Je, ndof) if want_jac else None)


def assemble(points, tets, w, d, Re, sigma, theta, mask, g, **kw):
    """(J, F) with the Dirichlet rule of oracle/assemble.assemble_ns: lifting F += A0[:,B](g - w_B), F_B = w_B - g, rows
    and columns of constrained dofs zeroed, unit diagonal."""
    F, J0 = raw(points, tets, w, d, Re, sigma, theta, **kw)
    B = mask.astype(bool)
    F = F + J0[:, B] @ (g[B] - w[B])
    F[B] = w[B] - g[B]
    return asm._apply_bc_matrix(J0, mask), F


def bdf(order, dt, w, wprev):
    """(sigma, d) of u_t = sigma u + d: BDF1 (u - u^n)/dt, BDF2 (3u - 4u^n + u^(n-1))/(2 dt)."""
    if order == 1:
        return 1.0 / dt, -w / dt
    return 1.5 / dt, (-2.0 * w + 0.5 * wprev) / dt


def step(points, tets, mask, g, Re, w, wprev, dt, order, theta_coeff, *, tol=1e-11, max_it=30, refresh=1, **kw):
    """One implicit step from the guess u^n (which must satisfy the Dirichlet data): Newton with a sparse LU of the
    autograd Jacobian, the factorisation kept for ``refresh`` iterations (chord steps, residual-only evaluations in
    between), until the update is below tol relative to the state."""
    sigma, d = bdf(order, dt, w, wprev)
    theta = theta_coeff / dt ** 2
    B = mask.astype(bool)
    x = w.copy()
    x[B] = g[B]
    lu = None
    for it in range(max_it):
        if it % refresh == 0:
            J, F = assemble(points, tets, x, d, Re, sigma, theta, mask, g, **kw)
            lu = spla.splu(sp.csc_matrix(J))
        else:
            F, _ = raw(points, tets, x, d, Re, sigma, theta, want_jac=False, **kw)
            F[B] = 0.0
        y = lu.solve(F)
        x = x - y
        if np.linalg.norm(y) <= tol * max(np.linalg.norm(x), 1e-300):
            return x, it + 1
    raise RuntimeError("oracle Newton did not converge")


def march(points, tets, mask, g, Re, w0, dt, n_steps, order, theta_coeff, **kw):
    """n_steps steps from w0: BDF1 first, then BDF of ``order``.  Returns the list of states [w0, w1, ...]."""
    hist = [np.asarray(w0, dtype=np.float64).copy()]
    for n in range(n_steps):
        o = 1 if n == 0 else order
        x, _ = step(points, tets, mask, g, Re, hist[-1], hist[-2] if n > 0 else hist[-1], dt, o, theta_coeff, **kw)
        hist.append(x)
    return hist
