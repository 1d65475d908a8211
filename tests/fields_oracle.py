"""CPU oracle of the 3-D NS form with a body force and a per-cell viscosity field (plain helper module of the fields tests, not
a conftest).

The reference has no right-hand side and a constant nu = 1/Re, so there is nothing to pin to: this is the literal restatement of
the form the library documents (include/sns.h, sns_set_body_force / sns_set_element_viscosity), written term by term with
explicit test functions like ``oracle/forms_literal.py`` and batched over tets, with the Jacobian by autograd.

    u_t = sigma u + d,  a = u_t - f                       (d, f: nodal, P1 like u; held fixed in the derivative)
    F  += (a, v)                                           Galerkin part
    viscous term  nu_t (grad u, grad v)                    stress_div off (:244; a body force alone keeps the reference's form)
                  (2 nu_t eps(u), grad v)                  stress_div on  (a viscosity field; nu_t per tet, held fixed)
    res_M = dot(u, grad(u)) + grad p + a                   div(2 nu_t eps(u)) = 0 inside a P1 tet
    tau = (theta + u.Gu + C_I nu_t^2 G:G)^-1/2             nu_LSIC = 1 / (tr G tau) with the same tau

F = 0, nu_t = 1/Re, stress_div off is ``transient_oracle.transient_residual``; stress_div on with d = 0, sigma = theta = 0 is
``viscosity_oracle.law_residual`` at n = 1.  On top: global assembly with the Dirichlet rule of ``oracle/assemble.py``, Newton
with a sparse LU, the mixture rule of sns_set_mixture and the fixed-point loop of ``solver.solve_coupled_flow``.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

from oracle import assemble as asm
from oracle import forms_literal as FL

import scalar_oracle as SO

_T = torch.float64


def residual(X, W, D, F, nu_t, Re, sigma, theta, stress_div, *, corrected_convection=False):
    """(E,16) element residuals.  X (E,4,3) vertices, W (E,16) nodal [ux,uy,uz,p]*4 (torch fp64, may require grad), D and F
    (E,4,3) nodal history and force (None: zero), nu_t (E,) per-tet viscosity (None: 1/Re).  The perturbations of
    ``forms_literal.VARIANT`` apply as there."""
    X = torch.as_tensor(X, dtype=_T)
    E = X.shape[0]
    D = torch.zeros(E, 4, 3, dtype=_T) if D is None else torch.as_tensor(D, dtype=_T)
    Fn = torch.zeros(E, 4, 3, dtype=_T) if F is None else torch.as_tensor(F, dtype=_T)
    nu = torch.full((E,), 1.0 / Re, dtype=_T) if nu_t is None else torch.as_tensor(nu_t, dtype=_T)
    V = FL.VARIANT
    J = torch.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 3] - X[:, 0]], dim=2)      # J[e,i,j] = dx_i/dX_j
    K = torch.linalg.inv(J)
    detJ = torch.abs(torch.linalg.det(J))
    gphi = torch.einsum("ak,ekj->eaj", torch.as_tensor(FL.GHAT, dtype=_T), K)              # d phi_a / d x_j
    G = torch.einsum("eki,ekj->eij", K, K)                                                  # :232-235
    Wn = W.reshape(-1, 4, 4)
    U, P = Wn[:, :, :3], Wn[:, :, 3]
    An = sigma * U + D - Fn                                                                  # nodal a = u_t - f
    grad_u = torch.einsum("eai,eaj->eij", U, gphi)                                          # du_i/dx_j
    div_u = grad_u[:, 0, 0] + grad_u[:, 1, 1] + grad_u[:, 2, 2]
    grad_p = torch.einsum("ea,eaj->ej", P, gphi)
    eps = 0.5 * (grad_u + grad_u.transpose(1, 2))
    GG = torch.sum(G * G, dim=(1, 2))
    trG = G[:, 0, 0] + G[:, 1, 1] + G[:, 2, 2]
    I3 = torch.eye(3, dtype=_T)
    out = torch.zeros(W.shape[0], 16, dtype=_T)
    for q in range(4):
        xi = torch.as_tensor([0.25, 0.25, 0.25] if V["one_point"] else FL.QPTS[q], dtype=_T)
        phi = FL._phi(xi)
        u = torch.einsum("a,eai->ei", phi, U)
        p = torch.einsum("a,ea->e", phi, P)
        a_q = torch.einsum("a,eai->ei", phi, An)
        Gu = torch.einsum("eij,ej->ei", G, u)
        tau = 1.0 / torch.sqrt(theta + torch.sum(u * Gu, dim=1) + V["ci"] * nu ** 2 * GG)
        conv = torch.einsum("eij,ej->ei", grad_u, u)                                        # (u.grad)u = u @ nabla_grad(u)
        if corrected_convection:
            res_M = a_q + conv + grad_p
        else:
            res_M = a_q + torch.einsum("ei,eij->ej", u, grad_u) + grad_p                    # dot(u, grad(u)) :241
        v_lsic = V["lsic"] / (trG * tau)
        wq = FL.QW[q] * detJ
        cols = []
        for a in range(4):
            for c in range(4):
                if c < 3:                                                                    # test (v, q) = (phi_a e_c, 0)
                    t = phi[a] * conv[:, c]                                                  # :243
                    if stress_div:                                                           # (2 nu_t eps(u), grad v)
                        t = t + 2.0 * nu * torch.einsum("ej,ej->e", eps[:, c, :], gphi[:, a, :])
                    else:                                                                    # :244
                        t = t + nu * torch.einsum("ej,ej->e", grad_u[:, c, :], gphi[:, a, :])
                    t = t - p * gphi[:, a, c]                                                # :245
                    t = t + phi[a] * a_q[:, c]                                               # (a, v)
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


def element(X, W, D, F, nu_t, Re, sigma, theta, stress_div, *, corrected_convection=False, want_jac=True):
    """numpy (F (E,16), J (E,16,16) or None); J = dF/dW by reverse-mode autodiff with D, F and nu_t held fixed."""
    Wt = torch.as_tensor(np.asarray(W, dtype=np.float64).reshape(len(X), 16), dtype=_T).clone().requires_grad_(want_jac)
    R = residual(X, Wt, D, F, nu_t, Re, sigma, theta, stress_div, corrected_convection=corrected_convection)
    if not want_jac:
        return R.detach().numpy(), None
    # element e depends on W[e] only: the gradient of sum_e F[e, i] is row i of every element Jacobian (16 cotangents, one batched pass)
    seeds = torch.eye(16, dtype=_T)[:, None, :].expand(16, R.shape[0], 16)
    rows = torch.autograd.grad(R, Wt, grad_outputs=seeds, is_grads_batched=True)[0]
    return R.detach().numpy(), rows.permute(1, 0, 2).detach().numpy()


def _nodal3(x, tets):
    return None if x is None else np.asarray(x, dtype=np.float64).reshape(-1, 4)[:, :3][tets]


def raw(points, tets, w, Re, *, d=None, f=None, nu_t=None, sigma=0.0, theta=0.0, corrected_convection=False, want_jac=True):
    """Unconstrained global residual (ndof,) and Jacobian (CSR or None).  d, f: (ndof,) history and force (pressure slots
    ignored) or None; nu_t: (n_tets,) or None.  The stress-divergence form is on exactly where nu_t is given, as in the library."""
    ndof = 4 * len(points)
    W = np.asarray(w, dtype=np.float64).reshape(-1, 4)
    Fe, Je = element(points[tets], W[tets].reshape(len(tets), 16), _nodal3(d, tets), _nodal3(f, tets), nu_t, Re, sigma, theta,
                     nu_t is not None, corrected_convection=corrected_convection, want_jac=want_jac)
    F = np.zeros(ndof)
    np.add.at(F, asm._dof_index(tets).ravel(), Fe.reshape(-1))
    return F, (asm._coo(tets, Je, ndof) if want_jac else None)


def assemble(points, tets, w, Re, mask, g, **kw):
    """(J, F) with the Dirichlet rule of oracle/assemble.assemble_ns: lifting F += A0[:,B](g - w_B), F_B = w_B - g, rows
    and columns of constrained dofs zeroed, unit diagonal."""
    F, J0 = raw(points, tets, w, Re, **kw)
    B = mask.astype(bool)
    F = F + J0[:, B] @ (g[B] - w[B])
    F[B] = w[B] - g[B]
    return asm._apply_bc_matrix(J0, mask), F


def newton(points, tets, mask, g, Re, w0, *, tol=1e-12, max_it=40, **kw):
    """Newton with a sparse LU of the autograd Jacobian from the guess w0, until the update is below tol relative to the
    state.  Steps are damped by halving while the residual norm does not fall (plain backtracking).  Returns (w, its)."""
    B = mask.astype(bool)
    x = np.asarray(w0, dtype=np.float64).copy()
    x[B] = g[B]
    for it in range(max_it):
        J, F = assemble(points, tets, x, Re, mask, g, **kw)
        y = spla.splu(sp.csc_matrix(J)).solve(F)
        if np.linalg.norm(y) <= tol * max(np.linalg.norm(x), 1e-300):         # (a start that is converged already: the
            return x - y, it + 1                                               #  residual test below would see round-off)
        f0, step = np.linalg.norm(F), 1.0
        while step > 1e-3:
            Ft, _ = raw(points, tets, x - step * y, Re, want_jac=False, **kw)
            Ft[B] = 0.0
            if np.linalg.norm(Ft) < f0:
                break
            step *= 0.5
        x = x - step * y
        if step == 1.0 and np.linalg.norm(y) <= tol * max(np.linalg.norm(x), 1e-300):
            return x, it + 1
    raise RuntimeError("oracle Newton did not converge")


def step(points, tets, mask, g, Re, w, wprev, dt, order, theta_coeff, *, tol=1e-11, max_it=30, **kw):
    """One implicit BDF step of ``transient_oracle.step`` with the fields of ``raw`` (f=, nu_t=): Newton with a sparse LU from
    the guess u^n until the update is below tol relative to the state.  Returns (w, its)."""
    sigma, d = (1.0 / dt, -w / dt) if order == 1 else (1.5 / dt, (-2.0 * w + 0.5 * wprev) / dt)
    B = mask.astype(bool)
    x = w.copy()
    x[B] = g[B]
    for it in range(max_it):
        J, F = assemble(points, tets, x, Re, mask, g, d=d, sigma=sigma, theta=theta_coeff / dt ** 2, **kw)
        y = spla.splu(sp.csc_matrix(J)).solve(F)
        x = x - y
        if np.linalg.norm(y) <= tol * max(np.linalg.norm(x), 1e-300):
            return x, it + 1
    raise RuntimeError("oracle Newton did not converge")


def mixture_fields(points, tets, m, Re, log_ratio, buoyancy):
    """(nu_t (n_tets,), f (ndof,)) of sns_set_mixture: nu_t = (1/Re) exp(log_ratio * mean of m over the tet's vertices), f_a = m_a *
    buoyancy in the velocity slots."""
    m = np.asarray(m, dtype=np.float64).ravel()
    mt = m[tets]
    nu_t = (1.0 / Re) * np.exp(log_ratio * (0.25 * (((mt[:, 0] + mt[:, 1]) + mt[:, 2]) + mt[:, 3])))
    f = np.zeros((len(points), 4))
    f[:, :3] = m[:, None] * np.asarray(buoyancy, dtype=np.float64)[None, :]
    return nu_t, f.ravel()


def coupled(points, tets, mask, g, Re, w0, kappa, cmask, cval, *, log_ratio=0.0, buoyancy=(0.0, 0.0, 0.0), max_outer=30, rtol=1e-8,
            relax=1.0, **kw):
    """The fixed-point loop of solver.solve_coupled_flow on species 0 of one scalar (the other three constrained to 0 on every
    node): mixture fields from c, flow Newton (sparse LU) from the last state, ``scalar_oracle.solve`` carried by the new state,
    c <- c + relax (c_new - c), until ||c_new - c|| <= rtol ||c_new||.  cmask, cval: (n,) Dirichlet data of the scalar.
    Returns (w, c (n,), changes): the list of relative changes, one per outer step."""
    n = len(points)
    m4, v4 = np.ones((n, 4), np.uint8), np.zeros((n, 4))
    m4[:, 0], v4[:, 0] = np.asarray(cmask).astype(np.uint8), np.where(cmask, cval, 0.0)
    kap4 = np.array([kappa, 1.0, 1.0, 1.0])
    w = np.asarray(w0, dtype=np.float64).copy()
    c = np.zeros(n)
    changes = []
    want_nu = log_ratio != 0.0
    want_f = any(b != 0.0 for b in buoyancy)
    for _ in range(max_outer):
        nu_t, f = mixture_fields(points, tets, c, Re, log_ratio, buoyancy)
        w, _ = newton(points, tets, mask, g, Re, w, nu_t=nu_t if want_nu else None, f=f if want_f else None, **kw)
        cn = SO.solve(points, tets, w, kap4, m4, v4)[:, 0]
        changes.append(float(np.linalg.norm(cn - c) / max(np.linalg.norm(cn), 1e-300)))
        c = c + relax * (cn - c)
        if changes[-1] <= rtol:
            return w, c, changes
    raise RuntimeError("oracle fixed point did not converge")
