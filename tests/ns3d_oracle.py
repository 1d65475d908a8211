"""CPU oracle of the 3-D NS form with every switch the library has (plain helper module of the form's tests, not a conftest).

The reference has the steady form with a constant nu = 1/Re and no right-hand side; ``oracle/forms_literal.py`` (the per-tet
literal form) and ``oracle/element.py`` pin that to it, independently of this module.  Everything on top has nothing to pin to:
this is the literal restatement of the form the library documents (include/sns.h: sns_set_time_term, sns_set_viscosity_law,
sns_set_body_force, sns_set_element_viscosity), written term by term with explicit test functions like ``forms_literal`` and
batched over tets, with the Jacobian by autograd.

    u_t = sigma u + d,  a = u_t - f                       (d, f: nodal, P1 like u; held fixed in the derivative)
    F  += (a, v)                                           Galerkin part
    eps  = sym(grad u),  s = 2 eps:eps                     constant on a P1 tet (s = gamma_dot^2; no square root, so smooth at rest)
    nu   = 1/Re                                            or nu_t per tet (held fixed)
                                                           or nu_e = nu0 (r + (1 - r)(1 + lambda^2 s)^((n-1)/2)), nu0 = 1/Re, r = nu_inf / nu0
    viscous term  nu (grad u, grad v)                      stress_div off (:244, the reference's form)
                  (2 nu eps(u), grad v)                    stress_div on: exactly where a law or a viscosity field is given
    res_M = dot(u, grad(u)) + grad p + a                   div(2 nu eps(u)) = 0 inside a P1 tet
    tau = (theta + u.Gu + C_I nu^2 G:G)^-1/2               nu_LSIC = 1 / (tr G tau) with the same tau

Every switch off is ``forms_literal.ns_residual_literal``; a switch that is off adds no operation.  On top: global assembly with
the Dirichlet rule of ``oracle/assemble.py``, one Newton (sparse LU), the BDF1 / BDF2 stepper, the mixture rule of
sns_set_mixture and the fixed-point loop of ``solver.solve_coupled_flow``.  The form keywords, the same for every function
here: d=, f=, nu_t=, law=(lambda, n, r), sigma=, theta=, stress_div=, corrected_convection=.
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


def residual(X, W, Re, *, d=None, f=None, nu_t=None, law=None, sigma=0.0, theta=0.0, stress_div=None, corrected_convection=False):
    """(E,16) element residuals.  X (E,4,3) vertices, W (E,16) nodal [ux,uy,uz,p]*4 (torch fp64, may require grad), d and f
    (E,4,3) nodal history and force, nu_t (E,) per-tet viscosity, law = (lambda, n, r) of the Carreau law; stress_div None: on
    exactly where a law or nu_t is given, as in the library.  The perturbations of ``forms_literal.VARIANT`` apply as there."""
    if law is not None and nu_t is not None:
        raise ValueError("a viscosity law and a viscosity field exclude each other (the library refuses the pair)")
    if stress_div is None:
        stress_div = law is not None or nu_t is not None
    V = FL.VARIANT
    detJ, gphi, G = _geometry(X)
    Wn = W.reshape(-1, 4, 4)
    U, P = Wn[:, :, :3], Wn[:, :, 3]
    An = None                                                                                # nodal a = u_t - f
    if sigma != 0.0:
        An = sigma * U
    if d is not None:
        An = torch.as_tensor(d, dtype=_T) if An is None else An + torch.as_tensor(d, dtype=_T)
    if f is not None:
        An = -torch.as_tensor(f, dtype=_T) if An is None else An - torch.as_tensor(f, dtype=_T)
    grad_u = torch.einsum("eai,eaj->eij", U, gphi)                                          # du_i/dx_j
    div_u = grad_u[:, 0, 0] + grad_u[:, 1, 1] + grad_u[:, 2, 2]
    grad_p = torch.einsum("ea,eaj->ej", P, gphi)
    if stress_div or law is not None:
        eps = 0.5 * (grad_u + grad_u.transpose(1, 2))
    if law is not None:
        nu = carreau(2.0 * torch.sum(eps * eps, dim=(1, 2)), 1.0 / Re, *law)
    else:
        nu = 1.0 / Re if nu_t is None else torch.as_tensor(nu_t, dtype=_T)
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
        uGu = torch.sum(u * Gu, dim=1)
        if theta != 0.0:
            uGu = theta + uGu
        tau = 1.0 / torch.sqrt(uGu + V["ci"] * nu ** 2 * GG)
        conv = torch.einsum("eij,ej->ei", grad_u, u)                                        # (u.grad)u = u @ nabla_grad(u)
        res_M = conv if corrected_convection else torch.einsum("ei,eij->ej", u, grad_u)     # dot(u, grad(u)) :241
        if An is not None:
            a_q = torch.einsum("a,eai->ei", phi, An)
            res_M = a_q + res_M
        res_M = res_M + grad_p
        v_lsic = V["lsic"] / (trG * tau)
        wq = FL.QW[q] * detJ
        cols = []
        for a in range(4):
            for c in range(4):
                if c < 3:                                                                    # test (v, q) = (phi_a e_c, 0)
                    t = phi[a] * conv[:, c]                                                  # :243
                    if stress_div:                                                           # (2 nu eps(u), grad v)
                        t = t + 2.0 * nu * torch.einsum("ej,ej->e", eps[:, c, :], gphi[:, a, :])
                    else:                                                                    # :244
                        t = t + nu * torch.einsum("ej,ej->e", grad_u[:, c, :], gphi[:, a, :])
                    t = t - p * gphi[:, a, c]                                                # :245
                    if An is not None:
                        t = t + phi[a] * a_q[:, c]                                           # (a, v)
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


def element(X, W, Re, *, want_jac=True, **form):
    """numpy (F (E,16), J (E,16,16) or None); J = dF/dW by reverse-mode autodiff with d, f and nu_t held fixed."""
    Wt = torch.as_tensor(np.asarray(W, dtype=np.float64).reshape(len(X), 16), dtype=_T).clone().requires_grad_(want_jac)
    F = residual(X, Wt, Re, **form)
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


def _nodal3(x, tets):
    return None if x is None else np.asarray(x, dtype=np.float64).reshape(-1, 4)[:, :3][tets]


def raw(points, tets, w, Re, *, d=None, f=None, want_jac=True, extra=None, **form):
    """Unconstrained global residual (ndof,) and Jacobian (CSR or None).  d, f: (ndof,) history and force (pressure slots
    ignored) or None; nu_t: (n_tets,) or None.  extra: callable (w, want_jac) -> (F, J) added to the raw form (the facet terms)."""
    ndof = 4 * len(points)
    W = np.asarray(w, dtype=np.float64).reshape(-1, 4)
    Fe, Je = element(points[tets], W[tets].reshape(len(tets), 16), Re, d=_nodal3(d, tets), f=_nodal3(f, tets), want_jac=want_jac, **form)
    F = np.zeros(ndof)
    np.add.at(F, asm._dof_index(tets).ravel(), Fe.reshape(-1))
    J = asm._coo(tets, Je, ndof) if want_jac else None
    if extra is not None:
        Fx, Jx = extra(w, want_jac)
        F, J = F + Fx, (J + Jx if want_jac else None)
    return F, J


def assemble(points, tets, w, Re, mask, g, **kw):
    """(J, F) with the Dirichlet rule of oracle/assemble.assemble_ns on the whole raw form: lifting F += A0[:,B](g - w_B),
    F_B = w_B - g, rows and columns of constrained dofs zeroed, unit diagonal."""
    F, J0 = raw(points, tets, w, Re, **kw)
    B = mask.astype(bool)
    F = F + J0[:, B] @ (g[B] - w[B])
    F[B] = w[B] - g[B]
    return asm._apply_bc_matrix(J0, mask), F


def newton(points, tets, mask, g, Re, w0, *, tol=1e-12, max_it=40, backtrack=True, refresh=1, **kw):
    """Newton with a sparse LU of the autograd Jacobian from the guess w0, until the update is below tol relative to the
    state.  Returns (w, its).  backtrack: steps are damped by halving while the residual norm does not fall, and a start
    that is converged already returns at once (the residual test would see round-off).  refresh: the factorisation is kept
    for that many iterations (chord steps, residual-only evaluations in between).

    The one rule in place of three that had drifted apart: the law's Newton tested convergence only after a full step, the
    fields' also returned early from a converged start, and the boundary terms' could leave only through that early return,
    one factorisation after the other two."""
    B = mask.astype(bool)
    x = np.asarray(w0, dtype=np.float64).copy()
    x[B] = g[B]
    for it in range(max_it):
        if it % refresh == 0:
            J, F = assemble(points, tets, x, Re, mask, g, **kw)
            lu = spla.splu(sp.csc_matrix(J))
        else:
            F, _ = raw(points, tets, x, Re, want_jac=False, **kw)
            F[B] = 0.0
        y = lu.solve(F)
        step = 1.0
        if backtrack:
            if np.linalg.norm(y) <= tol * max(np.linalg.norm(x), 1e-300):
                return x - y, it + 1
            f0 = np.linalg.norm(F)
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


def stokes_start(points, tets, mask, g):
    """The Stokes solution of oracle/assemble.py: the Newton start of the fixtures' runs."""
    A, b = asm.assemble_stokes(points, tets, mask, g)
    return spla.splu(sp.csc_matrix(A)).solve(b)


def bdf(order, dt, w, wprev):
    """(sigma, d) of u_t = sigma u + d: BDF1 (u - u^n)/dt, BDF2 (3u - 4u^n + u^(n-1))/(2 dt)."""
    if order == 1:
        return 1.0 / dt, -w / dt
    return 1.5 / dt, (-2.0 * w + 0.5 * wprev) / dt


def step(points, tets, mask, g, Re, w, wprev, dt, order, theta_coeff, *, tol=1e-11, max_it=30, refresh=1, **kw):
    """One implicit step from the guess u^n (which must satisfy the Dirichlet data): the undamped ``newton`` on the form with
    the time term of ``bdf`` and theta = theta_coeff / dt^2.  Returns (w, its)."""
    sigma, d = bdf(order, dt, w, wprev)
    return newton(points, tets, mask, g, Re, w, tol=tol, max_it=max_it, backtrack=False, refresh=refresh,
                  d=d, sigma=sigma, theta=theta_coeff / dt ** 2, **kw)


def march(points, tets, mask, g, Re, w0, dt, n_steps, order, theta_coeff, **kw):
    """n_steps steps from w0: BDF1 first, then BDF of ``order``.  Returns the list of states [w0, w1, ...]."""
    hist = [np.asarray(w0, dtype=np.float64).copy()]
    for n in range(n_steps):
        o = 1 if n == 0 else order
        x, _ = step(points, tets, mask, g, Re, hist[-1], hist[-2] if n > 0 else hist[-1], dt, o, theta_coeff, **kw)
        hist.append(x)
    return hist


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
