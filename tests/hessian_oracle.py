"""CPU oracle of the Hessian pass and the two eigenvalue sensitivities built on it (plain helper module of
tests/test_host_hessian.py and tests/test_gpu_hessian.py, not a conftest): everything on top of tests/ns3d_oracle.py,
tests/stability_oracle.py and tests/left_modes_oracle.py.

    state_gradient(c, w, x, z, c_jac, c_mass)   g = grad_w [ z~^T (c_J J(w) + c_B B(w)) x~ ] by double backward through the
                                                oracle's element residual: per cell
                                                phi_e = c_J d/d eps [z_e . R_e(W + eps x_e)] + c_B z_e . (R_e(W; d = x_u) - R_e(W)),
                                                scattered over the cells, constrained entries 0
    mass_by_identity(c, w, x)                   B(w) x~ = R(w; d = x_u) - R(w), constrained rows 0
    mass_transpose(c, w, z)                     B(w)^T z~ by autograd in d
    contraction(c, w, x, z, c_jac, c_mass)      the number z~^T (c_J J(w) + c_B B(w)) x~ from the assembled operators
    s_vector / base_flow_sensitivity            s = H_J(z, x) + lam H_B(z, x) and grad_w lam = -s / (z^T B x) for a complex pair
    e_vector / e_vector_fd                      E = D_w[B(w)^T z][x] by double backward, and by the central difference of
                                                mass_transpose along x the library takes
    forcing_sensitivity                         grad_f lam = B^T J^-T grad_w lam + E / (z^T B x), sparse LU (inner_rtol: the two
                                                solves perturbed to that relative residual, as stability_oracle.Solver does)
    seeded_force / forced_state / forced_eigenvalue    the check of grad_f lam against dense spectra of re-converged states
    lumped_volume                               a quarter of the incident cells' volumes per node
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp
import torch

import left_modes_oracle as LO
import ns3d_oracle as NS
import stability_oracle as SO

_T = torch.float64


def masked(c, v):
    return np.where(c.constrained, 0.0, np.asarray(v, dtype=np.float64))


def _cells(c, v):
    return torch.as_tensor(np.asarray(v, dtype=np.float64).reshape(-1, 4)[c.mesh.tets].reshape(len(c.mesh.tets), 16), dtype=_T)


def _scatter(c, ge):
    tets = c.mesh.tets
    dofs = (4 * tets[:, :, None] + np.arange(4)[None, None, :]).reshape(-1)
    g = np.zeros(4 * len(c.mesh.points))
    np.add.at(g, dofs, np.asarray(ge).reshape(-1))
    g[c.constrained] = 0.0
    return g


def cell_gradients(c, w, x, z, c_jac, c_mass, **form):
    """(E, 16) d phi_e / d W_e, unmasked (x and z are masked here)."""
    X = c.mesh.points[c.mesh.tets]
    W = _cells(c, w).clone().requires_grad_(True)
    xe, ze = _cells(c, masked(c, x)), _cells(c, masked(c, z))
    R = NS.residual(X, W, c.Re, **form)
    phi = torch.zeros((), dtype=_T)
    if c_jac != 0.0:
        gW, = torch.autograd.grad(torch.sum(ze * R), W, create_graph=True)
        phi = phi + c_jac * torch.sum(gW * xe)
    if c_mass != 0.0:
        Rd = NS.residual(X, W, c.Re, d=xe.reshape(-1, 4, 4)[:, :, :3], **form)
        phi = phi + c_mass * torch.sum(ze * (Rd - R))
    ge, = torch.autograd.grad(phi, W)
    return ge.numpy()


def state_gradient(c, w, x, z, c_jac=1.0, c_mass=0.0, **form):
    return _scatter(c, cell_gradients(c, w, x, z, c_jac, c_mass, **form))


def mass_by_identity(c, w, x, **form):
    X = c.mesh.points[c.mesh.tets]
    W = _cells(c, w)
    xe = _cells(c, masked(c, x))
    with torch.no_grad():
        d = NS.residual(X, W, c.Re, d=xe.reshape(-1, 4, 4)[:, :, :3], **form) - NS.residual(X, W, c.Re, **form)
    return _scatter(c, d.numpy())


def _theta(c, W, ze, d, **form):
    return torch.sum(ze * NS.residual(c.mesh.points[c.mesh.tets], W, c.Re, d=d, **form))


def _scatter3(c, de):
    """(E, 4, 3) adjoints of the nodal history -> (ndof,) with the pressure slots 0, constrained rows 0."""
    full = np.zeros((len(c.mesh.tets), 4, 4))
    full[:, :, :3] = np.asarray(de)
    return _scatter(c, full)


def mass_transpose(c, w, z, **form):
    d = torch.zeros(len(c.mesh.tets), 4, 3, dtype=_T, requires_grad=True)
    gd, = torch.autograd.grad(_theta(c, _cells(c, w), _cells(c, masked(c, z)), d, **form), d)
    return _scatter3(c, gd.numpy())


def contraction(c, w, x, z, c_jac, c_mass, **form):
    xm, zm = masked(c, x), masked(c, z)
    v = 0.0
    if c_jac != 0.0:
        v += c_jac * (zm @ (c.jacobian(0.0, w, **form) @ xm))
    if c_mass != 0.0:
        v += c_mass * (zm @ (c.mass(w, **form) @ xm))
    return v


def _bilinear(op, z, x):
    """op(z, x) real bilinear, extended to complex z and x."""
    zr, zi, xr, xi = np.real(z), np.imag(z), np.real(x), np.imag(x)
    return (op(zr, xr) - op(zi, xi)) + 1j * (op(zr, xi) + op(zi, xr))


def s_vector(c, w, lam, x, z, **form):
    hj = _bilinear(lambda a, b: state_gradient(c, w, b, a, 1.0, 0.0, **form), z, x)
    hb = _bilinear(lambda a, b: state_gradient(c, w, b, a, 0.0, 1.0, **form), z, x)
    return hj + lam * hb


def pairing(c, x, z):
    _, B = c.operators()
    return z @ (B @ x)


def base_flow_sensitivity(c, lam, x, z):
    return -s_vector(c, c.w, lam, x, z) / pairing(c, x, z)


def _e_real(c, w, z, x, **form):
    W = _cells(c, w).clone().requires_grad_(True)
    d = torch.zeros(len(c.mesh.tets), 4, 3, dtype=_T, requires_grad=True)
    gW, = torch.autograd.grad(_theta(c, W, _cells(c, masked(c, z)), d, **form), W, create_graph=True)
    gd, = torch.autograd.grad(torch.sum(gW * _cells(c, masked(c, x))), d)
    return _scatter3(c, gd.numpy())


def e_vector(c, x, z):
    """E = D_w[B(w)^T z][x] at the case's state, exactly (theta = z . R(w; d) is linear in d: E = d/dd of x . d theta / dw)."""
    return _bilinear(lambda a, b: _e_real(c, c.w, a, b), z, x)


def fd_step(c, x, fd_rel):
    wu = np.abs(c.w.reshape(-1, 4)[:, :3]).max()
    xu = max(np.abs(np.real(x).reshape(-1, 4)[:, :3]).max(), np.abs(np.imag(x).reshape(-1, 4)[:, :3]).max())
    return fd_rel * wu / xu


def e_vector_fd(c, x, z, fd_rel=1e-5):
    """E as the library takes it: central differences of B^T z along the masked real and imaginary parts of x."""
    h = fd_step(c, x, fd_rel)

    def op(a, b):
        bm = masked(c, b)
        return (mass_transpose(c, c.w + h * bm, a) - mass_transpose(c, c.w - h * bm, a)) / (2.0 * h)
    return _bilinear(op, z, x)


def forcing_sensitivity(c, lam, x, z, inner_rtol=0.0, E=None, seed=0, with_e=True):
    J, B = c.operators()
    gw = base_flow_sensitivity(c, lam, x, z)
    solve = SO.Solver(sp.csr_matrix(J.T), B, 0.0, c.constrained, inner_rtol, seed)
    y = solve(gw.real) + 1j * solve(gw.imag)
    y[c.constrained] = 0.0
    out = B.T @ y
    if with_e:
        out = out + (e_vector(c, x, z) if E is None else E) / pairing(c, x, z)
    return out


def seeded_force(c, seed=1):
    """The random nodal force of the checks against re-converged states (standard normal, seed fixed): pressure slots and
    constrained dofs 0.  On duct633, mode 0 it gives grad_f lam . f = -0.0064397 - 0.0329414i, the first term alone
    +0.1268 + 0.0584i."""
    f = np.random.default_rng(seed).standard_normal(len(c.w))
    f[3::4] = 0.0
    f[c.constrained] = 0.0
    return f


@functools.lru_cache(maxsize=None)
def forced_state(name, eps, seed=1):
    c = SO.case(name)
    w, _ = NS.newton(c.mesh.points, c.mesh.tets, c.mask, c.g, c.Re, c.w.copy(), tol=1e-13, f=eps * seeded_force(c, seed))
    return w


@functools.lru_cache(maxsize=None)
def forced_eigenvalue(name, eps, lam, seed=1):
    """The eigenvalue nearest lam of the pencil at the state re-converged under the force eps f."""
    c = SO.case(name)
    w, f = forced_state(name, eps, seed), eps * seeded_force(c, seed)
    spec = SO.dense_spectrum(c.jacobian(0.0, w, f=f), c.mass(w, f=f), c.constrained)
    return spec[np.abs(spec - lam).argmin()]


def forcing_fd(name, eps, lam, seed=1):
    return (forced_eigenvalue(name, eps, lam, seed) - forced_eigenvalue(name, -eps, lam, seed)) / (2.0 * eps)


@functools.lru_cache(maxsize=None)
def exact_pairs(name):
    """(lam, X, Z) of left_modes_oracle.exact_pairs at the case's state, computed once."""
    c = SO.case(name)
    return LO.exact_pairs(*c.operators(), c.constrained)


@functools.lru_cache(maxsize=None)
def exact_sensitivities(name, k=0):
    """(grad_w lam, grad_f lam, E) of exact pair k, computed once and left unchanged."""
    c = SO.case(name)
    lam, X, Z = exact_pairs(name)
    E = e_vector(c, X[:, k], Z[:, k])
    return base_flow_sensitivity(c, lam[k], X[:, k], Z[:, k]), forcing_sensitivity(c, lam[k], X[:, k], Z[:, k], E=E), E


def forcing_formula_error(name, eps, k=0):
    """(relative difference, prediction, difference quotient): grad_f lam . f against the central difference of the dense
    spectra of the states re-converged under +- eps f, f = seeded_force."""
    c = SO.case(name)
    lam = exact_pairs(name)[0][k]
    pred = exact_sensitivities(name, k)[1] @ seeded_force(c)
    fd = forcing_fd(name, eps, complex(lam))
    return abs(pred - fd) / abs(fd), pred, fd


def lumped_volume(points, tets):
    X = np.asarray(points)[np.asarray(tets)]
    vol = np.abs(np.linalg.det(np.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 3] - X[:, 0]], axis=2))) / 6.0
    out = np.zeros(len(points))
    np.add.at(out, np.asarray(tets).reshape(-1), np.repeat(0.25 * vol, 4))
    return out
