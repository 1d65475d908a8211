"""CPU oracle of the eigenvalue shape pass and of the shape sensitivity of an eigenvalue (plain helper module of
tests/test_host_eigshape.py and tests/test_gpu_eigshape.py, not a conftest): everything on top of tests/ns3d_oracle.py,
tests/hessian_oracle.py, tests/shape_oracle.py and tests/stability_oracle.py.

    cell_shape_gradients(c, w, x, z, c_jac, c_mass)   (E, 4, 3) d phi_e / d X_e by autograd in X through the oracle's element
                                                      residual, phi_e the Hessian pass's own scalar
                                                      c_J d/d eps [z_e . R_e(W + eps x_e; X_e)] + c_B z_e . (R_e(W; d = x_u) - R_e(W))
    cell_values(...)                                  (E,) phi_e
    shape_contraction_gradient(...)                   (n, 3) gX = d/dX [ z~^T (c_J J0(w; X) + c_B B(w; X)) x~ ], the scatter
    explicit_part / path_part                         -(S_J + lam S_B) / (z^T B x)   and   -mu . dF/dX, A^T mu = grad_w lam, mu_B = 0
    eigenvalue_shape_sensitivity(c, lam, x, z)        their sum, complex (n, 3); inner_rtol: the two LU solves perturbed to that
                                                      relative residual, as stability_oracle.Solver does
    test_field(points)                                the deformation field V of the checks against moved meshes
    moved_state / moved_eigenvalue(name, eps, lam)    Newton at tol 1e-13 and a dense spectrum on the mesh moved by eps V; the
                                                      Dirichlet values stay at the nodes
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp
import torch

import hessian_oracle as HO
import ns3d_oracle as NS
import shape_oracle as SH
import stability_oracle as SO

_T = torch.float64


class JitteredCase:
    """The jittered (4,3,3) duct, 80 nodes and 216 tets, with a random state: what the pass is compared on (it needs no
    converged state).  The attributes the oracles read of a stability_oracle.Case."""

    def __init__(self, shape=(4, 3, 3), Re=50.0, seed=11):
        from stabilized_navier_stokes_flow_fenicsx_amd import bcs as Bc
        from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
        self.mesh = M.duct_mesh(shape, 2.0, jitter=0.2)
        self.mask, self.g = Bc.duct_bcs(self.mesh).flatten()
        self.Re = float(Re)
        self.constrained = self.mask.astype(bool)
        self.w = np.random.default_rng(seed).standard_normal(4 * len(self.mesh.points))

    def jacobian(self, sigma=0.0, w=None, **form):
        return SO.Case.jacobian(self, sigma, w, **form)

    def mass(self, w=None, **form):
        return SO.Case.mass(self, w, **form)


@functools.lru_cache(maxsize=None)
def jittered_case():
    return JitteredCase()


def _phi(c, X, w, x, z, c_jac, c_mass, **form):
    """(E,) phi_e as a torch tensor on the graph of X."""
    W = HO._cells(c, w).clone().requires_grad_(True)
    xe, ze = HO._cells(c, HO.masked(c, x)), HO._cells(c, HO.masked(c, z))
    R = NS.residual(X, W, c.Re, **form)
    phi = torch.zeros(len(c.mesh.tets), dtype=_T)
    if c_jac != 0.0:
        gW, = torch.autograd.grad(torch.sum(ze * R), W, create_graph=True)
        phi = phi + c_jac * torch.sum(gW * xe, dim=1)
    if c_mass != 0.0:
        # R is affine in the history d, so R(W; d = x_u) - R(W) = dR/dd . x_u exactly; taken as that derivative the cell's
        # value carries no cancellation of two O(|R|) residuals (which would cost eps |z||R| whatever the size of the result)
        d = torch.zeros(len(c.mesh.tets), 4, 3, dtype=_T, requires_grad=True)
        gd, = torch.autograd.grad(torch.sum(ze * NS.residual(X, W, c.Re, d=d, **form)), d, create_graph=True)
        phi = phi + c_mass * torch.sum(gd * xe.reshape(-1, 4, 4)[:, :, :3], dim=(1, 2))
    return phi


def cell_values(c, w, x, z, c_jac, c_mass, points=None, **form):
    pts = c.mesh.points if points is None else points
    return _phi(c, torch.as_tensor(pts[c.mesh.tets], dtype=_T), w, x, z, c_jac, c_mass, **form).detach().numpy()


def cell_shape_gradients(c, w, x, z, c_jac, c_mass, points=None, **form):
    """(E, 4, 3) d phi_e / d X_e (x and z are masked here)."""
    pts = c.mesh.points if points is None else points
    X = torch.as_tensor(pts[c.mesh.tets], dtype=_T).clone().requires_grad_(True)
    phi = _phi(c, X, w, x, z, c_jac, c_mass, **form)
    if not phi.requires_grad:                                  # both coefficients 0
        return np.zeros((len(c.mesh.tets), 4, 3))
    g, = torch.autograd.grad(phi.sum(), X)                     # a cell's scalar depends on its own vertices only
    return g.numpy()


def scatter_nodes(c, ge):
    out = np.zeros((len(c.mesh.points), 3))
    np.add.at(out, c.mesh.tets.ravel(), np.asarray(ge).reshape(-1, 3))
    return out


def shape_contraction_gradient(c, w, x, z, c_jac=1.0, c_mass=0.0, **form):
    return scatter_nodes(c, cell_shape_gradients(c, w, x, z, c_jac, c_mass, **form))


def explicit_part(c, lam, x, z):
    sj = HO._bilinear(lambda a, b: shape_contraction_gradient(c, c.w, b, a, 1.0, 0.0), z, x)
    sb = HO._bilinear(lambda a, b: shape_contraction_gradient(c, c.w, b, a, 0.0, 1.0), z, x)
    return -(sj + lam * sb) / HO.pairing(c, x, z)


def path_part(c, lam, x, z, inner_rtol=0.0, seed=0, gw=None):
    J, B = c.operators()
    gw = HO.base_flow_sensitivity(c, lam, x, z) if gw is None else gw
    solve = SO.Solver(sp.csr_matrix(J.T), B, 0.0, c.constrained, inner_rtol, seed)
    out = []
    for part in (gw.real, gw.imag):
        mu = solve(part)
        mu[c.constrained] = 0.0
        out.append(-SH.gradient_3d(c.mesh.points, c.mesh.tets, c.w, mu, c.Re))
    return out[0] + 1j * out[1]


def eigenvalue_shape_sensitivity(c, lam, x, z, inner_rtol=0.0, seed=0, return_parts=False):
    e, p = explicit_part(c, lam, x, z), path_part(c, lam, x, z, inner_rtol, seed)
    return (e + p, e, p) if return_parts else e + p


@functools.lru_cache(maxsize=None)
def exact_shape_sensitivity(name, k=0):
    """(total, explicit, path) of exact pair k of the case, computed once and left unchanged."""
    c = SO.case(name)
    lam, X, Z = HO.exact_pairs(name)
    return eigenvalue_shape_sensitivity(c, lam[k], X[:, k], Z[:, k], return_parts=True)


def test_field(points):
    """V = (0.3 b sin 2y, b (y - 1/2), b (z - 1/2) / 2), b = exp(-((x - 1) / 0.5)^2): boundary and Dirichlet nodes move too."""
    p = np.asarray(points, dtype=np.float64)
    b = np.exp(-((p[:, 0] - 1.0) / 0.5) ** 2)
    return np.stack([0.3 * b * np.sin(2.0 * p[:, 1]), b * (p[:, 1] - 0.5), 0.5 * b * (p[:, 2] - 0.5)], axis=1)


test_field.__test__ = False                                    # a helper, whatever its name says to a collector


def moved_points(name, eps):
    c = SO.case(name)
    return c.mesh.points + eps * test_field(c.mesh.points)


@functools.lru_cache(maxsize=None)
def moved_state(name, eps):
    c = SO.case(name)
    w, _ = NS.newton(moved_points(name, eps), c.mesh.tets, c.mask, c.g, c.Re, c.w.copy(), tol=1e-13)
    return w


@functools.lru_cache(maxsize=None)
def moved_eigenvalue(name, eps, lam):
    """The eigenvalue nearest lam of the pencil on the mesh moved by eps V, at the state re-converged there."""
    c = SO.case(name)
    pts, w = moved_points(name, eps), moved_state(name, eps)

    def jac(sigma):
        d = None if sigma == 0.0 else -sigma * w
        return sp.csr_matrix(NS.assemble(pts, c.mesh.tets, w, c.Re, c.mask, c.g, sigma=sigma, d=d)[0])
    J = jac(0.0)
    spec = SO.dense_spectrum(J, sp.csr_matrix(jac(1.0) - J), c.constrained)
    return spec[np.abs(spec - lam).argmin()]


def formula_error(name, eps, k=0):
    """(relative difference, prediction, difference quotient): d lam / dX . V against the central difference of the dense
    spectra on the meshes moved by +- eps V."""
    c = SO.case(name)
    lam = complex(HO.exact_pairs(name)[0][k])
    pred = np.sum(exact_shape_sensitivity(name, k)[0] * test_field(c.mesh.points))
    fd = (moved_eigenvalue(name, eps, lam) - moved_eigenvalue(name, -eps, lam)) / (2.0 * eps)
    return abs(pred - fd) / abs(fd), pred, fd
