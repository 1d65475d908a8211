"""CPU oracle of the left (adjoint) stability modes (plain helper module of tests/test_host_left_modes.py and
tests/test_gpu_left_modes.py, not a conftest): everything on top of tests/stability_oracle.py, whose B = J(1) - J(0) DEFINES
B^T as its transpose.

    mass_transpose_closed_form(...)     y = B^T z element by element in numpy from the closed forms the kernel implements -- an
                                        independent restatement: no Jacobian, no autograd, only the geometry, tau and grad z
    left_arnoldi(...)                   the left process: stability_oracle.arnoldi fed J^T and B^T
    exact_pairs(J, B, constrained)      (lam, X, Z) by scipy.linalg.eig(left=True) on the free dofs: J x = -lam B x,
                                        z^T J = -lam z^T B (unconjugated), columns over all dofs, scaled so that z^T B x = 1
    drift(lam, z, x, dJ, dB, B)         the perturbation formula -z^T (dJ + lam dB) x / (z^T B x)
    state_at / operators_at             the re-converged steady state and (J, B) of a case at another Reynolds number
    reynolds_formula / reynolds_fd      d lam / d Re of one eigenvalue by the formula with exact modes and central differences of
                                        the operators at Re (1 +- eps), and by the central difference of the dense spectra there
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

import ns3d_oracle as NS
import stability_oracle as SO
from oracle import forms_literal as FL


# ---- B^T z from the closed forms ---------------------------------------------------------------------------------------------
def mass_transpose_closed_form(points, tets, w, z, Re, mask, *, corrected_convection=False, nu_t=None):
    """y = B(w)^T z.  On a P1 tet grad z_c is constant; with the quadrature points q, N_a(q), tau_q and w_q of the form,
        row (a, i) = sum_q w_q N_a z_i(q) + sum_q w_q tau_q N_a (u_q . grad z_i) + pspg sum_q w_q tau_q N_a d_i z_p
    (corrected_convection; otherwise the middle term is sum_q w_q tau_q N_a sum_j u_{q,j} d_i z_j), pressure rows 0.
    Constrained entries of z (all four per node) are read as 0, constrained rows are stored as 0."""
    V = FL.VARIANT
    points, tets = np.asarray(points, dtype=np.float64), np.asarray(tets)
    n, E = len(points), len(tets)
    held = np.asarray(mask).reshape(n, 4).astype(bool)
    Zn = np.where(held, 0.0, np.asarray(z, dtype=np.float64).reshape(n, 4))[tets]              # (E, 4, 4)
    Un = np.asarray(w, dtype=np.float64).reshape(n, 4)[:, :3][tets]                             # (E, 4, 3)
    X = points[tets]
    Jm = np.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 3] - X[:, 0]], axis=2)           # dx_i / dX_j
    K = np.linalg.inv(Jm)
    det = np.abs(np.linalg.det(Jm))
    g = np.einsum("ak,ekj->eaj", FL.GHAT, K)                                                    # d N_a / d x_j
    G = np.einsum("eki,ekj->eij", K, K)
    GG = np.sum(G * G, axis=(1, 2))
    nu = np.full(E, 1.0 / Re) if nu_t is None else np.asarray(nu_t, dtype=np.float64)
    dz = np.einsum("eac,eak->eck", Zn, g)                                                       # dz[e, c, k] = d_k z_c
    out = np.zeros((E, 4, 4))
    for q in range(4):
        xi = np.array([0.25, 0.25, 0.25]) if V["one_point"] else FL.QPTS[q]
        N = np.array([1.0 - xi.sum(), xi[0], xi[1], xi[2]])
        u = np.einsum("a,eaj->ej", N, Un)
        zq = np.einsum("a,eac->ec", N, Zn[:, :, :3])
        tau = 1.0 / np.sqrt(np.einsum("ei,eij,ej->e", u, G, u) + V["ci"] * nu ** 2 * GG)
        wq = FL.QW[q] * det
        if corrected_convection:
            mid = np.einsum("ek,eik->ei", u, dz[:, :3, :])                                      # u . grad z_i
        else:
            mid = np.einsum("ej,eji->ei", u, dz[:, :3, :])                                      # sum_j u_j d_i z_j
        stab = mid + V["pspg"] * dz[:, 3, :]
        for a in range(4):
            out[:, a, :3] += (wq * N[a])[:, None] * zq + (wq * tau * N[a])[:, None] * stab
    y = np.zeros((n, 4))
    np.add.at(y, tets, out)
    y[held] = 0.0
    return y.ravel()


# ---- the left process ----------------------------------------------------------------------------------------------------------
def transposed(J, B):
    return sp.csr_matrix(J.T), sp.csr_matrix(B.T)


def left_arnoldi(J, B, constrained, **kw):
    """stability_oracle.arnoldi on (J^T, B^T): the algorithm of sns_stability_arnoldi_left."""
    return SO.arnoldi(*transposed(J, B), constrained, **kw)


def left_relation(J, B, constrained, shift, V, H, m_done):
    return SO.arnoldi_relation(*transposed(J, B), constrained, shift, V, H, m_done)


def left_mode_residual(J, B, lam, z):
    """|J^T z + lam B^T z| / (|lam| |B^T z|)."""
    return SO.mode_residual(*transposed(J, B), lam, z)


# ---- exact pairs ---------------------------------------------------------------------------------------------------------------
def exact_pairs(J, B, constrained):
    """(lam (k,), X (ndof, k), Z (ndof, k)) of the finite eigenvalues, by QZ on the free dofs: J x = -lam B x and
    z^T J = -lam z^T B (scipy's left vectors satisfy vl^H J = lam vl^H (-B): z = conj(vl)), z^T B x = 1, descending real part."""
    f = ~constrained
    Jf, Bf = J.toarray()[np.ix_(f, f)], B.toarray()[np.ix_(f, f)]
    alpha, vl, vr = sla.eig(Jf, -Bf, left=True, right=True, homogeneous_eigvals=True)
    finite = np.abs(alpha[1]) > 1e-9 * np.abs(alpha[0])
    lam = alpha[0][finite] / alpha[1][finite]
    order = np.lexsort((-lam.imag, -lam.real))
    lam = lam[order]
    X = np.zeros((J.shape[0], len(lam)), dtype=complex)
    Z = np.zeros_like(X)
    X[f] = vr[:, finite][:, order]
    Z[f] = vl[:, finite][:, order].conj()
    Z /= np.einsum("ik,ik->k", Z, B @ X)[None, :]
    return lam, X, Z


def drift(lam, z, x, dJ, dB, B):
    """-z^T (dJ + lam dB) x / (z^T B x), unconjugated."""
    return -(z @ (dJ @ x + lam * (dB @ x))) / (z @ (B @ x))


# ---- other Reynolds numbers ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def state_at(name, Re):
    """The steady state of the case's duct at the Reynolds number Re, by the oracle's Newton from the case's state."""
    c = SO.case(name)
    w, _ = NS.newton(c.mesh.points, c.mesh.tets, c.mask, c.g, float(Re), c.w.copy(), tol=1e-13)
    return w


@functools.lru_cache(maxsize=None)
def operators_at(name, Re):
    """(J, B) at state_at(name, Re) and that Reynolds number."""
    c = SO.case(name)
    w = state_at(name, Re)

    def jac(sigma):
        J, _ = NS.assemble(c.mesh.points, c.mesh.tets, w, float(Re), c.mask, c.g, sigma=sigma, d=None if sigma == 0.0 else -sigma * w)
        return sp.csr_matrix(J)
    J0 = jac(0.0)
    return J0, sp.csr_matrix(jac(1.0) - J0)


def operator_differences(name, eps):
    """(dJ/dRe, dB/dRe) by central differences between the re-converged states at Re (1 +- eps)."""
    Re = SO.case(name).Re
    (Jp, Bp), (Jm, Bm) = operators_at(name, Re * (1.0 + eps)), operators_at(name, Re * (1.0 - eps))
    h = 2.0 * eps * Re
    return (Jp - Jm) / h, (Bp - Bm) / h


def reynolds_formula(name, lam, z, x, eps):
    """d lam / d Re by the perturbation formula with the modes (z, x) of lam at the case's state."""
    _, B = SO.case(name).operators()
    dJ, dB = operator_differences(name, eps)
    return drift(lam, z, x, dJ, dB, B)


def reynolds_fd(name, lam, eps):
    """d lam / d Re by the central difference of the dense spectra at Re (1 +- eps): the eigenvalue nearest lam on each side
    (eps small against the gaps of the spectrum)."""
    c = SO.case(name)
    ends = []
    for sign in (1.0, -1.0):
        spec = SO.dense_spectrum(*operators_at(name, c.Re * (1.0 + sign * eps)), c.constrained)
        ends.append(spec[np.abs(spec - lam).argmin()])
    return (ends[0] - ends[1]) / (2.0 * eps * c.Re)


def wavemaker(z, x, B):
    """|z_u(node)| |x_u(node)| / |z^T B x| per node."""
    zu = np.linalg.norm(z.reshape(-1, 4)[:, :3], axis=1)
    xu = np.linalg.norm(x.reshape(-1, 4)[:, :3], axis=1)
    return zu * xu / abs(z @ (B @ x))
