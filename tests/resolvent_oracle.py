"""CPU oracle of the resolvent analysis (plain helper module of tests/test_host_resolvent.py and tests/test_gpu_resolvent.py, not a
conftest), on top of tests/stability_oracle.py, whose cases supply the oracle's J and B:

    mass_matrix(mesh)            the consistent P1 Galerkin mass matrix M on the three velocity components from the mesh: per tet
                                 |det J| (1 + delta_ab) / 120, pressure rows and columns 0; no mask
    energy_matrix(case, weight)  Q = P D M D P: the nodal weight on both sides, then rows and columns of constrained dofs zeroed
                                 (the library reads constrained entries as 0 and writes 0 on constrained rows)
    lumped(mesh)                 the lumped nodal volumes in the layout of a dof vector: a quarter of the incident tets' volumes
                                 in the velocity slots, 0 in the pressure slot
    forcing_scale(case, weight)  the diagonal of S = D_f M_L^-1/2: 0 on pressure and constrained dofs
    Resolvent                    T = S B^T A^-H Q A^-1 B S with A = J + i omega B by scipy's complex sparse LU (one factorisation,
                                 the adjoint solve through trans="H"); inner_rtol > 0 perturbs each solve to that relative
                                 residual (a random complex residual on the free dofs, solved exactly and added), the emulation
                                 of an inner Krylov tolerance in the manner of stability_oracle.Solver
    dense_T / dense_gains        T as a dense Hermitian matrix over all dofs, column by column with exact solves, and the square
                                 roots of its eigenvalues in descending order
    lanczos(...)                 the algorithm of sns_resolvent_lanczos in numpy: start vector zeroed on pressure and constrained
                                 dofs and normalised, per step T v, classical Gram-Schmidt twice in the complex inner product,
                                 breakdown by the norm ratio
    relation / skew / gains      |T V_m - V_{m+1} H|_F / |H|_F with exact solves; |H_m - H_m^H|_F / |H_m|_F; the square roots of the
                                 eigenvalues of the Hermitian part of H_m, descending
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import stability_oracle as SO


def _abs_det(mesh):
    X = np.asarray(mesh.points, dtype=np.float64)[np.asarray(mesh.tets)]
    return np.abs(np.linalg.det(np.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 3] - X[:, 0]], axis=2)))


def mass_matrix(mesh):
    tets = np.asarray(mesh.tets, dtype=np.int64)
    n = len(mesh.points)
    ad = _abs_det(mesh)
    rows, cols, vals = [], [], []
    for a in range(4):
        for b in range(4):
            for c in range(3):
                rows.append(4 * tets[:, a] + c)
                cols.append(4 * tets[:, b] + c)
                vals.append(ad * ((2.0 if a == b else 1.0) / 120.0))
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(4 * n, 4 * n))


def nodal_to_dofs(weight, n):
    return np.ones(4 * n) if weight is None else np.repeat(np.asarray(weight, dtype=np.float64), 4)


def energy_matrix(case, weight=None):
    n = len(case.mesh.points)
    D = sp.diags(nodal_to_dofs(weight, n))
    P = sp.diags((~case.constrained).astype(np.float64))
    return sp.csr_matrix(P @ D @ mass_matrix(case.mesh) @ D @ P)


def lumped(mesh):
    tets = np.asarray(mesh.tets, dtype=np.int64)
    node = np.zeros(len(mesh.points))
    np.add.at(node, tets.reshape(-1), np.repeat(_abs_det(mesh) / 24.0, 4))
    out = np.repeat(node, 4)
    out[3::4] = 0.0
    return out


def forcing_scale(case, weight=None):
    ml = lumped(case.mesh)
    s = np.zeros(len(ml))
    on = (ml > 0.0) & ~case.constrained
    s[on] = nodal_to_dofs(weight, len(case.mesh.points))[on] / np.sqrt(ml[on])
    return s


class Resolvent:
    """T of one case at one frequency with its weights; apply(v) = T v with the solves at inner_rtol."""

    def __init__(self, case, omega, forcing_weight=None, response_weight=None, inner_rtol=0.0, seed=0):
        J, B = case.operators()
        self.case, self.B = case, B
        self.A = sp.csc_matrix(J.astype(complex) + 1j * float(omega) * B)
        self.lu = spla.splu(self.A)
        self.Q = energy_matrix(case, response_weight)
        self.s = forcing_scale(case, forcing_weight)
        self.free = ~case.constrained
        self.inner_rtol = inner_rtol
        self.rng = np.random.default_rng(seed)

    def solve(self, b, adjoint=False, exact=False):
        trans = "H" if adjoint else "N"
        b = np.asarray(b, dtype=complex)
        x = self.lu.solve(b, trans=trans)
        nb = np.linalg.norm(b)
        if self.inner_rtol > 0.0 and nb > 0.0 and not exact:
            r = np.where(self.free, self.rng.standard_normal(len(b)) + 1j * self.rng.standard_normal(len(b)), 0.0)
            x = x + self.lu.solve(r * (self.inner_rtol * nb / np.linalg.norm(r)), trans=trans)
        return x

    def response(self, f, exact=True):
        """q = (J + i omega B)^-1 B f."""
        return self.solve(self.B @ f, exact=exact)

    def apply(self, v, exact=False):
        q = self.solve(self.B @ (self.s * v), exact=exact)
        y = self.solve(self.Q @ q, adjoint=True, exact=exact)
        return self.s * (self.B.T @ y)


def dense_T(R):
    n = len(R.s)
    T = np.zeros((n, n), dtype=complex)
    for j in np.nonzero(R.s)[0]:
        e = np.zeros(n)
        e[j] = 1.0
        T[:, j] = R.apply(e, exact=True)
    return T


def dense_gains(R):
    T = dense_T(R)
    lam = np.linalg.eigvalsh(0.5 * (T + T.conj().T))[::-1]
    return np.sqrt(np.maximum(lam, 0.0)), T


def start_vector(case):
    """The default start vector of FlowProblem.resolvent_lanczos (real), before the call's mask."""
    return SO.start_vector(len(case.w)).astype(complex)


def lanczos(R, m=24, start=None, breakdown_rel=1e-6):
    """(V (m+1, ndof) complex rows = basis, H (m+1, m) complex, m_done, reason, ratios)."""
    case = R.case
    n = len(case.w)
    V, H = np.zeros((m + 1, n), dtype=complex), np.zeros((m + 1, m), dtype=complex)
    v = start_vector(case) if start is None else np.array(start, dtype=complex)
    v[case.constrained] = 0.0
    v[3::4] = 0.0
    n0 = np.linalg.norm(v)
    if not n0 > 0.0:
        return V, H, 0, 2, np.zeros(0)
    V[0] = v / n0
    m_done, reason, ratios = 0, 1, []
    for j in range(m):
        u = R.apply(V[j])
        before = np.linalg.norm(u)
        for _ in range(2):
            h = V[:j + 1].conj() @ u
            u = u - V[:j + 1].T @ h
            H[:j + 1, j] += h
        after = np.linalg.norm(u)
        ratios.append(after / before if before > 0.0 else 0.0)
        m_done = j + 1
        if not after > breakdown_rel * before:
            reason = 2
            break
        H[j + 1, j] = after
        V[j + 1] = u / after
    return V, H, m_done, reason, np.array(ratios)


def orthogonality(V, k):
    """max |V V^H - I| over the first k basis vectors."""
    return np.abs(V[:k].conj() @ V[:k].T - np.eye(k)).max()


def relation(R, V, H, m_done):
    k = m_done
    TV = np.stack([R.apply(V[j], exact=True) for j in range(k)], axis=1)
    rows = min(k + 1, V.shape[0])
    return np.linalg.norm(TV - V[:rows].T @ H[:rows, :k]) / np.linalg.norm(H[:rows, :k])


def skew(H, m_done):
    Hk = H[:m_done, :m_done]
    return np.linalg.norm(Hk - Hk.conj().T) / np.linalg.norm(Hk)


def gains(H, m_done):
    Hk = H[:m_done, :m_done]
    lam = np.linalg.eigvalsh(0.5 * (Hk + Hk.conj().T))[::-1]
    return np.sqrt(np.maximum(lam, 0.0))
