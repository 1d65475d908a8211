"""CPU oracle of the thick-restarted (Krylov-Schur) stability analysis (plain helper module of tests/test_host_krylov_schur.py and
tests/test_gpu_krylov_schur.py, not a conftest), on top of tests/stability_oracle.py:

    extend(solve, B, constrained, V, H, k, m, breakdown_rel)   the arithmetic of stability_oracle.arnoldi from column k: per step one
                                                               solve, constrained dofs zeroed, classical Gram-Schmidt with one
                                                               re-orthogonalisation against ALL earlier columns, breakdown by
                                                               the norm ratio -- the algorithm of sns_stability_arnoldi_extend
    restarted(...)                                             the loop of solver.linear_stability(max_restarts > 0) on one side:
                                                               m steps, then estimates (solver.krylov_ritz_pairs), the PACKAGE's
                                                               krylov_schur_truncate, the rotation V <- Q^T V in numpy, extend
    StandIn                                                    a problem object for solver.linear_stability on CPU tensors: the
                                                               oracle's J, B and LU behind the four methods the function calls
"""
from __future__ import annotations

import types

import numpy as np
import scipy.sparse as sp
import torch

import stability_oracle as SO
from stabilized_navier_stokes_flow_fenicsx_amd import solver as S


def extend(solve, B, constrained, V, H, k, m, breakdown_rel=1e-6):
    """Steps j = k .. m - 1 on V (m + 1, ndof) and H (m + 1, m) in place; (m_done, reason): 1 all steps, 2 breakdown."""
    m_done = k
    for j in range(k, m):
        w = solve(B @ V[j])
        w[constrained] = 0.0
        before = np.linalg.norm(w)
        for _ in range(2):
            h = V[:j + 1] @ w
            w = w - V[:j + 1].T @ h
            H[:j + 1, j] += h
        after = np.linalg.norm(w)
        m_done = j + 1
        if not after > breakdown_rel * before:
            V[j + 1:] = 0.0
            return m_done, 2
        H[j + 1, j] = after
        V[j + 1] = w / after
    return m_done, 1


def first_cycle(solve, B, constrained, m, start=None, breakdown_rel=1e-6):
    """stability_oracle.arnoldi with the solver given: (V, H, m_done, reason)."""
    n = B.shape[0]
    V, H = np.zeros((m + 1, n)), np.zeros((m + 1, m))
    v = SO.start_vector(n) if start is None else np.array(start, dtype=np.float64)
    v[constrained] = 0.0
    t = solve(B @ v)
    t[constrained] = 0.0
    V[0] = t / np.linalg.norm(t)
    m_done, reason = extend(solve, B, constrained, V, H, 0, m, breakdown_rel)
    return V, H, m_done, reason


def leading_converged(H, m_done, shift, n_modes, tol):
    """(all of the n_modes Ritz pairs nearest the shift are within tol, lam, est, their indices)."""
    lam, _, est = S.krylov_ritz_pairs(H, m_done, shift)
    lead = np.argsort(np.abs(lam - shift), kind="stable")[:n_modes]
    return bool((est[lead] <= tol).all()), lam, est, lead


def restarted(J, B, constrained, shift, m, keep, n_modes, max_restarts, tol, inner_rtol, left=False, seed=0, breakdown_rel=1e-6,
              after_restart=None):
    """One side of the restarted analysis.  Returns (V, H, restarts, eigenvalues, info): eigenvalues = the n_modes Ritz values
    nearest the shift, info = dict(m_done, reason, converged, estimates, solves).  after_restart(V, H, m_done), if given, is
    called after every restart's extension (the tests hang their per-restart checks there)."""
    if left:
        J, B = sp.csr_matrix(J.T), sp.csr_matrix(B.T)
    solve = SO.Solver(J, B, shift, constrained, inner_rtol, seed)
    count = types.SimpleNamespace(n=0)

    def counted(b):
        count.n += 1
        return solve(b)

    V, H, m_done, reason = first_cycle(counted, B, constrained, m, breakdown_rel=breakdown_rel)
    restarts = 0
    while True:
        done, lam, est, lead = leading_converged(H, m_done, shift, n_modes, tol)
        if reason != 1 or done or restarts >= max_restarts:
            break
        k, Q, Hk = S.krylov_schur_truncate(H, m_done, keep)
        V[:k + 1] = Q.T @ V[:m_done + 1]
        V[k + 1:] = 0.0
        H[:] = 0.0
        H[:k + 1, :k] = Hk
        m_done, reason = extend(counted, B, constrained, V, H, k, m, breakdown_rel)
        restarts += 1
        if after_restart is not None:
            after_restart(V, H, m_done)
    return V, H, restarts, lam[lead], dict(m_done=m_done, reason=reason, converged=done, estimates=est[lead], solves=count.n)


class StandIn:
    """What solver.linear_stability asks of a problem, on CPU torch tensors with the oracle's operators and LU solves
    (inner_rtol emulates the inner tolerance).  calls: the names of the methods called, in order."""

    def __init__(self, J, B, constrained, inner_rtol=0.0):
        self.J, self.B, self.constrained = J, B, constrained
        self.JT, self.BT = sp.csr_matrix(J.T), sp.csr_matrix(B.T)
        self.inner_rtol = inner_rtol
        self.ndof = J.shape[0]
        self.options = types.SimpleNamespace(ksp_rtol=1e-8)
        self.calls = []

    def set_options(self, **kw):
        for name, value in kw.items():
            setattr(self.options, name, value)

    def _side(self, side, shift):
        J, B = (self.J, self.B) if side == "right" else (self.JT, self.BT)
        return SO.Solver(J, B, shift, self.constrained, self.inner_rtol), B

    def stability_arnoldi(self, w, shift=0.0, m=64, start=None, breakdown_rel=1e-6, side="right"):
        self.calls.append("stability_arnoldi")
        solve, B = self._side(side, shift)
        V, H, m_done, reason = first_cycle(solve, B, self.constrained, m, start=start, breakdown_rel=breakdown_rel)
        return torch.from_numpy(V), H, S.ArnoldiResult(m_done, reason, m_done + 1)

    def stability_arnoldi_extend(self, w, V, H, k, shift=0.0, breakdown_rel=1e-6, side="right"):
        self.calls.append("stability_arnoldi_extend")
        solve, B = self._side(side, shift)
        m_done, reason = extend(solve, B, self.constrained, V.numpy(), H, k, H.shape[1], breakdown_rel)
        return S.ArnoldiResult(m_done, reason, m_done - k)

    def basis_rotate(self, V, Q):
        self.calls.append("basis_rotate")
        n_in, n_out = Q.shape
        Vn = V.numpy()
        Vn[:n_out] = Q.T @ Vn[:n_in]
        Vn[n_out:n_in] = 0.0
        return V

    def mass_apply(self, w, x):
        return torch.from_numpy(self.B @ x.numpy())
