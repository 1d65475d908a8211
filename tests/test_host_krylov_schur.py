"""CPU checks behind the thick-restarted stability analysis (sns_stability_arnoldi_extend, sns_basis_rotate;
solver.krylov_schur_truncate, solver.krylov_ritz_pairs, solver.linear_stability(max_restarts > 0)): the restarted process of the
oracle (tests/krylov_schur_oracle.py: the arithmetic of stability_oracle.arnoldi with the PACKAGE's truncation) against the
dense spectrum, with orthogonality and the Krylov relation after every restart; the truncation alone on random matrices;
linear_stability end to end through a CPU stand-in problem; the argument rule of the extension through its stand-alone main
(tests/extend_request_main.cpp); the binding.  The bounds are conditions on the oracle and on pure-numpy code."""
import ctypes as C
import functools
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import krylov_schur_oracle as KO
import request_gate as RG
import stability_oracle as SO
from conftest import ROOT
from stabilized_navier_stokes_flow_fenicsx_amd import solver as S

E_ARG, E_STATE = -1, -3
TOL = 1e-7
PARAMS = ((12, 6, 4), (16, 8, 6))
SHIFTS = (0.0, 2.5)


@functools.lru_cache(maxsize=None)
def dense_spectrum(name):
    c = SO.case(name)
    return SO.dense_spectrum(*c.operators(), c.constrained)


@functools.lru_cache(maxsize=None)
def oracle_run(name, shift, params, inner_rtol):
    """One restarted run of the oracle with the per-restart figures: (restarts, eigenvalues, info, worst orthogonality, worst
    Krylov relation) over the restarts taken."""
    c = SO.case(name)
    J, B = c.operators()
    m, keep, n_modes = params
    seen = []

    def after_restart(V, H, m_done):
        seen.append((SO.orthogonality(V, m_done + 1), SO.arnoldi_relation(J, B, c.constrained, shift, V, H, m_done)))

    V, H, restarts, lam, info = KO.restarted(J, B, c.constrained, shift, m, keep, n_modes, 20, TOL, inner_rtol,
                                             after_restart=after_restart)
    assert len(seen) == restarts
    return restarts, lam, info, max(o for o, _ in seen), max(r for _, r in seen)


# ---- 1. the restarted process of the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("inner_rtol", [0.0, 1e-10])
@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("shift", SHIFTS)
def test_restarted_oracle_converges_to_the_dense_spectrum(shift, params, inner_rtol):
    """duct633: convergence of the n_modes pairs nearest the shift within 20 restarts (a condition, not a tolerance: 6 - 13 were
    seen); after every restart orthogonality <= 1e-12 and, with exact solves, the Krylov relation on the non-Hessenberg H
    <= 1e-12 (3e-15 - 6e-15 seen); the converged eigenvalues within 10 tol relative of the dense spectrum (2e-8 - 9e-8 seen)."""
    restarts, lam, info, orth, rel = oracle_run("duct633", shift, params, inner_rtol)
    worst = SO.nearest(dense_spectrum("duct633"), lam).max()
    print(shift, params, inner_rtol, "restarts", restarts, "solves", info["solves"], "orthogonality", orth, "relation", rel,
          "worst distance", worst, "estimates", info["estimates"].max())
    assert info["converged"] and info["reason"] == 1 and 1 <= restarts <= 20
    assert orth <= 1e-12
    if inner_rtol == 0.0:
        assert rel <= 1e-12
    assert len(lam) == params[2] and worst <= 10.0 * TOL


def test_the_kept_values_are_the_eigenvalues_nearest_the_shift():
    """What the restarted run converges to is what the analysis is after: the n_modes dense eigenvalues nearest the shift."""
    dense = dense_spectrum("duct633")
    for shift, params in itertools.product(SHIFTS, PARAMS):
        _, lam, _, _, _ = oracle_run("duct633", shift, params, 0.0)
        target = dense[np.argsort(np.abs(dense - shift))][:params[2]]
        assert SO.nearest(np.concatenate([lam, lam.conj()]), target).max() <= 10.0 * TOL, (shift, params)    # (the cut may hold one member of a pair)


# ---- 2. the truncation alone -----------------------------------------------------------------------------------------------------
def _random_h(rng, m, full_row, pairs=True):
    """(m + 1, m): a Hessenberg block (or, pairs=False, a symmetric one: a real spectrum) and a last row e_m or full."""
    A = np.triu(rng.standard_normal((m, m)), -1)
    if not pairs:
        A = rng.standard_normal((m, m))
        A = A + A.T
    H = np.zeros((m + 1, m))
    H[:m] = A
    H[m] = rng.standard_normal(m) if full_row else 0.0
    if not full_row:
        H[m, m - 1] = abs(rng.standard_normal()) + 0.1
    return H


@pytest.mark.parametrize("full_row", [False, True])
def test_truncation_on_random_matrices(full_row):
    rng = np.random.default_rng(11 + full_row)
    seen_cut, seen_whole = 0, 0
    for trial in range(60):
        m = int(rng.integers(6, 20))
        keep = int(rng.integers(2, m - 1))
        H = _random_h(rng, m, full_row)
        k, Q, Hk = S.krylov_schur_truncate(H, m, keep)
        theta = np.linalg.eigvals(H[:m, :m])
        theta = theta[np.argsort(-np.abs(theta), kind="stable")]
        inside = theta[keep - 1].imag != 0.0 and abs(theta[keep] - theta[keep - 1].conj()) <= 1e-12 * abs(theta[0])
        assert k == (keep - 1 if inside else keep), (trial, m, keep, k)
        seen_cut += inside
        seen_whole += not inside
        assert Q.shape == (m + 1, k + 1) and Hk.shape == (k + 1, k)
        assert np.abs(Q.T @ Q - np.eye(k + 1)).max() <= 1e-13
        assert Q[m, k] == 1.0 and not Q[m, :k].any() and not Q[:m, k].any()
        scale = np.abs(H).max()
        assert np.abs(Q[:m, :k].T @ H[:m, :m] @ Q[:m, :k] - Hk[:k]).max() <= 1e-13
        assert np.abs(H[m, :m] @ Q[:m, :k] - Hk[k]).max() <= 1e-13 * max(1.0, scale) * m
        # the kept Ritz values are the k of largest modulus
        kept = np.linalg.eigvals(Hk[:k])
        assert np.abs(np.sort(np.abs(kept))[::-1] - np.abs(theta[:k])).max() <= 1e-10 * abs(theta[0])
        assert np.abs(kept).min() > np.abs(theta[k:]).max() * (1.0 - 1e-10)
        # the decomposition is preserved: with S V = V A + v b^T for a random orthonormal [V v], (V Q)_k Hk is S (V Q)_k
        n = m + 5
        W, _ = np.linalg.qr(rng.standard_normal((n, m + 1)))
        SV = W @ H                                         # S V_m, whatever S is
        assert np.abs(SV @ Q[:m, :k] - (W @ Q) @ Hk).max() <= 1e-12 * max(1.0, scale) * m
    assert seen_cut >= 5 and seen_whole >= 5


def test_truncation_of_a_real_spectrum_keeps_keep():
    rng = np.random.default_rng(3)
    for _ in range(20):
        m = int(rng.integers(6, 20))
        keep = int(rng.integers(1, m))
        H = _random_h(rng, m, True, pairs=False)
        k, Q, Hk = S.krylov_schur_truncate(H, m, keep)
        assert k == keep
        assert np.abs(np.tril(Hk[:k], -1)).max() == 0.0 if k > 1 else True      # a real spectrum: T is triangular


def test_truncation_refuses_what_it_cannot_cut():
    H = _random_h(np.random.default_rng(0), 8, True)
    for keep in (0, 8, 9, -1):
        with pytest.raises(ValueError):
            S.krylov_schur_truncate(H, 8, keep)
    with pytest.raises(ValueError):
        S.krylov_schur_truncate(H, 1, 1)
    with pytest.raises(ValueError):
        S.krylov_schur_truncate(H[:8], 8, 4)                # the row behind the block is missing


def test_krylov_ritz_pairs_is_ritz_pairs_on_hessenberg_input_and_sees_a_full_row():
    rng = np.random.default_rng(8)
    H = _random_h(rng, 12, False)
    lam, Y, est = S.ritz_pairs(H, 12, 0.5)
    lam2, Y2, est2 = S.krylov_ritz_pairs(H, 12, 0.5)
    assert np.array_equal(lam, lam2) and np.array_equal(Y, Y2)
    assert np.abs(est - est2).max() <= 1e-15 * est.max()
    # a full last row: the estimate is the residual of the pair in S V = V A + v b^T
    H = _random_h(rng, 12, True)
    lam, Y, est = S.krylov_ritz_pairs(H, 12, 0.0)
    theta = -1.0 / lam
    assert np.abs(est - np.abs(H[12, :12] @ Y) / np.abs(theta)).max() <= 1e-13 * est.max()
    lam0, Y0, est0 = S.krylov_ritz_pairs(H, 0)
    assert len(lam0) == 0 and Y0.shape == (0, 0) and len(est0) == 0


def test_default_keep():
    assert S.default_keep(12, 4) == 6 and S.default_keep(16, 6) == 8 and S.default_keep(64, 6) == 32
    assert S.default_keep(8, 6) == 6 and S.default_keep(10, 3) == 5


# ---- 3. linear_stability through a stand-in problem ----------------------------------------------------------------------------
@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("shift", SHIFTS)
def test_linear_stability_restarted_through_a_stand_in(shift, params):
    """The same eigenvalues as the oracle's loop (the same arithmetic: agreement to the tolerance both stop at), restarts
    reported, the options restored."""
    c = SO.case("duct633")
    m, keep, n_modes = params
    P = KO.StandIn(*c.operators(), c.constrained)
    r = S.linear_stability(P, None, n_modes=n_modes, shift=shift, m=m, tol=TOL, max_restarts=20, keep=keep)
    restarts, lam, info, _, _ = oracle_run("duct633", shift, params, 0.0)
    print(shift, params, "restarts", r.restarts, "oracle", restarts, "eigenvalues", r.eigenvalues)
    assert P.options.ksp_rtol == 1e-8
    assert r.restarts == restarts and r.left_restarts == 0 and r.reason == 1 and r.m_done == m
    assert r.converged.all() and len(r.eigenvalues) == n_modes
    # (the oracle lists the n_modes pairs nearest the shift, the function the least stable converged ones: where the cut holds one
    # member of a conjugate pair the two lists differ by a conjugation)
    both = lambda v: np.concatenate([v, v.conj()])
    assert SO.nearest(both(lam), r.eigenvalues).max() <= 10.0 * TOL and SO.nearest(both(r.eigenvalues), lam).max() <= 10.0 * TOL
    assert SO.nearest(dense_spectrum("duct633"), r.eigenvalues).max() <= 10.0 * TOL
    assert P.calls.count("stability_arnoldi") == 1
    assert P.calls.count("basis_rotate") == restarts and P.calls.count("stability_arnoldi_extend") == restarts
    X = r.modes.numpy()
    J, B = c.operators()
    assert max(SO.mode_residual(J, B, l, x) for l, x in zip(r.eigenvalues, X)) <= 100.0 * TOL
    # the default keep is the documented one
    P2 = KO.StandIn(*c.operators(), c.constrained)
    r2 = S.linear_stability(P2, None, n_modes=n_modes, shift=shift, m=m, tol=TOL, max_restarts=20)
    assert S.default_keep(m, n_modes) == keep and r2.restarts == r.restarts and np.array_equal(r2.eigenvalues, r.eigenvalues)


def test_without_restarts_the_new_methods_are_never_called():
    c = SO.case("duct633")
    P = KO.StandIn(*c.operators(), c.constrained)
    r0 = S.linear_stability(P, None, n_modes=4, m=12, tol=TOL)
    r1 = S.linear_stability(P, None, n_modes=4, m=12, tol=TOL, max_restarts=0, keep=5)
    assert P.calls == ["stability_arnoldi", "stability_arnoldi"]
    assert r0.restarts == 0 and r1.restarts == 0
    assert np.array_equal(r0.eigenvalues, r1.eigenvalues) and np.array_equal(r0.estimates, r1.estimates)
    assert np.array_equal(r0.modes.numpy(), r1.modes.numpy())
    # a cap that is reached is reported as it is: unconverged pairs, the cap's count
    r2 = S.linear_stability(P, None, n_modes=4, m=12, tol=TOL, max_restarts=1)
    assert r2.restarts == 1 and not r2.converged.all()
    with pytest.raises(ValueError):
        S.linear_stability(P, None, n_modes=4, m=12, max_restarts=3, keep=12)


def test_left_modes_of_a_restarted_run_pair_every_right_mode():
    c = SO.case("duct633")
    J, B = c.operators()
    P = KO.StandIn(J, B, c.constrained)
    r = S.linear_stability(P, None, n_modes=6, m=16, tol=TOL, left=True, max_restarts=20, keep=8)
    print("restarts", r.restarts, "left", r.left_restarts, "eigenvalues", r.eigenvalues)
    assert r.converged.all() and r.left_converged.all() and r.restarts >= 1 and r.left_restarts >= 1
    assert r.left_reason == 1 and r.left_m_done == 16
    X, Z = r.modes.numpy(), r.left_modes.numpy()
    pairing = np.array([Z[k] @ (B @ X[k]) for k in range(6)])
    assert np.abs(pairing - 1.0).max() <= 1e-10
    assert np.abs(r.left_eigenvalues - r.eigenvalues).max() <= 1e-5 * np.abs(r.eigenvalues).max()


def test_breakdown_in_the_first_cycle_of_a_restarted_run():
    """duct322: 9 free velocity dofs, the exact process ends at step 8 - 9 of the first cycle (m = 12): reason 2, no restart,
    finite eigenvalues that are dense eigenvalues."""
    c = SO.case("duct322")
    J, B = c.operators()
    P = KO.StandIn(J, B, c.constrained)
    r = S.linear_stability(P, None, n_modes=4, m=12, tol=TOL, max_restarts=20)
    print("m_done", r.m_done, "reason", r.reason, "eigenvalues", r.eigenvalues)
    assert r.reason == 2 and r.m_done <= 9 and r.restarts == 0 and P.calls == ["stability_arnoldi"]
    assert np.isfinite(r.eigenvalues).all() and len(r.eigenvalues) == 4
    assert SO.nearest(dense_spectrum("duct322"), r.eigenvalues).max() <= 1e-6


# ---- 4. the argument rule of the extension -------------------------------------------------------------------------------------
def test_extend_request_rules(tmp_path):
    """check_arnoldi_extend_args behind the stability rows, every combination of the nine facts, both sides, the m / shift /
    breakdown_rel sweep of the Arnoldi request and k in {0, 1, m - 1, m, -1}, against a transcription written here: the
    dimension, m, the shift, breakdown_rel, k (all SNS_E_ARG), then the state.  For a valid k the verdict is the plain
    request's."""
    K_TEXT = "k must lie in [1, m - 1]"

    def expected(dim, part, tt, vl, m, shift, brel, k):
        shift, brel = float(shift), float(brel)
        checks = [(dim != 3, E_ARG, "3-D handles only"),
                  (not 2 <= m <= 64, E_ARG, "m must lie in [2, 64]"),
                  (not (shift >= 0.0 and math.isfinite(shift)), E_ARG, "the shift must be finite and >= 0"),
                  (not 0.0 < brel < 1.0, E_ARG, "breakdown_rel must lie in (0, 1)"),
                  (not 1 <= k <= m - 1, E_ARG, K_TEXT),
                  (part, E_STATE, "not with a communicator attached (partitioned stability analysis is not built)"),
                  (vl, E_STATE, "not with a viscosity law set (the mass operator of the law's form is not built)"),
                  (tt, E_STATE, "not with a time term set (the analysis sets its own and clears it)")]
        return next(((code, tail) for cond, code, tail in checks if cond), (0, ""))

    exe = RG.policy_main(tmp_path, "extend_request")
    args = [(64, "0", "1e-6"), (2, "2.5", "0.5"), (1, "0", "1e-6"), (65, "0", "1e-6"), (0, "0", "1e-6"), (-3, "0", "1e-6"),
            (32, "-1e-300", "1e-6"), (32, "-2", "1e-6"), (32, "nan", "1e-6"), (32, "inf", "1e-6"), (32, "1e308", "1e-6"),
            (32, "0", "0"), (32, "0", "1"), (32, "0", "-0.1"), (32, "0", "nan"), (32, "0", "1.5"), (32, "0", "1e-300"),
            (65, "nan", "2"), (1, "-1", "0")]
    questions = [(left, f, a, k) for left in (0, 1) for f in RG.FACTS for a in args for k in (0, 1, a[0] - 1, a[0], -1)]
    assert len(questions) == 2 * 2 ** 9 * 19 * 5
    text = "".join(" ".join(map(str, (left,) + tuple(f) + a + (k,))) + "\n" for left, f, a, k in questions)
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.returncode
    lines = run.stdout.split("\n")
    assert list(map(int, lines[0].split())) == [2, 4, 2, 64]                       # no new request kind
    rows = [ln.split("\t") for ln in lines[1:1 + len(questions)]]
    assert len(rows) == len(questions) and lines[1 + len(questions):] == [""]
    got, right = set(), {}
    for (left, f, a, k), (code, tail, pcode, ptail) in zip(questions, rows):
        want = expected(*f[:RG.VL + 1], *a, k)
        assert (int(code), tail) == want, (left, f, a, k, code, tail)
        if 1 <= k <= a[0] - 1:
            assert (code, tail) == (pcode, ptail), (left, f, a, k)              # a valid k: the plain request's verdict
        elif int(pcode) == E_ARG:
            assert (code, tail) == (pcode, ptail)                               # the other arguments come first
        else:
            assert (int(code), tail) == (E_ARG, K_TEXT)                         # ... and k before the state
        if left == 0:
            right[(f, a, k)] = (code, tail)
        else:
            assert right[(f, a, k)] == (code, tail)                             # both sides alike
        got.add((int(code), tail))
    assert got >= {(0, ""), (E_ARG, "3-D handles only"), (E_ARG, "m must lie in [2, 64]"), (E_ARG, K_TEXT),
                   (E_ARG, "the shift must be finite and >= 0"), (E_ARG, "breakdown_rel must lie in (0, 1)"),
                   (E_STATE, "not with a communicator attached (partitioned stability analysis is not built)"),
                   (E_STATE, "not with a viscosity law set (the mass operator of the law's form is not built)"),
                   (E_STATE, "not with a time term set (the analysis sets its own and clears it)")}
    for text in ("2 3 0 0 0 0 0 0 0 0 8 0 1e-6 4\n", "0 3 0 0\n"):
        assert subprocess.run([exe], input=text, capture_output=True, text=True).returncode == 2


# ---- 5. the binding --------------------------------------------------------------------------------------------------------------
def test_restart_entry_points_are_bound(built_lib):
    """Symbols, argtypes, header declarations; a null handle is SNS_E_ARG before any GPU call; the ABI version stays 8."""
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    H, P, D, I, PI = C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.POINTER(C.c_int)
    hdr = open(os.path.join(ROOT, "include", "sns.h")).read()
    for name in ("sns_stability_arnoldi_extend", "sns_basis_rotate"):
        assert name in _lib.SYMBOLS and hasattr(built_lib, name)
        assert ("SNS_API int %s(" % name) in hdr
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert " T sns_stability_arnoldi_extend\n" in nm and " T sns_basis_rotate\n" in nm
    assert built_lib.sns_stability_arnoldi_extend.argtypes == [H, P, D, I, I, D, I, P, P, PI, PI, PI]
    assert built_lib.sns_stability_arnoldi_extend.restype == C.c_int
    assert built_lib.sns_basis_rotate.argtypes == [H, I, I, P, P] and built_lib.sns_basis_rotate.restype == C.c_int
    buf = (C.c_double * 16)()
    a = C.addressof(buf)
    k = C.c_int()
    assert built_lib.sns_stability_arnoldi_extend(None, a, 0.0, 2, 4, 1e-6, 0, a, a, C.byref(k), C.byref(k), C.byref(k)) == E_ARG
    assert b"sns_stability_arnoldi_extend: null" in built_lib.sns_last_error()
    assert built_lib.sns_basis_rotate(None, 2, 1, a, a) == E_ARG
    assert b"sns_basis_rotate: null" in built_lib.sns_last_error()
    assert built_lib.sns_abi_version() == 8


def test_stability_result_gains_the_restart_counts_last():
    r = S.StabilityResult(np.zeros(0, complex), None, np.zeros(0), np.zeros(0, bool), 0, 0, 1)
    assert r.restarts == 0 and r.left_restarts == 0 and r.left_modes is None and r.shift == 0.0
