"""CPU checks behind the stability analysis with a complex or negative shift (sns_shifted_apply, sns_shifted_solve,
sns_stability_arnoldi_shifted; solver.shifted_roots, solver.shifted_eigenpairs, solver.linear_stability(shift=complex)): the
oracle's process on Re[(J + s B)^-1 B] (tests/complex_shift_oracle.py) against the dense QZ spectrum; the eigenvalue recovery and
the root selection of the package on a synthetic real pencil with a singular B against scipy.linalg.eig; s and conj(s); a
negative real shift; linear_stability end to end through a CPU stand-in; the argument rules through their stand-alone main
(tests/shifted_request_main.cpp); the binding.  The bounds are conditions on the oracle and on pure-numpy code: TOL = 1e-7 is
the analysis' own convergence tolerance, 10 TOL the distance to the dense spectrum the other stability tests grant a converged
pair."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp
import torch

import complex_shift_oracle as CO
import request_gate as RG
import stability_oracle as SO
from conftest import ROOT
from stabilized_navier_stokes_flow_fenicsx_amd import solver as S

E_ARG, E_STATE = -1, -3
TOL = 1e-7
# the record of the issue: case, shift, the eigenvalues with Im > 0 an unrestarted m = 24 process recovers
TABLE = {"duct633": (-5 + 6j, [-5.35278 + 6.06606j, -5.94101 + 5.83224j, -6.34740 + 4.67745j]),
         "duct833": (-2 + 8j, [-3.05789 + 6.85097j, -3.01694 + 6.69459j])}


@functools.lru_cache(maxsize=None)
def dense_spectrum(name):
    c = SO.case(name)
    return SO.dense_spectrum(*c.operators(), c.constrained)


@functools.lru_cache(maxsize=None)
def oracle_run(name, shift, m=24, left=False):
    c = SO.case(name)
    J, B = c.operators()
    V, H, m_done, reason = CO.arnoldi(J, B, c.constrained, shift, m=m, left=left)
    Jm, Bm = (sp.csr_matrix(J.T), sp.csr_matrix(B.T)) if left else (J, B)
    return V, H, m_done, reason, CO.recover(Jm, Bm, V, H, m_done, shift)


# ---- 1. the oracle's own check -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TABLE))
def test_the_oracle_recovers_the_recorded_pairs(name):
    """Exact LU solves, m = 24, no restart: the recorded eigenvalues to their six digits, each within 10 TOL relative of the
    dense QZ spectrum and with a true residual <= TOL (3e-15 .. 2e-10 recorded); the basis orthonormal and the Arnoldi relation
    of the REAL operator Re[(J + s B)^-1 B] to 1e-12 (1e-16 seen)."""
    shift, recorded = TABLE[name]
    c = SO.case(name)
    J, B = c.operators()
    V, H, m_done, reason, (lam, X, res) = oracle_run(name, shift)
    assert (m_done, reason) == (24, 1)
    assert SO.orthogonality(V, 25) <= 1e-12 and CO.relation(J, B, c.constrained, shift, V, H, m_done) <= 1e-12
    assert not V[:, c.constrained].any()
    for want in recorded:
        j = int(np.abs(lam - want).argmin())
        print(name, want, "->", lam[j], "residual", res[j], "dense distance", SO.nearest(dense_spectrum(name), [lam[j]])[0])
        assert abs(lam[j] - want) <= 1e-5
        assert res[j] <= TOL and SO.nearest(dense_spectrum(name), [lam[j]])[0] <= 10.0 * TOL
        assert np.abs(lam - np.conj(want)).min() <= 1e-5                               # ... and the conjugate partner


def test_a_shift_and_its_conjugate_give_the_same_spectrum():
    """Re[(J + conj(s) B)^-1 B] is the same real operator: the same H up to rounding, the same eigenvalues."""
    shift = TABLE["duct633"][0]
    _, H, _, _, (lam, _, res) = oracle_run("duct633", shift)
    _, Hc, _, _, (lamc, _, resc) = oracle_run("duct633", np.conj(shift))
    assert np.abs(H - Hc).max() <= 1e-12 * np.abs(H).max()
    ok, okc = res <= TOL, resc <= TOL
    assert ok.sum() >= 6 and ok.sum() == okc.sum()
    assert SO.nearest(lamc[okc], lam[ok]).max() <= 10.0 * TOL and SO.nearest(lam[ok], lamc[okc]).max() <= 10.0 * TOL


def test_the_left_process_has_the_same_eigenvalues():
    shift, recorded = TABLE["duct633"]
    _, _, m_done, reason, (lam, _, res) = oracle_run("duct633", shift, left=True)
    assert (m_done, reason) == (24, 1)
    for want in recorded[:2]:
        j = int(np.abs(lam - want).argmin())
        assert abs(lam[j] - want) <= 1e-5 and res[j] <= TOL


# ---- 2. the recovery formula and the root selection on a synthetic pencil ----------------------------------------------------------
def test_shifted_roots_invert_the_ritz_value_map():
    rng = np.random.default_rng(5)
    for s in (-5 + 6j, 2 + 17j, 0.3 - 4j, complex(-3.0, 0.0), complex(1.5, 0.0), 1e-3j):
        lam = rng.standard_normal(50) * 5 + 1j * rng.standard_normal(50) * 5
        theta = (s.real - lam) / ((s - lam) * (np.conj(s) - lam))
        l1, l2 = S.shifted_roots(theta, s)
        err = np.minimum(np.abs(l1 - lam), np.abs(l2 - lam)) / np.abs(lam)
        assert err.max() <= 1e-9, (s, err.max())
        if s.imag == 0.0:                                                             # a real shift: a - 1 / theta, and the shift itself
            assert np.abs(l1 - (s.real - 1.0 / theta)).max() <= 1e-12 * np.abs(l1).max() and np.abs(l2 - s.real).max() == 0.0


@pytest.mark.parametrize("shift", [-1.5 + 2j, 0.5 + 3j, complex(-2.0, 0.0)])
def test_recovery_and_root_selection_on_a_synthetic_pencil(shift):
    """A random real pencil J x = -lam B x of order 40 with a singular B (10 zero columns: infinite eigenvalues, as the flow's
    pressure columns give): with V = I and H = S = Re[(J + s B)^-1 B] every eigenpair of S is a Ritz pair, and the package's
    ``shifted_eigenpairs`` must return every finite eigenvalue of scipy.linalg.eig(J, -B) -- the right root each time -- with a
    true residual at rounding level; the wrong root is not in the spectrum."""
    rng = np.random.default_rng(21)
    n = 40
    J = rng.standard_normal((n, n)) + 4.0 * np.eye(n)
    B = rng.standard_normal((n, n)) * 0.2 + np.eye(n)
    B[:, 30:] = 0.0
    alpha, beta = sla.eig(J, -B, right=False, homogeneous_eigvals=True)
    finite = np.abs(beta) > 1e-9 * np.abs(alpha)
    want = alpha[finite] / beta[finite]
    assert len(want) == 30
    Sop = np.linalg.solve(J + shift * B, B.astype(complex)).real
    P = CO.StandIn(sp.csr_matrix(J), sp.csr_matrix(B), np.zeros(n, bool))
    P.A = sp.csr_matrix(J + abs(shift) * B)                                           # what a shifted run leaves: J + pc_shift B
    H = np.vstack([Sop, np.zeros((1, n))])
    lam, Y, est, theta = S.shifted_eigenpairs(P, None, torch.eye(n + 1, n, dtype=torch.float64), H, n, shift, abs(shift))
    good = est <= 1e-9
    print(shift, "finite pairs", good.sum(), "worst residual", est[good].max(), "worst distance", SO.nearest(lam[good], want).max())
    assert good.sum() == 30 and not np.isfinite(est[~np.isfinite(lam)]).any()
    assert SO.nearest(lam[good], want).max() <= 1e-9 and SO.nearest(want, lam[good]).max() <= 1e-9
    assert np.all(np.diff(lam[good].real) <= 0.0)                                      # the order of ritz_pairs
    # the rejected roots: their true residual is not small (otherwise the choice would be arbitrary)
    l1, l2 = S.shifted_roots(theta[good], shift)
    other = np.where(np.abs(l1 - lam[good]) <= np.abs(l2 - lam[good]), l2, l1)
    assert SO.nearest(want, other).min() >= 1e-6
    # the oracle's independent recovery (numpy.roots) agrees
    lam_o, _, res_o = CO.recover(sp.csr_matrix(J), sp.csr_matrix(B), np.eye(n + 1, n), H, n, shift)
    assert SO.nearest(lam_o[res_o <= 1e-9], lam[good]).max() <= 1e-9 and (res_o <= 1e-9).sum() == 30


# ---- 3. linear_stability through a stand-in ------------------------------------------------------------------------------------
def test_linear_stability_with_a_complex_shift_through_a_stand_in():
    """m = 24 unrestarted and m = 12 restarted return the three recorded pairs of duct633; left modes pair every one with
    z^T B x = 1; the estimates are true residuals; a float shift never reaches the new methods."""
    shift, recorded = TABLE["duct633"]
    c = SO.case("duct633")
    J, B = c.operators()
    P = CO.StandIn(J, B, c.constrained)
    r = S.linear_stability(P, None, n_modes=8, shift=shift, m=24, tol=TOL, left=True)
    assert P.options.ksp_rtol == 1e-8 and not P.flipped and r.shift == shift
    assert "stability_arnoldi" not in P.calls and P.calls.count("stability_arnoldi_shifted") == 2
    X, Z = r.modes.numpy(), r.left_modes.numpy()
    for want in recorded:
        for target in (want, np.conj(want)):
            j = int(np.abs(r.eigenvalues - target).argmin())
            assert abs(r.eigenvalues[j] - target) <= 1e-5 and r.converged[j] and r.left_converged[j]
            assert abs(r.estimates[j] - SO.mode_residual(J, B, r.eigenvalues[j], X[j])) <= 1e-3 * r.estimates[j] + 1e-14
            assert abs(Z[j] @ (B @ X[j]) - 1.0) <= 1e-10
            assert SO.mode_residual(sp.csr_matrix(J.T), sp.csr_matrix(B.T), r.eigenvalues[j], Z[j]) <= 10.0 * TOL
    assert SO.nearest(dense_spectrum("duct633"), r.eigenvalues[r.converged]).max() <= 10.0 * TOL
    P2 = CO.StandIn(J, B, c.constrained)
    r2 = S.linear_stability(P2, None, n_modes=6, shift=shift, m=12, tol=TOL, max_restarts=40)
    print("restarts", r2.restarts, r2.eigenvalues, r2.estimates)
    assert 1 <= r2.restarts < 40 and r2.converged.all() and r2.m_done == 12
    assert P2.calls.count("stability_arnoldi_shifted") == 1 + r2.restarts and P2.calls.count("basis_rotate") == r2.restarts
    for want in recorded:
        assert np.abs(r2.eigenvalues - want).min() <= 1e-5 and np.abs(r2.eigenvalues - np.conj(want)).min() <= 1e-5
    # a float shift: the old path, the old result
    P3, P4 = CO.StandIn(J, B, c.constrained), CO.StandIn(J, B, c.constrained)
    r3 = S.linear_stability(P3, None, n_modes=4, shift=2.5, m=16, tol=TOL)
    assert P3.calls == ["stability_arnoldi"] and isinstance(r3.shift, float)
    lam, Y, est = S.ritz_pairs(*P4.stability_arnoldi(None, shift=2.5, m=16)[1:2], 16, 2.5)
    assert set(r3.eigenvalues) <= set(lam)
    with pytest.raises(ValueError):
        S.linear_stability(P3, None, shift=2.5, pc_shift=1.0)


def test_a_negative_real_shift_through_a_stand_in():
    """complex(a, 0) with a < 0: the eigenvalues nearest a, which no real shift >= 0 reaches first."""
    c = SO.case("duct633")
    J, B = c.operators()
    a = -6.0
    P = CO.StandIn(J, B, c.constrained)
    r = S.linear_stability(P, None, n_modes=3, shift=complex(a, 0.0), m=16, tol=TOL, max_restarts=40)
    dense = dense_spectrum("duct633")
    target = dense[np.argsort(np.abs(dense - a))][:3]
    print("restarts", r.restarts, r.eigenvalues, r.estimates, "nearest", target)
    assert r.converged.all() and SO.nearest(dense, r.eigenvalues).max() <= 10.0 * TOL
    both = np.concatenate([r.eigenvalues, r.eigenvalues.conj()])
    assert SO.nearest(both, target).max() <= 10.0 * TOL
    # pc_shift: another preconditioned matrix, the same operator -- the stand-in's exact solves give the same eigenvalues
    P2 = CO.StandIn(J, B, c.constrained)
    r2 = S.linear_stability(P2, None, n_modes=3, shift=complex(a, 0.0), m=16, tol=TOL, max_restarts=40, pc_shift=0.0)
    assert abs(P2.A - J).max() == 0.0 and np.abs(r2.eigenvalues - r.eigenvalues).max() <= 10.0 * TOL * np.abs(r.eigenvalues).max()


# ---- 4. the argument rules -------------------------------------------------------------------------------------------------------
def test_shifted_request_rules(tmp_path):
    """check_shifted_args / check_shifted_coefficient behind the stability rows, every combination of the nine facts, both
    sides, against a transcription of the rules written here: the dimension, then m in [2, 64], k in [0, m - 1], finite shift
    parts, a finite pc_shift >= 0, breakdown_rel in (0, 1) (the operator calls: c finite) -- all SNS_E_ARG --, then the state.
    Every refusal occurs in the sweep; no new request kind."""
    TEXT = dict(dim="3-D handles only", m="m must lie in [2, 64]", k="k must lie in [0, m - 1]",
                shift="both parts of the shift must be finite", pc="pc_shift must be finite and >= 0",
                brel="breakdown_rel must lie in (0, 1)", c="both parts of c must be finite",
                part="not with a communicator attached (partitioned stability analysis is not built)",
                vl="not with a viscosity law set (the mass operator of the law's form is not built)",
                tt="not with a time term set (the analysis sets its own and clears it)")
    fin = lambda t: math.isfinite(float(t))

    def expected_process(dim, part, tt, vl, m, k, sre, sim, pc, brel):
        checks = [(dim != 3, E_ARG, TEXT["dim"]), (not 2 <= m <= 64, E_ARG, TEXT["m"]), (not 0 <= k <= m - 1, E_ARG, TEXT["k"]),
                  (not (fin(sre) and fin(sim)), E_ARG, TEXT["shift"]), (not (fin(pc) and float(pc) >= 0.0), E_ARG, TEXT["pc"]),
                  (not 0.0 < float(brel) < 1.0, E_ARG, TEXT["brel"]), (part, E_STATE, TEXT["part"]), (vl, E_STATE, TEXT["vl"]),
                  (tt, E_STATE, TEXT["tt"])]
        return next(((code, tail) for cond, code, tail in checks if cond), (0, ""))

    def expected_operator(dim, part, tt, vl, cre, cim):
        checks = [(dim != 3, E_ARG, TEXT["dim"]), (not (fin(cre) and fin(cim)), E_ARG, TEXT["c"]), (part, E_STATE, TEXT["part"]),
                  (vl, E_STATE, TEXT["vl"])]                                          # (a time term does not concern the operator)
        return next(((code, tail) for cond, code, tail in checks if cond), (0, ""))

    exe = RG.policy_main(tmp_path, "shifted_request")
    pargs = [(24, 0, "-5", "6", "7.8", "1e-6"), (2, 1, "0", "0", "0", "0.5"), (64, 63, "-1e300", "1e300", "1e308", "1e-300"),
             (1, 0, "-5", "6", "1", "1e-6"), (65, 0, "-5", "6", "1", "1e-6"), (24, -1, "-5", "6", "1", "1e-6"),
             (24, 24, "-5", "6", "1", "1e-6"), (24, 0, "nan", "6", "1", "1e-6"), (24, 0, "-5", "inf", "1", "1e-6"),
             (24, 0, "-inf", "6", "1", "1e-6"), (24, 0, "-5", "6", "-1e-300", "1e-6"), (24, 0, "-5", "6", "nan", "1e-6"),
             (24, 0, "-5", "6", "inf", "1e-6"), (24, 0, "-5", "6", "1", "0"), (24, 0, "-5", "6", "1", "1"),
             (24, 0, "-5", "6", "1", "nan"), (0, 5, "nan", "nan", "-1", "2"), (24, 30, "nan", "6", "-1", "2"),
             (24, 3, "nan", "6", "-1", "2"), (24, 3, "5", "6", "-1", "2")]
    oargs = [("0", "0"), ("-12.8", "6"), ("nan", "0"), ("0", "inf"), ("-inf", "nan"), ("1e308", "-1e308")]
    questions = [("P", left, f, a) for left in (0, 1) for f in RG.FACTS for a in pargs]
    questions += [("O", left, f, a) for left in (0, 1) for f in RG.FACTS for a in oargs]
    text = "".join(" ".join(map(str, (kind, left) + tuple(f) + a)) + "\n" for kind, left, f, a in questions)
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.returncode
    lines = run.stdout.split("\n")
    assert list(map(int, lines[0].split())) == [2, 4, 2, 64]                          # no new request kind
    rows = [ln.split("\t") for ln in lines[1:1 + len(questions)]]
    assert len(rows) == len(questions) and lines[1 + len(questions):] == [""]
    got = {"P": set(), "O": set()}
    right = {}
    for (kind, left, f, a), (code, tail) in zip(questions, rows):
        want = (expected_process if kind == "P" else expected_operator)(*f[:RG.VL + 1], *a)
        assert (int(code), tail) == want, (kind, left, f, a, code, tail)
        if left == 0:
            right[(kind, f, a)] = (code, tail)
        else:
            assert right[(kind, f, a)] == (code, tail)                                # both sides alike
        got[kind].add((int(code), tail))
    assert got["P"] == {(0, "")} | {(E_ARG, TEXT[k]) for k in ("dim", "m", "k", "shift", "pc", "brel")} | \
        {(E_STATE, TEXT[k]) for k in ("part", "vl", "tt")}
    assert got["O"] == {(0, ""), (E_ARG, TEXT["dim"]), (E_ARG, TEXT["c"]), (E_STATE, TEXT["part"]), (E_STATE, TEXT["vl"])}
    for text in ("X 0 3 0 0 0 0 0 0 0 0 1 2\n", "P 2 3 0 0 0 0 0 0 0 0 24 0 -5 6 1 1e-6\n", "O 0 3 0 0\n", "P 0 3 0 0 0 0 0 0 0 0 24 0 -5\n"):
        assert subprocess.run([exe], input=text, capture_output=True, text=True).returncode == 2


# ---- 5. the binding --------------------------------------------------------------------------------------------------------------
def test_complex_shift_entry_points_are_bound(built_lib):
    """Symbols, argtypes, header declarations; a null handle is SNS_E_ARG before any GPU call; the ABI version stays 8."""
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    H, P, D, I, PI, PD = C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)
    names = ("sns_shifted_apply", "sns_shifted_solve", "sns_stability_arnoldi_shifted")
    hdr = open(os.path.join(ROOT, "include", "sns.h")).read()
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in names:
        assert name in _lib.SYMBOLS and hasattr(built_lib, name)
        assert ("SNS_API int %s(" % name) in hdr and (" T %s\n" % name) in nm
        assert getattr(built_lib, name).restype == C.c_int
    assert built_lib.sns_shifted_apply.argtypes == [H, P, D, D, I, P, P]
    assert built_lib.sns_shifted_solve.argtypes == [H, P, D, D, I, P, P, PI, PI, PD]
    assert built_lib.sns_stability_arnoldi_shifted.argtypes == [H, P, D, D, D, I, I, D, I, P, P, PI, PI, PI]
    buf = (C.c_double * 16)()
    a = C.addressof(buf)
    k, rn = C.c_int(), C.c_double()
    assert built_lib.sns_shifted_apply(None, a, 0.0, 1.0, 0, a, a) == E_ARG
    assert b"sns_shifted_apply: null" in built_lib.sns_last_error()
    assert built_lib.sns_shifted_solve(None, a, 0.0, 1.0, 0, a, a, C.byref(k), C.byref(k), C.byref(rn)) == E_ARG
    assert b"sns_shifted_solve: null" in built_lib.sns_last_error()
    assert built_lib.sns_stability_arnoldi_shifted(None, a, -5.0, 6.0, 7.8, 0, 4, 1e-6, 0, a, a, C.byref(k), C.byref(k), C.byref(k)) == E_ARG
    assert b"sns_stability_arnoldi_shifted: null" in built_lib.sns_last_error()
    assert built_lib.sns_abi_version() == 8
    for name in ("shifted_apply", "shifted_solve", "stability_arnoldi_shifted"):
        assert callable(getattr(S.FlowProblem, name))
    assert callable(S.shifted_eigenpairs) and callable(S.harmonic_response) and callable(S.shifted_roots)
