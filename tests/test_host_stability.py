"""CPU checks behind the linear stability analysis (sns_mass_apply, sns_stability_arnoldi, solver.ritz_pairs): the request
rules of csrc/sns_policy.h through their stand-alone main against a transcription written here, the oracle
tests/stability_oracle.py against itself -- the sigma-affinity of the Jacobian that justifies B = J(1) - J(0), its Arnoldi
process against the dense spectrum through solver.ritz_pairs, the breakdown of the 9-dof duct -- and the binding of the two
entry points.  The bounds here are conditions on the oracle and on pure-numpy code, not on the GPU code."""
import ctypes as C
import itertools
import math
import os

import numpy as np
import pytest

import request_gate as RG
import stability_oracle as SO
from conftest import ROOT
from stabilized_navier_stokes_flow_fenicsx_amd import solver as S

E_ARG, E_STATE = -1, -3


def test_stability_request_rules(tmp_path):
    """check_stability_request for both requests, every combination of the facts and a sweep of the arguments, against a
    transcription of the issue's rules written here and not derived from the header: argument errors first (dimension, m,
    shift, breakdown_rel), then the state (communicator, law, time term; the mass pass ignores a time term and the arguments)."""
    MASS, ARNOLDI = 0, 1

    def expected(req, dim, part, tt, vl, m, shift, brel):
        shift, brel = float(shift), float(brel)
        checks = [(dim != 3, E_ARG, "3-D handles only")]
        if req == ARNOLDI:
            checks += [(not 2 <= m <= 64, E_ARG, "m must lie in [2, 64]"),
                       (not (shift >= 0.0 and math.isfinite(shift)), E_ARG, "the shift must be finite and >= 0"),
                       (not 0.0 < brel < 1.0, E_ARG, "breakdown_rel must lie in (0, 1)")]
        checks += [(part, E_STATE, "not with a communicator attached (partitioned stability analysis is not built)"),
                   (vl, E_STATE, "not with a viscosity law set (the mass operator of the law's form is not built)")]
        if req == ARNOLDI:
            checks.append((tt, E_STATE, "not with a time term set (the analysis sets its own and clears it)"))
        return next(((code, tail) for cond, code, tail in checks if cond), (0, ""))

    facts = list(itertools.product((MASS, ARNOLDI), (2, 3), (0, 1), (0, 1), (0, 1)))
    args = [(64, "0", "1e-6"), (2, "2.5", "0.5"), (1, "0", "1e-6"), (65, "0", "1e-6"), (0, "0", "1e-6"), (-3, "0", "1e-6"),
            (32, "-1e-300", "1e-6"), (32, "-2", "1e-6"), (32, "nan", "1e-6"), (32, "inf", "1e-6"), (32, "1e308", "1e-6"),
            (32, "0", "0"), (32, "0", "1"), (32, "0", "-0.1"), (32, "0", "nan"), (32, "0", "1.5"), (32, "0", "1e-300"),
            (65, "nan", "2"), (1, "-1", "0")]
    assert set(facts) == {(req,) + f[:RG.VL + 1] for req in (MASS, ARNOLDI) for f in RG.FACTS}
    combos = [(req, f, a) for req in (MASS, ARNOLDI) for f in RG.FACTS for a in args]      # all nine facts of the handle
    assert len(combos) == 2 * 2 * 2 ** 8 * 19
    header, rows = RG.ask(tmp_path, "s", combos)
    assert [header[k] for k in ("SREQ_COUNT", "STABILITY_M_MIN", "STABILITY_M_MAX")] == [2, 2, 64]   # SREQ_COUNT, the bounds of m
    got = [(int(code), tail) for code, tail in rows]
    for (req, f, a), g in zip(combos, got):
        assert g == expected(req, *f[:RG.VL + 1], *a), (req, f, a, g)
    # every verdict of the rules occurs in the sweep
    assert {g for g in got} >= {(0, ""), (E_ARG, "3-D handles only"), (E_ARG, "m must lie in [2, 64]"),
                                (E_STATE, "not with a time term set (the analysis sets its own and clears it)")}


def test_form_request_table_is_untouched():
    """The stability rules live beside policy::FormRequest, not in it."""
    hdr = open(os.path.join(ROOT, "stabilized_navier_stokes_flow_fenicsx_amd", "csrc", "sns_policy.h")).read()
    enum = hdr[hdr.index("enum FormRequest {"):]
    enum = enum[:enum.index("};")]
    assert "STAB" not in enum.upper() and "ARNOLDI" not in enum.upper() and "MASS" not in enum.upper()


@pytest.mark.parametrize("form", [dict(), dict(corrected_convection=True)])
def test_the_jacobian_is_affine_in_sigma_where_u_t_vanishes(form):
    """J(sigma) with d = -sigma u: (J(2) - J(0)) = 2 (J(1) - J(0)) to round-off, which makes B = J(1) - J(0) the mass operator
    of every shift; B has no pressure columns, and zero rows and columns on the constrained dofs."""
    c = SO.case("duct633")
    J0, J1, J2 = (c.jacobian(s, **form) for s in (0.0, 1.0, 2.0))
    dev = abs((J2 - J0) - 2.0 * (J1 - J0)).max()
    print("sigma-affinity", form, dev)
    assert dev < 1e-14
    B = (J1 - J0).toarray()
    assert not B[:, 3::4].any()
    assert not B[c.constrained].any() and not B[:, c.constrained].any()
    assert np.abs(B).max() > 1e-3


@pytest.mark.parametrize("name,shift,n_conv", [("duct633", 0.0, 33), ("duct633", 2.0, 29), ("duct833", 0.0, 30), ("duct833", 2.0, 24)])
def test_ritz_pairs_of_the_oracle_arnoldi_match_the_dense_spectrum(name, shift, n_conv):
    """m = 64 exact-solve Arnoldi: orthogonality and the Arnoldi relation at round-off, the count of pairs with estimate <= 1e-7
    the issue records, every such pair a dense eigenvalue to 1e-6 relative (the estimate bounds the residual, not the error),
    the six dense eigenvalues nearest the shift matched to 1e-8, the order of solver.ritz_pairs."""
    c = SO.case(name)
    J, B = c.operators()
    V, H, m_done, ratios = SO.arnoldi(J, B, c.constrained, shift=shift)
    assert m_done == 64 and ratios.min() >= 0.02
    assert SO.orthogonality(V, 65) < 5e-15
    assert SO.arnoldi_relation(J, B, c.constrained, shift, V, H, 64) < 1e-13
    assert not H[np.tril_indices(65, -2, 64)].any()
    lam, Y, est = S.ritz_pairs(H, m_done, shift)
    assert lam.shape == (64,) and Y.shape == (64, 64) and est.shape == (64,)
    assert np.allclose(np.linalg.norm(Y, axis=0), 1.0)
    assert (np.diff(lam.real) <= 0.0).all()                     # descending real part
    theta = 1.0 / (shift - lam)
    assert np.abs(H[:64, :64] @ Y - Y * theta).max() < 1e-9 * np.abs(theta).max()
    conv = est <= 1e-7
    print(name, shift, "converged", conv.sum(), "leading", lam[conv][:4])
    assert conv.sum() == n_conv
    dense = SO.dense_spectrum(J, B, c.constrained)
    assert SO.nearest(dense, lam[conv]).max() < 1e-6
    six = dense[np.argsort(np.abs(dense - shift))][:6]
    assert SO.nearest(lam[conv], six).max() < 1e-8
    assert lam[conv].real.max() < 0.0                           # these ducts are stable


def test_ritz_pairs_edge_cases():
    """No step done: empty arrays.  A conjugate pair comes out with the positive imaginary part first; a zero Ritz value (an
    infinite eigenvalue) sorts last with an infinite estimate; the estimate is |h_{m+1,m} y_m| / |theta|."""
    lam, Y, est = S.ritz_pairs(np.zeros((3, 2)), 0)
    assert len(lam) == 0 and len(est) == 0
    H = np.zeros((4, 3))
    H[:3, :3] = [[1.0, -2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 0.0]]
    H[2, 1] = 0.0
    H[3, 2] = 0.5
    lam, Y, est = S.ritz_pairs(H, 3, shift=1.0)
    theta = np.array([1.0 + 2.0j, 1.0 - 2.0j])
    ref = 1.0 - 1.0 / theta
    assert np.allclose(lam[:2], ref[np.argsort(-ref.imag)]) and lam[0].imag > 0.0 > lam[1].imag
    assert np.isinf(lam[2].real) and lam[2].real < 0.0 and np.isinf(est[2])
    assert np.allclose(est[:2], 0.0)                            # their vectors have no last component
    lam, Y, est = S.ritz_pairs(H[:3, :2], 2, shift=0.0)        # the leading 2 x 2 block, subdiagonal entry H[2, 1] = 0
    assert np.allclose(est, 0.0)
    H[2, 1] = 0.25
    lam, Y, est = S.ritz_pairs(H, 2, shift=0.0)
    th, y = np.linalg.eig(H[:2, :2])
    assert np.allclose(np.sort(est), np.sort(0.25 * np.abs(y[1] / np.linalg.norm(y, axis=0)) / np.abs(th)))


def test_the_small_duct_breaks_down_at_step_nine():
    """9 free velocity dofs: B has rank <= 9, the Krylov space of S is exhausted by 9 vectors."""
    c = SO.case("duct322")
    assert len(c.mesh.points) == 36
    free_u = (~c.constrained).reshape(-1, 4)[:, :3].sum()
    assert free_u == 9
    J, B = c.operators()
    V, H, m_done, ratios = SO.arnoldi(J, B, c.constrained)
    print("ratios", ratios)
    assert m_done == 9 and ratios[-1] < 1e-8 and ratios[:-1].min() >= 0.04
    assert not H[9:].any() and not H[:, 9:].any() and not V[9:].any()


def test_entry_points_are_bound(built_lib):
    """Symbols, argtypes, header declarations; a null handle is SNS_E_ARG before any GPU call (this machine has none)."""
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    H, P, D, I = C.c_void_p, C.c_void_p, C.c_double, C.POINTER(C.c_int)
    hdr = open(os.path.join(ROOT, "include", "sns.h")).read()
    mk = open(os.path.join(ROOT, "stabilized_navier_stokes_flow_fenicsx_amd", "csrc", "Makefile")).read()
    for name in ("sns_mass_apply", "sns_stability_arnoldi"):
        assert name in _lib.SYMBOLS and hasattr(built_lib, name)
        assert ("SNS_API int %s(" % name) in hdr
    assert mk.count("sns_stability.o") >= 2
    assert built_lib.sns_mass_apply.argtypes == [H, P, P, P] and built_lib.sns_mass_apply.restype == C.c_int
    assert built_lib.sns_stability_arnoldi.argtypes == [H, P, D, C.c_int, D, P, P, I, I, I]
    assert built_lib.sns_stability_arnoldi.restype == C.c_int
    buf = (C.c_double * 16)()
    a = C.addressof(buf)
    k = C.c_int()
    assert built_lib.sns_mass_apply(None, a, a, a) == E_ARG
    assert built_lib.sns_stability_arnoldi(None, a, 0.0, 4, 1e-6, a, a, C.byref(k), C.byref(k), C.byref(k)) == E_ARG
    assert b"null" in built_lib.sns_last_error()
