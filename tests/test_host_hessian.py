"""CPU checks behind the Hessian pass (sns_jacobian_state_gradient) and the two eigenvalue sensitivities built on it
(solver.eigenvalue_base_flow_sensitivity, solver.eigenvalue_forcing_sensitivity): they pin the formulas before any GPU run.
The oracle is tests/hessian_oracle.py -- double backward through the element residual of tests/ns3d_oracle.py.  Cases: the
ducts (3,2,2) and (6,3,3) at Re 50 of tests/stability_oracle.py.  The per-cell text the kernel runs (csrc/sns_hessian_cell.h)
is compiled on the host and compared with the oracle cell by cell; the request rules run through their stand-alone main."""
import ctypes as C
import itertools
import math
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import hessian_oracle as HO
import request_gate as RG
import stability_oracle as SO
from conftest import ROOT
from oracle import forms_literal as FL

E_ARG, E_STATE = -1, -3
CASES = ["duct322", "duct633"]
VARIANTS = ["plain", "corrected", "form_variant", "viscosity_field"]
CSRC = os.path.join(ROOT, "stabilized_navier_stokes_flow_fenicsx_amd", "csrc")


class variant_form:
    """``with variant_form(c, variant) as form``: the oracle's form keywords; FL.VARIANT is perturbed inside and put back."""

    def __init__(self, c, variant):
        self.c, self.variant, self.base = c, variant, dict(FL.VARIANT)

    def __enter__(self):
        if self.variant == "corrected":
            return dict(corrected_convection=True)
        if self.variant == "form_variant":
            FL.VARIANT.update(ci=144.0, lsic=0.5, pspg=-1.0, one_point=True)
        if self.variant == "viscosity_field":
            rng = np.random.default_rng(9)
            return dict(nu_t=(1.0 / self.c.Re) * np.exp(rng.uniform(-1.5, 1.5, len(self.c.mesh.tets))))
        return {}

    def __exit__(self, *exc):
        FL.VARIANT.update(self.base)


def _random(c, seed, k=1):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(len(c.w)) for _ in range(k)]


# ---- 1. the identity behind the mass part ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_mass_is_the_residual_difference_in_the_history(name):
    """B(w) x = R(w; d = x_u) - R(w): the form is linear in a = u_t - f."""
    c = SO.case(name)
    x, = _random(c, 1)
    ref = c.mass() @ HO.masked(c, x)
    got = HO.mass_by_identity(c, c.w, x)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(name, "B x by the identity against (J(1) - J(0)) x:", err)
    assert err <= 1e-14
    # and B^T z by autograd in d is the transpose
    z, = _random(c, 2)
    reft = c.mass().T @ HO.masked(c, z)
    errt = np.abs(HO.mass_transpose(c, c.w, z) - reft).max() / np.abs(reft).max()
    print(name, "B^T z by autograd in d:", errt)
    assert errt <= 1e-14


# ---- 2. the contraction against central differences of the assembled operators -----------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", CASES)
def test_contraction_against_the_central_difference(name, variant):
    """g . delta against [C(w + eps delta) - C(w - eps delta)] / (2 eps), C(w) = z~^T (J(w) + 0.7 B(w)) x~, along a random free
    direction: second-order behaviour.  Measured on duct322: 5e-7 at eps = 1e-3, 1e-8 at 1e-4."""
    c = SO.case(name)
    x, z, delta = _random(c, 3, 3)
    delta = HO.masked(c, delta)
    with variant_form(c, variant) as form:
        g = HO.state_gradient(c, c.w, x, z, 1.0, 0.7, **form)
        rel = {}
        for eps in (1e-3, 1e-4):
            fd = (HO.contraction(c, c.w + eps * delta, x, z, 1.0, 0.7, **form) -
                  HO.contraction(c, c.w - eps * delta, x, z, 1.0, 0.7, **form)) / (2.0 * eps)
            rel[eps] = abs(g @ delta - fd) / abs(fd)
    print(name, variant, "relative difference", rel)
    assert rel[1e-4] < 1e-7
    assert rel[1e-4] * 30.0 <= rel[1e-3]
    assert not g[c.constrained].any()
    assert np.abs(g[3::4]).max() > 1e-3 * np.abs(g).max()                               # pressure rows are not zero


# ---- 3. second derivatives commute ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_the_jacobian_part_is_symmetric_and_the_mass_part_is_not(name):
    """g(x, z) . y = g(y, z) . x for the J part (J = dR/dw: its derivative is the symmetric second derivative of z . R),
    relative to the sum of the terms' magnitudes at 1e-13; B is no derivative in w of anything: no such symmetry."""
    c = SO.case(name)
    x, y, z = (HO.masked(c, v) for v in _random(c, 4, 3))
    a, b = HO.state_gradient(c, c.w, x, z, 1.0, 0.0), HO.state_gradient(c, c.w, y, z, 1.0, 0.0)
    sym = abs(a @ y - b @ x) / (np.abs(a * y).sum() + np.abs(b * x).sum())
    am, bm = HO.state_gradient(c, c.w, x, z, 0.0, 1.0), HO.state_gradient(c, c.w, y, z, 0.0, 1.0)
    asym = abs(am @ y - bm @ x) / (np.abs(am * y).sum() + np.abs(bm * x).sum())
    print(name, "J part", sym, "B part", asym)
    assert sym <= 1e-13
    assert asym > 1e-3


# ---- 4. the forcing sensitivity against dense spectra of re-converged states -------------------------------------------------------
def test_forcing_sensitivity_against_the_difference_of_dense_spectra():
    """duct633, mode 0: grad_f lam . f against [lam(+eps f) - lam(-eps f)] / (2 eps), the state re-converged by the oracle's
    Newton under the force, the eigenvalue nearest lam on each side.  Measured: 4.3e-5 at eps = 1e-2, 4.3e-7 at 1e-3, 3.5e-9 at
    1e-4.  Without E = D_w[B^T z][x] the formula misses by more than half: nobody simplifies it."""
    name = "duct633"
    c = SO.case(name)
    lam, X, Z = HO.exact_pairs(name)
    r2, pred, fd2 = HO.forcing_formula_error(name, 1e-2)
    r3, _, fd3 = HO.forcing_formula_error(name, 1e-3)
    print("lambda", lam[0], "formula", pred, "difference quotients", fd2, fd3, "relative difference", r2, r3)
    assert r3 < 1e-5
    assert r3 * 30.0 <= r2
    without = HO.forcing_sensitivity(c, lam[0], X[:, 0], Z[:, 0], with_e=False) @ HO.seeded_force(c)
    miss = abs(without - fd3) / abs(fd3)
    print("the first term alone", without, "misses by", miss)
    assert miss > 0.5
    g = HO.exact_sensitivities(name)[1]
    assert not g[3::4].any() and not g[c.constrained].any()
    # the central difference of B^T z the library takes for E: O(step^2)
    E = HO.exact_sensitivities(name)[2]
    e5 = np.abs(HO.e_vector_fd(c, X[:, 0], Z[:, 0], 1e-5) - E).max() / np.abs(E).max()
    e3 = np.abs(HO.e_vector_fd(c, X[:, 0], Z[:, 0], 1e-3) - E).max() / np.abs(E).max()
    print("E by central differences: fd_rel 1e-3", e3, "1e-5", e5)
    assert e3 < 1e-4 and e5 < 1e-6


# ---- 5. the pieces -------------------------------------------------------------------------------------------------------------------
def test_the_pieces_of_the_forcing_sensitivity():
    """dw = J^-1 B f against the difference of the two Newton states (central: O(eps^2) = 1e-8 at eps = 1e-4, times the ratio of
    the third to the first derivative, O(10) at Re 50; measured 1e-10), and s . dw against the central difference of
    z^T (J + lam B) x along dw (the bound of check 2)."""
    name = "duct633"
    c = SO.case(name)
    J, B = c.operators()
    f = HO.seeded_force(c)
    dw = spla.splu(sp.csc_matrix(J)).solve(B @ f)
    eps = 1e-4
    fd = (HO.forced_state(name, eps) - HO.forced_state(name, -eps)) / (2.0 * eps)
    err = np.abs(dw - fd).max() / np.abs(fd).max()
    print("dw = J^-1 B f against the Newton states:", err)
    assert err < 1e-7
    assert not dw[c.constrained].any()
    lam, X, Z = HO.exact_pairs(name)
    x, z = X[:, 0], Z[:, 0]
    s = HO.s_vector(c, c.w, lam[0], x, z)
    d = dw / np.abs(dw).max()

    def pencil(w):
        return z @ ((c.jacobian(0.0, w) + lam[0] * c.mass(w)) @ x)
    quot = (pencil(c.w + eps * d) - pencil(c.w - eps * d)) / (2.0 * eps)
    rel = abs(s @ d - quot) / abs(quot)
    print("s . dw against the central difference of z^T (J + lam B) x:", rel)
    assert rel < 1e-7


# ---- 6. the request rules --------------------------------------------------------------------------------------------------------------
def test_request_rules(tmp_path):
    """check_state_gradient_request over every combination of the facts and a sweep of the coefficients, against a transcription
    of the rules written here: argument errors first (dimension, finite coefficients), then the state."""
    tails = dict(part="not with a communicator attached (the partitioned Hessian pass is not built)",
                 vl="not with a viscosity law set (the second derivative of nu_e is not built)",
                 tt="not with a time term set (the pass is taken on the steady form)",
                 bf="not with a body force set (J depends on f through the stabilisation's weighting: that contraction is not built)",
                 bk="not with a backflow coefficient set (the Hessian of the backflow term is not built)")

    def expected(dim, part, tt, vl, bf, ev, tr, bk, cj, cb):
        checks = [(dim != 3, E_ARG, "3-D handles only"),
                  (not (math.isfinite(float(cj)) and math.isfinite(float(cb))), E_ARG, "the coefficients must be finite"),
                  (part, E_STATE, tails["part"]), (vl, E_STATE, tails["vl"]), (tt, E_STATE, tails["tt"]), (bf, E_STATE, tails["bf"]),
                  (bk, E_STATE, tails["bk"])]
        return next(((code, tail) for cond, code, tail in checks if cond), (0, ""))

    facts = list(itertools.product((2, 3), *([(0, 1)] * 7)))
    coeffs = [("1", "0"), ("0", "1"), ("1", "0.7"), ("-2.5", "1e300"), ("nan", "0"), ("0", "nan"), ("inf", "1"), ("1", "-inf")]
    def read(f):                                               # the eight facts the transcription takes, in its order
        return f[:RG.EV + 1] + (f[RG.TRACTION], f[RG.BACKFLOW])

    assert set(facts) == {read(f) for f in RG.FACTS}
    combos = [(0, f, a) for f in RG.FACTS for a in coeffs]     # all nine facts of the handle
    assert len(combos) == 2 * 2 ** 8 * 8
    header, rows = RG.ask(tmp_path, "g", combos)
    assert [header[k] for k in ("SREQ_COUNT", "SREQ_KINDS")] == [2, 4]     # StabilityRequest is neither renumbered nor extended
    got = set()
    for (_, f, a), (code, tail) in zip(combos, rows):
        assert (int(code), tail) == expected(*read(f), *a), (f, a, code, tail)
        got.add((int(code), tail))
    assert got == {(0, ""), (E_ARG, "3-D handles only"), (E_ARG, "the coefficients must be finite")} | {(E_STATE, t) for t in tails.values()}
    # allowed: a traction alone, a viscosity field, both
    for ev, tr in ((0, 1), (1, 0), (1, 1)):
        assert expected(3, 0, 0, 0, 0, ev, tr, 0, "1", "0.7") == (0, "")


# ---- 7. the text the kernel runs, on the host ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cell_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hessian") / "hessian_cell")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tests", "hessian_cell_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    return exe


def _run_cells(exe, c, x, z, cj, cb, corrected, nu_t):
    V = FL.VARIANT
    qa, qb = (0.25, 0.25) if V["one_point"] else (0.1381966011250105, 0.5854101966249685)
    tets = c.mesh.tets
    E = len(tets)
    nu = np.full(E, 1.0 / c.Re) if nu_t is None else np.asarray(nu_t)
    data = np.concatenate([c.mesh.points[tets].reshape(E, 12), c.w.reshape(-1, 4)[tets].reshape(E, 16),
                           HO.masked(c, x).reshape(-1, 4)[tets].reshape(E, 16), HO.masked(c, z).reshape(-1, 4)[tets].reshape(E, 16),
                           nu[:, None]], axis=1)
    head = f"{int(corrected)} {V['ci']!r} {V['lsic']!r} {V['pspg']!r} {qa!r} {qb!r} {cj!r} {cb!r} {E}\n"
    run = subprocess.run([exe], input=head + "\n".join(" ".join(repr(float(v)) for v in row) for row in data) + "\n",
                         capture_output=True, text=True)
    assert run.returncode == 0, run.returncode
    return np.array(run.stdout.split(), dtype=np.float64).reshape(E, 16)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", CASES)
def test_cell_text_against_the_oracle(cell_exe, name, variant):
    """state_gradient_cell (csrc/sns_hessian_cell.h), the hand derivative k_state_gradient runs per lane, against double
    backward, cell by cell and after the scatter: 1e-13 of the largest entry (a few hundred products of O(1) factors per
    entry, fp64; measured 3e-15).  Doubling both coefficients doubles every bit."""
    c = SO.case(name)
    x, z = _random(c, 5, 2)
    with variant_form(c, variant) as form:
        for cj, cb in ((1.0, 0.0), (0.0, 1.0), (1.0, 0.7)):
            ref = HO.cell_gradients(c, c.w, x, z, cj, cb, **form)
            got = _run_cells(cell_exe, c, x, z, cj, cb, variant == "corrected", form.get("nu_t"))
            err = np.abs(got - ref).max() / np.abs(ref).max()
            gerr = np.abs(HO._scatter(c, got) - HO._scatter(c, ref)).max() / np.abs(HO._scatter(c, ref)).max()
            print(name, variant, cj, cb, "per cell", err, "scattered", gerr)
            assert err <= 1e-13 and gerr <= 1e-13
        twice = _run_cells(cell_exe, c, x, z, 2.0, 1.4, variant == "corrected", form.get("nu_t"))
        assert np.array_equal(twice, 2.0 * got)


# ---- 8. the binding ----------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_bound(built_lib):
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    H, P, D = C.c_void_p, C.c_void_p, C.c_double
    hdr = open(os.path.join(ROOT, "include", "sns.h")).read()
    name = "sns_jacobian_state_gradient"
    assert name in _lib.SYMBOLS and hasattr(built_lib, name)
    assert ("SNS_API int %s(" % name) in hdr and "#define SNS_ABI_VERSION 8" in hdr
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert " T sns_jacobian_state_gradient\n" in nm
    fn = built_lib.sns_jacobian_state_gradient
    assert fn.argtypes == [H, P, P, P, D, D, P] and fn.restype == C.c_int
    buf = (C.c_double * 16)()
    a = C.addressof(buf)
    assert fn(None, a, a, a, 1.0, 0.0, a) == E_ARG
    assert b"sns_jacobian_state_gradient: null" in built_lib.sns_last_error()
