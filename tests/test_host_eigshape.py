"""CPU checks behind the eigenvalue shape pass (sns_jacobian_shape_gradient) and solver.eigenvalue_shape_sensitivity: they pin
the formulas before any GPU run.  The oracle is tests/eigshape_oracle.py -- autograd in the vertex coordinates through the
element residual of tests/ns3d_oracle.py.  The per-cell text the kernel runs (csrc/sns_eigshape_cell.h) is compiled on the
host, once plain and once with the address and undefined-behaviour sanitizers, and compared with the oracle cell by cell on
the jittered (4,3,3) duct; the formula d lam / dX is compared with dense spectra of states re-converged on moved meshes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import eigshape_oracle as EO
import hessian_oracle as HO
import stability_oracle as SO
from conftest import ROOT
from oracle import forms_literal as FL
from test_host_hessian import variant_form

E_ARG = -1
CASES = ["duct322", "duct633"]
VARIANTS = ["plain", "corrected", "form_variant", "viscosity_field"]
COEFFS = ((1.0, 0.0), (0.0, 1.0), (1.0, 0.7))
CSRC = os.path.join(ROOT, "stabilized_navier_stokes_flow_fenicsx_amd", "csrc")


def _random(c, seed, k):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(len(c.w)) for _ in range(k)]


# ---- a. the text the kernel runs, on the host ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def cell_exe(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("eigshape") / ("eigshape_cell_" + request.param))
    flags = ["-O1"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    build = subprocess.run(["g++", "-std=c++17", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "eigshape_cell_main.cpp"), "-o", exe],
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
    head = f"{int(corrected)} {int(nu_t is not None)} {V['ci']!r} {V['lsic']!r} {V['pspg']!r} {qa!r} {qb!r} {cj!r} {cb!r} {E}\n"
    run = subprocess.run([exe], input=head + "\n".join(" ".join(repr(float(v)) for v in row) for row in data) + "\n",
                         capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    return np.array(run.stdout.split(), dtype=np.float64).reshape(E, 4, 3)


def _dead_cells(c, x, z, cj):
    """Cells whose contraction vanishes identically: no free entry of x~ or of z~ on the cell, and, for the mass part alone,
    no free velocity entry of x~ (B has no pressure columns) -- on a duct, the cells whose four nodes all sit on the walls."""
    tets = c.mesh.tets
    xe, ze = HO.masked(c, x).reshape(-1, 4)[tets], HO.masked(c, z).reshape(-1, 4)[tets]
    dead = ~xe.reshape(len(tets), -1).any(axis=1) | ~ze.reshape(len(tets), -1).any(axis=1)
    if cj == 0.0:
        dead |= ~xe[:, :, :3].reshape(len(tets), -1).any(axis=1)
    return dead


@pytest.mark.parametrize("variant", VARIANTS)
def test_cell_text_against_the_oracle(cell_exe, variant):
    """eigshape_cell (csrc/sns_eigshape_cell.h), the hand derivative k_eigshape_tet runs per lane, against autograd in X on the
    216 tets of the jittered (4,3,3) duct with random w, x, z: 1e-12 of the cell's largest entry (the oracle's own rounding
    floor is 1.2e-14 at cell level; measured here 2e-15 to 6e-15).  A cell on which the contraction vanishes identically
    (every velocity node constrained) gives exact zeros, compared by equality.  Doubling both coefficients doubles every bit."""
    c = EO.jittered_case()
    assert len(c.mesh.points) == 80 and len(c.mesh.tets) == 216
    x, z = _random(c, 5, 2)
    with variant_form(c, variant) as form:
        for cj, cb in COEFFS:
            ref = EO.cell_shape_gradients(c, c.w, x, z, cj, cb, **form)
            got = _run_cells(cell_exe, c, x, z, cj, cb, variant == "corrected", form.get("nu_t"))
            dead = _dead_cells(c, x, z, cj)
            assert not got[dead].any() and not ref[dead].any()
            err = np.abs(got - ref)[~dead].max(axis=(1, 2)) / np.abs(ref)[~dead].max(axis=(1, 2))
            print(variant, cj, cb, "worst cell", err.max(), "cells that vanish identically", int(dead.sum()))
            assert err.max() <= 1e-12
            if cj == 0.0:
                assert dead.sum() > 0                                                   # (the equality branch is exercised)
        twice = _run_cells(cell_exe, c, x, z, 2.0, 1.4, variant == "corrected", form.get("nu_t"))
        assert np.array_equal(twice, 2.0 * got)


def test_a_cell_of_constrained_nodes_gives_exact_zeros(cell_exe):
    """Every entry of x~ and z~ masked on every cell (the mask of a mesh whose nodes are all constrained, pressure too): exact
    zeros, not small numbers."""
    c = EO.jittered_case()
    zero = np.zeros(len(c.w))
    for cj, cb in COEFFS:
        assert not _run_cells(cell_exe, c, zero, zero, cj, cb, False, None).any()


# ---- b. the formula against dense spectra on moved meshes ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_formula_against_the_difference_of_dense_spectra(name):
    """d lam / dX . V of mode 0 against [lam(X + eps V) - lam(X - eps V)] / (2 eps), the state re-converged by the oracle's Newton
    (tol 1e-13) on each moved mesh, boundary and Dirichlet nodes moving with their values held.  Measured: duct322 1.29e-6 at
    eps = 1e-3 and 3.2e-7 at 5e-4; duct633 6.9e-7 and 1.7e-7 -- second order.  Neither part of the formula is negligible."""
    c = SO.case(name)
    r1, pred, fd1 = EO.formula_error(name, 1e-3)
    r2, _, fd2 = EO.formula_error(name, 5e-4)
    _, e, p = EO.exact_shape_sensitivity(name)
    V = EO.test_field(c.mesh.points)
    pe, pp = np.sum(e * V), np.sum(p * V)
    print(name, "lambda", HO.exact_pairs(name)[0][0], "formula", pred, "explicit", pe, "path", pp, "difference quotients", fd1, fd2,
          "relative difference", r1, r2)
    assert r1 <= 1e-5
    assert r2 < r1 / 3.0
    assert abs(pe) > 0.1 * abs(pred) and abs(pp) > 0.1 * abs(pred)


# ---- c. the cell scalars and translation invariance --------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", CASES)
def test_cell_scalars_sum_to_the_contraction(name, variant):
    """sum_e phi_e = z~^T (c_J J + c_B B) x~ of the assembled operators to 1e-13, and sum_nodes gX = 0 (a translation of the
    whole mesh changes nothing) to 1e-13 of sum |gX|."""
    c = SO.case(name)
    x, z = _random(c, 6, 2)
    with variant_form(c, variant) as form:
        phi = EO.cell_values(c, c.w, x, z, 1.0, 0.7, **form).sum()
        ref = HO.contraction(c, c.w, x, z, 1.0, 0.7, **form)
        g = EO.shape_contraction_gradient(c, c.w, x, z, 1.0, 0.7, **form)
    inv = np.abs(g.sum(axis=0)).max() / np.abs(g).sum()
    print(name, variant, "sum phi_e", phi, "contraction", ref, "sum gX / sum |gX|", inv)
    assert abs(phi - ref) <= 1e-13 * abs(ref)
    assert inv <= 1e-13


# ---- d. the binding -------------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_bound(built_lib):
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    H, P, D = C.c_void_p, C.c_void_p, C.c_double
    hdr = open(os.path.join(ROOT, "include", "sns.h")).read()
    name = "sns_jacobian_shape_gradient"
    assert name in _lib.SYMBOLS and hasattr(built_lib, name)
    assert ("SNS_API int %s(" % name) in hdr and "#define SNS_ABI_VERSION 8" in hdr
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert " T sns_jacobian_shape_gradient\n" in nm
    fn = built_lib.sns_jacobian_shape_gradient
    assert fn.argtypes == [H, P, P, P, D, D, P] and fn.restype == C.c_int
    buf = (C.c_double * 16)()
    a = C.addressof(buf)
    assert fn(None, a, a, a, 1.0, 0.0, a) == E_ARG
    assert b"sns_jacobian_shape_gradient: null" in built_lib.sns_last_error()


def test_solver_exposes_the_sensitivity():
    from stabilized_navier_stokes_flow_fenicsx_amd import solver as S
    import inspect
    sig = inspect.signature(S.eigenvalue_shape_sensitivity)
    assert list(sig.parameters) == ["problem", "w", "result", "k", "pair", "ksp_rtol", "return_parts"]
    assert sig.parameters["ksp_rtol"].default == 1e-10 and sig.parameters["return_parts"].default is False
    m = inspect.signature(S.FlowProblem.jacobian_shape_gradient)
    assert list(m.parameters) == ["self", "w", "x", "z", "c_jac", "c_mass", "out"]
    assert (m.parameters["c_jac"].default, m.parameters["c_mass"].default) == (1.0, 0.0)
