"""The generalised-Newtonian (Carreau) 3-D NS form on the CPU: the test-side oracle (tests/ns3d_oracle.py) against the
literal Newtonian restatement plus the transpose term of the stress-divergence form, its own autograd Jacobian against
central differences, the law against its closed form in pure shear, the binding of the two new entry points, and the fixture
tests/golden/viscosity_cases.npz against its recipe scripts/make_viscosity_golden.py (the GPU tests reproduce its fields)."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, rel

torch = pytest.importorskip("torch")

import ns3d_oracle as NS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(GOLDEN, "viscosity_cases.npz")


def golden_script():
    spec = importlib.util.spec_from_file_location("make_viscosity_golden", os.path.join(ROOT, "scripts", "make_viscosity_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("corrected", [False, True])
def test_lambda_zero_is_the_literal_form_plus_the_transpose_term(corrected):
    from oracle import forms_literal as FL
    rng = np.random.default_rng(51)
    X = golden_script().random_tets(rng, 6)
    W = rng.normal(size=(6, 16))
    for lam, n in ((0.0, 0.4), (2.5, 1.0)):                                    # either switches the law off: nu_e = nu0
        F, _ = NS.element(X, W, 37.0, law=(lam, n, 0.05), corrected_convection=corrected, want_jac=False)
        T = NS.transpose_term(X, W, 37.0).numpy()
        for e in range(6):
            Fo = FL.ns_residual_literal(X[e], torch.as_tensor(W[e]), 37.0, corrected_convection=corrected).numpy()
            assert rel(F[e], Fo + T[e]) < 1e-13
    assert np.abs(T).max() > 1e-3                                              # (the transpose term is something)


@pytest.mark.parametrize("corrected", [False, True])
def test_autograd_jacobian_against_central_differences(corrected):
    rng = np.random.default_rng(52)
    X = golden_script().random_tets(rng, 4)
    W = rng.normal(size=(4, 16))
    kw = dict(corrected_convection=corrected)
    _, J = NS.element(X, W, 20.0, law=(3.0, 0.5, 0.01), **kw)
    _, J1 = NS.element(X, W, 20.0, law=(3.0, 1.0, 0.01), **kw)
    assert rel(J, J1) > 1e-2                                                   # (the law's derivative is in it)
    h = 1e-6
    for k in range(16):
        dW = np.zeros_like(W)
        dW[:, k] = h
        Fp, _ = NS.element(X, W + dW, 20.0, law=(3.0, 0.5, 0.01), want_jac=False, **kw)
        Fm, _ = NS.element(X, W - dW, 20.0, law=(3.0, 0.5, 0.01), want_jac=False, **kw)
        assert rel(J[:, :, k], (Fp - Fm) / (2 * h)) < 1e-7


def test_pure_shear_gives_the_closed_form():
    """u = (g y, 0, 0): eps has the two entries g / 2, so s = 2 eps:eps = g^2 = gamma_dot^2 on every tet."""
    rng = np.random.default_rng(53)
    X = golden_script().random_tets(rng, 8)
    for g, Re, lam, n, r in ((0.7, 10.0, 3.0, 0.5, 0.01), (-4.0, 150.0, 0.3, 1.5, 0.0), (25.0, 40.0, 10.0, 0.3, 0.05)):
        W = np.zeros((8, 4, 4))
        W[:, :, 0] = g * X[:, :, 1]
        W[:, :, 3] = rng.normal(size=(8, 4))                                   # (the pressure does not enter)
        s = NS.shear_rate2(X, W.reshape(8, 16)).numpy()
        assert rel(s, np.full(8, g * g)) < 1e-12
        want = (1.0 / Re) * (r + (1.0 - r) * (1.0 + lam ** 2 * g * g) ** ((n - 1.0) / 2.0))
        assert rel(NS.carreau(torch.as_tensor(s), 1.0 / Re, lam, n, r).numpy(), np.full(8, want)) < 1e-12
        pts, tets = X.reshape(-1, 3), np.arange(32, dtype=np.int32).reshape(8, 4)
        nu, gd = NS.element_viscosity(pts, tets, W.reshape(-1), Re, lam, n, r)
        assert rel(nu, np.full(8, want)) < 1e-12 and rel(gd, np.full(8, abs(g))) < 1e-12


def test_the_new_entry_points_are_bound():
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    lib = _lib.load()
    import ctypes as C
    assert lib.sns_set_viscosity_law.argtypes == [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double]
    assert lib.sns_element_viscosity.argtypes == [C.c_void_p] * 4
    assert lib.sns_set_viscosity_law(None, 1, 1.0, 0.5, 0.0) == -1             # SNS_E_ARG without a handle, no GPU touched


def test_fixture_regenerates_from_the_script():
    G = golden_script()
    fx = np.load(FIXTURE)
    a, b = G.build(), G.build()
    assert set(a) == set(fx.files)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k          # bit-stable from run to run
        tol = 0.0 if k.startswith("el_") and k != "el_F" else 1e-9             # inputs: the seeded draws themselves
        assert rel(np.asarray(a[k], dtype=np.float64), np.asarray(fx[k], dtype=np.float64)) <= tol, k
    D = G.DUCT
    assert tuple(fx["cells"]) == D["cells"] and float(fx["n"]) == D["n"] and float(fx["n_low"]) == D["n_low"]
    assert float(fx["ratio_law"]) < float(fx["ratio_newton"])                  # shear thinning blunts the profile
