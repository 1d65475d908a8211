"""CPU checks of the scalar-transport oracle (tests/scalar_oracle.py) and of the binding of the two entry points: the fixture
tests/golden/scalar_cases.npz against its recipe scripts/make_scalar_golden.py, constants in the kernel of the steady operator,
the pure-diffusion limit against the Laplace stiffness of oracle/, and the Galerkin part against a degree-6 quadrature.  The
bounds here are conditions on the oracle, not on the GPU code."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np

import scalar_oracle as SO
from conftest import GOLDEN, ROOT, rel
from oracle import element as el

FIXTURE = os.path.join(GOLDEN, "scalar_cases.npz")


def golden_script():
    spec = importlib.util.spec_from_file_location("make_scalar_golden", os.path.join(ROOT, "scripts", "make_scalar_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = golden_script()


def test_oracle_reproduces_the_fixture():
    g = np.load(FIXTURE)
    assert os.path.getsize(FIXTURE) < 300_000
    fresh = G.build()
    assert sorted(g.files) == sorted(fresh)
    for k in g.files:
        a, b = g[k], np.asarray(fresh[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if k in ("el_A", "el_S", "box_A", "box_b", "box_c"):             # computed: up to the library's reduction order
            assert rel(b, a) < 1e-13, k
        else:
            assert np.array_equal(a, b), k
    # the records cover both orientations and the steady and the reactive form
    X = g["el_X"]
    det = np.linalg.det(np.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 3] - X[:, 0]], axis=2))
    assert (det > 0).any() and (det < 0).any()
    assert (g["el_sigma"] == 0).any() and (g["el_sigma"] > 0).any() and (g["el_theta"] > 0).any()


def test_global_case_solves_its_own_system():
    g = np.load(FIXTURE)
    A, b, c = g["box_A"], g["box_b"], g["box_c"].ravel()
    assert rel(A @ c, b) < 1e-12
    B = g["box_cmask"].ravel().astype(bool)
    assert np.array_equal(c[B], g["box_cval"].ravel()[B])
    # the four species do not couple
    idx = np.arange(len(b)) % 4
    assert np.all(A[idx[:, None] != idx[None, :]] == 0.0)


def test_constants_lie_in_the_kernel_of_the_steady_operator():
    c = G.box_case()
    A0, _ = SO.raw(c["points"], c["tets"], c["w"], c["kappa"], 0.0, 3.0)
    one = np.ones(A0.shape[0])
    assert np.all(np.abs(A0 @ one) <= 1e-13 * (abs(A0) @ one))
    A1, _ = SO.raw(c["points"], c["tets"], c["w"], c["kappa"], 0.5, 3.0)      # ... and not with a reaction term
    assert np.abs(A1 @ one).max() > 1e-3


def test_pure_diffusion_is_the_laplace_stiffness():
    rng = np.random.default_rng(73)
    X = G.random_tets(rng, 6)
    lap = el.stokes_element(X)[:, :, 0, :, 0]                            # (grad u_x, grad v_x) of the Stokes form
    for kappa in (1.0, 3e-3):
        A, _ = SO.element(X, np.zeros((6, 4, 3)), kappa)
        assert rel(A, kappa * lap) < 1e-13


def test_galerkin_part_against_a_degree_6_rule():
    rng = np.random.default_rng(74)
    X = G.random_tets(rng, 6)
    U, src = rng.standard_normal((6, 4, 3)), rng.standard_normal((6, 4))
    rule = SO.conical_rule(5)                                            # exact to degree 7
    assert abs(rule[1].sum() - 1.0 / 6.0) < 1e-15
    A2, S2 = SO.element(X, U, 0.05, 1.3, 0.0, src, stabilised=False)
    A6, S6 = SO.element(X, U, 0.05, 1.3, 0.0, src, rule=rule, stabilised=False)
    assert rel(A2, A6) < 1e-13 and rel(S2, S6) < 1e-13                   # (degree 2: the 4-point rule is exact)
    As, _ = SO.element(X, U, 0.05, 1.3, 0.0, src)
    assert rel(As, A2) > 1e-3                                            # the stabilisation is not nothing


def test_entry_points_are_declared_bound_and_exported(built_lib):
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    names = ("sns_scalar_system", "sns_scalar_solve")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sns.h")).read(), flags=re.S)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in names:
        assert name in _lib.SYMBOLS
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s$" % name, nm, flags=re.M), name
    H, P, D = C.c_void_p, C.c_void_p, C.c_double
    K, I = C.POINTER(C.c_double), C.POINTER(C.c_int)
    assert built_lib.sns_scalar_system.argtypes == [H, P, K, D, D, P, P, P, P] and built_lib.sns_scalar_system.restype == C.c_int
    assert built_lib.sns_scalar_solve.argtypes == [H, P, K, D, D, P, P, P, P, I, I, K] and built_lib.sns_scalar_solve.restype == C.c_int
    assert _lib.ABI_VERSION == 8 and built_lib.sns_abi_version() == 8    # sns_options did not change


def test_a_null_handle_is_refused_before_any_device_call(built_lib):
    buf = (C.c_double * 16)()
    a = C.addressof(buf)
    kap = (C.c_double * 4)(1.0, 1.0, 1.0, 1.0)
    its, reason, rn = C.c_int(), C.c_int(), C.c_double()
    assert built_lib.sns_scalar_system(None, a, kap, 0.0, 0.0, None, a, a, a) == -1
    assert built_lib.sns_scalar_solve(None, a, kap, 0.0, 0.0, None, a, a, a, C.byref(its), C.byref(reason), C.byref(rn)) == -1
    assert b"sns_scalar_solve" in built_lib.sns_last_error()


def test_inner_stream_inlet_data_of_the_driver_switch():
    """SNS_SCALAR_PECLET's Dirichlet data: the inner inlet region's nodes carry 1, the other inlet nodes 0, nothing else is
    constrained; a mesh with one inlet tag takes the centred square of inner_half_width."""
    from stabilized_navier_stokes_flow_fenicsx_amd import drivers as D
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
    mc = M.channel_mesh((4, 8, 8))
    mask, val = D.inner_stream_inlet_data(mc)
    t = mc.meta["tags"]
    inner, outer = mc.facet_nodes(t["inlet_1"]), mc.facet_nodes(t["inlet_2"])
    assert mask.shape == val.shape == (mc.num_nodes, 1) and len(inner) > 0
    assert np.array_equal(np.nonzero(mask[:, 0])[0], np.union1d(inner, outer))
    assert np.all(val[inner, 0] == 1.0) and np.all(val[np.setdiff1d(outer, inner), 0] == 0.0) and val.sum() == len(inner)
    md = M.duct_mesh((2, 8, 8), 1.0)
    mask, val = D.inner_stream_inlet_data(md)
    inlet = md.facet_nodes(md.meta["tags"]["inlet"])
    assert np.array_equal(np.nonzero(mask[:, 0])[0], inlet)
    on = np.all(np.abs(md.points[inlet, 1:]) <= 0.25 + 1e-12, axis=1)
    assert on.sum() == 25 and np.array_equal(val[inlet, 0], on.astype(float))
