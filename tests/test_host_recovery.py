"""CPU checks of the gradient-recovery oracle (tests/recovery_oracle.py): exactness on affine fields, convergence and
effectivity of the Zienkiewicz-Zhu estimate on a smooth field, the closed forms of pure shear with the wall shear stress of
functionals.wall_shear_stress, the binding of the two entry points, and the fixture tests/golden/recovery_cases.npz against
its recipe scripts/make_recovery_golden.py.  The bounds here are conditions on the oracle, not on the GPU code."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

import recovery_oracle as RO
from conftest import GOLDEN, ROOT, rel
from stabilized_navier_stokes_flow_fenicsx_amd import functionals as Fn
from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
from stabilized_navier_stokes_flow_fenicsx_amd import mesh2d as M2

FIXTURE = os.path.join(GOLDEN, "recovery_cases.npz")


def golden_script():
    spec = importlib.util.spec_from_file_location("make_recovery_golden", os.path.join(ROOT, "scripts", "make_recovery_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def affine_state(points, seed):
    """w = A x + b at the nodes, A (4, 3) with zero columns past the mesh dimension."""
    rng = np.random.default_rng(seed)
    d = points.shape[1]
    A = np.zeros((4, 3))
    A[:, :d] = rng.standard_normal((4, d))
    return A, (points @ A[:, :d].T + rng.standard_normal(4)).ravel()


def closed_forms(A):
    """D of u = A x from A's velocity rows."""
    U = A[:3]
    S, Om = 0.5 * (U + U.T), 0.5 * (U - U.T)
    return np.array([U[2, 1] - U[1, 2], U[0, 2] - U[2, 0], U[1, 0] - U[0, 1], 0.5 * ((Om ** 2).sum() - (S ** 2).sum()),
                     math.sqrt(2.0 * (S ** 2).sum()), np.trace(U)])


@pytest.mark.parametrize("dim", [3, 2])
def test_affine_fields_are_recovered_exactly(dim):
    """Every cell gradient of an affine field is A, so every weighted mean is A: at every node, boundary included."""
    if dim == 3:
        m = M.duct_mesh((8, 4, 4), 2.0, jitter=0.2)
        pts, cells = m.points, m.tets
    else:
        pts, cells = golden_script().meshes()["tri"]
    A, w = affine_state(pts, 41)
    G = RO.recover(pts, cells, w)
    assert G.shape == (len(pts), 4, 3)
    assert rel(G, np.broadcast_to(A, G.shape)) < 1e-12
    eta, eta_rel, _ = RO.zz(pts, cells, w)
    assert eta_rel < 1e-12
    D, ref = RO.derived(G), closed_forms(A)
    assert np.abs(D - ref).max() < 1e-12 * np.abs(A).max() ** 2 * 10
    if dim == 2:
        assert not G[:, :, 2].any()


def smooth_u(x):
    return np.stack([np.sin(1.3 * x[:, 0] + 0.4 * x[:, 1]) * np.cos(0.7 * x[:, 2]),
                     np.exp(0.5 * x[:, 0] - 0.3 * x[:, 1] + 0.2 * x[:, 2]),
                     np.cos(x[:, 0]) * np.sin(1.1 * x[:, 1] + 0.6 * x[:, 2])], axis=1)


def smooth_grad(x):
    a, c = 1.3 * x[:, 0] + 0.4 * x[:, 1], 0.7 * x[:, 2]
    e = np.exp(0.5 * x[:, 0] - 0.3 * x[:, 1] + 0.2 * x[:, 2])
    b = 1.1 * x[:, 1] + 0.6 * x[:, 2]
    g = np.zeros((len(x), 3, 3))
    g[:, 0, 0], g[:, 0, 1], g[:, 0, 2] = 1.3 * np.cos(a) * np.cos(c), 0.4 * np.cos(a) * np.cos(c), -0.7 * np.sin(a) * np.sin(c)
    g[:, 1, 0], g[:, 1, 1], g[:, 1, 2] = 0.5 * e, -0.3 * e, 0.2 * e
    g[:, 2, 0], g[:, 2, 1], g[:, 2, 2] = -np.sin(x[:, 0]) * np.sin(b), 1.1 * np.cos(x[:, 0]) * np.cos(b), 0.6 * np.cos(x[:, 0]) * np.cos(b)
    return g


@pytest.mark.parametrize("jitter", [0.0, 0.2])
def test_estimate_converges_and_tracks_the_true_error(jitter):
    """A smooth non-polynomial field interpolated on duct_mesh((2n, n, n), 2.0), n = 4, 8, 16: eta falls by more than 1.7 per
    halving (first order in h: 2 in the limit) and eta over the true |grad u - grad u_h| (4-point rule) lies in [0.8, 1.25]."""
    etas = []
    for n in (4, 8, 16):
        m = M.duct_mesh((2 * n, n, n), 2.0, jitter=jitter)
        w = np.zeros((m.num_nodes, 4))
        w[:, :3] = smooth_u(m.points)
        eta = RO.zz(m.points, m.tets, w.ravel())[0]
        true = RO.true_gradient_error(m.points, m.tets, w.ravel(), smooth_grad)
        print(f"jitter {jitter} n {n}: eta {eta:.6e} true {true:.6e} effectivity {eta / true:.4f}")
        assert 0.8 <= eta / true <= 1.25
        etas.append(eta)
    print("ratios", etas[0] / etas[1], etas[1] / etas[2])
    assert etas[0] / etas[1] > 1.7 and etas[1] / etas[2] > 1.7


def test_pure_shear_and_its_wall_shear_stress():
    """u = (g y, 0, 0): shear rate |g|, omega_z = -g, Q = 0, div u = 0 at every node; on the walls y = +-0.5 of the duct (outward
    normal +-y, so n = -+y into the fluid) the wall shear stress is -+ nu g e_x."""
    g, nu = -0.7, 0.05
    m = M.duct_mesh((8, 4, 4), 2.0, jitter=0.2)
    w = np.zeros((m.num_nodes, 4))
    w[:, 0] = g * m.points[:, 1]
    G = RO.recover(m.points, m.tets, w.ravel())
    D = RO.derived(G)
    ref = np.array([0.0, 0.0, -g, 0.0, abs(g), 0.0])
    assert np.abs(D - ref).max() < 1e-13
    wall = m.meta["tags"]["wall"]
    nodes, tau = Fn.wall_shear_stress(m, G, nu, wall)
    n2, tau2 = RO.wall_shear_stress(m.points, m.tets, m.facets[m.find(wall)], G, nu)
    assert np.array_equal(nodes, n2) and np.abs(tau - tau2).max() < 1e-15
    y, z = m.points[nodes, 1], m.points[nodes, 2]
    flat = np.abs(np.abs(z) - 0.5) > 1e-9                     # not on an edge of the duct, where the nodal normal is a mix
    for side in (1.0, -1.0):
        on = flat & (np.abs(y - 0.5 * side) < 1e-12)
        assert on.sum() > 4
        assert np.abs(tau[on] - np.array([-side * nu * g, 0.0, 0.0])).max() < 1e-14
    on = np.abs(np.abs(y) - 0.5) > 1e-9                       # the walls z = +-0.5: S n = 0
    assert np.abs(tau[on]).max() < 1e-14


def test_wall_shear_stress_2d_matches_the_oracle():
    m = M2.rectangle_mesh(6, 5)
    w = np.random.default_rng(43).standard_normal(m.num_dofs)
    G = RO.recover(m.points, m.tris, w)
    tag = M2.CAVITY2D_TAGS["noslip"]
    nodes, tau = M2.wall_shear_stress_2d(m, G, 0.3, tag)
    n2, tau2 = RO.wall_shear_stress(m.points, m.tris, m.facets[m.find(tag)], G, 0.3)
    assert np.array_equal(nodes, n2) and np.abs(tau - tau2).max() < 1e-13 * np.abs(tau2).max()


def test_entry_points_are_bound(built_lib):
    """argtypes of the two entry points; a null handle is SNS_E_ARG before any GPU call (this machine has none)."""
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    H, P = C.c_void_p, C.c_void_p
    assert "sns_recover_gradient" in _lib.SYMBOLS and "sns_error_indicator" in _lib.SYMBOLS
    assert built_lib.sns_recover_gradient.argtypes == [H, P, P, P] and built_lib.sns_recover_gradient.restype == C.c_int
    assert built_lib.sns_error_indicator.argtypes == [H, P, P, P, P] and built_lib.sns_error_indicator.restype == C.c_int
    buf = (C.c_double * 16)()
    a = C.addressof(buf)
    assert built_lib.sns_recover_gradient(None, a, a, a) == -1
    assert built_lib.sns_error_indicator(None, a, None, a, None) == -1


def test_fixture_regenerates_from_the_script():
    g = np.load(FIXTURE)
    assert os.path.getsize(FIXTURE) < 200_000
    fresh = golden_script().build()
    assert sorted(g.files) == sorted(fresh)
    for k in g.files:
        a, b = g[k], np.asarray(fresh[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if k.endswith(("_G", "_D", "_eta2")):            # sums: reproducible up to the library's reduction order
            assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max(), k
        else:
            assert np.array_equal(a, b), k
