"""The boundary terms on the CPU: two known answers that pin sign, orientation and the facet mass matrix independently of any
restatement (a hydrostatic state, a Robin wall), the backflow Jacobian of the oracle (tests/boundary_oracle.py) against central
differences, the host lists of the boundary pass (sns_host_facet_lists) against a numpy restatement, the table of what a handle
allows (csrc/sns_policy.h: check_boundary_request) against a transcription, and the fixture tests/golden/boundary_cases.npz
against its recipe scripts/make_boundary_golden.py (the GPU tests run its cases through the library)."""
import ctypes
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN

torch = pytest.importorskip("torch")

import boundary_oracle as BO  # noqa: E402
import ns3d_oracle as NS  # noqa: E402
import request_gate as RG  # noqa: E402
import scalar_oracle as SO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(GOLDEN, "boundary_cases.npz")


def golden_script():
    spec = importlib.util.spec_from_file_location("make_boundary_golden", os.path.join(ROOT, "scripts", "make_boundary_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def duct():
    from stabilized_navier_stokes_flow_fenicsx_amd import functionals as FN
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
    m = M.duct_mesh((4, 3, 3), 2.0, jitter=0.2)
    return m, FN.facet_parent_tets(m, np.arange(len(m.facets)))


def hydrostatic_problem():
    """u = 0, p = b.x + p0 with the body force b and the traction t = -p n on every boundary facet: the raw residual vanishes.
    Returns (mesh, owners, state, force, traction (F, 3, 3))."""
    m, par = duct()
    rng = np.random.default_rng(91)
    b, p0 = rng.normal(size=3), rng.normal()
    p = m.points @ b + p0
    w = np.zeros((m.num_nodes, 4))
    w[:, 3] = p
    f = np.zeros((m.num_nodes, 4))
    f[:, :3] = b
    _, n = BO.facet_geometry(m.points, m.tets, m.facets, par)
    t = -p[m.facets.astype(np.int64)][:, :, None] * n[:, None, :]
    return m, par, w.ravel(), f.ravel(), t


def test_hydrostatic_state_has_no_residual():
    m, par, w, f, t = hydrostatic_problem()
    Fv, _ = NS.raw(m.points, m.tets, w, 10.0, f=f, want_jac=False)
    Fb, _ = BO.flow_raw(m.points, m.tets, w, m.facets, par, t, None, want_jac=False)
    print("hydrostatic: volume alone", abs(Fv).max(), "volume + boundary", abs(Fv + Fb).max())
    assert abs(Fv).max() > 0.1                                  # (the volume part alone is far from zero)
    assert abs(Fv + Fb).max() <= 1e-13


def robin_problem():
    """u = 0, c = 1 on the inlet nodes (x = 0), on the outlet (x = L) kappa d_n c = alpha (c_ext - c) + q with four different
    (kappa, alpha, c_ext, q); every other wall natural.  The solution is linear in x: c = 1 - s x, s = (alpha (1 - c_ext) - q) /
    (alpha L + kappa).  Returns (mesh, owners, outlet facet ids, kappa, alpha, c_ext, q, cmask, cval, exact (n, 4))."""
    m, par = duct()
    tags = m.meta["tags"]
    out = m.find(tags["outlet"])
    L = 2.0
    kappa = np.array([1.0, 0.3, 2.5, 0.05])
    alpha = np.array([2.0, 0.0, 0.7, 5.0])                      # (species 1: a pure flux condition)
    c_ext = np.array([0.25, 0.0, -1.5, 3.0])
    q = np.array([0.0, -0.4, 0.9, 0.3])
    cmask = np.zeros((m.num_nodes, 4), np.uint8)
    cmask[m.facet_nodes(tags["inlet"])] = 1
    cval = np.where(cmask, 1.0, 0.0)
    s = (alpha * (1.0 - c_ext) - q) / (alpha * L + kappa)
    return m, par, out, kappa, alpha, c_ext, q, cmask, cval, 1.0 - m.points[:, :1] * s[None, :]


def test_robin_wall_known_answer():
    m, par, out, kappa, alpha, c_ext, q, cmask, cval, exact = robin_problem()
    nf = len(out)
    a = np.broadcast_to(alpha, (nf, 4))
    g = np.broadcast_to(alpha * c_ext + q, (nf, 3, 4))
    c = BO.scalar_solve(m.points, m.tets, np.zeros(4 * m.num_nodes), kappa, cmask, cval, m.facets[out], par[out], alpha=a, g=g)
    print("robin: max error", abs(c - exact).max())
    assert abs(c - exact).max() <= 1e-12
    # without the facet terms the same data gives c = 1 everywhere
    c0 = SO.solve(m.points, m.tets, np.zeros(4 * m.num_nodes), kappa, cmask, cval)
    assert abs(c0 - 1.0).max() <= 1e-12 and abs(c0 - exact).max() > 0.1


def backflow_state():
    """The duct, its outlet's 18 facets and the random state of the Jacobian tests (nodal values x 0.5)."""
    m, par = duct()
    out = m.find(m.meta["tags"]["outlet"])
    w = 0.5 * np.random.default_rng(92).standard_normal(4 * m.num_nodes)
    return m, par, out, w


def test_backflow_jacobian_against_central_differences():
    m, par, out, w = backflow_state()
    assert len(out) == 18
    facets, own = m.facets[out], par[out]
    area, n = BO.facet_geometry(m.points, m.tets, facets, own)
    U = w.reshape(-1, 4)[:, :3][facets.astype(np.int64)]                                    # (F, 3, 3)
    un = np.einsum("qa,fac,fc->fq", BO.QPTS, U, n)
    mixed = int(np.sum((un.min(axis=1) < 0) & (un.max(axis=1) > 0)))
    all_in, all_out = int(np.sum(un.max(axis=1) < 0)), int(np.sum(un.min(axis=1) > 0))
    print("backflow: min |u.n|", abs(un).min(), "mixed", mixed, "all-in", all_in, "all-out", all_out)
    # the test's own preconditions: no quadrature point near the kink, every kind of facet present
    assert abs(un).min() >= 1e-3
    assert mixed >= 1 and all_in >= 1 and all_out >= 1
    beta = np.linspace(0.5, 2.0, len(out))
    F0, J = BO.flow_raw(m.points, m.tets, w, facets, own, None, beta)
    dofs = np.unique(BO._vel_dofs(facets))
    h = 1e-6                                                    # (h |phi . n| <= 1e-6 << 1e-3: no point changes its branch)
    Jfd = np.zeros((len(w), len(dofs)))
    for k, d in enumerate(dofs):
        e = np.zeros_like(w)
        e[d] = h
        Jfd[:, k] = (BO.flow_raw(m.points, m.tets, w + e, facets, own, None, beta, want_jac=False)[0] -
                     BO.flow_raw(m.points, m.tets, w - e, facets, own, None, beta, want_jac=False)[0]) / (2.0 * h)
    Ja = J[:, dofs].toarray()
    err = abs(Ja - Jfd).max() / abs(Ja).max()
    print("backflow: autograd against central differences", err)
    # the term is quadratic in u on each branch: central differences are exact up to rounding, ~ eps |R| / h = 1e-10 relative
    assert err <= 1e-8
    assert abs(J[:, 3::4]).max() == 0.0 and abs(J[3::4]).max() == 0.0 and abs(F0[3::4]).max() == 0.0    # no pressure rows or columns


def numpy_lists(points, tets, facets, own):
    """The lists of the boundary pass restated: rewound facets, boundary rows, per row its (facet, vertex) entries."""
    f = np.asarray(facets, dtype=np.int64).copy()
    opp = np.asarray(tets, dtype=np.int64)[own].sum(axis=1) - f.sum(axis=1)
    P = points[f]
    cr = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    flip = np.einsum("fi,fi->f", cr, P[:, 0] - points[opp]) < 0
    f[flip] = f[flip][:, [0, 2, 1]]
    rows = np.unique(f)
    lists = [[4 * k + a for k in range(len(f)) for a in range(3) if f[k, a] == i] for i in rows]
    return f, rows, lists


def test_host_facet_lists(built_lib):
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    m, par = duct()
    rng = np.random.default_rng(93)
    ids = rng.permutation(len(m.facets))[:40]
    facets = m.facets[ids].copy()
    for k in range(0, len(facets), 2):                          # any winding, any first vertex
        facets[k] = facets[k][rng.permutation(3)]
    out, rows, row_ptr, row_fv = _lib.host_facet_lists(m.points, m.tets, facets, par[ids])
    # orientation against centroids: the normal of the rewound facet points away from the owner's centroid; the nodes are kept
    P = m.points[out.astype(np.int64)]
    cr = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    cen = m.points[m.tets[par[ids]].astype(np.int64)].mean(axis=1)
    assert np.all(np.einsum("fi,fi->f", cr, P.mean(axis=1) - cen) > 0)
    assert np.array_equal(np.sort(out, axis=1), np.sort(facets, axis=1)) and np.array_equal(out[:, 0], facets[:, 0])
    f_np, rows_np, lists_np = numpy_lists(m.points, m.tets, facets, par[ids])
    assert np.array_equal(out, f_np) and np.array_equal(rows, rows_np)
    assert row_ptr[0] == 0 and row_ptr[-1] == 3 * len(facets) and len(row_ptr) == len(rows) + 1
    for r in range(len(rows)):
        assert list(row_fv[row_ptr[r]:row_ptr[r + 1]]) == lists_np[r]
    # the three refusals: SNS_E_MESH, with nothing written
    good = (m.points, m.tets, facets, par[ids])

    def refused(points, tets, fc, own):
        with pytest.raises(_lib.SnsError) as e:
            _lib.host_facet_lists(points, tets, fc, own)
        assert e.value.code == -4, e.value
        return str(e.value)

    wrong = par[ids].copy()
    wrong[3] = (wrong[3] + 7) % len(m.tets)
    while np.isin(facets[3], m.tets[wrong[3]]).all():
        wrong[3] = (wrong[3] + 1) % len(m.tets)
    assert "not three of the four nodes" in refused(good[0], good[1], facets, wrong)
    twice = np.concatenate([facets, facets[5:6][:, [1, 2, 0]]])
    assert "listed twice" in refused(good[0], good[1], twice, np.concatenate([par[ids], par[ids][5:6]]))
    flat = m.points.copy()
    flat[facets[7, 1]] = 0.5 * (flat[facets[7, 0]] + flat[facets[7, 2]])
    assert "degenerate" in refused(flat, good[1], facets, par[ids])
    lib = _lib.load()                                           # nothing written: the outputs keep their fill
    o = np.full((len(twice), 3), -7, np.int32)
    nb = np.array([-7], np.int32)
    tw = np.ascontiguousarray(twice, dtype=np.int32)
    ow = np.concatenate([par[ids], par[ids][5:6]]).astype(np.int64)
    t32 = np.ascontiguousarray(m.tets, dtype=np.int32)
    rc = lib.sns_host_facet_lists(m.num_nodes, len(t32), t32.ctypes.data, m.points.ctypes.data, len(tw), tw.ctypes.data,
                                  ow.ctypes.data, o.ctypes.data, nb.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                  None, None, None)
    assert rc == -4 and np.all(o == -7) and nb[0] == -7


def test_facet_lists_under_sanitizers(tmp_path):
    """build_facet_lists in a stand-alone program (tests/sanitize_facet_lists_main.cpp) under ASan + UBSan, as test_host.py runs
    the pattern and aggregation code: a mesh's whole boundary with shuffled windings, and the three refusals."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "sanitize_facet_lists")
    csrc = os.path.join(ROOT, "stabilized_navier_stokes_flow_fenicsx_amd", "csrc")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fopenmp", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                            os.path.join(ROOT, "tests", "sanitize_facet_lists_main.cpp"), os.path.join(csrc, "sns_host.cpp"), "-o", exe],
                           capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("toolchain without sanitizer runtimes")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS="4", ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-2000:])
    assert "facet lists ok" in run.stdout and "ERROR" not in run.stdout + run.stderr


def test_new_symbols_are_bound(built_lib):
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    for name in ("sns_set_boundary_facets", "sns_set_boundary_flow", "sns_set_boundary_scalar", "sns_host_facet_lists"):
        assert name in _lib.SYMBOLS and hasattr(built_lib, name)
    assert _lib.ABI_VERSION == built_lib.sns_abi_version() == 8


def test_boundary_request_table(tmp_path):
    """check_boundary_request for every request and all combinations of the handle's facts against a transcription written here
    and not derived from the header.  (The rule the boundary terms added to the shape gradient is checked with its request, in
    tests/test_host.py::test_form_request_table.)"""
    E_ARG, E_STATE = -1, -3
    SET_FACETS, SET_FLOW, SET_SCALAR = range(3)
    COMM = "not with a communicator attached (partitioned boundary terms are not built)"

    def expected(req, dim, part, facets):
        checks = [(dim != 3, E_ARG, "3-D handles only"), (part, E_STATE, COMM)]
        if req != SET_FACETS:
            checks.append((not facets, E_STATE, "set the boundary facets first (sns_set_boundary_facets)"))
        return next(((code, tail) for cond, code, tail in checks if cond), (0, ""))

    bcombos = [(req, f, ()) for req in range(3) for f in RG.FACTS]
    header, rows = RG.ask(tmp_path, "b", bcombos)
    assert header["BREQ_COUNT"] == 3                            # policy::BREQ_COUNT
    got = [(int(code), tail) for code, tail in rows]
    for (req, f, _), g in zip(bcombos, got):
        assert g == expected(req, f[RG.DIM], f[RG.PART], f[RG.FACETS]), (req, f, g)
    assert set(got) == {(0, ""), (E_ARG, "3-D handles only"), (E_STATE, COMM),
                        (E_STATE, "set the boundary facets first (sns_set_boundary_facets)")}


def test_fixture_matches_its_recipe():
    fresh = golden_script().build()
    with np.load(FIXTURE) as z:
        assert sorted(z.files) == sorted(fresh)
        for k in z.files:
            a, b = z[k], np.asarray(fresh[k])
            assert a.shape == b.shape, k
            assert abs(a - b).max() <= 1e-13 * max(1.0, abs(b).max()), k
        # the cases are worth running: mixed signs of u.n over the quadrature points of every tet's faces
        for i in range(len(z["X"])):
            _, n = BO.facet_geometry(z["X"][i], np.arange(4)[None], z["faces"], np.zeros(4, np.int64))
            U = z["W"][i].reshape(4, 4)[:, :3][z["faces"].astype(np.int64)]
            un = np.einsum("qa,fac,fc->fq", BO.QPTS, U, n)
            assert un.min() < 0 < un.max()
    assert os.path.getsize(FIXTURE) <= os.path.getsize(os.path.join(GOLDEN, "fields_cases.npz"))
