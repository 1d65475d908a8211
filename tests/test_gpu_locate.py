"""Device point location and P1 evaluation (sns_locate_points / sns_eval_p1, csrc/sns_locate.hip) against the host rule of
interpolate.locate_points: exact on affine fields, the same tets, values and misses as the host, deterministic, the driver's
warm start and the stream tracer's seeds unchanged, and a 648 k-tet source located in well under two seconds."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 1e-6


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    return _lib.load()


def _meshes():
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M, nozzle_mesh as NM
    img = os.path.join(ROOT, "tests", "golden", "inlet_PlusF_final.png")
    duct = M.duct_mesh((12, 5, 5), 2.0, jitter=0.25)
    dela = M.delaunay_channel_mesh(5, lattice="cubic")
    noz = NM.channel_from_image_bodyfitted(img, 0.5, 0.1)[0]
    return {"duct": (duct, M.duct_mesh((17, 7, 7), 2.0)),
            "delaunay": (dela, M.delaunay_channel_mesh(7, lattice="bcc", seed=3)),
            "nozzle": (noz, NM.channel_from_image_bodyfitted(img, 0.5, 0.07)[0])}


@pytest.fixture(scope="module")
def meshes(lib):
    return _meshes()


def _interior(mesh, m, rng):
    """m random points inside random tets (random convex combinations of their corners)."""
    t = rng.integers(0, mesh.num_tets, m)
    w = rng.dirichlet(np.ones(4), m)
    return np.einsum("na,nad->nd", w, mesh.points[mesh.tets[t]])


def _shared(mesh):
    """Vertices, edge midpoints and face centroids of the mesh: the nodes of its nested refinement (plus the face centroids)."""
    T = mesh.tets
    e = np.unique(np.sort(np.concatenate([T[:, [a, b]] for a in range(4) for b in range(a + 1, 4)]), axis=1), axis=0)
    f = np.unique(np.sort(np.concatenate([T[:, [1, 2, 3]], T[:, [0, 2, 3]], T[:, [0, 1, 3]], T[:, [0, 1, 2]]]), axis=1), axis=0)
    P = mesh.points
    return np.concatenate([P, P[e].mean(axis=1), P[f].mean(axis=1)])


def _outside(mesh, rng, m=400):
    """Points off boundary faces: just outside (0.1 .. 0.9 x padding x h and 2 .. 1000 x padding x h) and beyond the box."""
    T = mesh.tets
    f = np.sort(np.concatenate([T[:, [1, 2, 3]], T[:, [0, 2, 3]], T[:, [0, 1, 3]], T[:, [0, 1, 2]]]), axis=1)
    u, c = np.unique(f, axis=0, return_counts=True)
    bf = u[c == 1][rng.integers(0, int((c == 1).sum()), m)]
    X = mesh.points[bf]
    n = np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0])
    h = np.sqrt(np.linalg.norm(n, axis=1))
    n /= np.linalg.norm(n, axis=1)[:, None]
    cen = mesh.points.mean(axis=0)
    p0 = np.einsum("na,nad->nd", rng.dirichlet(np.ones(3), m), X)
    n *= np.sign(((p0 - cen) * n).sum(axis=1))[:, None]                     # roughly outward
    s = np.concatenate([rng.uniform(0.1, 0.9, m // 2), rng.uniform(2.0, 1000.0, m - m // 2)])
    lo, hi = mesh.points.min(axis=0), mesh.points.max(axis=0)
    far = rng.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), (m, 3))
    far = far[np.any((far < lo) | (far > hi), axis=1)]
    return np.concatenate([p0 + (s * PAD * h)[:, None] * n, far])


def _affine(rng):
    a, B = rng.normal(size=4), rng.normal(size=(4, 3))
    return lambda x: a + x @ B.T


@pytest.mark.parametrize("name", ["duct", "delaunay", "nozzle"])
def test_affine_fields_are_exact(meshes, name):
    from stabilized_navier_stokes_flow_fenicsx_amd import interpolate as IP
    src, fine = meshes[name]
    rng = np.random.default_rng(1)
    f = _affine(rng)
    vals = f(src.points)
    q = _interior(src, 20000, rng)
    # padding 0: with the default padding the rule may take a neighbour that misses the point by up to 1e-6 in barycentric
    # terms (first candidate >= -padding), and the clamped value is then off by that much -- on the host as on the device
    out = IP.eval_points(src, vals, q, DEV, padding=0.0)
    scale = np.abs(f(q)).max()
    err_in = np.abs(out - f(q)).max() / scale
    # nodes of a non-nested finer mesh: exact where the point lies in the mesh (a curved wall or a jittered hull leaves some
    # nodes outside, where the clamped value of the best tet is what both paths give)
    t, lam = IP.locate_points(src, fine.points, 0.0, device=DEV)
    inside = IP._bary(src.points[src.tets[t]], fine.points).min(axis=1) >= -1e-12
    ev = IP.eval_points(src, vals, fine.points, DEV, padding=0.0)
    err_fine = np.abs(ev - f(fine.points))[inside].max() / np.abs(f(fine.points)).max()
    print(f"\n  {name}: {src.num_tets} tets; affine error {err_in:.1e} at {len(q)} interior points, {err_fine:.1e} at "
          f"{inside.sum()} of {len(inside)} finer-mesh nodes inside")
    assert err_in <= 1e-12 and err_fine <= 1e-12
    assert inside.mean() > (0.99 if name == "duct" else 0.9)


@pytest.mark.parametrize("name", ["duct", "delaunay", "nozzle"])
def test_device_matches_the_host_rule(meshes, name):
    from stabilized_navier_stokes_flow_fenicsx_amd import interpolate as IP
    src, fine = meshes[name]
    rng = np.random.default_rng(2)
    q = np.concatenate([_interior(src, 5000, rng), fine.points, _shared(src), _outside(src, rng)])
    vals = rng.normal(size=(src.num_nodes, 4))
    th, lh = IP.locate_points(src, q, PAD)
    td, ld = IP.locate_points(src, q, PAD, device=DEV)
    assert td.dtype == th.dtype and ld.shape == lh.shape
    eh = np.einsum("na,nac->nc", lh, vals[src.tets[th]])
    ed = IP.eval_points(src, vals, q, DEV, PAD)
    diff, tie = _ties(src, q, th, td)
    same = td == th
    err = np.abs(ed - eh)[same].max() / np.abs(vals).max()
    # misses: the host's are the points whose bucket has no candidate; the device reports its count
    n_miss = locate_n_missed(IP._DeviceMesh(src, DEV), q)
    print(f"\n  {name}: {len(q)} points, value error {err:.1e}, {len(diff)} different tets ({tie.sum()} ties), "
          f"{n_miss} missed")
    assert err <= 1e-12
    assert tie.all(), diff[~tie][:5]
    assert len(diff) <= 2e-3 * len(q)
    assert n_miss == _host_misses(src, q).sum()


def _ties(mesh, q, th, td):
    """Points where the two paths chose different tets, and whether each is a tie: the two tets' smallest barycentric
    coordinates within 1e-9 of each other, or one of them within 1e-9 of -padding.  Ties arise outside the mesh, where the best
    candidate wins and a structured mesh offers several tets at exactly the same distance: numpy's LU solve and the kernel's
    Cramer rule round differently, so either may win (and the clamped values then differ).  Inside, the first candidate wins."""
    diff = np.nonzero(td != th)[0]
    from stabilized_navier_stokes_flow_fenicsx_amd.interpolate import _bary
    mh = _bary(mesh.points[mesh.tets[th[diff]]], q[diff]).min(axis=1)
    md = _bary(mesh.points[mesh.tets[td[diff]]], q[diff]).min(axis=1)
    return diff, (np.abs(mh - md) <= 1e-9) | (np.minimum(np.abs(mh + PAD), np.abs(md + PAD)) <= 1e-9)


def _host_misses(mesh, pts):
    """Points whose bucket on the host's grid is empty (interpolate.locate_points' miss branch)."""
    X = mesh.points[mesh.tets]
    lo, hi = mesh.points.min(axis=0), mesh.points.max(axis=0)
    ext = np.maximum(hi - lo, 1e-300)
    E = len(mesh.tets)
    res = np.maximum(1, np.round((E / 6.0) ** (1.0 / 3.0) * ext / ext.max() * (ext.max() ** 3 / ext.prod()) ** (1 / 3)))
    res = res.astype(np.int64)
    h = ext / res
    tlo = np.clip(np.floor((X.min(axis=1) - lo) / h - 1e-9).astype(np.int64), 0, res - 1)
    thi = np.clip(np.floor((X.max(axis=1) - lo) / h + 1e-9).astype(np.int64), 0, res - 1)
    occ = np.zeros(tuple(res), dtype=bool)
    for t in range(E):
        occ[tlo[t, 0]:thi[t, 0] + 1, tlo[t, 1]:thi[t, 1] + 1, tlo[t, 2]:thi[t, 2] + 1] = True
    q = np.clip(np.floor((pts - lo) / h).astype(np.int64), 0, res - 1)
    return ~occ[q[:, 0], q[:, 1], q[:, 2]]


def test_misses_take_the_nearest_centroid(lib):
    """An L-shaped mesh leaves empty buckets in its bounding box: points there take the nearest centroid, like the host."""
    from stabilized_navier_stokes_flow_fenicsx_amd import interpolate as IP, mesh as M
    m = M.duct_mesh((8, 8, 4), 1.0, jitter=0.2)
    keep = m.points[m.tets].mean(axis=1)
    keep = ~((keep[:, 0] > 0.5) & (keep[:, 1] > 0.0))
    used = np.unique(m.tets[keep])
    remap = -np.ones(m.num_nodes, np.int64)
    remap[used] = np.arange(len(used))
    L = M.TetMesh(m.points[used], remap[m.tets[keep]].astype(np.int32), np.zeros((0, 3), np.int32), np.zeros(0, np.int32))
    rng = np.random.default_rng(4)
    q = rng.uniform((0.55, 0.05, -0.45), (0.95, 0.45, 0.45), (300, 3))
    th, lh = IP.locate_points(L, q)
    td, ld = IP.locate_points(L, q, device=DEV)
    miss = _host_misses(L, q)
    dm = IP._DeviceMesh(L, DEV)
    assert miss.sum() > 50 and locate_n_missed(dm, q) == miss.sum()
    assert np.array_equal(td[miss], th[miss]) and np.abs(ld - lh)[miss].max() <= 1e-12       # nearest centroid: the same bits
    diff, tie = _ties(L, q, th, td)
    print(f"\n  L-shaped mesh: {miss.sum()} of {len(q)} points missed, {len(diff)} other differences ({tie.sum()} ties)")
    assert tie.all() and len(diff) <= 3


def locate_n_missed(dm, q):
    from stabilized_navier_stokes_flow_fenicsx_amd.interpolate import _dev_array, locate_points_device
    return locate_points_device(dm, _dev_array(q, dm.device), PAD)[2]


def test_determinism(meshes):
    from stabilized_navier_stokes_flow_fenicsx_amd import interpolate as IP
    src, fine = meshes["delaunay"]
    q = np.concatenate([fine.points, _shared(src)])
    t1, l1 = IP.locate_points(src, q, device=DEV)
    t2, l2 = IP.locate_points(src, q, device=DEV)
    assert np.array_equal(t1, t2) and np.array_equal(l1.view(np.int64), l2.view(np.int64))


def test_refusals_on_device_arrays(lib, meshes):
    import torch
    from stabilized_navier_stokes_flow_fenicsx_amd.interpolate import _DeviceMesh, _stream
    src = meshes["duct"][0]
    dm = _DeviceMesh(src, DEV)
    q = torch.zeros((3, 3), dtype=torch.float64, device=DEV)
    tet = torch.zeros(3, dtype=torch.int32, device=DEV)
    lam = torch.full((3, 4), 0.25, dtype=torch.float64, device=DEV)
    vals = torch.ones((src.num_nodes, 5), dtype=torch.float64, device=DEV)
    out = torch.empty(3 * 5, dtype=torch.float64, device=DEV)
    p = lambda x: C.c_void_p(x.data_ptr())
    s = _stream(dm.device)
    nmiss = C.c_int64(0)
    loc = lambda n_tets, nq, pad: lib.sns_locate_points(src.num_nodes, n_tets, p(dm.pts), p(dm.tets), nq, p(q), pad, p(tet),
                                                        p(lam), C.byref(nmiss), s)
    assert loc(0, 3, PAD) == -4 and loc(src.num_tets, 3, -1e-6) == -1 and loc(src.num_tets, 0, PAD) == 0
    assert loc(src.num_tets, 3, PAD) == 0
    for nc in (0, 5):
        assert lib.sns_eval_p1(src.num_tets, p(dm.tets), nc, p(vals), 3, p(tet), p(lam), p(out), s) == -1
    assert lib.sns_eval_p1(0, p(dm.tets), 4, p(vals), 3, p(tet), p(lam), p(out), s) == -4
    assert lib.sns_eval_p1(src.num_tets, p(dm.tets), 4, p(vals), 0, p(tet), p(lam), p(out), s) == 0
    # a tet id outside the mesh evaluates to NaN instead of reading outside the arrays
    tet[1] = src.num_tets
    assert lib.sns_eval_p1(src.num_tets, p(dm.tets), 4, p(vals), 3, p(tet), p(lam), p(out), s) == 0
    o = out[:12].view(3, 4).cpu().numpy()
    assert np.isnan(o[1]).all() and np.isfinite(o[[0, 2]]).all()


@pytest.fixture(scope="module")
def channel(lib):
    """The driver's coarse stage (channel_mesh_size 0.1) solved, and its fine mesh (0.07)."""
    from stabilized_navier_stokes_flow_fenicsx_amd import drivers as D
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
    img = os.path.join(ROOT, "tests", "golden", "inlet_asym_offset.png")
    msh, bcs = D.channel_problem_inputs(img, 0.4, 0.1)
    P = FlowProblem(msh, bcs, device=DEV, reynolds=5.0, ksp_type="bicgstab")
    U, _ = P.stokes_solve()
    w, n = P.newton_solve(U.clone())
    assert n.reason > 0
    fine, bcs_f = D.channel_problem_inputs(img, 0.4, 0.07)
    yield dict(img=img, msh=msh, P=P, w=w, fine=fine, bcs_f=bcs_f)
    P.close()


def test_interpolate_initial_guess_on_the_device(channel):
    from stabilized_navier_stokes_flow_fenicsx_amd.interpolate import interpolate_initial_guess
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
    msh, fine, wc = channel["msh"], channel["fine"], channel["w"].cpu().numpy()
    g_host = interpolate_initial_guess(msh, wc, fine)
    g_dev = interpolate_initial_guess(msh, wc, fine, device=DEV)
    err = np.abs(g_dev - g_host).max() / np.abs(g_host).max()
    ws = []
    for g in (g_host, g_dev):
        Pf = FlowProblem(fine, channel["bcs_f"], device=DEV, reynolds=5.0, ksp_type="bicgstab")
        w, n = Pf.newton_solve(g.copy())
        assert n.reason > 0
        ws.append((w.cpu().numpy(), n.its))
        Pf.close()
    d = np.linalg.norm(ws[0][0] - ws[1][0]) / np.linalg.norm(ws[0][0])
    print(f"\n  warm start {msh.num_tets} -> {fine.num_tets} tets: guess difference {err:.1e}; Newton its {ws[0][1]} / {ws[1][1]}, "
          f"solution difference {d:.1e}")
    assert err <= 1e-12 and d <= 1e-6


def test_eval_at_of_a_solved_problem(channel):
    from stabilized_navier_stokes_flow_fenicsx_amd import interpolate as IP
    P, msh, w = channel["P"], channel["msh"], channel["w"]
    q = channel["fine"].points
    out = P.eval_at(w, q)
    t, lam = IP.locate_points(msh, q)
    ref = np.einsum("na,nac->nc", lam, w.cpu().numpy().reshape(-1, 4)[msh.tets[t]])
    assert out.shape == (len(q), 4) and np.abs(out - ref).max() <= 1e-12 * np.abs(ref).max()
    P.part = object()                       # a partitioned problem is refused with a message
    try:
        with pytest.raises(NotImplementedError, match="single-GPU"):
            P.eval_at(w, q[:3])
    finally:
        P.part = None


def test_streamtrace_seed_location_on_the_device(channel):
    """The pipeline's seeds (inner inlet nodes forward, 12 x 12 plane seeds in reverse) on the solved channel: the same starting
    tets, trace status and step counts with locate="device"."""
    from stabilized_navier_stokes_flow_fenicsx_amd import inlet_contours as IC, streamtrace as ST
    msh, w = channel["msh"], channel["w"].cpu().numpy().reshape(-1, 4)
    vel = w[:, :3].copy()
    prof = IC.solve_inlet_profiles(channel["img"], 0.5, max_pixels=1024)
    used = np.unique(prof.inner.tris)
    fwd_seeds = np.hstack([np.zeros((len(used), 1)), prof.inner.points[used]])
    rev_seeds = ST.make_rev_streamtrace_seeds(-0.3, 0.3, -0.3, 0.3, 12)
    nbr = ST.tet_face_neighbors(msh.tets)
    for seeds, rev in ((fwd_seeds, False), (rev_seeds, True)):
        a = ST.run_streamtrace(msh, vel, seeds, reverse=rev, nbr=nbr)
        b = ST.run_streamtrace(msh, vel, seeds, reverse=rev, nbr=nbr, locate="device")
        diff, tie = _ties(msh, seeds, a["seed_tet"], b["seed_tet"])
        print(f"\n  {len(seeds)} {'reverse' if rev else 'forward'} seeds: {len(diff)} different starting tets ({tie.sum()} ties)")
        assert tie.all() and len(diff) <= 0.02 * len(seeds)                    # ties: seeds on the nozzle wall, outside the mesh
        assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["steps"], b["steps"])
        assert np.allclose(a["pos"], b["pos"], rtol=0, atol=1e-12)


def test_size_guard_648k_tets(lib):
    """The 896 761 nodes of the 240 x 60 x 60 duct located on the 120 x 30 x 30 duct (648 000 tets; 25.9 s on the host)."""
    import torch
    from stabilized_navier_stokes_flow_fenicsx_amd import interpolate as IP, mesh as M
    IP.locate_points(M.duct_mesh((4, 2, 2)), np.zeros((1, 3)), device=DEV)                # code objects loaded
    src, fine = M.duct_mesh((120, 30, 30)), M.duct_mesh((240, 60, 60))
    assert src.num_tets == 648000 and fine.num_nodes == 896761
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t, lam = IP.locate_points(src, fine.points, device=DEV)
    dt = time.perf_counter() - t0
    print(f"\n  locate {fine.num_nodes} points on {src.num_tets} tets on the device: {dt:.3f} s (host arrays in and out)")
    assert (t >= 0).all() and np.abs(np.einsum("na,nad->nd", lam, src.points[src.tets[t]]) - fine.points).max() < 1e-12
    assert dt < 2.0
