"""The hybrid fine-level aggregation (amg_aggregation = 3) pinned on the host, no GPU: a numpy restatement of its rule -- mark the
rows whose geometric aggregate cuts a dominant coupling, dissolve their aggregates, re-match the dissolved nodes by
sns_host_aggregate_strength on their induced subgraph, merge -- with the properties the device build relies on, and the policy
rule that the fine-level aggregate blocks come with value 3 exactly when something was re-matched."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_host_strength_aggregation import sliver_mesh, strength  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAPPA = 4.0                      # csrc/sns_policy.h HYBRID_KAPPA
PHI = 0.01                       # csrc/sns_policy.h HYBRID_PHI


def hybrid_map(rp, ci, s, g, n_active, max_agg=8, kappa=KAPPA, phi=PHI):
    """(agg, nc, marked, F) of the hybrid rule over the first n_active nodes (ghosts -1): s = the raw strength (one fp32 value per
    block slot), g = the geometric map of amg_aggregation = 0.  Row i is marked when cut_i > kappa x max(kept_i, mean_i) over the
    symmetrised strength to owned neighbours (cut_i: the largest outside g(i)'s aggregate, kept_i: inside it, mean_i: the row's
    mean, alone for a singleton); the aggregates of marked rows are dissolved (F = their nodes; every node when more than phi of
    the rows are marked) and F is aggregated by
    sns_host_aggregate_strength on its induced subgraph; the kept aggregates come first in the order of their old ids."""
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    n = len(rp) - 1
    na = n_active
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    col = np.asarray(ci, np.int64)
    s = np.asarray(s, np.float32)
    key = rows * n + col
    tkey = col * n + rows
    t = np.minimum(np.searchsorted(key, tkey), len(key) - 1)
    sji = np.where(key[t] == tkey, s[t], np.float32(0.0))
    w = np.maximum(s, sji).astype(np.float64)
    act = (rows < na) & (col < na) & (rows != col)
    ga = np.asarray(g[:na], np.int64)
    same = np.zeros(len(rows), bool)
    same[act] = ga[rows[act]] == ga[col[act]]
    cut, kept = np.zeros(na), np.zeros(na)
    np.maximum.at(cut, rows[act & ~same], w[act & ~same])
    np.maximum.at(kept, rows[act & same], w[act & same])
    tot = np.bincount(rows[act], w[act], minlength=na)
    cnt = np.bincount(rows[act], minlength=na)
    mean = np.where(cnt > 0, tot / np.maximum(cnt, 1), 0.0)
    ng = int(ga.max()) + 1 if na else 0
    size = np.bincount(ga, minlength=ng)
    ref = np.where(size[ga] == 1, mean, np.maximum(kept, mean))
    marked = cut > kappa * ref
    dis = np.zeros(ng, bool)
    dis[ga[marked]] = True
    if marked.sum() > phi * na:
        dis[:] = True
    F = dis[ga]
    agg = np.full(n, -1, np.int32)
    nkept = int((~dis).sum())
    agg[:na] = (np.cumsum(~dis) - 1)[ga]
    nF = int(F.sum())
    if nF == 0:
        return agg, nkept, marked, F
    fid = np.cumsum(F) - 1
    slot = (rows < na) & (col < na)
    slot[slot] = F[rows[slot]] & F[col[slot]]
    srp = np.zeros(nF + 1, np.int32)
    srp[1:] = np.cumsum(np.bincount(fid[rows[slot]], minlength=nF))
    sagg, snc = _lib.host_aggregate_strength(srp, fid[col[slot]].astype(np.int32), s[slot], max_agg=max_agg)
    head = agg[:na]
    head[F] = nkept + sagg[fid[F]]
    return agg, nkept + snc, marked, F


HALF_CELLS, HALF_AMP = (48, 12, 12), 0.3


def half_jittered_channel(cells=HALF_CELLS, amp=HALF_AMP, seed=7):
    """(mesh, left) of the two-stream channel (mesh.channel_mesh) whose interior nodes with x < L/2 (`left`) are moved by up to
    amp x h per axis; a move that would invert a tet is halved until none does, so every volume keeps its sign and the moves
    that remain make near-flat tets in the left half only.  amp = 0.3 marks some 0.2 % of the rows (below HYBRID_PHI) and
    dissolves some 3 % of the left half."""
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
    m0 = M.channel_mesh(cells)
    b = m0.points
    left = b[:, 0] < 2.0
    h = np.array([4.0 / cells[0], 1.0 / cells[1], 1.0 / cells[2]])
    interior = (b[:, 0] > 1e-9) & (b[:, 0] < 4.0 - 1e-9) & (np.abs(b[:, 1]) < 0.5 - 1e-9) & (np.abs(b[:, 2]) < 0.5 - 1e-9)
    d = np.random.default_rng(seed).uniform(-amp, amp, size=b.shape) * h
    d[~(interior & left)] = 0.0

    def vol(p):
        q = p[m0.tets]
        return np.einsum("ij,ij->i", np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]), q[:, 3] - q[:, 0])

    s0 = np.sign(vol(b))
    for _ in range(60):
        bad = np.sign(vol(b + d)) != s0
        if not bad.any():
            break
        d[np.unique(m0.tets[bad])] *= 0.5
    d[np.unique(m0.tets[np.sign(vol(b + d)) != s0])] = 0.0
    return M.TetMesh(b + d, m0.tets, m0.facets, m0.facet_tags, name="channel", meta=m0.meta), left


def test_kappa_is_the_policy_constant():
    text = open(os.path.join(ROOT, "stabilized_navier_stokes_flow_fenicsx_amd", "csrc", "sns_policy.h")).read()
    assert float(re.search(r"constexpr double HYBRID_KAPPA = ([0-9.]+);", text).group(1)) == KAPPA
    assert float(re.search(r"constexpr double HYBRID_PHI = ([0-9.]+);", text).group(1)) == PHI


def _check_properties(g, agg, nc, F, n_active, max_agg=8):
    na = n_active
    assert (agg[:na] >= 0).all() and (agg[na:] == -1).all()                 # total over the owned nodes
    assert set(np.unique(agg[:na])) == set(range(nc))                        # numbered densely
    ga = g[:na]
    dis = np.zeros(int(ga.max()) + 1, bool)
    dis[ga[F]] = True
    assert (dis[ga] == F).all()                                              # F is a union of whole geometric aggregates
    keep = ~F
    kept_old = np.unique(ga[keep])
    # kept aggregates unchanged, numbered first in the order of their old ids
    assert (agg[:na][keep] == np.searchsorted(kept_old, ga[keep])).all()
    if F.any():
        new = agg[:na][F]
        assert new.min() >= len(kept_old)
        assert np.bincount(new - len(kept_old)).max() <= max_agg             # re-matched aggregates of at most max_agg nodes


def test_restatement_properties_on_the_sliver_mesh(built_lib, sliver_mesh):
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    m, rp, ci, vals, s = sliver_mesh
    n = m.num_nodes
    for n_active in (n, n - 37):
        g, ng, _ = _lib.host_aggregate(rp, ci, n_active, 8, m.points)
        for kappa in (KAPPA, 2.0):
            agg, nc, marked, F = hybrid_map(rp, ci, s, g, n_active, 8, kappa, phi=1.0)
            assert marked.any() and F.sum() < n_active                       # the case is what it is meant to be
            _check_properties(g, agg, nc, F, n_active)
    for max_agg in (3, 6):
        g, _, _ = _lib.host_aggregate(rp, ci, None, max_agg, m.points)
        agg, nc, _, F = hybrid_map(rp, ci, s, g, n, max_agg, phi=1.0)
        _check_properties(g, agg, nc, F, n, max_agg)


def test_rematched_part_is_the_host_matcher_on_the_subgraph(built_lib, sliver_mesh):
    """More than PHI of the rows marked (the sliver mesh marks some 2 %): everything is dissolved and the map is the strength
    matcher's on the whole graph (amg_aggregation = 2's map)."""
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    m, rp, ci, vals, s = sliver_mesh
    n = m.num_nodes
    for n_active in (n, n - 37):
        g, _, _ = _lib.host_aggregate(rp, ci, n_active, 8, m.points)
        agg, nc, marked, F = hybrid_map(rp, ci, s, g, n_active)
        assert marked.sum() > PHI * n_active and F.all()
        want, nc_w = _lib.host_aggregate_strength(rp, ci, s, n_active=n_active, max_agg=8)
        assert nc == nc_w and (agg == want).all()


def test_empty_F_gives_the_geometric_map(built_lib):
    """A structured channel: nothing is marked, and the map is exactly amg_aggregation = 0's."""
    from oracle import cport
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib, bcs as B, mesh as M
    m = M.channel_mesh((24, 6, 6))
    mask, gv = B.channel_bcs(m, *B.two_stream_profiles(0.5)).flatten()
    rp, ci = cport.pattern(m.num_nodes, m.tets)
    vals, _ = cport.assemble("stokes", m.points, m.tets, None, 50.0, mask, gv, rp, ci)
    s = strength(rp, ci, vals)
    g, ng, _ = _lib.host_aggregate(rp, ci, None, 8, m.points)
    agg, nc, marked, F = hybrid_map(rp, ci, s, g, m.num_nodes)
    assert not marked.any() and not F.any()
    assert nc == ng and (agg == g).all()


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("hybrid_plan") / "hybrid_plan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            "-I", os.path.join(ROOT, "stabilized_navier_stokes_flow_fenicsx_amd", "csrc"),
                            os.path.join(ROOT, "tests", "hybrid_plan_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    return exe


def _plan(exe, tmp_path, rows, rematched, nranks=1, **kw):
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    opt = tmp_path / "opt.bin"
    opt.write_bytes(ctypes.string_at(ctypes.byref(_lib.default_options(**kw)), ctypes.sizeof(_lib.SnsOptions)))
    run = subprocess.run([exe, str(opt), str(nranks), str(rematched)] + [str(r) for r in rows], capture_output=True, text=True)
    assert run.returncode == 0, run.returncode
    return [tuple(map(int, ln.split())) for ln in run.stdout.split("\n") if ln.strip()]


SERIAL = [1738576, 218044, 27436, 3800, 475]
PART = [1738576, 218044, 27436, 3800, 475]


def test_policy_hybrid(built_lib, plan_exe, tmp_path):
    """Value 3 plans as value 0 unless level 0 was re-matched; then its fine level takes the aggregate blocks (kind 1) as 1 and 2
    do.  Values 1 and 2 do not depend on the fact."""
    for rows, nranks in ((SERIAL, 1), (PART, 2), (PART, 8)):
        base = _plan(plan_exe, tmp_path, rows, -1, nranks)
        assert _plan(plan_exe, tmp_path, rows, -1, nranks, amg_aggregation=3) == base
        assert _plan(plan_exe, tmp_path, rows, 0, nranks, amg_aggregation=3) == base
        hyb = _plan(plan_exe, tmp_path, rows, 1, nranks, amg_aggregation=3)
        assert hyb[0][:2] == (1, 1)
        for v in (1, 2):
            strength_plan = _plan(plan_exe, tmp_path, rows, -1, nranks, amg_aggregation=v)
            assert strength_plan[0][:2] == (1, 1)
            assert _plan(plan_exe, tmp_path, rows, 0, nranks, amg_aggregation=v) == strength_plan
            assert _plan(plan_exe, tmp_path, rows, 1, nranks, amg_aggregation=v) == strength_plan
            assert hyb == strength_plan
    assert _plan(plan_exe, tmp_path, SERIAL, -1, 1)[0][:2] == (0, 0)        # (the default fine level: nodal blocks)
    assert _plan(plan_exe, tmp_path, SERIAL, 0, 1, amg_aggregation=3, amg_block_smooth=2)[0][:2] == (1, 1)


def test_host_cycle_policy_reports_the_unmatched_plan(built_lib):
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    T = lambda rows, **kw: [(r["kind"], r["pre"], r["post"]) for r in _lib.host_cycle_policy(rows, **kw)]
    assert T(SERIAL, amg_aggregation=3) == T(SERIAL)
    assert T(SERIAL, nranks=2, amg_aggregation=3) == T(SERIAL, nranks=2)


def test_half_jittered_channel_is_rematched_locally(built_lib):
    """The restatement on the half-jittered channel: every volume keeps its sign, the marked rows stay below HYBRID_PHI (only
    their aggregates are re-matched), at least 1 % of the jittered half is re-matched, and every re-matched node lies within
    two cells of the jittered half."""
    from oracle import cport
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib, bcs as B, mesh as M
    m, left = half_jittered_channel()
    m0 = M.channel_mesh(HALF_CELLS)
    q, q0 = m.points[m.tets], m0.points[m0.tets]
    vol = lambda p: np.einsum("ij,ij->i", np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), p[:, 3] - p[:, 0])
    assert (np.sign(vol(q)) == np.sign(vol(q0))).all() and (np.abs(vol(q)) > 0).all()
    mask, gv = B.channel_bcs(m, *B.two_stream_profiles(0.5)).flatten()
    rp, ci = cport.pattern(m.num_nodes, m.tets)
    vals, _ = cport.assemble("stokes", m.points, m.tets, None, 50.0, mask, gv, rp, ci)
    g, _, _ = _lib.host_aggregate(rp, ci, None, 8, m.points)
    agg, nc, marked, F = hybrid_map(rp, ci, strength(rp, ci, vals), g, m.num_nodes)
    assert 0 < marked.sum() <= PHI * m.num_nodes
    assert F[left].mean() >= 0.01 and not F.all()
    assert m.points[F, 0].max() <= 2.0 + 2 * 4.0 / HALF_CELLS[0]
    _check_properties(g, agg, nc, F, m.num_nodes)
