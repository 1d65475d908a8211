"""The hybrid fine-level aggregation (amg_aggregation = 3, csrc/sns_aggregate.hip): on good meshes it re-matches nothing and runs
exactly what amg_aggregation = 0 runs; on a sliver-rich mesh its device map is the numpy restatement of
tests/test_host_hybrid_aggregation.py and it needs about the iterations of the aggregation by strength; on a 2-rank team every
rank's map is the restatement over its owned rows and both ranks plan the same cycle; the option's refusals."""
import numpy as np
import pytest

from conftest import golden, rel
from test_host_hybrid_aggregation import HALF_CELLS, PHI, half_jittered_channel, hybrid_map

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
    return FlowProblem


def _mesh(kind):
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B, mesh as M
    m = {"structured": lambda: M.channel_mesh((96, 24, 24)), "bcc": lambda: M.delaunay_channel_mesh(20),
         "cubic": lambda: M.delaunay_channel_mesh(24, lattice="cubic"), "cubic_small": lambda: M.delaunay_channel_mesh(8, lattice="cubic")}[kind]()
    return m, B.channel_bcs(m, *B.two_stream_profiles(0.5))


def _agg0(P, n):
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    return P.export(_lib.EXPORT_AGG0, torch.int32, n).cpu().numpy()


def _strength(P):
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    return P.export(_lib.EXPORT_STRENGTH, torch.float32, P.sizes()["nnzb"]).cpu().numpy()


def _built(gpu, m, bcs, **kw):
    P = gpu(m, bcs, reynolds=50.0, **kw)
    P.jacobian(None, "stokes")
    P.pc_setup()
    return P


def _run(gpu, m, bcs, **kw):
    P = gpu(m, bcs, reynolds=50.0, **kw)
    U, r = P.stokes_solve()
    agg = _agg0(P, m.num_nodes)
    kind0 = P.cycle()[0]["kind"]
    w, n = P.newton_solve(U.clone())
    out = dict(stokes=r.its, reason=(r.reason, n.reason), newton=n.its, ksp=n.ksp_its, fnorms=np.array(n.fnorms),
               w=w.cpu().numpy(), agg=agg, kind0=kind0)
    P.close()
    return out


@pytest.mark.parametrize("kind", ["structured", "bcc"])
def test_good_meshes_run_the_default_bitwise(gpu, kind):
    """Nothing re-matched: the map, the fine level's smoother, the Stokes count and the Newton history (residual norms and
    BiCGStab counts) equal amg_aggregation = 0's bit for bit."""
    m, bcs = _mesh(kind)
    a = _run(gpu, m, bcs)
    b = _run(gpu, m, bcs, amg_aggregation=3)
    assert a["reason"][1] > 0 and b["reason"] == a["reason"]
    assert (b["agg"] == a["agg"]).all()
    assert b["kind0"] == a["kind0"] == 0                     # SNS_LEVEL_NODAL_BLOCKS
    assert b["stokes"] == a["stokes"] and b["newton"] == a["newton"] and b["ksp"] == a["ksp"]
    assert np.array_equal(b["fnorms"], a["fnorms"])
    assert np.array_equal(b["w"], a["w"])


def test_sliver_map_is_the_restatement(gpu):
    """The device map equals the numpy restatement built from the handle's strength and a value-0 handle's map (some 2 % of the
    rows are marked here, more than HYBRID_PHI: everything is re-matched)."""
    m, bcs = _mesh("cubic")
    n = m.num_nodes
    P3 = _built(gpu, m, bcs, amg_aggregation=3)
    got = _agg0(P3, n)
    s = _strength(P3)
    rp, ci, _ = (t.cpu().numpy() for t in P3.bsr())
    kind0, rows1 = P3.cycle()[0]["kind"], P3.hierarchy()[1]["rows"]
    P3.close()
    P0 = _built(gpu, m, bcs)
    g = _agg0(P0, n)
    P0.close()
    want, nc, marked, F = hybrid_map(rp, ci, s, g, n)
    assert marked.any() and F.any()
    assert (got == want).all()
    assert rows1 == nc and kind0 == 1                          # SNS_LEVEL_AGGREGATE_BLOCKS


def test_sliver_iterations(gpu):
    """Two-stream channel at Re 50 on the jittered-cubic mesh: iterations per Newton step at most 1.2 x those of amg_aggregation
    = 2 and at most 0.55 x the default's; the same solution as the default's."""
    m, bcs = _mesh("cubic")
    r = {v: _run(gpu, m, bcs, amg_aggregation=v) for v in (0, 2, 3)}
    per = {v: r[v]["ksp"] / max(1, r[v]["newton"]) for v in r}
    print(f"  its per Newton step: 0 {per[0]:.1f}, 2 {per[2]:.1f}, 3 {per[3]:.1f}; stokes {r[0]['stokes']} {r[2]['stokes']} {r[3]['stokes']}")
    assert all(r[v]["reason"][1] > 0 for v in r)
    assert per[3] <= 1.2 * per[2]
    assert per[3] <= 0.55 * per[0]
    assert rel(r[3]["w"], r[0]["w"]) < 1e-6


def test_partitioned_team_with_hybrid_aggregation(gpu):
    """A 2-rank team: each rank's map is the restatement over its owned rows (from its strength and its geometric map), both
    ranks run the same plan with the fine-level aggregate blocks, and the team converges to the serial solution."""
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib, partition as PT
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import Team
    m, bcs = _mesh("cubic_small")
    mask, g = bcs.flatten()
    Ps = gpu(m, (mask, g), reynolds=50.0, amg_aggregation=3)
    Us, rs = Ps.stokes_solve()
    ws, ns = Ps.newton_solve(Us.clone())
    ws = ws.cpu().numpy()
    Ps.close()
    nranks = 2
    owner = PT.rcb_partition(m.points, nranks)
    team = Team(nranks)

    def work(rank, team):
        part = PT.build_local_part(m, mask, g, owner, rank, nranks)
        P = gpu(part.mesh, (part.bc_mask, part.bc_val), reynolds=50.0, part=part, group=team, amg_aggregation=3)
        U, r = P.stokes_solve()
        agg = _agg0(P, part.mesh.num_nodes)
        s = _strength(P)
        rp, ci, _ = (t.cpu().numpy() for t in P.bsr())
        w, n = P.newton_solve(U.clone())
        out = (part, r, w.cpu().numpy(), n, agg, s, rp, ci, P.cycle())
        P.close()
        return out

    outs = team.run(work)
    team.close()
    wg = np.zeros(m.num_dofs)
    plans, any_f = [], False
    for part, r, w, n, agg, s, rp, ci, cyc in outs:
        assert r.reason > 0 and n.reason > 0
        no = part.n_owned
        geo, _, _ = _lib.host_aggregate(rp, ci, no, 8, part.mesh.points)
        want, _, _, F = hybrid_map(rp, ci, s, geo, no)
        any_f |= bool(F.any())
        assert (agg == want).all()
        plans.append([(q["kind"], q["pre"], q["post"]) for q in cyc])
        gd = (4 * part.l2g[:no, None] + np.arange(4)[None]).ravel()
        wg[gd] = w[:4 * no]
    assert any_f
    assert plans[0] == plans[1] and plans[0][0][0] == 1
    assert rel(wg, ws) < 1e-6


def _half():
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B
    m, left = half_jittered_channel()
    return m, B.channel_bcs(m, *B.two_stream_profiles(0.5)), left


def test_half_jittered_channel_is_rematched_locally(gpu):
    """Slivers in the left half only, marked rows below HYBRID_PHI: the device dissolves a proper subset of the aggregates,
    compacts their subgraph, numbers the kept aggregates first and merges -- its map equals the restatement; the re-matched
    nodes lie within two cells of the jittered half and are at least 1 % of it; the fine level takes the aggregate blocks; and
    the Newton steps need no more BiCGStab iterations than value 0's, to the same solution."""
    m, bcs, left = _half()
    n = m.num_nodes
    P3 = _built(gpu, m, bcs, amg_aggregation=3)
    got = _agg0(P3, n)
    s = _strength(P3)
    rp, ci, _ = (t.cpu().numpy() for t in P3.bsr())
    kind0, rows1 = P3.cycle()[0]["kind"], P3.hierarchy()[1]["rows"]
    P3.close()
    P0 = _built(gpu, m, bcs)
    g = _agg0(P0, n)
    P0.close()
    want, nc, marked, F = hybrid_map(rp, ci, s, g, n)
    assert 0 < marked.sum() <= PHI * n and not F.all()
    assert (got == want).all()
    assert rows1 == nc and kind0 == 1
    assert (got[~F] == np.searchsorted(np.unique(g[~F]), g[~F])).all()       # the kept aggregates as value 0 built them
    assert F[left].mean() >= 0.01
    assert m.points[F, 0].max() <= 2.0 + 2 * 4.0 / HALF_CELLS[0]
    a = _run(gpu, m, bcs)
    b = _run(gpu, m, bcs, amg_aggregation=3)
    per = {v: r["ksp"] / max(1, r["newton"]) for v, r in ((0, a), (3, b))}
    print(f"  half-jittered channel: marked {marked.sum()} of {n}, |F| {F.sum()}; its per Newton step 0 {per[0]:.1f}, 3 {per[3]:.1f}; "
          f"stokes {a['stokes']} {b['stokes']}")
    assert a["reason"][1] > 0 and b["reason"][1] > 0
    assert per[3] <= per[0]
    assert rel(b["w"], a["w"]) < 1e-6


def test_team_with_slivers_on_one_rank(gpu):
    """The half-jittered channel split in x over 2 ranks: one rank re-matches, the other does not.  Each rank's map is the
    restatement over its owned rows, both ranks plan the fine-level aggregate blocks (the fact is agreed), and the team converges
    to the serial solution."""
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib, partition as PT
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import Team
    m, bcs, left = _half()
    mask, g = bcs.flatten()
    Ps = gpu(m, (mask, g), reynolds=50.0, amg_aggregation=3)
    Us, rs = Ps.stokes_solve()
    ws, ns = Ps.newton_solve(Us.clone())
    ws = ws.cpu().numpy()
    Ps.close()
    nranks = 2
    owner = (m.points[:, 0] >= 2.0).astype(np.int32)                          # rank 0: the jittered half
    team = Team(nranks)

    def work(rank, team):
        part = PT.build_local_part(m, mask, g, owner, rank, nranks)
        P = gpu(part.mesh, (part.bc_mask, part.bc_val), reynolds=50.0, part=part, group=team, amg_aggregation=3)
        U, r = P.stokes_solve()
        agg = _agg0(P, part.mesh.num_nodes)
        s = _strength(P)
        rp, ci, _ = (t.cpu().numpy() for t in P.bsr())
        w, n = P.newton_solve(U.clone())
        out = (part, r, w.cpu().numpy(), n, agg, s, rp, ci, P.cycle())
        P.close()
        return out

    outs = team.run(work)
    team.close()
    wg = np.zeros(m.num_dofs)
    plans, with_f = [], []
    for part, r, w, n, agg, s, rp, ci, cyc in outs:
        assert r.reason > 0 and n.reason > 0
        no = part.n_owned
        geo, _, _ = _lib.host_aggregate(rp, ci, no, 8, part.mesh.points)
        want, _, marked, F = hybrid_map(rp, ci, s, geo, no)
        with_f.append(bool(F.any()))
        assert (agg == want).all()
        plans.append([(q["kind"], q["pre"], q["post"]) for q in cyc])
        gd = (4 * part.l2g[:no, None] + np.arange(4)[None]).ravel()
        wg[gd] = w[:4 * no]
    assert with_f == [True, False]
    assert plans[0] == plans[1] and plans[0][0][0] == 1
    assert rel(wg, ws) < 1e-6


def test_hybrid_refusals(gpu):
    """A 2-D handle and amg_agg_size = 9 give SNS_E_ARG; a set-up before assembly gives SNS_E_STATE."""
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib, mesh2d as M2
    m, bcs = _mesh("cubic_small")
    P = gpu(m, bcs, reynolds=50.0, amg_aggregation=3)
    assert P.lib.sns_pc_setup(P.h) == -3
    with pytest.raises(_lib.SnsError) as e:
        P.set_options(amg_agg_size=9)
    assert e.value.code == -1
    U, r = P.stokes_solve()
    assert r.reason > 0
    P.close()
    with pytest.raises(_lib.SnsError) as e:
        gpu(m, bcs, reynolds=50.0, amg_aggregation=3, amg_agg_size=9)
    assert e.value.code == -1
    c = golden("cavity2d_8.npz")
    m2 = M2.TriMesh(c["points"], c["tris"], np.zeros((0, 2), np.int32), np.zeros(0, np.int32))
    with pytest.raises(_lib.SnsError) as e:
        gpu(m2, (c["mask"], c["g"]), reynolds=float(c["Re"]), amg_aggregation=3)
    assert e.value.code == -1
