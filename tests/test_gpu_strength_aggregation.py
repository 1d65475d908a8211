"""The fine-level aggregation by operator strength (amg_aggregation = 1) on the GPU: the strength kernel (csrc/sns_strength.hip,
SNS_EXPORT_STRENGTH) against a numpy restatement of the exported operator, the level-0 map the hierarchy build made from it
(SNS_EXPORT_AGG0) against sns_host_aggregate_strength, and what the option is for -- the iteration count on a sliver-rich mesh --
with the checks that it does no harm on good meshes and on a partitioned handle."""
import numpy as np
import pytest

from conftest import golden, rel
from test_host_strength_aggregation import strength

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
    return FlowProblem


def _channel(m):
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B
    return B.channel_bcs(m, *B.two_stream_profiles(0.5))


def _strength_of(P):
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    s = P.sizes()
    return P.export(_lib.EXPORT_STRENGTH, torch.float32, s["nnzb"]).cpu().numpy()


@pytest.mark.parametrize("kind", ["duct", "delaunay"])
def test_strength_kernel_vs_numpy(gpu, kind):
    """SNS_EXPORT_STRENGTH of the Stokes operator and of a Navier-Stokes Jacobian against the numpy restatement computed from
    SNS_EXPORT_ROWPTR / COLIND / VALS: relative error <= 1e-6 per slot (fp32 output); rows of odd and even block counts."""
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B, mesh as M
    if kind == "duct":
        m = M.duct_mesh((12, 4, 4), 2.0, jitter=0.1)
        bcs = B.duct_bcs(m)
    else:
        m = M.delaunay_channel_mesh(8, lattice="cubic")
        bcs = _channel(m)
    P = gpu(m, bcs, reynolds=50.0)
    U, r = P.stokes_solve()
    assert r.reason > 0
    for form in ("stokes", "ns"):
        if form == "ns":
            P.jacobian(U, "ns", residual_out=P.zeros())
        rp, ci, va = (t.cpu().numpy() for t in P.bsr())
        cnt = np.diff(rp)
        assert (cnt % 2 == 0).any() and (cnt % 2 == 1).any()
        want = strength(rp, ci, va)
        got = _strength_of(P)
        assert got.dtype == np.float32 and got.shape == want.shape
        err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.maximum(np.abs(want.astype(np.float64)), 1e-30)
        assert err.max() <= 1e-6, (kind, form, err.max())
        rows = np.repeat(np.arange(len(rp) - 1), cnt)
        assert (got[rows == ci] == 0).all() and (got[rows != ci] > 0).mean() > 0.5
    P.close()


def test_agg0_is_the_host_aggregation_of_the_gpu_strength(gpu):
    """The level-0 map the hierarchy build made (SNS_EXPORT_AGG0) is sns_host_aggregate_strength of the strength of the first
    assembled operator (the Stokes operator), exactly; it stays frozen through the Newton solve.  2-D handles refuse the option."""
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib, mesh as M, mesh2d as M2
    m = M.delaunay_channel_mesh(8, lattice="cubic")
    P = gpu(m, _channel(m), reynolds=50.0, amg_aggregation=1)
    assert P.lib.sns_pc_setup(P.h) == -3                          # SNS_E_STATE: no assembled operator to aggregate by yet
    U, r = P.stokes_solve()                                       # (the handle is as it was: the solve builds the hierarchy)
    assert r.reason > 0
    s = _strength_of(P)
    rp, ci, _ = (t.cpu().numpy() for t in P.bsr())
    agg = P.export(_lib.EXPORT_AGG0, torch.int32, m.num_nodes).cpu().numpy()
    want, nc = _lib.host_aggregate_strength(rp, ci, s)
    assert (agg == want).all()
    H = P.hierarchy()
    assert H[1]["rows"] == nc
    assert P.cycle()[0]["kind"] == 1                              # the fine level runs the aggregate blocks
    w, n = P.newton_solve(U.clone())
    assert n.reason > 0
    assert (P.export(_lib.EXPORT_AGG0, torch.int32, m.num_nodes).cpu().numpy() == want).all()
    P.close()
    # the default handle's map is the geometric aggregation
    P = gpu(m, _channel(m), reynolds=50.0)
    P.stokes_solve()
    agg_d = P.export(_lib.EXPORT_AGG0, torch.int32, m.num_nodes).cpu().numpy()
    assert (agg_d == _lib.host_aggregate(rp, ci, None, 8, m.points)[0]).all()
    assert P.cycle()[0]["kind"] == 0
    P.close()
    c = golden("cavity2d_8.npz")
    m2 = M2.TriMesh(c["points"], c["tris"], np.zeros((0, 2), np.int32), np.zeros(0, np.int32))
    with pytest.raises(_lib.SnsError) as e:
        gpu(m2, (c["mask"], c["g"]), reynolds=float(c["Re"]), amg_aggregation=1)
    assert e.value.code == -1


def _run(gpu, m, **kw):
    P = gpu(m, _channel(m), reynolds=50.0, **kw)
    U, r = P.stokes_solve()
    w, n = P.newton_solve(U.clone())
    out = dict(stokes=r.its, reason=(r.reason, n.reason), newton=n.its, per_step=n.ksp_its / max(1, n.its),
               w=w.cpu().numpy(), fnorm=n.fnorms[-1])
    P.close()
    return out


def test_sliver_mesh_iterations(gpu):
    """What the option is for: the two-stream channel at Re 50 on the jittered-cubic Delaunay mesh (sliver-rich, 0.37 M tets).
    BiCGStab iterations per Newton step with amg_aggregation = 1 against the default and against amg_block_smooth = 2 alone (the
    same fine-level smoother on the geometric aggregates); the same converged solution."""
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
    m = M.delaunay_channel_mesh(24, lattice="cubic")
    assert 300_000 < m.num_tets < 500_000
    base = _run(gpu, m)
    blk = _run(gpu, m, amg_block_smooth=2)
    opt = _run(gpu, m, amg_aggregation=1)
    for name, o in (("default", base), ("amg_block_smooth=2", blk), ("amg_aggregation=1", opt)):
        print(f"  {m.num_tets} tets {name:20s} stokes its {o['stokes']:4d}  newton {o['newton']} its reason {o['reason']}  "
              f"ksp its/step {o['per_step']:.1f}")
    assert base["reason"][1] > 0 and opt["reason"] == base["reason"]
    u = lambda w: w.reshape(-1, 4)[:, :3]
    assert rel(u(opt["w"]), u(base["w"])) < 1e-6
    # (measured: 82.5 / 90.8 / 40.2 iterations per Newton step)
    assert opt["per_step"] <= 0.5 * base["per_step"]
    assert opt["per_step"] <= 0.5 * blk["per_step"]


@pytest.mark.parametrize("kind", ["bcc", "structured"])
def test_no_harm_on_good_meshes(gpu, kind):
    """On the body-centred Delaunay mesh and the structured Kuhn box of about the same size the option converges within 1.3x the
    default's iterations per Newton step."""
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
    m = M.delaunay_channel_mesh(20) if kind == "bcc" else M.channel_mesh((96, 24, 24))
    base = _run(gpu, m)
    opt = _run(gpu, m, amg_aggregation=1)
    print(f"  {kind} {m.num_tets} tets: ksp its/step default {base['per_step']:.1f}, amg_aggregation=1 {opt['per_step']:.1f}")
    assert base["reason"][1] > 0 and opt["reason"][1] > 0
    assert opt["per_step"] <= 1.3 * base["per_step"]
    assert rel(opt["w"], base["w"]) < 1e-6


def test_partitioned_team_with_strength_aggregation(gpu):
    """A 2-rank in-process team with the option on (each rank aggregates its owned nodes by the strength of its rows, ghost
    columns' scales from the halo exchange) converges to the serial solution."""
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib, mesh as M, partition as PT
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import Team
    m = M.delaunay_channel_mesh(8, lattice="cubic")
    mask, g = _channel(m).flatten()
    Re = 50.0
    Ps = gpu(m, (mask, g), reynolds=Re, amg_aggregation=1)
    Us, rs = Ps.stokes_solve()
    s_serial = _strength_of(Ps)                                 # (of the Stokes operator)
    rp_s, ci_s, _ = (t.cpu().numpy() for t in Ps.bsr())
    ws, ns = Ps.newton_solve(Us.clone())
    Us, ws = Us.cpu().numpy(), ws.cpu().numpy()
    Ps.close()
    nranks = 2
    owner = PT.rcb_partition(m.points, nranks)
    team = Team(nranks)

    def work(rank, team):
        part = PT.build_local_part(m, mask, g, owner, rank, nranks)
        P = gpu(part.mesh, (part.bc_mask, part.bc_val), reynolds=Re, part=part, group=team, amg_aggregation=1)
        U, r = P.stokes_solve()
        # the strength of the owned rows (ghost columns included) is that of the serial operator's rows, restricted
        s = _strength_of(P)
        rp, ci, _ = (t.cpu().numpy() for t in P.bsr())
        agg = P.export(_lib.EXPORT_AGG0, torch.int32, part.mesh.num_nodes).cpu().numpy()
        w, n = P.newton_solve(U.clone())
        out = (part, U.cpu().numpy(), r, w.cpu().numpy(), n, s, rp, ci, agg, P.cycle()[0]["kind"])
        P.close()
        return out

    outs = team.run(work)
    team.close()
    Ug, wg = np.zeros(m.num_dofs), np.zeros(m.num_dofs)
    rows_s = np.repeat(np.arange(m.num_nodes), np.diff(rp_s))
    for part, U, r, w, n, s, rp, ci, agg, kind0 in outs:
        assert r.reason > 0 and n.reason == ns.reason and kind0 == 1
        no = part.n_owned
        gd = (4 * part.l2g[:no, None] + np.arange(4)[None]).ravel()
        Ug[gd], wg[gd] = U[:4 * no], w[:4 * no]
        assert (agg[:no] >= 0).all() and (agg[no:] == -1).all()
        assert (agg == _lib.host_aggregate_strength(rp, ci, s, n_active=no)[0]).all()
        rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
        own = rows < no
        key_l = part.l2g[rows[own]].astype(np.int64) * m.num_nodes + part.l2g[ci[own]]
        key_s = rows_s.astype(np.int64) * m.num_nodes + ci_s
        idx = np.searchsorted(key_s, key_l)
        assert (key_s[idx] == key_l).all()
        assert np.allclose(s[own], s_serial[idx], rtol=1e-6, atol=0)
    assert rel(Ug, Us) < 1e-6 and rel(wg, ws) < 1e-6
