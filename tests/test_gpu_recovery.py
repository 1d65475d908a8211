"""Gradient recovery on the GPU: sns_recover_gradient / sns_error_indicator (csrc/sns_recover.hip), FlowProblem.recover_gradient,
.derived_fields, .error_indicator, solver.zz_estimate and the SNS_DERIVED_FIELDS switch of the drivers, everything through the
C-ABI.

The yardstick is the numpy oracle tests/recovery_oracle.py (checked on the CPU by tests/test_host_recovery.py) at the project's
operator tolerance 1e-12 with conftest.rel: recovery is linear in w.  Q is the exception, its two terms cancel:
max |Q - Q_oracle| <= 1e-12 * max_i (|Omega|^2 + |S|^2) / 2, both sides taken over the oracle's values."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import recovery_oracle as RO
from conftest import ROOT, golden, rel
from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B
from stabilized_navier_stokes_flow_fenicsx_amd import functionals as Fn
from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
from stabilized_navier_stokes_flow_fenicsx_amd import mesh2d as M2
from stabilized_navier_stokes_flow_fenicsx_amd import partition as PT
from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem, Team, zz_estimate

pytestmark = pytest.mark.gpu
TOL = 1e-12                                          # the project's operator tolerance
E_STATE = -3


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _problem(pts, cells, **kw):
    n = len(pts)
    if pts.shape[1] == 2:
        m = M2.TriMesh(np.ascontiguousarray(pts), np.ascontiguousarray(cells, dtype=np.int32), np.zeros((0, 2), np.int32),
                       np.zeros(0, np.int32))
    else:
        m = M.TetMesh(np.ascontiguousarray(pts), np.ascontiguousarray(cells, dtype=np.int32), np.zeros((0, 3), np.int32),
                      np.zeros(0, np.int32))
    return FlowProblem(m, (np.zeros(4 * n, np.uint8), np.zeros(4 * n)), reynolds=10.0, **kw)


def _golden_script():
    spec = importlib.util.spec_from_file_location("make_recovery_golden", os.path.join(ROOT, "scripts", "make_recovery_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _check_against_oracle(P, pts, cells, w, label):
    """G, D, eta2, g2 of the handle against the oracle; returns the GPU's (G, D, eta2, g2) as numpy."""
    wd = _dev(w)
    G, D = P.recover_gradient(wd), P.derived_fields(wd)
    eta2, g2 = P.error_indicator(wd, G)
    G, D, eta2, g2 = (t.cpu().numpy() for t in (G, D, eta2, g2))
    Go = RO.recover(pts, cells, w)
    Do = RO.derived(Go)
    eo, go = RO.indicator(pts, cells, w, Go)
    q_err, q_bound = np.abs(D[:, 3] - Do[:, 3]).max(), TOL * RO.q_scale(Go)
    nq = [0, 1, 2, 4, 5]
    print(f"{label}: G {rel(G, Go):.2e} D(not Q) {rel(D[:, nq], Do[:, nq]):.2e} Q {q_err:.2e} (bound {q_bound:.2e}) "
          f"eta2 {rel(eta2, eo):.2e} g2 {rel(g2, go):.2e}")
    assert G.shape == (len(pts), 4, 3) and D.shape == (len(pts), 6) and eta2.shape == g2.shape == (len(cells),)
    assert rel(G, Go) < TOL
    assert rel(D[:, nq], Do[:, nq]) < TOL
    assert q_err <= q_bound
    assert rel(eta2, eo) < TOL and rel(g2, go) < TOL
    return G, D, eta2, g2


# ---- 1. single cells: only the masked tail of the list walk runs -------------------------------------------------------------
@pytest.mark.parametrize("flip", [False, True], ids=["as-drawn", "flipped"])
@pytest.mark.parametrize("dim", [3, 2])
def test_single_cell_in_both_orientations(dim, flip):
    rng = np.random.default_rng(60 + dim)
    pts = rng.standard_normal((dim + 1, dim))
    cells = np.arange(dim + 1, dtype=np.int32)[None, :].copy()
    if flip:
        cells[0, [0, 1]] = cells[0, [1, 0]]
    w = rng.standard_normal(4 * (dim + 1))
    P = _problem(pts, cells)
    G, _, _, _ = _check_against_oracle(P, pts, cells, w, f"one cell, dim {dim}, flip {flip}")
    P.close()
    assert np.abs(G - G[0]).max() == 0.0             # every node has the one cell's gradient
    if dim == 2:
        assert not G[:, :, 2].any()


# ---- 2. a connected mesh with both orientations -----------------------------------------------------------------------------
def test_channel_mesh_with_permuted_cells():
    """channel_mesh((9, 5, 4), jitter=0.2): 300 nodes (no multiple of the 64 nodes of a block), the cell-local vertex order
    permuted at random (both orientations), valences from the tail-only to several full batches of 8; random w."""
    m = M.channel_mesh((9, 5, 4), jitter=0.2)
    rng = np.random.default_rng(62)
    cells = np.stack([t[rng.permutation(4)] for t in m.tets]).astype(np.int32)
    X = m.points[cells]
    det = np.linalg.det(X[:, 1:] - X[:, :1])
    val = np.bincount(cells.ravel(), minlength=m.num_nodes)
    assert (det > 0).any() and (det < 0).any() and val.min() < 8 and val.max() >= 24 and m.num_nodes == 300
    w = rng.standard_normal(4 * m.num_nodes)
    P = _problem(m.points, cells)
    G, D, eta2, g2 = _check_against_oracle(P, m.points, cells, w, "channel")
    wd = _dev(w)
    D_only = P.derived_fields(wd)
    Gt = P.recover_gradient(wd)
    assert np.array_equal(D_only.cpu().numpy(), D)                         # D does not depend on whether G is stored
    assert np.array_equal(Gt.cpu().numpy(), G)                             # two calls agree bit for bit
    assert np.array_equal(P.derived_fields(wd).cpu().numpy(), D)
    e2, gg = P.error_indicator(wd)                                         # G = None: the handle's temporary
    assert np.array_equal(e2.cpu().numpy(), eta2) and np.array_equal(gg.cpu().numpy(), g2)
    # both outputs in one call (the C-ABI directly)
    Gb, Db = torch.empty_like(Gt), torch.empty_like(D_only)
    assert P.lib.sns_recover_gradient(P.h, wd.data_ptr(), Gb.data_ptr(), Db.data_ptr()) == 0
    assert np.array_equal(Gb.cpu().numpy(), G) and np.array_equal(Db.cpu().numpy(), D)
    # eta2 alone
    e3 = torch.empty_like(e2)
    assert P.lib.sns_error_indicator(P.h, wd.data_ptr(), Gt.data_ptr(), e3.data_ptr(), None) == 0
    assert np.array_equal(e3.cpu().numpy(), eta2)
    # refusals before any GPU work
    assert P.lib.sns_recover_gradient(P.h, wd.data_ptr(), None, None) == -1
    assert P.lib.sns_recover_gradient(P.h, None, Gb.data_ptr(), None) == -1
    assert P.lib.sns_error_indicator(P.h, wd.data_ptr(), None, None, None) == -1
    P.close()


# ---- 3. irregular valences, 2-D, and the committed fixture ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["duct", "tri"])
def test_fixture_meshes(name):
    """delaunay_duct_mesh(n=6) (valences up to 42) and the jittered triangle mesh of scripts/make_recovery_golden.py: against the
    oracle and against the arrays of tests/golden/recovery_cases.npz."""
    g = golden("recovery_cases.npz")
    pts, cells = _golden_script().meshes()[name]
    w = g[f"{name}_w"]
    assert len(w) == 4 * len(pts)
    P = _problem(pts, cells)
    G, D, eta2, _ = _check_against_oracle(P, pts, cells, w, name)
    P.close()
    assert rel(G, g[f"{name}_G"]) < TOL and rel(eta2, g[f"{name}_eta2"]) < TOL
    nq = [0, 1, 2, 4, 5]
    assert rel(D[:, nq], g[f"{name}_D"][:, nq]) < TOL
    assert np.abs(D[:, 3] - g[f"{name}_D"][:, 3]).max() <= TOL * RO.q_scale(g[f"{name}_G"])
    if name == "tri":
        assert not G[:, :, 2].any()


# ---- 4. affine field ---------------------------------------------------------------------------------------------------------
def test_affine_field_on_the_jittered_duct():
    from test_host_recovery import affine_state
    m = M.duct_mesh((8, 4, 4), 2.0, jitter=0.2)
    A, w = affine_state(m.points, 41)
    P = FlowProblem(m, B.duct_bcs(m).flatten(), reynolds=10.0)
    G = P.recover_gradient(_dev(w)).cpu().numpy()
    eta, eta_rel, eta2 = zz_estimate(P, _dev(w))
    P.close()
    print("affine: G", rel(G, np.broadcast_to(A, G.shape)), "eta_rel", eta_rel)
    assert rel(G, np.broadcast_to(A, G.shape)) < 1e-12
    assert eta_rel < 1e-11 and eta2.shape == (m.num_tets,)


# ---- 5. state independence ---------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_handle_state_and_nothing_else_is_written():
    m = M.duct_mesh((6, 3, 3), 2.0, jitter=0.2)
    rng = np.random.default_rng(65)
    w = _dev(rng.standard_normal(m.num_dofs))
    bcs = B.duct_bcs(m).flatten()

    def run(P):
        F0 = P.residual(w).clone()
        G, D = P.recover_gradient(w), P.derived_fields(w)
        e_none = P.error_indicator(w)
        e_G = P.error_indicator(w, G)
        assert torch.equal(P.residual(w), F0)                              # nothing the residual reads was written
        assert torch.equal(e_none[0], e_G[0]) and torch.equal(e_none[1], e_G[1])
        return [t.cpu().numpy() for t in (G, D, *e_G)]

    P = FlowProblem(m, bcs, reynolds=10.0)
    plain = run(P)
    P.set_viscosity_law(2.0, 0.5, 0.01)
    law = run(P)
    P.clear_viscosity_law()
    P.set_time_term(3.0, 11.0, rng.standard_normal(m.num_dofs))
    tt = run(P)
    P.close()
    for a, b, c in zip(plain, law, tt):
        assert np.array_equal(a, b) and np.array_equal(a, c)


# ---- 6. partitioned handles are refused --------------------------------------------------------------------------------------
def test_partitioned_handle_is_refused():
    """An in-process team of 2: both entry points return SNS_E_STATE with the reason in the error text, before any launch or
    collective (each rank returns on its own, so nothing can hang)."""
    team = Team(2)

    def work(rank, team):
        P = FlowProblem.from_part(PT.duct_slab_part((8, 3, 3), 2.0, rank, 2), group=team, reynolds=10.0)
        w = P.zeros()
        G = torch.zeros(12 * P.n_local, dtype=torch.float64, device="cuda")
        e = torch.zeros(len(P.mesh.tets), dtype=torch.float64, device="cuda")
        rc = (P.lib.sns_recover_gradient(P.h, w.data_ptr(), G.data_ptr(), None),
              P.lib.sns_error_indicator(P.h, w.data_ptr(), None, e.data_ptr(), None))
        msg = P.lib.sns_last_error().decode()
        P.close()
        return rc, msg

    out = team.run(work)
    team.close()
    for rc, msg in out:
        assert rc == (E_STATE, E_STATE)
        assert "communicator" in msg


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------
def test_duct_driver_with_derived_fields(tmp_path, monkeypatch, capsys):
    """DuctStokesFlow.py at the size of the driver test of tests/test_gpu_parity.py, switch off and on in the same test: the run
    with SNS_DERIVED_FIELDS=1 adds three file pairs and one line, everything else is byte for byte the run without."""
    import h5read_min as R
    from stabilized_navier_stokes_flow_fenicsx_amd import drivers as D
    argv = ["DuctStokesFlow.py", "ductmesh", "0.25", "2.0"]
    runs = {}
    for switch in ("0", "1"):
        d = tmp_path / switch
        d.mkdir()
        monkeypatch.chdir(d)
        if switch == "1":
            monkeypatch.setenv("SNS_DERIVED_FIELDS", "1")
        else:
            monkeypatch.delenv("SNS_DERIVED_FIELDS", raising=False)
        msh, W, res = D.duct_stokes_main(argv)
        assert res.reason > 0
        runs[switch] = (msh, W, capsys.readouterr().out, {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))})
    msh, W, out0, files0 = runs["0"]
    _, W1, out1, files1 = runs["1"]
    extra = sorted(set(files1) - set(files0))
    assert extra == sorted(f"StokesDuct{label}.{ext}" for label in ("Vorticity", "QCriterion", "ShearRate") for ext in ("h5", "xdmf"))
    assert np.array_equal(W, W1) and all(files1[f] == files0[f] for f in files0)
    lines1 = out1.splitlines()
    zz_lines = [ln for ln in lines1 if ln.startswith("ZZ error estimate")]
    assert len(zz_lines) == 1 and [ln for ln in lines1 if ln not in zz_lines] == out0.splitlines()
    assert "ZZ" not in out0

    P = FlowProblem(msh, B.duct_bcs(msh).flatten())
    w = _dev(W.ravel())
    Dg = P.derived_fields(w).cpu().numpy()
    G = P.recover_gradient(w).cpu().numpy()
    eta, eta_rel, _ = zz_estimate(P, w)
    nu = 1.0 / P.options.reynolds
    P.close()
    assert 0.0 < eta_rel < 1.0
    assert zz_lines[0] == f"ZZ error estimate of grad u: eta {eta} eta_rel {eta_rel}"
    d1 = tmp_path / "1"
    for label, name, ref in (("Vorticity", "vorticity", Dg[:, :3]), ("QCriterion", "q_criterion", Dg[:, 3:4]),
                             ("ShearRate", "shear_rate", Dg[:, 4:5])):
        back = R.H5File(str(d1 / f"StokesDuct{label}.h5"))["Function"][name]["0"]
        assert np.array_equal(back, ref)

    # wall shear stress of the developed profile.  n = -outward normal, the orientation of boundary_traction_force: tau_w is the
    # stress the fluid puts on the wall, along the flow (+x); the stress the wall puts on the fluid is its negative (-x).
    wall = msh.meta["tags"]["wall"]
    nodes, tau = Fn.wall_shear_stress(msh, G, nu, wall)
    F = Fn.boundary_traction_force(msh, W.ravel(), nu, wall)
    x = msh.points[nodes, 0]
    dev = x >= 1.0                                                         # the developed half of the duct
    live = np.linalg.norm(tau, axis=1) > 0                                 # (corner nodes have only wall neighbours: G = 0)
    assert np.all(tau[:, 0] >= 0.0) and F[0] > 0.0
    assert np.all(np.linalg.norm(tau[dev & live, 1:], axis=1) < 0.05 * tau[dev & live, 0])
    tn = np.zeros((msh.num_nodes, 3))
    tn[nodes] = tau
    fn = msh.facets[msh.find(wall)]
    Pf = msh.points[fn]
    area = 0.5 * np.linalg.norm(np.cross(Pf[:, 1] - Pf[:, 0], Pf[:, 2] - Pf[:, 0]), axis=1)
    integral = (area[:, None] * tn[fn].mean(axis=1)).sum(axis=0)
    # Margin: on the CPU, the oracle's wall shear stress of the LU Stokes solution (oracle.solve.solve_stokes) on this very mesh,
    # duct_mesh((8, 4, 4), 2.0), integrated the same way, differs from boundary_traction_force's x component (the component
    # tangential to all four walls; the pressure has none there) by 1.36e-3 of it -- the recovered gradient averages over the
    # cells around a wall node, the force takes the cell behind each facet.  Doubled: 2.8e-3.
    print("wall shear: integral", integral, "traction force", F, "rel", abs(integral[0] - F[0]) / F[0])
    assert abs(integral[0] - F[0]) <= 2.8e-3 * F[0]
