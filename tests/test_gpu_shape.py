"""Shape gradients on the GPU: sns_residual_shape_gradient (csrc/sns_shape.hip), FlowProblem.residual_shape_gradient and
solver.shape_sensitivity, everything through the C-ABI.

The yardstick of the kernel is the autograd oracle tests/shape_oracle.py (checked on the CPU by tests/test_host_shape.py) at
the project's operator tolerance 1e-12 relative to max |gX|; on top an oracle-free directional check against differences of
the GPU's own residual on moved meshes, and end-to-end sensitivities against Richardson-extrapolated central differences
of full Newton solves on moved meshes, with the band taken from the finite difference's own consistency."""
import copy

import numpy as np
import pytest
import torch

import shape_oracle as SO
from conftest import golden
from oracle import forms_literal as FL
from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B
from stabilized_navier_stokes_flow_fenicsx_amd import functionals as Fn
from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
from stabilized_navier_stokes_flow_fenicsx_amd import mesh2d as M2
from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem, SnsError, shape_sensitivity
from test_host_shape import richardson_band

pytestmark = pytest.mark.gpu
NU = 1e-3                                            # DFG_2D_Validation.py:148
RE_DUCT = 25.0
TIGHT = dict(ksp_rtol=1e-12, snes_rtol=1e-12, snes_atol=1e-12, snes_stol=1e-12)
TOL = 1e-12                                          # the project's operator tolerance
VARIANT = dict(ci=20.0, lsic=0.7, pspg=-1.0, one_point=True)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _moved(mesh, X):
    m = copy.copy(mesh)
    m.points = np.ascontiguousarray(X)
    return m


def _free(n):
    return np.zeros(4 * n, np.uint8), np.zeros(4 * n)


# ---- 1. single cells ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corrected", [0, 1])
def test_single_tets_against_the_oracle(corrected):
    """257 disconnected random tets (a second, partial workgroup), every node free, random state and lam: each cell's
    12 derivatives against autograd through the CPU form, 1e-12 of the cell's largest."""
    pts, tets, w, lam = SO.random_cells(257, 3, seed=21)
    m = M.TetMesh(pts, tets, np.zeros((0, 3), np.int32), np.zeros(0, np.int32))
    P = FlowProblem(m, _free(len(pts)), reynolds=7.0, corrected_convection=corrected)
    got = P.residual_shape_gradient(_dev(w), _dev(lam)).cpu().numpy().reshape(257, 4, 3)
    P.close()
    X, W, L, D = SO._cells3(pts, tets, w, lam, None)
    ref = SO.tet_cell_gradients(X, W, L, D, 7.0, corrected_convection=bool(corrected))
    err = np.abs(got - ref).max(axis=(1, 2)) / np.abs(ref).max(axis=(1, 2))
    print("single tets: worst cell", err.max())
    assert err.max() <= TOL


@pytest.mark.parametrize("scale,nu", [(1.0, 0.01), (1.0, 1.0)], ids=["Re_UGN>3", "Re_UGN<=3"])
def test_single_triangles_against_the_oracle(scale, nu):
    pts, tris, w, lam = SO.random_cells(257, 2, seed=22)
    w = scale * w
    m = M2.TriMesh(pts, tris, np.zeros((0, 2), np.int32), np.zeros(0, np.int32))
    P = FlowProblem(m, _free(len(pts)), reynolds=1.0 / nu)
    got = P.residual_shape_gradient(_dev(w), _dev(lam)).cpu().numpy().reshape(257, 3, 3)
    P.close()
    p3 = np.zeros((len(pts), 3))
    p3[:, :2] = pts
    X, W, L = SO._cells2(p3, tris, w, lam)
    ref = SO.tri_cell_gradients(X, W, L, nu)
    err = np.abs(got[:, :, :2] - ref).max(axis=(1, 2)) / np.abs(ref).max(axis=(1, 2))
    print("single triangles: worst cell", err.max())
    assert err.max() <= TOL and np.all(got[:, :, 2] == 0.0)


# ---- 2. connected meshes -------------------------------------------------------------------------------------------------
def _golden_duct():
    g = golden("duct_8x2x2.npz")
    pts, tets = g["points"].copy(), g["tets"]
    e = pts[tets[:, [0, 0, 0, 1, 1, 2]]] - pts[tets[:, [1, 2, 3, 2, 3, 3]]]
    h = np.sqrt((e * e).sum(axis=2)).min()
    pts += 0.2 * h * np.random.default_rng(23).uniform(-0.5, 0.5, pts.shape)
    return M.TetMesh(pts, tets, np.zeros((0, 3), np.int32), np.zeros(0, np.int32)), (g["mask"], g["g"]), float(g["Re"])


def _dense_duct():
    m = M.duct_mesh((4, 3, 3), 2.0, jitter=0.2)
    assert np.bincount(m.tets.ravel()).max() > 8                     # the gather reads such a node's cells in batches
    return m, B.duct_bcs(m).flatten(), RE_DUCT


@pytest.fixture(scope="module")
def meshes3d():
    return {"golden": _golden_duct(), "dense": _dense_duct()}


@pytest.mark.parametrize("variant", ["c0", "c1", "perturbed", "transient"])
@pytest.mark.parametrize("case", ["golden", "dense"])
def test_connected_3d_against_the_oracle(meshes3d, case, variant):
    m, bcs, Re = meshes3d[case]
    rng = np.random.default_rng(24)
    w, lam, d = (rng.standard_normal(m.num_dofs) for _ in range(3))
    P = FlowProblem(m, bcs, reynolds=Re, corrected_convection=int(variant == "c1"))
    kw, old = dict(corrected_convection=variant == "c1"), dict(FL.VARIANT)
    if variant == "perturbed":
        P.set_form_variant(VARIANT["ci"], VARIANT["lsic"], VARIANT["pspg"], VARIANT["one_point"])
        FL.VARIANT.update(VARIANT)
    if variant == "transient":
        P.set_time_term(3.0, 11.0, _dev(d))
        kw.update(d=d, sigma=3.0, theta=11.0)
    try:
        ref = SO.gradient_3d(m.points, m.tets, w, lam, Re, **kw)
    finally:
        FL.VARIANT.update(old)
    got = P.residual_shape_gradient(_dev(w), _dev(lam)).cpu().numpy()
    P.close()
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"connected {case} {variant}: {err:.2e}")
    assert err <= TOL


def _dfg_jittered(seed=25):
    m = M2.dfg_2d_mesh(0.5)
    pts = m.points.copy()
    e = np.concatenate([m.tris[:, [0, 1]], m.tris[:, [1, 2]], m.tris[:, [2, 0]]])
    ln = np.linalg.norm(pts[e[:, 0]] - pts[e[:, 1]], axis=1)
    hmin = np.full(len(pts), np.inf)
    np.minimum.at(hmin, e[:, 0], ln)
    np.minimum.at(hmin, e[:, 1], ln)
    interior = np.setdiff1d(np.arange(len(pts)), np.unique(m.facets))
    pts[interior] += 0.2 * hmin[interior, None] * np.random.default_rng(seed).uniform(-0.5, 0.5, (len(interior), 2))
    return _moved(m, pts)


def test_connected_2d_against_the_oracle():
    m = _dfg_jittered()
    rng = np.random.default_rng(26)
    w, lam = 0.3 * rng.standard_normal(m.num_dofs), rng.standard_normal(m.num_dofs)
    P = FlowProblem(m, M2.dfg2d_bcs(m).flatten(), reynolds=1.0 / NU)
    got = P.residual_shape_gradient(_dev(w), _dev(lam)).cpu().numpy()
    P.close()
    p3 = np.zeros((m.num_nodes, 3))
    p3[:, :2] = m.points
    ref = SO.gradient_2d(p3, m.tris, w, lam, NU)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"connected dfg2d: {err:.2e}")
    assert err <= TOL and np.all(got[:, 2] == 0.0)


# ---- 3. oracle-free directional check, 6. explicit part of the reaction force ------------------------------------------------
def _state_on(bcs, n, seed, amp=1.0):
    mask, g = bcs
    w = amp * np.random.default_rng(seed).standard_normal(4 * n)
    w[mask.astype(bool)] = g[mask.astype(bool)]
    return w


def _directional(m, bcs, V, opt, w, lam, dim):
    P = FlowProblem(m, bcs, **opt)
    gX = P.residual_shape_gradient(_dev(w), _dev(lam)).cpu().numpy()
    P.close()
    e = m.points[(m.tris if dim == 2 else m.tets)[:, [0, 0, 1]]] - m.points[(m.tris if dim == 2 else m.tets)[:, [1, 2, 2]]]
    h = np.sqrt((e * e).sum(axis=2)).min()

    def D_of(delta):
        F = []
        for s in (1.0, -1.0):
            Q = FlowProblem(_moved(m, m.points + s * delta * h * V[:, :dim]), bcs, **opt)
            F.append(Q.residual(_dev(w)).cpu().numpy())
            Q.close()
        return lam @ (F[0] - F[1]) / (2.0 * delta * h)

    Dstar, band = richardson_band(D_of, 2e-4)
    got = float((gX * V).sum())
    print(f"directional {dim}-D: gX.V {got:.12e} D* {Dstar:.12e} band {band:.2e} = {band / abs(Dstar):.2e} |D*|; diff {abs(got - Dstar):.2e}")
    assert band <= 1e-6 * abs(Dstar)
    assert abs(got - Dstar) <= band


def test_directional_check_3d(meshes3d):
    """lam . [F(w; X + eV) - F(w; X - eV)] / (2e) from the GPU's own residual on two moved meshes (same mask and Dirichlet
    values, a state that satisfies them, lam masked on the Dirichlet dofs) against gX . V, inside the Richardson band over
    e, e/2 (e = 2e-4 of the smallest edge), which must itself be below 1e-6 of the value."""
    m, bcs, Re = meshes3d["golden"]
    w = _state_on(bcs, m.num_nodes, 27)
    lam = np.random.default_rng(28).standard_normal(m.num_dofs) * (bcs[0] == 0)
    x = m.points
    V = np.stack([np.sin(2.0 * x[:, 1]) * np.cos(x[:, 0]), np.cos(1.5 * x[:, 0] + x[:, 2]), np.sin(x[:, 0] * x[:, 1] + 0.3)], axis=1)
    _directional(m, bcs, V, dict(reynolds=Re), w, lam, 3)


def test_directional_check_2d():
    """The same in 2-D.  The form has no derivative where two edges tie for the longest or Re_UGN sits on 3 (sns.h), and a
    finite difference across such a point checks nothing: the jitter seed is one for which no cell comes closer to either
    than four steps (seed 25 of the connected-mesh test has a cell whose two longest edges agree to 1e-6)."""
    m = _dfg_jittered(35)
    mask, g = M2.dfg2d_bcs(m).flatten()
    mask = mask.copy()
    mask[2::4] = 1
    g = g.copy()
    g[2::4] = 0.0
    w = _state_on((mask, g), m.num_nodes, 29, amp=0.3)
    lam = np.random.default_rng(30).standard_normal(m.num_dofs) * (mask == 0)
    x = m.points
    V = np.stack([np.sin(9.0 * x[:, 1]) * np.cos(3.0 * x[:, 0]), np.cos(4.0 * x[:, 0] + 7.0 * x[:, 1]), 0.0 * x[:, 0]], axis=1)
    ed = x[m.tris[:, [0, 0, 1]]] - x[m.tris[:, [1, 2, 2]]]
    ln = np.sort(np.sqrt((ed * ed).sum(axis=2)), axis=1)
    step = 2e-4 * ln.min() * 12.0          # relative change of an edge under the larger step: e |grad V|, |grad V| <= 9 + 3
    assert ((ln[:, 2] - ln[:, 1]) / ln[:, 2]).min() > 4.0 * step
    ph = np.array([[2 / 3, 1 / 6, 1 / 6], [1 / 6, 1 / 6, 2 / 3], [1 / 6, 2 / 3, 1 / 6]])
    uq = np.einsum("qa,eai->eqi", ph, w.reshape(-1, 4)[m.tris][:, :, :2])
    assert np.abs(np.linalg.norm(uq, axis=2) * ln[:, 2:3] / (2.0 * NU) / 3.0 - 1.0).min() > 4.0 * step
    _directional(m, (mask, g), V, dict(reynolds=1.0 / NU), w, lam, 2)


def test_explicit_part_of_the_reaction_force():
    """-gX(w, phi e_c) . V against central differences of functionals.reaction_force at fixed w on moved meshes."""
    m = M.duct_mesh((6, 3, 3), 2.0, jitter=0.2)
    bcs = B.duct_bcs(m).flatten()
    wall = m.meta["tags"]["wall"]
    w = _state_on(bcs, m.num_nodes, 31)
    x = m.points
    V = np.stack([np.sin(2.0 * x[:, 1]) * np.cos(x[:, 0]), np.cos(1.5 * x[:, 0] + x[:, 2]), np.sin(x[:, 0] * x[:, 1] + 0.3)], axis=1)
    phi = Fn.tag_node_weights(m, wall)
    P = FlowProblem(m, bcs, reynolds=RE_DUCT)
    h = 1.0 / 3.0
    for c in range(3):
        lam = np.zeros((m.num_nodes, 4))
        lam[:, c] = phi
        got = -float((P.residual_shape_gradient(_dev(w), _dev(lam.ravel())).cpu().numpy() * V).sum())

        def D_of(delta):
            F = []
            for s in (1.0, -1.0):
                Q = FlowProblem(_moved(m, m.points + s * delta * h * V), bcs, reynolds=RE_DUCT)
                F.append(Fn.reaction_force(Q, _dev(w), wall)[c])
                Q.close()
            return (F[0] - F[1]) / (2.0 * delta * h)

        Dstar, band = richardson_band(D_of, 2e-4)
        print(f"reaction force {c}: {got:.12e} D* {Dstar:.12e} band {band:.2e}; diff {abs(got - Dstar):.2e}")
        assert band <= 1e-6 * abs(Dstar) and abs(got - Dstar) <= band
    P.close()


# ---- 4. properties, 5. refusals ----------------------------------------------------------------------------------------------
def test_properties(meshes3d):
    m, bcs, Re = meshes3d["dense"]
    rng = np.random.default_rng(32)
    w = _dev(_state_on(bcs, m.num_nodes, 33))
    l1, l2 = _dev(rng.standard_normal(m.num_dofs)), _dev(rng.standard_normal(m.num_dofs))
    P = FlowProblem(m, bcs, reynolds=Re)
    P.jacobian(w, "ns")
    P.transpose_operator()
    vals0, F0, opt0 = P.bsr()[2].clone(), P.residual(w).clone(), bytes(P.options)
    g1 = P.residual_shape_gradient(w, l1)
    assert torch.equal(g1, P.residual_shape_gradient(w, l1))        # bitwise reproducible
    assert P.operator_transposed and torch.equal(vals0, P.bsr()[2]) and bytes(P.options) == opt0
    assert torch.equal(F0, P.residual(w))
    g2, g12 = P.residual_shape_gradient(w, l2), P.residual_shape_gradient(w, 2.0 * l1 - 0.5 * l2)
    scale = float(torch.abs(g1).max() + torch.abs(g2).max())
    assert float(torch.abs(g12 - (2.0 * g1 - 0.5 * g2)).max()) <= 1e-13 * scale       # linear in lam
    assert not torch.any(P.residual_shape_gradient(w, P.zeros()))
    s, a = torch.abs(g1.sum(dim=0)), torch.abs(g1).sum(dim=0)
    assert torch.all(s <= 1e-12 * a), (s / a)                        # translation invariance
    P.close()
    m2 = M2.dfg_2d_mesh(0.5)
    P2 = FlowProblem(m2, M2.dfg2d_bcs(m2).flatten(), reynolds=1.0 / NU)
    g = P2.residual_shape_gradient(_dev(0.3 * rng.standard_normal(m2.num_dofs)), _dev(rng.standard_normal(m2.num_dofs)))
    assert g.shape == (m2.num_nodes, 3) and not torch.any(g[:, 2])
    s, a = torch.abs(g.sum(dim=0))[:2], torch.abs(g).sum(dim=0)[:2]
    assert torch.all(s <= 1e-12 * a)
    P2.close()


def test_refusals(meshes3d):
    m, bcs, Re = meshes3d["dense"]
    P = FlowProblem(m, bcs, reynolds=Re)
    w, lam = P.zeros(), P.zeros()
    with pytest.raises(SnsError) as e:
        P.residual_shape_gradient(w, lam, form="stokes")
    assert e.value.code == -1
    out = torch.zeros(m.num_nodes, 3, dtype=torch.float64, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()
    for a in ((None, lam, out), (w, None, out), (w, lam, None)):
        assert P.lib.sns_residual_shape_gradient(P.h, 1, *map(ptr, a)) == -1
    assert P.lib.sns_residual_shape_gradient(None, 1, ptr(w), ptr(lam), ptr(out)) == -1
    assert P.lib.sns_residual_shape_gradient(P.h, 7, ptr(w), ptr(lam), ptr(out)) == -1
    P.close()
    from stabilized_navier_stokes_flow_fenicsx_amd import partition as PT
    part = PT.build_local_part(m, bcs[0], bcs[1], PT.rcb_partition(m.points, 2), 0, 2)
    R = FlowProblem(part.mesh, (part.bc_mask, part.bc_val), part=part, group="local-only", reynolds=Re)
    with pytest.raises(SnsError) as e:
        R.residual_shape_gradient(R.zeros(), R.zeros())
    assert e.value.code == -3
    R.close()


# ---- 7. / 8. end to end ----------------------------------------------------------------------------------------------------
def _smoothstep_down(s):
    s = np.clip(s, 0.0, 1.0)
    return 1.0 - s ** 3 * (10.0 - 15.0 * s + 6.0 * s * s)             # 1 -> 0, C^2


def _solve_on(mesh, bcs, w0, functional, **opt):
    Q = FlowProblem(mesh, bcs, **opt)
    w, res = Q.newton_solve(w0.clone())
    assert res.reason > 0, res
    out = np.asarray(functional(mesh, w.cpu().numpy()), dtype=np.float64)
    Q.close()
    return out


def _fd_of_solves(m, bcs, V, w, functional, delta, **opt):
    """Central differences of full Newton solves on X +- delta V and X +- delta V / 2, their Richardson value and the band of
    the existing Reynolds test: 4 |D(d/2) - D(d)| / 3 + 1e-7 |D*|."""
    D = []
    for d in (delta, 0.5 * delta):
        D.append((_solve_on(_moved(m, m.points + d * V), bcs, w, functional, **opt)
                  - _solve_on(_moved(m, m.points - d * V), bcs, w, functional, **opt)) / (2.0 * d))
    Dstar = (4.0 * D[1] - D[0]) / 3.0
    return D[0], D[1], Dstar, 4.0 * np.abs(D[1] - D[0]) / 3.0 + 1e-7 * np.abs(Dstar)


@pytest.fixture(scope="module")
def dfg2d_radius():
    """DFG 2D-1 at level 2 (the case of test_gpu_adjoint.py::dfg2d_level2), V = (x - c)/|x - c| psi(|x - c|): psi = 1 on the
    cylinder, falling C^2 to 0 at r = 0.12, inside the 0.15 gap to the walls.  dC/dr = dC/dX . V."""
    m = M2.dfg_2d_mesh(2.0)
    bcs = M2.dfg2d_bcs(m).flatten()
    opt = dict(reynolds=1.0 / NU, **TIGHT)
    P = FlowProblem(m, bcs, **opt)
    U, res = P.stokes_solve()
    assert res.reason > 0
    U.view(-1, 4)[:, 3] *= NU
    w, nres = P.newton_solve(U)
    assert nres.reason > 0
    r = m.points - np.array([0.2, 0.2])
    rn = np.linalg.norm(r, axis=1)
    V = r / rn[:, None] * _smoothstep_down((rn - 0.05) / 0.07)[:, None]
    fixed = np.unique(m.facets[m.facet_tags != M2.DFG2D_TAGS["obstacle"]])
    assert not np.any(V[fixed])                                      # walls, inlet and outlet do not move
    D1, D2, Dstar, band = _fd_of_solves(m, bcs, V, w, lambda mm, wh: M2.drag_lift_2d(mm, wh, NU), 1e-3, **opt)
    wh = w.cpu().numpy()
    G, E = M2.drag_lift_2d_gradient(m, NU), M2.drag_lift_2d_shape_gradient(m, wh, NU)
    out = []
    for k, name in enumerate(("C_d", "C_l")):
        dJ, lam, ares = shape_sensitivity(P, w, G[k], E[k])
        assert ares.reason > 0 and not P.operator_transposed
        adj = float((dJ.cpu().numpy()[:, :2] * V).sum())
        print(f"d{name}/dr: adjoint {adj:.10e}; D(d) {D1[k]:.10e} D(d/2) {D2[k]:.10e} D* {Dstar[k]:.10e} band {band[k]:.2e} = "
              f"{band[k] / abs(Dstar[k]):.2e} |D*|; |adjoint - D*| {abs(adj - Dstar[k]):.2e}; adjoint its {ares.its}")
        out.append((name, adj, Dstar[k], band[k]))
    P.close()
    return out


@pytest.mark.parametrize("k", [0, 1], ids=["C_d", "C_l"])
def test_dfg2d_radius_sensitivity_against_independent_solves(dfg2d_radius, k):
    """dC_d/dr and dC_l/dr (r = the cylinder radius) from ONE adjoint solve each against the Richardson value of central
    differences of full Newton solves on moved meshes, delta = 1e-3: |adjoint - D*| <= band and band <= 0.01 |D*|."""
    name, adj, Dstar, band = dfg2d_radius[k]
    assert band <= 1e-2 * abs(Dstar), (name, band, Dstar)
    assert abs(adj - Dstar) <= band, (name, adj, Dstar, band)


@pytest.fixture(scope="module")
def duct3d_squeeze():
    """The jittered duct of test_gpu_adjoint.py::duct3d, squeezed by V = b(x) (0, y, z), b a C^2 bump on x in [0.6, 1.4]:
    wall nodes move.  Functionals: the x-traction on the wall (explicit part: boundary_traction_shape_gradient) and the
    pressure difference between two points whose cells do not move (no explicit part)."""
    m = M.duct_mesh((24, 8, 8), 2.0, jitter=0.2)
    bcs = B.duct_bcs(m).flatten()
    opt = dict(reynolds=RE_DUCT, **TIGHT)
    P = FlowProblem(m, bcs, **opt)
    U, res = P.stokes_solve()
    assert res.reason > 0
    w, nres = P.newton_solve(U)
    assert nres.reason > 0
    wall, nu = m.meta["tags"]["wall"], 1.0 / RE_DUCT
    x = m.points
    s = (x[:, 0] - 1.0) / 0.4
    b = np.where(np.abs(s) < 1.0, (1.0 - s * s) ** 3, 0.0)
    V = b[:, None] * np.stack([0.0 * s, x[:, 1], x[:, 2]], axis=1)
    pa, pb = np.array([0.5, 0.03, -0.02]), np.array([1.5, 0.03, -0.02])
    from stabilized_navier_stokes_flow_fenicsx_amd.interpolate import locate_points
    cells, _ = locate_points(m, np.stack([pa, pb]), 1e-6)
    assert not np.any(V[m.tets[np.asarray(cells, dtype=np.int64)].ravel()])
    gp = Fn.pressure_difference_gradient(m, pa, pb)

    def functional(mm, wh):
        return np.array([Fn.boundary_traction_force(mm, wh, nu, wall)[0], gp @ wh])

    delta = 1e-2
    D1, D2, Dstar, band = _fd_of_solves(m, bcs, V, w, functional, delta, **opt)
    wh = w.cpu().numpy()
    G = np.stack([Fn.boundary_traction_gradient(m, nu, wall)[0], gp])
    E = [Fn.boundary_traction_shape_gradient(m, wh, nu, wall)[0], None]
    # dF/dX . V by differences of the GPU residual on the moved meshes (the state satisfies the same Dirichlet data there)
    Fpm = []
    for sg in (1.0, -1.0):
        Q = FlowProblem(_moved(m, m.points + sg * 0.5 * delta * V), bcs, **opt)
        Fpm.append(Q.residual(w).clone())
        Q.close()
    dFV = (Fpm[0] - Fpm[1]) / delta
    out = []
    for k, name in enumerate(("F_wall", "dp")):
        dJ, lam, ares = shape_sensitivity(P, w, G[k], E[k])
        assert ares.reason > 0 and not P.operator_transposed
        explicit = 0.0 if E[k] is None else float((E[k] * V).sum())
        adj = float((dJ.cpu().numpy() * V).sum())
        # tangent-linear identity with the same Jacobian: A dw = -dF/dX.V, grad_J . dw = -lam . dF/dX.V
        dw, rf = P.krylov_solve(-dFV)
        assert rf.reason > 0
        gd = _dev(G[k])
        nrm = lambda t: float(torch.linalg.norm(t))
        tan, adj_fd = float(torch.dot(gd, dw)), -float(torch.dot(lam, dFV))
        tb = nrm(lam) * rf.rnorm + nrm(dw) * ares.rnorm + 1e-13 * (nrm(lam) * nrm(dFV) + nrm(gd) * nrm(dw))
        print(f"d{name}/dV: adjoint {adj:.10e} (explicit {explicit:.3e}); tangent {tan:.10e} vs -lam.dFV {adj_fd:.10e} (|diff| "
              f"{abs(tan - adj_fd):.2e} <= {tb:.2e}); D(d) {D1[k]:.10e} D(d/2) {D2[k]:.10e} D* {Dstar[k]:.10e} band {band[k]:.2e} = "
              f"{band[k] / abs(Dstar[k]):.2e} |D*|; |adjoint - D*| {abs(adj - Dstar[k]):.2e}")
        out.append((name, adj, Dstar[k], band[k], tan, adj_fd, tb))
    P.close()
    return out


@pytest.mark.parametrize("k", [0, 1], ids=["F_wall", "dp"])
def test_duct3d_squeeze_sensitivity_against_independent_solves(duct3d_squeeze, k):
    """Acceptance as in 2-D; and the tangent-linear identity grad_J . dw = -lam . (dF/dX . V) with A dw = -(dF/dX . V) from
    directional differences of the residual, within the two solves' residual norms: it tells a wrong adjoint from a wrong
    kernel."""
    name, adj, Dstar, band, tan, adj_fd, tb = duct3d_squeeze[k]
    assert abs(tan - adj_fd) <= tb, (name, tan, adj_fd, tb)
    assert band <= 1e-2 * abs(Dstar), (name, band, Dstar)
    assert abs(adj - Dstar) <= band, (name, adj, Dstar, band)
