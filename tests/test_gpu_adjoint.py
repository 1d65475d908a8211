"""Adjoint solves on the GPU: the in-place BSR transpose (sns_transpose_operator, csrc/sns_transpose.hip), sns_adjoint_solve
and solver.reynolds_sensitivity.

The transpose is pure data movement, so it is compared bit for bit with scipy's transpose of the exported operator; the
adjoint solve is checked on the identity lam . b - g . x = lam . r_f - r_a . x between a forward and an adjoint solve, whose
right-hand side the two solves report themselves; the sensitivities are checked against Richardson-extrapolated central
differences of full Newton solves, with the band taken from the finite difference's own consistency."""
import numpy as np
import pytest
import torch

from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B
from stabilized_navier_stokes_flow_fenicsx_amd import functionals as Fn
from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
from stabilized_navier_stokes_flow_fenicsx_amd import mesh2d as M2
from stabilized_navier_stokes_flow_fenicsx_amd.solver import (FlowProblem, SnsError, reynolds_sensitivity,
                                                              residual_reynolds_derivative)

pytestmark = pytest.mark.gpu
NU = 1e-3                                            # DFG_2D_Validation.py:148
RE_DUCT = 25.0
TIGHT = dict(ksp_rtol=1e-12, snes_rtol=1e-12, snes_atol=1e-12, snes_stol=1e-12)


def _structured():
    m = M.duct_mesh((40, 10, 10), 2.0)                # 4961 nodes: fine level, an aggregate-block level, the dense level
    return m, B.duct_bcs(m).flatten(), dict(reynolds=RE_DUCT)


def _delaunay():
    m = M.delaunay_duct_mesh(13)                      # 1 - 38 tets per node: irregular rows
    return m, B.duct_bcs(m).flatten(), dict(reynolds=RE_DUCT)


def _dfg2d():
    m = M2.dfg_2d_mesh(0.5)
    return m, M2.dfg2d_bcs(m).flatten(), dict(reynolds=1.0 / NU)


CASES = {"structured": _structured, "delaunay": _delaunay, "dfg2d": _dfg2d}


def _jacobian_at_stokes(case, **kw):
    m, bcs, opt = CASES[case]()
    P = FlowProblem(m, bcs, **opt, **kw)
    U, res = P.stokes_solve()
    assert res.reason > 0
    if case == "dfg2d":
        U.view(-1, 4)[:, 3] *= NU                     # (the unit-viscosity Stokes pressure, rescaled as the driver's fallback does)
    P.jacobian(U, "ns")
    return P, U


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _sorted_csr(A):
    A = A.tocsr()
    A.sort_indices()
    return A


@pytest.mark.parametrize("case", ["structured", "delaunay", "dfg2d"])
def test_transpose_is_exact(case):
    P, U = _jacobian_at_stokes(case)
    assert not P.operator_transposed
    rp0, ci0, va0 = (t.cpu().numpy() for t in P.bsr())
    A = P.to_scipy()
    assert abs(A - A.T).max() > 1e-3 * abs(A).max()                 # the convective blocks make it non-symmetric
    P.transpose_operator()
    assert P.operator_transposed
    rp1, ci1, va1 = (t.cpu().numpy() for t in P.bsr())
    assert np.array_equal(rp0, rp1) and np.array_equal(ci0, ci1)
    # scipy's transpose of the un-flipped export, entry by entry in CSR order (explicit zeros of the blocks are kept)
    At, Bt = _sorted_csr(A.T), _sorted_csr(P.to_scipy())
    assert np.array_equal(At.indptr, Bt.indptr) and np.array_equal(At.indices, Bt.indices)
    assert np.array_equal(_bits(At.data), _bits(Bt.data))
    # ... and slot by slot: block (i, j) of A^T is the transposed block of slot (j, i)
    n = len(rp0) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp0))
    key = rows * n + ci0                                              # ascending: sorted rows of sorted columns
    partner = np.searchsorted(key, ci0.astype(np.int64) * n + rows)
    assert np.array_equal(key[partner], ci0.astype(np.int64) * n + rows)
    assert np.array_equal(_bits(va1), _bits(va0[partner].transpose(0, 2, 1)))
    # a second call restores the bits
    P.transpose_operator()
    assert not P.operator_transposed
    assert np.array_equal(_bits(P.bsr()[2].cpu().numpy()), _bits(va0))
    # an assembly after a flip clears the flag and gives the original bits
    P.transpose_operator()
    P.jacobian(U, "ns")
    assert not P.operator_transposed
    assert np.array_equal(_bits(P.bsr()[2].cpu().numpy()), _bits(va0))
    P.close()


# every route of the assembly driver that writes the matrix (csrc/sns_assemble.hip, DESIGN.md "Assembly routes"):
# (2-D?, options, form, perturbed form variant?)
MATRIX_ROUTES = {"fused_ns": (False, {}, "ns", False),
                 "staged_ns": (False, {"assembly_fused": 0}, "ns", False),
                 "variant_ns": (False, {"assembly_fused": 1}, "ns", True),
                 "fused_stokes": (False, {}, "stokes", False),
                 "staged_stokes": (False, {"assembly_fused": 0}, "stokes", False),
                 "ns_2d": (True, {}, "ns", False),
                 "stokes_2d": (True, {}, "stokes", False)}


@pytest.mark.parametrize("route", list(MATRIX_ROUTES))
def test_every_matrix_route_resets_the_matrix_state(route):
    """The state change of a matrix-writing assembly is written once for all routes: after pc_setup and a flip, an assembly by
    any of them clears the transposed flag, invalidates the preconditioner and gives the bits of the first assembly."""
    two_d, opts, form, variant = MATRIX_ROUTES[route]
    if two_d:
        m, bcs, opt = _dfg2d()
    else:
        m = M.channel_mesh((5, 3, 3), jitter=0.2)
        # a partial last workgroup in every kernel: 16 cells per workgroup of the element pass, 256 dofs of the node passes
        assert len(m.tets) % 16 != 0 and (4 * len(m.points)) % 256 != 0
        bcs, opt = B.channel_bcs(m, *B.two_stream_profiles(0.5)).flatten(), dict(reynolds=RE_DUCT)
    P = FlowProblem(m, bcs, **opt, **opts)
    w = None
    if form == "ns":
        w, res = P.stokes_solve()
        assert res.reason > 0
    if variant:
        P.set_form_variant(c_inverse=30.0)
    P.jacobian(w, form)
    va0 = P.bsr()[2].cpu().numpy().copy()
    P.pc_setup()
    P.pc_apply(P.zeros())
    P.transpose_operator()
    assert P.operator_transposed
    P.jacobian(w, form)
    assert not P.operator_transposed
    with pytest.raises(SnsError) as e:
        P.pc_apply(P.zeros())
    assert e.value.code == -3 and "pc_apply before pc_setup" in str(e.value)
    assert np.array_equal(_bits(P.bsr()[2].cpu().numpy()), _bits(va0))
    P.close()


def test_transpose_needs_a_matrix_and_a_single_gpu_handle():
    m, bcs, opt = _structured()
    P = FlowProblem(m, bcs, **opt)
    with pytest.raises(SnsError) as e:
        P.transpose_operator()
    assert e.value.code == -3                                        # SNS_E_STATE: nothing assembled
    with pytest.raises(SnsError):
        P.adjoint_solve(P.zeros())
    assert not P.operator_transposed
    P.close()
    # a handle with an owned / ghost split attached (no transport needed): out of scope, SNS_E_STATE
    from stabilized_navier_stokes_flow_fenicsx_amd import partition as PT
    mask, g = bcs
    owner = PT.rcb_partition(m.points, 2)
    part = PT.build_local_part(m, mask, g, owner, 0, 2)
    Q = FlowProblem(part.mesh, (part.bc_mask, part.bc_val), part=part, group="local-only", **opt)
    Q.jacobian(Q.zeros(), "ns")
    with pytest.raises(SnsError) as e:
        Q.transpose_operator()
    assert e.value.code == -3 and not Q.operator_transposed
    Q.close()


@pytest.mark.parametrize("case", ["structured", "delaunay", "dfg2d"])
def test_products_with_the_flipped_operator(case):
    P, U = _jacobian_at_stokes(case)
    A = P.to_scipy()
    x = np.random.default_rng(7).normal(size=A.shape[0])
    xd = torch.from_numpy(x).cuda()
    ref = A @ x
    e_fwd = np.linalg.norm(P.spmv(xd).cpu().numpy() - ref) / np.linalg.norm(ref)
    P.transpose_operator()
    ref_t = A.T @ x
    e_adj = np.linalg.norm(P.spmv(xd).cpu().numpy() - ref_t) / np.linalg.norm(ref_t)
    print(f"{case}: spmv relative difference to scipy: A x {e_fwd:.3e}, A^T x {e_adj:.3e}")
    # same kernel, same row lengths; the factor covers a different summation pairing
    assert e_adj <= 2.0 * e_fwd
    P.close()


def _adjoint_identity(P, A, b, g, tag):
    """Forward solve, adjoint solve, the identity between them and the state of the handle afterwards."""
    bd, gd = torch.from_numpy(b).cuda(), torch.from_numpy(g).cuda()
    x, rf = P.krylov_solve(bd)
    lam, ra = P.adjoint_solve(gd)
    assert not P.operator_transposed
    assert rf.reason > 0 and ra.reason > 0, (tag, rf, ra)
    xh, lh = x.cpu().numpy(), lam.cpu().numpy()
    nrm = np.linalg.norm
    lhs = abs(lh @ b - g @ xh)
    bound = nrm(lh) * rf.rnorm + nrm(xh) * ra.rnorm + 1e-13 * (nrm(lh) * nrm(b) + nrm(g) * nrm(xh))
    print(f"{tag}: its {rf.its} / {ra.its}, |lam.b - g.x| {lhs:.3e} <= {bound:.3e}; r_f {rf.rnorm:.3e} r_a {ra.rnorm:.3e}")
    assert lhs <= bound, (tag, lhs, bound)
    # the adjoint solve's own residual, against scipy's transpose of the exported operator
    assert nrm(g - A.T @ lh) <= ra.rnorm * (1.0 + 1e-6) + 1e-13 * (abs(A).max() * nrm(lh) + nrm(g))
    # lam_B = g_B on the Dirichlet dofs (unit rows and columns)
    Bm = P.bc_mask.astype(bool)
    assert np.abs(lh[Bm] - g[Bm]).max() <= 1e-14 * max(1.0, np.abs(g).max())
    # the handle holds A again: the next forward solve converges and reproduces x to the Krylov tolerance -- both
    # solve A x = b, so A (x2 - x) = r_f - r_f2 with the residual norms the solves report
    x2, rf2 = P.krylov_solve(bd)
    assert rf2.reason > 0
    d = nrm(A @ (x2.cpu().numpy() - xh))
    assert d <= rf.rnorm + rf2.rnorm + 1e-13 * abs(A).max() * nrm(xh), (tag, d, rf.rnorm, rf2.rnorm)


@pytest.mark.parametrize("opts", [{}, {"amg_f32_matrix": 0}], ids=["default", "fp64_matrix"])
@pytest.mark.parametrize("case", ["structured", "delaunay"])
def test_adjoint_identity(case, opts):
    P, U = _jacobian_at_stokes(case, **opts)
    A = P.to_scipy()
    rng = np.random.default_rng(21)
    free = P.bc_mask == 0
    for vanish in (True, True, False):
        b, g = rng.normal(size=P.ndof), rng.normal(size=P.ndof)
        if vanish:
            b, g = b * free, g * free
        _adjoint_identity(P, A, b, g, f"{case} {opts} vanish={vanish}")
    P.close()


def test_an_unconverged_adjoint_solve_gives_the_operator_back():
    """One BiCGStab iteration against a tolerance it cannot meet: sns_adjoint_solve returns without an error, and the handle
    holds A again bit for bit with its hierarchy marked stale, as after a solve that converged."""
    m = M.duct_mesh((6, 3, 3), 2.0)
    P = FlowProblem(m, B.duct_bcs(m).flatten(), reynolds=RE_DUCT)
    U, res = P.stokes_solve()
    assert res.reason > 0
    P.set_options(ksp_rtol=1e-14, ksp_max_it=1)
    P.jacobian(U, "ns")
    va0 = P.bsr()[2].cpu().numpy().copy()
    g = torch.from_numpy(np.random.default_rng(5).normal(size=P.ndof)).cuda()
    lam, ra = P.adjoint_solve(g)                                      # returns SNS_OK: no exception
    print("reason", ra.reason, "its", ra.its, "rnorm", ra.rnorm)
    assert ra.reason <= 0
    assert not P.operator_transposed
    assert np.array_equal(_bits(P.bsr()[2].cpu().numpy()), _bits(va0))
    with pytest.raises(SnsError) as e:
        P.pc_apply(P.zeros())
    assert e.value.code == -3 and "pc_apply before pc_setup" in str(e.value)
    P.close()


# ---- sensitivities -------------------------------------------------------------------------------------------------------
def _fd_band(J_of_re, Re, delta):
    """Central differences D(delta), D(delta / 2) of J over Re (1 +- delta), their Richardson value and the band the
    adjoint value must meet: 4 |D(delta/2) - D(delta)| / 3 plus 1e-7 |D*| for the rel_step difference of the residual."""
    D = []
    for d in (delta, 0.5 * delta):
        D.append((J_of_re(Re * (1.0 + d)) - J_of_re(Re * (1.0 - d))) / (2.0 * Re * d))
    D = np.array(D)
    Dstar = (4.0 * D[1] - D[0]) / 3.0
    return D[0], D[1], Dstar, 4.0 * np.abs(D[1] - D[0]) / 3.0 + 1e-7 * np.abs(Dstar)


def _check_sensitivities(P, w, Re, names, functional, grads_at, delta=1e-2):
    """functional(w_host, nu) -> array of the functionals; grads_at(nu) -> their gradients (k, ndof)."""

    def J_of_re(re):
        P.set_options(reynolds=re)
        wr, res = P.newton_solve(w.clone())
        assert res.reason > 0, (re, res)
        return np.asarray(functional(wr.cpu().numpy(), 1.0 / re), dtype=np.float64)

    try:
        D1, D2, Dstar, band = _fd_band(J_of_re, Re, delta)
    finally:
        P.set_options(reynolds=Re)
    G, G1, G0 = grads_at(1.0 / Re), grads_at(1.0), grads_at(0.0)
    wh = w.cpu().numpy()
    out = []
    for k, name in enumerate(names):
        explicit = -float((G1[k] - G0[k]) @ wh) / Re ** 2
        adj, lam, res = reynolds_sensitivity(P, w, G[k], dJ_dRe_explicit=explicit)
        assert res.reason > 0 and not P.operator_transposed
        assert abs(P.options.reynolds - Re) == 0.0
        # tangent-linear value with the same Jacobian: A dw = -dF/dRe by the forward solve
        dF = residual_reynolds_derivative(P, w)
        dw, rf = P.krylov_solve(-dF)
        assert rf.reason > 0
        gd = torch.from_numpy(np.ascontiguousarray(G[k])).cuda()
        tan = explicit + float(torch.dot(gd, dw))
        nrm = lambda t: float(torch.linalg.norm(t))
        tb = nrm(lam) * rf.rnorm + nrm(dw) * res.rnorm + 1e-13 * (nrm(lam) * nrm(dF) + nrm(gd) * nrm(dw))
        print(f"d{name}/dRe: adjoint {adj:.10e} tangent {tan:.10e} (|diff| {abs(adj - tan):.2e} <= {tb:.2e}); "
              f"D(d) {D1[k]:.10e} D(d/2) {D2[k]:.10e} D* {Dstar[k]:.10e} band {band[k]:.2e} = {band[k] / abs(Dstar[k]):.2e} |D*|; "
              f"|adjoint - D*| {abs(adj - Dstar[k]):.2e}; adjoint its {res.its}")
        out.append((name, adj, tan, tb, Dstar[k], band[k]))
    return out


@pytest.fixture(scope="module")
def dfg2d_level2():
    m = M2.dfg_2d_mesh(2.0)
    P = FlowProblem(m, M2.dfg2d_bcs(m).flatten(), reynolds=1.0 / NU, **TIGHT)
    U, res = P.stokes_solve()
    assert res.reason > 0
    U.view(-1, 4)[:, 3] *= NU
    w, nres = P.newton_solve(U)
    assert nres.reason > 0
    out = _check_sensitivities(P, w, 1.0 / NU, ("C_d", "C_l"), lambda wh, nu: M2.drag_lift_2d(m, wh, nu),
                               lambda nu: M2.drag_lift_2d_gradient(m, nu))
    P.close()
    return out


@pytest.fixture(scope="module")
def duct3d():
    """The 3-D case: a jittered duct at Re 25 with the wall drag (x component of the traction on the no-slip wall) and the
    pressure difference between two points on the axis.  (The pillar channel's coarse meshes do not converge without
    continuation at the driver's Reynolds number and its fine ones take five Newton solves of 2 M tets each.)"""
    m = M.duct_mesh((24, 8, 8), 2.0, jitter=0.2)
    P = FlowProblem(m, B.duct_bcs(m).flatten(), reynolds=RE_DUCT, **TIGHT)
    U, res = P.stokes_solve()
    assert res.reason > 0
    w, nres = P.newton_solve(U)
    assert nres.reason > 0
    wall = m.meta["tags"]["wall"]
    pa, pb = np.array([0.5, 0.03, -0.02]), np.array([1.5, 0.03, -0.02])
    gp = Fn.pressure_difference_gradient(m, pa, pb)
    pe = P.eval_at(w, np.stack([pa, pb]))[:, 3]                       # (the device's point evaluation: the same weights)
    assert abs(gp @ w.cpu().numpy() - (pe[0] - pe[1])) <= 1e-12 * np.abs(w.cpu().numpy()[3::4]).max()

    def functional(wh, nu):
        return np.array([Fn.boundary_traction_force(m, wh, nu, wall)[0], gp @ wh])

    def grads_at(nu):
        return np.stack([Fn.boundary_traction_gradient(m, nu, wall)[0], gp])

    out = _check_sensitivities(P, w, RE_DUCT, ("F_wall", "dp"), functional, grads_at)
    P.close()
    return out


@pytest.mark.parametrize("k", [0, 1], ids=["C_d", "C_l"])
def test_dfg2d_sensitivity_against_independent_solves(dfg2d_level2, k):
    """dC_d/dRe and dC_l/dRe of DFG 2D-1 (level 2, Re as the driver sets it) from ONE adjoint solve each against the
    Richardson value D* = (4 D(d/2) - D(d)) / 3 of central differences of full Newton solves, d = 1e-2, each started from
    w: |adjoint - D*| <= 4 |D(d/2) - D(d)| / 3 + 1e-7 |D*|.  A band wider than 1 % of |D*| would check nothing."""
    name, adj, tan, tb, Dstar, band = dfg2d_level2[k]
    assert band <= 0.01 * abs(Dstar), (name, band, Dstar)
    assert abs(adj - Dstar) <= band, (name, adj, Dstar, band)


@pytest.mark.parametrize("k", [0, 1], ids=["wall_drag", "pressure_drop"])
def test_duct3d_sensitivity_against_independent_solves(duct3d, k):
    name, adj, tan, tb, Dstar, band = duct3d[k]
    assert band <= 0.01 * abs(Dstar), (name, band, Dstar)
    assert abs(adj - Dstar) <= band, (name, adj, Dstar, band)


def test_tangent_linear_value_agrees_with_the_adjoint(dfg2d_level2, duct3d):
    """grad_J . dw with A dw = -dF/dRe (the existing forward solve) against -lam . dF/dRe: the two differ by
    lam . r_f - r_a . dw, bounded with the residual norms the solves return.  Separates "the adjoint solve is wrong" from
    "dF/dRe is wrong" when the comparison with the finite differences fails."""
    for name, adj, tan, tb, Dstar, band in list(dfg2d_level2) + list(duct3d):
        assert abs(adj - tan) <= tb, (name, adj, tan, tb)
