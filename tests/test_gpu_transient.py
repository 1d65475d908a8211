"""Implicit time stepping of the 3-D NS form on the GPU (sns_set_time_term, sns_time_step; solver.solve_unsteady,
solver.pseudo_transient_solve), everything through the C-ABI.

The reference has no unsteady form; the yardstick is the test-side oracle tests/ns3d_oracle.py (literal restatement,
autograd Jacobian, BDF stepper with a sparse LU) whose own checks are tests/test_host_transient.py.  Tolerances as in
tests/test_gpu_parity.py: operators 1e-12 relative, the two assembly paths against each other 1e-13, Krylov-converged
fields 1e-6, J dw against central differences of the residual 1e-6."""
import numpy as np
import pytest
import torch

import ns3d_oracle as NS
from conftest import rel
from oracle import forms_literal as FL
from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B
from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
from stabilized_navier_stokes_flow_fenicsx_amd import mesh2d as M2
from stabilized_navier_stokes_flow_fenicsx_amd import solver as S
from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem, SnsError
from test_gpu_adjoint import _adjoint_identity
from test_host_transient import CASE, FIXTURE, _random_tets, observed_orders, stepping_problem

pytestmark = pytest.mark.gpu
TIGHT = dict(ksp_rtol=1e-11, snes_rtol=1e-10, snes_atol=1e-14, snes_stol=1e-14)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _one_tet(X):
    return M.TetMesh(np.ascontiguousarray(X), np.array([[0, 1, 2, 3]], np.int32), np.zeros((0, 3), np.int32), np.zeros(0, np.int32))


def _hist(rng, n_nodes):
    d = rng.normal(size=(n_nodes, 4))
    return d.ravel()                                    # (the pressure slots hold noise on purpose: they must be ignored)


# ---- 1. element level ------------------------------------------------------------------------------------------------
SIGMA_THETA = [(1.0, 0.0), (25.0, 2500.0), (1e4, 4e8), (0.0, 50.0), (300.0, 0.0)]       # sigma h / |u| >> 1 and theta = 0 among them


@pytest.mark.parametrize("corrected", [0, 1])
def test_element_matrices_against_the_oracle(corrected):
    rng = np.random.default_rng(31)
    X = np.concatenate([_random_tets(rng, 4), _random_tets(rng, 3, sliver=True)])
    none = (np.zeros(16, np.uint8), np.zeros(16))
    for i in range(len(X)):
        W, d, Re = rng.normal(size=16), _hist(rng, 4), float(rng.uniform(5.0, 200.0))
        D = d.reshape(4, 4)[None, :, :3]
        for fused in (0, 1):
            P = FlowProblem(_one_tet(X[i]), none, reynolds=Re, corrected_convection=corrected, pc_type="bjacobi", assembly_fused=fused)
            for sigma, theta in SIGMA_THETA:
                Fo, Jo = NS.element(X[i][None], W[None], Re, d=D, sigma=sigma, theta=theta, corrected_convection=bool(corrected))
                P.set_time_term(sigma, theta, d)
                F = P.zeros()
                P.jacobian(_dev(W), "ns", residual_out=F)
                tag = (i, fused, sigma, theta)
                if not fused:                                        # the staged kernel's own output
                    Ke = P.element_matrices().cpu().numpy()[0]
                    assert rel(Ke.transpose(0, 2, 1, 3).reshape(16, 16), Jo[0]) < 1e-12, tag
                assert rel(P.to_scipy().toarray(), Jo[0]) < 1e-12, tag
                assert rel(F.cpu().numpy(), Fo[0]) < 1e-12, tag
                assert rel(P.residual(_dev(W), "ns").cpu().numpy(), Fo[0]) < 1e-12, tag      # one lane per tet
            P.close()


@pytest.mark.parametrize("corrected", [0, 1])
def test_perturbed_form_variant_with_a_time_term(corrected):
    rng = np.random.default_rng(32)
    X = _random_tets(rng, 2)
    none = (np.zeros(16, np.uint8), np.zeros(16))
    base = dict(FL.VARIANT)
    try:
        FL.VARIANT.update(ci=144.0, lsic=4.0, pspg=-1.0, one_point=True)
        for i in range(2):
            W, d = rng.normal(size=16), _hist(rng, 4)
            Fo, Jo = NS.element(X[i][None], W[None], 40.0, d=d.reshape(4, 4)[None, :, :3], sigma=12.0, theta=90.0, corrected_convection=bool(corrected))
            P = FlowProblem(_one_tet(X[i]), none, reynolds=40.0, corrected_convection=corrected, pc_type="bjacobi")
            P.set_form_variant(c_inverse=144.0, lsic_scale=4.0, pspg_sign=-1.0, one_point_quadrature=True)
            P.set_time_term(12.0, 90.0, d)
            F = P.zeros()
            P.jacobian(_dev(W), "ns", residual_out=F)
            assert rel(P.to_scipy().toarray(), Jo[0]) < 1e-12 and rel(F.cpu().numpy(), Fo[0]) < 1e-12
            assert rel(P.residual(_dev(W), "ns").cpu().numpy(), Fo[0]) < 1e-12
            P.close()
    finally:
        FL.VARIANT.update(base)


# ---- 2. global level -------------------------------------------------------------------------------------------------
def _channel():
    m = M.channel_mesh((9, 5, 4), jitter=0.2)
    mask, g = B.channel_bcs(m, *B.two_stream_profiles(0.4)).flatten()
    return m, mask, g


@pytest.mark.parametrize("corrected", [0, 1])
def test_fused_staged_and_oracle_agree_globally(corrected):
    rng = np.random.default_rng(33)
    m, mask, g = _channel()
    m.tets = np.ascontiguousarray(np.take_along_axis(m.tets, np.argsort(rng.random(m.tets.shape), axis=1), axis=1))
    Bm = mask.astype(bool)
    w = rng.normal(size=m.num_dofs) * 0.5
    w[Bm] = g[Bm]
    w2 = w.copy()
    w2[np.nonzero(Bm)[0][::3]] += 0.3                              # violates the Dirichlet data: lifting
    d = _hist(rng, m.num_nodes)
    Re, sigma, theta = 17.0, 20.0, 1600.0
    kw = dict(corrected_convection=bool(corrected))
    P = FlowProblem(m, (mask, g), reynolds=Re, corrected_convection=corrected)
    P.set_time_term(sigma, theta, d)
    for state in (w, w2):
        Jo, Fo = NS.assemble(m.points, m.tets, state, Re, mask, g, d=d, sigma=sigma, theta=theta, **kw)
        got = []
        for fused in (1, 0):
            P.set_options(assembly_fused=fused)
            F = P.zeros()
            P.jacobian(_dev(state), "ns", residual_out=F)
            got.append((P.to_scipy(), F.cpu().numpy()))
            assert abs(got[-1][0] - Jo).max() < 1e-12 * abs(Jo).max(), fused
            assert rel(got[-1][1], Fo) < 1e-12, fused
            assert rel(P.residual(_dev(state), "ns").cpu().numpy(), Fo) < 1e-12, fused
        assert abs(got[0][0] - got[1][0]).max() < 1e-13 * abs(got[1][0]).max()
        assert rel(got[0][1], got[1][1]) < 1e-13
    P.close()


# ---- 3. no-op --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
def test_cleared_time_term_is_bitwise_the_steady_handle(fused):
    rng = np.random.default_rng(34)
    m, mask, g = _channel()
    w = rng.normal(size=m.num_dofs) * 0.5
    w[mask.astype(bool)] = g[mask.astype(bool)]
    wd = _dev(w)

    def system(P):
        F = P.zeros()
        P.jacobian(wd, "ns", residual_out=F)
        return P.bsr()[2].clone(), F.clone(), P.residual(wd, "ns")

    P0 = FlowProblem(m, (mask, g), reynolds=30.0, assembly_fused=fused)
    v0, F0, R0 = system(P0)
    P0.close()
    P1 = FlowProblem(m, (mask, g), reynolds=30.0, assembly_fused=fused)
    P1.clear_time_term()                                           # set_time_term(0, 0, NULL) on a fresh handle
    v1, F1, R1 = system(P1)
    assert torch.equal(v0, v1) and torch.equal(F0, F1) and torch.equal(R0, R1)
    P1.set_time_term(5.0, 3.0, _hist(rng, m.num_nodes))
    v2, F2, _ = system(P1)
    assert not torch.equal(v0, v2) and not torch.equal(F0, F2)     # (the term does something)
    P1.clear_time_term()
    v3, F3, R3 = system(P1)
    assert torch.equal(v0, v3) and torch.equal(F0, F3) and torch.equal(R0, R3)
    P1.close()


# ---- 4. Jacobian against central differences ------------------------------------------------------------------------
@pytest.mark.parametrize("corrected", [0, 1])
def test_jacobian_against_central_differences_of_the_residual(corrected):
    m = M.duct_mesh((30, 24, 24), 4.0)                             # 103 680 tets
    mask, g = B.duct_bcs(m).flatten()
    P = FlowProblem(m, (mask, g), reynolds=80.0, corrected_convection=corrected)
    U, res = P.stokes_solve()
    assert res.reason > 0
    gen = torch.Generator(device="cuda").manual_seed(35)
    d = torch.randn(P.ndof, dtype=torch.float64, device="cuda", generator=gen)
    P.set_time_term(50.0, 1e4, d)
    free = torch.from_numpy(1.0 - P.bc_mask.astype(np.float64)).cuda()
    eps = 1e-4
    for k in range(3):
        dw = torch.randn(P.ndof, dtype=torch.float64, device="cuda", generator=gen) * free * 1e-2
        fd = (P.residual(U + eps * dw, "ns") - P.residual(U - eps * dw, "ns")) / (2 * eps)
        for fused in (1, 0):
            P.set_options(assembly_fused=fused)
            P.jacobian(U, "ns")
            e = float((P.spmv(dw) - fd).norm() / fd.norm())
            print(f"corrected {corrected} direction {k} fused {fused}: |J dw - fd| / |fd| = {e:.3e}")
            assert e < 1e-6
    P.close()


# ---- 5. stepping ------------------------------------------------------------------------------------------------------
def _fields_close(a, b, tol=1e-6):
    a, b = np.asarray(a).reshape(-1, 4), np.asarray(b).reshape(-1, 4)
    return rel(a[:, :3], b[:, :3]) < tol and rel(a[:, 3], b[:, 3]) < tol


@pytest.mark.parametrize("order", [1, 2])
def test_steps_against_the_oracle_stepper(order):
    fx = np.load(FIXTURE)
    m, mask, g, _ = stepping_problem()
    for tc in (0.0, 4.0):
        want = fx[f"steps_bdf{order}_tc{int(tc)}"]
        P = FlowProblem(m, (mask, g), reynolds=CASE["Re"], **TIGHT)
        w, wprev = _dev(want[0]), _dev(want[0])
        for n in range(1, len(want)):
            _, res = P.time_step(w, wprev, 0.05, order=1 if n == 1 else order, theta_coeff=tc)
            assert res.reason > 0, (n, res)
            e = (rel(w.cpu().numpy().reshape(-1, 4)[:, :3], want[n].reshape(-1, 4)[:, :3]),
                 rel(w.cpu().numpy().reshape(-1, 4)[:, 3], want[n].reshape(-1, 4)[:, 3]))
            print(f"BDF{order} theta_coeff {tc} step {n}: its {res.its} ksp {res.ksp_its}  rel err u {e[0]:.2e} p {e[1]:.2e}")
            assert _fields_close(w.cpu().numpy(), want[n]), (n, e)
            assert _fields_close(wprev.cpu().numpy(), want[n - 1], 1e-6)
        P.close()


@pytest.mark.parametrize("order", [1, 2])
def test_fixture_fields_at_T_and_the_observed_order(order):
    fx = np.load(FIXTURE)
    m, mask, g, _ = stepping_problem()
    fields = {16: fx[f"bdf{order}_x16"]}
    for k in (1, 2, 4):
        n = k * CASE["n0"]
        P = FlowProblem(m, (mask, g), reynolds=CASE["Re"], **TIGHT)
        w, recs = S.solve_unsteady(P, _dev(fx["w0"]), CASE["T"] / n, n, order=order, theta_coeff=0.0)
        assert len(recs) == n and all(r["reason"] > 0 for r in recs), recs
        fields[k] = w.cpu().numpy()
        assert _fields_close(fields[k], fx[f"bdf{order}_x{k}"]), k
        P.close()
    e, (p1, p2) = observed_orders(fields)
    print(f"BDF{order} on the GPU: errors {e}, observed orders {p1:.3f} {p2:.3f}")
    if order == 1:
        assert 0.7 < p1 < 1.3 and 0.7 < p2 < 1.3
    else:
        assert p1 > 1.5 and p2 > 1.5


# ---- 6. steady limit ---------------------------------------------------------------------------------------------------
def test_steady_limit_of_pseudo_transient_and_of_a_step():
    m, mask, g, _ = stepping_problem()
    P = FlowProblem(m, (mask, g), reynolds=CASE["Re"], ksp_rtol=1e-11, snes_rtol=1e-10)
    U, res = P.stokes_solve()
    f_stokes = float(P.residual(U, "ns").norm())
    ws, res = P.newton_solve(U.clone())
    assert res.reason > 0
    wp, rp = S.pseudo_transient_solve(P, P.zeros(), 0.5)
    print(f"pseudo-transient: {rp.ptc_steps} pseudo-steps, closing Newton {rp.its} its, reason {rp.reason}")
    assert rp.reason > 0 and rp.ptc_steps >= 1
    assert _fields_close(wp.cpu().numpy(), ws.cpu().numpy())
    # the helper leaves the steady handle behind
    f_steady = float(P.residual(ws, "ns").norm())
    # one BDF1 step with theta = 0 from the steady solution: u_t = 0 there, so the step's first residual IS the steady one
    dt = 0.1
    P.set_time_term(1.0 / dt, 0.0, ws * (-1.0 / dt))
    f_first = float(P.residual(ws, "ns").norm())
    P.clear_time_term()
    assert abs(f_first - f_steady) <= 1e-9 * f_stokes, (f_first, f_steady)
    P.set_options(snes_atol=1e-8 * f_stokes)                       # (the steady solve ended below this)
    w = ws.clone()
    _, r1 = P.time_step(w, None, dt, order=1, theta_coeff=0.0)
    assert r1.reason > 0 and r1.its <= 1, r1
    assert float((w - ws).norm() / ws.norm()) < 1e-6
    solve = S.solve_navier_stokes(P, P.zeros(), rank=1, continuation="ptc", ptc_dt0=0.5)[0]
    assert _fields_close(solve.cpu().numpy(), ws.cpu().numpy())
    P.close()


# ---- 7. forces ---------------------------------------------------------------------------------------------------------
def test_residual_moments_after_a_step_against_the_oracle():
    rng = np.random.default_rng(37)
    fx = np.load(FIXTURE)
    m, mask, g, _ = stepping_problem()
    P = FlowProblem(m, (mask, g), reynolds=CASE["Re"], **TIGHT)
    w0 = fx["w0"]
    w, wprev = _dev(w0), _dev(w0)
    dt = 0.05
    assert P.time_step(w, wprev, dt, order=1)[1].reason > 0
    w1 = w.cpu().numpy().copy()
    assert P.time_step(w, wprev, dt, order=2)[1].reason > 0
    sigma, d = NS.bdf(2, dt, w1, w0)
    wh = w.cpu().numpy()
    F, _ = NS.raw(m.points, m.tets, wh, CASE["Re"], d=d, sigma=sigma, theta=4.0 / dt ** 2, want_jac=False)
    for phi in (rng.uniform(-1.0, 1.0, size=m.num_nodes), (m.points[:, 0] < 0.5).astype(np.float64)):
        out = P.residual_moments(w, phi)
        ref = (phi[:, None] * F.reshape(-1, 4)).sum(axis=0)
        assert np.abs(out - ref).max() <= 1e-12 * np.linalg.norm(ref), (out, ref)
    Fs, _ = NS.raw(m.points, m.tets, wh, CASE["Re"], d=0 * d, want_jac=False)
    assert np.abs(F - Fs).max() > 1e-6 * np.abs(Fs).max()         # (the transient residual is another residual)
    P.close()


# ---- 8. error paths, adjoint -------------------------------------------------------------------------------------------
def test_refusals():
    m, mask, g, w0 = stepping_problem()
    P = FlowProblem(m, (mask, g), reynolds=CASE["Re"])
    d = P.zeros()
    for sigma, theta, dd in ((-1.0, 0.0, d), (float("nan"), 0.0, d), (float("inf"), 0.0, d), (1.0, -2.0, d), (1.0, float("nan"), d),
                             (1.0, 0.0, None)):
        with pytest.raises(SnsError) as e:
            P.set_time_term(sigma, theta, dd)
        assert e.value.code == -1, (sigma, theta)
    w, wprev = _dev(w0), _dev(w0)
    for kw in (dict(order=0), dict(order=3), dict(dt=0.0), dict(dt=-0.1)):
        a = dict(dt=0.1, order=1)
        a.update(kw)
        with pytest.raises(SnsError) as e:
            P.time_step(w, wprev, a["dt"], order=a["order"])
        assert e.value.code == -1, kw
    with pytest.raises(SnsError) as e:
        P.time_step(w, None, 0.1, order=2)                          # BDF2 needs the state before w
    assert e.value.code == -1
    assert torch.equal(w, _dev(w0))
    P.set_time_term(0.0, 7.0, None)                                 # theta alone is a valid term
    P.close()
    # a step that does not converge reports its reason and restores both states
    Q = FlowProblem(m, (mask, g), reynolds=CASE["Re"], snes_max_it=1, snes_rtol=1e-14, snes_atol=1e-30, snes_stol=0.0)
    w, wprev = _dev(w0), _dev(0.5 * w0)
    _, r = Q.time_step(w, wprev, 0.1, order=2)
    assert r.reason < 0 and torch.equal(w, _dev(w0)) and torch.equal(wprev, _dev(0.5 * w0))
    Q.close()
    # 2-D handles
    m2 = M2.dfg_2d_mesh(0.5)
    P2 = FlowProblem(m2, M2.dfg2d_bcs(m2).flatten(), reynolds=100.0)
    with pytest.raises(SnsError) as e:
        P2.set_time_term(1.0, 0.0, P2.zeros())
    assert e.value.code == -1
    with pytest.raises(SnsError) as e:
        P2.time_step(P2.zeros(), None, 0.1, order=1)
    assert e.value.code == -1
    P2.close()
    # a handle with an owned / ghost split attached (no transport needed): SNS_E_STATE, as for the adjoint solves
    from stabilized_navier_stokes_flow_fenicsx_amd import partition as PT
    part = PT.build_local_part(m, mask, g, PT.rcb_partition(m.points, 2), 0, 2)
    R = FlowProblem(part.mesh, (part.bc_mask, part.bc_val), part=part, group="local-only", reynolds=CASE["Re"])
    with pytest.raises(SnsError) as e:
        R.set_time_term(1.0, 0.0, R.zeros())
    assert e.value.code == -3
    with pytest.raises(SnsError) as e:
        R.time_step(R.zeros(), None, 0.1, order=1)
    assert e.value.code == -3
    R.close()


def test_stokes_form_ignores_the_term():
    rng = np.random.default_rng(38)
    m, mask, g, _ = stepping_problem()
    P = FlowProblem(m, (mask, g), reynolds=CASE["Re"])
    F0 = P.zeros()
    P.jacobian(None, "stokes", residual_out=F0)
    v0 = P.bsr()[2].clone()
    P.set_time_term(9.0, 4.0, _hist(rng, m.num_nodes))
    F1 = P.zeros()
    P.jacobian(None, "stokes", residual_out=F1)
    assert torch.equal(v0, P.bsr()[2]) and torch.equal(F0, F1)
    P.close()


def test_adjoint_identity_on_a_transient_jacobian():
    m = M.duct_mesh((40, 10, 10), 2.0)
    P = FlowProblem(m, B.duct_bcs(m).flatten(), reynolds=25.0)
    U, res = P.stokes_solve()
    assert res.reason > 0
    dt = 0.05
    P.set_time_term(1.5 / dt, 4.0 / dt ** 2, U * (-1.5 / dt))
    P.jacobian(U, "ns")
    A = P.to_scipy()
    rng = np.random.default_rng(39)
    free = P.bc_mask == 0
    for vanish in (True, False):
        b, gg = rng.normal(size=P.ndof), rng.normal(size=P.ndof)
        if vanish:
            b, gg = b * free, gg * free
        _adjoint_identity(P, A, b, gg, f"transient vanish={vanish}")
    P.close()
