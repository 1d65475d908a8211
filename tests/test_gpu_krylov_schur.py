"""Thick-restarted (Krylov-Schur) stability analysis on the GPU (sns_basis_rotate / k_basis_rotate, sns_stability_arnoldi_extend;
solver.linear_stability(max_restarts > 0)), everything through the C-ABI.

The yardstick is the test-side oracle tests/krylov_schur_oracle.py (the arithmetic of tests/stability_oracle.py's Arnoldi from a
column k, the package's own truncation, sparse-LU solves), whose own checks are tests/test_host_krylov_schur.py.  Cases: the
ducts (6,3,3) Re 50 -- 448 dofs, no multiple of the block of 256 -- and (3,2,2) Re 50 -- 144 dofs, 9 of them free velocities --,
the smallest on which a restart happens at all.  Bounds: the rotation 1e-14 n_in relative to the largest entry of the result
(n_in products and sums in fp64); orthogonality 1e-12; everything that depends on the inner tolerance -- the Krylov relation,
the eigenvalues, the modes' true residuals -- 10 x what the oracle's emulation of that tolerance (every LU solve perturbed to
the relative residual 1e-10) gives, computed here at run time, as tests/test_gpu_stability.py does and for its reason."""
import functools

import numpy as np
import pytest
import torch

import krylov_schur_oracle as KO
import stability_oracle as SO
from stabilized_navier_stokes_flow_fenicsx_amd import mesh2d as M2
from stabilized_navier_stokes_flow_fenicsx_amd import solver as S
from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem, SnsError

pytestmark = pytest.mark.gpu
INNER = 1e-10
TOL = 1e-7
PARAMS = ((12, 6, 4), (16, 8, 6))
SHIFTS = (0.0, 2.5)
K_TEXT = "k must lie in [1, m - 1]"


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _problem(c, **kw):
    return FlowProblem(c.mesh, (c.mask, c.g), reynolds=c.Re, **kw)


@functools.lru_cache(maxsize=None)
def dense_spectrum(name):
    c = SO.case(name)
    return SO.dense_spectrum(*c.operators(), c.constrained)


@functools.lru_cache(maxsize=None)
def emulation(shift, params, left=False):
    """The oracle's restarted run on duct633 at the inner tolerance: restarts, its worst distance to the dense spectrum and the
    worst true residual of its n_modes modes."""
    c = SO.case("duct633")
    J, B = c.operators()
    m, keep, n_modes = params
    V, H, restarts, lam, info = KO.restarted(J, B, c.constrained, shift, m, keep, n_modes, 20, TOL, INNER, left=left)
    assert info["converged"]
    lam_all, Y, est = S.krylov_ritz_pairs(H, info["m_done"], shift)
    lead = np.argsort(np.abs(lam_all - shift), kind="stable")[:n_modes]
    Jm, Bm = (J.T, B.T) if left else (J, B)
    res = max(SO.mode_residual(Jm, Bm, lam_all[i], V[:info["m_done"]].T @ Y[:, i]) for i in lead)
    return dict(restarts=restarts, worst=SO.nearest(dense_spectrum("duct633"), lam).max(), residual=res, est=est[lead].max())


# ---- 6. the rotation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["duct633", "duct322"])
def test_basis_rotate_against_numpy(name):
    c = SO.case(name)
    P = _problem(c)
    ndof = len(c.w)
    assert ndof == P.ndof and ndof in (448, 144)
    rng = np.random.default_rng(17)
    for n_in, n_out in ((65, 1), (65, 65), (65, 9), (13, 7), (3, 2), (1, 1)):
        qs = [("random", rng.standard_normal((n_in, n_out)))]
        if (n_in, n_out) == (65, 9):
            qs.append(("orthogonal", np.linalg.qr(rng.standard_normal((n_in, n_in)))[0][:, :n_out]))
        for kind, Q in qs:
            V0 = rng.standard_normal((66, ndof))
            ref = Q.T @ V0[:n_in]
            V = _dev(V0)
            assert P.basis_rotate(V, Q) is V
            got = V.cpu().numpy()
            err = np.abs(got[:n_out] - ref).max() / np.abs(ref).max()
            print(name, n_in, n_out, kind, "max|dV| / max|V_ref| =", err)
            assert err <= 1e-14 * n_in
            assert not got[n_out:n_in].any()                                           # the columns given up: exactly 0
            assert np.array_equal(got[n_in:], V0[n_in:])                               # the columns behind: not touched
            V2 = _dev(V0)
            P.basis_rotate(V2, Q)
            assert torch.equal(V, V2)                                                  # two runs: identical bits
        V = _dev(V0)
        P.basis_rotate(V, np.eye(n_in)[:, :n_out])
        got = V.cpu().numpy()
        assert np.array_equal(got[:n_out], V0[:n_out]) and not got[n_out:n_in].any() and np.array_equal(got[n_in:], V0[n_in:])
    # refusals: SNS_E_ARG, V untouched
    V = _dev(V0)
    for Q in (np.zeros((66, 1)), np.full((3, 2), np.nan), np.array([[1.0], [np.inf]]), np.zeros((0, 0))):
        with pytest.raises(SnsError) as e:
            P.basis_rotate(V, Q)
        assert e.value.code == -1 and "sns_basis_rotate" in str(e.value), Q.shape
    lib, q = P.lib, np.ones((4, 4))
    for n_in, n_out, Qp, Vp in ((0, 0, q.ctypes.data, V.data_ptr()), (66, 1, q.ctypes.data, V.data_ptr()), (2, 0, q.ctypes.data, V.data_ptr()),
                                (2, 3, q.ctypes.data, V.data_ptr()), (2, 2, None, V.data_ptr()), (2, 2, q.ctypes.data, None)):
        assert lib.sns_basis_rotate(P.h, n_in, n_out, Qp, Vp) == -1
        assert b"sns_basis_rotate: " in lib.sns_last_error()
    assert np.array_equal(V.cpu().numpy(), V0)
    with pytest.raises(ValueError):
        P.basis_rotate(_dev(V0[:3]), np.ones((4, 2)))                                  # fewer rows than Q reads
    P.close()


# ---- 7. the extension continues what stability_arnoldi began ---------------------------------------------------------------------
@pytest.mark.parametrize("side", ["right", "left"])
@pytest.mark.parametrize("shift", SHIFTS)
def test_extend_continues_the_decomposition(shift, side):
    c = SO.case("duct633")
    J, B = c.operators()
    Jm, Bm = (J.T.tocsr(), B.T.tocsr()) if side == "left" else (J, B)
    m, keep = 12, 6
    # the oracle's figure for the same sequence at the inner tolerance
    solve = SO.Solver(Jm, Bm, shift, c.constrained, INNER)
    Vo, Ho, mo, _ = KO.first_cycle(solve, Bm, c.constrained, m)
    ko, Qo, Hko = S.krylov_schur_truncate(Ho, mo, keep)
    Vo[:ko + 1] = Qo.T @ Vo
    Vo[ko + 1:] = 0.0
    Ho[:] = 0.0
    Ho[:ko + 1, :ko] = Hko
    mo, _ = KO.extend(solve, Bm, c.constrained, Vo, Ho, ko, m)
    ref = SO.arnoldi_relation(Jm, Bm, c.constrained, shift, Vo, Ho, mo)

    P = _problem(c, ksp_rtol=INNER)
    wd = _dev(c.w)
    before = P.residual(wd).clone()
    V, H, res = P.stability_arnoldi(wd, shift=shift, m=m, side=side)
    assert (res.m_done, res.reason) == (m, 1)
    k, Q, Hk = S.krylov_schur_truncate(H, res.m_done, keep)
    P.basis_rotate(V, Q)
    H[:] = 0.0
    H[:k + 1, :k] = Hk
    H[k + 1:, :] = 7.0                                                                 # (outside the block the call keeps: zeroed by it)
    H[:, k:] = 7.0
    res2 = P.stability_arnoldi_extend(wd, V, H, k, shift=shift, side=side)
    assert (res2.m_done, res2.reason) == (m, 1) and res2.ksp_its > 0
    Vn = V.cpu().numpy()
    orth = SO.orthogonality(Vn, m + 1)
    rel = SO.arnoldi_relation(Jm, Bm, c.constrained, shift, Vn, H, m)
    print(side, shift, "k", k, "orthogonality", orth, "relation", rel, "oracle", ref)
    assert orth <= 1e-12
    assert rel <= 10.0 * ref
    assert np.array_equal(H[:k + 1, :k], Hk) and not H[k + 1:, :k].any()               # the caller's block kept, zero below it
    ii, jj = np.tril_indices(m + 1, -2, m)
    assert not H[ii, jj][jj >= k].any() and H[:k, k:].all()                            # behind it: full above the subdiagonal
    assert not Vn[:, c.constrained].any()
    # the handle afterwards: steady, untransposed, its matrix J + shift B
    assert torch.equal(P.residual(wd), before)
    P.set_time_term(1.0, 0.0, P.zeros())                                               # (allowed again: none is set)
    P.clear_time_term()
    assert not P.operator_transposed
    Js = c.jacobian(shift) if shift else J
    assert abs(P.to_scipy() - Js).max() <= 1e-12 * abs(Js).max()
    P.close()


# ---- 8. linear_stability with restarts -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("shift", SHIFTS)
def test_linear_stability_with_restarts(shift, params):
    c = SO.case("duct633")
    J, B = c.operators()
    m, keep, n_modes = params
    emu, emuL = emulation(shift, params), emulation(shift, params, True)
    P = _problem(c, ksp_rtol=1e-6)
    wd = _dev(c.w)
    r = S.linear_stability(P, wd, n_modes=n_modes, shift=shift, m=m, tol=TOL, ksp_rtol=INNER, left=True, max_restarts=40, keep=keep)
    assert P.options.ksp_rtol == 1e-6 and not P.operator_transposed
    X, Z = r.modes.cpu().numpy(), r.left_modes.cpu().numpy()
    worst = SO.nearest(dense_spectrum("duct633"), r.eigenvalues).max()
    resid = max(SO.mode_residual(J, B, lam, x) for lam, x in zip(r.eigenvalues, X))
    print(shift, params, "restarts", r.restarts, "left", r.left_restarts, "oracle", emu["restarts"], emuL["restarts"], "worst", worst,
          "oracle", emu["worst"], "true residual", resid, "oracle", emu["residual"], "eigenvalues", r.eigenvalues)
    assert r.reason == 1 and r.m_done == m and r.converged.all() and len(r.eigenvalues) == n_modes
    assert 1 <= r.restarts <= 2 * emu["restarts"] and 1 <= r.left_restarts <= 2 * emuL["restarts"]
    assert worst <= 10.0 * emu["worst"]
    assert resid <= 10.0 * emu["residual"]
    assert r.left_converged.all()
    pairing = np.array([Z[k] @ (B @ X[k]) for k in range(n_modes)])
    print("max |z^T B x - 1|", np.abs(pairing - 1.0).max())
    assert np.abs(pairing - 1.0).max() <= 1e-8
    # d lambda / d Re of the leading mode against the unrestarted m = 64 analysis on the same handle
    r64 = S.linear_stability(P, wd, n_modes=6, shift=shift, m=64, tol=TOL, ksp_rtol=INNER, left=True)
    j = int(np.abs(r64.eigenvalues - r.eigenvalues[0]).argmin())
    assert r64.left_converged[j] and abs(r64.eigenvalues[j] - r.eigenvalues[0]) <= 10.0 * TOL * abs(r.eigenvalues[0])
    d_restarted, _ = S.eigenvalue_reynolds_sensitivity(P, wd, r, k=0)
    d_64, _ = S.eigenvalue_reynolds_sensitivity(P, wd, r64, k=j)
    bound = (r.estimates[0] + r64.estimates[j]) * abs(r.eigenvalues[0])
    print("d lam / d Re restarted", d_restarted, "m = 64", d_64, "difference", abs(d_restarted - d_64), "bound", bound)
    assert abs(d_restarted - d_64) <= bound
    P.close()


# ---- 9. edge cases ---------------------------------------------------------------------------------------------------------------
def test_breakdown_in_the_first_cycle_on_the_nine_dof_duct():
    """As test_breakdown_on_the_nine_dof_duct of tests/test_gpu_stability.py, through linear_stability with restarts allowed:
    the exact process ends at step 9, breakdown_rel sits between the emulation's step-9 ratio and the smallest genuine one."""
    c = SO.case("duct322")
    J, B = c.operators()
    ratios = np.array([SO.arnoldi(J, B, c.constrained, m=9, inner_rtol=INNER, seed=seed, breakdown_rel=1e-30)[3] for seed in range(8)])
    spurious, genuine = ratios[:, 8].max(), ratios[:, :8].min()
    breakdown_rel = float(np.sqrt(spurious * genuine))
    assert spurious * 10.0 < breakdown_rel < genuine / 10.0
    P = _problem(c)
    r = S.linear_stability(P, _dev(c.w), n_modes=4, m=12, tol=TOL, ksp_rtol=INNER, max_restarts=20, breakdown_rel=breakdown_rel)
    P.close()
    print("m_done", r.m_done, "reason", r.reason, "restarts", r.restarts, "eigenvalues", r.eigenvalues)
    assert r.reason == 2 and r.m_done <= 9 and r.restarts == 0
    assert np.isfinite(r.eigenvalues).all() and len(r.eigenvalues) == 4
    assert SO.nearest(dense_spectrum("duct322"), r.eigenvalues).max() <= 10.0 * spurious


def test_an_unconverged_inner_solve_ends_a_restarted_run_quietly():
    c = SO.case("duct633")
    P = _problem(c, ksp_max_it=1)
    wd = _dev(c.w)
    before = P.residual(wd).clone()
    calls = []
    extend, rotate = P.stability_arnoldi_extend, P.basis_rotate
    P.stability_arnoldi_extend = lambda *a, **kw: calls.append("extend") or extend(*a, **kw)
    P.basis_rotate = lambda *a, **kw: calls.append("rotate") or rotate(*a, **kw)
    r = S.linear_stability(P, wd, n_modes=4, shift=2.5, m=12, tol=TOL, ksp_rtol=1e-14, left=True, max_restarts=20)
    print("reason", r.reason, r.left_reason, "m_done", r.m_done, r.left_m_done)
    assert r.reason < 0 and r.left_reason < 0 and r.m_done == 0 and r.left_m_done == 0
    assert r.restarts == 0 and r.left_restarts == 0 and calls == [] and len(r.eigenvalues) == 0
    assert torch.equal(P.residual(wd), before) and not P.operator_transposed
    P.close()


def test_refusals_of_the_extension():
    c = SO.case("duct322")
    P = _problem(c)
    wd = _dev(c.w)
    m = 8

    def buffers(Q):
        return torch.zeros(m + 1, Q.ndof, dtype=torch.float64, device="cuda"), np.zeros((m + 1, m))

    V, H = buffers(P)
    for side in ("right", "left"):
        for k in (0, m, -1, m + 3):
            with pytest.raises(SnsError) as e:
                P.stability_arnoldi_extend(wd, V, H, k, side=side)
            assert e.value.code == -1 and str(e.value).endswith("sns_stability_arnoldi_extend: " + K_TEXT), (side, k)
        for kw in (dict(shift=-1.0), dict(shift=float("nan")), dict(breakdown_rel=0.0), dict(breakdown_rel=1.0)):
            with pytest.raises(SnsError) as e:
                P.stability_arnoldi_extend(wd, V, H, 0, side=side, **kw)                # the other arguments come before k
            assert e.value.code == -1 and K_TEXT not in str(e.value), kw
        P.set_time_term(1.0, 0.0, P.zeros())
        with pytest.raises(SnsError) as e:
            P.stability_arnoldi_extend(wd, V, H, 0, side=side)                          # k before the state
        assert e.value.code == -1 and K_TEXT in str(e.value)
        with pytest.raises(SnsError) as e:
            P.stability_arnoldi_extend(wd, V, H, 3, side=side)
        assert e.value.code == -3 and "time term" in str(e.value)
        P.clear_time_term()
        P.set_viscosity_law(0.5, 0.7)
        with pytest.raises(SnsError) as e:
            P.stability_arnoldi_extend(wd, V, H, 3, side=side)
        assert e.value.code == -3 and "viscosity law" in str(e.value)
        P.clear_viscosity_law()
    with pytest.raises(ValueError):
        P.stability_arnoldi_extend(wd, V[:m], H, 3)
    with pytest.raises(ValueError):
        P.stability_arnoldi_extend(wd, V, H[:, :m - 1], 3)
    with pytest.raises(ValueError):
        P.stability_arnoldi_extend(wd, V, H, 3, side="both")
    P.close()
    # 2-D handles
    m2 = M2.dfg_2d_mesh(0.5)
    P2 = FlowProblem(m2, M2.dfg2d_bcs(m2).flatten(), reynolds=100.0)
    V2, H2 = buffers(P2)
    for side in ("right", "left"):
        with pytest.raises(SnsError) as e:
            P2.stability_arnoldi_extend(P2.zeros(), V2, H2, 3, side=side)
        assert e.value.code == -1 and str(e.value).endswith("3-D handles only")
    P2.basis_rotate(V2, np.eye(3)[:, :2])                                              # the rotation works on any handle
    P2.close()
    # a handle with an owned / ghost split attached: SNS_E_STATE
    from stabilized_navier_stokes_flow_fenicsx_amd import partition as PT
    c6 = SO.case("duct633")
    part = PT.build_local_part(c6.mesh, c6.mask, c6.g, PT.rcb_partition(c6.mesh.points, 2), 0, 2)
    R = FlowProblem(part.mesh, (part.bc_mask, part.bc_val), part=part, group="local-only", reynolds=c6.Re)
    VR, HR = buffers(R)
    for side in ("right", "left"):
        with pytest.raises(SnsError) as e:
            R.stability_arnoldi_extend(R.zeros(), VR, HR, 3, side=side)
        assert e.value.code == -3 and "communicator" in str(e.value)
        with pytest.raises(SnsError) as e:
            R.stability_arnoldi_extend(R.zeros(), VR, HR, 0, side=side)
        assert e.value.code == -1 and K_TEXT in str(e.value)
    R.close()


# ---- 10. without restarts nothing changes ------------------------------------------------------------------------------------------
def test_max_restarts_zero_is_the_unrestarted_function_bit_for_bit():
    c = SO.case("duct633")
    out = []
    for kw in ({}, dict(max_restarts=0, keep=5)):
        P = _problem(c)
        r = S.linear_stability(P, _dev(c.w), n_modes=6, shift=2.5, m=16, tol=TOL, ksp_rtol=INNER, left=True, **kw)
        P.close()
        out.append(r)
    a, b = out
    assert a.restarts == b.restarts == 0 and a.left_restarts == b.left_restarts == 0
    for name in ("eigenvalues", "estimates", "converged", "left_converged"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(a.left_eigenvalues, b.left_eigenvalues, equal_nan=True)
    assert torch.equal(a.modes, b.modes) and torch.equal(a.left_modes, b.left_modes)
    assert (a.m_done, a.ksp_its, a.reason, a.left_m_done, a.left_ksp_its, a.left_reason) == \
           (b.m_done, b.ksp_its, b.reason, b.left_m_done, b.left_ksp_its, b.left_reason)


# ---- 11. the scripts' switch -----------------------------------------------------------------------------------------------------
def test_the_driver_switch_passes_the_restart_arguments_through(monkeypatch, capsys):
    """SNS_STABILITY_RESTARTS beside SNS_STABILITY: the modes' lines followed by one line with the restart counts; without it
    nothing new is printed; alone it does nothing."""
    from stabilized_navier_stokes_flow_fenicsx_amd import drivers as D
    c = SO.case("duct633")
    P = _problem(c)
    wd = _dev(c.w)
    for name in ("SNS_STABILITY_SENSITIVITY", "SNS_STABILITY_FORCING", "SNS_STABILITY"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SNS_STABILITY_RESTARTS", "20,12,6")
    assert D._stability(P, wd) is None and capsys.readouterr().out == ""
    monkeypatch.setenv("SNS_STABILITY", "4")
    r1 = D._stability(P, wd)
    restarted = capsys.readouterr().out.splitlines()
    monkeypatch.delenv("SNS_STABILITY_RESTARTS")
    r0 = D._stability(P, wd)
    plain = capsys.readouterr().out.splitlines()
    P.close()
    assert r0.restarts == 0 and r0.m_done == 64 and 1 <= r1.restarts <= 20 and r1.m_done == 12
    assert len(plain) == 4 and all(ln.startswith("Stability mode:") for ln in plain)
    assert len(restarted) == 5 and restarted[4].startswith(f"Stability restarts: right {r1.restarts} of at most 20")
    lam = lambda lines: np.array([complex(float(ln.split()[4]), float(ln.split()[5][:-1])) for ln in lines])
    # (the restarted run goes for the four pairs nearest the shift, the 64 steps also reach less stable ones farther away: the
    # lists differ.)  Either list is the dense spectrum's, to 10 tol plus the seven printed digits
    for lines in (restarted[:4], plain):
        assert SO.nearest(dense_spectrum("duct633"), lam(lines)).max() <= 10.0 * TOL + 1e-6
