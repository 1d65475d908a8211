"""The resolvent analysis on the GPU (sns_energy_apply / k_energy_pass, sns_lumped_volumes, sns_resolvent_lanczos;
solver.resolvent_analysis, the SNS_RESOLVENT switch of the drivers), everything through the C-ABI.

The yardstick is the test-side oracle tests/resolvent_oracle.py (the mass matrix from the mesh in numpy, scipy's complex sparse LU
on the oracle's J and B, the process in numpy, the dense T), whose own checks are tests/test_host_resolvent.py.  Cases: the ducts
(6,3,3) Re 50 -- 448 dofs, no multiple of the block of 256, node -> cell lists of every length mod 4, 72 free velocity dofs --,
(8,3,3) Re 200 and (3,2,2) with 9 free velocity dofs.  sigma_2 / sigma_1 is 0.80 - 0.96 on them: modes are paired by index after
sorting.  Bounds: the operator 1e-12 relative to the largest entry of the result (the project's operator standard); the symmetry
of Q 1e-13 of |x|_1 max|Q y| + |y|_1 max|Q x| (every entry of a result carries the rounding of at most 24 cells of 5 fused
operations each, some 100 eps of the largest); the lumped volumes 1e-14; orthogonality 1e-12; what depends on the inner tolerance
-- the relation T V_m = V_{m+1} H with the ORACLE's matrices, the skew part of H, the gains -- 10 x what the oracle's emulation of
that tolerance gives, computed here at run time (the convention of tests/test_gpu_complex_shift.py)."""
import functools
import os

import numpy as np
import pytest
import torch

import resolvent_oracle as RO
import stability_oracle as SO
from stabilized_navier_stokes_flow_fenicsx_amd import mesh2d as M2
from stabilized_navier_stokes_flow_fenicsx_amd import solver as S
from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem, SnsError

pytestmark = pytest.mark.gpu
INNER = 1e-10
KSP_DIVERGED_ITS = -3


def _dev(x):
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)).cuda()


def _problem(c, **kw):
    return FlowProblem(c.mesh, (c.mask, c.g), reynolds=c.Re, **kw)


def _halves(c):
    """Nodal weights: 1 on the upstream half of the nodes, and 1 on the downstream half."""
    x = c.mesh.points[:, 0]
    return (x < np.median(x)).astype(np.float64), (x >= np.median(x)).astype(np.float64)


def _sq_err(g, dense):
    """Relative distance of the squared gains, index by index."""
    k = len(g)
    return np.abs(g ** 2 - dense[:k] ** 2) / dense[:k] ** 2


@functools.lru_cache(maxsize=None)
def dense(name, omega, weighted=False):
    c = SO.case(name)
    up, down = _halves(c) if weighted else (None, None)
    return RO.dense_gains(RO.Resolvent(c, omega, forcing_weight=up, response_weight=down))[0]


@functools.lru_cache(maxsize=None)
def emulation(name, omega, m=16, weighted=False):
    """The oracle's process at the inner tolerance: its relation, the skew part of its H, the worst relative distance of its
    squared gains to the dense ones -- over the leading two, or over all of them where the process broke down."""
    c = SO.case(name)
    up, down = _halves(c) if weighted else (None, None)
    R = RO.Resolvent(c, omega, forcing_weight=up, response_weight=down, inner_rtol=INNER)
    V, H, k, reason, _ = RO.lanczos(R, m=m)
    err = _sq_err(RO.gains(H, k), dense(name, omega, weighted))
    exact = RO.Resolvent(c, omega, forcing_weight=up, response_weight=down)
    return dict(relation=RO.relation(exact, V, H, k), skew=RO.skew(H, k), worst=float((err if reason == 2 else err[:2]).max()),
                m_done=k, reason=reason)


# ---- 1. the energy pass --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", ["duct633", "duct322"])
def test_energy_pass_against_the_oracle(name, weighted):
    c = SO.case(name)
    rng = np.random.default_rng(17)
    n, nn = len(c.w), len(c.mesh.points)
    chi = rng.uniform(0.0, 1.0, nn) if weighted else None
    Q = RO.energy_matrix(c, chi)
    x, y = rng.standard_normal(n), rng.standard_normal(n)                        # (constrained and pressure entries are not zero)
    P = _problem(c)
    xd, yd = _dev(x), _dev(y)
    Qx, Qy = P.energy_apply(xd, chi).clone(), P.energy_apply(yd, chi).clone()
    ref = Q @ x
    err = np.abs(Qx.cpu().numpy() - ref).max() / np.abs(ref).max()
    a, b = float(xd @ Qy), float(yd @ Qx)
    scale = float(xd.abs().sum() * Qy.abs().max() + yd.abs().sum() * Qx.abs().max())
    print(name, weighted, "max|dy| / max|y_ref| =", err, "x.Qy - y.Qx =", a - b, "of", scale)
    assert err <= 1e-12
    assert abs(a - b) <= 1e-13 * scale
    assert torch.equal(Qx, P.energy_apply(xd, chi))                               # two runs: identical bits
    # parts = 2: each part is the single-vector pass, bit for bit
    z = P.energy_apply(torch.complex(xd, yd), chi)
    assert z.dtype == torch.complex128 and torch.equal(z.real, Qx) and torch.equal(z.imag, Qy)
    assert torch.equal(z, P.energy_apply(torch.complex(xd, yd), chi))
    # rows that are 0: exactly
    got = Qx.cpu().numpy()
    assert not got[c.constrained].any() and not got[3::4].any() and got[~c.constrained & (np.arange(n) % 4 != 3)].all()
    # the lumped volumes
    ml = P.lumped_volumes()
    node = S.lumped_volumes(c.mesh)
    mln = ml.cpu().numpy()
    assert torch.equal(ml, P.lumped_volumes()) and not mln[3::4].any()
    for comp in range(3):
        assert np.abs(mln[comp::4] - node).max() <= 1e-14 * node.max()
    P.close()


# ---- 2. the process ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gpu_run(name, omega, m=16):
    c = SO.case(name)
    J, _ = c.operators()
    fresh = _problem(c)
    w_ref, n_ref = fresh.newton_solve(_dev(c.w * 0.9 + 0.1 * c.g))
    fresh.close()
    P = _problem(c, gmres_restart=100)
    wd = _dev(c.w)
    default_rtol = P.options.ksp_rtol
    P.set_options(ksp_rtol=INNER)
    V, H, res = P.resolvent_lanczos(wd, omega, m=m)
    x = np.random.default_rng(7).standard_normal(len(c.w))
    ref = J @ x
    after = dict(flipped=P.operator_transposed, spmv=np.abs(P.spmv(_dev(x)).cpu().numpy() - ref).max() / np.abs(ref).max())
    P.set_time_term(1.0, 0.0, P.zeros())                                           # (allowed: the call left none set)
    P.clear_time_term()
    P.set_options(ksp_rtol=default_rtol)
    w2, n2 = P.newton_solve(_dev(c.w * 0.9 + 0.1 * c.g))
    after.update(newton=(n2.reason, n_ref.reason), dw=float((w2 - w_ref).abs().max() / w_ref.abs().max()))
    P.close()
    return V.cpu().numpy(), H, res, after


@pytest.mark.parametrize("name,omega", [("duct633", 6.0), ("duct833", 2.0)])
def test_the_process_basis_relation_and_gains(name, omega):
    c = SO.case(name)
    V, H, res, after = gpu_run(name, omega)
    emu = emulation(name, omega)
    R = RO.Resolvent(c, omega)
    assert (res.m_done, res.reason) == (16, 1) and res.ksp_its > 32
    orth = RO.orthogonality(V, 17)
    rel = RO.relation(R, V, H, 16)
    skew = RO.skew(H, 16)
    err = _sq_err(RO.gains(H, 16), dense(name, omega))
    print(name, omega, "orthogonality", orth, "relation", rel, "emulation", emu["relation"], "skew", skew, "emulation", emu["skew"],
          "gains", np.sqrt(np.linalg.eigvalsh(0.5 * (H[:16] + H[:16].conj().T))[::-1][:3]), "dense", dense(name, omega)[:3], "sq err", err[:3],
          "emulation", emu["worst"], "ksp its", res.ksp_its)
    assert orth <= 1e-12
    assert rel <= 10.0 * emu["relation"]
    assert skew <= 10.0 * emu["skew"]
    assert err[:2].max() <= 10.0 * emu["worst"]
    assert not V[:, c.constrained].any() and not V[:, 3::4].any() and not H[np.tril_indices(17, -2, 16)].any()
    # the handle afterwards: untransposed, J, the form steady, and a Newton solve as a fresh handle's
    print("afterwards", after)
    assert not after["flipped"] and after["spmv"] <= 1e-12
    assert after["newton"][0] > 0 and after["newton"][0] == after["newton"][1] and after["dw"] <= 1e-9


# ---- 3. breakdown --------------------------------------------------------------------------------------------------------------
def test_the_process_breaks_down_on_nine_free_velocity_dofs():
    c = SO.case("duct322")
    omega = 6.0
    emu = emulation("duct322", omega)
    assert (emu["m_done"], emu["reason"]) == (9, 2)
    P = _problem(c, ksp_rtol=INNER, gmres_restart=100)
    V, H, res = P.resolvent_lanczos(_dev(c.w), omega, m=16)
    flipped = P.operator_transposed
    P.close()
    V = V.cpu().numpy()
    err = _sq_err(RO.gains(H, res.m_done), dense("duct322", omega))
    print("m_done", res.m_done, "reason", res.reason, "sq err of the gains", err, "emulation", emu["worst"])
    assert (res.m_done, res.reason) == (9, 2) and not flipped
    assert len(err) == 9 and err.max() <= 10.0 * emu["worst"]
    assert RO.orthogonality(V, 9) <= 1e-12 and not V[9:].any() and not H[9:].any() and not H[:, 9:].any()


# ---- 4. weights ----------------------------------------------------------------------------------------------------------------
def test_weights_restrict_the_forcing_and_the_response():
    c = SO.case("duct633")
    omega = 6.0
    up, down = _halves(c)
    emu = emulation("duct633", omega, weighted=True)
    P = _problem(c, gmres_restart=100)
    r = S.resolvent_analysis(P, _dev(c.w), omega, n_modes=2, m=16, forcing_weight=up, response_weight=down, ksp_rtol=INNER)
    P.close()
    err = _sq_err(r.gains, dense("duct633", omega, True))
    print("weighted gains", r.gains, "dense", dense("duct633", omega, True)[:2], "unweighted", dense("duct633", omega)[:2], "sq err", err,
          "emulation", emu["worst"])
    assert (r.m_done, r.reason) == (16, 1) and len(r.gains) == 2
    assert err.max() <= 10.0 * emu["worst"]
    F = r.forcing_modes.cpu().numpy()
    outside = np.repeat(up == 0.0, 4)
    assert not F[:, outside].any() and not F[:, c.constrained].any() and not F[:, 3::4].any() and np.abs(F).max() > 0.0
    # the response is measured downstream alone: its norm there is 1
    Q = RO.energy_matrix(c, down)
    for k in range(2):
        q = r.response_modes[k].cpu().numpy()
        assert abs((q.conj() @ (Q @ q)).real - 1.0) <= 1e-12


# ---- 5. resolvent_analysis end to end --------------------------------------------------------------------------------------------
def test_resolvent_analysis_end_to_end():
    c = SO.case("duct633")
    omega = 6.0
    R = RO.Resolvent(c, omega)
    d = dense("duct633", omega)
    emu = emulation("duct633", omega, m=24)
    P = _problem(c, gmres_restart=100)
    wd = _dev(c.w)
    r = S.resolvent_analysis(P, wd, omega, n_modes=2, ksp_rtol=INNER)
    assert P.options.ksp_rtol == 1e-8 and not P.operator_transposed
    err = _sq_err(r.gains, d)
    print("gains", r.gains, "dense", d[:2], "sq err", err, "emulation", emu["worst"], "estimates", r.residuals, "converged", r.converged,
          "m_done", r.m_done, "ksp its", r.ksp_its)
    assert (r.m_done, r.reason) == (24, 1) and r.converged.all() and (np.diff(r.gains) <= 0.0).all()
    assert err.max() <= 10.0 * emu["worst"]
    ml = RO.lumped(c.mesh)
    for k in range(2):
        q, f = r.response_modes[k].cpu().numpy(), r.forcing_modes[k].cpu().numpy()
        assert abs((q.conj() @ (R.Q @ q)).real - 1.0) <= 1e-12                     # |q_k|_Q = 1
        assert abs((f.conj() @ (ml * f)).real - 1.0) <= 1e-12                      # |f_k|_ML = 1 (no forcing weight)
    # the response to the optimal forcing is sigma_1 q_1
    P.set_options(ksp_rtol=INNER)
    q1, kres = S.harmonic_response(P, wd, omega, r.forcing_modes[0])
    dq = float((q1 - r.gains[0] * r.response_modes[0]).abs().max() / q1.abs().max())
    exact = R.response(r.forcing_modes[0].cpu().numpy())
    print("harmonic response against sigma_1 q_1:", dq, "; against the oracle's exact response:",
          np.abs(q1.cpu().numpy() - exact).max() / np.abs(exact).max())
    assert kres.reason > 0 and dq <= 10.0 * INNER
    P.close()
    # no forcing gains more: five random ones, their responses by the oracle's exact solves
    rng = np.random.default_rng(23)
    on = RO.forcing_scale(c) > 0.0
    for _ in range(5):
        f = np.where(on, rng.standard_normal(len(c.w)) + 1j * rng.standard_normal(len(c.w)), 0.0)
        q = R.response(f)
        quotient = (q.conj() @ (R.Q @ q)).real / (f.conj() @ (ml * f)).real
        assert quotient <= r.gains[0] ** 2 * (1.0 + 1e-8), (quotient, r.gains[0] ** 2)


# ---- 6. an inner solve that does not converge ------------------------------------------------------------------------------------
def test_an_unconverged_inner_solve_ends_the_process_quietly():
    c = SO.case("duct633")
    P = _problem(c, ksp_max_it=3, ksp_rtol=1e-14, gmres_restart=100)
    wd = _dev(c.w)
    before = P.residual(wd).clone()
    V, H, res = P.resolvent_lanczos(wd, 6.0, m=8)
    print("reason", res.reason, "m_done", res.m_done, "ksp its", res.ksp_its)
    assert res.reason == KSP_DIVERGED_ITS and res.m_done <= 1 and not P.operator_transposed
    assert not H.any() and not V[res.m_done + 1:].any()
    assert torch.equal(P.residual(wd), before)
    P.set_options(ksp_max_it=10000, ksp_rtol=1e-8)
    V1, H1, r1 = P.resolvent_lanczos(wd, 6.0, m=8)
    V2, H2, r2 = P.resolvent_lanczos(wd, 6.0, m=8)
    assert (r1.m_done, r1.reason) == (8, 1) and not P.operator_transposed
    assert torch.equal(V1, V2) and np.array_equal(H1, H2) and (r1.m_done, r1.reason, r1.ksp_its) == (r2.m_done, r2.reason, r2.ksp_its)
    P.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_resolvent_calls():
    import ctypes as C
    c = SO.case("duct322")
    P = _problem(c)
    wd = _dev(c.w)
    x, y = P.zeros(), P.zeros()
    done = C.c_int()

    def lanczos_raw(h, w, omega, m, rel, V, Hbuf=None, lib=P.lib):
        Hbuf = np.zeros(2 * (max(m, 1) + 1) * max(m, 1)) if Hbuf is None else Hbuf
        rc = lib.sns_resolvent_lanczos(h, w, float(omega), int(m), float(rel), None, None, V, Hbuf.ctypes.data, C.byref(done), C.byref(done),
                                       C.byref(done))
        return rc, lib.sns_last_error().decode()

    # the call's own arguments
    for kw, text in ((dict(m=1), "m must lie in [2, 64]"), (dict(m=65), "m must lie in [2, 64]"),
                     (dict(omega=float("nan")), "omega must be finite"), (dict(omega=float("inf")), "omega must be finite"),
                     (dict(breakdown_rel=0.0), "breakdown_rel must lie in (0, 1)"), (dict(breakdown_rel=1.0), "breakdown_rel must lie in (0, 1)")):
        args = dict(omega=6.0, m=8)
        args.update(kw)
        with pytest.raises(SnsError) as e:
            P.resolvent_lanczos(wd, **args)
        assert e.value.code == -1 and str(e.value).endswith("sns_resolvent_lanczos: " + text), kw
    V = torch.zeros(9, 2 * P.ndof, dtype=torch.float64, device="cuda")
    rc, msg = lanczos_raw(P.h, V.data_ptr(), 6.0, 8, 1e-6, V.data_ptr())
    assert rc == -1 and msg.endswith("sns_resolvent_lanczos: V must not be the state or a weight vector")
    for call in (lambda: lanczos_raw(None, wd.data_ptr(), 6.0, 8, 1e-6, V.data_ptr()), lambda: lanczos_raw(P.h, None, 6.0, 8, 1e-6, V.data_ptr()),
                 lambda: lanczos_raw(P.h, wd.data_ptr(), 6.0, 8, 1e-6, None)):
        rc, msg = call()
        assert rc == -1 and msg.endswith("sns_resolvent_lanczos: null handle or pointer")
    assert P.lib.sns_energy_apply(P.h, None, 3, x.data_ptr(), y.data_ptr()) == -1
    assert P.lib.sns_last_error().decode().endswith("sns_energy_apply: parts must be 1 or 2")
    assert P.lib.sns_energy_apply(P.h, None, 1, x.data_ptr(), x.data_ptr()) == -1
    assert P.lib.sns_last_error().decode().endswith("sns_energy_apply: x and y must not be the same vector")
    assert P.lib.sns_energy_apply(P.h, None, 1, None, y.data_ptr()) == -1
    assert P.lib.sns_last_error().decode().endswith("sns_energy_apply: null handle or pointer")
    assert P.lib.sns_lumped_volumes(P.h, None) == -1
    assert P.lib.sns_last_error().decode().endswith("sns_lumped_volumes: null handle or pointer")
    with pytest.raises(ValueError):
        P.energy_apply(x, weight=np.ones(3))
    # the state: the process in the words of the stability family, after its arguments; the passes are not refused
    P.set_time_term(1.0, 0.0, P.zeros())
    with pytest.raises(SnsError) as e:
        P.resolvent_lanczos(wd, 6.0, m=8)
    assert e.value.code == -3 and str(e.value).endswith("sns_resolvent_lanczos: not with a time term set (the analysis sets its own and clears it)")
    with pytest.raises(SnsError) as e:
        P.resolvent_lanczos(wd, 6.0, m=1)
    assert e.value.code == -1 and str(e.value).endswith("m must lie in [2, 64]")
    P.energy_apply(x)
    P.lumped_volumes()
    P.clear_time_term()
    P.set_viscosity_law(0.5, 0.7)
    with pytest.raises(SnsError) as e:
        P.resolvent_lanczos(wd, 6.0, m=8)
    assert e.value.code == -3 and str(e.value).endswith("sns_resolvent_lanczos: not with a viscosity law set (the mass operator of the law's form is not built)")
    P.energy_apply(torch.complex(x, y))
    P.lumped_volumes()
    P.clear_viscosity_law()
    P.close()
    # 2-D handles: the dimension comes before the call's own arguments
    m2 = M2.dfg_2d_mesh(0.5)
    P2 = FlowProblem(m2, M2.dfg2d_bcs(m2).flatten(), reynolds=100.0)
    for call in (lambda: P2.resolvent_lanczos(P2.zeros(), 6.0, m=8), lambda: P2.resolvent_lanczos(P2.zeros(), 6.0, m=1),
                 lambda: P2.energy_apply(P2.zeros()), lambda: P2.lumped_volumes()):
        with pytest.raises(SnsError) as e:
            call()
        assert e.value.code == -1 and str(e.value).endswith("3-D handles only")
    x2 = P2.zeros()
    assert P2.lib.sns_energy_apply(P2.h, None, 3, x2.data_ptr(), x2.data_ptr()) == -1
    assert P2.lib.sns_last_error().decode().endswith("sns_energy_apply: 3-D handles only")
    P2.close()
    # a handle with an owned / ghost split attached (no transport needed): SNS_E_STATE from all three, after the arguments
    from stabilized_navier_stokes_flow_fenicsx_amd import partition as PT
    c6 = SO.case("duct633")
    part = PT.build_local_part(c6.mesh, c6.mask, c6.g, PT.rcb_partition(c6.mesh.points, 2), 0, 2)
    R = FlowProblem(part.mesh, (part.bc_mask, part.bc_val), part=part, group="local-only", reynolds=c6.Re)
    text = "not with a communicator attached (partitioned stability analysis is not built)"
    for who, call in (("sns_resolvent_lanczos", lambda: R.resolvent_lanczos(R.zeros(), 6.0, m=8)), ("sns_energy_apply", lambda: R.energy_apply(R.zeros())),
                      ("sns_lumped_volumes", lambda: R.lumped_volumes())):
        with pytest.raises(SnsError) as e:
            call()
        assert e.value.code == -3 and str(e.value).endswith(who + ": " + text)
    with pytest.raises(SnsError) as e:
        R.resolvent_lanczos(R.zeros(), float("nan"), m=8)
    assert e.value.code == -1 and str(e.value).endswith("omega must be finite")
    R.close()


# ---- 8. the scripts' switch ------------------------------------------------------------------------------------------------------
def test_the_driver_switch_prints_gains_and_writes_the_leading_pair(monkeypatch, capsys, tmp_path):
    """SNS_RESOLVENT=<n_modes>,<omega>,...: one line per frequency and mode, the result at the frequency of largest gain, its
    leading pair written as two fields; without the variable nothing is printed and nothing is written."""
    from stabilized_navier_stokes_flow_fenicsx_amd import drivers as D
    c = SO.case("duct633")
    P = _problem(c, gmres_restart=100)
    wd = _dev(c.w)
    monkeypatch.delenv("SNS_RESOLVENT", raising=False)
    assert D._resolvent(P, wd) is None and capsys.readouterr().out == ""
    D._write_resolvent(None, c.mesh, str(tmp_path / "DuctOptimalForcing"))
    assert os.listdir(tmp_path) == []
    monkeypatch.setenv("SNS_RESOLVENT", "2,2,6")
    r = D._resolvent(P, wd)
    lines = capsys.readouterr().out.splitlines()
    P.close()
    d2, d6 = dense("duct633", 2.0), dense("duct633", 6.0)
    print(lines)
    assert len(lines) == 4 and all(ln.startswith("Resolvent gain: omega ") for ln in lines)
    assert [float(ln.split()[3]) for ln in lines] == [2.0, 2.0, 6.0, 6.0]
    got = np.array([float(ln.split()[5]) for ln in lines])
    assert np.abs(got - np.array([d2[0], d2[1], d6[0], d6[1]])).max() <= 1e-6 * d2[0]
    assert d2[0] > d6[0] and r.omega == 2.0 and abs(r.gains[0] - d2[0]) <= 1e-6 * d2[0]
    D._write_resolvent(r, c.mesh, str(tmp_path / "DuctOptimalForcing"))
    assert sorted(os.listdir(tmp_path)) == ["DuctOptimalForcing.h5", "DuctOptimalForcing.xdmf", "DuctOptimalResponse.h5", "DuctOptimalResponse.xdmf"]
