"""Linear stability analysis on the GPU (sns_mass_apply, sns_stability_arnoldi; solver.ritz_pairs, solver.linear_stability),
everything through the C-ABI.

The reference has no counterpart; the yardstick is the test-side oracle tests/stability_oracle.py (B = J(1) - J(0) of
tests/ns3d_oracle.py, a numpy Arnoldi with sparse-LU solves, the dense spectrum by QZ), whose own checks are
tests/test_host_stability.py.  Cases: the ducts (6,3,3) Re 50, (8,3,3) Re 200 and (3,2,2) Re 50 of length 2 at the oracle's
converged state.  Bounds: the operator 1e-12 relative (the project's operator standard); orthogonality 1e-12 (the oracle has
7e-16; three orders for the GPU's summation orders); everything that depends on the inner tolerance -- the Arnoldi relation,
the eigenvalues, the modes' true residuals -- 10 x what the oracle's emulation of that tolerance (every LU solve perturbed to
the relative residual 1e-10) gives, computed here at run time: the solver stops on its recursive residual and not on the true
one, and the GPU operator differs from the oracle's at the 1e-12 level."""
import functools

import numpy as np
import pytest
import torch

import stability_oracle as SO
from oracle import forms_literal as FL
from stabilized_navier_stokes_flow_fenicsx_amd import mesh2d as M2
from stabilized_navier_stokes_flow_fenicsx_amd import solver as S
from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem, SnsError

pytestmark = pytest.mark.gpu
INNER = 1e-10
TOL = 1e-7
BIG = ("duct633", "duct833")
SHIFTS = (0.0, 2.0)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _problem(c, **kw):
    return FlowProblem(c.mesh, (c.mask, c.g), reynolds=c.Re, **kw)


# ---- shared results: one GPU run and one emulation per (case, shift) ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def gpu_run(name, shift):
    c = SO.case(name)
    P = _problem(c, ksp_rtol=INNER)
    V, H, res = P.stability_arnoldi(_dev(c.w), shift=shift, m=64)
    out = (V.cpu().numpy(), H, res)
    P.close()
    return out


@functools.lru_cache(maxsize=None)
def emulation(name, shift):
    """The oracle's Arnoldi at the inner tolerance, and its figures: (relation, worst relative distance of a converged pair to
    the dense spectrum, worst distance of the six dense eigenvalues nearest the shift to a converged pair, lam, conv, V, Y)."""
    c = SO.case(name)
    J, B = c.operators()
    V, H, m_done, _ = SO.arnoldi(J, B, c.constrained, shift=shift, inner_rtol=INNER)
    lam, Y, est = S.ritz_pairs(H, m_done, shift)
    conv = est <= TOL
    dense = dense_spectrum(name)
    six = dense[np.argsort(np.abs(dense - shift))][:6]
    return dict(relation=SO.arnoldi_relation(J, B, c.constrained, shift, V, H, m_done), worst=SO.nearest(dense, lam[conv]).max(),
                six=SO.nearest(lam[conv], six).max(), lam=lam, conv=conv, V=V, Y=Y, m_done=m_done)


@functools.lru_cache(maxsize=None)
def dense_spectrum(name):
    c = SO.case(name)
    return SO.dense_spectrum(*c.operators(), c.constrained)


# ---- 1. the mass pass ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "corrected", "form_variant", "viscosity_field"])
@pytest.mark.parametrize("name", ["duct633", "duct833"])
def test_mass_apply_against_the_oracle(name, variant):
    c = SO.case(name)
    rng = np.random.default_rng(71)
    x = rng.standard_normal(len(c.w))
    form, base = {}, dict(FL.VARIANT)
    P = _problem(c, corrected_convection=int(variant == "corrected"))
    try:
        if variant == "corrected":
            form = dict(corrected_convection=True)
        if variant == "form_variant":
            FL.VARIANT.update(ci=144.0, pspg=-1.0, one_point=True)
            P.set_form_variant(c_inverse=144.0, pspg_sign=-1.0, one_point_quadrature=True)
        if variant == "viscosity_field":
            nu = (1.0 / c.Re) * np.exp(rng.uniform(-1.5, 1.5, len(c.mesh.tets)))
            form = dict(nu_t=nu)
            P.set_element_viscosity(nu)
        B = c.mass(**form)
    finally:
        FL.VARIANT.update(base)
    ref = B @ x
    wd = _dev(c.w)
    y = P.mass_apply(wd, _dev(x))
    err = np.abs(y.cpu().numpy() - ref).max() / np.abs(ref).max()
    print(name, variant, "max|dy| / max|y_ref| =", err)
    assert err <= 1e-12
    assert torch.equal(y, P.mass_apply(wd, _dev(x)))                                   # two calls: identical bits
    assert not y.cpu().numpy()[c.constrained].any()                                    # constrained rows exactly 0
    x2 = x.copy()
    x2[c.constrained] = rng.standard_normal(c.constrained.sum()) * 1e3                 # constrained columns ...
    x2[3::4] = rng.standard_normal(len(x) // 4) * 1e3                                  # ... and pressure slots are ignored
    assert torch.equal(y, P.mass_apply(wd, _dev(x2)))
    out = P.zeros()
    assert P.mass_apply(wd, _dev(x), out=out) is out and torch.equal(out, y)
    P.close()


# ---- 2. the Arnoldi process ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("name", BIG)
def test_arnoldi_basis_and_relation(name, shift):
    c = SO.case(name)
    J, B = c.operators()
    V, H, res = gpu_run(name, shift)
    assert (res.m_done, res.reason) == (64, 1) and res.ksp_its > 0
    orth = SO.orthogonality(V, 65)
    rel = SO.arnoldi_relation(J, B, c.constrained, shift, V, H, 64)
    emu = emulation(name, shift)
    print(name, shift, "orthogonality", orth, "relation", rel, "emulation", emu["relation"], "ksp its", res.ksp_its)
    assert orth <= 1e-12
    assert rel <= 10.0 * emu["relation"]
    assert not V[:, c.constrained].any()
    assert not H[np.tril_indices(65, -2, 64)].any()


# ---- 3. eigenvalues --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("name", BIG)
def test_eigenvalues_against_the_dense_spectrum(name, shift):
    V, H, res = gpu_run(name, shift)
    lam, Y, est = S.ritz_pairs(H, res.m_done, shift)
    conv = est <= TOL
    emu = emulation(name, shift)
    dense = dense_spectrum(name)
    worst = SO.nearest(dense, lam[conv]).max()
    six = dense[np.argsort(np.abs(dense - shift))][:6]
    d6 = SO.nearest(lam[conv], six).max()
    print(name, shift, "converged", conv.sum(), "(emulation", emu["conv"].sum(), ") worst", worst, "emulation", emu["worst"],
          "six", d6, "emulation", emu["six"], "leading", lam[conv][:3])
    assert conv.sum() >= 20
    assert worst <= 10.0 * emu["worst"]
    assert d6 <= 10.0 * emu["six"]


@pytest.mark.parametrize("name", BIG)
def test_the_two_shifts_agree_on_the_six_nearest_eigenvalues(name):
    """For the six dense eigenvalues nearest each shift: the Ritz values the two runs assign to them differ by at most the sum
    of what either may be off, 10 x the emulation's distance to those six at that run's shift (triangle inequality through the
    dense eigenvalue)."""
    dense = dense_spectrum(name)
    for at in SHIFTS:
        six = dense[np.argsort(np.abs(dense - at))][:6]
        picks, bound = [], 0.0
        for shift in SHIFTS:
            _, H, res = gpu_run(name, shift)
            lam, _, est = S.ritz_pairs(H, res.m_done, shift)
            lam = lam[est <= TOL]
            picks.append(np.array([lam[np.abs(lam - t).argmin()] for t in six]))
            emu = emulation(name, shift)
            bound += 10.0 * SO.nearest(emu["lam"][emu["conv"]], six).max()
        diff = (np.abs(picks[0] - picks[1]) / np.abs(six)).max()
        print(name, "six nearest", at, "shift 0 vs shift 2", diff, "bound", bound)
        assert diff <= bound


# ---- 4. modes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("name", BIG)
def test_modes_satisfy_the_eigenproblem(name, shift):
    c = SO.case(name)
    J, B = c.operators()
    P = _problem(c, ksp_rtol=1e-6)
    r = S.linear_stability(P, _dev(c.w), n_modes=6, shift=shift, m=64, tol=TOL, ksp_rtol=INNER)
    assert P.options.ksp_rtol == 1e-6                                                  # restored
    P.close()
    assert r.m_done == 64 and r.converged.all() and len(r.eigenvalues) == 6 and r.modes.shape == (6, len(c.w))
    assert (np.diff(r.eigenvalues.real) <= 0.0).all()
    X = r.modes.cpu().numpy()
    assert np.abs(np.linalg.norm(X, axis=1) - 1.0).max() < 1e-13
    big = X[np.arange(6), np.abs(X).argmax(axis=1)]
    assert (big.real > 0.0).all() and np.abs(big.imag).max() < 1e-15
    got = max(SO.mode_residual(J, B, lam, x) for lam, x in zip(r.eigenvalues, X))
    emu = emulation(name, shift)
    k = emu["m_done"]
    first = np.nonzero(emu["conv"])[0][:6]
    ref = max(SO.mode_residual(J, B, emu["lam"][i], emu["V"][:k].T @ emu["Y"][:, i]) for i in first)
    print(name, shift, "true residual", got, "emulation", ref, "eigenvalues", r.eigenvalues[:3])
    assert got <= 10.0 * ref
    # the same six eigenvalues as the process's own Ritz values
    _, H, res = gpu_run(name, shift)
    lam, _, est = S.ritz_pairs(H, res.m_done, shift)
    assert np.abs(lam[est <= TOL][:6] - r.eigenvalues).max() <= 1e-6 * np.abs(r.eigenvalues).max()


# ---- 5. breakdown ----------------------------------------------------------------------------------------------------------
def test_breakdown_on_the_nine_dof_duct():
    """9 free velocity dofs: rank B <= 9, so the exact process ends at step 9 (norm ratio 1e-10 in the oracle, against at least
    0.04 for every genuine step).  An inner solve at the relative residual 1e-10 leaves an error in S v that the emulation puts
    at a ratio of about 1e-4 at that step (the residual is amplified by |(J)^-1| |b| / |S v|), so breakdown_rel has to sit
    between the two: the geometric mean of the emulation's largest step-9 ratio over 8 seeds and the smallest genuine one."""
    c = SO.case("duct322")
    J, B = c.operators()
    ratios = np.array([SO.arnoldi(J, B, c.constrained, m=9, inner_rtol=INNER, seed=seed, breakdown_rel=1e-30)[3] for seed in range(8)])
    spurious, genuine = ratios[:, 8].max(), ratios[:, :8].min()
    breakdown_rel = float(np.sqrt(spurious * genuine))
    print("emulated step-9 ratio", spurious, "smallest genuine ratio", genuine, "breakdown_rel", breakdown_rel)
    assert spurious * 10.0 < breakdown_rel < genuine / 10.0
    P = _problem(c, ksp_rtol=INNER)
    Vd, H, res = P.stability_arnoldi(_dev(c.w), shift=0.0, m=64, breakdown_rel=breakdown_rel)
    V = Vd.cpu().numpy()
    P.close()
    print("m_done", res.m_done, "reason", res.reason)
    assert res.m_done <= 9 and res.reason == 2
    assert np.isfinite(V).all() and np.isfinite(H).all()
    assert not H[res.m_done:].any() and not H[:, res.m_done:].any()
    assert not V[res.m_done:].any()
    assert SO.orthogonality(V, res.m_done) <= 1e-12
    lam, _, est = S.ritz_pairs(H, res.m_done, 0.0)
    dense = dense_spectrum("duct322")
    # an invariant space up to the inner solves' error: every pair is a dense eigenvalue to 10 x the emulated step-9 ratio
    assert np.isfinite(lam).all() and SO.nearest(dense, lam).max() <= 10.0 * spurious


# ---- 6. state --------------------------------------------------------------------------------------------------------------
def test_the_handle_is_steady_again_after_a_shifted_run():
    c = SO.case("duct633")
    P = _problem(c, ksp_rtol=1e-8)
    wd = _dev(c.w + 0.01 * np.where(c.constrained, 0.0, np.cos(np.arange(len(c.w)))))   # (not converged: a residual worth comparing)
    before = P.residual(wd).clone()
    V, H, res = P.stability_arnoldi(wd, shift=2.0, m=4)
    assert res.m_done == 4 and res.reason == 1
    assert torch.equal(P.residual(wd), before)
    P.set_time_term(1.0, 0.0, P.zeros())                                               # (allowed again: none is set)
    P.clear_time_term()
    # the assembled matrix stays J + shift B
    A = P.to_scipy()
    J2 = c.jacobian(2.0, w=wd.cpu().numpy())
    assert abs(A - J2).max() <= 1e-12 * abs(J2).max()
    P.close()


def test_an_unconverged_inner_solve_ends_the_process_quietly():
    c = SO.case("duct633")
    P = _problem(c, ksp_rtol=1e-14, ksp_max_it=1)
    wd = _dev(c.w)
    before = P.residual(wd).clone()
    V, H, res = P.stability_arnoldi(wd, shift=2.0, m=8)                                # returns SNS_OK: no exception
    print("reason", res.reason, "m_done", res.m_done)
    assert res.reason < 0 and res.m_done == 0 and res.ksp_its >= 1
    assert not H.any() and torch.isfinite(V).all() and not V[1:].any()
    assert torch.equal(P.residual(wd), before)                                         # the time term is cleared
    P.close()


def test_refusals():
    c = SO.case("duct322")
    P = _problem(c)
    wd = _dev(c.w)
    for kw in (dict(m=1), dict(m=65), dict(shift=-1.0), dict(shift=float("nan")), dict(shift=float("inf")),
               dict(breakdown_rel=0.0), dict(breakdown_rel=1.0), dict(breakdown_rel=float("nan"))):
        with pytest.raises(SnsError) as e:
            P.stability_arnoldi(wd, **kw)
        assert e.value.code == -1, kw
    P.set_time_term(1.0, 0.0, P.zeros())
    with pytest.raises(SnsError) as e:
        P.stability_arnoldi(wd, m=4)
    assert e.value.code == -3 and "time term" in str(e.value)
    P.mass_apply(wd, wd)                                                               # (the mass pass ignores a time term)
    P.clear_time_term()
    P.set_viscosity_law(0.5, 0.7)
    for call in (lambda: P.stability_arnoldi(wd, m=4), lambda: P.mass_apply(wd, wd)):
        with pytest.raises(SnsError) as e:
            call()
        assert e.value.code == -3 and "viscosity law" in str(e.value)
    P.clear_viscosity_law()
    P.close()
    # 2-D handles
    m2 = M2.dfg_2d_mesh(0.5)
    P2 = FlowProblem(m2, M2.dfg2d_bcs(m2).flatten(), reynolds=100.0)
    for call in (lambda: P2.stability_arnoldi(P2.zeros(), m=4), lambda: P2.mass_apply(P2.zeros(), P2.zeros())):
        with pytest.raises(SnsError) as e:
            call()
        assert e.value.code == -1 and str(e.value).endswith("3-D handles only")
    P2.close()
    # a handle with an owned / ghost split attached (no transport needed): SNS_E_STATE
    from stabilized_navier_stokes_flow_fenicsx_amd import partition as PT
    c6 = SO.case("duct633")
    part = PT.build_local_part(c6.mesh, c6.mask, c6.g, PT.rcb_partition(c6.mesh.points, 2), 0, 2)
    R = FlowProblem(part.mesh, (part.bc_mask, part.bc_val), part=part, group="local-only", reynolds=c6.Re)
    for call in (lambda: R.stability_arnoldi(R.zeros(), m=4), lambda: R.mass_apply(R.zeros(), R.zeros())):
        with pytest.raises(SnsError) as e:
            call()
        assert e.value.code == -3 and "communicator" in str(e.value)
    R.close()
