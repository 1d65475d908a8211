"""The raw Jacobian on the host: the formula of solver.dirichlet_sensitivity and the gradient of the residual-based force, both on
the CPU oracle alone (tests/rawjac_oracle.py), and the rule rows of the request family FAMILY_RAW_JACOBIAN of csrc/sns_policy.h
through a stand-alone main (tests/rawjac_request_main.cpp).

The band rule is the one of tests/test_gpu_adjoint.py: an exact derivative must lie within 4 |D(d/2) - D(d)| / 3 + 1e-7 |D*| of
the Richardson value D* of central differences, and a band wider than 1 % of |D*| would check nothing."""
import functools
import subprocess

import numpy as np
import pytest

import ns3d_oracle as NS
import rawjac_oracle as RO
import stability_oracle as SO
from request_gate import BACKFLOW, DIM, FACTS, PART, policy_main

FD_STEP = 1e-2                                       # of the Dirichlet data (inlet velocity 1) and of the state (velocities of order 1)


@functools.lru_cache(maxsize=None)
def _duct322():
    """duct322 at its converged state: J0, the wall's weights, the two functionals (the reaction drag on the wall, which is not
    linear in w and whose gradient does not vanish on constrained dofs, and a fixed linear functional) with their gradients,
    the two directions of the data (the inlet amplitude, one interior inlet node)."""
    c = SO.case("duct322")
    m = c.mesh
    pts, tets = m.points, m.tets
    J0 = RO.raw_jacobian(pts, tets, c.w, c.Re)
    phi = np.zeros(m.num_nodes)
    phi[m.facet_nodes(m.meta["tags"]["wall"])] = 1.0
    lin = np.cos(0.7 + 1.3 * np.arange(4 * m.num_nodes))
    z = np.zeros(4 * m.num_nodes)
    z[0::4] = phi
    functionals = {"reaction drag": (lambda w: -RO.moments(pts, tets, w, c.Re, phi)[0], -(J0.T @ z)),
                   "linear": (lambda w: float(lin @ w), lin)}
    amp = np.where(c.constrained, c.g, 0.0)
    amp[3::4] = 0.0
    inlet = m.facet_nodes(m.meta["tags"]["inlet"])
    inner = [i for i in inlet if abs(pts[i, 1]) < 0.49 and abs(pts[i, 2]) < 0.49]
    bump = np.zeros(4 * m.num_nodes)
    bump[4 * inner[0]] = 1.0
    assert np.abs(amp).sum() > 0 and c.constrained[4 * inner[0]]
    return c, J0, phi, functionals, {"amplitude": amp, "bump": bump}


@pytest.mark.parametrize("direction", ["amplitude", "bump"])
@pytest.mark.parametrize("name", ["reaction drag", "linear"])
def test_dirichlet_gradient_formula_against_resolves(name, direction):
    """dJ/dg . dg by the formula grad_J[B] - J0[f,B]^T J_ff^-T grad_J[f] against the Richardson value of central differences of
    oracle Newton re-solves with the data g +- d dg."""
    c, J0, _, functionals, directions = _duct322()
    J, grad = functionals[name]
    dg = directions[direction]
    exact = float(RO.dirichlet_gradient(J0, c.mask, grad)[0] @ dg)

    def J_of(s):
        w, _ = NS.newton(c.mesh.points, c.mesh.tets, c.mask, c.g + s * dg, c.Re, c.w)
        return J(w)

    D1, D2, Dstar, band = RO.fd_band(J_of, FD_STEP)
    print(f"{name} / {direction}: exact {exact:.10e} D(d) {D1:.10e} D(d/2) {D2:.10e} D* {Dstar:.10e} band {band:.2e} = "
          f"{band / abs(Dstar):.2e} |D*|; |exact - D*| {abs(exact - Dstar):.2e}")
    assert band <= 0.01 * abs(Dstar), (band, Dstar)
    assert abs(exact - Dstar) <= band, (exact, Dstar, band)


@pytest.mark.parametrize("comp", [0, 1, 2])
def test_force_gradient_against_differences_of_the_moments(comp):
    """-J0^T (phi e_c) . dw against a central difference of the oracle's raw residual moments along a direction dw that is not
    zero on constrained dofs, at a state that violates its data."""
    c, _, phi, _, _ = _duct322()
    pts, tets = c.mesh.points, c.mesh.tets
    w = c.w + 0.05 * np.cos(1.0 + 0.37 * np.arange(len(c.w)))
    dw = np.cos(0.3 + 0.91 * np.arange(len(c.w)))
    z = np.zeros(len(w))
    z[comp::4] = phi
    exact = float(-(RO.raw_jacobian(pts, tets, w, c.Re).T @ z) @ dw)
    D1, D2, Dstar, band = RO.fd_band(lambda s: -RO.moments(pts, tets, w + s * dw, c.Re, phi)[comp], FD_STEP)
    print(f"force component {comp}: exact {exact:.10e} D(d) {D1:.10e} D(d/2) {D2:.10e} D* {Dstar:.10e} band {band:.2e} = "
          f"{band / abs(Dstar):.2e} |D*|; |exact - D*| {abs(exact - Dstar):.2e}")
    assert band <= 0.01 * abs(Dstar), (band, Dstar)
    assert abs(exact - Dstar) <= band, (exact, Dstar, band)


# ---- the request family ------------------------------------------------------------------------------------------------------------
E_ARG, E_STATE = -1, -3
FORM_STOKES, FORM_NS = 0, 1
JREQ_APPLY, JREQ_SET_DIRICHLET = 0, 1


def _expected(req, facts, form, aliased, variant):
    """The rules, transcribed: the pass asks for the NS form and distinct vectors (ARG), then for the reference's constants, no
    communicator and no backflow coefficient (STATE, in that order); the setter refuses a communicator alone.  No other fact
    -- the dimension, the time term, the law, a force, a field, facets, a traction -- matters to either."""
    if req == JREQ_APPLY:
        if form == FORM_STOKES:
            return E_ARG, "the Stokes forms are not supported"
        if form != FORM_NS:
            return E_ARG, "bad form"
        if aliased:
            return E_ARG, "x and y must not be the same vector"
        if variant:
            return E_STATE, "not with a perturbed form variant set (the pass holds the reference's constants only)"
        if facts[PART]:
            return E_STATE, "not with a communicator attached (the partitioned raw-Jacobian pass is not built)"
        if facts[BACKFLOW]:
            return E_STATE, "not with a backflow coefficient set (the backflow term's share of the raw Jacobian is not built)"
        return 0, ""
    if facts[PART]:
        return E_STATE, "not with a communicator attached (partitioned handles keep the Dirichlet values they were created with)"
    return 0, ""


def test_request_rules_over_all_nine_facts(tmp_path):
    exe = policy_main(tmp_path, "rawjac_request")
    args = [(FORM_NS, 0, 0), (FORM_STOKES, 0, 0), (7, 0, 0), (FORM_NS, 1, 0), (FORM_NS, 0, 1), (FORM_STOKES, 1, 1), (FORM_NS, 1, 1)]
    questions = [(req, facts, a) for req in (JREQ_APPLY, JREQ_SET_DIRICHLET) for facts in FACTS for a in args]
    text = "".join(" ".join(map(str, (req,) + tuple(facts) + a)) + "\n" for req, facts, a in questions)
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.returncode
    lines = run.stdout.split("\n")
    count, family, before = map(int, lines[0].split())
    assert count == 2 and family == before + 1           # two requests; the family is appended after the Hessian pass's
    rows = [ln.split("\t") for ln in lines[1:1 + len(questions)]]
    assert len(rows) == len(questions) and lines[1 + len(questions):] == [""]
    assert len(FACTS[0]) == 9 and DIM == 0
    for (req, facts, a), row in zip(questions, rows):
        code, tail = _expected(req, facts, *a)
        assert (int(row[0]), row[1]) == (code, tail), (req, facts, a, row)


def test_request_main_rejects_malformed_questions(tmp_path):
    exe = policy_main(tmp_path, "rawjac_request")
    for text in ("2 3 0 0 0 0 0 0 0 0 1 0 0\n", "0 3 0 0\n"):
        assert subprocess.run([exe], input=text, capture_output=True, text=True).returncode == 2
