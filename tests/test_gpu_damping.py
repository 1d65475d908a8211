"""The damping state of the AMG smoothers over the life of a handle (csrc/sns_damping.hip: decide at a set-up, back off after a
failed solve, reset at an options call), through the public Python API only: when a set-up takes the levels' spectral estimates
again and when it keeps them, and that whatever path a handle took to an operator, a set-up that estimates leaves the dampings
a new handle given only that operator gets -- bit for bit (the estimators' reductions are fixed-order).  The retry itself is
tests/test_gpu_parity.py::test_damping_backoff_rescues_a_failed_linear_solve's.

The mesh is duct_mesh((6, 3, 3), 4.0, jitter=0.2): 112 nodes, the smallest jittered duct that gives three levels.  With
amg_dense_rows = 0 and amg_coarse_size = 8 the hierarchy has 112 / 32 / 6 rows (asserted: at least three levels): the fine level
runs 1 + 1 nodal sweeps per cycle, level 1 runs 1 + 3 aggregate-block sweeps (it takes the Ritz limit and the growth check:
its damping moves between 0.13 and 0.73 over the tests, 0.72 = 0.8 x 0.9 after one trial of the growth check among them), the
last is solved directly.  The states are the Stokes solution scaled by 0.5 ... 2.1: the convection of the Jacobian, and with
it the levels' spectra, moves from one to the next."""
import pytest
import torch

from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B
from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem

pytestmark = pytest.mark.gpu
RE, RE2 = 50.0, 80.0
OPTS = dict(amg_dense_rows=0, amg_coarse_size=8)


def _omegas(P):
    return tuple(L["omega"] for L in P.hierarchy())


def _hex(om):
    return " ".join(float(w).hex() for w in om)


@pytest.fixture(scope="module")
def case():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    m = M.duct_mesh((6, 3, 3), 4.0, jitter=0.2)
    bcs = B.duct_bcs(m).flatten()
    P = FlowProblem(m, bcs, reynolds=RE, **OPTS)
    U, res = P.stokes_solve()
    assert res.reason > 0
    hier, cyc = P.hierarchy(), P.cycle()
    P.close()
    print("levels", [(L["rows"], c["kind"], c["pre"], c["post"]) for L, c in zip(hier, cyc)])
    assert len(hier) >= 3 and cyc[1]["pre"] + cyc[1]["post"] >= 3, "take the next mesh size up"
    return dict(m=m, bcs=bcs, U=U, states=[U * (0.5 + 0.2 * k) for k in range(9)])


def _fresh(c, w, *, transposed=False, **opts):
    """The dampings of a new handle whose first set-up is on J(w) (or its transpose) under the options."""
    P = FlowProblem(c["m"], c["bcs"], **{**dict(reynolds=RE), **OPTS, **opts})
    P.jacobian(w, "ns")
    if transposed:
        P.transpose_operator()
    P.pc_setup()
    om, factor = _omegas(P), P.counters()["damping_factor"]
    P.close()
    assert factor == 1.0
    return om


def test_estimates_are_taken_every_fourth_setup_and_for_a_new_operator(case):
    c = case
    P = FlowProblem(c["m"], c["bcs"], reynolds=RE, **OPTS)
    U, res = P.stokes_solve()                                            # the handle's first set-up
    assert res.reason > 0
    om = [_omegas(P)]
    for k, w in enumerate(c["states"], 1):                               # set-ups 1 .. 9 after it, one operator key throughout
        P.jacobian(w, "ns")
        P.pc_setup()
        om.append(_omegas(P))
        print(f"set-up {k}: {_hex(om[-1])}")
    # the first Jacobian is another operator than the Stokes one; then the cadence alone: the fourth and the eighth
    for k in range(1, 10):
        if k in (1, 4, 8):
            assert om[k] != om[k - 1], k
        else:
            assert om[k] == om[k - 1], k
    # another Reynolds number alone: the very next set-up estimates, whatever the count (10 here)
    P.set_options(reynolds=RE2)
    P.jacobian(c["states"][2], "ns")
    P.pc_setup()
    got, want = _omegas(P), _fresh(c, c["states"][2], reynolds=RE2)
    print(f"Re {RE2}: {_hex(got)} / fresh {_hex(want)}")
    assert got == want and got != om[9]
    assert P.counters()["damping_factor"] == 1.0
    P.close()


def test_a_walked_handle_estimates_what_a_fresh_handle_does(case):
    c = case
    s = c["states"]
    P = FlowProblem(c["m"], c["bcs"], reynolds=RE, **OPTS)
    seen = []

    def setup(name, want):
        """One set-up of the walked handle; `want`: the fresh handle's dampings where this set-up estimates, else None (kept)."""
        P.pc_setup()
        got = _omegas(P)
        print(f"{name:22s} {_hex(got)}" + (f" / fresh {_hex(want)}" if want else " (kept)"))
        assert got == (want if want else seen[-1]), name
        seen.append(got)

    P.jacobian(s[0], "ns")
    setup("first", _fresh(c, s[0]))                                      # count 0
    P.jacobian(s[4], "ns")
    setup("same key, count 1", None)
    assert seen[-1] != _fresh(c, s[4])                                   # (keeping them shows: J(s[4]) has other dampings of its own)
    P.set_options(amg_omega=0.7)
    setup("amg_omega, count 2", _fresh(c, s[4], amg_omega=0.7))
    P.set_options(reynolds=RE2)
    P.jacobian(s[6], "ns")
    setup("Reynolds, count 3", _fresh(c, s[6], amg_omega=0.7, reynolds=RE2))
    P.jacobian(s[1], "ns")
    setup("cadence, count 4", _fresh(c, s[1], amg_omega=0.7, reynolds=RE2))
    P.transpose_operator()
    setup("transpose, count 5", _fresh(c, s[1], amg_omega=0.7, reynolds=RE2, transposed=True))
    assert len(set(seen)) >= 4, seen                                     # the walk has teeth: a stale estimate would show
    assert P.counters()["damping_factor"] == 1.0
    P.close()


def test_an_options_call_resets_the_estimates(case):
    c = case
    s = c["states"]
    P = FlowProblem(c["m"], c["bcs"], reynolds=RE, **OPTS)
    factors = []
    P.jacobian(s[8], "ns")
    P.pc_setup()
    first = _omegas(P)
    factors.append(P.counters()["damping_factor"])
    P.jacobian(s[0], "ns")
    P.pc_setup()                                                         # count 1: keeps the estimates of J(s[8])
    kept = _omegas(P)
    factors.append(P.counters()["damping_factor"])
    P.set_options(amg_omega=0.75)
    factors.append(P.counters()["damping_factor"])
    P.pc_setup()                                                         # count 2: the options call alone makes it estimate
    got, want = _omegas(P), _fresh(c, s[0], amg_omega=0.75)
    factors.append(P.counters()["damping_factor"])
    P.close()
    print(f"first {_hex(first)}\nkept  {_hex(kept)}\nreset {_hex(got)} / fresh {_hex(want)}")
    assert kept == first
    assert got == want and got != kept
    assert factors == [1.0] * 4
