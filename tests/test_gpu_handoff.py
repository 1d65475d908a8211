"""The hand-offs between the kernels of a solve (csrc/sns_policy.h: policy::Handoff) on the device: the window form of the
partitioned cycle with the puts carried by the kernels that produce a vector against the same cycle with separate put launches,
under the three Krylov methods -- they promise (BiCGStab) or do not promise (FGMRES, TFQMR) the operator application that takes
the put of the preconditioner's result, and TFQMR ends on a pc_apply no operator follows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CELLS, LENGTH, REPLICATE_ROWS = (16, 8, 8), 4.0, 120


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
    return FlowProblem


def _team_stokes(gpu, ksp_type):
    """Per rank (Stokes field, result, cycle, rows per level, counters) of the duct over an in-process team of 2."""
    from stabilized_navier_stokes_flow_fenicsx_amd import partition as PT
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import Team
    team = Team(2)

    def work(rank, team):
        P = gpu.from_part(PT.duct_slab_part(CELLS, LENGTH, rank, 2), group=team, reynolds=40.0, halo_windows=1, amg_exact_sweeps=1,
                          amg_replicate_rows=REPLICATE_ROWS, ksp_type=ksp_type)
        U, r = P.stokes_solve()
        out = (U.cpu().numpy()[:4 * P.n_owned], r, [(x["kind"], x["pre"], x["post"]) for x in P.cycle()],
               [hh["rows"] for hh in P.hierarchy()], P.counters(), P.comm_info()["transport"])
        P.close()
        return out

    outs = team.run(work)
    team.close()
    return outs


@pytest.mark.parametrize("ksp_type", ["bicgstab", "fgmres", "tfqmr"])
def test_carried_puts_change_nothing_under_any_krylov_method(gpu, ksp_type, monkeypatch):
    """Stokes on the smallest duct whose 2-rank hierarchy has the fine level and a PARTITIONED aggregate-block level 1 in the
    window form (1 + 4 exact sweeps) above a replicated tail -- asserted, so that a mesh taking another path fails: with the puts
    carried by the producing kernels and with SNS_NO_CARRIED_PUT (the same stores by a separate launch) the fields agree bitwise
    and the iterations and the exchange counter are equal; every solve converges."""
    res = {}
    for name in ("carried", "separate"):
        if name == "separate":
            monkeypatch.setenv("SNS_NO_CARRIED_PUT", "1")
        else:
            monkeypatch.delenv("SNS_NO_CARRIED_PUT", raising=False)
        res[name] = _team_stokes(gpu, ksp_type)
    for rank, (a, b) in enumerate(zip(res["carried"], res["separate"])):
        cyc, rows = a[2], a[3]
        print(f"  {ksp_type} rank {rank}: its {a[1].its} / {b[1].its}, exchanges {a[4]['exchanges']} / {b[4]['exchanges']}, "
              f"cycle {cyc}, rows {rows}")
        # the precondition: a window transport; aggregate blocks on the fine level (its window form) and on level 1, which runs the
        # exact sweeps' 1 + 4 (policy::pre_post_sweeps: only a partitioned level in the window form does); the replicated tail --
        # the first level with more rows than the one above -- from level 3, so that level 1 is cycled and partitioned
        assert a[5] == "team" and cyc == b[2] and rows == b[3]
        rep = next((l for l in range(1, len(rows)) if rows[l] > rows[l - 1]), 0)
        assert cyc[0][0] == 1 and cyc[1] == (1, 1, 4) and rep == 3, (cyc, rows)
        assert a[1].reason > 0 and b[1].reason > 0
        assert a[1].its == b[1].its and a[4]["exchanges"] == b[4]["exchanges"] and a[4]["exchanges"] > 0
        assert np.array_equal(a[0], b[0])
