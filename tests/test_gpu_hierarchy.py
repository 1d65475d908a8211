"""The shape of a partitioned hierarchy with a replicated tail as the symbolic build leaves it (csrc/sns_setup.hip:
build_hierarchy, build_replicated_tail), through the public Python API: three team ranks on the jittered (24, 6, 6) duct with
amg_coarse_size = 24, amg_replicate_rows = 1 << 20, amg_dense_rows = 0 -- level 0 and level 1 partitioned, level 1 the source
of the replicated copy, the copy at level 2 (the one level with more rows than the level above it: 214 after 69 / 74 / 71) and the
tail coarsened below it down to at most 24 rows (38, 9; asserted: at least one level below the copy)."""
import pytest
import torch

from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B
from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
from stabilized_navier_stokes_flow_fenicsx_amd import partition as PT
from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem, Team

pytestmark = pytest.mark.gpu
NRANKS = 3
OPTS = dict(amg_coarse_size=24, amg_replicate_rows=1 << 20, amg_dense_rows=0)


def test_replicated_tail_is_the_same_on_every_rank():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    m = M.duct_mesh((24, 6, 6), 4.0, jitter=0.1)
    mask, g = B.duct_bcs(m).flatten()
    owner = PT.rcb_partition(m.points, NRANKS)
    team = Team(NRANKS)

    def work(rank, team):
        part = PT.build_local_part(m, mask, g, owner, rank, NRANKS)
        P = FlowProblem(part.mesh, (part.bc_mask, part.bc_val), reynolds=12.0, part=part, group=team, **OPTS)
        P.jacobian(None, "stokes")
        P.pc_setup()                                                     # builds the hierarchy (collective)
        out = [(h["rows"], h["blocks"]) for h in P.hierarchy()]
        P.close()
        return out

    outs = team.run(work)
    team.close()
    hier = outs
    print("rows, blocks per rank:", hier)
    assert len({len(h) for h in hier}) == 1                              # every rank reports the same number of levels
    # the copy: the one level with more rows than the level above it (it has every rank's), at the same place on every rank
    reps = [[l for l in range(1, len(h)) if h[l][0] > h[l - 1][0]] for h in hier]
    assert all(len(r) == 1 and r == reps[0] for r in reps), reps
    rep = reps[0][0]
    assert len(hier[0]) >= rep + 2, "no level below the replicated copy: take a smaller amg_coarse_size"
    assert sum(h[0][0] for h in hier) == m.num_nodes                     # level 0: every node owned once
    assert hier[0][rep][0] == sum(h[rep - 1][0] for h in hier)           # the copy holds the source level's rows of all ranks
    for h in hier[1:]:
        assert h[rep:] == hier[0][rep:]                                  # rows and blocks from the copy down: identical everywhere
    assert all(hier[0][l + 1][0] < hier[0][l][0] for l in range(rep, len(hier[0]) - 1))
