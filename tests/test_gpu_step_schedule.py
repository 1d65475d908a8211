"""The fixed cost of a Newton step on a serial handle (csrc/sns_policy.h: policy::plan_step): no operator pass for a zero guess
the driver vouches for, A x of the returned iterate handed to the line search, the speculative half iteration of BiCGStab queued
in two stages, and the set-ups of a Newton sequence that take no estimates with their coarse chain on a stream of its own.  Every number a solve produces must be what the schedule before produced, which SNS_PLAIN_STEP=1 (read when a
handle is created) keeps: two handles in one process, one of each, compared as floats (array_equal: the sign of an exact zero
may differ where r0 = b replaces b - A 0)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# the jittered duct of profiles/hierarchy_build.txt: by default two levels, the blocked dense inverse last; with
# amg_dense_rows = 64 aggregate-block levels and a chain of Galerkin products
CONFIGS = {"two-level": {}, "deep": dict(amg_dense_rows=64)}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
    return FlowProblem


@pytest.fixture(scope="module")
def duct():
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B, mesh as M
    m = M.duct_mesh((16, 8, 8), 4.0, jitter=0.2)
    return m, B.duct_bcs(m).flatten()


@pytest.fixture
def pair(gpu, duct, monkeypatch):
    """make(**options) -> (plain, staged): two handles on the duct, the first created under SNS_PLAIN_STEP=1."""
    made = []

    def make(**kw):
        m, bcs = duct
        monkeypatch.setenv("SNS_PLAIN_STEP", "1")
        plain = gpu(m, bcs, reynolds=40.0, **kw)
        monkeypatch.delenv("SNS_PLAIN_STEP")
        staged = gpu(m, bcs, reynolds=40.0, **kw)
        made.extend([plain, staged])
        return plain, staged

    yield make
    for P in made:
        P.close()


def _same_result(a, b):
    assert (a.its, a.reason) == (b.its, b.reason), (a, b)
    assert a.rnorm == b.rnorm, (a.rnorm.hex(), b.rnorm.hex())


def _rhs(P, seed):
    """A right-hand side with zero Dirichlet rows, and a smooth vector of the same kind."""
    rng = np.random.default_rng(seed)
    free = torch.from_numpy(1.0 - P.bc_mask.astype(np.float64)).cuda()
    b = torch.from_numpy(rng.normal(size=P.ndof)).cuda() * free
    pts = np.asarray(P.mesh.points)
    smooth = np.repeat(np.sin(1.3 * pts[:, 0]) * np.cos(0.7 * pts[:, 1] + 0.4 * pts[:, 2]), 4)
    return b, torch.from_numpy(smooth).cuda() * free


@pytest.mark.parametrize("config", list(CONFIGS))
def test_stokes_and_newton_solves_are_what_they_were(pair, config):
    """Stokes and a full Newton solve: residual history, Newton and Krylov iteration counts, reasons, the reported true residual
    norm, every level's damping and the fields are equal; one host synchronisation per iteration on both; the deep
    configuration has aggregate-block levels, the default one ends in the blocked inverse -- asserted."""
    plain, staged = pair(**CONFIGS[config])
    out = []
    for P in (plain, staged):
        U, r = P.stokes_solve()
        c = P.counters()
        assert r.reason > 0 and c["host_syncs"] <= r.its + 4, (r, c)
        kinds = [x["kind"] for x in P.cycle()]
        w, n = P.newton_solve(U.clone())
        assert n.reason > 0 and n.its >= 2
        out.append((U.cpu().numpy(), r, w.cpu().numpy(), n, [hh["omega"] for hh in P.hierarchy()], kinds, c["host_syncs"]))
    a, b = out
    print(f"  {config}: stokes its {a[1].its} syncs {a[6]} / {b[6]}, newton its {a[3].its} ksp {a[3].ksp_its}, kinds {a[5]}")
    assert a[5] == b[5] and (len(a[5]) == 2 and a[5][-1] == 3 if config == "two-level" else len(a[5]) >= 3 and 1 in a[5][1:]), a[5]
    _same_result(a[1], b[1])
    assert np.array_equal(a[0], b[0])
    assert (a[3].its, a[3].reason, a[3].ksp_its) == (b[3].its, b[3].reason, b[3].ksp_its)
    assert a[3].fnorms == b[3].fnorms, (a[3].fnorms, b[3].fnorms)
    assert a[4] == b[4]
    assert np.array_equal(a[2], b[2])


@pytest.mark.parametrize("config", list(CONFIGS))
def test_general_path_and_the_exits_of_the_loop(pair, config):
    """Krylov solves through the C-ABI, which cannot vouch for its guess: a non-zero guess, a zero vector of the caller's, two
    solves in a row on one handle (a hand-off left by an abandoned head would show in the second); a solve that ends at
    ksp_max_it = 3; one that converges in its first iteration (ksp_rtol 0.5 under AMG, its == 1 asserted); and without a
    preconditioner the right-hand side A times a smooth vector."""
    plain, staged = pair(**CONFIGS[config])
    b, smooth = _rhs(plain, 5)
    out = []
    for P in (plain, staged):
        got = []
        P.jacobian(None, "stokes")
        x0 = 0.1 * smooth
        for guess in (x0, torch.zeros_like(b), None, x0):
            x, r = P.krylov_solve(b, guess)
            c = P.counters()
            assert r.reason > 0 and c["host_syncs"] <= r.its + 4, (r, c)
            got.append((x.cpu().numpy(), r))
        P.set_options(ksp_max_it=3)
        x, r = P.krylov_solve(b)
        assert r.reason < 0 and r.its == 3, r
        got.append((x.cpu().numpy(), r))
        x, r = P.krylov_solve(b, x0)                          # (again after the exit that queued no speculation)
        got.append((x.cpu().numpy(), r))
        P.set_options(ksp_max_it=1000, ksp_rtol=0.5)
        x, r = P.krylov_solve(b)
        assert r.reason > 0 and r.its == 1, r
        got.append((x.cpu().numpy(), r))
        x, r = P.krylov_solve(b)
        got.append((x.cpu().numpy(), r))
        P.set_options(ksp_rtol=1e-8, pc_type="none", ksp_max_it=400)
        x, r = P.krylov_solve(P.spmv(smooth))
        got.append((x.cpu().numpy(), r))
        P.set_options(ksp_rtol=0.5)
        x, r = P.krylov_solve(P.spmv(smooth))
        assert r.reason > 0 and r.its <= 2, r
        got.append((x.cpu().numpy(), r))
        out.append(got)
    for k, ((xa, ra), (xb, rb)) in enumerate(zip(*out)):
        print(f"  {config} solve {k}: its {ra.its} reason {ra.reason} rnorm {ra.rnorm:.6e}")
        _same_result(ra, rb)
        assert np.array_equal(xa, xb), k


def test_other_methods_leave_the_slope_to_the_driver(pair):
    """The methods that ignore the request for A x (FGMRES, TFQMR): the Newton driver applies the operator itself, as before."""
    for ksp in ("fgmres", "tfqmr"):
        plain, staged = pair(ksp_type=ksp)
        out = []
        for P in (plain, staged):
            U, r = P.stokes_solve()
            w, n = P.newton_solve(U.clone())
            assert r.reason > 0 and n.reason > 0
            out.append((U.cpu().numpy(), r, w.cpu().numpy(), n))
        a, b = out
        _same_result(a[1], b[1])
        assert a[3].fnorms == b[3].fnorms and a[3].ksp_its == b[3].ksp_its
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
