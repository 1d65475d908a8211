"""The fine-level aggregation by operator strength (amg_aggregation = 1) on the host, no GPU: sns_host_aggregate_strength on the
strength of the oracle's Stokes operator (restated in numpy below, what k_strength computes), the policy rule that the option
brings the aggregate-block smoother to the fine level, and mesh.tet_quality, which finds the slivers the option is for."""
import numpy as np
import pytest

THETA = 0.25                     # csrc/sns_policy.h STRENGTH_THETA


def strength(rowptr, colind, vals):
    """s_ij = || D_i^-1/2 A_ij D_j^-1/2 ||_F per block slot, D = |point diagonal|, 0 on the diagonal slot (fp32)."""
    n = len(rowptr) - 1
    V = np.asarray(vals, np.float64).reshape(-1, 4, 4)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    dslot = rows == colind
    d = np.zeros((n, 4))
    d[rows[dslot]] = np.abs(V[dslot][:, np.arange(4), np.arange(4)])
    si = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)
    S = si[rows][:, :, None] * V * si[colind][:, None, :]
    s = np.sqrt((S * S).sum(axis=(1, 2)))
    s[dslot] = 0.0
    return s.astype(np.float32)


def strong_edges(rowptr, colind, s, n_active):
    """Strong edges (i < j) of the active nodes: symmetrised max(s_ij, s_ji) >= THETA x the strongest coupling of i or of j."""
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    W = {}
    for i, j, v in zip(rows, colind, s.astype(np.float64)):
        if i != j and i < n_active and j < n_active:
            k = (min(i, j), max(i, j))
            W[k] = max(W.get(k, 0.0), v)
    mx = np.zeros(n)
    for (i, j), v in W.items():
        mx[i] = max(mx[i], v)
        mx[j] = max(mx[j], v)
    return [(i, j) for (i, j), v in W.items() if v > 0 and (v >= THETA * mx[i] or v >= THETA * mx[j])]


@pytest.fixture(scope="module")
def sliver_mesh():
    """A small jittered-cubic Delaunay channel (sliver-rich) with its oracle Stokes operator (BSR 4 x 4) and strength."""
    from oracle import cport
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B, mesh as M
    m = M.delaunay_channel_mesh(8, lattice="cubic")
    mask, g = B.channel_bcs(m, *B.two_stream_profiles(0.5)).flatten()
    rp, ci = cport.pattern(m.num_nodes, m.tets)
    vals, _ = cport.assemble("stokes", m.points, m.tets, None, 50.0, mask, g, rp, ci)
    return m, rp, ci, vals, strength(rp, ci, vals)


def canonical(agg):
    """The partition as a map node -> smallest node of its aggregate (-1 stays -1): independent of the aggregates' numbering."""
    out = np.full(len(agg), -1, np.int64)
    act = agg >= 0
    first = {}
    for i in np.nonzero(act)[0]:
        first.setdefault(int(agg[i]), int(i))
    out[act] = [first[int(a)] for a in agg[act]]
    return out


@pytest.mark.parametrize("max_agg", [8, 4])
def test_strength_aggregates_cover_fit_and_are_strongly_connected(built_lib, sliver_mesh, max_agg):
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    m, rp, ci, vals, s = sliver_mesh
    n = m.num_nodes
    n_active = n - 37                                       # the last nodes take no part (a partitioned handle's ghosts)
    agg, nc = _lib.host_aggregate_strength(rp, ci, s, n_active=n_active, max_agg=max_agg)
    assert (agg[:n_active] >= 0).all() and (agg[n_active:] == -1).all()
    assert set(np.unique(agg[:n_active])) == set(range(nc))
    size = np.bincount(agg[:n_active], minlength=nc)
    assert size.max() <= max_agg and size.min() >= 1
    assert n_active / nc > 0.6 * max_agg                    # it coarsens (8: ~6.6 nodes per aggregate on this mesh)
    # every aggregate is connected in the strong graph: union-find over the strong edges inside aggregates
    parent = np.arange(n_active)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in strong_edges(rp, ci, s, n_active):
        if agg[i] == agg[j]:
            parent[find(i)] = find(j)
    roots = np.array([find(i) for i in range(n_active)])
    for a in range(nc):
        assert len(np.unique(roots[agg[:n_active] == a])) == 1, a


def test_strength_aggregation_does_not_depend_on_the_numbering(built_lib, sliver_mesh):
    """Relabelling the nodes by a random permutation gives the same partition (the strengths of this mesh have no ties)."""
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    m, rp, ci, vals, s = sliver_mesh
    n = m.num_nodes
    off = s[np.repeat(np.arange(n), np.diff(rp)) != ci]
    assert len(np.unique(off)) > 0.45 * len(off)            # (each coupling appears twice, s_ij and s_ji)
    agg, _ = _lib.host_aggregate_strength(rp, ci, s)
    rng = np.random.default_rng(3)
    perm = rng.permutation(n)                               # new id of old node i: perm[i]
    inv = np.argsort(perm)
    rows = np.repeat(np.arange(n), np.diff(rp))
    r2, c2 = perm[rows], perm[ci]
    order = np.lexsort((c2, r2))
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(r2, minlength=n))]).astype(np.int32)
    agg2, _ = _lib.host_aggregate_strength(rp2, c2[order].astype(np.int32), s[order])
    back = agg2[perm]                                       # aggregate of old node i under the new numbering
    assert (canonical(back) == canonical(agg)).all()


def test_strength_aggregation_is_invariant_to_the_dof_scaling(built_lib, sliver_mesh):
    """A random positive scaling of the dofs, S A S, leaves the measure -- and the aggregates -- as they are: the point-diagonally
    balanced basis (a plain norm would report the 1/h of the velocity-pressure coupling, not slivers)."""
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    m, rp, ci, vals, s = sliver_mesh
    n = m.num_nodes
    rng = np.random.default_rng(11)
    sc = np.exp(rng.uniform(-3.0, 3.0, size=(n, 4)))
    rows = np.repeat(np.arange(n), np.diff(rp))
    V = vals.reshape(-1, 4, 4) * sc[rows][:, :, None] * sc[ci][:, None, :]
    s2 = strength(rp, ci, V)
    assert np.allclose(s2, s, rtol=1e-6, atol=0)
    a1, n1 = _lib.host_aggregate_strength(rp, ci, s)
    a2, n2 = _lib.host_aggregate_strength(rp, ci, s2)
    assert n1 == n2 and (a1 == a2).all()


def test_slivers_stay_together(built_lib, sliver_mesh):
    """The worst 1 % of the tets by radius ratio: the share whose four nodes fall into one aggregate is several times higher under
    the strength aggregation than under the geometric one (scripts/proto_strength_aggregation.py at 60 k nodes: 0.72 vs 0.08)."""
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib, mesh as M
    m, rp, ci, vals, s = sliver_mesh
    q, _ = M.tet_quality(m)
    worst = np.argsort(q, kind="stable")[: max(1, len(q) // 100)]
    assert q[worst].max() < 0.2

    def together(agg):
        a = agg[m.tets[worst]]
        return float(np.mean((a == a[:, :1]).all(axis=1)))

    f_s = together(_lib.host_aggregate_strength(rp, ci, s)[0])
    f_g = together(_lib.host_aggregate(rp, ci, None, 8, m.points)[0])
    print(f"  worst 1 % of {m.num_tets} tets in one aggregate: strength {f_s:.3f}, geometric {f_g:.3f}")
    assert f_s > f_g + 0.3 and f_s > 3.0 * f_g


def test_aggregate_strength_refuses_bad_arguments(built_lib, sliver_mesh):
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    m, rp, ci, vals, s = sliver_mesh
    with pytest.raises(_lib.SnsError):
        _lib.host_aggregate_strength(rp, ci, s, max_agg=9)           # beyond the 32 x 32 smoother blocks
    with pytest.raises(ValueError):
        _lib.host_aggregate_strength(rp, ci, s[:-1])


def test_policy_strength_aggregation_brings_fine_level_blocks(built_lib):
    """amg_aggregation = 1 smooths the fine level with the aggregates' blocks (the rule lives in policy::fine_blocks, read by
    plan_cycle); the default options report what they always did, and without blocks at all (amg_block_smooth = 0) there are none."""
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    T = lambda rows, **kw: [(r["kind"], r["pre"], r["post"]) for r in _lib.host_cycle_policy(rows, **kw)]
    serial = [1738576, 218044, 27436, 3800, 475]
    assert T(serial) == [(0, 1, 1), (1, 1, 3), (1, 4, 4), (1, 2, 2), (3, 0, 0)]
    assert T(serial, amg_aggregation=1) == [(1, 1, 1), (1, 1, 3), (1, 4, 4), (1, 2, 2), (3, 0, 0)]
    assert T(serial, amg_aggregation=1) == T(serial, amg_block_smooth=2)
    assert T(serial, amg_aggregation=1, amg_block_smooth=0)[0] == (0, 1, 1)
    part = [1738576, 218044, 27436, 29470, 4193, 597, 110]
    assert T(part, nranks=2, rep_level=3, rows_global_l1=218044)[0] == (0, 1, 1)
    assert T(part, nranks=2, rep_level=3, rows_global_l1=218044, amg_aggregation=1)[0] == (1, 1, 1)
    assert _lib.default_options().amg_aggregation == 0


def test_tet_quality():
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M

    def q(X):
        m = M.TetMesh(np.asarray(X, np.float64), np.array([[0, 1, 2, 3]], np.int32), np.zeros((0, 3), np.int32), np.zeros(0, np.int32))
        r, d = M.tet_quality(m)
        return float(r[0]), float(d[0])

    reg = [[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]
    r, d = q(reg)
    assert abs(r - 1.0) < 1e-12 and abs(d - np.degrees(np.arccos(1.0 / 3.0))) < 1e-9
    assert q([reg[1], reg[0], reg[2], reg[3]]) == pytest.approx((r, d), abs=1e-12)          # orientation does not matter
    r, d = q([[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1]])                                   # Kuhn tet
    assert abs(r - np.sqrt(3.0) / (1.0 + np.sqrt(2.0))) < 1e-12 and abs(d - 45.0) < 1e-9
    prev = 1.0
    for hgt in (1e-1, 1e-2, 1e-3, 1e-5):                                                     # a sliver flattening
        r, d = q([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, 0.4, hgt]])
        assert r < prev
        prev = r
    assert prev < 1e-4 and d < 0.01
    m = M.delaunay_channel_mesh(6, lattice="cubic")
    r, d = M.tet_quality(m)
    assert r.shape == d.shape == (m.num_tets,) and (r > 0).all() and (r <= 1 + 1e-12).all() and (d > 0).all() and (d < 70.6).all()
