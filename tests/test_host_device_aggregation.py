"""The device form of the aggregation by operator strength (amg_aggregation = 2) pinned on the host, no GPU: a numpy restatement of
the round-based locally-dominant matching and of the parallel leftover rule that csrc/sns_aggregate.hip runs, against the serial
greedy matcher of amg_aggregation = 1 (sns_host_aggregate_strength) -- the maps must be identical, not merely similar -- and the
policy rule that value 2 brings the fine-level aggregate blocks as value 1 does."""
import numpy as np
import pytest

from test_host_strength_aggregation import THETA, sliver_mesh  # noqa: F401  (the fixture)


def strong_graph(rp, ci, s, n_active):
    """Directed strong slots (i, j, w) of the active nodes, both directions: w = max(s_ij, s_ji) in fp64, strong when
    w > 0 and w >= THETA x smax of i or of j (smax over active off-diagonal neighbours)."""
    n = len(rp) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    col = ci.astype(np.int64)
    key = rows * n + col
    tkey = col * n + rows
    t = np.minimum(np.searchsorted(key, tkey), len(key) - 1)
    sji = np.where(key[t] == tkey, s[t].astype(np.float64), 0.0)
    w = np.maximum(s.astype(np.float64), sji)
    act = (rows < n_active) & (col < n_active) & (rows != col)
    smax = np.zeros(n)
    np.maximum.at(smax, rows[act], w[act])
    strong = act & (w > 0) & ((w >= THETA * smax[rows]) | (w >= THETA * smax[col]))
    return rows[strong], col[strong], w[strong]


def contract(si, sj, sw, of):
    """Directed edges between clusters (a, b, W): W = the fp64 sum of the member couplings (exact for these weights)."""
    a, b = of[si], of[sj]
    keep = a != b
    a, b, w = a[keep], b[keep], sw[keep]
    m = int(of.max()) + 1 if len(of) else 1
    u, inv = np.unique(a * m + b, return_inverse=True)
    W = np.zeros(len(u))
    np.add.at(W, inv, w)
    return u // m, u % m, W


def best_per_source(a, b, W, ok, n):
    """Each source's best eligible edge by the matcher's strict order: weight descending, then (min id, max id) ascending -- for a
    fixed source that is the smaller other end.  -1: none."""
    best = np.full(n, -1, np.int64)
    a, b, W = a[ok], b[ok], W[ok]
    if len(a) == 0:
        return best, a, b, W
    order = np.lexsort((b, -W, a))
    a, b, W = a[order], b[order], W[order]
    first = np.ones(len(a), bool)
    first[1:] = a[1:] != a[:-1]
    best[a[first]] = b[first]
    return best, a, b, W


def device_aggregation(rp, ci, s, n_active, max_agg):
    """(agg, nc) as the device builds them: log2(max_agg) pairwise rounds of locally-dominant matching, then the leftover singles'
    b-matching by the rule 'best pending edge of the single, fewer than room pending edges at the cluster heavier'."""
    n = len(rp) - 1
    si, sj, sw = strong_graph(rp, ci, s, n_active)
    of = np.arange(n_active, dtype=np.int64)
    size = np.ones(n_active, np.int64)
    rnd = 1
    while (1 << rnd) <= max_agg:
        ncl = len(size)
        a, b, W = contract(si, sj, sw, of)
        partner = np.full(ncl, -1, np.int64)
        for step in range(ncl + 1):
            ok = (partner[a] < 0) & (partner[b] < 0) & (size[a] + size[b] <= max_agg)
            best, *_ = best_per_source(a, b, W, ok, ncl)
            if not (best >= 0).any():
                break
            c = np.nonzero(best >= 0)[0]
            mutual = c[best[best[c]] == c]
            assert len(mutual) > 0, "a matching step without progress"
            partner[mutual] = best[mutual]
        lead = (partner < 0) | (np.arange(ncl) < partner)
        newid = np.cumsum(lead) - 1
        newid[~lead] = newid[partner[~lead]]
        nsize = np.zeros(int(lead.sum()), np.int64)
        np.add.at(nsize, newid, size)
        of, size = newid[of], nsize
        rnd += 1
    ncl = len(size)
    a, b, W = contract(si, sj, sw, of)
    target = np.full(ncl, -1, np.int64)
    fill = np.zeros(ncl, np.int64)
    for step in range(ncl + 1):
        room = max_agg - size - fill
        pend = (size[a] == 1) & (target[a] < 0) & (size[b] >= 2) & (room[b] > 0)
        best, pa, pb, pw = best_per_source(a, b, W, pend, ncl)
        if not (best >= 0).any():
            break
        acc = []
        for x in np.nonzero(best >= 0)[0]:
            c = best[x]
            wx = pw[(pa == x) & (pb == c)][0]
            at = pb == c
            heavier = np.count_nonzero((pw[at] > wx) | ((pw[at] == wx) & (pa[at] < x)))
            if heavier < room[c]:
                acc.append((x, c))
        assert acc, "a leftover step without progress"
        for x, c in acc:
            target[x] = c
            fill[c] += 1
    keep = target < 0
    nid = np.cumsum(keep) - 1
    nid[~keep] = nid[target[~keep]]
    agg = np.full(n, -1, np.int32)
    agg[:n_active] = nid[of]
    return agg, int(keep.sum())


@pytest.mark.parametrize("max_agg", [2, 3, 4, 6, 8])
def test_dominant_matching_restatement_equals_the_host_matcher(built_lib, sliver_mesh, max_agg):
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    m, rp, ci, vals, s = sliver_mesh
    n = m.num_nodes
    for n_active in (n, n - 37):
        want, nc_w = _lib.host_aggregate_strength(rp, ci, s, n_active=n_active, max_agg=max_agg)
        got, nc_g = device_aggregation(rp, ci, s, n_active, max_agg)
        assert nc_g == nc_w and (got == want).all(), (max_agg, n_active)


def test_dominant_matching_restatement_with_ties(built_lib, sliver_mesh):
    """Every strength rounded to 1/4 (many exactly tied weights, as on a structured mesh): the id tie-break decides."""
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    m, rp, ci, vals, s = sliver_mesh
    q = (np.round(s * 4.0) / 4.0).astype(np.float32)
    for max_agg in (3, 8):
        want, nc_w = _lib.host_aggregate_strength(rp, ci, q, max_agg=max_agg)
        got, nc_g = device_aggregation(rp, ci, q, m.num_nodes, max_agg)
        assert nc_g == nc_w and (got == want).all(), max_agg


def test_policy_device_aggregation_is_planned_as_the_host_one(built_lib):
    """amg_aggregation = 2 builds the same aggregates as 1, so it plans the same cycle: the fine-level aggregate blocks."""
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    T = lambda rows, **kw: [(r["kind"], r["pre"], r["post"]) for r in _lib.host_cycle_policy(rows, **kw)]
    serial = [1738576, 218044, 27436, 3800, 475]
    assert T(serial, amg_aggregation=2) == T(serial, amg_aggregation=1)
    assert T(serial, amg_aggregation=2)[0] == (1, 1, 1)
    assert T(serial, amg_aggregation=2, amg_block_smooth=0)[0] == (0, 1, 1)
    part = [1738576, 218044, 27436, 29470, 4193, 597, 110]
    assert T(part, nranks=2, rep_level=3, rows_global_l1=218044, amg_aggregation=2)[0] == (1, 1, 1)
