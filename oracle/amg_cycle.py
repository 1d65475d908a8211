"""CPU restatement (numpy / scipy) of the AMG V-cycle libsns applies as preconditioner -- TEST INFRASTRUCTURE like the rest of
oracle/: imported by tests/ only, never by the product (the product path is the HIP kernels of csrc/; the reference itself
preconditions with PETSc's ILU(0), NavierStokesChannelFlow.py:274-283, so there is no reference code to follow here: this file
restates the PRODUCT's own algorithm, DESIGN.md section 4, so that the GPU cycle can be checked operator-for-operator).

What is restated (single GPU):
  * hierarchy: greedy aggregates of <= 8 nodes from the product's host utility (sns_host_aggregate -- symbolic, CPU), 4 dofs per
    aggregate, Galerkin operators P^T A P with the level-0 Dirichlet dofs excluded from the transfer and a unit diagonal on
    empty coarse dofs; coarsening stops at the first level >= 1 with <= max(coarse_nodes, dense_rows) rows, which is solved exactly;
  * smoothers: damped nodal-block Jacobi x <- x + w D^-1 (b - A x) (D = the 4 x 4 diagonal blocks), or -- on the levels listed
    in `block_levels` -- aggregate-block Jacobi with B = the diagonal blocks of A over the aggregates that form the next level;
  * cycle: first pre-sweep from the zero guess (w S b), nu_pre - 1 further sweeps, residual, restriction P^T, recursive coarse
    solve, correction, nu_post sweeps.  Damping per level is an INPUT (the GPU's own values, FlowProblem.hierarchy()), because
    the estimate is not part of the operator being compared.

What the GPU applies (build(..., fmt=0 | 1 | 2), the level data of amg_f32_matrix = fmt; fmt=None, the default, is the all-fp64
cycle above, unchanged): every rule below is restated from the kernels, file:line under csrc/ of the package.
  * fmt 1: fp32 copies of A (k_cvt_f32, sns_setup.hip:1017-1022), of D^-1 (dinv32, :981-983) and of the aggregate-block inverses
    (k_binv<1>, sns_block.hip:606-611); M = A P summed in fp64, then rounded once (k_ap_cvt32, sns_kernels.hip:1873-1894);
  * fmt 2: A and M = A P as fp16 with one fp32 scale per dof row (k_lp_copies16, q16_rows: one rounding f64 -> f16 as the
    kernel is compiled), D^-1 fp32, the block inverses fp16 with k_binv<2>'s own scale rule (q16_binv);
  * fmt 0: the fp64 operator and D^-1 (no aggregate blocks, no fused passes: sns_policy.h:53, sns_ctx.h:750-753);
  * the coarsest level, in EVERY format: <= max(coarse_nodes, 40) nodes the one-workgroup fp64 inverse, up to dense_rows nodes the
    blocked Gauss-Jordan inverse applied as its fp32 copy (alloc_coarsest_solver, sns_setup.hip:197-213; k_dense_to_f32 :1123,
    k_dense_matvec32 sns_cycle.hip:280-283), a larger one 1 + 8 sweeps whose FIRST sweep takes the fp64 D^-1 (k_bjacobi,
    sns_cycle.hip:289-293) and the others the level's copies;
  * fused_post: the first post-sweep is z = (x1 + P xc) + w S (r1 - M_q xc), M_q = Q(A P) with M's OWN row scales -- not Q(A) P
    (k_post_lp sns_kernels.hip:1729-1730, k_bpost; sns_cycle.hip:397-445).  The fused restriction (k_resid_restrict) is the
    same arithmetic as residual + restriction + the next level's first sweep w S_c (P^T r) and needs no form of its own.
  * pts: aggregation with node coordinates (sns_setup.hip:435-436), coarse levels with the member-mean centroids (:528-538).
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from stabilized_navier_stokes_flow_fenicsx_amd import _lib      # host-only symbolic utility (no GPU needed)


class Level:
    pass


def _row_max(X):
    X = X.tocsr()
    m = np.zeros(X.shape[0])
    nz = np.diff(X.indptr) > 0
    m[nz] = np.maximum.reduceat(np.abs(X.data), X.indptr[:-1][nz]) if X.nnz else 0.0
    return m, np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))


def q16_rows(X):
    """fp16 copy with one fp32 scale per dof row, as k_lp_copies16 writes it (csrc/sns_kernels.hip:1936-1952 register path,
    :1955-1971 loop path, M :1995-2027 / :2037-2056): s = f32(max |a| over the row), h = f16(a * (1 / f64(s))), applied as s * h
    (k_spmv_lp :1696).  An all-zero row: s = 0, h = 0.  Returns (Xq, s, h) with Xq.data = s * h (exact: 24 x 11 significant bits)
    and h in Xq's entry order.
    ONE rounding f64 -> f16: the source reads (_Float16)(float)(a * inv), but hipcc folds the two conversions into one fptrunc
    double -> half (the gfx950 code of k_lp_copies16 has no v_cvt_f16_f32; the conversion is the integer expansion of the
    correctly rounded f64 -> f16).  The two differ where a * inv lies within 2^-30 of an fp16 tie -- 36 of the 1.06 M entries of
    the jittered 40 x 10 x 10 duct's Jacobian --, and the GPU matches the single rounding (pc_apply to 3e-16, through fp32: 1.5e-5)."""
    Xq = sp.csr_matrix(X, dtype=np.float64, copy=True)
    Xq.sort_indices()
    m, rows = _row_max(Xq)
    s = m.astype(np.float32).astype(np.float64)
    with np.errstate(divide="ignore"):
        inv = np.where(m > 0.0, 1.0 / s, 0.0)
    h = (Xq.data * inv[rows]).astype(np.float16)
    Xq.data = s[rows] * h.astype(np.float64)
    return Xq, s, h


def q16_binv(X):
    """fp16 copy of the aggregate-block inverses as k_binv<2> writes it (csrc/sns_block.hip:613-625): the row's largest |entry| mx in
    fp64, h = f16(b * (1 / mx)) with the fp64 reciprocal of mx itself, but f32(mx) stored as the scale -- a different rule from
    q16_rows where mx is not an fp32 number.  One rounding f64 -> f16 as in q16_rows.  Returns (Xq, s, h) like q16_rows."""
    Xq = sp.csr_matrix(X, dtype=np.float64, copy=True)
    Xq.sort_indices()
    m, rows = _row_max(Xq)
    with np.errstate(divide="ignore"):
        inv = np.where(m > 0.0, 1.0 / m, 0.0)
    s = m.astype(np.float32).astype(np.float64)
    h = (Xq.data * inv[rows]).astype(np.float16)
    Xq.data = s[rows] * h.astype(np.float64)
    return Xq, s, h


def f32(X):
    """fp32 copy (k_cvt_f32, csrc/sns_kernels.hip:2065-2068), back in fp64 for the arithmetic (which stays fp64 on the GPU)"""
    Xq = sp.csr_matrix(X, dtype=np.float64, copy=True)
    Xq.data = Xq.data.astype(np.float32).astype(np.float64)
    return Xq


def quantize(L, fmt, block, fused_post):
    """the level data the GPU's passes read under amg_f32_matrix = fmt (module docstring): L.Aq (sweeps, residual), L.Sq (sweeps,
    the first sweep included), L.S1 (the first sweep of a sweeps-only last level), L.Mq (fused post-sweep, or None)"""
    L.Mq = None
    L.S1 = L.S                                          # a sweeps-only last level's first sweep: k_bjacobi, fp64 D^-1
    if fmt is None or fmt == 0:
        L.Aq, L.Sq = L.A, L.S
        return
    if fmt == 1:
        L.Aq, L.Sq = f32(L.A), f32(L.S)
    else:
        L.Aq = q16_rows(L.A)[0]
        L.Sq = q16_binv(L.S)[0] if block else f32(L.S)
    if L.P is not None and fused_post:
        M = (L.A @ L.P).tocsr()                         # the Dirichlet dofs' columns of A are zero but for the unit diagonal
        L.Mq = f32(M) if fmt == 1 else q16_rows(M)[0]


def nodal_block_inverse(A, n):
    Ab = A.tobsr((4, 4))
    Ab.sort_indices()
    rows = np.repeat(np.arange(n), np.diff(Ab.indptr))
    sel = Ab.indices == rows
    D = np.zeros((n, 4, 4))
    D[rows[sel]] = Ab.data[sel]
    return sp.bsr_matrix((np.linalg.inv(D), np.arange(n), np.arange(n + 1)), shape=(4 * n, 4 * n)).tocsr()


def smoother_blocks(agg, nc):
    """the product's smoother blocks: the aggregates, one of more than 8 nodes split into chunks of 8 in ascending node order"""
    blk = np.empty_like(agg)
    nb = 0
    order = np.argsort(agg, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(agg, minlength=nc))])
    for I in range(nc):
        mem = order[ptr[I]:ptr[I + 1]]
        for k in range(0, len(mem), 8):
            blk[mem[k:k + 8]] = nb
            nb += 1
    return blk, nb


def aggregate_block_inverse(A, agg, nc):
    """blockdiag over the smoother blocks (aggregates, see smoother_blocks) of A, inverted, in the original numbering"""
    agg, nc = smoother_blocks(agg, nc)
    order = np.argsort(agg, kind="stable")
    dofs = (4 * order[:, None] + np.arange(4)[None]).ravel()
    Ap = A[dofs][:, dofs].tocsr()
    ptr = np.concatenate([[0], np.cumsum(4 * np.bincount(agg, minlength=nc))])
    blocks = [np.linalg.inv(Ap[ptr[i]:ptr[i + 1], ptr[i]:ptr[i + 1]].toarray()) for i in range(nc)]
    Bp = sp.block_diag(blocks, format="csr")
    Pm = sp.csr_matrix((np.ones(len(dofs)), (np.arange(len(dofs)), dofs)), shape=A.shape)
    return (Pm.T @ Bp @ Pm).tocsr()


def node_graph(A):
    """structural node graph (n x n, ones) of a matrix with 4 dofs per node: one entry per stored 4 x 4 block"""
    Ab = A.tobsr((4, 4))
    Ab.sort_indices()
    n = A.shape[0] // 4
    return sp.csr_matrix((np.ones(len(Ab.indices)), Ab.indices.copy(), Ab.indptr.copy()), shape=(n, n))


def build(A, free, coarse_nodes=32, dense_rows=512, agg_size=8, max_levels=12, block_levels=(), graph=None, pts=None, fmt=None,
          fused_post=False):
    """levels of the product's serial hierarchy for the fine operator A (scipy sparse, 4 dofs per node) and its free-dof mask.
    `graph`: the STRUCTURAL node graph of A (the BSR pattern the product assembles into, explicit zero blocks included; default:
    A's stored blocks).  The product aggregates on patterns, not values: a coarse pattern is the image of the fine one, whatever
    cancels numerically (Dirichlet rows / columns are zeroed in the values but stay in the pattern).
    `pts`: the node coordinates (n, 3): aggregation as the product runs it with them (sns_host_aggregate_pts: strong-only filter on
    anisotropic clouds, the pairwise aggregation where it wins), each level's choice in L.which (0 greedy, 1 pairwise); the coarse
    levels aggregate with the member-mean centroids (csrc/sns_setup.hip:528-538).  None: the pattern alone (L.which = None).
    `fmt` / `fused_post`: the level data and the fused post-sweep of amg_f32_matrix = fmt / amg_fused_post (module docstring);
    fmt=None: everything fp64.  The last level's L.kind is the GPU's (FlowProblem.cycle()): 2 the one-workgroup fp64 inverse, 3 the
    blocked Gauss-Jordan inverse -- applied as its fp32 copy in EVERY format fmt (with fmt=None: exact) --, 4 sweeps only."""
    levels = []
    stop = max(coarse_nodes, min(dense_rows, 4096))
    G = node_graph(A) if graph is None else graph.tocsr()
    X = None if pts is None else np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    while True:
        L = Level()
        n = A.shape[0] // 4
        L.A, L.n = A.tocsr(), n
        L.S = nodal_block_inverse(L.A, n)
        L.P = None
        L.which = None
        L.block = False
        levels.append(L)
        l = len(levels) - 1
        if n <= coarse_nodes or (l >= 1 and n <= stop) or len(levels) >= max_levels:
            break
        G.sort_indices()
        if X is None:
            agg, nc = _lib.host_aggregate(G.indptr.astype(np.int32), G.indices.astype(np.int32), None, agg_size)
        else:
            agg, nc, L.which = _lib.host_aggregate(G.indptr.astype(np.int32), G.indices.astype(np.int32), None, agg_size, pts=X)
        if nc >= n or nc == 0:
            L.which = None
            break
        T = sp.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, nc))
        Gc = (T.T @ G @ T).tocsr()                   # all-positive data: nothing cancels, the pattern is the image of G
        Gc.data[:] = 1.0
        dof = np.arange(4 * n)
        col = 4 * agg[dof // 4].astype(np.int64) + dof % 4
        w = np.ones(4 * n) if free is None else np.asarray(free, dtype=np.float64)
        L.P = sp.csr_matrix((w, (dof, col)), shape=(4 * n, 4 * nc))
        Ac = (L.P.T @ L.A @ L.P).tocsr()
        empty = np.asarray(abs(Ac).sum(axis=1)).ravel() == 0
        if empty.any():
            Ac = Ac + sp.diags(empty.astype(np.float64))
        if l in block_levels:
            L.S = aggregate_block_inverse(L.A, agg, nc)
            L.block = True
        if X is not None:
            X = (T.T @ X) / np.bincount(agg, minlength=nc)[:, None]
        A, free, G = Ac, None, Gc
    last = levels[-1]
    last.exact = last.n <= max(stop, 40) and len(levels) > 1
    last.kind = 4 if not last.exact else (2 if last.n <= max(coarse_nodes, 40) else 3)
    if last.exact:
        if fmt is not None and last.kind == 3:
            last.X32 = np.linalg.inv(last.A.toarray()).astype(np.float32).astype(np.float64)
        else:
            last.lu = spla.splu(sp.csc_matrix(last.A))
    for L in levels:
        quantize(L, fmt, L.block, fused_post)
    return levels


def cycle(levels, l, b, sweeps, omega):
    """x ~ A_l^-1 b.  sweeps[l] = (nu_pre, nu_post), omega[l] = damping of level l.  With the level data of build(fmt=None) the
    all-fp64 cycle; otherwise the passes read what the GPU's read (L.Aq, L.Sq, L.S1, L.Mq, L.X32)."""
    L = levels[l]
    om = omega[l]
    A, S = L.Aq, L.Sq
    if L.P is None:
        if L.exact:
            return L.X32 @ b if hasattr(L, "X32") else L.lu.solve(b)
        x = om * (L.S1 @ b)                      # a last level too large for the direct solve: 1 + 8 sweeps
        for _ in range(8):
            x = x + om * (S @ (b - A @ x))
        return x
    nu_pre, nu_post = sweeps[l]
    x = om * (S @ b)
    for _ in range(nu_pre - 1):
        x = x + om * (S @ (b - A @ x))
    r = b - A @ x
    xc = cycle(levels, l + 1, L.P.T @ r, sweeps, omega)
    first = 0
    if L.Mq is not None and nu_post >= 1:
        x = (x + L.P @ xc) + om * (S @ (r - L.Mq @ xc))          # k_post_lp / k_bpost
        first = 1
    else:
        x = x + L.P @ xc
    for _ in range(first, nu_post):
        x = x + om * (S @ (b - A @ x))
    return x
