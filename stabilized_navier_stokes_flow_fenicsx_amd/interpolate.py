"""P1 evaluation of a coarse-mesh field at the nodes of another tet mesh.

The reference warm-starts the fine Navier-Stokes solve from the coarse one with
``create_interpolation_data(..., padding=1e-6)`` + ``interpolate_nonmatching``
(NavierStokesChannelFlow.py:175-194, row a9 of SURVEY 8).  Host-side numpy: a
uniform bucket grid over the coarse tets, then barycentric tests; points outside
every tet (beyond the padding) take the value of the best candidate, clamped.
It only affects the Newton iteration COUNT, never the converged field.

``device=...`` runs the same rule on the GPU (``sns_locate_points`` / ``sns_eval_p1``, csrc/sns_locate.hip): the
same bucket grid and candidate lists, so the same tets and coordinates up to the rounding of the 3x3 solve;
``eval_points`` evaluates P1 fields at arbitrary points that way.  The host path stays the default.
"""
from __future__ import annotations

import numpy as np

from .mesh import TetMesh


def _bary(X, p):
    """Barycentric coordinates of points p (m,3) in tets X (m,4,3) -> (m,4)."""
    T = np.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 3] - X[:, 0]], axis=2)
    lam = np.linalg.solve(T, (p - X[:, 0])[:, :, None])[:, :, 0]
    return np.concatenate([1.0 - lam.sum(axis=1, keepdims=True), lam], axis=1)


def locate_points(mesh: TetMesh, pts: np.ndarray, padding: float = 1e-6, device=None):
    """(tet index, barycentric coords) for every query point; ``device`` (e.g. "cuda:0") locates on the GPU."""
    if device is not None:
        dm = _DeviceMesh(mesh, device)
        t, lam, _ = locate_points_device(dm, _dev_array(pts, dm.device).view(-1, 3), padding)
        return t.cpu().numpy().astype(np.int64), lam.cpu().numpy()
    X = mesh.points[mesh.tets]                                   # (E,4,3)
    lo, hi = mesh.points.min(axis=0), mesh.points.max(axis=0)
    ext = np.maximum(hi - lo, 1e-300)
    E = len(mesh.tets)
    res = np.maximum(1, np.round((E / 6.0) ** (1.0 / 3.0) * ext / ext.max() * (ext.max() ** 3 / ext.prod()) ** (1 / 3)))
    res = res.astype(np.int64)
    h = ext / res
    tlo = np.clip(np.floor((X.min(axis=1) - lo) / h - 1e-9).astype(np.int64), 0, res - 1)
    thi = np.clip(np.floor((X.max(axis=1) - lo) / h + 1e-9).astype(np.int64), 0, res - 1)
    span = thi - tlo + 1
    cnt = span.prod(axis=1)
    tid = np.repeat(np.arange(E), cnt)
    off = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    s = span[tid]
    k = off % s[:, 2]
    j = (off // s[:, 2]) % s[:, 1]
    i = off // (s[:, 2] * s[:, 1])
    cell = ((tlo[tid, 0] + i) * res[1] + (tlo[tid, 1] + j)) * res[2] + (tlo[tid, 2] + k)
    order = np.argsort(cell, kind="stable")
    cell_s, tid_s = cell[order], tid[order]
    ncell = int(res.prod())
    cptr = np.zeros(ncell + 1, dtype=np.int64)
    np.add.at(cptr, cell_s + 1, 1)
    cptr = np.cumsum(cptr)
    q = np.clip(np.floor((pts - lo) / h).astype(np.int64), 0, res - 1)
    qc = (q[:, 0] * res[1] + q[:, 1]) * res[2] + q[:, 2]
    ncand = cptr[qc + 1] - cptr[qc]
    best_t = np.full(len(pts), -1, dtype=np.int64)
    best_l = np.zeros((len(pts), 4))
    best_m = np.full(len(pts), -np.inf)
    todo = np.arange(len(pts))
    for kk in range(int(ncand.max()) if len(pts) else 0):
        sel = todo[ncand[todo] > kk]
        if len(sel) == 0:
            break
        t = tid_s[cptr[qc[sel]] + kk]
        lam = _bary(X[t], pts[sel])
        mn = lam.min(axis=1)
        better = mn > best_m[sel]
        idx = sel[better]
        best_t[idx], best_l[idx], best_m[idx] = t[better], lam[better], mn[better]
        todo = todo[best_m[todo] < -padding]
    miss = best_t < 0
    if miss.any():                                                # no candidate in the bucket: nearest centroid
        cen = X.mean(axis=1)
        for i0 in np.nonzero(miss)[0]:
            t = int(np.argmin(((cen - pts[i0]) ** 2).sum(axis=1)))
            best_t[i0], best_l[i0] = t, _bary(X[t:t + 1], pts[i0:i0 + 1])[0]
    lam = np.clip(best_l, 0.0, 1.0)
    lam /= lam.sum(axis=1, keepdims=True)
    return best_t, lam


def interpolate_initial_guess(coarse: TetMesh, w_coarse: np.ndarray, fine: TetMesh, device=None) -> np.ndarray:
    """Fine-mesh nodal [ux,uy,uz,p] from the coarse solution (:175-194); ``device`` locates and evaluates on the GPU."""
    if device is not None:
        return eval_points(coarse, np.asarray(w_coarse).reshape(-1, 4), fine.points, device).reshape(-1)
    t, lam = locate_points(coarse, fine.points)
    Wc = np.asarray(w_coarse).reshape(-1, 4)[coarse.tets[t]]      # (n,4 verts,4 comps)
    return np.einsum("na,nac->nc", lam, Wc).reshape(-1)


# ---- the device path (csrc/sns_locate.hip) ---------------------------------------------------------------------------------------
def _dev_array(a, device, dtype=None):
    import torch
    dtype = torch.float64 if dtype is None else dtype
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)


class _DeviceMesh:
    """Points (n,3) fp64 and tets (E,4) int32 of a tet mesh on one device."""

    def __init__(self, mesh: TetMesh, device):
        import torch
        if int(getattr(mesh, "dim", 3)) != 3:
            raise NotImplementedError("point location on the device covers 3-D tet meshes only")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"device point location needs a HIP device, got {device!r}; there is no CPU fallback")
        self.n_nodes, self.n_tets = mesh.num_nodes, mesh.num_tets
        self.pts = _dev_array(mesh.points, self.device)
        self.tets = _dev_array(mesh.tets, self.device, torch.int32)


def _stream(device):
    import ctypes as C
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def locate_points_device(dm: _DeviceMesh, query, padding: float = 1e-6):
    """(tet int32, lambda (m,4), number of missed points) on ``dm.device`` for the device tensor ``query`` (m,3)."""
    import ctypes as C
    import torch
    from . import _lib
    lib = _lib.load()
    m = query.shape[0]
    tet = torch.empty(m, dtype=torch.int32, device=dm.device)
    lam = torch.empty((m, 4), dtype=torch.float64, device=dm.device)
    n_missed = C.c_int64(0)
    p = lambda x: C.c_void_p(x.data_ptr())
    with torch.cuda.device(dm.device):
        _lib.check(lib.sns_locate_points(dm.n_nodes, dm.n_tets, p(dm.pts), p(dm.tets), m, p(query), float(padding), p(tet),
                                         p(lam), C.byref(n_missed), _stream(dm.device)))
    return tet, lam, int(n_missed.value)


def eval_p1_device(dm: _DeviceMesh, values, tet, lam):
    """out (m, ncomp) = P1 values (n_nodes, ncomp) at the located points (tet, lam), on ``dm.device``."""
    import ctypes as C
    import torch
    from . import _lib
    lib = _lib.load()
    ncomp = values.shape[1]
    out = torch.empty((tet.shape[0], ncomp), dtype=torch.float64, device=dm.device)
    p = lambda x: C.c_void_p(x.data_ptr())
    with torch.cuda.device(dm.device):
        _lib.check(lib.sns_eval_p1(dm.n_tets, p(dm.tets), ncomp, p(values), tet.shape[0], p(tet), p(lam), p(out),
                                   _stream(dm.device)))
    return out


def eval_points(mesh: TetMesh, values, pts, device, padding: float = 1e-6) -> np.ndarray:
    """P1 field ``values`` (n_nodes,) or (n_nodes, ncomp <= 4) of ``mesh`` at the points ``pts`` (m,3) -> (m, ncomp) numpy,
    located and evaluated on ``device`` by locate_points' rule (what DOLFINx' ``Function.eval`` with a bounding-box tree gives;
    a point outside the mesh takes its best candidate's clamped value, as the host interpolation does)."""
    n = mesh.num_nodes
    v = values if hasattr(values, "data_ptr") else np.asarray(values, dtype=np.float64)
    if v.ndim == 1:
        v = v.reshape(-1, 1)
    if v.ndim != 2 or v.shape[0] != n or not 1 <= v.shape[1] <= 4:
        raise ValueError(f"values must be (n_nodes,) or (n_nodes, 1..4) with n_nodes = {n}, got {tuple(values.shape)}")
    dm = _DeviceMesh(mesh, device)
    q = _dev_array(pts, dm.device).view(-1, 3)
    tet, lam, _ = locate_points_device(dm, q, padding)
    return eval_p1_device(dm, _dev_array(v, dm.device), tet, lam).cpu().numpy()
