"""Independent numpy restatement of the gradient recovery of sns_recover_gradient / sns_error_indicator and of
functionals.wall_shear_stress, for tets and triangles.  It imports nothing of the product.

    cells (E, d+1), points (n, d), w (4 n,) with dofs (u_x, u_y, u_z, p) per node
    G_i[c][j] = sum_{t in cells(i)} |t| d_j w_c|_t / sum_{t in cells(i)} |t|,   |t| = |det J| / d!      (n, 4, 3)
    D_i = (omega_x, omega_y, omega_z, Q, shear rate, div u) from the velocity rows of G_i                  (n, 6)
    eta_t^2 = int_t |G_h(u) - grad u_h|_F^2,  g_t^2 = |t| |grad u_h|_F^2                                   (E,), (E,)

The cell integral of the indicator is evaluated through the P1 mass matrix M_ab = |t| (1 + delta_ab) / ((d+1)(d+2)), which is
exact for the square of a P1 function.  In 2-D the third column of every gradient is zero."""
import math

import numpy as np


def cell_gradients(points, cells, w):
    """(grad (E, 4, 3) with grad[t, c, j] = d_j w_c on cell t, vol (E,))."""
    points, cells = np.asarray(points, dtype=np.float64), np.asarray(cells, dtype=np.int64)
    d = points.shape[1]
    assert cells.shape[1] == d + 1
    W = np.asarray(w, dtype=np.float64).reshape(-1, 4)
    X = points[cells]                                             # (E, d+1, d)
    J = np.swapaxes(X[:, 1:] - X[:, :1], 1, 2)                    # J[t, i, m] = X_{m+1, i} - X_{0, i}
    K = np.linalg.inv(J)                                          # K[t, m, j] = d_j phi_{m+1}
    gphi = np.concatenate([-K.sum(axis=1, keepdims=True), K], axis=1)      # (E, d+1, d)
    grad = np.zeros((len(cells), 4, 3))
    grad[:, :, :d] = np.einsum("tac,taj->tcj", W[cells], gphi)
    vol = np.abs(np.linalg.det(J)) / math.factorial(d)
    return grad, vol


def recover(points, cells, w):
    """The recovered nodal gradient G (n, 4, 3); nodes of no cell get zeros."""
    cells = np.asarray(cells, dtype=np.int64)
    n = len(points)
    grad, vol = cell_gradients(points, cells, w)
    num, den = np.zeros((n, 4, 3)), np.zeros(n)
    for a in range(cells.shape[1]):
        np.add.at(num, cells[:, a], vol[:, None, None] * grad)
        np.add.at(den, cells[:, a], vol)
    G = np.zeros_like(num)
    ok = den > 0
    G[ok] = num[ok] / den[ok, None, None]
    return G


def derived_parts(G):
    """(omega (n, 3), |Omega|_F^2, |S|_F^2, tr) of the velocity rows of G."""
    U = np.asarray(G)[:, :3, :]
    S, Om = 0.5 * (U + np.swapaxes(U, 1, 2)), 0.5 * (U - np.swapaxes(U, 1, 2))
    omega = np.stack([U[:, 2, 1] - U[:, 1, 2], U[:, 0, 2] - U[:, 2, 0], U[:, 1, 0] - U[:, 0, 1]], axis=1)
    return omega, (Om ** 2).sum(axis=(1, 2)), (S ** 2).sum(axis=(1, 2)), np.trace(U, axis1=1, axis2=2)


def derived(G):
    """D (n, 6): vorticity, Q = (|Omega|^2 - |S|^2) / 2, shear rate sqrt(2 S:S), div u."""
    omega, OO, SS, tr = derived_parts(G)
    return np.concatenate([omega, np.stack([0.5 * (OO - SS), np.sqrt(2.0 * SS), tr], axis=1)], axis=1)


def q_scale(G):
    """max_i (|Omega|^2 + |S|^2) / 2: the size of the terms that cancel in Q."""
    _, OO, SS, _ = derived_parts(G)
    return float((0.5 * (OO + SS)).max())


def indicator(points, cells, w, G=None):
    """(eta2 (E,), g2 (E,)) over the velocity rows; G defaults to recover(points, cells, w)."""
    cells = np.asarray(cells, dtype=np.int64)
    d = cells.shape[1] - 1
    if G is None:
        G = recover(points, cells, w)
    grad, vol = cell_gradients(points, cells, w)
    e = np.asarray(G)[cells][:, :, :3, :] - grad[:, None, :3, :]           # (E, d+1, 3, 3)
    M = (np.ones((d + 1, d + 1)) + np.eye(d + 1)) / ((d + 1) * (d + 2))
    eta2 = vol * np.einsum("ab,taij,tbij->t", M, e, e)
    return eta2, vol * (grad[:, :3, :] ** 2).sum(axis=(1, 2))


def zz(points, cells, w):
    """(eta, eta_rel, eta2): eta = sqrt(sum eta_t^2), eta_rel = eta / sqrt(sum g_t^2 + sum eta_t^2)."""
    eta2, g2 = indicator(points, cells, w)
    eta = math.sqrt(eta2.sum())
    return eta, eta / math.sqrt(g2.sum() + eta2.sum()), eta2


def wall_shear_stress(points, cells, facets, G, nu):
    """(nodes, tau (len(nodes), 3)): tau_w = 2 nu S n - (n . 2 nu S n) n at the nodes of the boundary ``facets`` (triangles of a
    tet mesh or edges of a triangle mesh), S from the recovered gradient, n the unit area-weighted nodal normal of those
    facets pointing INTO the fluid (away from the facet's cell)."""
    points, cells, facets = np.asarray(points, dtype=np.float64), np.asarray(cells, dtype=np.int64), np.asarray(facets, dtype=np.int64)
    d = points.shape[1]
    nodes = np.unique(facets)
    nrm = {int(i): np.zeros(3) for i in nodes}
    cellsets = [set(c) for c in cells.tolist()]
    for f in facets.tolist():
        (t,) = [k for k, c in enumerate(cellsets) if set(f) <= c]         # the single cell behind a boundary facet
        (opp,) = cellsets[t] - set(f)
        P = np.zeros((d, 3))
        P[:, :d] = points[f]
        inward = np.zeros(3)
        inward[:d] = points[opp] - points[f[0]]
        if d == 3:
            a = 0.5 * np.cross(P[1] - P[0], P[2] - P[0])
        else:
            tv = P[1] - P[0]
            a = np.array([tv[1], -tv[0], 0.0])
        if a @ inward < 0:
            a = -a
        for i in f:
            nrm[i] += a
    tau = np.zeros((len(nodes), 3))
    for k, i in enumerate(nodes):
        n = nrm[int(i)] / np.linalg.norm(nrm[int(i)])
        U = np.asarray(G)[i, :3, :]
        t = nu * (U + U.T) @ n
        tau[k] = t - (n @ t) * n
    return nodes, tau


def true_gradient_error(points, tets, w, grad_u):
    """sqrt(int |grad u - grad u_h|_F^2) over a tet mesh by the symmetric 4-point rule (degree 2: barycentric coordinates
    (5 + 3 sqrt 5) / 20 once and (5 - sqrt 5) / 20 three times, weights 1/4); ``grad_u(x (m, 3)) -> (m, 3, 3)`` is the exact
    velocity gradient [i, j] = d_j u_i."""
    tets = np.asarray(tets, dtype=np.int64)
    grad, vol = cell_gradients(points, tets, w)
    X = np.asarray(points, dtype=np.float64)[tets]                         # (E, 4, 3)
    a, b = (5.0 + 3.0 * math.sqrt(5.0)) / 20.0, (5.0 - math.sqrt(5.0)) / 20.0
    s = np.zeros(len(tets))
    for k in range(4):
        xq = b * X.sum(axis=1) + (a - b) * X[:, k]
        s += 0.25 * ((grad_u(xq) - grad[:, :3, :]) ** 2).sum(axis=(1, 2))
    return math.sqrt((vol * s).sum())
