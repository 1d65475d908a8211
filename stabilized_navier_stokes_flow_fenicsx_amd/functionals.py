"""Boundary functionals of a P1-P1 solution: traction force on tagged facets, drag / lift coefficients.

Mirrors the post-processing of the reference's DFG benchmark script
(Validation_Flow/DFG_3D_Validation.py:344-367):

    n        = -FacetNormal(msh)                       # pointing out of the obstacle, into the fluid
    stress   = -p I + 2 mu sym(grad u)
    traction = stress . n
    F_drag   = assemble(traction[0] * ds(obstacle)),  F_lift = assemble(traction[1] * ds(obstacle))
    C_d      = 2 F_drag / (rho Uc^2 Lc),               C_l   = 2 F_lift / (rho Uc^2 Lc)

For P1 fields grad u is constant in the tet behind a boundary facet and p is linear on the facet, so the
facet integrals are exact with  area * (stress(grad u, mean of the 3 nodal p) . n).  Host side (numpy): the
obstacle surface holds O(N^(2/3)) facets, there is nothing to accelerate.

``reaction_force`` is the variationally consistent (residual-based) alternative: F = -R_raw(w)(phi e_c), the raw residual
tested with the P1 function phi that is 1 on the surface's nodes and 0 elsewhere.  It runs on the
device (sns_residual_moments) over the cells behind the surface only, and on a partitioned problem needs no gather.
"""
from __future__ import annotations

import numpy as np

from .mesh import TetMesh


def facet_parent_tets(mesh: TetMesh, facet_ids: np.ndarray) -> np.ndarray:
    """Index of the (single) tet behind each boundary facet."""
    f = np.sort(mesh.facets[facet_ids].astype(np.int64), axis=1)
    n = mesh.num_nodes
    want = (f[:, 0] * n + f[:, 1]) * n + f[:, 2]
    t = mesh.tets.astype(np.int64)
    faces = np.concatenate([t[:, [1, 2, 3]], t[:, [0, 2, 3]], t[:, [0, 1, 3]], t[:, [0, 1, 2]]])
    faces.sort(axis=1)
    key = (faces[:, 0] * n + faces[:, 1]) * n + faces[:, 2]
    order = np.argsort(key, kind="stable")
    pos = np.searchsorted(key[order], want)
    if np.any(pos >= len(key)) or np.any(key[order][np.minimum(pos, len(key) - 1)] != want):
        raise ValueError("a boundary facet is not a face of any tet")
    return (order[pos] % len(t)).astype(np.int64)


def boundary_traction_force(mesh: TetMesh, w: np.ndarray, nu: float, tag: int) -> np.ndarray:
    """int_{facets tagged ``tag``} (-p I + 2 nu sym grad u) . n ds  with  n = -(outward normal of the fluid domain),
    as a 3-vector (DFG_3D_Validation.py:348-356: drag = component 0, lift = component 1)."""
    ids = mesh.find(tag)
    if len(ids) == 0:
        return np.zeros(3)
    W = np.asarray(w, dtype=np.float64).reshape(-1, 4)
    par = facet_parent_tets(mesh, ids)
    tn = mesh.tets[par].astype(np.int64)                     # (F,4)
    X = mesh.points[tn]                                      # (F,4,3)
    J = np.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 3] - X[:, 0]], axis=2)       # J_ij = dx_i/dX_j
    K = np.linalg.inv(J)                                     # K_ji = dX_j/dx_i
    g = np.concatenate([-K.sum(axis=1, keepdims=True), K], axis=1)                      # (F,4,3) grad phi_a
    gu = np.einsum("fai,faj->fij", W[tn][:, :, :3], g)       # (grad u)_ij = d u_i / d x_j
    fn = mesh.facets[ids].astype(np.int64)
    P = mesh.points[fn]                                      # (F,3,3)
    cr = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])      # |cr| = 2 area
    # orient outward from the fluid: away from the tet's 4th (non-facet) vertex
    opp = tn.sum(axis=1) - fn.sum(axis=1)                    # the facet's 3 nodes are 3 of the tet's 4
    sgn = np.sign(np.einsum("fi,fi->f", cr, P[:, 0] - mesh.points[opp]))
    n_area = -0.5 * cr * sgn[:, None]                        # n ds with n = -outward
    pm = W[fn][:, :, 3].mean(axis=1)
    stress = 2.0 * nu * 0.5 * (gu + gu.transpose(0, 2, 1))
    stress[:, [0, 1, 2], [0, 1, 2]] -= pm[:, None]
    return np.einsum("fij,fj->i", stress, n_area)


def wall_shear_stress(mesh: TetMesh, G, nu: float, tag: int):
    """Wall shear stress at the nodes of the facets tagged ``tag``: ``(nodes, tau)`` with tau (len(nodes), 3),

        tau_w = 2 nu S n - (n . 2 nu S n) n,     S = sym of the velocity rows of the recovered gradient ``G`` (n, 4, 3)

    (``FlowProblem.recover_gradient``, as numpy), n the unit area-weighted nodal normal of those facets with the orientation of
    ``boundary_traction_force`` (n = -outward normal of the fluid domain), so that the surface integral of tau_w is the
    tangential viscous part of that force.  Assumes a CONSTANT viscosity ``nu``: with a viscosity law set, the stress of the
    law is not what this returns.  3-D; ``mesh2d.wall_shear_stress_2d`` is the counterpart for triangle meshes.  Host numpy."""
    ids = mesh.find(tag)
    if len(ids) == 0:
        return np.zeros(0, np.int64), np.zeros((0, 3))
    tn = mesh.tets[facet_parent_tets(mesh, ids)].astype(np.int64)
    fn = mesh.facets[ids].astype(np.int64)
    P = mesh.points[fn]
    cr = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    opp = tn.sum(axis=1) - fn.sum(axis=1)
    sgn = np.sign(np.einsum("fi,fi->f", cr, P[:, 0] - mesh.points[opp]))
    n_area = -0.5 * cr * sgn[:, None]                        # as in boundary_traction_force
    return _tangential_stress(mesh.num_nodes, fn, n_area, G, nu)


def _tangential_stress(num_nodes: int, fn: np.ndarray, n_area: np.ndarray, G, nu: float):
    nrm = np.zeros((num_nodes, 3))
    for a in range(fn.shape[1]):
        np.add.at(nrm, fn[:, a], n_area)
    nodes = np.unique(fn)
    n = nrm[nodes] / np.linalg.norm(nrm[nodes], axis=1)[:, None]
    U = np.asarray(G, dtype=np.float64).reshape(-1, 4, 3)[nodes, :3, :]
    t = nu * np.einsum("kij,kj->ki", U + U.transpose(0, 2, 1), n)
    return nodes, t - np.einsum("ki,ki->k", n, t)[:, None] * n


def boundary_traction_gradient(mesh: TetMesh, nu: float, tag: int) -> np.ndarray:
    """d(boundary_traction_force)/dw as a (3, 4 n) array G: the force is linear in the state, ``G @ w`` equals
    ``boundary_traction_force(mesh, w, nu, tag)`` up to the rounding of a reordered sum.  Built from the same arrays
    (parent tets, P1 gradients, oriented facet areas); G is affine in nu, so the force's explicit nu-derivative at fixed w
    is ``(boundary_traction_gradient(mesh, 1, tag) - boundary_traction_gradient(mesh, 0, tag)) @ w``.  Row c is the
    right-hand side of the adjoint solve for force component c (solver.reynolds_sensitivity)."""
    G = np.zeros((3, 4 * mesh.num_nodes))
    ids = mesh.find(tag)
    if len(ids) == 0:
        return G
    par = facet_parent_tets(mesh, ids)
    tn = mesh.tets[par].astype(np.int64)                     # (F,4)
    X = mesh.points[tn]
    J = np.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 3] - X[:, 0]], axis=2)
    K = np.linalg.inv(J)
    g = np.concatenate([-K.sum(axis=1, keepdims=True), K], axis=1)                      # (F,4,3) grad phi_a
    fn = mesh.facets[ids].astype(np.int64)
    P = mesh.points[fn]
    cr = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    opp = tn.sum(axis=1) - fn.sum(axis=1)
    sgn = np.sign(np.einsum("fi,fi->f", cr, P[:, 0] - mesh.points[opp]))
    n_area = -0.5 * cr * sgn[:, None]
    # force_i = sum_f nu (gu_ij + gu_ji) nA_j - pm nA_i,  gu_ij = sum_a u_i(a) g_aj
    gn = nu * np.einsum("faj,fj->fa", g, n_area)             # u_i(a) -> force_i
    gx = nu * np.einsum("fai,fj->faij", g, n_area)           # u_j(a) -> force_i
    for i in range(3):
        np.add.at(G[i], 4 * tn + i, gn)
        for j in range(3):
            np.add.at(G[i], 4 * tn + j, gx[:, :, i, j])
        np.add.at(G[i], 4 * fn + 3, np.repeat(-n_area[:, i:i + 1] / 3.0, 3, axis=1))
    return G


def boundary_traction_shape_gradient(mesh: TetMesh, w: np.ndarray, nu: float, tag: int) -> np.ndarray:
    """d(boundary_traction_force)/dX at FIXED state ``w`` as a (3, n, 3) array: entry [c, k, j] is the derivative of force
    component c with respect to coordinate j of node k.  This is the explicit part dJ/dX of ``solver.shape_sensitivity``
    for a traction functional.  The force depends on the coordinates through the P1 gradients of the tets behind the
    tagged facets and through the facets' area vectors, so the result is non-zero only on the nodes of those tets.  Exact:
    reverse-mode autograd over the same expressions as ``boundary_traction_force`` on those few cells (the orientation
    sign of a facet is piecewise constant)."""
    import torch
    out = np.zeros((3, mesh.num_nodes, 3))
    ids = mesh.find(tag)
    if len(ids) == 0:
        return out
    W = np.asarray(w, dtype=np.float64).reshape(-1, 4)
    par = facet_parent_tets(mesh, ids)
    tn = mesh.tets[par].astype(np.int64)
    fn = mesh.facets[ids].astype(np.int64)
    nodes = np.unique(tn)
    Xn = torch.tensor(mesh.points[nodes], dtype=torch.float64, requires_grad=True)
    X = Xn[torch.from_numpy(np.searchsorted(nodes, tn))]                               # (F,4,3)
    P = Xn[torch.from_numpy(np.searchsorted(nodes, fn))]                               # (F,3,3)
    J = torch.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 3] - X[:, 0]], dim=2)
    K = torch.linalg.inv(J)
    g = torch.cat([-K.sum(dim=1, keepdim=True), K], dim=1)
    gu = torch.einsum("fai,faj->fij", torch.from_numpy(W[tn][:, :, :3]), g)
    cr = torch.linalg.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    opp = tn.sum(axis=1) - fn.sum(axis=1)
    Pn = mesh.points[fn]
    sgn = np.sign(np.einsum("fi,fi->f", np.cross(Pn[:, 1] - Pn[:, 0], Pn[:, 2] - Pn[:, 0]), Pn[:, 0] - mesh.points[opp]))
    n_area = -0.5 * cr * torch.from_numpy(sgn)[:, None]
    pm = torch.from_numpy(W[fn][:, :, 3].mean(axis=1))
    stress = nu * (gu + gu.transpose(1, 2)) - pm[:, None, None] * torch.eye(3, dtype=torch.float64)
    force = torch.einsum("fij,fj->i", stress, n_area)
    for c in range(3):
        out[c, nodes] = torch.autograd.grad(force[c], Xn, retain_graph=True)[0].numpy()
    return out


def point_value_gradient(mesh: TetMesh, pts, comp: int = 3, padding: float = 1e-6, device=None) -> np.ndarray:
    """d(value of component ``comp`` of the P1 solution at the points ``pts`` (m,3))/dw as an (m, 4 n) array: the
    barycentric weights of ``interpolate.locate_points`` -- what ``FlowProblem.eval_at`` evaluates with -- in the columns
    of the containing tet's nodes.  ``device`` locates on the GPU."""
    from .interpolate import locate_points
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    tet, lam = locate_points(mesh, pts, padding, device=device)
    G = np.zeros((len(pts), 4 * mesh.num_nodes))
    cols = 4 * mesh.tets[np.asarray(tet, dtype=np.int64)].astype(np.int64) + comp
    np.add.at(G, (np.arange(len(pts))[:, None], cols), np.asarray(lam, dtype=np.float64))
    return G


def pressure_difference_gradient(mesh: TetMesh, p_front, p_back, padding: float = 1e-6, device=None) -> np.ndarray:
    """d(p(p_front) - p(p_back))/dw as a dof vector (the DFG benchmarks' pressure drop across the obstacle)."""
    G = point_value_gradient(mesh, np.stack([np.asarray(p_front, float), np.asarray(p_back, float)]), 3, padding, device)
    return G[0] - G[1]


def drag_lift_coefficients(force: np.ndarray, rho: float = 1.0, Uc: float = 0.2, Lc: float = 0.1 * 0.41):
    """(C_d, C_l) = 2 F / (rho Uc^2 Lc)  (DFG_3D_Validation.py:345-346,364-365; defaults are the script's)."""
    s = 2.0 / (rho * Uc * Uc * Lc)
    return s * float(force[0]), s * float(force[1])


def tag_node_weights(mesh: TetMesh, tag: int, *, rim_tags=(), rim_weight: float = 1.0, part=None) -> np.ndarray:
    """Nodal weights phi of the surface tagged ``tag`` (the P1 indicator of its facets' nodes): 1 on those nodes, 0 elsewhere;
    nodes that also lie on a facet tagged one of ``rim_tags`` (the rim where the surface meets a no-slip wall) get
    ``rim_weight``.  With ``part`` (partition.LocalPart of ``mesh``) the weights are returned in that rank's local node
    numbering (owned nodes first, then ghosts); sns_residual_moments reads only the owned ones, so every node counts once
    over the ranks."""
    phi = np.zeros(mesh.num_nodes)
    phi[mesh.facet_nodes(tag)] = 1.0
    if len(rim_tags) and rim_weight != 1.0:
        other = np.unique(mesh.facets[np.isin(mesh.facet_tags, np.asarray(rim_tags))].ravel())
        phi[other[phi[other] != 0.0]] = rim_weight
    return np.ascontiguousarray(phi[part.l2g]) if part is not None else phi


def reaction_force(problem, w, tag: int, *, mesh: TetMesh | None = None, rim_tags=(), rim_weight: float = 1.0,
                   form: str = "ns") -> np.ndarray:
    """Residual-based force on the surface tagged ``tag``: F = -R_raw(w)(phi e_c), c = 0..2, phi = tag_node_weights, as a
    3-vector in the convention of boundary_traction_force (drag_lift_coefficients takes either).  ``w``: the problem's
    local device (or numpy) state.  ``mesh``: the tagged global mesh; defaults to the problem's own (the global mesh of a
    ``FlowProblem.distributed`` rank, whose local part carries no facet tags).  Every rank returns the same force."""
    part = getattr(problem, "part", None)
    if mesh is None:
        mesh = getattr(problem, "global_mesh", None) if part is not None else problem.mesh
        if mesh is None:
            raise ValueError("reaction_force: pass the tagged global mesh of this partitioned problem")
    phi = tag_node_weights(mesh, tag, rim_tags=rim_tags, rim_weight=rim_weight, part=part)
    return -problem.residual_moments(w, phi, form)[:3]


def reaction_force_gradient(problem, w, tag: int, *, mesh: TetMesh | None = None, rim_tags=(), rim_weight: float = 1.0):
    """d(reaction_force)/dw at fixed Re as a device tensor (3, ndof): row c is ``-J0(w)^T (phi e_c)``, J0 the Jacobian of the raw
    residual (``FlowProblem.raw_jacobian_apply``, one transposed pass per component) and phi the weights ``reaction_force``
    tests with.  The rows are not zero on Dirichlet dofs: the force of a state depends on the values the state takes there.  As
    the grad_J of ``solver.reynolds_sensitivity`` / ``shape_sensitivity`` / ``dirichlet_sensitivity`` they are used as they
    are; the explicit parts are ``reaction_force_reynolds_derivative`` and ``-problem.residual_shape_gradient(w, phi e_c)``.
    Single-GPU problems, NS form."""
    import torch
    m = problem.mesh if mesh is None else mesh
    phi = torch.from_numpy(tag_node_weights(m, tag, rim_tags=rim_tags, rim_weight=rim_weight)).to(problem.device)
    out = torch.empty(3, problem.ndof, dtype=torch.float64, device=problem.device)
    z = problem.zeros()
    for c in range(3):
        z.zero_()
        z[c::4] = phi
        problem.raw_jacobian_apply(w, z, transpose=True, out=out[c])
    return out.neg_()


def reaction_force_reynolds_derivative(problem, w, tag: int, rel_step: float = 1e-4, *, mesh: TetMesh | None = None, rim_tags=(),
                                       rim_weight: float = 1.0) -> np.ndarray:
    """The explicit part d(reaction_force)/dRe at fixed ``w`` as a 3-vector: central difference of ``residual_moments`` at
    Re (1 +- rel_step), mirroring ``solver.residual_reynolds_derivative``; the problem's options are restored afterwards."""
    m = problem.mesh if mesh is None else mesh
    phi = tag_node_weights(m, tag, rim_tags=rim_tags, rim_weight=rim_weight)
    Re = float(problem.options.reynolds)
    try:
        problem.set_options(reynolds=Re * (1.0 + rel_step))
        Fp = -problem.residual_moments(w, phi, "ns")[:3]
        problem.set_options(reynolds=Re * (1.0 - rel_step))
        Fm = -problem.residual_moments(w, phi, "ns")[:3]
    finally:
        problem.set_options(reynolds=Re)
    return (Fp - Fm) / (2.0 * Re * rel_step)
