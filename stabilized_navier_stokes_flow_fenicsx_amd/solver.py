"""Host-side mirror of the reference's solve seam over the HIP C-ABI.

Names, argument meaning and error behaviour follow
NavierStokes/NavierStokesChannelFlow.py:
  * ``NonlinearPDE_SNESProblem`` (:40-75)  -> F / J callbacks on device vectors
  * ``solve_stokes_problem``     (:197-218)
  * ``solve_navier_stokes``      (:268-312): returns ``(w, u, p)``, prints
    iterations / reason / seconds (:297-299); non-convergence is NOT an error.
All arithmetic happens in libsns.so (HIP); torch only owns device buffers and
the stream.  There is no CPU fallback: constructing a ``FlowProblem`` without
a GPU and the built library raises.
"""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import FORM_NS, FORM_STOKES, SnsError, SnsOptions, SnsTimings, check, default_options
from .bcs import DirichletSet
from .mesh import TetMesh

_FORMS = {"stokes": FORM_STOKES, "ns": FORM_NS, FORM_STOKES: FORM_STOKES, FORM_NS: FORM_NS}


def _ptr(t):
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


@dataclass
class KrylovResult:
    its: int
    reason: int
    rnorm: float


@dataclass
class NewtonResult:
    its: int
    reason: int
    ksp_its: int
    fnorms: list
    seconds: float
    ptc_steps: int = 0          # pseudo-steps taken before the closing solve (solver.pseudo_transient_solve)


@dataclass
class ArnoldiResult:
    m_done: int                 # columns of H (and Ritz values) the process produced
    reason: int                 # 1 all m steps, 2 breakdown (invariant Krylov space), < 0 the KSP reason of a failed inner solve
    ksp_its: int                # Krylov iterations over all inner solves


@dataclass
class StabilityResult:
    eigenvalues: np.ndarray     # (n,) complex, descending real part: the least stable first
    modes: torch.Tensor         # (n, ndof) complex128 on the device, unit 2-norm, largest-modulus entry real and positive
    estimates: np.ndarray       # (n,) residual estimates |h_{m+1,m} e_m^T y| / |theta| (a complex shift: true residuals)
    converged: np.ndarray       # (n,) bool: estimate <= tol
    m_done: int
    ksp_its: int
    reason: int
    # linear_stability(left=True) only:
    shift: float = 0.0          # (the complex shift of a complex-shift run)
    left_modes: Optional[torch.Tensor] = None     # (n, ndof) complex128: z with z^T J = -lam z^T B, scaled so that z^T B x = 1 (unconjugated); 0 where unpaired
    left_converged: Optional[np.ndarray] = None   # (n,) bool: the right pair converged and has a converged left partner
    left_eigenvalues: Optional[np.ndarray] = None  # (n,) complex: the partner's own Ritz value (nan where unpaired)
    left_m_done: int = 0
    left_ksp_its: int = 0
    left_reason: int = 0
    # linear_stability(max_restarts > 0) only: thick restarts taken by the right and by the left process
    restarts: int = 0
    left_restarts: int = 0


class FlowProblem:
    """Mesh + Dirichlet data + operator hierarchy on one GPU (one per rank).  ``mesh`` is a ``TetMesh`` (3-D
    G-metric forms) or a ``mesh2d.TriMesh`` (2-D UGN forms of the lid-driven / DFG-2D scripts; "stokes" and "ns"
    then name the 2-D forms, see sns_create_2d in include/sns.h).

    Keyword options are fields of ``sns_options`` (include/sns.h).  For sliver-rich meshes ``amg_aggregation=1`` aggregates the
    fine level by operator strength with the host matcher; ``amg_aggregation=2`` builds the identical aggregates on the GPU,
    which is what large meshes want (the host matcher alone takes about 1 s at 10 M tets).  ``amg_aggregation=3`` (hybrid) is
    for meshes whose quality is not known before the solve: where the geometric map of the default cuts no dominant coupling it
    runs the default bit for bit (at the cost of the strength kernel and one mark pass at the first ``pc_setup``); a mesh with
    more than 1 % of its rows marked (sliver-rich throughout) gets value 2's aggregates and blocks; a mesh bad only in a region
    (fewer rows marked) gets only the aggregates there re-matched, plus the fine-level aggregate blocks -- on a channel jittered
    in one half 22.2 instead of 30.5 BiCGStab iterations per Newton step (profiles/hybrid_aggregation.txt).

    Replaces what ``functionspace`` / ``dirichletbc`` / ``create_matrix`` /
    ``fem.form`` build for the reference (:127-147, :45-46, :271-272).
    """

    def __init__(self, mesh: TetMesh, bcs, *, device="cuda:0", options: SnsOptions | None = None, part=None,
                 group=None, **opt_kw):
        if not torch.cuda.is_available():
            raise RuntimeError("FlowProblem needs a HIP device; the hot path has no CPU fallback")
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.mesh = mesh
        if isinstance(bcs, DirichletSet):
            mask, g = bcs.flatten()
        else:
            mask, g = bcs
        self.bc_mask = np.ascontiguousarray(mask, dtype=np.uint8)
        self.bc_val = np.ascontiguousarray(g, dtype=np.float64)
        self.options = options if options is not None else default_options(**opt_kw)
        self.dim = int(getattr(mesh, "dim", 3))
        pts = np.ascontiguousarray(mesh.points, dtype=np.float64)
        tets = np.ascontiguousarray(mesh.tris if self.dim == 2 else mesh.tets, dtype=np.int32)
        if self.bc_mask.shape != (4 * len(pts),) or self.bc_val.shape != (4 * len(pts),):
            raise ValueError("bc arrays must have 4*num_nodes entries")
        if pts.shape[1] != self.dim or tets.shape[1] != self.dim + 1:
            raise ValueError("mesh arrays do not match the mesh dimension")
        if self.dim == 2:
            if part is not None:
                raise ValueError("2-D problems run on a single GPU (no partition)")
            # the unused z component is a homogeneous Dirichlet dof (libsns.so imposes the same)
            self.bc_mask = self.bc_mask.copy()
            self.bc_val = self.bc_val.copy()
            self.bc_mask[2::4] = 1
            self.bc_val[2::4] = 0.0
        h = C.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        create = self.lib.sns_create_2d if self.dim == 2 else self.lib.sns_create
        check(create(C.byref(h), len(pts), len(tets), pts.ctypes.data, tets.ctypes.data,
                     self.bc_mask.ctypes.data, self.bc_val.ctypes.data, idx, C.byref(self.options)))
        self.h = h
        self.viscosity_law = None                      # (lambda, n, nu_inf_ratio) while set_viscosity_law is in force
        self.n_local = len(pts)
        self.n_owned = len(pts)
        with torch.cuda.device(self.device):
            check(self.lib.sns_set_stream(self.h, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self.g_dev = torch.from_numpy(self.bc_val).to(self.device)
        self.part = part
        self.group = group
        if part is not None:
            self._attach_comm(part, group)

    @classmethod
    def distributed(cls, mesh: TetMesh, bcs, *, group=None, device=None, **kw):
        """One rank's problem of an element-partitioned run (one process per GPU).

        Every rank passes the same global mesh / BC data; RCB partition, local
        renumbering and the halo plan are computed here (partition.py); the RCCL
        communicator of the C-ABI is bootstrapped through torch.distributed."""
        import torch.distributed as dist
        from . import partition as PT
        if isinstance(group, PeerGroup):
            rank, world = group.rank, group.nranks
        else:
            rank, world = dist.get_rank(group), dist.get_world_size(group)
        mask, g = bcs.flatten() if isinstance(bcs, DirichletSet) else bcs
        owner = PT.rcb_partition(mesh.points, world)
        part = PT.build_local_part(mesh, mask, g, owner, rank, world)
        if device is None:
            device = f"cuda:{torch.cuda.current_device()}"
        self = cls(part.mesh, (part.bc_mask, part.bc_val), device=device, part=part, group=group, **kw)
        self.global_mesh = mesh
        return self

    @classmethod
    def from_part(cls, part, *, group=None, device=None, **kw):
        """One rank's problem from a ready-made LocalPart (e.g. partition.duct_slab_part, which meshes only
        this rank's slab); same communicator bootstrap as ``distributed``."""
        if device is None:
            device = f"cuda:{torch.cuda.current_device()}"
        self = cls(part.mesh, (part.bc_mask, part.bc_val), device=device, part=part, group=group, **kw)
        self.global_mesh = None
        self.n_global_nodes = int(part.mesh.meta.get("global_num_nodes", 0))
        return self

    def _attach_comm(self, part, group):
        nb = np.ascontiguousarray(part.neighbors, dtype=np.int32)
        sp_, si = np.ascontiguousarray(part.send_ptr, np.int32), np.ascontiguousarray(part.send_idx, np.int32)
        rp, ri = np.ascontiguousarray(part.recv_ptr, np.int32), np.ascontiguousarray(part.recv_idx, np.int32)
        if isinstance(group, Team):                    # tests: N ranks = N threads of this process
            with torch.cuda.device(self.device):
                check(self.lib.sns_attach_team(self.h, group.ptr, part.rank, part.nranks, part.n_owned, len(nb),
                                               nb.ctypes.data, sp_.ctypes.data, si.ctypes.data, rp.ctypes.data,
                                               ri.ctypes.data))
            self.n_owned = part.n_owned
            return
        if isinstance(group, PeerGroup):               # one process per GPU of one node, peer windows over xGMI
            if (group.rank, group.nranks) != (part.rank, part.nranks):
                raise ValueError("partition and peer communicator disagree about rank / ranks")
            with torch.cuda.device(self.device):
                check(self.lib.sns_attach_peer(self.h, group.ptr, part.n_owned, len(nb), nb.ctypes.data, sp_.ctypes.data,
                                               si.ctypes.data, rp.ctypes.data, ri.ctypes.data))
            self.n_owned = part.n_owned
            return
        if group == "local-only":                      # tests: owned/ghost split without a communicator
            box = [None]
        else:
            import torch.distributed as dist
            uid = C.create_string_buffer(128)
            if part.rank == 0:
                check(self.lib.sns_comm_unique_id(uid))
            box = [bytes(uid.raw)]
            if part.nranks > 1:
                dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0,
                                           group=group)
        with torch.cuda.device(self.device):
            check(self.lib.sns_attach_comm(self.h, part.rank, part.nranks, box[0], part.n_owned, len(nb),
                                           nb.ctypes.data, sp_.ctypes.data, si.ctypes.data, rp.ctypes.data,
                                           ri.ctypes.data))
        self.n_owned = part.n_owned

    def scatter(self, x_global) -> torch.Tensor:
        """Local (owned + ghost) device copy of a global host dof vector."""
        from . import partition as PT
        xg = np.asarray(x_global, dtype=np.float64)
        return torch.from_numpy(PT.scatter_global(self.part, xg) if self.part is not None else xg.copy()).to(self.device)

    def gather(self, x_local) -> torch.Tensor:
        """Global dof vector on every rank from the owned parts (setup / output only)."""
        from . import partition as PT
        if self.part is None or self.part.nranks == 1:
            if self.part is None:
                return x_local.clone()
            out = torch.zeros(4 * len(self.part.l2g), dtype=x_local.dtype, device=x_local.device)
            out.view(-1, 4)[torch.as_tensor(self.part.l2g, device=x_local.device)] = x_local.view(-1, 4)
            return out
        ng = self.global_mesh.num_nodes if self.global_mesh is not None else self.n_global_nodes
        return PT.gather_owned(self.part, x_local, ng, self.group.dist_group if isinstance(self.group, PeerGroup) else self.group)

    def eval_at(self, w, pts, padding: float = 1e-6) -> np.ndarray:
        """Nodal [ux, uy, uz, p] of the solution ``w`` at the points ``pts`` (m,3) -> (m,4) numpy: point location and P1
        evaluation on this problem's device (interpolate.eval_points; what ``Function.eval`` with a bounding-box tree gives a
        DOLFINx user).  Single-GPU 3-D problems only."""
        from .interpolate import eval_points
        if self.part is not None:
            raise NotImplementedError("eval_at covers single-GPU problems: a partitioned problem holds only its rank's part of "
                                      "the mesh; gather the solution and evaluate it on the global mesh with "
                                      "interpolate.eval_points")
        if self.dim != 3:
            raise NotImplementedError("eval_at covers 3-D tet meshes only")
        return eval_points(self.mesh, self._vec(w).view(-1, 4), pts, self.device, padding)

    # -- lifetime -----------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.sns_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers ------------------------------------------------------------
    @property
    def ndof(self) -> int:
        return 4 * self.n_local

    def zeros(self) -> torch.Tensor:
        return torch.zeros(self.ndof, dtype=torch.float64, device=self.device)

    def _vec(self, x) -> torch.Tensor:
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(self.device)
        if x.dtype != torch.float64 or x.device.type != "cuda" or not x.is_contiguous() or x.numel() != self.ndof:
            raise ValueError(f"expected a contiguous float64 device vector of {self.ndof} entries")
        return x

    def set_options(self, **kw):
        for k, v in kw.items():
            if k == "ksp_type" and isinstance(v, str):
                v = _lib.KSP_NAMES[v]
            if k == "pc_type" and isinstance(v, str):
                v = _lib.PC_NAMES[v]
            if not hasattr(self.options, k):
                raise TypeError(f"unknown option {k}")
            setattr(self.options, k, v)
        check(self.lib.sns_set_options(self.h, C.byref(self.options)))

    def set_form_variant(self, c_inverse=36.0, lsic_scale=1.0, pspg_sign=1.0, one_point_quadrature=False):
        """DIAGNOSTIC: perturb the 3-D NS form (sns_set_form_variant); the defaults restore the reference's form."""
        check(self.lib.sns_set_form_variant(self.h, float(c_inverse), float(lsic_scale), float(pspg_sign), int(bool(one_point_quadrature))))

    # -- hot path -------------------------------------------------------------
    def residual(self, w, form="ns", out=None) -> torch.Tensor:
        """F(w) as the reference's .F callback leaves it (:51-67)."""
        w = None if w is None else self._vec(w)
        out = self.zeros() if out is None else self._vec(out)
        check(self.lib.sns_residual(self.h, _FORMS[form], _ptr(w), _ptr(out)))
        return out

    def jacobian(self, w, form="ns", residual_out=None):
        """Assemble J(w) into the handle (:69-75); optionally the fused residual."""
        w = None if w is None else self._vec(w)
        F = None if residual_out is None else self._vec(residual_out)
        check(self.lib.sns_jacobian(self.h, _FORMS[form], _ptr(w), _ptr(F)))
        return F

    def residual_moments(self, w, phi, form="ns") -> np.ndarray:
        """sum_i phi_i R_raw(w)[4 i + c], c = 0..3, over the owned nodes of every rank (sns_residual_moments): R_raw is the
        residual without lifting and without the Dirichlet rows' w_B - g, so ``-out[:3]`` is the force on the surface whose
        node indicator is ``phi`` (functionals.reaction_force).  ``phi``: numpy or a device tensor, one weight per local node
        (owned + ghost, the handle's numbering).  ``w`` may violate its Dirichlet data; None evaluates the Stokes form at 0."""
        w = None if w is None else self._vec(w)
        if isinstance(phi, np.ndarray):
            phi = torch.from_numpy(np.ascontiguousarray(phi, dtype=np.float64)).to(self.device)
        if phi.dtype != torch.float64 or phi.device.type != "cuda" or not phi.is_contiguous() or phi.numel() != self.n_local:
            raise ValueError(f"phi: expected a contiguous float64 vector of {self.n_local} node weights")
        out = (C.c_double * 4)()
        check(self.lib.sns_residual_moments(self.h, _FORMS[form], _ptr(w), _ptr(phi), out))
        return np.array(out[:], dtype=np.float64)

    def residual_shape_gradient(self, w, lam, form="ns") -> torch.Tensor:
        """``lam . dR_raw(w; X)/dX`` as a device tensor (n_nodes, 3) (sns_residual_shape_gradient): the derivative of the raw
        residual (no lifting, no Dirichlet rows' w_B - g) with respect to every node coordinate, contracted with the dof vector
        ``lam``, at fixed state, Dirichlet values, nu and time-term history.  ``lam`` is used as given -- zero the Dirichlet
        rows of an adjoint vector first (``solver.shape_sensitivity`` does).  One element pass, exact derivative, bitwise
        reproducible; the z column of a 2-D problem is 0.  NS form only; single-GPU problems.  Overwrites the handle's
        element scratch (``export(SNS_EXPORT_FE, ...)``), nothing else."""
        w, lam = self._vec(w), self._vec(lam)
        out = torch.empty(self.n_local, 3, dtype=torch.float64, device=self.device)
        check(self.lib.sns_residual_shape_gradient(self.h, _FORMS[form], _ptr(w), _ptr(lam), _ptr(out)))
        return out

    def _recover(self, w, want_G: bool, want_D: bool):
        w = self._vec(w)
        G = torch.empty(self.n_local, 4, 3, dtype=torch.float64, device=self.device) if want_G else None
        D = torch.empty(self.n_local, 6, dtype=torch.float64, device=self.device) if want_D else None
        check(self.lib.sns_recover_gradient(self.h, _ptr(w), _ptr(G), _ptr(D)))
        return G, D

    def recover_gradient(self, w) -> torch.Tensor:
        """The gradient of the P1 state recovered at the nodes, a device tensor (n_nodes, 4, 3) (sns_recover_gradient):
        ``G[i, c, j]`` = the volume-weighted mean over the cells of node i of d_j w_c, c in (u_x, u_y, u_z, p) -- the lumped-mass
        L2 projection of the piecewise-constant gradient onto P1.  One pass over the node-to-cell lists in a fixed order: no
        atomics, bitwise reproducible.  2-D problems: column j = 2 is 0.  Reads ``w`` and the mesh only; single-GPU problems."""
        return self._recover(w, True, False)[0]

    def derived_fields(self, w) -> torch.Tensor:
        """Nodal fields derived from the recovered velocity gradient, a device tensor (n_nodes, 6): columns 0..2 the vorticity
        curl u, 3 the Q-criterion (|Omega|^2 - |S|^2) / 2, 4 the shear rate sqrt(2 S:S), 5 div u (S, Omega the symmetric and
        skew parts of the recovered gradient).  The gradient itself stays in registers and is not stored.  The shear rate is the
        recovered nodal value, not the per-cell value of ``element_viscosity``."""
        return self._recover(w, False, True)[1]

    def error_indicator(self, w, G=None):
        """Zienkiewicz-Zhu indicator per cell over the velocity components (sns_error_indicator): ``(eta2, gnorm2)``, device
        tensors of length n_cells, eta2[t] = int_t |G_h(u) - grad u_h|^2 (exact) and gnorm2[t] = |t| |grad u_h|^2.  ``G``: the
        tensor of ``recover_gradient(w)``; None recovers it into a temporary of the handle (same bits)."""
        w = self._vec(w)
        if G is not None and (G.dtype != torch.float64 or G.device.type != "cuda" or not G.is_contiguous()
                              or G.numel() != 12 * self.n_local):
            raise ValueError(f"expected a contiguous float64 device tensor of {12 * self.n_local} entries")
        E = len(self.mesh.tris if self.dim == 2 else self.mesh.tets)
        eta2 = torch.empty(E, dtype=torch.float64, device=self.device)
        gn2 = torch.empty(E, dtype=torch.float64, device=self.device)
        check(self.lib.sns_error_indicator(self.h, _ptr(w), _ptr(G), _ptr(eta2), _ptr(gn2)))
        return eta2, gn2

    # -- linear stability (no counterpart in the reference) -----------------------------------------------------------
    def mass_apply(self, w, x, out=None) -> torch.Tensor:
        """``B(w) x`` (sns_mass_apply): B = dR/du_t of the present 3-D NS form at the state ``w`` -- Galerkin mass plus the SUPG
        and PSPG parts of u_t, with the form's tau, form variant and viscosity field -- applied matrix-free in one pass, bitwise
        reproducible.  Rows of constrained dofs are 0; pressure and constrained entries of ``x`` are ignored.  Single-GPU 3-D
        problems."""
        w, x = self._vec(w), self._vec(x)
        out = self.zeros() if out is None else self._vec(out)
        check(self.lib.sns_mass_apply(self.h, _ptr(w), _ptr(x), _ptr(out)))
        return out

    def mass_apply_transpose(self, w, z, out=None) -> torch.Tensor:
        """``B(w)^T z`` (sns_mass_apply_transpose): the transpose of the operator of ``mass_apply``, matrix-free in one pass,
        bitwise reproducible -- the mass pass of the left (adjoint) eigenproblem J^T z = -lam B^T z.  Unlike ``mass_apply`` it
        reads the pressure entries of ``z`` (the PSPG rows of B); constrained entries of ``z`` are read as 0.  Pressure rows
        and rows of constrained dofs are 0.  Single-GPU 3-D problems."""
        w, z = self._vec(w), self._vec(z)
        out = self.zeros() if out is None else self._vec(out)
        check(self.lib.sns_mass_apply_transpose(self.h, _ptr(w), _ptr(z), _ptr(out)))
        return out

    def jacobian_state_gradient(self, w, x, z, c_jac: float = 1.0, c_mass: float = 0.0, out=None) -> torch.Tensor:
        """The Hessian pass (sns_jacobian_state_gradient): ``g = grad_w [ z~^T (c_jac J(w) + c_mass B(w)) x~ ]`` for real dof
        vectors ``x``, ``z`` held fixed -- J the steady Jacobian of the present 3-D NS form (form variant, corrected_convection,
        a viscosity field held fixed), B the operator of ``mass_apply``, x~ and z~ the vectors with every constrained entry read
        as 0.  g is 0 on constrained dofs; its pressure rows are not zero in general.  One element pass, bitwise reproducible;
        nothing of the problem besides the element scratch is written.  Refused (SnsError) with a body force, a backflow
        coefficient, a time term or a viscosity law set; a boundary traction alone is allowed.  Single-GPU 3-D problems."""
        w, x, z = self._vec(w), self._vec(x), self._vec(z)
        out = self.zeros() if out is None else self._vec(out)
        check(self.lib.sns_jacobian_state_gradient(self.h, _ptr(w), _ptr(x), _ptr(z), float(c_jac), float(c_mass), _ptr(out)))
        return out

    def jacobian_shape_gradient(self, w, x, z, c_jac: float = 1.0, c_mass: float = 0.0, out=None) -> torch.Tensor:
        """The eigenvalue shape pass (sns_jacobian_shape_gradient): ``gX = d/dX [ z~^T (c_jac J0(w; X) + c_mass B(w; X)) x~ ]``
        as a device tensor (n_nodes, 3), the derivative of the contraction of ``jacobian_state_gradient`` with respect to every
        node coordinate at fixed ``w``, ``x``, ``z``, Dirichlet values (held at the nodes) and viscosity.  x~ and z~ are the
        vectors with every constrained entry read as 0; their pressure entries matter.  One element pass, exact derivative,
        bitwise reproducible; overwrites the problem's element scratch (``export(SNS_EXPORT_FE, ...)``), nothing else.
        Refused (SnsError) as ``jacobian_state_gradient`` is: with a body force, a backflow coefficient, a time term or a
        viscosity law set; a boundary traction alone and a viscosity field are allowed.  Single-GPU 3-D problems."""
        w, x, z = self._vec(w), self._vec(x), self._vec(z)
        if out is None:
            out = torch.empty(self.n_local, 3, dtype=torch.float64, device=self.device)
        elif out.dtype != torch.float64 or out.device.type != "cuda" or not out.is_contiguous() or out.numel() != 3 * self.n_local:
            raise ValueError(f"out: expected a contiguous float64 device tensor of {3 * self.n_local} entries")
        check(self.lib.sns_jacobian_shape_gradient(self.h, _ptr(w), _ptr(x), _ptr(z), float(c_jac), float(c_mass), _ptr(out)))
        return out

    def raw_jacobian_apply(self, w, x, transpose: bool = False, out=None) -> torch.Tensor:
        """``J0(w) x``, or ``J0(w)^T x`` with ``transpose`` (sns_raw_jacobian_apply): J0 = dR_raw/dw, the Jacobian of the raw NS
        residual of ``residual_moments`` -- no lifting, no Dirichlet rows, no mask anywhere: ``x`` is used as given on
        constrained dofs and every row of the result is written; ``w`` need not satisfy its Dirichlet data.  The pass follows
        corrected_convection, a set time term, the Carreau law, a body force and a viscosity field as the assembly does, and on
        the free x free blocks it is the assembled Jacobian's arithmetic.  Matrix-free, one pass, bitwise reproducible; nothing
        of the problem is written.  2-D problems: the u_z rows and columns are 0.  Refused (SnsError) with a backflow
        coefficient or a perturbed form variant set, with ``out`` the same tensor as ``x``, and on partitioned problems."""
        w, x = self._vec(w), self._vec(x)
        out = self.zeros() if out is None else self._vec(out)
        check(self.lib.sns_raw_jacobian_apply(self.h, FORM_NS, _ptr(w), _ptr(x), int(bool(transpose)), _ptr(out)))
        return out

    def set_dirichlet_values(self, g):
        """New Dirichlet VALUES for this problem (sns_set_dirichlet_values): ``g`` holds 4 * n_nodes entries (numpy or a
        tensor); the mask stays, entries of unconstrained dofs are ignored, the u_z slots of a 2-D problem stay 0.  Every later
        residual, Jacobian and solve takes them, bit for bit as a problem created with them; an assembled matrix stays what it
        was.  Refreshes the host copy ``bc_val`` and the device copy ``g_dev``.  A non-finite value on a constrained dof is
        refused and leaves the problem untouched.  Single-GPU problems."""
        if isinstance(g, torch.Tensor):
            g = g.detach().cpu().numpy()
        g = np.ascontiguousarray(g, dtype=np.float64).ravel()
        if g.shape != (self.ndof,):
            raise ValueError(f"expected {self.ndof} Dirichlet values")
        check(self.lib.sns_set_dirichlet_values(self.h, g.ctypes.data))
        B = self.bc_mask.astype(bool)
        val = self.bc_val.copy()
        val[B] = g[B]
        if self.dim == 2:
            val[2::4] = 0.0
        self.bc_val = val
        self.g_dev = torch.from_numpy(self.bc_val).to(self.device)

    def _arnoldi_basis(self, m, start):
        """``(m, V, H)`` of a fresh Arnoldi process: V zero but for row 0, the start vector (by default cos(1 + 0.37 i) over the
        dofs), H zero.  (m outside [2, 64]: the library refuses.)"""
        m = int(m)
        V = torch.zeros(max(m, 0) + 1, self.ndof, dtype=torch.float64, device=self.device)
        if start is None:
            V[0] = torch.cos(1.0 + 0.37 * torch.arange(self.ndof, dtype=torch.float64, device=self.device))
        else:
            V[0] = self._vec(start)
        return m, V, np.zeros((max(m, 0) + 1, max(m, 0)))

    def _check_basis(self, V, H, who: str) -> int:
        """The ``V`` and ``H`` a caller hands back to the method ``who`` are the ones it was given; returns m."""
        if not (isinstance(H, np.ndarray) and H.dtype == np.float64 and H.ndim == 2 and H.flags.c_contiguous and
                H.shape[0] == H.shape[1] + 1):
            raise ValueError(f"H must be the C-contiguous float64 (m + 1, m) array of {who}")
        m = H.shape[1]
        if not (isinstance(V, torch.Tensor) and V.dtype == torch.float64 and V.shape == (m + 1, self.ndof) and V.is_contiguous()
                and V.device.type == "cuda"):
            raise ValueError(f"V must be the contiguous float64 (m + 1, ndof) device tensor of {who}")
        return m

    def stability_arnoldi(self, w, shift: float = 0.0, m: int = 64, start=None, breakdown_rel: float = 1e-6, side: str = "right"):
        """``m`` steps of shift-invert Arnoldi on (J + shift B)^-1 B at the steady state ``w`` (sns_stability_arnoldi), with
        the problem's ksp / pc options for the inner solves.  Returns ``(V, H, ArnoldiResult)``: V a device tensor
        (m + 1, ndof) whose rows are the orthonormal basis, H numpy (m + 1, m).  ``start``: a dof vector, by default
        cos(1 + 0.37 i) over the dofs.  Afterwards the handle's matrix is J + shift B and its form is steady again.
        ``side="left"``: the same process on (J + shift B)^-T B^T (sns_stability_arnoldi_left), whose Ritz vectors are the
        left (adjoint) modes; the operator is transposed for the call and transposed back."""
        if side not in ("right", "left"):
            raise ValueError("side must be 'right' or 'left'")
        run = self.lib.sns_stability_arnoldi if side == "right" else self.lib.sns_stability_arnoldi_left
        w = self._vec(w)
        m, V, H = self._arnoldi_basis(m, start)
        done, its, reason = C.c_int(), C.c_int(), C.c_int()
        check(run(self.h, _ptr(w), float(shift), m, float(breakdown_rel), _ptr(V), H.ctypes.data, C.byref(done), C.byref(its),
                  C.byref(reason)))
        return V, H, ArnoldiResult(done.value, reason.value, its.value)

    def stability_arnoldi_extend(self, w, V, H, k: int, shift: float = 0.0, breakdown_rel: float = 1e-6, side: str = "right"):
        """Continue the Krylov decomposition a previous ``stability_arnoldi`` (or this method) left in ``V`` (device tensor
        (m + 1, ndof)) and ``H`` (numpy (m + 1, m)) from column ``k`` (sns_stability_arnoldi_extend): rows 0 .. k of V orthonormal
        with zeros on the constrained dofs, H[:k + 1, :k] with S V_k = V_{k+1} H_k -- what ``krylov_schur_truncate`` and
        ``basis_rotate`` leave; the contract is the caller's and is not verified.  Both are modified in place: steps k .. m - 1
        run as in ``stability_arnoldi`` (same ``w``, ``shift`` and ``side`` as the run being continued), orthogonalising
        against every earlier column, so H is no longer Hessenberg: use ``krylov_ritz_pairs``.  Returns ``ArnoldiResult``
        (m_done = k + the steps completed; ksp_its of this call).  The handle ends as after ``stability_arnoldi``."""
        if side not in ("right", "left"):
            raise ValueError("side must be 'right' or 'left'")
        m = self._check_basis(V, H, "stability_arnoldi")
        w = self._vec(w)
        done, its, reason = C.c_int(), C.c_int(), C.c_int()
        check(self.lib.sns_stability_arnoldi_extend(self.h, _ptr(w), float(shift), int(k), m, float(breakdown_rel), int(side == "left"),
                                                    _ptr(V), H.ctypes.data, C.byref(done), C.byref(its), C.byref(reason)))
        return ArnoldiResult(done.value, reason.value, its.value)

    def basis_rotate(self, V, Q):
        """``V[:n_out] <- Q^T V[:n_in]`` in place, i.e. the basis vectors (the rows of ``V``, as ``stability_arnoldi`` returns
        them) recombined by the columns of ``Q`` (numpy (n_in, n_out), n_out <= n_in <= 65), then rows n_out .. n_in - 1 zeroed;
        rows from n_in on stay (sns_basis_rotate, k_basis_rotate).  No second copy of V is made; bitwise reproducible."""
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        if Q.ndim != 2:
            raise ValueError("Q must be (n_in, n_out)")
        n_in, n_out = Q.shape
        if not (isinstance(V, torch.Tensor) and V.dtype == torch.float64 and V.ndim == 2 and V.shape[1] == self.ndof and
                V.is_contiguous() and V.device.type == "cuda"):
            raise ValueError("V must be a contiguous float64 (rows, ndof) device tensor")
        if V.shape[0] < n_in:
            raise ValueError(f"V has {V.shape[0]} rows, Q asks for {n_in}")
        check(self.lib.sns_basis_rotate(self.h, n_in, n_out, Q.ctypes.data, _ptr(V)))
        return V

    # -- complex and negative shifts: the library's complex vectors are planar (real parts, then imaginary parts) --------
    def _planar(self, x) -> torch.Tensor:
        """A complex (or real) dof vector as the planar float64 tensor of 2 * ndof the library reads."""
        if not isinstance(x, torch.Tensor):
            x = torch.as_tensor(np.asarray(x))
        x = x.to(self.device)
        if x.shape != (self.ndof,):
            raise ValueError(f"expected a dof vector of {self.ndof} entries")
        if x.is_complex():
            return torch.cat([x.real.to(torch.float64), x.imag.to(torch.float64)]).contiguous()
        return torch.cat([x.to(torch.float64), torch.zeros(self.ndof, dtype=torch.float64, device=self.device)]).contiguous()

    def _unplanar(self, y) -> torch.Tensor:
        return torch.complex(y[:self.ndof], y[self.ndof:])

    def shifted_apply(self, w, c, x, transpose: bool = False) -> torch.Tensor:
        """``A x + c B(w) x`` for a complex scalar ``c`` and a complex dof vector ``x`` (sns_shifted_apply): A is the matrix the
        problem holds as it stands -- after ``jacobian(w)`` the Jacobian J, after a stability run J + pc_shift B --, B the
        operator of ``mass_apply``, with ``transpose`` that of ``mass_apply_transpose`` (the caller flips A itself:
        ``transpose_operator``).  Two operator passes and one pair mass pass, bitwise reproducible; with c = 0 the bits of
        ``spmv`` on each part.  Returns a complex128 device tensor.  Single-GPU 3-D problems."""
        w, xp = self._vec(w), self._planar(x)
        c = complex(c)
        out = torch.empty_like(xp)
        check(self.lib.sns_shifted_apply(self.h, _ptr(w), c.real, c.imag, int(bool(transpose)), _ptr(xp), _ptr(out)))
        return self._unplanar(out)

    def shifted_solve(self, w, c, b, x0=None, transpose: bool = False):
        """``(A + c B(w)) x = b`` by right-preconditioned complex FGMRES (sns_shifted_solve) with the problem's gmres_restart,
        ksp_rtol / ksp_atol / ksp_max_it and the preconditioner of A on each part; A and ``transpose`` as in
        ``shifted_apply``.  Returns (x complex128, KrylovResult); ``rnorm`` is the true residual norm, a solve that did not
        converge says so in ``reason`` and leaves the problem usable."""
        w, bp = self._vec(w), self._planar(b)
        c = complex(c)
        x = torch.zeros_like(bp) if x0 is None else self._planar(x0)
        its, reason, rn = C.c_int(), C.c_int(), C.c_double()
        check(self.lib.sns_shifted_solve(self.h, _ptr(w), c.real, c.imag, int(bool(transpose)), _ptr(bp), _ptr(x), C.byref(its),
                                         C.byref(reason), C.byref(rn)))
        return self._unplanar(x), KrylovResult(its.value, reason.value, rn.value)

    def stability_arnoldi_shifted(self, w, shift, pc_shift: Optional[float] = None, m: int = 64, start=None,
                                  breakdown_rel: float = 1e-6, side: str = "right", V=None, H=None, k: int = 0):
        """Shift-invert Arnoldi with a complex or negative ``shift`` s in real arithmetic (sns_stability_arnoldi_shifted): the
        process of ``stability_arnoldi`` on Re[(J + s B)^-1 B] (``side="left"``: Re[(J + s B)^-T B^T]), whose basis and H are
        real.  The problem assembles and preconditions P = J + pc_shift B (``pc_shift`` >= 0, by default |s|); each step solves
        the complex system (P + (s - pc_shift) B) y = B v (``shifted_solve``'s method) and keeps Re y.  ``k = 0``: a fresh
        process, returns ``(V, H, ArnoldiResult)`` as ``stability_arnoldi``.  ``k >= 1`` with the ``V`` and ``H`` of an earlier
        call: the continuation of ``stability_arnoldi_extend``, in place.  The eigenvalues follow from H by
        ``solver.shifted_eigenpairs``, not ``ritz_pairs``.  Afterwards the problem's matrix is J + pc_shift B."""
        if side not in ("right", "left"):
            raise ValueError("side must be 'right' or 'left'")
        s = complex(shift)
        pc_shift = abs(s) if pc_shift is None else float(pc_shift)
        w = self._vec(w)
        if V is None:
            m, V, H = self._arnoldi_basis(m, start)
        else:
            m = self._check_basis(V, H, "stability_arnoldi_shifted")
        done, its, reason = C.c_int(), C.c_int(), C.c_int()
        check(self.lib.sns_stability_arnoldi_shifted(self.h, _ptr(w), s.real, s.imag, pc_shift, int(k), m, float(breakdown_rel),
                                                     int(side == "left"), _ptr(V), H.ctypes.data, C.byref(done), C.byref(its),
                                                     C.byref(reason)))
        return V, H, ArnoldiResult(done.value, reason.value, its.value)

    # -- resolvent analysis (no counterpart in the reference) ----------------------------------------------------------
    def _nodal_weight(self, weight, name: str):
        """A nodal weight (n_local entries, numpy or a tensor) as a contiguous float64 device tensor; None stays None."""
        if weight is None:
            return None
        if not isinstance(weight, torch.Tensor):
            weight = torch.as_tensor(np.asarray(weight, dtype=np.float64))
        weight = weight.to(self.device, torch.float64).contiguous()
        if weight.shape != (self.n_local,):
            raise ValueError(f"{name}: expected one weight per node ({self.n_local})")
        return weight

    def energy_apply(self, x, weight=None) -> torch.Tensor:
        """``Q x`` with Q = D M D (sns_energy_apply): M the consistent P1 Galerkin mass matrix on the three velocity
        components, D the nodal ``weight`` (one entry per node; None: all ones), so that x^H Q x is the kinetic energy of the
        weighted field.  ``x``: a real dof vector (the result is float64) or a complex one (complex128; each part is summed
        exactly as a real vector is).  Matrix-free in one pass, bitwise reproducible; constrained entries of ``x`` are read as
        0, pressure entries are not read, constrained and pressure rows of the result are 0.  Single-GPU 3-D problems."""
        chi = self._nodal_weight(weight, "weight")
        if x.is_complex() if isinstance(x, torch.Tensor) else np.iscomplexobj(x):
            xp = self._planar(x)
            out = torch.empty_like(xp)
            check(self.lib.sns_energy_apply(self.h, _ptr(chi), 2, _ptr(xp), _ptr(out)))
            return self._unplanar(out)
        x = self._vec(x)
        out = self.zeros()
        check(self.lib.sns_energy_apply(self.h, _ptr(chi), 1, _ptr(x), _ptr(out)))
        return out

    def lumped_volumes(self) -> torch.Tensor:
        """The lumped nodal volumes as a dof vector (sns_lumped_volumes): a quarter of the incident tets' volumes in the three
        velocity slots of every node, 0 in its pressure slot; no mask.  Bitwise reproducible.  Single-GPU 3-D problems."""
        out = self.zeros()
        check(self.lib.sns_lumped_volumes(self.h, _ptr(out)))
        return out

    def resolvent_lanczos(self, w, omega: float, m: int = 24, start=None, breakdown_rel: float = 1e-6, forcing_weight=None,
                          response_weight=None):
        """``m`` steps of the Hermitian Krylov process on T = S B^T (J + i omega B)^-H Q (J + i omega B)^-1 B S at the steady
        state ``w`` (sns_resolvent_lanczos), whose eigenvalues are the squared resolvent gains: Q the operator of
        ``energy_apply`` with ``response_weight``, S = D_f M_L^-1/2 with M_L the ``lumped_volumes`` and D_f the
        ``forcing_weight`` (nodal weights; None: all ones).  The inner solves take the problem's ksp / pc options.  Returns
        ``(V, H, ArnoldiResult)``: V a complex128 device tensor (m + 1, ndof) whose rows are the orthonormal basis, H numpy
        complex (m + 1, m) with T V_m = V_{m+1} H.  ``start``: a real or complex dof vector, by default cos(1 + 0.37 i) over
        the dofs; its pressure and constrained entries are zeroed.  Afterwards the problem's matrix is J, untransposed and set
        up.  An inner solve that does not converge ends the process quietly: ``reason`` < 0, ``m_done`` the steps completed."""
        w = self._vec(w)
        m = int(m)
        chi_f, chi_q = self._nodal_weight(forcing_weight, "forcing_weight"), self._nodal_weight(response_weight, "response_weight")
        V = torch.zeros(max(m, 0) + 1, 2 * self.ndof, dtype=torch.float64, device=self.device)
        if start is None:
            V[0, :self.ndof] = torch.cos(1.0 + 0.37 * torch.arange(self.ndof, dtype=torch.float64, device=self.device))
        else:
            V[0] = self._planar(start)
        H = np.zeros((max(m, 0) + 1, max(m, 0)), dtype=np.complex128)
        done, its, reason = C.c_int(), C.c_int(), C.c_int()
        check(self.lib.sns_resolvent_lanczos(self.h, _ptr(w), float(omega), m, float(breakdown_rel), _ptr(chi_f), _ptr(chi_q), _ptr(V),
                                             H.ctypes.data, C.byref(done), C.byref(its), C.byref(reason)))
        return torch.complex(V[:, :self.ndof], V[:, self.ndof:]), H, ArnoldiResult(done.value, reason.value, its.value)

    def spmv(self, x, out=None) -> torch.Tensor:
        x = self._vec(x)
        out = self.zeros() if out is None else self._vec(out)
        check(self.lib.sns_spmv(self.h, _ptr(x), _ptr(out)))
        return out

    def pc_setup(self):
        check(self.lib.sns_pc_setup(self.h))

    def pc_apply(self, r, out=None) -> torch.Tensor:
        r = self._vec(r)
        out = self.zeros() if out is None else self._vec(out)
        check(self.lib.sns_pc_apply(self.h, _ptr(r), _ptr(out)))
        return out

    def krylov_solve(self, b, x0=None):
        b = self._vec(b)
        x = self.zeros() if x0 is None else self._vec(x0).clone()
        its, reason, rn = C.c_int(), C.c_int(), C.c_double()
        check(self.lib.sns_krylov_solve(self.h, _ptr(b), _ptr(x), C.byref(its), C.byref(reason), C.byref(rn)))
        return x, KrylovResult(its.value, reason.value, rn.value)

    def transpose_operator(self):
        """Flip the assembled fine operator in place between A and A^T (sns_transpose_operator): ``spmv``, ``pc_setup``,
        ``pc_apply``, ``krylov_solve``, ``bsr`` and ``to_scipy`` then act on A^T until the next call or the next assembly
        (``jacobian``, ``stokes_solve``, ``newton_solve``), which restores A.  Single-GPU problems only."""
        check(self.lib.sns_transpose_operator(self.h))

    @property
    def operator_transposed(self) -> bool:
        f = C.c_int()
        check(self.lib.sns_operator_is_transposed(self.h, C.byref(f)))
        return bool(f.value)

    def adjoint_solve(self, g, x0=None):
        """A^T lam = g with the operator the handle holds and its ksp / pc options (sns_adjoint_solve: transpose, set-up,
        Krylov solve, transpose back); the handle holds A again afterwards.  Returns (lam, KrylovResult) like
        ``krylov_solve``; ``rnorm`` is the true residual norm ||g - A^T lam||."""
        g = self._vec(g)
        x = self.zeros() if x0 is None else self._vec(x0).clone()
        its, reason, rn = C.c_int(), C.c_int(), C.c_double()
        check(self.lib.sns_adjoint_solve(self.h, _ptr(g), _ptr(x), C.byref(its), C.byref(reason), C.byref(rn)))
        return x, KrylovResult(its.value, reason.value, rn.value)

    def stokes_solve(self):
        U = self.zeros()
        its, reason, rn = C.c_int(), C.c_int(), C.c_double()
        check(self.lib.sns_stokes_solve(self.h, _ptr(U), C.byref(its), C.byref(reason), C.byref(rn)))
        return U, KrylovResult(its.value, reason.value, rn.value)

    def newton_solve(self, w):
        w = self._vec(w)
        its, reason, kits = C.c_int(), C.c_int(), C.c_int()
        cap = self.options.snes_max_it + 2
        hist = (C.c_double * cap)()
        t0 = time.time()
        check(self.lib.sns_newton_solve(self.h, _ptr(w), C.byref(its), C.byref(reason), C.byref(kits), hist, cap))
        dt = time.time() - t0
        return w, NewtonResult(its.value, reason.value, kits.value, list(hist[:its.value + 1]), dt)

    # -- time stepping (no counterpart in the reference, whose forms are all steady) ---------------------------------
    def set_time_term(self, sigma: float, theta: float, d):
        """Every NS assembly of this problem from now on takes the transient form with u_t = sigma u + d
        (sns_set_time_term): (u_t, v) in the Galerkin part, res_M + u_t in the SUPG / PSPG term, theta under the root of
        tau.  ``d``: a dof vector (numpy or device; pressure slots ignored, copied by the handle) or None for d = 0.
        Single-GPU 3-D problems."""
        d = None if d is None else self._vec(d)
        check(self.lib.sns_set_time_term(self.h, float(sigma), float(theta), _ptr(d)))

    def clear_time_term(self):
        """Back to the steady form, bit for bit."""
        check(self.lib.sns_set_time_term(self.h, 0.0, 0.0, None))

    def time_step(self, w, wprev, dt: float, order: int = 2, theta_coeff: float = 4.0):
        """One BDF step (sns_time_step): on entry ``w`` = u^n (with p^n as the pressure guess) and ``wprev`` = u^(n-1)
        (None allowed for order 1); on exit ``w`` = u^(n+1) and ``wprev`` = u^n, both updated in place.  theta =
        theta_coeff / dt^2 enters tau.  A step that does not converge (``reason`` <= 0) leaves both as they were.  The
        time term stays set, so ``residual_moments`` gives the force consistent with the step.  Returns (w, NewtonResult)."""
        w = self._vec(w)
        wprev = None if wprev is None else self._vec(wprev)
        its, reason, kits = C.c_int(), C.c_int(), C.c_int()
        t0 = time.time()
        check(self.lib.sns_time_step(self.h, _ptr(w), _ptr(wprev), float(dt), int(order), float(theta_coeff), C.byref(its),
                                     C.byref(reason), C.byref(kits)))
        return w, NewtonResult(its.value, reason.value, kits.value, [], time.time() - t0)

    # -- generalised-Newtonian viscosity (no counterpart in the reference: nu = 1/Re everywhere) ----------------------
    def set_viscosity_law(self, lam: float, n: float, nu_inf_ratio: float = 0.0):
        """Every NS assembly of this problem from now on takes the Carreau law (sns_set_viscosity_law): on each tet
        nu_e = nu0 (r + (1 - r)(1 + lam^2 s)^((n-1)/2)) with s = 2 eps:eps, nu0 = 1/Re and r = ``nu_inf_ratio``; the viscous
        term becomes (2 nu_e eps(u), grad v), nu_e enters tau, the Jacobian stays the exact derivative.  n < 1 shear-thins.
        Single-GPU 3-D problems; not together with a time term."""
        check(self.lib.sns_set_viscosity_law(self.h, _lib.LAW_CARREAU, float(lam), float(n), float(nu_inf_ratio)))
        self.viscosity_law = (float(lam), float(n), float(nu_inf_ratio))

    def clear_viscosity_law(self):
        """Back to the Newtonian form of the reference, bit for bit."""
        check(self.lib.sns_set_viscosity_law(self.h, _lib.LAW_NEWTONIAN, 0.0, 1.0, 0.0))
        self.viscosity_law = None

    def element_viscosity(self, w):
        """(nu_e, gamma_dot) of the state ``w``: one value per tet, device tensors (sns_element_viscosity); nu_e = 1/Re
        everywhere without a law, the viscosity field where one is set."""
        w = self._vec(w)
        nt = self.sizes()["n_tets"]
        nu = torch.empty(nt, dtype=torch.float64, device=self.device)
        gd = torch.empty(nt, dtype=torch.float64, device=self.device)
        check(self.lib.sns_element_viscosity(self.h, _ptr(w), _ptr(nu), _ptr(gd)))
        return nu, gd

    # -- external fields of the 3-D NS form (no counterpart in the reference: no right-hand side, nu = 1/Re everywhere) ----
    def set_body_force(self, f):
        """Every NS assembly of this problem from now on has the nodal P1 force density ``f`` on the right-hand side of the
        momentum equation (sns_set_body_force): with a = u_t - f, (a, v) in the Galerkin part and res_M + a in the SUPG / PSPG
        term.  ``f``: a dof vector (numpy or device; pressure slots ignored, copied by the handle).  The viscous form is not
        changed.  Single-GPU 3-D problems; not together with a viscosity law."""
        check(self.lib.sns_set_body_force(self.h, _ptr(self._vec(f))))

    def clear_body_force(self):
        check(self.lib.sns_set_body_force(self.h, None))

    def set_element_viscosity(self, nu):
        """Every NS assembly of this problem from now on takes the per-tet viscosity ``nu`` (n_tets values, each finite and
        > 0; sns_set_element_viscosity): the viscous term becomes (2 nu_t eps(u), grad v), nu_t enters tau, the Jacobian is the
        exact derivative with nu_t held fixed.  Single-GPU 3-D problems; not together with a viscosity law."""
        if not isinstance(nu, torch.Tensor):
            nu = torch.from_numpy(np.ascontiguousarray(nu, dtype=np.float64))
        nu = nu.to(self.device, torch.float64).contiguous().reshape(-1)
        if nu.numel() != self.sizes()["n_tets"]:
            raise ValueError("set_element_viscosity: one value per tet")
        check(self.lib.sns_set_element_viscosity(self.h, _ptr(nu)))

    def clear_element_viscosity(self):
        check(self.lib.sns_set_element_viscosity(self.h, None))

    def set_mixture(self, m, log_viscosity_ratio: float = 0.0, buoyancy=(0.0, 0.0, 0.0)):
        """Both fields from a nodal P1 mixture fraction ``m`` (n values; sns_set_mixture): nu_t = (1/Re) exp(
        ``log_viscosity_ratio`` * mean of m over the tet's vertices) with the Reynolds number the problem has NOW, and f =
        m * ``buoyancy`` (Boussinesq, buoyancy = Ri * g_hat).  A zero log ratio clears the viscosity field, a zero buoyancy
        the body force, ``m`` = None both."""
        if m is not None:
            if not isinstance(m, torch.Tensor):
                m = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float64))
            m = m.to(self.device, torch.float64).contiguous().reshape(-1)
            if m.numel() != self.n_local:
                raise ValueError("set_mixture: one value per node")
        b = (C.c_double * 3)(*[float(x) for x in buoyancy])
        check(self.lib.sns_set_mixture(self.h, _ptr(m), float(log_viscosity_ratio), b))

    # -- boundary terms (no counterpart in the reference: its forms are volume integrals, its outlets do-nothing) -------
    def set_boundary_facets(self, facet_ids):
        """The boundary facets the facet terms live on (sns_set_boundary_facets): indices into ``mesh.facets``.  Replaces an
        earlier list and clears the data of ``set_boundary_flow`` / ``set_boundary_scalar`` (they are per facet); an empty list
        is ``clear_boundary_terms``.  Keeps ``boundary_facet_ids``, and per listed facet ``boundary_normals`` (outward unit
        normals: away from the fourth vertex of the owning tet) and ``boundary_areas``.  Per-facet and per-vertex data of the
        two setters is in the order of this list and of the vertices of ``mesh.facets``.  Single-GPU 3-D problems."""
        from .functionals import facet_parent_tets
        ids = np.asarray(facet_ids, dtype=np.int64).ravel()
        if len(ids) == 0:
            return self.clear_boundary_terms()
        if self.dim != 3:                                      # (the library's refusal, before the mesh is asked for tets)
            z3, z1 = np.zeros(3, np.int32), np.zeros(1, np.int64)
            check(self.lib.sns_set_boundary_facets(self.h, 1, z3.ctypes.data, z1.ctypes.data))
        fn = np.ascontiguousarray(self.mesh.facets[ids], dtype=np.int32)
        par = np.ascontiguousarray(facet_parent_tets(self.mesh, ids), dtype=np.int64)
        check(self.lib.sns_set_boundary_facets(self.h, len(ids), fn.ctypes.data, par.ctypes.data))
        P = self.mesh.points[fn.astype(np.int64)]
        cr = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
        opp = self.mesh.tets[par].astype(np.int64).sum(axis=1) - fn.astype(np.int64).sum(axis=1)
        cr *= np.sign(np.einsum("fi,fi->f", cr, P[:, 0] - self.mesh.points[opp]))[:, None]
        nrm = np.linalg.norm(cr, axis=1)
        self.boundary_facet_ids, self.boundary_normals, self.boundary_areas = ids, cr / nrm[:, None], 0.5 * nrm

    def _facet_count(self) -> int:
        ids = getattr(self, "boundary_facet_ids", None)
        return 0 if ids is None else len(ids)

    def _facet_dev(self, x):
        return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).ravel()).to(self.device)

    def set_boundary_flow(self, traction=None, pressure=None, backflow=None):
        """Every NS assembly of this problem from now on has, on the facets of ``set_boundary_facets`` (sns_set_boundary_flow),

            R(w; v) += - int t.v ds - int beta (u.n)_- u.v ds,      (u.n)_- = min(u.n, 0).

        ``traction``: (3,), (nf, 3) or (nf, 3, 3) [facet][vertex][component], P1 per facet -- the pseudo-traction nu d_n u - p n
        under the reference's viscous term, the true traction 2 nu eps(u) n - p n under a viscosity law or field.
        ``pressure``: a scalar or one value per facet, added as t = -p n (a pressure boundary).  ``backflow``: beta >= 0, a
        scalar or one value per facet; 0 switches the term off on that facet.  What is None is cleared; the Jacobian is the
        exact derivative with t and beta held fixed.  ``residual_shape_gradient`` is refused while either is set."""
        nf = self._facet_count()
        t = None
        if nf and (traction is not None or pressure is not None):
            t = np.zeros((nf, 3, 3))
            if traction is not None:
                tr = np.asarray(traction, dtype=np.float64)
                t += tr[:, None, :] if tr.shape == (nf, 3) else tr           # (3,) and (nf, 3, 3) broadcast as they are
            if pressure is not None:
                p = np.broadcast_to(np.asarray(pressure, dtype=np.float64), (nf,))
                t -= (p[:, None] * self.boundary_normals)[:, None, :]
        elif traction is not None or pressure is not None:
            t = np.zeros(1)                                     # (no facets: the library refuses)
        beta = None if backflow is None else np.broadcast_to(np.asarray(backflow, dtype=np.float64), (max(nf, 1),)).copy()
        t, beta = self._facet_dev(t), self._facet_dev(beta)
        check(self.lib.sns_set_boundary_flow(self.h, _ptr(t), _ptr(beta)))

    def set_boundary_scalar(self, alpha=None, ambient=None, flux=None):
        """Every ``scalar_system`` / ``scalar_solve`` of this problem from now on has, on the facets of ``set_boundary_facets``
        (sns_set_boundary_scalar), R_k(c; v) += int (alpha_k c_k - g_k) v ds with g = alpha c_ext + q, i.e. the Robin condition
        kappa d_n c = alpha (c_ext - c) + q.  For k species: ``alpha`` >= 0 a scalar, (k,) or (nf, k); ``ambient`` (c_ext) and
        ``flux`` (q) a scalar, (k,), (nf, k) or P1 per facet (nf, 3, k).  alpha = None with a flux is the Neumann condition
        kappa d_n c = q; all None clears both terms."""
        nf = max(self._facet_count(), 1)
        given = [np.asarray(x, dtype=np.float64) for x in (alpha, ambient, flux) if x is not None]
        k = max([x.shape[-1] for x in given if x.ndim >= 1] + [1])
        if not 1 <= k <= 4:
            raise ValueError("boundary scalar data: one to four species")
        if ambient is not None and alpha is None:
            raise ValueError("an ambient value needs alpha")

        def p1(x):                                             # -> (nf, 3, k)
            x = np.asarray(x, dtype=np.float64)
            return np.broadcast_to(x[:, None, :] if x.ndim == 2 else x, (nf, 3, k))

        a4 = g4 = None
        if alpha is not None:
            a4 = np.zeros((nf, 4))
            a4[:, :k] = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (nf, k))
        if ambient is not None or flux is not None:
            g4 = np.zeros((nf, 3, 4))
            if ambient is not None:
                g4[:, :, :k] += a4[:, None, :k] * p1(ambient)
            if flux is not None:
                g4[:, :, :k] += p1(flux)
        a4, g4 = self._facet_dev(a4), self._facet_dev(g4)
        check(self.lib.sns_set_boundary_scalar(self.h, _ptr(a4), _ptr(g4)))

    def clear_boundary_terms(self):
        """No facets and no boundary data: back to the forms without facet terms, bit for bit."""
        check(self.lib.sns_set_boundary_facets(self.h, 0, None, None))
        self.boundary_facet_ids = self.boundary_normals = self.boundary_areas = None

    # -- scalar transport on the flow mesh (no counterpart in the reference, which traces streamlines instead) --------
    def _scalar_inputs(self, w, kappa, bcs, source):
        """Device arguments of the two scalar entry points, padded to four species: the unused ones are constrained to 0
        on every node (identity rows) with kappa 1."""
        w = self._vec(w)
        kap = np.atleast_1d(np.asarray(kappa, dtype=np.float64)).ravel()
        k, n = len(kap), self.n_local
        if not 1 <= k <= 4:
            raise ValueError("kappa: one to four species")
        mask, val = bcs
        mask = np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask).astype(bool).reshape(n, -1)
        val = np.asarray(val.cpu() if isinstance(val, torch.Tensor) else val, dtype=np.float64).reshape(n, -1)
        if mask.shape != (n, k) or val.shape != (n, k):
            raise ValueError(f"scalar bcs: (mask, values), each of shape ({n}, {k})")
        m4, v4, k4 = np.ones((n, 4), np.uint8), np.zeros((n, 4)), np.ones(4)
        m4[:, :k], v4[:, :k], k4[:k] = mask, np.where(mask, val, 0.0), kap
        src = None
        if source is not None:
            src = torch.zeros(n, 4, dtype=torch.float64, device=self.device)
            src[:, :k] = self._columns(source, k)
        return (w, k, (C.c_double * 4)(*k4), torch.from_numpy(m4.ravel()).to(self.device),
                torch.from_numpy(v4.ravel()).to(self.device), src)

    def _columns(self, x, k) -> torch.Tensor:
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
        x = x.to(self.device, torch.float64).reshape(self.n_local, -1)
        if x.shape[1] != k:
            raise ValueError(f"expected shape ({self.n_local}, {k})")
        return x

    def scalar_system(self, w, kappa, bcs, *, sigma=0.0, theta=0.0, source=None) -> torch.Tensor:
        """Assemble the transport operator of ``len(kappa)`` (one to four) scalars carried by the velocity of the state ``w``
        into the handle and return its right-hand side (sns_scalar_system, where the form is written out): species k has
        diffusivity ``kappa[k]``; ``sigma`` (reaction / 1/dt) and ``theta`` (under the root of tau) are shared.  ``bcs`` =
        (mask, values), each (n, k): the scalars' own Dirichlet data; ``source``: nodal P1 source (n, k) or None.  The
        right-hand side comes back as a dof vector of 4 n entries in the node-blocked layout (species k at [k::4]; the slots
        of unused species hold 0), ready for ``krylov_solve`` / ``adjoint_solve``: the scalar operator is the handle's matrix
        until the next flow assembly (``jacobian``, ``stokes_solve``, ``newton_solve``).  Single-GPU 3-D problems."""
        w, _, kap, m, v, src = self._scalar_inputs(w, kappa, bcs, source)
        rhs = self.zeros()
        check(self.lib.sns_scalar_system(self.h, _ptr(w), kap, float(sigma), float(theta), _ptr(src), _ptr(m), _ptr(v), _ptr(rhs)))
        return rhs

    def scalar_solve(self, w, kappa, bcs, *, sigma=0.0, theta=0.0, source=None, c0=None):
        """``scalar_system`` + preconditioner set-up + the Krylov solve with the problem's options (sns_scalar_solve).
        ``c0``: initial guess (n, k), default 0.  Returns (c (n, k) device tensor, KrylovResult); a species without a
        Dirichlet node under sigma = 0 is singular and is not detected."""
        w, k, kap, m, v, src = self._scalar_inputs(w, kappa, bcs, source)
        c = torch.zeros(self.n_local, 4, dtype=torch.float64, device=self.device)
        if c0 is not None:
            c[:, :k] = self._columns(c0, k)
        its, reason, rn = C.c_int(), C.c_int(), C.c_double()
        check(self.lib.sns_scalar_solve(self.h, _ptr(w), kap, float(sigma), float(theta), _ptr(src), _ptr(m), _ptr(v), _ptr(c),
                                        C.byref(its), C.byref(reason), C.byref(rn)))
        return c[:, :k].contiguous(), KrylovResult(its.value, reason.value, rn.value)

    # -- introspection ----------------------------------------------------------
    def sizes(self):
        nl, no, nt, nz = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        check(self.lib.sns_get_sizes(self.h, C.byref(nl), C.byref(no), C.byref(nt), C.byref(nz)))
        return dict(n_local=nl.value, n_owned=no.value, n_tets=nt.value, nnzb=nz.value)

    def export(self, what: int, dtype, count: int) -> torch.Tensor:
        t = torch.empty(count, dtype=dtype, device=self.device)
        check(self.lib.sns_export(self.h, what, _ptr(t), t.numel() * t.element_size()))
        return t

    def bsr(self):
        """(rowptr, colind, vals[nnzb,4,4]) copies of the assembled operator."""
        s = self.sizes()
        rp = self.export(_lib.EXPORT_ROWPTR, torch.int32, s["n_local"] + 1)
        ci = self.export(_lib.EXPORT_COLIND, torch.int32, s["nnzb"])
        va = self.export(_lib.EXPORT_VALS, torch.float64, s["nnzb"] * 16)
        return rp, ci, va.view(-1, 4, 4)

    def to_scipy(self):
        import scipy.sparse as sp
        rp, ci, va = self.bsr()
        n = self.n_local
        return sp.bsr_matrix((va.cpu().numpy(), ci.cpu().numpy(), rp.cpu().numpy()), shape=(4 * n, 4 * n)).tocsr()

    def element_matrices(self) -> torch.Tensor:
        """Ke [n_tets, a, b, c, d] of the last jacobian() call (element-kernel output)."""
        s = self.sizes()
        return self.export(_lib.EXPORT_KE, torch.float64, s["n_tets"] * 256).view(-1, 4, 4, 4, 4)

    def time_kernels(self, on=True):
        check(self.lib.sns_time_kernels(self.h, 1 if on else 0))

    def kernel_times(self):
        """{mode: (total_ms, calls)} of the level-0 k_spmv family since reset_timings()."""
        ms = (C.c_double * 8)()
        calls = (C.c_int64 * 8)()
        check(self.lib.sns_get_kernel_times(self.h, ms, calls))
        names = ("ax", "b_minus_ax", "jacobi", "ax_dot", "post_m")
        return {names[i]: (ms[i], calls[i]) for i in range(5)}

    def timings(self) -> SnsTimings:
        t = SnsTimings()
        check(self.lib.sns_get_timings(self.h, C.byref(t)))
        return t

    def counters(self):
        """Debug counters of the last Krylov solve: host syncs, all-reduces, halo exchanges (+ ksp its since reset)."""
        c = (C.c_int64 * 8)()
        check(self.lib.sns_get_counters(self.h, c))
        return dict(host_syncs=c[0], allreduces=c[1], exchanges=c[2], ksp_its=c[3], damping_retries=c[4],
                    damping_factor=c[5] * 1e-6, first_attempt_reason=c[6], ap_blocks=c[7])

    def comm_info(self):
        """Transport / rank / ranks of the handle's communicator; ``rccl_ranks`` is what ncclCommCount reports."""
        c = (C.c_int32 * 4)()
        check(self.lib.sns_comm_info(self.h, c))
        return dict(transport={0: "none", 1: "rccl", 2: "team", 3: "peer"}[c[0]], rank=c[1], nranks=c[2], rccl_ranks=c[3])

    def hierarchy(self):
        """The AMG hierarchy as built: one dict per level (rows, 4x4 blocks, sweeps per half cycle, block-Jacobi damping)."""
        nl = C.c_int32()
        rows, blocks, nu, om = (C.c_int64 * 16)(), (C.c_int64 * 16)(), (C.c_int32 * 16)(), (C.c_double * 16)()
        check(self.lib.sns_get_hierarchy(self.h, C.byref(nl), rows, blocks, nu, om))
        return [dict(rows=rows[l], blocks=blocks[l], sweeps=nu[l], omega=om[l]) for l in range(nl.value)]

    def cycle(self):
        """The V-cycle as run: per level dict(kind, pre, post) -- kind 0 nodal-block Jacobi, 1 aggregate-block Jacobi, 2 / 3 dense
        direct solve (one-workgroup / blocked Gauss-Jordan), 4 sweeps only (sns_get_cycle)."""
        nl = C.c_int32()
        kind, pre, post = (C.c_int32 * 16)(), (C.c_int32 * 16)(), (C.c_int32 * 16)()
        check(self.lib.sns_get_cycle(self.h, C.byref(nl), kind, pre, post))
        return [dict(kind=kind[l], pre=pre[l], post=post[l]) for l in range(nl.value)]

    def reset_timings(self):
        check(self.lib.sns_reset_timings(self.h))

    def bench_spmv(self, reps=20) -> float:
        x = torch.randn(self.ndof, dtype=torch.float64, device=self.device)
        y = self.zeros()
        ms = C.c_double()
        check(self.lib.sns_bench_spmv(self.h, _ptr(x), _ptr(y), reps, C.byref(ms)))
        return ms.value

    def bench_assemble(self, w, form="ns", reps=5) -> float:
        w = self._vec(w)
        F = self.zeros()
        ms = C.c_double()
        check(self.lib.sns_bench_assemble(self.h, _FORMS[form], _ptr(w), _ptr(F), reps, C.byref(ms)))
        return ms.value


def _bench_collective(self, which: str, count: int = 5, reps: int = 200) -> float:
    """ms per collective of the attached communicator, back to back (collective call; measurement hook)."""
    ms = C.c_double()
    check(self.lib.sns_bench_collective(self.h, {"exchange": 0, "allreduce": 1, "allgather": 2}[which], int(count), int(reps),
                                        C.byref(ms)))
    return ms.value


FlowProblem.bench_collective = _bench_collective


class PeerGroup:
    """Peer-window communicator of the C-ABI (sns_peer_*): one process per GPU of one node, the collectives of the solver are
    stores into the other ranks' IPC-mapped windows -- no RCCL in the data path.  The 64-byte IPC handles are exchanged through
    ``torch.distributed`` (any backend: gloo is enough, nothing but this bootstrap and ``close`` goes through it).

        dist.init_process_group(...)
        peers = PeerGroup(device="cuda:0")                 # collective
        P = FlowProblem.distributed(mesh, bcs, group=peers)
        ...
        P.close(); peers.close()                           # collective
    """

    def __init__(self, device=None, *, group=None, window_bytes: int = 0, check_rounds: int = 50):
        import torch.distributed as dist
        self.lib = _lib.load()
        self.dist_group = group
        self.rank, self.nranks = dist.get_rank(group), dist.get_world_size(group)
        if device is None:
            device = f"cuda:{torch.cuda.current_device()}"
        self.device = torch.device(device)
        p = C.c_void_p()
        hd = C.create_string_buffer(64)
        check(self.lib.sns_peer_create(self.device.index or 0, self.rank, self.nranks, int(window_bytes), C.byref(p), hd))
        self.ptr = p
        box = [None] * self.nranks
        dist.all_gather_object(box, bytes(hd.raw), group=group)          # (implies: every window exists and is zeroed)
        check(self.lib.sns_peer_connect(self.ptr, b"".join(box)))
        dist.barrier(group=group)                                        # every rank has mapped every window
        if check_rounds > 0:
            # verified all-reduces / all-gathers between the real ranks before anything relies on the links (sns_peer_check_links);
            # every rank learns the common verdict, so a failure raises everywhere instead of stranding the healthy ranks
            rc = self.lib.sns_peer_check_links(self.ptr, int(check_rounds))
            msg = self.lib.sns_last_error().decode() if rc != 0 else ""
            box2 = [None] * self.nranks
            dist.all_gather_object(box2, (rc, msg), group=group)
            bad = [(r, m) for r, (c, m) in enumerate(box2) if c != 0]
            if bad:
                raise RuntimeError("peer-window link check failed on rank(s) " + "; ".join(f"{r}: {m}" for r, m in bad))

    def close(self):
        """Collective; call after the problems attached to this communicator are closed."""
        if self.ptr:
            import torch.distributed as dist
            torch.cuda.synchronize(self.device)
            dist.barrier(group=self.dist_group)                          # nobody stores into a window that is about to go
            self.lib.sns_peer_disconnect(self.ptr)                       # unmap the others' windows ...
            dist.barrier(group=self.dist_group)                          # ... and free the own one only when nobody has it mapped
            self.lib.sns_peer_destroy(self.ptr)
            self.ptr = None


class Team:
    """In-process test transport (sns_team_*): N ranks = N threads sharing one GPU."""

    def __init__(self, nranks: int):
        self.lib = _lib.load()
        self.n = nranks
        p = C.c_void_p()
        check(self.lib.sns_team_create(nranks, C.byref(p)))
        self.ptr = p

    def close(self):
        if self.ptr:
            self.lib.sns_team_destroy(self.ptr)
            self.ptr = None

    def run(self, fn):
        """fn(rank, team) on N concurrent threads; returns the list of results, re-raises the first error."""
        import threading
        out, err = [None] * self.n, [None] * self.n

        def work(r):
            try:
                out[r] = fn(r, self)
            except BaseException as e:        # noqa: BLE001
                err[r] = e

        th = [threading.Thread(target=work, args=(r,)) for r in range(self.n)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for e in err:
            if e is not None:
                raise e
        return out


class NonlinearPDE_SNESProblem:
    """Drop-in for the reference class of the same name (:40-75): ``F(x, F)``
    assembles the residual, ``J(x)`` the Jacobian, both on device vectors.
    (The reference's first positional ``snes`` argument has no counterpart.)"""

    def __init__(self, problem: FlowProblem, u: torch.Tensor):
        self.problem = problem
        self.u = u

    def F(self, snes, x, F):
        self.u.copy_(x)
        self.problem.residual(x, "ns", out=F)

    def J(self, snes, x, J=None, P=None):
        self.problem.jacobian(x, "ns")


def solve_stokes_problem(problem: FlowProblem, rank: int = 0):
    """``solve_stokes_problem(a, L, bcs, W)`` of the reference (:197-218): returns U."""
    if rank == 0:
        print("Starting Linear Solve", flush=True)
    U, res = problem.stokes_solve()
    if rank == 0:
        print(f"Finished Linear Solve (its {res.its}, reason {res.reason}, |r| {res.rnorm:.3e})", flush=True)
    return U


def newton_with_reynolds_continuation(problem: FlowProblem, w: torch.Tensor, max_halvings: int = 6, verbose: bool = False):
    """Newton at the problem's Reynolds number; if it fails (typically the first Jacobian at a guess far from the
    solution, at a cell Reynolds number the preconditioner cannot handle), Re is halved until a solve converges and
    then doubled back up, each stage starting from the previous solution.  NOT in the reference (which reports the
    failed reason and carries on, :297-298): opt-in robustness.  Returns (w, result of the last stage)."""
    Re = float(problem.options.reynolds)
    w_try, res = problem.newton_solve(w.clone())
    if res.reason > 0:
        w.copy_(w_try)
        return w, res
    k = 0
    cur = w.clone()
    while True:                                         # go down until a stage converges from the given guess
        k += 1
        if k > max_halvings:
            problem.set_options(reynolds=Re)
            return w, res
        problem.set_options(reynolds=Re / 2 ** k)
        w_try, r = problem.newton_solve(cur.clone())
        if verbose:
            print(f"  continuation: Re {Re / 2 ** k:g}: SNES reason {r.reason}, {r.its} its, {r.ksp_its} ksp its", flush=True)
        if r.reason > 0:
            cur = w_try
            break
    total_ksp = res.ksp_its + r.ksp_its
    while k > 0:                                        # ... and back up
        k -= 1
        problem.set_options(reynolds=Re / 2 ** k)
        w_try, r = problem.newton_solve(cur.clone())
        total_ksp += r.ksp_its
        if verbose:
            print(f"  continuation: Re {Re / 2 ** k:g}: SNES reason {r.reason}, {r.its} its, {r.ksp_its} ksp its", flush=True)
        if r.reason <= 0:
            problem.set_options(reynolds=Re)
            return w, r
        cur = w_try
    w.copy_(cur)
    r.ksp_its = total_ksp
    return w, r


def newton_with_law_continuation(problem: FlowProblem, w: torch.Tensor, steps: int = 4, max_bisections: int = 6,
                                 verbose: bool = False):
    """Newton at the problem's viscosity law (``problem.set_viscosity_law``) by continuation in the power-law index: the
    index walks from 1 (nu_e = nu0: the Newtonian stress-divergence form) to the law's n in ``steps`` equal steps in log n,
    each stage starting from the previous solution; a stage that does not converge gets the geometric midpoint between it
    and the last converged index put in front of it (at most ``max_bisections`` times in all).  lambda and nu_inf_ratio
    stay at the law's values.  NOT in the reference: opt-in robustness, modelled on ``newton_with_reynolds_continuation``.
    Returns (w, result of the last stage); on failure ``w`` is unchanged and the result is the failed stage's.  The
    problem's law is the target law afterwards either way."""
    law = getattr(problem, "viscosity_law", None)
    if law is None:
        raise ValueError("newton_with_law_continuation needs a viscosity law: call problem.set_viscosity_law first")
    lam, n, r = law
    todo = [float(np.exp(np.log(n) * k / int(steps))) for k in range(int(steps))] + [n]      # n^(k/steps): 1 ... n
    cur, n_done, res = w.clone(), None, None
    total_ksp = bisections = 0
    try:
        while todo:
            problem.set_viscosity_law(lam, todo[0], r)
            w_try, res = problem.newton_solve(cur.clone())
            total_ksp += res.ksp_its
            if verbose:
                print(f"  continuation: n {todo[0]:g}: SNES reason {res.reason}, {res.its} its, {res.ksp_its} ksp its", flush=True)
            if res.reason > 0:
                cur, n_done = w_try, todo.pop(0)
                continue
            bisections += 1
            if n_done is None or bisections > max_bisections:
                return w, res
            todo.insert(0, float(np.sqrt(n_done * todo[0])))
    finally:
        problem.set_viscosity_law(lam, n, r)
    w.copy_(cur)
    res.ksp_its = total_ksp
    return w, res


def solve_unsteady(problem: FlowProblem, w0, dt: float, n_steps: int, order: int = 2, theta_coeff: float = 4.0, callback=None,
                   dirichlet=None):
    """``n_steps`` implicit steps of size ``dt`` from the state ``w0`` (not modified): BDF1 for the first step, then BDF
    of the given order (1 or 2).  ``callback(step, t, w)`` runs after every converged step (step = 1.., t = step dt) with
    the time term of that step still set -- the place to sample forces (``functionals.reaction_force``) or write output.
    Stops at the first step that does not converge.  Returns (w, records): the final state and one dict per step with
    ``its``, ``ksp_its`` and ``reason``.  NOT in the reference.  The problem keeps the last step's time term;
    ``problem.clear_time_term()`` returns it to the steady form.

    ``dirichlet``: an optional callable t -> g (4 * n_nodes Dirichlet values, numpy or tensor) for a ramped or pulsatile
    inflow: before step n + 1 the problem's values are set to g((n + 1) dt) (``FlowProblem.set_dirichlet_values``); the
    step starts from u^n, which then violates them, and its first Newton update carries the lifting term.  The problem keeps the values of the last step.  None: the values the problem
    has, and not one call more."""
    if order not in (1, 2):
        raise ValueError("order must be 1 or 2")
    w = problem._vec(w0).clone()
    wprev = w.clone()
    records = []
    for step in range(1, int(n_steps) + 1):
        if dirichlet is not None:
            problem.set_dirichlet_values(dirichlet(step * dt))
        _, res = problem.time_step(w, wprev, dt, order=1 if step == 1 else order, theta_coeff=theta_coeff)
        records.append(dict(its=res.its, ksp_its=res.ksp_its, reason=res.reason))
        if res.reason <= 0:
            break
        if callback is not None:
            callback(step, step * dt, w)
    return w, records


def solve_scalar_transport(problem: FlowProblem, w, kappa, bcs, source=None):
    """Steady transport of one to four scalars by the velocity of the state ``w``: u.grad c - kappa_k Lap c = s_k with the
    Dirichlet data ``bcs`` = (mask, values), each (n, k), and zero diffusive flux elsewhere (``FlowProblem.scalar_solve`` with
    sigma = theta = 0).  The age of fluid is source = 1 with c = 0 at the inlet.  Returns (c (n, k), KrylovResult).  NOT in the
    reference."""
    return problem.scalar_solve(w, kappa, bcs, source=source)


def solve_coupled_flow(problem: FlowProblem, w0, kappa, scalar_bcs, *, log_viscosity_ratio=0.0, buoyancy=(0.0, 0.0, 0.0), species=0,
                       source=None, c0=None, max_outer=30, rtol=1e-8, relax=1.0):
    """Steady two-way coupling of the flow with the scalars it carries, by fixed-point iteration: per outer step
    ``problem.set_mixture`` from species ``species`` of c (viscosity nu0 exp(log_viscosity_ratio m), force m * buoyancy),
    ``newton_solve`` from the last state, ``scalar_solve`` carried by the new state (``kappa``, ``scalar_bcs``, ``source`` as
    there), c <- c + relax (c_new - c).  Starts from the state ``w0`` (not modified) and ``c0`` (n, k; default 0) and stops when
    ||c_new - c|| <= rtol ||c_new|| with a converged Newton solve, at the first solve that fails, or after ``max_outer`` steps.
    Returns (w, c, records): one dict per outer step with ``newton_its``, ``ksp_its``, ``newton_reason``, ``scalar_its``,
    ``scalar_reason`` (None where the flow solve failed) and ``change`` = ||c_new - c|| / ||c_new||; the loop converged iff the
    last record has ``converged``.  The fields stay set: the converged ones on success, the last step's on a failure
    (``problem.set_mixture(None)`` clears them).  NOT in the reference."""
    k = len(np.atleast_1d(np.asarray(kappa, dtype=np.float64)).ravel())
    if not 0 <= int(species) < k:
        raise ValueError("species: an index into kappa")
    w = problem._vec(w0).clone()
    c = torch.zeros(problem.n_local, k, dtype=torch.float64, device=problem.device) if c0 is None else problem._columns(c0, k).clone()
    records = []
    for _ in range(int(max_outer)):
        problem.set_mixture(c[:, species], log_viscosity_ratio, buoyancy)
        w, nres = problem.newton_solve(w)
        rec = dict(newton_its=nres.its, ksp_its=nres.ksp_its, newton_reason=nres.reason, scalar_its=None, scalar_reason=None,
                   change=None, converged=False)
        records.append(rec)
        if nres.reason <= 0:
            break
        cn, sres = problem.scalar_solve(w, kappa, scalar_bcs, source=source, c0=c)
        rec.update(scalar_its=sres.its, scalar_reason=sres.reason)
        if sres.reason <= 0:
            break
        change = float(torch.linalg.norm(cn - c)) / max(float(torch.linalg.norm(cn)), 1e-300)
        rec["change"] = change
        c = c + relax * (cn - c)
        if change <= rtol:
            rec["converged"] = True
            problem.set_mixture(c[:, species], log_viscosity_ratio, buoyancy)
            break
    return w, c, records


def advance_scalars(problem: FlowProblem, w, c0, dt: float, n_steps: int, order: int = 2, callback=None, *, kappa, bcs,
                    source=None, theta_coeff: float = 4.0):
    """``n_steps`` implicit steps of size ``dt`` of c_t + u.grad c - kappa_k Lap c = s_k from the nodal field ``c0`` (n, k; not
    modified), each one ``FlowProblem.scalar_solve``: BDF1 for the first step, then BDF of the given order (1 or 2), i.e.
    sigma = 1/dt with the source s + c^n/dt, resp. sigma = 3/(2 dt) with s + (2 c^n - c^(n-1)/2)/dt, and theta = theta_coeff /
    dt^2 under the root of tau.  ``w``: the carrying state, or a callable ``step -> state`` (step = 1..) for a flow that moves,
    e.g. the states ``solve_unsteady`` hands its callback.  ``callback(step, t, c)`` runs after every converged step.  Stops at
    the first step that does not converge.  Returns (c, records), one dict(its, reason) per step.  NOT in the reference."""
    if order not in (1, 2):
        raise ValueError("order must be 1 or 2")
    k = len(np.atleast_1d(np.asarray(kappa, dtype=np.float64)).ravel())
    c = problem._columns(c0, k).clone()
    cprev = c.clone()
    s = None if source is None else problem._columns(source, k)
    records = []
    for step in range(1, int(n_steps) + 1):
        o = 1 if step == 1 else order
        hist = c / dt if o == 1 else (2.0 * c - 0.5 * cprev) / dt
        cn, res = problem.scalar_solve(w(step) if callable(w) else w, kappa, bcs, sigma=(1.0 if o == 1 else 1.5) / dt,
                                       theta=theta_coeff / (dt * dt), source=hist if s is None else hist + s, c0=c)
        records.append(dict(its=res.its, reason=res.reason))
        if res.reason <= 0:
            break
        cprev, c = c, cn
        if callback is not None:
            callback(step, step * dt, c)
    return c, records


def pseudo_transient_solve(problem: FlowProblem, w0, dt0: float, growth: float = 10.0, max_steps: int = 60,
                           switch_rtol: float = 1e-2, verbose: bool = False):
    """Pseudo-transient continuation to the STEADY solution for guesses Newton does not converge from.  Each pseudo-step
    is ONE linearised BDF1 step with theta = 0 (so the fixed point is exactly the steady solution), written with the
    primitives: ``set_time_term(1/dt, 0, -w/dt)``, ``jacobian`` with the fused residual, ``krylov_solve``, update.  At the
    linearisation point u_t = 0, so the steady residual (one ``residual`` call per step) is the step's residual; dt follows its reduction (switched evolution
    relaxation: dt <- dt * |F_prev| / |F|, by at most ``growth`` per step either way).  Once |F| has dropped by
    ``switch_rtol`` (or after ``max_steps``) the time term is cleared and a plain ``newton_solve`` finishes.  NOT in the
    reference.  Returns (w, NewtonResult of the closing solve, with the pseudo-steps' Krylov iterations added and their
    count in ``result.ptc_steps``)."""
    w = problem._vec(w0).clone()
    F = problem.zeros()
    dt, f0, fprev, ksp, steps = float(dt0), None, None, 0, 0
    try:
        for _ in range(int(max_steps)):
            # u_t = 0 at the linearisation point whatever dt is, so the steady residual decides dt BEFORE the one assembly
            problem.clear_time_term()
            f = float(torch.linalg.vector_norm(problem.residual(w, "ns")[:4 * problem.n_owned]))
            if not np.isfinite(f):
                raise RuntimeError(f"pseudo_transient_solve: non-finite steady residual after {steps} pseudo-steps (dt0 too large?)")
            if f0 is None:
                f0 = f
            if verbose:
                print(f"  ptc step {steps + 1}: dt {dt:.3e}  |F_steady| {f:.6e}", flush=True)
            if f <= switch_rtol * f0:
                break
            if fprev is not None:
                dt *= min(growth, max(fprev / f, 1.0 / growth))
            fprev = f
            problem.set_time_term(1.0 / dt, 0.0, w * (-1.0 / dt))
            problem.jacobian(w, "ns", residual_out=F)
            y, kres = problem.krylov_solve(F)
            ksp += kres.its
            if kres.reason <= 0:
                break
            w -= y
            steps += 1
    finally:
        problem.clear_time_term()
    w, res = problem.newton_solve(w)
    res.ksp_its += ksp
    res.ptc_steps = steps
    return w, res


def residual_reynolds_derivative(problem: FlowProblem, w, rel_step: float = 1e-4) -> torch.Tensor:
    """dF/dRe at the state ``w``: central difference of ``problem.residual(w)`` at Re (1 +- rel_step); the problem's
    options are restored afterwards.  Zero on the Dirichlet rows (F_B = w_B - g does not depend on Re)."""
    w = problem._vec(w)
    Re = float(problem.options.reynolds)
    try:
        problem.set_options(reynolds=Re * (1.0 + rel_step))
        Fp = problem.residual(w, "ns")
        problem.set_options(reynolds=Re * (1.0 - rel_step))
        Fm = problem.residual(w, "ns")
    finally:
        problem.set_options(reynolds=Re)
    return (Fp - Fm) / (2.0 * Re * rel_step)


def reynolds_sensitivity(problem: FlowProblem, w, grad_J, dJ_dRe_explicit: float = 0.0, rel_step: float = 1e-4):
    """Total derivative dJ/dRe of a functional J(w(Re), Re) at a converged state ``w`` (F(w; Re) = 0) by ONE adjoint solve
    with the Jacobian Newton assembles anyway, instead of the two extra nonlinear solves of a finite difference:

        A = dF/dw at w  (``problem.jacobian(w)``),    A^T lam = grad_J  (``problem.adjoint_solve``),
        dJ/dRe = dJ_dRe_explicit - lam . dF/dRe       (dF/dRe: ``residual_reynolds_derivative``)

    ``grad_J``: dJ/dw as a dof vector (numpy or device), e.g. a row of ``functionals.boundary_traction_gradient``.  This is
    the total derivative because the Dirichlet values do not move with Re (dw_B = 0): the assembled operator is the Jacobian
    of F on the free dofs and the identity on the Dirichlet dofs, where dF_B/dRe = 0.  A functional that depends on
    nu = 1/Re explicitly -- the traction's 2 nu sym grad u term -- contributes ``dJ_dRe_explicit`` = dJ/dnu * (-1/Re^2) at
    fixed w; for the traction, which is linear in nu:

        G1, G0 = boundary_traction_gradient(mesh, 1.0, tag), boundary_traction_gradient(mesh, 0.0, tag)
        explicit = -((G1 - G0)[0] @ w) / Re**2        # drag component

    Returns (dJ/dRe, lam, KrylovResult of the adjoint solve).  The handle is left with the Jacobian at w assembled and the
    caller's options.  Single-GPU problems."""
    w = problem._vec(w)
    g = problem._vec(grad_J if isinstance(grad_J, torch.Tensor) else np.asarray(grad_J, dtype=np.float64).ravel())
    problem.jacobian(w, "ns")
    lam, res = problem.adjoint_solve(g)
    dF = residual_reynolds_derivative(problem, w, rel_step)
    return float(dJ_dRe_explicit) - float(torch.dot(lam, dF)), lam, res


def shape_sensitivity(problem: FlowProblem, w, grad_J, dJ_dX_explicit=None):
    """Gradient dJ/dX of a functional J(w(X), X) with respect to EVERY node coordinate at a converged state ``w``
    (F(w; X) = 0), for the price of one adjoint solve and one element pass:

        A = dF/dw at w  (``problem.jacobian(w)``),    A^T lam = grad_J  (``problem.adjoint_solve``),    lam_B := 0,
        dJ/dX = dJ_dX_explicit - lam . dF/dX          (``problem.residual_shape_gradient(w, lam)``)

    ``grad_J``: dJ/dw as a dof vector (numpy or device).  ``dJ_dX_explicit``: (n_nodes, 3), the derivative of J with respect
    to the coordinates at FIXED w (``functionals.boundary_traction_shape_gradient``, ``mesh2d.drag_lift_2d_shape_gradient``;
    None for a functional without one, such as a point value in a cell that does not move).  Assumptions:

      * ``w`` is converged; the error of the result is of the order of the residual.
      * The Dirichlet values are held AT THE NODES and do not follow the coordinates (dw_B = 0): a node of an inlet that moves
        keeps its value.  That is why ``lam`` is zeroed on the Dirichlet dofs: the rows F_B = w_B - g do not depend on X.
      * The result is the gradient with respect to every node, boundary and interior; contract it with a deformation field V
        (n_nodes, 3) for a directional derivative: ``(dJdX * V).sum()``.
      * The components on interior nodes are mesh-motion terms of the discrete problem; they vanish only in the limit h -> 0.

    The residual-based force (``functionals.reaction_force``) serves as J too: its dJ/dw needs the Dirichlet-row x
    free-column block of the UNCONSTRAINED Jacobian, which the assembled operator does not hold (it has unit rows there) and
    the raw-Jacobian pass applies matrix-free -- ``grad_J`` = a row of ``functionals.reaction_force_gradient(problem, w, tag)``,
    ``dJ_dX_explicit`` = ``-problem.residual_shape_gradient(w, phi e_c)`` with phi = ``functionals.tag_node_weights``.

    Returns (dJ/dX as a device tensor (n_nodes, 3), lam, KrylovResult of the adjoint solve).  The handle is left as
    ``reynolds_sensitivity`` leaves it: the Jacobian at w assembled, the caller's options.  Single-GPU problems."""
    w = problem._vec(w)
    g = problem._vec(grad_J if isinstance(grad_J, torch.Tensor) else np.asarray(grad_J, dtype=np.float64).ravel())
    problem.jacobian(w, "ns")
    lam, res = problem.adjoint_solve(g)
    lam[torch.from_numpy(problem.bc_mask.astype(bool)).to(lam.device)] = 0.0
    dJ = -problem.residual_shape_gradient(w, lam)
    if dJ_dX_explicit is not None:
        e = dJ_dX_explicit
        if not isinstance(e, torch.Tensor):
            e = torch.from_numpy(np.ascontiguousarray(e, dtype=np.float64))
        dJ += e.to(dJ.device).reshape(dJ.shape)
    return dJ, lam, res


def dirichlet_sensitivity(problem: FlowProblem, w, grad_J):
    """Gradient dJ/dg of a functional J(w(g)) with respect to EVERY Dirichlet value at a converged state ``w`` (F(w; g) = 0),
    for the price of one adjoint solve and one raw-Jacobian pass.  With f the free and B the constrained dofs, the residual is

        F_f(w; g) = R_raw(w)_f + J0[f,B] (g - w_B),        F_B(w; g) = w_B - g,

    so at a state that satisfies its data (w_B = g) the assembled operator is A = [[J0[f,f], 0], [0, I]] and
    dF/dg = [J0[f,B]; -I].  With A^T lam = grad_J (lam_B = grad_J[B]) and lam~ = lam zeroed on B,

        dJ/dg = -lam . dF/dg = grad_J[B] - (J0^T lam~)[B]

    on the constrained dofs, and 0 on the unconstrained ones.  ``grad_J``: dJ/dw as a dof vector (numpy or device), used as
    given on the constrained dofs too -- a row of ``functionals.reaction_force_gradient`` is not zero there.  Contract the
    result with a direction of the data, e.g. ``dJdg @ g_inlet`` for the amplitude of an inlet profile.

    Returns (dJ/dg as a device dof vector, lam, KrylovResult of the adjoint solve).  The handle is left as
    ``reynolds_sensitivity`` leaves it: the Jacobian at w assembled, the caller's options.  Single-GPU problems."""
    w = problem._vec(w)
    g = problem._vec(grad_J if isinstance(grad_J, torch.Tensor) else np.asarray(grad_J, dtype=np.float64).ravel())
    problem.jacobian(w, "ns")
    lam, res = problem.adjoint_solve(g)
    B = torch.from_numpy(problem.bc_mask.astype(bool)).to(lam.device)
    lt = lam.clone()
    lt[B] = 0.0
    y = problem.raw_jacobian_apply(w, lt, transpose=True)
    dJ = torch.zeros_like(g)
    dJ[B] = g[B] - y[B]
    return dJ, lam, res


def zz_estimate(problem: FlowProblem, w):
    """Global Zienkiewicz-Zhu estimate of the velocity gradient's error at the state ``w``: ``(eta, eta_rel, eta2)`` with
    eta = sqrt(sum_t eta_t^2), eta_rel = eta / sqrt(sum_t g_t^2 + sum_t eta_t^2) (between 0 and 1) and eta2 the per-cell device
    tensor of ``problem.error_indicator`` -- the map of where the mesh is too coarse.  Reduced in float64 with torch."""
    eta2, gn2 = problem.error_indicator(w)
    s = float(eta2.sum())
    eta = s ** 0.5
    den = (float(gn2.sum()) + s) ** 0.5
    return eta, (eta / den if den > 0.0 else 0.0), eta2


def ritz_pairs(H, m_done: int, shift: float = 0.0):
    """Eigenvalue estimates from the Hessenberg matrix of ``FlowProblem.stability_arnoldi`` (pure numpy): with (theta, y) the
    eigenpairs of H[:m_done, :m_done], |y| = 1, returns ``(lam, Y, est)``: lam = shift - 1/theta, the eigenvalues of
    J x = -lam B x (x ~ exp(lam t)), sorted by descending real part so that the least stable comes first (of a conjugate pair
    the one with positive imaginary part first); Y[:, k] the Ritz coefficient vector of lam[k]; est[k] =
    |h_{m+1,m} e_m^T y_k| / |theta_k|, the residual of the pair in the Arnoldi relation relative to its Ritz value.  A Ritz value
    theta = 0 (an infinite eigenvalue) sorts last with an infinite estimate."""
    H = np.asarray(H, dtype=np.float64)
    k = int(m_done)
    if k < 1:
        return np.zeros(0, complex), np.zeros((0, 0), complex), np.zeros(0)
    theta, Y = np.linalg.eig(H[:k, :k])
    Y = Y / np.linalg.norm(Y, axis=0)
    sub = abs(H[k, k - 1]) if H.shape[0] > k else 0.0
    zero = theta == 0.0
    safe = np.where(zero, 1.0, theta)
    lam = np.where(zero, -np.inf, shift - 1.0 / safe)
    est = np.where(zero, np.inf, sub * np.abs(Y[k - 1]) / np.abs(safe))
    order = np.lexsort((-lam.imag, -lam.real))
    return lam[order], Y[:, order], est[order]


def krylov_ritz_pairs(H, m_done: int, shift: float = 0.0):
    """``ritz_pairs`` for the H of a Krylov decomposition S V_k = V_k H[:k, :k] + v_{k+1} H[k, :k] whose last row is full -- what
    ``FlowProblem.stability_arnoldi_extend`` leaves after a thick restart: the same ``(lam, Y, est)`` in the same order, with
    est[j] = |H[k, :k] y_j| / |theta_j|.  On a Hessenberg H the estimate is the one of ``ritz_pairs`` up to rounding."""
    H = np.asarray(H, dtype=np.float64)
    k = int(m_done)
    if k < 1:
        return np.zeros(0, complex), np.zeros((0, 0), complex), np.zeros(0)
    theta, Y = np.linalg.eig(H[:k, :k])
    Y = Y / np.linalg.norm(Y, axis=0)
    coupling = np.abs(H[k, :k] @ Y) if H.shape[0] > k else np.zeros(k)
    zero = theta == 0.0
    safe = np.where(zero, 1.0, theta)
    lam = np.where(zero, -np.inf, shift - 1.0 / safe)
    est = np.where(zero, np.inf, coupling / np.abs(safe))
    order = np.lexsort((-lam.imag, -lam.real))
    return lam[order], Y[:, order], est[order]


def krylov_schur_truncate(H, m_done: int, keep: int):
    """The host half of one thick restart (Stewart's Krylov-Schur; pure numpy and scipy.linalg): with m = ``m_done`` and the
    decomposition S V_m = V_m H[:m, :m] + v_{m+1} H[m, :m], the ordered real Schur form H[:m, :m] = Z T Z^T with the ``keep``
    Ritz values of largest modulus -- the eigenvalues nearest the shift -- leading.  A conjugate pair is never split: if the
    cut falls inside one, one fewer is kept (one more if that would leave none).  Returns ``(k, Q, Hk)``:
    Q = blockdiag(Z[:, :k], 1), (m + 1) x (k + 1), for ``FlowProblem.basis_rotate``, and Hk = [T[:k, :k]; H[m, :m] Z[:, :k]],
    (k + 1) x k, the leading block of the H that ``stability_arnoldi_extend`` continues: S (V Q)_k = (V Q)_{k+1} Hk.  The whole
    last row of H enters: after the first restart it is full.  1 <= keep <= m - 1."""
    import scipy.linalg as sla
    H = np.asarray(H, dtype=np.float64)
    m, keep = int(m_done), int(keep)
    if not (2 <= m <= H.shape[1] and H.shape[0] > m):
        raise ValueError("m_done must lie in [2, m] and H must hold row m_done")
    if not 1 <= keep <= m - 1:
        raise ValueError("keep must lie in [1, m_done - 1]")
    A = H[:m, :m]
    theta = np.linalg.eigvals(A)
    theta = theta[np.argsort(-np.abs(theta), kind="stable")]
    pair_tol = 1e-12 * max(np.abs(theta[0]), np.finfo(float).tiny)

    def splits(k):                                         # theta[k - 1] and theta[k] are the two members of one pair
        return theta[k - 1].imag != 0.0 and abs(theta[k] - np.conj(theta[k - 1])) <= pair_tol

    k = keep
    if splits(k):
        k = k - 1 if k > 1 else 2
    if not 1 <= k <= m - 1:
        raise ValueError("no cut between 1 and m_done - 1 that keeps a conjugate pair together")
    cut = 0.5 * (np.abs(theta[k - 1]) + np.abs(theta[k]))
    T, Z, sdim = sla.schur(A, output="real", sort=lambda re, im: np.hypot(re, im) > cut)
    if sdim != k or (T[k, k - 1] != 0.0):
        raise np.linalg.LinAlgError(f"the ordered Schur form kept {sdim} Ritz values, not {k}: two moduli at the cut coincide")
    Q = np.zeros((m + 1, k + 1))
    Q[:m, :k] = Z[:, :k]
    Q[m, k] = 1.0
    Hk = np.vstack([T[:k, :k], H[m, :m] @ Z[:, :k]])
    return k, Q, Hk


def pair_left_right(lam_right, lam_left, shift: float = 0.0, rtol: float = 1e-5):
    """Which left Ritz value belongs to which right one (pure numpy): ``partner[k]`` = the index into ``lam_left`` of the value
    nearest ``lam_right[k]``, or -1.  A pair is accepted only if the two differ by at most ``rtol`` |lam - shift| -- both sides
    are Ritz values of shift-inverted operators, theta = 1 / (shift - lam), whose relative error is what the residual estimate
    controls, so |lam - shift| is the scale on which two estimates of one eigenvalue agree -- and a left value serves one right
    value only, the nearest; candidates are taken in ascending distance.  Whatever is left over stays -1: flagged, not guessed.
    Non-finite values never pair."""
    lr, ll = np.asarray(lam_right, dtype=complex), np.asarray(lam_left, dtype=complex)
    partner = np.full(len(lr), -1, dtype=np.int64)
    if len(lr) == 0 or len(ll) == 0:
        return partner
    with np.errstate(invalid="ignore"):
        dist = np.abs(lr[:, None] - ll[None, :])
        ok = np.isfinite(dist) & (dist <= rtol * np.abs(lr - shift)[:, None])
    taken = np.zeros(len(ll), dtype=bool)
    for flat in np.argsort(np.where(ok, dist, np.inf), axis=None, kind="stable"):
        k, j = divmod(int(flat), len(ll))
        if not ok[k, j]:
            break
        if partner[k] < 0 and not taken[j]:
            partner[k], taken[j] = j, True
    return partner


def _complex_apply(op, x):
    """op (real, linear, device vector -> device vector) on a complex device vector."""
    return torch.complex(op(x.real.contiguous()), op(x.imag.contiguous()))


def mode_pairing(problem: FlowProblem, w, z, x):
    """z^T B(w) x of a left and a right mode (complex device vectors), unconjugated: the matrices are real.  Python complex."""
    Bx = _complex_apply(lambda v: problem.mass_apply(w, v), x)
    return complex(torch.sum(z * Bx))


def default_keep(m: int, n_modes: int) -> int:
    """How many Ritz directions a thick restart of ``linear_stability`` keeps by default: min(m - 2, max(n_modes + 2, m // 2))."""
    return min(int(m) - 2, max(int(n_modes) + 2, int(m) // 2))


def _restarted_arnoldi(problem, w, shift, m, n_modes, tol, max_restarts, keep, side, breakdown_rel, pc_shift=None):
    """One side of ``linear_stability`` (``max_restarts = 0``: the first call alone): ``stability_arnoldi``, then estimates,
    truncate, ``basis_rotate``, ``stability_arnoldi_extend`` until the ``n_modes`` Ritz pairs of largest |theta| (nearest the
    shift) all have an estimate <= tol, ``max_restarts`` is reached, the space is invariant (reason 2) or an inner solve failed
    (reason < 0).  Returns (V, H, ArnoldiResult with the Krylov iterations of all cycles, restarts).  ``pc_shift`` given (a
    complex ``shift``): the same loop over ``stability_arnoldi_shifted``, with the true residuals of ``shifted_eigenpairs`` as
    the estimates."""
    shifted = pc_shift is not None
    if shifted:
        V, H, res = problem.stability_arnoldi_shifted(w, shift, pc_shift, m=m, side=side, breakdown_rel=breakdown_rel)
    else:
        V, H, res = problem.stability_arnoldi(w, shift=shift, m=m, side=side, breakdown_rel=breakdown_rel)
    its, restarts = res.ksp_its, 0
    while res.reason == 1 and restarts < max_restarts:
        if shifted:
            lam, _, est, theta = shifted_eigenpairs(problem, w, V, H, res.m_done, shift, pc_shift, side)
            lead = np.argsort(-np.abs(theta), kind="stable")[:max(0, int(n_modes))]
        else:
            lam, _, est = krylov_ritz_pairs(H, res.m_done, shift)
            with np.errstate(invalid="ignore"):
                lead = np.argsort(np.abs(lam - shift), kind="stable")[:max(0, int(n_modes))]
        if (est[lead] <= tol).all():
            break
        k, Q, Hk = krylov_schur_truncate(H, res.m_done, keep)
        problem.basis_rotate(V, Q)
        H[:] = 0.0
        H[:k + 1, :k] = Hk
        if shifted:
            _, _, res = problem.stability_arnoldi_shifted(w, shift, pc_shift, side=side, breakdown_rel=breakdown_rel, V=V, H=H, k=k)
        else:
            res = problem.stability_arnoldi_extend(w, V, H, k, shift=shift, side=side, breakdown_rel=breakdown_rel)
        its += res.ksp_its
        restarts += 1
    return V, H, ArnoldiResult(res.m_done, res.reason, its), restarts


def shifted_roots(theta, shift):
    """The two eigenvalue candidates behind a Ritz value ``theta`` of S = Re[(J + s B)^-1 B], s = a + i b (pure numpy): an
    eigenvalue lam of J x = -lam B x has theta = (a - lam) / ((s - lam)(conj(s) - lam)), i.e.
    theta lam^2 + (1 - 2 a theta) lam + (theta |s|^2 - a) = 0, whose roots are a - r and a - b^2 / r with
    r = (1 + sqrt(1 - 4 b^2 theta^2)) / (2 theta) (the product of the two r is b^2: no cancellation for small b theta).  With
    b = 0 the first is the real-shift formula a - 1 / theta and the second is the shift itself.  Returns (lam1, lam2)."""
    s = complex(shift)
    a, b2 = s.real, s.imag * s.imag
    theta = np.asarray(theta, dtype=complex)
    r = (1.0 + np.sqrt(1.0 - 4.0 * b2 * theta * theta)) / (2.0 * theta)
    return a - r, a - b2 / r


def shifted_eigenpairs(problem: FlowProblem, w, V, H, m_done: int, shift, pc_shift: float, side: str = "right"):
    """Eigenvalue estimates from the V and H of ``FlowProblem.stability_arnoldi_shifted`` (Hessenberg or, after a thick restart,
    with a full last row).  Per Ritz pair (theta, y) of H[:m_done, :m_done], |y| = 1: x = V y, the two candidates of
    ``shifted_roots``, and of them the one with the smaller TRUE residual |J x + lam B x| / (|lam| |B x|) -- one
    ``shifted_apply`` at c = lam - pc_shift per candidate and two mass passes, so the problem must hold J + pc_shift B, as it
    does after the Arnoldi call; ``side="left"``: the operator flipped for the duration and B^T.  That residual is the
    estimate: it is what says whether a pair converged.  Of a conjugate pair of Ritz values only the member with Im theta > 0 is
    evaluated; its partner gets the conjugates.  Returns ``(lam, Y, est, theta)`` in the order of ``ritz_pairs`` (descending
    real part, the least stable first); theta = 0 (an infinite eigenvalue) sorts last with an infinite estimate."""
    if side not in ("right", "left"):
        raise ValueError("side must be 'right' or 'left'")
    H = np.asarray(H, dtype=np.float64)
    k = int(m_done)
    if k < 1:
        return np.zeros(0, complex), np.zeros((0, 0), complex), np.zeros(0), np.zeros(0, complex)
    s, p, left = complex(shift), float(pc_shift), side == "left"
    theta, Y = np.linalg.eig(H[:k, :k])
    theta, Y = theta.astype(complex), Y.astype(complex)
    Y = Y / np.linalg.norm(Y, axis=0)
    lam, est = np.full(k, -np.inf + 0j), np.full(k, np.inf)
    mass = problem.mass_apply_transpose if left else problem.mass_apply
    Vk = V[:k].T
    if left:
        problem.transpose_operator()
    try:
        j = 0
        while j < k:
            pair = theta[j].imag > 0.0 and j + 1 < k and theta[j + 1] == np.conj(theta[j])
            if theta[j] != 0.0:
                y = Y[:, j]
                x = torch.complex(Vk @ torch.from_numpy(y.real.copy()).to(V.device), Vk @ torch.from_numpy(y.imag.copy()).to(V.device))
                nb = float(torch.linalg.vector_norm(_complex_apply(lambda v: mass(w, v), x)))
                for cand in shifted_roots(theta[j], s):
                    cand = complex(cand)
                    if not np.isfinite(cand) or cand == 0.0 or not nb > 0.0:
                        continue
                    r = float(torch.linalg.vector_norm(problem.shifted_apply(w, cand - p, x, transpose=left))) / (abs(cand) * nb)
                    if r < est[j]:
                        lam[j], est[j] = cand, r
            if pair:
                lam[j + 1], est[j + 1], Y[:, j + 1] = np.conj(lam[j]), est[j], np.conj(Y[:, j])
            j += 2 if pair else 1
    finally:
        if left:
            problem.transpose_operator()
    order = np.lexsort((-lam.imag, -lam.real))
    return lam[order], Y[:, order], est[order], theta[order]


def linear_stability(problem: FlowProblem, w, n_modes: int = 6, shift: float = 0.0, m: int = 64, tol: float = 1e-7,
                     ksp_rtol: float = 1e-10, left: bool = False, pair_rtol: float = 1e-5, max_restarts: int = 0,
                     keep: Optional[int] = None, breakdown_rel: float = 1e-6, pc_shift: Optional[float] = None) -> StabilityResult:
    """Leading eigenvalues and modes of the linearised transient operator B x_t + J x = 0 at the steady state ``w``: is the
    state stable (every Re lam < 0), and if not, at which frequency Im lam / 2 pi does it go?  ``m`` steps of shift-invert
    Arnoldi (``FlowProblem.stability_arnoldi``) with the inner tolerance ``ksp_rtol`` (the problem's options are restored
    afterwards), ``ritz_pairs`` on the host, ``n_modes`` modes formed as V y on the device: the least stable of the pairs whose residual
    estimate is at most ``tol`` (``converged``), least stable first, and behind them, if fewer converged, the others by
    ascending estimate.  Eigenvalues nearest the shift converge first: shift = 0 finds
    those of smallest modulus, which are the least stable ones of a flow near its first instability.

    ``left=True`` runs the left process too (``stability_arnoldi(side="left")``, as many steps, the same tolerance) and pairs
    every selected right pair that converged with the converged left Ritz pair of nearest eigenvalue (``pair_left_right`` with
    ``pair_rtol``): ``left_converged`` says which entries have a partner, ``left_modes`` holds z = V_L y_L scaled so that
    z^T B x = 1 with the right mode as returned (unconjugated; z^T J = -lam z^T B), zero where there is none, and
    ``left_eigenvalues`` the partner's own Ritz value.  The other fields are what they are without it.

    ``max_restarts > 0`` turns the process into a thick-restarted one (Stewart's Krylov-Schur), so that ``m`` can be small --
    the basis is (m + 1) ndof doubles per side, 13 or 17 vectors instead of 65 -- and a mode that m steps do not reach is
    iterated on instead of reported unconverged: after the first ``m`` steps, while the ``n_modes`` Ritz pairs nearest the shift
    are not all within ``tol`` and fewer than ``max_restarts`` restarts were taken, the ``keep`` Ritz directions nearest the
    shift are kept (``krylov_schur_truncate``; one fewer where the cut would split a conjugate pair), the basis is compressed
    onto them in place (``FlowProblem.basis_rotate``) and the same process goes on from column ``keep``
    (``FlowProblem.stability_arnoldi_extend``): m - keep solves per restart.  A breakdown (reason 2: the space is invariant)
    and a failed inner solve (reason < 0) end the side as they end the unrestarted process.  The left side runs the same loop.
    Selection, normalisation, phase, pairing and the scaling z^T B x = 1 are then those above, on the final H and V with the
    estimates of ``krylov_ritz_pairs``; ``restarts`` / ``left_restarts`` say how many were taken, ``ksp_its`` counts all cycles.
    ``keep`` defaults to min(m - 2, max(n_modes + 2, m // 2)): it must leave head-room above ``n_modes`` -- on the test ducts
    (m, keep, n_modes) = (10, 4, 3) stagnated for 30 restarts where (12, 6, 4) converged in 8 -- and below m.  With
    ``max_restarts = 0`` the function is the unrestarted one, bit for bit.  What a restarted run looks for is the ``n_modes``
    eigenvalues NEAREST THE SHIFT and nothing else: a less stable eigenvalue farther away, which 64 unrestarted steps may reach
    in passing (on the (6,3,3) test duct -5.35 +- 6.07i, |lam| = 8.1, behind four nearer ones), is not kept; move the shift or
    raise ``n_modes`` and ``keep`` if the least stable mode need not be the one nearest the shift.  ``breakdown_rel`` (restarted runs only) is handed to
    every cycle: on a space that is invariant after a few steps it has to sit above what the inner tolerance leaves of the
    step's norm.

    A ``complex`` shift s = a + i b (and only that type: a ``float`` goes where it always went, bit for bit) runs shift-invert in
    real Arnoldi arithmetic on Re[(J + s B)^-1 B] (``FlowProblem.stability_arnoldi_shifted``; Parlett & Saad): the eigenvalues
    nearest s AND nearest conj(s), so a Hopf pair far from the real axis is reached directly, and a < 0 is allowed
    (``complex(a, 0)`` is a negative real shift).  The basis stays real, so restarts, ``left=True``, pairing and scaling are the
    ones above; eigenvalues and estimates come from ``shifted_eigenpairs``: ``estimates`` then holds TRUE residuals
    |J x + lam B x| / (|lam| |B x|), and ``tol`` is compared with those.  ``pc_shift`` >= 0 (default |s|): the real shift of the
    matrix J + pc_shift B that is assembled and preconditioned; the inner solver is a complex FGMRES whatever ksp_type says.
    Not built: explicit locking / deflation of converged pairs, selections other than "nearest the shift" (rightmost Re lam
    wanders), a complex Arnoldi basis."""
    max_restarts = int(max_restarts)
    cx = isinstance(shift, (complex, np.complexfloating))
    if cx:
        shift = complex(shift)
        pc_shift = abs(shift) if pc_shift is None else float(pc_shift)
    elif pc_shift is not None:
        raise ValueError("pc_shift belongs to a complex shift")
    if max_restarts > 0:
        keep = default_keep(m, n_modes) if keep is None else int(keep)
        if not 1 <= keep <= int(m) - 1:
            raise ValueError("keep must lie in [1, m - 1]")
    old = problem.options.ksp_rtol
    problem.set_options(ksp_rtol=float(ksp_rtol))
    restarts = restartsL = 0
    try:
        # (without restarts the loop of _restarted_arnoldi does not run, and breakdown_rel is the methods' default)
        cycle = dict(shift=shift, m=m, n_modes=n_modes, tol=tol, max_restarts=max_restarts, keep=keep, pc_shift=pc_shift,
                     breakdown_rel=breakdown_rel if max_restarts > 0 else 1e-6)
        V, H, res, restarts = _restarted_arnoldi(problem, w, side="right", **cycle)
        if left:
            VL, HL, resL, restartsL = _restarted_arnoldi(problem, w, side="left", **cycle)
    finally:
        problem.set_options(ksp_rtol=old)
    if cx:
        def pairs_of(Hs, k, _, Vs=None, side="right"):
            return shifted_eigenpairs(problem, w, V if Vs is None else Vs, Hs, k, shift, pc_shift, side)[:3]
    else:
        pairs_of = krylov_ritz_pairs if max_restarts > 0 else ritz_pairs
    lam, Y, est = pairs_of(H, res.m_done, shift)
    # the converged pairs in ritz_pairs' order, then the others by their estimate: an unconverged Ritz value near theta = 0 (the
    # infinite eigenvalues of the pencil; B has no pressure columns) has an arbitrary, often huge positive, real part
    ok = est <= tol
    pick = np.concatenate([np.nonzero(ok)[0], np.nonzero(~ok)[0][np.argsort(est[~ok], kind="stable")]])[:max(0, int(n_modes))]
    lam, Y, est = lam[pick], Y[:, pick], est[pick]
    n = len(pick)
    k = res.m_done
    if n:
        Vk = V[:k].T
        Yr = torch.from_numpy(np.ascontiguousarray(Y.real)).to(V.device)
        Yi = torch.from_numpy(np.ascontiguousarray(Y.imag)).to(V.device)
        modes = torch.complex(Vk @ Yr, Vk @ Yi).T.contiguous()
        modes = modes / torch.linalg.vector_norm(modes, dim=1, keepdim=True)
        big = modes.gather(1, modes.abs().argmax(dim=1, keepdim=True))
        modes = modes * (big.conj() / big.abs())
    else:
        modes = torch.zeros(0, problem.ndof, dtype=torch.complex128, device=V.device)
    result = StabilityResult(lam, modes, est, est <= tol, res.m_done, res.ksp_its, res.reason, shift if cx else float(shift))
    result.restarts = restarts
    if not left:
        return result
    lamL, YL, estL = pairs_of(HL, resL.m_done, shift, VL, "left") if cx else pairs_of(HL, resL.m_done, shift)
    okL = np.nonzero(estL <= tol)[0]
    partner = pair_left_right(np.where(result.converged, lam, np.nan), lamL[okL], shift, pair_rtol)
    zs = torch.zeros_like(modes)
    lam_left = np.full(n, np.nan + 0j)
    VLk = VL[:resL.m_done].T
    for k in np.nonzero(partner >= 0)[0]:
        j = okL[partner[k]]
        y = np.ascontiguousarray(YL[:, j])
        z = torch.complex(VLk @ torch.from_numpy(y.real.copy()).to(V.device), VLk @ torch.from_numpy(y.imag.copy()).to(V.device))
        zs[k] = z / mode_pairing(problem, w, z, modes[k])
        lam_left[k] = lamL[j]
    result.left_modes, result.left_converged, result.left_eigenvalues = zs, partner >= 0, lam_left
    result.left_m_done, result.left_ksp_its, result.left_reason = resL.m_done, resL.ksp_its, resL.reason
    result.left_restarts = restartsL
    return result


def harmonic_response(problem: FlowProblem, w, omega: float, f):
    """The frequency response of the flow linearised at the steady state ``w`` to a harmonic body force f exp(i omega t):
    q = (J + i omega B)^-1 B f, so that q exp(i omega t) solves B x_t + J x = B f exp(i omega t).  ``f``: a real or complex dof
    vector (pressure and constrained entries are ignored, as ``mass_apply`` ignores them).  The Jacobian is assembled at ``w``,
    its hierarchy preconditions the complex solve (``FlowProblem.shifted_solve`` at c = i omega, with the problem's ksp
    options).  Returns (q complex128 device tensor, KrylovResult); |q| against omega is the gain curve, whose peak sits at the
    frequency of the least damped mode."""
    problem.jacobian(w)
    f = f if isinstance(f, torch.Tensor) else torch.as_tensor(np.asarray(f))
    f = f.to(problem.device)
    if f.is_complex():
        b = _complex_apply(lambda v: problem.mass_apply(w, v), f)
    else:
        b = problem.mass_apply(w, f)
    return problem.shifted_solve(w, 1j * float(omega), b)


@dataclass
class ResolventResult:
    omega: float
    gains: np.ndarray           # (n,) sigma_k, descending: |q|_Q = sigma |f|_ML for the optimal pairs
    forcing_modes: torch.Tensor  # (n, ndof) complex128 on the device: f_k = S V s_k, of unit lumped-volume norm where the forcing weight is 1
    response_modes: torch.Tensor  # (n, ndof) complex128: q_k = R f_k / sigma_k by one forward solve each, of unit energy norm
    residuals: np.ndarray       # (n,) the estimates |h_{m+1,m}| |last component of s_k|, on the scale of sigma^2
    converged: np.ndarray       # (n,) bool: estimate <= tol * sigma_1^2
    m_done: int
    ksp_its: int                # the process's inner solves and the forward solves of the response modes
    reason: int                 # of the process: 1 all m steps, 2 breakdown, < 0 the KSP reason of a failed inner solve


def resolvent_ritz(H, m_done: int):
    """The Ritz pairs of the Hermitian Krylov process of ``FlowProblem.resolvent_lanczos`` (numpy only): the eigenpairs of the
    Hermitian part of H[:m_done, :m_done] in descending order of the eigenvalue -- the squared gains -- and per pair the
    residual estimate |h_{m_done+1, m_done}| |last component of the eigenvector|.  Returns (theta (k,), S (k, k) with unit
    columns, estimates (k,)); m_done = 0: three empty arrays."""
    k = int(m_done)
    H = np.asarray(H)
    if k <= 0:
        return np.zeros(0), np.zeros((0, 0), dtype=np.complex128), np.zeros(0)
    Hk = H[:k, :k]
    theta, Y = np.linalg.eigh(0.5 * (Hk + Hk.conj().T))
    order = np.argsort(-theta, kind="stable")
    theta, Y = theta[order], Y[:, order]
    beta = abs(H[k, k - 1]) if H.shape[0] > k else 0.0
    return theta, Y, beta * np.abs(Y[k - 1, :])


def resolvent_analysis(problem: FlowProblem, w, omega: float, n_modes: int = 3, m: int = 24, tol: float = 1e-6, forcing_weight=None,
                       response_weight=None, ksp_rtol: float = 1e-10) -> ResolventResult:
    """The leading resolvent gains of the flow linearised at the steady state ``w`` at the frequency ``omega``, with the optimal
    forcings and their responses: the largest singular values sigma_k of R = (J + i omega B)^-1 B with the response measured in
    kinetic energy (``FlowProblem.energy_apply`` with ``response_weight``) and the forcing in the lumped volume norm
    (``forcing_weight`` restricts it to where the weight is not 0).  ``m`` steps of ``FlowProblem.resolvent_lanczos`` with the
    inner tolerance ``ksp_rtol`` (the problem's options are restored afterwards), ``resolvent_ritz`` on the host, the ``n_modes``
    leading pairs: f_k = S V s_k, and q_k = R f_k / sigma_k by one forward solve each (``harmonic_response``'s), scaled to unit
    energy norm.  A pair whose estimate exceeds ``tol`` sigma_1^2 is returned and flagged in ``converged``, never dropped.  For
    a stable flow sigma_1 over omega is the gain curve (``resolvent_gain_curve``); its peak says which frequency the flow
    amplifies most, f_1 where to force it and q_1 what answers."""
    w = problem._vec(w)
    old = problem.options.ksp_rtol
    problem.set_options(ksp_rtol=float(ksp_rtol))
    try:
        V, H, res = problem.resolvent_lanczos(w, omega, m=m, forcing_weight=forcing_weight, response_weight=response_weight)
        theta, Y, est = resolvent_ritz(H, res.m_done)
        n = min(max(0, int(n_modes)), len(theta))
        theta, Y, est = theta[:n], Y[:, :n], est[:n]
        gains = np.sqrt(np.maximum(theta, 0.0))
        ml = problem.lumped_volumes()
        chi = problem._nodal_weight(forcing_weight, "forcing_weight")
        scale = torch.where(ml > 0.0, 1.0 / torch.sqrt(torch.where(ml > 0.0, ml, torch.ones_like(ml))), torch.zeros_like(ml))
        scale[torch.from_numpy(problem.bc_mask.astype(bool)).to(problem.device)] = 0.0
        if chi is not None:
            scale = scale * chi.repeat_interleave(4)
        Yd = torch.from_numpy(np.ascontiguousarray(Y.T)).to(problem.device)          # (n, m_done)
        F = (Yd @ V[:res.m_done]) * scale if n else torch.zeros(0, problem.ndof, dtype=torch.complex128, device=problem.device)
        Q = torch.zeros_like(F)
        its = res.ksp_its
        for k in range(n):
            q, kres = harmonic_response(problem, w, omega, F[k])
            its += kres.its
            qn = float(torch.sqrt(torch.vdot(q, problem.energy_apply(q, response_weight)).real))
            Q[k] = q / qn if qn > 0.0 else q
    finally:
        problem.set_options(ksp_rtol=old)
    conv = est <= tol * (theta[0] if n else 0.0)
    return ResolventResult(float(omega), gains, F, Q, est, conv, res.m_done, its, res.reason)


def resolvent_gain_curve(problem: FlowProblem, w, omegas, **kw) -> np.ndarray:
    """The leading resolvent gain sigma_1 at every frequency of ``omegas`` (``resolvent_analysis`` with n_modes = 1 unless
    ``kw`` says otherwise; nan where the process produced no pair)."""
    kw.setdefault("n_modes", 1)
    out = np.full(len(omegas), np.nan)
    for i, om in enumerate(omegas):
        r = resolvent_analysis(problem, w, float(om), **kw)
        if len(r.gains):
            out[i] = r.gains[0]
    return out


def print_resolvent(result: ResolventResult, rank: int = 0):
    if rank != 0:
        return
    for k in range(len(result.gains)):
        flag = "" if result.converged[k] else "  (not converged)"
        print(f"Resolvent gain: omega {result.omega:.6g} sigma {result.gains[k]:.8e} residual estimate {result.residuals[k]:.2e}{flag}",
              flush=True)


def _mode_pair(result: StabilityResult, k: int):
    if result.left_modes is None:
        raise ValueError("the result has no left modes: run linear_stability(..., left=True)")
    if not result.left_converged[k]:
        raise ValueError(f"mode {k} has no converged left partner")
    return complex(result.eigenvalues[k]), result.modes[k], result.left_modes[k]


def structural_sensitivity(problem: FlowProblem, w, result: StabilityResult, k: int = 0) -> torch.Tensor:
    """The wavemaker map of mode ``k`` of a ``linear_stability(..., left=True)`` result: per node
    |z_u(node)| |x_u(node)| / |z^T B x| over the three velocity components, a device tensor of n_nodes.  It bounds the drift of
    the eigenvalue under a local feedback dJ = C delta(node) (|d lam| <= |C| times the map): where it is large the
    instability lives.  Invariant under a rescaling of x or z."""
    _, x, z = _mode_pair(result, k)
    zu = torch.linalg.vector_norm(z.view(-1, 4)[:, :3], dim=1)
    xu = torch.linalg.vector_norm(x.view(-1, 4)[:, :3], dim=1)
    return zu * xu / abs(mode_pairing(problem, w, z, x))


def eigenvalue_drift(problem: FlowProblem, w, result: StabilityResult, k: int, dJx, dBx=None) -> complex:
    """First-order change of eigenvalue ``k`` under a perturbation (dJ, dB) of the pencil J x = -lam B x:
    d lam = -z^T (dJ x + lam dB x) / (z^T B x), from the caller's ``dJx`` = dJ . x (and ``dBx`` = dB . x, if B changes too):
    complex device vectors, x = ``result.modes[k]``."""
    lam, x, z = _mode_pair(result, k)
    t = dJx if dBx is None else dJx + lam * dBx
    return -complex(torch.sum(z * t)) / mode_pairing(problem, w, z, x)


def eigenvalue_reynolds_sensitivity(problem: FlowProblem, w, result: StabilityResult, k: int = 0, rel_step: float = 1e-3,
                                    newton_tol: float = 1e-11):
    """``(dlam_dRe, Re_c)``: the total derivative of eigenvalue ``k`` with respect to the Reynolds number, the change of the
    base flow included, and the linear estimate Re_c = Re - real(lam) / real(dlam/dRe) of where the mode crosses the imaginary
    axis (nan if the real part does not move).

    Two Newton solves from ``w`` at Re (1 +- rel_step) give the steady states there; at each, ``jacobian`` + ``spmv`` and
    ``mass_apply`` on the real and imaginary part of x give J x and B x; their central differences are dJ x and dB x of
    ``eigenvalue_drift``.  No eigenproblem is solved again.  The error is O(rel_step^2): the second-order term of the
    perturbation series (3e-8 relative at 1e-3, 3e-6 at 1e-2 for the leading mode of the (6, 3, 3) test duct against the
    difference of dense spectra), plus the error of the two states over rel_step -- which is why the two Newton solves run
    with snes_rtol = snes_stol = ``newton_tol`` and snes_atol = newton_tol / 100 (restored afterwards) and why ``w`` should be
    converged as well.  Afterwards the problem has its Reynolds number and options back and holds the steady Jacobian at
    ``w``, untransposed."""
    lam, x, z = _mode_pair(result, k)
    w = problem._vec(w)
    Re = float(problem.options.reynolds)
    old = {name: getattr(problem.options, name) for name in ("snes_rtol", "snes_atol", "snes_stol")}
    Jx, Bx = [], []
    try:
        problem.set_options(snes_rtol=float(newton_tol), snes_stol=float(newton_tol), snes_atol=0.01 * float(newton_tol))
        for sign in (1.0, -1.0):
            problem.set_options(reynolds=Re * (1.0 + sign * rel_step))
            ws, nres = problem.newton_solve(w.clone())
            if nres.reason <= 0:
                raise RuntimeError(f"eigenvalue_reynolds_sensitivity: Newton at Re {Re * (1.0 + sign * rel_step):g} ended with reason {nres.reason}")
            problem.jacobian(ws, "ns")
            Jx.append(_complex_apply(problem.spmv, x))
            Bx.append(_complex_apply(lambda v: problem.mass_apply(ws, v), x))
    finally:
        problem.set_options(reynolds=Re, **old)
        problem.jacobian(w, "ns")
    h = 2.0 * rel_step * Re
    dlam = eigenvalue_drift(problem, w, result, k, (Jx[0] - Jx[1]) / h, (Bx[0] - Bx[1]) / h)
    Re_c = Re - lam.real / dlam.real if dlam.real != 0.0 else float("nan")
    return dlam, Re_c


def _sensitivity_pair(problem: FlowProblem, result, k: int, pair):
    """(lam, x, z) of mode ``k`` of ``result``, or of ``pair`` = (lam, x, z) given directly: complex device vectors."""
    if pair is None:
        return _mode_pair(result, k)
    lam, x, z = pair

    def dev(v):
        v = torch.as_tensor(v).to(device=problem.device, dtype=torch.complex128).contiguous()
        if v.numel() != problem.ndof:
            raise ValueError(f"expected a mode of {problem.ndof} entries")
        return v
    return complex(lam), dev(x), dev(z)


def _bilinear_complex(op, z, x):
    """op(z, x) -- real, bilinear, on real device vectors -- extended to complex z and x: four passes."""
    zr, zi, xr, xi = z.real.contiguous(), z.imag.contiguous(), x.real.contiguous(), x.imag.contiguous()
    return torch.complex(op(zr, xr) - op(zi, xi), op(zr, xi) + op(zi, xr))


def eigenvalue_base_flow_sensitivity(problem: FlowProblem, w, result: StabilityResult = None, k: int = 0, pair=None) -> torch.Tensor:
    """The sensitivity of eigenvalue ``k`` of a ``linear_stability(..., left=True)`` result to the base flow, a complex device
    vector over the dofs:

        grad_w lam = -s / (z^T B x),    s = H_J(z, x) + lam H_B(z, x),    H_A(z, x) = grad_w [ z~^T A(w) x~ ]

    so that the first-order drift under a change dw of the base flow (whatever causes it) is d lam = grad_w lam . dw,
    unconjugated.  J and B are real: with z = z_r + i z_i, x = x_r + i x_i, lam = a + i b this is
    ``jacobian_state_gradient`` on four real pairs, each with (c_jac, c_mass) = (1, a) and (0, b) -- eight passes.  Entries of
    constrained dofs are 0.  ``pair=(lam, x, z)`` supplies a mode directly instead of ``result`` / ``k``.  Nothing of the
    problem is changed."""
    lam, x, z = _sensitivity_pair(problem, result, k, pair)
    w = problem._vec(w)
    a, b = lam.real, lam.imag
    s1 = _bilinear_complex(lambda zz, xx: problem.jacobian_state_gradient(w, xx, zz, 1.0, a), z, x)
    sb = _bilinear_complex(lambda zz, xx: problem.jacobian_state_gradient(w, xx, zz, 0.0, b), z, x)
    s = s1 + 1j * sb                                         # H_J + a H_B + i b H_B
    return -s / mode_pairing(problem, w, z, x)


def lumped_volumes(mesh) -> np.ndarray:
    """Per node a quarter of the incident tets' volumes (host, from the mesh)."""
    X = np.asarray(mesh.points, dtype=np.float64)[np.asarray(mesh.tets)]
    vol = np.abs(np.linalg.det(np.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 3] - X[:, 0]], axis=2))) / 6.0
    out = np.zeros(len(mesh.points))
    np.add.at(out, np.asarray(mesh.tets).reshape(-1), np.repeat(0.25 * vol, 4))
    return out


def eigenvalue_forcing_sensitivity(problem: FlowProblem, w, result: StabilityResult = None, k: int = 0, pair=None,
                                   fd_rel: float = 1e-5, density: bool = False, ksp_rtol: float = 1e-10) -> torch.Tensor:
    """The sensitivity of eigenvalue ``k`` to a steady body force (passive control: where to push the flow, or where to put
    a small body, to move the eigenvalue), a complex device vector of 4 n entries with the pressure slots 0:

        grad_f lam = B^T J^-T grad_w lam  +  E / (z^T B x),        E = D_w[ B(w)^T z ][x],

    so that d lam = grad_f lam . df to first order for a nodal force df as ``set_body_force`` takes it, the re-converged base
    flow included.  dR/df = -B(w) gives dw = J^-1 B df and the first term (``eigenvalue_base_flow_sensitivity``); the Jacobian
    also depends on f explicitly, dJ/df[df] = -D_w[B(w) df] -- the stabilisation's own dependence on u in the weighting of f,
    with no counterpart in the continuous theory -- which is the second term.  It is not small on coarse meshes.

    This holds for forces that vanish on velocity-constrained dofs: the mass passes read those entries as 0, the result is 0
    there, and the sensitivity to forcing on Dirichlet nodes is not computed.

    J^-T is two ``adjoint_solve`` calls (real and imaginary part) on J(w), which is assembled here, with the inner tolerance
    ``ksp_rtol`` (the problem's own is restored afterwards); B^T is ``mass_apply_transpose``.  E is the one approximation in
    the function: the central difference of ``mass_apply_transpose`` along x~ with the step ``fd_rel`` max|w_u| / max|x_u|,
    real and imaginary parts combined bilinearly (eight passes); its error is O(step^2) on a term that is smooth in w.
    ``density=True`` divides each node's entries by its lumped volume (``lumped_volumes``) so that maps compare across
    meshes.  Afterwards the problem holds J(w), untransposed."""
    lam, x, z = _sensitivity_pair(problem, result, k, pair)
    w = problem._vec(w)
    pairing = mode_pairing(problem, w, z, x)
    gw = eigenvalue_base_flow_sensitivity(problem, w, pair=(lam, x, z))
    old = problem.options.ksp_rtol
    problem.set_options(ksp_rtol=float(ksp_rtol))
    try:
        problem.jacobian(w, "ns")
        parts = []
        for g in (gw.real.contiguous(), gw.imag.contiguous()):
            y, res = problem.adjoint_solve(g)
            if res.reason <= 0:
                raise RuntimeError(f"eigenvalue_forcing_sensitivity: the adjoint solve ended with reason {res.reason}")
            parts.append(problem.mass_apply_transpose(w, y))
    finally:
        problem.set_options(ksp_rtol=old)
    first = torch.complex(parts[0], parts[1])
    free = torch.from_numpy(problem.bc_mask == 0).to(problem.device)
    wu = float(w.view(-1, 4)[:, :3].abs().max())
    xu = float(torch.view_as_real(x).view(-1, 4, 2)[:, :3].abs().max())
    h = float(fd_rel) * wu / xu

    def dBt(zz, xx):
        step = h * torch.where(free, xx, torch.zeros_like(xx))
        return (problem.mass_apply_transpose(w + step, zz) - problem.mass_apply_transpose(w - step, zz)) / (2.0 * h)
    out = first + _bilinear_complex(dBt, z, x) / pairing
    if density:
        vol = torch.from_numpy(lumped_volumes(problem.mesh)).to(problem.device)
        out = (out.view(-1, 4) / vol[:, None]).reshape(-1)
    return out


def eigenvalue_shape_sensitivity(problem: FlowProblem, w, result: StabilityResult = None, k: int = 0, pair=None,
                                 ksp_rtol: float = 1e-10, return_parts: bool = False):
    """The sensitivity of eigenvalue ``k`` to the geometry (where to reshape a wall or a body to damp a mode or shift its
    frequency), a complex device tensor (n_nodes, 3) over EVERY node coordinate at a converged state ``w``:

        d lam / dX = -( S_J(z, x) + lam S_B(z, x) ) / (z^T B x)  -  mu . dF/dX,      A^T mu = grad_w lam,  mu_B := 0,
        S_A(z, x) = d/dX [ z~^T A(w; X) x~ ]   (``jacobian_shape_gradient``),

    so that d lam = sum(d lam / dX * V), unconjugated, to first order under a deformation field V (n_nodes, 3), the
    re-converged base flow included.  The first term is the explicit dependence of the pencil J x = -lam B x on the mesh at a
    fixed base flow: with z = z_r + i z_i, x = x_r + i x_i, lam = a + i b it is the pass on four real pairs, each with
    (c_jac, c_mass) = (1, a) and (0, b) -- eight passes.  The second is the path through the base flow: F(w; X) = 0 gives
    dw = -A^-1 dF/dX dX, and grad_w lam is ``eigenvalue_base_flow_sensitivity``; it is ``shape_sensitivity`` with
    grad_J = grad_w lam, on the real and on the imaginary part (two adjoint solves with the inner tolerance ``ksp_rtol``; the
    problem's own is restored afterwards).  Neither term is negligible.  Assumptions, as for ``shape_sensitivity``:

      * the Dirichlet values are held AT THE NODES and do not follow the coordinates: a node of an inlet that moves keeps its
        value, and the constrained entries of the modes stay 0;
      * the components on interior nodes are mesh-motion terms of the discrete problem; they vanish only in the limit h -> 0.

    ``pair=(lam, x, z)`` supplies a mode directly instead of ``result`` / ``k``.  ``return_parts=True`` returns
    ``(total, explicit, path)``.  Raises RuntimeError if an adjoint solve does not converge.  Afterwards the problem holds
    J(w), untransposed.  Refused where ``jacobian_shape_gradient`` or ``residual_shape_gradient`` is."""
    lam, x, z = _sensitivity_pair(problem, result, k, pair)
    w = problem._vec(w)
    a, b = lam.real, lam.imag
    s1 = _bilinear_complex(lambda zz, xx: problem.jacobian_shape_gradient(w, xx, zz, 1.0, a), z, x)
    sb = _bilinear_complex(lambda zz, xx: problem.jacobian_shape_gradient(w, xx, zz, 0.0, b), z, x)
    explicit = -(s1 + 1j * sb) / mode_pairing(problem, w, z, x)         # S_J + a S_B + i b S_B
    gw = eigenvalue_base_flow_sensitivity(problem, w, pair=(lam, x, z))
    old = problem.options.ksp_rtol
    problem.set_options(ksp_rtol=float(ksp_rtol))
    try:
        parts = []
        for g in (gw.real.contiguous(), gw.imag.contiguous()):
            dX, _, res = shape_sensitivity(problem, w, g)
            if res.reason <= 0:
                raise RuntimeError(f"eigenvalue_shape_sensitivity: the adjoint solve ended with reason {res.reason}")
            parts.append(dX)
    finally:
        problem.set_options(ksp_rtol=old)
    path = torch.complex(parts[0], parts[1])
    total = explicit + path
    return (total, explicit, path) if return_parts else total


def print_stability(result: StabilityResult, rank: int = 0):
    """One line per converged mode: lam, the frequency Im lam / 2 pi, the residual estimate."""
    if rank != 0:
        return
    for lam, est, ok in zip(result.eigenvalues, result.estimates, result.converged):
        if ok:
            print(f"Stability mode: lambda = {lam.real:+.6e} {lam.imag:+.6e}i  frequency = {lam.imag / (2.0 * np.pi):.6e}  estimate = {est:.2e}",
                  flush=True)


def solve_navier_stokes(problem: FlowProblem, w: torch.Tensor, rank: int = 0, continuation=False, ptc_dt0: float = 1.0):
    """``solve_navier_stokes(a, w, dF, bcs, W, ksp_type, comm, rank)`` (:268-312).

    ``w`` is updated in place (``snes.solve(None, w)`` :293); returns
    ``(w, u, p)`` with u (n,3) and p (n,) the collapsed sub-functions (:310-312).
    ``continuation=True`` (not in the reference) retries a failed solve with Reynolds-number continuation;
    ``continuation="ptc"`` goes through pseudo-transient continuation (``pseudo_transient_solve`` from ``ptc_dt0``).
    """
    if rank == 0:
        print("Running SNES solver", flush=True)
        print("Start Nonlinear Solve", flush=True)
    if continuation == "ptc":
        w_ptc, res = pseudo_transient_solve(problem, w, ptc_dt0, verbose=(rank == 0))
        w.copy_(w_ptc)
    elif continuation:
        w, res = newton_with_reynolds_continuation(problem, w, verbose=(rank == 0))
    else:
        w, res = problem.newton_solve(w)
    if rank == 0:
        print(f"Num SNES iterations: {res.its}", flush=True)
        print(f"SNES termination reason: {res.reason}", flush=True)
        print(f"Navier-Stokes solve time: {res.seconds:.2f} sec", flush=True)
        print("Finished Nonlinear Solve", flush=True)
    problem.last_newton = res
    W = w.view(-1, 4)
    return w, W[:, :3].contiguous(), W[:, 3].contiguous()
