"""Entry points with the reference's command lines, on the HIP hot path.

  NavierStokesChannelFlow.py <Re> <img_fname> <flowrate_ratio> [<channel_mesh_size>=0.1]
        (NavierStokes/NavierStokesChannelFlow.py:81-93, flow :468-580)
  StokesChannelFlow.py       <img_fname> <flowrate_ratio> [<mesh_size>=0.25]
        (StokesFlow/StokesChannelFlow.py:34-41)
  DuctStokesFlow.py          <gmsh_fname> <mesh_lc> <x_outlet>
        (StokesFlow/DuctStokesFlow.py:18-20)
  LidDrivenNavierStokesFlow.py <Re> [<NumCells>=64]
        (LidDrivenFlow/LidDrivenNavierStokesFlow.py:17-23)

What is kept: argv, the Stokes -> coarse NS -> fine NS continuation (:513-530),
boundary-condition sets, solver settings, printed diagnostics, output folder /
file names.  What differs, because gmsh / skimage / dolfinx do not exist offline
(SURVEY 8f, next-row 2): an existing inlet PNG goes through the repository's own
restatement of the reference's pipeline (inlet_contours.py: marching-squares contours,
FFT low-pass, RDP, P1 Poisson profiles with the flow-ratio scaling of image2inlet.py:
240-339) and -- since round 5 -- drives the BODY-FITTED channel of nozzle_mesh.py: the box
4 x 1 x 1 minus the nozzle wall extruded over x in [0, 0.5], tags inlet_1 / inlet_2 /
outlet / wall = 1-4, sizes along x after the reference's Box fields
(image2gmsh3D.py:164-486).  SNS_CHANNEL_MESH=structured selects rounds 2-4's
structured box with the nozzle wall as staircase no-slip nodes (inlet_image.py).
``<img_fname>`` may also be a gmsh ``.msh`` file (tags inlet_1=1, inlet_2=2,
outlet=3, wall=4); with neither, a centred square inner stream with analytic
profiles of the same normalisation is used.  DuctStokesFlow keeps
the geometry/BCs/CLI of the reference file but solves the P1-P1 stabilised form
(the north-star discretisation), not its P2-P1 + MUMPS one.
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

from . import bcs as B, mesh as M
from .interpolate import interpolate_initial_guess

snes_ksp_type = "bicgstab"          # reference: 'tfqmr' (:77); both are short-recurrence Lanczos-type methods


def _continuation() -> bool:
    """SNS_CONTINUATION=1: retry a failed Newton solve with Reynolds-number continuation (the command lines stay
    those of the reference scripts, so this is an environment switch)."""
    return bool(os.environ.get("SNS_CONTINUATION"))


def _viscosity_law():
    """SNS_VISCOSITY_LAW=carreau:<lambda>,<n>,<ratio>: the Navier-Stokes legs of DuctStokesFlow.py and
    NavierStokesChannelFlow.py run with the Carreau law (FlowProblem.set_viscosity_law; the Stokes start stays Newtonian).
    Returns (lambda, n, ratio) or None."""
    spec = os.environ.get("SNS_VISCOSITY_LAW")
    if not spec:
        return None
    kind, _, args = spec.partition(":")
    vals = [float(v) for v in args.split(",")] if args else []
    if kind != "carreau" or len(vals) != 3:
        raise ValueError("SNS_VISCOSITY_LAW=carreau:<lambda>,<n>,<ratio>")
    return tuple(vals)


def _solve_ns(P, w, rank):
    """solve_navier_stokes as the reference calls it; with SNS_VISCOSITY_LAW the problem takes the law first
    (SNS_CONTINUATION=1 then also walks the power-law index down from 1) and the range of nu_e is printed."""
    from .solver import newton_with_law_continuation, solve_navier_stokes
    law = _viscosity_law()
    if law is None:
        return solve_navier_stokes(P, w, rank, continuation=_continuation())
    P.set_viscosity_law(*law)
    if _continuation():
        w0 = w.clone()
        w, res = newton_with_law_continuation(P, w, verbose=(rank == 0))
        if res.reason <= 0:
            w = w0
    out = solve_navier_stokes(P, w, rank, continuation=_continuation())
    nu, _ = P.element_viscosity(out[0])
    if rank == 0:
        print(f"Viscosity law carreau lambda={law[0]:g} n={law[1]:g} ratio={law[2]:g}: min / max nu_e = "
              f"{float(nu.min()):.6e} / {float(nu.max()):.6e}", flush=True)
    return out


def _rank():
    try:
        import torch.distributed as dist
        return dist.get_rank() if dist.is_initialized() else 0
    except Exception:
        return 0


# --------------------------------------------------------------------------- #
# argv
# --------------------------------------------------------------------------- #
def parse_arguments(argv=None):
    """Same contract and error as the reference (:81-93)."""
    argv = sys.argv if argv is None else argv
    if len(argv) not in [4, 5]:
        raise ValueError("Usage: script.py <Re> <img_fname> <flowrate_ratio> [<channel_mesh_size>]")
    Re = int(argv[1])
    given = argv[2]
    img_fname = given[1:] if given.startswith(".") else given         # str.removeprefix(".")  (:87)
    img_fname = os.getcwd() + img_fname                                # (:88-89)
    if os.path.isabs(given) and os.path.exists(given):                 # leniency: an existing absolute path is used as is
        img_fname = given
    flowrate_ratio = float(argv[3])
    channel_mesh_size = float(argv[4]) if len(argv) == 5 else 0.1
    return Re, img_fname, flowrate_ratio, channel_mesh_size


def lc_to_cells(lc: float, length: float = 4.0):
    """Structured stand-in for gmsh's characteristic length: h = lc on a length x 1 x 1 box."""
    n = max(2, int(round(1.0 / lc)))
    return (max(2, int(round(length / lc))), n, n)


# --------------------------------------------------------------------------- #
# mesh + BCs  (generate_mesh :107-116, create_boundary_conditions :127-147)
# --------------------------------------------------------------------------- #
def generate_mesh(img_fname: str, channel_mesh_size: float):
    if _rank() == 0:
        print("Meshing", flush=True)
    if img_fname.endswith(".msh") and os.path.exists(img_fname):
        msh = M.read_msh(img_fname)
        msh.meta.update(kind="channel", tags=dict(M.CHANNEL_TAGS))
    else:
        msh = M.channel_mesh(lc_to_cells(channel_mesh_size))
    if _rank() == 0:
        print(f"Num elem: {msh.num_tets}", flush=True)
    return msh


def create_boundary_conditions(msh, flowrate_ratio):
    p1, p2 = B.two_stream_profiles(flowrate_ratio, msh.meta.get("inner_half_width", 0.25))
    return B.channel_bcs(msh, p1, p2)


def channel_problem_inputs(img_fname: str, flowrate_ratio: float, channel_mesh_size: float):
    """(mesh, bcs) of one continuation stage (generate_mesh + create_boundary_conditions, :107-147).
    An existing image drives the inlet as in image2inlet.py + image2gmsh3D.py: contour pipeline, Poisson profiles and the
    body-fitted nozzle channel (nozzle_mesh.py; SNS_CHANNEL_MESH=structured: the structured box with staircase walls);
    a ``.msh`` file is read as is; anything else falls back to the synthetic centred-square inlet."""
    is_img = img_fname.lower().endswith((".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff")) and os.path.exists(img_fname)
    if is_img:
        if _rank() == 0:
            print("Meshing", flush=True)
        if os.environ.get("SNS_CHANNEL_MESH", "bodyfitted") == "structured":
            from .inlet_image import channel_from_image
            msh, bcs, _ = channel_from_image(img_fname, flowrate_ratio, lc_to_cells(channel_mesh_size))
        else:
            from .nozzle_mesh import channel_from_image_bodyfitted
            msh, bcs, _ = channel_from_image_bodyfitted(img_fname, flowrate_ratio, channel_mesh_size)
        if _rank() == 0:
            print(f"Num elem: {msh.num_tets}", flush=True)
        return msh, bcs
    msh = generate_mesh(img_fname, channel_mesh_size)
    return msh, create_boundary_conditions(msh, flowrate_ratio)


# --------------------------------------------------------------------------- #
# output (make_output_folder :416-465, write_run_metadata :384-413,
#         save_navier_stokes_solution :316-346)
# --------------------------------------------------------------------------- #
def make_output_folder(Re, img_fname, channel_mesh_size):
    cwd = os.getcwd()
    img_name = img_fname[:-4] if img_fname.endswith((".png", ".msh")) else img_fname
    if img_name.startswith(cwd):
        img_name = img_name[len(cwd):]
    if img_name.startswith("/InletImages/"):
        img_name = img_name[len("/InletImages/"):]
    img_name = img_name.strip("/").replace("/", "_")
    mesh_str = str(channel_mesh_size).replace(".", "")
    noether = os.path.join(cwd, "noether_data")
    folder = os.path.join(noether, f"NSChannelFlow_RE{Re}_MeshLC{mesh_str}_{img_name}")
    if _rank() == 0:
        os.makedirs(folder, exist_ok=True)
    return folder, img_name


def write_run_metadata(folder, Re, img_fname, flowrate_ratio, channel_mesh_size, msh, nranks=1):
    if _rank() != 0:
        return
    with open(os.path.join(folder, "RunParameters.txt"), "w") as fh:
        fh.write(f"Re={Re}\n")
        fh.write(f"img_filename={img_fname}\n")
        fh.write(f"Flowrate Ratio={flowrate_ratio}\n")
        fh.write(f"Channel Mesh Size={channel_mesh_size}\n")
        fh.write(f"Pressure DOFs: {msh.num_nodes}\n")
        fh.write(f"Velocity DOFs: {msh.num_nodes}\n")        # dolfinx counts blocked dofs: one per node
        fh.write(f"{nranks} Cores Used\n")


def write_xdmf(path_noext: str, msh, name: str, values: np.ndarray):
    """P1 nodal field as ``<path>.xdmf`` + ``<path>.h5`` -- ``XDMFFile.write_mesh`` + ``write_function`` of
    :333-341.  Same container layout as dolfinx 0.9 writes: ``/Mesh/mesh/geometry`` (N x gdim float64),
    ``/Mesh/mesh/topology`` (E x nodes-per-cell int64), ``/Function/<name>/0`` (N x ncomp float64; a scalar is
    N x 1, a 2-D vector is padded to N x 3 with uz = 0 as dolfinx does), the light data pointing into it with ``Format="HDF"`` items -- so the reference's consumer
    (streamtrace.py:87-96: ``h5f["Function"][name]["0"]``) and ParaView open it unchanged.  h5py does not exist
    offline; the container is written by ``h5lite`` (file-format spec, v1 objects)."""
    from .h5lite import H5Writer
    base = os.path.basename(path_noext)
    dim = int(getattr(msh, "dim", 3))
    cells = msh.tris if dim == 2 else msh.tets
    values = np.asarray(values, dtype=np.float64)
    vals2 = values.reshape(len(values), -1)
    if vals2.shape[1] == 2:
        # dolfinx' XDMF write_function pads a 2-component vector to 3 (XDMF has no 2-vector attribute): N x 3, uz == 0
        vals2 = np.concatenate([vals2, np.zeros((len(vals2), 1))], axis=1)
    ncomp = vals2.shape[1]
    w = H5Writer()
    w.dataset("/Mesh/mesh/geometry", np.asarray(msh.points, dtype=np.float64))
    w.dataset("/Mesh/mesh/topology", np.asarray(cells, dtype=np.int64))
    w.dataset(f"/Function/{name}/0", vals2)
    w.write(path_noext + ".h5")
    atype = "Scalar" if ncomp == 1 else "Vector"
    ttype, npe, gtype = ("Triangle", 3, "XY") if dim == 2 else ("Tetrahedron", 4, "XYZ")
    ncell, nn = len(cells), msh.num_nodes
    xml = f"""<?xml version="1.0"?>
<!DOCTYPE Xdmf SYSTEM "Xdmf.dtd" []>
<Xdmf Version="3.0" xmlns:xi="https://www.w3.org/2001/XInclude">
  <Domain>
    <Grid Name="mesh" GridType="Uniform">
      <Topology TopologyType="{ttype}" NumberOfElements="{ncell}" NodesPerElement="{npe}">
        <DataItem Dimensions="{ncell} {npe}" NumberType="Int" Format="HDF">{base}.h5:/Mesh/mesh/topology</DataItem>
      </Topology>
      <Geometry GeometryType="{gtype}">
        <DataItem Dimensions="{nn} {dim}" Format="HDF">{base}.h5:/Mesh/mesh/geometry</DataItem>
      </Geometry>
    </Grid>
    <Grid Name="{name}" GridType="Collection" CollectionType="Temporal">
      <Grid Name="{name}" GridType="Uniform">
        <xi:include xpointer="xpointer(/Xdmf/Domain/Grid[@GridType='Uniform'][1]/*[self::Topology or self::Geometry])" />
        <Time Value="0" />
        <Attribute Name="{name}" AttributeType="{atype}" Center="Node">
          <DataItem Dimensions="{nn} {ncomp}" Format="HDF">{base}.h5:/Function/{name}/0</DataItem>
        </Attribute>
      </Grid>
    </Grid>
  </Domain>
</Xdmf>
"""
    with open(path_noext + ".xdmf", "w") as fh:
        fh.write(xml)


def read_xdmf_function(path_noext: str, name: str):
    """(points, cells, values) back from a ``write_xdmf`` / dolfinx file pair, the access pattern of
    ``read_mesh_and_function`` (streamtrace.py:58-130): mesh from ``/Mesh/mesh``, data from ``/Function/<name>/0``."""
    from .h5lite import read_datasets
    d = read_datasets(path_noext + ".h5")
    return d["/Mesh/mesh/geometry"], d["/Mesh/mesh/topology"], d[f"/Function/{name}/0"]


def save_navier_stokes_solution(u, p, msh, FolderName, Re):
    if _rank() != 0:
        return
    print("[Rank 0] Starting save_navier_stokes_solution()", flush=True)
    write_xdmf(os.path.join(FolderName, f"Re{Re}ChannelPressure"), msh, "Pressure", np.asarray(p))
    write_xdmf(os.path.join(FolderName, f"Re{Re}ChannelVelocity"), msh, "Velocity", np.asarray(u))
    print("[Rank 0] Solution writing complete.", flush=True)


# --------------------------------------------------------------------------- #
# drivers
# --------------------------------------------------------------------------- #
def _init_distributed():
    """Under ``torchrun`` / ``torch.distributed.run`` (the counterpart of the reference's
    ``mpirun -n 6``, run_all_images.sh:6): one rank per GPU over RCCL."""
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and not dist.is_initialized():
        lr = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(lr)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device(f"cuda:{lr}"))
    return world


def _problem(msh, bcs, **opt):
    """One FlowProblem per rank: element-partitioned when launched on several GPUs."""
    import torch
    from .solver import FlowProblem
    if _init_distributed() > 1:
        opt.pop("device", None)
        return FlowProblem.distributed(msh, bcs, device=f"cuda:{torch.cuda.current_device()}", **opt)
    return FlowProblem(msh, bcs, **opt)


def _to_global_host(P, x):
    """Global nodal vector on the host (identical on every rank)."""
    return (P.gather(x) if getattr(P, "part", None) is not None else x).cpu().numpy()


def _from_global_host(P, xg):
    import torch
    return P.scatter(xg) if getattr(P, "part", None) is not None else torch.from_numpy(np.ascontiguousarray(xg)).to(P.device)


def solve_NS_flow(argv=None, *, coarse_mesh_size: float = 0.1, device="cuda:0", interp_device=None):
    """The reference's three-stage continuation (:468-549): Stokes on the 0.1 mesh ->
    Navier-Stokes on the 0.1 mesh -> Navier-Stokes on the user mesh, each stage
    warm-started from the previous one.  ``interp_device`` (e.g. "cuda:0") runs the coarse-to-fine
    interpolation on that GPU instead of the host (interpolate_initial_guess)."""
    import torch
    from .solver import solve_stokes_problem
    Re, img_fname, flowrate_ratio, channel_mesh_size = parse_arguments(argv)
    rank = _rank()
    if rank == 0:
        print("Accepted Inputs", flush=True)
    # Solve Stokes Flow
    msh, bcs = channel_problem_inputs(img_fname, flowrate_ratio, coarse_mesh_size)
    P = _problem(msh, bcs, reynolds=float(Re), ksp_type=snes_ksp_type, device=device)
    U_stokes = solve_stokes_problem(P, rank)
    # Solve Coarse Navier Stokes
    if rank == 0:
        print("Interpolating Stokes Flow", flush=True)
    w_coarse, u, p = _solve_ns(P, U_stokes.clone(), rank)
    w_coarse_host = _to_global_host(P, w_coarse)
    P.close()
    # Solve Navier Stokes With User Defined Mesh
    msh_f, bcs_f = channel_problem_inputs(img_fname, flowrate_ratio, channel_mesh_size)
    Pf = _problem(msh_f, bcs_f, reynolds=float(Re), ksp_type=snes_ksp_type, device=device)
    if rank == 0:
        print("Interpolating Coarse NS Flow", flush=True)
    w0 = interpolate_initial_guess(msh, w_coarse_host, msh_f, device=interp_device)
    w, u, p = _solve_ns(Pf, _from_global_host(Pf, w0), rank)
    coupled = _coupled_flow(Pf, w, msh_f)                          # opt-in: the two-way coupling replaces the one-way transport
    if coupled is not None:
        w = coupled[0]
    wg = _to_global_host(Pf, w)
    out = dict(msh=msh_f, w=wg, u=wg.reshape(-1, 4)[:, :3].copy(), p=wg.reshape(-1, 4)[:, 3].copy(), Re=Re, img_fname=img_fname,
               channel_mesh_size=channel_mesh_size, flowrate_ratio=flowrate_ratio, newton=Pf.last_newton)
    derived = _derived_fields(Pf, w)
    stab = _stability(Pf, w)
    if stab is not None:
        out["stability"] = stab
    resolvent = _resolvent(Pf, w)
    if resolvent is not None:
        out["resolvent"] = resolvent
    if derived is not None:
        out["derived"] = derived
    conc = coupled[1] if coupled is not None else _scalar_transport(Pf, w, msh_f)
    if conc is not None:
        out["concentration"] = conc
    Pf.close()
    return out


def navier_stokes_channel_main(argv=None):
    t0 = time.time()
    r = solve_NS_flow(argv)
    folder, _ = make_output_folder(r["Re"], r["img_fname"], r["channel_mesh_size"])
    save_navier_stokes_solution(r["u"], r["p"], r["msh"], folder, r["Re"])
    _write_derived_fields(r.get("derived"), r["msh"], lambda label: os.path.join(folder, f"Re{r['Re']}Channel{label}"))
    _write_wavemaker(r.get("stability"), r["msh"], os.path.join(folder, f"Re{r['Re']}ChannelWavemaker"))
    _write_resolvent(r.get("resolvent"), r["msh"], os.path.join(folder, f"Re{r['Re']}ChannelOptimalForcing"))
    if r.get("concentration") is not None and _rank() == 0:
        write_xdmf(os.path.join(folder, f"Re{r['Re']}ChannelConcentration"), r["msh"], "Concentration", r["concentration"])
    write_run_metadata(folder, r["Re"], r["img_fname"], r["flowrate_ratio"], r["channel_mesh_size"], r["msh"])
    if _rank() == 0:
        print(f"Run Time = {time.time() - t0:.2f} sec; output in {folder}", flush=True)
    return r


def stokes_channel_main(argv=None):
    """StokesChannelFlow.py: linear P1-P1 pressure-stabilised Stokes, bcgs rtol=atol=1e-10 (:166)."""
    argv = sys.argv if argv is None else argv
    if len(argv) not in [3, 4]:
        raise ValueError("Usage: script.py <img_fname> <flowrate_ratio> [<mesh_size>]")
    img_fname, ratio = argv[1], float(argv[2])
    mesh_size = float(argv[3]) if len(argv) == 4 else 0.25
    t0 = time.perf_counter()
    msh, bcs = channel_problem_inputs(os.path.abspath(img_fname), ratio, mesh_size)
    P = _problem(msh, bcs, ksp_type="bicgstab", ksp_rtol=1e-10, ksp_atol=1e-10)
    print("\nStart Assembling Stiffness Matrix and Forcing Vector", flush=True)
    U, res = P.stokes_solve()
    print(f"Solve finished: {res.its} iterations, reason {res.reason}, {time.perf_counter() - t0:.2f} s", flush=True)
    W = _to_global_host(P, U).reshape(-1, 4)
    if _rank() == 0:
        write_xdmf("StokesChannelPressure", msh, "Pressure", W[:, 3])
        write_xdmf("StokesChannelVelocity", msh, "Velocity", W[:, :3])
    P.close()
    return msh, W


def duct_stokes_main(argv=None):
    """DuctStokesFlow.py <gmsh_fname> <mesh_lc> <x_outlet> (:18-20): geometry :36-124, BCs :156-183,
    printed norms :234-241 (labels as in the reference: 'L1' is the l2 norm of the coefficient vector)."""
    argv = sys.argv if argv is None else argv
    if len(argv) != 4:
        raise ValueError("Usage: DuctStokesFlow.py <gmsh_fname> <mesh_lc> <x_outlet>")
    gmsh_fname, mesh_lc, x_outlet = argv[1], float(argv[2]), float(argv[3])
    msh = M.duct_mesh(lc_to_cells(mesh_lc, x_outlet), x_outlet)
    M.write_msh2(msh, f"{gmsh_fname}.msh")                        # gmsh.write(f'{gmsh_fname}.msh') :141
    P = _problem(msh, B.duct_bcs(msh))
    U, res = P.stokes_solve()
    if _viscosity_law() is not None:                              # opt-in: a Navier-Stokes leg with the law, from the Stokes start
        U = _solve_ns(P, U.clone(), _rank())[0]
    coupled = _coupled_flow(P, U, msh)                             # opt-in: a coupled Navier-Stokes leg from the state so far
    if coupled is not None:
        U = coupled[0]
    W = _to_global_host(P, U).reshape(-1, 4)
    u, p = W[:, :3], W[:, 3]
    if _rank() == 0:
        print(f"L1 norm of velocity coefficient vector: {np.linalg.norm(u.ravel())}")
        print(f"L1 norm of pressure coefficient vector: {np.linalg.norm(p)}")
        print(f"Linf norm of pressure coefficient vector: {np.abs(u).max()}")
        print(f"Linf norm of pressure coefficient vector: {np.abs(p).max()}")
        write_xdmf("StokesDuctPressure", msh, "f", p)
        write_xdmf("StokesDuctVelcoity", msh, "f", u)             # (sic) file name of the reference :255
    _write_derived_fields(_derived_fields(P, U), msh, lambda label: f"StokesDuct{label}")
    _write_wavemaker(_stability(P, U), msh, "StokesDuctWavemaker")
    _write_resolvent(_resolvent(P, U), msh, "StokesDuctOptimalForcing")
    conc = coupled[1] if coupled is not None else _scalar_transport(P, U, msh)
    if conc is not None and _rank() == 0:
        write_xdmf("StokesDuctConcentration", msh, "Concentration", conc)
    P.close()
    return msh, W, res


def lid_driven_main(argv=None):
    """LidDrivenNavierStokesFlow.py <Re> [<NumCells>=64] (:17-23).

    Default = the script as written: the 2-D unit square, ``create_rectangle`` triangles (:29-30), lid y=1 moving
    with (1,0), no-slip elsewhere, p=0 at the origin (:57-77); Stokes with viscosity nu and mu_T = a0 h^2/(4 nu)
    (:96-109) as initial guess, then the UGN-stabilised NS form (:123-143).  A trailing ``3d`` argument (or
    SNS_CAVITY_DIM=3) runs the 3-D unit-cube extension with the G-metric form instead."""
    import torch
    from .solver import solve_navier_stokes
    argv = list(sys.argv if argv is None else argv)
    three_d = os.environ.get("SNS_CAVITY_DIM", "2") == "3"
    if argv and argv[-1].lower() == "3d":
        three_d = True
        argv = argv[:-1]
    if len(argv) not in [2, 3]:
        raise ValueError("Usage: LidDrivenNavierStokesFlow.py <Re> [<NumCells>] [3d]")
    Re = int(argv[1])
    n = int(argv[2]) if len(argv) == 3 else 64
    t0 = time.time()
    if three_d:
        msh = M.cavity_mesh(n)
        bcs, opt = B.cavity_bcs(msh), {}
    else:
        from . import mesh2d as M2
        nu = 1.0 / Re
        msh = M2.rectangle_mesh(n)
        bcs, opt = M2.cavity2d_bcs(msh), dict(stokes_viscosity=nu, stokes_beta=(1.0 / 3.0) / (4.0 * nu))   # :98-100
    print(f"Pressure Degress of Freedom: {msh.num_nodes}")
    print(f"Velocity Degress of Freedom: {msh.num_nodes}")
    P = _problem(msh, bcs, reynolds=float(Re), **opt)
    U, res = P.stokes_solve()
    print("Solved Stokes Flow")
    w, u, p = solve_navier_stokes(P, U.clone(), _rank(), continuation=_continuation())
    wg = _to_global_host(P, w)
    nd = 3 if three_d else 2
    if _rank() == 0:
        print(f"run time = {time.time() - t0: 0.2f} sec")
        write_xdmf(f"NavierStokesLidDrivenPressureLinear{Re}", msh, "Pressure", wg.reshape(-1, 4)[:, 3].copy())
        write_xdmf(f"NavierStokesLidDrivenPressureVelocity{Re}", msh, "Velocity", wg.reshape(-1, 4)[:, :nd].copy())
    r = P.last_newton
    P.close()
    return msh, wg, r


def lid_driven_stokes_main(argv=None):
    """LidDrivenStokesFlow.py (no arguments): Stokes flow in the 2-D unit square, 64 x 64 ``create_rectangle`` triangles
    (:16-17), lid y = 1 moving with (1, 0), no slip on the other three sides (:20-56), nu = 0.01 and the pressure
    stabilisation mu_T = a0 h^2 / (4 nu), a0 = 1/3 (:67-75), bcgs to 1e-10 (:81), norms of the coefficient vectors (:87-93),
    XDMF + HDF5 output (:100-121).  The script's active element is Taylor-Hood P2-P1 with its P1-P1 line commented out
    (:33-34); here it is the P1-P1 pair with exactly that stabilised form, as for DuctStokesFlow.py.
    The script pins no pressure level; the hot path keeps the cavity's p = 0 at the origin of the NS script (the constant
    is otherwise free)."""
    from . import mesh2d as M2
    argv = list(sys.argv if argv is None else argv)
    n = int(argv[1]) if len(argv) > 1 else 64
    nu = 0.01
    msh = M2.rectangle_mesh(n)
    print(f"There are this Many Degrees of Freedom in the Pressure Nodes: {msh.num_nodes}")
    P = _problem(msh, M2.cavity2d_bcs(msh), reynolds=1.0 / nu, stokes_viscosity=nu, stokes_beta=(1.0 / 3.0) / (4.0 * nu),
                 ksp_type="bicgstab", ksp_rtol=1e-10, ksp_atol=1e-10)
    U, res = P.stokes_solve()
    Ug = _to_global_host(P, U).reshape(-1, 4)
    u, p = Ug[:, :2], Ug[:, 3]
    if _rank() == 0:
        print(f"\nL2 Norm of velocity coefficient vector: {np.linalg.norm(u)}")
        print(f"Infinite Norm of velocity coefficient vector: {np.abs(u).max()}")
        print(f"L2 Norm of pressure coefficient vector: {np.linalg.norm(p)}")
        print(f"Infinite Norm of pressure coefficient vector: {np.abs(p).max()}")
        print("\nFinished Solving, Saving Solution Field")
        write_xdmf("StokesLidDrivenPressureHighRe", msh, "Pressure", p.copy())
        write_xdmf("StokesLidDrivenVelocityHighRe", msh, "Velocity", u.copy())
    P.close()
    return msh, Ug.ravel(), res


def _print_reynolds_sensitivities(P, w, wg, grads, grads_nu, names):
    """SNS_SENSITIVITY=1 (opt-in; single-GPU runs): d<name>/dRe at the converged state for the functionals whose gradients
    are the rows of ``grads`` (``grads_nu``: their derivative with respect to nu at fixed state, the explicit part), one
    adjoint solve each (solver.reynolds_sensitivity)."""
    from .solver import reynolds_sensitivity
    if getattr(P, "part", None) is not None:
        if _rank() == 0:
            print("SNS_SENSITIVITY: adjoint solves run on single-GPU problems only; skipped", flush=True)
        return None
    Re = float(P.options.reynolds)
    out = []
    for name, g, gnu in zip(names, grads, grads_nu):
        d, _, res = reynolds_sensitivity(P, w, g, dJ_dRe_explicit=-float(gnu @ wg) / Re ** 2)
        print(f"d{name}/dRe: {d} (adjoint solve: {res.its} its, reason {res.reason})", flush=True)
        out.append(d)
    return out


def _print_inlet_sensitivities(P, w, grads, names):
    """SNS_INLET_SENSITIVITY=1 (opt-in; single-GPU runs): for the functionals whose gradients are the rows of ``grads``, the
    derivative with respect to the amplitude of the inlet profile at the converged state -- dJ/dg of
    solver.dirichlet_sensitivity (one adjoint solve and one raw-Jacobian pass each) contracted with g on the inlet's velocity
    dofs, the only Dirichlet dofs of these problems whose value is not 0."""
    from .solver import dirichlet_sensitivity
    if getattr(P, "part", None) is not None:
        if _rank() == 0:
            print("SNS_INLET_SENSITIVITY: adjoint solves run on single-GPU problems only; skipped", flush=True)
        return None
    amp = np.where(P.bc_mask.astype(bool), P.bc_val, 0.0)
    amp[3::4] = 0.0
    out = []
    for name, g in zip(names, grads):
        dJ, _, res = dirichlet_sensitivity(P, w, g)
        d = float(dJ.cpu().numpy() @ amp)
        print(f"d{name}/d(inlet amplitude): {d} (adjoint solve: {res.its} its, reason {res.reason})", flush=True)
        out.append(d)
    return out


def _print_radius_sensitivities(P, msh, w, wg, nu):
    """SNS_SHAPE_SENSITIVITY=1 (opt-in; single-GPU runs): dC_d/dr and dC_l/dr, r the cylinder radius, at the converged
    state: the node gradients of solver.shape_sensitivity (one adjoint solve and one element pass each) contracted with
    the radial field mesh2d.dfg2d_radial_field."""
    from . import mesh2d as M2
    from .solver import shape_sensitivity
    if getattr(P, "part", None) is not None:
        if _rank() == 0:
            print("SNS_SHAPE_SENSITIVITY: adjoint solves run on single-GPU problems only; skipped", flush=True)
        return None
    G, E, V = M2.drag_lift_2d_gradient(msh, nu), M2.drag_lift_2d_shape_gradient(msh, wg, nu), M2.dfg2d_radial_field(msh)
    out = []
    for k, name in enumerate(("C_d", "C_l")):
        dJ, _, res = shape_sensitivity(P, w, G[k], E[k])
        d = float((dJ.cpu().numpy() * V).sum())
        print(f"d{name}/dr: {d} (adjoint solve: {res.its} its, reason {res.reason})", flush=True)
        out.append(d)
    return out


DERIVED_FIELD_NAMES = ("vorticity", "q_criterion", "shear_rate")


def _derived_fields(P, w):
    """SNS_DERIVED_FIELDS=1 (opt-in; single-GPU runs): the nodal vorticity, Q-criterion and shear rate of the state ``w`` from
    the recovered gradient (``FlowProblem.derived_fields``) as a dict name -> host array, and one printed line with the
    Zienkiewicz-Zhu estimate (``solver.zz_estimate``).  None without the switch: output and stdout stay as they are."""
    if os.environ.get("SNS_DERIVED_FIELDS", "0") != "1":
        return None
    if getattr(P, "part", None) is not None:
        if _rank() == 0:
            print("SNS_DERIVED_FIELDS: gradient recovery runs on single-GPU problems only; skipped", flush=True)
        return None
    from .solver import zz_estimate
    D = P.derived_fields(w).cpu().numpy()
    eta, eta_rel, _ = zz_estimate(P, w)
    print(f"ZZ error estimate of grad u: eta {eta} eta_rel {eta_rel}", flush=True)
    return dict(vorticity=D[:, :3].copy(), q_criterion=D[:, 3].copy(), shear_rate=D[:, 4].copy())


def _write_derived_fields(fields, msh, path_of):
    """``path_of(label)`` -> file path without extension for the labels Vorticity, QCriterion, ShearRate."""
    if fields is None or _rank() != 0:
        return
    for label, name in zip(("Vorticity", "QCriterion", "ShearRate"), DERIVED_FIELD_NAMES):
        write_xdmf(path_of(label), msh, name, fields[name])


def _stability(P, w):
    """SNS_STABILITY=<n_modes>[,<shift>] (opt-in; single-GPU runs): after the solve, the leading eigenvalues of the transient
    operator linearised at the state ``w`` (``solver.linear_stability``, the 3-D NS form at the problem's Reynolds number), one
    printed line per converged mode: lambda, the frequency Im lambda / 2 pi and the residual estimate.  Re lambda > 0 is a
    growing mode: the steady state is unstable.  Nothing without the switch: files and stdout stay as they are.
    SNS_STABILITY_RESTARTS=<max_restarts>[,<m>[,<keep>]] beside it: the thick-restarted process of ``linear_stability`` (a basis
    of m + 1 vectors instead of 65; m defaults to 64, keep to the function's default) and one more printed line, the restarts
    taken.  Without that variable the call and the output are what they are without it.
    SNS_STABILITY_SHIFT_IMAG=<b> beside it: the shift becomes the complex <shift> + <b> i (``linear_stability`` with a complex
    shift: the eigenvalues nearest a point off the real axis, where a Hopf pair sits; <shift> may then be negative, and b = 0
    serves a negative real shift).  Without that variable the call and the output are what they are without it."""
    spec = os.environ.get("SNS_STABILITY", "")
    if not spec:
        return None
    if getattr(P, "part", None) is not None:
        if _rank() == 0:
            print("SNS_STABILITY: the stability analysis runs on single-GPU problems only; skipped", flush=True)
        return None
    parts = spec.split(",")
    n_modes, shift = int(parts[0]), (float(parts[1]) if len(parts) > 1 else 0.0)
    imag = os.environ.get("SNS_STABILITY_SHIFT_IMAG", "")
    if imag:
        shift = complex(shift, float(imag))
    from .solver import SnsError, linear_stability, print_stability
    sens = os.environ.get("SNS_STABILITY_SENSITIVITY", "0") == "1"
    forcing = os.environ.get("SNS_STABILITY_FORCING", "0") == "1"
    shape = os.environ.get("SNS_STABILITY_SHAPE", "0") == "1"
    restart = {}
    rspec = os.environ.get("SNS_STABILITY_RESTARTS", "")
    if rspec:
        rparts = rspec.split(",")
        restart = dict(max_restarts=int(rparts[0]))
        if len(rparts) > 1:
            restart["m"] = int(rparts[1])
        if len(rparts) > 2:
            restart["keep"] = int(rparts[2])
    try:
        res = (linear_stability(P, w, n_modes=n_modes, shift=shift, left=True, **restart) if sens or forcing or shape
               else linear_stability(P, w, n_modes=n_modes, shift=shift, **restart))
    except SnsError as e:                                 # (a viscosity law, a 2-D problem: the library says which)
        if _rank() == 0:
            print(f"SNS_STABILITY: skipped ({e})", flush=True)
        return None
    print_stability(res, _rank())
    if restart and _rank() == 0:
        print(f"Stability restarts: right {res.restarts}" + (f", left {res.left_restarts}" if sens or forcing or shape else "") +
              f" of at most {restart['max_restarts']} (reason {res.reason}, m_done {res.m_done})", flush=True)
    if sens:
        _stability_sensitivity(P, w, res)
    if forcing:
        _stability_forcing(P, w, res)
    if shape:
        _stability_shape(P, w, res)
    return res


def _resolvent(P, w):
    """SNS_RESOLVENT=<n_modes>,<omega>[,<omega>...] (opt-in; single-GPU runs): after the solve, the resolvent analysis of the flow
    linearised at the state ``w`` (``solver.resolvent_analysis``, the 3-D NS form at the problem's Reynolds number) at every
    frequency listed, one printed line per frequency and mode: omega, the gain sigma and the residual estimate.  Returns the
    result at the frequency of largest leading gain, whose leading forcing and response the scripts write as ...OptimalForcing
    and ...OptimalResponse fields (nodal velocity magnitudes) beside their other files.  Nothing without the switch: files and
    stdout stay as they are."""
    spec = os.environ.get("SNS_RESOLVENT", "")
    if not spec:
        return None
    if getattr(P, "part", None) is not None:
        if _rank() == 0:
            print("SNS_RESOLVENT: the resolvent analysis runs on single-GPU problems only; skipped", flush=True)
        return None
    parts = spec.split(",")
    if len(parts) < 2:
        raise ValueError("SNS_RESOLVENT=<n_modes>,<omega>[,<omega>...]")
    n_modes, omegas = int(parts[0]), [float(v) for v in parts[1:]]
    from .solver import SnsError, print_resolvent, resolvent_analysis
    best = None
    for omega in omegas:
        try:
            res = resolvent_analysis(P, w, omega, n_modes=n_modes)
        except SnsError as e:                             # (a viscosity law, a 2-D problem: the library says which)
            if _rank() == 0:
                print(f"SNS_RESOLVENT: skipped ({e})", flush=True)
            return None
        print_resolvent(res, _rank())
        if len(res.gains) and (best is None or res.gains[0] > best.gains[0]):
            best = res
    return best


def _write_resolvent(res, msh, path_noext):
    """``path_noext`` names the ...OptimalForcing file; the response goes beside it."""
    if res is None or not len(res.gains) or _rank() != 0:
        return
    head, base = os.path.split(path_noext)
    for name, mode in (("OptimalForcing", res.forcing_modes[0]), ("OptimalResponse", res.response_modes[0])):
        mag = mode.reshape(-1, 4)[:, :3].abs().pow(2).sum(dim=1).sqrt().cpu().numpy()
        write_xdmf(os.path.join(head, base.replace("OptimalForcing", name)), msh, name, np.ascontiguousarray(mag))


def _stability_sensitivity(P, w, res):
    """SNS_STABILITY_SENSITIVITY=1 beside SNS_STABILITY: for the leading converged mode that has a left partner, one printed
    line -- d lambda / d Re (``solver.eigenvalue_reynolds_sensitivity``) and the linear estimate of the critical Reynolds number
    -- and the wavemaker map (``solver.structural_sensitivity``) as ``res.wavemaker`` (numpy, one value per node), which the
    script writes as a ...Wavemaker field beside its other files."""
    from .solver import SnsError, eigenvalue_reynolds_sensitivity, structural_sensitivity
    res.wavemaker = None
    lead = [k for k, ok in enumerate(res.left_converged) if ok]
    if not lead:
        if _rank() == 0:
            print("SNS_STABILITY_SENSITIVITY: no converged mode with a converged left partner; skipped", flush=True)
        return
    k = lead[0]
    try:
        res.wavemaker = structural_sensitivity(P, w, res, k).cpu().numpy()
        dlam, Re_c = eigenvalue_reynolds_sensitivity(P, w, res, k)
    except (SnsError, RuntimeError) as e:
        if _rank() == 0:
            print(f"SNS_STABILITY_SENSITIVITY: skipped ({e})", flush=True)
        return
    if _rank() == 0:
        lam = res.eigenvalues[k]
        print(f"Stability sensitivity: lambda = {lam.real:+.6e} {lam.imag:+.6e}i  dlambda/dRe = {dlam.real:+.6e} {dlam.imag:+.6e}i  "
              f"Re_c estimate = {Re_c:.6e}", flush=True)


def _stability_forcing(P, w, res):
    """SNS_STABILITY_FORCING=1 beside SNS_STABILITY: for the leading converged mode that has a left partner, the sensitivity of
    its eigenvalue to a steady body force (``solver.eigenvalue_forcing_sensitivity`` as a nodal density) as
    ``res.forcing_sensitivity`` (numpy complex, n_nodes x 3: the real part moves the growth rate, the imaginary part the
    frequency), which the script writes as ...GrowthRateForcingSensitivity and ...FrequencyForcingSensitivity fields beside the
    ...Wavemaker field, and one printed line: the node and position of the largest |Re grad_f lambda|."""
    from .solver import SnsError, eigenvalue_forcing_sensitivity
    res.forcing_sensitivity = None
    lead = [k for k, ok in enumerate(res.left_converged) if ok]
    if not lead:
        if _rank() == 0:
            print("SNS_STABILITY_FORCING: no converged mode with a converged left partner; skipped", flush=True)
        return
    k = lead[0]
    try:
        g = eigenvalue_forcing_sensitivity(P, w, res, k, density=True)
    except (SnsError, RuntimeError) as e:                 # (a body force or a backflow term on the problem: the library says which)
        if _rank() == 0:
            print(f"SNS_STABILITY_FORCING: skipped ({e})", flush=True)
        return
    res.forcing_sensitivity = g.view(-1, 4)[:, :3].cpu().numpy()
    if _rank() == 0:
        mag = np.linalg.norm(res.forcing_sensitivity.real, axis=1)
        top = int(mag.argmax())
        x = np.asarray(P.mesh.points)[top]
        lam = res.eigenvalues[k]
        print(f"Stability forcing sensitivity: lambda = {lam.real:+.6e} {lam.imag:+.6e}i  max |Re grad_f lambda| = {mag[top]:.6e} "
              f"at node {top}, x = ({x[0]:.6g}, {x[1]:.6g}, {x[2]:.6g})", flush=True)


def _stability_shape(P, w, res):
    """SNS_STABILITY_SHAPE=1 beside SNS_STABILITY: for the leading converged mode that has a left partner, the sensitivity of
    its eigenvalue to every node coordinate (``solver.eigenvalue_shape_sensitivity``) as ``res.shape_sensitivity`` (numpy
    complex, n_nodes x 3: the real part moves the growth rate, the imaginary part the frequency), which the script writes as
    ...GrowthRateShapeSensitivity and ...FrequencyShapeSensitivity fields beside the ...Wavemaker field, and one printed line:
    the boundary node and position of the largest |Re d lambda / dX| (where to reshape the wall; interior components are
    mesh-motion terms of the discrete problem)."""
    from .solver import SnsError, eigenvalue_shape_sensitivity
    res.shape_sensitivity = None
    lead = [k for k, ok in enumerate(res.left_converged) if ok]
    if not lead:
        if _rank() == 0:
            print("SNS_STABILITY_SHAPE: no converged mode with a converged left partner; skipped", flush=True)
        return
    k = lead[0]
    try:
        g = eigenvalue_shape_sensitivity(P, w, res, k)
    except (SnsError, RuntimeError) as e:                 # (a time term, a body force, a traction: the library says which)
        if _rank() == 0:
            print(f"SNS_STABILITY_SHAPE: skipped ({e})", flush=True)
        return
    res.shape_sensitivity = g.cpu().numpy()
    if _rank() == 0:
        mag = np.linalg.norm(res.shape_sensitivity.real, axis=1)
        facets = np.asarray(P.mesh.facets)
        bnd = np.unique(facets) if facets.size else np.arange(len(mag))
        top = int(bnd[mag[bnd].argmax()])
        x = np.asarray(P.mesh.points)[top]
        lam = res.eigenvalues[k]
        print(f"Stability shape sensitivity: lambda = {lam.real:+.6e} {lam.imag:+.6e}i  max |Re dlambda/dX| on the boundary = "
              f"{mag[top]:.6e} at node {top}, x = ({x[0]:.6g}, {x[1]:.6g}, {x[2]:.6g})", flush=True)


def _write_wavemaker(res, msh, path_noext):
    if res is not None and getattr(res, "wavemaker", None) is not None and _rank() == 0:
        write_xdmf(path_noext, msh, "Wavemaker", res.wavemaker)
    if res is not None and getattr(res, "forcing_sensitivity", None) is not None and _rank() == 0:
        for name, part in (("GrowthRateForcingSensitivity", res.forcing_sensitivity.real), ("FrequencyForcingSensitivity", res.forcing_sensitivity.imag)):
            head, base = os.path.split(path_noext)
            write_xdmf(os.path.join(head, base.replace("Wavemaker", name)), msh, name, np.ascontiguousarray(part))
    if res is not None and getattr(res, "shape_sensitivity", None) is not None and _rank() == 0:
        for name, part in (("GrowthRateShapeSensitivity", res.shape_sensitivity.real), ("FrequencyShapeSensitivity", res.shape_sensitivity.imag)):
            head, base = os.path.split(path_noext)
            write_xdmf(os.path.join(head, base.replace("Wavemaker", name)), msh, name, np.ascontiguousarray(part))


def _sensitivity():
    return os.environ.get("SNS_SENSITIVITY", "0") == "1"


def inner_stream_inlet_data(msh):
    """(mask, values), each (n, 1): the inlet-stream indicator as Dirichlet data of one scalar -- c = 1 on the inlet nodes of
    the inner stream, 0 on the other inlet nodes.  A channel mesh carries the two inlet regions as facet tags (the inlet
    pipeline's regions, or the synthetic centred square); a mesh with a single inlet tag (the duct) takes the centred square
    of half width ``meta["inner_half_width"]`` (default 0.25) about the duct's axis."""
    t = msh.meta["tags"]
    n = msh.num_nodes
    mask, val = np.zeros((n, 1), bool), np.zeros((n, 1))
    if "inlet_1" in t:
        inner, outer = msh.facet_nodes(t["inlet_1"]), msh.facet_nodes(t["inlet_2"])
    else:
        outer = msh.facet_nodes(t["inlet"])
        a = float(msh.meta.get("inner_half_width", 0.25))
        yz = msh.points[outer, 1:]
        inner = outer[np.all(np.abs(yz) <= a * (1.0 + 1e-12), axis=1)]
    mask[outer] = mask[inner] = True
    val[inner] = 1.0
    return mask, val


def _scalar_transport(P, w, msh):
    """SNS_SCALAR_PECLET=<Pe> (opt-in; single-GPU runs): after the flow solve, the steady transport of the inlet-stream
    indicator (``inner_stream_inlet_data``) by the velocity of the state ``w`` with kappa = 1/Pe
    (``solver.solve_scalar_transport``), as a host array (n,), and one printed line with its range over the outlet nodes.  None
    without the switch: output and stdout stay as they are."""
    pe = os.environ.get("SNS_SCALAR_PECLET", "")
    if not pe:
        return None
    if getattr(P, "part", None) is not None:
        if _rank() == 0:
            print("SNS_SCALAR_PECLET: scalar transport runs on single-GPU problems only; skipped", flush=True)
        return None
    from .solver import solve_scalar_transport
    pe = float(pe)
    if not pe > 0.0:
        raise ValueError("SNS_SCALAR_PECLET must be a positive Peclet number")
    c, res = solve_scalar_transport(P, w, (1.0 / pe,), inner_stream_inlet_data(msh))
    c = c[:, 0].cpu().numpy()
    out = c[msh.facet_nodes(msh.meta["tags"]["outlet"])]
    print(f"Scalar transport Pe {pe:g}: {res.its} iterations, reason {res.reason}; concentration at the outlet "
          f"min {out.min()} max {out.max()}", flush=True)
    return c


def _coupled_flow(P, w, msh):
    """SNS_VISCOSITY_RATIO=<r> and / or SNS_BUOYANCY=<gx>,<gy>,<gz>, together with SNS_SCALAR_PECLET=<Pe> (opt-in; single-GPU
    runs): the inlet-stream indicator carried by the flow acts back on it -- the inner stream is r times as viscous (log-mixing
    rule) and feels the Boussinesq force c * (gx, gy, gz) -- and ``solver.solve_coupled_flow`` from the state ``w`` takes the
    place of the one-way transport.  Returns (state, concentration (n,) host array) after one printed line with the outer
    iteration count and the line of ``_scalar_transport``; None without the switches: output and stdout stay as they are."""
    ratio, buoy, pe = (os.environ.get(k, "") for k in ("SNS_VISCOSITY_RATIO", "SNS_BUOYANCY", "SNS_SCALAR_PECLET"))
    if not ratio and not buoy:
        return None
    if not pe:
        raise ValueError("SNS_VISCOSITY_RATIO / SNS_BUOYANCY need SNS_SCALAR_PECLET=<Pe>: the coupling acts through the transported scalar")
    if getattr(P, "part", None) is not None:
        if _rank() == 0:
            print("SNS_VISCOSITY_RATIO / SNS_BUOYANCY: the coupled solve runs on single-GPU problems only; skipped", flush=True)
        return None
    from .solver import solve_coupled_flow
    pe, r = float(pe), float(ratio) if ratio else 1.0
    b = tuple(float(x) for x in buoy.split(",")) if buoy else (0.0, 0.0, 0.0)
    if not pe > 0.0 or not r > 0.0 or len(b) != 3:
        raise ValueError("SNS_SCALAR_PECLET and SNS_VISCOSITY_RATIO must be positive, SNS_BUOYANCY three numbers gx,gy,gz")
    w, c, recs = solve_coupled_flow(P, w, (1.0 / pe,), inner_stream_inlet_data(msh), log_viscosity_ratio=float(np.log(r)), buoyancy=b)
    last = recs[-1]
    c = c[:, 0].cpu().numpy()
    out = c[msh.facet_nodes(msh.meta["tags"]["outlet"])]
    print(f"Coupled flow (viscosity ratio {r:g}, buoyancy {b[0]:g},{b[1]:g},{b[2]:g}): {len(recs)} outer iterations, "
          f"{'converged' if last['converged'] else 'NOT converged'}, last change of c {last['change']}; Newton reason "
          f"{last['newton_reason']}, scalar reason {last['scalar_reason']}", flush=True)
    print(f"Scalar transport Pe {pe:g}: {last['scalar_its']} iterations, reason {last['scalar_reason']}; concentration at the outlet "
          f"min {out.min()} max {out.max()}", flush=True)
    return w, c


def dfg_2d_main(argv=None):
    """DFG_2D_Validation.py <msh file> (:22-28): Stokes with unit viscosity and mu_T = 0.2 h^2 (:101-125), NS with
    nu = 1e-3 and the UGN stabilisation from the Stokes field (:141-187), drag / lift and their relative errors
    against the script's constants (:195-214), XDMF output (:216-238).

    ``<msh file>`` is a gmsh ASCII file of dfg_pillar_2D.geo, or ``builtin[:level]`` for the gmsh-free mesh of the
    same geometry (mesh2d.dfg_2d_mesh).  Newton starts from the Stokes field exactly as the script passes it on
    (:141-187).  Only if that solve does NOT converge is it repeated with the Stokes pressure rescaled by nu (the unit-
    viscosity pressure is 1/nu times too large for the NS problem; on meshes coarser than the .geo's the full Newton
    step from the unscaled field diverges, in the oracle's LU-Newton as well) -- a documented fallback, announced on
    stdout; SNS_DFG_RESCALED_GUESS=1 goes straight to the rescaled guess."""
    from . import mesh2d as M2
    from .solver import solve_navier_stokes
    argv = sys.argv if argv is None else argv
    if len(argv) != 2:
        raise ValueError("Usage: DFG_2D_Validation.py <msh file | builtin[:level]>")
    src = argv[1]
    if src.startswith("builtin"):
        msh = M2.dfg_2d_mesh(float(src.split(":")[1]) if ":" in src else 4.0)
    else:
        msh = M2.read_msh_2d(src)
    nu = 1e-3                                                          # :148
    if _rank() == 0:
        print(f"Pressure Degrees of Freedom: {msh.num_nodes}", flush=True)
        print(f"Velocity Degrees of Freedom: {msh.num_nodes}", flush=True)
    P = _problem(msh, M2.dfg2d_bcs(msh), reynolds=1.0 / nu, stokes_viscosity=1.0, stokes_beta=0.2,
                 snes_rtol=1e-9, snes_stol=1e-9)
    U, res = P.stokes_solve()
    if _rank() == 0:
        print("Solved Stokes Flow", flush=True)
    rescale_first = os.environ.get("SNS_DFG_RESCALED_GUESS", "0") == "1"
    U0 = U.clone()
    if rescale_first:
        U0.view(-1, 4)[:, 3] *= nu
    w, u, p = solve_navier_stokes(P, U0.clone(), _rank(), continuation=_continuation())
    if P.last_newton.reason <= 0 and not rescale_first:
        if _rank() == 0:
            print(f"Newton from the unit-viscosity Stokes field did not converge (reason {P.last_newton.reason}): "
                  "repeating with the Stokes pressure rescaled by nu", flush=True)
        U0 = U.clone()
        U0.view(-1, 4)[:, 3] *= nu
        w, u, p = solve_navier_stokes(P, U0, _rank(), continuation=_continuation())
    wg = _to_global_host(P, w)
    cd, cl = M2.drag_lift_2d(msh, wg, nu)
    if _rank() == 0:
        print(f"Coefficient of Lift: {[cl]}", flush=True)
        print(f"Cl Percent Error: {[(cl - M2.DFG2D_CL_REF) / M2.DFG2D_CL_REF]}", flush=True)
        print(f"Coefficient of Drag: {[cd]}", flush=True)
        print(f"Cd Percent Error: {[(cd - M2.DFG2D_CD_REF) / M2.DFG2D_CD_REF]}", flush=True)
        write_xdmf("DFG2DValidationPressure", msh, "Pressure", wg.reshape(-1, 4)[:, 3].copy())
        write_xdmf("DFG2DValidationVelocity", msh, "Velocity", wg.reshape(-1, 4)[:, :2].copy())
    if _sensitivity():
        G1, G0 = M2.drag_lift_2d_gradient(msh, 1.0), M2.drag_lift_2d_gradient(msh, 0.0)
        _print_reynolds_sensitivities(P, w, wg, G0 + nu * (G1 - G0), G1 - G0, ("C_d", "C_l"))
    if os.environ.get("SNS_SHAPE_SENSITIVITY", "0") == "1":
        _print_radius_sensitivities(P, msh, w, wg, nu)
    if os.environ.get("SNS_INLET_SENSITIVITY", "0") == "1":
        _print_inlet_sensitivities(P, w, M2.drag_lift_2d_gradient(msh, nu), ("C_d", "C_l"))
    r = P.last_newton
    P.close()
    return msh, wg, (cd, cl), r


def dfg_3d_main(argv=None):
    """DFG_3D_Validation.py (no arguments: reads ``dfg_pillar_3D.msh`` from the working directory, :73-79): Stokes,
    NS with nu = 1e-3 (:193) from the Stokes field, traction integral over the obstacle (tag 5) and
    C = 2 F / (rho Uc^2 Lc), Uc = 0.2, Lc = 0.1 * 0.41 (:344-367), XDMF output (:381-396).  Without the .msh (gmsh is
    absent offline) the same geometry is meshed by Delaunay (``mesh.dfg_pillar_mesh``; ``builtin[:n]`` as argument picks
    the resolution h = W/n, default 32)."""
    from . import functionals as Fn
    from .solver import solve_navier_stokes
    argv = sys.argv if argv is None else argv
    src = argv[1] if len(argv) > 1 else "dfg_pillar_3D.msh"
    if src.startswith("builtin") or not os.path.exists(src):
        n = int(src.split(":")[1]) if src.startswith("builtin") and ":" in src else 32
        msh = M.reorder_for_locality(M.dfg_pillar_mesh(n, lattice="bcc"))[0]
    else:
        msh = M.read_msh(src)
        msh.meta.setdefault("tags", {"inlet": 2, "outlet": 3, "wall": 4, "obstacle": 5})      # :104-109
        msh.meta.setdefault("width", 0.41)
    nu = 0.001
    if _rank() == 0:
        print(f"Pressure Degrees of Freedom: {msh.num_nodes}", flush=True)
        print(f"Velocity Degrees of Freedom: {msh.num_nodes}", flush=True)
    P = _problem(msh, B.dfg_bcs(msh), reynolds=1.0 / nu, ksp_type=snes_ksp_type)
    U, res = P.stokes_solve()
    if _rank() == 0:
        print("Solved Stokes Flow", flush=True)
    w, u, p = solve_navier_stokes(P, U.clone(), _rank(), continuation=_continuation())
    wg = _to_global_host(P, w)
    force = Fn.boundary_traction_force(msh, wg, nu, msh.meta["tags"]["obstacle"])
    cd, cl = Fn.drag_lift_coefficients(force)
    if _rank() == 0:
        print(f"Coefficient of Lift: {cl}", flush=True)
        print(f"Coefficient of Drag: {cd}", flush=True)
        write_xdmf("DFGValidationPressureNavierStokes", msh, "Pressure", wg.reshape(-1, 4)[:, 3].copy())
        write_xdmf("DFGValidationVelocityNavierStokes", msh, "Velocity", wg.reshape(-1, 4)[:, :3].copy())
    _write_derived_fields(_derived_fields(P, w), msh, lambda label: f"DFGValidation{label}NavierStokes")
    _write_wavemaker(_stability(P, w), msh, "DFGValidationWavemakerNavierStokes")
    _write_resolvent(_resolvent(P, w), msh, "DFGValidationOptimalForcingNavierStokes")
    if _sensitivity():
        sc = Fn.drag_lift_coefficients(np.ones(3))[0]
        ob = msh.meta["tags"]["obstacle"]
        G1, G0 = sc * Fn.boundary_traction_gradient(msh, 1.0, ob)[:2], sc * Fn.boundary_traction_gradient(msh, 0.0, ob)[:2]
        _print_reynolds_sensitivities(P, w, wg, G0 + nu * (G1 - G0), G1 - G0, ("C_d", "C_l"))
    if os.environ.get("SNS_INLET_SENSITIVITY", "0") == "1":
        sc = Fn.drag_lift_coefficients(np.ones(3))[0]
        _print_inlet_sensitivities(P, w, sc * Fn.boundary_traction_gradient(msh, nu, msh.meta["tags"]["obstacle"])[:2], ("C_d", "C_l"))
    r = P.last_newton
    P.close()
    return msh, wg, (cd, cl), r


def streamtrace_main(argv=None):
    """streamtrace.py <img_fname> <solname> <funcname> (:475-491, main :667-689): velocity from ``<solname>.xdmf/.h5``,
    forward trace of the inner inlet mesh, alpha-shape bound, 50 x 50 reverse seeds, contour filter; writes
    ``rev_seeds.csv`` and ``final_output.csv`` next to the image (save_figs :497-520; the SVG figures are not drawn)."""
    from . import streamtrace as ST
    argv = sys.argv if argv is None else argv
    if len(argv) != 4:
        raise ValueError("Usage: script.py <img_fname> <solname> <funcname>")
    img_fname, solname, funcname = argv[1], argv[2], argv[3]
    folder, base = os.path.dirname(os.path.abspath(solname)), os.path.basename(solname)
    if not (base.startswith("Re") and base.endswith("ChannelVelocity")) or funcname != "Velocity":
        raise ValueError("expected <solname> = .../Re<Re>ChannelVelocity and <funcname> = Velocity")
    Re = base[len("Re"):-len("ChannelVelocity")]
    out = ST.for_and_rev_streamtrace_files(50, img_fname, Re, folder, out_dir=os.path.dirname(os.path.abspath(img_fname)))
    print(f"{len(out['final_output'])} of {len(out['rev_seeds'])} reverse seeds end inside the inner inlet contour", flush=True)
    return out


def strouhal_from_lift(t, cl, diameter: float = 0.1, u_mean: float = 1.0, skip: float = 0.5):
    """St = f D / U_mean with f from the upward zero crossings of the lift about its mean over the last ``1 - skip`` of the
    record (linear interpolation between samples).  Returns (St, number of crossings); St is nan with fewer than two."""
    t, cl = np.asarray(t, dtype=np.float64), np.asarray(cl, dtype=np.float64)
    k0 = int(skip * len(t))
    t, c = t[k0:], cl[k0:] - cl[k0:].mean()
    up = np.nonzero((c[:-1] < 0.0) & (c[1:] >= 0.0))[0]
    if len(up) < 2:
        return float("nan"), len(up)
    tc = t[up] - c[up] * (t[up + 1] - t[up]) / (c[up + 1] - c[up])
    return float(diameter / (np.diff(tc).mean() * u_mean)), len(up)


def run_dfg2d2_slab(n: float = 2, dt: float = 0.01, n_steps: int = 800, *, theta_coeff: float = 4.0, corrected_convection: int = 1,
                    device=None, verbose: bool = True, backflow_beta: float = 0.0, **options):
    """The unsteady DFG benchmark 2D-2 (Re = 100: inlet peak 1.5, mean 1.0, nu = 1e-3) through the 3-D kernels, on the
    one-cell slab of ``mesh2d.dfg2d_slab_problem(n, u_max=1.5)``.  NOT in the reference (which has no unsteady form and
    runs 2D-1 only); the steady sibling is ``test_gpu_2d``'s slab series.  Starts from the Stokes solution, steps with
    BDF2 (``solver.solve_unsteady``) and samples C_d(t), C_l(t) per step with the residual-based force
    (``functionals.reaction_force``, consistent with the step's time term).  Prints max C_d, max C_l and the Strouhal
    number of the lift's zero crossings next to the Schaefer-Turek brackets (3.22-3.24, 0.99-1.01, 0.295-0.305), which a
    first-order P1-P1 discretisation on these meshes is not expected to hit.  ``backflow_beta`` > 0 adds the backflow
    term -beta (u.n)_- u.v on the outlet facets (``FlowProblem.set_boundary_flow``), which keeps a vortex that leaves through
    the do-nothing outlet from feeding energy in; the default 0 sets nothing and gives the run without it.  Returns a dict
    with the time series, the per-step records and the three numbers."""
    import torch
    from . import functionals as Fn, mesh2d as M2
    from .solver import FlowProblem, solve_unsteady
    nu = 1e-3
    m3, (mask, g), thick = M2.dfg2d_slab_problem(n, u_max=1.5)
    opts = dict(reynolds=1.0 / nu, corrected_convection=corrected_convection, snes_atol=1e-13, snes_rtol=1e-6, snes_stol=1e-9,
                ksp_rtol=1e-8)
    opts.update(options)
    P = FlowProblem(m3, (mask, g), device=device or f"cuda:{torch.cuda.current_device()}", **opts)
    U, rs = P.stokes_solve()
    if rs.reason <= 0:
        raise RuntimeError(f"Stokes start did not converge (reason {rs.reason})")
    U.view(-1, 4)[:, 3] *= nu                              # (unit-viscosity Stokes pressure -> the NS scaling)
    if backflow_beta > 0.0:
        P.set_boundary_facets(m3.find(m3.meta["tags"]["outlet"]))
        P.set_boundary_flow(backflow=backflow_beta)
    ob = m3.meta["tags"]["obstacle"]
    ts, cds, cls = [], [], []

    def sample(step, t, w):
        cd, cl = Fn.drag_lift_coefficients(Fn.reaction_force(P, w, ob), Uc=1.0, Lc=0.1 * thick)
        ts.append(t), cds.append(cd), cls.append(cl)
        if verbose and step % 50 == 0:
            print(f"  step {step:5d} t {t:7.3f}  C_d {cd:8.4f}  C_l {cl:+8.4f}", flush=True)

    t0 = time.time()
    w, recs = solve_unsteady(P, U, dt, n_steps, order=2, theta_coeff=theta_coeff, callback=sample)
    seconds = time.time() - t0
    P.close()
    half = len(ts) // 2
    cd_max = max(cds[half:]) if ts else float("nan")
    cl_max = max(cls[half:]) if ts else float("nan")
    st, ncross = strouhal_from_lift(ts, cls) if len(ts) > 4 else (float("nan"), 0)
    its = np.array([r["its"] for r in recs], dtype=np.float64)
    kits = np.array([r["ksp_its"] for r in recs], dtype=np.float64)
    if verbose:
        print(f"DFG 2D-2 on the slab, level {n}: {m3.num_tets} tets, dt {dt}, {len(ts)} of {n_steps} steps converged in {seconds:.1f} s, "
              f"Newton its / step {its.mean():.2f}, Krylov its / step {kits.mean():.1f}", flush=True)
        print(f"max C_d {cd_max:.4f} (3.22-3.24)   max C_l {cl_max:.4f} (0.99-1.01)   St {st:.4f} (0.295-0.305; {ncross} upward crossings)",
              flush=True)
    return dict(t=np.array(ts), cd=np.array(cds), cl=np.array(cls), records=recs, cd_max=cd_max, cl_max=cl_max, strouhal=st,
                crossings=ncross, n_tets=m3.num_tets, seconds=seconds, w=w, points=m3.points)


def run_pressure_driven_duct(cells=(12, 4, 4), length: float = 3.0, dp: float = 1.0, reynolds: float = 10.0, *, device=None,
                             verbose: bool = True, **options):
    """A duct driven by a pressure difference alone (NOT in the reference, whose inflows are all Dirichlet profiles): no-slip
    on the wall and nothing else (``bcs.wall_only_bcs``), the traction -dp n on the inlet facets and 0 on the outlet facets
    (``FlowProblem.set_boundary_flow``), Newton from rest.  Under the reference's viscous term the traction is the
    pseudo-traction nu d_n u - p n, so the developed flow has p = dp at the inlet and 0 at the outlet.  Prints the flow rate
    through the inlet and the outlet (outward fluxes of the P1 velocity, exact per facet).  Returns a dict with the state, the
    two fluxes, the Newton result and the mesh."""
    import torch
    from .solver import FlowProblem
    msh = M.duct_mesh(tuple(cells), float(length))
    tags = msh.meta["tags"]
    opts = dict(reynolds=float(reynolds), snes_rtol=1e-10, snes_atol=1e-12, ksp_rtol=1e-10)
    opts.update(options)
    P = FlowProblem(msh, B.wall_only_bcs(msh), device=device or f"cuda:{torch.cuda.current_device()}", **opts)
    inlet, outlet = msh.find(tags["inlet"]), msh.find(tags["outlet"])
    P.set_boundary_facets(np.concatenate([inlet, outlet]))
    P.set_boundary_flow(pressure=np.concatenate([np.full(len(inlet), float(dp)), np.zeros(len(outlet))]))
    w, res = P.newton_solve(P.zeros())
    wh = w.cpu().numpy()
    un = np.einsum("fac,fc->f", wh.reshape(-1, 4)[:, :3][msh.facets[P.boundary_facet_ids].astype(np.int64)], P.boundary_normals) / 3.0
    flux = un * P.boundary_areas
    q_in, q_out = -float(flux[:len(inlet)].sum()), float(flux[len(inlet):].sum())
    P.close()
    if verbose:
        print(f"pressure-driven duct {tuple(cells)}, L {length}, dp {dp}, Re {reynolds}: Newton its {res.its} reason {res.reason}, "
              f"flow rate in {q_in:.6e} out {q_out:.6e}", flush=True)
    return dict(w=wh, q_in=q_in, q_out=q_out, newton=res, mesh=msh)
