/*
 * sns.h -- C ABI of the MI355X-native stabilised Stokes / Navier-Stokes hot path.
 *
 * The reference (mungerct/Stabilized_Navier_Stokes_Flow_FEniCSx) has no FFI:
 * its seam is the PETSc-SNES callback pair plus two driver functions in
 * NavierStokes/NavierStokesChannelFlow.py.  Each entry point below replaces
 * what DOLFINx/FFCx/PETSc do behind the cited reference lines; a maintainer
 * binds them with the ctypes stub shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / HIP types in signatures
 *     (a HIP stream travels as void*).
 *   - "_host" pointers are host memory, "_dev" pointers are device memory of
 *     the GPU the handle was created on.  The caller owns every buffer it
 *     passes; the handle owns mesh, BSR matrix, preconditioner and scratch.
 *   - dof numbering: 4*node + c, c in {ux,uy,uz,p} (node-blocked P1-P1 mixed
 *     space of create_boundary_conditions, :128-129).
 *   - every function returns 0 on success, <0 on a hard error (SNS_E_*);
 *     non-convergence is NOT an error (the reference prints the reason and
 *     carries on, :297-298): it is reported through *reason, whose sign
 *     convention follows PETSc (>0 converged, <0 diverged).
 *   - calls are stream-ordered on the handle's stream and synchronous at
 *     return unless stated otherwise.  With a communicator attached every call
 *     is collective over all ranks (as every PETSc call at :288-293 is).
 */
#ifndef SNS_H
#define SNS_H

#include <stdint.h>

/* libsns.so is built with -fvisibility=hidden: the dynamic symbol table holds exactly the functions declared below */
#if defined(__GNUC__) || defined(__clang__)
#define SNS_API __attribute__((visibility("default")))
#else
#define SNS_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sns_ctx* sns_handle;

/* error codes */
#define SNS_OK            0
#define SNS_E_ARG        -1   /* bad argument / shape mismatch            */
#define SNS_E_HIP        -2   /* HIP runtime error (see sns_last_error)   */
#define SNS_E_STATE      -3   /* call order (e.g. solve before assemble)  */
#define SNS_E_MESH       -4   /* degenerate / inverted input mesh         */
#define SNS_E_COMM       -5   /* RCCL / peer-transport error              */

/* weak forms */
#define SNS_FORM_STOKES   0   /* setup_stokes_weak_form      :160-172 */
#define SNS_FORM_NS       1   /* define_navier_stokes_form   :220-251 */

/* Krylov methods (snes_ksp_type :77, petsc_options :198-202) */
#define SNS_KSP_BICGSTAB  0
#define SNS_KSP_FGMRES    1
#define SNS_KSP_TFQMR     2   /* the reference's snes_ksp_type (:77) */

/* preconditioners */
#define SNS_PC_NONE       0
#define SNS_PC_BJACOBI    1   /* 4x4 nodal block Jacobi                               */
#define SNS_PC_AMG        2   /* aggregation AMG, block-Jacobi smoothing (per-rank)   */

/* converged reasons (PETSc numbering, so logs read like the reference's) */
#define SNS_KSP_CONVERGED_RTOL        2
#define SNS_KSP_CONVERGED_ATOL        3
#define SNS_KSP_DIVERGED_ITS         -3
#define SNS_KSP_DIVERGED_BREAKDOWN   -5
#define SNS_KSP_DIVERGED_NANORINF    -9
/* not a PETSc reason and never the final reason of a solve: what sns_get_counters reports (out[6]) for a FIRST attempt that was
 * ended by the stagnation watch of amg_retry_damping and then retried */
#define SNS_KSP_STALLED              -100
#define SNS_SNES_CONVERGED_FNORM_ABS        2
#define SNS_SNES_CONVERGED_FNORM_RELATIVE   3
#define SNS_SNES_CONVERGED_SNORM_RELATIVE   4
#define SNS_SNES_DIVERGED_LINEAR_SOLVE     -3
#define SNS_SNES_DIVERGED_FNORM_NAN        -4
#define SNS_SNES_DIVERGED_MAX_IT           -5
#define SNS_SNES_DIVERGED_LINE_SEARCH      -6

/* solver knobs; sns_default_options() fills the reference's values.  The shape of the AMG hierarchy (amg_max_levels,
 * amg_coarse_size, amg_agg_size, amg_replicate_rows) is fixed when it is built, lazily at the first sns_pc_setup or
 * solve (after sns_attach_comm, if any): those four must be set before that; every other field can be changed at any
 * time with sns_set_options. */
typedef struct {
    double reynolds;        /* Re, nu = 1/Re                         :223            */
    int    ksp_type;        /* SNS_KSP_*                             :77,:199        */
    int    pc_type;         /* SNS_PC_*                              :200            */
    double ksp_rtol;        /* 1e-8                                  :283            */
    double ksp_atol;        /* 1e-50 (PETSc default)                                 */
    int    ksp_max_it;      /* 10000 (PETSc default)                                 */
    int    gmres_restart;   /* 30 (PETSc default)                                    */
    double snes_rtol;       /* 1e-8                                  :281            */
    double snes_atol;       /* 1e-8                                  :281            */
    double snes_stol;       /* 1e-8 (PETSc default)                                  */
    int    snes_max_it;     /* 30                                    :281            */
    int    amg_max_levels;  /* 12                                                    */
    int    amg_coarse_size; /* stop coarsening at <= this many nodes (dense solve)   */
    int    amg_agg_size;    /* max nodes per aggregate (8)                           */
    int    amg_nu;          /* pre = post smoothing sweeps on the fine level (1)     */
    double amg_omega;       /* block-Jacobi damping (0.8)                            */
    int    monitor;         /* 1: print ||r|| per Krylov/Newton iteration (ksp_monitor / snes_monitor :201,:276) */
    int    corrected_convection; /* 0 = reference as written (dot(u,grad(.)) :241,:247); 1 = (u.grad)(.) */
    int    amg_f32_matrix;  /* storage of the matrix copy the AMG smoother/residual passes read (vectors, D^-1, ALL
                               arithmetic and the Krylov operator stay fp64): 0 = the fp64 operator itself,
                               1 = fp32 copy, 2 (default) = fp16 copy with one fp32 scale per dof row (row-max
                               normalisation; relative perturbation of the preconditioner's matrix <= 2^-11) */
    int    amg_nu_coarse;   /* smoothing sweeps on level 1 (and deeper unless overridden) (4; 0 = same as amg_nu):
                               coarse sweeps are cheap and plain aggregation needs them */
    int    amg_nu_deep;     /* sweeps on levels >= 3 (2; 0 = same as amg_nu_coarse): these levels are launch-bound */
    int    amg_nu_l2;       /* sweeps on level 2 (6; 0 = same as amg_nu_coarse) */
    int    amg_sweep_exchange_rows; /* multi-GPU: AMG levels with at most this many rows per rank exchange the ghost
                               iterate before EVERY smoother sweep (exact global block-Jacobi) instead of smoothing
                               rank-locally; 0 (default) = never.  Fewer iterations, 2*nu instead of 1 exchange per
                               level and cycle */
    int    amg_replicate_rows; /* multi-GPU: the first AMG level (>= 1) with at most this many GLOBAL rows, and all below,
                               are held and cycled redundantly by every rank (values all-gathered at setup, one
                               all-gather of the right-hand side per cycle, no exchanges below); 0 = off.  Default 65536 */
    int    amg_post_exchange; /* multi-GPU: 1 (default) = on levels with ONE post-smoothing sweep (the fine level) one more
                               ghost exchange after the coarse-grid correction, which makes that sweep the exact
                               global block-Jacobi sweep */
    int    assembly_fused;  /* 1: scratch-free Jacobian assembly (each BSR block recomputed by its owner lane) when the
                               state satisfies the Dirichlet data; 0: always the staged element kernel + gather */
    double stokes_viscosity; /* 2-D handles only: viscosity of the Stokes form (1.0: DFG_2D_Validation.py:107-110;
                               nu = 1/Re: LidDrivenNavierStokesFlow.py:96-104) */
    double stokes_beta;     /* 2-D handles only: mu_T = stokes_beta * h^2 (0.2: DFG_2D_Validation.py:104-106;
                               a0/(4 nu), a0 = 1/3: LidDrivenNavierStokesFlow.py:98-100) */
    int    amg_nu_l1_pre;   /* sweeps BEFORE the coarse-grid correction on level 1; the first one is omega D^-1 b from the zero
                               guess, no matrix pass.  0 (default) = automatic, see amg_nu_l1_post */
    int    amg_nu_l1_post;  /* sweeps AFTER the coarse-grid correction on level 1.  Both 0 (default) = automatic: a single-GPU
                               handle runs 1 + (amg_nu_coarse + 2) = 1 + 6 -- post-smoothing is the more valuable half under a
                               piecewise-constant prolongation: the iterations of 4 + 4 with one level-1 matrix pass less
                               (-3 % per Newton iteration on the 10 M-tet duct, neutral on configs 3 / 4, Stokes +1 iteration);
                               a partitioned handle runs amg_nu_coarse + amg_nu_coarse (its post-sweeps are rank-local and
                               1 + 6 costs 8-11 % more iterations there).  Set both (e.g. 4 and 4) to fix the counts */
    int    amg_retry_damping; /* 1 (default): a Krylov solve that ends in BREAKDOWN or NANORINF under SNS_PC_AMG is retried
                               once from the same guess with every level's block-Jacobi damping scaled by 0.7 (see
                               sns_krylov_solve); 0: the failed reason is reported and that is it, as PETSc does */
    int    amg_retry_stall_its; /* with amg_retry_damping: the first BiCGStab attempt is also ended (SNS_KSP_STALLED) and retried when
                               it STAGNATES: no new best residual norm at all for this many iterations, or a best residual
                               still >= the initial one after this many (100; 0 = breakdown / NaN only).  A solve that converges
                               slowly keeps setting new bests and is never touched.  An over-relaxed smoother makes BiCGStab
                               stagnate far more often than break down outright */
    int    halo_overlap;    /* multi-GPU: 1 (default) = level-0 passes compute their interior rows on a second stream while the
                               halo exchange is in flight and the boundary rows after it; 0 = exchange, then one full pass
                               (same arithmetic per row, bitwise the same result).  The environment variable
                               SNS_NO_OVERLAP=1 forces 0 */
    int    amg_fused_post;  /* 1 (default): the coarse-grid correction and the first post-smoothing sweep of a level are ONE
                               pass over M = A P (fine rows x coarse columns, 0.37x the blocks of A on a tet mesh's fine
                               level; same low-precision format as the level matrix): z = (x1 + P xc) + w Dinv (r1 - M xc).
                               The same linear operator as prolongation + sweep up to rounding.  Needs amg_f32_matrix != 0;
                               0 = prolongation kernel + a full sweep over A */
    int    amg_nu_scale_with_size; /* 1 (default): more sweeps on level 2 and the deeper levels of LARGE problems, where they cost
                               next to nothing and the plain-aggregation V-cycle loses convergence with its depth: from 2.5 M fine
                               rows (all ranks together) -- or on a hierarchy of >= 7 levels whose first coarsening keeps more than
                               one row in six, i.e. an unstructured mesh -- amg_nu_l2 + 2 and amg_nu_deep + 2, from 8 M rows + 4 and + 6, from 20 M rows + 6
                               and + 10 (81 M tets on one GPU: 73 / 82 -> 53 / 57 BiCGStab iterations per Newton step, -25 % time;
                               192 M tets: 95 / 108 -> 55 / 66).  0 = the counts as given */
    int    amg_dense_rows;  /* (round 4) the first AMG level >= 1 with at most this many block rows (512 = 2048 dofs by default; a
                               partitioned handle: the first such level of its replicated tail) ends the hierarchy and is solved
                               EXACTLY by one matvec with its explicit inverse (fp32 storage, fp64 accumulation), rebuilt at every
                               numeric setup by a blocked Gauss-Jordan elimination on the fp64 matrix cores (csrc/sns_dense.hip,
                               2 N^3 flops, < 1 ms at N = 2048): one launch instead of the ~15 dependent latency-bound launches
                               of the deepest levels of the V-cycle.  Fixed when the hierarchy is built, like amg_coarse_size.
                               0 = coarsen down to amg_coarse_size nodes as in rounds 1-3 */
    int    amg_block_smooth; /* (round 4) 1 (default): the smoothed levels >= 1 use AGGREGATE-block Jacobi -- the dense block of the
                               <= 8 nodes (32 dofs) that form one node of the next level, inverted at every numeric setup, in place
                               of the 4 x 4 nodal block: x <- x + w B^-1 (b - A x), one launch per sweep like before and worth about
                               two point-block sweeps, so the levels run the shorter schedule below (csrc/sns_block.hip).  The inverse
                               blocks are held in the format of the level's matrix copy (fp16 + one fp32 scale per row by default,
                               2 KiB + 128 B per aggregate; fp32 with amg_f32_matrix = 1).  2: the fine level as well (1 takes it on partitioned handles only, see
                               amg_block_fine_rows).  0: nodal blocks everywhere (rounds 1-3).
                               Needs amg_f32_matrix != 0 and amg_agg_size <= 8; levels where it does not apply keep the nodal
                               blocks and their sweep counts.  Fixed when the hierarchy is built */
    int    amg_bnu_l1;      /* sweeps after the coarse-grid correction on level 1 under amg_block_smooth (3; one sweep before it);
                               a partitioned handle runs amg_bnu_l2 + amg_bnu_l2 there (rank-local post-sweeps, as with amg_nu_l1_*),
                               or, with exact global sweeps (amg_exact_sweeps over a window transport), 1 + (amg_bnu_l1 + 1) */
    int    amg_bnu_l2;      /* sweeps per half cycle on level 2 under amg_block_smooth (4) */
    int    amg_bnu_deep;    /* ... and on levels >= 3 (2: the nodal blocks' count, with the stronger smoother).  amg_nu_scale_with_size adds half of its extra sweeps (rounded up) to both */
    int    amg_ritz_limit;  /* 1 (default): on every level that runs 3 or more sweeps per cycle the damping is also capped by the
                               STABILITY limit of the dominant Ritz values of S A (S = the smoother's block inverse) from 8 Arnoldi
                               steps, w <= min 2 Re(theta) / |theta|^2: the power iteration of rounds 1-3 sees |lambda|max only,
                               and on a convection-dominated coarse level the dominant eigenvalues are complex -- a damping above
                               the limit is amplified by every one of the level's sweeps (jittered 120 x 30 x 30 duct, Re 200:
                               level 1 at w = 0.68 against a limit of 0.45 stalls BiCGStab; oracle/experiments/r4_damping.py).
                               0: the |lambda|max rule alone */
    int    amg_block_max_rows; /* aggregate blocks only on levels with at most this many rows per rank; 0 (default) = no limit.  (While the
                               inverse blocks were fp32 -- 4 KiB per aggregate -- a block sweep cost 1.5x a nodal sweep on a large
                               level and the limit was 8192; in the format of the level's fp16 matrix copy, 2 KiB + row scales, it
                               costs 1.2x and every coarse level gains: 10 M-tet duct 137.5 -> 127-130 ms per Newton iteration) */
    int    amg_block_fine_rows; /* under amg_block_smooth = 1: aggregate blocks on the FINE level too on a PARTITIONED handle (>= 2 ranks)
                               whose fine level has at most this many rows per rank (600000; 0 = never).  The strong split is
                               latency-bound: 15-21 % fewer BiCGStab iterations -- and collectives -- for 6 % more time per
                               iteration (10 M-tet duct on 2 / 4 / 8 ranks: 41 / 43 / 47 -> 35 / 33 / 36 iterations; its 1/8 share on
                               one GPU 19.3-20.2 -> 17.9-18.0 ms per Newton iteration), where a whole mesh on one GPU loses
                               (10 M tets: 42 -> 37 iterations, 129 -> 132 ms; 893 k nodes +2.5 %), which is why a single-GPU
                               handle takes them with amg_block_smooth = 2 only.  Fixed when the hierarchy is built */
    int    amg_fuse_restrict; /* 1 (default): below the fine level the residual r = b - A x, its restriction and the next level's
                               first sweep are ONE launch (k_resid_restrict, csrc/sns_block.hip) instead of two -- every launch down
                               there is 5-8 us of latency.  Same sums in the same order; 0 = the separate kernels; 2 = a single-GPU FINE level as
                               well (measured, no: 0.326 ms against 0.234 + 0.030 for the tuned fine-level residual + restriction) */
    int    halo_windows;    /* (round 5) multi-GPU over the window transports (peer windows; the in-process team): 1 (default) = a halo
                               exchange is ONE launch -- the put into the neighbours' receive windows -- and the level pass that consumes
                               it reads the ghost entries straight from its own window, the waves that meet a ghost column waiting for
                               the neighbours' arrival flags themselves: no unpack kernel, no interior / boundary split, no second
                               stream, no staging copies.  0 = put + wait / unpack into the vector's ghost tail, then the passes of
                               round 4 (the RCCL transport always works that way, with pack + send / recv + unpack) */
    /* (retired in round 5, VERDICT r4 item 6: amg_fine_cycle -- the experimental V(0,1) / V(1,0) fine-level cycles, never the default
       and untested since round 3 --, amg_growth_check -- its value 1 is the rule now, csrc/sns_policy.h takes_growth_check) */
    int    amg_exact_sweeps; /* (round 5) 1 (default): on the window transports the aggregate-block-smoothed PARTITIONED levels >= 1 run
                               the single-GPU schedule (level 1: 1 + (amg_bnu_l1 + 1) sweeps, the coarse-grid correction inside the
                               first post-sweep) with EXACT global sweeps -- a flag wait per sweep, the put rides in the kernel that
                               produces the iterate -- instead of amg_bnu_l2 + amg_bnu_l2 rank-local sweeps with an unfused
                               correction (8-way split of the 10 M-tet duct: 31 / 34 instead of 36 / 36 BiCGStab iterations with 6
                               instead of 9 level-1 launches per cycle).  0, and always over RCCL (an exchange per sweep costs a send / recv group there): round 4's cycle */
    int    amg_aggregation; /* (ABI 8) how the FINE level is aggregated.  0 (default): from the sparsity pattern and the node coordinates
                               (greedy sweep / pairwise by centroids), as before.  1: by operator strength -- s_ij = || D_i^-1/2 A_ij
                               D_j^-1/2 ||_F of the first assembled operator (the Stokes operator of a Newton run), pairwise heavy-edge
                               matching of its strong couplings into aggregates of at most 8 nodes (sns_host_aggregate_strength), frozen
                               for the handle's lifetime -- and the fine level smoothed with the aggregates' dense blocks as under
                               amg_block_smooth = 2 (SNS_LEVEL_AGGREGATE_BLOCKS; amg_block_smooth = 0 or amg_f32_matrix = 0 still turn
                               the blocks off altogether).  For sliver-rich
                               meshes: a sliver's four nodes share an aggregate and its coupling no longer sets the damping of the whole
                               level.  Levels >= 1 keep the default aggregation either way.  2: the IDENTICAL map as 1, built on the
                               device (parallel locally-dominant matching, csrc/sns_aggregate.hip); only the map is copied to the host
                               (10 M tets: 76 ms instead of 0.95 s for 1's host matcher).  Fixed when the hierarchy is built; 1
                               and 2 need an assembled operator then (SNS_E_STATE otherwise), amg_agg_size <= 8, and a 3-D handle
                               (SNS_E_ARG).  3 (hybrid): 0's map, with only the aggregates that cut a dominant coupling (a row
                               whose strongest outside coupling exceeds 4 x max(its strongest inside coupling, its mean coupling))
                               dissolved and their nodes re-matched as 2 matches, on the device; a handle with more than 1 % of its
                               rows marked re-matches everything (2's map).  The fine-level aggregate blocks come only when some
                               rank re-matched; with nothing marked the run is 0's bit for bit, at the cost of the strength kernel
                               and one mark pass.  Same rules as 1 and 2 */
} sns_options;

SNS_API void sns_default_options(sns_options* opt);
SNS_API const char* sns_last_error(void);
SNS_API const char* sns_version(void);
/* ABI guard (round 4): the library's SNS_ABI_VERSION and sizeof(sns_options).  sns_options grows at its END between rounds
 * and the fixed-size out-arrays of the getters below have grown (sns_get_counters / sns_get_kernel_times: 4 -> 8 entries in
 * round 3), so a binding built against an older header would pass short buffers: bindings compare both numbers with the
 * header they were written against before making any other call (the ctypes mirror does, _lib.py) and refuse on a mismatch. */
#define SNS_ABI_VERSION 8
SNS_API int sns_abi_version(void);
SNS_API int64_t sns_options_size(void);
/* Bytes of device memory the library holds right now in this process: every allocation behind the handles, their halo plans
 * and the scratch of the calls in flight, over all devices and threads.  Read-only; it is back at its earlier value once
 * everything created since has been destroyed (device-wide free memory is shared with other processes and says nothing
 * about that).  Not counted: the peer / team transport's windows (sns_peer_create, sns_attach_team), which are shared through
 * IPC and live until sns_peer_destroy / sns_team_destroy. */
SNS_API int64_t sns_live_device_bytes(void);

/* ---- setup: replaces gmshio.model_to_mesh + functionspace + create_matrix +
 *      locate_dofs_topological/dirichletbc (:111,:127-147,:271-272) ----------
 * points_host  [n_nodes*3]   vertex coordinates
 * tets_host    [n_tets*4]    connectivity, cell-local vertex order PRESERVED
 * bc_mask_host [4*n_nodes]   1 where the dof is Dirichlet-constrained
 * bc_val_host  [4*n_nodes]   prescribed value g (ignored where mask==0)
 * device       HIP device ordinal                                              */
SNS_API int sns_create(sns_handle* out, int32_t n_nodes, int64_t n_tets,
               const double* points_host, const int32_t* tets_host,
               const uint8_t* bc_mask_host, const double* bc_val_host,
               int device, const sns_options* opt);
/* 2-D variant (triangles, LidDrivenFlow/LidDrivenNavierStokesFlow.py:29-30 create_rectangle, Validation_Flow/
 * DFG_2D_Validation.py:28 read_from_msh(gdim=2)): points_host [n_nodes*2], tris_host [n_tris*3].  The handle keeps
 * the node-blocked layout of 4 dofs per node [ux, uy, uz, p]; uz is constrained to 0 by the library (identity rows),
 * bc_mask / bc_val still have 4*n_nodes entries.  On such a handle SNS_FORM_STOKES is the pressure-stabilised Stokes
 * form with (stokes_viscosity, stokes_beta) and SNS_FORM_NS the P1-P1 form with the h-based Tezduyar UGN
 * tau_SUPG / tau_LSIC (LidDrivenNavierStokesFlow.py:123-143 == DFG_2D_Validation.py:141-163) and its exact Gateaux
 * derivative; every other entry point works unchanged.  Single GPU only (no sns_attach_comm).                    */
SNS_API int sns_create_2d(sns_handle* out, int32_t n_nodes, int64_t n_tris,
                  const double* points_host, const int32_t* tris_host,
                  const uint8_t* bc_mask_host, const double* bc_val_host,
                  int device, const sns_options* opt);
SNS_API int sns_destroy(sns_handle h);
SNS_API int sns_set_stream(sns_handle h, void* hip_stream);
SNS_API int sns_set_options(sns_handle h, const sns_options* opt);
SNS_API int sns_get_options(sns_handle h, sns_options* opt);
/* DIAGNOSTIC (round 5): perturb the 3-D NS form of define_navier_stokes_form (:220-251) -- the study of what the reference-held
 * constants (DFG_2D_Validation.py:202-203) can tell apart, tests/test_gpu_2d.py.  c_inverse: C_I of the G-metric tau (:237; 36;
 * 0 drops the 36 nu^2 G:G term), lsic_scale: factor on nu_L (:249; 1; 0 = no LSIC term), pspg_sign: sign of (tau res_M, grad q)
 * (:247; +1), one_point_quadrature != 0: the 1-point centroid rule instead of the 4-point rule of dx(degree 2) (:222).  The values
 * in brackets restore the reference's form.  A perturbed form is assembled by the staged element kernel (Jacobian and residual,
 * exact Gateaux derivative of the perturbed form); the matrix must be re-assembled afterwards.                                 */
SNS_API int sns_set_form_variant(sns_handle h, double c_inverse, double lsic_scale, double pspg_sign, int one_point_quadrature);

/* sizes: n_owned = rows this rank owns, n_local = owned + ghost nodes */
SNS_API int sns_get_sizes(sns_handle h, int32_t* n_local_nodes, int32_t* n_owned_nodes,
                  int64_t* n_tets, int64_t* nnz_blocks);

/* ---- distributed setup (one process per GPU; RCCL over xGMI) ---------------
 * Local mesh = owned nodes first [0,n_owned), ghost nodes after; tets = all
 * tets touching an owned node (redundant ghost-tet assembly: no assembly
 * communication, replaces F.ghostUpdate(ADD,REVERSE) :66 and MatAssembly :75).
 * Neighbour k: we send the owned-node values listed in send_idx[send_ptr[k]..)
 * and receive into ghost slots recv_idx[recv_ptr[k]..) (local node ids).
 * nccl_unique_id: 128 bytes from sns_comm_unique_id on rank 0, broadcast by
 * the caller (torch.distributed).  NULL = no communicator: the handle only
 * learns its owned/ghost split and the caller moves ghost values itself
 * (single-GPU tests of the partitioned path).                                  */
SNS_API int sns_comm_unique_id(char id_out[128]);
SNS_API int sns_attach_comm(sns_handle h, int rank, int nranks, const char nccl_unique_id[128],
                    int32_t n_owned_nodes, int n_neighbors, const int32_t* neighbor_ranks,
                    const int32_t* send_ptr, const int32_t* send_idx,
                    const int32_t* recv_ptr, const int32_t* recv_idx);

/* In-process "team" communicator (TEST TRANSPORT): N ranks = N host threads of one
 * process sharing one GPU; halo exchange / all-reduce / all-gather are emulated with
 * barriers and device copies so the N-rank algorithm can be verified on a 1-GPU box.
 * Every rank (thread) attaches its own handle; all collective calls must then be made
 * concurrently from the N threads.  Never used by bench.py or the drivers.          */
SNS_API int sns_team_create(int nranks, void** team_out);
SNS_API int sns_team_destroy(void* team);
SNS_API int sns_attach_team(sns_handle h, void* team, int rank, int nranks,
                    int32_t n_owned_nodes, int n_neighbors, const int32_t* neighbor_ranks,
                    const int32_t* send_ptr, const int32_t* send_idx,
                    const int32_t* recv_ptr, const int32_t* recv_idx);

/* Peer-window communicator (PRODUCT TRANSPORT for the ranks of ONE node, round 4): no library in the data path.  Every rank
 * owns a window of fine-grained device memory that the other ranks map through HIP IPC; halo exchange, all-reduce and
 * all-gather are small kernels that store into the peers' windows over xGMI and raise sequence flags there (csrc/sns_comm.h).
 * It replaces the same PETSc/MPI traffic as sns_attach_comm (VecGhostUpdate inside MatMult, the KSP's MPI_Allreduce) where the
 * RCCL launch floor (~50 us per send/recv group, ~10 us per all-reduce on this image) dominates: the strong split.
 *   sns_peer_create  : allocate this rank's window (window_bytes, 0 = 64 MiB) on `device`; ipc_handle_out = 64 bytes for the peers
 *   sns_peer_connect : ipc_handles = nranks x 64 bytes in rank order (all-gathered by the caller, e.g. torch.distributed);
 *                      call on every rank, then synchronise the ranks once before the first attach
 *   sns_attach_peer  : as sns_attach_comm (same plan arguments; rank / nranks are the communicator's); collective
 *   sns_peer_disconnect : first half of the teardown, after every handle attached to the communicator is destroyed AND the ranks
 *                      have synchronised: unmaps the other ranks' windows.  Synchronise the ranks once more, then
 *   sns_peer_destroy : frees this rank's window (no peer has it mapped any more: the HIP IPC contract leaves freeing a
 *                      still-mapped allocation undefined).  Without a preceding sns_peer_disconnect it does both halves at once
 * At most 16 ranks.  Every device-side wait is bounded (SNS_PEER_TIMEOUT_MS, default 20000): a late or dead peer turns into
 * SNS_E_COMM at the next host synchronisation instead of a hang.                                                          */
SNS_API int sns_peer_create(int device, int rank, int nranks, int64_t window_bytes, void** peer_out, char ipc_handle_out[64]);
SNS_API int sns_peer_connect(void* peer, const char* ipc_handles);
SNS_API int sns_peer_disconnect(void* peer);
SNS_API int sns_peer_destroy(void* peer);
/* Link check between the REAL ranks of a connected communicator (collective, after sns_peer_connect and one synchronisation of the
 * ranks): `rounds` all-reduces whose contributions depend on rank and round, `rounds` all-gathers of 4096 patterned doubles per rank
 * and `rounds` halo exchanges over a ring between the ranks (2048 nodes per direction; read alternately through the wait / unpack
 * kernel and through the level passes' own path: the wait inside the consumer, the ghost entries straight from the window), every
 * value verified.  The first thing to run on a new machine: a visibility problem of the windows shows up here as SNS_E_COMM with a
 * count instead of as a solve that quietly diverges.                                                                              */
SNS_API int sns_peer_check_links(void* peer, int rounds);
/* Self-test and latency probe of the protocol inside ONE process: nranks (2 or 3) threads with a window, a stream and a
 * communicator end each, wired directly (no IPC), a ring of halo links of `halo_nodes` nodes per direction.  Per collective -- halo
 * exchange, all-reduce (4 doubles), all-gather (2048 doubles per rank) -- `reps` rounds with every payload verified, then `reps`
 * timed rounds of the collective alone: us_out = microseconds per round (max over ranks); then three verified rounds of the long forms
 * (an all-reduce of 40 doubles = two launches, an all-gather of more than three staging chunks).  SNS_E_COMM on a wrong value or a timeout. */
SNS_API int sns_peer_selftest(int device, int nranks, int halo_nodes, int reps, double us_out[3]);
SNS_API int sns_attach_peer(sns_handle h, void* peer, int32_t n_owned_nodes, int n_neighbors, const int32_t* neighbor_ranks,
                    const int32_t* send_ptr, const int32_t* send_idx,
                    const int32_t* recv_ptr, const int32_t* recv_idx);

/* ---- hot path --------------------------------------------------------------*/
/* NonlinearPDE_SNESProblem.F (:51-67): F(w) incl. lifting and F_B = w_B - g.
 * form = SNS_FORM_NS, or SNS_FORM_STOKES for the linear residual A w - b.     */
SNS_API int sns_residual(sns_handle h, int form, const double* w_dev, double* F_dev);
/* NonlinearPDE_SNESProblem.J (:69-75): assemble the Jacobian (BC rows+cols
 * zeroed, unit diagonal) into the handle's BSR matrix; if F_dev != NULL the
 * residual is produced by the same fused element pass.                        */
SNS_API int sns_jacobian(sns_handle h, int form, const double* w_dev, double* F_dev);
/* Weighted moments of the RAW residual (variationally consistent boundary forces):
 * out[c] = sum over owned nodes i of phi[i] * R_raw(w)[4 i + c], c = 0..3, summed over the ranks
 * (the handle's all-reduce; every rank returns the same value).  R_raw is the residual of the form
 * assembled WITHOUT lifting and without F_B = w_B - g (DOLFINx assemble_vector(F) alone): on rows
 * that are not Dirichlet rows it is what sns_residual returns for a state that satisfies the
 * Dirichlet data; w need not satisfy it.  phi_dev: one double per local node (owned + ghost; ghost
 * entries are ignored).  With phi = the indicator of the nodes of a tagged surface, -out[0..2] is the
 * force the fluid exerts on it (pseudo-traction -p I + nu grad u, n = -FacetNormal as
 * boundary_traction_force).  Honours corrected_convection and sns_set_form_variant; 2-D handles
 * leave out[2] = 0.  SNS_FORM_STOKES with w_dev == NULL evaluates at w = 0.  Only the cells with a
 * vertex i < n_owned and phi[i] != 0 are visited; deterministic (fixed-order reduction, no atomics).
 * Returns after out_host is written.  SNS_E_ARG: null handle / phi / out, bad form, NS form without
 * a state.                                                                    */
SNS_API int sns_residual_moments(sns_handle h, int form, const double* w_dev, const double* phi_dev, double out_host[4]);
/* Shape gradient of the raw residual, contracted with a dof vector (the reference has no counterpart):
 *     gX[3 k + j] = sum_i lam[i] * d R_raw(w; X)[i] / d X[k][j],   k = local node, j = 0..2
 * with R_raw as for sns_residual_moments (no lifting, no F_B = w_B - g; w need not satisfy the Dirichlet data) and
 * everything but the node coordinates held fixed: the state w, the Dirichlet values, nu, the time-term history d.
 * lam_dev (4*n_local doubles) is used as given, Dirichlet rows included: the caller zeroes the rows it does not want.
 * With lam = an adjoint vector (sns_adjoint_solve) masked on the Dirichlet dofs this is the lam . dF/dX of the adjoint
 * formula dJ/dX = dJ/dX|explicit - lam . dF/dX; with lam = phi e_c it is minus the explicit X-derivative of the
 * residual-based force of sns_residual_moments.  gX_dev (3*n_local doubles) is overwritten; 2-D handles write
 * gX[3 k + 2] = 0, nodes of no cell get 0.  One element pass (one lane per cell, exact reverse-mode derivative of the
 * cell's scalar lam_e . R_e through K = J^-1, |det J|, G and, in 2-D, h) plus a fixed-order sum over each node's cells:
 * no atomics, bitwise reproducible.
 * SNS_FORM_NS on a 3-D handle: the G-metric form (:220-251) with corrected_convection, sns_set_form_variant (one-point
 * quadrature included) and a time term that is set ((u_t, v), res_M + u_t and theta under the root of tau all depend on X
 * through det J, K and G).  SNS_FORM_NS on a 2-D handle: the UGN form; the derivative is that of the branch each
 * conditional takes at the state (|u| <= 1e-8, Re_UGN <= 3) and of the longest edge for h = CellDiameter, which is what
 * differentiating the form as written gives.  It is UNDEFINED where two edges of a cell tie for the longest or a
 * conditional sits on its switch point.  The Stokes forms are not supported (SNS_E_ARG): their stabilisation depends on h
 * as well, and nobody takes an adjoint of the start-up solve.
 * The per-cell gradients are staged in the handle's element scratch: after the call the Fe array of
 * sns_get_element_scratch / SNS_EXPORT_FE holds Ge [n_cells][a][4] = the cell's gradient with respect to its vertex a
 * (components 0..2, slot 3 zero) instead of element residuals.  Nothing else of the handle changes: the assembled matrix,
 * the preconditioner state, the transposed flag, the options and the time term stay bit for bit.
 * SNS_E_ARG: null handle / w / lam / gX, a form other than SNS_FORM_NS.  SNS_E_STATE: a handle with a communicator
 * attached (any transport, also the local-only split; as for the adjoint solves).  Returns after gX_dev is written. */
SNS_API int sns_residual_shape_gradient(sns_handle h, int form, const double* w_dev, const double* lam_dev,
                                        double* gX_dev);
/* Gradient recovery and derived fields of the P1 state (the reference has no counterpart).  w always has 4 dofs per node
 * (u_x, u_y, u_z, p); both dimensions use the same layouts.
 *   Recovered gradient, node i, component c, direction j = 0..2:
 *       G[12 i + 3 c + j] = ( sum_{t in cells(i)} |t| d_j w_c|_t ) / ( sum_{t in cells(i)} |t| ),   |t| = |det J| / d!
 *   the lumped-mass L2 projection of the piecewise-constant gradient onto P1.  Cells of either orientation count with a
 *   positive weight; the sum runs in the fixed order of the node's cell list, so results are bitwise reproducible; a node of
 *   no cell gets zeros.  2-D handles: column j = 2 is 0 and row c = 2 is the gradient of whatever the z dofs hold.
 *   Derived nodal fields from the velocity rows G_u (S, Omega its symmetric and skew parts):
 *       D[6 i + 0..2] = omega = curl u (2-D with u_z = 0: only k = 2 is non-zero),
 *       D[6 i + 3] = Q = (|Omega|_F^2 - |S|_F^2) / 2,   D[6 i + 4] = shear rate sqrt(2 S:S),   D[6 i + 5] = div u = tr G_u.
 *   The shear rate here is the RECOVERED NODAL value, not the per-cell value of sns_element_viscosity.
 * Either output may be NULL (not both); G_dev: 12*n_local doubles, D_dev: 6*n_local doubles.  D does not depend, bit for bit,
 * on whether G is stored.  One pass (4 lanes per node walk the node's cells), no atomics; reads w and the mesh only: no option,
 * time term, viscosity law, form variant or transposed operator matters, and nothing of the handle is written.
 * SNS_E_ARG: null handle / w, both outputs null.  SNS_E_STATE: a handle with a communicator attached (partitioned recovery
 * is not built).  Returns after the outputs are written.                         */
SNS_API int sns_recover_gradient(sns_handle h, const double* w_dev, double* G_dev, double* D_dev);
/* Zienkiewicz-Zhu error indicator per cell, over the velocity rows only, with e_a = G_{node a} - grad u_h|_t:
 *       eta2[t] = int_t |G_h(u) - grad u_h|_F^2 = |t| / ((d+1)(d+2)) * ( sum_a |e_a|_F^2 + |sum_a e_a|_F^2 )
 * (exact: the integrand is the square of a P1 function), and gnorm2[t] = |t| |grad u_h|_t|_F^2, the scale for a relative
 * indicator.  eta2_dev: n_cells doubles; gnorm2_dev: n_cells doubles or NULL; G_dev: a recovered gradient of w_dev from
 * sns_recover_gradient, or NULL (then the handle recovers it into a temporary it frees before returning; same bits).
 * Writes nothing of the handle.  SNS_E_ARG: null handle / w / eta2.  SNS_E_STATE: a handle with a communicator attached (the
 * indicator would need a halo exchange of G).  Returns after the outputs are written. */
SNS_API int sns_error_indicator(sns_handle h, const double* w_dev, const double* G_dev, double* eta2_dev, double* gnorm2_dev);
/* Linear stability of a steady state (the reference has no counterpart: its forms are steady, its Newton converges to unstable
 * steady states without complaint, and nothing in it asks whether the state it returns exists physically).  The linearised
 * transient problem at a state w is B x_t + J x = 0: J the steady Jacobian, B = dR/du_t the Petrov-Galerkin mass operator of
 * the stabilised 3-D NS form at theta = 0 and u_t = 0,
 *       momentum rows (a, i), columns (b, j):  sum_q w_q N_b (N_a + tau_q u_q.grad N_a) delta_ij    (corrected_convection; the
 *                                              reference's own test function dot(u, grad v): tau_q u_i d_j N_a N_b beside the mass)
 *       pressure rows a, columns (b, j):       pspg_sign sum_q w_q tau_q N_b d_j N_a                (B has no pressure columns)
 *   with the quadrature points, tau_q (C_I, nu or the field's nu_t under the root) and the PSPG sign of the handle's present
 *   form -- by definition B = J(sigma = 1, d = -u) - J(sigma = 0) of sns_jacobian under sns_set_time_term, which is affine in
 *   sigma where u_t = 0.  Body force and boundary terms do not enter B.  Rows and columns of constrained dofs are zero.
 * sns_mass_apply: y = B(w) x, matrix-free -- no second operator is stored (B has J's pattern and would cost what J costs): one
 *   owner-computes pass over the node -> cell lists, 4 lanes per row, no atomics, no element scratch, a fixed summation order
 *   (bitwise reproducible).  The pressure and constrained entries of x are ignored; a time term on the handle is ignored too.
 *   SNS_E_ARG: null handle / pointer, a 2-D handle.  SNS_E_STATE: a communicator attached, a viscosity law set.
 * sns_stability_arnoldi: plain Arnoldi (one cycle; restarts: below) on S = (J + shift B)^-1 B, whose Ritz values theta give the eigenvalues
 *   lambda = shift - 1/theta of J x = -lambda B x nearest the shift (x ~ exp(lambda t): Re lambda > 0 is an unstable mode).
 *   With shift > 0 the time term (sigma = shift, theta = 0, d = -shift u(w)) is set, sns_jacobian runs at w, the start vector
 *   (column 0 of V on entry) is zeroed on the constrained dofs, sent through S once (out of the null space of B) and
 *   normalised; then m steps, each one mass pass, one Krylov solve from a zero guess with the handle's ksp / pc options and
 *   damping retry, and classical Gram-Schmidt with one re-orthogonalisation.  A step whose norm after orthogonalisation is
 *   below breakdown_rel times the norm before ends the process (the Krylov space is invariant).  V_dev: (m + 1) * 4*n_local
 *   doubles, the orthonormal basis by columns, zero behind the last one reached; H_host: (m + 1) x m, row major,
 *   S V_m = V_{m+1} H, zero beyond m_done.  *reason: 1 all m steps, 2 breakdown (m_done columns, the subdiagonal entry of the
 *   last is 0), < 0 the SNS_KSP_* reason of an inner solve that did not converge (m_done = the steps completed; the call still
 *   returns SNS_OK).  On return the time term is cleared again (not after SNS_E_HIP); the assembled matrix stays J + shift B.
 *   SNS_E_ARG: null handle / pointer, a 2-D handle, m outside [2, 64], shift negative or not finite, breakdown_rel outside
 *   (0, 1).  SNS_E_STATE: a communicator attached, a time term set, a viscosity law set.
 * The left (adjoint) problem J^T z = -lambda B^T z, i.e. z^T J = -lambda z^T B, has the same eigenvalues; its modes z say where
 *   an eigenvalue is sensitive: with a right mode x of the same lambda, d lambda = -z^T (dJ + lambda dB) x / (z^T B x) to first
 *   order (the matrices are real: the pairing is the unconjugated z^T B x).  B^T is by definition the transpose of the B above.
 * sns_mass_apply_transpose: y = B(w)^T z, matrix-free, the same owner-computes pass (4 lanes per row, no atomics, no scratch,
 *   bitwise reproducible); B^T is as little stored as B (B is strongly non-symmetric, so B x cannot stand in).  On a cell grad z
 *   is constant, so momentum row (a, i) is  sum_q w_q N_a z_i(q) + (sum_q w_q tau_q N_a u_q).grad z_i + pspg_sign (sum_q w_q
 *   tau_q N_a) d_i z_p  (corrected_convection; the reference's test function has sum_j (sum_q w_q tau_q N_a u_q)_j d_i z_j in
 *   the middle).  Unlike B x it READS the pressure entries of z (the PSPG rows of B); constrained entries of z -- a constrained
 *   pressure dof included -- are read as 0.  Pressure rows and constrained rows of y are 0.  Errors as sns_mass_apply.
 * sns_stability_arnoldi_left: the same process on S_L = (J + shift B)^-T B^T with the same arguments, results and reasons: the
 *   operator is assembled as above, transposed in place (sns_transpose_operator), the hierarchy of the transposed operator is
 *   set up, each step is one transposed mass pass and one Krylov solve.  On return the operator is transposed back and the
 *   hierarchy marked stale (as sns_adjoint_solve does; after a solve that did not converge too, not after SNS_E_HIP), the time
 *   term is cleared: the handle holds J + shift B, untransposed, and its form is steady.  Errors as sns_stability_arnoldi.
 * sns_jacobian_state_gradient: the Hessian pass.  For real dof vectors x, z and real scalars c_jac, c_mass,
 *   g_k = sum_ij z~_i x~_j d( c_jac J_ij(w) + c_mass B_ij(w) ) / d w_k  on the unconstrained dofs k and 0 on the constrained
 *   ones: g = grad_w [ z~^T (c_jac J(w) + c_mass B(w)) x~ ] with x~, z~ held fixed -- J = dR_raw/dw of the handle's steady form
 *   (form variant, corrected_convection, nu constant or the viscosity field held fixed), B the operator above, x~ and z~ the
 *   vectors with every constrained entry (all four mask bytes of a node, the pressure's too) read as 0.  Pressure rows of g
 *   are not zero in general (the SUPG / PSPG terms tau(u) grad p . (..u..) couple p and u at second order); the viscous term is
 *   linear in u and drops out.  With a left and a right mode of lambda scaled to z^T B x = 1 the sensitivity of lambda to the
 *   base flow is grad_w lambda = -(H_J(z, x) + lambda H_B(z, x)), four real pairs of passes (solver.py:
 *   eigenvalue_base_flow_sensitivity), and to a steady forcing B^T J^-T grad_w lambda + D_w[B^T z][x]
 *   (eigenvalue_forcing_sensitivity).  One lane per tet differentiates the cell's scalar by hand, tangent along x then reverse
 *   mode; 16 values per tet go to the handle's element scratch and are gathered per row in the fixed order of the node ->
 *   cell lists: no atomics, bitwise reproducible, and doubling both coefficients doubles every bit.  Nothing of the handle
 *   besides the element scratch is written: operator, hierarchy, form and damping state stay what they were.
 *   SNS_E_ARG: null handle / pointer, a 2-D handle, a coefficient that is not finite.  SNS_E_STATE, the handle untouched: a
 *   communicator attached, a viscosity law, a time term, a body force (J then depends on f through dM/dw(w, -f), a second
 *   contraction that is not built) or a backflow coefficient (sns_set_boundary_flow: quadratic in u, its Hessian is not built)
 *   set.  A boundary traction alone (constant in w) and a viscosity field are allowed.
 * sns_jacobian_shape_gradient: the eigenvalue shape pass, the mesh derivative of the same contraction.  For real dof vectors x, z
 *   and real scalars c_jac, c_mass,
 *       gX[3 k + j] = d/dX[k][j] [ z~^T ( c_jac J0(w; X) + c_mass B(w; X) ) x~ ],   k = local node, j = 0..2,
 *   J0 = dR_raw/dw the steady Jacobian of the raw form (no lifting, no Dirichlet rows; with x~ and z~ masked it is the assembled
 *   J on the free dofs), B the operator above, x~ and z~ as for sns_jacobian_state_gradient.  Held fixed: w, x~, z~, the mask
 *   and the Dirichlet values AT THE NODES, nu or the per-cell viscosity field, the form variant.  Nothing drops out here: the
 *   viscous and pressure terms are linear in w but carry grad phi_a and |det J|.  gX_dev (3*n_local doubles) is overwritten;
 *   nodes of no cell get 0; an empty mesh writes zeros.  With a left and a right mode of lambda the explicit part of
 *   d lambda / dX is -(S_J(z, x) + lambda S_B(z, x)) / (z^T B x), four real pairs of passes with (c_jac, c_mass) = (1, Re lambda)
 *   and (0, Im lambda); the base-flow path adds -mu . dF/dX with A^T mu = grad_w lambda (solver.py:
 *   eigenvalue_shape_sensitivity).  One lane per tet differentiates the cell's scalar of the Hessian pass in its 12 vertex
 *   coordinates by hand, tangent along x then reverse mode through K = J^-1, G and |det J|; 16 values per tet go to the
 *   handle's element scratch -- after the call the Fe array of sns_get_element_scratch / SNS_EXPORT_FE holds Ge [n_cells][a][4]
 *   = the cell's gradient with respect to its vertex a, slot 3 zero, as after sns_residual_shape_gradient -- and are summed per
 *   node in the fixed order of the node -> cell lists: no atomics, bitwise reproducible, and doubling both coefficients doubles
 *   every bit.  Nothing of the handle besides the element scratch is written.  Errors exactly as sns_jacobian_state_gradient
 *   (the same request rows): SNS_E_ARG for a null handle / pointer, a 2-D handle, a coefficient that is not finite;
 *   SNS_E_STATE, the handle untouched, with a communicator attached, a viscosity law, a time term, a body force or a backflow
 *   coefficient set (their mesh derivatives inside the contraction are not built); a traction alone and a viscosity field are
 *   allowed (the facet terms do not enter J0's cell part; a traction is constant in w).
 * Thick restart (Stewart's Krylov-Schur) of the process above, for meshes on which (m + 1) basis vectors at m = 64 do not fit
 *   or modes that 64 steps do not reach.  One restart is: the ordered real Schur form H[:m, :m] = Z T Z^T on the host with the
 *   `keep` Ritz values of largest modulus (the eigenvalues nearest the shift) leading (solver.py: krylov_schur_truncate; this
 *   library holds no C implementation of it, sns_host_hessenberg_eigs gives the Ritz values); Q = blockdiag(Z[:, :k], 1) and
 *   H_k = [T[:k, :k]; H[m, :m] Z[:, :k]]; sns_basis_rotate(h, m + 1, k + 1, Q, V); H_k written into the leading (k + 1) x k
 *   block of H (row stride m); sns_stability_arnoldi_extend(..., k, m, ...).
 * sns_basis_rotate: V[:, 0:n_out] <- V[:, 0:n_in] Q in place, then columns n_out .. n_in - 1 of V zeroed; columns from n_in on
 *   are not touched.  V_dev by columns with leading dimension 4*n_local, Q_host n_in x n_out, row major.  One lane per dof holds
 *   its n_in values in registers before it stores any (no second copy of V exists at any time), Q is staged in LDS, every sum
 *   runs over the columns in ascending order: no atomics, bitwise reproducible, one streaming pass (n_in * 4*n_local * 8 B read
 *   and as many written).  Works on any handle (a vector operation on the handle's stream); synchronises the stream before it
 *   returns.  SNS_E_ARG: null handle / pointer, n_in outside [1, 65], n_out outside [1, n_in], a non-finite entry of Q.
 * sns_stability_arnoldi_extend: continues a Krylov decomposition from column k.  On entry columns 0 .. k of V are orthonormal
 *   with zeros on the constrained dofs and the leading (k + 1) x k block of H (row stride m) satisfies S V_k = V_{k+1} H_k --
 *   the caller's contract, not verified.  The operator is assembled, flipped for left != 0, set up and given back exactly as by
 *   sns_stability_arnoldi[_left] (stateless per call on purpose: the handle ends in the same state); there is no start vector
 *   treatment; the rest of H is zeroed and steps j = k .. m - 1 run as above, orthogonalising against all j + 1 columns, so
 *   column j of H is full above the subdiagonal.  m_done = k + the steps completed; reasons, breakdown and the zeroing of the
 *   columns not reached as above.  Errors as sns_stability_arnoldi[_left] by `left`, and SNS_E_ARG for k outside [1, m - 1]
 *   (after the other arguments, before the state).
 * Complex and negative shifts s = shift_re + i shift_im: shift-invert in real Arnoldi arithmetic (Parlett & Saad) on
 *   S = Re[(J + s B)^-1 B], a real operator with the eigenvectors of the pencil, so V, H, sns_basis_rotate and the truncation are
 *   what they are above.  A Ritz value theta of S belongs to lambda with theta = (a - lambda) / ((s - lambda)(conj(s) - lambda)),
 *   a = shift_re: two candidates per theta, told apart by their true residual (solver.py: shifted_eigenpairs).  The inner system
 *   is complex, (P + c B) y = b with P = J + pc_shift B the real matrix the handle assembles and preconditions, c = s - pc_shift.
 *   Complex device vectors are PLANAR: 4*n_local real parts, then 4*n_local imaginary parts, each in the layout of a state vector.
 * sns_shifted_apply: y = A x + (c_re + i c_im) B(w) x, or with transpose != 0 ... B(w)^T x, for planar complex x, y (which must
 *   not overlap); A is whatever matrix the handle holds (for the left problem the caller has flipped it).  Two operator passes
 *   fill y, one pair mass pass adds c B x to both parts (the geometry and tau of a cell formed once for both; each part summed
 *   in the order of sns_mass_apply[_transpose]; no atomics, bitwise reproducible); with c = 0 the result is the operator pass's.
 *   Entries of x are masked as the mass passes mask them.  SNS_E_ARG: null handle / pointer, a 2-D handle, a part of c not
 *   finite.  SNS_E_STATE: a communicator attached, a viscosity law set, no matrix assembled.
 * sns_shifted_solve: (A + c B) x = b by right-preconditioned complex FGMRES -- restart gmres_restart (at most 200), stopping by
 *   ksp_rtol / ksp_atol / ksp_max_it, the preconditioner of A applied to each part, no damping retry; x holds the initial guess
 *   on entry; *reason an SNS_KSP_* reason, *rnorm the true residual norm.  A solve that does not converge returns SNS_OK and
 *   says so in *reason.  Errors as sns_shifted_apply.
 * sns_stability_arnoldi_shifted: the process on Re[(J + s B)^-1 B] (left != 0: on Re[(J + s B)^-T B^T]).  k = 0: a fresh process
 *   as sns_stability_arnoldi[_left] runs it; k >= 1: the continuation of sns_stability_arnoldi_extend.  J + pc_shift B is
 *   assembled through the time term (pc_shift = 0: the plain J) and set up; each step is one mass pass, one complex solve of
 *   (P + (s - pc_shift) B) y = B v from a zero guess, and the real part of y.  V, H, m_done, reason and the state of the handle
 *   on return -- J + pc_shift B, untransposed, the form steady -- as there.  shift_im = 0 serves negative real shifts.
 *   SNS_E_ARG: null handle / pointer, a 2-D handle, m outside [2, 64], k outside [0, m - 1], a shift part or pc_shift not
 *   finite, pc_shift < 0, breakdown_rel outside (0, 1).  SNS_E_STATE: as sns_stability_arnoldi.
 * Not built: explicit locking / deflation of converged pairs, selections other than "nearest the shift", a C implementation of
 * the ordered Schur form, a complex Arnoldi basis; of the sensitivities, base flows with a body
 * force or a backflow term, the sensitivity to forcing on Dirichlet nodes, and the exact form of E = D_w[B^T z][x] (the
 * forcing sensitivity takes it by a central difference of sns_mass_apply_transpose). */
SNS_API int sns_mass_apply(sns_handle h, const double* w_dev, const double* x_dev, double* y_dev);
SNS_API int sns_stability_arnoldi(sns_handle h, const double* w_dev, double shift, int m, double breakdown_rel,
                                  double* V_dev /* (m+1) * 4*n_local; column 0 = start vector on entry */,
                                  double* H_host /* (m+1) x m, row major */, int* m_done, int* total_ksp_its, int* reason);
SNS_API int sns_mass_apply_transpose(sns_handle h, const double* w_dev, const double* z_dev, double* y_dev);
SNS_API int sns_stability_arnoldi_left(sns_handle h, const double* w_dev, double shift, int m, double breakdown_rel,
                                       double* V_dev /* (m+1) * 4*n_local; column 0 = start vector on entry */,
                                       double* H_host /* (m+1) x m, row major */, int* m_done, int* total_ksp_its, int* reason);
SNS_API int sns_jacobian_state_gradient(sns_handle h, const double* w_dev, const double* x_dev, const double* z_dev,
                                        double c_jac, double c_mass, double* g_dev);
SNS_API int sns_jacobian_shape_gradient(sns_handle h, const double* w_dev, const double* x_dev, const double* z_dev,
                                        double c_jac, double c_mass, double* gX_dev /* 3*n_local */);
SNS_API int sns_stability_arnoldi_extend(sns_handle h, const double* w_dev, double shift, int k, int m, double breakdown_rel,
                                         int left, double* V_dev /* (m+1) * 4*n_local; columns 0 .. k on entry */,
                                         double* H_host /* (m+1) x m, row major; the leading (k+1) x k block on entry */,
                                         int* m_done, int* total_ksp_its, int* reason);
SNS_API int sns_basis_rotate(sns_handle h, int n_in, int n_out, const double* Q_host /* n_in x n_out, row major */,
                             double* V_dev /* n_in * 4*n_local */);
SNS_API int sns_shifted_apply(sns_handle h, const double* w_dev, double c_re, double c_im, int transpose,
                              const double* x_dev /* 2 * 4*n_local, planar */, double* y_dev /* 2 * 4*n_local, planar */);
SNS_API int sns_shifted_solve(sns_handle h, const double* w_dev, double c_re, double c_im, int transpose,
                              const double* b_dev /* 2 * 4*n_local, planar */, double* x_dev /* 2 * 4*n_local; the guess on entry */,
                              int* its, int* reason, double* rnorm);
SNS_API int sns_stability_arnoldi_shifted(sns_handle h, const double* w_dev, double shift_re, double shift_im, double pc_shift,
                                          int k, int m, double breakdown_rel, int left,
                                          double* V_dev /* (m+1) * 4*n_local; column 0 = start vector (k = 0), columns 0 .. k */,
                                          double* H_host /* (m+1) x m, row major; the leading (k+1) x k block on entry (k >= 1) */,
                                          int* m_done, int* total_ksp_its, int* reason);
/* Resolvent analysis of a steady state w of the 3-D NS form (no counterpart in the reference): how strongly the linearised flow
 * amplifies a harmonic body force f exp(i omega t), and which force it amplifies most.  The response is q = R f,
 * R = (J + i omega B)^-1 B; the gains are the singular values of R with the response in kinetic energy, q^H Q q, and the forcing
 * in the lumped volume norm, f^H M_L f.  Complex device vectors are planar, as above.
 * sns_energy_apply: y = Q x, Q = D_chi M D_chi with M the consistent P1 Galerkin mass matrix on the three velocity components
 *   (on a tet M_ab = |det J| (1 + delta_ab) / 120; pressure rows and columns 0) and D_chi the nodal weight chi_dev (n_local
 *   doubles; NULL: all ones), which restricts the norm to a region.  parts = 1: real x, y of 4*n_local; parts = 2: planar complex
 *   x, y, each part summed exactly as parts = 1 sums it.  Matrix-free, one pass over the node -> cell lists, no atomics, bitwise
 *   reproducible.  Constrained entries of x are read as 0, pressure entries are not read; constrained rows and pressure rows of y
 *   are 0.  x and y must not be the same vector.  Reads the mesh and the mask alone: a viscosity law or a time term does not
 *   refuse it.  SNS_E_ARG: null handle / pointer (chi_dev may be NULL), a 2-D handle, parts not 1 or 2, x_dev == y_dev.
 *   SNS_E_STATE: a communicator attached.
 * sns_lumped_volumes: m_i = sum over the cells of node i of |det J| / 24 (a quarter of their volumes) into the three velocity
 *   slots of node i, 0 into its pressure slot; no mask.  Same pass, same order, bitwise reproducible.  Errors as
 *   sns_energy_apply without its arguments.
 * sns_resolvent_lanczos: m steps without restart of the Hermitian Krylov process on
 *       T = S B^T (J + i omega B)^-H Q_q (J + i omega B)^-1 B S,     S = D_f M_L^-1/2 on the velocity dofs, 0 elsewhere,
 *   whose eigenvalues are the squared gains; with a Ritz vector g the optimal forcing is f = S g, of unit M_L norm where
 *   chi_f = 1.  chi_f_dev, chi_q_dev: nodal weights of the forcing and of the response (n_local doubles each; NULL: all ones).
 *   J is assembled at w as the steady form and set up; per step: S, the pair mass pass, the complex solve of
 *   (J + i omega B) q = b from a zero guess (the method of sns_shifted_solve, the handle's ksp options), the energy pass, the
 *   operator flipped in place and set up, the solve of (J^T - i omega B^T) y = r, the operator flipped back and set up, the
 *   transposed pair mass pass, S, classical Gram-Schmidt with one re-orthogonalisation in the complex inner product, and the
 *   breakdown test by the norm ratio against breakdown_rel.  Column 0 of V is the start vector on entry; the call zeroes its
 *   pressure and constrained entries and normalises it.  V: (m + 1) planar complex columns of 2 * 4*n_local doubles, zero behind
 *   the last one reached; H: (m + 1) x m complex, row major, (re, im) interleaved, T V_m = V_{m+1} H.  *reason: 1 all m steps,
 *   2 breakdown (the Krylov space is invariant: m_done columns; m_done = 0: the mask annihilates the start vector), < 0 the
 *   SNS_KSP_* reason of an inner solve that did not converge -- the call then returns SNS_OK with m_done = the steps completed.
 *   On every return except SNS_E_HIP the handle holds J untransposed, its hierarchy set up, no time term.
 *   SNS_E_ARG: null handle / pointer (the weights may be NULL), a 2-D handle, m outside [2, 64], omega not finite, breakdown_rel
 *   outside (0, 1), V_dev the same vector as w_dev or a weight.  SNS_E_STATE: as sns_stability_arnoldi.
 * Not built: 2-D and partitioned handles, the Carreau law, restarts of this process, norms other than kinetic energy over lumped
 * volume, forcing through Dirichlet data, gain sensitivities, transient growth. */
SNS_API int sns_energy_apply(sns_handle h, const double* chi_dev /* n_local or NULL */, int parts /* 1 or 2 */,
                             const double* x_dev, double* y_dev);
SNS_API int sns_lumped_volumes(sns_handle h, double* m_dev /* 4*n_local */);
SNS_API int sns_resolvent_lanczos(sns_handle h, const double* w_dev, double omega, int m, double breakdown_rel,
                                  const double* chi_f_dev /* n_local or NULL */, const double* chi_q_dev /* n_local or NULL */,
                                  double* V_dev /* (m+1) * 2 * 4*n_local; column 0 = start vector on entry */,
                                  double* H_host /* (m+1) x m complex, row major, (re, im) interleaved */,
                                  int* m_done, int* total_ksp_its, int* reason);
/* The raw Jacobian and the Dirichlet values of a live handle (no counterpart in the reference).
 * sns_raw_jacobian_apply: y = J0(w) x for transposed == 0, y = J0(w)^T x otherwise, J0 = dR_raw/dw the exact Gateaux derivative
 *   of the raw residual sns_residual_moments sums -- without lifting and without the Dirichlet rows' w_B - g.  With K_t the
 *   element Jacobian of cell t,  y[4i+c] = sum_{t containing i, a = loc(i,t)} sum_b sum_d K_t[(a,c),(b,d)] x[4 n_b + d],  and
 *   K_t[(b,d),(a,c)] in its place for the transpose.  No mask is applied anywhere: x is used as given on constrained dofs and
 *   every row of y is written; w need not satisfy the Dirichlet data.  2-D handles: the uz rows and columns are 0.  The pass
 *   follows what the handle's NS assembly follows -- corrected_convection, a set time term (sigma, theta, d), the Carreau law,
 *   a body force, a viscosity field -- and its free x free blocks are the assembled Jacobian's own arithmetic (the same block
 *   code).  The [B, free] block is what differentiates the residual-based force (functionals.reaction_force_gradient), the
 *   [free, B] block what differentiates the state with respect to the Dirichlet values (solver.dirichlet_sensitivity); the
 *   assembled operator holds neither.  Matrix-free, one pass over the node -> cell lists, 4 lanes per row, quad sums in a fixed
 *   order: no atomics, no scratch, bitwise reproducible.  Nothing of the handle is written.  form: SNS_FORM_NS (the G-metric
 *   form on 3-D handles, the UGN form on 2-D handles, with the branch every conditional takes at the state).
 *   SNS_E_ARG: null handle / pointer, x_dev == y_dev, a form other than SNS_FORM_NS.  SNS_E_STATE: a communicator attached, a
 *   backflow coefficient set (the backflow term's share of J0 is not built; a traction alone is constant in w and allowed), a
 *   perturbed form variant (sns_set_form_variant: the block code holds the reference's constants only).
 * sns_set_dirichlet_values: new Dirichlet VALUES for a live handle, 4 * n_nodes doubles on the host.  The mask stays what
 *   sns_create got; entries of unconstrained dofs are ignored and the uz slots of a 2-D handle stay 0.  Every later residual,
 *   Jacobian and solve takes the new values, bit for bit as a handle created with them; an assembled matrix, the hierarchy and
 *   the smoother's estimates stay what they were (none depends on the values).  Synchronises the handle's stream.
 *   SNS_E_ARG, the handle untouched: null handle / pointer, a non-finite value on a constrained dof.  SNS_E_STATE: a
 *   communicator attached. */
SNS_API int sns_raw_jacobian_apply(sns_handle h, int form, const double* w_dev, const double* x_dev, int transposed, double* y_dev);
SNS_API int sns_set_dirichlet_values(sns_handle h, const double* bc_val_host);
/* MatMult with the assembled operator: y = A x (halo exchange inside).  Acts on whatever
 * the handle holds: y = A^T x after sns_transpose_operator.                   */
SNS_API int sns_spmv(sns_handle h, const double* x_dev, double* y_dev);
/* PCSetUp / PCApply for the current matrix (of A^T while the handle is transposed). */
SNS_API int sns_pc_setup(sns_handle h);
SNS_API int sns_pc_apply(sns_handle h, const double* r_dev, double* z_dev);
/* KSPSolve: A x = b with the handle's ksp/pc options (A^T x = b while the handle is
 * transposed); x_dev holds the initial
 * guess on entry.  rnorm = 2-norm of the TRUE residual b - A x at exit.  With
 * amg_retry_damping (default on) a solve that ends in DIVERGED_BREAKDOWN or
 * DIVERGED_NANORINF (or, BiCGStab, stagnates for amg_retry_stall_its iterations: first-attempt
 * reason SNS_KSP_STALLED) under SNS_PC_AMG is retried ONCE from the same guess with every
 * level's block-Jacobi damping scaled by 0.7; the factor stays until the next
 * sns_set_options.  *its then counts both attempts (<= 2 ksp_max_it), *reason is the
 * last attempt's, the first attempt's is out[6] of sns_get_counters.  Running out of
 * iterations (DIVERGED_ITS) is never retried.                                    */
SNS_API int sns_krylov_solve(sns_handle h, const double* b_dev, double* x_dev,
                     int* its, int* reason, double* rnorm);
/* ---- adjoint solves: MatTranspose / KSPSolveTranspose on the Jacobian the SNES callback J assembled
 *      (NavierStokesChannelFlow.py:69-75) --------------------------------------------------------------
 * sns_transpose_operator flips the assembled fine operator IN PLACE between A and A^T and toggles the handle's flag.
 * The P1-P1 pattern is structurally symmetric with sorted rows and the Dirichlet rule zeroes rows and columns, so A^T
 * keeps rowptr / colind: block (i, j) of A^T is the transposed 4 x 4 block of slot (j, i), and the transpose is a
 * permutation of vals (csrc/sns_transpose.hip; pure data movement, a second call restores the bits).  The slot -> partner
 * map (4 B per block) is built at the first call and kept by the handle.  The preconditioner must be set up again
 * (sns_pc_setup, or the next solve does it) and re-estimates its smoother damping: the caps were taken on the other
 * operator.  The hierarchy of the flipped values is the hierarchy of A^T (P^T A^T P = (P^T A P)^T); the cycle's sweep
 * schedules stay as they are.  Every assembly into the handle (sns_jacobian, and those inside sns_stokes_solve /
 * sns_newton_solve) overwrites vals with A and clears the flag.  sns_spmv, sns_pc_setup, sns_pc_apply, sns_krylov_solve,
 * sns_get_bsr and sns_export act on whatever the handle holds.
 * SNS_E_STATE: no assembled matrix; a handle with a communicator attached (any transport, also the local-only split: a
 * rank's ghost rows are not complete rows of A).  SNS_E_MESH: the pattern is not structurally symmetric; nothing is
 * modified.  2-D handles work as they are.                                                                          */
SNS_API int sns_transpose_operator(sns_handle h);
SNS_API int sns_operator_is_transposed(sns_handle h, int* flag);
/* A^T lam = g_dev with the handle's ksp / pc options, lam_dev holding the initial guess on entry: transpose,
 * sns_pc_setup, the Krylov solve (damping retry as in sns_krylov_solve), transpose back -- also after a solve that did
 * not converge, not after SNS_E_HIP / SNS_E_COMM -- and the preconditioner marked stale, so that the handle holds A as
 * before and the next solve sets up for it.  rnorm = 2-norm of the TRUE residual g - A^T lam at the end of the Krylov
 * solve; a converged solve then returns lam_B = g_B exactly on the Dirichlet dofs (unit rows and columns of A), which
 * only removes their part of that residual.  With g = dJ/dw of a
 * functional J at a converged state w and A the Jacobian assembled there, dJ/dq = dJ/dq|explicit - lam . dF/dq for a
 * parameter q of the residual F (solver.reynolds_sensitivity): one linear solve instead of two nonlinear ones per
 * parameter.  Errors as sns_transpose_operator and sns_krylov_solve.                                                 */
SNS_API int sns_adjoint_solve(sns_handle h, const double* g_dev, double* lam_dev, int* its, int* reason, double* rnorm);
/* ---- scalar transport on the flow mesh: four species through one solve (the reference has no counterpart; it answers "where
 *      does the inner stream go" kinematically, with streamlines) ------------------------------------------------------------
 * Species k = 0..3 in the node-blocked layout [c0, c1, c2, c3] of the flow state (c_dev, src_dev, cmask_dev, cval_dev, rhs_dev:
 * 4*n_local entries each), carried by the P1 velocity u of the state w_dev (its pressure slots are ignored):
 *     R_k(c; v) = int (sigma c + u.grad c - s_k)(v + tau_k u.grad v) + kappa_k grad c . grad v dx = 0,
 *     tau_k = (theta + u.G u + C_I kappa_k^2 G:G)^(-1/2),   C_I = 36, G = K^T K (the flow form's metric, :232-237),
 * tau_k taken at each point of the 4-point degree-2 rule every integral uses (:222).  Inside a P1 tet the Laplacian of c
 * vanishes, so the strong residual is sigma c + u.grad c - s.  sigma >= 0 and theta >= 0 are shared by the species; src_dev is a
 * nodal P1 source or NULL for zero.  Steady transport: sigma = theta = 0.  Age of fluid: s = 1, c = 0 at the inlet.  An implicit
 * BDF1 step: sigma = 1/dt, s = c^n/dt, theta = 4/dt^2.  Cells of either orientation count with |det J|.
 * Dirichlet data of the scalars are the caller's, independent of the flow's (cmask_dev / cval_dev), and are treated as the flow
 * operator treats its own: rows and columns zeroed, diagonal one, b_i -= sum_{j in B} A0_ij g_j, b_B = g.  Every other boundary
 * is natural (zero diffusive flux).  A species without a Dirichlet node under sigma = 0 is singular (constants lie in its
 * kernel); this is NOT detected.  An unused species: constrain all of its dofs (identity rows).
 * The species do not couple, so the operator is blockdiag(A_0..A_3) in the handle's BSR pattern: every 4 x 4 block is diagonal,
 * stored with its twelve explicit zeros.  sns_scalar_system writes it into the handle's fine-level values (all of them) and the
 * right-hand side into rhs_dev in one scratch-free owner-computes pass (csrc/sns_scalar.hip: no atomics, fixed summation order,
 * bitwise reproducible; the only device memory it adds is the handle's copy of cmask, 4*n_local bytes).  It leaves the scalar
 * operator as the handle's matrix under the contract of any assembly: the transposed flag is cleared, the preconditioner is
 * stale, and the next sns_pc_setup re-estimates the smoother damping (also after a change of kappa, sigma or theta).
 * sns_spmv, sns_pc_setup, sns_pc_apply, sns_krylov_solve, sns_transpose_operator, sns_adjoint_solve (lam_B = g_B on the SCALARS'
 * Dirichlet dofs), sns_get_bsr and sns_export then act on it; the next sns_jacobian (or flow solve) restores the flow operator.
 * The hierarchy keeps the aggregates it was built with; its transfer operators leave out the Dirichlet dofs of the operator in
 * the handle, so the fine level's free mask is rewritten from cmask here and from the flow's mask at the next flow assembly (in
 * place, O(n); the set-up that every assembly makes stale rebuilds what depends on it).  Where sns_scalar_system is the
 * handle's first assembly the hierarchy is built at the following set-up from the scalar operator's pattern -- the same
 * pattern -- and amg_aggregation = 1, 2 or 3 take their strengths from the scalar operator, for the rest of the handle's life.
 * sns_scalar_solve = sns_scalar_system + sns_pc_setup + the Krylov solve with the handle's options (damping retry as in
 * sns_krylov_solve); c_dev holds the guess on entry and the solution on exit, rnorm = the 2-norm of the TRUE residual; a
 * converged solve returns the Dirichlet data exactly.  Neither call writes the time term, the viscosity law, the form variant or
 * the options.  Not built: 2-D handles, partitioned handles, discontinuity capturing (expect over- and undershoots of a few
 * per cent at sharp layers).  The coupling of c back into the flow is sns_set_mixture below.
 * SNS_E_ARG: null handle / w / kappa / mask / values / output; a 2-D handle; a kappa_k that is <= 0 or not finite; sigma or
 * theta negative or not finite.  SNS_E_STATE: a handle with a communicator attached (any transport, also the local-only split).
 * After an error the handle's matrix is untouched.  Both return after their outputs are written.                          */
SNS_API int sns_scalar_system(sns_handle h, const double* w_dev, const double kappa[4], double sigma, double theta,
                              const double* src_dev, const uint8_t* cmask_dev, const double* cval_dev, double* rhs_dev);
SNS_API int sns_scalar_solve(sns_handle h, const double* w_dev, const double kappa[4], double sigma, double theta,
                             const double* src_dev, const uint8_t* cmask_dev, const double* cval_dev, double* c_dev, int* its,
                             int* reason, double* rnorm);
/* solve_stokes_problem (:197-218): assemble + lift + KSP; U_dev receives U.   */
SNS_API int sns_stokes_solve(sns_handle h, double* U_dev, int* ksp_its, int* reason, double* rnorm);
/* solve_navier_stokes (:268-312): SNES newtonls + bt; w_dev updated in place
 * (snes.solve(None, w) :293).  fnorm_hist (nullable) gets ||F|| per iteration
 * (snes_monitor :276), at most hist_cap entries.                              */
SNS_API int sns_newton_solve(sns_handle h, double* w_dev, int* its, int* reason,
                     int* total_ksp_its, double* fnorm_hist, int hist_cap);
/* Time term of the 3-D NS form.  The reference has no counterpart: all of its forms are steady; this is the standard
 * VMS / SUPG-PSPG extension of its G-metric form (:220-251).  With the discrete time derivative u_t = sigma u + d (d_dev:
 * 4*n_local doubles, node-blocked like the state, pressure slots ignored; copied into a buffer the handle owns) every NS
 * assembly of the handle from this call on -- sns_residual, sns_jacobian, sns_newton_solve, sns_residual_moments,
 * sns_bench_assemble -- takes the transient form: (u_t, v) joins the Galerkin part, res_M becomes res_M + u_t in the SUPG
 * and the PSPG term, and tau = (theta + u.Gu + C_I nu^2 G:G)^-1/2 (nu_LSIC = 1/(tr G tau) with the same tau; theta =
 * 4/dt^2 is the usual choice, 0 keeps the steady tau).  The Jacobian is the exact Gateaux derivative with d held fixed.
 * BDF1: sigma = 1/dt, d = -u^n/dt;  BDF2: sigma = 3/(2 dt), d = (-2 u^n + u^(n-1)/2)/dt.  sigma = 0, theta = 0 and
 * d_dev = NULL remove the term: the handle is the steady handle again, bit for bit.  The Stokes form ignores the term;
 * sns_set_form_variant and corrected_convection apply as for the steady form.  An assembled matrix stays what it was;
 * a change of sigma or theta makes the next preconditioner set-up re-estimate its smoother damping.
 * SNS_E_ARG: a 2-D handle; sigma or theta negative or not finite; sigma > 0 without d_dev.  SNS_E_STATE: a handle with
 * a communicator attached (any transport, also the local-only split; as for the adjoint solves).                     */
SNS_API int sns_set_time_term(sns_handle h, double sigma, double theta, const double* d_dev);
/* One implicit time step of the transient form above (the reference has no counterpart).  On entry w_dev = u^n with
 * p^n as the pressure guess and wprev_dev = u^(n-1) (ignored, may be NULL, for order 1).  Builds d on the device (order
 * 1: BDF1, order 2: BDF2), sets the term with theta = theta_coeff / dt^2 and runs the Newton loop of sns_newton_solve
 * (same options, same line search) from the guess u^n.  On exit w_dev = u^(n+1) and, where given, wprev_dev = u^n.  The
 * term stays set, so sns_residual_moments returns the force consistent with the step just taken.  Non-convergence is
 * reported through *reason as everywhere else; w_dev and wprev_dev then hold their entry values.  total_ksp_its may be
 * NULL.  SNS_E_ARG: order outside {1, 2}, dt <= 0, order 2 without wprev_dev, and as sns_set_time_term; SNS_E_STATE
 * as there.                                                                                                          */
SNS_API int sns_time_step(sns_handle h, double* w_dev, double* wprev_dev, double dt, int order, double theta_coeff,
                          int* its, int* reason, int* total_ksp_its);
/* Generalised-Newtonian viscosity of the 3-D NS form (the reference has no counterpart: every form of it has the constant
 * nu = 1/Re).  law = SNS_LAW_CARREAU: on each tet, with eps = sym(grad u) (constant on a P1 tet) and
 *   s = 2 eps:eps (= gamma_dot^2),   nu_e = nu0 (r + (1 - r) (1 + lambda^2 s)^((n-1)/2)),   nu0 = 1/Re, r = nu_inf_ratio,
 * every NS assembly of the handle from this call on -- sns_residual, sns_jacobian, sns_newton_solve, sns_adjoint_solve's
 * operator, sns_residual_moments, sns_bench_assemble -- takes
 *   - the viscous Galerkin term in the stress-divergence form (2 nu_e eps(u), grad v).  The reference's nu (grad u, grad v)
 *     (:244) is a momentum flux only for a constant nu; for a constant nu the two differ by nu (grad u^T, grad v), so a
 *     Carreau law with lambda = 0 or n = 1 is NOT the law-off handle: it is the Newtonian stress-divergence form;
 *   - res_M unchanged (div(2 nu_e eps(u)) vanishes inside a P1 element, as div sigma does at :240-241);
 *   - tau = (u.Gu + C_I nu_e^2 G:G)^-1/2 and nu_LSIC = 1/(tr G tau) with that tau.
 * The Jacobian is the exact Gateaux derivative: with d nu_e = nu'(s) 4 eps(u):grad(du) the velocity-velocity part gains
 * nu_e (grad du^T, grad v) and the rank-one block 4 |T| nu' (2 eps g_a)(eps g_b)^T, and d tau, d nu_LSIC gain the
 * derivative of nu_e under the root.  s enters without a square root, so the form is smooth at rest.  law =
 * SNS_LAW_NEWTONIAN clears the law (the other arguments are ignored): the handle is the Newtonian handle again, bit for
 * bit.  The Stokes form ignores the law; sns_set_form_variant and corrected_convection apply as without one.  An assembled
 * matrix stays what it was; a change of law makes the next preconditioner set-up re-estimate its smoother damping.
 * SNS_E_ARG: a 2-D handle; an unknown law; lambda negative or not finite; n <= 0 or not finite; nu_inf_ratio negative or
 * not finite.  SNS_E_STATE: a handle with a communicator attached; a handle with a time term set (sns_set_time_term and
 * sns_time_step refuse the same way while a law is set, and so does sns_residual_shape_gradient: the mesh derivative of
 * nu_e is not built).                                                                                                  */
#define SNS_LAW_NEWTONIAN 0
#define SNS_LAW_CARREAU 1
SNS_API int sns_set_viscosity_law(sns_handle h, int law, double lambda, double n, double nu_inf_ratio);
/* Per-tet viscosity of the state w_dev under the handle's law: nu_dev[t] = nu_e (nu0 = 1/Re without a law),
 * gamma_dot_dev[t] = sqrt(2 eps:eps); n_tets doubles each, either may be NULL.  SNS_E_ARG: a 2-D handle, no state.    */
SNS_API int sns_element_viscosity(sns_handle h, const double* w_dev, double* nu_dev, double* gamma_dot_dev);
/* Two external fields of the 3-D NS form (the reference has no counterpart: no form of it has a right-hand side, and its
 * viscosity is the constant 1/Re).  Both are copied into buffers the handle owns (allocated at the first set); NULL clears.
 *   sns_set_body_force         f_dev: 4*n_local doubles, node-blocked like the state, pressure slots ignored: a P1 force
 *                              density f on the right-hand side of the momentum equation;
 *   sns_set_element_viscosity  nu_dev: n_tets doubles nu_t, every one finite and > 0 (checked on the device: one reduction
 *                              launch, one host read; a bad entry gives SNS_E_ARG and leaves the handle untouched).
 * From the call on every NS assembly of the handle -- sns_residual, sns_jacobian, sns_newton_solve, sns_time_step,
 * sns_adjoint_solve's operator, sns_residual_moments, sns_bench_assemble -- takes, with u_t = sigma u + d the handle's time
 * term (0 without one) and a = u_t - f:
 *   - (a, v) added to the Galerkin part (:243-246) and res_M = dot(u, grad(u)) + grad p + a in the SUPG and the PSPG term;
 *   - without a viscosity field the reference's viscous term nu (grad u, grad v) (:244), nu = 1/Re: a body force alone does
 *     not change the viscous form;
 *   - with a viscosity field the stress-divergence form (2 nu_t eps(u), grad v), as under the Carreau law
 *     (div(2 nu_t eps(u)) vanishes inside a P1 tet with a per-tet nu_t, so res_M has no viscous part);
 *   - tau = (theta + u.Gu + C_I nu_t^2 G:G)^-1/2 and nu_LSIC = 1/(tr G tau), nu_t = 1/Re where no field is set.
 * The Jacobian is the exact Gateaux derivative with f, nu_t and d held fixed (f enters it through d tau . res_M; against the
 * law it gains nu_t (grad du^T, grad v) and no nu' terms).  The handle keeps the caller's d, the caller's f and the effective
 * history d - f the kernels read, rewritten whenever d or f changes (sns_time_step included).  The Stokes form ignores both
 * fields; sns_set_form_variant and corrected_convection apply as without them.  Clearing both gives back the handle as it
 * was, bit for bit.  An assembled matrix stays what it was; a changed viscosity field makes the next preconditioner set-up
 * re-estimate its smoother damping, a changed body force does not.
 *   sns_set_mixture  the convenience for two miscible fluids: from a nodal P1 field m_dev (n_local doubles, typically species
 *                    0 of a scalar solve) it sets, in one small kernel (csrc/sns_form.hip),
 *                      nu_t = (1/Re) exp(log_viscosity_ratio * 1/4 sum_a m_a)   (log-mixing rule at the centroid: positive
 *                                                                               whatever over- or undershoot m has),
 *                      f_a  = m_a * buoyancy                                    (Boussinesq; buoyancy = Ri * g_hat).
 *                    It reads opt.reynolds AT THE CALL: a later sns_set_options does not rescale the field.
 *                    log_viscosity_ratio == 0 clears the viscosity field, buoyancy == {0,0,0} (or NULL) clears the body
 *                    force, m_dev == NULL clears both.
 * sns_element_viscosity reports the field where one is set.
 * SNS_E_ARG: a null handle; a 2-D handle; a viscosity entry that is <= 0 or not finite; a log ratio or buoyancy that is not
 * finite.  SNS_E_STATE: a handle with a communicator attached (any transport, also the local-only split); a handle with a
 * Carreau law set (sns_set_viscosity_law(CARREAU) refuses the same way while either field is set, and so does
 * sns_residual_shape_gradient: the mesh derivative is not built with them).  After a refusal the handle is untouched.      */
SNS_API int sns_set_body_force(sns_handle h, const double* f_dev);
SNS_API int sns_set_element_viscosity(sns_handle h, const double* nu_dev);
SNS_API int sns_set_mixture(sns_handle h, const double* m_dev, double log_viscosity_ratio, const double buoyancy[3]);

/* Boundary terms (the reference has no counterpart: every form of it is a volume integral, every outlet do-nothing): facet
 * integrals over a list of boundary facets the handle keeps (csrc/sns_boundary.hip).  A facet k has three nodes, area |Gamma_k|
 * and the outward unit normal n_k -- outward = away from the fourth vertex of the tet that owns it.
 *   sns_set_boundary_facets  facets_host: 3*n_facets node ids (any winding), facet_tets_host: the owning tet of each (host
 *                            arrays, read before the call returns).  Builds the lists of the pass -- the facets rewound
 *                            outward, the boundary rows, per row its (facet, vertex) entries (sns_host_facet_lists) -- and finds
 *                            the BSR slot of every (facet, a, b) once, on the device.  Replaces an earlier list and CLEARS the
 *                            data of the two setters below (they are per facet); n_facets = 0 clears facets and data.
 *   sns_set_boundary_flow    the 3-D NS form gains
 *                                R(w; v) += - int_Gamma t.v ds - int_Gamma beta_k (u.n)_- u.v ds,   (u.n)_- = min(u.n, 0).
 *                            t_dev: 9*n_facets doubles [facet][vertex][component] in the vertex order of facets_host, P1 on each
 *                            facet (it may jump between facets), integrated exactly by the facet mass matrix |Gamma|/12 (1 +
 *                            delta_ab).  Under the reference's viscous term nu (grad u, grad v) t is the PSEUDO-traction
 *                            nu d_n u - p n; under the stress-divergence form (a Carreau law or a viscosity field) it is the TRUE
 *                            traction 2 nu eps(u) n - p n.  A pressure boundary is t = -p0 n.  beta_dev: n_facets doubles, each
 *                            finite and >= 0, 0 switches the backflow term off on that facet; the term is taken with the 6-point
 *                            degree-4 rule with positive weights (a1 = 0.445948490915965, w1 = 0.223381589678011, a2 =
 *                            0.091576213509771, w2 = 0.109951743655322).  The Jacobian gains the exact derivative of the branch
 *                            each quadrature point takes, -beta [(u.n)_- du.v + H(-u.n)(du.n) u.v], in the 3 x 3 velocity part
 *                            of the facet's blocks; t and beta are held fixed.  The pressure rows get nothing.  NULL clears a term.
 *   sns_set_boundary_scalar  the form of sns_scalar_system gains R_k(c; v) += int_Gamma (alpha_k c_k - g_k) v ds, i.e.
 *                            kappa d_n c = alpha (c_ext - c) + q with g = alpha c_ext + q.  alpha_dev: 4*n_facets doubles
 *                            [facet][species], each finite and >= 0; g_dev: 12*n_facets doubles [facet][vertex][species], P1 per
 *                            facet.  Both by the facet mass matrix: alpha M_Gamma on the diagonal entries of the facet's blocks
 *                            (the operator stays block diagonal over the species), int g v into rhs_dev.  NULL clears a term.
 * The data is copied into buffers the handle owns; the calls return after the copy.  The terms are part of the raw form: rows of
 * constrained dofs get nothing, columns of constrained dofs are not stored and their product with the Dirichlet defect goes into
 * the lifting (F += J0[:,B](g - w_B), b -= A0[:,B] g).  From the call on every NS assembly -- sns_residual, sns_jacobian,
 * sns_newton_solve, sns_time_step, sns_adjoint_solve's operator, sns_bench_assemble, fused or staged -- ends with one
 * owner-computes pass over the boundary rows (4 lanes per row, no atomics, no scratch, bitwise reproducible), and
 * sns_residual_moments adds phi . (the boundary residual without the Dirichlet rule).  The Stokes forms ignore both flow terms,
 * as they ignore the time term and the body force.  With nothing set nothing is launched or allocated; clearing gives back the
 * handle as it was, bit for bit.  Another beta or alpha -- set, cleared, or any entry changed -- is another operator: the next
 * preconditioner set-up takes its spectral estimates again; t and g (and the same beta or alpha written again) change none.
 * SNS_E_ARG: a null handle; a 2-D handle; a negative count or a null list; a beta or alpha that is negative or not finite
 * (checked on the device: one reduction launch, one host read).  SNS_E_STATE: a communicator attached; flow or scalar data before
 * facets are set.  SNS_E_MESH: a facet whose nodes are not three of the four nodes of its tet, a facet listed twice, a facet
 * without area.  sns_residual_shape_gradient is refused (SNS_E_STATE) while t or beta is set: the mesh derivative of the facet
 * terms is not built.  After a refusal the handle is untouched.                                                              */
SNS_API int sns_set_boundary_facets(sns_handle h, int32_t n_facets, const int32_t* facets_host, const int64_t* facet_tets_host);
SNS_API int sns_set_boundary_flow(sns_handle h, const double* t_dev /* 9*nf or NULL */, const double* beta_dev /* nf or NULL */);
SNS_API int sns_set_boundary_scalar(sns_handle h, const double* alpha_dev /* 4*nf or NULL */, const double* g_dev /* 12*nf or NULL */);

/* ---- introspection (tests, profiling) --------------------------------------*/
/* device pointers of the assembled BSR4 operator (block row-major 4x4); the values are those of A^T while the handle
 * is transposed (sns_transpose_operator), like SNS_EXPORT_VALS below                                                */
SNS_API int sns_get_bsr(sns_handle h, int32_t* n_rows, int64_t* nnzb, const int32_t** rowptr_dev,
                const int32_t** colind_dev, const double** vals_dev);
/* element-level output of the last sns_jacobian call: Ke [n_tets][a][b][c][d]
 * (16 blocks of 4x4) as produced by the element kernel before the gather.     */
SNS_API int sns_get_element_scratch(sns_handle h, const double** Ke_dev, const double** Fe_dev);
/* copy an internal device array into a caller-owned device buffer of nbytes
 * (exact size required): tests read the assembled operator through this.      */
#define SNS_EXPORT_ROWPTR 0   /* int32 [n_local+1]        */
#define SNS_EXPORT_COLIND 1   /* int32 [nnzb]             */
#define SNS_EXPORT_VALS   2   /* double [nnzb*16]         */
#define SNS_EXPORT_KE     3   /* double [n_tets*256]      */
#define SNS_EXPORT_FE     4   /* double [n_tets*16]       */
#define SNS_EXPORT_STRENGTH 5 /* float [nnzb]: the strength || D_i^-1/2 A_ij D_j^-1/2 ||_F of every block slot of the CURRENT fine
                                 operator (owned rows; 0 on the diagonal slot and on ghost rows), computed into dst by the
                                 strength kernel -- what amg_aggregation = 1 aggregates by.  Collective on a partitioned handle */
#define SNS_EXPORT_AGG0   6   /* int32 [n_local]: the level-0 aggregate map as built (-1: node takes no part; ghost nodes -1) */
SNS_API int sns_export(sns_handle h, int what, void* dst_dev, int64_t nbytes);
/* timing of the phases of the last solve, milliseconds (HIP events)           */
typedef struct {
    double assemble_ms, pc_setup_ms, krylov_ms, spmv_ms_avg;
    int64_t spmv_calls; int ksp_its; int amg_levels;
} sns_timings;
SNS_API int sns_get_timings(sns_handle h, sns_timings* t);
/* debug counters of the LAST Krylov solve: out[0] = host<->device synchronisations (stream / event waits),
 * out[1] = all-reduces, out[2] = neighbour (halo) exchanges; out[3] = Krylov iterations since reset_timings,
 * out[4] = damping retries since reset_timings, out[5] = current damping factor x 1e6 (1000000 = no retry so far),
 * out[6] = reason of the first attempt of the last solve if it was retried (else 0), out[7] = blocks of the fine level's
 * M = A P (fused post-smoothing sweep; 0 until the hierarchy exists) */
SNS_API int sns_get_counters(sns_handle h, int64_t out[8]);
/* communicator of the handle: out[0] = transport (0 none, 1 RCCL, 2 in-process team, 3 peer windows), out[1] = this rank,
 * out[2] = ranks the handle was attached with, out[3] = ranks RCCL itself reports (ncclCommCount; 0 without RCCL):
 * bench.py prints it so that "did RCCL see N ranks" can be read off the result line */
SNS_API int sns_comm_info(sns_handle h, int32_t out[4]);
/* the AMG hierarchy as built (what PETSc's -ksp_view prints of a PCGAMG/PCMG): *nlevels levels (at most 16 reported; a
 * partitioned handle counts its replicated tail copy), per level the rows this rank solves for, the 4x4 blocks of its
 * operator, the sweeps per half cycle level_nu gives it (after amg_nu_scale_with_size) and the block-Jacobi damping in use */
SNS_API int sns_get_hierarchy(sns_handle h, int32_t* nlevels, int64_t rows[16], int64_t blocks[16], int32_t sweeps[16], double omega[16]);
/* the dense coarsest-level solver on its own (tests): Ainv_dev <- inverse of the N x N row-major fp64 matrix A_dev by the blocked
 * Gauss-Jordan elimination of csrc/sns_dense.hip (64 x 64 blocks, v_mfma_f64_16x16x4_f64 rank-64 updates, NO pivoting: meant for
 * matrices whose symmetric part is positive definite, like the level operators).  SNS_E_STATE on a zero / non-finite pivot. */
SNS_API int sns_dense_inverse(int device, int32_t N, const double* A_dev, double* Ainv_dev);
/* the V-cycle as run: per level the smoother / solver kind and the sweeps before and after the coarse-grid correction (the
 * first pre-sweep starts from the zero guess).  Tests restate the cycle from this (oracle/amg_cycle.py).                    */
#define SNS_LEVEL_NODAL_BLOCKS      0   /* damped Jacobi with the 4 x 4 nodal blocks                                         */
#define SNS_LEVEL_AGGREGATE_BLOCKS  1   /* damped Jacobi with the aggregates' dense blocks (amg_block_smooth)                */
#define SNS_LEVEL_DIRECT            2   /* coarsest level: dense inverse by the one-workgroup Gauss-Jordan with pivoting     */
#define SNS_LEVEL_DIRECT_BLOCKED    3   /* coarsest level: dense inverse by the blocked Gauss-Jordan of csrc/sns_dense.hip   */
#define SNS_LEVEL_SWEEPS_ONLY       4   /* coarsest level too large for a direct solve: 1 + 8 nodal-block sweeps              */
SNS_API int sns_get_cycle(sns_handle h, int32_t* nlevels, int32_t kind[16], int32_t nu_pre[16], int32_t nu_post[16]);
SNS_API int sns_reset_timings(sns_handle h);
/* per-launch HIP-event timing of the level-0 k_spmv family inside solves
 * (index = mode: 0 y=Ax, 1 r=b-Ax, 2 Jacobi sweep, 3 y=Ax with fused dot,
 *  4 fused correction + post-sweep on M = A P; 5..7 reserved)                  */
SNS_API int sns_time_kernels(sns_handle h, int on);
SNS_API int sns_get_kernel_times(sns_handle h, double ms_total[8], int64_t calls[8]);
/* raw kernel launchers for micro-benchmarks (bench.py roofline leg): run the
 * kernel `reps` times between two HIP events on the handle's stream and return
 * the average duration in ms.                                                  */
SNS_API int sns_bench_spmv(sns_handle h, const double* x_dev, double* y_dev, int reps, double* ms_avg);
SNS_API int sns_bench_assemble(sns_handle h, int form, const double* w_dev, double* F_dev, int reps, double* ms_avg);
/* one collective of the attached communicator, `reps` times back to back (COLLECTIVE: every rank calls it with the same arguments):
 * which 0 = halo exchange of the assembled operator's plan, 1 = all-reduce of `count` (1..32) doubles, 2 = all-gather of `count`
 * doubles per rank.  Any transport.                                                                                          */
SNS_API int sns_bench_collective(sns_handle h, int which, int count, int reps, double* ms_avg);
/* ---- batched particle tracing (next row after the solve path; replaces the per-seed
 *      solve_ivp(RK45) of NavierStokes/streamtrace.py:208-232, :357-383) ---------------
 * One lane per seed: scipy's RK45 (same tableau, controller and initial step; rtol/atol as
 * given, the reference uses solve_ivp's defaults 1e-3 / 1e-6 and max_step 0.125, t in [0,20]).
 * Velocity = P1 interpolation of vel_dev (n_nodes x 3) in the containing tet, zero outside
 * (velfunc :144-158); reverse != 0 negates it (:160-173).  Terminal events: speed falling
 * below speed_min (1e-6, :175-178) -> status 1; x crossing x_stop upward (forward, 3.7 :180-183)
 * or downward (reverse, 0.13 :185-188) -> status 2; t_end reached -> 0; step underflow -> 3.
 * nbr_dev[4t+a] = tet across the face opposite local vertex a of tet t, -1 on the boundary;
 * seed_tet_dev = a tet containing (or near) each seed.  All pointers are device memory.   */
SNS_API int sns_streamtrace(int32_t n_nodes, int64_t n_tets, const double* pts_dev, const int32_t* tets_dev,
                    const int32_t* nbr_dev, const double* vel_dev, int32_t n_seeds,
                    const double* seeds_dev, const int32_t* seed_tet_dev, int reverse, double t_end,
                    double max_step, double rtol, double atol, double x_stop, double speed_min,
                    double* pos_out_dev, double* t_out_dev, int32_t* status_out_dev,
                    int32_t* steps_out_dev, void* hip_stream);
/* ---- point location and P1 evaluation at arbitrary points (row a9: interpolate.locate_points on the
 *      device; what interpolate_nonmatching and Function.eval with a bb_tree do for the reference,
 *      NavierStokesChannelFlow.py:175-194, streamtrace.py) ------------------------------------------
 * No handle.  All arrays are device memory; n_missed_out is a HOST pointer (may be NULL).  Both calls
 * return after their work on hip_stream has finished.
 * sns_locate_points: for each of the n_query points query_dev (n_query x 3) the tet tet_out_dev[q]
 * and its barycentric coordinates lam_out_dev (n_query x 4, clipped to [0,1] and divided by their
 * sum) by the rule of interpolate.locate_points: a uniform bucket grid over the tets' bounding boxes
 * (the host's lo / res / h); the FIRST candidate of the point's bucket (ascending tet id) whose
 * smallest coordinate is >= -padding, else the candidate with the largest smallest coordinate (the
 * first on ties); a point without a candidate takes the tet of the nearest centroid over all tets
 * (lowest index on ties) and counts in *n_missed_out.  Deterministic: repeated calls give the same
 * bits.  Temporary device memory, allocated and freed inside the call: 8 B per (tet, bucket) pair,
 * i.e. 8 n_tets x buckets per tet (8 on a Delaunay mesh, 24 on a structured duct whose nodes lie on
 * bucket faces: 200 MB at 1 M tets), 12 B per bucket (about n_tets / 6 buckets), 4 B per query
 * point, and 24 B per tet when some point misses.
 * SNS_E_ARG: negative sizes, n_tets or n_query >= 2^31, padding < 0 or NaN; SNS_E_MESH: no tets, a
 * node id outside [0, n_nodes), non-finite coordinates.  n_query == 0: no-op, SNS_OK.             */
SNS_API int sns_locate_points(int32_t n_nodes, int64_t n_tets, const double* pts_dev, const int32_t* tets_dev,
                      int64_t n_query, const double* query_dev, double padding,
                      int32_t* tet_out_dev, double* lam_out_dev, int64_t* n_missed_out, void* hip_stream);
/* out[q*ncomp+c] = sum_a lam[q,a] * vals[tets[tet[q],a]*ncomp+c], 1 <= ncomp <= 4 (vals: n_nodes x
 * ncomp, e.g. the nodal [ux,uy,uz,p] of a solution with ncomp = 4); a tet id outside [0, n_tets)
 * gives NaN.  SNS_E_ARG for ncomp outside 1..4 or negative sizes, SNS_E_MESH for n_tets == 0;
 * n_query == 0: no-op, SNS_OK.                                                                     */
SNS_API int sns_eval_p1(int64_t n_tets, const int32_t* tets_dev, int32_t ncomp, const double* vals_dev,
                int64_t n_query, const int32_t* tet_dev, const double* lam_dev, double* out_dev, void* hip_stream);

/* ---- host-only symbolic utilities (no GPU needed; used by sns_create and by
 *      the CPU test-suite) ------------------------------------------------------
 * BSR sparsity pattern of the P1-P1 operator (what create_matrix derives from
 * the dofmap, :272) and the slot -> element-block gather lists of the
 * atomic-free assembly.  Call with NULL outputs to query sizes.               */
SNS_API int sns_host_pattern(int32_t n_nodes, int64_t n_tets, const int32_t* tets_host,
                     int64_t* nnzb_out,
                     int32_t* rowptr_out /*n_nodes+1*/, int32_t* colind_out /*nnzb*/,
                     int64_t* c_ptr_out /*nnzb+1*/, int32_t* c_idx_out /*16*n_tets*/);
/* The lists of the boundary pass (sns_set_boundary_facets builds the same): from n_facets boundary facets (3 node ids each, any
 * winding) and the tet that owns each, facets_out = the facets rewound so that (x1 - x0) x (x2 - x0) points away from the
 * owner's fourth vertex (vertex 0 stays, vertices 1 and 2 change places where needed); rows_out = the boundary rows, i.e. the
 * nodes of listed facets, ascending (at most min(n_nodes, 3*n_facets); their number in n_rows_out); row_ptr_out / row_fv_out =
 * per boundary row its entries facet * 4 + local vertex (of the rewound facet) in ascending facet order.  Outputs may be NULL.
 * SNS_E_MESH, with nothing written: a facet's nodes are not three of the four nodes of its tet, a facet is listed twice, a facet
 * is degenerate (zero area).                                                                                                  */
SNS_API int sns_host_facet_lists(int32_t n_nodes, int64_t n_tets, const int32_t* tets_host, const double* pts_host /*3*n_nodes*/,
                     int32_t n_facets, const int32_t* facets_host /*3*n_facets*/, const int64_t* facet_tets_host /*n_facets*/,
                     int32_t* facets_out /*3*n_facets*/, int32_t* n_rows_out, int32_t* rows_out, int32_t* row_ptr_out /*rows+1*/,
                     int32_t* row_fv_out /*3*n_facets*/);
/* size-limited greedy aggregation of the first n_active nodes of a pattern;
 * agg_out[n_nodes] gets the aggregate id (-1 for inactive nodes).             */
SNS_API int sns_host_aggregate(int32_t n_nodes, const int32_t* rowptr, const int32_t* colind,
                       int32_t n_active, int max_agg, int32_t* agg_out, int32_t* n_agg_out);
/* (round 5) ... with the nodes' coordinates pts[3 * n_nodes], as the hierarchy build runs it on a 3-D level: the greedy sweep
 * (on an anisotropic cloud along the short edges only), and -- unless its aggregates are as compact as cubes already -- a pairwise
 * aggregation (nodes -> pairs -> quadruples -> octets by closest centroids), which does not depend on how the node numbers run
 * through the mesh; the more compact of the two is returned.  *which_out: 0 = greedy sweep, 1 = pairwise.  pts = NULL: the
 * greedy sweep, = sns_host_aggregate.                                          */
SNS_API int sns_host_aggregate_pts(int32_t n_nodes, const int32_t* rowptr, const int32_t* colind, int32_t n_active, int max_agg,
                           const double* pts, int32_t* agg_out, int32_t* n_agg_out, int32_t* which_out);

/* (amg_aggregation = 1; 2 builds the same map on the device) aggregation of the first n_active nodes by operator strength: strength[nnzb] = one value per block slot
 * (what SNS_EXPORT_STRENGTH returns: || D_i^-1/2 A_ij D_j^-1/2 ||_F in the point-diagonally balanced basis), symmetrised by the
 * larger of s_ij and s_ji; pairwise heavy-edge matching of the strong graph, nodes -> pairs -> quadruples -> octets.  At most
 * max_agg (1..8) members per aggregate, every aggregate connected in the strong graph; agg_out[n_nodes] gets the aggregate id
 * (-1 for inactive nodes).  What the hierarchy build runs on level 0 (sns_export SNS_EXPORT_AGG0).                       */
SNS_API int sns_host_aggregate_strength(int32_t n_nodes, const int32_t* rowptr, const int32_t* colind, int32_t n_active,
                                        int max_agg, const float* strength, int32_t* agg_out, int32_t* n_agg_out);

/* owned rows (i < n_owned) of a local pattern that reference a ghost column (>= n_owned): the boundary rows of the
 * interior / boundary split of the multi-GPU SpMV -- interior rows are computed while the halo is in flight
 * (MatMult's VecScatter overlap in the reference's PETSc).  rows_out [n_owned], *n_out entries are valid.        */
SNS_API int sns_host_boundary_rows(int32_t n_owned, const int32_t* rowptr, const int32_t* colind,
                           int32_t* rows_out, int32_t* n_out);

/* The policy table of the AMG hierarchy on its own (csrc/sns_policy.h: the ONE place that holds its size thresholds and sweep
 * schedules): for a hierarchy of `nlevels` levels with rows_global[l] rows (a replicated level: its rows) on `nranks` ranks --
 * rep_level = first level held redundantly by every rank (0: none; the level before it is only the source of the copy and gets
 * kind -1), windows != 0: a window transport (peer / team), rows_global_l1 = rows of level 1 as coarsened (decides the
 * unstructured tier of amg_nu_scale_with_size), has_blocks[l] (NULL: all 1) = the level's aggregates fit the 32 x 32 smoother
 * blocks -- the smoother / solver kind (SNS_LEVEL_*), the sweeps before and after the coarse-grid correction and whether the
 * level's sweeps are the exact global ones (amg_exact_sweeps).  What sns_get_cycle reports of a handle of that shape.            */
SNS_API int sns_host_cycle_policy(const sns_options* opt, int nranks, int windows, int nlevels, const int64_t* rows_global,
                                  int rep_level, int64_t rows_global_l1, const uint8_t* has_blocks, int32_t* kind,
                                  int32_t* nu_pre, int32_t* nu_post, int32_t* exact);

/* eigenvalues of a small real upper-Hessenberg matrix (row-major n x n, n <= 32; entries below the first subdiagonal ignored):
 * the Ritz values of the short Arnoldi process that caps the smoother damping (amg_ritz_limit).                          */
SNS_API int sns_host_hessenberg_eigs(int n, const double* H, double* re_out, double* im_out);

#ifdef __cplusplus
}
#endif
#endif /* SNS_H */
