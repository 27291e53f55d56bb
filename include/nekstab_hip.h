/* libnekstab_hip.so -- C-ABI of the MI355X-native Arnoldi hot path for nekStab.
 *
 * The reference (nekStab, Fortran on Nek5000) has no FFI layer; its seam is the
 * Fortran call interface  `matvec(f,q)`  ("all subroutines need to have the
 * same interface", core/matvec.f:64-68)  plus the `krylov_*` vector algebra
 * (core/krylov_subspace.f:24-258).  Every entry point below names the
 * reference routine it replaces.  Plain pointers and sizes only; vectors are
 * opaque device-resident handles so the Krylov basis never leaves HBM.
 *
 * Conventions: every function returns 0 on success, a negative nsk_status
 * otherwise (the reference aborts through nek_end/exitt instead);
 * one context per process; calls are serialised by the caller.
 * Host arrays are Nek element-major:  index = i + lx1*(j + lx1*e).
 */
#ifndef NEKSTAB_HIP_H
#define NEKSTAB_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nsk_ctx nsk_ctx;
typedef void* nsk_vec;               /* device state vector [vx | vy | pr]  (3-D: [vx | vy | vz | pr]) */

enum nsk_status {
  NSK_OK = 0,
  NSK_EINVAL = -1,      /* bad argument / unsupported lx1 */
  NSK_EHIP = -2,        /* HIP runtime error */
  NSK_ENAN = -3,        /* NaN in an inner product (core/krylov_subspace.f:53 aborts) */
  NSK_ENOCONV = -4,     /* an inner Helmholtz / pressure solve hit its iteration cap */
  NSK_ENOMEM = -5,
  NSK_ECOMM = -6        /* the ranks of a sharded run received DIFFERENT results from one all-reduce (checked bit for bit on the first
                           all-reduces of a context): device-side convergence flags would diverge; the map is refused */
};

enum nsk_mode {          /* `evop`, core/matvec.f:124-151 */
  NSK_DIRECT = 0,        /* 'd'  forward_linearized_map   core/matvec.f:163-243 */
  NSK_ADJOINT = 1,       /* 'a'  adjoint_linearized_map   core/matvec.f:249-326 */
  NSK_DIRECT_ADJOINT = 2,/* 'p'  transient_growth_map     core/matvec.f:332-349 */
  NSK_NEWTON = 3,        /* 'n'  newton_linearized_map    core/matvec.f:381-428 (exp(LT)-I) */
  NSK_FORCE_SENSITIVITY = 4 /*  ts_force_sensitivity_map   core/matvec.f:357-374 (uparam(1) = 4: (I - exp(L^+ T)) q, adjoint map) */
};

/* Case description = what Nek5000 holds in COMMON when nekStab_init runs
 * (core/usr_extra.f:72-132): geometry, numbering, masks, base flow, sponge. */
typedef struct {
  int ndim;                 /* 2: quadrilaterals; 3: hexahedra (arrays [nel*lx1^3], z / wb / 8 vertices per element) */
  int nel;                  /* elements on this rank */
  int lx1;                  /* GLL points per direction: 6, 8, 10 or 12 (SIZE:13) */
  int lxd;                  /* dealiasing points, 3*lx1/2 (SIZE:14) */
  long long nglob;          /* number of distinct global GLL nodes */
  const double* x;          /* [nel*lx1*lx1] GLL coordinates (xm1) */
  const double* y;
  const long long* gid;     /* [nel*lx1*lx1] 0-based global node id (gslib numbering) */
  const double* mask;       /* [nel*lx1*lx1] velocity Dirichlet mask v1mask (1 free / 0 fixed) */
  const double* ub;         /* [nel*lx1*lx1] base flow ubase (core/NEKSTAB:26) */
  const double* vb;
  const double* spng;       /* [nel*lx1*lx1] spng_fun (core/utils.f:283-318) */
  const long long* vert;    /* [nel*4] 0-based vertex ids, lexicographic corners (.ma2) */
  long long nvert;
  double re;                /* Reynolds number; viscosity = 1/re (1cyl.par:37) */
  double endtime;           /* sampling period T = param(10) */
  double cfl;               /* target CFL = param(26) (0.5) */
  int has_outflow;          /* 0: all-Dirichlet/periodic => pressure null space (`ortho`) */
  double tol_helm;          /* [VELOCITY] residualTol, Nek norm (1cyl.par:34) */
  double tol_pres;          /* [PRESSURE] residualTol, Nek norm (1cyl.par:29) */
  int tol_relative;         /* 0: absolute tolerances as Nek (param(21/22)>0); 1: relative to the initial residual */
  int schwarz_layers;       /* overlap (GL-node layers) of the pressure Schwarz patches */
  int max_helm_iter;        /* iteration caps per solve */
  int max_pres_iter;
  int nproj;                /* pressure projection space (residualProj; mxprev, SIZE:33); 0 = off */
  const double* z;          /* ndim = 3: zm1 */
  const double* wb;         /* ndim = 3: third base-flow component (wbase, core/NEKSTAB:26) */
} nsk_case;

/* nekStab_init + prepare_linearized_solver (core/usr_extra.f:72-132, core/matvec.f:1-52):
 * uploads the case, builds operators/preconditioners, derives dt and nsteps. */
int nsk_init(const nsk_case* c, nsk_ctx** out);
/* The same with one Dirichlet mask per velocity component: symmetry boundaries.  On a face whose normal is a coordinate axis
 * 'SYM' fixes the normal component only, 'ON ' the tangential one only, 'v' / 'V' / 'W' all; a node takes the minimum over its
 * copies, per component; the free components get the natural (zero-stress) condition of the weak form
 * [UPSTREAM bcmask, non-stress branch: v1mask, v2mask, v3mask].  cmask[k], k < ndim: [nel*lx1^ndim], 1 free / 0 fixed (ndim = 3:
 * no other value, NSK_EINVAL); c->mask is not read.  Every masked operation then takes its component's mask: Helmholtz residual
 * and Jacobi diagonal, opbinv inside E = D B^-1 D^T (and with it the Schwarz patches -- the face ratio of the component along the
 * face normal --, the coarse operator and its image, all built from E), the velocity correction, bcdirvc in nsk_seed_noise
 * (core/utils.f:398).  cmask == NULL: nsk_init.  Equal components: the context nsk_init makes of that mask, bit for bit.
 * Quadrilaterals (lx1 = 6, 8, 10, 12) on one rank and their nsk_clone lanes; hexahedra (lx1 = 6, 8, 10) on one rank.  NSK_EINVAL on such
 * a context: nsk_shard_create / nsk_shard_create_local, the options "fused" and "helm_fdm", on hexahedra also "eapply_pipe" = 3
 * (k_divgs_w), and the kernel hooks
 * nsk_bench_kernel, nsk_debug_stamps, nsk_test_helm_solve.  A symmetry face that is not axis-aligned needs
 * the stress formulation, which is not built: the caller refuses it (nekstab_amd/mesh.py and mesh3d.py do). */
int nsk_init_masks(const nsk_case* c, const double* const* cmask, nsk_ctx** out);
int nsk_finalize(nsk_ctx* ctx);
const char* nsk_last_error(void);

/* dt, nsteps (core/matvec.f:30-34), state length S = 2*P + P2, P, P2 */
int nsk_get_info(nsk_ctx* ctx, double* dt, int* nsteps, long long* nstate,
                 long long* nvel, long long* npres);
int nsk_set_nsteps(nsk_ctx* ctx, int nsteps);   /* test hook: shorten the map (dt unchanged) */
int nsk_set_tolerances(nsk_ctx* ctx, double tol_helm, double tol_pres, int relative);
/* run-time switches: "use_graph" (hipGraph replay of the step classes, default 1), "min_pres_iter" (at least this many
 * GMRES iterations per pressure solve, default 0), "pres_cap" (at most this many in time steps >= 4, default 0 = none),
 * "helm_guess" (extrapolated Helmholtz initial guess, default 1), "early_pres_mul" (pressure tolerance factor of
 * time steps 1-3 of every map, default 0.01: they project out the divergence of the input vector),
 * "proj_reset" (1: every map starts with an empty pressure projection space: default on hexahedra; 0: the space carries over: default on quadrilaterals),
 * "pres_floor" (absolute floor under the relative pressure tolerance, in the scaled units of nsk_stats.last_pres_res; 0 = off),
 * "budget_helm" / "budget_pres" (launch budgets), "fused" (persistent velocity solve: right-hand side, all CG iterations and
 * the pressure right-hand side in one launch with device-side grid barriers; default 0: not faster on config 2),
 * "endtime" (the sampling period T = param(10); used by the next nsk_set_baseflow / nsk_set_orbit),
 * "orbit_phase" (Fourier orbits, nsk_set_orbit_fourier / nsk_set_orbit_modes: 0 <= phi < 1, default 0 -- maps start at
 * t0 = phi T of the cycle (intracycle growth, core/matvec.f:193,292); ignored while no Fourier orbit is active, takes effect at
 * the next map),
 * "gmres_cycle" (the pressure GMRES restarts after this many iterations, default and maximum 48; `max_pres_iter` may be up to 4 x 48),
 * "mfma_convect" (hexahedra, lx1 = 8: convection contractions on v_mfma_f64_16x16x4_f64, default 1),
 * "merged_update" / "merged_iters" (quadrilaterals with the dense in-LDS coarse solve: the GMRES column bookkeeping runs inside
 * the coarse-solve kernel for the first `merged_iters` iterations of a solve, default 1 / 24; same iteration counts and results to
 * rounding as the classic four-kernel iteration), "shard_graph" / "shard_hostcheck" / "halo_overlap" (shard contexts, see
 * nsk_shard_release_parent and nsk_shard_elems below), "hostcheck" (full-mesh contexts: eager time steps in which the host reads
 * the device's convergence flags and stops issuing solver iterations -- no launch budgets, no redone maps; -1 = default: yes on
 * hexahedral meshes of >= 8192 elements, where a launch that only finds its solve converged costs 25-140 us; 0 / 1; bit-identical),
 * "proj_restart" (1, default: a full projection space restarts on the latest total solution -- Fischer's / Nek5000's rule; 0: the
 * rounds-1-2 policy of merging into the oldest slot, kept for A/B runs), "gs2_from" (quadrilaterals: GMRES columns from this
 * iteration of a cycle on get a second Gram-Schmidt pass, default 48 = never; hexahedra always), "orth_overlap" (RCCL ranks: nsk_orth
 * all-reduces its coefficients in chunks on a second stream while the next chunk's dots are computed, default 1),
 * "gs_lag" (hexahedra: lagged second Gram-Schmidt correction of the pressure GMRES, two basis reads per column instead of four;
 * -1 = default: on for single-rank contexts; 0 / 1 / 2), "flat_proj" (hexahedra: once-per-step sums over the bases as streaming
 * kernels; -1 = default: on for single-rank contexts), "eapply_pipe" (hexahedra, form of the Schwarz + D^T kernel: 0 = one
 * workgroup per element, 1 = resident workgroups, 2 = one wavefront per element, 3 = 2 + the divergence kernel in that form,
 * 4 = default: one wavefront per element, sixteen per CU, at lx1 <= 8 and form 5 at lx1 = 10; 5 = four wavefronts per element,
 * lx1 = 10 only; same results to rounding: DESIGN.md section 4.3, 4.36),
 * "divgs_c3" (hexahedra: divergence kernel with its components side by side; -1 = default: at lx1 = 10, where it runs two
 * workgroups per CU and the plain form one; 0 / 1), "helm_pf" (hexahedra, lx1 = 10: the CG iteration as resident workgroups with
 * the next element's vectors arriving in LDS by LDS-DMA, default 1; bit-identical to 0), "helm_pf_grid" (its resident workgroups;
 * default: what the device holds), "mfma_convect" (hexahedra, lx1 = 8 and 10: convection kernel on the matrix cores, default 1),
 * "helm_fdm" (hexahedra:
 * element-block fast-diagonalisation preconditioner of the velocity solves, default 0: measured slower), "graph_steps" (time steps
 * per captured graph of the last step class, default 1),
 * "budget_freeze" / "budget_add_helm" / "budget_add_pres" (measurement switches of scripts/noop_cost.py),
 * "dbg_max_order" / "dbg_ab2" / "dbg_pext" (time-scheme sensitivity switches of scripts/wake_bisect.py; defaults = SURVEY App. A),
 * "dbg" (developer ablation mask),
 * "step_budgets" (1, default: launch budgets per TIME STEP from the per-step iteration record of the last maps instead of one
 *   per step class; graph-replayed single-rank contexts), "tail" (persistent tail kernels of the two inner solves behind the launches
 *   of a solve: -1 (DEFAULT) = as a safety net behind the per-time-step budgets (mode 2) wherever every workgroup of the grid is
 *   resident, else none; 0 = never; 1 = heads (median counts) + tail; 2 = budgets + safety net; with "tail_off_h" / "tail_off_p"
 *   = offsets of the heads from the median count), "rccl_fuse" (1, default: on RCCL ranks the all-reduce of an iteration rides
 *   in the group of that iteration's halo messages), "allred_verify" (24, default: that many all-reduces of a sharded context
 *   are verified bit for bit across the ranks; a mismatch makes the map return NSK_ECOMM),
 * "fuse2" (1, default; round 6: the merged pressure GMRES iteration in TWO launches -- k_schwarz_uc: Schwarz workgroups and
 *   coarse-solve workgroups side by side, k_divgs_t: the coarse part through its precomputed image under E; 0 = the three
 *   launches of rounds 3-5), "fuse2_start" (1: the solve starts inside the first of them, no k_gmres_update(-1) launch),
 *   "tc32" (0, default; 1: fp32 copy of the coarse image, moves a map by 2e-8; -1: where the relative tolerance is >= 1e-5),
 * "zero_metrics" (hexahedra; 1, default: arrays of the mapping and of the base-flow constants that are zero on every node -- the
 *   cross terms Nek5000 skips on its undeformed elements, hmholtz.f axhelm / ifdfrm -- are not loaded; 0: every array is loaded,
 *   same bits.  The set-up sets derivatives of the mapping that are rounding noise on every node to zero; NSK_ZERO_METRICS=0 in
 *   the environment of nsk_init keeps the noise, as rounds 1-4 did) */
int nsk_set_option(nsk_ctx* ctx, const char* name, double value);

/* allocate(Q(k_dim+1)) (core/eigensolvers.f:170) */
int nsk_vec_alloc(nsk_ctx* ctx, int n, nsk_vec* out);
int nsk_vec_free(nsk_ctx* ctx, int n, nsk_vec* v);
/* nopcopy / outpost / load_files (core/utils.f:471-550, core/IO.f:15-60) */
int nsk_vec_upload(nsk_ctx* ctx, nsk_vec v, const double* vx, const double* vy, const double* pr);
int nsk_vec_download(nsk_ctx* ctx, nsk_vec v, double* vx, double* vy, double* pr);
/* krylov_vector%theta(:, m) (core/krylov_subspace.f:13): after nsk_set_option(ctx, "nscal", ldimt) -- set it before the first
 * nsk_vec_alloc -- every vector carries `nscal` scalar fields of P entries behind the pressure; the inner product adds their
 * bm1s-weighted products (:46-50), the vector operations scale / add / rotate them, and the time steppers pass them through
 * unchanged, as the reference does when ifheat = .false. (no case in scope solves a scalar equation) */
int nsk_vec_upload_scalar(nsk_ctx* ctx, nsk_vec v, int m, const double* theta);
int nsk_vec_download_scalar(nsk_ctx* ctx, nsk_vec v, int m, double* theta);
/* hexahedral contexts (krylov_vector carries vz, core/krylov_subspace.f:9-11) */
int nsk_vec_upload3(nsk_ctx* ctx, nsk_vec v, const double* vx, const double* vy, const double* vz, const double* pr);
int nsk_vec_download3(nsk_ctx* ctx, nsk_vec v, double* vx, double* vy, double* vz, double* pr);

/* matvec(f,q) (core/matvec.f:64-154) */
int nsk_matvec(nsk_ctx* ctx, int mode, nsk_vec f, nsk_vec q);

/* Newton-Krylov support (core/newton_krylov.f): the full nonlinear map Phi_T(q) [optionally minus q] and
 * the change of linearisation point (base flow := q, new dt / nsteps from the CFL rule). */
int nsk_nonlinear_map(nsk_ctx* ctx, nsk_vec f, nsk_vec q, int subtract_q);
int nsk_set_baseflow(nsk_ctx* ctx, nsk_vec q);
/* Floquet (uparam(1)=3.11): time-periodic base flow over one period T = endtime, stored per step on the
 * device (quadrilaterals: six arrays per step; hexahedra: the twelve dealiasing-mesh constants per step, 12 * nel * lxd^3 doubles);
 * `end` (optional) receives Phi_T(q0) for a periodicity check. */
int nsk_set_orbit(nsk_ctx* ctx, nsk_vec q0, double spng_str, nsk_vec end);
/* The same orbit as its temporal Fourier modes (core/fourier.f):
 *   U(t_n) = A_0 + sum_{k=1..M} A_k cos(2 pi k n / N) + B_k sin(2 pi k n / N),  n = 0 .. N-1 = nsteps - 1.
 * Device memory: stored orbit nsteps * (quadrilaterals 6 * nel * lxd^2, hexahedra 12 * nel * lxd^3) doubles;
 * Fourier orbit (2 M + 1) * ndim * nel * lx1^ndim doubles whatever the number of steps (+ nsteps * 2 M cos / sin factors).
 * The linearised maps rebuild the base-flow constants of the running step from the modes; a map may then be longer than one
 * period (nsk_set_nsteps), use another dt, or start at another phase (option "orbit_phase").  These three entries take full-mesh
 * contexts: shards (use nsk_group_set_orbit_fourier / _set_orbit_modes / _get_orbit_modes below), rank-local contexts and lanes
 * return NSK_EINVAL.  nsk_set_baseflow / nsk_set_orbit end the Fourier form; nsk_clone refuses it.
 *
 * nsk_set_orbit_fourier (fourier_decomposition, core/fourier.f:23-88): the integration of nsk_set_orbit (same dt / nsteps,
 * sponge and `end`, bit for bit), keeping the lowest `nmodes` harmonics, 0 <= nmodes <= nsteps / 2 (0: the time average);
 * no snapshot is stored at any point.  `amp` (NULL or 2 nmodes + 1 doubles) receives the bm1-weighted L2 norms of
 * A_0, A_1, B_1, .. over all velocity components (amp_real / amp_img, core/fourier.f:46-53). */
int nsk_set_orbit_fourier(nsk_ctx* ctx, nsk_vec q0, double spng_str, int nmodes, nsk_vec end, double* amp);
/* fourier_reconstruction (core/fourier.f:2-21) from modes computed elsewhere: A[0 .. nmodes], B[0 .. nmodes-1] = B_1 ..
 * are state vectors (velocity components used, pressure ignored).  dt / nsteps follow the rule of nsk_set_baseflow applied
 * to U(0) = sum_k A_k with "endtime" as set; `period` is the orbit's T and need not equal endtime. */
int nsk_set_orbit_modes(nsk_ctx* ctx, int nmodes, double period, const nsk_vec* A, const nsk_vec* B);
/* the modes of the active Fourier orbit (the fRe / fIm fields of core/fourier.f:78-85, un-normalised) into A[0 .. nmodes],
 * B[0 .. nmodes-1]; A = B = NULL: count and period only.  NSK_EINVAL when no Fourier orbit is active. */
int nsk_get_orbit_modes(nsk_ctx* ctx, int* nmodes, double* period, nsk_vec* A, nsk_vec* B);

/* krylov_inner_product / norm / cmult / add2,sub2 / copy / zero
 * (core/krylov_subspace.f:24-212) */
int nsk_dot(nsk_ctx* ctx, nsk_vec p, nsk_vec q, double* alpha);
int nsk_norm(nsk_ctx* ctx, nsk_vec p, double* alpha);
int nsk_scal(nsk_ctx* ctx, nsk_vec p, double alpha);
int nsk_axpy(nsk_ctx* ctx, nsk_vec p, double alpha, nsk_vec q);   /* p += alpha*q */
int nsk_copy(nsk_ctx* ctx, nsk_vec dst, nsk_vec src);
int nsk_zero(nsk_ctx* ctx, nsk_vec p);

/* update_hessenberg_matrix (core/krylov_decomposition.f:116-202): two
 * projection passes against Q(1:j) + normalisation; h[0..j-1] = H(1:j,j),
 * *beta = H(j+1,j).  f is overwritten with the new unit Krylov vector. */
int nsk_orth(nsk_ctx* ctx, nsk_vec f, const nsk_vec* Q, int j, double* h, double* beta);

/* Q(:,1:k) <- Q(:,1:k) * Z   (schur_condensation, core/eigensolvers.f:455-474) */
int nsk_basis_gemm(nsk_ctx* ctx, nsk_vec* Q, int k, const double* Z, int ldz);
/* krylov_matmul / eigenmode assembly  re + i im = Q (y_re + i y_im)
 * (core/krylov_subspace.f:214-258, core/eigensolvers.f:607-615) */
int nsk_basis_gemv(nsk_ctx* ctx, const nsk_vec* Q, int k, const double* y_re,
                   const double* y_im, nsk_vec re, nsk_vec im);

/* add_noise seed (core/utils.f:344-408): deterministic pseudo-noise, dssum-averaged, masked */
int nsk_seed_noise(nsk_ctx* ctx, nsk_vec v);

/* ---- sensitivity post-processing (core/sensitivity.f; uparam(1) = 4.2, 4.3, 4.41 / 4.42) and the energy budget (4.1) ----
 * Single-rank full-mesh contexts, quadrilaterals and hexahedra; shard and rank-local contexts return NSK_EINVAL here and take
 * the nsk_group_* twins declared behind the sharding entries below (same fields, same files, under the element decomposition of
 * every other entry).  Inner products are the bm1s-weighted velocity products of nsk_dot. */
/* biorthogonalize (core/sensitivity.f:428-504), in place: d <- d / ||d|| (||d||^2 = ||dRe||^2 + ||dIm||^2; the whole vector is
 * scaled), then with <a, d> = gamma + i delta: a <- a / (gamma - i delta), so that <a, d> = 1 afterwards.  gamma_delta (optional)
 * receives {gamma, delta}. */
int nsk_biorthogonalize(nsk_ctx* ctx, nsk_vec dRe, nsk_vec dIm, nsk_vec aRe, nsk_vec aIm, double* gamma_delta);
/* wave_maker (core/sensitivity.f:7-81) on modes already biorthogonalised: |d| |a| pointwise (velocity components), in wm's
 * first component; the other components and the pressure of wm are 0. */
int nsk_wavemaker(nsk_ctx* ctx, nsk_vec dRe, nsk_vec dIm, nsk_vec aRe, nsk_vec aIm, nsk_vec wm);
/* bf_sensitivity (core/sensitivity.f:93-284) on modes already biorthogonalised (Marquet, Sipp & Jacquin 2008):
 *   tr_i = -sum_j (aRe_j d dRe_j/dx_i + aIm_j d dIm_j/dx_i)    ti_i = sum_j (aRe_j d dIm_j/dx_i - aIm_j d dRe_j/dx_i)
 *   pr_i =  sum_j (dRe_j d aRe_i/dx_j + dIm_j d aIm_i/dx_j)    pi_i = sum_j (dRe_j d aIm_i/dx_j - dIm_j d aRe_i/dx_j)
 *   sr = tr + pr, si = ti + pi,
 * with the physical gradients of the GLL mesh averaged over shared nodes (gradm1 + dsavg).  parts: NULL or {tr, ti, pr, pi}.
 * The pressure of every output is 0.  In 3-D the reference's transport term reads d w / d z where the formula has d v / d z
 * (core/sensitivity.f:219, 222, 228, 231): this entry implements the formula; on 2-D and z-invariant fields the two agree. */
int nsk_bf_sensitivity(nsk_ctx* ctx, nsk_vec dRe, nsk_vec dIm, nsk_vec aRe, nsk_vec aIm, nsk_vec sr, nsk_vec si, nsk_vec* parts);
/* f = the linearised map of q under the steady body force `force` (fcx / fcy / fcz of nekStab_forcing, core/utils.f:160-162),
 * mode NSK_DIRECT or NSK_ADJOINT: B force enters every time step where the sponge term does, before the EXT extrapolation.
 * initialize_rhs_ts_steady_force_sensitivity (core/sensitivity.f:380-422) is the adjoint map with q = 0.  The time steps run
 * eagerly (the captured step graphs belong to the unforced maps); force = 0 gives the bits of nsk_matvec. */
int nsk_forced_map(nsk_ctx* ctx, int mode, nsk_vec f, nsk_vec q, nsk_vec force);
/* stability_energy_budget (core/postproc.f:657-872, uparam(1) = 4.1) of the direct mode dRe + i dIm about the base flow ub
 * (velocity of a state vector).  prod: NULL or ndim vectors, vector c holding P[c][1..ndim] in its velocity components;
 * diss: NULL or a vector receiving D in its first component; integrals[10]: bm1-weighted sums (reference order).
 * Pressure and unused components of every output are 0; inputs are not modified.
 *   P[c][j] = -1/2 (uR_c uR_j + uI_c uI_j) dU_c/dx_j    (gradm1 of the base flow, element-local: no dsavg)
 *   D = 1/2 nu sum_j (uR_j Lap uR_j + uI_j Lap uI_j),  Lap a = dsavg(sum_i d/dx_i dsavg(d a/dx_i)),  nu = 1/Re
 * integrals = {P[1][1..3], P[2][1..3], P[3][1..3], D} (2-D: entries of a third component or direction are 0).  The mode enters
 * divided by alpha = sqrt(||dRe||^2 + ||dIm||^2) (nsk_dot's product), so the budget does not depend on the mode's scale: the
 * reference's comment says "normalize to unit-norm" where its code multiplies by alpha (postproc.f:703-707; the two agree when
 * alpha = 1).  A zero mode returns NSK_EINVAL. */
int nsk_energy_budget(nsk_ctx* ctx, nsk_vec ub, nsk_vec dRe, nsk_vec dIm, nsk_vec* prod, nsk_vec diss, double* integrals);
/* comp_vort3 as outpost_ks calls it for the Rv files (core/eigensolvers.f:629-637): w = the vorticity of q's velocity.  The
 * element-local curl (metrics derived from the GLL coordinates) is multiplied by the unassembled mass bm1, summed over
 * co-located nodes and divided by the assembled mass -- a mass-weighted average, not dsavg, and WITHOUT the Dirichlet mask:
 * wall nodes keep their vorticity.  Layout of w: 2-D vx = dv/dx - du/dy, vy = 0; 3-D (vx, vy, vz) = curl; pressure and scalar
 * slots 0.  q is read only; w == q: NSK_EINVAL.  The sums run in a fixed order (no atomics): two calls give the same bits.
 * The assembled unmasked mass (one double per velocity node) is built at a context's first call and kept until nsk_finalize;
 * nothing else is allocated, no captured step graph or launch budget is touched. */
int nsk_vorticity(nsk_ctx* ctx, nsk_vec q, nsk_vec w);
/* vortex_core('lambda2'), ('q') and ('omega') as nekStab_outpost calls them for the vox and omg files (core/usr_extra.f:256-281)
 * on q's velocity.  With g[i][j] = d u_i / d x_j at the GLL nodes, element-local and unaveraged (comp_gije; metrics derived from
 * the element's own coordinates), S = (g + g^T) / 2, O = (g - g^T) / 2, ndim x ndim (2 x 2 on quadrilaterals):
 *   lambda2  the second largest eigenvalue of S S + O O (Jeong & Hussain): the middle of three, the smaller of two; cyclic Jacobi
 *            sweeps, accurate where eigenvalues coincide (a z-invariant divergence-free field: at every node)
 *   Q        compute_q -> compute_secondInv (core/postproc.f:374-403): 3-D the sum of the three principal 2 x 2 minors of g;
 *            2-D (g11 + g22)^2 - 2 g12 g21 - g11^2 - g22^2 = 2 det g, the reference's form: twice the 3-D value of the same
 *            field made z-invariant
 *   Omega    compute_omega_jc (core/postproc.f:31-79): b / (a + b + 1e-5), a = (||S||_F^2)^2, b = (||O||_F^2)^2 (1e-5 unscaled)
 * each then filtered as filter_s0(f, wght, 1, .) does (the reference: wght = 0.5), element by element along the reference
 * directions with F = Phi diag(1, ..., 1, 1 - wght) Phi^-1, Phi[j][k] = phi_k(xi_j), phi_0 = L_0, phi_1 = L_1,
 * phi_k = L_k - L_{k-2}: polynomials of degree <= lx1 - 2 stay, phi_{lx1-1} is multiplied by 1 - wght.  wght = 0: no filter, the
 * criteria bit for bit.  wght outside [0, 1] or not finite: NSK_EINVAL.
 * Layout: w gets vx = lambda2, vy = Q and in 3-D vz = Omega; omega (NULL or a vector) gets Omega in vx -- the omg file, and the
 * only way to Omega in 2-D.  Pressure, scalar and unused velocity slots of both are 0.  q is read only; w == q, omega == q,
 * omega == w, a NULL q or w: NSK_EINVAL.  Contexts of nsk_init_masks are accepted (no mask is read).  One launch, no gather, no
 * atomics: two calls give the same bits.  F (lx1^2 doubles, built on the host for the weight of the call and kept until the
 * weight changes or nsk_finalize) is the only allocation; no captured step graph, launch budget or option is touched. */
int nsk_vortex_criteria(nsk_ctx* ctx, nsk_vec q, double wght, nsk_vec w, nsk_vec omega);
/* Selective frequency damping (SFD, core/fixedp.f:114-242, uparam(1) = 1.1): f = v^nsteps, the state after nsteps steps of the
 * FULL equations from v^0 = q under the force -chi (v - qbar), qbar a low-pass-filtered copy of the velocity.  nsteps, dt and
 * the base state of the CFL rule are nsk_nonlinear_map's (nsk_set_baseflow / nsk_set_nsteps).  The reference calls SFD after
 * every step; call j sees v^j:
 *   call 0:      vxo = v^0, the Adams-Bashforth lags uta = utb = utc = 0; qbar^0 is the caller's `qbar` (velocity components
 *                read, the rest ignored) where the reference sets qbar^0 = v^0 -- pass a copy of q for the reference's run
 *   call j >= 1: utc <- utb, utb <- uta, uta <- vxo - qbar^{j-1};  qbar^j = qbar^{j-1} + omega_c dt (a uta + b utb + c utc),
 *                (a, b, c) = setab3 at constant dt: (3/2, -1/2, 0) for j <= 2, (23/12, -16/12, 5/12) after
 *   every call:  the force of step j + 1 is -chi (vxo - qbar^j), added times bm1 where nekStab_forcing adds fcx (before the EXT
 *                extrapolation).  vxo is still v^{j-1} there: the force LAGS THE VELOCITY BY ONE STEP, the reference's order,
 *                kept.  (The force of step 1 is -chi (v^0 - qbar^0).)
 *   call j >= 1: residu_j = sqrt(sum_c sum bm1 (v^{j-1} - v^j)_c^2 / volume) (normvc's l2: plain bm1), then vxo <- v^j
 * qbar leaves as qbar^nsteps (its velocity components; the rest is not written).  residu: NULL or nsteps doubles, residu_1 ..
 * residu_nsteps, accumulated on the device in a fixed order (no atomics) and copied once behind the map: no host
 * synchronisation per step.  A following call with q <- f and the returned qbar continues the run; the seams are the restart
 * of the BDF / EXT order ramp, which every map of this library has, and of the filter's Adams-Bashforth ramp (lags zero, second
 * order for two calls).  Neither moves the fixed point v = qbar = steady solution.  chi = 0: f has the bits of
 * nsk_nonlinear_map from the same context state (the filter still runs) -- an SFD map takes eager steps on the class launch
 * budgets with convection and right-hand side as two kernels, the plain map may replay captured steps on per-step budgets or
 * persistent tails with the two fused (option "conv_fuse"); those forms return the same bits (checked on the cylinder at
 * lx1 = 6 with every default on).  The steps run eagerly, as nsk_forced_map's: no captured step graph and no launch budget
 * of the unforced maps is touched -- the budgets are frozen and put back.  An SFD map whose solves outrun them is
 * redone once with doubled budgets; those are kept aside for the SFD maps that follow on this context (they only grow).
 * Memory: three velocity-sized arrays per context (vxo and two lags; uta is recomputed), allocated at the first call and kept
 * until nsk_finalize -- 3 x ndim x nloc doubles, about 7 GB at BASELINE config 5's size; the filter state itself lives in f
 * while the map runs.  Shards keep their own elements' part.
 * NSK_EINVAL: shards (use nsk_group_sfd_map), rank-local contexts, lanes; a NULL vector; f, q, qbar not three distinct
 * vectors; chi < 0 or omega_c < 0. */
int nsk_sfd_map(nsk_ctx* ctx, nsk_vec f, nsk_vec q, nsk_vec qbar, double chi, double omega_c, double* residu);
/* BoostConv (core/fixedp.f:282-468, uparam(1) = 1.2): the residual-recombination accelerator of the fixed-point iteration
 * v <- v + r(v), r = the velocity behind a time step minus the velocity before it.
 *
 * nsk_boostconv_init (:353-368): allocate or reset the state of boostconv_core -- X(snp), Y(snp) velocity-sized and zero, the
 * Gram matrix D = Y^T bm1 Y, rot -- so that the next call is a first call.  1 <= snp <= 16 (bst_snp).  Memory: 2 x snp x ndim x
 * nloc doubles, about 48 GB at BASELINE config 5's size with snp = 10, kept until nsk_finalize or an init with another snp;
 * the first nsk_boostconv_map adds a copy of the same size (below).  Shards keep their own elements' part.
 *
 * nsk_boostconv_core (:331-393): boostconv_core on the velocity components of rb, in place: rb = r on entry, xi on return; the
 * rest of rb (pressure, scalars) is not touched.
 *   first call:  Y(1) = X(1) = r;  rot = 1;  xi = r
 *   later calls: Y(rot) -= r;  X(rot) -= Y(rot);  c = argmin |Y c - r| in the bm1 inner product (plain bm1, velocity only);
 *                rot = mod(rot, snp) + 1;  Y(rot) = r;  xi = r + sum_j c_j X(j) (the OLD X(rot) included);  X(rot) = xi
 * The reference finds c by a modified Gram-Schmidt QR of all snp columns at every call (qr_dec, linear_system).  Here only the
 * column of D that changed is recomputed (2 snp + 1 sums per call, fixed order, no atomics) and D c = Y^T bm1 r is solved on
 * the device: scaled by its diagonal, columns with D_jj < 1e-60 get c_j = 0 (the reference's rule, :436), Cholesky with
 * diagonal pivoting, a scaled pivot below snp 2^-52 ends the factorisation and the columns left get c = 0.  ONE DEVIATION:
 * where two stored differences are parallel to within about 1e-8 the reference divides by a tiny R_jj; this code drops the column.
 *
 * nsk_boostconv_map (:282-329): f = the state after nsteps steps of the FULL equations from q -- nsk_nonlinear_map's steps, run
 * eagerly on frozen launch budgets exactly as nsk_sfd_map runs them -- with one BoostConv call behind certain steps.  step0 is
 * the global step count at the start of the map (the reference's istep): a call follows step j = 1 .. nsteps of the map when
 * (step0 + j) % skip == 0 (bst_skp), and j = 0 when step0 == 0.  A call behind step j:
 *   r = v^j - v^{j-1} (the time stepper's lag slot 1; j = 0: the lag arrays of the reference are still zero at istep = 0, so
 *   r = v^0 -- kept);  residu = sqrt(sum_c sum bm1 r_c^2 / volume) (normvc's l2);  xi = boostconv_core(r);  v^j <- v^{j-1} + xi.
 * The lag arrays, the pressure and every other time-stepper array stay as they are, as in the reference.  residu: NULL or at
 * least nsteps / skip + 2 doubles, one per call in call order, written on the device and copied once behind the map (no host
 * read inside a map); ncalls: NULL or their count.  With skip > nsteps and step0 = 1 no call is made and f has the bits of
 * nsk_nonlinear_map from the same context state.  A following map with q <- f and step0 + nsteps continues the run (the seam is
 * the restart of the BDF / EXT ramp, as every map's).  A map whose solves outrun the launch budgets is redone once with doubled
 * ones, kept aside for the BoostConv maps that follow; the calls of the first attempt have advanced X, Y and D, so a map copies
 * them when it starts (the second 2 x snp velocity vectors) and a redone or failed map starts from / leaves that copy.
 * NSK_EINVAL: shards (use nsk_group_boostconv_*), rank-local contexts, lanes; a NULL vector; f == q; skip < 1; step0 < 0;
 * snp out of range; core or map without a prior nsk_boostconv_init. */
int nsk_boostconv_init(nsk_ctx* ctx, int snp);
int nsk_boostconv_core(nsk_ctx* ctx, nsk_vec rb);
int nsk_boostconv_map(nsk_ctx* ctx, nsk_vec f, nsk_vec q, int skip, long long step0, double* residu, int* ncalls);
/* Put X, Y, D and rot back to what the last nsk_boostconv_map of this context found when it started (the copy it took), so that
 * the same map can be run again, shorter: how a driver stops at the call that converged (the reference ends the run there,
 * :315-324).  NSK_EINVAL: no map since nsk_boostconv_init, and nsk_boostconv_core's refusals. */
int nsk_boostconv_rewind(nsk_ctx* ctx);

/* ---- lanes: independent maps in flight at once on one GPU ----
 * nsk_clone gives a context a second LANE: its own stream, time-stepper state, solver work arrays and projection space; geometry,
 * operators and preconditioner are shared (quadrilateral full-mesh contexts).  nsk_matvec_batch(lanes, b, mode, f, q) runs
 * f[k] = map(q[k]) on lane k, all b maps queued before any is waited for: a single map is a chain of dependent 5-15 us kernels and
 * leaves the launch pipeline ~40 % idle on BASELINE config 2; two lanes reach ~1.6x the matvecs/s of one.  The reference has no
 * counterpart (one MPI job = one map); users: band Arnoldi (nekstab_amd/krylov.py: band_arnoldi), sweeps.  Vectors allocated on
 * any lane are usable on all of them; finalize clones before the context they were cloned from. */
int nsk_clone(nsk_ctx* ctx, nsk_ctx** lane);
int nsk_matvec_batch(nsk_ctx** lanes, int b, int mode, nsk_vec* f, nsk_vec* q);

/* ---- statistics of the last nsk_matvec (define the algorithmic bytes) ---- */
typedef struct {
  long long steps;
  long long helm_iters;     /* summed over steps (both components advance together) */
  long long pres_iters;
  long long unconverged;    /* solves that hit the cap */
  double last_helm_res, last_pres_res;
  long long max_helm_iter, max_pres_iter;   /* worst single solve */
  long long budget_helm, budget_pres;       /* iterations currently launched per solve */
  long long recaptures, retries;            /* graph re-captures / maps redone with larger budgets (since init) */
  long long capped_solves;                  /* pressure solves ended by "pres_cap" above their tolerance (last matvec) */
  double worst_cap_ratio;                   /* largest residual / tolerance among them */
  long long total_capped_solves;            /* the same two since nsk_init */
  double total_worst_cap_ratio;
  long long total_helm_iters, total_pres_iters, total_steps;   /* since nsk_init: what bytes_per_matvec is computed from */
  double recapture_seconds;                 /* host time spent (re)capturing and instantiating the step graphs since nsk_init */
  long long total_pres_jsum;                /* since nsk_init: sum over all GMRES columns of their basis index j (Gram-Schmidt bytes) */
  double coarse_bytes_per_solve;            /* operator bytes ONE coarse solve reads (dense / block-circulant inverse, or degree x sparse rows) */
  /* per-time-step launch budgets (option "step_budgets"): maps run on them since init and the launches they budgeted per
   * time step on average (velocity: k_helm launches; pressure: GMRES iterations), 0 while none ran */
  long long step_budget_maps;
  double step_budget_helm_mean, step_budget_pres_mean;
  long long tail_maps;                      /* maps whose solves ended in the persistent tail kernels (option "tail"): the per-step numbers above are then HEADS */
  long long zero_arrays;                    /* hexahedra: bit mask of the arrays that are zero on every node and therefore not loaded: bits 0-8 the
                                               nine metric terms, 9-11 the G factors g4 g5 g6 (set-up), 12-23 the twelve base-flow constants of the
                                               convection kernel (nsk_set_baseflow); 0 on quadrilaterals, on deformed meshes, with option zero_metrics = 0 */
  long long absorb_maps;                    /* maps since init whose time steps ran without a k_proj_update launch: the update of the pressure projection
                                               space applied by its next readers (option "proj_absorb"; one flush launch per map).  0 wherever the option
                                               does not apply: hexahedra, shards, host-checked meshes, fuse2 = 0, nproj = 0 */
  long long convfuse_steps;                 /* time steps since init that ran convection and the velocity right-hand side in ONE launch (k_convect_rhs, option
                                               "conv_fuse") instead of k_convect + k_rhs (a redone map counts again).  0 wherever the option does not apply:
                                               hexahedra, shards, forced maps, the persistent velocity solve */
  long long helmpack_steps;                 /* time steps since init whose velocity solve ran on the packed scratch arrays (option "helm_pack": 16-byte
                                               accesses in k_helm / k_helm_tail / k_pres_rhs; a redone map counts again).  0 wherever the option does not
                                               apply: hexahedra, shards, the persistent velocity solve, and lx1 = 12 unless the option is 1 */
  long long leanargs_steps;                 /* time steps since init whose iteration kernels (k_helm, k_schwarz_uc, k_divgs_t) took their arguments as compact
                                               blocks (option "lean_args"; a redone map counts again).  0 wherever the option does not apply: hexahedra,
                                               shards, the persistent velocity solve */
  long long idxfirst_steps;                 /* time steps since init whose k_divgs_t_l (B_j of the pressure iteration) loaded its gather-table entry together
                                               with the convergence flag (option "idx_first"; a redone map counts again).  0 wherever the compact blocks do
                                               not run: hexahedra, shards, the persistent velocity solve, lean_args = 0 */
} nsk_stats;
int nsk_get_stats(nsk_ctx* ctx, nsk_stats* s);

/* ---- element sharding: one shard per rank, cut out of a full-mesh context --------
 * part[e] = owning rank of global element e.  The parent's set-up (geometry, Jacobi diagonal,
 * Schwarz patches, coarse inverse) is replicated; state, halos and reductions are per rank.
 * Vectors of a shard hold its own elements only ([vx | vy | pr], local element order: nsk_shard_elems).  Ranks that live in one process ("virtual ranks", what the single-GPU tests
 * use) advance in lock-step through nsk_group_matvec with loop-back copies as transport; ranks in
 * separate processes use RCCL (build with -DNSK_WITH_RCCL, nsk_comm_init_rccl). */
int nsk_shard_create(nsk_ctx* parent, const int* part, int rank, int nranks, nsk_ctx** out);
/* Local element order of a shard: its BOUNDARY elements (a node shared with another rank) first, the interior behind, each
 * group by ascending global id; out[le] = global id of local element le (nsk_vec_upload / _download of a shard move element
 * blocks in this order).  Option "halo_overlap" (nsk_set_option on the shard, eager steps): the velocity solve and the
 * pressure iteration launch the boundary workgroups apart from the interior ones and move the halos on a second stream while
 * the interior workgroups run; the all-reduces wait for both (events).  Bit-identical to the serial order of the same shard. */
int nsk_shard_elems(nsk_ctx* shard, long long* out);
/* The exchange plan of a shard, per peer rank p (arrays of nranks entries, 0 where p is no neighbour): vel[p] = global nodes
 * whose partial sums travel in one dssum message to AND from p (one double per node and component); pres_send[p] / pres_recv[p]
 * = pressure dofs of a GMRES basis vector sent to / received from p (the Schwarz patch layers).  Two ranks' plans must agree:
 * vel is symmetric and pres_send[p] on rank r = pres_recv[r] on rank p (tests/test_local_setup_gpu.py checks it on 8 ranks
 * against the host-side derivation nekstab_amd.sharded.velocity_halo_plan). */
int nsk_shard_halo_counts(nsk_ctx* shard, int* vel, int* pres_send, int* pres_recv);
int nsk_group_matvec(nsk_ctx** shards, int n, int mode, nsk_vec* f, nsk_vec* q);    /* every mode of nsk_matvec */
/* The rest of the operator interface on shards, for the ranks living in this process (the reference runs all of it under MPI):
 *   nsk_group_nonlinear_map  nonlinear_forward_map, core/newton_krylov.f:336-378 (subtract_q != 0: Phi_T(q) - q)
 *   nsk_group_set_baseflow   new linearisation point + prepare_linearized_solver: dt / nsteps from the CFL maximum over ALL ranks
 *   nsk_group_set_orbit      time-periodic base flow (uparam(1) = 3.11 / 3.21, core/matvec.f:191-236), stored per rank
 * Singular pressure operators (adjoint runs, closed domains) shard like the others: `ortho` takes its mean over all ranks.
 * Shards keep the parent's pressure projection space size (nsk_case.nproj), so the sharded operator is the single-rank one. */
int nsk_group_nonlinear_map(nsk_ctx** shards, int n, nsk_vec* f, nsk_vec* q, int subtract_q);
int nsk_group_set_baseflow(nsk_ctx** shards, int n, nsk_vec* q);
int nsk_group_set_orbit(nsk_ctx** shards, int n, nsk_vec* q0, double spng_str, nsk_vec* end);
/* The Fourier form of the orbit on shards (nsk_set_orbit_fourier / nsk_set_orbit_modes / nsk_get_orbit_modes for the ranks of
 * this process; n = 1 with a transport attached: one process per GPU).  Every rank keeps the modes of its OWN elements,
 * (2 M + 1) * ndim * nloc_of_the_shard doubles, and its own cos / sin table; the sharded step rebuilds the base-flow constants of
 * the running step per rank.  Shards of full-mesh and of rank-local parents alike.
 *   nsk_group_set_orbit_fourier: the integration of nsk_group_set_orbit (bit for bit: the modes are summed from the stepper's
 *     field, which is only read), 0 <= nmodes <= nsteps / 2 checked once nsteps is known.  `amp` (NULL or 2 nmodes + 1 doubles):
 *     the bm1-weighted L2 norms of A_0, A_1, B_1, .. over ALL ranks, reduced on the device per rank and summed over the ranks
 *     (rank order for virtual ranks, the transport's all-reduce otherwise); every rank receives the same values.
 *   nsk_group_set_orbit_modes / nsk_group_get_orbit_modes: the mode vectors are RANK-MAJOR,
 *       A[r * (nmodes + 1) + k], k = 0 .. nmodes    and    B[r * nmodes + k - 1], k = 1 .. nmodes
 *     for rank r = 0 .. n-1 of this call, each a vector of shard r.  dt / nsteps: nsk_group_set_baseflow applied to
 *     U(0) = sum_k A_k (CFL maximum over all ranks); `period` need not equal endtime.  get: A = B = NULL for count and period only;
 *     NSK_EINVAL ("no Fourier orbit is active") when none is.
 * nsk_group_set_baseflow / nsk_group_set_orbit end the Fourier form; the two setters here end a stored orbit. */
int nsk_group_set_orbit_fourier(nsk_ctx** shards, int n, nsk_vec* q0, double spng_str, int nmodes, nsk_vec* end, double* amp);
int nsk_group_set_orbit_modes(nsk_ctx** shards, int n, int nmodes, double period, const nsk_vec* A, const nsk_vec* B);
int nsk_group_get_orbit_modes(nsk_ctx** shards, int n, int* nmodes, double* period, nsk_vec* A, nsk_vec* B);
/* Eigenmode post-processing on shards (uparam(1) = 4.0 / 4.1 / 4.2 / 4.3 / 4.41 / 4.42 under the element decomposition): the
 * twins of nsk_biorthogonalize, nsk_wavemaker, nsk_bf_sensitivity, nsk_energy_budget, nsk_forced_map, nsk_vorticity and nsk_vortex_criteria for the ranks living in
 * this process -- same argument checks, NULL rules and outputs, every vector argument an array of n handles (rank r's at [r];
 * n = 1 with a transport attached: one process per GPU).  Shards of full-mesh and of rank-local parents alike, before and after
 * nsk_shard_release_parent (every shard keeps the GLL coordinates of its own elements); other contexts: NSK_EINVAL ("needs
 * shard contexts").
 *   parts: NULL or 4 n handles, RANK-MAJOR: parts[4 r + k], k = tr, ti, pr, pi;  prod: NULL or ndim n handles, prod[ndim r + c]
 *   (the layout of nsk_group_set_orbit_modes);  diss: NULL or n handles.
 *   gamma_delta, integrals[10] and the norms inside biorthogonalize / energy_budget are sums over ALL ranks: every rank reduces
 *   on the device in a fixed order, the ranks are added in rank order (virtual ranks) or by the transport's all-reduce; every
 *   rank receives the same values and two calls on virtual ranks give the same bits.
 *   Averaging over shared nodes (dsavg) exchanges halos: nsk_group_bf_sensitivity makes 4 ndim exchanges of ndim components,
 *   nsk_group_energy_budget two per mode component (ndim components, then 1); the production terms are element-local.
 *   nsk_group_forced_map: NSK_DIRECT / NSK_ADJOINT, force[r] != f[r] on every rank; eager sharded steps -- the captured step
 *   graphs and the launch budgets of the unforced maps are neither used nor changed; force = 0 gives the bits of the eager
 *   nsk_group_matvec.
 *   nsk_group_vorticity: q and w hold n handles each (a NULL entry, or w[r] == q[r]: NSK_EINVAL); ONE halo exchange per call
 *   carrying every curl component (1 in 2-D, 3 in 3-D) in one message per peer.  The divisor is the mass assembled over ALL
 *   ranks: the first call of a group builds it with one further exchange of one component, every shard keeps it (one double per
 *   velocity node) until it is finalised.
 *   nsk_group_vortex_criteria: q, w and (when not NULL) omega hold n handles each; the refusals of nsk_vortex_criteria, per
 *   rank.  The criteria and their filter are element-local (comp_gije, pointwise, filter_s0): NO exchange happens, every rank
 *   computes its own elements; the component stride of the outputs is the shard's own nloc. */
int nsk_group_biorthogonalize(nsk_ctx** shards, int n, nsk_vec* dRe, nsk_vec* dIm, nsk_vec* aRe, nsk_vec* aIm, double* gamma_delta);
int nsk_group_wavemaker(nsk_ctx** shards, int n, nsk_vec* dRe, nsk_vec* dIm, nsk_vec* aRe, nsk_vec* aIm, nsk_vec* wm);
int nsk_group_bf_sensitivity(nsk_ctx** shards, int n, nsk_vec* dRe, nsk_vec* dIm, nsk_vec* aRe, nsk_vec* aIm, nsk_vec* sr, nsk_vec* si, nsk_vec* parts);
int nsk_group_energy_budget(nsk_ctx** shards, int n, nsk_vec* ub, nsk_vec* dRe, nsk_vec* dIm, nsk_vec* prod, nsk_vec* diss, double* integrals);
int nsk_group_forced_map(nsk_ctx** shards, int n, int mode, nsk_vec* f, nsk_vec* q, nsk_vec* force);
int nsk_group_vorticity(nsk_ctx** shards, int n, nsk_vec* q, nsk_vec* w);
int nsk_group_vortex_criteria(nsk_ctx** shards, int n, nsk_vec* q, double wght, nsk_vec* w, nsk_vec* omega);
/* nsk_sfd_map on the ranks of this process: f, q, qbar hold n handles each, every rank filters and forces its own elements (no
 * halo exchange beyond the steps' own).  residu (NULL or nsteps doubles) holds the sums over ALL ranks -- per rank on the device
 * in a fixed order, the ranks added in rank order (virtual ranks) or by the transport's all-reduce behind the map: every rank
 * receives the same values.  Same refusals as nsk_sfd_map, per rank; contexts that are not shards: NSK_EINVAL. */
int nsk_group_sfd_map(nsk_ctx** shards, int n, nsk_vec* f, nsk_vec* q, nsk_vec* qbar, double chi, double omega_c, double* residu);
/* nsk_boostconv_init / _core / _map (core/fixedp.f:282-468) on the ranks of this process: rb, f, q hold n handles each, every
 * rank keeps X and Y of its own elements.  The 2 snp + 1 sums of a call are formed per rank on the device in a fixed order and
 * added over the ranks in rank order (virtual ranks) or by the transport's all-reduce, inside the map; every rank then solves
 * the same small system and gets the same bits of c and residu.  residu and ncalls as nsk_boostconv_map (one array for all
 * ranks).  Same refusals, per rank; contexts that are not shards, ranks that differ in their BoostConv state: NSK_EINVAL. */
int nsk_group_boostconv_init(nsk_ctx** shards, int n, int snp);
int nsk_group_boostconv_core(nsk_ctx** shards, int n, nsk_vec* rb);
int nsk_group_boostconv_map(nsk_ctx** shards, int n, nsk_vec* f, nsk_vec* q, int skip, long long step0, double* residu, int* ncalls);
int nsk_group_boostconv_rewind(nsk_ctx** shards, int n);
/* Once a process has cut its shard(s): free every device array of the parent that shards do not share (element-major geometry,
 * preconditioner factors, state, work arrays and ALL vectors allocated on the parent -- their handles become invalid).  The 1-D
 * bases and the replicated coarse operator stay.  The parent then only answers nsk_info / nsk_get_stats / nsk_finalize
 * (finalize it after its shards).  Option "shard_graph" (nsk_set_option on a shard): the sharded step runs as one hipGraph per
 * step class; -1 (default) = yes unless an RCCL communicator is attached, 0 = eager, 1 = yes, RCCL calls captured too.
 * Option "shard_hostcheck": eager sharded steps read the device's convergence flags on the host (one 4-128 byte copy and a stream
 * synchronisation, from the iteration where the previous solve of the step class ended) and stop ISSUING iterations -- a launch
 * that finds its solve converged costs 2 us, its halo exchange and all-reduce do not; the flags follow from all-reduced sums, so
 * every rank takes the same decision without talking.  -1 (default) = yes once a transport is attached (RCCL or host-staged),
 * 0 = never (launch budgets, as the captured graphs), 1 = always (also virtual ranks: no graphs then).  Bit-identical maps. */
int nsk_shard_release_parent(nsk_ctx* parent);
/* ---- rank-local set-up (what Nek5000 does by construction: every MPI rank sets up its own elements) ------------
 * Instead of the whole mesh, a rank hands over ITS sub-mesh: the elements it owns plus two rings of node-sharing
 * neighbours, in ascending global element id, with the global node ids (gid), the global vertex ids (vert / nvert) and
 * nglob of the whole mesh; own[e] = 1 for the owned elements.  On the owned elements everything element-local is then
 * exactly what the whole-mesh set-up computes (assembled mass, Jacobi diagonals, Schwarz factors: their stencils end
 * inside the rings).  Global facts travel through the caller (MPI / torch.distributed / a loop over virtual ranks):
 *   nsk_local_info    vol_own (sum), ctarg (max), fd_lmax (max), npr_own (sum), nrows = entries of this rank's coarse rows
 *   nsk_local_rows    the rows of the vertex coarse operator A_c of the vertices this rank owns, as (u, v, a) triplets
 *   nsk_local_finish  the reduced scalars and the triplets of ALL ranks (concatenated): sets dt / nsteps, the Jacobi
 *                     diagonals for that dt and builds the (replicated, vertex-level) coarse solve
 *   nsk_shard_create_local   part_sub[e] = owning rank of sub-mesh element e, elem_glob[e] = its global id
 * The shard behaves exactly like one cut from a whole-mesh parent by nsk_shard_create (tests/test_local_setup_gpu.py holds
 * the two against each other); set-up time and memory scale with the sub-mesh. */
int nsk_init_local(const nsk_case* sub, const int* own, nsk_ctx** out);
int nsk_local_info(nsk_ctx* ctx, double* vol_own, double* ctarg, double* fd_lmax, long long* npr_own, long long* nrows);
int nsk_local_rows(nsk_ctx* ctx, int* u, int* v, double* a);
int nsk_local_finish(nsk_ctx* ctx, double vol, double ctarg, double fd_lmax, long long npr_glob, long long nrows, const int* u,
                     const int* v, const double* a);
int nsk_shard_create_local(nsk_ctx* local_parent, const int* part_sub, const long long* elem_glob, int rank, int nranks, nsk_ctx** out);
/* virtual ranks made from separate rank-local parents: move `shard` onto `leader`'s stream (one process, lock-step) */
int nsk_shard_share_stream(nsk_ctx* shard, nsk_ctx* leader);
/* RCCL transport, one process per GPU: rank 0 creates the id, everybody calls init on its shard;
 * afterwards nsk_group_matvec(&shard, 1, ...) exchanges halos / all-reduces over xGMI. */
/* Host-staged transport for ranks in separate processes WITHOUT RCCL (any host message layer: MPI, torch.distributed gloo;
 * what lets several ranks share one GPU in the tests): the library packs on the device, copies to pinned host buffers and
 * calls back.  exchange: send[k] / recv[k] hold counts[k] doubles for peer peers[k] (both directions have the same count);
 * allreduce: sum buf[0..n) over all ranks in place.  Return 0 on success. */
typedef int (*nsk_exchange_fn)(void* user, int npeers, const int* peers, const int* counts, const double* const* send, double* const* recv);
typedef int (*nsk_allreduce_fn)(void* user, double* buf, int n);
int nsk_comm_init_host(nsk_ctx* shard, nsk_exchange_fn exchange, nsk_allreduce_fn allreduce, void* user);
int nsk_comm_unique_id(unsigned char* out128);
int nsk_comm_init_rccl(nsk_ctx* shard, const unsigned char* id128);
int nsk_allreduce_host(nsk_ctx* shard, double* buf, int n);
int nsk_group_test(nsk_ctx** shards, int n, int which, const double* const* in, double* const* out);  /* 0: dssum, 1: E apply */
/* rank-local pieces of update_hessenberg_matrix: partial bm1s dots and the projection update;
 * the host (or an all-reduce) sums the partial dots over the ranks */
int nsk_local_dots(nsk_ctx* ctx, nsk_vec f, const nsk_vec* Q, int nq, double* out);
int nsk_project_out(nsk_ctx* ctx, nsk_vec f, const nsk_vec* Q, int nq, const double* h);

/* diagnostics: CG (slower component) and GMRES iteration counts of every time step of the last map of this context (what the
 * per-step launch budgets follow); *nsteps = steps recorded (0 before the first map and on shard contexts) */
int nsk_get_step_iters(nsk_ctx* ctx, int n, int* helm, int* pres, int* nsteps);

/* measurement hook for bench.py: average duration (us) of `reps` back-to-back launches of a hot
 * kernel ("helm", .., "baseflow_fourier": the per-step reconstruction of an active Fourier orbit), HIP events on the
 * library's stream, full work in every launch */
int nsk_bench_kernel(nsk_ctx* ctx, const char* name, int reps, double* avg_us);

/* ---- kernel-level test hooks (parity against oracle/, tests/test_kernels_gpu.py) ---- */
int nsk_test_axhelm(nsk_ctx* ctx, const double* u, double h1, double h2, double* out); /* local */
int nsk_test_dssum(nsk_ctx* ctx, const double* u, double* out);
int nsk_test_opdiv(nsk_ctx* ctx, const double* u, const double* v, double* out);
int nsk_test_opgradt(nsk_ctx* ctx, const double* p, double* ox, double* oy);
int nsk_test_convect(nsk_ctx* ctx, int adjoint, const double* u, const double* v,
                     double* ox, double* oy);      /* mass-weighted forcing bf (sponge+convection) */
int nsk_test_eapply(nsk_ctx* ctx, const double* p, double* out);   /* D B^-1 D^T p */
int nsk_test_helm_solve(nsk_ctx* ctx, const double* rx, const double* ry, int order,
                        double* ox, double* oy, int* iters);
int nsk_test_pres_solve(nsk_ctx* ctx, const double* g, double* out, int* iters);
/* 3-D element operators, packed arrays: which = 1 weak divergence, 2 D^T p, 3 convection (a = mode), 5 Helmholtz solve (a = order),
 * 8 convection on the matrix cores (lx1 = 8) */
int nsk_test_op3(nsk_ctx* ctx, int which, const double* in, double* out, int a, int* iters);

#ifdef __cplusplus
}
#endif
#endif
