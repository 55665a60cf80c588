/*
 * mamg.h -- C-ABI of the MI355X-native metric-AMG preconditioner.
 *
 * This is the drop-in boundary for the reference's `metric_mono` hot path.
 * In the reference the boundary is Python -> SWIG (haznics) -> HAZmath C:
 *
 *   metricAMG(A, W, idofs=interface_dofs, parameters=parameters)
 *       /root/reference/src/utils.py:86  (without idofs: :88)
 *   BB * r   (cbc.block operator -> HAZmath precond fct, one cycle per call,
 *             `maxit: 1` /root/reference/src/amg_parameters.py:71)
 *       invoked by ConjGrad  /root/reference/src/bidomain_3d.py:149-150
 *   haznics.create_dvector / dvec_create_p / create_ivector  src/utils.py:104-111
 *   PETSc_to_dCSRmat(A)                                      src/utils.py:96,108
 *   haznics.fenics_metric_amg_solver_dcsr(A, b, x, idofs)    src/utils.py:119
 *
 * Conventions: plain pointers and sizes only; 0 = success, negative = error
 * (message via mamg_last_error(), thread-local); no exceptions cross the ABI;
 * the caller owns every input buffer (setup reads them, never keeps them);
 * the handle owns all device memory.  One handle per host thread / stream.
 * All arithmetic is IEEE binary64.  Matrices are CSR with int64 row pointers,
 * int32 column indices, column indices sorted within a row.
 */
#ifndef MAMG_H
#define MAMG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAMG_ABI_VERSION 4

/* ---- status codes ---------------------------------------------------- */
enum {
  MAMG_OK = 0,
  MAMG_ERR_ARG = -1,          /* bad argument / shape                         */
  MAMG_ERR_HIP = -2,          /* HIP runtime error (no device, OOM, launch)   */
  MAMG_ERR_SETUP = -3,        /* hierarchy construction failed                */
  MAMG_ERR_UNSUPPORTED = -4,  /* parameter combination not implemented        */
  MAMG_ERR_NOMEM = -5,        /* host allocation failed                       */
  MAMG_ERR_BREAKDOWN = -6     /* PCG: <r,Br> < 0 (indefinite preconditioner)  */
};

/* ---- parameter enums (HAZmath names, build-defined values) ---------- */
enum { MAMG_UA_AMG = 1, MAMG_SA_AMG = 2 };                       /* AMG_type   */
enum {                                                           /* cycle_type */
  MAMG_V_CYCLE = 1, MAMG_W_CYCLE = 2,
  /* 3 (HAZmath's linear AMLI) is not built: MAMG_ERR_UNSUPPORTED.
   * Nonlinear AMLI (K-cycle; HAZmath's NL_AMLI with its GCG inner solver):
   * on every level but the coarsest, the coarse problem A_c e = b_c is solved
   * by amli_degree steps of flexible (generalised) CG preconditioned by the
   * cycle of that level; the coarsest level is the one dense solve, as in V
   * and W.  The step count is fixed (no residual-based early exit, so an apply
   * stays one graph), and a direction with <p, A p> <= 0 is dropped (no update;
   * K(0) = 0).  The preconditioner is nonlinear in r, homogeneous of degree 1.
   * amli_degree in [1, MAMG_NL_AMLI_MAX], else MAMG_ERR_ARG.  Single GPU:
   * mamg_setup_dist returns MAMG_ERR_UNSUPPORTED before the rank touches its
   * GPU; mamg_set_cycle_storage(MAMG_STORE_F32) on such a handle returns
   * MAMG_ERR_UNSUPPORTED and leaves it as it was.
   * The inner CG's vector steps are launches unless the handle opts in with
   * mamg_set_kcycle_tail(h, 1): the steps of the Krylov levels below the coarse
   * tail's first level then run inside the tail's programs. */
  MAMG_NL_AMLI_CYCLE = 4
};
#define MAMG_NL_AMLI_MAX 4   /* largest amli_degree of MAMG_NL_AMLI_CYCLE */
enum {                                                          /* smoother   */
  MAMG_SMOOTHER_JACOBI = 1,      /* x += w D^-1 r, w = relaxation             */
  MAMG_SMOOTHER_L1DIAG = 2,      /* x += w L1^-1 r, L1_ii = sum_j |a_ij|      */
  MAMG_SMOOTHER_JACOBI_RHO = 3,  /* x += (w/rho(D^-1A)) D^-1 r                */
  /* HAZmath's GS / SGS in a GPU-parallel order: multicolour node-block
   * Gauss-Seidel (forward / forward+backward), BSR2 layout only */
  MAMG_SMOOTHER_GS = 10,
  MAMG_SMOOTHER_SGS = 11,
  /* polynomial smoother (HAZmath/FASP SMOOTHER_POLY): Chebyshev of degree
   * poly_degree in W A on [relaxation/poly_ratio, relaxation], W the
   * JACOBI_RHO (block) smoother, applied as poly_degree weighted steps
   * x += w_k W (b - A x); pre steps k = 1..m, post m..1 (default profile) */
  MAMG_SMOOTHER_POLY = 12,
  /* HAZmath's point-wise GS / SGS (the smoother of the reference's plain AMG,
   * AMGhaz) in a multicolour order: per level the rows of the scalar A_l are
   * coloured on its off-diagonal pattern and swept colour by colour,
   * x_i += (b_i - sum_j a_ij x_j) / a_ii (forward / forward+backward);
   * relaxation does not enter.  CSR layout, num_functions 1 or 2 (2: nodal
   * aggregation, point sweeps); the setup resolves node_block_smoother to 0
   * and builds the hierarchy of SMOOTHER_JACOBI_RHO (winv is exported, the
   * sweeps do not use it).  Level-0 seeds (Schwarz_levels >= 1 with idofs)
   * with any Schwarz_type but MAMG_SCHWARZ_RINGS, a non-symmetric pattern or
   * more than 64 colours: MAMG_ERR_UNSUPPORTED; a missing or non-positive
   * diagonal entry: MAMG_ERR_SETUP.  Single GPU. */
  MAMG_SMOOTHER_GS_POINT = 13,
  MAMG_SMOOTHER_SGS_POINT = 14
};
enum {                                                   /* aggregation_type  */
  MAMG_VMB = 1, MAMG_MIS = 2, MAMG_MWM = 3, MAMG_HEC = 4, MAMG_HEM = 5
};  /* accepted: MIS (deterministic parallel MIS-2), HEM (parallel heavy-edge
       matching) and VMB (Vanek-Mandel-Brezina in
       index order; mamg_setup_gpu reaches the sequential loop's aggregates
       by worklist rounds on the device on its large levels, DESIGN.md
       section 2.10);
       MWM/HEC -> MAMG_ERR_UNSUPPORTED */
enum {                                                   /* Schwarz_type      */
  /* The reference's names (src/amg_parameters.py:83-87, src/utils.py:84):
   * multiplicative Schwarz on the OVERLAPPING blocks seed + Schwarz_maxlvl
   * ring.  SYMMETRIC with Schwarz_maxlvl >= 1 on a nodal system
   * (num_functions 2) runs as MAMG_SCHWARZ_PATCHES when the rings are 1-rings
   * and every node holds a seed (the bidomain), else as MAMG_SCHWARZ_RINGS
   * (sparse seed sets, e.g. EMI's interface); without seeds the level
   * smoother runs everywhere (Schwarz_levels resolved to 0).  With
   * Schwarz_maxlvl 0 the blocks are the seeds' nodes (no overlap) and the
   * type must match the smoother (SYMMETRIC: SGS, FORWARD: GS).  FORWARD /
   * BACKWARD on overlapping blocks, and all three names with rings on scalar
   * systems, return MAMG_ERR_UNSUPPORTED (a scalar system takes the seed
   * rings by their own name, MAMG_SCHWARZ_RINGS). */
  MAMG_SCHWARZ_FORWARD = 1, MAMG_SCHWARZ_BACKWARD = 2, MAMG_SCHWARZ_SYMMETRIC = 3,
  MAMG_SCHWARZ_BLOCK_JACOBI = 4, /* additive non-overlapping seed blocks (GPU) */
  MAMG_SCHWARZ_ADDITIVE = 5,     /* additive overlapping seed + maxlvl-ring blocks
                                    (sparse seed sets, e.g. 3D-1D; CSR layout) */
  /* symmetric multiplicative Schwarz on the seeds' overlapping 1-ring blocks
     (the reference's SCHWARZ_SYMMETRIC with Schwarz_maxlvl 1): one patch per
     node = both fields of its closed neighbourhood, exact local solves, in a
     distance-3 multicolour order; level 0, BSR2 layout, 1 or N GPUs; needs a
     seed dof on every node (the bidomain's idofs) */
  MAMG_SCHWARZ_PATCHES = 6,
  /* the level smoother applied to NON-overlapping seed blocks (a seed plus
     the non-seed dofs that join it, <= Schwarz_mmsize): additive with the
     Jacobi family, multicolour forward with GS, symmetric with SGS (for the
     bidomain: node-block SGS on level 0) */
  MAMG_SCHWARZ_SEED_BLOCKS = 7,
  /* symmetric multiplicative Schwarz on one block per seed = the seed and its
     breadth-first Schwarz_maxlvl ring (<= Schwarz_mmsize dofs), exact local
     solves, blocks in a greedy conflict-colour order (a substitution for
     HAZmath's sequential seed order: the same blocks and local solves in
     another multiplicative order; the oracle's seed-order sweep gives the
     same EMI PCG counts, tests/test_rings_oracle.py), plus node-block GS on
     the dofs in no block (src/utils.py:84: "the interface_dofs has the
     Schwarz and the rest the GS smoother"): the reference's SCHWARZ_SYMMETRIC
     for any seed set that is not one seed per node with 1-rings (EMI's
     interface seeds, the default dict of src/utils.py:60-82); level 0, BSR2
     layout (num_functions 2), 1 or N GPUs.
     Named explicitly it also runs on hierarchies that upload in the CSR
     layout (num_functions 1, or 2 with node_block_smoother 0 or a point-GS
     smoother; the 3D-1D system): the same blocks, inverses and colours, and
     on the dofs in no block point-wise GS, coloured on A_0's pattern
     restricted to uncovered x uncovered.  One level-0 step = ring colours
     ascending, rest forward, rest backward, ring colours descending, nu1
     times before and nu2 times after the coarse correction, whatever
     `smoother` is; levels >= 1 run the level smoother (Jacobi family, POLY,
     GS_POINT / SGS_POINT).  The hierarchy is the Schwarz_levels 0 one, bit
     for bit.  More than 64 rest colours or a non-symmetric rest pattern:
     MAMG_ERR_UNSUPPORTED; a missing or non-positive diagonal entry on an
     uncovered row: MAMG_ERR_SETUP; without seeds Schwarz_levels resolves to
     0.  Single GPU. */
  MAMG_SCHWARZ_RINGS = 8
};
enum { MAMG_OFF = 0, MAMG_ON = 1 };
enum {                                                   /* strength_measure  */
  /* J strong for I iff |a_IJ| >= strong_coupled * (the row's largest
   * off-diagonal |a_IK|): the default, because the classical measure below
   * collapses the bidomain hierarchy at strong_coupled 0.1 */
  MAMG_STRENGTH_ROWMAX = 1,
  /* classical: |a_IJ| >= strong_coupled * sqrt(|a_II a_JJ|) (Vanek, Mandel,
   * Brezina 1996; the measure HAZmath's aggregations are described with) */
  MAMG_STRENGTH_DIAG = 0
};
enum { MAMG_COARSE_DENSE = 32 };  /* coarse_solver: 32 (UMFPACK in HAZmath)  */

/* Parameter dictionary keys of /root/reference/src/amg_parameters.py:67-89
 * (and src/utils.py:60-82), same names, POD, versioned by abi_version. */
typedef struct mamg_params {
  int32_t abi_version;       /* = MAMG_ABI_VERSION                           */
  int32_t AMG_type;          /* MAMG_SA_AMG (default) | MAMG_UA_AMG          */
  int32_t cycle_type;        /* MAMG_V_CYCLE (default) | MAMG_W_CYCLE | MAMG_NL_AMLI_CYCLE */
  int32_t max_levels;        /* 20                                           */
  int32_t maxit;             /* cycles per apply, 1                          */
  int32_t smoother;          /* MAMG_SMOOTHER_JACOBI_RHO (mamg_params_default) */
  double relaxation;         /* 4/3                                          */
  int32_t presmooth_iter;    /* 1                                            */
  int32_t postsmooth_iter;   /* 1                                            */
  int32_t coarse_dof;        /* 100                                          */
  int32_t coarse_solver;     /* 32 -> dense direct                           */
  int32_t coarse_scaling;    /* MAMG_OFF | MAMG_ON: e <- <b_c,e>/<A_c e,e> e  */
  int32_t aggregation_type;  /* MAMG_MIS (parallel MIS-2) | MAMG_HEM | MAMG_VMB */
  double strong_coupled;     /* SoC threshold theta, 0.0                     */
  int32_t max_aggregation;   /* accepted, unused by MIS-2 (documented)       */
  int32_t amli_degree;       /* MAMG_NL_AMLI_CYCLE: inner flexible-CG steps per coarse
                                visit, 1 .. MAMG_NL_AMLI_MAX; V / W: accepted, unused */
  int32_t Schwarz_levels;    /* 1: seed-block Jacobi on level 0 if idofs     */
  int32_t Schwarz_mmsize;    /* max dofs per seed block, 100                 */
  int32_t Schwarz_maxlvl;    /* 1: seed + joined 1-ring; 0: seed node only   */
  int32_t Schwarz_type;      /* MAMG_SCHWARZ_BLOCK_JACOBI                    */
  int32_t Schwarz_blksolver; /* 32 -> dense block inverse                    */
  int32_t print_level;       /* 0 silent                                     */
  double sa_omega;           /* prolongator smoothing numerator, 4/3         */
  int32_t rho_iters;         /* 0: Gershgorin bound of rho(D^-1 A)           */
  int32_t max_coarse_dense;  /* largest coarsest level for dense solve, 8192 */
  int32_t device;            /* HIP device ordinal, 0                        */
  int32_t spmv_lanes;        /* 0 = auto; else lanes per row (2..64, pow2)   */
  /* nodal (systems) aggregation, build-defined extension: dofs field-major,
   * dof = f*nv + node for f < num_functions (the monolithic [u1; u2] order of
   * ii_convert, src/bidomain_3d.py:124,138).  >1 aggregates nodes with a
   * block-norm strength and keeps one coarse column per field/aggregate. */
  int32_t num_functions;     /* 1                                            */
  int32_t node_block_smoother; /* nodal: node-block Jacobi where no seed blocks (1) */
  int32_t sa_block_diag;     /* nodal: smooth P with node-block D^-1 (1)     */
  /* BSR2 device path: fold prolongation into the first post-smoothing sweep,
   * x = x1 + P e + W (r1 - (A P) e), with A P kept from the Galerkin product
   * (one pass over [P | AP] instead of P then A).  1 */
  int32_t post_fusion;
  /* MAMG_SMOOTHER_POLY: Chebyshev degree (1..8, 2) and interval ratio (16) */
  int32_t poly_degree;
  double poly_ratio;
  /* strength of connection: MAMG_STRENGTH_ROWMAX (default) | MAMG_STRENGTH_DIAG
   * (ABI 4) */
  int32_t strength_measure;
} mamg_params;

/* Host CSR view (caller-owned). */
typedef struct mamg_csr {
  int64_t nrows, ncols, nnz;
  const int64_t* rowptr;   /* nrows+1 */
  const int32_t* colind;   /* nnz, sorted per row */
  const double* values;    /* nnz */
} mamg_csr;

typedef struct mamg_handle mamg_handle;   /* device hierarchy + workspace   */
typedef struct mamg_hier mamg_hier;       /* host hierarchy (setup result)  */

/* ---- library ---------------------------------------------------------- */
int mamg_abi_version(void);
/* Release the device blocks the GPU setups keep cached for the process's next
 * setup (their temporaries: after a setup returns, none is in use).  Library
 * housekeeping with no reference counterpart: a caller sharing the GPU with
 * other allocators calls it after its setups; the library also releases them
 * by itself when one of its own allocations runs out of HBM. */
int mamg_release_setup_cache(void);
/* Bound of that cache, bytes per device: at the end of every setup the idle
 * blocks above it are freed (largest first).  bytes < 0: the default, an
 * eighth of the device's HBM; 0: everything released after every setup.
 * The SpGEMM staging block of the GPU setup counts against it. */
int mamg_set_setup_cache_limit(int64_t bytes);
/* Idle cached bytes of a device and its current limit (either may be NULL). */
int mamg_setup_cache_bytes(int device, int64_t* idle_bytes, int64_t* limit_bytes);
const char* mamg_last_error(void);
void mamg_params_default(mamg_params* p);

/* ---- problem generators (the reference's FEniCS assembly restated;
 *      src/bidomain_2d.py:51-99, meshes src/utils.py:149-182) ------------- */
/* Sizes of the monolithic bidomain system on UnitSquare/UnitCube(n). */
int mamg_gen_bidomain_size(int dim, int64_t n, int64_t* nrows, int64_t* nnz);
/* Fill caller buffers rowptr[nrows+1], colind[nnz], values[nnz]. */
int mamg_gen_bidomain(int dim, int64_t n, double gamma, double kappa1,
                      double kappa2, int64_t* rowptr, int32_t* colind,
                      double* values);

/* The same matrix built in device memory by gfx950 kernels (bitwise the host
 * generator's), into caller buffers d_rowptr[nrows+1], d_colind / d_values[nnz]
 * (sizes from mamg_gen_bidomain_size); synchronous.  Multi-GPU ranks generate
 * A_0 in HBM instead of holding it on the host. */
int mamg_gen_bidomain_device(int dim, int64_t n, double gamma, double kappa1, double kappa2, int64_t nnz,
                             int64_t* d_rowptr, int32_t* d_colind, double* d_values);

/* Manufactured solution of the bidomain drivers (src/bidomain_2d.py:7-99,
 * src/bidomain_3d.py:7-49): b[nrows] = the right-hand side of the system
 * mamg_gen_bidomain builds (loads, full-flux terms on tags 3/4, Dirichlet
 * lifting; exact values on the Dirichlet rows). */
int mamg_gen_bidomain_mms(int dim, int64_t n, double gamma, double kappa1,
                          double kappa2, double* b);
/* H1 errors err[2] = |u1 - u1h|_1, |u2 - u2h|_1 of a solution x[nrows]
 * (errornorm(u, uh, 'H1'), src/bidomain_2d.py:239-240). */
int mamg_bidomain_mms_error(int dim, int64_t n, double gamma, double kappa1,
                            double kappa2, const double* x, double* err);

/* ---- host setup (no GPU needed).  The hierarchy keeps a VIEW of A (level
 *      0): the caller keeps A alive until mamg_hier_free. ------------------ */
/* Replaces metricAMG.__init__'s HAZmath setup (src/utils.py:86).  idofs may
 * be NULL (n_idofs = 0): then no seed blocks (src/utils.py:88). */
int mamg_host_setup(const mamg_csr* A, const int32_t* idofs, int64_t n_idofs,
                    const mamg_params* params, mamg_hier** out);
void mamg_hier_free(mamg_hier* h);
int mamg_hier_num_levels(const mamg_hier* h);
/* The parameters the setup ran with, after the reference's Schwarz names are
 * resolved (SCHWARZ_SYMMETRIC on the 1-rings of a nodal system ->
 * SCHWARZ_PATCHES; see the Schwarz_type enum). */
int mamg_hier_params(const mamg_hier* h, mamg_params* out);
/* Sizes of level l: n, nnz(A), nnz(P), nnz(R), nnz(WB) (0 if point smoother),
 * ncoarse (n of level l+1, 0 on the coarsest). */
int mamg_hier_level_sizes(const mamg_hier* h, int l, int64_t* sizes6);
/* Export level l into caller buffers (any pointer may be NULL to skip):
 * A (ptr,col,val), P, R, WB (CSR), winv[n], agg[n] (int64), Ainv[n*n]. */
int mamg_hier_level_export(const mamg_hier* h, int l,
                           int64_t* Aptr, int32_t* Acol, double* Aval,
                           int64_t* Pptr, int32_t* Pcol, double* Pval,
                           int64_t* Rptr, int32_t* Rcol, double* Rval,
                           int64_t* Wptr, int32_t* Wcol, double* Wval,
                           double* winv, int64_t* agg, double* Ainv);

/* ---- multi-GPU partition plan (host only) --------- */
/* Rank `rank` of `nranks`: contiguous node ranges per level, ghost lists,
 * send lists, rank-local matrices.  Levels with <= rep_nodes nodes (and all
 * coarser ones) are replicated.  A nodal hierarchy (num_functions 2,
 * node-block smoothers) gives a BSR2 plan: a node is a pair of dofs, the
 * matrices are 2x2-block.  A scalar hierarchy (num_functions 1) gives a CSR
 * plan: a node is a dof, the matrices are CSR with
 * columns numbered [owned | ghost] and every row sorted by local column, the
 * smoother is the slice of winv or, on level 0 with seed blocks, the owned
 * rows of WB (whose external columns are ghosts too).  num_functions > 2,
 * num_functions 2 with node_block_smoother 0, point-wise GS / SGS and
 * SCHWARZ_RINGS on CSR hierarchies return MAMG_ERR_UNSUPPORTED. */
typedef struct mamg_plan mamg_plan;
int mamg_hier_dist_plan(const mamg_hier* h, int rank, int nranks, int64_t rep_nodes,
                        mamg_plan** out);
void mamg_plan_free(mamg_plan* p);
int mamg_plan_num_levels(const mamg_plan* p);
/* s[16]: nv, replicated, coarsest, o0, o1, nghost, nsend, nbA, nrA, ncA,
 *        nbP, nrP, ncP, nbR, nrR, ncR */
int mamg_plan_level_sizes(const mamg_plan* p, int l, int64_t* s);
/* Export (any pointer may be NULL): ghosts[nghost], ghost_off[nranks+1],
 * send_idx[nsend], send_off[nranks+1], A/P/Rp as BSR2 (ptr, col, val[4 nb]),
 * W[4 nloc].  Scalar plan: nb counts entries, A/P/Rp are CSR (val[nb]) and
 * W[nloc] = winv (untouched where the level smooths with WB). */
int mamg_plan_level_export(const mamg_plan* p, int l, int64_t* ghosts, int64_t* ghost_off,
                           int64_t* send_idx, int64_t* send_off,
                           int64_t* Aptr, int32_t* Acol, double* Aval,
                           int64_t* Pptr, int32_t* Pcol, double* Pval,
                           int64_t* Rptr, int32_t* Rcol, double* Rval, double* W);
/* dofs per node of the plan: 2 (BSR2 plan) or 1 (scalar CSR plan) */
int mamg_plan_dofs_per_node(const mamg_plan* p);
/* Scalar plan: the owned rows of the level's sparse block smoother WB, columns
 * local [owned | ghost] (any pointer may be NULL).  sizes[3] = entries, rows,
 * columns (zeros where the level smooths with winv); ptr[rows + 1],
 * col[entries], val[entries]. */
int mamg_plan_level_wb(const mamg_plan* p, int l, int64_t* sizes, int64_t* ptr, int32_t* col, double* val);

/* ---- multi-GPU apply (one process per GPU, RCCL over xGMI) ------------- */
typedef struct mamg_dhandle mamg_dhandle;
/* size of the RCCL unique id (128); rank 0 creates it, every rank passes it */
int mamg_comm_id_bytes(void);
int mamg_comm_unique_id(void* id);
/* Every rank passes the same global A / idofs / params (the setup -- on the
 * rank's GPU where the profile allows it, else on the host -- is replicated
 * and deterministic) and keeps only its node range of each level; levels
 * with <= rep_nodes nodes are replicated.  V and W cycles, coarse-grid
 * scaling, nu1 / nu2 >= 1.
 *  - Nodal hierarchies (num_functions 2, node-block smoothers, BSR2 layout):
 *    Jacobi-family, POLY and multicolour GS / SGS smoothers, SCHWARZ_PATCHES
 *    and SCHWARZ_RINGS (the latter three with a GPU-setup profile).
 *  - Scalar hierarchies (num_functions 1, CSR layout):
 *    SMOOTHER_JACOBI / L1DIAG / JACOBI_RHO / POLY and the level-0 sparse block
 *    smoother of the seeds (SCHWARZ_ADDITIVE / BLOCK_JACOBI / SEED_BLOCKS with
 *    Schwarz_maxlvl >= 1), e.g. the 3D-1D preset.  Every rank runs the host
 *    setup and plans the whole hierarchy on the host (O(global nnz) host work
 *    per rank).  Local vectors are the plain slices r[o0:o1], z[o0:o1].
 * MAMG_ERR_UNSUPPORTED, the message naming the alternative: point-wise GS /
 * SGS, SCHWARZ_RINGS on CSR hierarchies, num_functions 2 with
 * node_block_smoother 0 (a nodal hierarchy in the CSR layout), num_functions
 * > 2, maxit > 1. */
int mamg_setup_dist(const mamg_csr* A, const int32_t* idofs, int64_t n_idofs,
                    const mamg_params* params, int rank, int nranks, const void* comm_id,
                    int64_t rep_nodes, mamg_dhandle** out);
/* Same with A_0's rowptr / colind / values in device memory (read during
 * setup only), e.g. from mamg_gen_bidomain_device: no rank holds the global
 * matrix on the host.  Covers the GPU setup's node-block profiles (the rank's
 * operators are cut out of the hierarchy in HBM); profiles that plan on the
 * host (scalar hierarchies among them) return MAMG_ERR_UNSUPPORTED. */
int mamg_setup_dist_device(const mamg_csr* dA, const int32_t* idofs, int64_t n_idofs,
                           const mamg_params* params, int rank, int nranks, const void* comm_id,
                           int64_t rep_nodes, mamg_dhandle** out);
/* local node range [o0, o1) of level 0 and the level's nodes nv; local vectors
 * are field-major [u1(o0:o1); u2(o0:o1)] of length 2*(o1-o0) on a nodal
 * handle, the plain slice v[o0:o1] on a scalar one (nv = rows) */
int mamg_dist_range(const mamg_dhandle* h, int64_t* o0, int64_t* o1, int64_t* nv);
/* dofs per node of the handle: 2 (nodal, BSR2) or 1 (scalar, CSR) */
int mamg_dist_dofs_per_node(const mamg_dhandle* h);
/* algorithmic bytes of one apply on this rank: the sum over its op list.
 * Kernels as mamg_apply_bytes counts them on the rank-local operators (CSR:
 * 12 nnz + 8 (rows + 1) + 8 columns + 8 rows, + 8 rows per extra vector of the
 * epilogue).  Exchanges, with w = dofs per node, ns = send-list nodes, ng =
 * ghosts: forward halo 8 ns (indices) + 2 * 8 w ns (pack) + 8 w ng (ghost
 * writes); reverse-add 8 w ng + 3 * 8 w ns + 8 ns; all-reduce of a replicated
 * right-hand side 2 * 8 w nv; of the scaling partials 16 * 256. */
int mamg_dist_apply_bytes(const mamg_dhandle* h, double* bytes);
/* what one mamg_dist_apply_device issues on this rank (counted from its op
 * list, nothing launched): counts[0] kernels, [1] RCCL send / receive groups,
 * [2] point-to-point messages, [3] all-reduces, [4] side-stream forks */
int mamg_dist_apply_launches(const mamg_dhandle* h, int64_t counts[5]);
/* z_local = (B r)_local, enqueued on `stream`.  Streams and ordering: see
 * "Streams and ordering" above mamg_apply -- a rank handle orders its calls
 * across streams exactly as a single-GPU handle does. */
int mamg_dist_apply_device(mamg_dhandle* h, const double* d_r_local, double* d_z_local,
                           void* stream);
/* The same apply replayed from a hipGraph: captured on the first call per
 * (d_r_local, d_z_local) pair, with the rank's kernels, the interior-row
 * side-stream fork and the RCCL send / receive groups and all-reduces inside
 * the capture, then one hipGraphLaunch per call on `stream`.  Bitwise the
 * eager apply's result (same kernels, same order).  MAMG_ERR_UNSUPPORTED for
 * a handle without an RCCL communicator and more than one rank (host-staged
 * or virtual exchanges) and after a failed capture on the handle (the message
 * names the capture error; mamg_dist_apply_device stays available).  No
 * reference counterpart (the reference is serial). */
int mamg_dist_apply_graph(mamg_dhandle* h, const double* d_r_local, double* d_z_local, void* stream);
/* Capture (or find) that graph without launching it: every rank can capture
 * and agree on the outcome before any rank launches a graph whose RCCL calls
 * wait for its peers. */
int mamg_dist_graph_prepare(mamg_dhandle* h, const double* d_r_local, double* d_z_local);
/* y = A x on the rank's rows (the PCG operator; x, y local slices as for the
 * apply): forward halo of x, then the rank-local A.  Replaces the A * d
 * product inside cbc.block ConjGrad (src/bidomain_3d.py:149) on N GPUs. */
int mamg_dist_spmv_device(mamg_dhandle* h, const double* d_x_local, double* d_y_local, void* stream);
/* mode 0: eager, events around the level-0 residual and K launches; 1:
 * eager, events around every op; 2: mamg_dist_apply_graph replays (events
 * around the whole run only, kernel_ms zero) */
int mamg_dist_time_apply(mamg_dhandle* h, const double* d_r, double* d_z, int reps, int mode,
                         double* ms_per_apply, double* kernel_ms, double* class_bytes,
                         void* stream);
/* Test mode: handles created with comm_id == NULL (no RCCL) on one device;
 * apply all n ranks in lockstep, exchanges as device copies. */
int mamg_dist_virtual_apply(mamg_dhandle** hs, int n, const double** d_r, double** d_z,
                            void* stream);
int mamg_dist_virtual_spmv(mamg_dhandle** hs, int n, const double** d_x, double** d_y, void* stream);
/* The virtual ranks' lockstep apply captured into one hipGraph and replayed
 * once (tests: the graph path against the eager lockstep run). */
int mamg_dist_virtual_apply_graph(mamg_dhandle** hs, int n, const double** d_r, double** d_z,
                                  void* stream);
/* Device-resident PCG on the rank's local slices (a contiguous run of
 * w * nloc doubles: field-major on a nodal handle, plain on a scalar one):
 * mamg_pcg_device's loop and semantics on N ranks.  x0 = d_x_local on entry;
 * residuals[k] = sqrt(<r, B r>) (maxiter + 1 entries), alphas / betas maxiter
 * entries, *niters = len(residuals) - 1; MAMG_ERR_BREAKDOWN with the messages
 * of mamg_pcg_device and what it leaves in residuals / alphas / betas /
 * *niters / d_x_local on each of them (not positive: *niters = 0,
 * residuals[0] = 0.0, nothing else written, every rank's x slice untouched;
 * <r,Br> < 0 in iteration k: *niters = k, k + 1 residuals (and rnorms), k
 * alphas / betas, x slices restored to x_k to round-off).  stop_type 0: cbc.block's rule (tol absolute unless
 * relativeconv); 1: HAZmath's linear_stop_type 1, ||r||_2 <= tol ||b||_2 with
 * ||b|| = 0 taken as 1 (one more dot per iteration, fused into the x / r
 * update); rnorms[maxiter + 1] then receives ||r||_2 per iteration and may be
 * NULL for stop_type 0.  Any other stop_type, a NULL handle or buffer and
 * maxiter < 0 return MAMG_ERR_ARG before anything touches the GPU.
 * Every scalar lives in HBM.  One iteration is one op list -- halo + A_loc,
 * <d,q>, alpha, x / r update, the apply, <r,z>, beta + stop test, d update --
 * replayed as one hipGraph per (d_x_local, maxiter, stop_type) on an RCCL or
 * single-rank handle (RCCL calls inside the capture; eager after a failed
 * capture) and run op by op through the callbacks on a host-staged handle.
 * Each rank writes its share of a dot to its own slot of a zeroed P-vector,
 * the P-vector is all-reduced and every rank adds the slots in rank order,
 * so all ranks hold the same bits and issue the same number of iterations;
 * the host stays one iteration ahead and an iteration queued after the
 * stopping one runs its exchanges but leaves x, r and d untouched.
 * Replaces the ConjGrad loop of src/bidomain_3d.py:149 on N GPUs. */
int mamg_dist_pcg_device(mamg_dhandle* h, const double* d_b_local, double* d_x_local,
                         double tol, int maxiter, int relativeconv, int stop_type,
                         double* residuals, double* rnorms, double* alphas, double* betas,
                         int* niters, void* stream);
/* Test mode, as mamg_dist_virtual_apply: the n virtual ranks' iterations in
 * lockstep on one device; graph != 0 captures one lockstep iteration once and
 * replays it.  Every rank's state is compared with rank 0's byte for byte
 * whenever it is read back (a difference: MAMG_ERR_SETUP, the message names
 * the iteration); the histories are rank 0's. */
int mamg_dist_virtual_pcg(mamg_dhandle** hs, int n, const double** d_b, double** d_x,
                          double tol, int maxiter, int relativeconv, int stop_type, int graph,
                          double* residuals, double* rnorms, double* alphas, double* betas,
                          int* niters, void* stream);
/* what one PCG iteration issues on this rank, counted as by
 * mamg_dist_apply_launches: the SpMV, the apply, the PCG kernels and two
 * all-reduces of the dots */
int mamg_dist_pcg_launches(const mamg_dhandle* h, int stop_type, int64_t counts[5]);
void mamg_dist_destroy(mamg_dhandle* h);
/* Host-staged exchange backend: a pluggable transport for a handle made
 * with comm_id == NULL (one process per rank, e.g. torch.distributed gloo).
 * The pack / unpack kernels, the reverse-add in rank order and the op
 * schedule are the RCCL path's; only the transport differs: payloads are
 * staged through pinned host buffers and handed to the callbacks (0 = ok).
 * Arrays are indexed by rank; entries for this rank and zero counts are
 * unused.  Replaces RCCL where it cannot run (two ranks on one GPU). */
typedef struct mamg_exchange {
  void* ctx;
  /* send scount[q] doubles from send[q] to every rank q, receive rcount[q]
     doubles from q into recv[q] */
  int (*sendrecv)(void* ctx, int nranks, double* const* send, const int64_t* scount,
                  double* const* recv, const int64_t* rcount);
  /* in-place sum of buf[count] over all ranks (the same result on every rank) */
  int (*allreduce)(void* ctx, double* buf, int64_t count);
} mamg_exchange;
int mamg_dist_set_exchange(mamg_dhandle* h, const mamg_exchange* ex);

/* ---- device hierarchy ------------------------------------------------- */
/* Host setup + upload.  Level-0 matrix is uploaded from A directly. */
int mamg_setup(const mamg_csr* A, const int32_t* idofs, int64_t n_idofs,
               const mamg_params* params, mamg_handle** out);
/* GPU setup: the same hierarchy as mamg_setup, bit
 * for bit, built by gfx950 kernels -- strength, MIS-2 / HEM / VMB aggregation (VMB: a
 * level of fewer than 131072 nodes, or one whose device rounds pass the cap
 * of DESIGN.md section 2.10, one long chain in index order, is aggregated by
 * the host loop instead, the same numbers), smoothers, SA prolongator, Galerkin
 * products, coarsest inverse -- and the apply layouts built in HBM (no host
 * round trip).  Covers num_functions 1 and 2 with every smoother the host
 * setup builds: node blocks, general (not node-aligned) seed blocks,
 * SCHWARZ_ADDITIVE rings, SCHWARZ_PATCHES / SCHWARZ_RINGS level-0 Schwarz,
 * point smoothers; nodal or point SA.  Other profiles (num_functions > 2, a
 * hash SpGEMM row of more than 2048 distinct columns) return
 * MAMG_ERR_UNSUPPORTED (use mamg_setup).  Replaces the setup half of
 * metricAMG.__init__ (src/utils.py:86).  A: host CSR, copied once. */
int mamg_setup_gpu(const mamg_csr* A, const int32_t* idofs, int64_t n_idofs,
                   const mamg_params* params, mamg_handle** out);
/* Same with A's rowptr/colind/values in device memory (read during setup
 * only; the caller may free them afterwards).  idofs: host array. */
int mamg_setup_gpu_device(const mamg_csr* dA, const int32_t* idofs, int64_t n_idofs,
                          const mamg_params* params, mamg_handle** out);
/* GPU setup, hierarchy copied back into a host mamg_hier (tests, multi-GPU
 * planning); the hierarchy keeps a view of A as mamg_host_setup does. */
int mamg_gpu_host_setup(const mamg_csr* A, const int32_t* idofs, int64_t n_idofs,
                        const mamg_params* params, mamg_hier** out);
/* Setup phase timings of a GPU-setup handle, ms[8]: aggregation, smoothers,
 * prolongator, Galerkin, coarsest, apply-layout build, setup total, A upload
 * (zeros for handles from mamg_setup / mamg_upload). */
int mamg_setup_timings(const mamg_handle* h, double* ms8);
/* The apply-layout phase of any handle split, ms[4]: layout build (device
 * formats of every level), level-0 K value region trials (bounded by time and
 * free HBM), operator re-homing, finish (tail plan,
 * final synchronisation). */
int mamg_layout_timings(const mamg_handle* h, double* ms4);

/* Upload an existing host hierarchy (level 0 matrix taken from A). */
int mamg_upload(const mamg_hier* h, const mamg_csr* A, const mamg_params* params,
                mamg_handle** out);
void mamg_destroy(mamg_handle* h);

int64_t mamg_nrows(const mamg_handle* h);
int mamg_num_levels(const mamg_handle* h);
/* Device layout chosen at upload: 0 = CSR (general; always with the
 * point-wise SMOOTHER_GS_POINT / SGS_POINT), 1 = BSR2 (nodal hierarchy with
 * num_functions == 2 and node-block smoothers). */
int mamg_device_layout(const mamg_handle* h);
/* Storage of level l's operator on the device (BSR2 layout), bit flags:
 * MAMG_FMT_SELL (sliced-ELL, one lane per node row), MAMG_FMT_SYM (3 doubles
 * per symmetric 2x2 block), MAMG_FMT_POST_FUSED (prolongation fused with the
 * first post sweep), MAMG_FMT_POST_K (... through one stored operator
 * K = P - W (A P): z = x1 + W r1 + K e; else through [P | AP]),
 * MAMG_FMT_POST_SELL (K stored sliced-ELL), MAMG_FMT_HALF (A stored as its
 * upper half, ELL-64, lower blocks read through their mirrors), MAMG_FMT_BANDS
 * (the half-symmetric kernel walks the rows in plane bands per XCD; order
 * only, results are bitwise those of row order).
 * Returns flags >= 0, or < 0. */
enum { MAMG_FMT_SELL = 1, MAMG_FMT_SYM = 2, MAMG_FMT_POST_FUSED = 4, MAMG_FMT_POST_K = 8,
       MAMG_FMT_POST_SELL = 16, MAMG_FMT_HALF = 32, MAMG_FMT_BANDS = 64,
       MAMG_FMT_PATCHES = 128,  /* smoother: multiplicative node-patch Schwarz (SCHWARZ_PATCHES) */
       MAMG_FMT_GS = 256,       /* smoother: multicolour GS / SGS sweeps (node-block: BSR2 layout;
                                   point-wise, SMOOTHER_GS_POINT / SGS_POINT: CSR layout) */
       MAMG_FMT_RINGS = 512,    /* smoother: multiplicative seed-ring Schwarz + GS on the rest (SCHWARZ_RINGS;
                                   on the CSR layout level 0 reports MAMG_FMT_RINGS | MAMG_FMT_GS) */
       MAMG_FMT_R_BANDS = 1024,    /* restriction rows walked plane band by plane band per XCD */
       MAMG_FMT_K_COL16 = 2048,    /* K's columns as 16-bit offsets from a per-slice base */
       MAMG_FMT_ROWDICT = 4096,    /* A stored as one row-type code per node row plus a table of the
                                      distinct rows (its rows repeat; neither SELL nor HALF is then set) */
       MAMG_FMT_POST_MF = 8192 };  /* matrix-free prolongation (level 0 on the dictionary): P e =
                                      (I - w D_B^-1 A)(T e) through the aggregate index and A's dictionary,
                                      no stored K or P; neither POST_FUSED nor POST_K is then set, and
                                      every post sweep is the plain block-Jacobi pass */
int mamg_level_format(const mamg_handle* h, int level);
/* The parameters the handle runs (as mamg_hier_params). */
int mamg_handle_params(const mamg_handle* h, mamg_params* out);
/* Placement of the level-0 K values: the K kernel's
 * time per candidate memory region tried at upload, ms[0 .. *n) (at most cap),
 * and the index kept (*kept = -1: no selection ran). */
int mamg_kregion_info(const mamg_handle* h, double* ms, int cap, int* n, int* kept);
/* Algorithmic HBM bytes of one apply (SURVEY 8d formula) and of its dominant
 * kernel class; see DESIGN.md section 4.  A point-wise GS colour step of
 * `rows` rows holding `nnz` entries counts 12 nnz (values, columns) +
 * 8 (rows + 1) (pointers) + 4 rows (perm) + 8 rows (1/a_ii) + 8 rows (b) +
 * 16 rows (own x read, written) + 8 n / ncolours (the gathered x, every entry
 * once per sweep); a small level's one-launch smoothing call counts the sum
 * over its colour steps.  A seed-ring colour step
 * on the CSR layout whose blocks hold d_k members each, `m` members in all
 * with `nnz` entries in their rows of A_0, counts 8 sum d_k^2 (inverses) +
 * 12 nnz (values, columns) + 8 nnz (the gathered x) + 16 m (pointers) +
 * 4 m (members) + 8 m (b) + 16 m (own x read, written) + 16 per block
 * (offsets). */
int mamg_apply_bytes(const mamg_handle* h, double* total_bytes);

/* Storage precision of the operators the cycle streams (DESIGN.md section
 * 4.7).  MAMG_STORE_F32 narrows a single-GPU BSR2 handle (Jacobi family or
 * SMOOTHER_POLY; V or W cycle, any nu1 / nu2, with or without coarse scaling)
 * after its setup: every value array the cycle's launches read -- A_l, K_l or
 * P_l, R_l of the levels above the coarse tail and the coarsest level -- is
 * replaced by an fp32 copy rounded to nearest even, in the same layout, and
 * the kernels convert on load.  Sums, the smoother blocks W, the POLY step
 * smoothers, the coarsest inverse, every vector and every dot stay fp64: one
 * apply is the fp64 cycle on the rounded operators up to summation order.
 * mamg_spmv_device and the A d product of mamg_pcg_device keep reading the
 * fp64 A_0 (the handle holds both value arrays of A_0; the other fp64
 * originals are freed), so the PCG solves the caller's system.  A level
 * stored as merged [P | AP] (MAMG_POST_K=0) keeps that operator fp64.
 * One way: MAMG_STORE_F32 on a narrowed handle is a no-op, MAMG_STORE_F64
 * returns MAMG_OK on an un-narrowed handle and MAMG_ERR_UNSUPPORTED on a
 * narrowed one.  MAMG_ERR_UNSUPPORTED, the handle untouched and the message
 * naming the reason, for CSR-layout handles, GS / SGS, SCHWARZ_PATCHES and
 * SCHWARZ_RINGS handles, and for a handle holding a finite value whose fp32
 * rounding is not finite.  MAMG_ERR_ARG for a NULL handle or another storage
 * value.  The call waits for the handle's queued work and drops its cached
 * apply and PCG graphs; it must not run concurrently with other calls on the
 * same handle.
 * Bytes (mamg_apply_bytes, mamg_time_apply's class_bytes): a narrowed
 * operator counts 4 bytes per stored value, so a block with its column is
 * 16 B where fp64 counts 28 (SYM and half-symmetric upper blocks: 3 values +
 * a 4-byte column), 20 B where it counts 36 (general: 4 values + a 4-byte
 * column) and 18 B where it counts 34 (K with 16-bit columns); pointers, row
 * meta, mirror slots and every vector term are unchanged. */
enum { MAMG_STORE_F64 = 0, MAMG_STORE_F32 = 1 };
/* Narrow the operators the cycle reads to fp32 storage (one way). */
int mamg_set_cycle_storage(mamg_handle* h, int storage);
/* bit 0: A_l as the cycle reads it, bit 1: K_l / P_l, bit 2: R_l stored fp32; 0 before narrowing */
int mamg_level_storage(const mamg_handle* h, int level);

/* ---- the nonlinear AMLI cycle's inner CG inside the coarse tail --------
 * (DESIGN.md sections 2.13, 4.2).  The coarse tail runs the cycle of the small
 * levels as one single-workgroup program per visit.  After setup (state 0) a
 * MAMG_NL_AMLI_CYCLE handle keeps every level with a Krylov level below it out
 * of the tail, because the flexible CG's steps (dots, orthogonalisation,
 * update) exist as launches only.  on = 1: those steps become tail ops, so the
 * tail starts at the level its size rule picks (MAMG_TAIL_NODES), Krylov levels
 * inside it included; on = 0: back to launches.  Both states compute the same
 * steps with the same reduction order; the results agree to summation order of
 * the tail's SpMVs (1e-11 relative on the tested systems, 1e-10 against the
 * restatement tests/kcycle_ref.py).  The call is made after setup, waits for
 * the handle's queued work, drops its cached apply graphs, PCG graphs and tail
 * programs, and the next apply plans again; nothing is destroyed, so it is
 * reversible.  MAMG_OK and no effect on the apply for a K-cycle BSR2 handle
 * without a tail level.  MAMG_ERR_UNSUPPORTED, the handle untouched and the
 * message naming the reason, for a handle whose cycle is not
 * MAMG_NL_AMLI_CYCLE and for a CSR-layout handle (the tail is BSR2 only).
 * MAMG_ERR_ARG for a NULL handle or another value of on.  Single GPU (rank
 * handles refuse the cycle itself); mamg_set_cycle_storage(MAMG_STORE_F32)
 * keeps refusing the handle in either state.  It must not run concurrently
 * with other calls on the same handle. */
int mamg_set_kcycle_tail(mamg_handle* h, int on);
/* the state: 1 / 0; MAMG_ERR_ARG for a NULL handle */
int mamg_kcycle_tail(const mamg_handle* h);

/* What one mamg_apply_device issues: the launches (kernels and memsets) of the
 * handle's op list as it stands, a coarse-tail program counting as one.
 * Counted from the list, nothing is launched (a tail program not planned yet
 * is planned); as mamg_dist_apply_launches on a rank handle. */
int mamg_apply_launches(const mamg_handle* h, int64_t* launches);

/* The same on a rank handle, after its setup.  The
 * call needs no communication and every rank of a communicator (every
 * virtual rank of a list) MUST make the same call: ranks cannot check each
 * other without an exchange, and a narrowed rank next to an fp64 one applies
 * an operator that is neither.  Narrowed, on every level above the coarsest,
 * distributed or replicated: A_loc (on level 0 both value arrays of the
 * half-symmetric form, the owned part and the ghost part), K_loc -- formed in
 * fp64, then rounded -- or plain P_loc under post_fusion 0, and the partial
 * restriction Rp_loc.  Kept fp64: the smoother blocks W / Wk, the coarsest
 * inverse, every vector, the halo, send and receive buffers, a merged
 * [P_loc | AP_loc] (MAMG_POST_K=0: bits 1 and 4 only), and the Krylov
 * operator -- mamg_dist_spmv_device, mamg_dist_virtual_spmv and the A d
 * product of mamg_dist_pcg_device / mamg_dist_virtual_pcg keep reading the
 * fp64 level-0 A_loc, whose index arrays the fp32 copy shares.  One apply of
 * N narrowed ranks is the narrowed one-GPU apply up to summation order.
 * Returns as mamg_set_cycle_storage: MAMG_ERR_UNSUPPORTED, the handle
 * untouched and the reason named, for scalar (CSR, dofs_per_node 1) rank
 * handles, GS / SGS, SCHWARZ_PATCHES and SCHWARZ_RINGS rank handles, a finite
 * value whose fp32 rounding is not finite (every array is checked before any
 * is converted) and MAMG_STORE_F64 on a narrowed handle; MAMG_OK for
 * MAMG_STORE_F64 on an un-narrowed handle and a second MAMG_STORE_F32;
 * MAMG_ERR_ARG for a NULL handle or another storage value.  The call waits
 * for the handle's queued work, drops its cached apply graphs and PCG plans
 * and recounts mamg_dist_apply_bytes at 4 bytes per narrowed value.
 * mamg_dist_virtual_apply, _apply_graph, _spmv and _virtual_pcg return
 * MAMG_ERR_ARG when the handles of one list disagree in storage. */
int mamg_dist_set_cycle_storage(mamg_dhandle* h, int storage);
/* mamg_level_storage's bits for the rank-local operators of `level` */
int mamg_dist_level_storage(const mamg_dhandle* h, int level);
/* levels of the rank's hierarchy, and mamg_level_format's bits for the
 * rank-local operators of one (0 on a scalar rank handle) */
int mamg_dist_num_levels(const mamg_dhandle* h);
int mamg_dist_level_format(const mamg_dhandle* h, int level);

/* Streams and ordering, for both handle types (mamg_handle, mamg_dhandle).
 * Every call that takes a `stream` enqueues all of its device work -- kernels,
 * copies, memsets, graph launches, RCCL calls -- on that stream (hipStream_t,
 * NULL = the legacy default stream), behind whatever the caller queued there
 * before; the handle's own streams (graph capture, the side stream of the
 * interior rows) are forked from and joined back into it by events, so the
 * caller's stream order covers them.  The inputs are read and the outputs
 * written in stream order: a buffer filled by work queued on `stream` before
 * the call is a valid input, no host synchronisation needed.
 * A handle's work vectors (level vectors, ghost, send and receive buffers,
 * the PCG vectors) are shared by all of its calls, so the handle orders them:
 * each call first makes `stream` wait for the handle's previous call, on
 * whatever stream that ran (an event, no host wait), and records its own end.
 * Calls on one handle from different streams therefore run one after the
 * other, in the order the host issued them; calls on different handles are
 * independent.  mamg_dist_virtual_* order against every handle of the list.
 * The ordering is between device work only: the host must not issue calls on
 * one handle from two threads at once (one handle per host thread).
 * mamg_apply_device, mamg_spmv_device, mamg_dist_apply_device,
 * mamg_dist_apply_graph, mamg_dist_spmv_device, mamg_dist_virtual_apply and
 * mamg_dist_virtual_spmv return with the work queued (a host-staged exchange
 * waits for `stream` at every exchange); the PCG calls, the timing hooks,
 * mamg_dist_virtual_apply_graph and the host-pointer mamg_apply wait for
 * their own work before they return. */

/* z = B r : one preconditioner application (`maxit` cycles from x0 = 0).
 * Host pointers (copies in/out, synchronous; ordered behind the handle's
 * queued device-pointer calls). */
int mamg_apply(mamg_handle* h, const double* r, double* z);
/* Device pointers, enqueued on `stream` (hipStream_t, NULL = default).
 * r is not modified; r and z must not alias. */
int mamg_apply_device(mamg_handle* h, const double* d_r, double* d_z,
                      void* stream);
/* y = A x with the level-0 operator (device pointers). */
int mamg_spmv_device(mamg_handle* h, const double* d_x, double* d_y,
                     void* stream);

/* Device-resident preconditioned CG with cbc.block ConjGrad semantics
 * (src/bidomain_3d.py:149-160): x0 = d_x on entry, residuals = sqrt(<r,Br>),
 * stop when residual <= tol (times residual[0] if relativeconv) or after
 * maxiter iterations.  residuals[maxiter+1], alphas[maxiter], betas[maxiter]
 * are host buffers; *niters = len(residuals)-1.  maxiter = 0 is legal: one
 * residual, d_x untouched.
 * MAMG_ERR_BREAKDOWN (mamg_last_error tells the three apart) leaves:
 *   "Matrix is not positive" (<r0,Br0> < 0 at the start, cbc.block's
 *     ValueError): *niters = 0, residuals[0] = 0.0, alphas / betas and every
 *     other entry of residuals not written, d_x untouched (bitwise x0);
 *   "ConjGrad breakdown (<r,Br> < 0)" in iteration k: *niters = k, the k + 1
 *     residuals and k alphas / betas of the completed iterations (the negative
 *     <r,Br> and the alpha of the broken iteration are not recorded), d_x =
 *     (x_k + alpha d) - alpha d: the iterate of the last completed iteration
 *     restored as cbc.block restores it, equal to x_k to round-off of the
 *     step, not bitwise (k = 0: x0 to round-off);
 *   "ConjGrad stopped: <d,Ad> = 0" in iteration k: *niters = k, histories as
 *     above, d_x = x_k bitwise (the x update had not run). */
int mamg_pcg_device(mamg_handle* h, const double* d_b, double* d_x, double tol,
                    int maxiter, int relativeconv, double* residuals,
                    double* alphas, double* betas, int* niters, void* stream);

/* Timing hook for bench/profiling: run `reps` applies eagerly (kernel by
 * kernel, no graph) on `stream`, timed with HIP events recorded on that
 * stream.  *ms_per_apply = mean wall time per apply.  kernel_ms[16] (if
 * non-NULL) = mean ms per apply per kernel class:
 * mode 0 instruments only classes 0 and 1 (the level-0 residual SpMV and the
 * level-0 post-smoothing / fused prolongation kernel, the two dominant
 * kernels), mode 1 instruments every launch.  class_bytes[16] (if non-NULL) =
 * algorithmic HBM bytes per apply of each class. */
int mamg_time_apply(mamg_handle* h, const double* d_r, double* d_z, int reps,
                    int mode, double* ms_per_apply, double* kernel_ms,
                    double* class_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MAMG_H */
