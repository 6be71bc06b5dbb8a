/*
 * spk.h -- C ABI of libspk.so: the MI355X-native replacement for what
 * KSPSolve() executes at /root/reference/src/SaddlePointProblem.c:70.
 *
 * The reference reaches its solver through six PETSc calls
 * (SaddlePointProblem.c:65-72):
 *     KSPCreate, KSPSetOperators(ksp,A,A), KSPSetFromOptions, KSPSetUp,
 *     KSPSolve(ksp,f,u), KSPDestroy.
 * Everything below KSPSolve (MatMult_*AIJ, PCApply_Jacobi,
 * PCApply_FieldSplit_Schur, KSPSolve_FGMRES, VecMDot/VecMAXPY/VecNorm,
 * VecScatter halo, MPI_Allreduce) runs inside PETSc.  This header is what a
 * PETSc plugin (PCSHELL / MATSHELL / KSPRegister'd type, see
 * plugin/spk_petsc.c and INTEGRATION.md) binds instead.  Plain C: opaque
 * context, raw CSR / vector pointers, sizes, int status.  No PETSc, no torch.
 *
 * Conventions
 *   - every function returns 0 on success, a negative SPK_ERR_* otherwise;
 *     spk_last_error() then holds a message.  Non-convergence is NOT an error:
 *     it is reported through spk_result.reason (PETSc KSPConvergedReason
 *     values), as KSPSolve does.
 *   - the caller owns every array it passes; the library copies at
 *     spk_set_block() and never keeps host pointers.  All device memory
 *     belongs to the context and is released by spk_destroy().
 *   - one context per KSP; no global state; a context is driven by one host
 *     thread at a time; every call is synchronous at return.
 *   - vectors are FP64.  A system vector is [u ; lambda]: the rank's n_local
 *     rows of the (0,0) block followed by ALL m constraint multipliers
 *     (replicated on every rank).  m = 0 when no constraint block is set.
 *   - `mem` arguments: SPK_MEM_HOST or SPK_MEM_DEVICE for the x/y/b pointers.  Device
 *     vectors must come from spk_vec_create (zero-padded to a whole 16-byte pair: the
 *     kernels read and write vectors two doubles at a time).
 */
#ifndef SPK_H
#define SPK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPK_VERSION 100

typedef struct spk_ctx spk_ctx;

enum { SPK_OK = 0, SPK_ERR_ARG = -1, SPK_ERR_HIP = -2, SPK_ERR_STATE = -3,
       SPK_ERR_COMM = -4, SPK_ERR_NOMEM = -5, SPK_ERR_UNSUPPORTED = -6 };

enum { SPK_MEM_HOST = 0, SPK_MEM_DEVICE = 1 };

/* Blocks of the nest K = [A00 A01; A10 0] sketched at
 * SaddlePointProblem.c:45-60 (MatGetSize/MatSetSizes(B, 4, nCols)).
 * A01 is always A10^T and is derived by the library. */
enum { SPK_BLOCK_A00 = 0, SPK_BLOCK_A10 = 1 };

/* -pc_type {none,jacobi,fieldsplit(schur)} as read by KSPSetFromOptions
 * (SaddlePointProblem.c:67). */
enum { SPK_PC_NONE = 0, SPK_PC_JACOBI = 1, SPK_PC_SCHUR = 2 };
/* -pc_fieldsplit_schur_fact_type */
enum { SPK_SCHUR_DIAG = 0, SPK_SCHUR_LOWER = 1, SPK_SCHUR_UPPER = 2, SPK_SCHUR_FULL = 3 };
/* -ksp_gmres_{classical,modified}gramschmidt */
enum { SPK_ORTHOG_CGS = 0, SPK_ORTHOG_MGS = 1 };
/* -ksp_gmres_cgs_refinement_type {never,ifneeded,always} */
enum { SPK_REFINE_NEVER = 0, SPK_REFINE_IFNEEDED = 1, SPK_REFINE_ALWAYS = 2 };
/* SpMV storage of the (0,0) block */
enum { SPK_SPMV_CSR = 0 };

/* KSPConvergedReason values (PETSc numbering). */
enum { SPK_CONVERGED_RTOL = 2, SPK_CONVERGED_ATOL = 3, SPK_CONVERGED_ITS = 4,
       SPK_CONVERGED_HAPPY_BREAKDOWN = 7, SPK_DIVERGED_NULL = -2,
       SPK_DIVERGED_ITS = -3, SPK_DIVERGED_DTOL = -4, SPK_DIVERGED_BREAKDOWN = -5,
       SPK_DIVERGED_INDEFINITE_PC = -8, SPK_DIVERGED_NANORINF = -9, SPK_DIVERGED_INDEFINITE_MAT = -10,
       SPK_ITERATING = 0 };

/* Solver options = the slice of the PETSc options database the reference
 * exposes through KSPSetFromOptions (SaddlePointProblem.c:67).  Fill with
 * spk_default_opts() first (PETSc defaults). */
typedef struct spk_opts {
    int32_t restart;        /* -ksp_gmres_restart            (30); 1..1022 -- restart + m <= 62: the fused iteration forms;
                               beyond: the head kernel stays, Gram-Schmidt runs in chunks of 40 vectors and the
                               Givens step is a launch of its own */
    int32_t max_it;         /* -ksp_max_it                   (10000) */
    double rtol;            /* -ksp_rtol                     (1e-5)  */
    double abstol;          /* -ksp_atol                     (1e-50) */
    double dtol;            /* -ksp_divtol                   (1e4)   */
    int32_t guess_nonzero;  /* -ksp_initial_guess_nonzero    (0)     */
    int32_t orthog;         /* SPK_ORTHOG_*                  (CGS)   */
    int32_t check_every;    /* host looks at the device convergence word every
                               this many iterations (a stream synchronisation each
                               time); 0 = once per restart cycle, without draining the
                               stream: the cycle's first kernel reports the state into
                               pinned memory and the host reads it while the cycle runs.
                               The iterate never depends on it.       */
    int32_t fused;          /* 1: fused PC+operator kernels where the PC allows,
                               0: PCApply and MatMult as separate steps */
    int32_t cgs_refine;     /* -ksp_gmres_cgs_refinement_type: SPK_REFINE_* (never) */
    int32_t single_reduce;  /* head-kernel paths with CGS only, OFF by default: 1 = h = V^T w, B D w and
                               w.w from ONE pass and ONE all-reduce per iteration; ||w'||^2 = w.w - |h|^2
                               and B D w' by recurrence.  Every scalar the next iteration's head needs
                               is then known before the update starts, so MAXPY, VecScale, PCApply
                               and the Givens step run as ONE launch: three launches per iteration
                               instead of four (1024^2: 227 -> 219 us, a 1/8 slab: 51 -> 45 us) and one
                               collective per iteration instead of two on many GPUs.  The price: the
                               subtraction cancels (||w'|| << ||w|| behind a good preconditioner):
                               measured 5e-6 relative drift of the residual history inside the
                               first cycle at 1024^2 (two-reduction path: 3e-11).  Safeguards: below
                               64 eps w.w the difference is kept at that floor (an over-estimated
                               ||w'|| over-estimates the residual), and a convergence seen by the
                               recurrence only ENDS THE CYCLE -- the solve ends when the true
                               residual computed at the restart confirms it, never on the
                               recurrence alone.  Needs restart + m <= 63 and restart <= 62
                               (falls back to two reductions otherwise). */
    int32_t iteration_form; /* how the head-kernel paths launch one classical Gram-Schmidt iteration (same
                               algorithm, two reductions, norms taken from w' itself):
                               SPK_ITER_AUTO (0): 6, 7 or SPK_ITER_UNNORM wherever it applies (classical Gram-Schmidt
                               without refinement, two reductions), else four launches;
                               SPK_ITER_UNNORM (5): three launches on an UN-NORMALISED basis -- VecMDot (raw inner
                               products and B D w~), VecMAXPY + norm + the next PCApply (+ B^T part), plain MatMult
                               carrying the Givens step in one extra workgroup.  V~_j = h_{j,j-1} v_j is stored with
                               a scale factor beside it and every consumer scales the scalars, never the vectors:
                               no VecScale traffic, either matrix format, any number of ranks;
                               SPK_ITER_FOUR_LAUNCH (1): head (VecScale + PCApply), SpMV, MDot, MAXPY; what every
                               form falls back to where it does not apply (MGS, CGS refinement, single reduction,
                               restart + m beyond 62);
                               SPK_ITER_RESIDENT (6; what AUTO takes on small single-rank systems: <= 512 block rows per
                               compute unit, restart <= 30, the row-type matrix layout): ONE launch per restart cycle, one
                               workgroup per CU, every thread keeps its entries of the un-normalised basis in registers --
                               VecMDot is a register dot product + an all-to-all of the partial sums (every workgroup adds
                               all of them in one order and runs the Hessenberg / Givens / convergence scalars itself),
                               VecMAXPY touches no memory, the product gathers z~ from the neighbours' write-through
                               stores.  Same algorithm and basis as 5.  SPK_RESIDENT=0 keeps AUTO on 5;
                               SPK_ITER_GS_FUSED (7; what AUTO takes on one rank with >= 1 M local rows where form 6
                               does not fit): form 5 with VecMDot and the VecMAXPY + PCApply pass in ONE launch (every
                               iteration of a cycle but its last), the MDot totals handed over inside the launch: the
                               first MAXPY loads are in flight while they are summed.  Same tiles and summation orders
                               as 5: the same bits.  Needs restart + m <= 41 and every workgroup resident at once.
                               SPK_ITER_TWO_LAUNCH, SPK_ITER_THREE_LAUNCH, SPK_ITER_BA (2, 3, 4): retired aliases of
                               5 (same algorithm; spk_get_iteration_form reports what ran).
                               Measured us per iteration, forms 1 / 5: 1/8 slab of 1024^2 47.9 / 43.3,
                               512^2 71.8 / 66.0, 1024^2 219.7 / 209.2. */
    int32_t basis_precision; /* -spk_basis_precision: how the Krylov basis V is STORED (the arithmetic is FP64 either way):
                               SPK_BASIS_DOUBLE (0, default) | SPK_BASIS_SINGLE (1): a compressed basis -- the un-normalised
                               vectors V~_j are kept as float(w') with their FP64 scale factor beside them, half the bytes
                               of the two Gram-Schmidt passes and of the basis itself; w~, z~, c~ and Z~ stay FP64.  Runs
                               form 5 only (AUTO, 6, 7 resolve to 5) on one rank; everything that is not form 5 (MGS, CGS
                               refinement, single_reduce, fused = 0, restart + 2 m > 62, an odd local size, V-cycles, FP32
                               inner sweeps, a dense Schur complement, Schur DIAG / UPPER, no PC, several ranks) is refused with SPK_ERR_UNSUPPORTED
                               before anything is enqueued.  Two rules keep the answer honest: a convergence or max_it seen
                               by the recurrence only ends the cycle, the true residual at the restart decides; and a
                               cycle also ends once the recurrence residual is <= 2^-20 of the cycle's starting residual
                               (below that the stored vectors carry rounding noise only).  spk_get_basis_info reports
                               what ran. */
} spk_opts;
enum { SPK_BASIS_DOUBLE = 0, SPK_BASIS_SINGLE = 1 };
enum { SPK_ITER_AUTO = 0, SPK_ITER_FOUR_LAUNCH = 1,
       SPK_ITER_TWO_LAUNCH = 2, SPK_ITER_THREE_LAUNCH = 3, SPK_ITER_BA = 4,   /* retired: run as SPK_ITER_UNNORM */
       SPK_ITER_UNNORM = 5, SPK_ITER_RESIDENT = 6, SPK_ITER_GS_FUSED = 7,
       SPK_ITER_LAST = 7 };

typedef struct spk_result {
    int32_t its;            /* KSPGetIterationNumber   */
    int32_t reason;         /* KSPGetConvergedReason   */
    double rnorm;           /* KSPGetResidualNorm (unpreconditioned estimate) */
    double rnorm0;          /* residual norm at iteration 0 */
    int32_t hist_len;       /* entries written to history[] */
    int32_t cycles;         /* restart cycles executed */
    double solve_seconds;   /* wall time inside spk_fgmres / spk_minres / spk_pipecg, upload excluded */
} spk_result;

/* ---- lifetime (KSPCreate / KSPDestroy, SaddlePointProblem.c:65,72) ------- */
int spk_create(spk_ctx **ctx, int device);
int spk_destroy(spk_ctx *ctx);
/* Message of the last failure on ctx (ctx may be NULL: last spk_create error). */
const char *spk_last_error(const spk_ctx *ctx);
int spk_version(void);
void spk_default_opts(spk_opts *opts);

/* ---- multi-GPU wiring (replaces PETSC_COMM_WORLD, SaddlePointProblem.c:65) */
/* One process per GPU: rank 0 calls spk_comm_unique_id, the host side
 * broadcasts the 128 bytes (MPI_Bcast in a PETSc plugin, torch.distributed in
 * bench.py), every rank calls spk_comm_init_rccl before spk_set_block. */
int spk_comm_unique_id(void *id128);
int spk_comm_init_rccl(spk_ctx *ctx, int rank, int nranks, const void *id128);
/* Host-callback transport (rehearsal only: lets N processes share ONE GPU, which RCCL
 * refuses, so that the multi-process flow of bench.py can be run on a 1-GPU box over
 * gloo/MPI).  Every collective is staged through the host and synchronises the stream.
 *   allreduce(user, buf, count): in-place sum over ranks of `count` doubles
 *   exchange(user, peer, send, nsend, recv, nrecv): one matched send/recv pair of doubles
 *   allgather(user, in, out, bytes_each): bytes from every rank, rank order */
typedef struct spk_host_comm {
    void *user;
    int (*allreduce)(void *user, double *buf, int count);
    int (*exchange)(void *user, int peer, const double *send, int64_t nsend, double *recv, int64_t nrecv);
    int (*allgather)(void *user, const void *in, void *out, int64_t bytes_each);
} spk_host_comm;
int spk_comm_init_host(spk_ctx *ctx, int rank, int nranks, const spk_host_comm *cb);
/* Peer-store collectives (call after spk_comm_init_*, before spk_set_block; collective over the
 * ranks).  The Krylov all-reduces (<= 64 doubles) and the halo rows are then written by the solver's
 * own kernels straight into windows of the peers' HBM over xGMI -- 8-byte {sequence, payload}
 * granules that are their own arrival flags: one network traversal, no RCCL launch, and where the
 * kernel allows it no launch at all (the all-reduce rides in the finish of the reducing kernel).
 * Sums are formed in rank order on every rank: all ranks hold the same bits.  The windows are
 * uncached device memory shared through HIP IPC; the communicator set before stays in place for
 * set-up traffic and as the fallback.  *enabled = 1 when every rank mapped every window and a
 * self-test all-reduce gave the right sums everywhere, else 0 (the previous backend keeps
 * working; spk_comm_backend() tells which one is active).  2..8 ranks.  Device-side waits are
 * bounded (SPK_PEER_TIMEOUT_MS, default 30000): a rank that never arrives turns into SPK_ERR_COMM. */
int spk_comm_enable_peer(spk_ctx *ctx, int32_t *enabled);
/* "self" | "rccl" | "host-callback" | "local" | "peer-store" */
const char *spk_comm_backend(const spk_ctx *ctx);
/* Diagnostics of the communicator, per rank (bench.py gathers them to rank 0 so that an N-GPU run
 * explains itself): which backend is active and why the peer-store backend stayed off if it did,
 * which kind of window memory passed the self-test, how many collectives went which way, and how
 * long the device waited inside them (100 MHz ticks, accumulated by one lane per collective). */
typedef struct spk_comm_info {
    int32_t rank, nranks;
    int32_t peer_enabled;        /* 1: peer-store collectives active */
    int32_t window_tier;         /* 0 uncached, 1 fine-grained, 2 plain device memory, -1 none */
    int32_t self_test_ok;        /* all-reduce self-test passed on every rank */
    int32_t halo_mode;           /* 0 none, 1 granules, 2 bulk chunks, 3 inner backend (fallback) */
    int32_t halo_fused;          /* 1: the exchange rides inside the head kernels */
    int32_t device;
    int64_t n_allreduce_fused;   /* all-reduces executed in the finish of a reducing kernel */
    int64_t n_allreduce_kernel;  /* as stand-alone granule launches */
    int64_t n_allreduce_inner;   /* handed to the inner backend (RCCL / host) */
    int64_t n_halo_fused, n_halo_kernel, n_halo_inner;
    uint64_t wait_ticks[4];      /* [0] all-reduce after MDot, [1] after MAXPY, [2] stand-alone, [3] halo */
    uint64_t wait_count[4];
    char backend[32];
    char inner_backend[32];
    char why[256];               /* reason the peer-store backend is off / last set-up message */
} spk_comm_info;
int spk_comm_get_info(spk_ctx *ctx, spk_comm_info *info);
/* Test hook: a `nranks`-rank peer-store all-reduce played by `nranks` workgroups of one launch through
 * `nranks` windows that all live in this process (no IPC): exercises every lane of the window layout
 * (up to 8) on one device.  vals: nranks x count inputs; out: nranks x count results (identical rows). */
int spk_debug_peer_allreduce_loopback(spk_ctx *ctx, int nranks, int count, int rounds, const double *vals, double *out);
/* In-process logical ranks on one device (parity tests of the partitioned
 * algorithm on a 1-GPU box): a group is shared by `nranks` contexts, each
 * driven by its own host thread. */
typedef struct spk_local_group spk_local_group;
int spk_local_group_create(spk_local_group **grp, int nranks);
int spk_local_group_destroy(spk_local_group *grp);
int spk_comm_init_local(spk_ctx *ctx, spk_local_group *grp, int rank);

/* ---- operators (KSPSetOperators, SaddlePointProblem.c:66) ---------------- */
/* CSR rows [row_begin, row_begin+nrows_local) of a block with ncols_global
 * columns; colidx are GLOBAL column numbers, int32 (PetscInt), ascending or
 * not.  The library splits diagonal / off-rank columns and builds the halo
 * plan (what MatMPIAIJ + VecScatter do in the reference's PETSc).
 *   A00: the rank's row slab of A; rows must tile [0,n) in rank order.
 *   A10: ALL m rows of B restricted to the rank's owned columns
 *        (column-partitioned like the rows of A00); pass row_begin = 0,
 *        nrows_local = m. */
int spk_set_block(spk_ctx *ctx, int which, int64_t row_begin, int32_t nrows_local,
                  int64_t ncols_global, const int32_t *rowptr, const int32_t *colidx,
                  const double *val);

/* KSPSetOperators for A00 of the reference's own discretisation, assembled on the device: what
 * SpkAssembleOperator_Laplace[Kappa] (spk_assembly.h) + spk_set_block(SPK_BLOCK_A00) do, without the host arrays.
 * A kernel writes the rank's slab -- the rows spk_partition_slab(my, 2*mx, rank, nranks) deals it -- bit for bit as
 * the host assembler would, into device memory, and the chain of spk_set_block runs from there.  kappa: one
 * coefficient per element, (mx-1)*(my-1) values of the WHOLE grid, element e = ej*(mx-1) + ei, in host or device
 * memory (kappa_mem: SPK_MEM_HOST / SPK_MEM_DEVICE), or NULL for ones.  f_dev: n_local values of spk_vec_create
 * memory that receive the right-hand side (zero on Dirichlet rows with apply_bc), or NULL.
 * Refused with the previous operator left in place and usable, before anything large is allocated: mx or my < 2
 * and an entry of kappa that is not finite and > 0 (SPK_ERR_ARG); 2*mx*my or the slab's non-zeros beyond INT32_MAX
 * (SPK_ERR_UNSUPPORTED).  Collective like spk_set_block. */
int spk_set_block_laplace(spk_ctx *ctx, int mx, int my, const double *kappa, int kappa_mem,
                          int apply_bc, double *f_dev /* n_local values, spk_vec_create memory, or NULL */);
/* Test hook: the same kernels on rows [row_begin,row_end), the result copied to host arrays sized as for
 * SpkAssembleOperator_Laplace.  Touches nothing of the context's operator. */
int spk_assemble_laplace_csr(spk_ctx *ctx, int mx, int my, int64_t row_begin, int64_t row_end,
                             const double *kappa, int kappa_mem, int apply_bc,
                             int32_t *rowptr, int32_t *colidx, double *val, double *f);
/* The same for the 3-D generator of spk_assembly.h (Q1 hexahedra, dof 3, mx x my x mz nodes): what
 * SpkAssembleOperator_Laplace3D[Kappa] + spk_set_block(SPK_BLOCK_A00) do, without the host arrays.  The rank's slab is
 * the node planes spk_partition_slab(mz, 3*mx*my, rank, nranks) deals it.  kappa: one coefficient per hexahedron,
 * (mx-1)*(my-1)*(mz-1) values of the WHOLE grid, element e = (ek*(my-1) + ej)*(mx-1) + ei, host or device memory, or
 * NULL for ones.  f_dev as above.  Refused with the previous operator left in place and usable, before anything large
 * is allocated: a grid side < 2 and an entry of kappa that is not finite and > 0 (SPK_ERR_ARG); 3*mx*my*mz, the slab's
 * non-zeros or the launch grid beyond INT32_MAX (SPK_ERR_UNSUPPORTED).  Collective like spk_set_block. */
int spk_set_block_laplace3d(spk_ctx *ctx, int mx, int my, int mz, const double *kappa, int kappa_mem,
                            int apply_bc, double *f_dev /* n_local values, spk_vec_create memory, or NULL */);
/* Test hook: the same kernel on any range of whole node planes, the result copied to host arrays sized as for
 * SpkAssembleOperator_Laplace3D.  Touches nothing of the context's operator. */
int spk_assemble_laplace3d_csr(spk_ctx *ctx, int mx, int my, int mz, int64_t row_begin, int64_t row_end,
                               const double *kappa, int kappa_mem, int apply_bc,
                               int32_t *rowptr, int32_t *colidx, double *val, double *f);
/* Wall seconds of the last device assembly's kernels up to a device synchronise (0 before one). */
int spk_get_assembly_seconds(const spk_ctx *ctx, double *seconds);

/* KSPSetOperators for A10 of the reference's own discretisation, written on the device: what
 * SpkAssembleOperator_Constraints[3D] (spk_assembly.h) + spk_set_block(SPK_BLOCK_A10) do, without the host arrays.
 * Kernels write the rank's column slice -- the columns of the rows A00 gave it -- as B by rows, B^T by rows and the
 * column-window pointers, bit for bit what the host chain uploads, and the rest of spk_set_block's chain runs from
 * there.  mz == 0: the 2-D block of 4 rows over the mx x my grid, else the 3-D block of 6 rows.  g_dev: m values of
 * spk_vec_create memory that receive SpkAssembleRHS_Constraints[3D], or NULL.
 * Refused with the previous B left in place and usable: no A00 yet (SPK_ERR_STATE); a grid side < 3, dof*mx*my[*mz]
 * that is not A00's n_global, rows of the rank that are not whole node lines (2-D) or planes (3-D) (SPK_ERR_ARG).
 * Collective like spk_set_block.  A caller's own B still goes through spk_set_block. */
int spk_set_block_constraints(spk_ctx *ctx, int mx, int my, int mz /* 0: the 2-D block */,
                              double *g_dev /* m values of spk_vec_create memory, or NULL */);
/* Test hook: the same kernels on the columns [row_begin,row_end) of any slab of whole node lines / planes, copied to host
 * arrays.  nnz = SpkConstraintsSlabNnz[3D]: b_colidx, b_val (B by rows, m rows of nnz / m entries each, localised
 * columns), bt_colidx, bt_val; bt_rowptr: row_end - row_begin + 1; win, nwin: the window width and count; winptr:
 * (nwin + 1) * m values, refused (SPK_ERR_ARG) beyond winptr_cap.  Touches nothing of the context's operator. */
int spk_assemble_constraints_csr(spk_ctx *ctx, int mx, int my, int mz, int64_t row_begin, int64_t row_end,
                                 int32_t *b_colidx, double *b_val, int32_t *bt_rowptr, int32_t *bt_colidx, double *bt_val,
                                 int32_t *win, int32_t *nwin, int32_t *winptr, int64_t winptr_cap);
/* The same arrays by the host chain of spk_set_block(SPK_BLOCK_A10) over the generator's block: the reference of the
 * hook above.  Needs neither a context nor a GPU. */
int spk_host_constraints_csr(int mx, int my, int mz, int64_t row_begin, int64_t row_end,
                             int32_t *b_colidx, double *b_val, int32_t *bt_rowptr, int32_t *bt_colidx, double *bt_val,
                             int32_t *win, int32_t *nwin, int32_t *winptr, int64_t winptr_cap);
/* Wall seconds of the last spk_set_block_constraints' kernels up to a device synchronise (0 before one). */
int spk_get_constraints_seconds(const spk_ctx *ctx, double *seconds);

/* ---- preconditioner (KSPSetUp, SaddlePointProblem.c:68) ------------------ */
/* Builds diag(A)^-1 and, for SPK_PC_SCHUR, S^ = diag(B diag(A)^-1 B^T). */
int spk_pc_setup(spk_ctx *ctx, int pc_type, int schur_fact);
/* Inner solve standing for A^-1 inside the preconditioner (BASELINE config 5: "mixed FP32
 * inner solve"; PETSc: -fieldsplit_0_ksp_type richardson -fieldsplit_0_ksp_max_it k
 * -fieldsplit_0_ksp_richardson_scale omega -fieldsplit_0_pc_type jacobi): `sweeps` damped-Jacobi
 * Richardson sweeps on A in SINGLE precision,
 *     y_1 = omega D^-1 x ;  y_{s+1} = y_s + omega D^-1 (x - A y_s),
 * input and result converted from / to FP64 (the outer FGMRES is flexible, so an inexact,
 * lower-precision A^-1 is legitimate).  sweeps = 0 (default) keeps the plain diag(A)^-1.
 * Call before spk_pc_setup. */
int spk_pc_set_inner(spk_ctx *ctx, int sweeps, double omega);
/* Smoothed-aggregation algebraic multigrid standing for A^-1 (PETSc: -pc_type gamg on K = A, or
 * -fieldsplit_0_pc_type gamg inside the Schur fieldsplit).  One V-cycle per application: nu smoothing steps
 * (Chebyshev with Jacobi inside, or damped-Jacobi Richardson) before and after the coarse-grid correction,
 * R = P^T, the coarsest operator inverted exactly (dense, at most SPK_AMG_MAX_COARSE equations).  The hierarchy
 * is built at spk_pc_setup from the A00 block the context holds (Vanek's greedy three-phase aggregation over the
 * bs x bs node graph -- not PETSc's MIS coarsening; see DESIGN.md "Algebraic multigrid"): on the host and uploaded
 * (setup = SPK_AMG_SETUP_HOST, the default), or on the device from the context's CSR copy of A00
 * (SPK_AMG_SETUP_DEVICE: node graph, Lanczos, the sparse products and the transposes are kernels; only the greedy
 * aggregation and the dense coarse Cholesky stay on the host, so the aggregates and every pattern are the host's).
 * spk_pc_set_amg(ctx, &o) before spk_pc_setup switches it on, NULL switches it off; SPK_PC_JACOBI then means
 * M^-1 = one V-cycle on A (no B block), SPK_PC_SCHUR takes the V-cycle wherever it takes diag(A)^-1 (S^ stays
 * diag(B diag(A)^-1 B^T)).  spk_fgmres runs it on the step-by-step path (spk_get_iteration_form reports -1).
 * Out of scope, refused with SPK_ERR_UNSUPPORTED: more than one rank (at spk_pc_setup; the context stays usable),
 * spk_minres with it (spk_pipecg takes it on K = A), and FP32 inner sweeps beside it (spk_pc_set_inner > 0 and spk_pc_set_amg are exclusive). */
enum { SPK_AMG_CHEBYSHEV = 0, SPK_AMG_RICHARDSON = 1 };
enum { SPK_AMG_SETUP_HOST = 0, SPK_AMG_SETUP_DEVICE = 1 };
/* How a level is coarsened.  AGGREGATION: the smoothed aggregation above (PETSc: -pc_type gamg).  GRID (PETSc: -pc_type mg
 * -pc_mg_galerkin on a DMDA): the unknowns sit on an mx x my (x mz) node grid, bs per node, in natural ordering
 * row = ((k my + j) mx + i) bs + c; a direction of m nodes halves to (m + 1) / 2 while m is odd and >= 5 (the others
 * keep m: semi-coarsening), P_l = P_z (x) P_y (x) P_x (x) I_bs with linear interpolation (even fine index i -> coarse i / 2,
 * weight 1; odd i -> (i - 1) / 2 and (i + 1) / 2, weight 1/2 each), boundary nodes included; the coarse operators are the
 * same Galerkin products.  threshold and nsmooths are not read, there are no aggregates, SPK_AMG_TENTATIVE returns P.
 * A level built by the grid rule applies P and R in the V-cycle without reading them (SPK_AMG_TRANSFER_MATRIX_FREE:
 * every weight is a power of two, the sums run in ascending column order) or as stored CSR like gamg's (STORED).
 * Which sides halve (grid coarsening only).  ODD: the rule above -- a grid with an even side that is too large for the
 * dense coarse solve is refused.  ANY: an even side of m >= 4 nodes halves too, to m / 2 + 1: its coarse nodes are the
 * fine indices 0, 2, ..., m - 2 and m - 1 (the last fine element is itself a coarse element, so the coarse Q1 space stays
 * nested); fine index i < m - 1 has the parents of the odd rule, fine index m - 1 the one parent m / 2 with weight 1.
 * Odd sides halve as under ODD, sides of 2 and 3 nodes never do: 1024 -> 513 -> 257 -> ... -> 5. */
enum { SPK_AMG_COARSEN_AGGREGATION = 0, SPK_AMG_COARSEN_GRID = 1 };
enum { SPK_AMG_TRANSFER_MATRIX_FREE = 0, SPK_AMG_TRANSFER_STORED = 1 };
enum { SPK_AMG_SIDES_ODD = 0, SPK_AMG_SIDES_ANY = 1 };
/* What forms the coarse operators of a grid-coarsened hierarchy (grid coarsening only; both give A_{l+1} =
 * (P^T A_l P + (P^T A_l P)^T) / 2 up to the rounding of their sums).  PRODUCTS (the default): the generic sparse products
 * and transposes gamg uses, on any level-0 pattern.  STENCIL: a gather on the node grid, with every pattern in closed form.
 *   Children.  In a halved direction of m fine nodes coarse index c sits at fine index 2c; under SPK_AMG_SIDES_ANY with m
 *   even the last coarse index m / 2 sits at fine m - 1.  Its children are fine 2c - 1 (weight 1/2), 2c (1) and 2c + 1
 *   (1/2), clipped to the line; fine m - 1 of an even halved side is the child of m / 2 alone, with weight 1.  A direction
 *   that keeps its nodes is the identity.  ch(C) is the tensor product, w(f, C) the product of the weights (1 .. 1/8):
 *   exactly the non-zeros of column C of P.
 *   The sum.  For coarse row r = C bs + a and column c = C' bs + b, C' within one node of C in every direction,
 *     S[r, c] = sum (w(f, C) w(f', C')) A_l[f bs + a, f' bs + b]
 *   over f in ch(C) in ascending node index and, within a fine row, over its stored entries in ascending position whose
 *   column node f' lies in ch(C'); plain additions from +0.0, entries A_l does not store count as zero.  Every product is
 *   exact, so host and device agree byte for byte.  A_{l+1}[r, c] = 0.5 S[r, c] + 0.5 S[c, r]: bitwise symmetric.
 *   The pattern.  Every coarse node row stores the full bs x bs blocks of its clipped 3^d-node neighbourhood in ascending
 *   column order, zeros included; nnz of a level is bs^2 prod (3 n_a - 2) over its sides n_a.
 *   Level 0 is the only level with a foreign pattern: every stored entry's column node must lie within one node of its
 *   row's node in every direction (a 5-point operator qualifies).  Otherwise spk_pc_setup / spk_amg_build_host fail with
 *   SPK_ERR_UNSUPPORTED, the message naming the row and column and `-spk_mg_galerkin products`; the context stays usable.
 *   Host and device levels being the same bytes, the device set-up takes the Ritz values of a level >= 1 of at most
 *   SPK_AMG_MAX_COARSE rows from the host's Lanczos on a download of it: lambda_max there is the host's to the bit. */
enum { SPK_AMG_GALERKIN_PRODUCTS = 0, SPK_AMG_GALERKIN_STENCIL = 1 };
/* How the cycle applies the operators of the levels between level 0 and the coarsest one (it steers the application, not
 * the hierarchy: a set-up that differs in it alone may refresh, and the hierarchy's bytes are those of CSR).  CSR (the
 * default): as sparse matrices -- row pointers, column indices, eight lanes per row and a butterfly.  STENCIL: every level
 * l with 1 <= l < levels - 1 applies A_l from its value array alone, in the residual product of the DOWN step and in the
 * fused smoothing step out = y + alpha D^-1 (b - A_l y) + beta (y - y-): the pattern of such a level is the closed form of
 * SPK_AMG_GALERKIN_STENCIL, so the row pointers and column indices carry no information and are not read (they stay
 * allocated -- the device Lanczos, the hooks and the stored transfers use them -- so device memory is unchanged; the value
 * array is the one the CSR level owns, no copy, no repack).  A row's sum runs over its stored entries in ascending position
 * from the first product, every product rounded on its own, one row per thread: not the bits of the CSR route (eight
 * strided partial sums), the same on every run, and the same in the fused tail as in the launches.  Level 0 keeps the
 * context's layout, the coarsest level its dense inverse.  Needs coarsening = GRID and galerkin = STENCIL -- only that
 * route guarantees the pattern on both set-up routes; otherwise spk_pc_set_amg / spk_amg_build_host fail with
 * SPK_ERR_UNSUPPORTED naming `-spk_mg_galerkin stencil` (or `-pc_type mg` under aggregation) and nothing changes. */
enum { SPK_AMG_OPERATOR_CSR = 0, SPK_AMG_OPERATOR_STENCIL = 1 };
/* Who holds the scalars of the device set-up's Lanczos (SPK_AMG_SETUP_DEVICE only; the tridiagonal, lambda_max and with
 * them every byte of the hierarchy are the same under both).  STEPWISE (the default): the host reads the two sums of every
 * step back -- it passes them to the next launch and keeps the break rule: 1 + 2 steps drained read-backs per level.
 * RESIDENT: the sums stay in a small block on the device; the workgroup that finishes a sum applies the host loop's rule
 * to it (the square root correctly rounded, the same break test), the next launch loads what it needs from the block, and a
 * launch after the break returns at once.  All 30 steps of a level are enqueued without a synchronise and the host reads
 * the block back once per level.  The sums are reduced by the same finish in the same launch geometry, so their bits are
 * the stepwise route's.  RESIDENT with setup = SPK_AMG_SETUP_HOST: spk_pc_set_amg fails with SPK_ERR_UNSUPPORTED naming
 * `-spk_gamg_setup device` and nothing changes; spk_amg_build_host range-checks the field and does not read it. */
enum { SPK_AMG_LANCZOS_STEPWISE = 0, SPK_AMG_LANCZOS_RESIDENT = 1 };
/* The precision of the levels >= 1 in the cycle (it steers the application, not the hierarchy: a set-up that differs in it
 * alone may refresh).  DOUBLE (the default): everything FP64.  SINGLE: the cycle runs every level l >= 1 in FP32.
 *   What stays FP64.  The hierarchy, byte for byte: the set-up, the Galerkin gather, the Lanczos, lambda_max, what
 *   spk_get_amg_level returns and the refresh are untouched.  Level 0 keeps the context's layout and its FP64 vectors.
 *   FP32 copies, made behind every build and every refresh: the value array of every level >= 1, its D^-1 (the FP64 D^-1
 *   rounded, not recomputed), its Chebyshev / Richardson coefficients and the coarsest level's dense inverse -- every
 *   conversion one round-to-nearest.  The cycle vectors of the levels >= 1 are float.  The FP64 value arrays stay (the
 *   refresh and the hooks read them): device memory grows by 4 B per stored entry of the levels >= 1 and shrinks by 4 B per
 *   entry of their vectors.
 *   Arithmetic.  On the levels >= 1 all of it is FP32: the expressions of the FP64 route in its order (the row sums of
 *   SPK_AMG_OPERATOR_STENCIL, the step, the transfers, the lane-strided sums and the butterfly of the dense product),
 *   every product and every addition rounded on its own -- the same bits on every run, and in the fused tail (which
 *   never holds level 0) the bits of the launches.
 *   The boundary.  DOWN on level 0 computes R (b - A y) in FP64 as under DOUBLE and rounds each result once to float
 *   on the store; UP on level 0 widens each entry of the correction to double, which is exact, and adds in FP64 as
 *   under DOUBLE.  The transfer weights are powers of two: between FP32 levels the transfers keep their stated order of
 *   additions and nothing else.
 *   No scaling.  Nothing rescales the restricted residual: an input whose restricted residual leaves FP32's normal range
 *   (below 1.2e-38 or above 3.4e38 in magnitude) loses accuracy or overflows; scale such a system first.  Inside the normal
 *   range a scaling of the input by a power of two scales the output by it, bit for bit.  Below it the FP32 kernels
 *   underflow gradually (IEEE subnormals, nothing is flushed to zero: the code objects are built with FP32 denormals on,
 *   the compiler's default for gfx950), so accuracy is lost bit by bit down to 1.4e-45 and not at once.
 *   The rounded cycle is not an exactly symmetric linear operator: spk_pipecg / spk_pipecgrr refuse a context whose
 *   hierarchy was built with SINGLE (SPK_ERR_UNSUPPORTED, the message pointing to -ksp_type fgmres), as they and
 *   spk_minres refuse the FP32 inner sweeps; FGMRES is flexible and takes it.
 *   Needs coarsening = GRID, galerkin = STENCIL, op = STENCIL and transfer = MATRIX_FREE -- on that route no kernel of
 *   a level >= 1 reads an index array; otherwise spk_pc_set_amg fails with SPK_ERR_UNSUPPORTED naming the missing one
 *   (`-pc_type mg`, `-spk_mg_galerkin stencil`, `-spk_mg_operator stencil`, `-spk_mg_transfer matrixfree`) and nothing
 *   changes.  spk_amg_build_host range-checks the field and does not read it. */
enum { SPK_AMG_PRECISION_DOUBLE = 0, SPK_AMG_PRECISION_SINGLE = 1 };
/* The cycle of one application (it steers the application, not the hierarchy: a set-up that differs in cycle, tail,
 * tail_rows, op and precision alone may refresh).  V: every level once.  W: the textbook recursion with two visits of the next level,
 *     cycle(l, fresh): l == L-1: COARSE; return
 *                      fresh ? PRE0 : PRE;  DOWN;  cycle(l+1, true);  if W and l+1 < L-1: cycle(l+1, false);  UP;  POST
 * (PETSc's PCMGMCycle): level l < L-1 is entered 2^l times, the coarsest 2^(L-2) times (a repeated exact solve changes
 * nothing).  PRE0: nu smoothing steps from the zero guess, PRE: nu steps from the level's own iterate (the second visit),
 * DOWN: b_{l+1} = R_l (b_l - A_l y_l), COARSE: y = A_L^-1 b, UP: y_l += P_l y_{l+1}, POST: nu steps from y_l.  Same smoother
 * before and after, R = P^T and an exact coarse solve keep the W-cycle symmetric, like the V-cycle.
 * The tail: the coarse levels l >= tail_first >= 1 -- those whose every level has at most tail_rows rows -- run as one
 * workgroup in one launch per tail run (a maximal stretch of consecutive steps on those levels), with a workgroup barrier
 * where the launches have a kernel boundary; the bits are those of the launches.  LAUNCHES: every step a launch of its own
 * (no tail).  AUTO: LAUNCHES under V, FUSED under W.  tail_rows 0: the library's default (SPK_AMG_TAIL_ROWS_DEFAULT). */
enum { SPK_AMG_CYCLE_V = 0, SPK_AMG_CYCLE_W = 1 };
enum { SPK_AMG_TAIL_AUTO = 0, SPK_AMG_TAIL_LAUNCHES = 1, SPK_AMG_TAIL_FUSED = 2 };
enum { SPK_AMG_STEP_PRE0 = 0, SPK_AMG_STEP_PRE = 1, SPK_AMG_STEP_DOWN = 2, SPK_AMG_STEP_COARSE = 3, SPK_AMG_STEP_UP = 4,
       SPK_AMG_STEP_POST = 5 };
#define SPK_AMG_MAX_LEVELS 16
#define SPK_AMG_MAX_COARSE 1024
#define SPK_AMG_TAIL_ROWS_DEFAULT 1024   /* tail_rows = 0 (DESIGN.md "The cycle and the fused tail" has the sweep behind it) */
typedef struct spk_amg_opts {
    int32_t max_levels;       /* -pc_mg_levels                      (10; 1..SPK_AMG_MAX_LEVELS) */
    int32_t coarse_eq_limit;  /* -pc_gamg_coarse_eq_limit           (50)  */
    int32_t nsmooths;         /* -pc_gamg_agg_nsmooths              (1; 0 keeps the tentative prolongator) */
    int32_t smoother;         /* -mg_levels_ksp_type: SPK_AMG_*     (chebyshev) */
    double threshold;         /* -pc_gamg_threshold                 (0: every stored block is a strong connection) */
    int32_t smooth_its;       /* -mg_levels_ksp_max_it              (2) */
    int32_t block_size;       /* node size bs; 0 = detect 3, 2 or 1 from the pattern (0) */
    double esteig[4];         /* -mg_levels_ksp_chebyshev_esteig a,b,c,d (0,0.1,0,1.1): the Chebyshev interval is
                                 [a lmin + b lmax, c lmin + d lmax], lmin / lmax the extreme Ritz values of D^-1 A_l */
    double richardson_scale;  /* -mg_levels_ksp_richardson_scale    (1.0) */
    int32_t setup;            /* -spk_gamg_setup host|device: SPK_AMG_SETUP_* (host); spk_amg_build_host takes either
                                 and builds on the host */
    int32_t coarsening;       /* SPK_AMG_COARSEN_*                  (aggregation; -pc_type mg selects grid) */
    int32_t grid[3];          /* grid coarsening: nodes per side mx, my, mz (mz = 1 in 2-D); rows = bs mx my mz */
    int32_t transfer;         /* -spk_mg_transfer matrixfree|stored: SPK_AMG_TRANSFER_* (grid coarsening only) */
    int32_t sides;            /* -spk_mg_sides odd|any: SPK_AMG_SIDES_* (odd; grid coarsening only) */
    int32_t cycle;            /* -spk_mg_cycle v|w: SPK_AMG_CYCLE_*  (v) */
    int32_t tail;             /* -spk_mg_tail auto|launches|fused: SPK_AMG_TAIL_* (auto: launches under v, fused under w) */
    int32_t tail_rows;        /* -spk_mg_tail_rows n: the largest level the fused tail takes (0: SPK_AMG_TAIL_ROWS_DEFAULT; else >= 1) */
    int32_t galerkin;         /* -spk_mg_galerkin products|stencil: SPK_AMG_GALERKIN_* (products; grid coarsening only) */
    int32_t op;               /* -spk_mg_operator csr|stencil: SPK_AMG_OPERATOR_* (csr; stencil needs grid coarsening and galerkin stencil) */
    int32_t lanczos;          /* -spk_amg_lanczos stepwise|resident: SPK_AMG_LANCZOS_* (stepwise; resident needs setup device) */
    int32_t precision;        /* -spk_mg_precision double|single: SPK_AMG_PRECISION_* (double; single needs grid coarsening,
                                 galerkin stencil, op stencil and matrix-free transfers) */
} spk_amg_opts;
void spk_default_amg_opts(spk_amg_opts *opts);
int spk_pc_set_amg(spk_ctx *ctx, const spk_amg_opts *opts);
typedef struct spk_amg_info {
    int32_t levels, block_size;
    int32_t rows[SPK_AMG_MAX_LEVELS];
    int64_t nnz[SPK_AMG_MAX_LEVELS];
    double lambda_max[SPK_AMG_MAX_LEVELS];   /* largest Ritz value of D^-1 A_l (the coarsest level: 0) */
    double operator_complexity;              /* sum of nnz(A_l) / nnz(A_0) */
    double setup_seconds;                    /* host build + upload; device build: its wall time up to a device synchronise */
    int32_t setup;                           /* where this hierarchy was built: SPK_AMG_SETUP_* */
    int32_t coarsening;                      /* SPK_AMG_COARSEN_* */
    int32_t dims[SPK_AMG_MAX_LEVELS][3];     /* grid coarsening: the node grid of every level (else 0) */
    int32_t sides;                           /* grid coarsening: SPK_AMG_SIDES_* of the rule that built it (else 0) */
    int32_t cycle;                           /* SPK_AMG_CYCLE_* of the application */
    int32_t tail_first;                      /* the first level inside the fused tail launch (>= 1), -1: no tail */
    int32_t tail_launches;                   /* launches of the tail kernel per application (0 without a tail) */
    int32_t galerkin;                        /* grid coarsening: SPK_AMG_GALERKIN_* of what built the coarse operators (else 0) */
    int32_t op;                              /* SPK_AMG_OPERATOR_* of the application: how the levels 1 .. levels - 2 apply A_l */
    int32_t lanczos;                         /* SPK_AMG_LANCZOS_* of the route the last build or refresh took (a host-built hierarchy: 0) */
    int32_t ritz_readbacks;                  /* device -> host reads the Ritz estimates of the last build or refresh made: a stepwise level
                                                1 + 2 steps, a resident level 1, a level whose Lanczos ran on a download of it 1; a
                                                host-built hierarchy 0 */
    int32_t precision;                       /* SPK_AMG_PRECISION_* of the application: what the levels >= 1 run in */
} spk_amg_info;
/* SPK_ERR_STATE unless spk_pc_setup built a hierarchy. */
int spk_get_amg_info(const spk_ctx *ctx, spk_amg_info *info);
/* Test hook: one matrix of a level as CSR (sorted columns).  which: SPK_AMG_OP = A_l, SPK_AMG_PROLONG = P_l (rows of
 * level l, columns of level l+1), SPK_AMG_TENTATIVE = the tentative prolongator of level l, SPK_AMG_COARSE_INV = the
 * dense inverse of the coarsest operator (level = levels - 1) as full rows.  Call with rowptr / colidx / val NULL first
 * for the sizes.  A device-built hierarchy is downloaded on demand, one matrix per call. */
enum { SPK_AMG_OP = 0, SPK_AMG_PROLONG = 1, SPK_AMG_TENTATIVE = 2, SPK_AMG_COARSE_INV = 3 };
int spk_get_amg_level(const spk_ctx *ctx, int level, int which, int32_t *nrows, int32_t *ncols, int64_t *nnz,
                      int32_t *rowptr, int32_t *colidx, double *val);
/* Test hook: the aggregate of every node of a level of the context's hierarchy (-1: isolated); agg NULL for the size.
 * SPK_ERR_UNSUPPORTED on a grid-coarsened hierarchy (it has none). */
int spk_get_amg_aggregates(const spk_ctx *ctx, int level, int32_t *nnodes, int32_t *agg);
/* Test hook: one transfer of level `level` (< levels - 1) of the context's hierarchy alone, on host vectors.
 * which 0: out = y + P e (e: the rows of level + 1, y and out: fine_len entries);  which 1: out = R (b - t) (b, t: fine_len
 * entries, out: the rows of level + 1).  stored 0: the matrix-free kernels (SPK_ERR_STATE unless the level was built by
 * the grid rule), 1: the CSR kernels on the stored P / R.  fine_len >= the rows of the level: the entries behind them
 * stand for a padded vector and come back untouched (which 0). */
int spk_debug_amg_transfer(spk_ctx *ctx, int level, int which, int stored, int64_t fine_len, const double *a, const double *b,
                           double *out);
/* Test hook: the operator of level `level` (1 <= level < levels - 1, else SPK_ERR_ARG) of the context's hierarchy alone, on
 * host vectors of the level's rows, one launch.  which 0: out = A x (b and xo are not read);  which 1: the smoothing step
 * out = x + alpha D^-1 (b - A x) + beta (x - xo) with the level's own D^-1 (xo NULL: the zero vector).  which 2 and 3: the
 * same two launches behind a set `done` gate: out comes back as it was passed in.  stencil 0: the CSR kernels, 1: the
 * value-array kernels of SPK_AMG_OPERATOR_STENCIL, whatever the context's option is (SPK_ERR_STATE unless the hierarchy
 * was built with grid coarsening and SPK_AMG_GALERKIN_STENCIL: the level has no closed-form pattern). */
int spk_debug_amg_operator(spk_ctx *ctx, int level, int which, int stencil, double alpha, double beta, const double *x,
                           const double *xo, const double *b, double *out);
/* The two hooks above on the FP32 kernels of SPK_AMG_PRECISION_SINGLE (SPK_ERR_STATE unless the hierarchy was built with
 * it), on float host vectors.  Operator: the value-array kernel on the level's FP32 copies, levels 1 .. levels - 2, `which`
 * as above.  Transfer: the matrix-free kernels; on a level >= 1 every vector is float (a, b: const float *, out: float *);
 * on level 0 the boundary forms: which 1 takes double a and b (fine_len entries) and gives a float out, which 0 takes a
 * float a (the correction e) and a double b and out (y, fine_len entries). */
int spk_debug_amg_operator_f32(spk_ctx *ctx, int level, int which, float alpha, float beta, const float *x, const float *xo,
                               const float *b, float *out);
int spk_debug_amg_transfer_f32(spk_ctx *ctx, int level, int which, int64_t fine_len, const void *a, const void *b, void *out);
/* Test hook: the Lanczos of the device set-up alone on level `level` (0 <= level < levels - 1, else SPK_ERR_ARG) of the
 * context's device-built hierarchy (SPK_ERR_STATE without one), on the unscaled operator.  resident 0: the stepwise route,
 * 1: the resident route, whatever the context's option is.  *steps: the steps taken (<= 30); al: 30 doubles, be: 31 doubles
 * (be[0] = 0), both filled up to *steps -- the tridiagonal whose extreme eigenvalues are the level's Ritz values. */
int spk_debug_amg_lanczos(spk_ctx *ctx, int level, int resident, int32_t *steps, double *al, double *be);
/* Reuse of the interpolation (PETSc: -pc_gamg_reuse_interpolation).  Sticky like spk_pc_set_schur_pre, default 0.  With
 * reuse on, a spk_pc_setup that finds a hierarchy an earlier set-up built with reuse on, the same spk_amg_opts (field by
 * field, route and block size included), the same local size and padded vector length, and a diagonal A00 block with the
 * pattern that hierarchy was built on REFRESHES it instead of building it: the aggregates, the tentative and the smoothed
 * prolongators, the restrictions and every sparsity pattern stay, bit for bit (the omega inside P_l is not revisited);
 * every A_{l+1} = ((R_l A_l P_l) + (R_l A_l P_l)^T) / 2, every D_l^-1, the Ritz values with the Chebyshev intervals and
 * coefficients, and the dense coarse inverse are computed again from the new values, on the route that built (host: the
 * host products and an upload of values; device: three kernels per level into buffers the build kept, in the build's
 * summation order -- unchanged values give the build's bits; an A00 multiplied by a power of two gives the build's
 * lambda_max to the bit and a V-cycle scaled by exactly its inverse: the Lanczos and the coarse Cholesky run on the
 * operator scaled back to the binade it was built in).  The case is a time step, a Newton step or a coefficient
 * sweep on a fixed mesh.  Anything else is a full build, silently.  To compare patterns the set-up keeps a device copy of
 * rowptr / colidx as the context stores them (about 150 MB at 1024 x 1024, bs 2; the same pattern in another column order
 * counts as different), and the device route the patterns and values of A_l P_l and R_l A_l P_l (not under
 * SPK_AMG_GALERKIN_STENCIL, whose refresh is the build's kernel on the new values); reuse = 0 releases
 * both and leaves the hierarchy.  A refresh fails where a build would (an empty Chebyshev interval, a coarse operator that
 * is not positive definite: SPK_ERR_ARG); the half-refreshed hierarchy is then dropped and the context is without a
 * preconditioner until the next spk_pc_setup, which builds.  Everything behind the hierarchy (diag(A)^-1, S^, the B D
 * planes, W / S / the factor of SPK_SCHUR_PRE_FULL) is set up behind a refresh as behind a build.  With reuse never
 * set, spk_pc_setup does what it did before this option existed. */
int spk_pc_set_amg_reuse(spk_ctx *ctx, int reuse);
/* *refreshed: 1 when the last spk_pc_setup refreshed the hierarchy, 0 when it built it; *seconds: the wall time of that
 * refresh or build (the pattern comparison and the pattern copy included), up to a device synchronise.  Either may be
 * NULL.  SPK_ERR_STATE without a hierarchy. */
int spk_get_amg_reuse_info(const spk_ctx *ctx, int32_t *refreshed, double *seconds);
/* Host-only builder (no GPU): the same hierarchy from a square CSR matrix, for tests.  agg: the aggregate of every
 * node of a level (-1: isolated, in no aggregate).  Errors: spk_last_error(NULL). */
typedef struct spk_amg_hier spk_amg_hier;
int spk_amg_build_host(int32_t n, const int32_t *rowptr, const int32_t *colidx, const double *val,
                       const spk_amg_opts *opts, spk_amg_hier **out);
/* The refresh of spk_pc_set_amg_reuse on a host hierarchy: val holds the new values of the same pattern, rowptr[n] of them
 * in the CSR order spk_amg_build_host was given -- the call has no length to check: passing that many is the caller's
 * part (AmgHierarchy.refresh of the Python package checks it); read the result through the spk_amg_host_* calls.  After a failure
 * (SPK_ERR_ARG, as from the build) the hierarchy is empty: only spk_amg_destroy_host remains. */
int spk_amg_refresh_host(spk_amg_hier *h, const double *val);
int spk_amg_destroy_host(spk_amg_hier *h);
int spk_amg_host_info(const spk_amg_hier *h, spk_amg_info *info);
int spk_amg_host_level(const spk_amg_hier *h, int level, int which, int32_t *nrows, int32_t *ncols, int64_t *nnz,
                       int32_t *rowptr, int32_t *colidx, double *val);
int spk_amg_host_aggregates(const spk_amg_hier *h, int level, int32_t *nnodes, int32_t *agg);
/* Test hook (host only): the steps of one cycle over `levels` levels (1..SPK_AMG_MAX_LEVELS) in the order both routes
 * run them, as pairs of int32 (SPK_AMG_STEP_*, level).  steps NULL: *nsteps alone. */
int spk_amg_cycle_steps(int32_t levels, int32_t cycle, int64_t *nsteps, int32_t *steps);
/* Test hook (host only): the children of coarse node `node` under SPK_AMG_GALERKIN_STENCIL between the node grids
 * fine[3] and coarse[3] -- the fine nodes in ascending order and their weights (at most 27 each; either may be NULL);
 * *n: how many.  They are the non-zeros of the node's column of P. */
int spk_amg_stencil_children(const int32_t *fine, const int32_t *coarse, int32_t node, int32_t *n, int32_t *nodes, double *weights);

/* What stands for the Schur complement in SPK_PC_SCHUR (PETSc: -pc_fieldsplit_schur_precondition):
 *   SPK_SCHUR_PRE_SELFP_DIAG (default): S^ = diag(B diag(A)^-1 B^T), divided by entry by entry;
 *   SPK_SCHUR_PRE_FULL: the exact complement S = B A^ ^-1 B^T of the A^ ^-1 the split applies -- the V-cycle itself with
 *     spk_pc_set_amg, diag(A)^-1 without -- as a dense m x m matrix, Cholesky-factored on the host at spk_pc_setup
 *     (PETSc: -pc_fieldsplit_schur_precondition full -fieldsplit_1_pc_type cholesky).  The set-up also keeps the m dense
 *     columns W = A^ ^-1 B^T, so every factorisation applies A^ ^-1 ONCE:
 *         t = W^T x0 ;  DIAG y1 = S^-1 x1 ;  LOWER / FULL y1 = S^-1 (t - x1) ;  UPPER y1 = -S^-1 x1 ;
 *         y0 = A^ ^-1 x0  (DIAG, LOWER)  |  A^ ^-1 x0 - W y1  (UPPER, FULL).
 *     With FULL the application is the exact inverse of [A^ B^T; B 0].  spk_fgmres runs it on the step-by-step path,
 *     spk_minres (DIAG, diag(A)^-1) with the preconditioner as a step of its own.
 * Sticky like spk_pc_set_inner: call before spk_pc_setup; no effect unless pc_type is SPK_PC_SCHUR.  Refused at
 * spk_pc_setup with SPK_ERR_UNSUPPORTED (the context stays usable): more than 8 constraint rows, more than one rank,
 * FP32 inner sweeps beside it (not a linear operator in FP64), and an S that is not positive definite (rank-deficient B). */
enum { SPK_SCHUR_PRE_SELFP_DIAG = 0, SPK_SCHUR_PRE_FULL = 1 };
int spk_pc_set_schur_pre(spk_ctx *ctx, int pre);
/* Copies the dense S (symmetrised, as it was factored) to the host; SPK_ERR_STATE unless the last spk_pc_setup built one. */
int spk_get_schur_matrix(spk_ctx *ctx, double *S /* m*m, row-major */);
/* Wall seconds the last spk_pc_setup spent on W, S and the factor (0 without a dense S).  For measurements. */
int spk_get_schur_setup_seconds(const spk_ctx *ctx, double *seconds);

/* Copies S^ (m doubles) to the host, for inspection. */
int spk_get_schur_diag(spk_ctx *ctx, double *shat);
int spk_get_jacobi_diag(spk_ctx *ctx, double *dinv /* n_local */);
/* Dense planes of B diag(A)^-1 the fused Schur kernels stream per pass: m, or m/2 when rows 2q / 2q+1
 * live on even / odd vector entries (x / y degrees of freedom of a dof-2 grid) and share a plane;
 * 0 when the fused path is not set up.  For byte models. */
int spk_get_bd_planes(const spk_ctx *ctx, int32_t *planes);
/* Which path the rows of the constraint block A10 take on this rank, as the last set_block left it (reads the context,
 * launches nothing): *general = 1 for a block of more than 8 rows (short rows through the CSR stream kernel, its rows of
 * more than 8192 local entries -- at most 8 -- through the column-window kernel), 0 for the few-rows path (every row
 * through the window kernel); *m_wide = rows the window kernel takes and wide_rows[0 .. *m_wide) their row numbers,
 * ascending; *win, *nwin = width and count of the column windows (nwin = 0 without a window row); *bc_tiles, *bt_tiles =
 * workgroups of the stream kernel over the block by rows and over B^T (0 where that form is not tiled).  Any pointer may
 * be NULL.  For tests. */
int spk_get_constraint_layout(const spk_ctx *ctx, int32_t *general, int32_t *m_wide, int32_t wide_rows[8], int32_t *win,
                              int32_t *nwin, int32_t *bc_tiles, int32_t *bt_tiles);

/* ---- the three plug points ------------------------------------------------ */
/* MATSHELL:  y = K x.   PCSHELL: y = M^-1 x.   Lengths n_local + m. */
int spk_mult(spk_ctx *ctx, const double *x, double *y, int mem);
int spk_pc_apply(spk_ctx *ctx, const double *x, double *y, int mem);
/* KSP type: the whole KSPSolve (SaddlePointProblem.c:70) on the device.
 * b, x: n_local + m values.  history (may be NULL) receives the residual norm
 * per iteration, starting with iteration 0. */
int spk_fgmres(spk_ctx *ctx, const double *b, double *x, int mem, const spk_opts *opts,
               spk_result *result, double *history, int32_t history_cap);

/* KSP type minres: preconditioned MINRES (Paige-Saunders; Elman-Silvester-Wathen Alg. 4.1) on the device, for a
 * symmetric K and a symmetric positive definite M^-1: PC none, Jacobi (with or without B) and Schur DIAG (any
 * constraint block).  LOWER / UPPER / FULL (not symmetric) and FP32 inner sweeps (spk_pc_set_inner > 0) are refused
 * with SPK_ERR_UNSUPPORTED.  A short recurrence: no restart, twelve work vectors of its own (allocated on first use;
 * nothing of spk_fgmres's workspace or state is touched).  Per iteration: the product K z, one pass with the previous
 * iteration's lagged w / x (/ Kw / r) update and <K z, z>, one pass forming v_{j+1} and z_{j+1} = M^-1 v_{j+1}
 * (PC applied in the pass) with <z, v>; the scalar recurrence runs in the finishing workgroup of each pass (one rank)
 * or as a one-thread launch after the all-reduce.
 * norm_type: the norm of the convergence test (KSPConvergedDefault: ttol = max(rtol ||b||, abstol), divergence at
 * dtol ||b||, both in that norm):
 *   SPK_NORM_UNPRECONDITIONED: ||b - K x||, kept by recurrence (K w_j by recurrence too: no extra product);
 *   SPK_NORM_NATURAL: ||b - K x||_{M^-1} = |eta| of the recurrence (no r / K w streams).
 * A convergence (or -ksp_max_it) seen by the recurrence is confirmed on the true b - K x in the same norm; if that
 * misses ttol the recurrence restarts from the current x.  <z, v> < 0 ends the solve with
 * SPK_DIVERGED_INDEFINITE_PC (a reason, not an error); gamma_{j+1} = 0 with SPK_CONVERGED_HAPPY_BREAKDOWN.
 * opts: max_it, rtol, abstol, dtol, guess_nonzero, check_every (0: the host looks at the state once per chunk of
 * iterations while the next chunk is queued), fused (0: PCApply as a step of its own, same algorithm);
 * restart, orthog, cgs_refine, single_reduce and iteration_form are ignored.
 * history[0] = the initial residual norm, then one recurrence value per iteration; result.rnorm = the true norm
 * confirmed at the end; result.cycles = recurrence (re)starts. */
enum { SPK_NORM_UNPRECONDITIONED = 0, SPK_NORM_NATURAL = 1 };
int spk_minres(spk_ctx *ctx, const double *b, double *x, int mem, const spk_opts *opts, int norm_type,
               spk_result *result, double *history, int32_t history_cap);

/* KSP type pipecg: preconditioned pipelined CG (Ghysels-Vanroose 2014, Alg. 3; PETSc KSPPIPECG) on the device, for a
 * symmetric positive definite K = A (no constraint block: a context with one is refused with SPK_ERR_UNSUPPORTED, the
 * saddle matrix is indefinite -- use spk_minres) and PC none, Jacobi or the V-cycle (spk_pc_set_amg).  The Schur
 * preconditioners, FP32 inner sweeps and a V-cycle with FP32 levels (SPK_AMG_PRECISION_SINGLE: not exactly symmetric) are
 * refused with SPK_ERR_UNSUPPORTED.  A short recurrence with ONE reduction per
 * iteration whose scalars are ready a pass before they are needed: with none / Jacobi an iteration is the product n = K m
 * plus one pass that applies the eight updates (u = D r and q = D s formed in the pass, not stored), writes m = D w for
 * the next product and reduces [<r, u>, <w, u>, r.r]; the scalar step runs in the finishing workgroup of that pass (one
 * rank) or as a one-thread launch after the all-reduce, which goes behind the next product.  With the V-cycle,
 * m = M^-1 w runs before the product and u, q are recurrences.  Its own work vectors (allocated on first use; nothing of
 * spk_fgmres's or spk_minres's workspace or state is touched).
 * norm_type: SPK_NORM_UNPRECONDITIONED (||b - K x||) or SPK_NORM_NATURAL (sqrt(<r, M^-1 r>)), tested by
 * KSPConvergedDefault as in spk_minres.  A convergence (or -ksp_max_it) seen by the recurrence is confirmed on the true
 * b - K x; if that misses ttol the recurrence restarts from the current x (residual replacement), so result.rnorm is
 * always the true norm.  <r, M^-1 r> < 0 ends the solve with SPK_DIVERGED_INDEFINITE_PC, a non-positive step-length
 * denominator (delta - beta gamma / alpha_old) with SPK_DIVERGED_INDEFINITE_MAT (reasons, not errors).
 * opts: max_it, rtol, abstol, dtol, guess_nonzero, check_every, fused (0: PCApply as a launch of its own and the sums in
 * a second pass, same recurrence and summation order); restart, orthog, cgs_refine, single_reduce and iteration_form are
 * ignored.  history[0] = the initial residual norm, then one recurrence value per iteration; result.cycles =
 * recurrence (re)starts. */
int spk_pipecg(spk_ctx *ctx, const double *b, double *x, int mem, const spk_opts *opts, int norm_type,
               spk_result *result, double *history, int32_t history_cap);

/* KSP type pipecgrr: spk_pipecg with residual replacement (PETSc KSPPIPECGRR), same rules and refusals.  At the end of
 * every chunk of opts.check_every iterations (16 when 0) of a recurrence the device computes t = K x and the measured
 * gap ||(b - t) - r||; when it crosses tau ||r|| (above now, at or below at the check before in the recurrence) the
 * recurrence vectors are recomputed from their definitions: r = b - t, u = M^-1 r, w = K u, s = K p, q = M^-1 s,
 * z = K q, then gamma = <r, u>, delta = <w, u> and the next step lengths as after an iteration.  x, p and the scalar
 * history are kept: a replacement is neither an iteration nor a start (result.cycles) and keeps the Krylov space that a
 * restart throws away.  The check and the replacement are enqueued at every boundary and gated on the device (the
 * host does not wait); without a replacement the check costs one product and one pass per chunk.  tau:
 * spk_pipecgrr_set_tau (SPK_PIPECGRR_TAU_DEFAULT until set).  *replacements (may be null) = replacements run. */
#define SPK_PIPECGRR_TAU_DEFAULT 1e-6
int spk_pipecgrr(spk_ctx *ctx, const double *b, double *x, int mem, const spk_opts *opts, int norm_type,
                 spk_result *result, double *history, int32_t history_cap, int32_t *replacements);
/* tau of spk_pipecgrr on ctx: >= 0 and finite (0: a replacement at every crossing of a nonzero gap). */
int spk_pipecgrr_set_tau(spk_ctx *ctx, double tau);

/* How the LAST spk_fgmres on ctx launched its iterations: *form = the SPK_ITER_* actually run (AUTO resolved; options
 * the chosen form does not cover fall back, see spk_opts.iteration_form), or -1 for the step-by-step path (PCApply and
 * MatMult as launches of their own: unfused preconditioners, FP32 inner sweeps, general constraint blocks; a restart
 * beyond 62, MGS or CGS refinement on a fusable preconditioner report SPK_ITER_FOUR_LAUNCH: the head kernel runs);
 * *single_reduce = 1 when the single-reduction mode ran.  For byte models (bench.py). */
int spk_get_iteration_form(const spk_ctx *ctx, int32_t *form, int32_t *single_reduce);
/* Form 7's launches of the LAST spk_fgmres on ctx (0 where another form ran): *launches = how many were enqueued,
 * *tail = how many of them staged a short remainder tile of VecMDot's pass in LDS instead of walking it as a tile of its
 * own (all of them or none: the vector length decides, and SPK_GS_TAIL=0 turns it off).  Either pointer may be NULL. */
int spk_get_gs_launch(const spk_ctx *ctx, int32_t *launches, int32_t *tail);
/* The basis of the last spk_fgmres on this context: SPK_BASIS_* it ran with and the bytes allocated for V (restart + 2
 * vectors of ld doubles, or restart + 1 vectors of ld floats; the two FP64 work vectors of a single-precision solve are
 * not part of it).  -1 and 0 before the first solve.  Either pointer may be NULL. */
int spk_get_basis_info(const spk_ctx *ctx, int32_t *precision, int64_t *basis_bytes);

/* ---- device vectors for callers that keep b/x resident in HBM --------------- */
/* (a PCSHELL/MATSHELL glue over device Vecs, bench.py).  Zero-filled, length
 * rounded up so that every kernel may read whole 16-byte pairs. */
int spk_vec_create(spk_ctx *ctx, int64_t n, double **dev);
int spk_vec_destroy(spk_ctx *ctx, double *dev);
int spk_vec_set(spk_ctx *ctx, double *dev, const double *host, int64_t n);
int spk_vec_get(spk_ctx *ctx, const double *dev, double *host, int64_t n);

/* ---- sizes ---------------------------------------------------------------- */
int spk_get_sizes(const spk_ctx *ctx, int64_t *n_global, int32_t *n_local, int32_t *m,
                  int64_t *nnz_local, int32_t *n_ghost);

/* Storage the A-block SpMV actually streams: format 0 = CSR (12 B per stored non-zero),
 * 1 = 2x2-blocked CSR (36 B per 4 non-zeros; chosen automatically when rows 2k, 2k+1 share
 * their pattern and columns pair up, as for a dof-2 DMDA; SPK_SPMV_FORMAT=csr forces CSR).
 * layout_bytes = bytes one SpMV reads and writes in that layout (matrix + x + y). */
int spk_get_spmv_info(const spk_ctx *ctx, int32_t *format, int64_t *layout_bytes);
/* Test hook: the row-type layout of the A block as set up. out[0..11] = ok, bs, nbrows, kmax, ntype, nclass, lds_bytes,
 * uniform, straddle, uniform3, product kernel (0 plain, 1 pipelined 2x2, 2 pipelined 3x3), chunks_per_wg.  ok = 0: the rest is 0. */
int spk_debug_dict_layout(const spk_ctx *ctx, int32_t out[12]);
/* Formats 3 / 4: ROW TYPES + DEVIATION CODES over the 2x2 / 3x3 blocks (the default wherever the layout exists).  On the
 * reference's uniform grid (Discretization.c:25; one element matrix for all elements, :293-332) the assembled entries
 * scatter by rounding noise around a handful of ideal values (:96-128: a Jacobian formed from coordinates): A holds a few
 * dozen block CLASSES (blocks equal up to that noise) in a few dozen ROW TYPES (sequences of (column offset, class)).
 * They are found in the caller's CSR at spk_set_block (hashing, then EVERY value decoded and compared bit for bit;
 * nothing is assumed about the grid).  Stored: two bytes of type per block row and per value an integer k with
 * value = base + k 2^g exactly, as a bit field of the width its class entry needs (one 64-bit word per 2x2 block, two
 * per 3x3 block) -- same products, same order, same bits as the CSR loop.  Matrices that do not fit keep formats 0..2;
 * SPK_SPMV_FORMAT=bcsr (or csr) switches the layout off, SPK_DICT_VERBOSE=1 reports what was found or why not.
 * Byte models of one product y = A x on this rank's diagonal block in the three layouts (0 where a layout does not
 * exist), and the layout's size (patterns = row types, blocks = block classes). */
int spk_get_spmv_models(const spk_ctx *ctx, int64_t *csr_bytes, int64_t *blocked_bytes, int64_t *dict_bytes,
                        int32_t *patterns, int32_t *blocks);

/* ---- single kernels through the ABI (parity tests, bench.py) -------------- */
/* h[i] = V_i . w  (i < nv), V given as nv vectors of length n with stride ldv
 * (VecMDot).  Host pointers. */
int spk_kernel_mdot(spk_ctx *ctx, int64_t n, int32_t nv, const double *V, int64_t ldv,
                    const double *w, double *h);
/* w += sum_i a[i] V_i   (VecMAXPY); returns ||w_new||^2 in *nrm2 if non-NULL. */
int spk_kernel_maxpy(spk_ctx *ctx, int64_t n, int32_t nv, const double *a, const double *V,
                     int64_t ldv, double *w, double *nrm2);
/* Times `reps` launches of the A-block SpMV kernel with HIP events on the
 * context's stream after `warmup` untimed launches; *ms_per_launch = average.
 * x is a deterministic fill sin(0.37 i). */
int spk_time_spmv(spk_ctx *ctx, int warmup, int reps, double *ms_per_launch);
/* Generic form for the other kernels of an iteration (tuning / profiles):
 * which = "spmv" | "spmv_bcsr" | "spmv_bcsr3" | "spmv_dict" | "spmv_acc" | "spmv_ride" | "spmv_gated" | "mult" | "pc" | "mdot" | "maxpy" | "maxpy_nonorm" | "scale" | "wide_dot" |
 * "bt_update"; nv = vectors for mdot/maxpy.  Needs operators (and pc_setup for
 * "pc"); allocates its own scratch vectors. */
int spk_time_kernel(spk_ctx *ctx, const char *which, int nv, int warmup, int reps,
                    double *ms_per_launch);

/* Test hook: launches a small cross-workgroup reduction in which one partial sum is never
 * published.  The reducer gives up after timeout_ms and raises the context's sticky execution-error
 * word; the call (like spk_fgmres / spk_mult when it happens inside them) returns SPK_ERR_HIP -- an
 * execution failure is never reported as a numerical reason (KSP_DIVERGED_NANORINF).  The context
 * re-arms its reduction buffer and stays usable. */
int spk_debug_finish_timeout(spk_ctx *ctx, int timeout_ms);

/* Test hook: one 512-thread workgroup takes the eight wave sums of each of na values (in[i * 512 + t]: value i of thread
 * t; na one of VecMDot's accumulator counts 9, 17, 25, 33, 41) with the one-value shuffle chain and with the multi-value
 * reduction of form 7's launch.  out[w * na + i]: wave w's sum of value i by the chain, out[8 * na + w * na + i] by the
 * multi-value reduction (16 na doubles).  The two halves must hold the same bits. */
int spk_debug_wave_sums(spk_ctx *ctx, int na, const double *in, double *out);

/* Test hooks for the Gram-Schmidt kernels (tests/test_gpu_vec_kernels.py): each takes host arrays, runs the PRODUCTION host
 * wrapper (k::mdot, k::maxpy, k::sqnorm_bd, k::pack_bd, k::fused_head) with every argument the solver passes, and copies the
 * results back.  Vectors are given densely (row i at V + i * n) and live on the device with stride ld = roundup(n, 256);
 * entries [n, ld) of every vector hold `pad`.  done: -1 passes a null pointer, 0 / 1 a device word holding that value.
 * Outputs a launch may leave alone are pre-filled with SPK_DEBUG_MARKER. */
#define SPK_DEBUG_MARKER (-7777777.0)
/* out (13 values): ws_shape {on, U, grid}, vec_shape(n2) {T, U, G, grid} and vec_shape(n2, maxpy) {T, U, G, grid} of a
 * vector of n entries, then the knobs SPK_VEC_WS16 and SPK_VEC_DEEP as this process reads them. */
int spk_debug_vec_shape(spk_ctx *ctx, int64_t n, int32_t *out);
typedef struct spk_debug_mdot_opts {
    int64_t n, n_dot;
    int32_t nv, nv2;   /* vectors of V; results of the second slab V2 (split: nv2 / 2 parity planes, else nv2 dense rows) */
    int32_t split, done;
    double pad;
} spk_debug_mdot_opts;
/* out: nv + nv2 + 1 values (the dot products, then w.w) */
int spk_debug_mdot(spk_ctx *ctx, const spk_debug_mdot_opts *o, const double *V, const double *V2, const double *w, double *out);
/* The same over an FP32 basis (k::mdot_f32, what a -spk_basis_precision single solve launches): V holds floats (stride ld
 * floats on the device), V2 and w stay FP64.  nv2 <= 8, nv + 2 nv2 <= 63.  out: nv + 2 nv2 + 1 values -- the dot products
 * with w, w.w, then the nv2 plane values of the LAST vector of V (B D of the newest basis vector as stored). */
int spk_debug_mdot_f32(spk_ctx *ctx, const spk_debug_mdot_opts *o, const float *V, const double *V2, const double *w, double *out);
typedef struct spk_debug_maxpy_opts {
    int64_t n, n_dot, n_bd;
    double sign, pad;
    int32_t nv, nv_live;   /* nv_live >= 0: a device word holding it is passed as nv_dev (nv is the larger host count) */
    int32_t want_norm;     /* 0: Finish::out = NULL */
    int32_t m, bd_mode;    /* bd_mode 0: no planes, 1: m dense rows, 2: m / 2 parity planes */
    int32_t w1side, pyth, done;
} spk_debug_maxpy_opts;
/* w: n entries in and out; bd: the planes (bd_mode rows of n); dots: nv_live + m + 1 reduced values and tb: (nv + 1) x 8,
 * in and out (pyth only); red: 1 + m reduced values; w1side: m; nrm_out: 1 + m (pyth only) */
int spk_debug_maxpy(spk_ctx *ctx, const spk_debug_maxpy_opts *o, const double *V, const double *a, double *w, const double *bd,
                    const double *dots, double *tb, double *red, double *w1side, double *nrm_out);
/* k::sqnorm_bd: x of n entries (sa, sb != NULL: x = sa - sb is formed, x is output only), m dense planes bd of n entries;
 * red: 1 + m, w1side: m */
int spk_debug_cycle_norm(spk_ctx *ctx, int64_t n, int64_t n_dot, int64_t n_bd, int32_t m, double pad, double *x, const double *sa,
                         const double *sb, const double *bd, double *red, double *w1side);
/* k::schur_w_dot / schur_w_y1 / schur_w_out as op_pc_apply chains them for one factorisation (fact: SPK_SCHUR_*): W: m planes
 * of nl entries, L: the Cholesky factor (m x m, lower), x: nl + m entries.  UPPER / FULL: y0 = s - W y1 with s = src (nl
 * entries), dinv .* x0 (dinv given) or x0.  y: the WHOLE padded output row, (nl + m) rounded up to 256 entries, filled
 * with SPK_DEBUG_MARKER before the launches (DIAG / LOWER leave y0 at the marker: their A^-1 x0 is not this file's). */
int spk_debug_schur_w(spk_ctx *ctx, int64_t nl, int32_t m, int32_t fact, int32_t done, double pad, const double *W, const double *L,
                      const double *x, const double *src, const double *dinv, double *y);
/* k::pack_bd: m dense rows of n entries -> m / 2 planes (bdp: (m / 2) x n) and the `bad` word */
int spk_debug_pack_bd(spk_ctx *ctx, int64_t n, int32_t m, const double *bd, double *bdp, int32_t *bad);
typedef struct spk_debug_head_opts {
    int64_t nl;            /* even */
    int32_t m, packed, fact, jacobi, want_wl, reserved;
    double pad;
} spk_debug_head_opts;
/* k::fused_head with loc_prev = -1, no SendRanges and a zero `done` word.  v: nl + m in and out; nrm: 1 + m; w1raw, shat: m;
 * dinv: nl; bd: m rows (packed: m / 2) of nl; gram: m x m; z, c: nl + m out (jacobi: c is not passed, m = 0); wl: m */
int spk_debug_cycle_head(spk_ctx *ctx, const spk_debug_head_opts *o, double *v, const double *nrm, const double *w1raw,
                         const double *dinv, const double *bd, const double *shat, const double *gram, double *z, double *c,
                         double *wl);

/* Developer hook (library built with `make GS_STAMPS=1`; SPK_ERR_STATE otherwise): the phase time stamps of form 7's fused
 * Gram-Schmidt launches of the solves so far, out[(loc * 256 + workgroup) * 8 + phase] in 100 MHz ticks of one device-wide
 * counter (64 x 256 x 8 values; per loc the last launch that ran; phases in csrc/spk_gs_stamps.hpp; 0: never written). */
int spk_debug_gs_stamps(spk_ctx *ctx, uint64_t *out);

/* Test hook: the bound of every device-side wait for another workgroup's data (cross-workgroup reductions, the resident
 * cycle kernel's exchanges) in 100 MHz ticks; 0 restores the default (4 s).  A bound of one tick makes the next solve fail
 * in the MIDDLE of a cycle with SPK_ERR_HIP -- what a lost workgroup would cause -- so that tests can check that the context
 * stays usable afterwards. */
int spk_debug_set_wait_bound(spk_ctx *ctx, uint32_t ticks);

/* Measurement hook (bench.py's roofline): with max_launches > 0 the next solves take the kernel's OWN start and stop time
 * stamps (hipExtLaunchKernelGGL) of each product launch of their ITERATIONS (y (+)= A x with the Givens rider in the
 * launch -- the kernel the roofline names) into a pair of HIP events on the solver's stream, up to max_launches of them; 0
 * switches it off.  spk_get_product_timing waits for the stream and returns their count and the mean / median / shortest /
 * longest duration in ms: the kernel as it runs inside a solve -- behind the MAXPY pass, with the caches in the state that
 * pass leaves -- not a batch of back-to-back repetitions; what `rocprofv3 --kernel-trace --stats` averages for it.
 * Launches shorter than half the median (gated off by the device: the iterations enqueued ahead of a solve's end) are left
 * out and reported apart (gated, gated_mean_ms).  (The resident form launches no product per iteration: count 0.) */
int spk_debug_time_products(spk_ctx *ctx, int32_t max_launches);
int spk_get_product_timing(spk_ctx *ctx, int32_t *launches, double *mean_ms, double *median_ms, double *min_ms, double *max_ms,
                           int32_t *gated, double *gated_mean_ms);

/* ---- host-only helpers: row-slab partition and halo plan ------------------ */
/* (callable without a GPU; used by the multi-rank CPU tests) */
/* Rows owned by `rank` of `nranks` when `nlines` grid lines of `line_rows`
 * rows each are dealt in contiguous slabs (PETSc's default DMDA split in y). */
int spk_partition_slab(int64_t nlines, int64_t line_rows, int rank, int nranks,
                       int64_t *row_begin, int64_t *row_end);
/* Splits a local CSR slab with global columns into the diagonal block (local
 * column numbers) and the off-diagonal block (ghost numbers 0..n_ghost-1,
 * ghosts sorted by global column) -- MatMPIAIJ's (Ad, Ao, garray).
 * Call once with the output arrays NULL to get the sizes. */
int spk_partition_split(int64_t row_begin, int32_t nrows_local, const int32_t *rowptr,
                        const int32_t *colidx, const double *val,
                        int32_t *d_rowptr, int32_t *d_colidx, double *d_val,
                        int32_t *o_rowptr, int32_t *o_colidx, double *o_val,
                        int32_t *garray, int64_t *nnz_d, int64_t *nnz_o, int32_t *n_ghost);

#ifdef __cplusplus
}
#endif
#endif /* SPK_H */
