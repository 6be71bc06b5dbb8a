/*
 * spk_ksp.h -- host-side mirror of the reference's solver call site.
 *
 * /root/reference/src/SaddlePointProblem.c:65-72 is
 *     KSPCreate(PETSC_COMM_WORLD,&ksp); KSPSetOperators(ksp,A,A);
 *     KSPSetFromOptions(ksp); KSPSetUp(ksp); KSPSolve(ksp,f,*u); KSPDestroy(&ksp);
 * The functions below keep those names (Spk prefix), argument meaning and
 * error behaviour (int error code, 0 = success, non-convergence is a reason,
 * not an error) on plain CSR arrays instead of Mat/Vec, and read the same
 * option names KSPSetFromOptions reads from the PETSc options database (:67).
 * They sit on top of the C ABI in spk.h; nothing here touches the GPU directly.
 */
#ifndef SPK_KSP_H
#define SPK_KSP_H
#include <stdint.h>
#include "spk.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct SpkKSP_s *SpkKSP;

/* A CSR row slab with GLOBAL column indices (what MatMPIAIJ rows look like);
 * single rank: row_begin = 0, nrows_local = ncols_global. */
typedef struct SpkMatCSR {
    int64_t row_begin;
    int32_t nrows_local;
    int32_t pad;
    int64_t ncols_global;
    const int32_t *rowptr, *colidx;
    const double *val;
} SpkMatCSR;

int SpkKSPCreate(int device, SpkKSP *ksp);                                 /* KSPCreate      :65 */
/* optional, before SetOperators: one process per GPU over RCCL */
int SpkKSPSetCommRCCL(SpkKSP ksp, int rank, int nranks, const void *id128);
/* A = (0,0) block (operator and preconditioning matrix, as KSPSetOperators(ksp,A,A));
 * B = (1,0) block of the nest sketched at :45-60, or NULL for the as-written A-only solve */
int SpkKSPSetOperators(SpkKSP ksp, const SpkMatCSR *A, const SpkMatCSR *B); /* KSPSetOperators :66 */
/* The same with A of the reference's own discretisation assembled on the device (spk_set_block_laplace, boundary
 * conditions applied): mx x my nodes; kappa: one host value per element, (mx-1)*(my-1) of them, or NULL for ones;
 * B as above; f_host: receives the rank's n_local right-hand side values, or NULL.  Leaves the KSP in the state
 * SpkKSPSetOperators would; -ksp_view names the route. */
int SpkKSPSetOperatorsLaplace(SpkKSP ksp, int mx, int my, const double *kappa, const SpkMatCSR *B, double *f_host);
/* The same for the 3-D generator of spk_assembly.h (spk_set_block_laplace3d): mx x my x mz nodes, dof 3; kappa: one host
 * value per hexahedron, (mx-1)*(my-1)*(mz-1) of them, or NULL for ones. */
int SpkKSPSetOperatorsLaplace3D(SpkKSP ksp, int mx, int my, int mz, const double *kappa, const SpkMatCSR *B, double *f_host);
/* The saddle system of the reference's own discretisation without a host matrix: A as SpkKSPSetOperatorsLaplace[3D]
 * assembles it, and the generator's constraint block (SpkAssembleOperator_Constraints[3D]: 4 rows in 2-D, 6 in 3-D)
 * written on the device by spk_set_block_constraints.  rhs_host: receives the rank's n_local values of f and, behind
 * them, the multipliers' right-hand side g (n_local + 4 values, + 6 in 3-D), or NULL.  Grid sides of at least 3.
 * Leaves the KSP in the state SpkKSPSetOperators(A, B) would; -ksp_view names the route. */
int SpkKSPSetOperatorsLaplaceConstrained(SpkKSP ksp, int mx, int my, const double *kappa, double *rhs_host);
int SpkKSPSetOperatorsLaplaceConstrained3D(SpkKSP ksp, int mx, int my, int mz, const double *kappa, double *rhs_host);
/* The node grid behind the operator of SpkKSPSetOperators: mx x my (x mz; 1 or 0 in 2-D) nodes in natural ordering, bs
 * unknowns per node (the role of KSPSetDM).  -pc_type mg and -fieldsplit_0_pc_type mg coarsen it; without a known grid
 * they are refused at SpkKSPSetUp.  SpkKSPSetOperatorsLaplace / ...3D set it themselves. */
int SpkKSPSetGrid(SpkKSP ksp, int mx, int my, int mz);
/* argv-style option list, e.g. {"-ksp_type","fgmres","-ksp_rtol","1e-8",
 * "-pc_type","fieldsplit","-pc_fieldsplit_type","schur",
 * "-pc_fieldsplit_schur_fact_type","full"}.  Unknown -ksp_/-pc_/-fieldsplit_
 * options are an error; other options are ignored (as PETSc leaves them unused).
 * DEVIATION from PETSc, on purpose: -ksp_type and -pc_type have NO default here.  PETSc would fall
 * back to gmres (left preconditioning) and ilu (bjacobi+ilu in parallel), neither of which this
 * library implements; SpkKSPSetUp / SpkKSPSolve return SPK_ERR_UNSUPPORTED with a message unless
 * "-ksp_type fgmres|minres|pipecg|pipecgrr" and "-pc_type jacobi|fieldsplit|gamg|none" were given.
 * -ksp_type minres (spk_minres) takes -ksp_norm_type unpreconditioned (default) | natural and needs a symmetric
 * positive definite preconditioner: none, jacobi, or fieldsplit with -pc_fieldsplit_schur_fact_type diag and no
 * FP32 inner sweeps; SpkKSPSetUp refuses the others with SPK_ERR_UNSUPPORTED before it looks at the operators.
 * -ksp_type pipecg (spk_pipecg) takes the same two norms and -pc_type none | jacobi | gamg on K = A; SpkKSPSetUp refuses
 * it with SPK_ERR_UNSUPPORTED beside -pc_type fieldsplit, the FP32 inner sweeps or -ksp_pc_side right (left only, as
 * PETSc's KSPPIPECG) before it looks at the operators, and with a B block once they are set.  -ksp_type pipecgrr
 * (spk_pipecgrr, pipecg with residual replacement) follows the same rules, with "pipecgrr" in the messages, and takes
 * -spk_pipecgrr_tau <tau >= 0> (SPK_PIPECGRR_TAU_DEFAULT); -ksp_view prints tau and the replacements of the last
 * solve.  -ksp_type cg is not implemented and stays refused.
 * -spk_basis_precision double (default) | single: how fgmres stores its Krylov basis (spk_opts.basis_precision; single:
 * FP32 storage, FP64 arithmetic, iteration form 5 on one rank; any other value: SPK_ERR_ARG; -ksp_view shows it).  What a
 * single-precision basis cannot run is refused by SpkKSPSolve with SPK_ERR_UNSUPPORTED. */
int SpkKSPSetFromOptions(SpkKSP ksp, int argc, const char *const *argv);    /* KSPSetFromOptions :67 */
int SpkKSPSetUp(SpkKSP ksp);                                                /* KSPSetUp       :68 */
/* b, x: host vectors of n_local + m values ([u ; lambda]) */
int SpkKSPSolve(SpkKSP ksp, const double *b, double *x);                    /* KSPSolve       :70 */
int SpkKSPDestroy(SpkKSP *ksp);                                             /* KSPDestroy     :72 */

int SpkKSPGetIterationNumber(SpkKSP ksp, int32_t *its);
int SpkKSPGetConvergedReason(SpkKSP ksp, int32_t *reason);
int SpkKSPGetResidualNorm(SpkKSP ksp, double *rnorm);
int SpkKSPGetResidualHistory(SpkKSP ksp, const double **hist, int32_t *n);
int SpkKSPGetSolveTime(SpkKSP ksp, double *seconds);
int SpkKSPGetOptions(SpkKSP ksp, spk_opts *opts, int32_t *pc_type, int32_t *schur_fact);
/* Multigrid options as read: fieldsplit0 = 0 the plain set (-pc_type gamg on K = A: -pc_gamg_threshold,
 * -pc_gamg_agg_nsmooths, -pc_gamg_coarse_eq_limit, -pc_mg_levels, -mg_levels_ksp_type chebyshev|richardson,
 * -spk_gamg_setup host|device (where the hierarchy is built; -ksp_view names it),
 * -mg_levels_ksp_max_it, -mg_levels_ksp_richardson_scale, -mg_levels_ksp_chebyshev_esteig a,b,c,d,
 * -mg_levels_pc_type jacobi), 1 the same names with the -fieldsplit_0_ prefix (-fieldsplit_0_pc_type gamg inside
 * -pc_type fieldsplit).  *selected = 1 when that gamg was asked for.  Unknown -mg_ options are refused like unknown
 * -ksp_ ones.  -pc_type gamg with a B block, gamg with -ksp_type minres (pipecg takes it) and gamg beside the FP32 inner sweeps are
 * refused by SpkKSPSetUp with SPK_ERR_UNSUPPORTED.  (SpkKSPGetOptions reports -pc_type gamg as SPK_PC_JACOBI, the
 * slot the V-cycle takes.)
 * -pc_type mg and -fieldsplit_0_pc_type mg select the same slots with grid coarsening (opts->coarsening =
 * SPK_AMG_COARSEN_GRID; PETSc: -pc_type mg -pc_mg_galerkin on a DMDA) and share the option sets: -pc_mg_levels,
 * -mg_levels_*, -pc_gamg_coarse_eq_limit, -pc_gamg_reuse_interpolation, -spk_gamg_setup; -pc_gamg_threshold and
 * -pc_gamg_agg_nsmooths are read and not used.  -pc_mg_galerkin takes no value, both or pmat (every coarse operator is
 * the Galerkin product; anything else: SPK_ERR_UNSUPPORTED); -spk_mg_transfer matrixfree|stored selects how the V-cycle
 * applies P and R (opts->transfer); -spk_mg_sides odd|any selects which sides halve (opts->sides: odd, the default, refuses
 * a grid whose even side keeps the coarsest level too large; any halves an even side of m >= 4 nodes to m / 2 + 1, so
 * 1024 -> 513 -> ... -> 5; another value: SPK_ERR_UNSUPPORTED; given without mg it is read and not used);
 * -spk_mg_galerkin products|stencil selects what forms the coarse operators (opts->galerkin: the generic sparse products,
 * the default, or the gather on the node grid of SPK_AMG_GALERKIN_STENCIL; another value: SPK_ERR_UNSUPPORTED naming the
 * two, no value: SPK_ERR_ARG; given without mg it is read and not used; -pc_mg_galerkin keeps its meaning);
 * -spk_mg_operator csr|stencil selects how the cycle applies the levels between level 0 and the coarsest (opts->op: as
 * sparse matrices, the default, or from their value arrays alone, SPK_AMG_OPERATOR_STENCIL, which needs mg with
 * -spk_mg_galerkin stencil: otherwise SpkKSPSetUp fails with SPK_ERR_UNSUPPORTED naming what is missing; another value:
 * SPK_ERR_UNSUPPORTED naming the two, no value: SPK_ERR_ARG; given without multigrid it is read and not used).
 * -spk_amg_lanczos stepwise|resident (both multigrids, also as -fieldsplit_0_spk_amg_lanczos) selects who holds the scalars
 * of the device set-up's Lanczos (opts->lanczos: the host, reading two sums back per step, the default, or a block on the
 * device read once per level, SPK_AMG_LANCZOS_RESIDENT -- the same hierarchy byte for byte; it needs -spk_gamg_setup device:
 * otherwise SpkKSPSetUp fails with SPK_ERR_UNSUPPORTED naming that option; another value: SPK_ERR_UNSUPPORTED naming the
 * two, no value: SPK_ERR_ARG; given without multigrid it is read and not used).
 * -spk_mg_precision double|single (also as -fieldsplit_0_spk_mg_precision) selects what the levels >= 1 of the cycle run in
 * (opts->precision: FP64, the default, or FP32, SPK_AMG_PRECISION_SINGLE, which needs mg with -spk_mg_galerkin stencil,
 * -spk_mg_operator stencil and matrix-free transfers: otherwise SpkKSPSetUp fails with SPK_ERR_UNSUPPORTED naming what is
 * missing; with -ksp_type pipecg | pipecgrr SpkKSPSetUp fails with SPK_ERR_UNSUPPORTED pointing to -ksp_type fgmres: the
 * rounded cycle is not an exactly symmetric operator; another value: SPK_ERR_UNSUPPORTED naming the two, no value:
 * SPK_ERR_ARG; given without multigrid it is read and not used).  The grid comes from SpkKSPSetOperatorsLaplace / ...3D or SpkKSPSetGrid and is
 * copied into opts->grid at SpkKSPSetUp, which refuses mg without one (SPK_ERR_STATE) before any GPU work; mg is refused
 * where gamg is. */
int SpkKSPGetAMGOptions(SpkKSP ksp, int fieldsplit0, spk_amg_opts *opts, int32_t *selected);
/* -pc_gamg_reuse_interpolation <bool> (fieldsplit0 = 1: -fieldsplit_0_pc_gamg_reuse_interpolation) as read; default
 * false, a name without a value means true.  On: SpkKSPSetUp passes spk_pc_set_amg_reuse(ctx, 1), so a second
 * SpkKSPSetOperators with new values on the same pattern followed by SpkKSPSetUp (or SpkKSPSolve) on the same SpkKSP
 * refreshes the hierarchy instead of building it (-ksp_view says which the last set-up did).  Given for a gamg that is
 * not selected, SpkKSPSetUp refuses it with SPK_ERR_UNSUPPORTED. */
int SpkKSPGetAMGReuse(SpkKSP ksp, int fieldsplit0, int32_t *reuse);
/* -ksp_type as set ("fgmres", "minres", "pipecg", "pipecgrr", or "" before KSPSetFromOptions gave one) and -ksp_norm_type
 * (SPK_NORM_*) */
int SpkKSPGetType(SpkKSP ksp, const char **type, int32_t *norm_type);
/* -pc_fieldsplit_schur_precondition selfp | full (SPK_SCHUR_PRE_*) and -fieldsplit_1_pc_type as they resolve: *dense_split1
 * = 0 for jacobi (entry-by-entry division by S^), 1 for cholesky | lu (the dense factor of the exact S).  Left out,
 * -fieldsplit_1_pc_type follows the precondition: jacobi for selfp, cholesky for full.  full with jacobi and selfp with
 * cholesky | lu are refused by SpkKSPSetUp with SPK_ERR_UNSUPPORTED before any GPU work. */
int SpkKSPGetSchurPre(SpkKSP ksp, int32_t *schur_pre, int32_t *dense_split1);
int SpkKSPGetContext(SpkKSP ksp, spk_ctx **ctx);
const char *SpkKSPGetError(SpkKSP ksp);
const char *SpkKSPConvergedReasonName(int32_t reason);

#ifdef __cplusplus
}
#endif
#endif
