// saddle_point_run.cpp -- stand-alone driver with the shape of the reference's
// program (/root/reference/src/main.c:7-19 -> SolveSaddlePointProblem,
// SaddlePointProblem.c:8-25 -> SolveConstraintLaplaceProblem, :34-76):
// set up the grid, assemble A, f (and the build-defined B, g), apply the
// boundary conditions, then the six solver calls of :65-72 through the
// KSP-shaped facade, options PETSc-style on the command line:
//
//   saddle_point_run -da_grid_x 257 -da_grid_y 257 -ksp_type fgmres -ksp_rtol 1e-8 \
//       -pc_type fieldsplit -pc_fieldsplit_type schur -pc_fieldsplit_schur_fact_type full \
//       -ksp_converged_reason [-saddle 0] [-solution_view] [-no_vtk] [-spk_assembly host|device]
//       [-spk_constraints host|device] [-spk_basis_precision double|single]
// (every option of SpkKSPSetFromOptions, include/spk_ksp.h: e.g. -pc_type mg -spk_mg_galerkin stencil -spk_mg_operator
// stencil -spk_mg_precision single)
//
// The reference hard-codes Nx = Ny = 3 elements (main.c:14), i.e. a 4 x 4 node
// grid; that is the default here too.  -saddle 0 solves A u = f alone, as the
// reference does at HEAD (KSPSetOperators(ksp, A, A), :66).  -spk_assembly device assembles A and f on
// the GPU (SpkKSPSetOperatorsLaplace) instead of on host threads; the default, host, is the flow above.
// -spk_constraints device (with -spk_assembly device) writes B and g there as well
// (SpkKSPSetOperatorsLaplaceConstrained): the saddle system comes up without a host matrix.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/spk_assembly.h"
#include "../../include/spk_ksp.h"

static int opt_int(int argc, char **argv, const char *name, int dflt)
{
    for (int i = 1; i + 1 < argc; ++i)
        if (!std::strcmp(argv[i], name)) return std::atoi(argv[i + 1]);
    return dflt;
}
static const char *opt_str(int argc, char **argv, const char *name, const char *dflt)
{
    for (int i = 1; i + 1 < argc; ++i)
        if (!std::strcmp(argv[i], name)) return argv[i + 1];
    return dflt;
}
static bool opt_flag(int argc, char **argv, const char *name)
{
    for (int i = 1; i < argc; ++i)
        if (!std::strcmp(argv[i], name)) return true;
    return false;
}

#define CHK(call)                                                             \
    do {                                                                      \
        int rc_ = (call);                                                     \
        if (rc_) {                                                            \
            std::fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, ksp ? SpkKSPGetError(ksp) : ""); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

int main(int argc, char **argv)
{
    SpkKSP ksp = nullptr;
    const int mx = opt_int(argc, argv, "-da_grid_x", 4), my = opt_int(argc, argv, "-da_grid_y", 4);
    const bool saddle = opt_int(argc, argv, "-saddle", 1) != 0;
    const char *route = opt_str(argc, argv, "-spk_assembly", "host");
    const bool on_device = !std::strcmp(route, "device");
    if (!on_device && std::strcmp(route, "host")) { std::fprintf(stderr, "-spk_assembly %s is not supported (host | device)\n", route); return 1; }
    const char *broute = opt_str(argc, argv, "-spk_constraints", "host");
    const bool b_on_device = !std::strcmp(broute, "device");
    if (!b_on_device && std::strcmp(broute, "host")) { std::fprintf(stderr, "-spk_constraints %s is not supported (host | device)\n", broute); return 1; }
    if (b_on_device && !on_device) { std::fprintf(stderr, "-spk_constraints device needs -spk_assembly device\n"); return 1; }
    if (b_on_device && !saddle) { std::fprintf(stderr, "-spk_constraints device needs the saddle system (-saddle 1)\n"); return 1; }
    int64_t n = 0, nnz = 0;
    CHK(SpkAssemblySizes(mx, my, &n, &nnz));

    // SetupDMDA + AssembleOperator_Laplace + AssembleRHS_Laplace + ApplyBC_Laplace (host route; the device route
    // does the same inside KSPSetOperators below)
    std::vector<int32_t> rowptr, colidx;
    std::vector<double> val, rhs((size_t)n + 4, 0.0), sol((size_t)n + 4, 0.0);
    if (!on_device) {
        rowptr.resize((size_t)n + 1);
        colidx.resize((size_t)nnz);
        val.resize((size_t)nnz);
        CHK(SpkAssembleOperator_Laplace(mx, my, 0, n, rowptr.data(), colidx.data(), val.data(), rhs.data(), 1, 0));
    }
    SpkMatCSR A = {0, (int32_t)n, 0, n, rowptr.data(), colidx.data(), val.data()};

    // AssembleOperator_Constraints + AssembleRHS_Constraints (stubs in the reference)
    std::vector<int32_t> brp(5), bci;
    std::vector<double> bv;
    SpkMatCSR B = {0, 4, 0, n, nullptr, nullptr, nullptr};
    if (saddle) {
        const int64_t bn = SpkConstraintsSlabNnz(mx, my, 0, n);
        if (bn < 0) { std::fprintf(stderr, "grid too small for the constraint block\n"); return 1; }
    }
    if (saddle && !b_on_device) {
        const int64_t bn = SpkConstraintsSlabNnz(mx, my, 0, n);
        bci.resize((size_t)bn);
        bv.resize((size_t)bn);
        CHK(SpkAssembleOperator_Constraints(mx, my, 0, n, brp.data(), bci.data(), bv.data()));
        CHK(SpkAssembleRHS_Constraints(rhs.data() + n));
        B.rowptr = brp.data(); B.colidx = bci.data(); B.val = bv.data();
    }

    // the call site SaddlePointProblem.c:65-72
    CHK(SpkKSPCreate(opt_int(argc, argv, "-spk_device", 0), &ksp));
    if (b_on_device) CHK(SpkKSPSetOperatorsLaplaceConstrained(ksp, mx, my, nullptr, rhs.data()));
    else if (on_device) CHK(SpkKSPSetOperatorsLaplace(ksp, mx, my, nullptr, saddle ? &B : nullptr, rhs.data()));
    else CHK(SpkKSPSetOperators(ksp, &A, saddle ? &B : nullptr));
    CHK(SpkKSPSetGrid(ksp, mx, my, 1));   // the DMDA's grid: what -pc_type mg coarsens
    CHK(SpkKSPSetFromOptions(ksp, argc - 1, argv + 1));
    CHK(SpkKSPSetUp(ksp));
    CHK(SpkKSPSolve(ksp, rhs.data(), sol.data()));

    int32_t its = 0, reason = 0;
    double rnorm = 0.0, secs = 0.0;
    SpkKSPGetIterationNumber(ksp, &its);
    SpkKSPGetConvergedReason(ksp, &reason);
    SpkKSPGetResidualNorm(ksp, &rnorm);
    SpkKSPGetSolveTime(ksp, &secs);
    std::printf("grid %d x %d nodes, %lld rows%s: %s after %d iterations, residual %.6e, solve %.3f ms\n", mx, my,
                (long long)n, saddle ? " + 4 multipliers" : "", SpkKSPConvergedReasonName(reason), its, rnorm, secs * 1e3);
    if (opt_flag(argc, argv, "-solution_view")) {  // VecViewFromOptions(u, NULL, "-solution_view"), :20
        for (int64_t i = 0; i < n + (saddle ? 4 : 0); ++i) std::printf("%.15e\n", sol[(size_t)i]);
    }
    // WriteVTK(da_u, u, "test.vtk"), SaddlePointProblem.c:22 -- with the field this time
    if (!opt_flag(argc, argv, "-no_vtk")) CHK(SpkWriteVTK(mx, my, sol.data(), "test.vtk"));
    CHK(SpkKSPDestroy(&ksp));
    return reason > 0 ? 0 : 2;
}
