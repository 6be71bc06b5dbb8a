// spk_k_assembly.hip -- the A block and right-hand side of the reference's 2-D discretisation, written where
// KSPSetOperators consumes them: the CSR slab rowptr / colidx / val (global ascending columns) and f of rows
// [2 mx j0, 2 mx j1) in device memory, bit for bit what SpkAssembleOperator_Laplace[Kappa] (spk_assembly.cpp) produces.
//
// Why the bits match: the phases below and the host assembler call the same functions of spk_assembly_core.hpp (coord,
// gauss2, ke2_entry, fe2_entry), both sides are compiled without contraction (the x86-64 host build has no FMA; FP64
// division is correctly rounded on both sides), and every stored entry is GATHERED: the sum, started at 0.0, of the at
// most four element entries that hold both nodes, visited in ascending (ej, ei).  No atomics, no entry written twice.
// tests/test_assembly_kernel_host_cpu.py runs the same phases on the CPU, thread by thread, against the host assembler.
//
// One workgroup per node line j and strip of kStrip2 nodes (the phases are in spk_assembly_core.hpp):
//   phase 1a  one thread per (element, Gauss point) of the two element lines j-1, j over the strip: physical gradients
//             and det J into LDS (the element coordinates carry the rounding of coord(), so they differ per element)
//   phase 1b  one thread per entry of Ke (64 per element) and of Fe (8): twelve / four ordered additions
//   phase 2   the threads stride over the workgroup's contiguous output range; the row pointers are closed-form, so
//             entry -> (node, c, dj, di, d) is index arithmetic and the 12 B per entry go out coalesced
#include "spk_internal.hpp"
#include "spk_assembly_core.hpp"

#pragma clang fp contract(off)

namespace spk {
namespace k {

namespace {

namespace as = spk::assembly;
constexpr int kAsmThreads = 256;

__global__ __launch_bounds__(kAsmThreads) void assemble_laplace_kernel(int mx, int my, int j0, int j1, int nstrips,
                                                                       const double *__restrict__ kappa, int apply_bc,
                                                                       int32_t *__restrict__ rowptr, int32_t *__restrict__ colidx,
                                                                       double *__restrict__ val, double *__restrict__ f)
{
    __shared__ double Ke[as::kLdsKe2];
    __shared__ double Fe[as::kLdsFe2];
    __shared__ double G[as::kLdsG2];
    __shared__ double kap[as::kLdsKap2];
    const int tid = (int)threadIdx.x;
    as::asm2_phase1a(tid, kAsmThreads, blockIdx.x, mx, my, j0, nstrips, kappa, G, kap);
    __syncthreads();
    as::asm2_phase1b(tid, kAsmThreads, blockIdx.x, mx, my, j0, nstrips, G, kap, Ke, Fe);
    __syncthreads();
    as::asm2_phase2(tid, kAsmThreads, blockIdx.x, mx, my, j0, j1, nstrips, apply_bc, Ke, Fe, rowptr, colidx, val, f);
}

// flag[0] := 1 when an entry is not finite and > 0 (the same word from every thread that finds one)
__global__ __launch_bounds__(kAsmThreads) void kappa_check_kernel(const double *__restrict__ kappa, int64_t ne, int32_t *flag)
{
    for (int64_t e = (int64_t)blockIdx.x * kAsmThreads + threadIdx.x; e < ne; e += (int64_t)gridDim.x * kAsmThreads) {
        const double v = kappa[e];
        if (!(v > 0.0) || !(v <= 1.7976931348623157e308)) flag[0] = 1;
    }
}

}  // namespace

void assemble_laplace(int mx, int my, int j0, int j1, const double *kappa, int apply_bc, int32_t *rowptr, int32_t *colidx, double *val,
                      double *f, hipStream_t s)
{
    if (j1 <= j0) {   // an empty slab: rowptr[0] alone
        SPK_HIP(hipMemsetAsync(rowptr, 0, sizeof(int32_t), s));
        return;
    }
    const int64_t grid = assemble_laplace_grid(mx, j0, j1);
    if (grid > INT32_MAX) fail(SPK_ERR_UNSUPPORTED, "device assembly: %lld workgroups", (long long)grid);
    hipLaunchKernelGGL(assemble_laplace_kernel, dim3((unsigned)grid), dim3(kAsmThreads), 0, s, mx, my, j0, j1, as::strips2(mx), kappa,
                       apply_bc, rowptr, colidx, val, f);
    SPK_HIP(hipGetLastError());
}
int64_t assemble_laplace_grid(int mx, int j0, int j1) { return as::grid2(mx, j0, j1); }

void kappa_check(const double *kappa, int64_t ne, int32_t *flag, hipStream_t s)
{
    if (ne <= 0) return;
    const int grid = (int)std::min<int64_t>((ne + kAsmThreads - 1) / kAsmThreads, kMaxBlocks);
    hipLaunchKernelGGL(kappa_check_kernel, dim3(grid), dim3(kAsmThreads), 0, s, kappa, ne, flag);
    SPK_HIP(hipGetLastError());
}

}  // namespace k
}  // namespace spk
