// spk_k_assembly3d.hip -- the A block and right-hand side of the 3-D generator (Q1 hexahedra, dof 3; spk_assembly.h),
// written where KSPSetOperators consumes them: the CSR slab rowptr / colidx / val (global ascending columns) and f of
// the node planes [k0, k1) in device memory, bit for bit what SpkAssembleOperator_Laplace3D[Kappa] produces.
//
// Why the bits match: the phases below and the host assembler call the same functions of spk_assembly_core.hpp (coord,
// gauss3, ke3_entry, fe3_entry), both sides are compiled without contraction (the x86-64 host build has no FMA; FP64
// division is correctly rounded on both sides), and every stored entry is GATHERED: the sum, started at 0.0, of the at
// most eight element entries of the hexahedra that hold both nodes, visited in ascending (ek, ej, ei).  No atomics, no
// entry written twice.  The structural zeros of the strain-displacement matrix are multiplied through on both sides (a
// select puts the 0.0 there), so no argument about signed zeros is needed.  tests/test_assembly_kernel_host_cpu.py runs
// the same phases on the CPU, thread by thread, against the host assembler.
//
// The 24 x 24 element matrix (4608 B) does not fit in LDS for the 4 (S + 1) hexahedra a strip of S nodes touches, so it
// is never stored whole: a node needs only its own three rows of each of its eight hexahedra.  One workgroup per node
// line (j, k) and strip of kStrip3 nodes (the phases are in spk_assembly_core.hpp):
//   phase 1   one thread per (element, Gauss point) of the four element lines (j-1..j, k-1..k) over the strip: the
//             physical gradients Gx[3][8], det J and the two values of tD into LDS (27 doubles; the element coordinates
//             carry the rounding of coord(), so they differ per element)
//   phase 2a  one thread per element entry the strip's rows need -- (node, c, one of the node's eight hexahedra, b): every
//             thread does the same work, eight Gauss points outermost with the six strain rows inside, each term
//             Bm[k][b] * tD[k] * Bm[k][a] from six gradients and tD in LDS -- into LDS.  Every Ke[a][b] of every
//             element feeds exactly one stored entry, so nothing is computed twice across the grid.
//   phase 2b  the threads stride over the workgroup's contiguous output range; the row pointers are closed-form, so
//             entry -> (node, c, dk, dj, di, d) is index arithmetic, the entry is the ordered sum of its at most eight
//             element entries, and the 12 B per entry go out coalesced.  One thread per row writes rowptr and f (the
//             element loads are eight ordered additions each, recomputed from det J).
// (Summing an entry's hexahedra in one thread straight from phase 1 leaves most lanes idle: an entry has 1, 2, 4 or 8 of
// them, 2.4 on average, and a wave runs as long as its longest lane.)
#include "spk_internal.hpp"
#include "spk_assembly_core.hpp"

#pragma clang fp contract(off)

namespace spk {
namespace k {

namespace {

namespace as = spk::assembly;
constexpr int kAsm3Threads = 256;

__global__ __launch_bounds__(kAsm3Threads) void assemble_laplace3d_kernel(int mx, int my, int mz, int k0, int k1, int nstrips,
                                                                          const double *__restrict__ kappa, int apply_bc,
                                                                          int32_t *__restrict__ rowptr, int32_t *__restrict__ colidx,
                                                                          double *__restrict__ val, double *__restrict__ f)
{
    __shared__ double G[as::kLdsG3];
    __shared__ double Kv[as::kLdsKv3];
    const int tid = (int)threadIdx.x;
    as::asm3_phase1(tid, kAsm3Threads, blockIdx.x, mx, my, mz, k0, nstrips, kappa, G);
    __syncthreads();
    as::asm3_phase2a(tid, kAsm3Threads, blockIdx.x, mx, my, mz, k0, nstrips, G, Kv);
    __syncthreads();
    as::asm3_phase2b(tid, kAsm3Threads, blockIdx.x, mx, my, mz, k0, k1, nstrips, apply_bc, G, Kv, rowptr, colidx, val, f);
}

}  // namespace

void assemble_laplace3d(int mx, int my, int mz, int k0, int k1, const double *kappa, int apply_bc, int32_t *rowptr, int32_t *colidx,
                        double *val, double *f, hipStream_t s)
{
    if (k1 <= k0) {   // an empty slab: rowptr[0] alone
        SPK_HIP(hipMemsetAsync(rowptr, 0, sizeof(int32_t), s));
        return;
    }
    const int64_t grid = assemble_laplace3d_grid(mx, my, k0, k1);
    if (grid > INT32_MAX) fail(SPK_ERR_UNSUPPORTED, "device assembly: %lld workgroups", (long long)grid);
    hipLaunchKernelGGL(assemble_laplace3d_kernel, dim3((unsigned)grid), dim3(kAsm3Threads), 0, s, mx, my, mz, k0, k1, as::strips3(mx), kappa,
                       apply_bc, rowptr, colidx, val, f);
    SPK_HIP(hipGetLastError());
}

int64_t assemble_laplace3d_grid(int mx, int my, int k0, int k1) { return as::grid3(mx, my, k0, k1); }

}  // namespace k
}  // namespace spk
