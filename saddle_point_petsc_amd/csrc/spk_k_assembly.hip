// spk_k_assembly.hip -- the A block and right-hand side of the reference's 2-D discretisation, written where
// KSPSetOperators consumes them: the CSR slab rowptr / colidx / val (global ascending columns) and f of rows
// [2 mx j0, 2 mx j1) in device memory, bit for bit what SpkAssembleOperator_Laplace[Kappa] (spk_assembly.cpp) produces.
//
// Why the bits match: every floating-point expression below is the host's, operand for operand and in the host's
// order (coord, make_gp, phys_grad, stiffness, load), the file is compiled without contraction (the x86-64 host
// build has no FMA; FP64 division is correctly rounded on both sides), and every stored entry is GATHERED: the sum,
// started at 0.0, of the at most four element entries that hold both nodes, visited in ascending (ej, ei).  No
// atomics, no entry written twice.
//
// One workgroup per node line j and strip of kAsmStrip nodes:
//   phase 1a  one thread per (element, Gauss point) of the two element lines j-1, j over the strip: physical gradients
//             and det J into LDS (the element coordinates carry the rounding of coord(), so they differ per element)
//   phase 1b  one thread per entry of Ke (64 per element) and of Fe (8): twelve / four ordered additions
//   phase 2   the threads stride over the workgroup's contiguous output range; the row pointers are closed-form, so
//             entry -> (node, c, dj, di, d) is index arithmetic and the 12 B per entry go out coalesced
#include "spk_internal.hpp"

#pragma clang fp contract(off)

namespace spk {
namespace k {

namespace {

constexpr int kAsmThreads = 256;
constexpr int kAsmStrip = 32;               // nodes of a line per workgroup
constexpr int kAsmElems = kAsmStrip + 1;    // elements of one element line that touch them
constexpr int kAsmSlots = 2 * kAsmElems;    // element lines j-1 (slots 0..) and j (slots kAsmElems..)
constexpr int kAsmG = 9;                    // per (element, Gauss point): gx[2][4], det J

// the reference's truncated abscissa (Discretization.c:52-55)
__device__ inline double gp_xi(int p) { return p < 2 ? -0.57735026919 : 0.57735026919; }
__device__ inline double gp_eta(int p) { return (p == 0 || p == 3) ? -0.57735026919 : 0.57735026919; }

__device__ inline double asm_coord(int i, int m) { return 0.0 + (1.0 / (double)(m - 1)) * (double)i; }

// stored entries of the rows in front of node i of a line, in units of (2 rows) x (2 columns) x wj: sum of the widths
__device__ inline int asm_prefix(int i, int m) { return 3 * i - (i > 0) - (i > m - 1); }
__device__ inline int asm_width(int i, int m) { return (i > 0) + 1 + (i < m - 1); }
__device__ inline int asm_corner(int oi, int oj) { return oi == 0 ? (oj == 0 ? 0 : 1) : (oj == 0 ? 3 : 2); }
__device__ inline bool asm_boundary(int mx, int my, int i, int j) { return i == 0 || i == mx - 1 || j == 0 || j == my - 1; }

__global__ __launch_bounds__(kAsmThreads) void assemble_laplace_kernel(int mx, int my, int j0, int j1, int nstrips,
                                                                       const double *__restrict__ kappa, int apply_bc,
                                                                       int32_t *__restrict__ rowptr, int32_t *__restrict__ colidx,
                                                                       double *__restrict__ val, double *__restrict__ f)
{
    __shared__ double Ke[kAsmSlots * 64];
    __shared__ double Fe[kAsmSlots * 8];
    __shared__ double G[kAsmSlots * 4 * kAsmG];
    __shared__ double kap[kAsmSlots];
    const int tid = (int)threadIdx.x;
    const int j = j0 + (int)(blockIdx.x / (unsigned)nstrips);
    const int i0 = (int)(blockIdx.x % (unsigned)nstrips) * kAsmStrip;
    const int i1 = min(i0 + kAsmStrip, mx);
    // element (ej, ei) of slot: ej = j - 1 + slot / kAsmElems, ei = i0 - 1 + slot % kAsmElems; the ones that exist and touch the strip
    auto live = [&](int slot, int &ei, int &ej) {
        const int l = slot / kAsmElems;
        ej = j - 1 + l;
        ei = i0 - 1 + (slot - l * kAsmElems);
        return ej >= 0 && ej <= my - 2 && ei >= 0 && ei <= mx - 2 && ei <= i1 - 1;
    };

    // ---- phase 1a: make_gp + phys_grad per (element, Gauss point)
    for (int t = tid; t < kAsmSlots * 4; t += kAsmThreads) {
        const int p = t & 3, slot = t >> 2;
        int ei, ej;
        if (!live(slot, ei, ej)) continue;
        double xe[8];
        xe[0] = asm_coord(ei, mx);     xe[1] = asm_coord(ej, my);
        xe[2] = asm_coord(ei, mx);     xe[3] = asm_coord(ej + 1, my);
        xe[4] = asm_coord(ei + 1, mx); xe[5] = asm_coord(ej + 1, my);
        xe[6] = asm_coord(ei + 1, mx); xe[7] = asm_coord(ej, my);
        const double xi = gp_xi(p), eta = gp_eta(p);
        double dN[2][4];
        dN[0][0] = -0.25 * (1.0 - eta);
        dN[0][1] = -0.25 * (1.0 + eta);
        dN[0][2] = 0.25 * (1.0 + eta);
        dN[0][3] = 0.25 * (1.0 - eta);
        dN[1][0] = -0.25 * (1.0 - xi);
        dN[1][1] = 0.25 * (1.0 - xi);
        dN[1][2] = 0.25 * (1.0 + xi);
        dN[1][3] = -0.25 * (1.0 + xi);
        double J[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int d = 0; d < 2; ++d)
#pragma unroll
                for (int i = 0; i < 4; ++i) J[c][d] += dN[c][i] * xe[2 * i + d];
        const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
        const double i00 = J[1][1] / det, i01 = -J[0][1] / det, i10 = -J[1][0] / det, i11 = J[0][0] / det;
        double *g = G + (size_t)t * kAsmG;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            g[i] = i00 * dN[0][i] + i01 * dN[1][i];
            g[4 + i] = i10 * dN[0][i] + i11 * dN[1][i];
        }
        g[8] = det;
        if (p == 0) kap[slot] = kappa ? kappa[(size_t)ej * (size_t)(mx - 1) + (size_t)ei] : 1.0;
    }
    __syncthreads();

    // ---- phase 1b: Ke, entry acc[i + 8 jj] of the host (Gauss points outermost, the three strain rows inside)
    for (int t = tid; t < kAsmSlots * 64; t += kAsmThreads) {
        const int slot = t >> 6, i = t & 7, jj = (t >> 3) & 7;
        int ei, ej;
        if (!live(slot, ei, ej)) continue;
        const double kp = kap[slot];
        const int a = i >> 1, b = jj >> 1;
        const bool ix = (i & 1) == 0, jx = (jj & 1) == 0;
        double acc = 0.0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const double *g = G + (size_t)(slot * 4 + p) * kAsmG;
            const double det = g[8];
            const double tD0 = 2.0 * 1.0 * det * kp;
            const double tD1 = 2.0 * 1.0 * det * kp;
            const double tD2 = 1.0 * det * kp;
            // Bm[k][2 n] = (gx0, 0, gx1), Bm[k][2 n + 1] = (0, gx1, gx0)
            const double bi0 = ix ? g[a] : 0.0, bi1 = ix ? 0.0 : g[4 + a], bi2 = ix ? g[4 + a] : g[a];
            const double bj0 = jx ? g[b] : 0.0, bj1 = jx ? 0.0 : g[4 + b], bj2 = jx ? g[4 + b] : g[b];
            acc += bi0 * tD0 * bj0;
            acc += bi1 * tD1 * bj1;
            acc += bi2 * tD2 * bj2;
        }
        Ke[t] = acc;
    }
    // ... and Fe (FormRHS, body force (1, 2))
    for (int t = tid; t < kAsmSlots * 8; t += kAsmThreads) {
        const int slot = t >> 3, n = (t >> 1) & 3, c = t & 1;
        int ei, ej;
        if (!live(slot, ei, ej)) continue;
        double fe = 0.0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const double xi = gp_xi(p), eta = gp_eta(p);
            const double N = n == 0 ? 0.25 * (1.0 - xi) * (1.0 - eta)
                           : n == 1 ? 0.25 * (1.0 - xi) * (1.0 + eta)
                           : n == 2 ? 0.25 * (1.0 + xi) * (1.0 + eta)
                                    : 0.25 * (1.0 + xi) * (1.0 - eta);
            const double fac = 1.0 * G[(size_t)(slot * 4 + p) * kAsmG + 8];
            const double body = c ? 2.0 : 1.0;
            fe += fac * N * body;
        }
        Fe[t] = fe;
    }
    __syncthreads();

    // ---- phase 2: the workgroup's rows, entry by entry
    const int wj = asm_width(j, my);
    const int64_t lines_before = (int64_t)asm_prefix(j, my) - asm_prefix(j0, my);
    const int64_t line_base = 4 * (3 * (int64_t)mx - 2) * lines_before;
    const int x0 = asm_prefix(i0, mx);
    const int64_t wg_base = line_base + (int64_t)4 * wj * x0;
    const int count = 4 * wj * (asm_prefix(i1, mx) - x0);
    for (int o = tid; o < count; o += kAsmThreads) {
        const int i = (o / (4 * wj) + x0 + 1) / 3;
        const int wi = asm_width(i, mx);
        const int r = o - 4 * wj * (asm_prefix(i, mx) - x0);
        const int rowlen = 2 * wi * wj;
        const int c = r >= rowlen ? 1 : 0;
        const int r2 = r - c * rowlen;
        const int d = r2 & 1, t2 = r2 >> 1;
        const int djx = t2 / wi;
        const int cj = j - (j > 0) + djx, ci = i - (i > 0) + (t2 - djx * wi);
        const int64_t grow = ((int64_t)j * mx + i) * 2 + c, gcol = ((int64_t)cj * mx + ci) * 2 + d;
        double v = 0.0;
        // elements that hold both nodes, ascending (ej, ei)
        for (int ej = max(j, cj) - 1; ej <= min(j, cj); ++ej) {
            if (ej < 0 || ej > my - 2) continue;
            for (int ei = max(i, ci) - 1; ei <= min(i, ci); ++ei) {
                if (ei < 0 || ei > mx - 2) continue;
                const int slot = (ej - (j - 1)) * kAsmElems + (ei - (i0 - 1));
                const int a = asm_corner(i - ei, j - ej) * 2 + c;
                const int b = asm_corner(ci - ei, cj - ej) * 2 + d;
                v += Ke[slot * 64 + a * 8 + b];
            }
        }
        if (apply_bc && (asm_boundary(mx, my, i, j) || asm_boundary(mx, my, ci, cj))) v = (gcol == grow) ? 1.0 : 0.0;
        colidx[wg_base + o] = (int32_t)gcol;
        val[wg_base + o] = v;
    }
    // row pointers and f of the strip's rows
    if (tid < 2 * (i1 - i0)) {
        const int i = i0 + (tid >> 1), c = tid & 1;
        const int wi = asm_width(i, mx);
        const int64_t lrow = ((int64_t)(j - j0) * mx + i) * 2 + c;
        rowptr[lrow] = (int32_t)(line_base + (int64_t)4 * wj * asm_prefix(i, mx) + (int64_t)c * 2 * wi * wj);
        if (f) {
            double fv = 0.0;
            for (int ej = j - 1; ej <= j; ++ej) {
                if (ej < 0 || ej > my - 2) continue;
                for (int ei = i - 1; ei <= i; ++ei) {
                    if (ei < 0 || ei > mx - 2) continue;
                    const int slot = (ej - (j - 1)) * kAsmElems + (ei - (i0 - 1));
                    fv += Fe[slot * 8 + asm_corner(i - ei, j - ej) * 2 + c];
                }
            }
            f[lrow] = (apply_bc && asm_boundary(mx, my, i, j)) ? 0.0 : fv;
        }
    }
    if (tid == 0 && j == j1 - 1 && i1 == mx)
        rowptr[(int64_t)(j1 - j0) * mx * 2] = (int32_t)(line_base + 4 * (3 * (int64_t)mx - 2) * wj);
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
    const int nstrips = (mx + kAsmStrip - 1) / kAsmStrip;
    const int64_t grid = (int64_t)nstrips * (j1 - j0);
    if (grid > INT32_MAX) fail(SPK_ERR_UNSUPPORTED, "device assembly: %lld workgroups", (long long)grid);
    hipLaunchKernelGGL(assemble_laplace_kernel, dim3((unsigned)grid), dim3(kAsmThreads), 0, s, mx, my, j0, j1, nstrips, kappa, apply_bc,
                       rowptr, colidx, val, f);
    SPK_HIP(hipGetLastError());
}

void kappa_check(const double *kappa, int64_t ne, int32_t *flag, hipStream_t s)
{
    if (ne <= 0) return;
    const int grid = (int)std::min<int64_t>((ne + kAsmThreads - 1) / kAsmThreads, kMaxBlocks);
    hipLaunchKernelGGL(kappa_check_kernel, dim3(grid), dim3(kAsmThreads), 0, s, kappa, ne, flag);
    SPK_HIP(hipGetLastError());
}

}  // namespace k
}  // namespace spk
