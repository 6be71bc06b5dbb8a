// spk_k_assembly3d.hip -- the A block and right-hand side of the 3-D generator (Q1 hexahedra, dof 3; spk_assembly.h),
// written where KSPSetOperators consumes them: the CSR slab rowptr / colidx / val (global ascending columns) and f of
// the node planes [k0, k1) in device memory, bit for bit what SpkAssembleOperator_Laplace3D[Kappa] produces.
//
// Why the bits match: every floating-point expression below is the host's (coord, element3d), operand for operand and
// in the host's order, the file is compiled without contraction (the x86-64 host build has no FMA; FP64 division is
// correctly rounded on both sides), and every stored entry is GATHERED: the sum, started at 0.0, of the at most eight
// element entries of the hexahedra that hold both nodes, visited in ascending (ek, ej, ei).  No atomics, no entry
// written twice.  The structural zeros of the strain-displacement matrix are multiplied through as on the host (a
// select puts the 0.0 where the host's memset left it), so no argument about signed zeros is needed.
//
// The 24 x 24 element matrix (4608 B) does not fit in LDS for the 4 (S + 1) hexahedra a strip of S nodes touches, so it
// is never stored whole: a node needs only its own three rows of each of its eight hexahedra.  One workgroup per node
// line (j, k) and strip of kAsm3Strip nodes:
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

#pragma clang fp contract(off)

namespace spk {
namespace k {

namespace {

constexpr int kAsm3Threads = 256;
constexpr int kAsm3Strip = 4;                  // nodes of a line per workgroup
constexpr int kAsm3Elems = kAsm3Strip + 1;     // elements of one element line that touch them
constexpr int kAsm3Slots = 4 * kAsm3Elems;     // element lines (ej, ek) = (j-1, k-1), (j, k-1), (j-1, k), (j, k)
constexpr int kAsm3G = 27;                     // per (element, Gauss point): Gx[3][8], det J, tD of the normal and of the shear rows
constexpr int kAsm3Kv = kAsm3Strip * 3 * 8 * 24;   // element entries of the strip's rows: (node, c, hexahedron of the node, b)

// corner a of the hexahedron and Gauss point p: the signs (-1,-1,-1) (-1,1,-1) (1,1,-1) (1,-1,-1), then the same at +1 in z
__device__ inline double asm3_sx(int a) { return (a & 3) >= 2 ? 1.0 : -1.0; }
__device__ inline double asm3_sy(int a) { return (a & 3) == 1 || (a & 3) == 2 ? 1.0 : -1.0; }
__device__ inline double asm3_sz(int a) { return a >= 4 ? 1.0 : -1.0; }

__device__ inline double asm3_coord(int i, int m) { return 0.0 + (1.0 / (double)(m - 1)) * (double)i; }
// sum of the widths of the nodes in front of node i of a line of m
__device__ inline int asm3_prefix(int i, int m) { return 3 * i - (i > 0) - (i > m - 1); }
__device__ inline int asm3_width(int i, int m) { return (i > 0) + 1 + (i < m - 1); }
__device__ inline int asm3_corner(int oi, int oj, int ok) { return (oi == 0 ? (oj == 0 ? 0 : 1) : (oj == 0 ? 3 : 2)) + 4 * ok; }
__device__ inline bool asm3_boundary(int mx, int my, int mz, int i, int j, int k)
{
    return i == 0 || i == mx - 1 || j == 0 || j == my - 1 || k == 0 || k == mz - 1;
}
__device__ inline int asm3_min(int a, int b) { return a < b ? a : b; }
__device__ inline int asm3_max(int a, int b) { return a > b ? a : b; }

// Bm[row][3 n + comp] of the host: g0, g1, g2 are Gx[0..2][n]; 0.0 where the host's memset left it
template <int ROW>
__device__ inline double asm3_bm(int comp, double g0, double g1, double g2)
{
    if (ROW == 0) return comp == 0 ? g0 : 0.0;
    if (ROW == 1) return comp == 1 ? g1 : 0.0;
    if (ROW == 2) return comp == 2 ? g2 : 0.0;
    if (ROW == 3) return comp == 0 ? g1 : comp == 1 ? g0 : 0.0;
    if (ROW == 4) return comp == 1 ? g2 : comp == 2 ? g1 : 0.0;
    return comp == 0 ? g2 : comp == 2 ? g0 : 0.0;
}

// the workgroup's node line and strip
struct Asm3Wg {
    int j, k, i0, i1;
};
__device__ inline Asm3Wg asm3_wg(unsigned block, int mx, int my, int k0, int nstrips)
{
    Asm3Wg w;
    const int line = (int)(block / (unsigned)nstrips);
    w.i0 = (int)(block % (unsigned)nstrips) * kAsm3Strip;
    w.i1 = asm3_min(w.i0 + kAsm3Strip, mx);
    w.j = line % my;
    w.k = k0 + line / my;
    return w;
}
// element of slot: ej = j - 1 + (l & 1), ek = k - 1 + (l >> 1), ei = i0 - 1 + slot % kAsm3Elems; whether it exists and touches the strip
__device__ inline bool asm3_live(const Asm3Wg &w, int mx, int my, int mz, int slot, int &ei, int &ej, int &ek)
{
    const int l = slot / kAsm3Elems;
    ej = w.j - 1 + (l & 1);
    ek = w.k - 1 + (l >> 1);
    ei = w.i0 - 1 + (slot - l * kAsm3Elems);
    return ek >= 0 && ek <= mz - 2 && ej >= 0 && ej <= my - 2 && ei >= 0 && ei <= mx - 2 && ei <= w.i1 - 1;
}
__device__ inline int asm3_slot(const Asm3Wg &w, int ei, int ej, int ek)
{
    return ((ek - (w.k - 1)) * 2 + (ej - (w.j - 1))) * kAsm3Elems + (ei - (w.i0 - 1));
}

// ---- phase 1: the gradients, det J and tD of element3d per (element, Gauss point); G is the workgroup's LDS
__device__ inline void asm3_phase1(int tid, unsigned block, int mx, int my, int mz, int k0, int nstrips, const double *kappa, double *G)
{
    const Asm3Wg w = asm3_wg(block, mx, my, k0, nstrips);
    const double gp1 = 0.57735026919;
    for (int t = tid; t < kAsm3Slots * 8; t += kAsm3Threads) {
        const int p = t & 7, slot = t >> 3;
        int ei, ej, ek;
        if (!asm3_live(w, mx, my, mz, slot, ei, ej, ek)) continue;
        const double xi[3] = {asm3_sx(p) * gp1, asm3_sy(p) * gp1, asm3_sz(p) * gp1};
        const double cx[2] = {asm3_coord(ei, mx), asm3_coord(ei + 1, mx)};
        const double cy[2] = {asm3_coord(ej, my), asm3_coord(ej + 1, my)};
        const double cz[2] = {asm3_coord(ek, mz), asm3_coord(ek + 1, mz)};
        double xe[24], Gr[3][8], J[3][3], iJ[3][3];
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const double sx = asm3_sx(a), sy = asm3_sy(a), sz = asm3_sz(a);
            xe[3 * a] = cx[sx > 0.0];
            xe[3 * a + 1] = cy[sy > 0.0];
            xe[3 * a + 2] = cz[sz > 0.0];
            Gr[0][a] = 0.125 * sx * (1.0 + sy * xi[1]) * (1.0 + sz * xi[2]);
            Gr[1][a] = 0.125 * sy * (1.0 + sx * xi[0]) * (1.0 + sz * xi[2]);
            Gr[2][a] = 0.125 * sz * (1.0 + sx * xi[0]) * (1.0 + sy * xi[1]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                J[c][d] = 0.0;
#pragma unroll
                for (int a = 0; a < 8; ++a) J[c][d] += Gr[c][a] * xe[a * 3 + d];
            }
        const double det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
                           J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
        iJ[0][0] = (J[1][1] * J[2][2] - J[1][2] * J[2][1]) / det;
        iJ[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) / det;
        iJ[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) / det;
        iJ[1][0] = (J[1][2] * J[2][0] - J[1][0] * J[2][2]) / det;
        iJ[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) / det;
        iJ[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) / det;
        iJ[2][0] = (J[1][0] * J[2][1] - J[1][1] * J[2][0]) / det;
        iJ[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) / det;
        iJ[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) / det;
        double *g = G + (size_t)t * kAsm3G;
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) g[c * 8 + a] = iJ[c][0] * Gr[0][a] + iJ[c][1] * Gr[1][a] + iJ[c][2] * Gr[2][a];
        const double kp = kappa ? kappa[((size_t)ek * (size_t)(my - 1) + (size_t)ej) * (size_t)(mx - 1) + (size_t)ei] : 1.0;
        g[24] = det;
        g[25] = 2.0 * 1.0 * det * kp;
        g[26] = 1.0 * 1.0 * det * kp;
    }
}

// ---- phase 2a: the element entries of the strip's rows, Kv[((node * 3 + c) * 8 + q) * 24 + b] = Ke[3 na + c][b] of the node's
// hexahedron q = 4 ok + 2 oj + oi at (i - 1 + oi, j - 1 + oj, k - 1 + ok), in which the node is corner na
__device__ inline void asm3_phase2a(int tid, unsigned block, int mx, int my, int mz, int k0, int nstrips, const double *G, double *Kv)
{
    const Asm3Wg w = asm3_wg(block, mx, my, k0, nstrips);
    const int count = (w.i1 - w.i0) * 576;
    for (int t = tid; t < count; t += kAsm3Threads) {
        const int node = t / 576, r = t - node * 576;
        const int c = r / 192, r2 = r - c * 192;
        const int q = r2 / 24, b = r2 - q * 24;
        const int nb = b / 3, d = b - 3 * nb;
        const int oi = q & 1, oj = (q >> 1) & 1, ok = q >> 2;
        const int ei = w.i0 + node - 1 + oi, ej = w.j - 1 + oj, ek = w.k - 1 + ok;
        if (ei < 0 || ei > mx - 2 || ej < 0 || ej > my - 2 || ek < 0 || ek > mz - 2) continue;
        const int slot = asm3_slot(w, ei, ej, ek);
        const int na = asm3_corner(1 - oi, 1 - oj, 1 - ok);
        // Ke[a*24+b] = acc[b + 24 a]: the host's index i is b = 3 nb + d, its j is a = 3 na + c
        double acc = 0.0;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const double *g = G + (size_t)(slot * 8 + p) * kAsm3G;
            const double b0 = g[nb], b1 = g[8 + nb], b2 = g[16 + nb];
            const double a0 = g[na], a1 = g[8 + na], a2 = g[16 + na];
            const double tDn = g[25], tDs = g[26];
            acc += asm3_bm<0>(d, b0, b1, b2) * tDn * asm3_bm<0>(c, a0, a1, a2);
            acc += asm3_bm<1>(d, b0, b1, b2) * tDn * asm3_bm<1>(c, a0, a1, a2);
            acc += asm3_bm<2>(d, b0, b1, b2) * tDn * asm3_bm<2>(c, a0, a1, a2);
            acc += asm3_bm<3>(d, b0, b1, b2) * tDs * asm3_bm<3>(c, a0, a1, a2);
            acc += asm3_bm<4>(d, b0, b1, b2) * tDs * asm3_bm<4>(c, a0, a1, a2);
            acc += asm3_bm<5>(d, b0, b1, b2) * tDs * asm3_bm<5>(c, a0, a1, a2);
        }
        Kv[t] = acc;
    }
}

// ---- phase 2b: the workgroup's rows, entry by entry; then the row pointers and f of the strip's rows
__device__ inline void asm3_phase2b(int tid, unsigned block, int mx, int my, int mz, int k0, int k1, int nstrips, int apply_bc,
                                    const double *G, const double *Kv, int32_t *rowptr, int32_t *colidx, double *val, double *f)
{
    const Asm3Wg w = asm3_wg(block, mx, my, k0, nstrips);
    const int j = w.j, k = w.k, i0 = w.i0, i1 = w.i1;
    const int wj = asm3_width(j, my), wk = asm3_width(k, mz);
    const int64_t X = 3 * (int64_t)mx - 2, Y = 3 * (int64_t)my - 2;
    // stored entries in front of the node line, of the strip and per unit of width in i: 9 = 3 rows x 3 columns per node pair
    const int64_t line_base = 9 * (((int64_t)asm3_prefix(k, mz) - asm3_prefix(k0, mz)) * X * Y + (int64_t)wk * asm3_prefix(j, my) * X);
    const int unit = 9 * wj * wk;
    const int x0 = asm3_prefix(i0, mx);
    const int64_t wg_base = line_base + (int64_t)unit * x0;
    const int count = unit * (asm3_prefix(i1, mx) - x0);
    for (int o = tid; o < count; o += kAsm3Threads) {
        const int i = (o / unit + x0 + 1) / 3;
        const int wi = asm3_width(i, mx);
        const int r = o - unit * (asm3_prefix(i, mx) - x0);
        const int rowlen = 3 * wi * wj * wk;
        const int c = r / rowlen;
        const int r2 = r - c * rowlen;
        const int t2 = r2 / 3, d = r2 - 3 * t2;
        const int t3 = t2 / wi, t4 = t3 / wj;
        const int ci = i - (i > 0) + (t2 - t3 * wi), cj = j - (j > 0) + (t3 - t4 * wj), ck = k - (k > 0) + t4;
        const int64_t grow = (((int64_t)k * my + j) * mx + i) * 3 + c, gcol = (((int64_t)ck * my + cj) * mx + ci) * 3 + d;
        double v = 0.0;
        // hexahedra that hold both nodes, ascending (ek, ej, ei)
        for (int ek = asm3_max(k, ck) - 1; ek <= asm3_min(k, ck); ++ek) {
            if (ek < 0 || ek > mz - 2) continue;
            for (int ej = asm3_max(j, cj) - 1; ej <= asm3_min(j, cj); ++ej) {
                if (ej < 0 || ej > my - 2) continue;
                for (int ei = asm3_max(i, ci) - 1; ei <= asm3_min(i, ci); ++ei) {
                    if (ei < 0 || ei > mx - 2) continue;
                    const int q = (ek - (k - 1)) * 4 + (ej - (j - 1)) * 2 + (ei - (i - 1));
                    const int nb = asm3_corner(ci - ei, cj - ej, ck - ek);
                    v += Kv[(((i - i0) * 3 + c) * 8 + q) * 24 + nb * 3 + d];
                }
            }
        }
        if (apply_bc && (asm3_boundary(mx, my, mz, i, j, k) || asm3_boundary(mx, my, mz, ci, cj, ck))) v = (gcol == grow) ? 1.0 : 0.0;
        colidx[wg_base + o] = (int32_t)gcol;
        val[wg_base + o] = v;
    }
    if (tid < 3 * (i1 - i0)) {
        const int i = i0 + tid / 3, c = tid % 3;
        const int wi = asm3_width(i, mx);
        const int64_t lrow = ((((int64_t)(k - k0) * my + j) * mx) + i) * 3 + c;
        rowptr[lrow] = (int32_t)(line_base + (int64_t)unit * asm3_prefix(i, mx) + (int64_t)c * 3 * wi * wj * wk);
        if (f) {
            const double gp1 = 0.57735026919;
            double fv = 0.0;
            for (int ek = k - 1; ek <= k; ++ek) {
                if (ek < 0 || ek > mz - 2) continue;
                for (int ej = j - 1; ej <= j; ++ej) {
                    if (ej < 0 || ej > my - 2) continue;
                    for (int ei = i - 1; ei <= i; ++ei) {
                        if (ei < 0 || ei > mx - 2) continue;
                        const int slot = asm3_slot(w, ei, ej, ek);
                        const int a = asm3_corner(i - ei, j - ej, k - ek);
                        const double sx = asm3_sx(a), sy = asm3_sy(a), sz = asm3_sz(a);
                        // Fe[3 a + c] of the element: body force (1, 2, 3)
                        double fe = 0.0;
                        for (int p = 0; p < 8; ++p) {
                            const double xi[3] = {asm3_sx(p) * gp1, asm3_sy(p) * gp1, asm3_sz(p) * gp1};
                            const double N = 0.125 * (1.0 + sx * xi[0]) * (1.0 + sy * xi[1]) * (1.0 + sz * xi[2]);
                            const double fac = 1.0 * G[(size_t)(slot * 8 + p) * kAsm3G + 24];
                            const double body = c == 0 ? 1.0 : c == 1 ? 2.0 : 3.0;
                            fe += fac * N * body;
                        }
                        fv += fe;
                    }
                }
            }
            f[lrow] = (apply_bc && asm3_boundary(mx, my, mz, i, j, k)) ? 0.0 : fv;
        }
    }
    if (tid == 0 && k == k1 - 1 && j == my - 1 && i1 == mx) rowptr[(int64_t)(k1 - k0) * my * mx * 3] = (int32_t)(line_base + (int64_t)unit * X);
}

__global__ __launch_bounds__(kAsm3Threads) void assemble_laplace3d_kernel(int mx, int my, int mz, int k0, int k1, int nstrips,
                                                                          const double *__restrict__ kappa, int apply_bc,
                                                                          int32_t *__restrict__ rowptr, int32_t *__restrict__ colidx,
                                                                          double *__restrict__ val, double *__restrict__ f)
{
    __shared__ double G[kAsm3Slots * 8 * kAsm3G];
    __shared__ double Kv[kAsm3Kv];
    asm3_phase1((int)threadIdx.x, blockIdx.x, mx, my, mz, k0, nstrips, kappa, G);
    __syncthreads();
    asm3_phase2a((int)threadIdx.x, blockIdx.x, mx, my, mz, k0, nstrips, G, Kv);
    __syncthreads();
    asm3_phase2b((int)threadIdx.x, blockIdx.x, mx, my, mz, k0, k1, nstrips, apply_bc, G, Kv, rowptr, colidx, val, f);
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
    hipLaunchKernelGGL(assemble_laplace3d_kernel, dim3((unsigned)grid), dim3(kAsm3Threads), 0, s, mx, my, mz, k0, k1,
                       (mx + kAsm3Strip - 1) / kAsm3Strip, kappa, apply_bc, rowptr, colidx, val, f);
    SPK_HIP(hipGetLastError());
}

int64_t assemble_laplace3d_grid(int mx, int my, int k0, int k1)
{
    return (int64_t)((mx + kAsm3Strip - 1) / kAsm3Strip) * my * (int64_t)(k1 - k0);
}

}  // namespace k
}  // namespace spk
