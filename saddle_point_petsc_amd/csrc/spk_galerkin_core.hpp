// spk_galerkin_core.hpp -- the one source of the grid-stencil Galerkin product (-spk_mg_galerkin stencil): the coarse
// operator A_{l+1} = (P^T A_l P + its transpose) / 2 of a grid-coarsened level as a gather over the <= 3^d fine node rows
// of a coarse node, with the pattern, every row pointer and every position in closed form.  The host route
// (spk_galerkin_host.cpp: galerkin_stencil_host), the kernels (spk_k_amg_setup.hip: amgs_galerkin_stencil...) and the CPU run
// (tests/host/galerkin_stencil_check.cpp) all call these functions, so host and device write the same bits because
// they execute the same expressions.  Standard library only; no ROCm.
//
// The rule, per direction of m fine and n coarse nodes (gs_dir: halved `h`, halved with an even fine side `e`):
//   coarse index c sits at fine index 2c (under e the last one, n - 1 = m / 2, at m - 1); its children are the fine
//   indices 2c - 1 (weight 1/2), 2c (1), 2c + 1 (1/2), clipped to the line; under e fine m - 1 is the child of n - 1
//   alone, with weight 1; a direction that does not halve is the identity.  A node's weight is the product over the
//   directions.  This is grid_parents (spk_amg_host.cpp) read from the coarse side.
//   S[C bs + a, C' bs + b] = sum over f in ch(C), ascending node index, over the stored entries of row f bs + a in
//   ascending position whose column is f' bs + b with f' in ch(C'), of (w(f, C) w(f', C')) A_l[f bs + a, f' bs + b],
//   added from +0.0.  Every product is exact (the weights are powers of two), so contraction cannot change a bit; it
//   stays off all the same (SPK_GS_EXACT under clang; g++ for x86-64 has no fused multiply-add to contract to).
//   A_{l+1}[r, c] = 0.5 S[r, c] + 0.5 S[c, r]: the gather writes S, then the owner of every pair (r <= c) writes both.
// The pattern: a coarse node row holds the full bs x bs blocks of its clipped 3^d-node neighbourhood, ascending.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef SPK_HD
#ifdef __HIPCC__
#define SPK_HD __host__ __device__
#else
#define SPK_HD
#endif
#endif
// contraction off inside the functions that add and multiply, not for the rest of whatever file includes this
#ifdef __clang__
#define SPK_GS_EXACT _Pragma("clang fp contract(off)")
#else
#define SPK_GS_EXACT
#endif

namespace spk {
namespace galerkin {

struct GsDir { int32_t m, n, h, e; };   // fine and coarse nodes of a direction; it halves; ... and m is even
struct GsGrid { GsDir d[3]; };          // x, y, z (a 2-D grid: z has m = n = 1)
SPK_HD inline GsGrid gs_grid(const int32_t fd[3], const int32_t cd[3])
{
    GsGrid g;
    for (int a = 0; a < 3; ++a) {
        const int32_t h = cd[a] != fd[a];
        g.d[a] = GsDir{fd[a], cd[a], h, h && !(fd[a] & 1)};
    }
    return g;
}

// ---- children and weights of one direction --------------------------------------------------------------------------
// the fine indices [lo, hi] that are children of coarse index c
SPK_HD inline void gs_children(const GsDir &d, int32_t c, int32_t *lo, int32_t *hi)
{
    if (!d.h) { *lo = *hi = c; return; }
    if (d.e && c == d.n - 1) { *lo = *hi = d.m - 1; return; }
    *lo = c > 0 ? 2 * c - 1 : 0;
    const int32_t last = d.e ? d.m - 2 : d.m - 1;   // under e fine m - 1 belongs to the last coarse index alone
    *hi = 2 * c + 1 <= last ? 2 * c + 1 : 2 * c;
}
// the weight with which fine index i is a child of coarse index c: 1, 1/2, or 0 when it is none
SPK_HD inline double gs_weight(const GsDir &d, int32_t i, int32_t c)
{
    if (!d.h) return i == c ? 1.0 : 0.0;
    if (d.e && c == d.n - 1) return i == d.m - 1 ? 1.0 : 0.0;
    if (d.e && i == d.m - 1) return 0.0;
    const int32_t t = i - 2 * c;
    return t == 0 ? 1.0 : (t == 1 || t == -1) ? 0.5 : 0.0;
}

// ---- the closed-form pattern ----------------------------------------------------------------------------------------
// the clipped neighbours [c - 1, c + 1] of index c of a line of n: the first one, how many, and how many the indices in
// front of c have together
SPK_HD inline int32_t gs_first(int32_t c) { return c > 0 ? c - 1 : 0; }
SPK_HD inline int32_t gs_width(int32_t c, int32_t n) { return (c > 0) + 1 + (c < n - 1); }
SPK_HD inline int64_t gs_prefix(int32_t c) { return c > 0 ? 3 * (int64_t)c - 1 : 0; }
SPK_HD inline int64_t gs_total(int32_t n) { return 3 * (int64_t)n - 2; }
// stored entries of a level of cd nodes
SPK_HD inline int64_t gs_nnz(const int32_t cd[3], int bs) { return gs_total(cd[0]) * gs_total(cd[1]) * gs_total(cd[2]) * bs * bs; }
// neighbour nodes of node (i, j, k), and the position of the first entry of its row a
SPK_HD inline int32_t gs_row_nodes(const int32_t cd[3], int32_t i, int32_t j, int32_t k)
{
    return gs_width(i, cd[0]) * gs_width(j, cd[1]) * gs_width(k, cd[2]);
}
SPK_HD inline int64_t gs_row_offset(const int32_t cd[3], int bs, int32_t i, int32_t j, int32_t k, int a)
{
    const int64_t nodes = gs_prefix(k) * gs_total(cd[1]) * gs_total(cd[0]) +
                          gs_width(k, cd[2]) * (gs_prefix(j) * gs_total(cd[0]) + gs_width(j, cd[1]) * gs_prefix(i));
    return (nodes * bs + (int64_t)a * gs_row_nodes(cd, i, j, k)) * bs;
}
// the rank of neighbour (i2, j2, k2) among the neighbours of (i, j, k), ascending
SPK_HD inline int32_t gs_rank(const int32_t cd[3], int32_t i, int32_t j, int32_t k, int32_t i2, int32_t j2, int32_t k2)
{
    return ((k2 - gs_first(k)) * gs_width(j, cd[1]) + (j2 - gs_first(j))) * gs_width(i, cd[0]) + (i2 - gs_first(i));
}
// the position of entry (node (i, j, k), component a; node (i2, j2, k2), component b)
SPK_HD inline int64_t gs_pos(const int32_t cd[3], int bs, int32_t i, int32_t j, int32_t k, int a, int32_t i2, int32_t j2, int32_t k2, int b)
{
    return gs_row_offset(cd, bs, i, j, k, a) + (int64_t)gs_rank(cd, i, j, k, i2, j2, k2) * bs + b;
}

// one (coarse row, neighbour node) pair: what a device thread or one turn of the host loops works on.  t counts
// rows x slots, 9 slots on a grid of one plane and 27 otherwise; the slot is (dz + 1) 9 + (dy + 1) 3 + (dx + 1), in one
// plane (dy + 1) 3 + (dx + 1).  false: the neighbour lies outside the grid
struct GsItem {
    int32_t i, j, k, a;      // the row's node and component
    int32_t i2, j2, k2;      // the neighbour node
};
SPK_HD inline int32_t gs_slots(const int32_t cd[3]) { return cd[2] > 1 ? 27 : 9; }
SPK_HD inline bool gs_item(const int32_t cd[3], int bs, int64_t t, GsItem *it)
{
    const int32_t ns = gs_slots(cd), q = (int32_t)(t % ns);
    const int64_t r = t / ns;
    const int32_t node = (int32_t)(r / bs);
    it->a = (int32_t)(r - (int64_t)node * bs);
    it->i = node % cd[0], it->j = (node / cd[0]) % cd[1], it->k = node / cd[0] / cd[1];
    it->i2 = it->i + q % 3 - 1, it->j2 = it->j + (q / 3) % 3 - 1, it->k2 = ns == 27 ? it->k + q / 9 - 1 : it->k;
    return it->i2 >= 0 && it->i2 < cd[0] && it->j2 >= 0 && it->j2 < cd[1] && it->k2 >= 0 && it->k2 < cd[2];
}
SPK_HD inline int64_t gs_items(const int32_t cd[3], int bs) { return (int64_t)cd[0] * cd[1] * cd[2] * bs * gs_slots(cd); }

// ---- the gather -----------------------------------------------------------------------------------------------------
// S[row, (i2, j2, k2) bs + b], b < BS, of one item, and with it the item's share of the pattern: the row pointer (the
// item of the node itself writes it; the last row the end too), the columns and the raw sums
template <int BS>
SPK_HD inline void gs_gather(const GsGrid &g, const int32_t *arp, const int32_t *aci, const double *av, const GsItem &it,
                             int32_t *rp, int32_t *ci, double *v)
{
    SPK_GS_EXACT
    const int32_t fx = g.d[0].m, fy = g.d[1].m;
    const int32_t cd[3] = {g.d[0].n, g.d[1].n, g.d[2].n};
    double acc[BS];
    for (int b = 0; b < BS; ++b) acc[b] = 0.0;
    int32_t xl, xh, yl, yh, zl, zh;
    gs_children(g.d[0], it.i, &xl, &xh);
    gs_children(g.d[1], it.j, &yl, &yh);
    gs_children(g.d[2], it.k, &zl, &zh);
    for (int32_t z = zl; z <= zh; ++z)
        for (int32_t y = yl; y <= yh; ++y)
            for (int32_t x = xl; x <= xh; ++x) {
                const double w = gs_weight(g.d[2], z, it.k) * gs_weight(g.d[1], y, it.j) * gs_weight(g.d[0], x, it.i);
                const int64_t row = ((int64_t)(z * fy + y) * fx + x) * BS + it.a;
                for (int32_t p = arp[row]; p < arp[row + 1]; ++p) {
                    const int32_t col = aci[p], f2 = col / BS, b = col - f2 * BS;
                    const int32_t x2 = f2 % fx, y2 = (f2 / fx) % fy, z2 = f2 / fx / fy;
                    const double w2 = gs_weight(g.d[2], z2, it.k2) * gs_weight(g.d[1], y2, it.j2) * gs_weight(g.d[0], x2, it.i2);
                    if (w2 == 0.0) continue;
                    const double t = (w * w2) * av[p];
                    for (int bb = 0; bb < BS; ++bb)   // (a constant index: the sums stay in registers)
                        if (bb == b) acc[bb] = acc[bb] + t;
                }
            }
    const int64_t off = gs_row_offset(cd, BS, it.i, it.j, it.k, it.a);
    if (it.i2 == it.i && it.j2 == it.j && it.k2 == it.k) {
        const int64_t r = ((int64_t)(it.k * cd[1] + it.j) * cd[0] + it.i) * BS + it.a;
        rp[r] = (int32_t)off;
        if (r + 1 == (int64_t)cd[0] * cd[1] * cd[2] * BS) rp[r + 1] = (int32_t)(off + (int64_t)gs_row_nodes(cd, it.i, it.j, it.k) * BS);
    }
    const int64_t p0 = off + (int64_t)gs_rank(cd, it.i, it.j, it.k, it.i2, it.j2, it.k2) * BS;
    const int32_t c0 = ((it.k2 * cd[1] + it.j2) * cd[0] + it.i2) * BS;
    for (int b = 0; b < BS; ++b) {
        ci[p0 + b] = c0 + b;
        v[p0 + b] = acc[b];
    }
}

// A[r, c] = A[c, r] = 0.5 S[r, c] + 0.5 S[c, r] in place, by the owner of the pair: the item whose row is not behind
// the column.  No two items touch the same pair
template <int BS>
SPK_HD inline void gs_symmetrise(const int32_t cd[3], const GsItem &it, double *v)
{
    SPK_GS_EXACT
    const int64_t r = ((int64_t)(it.k * cd[1] + it.j) * cd[0] + it.i) * BS + it.a;
    const int64_t c0 = ((int64_t)(it.k2 * cd[1] + it.j2) * cd[0] + it.i2) * BS;
    for (int b = 0; b < BS; ++b) {
        if (c0 + b < r) continue;
        const int64_t p = gs_pos(cd, BS, it.i, it.j, it.k, it.a, it.i2, it.j2, it.k2, b);
        const int64_t q = gs_pos(cd, BS, it.i2, it.j2, it.k2, b, it.i, it.j, it.k, it.a);
        const double t = 0.5 * v[p] + 0.5 * v[q];
        v[p] = t;
        v[q] = t;
    }
}

// level 0's one condition: every stored column node of row `row` lies within one node of the row's node in every
// direction.  Returns the first offending column, or -1
SPK_HD inline int32_t gs_check_row(const int32_t fd[3], int bs, const int32_t *arp, const int32_t *aci, int64_t row)
{
    const int32_t f = (int32_t)(row / bs);
    const int32_t x = f % fd[0], y = (f / fd[0]) % fd[1], z = f / fd[0] / fd[1];
    for (int32_t p = arp[row]; p < arp[row + 1]; ++p) {
        const int32_t f2 = aci[p] / bs;
        const int32_t dx = f2 % fd[0] - x, dy = (f2 / fd[0]) % fd[1] - y, dz = f2 / fd[0] / fd[1] - z;
        if (dx < -1 || dx > 1 || dy < -1 || dy > 1 || dz < -1 || dz > 1) return aci[p];
    }
    return -1;
}

}  // namespace galerkin
}  // namespace spk
