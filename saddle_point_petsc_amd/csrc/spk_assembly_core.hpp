// spk_assembly_core.hpp -- the one source of the assembly arithmetic: the index algebra of the node grid, the element
// routines of the 2-D (Q1 quadrilateral, dof 2) and 3-D (Q1 hexahedron, dof 3) discretisations entry by entry, and the
// phases of the two device kernels as plain functions of (thread, workgroup).  The host assembler (spk_assembly.cpp),
// the kernels (spk_k_assembly.hip, spk_k_assembly3d.hip) and the CPU run of the kernels
// (tests/host/assembly_kernel_check.cpp) all call these functions, so host and device write the same bits because they
// execute the same expressions, not because two texts agree.  Standard library only; no ROCm.
//
// Contraction must stay off wherever this is compiled: the pragma below under clang, -ffp-contract=off with g++.
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define SPK_HD __host__ __device__
#else
#define SPK_HD
#endif
#ifdef __clang__
#pragma clang fp contract(off)
#define SPK_UNROLL _Pragma("unroll")
#else
#define SPK_UNROLL
#endif

namespace spk {
namespace assembly {

// ---- index algebra -------------------------------------------------------------------------------------------------
SPK_HD inline double coord(int i, int m) { return 0.0 + (1.0 / (double)(m - 1)) * (double)i; }
// stored neighbours of node i of a line of m, and the sum of the widths of the nodes in front of it
SPK_HD inline int width(int i, int m) { return (i > 0) + 1 + (i < m - 1); }
SPK_HD inline int prefix(int i, int m) { return 3 * i - (i > 0) - (i > m - 1); }
// local node number of the corner at offset (oi, oj[, ok]) from the element origin
SPK_HD inline int corner(int oi, int oj) { return oi == 0 ? (oj == 0 ? 0 : 1) : (oj == 0 ? 3 : 2); }
SPK_HD inline int corner(int oi, int oj, int ok) { return corner(oi, oj) + 4 * ok; }
SPK_HD inline bool on_boundary(int mx, int my, int i, int j) { return i == 0 || i == mx - 1 || j == 0 || j == my - 1; }
SPK_HD inline bool on_boundary(int mx, int my, int mz, int i, int j, int k)
{
    return on_boundary(mx, my, i, j) || k == 0 || k == mz - 1;
}
SPK_HD inline int imin(int a, int b) { return a < b ? a : b; }
SPK_HD inline int imax(int a, int b) { return a > b ? a : b; }
// closed-form entry offsets: stored entries of a slab that starts at line j0 (plane k0) in front of node line j (j, k)
SPK_HD inline int64_t line_offset(int mx, int my, int j0, int j)
{
    return 4 * (3 * (int64_t)mx - 2) * ((int64_t)prefix(j, my) - prefix(j0, my));
}
SPK_HD inline int64_t line_offset(int mx, int my, int mz, int k0, int j, int k)
{
    const int64_t X = 3 * (int64_t)mx - 2, Y = 3 * (int64_t)my - 2;
    return 9 * (((int64_t)prefix(k, mz) - prefix(k0, mz)) * X * Y + (int64_t)width(k, mz) * prefix(j, my) * X);
}
// corner a of an element and Gauss point p of the hexahedron: the signs (-1,-1,-1) (-1,1,-1) (1,1,-1) (1,-1,-1), then the
// same at +1 in z; the first four are the quadrilateral's
SPK_HD inline double sgn_x(int a) { return (a & 3) >= 2 ? 1.0 : -1.0; }
SPK_HD inline double sgn_y(int a) { return (a & 3) == 1 || (a & 3) == 2 ? 1.0 : -1.0; }
SPK_HD inline double sgn_z(int a) { return a >= 4 ? 1.0 : -1.0; }
constexpr double kGauss = 0.57735026919;   // the reference's truncated abscissa (Discretization.c:52-55)

// ---- 2-D element ---------------------------------------------------------------------------------------------------
constexpr int kG2 = 9;   // per Gauss point: gx[2][4], det J
SPK_HD inline void quad_coords(int mx, int my, int ei, int ej, double *xe)
{
    xe[0] = coord(ei, mx);     xe[1] = coord(ej, my);
    xe[2] = coord(ei, mx);     xe[3] = coord(ej + 1, my);
    xe[4] = coord(ei + 1, mx); xe[5] = coord(ej + 1, my);
    xe[6] = coord(ei + 1, mx); xe[7] = coord(ej, my);
}
SPK_HD inline double shape2(int n, int p)
{
    const double xi = sgn_x(p) * kGauss, eta = sgn_y(p) * kGauss;
    return n == 0 ? 0.25 * (1.0 - xi) * (1.0 - eta)
         : n == 1 ? 0.25 * (1.0 - xi) * (1.0 + eta)
         : n == 2 ? 0.25 * (1.0 + xi) * (1.0 + eta)
                  : 0.25 * (1.0 + xi) * (1.0 - eta);
}
// Gauss point p of the element with corners xe[8]: physical gradients g[0..3] (d/dx), g[4..7] (d/dy) and det J in g[8]
SPK_HD inline void gauss2(int p, const double *xe, double *g)
{
    const double xi = sgn_x(p) * kGauss, eta = sgn_y(p) * kGauss;
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
    SPK_UNROLL
    for (int c = 0; c < 2; ++c)
        SPK_UNROLL
        for (int d = 0; d < 2; ++d)
            SPK_UNROLL
            for (int i = 0; i < 4; ++i) J[c][d] += dN[c][i] * xe[2 * i + d];
    const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    const double i00 = J[1][1] / det, i01 = -J[0][1] / det, i10 = -J[1][0] / det, i11 = J[0][0] / det;
    SPK_UNROLL
    for (int i = 0; i < 4; ++i) {
        g[i] = i00 * dN[0][i] + i01 * dN[1][i];
        g[4 + i] = i10 * dN[0][i] + i11 * dN[1][i];
    }
    g[8] = det;
}
// entry acc[i + 8 j] of Ke: Gauss points outermost, the three strain rows (exx, eyy, 2exy; D = diag(2,2,1)) inside, Bm's
// structural zeros multiplied through.  ke2_terms adds the three terms of one Gauss point from the two columns of Bm
// (bm2) and tD (td2); the host loops over the points outside its loop over the entries and keeps the columns, so that
// independent additions are in flight, with the same sequence of additions into an entry.  ke2_point is that step from
// the point's g[kG2], ke2_entry the whole entry from the four points G[4][kG2].
// b[k * ld] = Bm[k][i], k = 0..2: Bm[k][2 n] = (gx0, 0, gx1), Bm[k][2 n + 1] = (0, gx1, gx0)
SPK_HD inline void bm2(const double *g, int i, double *b, int ld = 1)
{
    const double gx = g[i >> 1], gy = g[4 + (i >> 1)];   // (both are needed whichever component i is: loaded without a branch)
    const bool x = (i & 1) == 0;
    b[0] = x ? gx : 0.0;
    b[ld] = x ? 0.0 : gy;
    b[2 * ld] = x ? gy : gx;
}
SPK_HD inline void td2(const double *g, double coeff, double *tD)
{
    tD[0] = 2.0 * 1.0 * g[8] * coeff;
    tD[1] = 2.0 * 1.0 * g[8] * coeff;
    tD[2] = 1.0 * g[8] * coeff;
}
SPK_HD inline double ke2_terms(double acc, const double *bi, const double *tD, const double *bj, int ld = 1)
{
    acc += bi[0] * tD[0] * bj[0];
    acc += bi[ld] * tD[1] * bj[ld];
    acc += bi[2 * ld] * tD[2] * bj[2 * ld];
    return acc;
}
SPK_HD inline double ke2_point(double acc, const double *g, double coeff, int i, int j)
{
    double bi[3], bj[3], tD[3];
    bm2(g, i, bi);
    bm2(g, j, bj);
    td2(g, coeff, tD);
    return ke2_terms(acc, bi, tD, bj);
}
SPK_HD inline double ke2_entry(const double *G, const double *coeff, int i, int j)
{
    double acc = 0.0;
    SPK_UNROLL
    for (int p = 0; p < 4; ++p) acc = ke2_point(acc, G + p * kG2, coeff[p], i, j);
    return acc;
}
// entry Fe[2 n + c]: FormRHS (Discretization.c:397-402), body force (1, 2)
SPK_HD inline double fe2_entry(const double *G, int n, int c)
{
    double fe = 0.0;
    SPK_UNROLL
    for (int p = 0; p < 4; ++p) {
        const double fac = 1.0 * G[p * kG2 + 8];
        const double body = c ? 2.0 : 1.0;
        fe += fac * shape2(n, p) * body;
    }
    return fe;
}

// ---- 3-D element ---------------------------------------------------------------------------------------------------
constexpr int kG3 = 27;   // per Gauss point: Gx[3][8], det J, tD of the normal and of the shear strain rows
SPK_HD inline void hex_coords(int mx, int my, int mz, int ei, int ej, int ek, double *xe)
{
    const double cx[2] = {coord(ei, mx), coord(ei + 1, mx)};
    const double cy[2] = {coord(ej, my), coord(ej + 1, my)};
    const double cz[2] = {coord(ek, mz), coord(ek + 1, mz)};
    SPK_UNROLL
    for (int a = 0; a < 8; ++a) {
        xe[3 * a] = cx[sgn_x(a) > 0.0];
        xe[3 * a + 1] = cy[sgn_y(a) > 0.0];
        xe[3 * a + 2] = cz[sgn_z(a) > 0.0];
    }
}
SPK_HD inline double shape3(int a, int p)
{
    const double xi[3] = {sgn_x(p) * kGauss, sgn_y(p) * kGauss, sgn_z(p) * kGauss};
    return 0.125 * (1.0 + sgn_x(a) * xi[0]) * (1.0 + sgn_y(a) * xi[1]) * (1.0 + sgn_z(a) * xi[2]);
}
// Gauss point p of the hexahedron with corners xe[24] and coefficient kp: g[c * 8 + a] = Gx[c][a], g[24] = det J,
// g[25] = tD of the strain rows 0..2, g[26] = of the rows 3..5
SPK_HD inline void gauss3(int p, const double *xe, double kp, double *g)
{
    const double xi[3] = {sgn_x(p) * kGauss, sgn_y(p) * kGauss, sgn_z(p) * kGauss};
    double Gr[3][8], J[3][3], iJ[3][3];
    SPK_UNROLL
    for (int a = 0; a < 8; ++a) {
        const double sx = sgn_x(a), sy = sgn_y(a), sz = sgn_z(a);
        Gr[0][a] = 0.125 * sx * (1.0 + sy * xi[1]) * (1.0 + sz * xi[2]);
        Gr[1][a] = 0.125 * sy * (1.0 + sx * xi[0]) * (1.0 + sz * xi[2]);
        Gr[2][a] = 0.125 * sz * (1.0 + sx * xi[0]) * (1.0 + sy * xi[1]);
    }
    SPK_UNROLL
    for (int c = 0; c < 3; ++c)
        SPK_UNROLL
        for (int d = 0; d < 3; ++d) {
            J[c][d] = 0.0;
            SPK_UNROLL
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
    SPK_UNROLL
    for (int a = 0; a < 8; ++a)
        SPK_UNROLL
        for (int c = 0; c < 3; ++c) g[c * 8 + a] = iJ[c][0] * Gr[0][a] + iJ[c][1] * Gr[1][a] + iJ[c][2] * Gr[2][a];
    g[24] = det;
    g[25] = 2.0 * 1.0 * det * kp;
    g[26] = 1.0 * 1.0 * det * kp;
}
// Bm[row][3 n + comp] of the strain-displacement matrix: g0, g1, g2 are Gx[0..2][n]; 0.0 at its structural zeros
template <int ROW>
SPK_HD inline double bm3(int comp, double g0, double g1, double g2)
{
    if (ROW == 0) return comp == 0 ? g0 : 0.0;
    if (ROW == 1) return comp == 1 ? g1 : 0.0;
    if (ROW == 2) return comp == 2 ? g2 : 0.0;
    if (ROW == 3) return comp == 0 ? g1 : comp == 1 ? g0 : 0.0;
    if (ROW == 4) return comp == 1 ? g2 : comp == 2 ? g1 : 0.0;
    return comp == 0 ? g2 : comp == 2 ? g0 : 0.0;
}
// entry acc[b + 24 a] = Ke[a * 24 + b], a = 3 na + c, b = 3 nb + d: Gauss points outermost, the six strain rows inside, each
// term Bm[k][b] * tD[k] * Bm[k][a] with the zeros multiplied through.  ke3_point adds the six terms of one Gauss point
// g[kG3] (the host's loop, as in 2-D); ke3_entry is the whole entry from the eight points G[8][kG3].
SPK_HD inline double ke3_point(double acc, const double *g, int nb, int d, int na, int c)
{
    const double b0 = g[nb], b1 = g[8 + nb], b2 = g[16 + nb];
    const double a0 = g[na], a1 = g[8 + na], a2 = g[16 + na];
    const double tDn = g[25], tDs = g[26];
    acc += bm3<0>(d, b0, b1, b2) * tDn * bm3<0>(c, a0, a1, a2);
    acc += bm3<1>(d, b0, b1, b2) * tDn * bm3<1>(c, a0, a1, a2);
    acc += bm3<2>(d, b0, b1, b2) * tDn * bm3<2>(c, a0, a1, a2);
    acc += bm3<3>(d, b0, b1, b2) * tDs * bm3<3>(c, a0, a1, a2);
    acc += bm3<4>(d, b0, b1, b2) * tDs * bm3<4>(c, a0, a1, a2);
    acc += bm3<5>(d, b0, b1, b2) * tDs * bm3<5>(c, a0, a1, a2);
    return acc;
}
SPK_HD inline double ke3_entry(const double *G, int nb, int d, int na, int c)
{
    double acc = 0.0;
    SPK_UNROLL
    for (int p = 0; p < 8; ++p) acc = ke3_point(acc, G + p * kG3, nb, d, na, c);
    return acc;
}
// entry Fe[3 a + c]: body force (1, 2, 3)
SPK_HD inline double fe3_entry(const double *G, int a, int c)
{
    double fe = 0.0;
    for (int p = 0; p < 8; ++p) {
        const double fac = 1.0 * G[p * kG3 + 24];
        const double body = c == 0 ? 1.0 : c == 1 ? 2.0 : 3.0;
        fe += fac * shape3(a, p) * body;
    }
    return fe;
}

// ---- the 2-D kernel (spk_k_assembly.hip): one workgroup per node line j and strip of kStrip2 nodes -------------------
constexpr int kStrip2 = 32;               // nodes of a line per workgroup
constexpr int kElems2 = kStrip2 + 1;      // elements of one element line that touch them
constexpr int kSlots2 = 2 * kElems2;      // element lines j-1 (slots 0..) and j (slots kElems2..)
// the workgroup's LDS, in doubles: Ke, Fe, the Gauss points, the coefficient per slot
constexpr int kLdsKe2 = kSlots2 * 64, kLdsFe2 = kSlots2 * 8, kLdsG2 = kSlots2 * 4 * kG2, kLdsKap2 = kSlots2;
inline int strips2(int mx) { return (mx + kStrip2 - 1) / kStrip2; }
inline int64_t grid2(int mx, int j0, int j1) { return (int64_t)strips2(mx) * (j1 - j0); }

struct Wg2 {
    int j, i0, i1;
};
SPK_HD inline Wg2 wg2(unsigned block, int mx, int j0, int nstrips)
{
    Wg2 w;
    w.j = j0 + (int)(block / (unsigned)nstrips);
    w.i0 = (int)(block % (unsigned)nstrips) * kStrip2;
    w.i1 = imin(w.i0 + kStrip2, mx);
    return w;
}
// element of slot: ej = j - 1 + slot / kElems2, ei = i0 - 1 + slot % kElems2; whether it exists and touches the strip
SPK_HD inline bool live2(const Wg2 &w, int mx, int my, int slot, int &ei, int &ej)
{
    const int l = slot / kElems2;
    ej = w.j - 1 + l;
    ei = w.i0 - 1 + (slot - l * kElems2);
    return ej >= 0 && ej <= my - 2 && ei >= 0 && ei <= mx - 2 && ei <= w.i1 - 1;
}
SPK_HD inline int slot2(const Wg2 &w, int ei, int ej) { return (ej - (w.j - 1)) * kElems2 + (ei - (w.i0 - 1)); }

// phase 1a: one thread per (element, Gauss point) of the two element lines over the strip
SPK_HD inline void asm2_phase1a(int tid, int nthreads, unsigned block, int mx, int my, int j0, int nstrips, const double *kappa, double *G,
                                double *kap)
{
    const Wg2 w = wg2(block, mx, j0, nstrips);
    for (int t = tid; t < kSlots2 * 4; t += nthreads) {
        const int p = t & 3, slot = t >> 2;
        int ei, ej;
        if (!live2(w, mx, my, slot, ei, ej)) continue;
        double xe[8];
        quad_coords(mx, my, ei, ej, xe);
        gauss2(p, xe, G + (size_t)t * kG2);
        if (p == 0) kap[slot] = kappa ? kappa[(size_t)ej * (size_t)(mx - 1) + (size_t)ei] : 1.0;
    }
}
// phase 1b: one thread per entry of Ke (64 per element) and of Fe (8)
SPK_HD inline void asm2_phase1b(int tid, int nthreads, unsigned block, int mx, int my, int j0, int nstrips, const double *G, const double *kap,
                                double *Ke, double *Fe)
{
    const Wg2 w = wg2(block, mx, j0, nstrips);
    int ei, ej;
    for (int t = tid; t < kSlots2 * 64; t += nthreads) {
        const int slot = t >> 6;
        if (!live2(w, mx, my, slot, ei, ej)) continue;
        const double kp = kap[slot];   // one value per element, at its four Gauss points
        const double coeff[4] = {kp, kp, kp, kp};
        Ke[t] = ke2_entry(G + (size_t)slot * 4 * kG2, coeff, t & 7, (t >> 3) & 7);
    }
    for (int t = tid; t < kSlots2 * 8; t += nthreads) {
        const int slot = t >> 3;
        if (!live2(w, mx, my, slot, ei, ej)) continue;
        Fe[t] = fe2_entry(G + (size_t)slot * 4 * kG2, (t >> 1) & 3, t & 1);
    }
}
// phase 2: the threads stride over the workgroup's contiguous output range, entry -> (node, c, dj, di, d) by index
// arithmetic; then the row pointers and f of the strip's rows (nthreads >= 2 kStrip2)
SPK_HD inline void asm2_phase2(int tid, int nthreads, unsigned block, int mx, int my, int j0, int j1, int nstrips, int apply_bc,
                               const double *Ke, const double *Fe, int32_t *rowptr, int32_t *colidx, double *val, double *f)
{
    const Wg2 w = wg2(block, mx, j0, nstrips);
    const int j = w.j, i0 = w.i0, i1 = w.i1;
    const int wj = width(j, my);
    const int64_t line_base = line_offset(mx, my, j0, j);
    const int x0 = prefix(i0, mx);
    const int64_t wg_base = line_base + (int64_t)4 * wj * x0;
    const int count = 4 * wj * (prefix(i1, mx) - x0);
    for (int o = tid; o < count; o += nthreads) {
        const int i = (o / (4 * wj) + x0 + 1) / 3;
        const int wi = width(i, mx);
        const int r = o - 4 * wj * (prefix(i, mx) - x0);
        const int rowlen = 2 * wi * wj;
        const int c = r >= rowlen ? 1 : 0;
        const int r2 = r - c * rowlen;
        const int d = r2 & 1, t2 = r2 >> 1;
        const int djx = t2 / wi;
        const int cj = j - (j > 0) + djx, ci = i - (i > 0) + (t2 - djx * wi);
        const int64_t grow = ((int64_t)j * mx + i) * 2 + c, gcol = ((int64_t)cj * mx + ci) * 2 + d;
        double v = 0.0;
        // elements that hold both nodes, ascending (ej, ei)
        for (int ej = imax(j, cj) - 1; ej <= imin(j, cj); ++ej) {
            if (ej < 0 || ej > my - 2) continue;
            for (int ei = imax(i, ci) - 1; ei <= imin(i, ci); ++ei) {
                if (ei < 0 || ei > mx - 2) continue;
                const int a = corner(i - ei, j - ej) * 2 + c;
                const int b = corner(ci - ei, cj - ej) * 2 + d;
                v += Ke[slot2(w, ei, ej) * 64 + a * 8 + b];
            }
        }
        if (apply_bc && (on_boundary(mx, my, i, j) || on_boundary(mx, my, ci, cj))) v = (gcol == grow) ? 1.0 : 0.0;
        colidx[wg_base + o] = (int32_t)gcol;
        val[wg_base + o] = v;
    }
    if (tid < 2 * (i1 - i0)) {
        const int i = i0 + (tid >> 1), c = tid & 1;
        const int wi = width(i, mx);
        const int64_t lrow = ((int64_t)(j - j0) * mx + i) * 2 + c;
        rowptr[lrow] = (int32_t)(line_base + (int64_t)4 * wj * prefix(i, mx) + (int64_t)c * 2 * wi * wj);
        if (f) {
            double fv = 0.0;
            for (int ej = j - 1; ej <= j; ++ej) {
                if (ej < 0 || ej > my - 2) continue;
                for (int ei = i - 1; ei <= i; ++ei) {
                    if (ei < 0 || ei > mx - 2) continue;
                    fv += Fe[slot2(w, ei, ej) * 8 + corner(i - ei, j - ej) * 2 + c];
                }
            }
            f[lrow] = (apply_bc && on_boundary(mx, my, i, j)) ? 0.0 : fv;
        }
    }
    if (tid == 0 && j == j1 - 1 && i1 == mx)
        rowptr[(int64_t)(j1 - j0) * mx * 2] = (int32_t)(line_base + 4 * (3 * (int64_t)mx - 2) * wj);
}

// ---- the 3-D kernel (spk_k_assembly3d.hip): one workgroup per node line (j, k) and strip of kStrip3 nodes ------------
constexpr int kStrip3 = 4;                  // nodes of a line per workgroup
constexpr int kElems3 = kStrip3 + 1;        // elements of one element line that touch them
constexpr int kSlots3 = 4 * kElems3;        // element lines (ej, ek) = (j-1, k-1), (j, k-1), (j-1, k), (j, k)
// the workgroup's LDS, in doubles: the Gauss points, and the element entries of the strip's rows (node, c, hexahedron, b)
constexpr int kLdsG3 = kSlots3 * 8 * kG3, kLdsKv3 = kStrip3 * 3 * 8 * 24;
inline int strips3(int mx) { return (mx + kStrip3 - 1) / kStrip3; }
inline int64_t grid3(int mx, int my, int k0, int k1) { return (int64_t)strips3(mx) * my * (int64_t)(k1 - k0); }

struct Wg3 {
    int j, k, i0, i1;
};
SPK_HD inline Wg3 wg3(unsigned block, int mx, int my, int k0, int nstrips)
{
    Wg3 w;
    const int line = (int)(block / (unsigned)nstrips);
    w.i0 = (int)(block % (unsigned)nstrips) * kStrip3;
    w.i1 = imin(w.i0 + kStrip3, mx);
    w.j = line % my;
    w.k = k0 + line / my;
    return w;
}
// element of slot: ej = j - 1 + (l & 1), ek = k - 1 + (l >> 1), ei = i0 - 1 + slot % kElems3; whether it exists and touches the strip
SPK_HD inline bool live3(const Wg3 &w, int mx, int my, int mz, int slot, int &ei, int &ej, int &ek)
{
    const int l = slot / kElems3;
    ej = w.j - 1 + (l & 1);
    ek = w.k - 1 + (l >> 1);
    ei = w.i0 - 1 + (slot - l * kElems3);
    return ek >= 0 && ek <= mz - 2 && ej >= 0 && ej <= my - 2 && ei >= 0 && ei <= mx - 2 && ei <= w.i1 - 1;
}
SPK_HD inline int slot3(const Wg3 &w, int ei, int ej, int ek)
{
    return ((ek - (w.k - 1)) * 2 + (ej - (w.j - 1))) * kElems3 + (ei - (w.i0 - 1));
}

// phase 1: one thread per (element, Gauss point) of the four element lines over the strip
SPK_HD inline void asm3_phase1(int tid, int nthreads, unsigned block, int mx, int my, int mz, int k0, int nstrips, const double *kappa,
                               double *G)
{
    const Wg3 w = wg3(block, mx, my, k0, nstrips);
    for (int t = tid; t < kSlots3 * 8; t += nthreads) {
        const int p = t & 7, slot = t >> 3;
        int ei, ej, ek;
        if (!live3(w, mx, my, mz, slot, ei, ej, ek)) continue;
        double xe[24];
        hex_coords(mx, my, mz, ei, ej, ek, xe);
        const double kp = kappa ? kappa[((size_t)ek * (size_t)(my - 1) + (size_t)ej) * (size_t)(mx - 1) + (size_t)ei] : 1.0;
        gauss3(p, xe, kp, G + (size_t)t * kG3);
    }
}
// phase 2a: the element entries of the strip's rows, Kv[((node * 3 + c) * 8 + q) * 24 + b] = Ke[3 na + c][b] of the node's
// hexahedron q = 4 ok + 2 oj + oi at (i - 1 + oi, j - 1 + oj, k - 1 + ok), in which the node is corner na
SPK_HD inline void asm3_phase2a(int tid, int nthreads, unsigned block, int mx, int my, int mz, int k0, int nstrips, const double *G,
                                double *Kv)
{
    const Wg3 w = wg3(block, mx, my, k0, nstrips);
    const int count = (w.i1 - w.i0) * 576;
    for (int t = tid; t < count; t += nthreads) {
        const int node = t / 576, r = t - node * 576;
        const int c = r / 192, r2 = r - c * 192;
        const int q = r2 / 24, b = r2 - q * 24;
        const int nb = b / 3, d = b - 3 * nb;
        const int oi = q & 1, oj = (q >> 1) & 1, ok = q >> 2;
        const int ei = w.i0 + node - 1 + oi, ej = w.j - 1 + oj, ek = w.k - 1 + ok;
        if (ei < 0 || ei > mx - 2 || ej < 0 || ej > my - 2 || ek < 0 || ek > mz - 2) continue;
        Kv[t] = ke3_entry(G + (size_t)slot3(w, ei, ej, ek) * 8 * kG3, nb, d, corner(1 - oi, 1 - oj, 1 - ok), c);
    }
}
// phase 2b: the workgroup's rows, entry by entry; then the row pointers and f of the strip's rows (nthreads >= 3 kStrip3)
SPK_HD inline void asm3_phase2b(int tid, int nthreads, unsigned block, int mx, int my, int mz, int k0, int k1, int nstrips, int apply_bc,
                                const double *G, const double *Kv, int32_t *rowptr, int32_t *colidx, double *val, double *f)
{
    const Wg3 w = wg3(block, mx, my, k0, nstrips);
    const int j = w.j, k = w.k, i0 = w.i0, i1 = w.i1;
    const int wj = width(j, my), wk = width(k, mz);
    // stored entries in front of the node line, of the strip and per unit of width in i: 9 = 3 rows x 3 columns per node pair
    const int64_t line_base = line_offset(mx, my, mz, k0, j, k);
    const int unit = 9 * wj * wk;
    const int x0 = prefix(i0, mx);
    const int64_t wg_base = line_base + (int64_t)unit * x0;
    const int count = unit * (prefix(i1, mx) - x0);
    for (int o = tid; o < count; o += nthreads) {
        const int i = (o / unit + x0 + 1) / 3;
        const int wi = width(i, mx);
        const int r = o - unit * (prefix(i, mx) - x0);
        const int rowlen = 3 * wi * wj * wk;
        const int c = r / rowlen;
        const int r2 = r - c * rowlen;
        const int t2 = r2 / 3, d = r2 - 3 * t2;
        const int t3 = t2 / wi, t4 = t3 / wj;
        const int ci = i - (i > 0) + (t2 - t3 * wi), cj = j - (j > 0) + (t3 - t4 * wj), ck = k - (k > 0) + t4;
        const int64_t grow = (((int64_t)k * my + j) * mx + i) * 3 + c, gcol = (((int64_t)ck * my + cj) * mx + ci) * 3 + d;
        double v = 0.0;
        // hexahedra that hold both nodes, ascending (ek, ej, ei)
        for (int ek = imax(k, ck) - 1; ek <= imin(k, ck); ++ek) {
            if (ek < 0 || ek > mz - 2) continue;
            for (int ej = imax(j, cj) - 1; ej <= imin(j, cj); ++ej) {
                if (ej < 0 || ej > my - 2) continue;
                for (int ei = imax(i, ci) - 1; ei <= imin(i, ci); ++ei) {
                    if (ei < 0 || ei > mx - 2) continue;
                    const int q = (ek - (k - 1)) * 4 + (ej - (j - 1)) * 2 + (ei - (i - 1));
                    const int nb = corner(ci - ei, cj - ej, ck - ek);
                    v += Kv[(((i - i0) * 3 + c) * 8 + q) * 24 + nb * 3 + d];
                }
            }
        }
        if (apply_bc && (on_boundary(mx, my, mz, i, j, k) || on_boundary(mx, my, mz, ci, cj, ck))) v = (gcol == grow) ? 1.0 : 0.0;
        colidx[wg_base + o] = (int32_t)gcol;
        val[wg_base + o] = v;
    }
    if (tid < 3 * (i1 - i0)) {
        const int i = i0 + tid / 3, c = tid % 3;
        const int wi = width(i, mx);
        const int64_t lrow = ((((int64_t)(k - k0) * my + j) * mx) + i) * 3 + c;
        rowptr[lrow] = (int32_t)(line_base + (int64_t)unit * prefix(i, mx) + (int64_t)c * 3 * wi * wj * wk);
        if (f) {
            double fv = 0.0;
            for (int ek = k - 1; ek <= k; ++ek) {
                if (ek < 0 || ek > mz - 2) continue;
                for (int ej = j - 1; ej <= j; ++ej) {
                    if (ej < 0 || ej > my - 2) continue;
                    for (int ei = i - 1; ei <= i; ++ei) {
                        if (ei < 0 || ei > mx - 2) continue;
                        fv += fe3_entry(G + (size_t)slot3(w, ei, ej, ek) * 8 * kG3, corner(i - ei, j - ej, k - ek), c);
                    }
                }
            }
            f[lrow] = (apply_bc && on_boundary(mx, my, mz, i, j, k)) ? 0.0 : fv;
        }
    }
    if (tid == 0 && k == k1 - 1 && j == my - 1 && i1 == mx)
        rowptr[(int64_t)(k1 - k0) * my * mx * 3] = (int32_t)(line_base + (int64_t)unit * (3 * (int64_t)mx - 2));
}

}  // namespace assembly
}  // namespace spk
