// spk_constraints_core.hpp -- the one source of the constraint block's arithmetic: B (the mean and moment rows of
// SpkAssembleOperator_Constraints[3D], spk_assembly.cpp) over a rank's slab of whole node lines (2-D) or planes (3-D), in
// the three forms KSPSetOperators keeps: B by rows with localised columns, B^T by rows, and the column-window pointers.
// Everything is closed form: interior node (i, j[, k]), component c, holds exactly two entries -- row c (the mean, value
// w) and row c + dof (the moment about the centre along axis c, value w * (coord - 0.5)) -- and a boundary node holds
// none.  The kernels (spk_k_constraints.hip) and the CPU check (tests/host/constraints_core_check.cpp) call these
// functions; the values are the host generator's expressions in the host generator's order.  Standard library only.
//
// Contraction must stay off wherever this is compiled (spk_assembly_core.hpp sets the pragma under clang).
#pragma once
#include "spk_assembly_core.hpp"

namespace spk {
namespace constraints {

// The slab: units [u0, u1) of the grid, a unit being a node line j (mz == 0: the 2-D grid, dof 2) or a node plane k (dof 3).
struct Slab {
    int mx, my, mz, u0, u1;
};
SPK_HD inline int dof(const Slab &g) { return g.mz ? 3 : 2; }
SPK_HD inline int rows(const Slab &g) { return 2 * dof(g); }                                   // m: 4 or 6
SPK_HD inline int units(const Slab &g) { return g.mz ? g.mz : g.my; }
SPK_HD inline int64_t unit_nodes(const Slab &g) { return g.mz ? (int64_t)g.mx * g.my : g.mx; }
SPK_HD inline int64_t unit_interior(const Slab &g) { return g.mz ? (int64_t)(g.mx - 2) * (g.my - 2) : g.mx - 2; }
SPK_HD inline int64_t local_cols(const Slab &g) { return dof(g) * unit_nodes(g) * (g.u1 - g.u0); }   // n_local of the slab
SPK_HD inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// interior units among [a, b)
SPK_HD inline int interior_units(const Slab &g, int a, int b)
{
    const int lo = assembly::imax(a, 1), hi = assembly::imin(b, units(g) - 1);
    return hi > lo ? hi - lo : 0;
}
// ---- counts ----------------------------------------------------------------------------------------------------------
// interior nodes of the slab = entries of every row of B; all its entries
SPK_HD inline int64_t row_count(const Slab &g) { return interior_units(g, g.u0, g.u1) * unit_interior(g); }
SPK_HD inline int64_t nnz(const Slab &g) { return rows(g) * row_count(g); }
// interior nodes of one interior unit in front of its node n (n in [0, unit_nodes])
SPK_HD inline int64_t unit_interior_before(const Slab &g, int64_t n)
{
    if (!g.mz) return clampi((int)n - 1, 0, g.mx - 2);
    const int j = (int)(n / g.mx), i = (int)(n - (int64_t)j * g.mx);
    return (int64_t)clampi(j - 1, 0, g.my - 2) * (g.mx - 2) + ((j >= 1 && j <= g.my - 2) ? clampi(i - 1, 0, g.mx - 2) : 0);
}
// interior nodes of the slab in front of its local node N (N in [0, nodes of the slab])
SPK_HD inline int64_t interior_before(const Slab &g, int64_t N)
{
    const int64_t un = unit_nodes(g);
    const int u = (int)(N / un);
    const int64_t n = N - u * un;
    const int gu = g.u0 + u;
    int64_t q = interior_units(g, g.u0, gu) * unit_interior(g);
    if (gu >= 1 && gu <= units(g) - 2) q += unit_interior_before(g, n);
    return q;
}

// ---- nodes -----------------------------------------------------------------------------------------------------------
struct Node {
    int i, j, k;         // grid position (k = 0 in 2-D)
    int64_t local;       // node number inside the slab
};
// the q-th interior node of the slab, ascending
SPK_HD inline Node interior_node(const Slab &g, int64_t q)
{
    const int64_t ui = unit_interior(g);
    const int u = (int)(q / ui) + assembly::imax(g.u0, 1);
    const int64_t r = q - (q / ui) * ui;
    Node nd;
    if (!g.mz) {
        nd.i = (int)r + 1, nd.j = u, nd.k = 0;
        nd.local = (int64_t)(u - g.u0) * g.mx + nd.i;
    } else {
        const int jj = (int)(r / (g.mx - 2));
        nd.i = (int)(r - (int64_t)jj * (g.mx - 2)) + 1, nd.j = jj + 1, nd.k = u;
        nd.local = ((int64_t)(u - g.u0) * g.my + nd.j) * g.mx + nd.i;
    }
    return nd;
}
// local node N of the slab: its position, and whether it is an interior node of the grid
SPK_HD inline Node local_node(const Slab &g, int64_t N, bool &interior)
{
    Node nd;
    nd.local = N;
    if (!g.mz) {
        nd.j = g.u0 + (int)(N / g.mx), nd.i = (int)(N - (int64_t)(nd.j - g.u0) * g.mx), nd.k = 0;
        interior = !assembly::on_boundary(g.mx, g.my, nd.i, nd.j);
    } else {
        const int64_t line = N / g.mx;
        nd.i = (int)(N - line * g.mx);
        nd.k = g.u0 + (int)(line / g.my), nd.j = (int)(line - (int64_t)(nd.k - g.u0) * g.my);
        interior = !assembly::on_boundary(g.mx, g.my, g.mz, nd.i, nd.j, nd.k);
    }
    return nd;
}

// ---- values: the host generator's expressions, in its order -----------------------------------------------------------
SPK_HD inline double weight(const Slab &g)
{
    if (!g.mz) {
        const double hx = 1.0 / (double)(g.mx - 1), hy = 1.0 / (double)(g.my - 1), w = hx * hy;
        return w;
    }
    const double w = (1.0 / (g.mx - 1)) * (1.0 / (g.my - 1)) * (1.0 / (g.mz - 1));
    return w;
}
// the entry of row r at the node (the node carries one for the component r % dof)
SPK_HD inline double value(const Slab &g, double w, int r, const Node &nd)
{
    const int d = dof(g);
    if (r < d) return w;
    const int axis = r - d;
    return w * ((axis == 0 ? assembly::coord(nd.i, g.mx) : axis == 1 ? assembly::coord(nd.j, g.my) : assembly::coord(nd.k, g.mz)) - 0.5);
}

// ---- B by rows: entry q of row r sits at r * row_count + q, on the q-th interior node --------------------------------
SPK_HD inline int64_t b_position(const Slab &g, int r, int64_t q) { return r * row_count(g) + q; }
SPK_HD inline int32_t b_column(const Slab &g, int r, const Node &nd) { return (int32_t)(nd.local * dof(g) + r % dof(g)); }

// ---- B^T by rows: local row lr = (node, c) holds 0 or 2 entries, (c, w) then (c + dof, moment) ------------------------
SPK_HD inline int64_t bt_rowptr(const Slab &g, int64_t lr)
{
    const int d = dof(g);
    const int64_t N = lr / d;
    const int c = (int)(lr - N * d);
    if (N >= unit_nodes(g) * (g.u1 - g.u0)) return 2 * d * row_count(g);   // the end pointer
    bool in;
    local_node(g, N, in);
    return 2 * (d * interior_before(g, N) + (in ? c : 0));
}

// ---- window pointers: winptr[w * m + r] = start of row r + its entries with a column below min(w * win, n_local) -------
SPK_HD inline int32_t window_pointer(const Slab &g, int r, int w, int32_t win)
{
    const int d = dof(g), c = r % d;
    const int64_t nl = local_cols(g);
    int64_t bound = (int64_t)w * win;
    if (bound > nl) bound = nl;
    // columns N d + c < bound  <=>  N < ceil((bound - c) / d)
    const int64_t N = bound > c ? (bound - c + d - 1) / d : 0;
    return (int32_t)(r * row_count(g) + interior_before(g, N));
}

}  // namespace constraints
}  // namespace spk
