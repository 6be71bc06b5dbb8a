// spk_stencil_op_core.hpp -- the one source of a row of a grid-stencil level operator (-spk_mg_operator stencil): the
// product and the fused smoothing step of a level whose pattern is the closed form of spk_galerkin_core.hpp, from the
// level's value array alone -- no row pointer, no column index.  The kernels (spk_k_amg.hip: amg_stencil_kernel, the fused
// tail) and the CPU run (tests/host/stencil_op_check.cpp) all call so_row, so they compute the same bits because they
// execute the same expressions; where the row's values lie (LDS in the launch, global memory in the tail, the heap on the
// host) changes nothing.  Standard library only; no ROCm.
//
// The rule, for the row of node (i, j, k), component a, on a level of nd[0] x nd[1] x nd[2] nodes of BS unknowns:
//   d = sum over the clipped neighbour nodes (i2, j2, k2) ascending -- z outermost, x innermost -- and b < BS innermost of
//       v[p] x[((k2 ny + j2) nx + i2) BS + b],  p = 0, 1, ... counting in that order (the stored order of the row);
//   the sum starts with the first product, every product is rounded on its own and then added (contraction off).
//   MODE 0: d.   MODE 1: y + alpha (dinv (b - d)) [+ beta (y - yo) when beta != 0; yo null: y - 0], y = x of the row itself:
//   amg_csr_kernel<1>'s expressions in its order.
// These are not the CSR route's bits (eight strided partial sums and a butterfly); they are held to this statement.
// The scalar type T of the values and the vectors is double, or float under SPK_AMG_PRECISION_SINGLE: the same expressions in
// the same order, every operation rounded to T.
#pragma once
#include "spk_galerkin_core.hpp"

// the loops of so_row have constant trip counts; unrolled, its two small arrays are registers
#ifdef __clang__
#define SPK_SO_UNROLL _Pragma("unroll")
#else
#define SPK_SO_UNROLL
#endif

namespace spk {
namespace stencil_op {

// the node (i, j, k) and the component of row r
struct SoRow { int32_t i, j, k, a; };
template <int BS>
SPK_HD inline SoRow so_row_of(const int32_t nd[3], int32_t r)
{
    const int32_t node = r / BS, line = node / nd[0];
    SoRow w;
    w.a = r - node * BS;
    w.i = node - line * nd[0];
    w.k = line / nd[1];
    w.j = line - w.k * nd[1];
    return w;
}
// the position of the first value of row r; r == rows: the end of the last row
template <int BS>
SPK_HD inline int64_t so_row_begin(const int32_t nd[3], int32_t r)
{
    if ((int64_t)r >= (int64_t)nd[0] * nd[1] * nd[2] * BS) return galerkin::gs_nnz(nd, BS);
    const SoRow w = so_row_of<BS>(nd, r);
    return galerkin::gs_row_offset(nd, BS, w.i, w.j, w.k, w.a);
}
// the most values a row of the level holds
SPK_HD inline int32_t so_max_row(const int32_t nd[3], int bs)
{
    const int32_t wx = nd[0] < 3 ? nd[0] : 3, wy = nd[1] < 3 ? nd[1] : 3, wz = nd[2] < 3 ? nd[2] : 3;
    return wx * wy * wz * bs;
}

// The rows of one workgroup of the launch (amg_stencil_kernel: one row per thread, the workgroup's values in LDS): whole
// waves of 64 whose longest rows fill at most 32 KiB, at most 256 rows.  elem: sizeof of the scalar type -- the byte budget
// is the same for float, so its workgroups take up to twice the rows.
// 2-D: 256, 192, 128 rows for bs 1, 2, 3 in double, 256 each in float; 3-D: 128, 64, 64 (bs 3: 41 KiB) and 256, 128, 64
SPK_HD inline int32_t so_wg_rows(const int32_t nd[3], int bs, int32_t elem)
{
    const int32_t per = 32768 / (so_max_row(nd, bs) * elem), whole = per / 64 * 64;
    return whole < 64 ? 64 : whole > 256 ? 256 : whole;
}

// one row: v points at the row's first value; x is the level's vector (MODE 1: the iterate y).  Returns out[row].
// G: the grid lines whose loads are issued together, 3 (a plane) or 1 -- registers against loads in flight; it changes
// no bit (the additions keep their order).  T is deduced from v and x; the other operands are of it (a null pointer or a
// double constant may stand there)
template <typename T> struct SoSame { using type = T; };
template <int BS, int MODE, int G = (BS <= 2 ? 3 : 1), typename T>
SPK_HD inline T so_row(const int32_t nd[3], const SoRow &w, const T *v, const T *x, const typename SoSame<T>::type *dinv,
                       const typename SoSame<T>::type *b, const typename SoSame<T>::type *yo, typename SoSame<T>::type alpha,
                       typename SoSame<T>::type beta)
{
    SPK_GS_EXACT
    const int32_t i0 = galerkin::gs_first(w.i), j0 = galerkin::gs_first(w.j), k0 = galerkin::gs_first(w.k);
    const int32_t ni = galerkin::gs_width(w.i, nd[0]), wi = ni * BS, wj = galerkin::gs_width(w.j, nd[1]), wk = galerkin::gs_width(w.k, nd[2]);
    // A group of G grid lines at a time -- by default a whole plane of neighbours for BS <= 2, one line for BS 3 -- with
    // constant trip counts: the group's values and x first (an absent neighbour reads the last present one of its line
    // again, so every address is the row's own), then the additions of the present ones in stored order -- on the device
    // the loads of a group are in flight together.  The neighbours of one grid line lie side by side in x: i2 ascending,
    // b innermost, wi values
    static_assert(G == 1 || G == 3, "lines per group");
    constexpr int W = 3 * BS;
    T d = T(0);
    const T *vp = v;
    SPK_SO_UNROLL
    for (int kk = 0; kk < 3; ++kk) {
        if (kk >= wk) break;
        SPK_SO_UNROLL
        for (int jg = 0; jg < 3; jg += G) {
            if (jg >= wj) break;
            T vv[G][W], xv[G][W];
            SPK_SO_UNROLL
            for (int u = 0; u < G; ++u) {
                const int32_t jc = jg + u < wj ? jg + u : wj - 1;
                const T *xr = x + ((int64_t)((k0 + kk) * nd[1] + (j0 + jc)) * nd[0] + i0) * BS;
                const T *vr = vp + jc * wi;
                SPK_SO_UNROLL
                for (int n = 0; n < 3; ++n) {   // the line's neighbour nodes: one address each, b at constant offsets
                    const int32_t nc = (n < ni ? n : ni - 1) * BS;
                    SPK_SO_UNROLL
                    for (int c = 0; c < BS; ++c) {
                        vv[u][n * BS + c] = vr[nc + c];
                        xv[u][n * BS + c] = xr[nc + c];
                    }
                }
            }
            SPK_SO_UNROLL
            for (int u = 0; u < G; ++u)
                SPK_SO_UNROLL
                for (int t = 0; t < W; ++t) {
                    if (jg + u >= wj || t >= wi) continue;
                    const T term = vv[u][t] * xv[u][t];
                    d = (kk == 0 && jg + u == 0 && t == 0) ? term : d + term;
                }
        }
        vp += wj * wi;
    }
    if (MODE == 0) return d;
    const int64_t row = ((int64_t)(w.k * nd[1] + w.j) * nd[0] + w.i) * BS + w.a;
    const T y = x[row];
    T r = y + alpha * (dinv[row] * (b[row] - d));
    if (beta != T(0)) r += beta * (y - (yo ? yo[row] : T(0)));   // yo null: the zero initial guess
    return r;
}

}  // namespace stencil_op
}  // namespace spk
