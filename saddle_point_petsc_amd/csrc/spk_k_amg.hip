// spk_k_amg.hip -- the V-cycle of the smoothed-aggregation multigrid (-pc_type gamg; host side in spk_amg_cycle.cpp).
// gfx950, wave64, FP64.  The levels >= 1 are CSR (sorted columns): eight lanes per row, each lane a fixed stride of
// the row, the eight partial sums added in a fixed butterfly -- no atomics, the same bits on every run.  Every launch
// takes the solver's `done` gate.  A level coarsened by the grid rule (-pc_type mg) applies P and R without reading
// them: amg_prolong_grid_kernel / amg_restrict_grid_kernel below.  The per-row work of every kernel of a coarse level is a
// __device__ function of the row index, shared with amg_tail_kernel, which runs the coarse levels' steps as one workgroup
// in one launch (-spk_mg_tail fused) and gives the launches' bits.  A level whose pattern is the grid stencil's closed form
// applies A from its value array alone where the options ask for it (-spk_mg_operator stencil): amg_stencil_kernel.
#include "spk_dict.hpp"
#include "spk_stencil_op_core.hpp"

namespace spk {
namespace k {

namespace {
constexpr int kAmgLanes = 8;                     // lanes per CSR row
constexpr int kAmgRows = kThreads / kAmgLanes;   // rows per workgroup

// sum over the row's entries of v * (x (- sub)) in the lane's slice, then over the eight lanes
__device__ __forceinline__ double row_dot(const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                          const double *__restrict__ v, const double *x, const double *sub, int32_t i,
                                          int lane)
{
    double acc = 0.0;
    const int32_t k1 = rp[i + 1];
    if (sub)
        for (int32_t k = rp[i] + lane; k < k1; k += kAmgLanes) { const int32_t c = ci[k]; acc += v[k] * (x[c] - sub[c]); }
    else
        for (int32_t k = rp[i] + lane; k < k1; k += kAmgLanes) acc += v[k] * x[ci[k]];
    acc += __shfl_xor(acc, 4);
    acc += __shfl_xor(acc, 2);
    acc += __shfl_xor(acc, 1);
    return acc;
}

// one CSR row in its eight lanes (all eight call it together), MODE as amg_csr_kernel states them; lane 0 writes
template <int MODE>
__device__ __forceinline__ void csr_row(const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                        const double *__restrict__ v, const double *x, const double *sub, const double *dinv,
                                        const double *b, const double *yo, double *out, double alpha, double beta, int32_t i,
                                        int lane)
{
    const double d = row_dot(rp, ci, v, x, MODE == 2 ? sub : nullptr, i, lane);
    if (lane != 0) return;
    if (MODE == 0 || MODE == 2) out[i] = d;
    else if (MODE == 3) out[i] += d;
    else {
        const double y = x[i];
        double r = y + alpha * (dinv[i] * (b[i] - d));
        if (beta != 0.0) r += beta * (y - (yo ? yo[i] : 0.0));   // yo null: the zero initial guess
        out[i] = r;
    }
}

// row i of y = C b, C dense row-major n x n: the lanes of one wave, lane-strided sums, fixed butterfly; lane 0 writes
__device__ __forceinline__ void dense_row(const double *__restrict__ C, int32_t n, const double *b, double *y, int32_t i, int lane)
{
    double acc = 0.0;
    for (int32_t j = lane; j < n; j += kWave) acc += C[(size_t)i * n + j] * b[j];
    for (int off = kWave / 2; off > 0; off /= 2) acc += __shfl_xor(acc, off);
    if (lane == 0) y[i] = acc;
}
}  // namespace

// MODE 0: out = A x
// MODE 1: out = y + alpha dinv (b - A y) + beta (y - yo)     (one Chebyshev / Richardson step; out may be yo, yo may be
//         null: the zero initial guess)
// MODE 2: out = A (x - sub)                                   (restriction of the residual: A = R, x = b, sub = A y)
// MODE 3: out += A x                                          (prolongation + correction: A = P)
template <int MODE>
__global__ __launch_bounds__(kThreads) void amg_csr_kernel(const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                           const double *__restrict__ v, int32_t n, const double *x,
                                                           const double *sub, const double *dinv, const double *b,
                                                           const double *yo, double *out, double alpha, double beta,
                                                           const int32_t *__restrict__ done)
{
    if (done && *done) return;
    const int lane = threadIdx.x % kAmgLanes;
    const int32_t i = (int32_t)blockIdx.x * kAmgRows + (int32_t)(threadIdx.x / kAmgLanes);
    if (i >= n) return;   // whole groups of eight leave together: the butterfly stays inside live lanes
    csr_row<MODE>(rp, ci, v, x, sub, dinv, b, yo, out, alpha, beta, i, lane);
}

// ---- a level >= 1 with the grid stencil's closed-form pattern, from its value array alone (SPK_AMG_OPERATOR_STENCIL) ----
// MODE 0: out = A x;  MODE 1: out = y + alpha dinv (b - A y) + beta (y - yo) (amg_csr_kernel<1>'s formula; out may be yo,
// never y).  One row per thread, `rows` = blockDim.x consecutive rows per workgroup: their values are one contiguous range
// of `v` (so_row_begin of the first row to that of the row behind the last), streamed into LDS by consecutive lanes in
// 16-byte pieces; then every thread runs so_row (spk_stencil_op_core.hpp) on its own row from there -- the gather of x is
// contiguous across lanes, neighbouring rows being neighbouring nodes of a grid line.  The range begins at a multiple of
// BS, not of two: it is staged from the even position at or below its begin, so that 16-byte pieces of global memory
// are 16-byte pieces of LDS, with the odd first and last values peeled.  No row pointer or column index is read.
// Byte model: 8 B per stored entry + x (gathered, cached) + out; MODE 1: + dinv, b, yo.
template <int BS, int MODE>
__global__ __launch_bounds__(kThreads) void amg_stencil_kernel(StencilOpArgs g, const double *__restrict__ v, const double *x,
                                                               const double *__restrict__ dinv, const double *__restrict__ b,
                                                               const double *yo, double *out, double alpha, double beta,
                                                               const int32_t *__restrict__ done)
{
    if (done && *done) return;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *sv = reinterpret_cast<double *>(smem);
    const int32_t nd[3] = {g.nx, g.ny, g.nz};
    const int32_t rows = (int32_t)blockDim.x, r0 = (int32_t)blockIdx.x * rows, r1 = min(r0 + rows, g.n);
    if (r0 >= g.n) return;   // (workgroup-uniform)
    const int64_t p0 = stencil_op::so_row_begin<BS>(nd, r0), p1 = stencil_op::so_row_begin<BS>(nd, r1);
    const int64_t base = p0 & ~(int64_t)1;   // sv[e] = v[base + e]
    const int64_t q0 = (p0 + 1) >> 1, q1 = p1 >> 1;   // the whole pairs [2 q0, 2 q1) of the range
    const double2 *v2 = reinterpret_cast<const double2 *>(v);
    double2 *s2 = reinterpret_cast<double2 *>(sv);
    for (int64_t q = q0 + threadIdx.x; q < q1; q += 4 * rows) {   // four pieces per thread in flight
        double2 t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) t[u] = v2[min(q + u * rows, q1 - 1)];   // (past the range: its last piece again, not stored)
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (q + u * rows < q1) s2[q + u * rows - (base >> 1)] = t[u];
    }
    if (threadIdx.x == 0 && (p0 & 1)) sv[p0 - base] = v[p0];
    if (threadIdx.x == 1 && (p1 & 1) && p1 - 1 >= 2 * q0) sv[p1 - 1 - base] = v[p1 - 1];
    __syncthreads();
    const int32_t r = r0 + (int32_t)threadIdx.x;
    if (r >= r1) return;
    const stencil_op::SoRow w = stencil_op::so_row_of<BS>(nd, r);
    const int64_t off = galerkin::gs_row_offset(nd, BS, w.i, w.j, w.k, w.a);
    out[r] = stencil_op::so_row<BS, MODE>(nd, w, sv + (off - base), x, dinv, b, yo, alpha, beta);
}

// the fine level's vector pass behind the layout's own product t = A y:
//   y == nullptr (zero initial guess): out = alpha dinv b;  else out = y + alpha dinv (b - t) + beta (y - yo)
__global__ __launch_bounds__(kThreads) void amg_cheb_vec_kernel(int64_t n, const double *__restrict__ dinv,
                                                                const double *__restrict__ b, const double *__restrict__ t,
                                                                const double *y, const double *yo, double *out, double alpha,
                                                                double beta, const int32_t *__restrict__ done)
{
    if (done && *done) return;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        if (!y) { out[i] = alpha * (dinv[i] * b[i]); continue; }
        const double yi = y[i];
        double r = yi + alpha * (dinv[i] * (b[i] - t[i]));
        if (beta != 0.0) r += beta * (yi - (yo ? yo[i] : 0.0));
        out[i] = r;
    }
}

// the fine level's fused step on the 2x2 row-type layout (row types + deviation codes, spk_k_dict.hip): the product of a
// block row and the three-term update in one pass, out = y + alpha dinv (b - A y) + beta (y - yo).  Modelled on
// jacobi_sweep_f32_dict_kernel, in FP64: the values decoded exactly, the products summed per row in block order as
// spmv_dict_kernel sums them.  One block row per thread, workgroups over XCD-contiguous chunks.  out may be yo (each
// entry is read by its own thread before it is written), never y (the neighbours' rows read it).
__global__ __launch_bounds__(kThreads) void amg_cheb_dict2_kernel(DictArgs d, const double *__restrict__ dinv,
                                                                  const double *__restrict__ b, const double *__restrict__ y,
                                                                  const double *yo, double *out, double alpha, double beta,
                                                                  const int32_t *__restrict__ done)
{
    if (done && *done) return;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int bx = (int)blockIdx.x;
    const int c0 = ((bx & 7) * d.chunks_per_xcd + (bx >> 3) * d.chunks_per_wg);
    const int c1 = min(min(c0 + d.chunks_per_wg, ((bx & 7) + 1) * d.chunks_per_xcd), d.nchunks);
    if (c0 >= c1) return;
    dict_load_lds(d, (d.nclass + 1) * 4, smem);
    const int32_t *tlen = reinterpret_cast<const int32_t *>(smem);
    const int2 *tent = reinterpret_cast<const int2 *>(smem + 4 * ((d.ntype + 1) & ~1));
    const double2 *cv = reinterpret_cast<const double2 *>(smem + d.cls_off);
    const int32_t *fl = reinterpret_cast<const int32_t *>(smem + d.fld_off);
    const double2 *y2 = reinterpret_cast<const double2 *>(y);
    for (int ch = c0; ch < c1; ++ch) {
        const int br = ch * kDictChunk + (int)threadIdx.x;
        if (br >= d.nbrows) continue;
        const int tc = (int)d.tid[br];
        double s0 = 0.0, s1 = 0.0;
        const int len = tlen[tc];
        const int2 *te = tent + (size_t)tc * d.kmax;
        constexpr int G = 10;   // a 2-D interior block row whole: five 16-byte code loads + nine gathers of y in flight
        for (int k0 = 0; k0 < len; k0 += G) {
#pragma clang fp contract(off)  // the sums of spmv_dict_kernel: every product rounded on its own (the update below is amg_cheb_vec's)
            int2 e[G];
            u64 w0[G];
            double2 yv[G];
#pragma unroll
            for (int h = 0; h < G / 2; ++h) {
                w0[2 * h] = w0[2 * h + 1] = 0ull;
                if (k0 + 2 * h < len) dict_issue_pair2(d, (k0 >> 1) + h, br, w0[2 * h], w0[2 * h + 1]);
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const bool in = k0 + g < len;
                e[g] = in ? te[k0 + g] : make_int2(0, 0);
                yv[g] = in ? y2[(int64_t)br + e[g].x] : make_double2(0.0, 0.0);
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (k0 + g < len) {
                    const double2 *cb = cv + (size_t)e[g].y * 4;
                    const int32_t *fb = fl + (size_t)e[g].y * 4;
                    const bool st = d.strad != 0;
                    s0 += dict_decode(dict_field2(w0[g], fb[0], st), cb[0]) * yv[g].x;
                    s0 += dict_decode(dict_field2(w0[g], fb[1], st), cb[1]) * yv[g].y;
                    s1 += dict_decode(dict_field2(w0[g], fb[2], st), cb[2]) * yv[g].x;
                    s1 += dict_decode(dict_field2(w0[g], fb[3], st), cb[3]) * yv[g].y;
                }
            }
        }
        const double2 yi = y2[br], bi = reinterpret_cast<const double2 *>(b)[br],
                      di = reinterpret_cast<const double2 *>(dinv)[br];
        double2 r;
        r.x = yi.x + alpha * (di.x * (bi.x - s0));
        r.y = yi.y + alpha * (di.y * (bi.y - s1));
        if (beta != 0.0 && yo) {
            const double2 oi = reinterpret_cast<const double2 *>(yo)[br];
            r.x += beta * (yi.x - oi.x);
            r.y += beta * (yi.y - oi.y);
        } else if (beta != 0.0) {
            r.x += beta * yi.x;
            r.y += beta * yi.y;
        }
        reinterpret_cast<double2 *>(out)[br] = r;
    }
}

// y = C b, C dense row-major n x n (the coarsest level's inverse): one wave per row, lane-strided sums, fixed butterfly
__global__ __launch_bounds__(kThreads) void amg_dense_kernel(const double *__restrict__ C, int32_t n,
                                                             const double *__restrict__ b, double *__restrict__ y,
                                                             const int32_t *__restrict__ done)
{
    if (done && *done) return;
    const int lane = threadIdx.x % kWave;
    const int32_t i = (int32_t)blockIdx.x * (kThreads / kWave) + (int32_t)(threadIdx.x / kWave);
    if (i >= n) return;
    dense_row(C, n, b, y, i, lane);
}

// mode 0: dst = src; mode 1: dst -= src
__global__ __launch_bounds__(kThreads) void amg_out_kernel(int mode, int64_t n, const double *__restrict__ src,
                                                           double *__restrict__ dst, const int32_t *__restrict__ done)
{
    if (done && *done) return;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads)
        dst[i] = mode ? dst[i] - src[i] : src[i];
}

// ---- the transfers of a grid-coarsened level, matrix-free (SPK_AMG_TRANSFER_MATRIX_FREE) -------------------------------
// P = P_z (x) P_y (x) P_x (x) I_bs is never read: a fine index that is even in a halved direction has the one parent
// i / 2 (weight 1), an odd one the parents (i - 1) / 2 and (i + 1) / 2 (weight 1/2 each); a direction that does not
// halve is the identity.  A halved side of an even number m of nodes (SPK_AMG_SIDES_ANY) keeps fine m - 1 as its last
// coarse node m / 2: that fine index has this one parent (weight 1), and that coarse index gathers it alone -- coarse
// m / 2 - 1 (fine m - 2) does not reach it.  Every weight is a power of two, so every product is exact and the order of
// the additions alone defines the bits: ascending column of P (prolongation) or of R (restriction), from the first
// product -- z outermost, x innermost.  The grid's x is one row of dofs of a node row, y and z the node row: no integer
// division but by BS.
// (GridArgs: spk_internal.hpp)
namespace {
// fine dof xd of node row (j, k) of a grid with fz fine nodes in z: y[f] += sum_parents w e[c]
template <int BS>
__device__ __forceinline__ void prolong_grid_dof(const GridArgs g, int32_t fz, const double *e, double *y, int32_t xd, int32_t j,
                                                 int32_t k)
{
    const int32_t i = xd / BS, c = xd - i * BS;
    // the last index of an even halved side: a coarse node itself
    const int32_t lx = g.ex && i == g.fx - 1, ly = g.ey && j == g.fy - 1, lz = g.ez && k == fz - 1;
    const bool ox = g.hx && (i & 1) && !lx, oy = g.hy && (j & 1) && !ly, oz = g.hz && (k & 1) && !lz;   // two parents in the direction
    const int32_t ic = g.hx ? (i + lx) >> 1 : i, jc = g.hy ? (j + ly) >> 1 : j, kc = g.hz ? (k + lz) >> 1 : k;   // the first parent
    const double w = (ox ? 0.5 : 1.0) * (oy ? 0.5 : 1.0) * (oz ? 0.5 : 1.0);
    const int64_t sx = BS, sy = (int64_t)g.cx * BS, sz = sy * g.cy;
    const double *p = e + ((int64_t)kc * g.cy + jc) * sy + (int64_t)ic * BS + c;
    // the (up to) eight parents, loaded before the first addition; absent ones read the first parent again and add nothing
    const double e000 = p[0], e001 = p[ox ? sx : 0], e010 = p[oy ? sy : 0], e011 = p[(oy ? sy : 0) + (ox ? sx : 0)];
    const int64_t oz_ = oz ? sz : 0;
    const double e100 = p[oz_], e101 = p[oz_ + (ox ? sx : 0)], e110 = p[oz_ + (oy ? sy : 0)],
                 e111 = p[oz_ + (oy ? sy : 0) + (ox ? sx : 0)];
    double s = w * e000;
    if (ox) s += w * e001;
    if (oy) { s += w * e010; if (ox) s += w * e011; }
    if (oz) {
        s += w * e100;
        if (ox) s += w * e101;
        if (oy) { s += w * e110; if (ox) s += w * e111; }
    }
    const int64_t f = (((int64_t)k * g.fy + j) * g.fx) * BS + xd;
    y[f] = y[f] + s;
}

// coarse dof xd of coarse node row (jc, kc): out[c] = sum_children w (b[f] - t[f]), a gather over the <= 3 fine indices of
// every halved direction (<= 27 terms), no atomics
template <int BS>
__device__ __forceinline__ void restrict_grid_dof(const GridArgs g, int32_t fz, const double *b, const double *t, double *out,
                                                  int32_t xd, int32_t jc, int32_t kc)
{
    const int32_t ic = xd / BS, c = xd - ic * BS;
    // the last coarse index of an even halved side: the last fine index alone
    const int32_t tx = g.ex && ic == g.cx - 1, ty = g.ey && jc == g.cy - 1, tz = g.ez && kc == g.cz - 1;
    // the fine indices [lo, hi] of a direction and its centre (weight 1; the others 1/2); on an even side the last fine
    // index belongs to the last coarse one only
    const int32_t mi = g.hx ? 2 * ic - tx : ic, mj = g.hy ? 2 * jc - ty : jc, mk = g.hz ? 2 * kc - tz : kc;
    const int32_t i0 = g.hx && !tx ? max(mi - 1, 0) : mi, i1 = g.hx && !tx ? min(mi + 1, g.fx - 1 - g.ex) : mi;
    const int32_t j0 = g.hy && !ty ? max(mj - 1, 0) : mj, j1 = g.hy && !ty ? min(mj + 1, g.fy - 1 - g.ey) : mj;
    const int32_t k0 = g.hz && !tz ? max(mk - 1, 0) : mk, k1 = g.hz && !tz ? min(mk + 1, fz - 1 - g.ez) : mk;
    double s = 0.0;
    bool first = true;
#pragma unroll
    for (int dk = 0; dk < 3; ++dk) {
        const int32_t k = k0 + dk;
        if (k > k1) break;
#pragma unroll
        for (int dj = 0; dj < 3; ++dj) {
            const int32_t j = j0 + dj;
            if (j > j1) break;
            const double wyz = (k == mk ? 1.0 : 0.5) * (j == mj ? 1.0 : 0.5);
            const int64_t row = (((int64_t)k * g.fy + j) * g.fx) * BS + c;
            double r[3];
#pragma unroll
            for (int di = 0; di < 3; ++di) {   // the row's loads first: they do not wait for the sum
                const int32_t i = min(i0 + di, i1);
                r[di] = b[row + (int64_t)i * BS] - t[row + (int64_t)i * BS];
            }
#pragma unroll
            for (int di = 0; di < 3; ++di) {
                const int32_t i = i0 + di;
                if (i > i1) break;
                const double term = (wyz * (i == mi ? 1.0 : 0.5)) * r[di];
                s = first ? term : s + term;
                first = false;
            }
        }
    }
    out[(((int64_t)kc * g.cy + jc) * g.cx) * BS + xd] = s;
}
}  // namespace

// y[f] += sum_parents w e[c]: one thread per fine dof (the launch's y, z: the fine node rows); byte model: y read + y
// written + e read
template <int BS>
__global__ __launch_bounds__(kThreads) void amg_prolong_grid_kernel(GridArgs g, const double *__restrict__ e, double *y,
                                                                    const int32_t *__restrict__ done)
{
    if (done && *done) return;
    const int32_t xd = (int32_t)blockIdx.x * kThreads + (int32_t)threadIdx.x;   // dof within the node row
    if (xd >= g.fx * BS) return;
    prolong_grid_dof<BS>(g, (int32_t)gridDim.z, e, y, xd, (int32_t)blockIdx.y, (int32_t)blockIdx.z);
}

// out[c] = sum_children w (b[f] - t[f]): one thread per coarse dof (the launch's y, z: the coarse node rows); byte model:
// b + t read + out written
template <int BS>
__global__ __launch_bounds__(kThreads) void amg_restrict_grid_kernel(GridArgs g, int32_t fz, const double *__restrict__ b,
                                                                     const double *__restrict__ t, double *__restrict__ out,
                                                                     const int32_t *__restrict__ done)
{
    if (done && *done) return;
    const int32_t xd = (int32_t)blockIdx.x * kThreads + (int32_t)threadIdx.x;   // dof within the coarse node row
    if (xd >= g.cx * BS) return;
    restrict_grid_dof<BS>(g, fz, b, t, out, xd, (int32_t)blockIdx.y, (int32_t)blockIdx.z);
}

// ---- the fused tail: the levels >= d->first as one workgroup in one launch ----------------------------------------
// Steps [s0, s1) of the cycle's list (one tail run), interpreted in order by 1024 threads; where the launches have a kernel
// boundary there is a workgroup barrier.  The per-row work is the functions above, called in loops: the bits are the
// launches'.  Every thread reaches every barrier: the trip counts and every choice of buffer depend on the descriptor and
// the step alone (workgroup-uniform); the row predicates depend on threadIdx.x / 8 (CSR rows) or / 64 (dense rows), so
// the lanes of a butterfly enter it together; nothing returns before the last step.  The vectors b, ya, yb are written here
// and read by other waves behind a barrier: one CU, workgroup scope, plain pointers.
namespace {
constexpr int kTailRows = kAmgTailThreads / kAmgLanes;   // CSR rows per sweep
constexpr int kTailWaves = kAmgTailThreads / kWave;      // dense rows per sweep

template <int MODE>
__device__ __forceinline__ void tail_csr(const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                         const double *__restrict__ v, int32_t n, const double *x, const double *sub,
                                         const double *dinv, const double *b, const double *yo, double *out, double alpha,
                                         double beta)
{
    const int lane = threadIdx.x % kAmgLanes;
    const int32_t r = (int32_t)(threadIdx.x / kAmgLanes);
    for (int32_t i0 = 0; i0 < n; i0 += kTailRows)
        if (i0 + r < n) csr_row<MODE>(rp, ci, v, x, sub, dinv, b, yo, out, alpha, beta, i0 + r, lane);
    __syncthreads();
}

// the same steps on a level applied from its value array alone (V.stencil): so_row over the level's rows, the values
// read from global memory; the bits are amg_stencil_kernel's
template <int BS, int MODE>
__device__ __forceinline__ void tail_stencil_bs(const AmgTailLevel &V, const double *x, const double *yo, double *out, double alpha,
                                                double beta)
{
    const int32_t nd[3] = {V.nd[0], V.nd[1], V.nd[2]};
    for (int32_t r = (int32_t)threadIdx.x; r < V.n; r += kAmgTailThreads) {
        const stencil_op::SoRow w = stencil_op::so_row_of<BS>(nd, r);
        const double *v = V.av + galerkin::gs_row_offset(nd, BS, w.i, w.j, w.k, w.a);
        out[r] = stencil_op::so_row<BS, MODE, 1>(nd, w, v, x, V.dinv, V.b, yo, alpha, beta);   // (one line at a time: 1024 threads leave 128 registers each)
    }
    __syncthreads();
}
template <int MODE>
__device__ __forceinline__ void tail_stencil(const AmgTailLevel &V, const double *x, const double *yo, double *out, double alpha,
                                             double beta)
{
    if (V.bs == 1) tail_stencil_bs<1, MODE>(V, x, yo, out, alpha, beta);
    else if (V.bs == 2) tail_stencil_bs<2, MODE>(V, x, yo, out, alpha, beta);
    else tail_stencil_bs<3, MODE>(V, x, yo, out, alpha, beta);
}

// nu smoothing steps on level V from y (null: the zero guess), as smooth() orders them; ends in sel ^ (nu & 1) (from null: in ya for odd nu)
template <bool STENCIL>
__device__ __forceinline__ void tail_smooth(const AmgTailLevel &V, double *y)
{
    const double *prev = nullptr;
    for (int32_t k = 0; k < V.nu; ++k) {
        double *dst = y == V.ya ? V.yb : V.ya;
        if (STENCIL && y && V.stencil) tail_stencil<1>(V, y, prev, dst, V.alpha[k], V.beta[k]);
        else if (y) tail_csr<1>(V.arp, V.aci, V.av, V.n, y, nullptr, V.dinv, V.b, prev, dst, V.alpha[k], V.beta[k]);
        else {   // amg_cheb_vec_kernel from the zero guess
            const double alpha = V.alpha[k];
            for (int32_t i = (int32_t)threadIdx.x; i < V.n; i += kAmgTailThreads) dst[i] = alpha * (V.dinv[i] * V.b[i]);
            __syncthreads();
        }
        prev = y;
        y = dst;
    }
}

template <int BS>
__device__ __forceinline__ void tail_restrict_grid(const AmgTailLevel &V, const double *t, double *out)
{
    const GridArgs g = V.g;
    const int32_t w = g.cx * BS, wy = w * g.cy, tot = wy * g.cz;   // (tot = the rows of the next level <= tail_rows)
    for (int32_t q = (int32_t)threadIdx.x; q < tot; q += kAmgTailThreads) {
        const int32_t kc = q / wy, r = q - kc * wy, jc = r / w;
        restrict_grid_dof<BS>(g, V.fz, V.b, t, out, r - jc * w, jc, kc);
    }
}
template <int BS>
__device__ __forceinline__ void tail_prolong_grid(const AmgTailLevel &V, const double *e, double *y)
{
    const GridArgs g = V.g;
    const int32_t w = g.fx * BS, wy = w * g.fy, tot = wy * V.fz;
    for (int32_t q = (int32_t)threadIdx.x; q < tot; q += kAmgTailThreads) {
        const int32_t k = q / wy, r = q - k * wy, j = r / w;
        prolong_grid_dof<BS>(g, V.fz, e, y, r - j * w, j, k);
    }
}
}  // namespace

// STENCIL: a level of the tail may apply A from its value array alone (AmgTailLevel.stencil): amg_stencil_tail_kernel;
// without, the body is amg_tail_kernel as it was before that option existed
namespace {
template <bool STENCIL>
__device__ __forceinline__ void tail_run(const AmgTailDesc *__restrict__ d, int32_t s0, int32_t s1)
{
    for (int32_t s = s0; s < s1; ++s) {
        const AmgTailStep st = d->steps[s];
        const AmgTailLevel &V = d->lv[st.level];
        double *y = st.sel ? V.yb : V.ya, *o = st.sel ? V.ya : V.yb;   // the level's iterate and the other buffer
        switch (st.kind) {
        case SPK_AMG_STEP_PRE0: tail_smooth<STENCIL>(V, nullptr); break;
        case SPK_AMG_STEP_PRE:
        case SPK_AMG_STEP_POST: tail_smooth<STENCIL>(V, y); break;
        case SPK_AMG_STEP_DOWN: {   // o = A y, then b of the next level = R (b - o)
            double *bn = d->lv[st.level + 1].b;
            if (STENCIL && V.stencil) tail_stencil<0>(V, y, nullptr, o, 0.0, 0.0);
            else tail_csr<0>(V.arp, V.aci, V.av, V.n, y, nullptr, nullptr, nullptr, nullptr, o, 0.0, 0.0);
            if (V.matrix_free) {
                if (V.bs == 1) tail_restrict_grid<1>(V, o, bn);
                else if (V.bs == 2) tail_restrict_grid<2>(V, o, bn);
                else tail_restrict_grid<3>(V, o, bn);
                __syncthreads();
            } else {
                tail_csr<2>(V.rrp, V.rci, V.rv, V.nc, V.b, o, nullptr, nullptr, nullptr, bn, 0.0, 0.0);
            }
            break;
        }
        case SPK_AMG_STEP_COARSE: {   // always into ya
            const int lane = threadIdx.x % kWave;
            const int32_t r = (int32_t)(threadIdx.x / kWave);
            for (int32_t i0 = 0; i0 < V.n; i0 += kTailWaves)
                if (i0 + r < V.n) dense_row(d->cinv, V.n, V.b, V.ya, i0 + r, lane);
            __syncthreads();
            break;
        }
        default: {   // SPK_AMG_STEP_UP: y += P e, e the iterate of the next level
            const AmgTailLevel &N = d->lv[st.level + 1];
            const double *e = st.sel_next ? N.yb : N.ya;
            if (V.matrix_free) {
                if (V.bs == 1) tail_prolong_grid<1>(V, e, y);
                else if (V.bs == 2) tail_prolong_grid<2>(V, e, y);
                else tail_prolong_grid<3>(V, e, y);
                __syncthreads();
            } else {
                tail_csr<3>(V.prp, V.pci, V.pv, V.n, e, nullptr, nullptr, nullptr, nullptr, y, 0.0, 0.0);
            }
        }
        }
    }
}
}  // namespace

__global__ __launch_bounds__(kAmgTailThreads) void amg_tail_kernel(const AmgTailDesc *__restrict__ d, int32_t s0, int32_t s1,
                                                                   const int32_t *__restrict__ done)
{
    if (done && *done) return;   // written by launches before this one only: the whole workgroup reads one value
    tail_run<false>(d, s0, s1);
}
__global__ __launch_bounds__(kAmgTailThreads) void amg_stencil_tail_kernel(const AmgTailDesc *__restrict__ d, int32_t s0, int32_t s1,
                                                                           const int32_t *__restrict__ done)
{
    if (done && *done) return;
    tail_run<true>(d, s0, s1);
}

namespace {
// x: the dofs of one node row in workgroups; y, z: the node rows (amg_check_opts keeps both within 65535)
inline dim3 transfer_grid(const int32_t d[3], int bs) { return dim3((unsigned)(((int64_t)d[0] * bs + kThreads - 1) / kThreads), (unsigned)d[1], (unsigned)d[2]); }
}  // namespace

void amg_prolong_add_grid(const AmgGrid &a, const double *e, double *y, const int32_t *done, hipStream_t s)
{
    const GridArgs g = grid_args(a);
    const dim3 grid = transfer_grid(a.fd, a.bs);
    if (a.bs == 1) hipLaunchKernelGGL(amg_prolong_grid_kernel<1>, grid, dim3(kThreads), 0, s, g, e, y, done);
    else if (a.bs == 2) hipLaunchKernelGGL(amg_prolong_grid_kernel<2>, grid, dim3(kThreads), 0, s, g, e, y, done);
    else hipLaunchKernelGGL(amg_prolong_grid_kernel<3>, grid, dim3(kThreads), 0, s, g, e, y, done);
}
void amg_restrict_grid(const AmgGrid &a, const double *b, const double *t, double *out, const int32_t *done, hipStream_t s)
{
    const GridArgs g = grid_args(a);
    const dim3 grid = transfer_grid(a.cd, a.bs);
    if (a.bs == 1) hipLaunchKernelGGL(amg_restrict_grid_kernel<1>, grid, dim3(kThreads), 0, s, g, a.fd[2], b, t, out, done);
    else if (a.bs == 2) hipLaunchKernelGGL(amg_restrict_grid_kernel<2>, grid, dim3(kThreads), 0, s, g, a.fd[2], b, t, out, done);
    else hipLaunchKernelGGL(amg_restrict_grid_kernel<3>, grid, dim3(kThreads), 0, s, g, a.fd[2], b, t, out, done);
}

namespace {
inline dim3 csr_grid(int32_t n) { return dim3((unsigned)std::max<int64_t>(((int64_t)n + kAmgRows - 1) / kAmgRows, 1)); }
inline dim3 vec_grid1(int64_t n) { return dim3((unsigned)std::max<int64_t>(std::min<int64_t>((n + kThreads - 1) / kThreads, kMaxBlocks * 4), 1)); }
}  // namespace

void amg_spmv(const CsrDev &A, const double *x, double *out, const int32_t *done, hipStream_t s)
{
    if (A.nrows == 0) return;
    hipLaunchKernelGGL(amg_csr_kernel<0>, csr_grid(A.nrows), dim3(kThreads), 0, s, A.rowptr.p, A.colidx.p, A.val.p, A.nrows,
                       x, (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, (const double *)nullptr,
                       out, 0.0, 0.0, done);
}
void amg_cheb_csr(const CsrDev &A, const double *dinv, const double *b, const double *y, const double *yo, double *out,
                  double alpha, double beta, const int32_t *done, hipStream_t s)
{
    if (A.nrows == 0) return;
    hipLaunchKernelGGL(amg_csr_kernel<1>, csr_grid(A.nrows), dim3(kThreads), 0, s, A.rowptr.p, A.colidx.p, A.val.p, A.nrows,
                       y, (const double *)nullptr, dinv, b, yo, out, alpha, beta, done);
}
// rows per workgroup of amg_stencil_kernel: whole waves whose longest rows fill at most 32 KiB of LDS (several
// workgroups per CU), at most kThreads.  2-D: 256 (bs 1), 192 (bs 2), 128 (bs 3); 3-D: 128, 64, 64 (bs 3: 41 KiB)
int stencil_op_rows(const int32_t nd[3], int bs)
{
    const int per = 32768 / (stencil_op::so_max_row(nd, bs) * (int)sizeof(double));
    return std::min(std::max(per / kWave * kWave, kWave), kThreads);
}
template <int BS>
static void stencil_op_launch(const StencilOpArgs &g, int rows, size_t lds, int mode, const double *v, const double *x,
                              const double *dinv, const double *b, const double *yo, double *out, double alpha, double beta,
                              const int32_t *done, hipStream_t s)
{
    const dim3 grid((unsigned)((g.n + rows - 1) / rows));
    if (mode == 0) hipLaunchKernelGGL((amg_stencil_kernel<BS, 0>), grid, dim3(rows), lds, s, g, v, x, dinv, b, yo, out, alpha, beta, done);
    else hipLaunchKernelGGL((amg_stencil_kernel<BS, 1>), grid, dim3(rows), lds, s, g, v, x, dinv, b, yo, out, alpha, beta, done);
}
void amg_stencil_op(const CsrDev &A, const int32_t nd[3], int bs, int mode, const double *x, const double *dinv, const double *b,
                    const double *yo, double *out, double alpha, double beta, const int32_t *done, hipStream_t s)
{
    if (A.nrows == 0) return;
    const StencilOpArgs g{nd[0], nd[1], nd[2], A.nrows};
    const int rows = stencil_op_rows(nd, bs);
    // the workgroup's range and the one value in front of an odd begin, rounded up to whole pairs
    const size_t lds = ((size_t)rows * (size_t)stencil_op::so_max_row(nd, bs) + 2) * sizeof(double);
    if (bs == 1) stencil_op_launch<1>(g, rows, lds, mode, A.val.p, x, dinv, b, yo, out, alpha, beta, done, s);
    else if (bs == 2) stencil_op_launch<2>(g, rows, lds, mode, A.val.p, x, dinv, b, yo, out, alpha, beta, done, s);
    else stencil_op_launch<3>(g, rows, lds, mode, A.val.p, x, dinv, b, yo, out, alpha, beta, done, s);
}
void amg_restrict(const CsrDev &R, const double *b, const double *t, double *out, const int32_t *done, hipStream_t s)
{
    if (R.nrows == 0) return;
    hipLaunchKernelGGL(amg_csr_kernel<2>, csr_grid(R.nrows), dim3(kThreads), 0, s, R.rowptr.p, R.colidx.p, R.val.p, R.nrows,
                       b, t, (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, out, 0.0, 0.0, done);
}
void amg_prolong_add(const CsrDev &P, const double *e, double *y, const int32_t *done, hipStream_t s)
{
    if (P.nrows == 0) return;
    hipLaunchKernelGGL(amg_csr_kernel<3>, csr_grid(P.nrows), dim3(kThreads), 0, s, P.rowptr.p, P.colidx.p, P.val.p, P.nrows,
                       e, (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, (const double *)nullptr,
                       y, 0.0, 0.0, done);
}
void amg_cheb_vec(int64_t n, const double *dinv, const double *b, const double *t, const double *y, const double *yo,
                  double *out, double alpha, double beta, const int32_t *done, hipStream_t s)
{
    if (n == 0) return;
    hipLaunchKernelGGL(amg_cheb_vec_kernel, vec_grid1(n), dim3(kThreads), 0, s, n, dinv, b, t, y, yo, out, alpha, beta, done);
}
bool amg_cheb_dict2(const DictDev &A, const double *dinv, const double *b, const double *y, const double *yo, double *out,
                    double alpha, double beta, const int32_t *done, hipStream_t s)
{
    if (!A.ok || A.bs != 2) return false;
    if (A.nbrows == 0) return true;
    int grid = 0;
    DictArgs d = dict_args(A, &grid);
    // one chunk per workgroup: the kernel does not pipeline its chunks (the 512 workgroups dict_args sizes for the
    // pipelined product left it latency-bound: 45.6 us at 1024^2 against 21.8 + 9.9 for the product and the vector pass)
    d.chunks_per_wg = 1;
    d.chunks_per_xcd = (d.nchunks + 7) / 8;
    grid = 8 * d.chunks_per_xcd;
    hipLaunchKernelGGL(amg_cheb_dict2_kernel, dim3(grid), dim3(kThreads), (size_t)A.lds_bytes, s, d, dinv, b, y, yo, out, alpha,
                       beta, done);
    return true;
}
void amg_dense(const double *C, int32_t n, const double *b, double *y, const int32_t *done, hipStream_t s)
{
    if (n == 0) return;
    const int rows = kThreads / kWave;
    hipLaunchKernelGGL(amg_dense_kernel, dim3((unsigned)((n + rows - 1) / rows)), dim3(kThreads), 0, s, C, n, b, y, done);
}
void amg_tail(const AmgTailDesc *d, bool stencil, int32_t s0, int32_t s1, const int32_t *done, hipStream_t s)
{
    if (s0 >= s1) return;
    if (stencil) hipLaunchKernelGGL(amg_stencil_tail_kernel, dim3(1), dim3(kAmgTailThreads), 0, s, d, s0, s1, done);
    else hipLaunchKernelGGL(amg_tail_kernel, dim3(1), dim3(kAmgTailThreads), 0, s, d, s0, s1, done);
}
void amg_out(int mode, int64_t n, const double *src, double *dst, const int32_t *done, hipStream_t s)
{
    if (n == 0) return;
    hipLaunchKernelGGL(amg_out_kernel, vec_grid1(n), dim3(kThreads), 0, s, mode, n, src, dst, done);
}

}  // namespace k
}  // namespace spk
