// spk_k_amg.hip -- the V-cycle of the smoothed-aggregation multigrid (-pc_type gamg; host side in spk_amg_cycle.cpp).
// gfx950, wave64, FP64.  The levels >= 1 are CSR (sorted columns): eight lanes per row, each lane a fixed stride of
// the row, the eight partial sums added in a fixed butterfly -- no atomics, the same bits on every run.  Every launch
// takes the solver's `done` gate.  A level coarsened by the grid rule (-pc_type mg) applies P and R without reading
// them: amg_prolong_grid_kernel / amg_restrict_grid_kernel below.  The per-row work of every kernel of a coarse level is a
// __device__ function of the row index, shared with amg_tail_kernel, which runs the coarse levels' steps as one workgroup
// in one launch (-spk_mg_tail fused) and gives the launches' bits.  A level whose pattern is the grid stencil's closed form
// applies A from its value array alone where the options ask for it (-spk_mg_operator stencil): amg_stencil_kernel.
// Under -spk_mg_precision single (SPK_AMG_PRECISION_SINGLE) the levels >= 1 of that route are FP32: the per-row functions
// are templates over the scalar type and the kernels have a float instantiation -- the same expressions in the same
// order, every product and every addition rounded on its own; the transfers between level 0 and level 1 compute in FP64
// and round (DOWN) or widen (UP) once.
#include <type_traits>

#include "spk_dict.hpp"
#include "spk_stencil_op_core.hpp"

namespace spk {
namespace k {

namespace {
constexpr int kAmgLanes = 8;                     // lanes per CSR row
constexpr int kAmgRows = kThreads / kAmgLanes;   // rows per workgroup

// the 16-byte piece of a value array
template <typename T> struct Piece;
template <> struct Piece<double> { using type = double2; static constexpr int shift = 1; };
template <> struct Piece<float> { using type = float4; static constexpr int shift = 2; };
// a product that an addition follows: in FP32 rounded on its own; in FP64 the expression the compiler has always seen
__device__ __forceinline__ double mul(double a, double b) { return a * b; }
__device__ __forceinline__ float mul(float a, float b)
{
    SPK_GS_EXACT
    return a * b;
}

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
template <typename T>
__device__ __forceinline__ void dense_row(const T *__restrict__ C, int32_t n, const T *b, T *y, int32_t i, int lane)
{
    T acc = T(0);
    for (int32_t j = lane; j < n; j += kWave) acc += mul(C[(size_t)i * n + j], b[j]);
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
// BS, not of the P = 2 doubles or 4 floats of a piece: it is staged from the multiple of P at or below its begin, so that
// 16-byte pieces of global memory are 16-byte pieces of LDS, with the up to P - 1 values in front of the first whole piece
// and behind the last one peeled.  No row pointer or column index is read.
// Byte model: sizeof(T) per stored entry + x (gathered, cached) + out; MODE 1: + dinv, b, yo.
// The body is one template over the scalar type; the FP64 kernel keeps its name, the FP32 one is amg_stencil_f32_kernel.
namespace {
template <int BS, int MODE, typename T>
__device__ __forceinline__ void stencil_rows(const StencilOpArgs &g, const T *__restrict__ v, const T *x, const T *__restrict__ dinv,
                                             const T *__restrict__ b, const T *yo, T *out, T alpha, T beta)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T *sv = reinterpret_cast<T *>(smem);
    using V = typename Piece<T>::type;
    constexpr int SH = Piece<T>::shift, P = 1 << SH;
    const int32_t nd[3] = {g.nx, g.ny, g.nz};
    const int32_t rows = (int32_t)blockDim.x, r0 = (int32_t)blockIdx.x * rows, r1 = min(r0 + rows, g.n);
    if (r0 >= g.n) return;   // (workgroup-uniform)
    const int64_t p0 = stencil_op::so_row_begin<BS>(nd, r0), p1 = stencil_op::so_row_begin<BS>(nd, r1);
    const int64_t base = p0 & ~(int64_t)(P - 1);   // sv[e] = v[base + e]
    const int64_t q0 = (p0 + P - 1) >> SH, q1 = p1 >> SH;   // the whole pieces [P q0, P q1) of the range
    const V *v2 = reinterpret_cast<const V *>(v);
    V *s2 = reinterpret_cast<V *>(sv);
    for (int64_t q = q0 + threadIdx.x; q < q1; q += 4 * rows) {   // four pieces per thread in flight
        V t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) t[u] = v2[min(q + u * rows, q1 - 1)];   // (past the range: its last piece again, not stored)
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (q + u * rows < q1) s2[q + u * rows - (base >> SH)] = t[u];
    }
    // [p0, h1): the values in front of the first whole piece; [t0, p1): those behind the last (a range without a whole
    // piece is all head); fewer than P each
    const int64_t h1 = min(q0 << SH, p1), t0 = max(q1 << SH, h1);
    if (threadIdx.x < P) {
        const int64_t a = p0 + threadIdx.x, z = t0 + threadIdx.x;
        if (a < h1) sv[a - base] = v[a];
        if (z < p1) sv[z - base] = v[z];
    }
    __syncthreads();
    const int32_t r = r0 + (int32_t)threadIdx.x;
    if (r >= r1) return;
    const stencil_op::SoRow w = stencil_op::so_row_of<BS>(nd, r);
    const int64_t off = galerkin::gs_row_offset(nd, BS, w.i, w.j, w.k, w.a);
    out[r] = stencil_op::so_row<BS, MODE>(nd, w, sv + (off - base), x, dinv, b, yo, alpha, beta);
}
}  // namespace
template <int BS, int MODE>
__global__ __launch_bounds__(kThreads) void amg_stencil_kernel(StencilOpArgs g, const double *__restrict__ v, const double *x,
                                                               const double *__restrict__ dinv, const double *__restrict__ b,
                                                               const double *yo, double *out, double alpha, double beta,
                                                               const int32_t *__restrict__ done)
{
    if (done && *done) return;
    stencil_rows<BS, MODE, double>(g, v, x, dinv, b, yo, out, alpha, beta);
}
template <int BS, int MODE>
__global__ __launch_bounds__(kThreads) void amg_stencil_f32_kernel(StencilOpArgs g, const float *__restrict__ v, const float *x,
                                                                   const float *__restrict__ dinv, const float *__restrict__ b,
                                                                   const float *yo, float *out, float alpha, float beta,
                                                                   const int32_t *__restrict__ done)
{
    if (done && *done) return;
    stencil_rows<BS, MODE, float>(g, v, x, dinv, b, yo, out, alpha, beta);
}

// the fine level's vector pass behind the layout's own product t = A y:
//   y == nullptr (zero initial guess): out = alpha dinv b;  else out = y + alpha dinv (b - t) + beta (y - yo)
// (float: the zero initial guess of an FP32 level alone)
template <typename T>
__global__ __launch_bounds__(kThreads) void amg_cheb_vec_kernel(int64_t n, const T *__restrict__ dinv,
                                                                const T *__restrict__ b, const T *__restrict__ t,
                                                                const T *y, const T *yo, T *out, T alpha,
                                                                T beta, const int32_t *__restrict__ done)
{
    if (done && *done) return;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        if (!y) { out[i] = alpha * (dinv[i] * b[i]); continue; }
        const T yi = y[i];
        T r = yi + alpha * (dinv[i] * (b[i] - t[i]));
        if (beta != T(0)) r += beta * (yi - (yo ? yo[i] : T(0)));
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
template <typename T>
__global__ __launch_bounds__(kThreads) void amg_dense_kernel(const T *__restrict__ C, int32_t n,
                                                             const T *__restrict__ b, T *__restrict__ y,
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
// The functions are templates over (input type TI, output type TO): double -> double, float -> float between FP32 levels,
// and the two forms of the level 0 / level 1 boundary under SPK_AMG_PRECISION_SINGLE.  The prolongation adds in TO (float ->
// double: every e widened, which is exact, then the FP64 sums); the restriction adds in TI (double -> float: the FP64 sums,
// rounded once on the store).
// (GridArgs: spk_internal.hpp)
namespace {
// fine dof xd of node row (j, k) of a grid with fz fine nodes in z: y[f] += sum_parents w e[c]
template <int BS, typename TI, typename TO>
__device__ __forceinline__ void prolong_grid_dof(const GridArgs g, int32_t fz, const TI *e, TO *y, int32_t xd, int32_t j,
                                                 int32_t k)
{
    const int32_t i = xd / BS, c = xd - i * BS;
    // the last index of an even halved side: a coarse node itself
    const int32_t lx = g.ex && i == g.fx - 1, ly = g.ey && j == g.fy - 1, lz = g.ez && k == fz - 1;
    const bool ox = g.hx && (i & 1) && !lx, oy = g.hy && (j & 1) && !ly, oz = g.hz && (k & 1) && !lz;   // two parents in the direction
    const int32_t ic = g.hx ? (i + lx) >> 1 : i, jc = g.hy ? (j + ly) >> 1 : j, kc = g.hz ? (k + lz) >> 1 : k;   // the first parent
    const TO w = (TO)((ox ? 0.5 : 1.0) * (oy ? 0.5 : 1.0) * (oz ? 0.5 : 1.0));
    const int64_t sx = BS, sy = (int64_t)g.cx * BS, sz = sy * g.cy;
    const TI *p = e + ((int64_t)kc * g.cy + jc) * sy + (int64_t)ic * BS + c;
    // the (up to) eight parents, loaded before the first addition; absent ones read the first parent again and add nothing
    const TO e000 = p[0], e001 = p[ox ? sx : 0], e010 = p[oy ? sy : 0], e011 = p[(oy ? sy : 0) + (ox ? sx : 0)];
    const int64_t oz_ = oz ? sz : 0;
    const TO e100 = p[oz_], e101 = p[oz_ + (ox ? sx : 0)], e110 = p[oz_ + (oy ? sy : 0)],
                 e111 = p[oz_ + (oy ? sy : 0) + (ox ? sx : 0)];
    TO s = w * e000;
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
template <int BS, typename TI, typename TO>
__device__ __forceinline__ void restrict_grid_dof(const GridArgs g, int32_t fz, const TI *b, const TI *t, TO *out,
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
    TI s = TI(0);
    bool first = true;
#pragma unroll
    for (int dk = 0; dk < 3; ++dk) {
        const int32_t k = k0 + dk;
        if (k > k1) break;
#pragma unroll
        for (int dj = 0; dj < 3; ++dj) {
            const int32_t j = j0 + dj;
            if (j > j1) break;
            const TI wyz = (TI)((k == mk ? 1.0 : 0.5) * (j == mj ? 1.0 : 0.5));
            const int64_t row = (((int64_t)k * g.fy + j) * g.fx) * BS + c;
            TI r[3];
#pragma unroll
            for (int di = 0; di < 3; ++di) {   // the row's loads first: they do not wait for the sum
                const int32_t i = min(i0 + di, i1);
                r[di] = b[row + (int64_t)i * BS] - t[row + (int64_t)i * BS];
            }
#pragma unroll
            for (int di = 0; di < 3; ++di) {
                const int32_t i = i0 + di;
                if (i > i1) break;
                const TI term = (wyz * (i == mi ? TI(1) : TI(0.5))) * r[di];
                s = first ? term : s + term;
                first = false;
            }
        }
    }
    out[(((int64_t)kc * g.cy + jc) * g.cx) * BS + xd] = (TO)s;
}
}  // namespace

// y[f] += sum_parents w e[c]: one thread per fine dof (the launch's y, z: the fine node rows); byte model: y read + y
// written + e read
template <int BS, typename TI, typename TO>
__global__ __launch_bounds__(kThreads) void amg_prolong_grid_kernel(GridArgs g, const TI *__restrict__ e, TO *y,
                                                                    const int32_t *__restrict__ done)
{
    if (done && *done) return;
    const int32_t xd = (int32_t)blockIdx.x * kThreads + (int32_t)threadIdx.x;   // dof within the node row
    if (xd >= g.fx * BS) return;
    prolong_grid_dof<BS, TI, TO>(g, (int32_t)gridDim.z, e, y, xd, (int32_t)blockIdx.y, (int32_t)blockIdx.z);
}

// out[c] = sum_children w (b[f] - t[f]): one thread per coarse dof (the launch's y, z: the coarse node rows); byte model:
// b + t read + out written
template <int BS, typename TI, typename TO>
__global__ __launch_bounds__(kThreads) void amg_restrict_grid_kernel(GridArgs g, int32_t fz, const TI *__restrict__ b,
                                                                     const TI *__restrict__ t, TO *__restrict__ out,
                                                                     const int32_t *__restrict__ done)
{
    if (done && *done) return;
    const int32_t xd = (int32_t)blockIdx.x * kThreads + (int32_t)threadIdx.x;   // dof within the coarse node row
    if (xd >= g.cx * BS) return;
    restrict_grid_dof<BS, TI, TO>(g, fz, b, t, out, xd, (int32_t)blockIdx.y, (int32_t)blockIdx.z);
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
template <int BS, int MODE, typename T>
__device__ __forceinline__ void tail_stencil_bs(const AmgTailLevelT<T> &V, const T *x, const T *yo, T *out, T alpha, T beta)
{
    const int32_t nd[3] = {V.nd[0], V.nd[1], V.nd[2]};
    for (int32_t r = (int32_t)threadIdx.x; r < V.n; r += kAmgTailThreads) {
        const stencil_op::SoRow w = stencil_op::so_row_of<BS>(nd, r);
        const T *v = V.av + galerkin::gs_row_offset(nd, BS, w.i, w.j, w.k, w.a);
        out[r] = stencil_op::so_row<BS, MODE, 1>(nd, w, v, x, V.dinv, V.b, yo, alpha, beta);   // (one line at a time: 1024 threads leave 128 registers each)
    }
    __syncthreads();
}
template <int MODE, typename T>
__device__ __forceinline__ void tail_stencil(const AmgTailLevelT<T> &V, const T *x, const T *yo, T *out, T alpha, T beta)
{
    if (V.bs == 1) tail_stencil_bs<1, MODE>(V, x, yo, out, alpha, beta);
    else if (V.bs == 2) tail_stencil_bs<2, MODE>(V, x, yo, out, alpha, beta);
    else tail_stencil_bs<3, MODE>(V, x, yo, out, alpha, beta);
}

// nu smoothing steps on level V from y (null: the zero guess), as smooth() orders them; ends in sel ^ (nu & 1) (from null: in ya for odd nu)
// (a float tail has no CSR level: where the launches would take a CSR kernel it does nothing -- the host never plans that)
template <bool STENCIL, typename T>
__device__ __forceinline__ void tail_smooth(const AmgTailLevelT<T> &V, T *y)
{
    const T *prev = nullptr;
    for (int32_t k = 0; k < V.nu; ++k) {
        T *dst = y == V.ya ? V.yb : V.ya;
        if (STENCIL && y && V.stencil) tail_stencil<1>(V, y, prev, dst, V.alpha[k], V.beta[k]);
        else if (y) {
            if constexpr (std::is_same<T, double>::value)
                tail_csr<1>(V.arp, V.aci, V.av, V.n, y, nullptr, V.dinv, V.b, prev, dst, V.alpha[k], V.beta[k]);
        } else {   // amg_cheb_vec_kernel from the zero guess
            const T alpha = V.alpha[k];
            for (int32_t i = (int32_t)threadIdx.x; i < V.n; i += kAmgTailThreads) dst[i] = alpha * (V.dinv[i] * V.b[i]);
            __syncthreads();
        }
        prev = y;
        y = dst;
    }
}

template <int BS, typename T>
__device__ __forceinline__ void tail_restrict_grid(const AmgTailLevelT<T> &V, const T *t, T *out)
{
    const GridArgs g = V.g;
    const int32_t w = g.cx * BS, wy = w * g.cy, tot = wy * g.cz;   // (tot = the rows of the next level <= tail_rows)
    for (int32_t q = (int32_t)threadIdx.x; q < tot; q += kAmgTailThreads) {
        const int32_t kc = q / wy, r = q - kc * wy, jc = r / w;
        restrict_grid_dof<BS, T, T>(g, V.fz, V.b, t, out, r - jc * w, jc, kc);
    }
}
template <int BS, typename T>
__device__ __forceinline__ void tail_prolong_grid(const AmgTailLevelT<T> &V, const T *e, T *y)
{
    const GridArgs g = V.g;
    const int32_t w = g.fx * BS, wy = w * g.fy, tot = wy * V.fz;
    for (int32_t q = (int32_t)threadIdx.x; q < tot; q += kAmgTailThreads) {
        const int32_t k = q / wy, r = q - k * wy, j = r / w;
        prolong_grid_dof<BS, T, T>(g, V.fz, e, y, r - j * w, j, k);
    }
}
}  // namespace

// STENCIL: a level of the tail may apply A from its value array alone (AmgTailLevel.stencil): amg_stencil_tail_kernel;
// without, the body is amg_tail_kernel as it was before that option existed.  T = float (SPK_AMG_PRECISION_SINGLE): every
// level below the coarsest is a stencil level with matrix-free transfers, and the CSR branches are not compiled
namespace {
template <bool STENCIL, typename T>
__device__ __forceinline__ void tail_run(const AmgTailDescT<T> *__restrict__ d, int32_t s0, int32_t s1)
{
    constexpr bool CSR = std::is_same<T, double>::value;
    for (int32_t s = s0; s < s1; ++s) {
        const AmgTailStep st = d->steps[s];
        const AmgTailLevelT<T> &V = d->lv[st.level];
        T *y = st.sel ? V.yb : V.ya, *o = st.sel ? V.ya : V.yb;   // the level's iterate and the other buffer
        switch (st.kind) {
        case SPK_AMG_STEP_PRE0: tail_smooth<STENCIL, T>(V, nullptr); break;
        case SPK_AMG_STEP_PRE:
        case SPK_AMG_STEP_POST: tail_smooth<STENCIL, T>(V, y); break;
        case SPK_AMG_STEP_DOWN: {   // o = A y, then b of the next level = R (b - o)
            T *bn = d->lv[st.level + 1].b;
            if (STENCIL && V.stencil) tail_stencil<0, T>(V, y, nullptr, o, T(0), T(0));
            else if constexpr (CSR) tail_csr<0>(V.arp, V.aci, V.av, V.n, y, nullptr, nullptr, nullptr, nullptr, o, 0.0, 0.0);
            if (V.matrix_free) {
                if (V.bs == 1) tail_restrict_grid<1, T>(V, o, bn);
                else if (V.bs == 2) tail_restrict_grid<2, T>(V, o, bn);
                else tail_restrict_grid<3, T>(V, o, bn);
                __syncthreads();
            } else if constexpr (CSR) {
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
            const AmgTailLevelT<T> &N = d->lv[st.level + 1];
            const T *e = st.sel_next ? N.yb : N.ya;
            if (V.matrix_free) {
                if (V.bs == 1) tail_prolong_grid<1, T>(V, e, y);
                else if (V.bs == 2) tail_prolong_grid<2, T>(V, e, y);
                else tail_prolong_grid<3, T>(V, e, y);
                __syncthreads();
            } else if constexpr (CSR) {
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
    tail_run<false, double>(d, s0, s1);
}
__global__ __launch_bounds__(kAmgTailThreads) void amg_stencil_tail_kernel(const AmgTailDesc *__restrict__ d, int32_t s0, int32_t s1,
                                                                           const int32_t *__restrict__ done)
{
    if (done && *done) return;
    tail_run<true, double>(d, s0, s1);
}
__global__ __launch_bounds__(kAmgTailThreads) void amg_stencil_tail_f32_kernel(const AmgTailDescF32 *__restrict__ d, int32_t s0, int32_t s1,
                                                                               const int32_t *__restrict__ done)
{
    if (done && *done) return;
    tail_run<true, float>(d, s0, s1);
}

namespace {
// x: the dofs of one node row in workgroups; y, z: the node rows (amg_check_opts keeps both within 65535)
inline dim3 transfer_grid(const int32_t d[3], int bs) { return dim3((unsigned)(((int64_t)d[0] * bs + kThreads - 1) / kThreads), (unsigned)d[1], (unsigned)d[2]); }
}  // namespace

template <typename TI, typename TO>
static void prolong_grid_launch(const AmgGrid &a, const TI *e, TO *y, const int32_t *done, hipStream_t s)
{
    const GridArgs g = grid_args(a);
    const dim3 grid = transfer_grid(a.fd, a.bs);
    if (a.bs == 1) hipLaunchKernelGGL((amg_prolong_grid_kernel<1, TI, TO>), grid, dim3(kThreads), 0, s, g, e, y, done);
    else if (a.bs == 2) hipLaunchKernelGGL((amg_prolong_grid_kernel<2, TI, TO>), grid, dim3(kThreads), 0, s, g, e, y, done);
    else hipLaunchKernelGGL((amg_prolong_grid_kernel<3, TI, TO>), grid, dim3(kThreads), 0, s, g, e, y, done);
}
template <typename TI, typename TO>
static void restrict_grid_launch(const AmgGrid &a, const TI *b, const TI *t, TO *out, const int32_t *done, hipStream_t s)
{
    const GridArgs g = grid_args(a);
    const dim3 grid = transfer_grid(a.cd, a.bs);
    if (a.bs == 1) hipLaunchKernelGGL((amg_restrict_grid_kernel<1, TI, TO>), grid, dim3(kThreads), 0, s, g, a.fd[2], b, t, out, done);
    else if (a.bs == 2) hipLaunchKernelGGL((amg_restrict_grid_kernel<2, TI, TO>), grid, dim3(kThreads), 0, s, g, a.fd[2], b, t, out, done);
    else hipLaunchKernelGGL((amg_restrict_grid_kernel<3, TI, TO>), grid, dim3(kThreads), 0, s, g, a.fd[2], b, t, out, done);
}
void amg_prolong_add_grid(const AmgGrid &a, const double *e, double *y, const int32_t *done, hipStream_t s) { prolong_grid_launch(a, e, y, done, s); }
void amg_prolong_add_grid(const AmgGrid &a, const float *e, float *y, const int32_t *done, hipStream_t s) { prolong_grid_launch(a, e, y, done, s); }
void amg_prolong_add_grid(const AmgGrid &a, const float *e, double *y, const int32_t *done, hipStream_t s) { prolong_grid_launch(a, e, y, done, s); }
void amg_restrict_grid(const AmgGrid &a, const double *b, const double *t, double *out, const int32_t *done, hipStream_t s) { restrict_grid_launch(a, b, t, out, done, s); }
void amg_restrict_grid(const AmgGrid &a, const float *b, const float *t, float *out, const int32_t *done, hipStream_t s) { restrict_grid_launch(a, b, t, out, done, s); }
void amg_restrict_grid(const AmgGrid &a, const double *b, const double *t, float *out, const int32_t *done, hipStream_t s) { restrict_grid_launch(a, b, t, out, done, s); }

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
// rows per workgroup of amg_stencil_kernel (so_wg_rows, spk_stencil_op_core.hpp: whole waves whose longest rows fill at
// most 32 KiB of LDS -- several workgroups per CU -- at most kThreads)
int stencil_op_rows(const int32_t nd[3], int bs, size_t elem)
{
    static_assert(kWave == 64 && kThreads == 256, "so_wg_rows states the wave and the largest workgroup");
    return stencil_op::so_wg_rows(nd, bs, (int32_t)elem);
}
template <int BS, typename T>
static void stencil_op_launch(const StencilOpArgs &g, int rows, size_t lds, int mode, const T *v, const T *x, const T *dinv,
                              const T *b, const T *yo, T *out, T alpha, T beta, const int32_t *done, hipStream_t s)
{
    const dim3 grid((unsigned)((g.n + rows - 1) / rows));
    if constexpr (std::is_same<T, double>::value) {
        if (mode == 0) hipLaunchKernelGGL((amg_stencil_kernel<BS, 0>), grid, dim3(rows), lds, s, g, v, x, dinv, b, yo, out, alpha, beta, done);
        else hipLaunchKernelGGL((amg_stencil_kernel<BS, 1>), grid, dim3(rows), lds, s, g, v, x, dinv, b, yo, out, alpha, beta, done);
    } else {
        if (mode == 0) hipLaunchKernelGGL((amg_stencil_f32_kernel<BS, 0>), grid, dim3(rows), lds, s, g, v, x, dinv, b, yo, out, alpha, beta, done);
        else hipLaunchKernelGGL((amg_stencil_f32_kernel<BS, 1>), grid, dim3(rows), lds, s, g, v, x, dinv, b, yo, out, alpha, beta, done);
    }
}
template <typename T>
static void stencil_op_run(int32_t n, const T *val, const int32_t nd[3], int bs, int mode, const T *x, const T *dinv, const T *b,
                           const T *yo, T *out, T alpha, T beta, const int32_t *done, hipStream_t s)
{
    if (n == 0) return;
    const StencilOpArgs g{nd[0], nd[1], nd[2], n};
    const int rows = stencil_op_rows(nd, bs, sizeof(T));
    // the workgroup's range and the values in front of its begin back to a whole 16-byte piece
    const size_t lds = ((size_t)rows * (size_t)stencil_op::so_max_row(nd, bs) + 16 / sizeof(T)) * sizeof(T);
    if (bs == 1) stencil_op_launch<1>(g, rows, lds, mode, val, x, dinv, b, yo, out, alpha, beta, done, s);
    else if (bs == 2) stencil_op_launch<2>(g, rows, lds, mode, val, x, dinv, b, yo, out, alpha, beta, done, s);
    else stencil_op_launch<3>(g, rows, lds, mode, val, x, dinv, b, yo, out, alpha, beta, done, s);
}
void amg_stencil_op(int32_t n, const double *val, const int32_t nd[3], int bs, int mode, const double *x, const double *dinv,
                    const double *b, const double *yo, double *out, double alpha, double beta, const int32_t *done, hipStream_t s)
{
    stencil_op_run(n, val, nd, bs, mode, x, dinv, b, yo, out, alpha, beta, done, s);
}
void amg_stencil_op(int32_t n, const float *val, const int32_t nd[3], int bs, int mode, const float *x, const float *dinv,
                    const float *b, const float *yo, float *out, float alpha, float beta, const int32_t *done, hipStream_t s)
{
    stencil_op_run(n, val, nd, bs, mode, x, dinv, b, yo, out, alpha, beta, done, s);
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
    hipLaunchKernelGGL(amg_cheb_vec_kernel<double>, vec_grid1(n), dim3(kThreads), 0, s, n, dinv, b, t, y, yo, out, alpha, beta, done);
}
void amg_cheb_vec(int64_t n, const float *dinv, const float *b, const float *t, const float *y, const float *yo, float *out,
                  float alpha, float beta, const int32_t *done, hipStream_t s)
{
    if (n == 0) return;
    hipLaunchKernelGGL(amg_cheb_vec_kernel<float>, vec_grid1(n), dim3(kThreads), 0, s, n, dinv, b, t, y, yo, out, alpha, beta, done);
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
template <typename T>
static void dense_launch(const T *C, int32_t n, const T *b, T *y, const int32_t *done, hipStream_t s)
{
    if (n == 0) return;
    const int rows = kThreads / kWave;
    hipLaunchKernelGGL(amg_dense_kernel<T>, dim3((unsigned)((n + rows - 1) / rows)), dim3(kThreads), 0, s, C, n, b, y, done);
}
void amg_dense(const double *C, int32_t n, const double *b, double *y, const int32_t *done, hipStream_t s) { dense_launch(C, n, b, y, done, s); }
void amg_dense(const float *C, int32_t n, const float *b, float *y, const int32_t *done, hipStream_t s) { dense_launch(C, n, b, y, done, s); }
void amg_tail(const AmgTailDesc *d, bool stencil, int32_t s0, int32_t s1, const int32_t *done, hipStream_t s)
{
    if (s0 >= s1) return;
    if (stencil) hipLaunchKernelGGL(amg_stencil_tail_kernel, dim3(1), dim3(kAmgTailThreads), 0, s, d, s0, s1, done);
    else hipLaunchKernelGGL(amg_tail_kernel, dim3(1), dim3(kAmgTailThreads), 0, s, d, s0, s1, done);
}
void amg_tail(const AmgTailDescF32 *d, bool, int32_t s0, int32_t s1, const int32_t *done, hipStream_t s)
{
    if (s0 >= s1) return;
    hipLaunchKernelGGL(amg_stencil_tail_f32_kernel, dim3(1), dim3(kAmgTailThreads), 0, s, d, s0, s1, done);
}
__global__ __launch_bounds__(kThreads) void amg_round_f32_kernel(int64_t n, const double *__restrict__ src, float *__restrict__ dst)
{
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) dst[i] = (float)src[i];
}
void amg_round_f32(int64_t n, const double *src, float *dst, hipStream_t s)
{
    if (n == 0) return;
    hipLaunchKernelGGL(amg_round_f32_kernel, vec_grid1(n), dim3(kThreads), 0, s, n, src, dst);
}
void amg_out(int mode, int64_t n, const double *src, double *dst, const int32_t *done, hipStream_t s)
{
    if (n == 0) return;
    hipLaunchKernelGGL(amg_out_kernel, vec_grid1(n), dim3(kThreads), 0, s, mode, n, src, dst, done);
}

}  // namespace k
}  // namespace spk
