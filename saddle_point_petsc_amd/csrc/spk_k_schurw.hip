// spk_k_schurw.hip -- PCApply_FieldSplit_Schur with the exact Schur complement of a few constraint rows
// (spk_pc_set_schur_pre, -pc_fieldsplit_schur_precondition full).  gfx950, wave64, FP64, HBM-bound.
//
// The set-up keeps W = A^ ^-1 B^T as m <= 8 dense planes and the Cholesky factor L of S = B W.  A^ ^-1 is symmetric, so
// t = B A^ ^-1 x0 = W^T x0: the multiplier step needs x0 alone, not the V-cycle's result, and the second application of
// A^ ^-1 in the FULL and UPPER factorisations is the rank-m update y0 = A^ ^-1 x0 - W y1.
//   schur_w_dot: t in one pass (x0 in registers while the m planes stream), fixed-order sums and the sentinel finish of
//                spk_device.hpp; the finishing workgroup solves L L^T y1 = t - x1 in one wave.
//   schur_w_out: y0 = src - sum_r y1_r W_r in one pass, 16-byte loads and stores.
// Both take the solver's `done` gate; neither waits on anything but the finish's bounded poll of the partials.
#include "spk_device.hpp"

namespace spk {
namespace k {

namespace {
constexpr int kSwU = 2;            // double2 per thread and tile: with m = 4 planes 8 + 2 16-byte loads in flight per lane
constexpr int kSwMaxBlocks = 512;  // two workgroups per CU: 64 KB of plane loads in flight per CU at m = 4 (32 KiB
                                   // saturate a CU's share of HBM), 512 partial rows for the finish to read

// L L^T y = rhs for m <= 8 in one wave: lane r < m owns entry r, every step broadcasts one finished entry
__device__ __forceinline__ double chol_solve_wave(const double *__restrict__ L, int m, double rhs, int lane)
{
    double acc = rhs;
    for (int j = 0; j < m; ++j) {   // forward: L z = rhs
        const double zj = __shfl(acc, j, kWave) / L[j * m + j];
        if (lane == j) acc = zj;
        else if (lane > j && lane < m) acc -= L[lane * m + j] * zj;
    }
    for (int j = m - 1; j >= 0; --j) {   // backward: L^T y = z
        const double yj = __shfl(acc, j, kWave) / L[j * m + j];
        if (lane == j) acc = yj;
        else if (lane < j) acc -= L[j * m + lane] * yj;
    }
    return acc;
}
}  // namespace

// t_r = W_r . x0 over the first nl entries, r < M; then y1 = S^-1 (t - x1) by the finishing workgroup.
// Tile = kThreads x kSwU double2; the entry behind an odd nl (the first multiplier of the vector x0 lies in) is masked.
template <int M>
__global__ __launch_bounds__(kThreads) void schur_w_dot_kernel(const double *__restrict__ W, int64_t ldw,
                                                               const double *__restrict__ x0, int64_t nl,
                                                               const double *__restrict__ x1, const double *__restrict__ L,
                                                               double *__restrict__ y1, double *__restrict__ partials,
                                                               FinErr fe, const int32_t *__restrict__ done)
{
    if (done && *done) return;
    constexpr int NW = kThreads / kWave;
    __shared__ double lds[kThreads];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n2 = (nl + 1) / 2;
    double acc[M];
#pragma unroll
    for (int r = 0; r < M; ++r) acc[r] = 0.0;
    for (int64_t t0 = (int64_t)blockIdx.x * (kThreads * kSwU); t0 < n2; t0 += (int64_t)gridDim.x * (kThreads * kSwU)) {
        double2 xv[kSwU], wv[M][kSwU];
        int64_t idx[kSwU];
#pragma unroll
        for (int u = 0; u < kSwU; ++u) {
            idx[u] = t0 + u * kThreads + threadIdx.x;
            if (idx[u] < n2) {
                xv[u] = ld2(x0, idx[u]);
                if (2 * idx[u] + 1 >= nl) xv[u].y = 0.0;
            } else {
                xv[u].x = xv[u].y = 0.0;
                idx[u] = 0;
            }
        }
#pragma unroll
        for (int r = 0; r < M; ++r)   // every plane load of the tile is requested before the first product
#pragma unroll
            for (int u = 0; u < kSwU; ++u) wv[r][u] = ld2s<true>(W + (size_t)r * ldw, idx[u]);
#pragma unroll
        for (int r = 0; r < M; ++r)
#pragma unroll
            for (int u = 0; u < kSwU; ++u) acc[r] += wv[r][u].x * xv[u].x + wv[r][u].y * xv[u].y;
    }
#pragma unroll
    for (int r = 0; r < M; ++r) {
        const double sw = wave_sum(acc[r]);
        if (lane == 0) lds[wave * M + r] = sw;
    }
    __syncthreads();
    if ((int)threadIdx.x < M) {
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < NW; ++j) t += lds[j * M + threadIdx.x];
        publish(partials + (size_t)blockIdx.x * kPartialLd + threadIdx.x, t);
    }
    if (!arrive_last(gridDim.x)) return;
    final_reduce(partials, gridDim.x, kPartialLd, M, lds, fe);
    if (wave == 0) {
        const double y = chol_solve_wave(L, M, lane < M ? lds[lane] - x1[lane] : 0.0, lane);
        if (lane < M) y1[lane] = y;
    }
}

// y1 = S^-1 x1 (DIAG) | -S^-1 x1 (UPPER)
__global__ __launch_bounds__(kWave) void schur_w_y1_kernel(const double *__restrict__ L, int m, int fact,
                                                           const double *__restrict__ x1, double *__restrict__ y1,
                                                           const int32_t *__restrict__ done)
{
    if (done && *done) return;
    const int lane = threadIdx.x;
    const double y = chol_solve_wave(L, m, lane < m ? x1[lane] : 0.0, lane);
    if (lane < m) y1[lane] = fact == SPK_SCHUR_UPPER ? -y : y;
}

// y0[i] = s_i - sum_r y1_r W_r[i], s = src or (JAC) dinv .* src.  Whole double2 only: an odd last entry is written alone
// by one thread -- the entry behind it belongs to y1.
template <int M, bool JAC>
__global__ __launch_bounds__(kThreads) void schur_w_out_kernel(const double *__restrict__ W, int64_t ldw,
                                                               const double *__restrict__ src, const double *__restrict__ dinv,
                                                               const double *__restrict__ y1, double *__restrict__ y0, int64_t nl,
                                                               const int32_t *__restrict__ done)
{
    if (done && *done) return;
    double c[M];
#pragma unroll
    for (int r = 0; r < M; ++r) c[r] = y1[r];
    const int64_t n2 = nl / 2;
    for (int64_t t0 = (int64_t)blockIdx.x * (kThreads * kSwU); t0 < n2; t0 += (int64_t)gridDim.x * (kThreads * kSwU)) {
        double2 sv[kSwU], dv[kSwU], wv[M][kSwU];
        int64_t idx[kSwU];
        bool live[kSwU];
#pragma unroll
        for (int u = 0; u < kSwU; ++u) {
            idx[u] = t0 + u * kThreads + threadIdx.x;
            live[u] = idx[u] < n2;
            if (!live[u]) idx[u] = 0;
            sv[u] = ld2(src, idx[u]);
            if (JAC) dv[u] = ld2(dinv, idx[u]);
        }
#pragma unroll
        for (int r = 0; r < M; ++r)
#pragma unroll
            for (int u = 0; u < kSwU; ++u) wv[r][u] = ld2s<true>(W + (size_t)r * ldw, idx[u]);
#pragma unroll
        for (int u = 0; u < kSwU; ++u) {
            double2 v = sv[u];
            if (JAC) { v.x *= dv[u].x; v.y *= dv[u].y; }
#pragma unroll
            for (int r = 0; r < M; ++r) { v.x -= c[r] * wv[r][u].x; v.y -= c[r] * wv[r][u].y; }
            if (live[u]) reinterpret_cast<double2 *>(y0)[idx[u]] = v;
        }
    }
    if ((nl & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t i = nl - 1;
        double v = JAC ? src[i] * dinv[i] : src[i];
#pragma unroll
        for (int r = 0; r < M; ++r) v -= c[r] * W[(size_t)r * ldw + i];
        y0[i] = v;
    }
}

namespace {
inline int sw_grid(int64_t n2)
{
    const int64_t tiles = (n2 + kThreads * kSwU - 1) / (kThreads * kSwU);
    return (int)std::max<int64_t>(std::min<int64_t>(tiles, kSwMaxBlocks), 1);
}
inline void check_args(const SchurW &w, const void *a, const void *b)
{
    if (w.m < 1 || w.m > 8 || !w.W || !w.L) fail(SPK_ERR_STATE, "schur_w: no dense Schur complement of 1..8 rows");
    if (((uintptr_t)w.W | (uintptr_t)a | (uintptr_t)b | (uintptr_t)(w.ldw * 8)) & 15)
        fail(SPK_ERR_ARG, "schur_w: vectors and planes must be 16-byte aligned");
}
}  // namespace

#define SPK_SW_CASES(X) \
    switch (w.m) {      \
    case 1: X(1); break; case 2: X(2); break; case 3: X(3); break; case 4: X(4); break; \
    case 5: X(5); break; case 6: X(6); break; case 7: X(7); break; default: X(8); break; \
    }

void schur_w_dot(const SchurW &w, const double *x0, int64_t nl, const double *x1, double *y1, const Finish &f,
                 const int32_t *done, hipStream_t s)
{
    check_args(w, x0, nullptr);
    const int grid = sw_grid((nl + 1) / 2);
#define SPK_SW_DOT(MM) hipLaunchKernelGGL(schur_w_dot_kernel<MM>, dim3(grid), dim3(kThreads), 0, s, w.W, w.ldw, x0, nl, x1, \
                                          w.L, y1, f.partials, FinErr{f.err, f.fin_ticks}, done)
    SPK_SW_CASES(SPK_SW_DOT)
#undef SPK_SW_DOT
}

void schur_w_y1(const SchurW &w, int fact, const double *x1, double *y1, const int32_t *done, hipStream_t s)
{
    check_args(w, nullptr, nullptr);
    hipLaunchKernelGGL(schur_w_y1_kernel, dim3(1), dim3(kWave), 0, s, w.L, w.m, fact, x1, y1, done);
}

void schur_w_out(const SchurW &w, const double *src, const double *dinv, const double *y1, double *y0, int64_t nl,
                 const int32_t *done, hipStream_t s)
{
    check_args(w, src, y0);
    if (dinv && ((uintptr_t)dinv & 15)) fail(SPK_ERR_ARG, "schur_w: vectors and planes must be 16-byte aligned");
    if (nl == 0) return;
    const int grid = sw_grid(nl / 2);
#define SPK_SW_OUT(MM)                                                                                                          \
    do {                                                                                                                        \
        if (dinv) hipLaunchKernelGGL((schur_w_out_kernel<MM, true>), dim3(grid), dim3(kThreads), 0, s, w.W, w.ldw, src, dinv,   \
                                     y1, y0, nl, done);                                                                         \
        else hipLaunchKernelGGL((schur_w_out_kernel<MM, false>), dim3(grid), dim3(kThreads), 0, s, w.W, w.ldw, src, dinv, y1,  \
                                y0, nl, done);                                                                                  \
    } while (0)
    SPK_SW_CASES(SPK_SW_OUT)
#undef SPK_SW_OUT
}
#undef SPK_SW_CASES

}  // namespace k
}  // namespace spk
