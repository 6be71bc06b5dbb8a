// spk_k_amg_setup.hip -- the multigrid set-up on the device (-spk_gamg_setup device; host sequencing: amg_build_device
// in spk_amg_setup.cpp).  gfx950, wave64, FP64.  Node graph, tentative prolongator, Lanczos vector passes, CSR x CSR, union
// add and transpose; for the refresh of a kept hierarchy (amg_refresh_ctx) the pattern comparison and the numeric
// product and symmetrisation on known patterns; for grid coarsening the prolongator and the grid-stencil Galerkin product
// (amgs_galerkin_stencil...) in closed form.  Set-up runs before any solve: no launch here takes the solver's `done` gate.
//
// Every kernel is deterministic.  The sparse kernels work one row (or node) per thread in the host builder's traversal
// order, and where the host's result depends on the order and rounding of a sum (the strong-connection test, the
// entries of the products) the sum is written with unfused multiplies and adds in that order: the x86-64 host build has
// no FMA, the device contracts by default.  Integer atomics allocate slots only where a sort follows; there are no
// floating-point atomics.
#include "spk_device.hpp"
#include "spk_galerkin_core.hpp"

namespace spk {
namespace k {

namespace {
inline dim3 row_grid(int64_t n) { return dim3((unsigned)std::max<int64_t>((n + kThreads - 1) / kThreads, 1)); }
inline int lz_grid(int64_t n) { return (int)std::max<int64_t>(std::min<int64_t>((n + kVT - 1) / kVT, kVecMaxBlocks), 1); }
}  // namespace

// ---------------------------------------------------------------------------
// sorted columns
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void amgs_rows_sorted_kernel(const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                                    int32_t n, int32_t *flag)
{
    const int32_t i = (int32_t)(blockIdx.x * kThreads + threadIdx.x);
    if (i >= n) return;
    bool bad = false;
    for (int32_t k = rp[i] + 1; k < rp[i + 1]; ++k) bad = bad || ci[k - 1] > ci[k];
    if (bad) atomicOr(flag, 1);
}

// insertion sort of every row by column, one row per thread (any row length; rows are short or nearly sorted here)
__global__ __launch_bounds__(kThreads) void amgs_sort_rows_kernel(const int32_t *__restrict__ rp, int32_t *ci, double *v, int32_t n)
{
    const int32_t i = (int32_t)(blockIdx.x * kThreads + threadIdx.x);
    if (i >= n) return;
    const int32_t k0 = rp[i], k1 = rp[i + 1];
    for (int32_t k = k0 + 1; k < k1; ++k) {
        const int32_t c = ci[k];
        if (ci[k - 1] <= c) continue;
        const double x = v[k];
        int32_t t = k;
        for (; t > k0 && ci[t - 1] > c; --t) {
            ci[t] = ci[t - 1];
            v[t] = v[t - 1];
        }
        ci[t] = c;
        v[t] = x;
    }
}

// ---------------------------------------------------------------------------
// strong-connection graph of the bs x bs nodes (node_graph of the host builder): one node per thread, a bs-way merge
// over the node's sorted rows -- the neighbours come out ascending, and the squares of a block are added row by row,
// entry by entry, as the host adds them
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void amgs_node_norms_kernel(const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                                   const double *__restrict__ v, int32_t nn, int bs,
                                                                   double *__restrict__ dn)
{
    const int32_t I = (int32_t)(blockIdx.x * kThreads + threadIdx.x);
    if (I >= nn) return;
    double acc = 0.0;
    for (int32_t r = I * bs; r < (I + 1) * bs; ++r)
        for (int32_t k = rp[r]; k < rp[r + 1]; ++k)
            if (ci[k] / bs == I) acc = __dadd_rn(acc, __dmul_rn(v[k], v[k]));
    dn[I] = __dsqrt_rn(acc);
}

// FILL = false: out[I] = number of strong neighbours; FILL = true: the neighbours at out[gp[I]..)
template <bool FILL>
__global__ __launch_bounds__(kThreads) void amgs_graph_kernel(const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                              const double *__restrict__ v, int32_t nn, int bs, double theta,
                                                              const double *__restrict__ dn, const int32_t *__restrict__ gp,
                                                              int32_t *__restrict__ out)
{
    const int32_t I = (int32_t)(blockIdx.x * kThreads + threadIdx.x);
    if (I >= nn) return;
    int32_t p[3] = {0, 0, 0}, e[3] = {0, 0, 0};
#pragma unroll
    for (int r = 0; r < 3; ++r)
        if (r < bs) {
            p[r] = rp[I * bs + r];
            e[r] = rp[I * bs + r + 1];
        }
    const double dI = dn[I];
    const int32_t base = FILL ? gp[I] : 0;
    int32_t cnt = 0;
    for (;;) {
        int32_t J = INT32_MAX;
#pragma unroll
        for (int r = 0; r < 3; ++r)
            if (p[r] < e[r]) J = min(J, ci[p[r]] / bs);
        if (J == INT32_MAX) break;
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
            while (p[r] < e[r] && ci[p[r]] / bs == J) {
                const double a = v[p[r]];
                acc = __dadd_rn(acc, __dmul_rn(a, a));
                ++p[r];
            }
        if (J == I) continue;
        if (__dsqrt_rn(acc) > __dmul_rn(theta, __dsqrt_rn(__dmul_rn(dI, dn[J])))) {
            if (FILL) out[base + cnt] = J;
            ++cnt;
        }
    }
    if (!FILL) out[I] = cnt;
}

// ---------------------------------------------------------------------------
// tentative prolongator from the aggregates: row node * bs + c holds inv[aggregate] in column aggregate * bs + c
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void amgs_tent_count_kernel(const int32_t *__restrict__ agg, int32_t nrows, int bs,
                                                                   int32_t *__restrict__ cnt)
{
    const int32_t i = (int32_t)(blockIdx.x * kThreads + threadIdx.x);
    if (i < nrows) cnt[i] = agg[i / bs] >= 0 ? 1 : 0;
}
__global__ __launch_bounds__(kThreads) void amgs_tent_fill_kernel(const int32_t *__restrict__ agg, const double *__restrict__ inv,
                                                                  int32_t nrows, int bs, const int32_t *__restrict__ rp,
                                                                  int32_t *__restrict__ ci, double *__restrict__ v)
{
    const int32_t i = (int32_t)(blockIdx.x * kThreads + threadIdx.x);
    if (i >= nrows) return;
    const int32_t a = agg[i / bs];
    if (a < 0) return;
    ci[rp[i]] = a * bs + i % bs;
    v[rp[i]] = inv[a];
}

// ---------------------------------------------------------------------------
// grid coarsening: P = P_z (x) P_y (x) P_x (x) I_bs from the node grids alone, one row (fine dof) per thread.  i + i / 2
// parents lie before fine index i of a halved direction (i of one that keeps its nodes), so the row's offset follows
// from its indices: no count, no scan.  The last index of an even halved side (an odd index that is the last one) is a
// coarse node itself: one parent, (i + 1) / 2, so such a side has fx + fx / 2 - 1 parents.  Columns ascend (z
// outermost), the weights are 1, 1/2, 1/4 or 1/8.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void amgs_grid_prolongator_kernel(int32_t fx, int32_t fy, int32_t fz, int32_t cx, int32_t cy,
                                                                         int32_t cz, int bs, int32_t *__restrict__ rp,
                                                                         int32_t *__restrict__ ci, double *__restrict__ v)
{
    const int64_t nrows = (int64_t)fx * fy * fz * bs, f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= nrows) return;
    const int32_t node = (int32_t)(f / bs), c = (int32_t)(f - (int64_t)node * bs);
    const int32_t i = node % fx, j = (node / fx) % fy, k = node / fx / fy;
    const bool hx = cx != fx, hy = cy != fy, hz = cz != fz;
    const int32_t lx = hx && (i & 1) && i == fx - 1, ly = hy && (j & 1) && j == fy - 1, lz = hz && (k & 1) && k == fz - 1;
    const int32_t nx = hx && (i & 1) && !lx ? 2 : 1, ny = hy && (j & 1) && !ly ? 2 : 1, nz = hz && (k & 1) && !lz ? 2 : 1;
    const int32_t ic = hx ? (i + lx) >> 1 : i, jc = hy ? (j + ly) >> 1 : j, kc = hz ? (k + lz) >> 1 : k;
    // parents before this index per direction, and in a whole direction
    const int64_t bx = hx ? i + (i >> 1) : i, by = hy ? j + (j >> 1) : j, bz = hz ? k + (k >> 1) : k;
    const int64_t tx = hx ? fx + (fx >> 1) - !(fx & 1) : fx, ty = hy ? fy + (fy >> 1) - !(fy & 1) : fy;
    const int32_t len = nx * ny * nz;
    int64_t p = (tx * ty * bz + nz * (tx * by + ny * bx)) * bs + (int64_t)c * len;
    rp[f] = (int32_t)p;
    if (f + 1 == nrows) rp[nrows] = (int32_t)(p + len);
    const double w = 1.0 / (double)len;
    for (int32_t kk = 0; kk < nz; ++kk)
        for (int32_t jj = 0; jj < ny; ++jj)
            for (int32_t ii = 0; ii < nx; ++ii, ++p) {
                ci[p] = (((kc + kk) * cy + jc + jj) * cx + ic + ii) * bs + c;
                v[p] = w;
            }
}

// ---------------------------------------------------------------------------
// C = A B, one row per thread.  bound: what a row can hold at most (its number of products, or every column of B);
// expand: the row's slice of the scratch keeps a sorted list of (column, sum) -- a product finds its column by bisection
// or opens it by shifting the tail -- so each entry is summed in A's stored order, then B's, from 0, as the host's dense
// accumulator sums it; compact: the slices packed behind the scanned counts.  Correct for any row length (a long row
// costs its thread time, nothing else).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void amgs_spgemm_bound_kernel(const int32_t *__restrict__ arp, const int32_t *__restrict__ aci,
                                                                     const int32_t *__restrict__ brp, int32_t n, int32_t ncols_b,
                                                                     int32_t *__restrict__ bound, unsigned long long *total)
{
    __shared__ unsigned long long blk;
    if (threadIdx.x == 0) blk = 0ull;
    __syncthreads();
    const int32_t i = (int32_t)(blockIdx.x * kThreads + threadIdx.x);
    if (i < n) {
        int64_t s = 0;
        for (int32_t k = arp[i]; k < arp[i + 1]; ++k) s += brp[aci[k] + 1] - brp[aci[k]];
        if (s > ncols_b) s = ncols_b;
        bound[i] = (int32_t)s;
        atomicAdd(&blk, (unsigned long long)s);
    }
    __syncthreads();
    if (threadIdx.x == 0 && blk) atomicAdd(total, blk);
}

__global__ __launch_bounds__(kThreads) void amgs_spgemm_expand_kernel(const int32_t *__restrict__ arp, const int32_t *__restrict__ aci,
                                                                      const double *__restrict__ av, const int32_t *__restrict__ brp,
                                                                      const int32_t *__restrict__ bci, const double *__restrict__ bv,
                                                                      int32_t n, const int32_t *__restrict__ off, int32_t *sc,
                                                                      double *sv, int32_t *__restrict__ cnt)
{
    const int32_t i = (int32_t)(blockIdx.x * kThreads + threadIdx.x);
    if (i >= n) return;
    int32_t *c = sc + (size_t)off[i];
    double *w = sv + (size_t)off[i];
    int32_t len = 0;
    for (int32_t k = arp[i]; k < arp[i + 1]; ++k) {
        const int32_t r = aci[k];
        const double a = av[k];
        for (int32_t q = brp[r]; q < brp[r + 1]; ++q) {
            const int32_t j = bci[q];
            const double p = __dmul_rn(a, bv[q]);
            int32_t lo = 0, hi = len;
            if (len > 0 && c[len - 1] < j) lo = len;   // the common case: columns arrive ascending
            while (lo < hi) {
                const int32_t mid = (lo + hi) >> 1;
                if (c[mid] < j) lo = mid + 1; else hi = mid;
            }
            if (lo < len && c[lo] == j) {
                w[lo] = __dadd_rn(w[lo], p);
            } else {
                for (int32_t t = len; t > lo; --t) {
                    c[t] = c[t - 1];
                    w[t] = w[t - 1];
                }
                c[lo] = j;
                w[lo] = __dadd_rn(0.0, p);
                ++len;
            }
        }
    }
    cnt[i] = len;
}

__global__ __launch_bounds__(kThreads) void amgs_compact_kernel(int32_t n, const int32_t *__restrict__ off, const int32_t *__restrict__ rp,
                                                                const int32_t *__restrict__ sc, const double *__restrict__ sv,
                                                                int32_t *__restrict__ ci, double *__restrict__ v)
{
    const int32_t i = (int32_t)(blockIdx.x * kThreads + threadIdx.x);
    if (i >= n) return;
    const int32_t k0 = rp[i], len = rp[i + 1] - k0;
    const size_t o = (size_t)off[i];
    for (int32_t t = 0; t < len; ++t) {
        ci[k0 + t] = sc[o + t];
        v[k0 + t] = sv[o + t];
    }
}

// ---------------------------------------------------------------------------
// C = a A + b diag(scale) B over the union of the sorted patterns (scale null: 1), one row per thread
// FILL = false: cnt[i] = the row's length; FILL = true: the row at crp[i]
// ---------------------------------------------------------------------------
template <bool FILL>
__global__ __launch_bounds__(kThreads) void amgs_add_kernel(int32_t n, double a, const int32_t *__restrict__ arp,
                                                            const int32_t *__restrict__ aci, const double *__restrict__ av, double b,
                                                            const int32_t *__restrict__ brp, const int32_t *__restrict__ bci,
                                                            const double *__restrict__ bv, const double *__restrict__ scale,
                                                            const int32_t *__restrict__ crp, int32_t *__restrict__ cci,
                                                            double *__restrict__ cv, int32_t *__restrict__ cnt)
{
    const int32_t i = (int32_t)(blockIdx.x * kThreads + threadIdx.x);
    if (i >= n) return;
    int32_t p = arp[i], q = brp[i], o = FILL ? crp[i] : 0;
    const int32_t pe = arp[i + 1], qe = brp[i + 1];
    const double sc = scale ? scale[i] : 1.0;
    while (p < pe || q < qe) {
        const int32_t ca = p < pe ? aci[p] : INT32_MAX, cb = q < qe ? bci[q] : INT32_MAX;
        if (FILL) {
            double x;
            if (ca == cb) x = __dadd_rn(__dmul_rn(a, av[p]), __dmul_rn(b, scale ? __dmul_rn(bv[q], sc) : bv[q]));
            else if (ca < cb) x = __dmul_rn(a, av[p]);
            else x = __dmul_rn(b, scale ? __dmul_rn(bv[q], sc) : bv[q]);
            cci[o] = ca < cb ? ca : cb;
            cv[o] = x;
        }
        if (ca <= cb) ++p;
        if (cb <= ca) ++q;
        ++o;
    }
    if (!FILL) cnt[i] = o;
}

// ---------------------------------------------------------------------------
// transpose: entries per column (integer atomics), scan, slots handed out by integer atomics, then every row of the
// result sorted by column -- the columns of a row are distinct, so the result does not depend on who got which slot
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void amgs_col_count_kernel(const int32_t *__restrict__ ci, int64_t nnz, int32_t *cnt)
{
    const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k < nnz) atomicAdd(cnt + ci[k], 1);
}
__global__ __launch_bounds__(kThreads) void amgs_transpose_fill_kernel(const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                                       const double *__restrict__ v, int32_t n, int32_t *pos,
                                                                       int32_t *__restrict__ tci, double *__restrict__ tv)
{
    const int32_t i = (int32_t)(blockIdx.x * kThreads + threadIdx.x);
    if (i >= n) return;
    for (int32_t k = rp[i]; k < rp[i + 1]; ++k) {
        const int32_t p = atomicAdd(pos + ci[k], 1);
        tci[p] = i;
        tv[p] = v[k];
    }
}

// ---------------------------------------------------------------------------
// the refresh (spk_pc_set_amg_reuse): new values on the patterns a build kept.  Nothing is counted, scanned or
// allocated; a thread writes inside its own row only, and what cannot happen on patterns that belong together (a column
// outside the matrix, a product without a slot) sets err[0] instead of a store
// ---------------------------------------------------------------------------
// flag |= 1 where two int32 arrays differ (the pattern a hierarchy was built on against the context's)
__global__ __launch_bounds__(kThreads) void amgs_pattern_equal_kernel(const int32_t *__restrict__ a, const int32_t *__restrict__ b,
                                                                      int64_t n, int32_t *flag)
{
    const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k < n && a[k] != b[k]) atomicOr(flag, 1);
}

namespace {
// position of column j in the ascending ci[lo, hi), or -1
__device__ __forceinline__ int32_t find_col(const int32_t *__restrict__ ci, int32_t lo, int32_t hi, int32_t j)
{
    const int32_t end = hi;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (ci[mid] < j) lo = mid + 1; else hi = mid;
    }
    return lo < end && ci[lo] == j ? lo : -1;
}
// __dmul_rn / __dadd_rn as the expand kernel compiles them: a multiply and an add of their own.  The header's versions are
// a plain * and +, which the compiler contracts where a product has one use -- as it has here, and has not there
__device__ __forceinline__ double mul_unfused(double x, double y)
{
#pragma clang fp contract(off)
    return x * y;
}
__device__ __forceinline__ double add_unfused(double x, double y)
{
#pragma clang fp contract(off)
    return x + y;
}
}  // namespace

// the values of C = A B on C's sorted pattern, one row per thread: the products in the order of amgs_spgemm_expand_kernel
// (A's stored order, then B's; unfused; every entry summed from 0), so unchanged values give the build's bits
__global__ __launch_bounds__(kThreads) void amgs_spgemm_numeric_kernel(const int32_t *__restrict__ arp, const int32_t *__restrict__ aci,
                                                                       const double *__restrict__ av, const int32_t *__restrict__ brp,
                                                                       const int32_t *__restrict__ bci, const double *__restrict__ bv,
                                                                       int32_t n, int32_t nrows_b, const int32_t *__restrict__ crp,
                                                                       const int32_t *__restrict__ cci, double *cv, int32_t *err)
{
    const int32_t i = (int32_t)(blockIdx.x * kThreads + threadIdx.x);
    if (i >= n) return;
    const int32_t k0 = crp[i], k1 = crp[i + 1];
    for (int32_t t = k0; t < k1; ++t) cv[t] = 0.0;
    bool bad = false;
    for (int32_t k = arp[i]; k < arp[i + 1]; ++k) {
        const int32_t r = aci[k];
        if (r < 0 || r >= nrows_b) { bad = true; continue; }
        const double a = av[k];
        for (int32_t q = brp[r]; q < brp[r + 1]; ++q) {
            const double p = mul_unfused(a, bv[q]);
            const int32_t t = find_col(cci, k0, k1, bci[q]);
            if (t < 0) bad = true;
            else cv[t] = add_unfused(cv[t], p);
        }
    }
    if (bad) atomicOr(err, 1);
}

// N = (Ac + Ac^T) / 2 on N's sorted pattern, one row per thread: N(i,j) from Ac(i,j) and Ac(j,i) with the expressions of
// amgs_add_kernel<true> at a = b = 0.5 (an absent entry contributes nothing) -- the build's bits again, fused or not:
// a product with 0.5 is exact
__global__ __launch_bounds__(kThreads) void amgs_symmetrise_numeric_kernel(const int32_t *__restrict__ crp, const int32_t *__restrict__ cci,
                                                                           const double *__restrict__ cv, int32_t n,
                                                                           const int32_t *__restrict__ nrp, const int32_t *__restrict__ nci,
                                                                           double *__restrict__ nv, int32_t *err)
{
    const int32_t i = (int32_t)(blockIdx.x * kThreads + threadIdx.x);
    if (i >= n) return;
    bool bad = false;
    for (int32_t t = nrp[i]; t < nrp[i + 1]; ++t) {
        const int32_t j = nci[t];
        double x = 0.0;
        if (j < 0 || j >= n) {
            bad = true;
        } else {
            const int32_t p = find_col(cci, crp[i], crp[i + 1], j), q = find_col(cci, crp[j], crp[j + 1], i);
            if (p >= 0 && q >= 0) x = __dadd_rn(__dmul_rn(0.5, cv[p]), __dmul_rn(0.5, cv[q]));
            else if (p >= 0) x = __dmul_rn(0.5, cv[p]);
            else if (q >= 0) x = __dmul_rn(0.5, cv[q]);
            else bad = true;
        }
        nv[t] = x;
    }
    if (bad) atomicOr(err, 1);
}

// ---------------------------------------------------------------------------
// Lanczos on D^-1/2 A D^-1/2 (lanczos of the host builder): the vector steps as fused passes, each with one sum,
// reduced in a fixed order by the sentinel finish (spk_device.hpp)
// ---------------------------------------------------------------------------
namespace {
// true in thread 0 of the reducing workgroup, with the sum in red[0]
__device__ __forceinline__ bool lz_reduce(double acc, double *red, double *partials, FinErr fe)
{
    const double s = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < kVWaves; ++j) t += red[j];
        publish(partials + (size_t)blockIdx.x * kPartialLd, t);
    }
    if (!arrive_last(gridDim.x)) return false;
    final_reduce(partials, gridDim.x, kPartialLd, 1, red, fe);
    return threadIdx.x == 0;
}
__device__ __forceinline__ void lz_finish(double acc, double *red, double *partials, double *out, FinErr fe)
{
    if (lz_reduce(acc, red, partials, fe)) out[0] = red[0];
}

// The element passes of the four Lanczos kernels, each written once: the stepwise kernels take their scalars as
// arguments, the resident ones (SPK_AMG_LANCZOS_RESIDENT) load them from the state block, and both run these bodies --
// device code contracts a * b + c, so an expression written twice could round differently in its two copies.
__device__ __forceinline__ double lz_init_pass(int64_t n, const double *__restrict__ dinv, double dscale, double *__restrict__ sv,
                                               double *__restrict__ q)
{
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kVT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kVT) {
        sv[i] = sqrt(fabs(dinv[i] * dscale));
        uint32_t h = (uint32_t)i * 2654435761u + 0x9e3779b9u;
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        const double x = 0.5 + (double)(h & 0xffffu) / 65536.0;
        q[i] = x;
        acc += x * x;
    }
    return acc;
}
__device__ __forceinline__ void lz_scale_pass(int64_t n, double nb, const double *w, const double *__restrict__ sv, double *q,
                                              double *__restrict__ t)
{
    for (int64_t i = (int64_t)blockIdx.x * kVT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kVT) {
        const double x = w[i] / nb;
        q[i] = x;
        t[i] = sv[i] * x;
    }
}
__device__ __forceinline__ double lz_dot_pass(int64_t n, const double *__restrict__ sv, const double *__restrict__ aw, double ascale,
                                              double *__restrict__ w, const double *__restrict__ q)
{
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kVT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kVT) {
        const double x = sv[i] * (aw[i] * ascale);
        w[i] = x;
        acc += x * q[i];
    }
    return acc;
}
__device__ __forceinline__ double lz_update_pass(int64_t n, double a, double be, const double *__restrict__ q,
                                                 const double *__restrict__ qp, double *__restrict__ w)
{
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kVT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kVT) {
        const double x = w[i] - (a * q[i] + be * qp[i]);
        w[i] = x;
        acc += x * x;
    }
    return acc;
}
}  // namespace

// out[0] = sum |x|
__global__ __launch_bounds__(kVT) void amgs_abs_sum_kernel(int64_t n, const double *__restrict__ x, double *partials, double *out,
                                                           FinErr fe)
{
    __shared__ double red[kVT];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kVT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kVT) acc += fabs(x[i]);
    lz_finish(acc, red, partials, out, fe);
}
// sv = sqrt|dinv dscale| (dscale: a power of two, 1 on a build), q = the integer-hash start vector (not yet normalised),
// out[0] = q.q
__global__ __launch_bounds__(kVT) void amgs_lz_init_kernel(int64_t n, const double *__restrict__ dinv, double dscale,
                                                           double *__restrict__ sv, double *__restrict__ q, double *partials,
                                                           double *out, FinErr fe)
{
    __shared__ double red[kVT];
    lz_finish(lz_init_pass(n, dinv, dscale, sv, q), red, partials, out, fe);
}
// q = w / nb, t = sv q   (w may be q)
__global__ __launch_bounds__(kVT) void amgs_lz_scale_kernel(int64_t n, double nb, const double *w, const double *__restrict__ sv,
                                                            double *q, double *__restrict__ t)
{
    lz_scale_pass(n, nb, w, sv, q, t);
}
// w = sv (aw ascale) (ascale: a power of two, 1 on a build: the product with it is exact), out[0] = w.q
__global__ __launch_bounds__(kVT) void amgs_lz_dot_kernel(int64_t n, const double *__restrict__ sv, const double *__restrict__ aw,
                                                          double ascale, double *__restrict__ w, const double *__restrict__ q, double *partials,
                                                          double *out, FinErr fe)
{
    __shared__ double red[kVT];
    lz_finish(lz_dot_pass(n, sv, aw, ascale, w, q), red, partials, out, fe);
}
// w -= a q + be qp, out[0] = w.w
__global__ __launch_bounds__(kVT) void amgs_lz_update_kernel(int64_t n, double a, double be, const double *__restrict__ q,
                                                             const double *__restrict__ qp, double *__restrict__ w, double *partials,
                                                             double *out, FinErr fe)
{
    __shared__ double red[kVT];
    lz_finish(lz_update_pass(n, a, be, q, qp, w), red, partials, out, fe);
}

// The resident variants (SPK_AMG_LANCZOS_RESIDENT): the same passes and the same finish in the same launch geometry, so
// every sum is the stepwise route's to the bit; the scalars are plain loads from the state block at entry (the kernel
// boundary on the one stream has made the previous finisher's stores visible), and thread 0 of the reducing workgroup
// applies the host loop's rule to the sum (spk_lanczos_core.hpp) with ordinary stores.  `stopped` is the same in every
// workgroup of a launch -- only an earlier launch's finisher writes it -- so behind the break a whole launch returns
// before it touches a vector or the partials, and the sentinels stay armed.
__global__ __launch_bounds__(kVT) void amgs_lz_init_resident_kernel(int64_t n, const double *__restrict__ dinv, double dscale,
                                                                    double *__restrict__ sv, double *__restrict__ q, double *partials,
                                                                    lanczos_core::LzState *st, FinErr fe)
{
    __shared__ double red[kVT];
    if (st->stopped) return;   // (never set here: the block is zeroed in front of this launch)
    if (lz_reduce(lz_init_pass(n, dinv, dscale, sv, q), red, partials, fe)) lanczos_core::lz_after_init(st, red[0]);
}
// jb < 0: the start vector's norm, else be[jb]
__global__ __launch_bounds__(kVT) void amgs_lz_scale_resident_kernel(int64_t n, int jb, const double *w, const double *__restrict__ sv,
                                                                     double *q, double *__restrict__ t, const lanczos_core::LzState *st)
{
    if (st->stopped) return;
    const double nb = jb < 0 ? st->nq : st->be[jb];
    lz_scale_pass(n, nb, w, sv, q, t);
}
__global__ __launch_bounds__(kVT) void amgs_lz_dot_resident_kernel(int64_t n, int j, const double *__restrict__ sv,
                                                                   const double *__restrict__ aw, double ascale, double *__restrict__ w,
                                                                   const double *__restrict__ q, double *partials,
                                                                   lanczos_core::LzState *st, FinErr fe)
{
    __shared__ double red[kVT];
    if (st->stopped) return;
    if (lz_reduce(lz_dot_pass(n, sv, aw, ascale, w, q), red, partials, fe)) lanczos_core::lz_after_dot(st, j, red[0]);
}
__global__ __launch_bounds__(kVT) void amgs_lz_update_resident_kernel(int64_t n, int j, int kk, const double *__restrict__ q,
                                                                      const double *__restrict__ qp, double *__restrict__ w,
                                                                      double *partials, lanczos_core::LzState *st, FinErr fe)
{
    __shared__ double red[kVT];
    if (st->stopped) return;
    const double a = st->al[j], be = st->be[j];
    if (lz_reduce(lz_update_pass(n, a, be, q, qp, w), red, partials, fe)) lanczos_core::lz_after_update(st, j, kk, red[0]);
}

// ---------------------------------------------------------------------------
// the grid-stencil Galerkin product (SPK_AMG_GALERKIN_STENCIL; the arithmetic: spk_galerkin_core.hpp).  One thread per
// (coarse row, neighbour node): it walks the <= 3^d fine rows of the row's node once, keeps the bs sums of its block row
// in registers and writes bs consecutive columns and values, so the lanes of a wave fill consecutive entries of a few
// coarse rows while they read the same few fine rows out of cache.  (One thread per coarse row would carry 3^d bs
// accumulators -- 81 doubles in 3-D -- and write with a stride of a row.)  The thread of the node itself writes the row
// pointer.  A second launch symmetrises in place: the owner of a pair (row <= column) reads both raw sums and writes
// both entries, so nothing is scattered and nothing is atomic.  No scratch, no count, no scan.
// ---------------------------------------------------------------------------
namespace gs = galerkin;
template <int BS>
__global__ __launch_bounds__(kThreads) void amgs_galerkin_stencil_kernel(gs::GsGrid g, const int32_t *__restrict__ arp,
                                                                         const int32_t *__restrict__ aci, const double *__restrict__ av,
                                                                         int32_t *__restrict__ rp, int32_t *__restrict__ ci,
                                                                         double *__restrict__ v)
{
    const int32_t cd[3] = {g.d[0].n, g.d[1].n, g.d[2].n};
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    gs::GsItem it;
    if (t >= gs::gs_items(cd, BS) || !gs::gs_item(cd, BS, t, &it)) return;
    gs::gs_gather<BS>(g, arp, aci, av, it, rp, ci, v);
}
template <int BS>
__global__ __launch_bounds__(kThreads) void amgs_galerkin_stencil_sym_kernel(int32_t cx, int32_t cy, int32_t cz, double *v)
{
    const int32_t cd[3] = {cx, cy, cz};
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    gs::GsItem it;
    if (t >= gs::gs_items(cd, BS) || !gs::gs_item(cd, BS, t, &it)) return;
    gs::gs_symmetrise<BS>(cd, it, v);
}
// level 0's condition, one row per thread: *bad = min(*bad, row << 32 | column) over the entries whose nodes are not
// neighbours (the caller sets all ones)
__global__ __launch_bounds__(kThreads) void amgs_galerkin_stencil_check_kernel(int32_t fx, int32_t fy, int32_t fz, int bs,
                                                                               const int32_t *__restrict__ arp,
                                                                               const int32_t *__restrict__ aci, unsigned long long *bad)
{
    const int32_t fd[3] = {fx, fy, fz};
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= (int64_t)fx * fy * fz * bs) return;
    const int32_t c = gs::gs_check_row(fd, bs, arp, aci, r);
    if (c >= 0) atomicMin(bad, ((unsigned long long)r << 32) | (unsigned long long)(uint32_t)c);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
template <int BS>
static void galerkin_stencil_launch(const gs::GsGrid &g, const CsrDev &A, CsrDev &N, hipStream_t s)
{
    const int32_t cd[3] = {g.d[0].n, g.d[1].n, g.d[2].n};
    const dim3 grid = row_grid(gs::gs_items(cd, BS));
    hipLaunchKernelGGL(amgs_galerkin_stencil_kernel<BS>, grid, dim3(kThreads), 0, s, g, A.rowptr.p, A.colidx.p, A.val.p, N.rowptr.p,
                       N.colidx.p, N.val.p);
    hipLaunchKernelGGL(amgs_galerkin_stencil_sym_kernel<BS>, grid, dim3(kThreads), 0, s, cd[0], cd[1], cd[2], N.val.p);
}
void amgs_galerkin_stencil(const AmgGrid &a, const CsrDev &A, CsrDev &N, hipStream_t s)
{
    const gs::GsGrid g = gs::gs_grid(a.fd, a.cd);
    if ((gs::gs_items(a.cd, a.bs) + kThreads - 1) / kThreads > INT32_MAX)
        fail(SPK_ERR_UNSUPPORTED, "amg: the stencil products of a %d x %d x %d grid need more workgroups than a launch takes", (int)a.cd[0],
             (int)a.cd[1], (int)a.cd[2]);
    if (a.bs == 1) galerkin_stencil_launch<1>(g, A, N, s);
    else if (a.bs == 2) galerkin_stencil_launch<2>(g, A, N, s);
    else if (a.bs == 3) galerkin_stencil_launch<3>(g, A, N, s);
    else fail(SPK_ERR_ARG, "amg: the stencil products take node sizes 1, 2 and 3, not %d", (int)a.bs);
    SPK_HIP(hipGetLastError());
}
void amgs_galerkin_stencil_check(const AmgGrid &a, const CsrDev &A, unsigned long long *bad, hipStream_t s)
{
    hipLaunchKernelGGL(amgs_galerkin_stencil_check_kernel, row_grid(A.nrows), dim3(kThreads), 0, s, a.fd[0], a.fd[1], a.fd[2], (int)a.bs,
                       A.rowptr.p, A.colidx.p, bad);
}
void amgs_rows_sorted(const int32_t *rp, const int32_t *ci, int32_t n, int32_t *flag, hipStream_t s)
{
    if (n > 0) hipLaunchKernelGGL(amgs_rows_sorted_kernel, row_grid(n), dim3(kThreads), 0, s, rp, ci, n, flag);
}
void amgs_sort_rows(const int32_t *rp, int32_t *ci, double *v, int32_t n, hipStream_t s)
{
    if (n > 0) hipLaunchKernelGGL(amgs_sort_rows_kernel, row_grid(n), dim3(kThreads), 0, s, rp, ci, v, n);
}
void amgs_node_norms(const int32_t *rp, const int32_t *ci, const double *v, int32_t nn, int bs, double *dn, hipStream_t s)
{
    if (nn > 0) hipLaunchKernelGGL(amgs_node_norms_kernel, row_grid(nn), dim3(kThreads), 0, s, rp, ci, v, nn, bs, dn);
}
void amgs_graph(const int32_t *rp, const int32_t *ci, const double *v, int32_t nn, int bs, double theta, const double *dn,
                const int32_t *gp, int32_t *out, hipStream_t s)
{
    if (nn <= 0) return;
    if (gp) hipLaunchKernelGGL(amgs_graph_kernel<true>, row_grid(nn), dim3(kThreads), 0, s, rp, ci, v, nn, bs, theta, dn, gp, out);
    else hipLaunchKernelGGL(amgs_graph_kernel<false>, row_grid(nn), dim3(kThreads), 0, s, rp, ci, v, nn, bs, theta, dn, gp, out);
}
void amgs_tent_count(const int32_t *agg, int32_t nrows, int bs, int32_t *cnt, hipStream_t s)
{
    if (nrows > 0) hipLaunchKernelGGL(amgs_tent_count_kernel, row_grid(nrows), dim3(kThreads), 0, s, agg, nrows, bs, cnt);
}
void amgs_tent_fill(const int32_t *agg, const double *inv, int32_t nrows, int bs, const int32_t *rp, int32_t *ci, double *v,
                    hipStream_t s)
{
    if (nrows > 0) hipLaunchKernelGGL(amgs_tent_fill_kernel, row_grid(nrows), dim3(kThreads), 0, s, agg, inv, nrows, bs, rp, ci, v);
}
void amgs_grid_prolongator(const AmgGrid &g, int32_t *rp, int32_t *ci, double *v, hipStream_t s)
{
    hipLaunchKernelGGL(amgs_grid_prolongator_kernel, row_grid((int64_t)g.fd[0] * g.fd[1] * g.fd[2] * g.bs), dim3(kThreads), 0, s,
                       g.fd[0], g.fd[1], g.fd[2], g.cd[0], g.cd[1], g.cd[2], (int)g.bs, rp, ci, v);
}
void amgs_spgemm_bound(const CsrDev &A, const CsrDev &B, int32_t *bound, unsigned long long *total, hipStream_t s)
{
    if (A.nrows > 0)
        hipLaunchKernelGGL(amgs_spgemm_bound_kernel, row_grid(A.nrows), dim3(kThreads), 0, s, A.rowptr.p, A.colidx.p, B.rowptr.p,
                           A.nrows, B.ncols, bound, total);
}
void amgs_spgemm_expand(const CsrDev &A, const CsrDev &B, const int32_t *off, int32_t *sc, double *sv, int32_t *cnt, hipStream_t s)
{
    if (A.nrows > 0)
        hipLaunchKernelGGL(amgs_spgemm_expand_kernel, row_grid(A.nrows), dim3(kThreads), 0, s, A.rowptr.p, A.colidx.p, A.val.p,
                           B.rowptr.p, B.colidx.p, B.val.p, A.nrows, off, sc, sv, cnt);
}
void amgs_compact(int32_t n, const int32_t *off, const int32_t *rp, const int32_t *sc, const double *sv, int32_t *ci, double *v,
                  hipStream_t s)
{
    if (n > 0) hipLaunchKernelGGL(amgs_compact_kernel, row_grid(n), dim3(kThreads), 0, s, n, off, rp, sc, sv, ci, v);
}
void amgs_add(double a, const CsrDev &A, double b, const CsrDev &B, const double *scale, const int32_t *crp, int32_t *cci,
              double *cv, int32_t *cnt, hipStream_t s)
{
    const int32_t n = A.nrows;
    if (n <= 0) return;
    if (crp)
        hipLaunchKernelGGL(amgs_add_kernel<true>, row_grid(n), dim3(kThreads), 0, s, n, a, A.rowptr.p, A.colidx.p, A.val.p, b,
                           B.rowptr.p, B.colidx.p, B.val.p, scale, crp, cci, cv, cnt);
    else
        hipLaunchKernelGGL(amgs_add_kernel<false>, row_grid(n), dim3(kThreads), 0, s, n, a, A.rowptr.p, A.colidx.p, A.val.p, b,
                           B.rowptr.p, B.colidx.p, B.val.p, scale, crp, cci, cv, cnt);
}
void amgs_col_count(const int32_t *ci, int64_t nnz, int32_t *cnt, hipStream_t s)
{
    if (nnz > 0) hipLaunchKernelGGL(amgs_col_count_kernel, row_grid(nnz), dim3(kThreads), 0, s, ci, nnz, cnt);
}
void amgs_transpose_fill(const CsrDev &A, int32_t *pos, int32_t *tci, double *tv, hipStream_t s)
{
    if (A.nrows > 0)
        hipLaunchKernelGGL(amgs_transpose_fill_kernel, row_grid(A.nrows), dim3(kThreads), 0, s, A.rowptr.p, A.colidx.p, A.val.p,
                           A.nrows, pos, tci, tv);
}
void amgs_pattern_equal(const int32_t *a, const int32_t *b, int64_t n, int32_t *flag, hipStream_t s)
{
    if (n > 0) hipLaunchKernelGGL(amgs_pattern_equal_kernel, row_grid(n), dim3(kThreads), 0, s, a, b, n, flag);
}
void amgs_spgemm_numeric(const CsrDev &A, const CsrDev &B, CsrDev &C, int32_t *err, hipStream_t s)
{
    if (A.nrows > 0)
        hipLaunchKernelGGL(amgs_spgemm_numeric_kernel, row_grid(A.nrows), dim3(kThreads), 0, s, A.rowptr.p, A.colidx.p, A.val.p,
                           B.rowptr.p, B.colidx.p, B.val.p, A.nrows, B.nrows, C.rowptr.p, C.colidx.p, C.val.p, err);
}
void amgs_symmetrise_numeric(const CsrDev &Ac, CsrDev &N, int32_t *err, hipStream_t s)
{
    if (N.nrows > 0)
        hipLaunchKernelGGL(amgs_symmetrise_numeric_kernel, row_grid(N.nrows), dim3(kThreads), 0, s, Ac.rowptr.p, Ac.colidx.p, Ac.val.p,
                           N.nrows, N.rowptr.p, N.colidx.p, N.val.p, err);
}
void amgs_lz_init(int64_t n, const double *dinv, double dscale, double *sv, double *q, const Finish &f, hipStream_t s)
{
    hipLaunchKernelGGL(amgs_lz_init_kernel, dim3(lz_grid(n)), dim3(kVT), 0, s, n, dinv, dscale, sv, q, f.partials, f.out,
                       FinErr{f.err, f.fin_ticks});
}
void amgs_abs_sum(int64_t n, const double *x, const Finish &f, hipStream_t s)
{
    hipLaunchKernelGGL(amgs_abs_sum_kernel, dim3(lz_grid(n)), dim3(kVT), 0, s, n, x, f.partials, f.out, FinErr{f.err, f.fin_ticks});
}
void amgs_lz_scale(int64_t n, double nb, const double *w, const double *sv, double *q, double *t, hipStream_t s)
{
    hipLaunchKernelGGL(amgs_lz_scale_kernel, dim3(lz_grid(n)), dim3(kVT), 0, s, n, nb, w, sv, q, t);
}
void amgs_lz_dot(int64_t n, const double *sv, const double *aw, double ascale, double *w, const double *q, const Finish &f, hipStream_t s)
{
    hipLaunchKernelGGL(amgs_lz_dot_kernel, dim3(lz_grid(n)), dim3(kVT), 0, s, n, sv, aw, ascale, w, q, f.partials, f.out,
                       FinErr{f.err, f.fin_ticks});
}
void amgs_lz_init_resident(int64_t n, const double *dinv, double dscale, double *sv, double *q, const Finish &f,
                           lanczos_core::LzState *st, hipStream_t s)
{
    hipLaunchKernelGGL(amgs_lz_init_resident_kernel, dim3(lz_grid(n)), dim3(kVT), 0, s, n, dinv, dscale, sv, q, f.partials, st,
                       FinErr{f.err, f.fin_ticks});
}
void amgs_lz_scale_resident(int64_t n, int jb, const double *w, const double *sv, double *q, double *t, const lanczos_core::LzState *st,
                            hipStream_t s)
{
    hipLaunchKernelGGL(amgs_lz_scale_resident_kernel, dim3(lz_grid(n)), dim3(kVT), 0, s, n, jb, w, sv, q, t, st);
}
void amgs_lz_dot_resident(int64_t n, int j, const double *sv, const double *aw, double ascale, double *w, const double *q,
                          const Finish &f, lanczos_core::LzState *st, hipStream_t s)
{
    hipLaunchKernelGGL(amgs_lz_dot_resident_kernel, dim3(lz_grid(n)), dim3(kVT), 0, s, n, j, sv, aw, ascale, w, q, f.partials, st,
                       FinErr{f.err, f.fin_ticks});
}
void amgs_lz_update_resident(int64_t n, int j, int kk, const double *q, const double *qp, double *w, const Finish &f,
                             lanczos_core::LzState *st, hipStream_t s)
{
    hipLaunchKernelGGL(amgs_lz_update_resident_kernel, dim3(lz_grid(n)), dim3(kVT), 0, s, n, j, kk, q, qp, w, f.partials, st,
                       FinErr{f.err, f.fin_ticks});
}
void amgs_lz_update(int64_t n, double a, double be, const double *q, const double *qp, double *w, const Finish &f, hipStream_t s)
{
    hipLaunchKernelGGL(amgs_lz_update_kernel, dim3(lz_grid(n)), dim3(kVT), 0, s, n, a, be, q, qp, w, f.partials, f.out,
                       FinErr{f.err, f.fin_ticks});
}

}  // namespace k
}  // namespace spk
