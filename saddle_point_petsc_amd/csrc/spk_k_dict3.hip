// spk_k_dict3.hip -- the product and the FP32 Richardson sweep on ROW TYPES + DEVIATION CODES for 3x3 blocks whose row
// types hold at most 27 blocks (the 27-point stencil of a Q1 hexahedral grid: BASELINE config 5) and whose classes share
// one field layout (DictDev::uniform3), software-pipelined.  gfx950, wave64.
//
// The plain kernels (spk_k_dict.hip) issue the loads of a few blocks, wait, decode, and turn to the next few: a chain of
// memory round trips per block row (nine with three blocks in flight: 264 us per product on the 256 x 256 x 32 slab,
// three with nine: 232 us -- 0.97 GB, so 0.46 / 0.52 of the 8 TB/s peak).  Here a block row is three GROUPS of nine
// blocks and the groups of a workgroup's chunks form one sequence: the loads of group q+1 -- nine 16-byte code words
// per lane, the gathers of x, the row's y -- are in flight while group q is decoded, in two register stages.  As in
// spmv_dict2_kernel there is no branch around a load (the compiler's wait counts stay exact): a position beyond a row's
// length reads through the range check of a buffer descriptor (zeros) with the NULL class (decodes to +0), a group beyond
// the workgroup's range re-reads the last block row and is not computed.
//
// Parity: blocks in the block row's CSR order, every product rounded on its own (contraction off), added in that order
// from +0 -- the sums of the plain kernel, the blocked kernel, the CSR kernel and the oracle, bit for bit
// (tests/test_gpu_dict.py::test_dictionary_3d_grid, tests/test_gpu_configs.py).
#include "spk_dict.hpp"

#include <cstring>

namespace spk {
namespace k {

constexpr int kD3G = 9;        // blocks per group
constexpr int kD3Groups = 3;   // groups per block row (27 positions)

// The two register stages over the groups of a workgroup's chunks [c0, c1) (group q: chunk c0 + q / 3, positions 9 (q % 3) ...):
// issue(t, brr, g, S) requests group g of block row brr, whose row type is t, into S; compute(q, S) takes group q from S.
// tA: the row type of the first block row (requested by the caller before the tables are copied); the row type a group
// needs is requested one group ahead (two registers, alternating with the stages)
template <class Stage, class Issue, class Compute>
__device__ __forceinline__ void dict3_two_stage(const DictArgs &d, int c0, int c1, int tA, Issue issue, Compute compute)
{
    const int nq = (c1 - c0) * kD3Groups;
    auto rowq = [&](int q) { return dict_rowof(d, c0 + q / kD3Groups); };
    int tB = tA;
    Stage SA, SB;
    issue(tA, rowq(0), 0, SA);
    for (int q = 0;; q += 2) {
        tA = (int)d.tid[rowq(q + 2)];
        issue(tB, rowq(q + 1), (q + 1) % kD3Groups, SB);
        compute(q, SA);
        if (q + 1 >= nq) break;
        tB = (int)d.tid[rowq(q + 3)];
        issue(tA, rowq(q + 2), (q + 2) % kD3Groups, SA);
        compute(q + 1, SB);
        if (q + 2 >= nq) break;
    }
}

template <bool ACC>
struct Dict3Stage {
    u64 w0[kD3G], w1[kD3G];
    double x0[kD3G], x1[kD3G], x2[kD3G];
    int cls[kD3G];
    double y0, y1, y2;
};

// loads of group q (chunk q / 3, positions 9 (q % 3) ...): all of them unconditional
template <bool ACC>
__device__ __forceinline__ void dict3_issue(const DictArgs &d, __amdgpu_buffer_rsrc_t xr, const double *__restrict__ y,
                                            const int2 *tent, int tc, int brr, int g, Dict3Stage<ACC> &S)
{
    const int k0 = kD3G * g;
#pragma unroll
    for (int j = 0; j < kD3G; ++j) {
        const int4v r = __builtin_nontemporal_load(reinterpret_cast<const int4v *>(d.codes + d.plane_off[k0 + j]) + brr);
        S.w0[j] = (u64)(uint32_t)r.x | ((u64)(uint32_t)r.y << 32);
        S.w1[j] = (u64)(uint32_t)r.z | ((u64)(uint32_t)r.w << 32);
    }
    if (ACC) {
        S.y0 = y[3 * (int64_t)brr];
        S.y1 = y[3 * (int64_t)brr + 1];
        S.y2 = y[3 * (int64_t)brr + 2];
    }
    const int2 *te = tent + (size_t)tc * 27 + k0;
    const uint32_t b24 = (uint32_t)brr * 24u;
#pragma unroll
    for (int j = 0; j < kD3G; ++j) {
        const int2 e = te[j];
        S.cls[j] = e.y;
        const uint32_t off = b24 + (uint32_t)e.x;
        const int4v a = __builtin_bit_cast(int4v, __builtin_amdgcn_raw_buffer_load_b128(xr, (int)off, 0, 0));
        const int2v b = __builtin_bit_cast(int2v, __builtin_amdgcn_raw_buffer_load_b64(xr, (int)(off + 16u), 0, 0));
        S.x0[j] = __hiloint2double(a.y, a.x);
        S.x1[j] = __hiloint2double(a.w, a.z);
        S.x2[j] = __hiloint2double(b.y, b.x);
    }
}

template <bool ACC, bool RIDE, bool BT, int U3>
__global__ __launch_bounds__(kThreads) void spmv_dict3_kernel(DictArgs d, const double *__restrict__ x, double *__restrict__ y,
                                                              RowTail tail, const int32_t *__restrict__ done, GivensRider gr)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int bx = product_prologue<RIDE>(done, gr, reinterpret_cast<double *>(smem));
    int c0, c1;
    if (bx < 0 || !dict_chunk_range(d, bx, c0, c1)) return;
    const int tA = (int)d.tid[dict_rowof(d, c0)];
    dict_load_lds(d, (d.nclass + 1) * 9, smem);
    const DictTables T = dict_tables(d, smem);
    dict_prepare_types<27>(d, T, 24);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(x), 0, 24 * d.nbrows, 0x00020000);

    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    auto issue = [&](int tc, int brr, int g, Dict3Stage<ACC> &S) { dict3_issue<ACC>(d, xr, y, T.tent, tc, brr, g, S); };
    auto compute = [&](int q, const Dict3Stage<ACC> &S) {
        const int g = q % kD3Groups;
        if (g == 0) s0 = s1 = s2 = 0.0;
#pragma unroll
        for (int j = 0; j < kD3G; ++j) {
            const double2 *cb = T.cv + (size_t)S.cls[j] * 9;
            s0 += dict_decode(dict_field3u<U3>(S.w0[j], S.w1[j], d, 0), cb[0]) * S.x0[j];
            s0 += dict_decode(dict_field3u<U3>(S.w0[j], S.w1[j], d, 1), cb[1]) * S.x1[j];
            s0 += dict_decode(dict_field3u<U3>(S.w0[j], S.w1[j], d, 2), cb[2]) * S.x2[j];
            s1 += dict_decode(dict_field3u<U3>(S.w0[j], S.w1[j], d, 3), cb[3]) * S.x0[j];
            s1 += dict_decode(dict_field3u<U3>(S.w0[j], S.w1[j], d, 4), cb[4]) * S.x1[j];
            s1 += dict_decode(dict_field3u<U3>(S.w0[j], S.w1[j], d, 5), cb[5]) * S.x2[j];
            s2 += dict_decode(dict_field3u<U3>(S.w0[j], S.w1[j], d, 6), cb[6]) * S.x0[j];
            s2 += dict_decode(dict_field3u<U3>(S.w0[j], S.w1[j], d, 7), cb[7]) * S.x1[j];
            s2 += dict_decode(dict_field3u<U3>(S.w0[j], S.w1[j], d, 8), cb[8]) * S.x2[j];
        }
        if (g != kD3Groups - 1) return;
        const int brc = (c0 + q / kD3Groups) * kDictChunk + (int)threadIdx.x;
        if (brc >= d.nbrows) return;
        double s[3] = {s0, s1, s2};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int64_t row = 3 * (int64_t)brc + r;
            row_tail_add(tail, row, s[r], BT);
            if (ACC) s[r] += r == 0 ? S.y0 : r == 1 ? S.y1 : S.y2;
            y[row] = s[r];
        }
    };
    dict3_two_stage<Dict3Stage<ACC>>(d, c0, c1, tA, issue, compute);
}

bool dict3_pipelined(const DictDev &A)
{
    // SPK_DICT3_PIPELINE=0 / 1: never / at any size (tests run both forms on small grids); read at every call
    const char *env = getenv("SPK_DICT3_PIPELINE");
    const bool off = env && !strcmp(env, "0"), force = env && !strcmp(env, "1");
    // (from a million block rows: eight chunks and more per workgroup to pipeline over; measured on 96^3 = 0.88 M block
    // rows: 108 us plain with nine blocks in flight, 125 us pipelined; on the 256 x 256 x 32 slab 232 against 222)
    return !off && A.bs == 3 && A.uniform3 >= 1 && A.uniform3 <= 3 && A.kmax == 27 && (force || A.nbrows >= (1 << 20)) &&
           (int64_t)A.nbrows * 24 < (1ll << 31);
}

static DictArgs dict3_args(const DictDev &A, int *grid)
{
    DictArgs d = dict_args(A, grid);
    // workgroups of a large launch: two per CU, all co-resident, each pipelines its chunks
    static const int wgs = [] { const char *e = getenv("SPK_DICT3_WGS"); return e && atoi(e) > 0 ? atoi(e) : 512; }();   // (developer knob)
    d.chunks_per_wg = std::max(1, d.nchunks / wgs);
    const int cpx = (d.nchunks + 7) / 8;
    d.chunks_per_xcd = (cpx + d.chunks_per_wg - 1) / d.chunks_per_wg * d.chunks_per_wg;
    *grid = 8 * (d.chunks_per_xcd / d.chunks_per_wg);
    return d;
}

bool spmv_dict3(const DictDev &A, const double *x, double *y, const CsrDev *bt, const double *lam, const int32_t *done,
                hipStream_t s, bool accumulate, const OffDiag *odp, const GivensRider *rider)
{
    if (!dict3_pipelined(A) || A.nbrows == 0) return false;
    int grid = 0;
    const DictArgs d = dict3_args(A, &grid);
    const ProductLaunch p = make_product_launch(bt, lam, odp, rider, done, accumulate);
    const size_t lds = std::max((size_t)A.lds_bytes, p.rider_lds);
    dispatch_product(p.acc, p.ride, p.bt, [&](auto acc, auto ride, auto btf) {
        constexpr bool ACC = acc.value, RIDE = ride.value, BTF = btf.value;
        auto launch = [&](auto kern) {
            SPK_LAUNCH_PRODUCT(kern, dim3(grid + p.nride), dim3(kThreads), lds, s, d, x, y, p.tail, p.done, p.gr);
        };
        if (A.uniform3 == 1) launch(spmv_dict3_kernel<ACC, RIDE, BTF, 1>);
        else if (A.uniform3 == 2) launch(spmv_dict3_kernel<ACC, RIDE, BTF, 2>);
        else launch(spmv_dict3_kernel<ACC, RIDE, BTF, 3>);
    });
    return true;
}

// ---------------------------------------------------------------------------
// FP32 damped-Jacobi Richardson sweep (jacobi_sweep_f32_dict_kernel, spk_k_dict.hip), pipelined the same way: the value is
// decoded exactly, rounded to single precision, products rounded once each, summed per row in block order.
// ---------------------------------------------------------------------------
struct Dict3StageF {
    u64 w0[kD3G], w1[kD3G];
    float x0[kD3G], x1[kD3G], x2[kD3G];
    int cls[kD3G];
};

__device__ __forceinline__ void dict3_issue_f(const DictArgs &d, __amdgpu_buffer_rsrc_t yr, const int2 *tent, int tc, int brr, int g,
                                              Dict3StageF &S)
{
    const int k0 = kD3G * g;
#pragma unroll
    for (int j = 0; j < kD3G; ++j) {
        const int4v r = __builtin_nontemporal_load(reinterpret_cast<const int4v *>(d.codes + d.plane_off[k0 + j]) + brr);
        S.w0[j] = (u64)(uint32_t)r.x | ((u64)(uint32_t)r.y << 32);
        S.w1[j] = (u64)(uint32_t)r.z | ((u64)(uint32_t)r.w << 32);
    }
    const int2 *te = tent + (size_t)tc * 27 + k0;
    const uint32_t b12 = (uint32_t)brr * 12u;
#pragma unroll
    for (int j = 0; j < kD3G; ++j) {
        const int2 e = te[j];
        S.cls[j] = e.y;
        const uint32_t off = b12 + (uint32_t)e.x;
        const int2v a = __builtin_bit_cast(int2v, __builtin_amdgcn_raw_buffer_load_b64(yr, (int)off, 0, 0));
        const int b = __builtin_bit_cast(int, __builtin_amdgcn_raw_buffer_load_b32(yr, (int)(off + 8u), 0, 0));
        S.x0[j] = __int_as_float(a.x);
        S.x1[j] = __int_as_float(a.y);
        S.x2[j] = __int_as_float(b);
    }
}

template <int U3>
__global__ __launch_bounds__(kThreads) void jacobi_sweep_f32_dict3_kernel(DictArgs d, const float *__restrict__ d32, float omega,
                                                                          const float *__restrict__ x32,
                                                                          const float *__restrict__ yin, float *__restrict__ yout,
                                                                          const int32_t *__restrict__ done)
{
#pragma clang fp contract(off)
    if (done && *done) return;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int c0, c1;
    if (!dict_chunk_range(d, (int)blockIdx.x, c0, c1)) return;
    const int tA = (int)d.tid[dict_rowof(d, c0)];
    dict_load_lds(d, (d.nclass + 1) * 9, smem);
    const DictTables T = dict_tables(d, smem);
    dict_prepare_types<27>(d, T, 12);
    const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(yin), 0, 12 * d.nbrows, 0x00020000);

    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    auto issue = [&](int tc, int brr, int g, Dict3StageF &S) { dict3_issue_f(d, yr, T.tent, tc, brr, g, S); };
    auto compute = [&](int q, const Dict3StageF &S) {
        const int g = q % kD3Groups;
        if (g == 0) s0 = s1 = s2 = 0.0f;
#pragma unroll
        for (int j = 0; j < kD3G; ++j) {
            const double2 *cb = T.cv + (size_t)S.cls[j] * 9;
            s0 = s0 + (float)dict_decode(dict_field3u<U3>(S.w0[j], S.w1[j], d, 0), cb[0]) * S.x0[j];
            s0 = s0 + (float)dict_decode(dict_field3u<U3>(S.w0[j], S.w1[j], d, 1), cb[1]) * S.x1[j];
            s0 = s0 + (float)dict_decode(dict_field3u<U3>(S.w0[j], S.w1[j], d, 2), cb[2]) * S.x2[j];
            s1 = s1 + (float)dict_decode(dict_field3u<U3>(S.w0[j], S.w1[j], d, 3), cb[3]) * S.x0[j];
            s1 = s1 + (float)dict_decode(dict_field3u<U3>(S.w0[j], S.w1[j], d, 4), cb[4]) * S.x1[j];
            s1 = s1 + (float)dict_decode(dict_field3u<U3>(S.w0[j], S.w1[j], d, 5), cb[5]) * S.x2[j];
            s2 = s2 + (float)dict_decode(dict_field3u<U3>(S.w0[j], S.w1[j], d, 6), cb[6]) * S.x0[j];
            s2 = s2 + (float)dict_decode(dict_field3u<U3>(S.w0[j], S.w1[j], d, 7), cb[7]) * S.x1[j];
            s2 = s2 + (float)dict_decode(dict_field3u<U3>(S.w0[j], S.w1[j], d, 8), cb[8]) * S.x2[j];
        }
        if (g != kD3Groups - 1) return;
        const int brc = (c0 + q / kD3Groups) * kDictChunk + (int)threadIdx.x;
        if (brc >= d.nbrows) return;
        const float s[3] = {s0, s1, s2};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int64_t row = 3 * (int64_t)brc + r;
            yout[row] = sweep_update(yin[row], omega, d32[row], x32[row], s[r]);
        }
    };
    dict3_two_stage<Dict3StageF>(d, c0, c1, tA, issue, compute);
}

bool jacobi_sweep_f32_dict3(const DictDev &A, const float *d32, float omega, const float *x32, const float *yin, float *yout,
                            const int32_t *done, hipStream_t s)
{
    if (!dict3_pipelined(A) || A.nbrows == 0 || (int64_t)A.nbrows * 12 >= (1ll << 31)) return false;
    int grid = 0;
    const DictArgs d = dict3_args(A, &grid);
    if (A.uniform3 == 1)
        hipLaunchKernelGGL((jacobi_sweep_f32_dict3_kernel<1>), dim3(grid), dim3(kThreads), (size_t)A.lds_bytes, s, d, d32, omega, x32, yin, yout, done);
    else if (A.uniform3 == 2)
        hipLaunchKernelGGL((jacobi_sweep_f32_dict3_kernel<2>), dim3(grid), dim3(kThreads), (size_t)A.lds_bytes, s, d, d32, omega, x32, yin, yout, done);
    else
        hipLaunchKernelGGL((jacobi_sweep_f32_dict3_kernel<3>), dim3(grid), dim3(kThreads), (size_t)A.lds_bytes, s, d, d32, omega, x32, yin, yout, done);
    return true;
}

}  // namespace k
}  // namespace spk
