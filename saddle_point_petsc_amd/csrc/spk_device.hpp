// spk_device.hpp -- device-side helpers shared by the kernel files (spk_k_*.hip): workgroup reductions, the
// sentinel-based cross-workgroup finish, the peer-store granule protocol, the Givens step and its rider, launch shapes.
// Device code only: include from .hip files.
#pragma once
#include "spk_internal.hpp"
#include "spk_gs_stamps.hpp"

#include <cmath>
#include <cstdlib>
#include <type_traits>

namespace spk {
namespace k {

constexpr int kThreads = 256;
constexpr int kWave = 64;
// Reducing vector kernels on big vectors run fat workgroups on a grid of <= 256 (kVecMaxBlocks in spk_gs_launch.hpp,
// one per CU): the reducer reads one partial row per workgroup, so few fat workgroups beat many thin ones.
constexpr int kVT = 1024;
constexpr int kVWaves = kVT / kWave;
constexpr int kVecUnroll = 4;    // double2 per thread per vector tile

// ---------------------------------------------------------------------------
// reductions inside a workgroup
// ---------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;
}

// N wave sums together, without the LDS permutes of __shfl_down (12 per value above: with N = 41 the chains of a
// workgroup's eight waves queue ~4 000 of them on one LDS pipe behind the last byte of a reducing pass).  For every
// value the tree is the one lane 0 of wave_sum's chain produces: lanes 32 apart are added first, then 16, 8, 4, 2, 1.
// At each level a lane keeps one value of a pair and hands the other one to its partner, so level k works on N / 2^k
// values: ~N exchange-and-adds instead of 6 N.  Which lane of a pair holds a sum does not matter to its bits (IEEE
// addition commutes; no NaN payloads are involved).  The moves are v_permlane32_swap / v_permlane16_swap (gfx950) and
// DPP; xor 4 inside a row is quad_perm [3,2,1,0] followed by row_half_mirror.
// On return lane l holds the sum of value wave_sum_owner(l) in v[0], where that is below N.
__device__ __forceinline__ int wave_sum_owner(int lane) { return (int)(__brev((unsigned)lane) >> 26); }
template <int CTRL>
__device__ __forceinline__ double dpp_move(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// SW = 32: the upper half-wave of a trades places with the lower half-wave of b; 16: odd rows of a, even rows of b
template <int SW>
__device__ __forceinline__ void lane_swap(double &a, double &b)
{
    const unsigned alo = (unsigned)__double2loint(a), ahi = (unsigned)__double2hiint(a);
    const unsigned blo = (unsigned)__double2loint(b), bhi = (unsigned)__double2hiint(b);
    const auto l = SW == 32 ? __builtin_amdgcn_permlane32_swap(alo, blo, false, false) : __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
    const auto h = SW == 32 ? __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false) : __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
    a = __hiloint2double((int)h[0], (int)l[0]);
    b = __hiloint2double((int)h[1], (int)l[1]);
}
template <int OFF, int N>
__device__ __forceinline__ void wave_sum_level(double (&v)[N], int n, int lane)   // n values in, (n + 1) / 2 out
{
#pragma unroll
    for (int j = 0; j < (N + 1) / 2; ++j) {
        if (2 * j < n) {   // compile-time once unrolled
            double a = v[2 * j], b = v[2 * j + 1 < n ? 2 * j + 1 : 2 * j];   // an odd one out pairs with itself
            if (OFF >= 16) {
                lane_swap<OFF>(a, b);   // lower lanes: a and the partner's a; upper lanes: the partner's b and b
                v[j] = a + b;
            } else {
                const bool up = lane & OFF;
                const double mine = up ? b : a, give = up ? a : b;
                double got;
                if (OFF == 8) got = dpp_move<0x128>(give);                        // row_ror:8
                else if (OFF == 4) got = dpp_move<0x141>(dpp_move<0x1b>(give));   // quad_perm:[3,2,1,0], row_half_mirror
                else if (OFF == 2) got = dpp_move<0x4e>(give);                    // quad_perm:[2,3,0,1]
                else got = dpp_move<0xb1>(give);                                  // quad_perm:[1,0,3,2]
                v[j] = mine + got;
            }
        }
    }
}
template <int N>
__device__ __forceinline__ void wave_sum_multi(double (&v)[N])
{
    static_assert(N >= 1 && N <= 64, "one value per lane at the end");
    const int lane = threadIdx.x & 63;
    constexpr int n1 = (N + 1) / 2, n2 = (n1 + 1) / 2, n3 = (n2 + 1) / 2, n4 = (n3 + 1) / 2, n5 = (n4 + 1) / 2;
    wave_sum_level<32>(v, N, lane);
    wave_sum_level<16>(v, n1, lane);
    wave_sum_level<8>(v, n2, lane);
    wave_sum_level<4>(v, n3, lane);
    wave_sum_level<2>(v, n4, lane);
    wave_sum_level<1>(v, n5, lane);
}

// streamed-once operands: non-temporal 16-byte loads (global_load_dwordx4 ... nt);
// measured +9 % on the Krylov basis streams (5.25 -> 5.7 TB/s)
typedef double dbl2v __attribute__((ext_vector_type(2)));
typedef int int4v __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ double2 ld2s(const double *p, int64_t i2)
{
    if (NT) {
        const dbl2v v = __builtin_nontemporal_load(reinterpret_cast<const dbl2v *>(p) + i2);
        double2 r;
        r.x = v.x;
        r.y = v.y;
        return r;
    }
    return reinterpret_cast<const double2 *>(p)[i2];
}
__device__ __forceinline__ void st2nt(double *p, int64_t i2, double2 v)   // non-temporal 16-byte store
{
    dbl2v t;
    t.x = v.x;
    t.y = v.y;
    __builtin_nontemporal_store(t, reinterpret_cast<dbl2v *>(p) + i2);
}
// an FP32 Krylov basis (-spk_basis_precision single): two floats where the FP64 kernels read a double2
typedef float flt2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float2 ldf2s(const float *p, int64_t i2)   // streamed once: non-temporal 8-byte load
{
    const flt2v v = __builtin_nontemporal_load(reinterpret_cast<const flt2v *>(p) + i2);
    float2 r;
    r.x = v.x;
    r.y = v.y;
    return r;
}
__device__ __forceinline__ void stf2nt(float *p, int64_t i2, float2 v)   // non-temporal 8-byte store
{
    flt2v t;
    t.x = v.x;
    t.y = v.y;
    __builtin_nontemporal_store(t, reinterpret_cast<flt2v *>(p) + i2);
}
// How kernel B reads the basis it is instantiated for: pair i2 and entry i of vector `vec` (V as IterB carries it)
template <class BT>
struct BasisElem {
    using E2 = double2;
    static __device__ __forceinline__ E2 ld(const double *V, size_t vec, int64_t ldv, int64_t i2) { return ld2s<true>(V + vec * ldv, i2); }
    static __device__ __forceinline__ double at(const double *V, size_t vec, int64_t ldv, int64_t i) { return V[vec * ldv + i]; }
};
template <>
struct BasisElem<float> {
    using E2 = float2;
    static __device__ __forceinline__ E2 ld(const double *V, size_t vec, int64_t ldv, int64_t i2)
    {
        return ldf2s(reinterpret_cast<const float *>(V) + vec * ldv, i2);
    }
    static __device__ __forceinline__ double at(const double *V, size_t vec, int64_t ldv, int64_t i)
    {
        return (double)reinterpret_cast<const float *>(V)[vec * ldv + i];
    }
};
template <bool NT>
__device__ __forceinline__ int4 ld4i(const int32_t *p)
{
    if (NT) {
        const int4v v = __builtin_nontemporal_load(reinterpret_cast<const int4v *>(p));
        int4 r;
        r.x = v.x; r.y = v.y; r.z = v.z; r.w = v.w;
        return r;
    }
    return *reinterpret_cast<const int4 *>(p);
}

// ---------------------------------------------------------------------------
// Cross-workgroup finish without a second launch, without fences and without
// counters.  Every slot of the partials buffer rests at a SENTINEL (a NaN bit
// pattern no arithmetic produces).  Every workgroup PUBLISHES its k partial
// sums with sc1 (write-through) 8-byte stores and is done -- no drain, no
// arrival.  The workgroup with the highest block index (dispatched last) is the
// reducer: it reads all partials with sc1 loads, spinning on any slot that still
// holds the sentinel, puts the sentinel back, and sums in a FIXED order (bitwise
// reproducible, no float atomics).  A value is its own arrival flag, so the chain
// after the last producer is one store flight + one load round trip, where
// "drain -> atomic arrival -> re-read" (cdna_hip_programming.md Guideline 16, R1)
// was three to four dependent round trips: measured on a 262 k-row vector, MAXPY +
// norm 7.3 -> 5.8 us, MDOT 7.8 -> 6.4 us (3.4 us for the MAXPY stream without any reduction).
// The reducer asks for kFinBatch partials per thread at a time and simply asks again while any
// of them is still armed; a per-slot re-poll, or 32 at a time, doubled the VGPRs of the WHOLE
// kernel (75 -> 149..256) and cost more occupancy in the streaming part than the finish gained.
// The sentinel is restored inside the kernel that consumed it, so the next launch
// on the stream (ordered by the kernel boundary) finds every slot armed.
// Every spin is bounded; a slot that never arrives reads as NaN
// (-> KSP_DIVERGED_NANORINF), it cannot hang the kernel.
// ---------------------------------------------------------------------------
constexpr unsigned long long kSentinelBits = 0xFFF8DEADBEEF5A5Aull;
__device__ __forceinline__ void publish(double *p, double v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double peek(const double *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool is_sentinel(double v)
{
    return (unsigned long long)__double_as_longlong(v) == kSentinelBits;
}

// true in every thread of the reducing workgroup (the last block of the grid)
__device__ __forceinline__ bool arrive_last(unsigned nblocks)
{
    if (blockIdx.x != nblocks - 1) return false;
    __syncthreads();  // the caller's LDS staging is reused as scratch below
    return true;
}

// reducer (blockDim.x = T threads, power of two): scratch[i] = sum_b partials[b*ld + i], i < k <= 64.
// Strided slices (a thread's loads are all requested before its first add: one memory round trip
// when everything has arrived), then a fixed binary tree; the result is valid in LDS scratch[0..k)
// after return.  scratch: T doubles.
constexpr int kFinBatch = 16;  // partials a reducer thread requests together (registers of the WHOLE kernel: 32 cost 2x the VGPRs)
// (FinErr -- where a reducer reports a partial that never arrived -- is declared in spk_internal.hpp)
// FB: partials a reducer thread requests together (kFinBatch; 2 where the caller's kernel must stay small in registers)
template <int FB = kFinBatch>
__device__ __forceinline__ void final_reduce(double *partials, int nb, int ld, int k, double *scratch, FinErr fe)
{
    const int T = blockDim.x;
    int kk = 1;
    while (kk < k) kk <<= 1;
    const int i = threadIdx.x & (kk - 1), sl = threadIdx.x / kk, nsl = T / kk;
    const double armed = __longlong_as_double((long long)kSentinelBits);
    double acc = 0.0;
    if (i < k) {
        for (int b0 = sl; b0 < nb; b0 += nsl * FB) {
            double v[FB];
            // the whole batch is requested at once (one round trip) and simply requested again while
            // any of its slots is still armed, i.e. its workgroup has not published yet
            const unsigned long long t0 = wall_clock64();
            bool armed_seen;
            do {
                armed_seen = false;
#pragma unroll
                for (int u = 0; u < FB; ++u) {
                    const int b = b0 + u * nsl;
                    v[u] = b < nb ? peek(partials + (size_t)b * ld + i) : 0.0;
                }
#pragma unroll
                for (int u = 0; u < FB; ++u) armed_seen = armed_seen || is_sentinel(v[u]);
                if (armed_seen) __builtin_amdgcn_s_sleep(1);
            } while (armed_seen && wall_clock64() - t0 < (unsigned long long)fe.ticks);  // default 4 s at 100 MHz
            // a slot still armed after the bound: its workgroup never published (never dispatched, or the
            // launch was rejected half way).  Not a numerical event: raise the context's sticky error word --
            // the host turns it into SPK_ERR_HIP and re-arms the whole buffer before the next use
            if (armed_seen && fe.err) __hip_atomic_store(fe.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int u = 0; u < FB; ++u) {
                const int b = b0 + u * nsl;
                if (b < nb) publish(partials + (size_t)b * ld + i, armed);  // re-arm for the next launch
                acc += v[u];
            }
        }
    }
    scratch[sl * kk + i] = acc;
    __syncthreads();
    for (int st = nsl >> 1; st > 0; st >>= 1) {
        if (sl < st) scratch[sl * kk + i] += scratch[(sl + st) * kk + i];
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// Peer-store collectives over xGMI (replace MPI_Allreduce / VecScatter inside
// KSPSolve; SURVEY 8(e): the payloads are <= 64 doubles and one node line, so
// latency is everything).  Data travels as 8-byte GRANULES {sequence number,
// 32 payload bits} written by ONE system-scope store each into the receiver's
// window (uncached device memory mapped into every peer): a granule is its own
// arrival flag, so there is no fence and no second round trip -- the receiver
// spins on the tag of each granule it needs.  Every poll is bounded (the peer
// may have died): on time-out the error word is raised and the kernel ends.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void st_sys(unsigned long long *p, unsigned long long v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ unsigned long long ld_sys(const unsigned long long *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// waits until the granule at p carries `seq`; lo = its payload.  false: timed out, or an earlier
// wait of this context did (the error word is sticky: once a peer is lost every later wait gives up
// at once, so a whole enqueued restart cycle drains in one time-out, not one per collective).
__device__ __forceinline__ bool granule_wait(const unsigned long long *p, uint32_t seq, uint32_t timeout_ms, uint32_t &lo,
                                             const int32_t *err, const int32_t *done = nullptr)
{
    unsigned long long g = ld_sys(p);
    if ((uint32_t)(g >> 32) != seq) {
        const unsigned long long t0 = wall_clock64();  // 100 MHz
        for (;;) {
            __builtin_amdgcn_s_sleep(2);
            g = ld_sys(p);
            if ((uint32_t)(g >> 32) == seq) break;
            if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 ||
                wall_clock64() - t0 > (unsigned long long)timeout_ms * 100000ull) {
                lo = 0;
                return false;
            }
            // the solve converged while this kernel was in flight: the peers stop sending, nobody
            // reads what is missing (every consumer starts with "if (*done) return")
            if (done && __hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
                lo = 0;
                return true;
            }
        }
    }
    lo = (uint32_t)g;
    return true;
}
// Raises the sticky error word of the peer-store backend and notes WHICH wait gave up (first one wins):
// err[1] = where (1..3: all-reduce after MDot / after MAXPY / stand-alone; 16: halo rows in a head kernel,
// 17: in the MAXPY-head kernel, 18: in kernel B (MAXPY + PCApply, forms 5 and 7), 19: granule exchange kernel,
// 20: bulk exchange kernel, 21: in the resident cycle kernel), err[2] = sequence number waited for.
__device__ __forceinline__ void raise_comm_error(int32_t *err, int where, uint32_t seq)
{
    if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
        err[1] = where;
        err[2] = (int32_t)seq;
    }
    __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double join_halves(uint32_t lo, uint32_t hi)
{
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Threads 0 .. 2*count-1 of the calling workgroup (count <= 64; a double's two halves sit in
// adjacent lanes) sum vals[0..count) over the ranks into out[0..count): every rank adds the
// P contributions in rank order, its own included, so all ranks hold the same bits.
// No barrier inside; vals may be LDS or global, out may alias vals.
__device__ __forceinline__ void peer_allreduce_block(const PeerAR &a, const double *vals, int count, double *out)
{
    const int t = threadIdx.x;
    if (t >= 2 * count) return;
    const int slot = (int)(a.seq & (kArSlots - 1));
    const uint32_t half = reinterpret_cast<const uint32_t *>(vals)[t];
    const unsigned long long g = ((unsigned long long)a.seq << 32) | half;
    const size_t mine = ((size_t)slot * a.P + a.me) * kArGranules + t;
    for (int p = 0; p < a.P; ++p) st_sys(a.win[p] + mine, g);
    const unsigned long long *own = a.win[a.me] + (size_t)slot * a.P * kArGranules + t;
    const unsigned long long tw0 = (a.stats && t == 0) ? wall_clock64() : 0ull;
    double sum = 0.0;
    bool ok = true;
    for (int p = 0; p < a.P; ++p) {
        uint32_t lo;
        ok = granule_wait(own + (size_t)p * kArGranules, a.seq, a.timeout_ms, lo, a.err) && ok;
        const uint32_t other = __shfl_xor(lo, 1, kWave);
        sum += join_halves(lo, other);  // meaningful in even lanes
    }
    if (a.stats && t == 0) {  // one lane accounts for the collective: stores issued -> every rank's lane arrived
        atomicAdd(a.stats + 2 * a.kind, wall_clock64() - tw0);
        atomicAdd(a.stats + 2 * a.kind + 1, 1ull);
    }
    if (!(t & 1)) out[t >> 1] = sum;
    if (!ok) raise_comm_error(a.err, 1 + a.kind, a.seq);
}

__device__ __forceinline__ double2 ld2(const double *p, int64_t i2)
{
    return reinterpret_cast<const double2 *>(p)[i2];
}
__device__ __forceinline__ double ld1nt(const double *p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void st_agent(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double ld_agent(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int converged_default(double rnorm, const KrylovState *st)
{
    if (isnan(rnorm) || isinf(rnorm)) return SPK_DIVERGED_NANORINF;
    if (rnorm <= st->ttol) return (rnorm < st->abstol) ? SPK_CONVERGED_ATOL : SPK_CONVERGED_RTOL;
    if (rnorm >= st->dtol * st->cnorm0) return SPK_DIVERGED_DTOL;
    return 0;
}

// ---------------------------------------------------------------------------
// The frame MINRES and pipelined CG share (spk_k_minres.hip, spk_k_pipecg.hip): the finish of their passes, the ||b||
// and start steps of the state's head, one init and one scalar kernel.  Each solver brings its vector passes and its
// state_step (the per-iteration tests stay per solver: their reasons take precedence in different orders).
// ---------------------------------------------------------------------------
__device__ void state_step(MinresState *ms, int mode, const double *sums, double *hist, int32_t hist_cap);
__device__ void state_step(PipecgState *ps, int mode, const double *sums, double *hist, int32_t hist_cap);

// block partials of NS sums, then (last workgroup) the reduction into out[0..NS) and the scalar step.  state: the pass's
// own pointer to the state (= step.state, already in registers: loading step.state instead moved the SGPR count)
template <int NS, class S>
__device__ __forceinline__ void state_finish(const double (&acc)[NS], double *red, double *partials, double *out, FinErr fe,
                                             S *state, const Step<S> &step)
{
    double w[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) w[k] = wave_sum(acc[k]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) red[k * kVWaves + (threadIdx.x >> 6)] = w[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) t[k] = 0.0;
#pragma unroll
        for (int j = 0; j < kVWaves; ++j) {
#pragma unroll
            for (int k = 0; k < NS; ++k) t[k] += red[k * kVWaves + j];
        }
        double *row = partials + (size_t)blockIdx.x * kPartialLd;
#pragma unroll
        for (int k = 0; k < NS; ++k) publish(row + k, t[k]);
    }
    if (!arrive_last(gridDim.x)) return;
    final_reduce(partials, gridDim.x, kPartialLd, NS, red, fe);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) out[k] = red[k];
        if (step.mode >= 0) state_step(state, step.mode, red, step.hist, step.hist_cap);
    }
}

// a residual norm in the norm of the test: dot = <M^-1 r, r>, sq = r.r
__device__ __forceinline__ double head_norm(const SolverHead *h, double dot, double sq)
{
    return h->norm == SPK_NORM_NATURAL ? sqrt(fabs(dot)) : sqrt(sq);
}

// ||b|| in the norm of the test, the reference of rtol with a nonzero guess: dot = <M^-1 b, b>, sq = b.b
__device__ __forceinline__ void head_bnorm(SolverHead *h, double dot, double sq) { h->ks.bnorm = head_norm(h, dot, sq); }

// Start, confirmation, restart on r = b - K x: dot = <M^-1 r, r>, sq = r.r.  true: the recurrence (re)starts, the
// solver then resets its own scalars
__device__ __forceinline__ bool head_begin(SolverHead *h, double dot, double sq, double *hist, int32_t hist_cap)
{
    KrylovState *st = &h->ks;
    const double rn = head_norm(h, dot, sq);
    st->rnorm = rn;
    if (!h->started) {
        // KSPConvergedDefault at iteration 0, as krylov_cycle_begin: zero guess -> the initial residual, nonzero guess ->
        // ||b|| (or the initial residual when b = 0), both in the norm of the test
        h->started = 1;
        double snorm = rn;
        if (st->guess_nonzero) {
            snorm = st->bnorm;
            if (snorm == 0.0) snorm = rn;
        }
        st->rnorm0 = rn;
        st->cnorm0 = snorm;
        st->ttol = fmax(st->rtol * snorm, st->abstol);
        if (hist_cap > 0) hist[0] = rn;
    } else if (st->done && !h->tent) {
        return false;   // a final verdict of the recurrence (indefinite PC or matrix, breakdown, divergence) stands
    }
    int reason = dot < 0.0 ? SPK_DIVERGED_INDEFINITE_PC : converged_default(rn, st);
    if (!reason && st->its >= st->max_it) reason = SPK_DIVERGED_ITS;
    // M^-1 r = 0 with r != 0; a NaN that reached only M^-1 r (a NaN in diag(A)) leaves ||r|| finite in the unpreconditioned norm
    if (!reason && !(dot > 0.0)) reason = isnan(dot) ? SPK_DIVERGED_NANORINF : SPK_DIVERGED_BREAKDOWN;
    h->tent = 0;
    st->reason = reason;
    if (reason) {
        st->done = 1;
        return false;
    }
    h->starts += 1;
    st->done = 0;
    return true;
}

__device__ __forceinline__ void init_extra(MinresState &) {}
__device__ __forceinline__ void init_extra(PipecgState &z, double tau)   // pipecgrr: no replacement pending, its tau
{
    z.rr_idle = 1;
    z.tau = tau;
}

template <class S, class... Tau>
__global__ void state_init_kernel(S *state, spk_opts o, int norm, Tau... tau)
{
    if (threadIdx.x != 0) return;
    S z;
    __builtin_memset(&z, 0, sizeof(S));   // (not S z{}: that left the MINRES state in scratch)
    z.ks.max_it = o.max_it;
    z.ks.rtol = o.rtol;
    z.ks.abstol = o.abstol;
    z.ks.dtol = o.dtol;
    z.ks.guess_nonzero = o.guess_nonzero;
    z.ks.ttol = o.abstol;
    z.ks.done = 1;   // no iteration runs before the first start
    z.norm = norm;
    init_extra(z, tau...);
    *state = z;
}
template <class S, class... Tau>
void state_init(S *state, const spk_opts &o, int norm, hipStream_t s, Tau... tau)
{
    hipLaunchKernelGGL(state_init_kernel<S>, dim3(1), dim3(64), 0, s, state, o, norm, tau...);
}

// several ranks: the step after the all-reduce of the sums (the iteration steps are gated like the passes)
template <class S>
__global__ void state_scalar_kernel(Step<S> step, const double *sums, const int32_t *done)
{
    if (threadIdx.x != 0) return;
    if (done && *done) return;
    state_step(step.state, step.mode, sums, step.hist, step.hist_cap);
}
template <class S>
void state_scalar(Step<S> step, const double *sums, const int32_t *done, hipStream_t s)
{
    hipLaunchKernelGGL(state_scalar_kernel<S>, dim3(1), dim3(64), 0, s, step, sums, done);
}

// One Arnoldi step's scalar work (KSPFGMRESUpdateHessenberg + KSPConvergedDefault), run by a
// whole workgroup: the lanes stage the column and the stored rotations in LDS (parallel
// loads), lane 0 runs the dependent chain out of LDS and writes the column back once.
// Called from the stand-alone kernel (generic path) and from workgroup 0 of the fused
// iteration-head kernel, where it overlaps with that kernel's streaming.
// CAP: capacity of the LDS staging (restart + 2); the fused kernels carry the small instance, restart lengths beyond
// kMaxNv - 2 take the stand-alone kernel with the large one (krylov_givens)
// lds: 4 * cap + 4 doubles of LDS scratch (the caller's own staging where it has any: a rider workgroup of a product
// launch uses the tile's product buffer, so the launch needs no LDS beyond what its row tiles need)
// LEAN: loops kept rolled -- the step then fits 32 VGPRs, which is what a rider workgroup of the SpMV kernels may use
// without raising the register allocation of every row-tile wave of the launch (measured: 64 instead of 32 allocated
// VGPRs cost the 1024^2 product 5 us of 62); the serial chain takes ~1 us longer, beside the row tiles
// What the step reads that does NOT depend on the norm (the Hessenberg column, the stored rotations, rs[loc], the gate
// words), requested by the lanes that will stage it: a caller with work of its own between the request and the use (the
// rider's reduction) overlaps the two round trips.  loc <= blockDim.x - 1 (the small instance: restart <= 62).
struct GivensPre {
    double h, c, s, rs;
    int go;   // 0: the solve / cycle is over (uniform)
};
__device__ __forceinline__ GivensPre givens_prefetch(const KrylovArrays &ka, int loc, const double *dots)
{
    GivensPre p{0.0, 0.0, 0.0, 0.0, 0};
    const KrylovState *st = ka.st;
    p.go = !(st->done || st->skip_iter);
    if ((int)threadIdx.x <= loc) {
        p.h = dots[threadIdx.x];
        p.c = ka.cc[threadIdx.x];
        p.s = ka.ss[threadIdx.x];
    }
    if (threadIdx.x == 33) p.rs = ka.rs[loc];
    return p;
}
template <bool LEAN = false>
__device__ inline void givens_block_lds(const KrylovArrays &ka, int loc, const double *dots, const double *nrm2, double *lds, int cap, const GivensPre *pre = nullptr)
{
    double *Hc = lds, *Hr = lds + cap, *ccs = lds + 2 * cap, *sss = lds + 3 * cap, *sc = lds + 4 * cap;
    KrylovState *st = ka.st;
    if (pre ? !pre->go : (st->done || st->skip_iter)) return;  // uniform: read before anyone writes it
    const int ldh = ka.ldh;
    double *Hg = ka.H + (size_t)ldh * loc;  // column loc
    // every global value the serial chain needs is fetched here, in parallel, once
    if (pre) {
        if ((int)threadIdx.x <= loc) {
            Hc[threadIdx.x] = pre->h;
            ccs[threadIdx.x] = pre->c;
            sss[threadIdx.x] = pre->s;
        }
        if (threadIdx.x == 33) sc[1] = pre->rs;
    } else {
        for (int j = threadIdx.x; j <= loc; j += blockDim.x) {
            Hc[j] = dots[j];
            ccs[j] = ka.cc[j];
            sss[j] = ka.ss[j];
        }
        if (threadIdx.x == 33) sc[1] = ka.rs[loc];
    }
    if (threadIdx.x == 32) sc[0] = *nrm2;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double rs_loc = sc[1];
    const double tt = sqrt(sc[0]);
    if (isnan(tt) || isinf(tt)) {  // KSPCheckNorm: KSP_DIVERGED_NANORINF
        st->rnorm = tt;
        st->reason = SPK_DIVERGED_NANORINF;
        st->done = 1, st->skip_iter = 1;
        return;
    }
    // happy breakdown test
    double hapbnd = fabs(tt / rs_loc);
    if (hapbnd > 1e-30) hapbnd = 1e-30;
    const int hapend = !(tt > hapbnd);
    st->tt = tt;
    st->inv_tt = hapend ? 1.0 : 1.0 / tt;
    // previous rotations on the new column.  The running entry stays in a register and the rotated
    // entries go to an array of their own, so the loop's LDS loads do not wait for its stores: the
    // serial chain is two FMAs per step (LDS round trips per step cost ~3 us at loc = 30, on the
    // critical path of the head kernel this step rides in)
    double run = Hc[0];
    if constexpr (LEAN) {
#pragma unroll 2
        for (int j = 1; j <= loc; ++j) {
            const double h1 = Hc[j], cj = ccs[j - 1], sj = sss[j - 1];
            Hr[j - 1] = cj * run + sj * h1;
            run = cj * h1 - sj * run;
        }
    } else {
        for (int j = 1; j <= loc; ++j) {
            const double h1 = Hc[j], cj = ccs[j - 1], sj = sss[j - 1];
            Hr[j - 1] = cj * run + sj * h1;
            run = cj * h1 - sj * run;
        }
    }
    Hr[loc] = run;
    Hr[loc + 1] = tt;
    double rnorm;
    int reason = 0;
    if (!hapend) {
        const double h0 = run, h1 = tt;
        const double d = sqrt(h0 * h0 + h1 * h1);
        if (d == 0.0) {
            st->reason = SPK_DIVERGED_NULL;
            st->done = 1, st->skip_iter = 1;
            return;
        }
        const double c = h0 / d, sn = h1 / d;
        ka.cc[loc] = c;
        ka.ss[loc] = sn;
        ka.rs[loc + 1] = -sn * rs_loc;
        ka.rs[loc] = c * rs_loc;
        Hr[loc] = c * h0 + sn * h1;
        rnorm = fabs(sn * rs_loc);
    } else {
        rnorm = 0.0;
    }
    if constexpr (LEAN) {
#pragma unroll 1
        for (int j = 0; j <= loc + 1; ++j) Hg[j] = Hr[j];
    } else {
        for (int j = 0; j <= loc + 1; ++j) Hg[j] = Hr[j];
    }
    st->its += 1;
    st->loc_done = loc + 1;
    st->rnorm = rnorm;
    st->hapend = hapend;
    if (st->its < ka.hist_cap) ka.hist[st->its] = rnorm;
    reason = converged_default(rnorm, st);
    if (hapend && !reason) reason = SPK_DIVERGED_BREAKDOWN;
    if (!reason && st->its >= st->max_it) reason = SPK_DIVERGED_ITS;
    if (reason > 0 && ka.tentative) {
        // single-reduction mode: ||w'|| came out of a difference that can sit in rounding noise, so the
        // recurrence is trusted to END THE CYCLE only; the restart's true residual decides (krylov_cycle_begin)
        st->skip_iter = 1;
        return;
    }
    if (ka.theta > 0.0 && (reason == SPK_DIVERGED_ITS || (!reason && rnorm <= ka.theta * st->beta))) {
        // an FP32 basis: -ksp_max_it is confirmed on the true residual as well (the reported norm is then the true one),
        // and a cycle whose recurrence residual has fallen to theta of its starting residual ends here -- the stored
        // vectors carry rounding noise from there on (kBasisTheta)
        st->skip_iter = 1;
        return;
    }
    st->reason = reason;
    if (reason) {
        st->done = 1, st->skip_iter = 1;
    }
}

template <int CAP>
__device__ void givens_block_t(const KrylovArrays &ka, int loc, const double *dots, const double *nrm2)
{
    __shared__ double lds[4 * CAP + 4];
    givens_block_lds<false>(ka, loc, dots, nrm2, lds, CAP);
}
__device__ inline void givens_block(const KrylovArrays &ka, int loc, const double *dots, const double *nrm2)
{
    givens_block_t<kMaxNv + 2>(ka, loc, dots, nrm2);
}

__device__ __forceinline__ double inv_norm(double nrm2)  // the VecScale guard of the head kernels
{
    const double tt = sqrt(nrm2);
    return tt > 1e-300 ? 1.0 / tt : 1.0;
}
// lds: >= kThreads + 4 * (kMaxNv + 2) + 4 doubles of the calling workgroup's LDS
__device__ __forceinline__ void givens_rider(const GivensRider &gr, double *lds)
{
    // The MAXPY launch left ||w'||^2 as one partial per workgroup (IterB::defer_fin): reduced here, in the fixed order,
    // and all-reduced across ranks (peer-store) -- beside the row tiles, since nothing in a product on an un-normalised
    // basis needs the norm: neither the reduction tail nor the link latency is on the critical path
    // (what the Givens step reads besides the norm is requested first: one round trip beside the reduction's)
    const GivensPre pre = givens_prefetch(gr.ka, gr.loc, gr.h);
    if (gr.fin_n > 0) {
        double *red = lds;
        double *slot = gr.fin_partials + (size_t)gr.fin_n * kPartialLd;  // the multiplier entries' share
        double lam2 = 0.0;
        if (threadIdx.x == 0) lam2 = peek(slot);
        final_reduce<2>(gr.fin_partials, gr.fin_n, kPartialLd, 1, red, gr.fe);
        if (threadIdx.x == 0) {
            publish(slot, __longlong_as_double((long long)kSentinelBits));   // re-armed for the next user of the row
            red[0] = red[0] + lam2;
        }
        __syncthreads();
        if (gr.ar.P) peer_allreduce_block(gr.ar, red, 1, gr.nrm2);
        else if (threadIdx.x == 0) gr.nrm2[0] = red[0];
        __syncthreads();
    }
    // un-normalised basis: the scale factor of the vector the MAXPY launch just wrote (its norm is all-reduced by now)
    // (nothing compounds: V~_j = w' of the product of the NORMALISED v_{j-1}, so ||V~_j|| = h_{j,j-1} <= ||K M^-1||)
    if (gr.sc && threadIdx.x == 0) gr.sc[gr.loc + 1] = inv_norm(*gr.nrm2);
    givens_block_lds<true>(gr.ka, gr.loc, gr.h, gr.nrm2, lds + kThreads, kMaxNv + 2, &pre);
}

void givens_rider_alone(const GivensRider &gr, const int32_t *done, hipStream_t s);  // spk_k_krylov.hip
inline GivensRider no_rider()
{
    GivensRider g{};
    g.loc = -1;
    return g;
}

// ---------------------------------------------------------------------------
// The frame of the A-block product kernels  y (+)= A x (+ B^T lambda) (+ off-rank part)  (spk_k_spmv.hip, spk_k_dict.hip,
// spk_k_dict3.hip).  A layout supplies its own sum of A x per row, its early load of y and its store; what stands around
// them -- the gate and the rider, the workgroup's place on its XCD, the row's off-rank and B^T terms, the launch -- is here.
// ---------------------------------------------------------------------------
// what a row adds to its sum of A x: B^T rows times lam (bt_rowptr == nullptr: none) and the off-rank columns
struct RowTail {
    const int32_t *bt_rowptr, *bt_colidx;
    const double *bt_val, *lam;
    OffDiag od;
};

// the gate, then the rider in workgroup 0 of a RIDE launch (lds: see givens_rider).  Returns the workgroup's number among
// those that hold rows, -1: nothing (more) to do
template <bool RIDE>
__device__ __forceinline__ int product_prologue(const int32_t *done, const GivensRider &gr, double *lds)
{
    if (done && *done) return -1;
    if (RIDE && blockIdx.x == 0) {  // a pending Givens step beside the rows
        givens_rider(gr, lds);
        return -1;
    }
    return (int)blockIdx.x - (RIDE ? 1 : 0);
}
// workgroups b, b+8, ... share an XCD (round-robin dispatch): each XCD gets a contiguous run of row tiles, so the x window
// stays in ITS L2
__device__ __forceinline__ int xcd_tile(int bx, int tiles_per_xcd) { return (bx & 7) * tiles_per_xcd + (bx >> 3); }

// s += off-rank columns of the row (ghost values already exchanged), then (bt) its B^T entries times lam, each in stored
// order, one fused multiply-add per entry: the ONE spelling of these sums, so every layout gives the same bits.
// (In place: with s passed and returned by value the pipelined 2x2 kernel is scheduled into 222 VGPRs instead of 168.)
__device__ __forceinline__ void row_tail_bt(const RowTail &t, int k, int k1, double &s)
{
    for (; k < k1; ++k) s = __builtin_fma(t.bt_val[k], t.lam[t.bt_colidx[k]], s);
}
__device__ __forceinline__ void row_tail_add(const RowTail &t, int64_t row, double &s, bool bt)
{
    if (t.od.rowptr)
        for (int k = t.od.rowptr[row]; k < t.od.rowptr[row + 1]; ++k) s = __builtin_fma(t.od.val[k], t.od.xg[t.od.colidx[k]], s);
    if (bt) row_tail_bt(t, t.bt_rowptr[row], t.bt_rowptr[row + 1], s);
}
// The first B^T entries of a row fetched early, behind the matrix stream, not at the end of the kernel (MatMult on the nest
// operator, 1024^2: 80.2 us against 68.5 for the product without them); a longer row takes the rest in add().
// row_tail_add(t, row, s, false) followed by add(t, s) is row_tail_add(t, row, s, true), bit for bit.
constexpr int kBtPre = 4;
struct BtPre {
    int k0, k1;
    double v[kBtPre], l[kBtPre];
    __device__ __forceinline__ void load(const RowTail &t, int64_t row)
    {
        k0 = t.bt_rowptr[row];
        k1 = t.bt_rowptr[row + 1];
#pragma unroll
        for (int j = 0; j < kBtPre; ++j) {
            const bool in = k0 + j < k1;
            v[j] = in ? t.bt_val[k0 + j] : 0.0;
            l[j] = in ? t.lam[t.bt_colidx[k0 + j]] : 0.0;
        }
    }
    __device__ __forceinline__ void add(const RowTail &t, double &s) const
    {
#pragma unroll
        for (int j = 0; j < kBtPre; ++j)
            if (k0 + j < k1) s = __builtin_fma(v[j], l[j], s);
        row_tail_bt(t, k0 + kBtPre, k1, s);
    }
};

// the damped-Jacobi update of the FP32 sweeps on the same layouts, every operation rounded on its own (the oracle's float loop)
__device__ __forceinline__ float sweep_update(float y, float omega, float d, float x, float s)
{
#pragma clang fp contract(off)
    return y + ((omega * d) * (x - s));
}

// Host side: what every product launcher works out from its arguments before it launches
struct ProductLaunch {
    RowTail tail;
    GivensRider gr;
    const int32_t *done;
    int nride;          // workgroups in front of those that hold rows
    bool acc, ride, bt;
    size_t rider_lds;   // dynamic LDS the rider needs in its workgroup (kernels without static LDS of that size)
};
// a rank without rows: the rider without tiles, and nothing else to launch
inline bool product_is_empty(int64_t nrows, const GivensRider *rider, const int32_t *done, hipStream_t s)
{
    if (nrows == 0 && rider) givens_rider_alone(*rider, done, s);
    return nrows == 0;
}
inline ProductLaunch make_product_launch(const CsrDev *bt, const double *lam, const OffDiag *od, const GivensRider *rider,
                                         const int32_t *done, bool accumulate)
{
    // (B^T rows: MatMult on the nest operator, never the iteration's launch)
    if (bt && rider) fail(SPK_ERR_ARG, "A-block product: B^T rows and a rider in one launch");
    ProductLaunch p{};
    p.tail = RowTail{bt ? bt->rowptr.p : nullptr, bt ? bt->colidx.p : nullptr, bt ? bt->val.p : nullptr, lam,
                     od ? *od : OffDiag{nullptr, nullptr, nullptr, nullptr}};
    p.gr = rider ? *rider : no_rider();
    p.done = done;
    p.nride = rider ? 1 : 0;
    p.acc = accumulate;
    p.ride = rider != nullptr;
    p.bt = bt != nullptr;
    p.rider_lds = rider ? sizeof(double) * (size_t)(kThreads + 4 * (kMaxNv + 2) + 4) : 0;
    return p;
}
// f(ACC, RIDE, BT) as std::bool_constant values, for the six combinations a product is launched in
template <class F>
inline void dispatch_product(bool acc, bool ride, bool bt, F &&f)
{
    using Y = std::true_type;
    using N = std::false_type;
    if (bt) acc ? f(Y{}, N{}, Y{}) : f(N{}, N{}, Y{});
    else if (acc) ride ? f(Y{}, Y{}, N{}) : f(Y{}, N{}, N{});
    else ride ? f(N{}, Y{}, N{}) : f(N{}, N{}, N{});
}

// tile length (double2 per lane) and grid of the wave-split forms: about one tile per workgroup
struct WsShape {
    int U, grid;
    bool on;
};
inline WsShape ws_shape(int64_t n2)
{
    WsShape v;
    static const int knob = [] { const char *e = getenv("SPK_VEC_WS"); return e ? atoi(e) : -1; }();  // 0: off, 2/4/8: force U
    v.on = n2 < (int64_t)kVecMaxBlocks * 2048 && knob != 0;
    v.U = n2 >= (int64_t)kVecMaxBlocks * 64 * 8 ? 8 : (n2 >= (int64_t)kVecMaxBlocks * 64 * 4 ? 4 : 2);
    if (knob == 2 || knob == 4 || knob == 8) v.U = knob;
    int64_t tiles = (n2 + 64 * v.U - 1) / (64 * v.U);
    if (tiles < 1) tiles = 1;
    v.grid = (int)(tiles < kVecMaxBlocks ? tiles : kVecMaxBlocks);
    return v;
}

// The keep set of form 7 (gs_fused_kernel): operands of the workgroup's FIRST tile that VecMDot's pass has in registers
// and kernel B's pass reads again -- w~ (raw), the parity planes of B D, V_0 .. V_{KV-1} -- stay on chip between the two
// passes instead of being fetched from HBM a second time.  Items are numbered in that order; item k < KR lives in
// registers, the others in the workgroup's LDS (one double2 per lane and u: lane-private, no barrier needed).  Every
// index is a compile-time constant once the loops around put/get are unrolled, and the first tile is told by a flag
// inside the tile loops: a copy of the loop body for it costs > 35 VGPRs in either pass (scratch at MP = 4).  So register
// items must be dead before kernel B's tile loop (w~ and the planes are: they move into its prefetch arrays ahead of the
// loop); the kept basis vectors are read inside the loop and live in LDS.  NoKeep (the default of both bodies) keeps
// nothing and compiles to the code without a keep set.
// AH (SPK_GS_AHEAD, a launch with a keep set only): what kernel B's pass asks for ahead of the totals wait beyond the
// first group that is not kept -- the first AH vectors of the group behind it (V_{KV+G} .. V_{KV+G+AH-1}), requested
// into the tile loop's own buffer, which is empty until the loop's first trip.  No addition moves.
struct NoKeep {
    static constexpr int KW = 0, KP = 0, KV = 0, AH = 0;
    static constexpr bool any = false, fused = false, PK = false;
    __device__ __forceinline__ void put(int, int, double2) {}
    __device__ __forceinline__ double2 get(int, int) const { return double2{0.0, 0.0}; }
};
template <int T, int U, int KW_, int KP_, int KV_, int KR_, int AH_ = 0, bool PK_ = false>
struct KeepSet {
    static constexpr int KW = KW_, KP = KP_, KV = KV_, KR = KR_, N = KW_ + KP_ + KV_, KL = N > KR_ ? N - KR_ : 0;
    static constexpr int AH = AH_;
    static constexpr bool PK = PK_;   // kernel B's pass is only launched on parity planes of B D (IterB::packed)
    static_assert(AH_ == 0 || KV_ > 0, "the loads ahead of the wait follow the kept vectors");
    static constexpr bool any = N > 0, fused = true;   // fused: a KeepSet (an empty one too) is form 7's launch
    double2 r[KR_ > 0 ? KR_ : 1][U];
    double2 *l;   // KL * U * T double2 of LDS
    __device__ __forceinline__ void put(int k, int u, double2 v)
    {
        if (k < KR) r[k][u] = v;
        else l[((k - KR) * U + u) * T + threadIdx.x] = v;
    }
    __device__ __forceinline__ double2 get(int k, int u) const
    {
        return k < KR ? r[k][u] : l[((k - KR) * U + u) * T + threadIdx.x];
    }
};

// One element's step of a VecMDot sum with the contraction WRITTEN OUT: which product is fused into the FMA decides the
// rounding, and the remainder epilogue of the fused launch (TAIL below) must round as the tile loop does, so neither
// is left to the compiler's choice.  The forms are the ones the compiler chose for the loop before this helper existed
// (the loop's v_mul_f64 / v_fma_f64 / v_add_f64 sequence on gfx950 is unchanged).
__device__ __forceinline__ double mdot_step(double d, double2 a, double2 w)   // d + (a . w)
{
#pragma clang fp contract(off)
    return d + __builtin_fma(w.x, a.x, w.y * a.y);
}
__device__ __forceinline__ double mdot_step_x(double d, double2 a, double2 w) { return __builtin_fma(w.x, a.x, d); }   // parity planes:
__device__ __forceinline__ double mdot_step_y(double d, double2 a, double2 w) { return __builtin_fma(w.y, a.y, d); }   // one half each
__device__ __forceinline__ double mdot_step_ww(double s, double2 w)           // s + (w . w)
{
#pragma clang fp contract(off)
    return s + __builtin_fma(w.y, w.y, w.x * w.x);
}

// VecMDot body (mdot_kernel, gs_fused_kernel): the workgroup's tiles (tile = blockIdx.x + k gridDim.x of T x U double2),
// all nv dot products V_i . w in ONE pass over w (kept in registers), w.w in slot nv (with_ww); the workgroup's sums
// are published to partials[blockIdx.x][0..nv] for the reducer.  lds: max(W (NG 8 + 1), T) doubles.
// keep: the first tile leaves its operands in the keep set (needs gridDim.x whole tiles in n2).  With split, its kept
// planes are loaded ONCE: their slots in the groups turn into dead ones and their dot products, the same sums over u of
// the same values, are added behind the groups.  No order of additions changes.
// FUSED (gs_fused_kernel): gate is the launch's `done` word, requested by the caller and looked at behind the first
// tile's first loads (a gated workgroup returns true: nothing added, nothing published); the wave sums are taken by
// wave_sum_multi (the same trees as wave_sum, which mdot_kernel keeps: forms 5 and 7 agree to the bit).
// TAIL (the launcher vouches: 0 < n2 mod (T U) <= kGsTailMax, the whole tiles a multiple of the grid): the remainder
// tile is no loop trip.  Its owner -- the workgroup the loop would give it to -- requests the remainder's entries of w~,
// the vectors and the second slab at entry (two loads per thread), stores them to tl (kGsTailSrc x kGsTailMax double2 of
// LDS) where the gate is looked at, and adds their products behind the loop.  That is what the trip would have added:
// there every thread past n2 has wv = 0, so its d is a sum of +-0 and acc[i] += mk d leaves the accumulator as it is
// (one that starts at +0.0 and only receives sums is never -0.0); for the same reason the u >= 1 terms of the live
// threads (u T + t >= T > R) leave d's value, and a zero's sign in d is lost in acc[i] += d.  What remains per live
// slot, in slot order, is d = 0.0 + one mdot_step and acc[i] += d, with the same n_dot masks on w~.  The kept-plane
// path (kpl) is the first tile's; the remainder never is the first tile.
template <int NG, int T, int G, bool NT, int U, class Keep = NoKeep, bool FUSED = false, bool TAIL = false>
__device__ __forceinline__ bool mdot_tiles(const double *__restrict__ V, int64_t ldv, int nv,
                                           const double *__restrict__ V2, int nv1,
                                           const double *__restrict__ w, int64_t n2,
                                           int64_t n_dot, double *__restrict__ partials,
                                           int with_ww, int split, double *lds, Keep *keep = nullptr, int32_t gate = 0,
                                           double2 *tl = nullptr)
{
    constexpr int NA = NG * 8 + 1, W = T / kWave, TILE2 = T * U;
    constexpr int KW = Keep::KW, KP = Keep::KP, KV = Keep::KV;
    static_assert(!TAIL || (FUSED && kGsTailMax < T && kGsTailSrc * kGsTailMax <= 2 * T && NG * 8 + 1 <= kGsTailSrc),
                  "the remainder: fused launch, live in u = 0 only, two loads per thread, one source per slot and w~");
    double acc[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) acc[i] = 0.0;

    const int64_t ntw = n2 / TILE2;   // whole tiles
    const int R = TAIL ? (int)(n2 - ntw * TILE2) : 0;
    const bool own = TAIL && (int64_t)blockIdx.x == ntw % (int64_t)gridDim.x;   // workgroup-uniform
    double2 st[2];
    if (TAIL && own) {
        // sources: w~, V_0 .. V_{nv1-1}, the second slab's planes (split) or rows
        const int nsrc = 1 + nv1 + (nv > nv1 ? (split ? (nv - nv1 + 1) >> 1 : nv - nv1) : 0);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int q = (int)threadIdx.x + j * T, s = q / kGsTailMax, e = q % kGsTailMax;
            st[j].x = st[j].y = 0.0;
            if (s < nsrc && e < R) {
                const int64_t i2 = ntw * TILE2 + e;
                if (s == 0) st[j] = ld2(w, i2);
                else st[j] = ld2s<NT>(s <= nv1 ? V + (size_t)(s - 1) * ldv : V2 + (size_t)(s - 1 - nv1) * ldv, i2);
            }
        }
    }

    for (int64_t tile = blockIdx.x; TAIL ? tile < ntw : tile * TILE2 < n2; tile += gridDim.x) {
        const bool KF = Keep::any && tile == (int64_t)blockIdx.x;   // the first tile leaves its operands behind
        const bool kpl = KF && KP > 0 && split && nv > nv1;   // this tile's planes go through the keep set
        double2 wv[U];
        int64_t idx[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            idx[u] = tile * TILE2 + u * T + threadIdx.x;
            if (idx[u] < n2) {
                wv[u] = ld2(w, idx[u]);
                if (KF && KW) keep->put(0, u, wv[u]);
                if (2 * idx[u] >= n_dot) wv[u].x = 0.0;
                if (2 * idx[u] + 1 >= n_dot) wv[u].y = 0.0;
            } else {
                wv[u].x = wv[u].y = 0.0;
                idx[u] = 0;  // safe address, zero weight
            }
        }
        if (kpl) {
#pragma unroll
            for (int q = 0; q < KP; ++q) {
                const bool live = nv1 + 2 * q < nv;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    double2 e{0.0, 0.0};
                    if (live) e = ld2s<NT>(V2 + (size_t)q * ldv, idx[u]);
                    keep->put(KW + q, u, e);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc[NA - 1] = mdot_step_ww(acc[NA - 1], wv[u]);
#pragma unroll
        for (int g0 = 0; g0 < NG * 8; g0 += G) {
            if (g0 < nv) {  // wave-uniform
                double2 a[G][U];
#pragma unroll
                for (int v = 0; v < G; ++v) {
                    // a slot past nv loads ONE broadcast address (w[0..1], weight 0) instead of a
                    // vector tile: the group stays branch-free and costs no bandwidth
                    // (so does the slot of a kept plane: its dot product follows behind the groups)
                    const bool live = g0 + v < nv && !(kpl && g0 + v >= nv1 && ((g0 + v - nv1) >> 1) < KP);
                    const int ic = live ? g0 + v : 0;
                    // vectors nv1.. come from a second slab (the rows of B D in the single-reduction mode);
                    // split: that slab holds parity-interleaved planes, "vector" j is half j & 1 of plane j / 2
                    const int j2 = ic - nv1;
                    const double *Vi = !live ? w : (ic < nv1 ? V + (size_t)ic * ldv : V2 + (size_t)(split ? j2 >> 1 : j2) * ldv);
#pragma unroll
                    for (int u = 0; u < U; ++u) a[v][u] = ld2s<NT>(Vi, live ? idx[u] : 0);
                }
                if (FUSED && g0 == 0 && tile == (int64_t)blockIdx.x) {
                    // the first tile's loads are in flight; the empty statement pins the look at the gate HERE (the test
                    // is loop-invariant: hoisted ahead of the loop it waits for the gate before the first request)
                    asm volatile("" : "+v"(gate));
                    if (__builtin_amdgcn_readfirstlane(gate)) return true;
                    GS_STAMP_COPY(kGsEntry, kGsEntryRaw);
                    if (TAIL && own) {   // the remainder's entries were requested ahead of this tile's: they are back first
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const int q = (int)threadIdx.x + j * T;
                            if (q < kGsTailSrc * kGsTailMax) tl[q] = st[j];
                        }
                    }
                }
#pragma unroll
                for (int v = 0; v < G; ++v) {
                    const bool live = g0 + v < nv && !(kpl && g0 + v >= nv1 && ((g0 + v - nv1) >> 1) < KP);
                    const double mk = live ? 1.0 : 0.0;
                    double d = 0.0;
                    if (split && g0 + v >= nv1 && live) {  // wave-uniform
                        if ((g0 + v - nv1) & 1) {
#pragma unroll
                            for (int u = 0; u < U; ++u) d = mdot_step_y(d, a[v][u], wv[u]);
                        } else {
#pragma unroll
                            for (int u = 0; u < U; ++u) d = mdot_step_x(d, a[v][u], wv[u]);
                        }
                    } else {
#pragma unroll
                        for (int u = 0; u < U; ++u) d = mdot_step(d, a[v][u], wv[u]);
                    }
                    acc[g0 + v] += mk * d;
                }
                if (FUSED && g0 == 0 && tile == (int64_t)blockIdx.x) GS_STAMP(kGsFirstLoads);
                if (KF && g0 < KV) {  // behind the group's sums: a store of a loaded value waits for it
#pragma unroll
                    for (int v = 0; v < G; ++v) {
                        if (g0 + v < KV && g0 + v < nv1) {
#pragma unroll
                            for (int u = 0; u < U; ++u) keep->put(KW + KP + g0 + v, u, a[v][u]);
                        }
                    }
                }
            }
        }
        if (kpl) {
#pragma unroll
            for (int q = 0; q < KP; ++q) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int slot = nv1 + 2 * q + h;
                    if (slot < nv) {  // wave-uniform
                        double d = 0.0;
                        if (h) {
#pragma unroll
                            for (int u = 0; u < U; ++u) d = mdot_step_y(d, keep->get(KW + q, u), wv[u]);
                        } else {
#pragma unroll
                            for (int u = 0; u < U; ++u) d = mdot_step_x(d, keep->get(KW + q, u), wv[u]);
                        }
#pragma unroll
                        for (int i = 0; i < NA - 1; ++i)
                            if (i == slot) acc[i] += d;
                    }
                }
            }
        }
    }
    if (TAIL && own) {
        __syncthreads();   // the staged entries come from other threads (a branch the whole workgroup takes)
        if ((int)threadIdx.x < R) {
            const int e = threadIdx.x;
            const int64_t i2 = ntw * TILE2 + e;
            double2 wt = tl[e];
            if (2 * i2 >= n_dot) wt.x = 0.0;
            if (2 * i2 + 1 >= n_dot) wt.y = 0.0;
            acc[NA - 1] = mdot_step_ww(acc[NA - 1], wt);
#pragma unroll
            for (int g0 = 0; g0 < NG * 8; g0 += G) {
#pragma unroll
                for (int v = 0; v < G; ++v) {
                    if (g0 + v < nv) {  // wave-uniform: acc[] stays statically indexed
                        const int j2 = g0 + v - nv1;
                        const double2 a = tl[(g0 + v < nv1 ? 1 + g0 + v : 1 + nv1 + (split ? j2 >> 1 : j2)) * kGsTailMax + e];
                        double d = 0.0;
                        if (split && j2 >= 0) d = (j2 & 1) ? mdot_step_y(d, a, wt) : mdot_step_x(d, a, wt);
                        else d = mdot_step(d, a, wt);
                        acc[g0 + v] += d;
                    }
                }
            }
        }
    }
    // workgroup sums -> partials[block][i]; w.w goes to slot nv
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (FUSED) GS_STAMP(kGsTilesDone);
    if (FUSED) {
        wave_sum_multi(acc);
        const int i = wave_sum_owner(lane);
        if (i < NA) lds[wave * NA + i] = acc[0];
    } else {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const double s = wave_sum(acc[i]);
            if (lane == 0) lds[wave * NA + i] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x < NA) {
        const int i = threadIdx.x;
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < W; ++j) s += lds[j * NA + i];
        double *row = partials + (size_t)blockIdx.x * kPartialLd;
        if (i < nv) publish(row + i, s);
        else if (i == NA - 1 && with_ww) publish(row + nv, s);
    }
    if (FUSED) GS_STAMP(kGsPublished);
    return false;
}

// Workgroup shape of the reducing vector kernels: big vectors get 512 threads x 4 double2
// (few fat workgroups: cheap finish), small ones get thinner tiles so that ~256 workgroups
// still exist (a 131 k-row slab on 32 workgroups left 7/8 of the chip idle: 20 us instead of 5).
struct VecShape {
    int T, U, grid, G;
};
inline VecShape vec_shape(int64_t n2, bool maxpy = false)
{
    VecShape v;
    v.G = 4;
    int cap = kVecMaxBlocks;
    if (n2 >= (int64_t)kVecMaxBlocks * 2048) { v.T = 512; v.U = 4; }
    else if (n2 >= (int64_t)kVecMaxBlocks * 1024) { v.T = 256; v.U = 4; }
    else if (n2 >= (int64_t)kVecMaxBlocks * 512) { v.T = 256; v.U = 2; }
    else { v.T = 256; v.U = 1; }
    // MAXPY on small vectors: thin workgroups, 8 vectors in flight (1/8 slab, 30 vectors: 17.1 -> 12.7 us,
    // 1/4 slab: 84 -> 79 us per iteration)
    if (maxpy && n2 < (int64_t)kVecMaxBlocks * 1024) { v.T = 256; v.U = 1; v.G = 8; cap = 1024; }
    else if (maxpy && n2 < (int64_t)kVecMaxBlocks * 2048) { v.T = 256; v.U = 2; v.G = 8; cap = 1024; }
    int64_t tiles = (n2 + (int64_t)v.T * v.U - 1) / ((int64_t)v.T * v.U);
    if (tiles < 1) tiles = 1;
    v.grid = (int)(tiles < cap ? tiles : cap);
    return v;
}
inline int vec_grid(int64_t n2, int T = kVT)
{
    // one double2 per thread and pass: small vectors still get a workgroup per CU (a 1/8 slab of the 1024^2 grid ran its
    // restart norms on 64 workgroups)
    int64_t tiles = (n2 + (int64_t)T - 1) / (int64_t)T;
    if (tiles < 1) tiles = 1;
    const int cap = T >= 512 ? kVecMaxBlocks : 2 * kVecMaxBlocks;
    return (int)(tiles < cap ? tiles : cap);
}

}  // namespace k
}  // namespace spk
