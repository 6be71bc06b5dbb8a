// spk_k_pipecg.hip -- the vector passes and the scalar step of the device-resident pipelined CG (spk_pipecg;
// Ghysels-Vanroose 2014 Alg. 3 in the order of PETSc's KSPSolve_PIPECG), K = A only.
// Per iteration (one rank, none / Jacobi):
//   product       n = K m                                       (the product kernels, unchanged; m = w without a PC)
//   pipecg_pass   z = n + b z, s = w + b s, p = u + b p, x += a p, r -= a s, w -= a z, u = D r, m = D w,
//                 sums [<r, u>, <w, u>, r.r]                     finisher: the test, then alpha / beta of the next pass
// With a diagonal M^-1 (none, Jacobi) u = D r and q = D s are formed in the pass and never stored.  With the V-cycle (or
// opts.fused = 0) m = M^-1 w runs through op_pc_apply before the product; the V-cycle keeps u and q as recurrences
// (q = m + b q, u -= a q), the step-by-step path recomputes u = M^-1 r with a launch of its own and takes the sums in a
// second pass of this kernel, in the same order.
// Summation orders are fixed (block partials + the sentinel finish of spk_device.hpp): identical solves, identical bits.
// pipecgrr (spk_pipecgrr) adds, at a chunk boundary, the gap check pipecgrr_gap after t = K x (step kPcGap: rr_idle), and
// a replacement gated by rr_idle: pipecgrr_fill (r = b - t, u = D r), the products K u, K p, pipecgrr_fill (q = D s), K q,
// then pipecg_pass with upd = 0 (the sums; m = D w) and the step kPcReplace.  The iteration passes are pipecg's.
#include "spk_device.hpp"

namespace spk {
namespace k {

// One step of the scalar work; sums = the reduced [<r, u>, <w, u>, r.r] of the pass that ran before it.
__device__ void state_step(PipecgState *ps, int mode, const double *sums, double *hist, int32_t hist_cap)
{
    KrylovState *st = &ps->ks;
    const double g = sums[0], d = sums[1];
    const double rn = head_norm(ps, g, sums[2]);
    if (mode == kPcBnorm) {   // [<M^-1 b, b>, -, b.b]
        head_bnorm(ps, g, sums[2]);
        return;
    }
    if (mode == kPcBegin) {   // r = b - K x, u = M^-1 r: start, confirmation, restart
        head_begin(ps, g, sums[2], hist, hist_cap);
        return;
    }
    if (mode == kPcGap) {   // [||(b - K x) - r||^2, -, r.r]: the measured residual gap against tau ||r||
        // a replacement when the gap crosses tau ||r|| (van der Vorst - Ye): above now, at or below at the check before.
        // A gap that stays above is the noise floor of fl(b - K x) near the attainable accuracy, which no replacement lowers
        const int32_t above = sqrt(sums[0]) > ps->tau * sqrt(sums[2]);
        ps->rr_idle = !(above && !ps->rr_above);
        ps->rr_above = above;
        return;
    }
    if (mode == kPcReplace) {   // r, u, w, s, q, z recomputed; the scalars of the next pass as after the last iteration
        ps->rr_idle = 1;
        ps->replacements += 1;
        st->rnorm = rn;
        int reason = g < 0.0 ? SPK_DIVERGED_INDEFINITE_PC : isnan(g) ? SPK_DIVERGED_NANORINF : !(g > 0.0) ? SPK_DIVERGED_BREAKDOWN : 0;
        double beta = 0.0, den = 0.0;
        if (!reason) {
            beta = g / ps->gamma_old;
            den = d - beta * g / ps->alpha_old;
            if (isnan(den)) reason = SPK_DIVERGED_NANORINF;
            else if (!(den > 0.0)) reason = SPK_DIVERGED_INDEFINITE_MAT;   // b - K x decides, as after an iteration
        }
        if (reason) {
            ps->tent = reason == SPK_DIVERGED_INDEFINITE_MAT;
            st->reason = reason;
            st->done = 1;
            return;
        }
        ps->beta = beta;
        ps->alpha = g / den;
        ps->gamma = g;
        return;
    }
    if (mode == kPcStart) {   // w = K u: the first step length of the recurrence
        if (!(d > 0.0)) {
            st->reason = isnan(d) ? SPK_DIVERGED_NANORINF : SPK_DIVERGED_INDEFINITE_MAT;
            ps->tent = 0;
            st->done = 1;
            return;
        }
        ps->first = 1;
        ps->rr_above = 0;
        ps->alpha = g / d;
        ps->beta = 0.0;
        ps->gamma = g;
        return;
    }
    // kPcIter: the pass has applied iteration its + 1; its test, then the scalars of the next pass
    st->its += 1;
    st->rnorm = rn;
    if (st->its < hist_cap) hist[st->its] = rn;
    int reason = g < 0.0 ? SPK_DIVERGED_INDEFINITE_PC : converged_default(rn, st);
    ps->tent = 0;
    if (reason > 0) ps->tent = 1;   // the recurrence alone: b - K x confirms it
    else if (!reason && st->its >= st->max_it) {
        reason = SPK_DIVERGED_ITS;
        ps->tent = 1;
    }
    if (!reason && !(g > 0.0)) reason = isnan(g) ? SPK_DIVERGED_NANORINF : SPK_DIVERGED_BREAKDOWN;
    double beta = 0.0, den = 0.0;
    if (!reason) {
        beta = g / ps->gamma;
        den = d - beta * g / ps->alpha;
        // = <p, K p> gamma / alpha in exact arithmetic.  After the first pass of a recurrence its sign is the matrix's;
        // later the recurrences of w, s, z (and u, q) have drifted from K u, K p, K s (the residual gap of pipelined CG)
        // and the sign may flip on an SPD matrix: b - K x then decides (confirmation, or a restart that computes
        // <K u, u> afresh)
        if (isnan(den)) reason = SPK_DIVERGED_NANORINF;
        else if (!(den > 0.0)) {
            reason = SPK_DIVERGED_INDEFINITE_MAT;
            ps->tent = !ps->first;
        }
    }
    if (reason) {
        st->reason = reason;
        st->done = 1;
        return;
    }
    ps->first = 0;
    ps->alpha_old = ps->alpha;
    ps->gamma_old = ps->gamma;
    ps->beta = beta;
    ps->alpha = g / den;
    ps->gamma = g;
}

__device__ __forceinline__ double2 ldv(const double *p, int64_t i) { return reinterpret_cast<const double2 *>(p)[i]; }
__device__ __forceinline__ void stv(double *p, int64_t i, double2 v) { reinterpret_cast<double2 *>(p)[i] = v; }

// the pair (e, e + 1) of an unpadded caller vector (b): the entry past n is not read
__device__ __forceinline__ double2 ld_tail(const double *p, int64_t e, int64_t n)
{
    double2 v;
    v.x = e < n ? p[e] : 0.0;
    v.y = e + 1 < n ? p[e + 1] : 0.0;
    return v;
}

__device__ __forceinline__ double2 dscale(const double *dinv, int64_t i, double2 v)
{
    if (!dinv) return v;
    const double2 d = ldv(dinv, i);
    return double2{v.x * d.x, v.y * d.y};
}

struct BeginArgs {
    const double *b, *kx;
    double *r;
    const double *uin;   // u = M^-1 r from a launch of its own (nullptr: u = D r here)
    double *uout;        // u = D r written for the product (nullptr: not stored)
    const double *dinv;
    int sums;
    int64_t n, n2, n_dot;
    PipecgState *ps;
    Step<PipecgState> step;
    double *partials, *out;
    FinErr fe;
};

__global__ __launch_bounds__(kVT) void pipecg_begin_kernel(BeginArgs a)
{
    __shared__ double red[kVT];
    double ag = 0.0, ar = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kVT + threadIdx.x; i < a.n2; i += (int64_t)gridDim.x * kVT) {
        const int64_t e = 2 * i;
        double2 r = ld_tail(a.b, e, a.n);
        if (a.kx) {
            const double2 t = ldv(a.kx, i);
            r.x -= t.x;
            r.y -= t.y;
        }
        if (e + 1 >= a.n) r.y = 0.0;   // (the pad entry of an odd length stays zero)
        stv(a.r, i, r);
        const double2 u = a.uin ? ldv(a.uin, i) : dscale(a.dinv, i, r);
        if (a.uout) stv(a.uout, i, u);
        if (e < a.n_dot) {
            ag += r.x * u.x;
            ar += r.x * r.x;
        }
        if (e + 1 < a.n_dot) {
            ag += r.y * u.y;
            ar += r.y * r.y;
        }
    }
    if (a.sums) state_finish<3>({ag, 0.0, ar}, red, a.partials, a.out, a.fe, a.ps, a.step);
}

void pipecg_begin(const double *b, const double *kx, double *r, const double *uin, double *uout, const double *dinv, int sums,
                  int64_t n, int64_t n_dot, const PipecgState *ps, Step<PipecgState> step, const Finish &f, hipStream_t s)
{
    const int64_t n2 = (n + 1) / 2;
    BeginArgs a{b, kx, r, uin, uout, dinv, sums, n, n2, n_dot, const_cast<PipecgState *>(ps), step, f.partials, f.out,
                FinErr{f.err, f.fin_ticks}};
    hipLaunchKernelGGL(pipecg_begin_kernel, dim3(vec_grid(n2)), dim3(kVT), 0, s, a);
}

struct PassArgs {
    int upd, urec, sums;
    const double *nv;
    double *z, *s, *p, *x, *r, *w;
    double *u, *q;        // u: read (and with urec updated: u -= a q, q = m + b q); nullptr: u = D r in the pass
    const double *m;      // urec: m = M^-1 w of the product's input
    double *mout;         // m = D w written for the next product (nullptr: not stored)
    const double *dinv;
    int64_t n2, n_dot;
    PipecgState *ps;
    Step<PipecgState> step;
    double *partials, *out;
    FinErr fe;
    const int32_t *done;
};

// Every load of an element pair is issued before the arithmetic that needs it (8 streams in flight per thread on the
// Jacobi path: n, z, w, s, p, x, r, dinv).
__global__ __launch_bounds__(kVT) void pipecg_pass_kernel(PassArgs a)
{
    if (a.done && *a.done) return;
    __shared__ double red[kVT];
    double al = 0.0, be = 0.0;
    int first = 0;
    if (a.upd) {
        al = a.ps->alpha;
        be = a.ps->beta;
        first = a.ps->first;
    }
    double ag = 0.0, ad = 0.0, ar = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kVT + threadIdx.x; i < a.n2; i += (int64_t)gridDim.x * kVT) {
        const int64_t e = 2 * i;
        double2 w = ldv(a.w, i), r = ldv(a.r, i);
        double2 u;
        if (a.upd) {
            const double2 nn = ldv(a.nv, i);
            double2 x = ldv(a.x, i);
            double2 z, s, p;
            double2 dv = a.dinv ? ldv(a.dinv, i) : double2{1.0, 1.0};
            double2 uo = a.u ? ldv(a.u, i) : r;
            double2 mm{0.0, 0.0}, q{0.0, 0.0};
            if (a.urec) mm = ldv(a.m, i);
            if (first) {
                z = nn;
                s = w;
                if (a.urec) q = mm;
            } else {
                z = ldv(a.z, i);
                s = ldv(a.s, i);
                p = ldv(a.p, i);
                if (a.urec) q = ldv(a.q, i);
                z.x = nn.x + be * z.x;
                z.y = nn.y + be * z.y;
                s.x = w.x + be * s.x;
                s.y = w.y + be * s.y;
                if (a.urec) {
                    q.x = mm.x + be * q.x;
                    q.y = mm.y + be * q.y;
                }
            }
            if (!a.u && a.dinv) uo = double2{r.x * dv.x, r.y * dv.y};
            if (first) p = uo;
            else {
                p.x = uo.x + be * p.x;
                p.y = uo.y + be * p.y;
            }
            x.x += al * p.x;
            x.y += al * p.y;
            r.x -= al * s.x;
            r.y -= al * s.y;
            w.x -= al * z.x;
            w.y -= al * z.y;
            stv(a.z, i, z);
            stv(a.s, i, s);
            stv(a.p, i, p);
            stv(a.x, i, x);
            stv(a.r, i, r);
            stv(a.w, i, w);
            if (a.urec) {
                uo.x -= al * q.x;
                uo.y -= al * q.y;
                stv(a.q, i, q);
                stv(a.u, i, uo);
                u = uo;
            } else if (!a.u) {
                u = a.dinv ? double2{r.x * dv.x, r.y * dv.y} : r;
            } else {
                u = uo;   // (the step-by-step path: stale, its sums come from the next pass)
            }
            if (a.mout) stv(a.mout, i, double2{w.x * dv.x, w.y * dv.y});
        } else {
            u = a.u ? ldv(a.u, i) : dscale(a.dinv, i, r);
            if (a.mout) stv(a.mout, i, dscale(a.dinv, i, w));
        }
        if (e < a.n_dot) {
            ag += r.x * u.x;
            ad += w.x * u.x;
            ar += r.x * r.x;
        }
        if (e + 1 < a.n_dot) {
            ag += r.y * u.y;
            ad += w.y * u.y;
            ar += r.y * r.y;
        }
    }
    if (a.sums) state_finish<3>({ag, ad, ar}, red, a.partials, a.out, a.fe, a.ps, a.step);
}

void pipecg_pass(int upd, int urec, int sums, const double *nv, double *z, double *s_, double *p, double *x, double *r,
                 double *w, double *u, double *q, const double *m, double *mout, const double *dinv, int64_t n, int64_t n_dot,
                 const PipecgState *ps, Step<PipecgState> step, const Finish &f, const int32_t *done, hipStream_t s)
{
    const int64_t n2 = (n + 1) / 2;
    PassArgs a{upd, urec, sums, nv, z, s_, p, x, r, w, u, q, m, mout, dinv, n2, n_dot, const_cast<PipecgState *>(ps), step,
               f.partials, f.out, FinErr{f.err, f.fin_ticks}, done};
    hipLaunchKernelGGL(pipecg_pass_kernel, dim3(vec_grid(n2)), dim3(kVT), 0, s, a);
}

struct GapArgs {
    const double *b, *t, *r;
    int64_t n, n2, n_dot;
    PipecgState *ps;
    Step<PipecgState> step;
    double *partials, *out;
    FinErr fe;
    const int32_t *done;
};

// pipecgrr's gap check: reads b, t = K x and r once; [||(b - t) - r||^2, 0, r.r], then (one rank) the step kPcGap
__global__ __launch_bounds__(kVT) void pipecgrr_gap_kernel(GapArgs a)
{
    if (a.done && *a.done) return;
    __shared__ double red[kVT];
    double ag = 0.0, ar = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kVT + threadIdx.x; i < a.n2; i += (int64_t)gridDim.x * kVT) {
        const int64_t e = 2 * i;
        const double2 b = ld_tail(a.b, e, a.n), t = ldv(a.t, i), r = ldv(a.r, i);
        const double gx = (b.x - t.x) - r.x, gy = (b.y - t.y) - r.y;
        if (e < a.n_dot) {
            ag += gx * gx;
            ar += r.x * r.x;
        }
        if (e + 1 < a.n_dot) {
            ag += gy * gy;
            ar += r.y * r.y;
        }
    }
    state_finish<3>({ag, 0.0, ar}, red, a.partials, a.out, a.fe, a.ps, a.step);
}

void pipecgrr_gap(const double *b, const double *t, const double *r, int64_t n, int64_t n_dot, const PipecgState *ps,
                  Step<PipecgState> step, const Finish &f, const int32_t *done, hipStream_t s)
{
    const int64_t n2 = (n + 1) / 2;
    GapArgs a{b, t, r, n, n2, n_dot, const_cast<PipecgState *>(ps), step, f.partials, f.out, FinErr{f.err, f.fin_ticks},
              done};
    hipLaunchKernelGGL(pipecgrr_gap_kernel, dim3(vec_grid(n2)), dim3(kVT), 0, s, a);
}

// pipecgrr's replacement fills: r = a - t (t given) or r = a, then uout = D r
__global__ __launch_bounds__(kVT) void pipecgrr_fill_kernel(const double *a, const double *t, double *r, double *uout,
                                                            const double *dinv, int64_t n, int64_t n2, const int32_t *gate)
{
    if (*gate) return;
    for (int64_t i = (int64_t)blockIdx.x * kVT + threadIdx.x; i < n2; i += (int64_t)gridDim.x * kVT) {
        const int64_t e = 2 * i;
        double2 v = ld_tail(a, e, n);
        if (t) {
            const double2 tt = ldv(t, i);
            v.x -= tt.x;
            v.y -= tt.y;
            if (e + 1 >= n) v.y = 0.0;   // (the pad entry of an odd length stays zero)
            stv(r, i, v);
        }
        if (uout) stv(uout, i, dscale(dinv, i, v));
    }
}

void pipecgrr_fill(const double *a, const double *t, double *r, double *uout, const double *dinv, int64_t n,
                   const int32_t *gate, hipStream_t s)
{
    const int64_t n2 = (n + 1) / 2;
    hipLaunchKernelGGL(pipecgrr_fill_kernel, dim3(vec_grid(n2)), dim3(kVT), 0, s, a, t, r, uout, dinv, n, n2, gate);
}

template void state_init(PipecgState *, const spk_opts &, int, hipStream_t, double);
template void state_scalar(Step<PipecgState>, const double *, const int32_t *, hipStream_t);

}  // namespace k
}  // namespace spk
