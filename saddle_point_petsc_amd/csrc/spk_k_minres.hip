// spk_k_minres.hip -- the vector passes and the scalar recurrence of the device-resident preconditioned MINRES
// (spk_minres; Paige-Saunders, Elman-Silvester-Wathen Alg. 4.1).  M^-1 is diagonal for every preconditioner MINRES
// accepts (none, Jacobi, Schur DIAG), so it is applied inside the pass that forms the vector it acts on.
// Per iteration j (z_j is never scaled in memory: every consumer applies 1 / gamma_j to its scalars):
//   product       p_j = K z_j                                          (the product kernels, unchanged)
//   minres_wd     lagged update of iteration j-1 + <p_j, z_j>           finisher: convergence test of j-1, delta_j
//   minres_vz     v_{j+1}, z_{j+1} = M^-1 v_{j+1}, <z_{j+1}, v_{j+1}>   finisher: gamma_{j+1}, Givens, w / x coefficients
// Summation orders are fixed (block partials + the sentinel finish of spk_device.hpp): identical solves, identical bits.
#include "spk_device.hpp"

namespace spk {
namespace k {

// One step of the scalar work; sums = the reduced [<.,.>, ||.||^2] of the pass that ran before it.
__device__ void state_step(MinresState *ms, int mode, const double *sums, double *hist, int32_t hist_cap)
{
    KrylovState *st = &ms->ks;
    const bool natural = ms->norm == SPK_NORM_NATURAL;
    if (mode == kMrBnorm) {   // [<M^-1 b, b>, b.b]
        head_bnorm(ms, sums[0], sums[1]);
        return;
    }
    if (mode == kMrBegin) {   // [<z, r>, r.r] of r = b - K x: start, confirmation, restart
        if (!head_begin(ms, sums[0], sums[1], hist, hist_cap)) return;
        ms->first = 1;
        ms->pend = 0;
        ms->gam = sqrt(sums[0]);
        ms->gam_prev = 1.0;
        ms->eta = ms->gam;
        ms->c0 = ms->c1 = 1.0;
        ms->s0 = ms->s1 = 0.0;
        return;
    }
    if (mode == kMrDelta || mode == kMrTest) {
        // the update of the previous iteration has been applied (kMrTest: only that): its convergence test
        if (!ms->first || mode == kMrTest) {
            const double rn = natural ? fabs(ms->eta) : sqrt(sums[1]);
            st->its += 1;
            st->rnorm = rn;
            if (st->its < hist_cap) hist[st->its] = rn;
            int reason = converged_default(rn, st);
            ms->tent = 0;
            if (ms->pend) reason = ms->pend;
            else if (reason > 0) ms->tent = 1;   // the recurrence alone: b - K x confirms it
            else if (!reason && st->its >= st->max_it) {
                reason = SPK_DIVERGED_ITS;
                ms->tent = 1;
            }
            if (reason) {
                st->reason = reason;
                st->done = 1;
                return;
            }
        }
        if (mode == kMrDelta) {   // delta_j = <K z, z> with z = z_j / gamma_j
            const double g = ms->gam;
            ms->delta = sums[0] / (g * g);
            ms->vz_ig = 1.0 / g;
            ms->vz_dg = ms->delta / g;
            ms->vz_gg = ms->first ? 0.0 : g / ms->gam_prev;
        }
        return;
    }
    // kMrRecur: [<z_{j+1}, v_{j+1}>]: gamma_{j+1}, the Givens rotation, the coefficients of the lagged update
    const double zv = sums[0];
    if (zv < 0.0 || isnan(zv)) {
        st->reason = zv < 0.0 ? SPK_DIVERGED_INDEFINITE_PC : SPK_DIVERGED_NANORINF;
        ms->tent = 0;
        st->done = 1;
        return;
    }
    const double gn = sqrt(zv), g = ms->gam, d = ms->delta;
    const double a0 = ms->c1 * d - ms->c0 * ms->s1 * g;
    const double a1 = sqrt(a0 * a0 + gn * gn);
    const double a2 = ms->s1 * d + ms->c0 * ms->c1 * g;
    const double a3 = ms->s0 * g;
    if (!(a1 > 0.0)) {
        st->reason = isnan(a1) ? SPK_DIVERGED_NANORINF : SPK_DIVERGED_BREAKDOWN;
        ms->tent = 0;
        st->done = 1;
        return;
    }
    const double cn = a0 / a1, sn = gn / a1;
    ms->wx_ig = 1.0 / g;
    ms->wx_a2 = a2;
    ms->wx_a3 = a3;
    ms->wx_ia1 = 1.0 / a1;
    ms->wx_cx = cn * ms->eta;
    ms->eta = -sn * ms->eta;
    ms->c0 = ms->c1;
    ms->c1 = cn;
    ms->s0 = ms->s1;
    ms->s1 = sn;
    ms->gam_prev = g;
    ms->gam = gn;
    ms->first = 0;
    if (gn == 0.0) ms->pend = SPK_CONVERGED_HAPPY_BREAKDOWN;   // applied after the pending update
}

// M^-1 of element e (e < nl: the (0,0) block, else a multiplier)
__device__ __forceinline__ double mr_pc(int64_t e, double v, int64_t nl, const double *dinv, const double *shat)
{
    if (e < nl) return dinv ? v * dinv[e] : v;
    return shat ? v / shat[e - nl] : v;
}

struct VzArgs {
    const double *p, *vj;
    double *vm, *r2, *z;
    const double *dinv, *shat;
    int64_t nl, n, n2, n_dot;
    int resid, sq;
    MinresState *ms;
    Step<MinresState> step;
    double *partials, *out;
    FinErr fe;
    const int32_t *done;
};

__global__ __launch_bounds__(kVT) void minres_vz_kernel(VzArgs a)
{
    if (a.done && *a.done) return;
    __shared__ double red[kVT];
    double ig = 0.0, dg = 0.0, gg = 0.0;
    if (!a.resid) {
        ig = a.ms->vz_ig;
        dg = a.ms->vz_dg;
        gg = a.ms->vz_gg;
    }
    double acc0 = 0.0, acc1 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kVT + threadIdx.x; i < a.n2; i += (int64_t)gridDim.x * kVT) {
        const double2 pv = reinterpret_cast<const double2 *>(a.p)[i];
        double2 v;
        if (a.resid) {
            v = pv;
            if (a.vj) {
                const double2 kx = reinterpret_cast<const double2 *>(a.vj)[i];
                v.x -= kx.x;
                v.y -= kx.y;
            }
        } else {
            const double2 vj = reinterpret_cast<const double2 *>(a.vj)[i];
            const double2 vm = reinterpret_cast<const double2 *>(a.vm)[i];
            v.x = ig * pv.x - dg * vj.x - gg * vm.x;
            v.y = ig * pv.y - dg * vj.y - gg * vm.y;
        }
        const int64_t e = 2 * i;
        if (e >= a.n) v.x = 0.0;      // (the pad entry of an odd length stays zero)
        if (e + 1 >= a.n) v.y = 0.0;
        reinterpret_cast<double2 *>(a.vm)[i] = v;
        if (a.r2) reinterpret_cast<double2 *>(a.r2)[i] = v;
        if (a.z) {
            double2 zz;
            zz.x = e < a.n ? mr_pc(e, v.x, a.nl, a.dinv, a.shat) : 0.0;
            zz.y = e + 1 < a.n ? mr_pc(e + 1, v.y, a.nl, a.dinv, a.shat) : 0.0;
            reinterpret_cast<double2 *>(a.z)[i] = zz;
            if (e < a.n_dot) acc0 += zz.x * v.x;
            if (e + 1 < a.n_dot) acc0 += zz.y * v.y;
        }
        if (a.sq) {
            if (e < a.n_dot) acc1 += v.x * v.x;
            if (e + 1 < a.n_dot) acc1 += v.y * v.y;
        }
    }
    state_finish<2>({acc0, acc1}, red, a.partials, a.out, a.fe, a.ms, a.step);
}

void minres_vz(const double *p, const double *vj, double *vm, double *r2, double *z, const double *dinv, const double *shat,
               int64_t nl, int64_t n, int64_t n_dot, int resid, int sq, const MinresState *ms, Step<MinresState> step,
               const Finish &f, const int32_t *done, hipStream_t s)
{
    const int64_t n2 = (n + 1) / 2;
    VzArgs a{p, vj, vm, r2, z, dinv, shat, nl, n, n2, n_dot, resid, sq, const_cast<MinresState *>(ms), step,
             f.partials, f.out, FinErr{f.err, f.fin_ticks}, done};
    hipLaunchKernelGGL(minres_vz_kernel, dim3(vec_grid(n2)), dim3(kVT), 0, s, a);
}

struct WdArgs {
    int wx;
    const double *zp, *pp;
    double *wm;
    const double *w;
    double *x, *kwm;
    const double *kw;
    double *r;
    const double *da, *db;
    int sq;
    int64_t n2, n_dot;
    MinresState *ms;
    Step<MinresState> step;
    double *partials, *out;
    FinErr fe;
    const int32_t *done;
};

__global__ __launch_bounds__(kVT) void minres_wd_kernel(WdArgs a)
{
    if (a.done && *a.done) return;
    __shared__ double red[kVT];
    double ig = 0.0, a2 = 0.0, a3 = 0.0, ia1 = 0.0, cx = 0.0;
    if (a.wx) {
        ig = a.ms->wx_ig;
        a2 = a.ms->wx_a2;
        a3 = a.ms->wx_a3;
        ia1 = a.ms->wx_ia1;
        cx = a.ms->wx_cx;
    }
    double acc0 = 0.0, acc1 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kVT + threadIdx.x; i < a.n2; i += (int64_t)gridDim.x * kVT) {
        const int64_t e = 2 * i;
        if (a.wx) {
            const double2 z = reinterpret_cast<const double2 *>(a.zp)[i];
            const double2 wm = reinterpret_cast<const double2 *>(a.wm)[i];
            const double2 w = reinterpret_cast<const double2 *>(a.w)[i];
            double2 wn, x = reinterpret_cast<const double2 *>(a.x)[i];
            wn.x = (ig * z.x - a3 * wm.x - a2 * w.x) * ia1;
            wn.y = (ig * z.y - a3 * wm.y - a2 * w.y) * ia1;
            reinterpret_cast<double2 *>(a.wm)[i] = wn;
            x.x += cx * wn.x;
            x.y += cx * wn.y;
            reinterpret_cast<double2 *>(a.x)[i] = x;
            if (a.kwm) {
                const double2 p = reinterpret_cast<const double2 *>(a.pp)[i];
                const double2 km = reinterpret_cast<const double2 *>(a.kwm)[i];
                const double2 k = reinterpret_cast<const double2 *>(a.kw)[i];
                double2 kn, r = reinterpret_cast<const double2 *>(a.r)[i];
                kn.x = (ig * p.x - a3 * km.x - a2 * k.x) * ia1;
                kn.y = (ig * p.y - a3 * km.y - a2 * k.y) * ia1;
                reinterpret_cast<double2 *>(a.kwm)[i] = kn;
                r.x -= cx * kn.x;
                r.y -= cx * kn.y;
                reinterpret_cast<double2 *>(a.r)[i] = r;
                if (e < a.n_dot) acc1 += r.x * r.x;
                if (e + 1 < a.n_dot) acc1 += r.y * r.y;
            }
        }
        if (a.da) {
            const double2 u = reinterpret_cast<const double2 *>(a.da)[i];
            const double2 v = reinterpret_cast<const double2 *>(a.db)[i];
            if (e < a.n_dot) acc0 += u.x * v.x;
            if (e + 1 < a.n_dot) acc0 += u.y * v.y;
            if (a.sq) {
                if (e < a.n_dot) acc1 += v.x * v.x;
                if (e + 1 < a.n_dot) acc1 += v.y * v.y;
            }
        }
    }
    state_finish<2>({acc0, acc1}, red, a.partials, a.out, a.fe, a.ms, a.step);
}

void minres_wd(int wx, const double *zp, const double *pp, double *wm, const double *w, double *x, double *kwm,
               const double *kw, double *r, const double *da, const double *db, int sq, int64_t n, int64_t n_dot,
               const MinresState *ms, Step<MinresState> step, const Finish &f, const int32_t *done, hipStream_t s)
{
    const int64_t n2 = (n + 1) / 2;
    WdArgs a{wx, zp, pp, wm, w, x, kwm, kw, r, da, db, sq, n2, n_dot, const_cast<MinresState *>(ms), step,
             f.partials, f.out, FinErr{f.err, f.fin_ticks}, done};
    hipLaunchKernelGGL(minres_wd_kernel, dim3(vec_grid(n2)), dim3(kVT), 0, s, a);
}

template void state_init(MinresState *, const spk_opts &, int, hipStream_t);
template void state_scalar(Step<MinresState>, const double *, const int32_t *, hipStream_t);

}  // namespace k
}  // namespace spk
