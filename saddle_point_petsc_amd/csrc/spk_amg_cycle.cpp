// spk_amg_cycle.cpp -- the multigrid cycle: the application of a context's hierarchy (built by spk_amg_setup.cpp) as a
// launch sequence (kernels: spk_k_amg.hip).  amg_apply walks the step list of spk_host.cpp's amg_cycle_steps (V or W), a
// tail run of coarse levels as one launch where the options ask for it (amg_plan_cycle).
// -spk_mg_operator stencil (SPK_AMG_OPERATOR_STENCIL) has the cycle apply the levels between level 0 and the coarsest from
// their value arrays alone (spk_stencil_op_core.hpp): smooth(), the DOWN step and the tail descriptor dispatch on the
// level's flag, which amg_plan_cycle sets; the hierarchy is untouched.
// -spk_mg_precision single (SPK_AMG_PRECISION_SINGLE) runs the levels >= 1 of that route in FP32: their vectors are float,
// their values, D^-1, coefficients and the coarse inverse FP32 copies rounded here behind every set-up (amg_round_levels);
// level 0 and the hierarchy stay FP64, and the transfers of level 0 cross the boundary.  The walk, the tail's descriptor
// and the test hooks are written once over the scalar type T of a level's vectors: AmgLevelDev::view<T>() gives what a
// level holds in T.  The CSR operators and the stored transfers exist in FP64 alone (amg_check_opts plans no other), so
// their branches stand under `if constexpr`.
// Every step is deterministic: two cycles on the same hierarchy and vector give the same bytes.
#include <cstring>

#include "spk_amg_levels.hpp"
#include "spk_internal.hpp"

namespace spk {

template <typename T>
constexpr bool is_f64 = std::is_same<T, double>::value;

// the V-cycle's vectors; level 0 takes the context's padded length, as the layouts' products want them.  Both callers
// pass c->ld, the device build even before pc_setup's own ensure_vectors: every set_block ends in ensure_vectors and
// nothing else changes n_local or m, so c->ld is current whenever the context holds an operator (pc_setup asks for one).
// single: the vectors of the levels >= 1 are float (and the double ones are released: a set-up under reuse may change it)
void alloc_cycle_vectors(AmgDev &d, int64_t ld, bool single)
{
    const size_t L = d.lv.size();
    d.single = single;
    for (size_t l = 0; l < L; ++l) {
        AmgLevelDev &D = d.lv[l];
        const size_t nv = l == 0 ? (size_t)ld : (size_t)D.n;
        if (l > 0 && single) {
            D.b.release(), D.ya.release(), D.yb.release();
            D.f32.b.alloc(nv, 8);
            D.f32.ya.alloc(nv, 16);
            D.f32.yb.alloc(nv, 16);
            continue;
        }
        D.f32.b.release(), D.f32.ya.release(), D.f32.yb.release();
        if (l > 0) D.b.alloc(nv, 8);
        D.ya.alloc(nv, 16);
        D.yb.alloc(nv, 16);
        if (l == 0 && L > 1) D.t.alloc(nv, 16);
    }
}

// The FP32 copies of SPK_AMG_PRECISION_SINGLE, behind every build and every refresh: each value of the levels >= 1, each
// entry of their D^-1 (the FP64 D^-1 rounded, not recomputed), each smoothing coefficient and each entry of the coarse
// inverse rounded to nearest once.  Without the option the copies are released.
static void amg_round_levels(AmgDev &d, hipStream_t s)
{
    const size_t L = d.lv.size();
    for (size_t l = 1; l < L; ++l) {
        AmgLevelDev &D = d.lv[l];
        AmgLevelDev::F32 &F = D.f32;
        if (!d.single) {
            F.val.release(), F.dinv.release();
            continue;
        }
        if (F.val.n != (size_t)D.A.nnz || !F.val.p) F.val.alloc_raw((size_t)D.A.nnz, 4);
        if (F.dinv.n != (size_t)D.n || !F.dinv.p) F.dinv.alloc_raw((size_t)D.n, 4);
        k::amg_round_f32(D.A.nnz, D.A.val.p, F.val.p, s);
        k::amg_round_f32(D.n, D.dinv.p, F.dinv.p, s);
        F.alpha.assign(D.alpha.begin(), D.alpha.end());   // (double -> float: round to nearest)
        F.beta.assign(D.beta.begin(), D.beta.end());
    }
    if (!d.single) return d.f32.cinv.release();
    if (d.f32.cinv.n != d.cinv.n || !d.f32.cinv.p) d.f32.cinv.alloc_raw(d.cinv.n, 4);
    k::amg_round_f32((int64_t)d.cinv.n, d.cinv.p, d.f32.cinv.p, s);
    SPK_HIP(hipStreamSynchronize(s));
}

// the tail kernel's descriptor over the levels >= t in T.  float: the tail over the float buffers -- stencil levels and
// matrix-free transfers only (amg_check_opts), the index arrays are not read
template <typename T>
static void fill_tail_desc(AmgDev &d, int t, int nu)
{
    const int L = (int)d.lv.size();
    auto desc = std::make_unique<k::AmgTailDescT<T>>();
    std::memset(desc.get(), 0, sizeof *desc);
    desc->cinv = d.coarse_inv<T>().p;
    desc->steps = d.tail_steps.p;
    desc->first = t;
    desc->levels = L;
    for (int l = t; l < L; ++l) {
        AmgLevelDev &D = d.lv[(size_t)l];
        const AmgLevelView<T> W = D.view<T>();
        k::AmgTailLevelT<T> &V = desc->lv[l];
        if constexpr (is_f64<T>) V.arp = D.A.rowptr.p, V.aci = D.A.colidx.p;
        V.av = W.val, V.dinv = W.dinv;
        V.b = W.b, V.ya = W.ya, V.yb = W.yb;
        V.n = D.n;
        V.nu = nu;
        if (l + 1 == L) continue;
        V.nc = d.lv[(size_t)l + 1].n;
        V.matrix_free = V.stencil = 1;
        if constexpr (is_f64<T>) {
            V.prp = D.P.rowptr.p, V.pci = D.P.colidx.p, V.pv = D.P.val.p;
            V.rrp = D.R.rowptr.p, V.rci = D.R.colidx.p, V.rv = D.R.val.p;
            V.matrix_free = D.grid.matrix_free ? 1 : 0;
            V.stencil = D.stencil_op ? 1 : 0;
        }
        d.tail_stencil = d.tail_stencil || V.stencil;
        if (D.grid.on) std::memcpy(V.nd, D.grid.fd, sizeof V.nd);
        if (D.grid.on) V.g = k::grid_args(D.grid), V.bs = D.grid.bs, V.fz = D.grid.fd[2];
        for (int q = 0; q < nu; ++q) V.alpha[q] = W.alpha[(size_t)q], V.beta[q] = W.beta[(size_t)q];
    }
    d.tail<T>().upload(desc.get(), 1);
}

// The application's plan, rebuilt at every set-up (build or refresh) from the options and the levels as they are now:
// the steps of the cycle, the tail runs, and -- where there is a tail -- the kernel's descriptor and step list on the
// device: the pointers, the smoothing coefficients and, per step, the buffer that holds the iterate (amg_cycle_buffers).
void amg_plan_cycle(AmgDev &d, const spk_amg_opts &o, int64_t ld, hipStream_t s)
{
    if ((o.precision == SPK_AMG_PRECISION_SINGLE) != d.single) alloc_cycle_vectors(d, ld, !d.single);   // (a refresh that toggles it)
    amg_round_levels(d, s);
    fill_cycle_info(o, d.info);
    d.info.precision = d.single ? SPK_AMG_PRECISION_SINGLE : SPK_AMG_PRECISION_DOUBLE;
    const int L = (int)d.lv.size(), t = d.info.tail_first, nu = o.smooth_its;
    // (amg_check_opts: the option comes with grid coarsening and the stencil products, so these levels have the closed form)
    for (int l = 0; l < L; ++l) d.lv[(size_t)l].stencil_op = o.op == SPK_AMG_OPERATOR_STENCIL && l >= 1 && l + 1 < L;
    d.steps = amg_cycle_steps(L, o.cycle);
    d.runs = amg_tail_runs(d.steps, t);
    d.run_sel.assign(d.runs.size(), 0);
    d.tsteps.clear();
    d.tail_stencil = false;
    if (t < 0 || d.single) d.tail_desc.release();
    if (t < 0 || !d.single) d.f32.tail_desc.release();
    if (t < 0) {
        d.tail_steps.release();
        return;
    }
    if (d.steps.size() > (size_t)INT32_MAX) fail(SPK_ERR_UNSUPPORTED, "amg: the cycle has more steps than 32 bits count");
    d.tsteps.resize(d.steps.size());
    AmgBuffers buf = amg_cycle_buffers(d.steps, d.runs, L, nu, t);
    for (size_t i = 0; i < d.steps.size(); ++i) d.tsteps[i] = k::AmgTailStep{d.steps[i].kind, d.steps[i].level, buf.sel[i], buf.sel_next[i]};
    d.run_sel = std::move(buf.run_sel);
    d.tail_steps.upload(d.tsteps.data(), d.tsteps.size());
    if (d.single) fill_tail_desc<float>(d, t, nu);
    else fill_tail_desc<double>(d, t, nu);
}

// the FP32 hooks run the kernels of SPK_AMG_PRECISION_SINGLE on the copies it made
static void need_single(const AmgDev &d, const char *hook)
{
    if (!d.single) fail(SPK_ERR_STATE, "amg: %s: the hierarchy was not built with -spk_mg_precision single", hook);
}

// the test hook of the transfers: one launch on copies of the caller's vectors, TF the scalar type on the fine side of the
// transfer and TC on the coarse side.  which 0: out = y + P e on copies of e (nc entries) and y (fine_len), in place on
// the copy of y;  which 1: out = R (b - t)
template <typename TF, typename TC>
static void debug_transfer(spk_ctx *c, int l, int which, int stored, int64_t fine_len, const void *a, const void *b, void *out)
{
    AmgDev &d = *c->amg_d;
    if (l < 0 || l + 1 >= (int)d.lv.size()) fail(SPK_ERR_ARG, "amg: level %d has no transfer", l);
    if ((which != 0 && which != 1) || (stored != 0 && stored != 1)) fail(SPK_ERR_ARG, "amg: transfer hook: which and stored are 0 or 1");
    AmgLevelDev &D = d.lv[(size_t)l];
    const int64_t nf = D.n, nc = d.lv[(size_t)l + 1].n;
    if (fine_len < nf) fail(SPK_ERR_ARG, "amg: transfer hook: %lld entries for the %lld rows of level %d", (long long)fine_len, (long long)nf, l);
    if (!stored && !D.grid.on) fail(SPK_ERR_STATE, "amg: level %d was not built by the grid rule: it has no matrix-free transfer", l);
    hipStream_t s = c->stream;
    DevBuf<TF> fa, fb;   // the copies of a and b where they are fine vectors
    DevBuf<TC> co;       // the coarse vector: the copy of a (e), or the restriction's result
    fb.upload(static_cast<const TF *>(b), (size_t)fine_len, 16);
    if (which == 0) {    // a: e, b: y
        co.upload(static_cast<const TC *>(a), (size_t)nc, 16);
        if (!stored) k::amg_prolong_add_grid(D.grid, co.p, fb.p, nullptr, s);
        else if constexpr (is_f64<TC>) k::amg_prolong_add(D.P, co.p, fb.p, nullptr, s);
        SPK_HIP(hipMemcpyAsync(out, fb.p, sizeof(TF) * (size_t)fine_len, hipMemcpyDeviceToHost, s));
    } else {             // a: b, b: t
        fa.upload(static_cast<const TF *>(a), (size_t)fine_len, 16);
        co.alloc((size_t)nc, 16);
        if (!stored) k::amg_restrict_grid(D.grid, fa.p, fb.p, co.p, nullptr, s);
        else if constexpr (is_f64<TC>) k::amg_restrict(D.R, fa.p, fb.p, co.p, nullptr, s);
        SPK_HIP(hipMemcpyAsync(out, co.p, sizeof(TC) * (size_t)nc, hipMemcpyDeviceToHost, s));
    }
    SPK_HIP(hipStreamSynchronize(s));
}
void amg_debug_transfer(spk_ctx *c, int l, int which, int stored, int64_t fine_len, const double *a, const double *b, double *out)
{
    debug_transfer<double, double>(c, l, which, stored, fine_len, a, b, out);
}
void amg_debug_transfer_f32(spk_ctx *c, int l, int which, int64_t fine_len, const void *a, const void *b, void *out)
{
    need_single(*c->amg_d, "transfer hook");
    if (l > 0) debug_transfer<float, float>(c, l, which, 0, fine_len, a, b, out);
    else debug_transfer<double, float>(c, l, which, 0, fine_len, a, b, out);   // the boundary: level 0 is FP64
    c->check_device_error();
}

// the test hook of the level operators: one launch of either route on copies of the caller's vectors
template <typename T>
static void debug_operator(spk_ctx *c, int l, int which, int stencil, T alpha, T beta, const T *x, const T *xo, const T *b, T *out)
{
    AmgDev &d = *c->amg_d;
    if (l < 1 || l + 1 >= (int)d.lv.size())
        fail(SPK_ERR_ARG, "amg: operator hook: level %d is not between level 0 and the coarsest level %d", l, (int)d.lv.size() - 1);
    if (which < 0 || which > 3 || (stencil != 0 && stencil != 1)) fail(SPK_ERR_ARG, "amg: operator hook: which is 0..3, stencil 0 or 1");
    AmgLevelDev &D = d.lv[(size_t)l];
    if (stencil && !(d.info.coarsening == SPK_AMG_COARSEN_GRID && d.info.galerkin == SPK_AMG_GALERKIN_STENCIL && D.grid.on))
        fail(SPK_ERR_STATE, "amg: level %d was not built by -spk_mg_galerkin stencil: its pattern is no closed form", l);
    hipStream_t s = c->stream;
    const size_t n = (size_t)D.n;
    const bool step = which & 1, gated = which >= 2;
    DevBuf<T> dx, dxo, db, dout;
    DevBuf<int32_t> gate;
    dx.upload(x, n, 16);
    if (step) db.upload(b, n, 16);
    if (step && xo) dxo.upload(xo, n, 16);
    if (gated) {
        const int32_t one = 1;
        gate.upload(&one, 1);
        dout.upload(out, n, 16);
    } else {
        dout.alloc(n, 16);
    }
    const int32_t *done = gated ? gate.p : nullptr;
    const T *yo = step && xo ? dxo.p : nullptr;
    const AmgLevelView<T> V = D.view<T>();
    if (stencil) k::amg_stencil_op(D.n, V.val, D.grid.fd, D.grid.bs, step ? 1 : 0, dx.p, V.dinv, db.p, yo, dout.p, alpha, beta, done, s);
    else if constexpr (is_f64<T>) {
        if (step) k::amg_cheb_csr(D.A, V.dinv, db.p, dx.p, yo, dout.p, alpha, beta, done, s);
        else k::amg_spmv(D.A, dx.p, dout.p, done, s);
    }
    SPK_HIP(hipMemcpyAsync(out, dout.p, sizeof(T) * n, hipMemcpyDeviceToHost, s));
    SPK_HIP(hipStreamSynchronize(s));
    c->check_device_error();
}
void amg_debug_operator(spk_ctx *c, int l, int which, int stencil, double alpha, double beta, const double *x, const double *xo,
                        const double *b, double *out)
{
    debug_operator<double>(c, l, which, stencil, alpha, beta, x, xo, b, out);
}
void amg_debug_operator_f32(spk_ctx *c, int l, int which, float alpha, float beta, const float *x, const float *xo, const float *b,
                            float *out)
{
    need_single(*c->amg_d, "operator hook");
    debug_operator<float>(c, l, which, 1, alpha, beta, x, xo, b, out);   // (the FP32 levels are stencil levels)
}

// the fine level's product runs in the row-type 2x2 layout (what a_mult takes for it) on one rank
// (n_local % 2: never false here -- the 2x2 blocked copy the row types are built over exists only for an even n_local;
// the condition states what amg_cheb_dict2 needs rather than guarding a case that occurs)
static bool fused_fine(const spk_ctx *c)
{
    return c->spmv_format != 0 && c->Adict.ok && c->Adict.bs == 2 && c->n_ghost == 0 && c->n_local % 2 == 0;
}

// one smoothing step on level 0, FP64 on every route: from y (nullptr: the zero guess) and the iterate before it into dst
static void smooth_fine(spk_ctx *c, AmgLevelDev &D, const double *b, const double *y, const double *prev, double *dst, double alpha,
                        double beta, const int32_t *done)
{
    if (y && fused_fine(c)) {   // the 2x2 row-type layout: product and step in one pass
        k::amg_cheb_dict2(c->Adict, c->dinv.p, b, y, prev, dst, alpha, beta, done, c->stream);
    } else {                    // other layouts: the layout's own product, then a vector pass
        if (y) a_mult(c, y, D.t.p, nullptr, nullptr, done, false, nullptr);
        k::amg_cheb_vec(D.n, c->dinv.p, b, D.t.p, y, prev, dst, alpha, beta, done, c->stream);
    }
}

// nu smoothing steps on level l, whose vectors are T, from *y (nullptr: the zero guess); returns the buffer holding the
// result.  Which buffer that is follows the rule amg_cycle_buffers (spk_host.cpp) states for the tail kernel: each step
// writes the buffer its input is not in, the zero guess writes ya
template <typename T>
static T *smooth(spk_ctx *c, AmgLevelDev &D, size_t l, const T *b, T *y, const int32_t *done)
{
    hipStream_t s = c->stream;
    const AmgLevelView<T> V = D.view<T>();
    const T *prev = nullptr;   // the iterate before y (nullptr: zero)
    for (size_t k = 0; k < V.alpha.size(); ++k) {
        T *dst = y == V.ya ? V.yb : V.ya;   // may be `prev`: each entry is read before it is written
        if (l == 0) {
            if constexpr (is_f64<T>) smooth_fine(c, D, b, y, prev, dst, V.alpha[k], V.beta[k], done);
        } else if (y && D.stencil_op) {
            k::amg_stencil_op(D.n, V.val, D.grid.fd, D.grid.bs, 1, y, V.dinv, b, prev, dst, V.alpha[k], V.beta[k], done, s);
        } else if (y) {
            if constexpr (is_f64<T>) k::amg_cheb_csr(D.A, V.dinv, b, y, prev, dst, V.alpha[k], V.beta[k], done, s);
        } else {
            k::amg_cheb_vec(D.n, V.dinv, b, nullptr, nullptr, nullptr, dst, V.alpha[k], T(0), done, s);
        }
        prev = y;
        y = dst;
    }
    return y;
}

// One step of the cycle on level st.level, whose vectors are T and those of the level below it TN (level 0 under
// SPK_AMG_PRECISION_SINGLE: double and float, so that its DOWN rounds once on the store -- FP64 sums -- and its UP widens
// e and adds in FP64; the overloads of the grid transfers resolve it).  b: the level's right-hand side, y: its iterate,
// yn: the iterate of the level below
template <typename T, typename TN>
static void step(spk_ctx *c, AmgDev &d, const AmgStep &st, const T *b, T *&y, const TN *yn, const int32_t *done)
{
    hipStream_t s = c->stream;
    const size_t l = (size_t)st.level;
    AmgLevelDev &D = d.lv[l];
    const AmgLevelView<T> V = D.view<T>();
    switch (st.kind) {
    case SPK_AMG_STEP_PRE0: y = smooth<T>(c, D, l, b, nullptr, done); break;
    case SPK_AMG_STEP_PRE:
    case SPK_AMG_STEP_POST: y = smooth<T>(c, D, l, b, y, done); break;
    case SPK_AMG_STEP_DOWN: {   // residual, restriction
        T *t = V.ya == y ? V.yb : V.ya;   // A y: in the buffer y is not in; level 0 has one of its own
        if (l == 0) {
            if constexpr (is_f64<T>) a_mult(c, y, t = D.t.p, nullptr, nullptr, done, false, nullptr);
        } else if (D.stencil_op) {
            k::amg_stencil_op(D.n, V.val, D.grid.fd, D.grid.bs, 0, y, nullptr, nullptr, nullptr, t, T(0), T(0), done, s);
        } else if constexpr (is_f64<T>) {
            k::amg_spmv(D.A, y, t, done, s);
        }
        TN *bn = d.lv[l + 1].view<TN>().b;
        if (D.grid.matrix_free) k::amg_restrict_grid(D.grid, b, t, bn, done, s);
        else if constexpr (is_f64<TN>) k::amg_restrict(D.R, b, t, bn, done, s);
        break;
    }
    case SPK_AMG_STEP_COARSE:   // exact coarse solve
        k::amg_dense(d.coarse_inv<T>().p, D.n, b, V.ya, done, s);
        y = V.ya;
        break;
    default:   // SPK_AMG_STEP_UP: prolongation + correction
        if (D.grid.matrix_free) k::amg_prolong_add_grid(D.grid, yn, y, done, s);
        else if constexpr (is_f64<TN>) k::amg_prolong_add(D.P, yn, y, done, s);
    }
}

// the cycle's steps in order (amg_cycle_steps; under V: down, coarse, up) with the levels >= 1 in T; returns the buffer of
// level 0 that holds the result
template <typename T>
static const double *walk(spk_ctx *c, AmgDev &d, const double *x, const int32_t *done)
{
    const size_t L = d.lv.size();
    double *y0 = nullptr;
    std::vector<T *> cur(L + 1, nullptr);   // the iterates of the levels >= 1 ([L]: below the coarsest, none)
    size_t run = 0;
    for (size_t i = 0; i < d.steps.size(); ++i) {
        if (run < d.runs.size() && (size_t)d.runs[run].first == i) {   // a tail run: one launch of one workgroup
            const size_t t = (size_t)d.info.tail_first;
            const AmgLevelView<T> V = d.lv[t].view<T>();
            k::amg_tail(d.tail<T>().p, d.tail_stencil, (int32_t)d.runs[run].first, (int32_t)d.runs[run].second, done, c->stream);
            cur[t] = d.run_sel[run] ? V.yb : V.ya;
            i = (size_t)d.runs[run++].second - 1;
            continue;
        }
        const size_t l = (size_t)d.steps[i].level;
        if (l == 0) step<double, T>(c, d, d.steps[i], x, y0, cur[1], done);
        else step<T, T>(c, d, d.steps[i], d.lv[l].view<T>().b, cur[l], cur[l + 1], done);
    }
    return y0;
}

void amg_apply(spk_ctx *c, const double *x, double *y, int mode, const int32_t *done, const double **last)
{
    AmgDev &d = *c->amg_d;
    const double *v = d.single ? walk<float>(c, d, x, done) : walk<double>(c, d, x, done);
    if (last) *last = v;   // the caller's own pass reads the iterate where it lies
    else k::amg_out(mode, c->n_local, v, y, done, c->stream);
}

}  // namespace spk
