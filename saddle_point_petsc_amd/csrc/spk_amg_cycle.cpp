// spk_amg_cycle.cpp -- the multigrid cycle: the application of a context's hierarchy (built by spk_amg_setup.cpp) as a
// launch sequence (kernels: spk_k_amg.hip).  amg_apply walks the step list of spk_host.cpp's amg_cycle_steps (V or W), a
// tail run of coarse levels as one launch where the options ask for it (amg_plan_cycle).
// -spk_mg_operator stencil (SPK_AMG_OPERATOR_STENCIL) has the cycle apply the levels between level 0 and the coarsest from
// their value arrays alone (spk_stencil_op_core.hpp): smooth(), the DOWN step and the tail descriptor dispatch on the
// level's flag, which amg_plan_cycle sets; the hierarchy is untouched.
// -spk_mg_precision single (SPK_AMG_PRECISION_SINGLE) runs the levels >= 1 of that route in FP32: their vectors are float,
// their values, D^-1, coefficients and the coarse inverse FP32 copies rounded here behind every set-up (amg_round_levels);
// level 0 and the hierarchy stay FP64, and the transfers of level 0 cross the boundary.
// Every step is deterministic: two cycles on the same hierarchy and vector give the same bytes.
#include <cstring>

#include "spk_amg_levels.hpp"
#include "spk_internal.hpp"

namespace spk {

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
            D.b32.alloc(nv, 8);
            D.ya32.alloc(nv, 16);
            D.yb32.alloc(nv, 16);
            continue;
        }
        D.b32.release(), D.ya32.release(), D.yb32.release();
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
        if (!d.single) {
            D.val32.release(), D.dinv32.release();
            continue;
        }
        if (D.val32.n != (size_t)D.A.nnz || !D.val32.p) D.val32.alloc_raw((size_t)D.A.nnz, 4);
        if (D.dinv32.n != (size_t)D.n || !D.dinv32.p) D.dinv32.alloc_raw((size_t)D.n, 4);
        k::amg_round_f32(D.A.nnz, D.A.val.p, D.val32.p, s);
        k::amg_round_f32(D.n, D.dinv.p, D.dinv32.p, s);
        D.alpha32.assign(D.alpha.begin(), D.alpha.end());   // (double -> float: round to nearest)
        D.beta32.assign(D.beta.begin(), D.beta.end());
    }
    if (!d.single) return d.cinv32.release();
    if (d.cinv32.n != d.cinv.n || !d.cinv32.p) d.cinv32.alloc_raw(d.cinv.n, 4);
    k::amg_round_f32((int64_t)d.cinv.n, d.cinv.p, d.cinv32.p, s);
    SPK_HIP(hipStreamSynchronize(s));
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
    if (t < 0 || !d.single) d.tail_desc32.release();
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
    if (d.single) {   // the tail over the float buffers: stencil levels and matrix-free transfers only (amg_check_opts)
        auto desc = std::make_unique<k::AmgTailDescF32>();
        std::memset(desc.get(), 0, sizeof *desc);
        desc->cinv = d.cinv32.p;
        desc->steps = d.tail_steps.p;
        desc->first = t;
        desc->levels = L;
        for (int l = t; l < L; ++l) {
            AmgLevelDev &D = d.lv[(size_t)l];
            k::AmgTailLevelT<float> &V = desc->lv[l];
            V.av = D.val32.p, V.dinv = D.dinv32.p;
            V.b = D.b32.p, V.ya = D.ya32.p, V.yb = D.yb32.p;
            V.n = D.n;
            V.nu = nu;
            if (l + 1 == L) continue;
            V.nc = d.lv[(size_t)l + 1].n;
            V.matrix_free = 1, V.stencil = 1;
            d.tail_stencil = true;
            std::memcpy(V.nd, D.grid.fd, sizeof V.nd);
            V.g = k::grid_args(D.grid), V.bs = D.grid.bs, V.fz = D.grid.fd[2];
            for (int q = 0; q < nu; ++q) V.alpha[q] = D.alpha32[(size_t)q], V.beta[q] = D.beta32[(size_t)q];
        }
        d.tail_desc32.upload(desc.get(), 1);
        return;
    }
    auto desc = std::make_unique<k::AmgTailDesc>();
    std::memset(desc.get(), 0, sizeof *desc);
    desc->cinv = d.cinv.p;
    desc->steps = d.tail_steps.p;
    desc->first = t;
    desc->levels = L;
    for (int l = t; l < L; ++l) {
        AmgLevelDev &D = d.lv[(size_t)l];
        k::AmgTailLevel &V = desc->lv[l];
        V.arp = D.A.rowptr.p, V.aci = D.A.colidx.p, V.av = D.A.val.p;
        V.dinv = D.dinv.p;
        V.b = D.b.p, V.ya = D.ya.p, V.yb = D.yb.p;
        V.n = D.n;
        V.nu = nu;
        if (l + 1 == L) continue;
        V.nc = d.lv[(size_t)l + 1].n;
        V.prp = D.P.rowptr.p, V.pci = D.P.colidx.p, V.pv = D.P.val.p;
        V.rrp = D.R.rowptr.p, V.rci = D.R.colidx.p, V.rv = D.R.val.p;
        V.matrix_free = D.grid.matrix_free ? 1 : 0;
        V.stencil = D.stencil_op ? 1 : 0;
        d.tail_stencil = d.tail_stencil || D.stencil_op;
        if (D.grid.on) std::memcpy(V.nd, D.grid.fd, sizeof V.nd);
        if (D.grid.on) V.g = k::grid_args(D.grid), V.bs = D.grid.bs, V.fz = D.grid.fd[2];
        for (int q = 0; q < nu; ++q) V.alpha[q] = D.alpha[(size_t)q], V.beta[q] = D.beta[(size_t)q];
    }
    d.tail_desc.upload(desc.get(), 1);
}

// the test hook of the transfers: one launch on copies of the caller's vectors
void amg_debug_transfer(spk_ctx *c, int l, int which, int stored, int64_t fine_len, const double *a, const double *b, double *out)
{
    AmgDev &d = *c->amg_d;
    if (l < 0 || l + 1 >= (int)d.lv.size()) fail(SPK_ERR_ARG, "amg: level %d has no transfer", l);
    if ((which != 0 && which != 1) || (stored != 0 && stored != 1)) fail(SPK_ERR_ARG, "amg: transfer hook: which and stored are 0 or 1");
    AmgLevelDev &D = d.lv[(size_t)l];
    const int64_t nf = D.n, nc = d.lv[(size_t)l + 1].n;
    if (fine_len < nf) fail(SPK_ERR_ARG, "amg: transfer hook: %lld entries for the %lld rows of level %d", (long long)fine_len, (long long)nf, l);
    if (!stored && !D.grid.on) fail(SPK_ERR_STATE, "amg: level %d was not built by the grid rule: it has no matrix-free transfer", l);
    hipStream_t s = c->stream;
    DevBuf<double> da, db, dout;
    const int64_t na = which == 0 ? nc : fine_len, nb = fine_len, no = which == 0 ? fine_len : nc;
    da.upload(a, (size_t)na, 16);
    db.upload(b, (size_t)nb, 16);
    if (which == 0) {   // out = y + P e, in place on the copy of y
        if (stored) k::amg_prolong_add(D.P, da.p, db.p, nullptr, s);
        else k::amg_prolong_add_grid(D.grid, da.p, db.p, nullptr, s);
        SPK_HIP(hipMemcpyAsync(out, db.p, sizeof(double) * (size_t)no, hipMemcpyDeviceToHost, s));
    } else {
        dout.alloc((size_t)no, 16);
        if (stored) k::amg_restrict(D.R, da.p, db.p, dout.p, nullptr, s);
        else k::amg_restrict_grid(D.grid, da.p, db.p, dout.p, nullptr, s);
        SPK_HIP(hipMemcpyAsync(out, dout.p, sizeof(double) * (size_t)no, hipMemcpyDeviceToHost, s));
    }
    SPK_HIP(hipStreamSynchronize(s));
}

// the test hook of the level operators: one launch of either route on copies of the caller's vectors
void amg_debug_operator(spk_ctx *c, int l, int which, int stencil, double alpha, double beta, const double *x, const double *xo,
                        const double *b, double *out)
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
    DevBuf<double> dx, dxo, db, dout;
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
    const double *yo = step && xo ? dxo.p : nullptr;
    if (stencil) k::amg_stencil_op(D.A, D.grid.fd, D.grid.bs, step ? 1 : 0, dx.p, D.dinv.p, db.p, yo, dout.p, alpha, beta, done, s);
    else if (step) k::amg_cheb_csr(D.A, D.dinv.p, db.p, dx.p, yo, dout.p, alpha, beta, done, s);
    else k::amg_spmv(D.A, dx.p, dout.p, done, s);
    SPK_HIP(hipMemcpyAsync(out, dout.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    SPK_HIP(hipStreamSynchronize(s));
    c->check_device_error();
}

// the two hooks on the FP32 kernels of SPK_AMG_PRECISION_SINGLE
static void need_single(const AmgDev &d, const char *hook)
{
    if (!d.single) fail(SPK_ERR_STATE, "amg: %s: the hierarchy was not built with -spk_mg_precision single", hook);
}
// out = y + P e on copies of e (nc entries) and y (fine_len), in place on the copy of y;  out = R (b - t)
template <typename TE, typename TY>
static void prolong32(spk_ctx *c, const AmgLevelDev &D, int64_t nc, int64_t fine_len, const void *e, const void *y, void *out)
{
    DevBuf<TE> de;
    DevBuf<TY> dy;
    de.upload(static_cast<const TE *>(e), (size_t)nc, 16);
    dy.upload(static_cast<const TY *>(y), (size_t)fine_len, 16);
    k::amg_prolong_add_grid(D.grid, de.p, dy.p, nullptr, c->stream);
    SPK_HIP(hipMemcpyAsync(out, dy.p, sizeof(TY) * (size_t)fine_len, hipMemcpyDeviceToHost, c->stream));
    SPK_HIP(hipStreamSynchronize(c->stream));
}
template <typename TI>
static void restrict32(spk_ctx *c, const AmgLevelDev &D, int64_t nc, int64_t fine_len, const void *b, const void *t, void *out)
{
    DevBuf<TI> db, dt;
    DevBuf<float> dout;
    db.upload(static_cast<const TI *>(b), (size_t)fine_len, 16);
    dt.upload(static_cast<const TI *>(t), (size_t)fine_len, 16);
    dout.alloc((size_t)nc, 16);
    k::amg_restrict_grid(D.grid, db.p, dt.p, dout.p, nullptr, c->stream);
    SPK_HIP(hipMemcpyAsync(out, dout.p, sizeof(float) * (size_t)nc, hipMemcpyDeviceToHost, c->stream));
    SPK_HIP(hipStreamSynchronize(c->stream));
}
void amg_debug_transfer_f32(spk_ctx *c, int l, int which, int64_t fine_len, const void *a, const void *b, void *out)
{
    AmgDev &d = *c->amg_d;
    need_single(d, "transfer hook");
    if (l < 0 || l + 1 >= (int)d.lv.size()) fail(SPK_ERR_ARG, "amg: level %d has no transfer", l);
    if (which != 0 && which != 1) fail(SPK_ERR_ARG, "amg: transfer hook: which is 0 or 1");
    AmgLevelDev &D = d.lv[(size_t)l];
    const int64_t nf = D.n, nc = d.lv[(size_t)l + 1].n;
    if (fine_len < nf) fail(SPK_ERR_ARG, "amg: transfer hook: %lld entries for the %lld rows of level %d", (long long)fine_len, (long long)nf, l);
    if (which == 0 && l > 0) prolong32<float, float>(c, D, nc, fine_len, a, b, out);
    else if (which == 0) prolong32<float, double>(c, D, nc, fine_len, a, b, out);
    else if (l > 0) restrict32<float>(c, D, nc, fine_len, a, b, out);
    else restrict32<double>(c, D, nc, fine_len, a, b, out);
    c->check_device_error();
}
void amg_debug_operator_f32(spk_ctx *c, int l, int which, float alpha, float beta, const float *x, const float *xo, const float *b,
                            float *out)
{
    AmgDev &d = *c->amg_d;
    need_single(d, "operator hook");
    if (l < 1 || l + 1 >= (int)d.lv.size())
        fail(SPK_ERR_ARG, "amg: operator hook: level %d is not between level 0 and the coarsest level %d", l, (int)d.lv.size() - 1);
    if (which < 0 || which > 3) fail(SPK_ERR_ARG, "amg: operator hook: which is 0..3");
    AmgLevelDev &D = d.lv[(size_t)l];
    hipStream_t s = c->stream;
    const size_t n = (size_t)D.n;
    const bool step = which & 1, gated = which >= 2;
    DevBuf<float> dx, dxo, db, dout;
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
    k::amg_stencil_op(D.n, D.val32.p, D.grid.fd, D.grid.bs, step ? 1 : 0, dx.p, D.dinv32.p, db.p, step && xo ? dxo.p : nullptr, dout.p,
                      alpha, beta, gated ? gate.p : nullptr, s);
    SPK_HIP(hipMemcpyAsync(out, dout.p, sizeof(float) * n, hipMemcpyDeviceToHost, s));
    SPK_HIP(hipStreamSynchronize(s));
    c->check_device_error();
}

// the fine level's product runs in the row-type 2x2 layout (what a_mult takes for it) on one rank
// (n_local % 2: never false here -- the 2x2 blocked copy the row types are built over exists only for an even n_local;
// the condition states what amg_cheb_dict2 needs rather than guarding a case that occurs)
static bool fused_fine(const spk_ctx *c)
{
    return c->spmv_format != 0 && c->Adict.ok && c->Adict.bs == 2 && c->n_ghost == 0 && c->n_local % 2 == 0;
}

// nu smoothing steps on level l from *y (nullptr: the zero guess); returns the buffer holding the result.  Which buffer
// that is follows the rule amg_cycle_buffers (spk_host.cpp) states for the tail kernel: each step writes the buffer its
// input is not in, the zero guess writes ya
static double *smooth(spk_ctx *c, AmgLevelDev &D, int l, const double *b, double *y, const int32_t *done)
{
    hipStream_t s = c->stream;
    const double *dinv = l == 0 ? c->dinv.p : D.dinv.p;
    const double *prev = nullptr;   // the iterate before y (nullptr: zero)
    for (size_t k = 0; k < D.alpha.size(); ++k) {
        double *dst = y == D.ya.p ? D.yb.p : D.ya.p;   // may be `prev`: each entry is read before it is written
        if (l == 0 && y && fused_fine(c)) {   // the 2x2 row-type layout: product and step in one pass
            k::amg_cheb_dict2(c->Adict, dinv, b, y, prev, dst, D.alpha[k], D.beta[k], done, s);
        } else if (l == 0) {                   // other layouts: the layout's own product, then a vector pass
            if (y) a_mult(c, y, D.t.p, nullptr, nullptr, done, false, nullptr);
            k::amg_cheb_vec(D.n, dinv, b, D.t.p, y, prev, dst, D.alpha[k], D.beta[k], done, s);
        } else if (y && D.stencil_op) {
            k::amg_stencil_op(D.A, D.grid.fd, D.grid.bs, 1, y, dinv, b, prev, dst, D.alpha[k], D.beta[k], done, s);
        } else if (y) {
            k::amg_cheb_csr(D.A, dinv, b, y, prev, dst, D.alpha[k], D.beta[k], done, s);
        } else {
            k::amg_cheb_vec(D.n, dinv, b, nullptr, nullptr, nullptr, dst, D.alpha[k], 0.0, done, s);
        }
        prev = y;
        y = dst;
    }
    return y;
}

// smooth() on a level >= 1 under SPK_AMG_PRECISION_SINGLE: every such level below the coarsest is a stencil level
static float *smooth32(spk_ctx *c, AmgLevelDev &D, float *y, const int32_t *done)
{
    hipStream_t s = c->stream;
    const float *prev = nullptr;
    for (size_t k = 0; k < D.alpha32.size(); ++k) {
        float *dst = y == D.ya32.p ? D.yb32.p : D.ya32.p;
        if (y) k::amg_stencil_op(D.n, D.val32.p, D.grid.fd, D.grid.bs, 1, y, D.dinv32.p, D.b32.p, prev, dst, D.alpha32[k], D.beta32[k], done, s);
        else k::amg_cheb_vec0(D.n, D.dinv32.p, D.b32.p, dst, D.alpha32[k], done, s);
        prev = y;
        y = dst;
    }
    return y;
}

// one step of the cycle on level l >= 1 in FP32 (amg_apply's switch on float buffers; cur: the levels' iterates)
static void step32(spk_ctx *c, AmgDev &d, int kind, size_t l, std::vector<float *> &cur, const int32_t *done)
{
    hipStream_t s = c->stream;
    AmgLevelDev &D = d.lv[l];
    switch (kind) {
    case SPK_AMG_STEP_PRE0: cur[l] = smooth32(c, D, nullptr, done); break;
    case SPK_AMG_STEP_PRE:
    case SPK_AMG_STEP_POST: cur[l] = smooth32(c, D, cur[l], done); break;
    case SPK_AMG_STEP_DOWN: {
        float *o = D.ya32.p == cur[l] ? D.yb32.p : D.ya32.p;
        k::amg_stencil_op(D.n, D.val32.p, D.grid.fd, D.grid.bs, 0, cur[l], nullptr, nullptr, nullptr, o, 0.0f, 0.0f, done, s);
        k::amg_restrict_grid(D.grid, D.b32.p, o, d.lv[l + 1].b32.p, done, s);
        break;
    }
    case SPK_AMG_STEP_COARSE:
        k::amg_dense(d.cinv32.p, D.n, D.b32.p, D.ya32.p, done, s);
        cur[l] = D.ya32.p;
        break;
    default: k::amg_prolong_add_grid(D.grid, cur[l + 1], cur[l], done, s);
    }
}

void amg_apply(spk_ctx *c, const double *x, double *y, int mode, const int32_t *done, const double **last)
{
    hipStream_t s = c->stream;
    AmgDev &d = *c->amg_d;
    const size_t L = d.lv.size();
    std::vector<double *> cur(L, nullptr);
    std::vector<float *> cur32(d.single ? L : 0, nullptr);   // SPK_AMG_PRECISION_SINGLE: the iterates of the levels >= 1
    auto rhs = [&](size_t l) -> const double * { return l == 0 ? x : d.lv[l].b.p; };
    size_t run = 0;
    for (size_t i = 0; i < d.steps.size(); ++i) {   // the cycle's steps in order (amg_cycle_steps); under V: down, coarse, up
        if (run < d.runs.size() && (size_t)d.runs[run].first == i) {   // a tail run: one launch of one workgroup
            const size_t t = (size_t)d.info.tail_first;
            if (d.single) {
                k::amg_tail(d.tail_desc32.p, (int32_t)d.runs[run].first, (int32_t)d.runs[run].second, done, s);
                cur32[t] = d.run_sel[run] ? d.lv[t].yb32.p : d.lv[t].ya32.p;
            } else {
                k::amg_tail(d.tail_desc.p, d.tail_stencil, (int32_t)d.runs[run].first, (int32_t)d.runs[run].second, done, s);
                cur[t] = d.run_sel[run] ? d.lv[t].yb.p : d.lv[t].ya.p;
            }
            i = (size_t)d.runs[run++].second - 1;
            continue;
        }
        const size_t l = (size_t)d.steps[i].level;
        AmgLevelDev &D = d.lv[l];
        if (d.single && l > 0) {
            step32(c, d, d.steps[i].kind, l, cur32, done);
            continue;
        }
        switch (d.steps[i].kind) {
        case SPK_AMG_STEP_PRE0: cur[l] = smooth(c, D, (int)l, rhs(l), nullptr, done); break;
        case SPK_AMG_STEP_PRE:
        case SPK_AMG_STEP_POST: cur[l] = smooth(c, D, (int)l, rhs(l), cur[l], done); break;
        case SPK_AMG_STEP_DOWN: {   // residual, restriction
            if (l == 0) a_mult(c, cur[l], D.t.p, nullptr, nullptr, done, false, nullptr);
            double *o = D.ya.p == cur[l] ? D.yb.p : D.ya.p;
            if (l > 0 && D.stencil_op) k::amg_stencil_op(D.A, D.grid.fd, D.grid.bs, 0, cur[l], nullptr, nullptr, nullptr, o, 0.0, 0.0, done, s);
            else if (l > 0) k::amg_spmv(D.A, cur[l], o, done, s);
            const double *t = l == 0 ? D.t.p : o;
            if (d.single) k::amg_restrict_grid(D.grid, rhs(l), t, d.lv[l + 1].b32.p, done, s);   // (level 0: FP64 sums, one rounding on the store)
            else if (D.grid.matrix_free) k::amg_restrict_grid(D.grid, rhs(l), t, d.lv[l + 1].b.p, done, s);
            else k::amg_restrict(D.R, rhs(l), t, d.lv[l + 1].b.p, done, s);
            break;
        }
        case SPK_AMG_STEP_COARSE:   // exact coarse solve
            k::amg_dense(d.cinv.p, D.n, rhs(l), D.ya.p, done, s);
            cur[l] = D.ya.p;
            break;
        default:   // SPK_AMG_STEP_UP: prolongation + correction
            if (d.single) k::amg_prolong_add_grid(D.grid, cur32[l + 1], cur[l], done, s);   // (level 0: e widened, FP64 sums)
            else if (D.grid.matrix_free) k::amg_prolong_add_grid(D.grid, cur[l + 1], cur[l], done, s);
            else k::amg_prolong_add(D.P, cur[l + 1], cur[l], done, s);
        }
    }
    if (last) *last = cur[0];   // the caller's own pass reads the iterate where it lies
    else k::amg_out(mode, c->n_local, cur[0], y, done, s);
}

}  // namespace spk
