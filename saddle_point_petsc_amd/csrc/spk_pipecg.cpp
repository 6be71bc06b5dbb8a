// spk_pipecg.cpp -- device-resident preconditioned pipelined CG (spk_pipecg, include/spk.h), K = A only.
//
// The host only ENQUEUES iterations, each gated by the state's `done` word, and looks at the state (copied into pinned
// memory behind an event) once per chunk of iterations while the next chunk is already queued.  The scalar recurrence
// runs on the device (spk_k_pipecg.hip).  A convergence or -ksp_max_it seen by the recurrence ends the chunk loop; the
// true residual b - K x then confirms it (kPcBegin), or restarts the recurrence from the current x.
// spk_pipecgrr runs the same loop and adds, at every chunk boundary, the gap check t = K x, ||(b - t) - r|| > tau ||r||,
// and the replacement it may ask for (r, u, w, s, q, z from their definitions; x, p and the scalars' history kept), all
// enqueued behind the chunk and gated on the device: the host never waits for the verdict.
#include <algorithm>
#include <chrono>
#include <cstring>

#include "spk_internal.hpp"

namespace spk {

namespace {
constexpr int kPcVecs = 11;   // n, z, s, p, x, r, w, m, u, q, K x
constexpr int kPcChunk = 16;  // iterations per look at the state when opts.check_every = 0

// rr: pipecgrr with tau (the gap check and the replacement); nullptr: pipecg
void run(spk_ctx *c, const double *b, double *x, const spk_opts &o, int norm, spk_result *res, double *history,
         int32_t history_cap, const double *rr, int32_t *replacements)
{
    const char *who = rr ? "pipecgrr" : "pipecg";
    require_setup(c, who);
    if (norm != SPK_NORM_UNPRECONDITIONED && norm != SPK_NORM_NATURAL) fail(SPK_ERR_ARG, "%s: unknown norm type %d", who, norm);
    if (c->m > 0)
        fail(SPK_ERR_UNSUPPORTED, "%s is for K = A (symmetric positive definite); the saddle matrix [A B^T; B 0] is "
             "indefinite -- use -ksp_type minres (spk_minres) or fgmres", who);
    if (c->pc_type == SPK_PC_SCHUR)
        fail(SPK_ERR_UNSUPPORTED, "%s takes the preconditioners none, Jacobi and gamg; the Schur fieldsplit needs a "
             "constraint block -- use -ksp_type minres or fgmres", who);
    if (c->inner_sweeps > 0 && c->pc_type != SPK_PC_NONE)
        fail(SPK_ERR_UNSUPPORTED, "%s needs a symmetric preconditioner: the FP32 inner sweeps are not -- call "
             "spk_pc_set_inner(ctx, 0, omega) before spk_pc_setup, or use -ksp_type fgmres", who);
    c->ensure_scratch();
    c->ensure_vectors();
    hipStream_t s = c->stream;
    const int64_t ld = c->ld, N = c->n_local, n_dot = N;   // m = 0: no multiplier rows
    if (c->pc_ld != ld) {
        c->pc_vec.alloc((size_t)ld * kPcVecs);   // zero-filled: the pad entries stay zero
        c->pc_ld = ld;
    }
    const int32_t hist_cap = (int32_t)std::min<int64_t>((int64_t)std::max(o.max_it, 0) + 2, 1 << 22);
    if (c->pc_hist.n < (size_t)hist_cap) c->pc_hist.alloc((size_t)hist_cap);
    if (!c->pc_out.p) c->pc_out.alloc(8);
    if (!c->pc_st.p) c->pc_st.alloc(1);
    if (!c->pc_pin) SPK_HIP(hipHostMalloc(&c->pc_pin, 2 * sizeof(PipecgState), hipHostMallocDefault));
    for (hipEvent_t &e : c->pc_ev)
        if (!e) SPK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));

    double *vec = c->pc_vec.p;
    auto vv = [&](int i) { return vec + (size_t)ld * i; };
    double *Nv = vv(0), *Z = vv(1), *S = vv(2), *P = vv(3), *X = vv(4), *R = vv(5), *W = vv(6), *M = vv(7), *U = vv(8),
           *Q = vv(9), *T = vv(10);
    PipecgState *ps = c->pc_st.p;
    double *out = c->pc_out.p, *hist = c->pc_hist.p;
    const int32_t *done = &ps->ks.done;
    const bool one = c->comm->size() == 1;
    // gamg: m = V-cycle(w) through op_pc_apply, u and q recurrences.  Step-by-step (fused = 0, none / Jacobi): M^-1 as
    // launches of its own (m = M^-1 w, u = M^-1 r), the sums in a pass after them.  Otherwise u = D r, q = D s in the pass
    const bool gamg = c->amg_d && c->pc_type == SPK_PC_JACOBI;
    const bool diag = !gamg && o.fused != 0;
    const double *dinv = c->pc_type == SPK_PC_NONE ? nullptr : c->dinv.p;
    const k::Finish f = c->fin(out);
    const k::Finish fg = c->fin(out + 4);   // pipecgrr's gap sums

    // one rank: the scalar step runs in the finishing workgroup of the pass; several: after the all-reduce of its sums
    auto step = [&](int mode) { return k::PcStep{ps, one ? mode : -1, hist, hist_cap}; };
    auto after = [&](int mode, const int32_t *gate, double *sums = nullptr) {
        if (one) return;
        if (!sums) sums = out;
        c->comm->allreduce_sum(sums, 3, s);
        k::pipecg_scalar(k::PcStep{ps, mode, hist, hist_cap}, sums, gate, s);
    };
    // r = b - K x (kx: K x, nullptr: x = 0), u = M^-1 r, the sums [<r, u>, -, r.r] and the step `mode`.  Diagonal M:
    // u into M for the product w = K u that follows (none: the product reads r)
    auto begin = [&](const double *bb, const double *kx, int mode) {
        if (diag) {
            k::pipecg_begin(bb, kx, R, nullptr, dinv ? M : nullptr, dinv, 1, N, n_dot, ps, step(mode), f, s);
        } else {
            k::pipecg_begin(bb, kx, R, nullptr, nullptr, nullptr, 0, N, n_dot, ps, k::PcStep{ps, -1, hist, hist_cap}, f, s);
            op_pc_apply(c, R, U, nullptr);
            k::pipecg_begin(R, nullptr, R, U, nullptr, nullptr, 1, N, n_dot, ps, step(mode), f, s);
        }
        after(mode, nullptr);
    };
    const double *u_in = diag ? (dinv ? M : R) : U;   // the product's input at a start: u
    const double *m_in = diag && !dinv ? W : M;       // the product's input in an iteration: m = M^-1 w

    SPK_HIP(hipStreamSynchronize(s));
    const auto t0 = std::chrono::steady_clock::now();

    PipecgState *pin = (PipecgState *)c->pc_pin;
    auto report = [&](int slot) {
        SPK_HIP(hipMemcpyAsync(pin + slot, ps, sizeof(PipecgState), hipMemcpyDeviceToHost, s));
        SPK_HIP(hipEventRecord(c->pc_ev[slot], s));
    };
    auto look = [&](int slot) {
        SPK_HIP(hipEventSynchronize(c->pc_ev[slot]));
        return pin[slot];
    };

    k::pipecg_init(ps, o, norm, s, rr ? *rr : 0.0);
    if (o.guess_nonzero) begin(b, nullptr, k::kPcBnorm);   // ||b|| in the norm of the test: the reference of rtol
    const double *kx = nullptr;
    if (!o.guess_nonzero) {
        SPK_HIP(hipMemsetAsync(X, 0, sizeof(double) * (size_t)ld, s));
    } else {
        SPK_HIP(hipMemcpyAsync(X, x, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, s));
        op_mult(c, X, T, nullptr);
        kx = T;
    }
    PipecgState st{};
    for (;;) {
        // ---- (re)start: r = b - K x, u = M^-1 r, the test on the true residual ----
        begin(b, kx, k::kPcBegin);
        report(0);
        st = look(0);
        if (st.ks.done) break;
        // w = K u, delta = <w, u> (and m = D w): the first step length
        op_mult(c, u_in, W, done);
        k::pipecg_pass(0, 0, 1, nullptr, Z, S, P, X, R, W, diag ? nullptr : U, nullptr, nullptr, diag && dinv ? M : nullptr,
                       dinv, N, n_dot, ps, step(k::kPcStart), f, done, s);
        after(k::kPcStart, done);
        const int64_t cap = (int64_t)o.max_it - st.ks.its;   // iterations this recurrence may run
        const int64_t chunk = o.check_every > 0 ? o.check_every : kPcChunk;
        int64_t pending = -1;
        bool seen_done = false, owed = false;   // owed: the collective of the last pass (several ranks) is still to come
        for (int64_t j = 1; j <= cap && !seen_done; ++j) {
            if (!diag) op_pc_apply(c, W, M, done);   // m = M^-1 w
            op_mult(c, m_in, Nv, done);              // n = K m
            // several ranks: the collective of the previous pass goes behind this product, which needs only m
            if (owed) after(k::kPcIter, done);
            if (gamg) {
                k::pipecg_pass(1, 1, 1, Nv, Z, S, P, X, R, W, U, Q, M, nullptr, nullptr, N, n_dot, ps, step(k::kPcIter), f,
                               done, s);
            } else if (diag) {
                k::pipecg_pass(1, 0, 1, Nv, Z, S, P, X, R, W, nullptr, nullptr, nullptr, dinv ? M : nullptr, dinv, N, n_dot,
                               ps, step(k::kPcIter), f, done, s);
            } else {   // the updates with u as stored, u = M^-1 r, then the sums of the same pass shape
                k::pipecg_pass(1, 0, 0, Nv, Z, S, P, X, R, W, U, nullptr, nullptr, nullptr, dinv, N, n_dot, ps,
                               k::PcStep{ps, -1, hist, hist_cap}, f, done, s);
                op_pc_apply(c, R, U, done);
                k::pipecg_pass(0, 0, 1, nullptr, Z, S, P, X, R, W, U, nullptr, nullptr, nullptr, dinv, N, n_dot, ps,
                               step(k::kPcIter), f, done, s);
            }
            owed = true;
            if (rr && j % chunk == 0 && j < cap) {
                // ---- pipecgrr: the gap check; several ranks: the pass's collective goes behind the check product ----
                op_mult(c, X, T, done);   // t = K x
                after(k::kPcIter, done);
                owed = false;
                k::pipecgrr_gap(b, T, R, N, n_dot, ps, step(k::kPcGap), fg, done, s);
                after(k::kPcGap, done, out + 4);
                // ---- the replacement, gated by rr_idle: x, p, alpha_old, gamma_old are kept ----
                const int32_t *idle = &ps->rr_idle;
                if (diag) {
                    k::pipecgrr_fill(b, T, R, dinv ? U : nullptr, dinv, N, idle, s);   // r = b - t, u = D r
                    op_mult(c, dinv ? U : R, W, idle);                                 // w = K u
                    op_mult(c, P, S, idle);                                            // s = K p
                    if (dinv) k::pipecgrr_fill(S, nullptr, nullptr, Q, dinv, N, idle, s);   // q = D s
                    op_mult(c, dinv ? Q : S, Z, idle);                                 // z = K q
                    // [<r, u>, <w, u>, r.r], m = D w for the next product
                    k::pipecg_pass(0, 0, 1, nullptr, Z, S, P, X, R, W, nullptr, nullptr, nullptr, dinv ? M : nullptr, dinv,
                                   N, n_dot, ps, step(k::kPcReplace), f, idle, s);
                } else {   // the V-cycle, or the step-by-step path: u = M^-1 r and q = M^-1 s as launches of their own
                    k::pipecgrr_fill(b, T, R, nullptr, nullptr, N, idle, s);   // r = b - t
                    op_pc_apply(c, R, U, idle);
                    op_mult(c, U, W, idle);
                    op_mult(c, P, S, idle);
                    op_pc_apply(c, S, Q, idle);
                    op_mult(c, Q, Z, idle);
                    k::pipecg_pass(0, 0, 1, nullptr, Z, S, P, X, R, W, U, nullptr, nullptr, nullptr, dinv, N, n_dot, ps,
                                   step(k::kPcReplace), f, idle, s);
                }
                after(k::kPcReplace, idle);
            }
            if (j % chunk == 0 || j == cap) {
                const int slot = (int)((j / chunk) & 1);
                report(slot);
                if (o.check_every > 0) {
                    seen_done = look(slot).ks.done != 0;
                } else {   // the previous chunk's verdict, read while this one runs
                    if (pending >= 0) seen_done = look((int)pending).ks.done != 0;
                    pending = slot;
                }
            }
        }
        if (owed) after(k::kPcIter, done);   // the last pass's collective (several ranks)
        // ---- confirmation on b - K x (kPcBegin above: converged, -ksp_max_it, or a restart) ----
        op_mult(c, X, T, nullptr);
        kx = T;
        SPK_HIP(hipGetLastError());
    }
    SPK_HIP(hipMemcpyAsync(x, X, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, s));
    finish_solve(c, st.ks, st.starts, t0, hist, hist_cap, res, history, history_cap);
    if (replacements) *replacements = st.replacements;
}
}  // namespace

void pipecg(spk_ctx *c, const double *b, double *x, const spk_opts &o, int norm, spk_result *res, double *history,
            int32_t history_cap)
{
    run(c, b, x, o, norm, res, history, history_cap, nullptr, nullptr);
}

void pipecgrr(spk_ctx *c, const double *b, double *x, const spk_opts &o, int norm, double tau, spk_result *res,
              double *history, int32_t history_cap, int32_t *replacements)
{
    run(c, b, x, o, norm, res, history, history_cap, &tau, replacements);
}

}  // namespace spk
