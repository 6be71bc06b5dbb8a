// spk_pipecg.cpp -- device-resident preconditioned pipelined CG (spk_pipecg, include/spk.h), K = A only.
//
// The frame (enqueued iterations, the state read-back once per chunk) is SolverFrame (spk_internal.hpp); the scalar
// recurrence runs on the device (spk_k_pipecg.hip).  A convergence or -ksp_max_it seen by the recurrence ends the chunk
// loop; the true residual b - K x then confirms it (kPcBegin), or restarts the recurrence from the current x.
// spk_pipecgrr runs the same loop and adds, at every chunk boundary, the gap check t = K x, ||(b - t) - r|| > tau ||r||,
// and the replacement it may ask for (r, u, w, s, q, z from their definitions; x, p and the scalars' history kept), all
// enqueued behind the chunk and gated on the device: the host never waits for the verdict.
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
    if (c->m > 0)
        fail(SPK_ERR_UNSUPPORTED, "%s is for K = A (symmetric positive definite); the saddle matrix [A B^T; B 0] is "
             "indefinite -- use -ksp_type minres (spk_minres) or fgmres", who);
    if (c->pc_type == SPK_PC_SCHUR)
        fail(SPK_ERR_UNSUPPORTED, "%s takes the preconditioners none, Jacobi and gamg; the Schur fieldsplit needs a "
             "constraint block -- use -ksp_type minres or fgmres", who);
    if (c->inner_sweeps > 0 && c->pc_type != SPK_PC_NONE)
        fail(SPK_ERR_UNSUPPORTED, "%s needs a symmetric preconditioner: the FP32 inner sweeps are not -- call "
             "spk_pc_set_inner(ctx, 0, omega) before spk_pc_setup, or use -ksp_type fgmres", who);
    if (c->amg_d && c->amg_d->single && c->pc_type == SPK_PC_JACOBI)
        fail(SPK_ERR_UNSUPPORTED, "%s needs a symmetric preconditioner: the multigrid cycle of -spk_mg_precision single, rounded to "
             "FP32 on its levels >= 1, is not exactly one -- use -ksp_type fgmres (spk_fgmres), or -spk_mg_precision double", who);
    SolverFrame<PipecgState> F(c, c->pipecg_work, kPcVecs, 3, o, kPcChunk);   // vectors zero-filled: the pad entries stay zero
    hipStream_t s = c->stream;
    const int64_t ld = c->ld, N = c->n_local, n_dot = N;   // m = 0: no multiplier rows
    double *Nv = F.vec(0), *Z = F.vec(1), *S = F.vec(2), *P = F.vec(3), *X = F.vec(4), *R = F.vec(5), *W = F.vec(6),
           *M = F.vec(7), *U = F.vec(8), *Q = F.vec(9), *T = F.vec(10);
    PipecgState *ps = F.st;
    const int32_t *done = F.done();
    // gamg: m = V-cycle(w) through op_pc_apply, u and q recurrences.  Step-by-step (fused = 0, none / Jacobi): M^-1 as
    // launches of its own (m = M^-1 w, u = M^-1 r), the sums in a pass after them.  Otherwise u = D r, q = D s in the pass
    const bool gamg = c->amg_d && c->pc_type == SPK_PC_JACOBI;
    const bool diag = !gamg && o.fused != 0;
    const double *dinv = c->pc_type == SPK_PC_NONE ? nullptr : c->dinv.p;
    const k::Finish f = c->fin(F.out);
    const k::Finish fg = c->fin(F.out + 4);   // pipecgrr's gap sums
    // r = b - K x (kx: K x, nullptr: x = 0), u = M^-1 r, the sums [<r, u>, -, r.r] and the step `mode`.  Diagonal M:
    // u into M for the product w = K u that follows (none: the product reads r)
    auto begin = [&](const double *bb, const double *kx, int mode) {
        if (diag) {
            k::pipecg_begin(bb, kx, R, nullptr, dinv ? M : nullptr, dinv, 1, N, n_dot, ps, F.step(mode), f, s);
        } else {
            k::pipecg_begin(bb, kx, R, nullptr, nullptr, nullptr, 0, N, n_dot, ps, F.step(-1), f, s);
            op_pc_apply(c, R, U, nullptr);
            k::pipecg_begin(R, nullptr, R, U, nullptr, nullptr, 1, N, n_dot, ps, F.step(mode), f, s);
        }
        F.after(mode, nullptr);
    };
    const double *u_in = diag ? (dinv ? M : R) : U;   // the product's input at a start: u
    const double *m_in = diag && !dinv ? W : M;       // the product's input in an iteration: m = M^-1 w

    k::state_init(ps, o, norm, s, rr ? *rr : 0.0);
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
        st = F.start();
        if (st.ks.done) break;
        // w = K u, delta = <w, u> (and m = D w): the first step length
        op_mult(c, u_in, W, done);
        k::pipecg_pass(0, 0, 1, nullptr, Z, S, P, X, R, W, diag ? nullptr : U, nullptr, nullptr, diag && dinv ? M : nullptr,
                       dinv, N, n_dot, ps, F.step(k::kPcStart), f, done, s);
        F.after(k::kPcStart, done);
        const int64_t cap = (int64_t)o.max_it - st.ks.its;   // iterations this recurrence may run
        bool seen_done = false, owed = false;   // owed: the collective of the last pass (several ranks) is still to come
        for (int64_t j = 1; j <= cap && !seen_done; ++j) {
            if (!diag) op_pc_apply(c, W, M, done);   // m = M^-1 w
            op_mult(c, m_in, Nv, done);              // n = K m
            // several ranks: the collective of the previous pass goes behind this product, which needs only m
            if (owed) F.after(k::kPcIter, done);
            if (gamg) {
                k::pipecg_pass(1, 1, 1, Nv, Z, S, P, X, R, W, U, Q, M, nullptr, nullptr, N, n_dot, ps, F.step(k::kPcIter),
                               f, done, s);
            } else if (diag) {
                k::pipecg_pass(1, 0, 1, Nv, Z, S, P, X, R, W, nullptr, nullptr, nullptr, dinv ? M : nullptr, dinv, N, n_dot,
                               ps, F.step(k::kPcIter), f, done, s);
            } else {   // the updates with u as stored, u = M^-1 r, then the sums of the same pass shape
                k::pipecg_pass(1, 0, 0, Nv, Z, S, P, X, R, W, U, nullptr, nullptr, nullptr, dinv, N, n_dot, ps, F.step(-1), f,
                               done, s);
                op_pc_apply(c, R, U, done);
                k::pipecg_pass(0, 0, 1, nullptr, Z, S, P, X, R, W, U, nullptr, nullptr, nullptr, dinv, N, n_dot, ps,
                               F.step(k::kPcIter), f, done, s);
            }
            owed = true;
            if (rr && j % F.chunk == 0 && j < cap) {
                // ---- pipecgrr: the gap check; several ranks: the pass's collective goes behind the check product ----
                op_mult(c, X, T, done);   // t = K x
                F.after(k::kPcIter, done);
                owed = false;
                k::pipecgrr_gap(b, T, R, N, n_dot, ps, F.step(k::kPcGap), fg, done, s);
                F.after(k::kPcGap, done, F.out + 4);
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
                                   N, n_dot, ps, F.step(k::kPcReplace), f, idle, s);
                } else {   // the V-cycle, or the step-by-step path: u = M^-1 r and q = M^-1 s as launches of their own
                    k::pipecgrr_fill(b, T, R, nullptr, nullptr, N, idle, s);   // r = b - t
                    op_pc_apply(c, R, U, idle);
                    op_mult(c, U, W, idle);
                    op_mult(c, P, S, idle);
                    op_pc_apply(c, S, Q, idle);
                    op_mult(c, Q, Z, idle);
                    k::pipecg_pass(0, 0, 1, nullptr, Z, S, P, X, R, W, U, nullptr, nullptr, nullptr, dinv, N, n_dot, ps,
                                   F.step(k::kPcReplace), f, idle, s);
                }
                F.after(k::kPcReplace, idle);
            }
            seen_done = F.chunk_end(j, cap);
        }
        if (owed) F.after(k::kPcIter, done);   // the last pass's collective (several ranks)
        // ---- confirmation on b - K x (kPcBegin above: converged, -ksp_max_it, or a restart) ----
        op_mult(c, X, T, nullptr);
        kx = T;
        SPK_HIP(hipGetLastError());
    }
    SPK_HIP(hipMemcpyAsync(x, X, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, s));
    F.finish(st, res, history, history_cap);
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
