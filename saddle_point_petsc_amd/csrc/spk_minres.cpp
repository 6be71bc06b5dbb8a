// spk_minres.cpp -- device-resident preconditioned MINRES (spk_minres, include/spk.h).
//
// The frame (enqueued iterations, the state read-back once per chunk) is SolverFrame (spk_internal.hpp); the scalar
// recurrence runs on the device (spk_k_minres.hip).  A convergence or -ksp_max_it seen by the recurrence ends the chunk
// loop; the true residual b - K x then confirms it (kMrBegin), or restarts the recurrence from the current x.
#include "spk_internal.hpp"

namespace spk {

namespace {
constexpr int kMrVecs = 12;   // v x2, z x2, p x2, w x2, K w x2, r, K x
constexpr int kMrChunk = 16;  // iterations per look at the state when opts.check_every = 0
}

void minres(spk_ctx *c, const double *b, double *x, const spk_opts &o, int norm, spk_result *res, double *history,
            int32_t history_cap)
{
    require_setup(c, "minres");
    if (c->pc_type == SPK_PC_SCHUR && c->schur_fact != SPK_SCHUR_DIAG)
        fail(SPK_ERR_UNSUPPORTED, "minres needs a symmetric positive definite preconditioner: the Schur %s factorisation is not "
             "symmetric -- use -pc_fieldsplit_schur_fact_type diag (SPK_SCHUR_DIAG), or -ksp_type fgmres",
             c->schur_fact == SPK_SCHUR_LOWER ? "lower" : c->schur_fact == SPK_SCHUR_UPPER ? "upper" : "full");
    if (c->amg_d && c->pc_type != SPK_PC_NONE)
        fail(SPK_ERR_UNSUPPORTED, "minres with the multigrid preconditioner (gamg) is not implemented -- call "
             "spk_pc_set_amg(ctx, NULL) before spk_pc_setup, or use -ksp_type fgmres");
    if (c->inner_sweeps > 0 && c->pc_type != SPK_PC_NONE)
        fail(SPK_ERR_UNSUPPORTED, "minres needs a symmetric preconditioner: the FP32 inner sweeps are not -- call "
             "spk_pc_set_inner(ctx, 0, omega) before spk_pc_setup (drop -fieldsplit_0_ksp_type richardson), or use -ksp_type fgmres");
    SolverFrame<MinresState> F(c, c->minres_work, kMrVecs, 2, o, kMrChunk);
    hipStream_t s = c->stream;
    const int64_t ld = c->ld, nl = c->n_local, N = nl + c->m;
    const int64_t n_dot = nl + (c->comm->rank() == 0 ? c->m : 0);   // the multipliers count on rank 0 only
    double *V[2] = {F.vec(0), F.vec(1)}, *Zb[2] = {F.vec(2), F.vec(3)}, *Pb[2] = {F.vec(4), F.vec(5)},
           *W[2] = {F.vec(6), F.vec(7)}, *KW[2] = {F.vec(8), F.vec(9)}, *R = F.vec(10), *T = F.vec(11);
    MinresState *ms = F.st;
    const int32_t *done = F.done();
    const bool unprec = norm == SPK_NORM_UNPRECONDITIONED;
    const bool fused = o.fused != 0 && !c->schur_dense;   // a dense S: the preconditioner as a step of its own
    const double *dinv = c->pc_type == SPK_PC_NONE ? nullptr : c->dinv.p;
    const double *shat = c->pc_type == SPK_PC_SCHUR ? c->shat.p : nullptr;
    const k::Finish f = c->fin(F.out);
    // vm = v (resid: p - vj), z = M^-1 v and the sums [<z, v>, v.v] -- PC in the pass, or (opts.fused = 0) as its own step
    auto pass_v = [&](int resid, const double *p, const double *vj, double *vm, double *r2, double *z, int sq, int mode,
                      const int32_t *gate) {
        if (fused) {
            k::minres_vz(p, vj, vm, r2, z, dinv, shat, nl, N, n_dot, resid, sq, ms, F.step(mode), f, gate, s);
        } else {
            k::minres_vz(p, vj, vm, r2, nullptr, dinv, shat, nl, N, n_dot, resid, 0, ms, F.step(-1), f, gate, s);
            op_pc_apply(c, vm, z, gate);
            k::minres_wd(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, z, vm, sq, N, n_dot, ms,
                         F.step(mode), f, gate, s);
        }
        F.after(mode, gate);
    };

    k::state_init(ms, o, norm, s);
    if (o.guess_nonzero)   // ||b|| in the norm of the test: the reference of rtol with a nonzero guess
        pass_v(1, b, nullptr, R, nullptr, Zb[0], 1, k::kMrBnorm, nullptr);
    const double *kx = nullptr;
    if (!o.guess_nonzero) {
        SPK_HIP(hipMemsetAsync(x, 0, sizeof(double) * (size_t)N, s));
    } else {
        op_mult(c, x, T, nullptr);
        kx = T;
    }
    MinresState st{};
    for (;;) {
        // ---- (re)start: r = b - K x into v_1 (and r), z_1 = M^-1 r, the test on the true residual ----
        for (double *p : {V[0], W[0], W[1], KW[0], KW[1]}) SPK_HIP(hipMemsetAsync(p, 0, sizeof(double) * (size_t)ld, s));
        pass_v(1, b, kx, V[1], unprec ? R : nullptr, Zb[0], 1, k::kMrBegin, nullptr);
        st = F.start();
        if (st.ks.done) break;
        const int64_t cap = (int64_t)o.max_it - st.ks.its;   // iterations this recurrence may run
        int64_t j = 1;
        bool seen_done = false;
        for (; j <= cap && !seen_done; ++j) {
            const int a = (int)(j & 1), bq = 1 - a;   // z_j = Zb[bq], v_j = V[a], p_j = Pb[a], w_{j-1} = W[bq]
            op_mult(c, Zb[bq], Pb[a], done);
            // the update of iteration j-1 (w_j into w_{j-2}'s place) + <p_j, z_j>, then delta_j
            k::minres_wd(j > 1, Zb[a], Pb[bq], W[a], W[bq], x, unprec ? KW[a] : nullptr, KW[bq], R, Pb[a], Zb[bq], 0, N, n_dot,
                         ms, F.step(k::kMrDelta), f, done, s);
            F.after(k::kMrDelta, done);
            // v_{j+1} into v_{j-1}'s place, z_{j+1}, <z_{j+1}, v_{j+1}>, then the recurrence
            pass_v(0, Pb[a], V[a], V[bq], nullptr, Zb[a], 0, k::kMrRecur, done);
            seen_done = F.chunk_end(j, cap);
        }
        // the update of the recurrence's last iteration has no next pass to ride in (gated off when the solve stopped)
        {
            const int64_t jl = j - 1;
            const int a = (int)(jl & 1), bq = 1 - a;
            k::minres_wd(1, Zb[bq], Pb[a], W[bq], W[a], x, unprec ? KW[bq] : nullptr, KW[a], R, nullptr, nullptr, 0, N, n_dot,
                         ms, F.step(k::kMrTest), f, done, s);
            F.after(k::kMrTest, done);
        }
        // ---- confirmation on b - K x (kMrBegin above: converged, -ksp_max_it, or a restart) ----
        op_mult(c, x, T, nullptr);
        kx = T;
        SPK_HIP(hipGetLastError());
    }
    F.finish(st, res, history, history_cap);
}

}  // namespace spk
