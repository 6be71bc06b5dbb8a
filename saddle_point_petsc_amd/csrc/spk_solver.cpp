// spk_solver.cpp -- applying the operator and the preconditioner, and the device-resident FGMRES
// (their set-up: spk_operator.cpp).
//
// Replaces what executes below KSPSolve(ksp, f, *u) at
// /root/reference/src/SaddlePointProblem.c:70 when the reference is run with
// -ksp_type fgmres -pc_type fieldsplit -pc_fieldsplit_type schur ... (options
// read at :67): PETSc's KSPSolve_FGMRES drives the loop from the host and waits
// on every dot product; here the host only ENQUEUES a whole restart cycle on
// one HIP stream.  The Hessenberg column, the Givens rotations, the convergence
// test and the back substitution run in single-wave kernels on the device, and
// every kernel of an iteration starts with "if (*done) return", so the iterate
// is exactly the one a stop-at-convergence loop would produce while the host
// looks at the state only once per cycle (or every opts.check_every
// iterations).  Inner products across ranks go through Comm::allreduce_sum on
// the same stream (RCCL), never through the host.
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "spk_internal.hpp"

using namespace spk;

void spk_ctx::ensure_scratch()
{
    if (!partials.p) {
        partials.alloc((size_t)k::kMaxBlocks * k::kPartialLd);
        k::arm_partials(partials.p, partials.n, stream);
        SPK_HIP(hipStreamSynchronize(stream));
    }
    if (!errw.p) errw.alloc(4);
    if (!small.p) small.alloc(512);
    if (!y1tmp.p) y1tmp.alloc(64);
    if (!ttmp.p) ttmp.alloc(64);
}

void spk_ctx::check_device_error()
{
    if (!errw.p) return;
    int32_t e = 0;
    SPK_HIP(hipMemcpy(&e, errw.p, sizeof e, hipMemcpyDeviceToHost));
    if (!e) return;
    // the word is sticky on the device; clear it and put every slot of the partials buffer back to the
    // sentinel (a workgroup that publishes late would otherwise leave a stale "arrived" slot behind)
    SPK_HIP(hipStreamSynchronize(stream));
    SPK_HIP(hipMemset(errw.p, 0, sizeof(int32_t)));
    k::arm_partials(partials.p, partials.n, stream);
    if (gs_tot.p) k::arm_partials(gs_tot.p, gs_tot.n, stream);
    SPK_HIP(hipStreamSynchronize(stream));
    fail(SPK_ERR_HIP, "a cross-workgroup reduction timed out on the device (a workgroup never published its partial "
                      "sums within %.1f s): execution failure, the result of this call is not valid", fin_ticks / 1e8);
}

bool spk_ctx::gs_fused_fits(int64_t nl, int m, bool keep)
{
    const int64_t grid = k::gs_fused_grid(nl);
    if (!grid) return false;
    const int mi = k::plane_class(m) / 4 + (keep ? 3 : 0);
    if (gs_occ[mi] < 0) {   // blocks per CU of the fused kernel at its real block size and LDS: the fewest over its instantiations
        int occ = 1 << 30;
        for (int ng = 1; ng <= 5; ++ng) occ = std::min(occ, k::gs_fused_occupancy(ng, m, keep));
        gs_occ[mi] = occ;
    }
    return (int64_t)gs_occ[mi] * num_cus >= grid;
}

void spk_ctx::ensure_vectors()
{
    const int64_t want = ((int64_t)n_local + m + 255) / 256 * 256;
    if (want != ld) {
        ld = want;
        ws_restart = -1;
        tmp.release();   // every vector sized by ld goes with it (a second KSPSetOperators may bring a larger system)
        tmpb.release();
        bt_cached = nullptr;
        stage_x.release();
        stage_y.release();
        xsol.release();
        rhs.release();
    }
    if (!tmp.p) tmp.alloc((size_t)ld);
    if (!xsol.p) xsol.alloc((size_t)ld);
    if (!rhs.p) rhs.alloc((size_t)ld);
    if (!stage_x.p) stage_x.alloc((size_t)ld);
    if (!stage_y.p) stage_y.alloc((size_t)ld);
}

// Pageable host array -> device through two pinned staging buffers: host threads fill one while the other is on
// the wire (a plain hipMemcpy of pageable memory runs far below the link: 0.35-0.55 s for the 461 MB of the
// 1024^2 matrix in round 1, against ~10 ms of PCIe time).
void spk_ctx::upload_staged(void *dst, const void *src, size_t bytes)
{
    constexpr size_t kChunk = (size_t)32 << 20;
    if (bytes == 0) return;
    if (bytes < ((size_t)1 << 20)) {  // small arrays: not worth the pipeline
        SPK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
        SPK_HIP(hipStreamSynchronize(stream));
        return;
    }
    for (int i = 0; i < 2; ++i) {
        if (!pin[i]) SPK_HIP(hipHostMalloc(&pin[i], kChunk, hipHostMallocDefault));
        if (!pin_ev[i]) SPK_HIP(hipEventCreateWithFlags(&pin_ev[i], hipEventDisableTiming));
    }
    int which = 0;
    for (size_t off = 0; off < bytes; off += kChunk, which ^= 1) {
        const size_t len = std::min(kChunk, bytes - off);
        SPK_HIP(hipEventSynchronize(pin_ev[which]));  // the copy that last used this buffer has left it
        char *stage = (char *)pin[which];
        const char *from = (const char *)src + off;
        parallel_for((int64_t)len, [&](int64_t b0, int64_t b1, int) { std::memcpy(stage + b0, from + b0, (size_t)(b1 - b0)); }, 16);
        SPK_HIP(hipMemcpyAsync((char *)dst + off, stage, len, hipMemcpyHostToDevice, stream));
        SPK_HIP(hipEventRecord(pin_ev[which], stream));
    }
}

namespace spk {

namespace k {
LaunchTimer &launch_timer()
{
    static thread_local LaunchTimer t;
    return t;
}
}  // namespace k

void a_mult(spk_ctx *c, const double *x, double *y, const CsrDev *bt, const double *lam, const int32_t *done, bool accumulate,
            const k::OffDiag *od, const k::GivensRider *rider)
{
    hipStream_t s = c->stream;
    // (bench.py's roofline: the iteration's product launches timed where they run, inside a solve)
    // the kernel's own start / stop time stamps go into a pair of events (SPK_LAUNCH_PRODUCT)
    const bool timed = c->time_products && rider && c->tp_used + 2 <= c->tp_ev.size();
    struct Timed {
        spk_ctx *c; bool on;
        Timed(spk_ctx *c_, bool on_) : c(c_), on(on_) { if (on) k::launch_timer() = k::LaunchTimer{c->tp_ev[c->tp_used], c->tp_ev[c->tp_used + 1]}; }
        ~Timed() { if (on) { k::launch_timer() = k::LaunchTimer{}; c->tp_used += 2; } }
    } timer(c, timed);
    if (c->spmv_format != 0 && c->Adict.ok) k::spmv_dict(c->Adict, x, y, bt, lam, done, s, accumulate, od, rider);
    else if (c->spmv_format == 2) k::spmv_bcsr3(c->Ab3, x, y, bt, lam, done, s, accumulate, od, rider);
    else if (c->spmv_format == 1) k::spmv_bcsr(c->Ab, x, y, bt, lam, done, s, accumulate, od, rider);
    else k::spmv(c->Ad, x, y, bt, lam, done, s, accumulate, od, rider);
}

// out[r] = B_r . (x .* scale)  over this rank's columns (scale == nullptr: B_r . x); MatMult on the (1,0) block.
// m <= 8: the column-window kernel for every row.  General block: short rows row by row through the CSR
// stream kernel, its few long rows through the window kernel (results scattered to their row numbers).
void apply_B(spk_ctx *c, const double *x, const double *scale, double *out, const int32_t *done)
{
    hipStream_t s = c->stream;
    if (!c->b_general) {
        if (scale) k::wide_dot_jacobi(c->B, x, scale, c->fin(out), done, s);
        else k::wide_dot(c->B, x, c->fin(out), done, s);
        return;
    }
    const double *xs = x;
    if (scale) {  // D x0 as a vector of its own (the fused forms that avoid it are for the reference's 4 rows)
        if (c->tmpb.n < (size_t)c->ld) c->tmpb.alloc((size_t)c->ld);
        c->bt_cached = nullptr;
        k::jacobi(scale, x, c->tmpb.p, c->n_local, done, s);
        xs = c->tmpb.p;
    }
    k::spmv(c->Bc, xs, out, nullptr, nullptr, done, s);
    if (c->m_wide > 0) k::wide_dot(c->B, xs, c->fin(out), done, s, c->wide_rows.p);
}

// ---------------------------------------------------------------------------
// y = K x   (MatMult_Nest over MatMult_MPIAIJ blocks)
// ---------------------------------------------------------------------------
void op_mult(spk_ctx *c, const double *x, double *y, const int32_t *done, bool halo_done, bool reuse_bt)
{
    hipStream_t s = c->stream;
    const int32_t nl = c->n_local, m = c->m;
    if (!c->peers.empty() && !halo_done) {  // a rank may have rows to send without needing any itself
        k::gather(x, c->send_idx.p, c->send_off.back(), c->send_buf.p, done, s);
        c->comm->exchange(c->send_buf.p, c->peers, c->send_off, c->xghost.p, c->recv_off, s);
    }
    const k::OffDiag od = c->offdiag();
    const k::OffDiag *odp = c->n_ghost > 0 ? &od : nullptr;   // off-rank columns in the same kernel
    if (m > 0 && c->b_general) {
        // B^T lambda of a general block first (tiled stream kernel), the A block accumulates onto it: the row-by-row
        // epilogue of the product kernels reads such rows uncoalesced (96^3 divergence block: 474 us against 148 + 52)
        // (right after PCApply on the same multipliers -- the step path of the solve -- that product is still in the
        // scratch vector: the same kernel on the same input, so the same bits; 58 us at 96^3 become a 7 us copy)
        if (reuse_bt && c->bt_cached == x + nl && c->Bt.ntiles > 0)
            SPK_HIP(hipMemcpyAsync(y, c->tmpb.p, sizeof(double) * (size_t)nl, hipMemcpyDeviceToDevice, s));
        else k::spmv(c->Bt, x + nl, y, nullptr, nullptr, done, s);
        a_mult(c, x, y, nullptr, nullptr, done, true, odp);
    } else {
        a_mult(c, x, y, m > 0 ? &c->Bt : nullptr, x + nl, done, false, odp);
    }
    if (m > 0) {
        apply_B(c, x, nullptr, y + nl, done);
        c->comm->allreduce_sum(y + nl, m, s);
    }
}

// ---------------------------------------------------------------------------
// y = M^-1 x   (PCApply_Jacobi / PCApply_FieldSplit_Schur)
// ---------------------------------------------------------------------------
// y (op) A^ ^-1 x with the FP32 Richardson/Jacobi sweeps; mode 0: y = , mode 1: y -=
static void inner_apply(spk_ctx *c, const double *x, double *y, int mode, const int32_t *done)
{
    hipStream_t s = c->stream;
    const int32_t nl = c->n_local;
    const float om = (float)c->inner_omega;
    float *ya = c->y32a.p, *yb = c->y32b.p;
    k::cvt_scale_f32(x, c->d32.p, om, c->x32.p, ya, nl, done, s);
    for (int sw = 1; sw < c->inner_sweeps; ++sw) {
        if (!c->peers.empty()) {  // halo of the single-precision iterate, staged as doubles
            k::gather_f32(ya, c->send_idx.p, c->send_off.back(), c->send_buf.p, done, s);
            c->comm->exchange(c->send_buf.p, c->peers, c->send_off, c->xghost.p, c->recv_off, s);
        }
        if (c->spmv_format != 0 && c->Adict.ok) k::jacobi_sweep_f32_dict(c->Adict, c->d32.p, om, c->x32.p, ya, yb, done, s);
        else if (c->spmv_format == 2) k::jacobi_sweep_f32_b3(c->Ab3, c->d32.p, om, c->x32.p, ya, yb, done, s);
        else if (c->spmv_format == 1) k::jacobi_sweep_f32_b2(c->Ab, c->d32.p, om, c->x32.p, ya, yb, done, s);
        else k::jacobi_sweep_f32(c->Ad, c->a32.p, c->d32.p, om, c->x32.p, ya, yb, done, s);
        if (c->n_ghost > 0) k::sweep_offdiag_f32(c->Ao, c->ao_rows.p, c->d32.p, om, c->xghost.p, yb, done, s);
        std::swap(ya, yb);
    }
    k::cvt_f32_out(ya, y, mode, nl, done, s);
}

// y (op) A^ ^-1 x: one multigrid V-cycle or the FP32 sweeps, whichever stands for A^-1
static void ahat_apply(spk_ctx *c, const double *x, double *y, int mode, const int32_t *done)
{
    if (c->amg_d) amg_apply(c, x, y, mode, done);
    else inner_apply(c, x, y, mode, done);
}

// The Schur fieldsplit with the exact complement of a few rows (spk_pc_set_schur_pre): S dense and factored, W = A^ ^-1 B^T
// kept.  t = W^T x0 needs x0 alone, so the multiplier step comes first; A^ ^-1 is applied once in every factorisation.
static void schur_dense_apply(spk_ctx *c, const double *x, double *y, const int32_t *done)
{
    hipStream_t s = c->stream;
    const int32_t nl = c->n_local;
    const int fact = c->schur_fact;
    const k::SchurW w = c->schur_w();
    double *y1 = y + nl;
    if (fact == SPK_SCHUR_DIAG || fact == SPK_SCHUR_UPPER) k::schur_w_y1(w, fact, x + nl, y1, done, s);
    else k::schur_w_dot(w, x, nl, x + nl, y1, c->fin(nullptr), done, s);
    const bool update = fact == SPK_SCHUR_UPPER || fact == SPK_SCHUR_FULL;   // y0 = A^ ^-1 x0 - W y1
    if (c->amg_d && update) {
        const double *last = nullptr;   // the V-cycle's last iterate, read where it lies instead of amg_out's copy
        amg_apply(c, x, y, 0, done, &last);
        k::schur_w_out(w, last, nullptr, y1, y, nl, done, s);
    } else if (c->amg_d) {
        amg_apply(c, x, y, 0, done);
    } else if (update) {
        k::schur_w_out(w, x, c->dinv.p, y1, y, nl, done, s);
    } else {
        k::jacobi(c->dinv.p, x, y, nl, done, s);
    }
}

void op_pc_apply(spk_ctx *c, const double *x, double *y, const int32_t *done)
{
    hipStream_t s = c->stream;
    const int32_t nl = c->n_local, m = c->m;
    const double *x0 = x, *x1 = x + nl;
    double *y0 = y, *y1 = y + nl;
    if (c->schur_dense && c->pc_type == SPK_PC_SCHUR) {
        c->bt_cached = nullptr;
        return schur_dense_apply(c, x, y, done);
    }
    // general block, UPPER / FULL: the last thing written to the scratch vector is B^T y1 (bt_update) -- op_mult on the
    // result may take it from there
    c->bt_cached = (c->b_general && c->Bt.ntiles > 0 && m > 0 && c->pc_type == SPK_PC_SCHUR &&
                    (c->schur_fact == SPK_SCHUR_UPPER || c->schur_fact == SPK_SCHUR_FULL)) ? y1 : nullptr;
    if ((c->inner_sweeps > 0 || c->amg_d) && c->pc_type != SPK_PC_NONE) {
        // same block algebra with the inner solve (FP32 sweeps or a V-cycle) standing for diag(A)^-1
        if (c->pc_type == SPK_PC_JACOBI) {
            ahat_apply(c, x0, y0, 0, done);
            k::copy_small(x1, y1, m, done, s);
            return;
        }
        switch (c->schur_fact) {
        case SPK_SCHUR_DIAG:
            ahat_apply(c, x0, y0, 0, done);
            k::schur_y1(SPK_SCHUR_DIAG, m, x1, nullptr, c->shat.p, y1, done, s);
            break;
        case SPK_SCHUR_UPPER:
            k::schur_y1(SPK_SCHUR_UPPER, m, x1, nullptr, c->shat.p, y1, done, s);
            k::bt_update(2, c->Bt, c->dinv.p, x0, y1, c->tmp.p, done, s, c->b_general ? c->tmpb.p : nullptr);   // x0 - B^T y1
            ahat_apply(c, c->tmp.p, y0, 0, done);
            break;
        default:  // LOWER, FULL
            ahat_apply(c, x0, y0, 0, done);
            apply_B(c, y0, nullptr, c->ttmp.p, done);
            c->comm->allreduce_sum(c->ttmp.p, m, s);
            k::schur_y1(c->schur_fact, m, x1, c->ttmp.p, c->shat.p, y1, done, s);
            if (c->schur_fact == SPK_SCHUR_FULL) {
                k::bt_update(3, c->Bt, c->dinv.p, x0, y1, c->tmp.p, done, s, c->b_general ? c->tmpb.p : nullptr);   // B^T y1
                ahat_apply(c, c->tmp.p, y0, 1, done);                            // y0 -= A^ ^-1 B^T y1
            }
            break;
        }
        return;
    }
    if (c->pc_type == SPK_PC_NONE) {
        k::axpby(1.0, x, 0.0, y, (int64_t)nl + m, done, s);
        return;
    }
    if (c->pc_type == SPK_PC_JACOBI) {
        k::jacobi(c->dinv.p, x0, y0, nl, done, s);
        k::copy_small(x1, y1, m, done, s);  // zero diagonal of the (1,1) block -> 1
        return;
    }
    switch (c->schur_fact) {
    case SPK_SCHUR_DIAG:
        k::jacobi(c->dinv.p, x0, y0, nl, done, s);
        k::schur_y1(SPK_SCHUR_DIAG, m, x1, nullptr, c->shat.p, y1, done, s);
        break;
    case SPK_SCHUR_UPPER:
        k::schur_y1(SPK_SCHUR_UPPER, m, x1, nullptr, c->shat.p, y1, done, s);
        k::bt_update(0, c->Bt, c->dinv.p, x0, y1, y0, done, s, c->b_general ? c->tmpb.p : nullptr);
        break;
    case SPK_SCHUR_LOWER:
    default:  // FULL
        // t = B (D x0) (without storing D x0 for the reference's few long rows)
        apply_B(c, x0, c->dinv.p, c->ttmp.p, done);
        c->comm->allreduce_sum(c->ttmp.p, m, s);
        k::schur_y1(c->schur_fact, m, x1, c->ttmp.p, c->shat.p, y1, done, s);
        if (c->schur_fact == SPK_SCHUR_LOWER) k::jacobi(c->dinv.p, x0, y0, nl, done, s);
        else k::bt_update(1, c->Bt, c->dinv.p, x0, y1, y0, done, s, c->b_general ? c->tmpb.p : nullptr);
        break;
    }
}

// ---------------------------------------------------------------------------
// What the two Krylov drivers (fgmres, minres) share
// ---------------------------------------------------------------------------
void require_setup(spk_ctx *c, const char *who)
{
    if (!c->have_A) fail(SPK_ERR_STATE, "%s: no operator", who);
    if (!c->pc_ready) fail(SPK_ERR_STATE, "%s: call spk_pc_setup first (KSPSetUp)", who);
}

void finish_solve(spk_ctx *c, const KrylovState &st, int32_t cycles, std::chrono::steady_clock::time_point t0,
                  const double *hist, int32_t hist_cap, spk_result *res, double *history, int32_t history_cap)
{
    SPK_HIP(hipStreamSynchronize(c->stream));  // (a speculative start of a cycle that will not run drains as no-ops)
    c->comm->check(c->stream);  // what was raised after the last report (once per solve: blocking reads)
    c->check_device_error();
    const auto t1 = std::chrono::steady_clock::now();
    res->its = st.its;
    res->reason = st.reason;
    res->rnorm = st.rnorm;
    res->rnorm0 = st.rnorm0;
    res->cycles = cycles;
    res->solve_seconds = std::chrono::duration<double>(t1 - t0).count();
    int32_t nh = history ? std::min<int32_t>(st.its + 1, hist_cap) : 0;
    nh = std::min(nh, history_cap);
    if (nh > 0) SPK_HIP(hipMemcpy(history, hist, sizeof(double) * (size_t)nh, hipMemcpyDeviceToHost));
    res->hist_len = nh;
}

void SolverWork::ensure(int64_t ld, int nvec, int32_t hist_cap, size_t state_bytes)
{
    if (vec.n != (size_t)ld * nvec) vec.alloc((size_t)ld * nvec);
    if (hist.n < (size_t)hist_cap) hist.alloc((size_t)hist_cap);
    if (!out.p) out.alloc(8);
    if (!state.p) state.alloc(state_bytes);
    if (!pin) SPK_HIP(hipHostMalloc(&pin, 2 * state_bytes, hipHostMallocDefault));
    for (hipEvent_t &e : ev)
        if (!e) SPK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
}

SolverWork::~SolverWork()
{
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    if (pin) (void)hipHostFree(pin);
}

// ---------------------------------------------------------------------------
// KSPSolve_FGMRES, device resident
// ---------------------------------------------------------------------------
static void ensure_krylov(spk_ctx *c, const spk_opts &o)
{
    c->ensure_scratch();
    c->ensure_vectors();
    const int mk = o.restart;
    const int32_t hist_cap = (int32_t)std::min<int64_t>((int64_t)std::max(o.max_it, 0) + 2, 1 << 22);
    if (c->ws_restart != mk || c->ws_basis != o.basis_precision) {
        if (o.basis_precision == SPK_BASIS_SINGLE) {
            // the basis as floats, restart + 1 vectors (the cycle's last iteration stores no w'), and two FP64 work vectors
            // that take turns as w~ and as the c~ the next product accumulates onto; the FP64 basis goes
            c->V.release();
            c->Vf.alloc((size_t)c->ld * (mk + 1));
            c->Vw.alloc((size_t)c->ld * 2);
        } else {
            c->Vf.release();
            c->Vw.release();
            // one more of each than the cycle uses: the un-normalised three-launch form lets the last iteration of a cycle
            // write its (unused) next vectors too
            c->V.alloc((size_t)c->ld * (mk + 2));
        }
        if (c->ws_restart != mk) c->Z.alloc((size_t)c->ld * (mk + 1));
        c->ws_restart = mk;
        c->ws_basis = o.basis_precision;
    }
    const int ldh = mk + 2;
    const size_t nd = (size_t)ldh * (mk + 1) + 4 * (size_t)(mk + 2) + 8 * (size_t)(mk + 2) + (size_t)hist_cap + 64;
    if (c->kry_d.n < nd) c->kry_d.alloc(nd);
    if (!c->kst.p) c->kst.alloc(1);
    double *p = c->kry_d.p;
    c->ka.st = c->kst.p;
    c->ka.ldh = ldh;
    c->ka.H = p;      p += (size_t)ldh * (mk + 1);
    c->ka.cc = p;     p += mk + 2;
    c->ka.ss = p;     p += mk + 2;
    c->ka.rs = p;     p += mk + 2;
    c->ka.nrs = p;    p += mk + 2;
    c->ka.hcol = nullptr;
    c->ka.tb = p;     p += 8 * (size_t)(mk + 2);
    c->ka.hist = p;
    c->ka.hist_cap = hist_cap;
}

namespace {
// How an FGMRES iteration is launched, resolved once per solve (plan_fgmres).  The product K z_j: forms 5-7 (the
// orthogonalisation inside their launches), a head kernel (Schur or Jacobi), or PCApply + MatMult.
struct FgmresPlan {
    enum Product { kUn3, kSchurHead, kJacobiHead, kStep } product;
    enum Orth { kOrthUn3, kOrthMgs, kOrthSingle, kOrthCgs } orth;
    bool schur, head;     // a head kernel scales v_j, runs the Givens step of j-1; Schur: B D w' out of the last MAXPY
    bool big;             // restart > kMaxNv - 2: the Givens step is a launch of its own
    bool f32;             // the basis is stored as floats (opts.basis_precision; form 5 only)
    bool resident, gsf;   // form 6: one launch per restart cycle; form 7: MDot inside kernel B's launch
    k::GsKnobs gs;        // form 7: the test knobs that choose between its launch variants (spk_gs_launch.hpp)
    int chunk, refine;    // CGS: vectors per MDot / MAXPY launch; -ksp_gmres_cgs_refinement_type
    int nn, bpk, form;    // norm (+ B D w') out of the last MAXPY; B D as m/2 parity planes; what is reported
    const double *bdp;    // the B D rows the kernels stream (Schur)
};

FgmresPlan plan_fgmres(spk_ctx *c, const spk_opts &o)
{
    FgmresPlan p{};
    const int mk = o.restart, m = c->m, nl = c->n_local;
    // How one classical Gram-Schmidt iteration (two reductions) is launched on the head-kernel paths
    // (opts.iteration_form / SPK_ITER_FORM; include/spk.h lists the forms and their measured times).
    int form = o.iteration_form;
    if (const char *e = getenv("SPK_ITER_FORM")) {   // test-only knob: the whole GPU suite is run under each form with it
        char *end = nullptr;
        const long f = strtol(e, &end, 10);
        if (end == e || *end || f < SPK_ITER_AUTO || f > SPK_ITER_LAST)
            fail(SPK_ERR_ARG, "SPK_ITER_FORM=%s: not an iteration form (%d..%d)", e, (int)SPK_ITER_AUTO, (int)SPK_ITER_LAST);
        form = (int)f;
    }
    if (form < SPK_ITER_AUTO || form > SPK_ITER_LAST) fail(SPK_ERR_ARG, "fgmres: unknown iteration_form %d", form);
    if (form == SPK_ITER_TWO_LAUNCH || form == SPK_ITER_THREE_LAUNCH || form == SPK_ITER_BA) form = SPK_ITER_UNNORM;   // retired: aliases of 5
    // -ksp_gmres_restart beyond 62: Gram-Schmidt in chunks of <= 40 vectors (the fused kernels keep one lane / one LDS
    // slot per basis vector).  A long restart keeps the head kernel -- VecScale + PCApply + the B^T part of the product in
    // one pass, the product accumulating onto it, B D w' out of the last MAXPY chunk -- and only the Givens step is a
    // launch of its own: its column no longer fits the head kernel's workgroup 0.
    p.big = mk > k::kMaxNv - 2;
    p.chunk = p.big ? 40 : k::kMaxNv;
    p.refine = o.cgs_refine;
    // fused Schur path: VecScale + PC + B^T part of the operator in one pass ("head"), B D w' in the MAXPY pass, the
    // Givens step of iteration j-1 inside the head kernel of iteration j
    // (a dense Schur complement, like the V-cycle and the FP32 sweeps, runs on the step-by-step path: its bd planes are W)
    p.schur = o.fused && c->bd.p && c->pc_type == SPK_PC_SCHUR && !c->schur_dense;
    // the same head kernel without a constraint block: Jacobi on K = A (the reference as written,
    // SaddlePointProblem.c:66, and BASELINE config 2): VecScale + PCApply_Jacobi + deferred Givens
    const bool jac = o.fused && !p.schur && c->pc_type == SPK_PC_JACOBI && m == 0 && c->even_all && c->nonempty_all &&
                     c->inner_sweeps == 0 && !c->amg_d;   // (a V-cycle, like the FP32 sweeps, runs on the step-by-step path)
    p.head = p.schur || jac;
    p.nn = p.schur ? 1 + m : 1;
    p.bpk = p.schur && c->bd_packed ? 1 : 0;
    p.bdp = p.schur ? (p.bpk ? c->bdpk.p : c->bd.p) : nullptr;
    // single-reduction Gram-Schmidt (fused CGS without refinement): h = V^T w, q = B D w and w.w
    // come out of ONE pass and ONE all-reduce; ||w'||^2 = w.w - |h|^2 and B D w' = q - sum h_i B D v_i
    // follow without touching w' -- one collective per iteration instead of two.
    // Opt-in (opts.single_reduce = 1): the subtraction cancels, see include/spk.h.
    // The Jacobi head path (K = A) takes the same route with m = 0: ||w'||^2 = w.w - |h|^2 only.
    // (MDot carries restart + m vectors: both must fit one reduction; a long restart runs its Givens step on its own.)
    const bool cgs1 = o.orthog == SPK_ORTHOG_CGS && o.cgs_refine == SPK_REFINE_NEVER;
    const bool single = p.head && cgs1 && o.single_reduce == 1 && !p.big && mk + m <= k::kMaxNv - 1;
    // AUTO: three launches on an UN-normalised basis -- MDot (raw inner products), MAXPY + norm + next PCApply, plain SpMV
    // with the Givens step and the new scale factor in one extra workgroup (GivensRider).  V~_j = h_{j,j-1} v_j: nothing
    // compounds, no vector is ever scaled in memory.  Either matrix format, any number of ranks, any transport.
    const bool un3 = p.head && !single && cgs1 && mk + m <= k::kMaxNv - 2 &&
                     (form == SPK_ITER_UNNORM || form == SPK_ITER_AUTO || form == SPK_ITER_RESIDENT || form == SPK_ITER_GS_FUSED);
    // RESIDENT: one launch per restart cycle, the basis in registers (spk_k_resident.hip): what AUTO takes where it fits
    static const bool res_env_off = [] { const char *e = getenv("SPK_RESIDENT"); return e && !strcmp(e, "0"); }();
    const int res_planes = !p.schur ? 0 : (p.bpk ? m / 2 : m);
    // several ranks: every rank must take it (agreed at KSPSetUp: res_fit_all), the collectives must be the peer-store
    // backend's (they run inside the launch), and the halo rows must be contiguous send ranges
    const bool res_multi = c->comm->size() > 1;
    const bool res_rank_ok = !res_multi ? (c->peers.empty() && c->n_ghost == 0)
                                        : (c->res_fit_all && c->comm->fuses() && (c->peers.empty() || c->send_ranges.n > 0));
    p.resident = un3 && (form == SPK_ITER_RESIDENT || (form == SPK_ITER_AUTO && !res_env_off)) && res_rank_ok &&
                 c->spmv_format == 1 && c->Adict.ok && c->Adict.bs == 2 && nl % 2 == 0 && mk >= (res_multi ? 3 : 2) &&
                 k::resident_fits(c->Adict, c->num_cus, mk, res_planes);
    // GS_FUSED (form 7): MDot and kernel B in one launch -- one rank, fat vectors,
    // every workgroup of the launch resident at once; what AUTO takes there
    // (the knob is read per solve, so that a test can flip it between two solves of one context)
    p.gs = k::gs_knobs_env();
    p.gsf = un3 && !p.resident && (form == SPK_ITER_GS_FUSED || form == SPK_ITER_AUTO) && c->comm->size() == 1 &&
            c->peers.empty() && c->n_ghost == 0 && mk + m <= 41 && c->gs_fused_fits(nl, m, p.gs.keep);
    p.product = un3 ? FgmresPlan::kUn3 : p.schur ? FgmresPlan::kSchurHead : jac ? FgmresPlan::kJacobiHead : FgmresPlan::kStep;
    p.orth = un3 ? FgmresPlan::kOrthUn3 : o.orthog == SPK_ORTHOG_MGS ? FgmresPlan::kOrthMgs
           : single ? FgmresPlan::kOrthSingle : FgmresPlan::kOrthCgs;
    if (o.basis_precision == SPK_BASIS_SINGLE) {
        // an FP32 basis: form 5 only (AUTO, 6 and 7 resolve to it).  Whatever does not run there is refused here, before
        // anything is allocated or enqueued -- the first reason that applies is named
        const char *why = c->comm->size() > 1 ? "it runs on one rank (the path agreed across ranks does not carry the precision)"
            : o.orthog != SPK_ORTHOG_CGS ? "modified Gram-Schmidt"
            : o.cgs_refine != SPK_REFINE_NEVER ? "CGS refinement"
            : o.single_reduce == 1 ? "single_reduce"
            : !o.fused ? "fused = 0"
            : c->amg_d ? "a multigrid V-cycle runs on the step-by-step path"
            : c->inner_sweeps > 0 ? "the FP32 inner sweeps run on the step-by-step path"
            : c->schur_dense && c->pc_type == SPK_PC_SCHUR ? "a dense Schur complement runs on the step-by-step path"
            : !c->even_all ? "an odd local size"
            : mk + 2 * m > k::kMaxNv - 2 ? "restart + 2 m beyond the fused limit of 62 (VecMDot carries B D of the newest vector too)"
            : !p.head ? "this preconditioner runs on the step-by-step path"
            : !un3 ? "this iteration_form is not the un-normalised one" : nullptr;
        if (why || !un3) fail(SPK_ERR_UNSUPPORTED, "fgmres: basis_precision single needs iteration form 5: %s", why ? why : "refused");
        p.resident = p.gsf = false;
    }
    p.f32 = o.basis_precision == SPK_BASIS_SINGLE;
    p.form = p.resident ? SPK_ITER_RESIDENT : p.gsf ? SPK_ITER_GS_FUSED : un3 ? SPK_ITER_UNNORM : p.head ? SPK_ITER_FOUR_LAUNCH : -1;
    return p;
}

// the plan's own buffers (after the solve's first launches: form 7's arming launch keeps its place in the stream)
void ensure_plan_buffers(spk_ctx *c, const FgmresPlan &p, int mk)
{
    if (p.big && c->bigdots.n < 2 * ((size_t)mk + 4)) c->bigdots.alloc(2 * ((size_t)mk + 4));   // first and refinement pass
    const size_t need = p.resident ? (size_t)k::resident_scratch_doubles(c->num_cus, mk) : 0;
    if (c->res_P.n < need) c->res_P.alloc(need);
    if (p.gsf && !c->gs_tot.p) {
        c->gs_tot.alloc(2 * k::kPartialLd);
        k::arm_partials(c->gs_tot.p, c->gs_tot.n, c->stream);
    }
    if (p.product == FgmresPlan::kUn3 && c->basis_sc.n < (size_t)mk + 2) c->basis_sc.alloc((size_t)mk + 2);
}

// One solve's constants and the views of its work space
struct FgmresRun {
    spk_ctx *c;
    const FgmresPlan &p;
    hipStream_t s;
    int mk, m, lam_in_dot, nl;
    int64_t N, ld, n_dot;
    double *V, *Z, *sm, *sm2, *nrm2b, *w1side;
    float *Vf;    // an FP32 basis (else nullptr): V~_j as floats, w~ / c~ in the two work vectors W
    double *W;
    double *Vj(int j) const { return V + (size_t)ld * j; }
    // forms 5-7: the residual of a restart (normalised into v_0 by the first head) and w~ of iteration loc (c~ of loc - 1)
    double *r0() const { return Vf ? W : V; }
    double *wun(int loc) const { return Vf ? W + (size_t)ld * ((loc + 1) & 1) : Vj(loc + 1); }
    double *Zj(int j) const { return Z + (size_t)ld * j; }
    // small[]: two parity sets so that a deferred Givens step (head paths) can still read iteration j-1's scalars while
    // iteration j produces its own: dots at q*128, norm (+ B D w') at q*128+64; lambda entries of w, side copies at 400
    double *dotsbuf(int q) const { return sm + (q & 1) * 128; }
    double *nrmbuf(int q) const { return sm + (q & 1) * 128 + 64; }
    double *wl(int q) const { return sm + 400 + (q & 1) * 8; }
};

// What an iteration hands to the next one and to the end of its cycle
struct CycleState {
    bool stop = false; int last = -1;               // last iteration whose Givens step is still pending (head paths)
    bool head_done = false, prev_inhead = false;    // single reduction: the previous MAXPY ran this head (and halo)
    int pend_loc = -1;                              // the Givens step handed to the cycle-end launch: iteration,
    const double *pend_h = nullptr; double *pend_n = nullptr;   // Hessenberg column and norm
};

// w (+)= A z: the halo exchange (unless done already), then diagonal and off-rank columns in one kernel, either format
void product(const FgmresRun &r, const double *z, double *w, bool halo_done, bool accumulate, const int32_t *done,
             const k::GivensRider *rider = nullptr)
{
    spk_ctx *c = r.c;
    if (!c->peers.empty() && !halo_done) {
        if (c->send_ranges.n == 0) k::gather(z, c->send_idx.p, c->send_off.back(), c->send_buf.p, done, r.s);
        c->comm->exchange(c->send_buf.p, c->peers, c->send_off, c->xghost.p, c->recv_off, r.s);
    }
    const k::OffDiag od = c->offdiag();
    a_mult(c, z, w, nullptr, nullptr, done, accumulate, c->n_ghost > 0 ? &od : nullptr, rider);
}

// v_j = Vj(j) / ||.|| (in place), z_j = M^-1 v_j, Schur: w = B^T z1 (u part) | B z0 (lambda part); workgroup 0 also runs
// the Givens step of iteration `givens` (< 0: none).  sr: the halo buffer is filled (and, from fused_halo, exchanged).
void launch_head(const FgmresRun &r, int j, double *w, int givens, const k::SendRanges *sr, const int32_t *done, double *wl)
{
    spk_ctx *c = r.c;
    double *vj = j == 0 ? r.r0() : r.Vj(j);
    if (r.p.schur)
        k::fused_head(vj, r.nrmbuf(j + 1), r.w1side, c->dinv.p, r.p.bdp, r.ld, c->shat.p, c->gram.p, c->schur_fact, r.nl,
                      r.m, r.Zj(j), w, c->ka, givens, r.dotsbuf(j + 1), done, r.s, sr, r.p.bpk, wl);
    else
        k::fused_head(vj, r.nrmbuf(j + 1), nullptr, c->dinv.p, nullptr, r.ld, nullptr, nullptr, SPK_SCHUR_LOWER, r.nl, 0,
                      r.Zj(j), nullptr, c->ka, givens, r.dotsbuf(j + 1), done, r.s, sr);
}

// Forms 5, 6 and 7: product and orthogonalisation of iteration loc.  Returns true when the cycle ran as one launch.
bool un3_iteration(const FgmresRun &r, CycleState &cs, int loc, const int32_t *done)
{
    spk_ctx *c = r.c;
    const bool schur = r.p.schur;
    double *w = r.wun(loc), *db = r.dotsbuf(loc), *nb = r.nrmbuf(loc);
    if (loc == 0) {
        // first iteration of a cycle: the classic head on the normalised r, then the plain product
        k::SendRanges sr = c->send_ranges;
        const bool inhead = sr.n > 0 && c->comm->fused_halo(sr, c->xghost.p);
        launch_head(r, 0, w, -1, sr.n > 0 ? &sr : nullptr, done, r.wl(0));
        if (r.Vf) k::cvt_basis_f32(r.r0(), r.Vf, r.N, done, r.s);   // V~_0 = float(v_0)
        product(r, r.Zj(0), w, inhead, schur, done);
    }
    if (r.p.resident) {
        // form 6: the rest of the cycle is ONE launch, iterations 0 .. mk-1 with the basis in registers
        k::ResidentArgs a{};
        a.mk = r.mk; a.m = schur ? r.m : 0; a.packed = r.p.bpk; a.fact = schur ? c->schur_fact : SPK_SCHUR_LOWER;
        a.lam_in_dot = r.lam_in_dot; a.nl = r.nl; a.ld = r.ld; a.err = c->errw.p; a.ticks = c->fin_ticks;
        a.V0 = r.Vj(0); a.V1 = r.Vj(1); a.Z = r.Z; a.dinv = c->dinv.p; a.bd = r.p.bdp; a.ldb = r.ld;
        a.shat = c->shat.p; a.gram = c->gram.p; a.P = c->res_P.p; a.ka = c->ka; a.sc_out = c->basis_sc.p;
        if (c->comm->size() > 1) {
            // the launch's mk + 1 all-reduces and mk - 1 halo exchanges: consecutive sequence numbers, reserved now
            a.sr0 = c->send_ranges;
            a.sr1 = c->send_ranges;
            if (!c->comm->resident_plan(r.mk + 1, c->peers.empty() ? 0 : r.mk - 1, a.ar, a.sr0, a.sr1, c->xghost.p))
                fail(SPK_ERR_COMM, "fgmres: the communicator cannot carry a resident cycle (agreed at set-up, refused now)");
            if (c->peers.empty()) a.sr0.n = a.sr1.n = 0;
            if (c->n_ghost > 0) a.od = c->offdiag();
        }
        if (!k::cycle_resident(c->Adict, c->num_cus, a, done, r.s)) fail(SPK_ERR_STATE, "fgmres: resident cycle kernel refused its shape");
        return true;
    }
    // raw inner products of the un-normalised basis with w~ (and B D w~); scaled where they are consumed
    // (form 7: inside the launch of kernel B, below)
    // (the cycle's last iteration too, where its loc + 1 + m values fit MDot's 40 accumulators)
    const bool gs = r.p.gsf && (loc + 1 < r.mk || loc + 1 + (schur ? r.m : 0) <= 40);
    if (r.Vf) {
        const bool spl = r.p.bpk != 0;
        k::mdot_f32(r.Vf, r.ld, loc + 1, w, r.N, r.n_dot, c->fin(db), done, r.s, schur ? (spl ? c->bdpk.p : c->bd.p) : nullptr, r.ld,
                    schur ? r.m : 0, spl ? 1 : 0);
    } else if (!gs) {
        const bool one = loc + 1 + r.m <= 40, spl = r.p.bpk && one;
        const k::PeerAR ar = one ? c->comm->fused_allreduce(loc + 2 + (schur ? r.m : 0), k::kStatArDots) : k::PeerAR{};
        k::mdot(r.V, r.ld, loc + 1, w, r.N, r.n_dot, c->fin(db, ar), done, r.s, schur ? (spl ? c->bdpk.p : c->bd.p) : nullptr,
                schur ? r.m : 0, spl ? 1 : 0);
        if (!ar.P) c->comm->allreduce_sum(db, loc + 2 + (schur ? r.m : 0), r.s);
    }
    const k::PeerAR ar2 = c->comm->fused_allreduce(1, k::kStatArNorm);
    k::IterB b{};
    b.V = r.Vf ? reinterpret_cast<const double *>(r.Vf) : r.V; b.ldv = r.ld; b.nv = loc + 1;
    b.w32 = r.Vf ? r.Vf + (size_t)r.ld * (loc + 1) : nullptr; b.dots = db; b.tb = c->ka.tb;
    b.w = w; b.dinv = c->dinv.p; b.bd = r.p.bdp; b.ldb = r.ld; b.shat = c->shat.p; b.gram = c->gram.p;
    b.fact = schur ? c->schur_fact : SPK_SCHUR_LOWER;
    b.nl = r.nl; b.m = r.m; b.packed = r.p.bpk;
    b.zun = r.Zj(loc + 1); b.c = schur ? r.wun(loc + 1) : nullptr; b.wl_in = r.wl(loc); b.wl_out = r.wl(loc + 1);
    b.lam_in_dot = r.lam_in_dot;
    b.partials = c->partials.p; b.out = nb; b.ar = ar2; b.err = c->errw.p; b.fin_ticks = c->fin_ticks;
    b.sc = c->basis_sc.p; b.hbuf = r.sm2; b.ka = c->ka; b.loc = loc;
    // ||w'||^2 is left as one partial per workgroup: the rider of the product launch reduces it (and all-reduces
    // it, peer-store) beside the row tiles -- the product of an un-normalised vector does not need the norm.
    // (Not with an all-reduce that is a launch of its own, nor behind the last iteration of a cycle.)
    const bool defer = loc + 1 < r.mk && (c->comm->size() == 1 || ar2.P);
    b.defer_fin = defer ? 1 : 0; b.done = done;
    b.dead_out = loc + 1 == r.mk ? 1 : 0;   // no iteration of this cycle follows
    k::SendRanges sr = c->send_ranges;
    const bool inb = sr.n > 0 && c->comm->fused_halo(sr, c->xghost.p);
    if (sr.n > 0) b.sr = sr;
    int fin_n;
    if (gs) {
        k::GsArgs g{};
        g.V2 = schur ? (r.p.bpk ? c->bdpk.p : c->bd.p) : nullptr;
        g.cnt = loc + 1 + (schur ? r.m : 0); g.split = r.p.bpk;
        g.n2 = (r.N + 1) / 2; g.n_dot = r.n_dot;
        g.partials = c->partials.p + 1;   // column 0 of the rows carries the ||w'||^2 partials
        g.out = db;
        g.tot = c->gs_tot.p + (c->gs_seq & 1) * k::kPartialLd;
        g.tot_next = c->gs_tot.p + ((c->gs_seq + 1) & 1) * k::kPartialLd;
        g.fe = k::FinErr{c->errw.p, c->fin_ticks};
        const k::GsVariant v = k::gs_fused_variant(r.p.gs, b.nl, g.n2, b.m, b.packed);
        fin_n = k::gs_fused(b, g, v, r.s);
        ++c->last_gs_launches;
        if (v == k::kGsKeepAheadTail) ++c->last_gs_tail;
        ++c->gs_seq;   // (launched: it arms tot_next even when the solve is over)
    } else {
        fin_n = k::iter_maxpy_uhead(b, r.s);
    }
    if (!ar2.P && !defer) c->comm->allreduce_sum(nb, 1, r.s);
    // the Givens step of this iteration (and the new vector's scale factor) ride in the next product launch
    k::GivensRider gr{c->ka, loc, r.sm2, nb, c->basis_sc.p, defer ? c->partials.p : nullptr, defer ? fin_n : 0,
                      k::FinErr{c->errw.p, c->fin_ticks}, defer ? ar2 : k::PeerAR{}};
    if (loc + 1 < r.mk) product(r, r.Zj(loc + 1), r.wun(loc + 1), inb, schur, done, &gr);
    else cs.pend_h = r.sm2, cs.pend_n = nb, cs.pend_loc = loc;   // no product behind it: the step runs in the cycle-end launch
    return false;
}

// w = K z_j on the head paths: the head kernel (unless the previous MAXPY ran it), then the A product onto it
void head_product(const FgmresRun &r, CycleState &cs, int loc, double *w, const int32_t *done)
{
    spk_ctx *c = r.c;
    bool inhead = cs.prev_inhead;
    if (!cs.head_done) {
        k::SendRanges sr = c->send_ranges;
        inhead = sr.n > 0 && c->comm->fused_halo(sr, c->xghost.p);   // the head does the whole exchange ...
        // ... or, Schur, fills the packed halo buffer (the Jacobi path's op_mult gathers itself)
        launch_head(r, loc, w, r.p.big ? -1 : loc - 1, sr.n > 0 && (r.p.schur || inhead) ? &sr : nullptr, done, nullptr);
        cs.last = r.p.big ? -1 : loc;
        if (r.p.schur && r.p.orth == FgmresPlan::kOrthSingle) k::copy_small(w + r.nl, r.wl(loc), r.m, done, r.s);
    }
    if (r.p.schur) product(r, r.Zj(loc), w, inhead, true, done);
    else op_mult(c, r.Zj(loc), w, done, inhead);    // w = A z_j (halo inside, unless the head kernel did it)
}

// KSPGMRESModifiedGramSchmidtOrthogonalization: one dot + one axpy per basis vector
void orth_mgs(const FgmresRun &r, int loc, double *w, double *db, double *nb, const int32_t *done)
{
    spk_ctx *c = r.c;
    for (int j = 0; j <= loc; ++j) {
        k::mdot(r.Vj(j), r.ld, 1, w, r.N, r.n_dot, c->fin(db + j), done, r.s);
        c->comm->allreduce_sum(db + j, 1, r.s);
        const bool lastv = j == loc;
        k::maxpy(r.Vj(j), r.ld, 1, nullptr, db + j, -1.0, w, r.N, r.n_dot, c->fin(lastv ? nb : nullptr), done, r.s,
                 lastv ? r.p.bdp : nullptr, r.ld, r.nl, r.m, lastv && r.p.schur ? r.w1side : nullptr, nullptr, r.p.bpk);
    }
    c->comm->allreduce_sum(nb, r.p.nn, r.s);
}

// single reduction: the MAXPY of iteration loc also runs the head of iteration loc+1 and the Givens step of iteration
// loc (k::maxpy_head): three launches and one reduction per iteration
void orth_single(const FgmresRun &r, CycleState &cs, int loc, double *w, double *db, double *nb, const int32_t *done)
{
    spk_ctx *c = r.c;
    const int m = r.m;
    const k::PeerAR ar = loc + 1 + m <= 40 ? c->comm->fused_allreduce(loc + 2 + m, k::kStatArDots) : k::PeerAR{};
    // B D w from the same pass: the dense rows, or two halves per parity-interleaved plane
    const bool spl = r.p.bpk && loc + 1 + m <= 40;
    k::mdot(r.V, r.ld, loc + 1, w, r.N, r.n_dot, c->fin(db, ar), done, r.s, spl ? c->bdpk.p : c->bd.p, m, spl ? 1 : 0);
    if (!ar.P) c->comm->allreduce_sum(db, loc + 2 + m, r.s);
    if (loc + 1 < r.mk) {
        k::SendRanges sr = c->send_ranges;
        cs.prev_inhead = sr.n > 0 && c->comm->fused_halo(sr, c->xghost.p);
        // Schur: the packed halo buffer is filled even without the peer backend; Jacobi: op_mult gathers
        const k::SendRanges *srp = sr.n > 0 && (r.p.schur || cs.prev_inhead) ? &sr : nullptr;
        k::maxpy_head(r.V, r.ld, loc + 1, db, c->ka.tb, nb, w, c->dinv.p, r.p.bdp, r.ld, c->shat.p, c->gram.p,
                      r.p.schur ? c->schur_fact : SPK_SCHUR_LOWER, r.nl, m, r.Zj(loc + 1), r.p.schur ? r.Vj(loc + 2) : nullptr,
                      r.w1side, r.wl(loc), r.wl(loc + 1), c->ka, loc, done, r.s, srp, r.p.bpk);
        cs.head_done = true, cs.last = -1;  // its Givens step is done
    } else {
        k::PythArgs py{m, db, c->ka.tb, nb};
        k::maxpy(r.V, r.ld, loc + 1, nullptr, db, -1.0, w, r.N, r.n_dot, c->fin(nullptr), done, r.s, nullptr, r.ld, r.nl, m,
                 r.w1side, &py);
        cs.head_done = false, cs.last = loc;
    }
}

// One classical Gram-Schmidt pass, in chunks: h = V^T w into dots (every product with the SAME w), w -= V h, ||w||^2
// (+ B D w') into nrm.  peer_ar: the all-reduces may ride in the finish of the two kernels (peer-store backend)
void cgs_pass(const FgmresRun &r, int loc, double *w, double *dots, double *nrm, const int32_t *gate, bool peer_ar)
{
    spk_ctx *c = r.c;
    const int chunk = r.p.chunk;
    const k::PeerAR ar1 = peer_ar && loc + 1 <= 40 ? c->comm->fused_allreduce(loc + 2, k::kStatArDots) : k::PeerAR{};
    for (int v0 = 0; v0 <= loc; v0 += chunk)
        k::mdot(r.Vj(v0), r.ld, std::min(chunk, loc + 1 - v0), w, r.N, r.n_dot, c->fin(dots + v0, ar1), gate, r.s);
    if (!ar1.P) c->comm->allreduce_sum(dots, loc + 2, r.s);
    const k::PeerAR ar2 = peer_ar ? c->comm->fused_allreduce(r.p.nn, k::kStatArNorm) : k::PeerAR{};
    for (int v0 = 0; v0 <= loc; v0 += chunk) {
        const bool lastc = v0 + chunk > loc;
        k::maxpy(r.Vj(v0), r.ld, std::min(chunk, loc + 1 - v0), nullptr, dots + v0, -1.0, w, r.N, r.n_dot,
                 c->fin(lastc ? nrm : nullptr, ar2), gate, r.s, lastc ? r.p.bdp : nullptr, r.ld, r.nl, r.m,
                 lastc && r.p.schur ? r.w1side : nullptr, nullptr, r.p.bpk);
    }
    if (!ar2.P) c->comm->allreduce_sum(nrm, r.p.nn, r.s);
}

// classical Gram-Schmidt, and the second pass on the device's own decision (-ksp_gmres_cgs_refinement_type; PETSc's
// ||w'|| < ||h|| test for ifneeded)
void orth_cgs(const FgmresRun &r, int loc, double *w, double *db, double *nb, const int32_t *done)
{
    cgs_pass(r, loc, w, db, nb, done, !r.p.big);
    if (r.p.refine == SPK_REFINE_NEVER) return;
    double *db2 = r.p.big ? r.c->bigdots.p + (size_t)r.mk + 4 : r.sm2;
    k::krylov_refine_decide(r.c->ka, loc, r.p.refine, db, nb, db2, r.s);
    cgs_pass(r, loc, w, db2, r.nrm2b, &r.c->kst.p->skip_refine, false);
    k::krylov_refine_merge(r.c->ka, loc, db, db2, nb, r.nrm2b, r.p.nn, r.s);
}
}  // namespace

void fgmres(spk_ctx *c, const double *b, double *x, const spk_opts &o, spk_result *res, double *history,
            int32_t history_cap)
{
    require_setup(c, "fgmres");
    if (o.orthog != SPK_ORTHOG_CGS && o.orthog != SPK_ORTHOG_MGS) fail(SPK_ERR_ARG, "fgmres: unknown orthogonalisation %d", o.orthog);
    if (o.cgs_refine < SPK_REFINE_NEVER || o.cgs_refine > SPK_REFINE_ALWAYS) fail(SPK_ERR_ARG, "fgmres: unknown cgs_refine %d", o.cgs_refine);
    if (o.basis_precision != SPK_BASIS_DOUBLE && o.basis_precision != SPK_BASIS_SINGLE)
        fail(SPK_ERR_ARG, "fgmres: unknown basis_precision %d", o.basis_precision);
    if (o.restart < 1 || o.restart > k::kBigNv - 2) fail(SPK_ERR_ARG, "fgmres: restart %d outside [1,%d]", o.restart, k::kBigNv - 2);
    const FgmresPlan p = plan_fgmres(c, o);   // (refuses before anything is allocated or enqueued)
    ensure_krylov(c, o);
    c->last_form = p.form;
    c->last_gs_launches = c->last_gs_tail = 0;
    c->last_basis = o.basis_precision;
    c->last_basis_bytes = p.f32 ? (int64_t)(c->Vf.n * sizeof(float)) : (int64_t)(c->V.n * sizeof(double));
    c->last_single = p.orth == FgmresPlan::kOrthSingle ? 1 : 0;
    hipStream_t s = c->stream;
    const int mk = o.restart;
    const int64_t N = (int64_t)c->n_local + c->m, ld = c->ld;
    const int64_t n_dot = (int64_t)c->n_local + (c->comm->rank() == 0 ? c->m : 0);
    const int32_t *done = &c->kst.p->done;
    const double *inv_tt = &c->kst.p->inv_tt;
    double *sm = c->small.p, *bn2 = sm + 384;   // small[]: FgmresRun's parity sets at 0..255, ||b||^2 at 384
    const FgmresRun r{c, p, s, mk, c->m, c->comm->rank() == 0 ? 1 : 0, c->n_local, N, ld, n_dot,
                      c->V.p, c->Z.p, sm, sm + 256, sm + 320, c->y1tmp.p + 48, p.f32 ? c->Vf.p : nullptr, c->Vw.p};
    const bool un3 = p.product == FgmresPlan::kUn3;

    SPK_HIP(hipStreamSynchronize(s));
    const auto t0 = std::chrono::steady_clock::now();

    // ||b|| for KSPConvergedDefault
    k::sqnorm(b, n_dot, c->fin(bn2), nullptr, s);
    c->comm->allreduce_sum(bn2, 1, s);
    k::krylov_init(c->ka, o, bn2, s);

    // initial residual into V0
    if (o.guess_nonzero) op_mult(c, x, c->tmp.p, nullptr);
    else SPK_HIP(hipMemsetAsync(x, 0, sizeof(double) * (size_t)N, s));
    SPK_HIP(hipMemcpyAsync(r.r0(), b, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, s));
    if (o.guess_nonzero) k::axpby(-1.0, c->tmp.p, 1.0, r.r0(), N, nullptr, s);
    ensure_plan_buffers(c, p, mk);

    c->ka.tentative = p.orth == FgmresPlan::kOrthSingle || p.f32 ? 1 : 0;
    c->ka.theta = p.f32 ? k::kBasisTheta : 0.0;
    KrylovState st{};
    int cycles = 0;
    // The solve's state reaches the host through pinned memory written by krylov_cycle_begin (no copy on the stream); the
    // host waits for the event behind that launch only after it has enqueued the start of the cycle (kAhead iterations),
    // whose kernels are gated off on the device if the solve is over: the stream never drains at a restart.  (Pageable
    // read-back copies and a stream synchronisation per cycle cost 35-85 us of idle GPU: 256^2 28.1 -> 23.7 us per iteration.)
    if (!c->pin_state) SPK_HIP(hipHostMalloc(&c->pin_state, 512, hipHostMallocDefault));
    if (!c->state_ev) SPK_HIP(hipEventCreateWithFlags(&c->state_ev, hipEventDisableTiming));
    KrylovState *ps = (KrylovState *)c->pin_state;
    int32_t *pe = (int32_t *)((char *)c->pin_state + 384);
    pe[0] = pe[1] = 0;
    bool pend_check = false;   // the previous cycle's state is on its way to the pinned slot (state_ev)
    bool finished = false;
    const int kAhead = 2;      // iterations of a cycle enqueued before the host looks at the previous cycle's verdict
    auto read_state = [&]() {
        SPK_HIP(hipEventSynchronize(c->state_ev));
        st = *ps;
        pend_check = false;
        if (pe[1]) c->comm->check(s);         // a peer that never arrived: SPK_ERR_COMM instead of a wrong answer
        if (pe[0]) c->check_device_error();     // a reduction that timed out: SPK_ERR_HIP, not KSP_DIVERGED_NANORINF
        return st.done != 0;
    };
    for (;;) {
        // ---- cycle start: ||r|| (parity slot 1 = "iteration -1"), convergence test, v0 = r/||r|| ----
        // (from the second cycle on the previous cycle's end has formed r = b - K x and these sums in one pass)
        if (cycles == 0) {
            if (p.schur) k::sqnorm_bd(r.r0(), N, n_dot, c->bd.p, ld, r.nl, r.m, r.w1side, c->fin(r.nrmbuf(1)), done, s);
            else k::sqnorm(r.r0(), n_dot, c->fin(r.nrmbuf(1)), done, s);
        }
        c->comm->allreduce_sum(r.nrmbuf(1), p.nn, s);
        // (the kernel also reports the state it finds / leaves into pinned memory: the verdict on the PREVIOUS cycle and,
        // through its own convergence test on the true residual, on the solve -- read by the host at loc == kAhead)
        const k::StateReport report{ps, pe, c->errw.p, c->comm->error_dev()};
        k::krylov_cycle_begin(c->ka, r.nrmbuf(1), s, (un3 || p.orth == FgmresPlan::kOrthSingle) ? c->ka.tb : nullptr, r.m,
                              un3 ? c->basis_sc.p : nullptr, &report);
        SPK_HIP(hipEventRecord(c->state_ev, s));
        pend_check = true;
        if (!p.head) k::scale_dev(r.Vj(0), N, inv_tt, done, s);

        CycleState cs;
        int64_t its_cap = INT64_MAX;   // iterations this cycle may still run before -ksp_max_it (known once the report is read)
        for (int loc = 0; loc < mk && !cs.stop; ++loc) {
            if (pend_check && loc == kAhead) {
                if (read_state()) {   // the previous cycle ended the solve: what was enqueued of this one is gated off
                    finished = true;  // on the device
                    break;
                }
                its_cap = (int64_t)o.max_it - st.its;   // (the report is this cycle's cycle_begin: its = iterations before it)
            }
            // -ksp_max_it ends the solve inside this cycle: the device stops there by itself, the host need not enqueue
            // (gated) launches beyond it
            if (loc >= its_cap) break;
            const int32_t *done = &c->kst.p->skip_iter;  // the gate of everything inside an iteration
            double *w = un3 ? nullptr : r.Vj(loc + 1);   // (forms 5-7 take theirs from the run: an FP32 basis has no such slot)
            double *db = p.big ? c->bigdots.p : r.dotsbuf(loc), *nb = r.nrmbuf(loc);
            if (un3) {
                if (un3_iteration(r, cs, loc, done)) break;   // (form 6: the whole cycle was one launch)
            } else {
                if (p.product == FgmresPlan::kStep) {
                    op_pc_apply(c, r.Vj(loc), r.Zj(loc), done);     // z_j = M^-1 v_j
                    op_mult(c, r.Zj(loc), w, done, false, true);   // w = K z_j (B^T z_1 of a general block: as PCApply left it)
                } else {
                    head_product(r, cs, loc, w, done);
                }
                if (p.orth == FgmresPlan::kOrthMgs) orth_mgs(r, loc, w, db, nb, done);
                else if (p.orth == FgmresPlan::kOrthSingle) orth_single(r, cs, loc, w, db, nb, done);
                else orth_cgs(r, loc, w, db, nb, done);
                if (!p.head || p.big) {
                    // Hessenberg column, Givens, convergence -- on the device; then v_{j+1} = w / ||w|| (the head kernel
                    // of the next iteration does that scaling where there is one)
                    k::krylov_givens(c->ka, loc, db, nb, s);
                    if (!p.head) k::scale_dev(w, N, inv_tt, done, s);
                }
            }
            if (o.check_every > 0 && (loc + 1) % o.check_every == 0 && loc + 1 < mk) {
                SPK_HIP(hipMemcpyAsync(&st, c->kst.p, sizeof st, hipMemcpyDeviceToHost, s));
                SPK_HIP(hipStreamSynchronize(s));
                cs.stop = st.done != 0 || st.skip_iter != 0;  // head paths: lags by one iteration, the iterate does not care
            }
        }
        if (finished || (pend_check && read_state())) break;   // (second form: cycles shorter than kAhead iterations)
        // head paths: the Givens step of the cycle's last iteration has no head kernel to ride on
        if (p.head && cs.last >= 0) cs.pend_h = r.dotsbuf(cs.last), cs.pend_n = r.nrmbuf(cs.last), cs.pend_loc = cs.last;
        // ---- x += Z y (KSPFGMRESBuildSoln); always runs, count comes from the device ----
        const k::GivensRider pend{c->ka, cs.pend_loc, cs.pend_h, cs.pend_n, nullptr, nullptr, 0, k::FinErr{nullptr, 0}, k::PeerAR{}};
        k::krylov_cycle_end(c->ka, s, un3 ? c->basis_sc.p : nullptr, mk, cs.pend_loc >= 0 ? &pend : nullptr);
        k::maxpy(r.Z, ld, mk, &c->kst.p->loc_done, c->ka.nrs, 1.0, x, N, 0, c->fin(nullptr), nullptr, s);
        // ---- true residual for the next cycle (KSPFGMRESResidual); skipped once done ----
        op_mult(c, x, c->tmp.p, done);
        // r = b - K x into V0 together with ||r||^2 (and B D r) for the start of the next cycle
        if (p.schur) k::sqnorm_bd(r.r0(), N, n_dot, c->bd.p, ld, r.nl, r.m, r.w1side, c->fin(r.nrmbuf(1)), done, s, b, c->tmp.p);
        else k::sqnorm_sub(b, c->tmp.p, r.r0(), N, n_dot, c->fin(r.nrmbuf(1)), done, s);
        ++cycles;
        SPK_HIP(hipGetLastError());  // a rejected launch inside the cycle surfaces here, not as a wrong answer
    }
    finish_solve(c, st, cycles, t0, c->ka.hist, c->ka.hist_cap, res, history, history_cap);
}

}  // namespace spk
