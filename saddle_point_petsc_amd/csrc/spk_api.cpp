// spk_api.cpp -- the extern "C" surface declared in include/spk.h.
// Argument checks, error capture (exceptions never cross the ABI), staging of
// host vectors.  The work is in spk_operator.cpp (set-up), spk_solver.cpp / spk_k_*.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

#include "spk_internal.hpp"

namespace spk {
void rccl_unique_id(void *id128);
}

#define SPK_TRY(ctx)                                                     \
    if (!(ctx)) return SPK_ERR_ARG;                                      \
    try {                                                                \
        if (hipSetDevice((ctx)->device) != hipSuccess)                   \
            spk::fail(SPK_ERR_HIP, "hipSetDevice(%d) failed", (ctx)->device);

#define SPK_CATCH(ctx)                                                   \
    }                                                                    \
    catch (const spk::Error &e)                                          \
    {                                                                    \
        (ctx)->err = e.msg;                                              \
        return e.code;                                                   \
    }                                                                    \
    catch (const std::exception &e)                                      \
    {                                                                    \
        (ctx)->err = e.what();                                           \
        return SPK_ERR_NOMEM;                                            \
    }                                                                    \
    return SPK_OK;

namespace {
// What the four solver entry points share: the argument checks (norm_type: nullptr for fgmres), the result reset and,
// for host vectors, the staging through the context's rhs / xsol.  run(b, x) solves on device vectors.
template <class Run>
void solve(spk_ctx *c, const char *name, const double *b, double *x, int mem, const spk_opts *opts, const int *norm_type,
           spk_result *result, Run run)
{
    if (!b || !x || !opts || !result) spk::fail(SPK_ERR_ARG, "%s: null argument", name);
    if (!c->have_A) spk::fail(SPK_ERR_STATE, "%s: no operator", name);
    if (!(opts->rtol >= 0) || !(opts->abstol >= 0) || !(opts->dtol > 0) || opts->max_it < 0)
        spk::fail(SPK_ERR_ARG, "%s: tolerances must be non-negative, max_it >= 0", name);
    if (norm_type && *norm_type != SPK_NORM_UNPRECONDITIONED && *norm_type != SPK_NORM_NATURAL)
        spk::fail(SPK_ERR_ARG, "%s: norm_type %d is neither SPK_NORM_UNPRECONDITIONED nor SPK_NORM_NATURAL", name, *norm_type);
    c->ensure_vectors();
    const int64_t N = (int64_t)c->n_local + c->m;
    std::memset(result, 0, sizeof *result);
    if (mem == SPK_MEM_DEVICE) {
        run(b, x);
    } else {
        double *xs = c->xsol.p, *rh = c->rhs.p;
        SPK_HIP(hipMemcpy(rh, b, sizeof(double) * (size_t)N, hipMemcpyHostToDevice));
        if (opts->guess_nonzero) SPK_HIP(hipMemcpy(xs, x, sizeof(double) * (size_t)N, hipMemcpyHostToDevice));
        run(rh, xs);
        SPK_HIP(hipMemcpy(x, xs, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost));
    }
}
}  // namespace

extern "C" {

int spk_version(void) { return SPK_VERSION; }

void spk_default_opts(spk_opts *o)
{
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->restart = 30;
    o->max_it = 10000;
    o->rtol = 1e-5;
    o->abstol = 1e-50;
    o->dtol = 1e4;
    o->guess_nonzero = 0;
    o->orthog = SPK_ORTHOG_CGS;
    o->check_every = 0;
    o->fused = 1;
}

int spk_create(spk_ctx **out, int device)
{
    if (!out) return SPK_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        spk::set_create_error(std::string("spk_create: no HIP device available (") + hipGetErrorString(e) +
                              "); libspk has no CPU fallback");
        return SPK_ERR_HIP;
    }
    if (device < 0 || device >= ndev) {
        spk::set_create_error("spk_create: device index out of range");
        return SPK_ERR_ARG;
    }
    spk_ctx *c = nullptr;
    try {
        c = new spk_ctx();
        c->device = device;
        SPK_HIP(hipSetDevice(device));
        SPK_HIP(hipStreamCreate(&c->stream));
        SPK_HIP(hipDeviceGetAttribute(&c->num_cus, hipDeviceAttributeMultiprocessorCount, device));
        // the solver's state report (pinned block + event): here, not inside the first solve
        SPK_HIP(hipHostMalloc(&c->pin_state, 512, hipHostMallocDefault));
        SPK_HIP(hipEventCreateWithFlags(&c->state_ev, hipEventDisableTiming));
        c->comm.reset(spk::make_self_comm());
        c->ensure_scratch();
    } catch (const spk::Error &er) {
        spk::set_create_error(er.msg);
        delete c;
        return er.code;
    } catch (const std::exception &er) {
        spk::set_create_error(er.what());
        delete c;
        return SPK_ERR_NOMEM;
    }
    *out = c;
    return SPK_OK;
}

int spk_destroy(spk_ctx *c)
{
    if (!c) return SPK_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) {
        (void)hipStreamSynchronize(c->stream);
    }
    c->comm.reset();
    hipStream_t s = c->stream;
    for (int i = 0; i < 2; ++i) {
        if (c->pin[i]) (void)hipHostFree(c->pin[i]);
        if (i == 0 && c->pin_state) (void)hipHostFree(c->pin_state);
        if (i == 0 && c->state_ev) (void)hipEventDestroy(c->state_ev);
        if (c->pin_ev[i]) (void)hipEventDestroy(c->pin_ev[i]);
    }
    for (hipEvent_t e : c->tp_ev) (void)hipEventDestroy(e);
    delete c;  // DevBuf destructors free device memory, SolverWork's destructor its pinned slots and events
    if (s) (void)hipStreamDestroy(s);
    return SPK_OK;
}

const char *spk_last_error(const spk_ctx *c) { return c ? c->err.c_str() : spk::create_error(); }

int spk_comm_unique_id(void *id128)
{
    if (!id128) return SPK_ERR_ARG;
    try {
        spk::rccl_unique_id(id128);
    } catch (const spk::Error &e) {
        spk::set_create_error(e.msg);
        return e.code;
    }
    return SPK_OK;
}

int spk_comm_init_rccl(spk_ctx *c, int rank, int nranks, const void *id128)
{
    SPK_TRY(c)
    if (!id128 || nranks < 1 || rank < 0 || rank >= nranks) spk::fail(SPK_ERR_ARG, "comm_init_rccl: bad rank/nranks");
    if (c->have_A) spk::fail(SPK_ERR_STATE, "comm_init: must precede spk_set_block");
    c->comm.reset(spk::make_rccl_comm(rank, nranks, id128, c->device));
    SPK_CATCH(c)
}

int spk_comm_init_host(spk_ctx *c, int rank, int nranks, const spk_host_comm *cb)
{
    SPK_TRY(c)
    if (!cb || !cb->allreduce || !cb->exchange || !cb->allgather || nranks < 1 || rank < 0 || rank >= nranks)
        spk::fail(SPK_ERR_ARG, "comm_init_host: bad arguments");
    if (c->have_A) spk::fail(SPK_ERR_STATE, "comm_init: must precede spk_set_block");
    c->comm.reset(spk::make_host_comm(rank, nranks, *cb));
    SPK_CATCH(c)
}

int spk_comm_init_local(spk_ctx *c, spk_local_group *grp, int rank)
{
    SPK_TRY(c)
    if (!grp) spk::fail(SPK_ERR_ARG, "comm_init_local: null group");
    if (c->have_A) spk::fail(SPK_ERR_STATE, "comm_init: must precede spk_set_block");
    c->comm.reset(spk::make_local_comm(grp, rank));
    SPK_CATCH(c)
}

int spk_comm_enable_peer(spk_ctx *c, int32_t *enabled)
{
    SPK_TRY(c)
    if (enabled) *enabled = 0;
    if (c->have_A) spk::fail(SPK_ERR_STATE, "comm_enable_peer: must precede spk_set_block");
    const char *off = getenv("SPK_COMM_PEER");
    if (!(off && !strcmp(off, "0")) && c->comm->size() > 1 && strcmp(c->comm->name(), "peer-store") != 0) {
        std::string why;
        spk::Comm *inner = c->comm.release();
        c->comm.reset(spk::make_peer_comm(inner, c->device, &why));  // never throws: returns `inner` when it cannot
        c->err = why;  // informational when the backend stayed off
        c->peer_why = why;
    } else if (off && !strcmp(off, "0")) {
        c->peer_why = "switched off (SPK_COMM_PEER=0)";
    }
    if (enabled) *enabled = strcmp(c->comm->name(), "peer-store") == 0;
    SPK_CATCH(c)
}

const char *spk_comm_backend(const spk_ctx *c) { return c && c->comm ? c->comm->name() : "self"; }

int spk_comm_get_info(spk_ctx *c, spk_comm_info *o)
{
    SPK_TRY(c)
    if (!o) spk::fail(SPK_ERR_ARG, "spk_comm_get_info: null output");
    std::memset(o, 0, sizeof *o);
    o->rank = c->comm->rank();
    o->nranks = c->comm->size();
    o->device = c->device;
    o->window_tier = -1;
    o->halo_mode = c->peers.empty() ? 0 : 3;
    std::snprintf(o->backend, sizeof o->backend, "%s", c->comm->name());
    std::snprintf(o->inner_backend, sizeof o->inner_backend, "%s", c->comm->name());
    std::snprintf(o->why, sizeof o->why, "%s", c->peer_why.c_str());
    c->comm->info(o);  // the peer-store backend fills in the rest
    SPK_CATCH(c)
}

/* Test hook: a P-rank peer-store all-reduce played by P workgroups of ONE launch through P windows of this
 * process (no IPC): checks the window layout for every lane up to kPeerMax = 8 on one device.
 * vals: P x count inputs (row r = rank r's contribution); out: P x count results (every row must hold the
 * same rank-ordered sums). */
int spk_debug_peer_allreduce_loopback(spk_ctx *c, int nranks, int count, int rounds, const double *vals, double *out)
{
    SPK_TRY(c)
    if (!vals || !out || nranks < 1 || nranks > spk::k::kPeerMax || count < 1 || count > 64 || rounds < 1)
        spk::fail(SPK_ERR_ARG, "spk_debug_peer_allreduce_loopback: bad arguments");
    const size_t wbytes = sizeof(unsigned long long) * (size_t)spk::k::kArSlots * nranks * spk::k::kArGranules;
    std::vector<unsigned long long *> win((size_t)nranks, nullptr);
    spk::DevBuf<double> buf;
    spk::DevBuf<int32_t> err;
    buf.alloc((size_t)nranks * 64);
    err.alloc(4);
    auto cleanup = [&]() { for (auto *w : win) if (w) (void)hipFree(w); };
    try {
        for (int r = 0; r < nranks; ++r) {
            if (hipExtMallocWithFlags((void **)&win[(size_t)r], wbytes, hipDeviceMallocUncached) != hipSuccess) {
                (void)hipGetLastError();
                SPK_HIP(hipMalloc((void **)&win[(size_t)r], wbytes));
            }
            SPK_HIP(hipMemset(win[(size_t)r], 0, wbytes));
        }
        std::vector<double> h((size_t)nranks * 64, 0.0);
        for (int round = 0; round < rounds; ++round) {   // walks through every slot, and the wrap
            for (int r = 0; r < nranks; ++r)
                for (int i = 0; i < count; ++i) h[(size_t)r * 64 + i] = vals[(size_t)r * count + i] * (1.0 + round);
            SPK_HIP(hipMemcpy(buf.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
            spk::k::PeerAR a{};
            a.P = nranks;
            a.seq = (uint32_t)(round + 1);
            a.timeout_ms = 3000;
            for (int r = 0; r < nranks; ++r) a.win[r] = win[(size_t)r];
            a.err = err.p;
            spk::k::peer_allreduce_loopback(a, buf.p, count, c->stream);
            SPK_HIP(hipStreamSynchronize(c->stream));
            int32_t e = 0;
            SPK_HIP(hipMemcpy(&e, err.p, sizeof e, hipMemcpyDeviceToHost));
            if (e) spk::fail(SPK_ERR_COMM, "loop-back all-reduce timed out in round %d", round);
            SPK_HIP(hipMemcpy(h.data(), buf.p, h.size() * sizeof(double), hipMemcpyDeviceToHost));
            for (int r = 0; r < nranks; ++r)
                for (int i = 0; i < count; ++i) {
                    const double v = h[(size_t)r * 64 + i] / (1.0 + round);
                    if (round == 0) out[(size_t)r * count + i] = v;
                    else if ((round == 1 && out[(size_t)r * count + i] != v) ||   // x2 is exact: the same bits
                             std::fabs(out[(size_t)r * count + i] - v) > 1e-13 * std::fabs(v) + 1e-300)
                        spk::fail(SPK_ERR_COMM, "loop-back all-reduce: round %d differs from round 0", round);
                }
        }
    } catch (...) {
        cleanup();
        throw;
    }
    cleanup();
    SPK_CATCH(c)
}

int spk_set_block(spk_ctx *c, int which, int64_t row_begin, int32_t nrows_local, int64_t ncols_global,
                  const int32_t *rowptr, const int32_t *colidx, const double *val)
{
    SPK_TRY(c)
    spk::set_block(c, which, row_begin, nrows_local, ncols_global, rowptr, colidx, val);
    SPK_CATCH(c)
}

int spk_set_block_laplace(spk_ctx *c, int mx, int my, const double *kappa, int kappa_mem, int apply_bc, double *f_dev)
{
    SPK_TRY(c)
    spk::set_block_laplace(c, mx, my, 0, kappa, kappa_mem, apply_bc, f_dev);
    SPK_CATCH(c)
}

int spk_assemble_laplace_csr(spk_ctx *c, int mx, int my, int64_t row_begin, int64_t row_end, const double *kappa, int kappa_mem,
                             int apply_bc, int32_t *rowptr, int32_t *colidx, double *val, double *f)
{
    SPK_TRY(c)
    spk::assemble_laplace_csr(c, mx, my, 0, row_begin, row_end, kappa, kappa_mem, apply_bc, rowptr, colidx, val, f);
    SPK_CATCH(c)
}

int spk_set_block_laplace3d(spk_ctx *c, int mx, int my, int mz, const double *kappa, int kappa_mem, int apply_bc, double *f_dev)
{
    SPK_TRY(c)
    spk::set_block_laplace(c, mx, my, spk::laplace_mz3(mx, my, mz), kappa, kappa_mem, apply_bc, f_dev);
    SPK_CATCH(c)
}

int spk_assemble_laplace3d_csr(spk_ctx *c, int mx, int my, int mz, int64_t row_begin, int64_t row_end, const double *kappa,
                               int kappa_mem, int apply_bc, int32_t *rowptr, int32_t *colidx, double *val, double *f)
{
    SPK_TRY(c)
    spk::assemble_laplace_csr(c, mx, my, spk::laplace_mz3(mx, my, mz), row_begin, row_end, kappa, kappa_mem, apply_bc, rowptr, colidx, val, f);
    SPK_CATCH(c)
}

int spk_get_assembly_seconds(const spk_ctx *c, double *seconds)
{
    if (!c || !seconds) return SPK_ERR_ARG;
    *seconds = c->assembly_seconds;
    return SPK_OK;
}

int spk_set_block_constraints(spk_ctx *c, int mx, int my, int mz, double *g_dev)
{
    SPK_TRY(c)
    spk::set_block_constraints(c, mx, my, mz, g_dev);
    SPK_CATCH(c)
}

int spk_assemble_constraints_csr(spk_ctx *c, int mx, int my, int mz, int64_t row_begin, int64_t row_end, int32_t *b_colidx, double *b_val,
                                 int32_t *bt_rowptr, int32_t *bt_colidx, double *bt_val, int32_t *win, int32_t *nwin, int32_t *winptr,
                                 int64_t winptr_cap)
{
    SPK_TRY(c)
    spk::assemble_constraints_csr(c, mx, my, mz, row_begin, row_end, b_colidx, b_val, bt_rowptr, bt_colidx, bt_val, win, nwin, winptr,
                                  winptr_cap);
    SPK_CATCH(c)
}

int spk_host_constraints_csr(int mx, int my, int mz, int64_t row_begin, int64_t row_end, int32_t *b_colidx, double *b_val,
                             int32_t *bt_rowptr, int32_t *bt_colidx, double *bt_val, int32_t *win, int32_t *nwin, int32_t *winptr,
                             int64_t winptr_cap)
{
    try {
        spk::host_constraints_csr(mx, my, mz, row_begin, row_end, b_colidx, b_val, bt_rowptr, bt_colidx, bt_val, win, nwin, winptr,
                                  winptr_cap);
    } catch (const spk::Error &e) {
        return e.code;
    } catch (const std::exception &) {
        return SPK_ERR_NOMEM;
    }
    return SPK_OK;
}

int spk_get_constraints_seconds(const spk_ctx *c, double *seconds)
{
    if (!c || !seconds) return SPK_ERR_ARG;
    *seconds = c->constraints_seconds;
    return SPK_OK;
}

int spk_pc_setup(spk_ctx *c, int pc_type, int schur_fact)
{
    SPK_TRY(c)
    spk::pc_setup(c, pc_type, schur_fact);
    SPK_CATCH(c)
}

int spk_pc_set_inner(spk_ctx *c, int sweeps, double omega)
{
    SPK_TRY(c)
    if (sweeps < 0 || sweeps > 64 || !(omega > 0.0) || !(omega < 2.0)) spk::fail(SPK_ERR_ARG, "pc_set_inner: sweeps in [0,64], omega in (0,2)");
    if (sweeps > 0 && c->amg_on)
        spk::fail(SPK_ERR_UNSUPPORTED, "pc_set_inner: the multigrid preconditioner is set (spk_pc_set_amg); one inner solve "
                  "stands for A^-1, not two -- call spk_pc_set_amg(ctx, NULL) first");
    c->inner_sweeps = sweeps;
    c->inner_omega = omega;
    c->pc_ready = false;
    SPK_CATCH(c)
}

int spk_pc_set_amg(spk_ctx *c, const spk_amg_opts *o)
{
    SPK_TRY(c)
    if (o) {
        spk::amg_check_opts(*o);
        if (c->inner_sweeps > 0)
            spk::fail(SPK_ERR_UNSUPPORTED, "pc_set_amg: the FP32 inner sweeps are set (spk_pc_set_inner); one inner solve "
                      "stands for A^-1, not two -- call spk_pc_set_inner(ctx, 0, omega) first");
        c->amg_opts = *o;
    }
    c->amg_on = o != nullptr;
    c->pc_ready = false;
    SPK_CATCH(c)
}

// both set-up routes leave c->amg_d behind
static void need_amg(const spk_ctx *c)
{
    if (!c->amg_d || !c->pc_ready) spk::fail(SPK_ERR_STATE, "no multigrid hierarchy: spk_pc_set_amg, then spk_pc_setup");
}

int spk_get_amg_info(const spk_ctx *cc, spk_amg_info *info)
{
    spk_ctx *c = const_cast<spk_ctx *>(cc);
    SPK_TRY(c)
    if (!info) spk::fail(SPK_ERR_ARG, "null output");
    need_amg(c);
    *info = c->amg_d->info;
    SPK_CATCH(c)
}

int spk_get_amg_level(const spk_ctx *cc, int level, int which, int32_t *nrows, int32_t *ncols, int64_t *nnz,
                      int32_t *rowptr, int32_t *colidx, double *val)
{
    spk_ctx *c = const_cast<spk_ctx *>(cc);
    SPK_TRY(c)
    need_amg(c);
    spk::amg_ctx_level(c, level, which, {nrows, ncols, nnz, rowptr, colidx, val});
    SPK_CATCH(c)
}

int spk_get_amg_aggregates(const spk_ctx *cc, int level, int32_t *nnodes, int32_t *agg)
{
    spk_ctx *c = const_cast<spk_ctx *>(cc);
    SPK_TRY(c)
    need_amg(c);
    spk::amg_ctx_aggregates(c, level, nnodes, agg);
    SPK_CATCH(c)
}

int spk_debug_amg_transfer(spk_ctx *c, int level, int which, int stored, int64_t fine_len, const double *a, const double *b,
                           double *out)
{
    SPK_TRY(c)
    if (!a || !b || !out) spk::fail(SPK_ERR_ARG, "debug_amg_transfer: null pointer");
    need_amg(c);
    spk::amg_debug_transfer(c, level, which, stored, fine_len, a, b, out);
    SPK_CATCH(c)
}

int spk_debug_amg_operator(spk_ctx *c, int level, int which, int stencil, double alpha, double beta, const double *x,
                           const double *xo, const double *b, double *out)
{
    SPK_TRY(c)
    if (!x || !out || (!b && (which & 1))) spk::fail(SPK_ERR_ARG, "debug_amg_operator: null pointer");
    need_amg(c);
    spk::amg_debug_operator(c, level, which, stencil, alpha, beta, x, xo, b, out);
    SPK_CATCH(c)
}

int spk_debug_amg_operator_f32(spk_ctx *c, int level, int which, float alpha, float beta, const float *x, const float *xo,
                               const float *b, float *out)
{
    SPK_TRY(c)
    if (!x || !out || (!b && (which & 1))) spk::fail(SPK_ERR_ARG, "debug_amg_operator_f32: null pointer");
    need_amg(c);
    spk::amg_debug_operator_f32(c, level, which, alpha, beta, x, xo, b, out);
    SPK_CATCH(c)
}

int spk_debug_amg_transfer_f32(spk_ctx *c, int level, int which, int64_t fine_len, const void *a, const void *b, void *out)
{
    SPK_TRY(c)
    if (!a || !b || !out) spk::fail(SPK_ERR_ARG, "debug_amg_transfer_f32: null pointer");
    need_amg(c);
    spk::amg_debug_transfer_f32(c, level, which, fine_len, a, b, out);
    SPK_CATCH(c)
}

int spk_debug_amg_lanczos(spk_ctx *c, int level, int resident, int32_t *steps, double *al, double *be)
{
    SPK_TRY(c)
    if (!steps || !al || !be) spk::fail(SPK_ERR_ARG, "debug_amg_lanczos: null pointer");
    need_amg(c);
    spk::amg_debug_lanczos(c, level, resident, steps, al, be);
    SPK_CATCH(c)
}

int spk_pc_set_amg_reuse(spk_ctx *c, int reuse)
{
    SPK_TRY(c)
    c->amg_reuse = reuse != 0;
    if (!c->amg_reuse) spk::amg_drop_reuse(c);   // the pattern copy and the refresh's buffers go; the hierarchy stays
    SPK_CATCH(c)
}

int spk_get_amg_reuse_info(const spk_ctx *cc, int32_t *refreshed, double *seconds)
{
    spk_ctx *c = const_cast<spk_ctx *>(cc);
    SPK_TRY(c)
    need_amg(c);
    if (refreshed) *refreshed = c->amg_refreshed ? 1 : 0;
    if (seconds) *seconds = c->amg_reuse_seconds;
    SPK_CATCH(c)
}

int spk_pc_set_schur_pre(spk_ctx *c, int pre)
{
    SPK_TRY(c)
    if (pre != SPK_SCHUR_PRE_SELFP_DIAG && pre != SPK_SCHUR_PRE_FULL) spk::fail(SPK_ERR_ARG, "pc_set_schur_pre: unknown value %d", pre);
    if (pre != c->schur_pre) c->pc_ready = false;
    c->schur_pre = pre;
    SPK_CATCH(c)
}

int spk_get_schur_matrix(spk_ctx *c, double *S)
{
    SPK_TRY(c)
    if (!S) spk::fail(SPK_ERR_ARG, "null output");
    if (!c->pc_ready || !c->schur_dense)
        spk::fail(SPK_ERR_STATE, "no dense Schur complement: spk_pc_set_schur_pre(ctx, SPK_SCHUR_PRE_FULL), then spk_pc_setup "
                  "with SPK_PC_SCHUR");
    std::copy(c->schur_S.begin(), c->schur_S.end(), S);
    SPK_CATCH(c)
}

int spk_get_schur_setup_seconds(const spk_ctx *c, double *seconds)
{
    if (!c || !seconds) return SPK_ERR_ARG;
    *seconds = c->schur_dense ? c->schur_setup_seconds : 0.0;
    return SPK_OK;
}

int spk_get_schur_diag(spk_ctx *c, double *shat)
{
    SPK_TRY(c)
    if (!shat) spk::fail(SPK_ERR_ARG, "null output");
    if (!c->pc_ready || c->m == 0 || !c->shat.p) spk::fail(SPK_ERR_STATE, "no Schur data: call spk_pc_setup with the A10 block set");
    SPK_HIP(hipMemcpy(shat, c->shat.p, sizeof(double) * (size_t)c->m, hipMemcpyDeviceToHost));
    SPK_CATCH(c)
}

int spk_get_jacobi_diag(spk_ctx *c, double *dinv)
{
    SPK_TRY(c)
    if (!dinv) spk::fail(SPK_ERR_ARG, "null output");
    if (!c->pc_ready) spk::fail(SPK_ERR_STATE, "call spk_pc_setup first");
    SPK_HIP(hipMemcpy(dinv, c->dinv.p, sizeof(double) * (size_t)c->n_local, hipMemcpyDeviceToHost));
    SPK_CATCH(c)
}

int spk_get_bd_planes(const spk_ctx *c, int32_t *planes)
{
    if (!c || !planes) return SPK_ERR_ARG;
    *planes = !c->bd.p || c->schur_dense ? 0 : (c->bd_packed ? c->m / 2 : c->m);   // (a dense S keeps its W there: not the fused path)
    return SPK_OK;
}

int spk_get_constraint_layout(const spk_ctx *c, int32_t *general, int32_t *m_wide, int32_t wide_rows[8], int32_t *win,
                              int32_t *nwin, int32_t *bc_tiles, int32_t *bt_tiles)
{
    if (!c) return SPK_ERR_ARG;
    if (general) *general = c->b_general ? 1 : 0;
    if (m_wide) *m_wide = c->m_wide;
    if (wide_rows)
        for (int r = 0; r < 8; ++r) wide_rows[r] = r < (int)c->wide_rows_h.size() ? c->wide_rows_h[(size_t)r] : -1;
    if (win) *win = c->B.win;
    if (nwin) *nwin = c->B.nwin;
    if (bc_tiles) *bc_tiles = c->Bc.ntiles;
    if (bt_tiles) *bt_tiles = c->Bt.ntiles;
    return SPK_OK;
}

int spk_get_sizes(const spk_ctx *c, int64_t *n_global, int32_t *n_local, int32_t *m, int64_t *nnz_local,
                  int32_t *n_ghost)
{
    if (!c) return SPK_ERR_ARG;
    if (n_global) *n_global = c->n_global;
    if (n_local) *n_local = c->n_local;
    if (m) *m = c->m;
    if (nnz_local) *nnz_local = c->Ad.nnz + c->Ao.nnz;
    if (n_ghost) *n_ghost = c->n_ghost;
    return SPK_OK;
}

int spk_get_spmv_info(const spk_ctx *c, int32_t *format, int64_t *layout_bytes)
{
    if (!c) return SPK_ERR_ARG;
    const bool dict = c->spmv_format != 0 && c->Adict.ok;
    if (format) *format = dict ? 2 + c->spmv_format : c->spmv_format;
    if (layout_bytes) {
        const int64_t n = c->n_local;
        *layout_bytes = dict                  ? c->Adict.code_bytes + 2 * (int64_t)c->Adict.nbrows + c->Adict.lds_bytes + 16 * n
                        : c->spmv_format == 1 ? 36 * c->Ab.nblocks + 4 * ((int64_t)c->Ab.nbrows + 1) + 16 * n
                        : c->spmv_format == 2 ? 76 * c->Ab3.nblocks + 4 * ((int64_t)c->Ab3.nbrows + 1) + 16 * n
                                              : 12 * c->Ad.nnz + 4 * (n + 1) + 16 * n;
    }
    return SPK_OK;
}

int spk_debug_dict_layout(const spk_ctx *c, int32_t out[12])
{
    if (!c || !out) return SPK_ERR_ARG;
    std::fill(out, out + 12, 0);
    const spk::DictDev &D = c->Adict;
    if (c->spmv_format == 0 || !D.ok) return SPK_OK;
    const int32_t v[12] = {1, D.bs, D.nbrows, D.kmax, D.ntype, D.nclass, D.lds_bytes, D.uniform ? 1 : 0, D.straddle ? 1 : 0, D.uniform3,
                           spk::k::dict_product_kernel(D), spk::k::dict_chunks_per_wg(D)};
    std::copy(v, v + 12, out);
    return SPK_OK;
}

int spk_get_iteration_form(const spk_ctx *c, int32_t *form, int32_t *single_reduce)
{
    if (!c) return SPK_ERR_ARG;
    if (form) *form = c->last_form;
    if (single_reduce) *single_reduce = c->last_single;
    return SPK_OK;
}

int spk_get_gs_launch(const spk_ctx *c, int32_t *launches, int32_t *tail)
{
    if (!c) return SPK_ERR_ARG;
    if (launches) *launches = c->last_gs_launches;
    if (tail) *tail = c->last_gs_tail;
    return SPK_OK;
}

int spk_get_basis_info(const spk_ctx *c, int32_t *precision, int64_t *basis_bytes)
{
    if (!c) return SPK_ERR_ARG;
    if (precision) *precision = c->last_basis;
    if (basis_bytes) *basis_bytes = c->last_basis_bytes;
    return SPK_OK;
}

int spk_get_spmv_models(const spk_ctx *c, int64_t *csr_bytes, int64_t *blocked_bytes, int64_t *dict_bytes, int32_t *npat,
                        int32_t *nblk)
{
    if (!c) return SPK_ERR_ARG;
    const int64_t n = c->n_local;
    if (csr_bytes) *csr_bytes = 12 * c->Ad.nnz + 4 * (n + 1) + 16 * n;
    if (blocked_bytes)
        *blocked_bytes = c->Ab.ok ? 36 * c->Ab.nblocks + 4 * ((int64_t)c->Ab.nbrows + 1) + 16 * n
                         : c->Ab3.ok ? 76 * c->Ab3.nblocks + 4 * ((int64_t)c->Ab3.nbrows + 1) + 16 * n : 0;
    if (dict_bytes) *dict_bytes = c->Adict.ok ? c->Adict.code_bytes + 2 * (int64_t)c->Adict.nbrows + c->Adict.lds_bytes + 16 * n : 0;
    if (npat) *npat = c->Adict.ok ? c->Adict.ntype : 0;
    if (nblk) *nblk = c->Adict.ok ? c->Adict.nclass : 0;
    return SPK_OK;
}

// stage a host vector into a zero-padded device buffer / pass a device pointer through
static const double *stage_in(spk_ctx *c, const double *p, int mem, spk::DevBuf<double> &buf, int64_t n)
{
    if (mem == SPK_MEM_DEVICE) return p;
    SPK_HIP(hipMemcpyAsync(buf.p, p, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    return buf.p;
}

int spk_mult(spk_ctx *c, const double *x, double *y, int mem)
{
    SPK_TRY(c)
    if (!x || !y) spk::fail(SPK_ERR_ARG, "spk_mult: null vector");
    if (!c->have_A) spk::fail(SPK_ERR_STATE, "spk_mult: no operator");
    c->ensure_vectors();
    const int64_t N = (int64_t)c->n_local + c->m;
    const double *xd = stage_in(c, x, mem, c->stage_x, N);
    double *yd = mem == SPK_MEM_DEVICE ? y : c->stage_y.p;
    spk::op_mult(c, xd, yd, nullptr);
    SPK_HIP(hipGetLastError());
    if (mem != SPK_MEM_DEVICE) SPK_HIP(hipMemcpyAsync(y, yd, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, c->stream));
    SPK_HIP(hipStreamSynchronize(c->stream));
    c->comm->check(c->stream);
    c->check_device_error();
    SPK_CATCH(c)
}

int spk_pc_apply(spk_ctx *c, const double *x, double *y, int mem)
{
    SPK_TRY(c)
    if (!x || !y) spk::fail(SPK_ERR_ARG, "spk_pc_apply: null vector");
    if (!c->pc_ready) spk::fail(SPK_ERR_STATE, "spk_pc_apply: call spk_pc_setup first");
    const int64_t N = (int64_t)c->n_local + c->m;
    const double *xd = stage_in(c, x, mem, c->stage_x, N);
    double *yd = mem == SPK_MEM_DEVICE ? y : c->stage_y.p;
    spk::op_pc_apply(c, xd, yd, nullptr);
    SPK_HIP(hipGetLastError());
    if (mem != SPK_MEM_DEVICE) SPK_HIP(hipMemcpyAsync(y, yd, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, c->stream));
    SPK_HIP(hipStreamSynchronize(c->stream));
    c->comm->check(c->stream);
    c->check_device_error();
    SPK_CATCH(c)
}

int spk_fgmres(spk_ctx *c, const double *b, double *x, int mem, const spk_opts *opts, spk_result *result,
               double *history, int32_t history_cap)
{
    SPK_TRY(c)
    solve(c, "spk_fgmres", b, x, mem, opts, nullptr, result,
          [&](const double *bd, double *xd) { spk::fgmres(c, bd, xd, *opts, result, history, history_cap); });
    SPK_CATCH(c)
}

int spk_minres(spk_ctx *c, const double *b, double *x, int mem, const spk_opts *opts, int norm_type, spk_result *result,
               double *history, int32_t history_cap)
{
    SPK_TRY(c)
    solve(c, "spk_minres", b, x, mem, opts, &norm_type, result,
          [&](const double *bd, double *xd) { spk::minres(c, bd, xd, *opts, norm_type, result, history, history_cap); });
    SPK_CATCH(c)
}

int spk_pipecg(spk_ctx *c, const double *b, double *x, int mem, const spk_opts *opts, int norm_type, spk_result *result,
               double *history, int32_t history_cap)
{
    SPK_TRY(c)
    solve(c, "spk_pipecg", b, x, mem, opts, &norm_type, result,
          [&](const double *bd, double *xd) { spk::pipecg(c, bd, xd, *opts, norm_type, result, history, history_cap); });
    SPK_CATCH(c)
}

int spk_pipecgrr(spk_ctx *c, const double *b, double *x, int mem, const spk_opts *opts, int norm_type, spk_result *result,
                 double *history, int32_t history_cap, int32_t *replacements)
{
    SPK_TRY(c)
    int32_t nrep = 0;
    solve(c, "spk_pipecgrr", b, x, mem, opts, &norm_type, result, [&](const double *bd, double *xd) {
        spk::pipecgrr(c, bd, xd, *opts, norm_type, c->pc_tau, result, history, history_cap, &nrep);
    });
    if (replacements) *replacements = nrep;
    SPK_CATCH(c)
}

int spk_pipecgrr_set_tau(spk_ctx *c, double tau)
{
    SPK_TRY(c)
    if (!(tau >= 0.0) || !std::isfinite(tau)) spk::fail(SPK_ERR_ARG, "spk_pipecgrr_set_tau: tau = %g must be >= 0 and finite", tau);
    c->pc_tau = tau;
    SPK_CATCH(c)
}

int spk_debug_finish_timeout(spk_ctx *c, int timeout_ms)
{
    SPK_TRY(c)
    if (timeout_ms < 1 || timeout_ms > 4000) spk::fail(SPK_ERR_ARG, "spk_debug_finish_timeout: 1..4000 ms");
    c->ensure_scratch();
    const uint32_t keep = c->fin_ticks;
    c->fin_ticks = (uint32_t)timeout_ms * 100000u;
    spk::k::finish_probe(c->fin(c->small.p + 500), c->stream);
    c->fin_ticks = keep;
    SPK_HIP(hipStreamSynchronize(c->stream));
    c->check_device_error();  // throws SPK_ERR_HIP: that is the expected outcome
    SPK_CATCH(c)
}

int spk_debug_wave_sums(spk_ctx *c, int na, const double *in, double *out)
{
    SPK_TRY(c)
    if (!in || !out) spk::fail(SPK_ERR_ARG, "spk_debug_wave_sums: null argument");
    if (na < 9 || na > 41 || (na - 1) % 8) spk::fail(SPK_ERR_ARG, "spk_debug_wave_sums: na = %d is none of 9, 17, 25, 33, 41", na);
    spk::DevBuf<double> din, dout;
    din.upload(in, (size_t)na * 512);
    dout.alloc((size_t)16 * na);
    spk::k::wave_sums_probe(na, din.p, dout.p, c->stream);
    SPK_HIP(hipStreamSynchronize(c->stream));
    SPK_HIP(hipMemcpy(out, dout.p, (size_t)16 * na * sizeof(double), hipMemcpyDeviceToHost));
    SPK_CATCH(c)
}

// ---- Gram-Schmidt kernel hooks: host arrays in, the production wrapper, results out -------------------------------
namespace {
int64_t dbg_ld(int64_t n) { return (n + 255) / 256 * 256; }
// rows of n entries -> device rows of stride ld, entries [n, ld) = pad (one slack row of zeros behind the last)
void dbg_upload(spk::DevBuf<double> &d, const double *h, int rows, int64_t n, int64_t ld, double pad)
{
    d.alloc_raw((size_t)ld * (size_t)std::max(rows, 1), 256);
    std::vector<double> row((size_t)ld, pad);
    for (int i = 0; i < std::max(rows, 1); ++i) {
        if (i < rows && h) std::memcpy(row.data(), h + (size_t)i * (size_t)n, sizeof(double) * (size_t)n);
        SPK_HIP(hipMemcpy(d.p + (size_t)ld * i, row.data(), sizeof(double) * (size_t)ld, hipMemcpyHostToDevice));
    }
}
void dbg_fill(spk::DevBuf<double> &d, size_t count, double v)
{
    std::vector<double> h(count, v);
    d.upload(h.data(), count, 8);
}
// done: -1 -> null, else a device word holding the value
const int32_t *dbg_done(spk::DevBuf<int32_t> &d, int32_t done)
{
    if (done < 0) return nullptr;
    d.upload(&done, 1, 3);
    return d.p;
}
}  // namespace

int spk_debug_vec_shape(spk_ctx *c, int64_t n, int32_t *out)
{
    SPK_TRY(c)
    if (!out || n <= 0) spk::fail(SPK_ERR_ARG, "spk_debug_vec_shape: bad arguments");
    spk::k::vec_shapes_probe(n, out);
    SPK_CATCH(c)
}

int spk_debug_mdot(spk_ctx *c, const spk_debug_mdot_opts *o, const double *V, const double *V2, const double *w, double *out)
{
    SPK_TRY(c)
    if (!o || !w || !out || o->n <= 0 || o->n_dot < 0 || o->n_dot > o->n || o->nv < 0 || o->nv2 < 0 ||
        o->nv + o->nv2 > spk::k::kMaxNv - 1 || (o->nv && !V) || (o->nv2 && !V2) || (o->split && (o->nv2 & 1)) || o->done > 1)
        spk::fail(SPK_ERR_ARG, "spk_debug_mdot: bad arguments");
    c->ensure_scratch();
    const int64_t n = o->n, ld = dbg_ld(n);
    const int rows2 = o->split ? o->nv2 / 2 : o->nv2, k = o->nv + o->nv2 + 1;
    spk::DevBuf<double> dV, dV2, dw, dout;
    spk::DevBuf<int32_t> ddone;
    dbg_upload(dV, V, o->nv, n, ld, o->pad);
    dbg_upload(dV2, V2, rows2, n, ld, o->pad);
    dbg_upload(dw, w, 1, n, ld, o->pad);
    dbg_fill(dout, (size_t)k, SPK_DEBUG_MARKER);
    const int32_t *done = dbg_done(ddone, o->done);
    spk::k::mdot(dV.p, ld, o->nv, dw.p, n, o->n_dot, c->fin(dout.p), done, c->stream, o->nv2 ? dV2.p : nullptr, o->nv2, o->split);
    SPK_HIP(hipStreamSynchronize(c->stream));
    c->check_device_error();
    SPK_HIP(hipMemcpy(out, dout.p, sizeof(double) * (size_t)k, hipMemcpyDeviceToHost));
    SPK_CATCH(c)
}

int spk_debug_mdot_f32(spk_ctx *c, const spk_debug_mdot_opts *o, const float *V, const double *V2, const double *w, double *out)
{
    SPK_TRY(c)
    if (!o || !w || !out || o->n <= 0 || o->n_dot < 0 || o->n_dot > o->n || o->nv < 0 || o->nv2 < 0 || o->nv2 > 8 ||
        o->nv + 2 * o->nv2 > spk::k::kMaxNv - 1 || (o->nv && !V) || (o->nv2 && !V2) || (o->split && (o->nv2 & 1)) || o->done > 1)
        spk::fail(SPK_ERR_ARG, "spk_debug_mdot_f32: bad arguments");
    c->ensure_scratch();
    const int64_t n = o->n, ld = dbg_ld(n);
    const int rows2 = o->split ? o->nv2 / 2 : o->nv2, k = o->nv + 2 * o->nv2 + 1;
    spk::DevBuf<float> dV;
    spk::DevBuf<double> dV2, dw, dout;
    spk::DevBuf<int32_t> ddone;
    {   // rows of n floats -> device rows of stride ld floats, entries [n, ld) = pad
        dV.alloc_raw((size_t)ld * (size_t)std::max(o->nv, 1), 256);
        std::vector<float> row((size_t)ld, (float)o->pad);
        for (int i = 0; i < std::max(o->nv, 1); ++i) {
            if (i < o->nv) std::memcpy(row.data(), V + (size_t)i * (size_t)n, sizeof(float) * (size_t)n);
            SPK_HIP(hipMemcpy(dV.p + (size_t)ld * i, row.data(), sizeof(float) * (size_t)ld, hipMemcpyHostToDevice));
        }
    }
    dbg_upload(dV2, V2, rows2, n, ld, o->pad);
    dbg_upload(dw, w, 1, n, ld, o->pad);
    dbg_fill(dout, (size_t)k, SPK_DEBUG_MARKER);
    const int32_t *done = dbg_done(ddone, o->done);
    spk::k::mdot_f32(dV.p, ld, o->nv, dw.p, n, o->n_dot, c->fin(dout.p), done, c->stream, o->nv2 ? dV2.p : nullptr, ld, o->nv2, o->split);
    SPK_HIP(hipStreamSynchronize(c->stream));
    c->check_device_error();
    SPK_HIP(hipMemcpy(out, dout.p, sizeof(double) * (size_t)k, hipMemcpyDeviceToHost));
    SPK_CATCH(c)
}

int spk_debug_maxpy(spk_ctx *c, const spk_debug_maxpy_opts *o, const double *V, const double *a, double *w, const double *bd,
                    const double *dots, double *tb, double *red, double *w1side, double *nrm_out)
{
    SPK_TRY(c)
    if (!o || !w || !a || !red || o->n <= 0 || o->n_dot < 0 || o->n_dot > o->n || o->nv < 0 || o->nv > spk::k::kMaxNv - 1 ||
        o->nv_live > o->nv || (o->nv && !V) || o->m < 0 || o->m > 8 || o->bd_mode < 0 || o->bd_mode > 2 ||
        (o->bd_mode && (!bd || o->m == 0)) || (o->bd_mode == 2 && (o->m & 1)) || o->n_bd < 0 || o->n_bd > o->n ||
        (o->w1side && (!w1side || o->n_bd + o->m > o->n)) || (o->pyth && (!dots || !tb || !nrm_out)) || o->done > 1)
        spk::fail(SPK_ERR_ARG, "spk_debug_maxpy: bad arguments");
    c->ensure_scratch();
    const int64_t n = o->n, ld = dbg_ld(n);
    const int m = o->m, rows = o->bd_mode == 2 ? m / 2 : (o->bd_mode == 1 ? m : 0);
    const int live = o->nv_live >= 0 ? o->nv_live : o->nv;
    spk::DevBuf<double> dV, dw, da, dbd, ddots, dtb, dred, dside, dnrm;
    spk::DevBuf<int32_t> ddone, dnv;
    dbg_upload(dV, V, o->nv, n, ld, o->pad);
    dbg_upload(dw, w, 1, n, ld, o->pad);
    dbg_upload(dbd, bd, rows, n, ld, o->pad);
    da.upload(a, (size_t)o->nv, 8);
    dbg_fill(dred, (size_t)(1 + m), SPK_DEBUG_MARKER);
    dbg_fill(dside, (size_t)std::max(m, 1), SPK_DEBUG_MARKER);
    dbg_fill(dnrm, (size_t)(1 + m), SPK_DEBUG_MARKER);
    spk::k::PythArgs py{};
    py.m = -1;
    if (o->pyth) {
        ddots.upload(dots, (size_t)(live + m + 1), 8);
        dtb.upload(tb, (size_t)(o->nv + 1) * 8, 8);
        py = spk::k::PythArgs{m, ddots.p, dtb.p, dnrm.p};
    }
    if (o->nv_live >= 0) dnv.upload(&o->nv_live, 1, 3);
    const int32_t *done = dbg_done(ddone, o->done);
    spk::k::maxpy(dV.p, ld, o->nv, o->nv_live >= 0 ? dnv.p : nullptr, da.p, o->sign, dw.p, n, o->n_dot,
                  c->fin(o->want_norm ? dred.p : nullptr), done, c->stream, rows ? dbd.p : nullptr, ld, o->n_bd, m,
                  o->w1side ? dside.p : nullptr, o->pyth ? &py : nullptr, o->bd_mode == 2);
    SPK_HIP(hipStreamSynchronize(c->stream));
    c->check_device_error();
    SPK_HIP(hipMemcpy(w, dw.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    SPK_HIP(hipMemcpy(red, dred.p, sizeof(double) * (size_t)(1 + m), hipMemcpyDeviceToHost));
    if (w1side && m) SPK_HIP(hipMemcpy(w1side, dside.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost));
    if (o->pyth) {
        SPK_HIP(hipMemcpy(nrm_out, dnrm.p, sizeof(double) * (size_t)(1 + m), hipMemcpyDeviceToHost));
        SPK_HIP(hipMemcpy(tb, dtb.p, sizeof(double) * (size_t)(o->nv + 1) * 8, hipMemcpyDeviceToHost));
    }
    SPK_CATCH(c)
}

int spk_debug_cycle_norm(spk_ctx *c, int64_t n, int64_t n_dot, int64_t n_bd, int32_t m, double pad, double *x, const double *sa,
                         const double *sb, const double *bd, double *red, double *w1side)
{
    SPK_TRY(c)
    if (!x || !red || n <= 0 || n_dot < 0 || n_dot > n || n_bd < 0 || n_bd + m > n || m < 0 || m > 8 || (m && (!bd || !w1side)) ||
        (!sa != !sb))
        spk::fail(SPK_ERR_ARG, "spk_debug_cycle_norm: bad arguments");
    c->ensure_scratch();
    const int64_t ld = dbg_ld(n);
    spk::DevBuf<double> dx, dsa, dsb, dbd, dred, dside;
    dbg_upload(dx, sa ? nullptr : x, 1, n, ld, pad);
    if (sa) {
        dbg_upload(dsa, sa, 1, n, ld, pad);
        dbg_upload(dsb, sb, 1, n, ld, pad);
    }
    dbg_upload(dbd, bd, m, n, ld, pad);
    dbg_fill(dred, (size_t)(1 + m), SPK_DEBUG_MARKER);
    dbg_fill(dside, (size_t)std::max<int>(m, 1), SPK_DEBUG_MARKER);
    spk::k::sqnorm_bd(dx.p, n, n_dot, dbd.p, ld, n_bd, m, dside.p, c->fin(dred.p), nullptr, c->stream, sa ? dsa.p : nullptr,
                      sa ? dsb.p : nullptr);
    SPK_HIP(hipStreamSynchronize(c->stream));
    c->check_device_error();
    SPK_HIP(hipMemcpy(x, dx.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    SPK_HIP(hipMemcpy(red, dred.p, sizeof(double) * (size_t)(1 + m), hipMemcpyDeviceToHost));
    if (m) SPK_HIP(hipMemcpy(w1side, dside.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost));
    SPK_CATCH(c)
}

int spk_debug_schur_w(spk_ctx *c, int64_t nl, int32_t m, int32_t fact, int32_t done, double pad, const double *W, const double *L,
                      const double *x, const double *src, const double *dinv, double *y)
{
    SPK_TRY(c)
    if (!W || !L || !x || !y || nl <= 0 || m < 1 || m > 8 || fact < SPK_SCHUR_DIAG || fact > SPK_SCHUR_FULL || (src && dinv))
        spk::fail(SPK_ERR_ARG, "spk_debug_schur_w: bad arguments");
    c->ensure_scratch();
    const int64_t ld = dbg_ld(nl + m);
    spk::DevBuf<double> dW, dL, dx, dsrc, ddinv, dy;
    spk::DevBuf<int32_t> ddone;
    dbg_upload(dW, W, m, nl, ld, 0.0);   // the planes' contract: zero beyond the local rows
    dL.upload(L, (size_t)m * m, 8);
    dbg_upload(dx, x, 1, nl + m, ld, pad);
    if (src) dbg_upload(dsrc, src, 1, nl, ld, pad);
    if (dinv) dbg_upload(ddinv, dinv, 1, nl, ld, pad);
    dbg_upload(dy, nullptr, 1, nl + m, ld, SPK_DEBUG_MARKER);
    const int32_t *gate = dbg_done(ddone, done);
    const spk::k::SchurW w{dW.p, ld, m, dL.p};
    if (fact == SPK_SCHUR_DIAG || fact == SPK_SCHUR_UPPER) spk::k::schur_w_y1(w, fact, dx.p + nl, dy.p + nl, gate, c->stream);
    else spk::k::schur_w_dot(w, dx.p, nl, dx.p + nl, dy.p + nl, c->fin(nullptr), gate, c->stream);
    if (fact == SPK_SCHUR_UPPER || fact == SPK_SCHUR_FULL)
        spk::k::schur_w_out(w, src ? dsrc.p : dx.p, dinv ? ddinv.p : nullptr, dy.p + nl, dy.p, nl, gate, c->stream);
    SPK_HIP(hipStreamSynchronize(c->stream));
    c->check_device_error();
    SPK_HIP(hipMemcpy(y, dy.p, sizeof(double) * (size_t)ld, hipMemcpyDeviceToHost));
    SPK_CATCH(c)
}

int spk_debug_pack_bd(spk_ctx *c, int64_t n, int32_t m, const double *bd, double *bdp, int32_t *bad)
{
    SPK_TRY(c)
    if (!bd || !bad || n <= 0 || m < 1 || m > 8 || (m > 1 && !bdp)) spk::fail(SPK_ERR_ARG, "spk_debug_pack_bd: bad arguments");
    const int64_t ld = dbg_ld(n);
    spk::DevBuf<double> dbd, dbdp;
    spk::DevBuf<int32_t> dbad;
    dbg_upload(dbd, bd, m, n, ld, 0.0);
    dbg_upload(dbdp, nullptr, m / 2, n, ld, SPK_DEBUG_MARKER);
    dbad.alloc(4);
    spk::k::pack_bd(dbd.p, ld, n, m, dbdp.p, dbad.p, c->stream);
    SPK_HIP(hipStreamSynchronize(c->stream));
    for (int q = 0; q < m / 2; ++q)
        SPK_HIP(hipMemcpy(bdp + (size_t)q * (size_t)n, dbdp.p + (size_t)q * ld, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    SPK_HIP(hipMemcpy(bad, dbad.p, sizeof(int32_t), hipMemcpyDeviceToHost));
    SPK_CATCH(c)
}

int spk_debug_cycle_head(spk_ctx *c, const spk_debug_head_opts *o, double *v, const double *nrm, const double *w1raw,
                         const double *dinv, const double *bd, const double *shat, const double *gram, double *z, double *cvec,
                         double *wl)
{
    SPK_TRY(c)
    if (!o || !v || !nrm || !dinv || !z || o->nl < 2 || (o->nl & 1) || o->m < 0 || o->m > 8 || (o->packed && (o->m & 1)) ||
        (o->jacobi ? o->m != 0 : !cvec) || (o->m && (!w1raw || !bd || !shat || !gram)) || (o->want_wl && !wl) ||
        (o->fact != SPK_SCHUR_LOWER && o->fact != SPK_SCHUR_FULL))
        spk::fail(SPK_ERR_ARG, "spk_debug_cycle_head: bad arguments");
    const int64_t nl = o->nl, n = nl + o->m, ld = dbg_ld(n);
    const int m = o->m, rows = o->packed ? m / 2 : m;
    spk::DevBuf<double> dv, dz, dc, ddinv, dbd, dnrm, dw1, dshat, dgram, dwl;
    spk::DevBuf<int32_t> ddone;
    dbg_upload(dv, v, 1, n, ld, o->pad);
    dbg_upload(dz, nullptr, 1, n, ld, SPK_DEBUG_MARKER);
    dbg_upload(dc, nullptr, 1, n, ld, SPK_DEBUG_MARKER);
    dbg_upload(ddinv, dinv, 1, nl, ld, o->pad);
    {   // the planes cover the nl entries of the A block; what lies behind them is padding
        dbd.alloc_raw((size_t)ld * (size_t)std::max(rows, 1), 256);
        std::vector<double> row((size_t)ld, o->pad);
        for (int i = 0; i < rows; ++i) {
            std::memcpy(row.data(), bd + (size_t)i * (size_t)nl, sizeof(double) * (size_t)nl);
            SPK_HIP(hipMemcpy(dbd.p + (size_t)ld * i, row.data(), sizeof(double) * (size_t)ld, hipMemcpyHostToDevice));
        }
    }
    dnrm.upload(nrm, (size_t)(1 + m), 8);
    dw1.upload(w1raw, (size_t)m, 8);
    dshat.upload(shat, (size_t)m, 8);
    dgram.upload(gram, (size_t)m * m, 8);
    dbg_fill(dwl, (size_t)std::max(m, 1), SPK_DEBUG_MARKER);
    const int32_t *done = dbg_done(ddone, 0);   // the kernel dereferences its gate word unconditionally
    spk::k::fused_head(dv.p, dnrm.p, m ? dw1.p : nullptr, ddinv.p, m ? dbd.p : nullptr, ld, m ? dshat.p : nullptr,
                       m ? dgram.p : nullptr, o->fact, nl, m, dz.p, o->jacobi ? nullptr : dc.p, spk::k::KrylovArrays{}, -1, nullptr,
                       done, c->stream, nullptr, o->packed, o->want_wl ? dwl.p : nullptr);
    SPK_HIP(hipStreamSynchronize(c->stream));
    SPK_HIP(hipMemcpy(v, dv.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    SPK_HIP(hipMemcpy(z, dz.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    if (cvec) SPK_HIP(hipMemcpy(cvec, dc.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    if (o->want_wl && m) SPK_HIP(hipMemcpy(wl, dwl.p, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost));
    SPK_CATCH(c)
}

int spk_debug_gs_stamps(spk_ctx *c, uint64_t *out)
{
    SPK_TRY(c)
    if (!out) spk::fail(SPK_ERR_ARG, "spk_debug_gs_stamps: null argument");
    SPK_HIP(hipStreamSynchronize(c->stream));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "stamps are 64-bit");
    if (!spk::k::gs_stamps(reinterpret_cast<unsigned long long *>(out)))
        spk::fail(SPK_ERR_STATE, "spk_debug_gs_stamps: the library was not built with GS_STAMPS=1");
    SPK_CATCH(c)
}

int spk_debug_set_wait_bound(spk_ctx *c, uint32_t ticks)
{
    if (!c) return SPK_ERR_ARG;
    c->fin_ticks = ticks ? ticks : 400000000u;
    return SPK_OK;
}

int spk_debug_time_products(spk_ctx *c, int32_t max_launches)
{
    SPK_TRY(c)
    SPK_HIP(hipStreamSynchronize(c->stream));
    c->tp_used = 0;
    c->time_products = max_launches > 0;
    const size_t want = max_launches > 0 ? 2 * (size_t)max_launches : 0;
    while (c->tp_ev.size() < want) {
        hipEvent_t e;
        SPK_HIP(hipEventCreate(&e));
        c->tp_ev.push_back(e);
    }
    SPK_CATCH(c)
}

int spk_get_product_timing(spk_ctx *c, int32_t *launches, double *mean_ms, double *median_ms, double *min_ms, double *max_ms,
                           int32_t *gated, double *gated_mean_ms)
{
    SPK_TRY(c)
    SPK_HIP(hipStreamSynchronize(c->stream));
    std::vector<float> t;
    for (size_t i = 0; i + 1 < c->tp_used; i += 2) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, c->tp_ev[i], c->tp_ev[i + 1]) != hipSuccess) {   // (a launch that took no stamps: an
            (void)hipGetLastError();                                                   // empty rank runs the rider alone)
            continue;
        }
        t.push_back(ms);
    }
    std::sort(t.begin(), t.end());
    // (launches the device had gated off -- the iterations the host enqueues ahead of a solve's end return at once -- are
    // not the kernel at work: anything shorter than half the median is left out of the mean and the count)
    const double med = t.empty() ? 0.0 : t[t.size() / 2];
    double sum = 0.0;
    size_t used = 0;
    double lo = 0.0;
    for (float v : t)
        if (v >= 0.5 * med) {
            if (!used) lo = v;
            sum += v;
            ++used;
        }
    double gsum = 0.0;
    size_t ng = 0;
    for (float v : t)
        if (v < 0.5 * med) {
            gsum += v;
            ++ng;
        }
    if (gated) *gated = (int32_t)ng;
    if (gated_mean_ms) *gated_mean_ms = ng ? gsum / (double)ng : 0.0;
    if (launches) *launches = (int32_t)used;
    if (mean_ms) *mean_ms = used ? sum / (double)used : 0.0;
    if (median_ms) *median_ms = med;
    if (min_ms) *min_ms = lo;
    if (max_ms) *max_ms = t.empty() ? 0.0 : t.back();
    SPK_CATCH(c)
}

int spk_vec_create(spk_ctx *c, int64_t n, double **dev)
{
    SPK_TRY(c)
    if (!dev || n < 0) spk::fail(SPK_ERR_ARG, "spk_vec_create: bad arguments");
    const size_t len = (size_t)((n + 255) / 256 * 256 + 256);
    SPK_HIP(hipMalloc((void **)dev, len * sizeof(double)));
    SPK_HIP(hipMemset(*dev, 0, len * sizeof(double)));
    SPK_CATCH(c)
}

int spk_vec_destroy(spk_ctx *c, double *dev)
{
    SPK_TRY(c)
    if (dev) SPK_HIP(hipFree(dev));
    SPK_CATCH(c)
}

int spk_vec_set(spk_ctx *c, double *dev, const double *host, int64_t n)
{
    SPK_TRY(c)
    if (!dev || !host || n < 0) spk::fail(SPK_ERR_ARG, "spk_vec_set: bad arguments");
    SPK_HIP(hipMemcpy(dev, host, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    SPK_CATCH(c)
}

int spk_vec_get(spk_ctx *c, const double *dev, double *host, int64_t n)
{
    SPK_TRY(c)
    if (!dev || !host || n < 0) spk::fail(SPK_ERR_ARG, "spk_vec_get: bad arguments");
    SPK_HIP(hipStreamSynchronize(c->stream));
    SPK_HIP(hipMemcpy(host, dev, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    SPK_CATCH(c)
}

// ---- single kernels through the ABI -----------------------------------------
int spk_kernel_mdot(spk_ctx *c, int64_t n, int32_t nv, const double *V, int64_t ldv, const double *w, double *h)
{
    SPK_TRY(c)
    if (!V || !w || !h || n <= 0 || nv < 0 || nv > spk::k::kMaxNv - 1 || ldv < n)
        spk::fail(SPK_ERR_ARG, "spk_kernel_mdot: bad arguments");
    c->ensure_scratch();
    const int64_t ld = (n + 255) / 256 * 256;
    spk::DevBuf<double> dV, dw;
    dV.alloc((size_t)ld * (size_t)std::max(nv, 1));
    dw.alloc((size_t)ld);
    for (int i = 0; i < nv; ++i)
        SPK_HIP(hipMemcpy(dV.p + (size_t)ld * i, V + (size_t)ldv * i, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    SPK_HIP(hipMemcpy(dw.p, w, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    spk::k::mdot(dV.p, ld, nv, dw.p, n, n, c->fin(c->small.p), nullptr, c->stream);
    SPK_HIP(hipStreamSynchronize(c->stream));
    SPK_HIP(hipMemcpy(h, c->small.p, sizeof(double) * (size_t)(nv + 1), hipMemcpyDeviceToHost));
    SPK_CATCH(c)
}

int spk_kernel_maxpy(spk_ctx *c, int64_t n, int32_t nv, const double *a, const double *V, int64_t ldv,
                     double *w, double *nrm2)
{
    SPK_TRY(c)
    if (!V || !w || !a || n <= 0 || nv < 0 || nv > spk::k::kMaxNv - 1 || ldv < n)
        spk::fail(SPK_ERR_ARG, "spk_kernel_maxpy: bad arguments");
    c->ensure_scratch();
    const int64_t ld = (n + 255) / 256 * 256;
    spk::DevBuf<double> dV, dw, da;
    dV.alloc((size_t)ld * (size_t)std::max(nv, 1));
    dw.alloc((size_t)ld);
    da.upload(a, (size_t)nv, 8);
    for (int i = 0; i < nv; ++i)
        SPK_HIP(hipMemcpy(dV.p + (size_t)ld * i, V + (size_t)ldv * i, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    SPK_HIP(hipMemcpy(dw.p, w, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    spk::k::maxpy(dV.p, ld, nv, nullptr, da.p, 1.0, dw.p, n, n, c->fin(c->small.p), nullptr, c->stream);
    SPK_HIP(hipStreamSynchronize(c->stream));
    SPK_HIP(hipMemcpy(w, dw.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    if (nrm2) SPK_HIP(hipMemcpy(nrm2, c->small.p, sizeof(double), hipMemcpyDeviceToHost));
    SPK_CATCH(c)
}

int spk_time_spmv(spk_ctx *c, int warmup, int reps, double *ms_per_launch)
{
    SPK_TRY(c)
    if (!ms_per_launch || reps < 1 || warmup < 0) spk::fail(SPK_ERR_ARG, "spk_time_spmv: bad arguments");
    if (!c->have_A) spk::fail(SPK_ERR_STATE, "spk_time_spmv: no operator");
    c->ensure_vectors();
    const int64_t N = (int64_t)c->n_local + c->m;
    std::vector<double> hx((size_t)N);
    for (int64_t i = 0; i < N; ++i) hx[(size_t)i] = std::sin(0.37 * (double)(c->row_begin + i));
    SPK_HIP(hipMemcpy(c->stage_x.p, hx.data(), sizeof(double) * (size_t)N, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    SPK_HIP(hipEventCreate(&e0));
    SPK_HIP(hipEventCreate(&e1));
    auto one = [&]() {  // the kernel the solver launches for the A block
        spk::a_mult(c, c->stage_x.p, c->stage_y.p, nullptr, nullptr, nullptr, false, nullptr);
    };
    for (int i = 0; i < warmup; ++i) one();
    SPK_HIP(hipEventRecord(e0, c->stream));
    for (int i = 0; i < reps; ++i) one();
    SPK_HIP(hipEventRecord(e1, c->stream));
    SPK_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    SPK_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *ms_per_launch = (double)ms / reps;
    SPK_CATCH(c)
}

int spk_time_kernel(spk_ctx *c, const char *which, int nv, int warmup, int reps, double *ms_per_launch)
{
    SPK_TRY(c)
    if (!which || !ms_per_launch || reps < 1 || warmup < 0) spk::fail(SPK_ERR_ARG, "spk_time_kernel: bad arguments");
    if (!c->have_A) spk::fail(SPK_ERR_STATE, "spk_time_kernel: no operator");
    if (nv < 0 || nv > spk::k::kMaxNv - 2) spk::fail(SPK_ERR_ARG, "spk_time_kernel: nv out of range");
    c->ensure_scratch();
    c->ensure_vectors();
    const std::string w(which);
    const int64_t N = (int64_t)c->n_local + c->m, ld = c->ld;
    spk::DevBuf<double> V, coef;
    V.alloc((size_t)ld * (size_t)(nv + 2));
    {
        std::vector<double> h((size_t)ld, 0.0);
        for (int j = 0; j < nv + 2; ++j) {
            for (int64_t i = 0; i < N; ++i) h[(size_t)i] = std::sin(0.37 * (double)i + (double)j) * 1e-3;
            SPK_HIP(hipMemcpy(V.p + (size_t)ld * j, h.data(), sizeof(double) * (size_t)ld, hipMemcpyHostToDevice));
        }
        std::vector<double> a((size_t)nv + 8, 1e-6);
        coef.upload(a.data(), a.size(), 8);
    }
    double *x = V.p + (size_t)ld * nv, *y = V.p + (size_t)ld * (nv + 1);
    hipStream_t s = c->stream;
    auto run = [&]() {
        if (w == "spmv") spk::k::spmv(c->Ad, x, y, nullptr, nullptr, nullptr, s);
        else if (w == "spmv_bcsr3") { if (!c->Ab3.ok) spk::fail(SPK_ERR_STATE, "no 3x3-blocked copy"); spk::k::spmv_bcsr3(c->Ab3, x, y, nullptr, nullptr, nullptr, s); }
        else if (w == "spmv_dict") { if (!c->Adict.ok) spk::fail(SPK_ERR_STATE, "no row-type layout"); spk::k::spmv_dict(c->Adict, x, y, nullptr, nullptr, nullptr, s); }
        else if (w == "spmv_bcsr") { if (!c->Ab.ok) spk::fail(SPK_ERR_STATE, "no 2x2-blocked copy"); spk::k::spmv_bcsr(c->Ab, x, y, nullptr, nullptr, nullptr, s); }
        else if (w == "spmv_gated") {
            // the iteration's product launch as the device gates it off (`done` set: every workgroup returns at once)
            spk::k::GivensRider gr{c->ka, 0, c->small.p, c->small.p + 64, nullptr, nullptr, 0, spk::k::FinErr{nullptr, 0}, spk::k::PeerAR{}};
            if (!c->kst.p) spk::fail(SPK_ERR_STATE, "spk_time_kernel: spmv_gated needs the state of a solve");
            spk::a_mult(c, x, y, nullptr, nullptr, &c->kst.p->done, true, nullptr, &gr);
        }
        else if (w == "spmv_acc" || w == "spmv_ride") {
            // y += A x (spmv_ride: y = A x) in the active format, as the default iteration launches it: with the Givens
            // rider in workgroup 0 once a solve has left its state behind (the rider finds `done` set and leaves)
            spk::k::GivensRider gr{c->ka, 0, c->small.p, c->small.p + 64, nullptr, nullptr, 0, spk::k::FinErr{nullptr, 0}, spk::k::PeerAR{}};
            const spk::k::GivensRider *rp = c->kst.p ? &gr : nullptr;
            const bool acc = w == "spmv_acc";
            spk::a_mult(c, x, y, nullptr, nullptr, nullptr, acc, nullptr, rp);
        }
        else if (w == "mult") spk::op_mult(c, x, y, nullptr);
        else if (w == "pc") { if (!c->pc_ready) spk::fail(SPK_ERR_STATE, "pc not set up"); spk::op_pc_apply(c, x, y, nullptr); }
        else if (w == "mdot") spk::k::mdot(V.p, ld, nv, x, N, N, c->fin(c->small.p), nullptr, s);
        else if (w == "maxpy") spk::k::maxpy(V.p, ld, nv, nullptr, coef.p, -1.0, x, N, N, c->fin(c->small.p + 64), nullptr, s);
        else if (w == "maxpy_nonorm") spk::k::maxpy(V.p, ld, nv, nullptr, coef.p, -1.0, x, N, N, c->fin(nullptr), nullptr, s);
        else if (w == "scale") spk::k::scale_dev(x, N, coef.p, nullptr, s);
        else if (w == "wide_dot") { if (!c->have_B) spk::fail(SPK_ERR_STATE, "no B"); spk::k::wide_dot(c->B, x, c->fin(c->small.p), nullptr, s); }
        else if (w == "bt_update") { if (!c->have_B || !c->pc_ready) spk::fail(SPK_ERR_STATE, "no B / pc"); spk::k::bt_update(1, c->Bt, c->dinv.p, x, c->small.p + 200, y, nullptr, s); }
        else spk::fail(SPK_ERR_ARG, "spk_time_kernel: unknown kernel '%s'", which);
    };
    if ((w == "spmv_acc" || w == "spmv_ride" || w == "spmv_gated") && c->kst.p) {
        const int32_t one = 1;   // (krylov_init of the next solve resets it)
        SPK_HIP(hipMemcpyAsync(&c->kst.p->done, &one, sizeof one, hipMemcpyHostToDevice, s));
    }
    hipEvent_t e0, e1;
    SPK_HIP(hipEventCreate(&e0));
    SPK_HIP(hipEventCreate(&e1));
    for (int i = 0; i < warmup; ++i) run();
    SPK_HIP(hipEventRecord(e0, s));
    for (int i = 0; i < reps; ++i) run();
    SPK_HIP(hipEventRecord(e1, s));
    SPK_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    SPK_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *ms_per_launch = (double)ms / reps;
    SPK_CATCH(c)
}

}  // extern "C"
