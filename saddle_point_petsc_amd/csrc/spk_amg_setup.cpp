// spk_amg_setup.cpp -- the multigrid hierarchy of a context: everything that builds, uploads, refreshes or downloads one.
// The hierarchy comes from the context's A00 (single rank: the diagonal block is all of A) by the loops of
// spk_amg_levels.hpp over one of two routes -- spk_amg_host.cpp's, on the host, whose result amg_upload copies to the
// device (the default), or DevRoute here, on the device (-spk_gamg_setup device; kernels: spk_k_amg_setup.hip), with the
// Lanczos scalars read back per step or kept in a state block (-spk_amg_lanczos resident, spk_lanczos_core.hpp).  With
// reuse on (spk_pc_set_amg_reuse) a set-up on an unchanged pattern and unchanged hierarchy options (amg_can_refresh) puts
// the new values of A00 through the kept hierarchy on the route that built it (amg_refresh_ctx).  Every set-up ends in
// the application's plan (amg_plan_cycle, spk_amg_cycle.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "spk_amg.hpp"
#include "spk_amg_levels.hpp"
#include "spk_galerkin_core.hpp"
#include "spk_internal.hpp"

namespace spk {

// the node size the options ask for, else the blocking the context found for its A layout (0: detect from the pattern)
static int ctx_block_size(const spk_ctx *c, const spk_amg_opts &o)
{
    if (o.block_size > 0) return o.block_size;
    if (c->Adict.ok) return c->Adict.bs;
    return c->spmv_format == 1 ? 2 : c->spmv_format == 2 ? 3 : 0;
}

static HostCsr dev_csr_download(const CsrDev &A, bool values, hipStream_t s)
{
    HostCsr H;
    H.nrows = A.nrows;
    H.ncols = A.ncols;
    H.rp.resize((size_t)A.nrows + 1);
    SPK_HIP(hipMemcpyAsync(H.rp.data(), A.rowptr.p, sizeof(int32_t) * H.rp.size(), hipMemcpyDeviceToHost, s));
    SPK_HIP(hipStreamSynchronize(s));
    H.ci.resize((size_t)H.rp[(size_t)A.nrows]);
    H.v.resize(H.ci.size());
    if (!H.ci.empty()) {
        SPK_HIP(hipMemcpyAsync(H.ci.data(), A.colidx.p, sizeof(int32_t) * H.ci.size(), hipMemcpyDeviceToHost, s));
        if (values) SPK_HIP(hipMemcpyAsync(H.v.data(), A.val.p, sizeof(double) * H.v.size(), hipMemcpyDeviceToHost, s));
        SPK_HIP(hipStreamSynchronize(s));
    }
    return H;
}

std::unique_ptr<spk_amg_hier> amg_build_ctx(spk_ctx *c)
{
    spk_amg_opts o = c->amg_opts;
    o.block_size = ctx_block_size(c, o);
    auto h = std::make_unique<spk_amg_hier>();
    amg_build(h->h, dev_csr_download(c->Ad, true, c->stream), o);
    return h;
}

static void upload_host_csr(CsrDev &D, const HostCsr &H)
{
    D.nrows = H.nrows;
    D.ncols = H.ncols;
    D.nnz = H.nnz();
    D.rowptr.upload(H.rp.data(), H.rp.size());
    D.colidx.upload(H.ci.data(), H.ci.size(), 4);
    D.val.upload(H.v.data(), H.v.size(), 4);
}

// reuse on: what the next set-up compares before it refreshes -- the options, the sizes and a device copy of the
// diagonal block's pattern as the context stores it
static void keep_pattern(spk_ctx *c, AmgDev &d)
{
    if (!d.reuse) d.reuse = std::make_unique<AmgReuse>();
    AmgReuse &ru = *d.reuse;
    ru.o = c->amg_opts;
    ru.bs = ctx_block_size(c, c->amg_opts);
    ru.n = c->n_local;
    ru.nnz = c->Ad.nnz;
    ru.ld = c->ld;
    ru.rowptr.alloc_raw((size_t)ru.n + 1);
    ru.colidx.alloc_raw((size_t)ru.nnz);
    ru.flag.alloc(2);
    SPK_HIP(hipMemcpyAsync(ru.rowptr.p, c->Ad.rowptr.p, sizeof(int32_t) * ((size_t)ru.n + 1), hipMemcpyDeviceToDevice, c->stream));
    if (ru.nnz)
        SPK_HIP(hipMemcpyAsync(ru.colidx.p, c->Ad.colidx.p, sizeof(int32_t) * (size_t)ru.nnz, hipMemcpyDeviceToDevice, c->stream));
}

void amg_upload(spk_ctx *c, std::unique_ptr<spk_amg_hier> hp)
{
    const auto t0 = Clock::now();
    const AmgHier &h = hp->h;
    auto d = std::make_unique<AmgDev>();
    const size_t L = h.lv.size();
    std::vector<AmgLevelDev>(L).swap(d->lv);   // (the levels own device buffers: constructed in place, never moved)
    for (size_t l = 0; l < L; ++l) {
        const AmgLevel &H = h.lv[l];
        AmgLevelDev &D = d->lv[l];
        D.n = H.A.nrows;
        if (l > 0) {
            upload_host_csr(D.A, H.A);
            D.dinv.upload(H.dinv.data(), H.dinv.size(), 8);
        }
        if (l + 1 == L) break;
        upload_host_csr(D.P, H.P);
        upload_host_csr(D.R, H.R);
        smoother_coeffs(h.o, H.lo, H.hi, D.alpha, D.beta);
        if (h.info.coarsening == SPK_AMG_COARSEN_GRID) D.grid.set(h.info.dims[l], h.info.dims[l + 1], h.info.block_size, h.o.transfer);
    }
    d->cinv.upload(h.cinv.data(), h.cinv.size());
    alloc_cycle_vectors(*d, c->ld, h.o.precision == SPK_AMG_PRECISION_SINGLE);
    if (c->amg_reuse) keep_pattern(c, *d);
    SPK_HIP(hipDeviceSynchronize());
    d->info = h.info;
    amg_plan_cycle(*d, h.o, c->ld, c->stream);
    d->info.setup_seconds += seconds_since(t0);
    c->amg_d = std::move(d);
    c->amg_h = std::move(hp);
}

// ---------------------------------------------------------------------------
// the device route (-spk_gamg_setup device; kernels: spk_k_amg_setup.hip).  Per level: node graph -> host (the greedy
// aggregation is sequential by definition and runs unchanged, so the aggregates and every pattern are the host
// route's) -> tentative prolongator, Lanczos, the products and transposes as kernels.  Only the graph, the aggregates,
// the Lanczos scalars and the coarsest operator cross the bus.
// ---------------------------------------------------------------------------
namespace {

int32_t scan_counts(const int32_t *cnt, int32_t n, int32_t *out, hipStream_t s)   // out[0..n]; returns out[n]
{
    DevBuf<int32_t> scr;
    scr.alloc_raw((size_t)n / 2048 + 8);
    k::exclusive_scan_i32(cnt, n, out, scr.p, s);
    int32_t tot = 0;
    SPK_HIP(hipMemcpyAsync(&tot, out + n, sizeof tot, hipMemcpyDeviceToHost, s));
    SPK_HIP(hipStreamSynchronize(s));
    return tot;
}

void dev_csr_values(CsrDev &C, int64_t nnz)
{
    C.nnz = nnz;
    C.colidx.alloc_raw((size_t)nnz, 4);
    C.val.alloc_raw((size_t)nnz, 4);
}

void dev_csr_copy(CsrDev &C, const CsrDev &A, hipStream_t s)
{
    C.nrows = A.nrows;
    C.ncols = A.ncols;
    C.rowptr.alloc_raw((size_t)A.nrows + 1, 8);
    dev_csr_values(C, A.nnz);
    SPK_HIP(hipMemcpyAsync(C.rowptr.p, A.rowptr.p, sizeof(int32_t) * ((size_t)A.nrows + 1), hipMemcpyDeviceToDevice, s));
    if (A.nnz) {
        SPK_HIP(hipMemcpyAsync(C.colidx.p, A.colidx.p, sizeof(int32_t) * (size_t)A.nnz, hipMemcpyDeviceToDevice, s));
        SPK_HIP(hipMemcpyAsync(C.val.p, A.val.p, sizeof(double) * (size_t)A.nnz, hipMemcpyDeviceToDevice, s));
    }
}

// C = A B (sorted columns, no entry dropped, each entry summed in A's stored order, then B's)
void dev_spgemm(CsrDev &C, const CsrDev &A, const CsrDev &B, hipStream_t s)
{
    const int32_t n = A.nrows;
    C.nrows = n;
    C.ncols = B.ncols;
    DevBuf<int32_t> bound, off, cnt, sc;
    DevBuf<double> sv;
    DevBuf<unsigned long long> tot;
    bound.alloc_raw((size_t)n, 8);
    off.alloc_raw((size_t)n + 1, 8);
    cnt.alloc_raw((size_t)n, 8);
    tot.alloc(1);
    k::amgs_spgemm_bound(A, B, bound.p, tot.p, s);
    unsigned long long slots = 0;
    SPK_HIP(hipMemcpyAsync(&slots, tot.p, sizeof slots, hipMemcpyDeviceToHost, s));
    SPK_HIP(hipStreamSynchronize(s));
    if (slots > (unsigned long long)INT32_MAX)
        fail(SPK_ERR_UNSUPPORTED, "amg: a sparse product of the device set-up needs %llu scratch slots, more than its 32-bit "
             "offsets address -- use -spk_gamg_setup host", slots);
    scan_counts(bound.p, n, off.p, s);
    sc.alloc_raw((size_t)slots, 4);
    sv.alloc_raw((size_t)slots, 4);
    k::amgs_spgemm_expand(A, B, off.p, sc.p, sv.p, cnt.p, s);
    C.rowptr.alloc_raw((size_t)n + 1, 8);
    dev_csr_values(C, scan_counts(cnt.p, n, C.rowptr.p, s));
    k::amgs_compact(n, off.p, C.rowptr.p, sc.p, sv.p, C.colidx.p, C.val.p, s);
    SPK_HIP(hipStreamSynchronize(s));   // the scratch goes out of scope
}

// C = a A + b diag(scale) B over the union pattern
void dev_add(CsrDev &C, double a, const CsrDev &A, double b, const CsrDev &B, const double *scale, hipStream_t s)
{
    const int32_t n = A.nrows;
    C.nrows = n;
    C.ncols = A.ncols;
    DevBuf<int32_t> cnt;
    cnt.alloc_raw((size_t)n, 8);
    k::amgs_add(a, A, b, B, scale, nullptr, nullptr, nullptr, cnt.p, s);
    C.rowptr.alloc_raw((size_t)n + 1, 8);
    dev_csr_values(C, scan_counts(cnt.p, n, C.rowptr.p, s));
    k::amgs_add(a, A, b, B, scale, C.rowptr.p, C.colidx.p, C.val.p, nullptr, s);
    SPK_HIP(hipStreamSynchronize(s));
}

void dev_transpose(CsrDev &T, const CsrDev &A, hipStream_t s)
{
    T.nrows = A.ncols;
    T.ncols = A.nrows;
    DevBuf<int32_t> cnt, pos;
    cnt.alloc_raw((size_t)T.nrows, 8);
    pos.alloc_raw((size_t)T.nrows, 8);
    SPK_HIP(hipMemsetAsync(cnt.p, 0, sizeof(int32_t) * (size_t)T.nrows, s));
    k::amgs_col_count(A.colidx.p, A.nnz, cnt.p, s);
    T.rowptr.alloc_raw((size_t)T.nrows + 1, 8);
    dev_csr_values(T, scan_counts(cnt.p, T.nrows, T.rowptr.p, s));
    SPK_HIP(hipMemcpyAsync(pos.p, T.rowptr.p, sizeof(int32_t) * (size_t)T.nrows, hipMemcpyDeviceToDevice, s));
    k::amgs_transpose_fill(A, pos.p, T.colidx.p, T.val.p, s);
    k::amgs_sort_rows(T.rowptr.p, T.colidx.p, T.val.p, T.nrows, s);
    SPK_HIP(hipStreamSynchronize(s));
}

// the 30 Lanczos steps of `lanczos` with the level's own product (level 0: the context's layout, else the CSR kernel);
// the two sums of a step come back to the host, which keeps the tridiagonal and the break rule
// tri (the test hook's): the tridiagonal itself;  *reads += the read-backs made
struct LzTri { std::vector<double> al, be; };
void dev_lanczos(spk_ctx *c, const CsrDev *A, int32_t n, int64_t nv, const double *dinv, double *lmin, double *lmax,
                 double a_scale = 1.0, int32_t *reads = nullptr, LzTri *tri = nullptr)
{
    hipStream_t s = c->stream;
    DevBuf<double> sv, q, qp, w, t, aw, res;
    for (DevBuf<double> *b : {&sv, &q, &qp, &w, &t, &aw}) b->alloc((size_t)nv, 16);
    res.alloc(8);
    const k::Finish f = c->fin(res.p);
    auto sum = [&]() {
        double h = 0.0;
        SPK_HIP(hipMemcpyAsync(&h, res.p, sizeof h, hipMemcpyDeviceToHost, s));
        SPK_HIP(hipStreamSynchronize(s));
        if (reads) ++*reads;
        return h;
    };
    k::amgs_lz_init(n, dinv, 1.0 / a_scale, sv.p, q.p, f, s);
    const double nq = std::sqrt(sum());
    k::amgs_lz_scale(n, nq, q.p, sv.p, q.p, t.p, s);
    std::vector<double> al, be{0.0};
    const int kk = (int)std::min<int64_t>(kLanczosSteps, n);
    double *qc = q.p, *qo = qp.p;
    for (int j = 0; j < kk; ++j) {
        if (A) k::amg_spmv(*A, t.p, aw.p, nullptr, s);
        else a_mult(c, t.p, aw.p, nullptr, nullptr, nullptr, false, nullptr);
        k::amgs_lz_dot(n, sv.p, aw.p, a_scale, w.p, qc, f, s);
        const double a = sum();
        al.push_back(a);
        k::amgs_lz_update(n, a, be.back(), qc, qo, w.p, f, s);
        const double nb = std::sqrt(sum());
        if (j + 1 == kk || nb <= 1e-12 * std::fabs(a)) break;
        be.push_back(nb);
        std::swap(qc, qo);
        k::amgs_lz_scale(n, nb, w.p, sv.p, qc, t.p, s);
    }
    c->check_device_error();
    if (tri) tri->al = al, tri->be = be;
    ritz_extremes(al, be, lmin, lmax);
}

// What the resident route (SPK_AMG_LANCZOS_RESIDENT) owns for a whole build or refresh: the six vectors, sized once for
// level 0's padded length, and the state block.  No level allocates; a level clears what it uses (dev_lanczos gets its
// vectors zeroed too: the first update reads qp, and level 0's product reads t over the padded length).
struct LzWork {
    DevBuf<double> v;
    DevBuf<lanczos_core::LzState> st;
    size_t cap = 0;   // doubles per vector
    static size_t stride(int64_t nv) { return ((size_t)nv + 16 + 31) / 32 * 32; }   // 256-byte aligned, like an allocation of its own
    void ensure(int64_t nv)
    {
        if (v.p && stride(nv) <= cap) return;
        cap = stride(nv);
        v.alloc_raw(6 * cap);
        st.alloc_raw(1);
    }
};

// dev_lanczos without the host in the loop: all kk steps enqueued blind, the scalars in the state block (the rule:
// spk_lanczos_core.hpp), the kernels behind the break returning at their entry (the product still runs, on a stale t into
// aw, which nothing reads); one read of the block per call.  The sums are dev_lanczos's to the bit, so is the tridiagonal.
void dev_lanczos_resident(spk_ctx *c, LzWork &wk, const CsrDev *A, int32_t n, int64_t nv, const double *dinv, double *lmin,
                          double *lmax, double a_scale = 1.0, int32_t *reads = nullptr, LzTri *tri = nullptr)
{
    hipStream_t s = c->stream;
    wk.ensure(nv);
    const size_t ld = LzWork::stride(nv);
    double *sv = wk.v.p, *q = sv + ld, *qp = q + ld, *w = qp + ld, *t = w + ld, *aw = t + ld;
    lanczos_core::LzState *st = wk.st.p;
    SPK_HIP(hipMemsetAsync(wk.v.p, 0, sizeof(double) * 6 * ld, s));
    SPK_HIP(hipMemsetAsync(st, 0, sizeof *st, s));
    const k::Finish f = c->fin(nullptr);
    k::amgs_lz_init_resident(n, dinv, 1.0 / a_scale, sv, q, f, st, s);
    k::amgs_lz_scale_resident(n, -1, q, sv, q, t, st, s);
    const int kk = (int)std::min<int64_t>(kLanczosSteps, n);
    double *qc = q, *qo = qp;
    for (int j = 0; j < kk; ++j) {
        if (A) k::amg_spmv(*A, t, aw, nullptr, s);
        else a_mult(c, t, aw, nullptr, nullptr, nullptr, false, nullptr);
        k::amgs_lz_dot_resident(n, j, sv, aw, a_scale, w, qc, f, st, s);
        k::amgs_lz_update_resident(n, j, kk, qc, qo, w, f, st, s);
        if (j + 1 == kk) break;
        std::swap(qc, qo);
        k::amgs_lz_scale_resident(n, j + 1, w, sv, qc, t, st, s);
    }
    lanczos_core::LzState h;
    SPK_HIP(hipMemcpyAsync(&h, st, sizeof h, hipMemcpyDeviceToHost, s));
    SPK_HIP(hipStreamSynchronize(s));
    if (reads) ++*reads;
    c->check_device_error();
    if (h.steps < 1 || h.steps > kk) fail(SPK_ERR_HIP, "amg: the resident Lanczos reports %d steps of %d", (int)h.steps, kk);
    const std::vector<double> al(h.al, h.al + h.steps), be(h.be, h.be + h.steps);
    if (tri) tri->al = al, tri->be = be;
    ritz_extremes(al, be, lmin, lmax);
}

// sum |x| in the fixed order of the sentinel finish (abs_sum of the host: exactly homogeneous under a power of two)
double dev_abs_sum(spk_ctx *c, const double *x, int32_t n, DevBuf<double> &res)
{
    hipStream_t s = c->stream;
    k::amgs_abs_sum(n, x, c->fin(res.p), s);
    double h = 0.0;
    SPK_HIP(hipMemcpyAsync(&h, res.p, sizeof h, hipMemcpyDeviceToHost, s));
    SPK_HIP(hipStreamSynchronize(s));
    c->check_device_error();
    return h;
}

// the context's CSR as it is when every row ascends, else a sorted copy in `copy`
const CsrDev &sorted_rows(spk_ctx *c, CsrDev &copy)
{
    hipStream_t s = c->stream;
    DevBuf<int32_t> flag;
    flag.alloc(1);
    k::amgs_rows_sorted(c->Ad.rowptr.p, c->Ad.colidx.p, c->n_local, flag.p, s);
    int32_t unsorted = 0;
    SPK_HIP(hipMemcpyAsync(&unsorted, flag.p, sizeof unsorted, hipMemcpyDeviceToHost, s));
    SPK_HIP(hipStreamSynchronize(s));
    if (!unsorted) return c->Ad;
    dev_csr_copy(copy, c->Ad, s);
    k::amgs_sort_rows(copy.rowptr.p, copy.colidx.p, copy.val.p, c->n_local, s);
    return copy;
}

// the device route: every matrix a CsrDev of d.lv.  Level 0 is special, throughout and only here: its operator is A0 (the
// context's CSR or the sorted copy), its D^-1 is dinv0 (pc_setup computes the context's afterwards), its Lanczos product
// the context's layout over vectors of the padded length; with one level it is the coarsest too.
struct DevRoute {
    spk_ctx *c;
    AmgDev &d;
    const spk_amg_opts &o;
    const CsrDev &A0;
    const double *dinv0;
    hipStream_t s;
    bool keep = false;        // reuse on: coarsen keeps A_l P_l and R_l A_l P_l for regalerkin
    int32_t *err = nullptr;   // regalerkin's error word
    double a_scale = 1.0;     // the refresh's (see lanczos)
    mutable LzWork work;             // SPK_AMG_LANCZOS_RESIDENT: the vectors and the state block of every level's Lanczos
    mutable int32_t readbacks = 0;   // device -> host reads of the Ritz estimates (spk_amg_info.ritz_readbacks)
    // the route's part of the info, behind build_levels / refresh_levels
    void ritz_info(spk_amg_info &info) const { info.lanczos = o.lanczos, info.ritz_readbacks = readbacks; }
    const CsrDev &A(int l) const { return l == 0 ? A0 : d.lv[(size_t)l].A; }
    const double *dinv(int l) const { return l == 0 ? dinv0 : d.lv[(size_t)l].dinv.p; }
    int32_t rows(int l) const { return A(l).nrows; }
    int64_t nnz(int l) const { return A(l).nnz; }

    // norms of the diagonal blocks, count, scan, fill; then to the host
    void graph(int l, int bs, double theta, std::vector<int32_t> &gp, std::vector<int32_t> &gi) const
    {
        const CsrDev &M = A(l);
        const int32_t nn = M.nrows / bs;
        DevBuf<double> dn;
        DevBuf<int32_t> cnt, gpd, gid;
        dn.alloc_raw((size_t)nn, 8);
        cnt.alloc_raw((size_t)nn, 8);
        gpd.alloc_raw((size_t)nn + 1, 8);
        k::amgs_node_norms(M.rowptr.p, M.colidx.p, M.val.p, nn, bs, dn.p, s);
        k::amgs_graph(M.rowptr.p, M.colidx.p, M.val.p, nn, bs, theta, dn.p, nullptr, cnt.p, s);
        const int32_t ne = scan_counts(cnt.p, nn, gpd.p, s);
        gid.alloc_raw((size_t)ne, 8);
        k::amgs_graph(M.rowptr.p, M.colidx.p, M.val.p, nn, bs, theta, dn.p, gpd.p, gid.p, s);
        gp.resize((size_t)nn + 1);
        gi.resize((size_t)ne);
        SPK_HIP(hipMemcpyAsync(gp.data(), gpd.p, sizeof(int32_t) * gp.size(), hipMemcpyDeviceToHost, s));
        if (ne) SPK_HIP(hipMemcpyAsync(gi.data(), gid.p, sizeof(int32_t) * gi.size(), hipMemcpyDeviceToHost, s));
        SPK_HIP(hipStreamSynchronize(s));
    }
    // Under SPK_AMG_GALERKIN_STENCIL a level >= 1 holds the host route's bytes, so where it is small enough to cross the bus
    // as the coarsest operator does (at most SPK_AMG_MAX_COARSE rows) the host's own Lanczos runs on a download of it: the
    // host's Ritz values to the bit, and one download where the device steps read two sums back 30 times.  It is on such
    // levels that the bits matter: 30 steps without reorthogonalisation on a few dozen rows lose orthogonality altogether
    // before the largest Ritz value has converged, and its value then follows the rounding of every sum
    bool ritz_on_host(int l) const
    {
        return o.coarsening == SPK_AMG_COARSEN_GRID && o.galerkin == SPK_AMG_GALERKIN_STENCIL && l > 0 && rows(l) <= SPK_AMG_MAX_COARSE;
    }
    void ritz(int l, double *lmin, double *lmax) const
    {
        if (ritz_on_host(l)) {
            const HostCsr H = dev_csr_download(A(l), true, s);
            ++readbacks;
            return lanczos(H, diag_inv(H), lmin, lmax, a_scale);
        }
        const CsrDev *M = l ? &A(l) : nullptr;
        const int64_t nv = l ? rows(l) : c->ld;
        if (o.lanczos == SPK_AMG_LANCZOS_RESIDENT) dev_lanczos_resident(c, work, M, rows(l), nv, dinv(l), lmin, lmax, a_scale, &readbacks);
        else dev_lanczos(c, M, rows(l), nv, dinv(l), lmin, lmax, a_scale, &readbacks);
    }
    void set_interval(int l, double lo, double hi) { smoother_coeffs(o, lo, hi, d.lv[(size_t)l].alpha, d.lv[(size_t)l].beta); }
    void coarsen(int l, int bs, std::vector<int32_t> agg, int32_t na, double omega, int nsmooths)
    {
        AmgLevelDev &L = d.lv[(size_t)l];
        const int32_t n = rows(l);
        {   // tentative prolongator: 1/sqrt(|aggregate|) comes from the host, like the aggregates
            std::vector<int32_t> size((size_t)na, 0);
            for (int32_t a : agg) if (a >= 0) ++size[(size_t)a];
            std::vector<double> inv((size_t)na);
            for (int32_t a = 0; a < na; ++a) inv[(size_t)a] = 1.0 / std::sqrt((double)size[(size_t)a]);
            DevBuf<int32_t> aggd, cnt;
            DevBuf<double> invd;
            aggd.upload(agg.data(), agg.size(), 8);
            invd.upload(inv.data(), inv.size(), 8);
            cnt.alloc_raw((size_t)n, 8);
            CsrDev &T = L.Ptent;
            T.nrows = n;
            T.ncols = na * bs;
            k::amgs_tent_count(aggd.p, n, bs, cnt.p, s);
            T.rowptr.alloc_raw((size_t)n + 1, 8);
            dev_csr_values(T, scan_counts(cnt.p, n, T.rowptr.p, s));
            k::amgs_tent_fill(aggd.p, invd.p, n, bs, T.rowptr.p, T.colidx.p, T.val.p, s);
            SPK_HIP(hipStreamSynchronize(s));
        }
        L.agg = std::move(agg);
        dev_csr_copy(L.P, L.Ptent, s);
        for (int it = 0; it < nsmooths; ++it) {   // P = (I - omega D^-1 A) P
            CsrDev AP, Pn;
            dev_spgemm(AP, A(l), L.P, s);
            dev_add(Pn, 1.0, L.P, -omega, AP, dinv(l), s);
            L.P = std::move(Pn);
        }
        galerkin(l);
    }
    // P from the node grids alone: every row length is known, so one kernel writes row pointers, columns and weights
    void coarsen_grid(int l, int bs, const int32_t fd[3], const int32_t cd[3])
    {
        AmgLevelDev &L = d.lv[(size_t)l];
        const int64_t nz = grid_prolong_nnz(fd, cd, bs);
        if (nz > INT32_MAX)
            fail(SPK_ERR_UNSUPPORTED, "amg: the prolongator of level %d has more entries than 32-bit offsets address", l);
        L.grid.set(fd, cd, bs, o.transfer);
        L.P.nrows = rows(l);
        L.P.ncols = cd[0] * cd[1] * cd[2] * bs;
        L.P.rowptr.alloc_raw((size_t)L.P.nrows + 1, 8);
        dev_csr_values(L.P, nz);
        k::amgs_grid_prolongator(L.grid, L.P.rowptr.p, L.P.colidx.p, L.P.val.p, s);
        if (o.galerkin != SPK_AMG_GALERKIN_STENCIL) return galerkin(l);
        const int64_t nc = galerkin::gs_nnz(cd, bs);
        if (nc > INT32_MAX)
            fail(SPK_ERR_UNSUPPORTED, "amg: the operator of level %d has more entries than 32-bit offsets address", l + 1);
        dev_transpose(L.R, L.P, s);
        d.lv.emplace_back();   // (reserved)
        AmgLevelDev &N = d.lv.back();
        N.n = N.A.nrows = N.A.ncols = L.P.ncols;
        N.A.rowptr.alloc_raw((size_t)N.n + 1, 8);
        dev_csr_values(N.A, nc);
        N.dinv.alloc((size_t)N.n, 8);
        DevBuf<unsigned long long> bad;   // (row << 32 | column) of the first entry outside the stencil, else all ones
        if (l == 0) {   // level 0 alone has a foreign pattern: its one check, read back behind the level's launches
            bad.alloc_raw(1);
            SPK_HIP(hipMemsetAsync(bad.p, 0xff, sizeof(unsigned long long), s));
            k::amgs_galerkin_stencil_check(L.grid, A(0), bad.p, s);
        }
        stencil(l);
        if (l == 0) {
            unsigned long long key = 0;
            SPK_HIP(hipMemcpyAsync(&key, bad.p, sizeof key, hipMemcpyDeviceToHost, s));
            SPK_HIP(hipStreamSynchronize(s));
            if (key != ~0ull)
                fail(SPK_ERR_UNSUPPORTED, "amg: the entry in row %d, column %d of the operator couples nodes that are not neighbours "
                     "on the %d x %d x %d grid; the stencil products take couplings between neighbouring nodes only -- use "
                     "-spk_mg_galerkin products", (int)(key >> 32), (int)(key & 0xffffffffull), (int)fd[0], (int)fd[1], (int)fd[2]);
        }
    }
    // level l+1 by the grid-stencil gather, the build's and the refresh's: three launches into buffers whose sizes follow
    // from the node grids -- no count, no scan, no scratch, no read-back
    void stencil(int l)
    {
        AmgLevelDev &L = d.lv[(size_t)l], &N = d.lv[(size_t)l + 1];
        k::amgs_galerkin_stencil(L.grid, A(l), N.A, s);
        k::extract_diag_inv(N.A, N.dinv.p, s);
    }
    // R = P^T and level l+1 from the P of level l
    void galerkin(int l)
    {
        AmgLevelDev &L = d.lv[(size_t)l];
        dev_transpose(L.R, L.P, s);
        CsrDev AP, Ac, AcT;
        dev_spgemm(AP, A(l), L.P, s);
        dev_spgemm(Ac, L.R, AP, s);
        dev_transpose(AcT, Ac, s);
        d.lv.emplace_back();   // (reserved)
        AmgLevelDev &N = d.lv.back();
        dev_add(N.A, 0.5, Ac, 0.5, AcT, nullptr, s);   // exactly symmetric (the products agree to rounding)
        N.n = N.A.nrows;
        N.dinv.alloc((size_t)N.n, 8);
        k::extract_diag_inv(N.A, N.dinv.p, s);
        if (keep) {
            AmgLevelDev &K = d.lv[(size_t)l];
            K.AP = std::move(AP);
            K.Ac = std::move(Ac);
        }
    }
    int levels() const { return (int)d.lv.size(); }
    // three launches into buffers the build left: nothing is allocated, counted or scanned
    void regalerkin(int l)
    {
        if (o.galerkin == SPK_AMG_GALERKIN_STENCIL) return stencil(l);
        AmgLevelDev &L = d.lv[(size_t)l], &N = d.lv[(size_t)l + 1];
        k::amgs_spgemm_numeric(A(l), L.P, L.AP, err, s);
        k::amgs_spgemm_numeric(L.R, L.AP, L.Ac, err, s);
        k::amgs_symmetrise_numeric(L.Ac, N.A, err, s);
        k::extract_diag_inv(N.A, N.dinv.p, s);
    }
    void check() const
    {
        int32_t bad = 0;
        SPK_HIP(hipMemcpyAsync(&bad, err, sizeof bad, hipMemcpyDeviceToHost, s));
        SPK_HIP(hipStreamSynchronize(s));
        if (bad) fail(SPK_ERR_STATE, "amg: a product of the refresh has no slot in the kept pattern");
    }
    HostCsr coarsest() const { return dev_csr_download(A((int)d.lv.size() - 1), true, s); }
    void set_coarse_inverse(const std::vector<double> &cinv) { d.cinv.upload(cinv.data(), cinv.size()); }
};

}  // namespace

std::unique_ptr<AmgDev> amg_build_device(spk_ctx *c)
{
    const auto t0 = Clock::now();
    const spk_amg_opts &o = c->amg_opts;
    amg_check_opts(o);
    c->ensure_scratch();
    if (c->n_local <= 0) fail(SPK_ERR_ARG, "amg: the operator must be square and non-empty");
    auto d = std::make_unique<AmgDev>();
    if (c->amg_reuse) d->reuse = std::make_unique<AmgReuse>();   // level 0's sorted copy and D^-1 outlive the build
    CsrDev copy_here;
    DevBuf<double> dinv0_here;
    CsrDev &copy = d->reuse ? d->reuse->sorted : copy_here;
    DevBuf<double> &dinv0 = d->reuse ? d->reuse->dinv0 : dinv0_here;
    const CsrDev &A0 = sorted_rows(c, copy);
    if (d->reuse) d->reuse->use_sorted = &A0 == &copy;
    const int cbs = ctx_block_size(c, o), bs = cbs > 0 ? cbs : detect_bs(dev_csr_download(A0, false, c->stream));
    d->lv.reserve((size_t)o.max_levels);   // the levels own device buffers and never move
    d->lv.emplace_back();
    d->lv[0].n = c->n_local;
    dinv0.alloc((size_t)c->n_local, 8);
    k::extract_diag_inv(c->Ad, dinv0.p, c->stream);
    if (d->reuse) {
        d->reuse->sum.alloc(8);
        d->reuse->dinv_sum = dev_abs_sum(c, dinv0.p, c->n_local, d->reuse->sum);
    }
    DevRoute r{c, *d, o, A0, dinv0.p, c->stream, d->reuse != nullptr, nullptr, 1.0, {}, 0};
    build_levels(r, bs, o, SPK_AMG_SETUP_DEVICE, t0, d->info);
    r.ritz_info(d->info);
    alloc_cycle_vectors(*d, c->ld, o.precision == SPK_AMG_PRECISION_SINGLE);
    amg_plan_cycle(*d, o, c->ld, c->stream);
    if (d->reuse) keep_pattern(c, *d);
    SPK_HIP(hipDeviceSynchronize());
    d->info.setup_seconds = seconds_since(t0);   // the vectors count too, up to the synchronise
    return d;
}

bool amg_can_refresh(spk_ctx *c)
{
    if (!c->amg_reuse || !c->amg_on || !c->amg_d || !c->amg_d->reuse) return false;
    AmgReuse &ru = *c->amg_d->reuse;
    const spk_amg_opts &a = c->amg_opts;
    if (!amg_same_hierarchy_opts(a, ru.o) || ctx_block_size(c, a) != ru.bs || c->n_local != ru.n || c->Ad.nnz != ru.nnz || c->ld != ru.ld)
        return false;
    if ((a.setup == SPK_AMG_SETUP_HOST) != (c->amg_h != nullptr)) return false;
    hipStream_t s = c->stream;
    SPK_HIP(hipMemsetAsync(ru.flag.p, 0, 2 * sizeof(int32_t), s));
    k::amgs_pattern_equal(ru.rowptr.p, c->Ad.rowptr.p, (int64_t)ru.n + 1, ru.flag.p, s);
    k::amgs_pattern_equal(ru.colidx.p, c->Ad.colidx.p, ru.nnz, ru.flag.p, s);
    int32_t differ = 1;
    SPK_HIP(hipMemcpyAsync(&differ, ru.flag.p, sizeof differ, hipMemcpyDeviceToHost, s));
    SPK_HIP(hipStreamSynchronize(s));
    return differ == 0;
}

void amg_refresh_ctx(spk_ctx *c)
{
    const auto t0 = Clock::now();
    hipStream_t s = c->stream;
    AmgDev &d = *c->amg_d;
    AmgReuse &ru = *d.reuse;
    const size_t L = d.lv.size();
    // the options of the application are not the hierarchy's (amg_can_refresh does not compare them): the refresh takes
    // the ones this set-up was given
    amg_take_application_opts(ru.o, c->amg_opts);
    if (c->amg_h) {   // the host route: the values down, the host refresh, the values of the levels up
        AmgHier &h = c->amg_h->h;
        amg_take_application_opts(h.o, ru.o);
        std::vector<double> val((size_t)c->Ad.nnz);
        if (!val.empty()) SPK_HIP(hipMemcpyAsync(val.data(), c->Ad.val.p, sizeof(double) * val.size(), hipMemcpyDeviceToHost, s));
        SPK_HIP(hipStreamSynchronize(s));
        amg_refresh(h, val.data());
        for (size_t l = 0; l < L; ++l) {
            const AmgLevel &H = h.lv[l];
            AmgLevelDev &D = d.lv[l];
            if (l > 0) {
                if (H.A.nnz()) SPK_HIP(hipMemcpyAsync(D.A.val.p, H.A.v.data(), sizeof(double) * H.A.v.size(), hipMemcpyHostToDevice, s));
                SPK_HIP(hipMemcpyAsync(D.dinv.p, H.dinv.data(), sizeof(double) * H.dinv.size(), hipMemcpyHostToDevice, s));
            }
            if (l + 1 < L) smoother_coeffs(h.o, H.lo, H.hi, D.alpha, D.beta);
        }
        SPK_HIP(hipMemcpyAsync(d.cinv.p, h.cinv.data(), sizeof(double) * h.cinv.size(), hipMemcpyHostToDevice, s));
        SPK_HIP(hipDeviceSynchronize());   // (the host vectors are pageable: the copies have left them by now anyway)
        d.info = h.info;
    } else {
        c->ensure_scratch();
        if (ru.use_sorted) {   // the build's sorted copy of level 0 again, in its buffers
            if (ru.nnz) {
                SPK_HIP(hipMemcpyAsync(ru.sorted.colidx.p, c->Ad.colidx.p, sizeof(int32_t) * (size_t)ru.nnz, hipMemcpyDeviceToDevice, s));
                SPK_HIP(hipMemcpyAsync(ru.sorted.val.p, c->Ad.val.p, sizeof(double) * (size_t)ru.nnz, hipMemcpyDeviceToDevice, s));
            }
            k::amgs_sort_rows(ru.sorted.rowptr.p, ru.sorted.colidx.p, ru.sorted.val.p, ru.n, s);
        }
        k::extract_diag_inv(c->Ad, ru.dinv0.p, s);
        const double a_scale = binade_scale(ru.dinv_sum, dev_abs_sum(c, ru.dinv0.p, ru.n, ru.sum));
        DevRoute r{c, d, ru.o, ru.use_sorted ? ru.sorted : c->Ad, ru.dinv0.p, s, true, ru.flag.p + 1, a_scale, {}, 0};
        refresh_levels(r, ru.o, t0, d.info);
        r.ritz_info(d.info);
        SPK_HIP(hipDeviceSynchronize());
    }
    amg_plan_cycle(d, ru.o, c->ld, s);   // the coefficients are new, and the device route's coarse inverse lies elsewhere
    d.info.setup_seconds = seconds_since(t0);
}

void amg_drop_reuse(spk_ctx *c)
{
    if (!c->amg_d || !c->amg_d->reuse) return;
    c->amg_d->reuse.reset();
    for (AmgLevelDev &D : c->amg_d->lv) {
        D.AP = CsrDev{};
        D.Ac = CsrDev{};
    }
}

// the test hooks: the host hierarchy where pc_setup kept one, else one download from the device-built levels
void amg_ctx_level(spk_ctx *c, int l, int which, const CsrOut &out)
{
    if (c->amg_h) return c->amg_h->h.level(l, which, out);
    const AmgDev &d = *c->amg_d;
    check_level_query((int)d.lv.size(), l, which);
    const AmgLevelDev &V = d.lv[(size_t)l];
    if (which == SPK_AMG_COARSE_INV) {
        std::vector<double> cinv(out.val ? (size_t)V.n * V.n : 0);
        if (out.val) SPK_HIP(hipMemcpy(cinv.data(), d.cinv.p, sizeof(double) * cinv.size(), hipMemcpyDeviceToHost));
        return coarse_inv_out(V.n, cinv.data(), out);
    }
    const bool grid = d.info.coarsening == SPK_AMG_COARSEN_GRID;   // no tentative prolongator: SPK_AMG_TENTATIVE is P
    const CsrDev &M = which == SPK_AMG_OP ? (l == 0 ? c->Ad : V.A) : which == SPK_AMG_PROLONG || grid ? V.P : V.Ptent;
    if (!out.rowptr && !out.colidx && !out.val) return out.sizes(M.nrows, M.ncols, M.nnz);   // nothing to download
    HostCsr H = dev_csr_download(M, true, c->stream);
    if (which == SPK_AMG_OP && l == 0) sort_rows(H);   // the context's CSR keeps the caller's order
    csr_out(H, out);
}

void amg_ctx_aggregates(spk_ctx *c, int l, int32_t *nnodes, int32_t *agg)
{
    if (c->amg_h) aggregates_out(c->amg_h->h.lv, c->amg_d->info, l, nnodes, agg);
    else aggregates_out(c->amg_d->lv, c->amg_d->info, l, nnodes, agg);
}

// the test hook of the set-up's Lanczos: either route on one level of the device-built hierarchy as it stands (level 0:
// the context's layout and the D^-1 of its CSR copy, as at the build; no binade scale)
void amg_debug_lanczos(spk_ctx *c, int l, int resident, int32_t *steps, double *al, double *be)
{
    if (c->amg_h) fail(SPK_ERR_STATE, "amg: Lanczos hook: the hierarchy was built on the host -- pass -spk_gamg_setup device");
    AmgDev &d = *c->amg_d;
    if (l < 0 || l + 1 >= (int)d.lv.size()) fail(SPK_ERR_ARG, "amg: Lanczos hook: level %d has no Ritz estimate (levels: %d)", l, (int)d.lv.size());
    if (resident != 0 && resident != 1) fail(SPK_ERR_ARG, "amg: Lanczos hook: resident is 0 or 1");
    c->ensure_scratch();
    AmgLevelDev &D = d.lv[(size_t)l];
    DevBuf<double> dinv0;
    if (l == 0) {
        dinv0.alloc((size_t)c->n_local, 8);
        k::extract_diag_inv(c->Ad, dinv0.p, c->stream);
    }
    const CsrDev *M = l ? &D.A : nullptr;
    const int32_t n = l ? D.A.nrows : c->n_local;
    const int64_t nv = l ? n : c->ld;
    const double *dinv = l ? D.dinv.p : dinv0.p;
    double lmin = 0.0, lmax = 0.0;
    LzTri tri;
    LzWork work;
    if (resident) dev_lanczos_resident(c, work, M, n, nv, dinv, &lmin, &lmax, 1.0, nullptr, &tri);
    else dev_lanczos(c, M, n, nv, dinv, &lmin, &lmax, 1.0, nullptr, &tri);
    *steps = (int32_t)tri.al.size();
    std::copy(tri.al.begin(), tri.al.end(), al);
    std::copy(tri.be.begin(), tri.be.end(), be);
}

}  // namespace spk
