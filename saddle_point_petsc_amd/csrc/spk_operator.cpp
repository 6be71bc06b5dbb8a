// spk_operator.cpp -- KSPSetOperators and KSPSetUp: the device half of the set-up, as named steps.
//
// What runs at /root/reference/src/SaddlePointProblem.c:66 (KSPSetOperators on the nest of :45-60) and inside KSPSetUp:
// upload of a row slab, its split into diagonal and off-rank part, the blocked copies and the dictionary of the A
// block, the halo plan, the column windows and the transpose of the constraint block, diag(A)^-1 and
// S^ = diag(B diag(A)^-1 B^T).  The integer arithmetic between the device rounds is in spk_host.cpp (no HIP there,
// tested on the CPU); this file allocates, launches, reads back and keeps the order of the collectives.
#include <cstdlib>
#include <cstring>

#include "spk_internal.hpp"
#include "spk_constraints_core.hpp"
#include "../../include/spk_assembly.h"

namespace spk {

// host array -> fresh device buffer through the pinned staging pipeline (large arrays), pad zeroed
template <class T>
static void up(spk_ctx *c, DevBuf<T> &d, const T *h, size_t count, size_t pad)
{
    d.alloc_raw(count, pad);
    c->upload_staged(d.p, h, count * sizeof(T));
}

template <class VR, class VI, class VD>
static void upload_csr(spk_ctx *c, CsrDev &D, int32_t nrows, int32_t ncols, const VR &rowptr, const VI &colidx, const VD &val,
                       bool tiles)
{
    D.nrows = nrows;
    D.ncols = ncols;
    D.nnz = (int64_t)colidx.size();
    up(c, D.rowptr, rowptr.data(), rowptr.size(), 8);
    up(c, D.colidx, colidx.data(), colidx.size(), 16);
    up(c, D.val, val.data(), val.size(), 16);
    if (tiles) {
        std::vector<int32_t> tr;
        k::build_tiles(rowptr.data(), nrows, tr);
        D.ntiles = (int32_t)tr.size() - 1;
        D.tile_row.upload(tr.data(), tr.size(), 8);
    }
}

// the LOCAL part of a collective set-up step, run to its end or to its first error (code 0: none)
template <class F>
static Error locally(F &&fn)
{
    try {
        fn();
    } catch (const Error &e) {
        return e;
    } catch (const std::exception &e) {
        return Error{SPK_ERR_NOMEM, e.what()};
    }
    return Error{0, ""};
}

// Collective agreement on a set-up step (KSPSetOperators is collective, as in PETSc): every rank
// reports whether its LOCAL part succeeded; when any rank failed, ALL ranks throw -- the failing one its
// own message, the others a note naming it -- so nobody is left waiting inside the next collective.
static void agree_or_fail(spk_ctx *c, const Error &mine, const char *step)
{
    const int P = c->comm->size();
    if (P > 1) {
        std::vector<int32_t> all((size_t)P, 0);
        const int32_t ok = mine.code ? 0 : 1;
        c->comm->host_allgather(&ok, all.data(), sizeof ok);
        if (!mine.code)
            for (int r = 0; r < P; ++r)
                if (!all[(size_t)r])
                    fail(SPK_ERR_COMM, "%s: rank %d failed its local part; the collective set-up is abandoned on every rank", step, r);
    }
    if (mine.code) throw mine;
}

// bitwise AND of every rank's `bits`: what the solve does must not depend on one rank's slab (KSPSetUp is collective)
static int32_t and_over_ranks(spk_ctx *c, int32_t bits)
{
    const int P = c->comm->size();
    std::vector<int32_t> all((size_t)P, bits);
    if (P > 1) c->comm->host_allgather(&bits, all.data(), sizeof bits);
    for (int32_t v : all) bits &= v;
    return bits;
}

// ---------------------------------------------------------------------------
// Row types + deviation codes over the blocked copy just built (DictDev, spk_internal.hpp)
// ---------------------------------------------------------------------------
// the blocked copy the dictionary is found in
struct DictSrc {
    int bs;
    int32_t nbr;
    int64_t nb, ldp;
    const int32_t *browptr, *bcol;
    const double *v0, *v1;
};

// Scratch of the hashing rounds and every host array a pending copy of build_dict reads or writes.
struct DictWork {
    hipStream_t s;
    DevBuf<unsigned long long> keys;
    DevBuf<int32_t> rep, ctl, slot2id_d, rep_d, bad, slot;
    std::vector<unsigned long long> hk;
    std::vector<int32_t> hr, s2i, reps, hfld;
    std::vector<int> hwid;
    std::vector<double> hcls;
    int32_t hctl[4] = {0, 0, 0, 0};
    DictWork(hipStream_t s_, int64_t nb) : s(s_), hk(k::kDictSlots), hr(k::kDictSlots), s2i(k::kDictSlots)
    {
        keys.alloc_raw(k::kDictSlots);
        rep.alloc_raw(k::kDictSlots);
        ctl.alloc_raw(4);
        bad.alloc(4);
        slot2id_d.alloc_raw(k::kDictSlots);
        rep_d.alloc_raw(std::max(k::kDictMaxPat, k::kDictMaxBlk));
        slot.alloc_raw((size_t)nb, 8);
    }
    void reset()
    {
        SPK_HIP(hipMemsetAsync(keys.p, 0, sizeof(unsigned long long) * k::kDictSlots, s));
        SPK_HIP(hipMemsetAsync(rep.p, 0x7f, sizeof(int32_t) * k::kDictSlots, s));
        SPK_HIP(hipMemsetAsync(ctl.p, 0, sizeof(int32_t) * 4, s));
    }
    // after a hashing launch: read the table back, number the classes by their first member; the class count or -1
    int classes()
    {
        SPK_HIP(hipMemcpyAsync(hctl, ctl.p, sizeof hctl, hipMemcpyDeviceToHost, s));
        SPK_HIP(hipMemcpyAsync(hk.data(), keys.p, sizeof(unsigned long long) * k::kDictSlots, hipMemcpyDeviceToHost, s));
        SPK_HIP(hipMemcpyAsync(hr.data(), rep.p, sizeof(int32_t) * k::kDictSlots, hipMemcpyDeviceToHost, s));
        SPK_HIP(hipStreamSynchronize(s));
        if (hctl[1]) return -1;
        dict_number_classes(hk.data(), hr.data(), k::kDictSlots, s2i.data(), reps);
        SPK_HIP(hipMemcpyAsync(slot2id_d.p, s2i.data(), sizeof(int32_t) * k::kDictSlots, hipMemcpyHostToDevice, s));
        SPK_HIP(hipMemcpyAsync(rep_d.p, reps.data(), sizeof(int32_t) * reps.size(), hipMemcpyHostToDevice, s));
        SPK_HIP(hipStreamSynchronize(s));
        return (int)reps.size();
    }
    bool flagged()   // the verification word of the last launch
    {
        int32_t hbad = 1;
        SPK_HIP(hipMemcpyAsync(&hbad, bad.p, sizeof hbad, hipMemcpyDeviceToHost, s));
        SPK_HIP(hipStreamSynchronize(s));
        return hbad != 0;
    }
};

// Round 2: granule and range of every class entry (slot[q] := class of block q), then widths and the field layout.
static DictRefusal dict_class_fields(DictDev &D, const DictSrc &A, DictWork &W, int ncls)
{
    hipStream_t s = W.s;
    const int bb = A.bs * A.bs;
    const size_t ne = (size_t)ncls * bb;
    DevBuf<unsigned long long> dmax;
    DevBuf<int32_t> gexp;
    D.cls.alloc_raw((size_t)(ncls + 1) * bb * 2, 8);
    gexp.alloc_raw(ne, 8);
    dmax.alloc(ne, 8);
    SPK_HIP(hipMemsetAsync(gexp.p, 0x7f, sizeof(int32_t) * ne, s));
    k::dict_class_stats(A.bs, A.v0, A.v1, A.ldp, A.nb, W.rep_d.p, ncls, W.slot2id_d.p, W.slot.p, D.cls.p, gexp.p, dmax.p, W.bad.p, s);
    std::vector<int32_t> hg(ne);
    std::vector<unsigned long long> hm(ne);
    W.hcls.assign((size_t)(ncls + 1) * bb * 2, 0.0);   // (the null class behind the found ones: zeros)
    SPK_HIP(hipMemcpyAsync(hg.data(), gexp.p, sizeof(int32_t) * ne, hipMemcpyDeviceToHost, s));
    SPK_HIP(hipMemcpyAsync(hm.data(), dmax.p, sizeof(unsigned long long) * ne, hipMemcpyDeviceToHost, s));
    SPK_HIP(hipMemcpyAsync(W.hcls.data(), D.cls.p, sizeof(double) * ne * 2, hipMemcpyDeviceToHost, s));
    if (W.flagged()) return {"a deviation from its class base is not exactly representable"};
    W.hwid.resize(ne);
    W.hfld.resize((size_t)(ncls + 1) * bb);
    std::vector<double> hscale(ne);
    if (DictRefusal r = dict_field_widths((int)ne, hg.data(), hm.data(), W.hwid.data(), hscale.data()); r.why) return r;
    DictLayout L;
    const DictRefusal r = dict_field_layout(A.bs, ncls, W.hwid.data(), hscale.data(), !getenv("SPK_DICT_NOUNIFORM"), W.hfld.data(),
                                            W.hcls.data(), L);
    D.uniform = L.uniform;
    D.uniform3 = L.uniform3;
    D.straddle = L.straddle;
    if (L.uniform) std::copy(L.uw, L.uw + 4, D.uw);
    if (L.uniform3) std::copy(L.u3l, L.u3l + 9, D.u3l), std::copy(L.u3r, L.u3r + 9, D.u3r);
    if (r.why) return r;
    SPK_HIP(hipMemcpyAsync(D.cls.p, W.hcls.data(), sizeof(double) * W.hcls.size(), hipMemcpyHostToDevice, s));
    D.fld.alloc_raw((size_t)(ncls + 1) * bb, 8);
    D.zpad.alloc(8, 8);
    SPK_HIP(hipMemcpyAsync(D.fld.p, W.hfld.data(), sizeof(int32_t) * W.hfld.size(), hipMemcpyHostToDevice, s));
    return {};
}

// Rounds 3 and 4: row types by hashing the (column offset, class) sequences, then the type table and every row's type.
static DictRefusal dict_row_types(DictDev &D, const DictSrc &A, DictWork &W, const int32_t *brp, int ncls)
{
    hipStream_t s = W.s;
    DevBuf<int32_t> rslot;
    rslot.alloc_raw((size_t)A.nbr, 8);
    W.reset();
    k::dict_hash_rows(A.browptr, A.bcol, W.slot.p, A.nbr, W.keys.p, W.rep.p, rslot.p, W.ctl.p, k::kDictMaxPat, kDictMaxK, s);
    const int ntype = W.classes();
    if (ntype <= 0) return {"row types beyond the table, or a row beyond kDictMaxK blocks", W.hctl[0], W.hctl[1]};
    int kmax = 1;
    for (int32_t r : W.reps) kmax = std::max(kmax, brp[(size_t)r + 1] - brp[(size_t)r]);
    const int lds_bytes = dict_lds_bytes(ntype, kmax, ncls, A.bs);
    if (lds_bytes > k::kDictLdsMax) return {"tables beyond the LDS budget", lds_bytes, ntype};
    D.tab.alloc((size_t)dict_tab_ints(ntype, kmax), 8);
    D.tid.alloc_raw((size_t)A.nbr, 64);
    k::dict_fill_rows(A.browptr, A.bcol, W.slot.p, A.nbr, W.rep_d.p, ntype, kmax, W.slot2id_d.p, rslot.p, D.tab.p, D.tid.p, W.bad.p, s);
    if (W.flagged()) return {"row type verification failed (hash collision)", ntype, ncls};
    D.ntype = ntype;
    D.kmax = kmax;
    D.lds_bytes = lds_bytes;
    return {};
}

static void dict_report(const DictDev &D, const DictWork &W)
{
    const int bb = D.bs * D.bs, ncls = D.nclass;
    int wmax = 0;
    for (int cl = 0; cl < ncls; ++cl) {
        int tot = 0;
        for (int e = 0; e < bb; ++e) tot += (W.hfld[(size_t)cl * bb + e] >> 8) & 255;
        wmax = std::max(wmax, tot);
    }
    fprintf(stderr, "[spk] row types + codes: %d block rows, %d types (<= %d blocks), %d classes of %d x %d (<= %d bits of codes per block), "
                    "%d B of LDS, %.1f B of codes per block row%s\n", D.nbrows, D.ntype, D.kmax, ncls, D.bs, D.bs, wmax, D.lds_bytes,
            (double)D.code_bytes / D.nbrows, D.uniform || D.uniform3 ? ", one field layout for all classes" : "");
    fprintf(stderr, "[spk]   widest need per block entry:");
    for (int e = 0; e < bb; ++e) {
        int w = 1;
        for (int cl = 0; cl < ncls; ++cl) w = std::max(w, W.hwid[(size_t)cl * bb + e]);
        fprintf(stderr, " %d", w);
    }
    fprintf(stderr, "\n");
}

// Block classes, then row types, proposed by hashing on the device; granule and range of every class entry; codes; every
// value decoded and compared bit by bit.  Leaves Adict.ok = false (the blocked kernels stay) for matrices that do not
// fit.  brp: the block row pointers on the host.
static void build_dict(spk_ctx *c, int bs, const int32_t *brp)
{
    DictDev &D = c->Adict;
    D.ok = false;
    auto release = [&] { D.tid.release(); D.tab.release(); D.cls.release(); D.fld.release(); D.codes.release(); D.zpad.release(); };
    release();
    const char *fmt = getenv("SPK_SPMV_FORMAT");
    if (fmt && (!strcmp(fmt, "csr") || !strcmp(fmt, "bcsr"))) return;
    static const bool verbose = getenv("SPK_DICT_VERBOSE") != nullptr;
    auto refuse = [&](const char *why, long a = 0, long b = 0) {
        release();
        if (verbose) fprintf(stderr, "[spk] row types + codes refused: %s (%ld, %ld)\n", why, a, b);
    };
    hipStream_t s = c->stream;
    const DictSrc A = bs == 2 ? DictSrc{2, c->Ab.nbrows, c->Ab.nblocks, 0, c->Ab.browptr.p, c->Ab.bcol.p, c->Ab.vtop.p, c->Ab.vbot.p}
                              : DictSrc{3, c->Ab3.nbrows, c->Ab3.nblocks, c->Ab3.ldp, c->Ab3.browptr.p, c->Ab3.bcol.p, c->Ab3.v.p, nullptr};
    if (A.nbr == 0 || A.nb == 0 || A.nb > INT32_MAX) return refuse("empty or too many blocks", A.nbr, (long)A.nb);
    DictWork W(s, A.nb);
    // ---- round 1, block classes: blocks equal up to ~1e-6 absolute; base = the first member
    W.reset();
    k::dict_hash_blocks(bs, A.v0, A.v1, A.ldp, A.nb, W.keys.p, W.rep.p, W.slot.p, W.ctl.p, k::kDictMaxBlk, s);
    const int ncls = W.classes();
    if (ncls <= 0) return refuse("block classes beyond the table", W.hctl[0], W.hctl[1]);
    if (DictRefusal r = dict_class_fields(D, A, W, ncls); r.why) return refuse(r.why, r.a, r.b);
    if (DictRefusal r = dict_row_types(D, A, W, brp, ncls); r.why) return refuse(r.why, r.a, r.b);
    // ---- round 5: the code planes, every value encoded, decoded again and compared
    static const int64_t skew = [] { const char *e = getenv("SPK_DICT_SKEW"); return e ? (int64_t)atoll(e) : (int64_t)(17 * 256); }();
    D.codes.alloc((size_t)dict_plane_offsets(bs, D.kmax, A.nbr, skew, D.plane_off), 64);
    D.bs = bs;
    D.nbrows = A.nbr;
    D.nblocks = A.nb;
    D.nclass = ncls;
    D.code_bytes = (int64_t)(bs == 2 ? 8 : 16) * A.nb;   // bytes of codes one product reads: every stored block once
    k::dict_encode_verify(D, A.browptr, A.bcol, W.slot.p, A.v0, A.v1, A.ldp, W.bad.p, s);
    if (W.flagged()) return refuse("a decoded value differs from the stored one", D.ntype, ncls);
    D.ok = true;
    if (verbose) dict_report(D, W);
}

// ---------------------------------------------------------------------------
// KSPSetOperators, A00: one row slab of the A block
// ---------------------------------------------------------------------------
// the caller's slab on the device, as it came, with the scan of its off-rank entries per row
struct SlabIn {
    DevBuf<int32_t> rowptr, colidx, orp, flags;
    DevBuf<double> val;
    int32_t noff = 0;
};

// Validation, host part: nothing of the context changes here.
static void a_check_host(int64_t row_begin, int32_t n, int64_t ncols_global, const int32_t *rowptr)
{
    if (rowptr[0] != 0) fail(SPK_ERR_ARG, "A00: rowptr[0] must be 0");
    if (row_begin < 0 || row_begin + n > ncols_global)
        fail(SPK_ERR_ARG, "A00: rows [%lld,%lld) outside the %lld x %lld block", (long long)row_begin,
             (long long)(row_begin + n), (long long)ncols_global, (long long)ncols_global);
    for (int32_t r = 0; r < n; ++r)
        if (rowptr[r + 1] < rowptr[r]) fail(SPK_ERR_ARG, "A00: rowptr not monotone at row %d", r);
}

// One source of the slab: the caller's host arrays through the staging pipeline ...
static void a_bring_upload(spk_ctx *c, int32_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, SlabIn &in)
{
    const int64_t nnz = rowptr[n];
    up(c, in.rowptr, rowptr, (size_t)n + 1, 8);
    up(c, in.colidx, colidx, (size_t)nnz, 16);
    up(c, in.val, val, (size_t)nnz, 16);
}

// The node grid of the device assembly.  mz == 0: the reference's 2-D grid (dof 2, the ranks share out node lines,
// spk_k_assembly.hip), else the 3-D generator's (dof 3, node planes, spk_k_assembly3d.hip).  Everything in which the two
// routes differ is answered here; the chain over it is one.
struct LaplaceGrid {
    int mx, my, mz;
    bool sides_ok() const { return mx >= 2 && my >= 2 && (mz == 0 || mz >= 2); }
    int64_t rows() const { return (mz ? 3 * (int64_t)mz : 2) * mx * my; }
    int64_t unit_rows() const { return mz ? 3 * (int64_t)mx * my : 2 * (int64_t)mx; }   // rows of a node line / plane
    int units() const { return mz ? mz : my; }                                          // the lines / planes to share out
    const char *unit_name() const { return mz ? "planes" : "lines"; }
    int64_t slab_nnz(int64_t rb, int64_t re) const { return mz ? SpkAssemblySlabNnz3D(mx, my, mz, rb, re) : SpkAssemblySlabNnz(mx, my, rb, re); }
    int row_pointers(int64_t rb, int64_t re, int32_t *rowptr) const
    {
        return mz ? SpkAssemblyRowPointers3D(mx, my, mz, rb, re, rowptr) : SpkAssemblyRowPointers(mx, my, rb, re, rowptr);
    }
    int64_t launch_grid(int u0, int u1) const { return mz ? k::assemble_laplace3d_grid(mx, my, u0, u1) : k::assemble_laplace_grid(mx, u0, u1); }
    void launch(int u0, int u1, const double *kappa_d, int apply_bc, int32_t *rowptr, int32_t *colidx, double *val, double *f, hipStream_t s) const
    {
        if (mz) k::assemble_laplace3d(mx, my, mz, u0, u1, kappa_d, apply_bc, rowptr, colidx, val, f, s);
        else k::assemble_laplace(mx, my, u0, u1, kappa_d, apply_bc, rowptr, colidx, val, f, s);
    }
};

// ... the other: the assembly kernel writes it where the chain reads it (kappa_d: on the device, or null)
static void a_bring_laplace(spk_ctx *c, const LaplaceGrid &g, int64_t row_begin, int32_t n, int64_t nnz, const double *kappa_d, int apply_bc,
                            double *f_dev, SlabIn &in)
{
    hipStream_t s = c->stream;
    in.rowptr.alloc_raw((size_t)n + 1, 8);
    in.colidx.alloc_raw((size_t)nnz, 16);
    in.val.alloc_raw((size_t)nnz, 16);
    const int u0 = (int)(row_begin / g.unit_rows());
    SPK_HIP(hipStreamSynchronize(s));
    const auto t0 = std::chrono::steady_clock::now();
    g.launch(u0, u0 + (int)(n / g.unit_rows()), kappa_d, apply_bc, in.rowptr.p, in.colidx.p, in.val.p, f_dev, s);
    SPK_HIP(hipStreamSynchronize(s));
    c->assembly_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// Validation, device part: off-rank entries per row (and the column range check), exclusive scan
static void a_check_device(spk_ctx *c, int64_t row_begin, int32_t n, int64_t ncols_global, SlabIn &in)
{
    hipStream_t s = c->stream;
    DevBuf<int32_t> cnt, scratch;
    cnt.alloc_raw((size_t)n, 8);
    in.orp.alloc_raw((size_t)n + 1, 8);
    scratch.alloc_raw((size_t)n / 2048 + 8);
    in.flags.alloc(4);
    k::csr_count_off(in.rowptr.p, in.colidx.p, n, row_begin, row_begin + n, ncols_global, cnt.p, in.flags.p, s);
    k::exclusive_scan_i32(cnt.p, n, in.orp.p, scratch.p, s);
    int32_t hflags[4] = {0, 0, 0, 0};
    SPK_HIP(hipMemcpyAsync(hflags, in.flags.p, sizeof hflags, hipMemcpyDeviceToHost, s));
    SPK_HIP(hipMemcpyAsync(&in.noff, in.orp.p + n, sizeof in.noff, hipMemcpyDeviceToHost, s));
    SPK_HIP(hipStreamSynchronize(s));
    if (hflags[0]) fail(SPK_ERR_ARG, "A00: column %d out of range [0,%lld)", hflags[1], (long long)ncols_global);
}

// Validation passed: from here on the previous operator is being replaced (a refused block leaves it in place and usable).
static void a_replace_state(spk_ctx *c, int64_t row_begin, int32_t nrows_local, int64_t ncols_global)
{
    c->have_A = false;
    c->pc_ready = false;
    if (c->n_global != ncols_global || c->row_begin != row_begin || c->n_local != nrows_local) {
        // another row range: a constraint block set before belongs to the old one (its column slice and every
        // array sized by it); KSPSetOperators has to bring the new A10 as well
        c->have_B = false;
        c->m = 0;
        c->b_general = false;
        c->m_wide = 0;
        c->bd.release();
        c->bdpk.release();
    }
    c->n_global = ncols_global;
    c->row_begin = row_begin;
    c->n_local = nrows_local;
}

// Diagonal block with local columns into Ad, off-rank entries into Ao (global columns still).  What the host still
// needs comes back: the diagonal block's row pointers (tile tables are a greedy scan of them) and the few off-rank
// entries (ghost numbering, halo plan).
static void a_split(spk_ctx *c, const SlabIn &in, const int32_t *rowptr, HostBuf<int32_t> &drp, std::vector<int32_t> &orp_h,
                    std::vector<int32_t> &ocol_h)
{
    hipStream_t s = c->stream;
    const int32_t n = c->n_local, noff = in.noff;
    const int64_t lo = c->row_begin, nnzd = (int64_t)rowptr[n] - noff;
    CsrDev &Ad = c->Ad;
    Ad.nrows = n;
    Ad.ncols = n;
    Ad.nnz = nnzd;
    Ad.rowptr.alloc_raw((size_t)n + 1, 8);
    Ad.colidx.alloc_raw((size_t)nnzd, 16);
    Ad.val.alloc_raw((size_t)nnzd, 16);
    c->Ao.nrows = 0;
    c->Ao.ncols = 0;
    c->Ao.nnz = noff;
    c->Ao.colidx.alloc_raw((size_t)noff, 16);
    c->Ao.val.alloc_raw((size_t)noff, 16);
    k::csr_split(in.rowptr.p, in.colidx.p, in.val.p, n, lo, lo + n, in.orp.p, Ad.rowptr.p, Ad.colidx.p, Ad.val.p, c->Ao.colidx.p,
                 c->Ao.val.p, s);
    drp.alloc((size_t)n + 1);
    ocol_h.resize((size_t)noff);
    if (noff > 0) {
        orp_h.resize((size_t)n + 1);
        SPK_HIP(hipMemcpyAsync(orp_h.data(), in.orp.p, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, s));
        SPK_HIP(hipMemcpyAsync(ocol_h.data(), c->Ao.colidx.p, sizeof(int32_t) * (size_t)noff, hipMemcpyDeviceToHost, s));
        SPK_HIP(hipStreamSynchronize(s));
    }
    parallel_for((int64_t)n + 1, [&](int64_t r0, int64_t r1, int) {
        for (int64_t r = r0; r < r1; ++r) drp[(size_t)r] = rowptr[r] - (noff > 0 ? orp_h[(size_t)r] : 0);
    });
    std::vector<int32_t> tr;
    k::build_tiles(drp.data(), n, tr);
    Ad.ntiles = (int32_t)tr.size() - 1;
    Ad.tile_row.upload(tr.data(), tr.size(), 8);
}

// Off-rank block: columns as ghost numbers; compressed to the rows that have entries (FP32 sweeps), and over all rows
// (SpMV epilogue: the scan result of the validation, kept).
static void a_offrank(spk_ctx *c, SlabIn &in, const std::vector<int32_t> &orp_h, std::vector<int32_t> &ocol_h, std::vector<int32_t> &garray)
{
    garray = ocol_h;
    ghost_list(garray);
    c->n_ghost = (int32_t)garray.size();
    if (in.noff > 0) {
        ghost_renumber(garray, ocol_h.data(), ocol_h.size());
        SPK_HIP(hipMemcpyAsync(c->Ao.colidx.p, ocol_h.data(), sizeof(int32_t) * ocol_h.size(), hipMemcpyHostToDevice, c->stream));
        SPK_HIP(hipStreamSynchronize(c->stream));
    }
    std::vector<int32_t> rows, corp;
    compress_offrank_rows(in.noff > 0 ? orp_h.data() : nullptr, c->n_local, rows, corp);
    c->Ao.nrows = (int32_t)rows.size();
    c->Ao.ncols = c->n_ghost;
    c->Ao.rowptr.upload(corp.data(), corp.size(), 8);
    c->ao_rows.upload(rows.data(), rows.size(), 8);
    c->ao_rowptr_full.release();
    if (c->n_ghost > 0) c->ao_rowptr_full = std::move(in.orp);
}

// A bs x bs-blocked copy of Ad when every bs rows share their pattern and columns come in runs of bs (dof-bs grids):
// verified and filled by one kernel (`fill(nbr, nb)` allocates the value planes and launches it), block row br starting
// at block rowptr[bs br] / bs^2; then the dictionary over it.  Every path that does not end with A.ok releases.
template <class Blocked, class Fill, class Release>
static void blocked_copy(spk_ctx *c, Blocked &A, int bs, bool attempt, const HostBuf<int32_t> &drp, DevBuf<int32_t> &flags, Fill fill,
                         void (*tiles)(const int32_t *, int32_t, std::vector<int32_t> &), Release release_values)
{
    hipStream_t s = c->stream;
    const int32_t n = c->Ad.nrows, bb = bs * bs;
    A.ok = false;
    A.nbrows = 0;
    A.ntiles = 0;
    if (attempt && n % bs == 0 && n > 0 && c->Ad.nnz % bb == 0) {
        const int32_t nbr = n / bs;
        const int64_t nb = c->Ad.nnz / bb;
        int32_t hflags[4] = {0, 0, 0, 0};
        A.browptr.alloc_raw((size_t)nbr + 1, 8);
        A.bcol.alloc_raw((size_t)nb, 16);
        SPK_HIP(hipMemsetAsync(flags.p, 0, sizeof(int32_t) * 4, s));
        fill(nbr, nb);
        SPK_HIP(hipMemcpyAsync(hflags, flags.p, sizeof hflags, hipMemcpyDeviceToHost, s));
        SPK_HIP(hipStreamSynchronize(s));
        if (!hflags[0]) {
            HostBuf<int32_t> brp;
            brp.alloc((size_t)nbr + 1);
            parallel_for((int64_t)nbr + 1, [&](int64_t b0, int64_t b1, int) {
                for (int64_t br = b0; br < b1; ++br) brp[(size_t)br] = drp[(size_t)(bs * br)] / bb;
            });
            std::vector<int32_t> tb;
            tiles(brp.data(), nbr, tb);
            A.nbrows = nbr;
            A.nblocks = nb;
            A.ntiles = (int32_t)tb.size() - 1;
            A.tile_brow.upload(tb.data(), tb.size(), 8);
            A.ok = true;
            return build_dict(c, bs, brp.data());
        }
    }
    A.browptr.release();
    A.bcol.release();
    release_values();
}

// 2x2 (dof-2 grids), else 3x3 (the 3-D generator: 81 entries per row in 27 blocks); the format of the product last.
static void a_blocked_copies(spk_ctx *c, const HostBuf<int32_t> &drp, DevBuf<int32_t> &flags)
{
    hipStream_t s = c->stream;
    const CsrDev &Ad = c->Ad;
    BcsrDev &Ab = c->Ab;
    Bcsr3Dev &A3 = c->Ab3;
    c->Adict.ok = false;
    blocked_copy(c, Ab, 2, true, drp, flags, [&](int32_t nbr, int64_t nb) {
        Ab.vtop.alloc_raw((size_t)(2 * nb), 32);
        Ab.vbot.alloc_raw((size_t)(2 * nb), 32);
        k::bcsr_fill(Ad.rowptr.p, Ad.colidx.p, Ad.val.p, nbr, Ab.browptr.p, Ab.bcol.p, Ab.vtop.p, Ab.vbot.p, flags.p, s);
    }, k::build_btiles, [&] { Ab.vtop.release(); Ab.vbot.release(); });
    A3.v32.release();
    blocked_copy(c, A3, 3, !Ab.ok, drp, flags, [&](int32_t nbr, int64_t nb) {
        A3.ldp = (nb + 1 + 7) & ~(int64_t)7;
        A3.v.alloc_raw((size_t)(9 * A3.ldp), 32);
        k::bcsr3_fill(Ad.rowptr.p, Ad.colidx.p, Ad.val.p, nbr, A3.browptr.p, A3.bcol.p, A3.v.p, A3.ldp, flags.p, s);
    }, k::build_b3tiles, [&] { A3.v.release(); });
    const char *fmt = getenv("SPK_SPMV_FORMAT");
    const bool csr_forced = fmt && !strcmp(fmt, "csr");
    c->spmv_format = csr_forced ? 0 : (Ab.ok ? 1 : (A3.ok ? 2 : 0));
}

// the halo plan into the context, with its device arrays
static void a_install_halo(spk_ctx *c, HaloPlan &h)
{
    c->send_idx.upload(h.send_idx.data(), h.send_idx.size(), 8);
    c->send_buf.alloc(h.send_idx.size(), 8);
    const HostSendRanges R = send_ranges(h);
    c->send_ranges = k::SendRanges{};
    c->send_ranges.n = R.n;
    std::copy(R.r0, R.r0 + 4, c->send_ranges.r0);
    std::copy(R.len, R.len + 4, c->send_ranges.len);
    std::copy(R.off, R.off + 4, c->send_ranges.off);
    if (R.n) c->send_ranges.buf = c->send_buf.p;
    c->peers = std::move(h.peers);
    c->send_off = std::move(h.send_off);
    c->recv_off = std::move(h.recv_off);
    c->xghost.alloc((size_t)c->n_ghost, 8);
}

// One chain for both sources of the slab.  prepare(): the source's own refusals and the host row pointers (returned),
// before anything is allocated; bring(in): the slab into device memory.
template <class Prepare, class Bring>
static void set_block_A(spk_ctx *c, int64_t row_begin, int32_t nrows_local, int64_t ncols_global, Prepare prepare, Bring bring)
{
    std::vector<int32_t> garray;   // sorted global numbers of the off-rank columns (MatMPIAIJ's garray)
    // ---- local part: validation, upload or assembly, split and blocking on the device (no collective inside)
    agree_or_fail(c, locally([&] {
        SlabIn in;
        HostBuf<int32_t> drp;
        std::vector<int32_t> orp_h, ocol_h;
        const int32_t *rowptr = prepare();
        a_check_host(row_begin, nrows_local, ncols_global, rowptr);
        bring(in);
        a_check_device(c, row_begin, nrows_local, ncols_global, in);
        a_replace_state(c, row_begin, nrows_local, ncols_global);
        a_split(c, in, rowptr, drp, orp_h, ocol_h);
        a_offrank(c, in, orp_h, ocol_h, garray);
        a_blocked_copies(c, drp, in.flags);
    }), "A00");
    // ---- halo plan (VecScatter of MatMult_MPIAIJ): every rank's slab and ghosts, then local again -- the plan and its
    // uploads, agreed on before the collective setup_halo
    const int P = c->comm->size(), me = c->comm->rank();
    std::vector<int64_t> slabs((size_t)2 * P, row_begin);
    std::vector<std::vector<char>> ghosts(1);
    slabs[1] = row_begin + nrows_local;
    if (P > 1) {
        const int64_t mine[2] = {slabs[0], slabs[1]};
        c->comm->host_allgather(mine, slabs.data(), sizeof mine);
        c->comm->host_allgatherv(garray.data(), garray.size() * sizeof(int32_t), ghosts);
    }
    agree_or_fail(c, locally([&] {
        if (P == 1 && c->n_ghost != 0)
            fail(SPK_ERR_ARG, "A00: %d columns fall outside the local rows but there is only one rank", c->n_ghost);
        HaloPlan h;
        halo_plan(me, P, slabs.data(), garray, ghosts, h);
        a_install_halo(c, h);
    }), "A00 (halo plan)");
    c->comm->setup_halo(c->n_ghost, c->peers, c->send_off, c->recv_off);  // collective
    c->have_A = true;
    c->pc_ready = false;
    c->ensure_vectors();
}

// ---------------------------------------------------------------------------
// KSPSetOperators, A10: this rank's column slice of the constraint block
// ---------------------------------------------------------------------------
// Column windows over the wide rows (concatenated in `wide` order); for m <= 8 every row, in order: the arrays as they are.
constexpr int32_t kWideRowNnz = 8192;   // a general block's rows beyond this many local entries take the window kernel
static void b_windows(spk_ctx *c, int32_t m, const int32_t *rowptr, const int32_t *col, const double *v, const std::vector<int32_t> &wide)
{
    WideDev &B = c->B;
    const int32_t nl = c->n_local, mw = (int32_t)wide.size();
    std::vector<int32_t> wcol_own, wrp;
    std::vector<double> wv_own;
    if (!c->b_general) {
        wrp.assign(1, 0);
        for (int32_t r = 0; r < m; ++r) wrp.push_back(rowptr[r + 1]);
    } else {
        gather_rows(m, rowptr, col, v, wide, false, wrp, wcol_own, wv_own);
        col = wcol_own.data();
        v = wv_own.data();
    }
    B.m = mw;
    B.ncols = nl;
    B.nnz = wrp.back();
    B.win = window_width(nl, k::kMaxBlocks);
    B.nwin = mw > 0 ? (nl + B.win - 1) / B.win : 0;
    std::vector<int32_t> winptr((size_t)(B.nwin + 1) * (size_t)std::max(mw, 1));
    window_pointers(mw, wrp.data(), col, nl, B.win, B.nwin, winptr.data());
    up(c, B.colidx, col, (size_t)B.nnz, 16);
    up(c, B.val, v, (size_t)B.nnz, 16);
    B.winptr.upload(winptr.data(), winptr.size(), 8);
}

// the rows that take the window kernel (wide_rows, spk_host.cpp), into the context
static void b_install_wide(spk_ctx *c, const std::vector<int32_t> &wide)
{
    c->m_wide = (int32_t)wide.size();
    c->wide_rows_h = wide;
    c->wide_rows.upload(wide.data(), wide.size(), 8);
}

static void b_release_general(spk_ctx *c)
{
    c->Bc.rowptr.release(); c->Bc.colidx.release(); c->Bc.val.release(); c->Bc.tile_row.release();
    c->Bc.nrows = c->Bc.ncols = c->Bc.ntiles = 0;
    c->Bc.nnz = 0;
    c->Bt.tile_row.release();   // (B^T is tiled for a general block only: upload_csr builds the table again then)
    c->Bt.ntiles = 0;
}

// One source of the block: the caller's arrays, localised, windowed and transposed on the host and uploaded
static void b_bring_upload(spk_ctx *c, int32_t m, const int32_t *rowptr, const int32_t *colidx, const double *val)
{
    const int32_t nl = c->n_local;
    HostBuf<int32_t> col;
    HostBuf<double> v;
    col.alloc((size_t)rowptr[m]);
    v.alloc((size_t)rowptr[m]);
    localise_and_sort(m, rowptr, colidx, val, c->row_begin, c->row_begin + nl, col.data(), v.data());
    c->b_general = m > 8;
    const std::vector<int32_t> wide = wide_rows(m, rowptr, kWideRowNnz);
    b_install_wide(c, wide);
    b_windows(c, m, rowptr, col.data(), v.data(), wide);
    // the general block by rows (its long rows left empty: the window kernel fills their results in)
    b_release_general(c);
    if (c->b_general) {
        std::vector<int32_t> crp, cci;
        std::vector<double> cv;
        gather_rows(m, rowptr, col.data(), v.data(), wide, true, crp, cci, cv);
        upload_csr(c, c->Bc, m, nl, crp, cci, cv, true);
    }
    // B^T by rows (n_local x m), entries of a row ordered by constraint index
    std::vector<int32_t> trp((size_t)nl + 1, 0), tci((size_t)rowptr[m]);
    std::vector<double> tv((size_t)rowptr[m]);
    transpose_rows(m, nl, rowptr, col.data(), v.data(), trp.data(), tci.data(), tv.data());
    upload_csr(c, c->Bt, nl, m, trp, tci, tv, c->b_general);   // (a general block: tiles for the stream kernel)
}

// One chain for both sources of the block.  prepare(): the source's own refusals, before anything of the previous block
// is touched; bring(): c->B, c->Bt (a general block: c->Bc), b_general and the wide rows, in device memory.
template <class Prepare, class Bring>
static void set_block_B(spk_ctx *c, int32_t m, int64_t ncols_global, Prepare prepare, Bring bring)
{
    if (!c->have_A) fail(SPK_ERR_STATE, "A10: set SPK_BLOCK_A00 first");
    c->bt_cached = nullptr;
    if (ncols_global != c->n_global) fail(SPK_ERR_ARG, "A10: %lld columns, A00 has %lld", (long long)ncols_global, (long long)c->n_global);
    if (m < 0) fail(SPK_ERR_ARG, "A10: negative row count");
    if ((int64_t)c->n_local + m > INT32_MAX - 1024) fail(SPK_ERR_UNSUPPORTED, "A10: n_local + m exceeds 32-bit vector indices");
    prepare();
    bring();
    if ((size_t)m + 64 > c->y1tmp.n) c->y1tmp.alloc((size_t)m + 64);
    if ((size_t)m + 64 > c->ttmp.n) c->ttmp.alloc((size_t)m + 64);
    c->m = m;
    c->have_B = m > 0;
    c->pc_ready = false;
    c->ensure_vectors();
    if (c->b_general && c->tmpb.n < (size_t)c->ld) c->tmpb.alloc((size_t)c->ld);   // scratch of the B^T products (bt_update)
}

void set_block(spk_ctx *c, int which, int64_t row_begin, int32_t nrows_local, int64_t ncols_global,
               const int32_t *rowptr, const int32_t *colidx, const double *val)
{
    if (!rowptr || (!colidx && rowptr[nrows_local] > 0) || (!val && rowptr[nrows_local] > 0))
        fail(SPK_ERR_ARG, "set_block: null array");
    if (nrows_local < 0) fail(SPK_ERR_ARG, "set_block: negative row count");
    c->ensure_scratch();
    if (which == SPK_BLOCK_A00)
        set_block_A(c, row_begin, nrows_local, ncols_global, [&] { return rowptr; },
                    [&](SlabIn &in) { a_bring_upload(c, nrows_local, rowptr, colidx, val, in); });
    else if (which == SPK_BLOCK_A10)
        // no collective inside, but every rank sets its column slice: agree on the outcome so that a rank
        // whose slice was refused does not leave the others to run into the next collective alone
        agree_or_fail(c, locally([&] {
            set_block_B(c, nrows_local, ncols_global, [&] {
                for (int32_t r = 0; r < nrows_local; ++r)
                    if (rowptr[r + 1] < rowptr[r]) fail(SPK_ERR_ARG, "A10: rowptr not monotone at row %d", r);
            }, [&] { b_bring_upload(c, nrows_local, rowptr, colidx, val); });
        }), "A10");
    else fail(SPK_ERR_ARG, "set_block: unknown block %d", which);
}

// ---------------------------------------------------------------------------
// KSPSetOperators, A00 of the reference's own discretisation: the slab assembled on the device
// ---------------------------------------------------------------------------
// kappa on the device, checked: a host array is checked on the host and uploaded, a device array by one kernel.  Null stays null.
// mz == 0: the 2-D grid.
static const double *kappa_on_device(spk_ctx *c, int mx, int my, int mz, const double *kappa, int kappa_mem, DevBuf<double> &own)
{
    if (!kappa) return nullptr;
    if (kappa_mem != SPK_MEM_HOST && kappa_mem != SPK_MEM_DEVICE) fail(SPK_ERR_ARG, "device assembly: kappa_mem %d", kappa_mem);
    const int64_t ne = (int64_t)(mx - 1) * (my - 1) * (mz ? mz - 1 : 1);
    const char *bad = "device assembly: an entry of kappa is not finite and > 0";
    if (kappa_mem == SPK_MEM_HOST) {
        if ((mz ? SpkAssemblyCheckKappa3D(mx, my, mz, kappa) : SpkAssemblyCheckKappa(mx, my, kappa)) != SPK_OK) fail(SPK_ERR_ARG, "%s", bad);
        own.upload(kappa, (size_t)ne);
        return own.p;
    }
    DevBuf<int32_t> flag;
    flag.alloc(4);
    int32_t h = 1;
    k::kappa_check(kappa, ne, flag.p, c->stream);
    SPK_HIP(hipMemcpyAsync(&h, flag.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    SPK_HIP(hipStreamSynchronize(c->stream));
    if (h) fail(SPK_ERR_ARG, "%s", bad);
    return kappa;
}

// the refusals that need no GPU; returns the slab's stored non-zeros.  (The launch grid of a 2-D slab is at most half its
// node count, so that limit can only stop a 3-D grid.)
static int64_t laplace_slab_limits(const LaplaceGrid &g, int64_t row_begin, int64_t row_end)
{
    if (!g.sides_ok()) {
        if (g.mz) fail(SPK_ERR_ARG, "device assembly: a grid of %d x %d x %d nodes (at least 2 x 2 x 2)", g.mx, g.my, g.mz);
        fail(SPK_ERR_ARG, "device assembly: a grid of %d x %d nodes (at least 2 x 2)", g.mx, g.my);
    }
    if (g.rows() > INT32_MAX) fail(SPK_ERR_UNSUPPORTED, "device assembly: %lld rows exceed 32-bit indices", (long long)g.rows());
    const int64_t nnz = g.slab_nnz(row_begin, row_end);
    if (nnz < 0)
        fail(SPK_ERR_ARG, "device assembly: rows [%lld,%lld) are not whole node %s of the grid", (long long)row_begin, (long long)row_end, g.unit_name());
    if (nnz > INT32_MAX) fail(SPK_ERR_UNSUPPORTED, "device assembly: %lld stored non-zeros of the slab exceed 32-bit indices", (long long)nnz);
    const int64_t grid = g.launch_grid((int)(row_begin / g.unit_rows()), (int)(row_end / g.unit_rows()));
    if (grid > INT32_MAX) fail(SPK_ERR_UNSUPPORTED, "device assembly: %lld workgroups exceed the launch grid", (long long)grid);
    return nnz;
}

int laplace_mz3(int mx, int my, int mz)
{
    if (mz == 0) fail(SPK_ERR_ARG, "device assembly: a grid of %d x %d x %d nodes (at least 2 x 2 x 2)", mx, my, mz);
    return mz;
}

void set_block_laplace(spk_ctx *c, int mx, int my, int mz, const double *kappa, int kappa_mem, int apply_bc, double *f_dev)
{
    const LaplaceGrid g{mx, my, mz};
    c->ensure_scratch();
    int64_t rb = 0, re = 0, nnz = 0;
    // sizes first, and only where they make sense (the chain's own refusal path reports the rest)
    const bool sane = g.sides_ok() && g.rows() <= INT32_MAX;
    if (sane && spk_partition_slab(g.units(), g.unit_rows(), c->comm->rank(), c->comm->size(), &rb, &re) != SPK_OK)
        fail(SPK_ERR_ARG, "device assembly: spk_partition_slab failed");
    const int32_t n = (int32_t)(re - rb);
    HostBuf<int32_t> rowptr;
    DevBuf<double> kappa_own;
    const double *kappa_d = nullptr;
    set_block_A(c, rb, n, g.rows(), [&] {
        nnz = laplace_slab_limits(g, rb, re);
        kappa_d = kappa_on_device(c, mx, my, mz, kappa, kappa_mem, kappa_own);
        rowptr.alloc((size_t)n + 1);
        if (g.row_pointers(rb, re, rowptr.data()) != SPK_OK) fail(SPK_ERR_UNSUPPORTED, "device assembly: row pointers beyond 32-bit indices");
        return (const int32_t *)rowptr.data();
    }, [&](SlabIn &in) { a_bring_laplace(c, g, rb, n, nnz, kappa_d, apply_bc, f_dev, in); });
}

void assemble_laplace_csr(spk_ctx *c, int mx, int my, int mz, int64_t row_begin, int64_t row_end, const double *kappa, int kappa_mem,
                          int apply_bc, int32_t *rowptr, int32_t *colidx, double *val, double *f)
{
    const LaplaceGrid g{mx, my, mz};
    if (!rowptr || !colidx || !val) fail(SPK_ERR_ARG, "assemble_laplace%s_csr: null array", mz ? "3d" : "");
    const int64_t nnz = laplace_slab_limits(g, row_begin, row_end);
    DevBuf<double> kappa_own, fd;
    const double *kappa_d = kappa_on_device(c, mx, my, mz, kappa, kappa_mem, kappa_own);
    const int32_t n = (int32_t)(row_end - row_begin);
    SlabIn in;
    if (f) fd.alloc_raw((size_t)n, 8);
    const double keep = c->assembly_seconds;
    a_bring_laplace(c, g, row_begin, n, nnz, kappa_d, apply_bc, f ? fd.p : nullptr, in);
    c->assembly_seconds = keep;   // (a test hook: the context's last assembly is the operator's)
    SPK_HIP(hipMemcpy(rowptr, in.rowptr.p, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyDeviceToHost));
    SPK_HIP(hipMemcpy(colidx, in.colidx.p, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost));
    SPK_HIP(hipMemcpy(val, in.val.p, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToHost));
    if (f) SPK_HIP(hipMemcpy(f, fd.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
}

// ---------------------------------------------------------------------------
// KSPSetOperators, A10 of the reference's own discretisation: the column slice written on the device
// ---------------------------------------------------------------------------
namespace cs = spk::constraints;

// the refusals that need no GPU; returns the slab (mz == 0: the 2-D grid)
static cs::Slab constraints_slab(int mx, int my, int mz, int64_t row_begin, int64_t row_end)
{
    if (mx < 3 || my < 3 || (mz != 0 && mz < 3)) {
        if (mz) fail(SPK_ERR_ARG, "device constraints: a grid of %d x %d x %d nodes (at least 3 x 3 x 3)", mx, my, mz);
        fail(SPK_ERR_ARG, "device constraints: a grid of %d x %d nodes (at least 3 x 3)", mx, my);
    }
    const LaplaceGrid lg{mx, my, mz};
    if (lg.rows() > INT32_MAX) fail(SPK_ERR_UNSUPPORTED, "device constraints: %lld columns exceed 32-bit indices", (long long)lg.rows());
    const int64_t nnz = mz ? SpkConstraintsSlabNnz3D(mx, my, mz, row_begin, row_end) : SpkConstraintsSlabNnz(mx, my, row_begin, row_end);
    if (nnz < 0)
        fail(SPK_ERR_ARG, "device constraints: rows [%lld,%lld) are not whole node %s of the grid", (long long)row_begin, (long long)row_end,
             lg.unit_name());
    if (nnz > INT32_MAX) fail(SPK_ERR_UNSUPPORTED, "device constraints: %lld stored non-zeros of the slice exceed 32-bit indices", (long long)nnz);
    const cs::Slab g{mx, my, mz, (int)(row_begin / lg.unit_rows()), (int)(row_end / lg.unit_rows())};
    if (cs::nnz(g) != nnz) fail(SPK_ERR_STATE, "device constraints: the closed-form entry count disagrees with the generator's");
    return g;
}

// B, B^T and the window pointers of the slab into fresh device arrays, with the pads of the host route's uploads
static void constraints_fill(spk_ctx *c, const cs::Slab &g, WideDev &B, CsrDev &Bt)
{
    hipStream_t s = c->stream;
    const int32_t m = cs::rows(g), nl = (int32_t)cs::local_cols(g);
    const int64_t nnz = cs::nnz(g);
    B.m = m;
    B.ncols = nl;
    B.nnz = nnz;
    B.win = window_width(nl, k::kMaxBlocks);
    B.nwin = (nl + B.win - 1) / B.win;
    B.colidx.alloc_raw((size_t)nnz, 16);
    B.val.alloc_raw((size_t)nnz, 16);
    B.winptr.alloc_raw((size_t)(B.nwin + 1) * (size_t)m, 8);
    Bt.nrows = nl;
    Bt.ncols = m;
    Bt.nnz = nnz;
    Bt.rowptr.alloc_raw((size_t)nl + 1, 8);
    Bt.colidx.alloc_raw((size_t)nnz, 16);
    Bt.val.alloc_raw((size_t)nnz, 16);
    SPK_HIP(hipStreamSynchronize(s));
    const auto t0 = std::chrono::steady_clock::now();
    k::assemble_constraints(g.mx, g.my, g.mz, g.u0, g.u1, B.colidx.p, B.val.p, Bt.rowptr.p, Bt.colidx.p, Bt.val.p, B.win, B.nwin,
                            B.winptr.p, s);
    SPK_HIP(hipStreamSynchronize(s));
    c->constraints_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

void set_block_constraints(spk_ctx *c, int mx, int my, int mz, double *g_dev)
{
    c->ensure_scratch();
    // every rank fills the column slice of the rows A00 gave it; agreed on as set_block(A10) is
    agree_or_fail(c, locally([&] {
        cs::Slab g{};
        const int32_t m = mz ? 6 : 4;
        set_block_B(c, m, (int64_t)(mz ? 3 : 2) * mx * my * (mz ? mz : 1),
                    [&] { g = constraints_slab(mx, my, mz, c->row_begin, c->row_begin + c->n_local); },
                    [&] {
                        c->b_general = false;
                        std::vector<int32_t> wide((size_t)m);
                        for (int32_t r = 0; r < m; ++r) wide[(size_t)r] = r;
                        b_install_wide(c, wide);
                        b_release_general(c);
                        constraints_fill(c, g, c->B, c->Bt);
                    });
        if (g_dev) {
            double gh[6];
            if ((mz ? SpkAssembleRHS_Constraints3D(gh) : SpkAssembleRHS_Constraints(gh)) != SPK_OK) fail(SPK_ERR_STATE, "device constraints: g");
            SPK_HIP(hipMemcpy(g_dev, gh, sizeof(double) * (size_t)m, hipMemcpyHostToDevice));
        }
    }), "A10 (device)");
}

void assemble_constraints_csr(spk_ctx *c, int mx, int my, int mz, int64_t row_begin, int64_t row_end, int32_t *b_colidx, double *b_val,
                              int32_t *bt_rowptr, int32_t *bt_colidx, double *bt_val, int32_t *win, int32_t *nwin, int32_t *winptr,
                              int64_t winptr_cap)
{
    if (!b_colidx || !b_val || !bt_rowptr || !bt_colidx || !bt_val || !win || !nwin || !winptr)
        fail(SPK_ERR_ARG, "assemble_constraints_csr: null array");
    const cs::Slab g = constraints_slab(mx, my, mz, row_begin, row_end);
    WideDev B;
    CsrDev Bt;
    const double keep = c->constraints_seconds;
    constraints_fill(c, g, B, Bt);
    c->constraints_seconds = keep;   // (a test hook: the context's last figure is the operator's)
    const size_t nw = (size_t)(B.nwin + 1) * (size_t)B.m;
    if ((int64_t)nw > winptr_cap) fail(SPK_ERR_ARG, "assemble_constraints_csr: %zu window pointers, room for %lld", nw, (long long)winptr_cap);
    *win = B.win;
    *nwin = B.nwin;
    SPK_HIP(hipMemcpy(b_colidx, B.colidx.p, sizeof(int32_t) * (size_t)B.nnz, hipMemcpyDeviceToHost));
    SPK_HIP(hipMemcpy(b_val, B.val.p, sizeof(double) * (size_t)B.nnz, hipMemcpyDeviceToHost));
    SPK_HIP(hipMemcpy(winptr, B.winptr.p, sizeof(int32_t) * nw, hipMemcpyDeviceToHost));
    SPK_HIP(hipMemcpy(bt_rowptr, Bt.rowptr.p, sizeof(int32_t) * ((size_t)Bt.nrows + 1), hipMemcpyDeviceToHost));
    SPK_HIP(hipMemcpy(bt_colidx, Bt.colidx.p, sizeof(int32_t) * (size_t)Bt.nnz, hipMemcpyDeviceToHost));
    SPK_HIP(hipMemcpy(bt_val, Bt.val.p, sizeof(double) * (size_t)Bt.nnz, hipMemcpyDeviceToHost));
}

// The same arrays by the host chain (the generator, localise_and_sort, window_pointers, transpose_rows): what
// set_block(A10) uploads for the generated block.  Needs no GPU; the reference of the tests and of tools/assembly_bench.py.
void host_constraints_csr(int mx, int my, int mz, int64_t row_begin, int64_t row_end, int32_t *b_colidx, double *b_val,
                          int32_t *bt_rowptr, int32_t *bt_colidx, double *bt_val, int32_t *win, int32_t *nwin, int32_t *winptr,
                          int64_t winptr_cap)
{
    if (!b_colidx || !b_val || !bt_rowptr || !bt_colidx || !bt_val || !win || !nwin || !winptr)
        fail(SPK_ERR_ARG, "host_constraints_csr: null array");
    const int64_t nnz = mz ? SpkConstraintsSlabNnz3D(mx, my, mz, row_begin, row_end) : SpkConstraintsSlabNnz(mx, my, row_begin, row_end);
    if (nnz < 0 || nnz > INT32_MAX || row_end - row_begin > INT32_MAX) fail(SPK_ERR_ARG, "host_constraints_csr: not a slab of the grid");
    const int32_t m = mz ? 6 : 4, nl = (int32_t)(row_end - row_begin);
    std::vector<int32_t> rowptr((size_t)m + 1), colidx((size_t)nnz + 1);   // (+ 1: the generator refuses a null array)
    std::vector<double> val((size_t)nnz + 1);
    const int rc = mz ? SpkAssembleOperator_Constraints3D(mx, my, mz, row_begin, row_end, rowptr.data(), colidx.data(), val.data())
                      : SpkAssembleOperator_Constraints(mx, my, row_begin, row_end, rowptr.data(), colidx.data(), val.data());
    if (rc != SPK_OK) fail(rc, "host_constraints_csr: the generator refused");
    localise_and_sort(m, rowptr.data(), colidx.data(), val.data(), row_begin, row_end, b_colidx, b_val);
    const std::vector<int32_t> wide = wide_rows(m, rowptr.data(), kWideRowNnz);
    if ((int32_t)wide.size() != m) fail(SPK_ERR_STATE, "host_constraints_csr: wide rows");
    *win = window_width(nl, k::kMaxBlocks);
    *nwin = (nl + *win - 1) / *win;
    if ((int64_t)(*nwin + 1) * m > winptr_cap) fail(SPK_ERR_ARG, "host_constraints_csr: room for %lld window pointers", (long long)winptr_cap);
    window_pointers(m, rowptr.data(), b_colidx, nl, *win, *nwin, winptr);
    std::fill(bt_rowptr, bt_rowptr + nl + 1, 0);
    transpose_rows(m, nl, rowptr.data(), b_colidx, b_val, bt_rowptr, bt_colidx, bt_val);
}

// ---------------------------------------------------------------------------
// KSPSetUp / PCSetUp: diag(A)^-1, S^ = diag(B diag(A)^-1 B^T)
// ---------------------------------------------------------------------------
// G = W D W^T over this rank's columns, W = the `rows` window rows of B: row r of W .* dinv scattered densely into the
// (zero) scratch vector, W * that = G[r, :], the scratch vector put back to zero.  dst: rows x rows on the device.
static void gram_rows(spk_ctx *c, int rows, double *dst)
{
    hipStream_t s = c->stream;
    const WideDev &B = c->B;
    SPK_HIP(hipMemsetAsync(c->tmp.p, 0, sizeof(double) * (size_t)c->ld, s));
    std::vector<int32_t> wp((size_t)(B.nwin + 1) * rows);
    SPK_HIP(hipMemcpy(wp.data(), B.winptr.p, wp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int r = 0; r < rows; ++r) {
        const int k0 = wp[(size_t)r], k1 = wp[(size_t)B.nwin * rows + r];
        k::scatter_row(B.colidx.p, B.val.p, k0, k1, c->dinv.p, c->tmp.p, s);
        k::wide_dot(B, c->tmp.p, c->fin(dst + (size_t)r * rows), nullptr, s);
        k::scatter_row(B.colidx.p, B.val.p, k0, k1, nullptr, c->tmp.p, s);
    }
}

// S^ = diag(B D B^T), summed over the ranks
static void schur_diag(spk_ctx *c)
{
    hipStream_t s = c->stream;
    const int m = c->m, mw = c->m_wide;
    if (c->b_general) {   // row by row: short rows one wave each, the long rows from their Gram matrix
        c->gram.release();
        c->shat.alloc((size_t)m, 8);
        k::schur_diag_rows(c->Bc, c->dinv.p, c->shat.p, s);
        if (mw > 0) {
            DevBuf<double> g;
            g.alloc((size_t)mw * mw);
            gram_rows(c, mw, g.p);
            for (int r = 0; r < mw; ++r)
                SPK_HIP(hipMemcpyAsync(c->shat.p + c->wide_rows_h[(size_t)r], g.p + (size_t)r * mw + r, sizeof(double),
                                       hipMemcpyDeviceToDevice, s));
            SPK_HIP(hipStreamSynchronize(s));
        }
        c->comm->allreduce_sum(c->shat.p, m, s);
        SPK_HIP(hipStreamSynchronize(s));
        return;
    }
    c->gram.alloc((size_t)m * m);
    c->shat.alloc((size_t)m);
    gram_rows(c, m, c->gram.p);
    c->comm->allreduce_sum(c->gram.p, m * m, s);
    SPK_HIP(hipStreamSynchronize(s));
    std::vector<double> G((size_t)m * m), sh((size_t)m);
    SPK_HIP(hipMemcpy(G.data(), c->gram.p, G.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int r = 0; r < m; ++r) sh[(size_t)r] = G[(size_t)r * m + r];
    SPK_HIP(hipMemcpy(c->shat.p, sh.data(), sh.size() * sizeof(double), hipMemcpyHostToDevice));
}

// FP32 copies for the inner solve: the values in the layout the product uses (with a dictionary the sweeps decode
// the codes and round to single precision), diag(A)^-1 and the sweeps' vectors
static void fp32_copies(spk_ctx *c)
{
    hipStream_t s = c->stream;
    c->a32.release(); c->d32.release(); c->x32.release(); c->y32a.release(); c->y32b.release();
    c->Ab3.v32.release();
    c->Ab.vtop32.release();
    c->Ab.vbot32.release();
    if (c->inner_sweeps <= 0) return;
    const bool dict = c->spmv_format != 0 && c->Adict.ok;
    if (!dict && c->spmv_format == 1) {   // the 2x2-blocked value planes
        c->Ab.vtop32.alloc_raw((size_t)(2 * c->Ab.nblocks + 8), 32);
        c->Ab.vbot32.alloc_raw((size_t)(2 * c->Ab.nblocks + 8), 32);
        k::cvt_vals_f32(c->Ab.vtop.p, c->Ab.vtop32.p, 2 * c->Ab.nblocks, s);
        k::cvt_vals_f32(c->Ab.vbot.p, c->Ab.vbot32.p, 2 * c->Ab.nblocks, s);
    }
    if (!dict && c->spmv_format == 2) {   // the 3x3-blocked planes
        c->Ab3.v32.alloc_raw((size_t)(9 * c->Ab3.ldp), 32);
        k::cvt_vals_f32(c->Ab3.v.p, c->Ab3.v32.p, 9 * c->Ab3.ldp, s);
    }
    if (c->spmv_format == 0) {
        c->a32.alloc((size_t)c->Ad.nnz, 32);
        k::cvt_vals_f32(c->Ad.val.p, c->a32.p, c->Ad.nnz, s);
    }
    c->d32.alloc((size_t)c->n_local, 8);
    c->x32.alloc((size_t)c->n_local, 8);
    c->y32a.alloc((size_t)c->n_local, 8);
    c->y32b.alloc((size_t)c->n_local, 8);
    k::cvt_vals_f32(c->dinv.p, c->d32.p, c->n_local, s);
}

// dense rows of B D for the fused path (Schur LOWER/FULL, even local size)
static void bd_planes(spk_ctx *c, int pc_type, int schur_fact)
{
    hipStream_t s = c->stream;
    const int m = c->m;
    c->bd.release();
    if (!(pc_type == SPK_PC_SCHUR && m > 0 && !c->b_general && (schur_fact == SPK_SCHUR_FULL || schur_fact == SPK_SCHUR_LOWER) &&
          c->even_all && c->inner_sweeps == 0 && !c->amg_d))
        return;
    c->bd.alloc((size_t)c->ld * m, 16);
    k::build_bd(c->Bt, c->dinv.p, m, c->ld, c->bd.p, s);
    // rows 2q / 2q+1 on even / odd entries (x / y degrees of freedom): m/2 planes instead of m rows
    c->bdpk.release();
    c->bd_packed = false;
    if (m % 2 == 0 && !getenv("SPK_BD_DENSE")) {
        c->bdpk.alloc((size_t)c->ld * (m / 2), 16);
        DevBuf<int32_t> bad;
        bad.alloc(1);
        k::pack_bd(c->bd.p, c->ld, c->n_local, m, c->bdpk.p, bad.p, s);
        int32_t hb = 1;
        SPK_HIP(hipMemcpyAsync(&hb, bad.p, sizeof hb, hipMemcpyDeviceToHost, s));
        SPK_HIP(hipStreamSynchronize(s));
        c->bd_packed = hb == 0;
        if (!c->bd_packed) c->bdpk.release();
    }
}

// The exact Schur complement of a few rows (spk_pc_set_schur_pre): W = A^ ^-1 B^T as m dense planes -- column r is one
// V-cycle on B^T e_r, or, A^ = diag(A), the plane build_bd writes -- then S = B W column by column, symmetrised and
// Cholesky-factored on the host; the factor goes to the device.  Throws when S is not positive definite.
static void schur_dense_build(spk_ctx *c)
{
    hipStream_t s = c->stream;
    const int m = c->m;
    const auto t0 = std::chrono::steady_clock::now();
    const double *W = nullptr;
    if (c->amg_d) {
        std::vector<double> eye((size_t)m * m, 0.0);
        for (int r = 0; r < m; ++r) eye[(size_t)r * m + r] = 1.0;
        DevBuf<double> e;
        e.upload(eye.data(), eye.size());
        c->sw.alloc((size_t)c->ld * m, 16);   // zero-filled: the V-cycle writes the local rows, the pad stays zero
        for (int r = 0; r < m; ++r) {
            k::bt_update(3, c->Bt, c->dinv.p, nullptr, e.p + (size_t)r * m, c->tmp.p, nullptr, s);   // B^T e_r
            amg_apply(c, c->tmp.p, c->sw.p + (size_t)c->ld * r, 0, nullptr);
        }
        W = c->sw.p;
    } else {
        // D B^T is what the fused path streams as `bd`: one copy serves both (here for every factorisation and any parity)
        c->sw.release();
        c->bdpk.release();
        c->bd_packed = false;
        c->bd.alloc((size_t)c->ld * m, 16);
        k::build_bd(c->Bt, c->dinv.p, m, c->ld, c->bd.p, s);
        W = c->bd.p;
    }
    DevBuf<double> g;
    g.alloc((size_t)m * m);
    for (int r = 0; r < m; ++r) apply_B(c, W + (size_t)c->ld * r, nullptr, g.p + (size_t)r * m, nullptr);   // column r of S
    std::vector<double> G((size_t)m * m), L((size_t)m * m);
    SPK_HIP(hipMemcpyAsync(G.data(), g.p, sizeof(double) * G.size(), hipMemcpyDeviceToHost, s));
    SPK_HIP(hipStreamSynchronize(s));
    c->check_device_error();
    c->schur_S.assign((size_t)m * m, 0.0);
    const int bad = schur_dense_factor(m, G.data(), c->schur_S.data(), L.data());
    if (bad >= 0)
        fail(SPK_ERR_UNSUPPORTED, "pc_setup: the exact Schur complement S = B A^-1 B^T (%d x %d) is not positive definite at "
             "pivot %d: the constraint rows are linearly dependent (rank-deficient B) -- remove the redundant row, or "
             "keep -pc_fieldsplit_schur_precondition selfp", m, m, bad);
    c->sfac.upload(L.data(), L.size());
    c->schur_setup_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

void pc_setup(spk_ctx *c, int pc_type, int schur_fact)
{
    if (!c->have_A) fail(SPK_ERR_STATE, "pc_setup: no A00 block");
    if (pc_type < SPK_PC_NONE || pc_type > SPK_PC_SCHUR) fail(SPK_ERR_ARG, "pc_setup: unknown pc_type %d", pc_type);
    if (pc_type == SPK_PC_SCHUR && !c->have_B) fail(SPK_ERR_STATE, "pc_setup: Schur fieldsplit needs the A10 block");
    if (schur_fact < SPK_SCHUR_DIAG || schur_fact > SPK_SCHUR_FULL) fail(SPK_ERR_ARG, "pc_setup: unknown schur_fact %d", schur_fact);
    // multigrid standing for A^-1: one rank only (every rank sees the same communicator size: all refuse together), built
    // on the host before anything of the context changes -- a refusal leaves it as it was
    // the exact Schur complement (spk_pc_set_schur_pre): its limits, equally before anything changes
    const bool dense = pc_type == SPK_PC_SCHUR && c->schur_pre == SPK_SCHUR_PRE_FULL;
    if (dense) {
        if (c->b_general || c->m > 8)
            fail(SPK_ERR_UNSUPPORTED, "pc_setup: the exact Schur complement (schur_precondition full) is dense and kept for at "
                 "most 8 constraint rows; this block has %d%s -- keep -pc_fieldsplit_schur_precondition selfp", (int)c->m,
                 c->b_general ? " (a general sparse block)" : "");
        if (c->comm->size() > 1)
            fail(SPK_ERR_UNSUPPORTED, "pc_setup: the exact Schur complement (schur_precondition full) runs on one rank only; "
                 "this communicator has %d", c->comm->size());
        if (c->inner_sweeps > 0)
            fail(SPK_ERR_UNSUPPORTED, "pc_setup: the exact Schur complement (schur_precondition full) needs a linear A^-1 and "
                 "the FP32 inner sweeps are not one in FP64 -- call spk_pc_set_inner(ctx, 0, omega), or keep "
                 "-pc_fieldsplit_schur_precondition selfp");
    }
    std::unique_ptr<spk_amg_hier> amg;
    std::unique_ptr<AmgDev> amg_dev;   // -spk_gamg_setup device: built on the device, equally before anything changes
    // reuse on and nothing but A00's values changed: the hierarchy the context holds is refreshed where it lies.  A refresh
    // that throws leaves it half-done: dropped, and the context without a preconditioner until the next spk_pc_setup
    bool refreshed = false;
    double amg_seconds = 0.0;
    const auto amg_t0 = std::chrono::steady_clock::now();
    auto amg_lap = [&](std::chrono::steady_clock::time_point t) { amg_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); };
    if (c->amg_on) {
        if (c->comm->size() > 1)
            fail(SPK_ERR_UNSUPPORTED, "pc_setup: the multigrid preconditioner (gamg) runs on one rank only; this communicator "
                 "has %d -- multi-rank AMG is not implemented", c->comm->size());
        if (pc_type == SPK_PC_NONE) fail(SPK_ERR_ARG, "pc_setup: the multigrid preconditioner needs pc_type jacobi or schur");
        refreshed = amg_can_refresh(c);
        if (refreshed) {
            try {
                amg_refresh_ctx(c);
            } catch (...) {
                c->amg_d.reset();
                c->amg_h.reset();
                c->pc_ready = false;
                throw;
            }
        } else if (c->amg_opts.setup == SPK_AMG_SETUP_DEVICE) {
            amg_dev = amg_build_device(c);
        } else {
            amg = amg_build_ctx(c);
        }
        amg_lap(amg_t0);
    }
    if (!refreshed) {
        c->amg_d.reset();
        c->amg_h.reset();
    }
    hipStream_t s = c->stream;
    c->ensure_scratch();
    c->ensure_vectors();
    // which iteration path the solve takes: every rank's slab even (bit 0) and non-empty (bit 1)
    const int32_t slabs = and_over_ranks(c, (c->n_local % 2 == 0 ? 1 : 0) | (c->n_local > 0 ? 2 : 0));
    c->even_all = (slabs & 1) != 0;
    c->nonempty_all = (slabs & 2) != 0;
    c->dinv.alloc((size_t)c->n_local, 8);
    k::extract_diag_inv(c->Ad, c->dinv.p, s);
    if (amg) {
        const auto t = std::chrono::steady_clock::now();
        amg_upload(c, std::move(amg));
        amg_lap(t);
    }
    if (amg_dev) c->amg_d = std::move(amg_dev);
    c->amg_refreshed = refreshed;
    c->amg_reuse_seconds = amg_seconds;
    if (c->m > 0) schur_diag(c);
    fp32_copies(c);
    bd_planes(c, pc_type, schur_fact);
    c->schur_dense = false;
    c->pc_ready = false;
    if (dense) {
        try {
            schur_dense_build(c);
        } catch (...) {   // a set-up without a preconditioner: released, the context takes the next spk_pc_setup
            c->sw.release(); c->sfac.release(); c->bd.release();
            c->schur_S.clear();
            throw;
        }
        c->schur_dense = true;
    } else {
        c->sw.release(); c->sfac.release();
        c->schur_S.clear();
        c->schur_setup_seconds = 0.0;
    }
    SPK_HIP(hipStreamSynchronize(s));
    c->pc_type = pc_type;
    c->schur_fact = schur_fact;
    // does EVERY rank's slab fit the resident cycle kernel (restart <= 30)?
    const int planes = !c->bd.p ? 0 : (c->bd_packed ? c->m / 2 : c->m);
    c->res_fit_all = and_over_ranks(c, (c->spmv_format == 1 && c->Adict.ok && c->Adict.bs == 2 && c->n_local % 2 == 0 &&
                                        k::resident_fits(c->Adict, c->num_cus, 30, planes)) ? 1 : 0) != 0;
    c->pc_ready = true;
}

}  // namespace spk
