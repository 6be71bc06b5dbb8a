// spk_host.cpp -- host-only steps of KSPSetOperators: the job MatMPIAIJ does inside PETSc when the reference creates
// its DMDA on PETSC_COMM_WORLD (/root/reference/src/Discretization.c:17, SaddlePointProblem.c:42) -- local rows, a
// "diagonal" block with local column numbers, an "off-diagonal" block whose columns are renumbered into a sorted ghost
// list (garray), the VecScatter plan -- and the integer arithmetic of the dictionary and of the constraint block.
// No HIP call and no ROCm header in this file: it is exercised by the CPU-only tests.
#include "spk_host.hpp"

#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstring>
#include <numeric>
#include <thread>

namespace spk {

void fail(int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    throw Error{code, std::string(buf)};
}

static thread_local std::string g_create_error;
void set_create_error(const std::string &m) { g_create_error = m; }
const char *create_error() { return g_create_error.c_str(); }

void parallel_for(int64_t n, const std::function<void(int64_t, int64_t, int)> &fn, int max_threads)
{
    int nt = max_threads > 0 ? max_threads : (int)std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if (nt > 32) nt = 32;  // setup work is memory bound; stay well inside the host's limits
    if ((int64_t)nt > n / 4096 + 1) nt = (int)(n / 4096 + 1);
    if (nt <= 1) {
        fn(0, n, 0);
        return;
    }
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t) pool.emplace_back([&, t] { fn(n * t / nt, n * (t + 1) / nt, t); });
    fn(0, n / nt, 0);
    for (auto &th : pool) th.join();
}

// Two threaded passes over the rows: count (and collect the off-range columns), then fill.
void split_csr(int64_t row_begin, int32_t nrows_local, const int32_t *rowptr, const int32_t *colidx,
               const double *val, SplitCsr &out, int64_t ncols_global)
{
    const int64_t lo = row_begin, hi = row_begin + nrows_local;
    out.d_rowptr.alloc((size_t)nrows_local + 1);
    out.o_rowptr.alloc((size_t)nrows_local + 1);
    out.bad_column = false;
    std::vector<std::vector<int32_t>> ghost_parts(64);
    std::vector<int> bad(64, 0);
    std::vector<int32_t> badv(64, 0);
    parallel_for(nrows_local, [&](int64_t r0, int64_t r1, int t) {
        auto &gp = ghost_parts[(size_t)t];
        for (int64_t r = r0; r < r1; ++r) {
            int32_t nd = 0, no = 0;
            for (int32_t k = rowptr[r]; k < rowptr[r + 1]; ++k) {
                const int32_t c = colidx[k];
                if (c >= lo && c < hi) ++nd;
                else {
                    ++no;
                    if (ncols_global >= 0 && (c < 0 || c >= ncols_global)) { bad[(size_t)t] = 1; badv[(size_t)t] = c; }
                    if (gp.empty() || gp.back() != c) gp.push_back(c);
                }
            }
            out.d_rowptr[(size_t)r + 1] = nd;
            out.o_rowptr[(size_t)r + 1] = no;
        }
    });
    for (size_t t = 0; t < bad.size(); ++t)
        if (bad[t]) { out.bad_column = true; out.bad_value = badv[t]; }
    std::vector<int32_t> &ghosts = out.garray;
    ghosts.clear();
    for (auto &gp : ghost_parts) ghosts.insert(ghosts.end(), gp.begin(), gp.end());
    ghost_list(ghosts);
    out.d_rowptr[0] = 0;
    out.o_rowptr[0] = 0;
    for (int32_t r = 0; r < nrows_local; ++r) {
        out.d_rowptr[(size_t)r + 1] += out.d_rowptr[(size_t)r];
        out.o_rowptr[(size_t)r + 1] += out.o_rowptr[(size_t)r];
    }
    const size_t nd = (size_t)out.d_rowptr[(size_t)nrows_local], no = (size_t)out.o_rowptr[(size_t)nrows_local];
    out.d_colidx.alloc(nd);
    out.d_val.alloc(nd);
    out.o_colidx.alloc(no);
    out.o_val.alloc(no);
    if (out.bad_column) return;
    parallel_for(nrows_local, [&](int64_t r0, int64_t r1, int) {
        for (int64_t r = r0; r < r1; ++r) {
            int32_t kd = out.d_rowptr[(size_t)r], ko = out.o_rowptr[(size_t)r];
            for (int32_t k = rowptr[r]; k < rowptr[r + 1]; ++k) {
                const int32_t c = colidx[k];
                if (c >= lo && c < hi) {
                    out.d_colidx[(size_t)kd] = (int32_t)(c - lo);
                    out.d_val[(size_t)kd++] = val[k];
                } else {
                    out.o_colidx[(size_t)ko] = ghost_number(ghosts, c);
                    out.o_val[(size_t)ko++] = val[k];
                }
            }
        }
    });
}

// ---------------------------------------------------------------------------
// row types + deviation codes
// ---------------------------------------------------------------------------
void dict_number_classes(const unsigned long long *keys, const int32_t *rep, int nslots, int32_t *slot2id, std::vector<int32_t> &reps)
{
    std::vector<std::pair<int32_t, int32_t>> used;   // (first member, slot)
    for (int i = 0; i < nslots; ++i)
        if (keys[i]) used.push_back({rep[i], i});
    std::sort(used.begin(), used.end());
    std::fill(slot2id, slot2id + nslots, -1);
    reps.clear();
    for (size_t i = 0; i < used.size(); ++i) {
        slot2id[used[i].second] = (int32_t)i;
        reps.push_back(used[i].first);
    }
}

DictRefusal dict_field_widths(int count, const int32_t *gexp, const unsigned long long *dmax, int *width, double *scale)
{
    for (int i = 0; i < count; ++i) {
        width[i] = 1;
        scale[i] = 1.0;
        if (gexp[i] >= 0x7f000000) continue;   // nobody deviates from the base
        // some member deviates: granule = the finest bit in use
        if (gexp[i] < -1000 || gexp[i] > 1000) return {"deviation granule out of range", i, gexp[i]};
        scale[i] = std::ldexp(1.0, gexp[i]);
        double mag;
        std::memcpy(&mag, &dmax[i], sizeof mag);
        const double kabs = mag / scale[i];
        if (!(kabs <= 1.0e9)) return {"a class entry scatters beyond 31-bit codes", i, (long)gexp[i]};
        width[i] = 2;
        while ((double)((1ll << (width[i] - 1)) - 1) < kabs) ++width[i];
    }
    return {};
}

// Bit fields: entry (class, e) gets the width its largest deviation needs, the fields of a block are packed into one
// 64-bit word (2x2 blocks) or two (3x3: a field never straddles the words).
DictRefusal dict_field_layout(int bs, int ncls, const int *width, const double *scale, bool allow_uniform, int32_t *fld, double *cls,
                              DictLayout &L)
{
    const int bb = bs * bs;
    L = DictLayout{};
    std::fill(fld, fld + (size_t)(ncls + 1) * bb, 1 << 8);   // (null class: one bit at offset 0)
    int uw[9];   // the widest need per entry
    for (int e = 0; e < bb; ++e) {
        uw[e] = 1;
        for (int cl = 0; cl < ncls; ++cl) uw[e] = std::max(uw[e], width[(size_t)cl * bb + e]);
    }
    // 2x2: one layout for all classes where the widest need per entry allows it (1024^2: 19 + 13 | 13 + 19 bits)
    if (bs == 2 && allow_uniform && uw[0] + uw[1] <= 32 && uw[2] + uw[3] <= 32) {
        L.uniform = true;
        for (int e = 0; e < 4; ++e) L.uw[e] = uw[e];
        const uint32_t f[4] = {0u | ((uint32_t)uw[0] << 8), (uint32_t)(32 - uw[1]) | ((uint32_t)uw[1] << 8),
                               0x80000000u | ((uint32_t)uw[2] << 8), 0x80000000u | (uint32_t)(32 - uw[3]) | ((uint32_t)uw[3] << 8)};
        for (int cl = 0; cl <= ncls; ++cl)   // (the null class too: any field of a zero word decodes to 0)
            for (int e = 0; e < 4; ++e) fld[(size_t)cl * 4 + e] = (int32_t)f[e];
    }
    // 3x3: the same idea over the two words of a block; the entries of the second word are one of three fixed sets
    for (int split = 1; bs == 3 && allow_uniform && split <= 3 && !L.uniform3; ++split) {
        auto in_w1 = [&](int e) { return split == 1 ? e >= 5 : split == 2 ? e >= 4 : (e == 4 || e >= 6); };
        int used[2] = {0, 0};
        for (int e = 0; e < 9; ++e) used[in_w1(e) ? 1 : 0] += uw[e];
        if (used[0] > 64 || used[1] > 64) continue;
        L.uniform3 = split;
        int sh[2] = {0, 0};
        for (int e = 0; e < 9; ++e) {
            const int wd = in_w1(e) ? 1 : 0;
            for (int cl = 0; cl <= ncls; ++cl) fld[(size_t)cl * 9 + e] = sh[wd] | (uw[e] << 8) | (wd << 16);
            L.u3l[e] = 64 - sh[wd] - uw[e];
            L.u3r[e] = 32 - uw[e];
            sh[wd] += uw[e];
        }
    }
    for (int cl = 0; cl < ncls; ++cl) {
        int used[2] = {0, 0}, word = 0;
        const int *w = &width[(size_t)cl * bb];
        if (bs == 2 && !L.uniform && !(w[0] + w[1] <= 32 && w[2] + w[3] <= 32) && w[0] + w[1] + w[2] + w[3] <= 64) {
            // no packing of this class's fields inside the halves, but 64 bits suffice: back to back, a field across
            // the halves flagged (the plain kernels extract it with 64-bit shifts)
            int sh = 0;
            for (int e = 0; e < 4; ++e) {
                const int i = cl * 4 + e;
                const bool across = sh < 32 && sh + w[e] > 32;
                fld[i] = across ? (int32_t)((uint32_t)sh | ((uint32_t)w[e] << 8) | (uint32_t)k::kDictAcrossHost)
                                : (int32_t)((uint32_t)(sh & 31) | ((uint32_t)w[e] << 8) | (sh >= 32 ? 0x80000000u : 0u));
                L.straddle = L.straddle || across;
                sh += w[e];
                cls[(size_t)2 * i + 1] = scale[i];
            }
            continue;
        }
        for (int e = 0; e < bb; ++e) {
            const int i = cl * bb + e;
            if (!L.uniform && !L.uniform3) {
                // 2x2: two 32-bit halves of one word, a field inside one half (hardware bit-field extract); 3x3: two 64-bit words
                const int cap = bs == 2 ? 32 : 64;
                if (used[word] + w[e] > cap) ++word;
                if (word > 1) return {"the codes of a block class do not fit its word(s)", cl, used[0] + used[1] + w[e]};
                fld[i] = bs == 2 ? (int32_t)((uint32_t)used[word] | ((uint32_t)w[e] << 8) | (word ? 0x80000000u : 0u))
                                 : (used[word] | (w[e] << 8) | (word << 16));
                used[word] += w[e];
            }
            cls[(size_t)2 * i + 1] = scale[i];
        }
    }
    return {};
}

// Code planes (DictArgs::plane_off): 2x2 blocks -- positions 2p, 2p+1 side by side in plane p; 3x3 -- plane k.
// (the planes are read side by side, row r of each at the same time: a skew per plane keeps planes whose size is a
// power of two -- 16 MiB each at 1024^2 -- from landing on one memory channel together)
int64_t dict_plane_offsets(int bs, int kmax, int32_t nbrows, int64_t skew, int64_t plane_off[kDictMaxK])
{
    const int64_t nbr_pad = ((int64_t)nbrows + 15) & ~(int64_t)15;
    int64_t off = 0;
    for (int kk = 0; kk < kDictMaxK; ++kk) {
        off += kk ? skew : 0;
        plane_off[kk] = off;
        if (bs == 2) {
            if (2 * kk + 1 < kmax) off += 16 * nbr_pad;
            else if (2 * kk < kmax) off += 8 * nbr_pad;
        } else if (kk < kmax) {
            off += 16 * nbr_pad;
        }
    }
    return off;
}

int dict_tab_ints(int ntype, int kmax) { return ((ntype + 1) & ~1) + 2 * ntype * kmax; }

int dict_lds_bytes(int ntype, int kmax, int ncls, int bs)
{
    const int bb = bs * bs;
    return ((((4 * dict_tab_ints(ntype, kmax) + 15) & ~15) + 16 * (ncls + 1) * bb + 4 * (ncls + 1) * bb) + 15) & ~15;
}

// ---------------------------------------------------------------------------
// A00: ghosts and the halo plan (VecScatter of MatMult_MPIAIJ)
// ---------------------------------------------------------------------------
void ghost_list(std::vector<int32_t> &cols)
{
    std::sort(cols.begin(), cols.end());
    cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
}

void ghost_renumber(const std::vector<int32_t> &garray, int32_t *cols, size_t n)
{
    for (size_t i = 0; i < n; ++i) cols[i] = ghost_number(garray, cols[i]);
}

void compress_offrank_rows(const int32_t *orp, int32_t n, std::vector<int32_t> &rows, std::vector<int32_t> &corp)
{
    rows.clear();
    corp.assign(1, 0);
    for (int32_t r = 0; orp && r < n; ++r)
        if (orp[r + 1] > orp[r]) {
            rows.push_back(r);
            corp.push_back(orp[r + 1]);
        }
}

void halo_plan(int me, int P, const int64_t *slabs, const std::vector<int32_t> &garray, const std::vector<std::vector<char>> &ghosts,
               HaloPlan &out)
{
    out = HaloPlan{};
    for (int r = 1; r < P; ++r)
        if (slabs[2 * r] != slabs[2 * r - 1]) fail(SPK_ERR_ARG, "A00: row slabs must tile [0,n) in rank order");
    const int64_t lo = slabs[2 * me], hi = slabs[2 * me + 1];
    for (int p = 0; p < P; ++p) {
        if (p == me) continue;
        // what I receive from p: my ghosts inside p's range (contiguous in sorted garray)
        const int64_t plo = slabs[2 * p], phi = slabs[2 * p + 1];
        int64_t nrecv = 0;
        for (int32_t g : garray) nrecv += (g >= plo && g < phi);
        // what I send to p: p's ghosts inside my range, in p's order
        const int32_t *pg = (const int32_t *)ghosts[(size_t)p].data();
        const size_t npg = ghosts[(size_t)p].size() / sizeof(int32_t);
        int64_t nsend = 0;
        for (size_t i = 0; i < npg; ++i)
            if (pg[i] >= lo && pg[i] < hi) {
                out.send_idx.push_back((int32_t)(pg[i] - lo));
                ++nsend;
            }
        if (nsend == 0 && nrecv == 0) continue;
        out.peers.push_back(p);
        out.send_off.push_back(out.send_off.back() + nsend);
        out.recv_off.push_back(out.recv_off.back() + nrecv);
    }
    if (P > 1 && out.recv_off.back() != (int64_t)garray.size()) fail(SPK_ERR_ARG, "A00: ghost columns not owned by any rank");
}

// halo rows as contiguous ranges (slab partitions): lets the producer of z fill the send buffer itself
HostSendRanges send_ranges(const HaloPlan &h)
{
    HostSendRanges R;
    bool ok = !h.peers.empty() && h.peers.size() <= 4;
    for (size_t p = 0; ok && p < h.peers.size(); ++p) {
        const int64_t a = h.send_off[p], b = h.send_off[p + 1];
        for (int64_t i = a + 1; ok && i < b; ++i) ok = h.send_idx[(size_t)i] == h.send_idx[(size_t)i - 1] + 1;
        R.r0[p] = b > a ? h.send_idx[(size_t)a] : 0;
        R.len[p] = (int32_t)(b - a);
        R.off[p] = (int32_t)a;
    }
    if (!ok) return HostSendRanges{};
    R.n = (int)h.peers.size();
    return R;
}

// ---------------------------------------------------------------------------
// A10: the constraint block
// ---------------------------------------------------------------------------
// (threaded over the entries: the reference's 4 rows hold ~n/2 entries each -- 4 M at 1024^2)
void localise_and_sort(int32_t m, const int32_t *rowptr, const int32_t *colidx, const double *val, int64_t lo, int64_t hi,
                       int32_t *col, double *v)
{
    // a flag of its own per thread: any int32 -- -1 included -- can be the offending column number
    std::vector<char> bad(64, 0);
    std::vector<int32_t> badcol(64, 0);
    parallel_for(rowptr[m], [&](int64_t a, int64_t b, int t) {
        for (int64_t k = a; k < b; ++k) {
            const int32_t g = colidx[k];
            if (g < lo || g >= hi) bad[(size_t)t] = 1, badcol[(size_t)t] = g;
            col[k] = (int32_t)(g - lo);
            v[k] = val[k];
        }
    });
    for (size_t t = 0; t < bad.size(); ++t)
        if (bad[t]) fail(SPK_ERR_ARG, "A10: column %d not owned by this rank [%lld,%lld)", badcol[t], (long long)lo, (long long)hi);
    for (int32_t r = 0; r < m; ++r) {   // PETSc rows come sorted: nothing to do then
        const int32_t k0 = rowptr[r], n = rowptr[r + 1] - k0;
        if (std::is_sorted(col + k0, col + k0 + n)) continue;
        std::vector<int32_t> perm((size_t)n), c2((size_t)n);
        std::vector<double> v2((size_t)n);
        std::iota(perm.begin(), perm.end(), 0);
        std::stable_sort(perm.begin(), perm.end(), [&](int32_t a, int32_t b) { return col[k0 + a] < col[k0 + b]; });
        for (int32_t i = 0; i < n; ++i) {
            c2[(size_t)i] = col[k0 + perm[(size_t)i]];
            v2[(size_t)i] = v[k0 + perm[(size_t)i]];
        }
        std::copy(c2.begin(), c2.end(), col + k0);
        std::copy(v2.begin(), v2.end(), v + k0);
    }
}

// Which rows go through the column-window (long-row) kernel: all of them for m <= 8 (the reference's 4 rows, the fused
// dense-plane path); for a general block only its LONG rows (local entries beyond the threshold; at most 8, the longest
// first, ties to the lower row) -- the rest is a CSR by rows for the stream kernel.  Ascending.
std::vector<int32_t> wide_rows(int32_t m, const int32_t *rowptr, int32_t threshold)
{
    std::vector<int32_t> cand;
    for (int32_t r = 0; r < m; ++r)
        if (m <= 8 || rowptr[r + 1] - rowptr[r] > threshold) cand.push_back(r);
    if (m <= 8) return cand;
    std::sort(cand.begin(), cand.end(), [&](int32_t a, int32_t b) {
        const int32_t la = rowptr[a + 1] - rowptr[a], lb = rowptr[b + 1] - rowptr[b];
        return la != lb ? la > lb : a < b;
    });
    if (cand.size() > 8) cand.resize(8);
    std::sort(cand.begin(), cand.end());
    return cand;
}

int32_t window_width(int32_t nl, int max_blocks)
{
    int32_t win = 8192;
    while (((int64_t)nl + win - 1) / win > max_blocks) win *= 2;
    // small local sizes: narrower windows, so that the launch still has ~128 workgroups (a rank's 1/8 slab of the
    // 1024^2 grid got 32 workgroups on 256 CUs: 12.6 us for 6 MB)
    while (win > 1024 && ((int64_t)nl + win - 1) / win < 128) win /= 2;
    return win;
}

void window_pointers(int32_t mw, const int32_t *wrp, const int32_t *wcol, int32_t nl, int32_t win, int32_t nwin, int32_t *winptr)
{
    for (int32_t r = 0; r < mw; ++r) {
        const int32_t *b = wcol + wrp[r], *e = wcol + wrp[r + 1];
        for (int32_t w = 0; w <= nwin; ++w) {
            const int64_t c0 = (int64_t)w * win;
            winptr[(size_t)w * mw + r] = wrp[r] + (int32_t)(std::lower_bound(b, e, (int32_t)std::min<int64_t>(c0, nl)) - b);
        }
    }
}

void gather_rows(int32_t m, const int32_t *rowptr, const int32_t *col, const double *v, const std::vector<int32_t> &rows, bool complement,
                 std::vector<int32_t> &rp, std::vector<int32_t> &ci, std::vector<double> &cv)
{
    std::vector<char> listed((size_t)m, 0);
    for (int32_t r : rows) listed[(size_t)r] = 1;
    rp.assign(1, 0);
    ci.clear();
    cv.clear();
    for (int32_t r = 0; r < m; ++r) {
        const bool take = (listed[(size_t)r] != 0) != complement;
        if (take) {
            ci.insert(ci.end(), col + rowptr[r], col + rowptr[r + 1]);
            cv.insert(cv.end(), v + rowptr[r], v + rowptr[r + 1]);
        }
        if (take || complement) rp.push_back((int32_t)ci.size());
    }
}

// Threads own disjoint column ranges and walk the sorted rows' entries inside them: counts, then fill in row order --
// the same arrays as a sequential counting sort.
void transpose_rows(int32_t m, int32_t nl, const int32_t *rowptr, const int32_t *col, const double *v, int32_t *trp, int32_t *tci,
                    double *tv, int max_threads)
{
    auto row_range = [&](int32_t r, int64_t c0, int64_t c1, int32_t &b, int32_t &e) {
        const int32_t *rb = col + rowptr[r], *re = col + rowptr[r + 1];
        b = rowptr[r] + (int32_t)(std::lower_bound(rb, re, (int32_t)c0) - rb);
        e = rowptr[r] + (int32_t)(std::lower_bound(rb, re, (int32_t)c1) - rb);
    };
    parallel_for(nl, [&](int64_t c0, int64_t c1, int) {
        for (int32_t r = 0; r < m; ++r) {
            int32_t b, e;
            row_range(r, c0, c1, b, e);
            for (int32_t k = b; k < e; ++k) trp[(size_t)col[k] + 1]++;
        }
    }, max_threads);
    for (int32_t i = 0; i < nl; ++i) trp[(size_t)i + 1] += trp[i];
    HostBuf<int32_t> fill;
    fill.alloc((size_t)nl + 1);
    parallel_for(nl, [&](int64_t c0, int64_t c1, int) {
        for (int64_t i = c0; i < c1; ++i) fill[(size_t)i] = trp[i];
        for (int32_t r = 0; r < m; ++r) {
            int32_t b, e;
            row_range(r, c0, c1, b, e);
            for (int32_t k = b; k < e; ++k) {
                const int32_t p = fill[(size_t)col[k]]++;
                tci[p] = r;
                tv[p] = v[k];
            }
        }
    }, max_threads);
}

// ---------------------------------------------------------------------------
// the multigrid cycle: its steps in order, and which of them the fused tail takes
// ---------------------------------------------------------------------------
static void cycle_steps(std::vector<AmgStep> &out, int l, int L, bool w, bool fresh)
{
    if (l == L - 1) { out.push_back({SPK_AMG_STEP_COARSE, l}); return; }
    out.push_back({fresh ? SPK_AMG_STEP_PRE0 : SPK_AMG_STEP_PRE, l});
    out.push_back({SPK_AMG_STEP_DOWN, l});
    cycle_steps(out, l + 1, L, w, true);
    if (w && l + 1 < L - 1) cycle_steps(out, l + 1, L, w, false);
    out.push_back({SPK_AMG_STEP_UP, l});
    out.push_back({SPK_AMG_STEP_POST, l});
}

std::vector<AmgStep> amg_cycle_steps(int levels, int cycle)
{
    if (levels < 1 || levels > SPK_AMG_MAX_LEVELS) fail(SPK_ERR_ARG, "amg: %d levels outside [1,%d]", levels, SPK_AMG_MAX_LEVELS);
    if (cycle != SPK_AMG_CYCLE_V && cycle != SPK_AMG_CYCLE_W)
        fail(SPK_ERR_ARG, "amg: cycle %d is neither SPK_AMG_CYCLE_V (0) nor SPK_AMG_CYCLE_W (1)", cycle);
    std::vector<AmgStep> out;
    cycle_steps(out, 0, levels, cycle == SPK_AMG_CYCLE_W, true);
    return out;
}

int amg_resolve_tail(int cycle, int tail)
{
    if (tail != SPK_AMG_TAIL_AUTO) return tail;
    return cycle == SPK_AMG_CYCLE_W ? SPK_AMG_TAIL_FUSED : SPK_AMG_TAIL_LAUNCHES;
}

int amg_tail_first(int levels, const int32_t *rows, int cycle, int tail, int tail_rows)
{
    if (levels < 2 || amg_resolve_tail(cycle, tail) != SPK_AMG_TAIL_FUSED) return -1;
    const int32_t limit = tail_rows > 0 ? tail_rows : SPK_AMG_TAIL_ROWS_DEFAULT;
    int t = levels;
    while (t > 1 && rows[t - 1] <= limit) --t;
    return t < levels ? t : -1;
}

std::vector<std::pair<int64_t, int64_t>> amg_tail_runs(const std::vector<AmgStep> &steps, int tail_first)
{
    std::vector<std::pair<int64_t, int64_t>> runs;
    if (tail_first < 1) return runs;
    for (int64_t s = 0, n = (int64_t)steps.size(); s < n;) {
        if (steps[(size_t)s].level < tail_first) { ++s; continue; }
        int64_t e = s;
        while (e < n && steps[(size_t)e].level >= tail_first) ++e;
        runs.push_back({s, e});
        s = e;
    }
    return runs;
}

AmgBuffers amg_cycle_buffers(const std::vector<AmgStep> &steps, const std::vector<std::pair<int64_t, int64_t>> &runs, int levels,
                             int nu, int tail_first)
{
    AmgBuffers b;
    b.sel.resize(steps.size());
    b.sel_next.resize(steps.size());
    b.run_sel.assign(runs.size(), 0);
    int32_t sel[SPK_AMG_MAX_LEVELS] = {};
    size_t run = 0;
    for (size_t i = 0; i < steps.size(); ++i) {
        const AmgStep st = steps[i];
        b.sel[i] = sel[st.level];
        b.sel_next[i] = st.level + 1 < levels ? sel[st.level + 1] : 0;
        if (st.kind == SPK_AMG_STEP_PRE0) sel[st.level] = (nu & 1) ? 0 : 1;
        else if (st.kind == SPK_AMG_STEP_PRE || st.kind == SPK_AMG_STEP_POST) sel[st.level] ^= nu & 1;
        else if (st.kind == SPK_AMG_STEP_COARSE) sel[st.level] = 0;
        if (run < runs.size() && (size_t)runs[run].second == i + 1) b.run_sel[run++] = sel[tail_first];   // (a run: tail_first >= 1)
    }
    return b;
}

// (G + G^T) / 2 into S, its Cholesky factor (lower, row-major, zeros above) into L.  A pivot at or below the rounding of
// its own subtraction (64 eps S_jj) counts as zero: the rows of B are then linearly dependent to working precision.
int schur_dense_factor(int m, const double *G, double *S, double *L)
{
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) S[(size_t)i * m + j] = 0.5 * (G[(size_t)i * m + j] + G[(size_t)j * m + i]);
    std::fill(L, L + (size_t)m * m, 0.0);
    for (int j = 0; j < m; ++j) {
        double d = S[(size_t)j * m + j];
        for (int k = 0; k < j; ++k) d -= L[(size_t)j * m + k] * L[(size_t)j * m + k];
        if (!(d > 64.0 * DBL_EPSILON * S[(size_t)j * m + j])) return j;
        d = std::sqrt(d);
        L[(size_t)j * m + j] = d;
        for (int i = j + 1; i < m; ++i) {
            double s = S[(size_t)i * m + j];
            for (int k = 0; k < j; ++k) s -= L[(size_t)i * m + k] * L[(size_t)j * m + k];
            L[(size_t)i * m + j] = s / d;
        }
    }
    return -1;
}

}  // namespace spk
