// setup_host_check.cpp -- self-checking program over the host-pure set-up steps of csrc/spk_host.cpp.
// Every case compares against a brute-force reference written here; a failed check prints the case and its line and the
// program exits with status 1.  Built by tests/test_setup_host_cpu.py with the address and undefined-behaviour sanitizers.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <numeric>
#include <set>

#include "spk_host.hpp"

using namespace spk;

static const char *g_case = "";
static int g_failed = 0;
#define CASE(name) g_case = name
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            std::printf("FAILED %s: %s (line %d)\n", g_case, #cond, __LINE__);            \
            ++g_failed;                                                                    \
        }                                                                                  \
    } while (0)

typedef std::vector<int32_t> ivec;

// ---- field layout ----
struct Field { int word, lo, width; bool across; };   // bit range [lo, lo + width) of the block's word `word`
static Field decode2(int32_t f)
{
    const uint32_t u = (uint32_t)f;
    const int width = (u >> 8) & 255;
    if (u & (uint32_t)k::kDictAcrossHost) return {0, (int)(u & 63), width, true};
    return {0, (int)(u & 31) + ((u & 0x80000000u) ? 32 : 0), width, false};
}
static Field decode3(int32_t f) { return {(f >> 16) & 1, f & 255, (f >> 8) & 255, false}; }

struct LayoutOut { DictRefusal r; DictLayout L; ivec fld; std::vector<double> cls; };
static LayoutOut layout(int bs, const std::vector<int> &w, bool allow_uniform = true)
{
    const int bb = bs * bs, ncls = (int)w.size() / bb;
    LayoutOut o;
    std::vector<double> scale(w.size());
    for (size_t i = 0; i < w.size(); ++i) scale[i] = std::ldexp(1.0, -(int)i - 3);
    o.fld.assign((size_t)(ncls + 1) * bb, -12345);
    o.cls.assign((size_t)(ncls + 1) * bb * 2, 7.0);
    o.r = dict_field_layout(bs, ncls, w.data(), scale.data(), allow_uniform, o.fld.data(), o.cls.data(), o.L);
    if (o.r.why) return o;
    // invariants of every accepted layout
    for (int cl = 0; cl < ncls; ++cl) {
        unsigned long long used[2] = {0, 0};
        for (int e = 0; e < bb; ++e) {
            const int i = cl * bb + e;
            const Field f = bs == 2 ? decode2(o.fld[i]) : decode3(o.fld[i]);
            const int need = (o.L.uniform || o.L.uniform3) ? f.width : w[i];   // (one layout: the widest need per entry)
            CHECK(f.width >= w[i] && f.width == need);
            CHECK(f.lo >= 0 && f.lo + f.width <= 64);
            if (bs == 2 && !f.across) CHECK(f.lo / 32 == (f.lo + f.width - 1) / 32);   // inside its half unless flagged
            if (bs == 2 && f.across) CHECK(f.lo < 32 && f.lo + f.width > 32);
            const unsigned long long mask = (f.width == 64 ? ~0ull : ((1ull << f.width) - 1)) << f.lo;
            CHECK((used[f.word] & mask) == 0);   // the fields of one block do not overlap
            used[f.word] |= mask;
            CHECK(o.cls[(size_t)2 * i + 1] == scale[i]);   // the scale sits at cls[2 i + 1] ...
            CHECK(o.cls[(size_t)2 * i] == 7.0);            // ... and the base half is not touched
        }
    }
    for (int e = 0; e < bb * 2; ++e) CHECK(o.cls[(size_t)ncls * bb * 2 + e] == 7.0);   // the null class: the caller's
    return o;
}

static void test_field_layout_2()
{
    CASE("field layout bs=2 uniform 19 13 13 19");
    {
        LayoutOut o = layout(2, {19, 13, 13, 19, 19, 13, 13, 19});
        CHECK(!o.r.why && o.L.uniform && !o.L.straddle);
        const uint32_t f[4] = {0u | (19u << 8), 19u | (13u << 8), 0x80000000u | (13u << 8), 0x80000000u | 13u | (19u << 8)};
        for (int cl = 0; cl <= 2; ++cl)   // the null class gets the layout too
            for (int e = 0; e < 4; ++e) CHECK((uint32_t)o.fld[cl * 4 + e] == f[e]);
        const int uw[4] = {19, 13, 13, 19};
        for (int e = 0; e < 4; ++e) CHECK(o.L.uw[e] == uw[e]);
        LayoutOut p = layout(2, {19, 13, 13, 19, 19, 13, 13, 19}, false);   // the switch off: per class, null class one bit
        CHECK(!p.r.why && !p.L.uniform);
        for (int e = 0; e < 4; ++e) CHECK(p.fld[8 + e] == (1 << 8));
        CHECK((uint32_t)p.fld[1] == (19u | (13u << 8)) && (uint32_t)p.fld[3] == (0x80000000u | 13u | (19u << 8)));
    }
    CASE("field layout bs=2 per class");
    {
        // each class fits the halves; the per-entry maximum (20 + 20) does not
        LayoutOut o = layout(2, {20, 12, 12, 20, 12, 20, 20, 12});
        CHECK(!o.r.why && !o.L.uniform && !o.L.straddle);
        CHECK((uint32_t)o.fld[0] == (0u | (20u << 8)) && (uint32_t)o.fld[1] == (20u | (12u << 8)));
        CHECK((uint32_t)o.fld[2] == (0x80000000u | (12u << 8)) && (uint32_t)o.fld[3] == (0x80000000u | 12u | (20u << 8)));
        CHECK((uint32_t)o.fld[4] == (0u | (12u << 8)) && (uint32_t)o.fld[5] == (12u | (20u << 8)));
        for (int e = 0; e < 4; ++e) CHECK(o.fld[8 + e] == (1 << 8));
    }
    CASE("field layout bs=2 across the halves");
    {
        LayoutOut o = layout(2, {20, 20, 12, 12});
        CHECK(!o.r.why && !o.L.uniform && o.L.straddle);
        CHECK((uint32_t)o.fld[0] == (0u | (20u << 8)));
        CHECK((uint32_t)o.fld[1] == (20u | (20u << 8) | (uint32_t)k::kDictAcrossHost));   // entry 1: bits 20..39
        CHECK((uint32_t)o.fld[2] == (0x80000000u | 8u | (12u << 8)));
        CHECK((uint32_t)o.fld[3] == (0x80000000u | 20u | (12u << 8)));
    }
    CASE("field layout bs=2 a field ending on the boundary");
    {
        LayoutOut o = layout(2, {10, 10, 12, 25});   // 12 + 25 beyond a half: back to back, entry 2 ends at bit 32 -- not across
        CHECK(!o.r.why && !o.L.uniform && !o.L.straddle);
        CHECK((uint32_t)o.fld[2] == (20u | (12u << 8)) && (uint32_t)o.fld[3] == (0x80000000u | 0u | (25u << 8)));
    }
    CASE("field layout bs=2 refusal");
    {
        LayoutOut o = layout(2, {2, 2, 2, 2, 30, 30, 3, 3});   // class 1: 66 bits
        CHECK(o.r.why && !std::strcmp(o.r.why, "the codes of a block class do not fit its word(s)"));
        CHECK(o.r.a == 1 && o.r.b == 63);   // (class, bits asked for when a third half would open: 30 | 30 + 3)
    }
}

static void test_field_layout_3()
{
    auto formulas = [](const LayoutOut &o, const std::vector<int> &uw, int split) {
        CHECK(o.L.uniform3 == split);
        int sh[2] = {0, 0};
        for (int e = 0; e < 9; ++e) {
            const int wd = split == 1 ? e >= 5 : split == 2 ? e >= 4 : (e == 4 || e >= 6);
            CHECK(o.fld[e] == (sh[wd] | (uw[e] << 8) | (wd << 16)));
            CHECK(o.L.u3l[e] == 64 - sh[wd] - uw[e] && o.L.u3r[e] == 32 - uw[e]);
            sh[wd] += uw[e];
        }
    };
    CASE("field layout bs=3 split 1");
    { std::vector<int> w = {12, 12, 12, 12, 12, 16, 16, 16, 16}; LayoutOut o = layout(3, w); CHECK(!o.r.why); formulas(o, w, 1); }
    CASE("field layout bs=3 split 2");
    { std::vector<int> w = {16, 16, 16, 16, 12, 12, 12, 12, 12}; LayoutOut o = layout(3, w); CHECK(!o.r.why); formulas(o, w, 2); }
    CASE("field layout bs=3 split 3");   // entries 0-3 and 5 in the first word: 4 x 14 + 8 = 64; split 1 and 2 overflow a word
    { std::vector<int> w = {14, 14, 14, 14, 20, 8, 14, 14, 14}; LayoutOut o = layout(3, w); CHECK(!o.r.why); formulas(o, w, 3); }
    CASE("field layout bs=3 per class, two words");
    {
        // the maxima (15 everywhere: 135 bits, five entries of some word beyond 64) fit no split; each class alone fits
        // two words in order
        std::vector<int> w = {15, 15, 15, 15, 15, 1, 1, 1, 1, 1, 1, 1, 1, 15, 15, 15, 15, 15};
        LayoutOut o = layout(3, w);
        CHECK(!o.r.why && o.L.uniform3 == 0);
        CHECK(o.fld[0] == (0 | (15 << 8)) && o.fld[3] == (45 | (15 << 8)) && o.fld[4] == (0 | (15 << 8) | (1 << 16)) &&
              o.fld[5] == (15 | (1 << 8) | (1 << 16)) && o.fld[8] == (18 | (1 << 8) | (1 << 16)));
        CHECK(o.fld[9] == (0 | (1 << 8)) && o.fld[9 + 4] == (4 | (15 << 8)) && o.fld[9 + 7] == (49 | (15 << 8)) &&
              o.fld[9 + 8] == (0 | (15 << 8) | (1 << 16)));
        for (int e = 0; e < 9; ++e) CHECK(o.fld[18 + e] == (1 << 8));
    }
    CASE("field layout bs=3 refusal");
    {
        std::vector<int> w(9, 15);   // 135 bits
        LayoutOut o = layout(3, w);
        CHECK(o.r.why && !std::strcmp(o.r.why, "the codes of a block class do not fit its word(s)") && o.r.a == 0 && o.r.b == 135);
    }
}

static void test_field_widths()
{
    CASE("field widths");
    auto bits = [](double d) { unsigned long long u; std::memcpy(&u, &d, sizeof u); return u; };
    for (int w = 2; w <= 30; ++w) {   // (width 31 tops out at 2^30 - 1: beyond the 1e9 the codes may reach)
        const double top = (double)((1ll << (w - 1)) - 1);   // the largest code of width w
        const int32_t g[3] = {0x7f7f7f7f, -46, -46};
        const unsigned long long m[3] = {0, bits(top * std::ldexp(1.0, -46)), bits((top + 1) * std::ldexp(1.0, -46))};
        int width[3];
        double scale[3];
        DictRefusal r = dict_field_widths(3, g, m, width, scale);
        CHECK(!r.why);
        CHECK(width[0] == 1 && scale[0] == 1.0);   // nobody deviates
        CHECK(width[1] == w && width[2] == w + 1);
        CHECK(scale[1] == std::ldexp(1.0, -46) && scale[2] == scale[1]);
    }
    int width[2];
    double scale[2];
    {
        const int32_t g[2] = {0, 1001};
        const unsigned long long m[2] = {bits(1.0), bits(1.0)};
        DictRefusal r = dict_field_widths(2, g, m, width, scale);
        CHECK(r.why && !std::strcmp(r.why, "deviation granule out of range") && r.a == 1 && r.b == 1001);
        const int32_t g2[2] = {-1001, 0};
        r = dict_field_widths(2, g2, m, width, scale);
        CHECK(r.why && r.a == 0 && r.b == -1001);
    }
    {
        const int32_t g[2] = {-3, -3};
        const unsigned long long m[2] = {bits(1.0e9 / 8), bits((1.0e9 + 1) / 8)};
        DictRefusal r = dict_field_widths(2, g, m, width, scale);
        CHECK(r.why && !std::strcmp(r.why, "a class entry scatters beyond 31-bit codes") && r.a == 1 && r.b == -3);
        CHECK(width[0] == 31);
    }
}

static void test_plane_offsets()
{
    CASE("plane offsets");
    int64_t po[kDictMaxK];
    for (int64_t skew : {(int64_t)4352, (int64_t)0}) {
        // bs = 2, 17 block rows (padded to 32), 5 positions: planes 0, 1 hold two positions (16 B a row), plane 2 one (8 B)
        int64_t tot = dict_plane_offsets(2, 5, 17, skew, po);
        int64_t off = 0;
        for (int kk = 0; kk < kDictMaxK; ++kk) {
            off += kk ? skew : 0;
            CHECK(po[kk] == off);
            off += kk < 2 ? 16 * 32 : kk == 2 ? 8 * 32 : 0;
        }
        CHECK(tot == off && tot == 2 * 512 + 256 + 31 * skew);
        CHECK(po[1] == 512 + skew && po[2] == 1024 + 2 * skew && po[3] == 1280 + 3 * skew);
        tot = dict_plane_offsets(3, 27, 17, skew, po);
        for (int kk = 0; kk < kDictMaxK; ++kk) CHECK(po[kk] == (int64_t)std::min(kk, 27) * 512 + kk * skew);
        CHECK(tot == 27 * 512 + 31 * skew);
    }
    CHECK(dict_plane_offsets(2, 4, 16, 0, po) == 2 * 16 * 16);   // an even count: no half plane; 16 rows: no padding
    CASE("lds bytes");
    CHECK(dict_tab_ints(3, 5) == 4 + 30 && dict_tab_ints(4, 5) == 4 + 40);
    CHECK(dict_lds_bytes(3, 5, 2, 2) == 144 + 16 * 12 + 4 * 12);                      // 136 B of table rounded to 144
    CHECK(dict_lds_bytes(1, 1, 1, 3) == ((16 + 16 * 18 + 4 * 18 + 15) & ~15));
}

static void test_class_numbering()
{
    CASE("class numbering");
    const unsigned long long keys[8] = {0, 5, 0, 9, 7, 0, 0, 1};
    const int32_t rep[8] = {0x7f7f7f7f, 40, 0x7f7f7f7f, 3, 17, 0x7f7f7f7f, 0x7f7f7f7f, 0};
    ivec s2i(8, 99), reps = {1, 2, 3};
    dict_number_classes(keys, rep, 8, s2i.data(), reps);
    CHECK((reps == ivec{0, 3, 17, 40}));
    CHECK((s2i == ivec{-1, 3, -1, 1, 2, -1, -1, 0}));
}

// ---- halo plan ----
static std::vector<std::vector<char>> as_bytes(const std::vector<ivec> &g)
{
    std::vector<std::vector<char>> out;
    for (const ivec &v : g) out.emplace_back((const char *)v.data(), (const char *)(v.data() + v.size()));
    return out;
}

static void test_halo_plan()
{
    CASE("halo plan P=3");
    const int64_t slabs[6] = {0, 4, 4, 7, 7, 12};
    // rank 0 needs rows of rank 1 only, rank 2 likewise; the middle rank has ghosts on both sides.  Second round: rank 0
    // also needs row 9 of rank 2, which needs nothing of rank 0 -- peers all the same, one way
    const std::vector<ivec> sym = {{4, 6}, {1, 3, 7, 8, 11}, {5, 6}}, oneway = {{4, 6, 9}, {1, 3, 7, 8, 11}, {5, 6}};
    for (const std::vector<ivec> &g : {sym, oneway}) {
        const auto bytes = as_bytes(g);
        HaloPlan h[3];
        for (int me = 0; me < 3; ++me) {
            halo_plan(me, 3, slabs, g[(size_t)me], bytes, h[me]);
            // brute force: for every other rank, what I receive (my ghosts it owns) and what I send (its ghosts I own, its order)
            std::vector<int> peers;
            std::vector<int64_t> so{0}, ro{0};
            ivec si;
            for (int p = 0; p < 3; ++p) {
                if (p == me) continue;
                int64_t nr = 0, ns = 0;
                for (int32_t c : g[(size_t)me]) nr += c >= slabs[2 * p] && c < slabs[2 * p + 1];
                for (int32_t c : g[(size_t)p])
                    if (c >= slabs[2 * me] && c < slabs[2 * me + 1]) { si.push_back((int32_t)(c - slabs[2 * me])); ++ns; }
                if (!nr && !ns) continue;
                peers.push_back(p); so.push_back(so.back() + ns); ro.push_back(ro.back() + nr);
            }
            CHECK(h[me].peers == peers && h[me].send_off == so && h[me].recv_off == ro && h[me].send_idx == si);
        }
        if (g == sym) CHECK((h[0].peers == std::vector<int>{1}) && (h[2].peers == std::vector<int>{1}) && (h[1].peers == std::vector<int>{0, 2}));
        else CHECK((h[0].peers == std::vector<int>{1, 2}) && (h[2].peers == std::vector<int>{0, 1}) && h[2].recv_off[1] == 0 && h[2].send_off[1] == 1);
        // the send list of a for b = the order in which b receives: b's ghosts inside a's slab, ascending
        for (int a = 0; a < 3; ++a)
            for (size_t ia = 0; ia < h[a].peers.size(); ++ia) {
                const int b = h[a].peers[ia];
                ivec sent, recv;
                for (int64_t i = h[a].send_off[ia]; i < h[a].send_off[ia + 1]; ++i) sent.push_back((int32_t)(h[a].send_idx[(size_t)i] + slabs[2 * a]));
                const size_t ib = (size_t)(std::find(h[b].peers.begin(), h[b].peers.end(), a) - h[b].peers.begin());
                CHECK(ib < h[b].peers.size());
                // b's receive segment ib covers these positions of its (sorted) ghost list
                int64_t before = 0;
                for (int32_t c : g[(size_t)b]) before += c < slabs[2 * a];
                for (int64_t i = 0; i < h[b].recv_off[ib + 1] - h[b].recv_off[ib]; ++i) recv.push_back(g[(size_t)b][(size_t)(before + i)]);
                CHECK(sent == recv);
            }
    }
    const std::vector<ivec> &g = sym;
    CASE("halo plan one rank");
    {
        const int64_t one[2] = {0, 5};
        HaloPlan s;
        halo_plan(0, 1, one, {}, as_bytes({{}}), s);
        CHECK(s.peers.empty() && s.send_off == std::vector<int64_t>{0} && s.recv_off == std::vector<int64_t>{0} && s.send_idx.empty());
    }
    CASE("halo plan refusals");
    auto refused = [&](const int64_t *sl, const std::vector<ivec> &gg, const char *text) {
        HaloPlan x;
        try {
            halo_plan(1, 3, sl, gg[1], as_bytes(gg), x);
        } catch (const Error &e) {
            return e.code == SPK_ERR_ARG && e.msg == text;
        }
        return false;
    };
    const int64_t gap[6] = {0, 4, 5, 7, 7, 12}, overlap[6] = {0, 4, 3, 7, 7, 12};
    CHECK(refused(gap, g, "A00: row slabs must tile [0,n) in rank order"));
    CHECK(refused(overlap, g, "A00: row slabs must tile [0,n) in rank order"));
    CHECK(refused(slabs, {{4, 6}, {1, 3, 7, 8, 12}, {5, 6}}, "A00: ghost columns not owned by any rank"));   // 12: nobody's

    CASE("send ranges");
    {
        HaloPlan p;
        p.peers = {0, 2};
        p.send_off = {0, 3, 5};
        p.send_idx = {4, 5, 6, 0, 1};
        HostSendRanges R = send_ranges(p);
        CHECK(R.n == 2 && R.r0[0] == 4 && R.len[0] == 3 && R.off[0] == 0 && R.r0[1] == 0 && R.len[1] == 2 && R.off[1] == 3);
        p.send_idx = {4, 5, 7, 0, 1};   // one gap
        CHECK(send_ranges(p).n == 0);
        p.send_idx = {4, 5, 6, 1, 0};   // descending is not a range either
        CHECK(send_ranges(p).n == 0);
        p.peers = {0, 1, 2, 3, 5};      // five peers
        p.send_off = {0, 1, 2, 3, 4, 5};
        p.send_idx = {0, 1, 2, 3, 4};
        CHECK(send_ranges(p).n == 0);
        p.peers.pop_back(); p.send_off.pop_back(); p.send_idx.pop_back();
        CHECK(send_ranges(p).n == 4);
        p.peers = {3};                  // a peer I only receive from: an empty range
        p.send_off = {0, 0};
        p.send_idx.clear();
        R = send_ranges(p);
        CHECK(R.n == 1 && R.len[0] == 0 && R.r0[0] == 0);
        CHECK(send_ranges(HaloPlan{}).n == 0);
    }
}

static void test_ghosts()
{
    CASE("ghost numbering and split_csr");
    // rows 3..6 of an 11-column matrix; off-rank columns repeated and unsorted
    const int32_t rp[5] = {0, 4, 6, 9, 11};
    const int32_t ci[11] = {9, 3, 0, 9, 4, 10, 0, 5, 2, 6, 9};
    double va[11];
    for (int i = 0; i < 11; ++i) va[i] = 1.0 + i;
    ivec off;
    for (int32_t c : ci)
        if (c < 3 || c >= 7) off.push_back(c);
    ivec garray = off;
    ghost_list(garray);
    CHECK((garray == ivec{0, 2, 9, 10}));
    ivec num = off;
    ghost_renumber(garray, num.data(), num.size());
    for (size_t i = 0; i < off.size(); ++i) CHECK(garray[(size_t)num[i]] == off[i] && num[i] == ghost_number(garray, off[i]));
    SplitCsr s;
    split_csr(3, 4, rp, ci, va, s, 11);
    CHECK(!s.bad_column && s.garray == garray && s.o_colidx.size() == num.size());
    for (size_t i = 0; i < num.size(); ++i) CHECK(s.o_colidx[i] == num[i]);
    CHECK(s.d_rowptr[4] == 4 && s.o_rowptr[4] == 7 && s.d_colidx[0] == 0 && s.d_val[0] == 2.0 && s.o_val[0] == 1.0);
    CASE("off-rank row compression");
    ivec rows, corp;
    const int32_t orp[6] = {0, 0, 2, 2, 2, 5};
    compress_offrank_rows(orp, 5, rows, corp);
    CHECK((rows == ivec{1, 4}) && (corp == ivec{0, 2, 5}));
    compress_offrank_rows(nullptr, 5, rows, corp);
    CHECK(rows.empty() && (corp == ivec{0}));
}

// ---- the constraint block ----
static void test_localise()
{
    CASE("B localise and sort");
    const int64_t lo = 10, hi = 20;
    const int32_t rp[4] = {0, 2, 7, 8};
    const int32_t ci[8] = {11, 19, 15, 12, 15, 10, 12, 13};   // row 1 unsorted, 15 and 12 twice
    const double va[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    int32_t col[8];
    double v[8];
    localise_and_sort(3, rp, ci, va, lo, hi, col, v);
    const int32_t want_c[8] = {1, 9, 0, 2, 2, 5, 5, 3};
    const double want_v[8] = {1, 2, 6, 4, 7, 3, 5, 8};   // equal columns keep their order; values follow
    for (int i = 0; i < 8; ++i) CHECK(col[i] == want_c[i] && v[i] == want_v[i]);
    for (int32_t bad : {-1, (int32_t)lo - 1, (int32_t)hi}) {
        int32_t c2[8];
        std::memcpy(c2, ci, sizeof c2);
        c2[4] = bad;
        char text[128];
        std::snprintf(text, sizeof text, "A10: column %d not owned by this rank [10,20)", bad);
        bool caught = false;
        try {
            localise_and_sort(3, rp, c2, va, lo, hi, col, v);
        } catch (const Error &e) {
            caught = e.code == SPK_ERR_ARG && e.msg == text;
        }
        CHECK(caught);
    }
}

static void test_wide_rows()
{
    CASE("B wide rows");
    ivec rp(9, 0);
    for (int r = 0; r < 8; ++r) rp[(size_t)r + 1] = rp[(size_t)r] + (r % 3);   // some empty, all below the threshold
    CHECK((wide_rows(8, rp.data(), 4) == ivec{0, 1, 2, 3, 4, 5, 6, 7}));
    CHECK(wide_rows(0, rp.data(), 4).empty());
    // m = 12: nine rows over the threshold 4; rows 2 and 9 are the shortest of them, equally long: the lower one stays
    const int len[12] = {9, 4, 5, 8, 0, 7, 6, 10, 3, 5, 11, 12};
    rp.assign(13, 0);
    for (int r = 0; r < 12; ++r) rp[(size_t)r + 1] = rp[(size_t)r] + len[r];
    CHECK((wide_rows(12, rp.data(), 4) == ivec{0, 2, 3, 5, 6, 7, 10, 11}));
    CHECK((wide_rows(12, rp.data(), 9) == ivec{7, 10, 11}));
    CHECK(wide_rows(12, rp.data(), 12).empty());
    // the set-up's own threshold (8192, strict): 8193 is wide, 8192 is not; twelve rows above it, ten of them 8200..8209
    // entries with rows 7 and 12 equal at the eighth place -- the lower row goes wide, rows 12 and the shortest (5) stay,
    // and so do the two 8193-entry rows 0 and 15, which are shorter than all ten
    const int big[16] = {8193, 8192, 1, 8209, 8208, 8200, 8207, 8202, 2046, 8206, 8205, 8204, 8202, 8203, 2, 8193};
    rp.assign(17, 0);
    for (int r = 0; r < 16; ++r) rp[(size_t)r + 1] = rp[(size_t)r] + big[r];
    CHECK((wide_rows(16, rp.data(), 8192) == ivec{3, 4, 6, 7, 9, 10, 11, 13}));
    CHECK((wide_rows(16, rp.data(), 8193) == ivec{3, 4, 6, 7, 9, 10, 11, 13}));
    CHECK((wide_rows(16, rp.data(), 8202) == ivec{3, 4, 6, 9, 10, 11, 13}));   // strict: the two of 8202 are not above it
    // no more than eight above the threshold: all of them, the first and the last row included
    const int few[11] = {8193, 8192, 5, 8192, 9000, 1, 8191, 2048, 3, 0, 8193};
    rp.assign(12, 0);
    for (int r = 0; r < 11; ++r) rp[(size_t)r + 1] = rp[(size_t)r] + few[r];
    CHECK((wide_rows(11, rp.data(), 8192) == ivec{0, 4, 10}));
}

static void test_windows()
{
    CASE("B window width");
    auto brute = [](int64_t nl, int cap) {
        int64_t win = 8192;
        while ((nl + win - 1) / win > cap) win *= 2;
        while (win > 1024 && (nl + win - 1) / win < 128) win /= 2;
        return (int32_t)win;
    };
    for (int32_t nl : {1, 128 * 1024 - 1, 128 * 1024, 128 * 1024 + 1, 127 * 2048, 127 * 2048 + 1, 127 * 8192 + 1, 2048 * 8192, 2048 * 8192 + 1})
        CHECK(window_width(nl, 2048) == brute(nl, 2048));
    CHECK(window_width(1, 2048) == 1024 && window_width(128 * 1024 + 1, 2048) == 1024 && window_width(127 * 2048 + 1, 2048) == 2048);
    CHECK(window_width(2048 * 8192, 2048) == 8192 && window_width(2048 * 8192 + 1, 2048) == 16384);   // the width doubles

    CASE("B window pointers");
    // nl = 10, windows of 4: [0,4) [4,8) [8,10); row 0 has an entry exactly on a boundary and an empty middle window
    const int32_t wrp[3] = {0, 4, 6}, wcol[6] = {0, 3, 8, 9, 4, 7};
    const int32_t nwin = 3, mw = 2;
    ivec wp((size_t)(nwin + 1) * mw, -1);
    window_pointers(mw, wrp, wcol, 10, 4, nwin, wp.data());
    for (int r = 0; r < mw; ++r)
        for (int w = 0; w <= nwin; ++w) {
            int32_t want = wrp[r];
            while (want < wrp[r + 1] && wcol[want] < std::min(w * 4, 10)) ++want;
            CHECK(wp[(size_t)w * mw + r] == want);
        }
    CHECK((wp == ivec{0, 4, 2, 4, 2, 6, 4, 6}));
    ivec none(1, -7);
    window_pointers(0, wrp, wcol, 10, 4, 0, none.data());   // no wide row: nothing written
    CHECK(none[0] == -7);
}

static void test_gather_rows()
{
    CASE("B short-row CSR and wide concatenation");
    const int32_t rp[5] = {0, 2, 5, 5, 7}, col[7] = {1, 4, 0, 2, 3, 5, 6};
    const double v[7] = {1, 2, 3, 4, 5, 6, 7};
    ivec orp, oci;
    std::vector<double> ov;
    gather_rows(4, rp, col, v, {1, 3}, true, orp, oci, ov);    // rows 1 and 3 left empty
    CHECK((orp == ivec{0, 2, 2, 2, 2}) && (oci == ivec{1, 4}) && (ov == std::vector<double>{1, 2}));
    gather_rows(4, rp, col, v, {1, 3}, false, orp, oci, ov);   // rows 1 and 3 alone
    CHECK((orp == ivec{0, 3, 5}) && (oci == ivec{0, 2, 3, 5, 6}) && (ov == std::vector<double>{3, 4, 5, 6, 7}));
    gather_rows(4, rp, col, v, {}, true, orp, oci, ov);
    CHECK((orp == ivec(rp, rp + 5)) && (oci == ivec(col, col + 7)));
}

static void test_transpose()
{
    CASE("B transpose");
    const int32_t nl = 3 * 4096 + 5, m = 9, threads = 4;
    // parallel_for really splits this column range: the thread indices it reports
    std::set<int> seen;
    std::vector<int64_t> cuts;
    std::mutex mu;
    parallel_for(nl, [&](int64_t a, int64_t b, int t) { std::lock_guard<std::mutex> l(mu); seen.insert(t); cuts.push_back(a); (void)b; }, threads);
    CHECK((seen == std::set<int>{0, 1, 2, 3}));
    std::vector<ivec> rows((size_t)m);
    for (int32_t c = 0; c < nl; ++c) {
        if (c == 777) continue;                          // an empty column
        rows[0].push_back(c);                            // a row crossing every thread boundary
        if (c % 7 == 3) rows[1].push_back(c);
        if (c % 1000 < 3) rows[(size_t)(2 + c % 5)].push_back(c);
        for (int64_t cut : cuts)                         // entries right at and before the cuts
            if (c == cut || c + 1 == cut) rows[8].push_back(c);
    }
    rows[4].clear();                                     // an empty row
    ivec rp(1, 0), col;
    std::vector<double> v;
    for (const ivec &r : rows) {
        for (int32_t c : r) { col.push_back(c); v.push_back(0.5 * (double)col.size()); }
        rp.push_back((int32_t)col.size());
    }
    ivec trp((size_t)nl + 1, 0), tci(col.size(), -1);
    std::vector<double> tv(col.size(), -1.0);
    transpose_rows(m, nl, rp.data(), col.data(), v.data(), trp.data(), tci.data(), tv.data(), threads);
    // sequential counting sort
    ivec rrp((size_t)nl + 1, 0), rci(col.size());
    std::vector<double> rv(col.size());
    for (int32_t c : col) rrp[(size_t)c + 1]++;
    for (int32_t i = 0; i < nl; ++i) rrp[(size_t)i + 1] += rrp[(size_t)i];
    ivec fill(rrp.begin(), rrp.end() - 1);
    for (int32_t r = 0; r < m; ++r)
        for (int32_t k = rp[(size_t)r]; k < rp[(size_t)r + 1]; ++k) {
            const int32_t p = fill[(size_t)col[(size_t)k]]++;
            rci[(size_t)p] = r;
            rv[(size_t)p] = v[(size_t)k];
        }
    CHECK(trp == rrp && tci == rci && tv == rv);
    CHECK(trp[778] == trp[777]);
    ivec t1((size_t)nl + 1, 0), c1(col.size());   // and on one thread
    std::vector<double> v1(col.size());
    transpose_rows(m, nl, rp.data(), col.data(), v.data(), t1.data(), c1.data(), v1.data(), 1);
    CHECK(t1 == rrp && c1 == rci && v1 == rv);
}

int main()
{
    test_field_layout_2();
    test_field_layout_3();
    test_field_widths();
    test_plane_offsets();
    test_class_numbering();
    test_halo_plan();
    test_ghosts();
    test_localise();
    test_wide_rows();
    test_windows();
    test_gather_rows();
    test_transpose();
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("all set-up host checks passed\n");
    return 0;
}
