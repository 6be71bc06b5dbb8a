// amg_host_check.cpp -- the host multigrid hierarchy (csrc/spk_amg_host.cpp over spk_amg_levels.hpp) without a GPU and
// without ROCm, through the C entry points Python uses (spk_amg_build_host, spk_amg_refresh_host, spk_amg_host_info,
// spk_amg_host_level, spk_amg_host_aggregates, spk_amg_destroy_host), on the smallest shapes that reach each branch:
// compiled with g++ and the sanitizers by tests/test_amg_host_cpu.py and run as a plain process.  Every assertion on a
// hierarchy is exact; the one bound (the smoother's coefficients) is derived beside it.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "spk_amg.hpp"
#include "spk_amg_levels.hpp"
#include "spk_host.hpp"

static int failures = 0;
static std::string shape;   // what the failing line was working on
#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            std::printf("FAILED %s:%d [%s]: %s\n", __FILE__, __LINE__, shape.c_str(), #cond);   \
            ++failures;                                                                          \
        }                                                                                        \
    } while (0)

struct Csr {
    int32_t nrows = 0, ncols = 0;
    std::vector<int32_t> rp{0}, ci;
    std::vector<double> v;
};

// the (2 d)+1-point Laplacian plus a shift on mx x my x mz nodes, each entry times the bs x bs block M (SPD, so the
// Kronecker product is); `drop`: that node keeps its diagonal block only
static Csr laplacian(int mx, int my, int mz, int bs, int drop = -1)
{
    static const double M[2][2] = {{2.0, 0.5}, {0.5, 2.0}};
    const int m[3] = {mx, my, mz}, nn = mx * my * mz;
    Csr A;
    A.nrows = A.ncols = nn * bs;
    for (int node = 0; node < nn; ++node) {
        const int at[3] = {node % mx, node / mx % my, node / (mx * my)};
        int nb[7], cnt = 0;   // neighbours in ascending node order
        for (int a = 2; a >= 0; --a)
            if (at[a] > 0) nb[cnt++] = node - (a == 0 ? 1 : a == 1 ? mx : mx * my);
        nb[cnt++] = node;
        for (int a = 0; a < 3; ++a)
            if (at[a] + 1 < m[a]) nb[cnt++] = node + (a == 0 ? 1 : a == 1 ? mx : mx * my);
        for (int r = 0; r < bs; ++r) {
            for (int k = 0; k < cnt; ++k) {
                if (nb[k] != node && (node == drop || nb[k] == drop)) continue;
                const double a = nb[k] == node ? 2.0 * ((mx > 1) + (my > 1) + (mz > 1)) + 0.1 : -1.0;
                for (int c = 0; c < bs; ++c) {
                    A.ci.push_back(nb[k] * bs + c);
                    A.v.push_back(bs == 1 ? a : a * M[r][c]);
                }
            }
            A.rp.push_back((int32_t)A.ci.size());
        }
    }
    return A;
}

static Csr diagonal(const std::vector<double> &d)
{
    Csr A;
    A.nrows = A.ncols = (int32_t)d.size();
    for (size_t i = 0; i < d.size(); ++i) {
        A.ci.push_back((int32_t)i);
        A.v.push_back(d[i]);
        A.rp.push_back((int32_t)i + 1);
    }
    return A;
}

static Csr transpose(const Csr &A)
{
    Csr T;
    T.nrows = A.ncols, T.ncols = A.nrows;
    T.rp.assign((size_t)T.nrows + 1, 0);
    for (int32_t c : A.ci) ++T.rp[(size_t)c + 1];
    for (int32_t i = 0; i < T.nrows; ++i) T.rp[(size_t)i + 1] += T.rp[(size_t)i];
    T.ci.resize(A.ci.size());
    T.v.resize(A.v.size());
    std::vector<int32_t> pos(T.rp.begin(), T.rp.end() - 1);
    for (int32_t i = 0; i < A.nrows; ++i)
        for (int32_t k = A.rp[(size_t)i]; k < A.rp[(size_t)i + 1]; ++k) {
            const int32_t p = pos[(size_t)A.ci[(size_t)k]]++;
            T.ci[(size_t)p] = i, T.v[(size_t)p] = A.v[(size_t)k];
        }
    return T;
}

static bool same_bits(const std::vector<double> &a, const std::vector<double> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0);
}
static bool same(const Csr &a, const Csr &b)
{
    return a.nrows == b.nrows && a.ncols == b.ncols && a.rp == b.rp && a.ci == b.ci && same_bits(a.v, b.v);
}
static bool same(const spk::HostCsr &a, const Csr &b)
{
    return a.nrows == b.nrows && a.ncols == b.ncols && a.rp == b.rp && a.ci == b.ci && same_bits(a.v, b.v);
}
static bool ascending(const Csr &A)
{
    for (int32_t i = 0; i < A.nrows; ++i)
        for (int32_t k = A.rp[(size_t)i] + 1; k < A.rp[(size_t)i + 1]; ++k)
            if (A.ci[(size_t)k - 1] >= A.ci[(size_t)k]) return false;
    return true;
}

// one matrix through the entry point: the size query (all arrays NULL), then the filling call into arrays of exactly
// those sizes (the sanitizer sees a write past them), which must report the same sizes
static Csr level_matrix(const spk_amg_hier *h, int l, int which)
{
    Csr A;
    int64_t nnz = -1, nnz2 = -1;
    int32_t nr = -1, nc = -1;
    CHECK(spk_amg_host_level(h, l, which, &A.nrows, &A.ncols, &nnz, nullptr, nullptr, nullptr) == SPK_OK);
    if (nnz < 0 || A.nrows < 0) return Csr{};
    A.rp.assign((size_t)A.nrows + 1, -1);
    A.ci.assign((size_t)nnz, -1);
    A.v.assign((size_t)nnz, -1.0);
    CHECK(spk_amg_host_level(h, l, which, &nr, &nc, &nnz2, A.rp.data(), A.ci.data(), A.v.data()) == SPK_OK);
    CHECK(nr == A.nrows && nc == A.ncols && nnz2 == nnz);
    CHECK(A.rp[0] == 0 && A.rp[(size_t)A.nrows] == nnz);
    return A;
}

// everything a hierarchy holds, as the entry points give it
struct Snapshot {
    spk_amg_info info;
    std::vector<Csr> A, P, T;   // per level; P and the tentative P: all but the coarsest
    std::vector<std::vector<int32_t>> agg;
    Csr cinv;
};
static Snapshot snapshot(const spk_amg_hier *h)
{
    Snapshot s;
    CHECK(spk_amg_host_info(h, &s.info) == SPK_OK);
    const int L = s.info.levels;
    for (int l = 0; l < L; ++l) {
        s.A.push_back(level_matrix(h, l, SPK_AMG_OP));
        if (l + 1 == L) break;
        s.P.push_back(level_matrix(h, l, SPK_AMG_PROLONG));
        s.T.push_back(level_matrix(h, l, SPK_AMG_TENTATIVE));
        if (s.info.coarsening == SPK_AMG_COARSEN_GRID) continue;
        int32_t nn = -1, nn2 = -1;
        CHECK(spk_amg_host_aggregates(h, l, &nn, nullptr) == SPK_OK);
        std::vector<int32_t> agg((size_t)(nn > 0 ? nn : 0), -7);
        CHECK(spk_amg_host_aggregates(h, l, &nn2, agg.data()) == SPK_OK);
        CHECK(nn2 == nn);
        s.agg.push_back(agg);
    }
    s.cinv = level_matrix(h, L - 1, SPK_AMG_COARSE_INV);
    return s;
}
// the same bytes in every array, in cinv and in info.lambda_max
static bool same(const Snapshot &a, const Snapshot &b)
{
    if (a.A.size() != b.A.size() || a.P.size() != b.P.size() || a.agg != b.agg || !same(a.cinv, b.cinv)) return false;
    if (std::memcmp(a.info.lambda_max, b.info.lambda_max, sizeof a.info.lambda_max) != 0) return false;
    if (a.info.levels != b.info.levels || std::memcmp(a.info.rows, b.info.rows, sizeof a.info.rows) != 0) return false;
    for (size_t l = 0; l < a.A.size(); ++l)
        if (!same(a.A[l], b.A[l])) return false;
    for (size_t l = 0; l < a.P.size(); ++l)
        if (!same(a.P[l], b.P[l]) || !same(a.T[l], b.T[l])) return false;
    return true;
}

static std::vector<double> scaled(const std::vector<double> &v, double f)
{
    std::vector<double> w(v);
    for (double &x : w) x *= f;
    return w;
}

// what holds of every hierarchy, whatever built it
static void check_structure(const spk_amg_hier *h, const Snapshot &s, int bs, int isolated0)
{
    const int L = s.info.levels;
    const bool grid = s.info.coarsening == SPK_AMG_COARSEN_GRID;
    CHECK(L >= 1 && (int)s.A.size() == L && s.info.block_size == bs);
    CHECK((int)h->h.lv.size() == L);
    for (int l = 0; l < L; ++l) {
        const Csr &A = s.A[(size_t)l];
        CHECK(A.nrows == A.ncols && A.nrows == s.info.rows[l] && (int64_t)A.ci.size() == s.info.nnz[l]);
        CHECK(ascending(A));
        if (l >= 1) CHECK(same(transpose(A), A));   // symmetric to the bit
        if (l + 1 == L) break;
        const Csr &P = s.P[(size_t)l], &T = s.T[(size_t)l];
        CHECK(P.nrows == A.nrows && P.ncols == s.A[(size_t)l + 1].nrows && ascending(P) && ascending(T));
        CHECK(same(h->h.lv[(size_t)l].R, transpose(P)));   // R = P^T, entry for entry
        if (grid) {
            CHECK((int64_t)P.ci.size() == spk::grid_prolong_nnz(s.info.dims[l], s.info.dims[l + 1], bs));
            CHECK(same(T, P));   // no tentative prolongator: the hook returns P
            for (int32_t i = 0; i < P.nrows; ++i) {
                double sum = 0.0;
                for (int32_t k = P.rp[(size_t)i]; k < P.rp[(size_t)i + 1]; ++k) {
                    const double w = P.v[(size_t)k];
                    CHECK(w == 1.0 || w == 0.5 || w == 0.25 || w == 0.125);
                    sum += w;   // (exact: at most eight equal powers of two)
                }
                CHECK(sum == 1.0);
            }
            continue;
        }
        // the aggregates cover every non-isolated node once, with numbers in [0, na); an isolated node (no stored
        // non-zero outside its diagonal block: threshold 0) has none and its rows of P are empty
        const std::vector<int32_t> &agg = s.agg[(size_t)l];
        const int32_t nn = A.nrows / bs, na = P.ncols / bs;
        CHECK((int32_t)agg.size() == nn && P.ncols % bs == 0 && na >= 1);
        std::vector<int> used((size_t)na, 0);
        for (int32_t I = 0; I < nn; ++I) {
            bool isolated = true;
            for (int32_t r = I * bs; r < (I + 1) * bs; ++r)
                for (int32_t k = A.rp[(size_t)r]; k < A.rp[(size_t)r + 1]; ++k)
                    if (A.ci[(size_t)k] / bs != I && A.v[(size_t)k] != 0.0) isolated = false;
            const int32_t a = agg[(size_t)I];
            CHECK(isolated ? a == -1 : a >= 0 && a < na);
            if (l == 0 && isolated0 >= 0) CHECK(isolated == (I == isolated0));
            if (a >= 0 && a < na) ++used[(size_t)a];
            for (int32_t r = I * bs; r < (I + 1) * bs; ++r) {
                const int32_t tl = T.rp[(size_t)r + 1] - T.rp[(size_t)r], pl = P.rp[(size_t)r + 1] - P.rp[(size_t)r];
                CHECK(isolated ? tl == 0 && pl == 0 : tl == 1 && T.ci[(size_t)T.rp[(size_t)r]] == a * bs + (r - I * bs));
            }
        }
        for (int u : used) CHECK(u >= 1);
    }
    const int32_t nc = s.A[(size_t)L - 1].nrows;
    CHECK(s.cinv.nrows == nc && s.cinv.ncols == nc && (int64_t)s.cinv.v.size() == (int64_t)nc * nc);
    // what a query refuses
    int32_t nr = 0;
    CHECK(spk_amg_host_level(h, -1, SPK_AMG_OP, &nr, nullptr, nullptr, nullptr, nullptr, nullptr) == SPK_ERR_ARG);
    CHECK(spk_amg_host_level(h, L, SPK_AMG_OP, &nr, nullptr, nullptr, nullptr, nullptr, nullptr) == SPK_ERR_ARG);
    CHECK(spk_amg_host_level(h, 0, -1, &nr, nullptr, nullptr, nullptr, nullptr, nullptr) == SPK_ERR_ARG);
    CHECK(spk_amg_host_level(h, 0, SPK_AMG_COARSE_INV + 1, &nr, nullptr, nullptr, nullptr, nullptr, nullptr) == SPK_ERR_ARG);
    CHECK(spk_amg_host_level(h, L - 1, SPK_AMG_PROLONG, &nr, nullptr, nullptr, nullptr, nullptr, nullptr) == SPK_ERR_ARG);
    CHECK(spk_amg_host_level(h, L - 1, SPK_AMG_TENTATIVE, &nr, nullptr, nullptr, nullptr, nullptr, nullptr) == SPK_ERR_ARG);
    if (L > 1) CHECK(spk_amg_host_level(h, 0, SPK_AMG_COARSE_INV, &nr, nullptr, nullptr, nullptr, nullptr, nullptr) == SPK_ERR_ARG);
    if (grid) {
        CHECK(spk_amg_host_aggregates(h, 0, &nr, nullptr) == SPK_ERR_UNSUPPORTED);
    } else {
        CHECK(spk_amg_host_aggregates(h, -1, &nr, nullptr) == SPK_ERR_ARG);
        CHECK(spk_amg_host_aggregates(h, L - 1, &nr, nullptr) == SPK_ERR_ARG);
    }
}

static spk_amg_hier *build(const Csr &A, const std::vector<double> &val, const spk_amg_opts &o, int *rc = nullptr)
{
    spk_amg_hier *h = nullptr;
    const int r = spk_amg_build_host(A.nrows, A.rp.data(), A.ci.data(), val.data(), &o, &h);
    if (rc) *rc = r;
    else CHECK(r == SPK_OK);
    return h;
}

// one shape through everything: structure, two builds, the refreshes, the failing refresh
static void check_shape(const std::string &name, const Csr &A, const spk_amg_opts &o, int bs, int min_levels, int isolated0 = -1)
{
    shape = name;
    spk_amg_hier *h = build(A, A.v, o);
    if (!h) return;
    const Snapshot s = snapshot(h);
    CHECK(s.info.levels >= min_levels);
    check_structure(h, s, bs, isolated0);
    {   // a second build of the same input: the same bytes
        spk_amg_hier *h2 = build(A, A.v, o);
        if (h2) CHECK(same(snapshot(h2), s));
        CHECK(spk_amg_destroy_host(h2) == SPK_OK);
    }
    CHECK(spk_amg_refresh_host(h, A.v.data()) == SPK_OK);   // the same values: the same bytes
    CHECK(same(snapshot(h), s));
    CHECK(spk_amg_refresh_host(h, scaled(A.v, 8.0).data()) == SPK_OK);   // times 2^3 (binade_scale's claim)
    {
        const Snapshot s8 = snapshot(h);
        CHECK(std::memcmp(s8.info.lambda_max, s.info.lambda_max, sizeof s.info.lambda_max) == 0);
        CHECK(s8.A.size() == s.A.size() && s8.P.size() == s.P.size() && s8.agg == s.agg);
        for (size_t l = 0; l < s.A.size() && l < s8.A.size(); ++l) {
            CHECK(s8.A[l].rp == s.A[l].rp && s8.A[l].ci == s.A[l].ci && same_bits(s8.A[l].v, scaled(s.A[l].v, 8.0)));
            if (l < s.P.size() && l < s8.P.size()) CHECK(same(s8.P[l], s.P[l]) && same(s8.T[l], s.T[l]));
        }
        CHECK(same_bits(s8.cinv.v, scaled(s.cinv.v, 0.125)));
        check_structure(h, s8, bs, isolated0);
    }
    // an indefinite operator: the refresh returns what a build on those values returns, and leaves no hierarchy behind
    const std::vector<double> neg = scaled(A.v, -1.0);
    int rc_build = SPK_OK;
    spk_amg_hier *hn = build(A, neg, o, &rc_build);
    const std::string why_build = spk::create_error();
    CHECK(rc_build != SPK_OK && hn == nullptr && !why_build.empty());
    CHECK(spk_amg_refresh_host(h, neg.data()) == rc_build);
    CHECK(why_build == spk::create_error());
    CHECK(spk_amg_refresh_host(h, A.v.data()) == SPK_ERR_STATE);
    CHECK(spk_amg_destroy_host(h) == SPK_OK);
}

static spk_amg_opts defaults()
{
    spk_amg_opts o;
    spk_default_amg_opts(&o);
    return o;
}

static void check_hierarchies()
{
    spk_amg_opts agg = defaults();
    agg.coarse_eq_limit = 4;
    check_shape("7x7 aggregation", laplacian(7, 7, 1, 1), agg, 1, 2);
    check_shape("5x5 blocks of 2, node 12 decoupled", laplacian(5, 5, 1, 2, 12), agg, 2, 2, 12);
    check_shape("1x1", diagonal({3.0}), agg, 1, 1);
    {   // a diagonal matrix has no strong connection, so nothing coarsens and the loop never asks for its Ritz values: one
        // level through the entry points, and Lanczos itself called on it -- D^-1 A = I, so the first step's residual
        // vanishes, the loop breaks there and both Ritz values are the one entry a of the tridiagonal.  With D powers
        // of four every product with D^-1/2 and A is exact and a = sum q_i^2 of a vector normalised in floating point.
        // Roundings of DBL_EPSILON / 2 relative each: the squared norm 11 (6 products, 5 sums), halved by the square
        // root, which adds 1, as the division does -- 7.5 on q_i, 15 on q_i^2 -- and 11 more in the sum of the q_i^2:
        // 26 halves of DBL_EPSILON, below 16 DBL_EPSILON
        const std::vector<double> d{1.0, 4.0, 16.0, 64.0, 256.0, 1024.0};
        check_shape("6x6 diagonal", diagonal(d), agg, 1, 1);
        shape = "6x6 diagonal, Lanczos";
        spk::HostCsr H;
        const Csr D = diagonal(d);
        H.nrows = H.ncols = D.nrows, H.rp = D.rp, H.ci = D.ci, H.v = D.v;
        double lmin = 0.0, lmax = 0.0;
        spk::lanczos(H, spk::diag_inv(H), &lmin, &lmax);
        CHECK(lmin == lmax);
        CHECK(std::fabs(lmax - 1.0) <= 16.0 * DBL_EPSILON);
    }
    struct Grid { int m[3], sides; };
    for (const Grid &g : {Grid{{5, 5, 1}, SPK_AMG_SIDES_ODD}, Grid{{6, 7, 1}, SPK_AMG_SIDES_ANY}, Grid{{4, 4, 1}, SPK_AMG_SIDES_ANY},
                          Grid{{5, 5, 4}, SPK_AMG_SIDES_ANY}})
        for (int bs : {1, 2})
            for (int galerkin : {SPK_AMG_GALERKIN_PRODUCTS, SPK_AMG_GALERKIN_STENCIL}) {
                spk_amg_opts o = defaults();
                o.coarse_eq_limit = 4;
                o.coarsening = SPK_AMG_COARSEN_GRID;
                o.sides = g.sides;
                o.galerkin = galerkin;
                o.block_size = bs;
                std::memcpy(o.grid, g.m, sizeof o.grid);
                char name[96];
                std::snprintf(name, sizeof name, "grid %dx%dx%d sides %d bs %d galerkin %d", g.m[0], g.m[1], g.m[2], g.sides, bs, galerkin);
                check_shape(name, laplacian(g.m[0], g.m[1], g.m[2], bs), o, bs, 2);
            }
    {   // even sides: the last index has one parent (6 x 7 -> 4 x 4: fine x = 5 is coarse x = 3 alone)
        shape = "6x7 even side";
        spk_amg_opts o = defaults();
        o.coarse_eq_limit = 4, o.coarsening = SPK_AMG_COARSEN_GRID, o.sides = SPK_AMG_SIDES_ANY, o.block_size = 1;
        o.grid[0] = 6, o.grid[1] = 7, o.grid[2] = 1;
        const Csr A = laplacian(6, 7, 1, 1);
        spk_amg_hier *h = build(A, A.v, o);
        if (h) {
            const Snapshot s = snapshot(h);
            CHECK(s.info.dims[1][0] == 4 && s.info.dims[1][1] == 4 && s.info.dims[1][2] == 1);
            const Csr &P = s.P[0];
            CHECK(P.rp[6] - P.rp[5] == 1 && P.ci[(size_t)P.rp[5]] == 3 && P.v[(size_t)P.rp[5]] == 1.0);   // node (5, 0)
            CHECK(P.rp[4] - P.rp[3] == 2 && P.v[(size_t)P.rp[3]] == 0.5);                                  // node (3, 0): two parents
        }
        CHECK(spk_amg_destroy_host(h) == SPK_OK);
    }
}

// which options make the hierarchy: one field at a time from the defaults
static void check_opts_rule()
{
    shape = "option fields";
    struct Field { const char *name; std::function<void(spk_amg_opts &)> change; bool application; };
    std::vector<Field> fields{
        {"max_levels", [](spk_amg_opts &o) { o.max_levels += 1; }, false},
        {"coarse_eq_limit", [](spk_amg_opts &o) { o.coarse_eq_limit += 1; }, false},
        {"nsmooths", [](spk_amg_opts &o) { o.nsmooths += 1; }, false},
        {"smoother", [](spk_amg_opts &o) { o.smoother = SPK_AMG_RICHARDSON; }, false},
        {"threshold", [](spk_amg_opts &o) { o.threshold = 0.25; }, false},
        {"smooth_its", [](spk_amg_opts &o) { o.smooth_its += 1; }, false},
        {"block_size", [](spk_amg_opts &o) { o.block_size = 2; }, false},
        {"richardson_scale", [](spk_amg_opts &o) { o.richardson_scale = 0.5; }, false},
        {"setup", [](spk_amg_opts &o) { o.setup = SPK_AMG_SETUP_DEVICE; }, false},
        {"coarsening", [](spk_amg_opts &o) { o.coarsening = SPK_AMG_COARSEN_GRID; }, false},
        {"transfer", [](spk_amg_opts &o) { o.transfer = SPK_AMG_TRANSFER_STORED; }, false},
        {"sides", [](spk_amg_opts &o) { o.sides = SPK_AMG_SIDES_ANY; }, false},
        {"galerkin", [](spk_amg_opts &o) { o.galerkin = SPK_AMG_GALERKIN_STENCIL; }, false},
        {"lanczos", [](spk_amg_opts &o) { o.lanczos = SPK_AMG_LANCZOS_RESIDENT; }, false},
        {"cycle", [](spk_amg_opts &o) { o.cycle = SPK_AMG_CYCLE_W; }, true},
        {"tail", [](spk_amg_opts &o) { o.tail = SPK_AMG_TAIL_FUSED; }, true},
        {"tail_rows", [](spk_amg_opts &o) { o.tail_rows = 600; }, true},
        {"op", [](spk_amg_opts &o) { o.op = SPK_AMG_OPERATOR_STENCIL; }, true},
    };
    for (int i = 0; i < 4; ++i) fields.push_back({"esteig", [i](spk_amg_opts &o) { o.esteig[i] += 0.5; }, false});
    for (int i = 0; i < 3; ++i) fields.push_back({"grid", [i](spk_amg_opts &o) { o.grid[i] += 3; }, false});
    const spk_amg_opts a = defaults();
    CHECK(spk::amg_same_hierarchy_opts(a, a));
    for (const Field &f : fields) {
        shape = std::string("option field ") + f.name;
        spk_amg_opts b = a;
        f.change(b);
        CHECK(std::memcmp(&a, &b, sizeof a) != 0);
        CHECK(spk::amg_same_hierarchy_opts(a, b) == f.application);
        CHECK(spk::amg_same_hierarchy_opts(b, a) == f.application);
        spk_amg_opts c = a;
        spk::amg_take_application_opts(c, b);
        CHECK(spk::amg_same_hierarchy_opts(c, a));   // nothing of the hierarchy's is taken
        CHECK(c.cycle == b.cycle && c.tail == b.tail && c.tail_rows == b.tail_rows && c.op == b.op);
        if (f.application) CHECK(std::memcmp(&c, &b, sizeof b) == 0);
        else CHECK(std::memcmp(&c, &a, sizeof a) == 0);
    }
}

// the smoother's coefficients
static void check_smoother_coeffs()
{
    shape = "smoother coefficients";
    std::vector<double> al, be;
    spk_amg_opts o = defaults();
    o.smoother = SPK_AMG_RICHARDSON, o.richardson_scale = 0.6, o.smooth_its = 3;
    spk::smoother_coeffs(o, 0.1, 1.1, al, be);
    CHECK(al == std::vector<double>(3, 0.6) && be == std::vector<double>(3, 0.0));
    o = defaults();
    o.smooth_its = 1;
    spk::smoother_coeffs(o, 0.1, 1.1, al, be);
    CHECK(al.size() == 1 && be.size() == 1 && al[0] == 1.0 / (0.5 * (1.1 + 0.1)) && be[0] == 0.0);
    // Chebyshev (Saad, Alg. 12.1) against the same recurrence in long double from the same two doubles.  With u =
    // DBL_EPSILON / 2 the relative error of one rounding, to first order: theta and delta carry u each (one rounded sum;
    // the halving is exact), sigma = theta / delta 3 u, rho_0 = 1 / sigma 4 u.  In rho_k = 1 / (2 sigma - rho_{k-1}) the
    // error of 2 sigma enters with the factor 2 sigma rho_k <= 2 sigma rho_0 = 2 (rho_k decreases), that of rho_{k-1}
    // with rho_{k-1} rho_k < 1 -- d rho_k / d rho_{k-1} = rho_k^2 < 1: each step contracts what it inherits -- and the
    // subtraction and the division add u each: e_k <= 2 * 3 u + e_{k-1} + 2 u, so e_k <= (4 + 8 k) u.
    //   alpha_k = 2 rho_k / delta:   e_k + u (delta) + u (division)        = (6 + 8 k) u
    //   beta_k = rho_k rho_{k-1}:    e_k + e_{k-1} + u (product)           = (1 + 16 k) u
    // The reference's own roundings (2^-64 relative each, a few dozen of them) stay below one more u.  In DBL_EPSILON =
    // 2 u: alpha_k within (4 + 4 k) DBL_EPSILON, beta_k within (1 + 8 k) DBL_EPSILON, alpha_0 = 1 / theta exactly.
    const double intervals[2][2] = {{0.1, 1.1}, {0.3, 2.2}};
    for (int nu : {2, 3, 4})
        for (const auto &iv : intervals) {
            o = defaults();
            o.smooth_its = nu;
            spk::smoother_coeffs(o, iv[0], iv[1], al, be);
            CHECK((int)al.size() == nu && (int)be.size() == nu);
            const long double lo = iv[0], hi = iv[1], theta = 0.5L * (hi + lo), delta = 0.5L * (hi - lo), sigma = theta / delta;
            long double rho = 1.0L / sigma;
            CHECK(al[0] == 1.0 / (0.5 * (iv[1] + iv[0])) && be[0] == 0.0);
            for (int k = 1; k < nu && k < (int)al.size(); ++k) {
                const long double rn = 1.0L / (2.0L * sigma - rho), a = 2.0L * rn / delta, b = rn * rho;
                const double ea = (double)(std::fabs((long double)al[(size_t)k] - a) / a), eb = (double)(std::fabs((long double)be[(size_t)k] - b) / b);
                std::printf("smoother_coeffs [%g, %g] nu %d step %d: alpha off by %.2f eps (bound %d), beta by %.2f eps (bound %d)\n",
                            iv[0], iv[1], nu, k, ea / DBL_EPSILON, 4 + 4 * k, eb / DBL_EPSILON, 1 + 8 * k);
                CHECK(ea <= (4 + 4 * k) * DBL_EPSILON);
                CHECK(eb <= (1 + 8 * k) * DBL_EPSILON);
                rho = rn;
            }
        }
}

int main()
{
    check_hierarchies();
    check_opts_rule();
    check_smoother_coeffs();
    if (failures) return 1;
    std::printf("all multigrid host checks passed\n");
    return 0;
}
