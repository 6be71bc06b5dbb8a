// spk_amg_host.cpp -- the multigrid hierarchy on the host: smoothed aggregation (-pc_type gamg) and grid coarsening
// (-pc_type mg, SPK_AMG_COARSEN_GRID), built at KSPSetUp from the A00 block and, with reuse on (spk_pc_set_amg_reuse),
// refreshed on new values: HostRoute, the host's side of the two loops of spk_amg_levels.hpp, what it is made of, the
// rules on the options and the extern "C" entry points that need no GPU.  (The device's side: spk_amg_setup.cpp.)
// Under grid coarsening a level halves its odd sides (-spk_mg_sides any: the even ones too) and P is the tensor product of
// linear interpolations -- no graph, no aggregation, no prolongator smoothing; everything else (Ritz values, Galerkin
// products, coarse inverse, refresh) is shared.  -spk_mg_galerkin stencil (SPK_AMG_GALERKIN_STENCIL) forms the coarse
// operators of such a hierarchy by a gather on the node grid instead (spk_galerkin_core.hpp): both routes call it in
// coarsen_grid and, on new values, in regalerkin.
// Host-pure like spk_host.cpp (the standard library, include/spk.h and the host-pure headers: no HIP type, no device
// pointer): tests/host/amg_host_check.cpp runs it under the sanitizers.  Every step is deterministic (fixed traversal
// orders, no hashing of pointers, a fixed Lanczos start vector): two builds of the same matrix give the same bytes.
// DESIGN.md "Algebraic multigrid" has the algorithm and where it departs from PETSc's GAMG.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "spk_amg.hpp"
#include "spk_amg_levels.hpp"
#include "spk_galerkin_core.hpp"
#include "spk_host.hpp"
#include "spk_lanczos_core.hpp"

namespace spk {

// columns sorted within each row (the caller's order is arbitrary); perm: where every sorted entry stood
void sort_rows(HostCsr &A, std::vector<int32_t> *perm)
{
    struct Entry { int32_t first; double second; int32_t from; };
    std::vector<Entry> row;
    if (perm) perm->resize(A.ci.size());
    for (int32_t i = 0; i < A.nrows; ++i) {
        const int32_t k0 = A.rp[(size_t)i], k1 = A.rp[(size_t)i + 1];
        row.clear();
        for (int32_t k = k0; k < k1; ++k) row.push_back({A.ci[(size_t)k], A.v[(size_t)k], k});
        std::sort(row.begin(), row.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
        for (int32_t k = k0; k < k1; ++k) {
            A.ci[(size_t)k] = row[(size_t)(k - k0)].first;
            A.v[(size_t)k] = row[(size_t)(k - k0)].second;
            if (perm) (*perm)[(size_t)k] = row[(size_t)(k - k0)].from;
        }
    }
}

// bs = 3 or 2 when the rows of every block row share one column list made of whole blocks, else 1
int detect_bs(const HostCsr &A)
{
    for (int bs : {3, 2}) {
        if (A.nrows % bs) continue;
        bool ok = true;
        for (int32_t r0 = 0; ok && r0 < A.nrows; r0 += bs) {
            const int32_t b0 = A.rp[(size_t)r0], len = A.rp[(size_t)r0 + 1] - b0;
            if (len % bs) { ok = false; break; }
            for (int k = 1; ok && k < bs; ++k) {
                const int32_t bk = A.rp[(size_t)r0 + k];
                if (A.rp[(size_t)r0 + k + 1] - bk != len) { ok = false; break; }
                for (int32_t j = 0; j < len; ++j)
                    if (A.ci[(size_t)(bk + j)] != A.ci[(size_t)(b0 + j)]) { ok = false; break; }
            }
            for (int32_t j = 0; ok && j < len; j += bs) {
                const int32_t c0 = A.ci[(size_t)(b0 + j)];
                if (c0 % bs) { ok = false; break; }
                for (int k = 1; k < bs; ++k)
                    if (A.ci[(size_t)(b0 + j + k)] != c0 + k) { ok = false; break; }
            }
        }
        if (ok) return bs;
    }
    return 1;
}

static HostCsr transpose(const HostCsr &A)
{
    HostCsr T;
    T.nrows = A.ncols;
    T.ncols = A.nrows;
    T.rp.assign((size_t)T.nrows + 1, 0);
    for (int32_t c : A.ci) ++T.rp[(size_t)c + 1];
    for (int32_t i = 0; i < T.nrows; ++i) T.rp[(size_t)i + 1] += T.rp[(size_t)i];
    T.ci.resize(A.ci.size());
    T.v.resize(A.v.size());
    std::vector<int32_t> pos(T.rp.begin(), T.rp.end() - 1);
    for (int32_t i = 0; i < A.nrows; ++i)   // rows in order: the columns of T come out sorted
        for (int32_t k = A.rp[(size_t)i]; k < A.rp[(size_t)i + 1]; ++k) {
            const int32_t p = pos[(size_t)A.ci[(size_t)k]]++;
            T.ci[(size_t)p] = i;
            T.v[(size_t)p] = A.v[(size_t)k];
        }
    return T;
}

// C = A B (Gustavson, dense row accumulator; the sums run in A's then B's stored order; no entry is dropped)
static HostCsr spgemm(const HostCsr &A, const HostCsr &B)
{
    HostCsr C;
    C.nrows = A.nrows;
    C.ncols = B.ncols;
    C.rp.assign((size_t)C.nrows + 1, 0);
    std::vector<double> acc((size_t)B.ncols, 0.0);
    std::vector<int32_t> mark((size_t)B.ncols, -1), cols;
    for (int32_t i = 0; i < A.nrows; ++i) {
        cols.clear();
        for (int32_t k = A.rp[(size_t)i]; k < A.rp[(size_t)i + 1]; ++k) {
            const int32_t r = A.ci[(size_t)k];
            const double a = A.v[(size_t)k];
            for (int32_t q = B.rp[(size_t)r]; q < B.rp[(size_t)r + 1]; ++q) {
                const int32_t j = B.ci[(size_t)q];
                if (mark[(size_t)j] != i) {
                    mark[(size_t)j] = i;
                    acc[(size_t)j] = 0.0;
                    cols.push_back(j);
                }
                acc[(size_t)j] += a * B.v[(size_t)q];
            }
        }
        std::sort(cols.begin(), cols.end());
        for (int32_t j : cols) {
            C.ci.push_back(j);
            C.v.push_back(acc[(size_t)j]);
        }
        C.rp[(size_t)i + 1] = (int32_t)C.ci.size();
    }
    return C;
}

// C = a A + b B over the union of the patterns (both sorted)
static HostCsr add(double a, const HostCsr &A, double b, const HostCsr &B)
{
    HostCsr C;
    C.nrows = A.nrows;
    C.ncols = A.ncols;
    C.rp.assign((size_t)C.nrows + 1, 0);
    for (int32_t i = 0; i < A.nrows; ++i) {
        int32_t p = A.rp[(size_t)i], pe = A.rp[(size_t)i + 1], q = B.rp[(size_t)i], qe = B.rp[(size_t)i + 1];
        while (p < pe || q < qe) {
            const int32_t ca = p < pe ? A.ci[(size_t)p] : INT32_MAX, cb = q < qe ? B.ci[(size_t)q] : INT32_MAX;
            if (ca == cb) { C.ci.push_back(ca); C.v.push_back(a * A.v[(size_t)p++] + b * B.v[(size_t)q++]); }
            else if (ca < cb) { C.ci.push_back(ca); C.v.push_back(a * A.v[(size_t)p++]); }
            else { C.ci.push_back(cb); C.v.push_back(b * B.v[(size_t)q++]); }
        }
        C.rp[(size_t)i + 1] = (int32_t)C.ci.size();
    }
    return C;
}

std::vector<double> diag_inv(const HostCsr &A)
{
    std::vector<double> d((size_t)A.nrows);
    for (int32_t i = 0; i < A.nrows; ++i) {
        double a = 0.0;
        for (int32_t k = A.rp[(size_t)i]; k < A.rp[(size_t)i + 1]; ++k)
            if (A.ci[(size_t)k] == i) a = A.v[(size_t)k];
        d[(size_t)i] = a == 0.0 ? 1.0 : 1.0 / a;   // as the device's PCJACOBI set-up
    }
    return d;
}

// number of eigenvalues of the symmetric tridiagonal (al, be[1..k)) below x (Sturm sequence)
static int sturm_count(const std::vector<double> &al, const std::vector<double> &be, double x)
{
    int cnt = 0;
    double d = 1.0;
    for (size_t i = 0; i < al.size(); ++i) {
        const double b2 = i ? be[i] * be[i] : 0.0;
        d = al[i] - x - (i ? b2 / d : 0.0);
        if (d == 0.0) d = -1e-300;
        if (d < 0.0) ++cnt;
    }
    return cnt;
}

// extreme eigenvalues of the Lanczos tridiagonal (al, be[1..k)) by Sturm bisection: lmax from below, lmin from above
void ritz_extremes(const std::vector<double> &al, const std::vector<double> &be, double *lmin, double *lmax)
{
    double glo = al[0], ghi = al[0];   // Gershgorin bounds of the tridiagonal
    for (size_t i = 0; i < al.size(); ++i) {
        const double r = (i ? std::fabs(be[i]) : 0.0) + (i + 1 < al.size() ? std::fabs(be[i + 1]) : 0.0);
        glo = std::min(glo, al[i] - r);
        ghi = std::max(ghi, al[i] + r);
    }
    const int m = (int)al.size();
    double lo = glo, hi = ghi;
    for (int it = 0; it < 200 && hi - lo > 1e-15 * std::max(1.0, std::fabs(hi)); ++it) {
        const double mid = 0.5 * (lo + hi);
        if (sturm_count(al, be, mid) >= m) hi = mid; else lo = mid;
    }
    *lmax = lo;   // below the largest Ritz value
    lo = glo, hi = ghi;
    for (int it = 0; it < 200 && hi - lo > 1e-15 * std::max(1.0, std::fabs(hi)); ++it) {
        const double mid = 0.5 * (lo + hi);
        if (sturm_count(al, be, mid) >= 1) hi = mid; else lo = mid;
    }
    *lmin = hi;
}

static_assert(kLanczosSteps == lanczos_core::kSteps, "the state block of the resident route holds kLanczosSteps steps");

// extreme Ritz values of D^-1 A after kLanczosSteps Lanczos steps on the similar D^-1/2 A D^-1/2, from a fixed start vector.
// Ritz values lie inside the spectrum: both estimates approach from within (lmax from below).
// a_scale: a power of two; the steps run on a_scale A (every product with it is exact, and 1 changes no bit).  The refresh
// passes the one that brings A back to the binade it was built in, so that an operator rescaled by a power of two --
// where sqrt(d / 2) is no power-of-two multiple of sqrt(d) -- gives the Ritz values of the build to the bit.
void lanczos(const HostCsr &A, const std::vector<double> &dinv, double *lmin, double *lmax, double a_scale)
{
    const int32_t n = A.nrows;
    std::vector<double> s((size_t)n), q((size_t)n), qp((size_t)n, 0.0), w((size_t)n), t((size_t)n);
    for (int32_t i = 0; i < n; ++i) s[(size_t)i] = std::sqrt(std::fabs(dinv[(size_t)i] / a_scale));
    double nq = 0.0;
    for (int32_t i = 0; i < n; ++i) {   // integer hash: the same start vector on every machine
        uint32_t h = (uint32_t)i * 2654435761u + 0x9e3779b9u;
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        q[(size_t)i] = 0.5 + (double)(h & 0xffffu) / 65536.0;
        nq += q[(size_t)i] * q[(size_t)i];
    }
    nq = std::sqrt(nq);
    for (double &x : q) x /= nq;
    std::vector<double> al, be{0.0};
    const int k = (int)std::min<int64_t>(kLanczosSteps, n);
    for (int j = 0; j < k; ++j) {
        for (int32_t i = 0; i < n; ++i) t[(size_t)i] = s[(size_t)i] * q[(size_t)i];
        double a = 0.0;
        for (int32_t i = 0; i < n; ++i) {
            double acc = 0.0;
            for (int32_t p = A.rp[(size_t)i]; p < A.rp[(size_t)i + 1]; ++p) acc += A.v[(size_t)p] * t[(size_t)A.ci[(size_t)p]];
            w[(size_t)i] = s[(size_t)i] * (acc * a_scale);
            a += w[(size_t)i] * q[(size_t)i];
        }
        al.push_back(a);
        double nb = 0.0;
        for (int32_t i = 0; i < n; ++i) {
            w[(size_t)i] -= a * q[(size_t)i] + be.back() * qp[(size_t)i];
            nb += w[(size_t)i] * w[(size_t)i];
        }
        nb = std::sqrt(nb);
        if (j + 1 == k || nb <= 1e-12 * std::fabs(a)) break;
        be.push_back(nb);
        qp.swap(q);
        for (int32_t i = 0; i < n; ++i) q[(size_t)i] = w[(size_t)i] / nb;
    }
    ritz_extremes(al, be, lmin, lmax);
}

// strong-connection graph of the bs x bs nodes (sorted neighbour lists, the node itself left out)
static void node_graph(const HostCsr &A, int bs, double theta, std::vector<int32_t> &gp, std::vector<int32_t> &gi)
{
    const int32_t nn = A.nrows / bs;
    std::vector<double> dn((size_t)nn, 0.0), acc((size_t)nn, 0.0);
    std::vector<int32_t> mark((size_t)nn, -1), cols;
    for (int32_t i = 0; i < A.nrows; ++i)
        for (int32_t k = A.rp[(size_t)i]; k < A.rp[(size_t)i + 1]; ++k)
            if (A.ci[(size_t)k] / bs == i / bs) dn[(size_t)(i / bs)] += A.v[(size_t)k] * A.v[(size_t)k];
    for (double &d : dn) d = std::sqrt(d);
    gp.assign((size_t)nn + 1, 0);
    gi.clear();
    for (int32_t I = 0; I < nn; ++I) {
        cols.clear();
        for (int32_t r = I * bs; r < (I + 1) * bs; ++r)
            for (int32_t k = A.rp[(size_t)r]; k < A.rp[(size_t)r + 1]; ++k) {
                const int32_t J = A.ci[(size_t)k] / bs;
                if (J == I) continue;
                if (mark[(size_t)J] != I) { mark[(size_t)J] = I; acc[(size_t)J] = 0.0; cols.push_back(J); }
                acc[(size_t)J] += A.v[(size_t)k] * A.v[(size_t)k];
            }
        std::sort(cols.begin(), cols.end());
        for (int32_t J : cols)
            if (std::sqrt(acc[(size_t)J]) > theta * std::sqrt(dn[(size_t)I] * dn[(size_t)J])) gi.push_back(J);
        gp[(size_t)I + 1] = (int32_t)gi.size();
    }
}

// Vanek's greedy three-phase aggregation in node order; returns the number of aggregates
int32_t aggregate(const std::vector<int32_t> &gp, const std::vector<int32_t> &gi, std::vector<int32_t> &agg)
{
    const int32_t nn = (int32_t)gp.size() - 1;
    agg.assign((size_t)nn, -1);
    auto iso = [&](int32_t i) { return gp[(size_t)i] == gp[(size_t)i + 1]; };
    int32_t na = 0;
    // phase 1: a node whose strong neighbours are all free forms an aggregate with them
    for (int32_t i = 0; i < nn; ++i) {
        if (agg[(size_t)i] >= 0 || iso(i)) continue;
        bool free = true;
        for (int32_t k = gp[(size_t)i]; k < gp[(size_t)i + 1] && free; ++k) free = agg[(size_t)gi[(size_t)k]] < 0;
        if (!free) continue;
        agg[(size_t)i] = na;
        for (int32_t k = gp[(size_t)i]; k < gp[(size_t)i + 1]; ++k) agg[(size_t)gi[(size_t)k]] = na;
        ++na;
    }
    // phase 2: the rest join the phase-1 aggregate they have the most strong connections to (ties: lowest index)
    const std::vector<int32_t> a1 = agg;
    std::vector<std::pair<int32_t, int32_t>> cnt;
    for (int32_t i = 0; i < nn; ++i) {
        if (a1[(size_t)i] >= 0 || iso(i)) continue;
        cnt.clear();
        for (int32_t k = gp[(size_t)i]; k < gp[(size_t)i + 1]; ++k) {
            const int32_t a = a1[(size_t)gi[(size_t)k]];
            if (a < 0) continue;
            auto it = std::find_if(cnt.begin(), cnt.end(), [a](const auto &p) { return p.first == a; });
            if (it == cnt.end()) cnt.emplace_back(a, 1); else ++it->second;
        }
        int32_t best = -1, bc = 0;
        for (const auto &p : cnt)
            if (p.second > bc || (p.second == bc && p.first < best)) { best = p.first; bc = p.second; }
        agg[(size_t)i] = best;
    }
    // phase 3: the leftovers form aggregates with their free neighbours
    for (int32_t i = 0; i < nn; ++i) {
        if (agg[(size_t)i] >= 0 || iso(i)) continue;
        agg[(size_t)i] = na;
        for (int32_t k = gp[(size_t)i]; k < gp[(size_t)i + 1]; ++k)
            if (agg[(size_t)gi[(size_t)k]] < 0) agg[(size_t)gi[(size_t)k]] = na;
        ++na;
    }
    return na;
}

// bs columns per aggregate (the bs constant vectors), entries 1/sqrt(|aggregate|); isolated nodes: zero rows
static HostCsr tentative(const std::vector<int32_t> &agg, int32_t na, int bs)
{
    std::vector<int32_t> size((size_t)na, 0);
    for (int32_t a : agg) if (a >= 0) ++size[(size_t)a];
    HostCsr P;
    P.nrows = (int32_t)agg.size() * bs;
    P.ncols = na * bs;
    P.rp.assign((size_t)P.nrows + 1, 0);
    for (size_t i = 0; i < agg.size(); ++i)
        for (int c = 0; c < bs; ++c) {
            const int32_t a = agg[i];
            if (a >= 0) {
                P.ci.push_back(a * bs + c);
                P.v.push_back(1.0 / std::sqrt((double)size[(size_t)a]));
            }
            P.rp[i * bs + c + 1] = (int32_t)P.ci.size();
        }
    return P;
}

// ---- grid coarsening (SPK_AMG_COARSEN_GRID): the halving rule and the tensor-product prolongator -------------------
// a direction of m nodes halves iff m is odd and >= 5 (SPK_AMG_SIDES_ODD), or m >= 4 (SPK_AMG_SIDES_ANY)
static bool grid_halves(int32_t m, int sides) { return sides == SPK_AMG_SIDES_ANY ? m >= 4 : m >= 5 && (m & 1); }
// the coarse grid of `fd`; false when no direction halves.  A halved side of m nodes keeps m / 2 + 1: (m + 1) / 2 of an odd
// m; of an even m the fine indices 0, 2, ..., m - 2 and m - 1
bool grid_coarse_dims(const int32_t fd[3], int32_t cd[3], int sides)
{
    bool any = false;
    for (int a = 0; a < 3; ++a) {
        cd[a] = grid_halves(fd[a], sides) ? fd[a] / 2 + 1 : fd[a];
        any = any || cd[a] != fd[a];
    }
    return any;
}
// the parents of fine index i in one direction of m nodes: `first`, and one more behind it when cnt == 2 (weight 1/2 each,
// else 1).  An odd i that is the last index (m even) is a coarse node itself: the one parent m / 2
struct GridParents { int32_t first, cnt; };
static GridParents grid_parents(int32_t i, int32_t m, bool halved)
{
    if (!halved) return {i, 1};
    if ((i & 1) && i == m - 1) return {(i + 1) / 2, 1};
    return (i & 1) ? GridParents{(i - 1) / 2, 2} : GridParents{i / 2, 1};
}
// entries of P = P_z (x) P_y (x) P_x (x) I_bs: per direction i + i/2 parents lie before fine index i; the last index of an
// even side has one parent, not two
int64_t grid_prolong_nnz(const int32_t fd[3], const int32_t cd[3], int bs)
{
    int64_t t = bs;
    for (int a = 0; a < 3; ++a) t *= cd[a] != fd[a] ? (int64_t)fd[a] + fd[a] / 2 - !(fd[a] & 1) : (int64_t)fd[a];
    return t;
}
// P as CSR with ascending columns, boundary nodes included: no special case for Dirichlet rows
static HostCsr grid_prolongator(const int32_t fd[3], const int32_t cd[3], int bs)
{
    HostCsr P;
    P.nrows = fd[0] * fd[1] * fd[2] * bs;
    P.ncols = cd[0] * cd[1] * cd[2] * bs;
    P.rp.assign(1, 0);
    P.rp.reserve((size_t)P.nrows + 1);
    const size_t nz = (size_t)grid_prolong_nnz(fd, cd, bs);
    P.ci.reserve(nz);
    P.v.reserve(nz);
    for (int32_t k = 0; k < fd[2]; ++k)
        for (int32_t j = 0; j < fd[1]; ++j)
            for (int32_t i = 0; i < fd[0]; ++i) {
                const GridParents px = grid_parents(i, fd[0], cd[0] != fd[0]), py = grid_parents(j, fd[1], cd[1] != fd[1]),
                                  pz = grid_parents(k, fd[2], cd[2] != fd[2]);
                const double w = 1.0 / (double)(px.cnt * py.cnt * pz.cnt);   // 1, 1/2, 1/4 or 1/8
                for (int c = 0; c < bs; ++c) {
                    for (int32_t kk = 0; kk < pz.cnt; ++kk)
                        for (int32_t jj = 0; jj < py.cnt; ++jj)
                            for (int32_t ii = 0; ii < px.cnt; ++ii) {
                                P.ci.push_back((((pz.first + kk) * cd[1] + py.first + jj) * cd[0] + px.first + ii) * bs + c);
                                P.v.push_back(w);
                            }
                    P.rp.push_back((int32_t)P.ci.size());
                }
            }
    return P;
}

// dense inverse of the SPD coarsest operator through Cholesky (symmetrised); a_scale as in lanczos: the factor is that
// of a_scale A and the inverse is scaled back, both exactly
std::vector<double> coarse_inverse(const HostCsr &A, double a_scale)
{
    const int32_t n = A.nrows;
    std::vector<double> L((size_t)n * n, 0.0), X((size_t)n * n, 0.0);
    for (int32_t i = 0; i < n; ++i)
        for (int32_t k = A.rp[(size_t)i]; k < A.rp[(size_t)i + 1]; ++k) L[(size_t)i * n + A.ci[(size_t)k]] = A.v[(size_t)k] * a_scale;
    for (int32_t j = 0; j < n; ++j) {
        double d = L[(size_t)j * n + j];
        for (int32_t k = 0; k < j; ++k) d -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
        if (!(d > 0.0)) fail(SPK_ERR_ARG, "amg: the coarsest operator (%d equations) is not positive definite", (int)n);
        d = std::sqrt(d);
        L[(size_t)j * n + j] = d;
        for (int32_t i = j + 1; i < n; ++i) {
            double s = L[(size_t)i * n + j];
            for (int32_t k = 0; k < j; ++k) s -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
            L[(size_t)i * n + j] = s / d;
        }
    }
    std::vector<double> y((size_t)n);
    for (int32_t c = 0; c < n; ++c) {   // L L^T x = e_c
        for (int32_t i = 0; i < n; ++i) {
            double s = i == c ? 1.0 : 0.0;
            for (int32_t k = 0; k < i; ++k) s -= L[(size_t)i * n + k] * y[(size_t)k];
            y[(size_t)i] = s / L[(size_t)i * n + i];
        }
        for (int32_t i = n - 1; i >= 0; --i) {
            double s = y[(size_t)i];
            for (int32_t k = i + 1; k < n; ++k) s -= L[(size_t)k * n + i] * X[(size_t)k * n + c];
            X[(size_t)i * n + c] = s / L[(size_t)i * n + i];
        }
    }
    for (int32_t i = 0; i < n; ++i)
        for (int32_t j = i + 1; j < n; ++j) {
            const double s = 0.5 * (X[(size_t)i * n + j] + X[(size_t)j * n + i]);
            X[(size_t)i * n + j] = X[(size_t)j * n + i] = s;
        }
    if (a_scale != 1.0)
        for (double &x : X) x *= a_scale;
    return X;
}

// sum |D_0^-1|: exactly homogeneous under a power of two (every partial sum scales with it), so its binade tells by
// which power of two an operator was rescaled since the build
double abs_sum(const std::vector<double> &x)
{
    double t = 0.0;
    for (double v : x) t += std::fabs(v);
    return t;
}
// the power of two that brings an operator with this sum |D^-1| back to the binade of the one with sum `built`
double binade_scale(double built, double now)
{
    if (!(built > 0.0) || !(now > 0.0) || !std::isfinite(built) || !std::isfinite(now)) return 1.0;
    return std::ldexp(1.0, std::ilogb(now) - std::ilogb(built));   // A grew by 2^k: |D^-1| shrank by it, A is scaled by 2^-k
}

// the smoother's interval on level l from the extreme Ritz values: the esteig rule and its refusal, for both loops
void smoother_interval(const spk_amg_opts &o, int l, double lmin, double lmax, double *lo, double *hi)
{
    *lo = o.esteig[0] * lmin + o.esteig[1] * lmax, *hi = o.esteig[2] * lmin + o.esteig[3] * lmax;
    if (o.smoother == SPK_AMG_CHEBYSHEV && !(*lo > 0.0 && *hi > *lo))
        fail(SPK_ERR_ARG, "amg: Chebyshev interval [%g, %g] on level %d is empty or not positive (esteig)", *lo, *hi, l);
}

// the smoothing steps of a level from its interval [lo, hi]: y+ = y + alpha[k] D^-1 (b - A y) + beta[k] (y - y-)
void smoother_coeffs(const spk_amg_opts &o, double lo, double hi, std::vector<double> &alpha, std::vector<double> &beta)
{
    const int nu = o.smooth_its;
    alpha.assign((size_t)nu, o.richardson_scale);
    beta.assign((size_t)nu, 0.0);
    if (o.smoother == SPK_AMG_CHEBYSHEV) {   // Saad, Alg. 12.1: d_k = rho_k rho_{k-1} d_{k-1} + 2 rho_k / delta D^-1 r_k
        const double theta = 0.5 * (hi + lo), delta = 0.5 * (hi - lo), sigma = theta / delta;
        double rho = 1.0 / sigma;
        alpha[0] = 1.0 / theta;
        for (int k = 1; k < nu; ++k) {
            const double rn = 1.0 / (2.0 * sigma - rho);
            alpha[(size_t)k] = 2.0 * rn / delta;
            beta[(size_t)k] = rn * rho;
            rho = rn;
        }
    }
}

// Which options make the hierarchy, stated once: cycle, tail, tail_rows, op and precision steer the application
// (amg_plan_cycle reads them at every set-up) and are the second function's; every other field decides the hierarchy and is compared by the
// first -- a refresh keeps a hierarchy only where they all agree.  A new field of spk_amg_opts goes on one side or the
// other: a hierarchy option missing from the comparison would make a stale hierarchy pass for a fresh one.
// (precision took the four bytes of padding behind lanczos: the size is the same)
static_assert(sizeof(spk_amg_opts) == 128 && offsetof(spk_amg_opts, precision) == 124, "spk_amg_opts has changed: put the new field into amg_same_hierarchy_opts or amg_take_application_opts");
bool amg_same_hierarchy_opts(const spk_amg_opts &a, const spk_amg_opts &b)
{
    bool same = a.max_levels == b.max_levels && a.coarse_eq_limit == b.coarse_eq_limit && a.nsmooths == b.nsmooths &&
                a.smoother == b.smoother && a.threshold == b.threshold && a.smooth_its == b.smooth_its &&
                a.block_size == b.block_size && a.richardson_scale == b.richardson_scale && a.setup == b.setup &&
                a.coarsening == b.coarsening && a.transfer == b.transfer && a.sides == b.sides && a.galerkin == b.galerkin &&
                a.lanczos == b.lanczos;
    for (int i = 0; i < 4; ++i) same = same && a.esteig[i] == b.esteig[i];
    for (int i = 0; i < 3; ++i) same = same && a.grid[i] == b.grid[i];
    return same;
}
void amg_take_application_opts(spk_amg_opts &dst, const spk_amg_opts &src)
{
    dst.cycle = src.cycle, dst.tail = src.tail, dst.tail_rows = src.tail_rows, dst.op = src.op, dst.precision = src.precision;
}

// what the application's options make of the levels `info` lists: after every build and every refresh, on both routes
// (build_levels clears the info and the host-route refresh copies the host's over it)
void fill_cycle_info(const spk_amg_opts &o, spk_amg_info &info)
{
    info.cycle = o.cycle;
    info.op = o.op;
    info.tail_first = amg_tail_first(info.levels, info.rows, o.cycle, o.tail, o.tail_rows);
    info.tail_launches = info.tail_first < 0 ? 0 : (int32_t)amg_tail_runs(amg_cycle_steps(info.levels, o.cycle), info.tail_first).size();
}

// A_{l+1} = (R A P + (R A P)^T) / 2 from the A, P and R of a level: exactly symmetric (the products agree to rounding)
static HostCsr galerkin_product(const AmgLevel &L)
{
    const HostCsr Ac = spgemm(L.R, spgemm(L.A, L.P));
    return add(0.5, Ac, 0.5, transpose(Ac));
}

namespace {
// the host route: every matrix a HostCsr of h.lv (level 0 and its D^-1 are there before the loop runs)
struct HostRoute {
    AmgHier &h;
    double a_scale = 1.0;   // the refresh's (see lanczos)
    AmgLevel &lv(int l) const { return h.lv[(size_t)l]; }
    int32_t rows(int l) const { return lv(l).A.nrows; }
    int64_t nnz(int l) const { return lv(l).A.nnz(); }
    void graph(int l, int bs, double theta, std::vector<int32_t> &gp, std::vector<int32_t> &gi) const { node_graph(lv(l).A, bs, theta, gp, gi); }
    void ritz(int l, double *lmin, double *lmax) const { lanczos(lv(l).A, lv(l).dinv, lmin, lmax, a_scale); }
    void set_interval(int l, double lo, double hi) const { lv(l).lo = lo, lv(l).hi = hi; }
    void coarsen(int l, int bs, std::vector<int32_t> agg, int32_t na, double omega, int nsmooths) const
    {
        AmgLevel &L = lv(l);
        L.agg = std::move(agg);
        L.Ptent = tentative(L.agg, na, bs);
        L.P = L.Ptent;
        for (int s = 0; s < nsmooths; ++s) {   // P = (I - omega D^-1 A) P
            HostCsr AP = spgemm(L.A, L.P);
            for (int32_t i = 0; i < AP.nrows; ++i)
                for (int32_t k = AP.rp[(size_t)i]; k < AP.rp[(size_t)i + 1]; ++k) AP.v[(size_t)k] *= L.dinv[(size_t)i];
            L.P = add(1.0, L.P, -omega, AP);
        }
        galerkin(l);
    }
    void coarsen_grid(int l, int bs, const int32_t fd[3], const int32_t cd[3]) const
    {
        if (grid_prolong_nnz(fd, cd, bs) > INT32_MAX)
            fail(SPK_ERR_UNSUPPORTED, "amg: the prolongator of level %d has more entries than 32-bit offsets address", l);
        lv(l).P = grid_prolongator(fd, cd, bs);
        if (h.o.galerkin != SPK_AMG_GALERKIN_STENCIL) return galerkin(l);
        if (galerkin::gs_nnz(cd, bs) > INT32_MAX)
            fail(SPK_ERR_UNSUPPORTED, "amg: the operator of level %d has more entries than 32-bit offsets address", l + 1);
        if (l == 0) galerkin_stencil_check_host(fd, bs, lv(0).A.rp.data(), lv(0).A.ci.data());
        lv(l).R = transpose(lv(l).P);
        h.lv.emplace_back();
        HostCsr &N = h.lv.back().A;
        N.nrows = N.ncols = cd[0] * cd[1] * cd[2] * bs;
        N.rp.assign((size_t)N.nrows + 1, 0);
        N.ci.assign((size_t)galerkin::gs_nnz(cd, bs), 0);
        N.v.assign(N.ci.size(), 0.0);
        stencil(l, fd, cd, bs);
    }
    // level l+1 by the grid-stencil gather (SPK_AMG_GALERKIN_STENCIL), the build's and the refresh's: pattern, values, D^-1
    void stencil(int l, const int32_t fd[3], const int32_t cd[3], int bs) const
    {
        const HostCsr &F = lv(l).A;
        HostCsr &N = lv(l + 1).A;
        galerkin_stencil_host(fd, cd, bs, F.rp.data(), F.ci.data(), F.v.data(), N.rp.data(), N.ci.data(), N.v.data());
        lv(l + 1).dinv = diag_inv(N);
    }
    // R = P^T and level l+1 from the P of level l
    void galerkin(int l) const
    {
        AmgLevel &L = lv(l);
        L.R = transpose(L.P);
        HostCsr An = galerkin_product(L);
        h.lv.emplace_back();   // (L dangles from here)
        h.lv.back().A = std::move(An);
        h.lv.back().dinv = diag_inv(h.lv.back().A);
    }
    int levels() const { return (int)h.lv.size(); }
    void regalerkin(int l) const
    {
        if (h.info.galerkin == SPK_AMG_GALERKIN_STENCIL) return stencil(l, h.info.dims[l], h.info.dims[l + 1], h.info.block_size);
        AmgLevel &L = lv(l), &N = lv(l + 1);
        HostCsr An = galerkin_product(L);
        if (An.rp != N.A.rp || An.ci != N.A.ci)   // (no product drops an entry: the patterns follow from the kept ones)
            fail(SPK_ERR_STATE, "amg: the refreshed operator of level %d has another pattern than the kept one", l + 1);
        N.A.v = std::move(An.v);
        N.dinv = diag_inv(N.A);
    }
    void check() const {}
    const HostCsr &coarsest() const { return h.lv.back().A; }
    void set_coarse_inverse(std::vector<double> cinv) const { h.cinv = std::move(cinv); }
};
}  // namespace

// the test hooks' copy-out, shared by the host hierarchy and the download of a device-built one
void csr_out(const HostCsr &M, const CsrOut &o)
{
    o.sizes(M.nrows, M.ncols, M.nnz());
    if (o.rowptr) std::memcpy(o.rowptr, M.rp.data(), sizeof(int32_t) * M.rp.size());
    if (o.colidx && M.nnz()) std::memcpy(o.colidx, M.ci.data(), sizeof(int32_t) * M.ci.size());
    if (o.val && M.nnz()) std::memcpy(o.val, M.v.data(), sizeof(double) * M.v.size());
}

// SPK_AMG_COARSE_INV: the dense n x n inverse as full CSR rows
void coarse_inv_out(int32_t n, const double *cinv, const CsrOut &o)
{
    o.sizes(n, n, (int64_t)n * n);
    for (int32_t i = 0; o.rowptr && i <= n; ++i) o.rowptr[i] = i * n;
    for (int64_t k = 0; o.colidx && k < (int64_t)n * n; ++k) o.colidx[k] = (int32_t)(k % n);
    if (o.val) std::memcpy(o.val, cinv, sizeof(double) * (size_t)n * n);
}

// what a query for matrix `which` of level l refuses on a hierarchy of L levels
void check_level_query(int L, int l, int which)
{
    if (l < 0 || l >= L) fail(SPK_ERR_ARG, "amg: level %d outside [0,%d)", l, L);
    if (which == SPK_AMG_COARSE_INV && l != L - 1) fail(SPK_ERR_ARG, "amg: the coarse inverse lives on level %d", L - 1);
    if (which < SPK_AMG_OP || which > SPK_AMG_COARSE_INV) fail(SPK_ERR_ARG, "amg: unknown matrix %d", which);
    if ((which == SPK_AMG_PROLONG || which == SPK_AMG_TENTATIVE) && l == L - 1) fail(SPK_ERR_ARG, "amg: the coarsest level has no prolongator");
}

void amg_check_opts(const spk_amg_opts &o, bool host_builder)
{
    if (o.max_levels < 1 || o.max_levels > SPK_AMG_MAX_LEVELS)
        fail(SPK_ERR_ARG, "amg: max_levels %d outside [1,%d]", o.max_levels, SPK_AMG_MAX_LEVELS);
    if (o.coarse_eq_limit < 1) fail(SPK_ERR_ARG, "amg: coarse_eq_limit %d < 1", o.coarse_eq_limit);
    if (o.nsmooths < 0 || o.nsmooths > 4) fail(SPK_ERR_ARG, "amg: nsmooths %d outside [0,4]", o.nsmooths);
    if (o.smoother != SPK_AMG_CHEBYSHEV && o.smoother != SPK_AMG_RICHARDSON) fail(SPK_ERR_ARG, "amg: unknown smoother %d", o.smoother);
    if (!(o.threshold >= 0.0) || !std::isfinite(o.threshold)) fail(SPK_ERR_ARG, "amg: threshold must be >= 0");
    if (o.smooth_its < 1 || o.smooth_its > 64) fail(SPK_ERR_ARG, "amg: smooth_its %d outside [1,64]", o.smooth_its);
    if (o.block_size < 0 || o.block_size > 3) fail(SPK_ERR_ARG, "amg: block_size %d outside [0,3]", o.block_size);
    for (double e : o.esteig)
        if (!std::isfinite(e)) fail(SPK_ERR_ARG, "amg: esteig factors must be finite");
    if (!(o.richardson_scale > 0.0) || !std::isfinite(o.richardson_scale)) fail(SPK_ERR_ARG, "amg: richardson_scale must be > 0");
    if (o.setup != SPK_AMG_SETUP_HOST && o.setup != SPK_AMG_SETUP_DEVICE)
        fail(SPK_ERR_ARG, "amg: setup %d is neither SPK_AMG_SETUP_HOST (0) nor SPK_AMG_SETUP_DEVICE (1)", o.setup);
    if (o.coarsening != SPK_AMG_COARSEN_AGGREGATION && o.coarsening != SPK_AMG_COARSEN_GRID)
        fail(SPK_ERR_ARG, "amg: coarsening %d is neither SPK_AMG_COARSEN_AGGREGATION (0) nor SPK_AMG_COARSEN_GRID (1)", o.coarsening);
    if (o.coarsening == SPK_AMG_COARSEN_GRID) {   // (grid, transfer, sides and galerkin are read under grid coarsening only)
        if (o.grid[0] < 2 || o.grid[1] < 2 || o.grid[2] < 1)
            fail(SPK_ERR_ARG, "amg: grid %d x %d x %d: at least 2 x 2 nodes (x 1 in 2-D)", o.grid[0], o.grid[1], o.grid[2]);
        if ((int64_t)o.grid[0] * o.grid[1] > INT32_MAX || (int64_t)o.grid[0] * o.grid[1] * o.grid[2] > INT32_MAX)
            fail(SPK_ERR_ARG, "amg: grid %d x %d x %d has more nodes than 32-bit rows address", o.grid[0], o.grid[1], o.grid[2]);
        if (o.transfer != SPK_AMG_TRANSFER_MATRIX_FREE && o.transfer != SPK_AMG_TRANSFER_STORED)
            fail(SPK_ERR_ARG, "amg: transfer %d is neither SPK_AMG_TRANSFER_MATRIX_FREE (0) nor SPK_AMG_TRANSFER_STORED (1)", o.transfer);
        if (o.sides != SPK_AMG_SIDES_ODD && o.sides != SPK_AMG_SIDES_ANY)
            fail(SPK_ERR_ARG, "amg: sides %d is neither SPK_AMG_SIDES_ODD (0) nor SPK_AMG_SIDES_ANY (1)", o.sides);
        if (o.galerkin != SPK_AMG_GALERKIN_PRODUCTS && o.galerkin != SPK_AMG_GALERKIN_STENCIL)
            fail(SPK_ERR_ARG, "amg: galerkin %d is neither SPK_AMG_GALERKIN_PRODUCTS (0) nor SPK_AMG_GALERKIN_STENCIL (1)", o.galerkin);
        if (o.transfer == SPK_AMG_TRANSFER_MATRIX_FREE && (o.grid[1] > 65535 || o.grid[2] > 65535))   // they are launch dimensions
            fail(SPK_ERR_UNSUPPORTED, "amg: the matrix-free transfers take at most 65535 nodes in y and z (grid %d x %d x %d) -- "
                 "use -spk_mg_transfer stored", o.grid[0], o.grid[1], o.grid[2]);
    }
    if (o.cycle != SPK_AMG_CYCLE_V && o.cycle != SPK_AMG_CYCLE_W)
        fail(SPK_ERR_ARG, "amg: cycle %d is neither SPK_AMG_CYCLE_V (0) nor SPK_AMG_CYCLE_W (1)", o.cycle);
    if (o.tail != SPK_AMG_TAIL_AUTO && o.tail != SPK_AMG_TAIL_LAUNCHES && o.tail != SPK_AMG_TAIL_FUSED)
        fail(SPK_ERR_ARG, "amg: tail %d is none of SPK_AMG_TAIL_AUTO (0), SPK_AMG_TAIL_LAUNCHES (1), SPK_AMG_TAIL_FUSED (2)", o.tail);
    if (o.tail_rows < 0) fail(SPK_ERR_ARG, "amg: tail_rows %d < 0 (0: the default of %d)", o.tail_rows, SPK_AMG_TAIL_ROWS_DEFAULT);
    if (o.op != SPK_AMG_OPERATOR_CSR && o.op != SPK_AMG_OPERATOR_STENCIL)
        fail(SPK_ERR_ARG, "amg: op %d is neither SPK_AMG_OPERATOR_CSR (0) nor SPK_AMG_OPERATOR_STENCIL (1)", o.op);
    if (o.op == SPK_AMG_OPERATOR_STENCIL && o.coarsening != SPK_AMG_COARSEN_GRID)
        fail(SPK_ERR_UNSUPPORTED, "amg: -spk_mg_operator stencil applies levels whose pattern is the grid stencil's closed form; "
             "smoothed aggregation (gamg) has none -- use -pc_type mg with -spk_mg_galerkin stencil, or -spk_mg_operator csr");
    if (o.op == SPK_AMG_OPERATOR_STENCIL && o.galerkin != SPK_AMG_GALERKIN_STENCIL)
        fail(SPK_ERR_UNSUPPORTED, "amg: -spk_mg_operator stencil applies levels whose pattern is the grid stencil's closed form; "
             "only -spk_mg_galerkin stencil guarantees it (the generic products keep whatever pattern they meet) -- pass "
             "-spk_mg_galerkin stencil, or -spk_mg_operator csr");
    if (o.lanczos != SPK_AMG_LANCZOS_STEPWISE && o.lanczos != SPK_AMG_LANCZOS_RESIDENT)
        fail(SPK_ERR_ARG, "amg: lanczos %d is neither SPK_AMG_LANCZOS_STEPWISE (0) nor SPK_AMG_LANCZOS_RESIDENT (1)", o.lanczos);
    if (!host_builder && o.lanczos == SPK_AMG_LANCZOS_RESIDENT && o.setup == SPK_AMG_SETUP_HOST)
        fail(SPK_ERR_UNSUPPORTED, "amg: -spk_amg_lanczos resident keeps the scalars of the device set-up's Lanczos on the device; the "
             "host set-up has no device Lanczos -- pass -spk_gamg_setup device, or -spk_amg_lanczos stepwise");
    if (o.precision != SPK_AMG_PRECISION_DOUBLE && o.precision != SPK_AMG_PRECISION_SINGLE)
        fail(SPK_ERR_ARG, "amg: precision %d is neither SPK_AMG_PRECISION_DOUBLE (0) nor SPK_AMG_PRECISION_SINGLE (1)", o.precision);
    if (host_builder || o.precision != SPK_AMG_PRECISION_SINGLE) return;   // (the host builder has no cycle: it does not read the field)
    const char *const what = "amg: -spk_mg_precision single runs the levels >= 1 in FP32 from their value arrays alone, with "
                             "matrix-free transfers";
    if (o.coarsening != SPK_AMG_COARSEN_GRID)
        fail(SPK_ERR_UNSUPPORTED, "%s; smoothed aggregation (gamg) has neither -- use grid coarsening (-pc_type mg) with -spk_mg_galerkin "
             "stencil -spk_mg_operator stencil, or -spk_mg_precision double", what);
    if (o.galerkin != SPK_AMG_GALERKIN_STENCIL)
        fail(SPK_ERR_UNSUPPORTED, "%s; the generic products keep whatever pattern they meet -- pass -spk_mg_galerkin stencil, or "
             "-spk_mg_precision double", what);
    if (o.op != SPK_AMG_OPERATOR_STENCIL)
        fail(SPK_ERR_UNSUPPORTED, "%s; the CSR kernels are FP64 only -- pass -spk_mg_operator stencil, or -spk_mg_precision double", what);
    if (o.transfer != SPK_AMG_TRANSFER_MATRIX_FREE)
        fail(SPK_ERR_UNSUPPORTED, "%s; the stored transfers are FP64 CSR matrices -- pass -spk_mg_transfer matrixfree, or "
             "-spk_mg_precision double", what);
}

void amg_build(AmgHier &h, HostCsr A, const spk_amg_opts &o)
{
    const auto t0 = Clock::now();
    amg_check_opts(o, true);   // (the host builder reads neither setup nor lanczos: it range-checks both)
    if (A.nrows != A.ncols || A.nrows <= 0) fail(SPK_ERR_ARG, "amg: the operator must be square and non-empty");
    std::vector<int32_t> perm;
    sort_rows(A, &perm);
    h = AmgHier{};
    h.o = o;
    h.perm = std::move(perm);
    h.lv.emplace_back();
    h.lv[0].A = std::move(A);
    h.lv[0].dinv = diag_inv(h.lv[0].A);
    h.dinv_sum = abs_sum(h.lv[0].dinv);
    HostRoute r{h};
    build_levels(r, o.block_size > 0 ? o.block_size : detect_bs(h.lv[0].A), o, SPK_AMG_SETUP_HOST, t0, h.info);
    fill_cycle_info(o, h.info);
}

void amg_refresh(AmgHier &h, const double *val)
{
    const auto t0 = Clock::now();
    if (h.lv.empty()) fail(SPK_ERR_STATE, "amg: no hierarchy to refresh (an earlier refresh failed)");
    AmgLevel &F = h.lv[0];
    for (size_t k = 0; k < F.A.v.size(); ++k) F.A.v[k] = val[(size_t)h.perm[k]];
    F.dinv = diag_inv(F.A);
    HostRoute r{h, binade_scale(h.dinv_sum, abs_sum(F.dinv))};
    try {
        refresh_levels(r, h.o, t0, h.info);
        fill_cycle_info(h.o, h.info);
    } catch (...) {   // half-refreshed: never to be read or applied
        h.lv.clear();
        h.cinv.clear();
        std::memset(&h.info, 0, sizeof h.info);
        throw;
    }
}

void AmgHier::level(int l, int which, const CsrOut &out) const
{
    check_level_query((int)lv.size(), l, which);
    const AmgLevel &V = lv[(size_t)l];
    if (which == SPK_AMG_COARSE_INV) coarse_inv_out(V.A.nrows, cinv.data(), out);
    else csr_out(which == SPK_AMG_OP ? V.A : which == SPK_AMG_PROLONG || o.coarsening == SPK_AMG_COARSEN_GRID ? V.P : V.Ptent, out);
}

}  // namespace spk

// ---------------------------------------------------------------------------
// host-only entry points (no GPU); a failure leaves its words where spk_last_error(NULL) reads them
// ---------------------------------------------------------------------------
extern "C" {

void spk_default_amg_opts(spk_amg_opts *o)
{
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->max_levels = 10;
    o->coarse_eq_limit = 50;
    o->nsmooths = 1;
    o->smoother = SPK_AMG_CHEBYSHEV;
    o->threshold = 0.0;
    o->smooth_its = 2;
    o->block_size = 0;
    o->esteig[0] = 0.0;
    o->esteig[1] = 0.1;
    o->esteig[2] = 0.0;
    o->esteig[3] = 1.1;
    o->richardson_scale = 1.0;
    o->setup = SPK_AMG_SETUP_HOST;
    o->lanczos = SPK_AMG_LANCZOS_STEPWISE;
    o->precision = SPK_AMG_PRECISION_DOUBLE;
}

#define SPK_HOST_TRY try {
#define SPK_HOST_CATCH                                                                   \
    }                                                                                    \
    catch (const spk::Error &e) { spk::set_create_error(e.msg); return e.code; }         \
    catch (const std::exception &e) { spk::set_create_error(e.what()); return SPK_ERR_NOMEM; } \
    return SPK_OK;

int spk_amg_build_host(int32_t n, const int32_t *rowptr, const int32_t *colidx, const double *val, const spk_amg_opts *o,
                       spk_amg_hier **out)
{
    if (!out || !rowptr || !colidx || !val || !o || n <= 0) return SPK_ERR_ARG;
    *out = nullptr;
    SPK_HOST_TRY
    spk::HostCsr A;
    A.nrows = A.ncols = n;
    A.rp.assign(rowptr, rowptr + n + 1);
    A.ci.assign(colidx, colidx + rowptr[n]);
    A.v.assign(val, val + rowptr[n]);
    for (int32_t c : A.ci)
        if (c < 0 || c >= n) spk::fail(SPK_ERR_ARG, "amg: column %d outside [0,%d)", (int)c, (int)n);
    auto h = std::make_unique<spk_amg_hier>();
    spk::amg_build(h->h, std::move(A), *o);
    *out = h.release();
    SPK_HOST_CATCH
}

int spk_amg_refresh_host(spk_amg_hier *h, const double *val)
{
    if (!h || !val) return SPK_ERR_ARG;
    SPK_HOST_TRY
    spk::amg_refresh(h->h, val);
    SPK_HOST_CATCH
}

int spk_amg_destroy_host(spk_amg_hier *h)
{
    delete h;
    return SPK_OK;
}

int spk_amg_host_info(const spk_amg_hier *h, spk_amg_info *info)
{
    if (!h || !info) return SPK_ERR_ARG;
    *info = h->h.info;
    return SPK_OK;
}

int spk_amg_host_level(const spk_amg_hier *h, int level, int which, int32_t *nrows, int32_t *ncols, int64_t *nnz,
                       int32_t *rowptr, int32_t *colidx, double *val)
{
    if (!h) return SPK_ERR_ARG;
    SPK_HOST_TRY
    h->h.level(level, which, {nrows, ncols, nnz, rowptr, colidx, val});
    SPK_HOST_CATCH
}

int spk_amg_host_aggregates(const spk_amg_hier *h, int level, int32_t *nnodes, int32_t *agg)
{
    if (!h) return SPK_ERR_ARG;
    SPK_HOST_TRY
    spk::aggregates_out(h->h.lv, h->h.info, level, nnodes, agg);
    SPK_HOST_CATCH
}

int spk_amg_stencil_children(const int32_t *fine, const int32_t *coarse, int32_t node, int32_t *n, int32_t *nodes, double *weights)
{
    if (!fine || !coarse || !n) return SPK_ERR_ARG;
    SPK_HOST_TRY
    for (int a = 0; a < 3; ++a)
        if (fine[a] < 1 || (coarse[a] != fine[a] && coarse[a] != fine[a] / 2 + 1))
            spk::fail(SPK_ERR_ARG, "amg: %d coarse nodes are not a coarsening of %d fine ones", (int)coarse[a], (int)fine[a]);
    if (node < 0 || (int64_t)node >= (int64_t)coarse[0] * coarse[1] * coarse[2]) spk::fail(SPK_ERR_ARG, "amg: coarse node %d outside the grid", (int)node);
    *n = spk::galerkin_stencil_children(fine, coarse, node, nodes, weights);
    SPK_HOST_CATCH
}

int spk_amg_cycle_steps(int32_t levels, int32_t cycle, int64_t *nsteps, int32_t *steps)
{
    if (!nsteps) return SPK_ERR_ARG;
    SPK_HOST_TRY
    const std::vector<spk::AmgStep> st = spk::amg_cycle_steps(levels, cycle);
    *nsteps = (int64_t)st.size();
    for (size_t i = 0; steps && i < st.size(); ++i) steps[2 * i] = st[i].kind, steps[2 * i + 1] = st[i].level;
    SPK_HOST_CATCH
}

}  // extern "C"
