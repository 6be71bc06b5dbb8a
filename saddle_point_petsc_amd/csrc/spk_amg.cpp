// spk_amg.cpp -- smoothed-aggregation algebraic multigrid (-pc_type gamg): the hierarchy, built at KSPSetUp from the
// A00 CSR on the host and uploaded (the default) or on the device (-spk_gamg_setup device: amg_build_device, kernels:
// spk_k_amg_setup.hip), and the V-cycle's launch sequence (kernels: spk_k_amg.hip).
//
// Every step is deterministic (fixed traversal orders, no hashing of pointers, a fixed Lanczos start vector): two
// builds of the same matrix give the same bytes, and so do two V-cycles.  DESIGN.md "Algebraic multigrid" has the
// algorithm and where it departs from PETSc's GAMG.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "spk_amg.hpp"
#include "spk_internal.hpp"

namespace spk {
void set_create_error(const std::string &m);   // spk_api.cpp: what spk_last_error(NULL) returns

namespace {

// columns sorted within each row (the caller's order is arbitrary)
void sort_rows(HostCsr &A)
{
    std::vector<std::pair<int32_t, double>> row;
    for (int32_t i = 0; i < A.nrows; ++i) {
        const int32_t k0 = A.rp[(size_t)i], k1 = A.rp[(size_t)i + 1];
        row.clear();
        for (int32_t k = k0; k < k1; ++k) row.emplace_back(A.ci[(size_t)k], A.v[(size_t)k]);
        std::sort(row.begin(), row.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
        for (int32_t k = k0; k < k1; ++k) {
            A.ci[(size_t)k] = row[(size_t)(k - k0)].first;
            A.v[(size_t)k] = row[(size_t)(k - k0)].second;
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

HostCsr transpose(const HostCsr &A)
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
HostCsr spgemm(const HostCsr &A, const HostCsr &B)
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
HostCsr add(double a, const HostCsr &A, double b, const HostCsr &B)
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
int sturm_count(const std::vector<double> &al, const std::vector<double> &be, double x)
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

// extreme Ritz values of D^-1 A after `steps` Lanczos steps on the similar D^-1/2 A D^-1/2, from a fixed start vector.
// Ritz values lie inside the spectrum: both estimates approach from within (lmax from below).
void lanczos(const HostCsr &A, const std::vector<double> &dinv, int steps, double *lmin, double *lmax)
{
    const int32_t n = A.nrows;
    std::vector<double> s((size_t)n), q((size_t)n), qp((size_t)n, 0.0), w((size_t)n), t((size_t)n);
    for (int32_t i = 0; i < n; ++i) s[(size_t)i] = std::sqrt(std::fabs(dinv[(size_t)i]));
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
    const int k = (int)std::min<int64_t>(steps, n);
    for (int j = 0; j < k; ++j) {
        for (int32_t i = 0; i < n; ++i) t[(size_t)i] = s[(size_t)i] * q[(size_t)i];
        double a = 0.0;
        for (int32_t i = 0; i < n; ++i) {
            double acc = 0.0;
            for (int32_t p = A.rp[(size_t)i]; p < A.rp[(size_t)i + 1]; ++p) acc += A.v[(size_t)p] * t[(size_t)A.ci[(size_t)p]];
            w[(size_t)i] = s[(size_t)i] * acc;
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
void node_graph(const HostCsr &A, int bs, double theta, std::vector<int32_t> &gp, std::vector<int32_t> &gi)
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
HostCsr tentative(const std::vector<int32_t> &agg, int32_t na, int bs)
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

// dense inverse of the SPD coarsest operator through Cholesky (symmetrised)
std::vector<double> coarse_inverse(const HostCsr &A)
{
    const int32_t n = A.nrows;
    std::vector<double> L((size_t)n * n, 0.0), X((size_t)n * n, 0.0);
    for (int32_t i = 0; i < n; ++i)
        for (int32_t k = A.rp[(size_t)i]; k < A.rp[(size_t)i + 1]; ++k) L[(size_t)i * n + A.ci[(size_t)k]] = A.v[(size_t)k];
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
    return X;
}

constexpr int kLanczosSteps = 30;

}  // namespace

void amg_check_opts(const spk_amg_opts &o)
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
}

void amg_build(AmgHier &h, HostCsr A, const spk_amg_opts &o)
{
    const auto t0 = std::chrono::steady_clock::now();
    amg_check_opts(o);
    if (A.nrows != A.ncols || A.nrows <= 0) fail(SPK_ERR_ARG, "amg: the operator must be square and non-empty");
    sort_rows(A);
    h = AmgHier{};
    h.o = o;
    h.bs = o.block_size > 0 ? o.block_size : detect_bs(A);
    if (A.nrows % h.bs) fail(SPK_ERR_ARG, "amg: block_size %d does not divide %d rows", h.bs, (int)A.nrows);
    h.lv.emplace_back();
    h.lv.back().A = std::move(A);
    for (;;) {
        const size_t l = h.lv.size() - 1;
        bool last = h.lv[l].A.nrows <= o.coarse_eq_limit || (int)h.lv.size() == o.max_levels;
        std::vector<int32_t> gp, gi, agg;
        int32_t na = 0;
        if (!last) {
            node_graph(h.lv[l].A, h.bs, o.threshold, gp, gi);
            na = aggregate(gp, gi, agg);
            last = na == 0 || (int64_t)na * h.bs >= h.lv[l].A.nrows;   // no coarsening left
        }
        if (last) break;
        AmgLevel &L = h.lv[l];
        L.agg = std::move(agg);
        L.dinv = diag_inv(L.A);
        lanczos(L.A, L.dinv, kLanczosSteps, &L.lmin, &L.lmax);
        L.lo = o.esteig[0] * L.lmin + o.esteig[1] * L.lmax;
        L.hi = o.esteig[2] * L.lmin + o.esteig[3] * L.lmax;
        if (o.smoother == SPK_AMG_CHEBYSHEV && !(L.lo > 0.0 && L.hi > L.lo))
            fail(SPK_ERR_ARG, "amg: Chebyshev interval [%g, %g] on level %d is empty or not positive (esteig)", L.lo, L.hi, (int)l);
        L.Ptent = tentative(L.agg, na, h.bs);
        L.P = L.Ptent;
        const double omega = 4.0 / (3.0 * L.lmax);
        for (int s = 0; s < o.nsmooths; ++s) {   // P = (I - omega D^-1 A) P
            HostCsr AP = spgemm(L.A, L.P);
            for (int32_t i = 0; i < AP.nrows; ++i)
                for (int32_t k = AP.rp[(size_t)i]; k < AP.rp[(size_t)i + 1]; ++k) AP.v[(size_t)k] *= L.dinv[(size_t)i];
            L.P = add(1.0, L.P, -omega, AP);
        }
        L.R = transpose(L.P);
        HostCsr Ac = spgemm(L.R, spgemm(L.A, L.P));
        Ac = add(0.5, Ac, 0.5, transpose(Ac));   // exactly symmetric (the products agree to rounding)
        h.lv.emplace_back();
        h.lv.back().A = std::move(Ac);
    }
    AmgLevel &C = h.lv.back();
    if (C.A.nrows > SPK_AMG_MAX_COARSE)
        fail(SPK_ERR_UNSUPPORTED, "amg: the coarsest level keeps %d equations after %d levels; the dense coarse solve takes at "
             "most %d -- raise -pc_mg_levels or -pc_gamg_threshold 0", (int)C.A.nrows, (int)h.lv.size(), SPK_AMG_MAX_COARSE);
    C.dinv = diag_inv(C.A);
    h.cinv = coarse_inverse(C.A);
    h.setup_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

void AmgHier::info(spk_amg_info *out) const
{
    std::memset(out, 0, sizeof *out);
    out->levels = (int32_t)lv.size();
    out->block_size = bs;
    double tot = 0.0;
    for (size_t l = 0; l < lv.size(); ++l) {
        out->rows[l] = lv[l].A.nrows;
        out->nnz[l] = lv[l].A.nnz();
        out->lambda_max[l] = lv[l].lmax;
        tot += (double)lv[l].A.nnz();
    }
    out->operator_complexity = tot / (double)std::max<int64_t>(lv[0].A.nnz(), 1);
    out->setup_seconds = setup_seconds;
}

void AmgHier::level(int l, int which, int32_t *nrows, int32_t *ncols, int64_t *nnz, int32_t *rowptr, int32_t *colidx,
                    double *val) const
{
    const int L = (int)lv.size();
    if (l < 0 || l >= L) fail(SPK_ERR_ARG, "amg: level %d outside [0,%d)", l, L);
    if (which == SPK_AMG_COARSE_INV) {
        if (l != L - 1) fail(SPK_ERR_ARG, "amg: the coarse inverse lives on level %d", L - 1);
        const int32_t n = lv[(size_t)l].A.nrows;
        if (nrows) *nrows = n;
        if (ncols) *ncols = n;
        if (nnz) *nnz = (int64_t)n * n;
        for (int32_t i = 0; rowptr && i <= n; ++i) rowptr[i] = i * n;
        for (int64_t k = 0; colidx && k < (int64_t)n * n; ++k) colidx[k] = (int32_t)(k % n);
        if (val) std::memcpy(val, cinv.data(), sizeof(double) * cinv.size());
        return;
    }
    const HostCsr *M = which == SPK_AMG_OP ? &lv[(size_t)l].A : which == SPK_AMG_PROLONG ? &lv[(size_t)l].P
                     : which == SPK_AMG_TENTATIVE ? &lv[(size_t)l].Ptent : nullptr;
    if (!M) fail(SPK_ERR_ARG, "amg: unknown matrix %d", which);
    if (which != SPK_AMG_OP && l == L - 1) fail(SPK_ERR_ARG, "amg: the coarsest level has no prolongator");
    if (nrows) *nrows = M->nrows;
    if (ncols) *ncols = M->ncols;
    if (nnz) *nnz = M->nnz();
    if (rowptr) std::memcpy(rowptr, M->rp.data(), sizeof(int32_t) * M->rp.size());
    if (colidx && M->nnz()) std::memcpy(colidx, M->ci.data(), sizeof(int32_t) * M->ci.size());
    if (val && M->nnz()) std::memcpy(val, M->v.data(), sizeof(double) * M->v.size());
}

}  // namespace spk

// ---------------------------------------------------------------------------
// the context's hierarchy: built from its A00 (single rank: the diagonal block is all of A), uploaded, applied
// ---------------------------------------------------------------------------
namespace spk {

std::unique_ptr<spk_amg_hier> amg_build_ctx(spk_ctx *c)
{
    const int32_t n = c->n_local;
    HostCsr A;
    A.nrows = A.ncols = n;
    A.rp.resize((size_t)n + 1);
    SPK_HIP(hipMemcpy(A.rp.data(), c->Ad.rowptr.p, sizeof(int32_t) * A.rp.size(), hipMemcpyDeviceToHost));
    A.ci.resize((size_t)A.rp[(size_t)n]);
    A.v.resize(A.ci.size());
    if (!A.ci.empty()) {
        SPK_HIP(hipMemcpy(A.ci.data(), c->Ad.colidx.p, sizeof(int32_t) * A.ci.size(), hipMemcpyDeviceToHost));
        SPK_HIP(hipMemcpy(A.v.data(), c->Ad.val.p, sizeof(double) * A.v.size(), hipMemcpyDeviceToHost));
    }
    spk_amg_opts o = c->amg_opts;
    if (o.block_size == 0 && c->Adict.ok) o.block_size = c->Adict.bs;   // the blocking the context found
    else if (o.block_size == 0 && c->spmv_format == 1) o.block_size = 2;
    else if (o.block_size == 0 && c->spmv_format == 2) o.block_size = 3;
    auto h = std::make_unique<spk_amg_hier>();
    amg_build(h->h, std::move(A), o);
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

// the smoothing steps of a level from its Chebyshev interval [lo, hi]
static void smoother_coeffs(AmgLevelDev &D, const spk_amg_opts &o, double lo, double hi)
{
    const int nu = o.smooth_its;
    D.alpha.assign((size_t)nu, o.richardson_scale);
    D.beta.assign((size_t)nu, 0.0);
    if (o.smoother == SPK_AMG_CHEBYSHEV) {   // Saad, Alg. 12.1: d_k = rho_k rho_{k-1} d_{k-1} + 2 rho_k / delta D^-1 r_k
        const double theta = 0.5 * (hi + lo), delta = 0.5 * (hi - lo), sigma = theta / delta;
        double rho = 1.0 / sigma;
        D.alpha[0] = 1.0 / theta;
        for (int k = 1; k < nu; ++k) {
            const double rn = 1.0 / (2.0 * sigma - rho);
            D.alpha[(size_t)k] = 2.0 * rn / delta;
            D.beta[(size_t)k] = rn * rho;
            rho = rn;
        }
    }
}

void amg_upload(spk_ctx *c, std::unique_ptr<spk_amg_hier> hp)
{
    const auto t0 = std::chrono::steady_clock::now();
    const AmgHier &h = hp->h;
    auto d = std::make_unique<AmgDev>();
    const size_t L = h.lv.size();
    std::vector<AmgLevelDev>(L).swap(d->lv);   // (the levels own device buffers: constructed in place, never moved)
    for (size_t l = 0; l < L; ++l) {
        const AmgLevel &H = h.lv[l];
        AmgLevelDev &D = d->lv[l];
        D.n = H.A.nrows;
        const size_t nv = l == 0 ? (size_t)c->ld : (size_t)D.n;   // the fine level's vectors as the layouts' products want them
        if (l > 0) {
            upload_host_csr(D.A, H.A);
            D.dinv.upload(H.dinv.data(), H.dinv.size(), 8);
            D.b.alloc(nv, 8);
        }
        D.ya.alloc(nv, 16);
        D.yb.alloc(nv, 16);
        if (l + 1 == L) break;
        if (l == 0) D.t.alloc(nv, 16);
        upload_host_csr(D.P, H.P);
        upload_host_csr(D.R, H.R);
        smoother_coeffs(D, h.o, H.lo, H.hi);
    }
    d->cinv.upload(h.cinv.data(), h.cinv.size());
    SPK_HIP(hipDeviceSynchronize());
    hp->h.setup_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    c->amg_d = std::move(d);
    c->amg_h = std::move(hp);
}

// ---------------------------------------------------------------------------
// the same hierarchy built on the device (-spk_gamg_setup device; kernels: spk_k_amg_setup.hip).  Per level: node graph
// -> host (the greedy aggregation is sequential by definition and runs unchanged, so the aggregates and every pattern
// are the host build's) -> tentative prolongator, Lanczos, the products and transposes as kernels.  Only the graph,
// the aggregates, the Lanczos scalars and the coarsest operator cross the bus.
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

HostCsr dev_csr_download(const CsrDev &A, bool values, hipStream_t s)
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

// the 30 Lanczos steps of `lanczos` with the level's own product (level 0: the context's layout, else the CSR kernel);
// the two sums of a step come back to the host, which keeps the tridiagonal and the break rule
void dev_lanczos(spk_ctx *c, const CsrDev *A, int32_t n, int64_t nv, const double *dinv, int steps, double *lmin, double *lmax)
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
        return h;
    };
    k::amgs_lz_init(n, dinv, sv.p, q.p, f, s);
    const double nq = std::sqrt(sum());
    k::amgs_lz_scale(n, nq, q.p, sv.p, q.p, t.p, s);
    std::vector<double> al, be{0.0};
    const int kk = (int)std::min<int64_t>(steps, n);
    double *qc = q.p, *qo = qp.p;
    for (int j = 0; j < kk; ++j) {
        if (A) k::amg_spmv(*A, t.p, aw.p, nullptr, s);
        else a_mult(c, t.p, aw.p, nullptr, nullptr, nullptr, false, nullptr);
        k::amgs_lz_dot(n, sv.p, aw.p, w.p, qc, f, s);
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
    ritz_extremes(al, be, lmin, lmax);
}

}  // namespace

std::unique_ptr<AmgDev> amg_build_device(spk_ctx *c)
{
    const auto t0 = std::chrono::steady_clock::now();
    spk_amg_opts o = c->amg_opts;
    amg_check_opts(o);
    hipStream_t s = c->stream;
    c->ensure_scratch();
    const int32_t n0 = c->n_local;
    if (n0 <= 0) fail(SPK_ERR_ARG, "amg: the operator must be square and non-empty");
    const int64_t ld = ((int64_t)c->n_local + c->m + 255) / 256 * 256;   // as ensure_vectors pads the context's vectors

    // sorted columns: the context's CSR as it is when every row ascends, else a sorted copy
    CsrDev A0s;
    const CsrDev *A0 = &c->Ad;
    {
        DevBuf<int32_t> flag;
        flag.alloc(1);
        k::amgs_rows_sorted(c->Ad.rowptr.p, c->Ad.colidx.p, n0, flag.p, s);
        int32_t unsorted = 0;
        SPK_HIP(hipMemcpyAsync(&unsorted, flag.p, sizeof unsorted, hipMemcpyDeviceToHost, s));
        SPK_HIP(hipStreamSynchronize(s));
        if (unsorted) {
            dev_csr_copy(A0s, c->Ad, s);
            k::amgs_sort_rows(A0s.rowptr.p, A0s.colidx.p, A0s.val.p, n0, s);
            A0 = &A0s;
        }
    }
    if (o.block_size == 0 && c->Adict.ok) o.block_size = c->Adict.bs;   // the blocking the context found
    else if (o.block_size == 0 && c->spmv_format == 1) o.block_size = 2;
    else if (o.block_size == 0 && c->spmv_format == 2) o.block_size = 3;
    const int bs = o.block_size > 0 ? o.block_size : detect_bs(dev_csr_download(*A0, false, s));
    if (n0 % bs) fail(SPK_ERR_ARG, "amg: block_size %d does not divide %d rows", bs, (int)n0);

    auto d = std::make_unique<AmgDev>();
    d->device_built = true;
    spk_amg_info &info = d->info;
    std::memset(&info, 0, sizeof info);
    d->lv.reserve((size_t)o.max_levels);
    d->lv.emplace_back();
    d->lv[0].n = n0;
    DevBuf<double> dinv0;   // diag(A_0)^-1 as pc_setup computes it into the context afterwards
    dinv0.alloc((size_t)n0, 8);
    k::extract_diag_inv(c->Ad, dinv0.p, s);
    info.rows[0] = n0;
    info.nnz[0] = A0->nnz;
    for (;;) {
        const size_t l = d->lv.size() - 1;
        const CsrDev &A = l == 0 ? *A0 : d->lv[l].A;
        const int32_t n = A.nrows, nn = n / bs;
        bool last = n <= o.coarse_eq_limit || (int)d->lv.size() == o.max_levels;
        std::vector<int32_t> gp, gi, agg;
        int32_t na = 0;
        if (!last) {   // the node graph: norms of the diagonal blocks, count, scan, fill; then to the host
            DevBuf<double> dn;
            DevBuf<int32_t> cnt, gpd, gid;
            dn.alloc_raw((size_t)nn, 8);
            cnt.alloc_raw((size_t)nn, 8);
            gpd.alloc_raw((size_t)nn + 1, 8);
            k::amgs_node_norms(A.rowptr.p, A.colidx.p, A.val.p, nn, bs, dn.p, s);
            k::amgs_graph(A.rowptr.p, A.colidx.p, A.val.p, nn, bs, o.threshold, dn.p, nullptr, cnt.p, s);
            const int32_t ne = scan_counts(cnt.p, nn, gpd.p, s);
            gid.alloc_raw((size_t)ne, 8);
            k::amgs_graph(A.rowptr.p, A.colidx.p, A.val.p, nn, bs, o.threshold, dn.p, gpd.p, gid.p, s);
            gp.resize((size_t)nn + 1);
            gi.resize((size_t)ne);
            SPK_HIP(hipMemcpyAsync(gp.data(), gpd.p, sizeof(int32_t) * gp.size(), hipMemcpyDeviceToHost, s));
            if (ne) SPK_HIP(hipMemcpyAsync(gi.data(), gid.p, sizeof(int32_t) * gi.size(), hipMemcpyDeviceToHost, s));
            SPK_HIP(hipStreamSynchronize(s));
            na = aggregate(gp, gi, agg);
            last = na == 0 || (int64_t)na * bs >= n;   // no coarsening left
        }
        if (last) break;
        AmgLevelDev &L = d->lv[l];
        const double *dinv = l == 0 ? dinv0.p : L.dinv.p;
        double lmin = 0.0, lmax = 0.0;
        dev_lanczos(c, l == 0 ? nullptr : &A, n, l == 0 ? ld : (int64_t)n, dinv, kLanczosSteps, &lmin, &lmax);
        info.lambda_max[l] = lmax;
        const double lo = o.esteig[0] * lmin + o.esteig[1] * lmax, hi = o.esteig[2] * lmin + o.esteig[3] * lmax;
        if (o.smoother == SPK_AMG_CHEBYSHEV && !(lo > 0.0 && hi > lo))
            fail(SPK_ERR_ARG, "amg: Chebyshev interval [%g, %g] on level %d is empty or not positive (esteig)", lo, hi, (int)l);
        smoother_coeffs(L, o, lo, hi);
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
        const double omega = 4.0 / (3.0 * lmax);
        for (int it = 0; it < o.nsmooths; ++it) {   // P = (I - omega D^-1 A) P
            CsrDev AP, Pn;
            dev_spgemm(AP, A, L.P, s);
            dev_add(Pn, 1.0, L.P, -omega, AP, dinv, s);
            L.P = std::move(Pn);
        }
        dev_transpose(L.R, L.P, s);
        CsrDev Acs;
        {
            CsrDev AP, Ac, AcT;
            dev_spgemm(AP, A, L.P, s);
            dev_spgemm(Ac, L.R, AP, s);
            dev_transpose(AcT, Ac, s);
            dev_add(Acs, 0.5, Ac, 0.5, AcT, nullptr, s);   // exactly symmetric (the products agree to rounding)
        }
        d->lv.emplace_back();   // (reserved: the levels never move)
        AmgLevelDev &N = d->lv.back();
        N.A = std::move(Acs);
        N.n = N.A.nrows;
        N.dinv.alloc((size_t)N.n, 8);
        k::extract_diag_inv(N.A, N.dinv.p, s);
        info.rows[l + 1] = N.n;
        info.nnz[l + 1] = N.A.nnz;
    }
    const size_t L = d->lv.size();
    const CsrDev &AC = L == 1 ? *A0 : d->lv[L - 1].A;
    if (AC.nrows > SPK_AMG_MAX_COARSE)
        fail(SPK_ERR_UNSUPPORTED, "amg: the coarsest level keeps %d equations after %d levels; the dense coarse solve takes at "
             "most %d -- raise -pc_mg_levels or -pc_gamg_threshold 0", (int)AC.nrows, (int)L, SPK_AMG_MAX_COARSE);
    {
        const std::vector<double> cinv = coarse_inverse(dev_csr_download(AC, true, s));
        d->cinv.upload(cinv.data(), cinv.size());
    }
    for (size_t l = 0; l < L; ++l) {   // the V-cycle's vectors, as amg_upload sizes them
        AmgLevelDev &D = d->lv[l];
        const size_t nv = l == 0 ? (size_t)ld : (size_t)D.n;
        if (l > 0) D.b.alloc(nv, 8);
        D.ya.alloc(nv, 16);
        D.yb.alloc(nv, 16);
        if (l == 0 && L > 1) D.t.alloc(nv, 16);
    }
    info.levels = (int32_t)L;
    info.block_size = bs;
    double tot = 0.0;
    for (size_t l = 0; l < L; ++l) tot += (double)info.nnz[l];
    info.operator_complexity = tot / (double)std::max<int64_t>(info.nnz[0], 1);
    info.setup = SPK_AMG_SETUP_DEVICE;
    SPK_HIP(hipDeviceSynchronize());
    info.setup_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return d;
}

void amg_dev_level(spk_ctx *c, int l, int which, int32_t *nrows, int32_t *ncols, int64_t *nnz, int32_t *rowptr, int32_t *colidx,
                   double *val)
{
    const AmgDev &d = *c->amg_d;
    const int L = (int)d.lv.size();
    hipStream_t s = c->stream;
    if (l < 0 || l >= L) fail(SPK_ERR_ARG, "amg: level %d outside [0,%d)", l, L);
    if (which == SPK_AMG_COARSE_INV) {
        if (l != L - 1) fail(SPK_ERR_ARG, "amg: the coarse inverse lives on level %d", L - 1);
        const int32_t n = d.lv[(size_t)l].n;
        if (nrows) *nrows = n;
        if (ncols) *ncols = n;
        if (nnz) *nnz = (int64_t)n * n;
        for (int32_t i = 0; rowptr && i <= n; ++i) rowptr[i] = i * n;
        for (int64_t k = 0; colidx && k < (int64_t)n * n; ++k) colidx[k] = (int32_t)(k % n);
        if (val) SPK_HIP(hipMemcpy(val, d.cinv.p, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost));
        return;
    }
    if (which != SPK_AMG_OP && which != SPK_AMG_PROLONG && which != SPK_AMG_TENTATIVE) fail(SPK_ERR_ARG, "amg: unknown matrix %d", which);
    if (which != SPK_AMG_OP && l == L - 1) fail(SPK_ERR_ARG, "amg: the coarsest level has no prolongator");
    const CsrDev &M = which == SPK_AMG_OP ? (l == 0 ? c->Ad : d.lv[(size_t)l].A)
                    : which == SPK_AMG_PROLONG ? d.lv[(size_t)l].P : d.lv[(size_t)l].Ptent;
    if (nrows) *nrows = M.nrows;
    if (ncols) *ncols = M.ncols;
    if (nnz) *nnz = M.nnz;
    if (!rowptr && !colidx && !val) return;
    HostCsr H = dev_csr_download(M, true, s);
    if (which == SPK_AMG_OP && l == 0) sort_rows(H);   // the context's CSR keeps the caller's order
    if (rowptr) std::memcpy(rowptr, H.rp.data(), sizeof(int32_t) * H.rp.size());
    if (colidx && H.nnz()) std::memcpy(colidx, H.ci.data(), sizeof(int32_t) * H.ci.size());
    if (val && H.nnz()) std::memcpy(val, H.v.data(), sizeof(double) * H.v.size());
}

void amg_dev_aggregates(spk_ctx *c, int l, int32_t *nnodes, int32_t *agg)
{
    const AmgDev &d = *c->amg_d;
    if (l < 0 || l + 1 >= (int)d.lv.size()) fail(SPK_ERR_ARG, "amg: level %d has no aggregates", l);
    const auto &a = d.lv[(size_t)l].agg;
    if (nnodes) *nnodes = (int32_t)a.size();
    if (agg) std::memcpy(agg, a.data(), sizeof(int32_t) * a.size());
}

// the fine level's product runs in the row-type 2x2 layout (what a_mult takes for it) on one rank
// (n_local % 2: never false here -- the 2x2 blocked copy the row types are built over exists only for an even n_local;
// the condition states what amg_cheb_dict2 needs rather than guarding a case that occurs)
static bool fused_fine(const spk_ctx *c)
{
    return c->spmv_format != 0 && c->Adict.ok && c->Adict.bs == 2 && c->n_ghost == 0 && c->n_local % 2 == 0;
}

// nu smoothing steps on level l from *y (nullptr: the zero guess); returns the buffer holding the result
static double *smooth(spk_ctx *c, AmgLevelDev &D, int l, const double *b, double *y, const int32_t *done)
{
    hipStream_t s = c->stream;
    const double *dinv = l == 0 ? c->dinv.p : D.dinv.p;
    const double *prev = nullptr;   // the iterate before y (nullptr: zero)
    for (size_t k = 0; k < D.alpha.size(); ++k) {
        double *dst = y == D.ya.p ? D.yb.p : D.ya.p;   // may be `prev`: each entry is read before it is written
        if (l == 0 && y && fused_fine(c)) {   // the 2x2 row-type layout: product and step in one pass
            k::amg_cheb_dict2(c->Adict, dinv, b, y, prev, dst, D.alpha[k], D.beta[k], done, s);
        } else if (l == 0) {                   // other layouts: the layout's own product, then a vector pass
            if (y) a_mult(c, y, D.t.p, nullptr, nullptr, done, false, nullptr);
            k::amg_cheb_vec(D.n, dinv, b, D.t.p, y, prev, dst, D.alpha[k], D.beta[k], done, s);
        } else if (y) {
            k::amg_cheb_csr(D.A, dinv, b, y, prev, dst, D.alpha[k], D.beta[k], done, s);
        } else {
            k::amg_cheb_vec(D.n, dinv, b, nullptr, nullptr, nullptr, dst, D.alpha[k], 0.0, done, s);
        }
        prev = y;
        y = dst;
    }
    return y;
}

void amg_apply(spk_ctx *c, const double *x, double *y, int mode, const int32_t *done)
{
    hipStream_t s = c->stream;
    AmgDev &d = *c->amg_d;
    const size_t L = d.lv.size();
    std::vector<double *> cur(L, nullptr);
    auto rhs = [&](size_t l) -> const double * { return l == 0 ? x : d.lv[l].b.p; };
    for (size_t l = 0; l + 1 < L; ++l) {   // down: pre-smoothing, residual, restriction
        AmgLevelDev &D = d.lv[l];
        cur[l] = smooth(c, D, (int)l, rhs(l), nullptr, done);
        if (l == 0) a_mult(c, cur[l], D.t.p, nullptr, nullptr, done, false, nullptr);
        else k::amg_spmv(D.A, cur[l], D.ya.p == cur[l] ? D.yb.p : D.ya.p, done, s);
        const double *t = l == 0 ? D.t.p : (D.ya.p == cur[l] ? D.yb.p : D.ya.p);
        k::amg_restrict(D.R, rhs(l), t, d.lv[l + 1].b.p, done, s);
    }
    AmgLevelDev &C = d.lv[L - 1];   // exact coarse solve
    k::amg_dense(d.cinv.p, C.n, rhs(L - 1), C.ya.p, done, s);
    cur[L - 1] = C.ya.p;
    for (size_t l = L - 1; l-- > 0;) {   // up: prolongation + correction, post-smoothing
        AmgLevelDev &D = d.lv[l];
        k::amg_prolong_add(D.P, cur[l + 1], cur[l], done, s);
        cur[l] = smooth(c, D, (int)l, rhs(l), cur[l], done);
    }
    k::amg_out(mode, c->n_local, cur[0], y, done, s);
}

}  // namespace spk

// ---------------------------------------------------------------------------
// host-only entry points (no GPU)
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

int spk_amg_destroy_host(spk_amg_hier *h)
{
    delete h;
    return SPK_OK;
}

int spk_amg_host_info(const spk_amg_hier *h, spk_amg_info *info)
{
    if (!h || !info) return SPK_ERR_ARG;
    h->h.info(info);
    return SPK_OK;
}

int spk_amg_host_level(const spk_amg_hier *h, int level, int which, int32_t *nrows, int32_t *ncols, int64_t *nnz,
                       int32_t *rowptr, int32_t *colidx, double *val)
{
    if (!h) return SPK_ERR_ARG;
    SPK_HOST_TRY
    h->h.level(level, which, nrows, ncols, nnz, rowptr, colidx, val);
    SPK_HOST_CATCH
}

int spk_amg_host_aggregates(const spk_amg_hier *h, int level, int32_t *nnodes, int32_t *agg)
{
    if (!h) return SPK_ERR_ARG;
    SPK_HOST_TRY
    if (level < 0 || level + 1 >= (int)h->h.lv.size()) spk::fail(SPK_ERR_ARG, "amg: level %d has no aggregates", level);
    const auto &a = h->h.lv[(size_t)level].agg;
    if (nnodes) *nnodes = (int32_t)a.size();
    if (agg) std::memcpy(agg, a.data(), sizeof(int32_t) * a.size());
    SPK_HOST_CATCH
}

}  // extern "C"
