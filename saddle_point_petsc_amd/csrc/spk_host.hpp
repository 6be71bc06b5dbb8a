// spk_host.hpp -- the host-pure half of the set-up: errors, host arrays, the row-slab split and every step of
// KSPSetOperators that is arithmetic on small integer arrays (spk_host.cpp).  Standard library and include/spk.h only:
// no HIP type, no device pointer, no getenv -- spk_operator.cpp reads the switches and owns the device half.
// Exercised without a GPU by tests/host/setup_host_check.cpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../include/spk.h"

namespace spk {

struct Error {
    int code;
    std::string msg;
};
[[noreturn]] void fail(int code, const char *fmt, ...);
// the words of a failure that has no context to keep them (spk_create, the host-only entry points), per thread: what
// spk_last_error(NULL) returns
void set_create_error(const std::string &m);
const char *create_error();

// uninitialised host array (std::vector would zero hundreds of MB on one thread first)
template <class T>
struct HostBuf {
    std::unique_ptr<T[]> p;
    size_t n = 0;
    void alloc(size_t count)
    {
        p.reset(new T[count ? count : 1]);
        n = count;
    }
    T *data() { return p.get(); }
    const T *data() const { return p.get(); }
    size_t size() const { return n; }
    T &operator[](size_t i) { return p[i]; }
    const T &operator[](size_t i) const { return p[i]; }
};
// fn(begin, end, thread) over [0, n) on up to `hardware threads` host threads
void parallel_for(int64_t n, const std::function<void(int64_t, int64_t, int)> &fn, int max_threads = 0);

struct SplitCsr {
    HostBuf<int32_t> d_rowptr, d_colidx, o_rowptr, o_colidx;
    HostBuf<double> d_val, o_val;
    std::vector<int32_t> garray;
    bool bad_column = false;  // a column outside [0, ncols_global)
    int32_t bad_value = 0;
};
void split_csr(int64_t row_begin, int32_t nrows_local, const int32_t *rowptr,
               const int32_t *colidx, const double *val, SplitCsr &out, int64_t ncols_global = -1);

// ---- row types + deviation codes (DictDev, spk_internal.hpp): the arithmetic between the device rounds ----
constexpr int kDictMaxK = 32;      // blocks per block row
namespace k { constexpr int kDictAcrossHost = 1 << 30; }   // = kDictAcross (spk_dict.hpp, device side)
struct DictRefusal {               // why == nullptr: accepted; else the words and numbers of the verbose line
    const char *why = nullptr;
    long a = 0, b = 0;
};
// the "one layout for all classes" part of DictDev, as dict_field_layout finds it
struct DictLayout {
    bool uniform = false, straddle = false;
    int uniform3 = 0;
    int32_t uw[4] = {1, 1, 1, 1}, u3l[9] = {}, u3r[9] = {};
};
// classes numbered by their first member: slot2id[slot] = number or -1, reps[number] = first member
void dict_number_classes(const unsigned long long *keys, const int32_t *rep, int nslots, int32_t *slot2id, std::vector<int32_t> &reps);
// (granule exponent, largest deviation as the bits of a double) of `count` class entries -> two's-complement width and scale
DictRefusal dict_field_widths(int count, const int32_t *gexp, const unsigned long long *dmax, int *width, double *scale);
// fld: (ncls + 1) x bs*bs, all written (the null class last); cls: the scale halves cls[2 i + 1] of the ncls found classes
DictRefusal dict_field_layout(int bs, int ncls, const int *width, const double *scale, bool allow_uniform, int32_t *fld, double *cls,
                              DictLayout &L);
int64_t dict_plane_offsets(int bs, int kmax, int32_t nbrows, int64_t skew, int64_t plane_off[kDictMaxK]);   // returns the total
int dict_tab_ints(int ntype, int kmax);
int dict_lds_bytes(int ntype, int kmax, int ncls, int bs);

// ---- A00: ghosts and the halo plan ----
void ghost_list(std::vector<int32_t> &cols);   // global columns, any order, repeated -> sorted and unique (garray)
inline int32_t ghost_number(const std::vector<int32_t> &garray, int32_t g)
{
    return (int32_t)(std::lower_bound(garray.begin(), garray.end(), g) - garray.begin());
}
void ghost_renumber(const std::vector<int32_t> &garray, int32_t *cols, size_t n);
// orp: off-rank row pointers over n rows (nullptr: none) -> the rows that have entries and their row pointers
void compress_offrank_rows(const int32_t *orp, int32_t n, std::vector<int32_t> &rows, std::vector<int32_t> &corp);
struct HaloPlan {
    std::vector<int> peers;
    std::vector<int64_t> send_off{0}, recv_off{0};   // per peer offsets (+ total at end)
    std::vector<int32_t> send_idx;                   // local rows, in each peer's ghost order
};
// slabs: [begin, end) of every rank; ghosts[p]: rank p's garray as bytes (host_allgatherv)
void halo_plan(int me, int P, const int64_t *slabs, const std::vector<int32_t> &garray, const std::vector<std::vector<char>> &ghosts,
               HaloPlan &out);
struct HostSendRanges {
    int n = 0;   // 0: some peer's rows are not contiguous, no peer, or more than 4
    int32_t r0[4] = {}, len[4] = {}, off[4] = {};
};
HostSendRanges send_ranges(const HaloPlan &h);

// ---- A10: the constraint block ----
// col / v (rowptr[m] entries, the caller's): local columns ascending inside each row (stable), values with them
void localise_and_sort(int32_t m, const int32_t *rowptr, const int32_t *colidx, const double *val, int64_t lo, int64_t hi,
                       int32_t *col, double *v);
std::vector<int32_t> wide_rows(int32_t m, const int32_t *rowptr, int32_t threshold);
int32_t window_width(int32_t nl, int max_blocks);
// winptr[w * mw + r], w = 0..nwin: start of window w in row r of the concatenated wide rows (wrp: their row pointers)
void window_pointers(int32_t mw, const int32_t *wrp, const int32_t *wcol, int32_t nl, int32_t win, int32_t nwin, int32_t *winptr);
// rows of (rowptr, col, v) concatenated: the listed ones (rp over them), or all m with the listed ones left empty
void gather_rows(int32_t m, const int32_t *rowptr, const int32_t *col, const double *v, const std::vector<int32_t> &rows, bool complement,
                 std::vector<int32_t> &rp, std::vector<int32_t> &ci, std::vector<double> &cv);
// B^T by rows (nl x m), entries of a row ordered by constraint index; trp: nl + 1 zeros on entry
void transpose_rows(int32_t m, int32_t nl, const int32_t *rowptr, const int32_t *col, const double *v, int32_t *trp, int32_t *tci,
                    double *tv, int max_threads = 0);

// ---- the order of one multigrid cycle and the fused tail (spk_amg_opts.cycle / tail / tail_rows) ----
// One source for both routes: the launches walk this list and the tail kernel interprets its share of it.
struct AmgStep { int32_t kind, level; };   // kind: SPK_AMG_STEP_*
// cycle(0, fresh) of include/spk.h over L levels (L >= 1; L == 1: the coarse solve alone)
std::vector<AmgStep> amg_cycle_steps(int levels, int cycle);
// SPK_AMG_TAIL_AUTO resolved: LAUNCHES under V, FUSED under W
int amg_resolve_tail(int cycle, int tail);
// the smallest t >= 1 such that every level l >= t has rows[l] <= tail_rows (0: SPK_AMG_TAIL_ROWS_DEFAULT); -1 when the
// coarsest level exceeds it, with one level, or when `tail` resolves to LAUNCHES.  Level 0 is never in the tail.
int amg_tail_first(int levels, const int32_t *rows, int cycle, int tail, int tail_rows);
// the tail runs of a step list: maximal stretches [begin, end) of consecutive steps on levels >= tail_first (none for -1)
std::vector<std::pair<int64_t, int64_t>> amg_tail_runs(const std::vector<AmgStep> &steps, int tail_first);
// Where the iterate lies: of a level's two buffers (0: ya, 1: yb), the one that holds its iterate when a step begins --
// sel[i] for the level of step i, sel_next[i] for the level below it (0 on the coarsest) -- and run_sel[r], where tail run
// r leaves the iterate of level tail_first.  The rule is that of the launches (smooth(), spk_amg_cycle.cpp): each of
// the nu smoothing steps writes the buffer its input is not in, a fresh start (PRE0) writes ya first, the coarse solve
// writes ya, DOWN and UP leave the iterate where it is.  The fused tail kernel reads this; the launches follow the rule.
struct AmgBuffers { std::vector<int32_t> sel, sel_next, run_sel; };
AmgBuffers amg_cycle_buffers(const std::vector<AmgStep> &steps, const std::vector<std::pair<int64_t, int64_t>> &runs, int levels,
                             int nu, int tail_first);

// ---- the grid-stencil Galerkin product (SPK_AMG_GALERKIN_STENCIL; spk_galerkin_host.cpp over spk_galerkin_core.hpp) ----
// fd -> cd: the node grids of level l and l + 1 (grid_coarse_dims), bs the node size (1, 2 or 3).
// level 0's condition: throws SPK_ERR_UNSUPPORTED naming the first stored entry whose nodes are not neighbours
void galerkin_stencil_check_host(const int32_t fd[3], int bs, const int32_t *arp, const int32_t *aci);
// A_{l+1} from the sorted CSR of A_l: rp (rows + 1), ci and v (gs_nnz(cd, bs) entries each) are all written
void galerkin_stencil_host(const int32_t fd[3], const int32_t cd[3], int bs, const int32_t *arp, const int32_t *aci, const double *av,
                           int32_t *rp, int32_t *ci, double *v);
// the fine nodes of coarse node `node` in ascending order and their weights (at most 27; either pointer may be null);
// returns how many
int galerkin_stencil_children(const int32_t fd[3], const int32_t cd[3], int32_t node, int32_t *nodes, double *w);

// ---- the dense Schur complement of a few constraint rows (spk_pc_set_schur_pre) ----
// G: m x m as computed; S = (G + G^T) / 2; L: its Cholesky factor (lower, row-major).  Returns -1, or the first pivot that
// is not positive beyond rounding (S is not positive definite: linearly dependent rows of B)
int schur_dense_factor(int m, const double *G, double *S, double *L);

}  // namespace spk
