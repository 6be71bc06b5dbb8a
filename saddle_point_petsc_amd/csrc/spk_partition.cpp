// spk_partition.cpp -- C entry points of the host-only row-slab partition and of the diagonal/off-rank split of a
// CSR slab (spk_host.cpp: split_csr).  No HIP call in this file: it is exercised by the CPU-only tests.
#include <algorithm>
#include <cstring>

#include "spk_internal.hpp"

extern "C" int spk_partition_slab(int64_t nlines, int64_t line_rows, int rank, int nranks,
                                  int64_t *row_begin, int64_t *row_end)
{
    if (nranks <= 0 || rank < 0 || rank >= nranks || nlines < 0 || line_rows <= 0) return SPK_ERR_ARG;
    // PETSc's DMDA split of `nlines` lines over `nranks`: the first (nlines % nranks)
    // ranks get one extra line.
    const int64_t base = nlines / nranks, extra = nlines % nranks;
    const int64_t l0 = rank * base + std::min<int64_t>(rank, extra);
    const int64_t l1 = l0 + base + (rank < extra ? 1 : 0);
    if (row_begin) *row_begin = l0 * line_rows;
    if (row_end) *row_end = l1 * line_rows;
    return SPK_OK;
}

extern "C" int spk_partition_split(int64_t row_begin, int32_t nrows_local, const int32_t *rowptr,
                                   const int32_t *colidx, const double *val, int32_t *d_rowptr,
                                   int32_t *d_colidx, double *d_val, int32_t *o_rowptr,
                                   int32_t *o_colidx, double *o_val, int32_t *garray, int64_t *nnz_d,
                                   int64_t *nnz_o, int32_t *n_ghost)
{
    if (!rowptr || !colidx || !val || nrows_local < 0) return SPK_ERR_ARG;
    try {
        spk::SplitCsr s;
        spk::split_csr(row_begin, nrows_local, rowptr, colidx, val, s);
        if (nnz_d) *nnz_d = (int64_t)s.d_colidx.size();
        if (nnz_o) *nnz_o = (int64_t)s.o_colidx.size();
        if (n_ghost) *n_ghost = (int32_t)s.garray.size();
        auto cp = [](auto *dst, const auto &v) {
            if (dst && v.size()) std::memcpy(dst, v.data(), v.size() * sizeof(v[0]));
        };
        cp(d_rowptr, s.d_rowptr);
        cp(d_colidx, s.d_colidx);
        cp(d_val, s.d_val);
        cp(o_rowptr, s.o_rowptr);
        cp(o_colidx, s.o_colidx);
        cp(o_val, s.o_val);
        cp(garray, s.garray);
    } catch (...) {
        return SPK_ERR_NOMEM;
    }
    return SPK_OK;
}
