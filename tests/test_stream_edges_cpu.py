"""The layouts of the A block that do not need a grid -- the CSR stream kernel, the 2x2- and the 3x3-blocked kernels, and
the FP32 sweeps on them -- each have two paths per workgroup: a tile of many (block) rows staged in LDS and summed in CSR
order, or one (block) row longer than a tile summed on its own.  This file states, without a GPU, which row takes which
path, builds matrices whose rows sit at that switch, restates the sweeps in numpy float32 over logical ranks, and derives
the bounds the long rows are held to; test_gpu_stream_edges.py runs the device on the same inputs.

The path rules (build_tiles, build_btiles, build_b3tiles close a tile BEFORE a row that does not fit, so each holds per
row, whatever the tiling):
  csr      row r is long       iff  rowptr[r + 1] - (rowptr[r] & ~3) > 2048   (the tile starts at a 4-entry boundary)
  bcsr2x2  block row is long   iff  it holds more than 512 blocks
  bcsr3x3  block row is long   iff  it holds more than 256 blocks
A tile also closes at 256 rows, 128 block rows, 85 block rows.

The bounds (worst case, no margin on top).  A sum of L terms p_k in any order, tree or sequential, products rounded:
|computed - exact| <= (L + 1) u sum|p_k|, exact taken from the values the kernel reads.
  products (u = 2^-53)  + (nbt + noff) u (sum|b lambda| + sum|a_off x|) for the fused multiply-adds of the row tail
  sweeps (u = 2^-24)    omega d times the dot bound, + 4 u (|y| + omega d (|x| + |s|)) for the update's own roundings
The tail's term counts one rounding per rider on the riders alone: on a tiled row the (nbt + noff) roundings also fall on
the row's own sum, which the (L + 1) of the first term covers only where L is not small against nbt + noff.  So the
constraint blocks touch tiled rows of eight entries or more, the ragged rows take their columns from their neighbourhood
(few rows have columns across a cut), and tail_emulated restates the tiled rows' arithmetic exactly: the bound is seen to
hold on every row of these inputs before a device is asked (test_the_tail_restated_stays_inside_the_product_bound)."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import saddle_point_petsc_amd as S
from test_amg_cpu import general_spd

CSR_TILE, B2_TILE, B3_TILE = 2048, 512, 256          # kCsrTile, kBTile, kB3Tile
CSR_ROWS, B2_ROWS, B3_ROWS = 256, 128, 85            # rows of a tile at the most
U64, U32 = 2.0**-53, 2.0**-24
N_CSR = 3001
NB = 700
SWEEPS, OMEGAS = (1, 2, 3, 4), (0.8, 1.0)


# --------------------------------------------------------------------------- which path a row takes
def long_csr(rowptr):
    rp = np.asarray(rowptr, np.int64)
    return rp[1:] - (rp[:-1] & ~np.int64(3)) > CSR_TILE


def long_b2(browptr):
    return np.diff(np.asarray(browptr, np.int64)) > B2_TILE


def long_b3(browptr):
    return np.diff(np.asarray(browptr, np.int64)) > B3_TILE


def tiles_csr(rowptr):
    """build_tiles restated: the first row of every tile, and nrows"""
    rp = [int(v) for v in rowptr]
    n, t, r = len(rp) - 1, [0], 0
    while r < n:
        r0, a0 = r, rp[r] & ~3
        while r < n and r - r0 < CSR_ROWS and rp[r + 1] - a0 <= CSR_TILE:
            r += 1
        if r == r0:
            r += 1
        t.append(r)
    return np.array(t)


def tiles_blocked(browptr, tile, rows):
    """build_btiles (512, 128) and build_b3tiles (256, 85) restated"""
    rp = [int(v) for v in browptr]
    n, t, r = len(rp) - 1, [0], 0
    while r < n:
        r0 = r
        while r < n and r - r0 < rows and rp[r + 1] - rp[r0] <= tile:
            r += 1
        if r == r0:
            r += 1
        t.append(r)
    return np.array(t)


def block_rowptr(A, bs):
    return A.rowptr[::bs].astype(np.int64) // (bs * bs)


def long_rows(A, fmt):
    """per scalar row of A: does the layout `fmt` sum it on the long path"""
    if fmt == "csr":
        return long_csr(A.rowptr)
    bs = {"bcsr2x2": 2, "bcsr3x3": 3}[fmt]
    return np.repeat((long_b2 if bs == 2 else long_b3)(block_rowptr(A, bs)), bs)


def diag_block(A, lo, hi):
    """rows [lo, hi) of A with the columns in [lo, hi) only, as a rank keeps them (order inside a row kept)"""
    k0, k1 = int(A.rowptr[lo]), int(A.rowptr[hi])
    col, val = A.colidx[k0:k1], A.val[k0:k1]
    keep = (col >= lo) & (col < hi)
    rows = np.repeat(np.arange(hi - lo), np.diff(A.rowptr[lo:hi + 1]))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=hi - lo))]).astype(np.int32)
    return S.CSR(rp, col[keep] - lo, val[keep], hi - lo)


# --------------------------------------------------------------------------- the matrices
EDGE_E = (CSR_TILE - 1, CSR_TILE, CSR_TILE + 1)
RUN_CSR, RUN_START_CSR = 300, 2300
WINDOW = 60          # a ragged row's columns: among the 2 x 60 rows around it


def _edge_plan_csr():
    """row -> (start residue rowptr[r] % 4 or None, E = rowptr[r + 1] - (rowptr[r] & ~3) or the plain length)"""
    plan = {0: (0, CSR_TILE + 1), N_CSR - 1: (2, CSR_TILE + 1), 2100: (None, 2600),
            RUN_START_CSR + RUN_CSR: (1, CSR_TILE)}
    row = 100
    for rho in range(4):
        for E in EDGE_E:
            plan[row] = (rho, E)
            row += 170
    return plan


def _fill_rows(rng, rowptr, ok, wide, n):
    """columns and values: one diagonal entry at a random place of the row, the others drawn without repetition from
    `ok` (never a long row) -- a row listed in `wide` from all of them, any other from its neighbourhood --, unsorted;
    diagonal = 4 + sum |off-diagonal|"""
    colidx = np.empty(rowptr[-1], np.int32)
    val = np.empty(rowptr[-1])
    where = np.searchsorted(ok, np.arange(n))
    for r in range(n):
        k0, k1 = rowptr[r], rowptr[r + 1]
        ln = k1 - k0
        if r in wide:
            pool = ok
        else:
            lo = max(0, min(where[r] - WINDOW, len(ok) - 2 * WINDOW))
            pool = ok[lo:lo + 2 * WINDOW]
        cols = rng.choice(pool[pool != r], ln - 1, replace=False)
        at = int(rng.integers(0, ln))
        v = rng.standard_normal(ln - 1) * 0.3
        colidx[k0:k1] = np.insert(cols, at, r)
        val[k0:k1] = np.insert(v, at, 4.0 + np.abs(v).sum())
    return colidx, val


def edge_csr():
    """3001 rows (odd), ragged rows of 1-39 entries, and rows at the switch between the two paths of the CSR kernels: for
    every start residue rowptr[r] % 4 one row each with E = 2047, 2048 (tiled; the second fills its tile to the last
    entry) and 2049 (long) -- among them 2046 entries at residue 3 (long though shorter than a tile) and 2048 at residue 0
    (tiled) --, a row of 2600, rows 0 and n - 1 with E = 2049, and 300 one-entry rows in front of a row that fills a tile
    (the tile before it is closed by the 256-row cap).  Returns (A, plan)."""
    rng = np.random.default_rng(2049)
    n, plan = N_CSR, _edge_plan_csr()
    lens = rng.integers(1, 40, n)
    lens[RUN_START_CSR:RUN_START_CSR + RUN_CSR] = 1
    rowptr = np.zeros(n + 1, np.int64)
    for r in range(n):
        if r in plan:
            rho, E = plan[r]
            assert rho is None or rowptr[r] % 4 == rho
            lens[r] = E if rho is None else E - rho
        # the row in front of an edge row (or of the run that ends in one) steers the residue it starts at
        nxt = r + 1 + (RUN_CSR if r + 1 == RUN_START_CSR else 0)
        if nxt in plan and plan[nxt][0] is not None:
            assert r not in plan
            lens[r] += (plan[nxt][0] - (rowptr[r] + lens[r])) % 4
            if lens[r] > 39:
                lens[r] -= 4
        rowptr[r + 1] = rowptr[r] + lens[r]
    ok = np.flatnonzero(~long_csr(rowptr))
    colidx, val = _fill_rows(rng, rowptr, ok, set(plan), n)
    return S.CSR(rowptr.astype(np.int32), colidx, val, n), plan


def edge_bcsr(bs):
    """700 block rows of bs x bs blocks, ragged (1-40 blocks for bs = 2, 1-24 for bs = 3, arbitrary column order), with
    block rows of T - 1, T and T + 1 blocks (T = 512 / 256: tiled, tiled and filling its tile, long), the first and the
    last block row at T + 1, a run of one-block rows longer than the row cap (130 / 87) in front of another of T + 1, and
    one of 600 / 300 blocks (long on a rank that keeps nine tenths of the columns, with the others off-rank).
    Returns (A, {block row: blocks})."""
    T, cap_run = (B2_TILE, B2_ROWS + 2) if bs == 2 else (B3_TILE, B3_ROWS + 2)
    rng = np.random.default_rng(500 + bs)
    nb = NB
    plan = {0: T + 1, 37: 600 if bs == 2 else 300, 100: T - 1, 200: T, 300: T + 1, 400 + cap_run: T + 1, nb - 1: T + 1}
    lens = rng.integers(1, 41 if bs == 2 else 25, nb)
    lens[400:400 + cap_run] = 1
    for br, ln in plan.items():
        lens[br] = ln
    brp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    is_long = lens > T
    ok = np.flatnonzero(~is_long)
    bcol, _ = _fill_rows(rng, brp, ok, set(plan), nb)
    rp, ci, va = [0], [], []
    for br in range(nb):
        cols = bcol[brp[br]:brp[br + 1]].astype(np.int64)
        blocks = rng.standard_normal((bs, len(cols), bs)) * 0.3
        for r in range(bs):
            row = blocks[r]
            d = int(np.flatnonzero(cols == br)[0])
            row[d, r] = 0.0
            row[d, r] = 4.0 + np.abs(row).sum()
            ci.append((bs * cols[:, None] + np.arange(bs)[None, :]).ravel())
            va.append(row.ravel())
            rp.append(rp[-1] + bs * len(cols))
    A = S.CSR(np.array(rp, np.int32), np.concatenate(ci).astype(np.int32), np.concatenate(va), bs * nb)
    return A, plan


def touched_rows(A, fmt, seed=5):
    """the rows a constraint block may touch: (every row that is long in the layout, 60 tiled rows of eight entries or
    more -- see the file's docstring -- with the longest tiled rows among them)"""
    lg = long_rows(A, fmt) | long_rows(A, "csr")
    lens = np.diff(A.rowptr)
    cand = np.flatnonzero(~lg & (lens >= 8))
    rng = np.random.default_rng(seed)
    longest = cand[np.argsort(lens[cand])[-6:]]
    return np.flatnonzero(lg), np.unique(np.concatenate([longest, rng.choice(cand, 54, replace=False)]))


def constraints(n, m, touch, seed=17):
    """m random sparse rows over n columns: every row holds entries on two or more of touch[0] (long rows) and on about
    four in ten of touch[1] (tiled rows).  m <= 8 rides in the product's tail; m > 8 is a general block (the A product
    accumulates onto B^T lambda)."""
    rng = np.random.default_rng(seed + m)
    lg, tiled = (np.asarray(t) for t in touch)
    rp, ci, va = [0], [], []
    for _ in range(m):
        cols = np.concatenate([rng.choice(lg, int(rng.integers(2, min(len(lg), 5) + 1)), replace=False),
                               tiled[rng.random(len(tiled)) < 0.4]])
        cols = rng.permutation(cols)
        ci.append(cols)
        va.append(rng.standard_normal(len(cols)))
        rp.append(rp[-1] + len(cols))
    return S.CSR(np.array(rp, np.int32), np.concatenate(ci).astype(np.int32), np.concatenate(va), n)


def transposed(B, lo=0, hi=None):
    """B^T by rows (columns [lo, hi) of B), a row's entries ordered by constraint index: (rowptr, colidx, val)"""
    hi = B.ncols if hi is None else hi
    Bt = sp.csr_matrix((B.val, B.colidx, B.rowptr), shape=(B.nrows, B.ncols)).T.tocsr()[lo:hi]
    Bt.sort_indices()
    return Bt.indptr.astype(np.int64), Bt.indices.astype(np.int64), Bt.data.copy()


# --------------------------------------------------------------------------- exact sums in float64
def two_prod(a, b):
    """a b = p + e exactly (Dekker / Veltkamp), elementwise"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah = ca - (ca - a); al = a - ah
    bh = cb - (cb - b); bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, s):
    p, e = two_prod(a, b)
    return math.fsum((float(p), float(e), s))


def product_check(Sl, y, x, lo, hi, Bt=None, lam=None):
    """The product bound on the slab Sl (global columns; [lo, hi) are the rank's own) for the computed y: returns
    (|y - exact| rounded once, bound) per row.  exact = the row's entries times x, plus its B^T entries times lam."""
    nr = Sl.nrows
    rows = np.repeat(np.arange(nr), np.diff(Sl.rowptr))
    col = Sl.colidx.astype(np.int64)
    p, e = two_prod(Sl.val, x[col])
    local = (col >= lo) & (col < hi)
    L = np.bincount(rows[local], minlength=nr)
    noff = np.bincount(rows[~local], minlength=nr)
    sp_ = np.bincount(rows[local], np.abs(p[local]), nr)
    so = np.bincount(rows[~local], np.abs(p[~local]), nr)
    nbt, sq = np.zeros(nr, np.int64), np.zeros(nr)
    if Bt is not None:
        trp, tci, tv = Bt
        q, qe = two_prod(tv, lam[tci])
        trow = np.repeat(np.arange(nr), np.diff(trp))
        nbt = np.diff(trp)
        sq = np.bincount(trow, np.abs(q), nr)
    bound = (L + 1) * U64 * sp_ + (nbt + noff) * U64 * (sq + so)
    err = np.empty(nr)
    for r in range(nr):
        k0, k1 = Sl.rowptr[r], Sl.rowptr[r + 1]
        parts = [float(y[r])] + list(-p[k0:k1]) + list(-e[k0:k1])
        if Bt is not None:
            parts += list(-q[trp[r]:trp[r + 1]]) + list(-qe[trp[r]:trp[r + 1]])
        err[r] = abs(math.fsum(parts))
    return err, bound


def tail_emulated(oracle, Sl, x, lo, hi, Bt=None, lam=None, acc=False):
    """A TILED row as the kernels compute it, bit for bit: the local entries' products rounded and added in CSR order,
    then one fused multiply-add per off-rank entry, then per B^T entry (row_tail_add); acc: B^T lambda summed on its own
    first (the stream kernel on B^T, CSR order) and added last."""
    nr = Sl.nrows
    D = diag_block_of_slab(Sl, lo, hi)
    y = oracle.spmv(oracle.CSR(D.rowptr, D.colidx, D.val, hi - lo), x[lo:hi])
    col = Sl.colidx.astype(np.int64)
    off = (col < lo) | (col >= hi)
    for r in np.flatnonzero(np.add.reduceat(off.astype(np.int64), Sl.rowptr[:-1].astype(np.int64)) > 0):
        for k in range(Sl.rowptr[r], Sl.rowptr[r + 1]):
            if off[k]:
                y[r] = fma(Sl.val[k], x[col[k]], y[r])
    if Bt is not None:
        trp, tci, tv = Bt
        for r in np.flatnonzero(np.diff(trp) > 0):
            if acc:
                y0 = 0.0
                for k in range(trp[r], trp[r + 1]):
                    y0 = y0 + tv[k] * lam[tci[k]]
                y[r] = y[r] + y0
            else:
                for k in range(trp[r], trp[r + 1]):
                    y[r] = fma(tv[k], lam[tci[k]], y[r])
    return y


def diag_block_of_slab(Sl, lo, hi):
    keep = (Sl.colidx >= lo) & (Sl.colidx < hi)
    rows = np.repeat(np.arange(Sl.nrows), np.diff(Sl.rowptr))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=Sl.nrows))]).astype(np.int32)
    return S.CSR(rp, Sl.colidx[keep] - lo, Sl.val[keep], hi - lo)


# --------------------------------------------------------------------------- the sweeps in numpy float32
def _seq_sums(rows, p, n):
    """s[r] = (((0 + p_0) + p_1) + ...) over the entries of row r in the order given (`rows` ascending), every sum
    rounded to p's type"""
    s = np.zeros(n, p.dtype)
    if len(rows) == 0:
        return s
    start = np.flatnonzero(np.r_[True, rows[1:] != rows[:-1]])
    cnt = np.diff(np.r_[start, len(rows)])
    rr = rows[start]
    live, j = np.arange(len(rr)), 0
    while len(live):
        s[rr[live]] = s[rr[live]] + p[start[live] + j]
        j += 1
        live = live[cnt[live] > j]
    return s


def jacobi_d32(A):
    """float(1 / diagonal), the last diagonal entry of a row counting, a zero diagonal as 1 (PCJACOBI)"""
    rows = np.repeat(np.arange(A.nrows), np.diff(A.rowptr))
    d = np.zeros(A.nrows)
    on = A.colidx == rows
    d[rows[on]] = A.val[on]
    return (1.0 / np.where(d == 0.0, 1.0, d)).astype(np.float32)


def sweeps_ref(A, cuts, sweeps, omega, x):
    """inner_apply restated in float32 over the logical ranks [cuts[i], cuts[i + 1]): y_1 = (omega d) x; per later sweep
    and row s = the float sum over the row's LOCAL columns in stored order (each product rounded once, nothing
    contracted), y = y + (omega d) (x - s); then, on the rows that have them, sacc = the float sum over the off-rank
    columns in stored order of float(val) float(y_prev) (the halo is staged as doubles: exact) and y = y - (omega d) sacc.
    cuts = None: one rank.  Returns float64."""
    n = A.nrows
    cuts = np.asarray([0, n] if cuts is None else cuts)
    rows = np.repeat(np.arange(n), np.diff(A.rowptr))
    col = A.colidx.astype(np.int64)
    rank = np.searchsorted(cuts, np.arange(n), "right") - 1
    local = rank[rows] == rank[col]
    a32 = A.val.astype(np.float32)
    od = np.float32(omega) * jacobi_d32(A)
    x32 = np.asarray(x, np.float64).astype(np.float32)
    y = od * x32
    for _ in range(1, sweeps):
        p = a32 * y[col]
        s = _seq_sums(rows[local], p[local], n)
        yn = y + od * (x32 - s)
        if not local.all():
            sacc = _seq_sums(rows[~local], p[~local], n)
            has = np.unique(rows[~local])
            yn[has] = yn[has] - od[has] * sacc[has]
        y = yn
    assert y.dtype == np.float32
    return y.astype(np.float64)


def sweep_step_check(A, y_prev, x, omega, y_new):
    """The one-step bound on every row: y_new against y_prev + (omega d)(x - s) evaluated in float64 from the values the
    kernel reads (the float-rounded matrix, the previous iterate as floats), s over ALL the row's columns.  Returns
    (error, bound) per row."""
    rows = np.repeat(np.arange(A.nrows), np.diff(A.rowptr))
    a = A.val.astype(np.float32).astype(np.float64)
    yp = np.asarray(y_prev, np.float64)
    assert np.array_equal(yp, yp.astype(np.float32))
    x32 = np.asarray(x, np.float64).astype(np.float32).astype(np.float64)
    od = float(np.float32(omega)) * jacobi_d32(A).astype(np.float64)       # exact: 48 bits
    p = a * yp[A.colidx]                                                    # exact: 48 bits
    s = np.bincount(rows, p, A.nrows)
    sabs = np.bincount(rows, np.abs(p), A.nrows)
    L = np.diff(A.rowptr)
    exact = yp + od * (x32 - s)
    bound = np.abs(od) * (L + 1) * U32 * sabs + 4 * U32 * (np.abs(yp) + np.abs(od) * (np.abs(x32) + np.abs(s)))
    return np.abs(np.asarray(y_new, np.float64) - exact), bound


def vec(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


# --------------------------------------------------------------------------- the inputs, built once
@pytest.fixture(scope="module")
def csr_case():
    return edge_csr()


@pytest.fixture(scope="module", params=[2, 3])
def bcsr_case(request):
    return (request.param,) + edge_bcsr(request.param)


@pytest.fixture(scope="module")
def matrices(csr_case):
    return {"edge_csr": csr_case[0], "edge_bcsr2": edge_bcsr(2)[0], "edge_bcsr3": edge_bcsr(3)[0],
            "general_spd": general_spd(1001, 1001)[0]}


# --------------------------------------------------------------------------- tests
def test_edge_csr_has_every_row_at_the_switch(csr_case):
    A, plan = csr_case
    rp = A.rowptr.astype(np.int64)
    n = A.nrows
    assert n == N_CSR and n % 2 == 1 and A.nnz <= 110_000
    lens = np.diff(rp)
    E = rp[1:] - (rp[:-1] & ~np.int64(3))
    res = rp[:-1] % 4
    lg = long_csr(rp)
    for r, (rho, want) in plan.items():
        if rho is None:
            assert lens[r] == want == 2600 and lg[r]
        else:
            assert (res[r], E[r]) == (rho, want) and lg[r] == (want > CSR_TILE)
    got = {(int(res[r]), int(E[r])) for r in plan}
    assert {(rho, e) for rho in range(4) for e in EDGE_E} <= got
    short_but_long = [r for r in plan if lens[r] == CSR_TILE - 2 and res[r] == 3]
    assert short_but_long and lg[short_but_long].all()                     # 2046 entries at residue 3: long
    full = [r for r in plan if lens[r] == CSR_TILE and res[r] == 0]
    assert full and not lg[full].any()                                     # 2048 entries at residue 0: tiled
    assert lg[0] and lg[n - 1] and E[0] == E[n - 1] == CSR_TILE + 1
    assert lg.sum() == 7 and (lens[~lg & ~np.isin(np.arange(n), list(plan))] <= 39).all() and lens.min() == 1
    # the rows: one diagonal entry each, strictly dominant, unsorted, and nobody but itself reads a long row
    rows = np.repeat(np.arange(n), lens)
    assert (np.bincount(rows[A.colidx == rows], minlength=n) == 1).all()
    off = np.bincount(rows, np.where(A.colidx == rows, 0.0, np.abs(A.val)), n)
    dg = np.bincount(rows, np.where(A.colidx == rows, A.val, 0.0), n)
    assert (dg > 3.99 + off).all()
    assert not (lg[A.colidx] & (A.colidx != rows)).any()
    assert any((np.diff(A.colidx[rp[r]:rp[r + 1]]) < 0).any() for r in range(n) if lens[r] > 2)


def test_the_csr_rule_is_what_build_tiles_does(csr_case, matrices):
    """the rule per row against the tiling restated; the run of 300 one-entry rows closes a tile at the row cap; rows
    with E = 2048 fill theirs to the last entry"""
    for name, A in matrices.items():
        rp = A.rowptr.astype(np.int64)
        t = tiles_csr(rp)
        cnt = rp[t[1:]] - (rp[t[:-1]] & ~np.int64(3))
        alone = np.zeros(A.nrows, bool)
        alone[t[:-1][cnt > CSR_TILE]] = True
        assert ((np.diff(t) == 1) | (cnt <= CSR_TILE)).all()
        assert np.array_equal(alone, long_csr(rp)), name
    A, plan = csr_case
    rp = A.rowptr.astype(np.int64)
    t = tiles_csr(rp)
    cnt = rp[t[1:]] - (rp[t[:-1]] & ~np.int64(3))
    capped = np.flatnonzero(np.diff(t) == CSR_ROWS)
    assert len(capped) and (cnt[capped] < CSR_TILE).all()                  # closed by its rows, not by its entries
    assert any(t[i] < RUN_START_CSR + RUN_CSR and t[i + 1] > RUN_START_CSR + CSR_ROWS // 2 for i in capped)   # in the run
    after = RUN_START_CSR + RUN_CSR
    assert after in t and cnt[list(t).index(after)] == CSR_TILE            # the edge row behind the run starts a tile
    assert (cnt == CSR_TILE).sum() >= 5 and (cnt == CSR_TILE + 1).sum() >= 6


def test_edge_bcsr_has_every_block_row_at_the_switch(bcsr_case):
    bs, A, plan = bcsr_case
    T, cap, rule = (B2_TILE, B2_ROWS, long_b2) if bs == 2 else (B3_TILE, B3_ROWS, long_b3)
    nb = A.nrows // bs
    assert nb == NB >= 700 and A.nnz <= 110_000
    brp = block_rowptr(A, bs)
    assert np.array_equal(brp * bs * bs, A.rowptr[::bs])                   # block row br starts at rowptr[bs br] / bs^2
    lens = np.diff(brp)
    assert {T - 1, T, T + 1} <= set(lens.tolist()) and lens[0] == lens[nb - 1] == T + 1
    lg = rule(brp)
    assert np.array_equal(lg, lens > T) and sorted(np.flatnonzero(lg)) == sorted(b for b, v in plan.items() if v > T)
    assert not lg[[b for b, v in plan.items() if v <= T]].any()
    t = tiles_blocked(brp, T, cap)
    cnt = brp[t[1:]] - brp[t[:-1]]
    alone = np.zeros(nb, bool)
    alone[t[:-1][cnt > T]] = True
    assert np.array_equal(alone, lg)
    capped = np.flatnonzero(np.diff(t) == cap)
    assert len(capped) and (cnt[capped] < T).all() and (cnt == T).sum() >= 1       # closed by its rows; a full tile
    run_end = 400 + cap + 2
    assert lg[run_end] and (lens[400:run_end] == 1).all() and run_end in t
    # the structure the blocked copies need, and the rows
    n = A.nrows
    rows = np.repeat(np.arange(n), np.diff(A.rowptr))
    for r in range(bs):
        assert np.array_equal(np.diff(A.rowptr)[r::bs], bs * lens)
    bc = A.colidx // bs
    assert not (np.repeat(lg, bs)[A.colidx] & (bc != rows // bs)).any()    # nobody but itself reads a long block row
    assert (np.bincount(rows[A.colidx == rows], minlength=n) == 1).all()
    off = np.bincount(rows, np.where(A.colidx == rows, 0.0, np.abs(A.val)), n)
    dg = np.bincount(rows, np.where(A.colidx == rows, A.val, 0.0), n)
    assert (dg > 3.99 + off).all()
    # forced to the CSR kernels no row of these is long: the same rows, tiled
    assert not long_csr(A.rowptr).any()


def test_constraint_blocks_touch_long_and_tiled_rows(matrices):
    for name, fmt in (("edge_csr", "csr"), ("edge_bcsr2", "bcsr2x2"), ("edge_bcsr3", "bcsr3x3")):
        A = matrices[name]
        touch = touched_rows(A, fmt)
        lg = long_rows(A, fmt)
        assert lg[touch[0]].all() and not lg[touch[1]].any() and (np.diff(A.rowptr)[touch[1]] >= 8).all()
        for m in (4, 9):
            B = constraints(A.nrows, m, touch)
            assert B.nrows == m and B.ncols == A.nrows
            for r in range(m):
                cols = B.colidx[B.rowptr[r]:B.rowptr[r + 1]]
                assert lg[cols].sum() >= 2 and (~lg[cols]).sum() >= 2 and len(set(cols.tolist())) == len(cols)
            per_row = np.bincount(B.colidx, minlength=A.nrows)
            assert per_row[~lg].max() >= 3 and per_row[lg].max() >= 2     # several riders on one row, tiled and long


@pytest.mark.parametrize("omega", OMEGAS)
def test_sweeps_ref_is_the_oracle_on_one_rank(oracle, matrices, omega):
    """sweeps_ref without a cut against the oracle's float loop, bit for bit, for 1, 2, 3 and 4 sweeps (one: no sweep,
    the first buffer; two: one sweep, the other buffer)"""
    for name, A in matrices.items():
        x = vec(A.nrows, 31)
        for k in SWEEPS:
            z = sweeps_ref(A, None, k, omega, x)
            zo = oracle.pc_apply_inner(A, None, oracle.PC_JACOBI, 0, k, omega, x)
            assert np.array_equal(z, zo), (name, k)
        assert not np.array_equal(sweeps_ref(A, None, 1, omega, x), sweeps_ref(A, None, 2, omega, x))


def test_sweeps_ref_over_ranks_moves_only_rows_at_a_cut(matrices):
    """with cuts the rows whose columns are all their rank's keep the bits of the single-rank sweep while their inputs
    do (the first sweep: y_1 has no sum in it), the others add their off-rank columns last"""
    A = matrices["edge_csr"]
    x = vec(A.nrows, 32)
    cuts = CUTS["edge_csr"][0]
    rows = np.repeat(np.arange(A.nrows), np.diff(A.rowptr))
    rank = np.searchsorted(cuts, np.arange(A.nrows), "right") - 1
    crossing = np.bincount(rows[rank[rows] != rank[A.colidx]], minlength=A.nrows) > 0
    one, two = sweeps_ref(A, None, 2, 0.8, x), sweeps_ref(A, cuts, 2, 0.8, x)
    assert np.array_equal(one[~crossing], two[~crossing]) and crossing.sum() > 20
    assert (one[crossing] != two[crossing]).any() and np.allclose(one, two, rtol=1e-5, atol=1e-7)


def test_the_oracle_stays_inside_the_one_step_bound(oracle, matrices):
    """The one-step sweep bound on EVERY row, for the oracle's own float loop (sequential order): the largest
    error / bound is 0.27 over all rows (short rows: the update's four roundings are the bound) and 5.6e-4 on the rows the
    CSR layout calls long."""
    worst, worst_long = 0.0, 0.0
    for name, A in matrices.items():
        x = vec(A.nrows, 33)
        lg = long_csr(A.rowptr)
        for omega in OMEGAS:
            prev = oracle.pc_apply_inner(A, None, oracle.PC_JACOBI, 0, 1, omega, x)
            for k in (2, 3, 4):
                new = oracle.pc_apply_inner(A, None, oracle.PC_JACOBI, 0, k, omega, x)
                err, bound = sweep_step_check(A, prev, x, omega, new)
                assert (err <= bound).all(), (name, omega, k, (err / bound).max())
                worst = max(worst, (err / bound).max())
                if lg.any():
                    worst_long = max(worst_long, (err[lg] / bound[lg]).max())
                prev = new
    print(f"one-step bound, the oracle's loop: largest error / bound {worst:.3g} (all rows), {worst_long:.3g} (long rows)")
    assert 0 < worst_long < worst < 1


def test_a_dropped_entry_of_a_long_row_breaks_the_bounds(oracle, csr_case):
    """what the bounds are for: one off-diagonal entry of a long row left out moves the result by many bounds in the
    product (every long row); in the sweep, whose bound is 2050 u = 1.2e-4 of sum|p| against the 1 / 2049 = 4.9e-4 an
    average entry holds, by more than the bound on the rows where the entry is not a small one (here two of seven)"""
    A, _ = csr_case
    n = A.nrows
    x = vec(n, 34)
    lg = np.flatnonzero(long_csr(A.rowptr))
    y = oracle.spmv(A, x)
    err, bound = product_check(A, y, x, 0, n)
    assert (err <= bound).all()
    last = A.rowptr[lg + 1] - 1
    last = np.where(A.colidx[last] == lg, last - 1, last)                    # the last off-diagonal entry of each
    val = A.val.copy()
    val[last] = 0.0
    Ad = S.CSR(A.rowptr, A.colidx, val, n)
    err, _ = product_check(A, oracle.spmv(Ad, x), x, 0, n)
    assert (err[lg] > 100 * bound[lg]).all()
    prev = oracle.pc_apply_inner(A, None, oracle.PC_JACOBI, 0, 1, 0.8, x)
    err, bound = sweep_step_check(A, prev, x, 0.8, oracle.pc_apply_inner(Ad, None, oracle.PC_JACOBI, 0, 2, 0.8, x))
    assert (err[lg] > bound[lg]).any() and (err[~long_csr(A.rowptr)] <= bound[~long_csr(A.rowptr)]).all()


# A row is long on a rank only with more than a tile of LOCAL entries, and meets the off-rank part of the tail only with
# further columns elsewhere: the 2600-entry row (600 / 300 blocks) on a rank that owns nine tenths of the rows.  (Three
# ranks of the blocked matrices: even shares -- a rank of a few dozen short block rows would get a dictionary layout.)
CUTS = {"edge_csr": ([0, 2701, N_CSR], [0, 2701, 2851, N_CSR]),
        "edge_bcsr2": ([0, 2 * 640, 2 * NB], [0, 2 * 240, 2 * 480, 2 * NB]),
        "edge_bcsr3": ([0, 3 * 640, 3 * NB], [0, 3 * 240, 3 * 480, 3 * NB]),
        "general_spd": ([0, 501, 1001], [0, 333, 667, 1001])}


def test_cuts_leave_long_rows_with_off_rank_columns(matrices):
    """an odd row for the CSR matrices, a block boundary for the blocked ones (their diagonal blocks keep the structure);
    under every cut that gives a rank nine tenths of the rows a row is still long in that rank's diagonal block and has
    off-rank columns"""
    for name, fmt, bs in (("edge_csr", "csr", 1), ("edge_bcsr2", "bcsr2x2", 2), ("edge_bcsr3", "bcsr3x3", 3)):
        A = matrices[name]
        for cuts in CUTS[name]:
            assert all(c % bs == 0 for c in cuts) and (bs > 1 or any(c % 2 for c in cuts[1:-1]))
            seen = 0
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                D = diag_block(A, lo, hi)
                lg = long_rows(D, fmt)
                off = np.diff(A.rowptr[lo:hi + 1]) - np.diff(D.rowptr)
                seen += int((lg & (off > 0)).sum())
                if bs > 1:
                    assert D.nnz % (bs * bs) == 0 and np.array_equal(block_rowptr(D, bs) * bs * bs, D.rowptr[::bs])
            assert seen >= 1 or cuts[1] < 0.9 * cuts[-1], (name, cuts)
    assert all(c % 2 for c in CUTS["general_spd"][0][1:-1]) and 1001 % 2 == 1


def test_the_tail_restated_stays_inside_the_product_bound(oracle, matrices):
    """tail_emulated (a tiled row's arithmetic: CSR-order sum, then the fused multiply-adds of the off-rank columns and
    of B^T lambda; with a general block B^T lambda summed first and added last) stays inside the product bound on every
    row of these inputs -- on one rank with the m = 4 and the m = 9 block, and on two ranks.  (Long rows are summed in
    tree order on the device; the sequential order here obeys the same any-order bound.)  Largest error / bound: 0.56."""
    worst = 0.0
    for name, fmt in (("edge_csr", "csr"), ("edge_bcsr2", "bcsr2x2"), ("edge_bcsr3", "bcsr3x3")):
        A = matrices[name]
        n = A.nrows
        for m in (4, 9):
            B = constraints(n, m, touched_rows(A, fmt))
            xl = vec(n + m, 35 + m)
            Bt = transposed(B)
            y = tail_emulated(oracle, A, xl[:n], 0, n, Bt, xl[n:], acc=m > 8)
            err, bound = product_check(A, y, xl[:n], 0, n, Bt, xl[n:])
            assert (err <= bound).all(), (name, m, (err / bound).max())
            worst = max(worst, (err / bound).max())
        x = vec(n, 36)
        cuts = CUTS[name][0]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            Sl = A.slab(lo, hi)
            y = tail_emulated(oracle, Sl, x, lo, hi)
            err, bound = product_check(Sl, y, x, lo, hi)
            assert (err <= bound).all(), (name, lo, hi, (err / bound).max())
            worst = max(worst, (err / bound).max())
    print(f"product bound, the tail restated: largest error / bound {worst:.3g}")
    assert worst < 1
