"""The general constraint block (more than 8 rows) at the edges of its three paths: the inputs, a numpy restatement of the
rules that send a row down a path, the long-double reference of every operation and the bars the results are held to.
Shared by test_general_b_edges_cpu.py (no GPU: the cases hold the classes they were built for, a plain float64 evaluation
stays inside the bars) and test_gpu_general_b_edges.py (the device on the same inputs).

The three rules (spk_host.cpp wide_rows, spk_k_spmv.hip build_tiles, on this rank's row pointers):
  wide       a row of more than 8192 local entries goes to the column-window kernel -- at most 8 rows, the longest first,
             ties to the lower row; the others stay in the stream whatever their length
  long       a stream row r is summed by a workgroup of its own iff  crp[r + 1] - (crp[r] & ~3) > 2048, crp the row
             pointers of Bc = the block with its wide rows emptied (so a wide row in front shifts the residues)
  tiles      a tile closes before the row that would take it past 2048 entries (counted from the 4-entry boundary at or
             below its first entry) or past 256 rows; the same for B^T by rows, the operand of B^T lambda

The bars are component-wise and derived, gamma(k) = k u / (1 - k u) (the rigorous form of k u: (1 + u)^k - 1 <= gamma(k))
with u = 2^-53 + 2^-64.  The 2^-64 is the unit round-off of the long-double reference itself: what a result is compared
with is the reference's sum, which carries k roundings of its own, so a device result that sits exactly on the float64
bound may stand up to k 2^-64 sum|terms| from it.  It widens every bar by 2^-11 of itself (0.05 %), no more:
  a sum of k products in any order (sequential, tree, per window, over ranks)   gamma(k + c + ranks) sum|terms|
    c = the roundings of a term beyond its product: 0 for b x, 1 for b (d x), 2 for b b d; ranks = P for P > 1 (the sum
    over the ranks' shares), 0 on one rank.  A row of A with its B^T lambda is one sum over both kinds of term.
  PCApply                                                                       the same bounds pushed through the chain
    t = B D x0, y1 = -(x1 - t) / S^, B^T y1, the combination: every stage adds gamma(its own roundings) of its operands'
    magnitudes (the reference's, grown by the error they may carry) to the error it inherits.
Nothing here looks at a device result."""
import numpy as np

import saddle_point_petsc_amd as S
from test_amg_cpu import general_spd
from test_stream_edges_cpu import long_csr, tiles_csr

LD = np.longdouble
U = 2.0 ** -53
WIDE, MAX_WIDE = 8192, 8          # kWideRowNnz (strict), the cap of wide_rows
MAX_BLOCKS = 2048                 # k::kMaxBlocks
DIAG, LOWER, UPPER, FULL = 0, 1, 2, 3
FACTS = (DIAG, LOWER, UPPER, FULL)


U_REF = float(np.finfo(LD).eps) / 2   # the reference's own unit round-off (2^-64 where long double is the x87 format)


def gamma(k):
    """k roundings of the device's float64 plus the k of the long-double reference it is compared with"""
    k = np.asarray(k, LD)
    return k * LD(U + U_REF) / (1 - k * LD(U + U_REF))


# --------------------------------------------------------------------------- the rules restated
def wide_rows_ref(rowptr):
    lens = np.diff(np.asarray(rowptr, np.int64))
    m = len(lens)
    if m <= 8:
        return list(range(m))
    cand = sorted((r for r in range(m) if lens[r] > WIDE), key=lambda r: (-lens[r], r))
    return sorted(cand[:MAX_WIDE])


def window_width_ref(nl):
    win = 8192
    while (nl + win - 1) // win > MAX_BLOCKS:
        win *= 2
    while win > 1024 and (nl + win - 1) // win < 128:
        win //= 2
    return win


def classes(B, lo=0, hi=None):
    """What the set-up makes of the column slice [lo, hi) of B: `layout` = what Context.constraint_layout() must report,
    and per row of the slice: lens, wide, over (more than 8192 entries yet in the stream), long (a workgroup of its own in
    the stream), res (its Bc row pointer mod 4); bt_* = the same for B^T by rows; bt_empty_tiles = tiles of B^T whose
    rows are all empty."""
    hi = B.ncols if hi is None else hi
    Bs = B if (lo == 0 and hi == B.ncols) else B.col_slab(lo, hi)
    nl, m = hi - lo, Bs.nrows
    rp = Bs.rowptr.astype(np.int64)
    lens = np.diff(rp)
    general = m > 8
    wide = np.zeros(m, bool)
    wide[wide_rows_ref(rp)] = True
    clen = np.where(wide, 0, lens) if general else lens
    crp = np.concatenate([[0], np.cumsum(clen)])
    trp = np.concatenate([[0], np.cumsum(np.bincount(Bs.colidx.astype(np.int64) - lo, minlength=nl))])
    bt_tiles = tiles_csr(trp)
    win = window_width_ref(nl)
    layout = dict(general=general, m_wide=int(wide.sum()), wide_rows=[int(r) for r in np.flatnonzero(wide)], win=win,
                  nwin=(nl + win - 1) // win if wide.any() else 0,
                  bc_tiles=len(tiles_csr(crp)) - 1 if general else 0, bt_tiles=len(bt_tiles) - 1 if general else 0)
    return dict(layout=layout, lens=lens, wide=wide, over=(lens > WIDE) & ~wide, long=long_csr(crp) & ~wide, res=crp[:-1] % 4,
                crp=crp, trp=trp, bt_long=long_csr(trp), bt_tiles=bt_tiles,
                bt_empty_tiles=int(sum(trp[a] == trp[b] for a, b in zip(bt_tiles[:-1], bt_tiles[1:]))))


# --------------------------------------------------------------------------- the inputs
def vec(n, seed):
    """both signs, three decades of magnitude: the sums cancel"""
    rng = np.random.default_rng(seed)
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-1.5, 1.5, n)


def _block(rows, n):
    rp = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int32)
    return S.CSR(rp, np.concatenate([c for c, _ in rows]).astype(np.int32), np.concatenate([v for _, v in rows]), n)


def _row(rng, pool, k, must=(), sort=True):
    """k distinct columns from `pool`, the ones in `must` among them; normal values"""
    must = np.asarray(must, np.int64)
    rest = np.setdiff1d(pool, must)
    cols = np.concatenate([must, rng.choice(rest, k - len(must), replace=False)])
    cols = np.sort(cols) if sort else rng.permutation(cols)
    return cols, rng.standard_normal(k)


def small_case():
    """A = general_spd(1031): two windows of 1024 with seven columns in the second.  m = 9 (the first general size): row 0
    with unsorted columns, rows whose last column is 0, 1023, 1024 and 1030, four more of 3-40 entries."""
    n = 1031
    A = general_spd(n, 1031)[0]
    rng = np.random.default_rng(91)
    rows = [_row(rng, np.arange(n), 33, sort=False),
            _row(rng, np.arange(1), 1, must=[0]),
            _row(rng, np.arange(1024), 17, must=[1023]),
            _row(rng, np.arange(1025), 29, must=[0, 1024]),
            _row(rng, np.arange(n), 40, must=[1023, 1024, 1030])]
    rows += [_row(rng, np.arange(n), int(k)) for k in (3, 12, 25, 39)]
    return A, _block(rows, n)


LONG_GRID = (13, 13, 19)
# the ten rows of 8200..8209 entries in the order they stand in the block (rows 8..16 and the last row): sorted, the eighth
# and the ninth are equal (8202) -- the lower row (10) goes wide, row 13 and the shortest (15) stay in the stream
TEN = (8208, 8203, 8202, 8207, 8206, 8202, 8205, 8200, 8204, 8209)
BAND = (41, 700, 4100)


def _long_rows(rng, n, cut):
    """the rows of the `long` block; cut: four of the ten rows (the 8200, both 8202, the 8203) shortened into the band"""
    pool = np.arange(n)
    ten = [k if not (cut and k <= 8203) else k // 2 for k in TEN]
    lens = [8193, 8192, 1, 2, 7, 2046, 11, 2048] + ten[:9] + [5, 33] + list(BAND) + [ten[9]]
    return [_row(rng, pool, k) for k in lens]


def long_case(first_wide=False):
    """A = the 3-D operator on 13 x 13 x 19 (n = 9633: odd, ten windows of 1024), m = 23:
      row 0   8193 entries     row 1   8192 (over a tile, not wide)     rows 2, 3   1 and 2 entries
      row 5   2046 entries at Bc residue 3 (long)     row 7   2048 at residue 0 (fills a tile, not long)    (4, 6: fillers)
      rows 8-16 and 22   the ten rows of 8200..8209 (TEN)     rows 17-21   5, 33 and the band 41, 700, 4100
    Ten rows above row 0's length fill the cap of eight by themselves, so row 0 (8193 > 8192) cannot be wide in the same
    block: it stays in the stream as its longest row, with rows 13 and 15.  first_wide=True is the same block with four
    of the ten cut to half their length (band rows): seven wide rows, row 0 and row m - 1 among them, and row 0's 8193
    entries gone from Bc shift every residue behind it (row 5 comes to residue 2 and is tiled)."""
    A = S.AssembleOperator_Laplace3D(*LONG_GRID)[0]
    n = A.nrows
    return A, _block(_long_rows(np.random.default_rng(8193), n, first_wide), n)


def tall_case():
    """A = general_spd(1031), m = 2305 rows of 1-5 entries (more rows than columns; ten Bc tiles by the 256-row cap): every
    row holds column 5 (B^T row 5: 2305 entries, long), about 300 hold column 1030, columns 100..899 are untouched
    (whole tiles of empty B^T rows).  K is singular: products, S^ and PCApply only."""
    n, m = 1031, 2305
    A = general_spd(n, 1031)[0]
    rng = np.random.default_rng(2305)
    pool = np.concatenate([np.arange(0, 100), np.arange(900, 1030)])
    rows = []
    for r in range(m):
        k = 1 + r % 5
        must = [5, 1030] if (k >= 2 and r % 6 == 1) else [5]
        rows.append(_row(rng, pool, k, must=must))
    return A, _block(rows, n)


RANK_GRIDS = {2: (13, 13, 34), 3: (13, 13, 49)}


def rank_case(P):
    """z-slabs of the 3-D operator: 8619 | 8619 rows (P = 2), 8619 | 8112 | 8112 (P = 3).  Row a (0): 8193 entries on rank
    0.  Row b: 8193 on rank 0 and 100 on rank 1.  Row c (the last): 8192 on rank 0 and, for P = 2, 8193 on rank 1.  Three
    short rows per rank that live on that rank alone.  Returns (A, B, cuts)."""
    grid = RANK_GRIDS[P]
    A = S.AssembleOperator_Laplace3D(*grid)[0]
    n = A.nrows
    cuts = [S.partition_slab3d(*grid, r, P)[0] for r in range(P)] + [n]
    rng = np.random.default_rng(100 + P)
    own = [np.arange(cuts[r], cuts[r + 1]) for r in range(P)]

    def join(*parts):
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    shorts = [[_row(rng, own[r], int(k)) for k in (3, 17, 40)] for r in range(P)]
    a = _row(rng, own[0], 8193)
    b = join(_row(rng, own[0], 8193), _row(rng, own[1], 100))
    c = join(_row(rng, own[0], 8192), _row(rng, own[1], 8193)) if P == 2 else _row(rng, own[0], 8192)
    rows = [a] + shorts[0] + [b] + [s for r in range(1, P) for s in shorts[r]] + [c]
    return A, _block(rows, n), cuts


# --------------------------------------------------------------------------- sums over CSR arrays
def _rows(M):
    return np.repeat(np.arange(M.nrows), np.diff(M.rowptr))


def _sum_at(idx, terms, n, dtype=LD, reverse=False):
    """out[i] = the sum of terms[idx == i]: long double, or float64 added one by one in the stored (reversed) order"""
    out = np.zeros(n, dtype)
    terms = np.asarray(terms, dtype)
    if reverse:
        idx, terms = idx[::-1], terms[::-1]
    np.add.at(out, idx, terms)
    return out


def jacobi_d(A):
    """1 / diag(A) as the set-up takes it (the last diagonal entry of a row, a zero diagonal as 1)"""
    rows = _rows(A)
    d = np.zeros(A.nrows)
    on = A.colidx == rows
    d[rows[on]] = A.val[on]
    return 1.0 / np.where(d == 0.0, 1.0, d)


def _ranks(P):
    return P if P > 1 else 0


# --------------------------------------------------------------------------- K x, S^
def ref_mult(A, B, x, P=1):
    """K [x0; lam] in long double: (y0, y1, bar0, bar1)"""
    n, m = A.nrows, B.nrows
    x0, lam = np.asarray(x[:n], LD), np.asarray(x[n:], LD)
    ra, rb, cb = _rows(A), _rows(B), B.colidx.astype(np.int64)
    pa = A.val.astype(LD) * x0[A.colidx]
    qb = B.val.astype(LD) * lam[rb]
    y0 = _sum_at(ra, pa, n) + _sum_at(cb, qb, n)
    k0 = np.diff(A.rowptr) + np.bincount(cb, minlength=n)
    bar0 = gamma(k0) * (_sum_at(ra, np.abs(pa), n) + _sum_at(cb, np.abs(qb), n))
    pb = B.val.astype(LD) * x0[cb]
    y1 = _sum_at(rb, pb, m)
    bar1 = gamma(np.diff(B.rowptr) + _ranks(P)) * _sum_at(rb, np.abs(pb), m)
    return y0, y1, bar0, bar1


def f64_mult(A, B, x, reverse=False):
    n, m = A.nrows, B.nrows
    x0, lam = x[:n], x[n:]
    ra, rb, cb = _rows(A), _rows(B), B.colidx.astype(np.int64)
    bt = _sum_at(cb, B.val * lam[rb], n, np.float64, reverse)
    y0 = _sum_at(ra, A.val * x0[A.colidx], n, np.float64, reverse) + bt
    return np.concatenate([y0, _sum_at(rb, B.val * x0[cb], m, np.float64, reverse)])


def ref_shat(B, d, P=1):
    """S^ = diag(B D B^T) in long double from the float64 D: (shat, bar)"""
    rb = _rows(B)
    t = B.val.astype(LD) ** 2 * np.asarray(d, LD)[B.colidx]
    return _sum_at(rb, t, B.nrows), gamma(np.diff(B.rowptr) + 2 + _ranks(P)) * _sum_at(rb, np.abs(t), B.nrows)


def f64_shat(B, d, reverse=False):
    return _sum_at(_rows(B), B.val * B.val * d[B.colidx], B.nrows, np.float64, reverse)


# --------------------------------------------------------------------------- PCApply_FieldSplit_Schur
def _B_times(B, w, ew, c, P):
    """t = B w for a w known to ew: (t, its error bound); c = roundings of a term beyond its product"""
    rb, cb = _rows(B), B.colidx.astype(np.int64)
    bv = np.abs(B.val.astype(LD))
    t = _sum_at(rb, B.val.astype(LD) * w[cb], B.nrows)
    mag = _sum_at(rb, bv * (np.abs(w) + ew)[cb], B.nrows)
    return t, gamma(np.diff(B.rowptr) + c + _ranks(P)) * mag + _sum_at(rb, bv * ew[cb], B.nrows)


def _Bt_times(B, y1, e1, n):
    """c = B^T y1 for a y1 known to e1: (c, its error bound)"""
    rb, cb = _rows(B), B.colidx.astype(np.int64)
    bv = np.abs(B.val.astype(LD))
    c = _sum_at(cb, B.val.astype(LD) * y1[rb], n)
    mag = _sum_at(cb, bv * (np.abs(y1) + e1)[rb], n)
    return c, gamma(np.bincount(cb, minlength=n)) * mag + _sum_at(cb, bv * e1[rb], n)


def _y1_lower(x1, t, et, sh):
    """y1 = -(x1 - t) / S^: two roundings on top of t's error"""
    y1 = -(x1 - t) / sh
    return y1, (et + gamma(2) * (np.abs(x1) + np.abs(t) + et)) / sh


def ref_pc_apply(fact, B, d, sh, x, P=1):
    """The four factorisations as op_pc_apply states them (S~ = -S^), D and S^ the float64 arrays the device holds:
      DIAG   y0 = D x0                     y1 =  x1 / S^
      LOWER  y0 = D x0                     y1 = -(x1 - B D x0) / S^
      UPPER  y0 = D (x0 - B^T y1)          y1 = -x1 / S^
      FULL   y0 = D x0 - D (B^T y1)        y1 = -(x1 - B D x0) / S^
    Returns (y0, y1, bar0, bar1) in long double."""
    n = len(d)
    d, sh = np.asarray(d, LD), np.asarray(sh, LD)
    x0, x1 = np.asarray(x[:n], LD), np.asarray(x[n:], LD)
    zero = np.zeros(n, LD)
    if fact in (DIAG, UPPER):
        y1 = (x1 if fact == DIAG else -x1) / sh
        e1 = gamma(1) * np.abs(y1)
    else:
        t, et = _B_times(B, d * x0, zero, 1, P)
        y1, e1 = _y1_lower(x1, t, et, sh)
    if fact in (DIAG, LOWER):
        y0 = d * x0
        return y0, y1, gamma(1) * np.abs(y0), e1
    c, ec = _Bt_times(B, y1, e1, n)
    if fact == UPPER:      # (x0 - c) d
        y0 = (x0 - c) * d
    else:                  # x0 d - c d
        y0 = x0 * d - c * d
    e0 = np.abs(d) * ec + gamma(2) * np.abs(d) * (np.abs(x0) + np.abs(c) + ec)
    return y0, y1, e0, e1


def f64_pc_apply(fact, B, d, sh, x, reverse=False):
    n = len(d)
    x0, x1 = x[:n], x[n:]
    rb, cb = _rows(B), B.colidx.astype(np.int64)
    if fact in (DIAG, UPPER):
        y1 = (x1 if fact == DIAG else -x1) / sh
    else:
        y1 = -(x1 - _sum_at(rb, B.val * (d * x0)[cb], B.nrows, np.float64, reverse)) / sh
    if fact in (DIAG, LOWER):
        return np.concatenate([d * x0, y1])
    c = _sum_at(cb, B.val * y1[rb], n, np.float64, reverse)
    return np.concatenate([(x0 - c) * d if fact == UPPER else x0 * d - c * d, y1])


# --------------------------------------------------------------------------- with an inner solve
def _moved(ainv, v, ev, seed):
    """A^ ^-1 is not exactly linear (FP32 sweeps, a V-cycle): its result at float64(v), and ten times the largest movement
    of any component under three perturbations of v by +- its bound ev with random signs (0 where ev is 0: the same
    input gives the same bytes)."""
    v64 = np.asarray(v, np.float64)
    ev = np.asarray(ev, LD) + gamma(1) * np.abs(np.asarray(v, LD))      # the rounding of v to float64 is part of its bound
    z = ainv(v64)
    rng = np.random.default_rng(seed)
    mv = 0.0
    for _ in range(3):
        zp = ainv(np.asarray(np.asarray(v, LD) + rng.choice([-1.0, 1.0], len(v64)) * ev, np.float64))
        mv = max(mv, float(np.abs(zp - z).max()))
    return np.asarray(z, LD), mv


def ref_pc_apply_inner(fact, B, sh, x, ainv, P=1, seed=7):
    """The same block algebra with A^ ^-1 (ainv: float64 vector -> float64 vector, the context's own inner solve under
    PC_JACOBI) standing for D:
      DIAG   y0 = A^ x0                      y1 =  x1 / S^
      LOWER  y0 = A^ x0                      y1 = -(x1 - B y0) / S^
      UPPER  y0 = A^ (x0 - B^T y1)           y1 = -x1 / S^
      FULL   y0 = A^ x0 - A^ (B^T y1)        y1 = -(x1 - B (A^ x0)) / S^
    A^ x0 sees the same bytes as on the device: no allowance.  Where its input carries an error the allowance is measured
    on the reference (_moved).  Returns (y0, y1, bar0, bar1, movement): bar0 a scalar bound or an array."""
    n = len(x) - B.nrows
    sh = np.asarray(sh, LD)
    x0, x1 = np.asarray(x[:n], LD), np.asarray(x[n:], LD)
    zero = np.zeros(n, LD)
    mv = 0.0
    if fact == UPPER:
        y1 = -x1 / sh
        e1 = gamma(1) * np.abs(y1)
        c, ec = _Bt_times(B, y1, e1, n)
        v = x0 - c
        y0, mv = _moved(ainv, v, ec + gamma(1) * (np.abs(x0) + np.abs(c) + ec), seed)
        return y0, y1, 10 * mv + zero, e1, mv
    ya = np.asarray(ainv(np.asarray(x[:n], np.float64)), LD)
    if fact == DIAG:
        y1 = x1 / sh
        return ya, y1, zero, gamma(1) * np.abs(y1), mv
    t, et = _B_times(B, ya, zero, 0, P)
    y1, e1 = _y1_lower(x1, t, et, sh)
    if fact == LOWER:
        return ya, y1, zero, e1, mv
    c, ec = _Bt_times(B, y1, e1, n)
    z, mv = _moved(ainv, c, ec, seed)
    y0 = ya - z                                                         # one rounding: y0 -= A^ (B^T y1)
    return y0, y1, 10 * mv + gamma(1) * (np.abs(ya) + np.abs(z) + 10 * mv), e1, mv


# --------------------------------------------------------------------------- what a test reports
def worst(err, bar):
    """largest error / bar (an error on a zero bar counts as infinite)"""
    err, bar = np.asarray(err, LD), np.asarray(bar, LD) + np.zeros(np.shape(err), LD)
    r = np.where(bar > 0, err / np.where(bar > 0, bar, 1), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0
