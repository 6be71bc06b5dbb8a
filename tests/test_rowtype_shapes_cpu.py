"""The row-type layout (DictDev: row types + deviation codes) takes any CSR with 2x2 or 3x3 blocks, at most 32 blocks per
block row, at most 1024 row types and classes, and tables within 48 KB of LDS -- and the generator only ever gives it 9 and
27 blocks per row.  This file builds matrices off those two stencils: block rows of 1 to 33 blocks, arbitrary and far
column offsets, many classes and row types, and deviation widths chosen per class entry so that the matrix, not an
environment knob, decides the field layout.  Without a GPU it restates the set-up's rules (coarse_key, the class base, the
widths, dict_field_layout, dict_lds_bytes, dict_args' chunking, resident_lds_bytes) and shows that every case is what
test_gpu_rowtype_shapes.py takes it for; that module runs the device on the same matrices.

The values.  A block is an ideal block plus noise.  Ideal entries are multiples of 2^-10 of magnitude below 1, inside a
block pairwise 2^-9 or more apart, and two ideal blocks differ by 2^-9 or more in some entry; the noise stays below 2^-22.
coarse_key is rint(v 2^20): an ideal entry maps to a multiple of 2^10 and the noise moves v 2^20 by less than 1/4, so a
class is exactly the set of blocks of one ideal block -- never split, never merged.
noise[(offset or (offset, q), entry)] = (g, w) adds k 2^g to that entry of every member of the class (offset, variant q).
The set-up takes the class's FIRST member (lowest block index) as the base, so a member's code is (k - k_first); the
builder gives the first member k = 0, so the code is k itself.  The other members draw |k| < 2^(w-2), the last member
gets k = 2^(w-1) - 1 and the one before it -(2^(w-1) - 1): the largest |code| is 2^(w-1) - 1 exactly, an odd number, so
the granule found is 2^g and the width found (the smallest w' >= 2 with 2^(w'-1) - 1 >= max |code|) is w.  A (spd) diagonal
entry is below 128, so every value is a multiple of 2^-46 and k 2^g is added exactly for g >= -46."""
import numpy as np
import pytest

import saddle_point_petsc_amd as S

LDS_MAX, MAX_K, MAX_TYPES, MAX_CLASSES, CHUNK = 48 * 1024, 32, 1024, 1024, 256   # kDictLdsMax, kDictMaxK, kDictMaxPat, kDictMaxBlk, kDictChunk
G_DEFAULT = -44


# --------------------------------------------------------------------------- the builder
def _ideal_blocks(rng, count, bs):
    """count x bs x bs ideal blocks: entries +-m 2^-10 with m even in [2, 1022], distinct inside a block"""
    bb = bs * bs
    m = np.argsort(rng.random((count, 511)), axis=1)[:, :bb] * 2 + 2
    sign = rng.choice([-1.0, 1.0], (count, bb))
    return (sign * m * 2.0**-10).reshape(count, bs, bs)


def stencil_csr(dims, offsets, bs, blocks=None, noise=None, period=1, seed=0, spd=False):
    """The CSR of a block stencil on the node grid `dims` (natural ordering, the first index fastest), bs dofs per node:
    the block row of a node holds one dense bs x bs block per offset of `offsets` (node-index tuples; plain integers on a
    chain) whose target lies inside the grid, columns ascending, all bs*bs entries stored, the bs rows of a node with one
    pattern.  blocks[o]: the ideal block of offset o (drawn from `seed` where absent); period > 1: variant
    q = (node + index of the offset in ascending column order) % period of it, each variant a block of its own.
    noise: see the file's docstring.  spd: offsets in +- pairs around 0, blocks[-o] = blocks[o].T, the noise mirrored, the
    variant taken from the lower node of a pair, the diagonal entries above the absolute row sums: symmetric and strictly
    diagonally dominant with a positive diagonal, hence positive definite."""
    dims = tuple(int(d) for d in dims)
    nd, N = len(dims), int(np.prod(dims))
    stride = np.concatenate([[1], np.cumprod(dims[:-1])]).astype(np.int64)
    offs = [((int(o),) if np.isscalar(o) else tuple(int(v) for v in o)) for o in offsets]
    assert len(set(offs)) == len(offs) and all(len(o) == nd for o in offs)
    lin = np.array([int(np.dot(o, stride)) for o in offs], np.int64)
    order = np.argsort(lin, kind="stable")
    offs, lin = [offs[i] for i in order], lin[order]
    K, bb = len(offs), bs * bs
    index = {o: j for j, o in enumerate(offs)}
    rng = np.random.default_rng(seed)

    node = np.arange(N, dtype=np.int64)
    coord = [(node // stride[d]) % dims[d] for d in range(nd)]
    valid = np.ones((N, K), bool)
    for j, o in enumerate(offs):
        for d in range(nd):
            if o[d]:
                valid[:, j] &= (coord[d] + o[d] >= 0) & (coord[d] + o[d] < dims[d])
    bi, bj = np.nonzero(valid)                      # block -> (node, offset), in block-row order, columns ascending
    nblk = len(bi)
    posmap = np.full((N, K), -1, np.int64)
    posmap[bi, bj] = np.arange(nblk)
    cnt = valid.sum(1)

    # ---- ideal blocks ideal[j, q]
    ideal = _ideal_blocks(rng, K * period, bs).reshape(K, period, bs, bs)
    for o, blk in (blocks or {}).items():
        o = (int(o),) if np.isscalar(o) else tuple(o)
        ideal[index[o]] = np.asarray(blk, float)[None] + (np.arange(period) * 2.0**-9)[:, None, None] * (np.arange(bb).reshape(bs, bs) == 0)
    mirror = None
    if spd:
        mirror = np.array([index[tuple(-v for v in o)] for o in offs])
        j0 = index[(0,) * nd]
        for j in range(K):
            if lin[j] > 0:
                ideal[mirror[j]] = np.swapaxes(ideal[j], -1, -2)
        off_sum = np.abs(ideal).sum(-1).max(1)                       # [j, r]: the largest absolute row sum over the variants
        rows = off_sum.sum(0) - off_sum[j0]
        for q in range(period):
            D = np.triu(ideal[j0, q], 1)
            D = D + D.T
            D[np.arange(bs), np.arange(bs)] = rows + np.abs(D).sum(1) + 1.0 + (2 * q + np.arange(bs)) * 2.0**-9
            ideal[j0, q] = D
        assert np.abs(ideal).max() < 128.0
        sel = (np.minimum(bi, bi + lin[bj]) + np.minimum(bj, mirror[bj])) % period
    else:
        sel = (bi + bj) % period
    flat = np.round(ideal.reshape(K * period, bb) * 1024).astype(np.int64)
    assert len(np.unique(flat, axis=0)) == K * period, "two ideal blocks coincide"
    V = ideal[bj, sel].copy()                       # nblk x bs x bs

    # ---- noise
    for key, (g, w) in (noise or {}).items():
        cls, e = key
        o, qs = (cls[0], [cls[1]]) if isinstance(cls[0], tuple) else (cls, range(period))
        o = tuple(int(v) for v in o)
        j, r, c = index[o], e // bs, e % bs
        assert 2 <= w <= 31 and g >= -46 and g + w - 1 <= -22, (g, w)
        if spd:
            assert lin[j] >= 0, "spd: give the noise on the offsets of the upper triangle"
        for q in qs:
            mem = np.flatnonzero((bj == j) & (sel == q))
            assert len(mem) >= 3, "a class needs three members for a width to be exact"
            k = rng.integers(-(1 << (w - 2)) + 1, 1 << (w - 2), len(mem)).astype(np.float64)
            k[0], k[-1], k[-2] = 0.0, float((1 << (w - 1)) - 1), -float((1 << (w - 1)) - 1)
            dv = k * 2.0**g
            V[mem, r, c] += dv
            if spd and lin[j] > 0:
                V[posmap[bi[mem] + lin[j], mirror[j]], c, r] += dv
            elif spd and r != c:
                V[mem, c, r] += dv

    # ---- CSR: scalar row (node, r) = its blocks in order, a block's bs entries side by side
    start = np.concatenate([[0], np.cumsum(cnt)])
    kpos = np.arange(nblk) - start[bi]
    r_ = np.arange(bs)[None, :, None]
    c_ = np.arange(bs)[None, None, :]
    dest = bb * start[bi][:, None, None] + r_ * (cnt[bi] * bs)[:, None, None] + kpos[:, None, None] * bs + c_
    val = np.empty(nblk * bb)
    col = np.empty(nblk * bb, np.int32)
    val[dest.ravel()] = V.ravel()
    col[dest.ravel()] = np.broadcast_to((bs * (bi + lin[bj]))[:, None, None] + c_, dest.shape).ravel()
    rowptr = np.concatenate([[0], np.cumsum(np.repeat(cnt * bs, bs))])
    assert rowptr[-1] < 2**31
    return S.CSR(rowptr.astype(np.int32), col, val, bs * N)


def sparse_rows(n, m, seed=3, per_row=12):
    """m arbitrary sparse rows over n columns (an A10 block), columns unsorted"""
    rng = np.random.default_rng(seed + 31 * m)
    k = min(per_row, n)
    ci = np.concatenate([rng.choice(n, k, replace=False) for _ in range(m)])
    return S.CSR(np.arange(m + 1, dtype=np.int32) * k, ci.astype(np.int32), rng.uniform(0.2, 1.0, m * k) * rng.choice([-1, 1], m * k), n)


def vec(n, seed=41):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


# --------------------------------------------------------------------------- the set-up's rules restated
def blocks_of(A, bs):
    """(block row pointer, block column, nblk x bs*bs values) of a blockable CSR; asserts that it is blockable"""
    rp = A.rowptr.astype(np.int64)
    n = A.nrows
    assert n % bs == 0
    ln = np.diff(rp)
    assert np.all(ln.reshape(-1, bs) == ln.reshape(-1, bs)[:, :1]) and np.all(ln % bs == 0)
    cnt = ln[::bs] // bs
    brp = np.concatenate([[0], np.cumsum(cnt)])
    nblk = int(brp[-1])
    bi = np.repeat(np.arange(n // bs), cnt)
    kpos = np.arange(nblk) - brp[bi]
    r_ = np.arange(bs)[None, :, None]
    c_ = np.arange(bs)[None, None, :]
    src = (bs * bs * brp[bi])[:, None, None] + r_ * (cnt[bi] * bs)[:, None, None] + kpos[:, None, None] * bs + c_
    cols = A.colidx[src]
    assert np.all(cols == cols[:, :1, :1] + c_) and np.all(cols[:, 0, 0] % bs == 0)
    bcol = cols[:, 0, 0].astype(np.int64) // bs
    assert np.all((np.diff(bcol) > 0) | (np.diff(bi) > 0)), "columns ascend in a block row"
    return brp, bcol, A.val[src].reshape(nblk, bs * bs)


def coarse_key(v):
    assert np.all(np.abs(v) < 1e12)
    return np.rint(v * 1048576.0).astype(np.int64)


def classes_of(vals):
    """class of every block, numbered by first member as dict_number_classes does; the first members"""
    _, first, inv = np.unique(coarse_key(vals), axis=0, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[inv.ravel()], np.sort(first)


def row_types_of(brp, bcol, cls):
    """number of distinct (length, (column offset, class) ...) sequences, and the longest block row"""
    cnt = np.diff(brp)
    kmax, nbr = int(cnt.max()), len(cnt)
    bi = np.repeat(np.arange(nbr), cnt)
    kpos = np.arange(len(bcol)) - brp[bi]
    key = np.full((nbr, 2 * kmax + 1), np.iinfo(np.int64).min, np.int64)
    key[:, 0] = cnt
    key[bi, 1 + 2 * kpos] = bcol - bi
    key[bi, 2 + 2 * kpos] = cls
    return len(np.unique(key, axis=0)), kmax


def widths_of(vals, cls, first):
    """dict_cls_stats + dict_field_widths: per (class, entry) the granule exponent (None: nobody deviates) and the width;
    asserts that every deviation from the class's first member is exactly representable"""
    base = vals[first][cls]
    dv = vals - base
    assert np.array_equal(base + dv, vals)
    # v and base are multiples of 2^-46 below 2^7: v - base is exact (a multiple of 2^-46 below 2^8)
    assert np.array_equal(np.rint(vals * 2.0**46) - np.rint(base * 2.0**46), dv * 2.0**46)
    ncls, bb = len(first), vals.shape[1]
    mant, ex = np.frexp(np.abs(dv))
    M = np.rint(mant * 2.0**53).astype(np.int64)
    low = ex - 53 + np.log2(np.where(M > 0, M & -M, 1)).astype(np.int64)
    gexp = np.full((ncls, bb), 10**6, np.int64)
    dmax = np.zeros((ncls, bb))
    for e in range(bb):
        nz = dv[:, e] != 0
        np.minimum.at(gexp[:, e], cls[nz], low[nz, e])
        np.maximum.at(dmax[:, e], cls, np.abs(dv[:, e]))
    width = np.ones((ncls, bb), np.int64)
    some = gexp < 10**6
    kabs = np.where(some, dmax / 2.0**np.where(some, gexp, 0), 0.0)
    assert np.all(kabs <= 1.0e9)
    width[some] = np.maximum(2, np.ceil(np.log2(kabs[some] + 1)).astype(np.int64) + 1)
    return np.where(some, gexp, 10**6), width


def field_layout(bs, width):
    """dict_field_layout: (uniform, straddle, uniform3, refused)"""
    uw = np.maximum(1, width.max(0))
    uniform = bs == 2 and uw[0] + uw[1] <= 32 and uw[2] + uw[3] <= 32
    uniform3 = 0
    if bs == 3:
        for split, w1 in ((1, (5, 6, 7, 8)), (2, (4, 5, 6, 7, 8)), (3, (4, 6, 7, 8))):
            hi = sum(int(uw[e]) for e in w1)
            if hi <= 64 and int(uw.sum()) - hi <= 64:
                uniform3 = split
                break
    straddle = refused = False
    for w in width:
        if bs == 2 and not uniform and not (w[0] + w[1] <= 32 and w[2] + w[3] <= 32) and w.sum() <= 64:
            sh = 0
            for e in range(4):
                straddle |= bool(sh < 32 and sh + w[e] > 32)
                sh += w[e]
            continue
        if uniform or uniform3:
            continue
        used, word, cap = [0, 0], 0, 32 if bs == 2 else 64
        for e in range(bs * bs):
            if used[word] + w[e] > cap:
                word += 1
            if word > 1:
                refused = True
                break
            used[word] += w[e]
    return bool(uniform), straddle, uniform3, refused


def lds_bytes(ntype, kmax, ncls, bs):
    tab_ints = ((ntype + 1) & ~1) + 2 * ntype * kmax
    return ((((4 * tab_ints + 15) & ~15) + 20 * (ncls + 1) * bs * bs) + 15) & ~15


def chunking(nbrows, bs, kmax):
    """dict_args: (nchunks, chunks_per_wg, chunks_per_xcd, workgroups)"""
    nchunks = (nbrows + CHUNK - 1) // CHUNK
    cpw = max(1, nchunks // (512 if bs == 2 and kmax == 9 else 2048))
    cpx = ((nchunks + 7) // 8 + cpw - 1) // cpw * cpw
    return nchunks, cpw, cpx, 8 * (cpx // cpw)


def resident_lds(lds, kmax, T):
    """resident_lds_bytes (spk_k_resident.hip): tables, kmax code words per thread, kResPass = 20 staging rows of T + 8
    doubles, 1022 doubles of scalar work space, KrylovState (10 ints + 10 doubles = 120 B), 64 B of flags"""
    return ((lds + 15) & ~15) + kmax * T * 8 + (20 * (T + 8) + 128 + 32 + 68 + 34 * 5 + 32 * 8 * 2 + 8 * 6 + 64) * 8 + 120 + 64


def resident_takes(nbrows, lds, kmax, cus=256):
    G = min(min(cus, 256), (nbrows + 63) // 64)
    rpw = (nbrows + G - 1) // G
    return rpw <= 512 and resident_lds(lds, kmax, 256 if rpw <= 256 else 512) <= 160 * 1024


def analyse(A, bs):
    brp, bcol, vals = blocks_of(A, bs)
    cls, first = classes_of(vals)
    ntype, kmax = row_types_of(brp, bcol, cls)
    gexp, width = widths_of(vals, cls, first)
    uniform, straddle, uniform3, refused = field_layout(bs, width)
    return dict(nbrows=len(brp) - 1, kmax=kmax, ntype=ntype, nclass=len(first), gexp=gexp, width=width, uniform=uniform,
                straddle=straddle, uniform3=uniform3, refused=refused, lds=lds_bytes(ntype, kmax, len(first), bs), first=first,
                cls=cls)


# --------------------------------------------------------------------------- the cases
def _box(r, nd):
    return [tuple(o) for o in np.stack(np.meshgrid(*[np.arange(-r, r + 1)] * nd, indexing="ij"), -1).reshape(-1, nd)]


O8 = [-1000, -3, -1, 0, 1, 2, 7, 1000]
O10 = O8 + [-2, 5]
O11 = O10 + [11]
O12 = list(range(-5, 7))
FAR9 = [-1000, -37, -5, -1, 0, 2, 11, 300, 1000]
# twelve / ten blocks with +- pairs (spd): a strip of two grid lines, of which every node has one neighbour line
STRIP12 = [(a, 0) for a in range(-3, 4)] + [(b, s) for s in (-1, 1) for b in range(-2, 3)]
STRIP10 = [(a, 0) for a in range(-2, 3)] + [(b, s) for s in (-1, 1) for b in range(-2, 3)]
CUBE = _box(1, 3)
T27X = [-1000, -611, -300, -150, -77, -40, -21, -13, -8, -5, -3, -2, -1, 0, 1, 2, 4, 6, 9, 15, 30, 55, 99, 170, 420, 800, 1000]
Z10 = (0, 0)          # the offset whose class carries the widths of s1 .. rfit3, and a second one
P10 = (1, 0)


def _all_entries(o, widths, g=G_DEFAULT):
    return {(o, e): (g, w) for e, w in enumerate(widths) if w > 1}


# name -> (bs, builder arguments, expected: kmax, accepted, product kernel, uniform, straddle, uniform3)
CASES = {}


FILL = (-34, 12)      # codes of up to 2^-23: seen by the FP32 sweeps too (a value below 1 has 2^-25 or finer there)


def _case(name, bs, dims, offsets, kmax, ok=True, kernel=0, uniform=None, straddle=0, uniform3=None, fill=FILL, **kw):
    """fill: every offset the case gives no noise (spd: every such offset of the upper triangle) gets this (g, w) on one
    entry, so that no block of the matrix has all-zero codes -- a kernel that reads another block's code word is seen"""
    uniform = (1 if bs == 2 else 0) if uniform is None else uniform
    uniform3 = (1 if bs == 3 else 0) if uniform3 is None else uniform3
    if fill:
        stride = np.concatenate([[1], np.cumprod(dims[:-1])])
        tup = [((int(o),) if np.isscalar(o) else tuple(int(v) for v in o)) for o in offsets]
        noisy = {key[0] for key in kw.get("noise", {})}
        noise = dict(kw.get("noise", {}))
        for j, o in enumerate(tup):
            if o not in noisy and (not kw.get("spd") or np.dot(o, stride) >= 0):
                noise[o, j % (bs * bs)] = fill
        kw["noise"] = noise
    CASES[name] = dict(bs=bs, args=(dims, offsets, bs), kw=kw, kmax=kmax, ok=ok, kernel=kernel, uniform=uniform,
                       straddle=straddle, uniform3=uniform3)


for nb in (255, 256, 257):
    _case(f"k1_{nb}", 2, (nb,), [0], 1)
_case("k2_1", 2, (1,), [0, 1], 1, fill=None)
_case("k2", 2, (300,), [0, 1], 2, noise={((0,), 0): (G_DEFAULT, 9), ((1,), 3): (G_DEFAULT, 12)})
_case("k8", 2, (2049,), O8, 8, noise={((-1000,), 1): (G_DEFAULT, 11), ((7,), 2): (-46, 17)})
_case("k10", 2, (2049,), O10, 10, noise={((-1000,), 1): (G_DEFAULT, 11), ((5,), 2): (-46, 17)})
# (the eleventh block, offset +1000, is the second group and the half plane: its codes reach 2^-23, which the FP32 sweep sees)
_case("k11", 2, (2049,), O11, 11, noise={((1000,), 0): (-35, 13), ((11,), 3): (-46, 19), ((0,), 1): (G_DEFAULT, 6)})
_case("k12", 2, (700,), O12, 12, noise={((6,), 0): (G_DEFAULT, 13), ((-5,), 3): (-46, 19)})
_case("k31", 2, (700,), list(range(-15, 16)), 31, noise={((15,), 2): (G_DEFAULT, 10), ((-15,), 1): (-46, 18)})
_case("k32", 2, (700,), list(range(-15, 17)), 32, noise={((16,), 2): (G_DEFAULT, 10), ((-15,), 1): (-46, 18)})
_case("box25", 2, (37, 29), _box(2, 2), 25, spd=True, noise={((0, 0), 1): (G_DEFAULT, 8), ((2, 1), 2): (G_DEFAULT, 14)})
_case("k12s", 2, (350, 2), STRIP12, 12, spd=True, noise={((0, 0), 0): (G_DEFAULT, 9), ((1, 1), 1): (G_DEFAULT, 12)})
_case("far9", 2, (4000,), FAR9, 9, kernel=1, noise={((300,), 0): (G_DEFAULT, 13), ((-1000,), 3): (-46, 19)})
_case("far9p", 2, (4000,), FAR9, 9, kernel=1, period=4, noise={((300,), 0): (G_DEFAULT, 13), ((-1000,), 3): (-46, 19)})
# cls2: two classes wide in different entries -- 20 + 14 > 32 in the low half over all classes, 20 + 10 and 4 + 14 per class
_case("cls2", 2, (700,), O12, 12, uniform=0,
      noise={((0,), 0): (G_DEFAULT, 20), ((0,), 1): (G_DEFAULT, 10), ((0,), 2): (G_DEFAULT, 4), ((0,), 3): (G_DEFAULT, 4),
             ((1,), 0): (G_DEFAULT, 4), ((1,), 1): (G_DEFAULT, 14), ((1,), 2): (G_DEFAULT, 4), ((1,), 3): (G_DEFAULT, 4)})
_case("str12", 2, (700,), O12, 12, uniform=0, straddle=1, noise=_all_entries((0,), [20, 14, 14, 13], -46))
# (period 3: 256 % 3 != 0, so a thread's row type changes from chunk to chunk -- what the prefetch of the next type must follow)
_case("big2", 2, (1049361,), [0, 1], 2, period=3, noise={((1,), 0): (G_DEFAULT, 7)})
_case("t7", 3, (13, 13, 12), [o for o in CUBE if sum(abs(v) for v in o) <= 1], 7, noise={((0, 0, 1), 4): (G_DEFAULT, 9)})
_case("t9", 3, (45, 45), _box(1, 2), 9, noise={((1, 1), 8): (G_DEFAULT, 9)})
_case("t10", 3, (1000, 2), STRIP10, 10, noise={(P10, 2): (G_DEFAULT, 11), (Z10, 7): (-46, 15)})
_case("t10s", 3, (1000, 2), STRIP10, 10, spd=True, noise={(P10, 2): (G_DEFAULT, 11), (Z10, 1): (G_DEFAULT, 9)})
_case("t28", 3, (13, 13, 12), CUBE + [(2, 0, 0)], 28, noise={((2, 0, 0), 0): (G_DEFAULT, 9)})
_case("t32", 3, (13, 13, 12), CUBE + [(2, 0, 0), (-2, 0, 0), (0, 2, 0), (0, -2, 0), (0, 0, 2)], 32,
      noise={((0, 0, 2), 5): (G_DEFAULT, 12)})
_case("t27x", 3, (3000,), T27X, 27, noise={((800,), 3): (G_DEFAULT, 12), ((-611,), 8): (-46, 16)})
_case("s1", 3, (1000, 2), STRIP10, 10, uniform3=1, fill=(-30, 7), noise=_all_entries(Z10, [7] * 9))
_case("s2", 3, (1000, 2), STRIP10, 10, uniform3=2, fill=(-30, 8), noise=_all_entries(Z10, [16, 16, 16, 16, 16, 8, 8, 8, 8]))
_case("s3", 3, (1000, 2), STRIP10, 10, uniform3=3, fill=(-30, 8), noise=_all_entries(Z10, [14, 14, 14, 14, 22, 8, 14, 14, 14]))
_case("pc3", 3, (1000, 2), STRIP10, 10, uniform3=0,
      noise={**_all_entries(Z10, [20, 20, 20, 20, 1, 1, 1, 1, 1]), **_all_entries(P10, [1, 1, 1, 1, 20, 20, 20, 20, 20])})
_case("big3", 3, (1049361,), [0], 1, period=3)
_case("r33", 2, (700,), list(range(-16, 17)), 33, ok=False)
_case("rlds", 2, (3000,), list(range(-15, 17)), 32, ok=False, period=15)
# (a heavy diagonal block: nlds is solved with, too)
_case("nlds", 2, (3000,), list(range(-15, 17)), 32, period=14, noise={((16,), 2): (G_DEFAULT, 10)},
      blocks={(0,): [[64.0, 0.25], [-0.5, 65.0]]})
_case("rfit3", 3, (1000, 2), STRIP10, 10, ok=False, uniform3=0, noise=_all_entries(Z10, [20] * 9))
# the resident cycle beyond 65 536 block rows (512 threads per workgroup): see test_resident_budget_decides_by_kmax
_case("k12s_res", 2, (32896, 2), STRIP12, 12, spd=True, noise={((0, 0), 0): (G_DEFAULT, 9)})
_case("box25_res", 2, (257, 256), _box(2, 2), 25, spd=True, noise={((0, 0), 1): (G_DEFAULT, 8)})
_case("k12s_amg", 2, (2000, 2), STRIP12, 12, spd=True, noise={((0, 0), 0): (G_DEFAULT, 9), ((1, 1), 1): (G_DEFAULT, 12)})

SPD = [n for n, c in CASES.items() if c["kw"].get("spd")]
_built = {}


def build(name):
    """the matrix of a case (kept: the GPU module's tests share it)"""
    if name not in _built:
        c = CASES[name]
        _built[name] = stencil_csr(*c["args"], seed=sum(map(ord, name)), **c["kw"])
    return _built[name]


_analysed = {}


def analysed(name):
    if name not in _analysed:
        _analysed[name] = analyse(build(name), CASES[name]["bs"])
    return _analysed[name]


# --------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", list(CASES))
def test_case_is_what_the_gpu_tests_take_it_for(name):
    """blockable, the stated longest block row, row types and classes within the tables, the stated side of the LDS budget,
    exact deviations of the widths asked for, and the field layout the rules give those widths"""
    c, a = CASES[name], analysed(name)
    assert a["kmax"] == c["kmax"]
    assert a["ntype"] <= MAX_TYPES and a["nclass"] <= MAX_CLASSES, (a["ntype"], a["nclass"])
    fits = a["kmax"] <= MAX_K and a["lds"] <= LDS_MAX and not a["refused"]
    assert fits == c["ok"], (a["kmax"], a["lds"], a["refused"])
    if name == "r33":
        assert a["kmax"] == MAX_K + 1
    if name == "rlds":
        assert a["lds"] > LDS_MAX and a["kmax"] <= MAX_K and not a["refused"]
    if name == "nlds":
        assert 0.8 * LDS_MAX <= a["lds"] <= LDS_MAX, a["lds"]
    if name == "rfit3":
        assert a["refused"] and a["lds"] <= LDS_MAX
    if c["ok"]:
        assert (int(a["uniform"]), int(a["straddle"]), a["uniform3"]) == (c["uniform"], c["straddle"], c["uniform3"])
    # the widths asked for are the widths found, with the granule asked for; every other entry has no deviation at all
    dims, offsets, bs = c["args"]
    if not c["kw"].get("spd"):
        A = build(name)
        brp, bcol, vals = blocks_of(A, bs)
        asked = {}
        stride = np.concatenate([[1], np.cumprod(dims[:-1])])
        for (cls, e), (g, w) in c["kw"].get("noise", {}).items():
            asked[int(np.dot(cls, stride)), e] = (g, w)
        bi = np.repeat(np.arange(len(brp) - 1), np.diff(brp))
        off_of_class = (bcol - bi)[a["first"]]
        found = 0
        for cl in range(a["nclass"]):
            for e in range(bs * bs):
                g, w = asked.get((int(off_of_class[cl]), e), (10**6, 1))
                assert (a["gexp"][cl, e], a["width"][cl, e]) == (g, w), (name, cl, e)
                found += w > 1
        assert found == len(asked) * c["kw"].get("period", 1)


def test_the_paths_the_cases_are_named_for():
    """what the case table promises about chunking, the pipelined kernel's table pass and the widths' sums"""
    assert chunking(2049, 2, 8) == (9, 1, 2, 16)                      # k8 .. k11: 16 workgroups for 9 chunks, some run empty
    assert chunking(1049361, 2, 2) == (4100, 2, 514, 2056)            # big2: two chunks per workgroup, 514 per XCD run
    assert chunking(1049361, 3, 1)[1:3] == (2, 514)                   # big3
    assert 8 * 514 - 4100 == 12 and 1049361 % CHUNK == 17             # a short last XCD run, a ragged last chunk
    for name in ("big2", "big3"):                                    # a thread's row type differs from chunk to chunk
        first = blocks_of(build(name), CASES[name]["bs"])[0][:-1]    # (the class of a row's first block is part of its type)
        c = analysed(name)["cls"][first]
        assert np.all(c[:-CHUNK - 1] != c[CHUNK:-1])
    far9, far9p = analysed("far9"), analysed("far9p")
    assert far9["ntype"] * 9 <= 256 and (far9["nclass"] + 1) * 4 <= 256 and far9["ntype"] <= 28     # Dict2TableWords::fits
    assert far9p["ntype"] > 28
    w = analysed("cls2")["width"]
    assert w.max(0)[0] + w.max(0)[1] > 32 and all(r[0] + r[1] <= 32 and r[2] + r[3] <= 32 for r in w)
    w = analysed("str12")["width"]
    assert sorted(map(tuple, w), key=sum)[-1] == (20, 14, 14, 13)
    # box25: {3, 4, 5} x {3, 4, 5} blocks per row -- 25 row types of six lengths
    assert analysed("box25")["ntype"] == 25 and set(np.diff(blocks_of(build("box25"), 2)[0])) == {9, 12, 15, 16, 20, 25}
    assert analysed("pc3")["width"].max(0).sum() == 180 and analysed("rfit3")["width"].max() == 20


def test_resident_budget_decides_by_kmax():
    """Beyond 65 536 block rows a workgroup of the resident cycle has 512 threads: 91 376 + 184 B of its 160 KB are fixed,
    kmax * 4096 B hold the code words, the rest the tables -- kmax <= 16 fits with tables up to 6 736 B, kmax = 17 only with
    tables up to 2 640 B, and 25 never.  Up to 65 536 block rows (256 threads) kmax = 32 fits with tables up to 47 696 B
    of the 48 KB a layout may have."""
    assert resident_lds(0, 0, 512) == 91376 + 184
    assert resident_lds(6736, 16, 512) <= 160 * 1024 < resident_lds(6752, 16, 512)
    assert resident_lds(2640, 17, 512) <= 160 * 1024 < resident_lds(2656, 17, 512)
    assert resident_lds(47696, 32, 256) <= 160 * 1024 < resident_lds(47712, 32, 256)
    a, b = analysed("k12s_res"), analysed("box25_res")
    assert a["nbrows"] == b["nbrows"] == 65792 > 65536
    assert resident_takes(a["nbrows"], a["lds"], a["kmax"]) and not resident_takes(b["nbrows"], b["lds"], b["kmax"])
    assert b["lds"] < 72280 < b["kmax"] * 4096                        # the code words alone are over
    for name in ("box25", "k12s"):
        s = analysed(name)
        assert resident_takes(s["nbrows"], s["lds"], s["kmax"])


@pytest.mark.parametrize("name", SPD)
def test_spd_variants_are_symmetric_and_dominant(name):
    A = build(name)
    import scipy.sparse as sp
    M = sp.csr_matrix((A.val, A.colidx, A.rowptr), shape=(A.nrows, A.ncols))
    assert (M - M.T).nnz == 0 or abs(M - M.T).max() == 0.0
    d = M.diagonal()
    assert np.all(d > 0) and np.all(d > np.asarray(abs(M).sum(1)).ravel() - d)


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_product_is_the_sequential_csr_loop(oracle, name):
    """oracle.spmv = the CSR-order float64 loop bit for bit (a subsample of rows), and within len 2^-53 sum|a||x| of the
    longdouble sum: L - 1 additions and L roundings of products, each below 2^-53 of the partial sums' magnitude bound"""
    assert np.finfo(np.longdouble).nmant > np.finfo(np.float64).nmant
    A = build(name)
    x = vec(A.ncols)
    y = oracle.spmv(A, x)
    rows = np.unique(np.concatenate([np.arange(min(A.nrows, 40)), np.arange(max(A.nrows - 40, 0), A.nrows),
                                     np.random.default_rng(1).integers(0, A.nrows, 200)]))
    for r in rows:
        k0, k1 = int(A.rowptr[r]), int(A.rowptr[r + 1])
        s = 0.0
        for a, xc in zip(A.val[k0:k1].tolist(), x[A.colidx[k0:k1]].tolist()):
            s += a * xc
        assert s == y[r]
        ld = np.sum(A.val[k0:k1].astype(np.longdouble) * x[A.colidx[k0:k1]].astype(np.longdouble))
        bound = (k1 - k0) * 2.0**-53 * float(np.sum(np.abs(A.val[k0:k1] * x[A.colidx[k0:k1]])))
        assert abs(float(np.longdouble(y[r]) - ld)) <= bound * (1 + 2.0**-50)
