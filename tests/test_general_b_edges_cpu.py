"""The general constraint block at the edges of its three paths, without a GPU: every case of _general_b_cases.py holds
the classes of rows it was built for (counted from the rules restated there), and a plain float64 evaluation of every
operation -- the sums taken one by one in the stored order and in the reversed order -- stays inside the derived bars
against the long-double reference, before any kernel is asked (test_gpu_general_b_edges.py runs the device on the same
inputs, to the same bars).  wide_rows itself is checked at the same lengths by tests/host/setup_host_check.cpp."""
import numpy as np
import pytest

import _general_b_cases as G
from _cb_fgmres import fgmres_textbook
from test_stream_edges_cpu import CSR_ROWS, CSR_TILE

ONE_RANK = {"small": G.small_case, "long": G.long_case, "long_first_wide": lambda: G.long_case(True), "tall": G.tall_case}


@pytest.fixture(scope="module")
def cases():
    return {name: build() for name, build in ONE_RANK.items()}


@pytest.fixture(scope="module")
def rank_cases():
    return {P: G.rank_case(P) for P in (2, 3)}


def test_long_double_is_wider_than_double():
    assert np.finfo(G.LD).eps <= 2.0 ** -63


# --------------------------------------------------------------------------- the classes
def test_small_holds_its_classes(cases):
    A, B = cases["small"]
    assert A.nrows == 1031 and B.nrows == 9 and B.ncols == 1031
    ends = [int(B.colidx[B.rowptr[r]:B.rowptr[r + 1]].max()) for r in range(9)]
    assert ends[1:5] == [0, 1023, 1024, 1030] and np.diff(B.rowptr)[1] == 1
    row0 = B.colidx[:B.rowptr[1]]
    assert (np.diff(row0) < 0).any() and len(set(row0.tolist())) == len(row0)
    c = G.classes(B)
    assert c["layout"] == dict(general=True, m_wide=0, wide_rows=[], win=1024, nwin=0, bc_tiles=1, bt_tiles=5)
    assert not c["long"].any() and not c["bt_long"].any() and 1031 - 1024 == 7


def test_long_holds_its_classes(cases):
    A, B = cases["long"]
    n, m = A.nrows, B.nrows
    assert n == 9633 and n % 2 == 1 and m == 23 and (np.diff(B.rowptr) > 0).all()
    c = G.classes(B)
    lens, res = c["lens"], c["res"]
    assert c["layout"]["win"] == 1024 and c["layout"]["nwin"] == 10 and c["layout"]["general"]
    # ten rows of 8200..8209, two equal at the eighth place: eight go wide (ties to the lower row), the last row among them
    ten = np.flatnonzero(lens >= 8200)
    assert len(ten) == 10 and sorted(lens[ten])[1:3] == [8202, 8202] and set(lens[ten]) == set(range(8200, 8210)) - {8201}
    assert c["layout"]["wide_rows"] == [8, 9, 10, 11, 12, 14, 16, 22] and lens[10] == lens[13] == 8202 and lens[15] == 8200
    assert c["wide"][m - 1]
    # above the threshold and yet in the stream: the ninth and the tenth of the ten, and row 0 (8193)
    assert list(np.flatnonzero(c["over"])) == [0, 13, 15] and lens[0] == G.WIDE + 1 and lens[1] == G.WIDE
    # the stream's long rows, with the residue their first entry sits at
    assert list(np.flatnonzero(c["long"])) == [0, 1, 5, 13, 15, 21]
    assert (lens[5], res[5]) == (CSR_TILE - 2, 3) and (lens[7], res[7]) == (CSR_TILE, 0) and not c["long"][7]
    assert lens[2] == 1 and lens[3] == 2 and [lens[r] for r in (19, 20, 21)] == list(G.BAND)
    assert {int(res[r]) for r in np.flatnonzero(c["long"])} >= {0, 1, 3}
    # B^T: 23 entries a row at the most, tiles closed by their 256 rows or their 2048 entries
    assert not c["bt_long"].any() and c["layout"]["bt_tiles"] >= n // CSR_ROWS


def test_long_first_wide_holds_its_classes(cases):
    """four of the ten cut into the band: row 0 (8193) is wide now, with the last row; its entries gone from Bc, every
    residue behind it moves by one -- row 5 (2046 entries) comes to residue 2 and is tiled, row 7 (2048) to residue 3 and is
    long: the rule is applied to Bc's pointers, not to B's"""
    _, B = cases["long_first_wide"]
    c, c0 = G.classes(B), G.classes(cases["long"][1])
    m = B.nrows
    assert c["layout"]["wide_rows"] == [0, 8, 11, 12, 14, 16, m - 1] and not c["over"].any()
    assert c["lens"][1] == G.WIDE and not c["wide"][1]                      # strictly more than 8192, with the cap not full
    assert (c["res"][5], bool(c["long"][5])) == (2, False) and (c["res"][7], bool(c["long"][7])) == (3, True)
    assert (c0["res"][5], bool(c0["long"][5])) == (3, True) and (c0["res"][7], bool(c0["long"][7])) == (0, False)
    band = [r for r in range(m) if 40 < c["lens"][r] <= G.WIDE]
    assert len(band) >= 9 and sum(c["long"][band]) >= 6 and sum(~c["long"][band]) >= 2


def test_tall_holds_its_classes(cases):
    A, B = cases["tall"]
    n, m = A.nrows, B.nrows
    assert (n, m) == (1031, 2305) and m > n
    c = G.classes(B)
    lens = c["lens"]
    assert lens.min() == 1 and lens.max() == 5 and not c["wide"].any() and not c["long"].any()
    assert c["layout"]["bc_tiles"] == 10 and c["layout"]["m_wide"] == 0 and c["layout"]["nwin"] == 0
    per_col = np.diff(c["trp"])
    assert per_col[5] == m and list(np.flatnonzero(c["bt_long"])) == [5]          # B^T row 5: more than 2048 entries
    assert 280 <= per_col[1030] <= 330 and (per_col[100:900] == 0).all()
    assert c["bt_empty_tiles"] >= 2
    assert 5 in c["bt_tiles"] and 6 in c["bt_tiles"]                                # the long row has a tile of its own


@pytest.mark.parametrize("P", [2, 3])
def test_rank_cases_hold_their_classes(rank_cases, P):
    A, B, cuts = rank_cases[P]
    m = B.nrows
    assert np.diff(cuts).tolist() == ([8619, 8619] if P == 2 else [8619, 8112, 8112]) and m == 3 + 3 * P
    a, b, c = 0, 4, m - 1
    per = [G.classes(B, cuts[r], cuts[r + 1]) for r in range(P)]
    assert [int(p["lens"][a]) for p in per] == [8193] + [0] * (P - 1)
    assert [int(p["lens"][b]) for p in per] == [8193, 100] + [0] * (P - 2)
    assert [int(p["lens"][c]) for p in per] == ([8192, 8193] if P == 2 else [8192, 0, 0])
    assert [p["layout"]["wide_rows"] for p in per] == ([[a, b], [c]] if P == 2 else [[a, b], [], []])
    assert [p["layout"]["nwin"] for p in per] == ([9, 9] if P == 2 else [9, 0, 0])
    assert per[0]["long"][c] and not per[0]["wide"][c] and not per[1]["long"][b]   # 8192: the stream's long path; 100: tiled
    assert (np.diff(B.rowptr) > 0).all()
    shorts = [r for r in range(m) if r not in (a, b, c)]
    homes = [[r for r in shorts if per[k]["lens"][r] > 0] for k in range(P)]
    assert all(len(h) == 3 for h in homes) and len({r for h in homes for r in h}) == 3 * P      # each lives on one rank


# --------------------------------------------------------------------------- float64 inside the bars
def _x(A, B, seed):
    return G.vec(A.nrows + B.nrows, seed)


@pytest.mark.parametrize("name", list(ONE_RANK))
def test_float64_products_and_shat_stay_inside_the_bars(cases, name):
    A, B = cases[name]
    n = A.nrows
    x = _x(A, B, 11)
    d = G.jacobi_d(A)
    y0, y1, b0, b1 = G.ref_mult(A, B, x)
    sh, bs = G.ref_shat(B, d)
    assert (sh > 0).all()
    for rev in (False, True):
        y = G.f64_mult(A, B, x, rev)
        w0, w1 = G.worst(np.abs(y[:n] - y0), b0), G.worst(np.abs(y[n:] - y1), b1)
        ws = G.worst(np.abs(G.f64_shat(B, d, rev) - sh), bs)
        print(f"{name}, reversed {rev}: K x rows of A {w0:.3g}, rows of B {w1:.3g}, S^ {ws:.3g} of the bar")
        assert w0 <= 1 and w1 <= 1 and ws <= 1


@pytest.mark.parametrize("P", [2, 3])
def test_float64_on_ranks_stays_inside_the_bars(rank_cases, P):
    """every rank's share summed on its own, the shares added in rank order and in the reversed order"""
    A, B, cuts = rank_cases[P]
    n, m = A.nrows, B.nrows
    x = _x(A, B, 12)
    d = G.jacobi_d(A)
    _, y1, _, b1 = G.ref_mult(A, B, x, P)
    sh, bs = G.ref_shat(B, d, P)
    for rev in (False, True):
        t, s = np.zeros(m), np.zeros(m)
        for r in (range(P - 1, -1, -1) if rev else range(P)):
            Bs = B.col_slab(cuts[r], cuts[r + 1])
            t = t + G.f64_mult(A, Bs, x, rev)[n:]
            s = s + G.f64_shat(Bs, d, rev)
        assert G.worst(np.abs(t - y1), b1) <= 1 and G.worst(np.abs(s - sh), bs) <= 1


@pytest.mark.parametrize("fact", G.FACTS)
@pytest.mark.parametrize("name", list(ONE_RANK))
def test_float64_pc_apply_stays_inside_the_bars(cases, name, fact):
    A, B = cases[name]
    n = A.nrows
    x = _x(A, B, 13)
    d = G.jacobi_d(A)
    sh = G.f64_shat(B, d)
    y0, y1, b0, b1 = G.ref_pc_apply(fact, B, d, sh, x)
    for rev in (False, True):
        z = G.f64_pc_apply(fact, B, d, sh, x, rev)
        w0, w1 = G.worst(np.abs(z[:n] - y0), b0), G.worst(np.abs(z[n:] - y1), b1)
        print(f"{name}, fact {fact}, reversed {rev}: y0 {w0:.3g}, y1 {w1:.3g} of the bar")
        assert w0 <= 1 and w1 <= 1


def test_float64_inner_chain_stays_inside_the_bars(cases):
    """the chain with an inner solve, a float32 diagonal scaling standing for the sweeps (not linear in float64: it
    rounds its input): the float64 evaluation, either order, inside the measured allowance"""
    A, B = cases["long"]
    n = A.nrows
    x = _x(A, B, 14)
    d = G.jacobi_d(A)
    sh = G.f64_shat(B, d)
    d32 = d.astype(np.float32)
    ainv = lambda v: (d32 * v.astype(np.float32)).astype(np.float64)
    rb, cb = np.repeat(np.arange(B.nrows), np.diff(B.rowptr)), B.colidx.astype(np.int64)
    for fact in G.FACTS:
        y0, y1, b0, b1, mv = G.ref_pc_apply_inner(fact, B, sh, x, ainv)
        for rev in (False, True):
            x0, x1 = x[:n], x[n:]
            if fact == G.UPPER:
                z1 = -x1 / sh
                z0 = ainv(x0 - G._sum_at(cb, B.val * z1[rb], n, np.float64, rev))
            else:
                z0 = ainv(x0)
                z1 = x1 / sh if fact == G.DIAG else -(x1 - G._sum_at(rb, B.val * z0[cb], B.nrows, np.float64, rev)) / sh
                if fact == G.FULL:
                    z0 = z0 - ainv(G._sum_at(cb, B.val * z1[rb], n, np.float64, rev))
            w0, w1 = G.worst(np.abs(z0 - y0), b0), G.worst(np.abs(z1 - y1), b1)
            print(f"fact {fact}, reversed {rev}: movement {mv:.3g}, y0 {w0:.3g}, y1 {w1:.3g} of the bar")
            assert w0 <= 1 and w1 <= 1
            if fact in (G.DIAG, G.LOWER):
                assert w0 == 0                              # the same input: the same bytes


def test_a_dropped_entry_breaks_the_bars(cases):
    """what the bars are for: the first entry of a wide row's window left out, a wide row's result written to the wrong
    row, S^ of the last wide row left at the stream's zero -- each misses its bar by orders of magnitude"""
    A, B = cases["long"]
    n = A.nrows
    x = _x(A, B, 11)
    c = G.classes(B)
    _, y1, _, b1 = G.ref_mult(A, B, x)
    r = c["layout"]["wide_rows"][0]
    val = B.val.copy()
    val[B.rowptr[r]] = 0.0
    y = G.f64_mult(A, G.S.CSR(B.rowptr, B.colidx, val, n), x)[n:]
    assert np.abs(y[r] - y1[r]) > 1000 * b1[r] and G.worst(np.abs(np.delete(y, r) - np.delete(y1, r)), np.delete(b1, r)) <= 1
    good = G.f64_mult(A, B, x)[n:]
    swapped = good.copy()
    swapped[:8] = good[c["layout"]["wide_rows"]]
    assert G.worst(np.abs(swapped - y1), b1) > 1000
    d = G.jacobi_d(A)
    sh, bs = G.ref_shat(B, d)
    s = G.f64_shat(B, d)
    s[c["layout"]["wide_rows"][-1]] = 0.0
    assert G.worst(np.abs(s - sh), bs) > 1000


# --------------------------------------------------------------------------- the textbook model's two orders
def test_textbook_fgmres_takes_a_reversed_order(cases):
    """fgmres_textbook(reverse=True) sums its dot products over the reversed vectors: the same iteration, another order
    of the same numbers -- the histories differ, and by little"""
    A, B = cases["long"]
    n = A.nrows
    d = G.jacobi_d(A)
    sh = G.f64_shat(B, d)
    rhs = G.vec(n + B.nrows, 21)
    K = lambda v: G.f64_mult(A, B, v)
    M = lambda v: G.f64_pc_apply(G.FULL, B, d, sh, v)
    _, a = fgmres_textbook(K, M, rhs, restart=30, max_it=8, rtol=0.0)
    _, b = fgmres_textbook(K, M, rhs, restart=30, max_it=8, rtol=0.0, reverse=True)
    assert a["its"] == b["its"] == 8 and len(a["history"]) == 9
    move = np.abs(a["history"] - b["history"]) / a["history"]
    assert 0 < move.max() < 1e-10
