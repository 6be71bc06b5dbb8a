"""The general constraint block (more than 8 rows) on the device, at the edges of its three paths -- the column-window
kernel for at most eight rows of more than 8192 entries, the stream kernel's tiles, the stream kernel's one row per
workgroup -- and of what is built on them: B^T as a stream operand, S^ row by row, bt_update with the scratch vector in
its four modes, the B^T lambda that FGMRES's step path takes over from PCApply, a block replaced on a live context, and
column slices over logical ranks on which the same row is wide, short or empty.  _general_b_cases.py holds the inputs,
the rules restated, the long-double reference and the derived component-wise bars; test_general_b_edges_cpu.py shows
without a GPU that the cases hold their classes and that plain float64 stays inside the bars.  Here the layout the
context reports (Context.constraint_layout) must equal the restatement, so every row provably took the path it is named
for, and every component of every result is held to its bar.  D and S^ in the PCApply references are the context's own
jacobi_diag() and schur_diag(): only the chain under test contributes rounding.  Every test prints its largest
error / bar before it asserts (-s shows them).  Needs a real MI355X: run with -m gpu."""
import threading

import numpy as np
import pytest
import scipy.sparse as sp

import _general_b_cases as G
from _cb_fgmres import fgmres_textbook

pytestmark = pytest.mark.gpu

ONE_RANK = {"small": G.small_case, "long": G.long_case, "long_first_wide": lambda: G.long_case(True), "tall": G.tall_case}
INNER = {"sweeps": dict(inner_sweeps=3), "gamg": dict(amg=True)}
ITS = 25


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, build in ONE_RANK.items():
        A, B = build()
        out[name] = dict(A=A, B=B, n=A.nrows, m=B.nrows, x=G.vec(A.nrows + B.nrows, 11), rhs=G.vec(A.nrows + B.nrows, 21),
                         cls=G.classes(B))
    return out


def _per_key(run):
    """a module's device work key by key, each done when a test first asks for it and kept: a set-up that fails is an
    error of the tests of its own key only"""
    kept = {}

    def get(key):
        if key not in kept:
            kept[key] = run(key)
        return kept[key]
    return get


@pytest.fixture(scope="module")
def one_rank(spk, cases):
    """one_rank(case): one context -- the layout, K x twice, and per factorisation D, S^ and PCApply"""
    def run(name):
        cs, r = cases[name], {}
        with spk.Context(0) as c:
            c.set_block(spk.BLOCK_A00, cs["A"])
            c.set_block(spk.BLOCK_A10, cs["B"])
            r["layout"] = c.constraint_layout()
            r["y"], r["y_again"] = c.mult(cs["x"]), c.mult(cs["x"])
            for fact in G.FACTS:
                c.pc_setup(spk.PC_SCHUR, fact)
                r["d", fact], r["sh", fact] = c.jacobi_diag(), c.schur_diag()
                r["z", fact], r["z_again", fact] = c.pc_apply(cs["x"]), c.pc_apply(cs["x"])
        return r
    return _per_key(run)


def _hold(what, got, ref, bar):
    w = G.worst(np.abs(np.asarray(got, G.LD) - ref), bar)
    print(f"{what}: largest error / bar {w:.3g}")
    assert w <= 1, what
    return w


# --------------------------------------------------------------------------- layout
@pytest.mark.parametrize("name", list(ONE_RANK))
def test_layout_is_the_restatement(cases, one_rank, name):
    """every row took the path the restatement names; B^T is tiled in every case (bt_update's own one-thread-per-row
    kernel is not reachable with a general block on a rank that owns rows)"""
    assert one_rank(name)["layout"] == cases[name]["cls"]["layout"]
    assert one_rank(name)["layout"]["bt_tiles"] > 0 and one_rank(name)["layout"]["general"]


# --------------------------------------------------------------------------- K x and S^
@pytest.mark.parametrize("name", list(ONE_RANK))
def test_products_and_shat(cases, one_rank, name):
    cs, r = cases[name], one_rank(name)
    n = cs["n"]
    y0, y1, b0, b1 = G.ref_mult(cs["A"], cs["B"], cs["x"])
    _hold(f"K x, {name}, rows of A", r["y"][:n], y0, b0)
    _hold(f"K x, {name}, rows of B", r["y"][n:], y1, b1)
    assert r["y"].tobytes() == r["y_again"].tobytes()
    sh, bs = G.ref_shat(cs["B"], r["d", G.FULL])
    for fact in G.FACTS:
        assert r["sh", fact].tobytes() == r["sh", G.FULL].tobytes() and r["d", fact].tobytes() == r["d", G.FULL].tobytes()
    assert np.array_equal(r["d", G.FULL], G.jacobi_d(cs["A"]))
    _hold(f"S^, {name}", r["sh", G.FULL], sh, bs)
    assert (r["sh", G.FULL] > 0).all()


# --------------------------------------------------------------------------- PCApply, no inner solve
@pytest.mark.parametrize("fact", G.FACTS)
@pytest.mark.parametrize("name", list(ONE_RANK))
def test_pc_apply(cases, one_rank, name, fact):
    """bt_update modes 0 (UPPER) and 1 (FULL) through the scratch vector, the scaled apply_B (LOWER, FULL)"""
    cs, r = cases[name], one_rank(name)
    n = cs["n"]
    y0, y1, b0, b1 = G.ref_pc_apply(fact, cs["B"], r["d", fact], r["sh", fact], cs["x"])
    _hold(f"PCApply, {name}, fact {fact}, y0", r["z", fact][:n], y0, b0)
    _hold(f"PCApply, {name}, fact {fact}, y1", r["z", fact][n:], y1, b1)
    assert r["z", fact].tobytes() == r["z_again", fact].tobytes()


# --------------------------------------------------------------------------- PCApply with an inner solve
@pytest.fixture(scope="module")
def inner_runs(spk, cases):
    """inner_runs(inner): `long` under FP32 sweeps or under a V-cycle -- PCApply per factorisation, then the reference
    chain with the same context's A^ ^-1 (PC_JACOBI, the same inner options, applied to [v; 0])"""
    cs = cases["long"]
    n, m = cs["n"], cs["m"]

    def run(inner):
        out = {}
        with spk.Context(0) as c:
            c.set_block(spk.BLOCK_A00, cs["A"])
            c.set_block(spk.BLOCK_A10, cs["B"])
            for fact in G.FACTS:
                c.pc_setup(spk.PC_SCHUR, fact, **INNER[inner])
                out[fact, "z"], out[fact, "sh"] = c.pc_apply(cs["x"]), c.schur_diag()
            c.pc_setup(spk.PC_JACOBI, 0, **INNER[inner])
            ainv = lambda v: c.pc_apply(np.concatenate([np.asarray(v, np.float64), np.zeros(m)]))[:n]
            for fact in G.FACTS:
                out[fact, "ref"] = G.ref_pc_apply_inner(fact, cs["B"], out[fact, "sh"], cs["x"], ainv)
        return out
    return _per_key(run)


@pytest.mark.parametrize("fact", G.FACTS)
@pytest.mark.parametrize("inner", list(INNER))
def test_pc_apply_with_an_inner_solve(cases, inner_runs, inner, fact):
    """bt_update modes 2 (UPPER: x0 - B^T y1) and 3 (FULL: B^T y1) through the scratch vector, the unscaled apply_B
    (LOWER, FULL)"""
    n = cases["long"]["n"]
    y0, y1, b0, b1, mv = inner_runs(inner)[fact, "ref"]
    z = inner_runs(inner)[fact, "z"]
    print(f"{inner}, fact {fact}: inner-solve movement {mv:.3g}, bar on y0 {float(np.max(b0)):.3g}, |y0| up to {float(np.abs(y0).max()):.3g}")
    _hold(f"PCApply, long, {inner}, fact {fact}, y1", z[n:], y1, b1)
    _hold(f"PCApply, long, {inner}, fact {fact}, y0", z[:n], y0, b0)


# --------------------------------------------------------------------------- solves on `long`
def _true_rnorm(cs, rhs, x):
    """(the long-double ||b - K x||, the floor below which no float64 residual is known: the norm of the product bars at
    this x, gamma(entries of the row) sum|terms| per component -- what one float64 evaluation of K x may be off by)"""
    y0, y1, b0, b1 = G.ref_mult(cs["A"], cs["B"], x)
    r = np.asarray(rhs, G.LD) - np.concatenate([y0, y1])
    floor = np.concatenate([b0, b1])
    return float(np.sqrt(np.sum(r * r))), float(np.sqrt(np.sum(floor * floor)))


def _agrees(true, reported, floor):
    return abs(true - reported) <= 1e-6 * reported if reported >= floor else true <= floor


# {UPPER, FULL} x {none, sweeps, gamg} at 25 iterations; LOWER and DIAG under the sweeps (where PCApply leaves something
# else than B^T y1 in the scratch vector); the V-cycle also at 10 iterations, where its residual is still far above the
# rounding floor: key -> (inner options, iterations, factorisations)
SOLVES = {"none": ({}, ITS, (G.UPPER, G.FULL)), "sweeps": (INNER["sweeps"], ITS, (G.UPPER, G.FULL, G.LOWER, G.DIAG)),
          "gamg": (INNER["gamg"], ITS, (G.UPPER, G.FULL)), "gamg10": (INNER["gamg"], 10, (G.UPPER, G.FULL))}


@pytest.fixture(scope="module")
def solves(spk, cases):
    """solves(key): the solves of SOLVES[key] on `long`, one after the other on one context"""
    cs = cases["long"]

    def run(key):
        opts, its, facts = SOLVES[key]
        out = {}
        with spk.Context(0) as c:
            c.set_block(spk.BLOCK_A00, cs["A"])
            c.set_block(spk.BLOCK_A10, cs["B"])
            for fact in facts:
                c.pc_setup(spk.PC_SCHUR, fact, **opts)
                out[fact] = c.fgmres(cs["rhs"], rtol=0.0, abstol=0.0, max_it=its)
                out["d", fact], out["sh", fact] = c.jacobi_diag(), c.schur_diag()
        return out
    return _per_key(run)


@pytest.mark.parametrize("inner,fact", [(key, f) for key, (_, _, facts) in SOLVES.items() for f in facts])
def test_solve_residual_is_the_true_one(cases, solves, inner, fact):
    """the long-double ||b - K x|| of the returned x against the reported norm, to 1e-6 of it: a wrong B^T lambda anywhere
    in the step path (taken over from PCApply's scratch vector under UPPER and FULL, recomputed under LOWER and DIAG)
    breaks the Arnoldi relation and with it this agreement.  Under the V-cycle 25 iterations take the residual from 8.3e2
    to the rounding floor (reported 2.3e-12 / 1.9e-13, true 5.0e-12 / 3.9e-12 on one MI355X), where the recurrence goes
    on falling and b - K x cannot.  So the 1e-6 holds wherever the reported norm is above the floor of _true_rnorm
    (4.6e-7 at these x: a figure of the inputs and u alone), and a reported norm below it asks that the true one is below
    it too.  Every solve but the V-cycle's at 25 iterations must be above the floor, which is asserted; the V-cycle is
    held to the 1e-6 after 10 iterations (`gamg10`), both factorisations."""
    x, info = solves(inner)[fact]
    its = SOLVES[inner][1]
    assert info["its"] == its and len(info["history"]) == its + 1 and np.isfinite(info["history"]).all()
    true, floor = _true_rnorm(cases["long"], cases["long"]["rhs"], x)
    print(f"{inner}, fact {fact}: reported {info['rnorm']:.6e}, true {true:.6e}, floor {floor:.3e}, first {info['history'][0]:.3e}")
    assert _agrees(true, info["rnorm"], floor)
    assert inner == "gamg" or info["rnorm"] >= floor
    assert info["rnorm"] < info["history"][0]


@pytest.mark.parametrize("fact", [G.UPPER, G.FULL])
def test_solve_history_is_the_textbook_one(cases, solves, fact):
    """no inner solve: the history against a plain FP64 FGMRES on the numpy K and the numpy M (the context's D and S^); the
    bar is 1e-7 or 100 x what the model itself moves by when its dot products are summed in the reversed order"""
    cs = cases["long"]
    n, m = cs["n"], cs["m"]
    A = sp.csr_matrix((cs["A"].val, cs["A"].colidx, cs["A"].rowptr), shape=(n, n))
    B = sp.csr_matrix((cs["B"].val, cs["B"].colidx, cs["B"].rowptr), shape=(m, n))
    Bt = B.T.tocsr()
    d, sh = solves("none")["d", fact], solves("none")["sh", fact]
    K = lambda v: np.concatenate([A @ v[:n] + Bt @ v[n:], B @ v[:n]])

    def M(v):
        x0, x1 = v[:n], v[n:]
        if fact == G.UPPER:
            y1 = -x1 / sh
            return np.concatenate([(x0 - Bt @ y1) * d, y1])
        y1 = -(x1 - B @ (d * x0)) / sh
        return np.concatenate([x0 * d - (Bt @ y1) * d, y1])
    _, fwd = fgmres_textbook(K, M, cs["rhs"], restart=30, max_it=ITS, rtol=0.0)
    _, rev = fgmres_textbook(K, M, cs["rhs"], restart=30, max_it=ITS, rtol=0.0, reverse=True)
    own = float(np.max(np.abs(fwd["history"] - rev["history"]) / fwd["history"]))
    bar = max(1e-7, 100 * own)
    h = solves("none")[fact][1]["history"]
    off = float(np.max(np.abs(h - fwd["history"]) / fwd["history"]))
    print(f"fact {fact}: history off the textbook's by {off:.3g}, the model's own movement {own:.3g}, bar {bar:.3g}")
    assert len(h) == len(fwd["history"]) == ITS + 1 and off <= bar


@pytest.mark.parametrize("inner,fact", [("none", G.UPPER), ("none", G.FULL), ("sweeps", G.UPPER), ("sweeps", G.FULL),
                                        ("sweeps", G.LOWER), ("gamg", G.UPPER), ("gamg", G.FULL)])
def test_the_cached_bt_product_survives_what_lies_between_solves(spk, cases, solves, inner, fact):
    """bt_cached is a pointer rule: the same right-hand side twice on one context, a product in between, and again -- the
    same history and solution bytes every time, and those of the context that ran the other solves before"""
    cs = cases["long"]
    rhs = cs["rhs"]
    with spk.Context(0) as c:
        c.set_block(spk.BLOCK_A00, cs["A"])
        c.set_block(spk.BLOCK_A10, cs["B"])
        c.pc_setup(spk.PC_SCHUR, fact, **INNER.get(inner, {}))
        runs = [c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=ITS), c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=ITS)]
        y = c.mult(cs["x"])
        z = c.pc_apply(cs["x"])
        runs.append(c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=ITS))
        assert c.mult(cs["x"]).tobytes() == y.tobytes() and c.pc_apply(cs["x"]).tobytes() == z.tobytes()
    for x, info in runs + [solves(inner)[fact]]:
        assert info["history"].tobytes() == runs[0][1]["history"].tobytes() and x.tobytes() == runs[0][0].tobytes()


# --------------------------------------------------------------------------- a block replaced on a live context
def test_block_change_on_one_context(spk, cases):
    """long, then small's rows, then tall's rows (m = 2305: the vectors and the scratch vector grow), then the first eight
    rows of small (not a general block: every row through the window kernel, nothing tiled -- B^T's tile table of the
    block before must be gone), then long again on one context: the layout is the restatement's and every product equals
    a fresh context's bytes (b_release_general, the regrowth of the scratch vector)"""
    A, n = cases["long"]["A"], cases["long"]["n"]

    def over_n(B):
        return spk.CSR(B.rowptr, B.colidx, B.val, n)
    Bs = cases["small"]["B"]
    few = spk.CSR(Bs.rowptr[:9], Bs.colidx[:Bs.rowptr[8]], Bs.val[:Bs.rowptr[8]], n)
    seq = [("long", cases["long"]["B"]), ("small", over_n(Bs)), ("tall", over_n(cases["tall"]["B"])), ("few", few),
           ("long", cases["long"]["B"])]

    def products(c, B):
        x = G.vec(n + B.nrows, 31)
        c.set_block(spk.BLOCK_A10, B)
        lay = c.constraint_layout()
        y = c.mult(x)
        c.pc_setup(spk.PC_SCHUR, spk.SCHUR_FULL)
        z = c.pc_apply(x)
        c.pc_setup(spk.PC_SCHUR, spk.SCHUR_UPPER, inner_sweeps=3)
        return lay, y, z, c.pc_apply(x), c.schur_diag()
    fresh = {}
    for name, B in seq[:4]:
        with spk.Context(0) as c:
            c.set_block(spk.BLOCK_A00, A)
            fresh[name] = products(c, B)
        assert fresh[name][0] == G.classes(B)["layout"]
    assert fresh["few"][0] == dict(general=False, m_wide=8, wide_rows=list(range(8)), win=1024, nwin=10, bc_tiles=0, bt_tiles=0)
    with spk.Context(0) as c:
        c.set_block(spk.BLOCK_A00, A)
        for name, B in seq:
            got = products(c, B)
            assert got[0] == fresh[name][0], name
            for a, b in zip(got[1:], fresh[name][1:]):
                assert a.tobytes() == b.tobytes(), name


# --------------------------------------------------------------------------- column slices over logical ranks
@pytest.fixture(scope="module", params=[2, 3])
def rank_runs(spk, request):
    """one logical rank per thread: layout, K x twice, D, S^, PCApply under FULL and UPPER; P = 2: a solve under FULL"""
    P = request.param
    A, B, cuts = G.rank_case(P)
    n, m = A.nrows, B.nrows
    x, rhs = G.vec(n + m, 12), G.vec(n + m, 22)
    grp = spk.LocalGroup(P)
    out, errs = [None] * P, []

    def body(r):
        try:
            lo, hi = cuts[r], cuts[r + 1]
            res = {}
            with spk.Context(0) as c:
                c.comm_init_local(grp, r)
                c.set_block(spk.BLOCK_A00, A.slab(lo, hi))
                c.set_block(spk.BLOCK_A10, B.col_slab(lo, hi))
                res["layout"] = c.constraint_layout()
                xl = np.concatenate([x[lo:hi], x[n:]])
                res["y"], res["y_again"] = c.mult(xl), c.mult(xl)
                for fact in (G.FULL, G.UPPER):
                    c.pc_setup(spk.PC_SCHUR, fact)
                    res["d"], res["sh"] = c.jacobi_diag(), c.schur_diag()
                    res["z", fact] = c.pc_apply(xl)
                if P == 2:
                    c.pc_setup(spk.PC_SCHUR, G.FULL)
                    res["solve"] = c.fgmres(np.concatenate([rhs[lo:hi], rhs[n:]]), rtol=0.0, abstol=0.0, max_it=ITS)
            out[r] = res
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=body, args=(r,)) for r in range(P)]
    [t.start() for t in th]
    [t.join(timeout=120) for t in th]
    alive = [t.is_alive() for t in th]
    grp.close()
    assert not errs and not any(alive), errs
    return dict(P=P, A=A, B=B, cuts=cuts, x=x, rhs=rhs, runs=out)


def _gathered(rr, key):
    """the ranks' shares of a result put together; the multiplier part is replicated, byte for byte"""
    n = rr["A"].nrows
    top = np.concatenate([run[key][:hi - lo] for run, lo, hi in zip(rr["runs"], rr["cuts"][:-1], rr["cuts"][1:])])
    for run, lo, hi in zip(rr["runs"], rr["cuts"][:-1], rr["cuts"][1:]):
        assert run[key][hi - lo:].tobytes() == rr["runs"][0][key][rr["cuts"][1]:].tobytes()
    assert len(top) == n
    return top, rr["runs"][0][key][rr["cuts"][1]:]


def test_ranks_layout_is_the_restatement(rank_runs):
    """the same row wide on one rank, short on the next, empty on a third: wide_rows sees the slab's row pointers"""
    rr = rank_runs
    for r, (lo, hi) in enumerate(zip(rr["cuts"][:-1], rr["cuts"][1:])):
        assert rr["runs"][r]["layout"] == G.classes(rr["B"], lo, hi)["layout"], r


def test_ranks_products_and_shat(rank_runs):
    rr = rank_runs
    P, A, B = rr["P"], rr["A"], rr["B"]
    y0, y1, b0, b1 = G.ref_mult(A, B, rr["x"], P)
    top, lam = _gathered(rr, "y")
    _hold(f"K x on {P} ranks, rows of A", top, y0, b0)
    _hold(f"K x on {P} ranks, rows of B", lam, y1, b1)
    for run in rr["runs"]:
        assert run["y"].tobytes() == run["y_again"].tobytes() and run["sh"].tobytes() == rr["runs"][0]["sh"].tobytes()
    d = np.concatenate([run["d"] for run in rr["runs"]])
    assert np.array_equal(d, G.jacobi_d(A))
    sh, bs = G.ref_shat(B, d, P)
    _hold(f"S^ on {P} ranks", rr["runs"][0]["sh"], sh, bs)


@pytest.mark.parametrize("fact", [G.FULL, G.UPPER])
def test_ranks_pc_apply(rank_runs, fact):
    rr = rank_runs
    d = np.concatenate([run["d"] for run in rr["runs"]])
    y0, y1, b0, b1 = G.ref_pc_apply(fact, rr["B"], d, rr["runs"][0]["sh"], rr["x"], rr["P"])
    top, lam = _gathered(rr, ("z", fact))
    _hold(f"PCApply on {rr['P']} ranks, fact {fact}, y0", top, y0, b0)
    _hold(f"PCApply on {rr['P']} ranks, fact {fact}, y1", lam, y1, b1)


@pytest.mark.parametrize("rank_runs", [2], indirect=True)
def test_ranks_solve(rank_runs):
    """P = 2 under FULL: both ranks return the same history, and the true residual of the gathered x is the reported one"""
    rr = rank_runs
    infos = [run["solve"][1] for run in rr["runs"]]
    assert infos[0]["history"].tobytes() == infos[1]["history"].tobytes() and infos[0]["its"] == ITS
    n = rr["A"].nrows
    x = np.concatenate([run["solve"][0][:hi - lo] for run, lo, hi in zip(rr["runs"], rr["cuts"][:-1], rr["cuts"][1:])]
                       + [rr["runs"][0]["solve"][0][rr["cuts"][1]:]])
    assert rr["runs"][0]["solve"][0][rr["cuts"][1]:].tobytes() == rr["runs"][1]["solve"][0][n - rr["cuts"][1]:].tobytes()
    true, floor = _true_rnorm(dict(A=rr["A"], B=rr["B"]), rr["rhs"], x)
    print(f"2 ranks, FULL: reported {infos[0]['rnorm']:.6e}, true {true:.6e}, floor {floor:.3e}")
    assert _agrees(true, infos[0]["rnorm"], floor) and infos[0]["rnorm"] >= floor
