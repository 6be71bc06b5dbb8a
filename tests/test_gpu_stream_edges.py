"""The CSR stream kernel, the 2x2- and the 3x3-blocked kernels and the FP32 sweeps on the same layouts, on rows that sit at
the switch between their two paths (a tile of rows summed in CSR order / one long row on its own): test_stream_edges_cpu.py
holds the matrices, the rules that say which row takes which path, the float32 restatement of the sweeps over logical
ranks and the bounds.  Tiled rows are compared bit for bit, long rows to the worst-case bounds (no margin), with the
riders of the row tail (B^T lambda in the tail, B^T lambda accumulated onto, off-rank columns) on both kinds of row.
Every test prints its largest error / bound before it asserts (-s shows them); on one MI355X: 1.2e-3 on the products' long
rows, 8e-5 on the sweeps' long rows, 0.66 on short rows (where the bound is the rounding of the product itself).
Needs a real MI355X: run with -m gpu."""
import threading

import numpy as np
import pytest

from conftest import relerr
from test_gpu_product_tail import _env
from test_stream_edges_cpu import (CUTS, OMEGAS, SWEEPS, constraints, diag_block, edge_bcsr, edge_csr, general_spd, long_rows,
                                   product_check, sweep_step_check, sweeps_ref, tail_emulated, touched_rows, transposed, vec)

pytestmark = pytest.mark.gpu

FORCE_CSR = {"SPK_SPMV_FORMAT": "csr"}
# case -> (matrix, environment the operator is set under, format it must report)
CASES = {"csr": ("edge_csr", {}, "csr"),
         "b2": ("edge_bcsr2", {}, "bcsr2x2"), "b2_as_csr": ("edge_bcsr2", FORCE_CSR, "csr"),
         "b3": ("edge_bcsr3", {}, "bcsr3x3"), "b3_as_csr": ("edge_bcsr3", FORCE_CSR, "csr")}
NATURAL = {"edge_csr": "csr", "edge_bcsr2": "bcsr2x2", "edge_bcsr3": "bcsr3x3", "general_spd": "csr"}
MS = (4, 9)          # rows of the constraint block: in the product's tail / a general block the A product accumulates onto
RANK_OMEGA = 0.8


@pytest.fixture(scope="module")
def mats():
    return {"edge_csr": edge_csr()[0], "edge_bcsr2": edge_bcsr(2)[0], "edge_bcsr3": edge_bcsr(3)[0],
            "general_spd": general_spd(1001, 1001)[0]}


@pytest.fixture(scope="module")
def xs(mats):
    return {name: vec(A.nrows + max(MS), 41) for name, A in mats.items()}


@pytest.fixture(scope="module")
def blocks(mats):
    """(matrix, m) -> B; the same block under both layouts of a matrix (rows long in either are `long` to it)"""
    return {(name, m): constraints(mats[name].nrows, m, touched_rows(mats[name], NATURAL[name]))
            for name in ("edge_csr", "edge_bcsr2", "edge_bcsr3") for m in MS}


@pytest.fixture(scope="module")
def one_rank(spk, mats, xs, blocks):
    """per case: the format, A x, K [x; lambda] with the m = 4 and the m = 9 block, and the sweeps' results z[omega, k]"""
    out = {}
    for case, (name, env, _) in CASES.items():
        A, n = mats[name], mats[name].nrows
        r = {}
        with _env(env):
            with spk.Context(0) as c:
                c.set_block(spk.BLOCK_A00, A)
                r["format"] = c.spmv_info()["format"]
                r["y"] = c.mult(xs[name][:n])
                for om in OMEGAS:
                    for k in SWEEPS:
                        c.pc_setup(spk.PC_JACOBI, 0, inner_sweeps=k, inner_omega=om)
                        r["z", om, k] = c.pc_apply(xs[name][:n])
            for m in MS:
                with spk.Context(0) as c:
                    c.set_block(spk.BLOCK_A00, A)
                    c.set_block(spk.BLOCK_A10, blocks[name, m])
                    r["K", m] = c.mult(xs[name][:n + m])
        out[case] = r
    return out


def run_ranks(spk, A, cuts, work):
    """one logical rank per thread on the slabs [cuts[i], cuts[i + 1]): [work(context, lo, hi)] by rank"""
    P = len(cuts) - 1
    grp = spk.LocalGroup(P)
    out, errs = [None] * P, []

    def body(r):
        try:
            lo, hi = cuts[r], cuts[r + 1]
            with spk.Context(0) as c:
                c.comm_init_local(grp, r)
                c.set_block(spk.BLOCK_A00, A.slab(lo, hi))
                out[r] = work(c, lo, hi)
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=body, args=(r,)) for r in range(P)]
    [t.start() for t in th]
    [t.join(timeout=120) for t in th]
    alive = [t.is_alive() for t in th]
    grp.close()
    assert not errs and not any(alive), errs
    return out


def _report(what, err, bound, sel=None):
    ratio = (err / np.where(bound > 0, bound, 1.0))[sel if sel is not None else slice(None)]
    print(f"{what}: largest error / bound {ratio.max() if ratio.size else 0.0:.3g} over {ratio.size} rows")


# --------------------------------------------------------------------------- products
def test_products_at_the_switch(oracle, mats, xs, one_rank):
    """A x: the bits of the oracle's CSR loop on every row the layout's rule calls tiled, the any-order bound on the others;
    a row tiled under both layouts of a matrix holds the same bits in both"""
    for case, (name, _, fmt) in CASES.items():
        A, r = mats[name], one_rank[case]
        assert r["format"] == fmt, case
        x = xs[name][:A.nrows]
        lg = long_rows(A, fmt)
        assert lg.sum() >= (7 if case == "csr" else 0 if fmt == "csr" else 5 * int(fmt[-1]))
        y_ref = oracle.spmv(A, x)
        err, bound = product_check(A, r["y"], x, 0, A.nrows)
        _report(f"A x, {case}, long rows", err, bound, lg)
        assert np.array_equal(r["y"][~lg], y_ref[~lg]), case
        assert (err <= bound).all(), case
    for a, b in (("b2", "b2_as_csr"), ("b3", "b3_as_csr")):
        both = ~long_rows(mats[CASES[a][0]], CASES[a][2]) & ~long_rows(mats[CASES[b][0]], CASES[b][2])
        assert np.array_equal(one_rank[a]["y"][both], one_rank[b]["y"][both]) and both.sum() > 0.9 * len(both)


@pytest.mark.parametrize("m", MS)
def test_products_with_riders(oracle, mats, xs, blocks, one_rank, m):
    """K [x; lambda]: the rows of A with their B^T lambda (m = 4: fused multiply-adds in the row tail, behind the tiled and
    behind the long-row sums; m = 9: summed by the stream kernel first, the A product accumulates onto it) and the rows
    of B, every one to the product bound; tiled rows also against their arithmetic restated, bit for bit"""
    for case, (name, _, fmt) in CASES.items():
        A, B, n = mats[name], blocks[name, m], mats[name].nrows
        x, lam, K = xs[name][:n], xs[name][n:n + m], one_rank[case]["K", m]
        Bt = transposed(B)
        lg = long_rows(A, fmt)
        assert (np.diff(Bt[0])[lg] > 0).sum() >= (2 if lg.any() else 0) and (np.diff(Bt[0])[~lg] > 0).sum() >= 20
        err, bound = product_check(A, K[:n], x, 0, n, Bt, lam)
        _report(f"K x, m = {m}, {case}, rows of A", err, bound)
        assert (err <= bound).all(), (case, np.flatnonzero(err > bound))
        errb, boundb = product_check(B, K[n:], x, 0, n)
        _report(f"K x, m = {m}, {case}, rows of B", errb, boundb)
        assert (errb <= boundb).all(), case
        emu = tail_emulated(oracle, A, x, 0, n, Bt, lam, acc=m > 8)
        assert np.array_equal(K[:n][~lg], emu[~lg]), case
    for a, b in (("b2", "b2_as_csr"), ("b3", "b3_as_csr")):
        both = ~long_rows(mats[CASES[a][0]], CASES[a][2]) & ~long_rows(mats[CASES[b][0]], CASES[b][2])
        assert np.array_equal(one_rank[a]["K", m][:len(both)][both], one_rank[b]["K", m][:len(both)][both])


@pytest.mark.parametrize("name", ["edge_csr", "edge_bcsr2", "edge_bcsr3"])
def test_products_on_two_ranks(spk, oracle, mats, xs, name):
    """two logical ranks, cut at an odd row (CSR) or a block boundary: a row long in its rank's diagonal block has off-rank
    columns, added in the tail behind the tree sum; every row to the product bound, tiled rows without off-rank columns
    with the oracle's bits, tiled rows with them as restated"""
    A, cuts = mats[name], CUTS[name][0]
    x = xs[name][:A.nrows]
    runs = run_ranks(spk, A, cuts, lambda c, lo, hi: (c.spmv_info()["format"], c.mult(x[lo:hi])))
    y_ref = oracle.spmv(A, x)
    met = 0
    for (fmt, y), lo, hi in zip(runs, cuts[:-1], cuts[1:]):
        assert fmt == NATURAL[name]
        Sl = A.slab(lo, hi)
        D = diag_block(A, lo, hi)
        lg = long_rows(D, fmt)
        off = np.diff(Sl.rowptr) > np.diff(D.rowptr)
        met += int((lg & off).sum())
        err, bound = product_check(Sl, y, x, lo, hi)
        _report(f"A x on ranks, {name}, rows [{lo}, {hi})", err, bound)
        assert (err <= bound).all(), (lo, hi, np.flatnonzero(err > bound))
        assert np.array_equal(y[~lg & ~off], y_ref[lo:hi][~lg & ~off]) and (~lg & off).sum() >= 5
        assert np.array_equal(y[~lg], tail_emulated(oracle, Sl, x, lo, hi)[~lg])
    assert met >= 1


# --------------------------------------------------------------------------- FP32 sweeps, one rank
@pytest.mark.parametrize("case", list(CASES))
def test_sweeps_at_the_switch(oracle, mats, xs, one_rank, case):
    """1, 2, 3 and 4 sweeps (one: no sweep kernel, the first buffer; an even count ends in the other buffer), omega 0.8 and
    1: the blocked layouts equal the oracle's float loop on every row (their long block rows are summed in CSR order, 513
    and 257 blocks included); the CSR layout on every tiled row, its long rows (tree order) within the one-step bound --
    from y_1, known bit for bit, for two sweeps; from the device's own result of one sweep fewer for three and four"""
    name, _, fmt = CASES[case]
    A, r = mats[name], one_rank[case]
    x = xs[name][:A.nrows]
    assert r["format"] == fmt
    lg = long_rows(A, fmt) if fmt == "csr" else np.zeros(A.nrows, bool)
    for om in OMEGAS:
        for k in SWEEPS:
            z, zo = r["z", om, k], oracle.pc_apply_inner(A, None, oracle.PC_JACOBI, 0, k, om, x)
            assert np.array_equal(z[~lg], zo[~lg]), (case, om, k, int((z != zo)[~lg].sum()))
            if k == 1:
                assert np.array_equal(z, zo)
            elif lg.any():
                err, bound = sweep_step_check(A, r["z", om, k - 1], x, om, z)
                _report(f"sweeps, {case}, omega {om}, {k} sweeps, long rows", err, bound, lg)
                assert (err[lg] <= bound[lg]).all(), (case, om, k, err[lg] / bound[lg])
    assert lg.sum() == (7 if case == "csr" else 0)


@pytest.mark.parametrize("fact", [0, 3])
def test_schur_with_sweeps_on_long_rows(spk, oracle, mats, xs, blocks, fact):
    """the sweeps standing for diag(A)^-1 inside the Schur fieldsplit (test_fp32_inner_solve's bars) on edge_csr with the
    m = 4 block, whose rows touch long rows"""
    A, B, n = mats["edge_csr"], blocks["edge_csr", 4], mats["edge_csr"].nrows
    x = xs["edge_csr"][:n + 4]
    with spk.Context(0) as c:
        c.set_block(spk.BLOCK_A00, A)
        c.set_block(spk.BLOCK_A10, B)
        assert c.spmv_info()["format"] == "csr"
        c.pc_setup(spk.PC_SCHUR, fact, inner_sweeps=3, inner_omega=0.8)
        z = c.pc_apply(x)
    zo = oracle.pc_apply_inner(A, B, oracle.PC_SCHUR, fact, 3, 0.8, x)
    assert relerr(z, zo) < 1e-6
    if fact == 0:
        lg = long_rows(A, "csr")
        assert np.array_equal(z[:n][~lg], zo[:n][~lg])


# --------------------------------------------------------------------------- FP32 sweeps on logical ranks
@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("name", ["general_spd", "edge_bcsr2", "edge_bcsr3", "edge_csr"])
def test_sweeps_on_ranks(spk, mats, xs, name, P):
    """sweep_offdiag_f32 behind the CSR and the blocked sweeps, odd shares on the general operator: every rank's result
    after 1-4 sweeps equals sweeps_ref with the same cuts, bit for bit, on every row its layout sums in CSR order (the
    rule on the rank's diagonal block; the blocked layouts: every row); a row the CSR layout calls long within the
    one-step bound from the ranks' own result of one sweep fewer"""
    A, cuts = mats[name], CUTS[name][P - 2]
    n = A.nrows
    x = xs[name][:n]

    def work(c, lo, hi):
        z = {}
        for k in SWEEPS:
            c.pc_setup(spk.PC_JACOBI, 0, inner_sweeps=k, inner_omega=RANK_OMEGA)
            z[k] = c.pc_apply(x[lo:hi])
        return c.spmv_info()["format"], c.sizes()["n_ghost"], z
    runs = run_ranks(spk, A, cuts, work)
    assert len(cuts) == P + 1 and [f for f, _, _ in runs] == [NATURAL[name]] * P and all(g > 0 for _, g, _ in runs)
    lg = np.zeros(n, bool)
    if NATURAL[name] == "csr":
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            lg[lo:hi] = long_rows(diag_block(A, lo, hi), "csr")
    z = {k: np.concatenate([zr[k] for _, _, zr in runs]) for k in SWEEPS}
    for k in SWEEPS:
        ref = sweeps_ref(A, cuts, k, RANK_OMEGA, x)
        assert np.array_equal(z[k][~lg], ref[~lg]), (name, P, k, np.flatnonzero((z[k] != ref) & ~lg)[:10])
        if k == 1:
            assert np.array_equal(z[k], ref)
        elif lg.any():
            err, bound = sweep_step_check(A, z[k - 1], x, RANK_OMEGA, z[k])
            _report(f"sweeps on {P} ranks, {name}, {k} sweeps, long rows", err, bound, lg)
            assert (err[lg] <= bound[lg]).all(), (name, P, k, err[lg] / bound[lg])
    assert lg.sum() == (1 if name == "edge_csr" else 0)
