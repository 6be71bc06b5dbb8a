"""The row-type kernels (spk_k_dict.hip, spk_k_dict3.hip, the resident cycle, gamg's fused fine-level step) on block rows
that are NOT the generator's 9 and 27 blocks: test_rowtype_shapes_cpu.py holds the matrices and shows, without a GPU, what
each is (longest block row, row types, classes, widths, field layout, side of the LDS budget).  Every accepted case asserts
through Context.dict_layout() the kernel and field layout it was written for, so a case that fell back to the blocked
kernels cannot pass for the wrong reason.  Products and FP32 sweeps are held bit for bit to the oracle's CSR-order loops --
the layout's own standard: same products, same order.  Needs a real MI355X: run with -m gpu."""
import threading
import time

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import relerr
from test_amg_cpu import hierarchy_mats, vcycle_ref
from test_gpu_product_tail import KERNEL_TOL, _env
from test_rowtype_shapes_cpu import CASES, analysed, build, sparse_rows, vec

pytestmark = pytest.mark.gpu

BCSR, CSR_FMT = {"SPK_SPMV_FORMAT": "bcsr"}, {"SPK_SPMV_FORMAT": "csr"}
PRODUCT_CASES = [n for n in CASES if not n.endswith(("_res", "_amg"))]
SWEEP_CASES = ["k1_256", "k10", "k11", "k32", "box25", "cls2", "str12", "t7", "t10", "t32", "pc3", "big2", "t27x"]
SWEEPS, OMEGA = (1, 2, 3, 4), 0.7
REFUSED = ["r33", "rlds", "rfit3"]
FORM5, FORM6 = 5, 6
MS = (4, 9)


def _blocked_name(bs):
    return "bcsr2x2" if bs == 2 else "bcsr3x3"


def _check_layout(name, c, env=None):
    """the layout the case was written for, as the context reports it"""
    want, a = CASES[name], analysed(name)
    lay, fmt = c.dict_layout(), c.spmv_info()["format"]
    if not want["ok"]:
        assert fmt == _blocked_name(want["bs"]) and lay["ok"] == 0 and not any(lay.values()), (name, fmt, lay)
        return lay
    assert lay["ok"] == 1 and fmt == ("dict2x2" if want["bs"] == 2 else "dict3x3"), (name, fmt, lay)
    kernel = 2 if env and env.get("SPK_DICT3_PIPELINE") == "1" else want["kernel"]
    got = (lay["bs"], lay["nbrows"], lay["kmax"], lay["ntype"], lay["nclass"], lay["lds_bytes"], lay["uniform"], lay["straddle"],
           lay["uniform3"], lay["product_kernel"])
    assert got == (want["bs"], a["nbrows"], want["kmax"], a["ntype"], a["nclass"], a["lds"], want["uniform"], want["straddle"],
                   want["uniform3"], kernel), (name, lay)
    return lay


def _set(spk, A, B=None):
    c = spk.Context(0)
    c.set_block(spk.BLOCK_A00, A)
    if B is not None:
        c.set_block(spk.BLOCK_A10, B)
    return c


# --------------------------------------------------------------------------- (1) y = A x
@pytest.mark.parametrize("name", PRODUCT_CASES)
def test_product_bits(spk, oracle, name):
    """y = A x in the row-type layout (or, for a refused case, the blocked one it fell back to) = the oracle's CSR loop =
    the blocked and the CSR kernels' results on the same matrix, bit for bit"""
    A = build(name)
    x = vec(A.ncols, 5)
    y_ref = oracle.spmv(A, x)
    t0 = time.perf_counter()
    with _env({}):
        with _set(spk, A) as c:
            lay = _check_layout(name, c)
            y = c.mult(x)
    print(f"{name}: layout {lay}, set-up + product {time.perf_counter() - t0:.2f} s")
    assert np.array_equal(y, y_ref)
    for env, fmt in ((BCSR, _blocked_name(CASES[name]["bs"])), (CSR_FMT, "csr")):
        with _env(env):
            with _set(spk, A) as c:
                assert c.spmv_info()["format"] == fmt and c.dict_layout()["ok"] == 0
                assert np.array_equal(c.mult(x), y_ref), (name, fmt)
    if name == "t27x":      # 27 arbitrary offsets through the pipelined 3x3 kernel
        env = {"SPK_DICT3_PIPELINE": "1"}
        with _env(env):
            with _set(spk, A) as c:
                _check_layout(name, c, env)
                assert np.array_equal(c.mult(x), y_ref)


def test_chunking_of_the_large_cases(spk):
    """big2 / big3: two chunks per workgroup of the plain kernels -- the multi-chunk loop and its prefetch of the next row type"""
    for name in ("big2", "big3"):
        with _env({}):
            with _set(spk, build(name)) as c:
                assert c.dict_layout()["chunks_per_wg"] == 2 and c.dict_layout()["product_kernel"] == 0
    with _env({}):
        with _set(spk, build("k11")) as c:
            assert c.dict_layout()["chunks_per_wg"] == 1


# --------------------------------------------------------------------------- (2) K [x; lambda]
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("name", ["k11", "box25", "t10", "str12"])
def test_nest_product_bits(spk, oracle, name, m):
    """A10 of 4 (in the product's tail) and of 9 arbitrary sparse rows (accumulated onto): the row-type and the blocked
    layout give the same bits on every row; against the oracle, the same bits on the rows no B^T entry touches and the
    existing kernel tolerance on all of them (the tail's fused multiply-adds are not the oracle's order)"""
    A = build(name)
    B = sparse_rows(A.nrows, m)
    x = vec(A.nrows + m, 6)
    out = {}
    for key, env in (("dict", {}), ("bcsr", BCSR)):
        with _env(env):
            with _set(spk, A, B) as c:
                if key == "dict":
                    _check_layout(name, c)
                else:
                    assert c.dict_layout()["ok"] == 0
                out[key] = c.mult(x)
    assert np.array_equal(out["dict"], out["bcsr"])
    y_ref = oracle.apply_K(A, B, x)
    free = np.ones(A.nrows + m, bool)
    free[B.colidx] = False
    free[A.nrows:] = False
    assert np.array_equal(out["dict"][free], y_ref[free])
    assert relerr(out["dict"], y_ref) < KERNEL_TOL


# --------------------------------------------------------------------------- (3) FP32 sweeps
@pytest.mark.parametrize("name", SWEEP_CASES)
def test_fp32_sweeps_bits(spk, oracle, name):
    A = build(name)
    x = vec(A.nrows, 8)
    envs = [{}] + ([{"SPK_DICT3_PIPELINE": "1"}] if name == "t27x" else [])
    ref = {s: oracle.pc_apply_inner(A, None, oracle.PC_JACOBI, 0, s, OMEGA, x) for s in SWEEPS}
    for env in envs:
        with _env(env):
            with _set(spk, A) as c:
                _check_layout(name, c, env)
                for s in SWEEPS:
                    c.pc_setup(spk.PC_JACOBI, 0, inner_sweeps=s, inner_omega=OMEGA)
                    assert np.array_equal(c.pc_apply(x), ref[s]), (name, s, env)


# --------------------------------------------------------------------------- (4) two logical ranks
@pytest.mark.parametrize("name,cut", [("k11", 1024), ("t10", 1100), ("k31", 350)])
def test_two_ranks(spk, oracle, name, cut):
    """Slabs cut at block row `cut` (k11: its +-1000 offsets cross the cut): each rank's slab has its own row-type layout
    over the blocks it keeps (a row at the cut loses its off-rank blocks to the halo part, so a slab's longest block row is
    counted here from its local columns), and the concatenated product holds the one-rank bits on every row without an
    off-rank column.  A row with off-rank columns adds them after its local ones -- another order, not other values: there
    the row-type and the blocked layout agree bit for bit, and both stay within the bar test_dictionary_row_slabs sets for
    such rows."""
    A, bs = build(name), CASES[name]["bs"]
    x = vec(A.ncols, 9)
    y_ref = oracle.spmv(A, x)
    cuts = [0, bs * cut, A.nrows]
    out, kmaxes = {}, {}
    for key, env in (("dict", {}), ("bcsr", BCSR)):
        grp = spk.LocalGroup(2)
        ys, lays, errs = [None, None], [None, None], []

        def work(r):
            try:
                with spk.Context(0) as c:
                    c.comm_init_local(grp, r)
                    c.set_block(spk.BLOCK_A00, A.slab(cuts[r], cuts[r + 1]))
                    lays[r] = (c.spmv_info()["format"], c.dict_layout())
                    ys[r] = c.mult(x[cuts[r]:cuts[r + 1]])
            except Exception as e:  # noqa: BLE001
                errs.append(e)
        with _env(env):
            th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
            [t.start() for t in th]
            [t.join(timeout=120) for t in th]
        alive = [t.is_alive() for t in th]
        grp.close()
        assert not errs and not any(alive), errs
        for fmt, lay in lays:
            if key == "dict":
                assert fmt == ("dict2x2" if bs == 2 else "dict3x3") and lay["ok"] == 1 and lay["bs"] == bs, (fmt, lay)
                assert lay["product_kernel"] == 0
            else:
                assert fmt == _blocked_name(bs) and lay["ok"] == 0
        out[key] = np.concatenate(ys)
        kmaxes[key] = [lay["kmax"] for _, lay in lays]
    rows = np.repeat(np.arange(A.nrows), np.diff(A.rowptr))
    local = np.bincount(rows[(rows < cuts[1]) == (A.colidx < cuts[1])], minlength=A.nrows) // bs
    assert kmaxes["dict"] == [local[:cuts[1]].max(), local[cuts[1]:].max()] and max(kmaxes["dict"]) >= 10, kmaxes
    off = np.zeros(A.nrows, bool)
    off[rows[(rows < cuts[1]) != (A.colidx < cuts[1])]] = True
    assert 0 < off.sum() < A.nrows
    assert np.array_equal(out["dict"], out["bcsr"])
    assert np.array_equal(out["dict"][~off], y_ref[~off])
    assert np.allclose(out["dict"][off], y_ref[off], rtol=1e-13, atol=1e-15)


# --------------------------------------------------------------------------- (5) form 5 solves
def _solve_setup(spk, oracle, c, B):
    c.pc_setup(spk.PC_SCHUR if B is not None else spk.PC_JACOBI, spk.SCHUR_FULL)
    return dict(B=B, pc_type=oracle.PC_SCHUR, schur_fact=oracle.SCHUR_FULL) if B is not None else dict(pc_type=oracle.PC_JACOBI)


@pytest.mark.parametrize("saddle", [False, True], ids=["jacobi", "schur_full"])
@pytest.mark.parametrize("name", ["box25", "k12s", "t10s"])
def test_form5_solve_same_iterates_in_both_layouts(spk, oracle, name, saddle):
    """FGMRES form 5, 45 iterations: every product of the iterations carries the rider, with B accumulates onto B^T lambda
    (the RIDE and BT variants of the plain kernel): histories and solutions bit for bit those of the blocked layout, counts
    within one of the oracle's"""
    A = build(name)
    B = sparse_rows(A.nrows, 4) if saddle else None
    rhs = vec(A.nrows + (4 if saddle else 0), 10)
    out = {}
    for key, env in (("dict", {}), ("bcsr", BCSR)):
        with _env(env):
            with _set(spk, A, B) as c:
                if key == "dict":
                    _check_layout(name, c)
                okw = _solve_setup(spk, oracle, c, B)
                out[key] = c.fgmres(rhs, rtol=1e-30, max_it=45, iteration_form=FORM5)
                assert c.iteration_form()[0] == FORM5
    (xd, idd), (xb, ib) = out["dict"], out["bcsr"]
    assert len(idd["history"]) > 1 and np.array_equal(idd["history"], ib["history"]) and np.array_equal(xd, xb)
    assert idd["its"] == ib["its"] and idd["reason"] == ib["reason"]
    _, io = oracle.fgmres(A, rhs, rtol=1e-30, max_it=45, **okw)
    assert abs(idd["its"] - io["its"]) <= 1, (idd["its"], io["its"])


# --------------------------------------------------------------------------- (6) the resident cycle
def _resident_check(spk, oracle, name, saddle):
    A = build(name)
    B = sparse_rows(A.nrows, 4) if saddle else None
    rhs = vec(A.nrows + (4 if saddle else 0), 12)
    with _env({}):
        with _set(spk, A, B) as c:
            _check_layout(name, c)
            okw = _solve_setup(spk, oracle, c, B)
            x6, i6 = c.fgmres(rhs, rtol=1e-9, max_it=600)
            assert c.iteration_form()[0] == FORM6
            x5, i5 = c.fgmres(rhs, rtol=1e-9, max_it=600, iteration_form=FORM5)
            assert c.iteration_form()[0] == FORM5
    assert i6["reason"] == i5["reason"] == 2 and abs(i6["its"] - i5["its"]) <= 1
    k = min(len(i6["history"]), len(i5["history"]), 31)
    print(f"{name} saddle={saddle}: its {i6['its']} / {i5['its']}, history "
          f"{np.max(np.abs(i6['history'][:k] - i5['history'][:k]) / i5['history'][:k]):.2e}, x {relerr(x6, x5):.2e}")
    assert np.allclose(i6["history"][:k], i5["history"][:k], rtol=1e-9)
    assert relerr(x6, x5) < 1e-7
    xo, io = oracle.fgmres(A, rhs, rtol=1e-9, max_it=600, **okw)
    assert i6["reason"] == io["reason"] and abs(i6["its"] - io["its"]) <= 1
    assert relerr(x6, xo) < 1e-7


@pytest.mark.parametrize("saddle", [False, True], ids=["jacobi", "schur_full"])
@pytest.mark.parametrize("name", ["box25", "k12s"])
def test_resident_cycle_on_long_rows(spk, oracle, name, saddle):
    """AUTO takes form 6 (kmax code words per thread copied into LDS through dict_word_ptr<2>, odd and even last plane);
    held against form 5 on the same context and the oracle at the bars of test_resident_cycle_equals_three_launch_form"""
    _resident_check(spk, oracle, name, saddle)


def test_resident_cycle_takes_512_threads_where_kmax_fits(spk, oracle):
    """65 792 block rows: 257 per compute unit, so 512 threads per workgroup and kmax * 4096 B of code words.
    resident_lds_bytes at T = 512 is 91 560 B + the tables + kmax * 4096: 12 blocks per row fit the 160 KB
    (test_rowtype_shapes_cpu.test_resident_budget_decides_by_kmax derives the limit, 16)"""
    _resident_check(spk, oracle, "k12s_res", False)


def test_resident_cycle_refused_by_its_lds_budget(spk):
    """the same number of block rows with 25 blocks per row: the code words alone (102 400 B) are over what is left of the
    160 KB, so AUTO reports form 5 and a request for form 6 falls back to it"""
    A = build("box25_res")
    rhs = vec(A.nrows, 12)
    with _env({}):
        with _set(spk, A) as c:
            _check_layout("box25_res", c)
            c.pc_setup(spk.PC_JACOBI, 0)
            _, ia = c.fgmres(rhs, rtol=1e-9, max_it=100)
            assert c.iteration_form()[0] == FORM5
            _, ir = c.fgmres(rhs, rtol=1e-9, max_it=100, iteration_form=FORM6)
            assert c.iteration_form()[0] == FORM5
    assert ia["reason"] == 2 and np.array_equal(ia["history"], ir["history"])


# --------------------------------------------------------------------------- (7) gamg's fused fine-level step
@pytest.mark.parametrize("name", ["box25", "k12s_amg"])
def test_gamg_fine_level_on_long_rows(spk, name):
    """One V-cycle with three Chebyshev steps per sweep (amg_cheb_dict2_kernel on block rows longer than its group of ten):
    the numpy V-cycle over the exported hierarchy to 1e-12, the same bits on a second application, on the row-type and on
    the blocked fine layout, and pipecg with it to the direct solve."""
    from scipy.sparse.linalg import spsolve
    A = build(name)
    x = vec(A.nrows, 13)
    out = {}
    for key, env in (("dict", {}), ("bcsr", BCSR)):
        with _env(env):
            with _set(spk, A) as c:
                if key == "dict":
                    _check_layout(name, c)
                c.pc_setup(spk.PC_JACOBI, amg=dict(smooth_its=3))
                info = c.amg_info()
                y = c.pc_apply(x)
                assert np.array_equal(y, c.pc_apply(x))
                mats = hierarchy_mats(c.amg_level, info)
                ref = vcycle_ref(*mats, info["lambda_max"], x, smooth_its=3)
                err = np.linalg.norm(y - ref) / np.linalg.norm(ref)
                print(f"{name} {key}: levels {info['levels']}, V-cycle against numpy {err:.2e}")
                assert info["levels"] >= 2 and err <= 1e-12
                xs, res = c.pipecg(x, rtol=1e-10, max_it=500)
                out[key] = (y, xs, res)
    K = sp.csr_matrix((A.val, A.colidx, A.rowptr), shape=(A.nrows, A.nrows)).tocsc()
    xd = spsolve(K, x)
    for key in out:
        assert out[key][2]["reason"] == 2 and relerr(out[key][1], xd) < 1e-8, (key, out[key][2]["reason"])


def _vcycle_both_layouts(spk, A, x):
    out = []
    for env in ({}, BCSR):
        with _env(env):
            with _set(spk, A) as c:
                c.pc_setup(spk.PC_JACOBI, amg=dict(smooth_its=3))
                out.append(c.pc_apply(x))
    d = out[0] - out[1]
    return out[0], out[1], f"{np.count_nonzero(d)} of {d.size} entries differ, relative {np.linalg.norm(d) / np.linalg.norm(out[1]):.2e}"


@pytest.mark.parametrize("name", ["box25", "k12s_amg"])
def test_gamg_fine_level_same_bits_as_blocked_layout(spk, name):
    """The V-cycle of the row-type fine layout against that of the blocked fine layout, bit for bit -- on the long rows and
    on the generator's own 64 x 64 operator.  amg_cheb_dict2_kernel rounds every product of its block-row sums on its own,
    as spmv_dict_kernel does, and ends in amg_cheb_vec's update.  (This test found it summing with fused multiply-adds:
    three quarters of a V-cycle's entries differed from the blocked layout's, by 3e-16 relative, on every operator.)"""
    L, _ = spk.AssembleOperator_Laplace(64)
    ld, lb, what = _vcycle_both_layouts(spk, L, vec(L.nrows, 13))
    print("generator's 64 x 64 operator: row-type against blocked fine layout,", what)
    assert np.array_equal(ld, lb)
    A = build(name)
    yd, yb, what = _vcycle_both_layouts(spk, A, vec(A.nrows, 13))
    print(f"{name}: row-type against blocked fine layout, {what}")
    assert np.array_equal(yd, yb)


# --------------------------------------------------------------------------- (8) refusals, and the largest tables
@pytest.mark.parametrize("name", REFUSED)
def test_refused_matrices_keep_the_blocked_kernels(spk, oracle, name):
    """a row beyond kDictMaxK, tables beyond the LDS budget, codes that do not fit their words: the blocked layout, the
    oracle's bits; and the context takes the generator's operator afterwards as a fresh one does"""
    A = build(name)
    x = vec(A.ncols, 5)
    L, _ = spk.AssembleOperator_Laplace(12, 9)
    xl = vec(L.nrows, 3)
    with _env({}):
        with _set(spk, A) as c:
            _check_layout(name, c)
            assert np.array_equal(c.mult(x), oracle.spmv(A, x))
            c.set_block(spk.BLOCK_A00, L)
            lay = c.dict_layout()
            assert c.spmv_info()["format"] == "dict2x2" and lay["ok"] == 1 and (lay["kmax"], lay["product_kernel"]) == (9, 1)
            assert np.array_equal(c.mult(xl), oracle.spmv(L, xl))


def test_largest_accepted_tables(spk, oracle):
    """nlds: tables between 0.8 x 48 KB and 48 KB.  Product, sweeps and a form-5 solve with B (the rider's launch beside the
    largest tables) bit for bit those of the blocked layout"""
    A = build("nlds")
    B = sparse_rows(A.nrows, 4)
    x, rhs = vec(A.nrows, 5), vec(A.nrows + 4, 10)
    out = {}
    for key, env in (("dict", {}), ("bcsr", BCSR)):
        with _env(env):
            with _set(spk, A) as c:
                if key == "dict":
                    lay = _check_layout("nlds", c)
                    assert 0.8 * 48 * 1024 <= lay["lds_bytes"] <= 48 * 1024
                y = c.mult(x)
                c.pc_setup(spk.PC_JACOBI, 0, inner_sweeps=2, inner_omega=OMEGA)
                z = c.pc_apply(x)
            with _set(spk, A, B) as c:
                c.pc_setup(spk.PC_SCHUR, spk.SCHUR_FULL)
                xs, info = c.fgmres(rhs, rtol=1e-30, max_it=45, iteration_form=FORM5)
                assert c.iteration_form()[0] == FORM5
            out[key] = (y, z, xs, info["history"])
    assert np.array_equal(out["dict"][0], oracle.spmv(A, x))
    assert np.array_equal(out["dict"][1], oracle.pc_apply_inner(A, None, oracle.PC_JACOBI, 0, 2, OMEGA, x))
    assert len(out["dict"][3]) > 1
    for a, b in zip(out["dict"], out["bcsr"]):
        assert np.array_equal(a, b)
