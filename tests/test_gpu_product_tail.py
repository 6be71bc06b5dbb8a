"""The row tail of the A-block product -- off-rank columns, then B^T lambda, then += y -- is one piece of device code
(row_tail_add / BtPre in spk_device.hpp) under six kernels.  What it adds must not depend on the layout: the same bits from
the CSR stream kernel, the blocked kernels, the plain and the pipelined row-type kernels, on rows with B^T entries (fewer and
more of them than the early fetch takes), on rows with off-rank columns, and with ACC and the rider in a solve.
Needs a real MI355X: run with -m gpu."""
import contextlib
import os
import threading

import numpy as np
import pytest

from conftest import relerr
from test_gpu_parity import _six_row_constraints

pytestmark = pytest.mark.gpu

KERNEL_TOL = 1e-13
MX, MY = 30, 22

# name -> environment the operator is set and used under
LAYOUTS_2D = {"csr": {"SPK_SPMV_FORMAT": "csr"}, "bcsr": {"SPK_SPMV_FORMAT": "bcsr"}, "dict2": {},
              "dict2_per_class": {"SPK_DICT_NOUNIFORM": "1"}}
LAYOUTS_STRADDLE = {"csr": {"SPK_SPMV_FORMAT": "csr"}, "bcsr": {"SPK_SPMV_FORMAT": "bcsr"}, "dict_plain": {}}
LAYOUTS_3D = {"bcsr": {"SPK_SPMV_FORMAT": "bcsr"}, "dict": {}, "dict_per_class": {"SPK_DICT_NOUNIFORM": "1"},
              "dict3_pipelined": {"SPK_DICT3_PIPELINE": "1"}}
LAYOUTS_SLAB = {"csr": {"SPK_SPMV_FORMAT": "csr"}, "bcsr": {"SPK_SPMV_FORMAT": "bcsr"}, "dict2": {}}
KNOBS = ("SPK_SPMV_FORMAT", "SPK_DICT_NOUNIFORM", "SPK_DICT3_PIPELINE")


@contextlib.contextmanager
def _env(values):
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(values)
    try:
        yield
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def _x(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


def _straddling(spk, A):
    """test_dictionary_fields_across_the_halves' matrix at this size: entry (0, 0) of the diagonal blocks scattered over
    2^23 granules of 2^-46, a field across the halves of the code word -- the pipelined product stands back."""
    val = A.val.copy()
    rng = np.random.default_rng(11)
    rows = np.repeat(np.arange(A.nrows), np.diff(A.rowptr))
    diag = (np.abs(val) > 1e-3) & (rows == A.colidx) & (rows % 2 == 0)
    val[diag] += rng.integers(-2**22, 2**22, int(diag.sum())) * 2.0**-46
    return spk.CSR(A.rowptr, A.colidx, val, A.ncols)


def _eight_row_constraints(spk, mx, my):
    """the six rows + the x- and the xy-moment of Ux: five B^T entries on every constrained Ux row, one more than the early
    fetch takes (the six-row block has three per row), and still m <= 8: the rows ride in the product's tail"""
    B6, _ = _six_row_constraints(spk, mx, my)
    rows = [(B6.colidx[B6.rowptr[r]:B6.rowptr[r + 1]], B6.val[B6.rowptr[r]:B6.rowptr[r + 1]]) for r in range(6)]
    hx, hy = 1.0 / (mx - 1), 1.0 / (my - 1)
    c0, _ = rows[0]; node = c0 // 2
    xm, ym = (node % mx) * hx - 0.5, (node // mx) * hy - 0.5
    rows += [(c0, hx * hy * xm), (c0, hx * hy * xm * ym)]
    rp = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int32)
    return spk.CSR(rp, np.concatenate([c for c, _ in rows]), np.concatenate([v for _, v in rows]), B6.ncols)


def nest_runs(spk, A, B, rhs, x, layouts, solve):
    """per layout: format, K [x; lambda], and (solve) FGMRES form 5 to 45 iterations: ACC and the rider in every product"""
    out = {}
    for name, env in layouts.items():
        with _env(env), spk.Context(0) as c:
            c.set_block(spk.BLOCK_A00, A)
            c.set_block(spk.BLOCK_A10, B)
            r = dict(format=c.spmv_info()["format"], y=c.mult(x))
            if solve:
                c.pc_setup(spk.PC_SCHUR, spk.SCHUR_FULL)
                r["sol"], info = c.fgmres(rhs, rtol=1e-30, max_it=45, iteration_form=5)
                r["history"] = np.asarray(info["history"])
            out[name] = r
    return out


def slab_runs(spk, mx, my, x, layouts, P=3):
    """test_dictionary_row_slabs' arrangement: P logical ranks, rows at a cut add off-rank columns in the tail"""
    out = {}
    for name, env in layouts.items():
        with _env(env):
            grp = spk.LocalGroup(P)
            outs, fmts, errs = [None] * P, [None] * P, []

            def work(r):
                try:
                    rb, re_ = spk.partition_slab(mx, my, r, P)
                    Ar, _ = spk.AssembleOperator_Laplace(mx, my, rb, re_)
                    with spk.Context(0) as c:
                        c.comm_init_local(grp, r)
                        c.set_block(spk.BLOCK_A00, Ar)
                        fmts[r] = c.spmv_info()["format"]
                        outs[r] = c.mult(x[rb:re_])
                except Exception as e:  # noqa: BLE001
                    errs.append(e)
            th = [threading.Thread(target=work, args=(r,)) for r in range(P)]
            [t.start() for t in th]
            [t.join() for t in th]
            grp.close()
            assert not errs, errs
            out[name] = dict(format=fmts, y=np.concatenate(outs))
    return out


@pytest.fixture(scope="module")
def system_2d(spk):
    A, f = spk.AssembleOperator_Laplace(MX, MY)
    B6, g6 = _six_row_constraints(spk, MX, MY)
    assert B6.nrows == 6
    return A, B6, np.concatenate([f, g6]), _x(A.nrows + 6, 6)


@pytest.fixture(scope="module")
def runs_2d(spk, system_2d):
    A, B6, rhs, x = system_2d
    return nest_runs(spk, A, B6, rhs, x, LAYOUTS_2D, solve=True)


@pytest.fixture(scope="module")
def runs_straddle(spk, system_2d):
    A, B6, rhs, x = system_2d
    return nest_runs(spk, _straddling(spk, A), B6, rhs, x, LAYOUTS_STRADDLE, solve=True)


def _same_everywhere(runs, key, n=None):
    names = list(runs)
    for name in names[1:]:
        assert np.array_equal(runs[name][key][:n], runs[names[0]][key][:n]), (key, name, names[0])


def test_bt_rows_same_bits_in_every_2d_layout(spk, oracle, system_2d, runs_2d):
    """the six-row block (three B^T entries on a constrained row): CSR, 2x2-blocked, pipelined row types with the uniform
    and the per-class fields"""
    A, B6, _, x = system_2d
    assert [runs_2d[k]["format"] for k in LAYOUTS_2D] == ["csr", "bcsr2x2", "dict2x2", "dict2x2"]
    _same_everywhere(runs_2d, "y", A.nrows)
    y_ref = oracle.apply_K(A, B6, x)
    for name, r in runs_2d.items():
        assert relerr(r["y"], y_ref) < KERNEL_TOL, name


def test_bt_rows_same_bits_in_the_plain_row_type_kernel(spk, oracle, system_2d, runs_straddle):
    A, B6, _, x = system_2d
    assert [runs_straddle[k]["format"] for k in LAYOUTS_STRADDLE] == ["csr", "bcsr2x2", "dict2x2"]
    _same_everywhere(runs_straddle, "y", A.nrows)
    y_ref = oracle.apply_K(_straddling(spk, A), B6, x)
    for name, r in runs_straddle.items():
        assert relerr(r["y"], y_ref) < KERNEL_TOL, name


def test_bt_rows_beyond_the_early_fetch(spk, oracle, system_2d):
    """five B^T entries on a row: the loop behind BtPre's four (blocked and plain row-type kernels) against the one loop
    of the CSR and the pipelined kernels"""
    A, _, _, _ = system_2d
    B8 = _eight_row_constraints(spk, MX, MY)
    assert B8.nrows == 8 and np.bincount(B8.colidx).max() == 5
    x = _x(A.nrows + 8, 7)
    for mat, layouts in ((A, LAYOUTS_2D), (_straddling(spk, A), LAYOUTS_STRADDLE)):
        runs = nest_runs(spk, mat, B8, None, x, layouts, solve=False)
        _same_everywhere(runs, "y", A.nrows)
        y_ref = oracle.apply_K(mat, B8, x)
        for name, r in runs.items():
            assert relerr(r["y"], y_ref) < KERNEL_TOL, name


def test_bt_rows_same_bits_in_every_3d_layout(spk, oracle):
    A, _ = spk.AssembleOperator_Laplace3D(14, 11, 9)
    B, _ = spk.AssembleOperator_Constraints3D(14, 11, 9)
    assert B.nrows <= 8
    x = _x(A.nrows + B.nrows, 4)
    runs = nest_runs(spk, A, B, None, x, LAYOUTS_3D, solve=False)
    assert [runs[k]["format"] for k in LAYOUTS_3D] == ["bcsr3x3", "dict3x3", "dict3x3", "dict3x3"]
    _same_everywhere(runs, "y", A.nrows)
    y_ref = oracle.apply_K(A, B, x)
    for name, r in runs.items():
        assert relerr(r["y"], y_ref) < KERNEL_TOL, name


def test_off_rank_rows_same_bits_in_every_layout(spk, oracle):
    mx = my = 36
    A, _ = spk.AssembleOperator_Laplace(mx, my)
    x = _x(A.nrows, 11)
    runs = slab_runs(spk, mx, my, x, LAYOUTS_SLAB)
    assert [runs[k]["format"][0] for k in LAYOUTS_SLAB] == ["csr", "bcsr2x2", "dict2x2"]
    assert all(len(set(r["format"])) == 1 for r in runs.values())
    _same_everywhere(runs, "y")                              # every row, cut rows included
    cut = np.zeros(A.nrows, bool)
    for r in range(1, 3):
        rb, _ = spk.partition_slab(mx, my, r, 3)
        cut[rb - 2 * mx:rb + 2 * mx] = True
    y_ref = oracle.spmv(A, x)
    for name, r in runs.items():
        assert np.array_equal(r["y"][~cut], y_ref[~cut]), name


def test_acc_and_rider_same_iterates_in_every_layout(runs_2d, runs_straddle):
    """FGMRES form 5, Schur FULL: every product of the iterations accumulates onto B^T lambda and carries the rider"""
    for runs in (runs_2d, runs_straddle):
        assert all(len(r["history"]) > 1 for r in runs.values())
        _same_everywhere(runs, "history")
        _same_everywhere(runs, "sol")
