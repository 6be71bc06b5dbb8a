"""The edges of the pipelined row-type product (spmv_dict2_kernel, spk_k_dict.hip): its first requests go out before the
tables are in LDS, a stage is requested one chunk ahead of the one being decoded, and y is stored through a range-checked
buffer.  Grids chosen for where that can go wrong (dof 2, 256 block rows per chunk):

  16 x 16   256 block rows: exactly one chunk; the stage requested ahead lies beyond the workgroup's range
  17 x 16   272 block rows: a partial last chunk (its rows beyond the end are dropped by the store's range check)
  48 x 48   2304 block rows, 9 chunks: XCD 4 gets one chunk, XCDs 5-7 none; with SPK_DICT2_WGS = 2 / 3 a workgroup walks
            4 / 3 chunks -- the loop left after its second / its first half, and a short last workgroup

Everything is compared bit for bit: with the oracle's product, and with the same context under SPK_SPMV_FORMAT=csr
(products, residual histories and solutions of form-5 solves: y += A x with the Givens rider under Schur FULL, y = A x
with the rider under Jacobi).  Needs a real MI355X: run with -m gpu."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import relerr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _product_pipeline_worker as W  # noqa: E402

pytestmark = pytest.mark.gpu

GRIDS = [(16, 16), (17, 16), (48, 48)]
KEYS = ("y_plain", "y_bt", "jac_hist", "jac_x", "full_hist", "full_x")


@pytest.fixture(scope="module")
def runs(spk):
    """grid -> arrays of _product_pipeline_worker.run_grid, computed once"""
    os.environ.pop("SPK_DICT2_WGS", None)
    return {g: W.run_grid(spk, *g) for g in GRIDS}


def _check(spk, oracle, r, mx, my):
    assert str(r["dict_format"]) == "dict2x2" and str(r["csr_format"]) == "csr"
    for k in KEYS:
        assert np.all(np.isfinite(r["dict_" + k])), k
        assert np.array_equal(r["dict_" + k], r["csr_" + k]), (k, mx, my)
    assert len(r["dict_jac_hist"]) > 1 and len(r["dict_full_hist"]) > 1
    A, _, B, _, x, xs = W.inputs(spk, mx, my)
    assert np.array_equal(r["dict_y_plain"], oracle.spmv(A, x))
    # K [x; lambda]: the rows of A add their B^T entries behind A x, one fused multiply-add each -- the CSR kernel's
    # spelling, held bit for bit above; the oracle contracts nothing, so it is held to test_gpu_product_tail's bound
    assert r["dict_y_bt"].shape == (A.nrows + B.nrows,)
    assert relerr(r["dict_y_bt"], oracle.apply_K(A, B, xs)) < 1e-13


@pytest.mark.parametrize("mx,my", GRIDS)
def test_pipeline_edges_bitwise(spk, oracle, runs, mx, my):
    _check(spk, oracle, runs[(mx, my)], mx, my)


@pytest.mark.parametrize("wgs", [2, 3])
def test_chunks_per_workgroup_bitwise(spk, oracle, runs, tmp_path, wgs):
    """48 x 48 with 4 / 3 chunks per workgroup, in a fresh process (the knob is read once): the same bits as the default
    launch, the CSR kernel and the oracle"""
    out = tmp_path / "wgs.npz"
    env = dict(os.environ, SPK_DICT2_WGS=str(wgs))
    env.pop("SPK_SPMV_FORMAT", None)
    subprocess.run([sys.executable, W.__file__, "48", "48", str(out)], env=env, check=True, timeout=120)
    r = dict(np.load(out))
    _check(spk, oracle, r, 48, 48)
    for k in KEYS:
        assert np.array_equal(r["dict_" + k], runs[(48, 48)]["dict_" + k]), k


def test_gated_launch_is_timed(spk):
    """the launch the device gates off at a solve's end still returns (bench.py reads its cost as spmv_gated)"""
    A, f = spk.AssembleOperator_Laplace(48, 48)
    B, g = spk.AssembleOperator_Constraints(48, 48)
    with spk.Context(0) as c:
        c.set_block(spk.BLOCK_A00, A)
        c.set_block(spk.BLOCK_A10, B)
        c.pc_setup(spk.PC_SCHUR, spk.SCHUR_FULL)
        assert c.spmv_info()["format"] == "dict2x2"
        c.fgmres(np.concatenate([f, g]), **W.SOLVE)      # (the gated launch is timed on the state a solve leaves)
        ms = c.time_kernel("spmv_gated", 0, 5, 20)
    assert math.isfinite(ms) and ms >= 0.0
