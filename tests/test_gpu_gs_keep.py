"""Form 7's keep set (spk_k_iter.hip gs_fused_kernel, KeepSet in spk_device.hpp): the operands of each workgroup's first
tile -- w~, the parity planes of B D, V_0 .. V_3 -- stay in registers and LDS between VecMDot's pass and kernel B's pass
instead of being read from HBM twice.  A kept value is the very 64 bits a second load would return and no addition moves,
so the launch with its keep set, the one without (SPK_GS_KEEP=0, read per solve) and forced form 5 must agree bit for bit.
Needs a real MI355X: run with -m gpu."""
import numpy as np
import pytest

import _gs_rig as R
from _gs_rig import GSF, UN3, _ctx
from conftest import relerr

pytestmark = pytest.mark.gpu


def _system(spk, mx, my, saddle):
    return R._system(spk, (mx, my), saddle)


def _three_solves(c, rhs, monkeypatch, restart, max_it=45):
    """AUTO with the keep set, AUTO with SPK_GS_KEEP=0, forced form 5 -- on ONE context (the knob is read per solve)."""
    monkeypatch.delenv("SPK_GS_KEEP", raising=False)
    xk, ik = c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=max_it, restart=restart)
    fk = c.iteration_form()[0]
    monkeypatch.setenv("SPK_GS_KEEP", "0")
    x0, i0 = c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=max_it, restart=restart)
    f0 = c.iteration_form()[0]
    monkeypatch.delenv("SPK_GS_KEEP")
    x5, i5 = c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=max_it, restart=restart, iteration_form=UN3)
    assert c.iteration_form()[0] == UN3
    return (xk, ik, fk), (x0, i0, f0), (x5, i5)


def _assert_same_bits(k, n, u, its):
    (xk, ik, _), (x0, i0, _), (x5, i5) = k, n, u
    assert ik["its"] == i0["its"] == i5["its"] == its and ik["reason"] == i0["reason"] == i5["reason"]
    assert np.array_equal(ik["history"], i5["history"]) and np.array_equal(xk, x5)
    assert np.array_equal(i0["history"], i5["history"]) and np.array_equal(x0, x5)


@pytest.mark.parametrize("mx,my,saddle,fact,restart", [
    (1024, 1024, True, 3, 30),    # Schur FULL: w~, two parity planes, V_0..V_3 kept (NG 1..4), w~ and V_0..V_3 at NG = 5
    (1024, 1024, True, 1, 30),    # Schur LOWER
    (1024, 1024, False, 3, 30),   # Jacobi on K = A: MP = 0, no planes
    (1024, 512, True, 3, 30),     # one tile per workgroup: every operand of j <= 3 kept
    (1030, 1030, True, 3, 30),    # a partial last tile; some workgroups have three tiles
    (1536, 1536, True, 3, 30),    # four to five tiles per workgroup
    (1024, 1024, True, 3, 4),     # restart 4: nv never exceeds the four kept basis vectors
])
def test_keep_set_changes_no_bit(spk, monkeypatch, mx, my, saddle, fact, restart):
    """45 iterations, rtol 0 (restart 30: one whole cycle and half of the next, NG = 1..5): residual history and solution
    of the launch with its keep set == without it == forced form 5, np.array_equal."""
    A, B, rhs = _system(spk, mx, my, saddle)
    with _ctx(spk, A, B, fact) as c:
        k, n, u = _three_solves(c, rhs, monkeypatch, restart)
    assert k[2] == GSF and n[2] == GSF
    _assert_same_bits(k, n, u, 45)


def test_keep_set_3d_six_constraint_rows(spk, monkeypatch):
    """A fat 3-D system with the six rigid-body constraint rows (m = 6: MP = 8, planes of B D read one at a time inside
    the tile loop, none of them kept; w~ and V_0..V_3 are).  AUTO takes form 7 for it (observed on an MI355X; asserted,
    not forced), with and without the keep set, and the three solves are the same bits."""
    grid = (128, 128, 32)   # 1.57 M rows: fat vectors
    A, B, rhs = R._system(spk, grid, True)
    with _ctx(spk, A, B) as c:
        k, n, u = _three_solves(c, rhs, monkeypatch, 30)
    print(f"3-D {grid}, m = {B.nrows}: AUTO resolved to form {k[2]} (SPK_GS_KEEP=0: {n[2]})")
    assert k[2] == n[2] == GSF
    _assert_same_bits(k, n, u, 45)


def test_keep_set_wait_that_gives_up_leaves_the_context_usable(spk, oracle, monkeypatch):
    """The bounded in-launch waits with the keep set on: one tick -> SPK_ERR_HIP, never a numerical reason; the next solve
    with the bound restored reproduces the undisturbed one bit for bit."""
    monkeypatch.delenv("SPK_GS_KEEP", raising=False)
    A, B, rhs = _system(spk, 1024, 1024, True)
    with _ctx(spk, A, B) as c:
        x0, i0 = c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=45, iteration_form=GSF)
        assert c.iteration_form()[0] == GSF
        c.debug_set_wait_bound(1)
        with pytest.raises(spk.SpkError, match="timed out") as ei:
            c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=45, iteration_form=GSF)
        assert ei.value.code == -2
        c.debug_set_wait_bound(0)
        x1, i1 = c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=45, iteration_form=GSF)
        y = c.mult(rhs)
    assert i1["its"] == i0["its"] == 45 and np.array_equal(i1["history"], i0["history"]) and np.array_equal(x1, x0)
    assert relerr(y, oracle.apply_K(A, B, rhs)) < 1e-13
