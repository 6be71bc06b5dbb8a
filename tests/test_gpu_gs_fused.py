"""Form 7 (opts.iteration_form = 7, spk_k_iter.hip gs_fused_kernel): form 5 with VecMDot and the VecMAXPY + PCApply pass
in one launch on fat vectors (>= 1 M local rows).  Same tiles and summation orders as the two launches of form 5, so the
two forms must agree bit for bit.  Needs a real MI355X: run with -m gpu."""
import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu

UN3, GSF = 5, 7


def _system(spk, mx, my, saddle):
    A, f = spk.AssembleOperator_Laplace(mx, my)
    if not saddle:
        return A, None, f
    B, g = spk.AssembleOperator_Constraints(mx, my)
    return A, B, np.concatenate([f, g])


def _ctx(spk, A, B, fact=3):
    c = spk.Context(0)
    c.set_block(spk.BLOCK_A00, A)
    if B is not None:
        c.set_block(spk.BLOCK_A10, B)
    c.pc_setup(spk.PC_SCHUR if B is not None else spk.PC_JACOBI, fact)
    return c


@pytest.mark.parametrize("mx,my,saddle,fact", [(1024, 1024, True, 3), (1024, 1024, True, 1), (1024, 1024, False, 3),
                                               (1030, 1030, True, 3), (1024, 512, True, 3), (1024, 512, False, 3)])
def test_fused_gram_schmidt_is_form_5_bit_for_bit(spk, mx, my, saddle, fact):
    """45 iterations (one whole cycle of 30 and half of the next, restart 30, rtol 0): AUTO takes form 7 on these fat
    vectors, and its residual history and solution are the same bits as forced form 5.  Schur FULL and LOWER, Jacobi on
    K = A (DIAG has no fused head path: it runs step by step, where neither form applies).  1030^2: a partial last tile;
    1024 x 512: the smallest fat vector (exactly 256 tiles of 2048 double2)."""
    A, B, rhs = _system(spk, mx, my, saddle)
    with _ctx(spk, A, B, fact) as c:
        x7, i7 = c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=45, restart=30)
        assert c.iteration_form()[0] == GSF
        x5, i5 = c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=45, restart=30, iteration_form=UN3)
        assert c.iteration_form()[0] == UN3
    assert i7["its"] == i5["its"] == 45 and i7["reason"] == i5["reason"]
    assert np.array_equal(i7["history"], i5["history"]) and np.array_equal(x7, x5)


def test_fused_gram_schmidt_max_it_mid_cycle(spk, oracle):
    """-ksp_max_it ending the solve in the middle of a cycle: the count and reason of the oracle, its history."""
    A, B, rhs = _system(spk, 1024, 1024, True)
    with _ctx(spk, A, B) as c:
        _, tr = c.fgmres(rhs, rtol=1e-30, max_it=47, iteration_form=GSF)
        assert c.iteration_form()[0] == GSF
    _, it = oracle.fgmres(A, rhs, B=B, pc_type=oracle.PC_SCHUR, schur_fact=oracle.SCHUR_FULL, rtol=1e-30, max_it=47,
                          threads=8)
    assert tr["its"] == it["its"] == 47 and tr["reason"] == it["reason"] == -3
    assert np.allclose(tr["history"][:20], it["history"][:20], rtol=1e-6)


def test_fused_gram_schmidt_wait_that_gives_up_leaves_the_context_usable(spk, oracle):
    """The in-launch waits (MDot partials, the totals line) bounded to one tick: SPK_ERR_HIP, never a numerical reason; the
    next solve with the bound restored reproduces the undisturbed one bit for bit (partials and totals lines re-armed)."""
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


def test_auto_takes_fused_gram_schmidt_only_on_fat_vectors(spk):
    """AUTO: form 7 at 1024^2 (2 M rows), form 5 at 512^2 (0.5 M rows: thin vectors) and where restart + m > 41."""
    for M, restart, want in ((1024, 30, GSF), (512, 30, UN3), (1024, 40, UN3)):
        A, B, rhs = _system(spk, M, M, True)
        with _ctx(spk, A, B) as c:
            c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=3, restart=restart)
            assert c.iteration_form()[0] == want, (M, restart)
