"""The seams of form 7's fused Gram-Schmidt launch (spk_k_iter.hip gs_fused_kernel): the multi-value wave reduction that
ends its VecMDot pass (spk_device.hpp wave_sum_multi) against the one-value shuffle chain, the launch against forced
form 5 on the shapes where its first tile, its accumulator groups and the end of a restart cycle meet, and the `done` gate
looked at behind the first loads.  Everything is compared bit for bit.  Needs a real MI355X: run with -m gpu."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

UN3, GSF = 5, 7


@functools.lru_cache(maxsize=None)
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


def _wave_sum_inputs(na):
    """na x 512 finite values: mixed signs over 2^-30 .. 2^30, a row of +0, a row of -0, a row of both, a row of
    denormals, a row of denormals among normal values.  No NaN (payload choice does not commute; real data has none)."""
    rng = np.random.default_rng(1000 + na)
    v = rng.choice([-1.0, 1.0], (na, 512)) * rng.uniform(1.0, 2.0, (na, 512)) * 2.0 ** rng.integers(-30, 31, (na, 512))
    v[1] = 0.0
    v[2] = -0.0
    v[3] = np.where(rng.integers(0, 2, 512) == 1, 0.0, -0.0)
    v[4] = rng.choice([-1.0, 1.0], 512) * rng.integers(1, 1 << 20, 512) * 5e-324
    v[5] = np.where(rng.integers(0, 2, 512) == 1, v[4], v[5] * 2.0 ** -1000)
    v[na - 1] = np.abs(v[na - 1])   # the w.w slot: one sign
    return v


@pytest.mark.parametrize("na", [9, 17, 25, 33, 41])
def test_multi_value_wave_reduction_is_the_shuffle_chain_bit_for_bit(spk, na):
    """One 512-thread workgroup, the NA = 8 NG + 1 accumulators of VecMDot's groups NG = 1 .. 5: all 8 x NA wave sums by
    wave_sum_multi carry the bits of wave_sum's chain (the same tree per value; IEEE addition commutes)."""
    v = _wave_sum_inputs(na)
    with spk.Context(0) as c:
        out = c.debug_wave_sums(v)
    assert out.shape == (2, 8, na)
    # the chain itself adds what it should (lane 0's tree: 32, 16, 8, 4, 2, 1 apart)
    t = v.reshape(na, 8, 64).copy()
    for off in (32, 16, 8, 4, 2, 1):
        t = t[:, :, :off] + t[:, :, off:2 * off]
    assert np.array_equal(out[0].view(np.uint64), np.ascontiguousarray(t[:, :, 0].T).view(np.uint64))
    assert np.array_equal(out[1].view(np.uint64), out[0].view(np.uint64))


@pytest.mark.parametrize("mx,my,saddle,fact,restart", [
    (1024, 512, True, 3, 30),    # the smallest fat shape: one tile per workgroup, NG = 1 .. 5, the end of a cycle
    (1024, 516, True, 3, 30),    # 258 tiles: two workgroups have a second tile
    (1024, 512, False, 3, 30),   # Jacobi on K = A (MP = 0)
    (1024, 512, True, 1, 4),     # LOWER; the cycle's last iteration every few launches
    (1024, 512, True, 1, 2),
    (1024, 512, True, 3, 1),     # the only iteration of a cycle is its first and its last
])
def test_fused_launch_is_form_5_bit_for_bit_at_its_seams(spk, mx, my, saddle, fact, restart):
    """45 iterations, rtol = abstol = 0: AUTO (form 7) and forced form 5 leave the same history and the same x."""
    A, B, rhs = _system(spk, mx, my, saddle)
    with _ctx(spk, A, B, fact) as c:
        x7, i7 = c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=45, restart=restart)
        assert c.iteration_form()[0] == GSF
        x5, i5 = c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=45, restart=restart, iteration_form=UN3)
        assert c.iteration_form()[0] == UN3
    assert i7["its"] == i5["its"] == 45 and i7["reason"] == i5["reason"]
    assert np.array_equal(i7["history"], i5["history"]) and np.array_equal(x7, x5)


def test_gate_behind_the_first_loads_stops_the_solve_where_form_5_stops(spk):
    """A tolerance between entries 17 and 18 of the history: the solve ends in the middle of a cycle, the launches enqueued
    behind the stop are gated off.  AUTO (form 7), forced form 5 and the host checking every iteration (check_every = 1:
    no gated launch at all) stop at the same iteration for the same reason with the same bits -- a gated fused launch
    publishes nothing and leaves the armed totals line alone, or the solve after it would differ."""
    A, B, rhs = _system(spk, 1024, 512, True)
    with _ctx(spk, A, B) as c:
        _, i0 = c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=45, restart=30, iteration_form=UN3)
        h = i0["history"]
        assert h[18] < h[17]
        rtol = float(np.sqrt(h[17] * h[18]) / h[0])
        x7, i7 = c.fgmres(rhs, rtol=rtol, restart=30)
        assert c.iteration_form()[0] == GSF
        x5, i5 = c.fgmres(rhs, rtol=rtol, restart=30, iteration_form=UN3)
        assert c.iteration_form()[0] == UN3
        x1, i1 = c.fgmres(rhs, rtol=rtol, restart=30, check_every=1)
        assert c.iteration_form()[0] == GSF
        xa, ia = c.fgmres(rhs, rtol=rtol, restart=30)   # behind gated launches: partials and totals line still armed
    assert i7["its"] == i5["its"] == i1["its"] == ia["its"] and 0 < i7["its"] < 30
    assert i7["reason"] == i5["reason"] == i1["reason"] == ia["reason"] == 2
    for x, i in ((x5, i5), (x1, i1), (xa, ia)):
        assert np.array_equal(i["history"], i7["history"]) and np.array_equal(x, x7)
