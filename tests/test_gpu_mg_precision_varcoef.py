"""-spk_mg_precision single on the GPU with row-to-row varying values: the FP32 kernels of spk_k_amg.hip
(amg_stencil_f32_kernel, the float transfers and amg_cheb_vec_kernel, the float dense product, amg_stencil_tail_f32_kernel,
amg_round_f32_kernel) on the operator family of tests/_mg_fields.py.  tests/test_gpu_mg_precision.py runs them on
constant-coefficient operators, where the float32 D^-1 of every x-interior row of level 1 has the bits of the previous
node's (tests/test_mg_precision_varcoef_cpu.py counts them: all 408 on 33x33), so that its bit-for-bit checks pass a float
kernel that reads D^-1 one node off; on five17x9 the stored rows are equal too.  Under `smooth`, `lognormal`, `dad` and
`skew` no such row shares either.

Tried once on an MI355X against a library whose so_row (spk_stencil_op_core.hpp) on float read D^-1 of the previous node in
x at the nodes 3 <= i <= nx - 3: the hook check, the one-application check and the tail check of test_gpu_mg_precision
passed on all of its shapes (22 of 22), while the hook check and the one-application check below failed on every one of the
18 (shape, field) cases.  test_mg_precision_varcoef_cpu.py holds the host statement of the same mistake as assertions.

The assertions are those of test_gpu_mg_precision on other values, with the one-application bar taken per coefficient
region; bars, iteration allowances and scaling exponents come from test_mg_precision_varcoef_cpu.py, from the numpy
references alone.  Nothing here is larger than 65 x 33 (4290 rows; 33 x 33 has 2178) or 17 x 9 x 5."""
import numpy as np
import pytest
import scipy.sparse as sp

import _mg_fields as F
import saddle_point_petsc_amd as S
from test_gpu_mg_cycle import _tail_rows
from test_gpu_mg_grid import _ctx, _scipy
from test_gpu_mg_operator import STEPS, _vec
from test_gpu_mg_precision import _ordered, _step32, _vec32
from test_gpu_mg_varcoef import SOLVED
from test_mg_precision_cpu import vcycle_ref_mixed
from test_mg_precision_varcoef_cpu import SCALE_K, allowance, bar, mixed_against_double, numpy_iterations
from test_mg_sides_cpu import hierarchy_mats

pytestmark = pytest.mark.gpu
F32 = np.float32
CASES = F.cases(skew=True)
CYCLES = (("v", 1, "launches"), ("w", 2, "fused"))
TINY = np.finfo(F32).tiny   # 2^-126, the smallest normal float


def _kw(shape, **kw):
    """the all-stencil route on the device set-up"""
    assert max(F.SHAPES[shape][0]) <= 65
    return F.stencil_kw(shape, **dict(dict(setup="device"), **kw))


def _dinv32(rp, ci, v, shape):
    """the FP64 D^-1 of a downloaded level, rounded once: what amg_round_f32_kernel's copy holds, row for row"""
    return (1.0 / sp.csr_matrix((v, ci, rp), shape=shape).diagonal()).astype(F32)


# ---- 1. the hooks: bit for bit against numpy float32 ---------------------------------------------------------------------
@pytest.mark.parametrize("shape,field", CASES)
def test_hooks_are_numpy_float32_bit_for_bit(shape, field):
    """test_gpu_mg_precision.test_hooks_are_numpy_float32_bit_for_bit on these operators: the product, the three STEPS with
    the level's own D^-1 (the FP64 diagonal's inverse rounded once -- which also holds amg_round_f32_kernel's copies of
    D^-1 and of the values to the right row) and the `done` gate on every level between level 0 and the coarsest; prolong
    and restrict on every level, level 0's two boundary forms (float -> double, double -> float) included."""
    A = F.operator(shape, field)
    with _ctx(A, amg=_kw(shape, precision="single")) as c:
        info = c.amg_info()
        L = info["levels"]
        assert info["precision"] == S.AMG_PRECISION_SINGLE and info["operator"] == S.AMG_OPERATOR_STENCIL and L >= 3
        for l in range(1, L - 1):
            rp, ci, v, shp = c.amg_level(l)
            n = shp[0]
            x, xo, b = _vec32(n, 10 + l), _vec32(n, 20 + l), _vec32(n, 30 + l)
            dinv = _dinv32(rp, ci, v, shp)
            d = _ordered(rp, ci, v, x, F32)
            sentinel = _vec32(n, 40 + l)
            got = c.debug_amg_operator(l, "product", x, precision="single")
            assert got.dtype == F32 and got.tobytes() == d.tobytes(), f"{shape} {field} level {l}: the product is not the stated float32 sum"
            for alpha, beta, given in STEPS:
                yo = xo if given else None
                ref = _step32(d, x, dinv, b, alpha, beta, yo)
                got = c.debug_amg_operator(l, "step", x, b=b, xo=yo, alpha=alpha, beta=beta, precision="single")
                assert got.tobytes() == ref.tobytes(), f"{shape} {field} level {l}: step ({alpha}, {beta}, xo {given}) is not the stated formula"
                kept = c.debug_amg_operator(l, "step", x, b=b, xo=yo, alpha=alpha, beta=beta, done=True, out=sentinel, precision="single")
                assert kept.tobytes() == sentinel.tobytes(), f"{shape} {field} level {l}: the step wrote behind a set done gate"
            kept = c.debug_amg_operator(l, "product", x, done=True, out=sentinel, precision="single")
            assert kept.tobytes() == sentinel.tobytes(), f"{shape} {field} level {l}: the product wrote behind a set done gate"
        for l in range(L - 1):
            prp, pci, pv, pshape = c.amg_level(l, S.AMG_PROLONG)
            P = sp.csr_matrix((pv, pci, prp), shape=pshape)
            P.sort_indices()
            R = P.T.tocsr()
            R.sort_indices()
            nf, nc = P.shape
            ti = np.float64 if l == 0 else F32   # the fine side's type
            e, y = _vec32(nc, 50 + l), _vec(nf, 60 + l).astype(ti)
            ref = y + _ordered(P.indptr, P.indices, P.data, e.astype(ti), ti)   # (level 0: e widened, the sums in float64)
            got = c.debug_amg_transfer(l, "prolong", e, y, precision="single")
            assert got.dtype == ti and got.tobytes() == ref.tobytes(), f"{shape} {field} level {l}: y + P e is not the stated sum"
            b, t = _vec(nf, 70 + l).astype(ti), _vec(nf, 80 + l).astype(ti)
            ref = _ordered(R.indptr, R.indices, R.data, b - t, ti).astype(F32)   # (level 0: one rounding on the store)
            got = c.debug_amg_transfer(l, "restrict", b, t, precision="single")
            assert got.dtype == F32 and got.tobytes() == ref.tobytes(), f"{shape} {field} level {l}: R (b - t) is not the stated sum"


# ---- 2. one application, per region --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,field", CASES)
def test_one_application_per_region(shape, field):
    """V with the launches and W with the fused tail against the numpy cycle with FP32 levels over the downloaded hierarchy
    and against the same context's `double` route, || y - ref || / || ref || over each coefficient region separately.  The
    bar is test_mg_precision_varcoef_cpu.bar: four times the largest per-region distance between the two numpy cycles over
    these cases (V 5.17e-7 from 65x33 smooth, W 3.27e-6 from 33x33 lognormal) -- the reasoning of
    test_gpu_mg_precision.test_one_application.  Against the `double` route the whole vector also differs by more than 1e-10:
    the FP32 levels ran (per region that bound would not hold: the stiff half of `jump` differs by 1.6e-11 on the CPU).
    Two applications give equal bytes.

    Measured on an MI355X, largest per region over the cases: off the `double` route V 1.18e-7 (65x33 smooth, stiff), W
    5.43e-7 (65x33 lognormal, soft) -- the CPU's 1.29e-7 and 8.18e-7; off the numpy cycle with FP32 levels V 2.80e-8 (65x33
    smooth), W 6.09e-7 (65x33 lognormal, soft: under W on `lognormal` a flipped rounding grows to the size of the FP32
    effect itself).  Whole vector off the `double` route at least 1.8e-9 (17x9x5 lognormal, V); the stiff half of 17x9x5
    `jump` 1.2e-11."""
    A = F.operator(shape, field)
    x = F.rhs(A.nrows)
    reg = F.regions(shape)
    for cycle, gamma, tail in CYCLES:
        limit = bar(gamma)[0]
        with S.Context(0) as c:
            c.set_block(S.BLOCK_A00, A)
            c.pc_setup(S.PC_JACOBI, amg=_kw(shape, precision="single", cycle=cycle, tail=tail))
            info = c.amg_info()
            assert info["precision"] == S.AMG_PRECISION_SINGLE and info["cycle"] == (cycle == "w")
            assert info["tail_first"] >= 1 if tail == "fused" else info["tail_first"] == -1
            y, y2 = c.pc_apply(x), c.pc_apply(x)
            mats = hierarchy_mats(c.amg_level, info)
            c.pc_setup(S.PC_JACOBI, amg=_kw(shape, precision="double", cycle=cycle, tail=tail))
            assert c.amg_info()["precision"] == S.AMG_PRECISION_DOUBLE
            yd = c.pc_apply(x)
        assert y.tobytes() == y2.tobytes()
        whole = float(np.linalg.norm(y - yd) / np.linalg.norm(yd))
        to_double = F.region_rel(y, yd, reg)
        cpu_whole, cpu_reg = mixed_against_double(shape, field, gamma)
        print(f"{shape} {field} {cycle}: off the double route {whole:.3e} whole, {to_double[0]:.3e} (soft) {to_double[1]:.3e} (stiff); "
              f"on the CPU {cpu_whole:.3e}, {cpu_reg[0]:.3e}, {cpu_reg[1]:.3e}; bar {limit:.3e}")
        ref = vcycle_ref_mixed(*mats, info["lambda_max"], x, gamma=gamma)
        err = F.region_rel(y, ref, reg)
        print(f"{shape} {field} {cycle}: off the numpy cycle with FP32 levels {err[0]:.3e} (soft) {err[1]:.3e} (stiff); bar {limit:.3e}")
        assert whole > 1e-10, (shape, field, cycle, whole)
        assert max(to_double) <= limit, (shape, field, cycle, to_double, limit)
        assert max(err) <= limit, (shape, field, cycle, err, limit)


# ---- 3. the fused tail gives the launches' bits -------------------------------------------------------------------------
@pytest.mark.parametrize("cycle", ["v", "w"])
@pytest.mark.parametrize("shape,field", F.cases(("33x33", "12x10any", "17x9x5")))
def test_fused_tail_gives_the_bits_of_the_launches(shape, field, cycle):
    """amg_stencil_tail_f32_kernel against the launches with tail_rows at the sizes of level 1, level 2 and the coarsest
    level (and 1: no tail): with level 1 inside, every FP32 stencil level runs in the tail with its own D^-1 and values"""
    A = F.operator(shape, field)
    x = _vec(A.nrows, 7)
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        c.pc_setup(S.PC_JACOBI, amg=_kw(shape, precision="single", cycle=cycle, tail="launches"))
        info = c.amg_info()
        assert info["tail_first"] == -1 and info["precision"] == S.AMG_PRECISION_SINGLE
        ref = c.pc_apply(x)
        assert np.all(np.isfinite(ref)) and np.any(ref != 0.0)
        firsts = set()
        for tr in _tail_rows(info["rows"]):
            c.pc_setup(S.PC_JACOBI, amg=_kw(shape, precision="single", cycle=cycle, tail="fused", tail_rows=tr))
            t = c.amg_info()["tail_first"]
            assert (t == -1) == (tr == 1)
            firsts.add(t)
            y = c.pc_apply(x)
            assert y.tobytes() == ref.tobytes(), f"{shape} {field} {cycle} tail_rows {tr} (tail_first {t}): {np.abs(y - ref).max():.3e} off the launches"
        assert any(0 < t < info["levels"] - 1 for t in firsts), firsts   # an FP32 stencil level ran inside the tail


# ---- 4. solves ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,field", SOLVED)
def test_k_equals_a_solves_like_the_double_route(shape, field):
    """FGMRES to rtol 1e-8: reason 2, the true residual against scipy's product at most 2e-8, and the `single` count within
    the numpy difference + 1 of the `double` count (test_mg_precision_varcoef_cpu.allowance: the numpy cycles give equal
    counts on every case, 9 / 9, 9 / 9, 15 / 15 and 16 / 16, so the allowance is 1)."""
    A, f = F.problem(shape, field)
    Asp = _scipy(A)
    its = {}
    for prec in ("single", "double"):
        with _ctx(A, amg=_kw(shape, precision=prec)) as c:
            assert c.amg_info()["precision"] == (prec == "single")
            x, info = c.fgmres(f, rtol=1e-8, max_it=200)
            res = np.linalg.norm(f - Asp @ x) / np.linalg.norm(f)
            print(f"{shape} {field} {prec} fgmres: {info['its']} iterations (numpy {numpy_iterations(shape, field)}), true residual {res:.2e}")
            assert info["reason"] == 2 and res <= 2e-8
            its[prec] = info["its"]
    assert abs(its["single"] - its["double"]) <= allowance(shape, field), (its, numpy_iterations(shape, field))


# ---- 5. the refresh rounds the new values ---------------------------------------------------------------------------------
@pytest.mark.parametrize("setup", ["device", "host"])
def test_a_refresh_to_other_values_gives_a_fresh_builds_bytes(setup):
    """33x33 built on `smooth` under `single` with reuse, then `lognormal` on the same pattern: the set-up refreshes, and one
    application has the bytes of a fresh `single` build on `lognormal` -- amg_round_levels ran behind the refresh on the new
    values, D^-1 included (after `smooth`, stale copies differ in the leading digit)."""
    A, A2 = F.operator("33x33", "smooth"), F.operator("33x33", "lognormal")
    assert np.array_equal(A2.colidx, A.colidx) and np.array_equal(A2.rowptr, A.rowptr)
    x = F.rhs(A.nrows, 9)
    kw = _kw("33x33", setup=setup, precision="single")
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        c.pc_setup(S.PC_JACOBI, amg=kw, amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is False and c.amg_info()["precision"] == S.AMG_PRECISION_SINGLE
        y1 = c.pc_apply(x)
        c.set_block(S.BLOCK_A00, A2)
        c.pc_setup(S.PC_JACOBI, amg=kw, amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is True and c.amg_info()["precision"] == S.AMG_PRECISION_SINGLE
        y2 = c.pc_apply(x)
    with _ctx(A2, amg=kw) as f:
        fresh = f.pc_apply(x)
    assert y2.tobytes() == fresh.tobytes(), f"{setup}: the refreshed FP32 copies are {np.abs(y2 - fresh).max():.3e} off a fresh build's"
    assert not np.array_equal(y2, y1)


# ---- 6. the edges of the "no scaling" rule ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cycle,gamma,tail", CYCLES)
def test_an_application_commutes_with_a_power_of_two(cycle, gamma, tail):
    """33x33 `smooth`: pc_apply(2^k x) has the bytes of 2^k pc_apply(x) for k = +-40 -- nothing in the cycle rescales, and
    nothing in it depends on the size of the vector while its entries stay normal floats (the numpy cycle has the property at
    these k: test_mg_precision_varcoef_cpu.test_mixed_cycle_commutes_with_a_power_of_two)."""
    A = F.operator("33x33", "smooth")
    x = F.rhs(A.nrows)
    with _ctx(A, amg=_kw("33x33", precision="single", cycle=cycle, tail=tail)) as c:
        y = c.pc_apply(x)
        for k in SCALE_K:
            s = 2.0 ** k
            ys = c.pc_apply(s * x)
            assert ys.tobytes() == (s * y).tobytes(), f"{cycle} k = {k}: {np.abs(ys / s - y).max():.3e} off the scaled application"


def test_a_subnormal_step_underflows_gradually():
    """33x33 `smooth`, the step hook on level 1 with x, b and xo scaled by 2^-130: every input, product and sum is a
    subnormal float.  The kernels are compiled with FP32 denormals on (the code objects' kernel descriptors carry
    float_denorm_mode_32 = 3, hipcc's default for gfx950: no flush on input or output) and the step holds no fused
    multiply-add and no division, so the rule is IEEE gradual underflow: the bits of numpy float32.  A kernel that flushed
    would return zeros, which the reference is asserted not to be.  On an MI355X the product and the three steps have
    numpy's bits."""
    A = F.operator("33x33", "smooth")
    with _ctx(A, amg=_kw("33x33", precision="single")) as c:
        rp, ci, v, shp = c.amg_level(1)
        n = shp[0]
        s = F32(2.0 ** -130)
        x, xo, b = _vec32(n, 11) * s, _vec32(n, 21) * s, _vec32(n, 31) * s
        for t in (x, xo, b):
            assert t.dtype == F32 and np.all(np.abs(t) < TINY) and np.count_nonzero(t) == n
        dinv = _dinv32(rp, ci, v, shp)
        d = _ordered(rp, ci, v, x, F32)
        got = c.debug_amg_operator(1, "product", x, precision="single")
        assert np.count_nonzero(d) >= n - 2 and np.all(np.abs(d) < 64 * TINY)
        assert got.tobytes() == d.tobytes(), f"the subnormal product: {np.count_nonzero(got != d)} of {n} entries differ, {np.count_nonzero(got)} non-zero"
        for alpha, beta, given in STEPS:
            yo = xo if given else None
            ref = _step32(d, x, dinv, b, alpha, beta, yo)
            assert np.all(np.abs(ref) < TINY) and np.count_nonzero(ref) >= n - 2
            got = c.debug_amg_operator(1, "step", x, b=b, xo=yo, alpha=alpha, beta=beta, precision="single")
            assert got.tobytes() == ref.tobytes(), (f"the subnormal step ({alpha}, {beta}, xo {given}): {np.count_nonzero(got != ref)} of {n} entries "
                                                    f"differ, {np.count_nonzero(got)} non-zero")
