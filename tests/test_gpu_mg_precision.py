"""-spk_mg_precision single on the GPU (include/spk.h, SPK_AMG_PRECISION_SINGLE): the levels >= 1 of the all-stencil mg route
in FP32 (spk_k_amg.hip: amg_stencil_f32_kernel, the float transfers, the float dense product, amg_stencil_tail_f32_kernel).
The FP32 hooks against numpy float32 in the stated order bit for bit, the `done` gate; one application against the numpy
cycle with FP32 levels (test_mg_precision_cpu.vcycle_ref_mixed) and against the context's own FP64 route; the fused tail
against the launches; the default against bytes recorded from the commit before the option; solves; reuse; the runner.

Shapes: those of test_gpu_mg_operator (hierarchies built with coarse_eq_limit 10) -- bs 1, 2 and 3, both side rules, partial
last workgroups; 17x9x5's level 1 (405 rows of up to 81 floats in workgroups of 64) begins and ends its workgroups' value
ranges at every residue mod 4 (tests/test_mg_precision_cpu.py prints them); 4x4any has two levels, so only the coarsest,
its dense inverse, is FP32."""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest
import scipy.sparse as sp

import saddle_point_petsc_amd as S
from test_gpu_mg_grid import _ctx, _scipy
from test_gpu_mg_operator import SHAPES, STEPS, _problem, _vec
from test_mg_precision_cpu import GPU_SHAPES, cycle_difference, vcycle_ref_mixed
from test_mg_sides_cpu import hierarchy_mats

pytestmark = pytest.mark.gpu
SPK_ERR_ARG, SPK_ERR_STATE, SPK_ERR_UNSUPPORTED = -1, -3, -6
F32 = np.float32
ALL = GPU_SHAPES
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mg_precision_parent_65x33.npz")


def _kw(name, **kw):
    """the all-stencil route on the device set-up"""
    grid, bs, sides, _ = SHAPES[name]
    return dict(dict(coarsening="grid", grid=grid, sides=sides, block_size=bs, coarse_eq_limit=10, galerkin="stencil",
                     operator="stencil", setup="device"), **kw)


def _vec32(n, seed):
    return _vec(n, seed).astype(F32)


def _ordered(rp, ci, v, x, dt):
    """per row of a CSR matrix the sum in stored order in the type dt: the values rounded to dt once, the first product,
    then one product and one addition per entry, each a numpy operation of its own"""
    rp, ci, v = np.asarray(rp), np.asarray(ci), np.asarray(v).astype(dt)
    assert x.dtype == dt
    n, ln = len(rp) - 1, np.diff(rp)
    out = np.zeros(n, dt)
    for j in range(int(ln.max())):
        m = ln > j
        p = rp[:-1][m] + j
        t = v[p] * x[ci[p]]
        out[m] = t if j == 0 else out[m] + t
    assert out.dtype == dt
    return out


def _step32(d, y, dinv, b, alpha, beta, yo):
    """the step's expressions in their order on float32, every operation a numpy ufunc of its own"""
    alpha, beta = F32(alpha), F32(beta)
    r = y + alpha * (dinv * (b - d))
    if beta != 0.0:
        r = r + beta * (y - (yo if yo is not None else F32(0.0)))
    assert r.dtype == F32
    return r


@functools.lru_cache(maxsize=None)
def _bar(gamma=1):
    """four times the largest relative difference of one application between the two numpy cycles (gamma = 1: V, 2: W) over
    the shapes"""
    worst = max(cycle_difference(name, gamma) for name in ALL)
    return 4.0 * worst, worst


# ---- 1. the hooks: bit for bit against numpy float32, the done gate ------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_hooks_are_numpy_float32_bit_for_bit(name):
    A, _ = _problem(name)
    with _ctx(A, amg=_kw(name, precision="single")) as c:
        info = c.amg_info()
        L = info["levels"]
        assert info["precision"] == S.AMG_PRECISION_SINGLE and info["operator"] == S.AMG_OPERATOR_STENCIL
        if name == "4x4any":
            assert L == 2
        if name == "17x9x5":
            assert info["dims"][1] == (9, 5, 3)
        for l in range(1, L - 1):   # the operator: product and step
            rp, ci, v, shape = c.amg_level(l)
            n = shape[0]
            x, xo, b = _vec32(n, 10 + l), _vec32(n, 20 + l), _vec32(n, 30 + l)
            dinv = (1.0 / sp.csr_matrix((v, ci, rp), shape=shape).diagonal()).astype(F32)   # the FP64 D^-1, rounded
            d = _ordered(rp, ci, v, x, F32)
            sentinel = _vec32(n, 40 + l)
            got = c.debug_amg_operator(l, "product", x, precision="single")
            assert got.dtype == F32 and got.tobytes() == d.tobytes(), f"{name} level {l}: the product is not the stated float32 sum"
            for alpha, beta, given in STEPS:
                yo = xo if given else None
                ref = _step32(d, x, dinv, b, alpha, beta, yo)
                got = c.debug_amg_operator(l, "step", x, b=b, xo=yo, alpha=alpha, beta=beta, precision="single")
                assert got.tobytes() == ref.tobytes(), f"{name} level {l}: step ({alpha}, {beta}, xo {given}) is not the stated formula"
                kept = c.debug_amg_operator(l, "step", x, b=b, xo=yo, alpha=alpha, beta=beta, done=True, out=sentinel, precision="single")
                assert kept.tobytes() == sentinel.tobytes(), f"{name} level {l}: the step wrote behind a set done gate"
            kept = c.debug_amg_operator(l, "product", x, done=True, out=sentinel, precision="single")
            assert kept.tobytes() == sentinel.tobytes(), f"{name} level {l}: the product wrote behind a set done gate"
            assert c.debug_amg_operator(l, "product", x, precision="single").tobytes() == d.tobytes()   # a second run
        for l in range(L - 1):   # the transfers; level 0: the two boundary forms
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
            assert got.dtype == ti and got.tobytes() == ref.tobytes(), f"{name} level {l}: y + P e is not the stated sum"
            assert c.debug_amg_transfer(l, "prolong", e, y, precision="single").tobytes() == ref.tobytes()
            b, t = _vec(nf, 70 + l).astype(ti), _vec(nf, 80 + l).astype(ti)
            ref = _ordered(R.indptr, R.indices, R.data, b - t, ti).astype(F32)   # (level 0: one rounding on the store)
            got = c.debug_amg_transfer(l, "restrict", b, t, precision="single")
            assert got.dtype == F32 and got.tobytes() == ref.tobytes(), f"{name} level {l}: R (b - t) is not the stated sum"
            assert c.debug_amg_transfer(l, "restrict", b, t, precision="single").tobytes() == ref.tobytes()
        for l in (0, L - 1, L):
            with pytest.raises(S.SpkError) as e:
                c.debug_amg_operator(l, "product", np.zeros(info["rows"][min(l, L - 1)], F32), precision="single")
            assert e.value.code == SPK_ERR_ARG, l


def test_hooks_need_a_single_hierarchy():
    A, _ = _problem("33x9")
    with _ctx(A, amg=_kw("33x9")) as c:
        info = c.amg_info()
        assert info["precision"] == S.AMG_PRECISION_DOUBLE
        with pytest.raises(S.SpkError) as e:
            c.debug_amg_operator(1, "product", _vec32(info["rows"][1], 1), precision="single")
        assert e.value.code == SPK_ERR_STATE and "-spk_mg_precision single" in str(e.value)
        with pytest.raises(S.SpkError) as e:
            c.debug_amg_transfer(1, "restrict", _vec32(info["rows"][1], 1), _vec32(info["rows"][1], 2), precision="single")
        assert e.value.code == SPK_ERR_STATE


# ---- 2. one application ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_one_application(name):
    """|| y - ref || / || y || against the numpy cycle with FP32 levels and against the same context's FP64 route.
    The bar is an FP32-level one, not the 1e-12 of the FP64 routes: level 0 sums in another order than numpy (differences
    of a few 2^-53), which can flip the one rounding of an entry of the restricted residual -- 2^-24 relative in that entry,
    carried through the FP32 levels -- and the FP64 route differs from the FP32 one by the roundings of the FP32 levels
    themselves.  Their size is measured on the CPU, where it depends on the reference alone and not on the code under test:
    || vcycle_ref_mixed - cycle_ref || / || cycle_ref || on the same hierarchies and vectors, under V 6.7e-9 (4x4any) to
    4.6e-7 (66x34any); the W-cycle visits the FP32 levels more often and has its own figures (printed).  The bar of a cycle is
    four times the largest of its figures over the shapes (V: 1.8e-6, W: 1.4e-5, both from 66x34any): against the FP64 route the device differs as the numpy
    cycles do, and against the mixed numpy cycle by flipped roundings alone, far less; the factor covers the other summation
    order on level 0.  Against the FP64 route the difference is also above 1e-10: the FP32 levels ran."""
    A, _ = _problem(name)
    x = _vec(A.nrows, 3)
    for cycle, gamma, extra in (("v", 1, dict(tail="launches")), ("w", 2, dict(tail="fused"))):
        bar, worst = _bar(gamma)
        with S.Context(0) as c:
            c.set_block(S.BLOCK_A00, A)
            c.pc_setup(S.PC_JACOBI, amg=_kw(name, precision="single", cycle=cycle, **extra))
            info = c.amg_info()
            assert info["precision"] == S.AMG_PRECISION_SINGLE
            y, y2 = c.pc_apply(x), c.pc_apply(x)
            mats = hierarchy_mats(c.amg_level, info)
            c.pc_setup(S.PC_JACOBI, amg=_kw(name, precision="double", cycle=cycle, **extra))
            assert c.amg_info()["precision"] == S.AMG_PRECISION_DOUBLE
            yd = c.pc_apply(x)
        assert y.tobytes() == y2.tobytes()
        to_double = np.linalg.norm(y - yd) / np.linalg.norm(y)
        print(f"{name} {cycle}: {to_double:.3e} off the double route (bar {bar:.3e}; on the CPU {cycle_difference(name, gamma):.3e}, largest {worst:.3e})")
        assert 1e-10 < to_double <= bar
        ref = vcycle_ref_mixed(*mats, info["lambda_max"], x, gamma=gamma)
        err = np.linalg.norm(y - ref) / np.linalg.norm(y)
        print(f"{name} {cycle}: {err:.3e} off the numpy cycle with FP32 levels (bar {bar:.3e})")
        assert err <= bar


# ---- 3. the fused tail gives the launches' bits -------------------------------------------------------------------------
@pytest.mark.parametrize("cycle", ["v", "w"])
@pytest.mark.parametrize("name", ["65x33", "66x34any", "17x9x5"])
def test_fused_tail_gives_the_bits_of_the_launches(name, cycle):
    A, _ = _problem(name)
    x = _vec(A.nrows, 7)
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        c.pc_setup(S.PC_JACOBI, amg=_kw(name, precision="single", cycle=cycle, tail="launches"))
        assert c.amg_info()["tail_first"] == -1 and c.amg_info()["precision"] == 1
        ref = c.pc_apply(x)
        firsts = set()
        for tr in (50, 306, 1024):
            c.pc_setup(S.PC_JACOBI, amg=_kw(name, precision="single", cycle=cycle, tail="fused", tail_rows=tr))
            info = c.amg_info()
            firsts.add(info["tail_first"])
            y = c.pc_apply(x)
            assert y.tobytes() == ref.tobytes(), f"{name} {cycle} tail_rows {tr} (tail_first {info['tail_first']}): {np.abs(y - ref).max():.3e} off the launches"
        assert any(0 < t < c.amg_info()["levels"] - 1 for t in firsts), firsts   # an FP32 stencil level ran inside the tail


# ---- 4. the default ----------------------------------------------------------------------------------------------------
def test_double_is_the_default_and_gives_the_bytes_from_before_the_option():
    """tests/golden/mg_precision_parent_65x33.npz: one application on 65x33 (x = _vec(n, 5)) by the commit before the option,
    on the csr and on the stencil operator route, recorded on an MI355X"""
    A, _ = _problem("65x33")
    x = _vec(A.nrows, 5)
    gold = np.load(GOLDEN)
    assert gold["x"].tobytes() == x.tobytes()
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        for route in ("csr", "stencil"):
            kw = _kw("65x33", operator=route)
            c.pc_setup(S.PC_JACOBI, amg=kw)
            assert c.amg_info()["precision"] == S.AMG_PRECISION_DOUBLE == 0
            y = c.pc_apply(x)
            c.pc_setup(S.PC_JACOBI, amg=dict(kw, precision="double"))
            assert c.amg_info()["precision"] == 0 and c.pc_apply(x).tobytes() == y.tobytes()
            assert y.tobytes() == gold[route].tobytes(), f"{route}: {np.abs(y - gold[route]).max():.3e} off the recorded bytes"


# ---- 5. solves ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["65x33", "66x34any", "17x9x5"])
def test_k_equals_a_solves_like_the_double_route(name):
    A, f = _problem(name)
    Asp = _scipy(A)
    its = {}
    for prec in ("single", "double"):
        with _ctx(A, amg=_kw(name, precision=prec)) as c:
            assert c.amg_info()["precision"] == (prec == "single")
            x, info = c.fgmres(f, rtol=1e-8, max_it=200)
            res = np.linalg.norm(f - Asp @ x) / np.linalg.norm(f)
            print(f"{name} {prec} fgmres: {info['its']} iterations, true residual {res:.2e}")
            assert info["reason"] == 2 and res <= 2e-8
            its[prec] = info["its"]
    assert abs(its["single"] - its["double"]) <= 1, its


def test_saddle_system_with_the_exact_schur_complement():
    A, f = _problem("65x33")
    B, g = S.AssembleOperator_Constraints(65, 33)
    rhs = np.concatenate([f, g])
    Bsp = sp.csr_matrix((B.val, B.colidx, B.rowptr), shape=(B.nrows, A.nrows))
    K = sp.bmat([[_scipy(A), Bsp.T], [Bsp, None]], format="csr")
    its = {}
    for prec in ("single", "double"):
        with _ctx(A, B, S.PC_SCHUR, S.SCHUR_FULL, amg=_kw("65x33", precision=prec), schur_pre="full") as c:
            x, info = c.fgmres(rhs, rtol=1e-8, max_it=200)
        res = np.linalg.norm(rhs - K @ x) / np.linalg.norm(rhs)
        print(f"saddle 65x33 FULL + exact S + mg precision {prec}: {info['its']} iterations, true residual {res:.2e}")
        assert info["reason"] == 2 and res <= 2e-8
        its[prec] = info["its"]
    assert abs(its["single"] - its["double"]) <= 1, its


@pytest.mark.parametrize("ksp", ["pipecg", "pipecgrr"])
def test_pipelined_cg_is_refused_and_fgmres_then_solves(ksp):
    A, f = _problem("65x33")
    Asp = _scipy(A)
    with _ctx(A, amg=_kw("65x33", precision="single")) as c:
        with pytest.raises(S.SpkError) as e:
            getattr(c, ksp)(f, rtol=1e-8, max_it=200)
        assert e.value.code == SPK_ERR_UNSUPPORTED and "-ksp_type fgmres" in str(e.value) and "-spk_mg_precision" in str(e.value), str(e.value)
        x, info = c.fgmres(f, rtol=1e-8, max_it=200)
    assert info["reason"] == 2 and np.linalg.norm(f - Asp @ x) <= 2e-8 * np.linalg.norm(f)


# ---- 6. reuse ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setup", ["device", "host"])
def test_the_option_alone_refreshes_and_a_refresh_rounds_again(setup):
    A, _ = _problem("65x33")
    x = _vec(A.nrows, 9)
    kw = _kw("65x33", setup=setup)
    kappa = 1.0 + 0.5 * np.sin(0.37 * np.arange(64 * 32))   # a coefficient per element: new values on the same pattern
    A2 = S.AssembleOperator_Laplace(65, 33, kappa=kappa)[0]
    assert np.array_equal(A2.colidx, A.colidx) and not np.array_equal(A2.val, A.val)
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        c.pc_setup(S.PC_JACOBI, amg=dict(kw, precision="double"), amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is False and c.amg_info()["precision"] == 0
        yd = c.pc_apply(x)
        levels = [tuple(a.tobytes() for a in c.amg_level(l)[:3]) for l in range(1, c.amg_info()["levels"])]
        c.pc_setup(S.PC_JACOBI, amg=dict(kw, precision="single"), amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is True and c.amg_info()["precision"] == S.AMG_PRECISION_SINGLE
        assert [tuple(a.tobytes() for a in c.amg_level(l)[:3]) for l in range(1, c.amg_info()["levels"])] == levels   # the hierarchy stays FP64
        ys = c.pc_apply(x)
        assert not np.array_equal(ys, yd) and np.linalg.norm(ys - yd) <= _bar(1)[0] * np.linalg.norm(yd)
        c.pc_setup(S.PC_JACOBI, amg=dict(kw, precision="double"), amg_reuse=True)   # and back
        assert c.amg_reuse_info()["refreshed"] is True and c.pc_apply(x).tobytes() == yd.tobytes()
        c.pc_setup(S.PC_JACOBI, amg=dict(kw, precision="single"), amg_reuse=True)
        assert c.pc_apply(x).tobytes() == ys.tobytes()
        c.set_block(S.BLOCK_A00, A2)   # new values
        c.pc_setup(S.PC_JACOBI, amg=dict(kw, precision="single"), amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is True and c.amg_info()["precision"] == 1
        y2 = c.pc_apply(x)
    with _ctx(A2, amg=dict(kw, precision="single")) as f:   # a fresh build on the new values
        fresh = f.pc_apply(x)
    assert y2.tobytes() == fresh.tobytes(), f"{setup}: the refreshed FP32 copies are {np.abs(y2 - fresh).max():.3e} off a fresh build's"
    assert not np.array_equal(y2, ys)


# ---- 7. the refusals on a live context, and the runner -----------------------------------------------------------------
def test_refusals_name_the_missing_option_and_leave_the_context_usable():
    A, f = _problem("33x9")
    Asp = _scipy(A)
    grid, bs, sides, _ = SHAPES["33x9"]
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        c.pc_setup(S.PC_JACOBI, amg=_kw("33x9"))
        x = _vec(A.nrows, 2)
        y = c.pc_apply(x)
        for amg, words in ((dict(precision="single", setup="device"), "-pc_type mg"),
                           (_kw("33x9", precision="single", galerkin="products", operator="csr"), "-spk_mg_galerkin stencil"),
                           (_kw("33x9", precision="single", operator="csr"), "-spk_mg_operator stencil"),
                           (_kw("33x9", precision="single", transfer="stored"), "-spk_mg_transfer matrixfree"),
                           (_kw("33x9", precision=5), "precision 5")):
            with pytest.raises(S.SpkError) as e:
                c.pc_setup(S.PC_JACOBI, amg=amg)
            assert e.value.code == (SPK_ERR_ARG if words == "precision 5" else SPK_ERR_UNSUPPORTED) and words in str(e.value), str(e.value)
            if words != "precision 5":
                assert "-spk_mg_precision" in str(e.value), str(e.value)
        c.pc_setup(S.PC_JACOBI, amg=_kw("33x9"))   # the options the context held were not touched
        assert c.pc_apply(x).tobytes() == y.tobytes()
        c.pc_setup(S.PC_JACOBI, amg=_kw("33x9", precision="single"))
        u, r = c.fgmres(f, rtol=1e-8, max_it=200)
    assert r["reason"] == 2 and np.linalg.norm(f - Asp @ u) <= 2e-8 * np.linalg.norm(f)


def test_runner_takes_the_option_and_ksp_view_names_the_route():
    exe = os.path.join(os.path.dirname(S.LIB_PATH), "saddle_point_run")
    base = [exe, "-da_grid_x", "65", "-da_grid_y", "33", "-ksp_rtol", "1e-8", "-ksp_converged_reason", "-no_vtk", "-saddle", "0",
            "-ksp_type", "fgmres", "-pc_type", "mg", "-spk_mg_galerkin", "stencil", "-spk_mg_operator", "stencil", "-ksp_view"]
    out = subprocess.run(base + ["-spk_mg_precision", "single"], capture_output=True, text=True, timeout=120, cwd=tempfile.mkdtemp())
    assert out.returncode == 0, out.stdout + out.stderr
    assert "converged due to CONVERGED_RTOL" in out.stdout, out.stdout
    assert "precision: single (-spk_mg_precision single): levels 1.." in out.stdout and "FP32" in out.stdout, out.stdout
    out = subprocess.run(base[:-3] + ["-spk_mg_precision", "single"], capture_output=True, text=True, timeout=120, cwd=tempfile.mkdtemp())
    assert out.returncode != 0 and "-spk_mg_operator stencil" in out.stdout + out.stderr, out.stdout + out.stderr
