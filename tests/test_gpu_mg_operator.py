"""-spk_mg_operator stencil on the GPU: the levels between level 0 and the coarsest applied from their value arrays alone
(amg_stencil_kernel, spk_k_amg.hip, over csrc/spk_stencil_op_core.hpp).  The hook's product and smoothing step against a
numpy loop in the stated order bit for bit, against the CSR route within the rounding of two orders of the same products,
the `done` gate; one application against the numpy cycles; the fused tail against the launches; the default; solves;
reuse; the refusals on a live context and the runner.

Shapes, hierarchies built with coarse_eq_limit 10:
  65x33     bs 2: level 1 is 33 x 17 nodes, 1122 rows (six workgroups of 192 rows, the last one partial, chunk edges
            inside grid lines), level 2 306 rows
  66x34any  bs 2, even sides;  33x9 semi-coarsening;  12x10any;  4x4any (two levels: no level the option covers)
  five17x9  bs 1: rows of 4, 6 and 9 values, odd value offsets (the peeled head and tail of the 16-byte staging)
  17x9x5    bs 3: level 1 is 9 x 5 x 3 nodes, interior rows with all 27 neighbours (81 values), 405 rows in workgroups of 64:
            a node's three rows fall into two workgroups
  6x4x3any  bs 3"""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest
import scipy.sparse as sp

import saddle_point_petsc_amd as S
from test_gpu_mg_grid import _ctx, _scipy
from test_mg_cycle_cpu import cycle_ref
from test_mg_grid_cpu import five_point
from test_mg_sides_cpu import hierarchy_mats, vcycle_ref

pytestmark = pytest.mark.gpu
SPK_ERR_ARG, SPK_ERR_STATE, SPK_ERR_UNSUPPORTED = -1, -3, -6
U = 2.0 ** -53

# name -> (grid, bs, sides, operator and right-hand side)
SHAPES = {
    "65x33": ((65, 33, 1), 2, "odd", lambda: S.AssembleOperator_Laplace(65, 33)),
    "66x34any": ((66, 34, 1), 2, "any", lambda: S.AssembleOperator_Laplace(66, 34)),
    "33x9": ((33, 9, 1), 2, "odd", lambda: S.AssembleOperator_Laplace(33, 9)),
    "12x10any": ((12, 10, 1), 2, "any", lambda: S.AssembleOperator_Laplace(12, 10)),
    "4x4any": ((4, 4, 1), 2, "any", lambda: S.AssembleOperator_Laplace(4, 4)),
    "five17x9": ((17, 9, 1), 1, "odd", lambda: (five_point(17, 9), None)),
    "17x9x5": ((17, 9, 5), 3, "odd", lambda: S.AssembleOperator_Laplace3D(17, 9, 5)),
    "6x4x3any": ((6, 4, 3), 3, "any", lambda: S.AssembleOperator_Laplace3D(6, 4, 3)),
}
ALL = list(SHAPES)
STEPS = [(0.7, 0.0, False), (0.7, 0.3, False), (0.7, 0.3, True)]   # (alpha, beta, xo given)


@functools.lru_cache(maxsize=None)
def _problem(name):
    return SHAPES[name][3]()


def _kw(name, **kw):
    grid, bs, sides, _ = SHAPES[name]
    return dict(dict(coarsening="grid", grid=grid, sides=sides, block_size=bs, coarse_eq_limit=10, galerkin="stencil", setup="device"), **kw)


def _vec(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


def _ordered_rows(rp, ci, v, x):
    """per row the sum in stored order -- the first product, then one rounded product and one addition per entry -- and
    sum |v| |x| with the number of stored entries"""
    n = len(rp) - 1
    d, mag = np.zeros(n), np.zeros(n)
    for r in range(n):
        s = None
        for p in range(rp[r], rp[r + 1]):
            t = np.float64(v[p]) * np.float64(x[ci[p]])
            s = t if s is None else s + t
        d[r] = s
        mag[r] = np.abs(v[rp[r]:rp[r + 1]] * x[ci[rp[r]:rp[r + 1]]]).sum()
    return d, mag, np.diff(rp)


def _step(d, y, dinv, b, alpha, beta, yo):
    """amg_csr_kernel<1>'s expressions in its order, every operation a numpy ufunc of its own (rounded on its own)"""
    r = y + alpha * (dinv * (b - d))
    if beta != 0.0:
        r = r + beta * (y - (yo if yo is not None else 0.0))
    return r


# ---- 1. the hook: bit for bit, against the CSR route, the done gate ----------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_hook_product_and_step(name):
    """Against numpy: equal bits.  Against the CSR route of the same hook: the product within 2 (n_r + 1) 2^-53 sum |v| |x|
    per row (two orders of the same n_r products; each order is within (n_r + 1) u of the exact sum).  The step puts the
    product through y + alpha (dinv (b - d)) [+ beta (y - yo)]: the two d's differ by at most that bound, which
    alpha |dinv| scales, and each route then rounds at most seven operations whose results are bounded by
    M = |y| + alpha |dinv| (|b| + sum |v| |x|) + beta (|y| + |yo|): 8 u M more between the two."""
    A, _ = _problem(name)
    with _ctx(A, amg=_kw(name, operator="stencil")) as c:
        info = c.amg_info()
        L = info["levels"]
        assert info["operator"] == S.AMG_OPERATOR_STENCIL and info["galerkin"] == S.AMG_GALERKIN_STENCIL
        if name == "65x33":
            assert info["dims"][1] == (33, 17, 1) and info["rows"][1:3] == [1122, 306]
        if name == "17x9x5":
            assert info["dims"][1] == (9, 5, 3)
        if name == "4x4any":
            assert L == 2
        worst = 0.0
        for l in range(1, L - 1):
            rp, ci, v, shape = c.amg_level(l)
            n = shape[0]
            x, xo, b = _vec(n, 10 + l), _vec(n, 20 + l), _vec(n, 30 + l)
            diag = sp.csr_matrix((v, ci, rp), shape=shape).diagonal()
            dinv = 1.0 / diag
            d, mag, nr = _ordered_rows(rp, ci, v, x)
            bound = 2.0 * (nr + 1) * U * mag
            got = c.debug_amg_operator(l, "product", x)
            assert got.tobytes() == d.tobytes(), f"{name} level {l}: the product is not the stated sum"
            csr = c.debug_amg_operator(l, "product", x, stencil=False)
            assert np.all(np.abs(got - csr) <= bound), (name, l, float((np.abs(got - csr) - bound).max()))
            worst = max(worst, float((np.abs(got - csr)[bound > 0] / bound[bound > 0]).max()))
            sentinel = _vec(n, 40 + l)
            for alpha, beta, given in STEPS:
                yo = xo if given else None
                ref = _step(d, x, dinv, b, alpha, beta, yo)
                got = c.debug_amg_operator(l, "step", x, b=b, xo=yo, alpha=alpha, beta=beta)
                assert got.tobytes() == ref.tobytes(), f"{name} level {l}: step ({alpha}, {beta}, xo {given}) is not the stated formula"
                csr = c.debug_amg_operator(l, "step", x, b=b, xo=yo, alpha=alpha, beta=beta, stencil=False)
                M = np.abs(x) + alpha * np.abs(dinv) * (np.abs(b) + mag) + beta * (np.abs(x) + (np.abs(xo) if given else 0.0))
                assert np.all(np.abs(got - csr) <= alpha * np.abs(dinv) * bound + 8.0 * U * M), (name, l, alpha, beta, given)
                kept = c.debug_amg_operator(l, "step", x, b=b, xo=yo, alpha=alpha, beta=beta, done=True, out=sentinel)
                assert kept.tobytes() == sentinel.tobytes(), f"{name} level {l}: the step wrote behind a set done gate"
            kept = c.debug_amg_operator(l, "product", x, done=True, out=sentinel)
            assert kept.tobytes() == sentinel.tobytes(), f"{name} level {l}: the product wrote behind a set done gate"
            assert np.array_equal(c.debug_amg_operator(l, "product", x), d)   # the same bits on a second run
        print(f"{name}: largest |stencil - csr| / bound of a product row {worst:.4f}")
        for l in (0, L - 1, L):
            with pytest.raises(S.SpkError) as e:
                c.debug_amg_operator(l, "product", np.zeros(info["rows"][min(l, L - 1)]))
            assert e.value.code == SPK_ERR_ARG, l


def test_hook_refuses_a_level_without_the_closed_form():
    A, _ = _problem("33x9")
    with _ctx(A, amg=_kw("33x9", galerkin="products")) as c:
        info = c.amg_info()
        x = _vec(info["rows"][1], 1)
        with pytest.raises(S.SpkError) as e:
            c.debug_amg_operator(1, "product", x)
        assert e.value.code == SPK_ERR_STATE
        y = c.debug_amg_operator(1, "product", x, stencil=False)   # the CSR route works on any hierarchy
        rp, ci, v, shape = c.amg_level(1)
        ref = sp.csr_matrix((v, ci, rp), shape=shape) @ x
        assert np.linalg.norm(y - ref) <= 1e-13 * np.linalg.norm(ref)


# ---- 2. one application ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_one_application_matches_numpy(name):
    """1e-12 relative, the bar test_gpu_mg_galerkin.test_one_application_matches_numpy holds the csr route to; both cycles"""
    A, _ = _problem(name)
    x = _vec(A.nrows, 3)
    for cycle, gamma, extra in (("v", 1, dict(tail="launches")), ("w", 2, dict(tail="fused"))):
        with _ctx(A, amg=_kw(name, operator="stencil", cycle=cycle, **extra)) as c:
            info = c.amg_info()
            y, y2 = c.pc_apply(x), c.pc_apply(x)
            mats = hierarchy_mats(c.amg_level, info)
        assert y.tobytes() == y2.tobytes() and info["operator"] == S.AMG_OPERATOR_STENCIL
        ref = vcycle_ref(*mats, info["lambda_max"], x) if gamma == 1 else cycle_ref(*mats, info["lambda_max"], x, 2)
        err = np.linalg.norm(y - ref) / np.linalg.norm(ref)
        print(f"{name} stencil {cycle}: {err:.3e} off numpy (bound 1e-12)")
        assert err <= 1e-12


# ---- 3. the fused tail gives the launches' bits -------------------------------------------------------------------------
@pytest.mark.parametrize("cycle", ["v", "w"])
@pytest.mark.parametrize("name", ["65x33", "66x34any", "17x9x5"])
def test_fused_tail_gives_the_bits_of_the_launches(name, cycle):
    A, _ = _problem(name)
    x = _vec(A.nrows, 7)
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        c.pc_setup(S.PC_JACOBI, amg=_kw(name, operator="stencil", cycle=cycle, tail="launches"))
        assert c.amg_info()["tail_first"] == -1
        ref = c.pc_apply(x)
        c.pc_setup(S.PC_JACOBI, amg=_kw(name, operator="csr", cycle=cycle, tail="launches"))
        assert not np.array_equal(c.pc_apply(x), ref), "the stencil route gave the CSR route's bits: is it running?"
        firsts = set()
        for tr in (50, 306, 1024):
            c.pc_setup(S.PC_JACOBI, amg=_kw(name, operator="stencil", cycle=cycle, tail="fused", tail_rows=tr))
            info = c.amg_info()
            firsts.add(info["tail_first"])
            y = c.pc_apply(x)
            assert y.tobytes() == ref.tobytes(), f"{name} {cycle} tail_rows {tr} (tail_first {info['tail_first']}): {np.abs(y - ref).max():.3e} off the launches"
        assert any(0 < t < c.amg_info()["levels"] - 1 for t in firsts), firsts   # a stencil level ran inside the tail


# ---- 4. the default ----------------------------------------------------------------------------------------------------
def test_csr_is_the_default_byte_for_byte():
    A, _ = _problem("65x33")
    x = _vec(A.nrows, 5)
    kw = _kw("65x33")
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        c.pc_setup(S.PC_JACOBI, amg=kw)
        assert c.amg_info()["operator"] == S.AMG_OPERATOR_CSR == 0
        y = c.pc_apply(x)
        c.pc_setup(S.PC_JACOBI, amg=dict(kw, operator="csr"))
        assert c.amg_info()["operator"] == 0 and c.pc_apply(x).tobytes() == y.tobytes()


# ---- 5. solves ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["65x33", "66x34any", "17x9x5"])
def test_k_equals_a_solves_like_the_csr_route(name):
    A, f = _problem(name)
    Asp = _scipy(A)
    its = {}
    for route in ("stencil", "csr"):
        with _ctx(A, amg=_kw(name, operator=route)) as c:
            assert c.amg_info()["operator"] == (route == "stencil")
            for ksp in ("fgmres", "pipecg"):
                x, info = getattr(c, ksp)(f, rtol=1e-8, max_it=200)
                res = np.linalg.norm(f - Asp @ x) / np.linalg.norm(f)
                print(f"{name} {route} {ksp}: {info['its']} iterations, true residual {res:.2e}")
                assert info["reason"] == 2 and res <= 2e-8
                its[route, ksp] = info["its"]
    for ksp in ("fgmres", "pipecg"):
        assert abs(its["stencil", ksp] - its["csr", ksp]) <= 1, its


def test_saddle_system_with_the_exact_schur_complement():
    A, f = _problem("65x33")
    B, g = S.AssembleOperator_Constraints(65, 33)
    rhs = np.concatenate([f, g])
    Bsp = sp.csr_matrix((B.val, B.colidx, B.rowptr), shape=(B.nrows, A.nrows))
    K = sp.bmat([[_scipy(A), Bsp.T], [Bsp, None]], format="csr")
    its = {}
    for route in ("stencil", "csr"):
        with _ctx(A, B, S.PC_SCHUR, S.SCHUR_FULL, amg=_kw("65x33", operator=route), schur_pre="full") as c:
            x, info = c.fgmres(rhs, rtol=1e-8, max_it=200)
        res = np.linalg.norm(rhs - K @ x) / np.linalg.norm(rhs)
        print(f"saddle 65x33 FULL + exact S + mg operator {route}: {info['its']} iterations, true residual {res:.2e}")
        assert info["reason"] == 2 and res <= 2e-8
        its[route] = info["its"]
    assert abs(its["stencil"] - its["csr"]) <= 1, its


# ---- 6. reuse ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setup", ["device", "host"])
def test_the_option_alone_refreshes_and_a_refresh_reaches_the_kernels(setup):
    A, _ = _problem("65x33")
    x = _vec(A.nrows, 9)
    kw = _kw("65x33", setup=setup)
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        c.pc_setup(S.PC_JACOBI, amg=dict(kw, operator="csr"), amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is False and c.amg_info()["operator"] == 0
        y_csr = c.pc_apply(x)
        levels = [tuple(a.tobytes() for a in c.amg_level(l)[:3]) for l in range(1, c.amg_info()["levels"])]
        c.pc_setup(S.PC_JACOBI, amg=dict(kw, operator="stencil"), amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is True and c.amg_info()["operator"] == S.AMG_OPERATOR_STENCIL
        assert [tuple(a.tobytes() for a in c.amg_level(l)[:3]) for l in range(1, c.amg_info()["levels"])] == levels
        y_st = c.pc_apply(x)
        assert not np.array_equal(y_st, y_csr) and np.linalg.norm(y_st - y_csr) <= 1e-12 * np.linalg.norm(y_csr)
        # new values: A scaled by a factor that is no power of two
        A3 = S.CSR(A.rowptr.copy(), A.colidx.copy(), A.val * 3.0, A.nrows)
        c.set_block(S.BLOCK_A00, A3)
        c.pc_setup(S.PC_JACOBI, amg=dict(kw, operator="stencil"), amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is True and c.amg_info()["operator"] == S.AMG_OPERATOR_STENCIL
        info = c.amg_info()
        y3 = c.pc_apply(x)
        ref = vcycle_ref(*hierarchy_mats(c.amg_level, info), info["lambda_max"], x)
    err = np.linalg.norm(y3 - ref) / np.linalg.norm(ref)
    print(f"{setup}: after the refresh on 3 A, {err:.3e} off numpy on the new values (bound 1e-12)")
    assert err <= 1e-12 and np.linalg.norm(y3 - y_st / 3.0) <= 1e-10 * np.linalg.norm(y3)


# ---- 7. the refusals on a live context, and the runner -----------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    A, f = _problem("33x9")
    Asp = _scipy(A)
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        c.pc_setup(S.PC_JACOBI, amg=_kw("33x9"))
        x = _vec(A.nrows, 2)
        y = c.pc_apply(x)
        for amg, words in ((_kw("33x9", operator="stencil", galerkin="products"), "-spk_mg_galerkin stencil"),
                           (dict(operator="stencil"), "-pc_type mg"), (_kw("33x9", operator=5), "op 5")):
            with pytest.raises(S.SpkError) as e:
                c.pc_setup(S.PC_JACOBI, amg=amg)
            assert e.value.code == (SPK_ERR_ARG if words == "op 5" else SPK_ERR_UNSUPPORTED) and words in str(e.value), str(e.value)
        c.pc_setup(S.PC_JACOBI, amg=_kw("33x9"))   # the options the context held were not touched
        assert c.pc_apply(x).tobytes() == y.tobytes()
        c.pc_setup(S.PC_JACOBI, amg=_kw("33x9", operator="stencil"))
        u, r = c.fgmres(f, rtol=1e-8, max_it=200)
    assert r["reason"] == 2 and np.linalg.norm(f - Asp @ u) <= 2e-8 * np.linalg.norm(f)


def test_runner_takes_the_option_and_ksp_view_names_the_route():
    exe = os.path.join(os.path.dirname(S.LIB_PATH), "saddle_point_run")
    base = [exe, "-da_grid_x", "65", "-da_grid_y", "33", "-ksp_rtol", "1e-8", "-ksp_converged_reason", "-no_vtk", "-saddle", "0",
            "-ksp_type", "fgmres", "-pc_type", "mg", "-spk_mg_galerkin", "stencil", "-ksp_view"]
    out = subprocess.run(base + ["-spk_mg_operator", "stencil"], capture_output=True, text=True, timeout=120, cwd=tempfile.mkdtemp())
    assert out.returncode == 0, out.stdout + out.stderr
    assert "converged due to CONVERGED_RTOL" in out.stdout, out.stdout
    assert "level operators: stencil (-spk_mg_operator stencil): levels 1.." in out.stdout and "value arrays" in out.stdout, out.stdout
    out = subprocess.run(base[:-3] + ["-spk_mg_operator", "stencil"], capture_output=True, text=True, timeout=120, cwd=tempfile.mkdtemp())
    assert out.returncode != 0 and "-spk_mg_galerkin stencil" in out.stdout + out.stderr, out.stdout + out.stderr
