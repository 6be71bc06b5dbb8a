"""The W-cycle and the fused coarse tail on the device (-spk_mg_cycle w, -spk_mg_tail fused, -spk_mg_tail_rows): the tail
kernel -- one workgroup that interprets the coarse levels' steps behind barriers -- against the launches it replaces, bit
for bit; both cycles against the numpy restatement (test_mg_cycle_cpu.cycle_ref); the default untouched; the descriptor
after a refresh; inside the solvers; the symmetry of the W-cycle.  pc_apply on K = A is the probe.

Shapes, the smallest that reach every edge of the kernel's loops (128 CSR rows or 16 dense rows per sweep):
  a  mg 33 x 33, bs 2: rows 2178, 578, 162, 50 -- row loops that wrap with a ragged last sweep, and less than one sweep
  b  the same with coarse_eq_limit 200: a dense coarsest level of 162 rows, ragged over the lanes and over the 16 waves
  c  mg 12 x 10 with sides any: rows 240, 84, 32 -- the even-side flags inside the tail
  d  the 3-D generator at 9^3: rows 2187, 375, 81, bs 3, the z direction halves
  e  a with stored transfers (the CSR kernels on P and R)
  f  gamg at 64^2
tail_rows takes the size of level 1 (everything below level 0 fused), of level 2, of the coarsest level (it alone), and 1
(no tail: the launches run)."""
import functools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import scipy.sparse as sp

import saddle_point_petsc_amd as S
from test_amg_cpu import hierarchy_mats
from test_mg_cycle_cpu import cycle_ref

pytestmark = pytest.mark.gpu

# name -> (operator, multigrid options, rows expected or None)
HIER = {
    "a": (lambda: S.AssembleOperator_Laplace(33, 33)[0], dict(coarsening="grid", grid=(33, 33)), [2178, 578, 162, 50]),
    "b": (lambda: S.AssembleOperator_Laplace(33, 33)[0], dict(coarsening="grid", grid=(33, 33), coarse_eq_limit=200), [2178, 578, 162]),
    "c": (lambda: S.AssembleOperator_Laplace(12, 10)[0], dict(coarsening="grid", grid=(12, 10), sides="any"), [240, 84, 32]),
    "d": (lambda: S.AssembleOperator_Laplace3D(9, 9, 9)[0], dict(coarsening="grid", grid=(9, 9, 9)), [2187, 375, 81]),
    "e": (lambda: S.AssembleOperator_Laplace(33, 33)[0], dict(coarsening="grid", grid=(33, 33), transfer="stored"), [2178, 578, 162, 50]),
    "f": (lambda: S.AssembleOperator_Laplace(64)[0], {}, None),
}
SMOOTHERS = {"cheb1": dict(smooth_its=1), "cheb2": dict(smooth_its=2), "cheb3": dict(smooth_its=3),
             "rich2": dict(smoother="richardson", smooth_its=2, richardson_scale=0.6)}


@functools.lru_cache(maxsize=None)
def _operator(name):
    return HIER[name][0]()


def _x(n, seed=7):
    return np.random.default_rng(seed).standard_normal(n)


def _setup(c, name, **kw):
    c.pc_setup(S.PC_JACOBI, amg=dict(HIER[name][1], **kw))
    return c.amg_info()


def _tail_rows(rows):
    return sorted({rows[1], rows[min(2, len(rows) - 1)], rows[-1], 1}, reverse=True)


def _expected_first(rows, tr):
    t = len(rows)
    while t > 1 and rows[t - 1] <= tr:
        t -= 1
    return t if t < len(rows) else -1


# ---- 1. the fused tail gives the bits of the launches ----------------------------------------------------------------
@pytest.mark.parametrize("cycle", ["v", "w"])
@pytest.mark.parametrize("smoother", list(SMOOTHERS))
@pytest.mark.parametrize("name", list(HIER))
def test_fused_tail_gives_the_bits_of_the_launches(name, smoother, cycle):
    A = _operator(name)
    x = _x(A.nrows)
    sm = SMOOTHERS[smoother]
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        info = _setup(c, name, cycle=cycle, tail="launches", **sm)
        rows, L = info["rows"], info["levels"]
        if HIER[name][2] is not None:
            assert rows == HIER[name][2]
        assert L >= 3 and (info["tail_first"], info["tail_launches"]) == (-1, 0)
        ref = c.pc_apply(x)
        assert np.all(np.isfinite(ref)) and np.any(ref != 0.0)
        for tr in _tail_rows(rows):
            info = _setup(c, name, cycle=cycle, tail="fused", tail_rows=tr, **sm)
            t = _expected_first(rows, tr)
            assert info["tail_first"] == t and info["cycle"] == (cycle == "w"), (tr, info["tail_first"], t)
            want = 0 if t < 0 else 1 if cycle == "v" else 2 ** (t - 1) if t < L - 1 else 2 ** (L - 2)
            assert info["tail_launches"] == want
            y = c.pc_apply(x)
            y2 = c.pc_apply(x)
            assert np.array_equal(y, ref), f"{name} {smoother} {cycle} tail_rows {tr}: {np.abs(y - ref).max():.3e} off the launches"
            assert np.array_equal(y2, y)


# ---- 2. against numpy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HIER))
def test_fused_cycles_match_numpy(name):
    """1e-12 relative: the V-cycle's tolerance in test_gpu_amg.py"""
    A = _operator(name)
    x = _x(A.nrows, 3)
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        for cycle, gamma in (("v", 1), ("w", 2)):
            info = _setup(c, name, cycle=cycle, tail="fused", tail_rows=A.nrows)   # every level below level 0
            assert info["tail_first"] == 1
            y = c.pc_apply(x)
            ref = cycle_ref(*hierarchy_mats(c.amg_level, info), info["lambda_max"], x, gamma)
            err = np.linalg.norm(y - ref) / np.linalg.norm(ref)
            print(f"{name} fused {cycle}: {err:.3e} off numpy (bound 1e-12)")
            assert err <= 1e-12


# ---- 3. the default is the V-cycle of launches ------------------------------------------------------------------------
def test_default_is_unchanged():
    A = _operator("a")
    x = _x(A.nrows)
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        info = _setup(c, "a")
        assert (info["cycle"], info["tail_first"], info["tail_launches"]) == (0, -1, 0)
        y = c.pc_apply(x)
        info = _setup(c, "a", cycle="v", tail="launches")
        assert (info["cycle"], info["tail_first"]) == (0, -1)
        assert np.array_equal(c.pc_apply(x), y)
        info = _setup(c, "a", cycle="w")
        assert info["cycle"] == 1 and info["tail_first"] >= 1 and info["tail_launches"] >= 1
        assert not np.array_equal(c.pc_apply(x), y)


# ---- 4. the refresh rewrites the descriptor -----------------------------------------------------------------------------
@pytest.mark.parametrize("cycle", ["v", "w"])
@pytest.mark.parametrize("name,n", [("a", 33), ("f", 64)])
def test_refresh_rewrites_the_descriptor(name, n, cycle):
    """new values through a kept hierarchy: a stale descriptor (pointers, alpha / beta, the coarse inverse) would leave the
    fused tail on the old ones while the launches move on"""
    kappa = np.random.default_rng(11).uniform(0.5, 2.0, (n - 1) * (n - 1))
    x = _x(2 * n * n)
    got = {}
    for tail in ("fused", "launches"):
        amg = dict(HIER[name][1], setup="device", cycle=cycle, tail=tail, tail_rows=x.size)
        with S.Context(0) as c:
            c.set_block_laplace(n, n)
            c.pc_setup(S.PC_JACOBI, amg=amg, amg_reuse=True)
            assert c.amg_reuse_info()["refreshed"] is False
            before = c.pc_apply(x)
            c.set_block_laplace(n, n, kappa=kappa)
            c.pc_setup(S.PC_JACOBI, amg=amg, amg_reuse=True)
            assert c.amg_reuse_info()["refreshed"] is True
            info = c.amg_info()
            assert info["tail_first"] == (1 if tail == "fused" else -1)
            got[tail] = (before, c.pc_apply(x))
            if tail == "launches":   # the three options alone do not ask for a new hierarchy: the other route, refreshed
                c.pc_setup(S.PC_JACOBI, amg=dict(amg, tail="fused", tail_rows=info["rows"][-1]), amg_reuse=True)
                assert c.amg_reuse_info()["refreshed"] is True and c.amg_info()["tail_first"] == info["levels"] - 1
                assert np.array_equal(c.pc_apply(x), got[tail][1])
    assert np.array_equal(got["fused"][0], got["launches"][0])
    assert np.array_equal(got["fused"][1], got["launches"][1])
    assert not np.array_equal(got["fused"][1], got["fused"][0])


# ---- 5. inside the solvers ----------------------------------------------------------------------------------------------
def _scipy(A):
    return sp.csr_matrix((A.val, A.colidx, A.rowptr), shape=(A.nrows, A.nrows))


def test_fgmres_takes_the_fused_tail_as_the_launches():
    """the same iterations and the same solution bits, to convergence and truncated after three iterations (every launch
    behind the last one finds the `done` gate set)"""
    A, f = S.AssembleOperator_Laplace(65, 65)
    got = {}
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        for tail in ("launches", "fused"):
            c.pc_setup(S.PC_JACOBI, amg=dict(coarsening="grid", grid=(65, 65), cycle="v", tail=tail, tail_rows=A.nrows))
            info = c.amg_info()
            assert info["levels"] >= 5 and info["tail_first"] == (1 if tail == "fused" else -1)
            got[tail] = [c.fgmres(f, rtol=1e-8, restart=30, max_it=m) for m in (200, 3)]
    for (xl, il), (xf, jf) in zip(got["launches"], got["fused"]):
        assert il["its"] == jf["its"] and il["reason"] == jf["reason"] and np.array_equal(xl, xf)
    assert got["fused"][0][1]["reason"] == 2 and got["fused"][1][1]["its"] == 3
    res = np.linalg.norm(f - _scipy(A) @ got["fused"][0][0]) / np.linalg.norm(f)
    assert res <= 2e-8


def test_pipecg_with_the_w_cycle():
    A, f = S.AssembleOperator_Laplace(64)
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        c.pc_setup(S.PC_JACOBI, amg=dict(cycle="w"))
        assert c.amg_info()["tail_first"] >= 1
        x, info = c.pipecg(f, rtol=1e-8, max_it=200)
    res = np.linalg.norm(f - _scipy(A) @ x) / np.linalg.norm(f)
    print(f"pipecg + gamg W at 64^2: {info['its']} iterations, true residual {res:.2e}")
    assert info["reason"] == 2 and res <= 2e-8


@pytest.mark.parametrize("kind,n", [("gamg", 128), ("mg", 65)])
def test_w_cycle_needs_no_more_iterations(kind, n):
    A, f = S.AssembleOperator_Laplace(n, n)
    base = dict(coarsening="grid", grid=(n, n)) if kind == "mg" else {}
    its = {}
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        for cycle in ("v", "w"):
            c.pc_setup(S.PC_JACOBI, amg=dict(base, cycle=cycle))
            x, info = c.fgmres(f, rtol=1e-8, restart=30, max_it=200)
            assert info["reason"] == 2 and np.linalg.norm(f - _scipy(A) @ x) <= 2e-8 * np.linalg.norm(f)
            its[cycle] = info["its"]
    print(f"{kind} {n}^2 FGMRES(30): {its['v']} iterations with the V-cycle, {its['w']} with the W-cycle")
    assert its["w"] <= its["v"]


def test_saddle_system_through_the_facade():
    """FULL factorisation, the exact Schur complement, the W-cycle for A^-1: through the facade's options, and through the
    runner, whose -ksp_view names the cycle"""
    A, f = S.AssembleOperator_Laplace(33, 33)
    B, g = S.AssembleOperator_Constraints(33, 33)
    rhs = np.concatenate([f, g])
    Bsp = sp.csr_matrix((B.val, B.colidx, B.rowptr), shape=(B.nrows, A.nrows))
    K = sp.bmat([[_scipy(A), Bsp.T], [Bsp, None]], format="csr")
    opts = ("-ksp_type fgmres -ksp_rtol 1e-8 -pc_type fieldsplit -pc_fieldsplit_type schur -pc_fieldsplit_schur_fact_type full "
            "-pc_fieldsplit_schur_precondition full -fieldsplit_0_ksp_type preonly -fieldsplit_0_pc_type mg "
            "-fieldsplit_0_spk_mg_cycle w")
    k = S.KSP()
    k.setOperators(A, B)
    k.setGrid(33, 33)
    k.setFromOptions(opts)
    x = k.solve(rhs)
    reason = k.getConvergedReason()
    k.destroy()
    res = np.linalg.norm(rhs - K @ x) / np.linalg.norm(rhs)
    assert reason == 2 and res <= 2e-8
    exe = os.path.join(os.path.dirname(S.LIB_PATH), "saddle_point_run")
    out = subprocess.run([exe, "-da_grid_x", "33", "-da_grid_y", "33", "-ksp_converged_reason", "-no_vtk", "-ksp_view"] + opts.split(),
                         capture_output=True, text=True, timeout=120, cwd=tempfile.mkdtemp())
    assert out.returncode == 0, out.stdout + out.stderr
    assert "converged due to CONVERGED_RTOL" in out.stdout, out.stdout
    assert "cycle w (-spk_mg_cycle)" in out.stdout and "tail fused" in out.stdout, out.stdout
    assert re.search(r"tail_first [123], tail_rows \d+ \(default\)", out.stdout), out.stdout


# ---- 6. the W-cycle is symmetric ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "f"])
def test_fused_w_cycle_is_symmetric(name):
    A = _operator(name)
    x, y = _x(A.nrows, 21), _x(A.nrows, 22)
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        info = _setup(c, name, cycle="w", tail="fused", tail_rows=A.nrows)
        assert info["tail_first"] == 1 and info["levels"] >= 4
        Mx, My = c.pc_apply(x), c.pc_apply(y)
    asym = abs(x @ My - y @ Mx) / max(abs(x @ My), abs(y @ Mx))
    print(f"{name}: x^T M y and y^T M x differ by {asym:.3e} relative (bound 1e-12)")
    assert asym <= 1e-12
