"""The history bars of test_gpu_offgrid.py come from a measurement: how far the numpy references themselves move when
only the order of each row's sum in K x is reversed.  This file repeats that measurement without a GPU and holds the
figures recorded in the input tables to it, so that a bar cannot drift from its source."""
import numpy as np
import pytest

from conftest import relerr
import test_gpu_offgrid as T


def _moved(name, pcs, solvers, kmax, oracle=None):
    """the largest relative movement of the history over the compared window, and of x, per solver"""
    Krev = T._reversed_rows(T._input(name)["K"])
    b = T._input(name)["rhs"]
    out = {}
    for solver in solvers:
        mv = 0.0
        for pc in pcs:
            K, M = T._ops(name, pc, oracle)
            K2, _ = T._ops(name, pc, oracle, K=Krev)
            for norm in T.NORMS:
                x1, r1 = T._ref(solver, K, M, b, norm, rtol=0.0, abstol=0.0, max_it=kmax)
                x2, r2 = T._ref(solver, K2, M, b, norm, rtol=0.0, abstol=0.0, max_it=kmax)
                h1, h2 = r1["history"], r2["history"]
                w = T._window(h1)
                mv = max(mv, np.max(np.abs(h1[:w] - h2[:w]) / np.abs(h1[:w])), relerr(x2, x1))
        out[solver] = mv
    return out


def _within_a_factor_two(table, fresh, what):
    assert 0.5 * fresh <= table <= 2.0 * fresh, (what, table, fresh)


@pytest.mark.parametrize("name", list(T.INPUTS))
def test_recorded_movement_of_the_references(name):
    kmax = 3 if name in T.PAST_EXACT else T.K_STEPS[-1]    # (gen7: the steps that are compared)
    got = _moved(name, ("none", "jacobi"), T.SOLVERS, kmax)
    cg, mr = T.INPUTS[name]["moved"]
    _within_a_factor_two(cg, max(got["pipecg"], got["pipecgrr"]), (name, "cg"))
    _within_a_factor_two(mr, got["minres"], (name, "minres"))


@pytest.mark.parametrize("name", list(T.SADDLES))
def test_recorded_movement_of_minres_ref_on_the_saddle_systems(oracle, name):
    got = _moved(name, ("diag",), ("minres",), T.K_SADDLE[-1], oracle)
    _within_a_factor_two(T.SADDLES[name]["moved"], got["minres"], name)


@pytest.mark.parametrize("name", [n for n, m in T.GAMG_MOVED.items() if m is not None])
def test_recorded_movement_of_the_gamg_history(name):
    """pipecg_ref(urec=True) over the numpy V-cycle of the host builder's hierarchy, to rtol 1e-8: the whole history"""
    import saddle_point_petsc_amd as S
    inp = T._input(name)
    h = S.AmgHierarchy(inp["A"])
    info = h.info()
    assert info["rows"] == T.INPUTS[name]["rows"] and info["block_size"] == T.INPUTS[name]["bs"]
    mats, lam = T.hierarchy_mats(h.matrix, info), info["lambda_max"]
    K, Kr, b = inp["K"], T._reversed_rows(inp["K"]), inp["rhs"]
    mv = 0.0
    for norm in T.NORMS:
        runs = [T.pipecg_ref(lambda v: k @ v, lambda v: T.vcycle_ref(*mats, lam, v), b, rtol=1e-8, norm=norm, urec=True)
                for k in (K, Kr)]
        (x1, r1), (x2, r2) = runs
        assert r1["its"] == r2["its"] and r1["reason"] == r2["reason"] == 2 and relerr(x2, x1) < 1e-12
        mv = max(mv, np.max(np.abs(r1["history"] - r2["history"]) / r1["history"]))
    h.close()
    _within_a_factor_two(T.GAMG_MOVED[name], mv, name)


def test_bars_follow_from_the_tables():
    """max(the project's bar, 100 x moved), and no bar against the reference above 1e-8"""
    for name in T.INPUTS:
        for solver in T.SOLVERS:
            m = T.INPUTS[name]["moved"][1 if solver == "minres" else 0]
            assert T._bar(name, solver) == max(1e-10, 100 * m) <= 1e-8
            assert T._bar(name, solver, 1e-12) == max(1e-12, 100 * m)
    assert [n for n in T.INPUTS if T._gamg_bar(n) != 1e-6] == ["strip"] and T._gamg_bar("strip") == 100 * T.GAMG_MOVED["strip"]
    for name in T.SADDLES:
        assert T._bar(name, "minres") == 1e-8 >= 100 * T.SADDLES[name]["moved"]
