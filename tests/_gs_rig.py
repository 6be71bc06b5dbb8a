"""What the tests of form 7's launch variants share (tests/test_gpu_gs_keep.py, test_gpu_gs_ahead.py, test_gpu_gs_tail.py
and the child processes _gs_ahead_worker.py, _gs_tail_worker.py): the systems and contexts, the case loop of a child, the
fixture that runs one child per value of a knob, and the bit-for-bit comparisons.

A child runs all cases of its table under one value of its knob (SPK_GS_AHEAD=1 python _gs_ahead_worker.py OUT_DIR: a
fresh process per variant, clean contexts).  Per case it solves with AUTO (form 7 asserted by the test) and with forced
form 5 on one context, compares the two in place and writes the AUTO solve's x as OUT_DIR/<case>.npy and everything else
to OUT_DIR/results.json (the residual histories as hex floats: bit-exact).  Nothing here is imported by the CPU suite."""
import json
import os
import subprocess
import sys

import numpy as np

UN3, GSF, LOWER, FULL = 5, 7, 1, 3   # iteration forms; Schur factorisations
KNOBS = ("SPK_GS_KEEP", "SPK_GS_AHEAD", "SPK_GS_TAIL")


def _system(S, grid, saddle):
    if len(grid) == 3:
        A, f = S.AssembleOperator_Laplace3D(*grid, nthreads=16)
        B, g = S.AssembleOperator_Constraints3D(*grid)
        return A, B, np.concatenate([f, g])
    A, f = S.AssembleOperator_Laplace(*grid)
    if not saddle:
        return A, None, f
    B, g = S.AssembleOperator_Constraints(*grid)
    return A, B, np.concatenate([f, g])


def _ctx(S, A, B, fact=FULL):
    c = S.Context(0)
    c.set_block(S.BLOCK_A00, A)
    if B is not None:
        c.set_block(S.BLOCK_A10, B)
    c.pc_setup(S.PC_SCHUR if B is not None else S.PC_JACOBI, fact)
    return c


def _hist(r):
    return np.array([float.fromhex(v) for v in r["history"]])


def _record(x, info, form):
    return {"its": int(info["its"]), "reason": int(info["reason"]), "form": int(form),
            "history": [float(v).hex() for v in np.asarray(info["history"], float)]}


def package():
    """The package, for a child started from tests/."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import saddle_point_petsc_amd as S
    return S


def solved_cases(S, cases, stack, out_dir, res, record=lambda c, info: _record(None, info, c.iteration_form()[0])):
    """The child's case loop over cases = {name: (grid, saddle, fact, restart, max_it)}; consecutive cases share system
    and context (entered on stack).  Fills res[name], and res["gated"] behind the case "full"; yields
    (name, c, rhs, x7, restart, max_it) behind each case for what a child adds of its own, and writes res behind the last."""
    sys_key = ctx_key = None
    for name, (grid, saddle, fact, restart, max_it) in cases.items():
        if (grid, saddle) != sys_key:
            stack.close()
            ctx_key = None
            sys_key = (grid, saddle)
            A, B, rhs = _system(S, grid, saddle)
        if (sys_key, fact) != ctx_key:
            stack.close()
            ctx_key = (sys_key, fact)
            c = stack.enter_context(_ctx(S, A, B, fact))
        x7, i7 = c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=max_it, restart=restart)
        r = record(c, i7)
        r["rows"], r["m"] = int(A.nrows), 0 if B is None else int(B.nrows)
        x5, i5 = c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=max_it, restart=restart, iteration_form=UN3)
        r["form5"] = record(c, i5)
        r["x_equals_form5"] = bool(np.array_equal(x7, x5))
        np.save(os.path.join(out_dir, name + ".npy"), x7)
        res[name] = r
        if name == "full":
            # -ksp_max_it in the middle of the second cycle, the convergence test live: the launches enqueued behind the end
            # of the solve are gated off with their early loads in flight; the next solve must not notice
            _, ig = c.fgmres(rhs, rtol=1e-30, max_it=47, restart=restart)
            g = record(c, ig)
            xa, ia = c.fgmres(rhs, rtol=0.0, abstol=0.0, max_it=max_it, restart=restart)
            g["after"] = record(c, ia)
            g["after_x_equal"] = bool(np.array_equal(xa, x7))
            res["gated"] = g
        yield name, c, rhs, x7, restart, max_it
    with open(os.path.join(out_dir, "results.json"), "w") as fh:
        json.dump(res, fh)


def child_runs(knob, variants, worker):
    """A module-scoped fixture: {variant: (results, directory of the x arrays)} of one child per value of knob, the other
    knobs at their defaults; the children run one after the other (the launch needs all its workgroups resident)."""
    import pytest

    @pytest.fixture(scope="module")
    def runs(tmp_path_factory):
        out = {}
        for a in variants:
            d = tmp_path_factory.mktemp(knob[4:].lower() + "_" + a)
            env = {k: v for k, v in os.environ.items() if k not in KNOBS and k != "SPK_ITER_FORM"}
            env[knob] = a
            p = subprocess.run([sys.executable, worker, str(d)], env=env, capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, f"{knob}={a}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
            with open(d / "results.json") as fh:
                out[a] = (json.load(fh), d)
            assert out[a][0]["knob"] == a
        return out
    return runs


def assert_form_5_bit_for_bit(runs, variants, name, max_it):
    """AUTO took form 7 under every variant; its residual history and x equal forced form 5 on the same context and the
    other variants' (np.array_equal)."""
    ref, dref = runs[variants[0]]
    x0 = np.load(dref / (name + ".npy"))
    for a in variants:
        r, d = runs[a]
        r = r[name]
        assert r["form"] == GSF and r["form5"]["form"] == UN3, (a, r["form"], r["form5"]["form"])
        assert r["its"] == r["form5"]["its"] == max_it and r["reason"] == r["form5"]["reason"], a
        assert np.array_equal(_hist(r), _hist(r["form5"])) and r["x_equals_form5"], a
        assert len(r["history"]) >= max_it
        if a != variants[0]:
            assert np.array_equal(_hist(r), _hist(ref[name])), a
            assert np.array_equal(np.load(d / (name + ".npy")), x0), a
    assert np.isfinite(x0).all() and np.isfinite(_hist(ref[name])).all()


def assert_gated(r):
    """-ksp_max_it 47 at restart 30: the count and the reason are max_it's, the next solve the undisturbed one bit for bit."""
    g = r["gated"]
    assert g["form"] == GSF and g["its"] == 47 and g["reason"] == -3
    assert g["after"]["its"] == 45 and g["after"]["reason"] == r["full"]["reason"]
    assert np.array_equal(_hist(g["after"]), _hist(r["full"])) and g["after_x_equal"]
