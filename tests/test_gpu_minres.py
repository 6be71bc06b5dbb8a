"""spk_minres on the device (-ksp_type minres): the residual history against the numpy restatement of the recurrence
(test_minres_cpu.minres_ref over the CPU oracle's operator and preconditioner), iteration counts, the solution against a
direct solve, bitwise reproducibility, the step-by-step path, the reasons (-3, -8), general constraint blocks, logical
ranks, FGMRES's state left alone, the facade and the runner, device-resident vectors."""
import functools
import os
import subprocess
import tempfile
import threading

import numpy as np
import pytest

from conftest import relerr
from test_minres_cpu import minres_ref, scipy_K

pytestmark = pytest.mark.gpu
NORMS = ("unpreconditioned", "natural")
# History against the reference: 1e-10 relative on K = A.  On the saddle system the multiplier rows of K are four
# sums over the whole grid, and their summation order alone moves the history: the reference itself, run with those
# four rows summed by BLAS instead of in CSR order (a 7e-15 relative change of K x), drifts by 6e-10 within 20
# iterations at 256^2.  The device sums them across workgroups (and ranks), so the saddle system is held to 1e-8.
HIST_TOL = {"A": 1e-10, "diag": 1e-8}


@functools.lru_cache(maxsize=None)
def _problem(kind, mx):
    """kind 'A': K = A with Jacobi (the reference as written); 'diag': the saddle system with Schur DIAG."""
    import saddle_point_petsc_amd as S
    A, f = S.AssembleOperator_Laplace(mx)
    if kind == "A":
        return A, None, f, S.PC_JACOBI, 0
    B, g = S.AssembleOperator_Constraints(mx)
    return A, B, np.concatenate([f, g]), S.PC_SCHUR, S.SCHUR_DIAG


def _ops(oracle, A, B, pc, fact):
    return (lambda v: oracle.apply_K(A, B, v)), (lambda v: oracle.pc_apply(A, B, pc, fact, v))


def _ctx(spk, A, B, pc, fact):
    c = spk.Context(0)
    c.set_block(spk.BLOCK_A00, A)
    if B is not None:
        c.set_block(spk.BLOCK_A10, B)
    c.pc_setup(pc, fact)
    return c


def _hist_close(h, ref, tol):
    h, ref = np.asarray(h), np.asarray(ref)
    assert h.shape == ref.shape, (h.shape, ref.shape)
    err = np.max(np.abs(h - ref) / np.abs(ref))
    assert err <= tol, err


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("kind,mx", [("A", 256), ("A", 1024), ("diag", 256), ("diag", 1024)])
def test_history_and_iterations_match_reference(spk, oracle, kind, mx, norm):
    A, B, rhs, pc, fact = _problem(kind, mx)
    K, M = _ops(oracle, A, B, pc, fact)
    with _ctx(spk, A, B, pc, fact) as c:
        _, i20 = c.minres(rhs, norm=norm, rtol=0.0, abstol=0.0, max_it=20)
        x, info = c.minres(rhs, norm=norm, rtol=1e-8)
    _, r20 = minres_ref(K, M, rhs, rtol=0.0, abstol=0.0, max_it=20, norm=norm)
    assert i20["its"] == 20 and i20["reason"] == -3 and i20["cycles"] == 1
    _hist_close(i20["history"], r20["history"], HIST_TOL[kind])
    assert info["reason"] == 2 and len(info["history"]) == info["its"] + 1
    r = rhs - K(x)
    true = np.linalg.norm(r) if norm == "unpreconditioned" else np.sqrt(M(r) @ r)
    assert info["rnorm"] == pytest.approx(true, rel=1e-6)
    assert info["rnorm"] <= 1e-8 * info["rnorm0"] * (1 + 1e-12)
    if mx <= 256:   # (a whole CPU solve at 1024^2 takes minutes: the history above and the true residual stand for it)
        _, ref = minres_ref(K, M, rhs, rtol=1e-8, norm=norm)
        assert ref["reason"] == 2
        assert abs(info["its"] - ref["its"]) <= max(2, ref["its"] // 100), (info["its"], ref["its"])


def test_solution_matches_direct_solve(spk):
    from scipy.sparse.linalg import spsolve
    A, B, rhs, pc, fact = _problem("diag", 128)
    with _ctx(spk, A, B, pc, fact) as c:
        x, info = c.minres(rhs, rtol=1e-10)
    assert info["reason"] == 2
    assert relerr(x, spsolve(scipy_K(A, B), rhs)) < 1e-8


def test_identical_solves_are_bitwise_equal(spk):
    A, B, rhs, pc, fact = _problem("diag", 256)
    with _ctx(spk, A, B, pc, fact) as c:
        x1, i1 = c.minres(rhs, rtol=1e-8)
        x2, i2 = c.minres(rhs, rtol=1e-8)
    with _ctx(spk, A, B, pc, fact) as c:
        x3, i3 = c.minres(rhs, rtol=1e-8)
    for x, i in ((x2, i2), (x3, i3)):
        assert np.array_equal(x, x1) and np.array_equal(i["history"], i1["history"]) and i["its"] == i1["its"]


@pytest.mark.parametrize("kind", ["A", "diag"])
def test_step_by_step_path_matches_fused(spk, kind):
    A, B, rhs, pc, fact = _problem(kind, 128)
    with _ctx(spk, A, B, pc, fact) as c:
        xf, f = c.minres(rhs, rtol=1e-8)
        xu, u = c.minres(rhs, rtol=1e-8, fused=0)
    assert f["reason"] == u["reason"] == 2 and f["its"] == u["its"]
    _hist_close(u["history"], f["history"], 1e-12)
    assert relerr(xu, xf) < 1e-10


def test_max_it_cut_and_nonzero_guess(spk, oracle):
    A, B, rhs, pc, fact = _problem("diag", 128)
    K, M = _ops(oracle, A, B, pc, fact)
    with _ctx(spk, A, B, pc, fact) as c:
        _, cut = c.minres(rhs, rtol=1e-12, max_it=37)
        xs, _ = c.minres(rhs, rtol=1e-10)
        x0 = xs * (1.0 + 1e-3 * np.sin(0.37 * np.arange(len(xs))))
        for norm in NORMS:
            x, info = c.minres(rhs, x0=x0, norm=norm, rtol=1e-8)
            xr, ref = minres_ref(K, M, rhs, x0=x0, rtol=1e-8, norm=norm)
            assert info["reason"] == ref["reason"] == 2
            assert abs(info["its"] - ref["its"]) <= max(2, ref["its"] // 100)
            n = min(10, len(ref["history"]))
            _hist_close(info["history"][:n], ref["history"][:n], HIST_TOL["diag"])
            assert relerr(x, xr) < 1e-6
    assert cut["reason"] == -3 and cut["its"] == 37 and len(cut["history"]) == 38


def test_indefinite_preconditioner_is_a_reason(spk):
    import saddle_point_petsc_amd as S
    A, f = S.AssembleOperator_Laplace(64)
    An = S.CSR(A.rowptr, A.colidx, -A.val, A.ncols)
    with spk.Context(0) as c:
        c.set_block(spk.BLOCK_A00, An)
        c.pc_setup(spk.PC_JACOBI)
        _, info = c.minres(-f, rtol=1e-8)
        assert info["reason"] == spk.DIVERGED_INDEFINITE_PC == -8
        c.set_block(spk.BLOCK_A00, A)
        c.pc_setup(spk.PC_JACOBI)
        x, info = c.minres(f, rtol=1e-8)
        assert info["reason"] == 2
        assert np.linalg.norm(f - c.mult(x)) <= 1.0001e-8 * np.linalg.norm(f)


def test_general_constraint_block(spk, oracle):
    grid = (12, 10, 9)
    A, f = spk.AssembleOperator_Laplace3D(*grid)
    Bm, g = spk.AssembleOperator_Constraints3D(*grid)
    Bd = spk.AssembleOperator_Divergence3D(*grid)
    B = spk.CSR.vstack([Bm, Bd])
    rhs = np.concatenate([f, g, np.zeros(Bd.nrows)])
    Ao = oracle.CSR(A.rowptr, A.colidx, A.val, A.ncols)
    Bo = oracle.CSR(B.rowptr, B.colidx, B.val, B.ncols)
    K, M = _ops(oracle, Ao, Bo, oracle.PC_SCHUR, 0)
    # K is singular here (test_gpu_general_b.py): a fixed number of iterations is compared, as there
    with _ctx(spk, A, B, spk.PC_SCHUR, spk.SCHUR_DIAG) as c:
        assert c.sizes()["m"] > 8     # the general (CSR-by-rows) block
        x, info = c.minres(rhs, rtol=0.0, abstol=0.0, max_it=30)
    xr, ref = minres_ref(K, M, rhs, rtol=0.0, abstol=0.0, max_it=30)
    assert info["its"] == ref["its"] == 30 and info["reason"] == ref["reason"] == -3
    _hist_close(info["history"], ref["history"], HIST_TOL["diag"])
    assert relerr(x, xr) < 1e-6
    assert np.linalg.norm(rhs - K(x)) == pytest.approx(info["rnorm"], rel=1e-6)


@pytest.mark.parametrize("kind", ["diag", "A"])
@pytest.mark.parametrize("P", [2, 3])
def test_logical_ranks_match_one_rank(spk, P, kind):
    """Every rank holds the same history bits.  Against one rank: 1e-12 on K = A (the partition changes only the order
    of well-conditioned sums); on the saddle system the long multiplier rows of K are summed per rank, and that order
    moves the history as it moves the reference's (HIST_TOL): measured 4e-9 (2 ranks) and 1e-8 (3 ranks) at 256^2."""
    mx = my = 256
    A, B, rhs, pc, fact = _problem(kind, mx)
    n = A.nrows
    with _ctx(spk, A, B, pc, fact) as c:
        _, one = c.minres(rhs, rtol=0.0, abstol=0.0, max_it=30)
    grp = spk.LocalGroup(P)
    out, errs = [None] * P, []

    def work(r):
        try:
            b, e = spk.partition_slab(mx, my, r, P)
            As, _ = spk.AssembleOperator_Laplace(mx, my, b, e)
            c = spk.Context(0)
            c.comm_init_local(grp, r)
            c.set_block(spk.BLOCK_A00, As)
            if B is not None:
                Bs, _ = spk.AssembleOperator_Constraints(mx, my, b, e)
                c.set_block(spk.BLOCK_A10, Bs)
            c.pc_setup(pc, fact)
            _, info = c.minres(np.concatenate([rhs[b:e], rhs[n:]]), rtol=0.0, abstol=0.0, max_it=30)
            out[r] = info
            c.close()
        except Exception as ex:  # noqa: BLE001
            errs.append(ex)
            raise

    th = [threading.Thread(target=work, args=(r,)) for r in range(P)]
    [t.start() for t in th]
    [t.join(timeout=300) for t in th]
    grp.close()
    assert not errs, errs
    for info in out:
        assert info["its"] == 30 and np.array_equal(info["history"], out[0]["history"])
    _hist_close(out[0]["history"], one["history"], 1e-12 if kind == "A" else 1e-7)


def test_minres_leaves_fgmres_state_alone(spk):
    A, B, rhs, pc, fact = _problem("diag", 128)
    with _ctx(spk, A, B, pc, fact) as c:
        c.fgmres(rhs, rtol=1e-8)
        c.minres(rhs, rtol=1e-8)
        c.minres(rhs, norm="natural", rtol=1e-6, fused=0)
        x, info = c.fgmres(rhs, rtol=1e-8)
    with _ctx(spk, A, B, pc, fact) as c:
        xf, fresh = c.fgmres(rhs, rtol=1e-8)
    assert np.array_equal(x, xf) and np.array_equal(info["history"], fresh["history"])


def test_facade_and_runner(spk):
    A, B, rhs, pc, fact = _problem("diag", 64)
    k = spk.KSP()
    k.setOperators(A, B)
    k.setFromOptions("-ksp_type minres -ksp_rtol 1e-8 -pc_type fieldsplit -pc_fieldsplit_type schur "
                     "-pc_fieldsplit_schur_fact_type diag")
    x = k.solve(rhs)
    assert k.getType() == "minres" and k.getConvergedReason() == 2
    assert k.getIterationNumber() + 1 == len(k.getConvergenceHistory())
    k.destroy()
    with _ctx(spk, A, B, pc, fact) as c:
        xc, _ = c.minres(rhs, rtol=1e-8)
    assert np.array_equal(x, xc)
    exe = os.path.join(os.path.dirname(spk.LIB_PATH), "saddle_point_run")
    wd = tempfile.mkdtemp()
    common = ["-da_grid_x", "64", "-da_grid_y", "64", "-ksp_type", "minres", "-ksp_rtol", "1e-8", "-pc_type", "fieldsplit",
              "-pc_fieldsplit_type", "schur", "-ksp_converged_reason", "-ksp_view", "-no_vtk", "-pc_fieldsplit_schur_fact_type"]
    out = subprocess.run([exe] + common + ["diag"], capture_output=True, text=True, timeout=120, cwd=wd)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "converged due to CONVERGED_RTOL" in out.stdout and "type minres" in out.stdout
    bad = subprocess.run([exe] + common + ["full"], capture_output=True, text=True, timeout=120, cwd=wd)
    assert bad.returncode == 1 and "fact_type diag" in bad.stderr


def test_device_vectors_give_host_bits(spk):
    A, B, rhs, pc, fact = _problem("diag", 128)
    with _ctx(spk, A, B, pc, fact) as c:
        xh, ih = c.minres(rhs, rtol=1e-8)
        n = len(rhs)
        bd, xd = c.vec_create(rhs), c.vec_create(n=n)
        idev = c.minres_device(bd, xd, rtol=1e-8)
        x = c.vec_get(xd, n)
        c.vec_destroy(bd)
        c.vec_destroy(xd)
    assert np.array_equal(x, xh) and np.array_equal(idev["history"], ih["history"])
