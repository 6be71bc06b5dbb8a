"""spk_pipecg on the device (-ksp_type pipecg, K = A): the residual history against the numpy restatement of the
recurrence (test_pipecg_cpu.pipecg_ref), iteration counts, the solution against a direct solve, bitwise
reproducibility, the step-by-step path, the V-cycle preconditioner, the reasons (-3, -8, -10), the refused constraint
block, logical ranks, FGMRES's and MINRES's state left alone, device-resident vectors, the facade and the runner."""
import functools
import os
import subprocess
import tempfile
import threading

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import relerr
from test_amg_cpu import hierarchy_mats, vcycle_ref
from test_pipecg_cpu import pipecg_ref

pytestmark = pytest.mark.gpu
NORMS = ("unpreconditioned", "natural")


@functools.lru_cache(maxsize=None)
def _laplace(n):
    import saddle_point_petsc_amd as S
    A, f = S.AssembleOperator_Laplace(n)
    Asp = sp.csr_matrix((A.val, A.colidx, A.rowptr), shape=(A.nrows, A.nrows))
    return A, f, Asp, 1.0 / Asp.diagonal()


def _ops(Asp, d, pc):
    return (lambda v: Asp @ v), ((lambda v: d * v) if pc == "jacobi" else (lambda v: v.copy()))


def _ctx(spk, A, pc="jacobi", B=None):
    c = spk.Context(0)
    c.set_block(spk.BLOCK_A00, A)
    if B is not None:
        c.set_block(spk.BLOCK_A10, B)
    if pc == "gamg":
        c.pc_setup(spk.PC_JACOBI, amg=True)
    else:
        c.pc_setup(spk.PC_JACOBI if pc == "jacobi" else spk.PC_NONE)
    return c


def _hist_close(h, ref, tol):
    h, ref = np.asarray(h), np.asarray(ref)
    assert h.shape == ref.shape, (h.shape, ref.shape)
    err = np.max(np.abs(h - ref) / np.abs(ref))
    assert err <= tol, err


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("pc", ["jacobi", "none"])
@pytest.mark.parametrize("mx", [256, 1024])
def test_history_and_iterations_match_reference(spk, mx, pc, norm):
    A, f, Asp, d = _laplace(mx)
    K, M = _ops(Asp, d, pc)
    with _ctx(spk, A, pc) as c:
        _, i200 = c.pipecg(f, norm=norm, rtol=0.0, abstol=0.0, max_it=200)
        x, info = c.pipecg(f, norm=norm, rtol=1e-8, max_it=20000)
    _, r200 = pipecg_ref(K, M, f, rtol=0.0, abstol=0.0, max_it=200, norm=norm, urec=False)
    assert i200["its"] == 200 and i200["reason"] == -3 and i200["cycles"] == 1
    _hist_close(i200["history"], r200["history"], 1e-10)
    assert info["reason"] == 2 and len(info["history"]) == info["its"] + 1
    r = f - K(x)
    true = np.linalg.norm(r) if norm == "unpreconditioned" else np.sqrt(M(r) @ r)
    assert info["rnorm"] == pytest.approx(true, rel=1e-6)
    assert info["rnorm"] <= 1e-8 * info["rnorm0"] * (1 + 1e-12)
    print(f"{mx}^2 {pc} {norm}: {info['its']} iterations, {info['cycles']} start(s), {info['solve_seconds'] * 1e3:.1f} ms")
    if mx <= 256:   # (a whole CPU solve at 1024^2 takes minutes: the history above and the true residual stand for it)
        _, ref = pipecg_ref(K, M, f, rtol=1e-8, norm=norm, urec=False)
        assert ref["reason"] == 2
        assert abs(info["its"] - ref["its"]) <= max(1, ref["its"] // 100), (info["its"], ref["its"])


def test_solution_matches_direct_solve(spk):
    from scipy.sparse.linalg import spsolve
    A, f, Asp, _ = _laplace(256)
    with _ctx(spk, A) as c:
        x, info = c.pipecg(f, rtol=1e-10, max_it=20000)
    assert info["reason"] == 2
    assert relerr(x, spsolve(Asp.tocsc(), f)) < 1e-8
    assert info["rnorm"] == pytest.approx(np.linalg.norm(f - Asp @ x), rel=1e-6)


def test_identical_solves_are_bitwise_equal(spk):
    A, f, _, _ = _laplace(256)
    with _ctx(spk, A) as c:
        x1, i1 = c.pipecg(f, rtol=1e-8)
        x2, i2 = c.pipecg(f, rtol=1e-8)
    with _ctx(spk, A) as c:
        x3, i3 = c.pipecg(f, rtol=1e-8)
    for x, i in ((x2, i2), (x3, i3)):
        assert np.array_equal(x, x1) and np.array_equal(i["history"], i1["history"]) and i["its"] == i1["its"]


@pytest.mark.parametrize("pc", ["jacobi", "none"])
def test_step_by_step_path_matches_fused(spk, pc):
    A, f, _, _ = _laplace(256)
    with _ctx(spk, A, pc) as c:
        xf, fu = c.pipecg(f, rtol=1e-8)
        xu, u = c.pipecg(f, rtol=1e-8, fused=0)
    assert fu["reason"] == u["reason"] == 2 and fu["its"] == u["its"]
    _hist_close(u["history"], fu["history"], 1e-12)
    assert relerr(xu, xf) < 1e-12


def test_gamg_iterations_are_mesh_independent(spk):
    its = {}
    for n in (128, 1024):
        A, f, Asp, _ = _laplace(n)
        with _ctx(spk, A, "gamg") as c:
            x, info = c.pipecg(f, rtol=1e-8, max_it=500)
        assert info["reason"] == 2
        assert info["rnorm"] == pytest.approx(np.linalg.norm(f - Asp @ x), rel=1e-6)
        its[n] = info["its"]
    print("pipecg + gamg iterations to rtol 1e-8:", its)
    assert its[1024] <= 1.5 * its[128], its


@pytest.mark.parametrize("norm", NORMS)
def test_gamg_history_matches_numpy_vcycle(spk, norm):
    A, f, Asp, _ = _laplace(64)
    with _ctx(spk, A, "gamg") as c:
        info = c.amg_info()
        mats = hierarchy_mats(c.amg_level, info)
        x, dev = c.pipecg(f, norm=norm, rtol=1e-8, max_it=500)
    lam = info["lambda_max"]
    xr, ref = pipecg_ref(lambda v: Asp @ v, lambda v: vcycle_ref(*mats, lam, v), f, rtol=1e-8, norm=norm, urec=True)
    assert dev["reason"] == ref["reason"] == 2 and dev["its"] == ref["its"]
    # 1e-6, not 1e-8: one device V-cycle agrees with vcycle_ref to 1e-12 (test_gpu_amg.py), and the history falls by
    # 1e-8 in ~15 iterations, so the last entries carry that 1e-12 of the first ones (measured 1.2e-7 / 2.1e-8)
    _hist_close(dev["history"], ref["history"], 1e-6)
    assert relerr(x, xr) < 1e-8


def test_max_it_cut_and_nonzero_guess(spk):
    A, f, Asp, d = _laplace(128)
    K, M = _ops(Asp, d, "jacobi")
    with _ctx(spk, A) as c:
        _, cut = c.pipecg(f, rtol=1e-12, max_it=37)
        xs, _ = c.pipecg(f, rtol=1e-10)
        x0 = xs * (1.0 + 1e-3 * np.sin(0.37 * np.arange(len(xs))))
        for norm in NORMS:
            x, info = c.pipecg(f, x0=x0, norm=norm, rtol=1e-8)
            xr, ref = pipecg_ref(K, M, f, x0=x0, rtol=1e-8, norm=norm, urec=False)
            assert info["reason"] == ref["reason"] == 2
            assert abs(info["its"] - ref["its"]) <= max(1, ref["its"] // 100)
            # r = b - K x0 cancels three digits (x0 is 1e-3 off the solution): the two summation orders of K x0 differ
            # by more, relative to r, than those of a zero guess (measured 3.6e-10 over 50 iterations)
            n = min(50, len(ref["history"]))
            _hist_close(info["history"][:n], ref["history"][:n], 1e-8)
            assert relerr(x, xr) < 1e-6
    assert cut["reason"] == -3 and cut["its"] == 37 and len(cut["history"]) == 38


def test_indefinite_pc_and_matrix_are_reasons(spk):
    import saddle_point_petsc_amd as S
    A, f, _, _ = _laplace(64)
    An = S.CSR(A.rowptr, A.colidx, -A.val, A.ncols)
    with spk.Context(0) as c:
        c.set_block(spk.BLOCK_A00, An)
        c.pc_setup(spk.PC_JACOBI)
        _, info = c.pipecg(-f, rtol=1e-8)
        assert info["reason"] == spk.DIVERGED_INDEFINITE_PC == -8
        c.pc_setup(spk.PC_NONE)
        _, info = c.pipecg(-f, rtol=1e-8)
        assert info["reason"] == spk.DIVERGED_INDEFINITE_MAT == -10
        # the context stays usable
        c.set_block(spk.BLOCK_A00, A)
        c.pc_setup(spk.PC_JACOBI)
        x, info = c.pipecg(f, rtol=1e-8)
        assert info["reason"] == 2
        assert np.linalg.norm(f - c.mult(x)) <= 1.0001e-8 * np.linalg.norm(f)


def test_constraint_block_is_refused(spk):
    import saddle_point_petsc_amd as S
    A, f, _, _ = _laplace(64)
    B, g = S.AssembleOperator_Constraints(64)
    rhs = np.concatenate([f, g])
    with _ctx(spk, A, "jacobi", B) as c:
        with pytest.raises(spk.SpkError) as ei:
            c.pipecg(rhs, rtol=1e-8)
        assert ei.value.code == -6 and "minres" in str(ei.value)
        _, info = c.minres(rhs, rtol=1e-8)   # the context is untouched
        assert info["reason"] == 2
    k = spk.KSP()
    k.setOperators(A, B)
    k.setFromOptions("-ksp_type pipecg -pc_type jacobi")
    with pytest.raises(spk.SpkError) as ei:
        k.setUp()
    assert ei.value.code == -6 and "minres" in str(ei.value)
    k.destroy()


@pytest.mark.parametrize("P", [2, 3])
def test_logical_ranks_match_one_rank(spk, P):
    """Every rank holds the same history bits; against one rank 1e-12 (the partition changes only the order of
    well-conditioned sums)."""
    mx = my = 256
    A, f, _, _ = _laplace(mx)
    with _ctx(spk, A) as c:
        _, one = c.pipecg(f, rtol=0.0, abstol=0.0, max_it=40)
    grp = spk.LocalGroup(P)
    out, errs = [None] * P, []

    def work(r):
        try:
            b, e = spk.partition_slab(mx, my, r, P)
            As, _ = spk.AssembleOperator_Laplace(mx, my, b, e)
            c = spk.Context(0)
            c.comm_init_local(grp, r)
            c.set_block(spk.BLOCK_A00, As)
            c.pc_setup(spk.PC_JACOBI)
            _, info = c.pipecg(f[b:e], rtol=0.0, abstol=0.0, max_it=40)
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
        assert info["its"] == 40 and np.array_equal(info["history"], out[0]["history"])
    _hist_close(out[0]["history"], one["history"], 1e-12)


def test_pipecg_leaves_fgmres_and_minres_state_alone(spk):
    A, f, _, _ = _laplace(128)
    with _ctx(spk, A) as c:
        xg0, g0 = c.fgmres(f, rtol=1e-8)
        xm0, m0 = c.minres(f, rtol=1e-8)
        c.pipecg(f, rtol=1e-8)
        c.pipecg(f, norm="natural", rtol=1e-6, fused=0)
        xg, g = c.fgmres(f, rtol=1e-8)
        xm, m = c.minres(f, rtol=1e-8)
    with _ctx(spk, A) as c:
        xgf, gf = c.fgmres(f, rtol=1e-8)
        xmf, mf = c.minres(f, rtol=1e-8)
    for x, i in ((xg0, g0), (xg, g)):
        assert np.array_equal(x, xgf) and np.array_equal(i["history"], gf["history"])
    for x, i in ((xm0, m0), (xm, m)):
        assert np.array_equal(x, xmf) and np.array_equal(i["history"], mf["history"])


@pytest.mark.parametrize("pc", ["jacobi", "gamg"])
def test_device_vectors_give_host_bits(spk, pc):
    A, f, _, _ = _laplace(128)
    with _ctx(spk, A, pc) as c:
        xh, ih = c.pipecg(f, rtol=1e-8)
        n = len(f)
        bd, xd = c.vec_create(f), c.vec_create(n=n)
        idev = c.pipecg_device(bd, xd, rtol=1e-8)
        x = c.vec_get(xd, n)
        c.vec_destroy(bd)
        c.vec_destroy(xd)
    assert np.array_equal(x, xh) and np.array_equal(idev["history"], ih["history"])


def test_facade_and_runner(spk):
    A, f, _, _ = _laplace(64)
    k = spk.KSP()
    k.setOperators(A, None)
    k.setFromOptions("-ksp_type pipecg -ksp_norm_type natural -ksp_rtol 1e-8 -pc_type jacobi")
    x = k.solve(f)
    assert k.getType() == "pipecg" and k.getNormType() == "natural" and k.getConvergedReason() == 2
    assert k.getIterationNumber() + 1 == len(k.getConvergenceHistory())
    k.destroy()
    with _ctx(spk, A) as c:
        xc, _ = c.pipecg(f, norm="natural", rtol=1e-8)
    assert np.array_equal(x, xc)
    exe = os.path.join(os.path.dirname(spk.LIB_PATH), "saddle_point_run")
    wd = tempfile.mkdtemp()
    cmd = [exe, "-saddle", "0", "-da_grid_x", "257", "-da_grid_y", "257", "-ksp_type", "pipecg", "-pc_type", "gamg",
           "-ksp_rtol", "1e-8", "-ksp_converged_reason", "-ksp_view", "-no_vtk"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=wd)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "converged due to CONVERGED_RTOL" in out.stdout and "type pipecg" in out.stdout, out.stdout
    for pc in ("jacobi", "none"):
        out = subprocess.run(cmd[:10] + [pc] + cmd[11:], capture_output=True, text=True, timeout=240, cwd=wd)
        assert out.returncode == 0 and "converged due to CONVERGED_RTOL" in out.stdout, out.stdout + out.stderr
    bad = subprocess.run([exe, "-da_grid_x", "64", "-da_grid_y", "64", "-ksp_type", "pipecg", "-pc_type", "jacobi", "-no_vtk"],
                         capture_output=True, text=True, timeout=120, cwd=wd)
    assert bad.returncode == 1 and "minres" in bad.stderr
