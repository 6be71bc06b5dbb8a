"""The smoothed-aggregation multigrid preconditioner on the device (-pc_type gamg, -fieldsplit_0_pc_type gamg): one
V-cycle against the numpy restatement over the exported hierarchy, FGMRES solutions against direct solves, the
mesh-independent iteration count, the Schur fieldsplit with the V-cycle for A^-1, bitwise reproducibility, the context
afterwards, truncated solves, device vectors, the one-rank limit, the facade and the runner."""
import functools
import os
import subprocess
import tempfile
import threading

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from test_amg_cpu import hierarchy_mats, vcycle_ref

pytestmark = pytest.mark.gpu
SPK_ERR_UNSUPPORTED = -6


@functools.lru_cache(maxsize=None)
def _laplace(n):
    import saddle_point_petsc_amd as S
    A, f = S.AssembleOperator_Laplace(n)
    return A, f, sp.csr_matrix((A.val, A.colidx, A.rowptr), shape=(A.nrows, A.nrows))


@functools.lru_cache(maxsize=None)
def _saddle(n):
    import saddle_point_petsc_amd as S
    A, f, Asp = _laplace(n)
    B, g = S.AssembleOperator_Constraints(n)
    Bsp = sp.csr_matrix((B.val, B.colidx, B.rowptr), shape=(B.nrows, A.nrows))
    K = sp.bmat([[Asp, Bsp.T], [Bsp, None]], format="csc")
    return A, B, np.concatenate([f, g]), K


def _ctx(spk, A, B=None, pc=None, fact=None, amg=True):
    c = spk.Context(0)
    c.set_block(spk.BLOCK_A00, A)
    if B is not None:
        c.set_block(spk.BLOCK_A10, B)
    c.pc_setup(spk.PC_JACOBI if pc is None else pc, spk.SCHUR_FULL if fact is None else fact, amg=amg)
    return c


VCYCLES = [dict(smoother="chebyshev", smooth_its=1, nsmooths=1), dict(smoother="chebyshev", smooth_its=3, nsmooths=0),
           dict(smoother="richardson", smooth_its=1, nsmooths=0, richardson_scale=0.6),
           dict(smoother="richardson", smooth_its=3, nsmooths=1, richardson_scale=0.6), dict()]


@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("opts", VCYCLES, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()) or "default")
def test_one_vcycle_matches_numpy(spk, n, opts):
    A, f, _ = _laplace(n)
    rng = np.random.default_rng(7)
    x = rng.standard_normal(A.nrows)
    with _ctx(spk, A, amg=opts) as c:
        info = c.amg_info()
        y = c.pc_apply(x)
        mats = hierarchy_mats(c.amg_level, info)
    kw = {k: v for k, v in opts.items() if k in ("smoother", "smooth_its", "richardson_scale")}
    ref = vcycle_ref(*mats, info["lambda_max"], x, **kw)
    assert np.linalg.norm(y - ref) <= 1e-12 * np.linalg.norm(ref)


@pytest.mark.parametrize("fmt", [None, "bcsr", "csr"])
def test_vcycle_on_every_fine_layout(spk, monkeypatch, fmt):
    """The default 2x2 row-type layout takes the fused fine-level Chebyshev kernel; BCSR and CSR the layout's product and
    a vector pass.  All three match the numpy V-cycle, and one another."""
    if fmt is None:
        monkeypatch.delenv("SPK_SPMV_FORMAT", raising=False)
    else:
        monkeypatch.setenv("SPK_SPMV_FORMAT", fmt)
    A, f, _ = _laplace(256)
    x = np.random.default_rng(3).standard_normal(A.nrows)
    with _ctx(spk, A, amg=dict(smooth_its=3)) as c:
        layout = c.spmv_info()["format"]
        info = c.amg_info()
        y = c.pc_apply(x)
        y2 = c.pc_apply(x)
        mats = hierarchy_mats(c.amg_level, info)
    assert layout == {None: "dict2x2", "bcsr": "bcsr2x2", "csr": "csr"}[fmt]
    assert np.array_equal(y, y2)
    ref = vcycle_ref(*mats, info["lambda_max"], x, smooth_its=3)
    assert np.linalg.norm(y - ref) <= 1e-12 * np.linalg.norm(ref)


@pytest.mark.parametrize("n", [64, 128, 256])
def test_fgmres_gamg_solution_matches_spsolve(spk, n):
    A, f, Asp = _laplace(n)
    with _ctx(spk, A) as c:
        x, info = c.fgmres(f, rtol=1e-10, max_it=200)
        assert c.iteration_form()[0] == -1
    assert info["reason"] == 2
    xd = spl.spsolve(Asp.tocsc(), f)
    assert np.linalg.norm(x - xd) <= 1e-8 * np.linalg.norm(xd)


def test_iteration_count_is_mesh_independent(spk):
    its = {}
    for n in (128, 256, 512, 1024):
        A, f, _ = _laplace(n)
        with _ctx(spk, A) as c:
            _, info = c.fgmres(f, rtol=1e-8, max_it=500)
        assert info["reason"] == 2
        its[n] = info["its"]
    print("gamg iterations to rtol 1e-8:", its)
    assert max(its.values()) <= 40 and its[1024] <= 2 * its[128], its


@pytest.mark.parametrize("fact", ["DIAG", "LOWER", "UPPER", "FULL"])
def test_schur_fieldsplit_with_gamg_converges(spk, fact):
    A, B, rhs, K = _saddle(256)
    with _ctx(spk, A, B, spk.PC_SCHUR, getattr(spk, "SCHUR_" + fact)) as c:
        x, info = c.fgmres(rhs, rtol=1e-8, max_it=2000)
        assert c.iteration_form()[0] == -1
    assert info["reason"] == 2, info["its"]
    xd = spl.spsolve(K, rhs)
    assert np.linalg.norm(x - xd) <= 1e-6 * np.linalg.norm(xd)


def test_schur_full_with_gamg_at_1024(spk):
    A, B, rhs, _ = _saddle(1024)
    with _ctx(spk, A, B, spk.PC_SCHUR, spk.SCHUR_FULL) as c:
        x, info = c.fgmres(rhs, rtol=1e-8, max_it=100)
        r = rhs - c.mult(x)
    print("saddle FULL + gamg at 1024^2:", info["its"], "iterations", info["solve_seconds"], "s")
    assert info["reason"] == 2 and info["its"] <= 100
    assert np.linalg.norm(r) <= 1e-7 * np.linalg.norm(rhs)


def test_identical_solves_identical_bits_and_jacobi_afterwards(spk):
    A, B, rhs, _ = _saddle(128)
    with _ctx(spk, A, B, spk.PC_SCHUR, spk.SCHUR_FULL) as c:
        x1, i1 = c.fgmres(rhs, rtol=1e-8)
        x2, i2 = c.fgmres(rhs, rtol=1e-8)
        assert np.array_equal(x1, x2) and np.array_equal(i1["history"], i2["history"])
        c.pc_setup(spk.PC_SCHUR, spk.SCHUR_FULL)            # spk_pc_set_amg(NULL): the plain Schur PC again
        xj, ij = c.fgmres(rhs, rtol=1e-8, max_it=300)
        fj = c.iteration_form()
    with _ctx(spk, A, B, spk.PC_SCHUR, spk.SCHUR_FULL, amg=None) as c:
        xf, fresh = c.fgmres(rhs, rtol=1e-8, max_it=300)
        assert c.iteration_form() == fj
    assert np.array_equal(xj, xf) and np.array_equal(ij["history"], fresh["history"])
    A, f, _ = _laplace(128)
    with _ctx(spk, A) as c:
        c.fgmres(f, rtol=1e-8)
        c.pc_setup(spk.PC_JACOBI)
        xj, ij = c.fgmres(f, rtol=1e-8, max_it=200)
    with _ctx(spk, A, amg=None) as c:
        xf, fresh = c.fgmres(f, rtol=1e-8, max_it=200)
    assert np.array_equal(xj, xf) and np.array_equal(ij["history"], fresh["history"])


def test_truncated_solve_and_device_vectors(spk):
    A, f, Asp = _laplace(256)
    with _ctx(spk, A) as c:
        x, info = c.fgmres(f, rtol=1e-12, max_it=5)
        assert info["reason"] == -3 and info["its"] == 5 and len(info["history"]) == 6
        h = info["history"]
        assert h[0] == pytest.approx(np.linalg.norm(f), rel=1e-12)
        assert h[-1] == pytest.approx(np.linalg.norm(f - Asp @ x), rel=1e-8)
        assert np.all(np.diff(h) <= 0)
        xh, ih = c.fgmres(f, rtol=1e-8)
        bd, xd = c.vec_create(f), c.vec_create(n=len(f))
        idev = c.fgmres_device(bd, xd, rtol=1e-8)
        xv = c.vec_get(xd, len(f))
        c.vec_destroy(bd)
        c.vec_destroy(xd)
    assert np.array_equal(xv, xh) and np.array_equal(idev["history"], ih["history"])


def test_two_rank_group_refused_and_usable(spk):
    n, P = 64, 2
    A, f, _ = _laplace(n)
    grp = spk.LocalGroup(P)
    codes, its, errs = [None] * P, [None] * P, []

    def work(r):
        try:
            b, e = spk.partition_slab(n, n, r, P)
            As, _ = spk.AssembleOperator_Laplace(n, n, b, e)
            c = spk.Context(0)
            c.comm_init_local(grp, r)
            c.set_block(spk.BLOCK_A00, As)
            try:
                c.pc_setup(spk.PC_JACOBI, amg=True)
            except spk.SpkError as ex:
                codes[r] = (ex.code, str(ex))
            c.pc_setup(spk.PC_JACOBI)                        # the context stays usable
            _, info = c.fgmres(f[b:e], rtol=1e-8, max_it=3000)
            its[r] = info
            c.close()
        except Exception as ex:  # noqa: BLE001
            errs.append(ex)
            raise

    th = [threading.Thread(target=work, args=(r,)) for r in range(P)]
    [t.start() for t in th]
    [t.join(timeout=300) for t in th]
    grp.close()
    assert not errs, errs
    for code in codes:
        assert code is not None and code[0] == SPK_ERR_UNSUPPORTED and "one rank" in code[1]
    assert all(i["reason"] == 2 for i in its) and its[0]["its"] == its[1]["its"]


def test_minres_refuses_gamg(spk):
    A, f, _ = _laplace(64)
    with _ctx(spk, A) as c:
        with pytest.raises(spk.SpkError) as e:
            c.minres(f, rtol=1e-8)
        assert e.value.code == SPK_ERR_UNSUPPORTED
        x, info = c.fgmres(f, rtol=1e-8)
    assert info["reason"] == 2


def test_facade_and_runner(spk):
    A, B, rhs, K = _saddle(64)
    k = spk.KSP()
    k.setOperators(A, B)
    k.setFromOptions("-ksp_type fgmres -ksp_rtol 1e-8 -pc_type fieldsplit -pc_fieldsplit_type schur "
                     "-pc_fieldsplit_schur_fact_type full -fieldsplit_0_ksp_type preonly -fieldsplit_0_pc_type gamg "
                     "-fieldsplit_0_mg_levels_ksp_max_it 3")
    x = k.solve(rhs)
    assert k.getConvergedReason() == 2
    k.destroy()
    with _ctx(spk, A, B, spk.PC_SCHUR, spk.SCHUR_FULL, amg=dict(smooth_its=3)) as c:
        xc, _ = c.fgmres(rhs, rtol=1e-8)
    assert np.array_equal(x, xc)
    k = spk.KSP()
    k.setOperators(A, B)
    k.setFromOptions("-ksp_type fgmres -pc_type gamg")
    with pytest.raises(spk.SpkError) as e:
        k.setUp()
    assert e.value.code == SPK_ERR_UNSUPPORTED and "multigrid target" in str(e.value)
    k.destroy()

    exe = os.path.join(os.path.dirname(spk.LIB_PATH), "saddle_point_run")
    wd = tempfile.mkdtemp()
    grid = ["-da_grid_x", "128", "-da_grid_y", "128", "-ksp_rtol", "1e-8", "-ksp_converged_reason", "-no_vtk"]
    out = subprocess.run([exe] + grid + ["-saddle", "0", "-ksp_type", "fgmres", "-pc_type", "gamg", "-ksp_view"],
                         capture_output=True, text=True, timeout=120, cwd=wd)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "converged due to CONVERGED_RTOL" in out.stdout and "PC gamg" in out.stdout and "level 0" in out.stdout
    out = subprocess.run([exe] + grid + ["-ksp_type", "fgmres", "-pc_type", "fieldsplit", "-pc_fieldsplit_type", "schur",
                                         "-pc_fieldsplit_schur_fact_type", "full", "-fieldsplit_0_pc_type", "gamg"],
                         capture_output=True, text=True, timeout=120, cwd=wd)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "converged due to CONVERGED_RTOL" in out.stdout
    bad = subprocess.run([exe, "-ksp_type", "fgmres", "-pc_type", "gamg", "-no_vtk"], capture_output=True, text=True,
                         timeout=120, cwd=wd)
    assert bad.returncode == 1 and "not a multigrid target" in bad.stderr
