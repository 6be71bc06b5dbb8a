"""Grid-coarsening multigrid on the device (-pc_type mg, SPK_AMG_COARSEN_GRID): the device set-up against the host
builder (P byte for byte, the operators to the bar test_gpu_amg_setup.py holds gamg's routes to), the two matrix-free
transfer kernels alone against a numpy loop that adds in the stated order (bit for bit) and the stored route within
the rounding of a reordered sum, one V-cycle against the numpy restatement on every fine layout with both transfers,
solves, the refresh, and the context after a refusal.

Shapes: the smallest on which each part can go wrong -- 5 x 5 (one interior coarse node), 33 x 9 and 12 x 9 (mixed
halving, a direction that never halves), 9 x 9 x 5 (bs 3, three directions), 33 x 33 (2178 rows: no multiple of the
256-thread workgroup, level 0 padded)."""
import functools
import os
import subprocess
import tempfile
import threading

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import saddle_point_petsc_amd as S
from test_amg_cpu import hierarchy_mats, vcycle_ref
from test_mg_grid_cpu import prolong_ref

pytestmark = pytest.mark.gpu
SPK_ERR_STATE, SPK_ERR_UNSUPPORTED = -3, -6
U = 2.0 ** -53

# name -> (grid, bs); the operators are the package's own discretisation
GRIDS = {"5x5": ((5, 5, 1), 2), "33x9": ((33, 9, 1), 2), "12x9": ((12, 9, 1), 2), "9x9x5": ((9, 9, 5), 3), "33x33": ((33, 33, 1), 2)}


@functools.lru_cache(maxsize=None)
def _operator(name):
    g = GRIDS[name][0]
    A, f = S.AssembleOperator_Laplace3D(*g) if g[2] > 1 else S.AssembleOperator_Laplace(g[0], g[1])
    return A, f


def _scipy(A):
    return sp.csr_matrix((A.val, A.colidx, A.rowptr), shape=(A.nrows, A.nrows))


def _mg(name, **kw):
    """options of a grid hierarchy that coarsens the small grids to the end of the rule"""
    return dict(dict(coarsening="grid", grid=GRIDS[name][0], coarse_eq_limit=10), **kw)


def _ctx(A, B=None, pc=S.PC_JACOBI, fact=S.SCHUR_FULL, amg=None, **kw):
    c = S.Context(0)
    c.set_block(S.BLOCK_A00, A)
    if B is not None:
        c.set_block(S.BLOCK_A10, B)
    c.pc_setup(pc, fact, amg=amg, **kw)
    return c


def _export(get, info):
    L = info["levels"]
    return dict(A=[get(l, S.AMG_OP) for l in range(L)], P=[get(l, S.AMG_PROLONG) for l in range(L - 1)],
                cinv=get(L - 1, S.AMG_COARSE_INV)[2])


def _close(a, b, tol, what):
    err = np.abs(a - b).max() / np.abs(b).max()
    print(f"{what}: max deviation {err:.3e} of the largest entry (bound {tol:g})")
    assert err <= tol, what


# ---- 1. the device route against the host route -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["33x9", "12x9", "9x9x5"])
def test_device_setup_is_the_host_builds(name):
    """P byte for byte (every weight is dyadic); A_l to 1e-12 of its largest entry (a reordered sum of at most ~160
    products, levels compounding: the bar of test_entries_without_prolongator_smoothing), D^-1 with it, lambda_max to
    1e-12 relative and the coarse inverse to 1e-10 (test_entries_with_prolongator_smoothing).  Two device builds give the
    same bytes."""
    A, _ = _operator(name)
    got = []
    for _ in range(2):
        with _ctx(A, amg=_mg(name, setup="device")) as c:
            di = c.amg_info()
            got.append((di, _export(c.amg_level, di)))
            with pytest.raises(S.SpkError) as e:
                c.amg_aggregates(0)
            assert e.value.code == SPK_ERR_UNSUPPORTED
            T = c.amg_level(0, S.AMG_TENTATIVE)
    (di, dev), (di2, dev2) = got
    h = S.AmgHierarchy(A, **_mg(name))
    hi = h.info()
    host = _export(h.matrix, hi)
    h.close()
    assert di["setup"] == S.AMG_SETUP_DEVICE and di["coarsening"] == S.AMG_COARSEN_GRID and di["block_size"] == GRIDS[name][1]
    assert di["levels"] == hi["levels"] >= 3 and di["dims"] == hi["dims"] and di["rows"] == hi["rows"] and di["nnz"] == hi["nnz"]
    for l in range(di["levels"] - 1):
        for a, b in zip(dev["P"][l][:3], host["P"][l][:3]):
            assert a.tobytes() == b.tobytes(), f"P_{l}"
        assert dev["P"][l][3] == host["P"][l][3]
        rel = abs(di["lambda_max"][l] - hi["lambda_max"][l]) / hi["lambda_max"][l]
        print(f"{name} lambda_max[{l}]: relative {rel:.3e} off the host's")
        assert rel <= 1e-12
    assert all(a.tobytes() == b.tobytes() for a, b in zip(T[:3], host["P"][0][:3]))
    for l in range(di["levels"]):
        assert np.array_equal(dev["A"][l][0], host["A"][l][0]) and np.array_equal(dev["A"][l][1], host["A"][l][1]), f"pattern of A_{l}"
        _close(dev["A"][l][2], host["A"][l][2], 1e-12, f"{name} A_{l}")
        dd, dh = (sp.csr_matrix((m[2], m[1], m[0]), shape=m[3]).diagonal() for m in (dev["A"][l], host["A"][l]))
        _close(1.0 / dd, 1.0 / dh, 1e-12, f"{name} D^-1 of level {l}")
    _close(dev["cinv"], host["cinv"], 1e-10, f"{name} coarse inverse")
    assert di2["lambda_max"] == di["lambda_max"]
    for key in ("A", "P"):
        for a, b in zip(dev[key], dev2[key]):
            assert all(u.tobytes() == v.tobytes() for u, v in zip(a[:3], b[:3])), key
    assert dev["cinv"].tobytes() == dev2["cinv"].tobytes()


# ---- 2. the transfer kernels alone -------------------------------------------------------------------------------------------
def _ordered_sum(M, x):
    """per row of the CSR matrix M: the products M_ij x_j added in ascending column order, starting from the first
    product; also sum |terms|.  (numpy multiplies and adds in two roundings; the weights are powers of two.)"""
    n = M.shape[0]
    ln = np.diff(M.indptr)
    s, tot = np.zeros(n), np.zeros(n)
    for t in range(int(ln.max())):
        rows = np.nonzero(ln > t)[0]
        k = M.indptr[rows] + t
        term = M.data[k] * x[M.indices[k]]
        s[rows] = term if t == 0 else s[rows] + term
        tot[rows] += np.abs(term)
    return s, tot


@pytest.mark.parametrize("name", list(GRIDS))
def test_transfer_kernels_add_in_the_stated_order(name):
    """Matrix-free: bit for bit the numpy loop.  Stored (the CSR kernels on P and R): the products are exact, so n - 1
    additions in another order stay within (n - 1) 2^-53 sum|terms| per entry -- n = 9 for the prolongation (eight parents
    and y), n = 27 for the restriction."""
    A, _ = _operator(name)
    grid, bs = GRIDS[name]
    rng = np.random.default_rng(len(name))
    pad = 37
    with _ctx(A, amg=_mg(name, setup="device")) as c:
        info = c.amg_info()
        assert info["levels"] >= 2
        for l in range(info["levels"] - 1):
            nf, nc = info["rows"][l], info["rows"][l + 1]
            P = prolong_ref(info["dims"][l], bs)
            R = P.T.tocsr()
            R.sort_indices()
            assert P.shape == (nf, nc)
            # level 0 works on vectors of the context's padded length: entries behind the rows stay as they are
            e, y, b, t = rng.standard_normal(nc), rng.standard_normal(nf + pad), rng.standard_normal(nf + pad), rng.standard_normal(nf + pad)
            s, tot = _ordered_sum(P, e)
            ref = y[:nf] + s
            out = c.debug_amg_transfer(l, "prolong", e, y)
            assert out[:nf].tobytes() == ref.tobytes(), f"{name} prolongation of level {l}"
            assert out[nf:].tobytes() == y[nf:].tobytes()
            st = c.debug_amg_transfer(l, "prolong", e, y, stored=True)
            assert np.all(np.abs(st[:nf] - ref) <= 8 * U * (tot + np.abs(y[:nf]))), f"{name} stored prolongation of level {l}"
            assert st[nf:].tobytes() == y[nf:].tobytes()
            ref, tot = _ordered_sum(R, b[:nf] - t[:nf])
            assert int(np.diff(R.indptr).max()) <= 27
            out = c.debug_amg_transfer(l, "restrict", b, t)
            assert out.shape == (nc,) and out.tobytes() == ref.tobytes(), f"{name} restriction of level {l}"
            st = c.debug_amg_transfer(l, "restrict", b, t, stored=True)
            assert np.all(np.abs(st - ref) <= 26 * U * tot), f"{name} stored restriction of level {l}"


def test_transfer_hook_refuses_an_aggregation_level():
    A, _ = _operator("33x33")
    with _ctx(A, amg=True) as c:
        info = c.amg_info()
        with pytest.raises(S.SpkError) as e:
            c.debug_amg_transfer(0, "prolong", np.zeros(info["rows"][1]), np.zeros(info["rows"][0]))
        assert e.value.code == SPK_ERR_STATE
        y = c.debug_amg_transfer(0, "prolong", np.ones(info["rows"][1]), np.zeros(info["rows"][0]), stored=True)
        assert y.shape == (info["rows"][0],)


# ---- 3. one V-cycle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transfer", ["matrixfree", "stored"])
@pytest.mark.parametrize("name,fmt,layout", [("33x33", None, "dict2x2"), ("9x9x9", None, "dict3x3"), ("33x33", "csr", "csr")])
def test_one_vcycle_matches_numpy(monkeypatch, name, fmt, layout, transfer):
    """the tolerance of test_vcycle_on_every_fine_layout; two applications give the same bits"""
    if fmt is None:
        monkeypatch.delenv("SPK_SPMV_FORMAT", raising=False)
    else:
        monkeypatch.setenv("SPK_SPMV_FORMAT", fmt)
    if name == "9x9x9":
        A, grid = S.AssembleOperator_Laplace3D(9, 9, 9)[0], (9, 9, 9)
    else:
        A, grid = _operator(name)[0], GRIDS[name][0]
    x = np.random.default_rng(3).standard_normal(A.nrows)
    with _ctx(A, amg=dict(coarsening="grid", grid=grid, transfer=transfer)) as c:
        assert c.spmv_info()["format"] == layout
        info = c.amg_info()
        y = c.pc_apply(x)
        y2 = c.pc_apply(x)
        mats = hierarchy_mats(c.amg_level, info)
    assert info["levels"] >= 3 and info["coarsening"] == S.AMG_COARSEN_GRID
    assert y.tobytes() == y2.tobytes()
    ref = vcycle_ref(*mats, info["lambda_max"], x)
    err = np.linalg.norm(y - ref) / np.linalg.norm(ref)
    print(f"{name} {layout} {transfer}: V-cycle {err:.3e} off numpy (bound 1e-12)")
    assert err <= 1e-12


# ---- 4. solves to rtol 1e-8, the true residual recomputed in numpy -----------------------------------------------------
def test_k_equals_a_with_fgmres_and_pipecg():
    its = {}
    for n in (65, 129):
        A, f = S.AssembleOperator_Laplace(n, n)
        Asp = _scipy(A)
        for kind, amg in (("mg", dict(coarsening="grid", grid=(n, n))), ("gamg", True)):
            with _ctx(A, amg=amg) as c:
                for ksp in ("fgmres", "pipecg"):
                    x, info = getattr(c, ksp)(f, rtol=1e-8, max_it=200)
                    res = np.linalg.norm(f - Asp @ x) / np.linalg.norm(f)
                    its[kind, ksp, n] = info["its"]
                    print(f"{n}^2 {kind} {ksp}: {info['its']} iterations, true residual {res:.2e}")
                    assert info["reason"] == 2 and res <= 2e-8
    for ksp in ("fgmres", "pipecg"):
        assert its["mg", ksp, 129] <= its["mg", ksp, 65] + 1, its
        for n in (65, 129):
            assert its["mg", ksp, n] <= its["gamg", ksp, n], its


def test_saddle_system_with_the_exact_schur_complement():
    A, f = S.AssembleOperator_Laplace(65, 65)
    B, g = S.AssembleOperator_Constraints(65, 65)
    rhs = np.concatenate([f, g])
    Bsp = sp.csr_matrix((B.val, B.colidx, B.rowptr), shape=(B.nrows, A.nrows))
    K = sp.bmat([[_scipy(A), Bsp.T], [Bsp, None]], format="csr")
    with _ctx(A, B, S.PC_SCHUR, S.SCHUR_FULL, amg=dict(coarsening="grid", grid=(65, 65)), schur_pre="full") as c:
        x, info = c.fgmres(rhs, rtol=1e-8, max_it=200)
    res = np.linalg.norm(rhs - K @ x) / np.linalg.norm(rhs)
    print(f"saddle 65^2 FULL + exact S + mg: {info['its']} iterations, true residual {res:.2e}")
    assert info["reason"] == 2 and res <= 2e-8


def test_cube_with_three_unknowns_per_node():
    A, f = S.AssembleOperator_Laplace3D(17, 17, 17)
    with _ctx(A, amg=dict(coarsening="grid", grid=(17, 17, 17))) as c:
        info = c.amg_info()
        x, r = c.fgmres(f, rtol=1e-8, max_it=200)
    res = np.linalg.norm(f - _scipy(A) @ x) / np.linalg.norm(f)
    print(f"17^3: {r['its']} iterations, dims {info['dims']}, true residual {res:.2e}")
    assert info["block_size"] == 3 and info["dims"][:3] == [(17, 17, 17), (9, 9, 9), (5, 5, 5)]
    assert r["reason"] == 2 and res <= 2e-8


def test_runner_names_the_preconditioner():
    exe = os.path.join(os.path.dirname(S.LIB_PATH), "saddle_point_run")
    out = subprocess.run([exe, "-da_grid_x", "65", "-da_grid_y", "65", "-ksp_rtol", "1e-8", "-ksp_converged_reason", "-no_vtk",
                          "-saddle", "0", "-ksp_type", "fgmres", "-pc_type", "mg", "-pc_mg_galerkin", "-ksp_view"],
                         capture_output=True, text=True, timeout=120, cwd=tempfile.mkdtemp())
    assert out.returncode == 0, out.stdout + out.stderr
    assert "converged due to CONVERGED_RTOL" in out.stdout and "PC mg (grid coarsening" in out.stdout, out.stdout
    assert "level 0: grid 65 x 65 x 1" in out.stdout and "level 1: grid 33 x 33 x 1" in out.stdout, out.stdout


def test_facade_with_set_grid_and_inside_the_fieldsplit():
    A, f = S.AssembleOperator_Laplace(33, 33)
    B, g = S.AssembleOperator_Constraints(33, 33)
    rhs = np.concatenate([f, g])
    k = S.KSP()
    k.setOperators(A, B)
    k.setGrid(33, 33)
    k.setFromOptions("-ksp_type fgmres -ksp_rtol 1e-8 -pc_type fieldsplit -pc_fieldsplit_type schur "
                     "-pc_fieldsplit_schur_fact_type full -fieldsplit_0_ksp_type preonly -fieldsplit_0_pc_type mg "
                     "-fieldsplit_0_pc_mg_galerkin")
    x = k.solve(rhs)
    assert k.getConvergedReason() == 2
    k.destroy()
    with _ctx(A, B, S.PC_SCHUR, S.SCHUR_FULL, amg=dict(coarsening="grid", grid=(33, 33))) as c:
        xc, _ = c.fgmres(rhs, rtol=1e-8)
    assert np.array_equal(x, xc)
    k = S.KSP()
    fk = k.setOperatorsLaplace(33, 33)          # the grid comes with the operator
    k.setFromOptions("-ksp_type pipecg -ksp_rtol 1e-8 -pc_type mg -spk_mg_transfer stored")
    x = k.solve(fk)
    assert k.getConvergedReason() == 2 and np.linalg.norm(f - _scipy(A) @ x) <= 2e-8 * np.linalg.norm(f)
    k.destroy()


# ---- 5. the refresh -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["host", "device"])
def test_refresh_keeps_p_and_solves_like_a_fresh_build(route):
    """kappa changed by the device assembler with reuse on: the set-up refreshes, P keeps its bytes, and -- P does not
    depend on the values -- the refreshed operators are a fresh build's to the bar of the device build (1e-12); the solve
    meets spsolve to 1e-8 as in test_fgmres_on_the_new_operator_with_the_refreshed_hierarchy, in the fresh build's
    iterations +- 1.  Another grid or another coarsening is a full build."""
    n = 33
    kappa = 1.0 + np.random.default_rng(5).random((n - 1) * (n - 1))
    A1, f1 = S.AssembleOperator_Laplace(n, n, kappa=kappa)
    amg = dict(coarsening="grid", grid=(n, n), setup=route)
    with S.Context(0) as c:
        c.set_block_laplace(n, n)
        c.pc_setup(S.PC_JACOBI, amg=amg, amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is False
        i0 = c.amg_info()
        e0 = _export(c.amg_level, i0)
        c.set_block_laplace(n, n, kappa=kappa)
        c.pc_setup(S.PC_JACOBI, amg=amg, amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is True
        i1 = c.amg_info()
        e1 = _export(c.amg_level, i1)
        x, info = c.fgmres(f1, rtol=1e-8, max_it=200)
        # the same values again, other options: full builds
        c.pc_setup(S.PC_JACOBI, amg=dict(amg, grid=(n, n, 1), transfer="stored"), amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is False
        c.pc_setup(S.PC_JACOBI, amg=dict(setup=route), amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is False and c.amg_info()["coarsening"] == S.AMG_COARSEN_AGGREGATION
    assert i1["dims"] == i0["dims"] and i1["lambda_max"] != i0["lambda_max"]
    for l in range(i0["levels"] - 1):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(e1["P"][l][:3], e0["P"][l][:3])), f"P_{l}"
    with _ctx(A1, amg=amg) as c:
        fresh = _export(c.amg_level, c.amg_info())
        xf, finfo = c.fgmres(f1, rtol=1e-8, max_it=200)
    for l in range(i1["levels"]):
        assert np.array_equal(e1["A"][l][1], fresh["A"][l][1])
        _close(e1["A"][l][2], fresh["A"][l][2], 1e-12, f"{route} refreshed A_{l}")
    xd = spl.spsolve(_scipy(A1).tocsc(), f1)
    assert info["reason"] == 2 and np.linalg.norm(x - xd) <= 1e-8 * np.linalg.norm(xd)
    assert abs(info["its"] - finfo["its"]) <= 1


def test_a_changed_grid_is_a_full_build():
    """594 rows are a 33 x 9 and a 9 x 33 grid: the same pattern size, another hierarchy"""
    A = _operator("33x9")[0]
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        c.pc_setup(S.PC_JACOBI, amg=dict(coarsening="grid", grid=(33, 9)), amg_reuse=True)
        c.pc_setup(S.PC_JACOBI, amg=dict(coarsening="grid", grid=(33, 9)), amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is True
        c.pc_setup(S.PC_JACOBI, amg=dict(coarsening="grid", grid=(9, 33)), amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is False and c.amg_info()["dims"][0] == (9, 33, 1)


# ---- 6. the context after a refusal ------------------------------------------------------------------------------------------
def test_context_survives_a_grid_that_cannot_be_halved():
    A, f = S.AssembleOperator_Laplace(64, 64)
    for route in ("host", "device"):
        with S.Context(0) as c:
            c.set_block(S.BLOCK_A00, A)
            with pytest.raises(S.SpkError) as e:
                c.pc_setup(S.PC_JACOBI, amg=dict(coarsening="grid", grid=(64, 64), setup=route))
            assert e.value.code == SPK_ERR_UNSUPPORTED and "side of 64 nodes" in str(e.value)
            c.pc_setup(S.PC_JACOBI)
            x, info = c.fgmres(f, rtol=1e-8, max_it=3000)
        assert info["reason"] == 2 and np.linalg.norm(f - _scipy(A) @ x) <= 2e-8 * np.linalg.norm(f)


def test_two_rank_group_refused_and_usable():
    n, P = 64, 2   # (the rank check comes before the hierarchy: the grid is never looked at)
    A, f = S.AssembleOperator_Laplace(n, n)
    grp = S.LocalGroup(P)
    codes, its, errs = [None] * P, [None] * P, []

    def work(r):
        try:
            b, e = S.partition_slab(n, n, r, P)
            As, _ = S.AssembleOperator_Laplace(n, n, b, e)
            c = S.Context(0)
            c.comm_init_local(grp, r)
            c.set_block(S.BLOCK_A00, As)
            try:
                c.pc_setup(S.PC_JACOBI, amg=dict(coarsening="grid", grid=(n, n)))
            except S.SpkError as ex:
                codes[r] = (ex.code, str(ex))
            c.pc_setup(S.PC_JACOBI)                        # the context stays usable
            _, its[r] = c.fgmres(f[b:e], rtol=1e-8, max_it=3000)
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
