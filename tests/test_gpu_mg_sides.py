"""Grid coarsening on even sides on the device (spk_amg_opts.sides = SPK_AMG_SIDES_ANY, -spk_mg_sides any): the two
matrix-free transfer kernels alone against a numpy loop that adds in the stated order (bit for bit) with the stored route
within the rounding of a reordered sum, the device set-up against the host builder, one V-cycle against the numpy
restatement, solves on even grids against the odd grids one node larger, the refresh, and the context after the `odd`
refusal.

Shapes of the transfer test: the smallest on which the branches of an even halved side can go wrong -- 4 x 4 (-> 3 x 3:
the last coarse node and the clamp at 0 meet in one direction), 6 x 5 and 5 x 6 (one even side, one odd), 8 x 3 (x halves,
y does not), 4 x 2, 4 x 5 x 6 and 6 x 4 x 3, and 6 x 6 whose level 1 has the even side 4 again."""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest
import scipy.sparse as sp

import saddle_point_petsc_amd as S
from test_gpu_mg_grid import _close, _ctx, _export, _ordered_sum, _scipy
from test_mg_sides_cpu import hierarchy_mats, level_dims, prolong_ref, vcycle_ref

pytestmark = pytest.mark.gpu
SPK_ERR_UNSUPPORTED = -6
U = 2.0 ** -53


# ---- 1. the transfer kernels alone ---------------------------------------------------------------------------------------------
SHAPES = [(4, 4, 1), (6, 5, 1), (5, 6, 1), (8, 3, 1), (4, 2, 1), (6, 6, 1), (4, 5, 6), (6, 4, 3)]


@functools.lru_cache(maxsize=None)
def _grid_operator(grid, bs):
    """an SPD operator with full bs x bs blocks on the node grid: (sum of the 1-D Laplacians + 0.1 I) (x) (I + ones / 4)"""
    T = lambda m: sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1]) if m > 1 else sp.csr_matrix((1, 1))
    I = sp.identity
    mx, my, mz = grid
    N = (sp.kron(I(mz), sp.kron(I(my), T(mx))) + sp.kron(I(mz), sp.kron(T(my), I(mx))) + sp.kron(T(mz), sp.kron(I(my), I(mx)))
         + 0.1 * I(mx * my * mz))
    M = sp.kron(N, np.eye(bs) + 0.25 * np.ones((bs, bs))).tocsr()
    M.sort_indices()
    return S.CSR(M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.copy(), M.shape[0])


@pytest.mark.parametrize("bs", [1, 2, 3])
@pytest.mark.parametrize("grid", SHAPES, ids=lambda g: "x".join(map(str, g)))
def test_transfer_kernels_add_in_the_stated_order(grid, bs):
    """Matrix-free: bit for bit the numpy loop over the Kronecker P of the rule (ascending column, from the first product).
    Stored (the CSR kernels on the device-built P and R): the products are exact, so n - 1 additions in another order stay
    within (n - 1) 2^-53 sum|terms| per entry -- n = 9 for the prolongation (eight parents and y), n = 27 for the
    restriction.  The device-built P is the Kronecker product byte for byte."""
    A = _grid_operator(grid, bs)
    rng = np.random.default_rng(100 * bs + sum(grid))
    pad = 37
    with _ctx(A, amg=dict(coarsening="grid", grid=grid, sides="any", block_size=bs, coarse_eq_limit=1, setup="device")) as c:
        info = c.amg_info()
        dims = level_dims(grid, bs, coarse_eq_limit=1)
        assert info["sides"] == S.AMG_SIDES_ANY and info["dims"] == dims and info["levels"] >= 2
        if grid == (6, 6, 1):
            assert dims[1] == (4, 4, 1) and dims[2] == (3, 3, 1)
        for l in range(info["levels"] - 1):
            nf, nc = info["rows"][l], info["rows"][l + 1]
            P = prolong_ref(dims[l], bs)
            R = P.T.tocsr()
            R.sort_indices()
            assert P.shape == (nf, nc)
            rp, ci, v, _ = c.amg_level(l, S.AMG_PROLONG)
            assert (rp.tobytes(), ci.tobytes(), v.tobytes()) == (P.indptr.astype(np.int32).tobytes(), P.indices.astype(np.int32).tobytes(),
                                                                P.data.tobytes()), f"device-built P of level {l}"
            e, y, b, t = rng.standard_normal(nc), rng.standard_normal(nf + pad), rng.standard_normal(nf + pad), rng.standard_normal(nf + pad)
            s, tot = _ordered_sum(P, e)
            ref = y[:nf] + s
            out = c.debug_amg_transfer(l, "prolong", e, y)
            assert out[:nf].tobytes() == ref.tobytes(), f"prolongation of level {l} {dims[l]}"
            assert out[nf:].tobytes() == y[nf:].tobytes()
            st = c.debug_amg_transfer(l, "prolong", e, y, stored=True)
            assert np.all(np.abs(st[:nf] - ref) <= 8 * U * (tot + np.abs(y[:nf]))), f"stored prolongation of level {l}"
            assert st[nf:].tobytes() == y[nf:].tobytes()
            ref, tot = _ordered_sum(R, b[:nf] - t[:nf])
            assert int(np.diff(R.indptr).max()) <= 27
            out = c.debug_amg_transfer(l, "restrict", b, t)
            assert out.shape == (nc,) and out.tobytes() == ref.tobytes(), f"restriction of level {l} {dims[l]}"
            st = c.debug_amg_transfer(l, "restrict", b, t, stored=True)
            assert np.all(np.abs(st - ref) <= 26 * U * tot), f"stored restriction of level {l}"


# ---- 2. the device route against the host route -------------------------------------------------------------------------
@pytest.mark.parametrize("grid,bs", [((64, 48, 1), 2), ((6, 4, 8), 3)], ids=["64x48", "6x4x8"])
def test_device_setup_is_the_host_builds(grid, bs):
    """the bars of test_gpu_mg_grid.test_device_setup_is_the_host_builds: P byte for byte, A_l and D^-1 to 1e-12 of the
    largest entry, lambda_max to 1e-12 relative, the coarse inverse to 1e-10"""
    A = (S.AssembleOperator_Laplace3D(*grid) if grid[2] > 1 else S.AssembleOperator_Laplace(grid[0], grid[1]))[0]
    amg = dict(coarsening="grid", grid=grid, sides="any", coarse_eq_limit=10)
    with _ctx(A, amg=dict(amg, setup="device")) as c:
        di = c.amg_info()
        dev = _export(c.amg_level, di)
    h = S.AmgHierarchy(A, **amg)
    hi = h.info()
    host = _export(h.matrix, hi)
    h.close()
    assert di["setup"] == S.AMG_SETUP_DEVICE and di["sides"] == hi["sides"] == S.AMG_SIDES_ANY and di["block_size"] == bs
    assert di["dims"] == hi["dims"] == level_dims(grid, bs) and di["levels"] >= 3
    assert di["rows"] == hi["rows"] and di["nnz"] == hi["nnz"]
    for l in range(di["levels"] - 1):
        for a, b in zip(dev["P"][l][:3], host["P"][l][:3]):
            assert a.tobytes() == b.tobytes(), f"P_{l}"
        assert dev["P"][l][3] == host["P"][l][3]
        rel = abs(di["lambda_max"][l] - hi["lambda_max"][l]) / hi["lambda_max"][l]
        print(f"lambda_max[{l}]: relative {rel:.3e} off the host's")
        assert rel <= 1e-12
    for l in range(di["levels"]):
        assert np.array_equal(dev["A"][l][0], host["A"][l][0]) and np.array_equal(dev["A"][l][1], host["A"][l][1]), f"pattern of A_{l}"
        _close(dev["A"][l][2], host["A"][l][2], 1e-12, f"A_{l}")
        dd, dh = (sp.csr_matrix((m[2], m[1], m[0]), shape=m[3]).diagonal() for m in (dev["A"][l], host["A"][l]))
        _close(1.0 / dd, 1.0 / dh, 1e-12, f"D^-1 of level {l}")
    _close(dev["cinv"], host["cinv"], 1e-10, "coarse inverse")


# ---- 3. one V-cycle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transfer", ["matrixfree", "stored"])
def test_one_vcycle_matches_numpy(transfer):
    """the tolerance of test_gpu_mg_grid.test_one_vcycle_matches_numpy; two applications give the same bits"""
    A = S.AssembleOperator_Laplace(64, 48)[0]
    x = np.random.default_rng(3).standard_normal(A.nrows)
    with _ctx(A, amg=dict(coarsening="grid", grid=(64, 48), sides="any", transfer=transfer)) as c:
        info = c.amg_info()
        y = c.pc_apply(x)
        y2 = c.pc_apply(x)
        mats = hierarchy_mats(c.amg_level, info)
    assert info["dims"][:3] == [(64, 48, 1), (33, 25, 1), (17, 13, 1)] and info["sides"] == S.AMG_SIDES_ANY
    assert y.tobytes() == y2.tobytes()
    ref = vcycle_ref(*mats, info["lambda_max"], x)
    err = np.linalg.norm(y - ref) / np.linalg.norm(ref)
    print(f"64x48 {transfer}: V-cycle {err:.3e} off numpy (bound 1e-12)")
    assert err <= 1e-12


# ---- 4. solves to rtol 1e-8, the true residual recomputed in numpy -----------------------------------------------------
def _solve_its(A, f, amg):
    its = {}
    Asp = _scipy(A)
    with _ctx(A, amg=amg) as c:
        info = c.amg_info()
        for ksp in ("fgmres", "pipecg"):   # (FGMRES restarts at its default of 30)
            x, r = getattr(c, ksp)(f, rtol=1e-8, max_it=200)
            res = np.linalg.norm(f - Asp @ x) / np.linalg.norm(f)
            print(f"{amg['grid']} {amg.get('sides', 'odd')} {ksp}: {r['its']} iterations, {info['levels']} levels, true residual {res:.2e}")
            assert r["reason"] == 2 and res <= 2e-8   # the true residual confirms the recurrence's
            its[ksp] = r["its"]
    return its


@pytest.mark.parametrize("m", [64, 128])
def test_even_squares_solve_like_the_odd_ones(m):
    even = _solve_its(*S.AssembleOperator_Laplace(m, m), dict(coarsening="grid", grid=(m, m), sides="any"))
    odd = _solve_its(*S.AssembleOperator_Laplace(m + 1, m + 1), dict(coarsening="grid", grid=(m + 1, m + 1)))
    for ksp in ("fgmres", "pipecg"):
        assert even[ksp] <= odd[ksp] + 1, (even, odd)


def test_even_cube_solves_like_the_odd_one():
    even = _solve_its(*S.AssembleOperator_Laplace3D(16, 16, 16), dict(coarsening="grid", grid=(16, 16, 16), sides="any"))
    odd = _solve_its(*S.AssembleOperator_Laplace3D(17, 17, 17), dict(coarsening="grid", grid=(17, 17, 17)))
    for ksp in ("fgmres", "pipecg"):
        assert even[ksp] <= odd[ksp] + 1, (even, odd)


def test_saddle_system_with_the_exact_schur_complement():
    A, f = S.AssembleOperator_Laplace(64, 64)
    B, g = S.AssembleOperator_Constraints(64, 64)
    rhs = np.concatenate([f, g])
    Bsp = sp.csr_matrix((B.val, B.colidx, B.rowptr), shape=(B.nrows, A.nrows))
    K = sp.bmat([[_scipy(A), Bsp.T], [Bsp, None]], format="csr")
    with _ctx(A, B, S.PC_SCHUR, S.SCHUR_FULL, amg=dict(coarsening="grid", grid=(64, 64), sides="any"), schur_pre="full") as c:
        x, info = c.fgmres(rhs, rtol=1e-8, max_it=200)
    res = np.linalg.norm(rhs - K @ x) / np.linalg.norm(rhs)
    print(f"saddle 64^2 FULL + exact S + mg any: {info['its']} iterations, true residual {res:.2e}")
    assert info["reason"] == 2 and res <= 2e-8


def test_runner_and_facade_take_the_option():
    """saddle_point_run through the options alone, -ksp_view naming the rule and the chain; the -fieldsplit_0_ form through
    the facade under the exact Schur complement"""
    exe = os.path.join(os.path.dirname(S.LIB_PATH), "saddle_point_run")
    out = subprocess.run([exe, "-da_grid_x", "64", "-da_grid_y", "64", "-ksp_rtol", "1e-8", "-ksp_converged_reason", "-no_vtk",
                          "-saddle", "0", "-ksp_type", "fgmres", "-pc_type", "mg", "-pc_mg_galerkin", "-spk_mg_sides", "any", "-ksp_view"],
                         capture_output=True, text=True, timeout=120, cwd=tempfile.mkdtemp())
    assert out.returncode == 0, out.stdout + out.stderr
    assert "converged due to CONVERGED_RTOL" in out.stdout and "sides any" in out.stdout, out.stdout
    for l, g in enumerate((64, 33, 17, 9, 5)):
        assert f"level {l}: grid {g} x {g} x 1" in out.stdout, out.stdout
    A, f = S.AssembleOperator_Laplace(64, 64)
    B, g = S.AssembleOperator_Constraints(64, 64)
    rhs = np.concatenate([f, g])
    k = S.KSP()
    k.setOperators(A, B)
    k.setGrid(64, 64)
    k.setFromOptions("-ksp_type fgmres -ksp_rtol 1e-8 -pc_type fieldsplit -pc_fieldsplit_type schur "
                     "-pc_fieldsplit_schur_fact_type full -pc_fieldsplit_schur_precondition full -fieldsplit_0_ksp_type preonly "
                     "-fieldsplit_0_pc_type mg -fieldsplit_0_pc_mg_galerkin -fieldsplit_0_spk_mg_sides any")
    x = k.solve(rhs)
    assert k.getConvergedReason() == 2
    k.destroy()
    with _ctx(A, B, S.PC_SCHUR, S.SCHUR_FULL, amg=dict(coarsening="grid", grid=(64, 64), sides="any"), schur_pre="full") as c:
        xc, _ = c.fgmres(rhs, rtol=1e-8)
    assert np.array_equal(x, xc)


# ---- 5. the refresh -------------------------------------------------------------------------------------------------------------
def test_refresh_on_the_device_route():
    """kappa changed by the device assembler with reuse on: the set-up refreshes, P keeps its bytes, and the solve takes the
    iterations of a fresh build on the new operator"""
    mx, my = 64, 48
    kappa = 1.0 + np.random.default_rng(5).random((mx - 1) * (my - 1))
    A1, f1 = S.AssembleOperator_Laplace(mx, my, kappa=kappa)
    amg = dict(coarsening="grid", grid=(mx, my), sides="any", setup="device")
    with S.Context(0) as c:
        c.set_block_laplace(mx, my)
        c.pc_setup(S.PC_JACOBI, amg=amg, amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is False
        i0 = c.amg_info()
        P0 = [c.amg_level(l, S.AMG_PROLONG) for l in range(i0["levels"] - 1)]
        c.set_block_laplace(mx, my, kappa=kappa)
        c.pc_setup(S.PC_JACOBI, amg=amg, amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is True
        i1 = c.amg_info()
        P1 = [c.amg_level(l, S.AMG_PROLONG) for l in range(i1["levels"] - 1)]
        x, info = c.fgmres(f1, rtol=1e-8, max_it=200)
    assert i1["dims"] == i0["dims"] and i1["sides"] == S.AMG_SIDES_ANY and i1["lambda_max"] != i0["lambda_max"]
    for l, (p0, p1) in enumerate(zip(P0, P1)):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(p0[:3], p1[:3])), f"P_{l}"
    with _ctx(A1, amg=amg) as c:
        xf, finfo = c.fgmres(f1, rtol=1e-8, max_it=200)
    res = np.linalg.norm(f1 - _scipy(A1) @ x) / np.linalg.norm(f1)
    print(f"refreshed: {info['its']} iterations, fresh: {finfo['its']}, true residual {res:.2e}")
    assert info["reason"] == 2 and res <= 2e-8 and info["its"] == finfo["its"]


def test_another_side_rule_is_a_full_build():
    """33 x 10 builds under both rules (odd keeps the side of 10: 3 x 10 nodes stay below the dense limit)"""
    A = S.AssembleOperator_Laplace(33, 10)[0]
    amg = dict(coarsening="grid", grid=(33, 10), setup="device")
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        c.pc_setup(S.PC_JACOBI, amg=dict(amg, sides="any"), amg_reuse=True)
        c.pc_setup(S.PC_JACOBI, amg=dict(amg, sides="any"), amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is True and c.amg_info()["dims"][1] == (17, 6, 1)
        c.pc_setup(S.PC_JACOBI, amg=dict(amg, sides="odd"), amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is False and c.amg_info()["dims"][1] == (17, 10, 1) and c.amg_info()["sides"] == 0
        c.pc_setup(S.PC_JACOBI, amg=dict(amg, sides="any"), amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is False and c.amg_info()["dims"][1] == (17, 6, 1)


# ---- 6. the context after the refusal under `odd` ---------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["host", "device"])
def test_context_builds_under_any_after_the_odd_refusal(route):
    A, f = S.AssembleOperator_Laplace(64, 64)
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        with pytest.raises(S.SpkError) as e:
            c.pc_setup(S.PC_JACOBI, amg=dict(coarsening="grid", grid=(64, 64), setup=route))
        assert e.value.code == SPK_ERR_UNSUPPORTED and "side of 64 nodes" in str(e.value) and "-spk_mg_sides any" in str(e.value)
        c.pc_setup(S.PC_JACOBI, amg=dict(coarsening="grid", grid=(64, 64), setup=route, sides="any"))
        info = c.amg_info()
        x, r = c.fgmres(f, rtol=1e-8, max_it=200)
    assert info["dims"] == [(64, 64, 1), (33, 33, 1), (17, 17, 1), (9, 9, 1), (5, 5, 1)]
    assert r["reason"] == 2 and np.linalg.norm(f - _scipy(A) @ x) <= 2e-8 * np.linalg.norm(f)
