"""-spk_mg_galerkin stencil on the GPU: the device route's gather kernels against the host route byte for byte, the
refresh, one application against the numpy V-cycle, solves against the products route and the level-0 refusal."""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest
import scipy.sparse as sp

import saddle_point_petsc_amd as S
from test_gpu_mg_grid import _close, _ctx, _export, _scipy
from test_mg_cycle_cpu import cycle_ref
from test_mg_galerkin_cpu import SHAPES, _far_pair, _scaled, amg_kw, operator
from test_mg_sides_cpu import hierarchy_mats, vcycle_ref

pytestmark = pytest.mark.gpu
SPK_ERR_UNSUPPORTED = -6

# the shapes of the CPU tests, and 33x33: 2178 rows, no multiple of the workgroup, level 0 padded to the context's vector
# length (registered under the CPU module's helpers: its own parametrisations were fixed when it was imported)
SHAPES.setdefault("33x33", ((33, 33, 1), 2, "odd", lambda: S.AssembleOperator_Laplace(33, 33)[0]))
ALL = list(SHAPES)


def _bytes(ex):
    return ([tuple(a.tobytes() for a in m[:3]) for m in ex["A"][1:]], [tuple(a.tobytes() for a in m[:3]) for m in ex["P"]])


# ---- 1. device = host, byte for byte -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _both_routes(name):
    """two device stencil builds and the host stencil build of one shape, computed once"""
    A = operator(name)
    amg = amg_kw(name, galerkin="stencil")
    got = []
    for _ in range(2):
        with _ctx(A, amg=dict(amg, setup="device")) as c:
            di = c.amg_info()
            got.append((di, _export(c.amg_level, di)))
    h = S.AmgHierarchy(A, **amg)
    hi = h.info()
    host = _export(h.matrix, hi)
    h.close()
    return got[0], got[1], (hi, host)


@pytest.mark.parametrize("name", ALL)
def test_device_stencil_build_is_the_host_builds_bytes(name):
    (di, dev), (di2, dev2), (hi, host) = _both_routes(name)
    assert di["setup"] == S.AMG_SETUP_DEVICE and di["galerkin"] == hi["galerkin"] == S.AMG_GALERKIN_STENCIL
    assert di["levels"] == hi["levels"] >= 2 and di["dims"] == hi["dims"] and di["rows"] == hi["rows"] and di["nnz"] == hi["nnz"]
    assert di["operator_complexity"] == hi["operator_complexity"]
    assert _bytes(dev) == _bytes(host), f"{name}: a device-built A_l or P_l differs from the host's"
    for l in range(1, di["levels"]):   # D^-1 follows from the diagonal's bytes; the V-cycle test below reads the device's
        dd, dh = (sp.csr_matrix((m[2], m[1], m[0]), shape=m[3]).diagonal() for m in (dev["A"][l], host["A"][l]))
        assert dd.tobytes() == dh.tobytes()
    assert _bytes(dev2) == _bytes(dev) and dev2["cinv"].tobytes() == dev["cinv"].tobytes() and di2["lambda_max"] == di["lambda_max"]


@pytest.mark.parametrize("name", ALL)
def test_device_ritz_values_and_coarse_inverse_are_the_hosts(name):
    """lambda_max to 1e-12 relative and the coarse inverse to 1e-10 of its largest entry, the bars test_gpu_mg_grid.py holds
    the device route to, on levels whose bytes are the host's (the test above).  On a level >= 1 of at most
    SPK_AMG_MAX_COARSE rows the device route runs the host's Lanczos on a download of the level, so there lambda_max is
    the host's to the bit: five17x9's level 1 (9 x 5 nodes, 45 rows) was 4.79e-11 off with the device's Lanczos steps,
    under both routes -- 30 steps without reorthogonalisation on 45 rows lose orthogonality altogether (0.7) while the
    largest Ritz value is still 1.7e-7 from the eigenvalue, and it then follows the rounding of every sum."""
    (di, dev), _, (hi, host) = _both_routes(name)
    worst = 0.0
    for l in range(di["levels"] - 1):
        rel = abs(di["lambda_max"][l] - hi["lambda_max"][l]) / hi["lambda_max"][l]
        print(f"{name} lambda_max[{l}]: relative {rel:.3e} off the host's")
        worst = max(worst, rel)
        if 0 < l and di["rows"][l] <= 1024:
            assert di["lambda_max"][l] == hi["lambda_max"][l], f"{name}: lambda_max of level {l} is not the host's bits"
    _close(dev["cinv"], host["cinv"], 1e-10, f"{name} coarse inverse")
    assert worst <= 1e-12


# ---- 2. the device refresh ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["12x10any", "6x4x3any", "five17x9", "33x33"])
def test_device_refresh_runs_the_builds_kernel(name):
    A0, A1 = operator(name), _scaled(name)
    amg = amg_kw(name, galerkin="stencil", setup="device")
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A0)
        c.pc_setup(S.PC_JACOBI, amg=amg, amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is False
        i0 = c.amg_info()
        b0 = _export(c.amg_level, i0)
        c.pc_setup(S.PC_JACOBI, amg=amg, amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is True
        i1 = c.amg_info()
        b1 = _export(c.amg_level, i1)
        assert _bytes(b1) == _bytes(b0) and b1["cinv"].tobytes() == b0["cinv"].tobytes() and i1["lambda_max"] == i0["lambda_max"]
        c.set_block(S.BLOCK_A00, A1)
        c.pc_setup(S.PC_JACOBI, amg=amg, amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is True and c.amg_info()["galerkin"] == S.AMG_GALERKIN_STENCIL
        b2 = _export(c.amg_level, c.amg_info())
        c.pc_setup(S.PC_JACOBI, amg=dict(amg, galerkin="products"), amg_reuse=True)   # another route: a build
        assert c.amg_reuse_info()["refreshed"] is False and c.amg_info()["galerkin"] == S.AMG_GALERKIN_PRODUCTS
        c.pc_setup(S.PC_JACOBI, amg=amg, amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is False and c.amg_info()["galerkin"] == S.AMG_GALERKIN_STENCIL
    with _ctx(A1, amg=amg) as c:
        fresh = _export(c.amg_level, c.amg_info())
    assert _bytes(b2) == _bytes(fresh), f"{name}: the refreshed levels differ from a fresh device build"
    assert _bytes(b2)[1] == _bytes(b0)[1] and _bytes(b2)[0] != _bytes(b0)[0]


# ---- 3. one application ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,extra", [("33x33", dict(transfer="matrixfree")), ("33x33", dict(transfer="stored")),
                                        ("33x33", dict(cycle="w", tail="fused")), ("12x10any", dict(transfer="matrixfree")),
                                        ("9x9x5", dict(cycle="w", tail="fused"))],
                         ids=["33x33-matrixfree", "33x33-stored", "33x33-w-fused", "12x10any", "9x9x5-w-fused"])
def test_one_application_matches_numpy(name, extra):
    """the V-cycle bar of test_gpu_mg_grid (1e-12 relative) on the downloaded hierarchy, the W-cycle against the numpy
    recursion of test_mg_cycle_cpu; under the fused tail the kernel reads stencil-built levels and gives the launches' bits"""
    A = operator(name)
    x = np.random.default_rng(3).standard_normal(A.nrows)
    amg = amg_kw(name, galerkin="stencil", setup="device", **extra)
    with _ctx(A, amg=amg) as c:
        info = c.amg_info()
        y = c.pc_apply(x)
        y2 = c.pc_apply(x)
        mats = hierarchy_mats(c.amg_level, info)
    assert y.tobytes() == y2.tobytes() and info["galerkin"] == S.AMG_GALERKIN_STENCIL
    if extra.get("cycle") == "w":
        assert info["tail_first"] >= 1
        with _ctx(A, amg=dict(amg, tail="launches")) as c:
            yl = c.pc_apply(x)
        assert y.tobytes() == yl.tobytes(), "the fused tail on stencil-built levels differs from the launches"
        ref = cycle_ref(*mats, info["lambda_max"], x, 2)
    else:
        ref = vcycle_ref(*mats, info["lambda_max"], x)
    err = np.linalg.norm(y - ref) / np.linalg.norm(ref)
    print(f"{name} {extra}: V-cycle {err:.3e} off numpy (bound 1e-12)")
    assert err <= 1e-12


# ---- 4. solves ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["33x33", "12x10any", "9x9x5"])
def test_k_equals_a_solves_like_the_products_route(name):
    grid = SHAPES[name][0]
    A, f = S.AssembleOperator_Laplace3D(*grid) if grid[2] > 1 else S.AssembleOperator_Laplace(grid[0], grid[1])
    Asp = _scipy(A)
    its = {}
    for route in ("stencil", "products"):
        with _ctx(A, amg=amg_kw(name, galerkin=route, setup="device")) as c:
            for ksp in ("fgmres", "pipecg"):
                x, info = getattr(c, ksp)(f, rtol=1e-8, max_it=200)
                res = np.linalg.norm(f - Asp @ x) / np.linalg.norm(f)
                print(f"{name} {route} {ksp}: {info['its']} iterations, true residual {res:.2e}")
                assert info["reason"] == 2 and res <= 2e-8
                its[route, ksp] = info["its"]
    for ksp in ("fgmres", "pipecg"):
        assert abs(its["stencil", ksp] - its["products", ksp]) <= 1, its


def test_saddle_system_with_the_exact_schur_complement():
    A, f = S.AssembleOperator_Laplace(33, 33)
    B, g = S.AssembleOperator_Constraints(33, 33)
    rhs = np.concatenate([f, g])
    Bsp = sp.csr_matrix((B.val, B.colidx, B.rowptr), shape=(B.nrows, A.nrows))
    K = sp.bmat([[_scipy(A), Bsp.T], [Bsp, None]], format="csr")
    its = {}
    for route in ("stencil", "products"):
        with _ctx(A, B, S.PC_SCHUR, S.SCHUR_FULL, amg=dict(coarsening="grid", grid=(33, 33), galerkin=route, setup="device"), schur_pre="full") as c:
            x, info = c.fgmres(rhs, rtol=1e-8, max_it=200)
        res = np.linalg.norm(rhs - K @ x) / np.linalg.norm(rhs)
        print(f"saddle 33^2 FULL + exact S + mg {route}: {info['its']} iterations, true residual {res:.2e}")
        assert info["reason"] == 2 and res <= 2e-8
        its[route] = info["its"]
    assert abs(its["stencil"] - its["products"]) <= 1, its


def test_runner_takes_the_option_and_ksp_view_names_it():
    exe = os.path.join(os.path.dirname(S.LIB_PATH), "saddle_point_run")
    out = subprocess.run([exe, "-da_grid_x", "33", "-da_grid_y", "33", "-ksp_rtol", "1e-8", "-ksp_converged_reason", "-no_vtk",
                          "-saddle", "0", "-ksp_type", "fgmres", "-pc_type", "mg", "-pc_mg_galerkin", "-spk_mg_galerkin", "stencil",
                          "-spk_gamg_setup", "device", "-ksp_view"], capture_output=True, text=True, timeout=120, cwd=tempfile.mkdtemp())
    assert out.returncode == 0, out.stdout + out.stderr
    assert "converged due to CONVERGED_RTOL" in out.stdout and "(-spk_mg_galerkin stencil)" in out.stdout, out.stdout


# ---- 5. the refusal ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["host", "device"])
def test_an_entry_outside_the_stencil_is_refused_and_the_context_stays_usable(route):
    A = _far_pair()
    f = np.random.default_rng(5).standard_normal(A.nrows)
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        with pytest.raises(S.SpkError) as e:
            c.pc_setup(S.PC_JACOBI, amg=amg_kw("five17x9", galerkin="stencil", setup=route))
        assert e.value.code == SPK_ERR_UNSUPPORTED
        assert "row 20, column 22" in str(e.value) and "-spk_mg_galerkin products" in str(e.value), str(e.value)
        c.pc_setup(S.PC_JACOBI, amg=amg_kw("five17x9", galerkin="products", setup=route))
        assert c.amg_info()["galerkin"] == S.AMG_GALERKIN_PRODUCTS
        x, r = c.fgmres(f, rtol=1e-8, max_it=200)
    assert r["reason"] == 2 and np.linalg.norm(f - _scipy(A) @ x) <= 2e-8 * np.linalg.norm(f)
