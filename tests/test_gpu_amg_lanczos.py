"""-spk_amg_lanczos resident on the GPU (include/spk.h, SPK_AMG_LANCZOS_RESIDENT): the Lanczos of the device set-up with its
scalars in a block on the device against the stepwise route -- the tridiagonal, lambda_max, every level, the coarse
inverse and one application byte for byte; the read-back counts; the refresh; the refusals; and solves with equal
histories.  Equality throughout: the two routes reduce the same sums in the same order and apply the same scalar rule."""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import saddle_point_petsc_amd as S
from test_gpu_mg_grid import _ctx, _export, _scipy

pytestmark = pytest.mark.gpu
SPK_ERR_STATE, SPK_ERR_UNSUPPORTED = -3, -6


def _diagonal(n):
    i = np.arange(n, dtype=np.int32)
    return S.CSR(np.arange(n + 1, dtype=np.int32), i.copy(), 1.0 + (i % 5).astype(np.float64), n)


def _small():
    """3 x 3 nodes, bs 2, 18 rows that aggregate: no boundary rows (they would all be isolated), a kappa field, and a diagonal
    raised by 25 to 30 %, row by row -- positive definite, and D^-1 A has enough distinct eigenvalues for all 18 steps"""
    A = S.AssembleOperator_Laplace(3, 3, apply_bc=False, kappa=1.0 + np.random.default_rng(5).random(4))[0]
    rows = np.repeat(np.arange(A.nrows), np.diff(A.rowptr))
    v, d = A.val.copy(), rows == A.colidx
    v[d] *= 1.25 + 0.05 * rows[d] / 18.0
    return S.CSR(A.rowptr.copy(), A.colidx.copy(), v, A.nrows)


# name -> (operator, multigrid options, the rows of the first levels -- what the case is chosen for; the CPU module checks them
# with the host builder)
CASES = {
    "gamg33x33": (lambda: S.AssembleOperator_Laplace(33, 33)[0], dict(), [2178]),
    "mg33x17products": (lambda: S.AssembleOperator_Laplace(33, 17)[0],
                        dict(coarsening="grid", grid=(33, 17), coarse_eq_limit=10, galerkin="products"), [1122, 306]),
    "mg65x33stencil": (lambda: S.AssembleOperator_Laplace(65, 33)[0],   # level 1: 1122 rows, a ragged last workgroup
                       dict(coarsening="grid", grid=(65, 33), coarse_eq_limit=10, galerkin="stencil"), [4290, 1122, 306]),
    "mg129x129": (lambda: S.AssembleOperator_Laplace(129, 129)[0],      # many workgroups in the finish
                  dict(coarsening="grid", grid=(129, 129), coarse_eq_limit=10, galerkin="stencil"), [33282, 8450, 2178, 578]),
    "mg12x10any": (lambda: S.AssembleOperator_Laplace(12, 10)[0],
                   dict(coarsening="grid", grid=(12, 10), sides="any", coarse_eq_limit=10), [240, 84]),
    "mg9x9x5": (lambda: S.AssembleOperator_Laplace3D(9, 9, 5)[0],
                dict(coarsening="grid", grid=(9, 9, 5), block_size=3, coarse_eq_limit=10), [1215, 225]),
    "gamg3x3": (lambda: _small(), dict(coarse_eq_limit=4, block_size=2), [18, 2]),                               # kk = 18
    "diagonal9x9": (lambda: _diagonal(81), dict(coarsening="grid", grid=(9, 9), block_size=1, coarse_eq_limit=10, galerkin="products"),
                    [81, 25]),                                                                                   # stops at step 0
}
ALL = list(CASES)


@functools.lru_cache(maxsize=None)
def operator(name):
    return CASES[name][0]()


def _amg(name, **kw):
    return dict(CASES[name][1], setup="device", **kw)


def _on_host(amg, info, l):
    """DevRoute::ritz_on_host: the level's Lanczos runs on a download of it"""
    return amg.get("coarsening") == "grid" and amg.get("galerkin") == "stencil" and l > 0 and info["rows"][l] <= 1024


def _bytes(ex):
    return ([tuple(a.tobytes() for a in m[:3]) for m in ex["A"]], [tuple(a.tobytes() for a in m[:3]) for m in ex["P"]], ex["cinv"].tobytes())


@functools.lru_cache(maxsize=None)
def _built(name):
    """one build per route of a case, and on the stepwise context both hooks on every level: computed once, never changed"""
    A = operator(name)
    x = np.random.default_rng(11).standard_normal(A.nrows)
    out = {}
    for route in ("stepwise", "resident"):
        with _ctx(A, amg=_amg(name, lanczos=route)) as c:
            info = c.amg_info()
            out[route] = dict(info=info, bytes=_bytes(_export(c.amg_level, info)), y=c.pc_apply(x).tobytes())
            if route == "stepwise":
                out["hook"] = [(c.debug_amg_lanczos(l, resident=False), c.debug_amg_lanczos(l, resident=True))
                               for l in range(info["levels"] - 1)]
    return out


# ---- 1. the tridiagonal ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_tridiagonal_is_the_stepwise_routes_bits(name):
    b = _built(name)
    info = b["stepwise"]["info"]
    assert info["levels"] >= 2 and info["rows"][:len(CASES[name][2])] == CASES[name][2], info["rows"]
    for l, ((ss, sal, sbe), (rs, ral, rbe)) in enumerate(b["hook"]):
        print(f"{name} level {l} ({info['rows'][l]} rows): {ss} steps stepwise, {rs} resident; al[0] {sal[0]!r}")
        assert ss == rs and 1 <= ss <= min(30, info["rows"][l]), (name, l, ss, rs)
        assert len(sal) == len(sbe) == ss and sbe[0] == 0.0 and rbe[0] == 0.0
        assert sal.tobytes() == ral.tobytes(), f"{name} level {l}: al differs"
        assert sbe.tobytes() == rbe.tobytes(), f"{name} level {l}: be differs"
    steps0 = b["hook"][0][0][0]
    if name == "gamg3x3":
        assert steps0 == 18      # kk = n
    elif name == "diagonal9x9":
        assert steps0 == 1       # D^-1 A = I: the first norm is zero
    elif info["rows"][0] >= 240:
        assert steps0 == 30


# ---- 2. the hierarchy --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_hierarchy_is_the_stepwise_routes_bytes(name):
    b = _built(name)
    s, r = b["stepwise"], b["resident"]
    assert (s["info"]["lanczos"], r["info"]["lanczos"]) == (S.AMG_LANCZOS_STEPWISE, S.AMG_LANCZOS_RESIDENT)
    assert s["info"]["setup"] == r["info"]["setup"] == S.AMG_SETUP_DEVICE
    assert s["info"]["levels"] == r["info"]["levels"] and s["info"]["rows"] == r["info"]["rows"]
    for l, (a, c) in enumerate(zip(s["info"]["lambda_max"], r["info"]["lambda_max"])):
        assert a == c, f"{name}: lambda_max of level {l}: {a!r} stepwise, {c!r} resident"
    assert s["bytes"][0] == r["bytes"][0], f"{name}: an A_l differs"
    assert s["bytes"][1] == r["bytes"][1], f"{name}: a P_l differs"
    assert s["bytes"][2] == r["bytes"][2], f"{name}: the coarse inverse differs"
    assert s["y"] == r["y"], f"{name}: one application differs"


# ---- 3. the read-backs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_read_back_counts(name):
    b = _built(name)
    info, amg = b["stepwise"]["info"], CASES[name][1]
    host = [l for l in range(info["levels"] - 1) if _on_host(amg, info, l)]
    dev = [l for l in range(info["levels"] - 1) if l not in host]
    stepwise = sum(1 + 2 * b["hook"][l][0][0] for l in dev) + len(host)
    print(f"{name}: {len(dev)} levels on the device, {len(host)} downloaded; read-backs {b['stepwise']['info']['ritz_readbacks']} stepwise, "
          f"{b['resident']['info']['ritz_readbacks']} resident")
    assert b["resident"]["info"]["ritz_readbacks"] == len(dev) + len(host)
    assert b["stepwise"]["info"]["ritz_readbacks"] == stepwise
    if name == "mg129x129":
        assert len(dev) == 3 and len(host) >= 2


# ---- 4. the refresh ----------------------------------------------------------------------------------------------------
def _kappa(name):
    mx, my = (65, 33) if name == "mg65x33stencil" else (33, 33)
    return S.AssembleOperator_Laplace(mx, my, kappa=1.0 + np.random.default_rng(7).random((mx - 1) * (my - 1)))[0]


@pytest.mark.parametrize("name", ["mg65x33stencil", "gamg33x33"])
def test_refresh_under_the_resident_route(name):
    A0, A1 = operator(name), _kappa(name)
    A32 = S.CSR(A0.rowptr.copy(), A0.colidx.copy(), A0.val * 32.0, A0.nrows)
    assert np.array_equal(A0.colidx, A1.colidx) and not np.array_equal(A0.val, A1.val)
    amg = _amg(name, lanczos="resident")
    built = _built(name)["resident"]
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A0)
        c.pc_setup(S.PC_JACOBI, amg=amg, amg_reuse=True)
        i0 = c.amg_info()
        assert c.amg_reuse_info()["refreshed"] is False and i0["lanczos"] == 1
        assert _bytes(_export(c.amg_level, i0)) == built["bytes"] and i0["lambda_max"] == built["info"]["lambda_max"]
        c.pc_setup(S.PC_JACOBI, amg=amg, amg_reuse=True)   # unchanged values
        i1 = c.amg_info()
        assert c.amg_reuse_info()["refreshed"] is True and i1["lanczos"] == 1
        assert _bytes(_export(c.amg_level, i1)) == built["bytes"] and i1["lambda_max"] == i0["lambda_max"]
        assert i1["ritz_readbacks"] == i0["ritz_readbacks"] == built["info"]["ritz_readbacks"] == i0["levels"] - 1
        c.set_block(S.BLOCK_A00, A32)                      # a power of two: lambda_max to the bit
        c.pc_setup(S.PC_JACOBI, amg=amg, amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is True and c.amg_info()["lambda_max"] == i0["lambda_max"]
        c.set_block(S.BLOCK_A00, A1)                       # other values
        c.pc_setup(S.PC_JACOBI, amg=amg, amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is True
        lam_res = c.amg_info()["lambda_max"]
        c.pc_setup(S.PC_JACOBI, amg=dict(amg, lanczos="stepwise"), amg_reuse=True)   # the route alone changes: a build
        assert c.amg_reuse_info()["refreshed"] is False and c.amg_info()["lanczos"] == 0
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A0)
        c.pc_setup(S.PC_JACOBI, amg=dict(amg, lanczos="stepwise"), amg_reuse=True)
        c.set_block(S.BLOCK_A00, A1)
        c.pc_setup(S.PC_JACOBI, amg=dict(amg, lanczos="stepwise"), amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is True and c.amg_info()["lanczos"] == 0
        lam_step = c.amg_info()["lambda_max"]
    assert lam_res == lam_step and lam_res != i0["lambda_max"]


# ---- 5. the refusals ---------------------------------------------------------------------------------------------------
def test_refusals_on_a_context():
    A, f = S.AssembleOperator_Laplace(33, 33)
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        with pytest.raises(S.SpkError) as e:
            c.pc_setup(S.PC_JACOBI, amg=dict(lanczos="resident", setup="host"))
        assert e.value.code == SPK_ERR_UNSUPPORTED and "-spk_gamg_setup device" in str(e.value), str(e.value)
        with pytest.raises(S.SpkError) as e:
            c.pc_setup(S.PC_JACOBI, amg=dict(lanczos="resident"))   # host is the default
        assert e.value.code == SPK_ERR_UNSUPPORTED and "-spk_gamg_setup device" in str(e.value), str(e.value)
        c.pc_setup(S.PC_JACOBI, amg=dict(lanczos="resident", setup="device"))
        assert c.amg_info()["lanczos"] == 1
        x, r = c.fgmres(f, rtol=1e-8, max_it=200)
        assert r["reason"] == 2 and np.linalg.norm(f - _scipy(A) @ x) <= 2e-8 * np.linalg.norm(f)
        with pytest.raises(S.SpkError) as e:
            c.debug_amg_lanczos(c.amg_info()["levels"] - 1)
        assert e.value.code == -1
        c.pc_setup(S.PC_JACOBI, amg=dict(setup="host"))
        assert c.amg_info()["ritz_readbacks"] == 0 and c.amg_info()["lanczos"] == 0
        with pytest.raises(S.SpkError) as e:
            c.debug_amg_lanczos(0)
        assert e.value.code == SPK_ERR_STATE


def test_runner_takes_the_option_and_ksp_view_names_the_route():
    exe = os.path.join(os.path.dirname(S.LIB_PATH), "saddle_point_run")
    out = subprocess.run([exe, "-da_grid_x", "33", "-da_grid_y", "33", "-ksp_rtol", "1e-8", "-ksp_converged_reason", "-no_vtk",
                          "-saddle", "0", "-ksp_type", "fgmres", "-pc_type", "gamg", "-spk_gamg_setup", "device",
                          "-spk_amg_lanczos", "resident", "-ksp_view"], capture_output=True, text=True, timeout=120, cwd=tempfile.mkdtemp())
    assert out.returncode == 0, out.stdout + out.stderr
    assert "converged due to CONVERGED_RTOL" in out.stdout and "(-spk_amg_lanczos resident)" in out.stdout, out.stdout
    assert "2 read-backs" in out.stdout, out.stdout


# ---- 6. solves ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", ["mg", "gamg"])
def test_solves_have_equal_histories(pc):
    """by test 2 the two routes build the same preconditioner: equality, not a tolerance"""
    A, f = S.AssembleOperator_Laplace(65, 65)
    amg = dict(setup="device", **(dict(coarsening="grid", grid=(65, 65)) if pc == "mg" else {}))
    got = {}
    for route in ("stepwise", "resident"):
        with _ctx(A, amg=dict(amg, lanczos=route)) as c:
            x, r = c.fgmres(f, rtol=1e-8, max_it=200)
            assert r["reason"] == 2 and c.amg_info()["lanczos"] == (route == "resident")
            got[route] = (r["its"], r["history"].tobytes(), x.tobytes())
            print(f"{pc} {route}: {r['its']} iterations, {c.amg_info()['ritz_readbacks']} read-backs")
    assert got["stepwise"][0] == got["resident"][0]
    assert got["stepwise"][1] == got["resident"][1] and got["stepwise"][2] == got["resident"][2]
