"""The refresh of the context's multigrid hierarchy (spk_pc_set_amg_reuse, pc_setup(..., amg_reuse=True)) on the device,
both set-up routes: a second set-up on new values of the same pattern refreshes, and the refreshed hierarchy is the
host refresh's (spk_amg_refresh_host, tests/test_amg_refresh_cpu.py) -- patterns exactly, values to the bar the device
build is held to; the V-cycle over it against numpy; there and back gives the build's bytes on the device route (the
summation order of the two numeric kernels); solves; everything that must fall back to a full build; the exact Schur
complement behind a refresh; determinism; one refresh beyond a workgroup per launch.

Grids 33 x 33, 24 x 17 (odd, non-square, rows that are no multiple of the 256-thread workgroup) and 64 x 64 (four
levels, several workgroups per launch on level 0); new values by the `scaled` perturbation of the CPU file."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import saddle_point_petsc_amd as S
from test_amg_cpu import hierarchy_mats, vcycle_ref
from test_amg_refresh_cpu import perturbed

pytestmark = pytest.mark.gpu
GRIDS = [(33, 33), (24, 17), (64, 64)]
ROUTES = ["host", "device"]
VCYCLE_TOL = 1e-12
# GMRES(30) iterations of the unperturbed operator in numpy (test_amg_refresh_cpu.CONVERGENCE); the CPU case allows the
# refreshed hierarchy + 2,
# FGMRES on the device one more
UNPERTURBED_ITS = {(33, 33): 10, (24, 17): 12, (64, 64): 12}


@functools.lru_cache(maxsize=None)
def _grid(nx, ny):
    """(A, f, values of the `scaled` perturbation) of one grid"""
    A, f = S.AssembleOperator_Laplace(nx, ny)
    return A, f, perturbed(A, "scaled", (nx, ny), 2)


def _with(A, val):
    return S.CSR(A.rowptr, A.colidx, np.ascontiguousarray(val), A.nrows)


def _scipy(A, val=None):
    return sp.csr_matrix((A.val if val is None else val, A.colidx, A.rowptr), shape=(A.nrows, A.nrows))


def _setup(c, route, reuse=True, pc=S.PC_JACOBI, **kw):
    c.pc_setup(pc, S.SCHUR_FULL, amg=dict(setup=route, **kw), amg_reuse=reuse)
    return c.amg_reuse_info()["refreshed"]


def _built_then_refreshed(A, val, route):
    """a context that built on A and refreshed to val, both with reuse on; the two reports checked"""
    c = S.Context(0)
    c.set_block(S.BLOCK_A00, A)
    assert _setup(c, route) is False
    c.set_block(S.BLOCK_A00, _with(A, val))
    assert _setup(c, route) is True
    r = c.amg_reuse_info()
    assert r["seconds"] > 0.0
    return c


def _export(get, info):
    L = info["levels"]
    return dict(A=[get(l, S.AMG_OP) for l in range(L)], P=[get(l, S.AMG_PROLONG) for l in range(L - 1)],
                T=[get(l, S.AMG_TENTATIVE) for l in range(L - 1)], cinv=get(L - 1, S.AMG_COARSE_INV)[2])


@functools.lru_cache(maxsize=None)
def _host_refreshed(nx, ny):
    """the host builder's hierarchy of the grid refreshed to the scaled values: (info, export), computed once"""
    A, _, val = _grid(nx, ny)
    h = S.AmgHierarchy(A)
    h.refresh(val)
    info = h.info()
    e = _export(h.matrix, info)
    h.close()
    return info, e


def _close(a, b, tol, what):
    err = np.abs(a - b).max() / np.abs(b).max()
    print(f"{what}: max deviation {err:.3e} of the largest entry (bound {tol:g})")
    assert err <= tol, what


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_second_setup_refreshes_to_the_host_refresh(nx, ny, route):
    A, _, val = _grid(nx, ny)
    hi, host = _host_refreshed(nx, ny)
    x = np.random.default_rng(nx).standard_normal(A.nrows)
    with _built_then_refreshed(A, val, route) as c:
        info = c.amg_info()
        dev = _export(c.amg_level, info)
        y = c.pc_apply(x)
        assert np.array_equal(y, c.pc_apply(x))
        mats = hierarchy_mats(c.amg_level, info)
    assert info["setup"] == (S.AMG_SETUP_DEVICE if route == "device" else S.AMG_SETUP_HOST)
    assert info["levels"] == hi["levels"] >= 2 and info["rows"] == hi["rows"] and info["nnz"] == hi["nnz"]
    assert np.array_equal(dev["A"][0][2], host["A"][0][2])             # level 0 holds the new values
    for l in range(info["levels"]):
        for k in (0, 1):
            assert np.array_equal(dev["A"][l][k], host["A"][l][k]), f"pattern of A_{l}"
        _close(dev["A"][l][2], host["A"][l][2], 1e-12, f"{nx}x{ny} {route} A_{l}")
    for l in range(info["levels"] - 1):
        for key in ("P", "T"):
            for k in (0, 1):
                assert np.array_equal(dev[key][l][k], host[key][l][k]), f"pattern of {key}_{l}"
        _close(dev["P"][l][2], host["P"][l][2], 1e-12, f"{nx}x{ny} {route} P_{l}")
        rel = abs(info["lambda_max"][l] - hi["lambda_max"][l]) / hi["lambda_max"][l]
        print(f"{nx}x{ny} {route} lambda_max[{l}]: relative {rel:.3e} off the host refresh's")
        assert rel <= 1e-12
    _close(dev["cinv"], host["cinv"], 1e-12 if route == "host" else 1e-10, f"{nx}x{ny} {route} coarse inverse")
    ref = vcycle_ref(*mats, info["lambda_max"], x)
    err = np.linalg.norm(y - ref) / np.linalg.norm(ref)
    print(f"{nx}x{ny} {route} V-cycle on the refreshed hierarchy: {err:.3e} off numpy (bound {VCYCLE_TOL:g})")
    assert err <= VCYCLE_TOL


@pytest.mark.parametrize("nx,ny", GRIDS)
def test_device_route_there_and_back_gives_the_builds_bytes(nx, ny):
    """the numeric kernels sum every entry in the order of the build's kernels: the same values, the same bits"""
    A, _, val = _grid(nx, ny)
    x = np.random.default_rng(ny).standard_normal(A.nrows)
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        assert _setup(c, "device") is False
        i0 = c.amg_info()
        e0, y0 = _export(c.amg_level, i0), c.pc_apply(x)
        c.set_block(S.BLOCK_A00, _with(A, val))
        assert _setup(c, "device") is True
        assert c.amg_info()["lambda_max"] != i0["lambda_max"] and not np.array_equal(c.pc_apply(x), y0)
        c.set_block(S.BLOCK_A00, A)
        assert _setup(c, "device") is True
        i1 = c.amg_info()
        e1, y1 = _export(c.amg_level, i1), c.pc_apply(x)
    assert i1["lambda_max"] == i0["lambda_max"] and i1["rows"] == i0["rows"] and i1["nnz"] == i0["nnz"]
    for key in ("A", "P", "T"):
        for l, (a, b) in enumerate(zip(e1[key], e0[key])):
            assert all(u.tobytes() == v.tobytes() for u, v in zip(a[:3], b[:3])), f"{key}_{l}"
    assert e1["cinv"].tobytes() == e0["cinv"].tobytes()
    assert y1.tobytes() == y0.tobytes()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("factor", [2.0, 0.125])
def test_a_power_of_two_rescales_the_hierarchy_exactly(factor, route):
    """The refresh runs the Lanczos and the coarse Cholesky on the operator scaled back to the binade it was built in:
    lambda_max keeps its bytes, every A_l and the V-cycle scale exactly (64 x 64: several workgroups in the sum of |D^-1|)."""
    A, _, _ = _grid(64, 64)
    x = np.random.default_rng(64).standard_normal(A.nrows)
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        assert _setup(c, route) is False
        i0 = c.amg_info()
        e0, y0 = _export(c.amg_level, i0), c.pc_apply(x)
        c.set_block(S.BLOCK_A00, _with(A, A.val * factor))
        assert _setup(c, route) is True
        i1 = c.amg_info()
        e1, y1 = _export(c.amg_level, i1), c.pc_apply(x)
    assert i1["lambda_max"] == i0["lambda_max"]
    for l, (a, b) in enumerate(zip(e1["A"], e0["A"])):
        assert a[2].tobytes() == (factor * b[2]).tobytes(), f"A_{l}"
    assert e1["cinv"].tobytes() == (e0["cinv"] / factor).tobytes()
    assert y1.tobytes() == (y0 / factor).tobytes()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_fgmres_on_the_new_operator_with_the_refreshed_hierarchy(nx, ny, route):
    A, f, val = _grid(nx, ny)
    with _built_then_refreshed(A, val, route) as c:
        x, info = c.fgmres(f, rtol=1e-8, max_it=200)
    xd = spl.spsolve(_scipy(A, val).tocsc(), f)
    bound = UNPERTURBED_ITS[(nx, ny)] + 2 + 1
    print(f"{nx}x{ny} {route}: {info['its']} iterations on the refreshed hierarchy (bound {bound})")
    assert info["reason"] == 2
    assert np.linalg.norm(x - xd) <= 1e-8 * np.linalg.norm(xd)
    assert info["its"] <= bound


def _one_more_entry_per_row(A):
    """the same matrix with one explicit zero added to every row, columns sorted: n_local stays, the pattern does not"""
    n = A.nrows
    rp, ci, v = [0], [], []
    for i in range(n):
        cols = A.colidx[A.rowptr[i]:A.rowptr[i + 1]]
        extra = (i + n // 2) % n
        while extra in cols:
            extra = (extra + 1) % n
        c = np.concatenate([cols, [extra]])
        w = np.concatenate([A.val[A.rowptr[i]:A.rowptr[i + 1]], [0.0]])
        o = np.argsort(c, kind="stable")
        ci.append(c[o]); v.append(w[o]); rp.append(rp[-1] + len(c))
    return S.CSR(np.array(rp, np.int32), np.concatenate(ci).astype(np.int32), np.concatenate(v), n)


def _columns_reversed(A):
    """the same matrix, the same nnz, every row stored in descending column order"""
    ci, v = A.colidx.copy(), A.val.copy()
    for i in range(A.nrows):
        k0, k1 = A.rowptr[i], A.rowptr[i + 1]
        ci[k0:k1], v[k0:k1] = ci[k0:k1][::-1], v[k0:k1][::-1]
    return S.CSR(A.rowptr.copy(), ci, v, A.nrows)


def _solves(c, Asp, f):
    x, info = c.fgmres(f, rtol=1e-8, max_it=300)
    xd = spl.spsolve(Asp.tocsc(), f)
    return info["reason"] == 2 and np.linalg.norm(x - xd) <= 1e-8 * np.linalg.norm(xd)


@pytest.mark.parametrize("route", ROUTES)
def test_what_is_not_a_refresh_is_a_full_build(route):
    A, f, val = _grid(33, 33)
    Anew, Aspnew = _with(A, val), _scipy(A, val)
    # reuse off: never a refresh, and a hierarchy built with reuse off is none to refresh
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        assert _setup(c, route, reuse=False) is False
        c.set_block(S.BLOCK_A00, Anew)
        assert _setup(c, route, reuse=False) is False and _solves(c, Aspnew, f)
        c.set_block(S.BLOCK_A00, A)
        assert _setup(c, route, reuse=True) is False and _solves(c, _scipy(A), f)
        c.set_block(S.BLOCK_A00, Anew)
        assert _setup(c, route, reuse=True) is True       # (that one was built with reuse on)
        c.set_block(S.BLOCK_A00, A)
        assert _setup(c, route, reuse=False) is False     # off again: the pattern copy is gone ...
        c.set_block(S.BLOCK_A00, Anew)
        assert _setup(c, route, reuse=True) is False and _solves(c, Aspnew, f)   # ... and with it the refresh
    # other options
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        assert _setup(c, route) is False
        c.set_block(S.BLOCK_A00, Anew)
        assert _setup(c, route, smooth_its=3) is False and _solves(c, Aspnew, f)
        assert len(c.amg_level(0, S.AMG_PROLONG)[2]) > 0
        c.set_block(S.BLOCK_A00, A)
        assert _setup(c, "host" if route == "device" else "device", smooth_its=3) is False      # the other route
    # one more stored entry per row; the same entries in another column order
    for other in (_one_more_entry_per_row(Anew), _columns_reversed(Anew)):
        with S.Context(0) as c:
            c.set_block(S.BLOCK_A00, A)
            assert _setup(c, route) is False
            c.set_block(S.BLOCK_A00, other)
            assert _setup(c, route) is False and _solves(c, Aspnew, f)
            c.set_block(S.BLOCK_A00, other)
            assert _setup(c, route) is True and _solves(c, Aspnew, f)   # (its own pattern again: a refresh)
    # another grid size
    B, fb, _ = _grid(24, 17)
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        assert _setup(c, route) is False
        c.set_block(S.BLOCK_A00, B)
        assert _setup(c, route) is False and _solves(c, _scipy(B), fb)
        assert c.amg_info()["rows"][0] == B.nrows


@pytest.mark.parametrize("route", ROUTES)
def test_exact_schur_complement_behind_a_refresh(route):
    """33 x 33 saddle system, schur_pre="full", FULL: W, S and the factor come from the refreshed V-cycle"""
    A, f, val = _grid(33, 33)
    B, g = S.AssembleOperator_Constraints(33, 33)
    Bd = sp.csr_matrix((B.val, B.colidx, B.rowptr), shape=(B.nrows, B.ncols)).toarray()
    n, m = A.nrows, B.nrows
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        c.set_block(S.BLOCK_A10, B)
        c.pc_setup(S.PC_SCHUR, S.SCHUR_FULL, amg=dict(setup=route), schur_pre="full", amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is False
        S_built = c.schur_matrix()
        c.set_block(S.BLOCK_A00, _with(A, val))
        c.pc_setup(S.PC_SCHUR, S.SCHUR_FULL, amg=dict(setup=route), schur_pre="full", amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is True
        info = c.amg_info()
        mats = hierarchy_mats(c.amg_level, info)
        Sd = c.schur_matrix()
        x = np.random.default_rng(n + 1).standard_normal(n + m)
        y = c.pc_apply(x)
        rhs = np.concatenate([f, g])
        xs, si = c.fgmres(rhs, rtol=1e-8, max_it=200)
        res = np.linalg.norm(rhs - c.mult(xs)) / np.linalg.norm(rhs)
    W = np.stack([vcycle_ref(*mats, info["lambda_max"], Bd[r]) for r in range(m)], axis=1)
    G = Bd @ W
    Sref = 0.5 * (G + G.T)
    err = np.linalg.norm(Sd - Sref) / np.linalg.norm(Sref)
    print(f"{route}: S behind the refresh {err:.3e} off numpy's B V B^T (bound {VCYCLE_TOL:g}); "
          f"off the built S by {np.linalg.norm(Sd - S_built) / np.linalg.norm(S_built):.2e}")
    assert err <= VCYCLE_TOL and np.array_equal(Sd, Sd.T)
    assert np.linalg.norm(Sd - S_built) > 1e-3 * np.linalg.norm(S_built)      # it is the new operator's S
    bar = VCYCLE_TOL * np.linalg.cond(Sref)
    scale = np.linalg.norm(np.abs(Bd) @ np.abs(y[:n]) + np.abs(x[n:]))
    miss = np.linalg.norm(Bd @ y[:n] - x[n:])
    print(f"{route}: B y0 - x1 = {miss / scale:.3e} of the scale (bar {bar:.3e})")
    assert miss <= bar * scale
    assert si["reason"] == 2 and res <= 1e-7


@pytest.mark.parametrize("route", ROUTES)
def test_two_identical_sequences_give_the_same_bytes(route):
    A, _, val = _grid(24, 17)
    x = np.random.default_rng(17).standard_normal(A.nrows)
    out = []
    for _ in range(2):
        with _built_then_refreshed(A, val, route) as c:
            out.append((c.pc_apply(x), c.amg_info()["lambda_max"]))
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1] == out[1][1]


@pytest.mark.parametrize("route", ROUTES)
def test_refresh_at_256_squared_converges(route):
    """the smallest grid whose level-0 launches of one row per thread take more than one workgroup on every kernel"""
    A, f = S.AssembleOperator_Laplace(256)
    val = perturbed(A, "scaled", (256, 256), 2)
    with _built_then_refreshed(A, val, route) as c:
        r = c.amg_reuse_info()
        x, info = c.fgmres(f, rtol=1e-8, max_it=200)
        res = np.linalg.norm(f - c.mult(x)) / np.linalg.norm(f)
    print(f"256^2 {route}: refresh {r['seconds']:.4f} s, {info['its']} iterations, true residual {res:.2e}")
    assert r["refreshed"] is True and info["reason"] == 2 and res <= 1e-7
