"""The smoothed-aggregation multigrid hierarchy (-pc_type gamg) without a GPU, through the host-only builder
(spk_amg_build_host): aggregates, the tentative prolongator, the Galerkin coarse operators, the stopping rule,
determinism, the Lanczos estimates against eigsh; the KSP facade's gamg options and refusals.  vcycle_ref is the
numpy restatement of one V-cycle that test_gpu_amg holds the device to."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import saddle_point_petsc_amd as S
from saddle_point_petsc_amd._lib import SpkError

SPK_ERR_ARG, SPK_ERR_UNSUPPORTED = -1, -6


def to_sp(m):
    rp, ci, v, shape = m
    return sp.csr_matrix((v, ci, rp), shape=shape)


def laplace(n):
    A, f = S.AssembleOperator_Laplace(n)
    return A, f, sp.csr_matrix((A.val, A.colidx, A.rowptr), shape=(A.nrows, A.nrows))


def hierarchy_mats(get, info):
    """A_l, P_l and the coarse inverse through a getter get(level, which) -> (rowptr, colidx, val, shape)."""
    L = info["levels"]
    A = [to_sp(get(l, S.AMG_OP)) for l in range(L)]
    P = [to_sp(get(l, S.AMG_PROLONG)) for l in range(L - 1)]
    Ci = to_sp(get(L - 1, S.AMG_COARSE_INV)).toarray()
    return A, P, Ci


def vcycle_ref(A, P, Ci, lam, b, smoother="chebyshev", smooth_its=2, esteig=(0, 0.1, 0, 1.1), richardson_scale=1.0):
    """One V-cycle as spk_amg_cycle.cpp / spk_k_amg.hip run it: nu steps y+ = y + alpha D^-1 (b - A y) + beta (y - y-) from
    zero, residual restricted by P^T, recursion, y += P e, nu steps from y; the coarsest level y = C b.  Chebyshev
    coefficients of Saad Alg. 12.1 over [b lmax, d lmax] (a and c multiply the smallest Ritz value, 0 by default)."""
    L = len(A)
    dinv = []
    for a in A:
        d = a.diagonal()
        dinv.append(1.0 / np.where(d == 0.0, 1.0, d))
    coef = []
    for l in range(L - 1):
        if smoother == "chebyshev":
            lo, hi = esteig[1] * lam[l], esteig[3] * lam[l]
            th, de = 0.5 * (hi + lo), 0.5 * (hi - lo)
            sg = th / de
            rho = 1.0 / sg
            al, be = [1.0 / th], [0.0]
            for _ in range(1, smooth_its):
                rn = 1.0 / (2.0 * sg - rho)
                al.append(2.0 * rn / de)
                be.append(rn * rho)
                rho = rn
        else:
            al, be = [richardson_scale] * smooth_its, [0.0] * smooth_its
        coef.append((al, be))

    def smooth(l, bb, y):
        prev = None
        for al, be in zip(*coef[l]):
            if y is None:
                yn = al * (dinv[l] * bb)
            else:
                yn = y + al * (dinv[l] * (bb - A[l] @ y))
                if be != 0.0:
                    yn = yn + be * (y - (prev if prev is not None else 0.0))
            prev, y = y, yn
        return y

    def rec(l, bb):
        if l == L - 1:
            return Ci @ bb
        y = smooth(l, bb, None)
        e = rec(l + 1, P[l].T @ (bb - A[l] @ y))
        return smooth(l, bb, y + P[l] @ e)

    return rec(0, np.asarray(b, np.float64))


def general_spd(n, seed):
    """A general (non-grid) symmetric strictly diagonally dominant operator: 1-7 negative off-diagonals per row before
    symmetrising, no block structure, no Dirichlet rows.  Returns the CSR for the product and the scipy matrix."""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for i in range(n):
        c = rng.choice(n, int(rng.integers(1, 8)), replace=False)
        c = c[c != i]
        rows += [i] * len(c); cols += list(c); vals += list(-0.3 * np.abs(rng.standard_normal(len(c))))
    O = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    O = O + O.T                                            # symmetric pattern, negative off-diagonals
    d = np.asarray(abs(O).sum(1)).ravel() + 0.05 + rng.random(n)   # strictly diagonally dominant
    A = (O + sp.diags(d)).tocsr(); A.sort_indices()
    return S.CSR(A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy(), n), A


def _grid(A):
    return A, sp.csr_matrix((A.val, A.colidx, A.rowptr), shape=(A.nrows, A.nrows))


# Operators off the square 2-D grid (test_gpu_offgrid.py runs the device on the same ones): name -> (builder of
# (CSR, scipy), builder options, block size the builder must report, whether Dirichlet (isolated) nodes exist)
OFFGRID_BUILT = {
    "cube_odd": (lambda: _grid(S.AssembleOperator_Laplace3D(9, 9, 11)[0]), {}, 3, True),
    "gen1001": (lambda: general_spd(1001, 1001), {}, 1, False),
    "odd33_bs1": (lambda: _grid(S.AssembleOperator_Laplace(33, 33)[0]), dict(block_size=1), 1, True),
    "strip": (lambda: _grid(S.AssembleOperator_Laplace(50, 7)[0]), {}, 2, True),
}


@pytest.fixture(scope="module", params=[16, 32, 64] + list(OFFGRID_BUILT))
def built(request):
    """(name, A, scipy A, hierarchy, block size expected, has isolated nodes)"""
    if isinstance(request.param, int):
        A, f, Asp = laplace(request.param)
        kw, bs, iso = {}, 2, True
    else:
        make, kw, bs, iso = OFFGRID_BUILT[request.param]
        A, Asp = make()
    h = S.AmgHierarchy(A, **kw)
    yield request.param, A, Asp, h, bs, iso
    h.close()


def _isolated_nodes(Asp, bs):
    """nodes whose off-diagonal blocks hold only zeros (the Dirichlet rows of MatZeroRowsColumns)"""
    C = Asp.tocoo()
    off = (C.row // bs != C.col // bs) & (C.data != 0.0)
    has = np.zeros(Asp.shape[0] // bs, bool)
    has[C.row[off] // bs] = True
    return ~has


def test_aggregates_cover_every_connected_node_once(built):
    _, A, Asp, h, bs, has_iso = built
    info = h.info()
    assert info["block_size"] == bs and info["levels"] >= 2
    agg = h.aggregates(0)
    assert len(agg) * bs == A.nrows
    iso = _isolated_nodes(Asp, bs)
    if has_iso:
        assert iso.any()                            # the Dirichlet nodes are there ...
    else:
        assert not iso.any()                        # (a general operator has none)
    assert np.all(agg[iso] == -1)                   # ... and lie in no aggregate
    assert np.all(agg[~iso] >= 0)                   # every other node lies in exactly one (one index per node)
    na = agg.max() + 1
    assert np.all(np.bincount(agg[agg >= 0], minlength=na) > 0)
    Pt = to_sp(h.matrix(0, S.AMG_TENTATIVE))
    assert Pt.shape == (A.nrows, bs * na)


def test_tentative_prolongator_is_orthonormal(built):
    h = built[3]
    for l in range(h.info()["levels"] - 1):
        Pt = to_sp(h.matrix(l, S.AMG_TENTATIVE))
        G = (Pt.T @ Pt).toarray()
        assert np.abs(G - np.eye(G.shape[0])).max() < 1e-14


def test_coarse_operators_are_galerkin_and_symmetric(built):
    h = built[3]
    info = h.info()
    for l in range(info["levels"] - 1):
        Al, P, Ac = (to_sp(h.matrix(l, S.AMG_OP)), to_sp(h.matrix(l, S.AMG_PROLONG)), to_sp(h.matrix(l + 1, S.AMG_OP)))
        ref = (P.T @ Al @ P).toarray()
        assert np.linalg.norm(Ac.toarray() - ref) <= 1e-13 * np.linalg.norm(ref)
        assert (Ac != Ac.T).nnz == 0
        assert Ac.shape[0] == info["rows"][l + 1] and Ac.nnz == info["nnz"][l + 1]


def test_lambda_max_from_below_within_ten_percent(built):
    h = built[3]
    info = h.info()
    for l in range(info["levels"] - 1):
        Al = to_sp(h.matrix(l, S.AMG_OP))
        d = Al.diagonal()
        s = sp.diags(1.0 / np.sqrt(np.where(d == 0.0, 1.0, d)))
        ev = spl.eigsh(s @ Al @ s, k=1, which="LA", return_eigenvectors=False, tol=1e-12)[0]
        lam = info["lambda_max"][l]
        assert lam <= ev * (1 + 1e-10) and lam >= 0.9 * ev, (l, lam, ev)


@pytest.mark.parametrize("limit", [50, 200])
def test_levels_stop_at_coarse_eq_limit(limit):
    A, _, _ = laplace(64)
    h = S.AmgHierarchy(A, coarse_eq_limit=limit)
    rows = h.info()["rows"]
    assert rows[-1] <= limit and all(r > limit for r in rows[:-1])
    h2 = S.AmgHierarchy(A, coarse_eq_limit=limit, max_levels=2)
    assert h2.info()["levels"] == 2


def test_one_level_hierarchy_and_block_sizes_that_do_not_divide():
    """Seven rows are below coarse_eq_limit: one level, only the dense coarse inverse.  A block size that does not
    divide the number of rows is refused, not rounded."""
    A7, A7sp = general_spd(7, 7)
    h = S.AmgHierarchy(A7)
    info = h.info()
    assert info["levels"] == 1 and info["rows"] == [7]
    Ci = to_sp(h.matrix(0, S.AMG_COARSE_INV)).toarray()
    assert np.abs(Ci @ A7sp.toarray() - np.eye(7)).max() < 1e-13
    h.close()
    A1001, _ = general_spd(1001, 1001)
    A700, _ = S.AssembleOperator_Laplace(50, 7)
    for A, bs in ((A1001, 2), (A700, 3)):
        assert A.nrows % bs
        with pytest.raises(SpkError) as e:
            S.AmgHierarchy(A, block_size=bs)
        assert e.value.code == SPK_ERR_ARG and "does not divide" in str(e.value)


def test_two_builds_are_byte_identical():
    A, _, _ = laplace(48)
    h1, h2 = S.AmgHierarchy(A), S.AmgHierarchy(A)
    i1, i2 = h1.info(), h2.info()
    assert i1["rows"] == i2["rows"] and i1["nnz"] == i2["nnz"] and i1["lambda_max"] == i2["lambda_max"]
    L = i1["levels"]
    for l in range(L):
        whichs = [S.AMG_OP] + ([S.AMG_PROLONG, S.AMG_TENTATIVE] if l + 1 < L else [S.AMG_COARSE_INV])
        for w in whichs:
            for a, b in zip(h1.matrix(l, w)[:3], h2.matrix(l, w)[:3]):
                assert a.tobytes() == b.tobytes()


def test_nsmooths_zero_keeps_the_tentative_prolongator():
    A, _, _ = laplace(32)
    h = S.AmgHierarchy(A, nsmooths=0)
    for a, b in zip(h.matrix(0, S.AMG_PROLONG)[:3], h.matrix(0, S.AMG_TENTATIVE)[:3]):
        assert np.array_equal(a, b)


def test_vcycle_ref_preconditions_gmres_mesh_independently():
    its = {}
    for n in (32, 64, 128):
        A, f, Asp = laplace(n)
        h = S.AmgHierarchy(A)
        info = h.info()
        mats = hierarchy_mats(h.matrix, info)
        M = spl.LinearOperator(Asp.shape, matvec=lambda r: vcycle_ref(*mats, info["lambda_max"], r))
        cnt = [0]
        x, rc = spl.gmres(Asp, f, M=M, rtol=1e-8, restart=30, callback=lambda r: cnt.__setitem__(0, cnt[0] + 1),
                          callback_type="pr_norm")
        assert rc == 0
        its[n] = cnt[0]
    assert max(its.values()) <= 25 and its[128] <= 2 * its[32], its


def test_host_builder_refusals():
    A, _, _ = laplace(64)
    with pytest.raises(SpkError) as e:
        S.AmgHierarchy(A, max_levels=1)        # 8192 equations on the coarsest level
    assert e.value.code == SPK_ERR_UNSUPPORTED and "coarsest" in str(e.value)
    for bad in (dict(max_levels=0), dict(nsmooths=-1), dict(smooth_its=0), dict(threshold=-1.0), dict(block_size=4),
                dict(esteig=(0, 1.1, 0, 0.1))):
        with pytest.raises(SpkError) as e:
            S.AmgHierarchy(A, **bad)
        assert e.value.code == SPK_ERR_ARG, bad


# ---- the KSP facade (no GPU: SetFromOptions and the option checks of SetUp run before any context exists) -------------
AMG_OPTS = ["-pc_gamg_threshold", "0.02", "-pc_gamg_agg_nsmooths", "0", "-pc_gamg_coarse_eq_limit", "120",
            "-pc_mg_levels", "5", "-mg_levels_ksp_type", "richardson", "-mg_levels_ksp_max_it", "3",
            "-mg_levels_ksp_richardson_scale", "0.6", "-mg_levels_ksp_chebyshev_esteig", "0,0.2,0,1.2",
            "-mg_levels_pc_type", "jacobi"]
AMG_READ = dict(threshold=0.02, nsmooths=0, coarse_eq_limit=120, max_levels=5, smoother=S.AMG_RICHARDSON, smooth_its=3,
                richardson_scale=0.6, esteig=(0.0, 0.2, 0.0, 1.2))


@pytest.mark.parametrize("prefix", ["", "-fieldsplit_0_"])
def test_facade_reads_back_every_gamg_option(prefix):
    k = S.KSP()
    opts = [o if not o.startswith("-") or not prefix else prefix + o[1:] for o in AMG_OPTS]
    pc = ["-pc_type", "gamg"] if not prefix else ["-pc_type", "fieldsplit", "-fieldsplit_0_ksp_type", "preonly",
                                                  "-fieldsplit_0_pc_type", "gamg"]
    k.setFromOptions(["-ksp_type", "fgmres"] + pc + opts)
    got, sel = k.getAMGOptions(fieldsplit0=bool(prefix))
    other, osel = k.getAMGOptions(fieldsplit0=not prefix)
    assert sel and not osel
    for key, v in AMG_READ.items():
        assert got[key] == v, key
    dflt = dict(threshold=0.0, nsmooths=1, coarse_eq_limit=50, max_levels=10, smoother=S.AMG_CHEBYSHEV, smooth_its=2,
                richardson_scale=1.0, esteig=(0.0, 0.1, 0.0, 1.1), block_size=0)
    for key, v in dflt.items():
        assert other[key] == v, key
    _, pct, _ = k.getOptions()
    assert pct == (S.PC_JACOBI if not prefix else S.PC_SCHUR)
    k.destroy()


def _setup_code(opts):
    k = S.KSP()
    try:
        k.setFromOptions(opts)
        k.setUp()
    except SpkError as e:
        return e.code, str(e)
    finally:
        k.destroy()
    return 0, ""


def test_facade_refusals_before_any_gpu_work():
    fs = ["-pc_type", "fieldsplit", "-fieldsplit_0_pc_type", "gamg"]
    code, msg = _setup_code(["-ksp_type", "minres", "-pc_type", "gamg"])
    assert code == SPK_ERR_UNSUPPORTED and "minres" in msg and "gamg" in msg
    code, msg = _setup_code(["-ksp_type", "minres"] + fs + ["-pc_fieldsplit_schur_fact_type", "diag"])
    assert code == SPK_ERR_UNSUPPORTED and "gamg" in msg
    code, msg = _setup_code(["-ksp_type", "fgmres"] + fs + ["-fieldsplit_0_ksp_type", "richardson", "-fieldsplit_0_ksp_max_it", "3"])
    assert code == SPK_ERR_UNSUPPORTED and "FP32" in msg
    code, msg = _setup_code(["-ksp_type", "fgmres", "-pc_type", "gamg", "-spk_inner_sweeps", "2"])
    assert code == SPK_ERR_UNSUPPORTED and "FP32" in msg


@pytest.mark.parametrize("opts,code", [
    (["-pc_gamg_threshold", "x"], SPK_ERR_ARG),
    (["-pc_gamg_threshold", "-0.5"], SPK_ERR_ARG),
    (["-pc_gamg_agg_nsmooths", "1.5"], SPK_ERR_ARG),
    (["-pc_mg_levels", "17"], SPK_ERR_ARG),
    (["-pc_gamg_coarse_eq_limit", "0"], SPK_ERR_ARG),
    (["-mg_levels_ksp_max_it"], SPK_ERR_ARG),
    (["-mg_levels_ksp_chebyshev_esteig", "0,0.1,0"], SPK_ERR_ARG),
    (["-mg_levels_ksp_chebyshev_esteig", "0,0.1,0,1.1,2"], SPK_ERR_ARG),
    (["-fieldsplit_0_mg_levels_ksp_richardson_scale", "0"], SPK_ERR_ARG),
    (["-mg_levels_ksp_type", "gmres"], SPK_ERR_UNSUPPORTED),
    (["-mg_levels_pc_type", "sor"], SPK_ERR_UNSUPPORTED),
    (["-mg_coarse_ksp_type", "preonly"], SPK_ERR_UNSUPPORTED),
    (["-fieldsplit_0_mg_levels_ksp_monitor"], SPK_ERR_UNSUPPORTED),
    (["-pc_gamg_type", "classical"], SPK_ERR_UNSUPPORTED),
    (["-fieldsplit_0_pc_type", "hypre"], SPK_ERR_UNSUPPORTED),
])
def test_facade_refuses_malformed_and_unknown_options(opts, code):
    k = S.KSP()
    with pytest.raises(SpkError) as e:
        k.setFromOptions(["-ksp_type", "fgmres", "-pc_type", "gamg"] + opts)
    assert e.value.code == code
    k.destroy()
