"""Grid-coarsening multigrid (-pc_type mg, SPK_AMG_COARSEN_GRID) without a GPU, through the host-only builder: the
prolongators against the Kronecker product of the rule byte for byte, the level grids, the Galerkin operators,
determinism, what is ignored and what is refused, the iteration counts of the numpy V-cycle against the aggregation
hierarchy of the same builder, and the KSP facade's options and refusals."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import saddle_point_petsc_amd as S
from saddle_point_petsc_amd._lib import SpkError
from test_amg_cpu import hierarchy_mats, to_sp, vcycle_ref

SPK_ERR_ARG, SPK_ERR_STATE, SPK_ERR_UNSUPPORTED = -1, -3, -6


# ---- the rule, restated -------------------------------------------------------------------------------------------------
def halves(m):
    return m % 2 == 1 and m >= 5


def coarse_dims(d):
    return tuple((m + 1) // 2 if halves(m) else m for m in d)


def level_dims(d, bs, coarse_eq_limit=50, max_levels=10):
    """the node grid of every level: stop at n <= coarse_eq_limit, at max_levels, or when no direction halves"""
    out = [tuple(d)]
    while bs * int(np.prod(out[-1])) > coarse_eq_limit and len(out) < max_levels and coarse_dims(out[-1]) != out[-1]:
        out.append(coarse_dims(out[-1]))
    return out


def prolong_1d(m):
    """m fine nodes -> (m + 1) / 2: even i -> i / 2 (weight 1), odd i -> (i - 1) / 2 and (i + 1) / 2 (1/2 each); a
    direction that does not halve: the identity"""
    if not halves(m):
        return sp.identity(m, format="csr")
    P = sp.lil_matrix((m, (m + 1) // 2))
    for i in range(m):
        if i % 2 == 0:
            P[i, i // 2] = 1.0
        else:
            P[i, (i - 1) // 2] = P[i, (i + 1) // 2] = 0.5
    return P.tocsr()


def prolong_ref(d, bs):
    """P_z (x) P_y (x) P_x (x) I_bs as sorted CSR"""
    P = sp.kron(prolong_1d(d[2]), sp.kron(prolong_1d(d[1]), sp.kron(prolong_1d(d[0]), sp.identity(bs)))).tocsr()
    P.sum_duplicates()
    P.eliminate_zeros()   # (kron takes its block path for a dense right factor and keeps the zeros of I_bs)
    P.sort_indices()
    return P


def five_point(mx, my):
    """a user operator on a grid (one unknown per node, no Dirichlet rows): the 5-point Laplacian plus a shift"""
    T = lambda m: sp.diags([-np.ones(m - 1), 2.0 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])
    M = (sp.kron(sp.identity(my), T(mx)) + sp.kron(T(my), sp.identity(mx)) + 0.1 * sp.identity(mx * my)).tocsr()
    M.sort_indices()
    return S.CSR(M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.copy(), mx * my)


# name -> (operator, grid, bs, builder options).  coarse_eq_limit 10: the small grids coarsen to the end of the rule
CASES = {
    "17x17": (lambda: S.AssembleOperator_Laplace(17, 17)[0], (17, 17, 1), 2, {}),
    "33x9": (lambda: S.AssembleOperator_Laplace(33, 9)[0], (33, 9, 1), 2, {}),          # semi-coarsening
    "12x9": (lambda: S.AssembleOperator_Laplace(12, 9)[0], (12, 9, 1), 2, {}),          # x never halves
    "5x5": (lambda: S.AssembleOperator_Laplace(5, 5)[0], (5, 5, 1), 2, {}),
    "9x9x5": (lambda: S.AssembleOperator_Laplace3D(9, 9, 5)[0], (9, 9, 5), 3, {}),
    "user17x9": (lambda: five_point(17, 9), (17, 9, 1), 1, dict(block_size=1)),
}
EXPECT_DIMS = {"33x9": [(33, 9, 1), (17, 5, 1), (9, 3, 1), (5, 3, 1), (3, 3, 1)], "12x9": [(12, 9, 1), (12, 5, 1), (12, 3, 1)],
               "5x5": [(5, 5, 1), (3, 3, 1)], "9x9x5": [(9, 9, 5), (5, 5, 3), (3, 3, 3)]}


@functools.lru_cache(maxsize=None)
def _operator(name):
    return CASES[name][0]()


def _build(name, **kw):
    _, grid, _, opts = CASES[name]
    return S.AmgHierarchy(_operator(name), **dict(dict(opts, coarsening="grid", grid=grid, coarse_eq_limit=10), **kw))


@pytest.fixture(scope="module", params=list(CASES))
def built(request):
    h = _build(request.param)
    yield request.param, h
    h.close()


def test_prolongators_are_the_kronecker_product_byte_for_byte(built):
    name, h = built
    _, grid, bs, _ = CASES[name]
    info = h.info()
    dims = level_dims(grid, bs, coarse_eq_limit=10)
    assert info["coarsening"] == S.AMG_COARSEN_GRID and info["block_size"] == bs
    assert info["dims"] == dims and info["levels"] == len(dims) >= 2
    if name in EXPECT_DIMS:
        assert dims == EXPECT_DIMS[name]
    assert info["rows"] == [bs * int(np.prod(d)) for d in dims]
    for l in range(info["levels"] - 1):
        rp, ci, v, shape = h.matrix(l, S.AMG_PROLONG)
        ref = prolong_ref(dims[l], bs)
        assert shape == ref.shape == (info["rows"][l], info["rows"][l + 1])
        assert rp.tobytes() == ref.indptr.astype(np.int32).tobytes(), (name, l)
        assert ci.tobytes() == ref.indices.astype(np.int32).tobytes(), (name, l)
        assert v.tobytes() == ref.data.astype(np.float64).tobytes(), (name, l)
        assert set(np.unique(v)) <= {1.0, 0.5, 0.25, 0.125}


def test_coarse_operators_are_galerkin_and_exactly_symmetric(built):
    _, h = built
    info = h.info()
    for l in range(info["levels"] - 1):
        Al, P, Ac = (to_sp(h.matrix(l, S.AMG_OP)), to_sp(h.matrix(l, S.AMG_PROLONG)), to_sp(h.matrix(l + 1, S.AMG_OP)))
        G = (P.T @ Al @ P).toarray()
        ref = 0.5 * (G + G.T)
        assert np.linalg.norm(Ac.toarray() - ref) <= 1e-13 * np.linalg.norm(ref)
        assert (Ac != Ac.T).nnz == 0
        assert Ac.shape[0] == info["rows"][l + 1] and Ac.nnz == info["nnz"][l + 1]


def test_two_builds_are_byte_identical():
    h1, h2 = _build("33x9"), _build("33x9")
    i1, i2 = h1.info(), h2.info()
    assert i1["rows"] == i2["rows"] and i1["nnz"] == i2["nnz"] and i1["lambda_max"] == i2["lambda_max"] and i1["dims"] == i2["dims"]
    L = i1["levels"]
    for l in range(L):
        for w in [S.AMG_OP] + ([S.AMG_PROLONG] if l + 1 < L else [S.AMG_COARSE_INV]):
            for a, b in zip(h1.matrix(l, w)[:3], h2.matrix(l, w)[:3]):
                assert a.tobytes() == b.tobytes()


def test_nsmooths_and_threshold_are_ignored():
    h1, h2 = _build("17x17"), _build("17x17", nsmooths=0, threshold=0.3)
    i1, i2 = h1.info(), h2.info()
    assert i1["lambda_max"] == i2["lambda_max"] and i1["dims"] == i2["dims"]
    for l in range(i1["levels"]):
        for w in [S.AMG_OP] + ([S.AMG_PROLONG] if l + 1 < i1["levels"] else [S.AMG_COARSE_INV]):
            for a, b in zip(h1.matrix(l, w)[:3], h2.matrix(l, w)[:3]):
                assert a.tobytes() == b.tobytes()


def test_tentative_is_p_and_there_are_no_aggregates(built):
    _, h = built
    for l in range(h.info()["levels"] - 1):
        for a, b in zip(h.matrix(l, S.AMG_TENTATIVE)[:3], h.matrix(l, S.AMG_PROLONG)[:3]):
            assert a.tobytes() == b.tobytes()
    with pytest.raises(SpkError) as e:
        h.aggregates(0)
    assert e.value.code == SPK_ERR_UNSUPPORTED and "aggregates" in str(e.value)


@pytest.mark.parametrize("limit", [50, 1024])
def test_levels_stop_at_coarse_eq_limit(limit):
    A = S.AssembleOperator_Laplace(65, 65)[0]
    h = S.AmgHierarchy(A, coarsening="grid", grid=(65, 65), coarse_eq_limit=limit)
    info = h.info()
    assert info["dims"] == level_dims((65, 65, 1), 2, coarse_eq_limit=limit)
    assert info["rows"][-1] <= limit and all(r > limit for r in info["rows"][:-1])
    h.close()
    h2 = S.AmgHierarchy(A, coarsening="grid", grid=(65, 65), coarse_eq_limit=limit, max_levels=3)
    assert h2.info()["levels"] == 3 and h2.info()["dims"] == [(65, 65, 1), (33, 33, 1), (17, 17, 1)]
    h2.close()


def test_semi_coarsening_with_the_default_limit():
    h = _build("33x9", coarse_eq_limit=50)
    assert h.info()["dims"] == [(33, 9, 1), (17, 5, 1), (9, 3, 1), (5, 3, 1)]   # 30 equations: at most 50
    h.close()


def test_hierarchy_stops_when_no_direction_halves():
    h = _build("12x9", coarse_eq_limit=1)
    assert h.info()["dims"] == [(12, 9, 1), (12, 5, 1), (12, 3, 1)]   # 72 equations stay: below the dense limit
    h.close()


def test_refusals():
    A = S.AssembleOperator_Laplace(64, 64)[0]
    with pytest.raises(SpkError) as e:
        S.AmgHierarchy(A, coarsening="grid", grid=(64, 64))   # 63 elements per side: odd
    assert e.value.code == SPK_ERR_UNSUPPORTED and "coarsest" in str(e.value) and "side of 64 nodes" in str(e.value)
    A17 = _operator("17x17")
    for grid, what in (((17, 16), "544"), ((17, 17, 2), "1156"), ((9, 9, 3), "486")):
        with pytest.raises(SpkError) as e:
            S.AmgHierarchy(A17, coarsening="grid", grid=grid)
        assert e.value.code == SPK_ERR_ARG and "578" in str(e.value) and what in str(e.value), grid
    with pytest.raises(SpkError) as e:
        S.AmgHierarchy(A17, coarsening="grid", grid=(17, 17), block_size=1)   # 578 rows, 289 nodes of one unknown
    assert e.value.code == SPK_ERR_ARG
    for bad in (dict(coarsening=2), dict(coarsening=-1), dict(coarsening="grid", grid=(17, 17), transfer=2),
                dict(coarsening="grid", grid=(17, 17), transfer=-1), dict(coarsening="grid", grid=(578, 1)),
                dict(coarsening="grid", grid=(1, 289, 1)), dict(coarsening="grid", grid=(17, 17, 0)),
                dict(coarsening="grid"), dict(coarsening="grid", grid=(65536, 65536))):
        with pytest.raises(SpkError) as e:
            S.AmgHierarchy(A17, **bad)
        assert e.value.code == SPK_ERR_ARG, bad
    # under aggregation the new fields are not read
    h = S.AmgHierarchy(A17, grid=(3, 3), transfer=7)
    assert h.info()["coarsening"] == S.AMG_COARSEN_AGGREGATION and h.info()["dims"] == [(0, 0, 0)] * h.info()["levels"]
    h.close()


def test_options_mirror_the_struct():
    d = S.solver.amg_opts_dict(S.amg_opts())
    assert d["coarsening"] == S.AMG_COARSEN_AGGREGATION and d["grid"] == (0, 0, 0) and d["transfer"] == S.AMG_TRANSFER_MATRIX_FREE
    d = S.solver.amg_opts_dict(S.amg_opts(coarsening="grid", grid=(33, 9), transfer="stored"))
    assert d["coarsening"] == S.AMG_COARSEN_GRID and d["grid"] == (33, 9, 1) and d["transfer"] == S.AMG_TRANSFER_STORED
    assert S.solver.amg_opts_dict(S.amg_opts(grid=(9, 9, 5)))["grid"] == (9, 9, 5)


def _pcg_its(Asp, f, M, rtol=1e-8):
    cnt = [0]
    x, rc = spl.cg(Asp, f, M=M, rtol=rtol, maxiter=200, callback=lambda xk: cnt.__setitem__(0, cnt[0] + 1))
    assert rc == 0 and np.linalg.norm(f - Asp @ x) <= 10 * rtol * np.linalg.norm(f)
    return cnt[0]


def test_vcycle_iterations_are_grid_independent_and_no_more_than_aggregations():
    """The numpy V-cycle as a CG preconditioner to rtol 1e-8: the grid hierarchy's counts differ by at most 1 across
    33^2, 65^2, 129^2, and at each grid they are no larger than the aggregation hierarchy's, built by the same builder."""
    its = {}
    for n in (33, 65, 129):
        A, f = S.AssembleOperator_Laplace(n, n)
        Asp = sp.csr_matrix((A.val, A.colidx, A.rowptr), shape=(A.nrows, A.nrows))
        for kind, kw in (("grid", dict(coarsening="grid", grid=(n, n))), ("aggregation", {})):
            h = S.AmgHierarchy(A, **kw)
            info = h.info()
            mats = hierarchy_mats(h.matrix, info)
            M = spl.LinearOperator(Asp.shape, matvec=lambda r, m=mats, i=info: vcycle_ref(*m, i["lambda_max"], r))
            its[kind, n] = _pcg_its(Asp, f, M)
            print(f"{n}^2 {kind}: {its[kind, n]} iterations, {info['levels']} levels, complexity {info['operator_complexity']:.3f}")
            h.close()
    grid = [its["grid", n] for n in (33, 65, 129)]
    assert max(grid) - min(grid) <= 1, its
    for n in (33, 65, 129):
        assert its["grid", n] <= its["aggregation", n], its


# ---- the KSP facade (no GPU: SetFromOptions and the option checks of SetUp run before any context exists) -------------
@pytest.mark.parametrize("prefix", ["", "-fieldsplit_0_"])
def test_facade_reads_back_every_mg_option(prefix):
    k = S.KSP()
    opts = ["-pc_mg_galerkin", "-pc_mg_levels", "4", "-mg_levels_ksp_max_it", "3", "-pc_gamg_coarse_eq_limit", "120",
            "-spk_mg_transfer", "stored", "-spk_gamg_setup", "device", "-pc_gamg_reuse_interpolation", "-pc_mg_galerkin", "pmat"]
    opts = [o if not o.startswith("-") or not prefix else prefix + o[1:] for o in opts]
    pc = ["-pc_type", "mg"] if not prefix else ["-pc_type", "fieldsplit", "-fieldsplit_0_ksp_type", "preonly",
                                                "-fieldsplit_0_pc_type", "mg"]
    k.setFromOptions(["-ksp_type", "fgmres"] + pc + opts)
    got, sel = k.getAMGOptions(fieldsplit0=bool(prefix))
    other, osel = k.getAMGOptions(fieldsplit0=not prefix)
    assert sel and not osel
    assert got["coarsening"] == S.AMG_COARSEN_GRID and other["coarsening"] == S.AMG_COARSEN_AGGREGATION
    assert got["max_levels"] == 4 and got["smooth_its"] == 3 and got["coarse_eq_limit"] == 120
    assert got["transfer"] == S.AMG_TRANSFER_STORED and other["transfer"] == S.AMG_TRANSFER_MATRIX_FREE
    assert got["setup"] == S.AMG_SETUP_DEVICE and k.getAMGReuse(fieldsplit0=bool(prefix))
    k.setFromOptions([prefix + "spk_mg_transfer" if prefix else "-spk_mg_transfer", "matrixfree", "-pc_mg_galerkin", "both"])
    assert k.getAMGOptions(fieldsplit0=bool(prefix))[0]["transfer"] == S.AMG_TRANSFER_MATRIX_FREE
    _, pct, _ = k.getOptions()
    assert pct == (S.PC_JACOBI if not prefix else S.PC_SCHUR)
    k.setFromOptions(["-pc_type", "gamg"] if not prefix else ["-fieldsplit_0_pc_type", "gamg"])   # and back
    assert k.getAMGOptions(fieldsplit0=bool(prefix))[0]["coarsening"] == S.AMG_COARSEN_AGGREGATION
    k.destroy()


def _setup_code(opts, grid=None):
    k = S.KSP()
    try:
        if grid:
            k.setGrid(*grid)
        k.setFromOptions(opts)
        k.setUp()
    except SpkError as e:
        return e.code, str(e)
    finally:
        k.destroy()
    return 0, ""


def test_facade_refusals_before_any_gpu_work():
    fs = ["-pc_type", "fieldsplit", "-fieldsplit_0_pc_type", "mg"]
    code, msg = _setup_code(["-ksp_type", "fgmres", "-pc_type", "mg"])
    assert code == SPK_ERR_STATE and "SpkKSPSetGrid" in msg and "-pc_type mg" in msg
    code, msg = _setup_code(["-ksp_type", "fgmres"] + fs)
    assert code == SPK_ERR_STATE and "SpkKSPSetGrid" in msg and "-fieldsplit_0_pc_type mg" in msg
    # with a grid the option checks pass and the set-up stops at the missing operator
    code, msg = _setup_code(["-ksp_type", "fgmres", "-pc_type", "mg"], grid=(17, 17))
    assert code == SPK_ERR_STATE and "KSPSetOperators" in msg
    code, msg = _setup_code(["-ksp_type", "minres", "-pc_type", "mg"], grid=(17, 17))
    assert code == SPK_ERR_UNSUPPORTED and "minres" in msg and "(mg)" in msg
    code, msg = _setup_code(["-ksp_type", "minres"] + fs + ["-pc_fieldsplit_schur_fact_type", "diag"], grid=(17, 17))
    assert code == SPK_ERR_UNSUPPORTED and "(mg)" in msg
    code, msg = _setup_code(["-ksp_type", "fgmres"] + fs + ["-fieldsplit_0_ksp_type", "richardson", "-fieldsplit_0_ksp_max_it", "3"],
                            grid=(17, 17))
    assert code == SPK_ERR_UNSUPPORTED and "FP32" in msg and "mg" in msg
    code, msg = _setup_code(["-ksp_type", "fgmres", "-pc_type", "mg", "-spk_inner_sweeps", "2"], grid=(17, 17))
    assert code == SPK_ERR_UNSUPPORTED and "FP32" in msg
    k = S.KSP()
    for bad in ((1, 5, 1), (5, 1, 1), (5, 5, -1)):
        with pytest.raises(SpkError) as e:
            k.setGrid(*bad)
        assert e.value.code == SPK_ERR_ARG
    k.setGrid(5, 5, 0)   # mz = 0 reads as 2-D
    k.destroy()


@pytest.mark.parametrize("opts,code", [
    (["-pc_mg_galerkin", "none"], SPK_ERR_UNSUPPORTED),
    (["-pc_mg_galerkin", "mat"], SPK_ERR_UNSUPPORTED),
    (["-fieldsplit_0_pc_mg_galerkin", "0"], SPK_ERR_UNSUPPORTED),
    (["-spk_mg_transfer"], SPK_ERR_ARG),
    (["-spk_mg_transfer", "csr"], SPK_ERR_UNSUPPORTED),
    (["-fieldsplit_0_spk_mg_transfer", "free"], SPK_ERR_UNSUPPORTED),
    (["-pc_mg_type", "full"], SPK_ERR_UNSUPPORTED),
    (["-pc_mg_cycle_type", "w"], SPK_ERR_UNSUPPORTED),
])
def test_facade_refuses_malformed_mg_options(opts, code):
    k = S.KSP()
    with pytest.raises(SpkError) as e:
        k.setFromOptions(["-ksp_type", "fgmres", "-pc_type", "mg"] + opts)
    assert e.value.code == code
    k.destroy()
