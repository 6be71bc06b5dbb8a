"""-pc_type mg on the GPU with row-to-row varying values: the operator family of tests/_mg_fields.py through the device
Galerkin kernels, the device symmetrise, the products route, the refresh, the stencil level operator and its LDS staging,
the fused tail, the cycles and the Lanczos kernels.  On the constant-coefficient operators of the other mg files the rows
of a level are copies of one another, and a kernel that reads D^-1, b or a value of the neighbouring node, of the other
component or of the transposed block passes their bars; test_mg_varcoef_cpu.py shows that on these fields each such
mistake moves one V-cycle by 1e-6 or more in each coefficient region, where the bar below is 1e-12 per region.

Tried once on an MI355X against a library whose so_row (spk_stencil_op_core.hpp) read D^-1 of the previous node in x at the
nodes 3 <= i <= nx - 3: every one-application check of the constant-coefficient files passed (V and W, all eight shapes of
test_gpu_mg_operator at 1e-12; only its bit-for-bit hook saw it, on five of eight shapes), while d and f below failed on
every shape and field.

The assertions are those of test_gpu_mg_grid, _galerkin, _operator, _cycle and test_gpu_amg_lanczos, on other values;
nothing here is larger than 65 x 33 or 17 x 9 x 5.  The transfer kernels read no operator values and are not run alone."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import _mg_fields as F
import saddle_point_petsc_amd as S
from test_gpu_amg_lanczos import _bytes as _all_bytes
from test_gpu_mg_cycle import _tail_rows
from test_gpu_mg_galerkin import _bytes
from test_gpu_mg_grid import _close, _ctx, _export, _scipy
from test_gpu_mg_operator import STEPS, _ordered_rows, _step, _vec
from test_mg_cycle_cpu import cycle_ref
from test_mg_galerkin_cpu import _its
from test_mg_sides_cpu import hierarchy_mats, vcycle_ref

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
SOLVED = F.cases(("33x33", "17x9x5"), only=("smooth", "jump"))


def _host(shape, field, galerkin):
    h = S.AmgHierarchy(F.operator(shape, field), **F.amg_kw(shape, galerkin=galerkin))
    hi = h.info()
    ex = _export(h.matrix, hi)
    h.close()
    return hi, ex


@functools.lru_cache(maxsize=None)
def _both_routes(shape, field, galerkin):
    """two device builds and the host build of one operator under one Galerkin route, computed once and never changed"""
    A = F.operator(shape, field)
    got = []
    for _ in range(2):
        with _ctx(A, amg=F.amg_kw(shape, galerkin=galerkin, setup="device")) as c:
            di = c.amg_info()
            got.append((di, _export(c.amg_level, di)))
    return got[0], got[1], _host(shape, field, galerkin)


def _ritz_and_coarse_inverse(tag, di, dev, hi, host, bits):
    """test_device_ritz_values_and_coarse_inverse_are_the_hosts: lambda_max to 1e-12 relative -- the host's bits where the
    device route runs the host's Lanczos on a download (stencil-built levels >= 1 of at most 1024 rows) -- and the coarse
    inverse to 1e-10 of its largest entry"""
    worst = 0.0
    for l in range(di["levels"] - 1):
        rel = abs(di["lambda_max"][l] - hi["lambda_max"][l]) / hi["lambda_max"][l]
        print(f"{tag} lambda_max[{l}] = {di['lambda_max'][l]:.6g}: relative {rel:.3e} off the host's")
        worst = max(worst, rel)
        if bits and 0 < l and di["rows"][l] <= 1024:
            assert di["lambda_max"][l] == hi["lambda_max"][l], f"{tag}: lambda_max of level {l} is not the host's bits"
    _close(dev["cinv"], host["cinv"], 1e-10, f"{tag} coarse inverse")
    assert worst <= 1e-12
    return worst


def _row_relative(dev, host):
    """max over the entries of |dev - host| relative to the largest |host| entry of the same row"""
    rp, _, v, _ = host
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    big = np.zeros(len(rp) - 1)
    np.maximum.at(big, rows, np.abs(v))
    assert np.all(big > 0.0)
    return float((np.abs(dev[2] - v) / big[rows]).max())


def _products_bar(tag, di, dev, hi, host):
    """test_device_setup_is_the_host_builds: P byte for byte, the patterns equal, A_l and D^-1 to 1e-12 -- here of the largest
    entry of the same row, and of the entry itself: under `jump` the largest entry of the matrix hides the soft half --
    lambda_max to 1e-12 relative and the coarse inverse to 1e-10.  Returns the worst A_l and D^-1 figures."""
    assert di["setup"] == S.AMG_SETUP_DEVICE and di["coarsening"] == S.AMG_COARSEN_GRID and di["galerkin"] == S.AMG_GALERKIN_PRODUCTS
    assert di["levels"] == hi["levels"] >= 3 and di["dims"] == hi["dims"] and di["rows"] == hi["rows"] and di["nnz"] == hi["nnz"]
    for l in range(di["levels"] - 1):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(dev["P"][l][:3], host["P"][l][:3])) and dev["P"][l][3] == host["P"][l][3], f"P_{l}"
    wa = wd = 0.0
    for l in range(di["levels"]):
        assert np.array_equal(dev["A"][l][0], host["A"][l][0]) and np.array_equal(dev["A"][l][1], host["A"][l][1]), f"pattern of A_{l}"
        ea = _row_relative(dev["A"][l], host["A"][l])
        dd, dh = (sp.csr_matrix((m[2], m[1], m[0]), shape=m[3]).diagonal() for m in (dev["A"][l], host["A"][l]))
        ed = float((np.abs(1.0 / dd - 1.0 / dh) * np.abs(dh)).max())
        print(f"{tag} level {l}: A_l {ea:.3e} of the row's largest entry, D^-1 {ed:.3e} relative (bound 1e-12)")
        assert ea <= 1e-12 and ed <= 1e-12, (tag, l)
        wa, wd = max(wa, ea), max(wd, ed)
    _ritz_and_coarse_inverse(tag, di, dev, hi, host, bits=False)
    return wa, wd


# ---- a. the stencil Galerkin kernels and the device symmetrise against the host ----------------------------------------
@pytest.mark.parametrize("shape,field", F.cases(skew=True))
def test_device_stencil_build_is_the_host_builds_bytes(shape, field):
    """A_l, P_l, row pointers and columns byte for byte; two device builds the same bytes; lambda_max and the coarse inverse
    to the bars of test_gpu_mg_galerkin.  Under `skew` the symmetrisation kernel averages numbers that differ in the second
    digit -- the only case in which it does."""
    (di, dev), (di2, dev2), (hi, host) = _both_routes(shape, field, "stencil")
    assert di["setup"] == S.AMG_SETUP_DEVICE and di["galerkin"] == hi["galerkin"] == S.AMG_GALERKIN_STENCIL
    assert di["levels"] == hi["levels"] >= 3 and di["dims"] == hi["dims"] and di["rows"] == hi["rows"] and di["nnz"] == hi["nnz"]
    assert di["operator_complexity"] == hi["operator_complexity"]
    assert _bytes(dev) == _bytes(host), f"{shape} {field}: a device-built A_l or P_l differs from the host's"
    for l in range(1, di["levels"]):
        dd, dh = (sp.csr_matrix((m[2], m[1], m[0]), shape=m[3]).diagonal() for m in (dev["A"][l], host["A"][l]))
        assert dd.tobytes() == dh.tobytes()
    assert _bytes(dev2) == _bytes(dev) and dev2["cinv"].tobytes() == dev["cinv"].tobytes() and di2["lambda_max"] == di["lambda_max"]
    assert np.all(np.isfinite(di["lambda_max"][:-1]))
    _ritz_and_coarse_inverse(f"{shape} {field}", di, dev, hi, host, bits=True)


# ---- b. the products route against the host ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape,field", F.cases())
def test_device_products_build_is_the_host_builds(shape, field):
    (di, dev), (di2, dev2), (hi, host) = _both_routes(shape, field, "products")
    wa, wd = _products_bar(f"{shape} {field} products", di, dev, hi, host)
    print(f"{shape} {field} products: worst A_l {wa:.3e}, worst D^-1 {wd:.3e}")
    assert di2["lambda_max"] == di["lambda_max"]
    assert _all_bytes(dev2) == _all_bytes(dev)


# ---- c. the refresh against the host -----------------------------------------------------------------------------------
@pytest.mark.parametrize("galerkin", ["stencil", "products"])
@pytest.mark.parametrize("shape", list(F.SHAPES))
def test_device_refresh_gives_the_host_builds_levels(shape, galerkin):
    """Built on the constant operator, refreshed to `smooth` and then to `jump` (five_point: to `dad`): under the stencil
    route the refreshed A_l are the bytes of a fresh host stencil build of the new operator, under the products route they
    meet its bar; P keeps its bytes.  (lambda_max and the coarse inverse to the bars of a: the refresh runs the Lanczos
    and the Cholesky on the operator brought back to the binade of the build.)"""
    amg = F.amg_kw(shape, galerkin=galerkin, setup="device")
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, F.operator(shape, "const"))
        c.pc_setup(S.PC_JACOBI, amg=amg, amg_reuse=True)
        assert c.amg_reuse_info()["refreshed"] is False
        b0 = _export(c.amg_level, c.amg_info())
        for field in F.fields(shape)[:2]:
            A1 = F.operator(shape, field)
            assert np.array_equal(A1.colidx, F.operator(shape, "const").colidx)
            c.set_block(S.BLOCK_A00, A1)
            c.pc_setup(S.PC_JACOBI, amg=amg, amg_reuse=True)
            assert c.amg_reuse_info()["refreshed"] is True
            di = c.amg_info()
            dev = _export(c.amg_level, di)
            hi, host = _host(shape, field, galerkin)
            tag = f"{shape} refreshed to {field}, {galerkin}"
            assert _bytes(dev)[1] == _bytes(b0)[1], f"{tag}: the refresh changed P"
            assert _bytes(dev)[0] != _bytes(b0)[0]
            if galerkin == "stencil":
                assert _bytes(dev) == _bytes(host), f"{tag}: a refreshed level differs from the host's fresh build"
                _ritz_and_coarse_inverse(tag, di, dev, hi, host, bits=False)
            else:
                _products_bar(tag, di, dev, hi, host)


# ---- d. the stencil operator hook --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,field", F.cases())
def test_hook_product_and_step(shape, field):
    """test_gpu_mg_operator.test_hook_product_and_step on these levels: product and step bit for bit the numpy loop in the
    stated order with the level's own D^-1, the CSR route within its derived bound (2 (n_r + 1) 2^-53 sum |v| |x| per row
    for the product; alpha |dinv| times that plus 8 u M for the step), the `done` gate writes nothing."""
    A = F.operator(shape, field)
    with _ctx(A, amg=F.amg_kw(shape, galerkin="stencil", setup="device", operator="stencil")) as c:
        info = c.amg_info()
        L = info["levels"]
        assert info["operator"] == S.AMG_OPERATOR_STENCIL and info["galerkin"] == S.AMG_GALERKIN_STENCIL and L >= 3
        if shape == "65x33":
            assert info["dims"][1] == (33, 17, 1) and info["rows"][1:3] == [1122, 306]
        worst = 0.0
        for l in range(1, L - 1):
            rp, ci, v, shp = c.amg_level(l)
            n = shp[0]
            x, xo, b = _vec(n, 10 + l), _vec(n, 20 + l), _vec(n, 30 + l)
            dinv = 1.0 / sp.csr_matrix((v, ci, rp), shape=shp).diagonal()
            d, mag, nr = _ordered_rows(rp, ci, v, x)
            bound = 2.0 * (nr + 1) * U * mag
            got = c.debug_amg_operator(l, "product", x)
            assert got.tobytes() == d.tobytes(), f"{shape} {field} level {l}: the product is not the stated sum"
            csr = c.debug_amg_operator(l, "product", x, stencil=False)
            assert np.all(np.abs(got - csr) <= bound), (shape, field, l, float((np.abs(got - csr) - bound).max()))
            worst = max(worst, float((np.abs(got - csr)[bound > 0] / bound[bound > 0]).max()))
            sentinel = _vec(n, 40 + l)
            for alpha, beta, given in STEPS:
                yo = xo if given else None
                ref = _step(d, x, dinv, b, alpha, beta, yo)
                got = c.debug_amg_operator(l, "step", x, b=b, xo=yo, alpha=alpha, beta=beta)
                assert got.tobytes() == ref.tobytes(), f"{shape} {field} level {l}: step ({alpha}, {beta}, xo {given}) is not the stated formula"
                csr = c.debug_amg_operator(l, "step", x, b=b, xo=yo, alpha=alpha, beta=beta, stencil=False)
                M = np.abs(x) + alpha * np.abs(dinv) * (np.abs(b) + mag) + beta * (np.abs(x) + (np.abs(xo) if given else 0.0))
                assert np.all(np.abs(got - csr) <= alpha * np.abs(dinv) * bound + 8.0 * U * M), (shape, field, l, alpha, beta, given)
                kept = c.debug_amg_operator(l, "step", x, b=b, xo=yo, alpha=alpha, beta=beta, done=True, out=sentinel)
                assert kept.tobytes() == sentinel.tobytes(), f"{shape} {field} level {l}: the step wrote behind a set done gate"
            kept = c.debug_amg_operator(l, "product", x, done=True, out=sentinel)
            assert kept.tobytes() == sentinel.tobytes(), f"{shape} {field} level {l}: the product wrote behind a set done gate"
        print(f"{shape} {field}: largest |stencil - csr| / bound of a product row {worst:.4f}")


# ---- e. the fused tail gives the launches' bits -------------------------------------------------------------------------
@pytest.mark.parametrize("shape,field", F.cases(("33x33", "12x10any", "17x9x5")))
def test_fused_tail_gives_the_bits_of_the_launches(shape, field):
    """both cycles, the CSR and the stencil level operator, tail_rows at the sizes of level 1, level 2 and the coarsest level
    (and 1: no tail)"""
    A = F.operator(shape, field)
    x = _vec(A.nrows, 7)
    inside = set()
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        for cycle in ("v", "w"):
            ref = {}
            for op in ("csr", "stencil"):
                kw = F.amg_kw(shape, galerkin="stencil", setup="device", operator=op, cycle=cycle)
                c.pc_setup(S.PC_JACOBI, amg=dict(kw, tail="launches"))
                info = c.amg_info()
                assert info["tail_first"] == -1 and info["operator"] == (op == "stencil")
                ref[op] = c.pc_apply(x)
                assert np.all(np.isfinite(ref[op])) and np.any(ref[op] != 0.0)
                for tr in _tail_rows(info["rows"]):
                    c.pc_setup(S.PC_JACOBI, amg=dict(kw, tail="fused", tail_rows=tr))
                    t = c.amg_info()["tail_first"]
                    assert (t == -1) == (tr == 1)
                    if op == "stencil" and 0 < t < info["levels"] - 1:
                        inside.add(t)
                    y = c.pc_apply(x)
                    assert y.tobytes() == ref[op].tobytes(), f"{shape} {field} {cycle} {op} tail_rows {tr} (tail_first {t}): {np.abs(y - ref[op]).max():.3e} off the launches"
            assert not np.array_equal(ref["csr"], ref["stencil"]), "the stencil route gave the CSR route's bits: is it running?"
    assert inside, "no stencil level ran inside the tail"


# ---- f. one application against numpy ----------------------------------------------------------------------------------
CONFIGS = [(cycle, transfer, op) for cycle in ("v", "w") for transfer in ("matrixfree", "stored") for op in ("csr", "stencil")]


@pytest.mark.parametrize("shape,field", F.cases())
def test_one_application_matches_numpy(shape, field):
    """V (vcycle_ref) and W (cycle_ref) over the downloaded hierarchy, matrix-free and stored transfers, both operator
    routes: 1e-12 relative in the norm over each coefficient region separately -- test_mg_varcoef_cpu.py holds the numpy
    reference itself to 1e-14 per region against longdouble, and measures 3.7e-16.  Two applications give the same bytes."""
    A = F.operator(shape, field)
    x = F.rhs(A.nrows)
    reg = F.regions(shape)
    refs, worst = {}, [0.0, 0.0]
    with S.Context(0) as c:
        c.set_block(S.BLOCK_A00, A)
        for cycle, transfer, op in CONFIGS:
            c.pc_setup(S.PC_JACOBI, amg=F.amg_kw(shape, galerkin="stencil", setup="device", cycle=cycle, transfer=transfer, operator=op,
                                                 tail="fused" if cycle == "w" else "launches"))
            info = c.amg_info()
            y, y2 = c.pc_apply(x), c.pc_apply(x)
            if cycle not in refs:   # the hierarchy does not depend on the cycle, the transfers or the operator route
                mats = hierarchy_mats(c.amg_level, info)
                refs[cycle] = vcycle_ref(*mats, info["lambda_max"], x) if cycle == "v" else cycle_ref(*mats, info["lambda_max"], x, 2)
            assert y.tobytes() == y2.tobytes() and info["operator"] == (op == "stencil") and info["cycle"] == (cycle == "w")
            assert info["tail_first"] >= 1 if cycle == "w" else info["tail_first"] == -1
            err = F.region_rel(y, refs[cycle], reg)
            print(f"{shape} {field} {cycle} {transfer} {op}: {err[0]:.3e} (soft) {err[1]:.3e} (stiff) off numpy (bound 1e-12)")
            worst = [max(a, b) for a, b in zip(worst, err)]
            assert max(err) <= 1e-12, (shape, field, cycle, transfer, op, err)
    print(f"{shape} {field}: worst of one application {worst[0]:.3e} (soft) {worst[1]:.3e} (stiff)")


# ---- g. the Lanczos kernels on D^-1 A with a varying D -----------------------------------------------------------------
@pytest.mark.parametrize("galerkin", ["stencil", "products"])
@pytest.mark.parametrize("shape,field", SOLVED)
def test_resident_lanczos_is_the_stepwise_routes_bits(shape, field, galerkin):
    """test_gpu_amg_lanczos's equalities: the tridiagonal of every level by both hooks, lambda_max, every level, the coarse
    inverse and one application"""
    A = F.operator(shape, field)
    x = F.rhs(A.nrows, 11)
    out = {}
    for route in ("stepwise", "resident"):
        with _ctx(A, amg=F.amg_kw(shape, galerkin=galerkin, setup="device", lanczos=route)) as c:
            info = c.amg_info()
            out[route] = (info, _all_bytes(_export(c.amg_level, info)), c.pc_apply(x).tobytes())
            if route == "stepwise":
                hook = [(c.debug_amg_lanczos(l, resident=False), c.debug_amg_lanczos(l, resident=True)) for l in range(info["levels"] - 1)]
    (si, sb, sy), (ri, rb, ry) = out["stepwise"], out["resident"]
    for l, ((ss, sal, sbe), (rs, ral, rbe)) in enumerate(hook):
        print(f"{shape} {field} {galerkin} level {l} ({si['rows'][l]} rows): {ss} steps stepwise, {rs} resident; al[0] {sal[0]!r}")
        assert ss == rs and 1 <= ss <= min(30, si["rows"][l]), (l, ss, rs)
        assert len(sal) == len(sbe) == ss and sbe[0] == 0.0 and rbe[0] == 0.0
        assert sal.tobytes() == ral.tobytes(), f"level {l}: al differs by {np.abs(sal - ral).max():.3e}"
        assert sbe.tobytes() == rbe.tobytes(), f"level {l}: be differs by {np.abs(sbe - rbe).max():.3e}"
    assert hook[0][0][0] == 30
    assert (si["lanczos"], ri["lanczos"]) == (S.AMG_LANCZOS_STEPWISE, S.AMG_LANCZOS_RESIDENT)
    assert si["levels"] == ri["levels"] and si["rows"] == ri["rows"] and si["lambda_max"] == ri["lambda_max"]
    assert sb == rb and sy == ry


# ---- h. solves ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,field", SOLVED)
def test_k_equals_a_solves(shape, field):
    """fgmres and pipecg to rtol 1e-8: reason 2, the true residual against scipy's product at most 2e-8, the stencil and the
    CSR operator routes within one iteration of one another and of the numpy-preconditioned count (scipy's cg and gmres
    around vcycle_ref on the host-built hierarchy)."""
    A, f = F.problem(shape, field)
    Asp = _scipy(A)
    h = S.AmgHierarchy(A, **F.amg_kw(shape, galerkin="stencil"))
    ref = {"pipecg": _its(h, Asp, f, "cg"), "fgmres": _its(h, Asp, f, "gmres")}
    h.close()
    its = {}
    for op in ("stencil", "csr"):
        with _ctx(A, amg=F.amg_kw(shape, galerkin="stencil", setup="device", operator=op)) as c:
            assert c.amg_info()["operator"] == (op == "stencil")
            for ksp in ("fgmres", "pipecg"):
                x, info = getattr(c, ksp)(f, rtol=1e-8, max_it=200)
                res = np.linalg.norm(f - Asp @ x) / np.linalg.norm(f)
                print(f"{shape} {field} {op} {ksp}: {info['its']} iterations (numpy {ref[ksp]}), true residual {res:.2e}")
                assert info["reason"] == 2 and res <= 2e-8
                its[op, ksp] = info["its"]
    for ksp in ("fgmres", "pipecg"):
        assert abs(its["stencil", ksp] - its["csr", ksp]) <= 1, its
        for op in ("stencil", "csr"):
            assert abs(its[op, ksp] - ref[ksp]) <= 1, (its, ref)
