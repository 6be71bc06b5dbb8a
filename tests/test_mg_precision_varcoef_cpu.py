"""-spk_mg_precision single on variable-coefficient operators, without a GPU: the fields of tests/_mg_fields.py under the numpy
cycle with FP32 levels (test_mg_precision_cpu.vcycle_ref_mixed).  Everything here is computed from the numpy references on
host-built hierarchies; no code under test runs.  tests/test_gpu_mg_precision_varcoef.py takes its bar (bar), its iteration
allowance (numpy_iterations) and its scaling exponents (SCALE_K) from here.

a. The gap, recorded: on the constant-coefficient operator the float32 D^-1 of every x-interior row of level 1 has the bits
   of the previous node's, so the bit-for-bit hook checks of tests/test_gpu_mg_precision.py cannot see a float kernel that
   reads D^-1 one node off; under `smooth`, `lognormal`, `dad` and `skew` no such row shares D^-1 or its values.
b. The mixed cycle against the FP64 one (test_mg_cycle_cpu.cycle_ref) on every (shape, field), V and W, whole vector and
   per coefficient region: the bar of the GPU file.
c. The bar discriminates: the five mis-indexings of test_mg_varcoef_cpu.py restated in the mixed cycle.
d. FGMRES(30) around both cycles: the iteration allowance of the GPU solves.
e. The mixed cycle commutes with a scaling by 2^+-40 (the GPU file asks the device for the same)."""
import functools

import numpy as np
import pytest

import _mg_fields as F
import test_mg_precision_cpu as C
import test_mg_varcoef_cpu as V
from test_gpu_mg_operator import STEPS
from test_gpu_mg_precision import _ordered, _step32, _vec32
from test_gpu_mg_varcoef import SOLVED
from test_mg_cycle_cpu import cycle_ref
from test_mg_precision_cpu import fgmres_numpy, vcycle_ref_mixed

F32 = np.float32
CASES = F.cases(skew=True)
SCALE_K = (40, -40)


# ---- a. the gap ---------------------------------------------------------------------------------------------------------
def dirichlet_rows(A, P):
    """the rows of level 1 that no coefficient reaches: every fine row under the coarse basis function is a Dirichlet row of
    level 0 (nothing stored off its diagonal but zeros)"""
    off = A[0].tocsr().copy()
    off.setdiag(0.0)
    off.eliminate_zeros()
    free = (np.diff(off.indptr) > 0).astype(np.float64)
    return np.asarray(abs(P[0]).T @ free).ravel() == 0.0


@functools.lru_cache(maxsize=None)
def shared_with_the_previous_node(shape, field):
    """over the x-interior rows of level 1 that are not Dirichlet rows: (rows, those whose float32 D^-1 has the bits of the
    same component's one node back in x, those whose float32 values do, the Dirichlet rows left out)"""
    bs = F.SHAPES[shape][1]
    info, (A, P, _) = F.host_hierarchy(shape, field)
    A1 = A[1].tocsr()
    rp, v = A1.indptr, A1.data.astype(F32)
    dinv = (1.0 / A1.diagonal()).astype(F32)   # the FP64 D^-1 rounded once, as amg_round_levels makes it
    fixed = dirichlet_rows(A, P)
    rows = same_d = same_v = left = 0
    for n in V.x_interior_nodes(info["dims"][1]):
        for a in range(bs):
            r, q = n * bs + a, (n - 1) * bs + a
            if fixed[r] and field != "const":
                left += 1
                continue
            rows += 1
            same_d += int(dinv[r].tobytes() == dinv[q].tobytes())
            same_v += int(v[rp[r]:rp[r + 1]].tobytes() == v[rp[q]:rp[q + 1]].tobytes())
    return rows, same_d, same_v, left


@pytest.mark.parametrize("shape", list(F.SHAPES))
def test_float32_dinv_of_the_constant_operator_is_the_previous_nodes(shape):
    """The blind spot.  Rounding to float32 erases the last bits in which the FP64 D^-1 of neighbouring nodes differed: every
    x-interior row of level 1 (test_mg_varcoef_cpu.x_interior_nodes), Dirichlet rows included, has the float32 D^-1 of the
    previous node in x -- 33x33 408 of 408, 65x33 952 of 952, 12x10any 24 of 24, 17x9x5 180 of 180, five17x9 20 of 20.  The
    stored float32 rows still differ on most shapes (equal: 2 of 408, 19 of 952, 4 of 24 -- the Dirichlet rows --, 0 of 180)
    and on five17x9 not at all (20 of 20 equal), so there a float kernel that reads the previous node's row passes the bitwise
    checks too."""
    rows, same_d, same_v, _ = shared_with_the_previous_node(shape, "const")
    print(f"{shape} const: float32 D^-1 equal to the previous node's on {same_d} of {rows} x-interior rows of level 1, the values on {same_v}")
    assert rows > 0 and same_d == rows
    if shape == "five17x9":
        assert same_v == rows


@pytest.mark.parametrize("shape,field", F.cases(skew=True, only=("smooth", "lognormal", "dad", "skew")))
def test_no_row_of_a_variable_field_shares_its_float32_dinv_or_values(shape, field):
    """Under `smooth`, `lognormal`, `dad` (and `skew` on top of them) no x-interior row of level 1 that a coefficient reaches
    has the float32 D^-1 or the float32 values of the previous node: 0 of 408, 952, 20 (12x10any: its 4 x-interior rows on
    the Dirichlet side j = ny - 1 hold 0.25, 1.5, 0.25 under every field and are left out), 180 and 20 rows."""
    rows, same_d, same_v, left = shared_with_the_previous_node(shape, field)
    print(f"{shape} {field}: {same_d} D^-1 and {same_v} rows equal to the previous node's of {rows} ({left} Dirichlet rows left out)")
    assert rows > 0 and same_d == 0 and same_v == 0
    assert left == (4 if shape == "12x10any" else 0)


def test_jump_is_not_the_field_for_the_dinv_claim():
    """Printed, nothing asserted: inside each half of `jump` D^-1 stays equal in 2-D (33x33 340 of 408, 65x33 884 of 952,
    12x10any 0 of 20; 17x9x5, whose `jump` carries a factor per element, 0 of 180)."""
    for shape, field in F.cases(only=("jump",)):
        rows, same_d, same_v, left = shared_with_the_previous_node(shape, field)
        print(f"{shape} jump: float32 D^-1 equal on {same_d} of {rows} rows, the values on {same_v} ({left} Dirichlet rows left out)")


# ---- b. the mixed reference against the FP64 one: the bar ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cycles(shape, field, gamma):
    """(mixed, double) of one application of the two numpy cycles to F.rhs on the host-built hierarchy; nobody writes into them"""
    info, mats = F.host_hierarchy(shape, field)
    x = F.rhs(info["rows"][0])
    y32 = vcycle_ref_mixed(*mats, info["lambda_max"], x, gamma=gamma)
    y64 = cycle_ref(*mats, info["lambda_max"], x, gamma)
    for y in (y32, y64):
        y.setflags(write=False)
    return y32, y64


@functools.lru_cache(maxsize=None)
def mixed_against_double(shape, field, gamma):
    """(whole vector, [soft, stiff]): || mixed - double || / || double || of one application"""
    y32, y64 = cycles(shape, field, gamma)
    return float(np.linalg.norm(y32 - y64) / np.linalg.norm(y64)), F.region_rel(y32, y64, F.regions(shape))


@functools.lru_cache(maxsize=None)
def bar(gamma=1):
    """(bar, largest per-region figure, its case): the rule of test_gpu_mg_precision._bar on the new operators, per region --
    four times the largest per-region distance between the two numpy cycles over CASES"""
    worst, case = max((max(mixed_against_double(s, f, gamma)[1]), (s, f)) for s, f in CASES)
    return 4.0 * worst, worst, case


@pytest.mark.parametrize("gamma", [1, 2])
def test_mixed_cycle_against_the_double_one_per_region(gamma):
    """|| vcycle_ref_mixed - cycle_ref || / || cycle_ref || on every (shape, field) of cases(skew=True).

      cycle | whole vector, largest   | per region, largest | case of the per-region value | bar (four times it)
      V     | 1.24e-7 (65x33 smooth)  | 1.29e-7             | 65x33 smooth, stiff half     | 5.17e-7
      W     | 6.14e-7 (33x33 lognorm.)| 8.18e-7             | 33x33 lognormal, stiff half  | 3.27e-6

    Under `jump` the stiff half differs by 1.6e-11 (17x9x5) to 1.3e-10 (65x33) under V and by at most 3.3e-10 under W: with
    kappa = 1e4 the coarse correction there is 1e-4 of the soft half's.  So a lower bound that says "the FP32 levels ran"
    (> 1e-10) holds on the whole vector (smallest 1.8e-9, 17x9x5 lognormal under V) and not per region.  Every whole-vector
    figure lies between 1e-10 and 1e-4, the bounds of test_mg_precision_cpu.test_mixed_cycle_differs_at_the_fp32_level."""
    b, worst, case = bar(gamma)
    whole = {}
    for s, f in CASES:
        w, reg = mixed_against_double(s, f, gamma)
        whole[s, f] = w
        print(f"{s} {f} {'vw'[gamma - 1]}: mixed against double {w:.3e} whole, {reg[0]:.3e} (soft) {reg[1]:.3e} (stiff)")
        assert 1e-10 < w < 1e-4 and max(reg) < 1e-4, (s, f, gamma, w, reg)
    big = max(whole, key=whole.get)
    print(f"{'vw'[gamma - 1]}: largest whole-vector {whole[big]:.3e} ({big[0]} {big[1]}), smallest {min(whole.values()):.3e}; "
          f"largest per region {worst:.3e} ({case[0]} {case[1]}), bar {b:.3e}")
    assert b == 4.0 * worst and worst >= max(whole.values())   # the larger of a case's two regions is at least its whole-vector figure


# ---- c. the bar discriminates -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def moves(shape, field):
    """per region the distance of each mis-indexed mixed V-cycle from the right mixed V-cycle (test_mg_varcoef_cpu._moves in
    FP32 levels: the wrong D^-1 rounded as the right one is, the wrong A_1 rounded as the right one is)"""
    bs = F.SHAPES[shape][1]
    info, (A, P, Ci) = F.host_hierarchy(shape, field)
    lam, dims = info["lambda_max"], info["dims"]
    b = F.rhs(A[0].shape[0])
    ref = cycles(shape, field, 1)[0]
    assert vcycle_ref_mixed(A, P, Ci, lam, b, dinv=V._dinv(A)).tobytes() == ref.tobytes()   # nothing mis-indexed: the reference
    reg = F.regions(shape)
    out = {}
    for key, wrong in (("dinv", V.dinv_of_the_other_component(A, dims, bs)), ("dinv-inner", V.dinv_of_the_other_component(A, dims, bs, True)),
                       ("dinv-x", V.dinv_of_the_previous_node(A, dims, bs))):
        out[key] = F.region_rel(vcycle_ref_mixed(A, P, Ci, lam, b, dinv=wrong), ref, reg)
    for key, wrong in (("row", V.rows_of_the_previous_node), ("block", V.transposed_blocks)):
        B = list(A)
        B[1] = wrong(A[1], dims[1], bs)
        out[key] = F.region_rel(vcycle_ref_mixed(B, P, Ci, lam, b, dinv=V._dinv(A)), ref, reg)
    return out


@pytest.mark.parametrize("shape,field", CASES)
def test_every_mistake_moves_the_mixed_cycle_past_the_bar(shape, field):
    """Each mis-indexing on level 1 of the mixed V-cycle, per region, against twice the V bar of b (1.03e-6).

    `row` and `block`: at least twice the bar in each region on every case.  Smallest: row 1.1e-5, block 1.5e-5, both in the
    stiff half of 17x9x5 `jump` -- the FP64 figures of test_mg_varcoef_cpu.py, ten times the condition and twenty times the
    bar.

    The three D^-1 mis-indexings, asserted under `smooth`, `lognormal`, `dad` and `skew` on every case; smallest `dinv` 1.5e-3
    (17x9x5 lognormal), `dinv-inner` 3.2e-4 (33x33 smooth), `dinv-x` 3.3e-4 (17x9x5 smooth), all in the soft half: no case
    falls short, so none has to lean on the bitwise hook check alone.  (Under `lognormal` a wrong D^-1 or row can make the
    smoother diverge: moves of 1e2 to 1e7.)  Under `jump` they are printed: smallest `dinv` 4.1e-6 (33x33), `dinv-x` 2.8e-6
    (17x9x5), both in the stiff half and also above twice the bar; `dinv-inner` moves 33x33 `jump` by exactly 0 -- the
    record of test_mg_varcoef_cpu.py, unchanged in FP32: inside a half of `jump` the two components' D^-1 are equal off the
    level's edge, and there the bitwise hook check of tests/test_gpu_mg_precision_varcoef.py on `smooth` and `lognormal`
    carries the claim."""
    m = moves(shape, field)
    need = 2.0 * bar(1)[0]
    print(f"{shape} {field}: moved per region (soft, stiff) by " + ", ".join(f"{k} {v[0]:.2e} {v[1]:.2e}" for k, v in m.items())
          + f" (needed {need:.2e})")
    for k in ("row", "block"):
        assert min(m[k]) >= need, (shape, field, k, m[k], need)
    if field != "jump":
        for k in ("dinv", "dinv-inner", "dinv-x"):
            assert min(m[k]) >= need, (shape, field, k, m[k], need)


# ---- d. the iteration allowance -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def numpy_iterations(shape, field):
    """{'mixed', 'double'}: iterations of FGMRES(30) to rtol 1e-8 on K = A around the two numpy V-cycles, and the true
    residuals"""
    A, f = F.problem(shape, field)
    Asp = F.to_sp((A.rowptr, A.colidx, A.val, (A.nrows, A.nrows)))
    info, mats = F.host_hierarchy(shape, field)
    out = {}
    for label, cyc in (("double", lambda r: cycle_ref(*mats, info["lambda_max"], r, 1)), ("mixed", lambda r: vcycle_ref_mixed(*mats, info["lambda_max"], r))):
        x, its = fgmres_numpy(Asp, cyc, f, rtol=1e-8, restart=30)
        out[label] = its
        out[label + "_residual"] = float(np.linalg.norm(f - Asp @ x) / np.linalg.norm(f))
    return out


def allowance(shape, field):
    """what the GPU solve test allows between the device's `single` and `double` counts: the numpy difference plus one"""
    n = numpy_iterations(shape, field)
    return abs(n["mixed"] - n["double"]) + 1


@pytest.mark.parametrize("shape,field", SOLVED)
def test_mixed_cycle_in_fgmres_on_the_solved_cases(shape, field):
    """Iterations mixed / double: 33x33 smooth 9 / 9, 33x33 jump 9 / 9, 17x9x5 smooth 15 / 15, 17x9x5 jump 16 / 16 -- the FP32
    levels cost no iteration on a 1e4 contrast, the allowance of the GPU solves is 1 on every case; true residuals at most
    2e-8 (measured 1.1e-9 to 5.6e-9, the same to three digits under both cycles)."""
    n = numpy_iterations(shape, field)
    print(f"{shape} {field}: {n['mixed']} iterations with FP32 levels (true residual {n['mixed_residual']:.2e}), {n['double']} in FP64 "
          f"({n['double_residual']:.2e}); allowance {allowance(shape, field)}")
    assert n["mixed_residual"] <= 2e-8 and n["double_residual"] <= 2e-8
    assert n["mixed"] <= n["double"] + 1, n


# ---- e. scaling by a power of two ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [1, 2])
def test_mixed_cycle_commutes_with_a_power_of_two(gamma):
    """33x33 `smooth`: cycle(2^k x) has the bytes of 2^k cycle(x) for k = +-40.  Every operation of the cycle is linear in
    the vector and a power of two changes no rounding while every intermediate stays a normal float: the entries of the
    FP32 levels lie between 1.2e-38 2^40 = 1.3e-26 and 3.4e38 2^-40 = 3.1e26 in magnitude or are exact zeros.  (An entry
    that left the normal range would lose bits on one side only and break the equality.)"""
    info, mats = F.host_hierarchy("33x33", "smooth")
    x = F.rhs(info["rows"][0])
    y = cycles("33x33", "smooth", gamma)[0]
    for k in SCALE_K:
        s = 2.0 ** k
        ys = vcycle_ref_mixed(*mats, info["lambda_max"], s * x, gamma=gamma)
        assert ys.tobytes() == (s * y).tobytes(), (gamma, k, float(np.abs(ys - s * y).max()))


# ---- f. the host statement of the mistake the GPU file is for -----------------------------------------------------------
def _step_references(A1, d1, bs, seed):
    """the three step references of the GPU hook checks on a level (test_gpu_mg_precision's vectors and formula), with the
    level's own float32 D^-1 and with that of the previous node in x at the x-interior nodes"""
    A1 = A1.tocsr()
    n = A1.shape[0]
    x, xo, b = _vec32(n, 10 + seed), _vec32(n, 20 + seed), _vec32(n, 30 + seed)
    dinv = (1.0 / A1.diagonal()).astype(F32)
    nodes = np.array(V.x_interior_nodes(d1), np.int64)
    wrong = dinv.reshape(-1, bs).copy()
    if len(nodes):
        wrong[nodes] = dinv.reshape(-1, bs)[nodes - 1]
    wrong = wrong.ravel()
    d = _ordered(A1.indptr, A1.indices, A1.data, x, F32)
    right = [_step32(d, x, dinv, b, al, be, xo if given else None) for al, be, given in STEPS]
    moved = [_step32(d, x, wrong, b, al, be, xo if given else None) for al, be, given in STEPS]
    return right, moved, len(nodes) * bs


def test_the_existing_hook_check_passes_a_step_that_reads_the_previous_nodes_dinv():
    """The mutation, stated on the host: a float step kernel that reads D^-1 of the previous node in x at the nodes
    3 <= i <= nx - 3 returns, on every level and shape test_gpu_mg_precision.test_hooks_are_numpy_float32_bit_for_bit runs it
    on, the very bytes that test expects -- it cannot fail."""
    seen = 0
    for name in C.GPU_SHAPES:
        info, (A, _, _) = C.host_hierarchy(name)
        for l in range(1, info["levels"] - 1):
            right, moved, rows = _step_references(A[l], info["dims"][l], info["block_size"], l)
            seen += rows
            assert all(r.tobytes() == m.tobytes() for r, m in zip(right, moved)), (name, l)
    print(f"{seen} rows over the levels of {len(C.GPU_SHAPES)} shapes read the previous node's D^-1 and returned the expected bytes")
    assert seen > 1000


@pytest.mark.parametrize("shape,field", F.cases(skew=True, only=("smooth", "lognormal", "dad", "skew")))
def test_the_new_hook_check_fails_it(shape, field):
    """The same mutated step against the reference of test_gpu_mg_precision_varcoef.test_hooks_are_numpy_float32_bit_for_bit
    on level 1: the bytes differ under every step, at more than nine in ten of the rows that read the wrong D^-1."""
    info, (A, _, _) = F.host_hierarchy(shape, field)
    right, moved, rows = _step_references(A[1], info["dims"][1], F.SHAPES[shape][1], 1)
    for r, m in zip(right, moved):
        differ = int(np.count_nonzero(r != m))
        print(f"{shape} {field}: {differ} of the {rows} rows that read the previous node's D^-1 return other bits")
        assert differ > 0.9 * (rows - (4 if shape == "12x10any" else 0))
