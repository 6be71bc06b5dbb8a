"""The Gram-Schmidt kernels of spk_k_vec.hip (VecMDot, VecMAXPY, the cycle-start norm, pack_bd) and the head kernel of
spk_k_krylov.hip, each launch form with every argument the solver passes, through the spk_debug_* hooks (the production host
wrappers, unchanged).  Cases, inputs and references live in _vec_worker.py.

Exact tier: integer inputs, every sum an exact double, np.array_equal against the int64 reference; the integer 1000003 in all
padding and behind n_dot / n_bd.  Rounding tier: Gaussian data with heavy cancellation against np.longdouble, bound
d * 2^-53 * S with d counted from the launch shape (_vec_worker.depth).  The forms behind SPK_VEC_WS=0, SPK_VEC_WS16=0 and
SPK_VEC_DEEP=1 -- knobs read once per process -- run in one fresh child process each.  Needs a real MI355X: run with -m gpu."""
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vec_worker as W  # noqa: E402

pytestmark = pytest.mark.gpu

_ID = dict(ids=lambda c: c["id"] if isinstance(c, dict) else None)


@pytest.fixture(scope="module")
def ctx(spk):
    c = spk.Context(0)
    yield c
    c.close()


def _check(ctx, case, forms=None):
    res = W.run_case(ctx, case)
    if case.get("gauss"):
        print(f"{case['id']}: {res['forms']} reduced err / (2^-53 S) = {res['ratio']} (d = {res['d']}), "
              f"vector = {res['vratio']} (d = {res['vd']})")
    assert res["ok"], f"{case['id']} {res['forms']}: {res['mismatch']}"
    if forms is not None:
        assert res["forms"] == forms
    return res


def test_shape_hook_agrees_with_the_restatement(ctx):
    """The case lists name their forms through _vec_worker's restatement of ws_shape / vec_shape; here the library says the
    same at every size the lists use and at the thresholds."""
    sizes = {1, 2, 131071, 131072, 262143, 262144, 524287, 524288, 1048575, 1048576}
    sizes |= {n for ns in W.WS16_N.values() for n in ns} | set(W.STREAM_N) | {n for ns in W.MAXPY_N.values() for n in ns}
    for n in sorted(sizes):
        assert ctx.debug_vec_shape(n) == W.shapes(n, {}), n
    assert ctx.debug_vec_shape(1)["ws16"] == 1 and ctx.debug_vec_shape(1)["deep"] == 0


# --------------------------------------------------------------------------- VecMDot
@pytest.mark.parametrize("U,case", W.mdot_ws16_cases(), **_ID)
def test_mdot_sixteen_wave(ctx, U, case):
    """mdot_ws16_kernel: U = 2 / 4 / 8 double2 per lane, 1 / 2 / 3 vectors per wave, waves without vectors, the (3, 4) kernel
    on the U = 8 grid, ragged last tiles, a wrapped grid."""
    per = (case["nv"] + 15) // 16
    vw, u = (max(per, 1), U) if per <= 2 else (3, 4 if U == 8 else U)
    _check(ctx, case, [f"mdot_ws16_kernel<{vw},{u}>"])


@pytest.mark.parametrize("case", W.mdot_stream_cases(), **_ID)
def test_mdot_streaming(ctx, case):
    """mdot_kernel<NG, 512, 4, true, 4>, NG = 1 .. 5, one whole tile per workgroup, one entry more, a wrapped grid."""
    _check(ctx, case, [f"mdot_kernel<{(case['nv'] + 7) // 8},512,4,4>"])


@pytest.mark.parametrize("case", W.mdot_chunk_cases(), **_ID)
def test_mdot_chunks(ctx, case):
    """More than 40 vectors: two launches writing partials + v0 and out + v0; w.w comes from the last one, once."""
    res = _check(ctx, case)
    assert len(res["forms"]) == 2


@pytest.mark.parametrize("case", W.mdot_rider_cases(), **_ID)
def test_mdot_riders(ctx, case):
    """n_dot below n (odd and even), a second slab of dense rows, parity planes, 40 vectors exactly, the gate word."""
    _check(ctx, case)


# --------------------------------------------------------------------------- VecMAXPY
@pytest.mark.parametrize("form,case", W.maxpy_cases(), **_ID)
def test_maxpy(ctx, form, case):
    """maxpy_kernel<256, 8, ., 0, 1>, <256, 8, ., 0, 2> and <512, 4, ., 0, 4>: vector counts around the group size, both signs,
    no norm, a device-side live count, n_dot below n, the gate word."""
    T, U, G = form
    _check(ctx, case, [f"maxpy_kernel<{T},{G},0,{U}>"])


@pytest.mark.parametrize("case", W.maxpy_plane_cases(), **_ID)
def test_maxpy_planes(ctx, case):
    """B D planes: m = 1 .. 8 dense (MP = 4, 8), m = 2, 4, 6, 8 packed, n_bd even and odd, n_dot = n_bd and n; w1side is
    w'[n_bd : n_bd + m]; row r sums entries below n_bd only, packed .x feeds row 2q and .y row 2q + 1."""
    _check(ctx, case)


@pytest.mark.parametrize("case", W.maxpy_pyth_cases(), **_ID)
def test_maxpy_pythagorean_rider(ctx, case):
    """ww - sum h^2 a power of 4: nrm_out and row nv of tb exact; ww - sum h^2 <= 0: the floor 1.5e-14 ww."""
    _check(ctx, case)


# --------------------------------------------------------------------------- cycle start and head
@pytest.mark.parametrize("case", W.norm_cases(), **_ID)
def test_sqnorm_bd(ctx, case):
    _check(ctx, case)


@pytest.mark.parametrize("case", W.pack_cases(), **_ID)
def test_pack_bd(ctx, case):
    _check(ctx, case)


@pytest.mark.parametrize("case", W.head_cases(), **_ID)
def test_fused_head(ctx, case):
    _check(ctx, case)


# --------------------------------------------------------------------------- rounding tier
def test_longdouble_is_wide_enough():
    import numpy as np
    assert np.finfo(np.longdouble).nmant + 1 >= 64


@pytest.mark.parametrize("case", W.gauss_cases(), **_ID)
def test_rounding_tier(ctx, case):
    _check(ctx, case)


# --------------------------------------------------------------------------- the knob children
# One fresh process per knob, one at a time.  Measured on an MI355X: the same cases take 0.3 - 1.2 s in the default process
# (the largest list moves about 2 GB of vectors to the device) and a whole child, with the import of numpy and the library
# and the creation of its context, 1.0 - 2.2 s.  60 s is that with a wide margin for a busy machine and a cold file cache,
# and still ends a hung child long before anything else would.
CHILD_TIMEOUT = 60
_child_failed = []   # a child that died or hung: the remaining children fail at once without being started


@pytest.mark.parametrize("knob", ["SPK_VEC_WS", "SPK_VEC_WS16", "SPK_VEC_DEEP"])
def test_knob_child(knob, tmp_path):
    assert not _child_failed, f"not started: the {_child_failed[0]} child died or hung"
    extra, cases = W.knob_cases(knob)
    case_file, out_file = tmp_path / "cases.json", tmp_path / "out.json"
    case_file.write_text(json.dumps(cases))
    env = dict(os.environ)
    for k in ("SPK_VEC_WS", "SPK_VEC_WS16", "SPK_VEC_DEEP"):
        env.pop(k, None)
    env.update(extra)
    try:
        p = subprocess.run([sys.executable, W.__file__, str(case_file), str(out_file)], env=env, timeout=CHILD_TIMEOUT,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired as e:
        _child_failed.append(knob)
        pytest.fail(f"{knob} child ran into its timeout of {CHILD_TIMEOUT} s\n{e.stdout}\n{e.stderr}")
    if p.returncode < 0:
        _child_failed.append(knob)
    assert p.returncode == 0, f"{knob} child ended with {p.returncode}\n{p.stdout}\n{p.stderr}"
    out = json.loads(out_file.read_text())
    for n, got in out["shapes"].items():   # the child read its knob
        want = W.shapes(int(n), extra)
        assert {k: tuple(v) if isinstance(v, list) else v for k, v in got.items()} == want, n
    results = {r["id"]: r for r in out["results"]}
    assert sorted(results) == sorted(c["id"] for c in cases)
    for c in cases:
        r = results[c["id"]]
        if c.get("gauss"):
            print(f"{knob} {c['id']}: {r['forms']} reduced err / (2^-53 S) = {r['ratio']} (d = {r['d']}), "
                  f"vector = {r['vratio']} (d = {r['vd']})")
        assert r["forms"] == W.case_forms(c, extra)
    bad = [f"{r['id']} {r['forms']}: {r['mismatch']} (got {r.get('got')}, expected {r.get('expected')})"
           for r in out["results"] if not r["ok"]]
    assert not bad, "\n".join(bad)
