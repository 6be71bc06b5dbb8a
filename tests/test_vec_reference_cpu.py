"""The CPU-side pieces of the Gram-Schmidt kernel tests (tests/_vec_worker.py): the integer reference builders against
brute-force Python loops at n <= 64 for every rider -- a wrong reference can neither pass as a kernel bug nor hide one --,
the restated launch shapes at their thresholds, the depth function of the rounding tier, and the case lists: unique ids, and
every template instantiation the dispatch can reach has a case."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _vec_worker as W  # noqa: E402


def _small_cases():
    c = []
    for n in (1, 2, 7, 64):
        for nv in (0, 1, 5):
            c.append(W.mdot_case(n, nv))
            c.append(W.maxpy_case(n, nv, sign=-1.0))
    for n in (9, 10, 63, 64):
        for m in range(1, 9):
            c += [W.mdot_case(n, 3, nv2=m), W.mdot_case(n, 3, nv2=m, n_dot=n - 1), W.mdot_case(n, 3, nv2=m, n_dot=n - m)]
            c += [W.maxpy_case(n + m, 4, sign=-1.0, bd="dense", m=m, w1side=1), W.maxpy_case(n + m, 4, bd="dense", m=m, w1side=1, n_dot=n),
                  W.norm_case(n + m, m), W.norm_case(n + m, m, sub=1, full=1), W.pack_case(n, m), W.head_case(n & ~1, m, want_wl=1),
                  W.head_case(n & ~1, m, fact=W.SCHUR_LOWER)]
        for m in (2, 4, 6, 8):
            c += [W.mdot_case(n, 2, nv2=m, split=1), W.mdot_case(n, 2, nv2=m, split=1, n_dot=n - m),
                  W.mdot_case(n, 2, nv2=m, split=1, n_dot=n - m + 1), W.maxpy_case(n + m, 4, bd="packed", m=m, w1side=1),
                  W.maxpy_case(n + m, 4, sign=-1.0, bd="packed", m=m, n_dot=n), W.pack_case(n, m, bad=0), W.pack_case(n, m, bad=1),
                  W.head_case(n & ~1, m, packed=1), W.head_case(n & ~1, m, packed=1, fact=W.SCHUR_LOWER, want_wl=1)]
        c += [W.mdot_case(n, 4, nv2=2, split=1, done=1), W.mdot_case(n, 4, done=0), W.maxpy_case(n, 4, done=1), W.maxpy_case(n, 4, want_norm=0),
              W.maxpy_case(n, 6, nv_live=2), W.maxpy_case(n, 6, nv_live=0), W.norm_case(n, 0), W.head_case(n & ~1, 0, jacobi=1, fact=W.SCHUR_LOWER),
              W.maxpy_case(n + 4, 6, sign=-1.0, want_norm=0, m=4, w1side=1, pyth="pow4", pyth_k=2, n_dot=n),
              W.maxpy_case(n + 3, 6, nv_live=4, sign=-1.0, want_norm=0, m=3, w1side=1, pyth="pow4", pyth_k=-1, n_dot=n),
              W.maxpy_case(n + 4, 6, sign=-1.0, want_norm=0, m=4, w1side=1, pyth="floor", n_dot=n),
              W.maxpy_case(n + 4, 6, sign=-1.0, m=4, pyth="pow4", pyth_k=0, done=1)]
    return c


@pytest.mark.parametrize("case", _small_cases(), ids=lambda c: c["id"])
def test_reference_builders_agree_with_brute_force(case):
    inp = W.INPUTS[case["k"]](case)
    ref, brute = W.REFERENCE[case["k"]](case, inp), W.BRUTE[case["k"]](case, inp)
    assert sorted(ref) == sorted(brute)
    assert W.first_mismatch(ref, brute) is None


def test_exact_tier_inputs_carry_the_padding_value():
    case = W.mdot_case(64, 3, nv2=4, split=1, n_dot=60)
    inp = W.mdot_inputs(case)
    assert np.all(inp["V"][:, 60:] == W.PADV) and np.all(inp["V2"][:, 60:] == W.PADV) and np.all(inp["w"][60:] == W.PADV)
    assert np.abs(inp["V"][:, :60]).max() <= 3 and np.abs(inp["V2"][:, :60]).max() <= 2
    case = W.maxpy_case(64, 3, bd="packed", m=4, n_dot=60)
    inp = W.maxpy_inputs(case)
    assert np.all(inp["planes"][:, 60:] == W.PADV) and np.all(inp["w"][60:] == W.PADV)
    assert np.array_equal(inp["planes"][0, 0:60:2], inp["bd"][0, 0:60:2]) and np.array_equal(inp["planes"][0, 1:60:2], inp["bd"][1, 1:60:2])
    assert not inp["bd"][0, 1:60:2].any() and not inp["bd"][1, 0:60:2].any()


def test_pythagorean_inputs_hit_a_power_of_four_and_the_floor():
    for kind, k in (("pow4", 3), ("pow4", -2), ("floor", 0)):
        case = W.maxpy_case(40, 6, m=4, pyth=kind, pyth_k=k, want_norm=0)
        d = W.maxpy_inputs(case)["pyth"]["dots"]
        tt2 = d[-1] - d[:6] @ d[:6]
        assert (tt2 == 4.0 ** k) if kind == "pow4" else (tt2 <= 0.0 and d[-1] > 0.0)


def test_restated_shapes_at_their_thresholds():
    # (on, U, grid) of the wave-split forms
    assert W.ws_shape(65535) == (1, 2, 256) and W.ws_shape(65536) == (1, 4, 256)
    assert W.ws_shape(131071) == (1, 4, 256) and W.ws_shape(131072) == (1, 8, 256)
    assert W.ws_shape(524287)[0] == 1 and W.ws_shape(524288)[0] == 0
    assert W.ws_shape(1) == (1, 2, 1) and W.ws_shape(129) == (1, 2, 2)
    assert W.ws_shape(1000, {"SPK_VEC_WS": "0"})[0] == 0
    # (T, U, G, grid)
    assert W.vec_shape(131071) == (256, 1, 4, 256) and W.vec_shape(131072) == (256, 2, 4, 256)
    assert W.vec_shape(262144) == (256, 4, 4, 256) and W.vec_shape(524288) == (512, 4, 4, 256)
    assert W.vec_shape(262143, True) == (256, 1, 8, 1024) and W.vec_shape(262144, True) == (256, 2, 8, 512)
    assert W.vec_shape(524287, True) == (256, 2, 8, 1024) and W.vec_shape(524288, True) == (512, 4, 4, 256)
    assert W.vec_shape(256, True) == (256, 1, 8, 1) and W.vec_shape(257, True) == (256, 1, 8, 2)
    assert W.vec_grid(131073, 512) == 256 and W.vec_grid(513, 512) == 2 and W.vec_grid(1) == 1
    # the dispatch
    assert [f["name"] for f in W.mdot_forms(263169, 40)] == ["mdot_ws16_kernel<3,4>"]
    assert [f["name"] for f in W.mdot_forms(263169, 32)] == ["mdot_ws16_kernel<2,8>"]
    assert [(f["name"], f["k"]) for f in W.mdot_forms(1048577, 63)] == [("mdot_kernel<5,512,4,4>", 40), ("mdot_kernel<3,512,4,4>", 24)]
    assert [(f["name"], f["k"]) for f in W.mdot_forms(70001, 0)] == [("mdot_ws16_kernel<1,2>", 1)]
    assert [f["name"] for f in W.mdot_forms(262145, 33, {"SPK_VEC_WS16": "0"})] == ["mdot_ws_kernel<12,8,2>"]
    assert [f["name"] for f in W.mdot_forms(262145, 9, {"SPK_VEC_WS": "0"})] == ["mdot_kernel<2,256,4,2>"]
    assert W.maxpy_form(513, 17, 4, {"SPK_VEC_DEEP": "1"})["name"] == "maxpy_kernel<256,32,4,1>"
    assert W.maxpy_form(524289, 9, 0, {"SPK_VEC_DEEP": "1"})["name"] == "maxpy_kernel<256,16,0,2>"
    assert W.maxpy_form(524289, 9, 0)["name"] == "maxpy_kernel<256,8,0,2>"


def test_depth_counts_the_longest_path():
    # one tile of 64 x 2 double2, 16 waves publishing per wave, one workgroup: 1 + (2 * 2 + 1) + 6 + 0 + (1 + log2(1024 / 2))
    f = W.mdot_forms(129, 1)[0]
    assert (f["grid"], f["k"]) == (1, 2) and W.final_reduce_depth(1, 2, 1024) == 1 + 9
    assert W.depth(f, 129) == 1 + 5 + 6 + 0 + 10
    # streaming: 1052673 entries = 526337 double2 = 257 tiles of 2048 on 256 workgroups -> 2 tiles; 33 + 1 values -> kk = 64,
    # 8 slices of 32 blocks, a tree of 3
    f = W.mdot_forms(1052673, 33)[0]
    assert W.depth(f, 1052673) == 1 + 2 * 9 + 6 + 8 + (32 + 3)
    # MAXPY norm, thin form: 70005 entries = 35003 double2 = 137 tiles of 256, one each; 5 values -> kk = 8, 32 slices
    f = dict(W.maxpy_form(70005, 30, 4), k=5)
    assert W.depth(f, 70005, per_tile=2) == 1 + 2 + 6 + 4 + (5 + 5)
    f = W.norm_form(262145, 8)
    assert f["grid"] == 256 and W.depth(f, 262145, per_tile=2) == 1 + 2 * 2 + 6 + 8 + (8 + 5)


def _all_lists():
    default = [c for _, c in W.mdot_ws16_cases()] + W.mdot_stream_cases() + W.mdot_chunk_cases() + W.mdot_rider_cases() + \
        [c for _, c in W.maxpy_cases()] + W.maxpy_plane_cases() + W.maxpy_pyth_cases() + W.norm_cases() + W.pack_cases() + \
        W.head_cases() + W.gauss_cases()
    return default, {k: W.knob_cases(k) for k in ("SPK_VEC_WS", "SPK_VEC_WS16", "SPK_VEC_DEEP")}


def test_case_ids_are_unique_and_every_group_takes_the_form_it_names():
    default, knobs = _all_lists()
    for lst in [default] + [c for _, c in knobs.values()]:
        ids = [c["id"] for c in lst]
        assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    for U, c in W.mdot_ws16_cases():
        f = W.mdot_forms(c["n"], c["nv"])[0]
        assert f["name"].startswith("mdot_ws16_kernel") and W.ws_shape((c["n"] + 1) // 2)[1] == U
    assert all(W.case_forms(c) == [f"mdot_kernel<{(c['nv'] + 7) // 8},512,4,4>"] for c in W.mdot_stream_cases())
    assert all(len(W.case_forms(c)) == 2 for c in W.mdot_chunk_cases())
    for (T, U, G), c in W.maxpy_cases():
        assert W.case_forms(c) == [f"maxpy_kernel<{T},{G},0,{U}>"]


def test_every_reachable_instantiation_has_a_case():
    """The instantiations k::mdot, k::maxpy, k::sqnorm_bd, k::pack_bd and k::fused_head can launch, written out; the case
    lists of the default process and of the three knob children launch every one of them and nothing else."""
    reach = {f"mdot_ws16_kernel<{vw},{u}>" for u in (2, 4, 8) for vw in (1, 2, 3)} - {"mdot_ws16_kernel<3,8>"}
    reach |= {f"mdot_ws_kernel<{vw},{u},{g}>" for vw in (4, 8, 12) for u, g in ((2, 4), (4, 4), (8, 2))}
    reach |= {f"mdot_kernel<{ng},{t},4,{u}>" for ng in range(1, 6) for t, u in ((512, 4), (256, 4), (256, 2), (256, 1))}
    reach |= {f"maxpy_kernel<{t},{g},{mp},{u}>" for mp in (0, 4, 8)
              for t, g, u in ((512, 4, 4), (256, 8, 2), (256, 8, 1), (256, 16, 2), (256, 16, 1), (256, 32, 1))}
    reach |= {"sqnorm_bd_kernel<4>", "sqnorm_bd_kernel<8>", "pack_bd_kernel", "fused_head_kernel<4>", "fused_head_kernel<8>"}
    default, knobs = _all_lists()
    seen = {f for c in default for f in W.case_forms(c, {})}
    for env, cases in knobs.values():
        seen |= {f for c in cases for f in W.case_forms(c, env)}
    assert seen == reach, (sorted(reach - seen), sorted(seen - reach))
