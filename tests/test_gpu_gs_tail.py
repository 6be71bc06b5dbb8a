"""Form 7's short remainder tile (SPK_GS_TAIL; spk_k_iter.hip gs_fused_tail_kernel, mdot_tiles in spk_device.hpp).
By default the workgroup that the tile loop would give the remainder of VecMDot's pass to -- at most 16 double2 behind
whole tiles that are a multiple of the grid -- stages those entries in LDS at entry and adds their products behind its
loop; SPK_GS_TAIL=0 is the launch that walks the remainder as a loop trip, as before.  The epilogue adds exactly what
the trip would have added, so both variants and forced form 5 (mdot_kernel keeps the loop trip) must agree bit for bit,
history and x -- where the path engages (a remainder of multiplier entries only; of real nodes of the grid too) and
where the shape keeps the loop trip (no remainder; a long one; whole tiles that are no multiple of the grid), told by
Context.gs_launch().

No debug hook drives the fused launch with integer data (debug_mdot reaches form 5's mdot_kernel only), so the solves
are the check of the kernel.

Each variant runs all cases in ONE fresh child process (tests/_gs_tail_worker.py): the knob is read per solve, but the
variants are compared across clean contexts.  Needs a real MI355X: run with -m gpu."""
import pytest

import _gs_rig as R
import _gs_tail_worker as W

pytestmark = pytest.mark.gpu

VARIANTS = ("0", "1")
# where the default launch stages the remainder (the launcher's condition; tail_expected() must say the same)
TAKEN = {"full", "restart4", "restart8", "restart9", "restart12", "restart13", "lower", "real_nodes"}


runs = R.child_runs("SPK_GS_TAIL", VARIANTS, W.__file__)


@pytest.mark.parametrize("name", list(W.CASES))
def test_every_variant_is_form_5_bit_for_bit(runs, name):
    """AUTO takes form 7 under either SPK_GS_TAIL; its residual history and x equal forced form 5 on the same context and
    the other variant's (np.array_equal).  The remainder is staged exactly where the launcher's condition holds and the
    knob allows it: in every launch of the solve or in none."""
    R.assert_form_5_bit_for_bit(runs, VARIANTS, name, W.CASES[name][4])
    for a in VARIANTS:
        r = runs[a][0][name]
        assert W.tail_expected(r["rows"], r["m"]) == (name in TAKEN), (name, r["rows"], r["m"])
        print(f"{name} SPK_GS_TAIL={a}: {r['launches']} launches of form 7, {r['tail']} with the remainder staged")
        assert r["launches"] > 0 and r["form5"]["launches"] == r["form5"]["tail"] == 0, (a, r["launches"])
        assert r["tail"] == (r["launches"] if a == "1" and name in TAKEN else 0), (a, r["tail"], r["launches"])


@pytest.mark.parametrize("a", VARIANTS)
def test_launches_gated_off_behind_the_end_of_the_solve(runs, a):
    """-ksp_max_it 47 at restart 30: the launches enqueued behind iteration 47 return at the gate with the remainder's
    loads in flight and nothing staged.  The count and the reason are max_it's, and the next solve is the undisturbed one
    bit for bit."""
    R.assert_gated(runs[a][0])
    g = runs[a][0]["gated"]
    assert g["tail"] == (g["launches"] if a == "1" else 0) and g["launches"] > 0
