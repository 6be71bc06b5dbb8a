"""Form 7's loads ahead of the totals wait (SPK_GS_AHEAD; spk_k_iter.hip gs_fused_kernel, KeepSet in spk_device.hpp).
SPK_GS_AHEAD=0 is the launch with its keep set alone; 1 (the default) requests a second group of basis vectors of the
first tile ahead of the wait, into the tile loop's own buffer; 2 stood for groups of the first tile left to the XCD's L2
as well -- plain loads in both passes, which changed the bits from nv = 16 on and found nothing in the L2, so they were
taken out and 2 runs as 1; it stays among the variants so that it keeps doing so.  No addition moves and
every value read is the one a later load would return: the variants and forced form 5 must agree bit for bit, history and x.

Each variant runs all cases in ONE fresh child process (tests/_gs_ahead_worker.py): the knob is read per solve, but the
variants are compared across clean contexts.  Needs a real MI355X: run with -m gpu."""
import numpy as np
import pytest

import _gs_ahead_worker as W
import _gs_rig as R
from _gs_rig import _hist

pytestmark = pytest.mark.gpu

VARIANTS = ("0", "1", "2")

runs = R.child_runs("SPK_GS_AHEAD", VARIANTS, W.__file__)


@pytest.mark.parametrize("name", list(W.CASES))
def test_every_variant_is_form_5_bit_for_bit(runs, name):
    """AUTO takes form 7 under every SPK_GS_AHEAD; its residual history and x equal forced form 5 on the same context and
    the other variants' (np.array_equal)."""
    R.assert_form_5_bit_for_bit(runs, VARIANTS, name, W.CASES[name][4])


@pytest.mark.parametrize("a", VARIANTS)
def test_launches_gated_off_behind_the_end_of_the_solve(runs, a):
    """-ksp_max_it 47 at restart 30: the launches enqueued behind iteration 47 return at the gate with their loads ahead of
    the wait in flight.  The count and the reason are max_it's, and the next solve is the undisturbed one bit for bit."""
    R.assert_gated(runs[a][0])


@pytest.mark.parametrize("a", VARIANTS)
def test_wait_that_gives_up_leaves_the_context_usable(runs, a):
    """The bounded in-launch waits at one tick: SPK_ERR_HIP ("timed out"), never a numerical reason; with the bound restored
    the next solve reproduces the undisturbed one bit for bit."""
    r = runs[a][0]
    w = r["wait"]
    assert w["code"] == -2 and "timed out" in w["message"], w
    assert w["after"]["form"] == W.GSF and w["after"]["its"] == 45
    assert np.array_equal(_hist(w["after"]), _hist(r["full"])) and w["after_x_equal"]
