"""The set-up route of the multigrid hierarchy (spk_amg_opts.setup, -spk_gamg_setup host|device) without a GPU: the
default, the round trip through the Python options, the refusal of an unknown route, the host-only builder (which
accepts either route and builds on the host), the KSP facade's option, and what the level accessors refuse."""
import numpy as np
import pytest

import saddle_point_petsc_amd as S
from saddle_point_petsc_amd._lib import SpkError
from saddle_point_petsc_amd.solver import amg_opts_dict

from test_amg_cpu import laplace

SPK_ERR_ARG, SPK_ERR_UNSUPPORTED = -1, -6


def test_default_route_is_the_host():
    assert (S.AMG_SETUP_HOST, S.AMG_SETUP_DEVICE) == (0, 1)
    assert amg_opts_dict(S.amg_opts())["setup"] == S.AMG_SETUP_HOST


@pytest.mark.parametrize("value", ["device", 1])
def test_device_route_round_trips(value):
    o = S.amg_opts(setup=value, smooth_its=3)
    d = amg_opts_dict(o)
    assert d["setup"] == S.AMG_SETUP_DEVICE and d["smooth_its"] == 3 and d["richardson_scale"] == 1.0
    assert amg_opts_dict(S.amg_opts(setup="host"))["setup"] == S.AMG_SETUP_HOST


def test_unknown_route_is_refused():
    A, _, _ = laplace(16)
    for bad in (2, -1):
        with pytest.raises(SpkError) as e:
            S.AmgHierarchy(A, setup=bad)
        assert e.value.code == SPK_ERR_ARG and "setup" in str(e.value)


def test_host_builder_takes_either_route_and_builds_on_the_host():
    A, _, _ = laplace(32)
    h, d = S.AmgHierarchy(A, setup="host"), S.AmgHierarchy(A, setup="device")
    ih, idv = h.info(), d.info()
    assert ih["setup"] == idv["setup"] == S.AMG_SETUP_HOST
    assert ih["levels"] == idv["levels"] >= 2 and ih["rows"] == idv["rows"] and ih["lambda_max"] == idv["lambda_max"]
    L = ih["levels"]
    for l in range(L):
        kinds = [S.AMG_OP] + ([S.AMG_PROLONG, S.AMG_TENTATIVE] if l + 1 < L else [S.AMG_COARSE_INV])
        for which in kinds:
            a, b = h.matrix(l, which), d.matrix(l, which)
            assert a[3] == b[3] and all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])), (l, which)
        if l + 1 < L:
            assert np.array_equal(h.aggregates(l), d.aggregates(l))
    h.close()
    d.close()


def refused_queries(matrix, aggregates, L):
    """The eight queries the accessors refuse on a hierarchy of L levels, through matrix(level, which) and
    aggregates(level): {name: (code, message)}."""
    calls = {
        "level -1": lambda: matrix(-1, S.AMG_OP),
        "level L": lambda: matrix(L, S.AMG_OP),
        "matrix 99": lambda: matrix(0, 99),
        "prolongator of the coarsest": lambda: matrix(L - 1, S.AMG_PROLONG),
        "tentative of the coarsest": lambda: matrix(L - 1, S.AMG_TENTATIVE),
        "coarse inverse on level 0": lambda: matrix(0, S.AMG_COARSE_INV),
        "aggregates of the coarsest": lambda: aggregates(L - 1),
        "aggregates of level -1": lambda: aggregates(-1),
    }
    got = {}
    for name, call in calls.items():
        with pytest.raises(SpkError) as e:
            call()
        got[name] = (e.value.code, str(e.value))
    return got


REFUSED_16 = {   # laplace(16): 2 levels
    "level -1": "amg: level -1 outside [0,2)",
    "level L": "amg: level 2 outside [0,2)",
    "matrix 99": "amg: unknown matrix 99",
    "prolongator of the coarsest": "amg: the coarsest level has no prolongator",
    "tentative of the coarsest": "amg: the coarsest level has no prolongator",
    "coarse inverse on level 0": "amg: the coarse inverse lives on level 1",
    "aggregates of the coarsest": "amg: level 1 has no aggregates",
    "aggregates of level -1": "amg: level -1 has no aggregates",
}


def test_level_accessors_refuse_what_is_not_there():
    A, _, _ = laplace(16)
    h = S.AmgHierarchy(A)
    info = h.info()
    assert info["levels"] == 2 and info["rows"] == [512, 50] and info["block_size"] == 2
    got = refused_queries(h.matrix, h.aggregates, 2)
    h.close()
    assert set(got) == set(REFUSED_16)
    for name, (code, msg) in got.items():
        assert code == SPK_ERR_ARG and msg == f"libspk error {SPK_ERR_ARG}: {REFUSED_16[name]}", name


@pytest.mark.parametrize("prefix", ["", "-fieldsplit_0_"])
def test_facade_reads_the_route(prefix):
    k = S.KSP()
    pc = ["-pc_type", "gamg"] if not prefix else ["-pc_type", "fieldsplit", "-fieldsplit_0_pc_type", "gamg"]
    k.setFromOptions(["-ksp_type", "fgmres"] + pc + [prefix + "spk_gamg_setup" if prefix else "-spk_gamg_setup", "device"])
    got, sel = k.getAMGOptions(fieldsplit0=bool(prefix))
    other, osel = k.getAMGOptions(fieldsplit0=not prefix)
    assert sel and not osel
    assert got["setup"] == S.AMG_SETUP_DEVICE and other["setup"] == S.AMG_SETUP_HOST
    assert got["smooth_its"] == 2 and got["nsmooths"] == 1          # nothing else moved
    k.setFromOptions([prefix + "spk_gamg_setup" if prefix else "-spk_gamg_setup", "host"])
    assert k.getAMGOptions(fieldsplit0=bool(prefix))[0]["setup"] == S.AMG_SETUP_HOST
    k.destroy()


@pytest.mark.parametrize("opts,code", [(["-spk_gamg_setup", "gpu"], SPK_ERR_UNSUPPORTED),
                                       (["-fieldsplit_0_spk_gamg_setup", "2"], SPK_ERR_UNSUPPORTED),
                                       (["-spk_gamg_setup"], SPK_ERR_ARG)])
def test_facade_refuses_an_unknown_route(opts, code):
    k = S.KSP()
    with pytest.raises(SpkError) as e:
        k.setFromOptions(["-ksp_type", "fgmres", "-pc_type", "gamg"] + opts)
    assert e.value.code == code and opts[0] in str(e.value)
    k.destroy()
