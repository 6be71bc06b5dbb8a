"""-pc_fieldsplit_schur_precondition full | selfp and -fieldsplit_1_pc_type jacobi | cholesky | lu in the KSP facade,
without a GPU: the options read back as they resolve, and the pairings that make no sense are refused by KSPSetUp before
any context exists (a pairing that is accepted gets as far as "KSPSetOperators has not been called")."""
import pytest

import saddle_point_petsc_amd as S
from saddle_point_petsc_amd._lib import SpkError

SPK_ERR_ARG, SPK_ERR_STATE, SPK_ERR_UNSUPPORTED = -1, -3, -6
FS = ["-ksp_type", "fgmres", "-pc_type", "fieldsplit", "-pc_fieldsplit_type", "schur"]
PRE, PC1 = "-pc_fieldsplit_schur_precondition", "-fieldsplit_1_pc_type"


@pytest.mark.parametrize("opts,want", [
    ([], ("selfp", "jacobi")),
    ([PRE, "selfp"], ("selfp", "jacobi")),
    ([PRE, "full"], ("full", "cholesky")),                 # left out, the split's solver follows the precondition
    ([PRE, "full", PC1, "cholesky"], ("full", "cholesky")),
    ([PRE, "full", PC1, "lu"], ("full", "cholesky")),      # lu and cholesky both mean the dense factor
    ([PC1, "lu", PRE, "full"], ("full", "cholesky")),      # in either order
    ([PRE, "selfp", PC1, "jacobi"], ("selfp", "jacobi")),
    ([PRE, "full", PC1, "jacobi"], ("full", "jacobi")),    # read back as given; refused at KSPSetUp
    ([PRE, "full", PRE, "selfp"], ("selfp", "jacobi")),    # the last one given holds
])
def test_facade_reads_back_the_two_options(opts, want):
    k = S.KSP()
    k.setFromOptions(FS + opts)
    assert k.getSchurPre() == want
    _, pct, _ = k.getOptions()
    assert pct == S.PC_SCHUR
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


def test_bad_pairings_refused_before_any_gpu_work():
    code, msg = _setup_code(FS + [PRE, "full", PC1, "jacobi"])
    assert code == SPK_ERR_UNSUPPORTED and PRE in msg and PC1 in msg
    for dense in ("cholesky", "lu"):
        code, msg = _setup_code(FS + [PRE, "selfp", PC1, dense])
        assert code == SPK_ERR_UNSUPPORTED and PRE in msg and PC1 in msg
        code, msg = _setup_code(FS + [PC1, dense])             # selfp by default
        assert code == SPK_ERR_UNSUPPORTED and PRE in msg and PC1 in msg
    # the FP32 inner sweeps are no linear operator in FP64: no exact complement of them
    code, msg = _setup_code(FS + [PRE, "full", "-fieldsplit_0_ksp_type", "richardson", "-fieldsplit_0_ksp_max_it", "3"])
    assert code == SPK_ERR_UNSUPPORTED and "FP32" in msg and PRE in msg
    # minres takes the symmetric factorisation only, dense S or not
    code, msg = _setup_code(["-ksp_type", "minres"] + FS[2:] + [PRE, "full"])
    assert code == SPK_ERR_UNSUPPORTED and "minres" in msg


@pytest.mark.parametrize("opts", [
    [PRE, "full"], [PRE, "full", PC1, "cholesky"], [PRE, "full", PC1, "lu"], [PRE, "selfp"], [PRE, "selfp", PC1, "jacobi"],
    [PRE, "full", "-fieldsplit_0_pc_type", "gamg"],
])
def test_good_pairings_get_as_far_as_the_operators(opts):
    code, msg = _setup_code(FS + opts)
    assert code == SPK_ERR_STATE and "KSPSetOperators" in msg
    code, msg = _setup_code(["-ksp_type", "minres"] + FS[2:] + ["-pc_fieldsplit_schur_fact_type", "diag"] + opts[:2])
    assert code == SPK_ERR_STATE and "KSPSetOperators" in msg


@pytest.mark.parametrize("opts,code", [
    ([PRE, "a11"], SPK_ERR_UNSUPPORTED),
    ([PRE, "user"], SPK_ERR_UNSUPPORTED),
    ([PRE, "self"], SPK_ERR_UNSUPPORTED),
    ([PRE], SPK_ERR_ARG),
    ([PC1, "ilu"], SPK_ERR_UNSUPPORTED),
    ([PC1, "gamg"], SPK_ERR_UNSUPPORTED),
    ([PC1], SPK_ERR_ARG),
])
def test_unknown_values_refused_at_set_from_options(opts, code):
    k = S.KSP()
    with pytest.raises(SpkError) as e:
        k.setFromOptions(FS + opts)
    assert e.value.code == code
    k.destroy()


def test_context_binding_rejects_an_unknown_precondition():
    with pytest.raises(ValueError):
        S.Context.pc_setup(None, S.PC_SCHUR, schur_pre="a11")
