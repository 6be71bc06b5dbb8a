"""-ksp_type pipecgrr without a GPU: the numpy restatement of pipelined CG with residual replacement (pipecg_ref plus
a measured gap check every check_every iterations) that the GPU tests compare the device solver with, the tau rule it
was chosen by, the facade's option handling and KSP / PC checks, and the C ABI (spk_pipecgrr) as a C99 caller sees
it."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, relerr
from test_minres_cpu import scipy_K
from test_pipecg_cpu import pipecg_ref

TAU = 1e-6   # -spk_pipecgrr_tau default (chosen on this reference)


def pipecgrr_ref(K, M, b, x0=None, rtol=1e-8, abstol=1e-50, dtol=1e4, max_it=10000, norm="unpreconditioned", urec=False,
                 tau=TAU, check_every=16, iterates=None):
    """Pipelined CG with residual replacement as spk_pipecgrr runs it (include/spk.h): test_pipecg_cpu.pipecg_ref, plus
    after every check_every-th iteration of a recurrence (counted from its start) t = K x and the measured gap
    f = ||(b - t) - r||.  A check replaces when f > tau ||r|| and the check before it in the recurrence found f <= tau ||r||
    (the crossing of van der Vorst and Ye, on the measured gap: once the gap sits at the noise floor of fl(b - K x) near
    the attainable accuracy, a replacement cannot lower it and the crossing rule stops replacing).  A replacement recomputes r = b - t, u = M^-1 r, w = K u, s = K p, q = M^-1 s, z = K q
    from their definitions, keeps x and p, and forms beta and alpha from the fresh gamma = <r, u>, delta = <w, u> as after
    a normal iteration.  It is no iteration and no start.  Returns x and a dict like Context.pipecgrr, with `replaced`:
    the iteration counts after which a replacement ran."""
    return pipecg_ref(K, M, b, x0=x0, rtol=rtol, abstol=abstol, dtol=dtol, max_it=max_it, norm=norm, urec=urec, tau=tau,
                      check_every=check_every, iterates=iterates)


def pcg_textbook_its(K, M, b, rtol, norm="unpreconditioned", max_it=100000):
    """Hestenes-Stiefel preconditioned CG from x = 0: iterations until the recursive residual meets rtol in `norm`."""
    x = np.zeros_like(b)
    r = b.copy()
    z = M(r)
    p = z.copy()
    rz = r @ z

    def nrm():
        return np.sqrt(abs(rz)) if norm == "natural" else np.linalg.norm(r)

    ttol = rtol * nrm()
    for k in range(1, max_it + 1):
        q = K(p)
        a = rz / (p @ q)
        x = x + a * p
        r = r - a * q
        z = M(r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
        if nrm() <= ttol:
            return k
    return max_it


@pytest.fixture(scope="module")
def laplace64(spk):
    A, f = spk.AssembleOperator_Laplace(64)
    Ka = scipy_K(A).tocsr()
    return Ka, f, 1.0 / Ka.diagonal()


@pytest.mark.parametrize("norm", ["unpreconditioned", "natural"])
@pytest.mark.parametrize("pc", ["jacobi", "none"])
def test_reference_matches_direct_solve(laplace64, norm, pc):
    from scipy.sparse.linalg import spsolve
    Ka, f, d = laplace64
    M = (lambda v: d * v) if pc == "jacobi" else (lambda v: v.copy())
    xd = spsolve(Ka.tocsc(), f)
    for urec in (False, True):
        x, info = pipecgrr_ref(lambda v: Ka @ v, M, f, rtol=1e-10, norm=norm, urec=urec)
        assert info["reason"] == 2 and relerr(x, xd) < 1e-8, (urec, info["its"], relerr(x, xd))
        assert len(info["history"]) == info["its"] + 1 and info["cycles"] >= 1
        r = f - Ka @ x
        true = np.linalg.norm(r) if norm == "unpreconditioned" else np.sqrt(M(r) @ r)
        assert info["rnorm"] == pytest.approx(true, rel=1e-12)


def test_replacement_keeps_the_krylov_space(laplace64):
    """tau = 0: the first check replaces, and as the gap never falls back to 0 the crossing rule replaces no more; the
    iterates still follow textbook PCG across the replacement (a restart would not)."""
    from test_pipecg_cpu import pcg_textbook
    Ka, f, d = laplace64
    K, M = (lambda v: Ka @ v), (lambda v: d * v)
    ref = pcg_textbook(K, M, f, 80)
    for urec in (False, True):
        its = []
        _, info = pipecgrr_ref(K, M, f, rtol=0.0, abstol=0.0, max_it=80, urec=urec, tau=0.0, iterates=its)
        assert info["replaced"] == [16] and info["cycles"] == 1
        for k, (a, b) in enumerate(zip(its, ref)):
            assert relerr(a, b) < 1e-8, (urec, k, relerr(a, b))


@pytest.mark.parametrize("rtol", [1e-8, 1e-10])
@pytest.mark.parametrize("pc", ["jacobi", "none"])
def test_tau_rule_at_256(spk, pc, rtol):
    """The default tau: iterations within 2 % of textbook PCG, at most one replacement per 100 iterations, one start
    (DESIGN.md section 13 records 512^2 and 1024^2 as well)."""
    A, f = spk.AssembleOperator_Laplace(256)
    Ka = scipy_K(A).tocsr()
    d = 1.0 / Ka.diagonal()
    K, M = (lambda v: Ka @ v), ((lambda v: d * v) if pc == "jacobi" else (lambda v: v.copy()))
    x, info = pipecgrr_ref(K, M, f, rtol=rtol, max_it=20000)
    ref = pcg_textbook_its(K, M, f, rtol)
    assert info["reason"] == 2 and info["cycles"] == 1, info["cycles"]
    assert abs(info["its"] - ref) <= 0.02 * ref, (info["its"], ref)
    assert 100 * info["replacements"] <= info["its"], info["replaced"]
    assert np.linalg.norm(f - K(x)) <= rtol * np.linalg.norm(f) * (1 + 1e-9)


def test_ksp_type_pipecgrr_is_accepted_and_read_back(spk):
    k = spk.KSP()
    k.setFromOptions("-ksp_type pipecgrr -pc_type jacobi -ksp_rtol 1e-8")
    assert k.getType() == "pipecgrr" and k.getNormType() == "unpreconditioned"
    k.setFromOptions("-ksp_norm_type natural -spk_pipecgrr_tau 1e-4")
    assert k.getType() == "pipecgrr" and k.getNormType() == "natural"
    k.setFromOptions("-ksp_type pipecg")
    assert k.getType() == "pipecg"
    k.setFromOptions("-ksp_type pipecgrr -pc_type gamg")
    assert k.getType() == "pipecgrr"
    for bad, code in (("-ksp_type cg", -6), ("-ksp_norm_type preconditioned", -6), ("-spk_pipecgrr_tau -1", -1),
                      ("-spk_pipecgrr_tau x", -1), ("-spk_pipecgrr_tau inf", -1)):
        with pytest.raises(spk.SpkError) as ei:
            k.setFromOptions(bad)
        assert ei.value.code == code, bad
    k.destroy()


@pytest.mark.parametrize("opts,what", [
    ("-pc_type fieldsplit -pc_fieldsplit_schur_fact_type diag", "fieldsplit"),
    ("-pc_type fieldsplit", "fieldsplit"),
    ("-pc_type jacobi -fieldsplit_0_ksp_type richardson -fieldsplit_0_ksp_max_it 2", "inner"),
    ("-pc_type none -spk_inner_sweeps 3", "inner"),
    ("-pc_type jacobi -ksp_pc_side right", "left"),
    ("-pc_type gamg -ksp_pc_side right -ksp_norm_type natural", "left"),
])
def test_setup_refuses_pipecgrr_combinations_before_operators(spk, opts, what):
    k = spk.KSP()
    k.setFromOptions("-ksp_type pipecgrr " + opts)
    with pytest.raises(spk.SpkError) as ei:
        k.setUp()
    assert ei.value.code == -6
    msg = str(ei.value)
    assert "pipecgrr" in msg and what in msg, msg
    k.destroy()


@pytest.mark.parametrize("ok", ["-pc_type none", "-pc_type jacobi", "-pc_type gamg",
                                "-pc_type jacobi -ksp_norm_type natural -spk_pipecgrr_tau 1e-3"])
def test_setup_lets_pipecgrr_with_symmetric_pcs_through(spk, ok):
    k = spk.KSP()
    k.setFromOptions("-ksp_type pipecgrr " + ok)
    with pytest.raises(spk.SpkError, match="KSPSetOperators") as ei:
        k.setUp()
    assert ei.value.code == -3
    k.destroy()


def test_tau_setting_is_checked(spk):
    assert spk.lib.spk_pipecgrr_set_tau(None, 1e-6) == -1   # SPK_ERR_ARG: no context
    assert spk.PIPECGRR_TAU_DEFAULT == TAU


C99_CALLER = r"""
#include <stdio.h>
#include "spk.h"
#include "spk_ksp.h"
int main(void)
{
    spk_opts o;
    spk_result r;
    double h[4];
    int32_t nrep = -1;
    const char *t = 0;
    int32_t nt = -1;
    SpkKSP k = 0;
    const char *argv[] = {"-ksp_type", "pipecgrr", "-spk_pipecgrr_tau", "1e-5"};
    int (*fn)(spk_ctx *, const double *, double *, int, const spk_opts *, int, spk_result *, double *, int32_t,
              int32_t *) = spk_pipecgrr;
    spk_default_opts(&o);
    if (fn(0, h, h, SPK_MEM_HOST, &o, SPK_NORM_NATURAL, &r, h, 4, &nrep) != SPK_ERR_ARG) return 3;   /* null context */
    if (spk_pipecgrr_set_tau(0, SPK_PIPECGRR_TAU_DEFAULT) != SPK_ERR_ARG) return 4;
    if (SpkKSPCreate(0, &k) != SPK_OK || SpkKSPSetFromOptions(k, 4, argv) != SPK_OK) return 5;
    if (SpkKSPGetType(k, &t, &nt) != SPK_OK || nt != SPK_NORM_UNPRECONDITIONED) return 6;
    printf("%s\n", t);
    SpkKSPDestroy(&k);
    return 0;
}
"""


def test_c99_caller_compiles_links_and_runs(spk, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    src = tmp_path / "caller.c"
    src.write_text(C99_CALLER)
    libdir = os.path.dirname(spk.LIB_PATH)
    exe = tmp_path / "caller"
    out = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                          "-o", str(exe), "-L", libdir, "-lspk", "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "pipecgrr", (run.returncode, run.stdout, run.stderr)
