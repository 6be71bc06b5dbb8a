"""-ksp_type pipecg without a GPU: option handling and the KSP / PC compatibility checks of the facade, the C ABI
(spk_pipecg, SPK_DIVERGED_INDEFINITE_MAT) as a C99 caller sees it, and the numpy restatement of the preconditioned
pipelined CG recurrence (Ghysels-Vanroose Alg. 3, in PETSc's KSPSolve_PIPECG order) that the GPU tests compare the
device solver with."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, relerr
from test_minres_cpu import scipy_K


def pipecg_ref(K, M, b, x0=None, rtol=1e-8, abstol=1e-50, dtol=1e4, max_it=10000, norm="unpreconditioned", urec=True,
               tau=None, check_every=16, iterates=None):
    """Preconditioned pipelined CG as spk_pipecg runs it (include/spk.h): K, M are callables (operator, M^-1).  urec:
    u and q kept as recurrences (u -= alpha q; the V-cycle path); False: u = M^-1 r recomputed after every update (the
    diagonal path, where the pass forms u = D r).  The test is KSPConvergedDefault in the chosen norm; a convergence or
    max_it seen by the recurrence is confirmed on b - K x, and the recurrence restarts from x when that misses.
    tau (None: pipecg, no gap check): spk_pipecgrr's residual replacement, see test_pipecgrr_cpu.pipecgrr_ref.
    iterates: a list that receives x after every iteration.  Returns x and a dict like Context.pipecg, plus
    `replacements` and `replaced`: the iteration counts after which a replacement ran."""
    natural = norm == "natural"
    x = np.zeros_like(b) if x0 is None else np.array(x0, float)

    def nrm(r, g):
        return np.sqrt(abs(g)) if natural else np.linalg.norm(r)

    bnorm = nrm(b, M(b) @ b) if x0 is not None else 0.0
    hist, its, starts, reason, final, replaced = [], 0, 0, 0, False, []
    r = b - K(x)
    u = M(r)
    gamma = r @ u
    rn = nrm(r, gamma)
    rnorm0 = rn
    cnorm0 = bnorm if (x0 is not None and bnorm != 0.0) else rn
    ttol = max(rtol * cnorm0, abstol)
    hist.append(rn)

    def conv(v):
        if not np.isfinite(v):
            return -9
        if v <= ttol:
            return 3 if v < abstol else 2
        return -4 if v >= dtol * cnorm0 else 0

    while True:
        rn = nrm(r, gamma)
        if final:
            break
        reason = -8 if gamma < 0 else conv(rn)
        if not reason and its >= max_it:
            reason = -3
        if not reason and not gamma > 0:
            reason = -5
        if reason:
            break
        starts += 1
        w = K(u)
        delta = w @ u
        if not delta > 0:
            reason = -10
            break
        alpha, beta, gamma_old, first = gamma / delta, 0.0, gamma, True
        j, above = 0, False
        while True:
            m = M(w)
            n = K(m)
            if first:
                z, q, s, p = n.copy(), m.copy(), w.copy(), u.copy()
            else:
                z, q, s, p = n + beta * z, m + beta * q, w + beta * s, u + beta * p
            x = x + alpha * p
            r = r - alpha * s
            u = u - alpha * q if urec else M(r)
            w = w - alpha * z
            if iterates is not None:
                iterates.append(x.copy())
            gamma, delta = r @ u, w @ u
            its += 1
            j += 1
            rn = nrm(r, gamma)
            hist.append(rn)
            reason = -8 if gamma < 0 else conv(rn)
            if reason < 0:
                final = True
            elif not reason and its >= max_it:
                reason = -3
            if not reason and not gamma > 0:
                reason, final = -5, True
            if reason:
                break
            beta = gamma / gamma_old
            den = delta - beta * gamma / alpha
            if not den > 0:   # after the first pass: the residual gap, b - K x decides (confirmation or restart)
                reason, final = -10, first
                break
            alpha_old, gamma_oold = alpha, gamma_old
            alpha, gamma_old, first = gamma / den, gamma, False
            if tau is None or j % check_every:
                continue
            # ---- the gap check, and the replacement it may trigger ----
            t = K(x)
            was, above = above, bool(np.linalg.norm((b - t) - r) > tau * np.linalg.norm(r))
            if was or not above:
                continue
            replaced.append(its)
            r = b - t
            u = M(r)
            w = K(u)
            s = K(p)
            q = M(s)
            z = K(q)
            gamma, delta = r @ u, w @ u
            if gamma < 0:
                reason, final = -8, True
            elif not gamma > 0:
                reason, final = -5, True
            if reason:
                break
            beta = gamma / gamma_oold
            den = delta - beta * gamma / alpha_old
            if not den > 0:
                reason = -10
                break
            alpha, gamma_old = gamma / den, gamma
        r = b - K(x)
        u = M(r)
        gamma = r @ u
    return x, dict(its=its, reason=reason, rnorm=rn, rnorm0=rnorm0, cycles=starts, history=np.array(hist),
                   replacements=len(replaced), replaced=replaced)


def pcg_textbook(K, M, b, its):
    """Hestenes-Stiefel preconditioned CG from x = 0: the iterates x_1 .. x_its."""
    x = np.zeros_like(b)
    r = b.copy()
    z = M(r)
    p = z.copy()
    rz = r @ z
    out = []
    for _ in range(its):
        q = K(p)
        a = rz / (p @ q)
        x = x + a * p
        r = r - a * q
        z = M(r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
        out.append(x.copy())
    return out


@pytest.fixture(scope="module")
def laplace64(spk):
    A, f = spk.AssembleOperator_Laplace(64)
    Ka = scipy_K(A).tocsr()
    return Ka, f, 1.0 / Ka.diagonal()


@pytest.mark.parametrize("norm", ["unpreconditioned", "natural"])
@pytest.mark.parametrize("pc", ["jacobi", "none"])
def test_reference_recurrence_matches_direct_solve(laplace64, norm, pc):
    from scipy.sparse.linalg import spsolve
    Ka, f, d = laplace64
    M = (lambda v: d * v) if pc == "jacobi" else (lambda v: v.copy())
    xd = spsolve(Ka.tocsc(), f)
    for urec in (False, True):
        x, info = pipecg_ref(lambda v: Ka @ v, M, f, rtol=1e-10, norm=norm, urec=urec)
        assert info["reason"] == 2 and relerr(x, xd) < 1e-8, (urec, info["its"], relerr(x, xd))
        assert len(info["history"]) == info["its"] + 1 and info["cycles"] >= 1
        r = f - Ka @ x
        true = np.linalg.norm(r) if norm == "unpreconditioned" else np.sqrt(M(r) @ r)
        assert info["rnorm"] == pytest.approx(true, rel=1e-12)


def test_reference_iterates_match_textbook_pcg(laplace64):
    Ka, f, d = laplace64
    K, M = (lambda v: Ka @ v), (lambda v: d * v)
    ref = pcg_textbook(K, M, f, 50)
    for urec in (False, True):
        its = []
        pipecg_ref(K, M, f, rtol=0.0, abstol=0.0, max_it=50, urec=urec, iterates=its)
        assert len(its) == 50
        for k, (a, b) in enumerate(zip(its, ref)):
            assert relerr(a, b) < 1e-8, (urec, k, relerr(a, b))


def test_reference_cutoffs_and_reasons(laplace64):
    Ka, f, d = laplace64
    K = lambda v: Ka @ v  # noqa: E731
    x, info = pipecg_ref(K, lambda v: d * v, f, rtol=0.0, abstol=0.0, max_it=25)
    assert info["reason"] == -3 and info["its"] == 25 and len(info["history"]) == 26
    # K = -A: an indefinite Jacobi preconditioner (-8), an indefinite matrix without one (-10)
    Kn = lambda v: -(Ka @ v)  # noqa: E731
    _, info = pipecg_ref(Kn, lambda v: -d * v, -f)
    assert info["reason"] == -8
    _, info = pipecg_ref(Kn, lambda v: v.copy(), -f)
    assert info["reason"] == -10
    # a nonzero guess: rtol refers to ||b||
    xs, _ = pipecg_ref(K, lambda v: d * v, f, rtol=1e-10)
    x0 = xs * (1.0 + 1e-3 * np.sin(0.37 * np.arange(len(xs))))
    x, info = pipecg_ref(K, lambda v: d * v, f, x0=x0, rtol=1e-8)
    assert info["reason"] == 2 and info["rnorm"] <= 1e-8 * np.linalg.norm(f)


def test_ksp_type_pipecg_is_accepted_and_read_back(spk):
    k = spk.KSP()
    k.setFromOptions("-ksp_type pipecg -pc_type jacobi -ksp_rtol 1e-8")
    assert k.getType() == "pipecg" and k.getNormType() == "unpreconditioned"
    k.setFromOptions("-ksp_norm_type natural")
    assert k.getType() == "pipecg" and k.getNormType() == "natural"
    k.setFromOptions("-ksp_norm_type unpreconditioned -pc_type gamg")
    assert k.getType() == "pipecg" and k.getNormType() == "unpreconditioned"
    for bad in ("-ksp_type cg", "-ksp_norm_type preconditioned", "-ksp_pc_side left"):
        with pytest.raises(spk.SpkError) as ei:
            k.setFromOptions(bad)
        assert ei.value.code == -6
    k.destroy()
    assert spk.lib.SpkKSPConvergedReasonName(-10) == b"DIVERGED_INDEFINITE_MAT"
    assert spk.DIVERGED_INDEFINITE_MAT == -10


@pytest.mark.parametrize("opts,what", [
    ("-pc_type fieldsplit -pc_fieldsplit_schur_fact_type diag", "fieldsplit"),
    ("-pc_type fieldsplit", "fieldsplit"),
    ("-pc_type jacobi -fieldsplit_0_ksp_type richardson -fieldsplit_0_ksp_max_it 2", "inner"),
    ("-pc_type none -spk_inner_sweeps 3", "inner"),
    ("-pc_type jacobi -ksp_pc_side right", "left"),
    ("-pc_type gamg -ksp_pc_side right -ksp_norm_type natural", "left"),
])
def test_setup_refuses_pipecg_combinations_before_operators(spk, opts, what):
    """Checked at KSPSetUp before the operators are looked at: no GPU, no operators needed."""
    k = spk.KSP()
    k.setFromOptions("-ksp_type pipecg " + opts)
    with pytest.raises(spk.SpkError) as ei:
        k.setUp()
    assert ei.value.code == -6
    msg = str(ei.value)
    assert "pipecg" in msg and what in msg
    k.destroy()


@pytest.mark.parametrize("ok", ["-pc_type none", "-pc_type jacobi", "-pc_type gamg",
                                "-pc_type jacobi -ksp_norm_type natural", "-pc_type gamg -ksp_norm_type natural"])
def test_setup_lets_pipecg_with_symmetric_pcs_through(spk, ok):
    k = spk.KSP()
    k.setFromOptions("-ksp_type pipecg " + ok)
    with pytest.raises(spk.SpkError, match="KSPSetOperators") as ei:
        k.setUp()
    assert ei.value.code == -3
    k.destroy()


def test_cg_stays_refused(spk):
    k = spk.KSP()
    with pytest.raises(spk.SpkError) as ei:
        k.setFromOptions("-ksp_type cg -pc_type jacobi")
    assert ei.value.code == -6
    k.destroy()


C99_CALLER = r"""
#include <stdio.h>
#include "spk.h"
#include "spk_ksp.h"
int main(void)
{
    spk_opts o;
    spk_result r;
    double h[4];
    const char *t = 0;
    int32_t nt = -1;
    SpkKSP k = 0;
    const char *argv[] = {"-ksp_type", "pipecg", "-ksp_norm_type", "natural"};
    int (*fn)(spk_ctx *, const double *, double *, int, const spk_opts *, int, spk_result *, double *, int32_t) = spk_pipecg;
    spk_default_opts(&o);
    if (SPK_DIVERGED_INDEFINITE_MAT != -10) return 2;
    if (fn(0, h, h, SPK_MEM_HOST, &o, SPK_NORM_NATURAL, &r, h, 4) != SPK_ERR_ARG) return 3;   /* null context */
    if (SpkKSPCreate(0, &k) != SPK_OK || SpkKSPSetFromOptions(k, 4, argv) != SPK_OK) return 4;
    if (SpkKSPGetType(k, &t, &nt) != SPK_OK || nt != SPK_NORM_NATURAL) return 5;
    printf("%s %s\n", t, SpkKSPConvergedReasonName(SPK_DIVERGED_INDEFINITE_MAT));
    SpkKSPDestroy(&k);
    return 0;
}
"""


def test_c99_caller_compiles_and_links(spk, tmp_path):
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
    assert exe.exists()
