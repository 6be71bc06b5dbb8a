"""-ksp_type minres without a GPU: option handling and the KSP / PC compatibility checks of the facade, the C ABI
(spk_minres, SPK_NORM_*, SPK_DIVERGED_INDEFINITE_PC) as a C99 caller sees it, and the numpy restatement of the
preconditioned MINRES recurrence (Elman-Silvester-Wathen Alg. 4.1) that the GPU tests compare the device solver with."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, relerr


def minres_ref(K, M, b, x0=None, rtol=1e-8, abstol=1e-50, dtol=1e4, max_it=10000, norm="unpreconditioned"):
    """Preconditioned MINRES as spk_minres runs it (include/spk.h): K, M are callables (operator, M^-1).  The test is
    KSPConvergedDefault in the chosen norm; a convergence or max_it seen by the recurrence is confirmed on b - K x, and
    the recurrence restarts from x when that misses.  Returns x and a dict like Context.minres."""
    natural = norm == "natural"
    x = np.zeros_like(b) if x0 is None else np.array(x0, float)

    def nrm(r, z):
        return np.sqrt(abs(z @ r)) if natural else np.linalg.norm(r)

    bnorm = nrm(b, M(b)) if x0 is not None else 0.0
    hist, its, starts, reason, final = [], 0, 0, 0, False
    r = b - K(x)
    z = M(r)
    rn = nrm(r, z)
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
        zr = z @ r
        rn = nrm(r, z)
        if final:
            break
        reason = -8 if zr < 0 else conv(rn)
        if not reason and its >= max_it:
            reason = -3
        if not reason and not zr > 0:
            reason = -5
        if reason:
            break
        starts += 1
        gam, gam_prev, eta = np.sqrt(zr), 1.0, np.sqrt(zr)
        c0 = c1 = 1.0
        s0 = s1 = 0.0
        v_prev, v, zc = np.zeros_like(b), r.copy(), z.copy()
        w_prev, w, kw_prev, kw, rr = np.zeros_like(b), np.zeros_like(b), np.zeros_like(b), np.zeros_like(b), r.copy()
        first = True
        while True:
            zs = zc / gam
            q = K(zs)
            delta = q @ zs
            vn = q - (delta / gam) * v - (0.0 if first else gam / gam_prev) * v_prev
            zn = M(vn)
            zv = zn @ vn
            if zv < 0:
                reason, final = -8, True
                break
            gn = np.sqrt(zv)
            a0 = c1 * delta - c0 * s1 * gam
            a1 = np.sqrt(a0 * a0 + gn * gn)
            a2 = s1 * delta + c0 * c1 * gam
            a3 = s0 * gam
            cn, sn = a0 / a1, gn / a1
            wn = (zs - a3 * w_prev - a2 * w) / a1
            x = x + cn * eta * wn
            if not natural:
                kwn = (q - a3 * kw_prev - a2 * kw) / a1
                rr = rr - cn * eta * kwn
                kw_prev, kw = kw, kwn
            eta = -sn * eta
            w_prev, w = w, wn
            v_prev, v, zc = v, vn, zn
            c0, c1, s0, s1 = c1, cn, s1, sn
            gam_prev, gam, first = gam, gn, False
            its += 1
            rn = abs(eta) if natural else np.linalg.norm(rr)
            hist.append(rn)
            reason = conv(rn)
            if gn == 0.0:
                reason, final = 7, True
            elif reason < 0:
                final = True
            elif not reason and its >= max_it:
                reason = -3
            if reason:
                break
        r = b - K(x)
        z = M(r)
    return x, dict(its=its, reason=reason, rnorm=rn, rnorm0=rnorm0, cycles=starts, history=np.array(hist))


def scipy_K(A, B=None):
    import scipy.sparse as sp
    a = sp.csr_matrix((A.val, A.colidx, A.rowptr), shape=(A.nrows, A.ncols))
    if B is None:
        return a.tocsc()
    bm = sp.csr_matrix((B.val, B.colidx, B.rowptr), shape=(B.nrows, B.ncols))
    return sp.bmat([[a, bm.T], [bm, None]]).tocsc()


def test_reference_recurrence_matches_direct_solve(spk):
    """The numpy restatement on the 64 x 64 saddle system with the Schur DIAG preconditioner (both norms) and on
    K = A with Jacobi: x agrees with scipy's sparse direct solve."""
    from scipy.sparse.linalg import spsolve
    A, f = spk.AssembleOperator_Laplace(64)
    B, g = spk.AssembleOperator_Constraints(64)
    K = scipy_K(A, B)
    rhs = np.concatenate([f, g])
    d = 1.0 / K.diagonal()[:A.nrows]
    Bd = scipy_K(B).tocsr()
    shat = np.asarray(Bd.multiply(Bd).multiply(d[None, :]).sum(axis=1)).ravel()   # diag(B diag(A)^-1 B^T)
    n = A.nrows

    def M(v):
        return np.concatenate([d * v[:n], v[n:] / shat])

    xd = spsolve(K, rhs)
    for norm in ("unpreconditioned", "natural"):
        x, info = minres_ref(lambda v: K @ v, M, rhs, rtol=1e-12, norm=norm)
        assert info["reason"] == 2 and relerr(x, xd) < 1e-8, (norm, info["its"], relerr(x, xd))
        assert len(info["history"]) == info["its"] + 1
    x, info = minres_ref(lambda v: K @ v, M, rhs, rtol=0.0, abstol=0.0, max_it=25)
    assert info["reason"] == -3 and info["its"] == 25
    Ka = scipy_K(A)
    x, info = minres_ref(lambda v: Ka @ v, lambda v: d * v, f, rtol=1e-12)
    assert info["reason"] == 2 and relerr(x, spsolve(Ka, f)) < 1e-8
    # an indefinite preconditioner is a reason, not an error
    _, info = minres_ref(lambda v: Ka @ v, lambda v: -d * v, f, rtol=1e-8)
    assert info["reason"] == -8


def test_ksp_type_minres_is_accepted_and_read_back(spk):
    k = spk.KSP()
    assert k.getType() == ""
    k.setFromOptions("-ksp_type minres -pc_type fieldsplit -pc_fieldsplit_schur_fact_type diag -ksp_rtol 1e-8")
    assert k.getType() == "minres" and k.getNormType() == "unpreconditioned"
    k.setFromOptions("-ksp_norm_type natural")
    assert k.getNormType() == "natural"
    k.setFromOptions("-ksp_norm_type unpreconditioned -ksp_type fgmres")
    assert k.getType() == "fgmres" and k.getNormType() == "unpreconditioned"
    for bad in ("-ksp_type cg", "-ksp_norm_type preconditioned", "-ksp_type"):
        with pytest.raises(spk.SpkError):
            k.setFromOptions(bad)
    k.destroy()
    assert spk.lib.SpkKSPConvergedReasonName(-8) == b"DIVERGED_INDEFINITE_PC"
    assert (spk.NORM_UNPRECONDITIONED, spk.NORM_NATURAL, spk.DIVERGED_INDEFINITE_PC) == (0, 1, -8)


@pytest.mark.parametrize("opts,what", [
    ("-pc_type fieldsplit -pc_fieldsplit_schur_fact_type full", "full"),
    ("-pc_type fieldsplit -pc_fieldsplit_schur_fact_type lower", "lower"),
    ("-pc_type fieldsplit -pc_fieldsplit_schur_fact_type upper", "upper"),
    ("-pc_type fieldsplit", "full"),   # the facade's default factorisation
    ("-pc_type jacobi -fieldsplit_0_ksp_type richardson -fieldsplit_0_ksp_max_it 2", "inner sweeps"),
    ("-pc_type fieldsplit -pc_fieldsplit_schur_fact_type diag -spk_inner_sweeps 3", "inner sweeps"),
])
def test_setup_refuses_minres_with_a_nonsymmetric_pc(spk, opts, what):
    """Checked at KSPSetUp before the operators are looked at: no GPU, no operators needed."""
    k = spk.KSP()
    k.setFromOptions("-ksp_type minres " + opts)
    with pytest.raises(spk.SpkError) as ei:
        k.setUp()
    assert ei.value.code == -6
    msg = str(ei.value)
    assert "minres" in msg and ("-ksp_type fgmres" in msg)
    if what != "inner sweeps":
        assert what in msg and "diag" in msg
    k.destroy()
    # the symmetric ones get past the check (to the missing operators)
    for ok in ("-pc_type none", "-pc_type jacobi", "-pc_type fieldsplit -pc_fieldsplit_schur_fact_type diag"):
        k = spk.KSP()
        k.setFromOptions("-ksp_type minres " + ok)
        with pytest.raises(spk.SpkError, match="KSPSetOperators"):
            k.setUp()
        k.destroy()


def test_natural_norm_with_fgmres_is_refused_at_setup(spk):
    k = spk.KSP()
    k.setFromOptions("-ksp_type fgmres -ksp_norm_type natural -pc_type jacobi")
    with pytest.raises(spk.SpkError, match="natural") as ei:
        k.setUp()
    assert ei.value.code == -6
    k.setFromOptions("-ksp_type minres")
    with pytest.raises(spk.SpkError, match="KSPSetOperators"):
        k.setUp()
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
    int (*fn)(spk_ctx *, const double *, double *, int, const spk_opts *, int, spk_result *, double *, int32_t) = spk_minres;
    spk_default_opts(&o);
    if (SPK_NORM_NATURAL != 1 || SPK_NORM_UNPRECONDITIONED != 0 || SPK_DIVERGED_INDEFINITE_PC != -8) return 2;
    if (fn(0, h, h, SPK_MEM_HOST, &o, SPK_NORM_NATURAL, &r, h, 4) != SPK_ERR_ARG) return 3;   /* null context */
    if (SpkKSPCreate(0, &k) != SPK_OK || SpkKSPGetType(k, &t, &nt) != SPK_OK) return 4;
    printf("%d %s\n", spk_version(), SpkKSPConvergedReasonName(SPK_DIVERGED_INDEFINITE_PC));
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
