"""The compressed Krylov basis (-spk_basis_precision single) without a GPU: the numpy model of the algorithm
(tests/_cb_fgmres.py: un-normalised FP32 storage, the norm from the rounded vector, early restart at theta = 2^-20,
confirmation on the true residual) held against a textbook FP64 FGMRES, and the public switches."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from _cb_fgmres import THETA, cb_fgmres_ref, fgmres_textbook

RTOL = 1e-8


def laplace5(n):
    """5-point Laplacian on an n x n grid of unknowns (Dirichlet boundary eliminated)."""
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(n, n))
    return (sp.kron(sp.identity(n), T) + sp.kron(T, sp.identity(n))).tocsr()


def jacobi_system(n=24, seed=3):
    A = laplace5(n)
    # a varying diagonal so that Jacobi is not a multiple of the identity
    s = 1.0 + 0.5 * np.random.default_rng(seed).random(A.shape[0])
    A = (sp.diags(s) @ A @ sp.diags(s)).tocsr()
    dinv = 1.0 / A.diagonal()
    b = np.random.default_rng(seed + 1).standard_normal(A.shape[0])
    return A, (lambda x: A @ x), (lambda x: dinv * x), b


def strong_system(n=16, seed=5):
    """M^-1 = A^-1 diag(1 +- 0.01): one cycle of FP64 FGMRES passes rtol; on an FP32 basis the recurrence stalls near
    1e-7 of the cycle's starting residual."""
    A = laplace5(n)
    Ainv = np.linalg.inv(A.toarray())
    pert = 1.0 + 0.01 * np.random.default_rng(seed).uniform(-1.0, 1.0, A.shape[0])
    b = np.random.default_rng(seed + 1).standard_normal(A.shape[0])
    return A, (lambda x: A @ x), (lambda x: Ainv @ (pert * x)), b


def smooth_rhs_system(A, rough=1e-7, seed=9):
    """b = K e for the smoothest eigenvector e of D^-1 K plus a small rough part: Jacobi FGMRES drops six decades inside
    one cycle, which an FP32 basis must answer with an early restart."""
    d = A.diagonal()
    _, e = spl.eigsh(A, k=1, M=sp.diags(d).tocsc(), sigma=0, which="LM")
    e = e[:, 0] / np.linalg.norm(e[:, 0])
    z = np.random.default_rng(seed).standard_normal(A.shape[0])
    return A @ (e + rough * z / np.linalg.norm(z))


@pytest.mark.parametrize("system", [jacobi_system, strong_system], ids=["jacobi", "strong"])
def test_model_keeps_up_with_textbook_fp64(system):
    A, K, M, b = system()
    x64, i64 = fgmres_textbook(K, M, b, restart=30, max_it=2000, rtol=RTOL)
    x32, i32 = cb_fgmres_ref(K, M, b, restart=30, max_it=2000, rtol=RTOL, basis="single")
    xd, idb = cb_fgmres_ref(K, M, b, restart=30, max_it=2000, rtol=RTOL, basis="double")
    print(f"{system.__name__}: its textbook {i64['its']}, model double {idb['its']}, model single {i32['its']} "
          f"in cycles {i32['cycle_its']}")
    assert i64["reason"] == 2 and i32["reason"] == 2 and idb["reason"] == 2
    # the un-normalised classical Gram-Schmidt form on an FP64 basis is the textbook method up to rounding
    assert abs(idb["its"] - i64["its"]) <= 1
    assert i32["its"] <= i64["its"] + 2
    true = np.linalg.norm(b - K(x32))
    assert true <= RTOL * np.linalg.norm(b)
    assert i32["rnorm"] == pytest.approx(true, rel=1e-6)   # what the solve reports is a true residual


def test_strong_preconditioner_needs_both_rules():
    """Without the early restart the recurrence stalls and the cycle runs out; with it the solve takes FP64's count."""
    A, K, M, b = strong_system()
    rtol = 1e-10   # below the 1e-8 .. 1e-9 of the cycle's starting residual at which the recurrence stalls
    x64, i64 = fgmres_textbook(K, M, b, rtol=rtol)
    xon, on = cb_fgmres_ref(K, M, b, rtol=rtol, basis="single")
    _, off = cb_fgmres_ref(K, M, b, rtol=rtol, basis="single", theta=0.0)
    print(f"strong: textbook {i64['its']}, theta = 2^-20 {on['its']} {on['cycle_its']}, theta = 0 {off['its']} {off['cycle_its']}")
    assert on["cycles"] >= 2 and on["cycle_its"][0] < 30        # the first cycle ended early
    assert off["its"] > on["its"] + 10 and off["cycle_its"][0] == 30
    assert on["history"][on["cycle_its"][0]] <= THETA * on["history"][0]
    assert on["its"] <= i64["its"] + 2 and np.linalg.norm(b - K(xon)) <= rtol * np.linalg.norm(b)


def test_model_restarts_early_on_a_smooth_right_hand_side():
    A, K, M, _ = jacobi_system(n=32)
    b = smooth_rhs_system(A)
    _, info = cb_fgmres_ref(K, M, b, rtol=1e-10, basis="single")
    print(f"smooth rhs: cycles {info['cycle_its']}, history head {info['history'][:6]}")
    first = info["cycle_its"][0]
    assert first < 30 and info["history"][first] <= THETA * info["history"][0]
    assert info["history"][first] > 1e-10 * info["history"][0]   # ended by rule 2, not by convergence
    assert info["reason"] == 2


def test_reversed_dot_products_move_the_history_a_little():
    A, K, M, b = jacobi_system()
    _, f = cb_fgmres_ref(K, M, b, max_it=45, rtol=1e-12, basis="single")
    _, r = cb_fgmres_ref(K, M, b, max_it=45, rtol=1e-12, basis="single", reverse=True)
    gap = np.max(np.abs(f["history"] - r["history"])) / f["rnorm0"]
    print(f"forward against reversed dot products: {gap:.2e} of rnorm0")
    assert f["its"] == r["its"] == 45 and f["reason"] == r["reason"] == -3
    assert gap < 1e-6      # the orders agree to far below FP32's round-off; 0 would mean reverse does nothing
    assert f["rnorm"] == pytest.approx(np.linalg.norm(b - K(cb_fgmres_ref(K, M, b, max_it=45, rtol=1e-12)[0])), rel=1e-9)


# --------------------------------------------------------------------------- the public switches
def test_default_opts_takes_the_basis(spk):
    assert spk.default_opts().basis_precision == 0
    assert spk.default_opts(basis="double").basis_precision == 0
    assert spk.default_opts(basis="single").basis_precision == 1
    assert spk.default_opts(basis_precision=1).basis_precision == 1
    with pytest.raises(ValueError):
        spk.default_opts(basis="half")
    import ctypes as C
    assert C.sizeof(type(spk.default_opts())) == 64   # the field took the reserved word's place: size and layout stay


def test_facade_takes_spk_basis_precision(spk):
    k = spk.KSP()
    assert k.getOptions()[0].basis_precision == 0
    k.setFromOptions("-ksp_type fgmres -spk_basis_precision single")
    assert k.getOptions()[0].basis_precision == 1
    k.setFromOptions("-spk_basis_precision double")
    assert k.getOptions()[0].basis_precision == 0
    for bad in ("-spk_basis_precision half", "-spk_basis_precision", "-spk_basis_precision 1"):
        with pytest.raises(spk.SpkError) as ei:
            k.setFromOptions(bad)
        assert ei.value.code == -1   # SPK_ERR_ARG
    assert k.getOptions()[0].basis_precision == 0
    k.destroy()
