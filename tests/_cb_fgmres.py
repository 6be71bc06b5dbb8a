"""Numpy models for the compressed-basis FGMRES (-spk_basis_precision single): `cb_fgmres_ref`, the algorithm the device
runs on an FP32 basis, and `fgmres_textbook`, a plain FP64 FGMRES to hold it against.  Shared by
tests/test_basis_fp32_cpu.py and tests/test_gpu_basis_fp32.py.

cb_fgmres_ref follows iteration form 5 step by step:
  * the basis is UN-NORMALISED: V~_{j+1} = w' = s_w w~ - sum_i (h_i sc_i) V~_i with the scale factor sc_{j+1} = 1 / ||V~_{j+1}||
    beside it, h_i = sc_i s_w (V~_i . w~), v_0 = r / ||r|| with sc_0 = 1;
  * with basis="single" a vector is STORED as float32(w') and its norm (so its scale factor) is taken from the rounded
    values; every product and sum is FP64;
  * z~_{j+1} = M^-1 w' and the next w~ = K z~_{j+1} come from the UNROUNDED w' (the method is flexible);
  * rule 1, tentative convergence: a convergence or max_it seen by the recurrence only ends the cycle, the true residual
    b - K x at the restart decides;
  * rule 2, early restart: a cycle also ends once the recurrence residual is <= THETA * beta, beta the residual the cycle
    started from.
basis="double" keeps the storage in FP64 and drops both rules (the recurrence ends the solve, as the FP64 device path).
reverse=True sums every dot product over the reversed vectors: the same numbers in another order, which is how far two
correct implementations of this algorithm may differ."""
import numpy as np

THETA = 2.0 ** -20   # kBasisTheta (spk_internal.hpp): FP32's unit round-off 2^-24 with 16x head-room
RTOL, ATOL, ITS = 2, 3, -3   # KSPConvergedReason


def _converged(rnorm, ttol, abstol, dtol, cnorm0):
    if not np.isfinite(rnorm):
        return -9
    if rnorm <= ttol:
        return ATOL if rnorm < abstol else RTOL
    if rnorm >= dtol * cnorm0:
        return -4
    return 0


def _dot(a, b, reverse):
    a = np.asarray(a, np.float64)
    if reverse:
        return float(np.dot(np.ascontiguousarray(a[::-1]), np.ascontiguousarray(b[::-1])))
    return float(np.dot(a, b))


def cb_fgmres_ref(K, M, b, restart=30, max_it=10000, rtol=1e-5, abstol=1e-50, dtol=1e4, basis="single", reverse=False,
                  theta=THETA):
    """K, M: callables x -> K x and x -> M^-1 x.  Returns (x, info) with info = dict(its, reason, rnorm, rnorm0, cycles,
    history, cycle_its): history[i] is the recurrence residual after iteration i (history[0] the initial residual),
    rnorm the norm the solve ended on (single: always a true residual), cycle_its the iterations of every cycle."""
    single = basis == "single"
    store = (lambda v: v.astype(np.float32)) if single else (lambda v: v.copy())
    b = np.asarray(b, np.float64)
    n = b.shape[0]
    x = np.zeros(n)
    r = b.copy()
    its, cycles, reason = 0, 0, 0
    hist, cycle_its = [], []
    rnorm0 = ttol = cnorm0 = rnorm = 0.0
    while True:
        beta = np.sqrt(_dot(r, r, reverse))
        rnorm = beta
        if its == 0 and not hist:
            rnorm0 = cnorm0 = beta
            ttol = max(rtol * beta, abstol)
            hist.append(beta)
        reason = _converged(beta, ttol, abstol, dtol, cnorm0)
        if not reason and its >= max_it:
            reason = ITS
        if reason:
            break
        v0 = r / beta
        V = [store(v0)]
        sc = [1.0]
        Z = [M(v0)]
        wt = K(Z[0])
        H = np.zeros((restart + 2, restart + 1))
        cs, sn, rs = np.zeros(restart + 1), np.zeros(restart + 1), np.zeros(restart + 2)
        rs[0] = beta
        done_loc, stop = 0, False
        for loc in range(restart):
            nv = loc + 1
            s_w = sc[loc]
            h = np.array([sc[i] * s_w * _dot(V[i], wt, reverse) for i in range(nv)])
            wp = s_w * wt
            for i in range(nv):
                wp -= (h[i] * sc[i]) * V[i].astype(np.float64)
            vs = store(wp)
            tt = np.sqrt(_dot(vs, vs.astype(np.float64), reverse))
            # Givens step (KSPFGMRESUpdateHessenberg)
            col = np.append(h, tt)
            for j in range(loc):
                t = cs[j] * col[j] + sn[j] * col[j + 1]
                col[j + 1] = cs[j] * col[j + 1] - sn[j] * col[j]
                col[j] = t
            d = np.hypot(col[loc], tt)
            cs[loc], sn[loc] = col[loc] / d, tt / d
            rs[loc + 1] = -sn[loc] * rs[loc]
            rs[loc] = cs[loc] * rs[loc]
            col[loc] = d
            H[:loc + 1, loc] = col[:loc + 1]
            its += 1
            done_loc = loc + 1
            rec = abs(rs[loc + 1])
            hist.append(rec)
            rr = _converged(rec, ttol, abstol, dtol, cnorm0)
            if not rr and its >= max_it:
                rr = ITS
            if rr:
                if single and (rr > 0 or rr == ITS):
                    stop = True          # rule 1: the restart's true residual decides
                else:
                    reason, rnorm, stop = rr, rec, True
            elif single and rec <= theta * beta:
                stop = True              # rule 2
            if stop:
                break
            V.append(vs)
            sc.append(1.0 / tt if tt > 1e-300 else 1.0)
            Z.append(M(wp))
            wt = K(Z[-1])
        y = np.linalg.solve(np.triu(H[:done_loc, :done_loc]), rs[:done_loc]) if done_loc else np.zeros(0)
        for k in range(done_loc):
            x += (y[k] * sc[k]) * Z[k]
        cycles += 1
        cycle_its.append(done_loc)
        if reason:
            break
        r = b - K(x)
    return x, dict(its=its, reason=reason, rnorm=rnorm, rnorm0=rnorm0, cycles=cycles, history=np.array(hist),
                   cycle_its=cycle_its)


def fgmres_textbook(K, M, b, restart=30, max_it=10000, rtol=1e-5, reverse=False):
    """Right-preconditioned flexible GMRES with modified Gram-Schmidt on a normalised FP64 basis (Saad, Alg. 9.6), the
    convergence test on the recurrence residual against rtol ||b|| (zero initial guess).  reverse=True sums every dot
    product and norm over the reversed vectors, as in cb_fgmres_ref."""
    nrm = lambda v: np.sqrt(_dot(v, v, reverse))
    b = np.asarray(b, np.float64)
    x = np.zeros_like(b)
    its = 0
    ttol = rtol * nrm(b)
    hist = [nrm(b)]
    while True:
        r = b - K(x)
        beta = nrm(r)
        if beta <= ttol or its >= max_it:
            return x, dict(its=its, reason=RTOL if beta <= ttol else ITS, rnorm=beta, history=np.array(hist))
        V, Z = [r / beta], []
        H = np.zeros((restart + 1, restart))
        e1 = np.zeros(restart + 1)
        e1[0] = beta
        k = 0
        for j in range(restart):
            Z.append(M(V[j]))
            w = K(Z[j])
            for i in range(j + 1):
                H[i, j] = _dot(V[i], w, reverse)
                w -= H[i, j] * V[i]
            H[j + 1, j] = nrm(w)
            its += 1
            k = j + 1
            y, *_ = np.linalg.lstsq(H[:k + 1, :k], e1[:k + 1], rcond=None)
            rec = np.linalg.norm(e1[:k + 1] - H[:k + 1, :k] @ y)
            hist.append(rec)
            if rec <= ttol or its >= max_it or H[j + 1, j] == 0.0:
                break
            V.append(w / H[j + 1, j])
        for i in range(k):
            x += y[i] * Z[i]
        if its >= max_it:
            r = b - K(x)
            return x, dict(its=its, reason=ITS, rnorm=nrm(r), history=np.array(hist))
