"""Cases, inputs and references of the Gram-Schmidt kernel tests (test_gpu_vec_kernels.py, test_vec_reference_cpu.py), and
the child process that runs a list of them under one of the SPK_VEC_* knobs:

    python _vec_worker.py CASE_FILE OUT_FILE        (a fresh process: the knobs are read once per process)

Nothing in the upper part of this file touches the GPU: the restatement of the launch shapes (spk_device.hpp ws_shape /
vec_shape / vec_grid and the dispatch of k::mdot / k::maxpy), the depth function of the rounding tier, the input builders
and the integer references import and run anywhere.

Exact tier.  Every input is a small integer (vectors, w, coefficients in -3..3, B D planes in -2..2), so every product and
every partial sum in any order is an exact double (|sum| <= 9 * 1.3 M < 2^24, ||w'||^2 <= 570^2 * 1.3 M < 2^40) and the
kernel must return the int64 result bit for bit.  PADV, a distinct integer, sits in the padding [n, ld) of every device
vector and in entries [n_dot, n) (MAXPY planes: [n_bd, n)): a lane that reads past n or sums past its mask shows.

Rounding tier ("gauss": 1).  Gaussian data with heavy cancellation against an np.longdouble reference:
|got - ref| <= d * 2^-53 * S, S = sum |terms|, d from depth() below (the launch shape, never an observed error).
"""
import hashlib
import json
import math
import os
import sys

import numpy as np

PADV = 1000003.0
MARKER = -7777777.0          # SPK_DEBUG_MARKER (include/spk.h)
K_VEC_MAX_BLOCKS = 256       # spk_device.hpp kVecMaxBlocks
SCHUR_LOWER, SCHUR_FULL = 1, 3


# --------------------------------------------------------------------------- launch shapes, restated
def _knob(env, name, default):
    v = (os.environ if env is None else env).get(name)
    return default if v is None else int(v)


def ws_shape(n2, env=None):
    """spk_device.hpp ws_shape -> (on, U, grid)."""
    knob = _knob(env, "SPK_VEC_WS", -1)
    on = n2 < K_VEC_MAX_BLOCKS * 2048 and knob != 0
    U = 8 if n2 >= K_VEC_MAX_BLOCKS * 64 * 8 else (4 if n2 >= K_VEC_MAX_BLOCKS * 64 * 4 else 2)
    if knob in (2, 4, 8):
        U = knob
    tiles = max((n2 + 64 * U - 1) // (64 * U), 1)
    return int(on), U, min(tiles, K_VEC_MAX_BLOCKS)


def vec_shape(n2, maxpy=False):
    """spk_device.hpp vec_shape -> (T, U, G, grid)."""
    G, cap = 4, K_VEC_MAX_BLOCKS
    if n2 >= K_VEC_MAX_BLOCKS * 2048:
        T, U = 512, 4
    elif n2 >= K_VEC_MAX_BLOCKS * 1024:
        T, U = 256, 4
    elif n2 >= K_VEC_MAX_BLOCKS * 512:
        T, U = 256, 2
    else:
        T, U = 256, 1
    if maxpy and n2 < K_VEC_MAX_BLOCKS * 1024:
        T, U, G, cap = 256, 1, 8, 1024
    elif maxpy and n2 < K_VEC_MAX_BLOCKS * 2048:
        T, U, G, cap = 256, 2, 8, 1024
    tiles = max((n2 + T * U - 1) // (T * U), 1)
    return T, U, G, min(tiles, cap)


def vec_grid(n2, T=1024):
    tiles = max((n2 + T - 1) // T, 1)
    return min(tiles, K_VEC_MAX_BLOCKS if T >= 512 else 2 * K_VEC_MAX_BLOCKS)


def shapes(n, env=None):
    """What Context.debug_vec_shape(n) returns, from the restatement."""
    n2 = (n + 1) // 2
    return dict(ws=ws_shape(n2, env), mdot=vec_shape(n2), maxpy=vec_shape(n2, True), ws16=_knob(env, "SPK_VEC_WS16", 1),
                deep=_knob(env, "SPK_VEC_DEEP", 0))


def mdot_forms(n, ntot, env=None):
    """The launches of k::mdot for ntot vectors of n entries: one dict per chunk of <= 40 vectors (name: the template
    instantiation, k: reduced values of the launch, T / U / grid / tile / W: what depth() needs)."""
    n2 = (n + 1) // 2
    on, wu, wgrid = ws_shape(n2, env)
    T, U, G, grid = vec_shape(n2)
    ws16 = _knob(env, "SPK_VEC_WS16", 1)
    out, v0 = [], 0
    while True:
        cnt = min(ntot - v0, 40)
        k = cnt + (1 if v0 + 40 >= ntot else 0)
        if on and ws16:
            per = (cnt + 15) // 16
            vw, u = (1, wu) if per <= 1 else ((2, wu) if per <= 2 else (3, 4 if wu == 8 else wu))
            out.append(dict(name=f"mdot_ws16_kernel<{vw},{u}>", k=k, T=1024, U=u, grid=wgrid, tile=64 * u, W=0))
        elif on:
            per = (cnt + 3) // 4
            vw = 4 if per <= 4 else (8 if per <= 8 else 12)
            g = 2 if wu == 8 else 4
            out.append(dict(name=f"mdot_ws_kernel<{vw},{wu},{g}>", k=k, T=256, U=wu, grid=wgrid, tile=64 * wu, W=0))
        else:
            ng = min(max((cnt + 7) // 8, 1), 5)
            out.append(dict(name=f"mdot_kernel<{ng},{T},{G},{U}>", k=k, T=T, U=U, grid=grid, tile=T * U, W=T // 64))
        v0 += 40
        if v0 >= ntot:
            return out


def maxpy_form(n, nv, mp, env=None):
    """The launch of k::maxpy (nv: the host count the dispatch sees; mp: 0, 4 or 8)."""
    n2 = (n + 1) // 2
    T, U, G, grid = vec_shape(n2, True)
    deep = _knob(env, "SPK_VEC_DEEP", 0)
    if T == 256 and deep:
        if U == 2 and nv > 8:
            G = 16
        elif U == 1 and nv > 16:
            G = 32
        elif U == 1 and nv > 8:
            G = 16
    return dict(name=f"maxpy_kernel<{T},{G},{mp},{U}>", T=T, U=U, grid=grid, tile=T * U, W=T // 64)


def maxpy_mp(case):
    return (4 if case["m"] <= 4 else 8) if (case.get("bd") or case.get("pyth")) and case["m"] > 0 else 0


def case_forms(case, env=None):
    """Names of the template instantiations a case launches."""
    k = case["k"]
    if k == "mdot":
        return [f["name"] for f in mdot_forms(case["n"], case["nv"] + case.get("nv2", 0), env)]
    if k == "maxpy":
        return [maxpy_form(case["n"], case["nv"], maxpy_mp(case), env)["name"]]
    if k == "norm":
        return [f"sqnorm_bd_kernel<{4 if case['m'] <= 4 else 8}>"]
    if k == "pack":
        return ["pack_bd_kernel"]
    if k == "head":
        return [f"fused_head_kernel<{4 if case['m'] <= 4 else 8}>"]
    raise ValueError(k)


# --------------------------------------------------------------------------- rounding tier: additions on the longest path
def final_reduce_depth(nb, k, T):
    """final_reduce (spk_device.hpp): thread (slice sl, value i) adds the partials of blocks sl, sl + nsl, ... to 0.0 --
    ceil(nb / nsl) additions, nsl = T / kk slices, kk = k rounded up to a power of two -- then a binary tree over the nsl
    slices: log2(nsl) additions."""
    kk = 1
    while kk < k:
        kk <<= 1
    nsl = T // kk
    return -(-nb // nsl) + int(math.log2(nsl))


def depth(form, n, k=None, per_tile=None):
    """Additions (and the one rounding of the product itself) between a product and the output of a reducing launch:
       1                      the product (it may be fused into the first addition: then this term is slack)
       tiles * per_tile       the thread's chain: tiles = tiles per workgroup = ceil(ceil(n2 / tile) / grid); per tile
                              VecMDot adds its 2 U products to a tile sum and the tile sum to the accumulator (2 U + 1),
                              MAXPY's norm and plane sums add their 2 U products to the accumulator directly (2 U)
       6                      the wave's shuffle tree (32, 16, 8, 4, 2, 1)
       W                      the waves of the workgroup, summed serially from 0.0 (W = T / 64; the wave-split forms
                              publish per wave: W = 0)
       final_reduce_depth     the reducer's slice and tree
    """
    n2 = (n + 1) // 2
    tiles = -(-(-(-n2 // form["tile"])) // form["grid"])
    tiles = max(tiles, 1)
    if per_tile is None:
        per_tile = 2 * form["U"] + 1
    return 1 + tiles * per_tile + 6 + form["W"] + final_reduce_depth(form["grid"], form["k"] if k is None else k, form["T"])


def norm_form(n, m):
    """k::sqnorm_bd: 512 threads, one double2 per thread and pass (U = 1), grid = vec_grid(n2, 512)."""
    n2 = (n + 1) // 2
    return dict(name=f"sqnorm_bd_kernel<{4 if m <= 4 else 8}>", T=512, U=1, grid=vec_grid(n2, 512), tile=512, W=8, k=1 + m)


# --------------------------------------------------------------------------- inputs
def _ints(rng, shape, lim):
    return rng.integers(-lim, lim + 1, shape, dtype=np.int8).astype(np.float64)


def _parity_rows(rng, m, n):
    """m dense rows in -2..2 with the structure pack_bd needs: row 2q lives on even entries, row 2q + 1 on odd ones
    (a last unpaired row is dense)."""
    bd = _ints(rng, (m, n), 2)
    for r in range(m - (m & 1)):
        bd[r, (1 - (r & 1))::2] = 0.0
    return bd


def pack_rows(bd):
    """numpy interleave: plane q = row 2q on even entries, row 2q + 1 on odd ones."""
    m, n = bd.shape
    p = np.zeros((m // 2, n))
    for q in range(m // 2):
        p[q, 0::2] = bd[2 * q, 0::2]
        p[q, 1::2] = bd[2 * q + 1, 1::2]
    return p


def _cancelling(rng, n):
    """+-1e6 alternating + N(0, 1): sums against smooth vectors cancel to |result| << S."""
    return np.where(np.arange(n) & 1, -1.0, 1.0) * 1e6 + rng.standard_normal(n)


def mdot_inputs(case):
    n, nv, nv2, split, n_dot = case["n"], case["nv"], case.get("nv2", 0), case.get("split", 0), case.get("n_dot", case["n"])
    rng = np.random.default_rng(case["seed"])
    rows2 = nv2 // 2 if split else nv2
    if case.get("gauss"):
        V = 1.0 + 1e-3 * rng.standard_normal((nv, n))
        V2 = 1.0 + 1e-3 * rng.standard_normal((rows2, n))
        w = _cancelling(rng, n)
    else:
        V, V2, w = _ints(rng, (nv, n), 3), _ints(rng, (rows2, n), 2), _ints(rng, (n,), 3)
        V[:, n_dot:] = PADV
        V2[:, n_dot:] = PADV
        w[n_dot:] = PADV
    return dict(V=V, V2=V2 if nv2 else None, w=w)


def maxpy_inputs(case):
    n, nv, m = case["n"], case["nv"], case.get("m", 0)
    n_dot, n_bd = case.get("n_dot", n), case.get("n_bd", 0)
    rng = np.random.default_rng(case["seed"])
    bd = planes = None
    if case.get("gauss"):
        V = 1.0 + 1e-3 * rng.standard_normal((nv, n))
        a = rng.standard_normal(nv)
        w = rng.standard_normal(n)
        if nv:  # w' = w - V a cancels to the size of the noise
            w += (a.sum() * (1.0 if case.get("sign", 1.0) < 0 else -1.0))
        if case.get("bd"):
            bd = _parity_rows(rng, m, n) * _cancelling(rng, n)
    else:
        V, a, w = _ints(rng, (nv, n), 3), _ints(rng, (nv,), 3), _ints(rng, (n,), 3)
        V[:, n_dot:] = PADV
        w[n_dot:] = PADV
        if case.get("bd"):
            bd = _parity_rows(rng, m, n) if case["bd"] == "packed" else _ints(rng, (m, n), 2)
            bd[:, n_bd:] = PADV
    if bd is not None:
        planes = pack_rows(bd) if case["bd"] == "packed" else bd
        if case["bd"] == "packed":
            planes[:, n_bd:] = PADV
    pyth = None
    if case.get("pyth"):
        live = case.get("nv_live", -1)
        live = nv if live < 0 else live
        h = _ints(rng, (live,), 3)
        q = _ints(rng, (m,), 3) * 5.0
        hh = float(h @ h)
        # ww - sum h^2 is a power of 4 ("pow4") or <= 0 ("floor": the kernel keeps 1.5e-14 ww)
        ww = hh + 4.0 ** case["pyth_k"] if case["pyth"] == "pow4" else max(hh - 1.0, 1.0 if hh == 0 else hh * 0.5)
        tb = np.zeros((nv + 1, 8))
        tb[:nv, :] = _ints(rng, (nv, 8), 3)
        tb[nv, :] = PADV      # the row the kernel writes when nv_live = nv; any other row must stay
        pyth = dict(dots=np.concatenate([h, q, [ww]]), tb=tb)
    return dict(V=V, a=a, w=w, bd=bd, planes=planes, pyth=pyth)


def norm_inputs(case):
    n, m, n_bd, n_dot = case["n"], case["m"], case["n_bd"], case["n_dot"]
    rng = np.random.default_rng(case["seed"])
    if case.get("gauss"):
        x = rng.standard_normal(n)
        bd = (1.0 + 1e-3 * rng.standard_normal((m, n))) * _cancelling(rng, n)
        sb = rng.standard_normal(n) * 1e3
    else:
        x, bd, sb = _ints(rng, (n,), 3), _ints(rng, (m, n), 2), _ints(rng, (n,), 3)
        x[n_bd:n_bd + m] = PADV + 1.0 + np.arange(m)     # the multiplier entries: distinct, so their order shows
        x[n_bd + m:] = PADV
        bd[:, n_bd:] = PADV
    return dict(x=x, bd=bd, sa=x + sb, sb=sb)


def pack_inputs(case):
    rng = np.random.default_rng(case["seed"])
    n, m = case["n"], case["m"]
    bd = _parity_rows(rng, m, n)
    bad = case.get("bad")
    if bad is not None:   # one entry on the wrong parity of an "even" (bad = 0) or "odd" (bad = 1) row
        r = 2 * (case["seed"] % (m // 2)) + bad
        i = (n // 3) | 1 if bad == 0 else ((n // 3) & ~1)
        bd[r, i] = 2.0
    return dict(bd=bd)


def head_inputs(case):
    nl, m, packed = case["nl"], case["m"], case.get("packed", 0)
    rng = np.random.default_rng(case["seed"])
    if case.get("gauss"):
        g = rng.standard_normal
        return dict(v=g(nl + m), nrm=np.concatenate([[abs(g()) + 0.5], g(m)]), w1raw=g(m), dinv=np.abs(g(nl)) + 0.5,
                    bd=_parity_rows(rng, m, nl) * np.abs(g(nl)) if packed else g((m, nl)), shat=np.abs(g(m)) + 0.5,
                    gram=g((m, m)))
    kk = case["seed"] % 5 - 2
    nrm = np.concatenate([[4.0 ** kk], _ints(rng, (m,), 3)])
    dinv = 2.0 ** rng.integers(-2, 3, nl)
    shat = 2.0 ** rng.integers(-2, 3, m) * rng.choice([-1.0, 1.0], m)
    bd = _parity_rows(rng, m, nl) if packed else _ints(rng, (m, nl), 2)
    return dict(v=_ints(rng, (nl + m,), 3), nrm=nrm, w1raw=_ints(rng, (m,), 3), dinv=dinv, bd=bd, shat=shat,
                gram=_ints(rng, (m, m), 2))


# --------------------------------------------------------------------------- references (exact tier: int64)
def _i64(a):
    r = np.asarray(a).astype(np.int64)
    assert np.array_equal(r, a), "the exact tier needs integer inputs"
    return r


def mdot_reference(case, inp):
    nv, nv2, split, n_dot = case["nv"], case.get("nv2", 0), case.get("split", 0), case.get("n_dot", case["n"])
    out = np.full(nv + nv2 + 1, MARKER)
    if case.get("done", -1) == 1:
        return dict(out=out)
    w = _i64(inp["w"][:n_dot])
    for i in range(nv):
        out[i] = np.dot(_i64(inp["V"][i, :n_dot]), w)
    for j in range(nv2):
        if split:   # result nv + j is half j & 1 of plane j / 2
            out[nv + j] = np.dot(_i64(inp["V2"][j >> 1, (j & 1):n_dot:2]), w[(j & 1)::2])
        else:
            out[nv + j] = np.dot(_i64(inp["V2"][j, :n_dot]), w)
    out[nv + nv2] = np.dot(w, w)
    return dict(out=out)


def pyth_reference(case, inp, live):
    """The single-reduction rider (first wave of workgroup 0): -> nrm_out (1 + m), tb."""
    m = case["m"]
    dots, tb = inp["pyth"]["dots"], inp["pyth"]["tb"].copy()
    h = dots[:live]
    ww = dots[live + m]
    tt2 = ww - float(h @ h)
    if not tt2 > 1.5e-14 * ww:
        tt2 = 1.5e-14 * ww
    inv = 1.0 / np.sqrt(tt2) if tt2 > 0.0 else 0.0
    nrm_out = np.full(1 + m, MARKER)
    nrm_out[0] = tt2
    for r in range(m):
        t = dots[live + r] - float(h @ tb[:live, r])
        nrm_out[1 + r] = t
        tb[live, r] = t * inv
    return nrm_out, tb


def maxpy_reference(case, inp):
    n, nv, m = case["n"], case["nv"], case.get("m", 0)
    n_dot, n_bd = case.get("n_dot", n), case.get("n_bd", 0)
    live = case.get("nv_live", -1)
    live = nv if live < 0 else live
    mp = maxpy_mp(case)
    red, side = np.full(1 + m, MARKER), np.full(m, MARKER)
    ref = dict(w=inp["w"].copy(), red=red, w1side=side)
    if case.get("pyth"):
        ref["nrm_out"], ref["tb"] = np.full(1 + m, MARKER), inp["pyth"]["tb"].copy()
    if case.get("done", -1) == 1:
        return ref
    if case.get("pyth"):
        ref["nrm_out"], ref["tb"] = pyth_reference(case, inp, live)
    w = _i64(inp["w"])
    sg = int(case.get("sign", 1.0))
    for i in range(live):
        w = w + sg * int(inp["a"][i]) * _i64(inp["V"][i])
    ref["w"] = w.astype(np.float64)
    if case.get("w1side") and mp:
        side[:] = w[n_bd:n_bd + m]
    if case.get("want_norm", 1):
        red[0] = np.dot(w[:n_dot], w[:n_dot])
        for r in range(m if mp else 0):   # rows of B D: entries below n_bd only (no planes: the slots hold zero)
            red[1 + r] = np.dot(_i64(inp["bd"][r, :n_bd]), w[:n_bd]) if inp["bd"] is not None else 0.0
    return ref


def norm_reference(case, inp):
    m, n_bd, n_dot = case["m"], case["n_bd"], case["n_dot"]
    x = _i64(inp["sa"]) - _i64(inp["sb"]) if case.get("sub") else _i64(inp["x"])
    red = np.zeros(1 + m)
    red[0] = np.dot(x[:n_dot], x[:n_dot])
    for r in range(m):
        red[1 + r] = np.dot(_i64(inp["bd"][r, :n_bd]), x[:n_bd])
    return dict(x=x.astype(np.float64), red=red, w1side=x[n_bd:n_bd + m].astype(np.float64))


def pack_reference(case, inp):
    return dict(planes=pack_rows(inp["bd"]), bad=np.array([0.0 if case.get("bad") is None else 1.0]))


def head_reference(case, inp):
    """The formulas of fused_head_kernel's header comment, in double: exact on the exact tier's inputs (powers of two and
    small integers), and the thing to compare with in extended precision on the rounding tier (dtype)."""
    nl, m = case["nl"], case["m"]
    full = case.get("fact", SCHUR_FULL) == SCHUR_FULL
    dt = np.longdouble if case.get("gauss") else np.float64
    g = {k: np.asarray(v, dt) for k, v in inp.items()}
    inv = 1.0 / np.sqrt(g["nrm"][0])
    x1 = g["w1raw"] * inv
    t = g["nrm"][1:] * inv
    y = -(x1 - t) / g["shat"]
    wv = g["v"][:nl] * inv
    s = np.zeros(nl, dt)
    sabs = np.zeros(nl, dt)
    for r in range(m):
        s += g["bd"][r] * y[r]
        sabs += np.abs(g["bd"][r]) * (np.abs(x1[r]) + np.abs(t[r])) / np.abs(g["shat"][r])
    z0 = wv * g["dinv"] - (s if full else 0.0)
    w1 = t - (g["gram"] @ y if full and m else 0.0)
    ref = dict(v=np.concatenate([wv, x1]), z=np.concatenate([z0, y]))
    if not case.get("jacobi"):
        ref["c"] = np.concatenate([s / g["dinv"], w1])
    if case.get("want_wl"):
        ref["wl"] = w1
    if case.get("gauss"):   # S per component: the sum of the absolute values of the terms that form it
        ya = (np.abs(x1) + np.abs(t)) / np.abs(g["shat"])
        w1a = np.abs(t) + (np.abs(g["gram"]) @ ya if full and m else 0.0)
        ref["S"] = dict(v=np.abs(ref["v"]), z=np.concatenate([np.abs(wv * g["dinv"]) + (sabs if full else 0.0), ya]),
                        c=np.concatenate([sabs / g["dinv"], w1a]), wl=w1a)
    return ref


# --------------------------------------------------------------------------- brute force (the CPU test's second opinion)
def brute_mdot(case, inp):
    """Definition of k::mdot as plain Python loops over the arrays the kernel gets."""
    nv, nv2, split, n_dot = case["nv"], case.get("nv2", 0), case.get("split", 0), case.get("n_dot", case["n"])
    out = [MARKER] * (nv + nv2 + 1)
    if case.get("done", -1) == 1:
        return dict(out=np.array(out))
    w = [int(x) for x in inp["w"]]
    for i in range(nv):
        out[i] = sum(int(inp["V"][i, e]) * w[e] for e in range(n_dot))
    for j in range(nv2):
        if split:
            out[nv + j] = sum(int(inp["V2"][j // 2, e]) * w[e] for e in range(n_dot) if e % 2 == j % 2)
        else:
            out[nv + j] = sum(int(inp["V2"][j, e]) * w[e] for e in range(n_dot))
    out[nv + nv2] = sum(w[e] * w[e] for e in range(n_dot))
    return dict(out=np.array(out, np.float64))


def brute_maxpy(case, inp):
    n, nv, m = case["n"], case["nv"], case.get("m", 0)
    n_dot, n_bd = case.get("n_dot", n), case.get("n_bd", 0)
    live = nv if case.get("nv_live", -1) < 0 else case["nv_live"]
    mp = maxpy_mp(case)
    w = [int(x) for x in inp["w"]]
    red, side = [MARKER] * (1 + m), [MARKER] * m
    out = dict()
    if case.get("pyth"):
        out["nrm_out"], out["tb"] = np.full(1 + m, MARKER), inp["pyth"]["tb"].copy()
    if case.get("done", -1) != 1:
        for e in range(n):
            w[e] += int(case.get("sign", 1.0)) * sum(int(inp["a"][i]) * int(inp["V"][i, e]) for i in range(live))
        if case.get("w1side") and mp:
            side = [w[n_bd + r] for r in range(m)]
        if case.get("want_norm", 1):
            red[0] = sum(w[e] * w[e] for e in range(n_dot))
            for r in range(m if mp else 0):
                red[1 + r] = 0
                if case.get("bd") == "packed":   # .x of plane r / 2 feeds row 2q, .y row 2q + 1
                    red[1 + r] = sum(int(inp["planes"][r // 2, e]) * w[e] for e in range(n_bd) if e % 2 == r % 2)
                elif case.get("bd"):
                    red[1 + r] = sum(int(inp["planes"][r, e]) * w[e] for e in range(n_bd))
        if case.get("pyth"):
            dots, tb = [float(x) for x in inp["pyth"]["dots"]], out["tb"]
            hh = sum(dots[i] * dots[i] for i in range(live))
            ww = dots[live + m]
            tt2 = ww - hh if ww - hh > 1.5e-14 * ww else 1.5e-14 * ww
            out["nrm_out"][0] = tt2
            for r in range(m):
                t = dots[live + r] - sum(dots[i] * tb[i, r] for i in range(live))
                out["nrm_out"][1 + r] = t
                tb[live, r] = t * (1.0 / math.sqrt(tt2))
    out.update(w=np.array(w, np.float64), red=np.array(red, np.float64), w1side=np.array(side, np.float64))
    return out


def brute_norm(case, inp):
    n, m, n_bd, n_dot = case["n"], case["m"], case["n_bd"], case["n_dot"]
    x = [int(inp["sa"][e]) - int(inp["sb"][e]) if case.get("sub") else int(inp["x"][e]) for e in range(n)]
    red = [sum(x[e] * x[e] for e in range(n_dot))]
    red += [sum(int(inp["bd"][r, e]) * x[e] for e in range(n_bd)) for r in range(m)]
    return dict(x=np.array(x, np.float64), red=np.array(red, np.float64),
                w1side=np.array([x[n_bd + r] for r in range(m)], np.float64))


def brute_pack(case, inp):
    bd = inp["bd"]
    m, n = bd.shape
    planes = np.array([[bd[2 * q + (e & 1), e] for e in range(n)] for q in range(m // 2)]).reshape(m // 2, n)
    bad = any(bd[2 * q + 1 - (e & 1), e] != 0 for q in range(m // 2) for e in range(n))
    return dict(planes=planes, bad=np.array([float(bad)]))


def brute_head(case, inp):
    from fractions import Fraction as F
    nl, m = case["nl"], case["m"]
    full = case.get("fact", SCHUR_FULL) == SCHUR_FULL
    f = {k: [F(float(x)) for x in np.asarray(v).reshape(-1)] for k, v in inp.items()}
    tt = F(math.sqrt(float(inp["nrm"][0])))
    assert tt * tt == f["nrm"][0]
    x1 = [f["w1raw"][r] / tt for r in range(m)]
    t = [f["nrm"][1 + r] / tt for r in range(m)]
    y = [-(x1[r] - t[r]) / f["shat"][r] for r in range(m)]
    bd = np.asarray(inp["bd"]).reshape(m, nl) if m else None
    v, z, c = [], [], []
    for e in range(nl):
        s = sum((F(float(bd[r, e])) * y[r] for r in range(m)), F(0))
        wv = f["v"][e] / tt
        v.append(wv)
        z.append(wv * f["dinv"][e] - (s if full else 0))
        c.append(s / f["dinv"][e])
    w1 = [t[r] - (sum((f["gram"][r * m + q] * y[q] for q in range(m)), F(0)) if full else 0) for r in range(m)]
    out = dict(v=np.array([float(x) for x in v + x1]), z=np.array([float(x) for x in z + y]))
    if not case.get("jacobi"):
        out["c"] = np.array([float(x) for x in c + w1])
    if case.get("want_wl"):
        out["wl"] = np.array([float(x) for x in w1])
    return out


INPUTS = dict(mdot=mdot_inputs, maxpy=maxpy_inputs, norm=norm_inputs, pack=pack_inputs, head=head_inputs)
REFERENCE = dict(mdot=mdot_reference, maxpy=maxpy_reference, norm=norm_reference, pack=pack_reference, head=head_reference)
BRUTE = dict(mdot=brute_mdot, maxpy=brute_maxpy, norm=brute_norm, pack=brute_pack, head=brute_head)


# --------------------------------------------------------------------------- running a case on the GPU
def launch(c, case, inp):
    """Runs the case's kernel through its debug hook; -> dict of output arrays (the keys of the reference)."""
    k = case["k"]
    if k == "mdot":
        return dict(out=c.debug_mdot(inp["V"], inp["w"], n_dot=case.get("n_dot"), V2=inp["V2"], split=case.get("split", 0),
                                     done=case.get("done", -1), pad=PADV))
    if k == "maxpy":
        r = c.debug_maxpy(inp["V"], inp["a"], inp["w"], sign=case.get("sign", 1.0), n_dot=case.get("n_dot"),
                          nv_live=case.get("nv_live", -1), want_norm=case.get("want_norm", 1), bd=inp["planes"],
                          packed=int(case.get("bd") == "packed"), n_bd=case.get("n_bd", 0), m=case.get("m", 0),
                          w1side=case.get("w1side", 0), pyth=inp["pyth"], done=case.get("done", -1), pad=PADV)
        out = dict(w=r["w"], red=r["red"], w1side=r["w1side"])
        if case.get("pyth"):
            out.update(nrm_out=r["nrm_out"], tb=r["tb"])
        return out
    if k == "norm":
        return c.debug_cycle_norm(inp["x"], inp["bd"], case["n_bd"], n_dot=case["n_dot"],
                                  sub=(inp["sa"], inp["sb"]) if case.get("sub") else None, pad=PADV)
    if k == "pack":
        planes, bad = c.debug_pack_bd(inp["bd"])
        return dict(planes=planes, bad=np.array([float(bad)]))
    if k == "head":
        r = c.debug_cycle_head(inp["v"], inp["nrm"], inp["dinv"], w1raw=inp["w1raw"],
                               bd=pack_rows(inp["bd"]) if case.get("packed") else inp["bd"], shat=inp["shat"], gram=inp["gram"],
                               fact=case.get("fact", SCHUR_FULL), packed=case.get("packed", 0), jacobi=case.get("jacobi", 0),
                               want_wl=case.get("want_wl", 0), pad=PADV)
        return {k2: v for k2, v in r.items() if v is not None}
    raise ValueError(k)


def first_mismatch(got, exp):
    """None when every output equals its reference exactly, else a line naming the first difference."""
    for name in sorted(exp):
        g, e = np.asarray(got[name], np.float64).reshape(-1), np.asarray(exp[name], np.float64).reshape(-1)
        if g.shape != e.shape:
            return f"{name}: shape {g.shape} against {e.shape}"
        bad = np.flatnonzero(~(g == e))
        if bad.size:
            i = int(bad[0])
            return f"{name}[{i}]: got {g[i]!r}, expected {e[i]!r} ({bad.size} of {g.size} differ, last at {int(bad[-1])})"
    return None


def digest(d):
    h = hashlib.sha256()
    for name in sorted(d):
        h.update(name.encode())
        h.update(np.ascontiguousarray(d[name], np.float64).tobytes())
    return h.hexdigest()[:16]


def _ld(a):
    return np.asarray(a, np.longdouble)


def _sum_ld(terms):
    """(sum, sum of absolute values) of longdouble terms."""
    return terms.sum(), np.abs(terms).sum()


def gauss_ratio(case, inp, got):
    """Rounding tier: -> ([(|got - ref| / (2^-53 S), its bound d) per reduced output], (largest componentwise ratio of the
    vector outputs, its bound)) -- the vector pair is None where the kernel writes no vector."""
    assert np.finfo(np.longdouble).nmant + 1 >= 64, "np.longdouble carries fewer than 64 significand bits here"
    u = np.longdouble(2.0) ** -53
    k, n = case["k"], case.get("n")
    red, vec = [], None
    if k == "mdot":
        nv, nv2, split = case["nv"], case.get("nv2", 0), case.get("split", 0)
        w = _ld(inp["w"])
        rows = [inp["V"][i] for i in range(nv)]
        rows += [np.where((np.arange(n) & 1) == (j & 1), inp["V2"][j >> 1], 0.0) if split else inp["V2"][j] for j in range(nv2)]
        rows.append(inp["w"])
        forms = mdot_forms(n, nv + nv2)
        for i, row in enumerate(rows):
            ref, S = _sum_ld(_ld(row) * w)
            f = forms[min(i // 40, len(forms) - 1)]
            red.append((abs(_ld(got["out"][i]) - ref) / (u * S), depth(f, n)))
    elif k == "maxpy":
        nv, m, n_bd = case["nv"], case.get("m", 0), case.get("n_bd", 0)
        sg = case.get("sign", 1.0)
        terms = np.concatenate([_ld(inp["w"])[None, :], sg * _ld(inp["a"])[:, None] * _ld(inp["V"])])
        S = np.abs(terms).sum(axis=0)
        # w'_i: nv multiply-adds in sequence, two roundings each when they are not fused
        vec = (np.max(np.abs(_ld(got["w"]) - terms.sum(axis=0)) / (u * S)), 2 * nv)
        f = dict(maxpy_form(n, nv, maxpy_mp(case)), k=1 + (m if maxpy_mp(case) else 0))
        wn = _ld(got["w"])    # the sums are taken over the w' the kernel stored: their terms are exact
        ref, S = _sum_ld(wn * wn)
        red.append((abs(_ld(got["red"][0]) - ref) / (u * S), depth(f, n, per_tile=2 * f["U"])))
        for r in range(m if case.get("bd") else 0):
            ref, S = _sum_ld(_ld(inp["bd"][r, :n_bd]) * wn[:n_bd])
            red.append((abs(_ld(got["red"][1 + r]) - ref) / (u * S), depth(f, n, per_tile=2 * f["U"])))
    elif k == "norm":
        m, n_bd = case["m"], case["n_bd"]
        f = norm_form(n, m)
        x = _ld(got["x"])
        if case.get("sub"):   # one subtraction per entry
            vec = (np.max(np.abs(x - (_ld(inp["sa"]) - _ld(inp["sb"]))) / (u * (np.abs(inp["sa"]) + np.abs(inp["sb"])))), 1)
        ref, S = _sum_ld(x[:case["n_dot"]] ** 2)
        red.append((abs(_ld(got["red"][0]) - ref) / (u * S), depth(f, n, per_tile=2)))
        for r in range(m):
            ref, S = _sum_ld(_ld(inp["bd"][r, :n_bd]) * x[:n_bd])
            red.append((abs(_ld(got["red"][1 + r]) - ref) / (u * S), depth(f, n, per_tile=2)))
    elif k == "head":
        ref = head_reference(case, inp)
        worst = np.longdouble(0)
        for name in ("v", "z", "c", "wl"):
            if name in ref and name in got:
                S = ref["S"][name]
                err = np.abs(_ld(got[name]) - ref[name])
                ok = S > 0
                assert np.all(err[~ok] == 0)
                worst = max(worst, np.max(err[ok] / (u * S[ok])))
        vec = (worst, case["m"] + 4)
    return red, vec


def run_case(c, case):
    """-> dict(id, forms, ok, mismatch, got / expected digests; rounding tier: ratio, d, vratio, vd)."""
    inp = INPUTS[case["k"]](case)
    got = launch(c, case, inp)
    res = dict(id=case["id"], forms=case_forms(case))
    if case.get("gauss"):
        red, vec = gauss_ratio(case, inp, got)
        top = max(red, key=lambda t: t[0]) if red else None   # reported: the largest ratio; asserted: every one
        res.update(ratio=None if top is None else float(top[0]), d=None if top is None else int(top[1]),
                   vratio=None if vec is None else float(vec[0]), vd=None if vec is None else int(vec[1]))
        res["ok"] = bool(all(r <= d for r, d in red) and (vec is None or vec[0] <= vec[1]))
        res["mismatch"] = None if res["ok"] else f"rounding tier: ratio {res['ratio']} (d = {res['d']}), " \
                                                 f"vector ratio {res['vratio']} (d = {res['vd']})"
        return res
    exp = REFERENCE[case["k"]](case, inp)
    floor = None
    if case.get("pyth") == "floor" and case.get("done", -1) != 1:
        # 1 / sqrt(1.5e-14 ww) is no power of two: the square root within one ulp, the division and the product correctly
        # rounded leave the row t / sqrt(tt2) within 2 ulp; everything else of this case stays exact
        live, m = (case["nv"] if case.get("nv_live", -1) < 0 else case["nv_live"]), case["m"]
        g, e = got["tb"][live, :m].copy(), exp["tb"][live, :m].copy()
        got["tb"][live, :m] = exp["tb"][live, :m] = 0.0
        if not np.all(np.abs(g - e) <= 2 * np.spacing(np.abs(e))):
            floor = f"tb[{live}]: got {g!r}, expected {e!r} within 2 ulp"
    res.update(mismatch=first_mismatch(got, exp) or floor, got=digest(got), expected=digest(exp))
    res["ok"] = res["mismatch"] is None
    return res


# --------------------------------------------------------------------------- the case lists
def _case(k, ident, **kw):
    kw.update(k=k, id=ident)
    kw["seed"] = int(hashlib.sha256(ident.encode()).hexdigest()[:7], 16)
    return kw


def mdot_case(n, nv, nv2=0, split=0, n_dot=None, done=-1, gauss=0, tag=""):
    ident = f"mdot-n{n}-nv{nv}" + (f"-{'pl' if split else 'v2_'}{nv2}" if nv2 else "") + \
            (f"-nd{n_dot}" if n_dot is not None else "") + (f"-done{done}" if done >= 0 else "") + ("-gauss" if gauss else "") + tag
    return _case("mdot", ident, n=n, nv=nv, nv2=nv2, split=split, n_dot=n if n_dot is None else n_dot, done=done, gauss=gauss)


def maxpy_case(n, nv, sign=1.0, want_norm=1, nv_live=-1, bd=None, m=0, n_dot=None, w1side=0, pyth=None, pyth_k=0, done=-1,
               gauss=0, tag=""):
    n_bd = n - m if (bd or pyth) else 0
    ident = f"maxpy-n{n}-nv{nv}" + ("-neg" if sign < 0 else "") + ("" if want_norm else "-nonorm") + \
            (f"-live{nv_live}" if nv_live >= 0 else "") + (f"-{bd}{m}" if bd else "") + (f"-nd{n_dot}" if n_dot is not None else "") + \
            ("-side" if w1side else "") + (f"-{pyth}{m}" if pyth else "") + (f"-done{done}" if done >= 0 else "") + \
            ("-gauss" if gauss else "") + tag
    return _case("maxpy", ident, n=n, nv=nv, sign=sign, want_norm=want_norm, nv_live=nv_live, bd=bd, m=m, n_bd=n_bd,
                 n_dot=n if n_dot is None else n_dot, w1side=w1side, pyth=pyth, pyth_k=pyth_k, done=done, gauss=gauss)


def norm_case(n, m, sub=0, full=0, gauss=0):
    n_bd = n - m
    ident = f"norm-n{n}-m{m}" + ("-sub" if sub else "") + ("-full" if full else "") + ("-gauss" if gauss else "")
    return _case("norm", ident, n=n, m=m, n_bd=n_bd, n_dot=n if full else n_bd, sub=sub, gauss=gauss)


def pack_case(n, m, bad=None):
    return _case("pack", f"pack-n{n}-m{m}" + ("" if bad is None else f"-bad{'even' if bad == 0 else 'odd'}"), n=n, m=m, bad=bad)


def head_case(nl, m, packed=0, fact=SCHUR_FULL, jacobi=0, want_wl=0, gauss=0):
    ident = f"head-nl{nl}-m{m}" + ("-packed" if packed else "") + ("-full" if fact == SCHUR_FULL else "-lower") + \
            ("-jacobi" if jacobi else "") + ("-wl" if want_wl else "") + ("-gauss" if gauss else "")
    return _case("head", ident, nl=nl, m=m, packed=packed, fact=fact, jacobi=jacobi, want_wl=want_wl, gauss=gauss)


WS16_N = {2: [1, 2, 127, 128, 129, 257, 70001], 4: [131072, 131073], 8: [262144, 262145, 263169]}
STREAM_N = [1048576, 1048577, 1052673]
MAXPY_N = {(256, 1, 8): [1, 511, 512, 513, 70001], (256, 2, 8): [524288, 524289], (512, 4, 4): STREAM_N}
MAXPY_NV = [0, 1, 7, 8, 9, 17, 40, 63]


def mdot_ws16_cases():
    return [(U, mdot_case(n, nv)) for U, ns in WS16_N.items() for n in ns for nv in (0, 1, 16, 17, 32, 33, 40)]


def mdot_stream_cases():
    return [mdot_case(n, nv) for n in STREAM_N for nv in (1, 9, 17, 25, 40)]


def mdot_chunk_cases():
    return [mdot_case(n, nv) for n in (70001, 1048577) for nv in (41, 48, 63)]


def mdot_rider_cases(sizes=(70001, 131073, 262145, 1048577)):
    """One size per form (sixteen-wave U = 2, 4, 8 and the streaming form): n_dot, second slab, planes, 40 exactly, gate."""
    out = []
    for n in sizes:
        for m in range(1, 9):
            out.append(mdot_case(n, 5 + m, nv2=m))
            for nd in sorted({n - 1, n - m}):
                out.append(mdot_case(n, 5 + m, nv2=m, n_dot=nd))
        for m in (2, 4, 6, 8):
            out.append(mdot_case(n, 7 + m, nv2=m, split=1))
            out.append(mdot_case(n, 7 + m, nv2=m, split=1, n_dot=n - m))
            out.append(mdot_case(n, 2, nv2=m, split=1, n_dot=n - m + 1))
        out.append(mdot_case(n, 3, n_dot=n - 1))
        out.append(mdot_case(n, 3, n_dot=n - 2))
        out.append(mdot_case(n, 32, nv2=8, split=1, n_dot=n - 8, tag="-forty"))
        out.append(mdot_case(n, 33, nv2=7, tag="-forty"))
        out.append(mdot_case(n, 9, nv2=4, split=1, done=1))
        out.append(mdot_case(n, 9, nv2=4, split=1, done=0))
    return out


def maxpy_cases():
    out = []
    for form, ns in MAXPY_N.items():
        for j, n in enumerate(ns):
            for i, nv in enumerate(MAXPY_NV):
                out.append((form, maxpy_case(n, nv, sign=1.0 if (i + j) & 1 else -1.0)))
        n = ns[-1]
        out.append((form, maxpy_case(n, 9, want_norm=0)))
        out.append((form, maxpy_case(n, 17, nv_live=5, sign=-1.0)))
        out.append((form, maxpy_case(n, 9, nv_live=0)))
        out.append((form, maxpy_case(n, 3, n_dot=n - 1 if n > 1 else 0)))
        out.append((form, maxpy_case(n, 9, done=1)))
        out.append((form, maxpy_case(n, 9, done=0, sign=-1.0)))
    return out


def maxpy_plane_cases(bases=(504, 70000, 524290, 1048580), nv=5):
    """n = n_bd + m with n_bd even and odd; dense m = 1..8 (MP = 4, 8), packed m = 2, 4, 6, 8; n_dot = n_bd and n."""
    out = []
    for base in bases:
        for m in range(1, 9):
            for odd in (0, 1):
                n = base + odd + m
                out.append(maxpy_case(n, nv, sign=-1.0, bd="dense", m=m, w1side=1, n_dot=n - m if (m + odd) & 1 else None))
        for m in (2, 4, 6, 8):
            for odd in (0, 1):
                n = base + odd + m
                out.append(maxpy_case(n, nv, sign=-1.0, bd="packed", m=m, w1side=1, n_dot=None if (m // 2 + odd) & 1 else n - m))
        out.append(maxpy_case(base + 4, nv, bd="packed", m=4, w1side=0))
        out.append(maxpy_case(base + 4, nv, bd="dense", m=4, want_norm=0, w1side=1, n_dot=base))
    return out


def maxpy_pyth_cases():
    out = []
    for n, nv in ((70001, 30), (1048580, 3)):
        for m in (1, 4, 8):
            out.append(maxpy_case(n + m, nv, sign=-1.0, want_norm=0, m=m, w1side=1, pyth="pow4", pyth_k=m - 3, n_dot=n))
        out.append(maxpy_case(n + 4, nv, sign=-1.0, want_norm=0, m=4, w1side=1, pyth="floor", n_dot=n))
    out.append(maxpy_case(514 + 4, 63, sign=-1.0, want_norm=0, m=4, w1side=1, pyth="pow4", pyth_k=2, n_dot=514))
    out.append(maxpy_case(514 + 4, 40, nv_live=11, sign=-1.0, want_norm=0, m=4, w1side=1, pyth="pow4", pyth_k=1, n_dot=514))
    out.append(maxpy_case(514 + 2, 0, sign=-1.0, want_norm=0, m=2, w1side=1, pyth="pow4", pyth_k=0, n_dot=514))
    return out


def norm_cases():
    out = []
    for n in (1, 1023, 1024, 1025, 262145):
        for m in range(0, 9):
            if n >= m:   # n = n_bd + m: consecutive m (and 1024 / 1025) give both parities of n_bd
                out.append(norm_case(n, m, sub=0, full=m & 1))
                out.append(norm_case(n, m, sub=1, full=1 - (m & 1)))
    return out


def pack_cases():
    out = [pack_case(n, m) for n in (1, 255, 256, 257, 70001) for m in range(1, 9)]
    out += [pack_case(n, m, bad=b) for n in (257, 70001) for m in (2, 5, 8) for b in (0, 1)]
    return out


HEAD_NL = [2, 510, 512, 514, 4 * 256 * 2048 + 2]


def head_cases():
    out = []
    for nl in HEAD_NL:
        for fact in (SCHUR_LOWER, SCHUR_FULL):
            for m in (0, 1, 4, 5, 8):
                out.append(head_case(nl, m, fact=fact, want_wl=(m + fact) & 1 if m else 0))
            for m in (2, 4, 6, 8):
                out.append(head_case(nl, m, packed=1, fact=fact, want_wl=(m // 2 + fact) & 1))
        out.append(head_case(nl, 0, fact=SCHUR_LOWER, jacobi=1))
    return out


def gauss_cases():
    """One case per launch form of a default process."""
    return [mdot_case(70001, 17, nv2=4, split=1, gauss=1), mdot_case(131073, 33, nv2=3, gauss=1),
            mdot_case(263169, 30, nv2=2, split=1, gauss=1), mdot_case(1052673, 12, nv2=4, split=1, gauss=1),
            maxpy_case(70001 + 4, 30, sign=-1.0, bd="packed", m=4, gauss=1), maxpy_case(524289 + 5, 12, sign=-1.0, bd="dense", m=5, gauss=1),
            maxpy_case(1052673 + 4, 6, sign=-1.0, bd="packed", m=4, gauss=1),
            norm_case(262145, 8, sub=1, full=1, gauss=1), norm_case(1025, 3, gauss=1),
            head_case(70000, 5, fact=SCHUR_FULL, want_wl=1, gauss=1), head_case(70000, 8, packed=1, fact=SCHUR_FULL, gauss=1),
            head_case(70000, 4, fact=SCHUR_LOWER, gauss=1)]


def knob_cases(knob):
    """The exact-tier list (and one rounding-tier case per form) of a child process: -> (env, cases)."""
    if knob == "SPK_VEC_WS":       # mdot_kernel at T = 256: U = 1, 2, 4, NG = 1 .. 5 each (1048575 entries: already T = 512)
        cases = [mdot_case(n, nv) for n in (255, 70001, 262145, 524289, 1048573, 1048575) for nv in (1, 9, 17, 25, 40)]
        cases += [mdot_case(n, 11, nv2=6, split=1, n_dot=n - 6) for n in (70001, 262145, 524289)]
        cases += [mdot_case(n, 48) for n in (70001, 524289)]
        cases += [mdot_case(n, 20, nv2=4, split=1, gauss=1) for n in (70001, 262145, 1048573)]
        return {"SPK_VEC_WS": "0"}, cases
    if knob == "SPK_VEC_WS16":     # mdot_ws_kernel: VW 4 / 8 / 12, U 2 / 4 / 8, with planes and a second slab
        cases = [mdot_case(n, nv) for n in (129, 131073, 262145) for nv in (1, 16, 17, 32, 33, 40)]
        for n in (129, 131073, 262145):
            cases += [mdot_case(n, 11, nv2=6, split=1, n_dot=n - 6), mdot_case(n, 30, nv2=5, n_dot=n - 1),
                      mdot_case(n, 32, nv2=8, split=1, tag="-forty"), mdot_case(n, 41), mdot_case(n, 5, done=1),
                      mdot_case(n, 30, nv2=4, split=1, gauss=1)]
        return {"SPK_VEC_WS16": "0"}, cases
    if knob == "SPK_VEC_DEEP":     # maxpy_kernel with G = 16 and 32, with planes
        cases = [maxpy_case(n, nv, sign=-1.0 if nv & 1 else 1.0) for n in (513, 524289) for nv in (9, 16, 17, 33, 63)]
        for n in (513, 524289):
            for nv in (9, 17, 33):
                cases += [maxpy_case(n + 3, nv, sign=-1.0, bd="dense", m=3, w1side=1, n_dot=n),
                          maxpy_case(n + 7, nv, sign=-1.0, bd="dense", m=7, w1side=1),
                          maxpy_case(n + 4, nv, sign=-1.0, bd="packed", m=4, w1side=1, n_dot=n),
                          maxpy_case(n + 8, nv, sign=-1.0, bd="packed", m=8, w1side=1)]
            cases += [maxpy_case(n, 33, nv_live=10), maxpy_case(n, 17, want_norm=0),
                      maxpy_case(n + 4, 30, sign=-1.0, bd="packed", m=4, gauss=1), maxpy_case(n + 4, 12, sign=-1.0, bd="packed", m=4, gauss=1)]
        return {"SPK_VEC_DEEP": "1"}, cases
    raise ValueError(knob)


def main(case_file, out_file):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import saddle_point_petsc_amd as S
    with open(case_file) as fh:
        cases = json.load(fh)
    results = []
    with S.Context(0) as c:
        probe = {str(n): c.debug_vec_shape(n) for n in sorted({cs["n"] for cs in cases})}
        for cs in cases:
            results.append(run_case(c, cs))
            with open(out_file, "w") as fh:   # rewritten after every case: a child that dies leaves what it had
                json.dump(dict(shapes=probe, results=results), fh)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
