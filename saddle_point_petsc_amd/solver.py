"""Thin object wrappers over the C ABI (include/spk.h) and the KSP facade
(include/spk_ksp.h).  `KSP` mirrors the reference's call site
/root/reference/src/SaddlePointProblem.c:65-72 (petsc4py-style method names)."""
import ctypes as C
import math

import numpy as np

from ._lib import lib, Opts, Result, MatCSR, SpkError, AmgOpts, AmgInfo

PC_NONE, PC_JACOBI, PC_SCHUR = 0, 1, 2
SCHUR_DIAG, SCHUR_LOWER, SCHUR_UPPER, SCHUR_FULL = 0, 1, 2, 3
BLOCK_A00, BLOCK_A10 = 0, 1
MEM_HOST, MEM_DEVICE = 0, 1
NORM_UNPRECONDITIONED, NORM_NATURAL = 0, 1
DIVERGED_INDEFINITE_PC = -8
DIVERGED_INDEFINITE_MAT = -10
PIPECGRR_TAU_DEFAULT = 1e-6   # SPK_PIPECGRR_TAU_DEFAULT (include/spk.h)
_NORMS = {"unpreconditioned": NORM_UNPRECONDITIONED, "natural": NORM_NATURAL}
SCHUR_PRE_SELFP_DIAG, SCHUR_PRE_FULL = 0, 1
_SCHUR_PRES = {"selfp": SCHUR_PRE_SELFP_DIAG, "full": SCHUR_PRE_FULL}


BASIS_DOUBLE, BASIS_SINGLE = 0, 1   # SPK_BASIS_* (include/spk.h)
_BASES = {"double": BASIS_DOUBLE, "single": BASIS_SINGLE}


def default_opts(**kw):
    """spk_opts with PETSc's defaults, overridden by keyword.  basis="double" | "single" sets basis_precision: how the
    Krylov basis of fgmres is stored (single: FP32 storage, FP64 arithmetic, iteration form 5 on one rank)."""
    o = Opts()
    lib.spk_default_opts(C.byref(o))
    for k, v in kw.items():
        if k == "basis":
            if v not in _BASES:
                raise ValueError(f"basis must be one of {sorted(_BASES)}")
            k, v = "basis_precision", _BASES[v]
        if not hasattr(o, k):
            raise TypeError(f"unknown solver option {k}")
        setattr(o, k, v)
    return o


AMG_CHEBYSHEV, AMG_RICHARDSON = 0, 1
AMG_OP, AMG_PROLONG, AMG_TENTATIVE, AMG_COARSE_INV = 0, 1, 2, 3
AMG_SETUP_HOST, AMG_SETUP_DEVICE = 0, 1
AMG_COARSEN_AGGREGATION, AMG_COARSEN_GRID = 0, 1
AMG_TRANSFER_MATRIX_FREE, AMG_TRANSFER_STORED = 0, 1
AMG_SIDES_ODD, AMG_SIDES_ANY = 0, 1
AMG_CYCLE_V, AMG_CYCLE_W = 0, 1
AMG_GALERKIN_PRODUCTS, AMG_GALERKIN_STENCIL = 0, 1
AMG_OPERATOR_CSR, AMG_OPERATOR_STENCIL = 0, 1
AMG_LANCZOS_STEPWISE, AMG_LANCZOS_RESIDENT = 0, 1
AMG_PRECISION_DOUBLE, AMG_PRECISION_SINGLE = 0, 1
AMG_TAIL_AUTO, AMG_TAIL_LAUNCHES, AMG_TAIL_FUSED = 0, 1, 2
AMG_STEP_PRE0, AMG_STEP_PRE, AMG_STEP_DOWN, AMG_STEP_COARSE, AMG_STEP_UP, AMG_STEP_POST = range(6)
SPK_ERR_ARG = -1   # include/spk.h
_SMOOTHERS = {"chebyshev": AMG_CHEBYSHEV, "richardson": AMG_RICHARDSON}
_SETUPS = {"host": AMG_SETUP_HOST, "device": AMG_SETUP_DEVICE}
_COARSENINGS = {"aggregation": AMG_COARSEN_AGGREGATION, "grid": AMG_COARSEN_GRID}
_TRANSFERS = {"matrixfree": AMG_TRANSFER_MATRIX_FREE, "stored": AMG_TRANSFER_STORED}
_SIDES = {"odd": AMG_SIDES_ODD, "any": AMG_SIDES_ANY}
_CYCLES = {"v": AMG_CYCLE_V, "w": AMG_CYCLE_W}
_GALERKINS = {"products": AMG_GALERKIN_PRODUCTS, "stencil": AMG_GALERKIN_STENCIL}
_OPERATORS = {"csr": AMG_OPERATOR_CSR, "stencil": AMG_OPERATOR_STENCIL}
_LANCZOS = {"stepwise": AMG_LANCZOS_STEPWISE, "resident": AMG_LANCZOS_RESIDENT}
_PRECISIONS = {"double": AMG_PRECISION_DOUBLE, "single": AMG_PRECISION_SINGLE}
_TAILS = {"auto": AMG_TAIL_AUTO, "launches": AMG_TAIL_LAUNCHES, "fused": AMG_TAIL_FUSED}


def amg_opts(**kw):
    """spk_amg_opts with PETSc's defaults, overridden by keyword (smoother may be 'chebyshev' / 'richardson', setup
    'host' / 'device', coarsening 'aggregation' / 'grid', transfer 'matrixfree' / 'stored', sides 'odd' / 'any', cycle
    'v' / 'w', tail 'auto' / 'launches' / 'fused', galerkin 'products' / 'stencil' (what forms the coarse operators of a
    grid-coarsened hierarchy: the generic sparse products, or the gather on the node grid), operator 'csr' / 'stencil'
    (how the cycle applies the levels between level 0 and the coarsest: as sparse matrices, or from their value arrays
    alone -- the struct's field is `op`; 'stencil' needs coarsening='grid' and galerkin='stencil'), lanczos 'stepwise' /
    'resident' (who holds the scalars of the device set-up's Lanczos: the host, reading two sums back per step, or a block
    on the device read once per level -- the same hierarchy to the bit; 'resident' needs setup='device'), precision
    'double' / 'single' (what the levels >= 1 of the cycle run in: 'single' keeps the FP64 hierarchy and level 0 and runs
    the other levels in FP32 on rounded copies; it needs coarsening='grid', galerkin='stencil', operator='stencil' and
    transfer='matrixfree');
    grid=(mx, my[, mz]) are the nodes per side that grid coarsening halves: the odd ones, or under sides='any' the even
    ones too)."""
    o = AmgOpts()
    lib.spk_default_amg_opts(C.byref(o))
    for k, v in kw.items():
        if k == "operator":
            k = "op"
            if isinstance(v, str):
                v = _OPERATORS[v]
        if not hasattr(o, k):
            raise TypeError(f"unknown multigrid option {k}")
        if k == "smoother" and isinstance(v, str):
            v = _SMOOTHERS[v]
        if k == "setup" and isinstance(v, str):
            v = _SETUPS[v]
        if k == "coarsening" and isinstance(v, str):
            v = _COARSENINGS[v]
        if k == "transfer" and isinstance(v, str):
            v = _TRANSFERS[v]
        if k == "sides" and isinstance(v, str):
            v = _SIDES[v]
        if k == "cycle" and isinstance(v, str):
            v = _CYCLES[v]
        if k == "tail" and isinstance(v, str):
            v = _TAILS[v]
        if k == "galerkin" and isinstance(v, str):
            v = _GALERKINS[v]
        if k == "lanczos" and isinstance(v, str):
            v = _LANCZOS[v]
        if k == "precision" and isinstance(v, str):
            v = _PRECISIONS[v]
        if k == "esteig":
            v = (C.c_double * 4)(*v)
        if k == "grid":
            v = tuple(int(m) for m in v)
            if len(v) not in (2, 3):
                raise TypeError("grid takes (mx, my) or (mx, my, mz)")
            v = (C.c_int32 * 3)(*(v + (1,) * (3 - len(v))))
        setattr(o, k, v)
    return o


def amg_opts_dict(o):
    d = {k: getattr(o, k) for k, _ in AmgOpts._fields_}
    d["esteig"] = tuple(o.esteig)
    d["grid"] = tuple(o.grid)
    d["operator"] = o.op
    return d


def _amg_info(ai):
    L = ai.levels
    return dict(levels=L, block_size=ai.block_size, rows=list(ai.rows[:L]), nnz=list(ai.nnz[:L]),
                lambda_max=list(ai.lambda_max[:L]), operator_complexity=ai.operator_complexity,
                setup_seconds=ai.setup_seconds, setup=ai.setup, coarsening=ai.coarsening,
                dims=[tuple(ai.dims[l]) for l in range(L)], sides=ai.sides, cycle=ai.cycle, tail_first=ai.tail_first,
                tail_launches=ai.tail_launches, galerkin=ai.galerkin, operator=ai.op, lanczos=ai.lanczos,
                ritz_readbacks=ai.ritz_readbacks, precision=ai.precision)


def amg_stencil_children(fine, coarse, node):
    """The fine nodes of coarse node `node` between the node grids fine -> coarse (three sides each) under
    galerkin='stencil', ascending, and their weights (spk_amg_stencil_children, host only)."""
    f, c = (C.c_int32 * 3)(*fine), (C.c_int32 * 3)(*coarse)
    n = C.c_int32()
    nodes, w = np.zeros(27, np.int32), np.zeros(27, np.float64)
    rc = lib.spk_amg_stencil_children(f, c, int(node), C.byref(n), nodes.ctypes.data, w.ctypes.data)
    if rc != 0:
        raise SpkError(rc, (lib.spk_last_error(None) or b"").decode())
    return nodes[:n.value].copy(), w[:n.value].copy()


def amg_cycle_steps(levels, cycle="v"):
    """The steps of one multigrid cycle over `levels` levels in the order the library runs them (spk_amg_cycle_steps,
    host only): a list of (kind, level), kind one of AMG_STEP_*."""
    cyc = _CYCLES[cycle] if isinstance(cycle, str) else int(cycle)
    n = C.c_int64()
    rc = lib.spk_amg_cycle_steps(levels, cyc, C.byref(n), None)
    if rc != 0:
        raise SpkError(rc, (lib.spk_last_error(None) or b"").decode())
    st = np.zeros((n.value, 2), np.int32)
    rc = lib.spk_amg_cycle_steps(levels, cyc, C.byref(n), st.ctypes.data)
    if rc != 0:
        raise SpkError(rc, (lib.spk_last_error(None) or b"").decode())
    return [tuple(int(x) for x in r) for r in st]


def _amg_matrix(fn, level, which):
    """scipy-free CSR triple (rowptr, colidx, val, shape) of one matrix of a level, through a sized two-call getter."""
    nr, nc, nz = C.c_int32(), C.c_int32(), C.c_int64()
    fn(level, which, C.byref(nr), C.byref(nc), C.byref(nz), None, None, None)
    rp = np.zeros(nr.value + 1, np.int32)
    ci = np.zeros(nz.value, np.int32)
    v = np.zeros(nz.value, np.float64)
    fn(level, which, C.byref(nr), C.byref(nc), C.byref(nz), rp.ctypes.data, ci.ctypes.data, v.ctypes.data)
    return rp, ci, v, (nr.value, nc.value)


class AmgHierarchy:
    """Host-only multigrid hierarchy (spk_amg_build_host): the set-up the context runs at spk_pc_setup, without a GPU."""

    def __init__(self, A, **kw):
        self.h = C.c_void_p()
        o = amg_opts(**kw)
        rc = lib.spk_amg_build_host(A.nrows, A.rowptr, A.colidx, A.val, C.byref(o), C.byref(self.h))
        if rc != 0:
            raise SpkError(rc, lib.spk_last_error(None).decode())
        self._nnz = int(A.rowptr[A.nrows])

    def _chk(self, rc):
        if rc != 0:
            raise SpkError(rc, lib.spk_last_error(None).decode())

    def info(self):
        ai = AmgInfo()
        self._chk(lib.spk_amg_host_info(self.h, C.byref(ai)))
        return _amg_info(ai)

    def matrix(self, level, which=AMG_OP):
        return _amg_matrix(lambda *a: self._chk(lib.spk_amg_host_level(self.h, *a)), level, which)

    def refresh(self, val):
        """New values on the same pattern (spk_amg_refresh_host), in the order of the A.val this hierarchy was built
        from: the aggregates, the prolongators and every pattern stay; the coarse operators, the intervals and the coarse
        inverse are computed again.  None or another length: SPK_ERR_ARG."""
        if val is None:
            self._chk(lib.spk_amg_refresh_host(self.h, None))
            return
        v = np.ascontiguousarray(val, np.float64)
        if v.shape != (self._nnz,):
            raise SpkError(SPK_ERR_ARG, f"amg refresh: {v.size} values for a pattern of {self._nnz} entries")
        self._chk(lib.spk_amg_refresh_host(self.h, v.ctypes.data))

    def aggregates(self, level):
        n = C.c_int32()
        self._chk(lib.spk_amg_host_aggregates(self.h, level, C.byref(n), None))
        agg = np.zeros(n.value, np.int32)
        self._chk(lib.spk_amg_host_aggregates(self.h, level, C.byref(n), agg.ctypes.data))
        return agg

    def close(self):
        if self.h:
            lib.spk_amg_destroy_host(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        self.close()


def unique_id():
    buf = C.create_string_buffer(128)
    rc = lib.spk_comm_unique_id(buf)
    if rc != 0:
        raise SpkError(rc, lib.spk_last_error(None).decode())
    return buf.raw


class LocalGroup:
    """In-process logical ranks on one device (parity tests only)."""

    def __init__(self, nranks):
        self.h = C.c_void_p()
        rc = lib.spk_local_group_create(C.byref(self.h), nranks)
        if rc != 0:
            raise SpkError(rc, "spk_local_group_create")
        self.nranks = nranks

    def close(self):
        if self.h:
            lib.spk_local_group_destroy(self.h)
            self.h = C.c_void_p()


class Context:
    """One solver context (= one KSP) on one GPU."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        rc = lib.spk_create(C.byref(self.h), device)
        if rc != 0:
            raise SpkError(rc, lib.spk_last_error(None).decode())

    def _chk(self, rc):
        if rc != 0:
            raise SpkError(rc, lib.spk_last_error(self.h).decode())

    def close(self):
        if self.h:
            lib.spk_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def comm_init_rccl(self, rank, nranks, id128):
        self._chk(lib.spk_comm_init_rccl(self.h, rank, nranks, id128))

    def comm_init_torch(self, dist, rank, nranks):
        """Rehearsal transport over an initialised torch.distributed group (gloo): lets several
        processes share one GPU, which RCCL refuses.  Slow: every collective goes through the host."""
        import torch
        from ._lib import HostComm, ALLREDUCE_CB, EXCHANGE_CB, ALLGATHER_CB

        def allreduce(_u, buf, count):
            a = np.ctypeslib.as_array(buf, shape=(count,))
            t = torch.from_numpy(a.copy())
            dist.all_reduce(t)
            a[:] = t.numpy()
            return 0

        def exchange(_u, peer, send, nsend, recv, nrecv):
            reqs = []
            if nsend:
                reqs.append(dist.isend(torch.from_numpy(np.ctypeslib.as_array(send, shape=(nsend,)).copy()), peer))
            rt = torch.zeros(max(nrecv, 1), dtype=torch.float64)
            if nrecv:
                reqs.append(dist.irecv(rt[:nrecv], peer))
            for r in reqs:
                r.wait()
            if nrecv:
                np.ctypeslib.as_array(recv, shape=(nrecv,))[:] = rt[:nrecv].numpy()
            return 0

        def allgather(_u, inp, out, nbytes):
            mine = torch.frombuffer(bytearray(C.string_at(inp, nbytes)), dtype=torch.uint8)
            parts = [torch.zeros(nbytes, dtype=torch.uint8) for _ in range(nranks)]
            dist.all_gather(parts, mine)
            C.memmove(out, b"".join(bytes(p.numpy().tobytes()) for p in parts), nbytes * nranks)
            return 0

        self._cbs = (ALLREDUCE_CB(allreduce), EXCHANGE_CB(exchange), ALLGATHER_CB(allgather))   # keep alive
        self._hc = HostComm(None, *self._cbs)
        self._chk(lib.spk_comm_init_host(self.h, rank, nranks, C.byref(self._hc)))

    def comm_init_local(self, group, rank):
        self._chk(lib.spk_comm_init_local(self.h, group.h, rank))

    def comm_enable_peer(self):
        """Peer-store collectives over xGMI on top of the communicator set before (collective).
        Returns True when they are active, False when the previous backend stays (see
        spk_comm_enable_peer in include/spk.h)."""
        on = C.c_int32()
        self._chk(lib.spk_comm_enable_peer(self.h, C.byref(on)))
        return bool(on.value)

    def last_error(self):
        return lib.spk_last_error(self.h).decode()

    def comm_backend(self):
        return lib.spk_comm_backend(self.h).decode()

    def comm_info(self):
        """Per-rank diagnostics of the communicator (spk_comm_get_info): backend, why the peer-store
        backend is off if it is, window memory kind, collective counts, device-side wait times."""
        from ._lib import CommInfo
        ci = CommInfo()
        self._chk(lib.spk_comm_get_info(self.h, C.byref(ci)))
        kinds = ("allreduce_after_mdot", "allreduce_after_maxpy", "allreduce_standalone", "halo")
        return dict(rank=ci.rank, nranks=ci.nranks, device=ci.device, backend=ci.backend.decode(),
                    inner_backend=ci.inner_backend.decode(), peer_enabled=bool(ci.peer_enabled),
                    window_memory={0: "uncached", 1: "fine-grained", 2: "plain"}.get(ci.window_tier, "none"),
                    self_test_ok=bool(ci.self_test_ok),
                    halo={0: "none", 1: "granules", 2: "bulk", 3: "inner-backend"}[ci.halo_mode],
                    halo_fused=bool(ci.halo_fused),
                    allreduce=dict(fused=ci.n_allreduce_fused, kernel=ci.n_allreduce_kernel, inner=ci.n_allreduce_inner),
                    halo_exchanges=dict(fused=ci.n_halo_fused, kernel=ci.n_halo_kernel, inner=ci.n_halo_inner),
                    # 100 MHz ticks -> microseconds, mean per wait
                    wait_us={k: (ci.wait_ticks[i] / 100.0 / ci.wait_count[i] if ci.wait_count[i] else None)
                             for i, k in enumerate(kinds)},
                    wait_count={k: int(ci.wait_count[i]) for i, k in enumerate(kinds)},
                    why=ci.why.decode())

    def debug_peer_allreduce_loopback(self, vals, rounds=6):
        """Test hook: nranks x count inputs -> nranks x count rank-ordered sums (one launch, no IPC)."""
        vals = np.ascontiguousarray(vals, np.float64)
        out = np.zeros_like(vals)
        self._chk(lib.spk_debug_peer_allreduce_loopback(self.h, vals.shape[0], vals.shape[1], rounds,
                                                        vals.reshape(-1), out.reshape(-1)))
        return out

    def debug_finish_timeout(self, timeout_ms=50):
        """Test hook: a reduction with a partial that never arrives; raises SpkError (SPK_ERR_HIP)."""
        self._chk(lib.spk_debug_finish_timeout(self.h, timeout_ms))

    def debug_wave_sums(self, vals):
        """Test hook: na x 512 inputs -> (2, 8, na) wave sums, [0] by wave_sum per value, [1] by wave_sum_multi."""
        vals = np.ascontiguousarray(vals, np.float64)
        na = vals.shape[0]
        if vals.shape != (na, 512):
            raise ValueError("debug_wave_sums: na x 512 values")
        out = np.zeros(16 * na)
        self._chk(lib.spk_debug_wave_sums(self.h, na, vals.reshape(-1), out))
        return out.reshape(2, 8, na)

    # ---- test hooks of the Gram-Schmidt kernels (include/spk.h): host arrays in, the production wrapper, results out ----
    @staticmethod
    def _f64(a, shape=None):
        a = np.ascontiguousarray(a, np.float64)
        if shape is not None and a.shape != tuple(shape):
            raise ValueError(f"expected an array of shape {tuple(shape)}, got {a.shape}")
        return a

    @staticmethod
    def _ptr(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    def debug_vec_shape(self, n):
        """Launch shapes of a vector of n entries: dict(ws=(on, U, grid), mdot=(T, U, G, grid), maxpy=(T, U, G, grid),
        ws16=knob, deep=knob)."""
        out = np.zeros(13, np.int32)
        self._chk(lib.spk_debug_vec_shape(self.h, n, out))
        o = [int(x) for x in out]
        return dict(ws=tuple(o[0:3]), mdot=tuple(o[3:7]), maxpy=tuple(o[7:11]), ws16=o[11], deep=o[12])

    def debug_mdot(self, V, w, n_dot=None, V2=None, split=0, done=-1, pad=0.0):
        """k::mdot: V (nv, n), w (n,), V2 (nv2, n) dense rows or, with split, (nv2 / 2, n) parity planes.
        Returns the nv + nv2 + 1 outputs (SPK_DEBUG_MARKER where the launch wrote nothing)."""
        from ._lib import DebugMdotOpts
        w = self._f64(w)
        n = w.shape[0]
        V = self._f64(V, (np.shape(V)[0], n))
        rows2 = 0 if V2 is None else np.shape(V2)[0]
        V2 = None if V2 is None else self._f64(V2, (rows2, n))
        nv, nv2 = V.shape[0], (2 * rows2 if split else rows2)
        o = DebugMdotOpts(n, n if n_dot is None else n_dot, nv, nv2, int(split), int(done), float(pad))
        out = np.zeros(nv + nv2 + 1)
        self._chk(lib.spk_debug_mdot(self.h, C.byref(o), self._ptr(V), self._ptr(V2), w, out))
        return out

    def debug_mdot_f32(self, V, w, n_dot=None, V2=None, split=0, done=-1, pad=0.0):
        """k::mdot_f32, VecMDot over an FP32 basis: as debug_mdot with V (nv, n) float32; w and V2 stay float64.  Behind
        the nv + nv2 + 1 values of debug_mdot come the nv2 plane values of V[-1] (the first n_dot entries)."""
        from ._lib import DebugMdotOpts
        w = self._f64(w)
        n = w.shape[0]
        V = np.ascontiguousarray(V, np.float32)
        if V.shape != (np.shape(V)[0], n):
            raise ValueError(f"expected an array of shape {(np.shape(V)[0], n)}, got {V.shape}")
        rows2 = 0 if V2 is None else np.shape(V2)[0]
        V2 = None if V2 is None else self._f64(V2, (rows2, n))
        nv, nv2 = V.shape[0], (2 * rows2 if split else rows2)
        o = DebugMdotOpts(n, n if n_dot is None else n_dot, nv, nv2, int(split), int(done), float(pad))
        out = np.zeros(nv + 2 * nv2 + 1)
        self._chk(lib.spk_debug_mdot_f32(self.h, C.byref(o), self._ptr(V), self._ptr(V2), w, out))
        return out

    def debug_maxpy(self, V, a, w, sign=1.0, n_dot=None, nv_live=-1, want_norm=1, bd=None, packed=0, n_bd=0, m=0,
                    w1side=0, pyth=None, done=-1, pad=0.0):
        """k::maxpy: V (nv, n), a (nv,), w (n,); bd: (m, n) dense rows or, packed, (m / 2, n) parity planes;
        pyth: dict(dots=(nv_live + m + 1,), tb=(nv + 1, 8)) switches the single-reduction rider on.
        Returns dict(w, red (1 + m), w1side (m), nrm_out (1 + m), tb)."""
        from ._lib import DebugMaxpyOpts
        w = self._f64(w).copy()
        n = w.shape[0]
        V = self._f64(V, (np.shape(V)[0], n))
        nv = V.shape[0]
        a = self._f64(a, (nv,))
        mode = 0 if bd is None else (2 if packed else 1)
        bd = None if bd is None else self._f64(bd, ((m // 2 if packed else m), n))
        live = nv if nv_live < 0 else nv_live
        dots = tb = None
        if pyth is not None:
            dots = self._f64(pyth["dots"], (live + m + 1,))
            tb = self._f64(pyth["tb"], (nv + 1, 8)).copy()
        o = DebugMaxpyOpts(n, n if n_dot is None else n_dot, n_bd, float(sign), float(pad), nv, nv_live, int(want_norm), m, mode,
                           int(w1side), int(pyth is not None), int(done))
        red, side, nrm_out = np.zeros(1 + m), np.zeros(max(m, 1)), np.zeros(1 + m)
        self._chk(lib.spk_debug_maxpy(self.h, C.byref(o), self._ptr(V), a, w, self._ptr(bd), self._ptr(dots), self._ptr(tb), red,
                                      self._ptr(side), self._ptr(nrm_out)))
        return dict(w=w, red=red, w1side=side[:m], nrm_out=nrm_out, tb=tb)

    def debug_cycle_norm(self, x, bd, n_bd, n_dot=None, sub=None, pad=0.0):
        """k::sqnorm_bd: x (n,), bd (m, n) dense planes; sub = (sa, sb): x = sa - sb is formed on the way.
        Returns dict(x, red (1 + m), w1side (m))."""
        bd = self._f64(bd)
        m = bd.shape[0]
        sa = sb = None
        if sub is not None:
            sa, sb = self._f64(sub[0]), self._f64(sub[1])
            x = np.zeros_like(sa)
        x = self._f64(x).copy()
        n = x.shape[0]
        if m and bd.shape != (m, n):
            raise ValueError("debug_cycle_norm: bd must be (m, n)")
        red, side = np.zeros(1 + m), np.zeros(max(m, 1))
        self._chk(lib.spk_debug_cycle_norm(self.h, n, n if n_dot is None else n_dot, n_bd, m, float(pad), x, self._ptr(sa),
                                           self._ptr(sb), self._ptr(bd) if m else None, red, self._ptr(side)))
        return dict(x=x, red=red, w1side=side[:m])

    def debug_schur_w(self, W, L, x, fact=SCHUR_FULL, src=None, dinv=None, done=-1, pad=0.0):
        """The dense-Schur kernels as op_pc_apply chains them: W (m, nl) planes, L (m, m) Cholesky factor, x (nl + m,).
        Returns the whole padded output row (SPK_DEBUG_MARKER where nothing was written)."""
        W = self._f64(W)
        m, nl = W.shape
        L = self._f64(L, (m, m))
        x = self._f64(x, (nl + m,))
        src = None if src is None else self._f64(src, (nl,))
        dinv = None if dinv is None else self._f64(dinv, (nl,))
        y = np.zeros((nl + m + 255) // 256 * 256)
        self._chk(lib.spk_debug_schur_w(self.h, nl, m, int(fact), int(done), float(pad), W, L, x, self._ptr(src), self._ptr(dinv), y))
        return y

    def debug_pack_bd(self, bd):
        """k::pack_bd: bd (m, n) dense rows -> ((m // 2, n) planes, bad word)."""
        bd = self._f64(bd)
        m, n = bd.shape
        bdp = np.zeros((max(m // 2, 1), n))
        bad = C.c_int32(-1)
        self._chk(lib.spk_debug_pack_bd(self.h, n, m, bd, self._ptr(bdp), C.byref(bad)))
        return bdp[:m // 2], bad.value

    def debug_cycle_head(self, v, nrm, dinv, w1raw=None, bd=None, shat=None, gram=None, fact=SCHUR_FULL, packed=0, jacobi=False,
                         want_wl=False, pad=0.0):
        """k::fused_head (no Givens rider, no halo): v (nl + m,), nrm (1 + m,), dinv (nl,), bd (m, nl) dense rows or, packed,
        (m / 2, nl) planes.  Returns dict(v, z, c, wl); c is None for the Jacobi head."""
        from ._lib import DebugHeadOpts
        dinv = self._f64(dinv)
        nl = dinv.shape[0]
        nrm = self._f64(nrm)
        m = nrm.shape[0] - 1
        v = self._f64(v, (nl + m,)).copy()
        if m:
            w1raw, shat, gram = self._f64(w1raw, (m,)), self._f64(shat, (m,)), self._f64(gram, (m, m))
            bd = self._f64(bd, ((m // 2 if packed else m), nl))
        else:
            w1raw = shat = gram = bd = None
        z = np.zeros(nl + m)
        c = None if jacobi else np.zeros(nl + m)
        wl = np.zeros(max(m, 1))
        o = DebugHeadOpts(nl, m, int(packed), int(fact), int(bool(jacobi)), int(bool(want_wl)), 0, float(pad))
        self._chk(lib.spk_debug_cycle_head(self.h, C.byref(o), v, nrm, self._ptr(w1raw), dinv, self._ptr(bd), self._ptr(shat),
                                           self._ptr(gram), z, self._ptr(c), self._ptr(wl)))
        return dict(v=v, z=z, c=c, wl=wl[:m] if want_wl else None)

    def debug_gs_stamps(self):
        """Developer hook (GS_STAMPS=1 builds): (64, 256, 8) time stamps of the fused Gram-Schmidt launches, 100 MHz ticks."""
        out = np.zeros(64 * 256 * 8, np.uint64)
        self._chk(lib.spk_debug_gs_stamps(self.h, out))
        return out.reshape(64, 256, 8)

    def time_products(self, max_launches):
        """HIP events around the product launches of the next solves' iterations (0: off); see include/spk.h"""
        self._chk(lib.spk_debug_time_products(self.h, max_launches))

    def product_timing(self):
        n, ng, gm = C.c_int32(), C.c_int32(), C.c_double()
        v = [C.c_double() for _ in range(4)]
        self._chk(lib.spk_get_product_timing(self.h, C.byref(n), *[C.byref(x) for x in v], C.byref(ng), C.byref(gm)))
        return dict(launches=n.value, mean_ms=v[0].value, median_ms=v[1].value, min_ms=v[2].value, max_ms=v[3].value,
                    gated=ng.value, gated_mean_ms=gm.value)

    def debug_set_wait_bound(self, ticks=0):
        """Test hook: bound of the device-side waits in 100 MHz ticks (0: the default, 4 s)."""
        self._chk(lib.spk_debug_set_wait_bound(self.h, ticks))

    def set_block(self, which, A):
        nrows = A.nrows
        self._chk(lib.spk_set_block(self.h, which, A.row_begin if which == BLOCK_A00 else 0, nrows,
                                    A.ncols, A.rowptr, A.colidx, A.val))

    @staticmethod
    def _kappa(kappa, *grid):
        """(pointer, mem, keep-alive) of a coefficient on the 2-D or 3-D grid: None, a device vector of vec_create, or a
        host array."""
        from .assembly import element_kappa, element_kappa3d
        if kappa is None:
            return None, MEM_HOST, None
        if isinstance(kappa, C.c_void_p):
            return kappa, MEM_DEVICE, kappa
        k = (element_kappa if len(grid) == 2 else element_kappa3d)(*grid, kappa)
        return k.ctypes.data, MEM_HOST, k

    def _set_block_laplace(self, fn, grid, dof, kappa, apply_bc, rhs):
        """set_block_laplace / set_block_laplace3d: fn is the library's entry point for the grid (2 or 3 sides)"""
        kp, mem, _keep = self._kappa(kappa, *grid)
        if rhs is not True:
            self._chk(fn(self.h, *grid, kp, mem, int(apply_bc), rhs))
            return None
        n = dof * math.prod(grid)
        fd = self.vec_create(n=n if min(grid) >= 2 and n < 2 ** 31 else 1)
        try:
            self._chk(fn(self.h, *grid, kp, mem, int(apply_bc), fd))
            return self.vec_get(fd, self.sizes()["n_local"])
        finally:
            self.vec_destroy(fd)

    def _assemble_laplace_csr(self, fn, slab_nnz, grid, dof, units, row_begin, row_end, kappa, apply_bc):
        """assemble_laplace_csr / assemble_laplace3d_csr: fn and slab_nnz are the library's entry points for the grid"""
        from .csr import CSR
        n = dof * math.prod(grid)
        row_end = n if row_end is None else row_end
        nnz = slab_nnz(*grid, row_begin, row_end)
        if nnz < 0:
            raise SpkError(-1, f"row range must consist of whole node {units}")
        kp, mem, _keep = self._kappa(kappa, *grid)
        nl = row_end - row_begin
        rowptr, colidx, val, f = np.zeros(nl + 1, np.int32), np.zeros(nnz, np.int32), np.zeros(nnz), np.zeros(nl)
        self._chk(fn(self.h, *grid, row_begin, row_end, kp, mem, int(apply_bc), rowptr, colidx, val, f.ctypes.data))
        return CSR(rowptr, colidx, val, n, row_begin), f

    def set_block_laplace(self, mx, my=None, kappa=None, apply_bc=True, rhs=None):
        """KSPSetOperators for A00 of the reference's own discretisation, assembled on the device (spk_set_block_laplace):
        what AssembleOperator_Laplace(..., kappa=kappa) + set_block(BLOCK_A00, A) do for this rank's slab, without the host
        arrays.  kappa: None, one host value per element ((mx-1)*(my-1)), or a device vector of vec_create holding them.
        rhs: a device vector of vec_create (n_local values) that receives f, or True to get f back as a numpy array."""
        my = mx if my is None else my
        return self._set_block_laplace(lib.spk_set_block_laplace, (mx, my), 2, kappa, apply_bc, rhs)

    def assemble_laplace_csr(self, mx, my=None, row_begin=0, row_end=None, kappa=None, apply_bc=True):
        """Test hook: (CSR, f) of rows [row_begin,row_end) from the device assembly kernels (spk_assemble_laplace_csr);
        touches nothing of the context's operator."""
        my = mx if my is None else my
        return self._assemble_laplace_csr(lib.spk_assemble_laplace_csr, lib.SpkAssemblySlabNnz, (mx, my), 2, "lines", row_begin, row_end,
                                          kappa, apply_bc)

    def set_block_laplace3d(self, mx, my=None, mz=None, kappa=None, apply_bc=True, rhs=None):
        """set_block_laplace for the 3-D generator (spk_set_block_laplace3d): what AssembleOperator_Laplace3D(...,
        kappa=kappa) + set_block(BLOCK_A00, A) do for this rank's z-slab, without the host arrays.  kappa: None, one host
        value per hexahedron ((mx-1)*(my-1)*(mz-1)), or a device vector of vec_create holding them.  rhs: a device vector
        of vec_create (n_local values) that receives f, or True to get f back as a numpy array."""
        my = mx if my is None else my
        mz = mx if mz is None else mz
        return self._set_block_laplace(lib.spk_set_block_laplace3d, (mx, my, mz), 3, kappa, apply_bc, rhs)

    def assemble_laplace3d_csr(self, mx, my=None, mz=None, row_begin=0, row_end=None, kappa=None, apply_bc=True):
        """Test hook: (CSR, f) of the whole node planes [row_begin,row_end) from the 3-D device assembly kernel
        (spk_assemble_laplace3d_csr); touches nothing of the context's operator."""
        my = mx if my is None else my
        mz = mx if mz is None else mz
        return self._assemble_laplace_csr(lib.spk_assemble_laplace3d_csr, lib.SpkAssemblySlabNnz3D, (mx, my, mz), 3, "planes", row_begin,
                                          row_end, kappa, apply_bc)

    def set_block_constraints(self, mx, my=None, mz=0, rhs=None):
        """KSPSetOperators for A10 of the reference's own discretisation, written on the device (spk_set_block_constraints):
        what AssembleOperator_Constraints[3D] + set_block(BLOCK_A10, B) do for this rank's column slice, without the host
        arrays.  mz = 0: the 2-D block (4 rows), else the 3-D block (6 rows).  rhs: a device vector of vec_create (m values)
        that receives g, or True to get g back as a numpy array."""
        my = mx if my is None else my
        if rhs is not True:
            self._chk(lib.spk_set_block_constraints(self.h, mx, my, mz, rhs))
            return None
        gd = self.vec_create(n=8)
        try:
            self._chk(lib.spk_set_block_constraints(self.h, mx, my, mz, gd))
            return self.vec_get(gd, 6 if mz else 4)
        finally:
            self.vec_destroy(gd)

    def assemble_constraints_csr(self, mx, my=None, mz=0, row_begin=0, row_end=None):
        """Test hook (spk_assemble_constraints_csr): the arrays the constraint kernels write for the columns
        [row_begin,row_end) -- whole node lines, or planes with mz -- as a dict: b_colidx, b_val (B by rows, localised
        columns), bt_rowptr, bt_colidx, bt_val (B^T by rows), win, nwin, winptr ((nwin + 1) x m).  Touches nothing of the
        context's operator."""
        return constraints_csr(mx, my, mz, row_begin, row_end, ctx=self)

    def constraints_seconds(self):
        """Wall seconds of the kernels of the last set_block_constraints, up to a device synchronise (0 before one)."""
        v = C.c_double()
        self._chk(lib.spk_get_constraints_seconds(self.h, C.byref(v)))
        return v.value

    def assembly_seconds(self):
        """Wall seconds of the kernels of the last set_block_laplace, up to a device synchronise (0 before one)."""
        v = C.c_double()
        self._chk(lib.spk_get_assembly_seconds(self.h, C.byref(v)))
        return v.value

    def pc_setup(self, pc_type, schur_fact=SCHUR_FULL, inner_sweeps=0, inner_omega=1.0, amg=None, schur_pre="selfp",
                 amg_reuse=False):
        """inner_sweeps > 0: FP32 damped-Jacobi Richardson sweeps stand for diag(A)^-1.
        amg: None (off), True (defaults) or a dict of spk_amg_opts fields: one smoothed-aggregation V-cycle stands
        for A^-1 (PC_JACOBI: M^-1 on K = A; PC_SCHUR: inside the fieldsplit).
        schur_pre: "selfp" (S^ = diag(B diag(A)^-1 B^T)) or "full" (the exact S = B A^ ^-1 B^T of at most 8 rows, dense
        and Cholesky-factored; PC_SCHUR only).
        amg_reuse: a set-up that finds the hierarchy of an earlier amg_reuse=True set-up, the same options and an A00
        of the same pattern refreshes its values and keeps the prolongators (spk_pc_set_amg_reuse; amg_reuse_info())."""
        if schur_pre not in _SCHUR_PRES:
            raise ValueError(f"schur_pre must be one of {sorted(_SCHUR_PRES)}")
        self._chk(lib.spk_pc_set_schur_pre(self.h, _SCHUR_PRES[schur_pre]))
        self._chk(lib.spk_pc_set_amg_reuse(self.h, 1 if amg_reuse else 0))
        if amg is None or amg is False:
            self._chk(lib.spk_pc_set_amg(self.h, None))
            self._chk(lib.spk_pc_set_inner(self.h, inner_sweeps, inner_omega))
        else:
            self._chk(lib.spk_pc_set_inner(self.h, inner_sweeps, inner_omega))
            o = amg_opts(**({} if amg is True else dict(amg)))
            self._chk(lib.spk_pc_set_amg(self.h, C.byref(o)))
        self._chk(lib.spk_pc_setup(self.h, pc_type, schur_fact))

    def amg_info(self):
        """levels, rows / nnz / lambda_max per level, operator complexity, set-up seconds of the multigrid hierarchy."""
        ai = AmgInfo()
        self._chk(lib.spk_get_amg_info(self.h, C.byref(ai)))
        return _amg_info(ai)

    def amg_reuse_info(self):
        """Whether the last pc_setup refreshed the hierarchy (True) or built it, and the wall seconds of that."""
        r, t = C.c_int32(), C.c_double()
        self._chk(lib.spk_get_amg_reuse_info(self.h, C.byref(r), C.byref(t)))
        return dict(refreshed=bool(r.value), seconds=t.value)

    def debug_amg_transfer(self, level, which, a, b, stored=False, precision="double"):
        """Test hook (spk_debug_amg_transfer): one transfer of a level alone.  which 'prolong': b + P a (a: coarse, b: fine);
        'restrict': R (a - b) (both fine).  The fine vectors may be longer than the level (a padded vector).
        precision 'single' (spk_debug_amg_transfer_f32, a hierarchy built with it): the matrix-free FP32 kernels -- float32
        vectors on a level >= 1; on level 0 'restrict' takes float64 and gives float32, 'prolong' takes a float32 a and a
        float64 b and gives float64."""
        if precision == "single":
            pro = which == "prolong"
            ta = np.float32 if level > 0 or pro else np.float64
            tb = np.float32 if level > 0 else np.float64
            to = np.float32 if level > 0 or not pro else np.float64
            a, b = np.ascontiguousarray(a, ta), np.ascontiguousarray(b, tb)
            out = np.zeros(b.size if pro else self.amg_info()["rows"][level + 1], to)
            self._chk(lib.spk_debug_amg_transfer_f32(self.h, level, 0 if pro else 1, b.size, a.ctypes.data, b.ctypes.data,
                                                     out.ctypes.data))
            return out
        a = np.ascontiguousarray(a, np.float64)
        b = np.ascontiguousarray(b, np.float64)
        info = self.amg_info()
        pro = which == "prolong"
        out = np.zeros(b.size if pro else info["rows"][level + 1])
        self._chk(lib.spk_debug_amg_transfer(self.h, level, 0 if pro else 1, 1 if stored else 0, b.size, a, b, out))
        return out

    def debug_amg_operator(self, level, which, x, b=None, xo=None, alpha=0.0, beta=0.0, stencil=True, done=False, out=None,
                           precision="double"):
        """Test hook (spk_debug_amg_operator): the operator of a level between level 0 and the coarsest alone, one launch.
        which 'product': A x; 'step': x + alpha D^-1 (b - A x) + beta (x - xo) (xo None: the zero vector).  stencil: the
        value-array kernels, else the CSR kernels.  done: the launch finds the `done` gate set, and `out` (given, or
        zeros) comes back as it went in.  precision 'single' (spk_debug_amg_operator_f32, a hierarchy built with it): the
        FP32 value-array kernel on float32 vectors; alpha and beta are rounded to float32."""
        rows = self.amg_info()["rows"]
        if not 0 <= level < len(rows):
            raise SpkError(SPK_ERR_ARG, f"level {level} outside the hierarchy")
        n = rows[level]
        step = which == "step"
        dt = np.float32 if precision == "single" else np.float64
        vec = lambda v: None if v is None else np.ascontiguousarray(v, dt)
        x, b, xo = vec(x), vec(b), vec(xo)
        for v in (x, b, xo):
            if v is not None and v.size != n:
                raise SpkError(SPK_ERR_ARG, f"a vector of {v.size} entries for the {n} rows of level {level}")
        out = np.zeros(n, dt) if out is None else np.array(out, dt)
        ptr = lambda v: None if v is None else v.ctypes.data
        if precision == "single":
            self._chk(lib.spk_debug_amg_operator_f32(self.h, level, (1 if step else 0) + (2 if done else 0), float(alpha), float(beta),
                                                     ptr(x), ptr(xo), ptr(b), ptr(out)))
            return out
        self._chk(lib.spk_debug_amg_operator(self.h, level, (1 if step else 0) + (2 if done else 0), 1 if stencil else 0,
                                             float(alpha), float(beta), x, ptr(xo), ptr(b), out))
        return out

    def debug_amg_lanczos(self, level, resident=False):
        """Test hook (spk_debug_amg_lanczos): the device set-up's Lanczos alone on a level below the coarsest of the
        device-built hierarchy, by the stepwise or the resident route.  Returns (steps, al[:steps], be[:steps]): the
        tridiagonal whose extreme eigenvalues are the level's Ritz values (be[0] = 0)."""
        steps = C.c_int32()
        al, be = np.zeros(30), np.zeros(31)
        self._chk(lib.spk_debug_amg_lanczos(self.h, int(level), 1 if resident else 0, C.byref(steps), al, be))
        return steps.value, al[:steps.value].copy(), be[:steps.value].copy()

    def amg_aggregates(self, level):
        """The aggregate of every node of a level of the context's hierarchy (-1: isolated)."""
        n = C.c_int32()
        self._chk(lib.spk_get_amg_aggregates(self.h, level, C.byref(n), None))
        agg = np.zeros(n.value, np.int32)
        self._chk(lib.spk_get_amg_aggregates(self.h, level, C.byref(n), agg.ctypes.data))
        return agg

    def amg_level(self, level, which=AMG_OP):
        """(rowptr, colidx, val, shape) of A_l (AMG_OP), P_l (AMG_PROLONG), the tentative P_l or the coarse inverse."""
        return _amg_matrix(lambda *a: self._chk(lib.spk_get_amg_level(self.h, *a)), level, which)

    def sizes(self):
        ng, nl, m, nnz, gh = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
        lib.spk_get_sizes(self.h, C.byref(ng), C.byref(nl), C.byref(m), C.byref(nnz), C.byref(gh))
        return dict(n_global=ng.value, n_local=nl.value, m=m.value, nnz_local=nnz.value, n_ghost=gh.value)

    def spmv_info(self):
        fmt, b = C.c_int32(), C.c_int64()
        lib.spk_get_spmv_info(self.h, C.byref(fmt), C.byref(b))
        return dict(format={0: "csr", 1: "bcsr2x2", 2: "bcsr3x3", 3: "dict2x2", 4: "dict3x3"}[fmt.value], layout_bytes=b.value)

    def dict_layout(self):
        """The row-type layout of the A block as set up (spk_debug_dict_layout); ok = 0: the blocked / CSR kernels run."""
        out = (C.c_int32 * 12)()
        self._chk(lib.spk_debug_dict_layout(self.h, out))
        names = ("ok", "bs", "nbrows", "kmax", "ntype", "nclass", "lds_bytes", "uniform", "straddle", "uniform3", "product_kernel",
                 "chunks_per_wg")
        return dict(zip(names, (int(v) for v in out)))

    def iteration_form(self):
        """(form, single_reduce) of the last fgmres on this context: the SPK_ITER_* actually run, -1 = step-by-step path."""
        f, sr = C.c_int32(), C.c_int32()
        self._chk(lib.spk_get_iteration_form(self.h, C.byref(f), C.byref(sr)))
        return f.value, sr.value

    def gs_launch(self):
        """(launches, tail) of the last fgmres on this context: form 7's launches, and those of them that staged a short
        remainder tile in LDS (SPK_GS_TAIL; all or none)."""
        n, t = C.c_int32(), C.c_int32()
        self._chk(lib.spk_get_gs_launch(self.h, C.byref(n), C.byref(t)))
        return n.value, t.value

    def basis_info(self):
        """(precision, basis_bytes) of the last fgmres on this context: "double" / "single" (None before the first solve)
        and the bytes allocated for the basis V."""
        p, nb = C.c_int32(), C.c_int64()
        self._chk(lib.spk_get_basis_info(self.h, C.byref(p), C.byref(nb)))
        return {BASIS_DOUBLE: "double", BASIS_SINGLE: "single"}.get(p.value), nb.value

    def spmv_models(self):
        """Bytes of one product y = A x in the CSR, blocked and row-pattern-dictionary layouts (0: layout absent)."""
        a, b, d, p, q = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        self._chk(lib.spk_get_spmv_models(self.h, C.byref(a), C.byref(b), C.byref(d), C.byref(p), C.byref(q)))
        return dict(csr_bytes=a.value, blocked_bytes=b.value, dict_bytes=d.value, patterns=p.value, blocks=q.value)

    def _n(self):
        s = self.sizes()
        return s["n_local"] + s["m"]

    def schur_diag(self):
        out = np.zeros(self.sizes()["m"])
        self._chk(lib.spk_get_schur_diag(self.h, out))
        return out

    def schur_matrix(self):
        """The dense S = B A^ ^-1 B^T (m x m) the last pc_setup(..., schur_pre="full") factored."""
        m = self.sizes()["m"]
        out = np.zeros(m * m)
        self._chk(lib.spk_get_schur_matrix(self.h, out))
        return out.reshape(m, m)

    def schur_setup_seconds(self):
        v = C.c_double()
        self._chk(lib.spk_get_schur_setup_seconds(self.h, C.byref(v)))
        return v.value

    def bd_planes(self):
        v = C.c_int32()
        self._chk(lib.spk_get_bd_planes(self.h, C.byref(v)))
        return v.value

    def constraint_layout(self):
        """Which path the rows of A10 take on this rank (spk_get_constraint_layout; reads the context, launches nothing):
        general (more than 8 rows: stream kernel + window kernel), m_wide and wide_rows (the rows the window kernel takes,
        ascending), win / nwin (the column windows), bc_tiles / bt_tiles (stream-kernel workgroups over B by rows / B^T)."""
        g, mw, win, nwin, bc, bt = (C.c_int32() for _ in range(6))
        rows = (C.c_int32 * 8)()
        self._chk(lib.spk_get_constraint_layout(self.h, C.byref(g), C.byref(mw), rows, C.byref(win), C.byref(nwin), C.byref(bc),
                                                C.byref(bt)))
        return dict(general=bool(g.value), m_wide=mw.value, wide_rows=[int(r) for r in rows[:mw.value]], win=win.value,
                    nwin=nwin.value, bc_tiles=bc.value, bt_tiles=bt.value)

    def jacobi_diag(self):
        out = np.zeros(self.sizes()["n_local"])
        self._chk(lib.spk_get_jacobi_diag(self.h, out))
        return out

    def mult(self, x):
        x = np.ascontiguousarray(x, np.float64)
        assert x.shape == (self._n(),)
        y = np.zeros_like(x)
        self._chk(lib.spk_mult(self.h, x, y, MEM_HOST))
        return y

    def pc_apply(self, x):
        x = np.ascontiguousarray(x, np.float64)
        assert x.shape == (self._n(),)
        y = np.zeros_like(x)
        self._chk(lib.spk_pc_apply(self.h, x, y, MEM_HOST))
        return y

    def fgmres(self, b, x0=None, **kw):
        b = np.ascontiguousarray(b, np.float64)
        assert b.shape == (self._n(),)
        o = default_opts(**kw)
        x = np.zeros_like(b)
        if x0 is not None:
            x[:] = x0
            o.guess_nonzero = 1
        res = Result()
        cap = int(min(o.max_it + 2, 1 << 22))
        hist = np.zeros(cap)
        self._chk(lib.spk_fgmres(self.h, b, x, MEM_HOST, C.byref(o), C.byref(res), hist.ctypes.data, cap))
        return x, dict(its=res.its, reason=res.reason, rnorm=res.rnorm, rnorm0=res.rnorm0,
                       cycles=res.cycles, solve_seconds=res.solve_seconds,
                       history=hist[:res.hist_len].copy())

    def minres(self, b, x0=None, norm="unpreconditioned", **kw):
        """Preconditioned MINRES (spk_minres) with the context's PC (none, Jacobi or Schur DIAG); norm: the norm of the
        convergence test, "unpreconditioned" (||b - K x||) or "natural" (||b - K x|| in M^-1).  Same return as fgmres."""
        b = np.ascontiguousarray(b, np.float64)
        assert b.shape == (self._n(),)
        x = np.zeros_like(b)
        if x0 is not None:
            x[:] = x0
            kw["guess_nonzero"] = 1
        return x, self._short_recurrence(lib.spk_minres, b.ctypes.data, x.ctypes.data, MEM_HOST, norm, kw)

    def minres_device(self, b_dev, x_dev, norm="unpreconditioned", **kw):
        """MINRES on vectors that already live in device memory (vec_create)."""
        return self._short_recurrence(lib.spk_minres, b_dev, x_dev, MEM_DEVICE, norm, kw)

    def _short_recurrence(self, fn, bp, xp, mem, norm, kw, extra=()):
        """One solve of spk_minres, spk_pipecg or spk_pipecgrr (fn; extra: its arguments after the history)."""
        if norm not in _NORMS:
            raise ValueError(f"norm must be one of {sorted(_NORMS)}")
        o = default_opts(**kw)
        res = Result()
        cap = int(min(o.max_it + 2, 1 << 22))
        hist = np.zeros(cap)
        self._chk(fn(self.h, bp, xp, mem, C.byref(o), _NORMS[norm], C.byref(res), hist.ctypes.data, cap, *extra))
        return dict(its=res.its, reason=res.reason, rnorm=res.rnorm, rnorm0=res.rnorm0,
                    cycles=res.cycles, solve_seconds=res.solve_seconds,
                    history=hist[:res.hist_len].copy())

    def pipecg(self, b, x0=None, norm="unpreconditioned", **kw):
        """Preconditioned pipelined CG (spk_pipecg) on K = A with the context's PC (none, Jacobi or the V-cycle); norm:
        "unpreconditioned" (||b - K x||) or "natural" (sqrt(<r, M^-1 r>)).  Same return as fgmres."""
        b = np.ascontiguousarray(b, np.float64)
        assert b.shape == (self._n(),)
        x = np.zeros_like(b)
        if x0 is not None:
            x[:] = x0
            kw["guess_nonzero"] = 1
        return x, self._short_recurrence(lib.spk_pipecg, b.ctypes.data, x.ctypes.data, MEM_HOST, norm, kw)

    def pipecg_device(self, b_dev, x_dev, norm="unpreconditioned", **kw):
        """Pipelined CG on vectors that already live in device memory (vec_create)."""
        return self._short_recurrence(lib.spk_pipecg, b_dev, x_dev, MEM_DEVICE, norm, kw)

    def pipecgrr(self, b, x0=None, norm="unpreconditioned", tau=None, **kw):
        """Pipelined CG with residual replacement (spk_pipecgrr): pipecg plus, every check_every iterations, the gap
        check ||(b - K x) - r|| against tau ||r|| and the replacement of r, u, w, s, q, z it may trigger.  tau: None keeps
        the context's (PIPECGRR_TAU_DEFAULT until set).  Same return as pipecg, plus `replacements`."""
        b = np.ascontiguousarray(b, np.float64)
        assert b.shape == (self._n(),)
        x = np.zeros_like(b)
        if x0 is not None:
            x[:] = x0
            kw["guess_nonzero"] = 1
        return x, self._pipecgrr(b.ctypes.data, x.ctypes.data, MEM_HOST, norm, tau, kw)

    def pipecgrr_device(self, b_dev, x_dev, norm="unpreconditioned", tau=None, **kw):
        """Pipelined CG with residual replacement on vectors that already live in device memory (vec_create)."""
        return self._pipecgrr(b_dev, x_dev, MEM_DEVICE, norm, tau, kw)

    def _pipecgrr(self, bp, xp, mem, norm, tau, kw):
        if tau is not None:
            self._chk(lib.spk_pipecgrr_set_tau(self.h, float(tau)))
        nrep = C.c_int32(0)
        info = self._short_recurrence(lib.spk_pipecgrr, bp, xp, mem, norm, kw, (C.byref(nrep),))
        info["replacements"] = nrep.value
        return info

    # ---- device-resident vectors (inputs already in HBM when a solve starts)
    def vec_create(self, host=None, n=None):
        n = len(host) if host is not None else n
        p = C.c_void_p()
        self._chk(lib.spk_vec_create(self.h, n, C.byref(p)))
        if host is not None:
            self._chk(lib.spk_vec_set(self.h, p, np.ascontiguousarray(host, np.float64), n))
        return p

    def vec_get(self, p, n):
        out = np.zeros(n)
        self._chk(lib.spk_vec_get(self.h, p, out, n))
        return out

    def vec_destroy(self, p):
        self._chk(lib.spk_vec_destroy(self.h, p))

    def fgmres_device(self, b_dev, x_dev, **kw):
        """KSPSolve on vectors that already live in device memory."""
        o = default_opts(**kw)
        res = Result()
        cap = int(min(o.max_it + 2, 1 << 22))
        hist = np.zeros(cap)
        f = lib.spk_fgmres
        old = f.argtypes
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(Opts), C.POINTER(Result), C.c_void_p, C.c_int32]
        try:
            rc = f(self.h, b_dev, x_dev, MEM_DEVICE, C.byref(o), C.byref(res), hist.ctypes.data, cap)
        finally:
            f.argtypes = old
        self._chk(rc)
        return dict(its=res.its, reason=res.reason, rnorm=res.rnorm, rnorm0=res.rnorm0,
                    cycles=res.cycles, solve_seconds=res.solve_seconds,
                    history=hist[:res.hist_len].copy())

    def mdot(self, V, w):
        V = np.ascontiguousarray(V, np.float64)
        w = np.ascontiguousarray(w, np.float64)
        nv, n = V.shape
        h = np.zeros(nv + 1)
        self._chk(lib.spk_kernel_mdot(self.h, n, nv, V.reshape(-1), n, w, h))
        return h[:nv], h[nv]

    def maxpy(self, a, V, w):
        V = np.ascontiguousarray(V, np.float64)
        a = np.ascontiguousarray(a, np.float64)
        w = np.array(w, np.float64)
        nv, n = V.shape
        nrm2 = C.c_double()
        self._chk(lib.spk_kernel_maxpy(self.h, n, nv, a, V.reshape(-1), n, w, C.byref(nrm2)))
        return w, nrm2.value

    def time_spmv(self, warmup=5, reps=50):
        ms = C.c_double()
        self._chk(lib.spk_time_spmv(self.h, warmup, reps, C.byref(ms)))
        return ms.value


def _time_kernel(self, which, nv=0, warmup=5, reps=50):
    ms = C.c_double()
    self._chk(lib.spk_time_kernel(self.h, which.encode(), nv, warmup, reps, C.byref(ms)))
    return ms.value


Context.time_kernel = _time_kernel


def constraints_csr(mx, my=None, mz=0, row_begin=0, row_end=None, ctx=None):
    """The arrays KSPSetOperators keeps of the generator's constraint block over the columns [row_begin,row_end), as a
    dict (Context.assemble_constraints_csr).  ctx None: by the host chain of set_block(BLOCK_A10)
    (spk_host_constraints_csr; no GPU); a Context: by the device kernels."""
    my = mx if my is None else my
    dof = 3 if mz else 2
    n = dof * mx * my * (mz if mz else 1)
    row_end = n if row_end is None else row_end
    nnz = lib.SpkConstraintsSlabNnz3D(mx, my, mz, row_begin, row_end) if mz else lib.SpkConstraintsSlabNnz(mx, my, row_begin, row_end)
    if nnz < 0:
        raise SpkError(-1, f"columns must be whole node {'planes' if mz else 'lines'} of a grid with sides of at least 3")
    nl, m = row_end - row_begin, 2 * dof
    cap = (nl // 1024 + 2) * m   # (windows are at least 1024 columns wide)
    out = dict(b_colidx=np.zeros(nnz, np.int32), b_val=np.zeros(nnz), bt_rowptr=np.zeros(nl + 1, np.int32),
               bt_colidx=np.zeros(nnz, np.int32), bt_val=np.zeros(nnz))
    win, nwin, winptr = C.c_int32(), C.c_int32(), np.zeros(cap, np.int32)
    args = (mx, my, mz, row_begin, row_end, out["b_colidx"], out["b_val"], out["bt_rowptr"], out["bt_colidx"], out["bt_val"],
            C.byref(win), C.byref(nwin), winptr, cap)
    if ctx is None:
        rc = lib.spk_host_constraints_csr(*args)
        if rc != 0:
            raise SpkError(rc, "spk_host_constraints_csr")
    else:
        ctx._chk(lib.spk_assemble_constraints_csr(ctx.h, *args))
    out.update(win=win.value, nwin=nwin.value, winptr=winptr[:(nwin.value + 1) * m].reshape(nwin.value + 1, m).copy())
    return out


def _mat(A):
    m = MatCSR()
    m.row_begin, m.nrows_local, m.ncols_global = A.row_begin, A.nrows, A.ncols
    m.rowptr, m.colidx, m.val = A.rowptr.ctypes.data, A.colidx.ctypes.data, A.val.ctypes.data
    return m


class KSP:
    """Mirror of the reference's solver object: create / setOperators /
    setFromOptions / setUp / solve / destroy (SaddlePointProblem.c:65-72)."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        rc = lib.SpkKSPCreate(device, C.byref(self.h))
        if rc != 0:
            msg = lib.SpkKSPGetError(self.h).decode() if self.h else "SpkKSPCreate failed"
            lib.SpkKSPDestroy(C.byref(self.h))
            raise SpkError(rc, msg)
        self._keep = None

    def _chk(self, rc):
        if rc != 0:
            raise SpkError(rc, lib.SpkKSPGetError(self.h).decode())

    def setCommRCCL(self, rank, nranks, id128):
        self._chk(lib.SpkKSPSetCommRCCL(self.h, rank, nranks, id128))

    def setOperators(self, A, B=None):
        a = _mat(A)
        b = _mat(B) if B is not None else None
        self._chk(lib.SpkKSPSetOperators(self.h, C.byref(a), C.byref(b) if b is not None else None))
        self._n = A.nrows + (B.nrows if B is not None else 0)

    def setOperatorsLaplace(self, mx, my=None, kappa=None, B=None, with_rhs=True):
        """setOperators with A of the reference's own discretisation assembled on the device (SpkKSPSetOperatorsLaplace);
        kappa: None or one host value per element.  Returns f (numpy) when with_rhs.  B="device": the generator's
        constraint block written on the device as well (SpkKSPSetOperatorsLaplaceConstrained); returns f followed by g."""
        from .assembly import element_kappa
        my = mx if my is None else my
        k = element_kappa(mx, my, kappa)
        if isinstance(B, str):
            return self._set_operators_constrained(lib.SpkKSPSetOperatorsLaplaceConstrained, (mx, my), 2, k, B, with_rhs)
        b = _mat(B) if B is not None else None
        f = np.zeros(2 * mx * my if 2 <= mx and 2 <= my and 2 * mx * my < 2 ** 31 else 1) if with_rhs else None
        self._chk(lib.SpkKSPSetOperatorsLaplace(self.h, mx, my, k.ctypes.data if k is not None else None,
                                                C.byref(b) if b is not None else None, f.ctypes.data if with_rhs else None))
        ctx, nl = C.c_void_p(), C.c_int32()
        lib.SpkKSPGetContext(self.h, C.byref(ctx))
        lib.spk_get_sizes(ctx, None, C.byref(nl), None, None, None)
        self._n = nl.value + (B.nrows if B is not None else 0)
        return f[:nl.value] if with_rhs else None

    def setOperatorsLaplace3D(self, mx, my=None, mz=None, kappa=None, B=None, with_rhs=True):
        """setOperatorsLaplace for the 3-D generator (SpkKSPSetOperatorsLaplace3D); kappa: None or one host value per
        hexahedron.  Returns f (numpy) when with_rhs.  B="device": as in setOperatorsLaplace, the six rows of the 3-D block."""
        from .assembly import element_kappa3d
        my = mx if my is None else my
        mz = mx if mz is None else mz
        k = element_kappa3d(mx, my, mz, kappa)
        if isinstance(B, str):
            return self._set_operators_constrained(lib.SpkKSPSetOperatorsLaplaceConstrained3D, (mx, my, mz), 3, k, B, with_rhs)
        b = _mat(B) if B is not None else None
        n = 3 * mx * my * mz
        f = np.zeros(n if min(mx, my, mz) >= 2 and n < 2 ** 31 else 1) if with_rhs else None
        self._chk(lib.SpkKSPSetOperatorsLaplace3D(self.h, mx, my, mz, k.ctypes.data if k is not None else None,
                                                  C.byref(b) if b is not None else None, f.ctypes.data if with_rhs else None))
        ctx, nl = C.c_void_p(), C.c_int32()
        lib.SpkKSPGetContext(self.h, C.byref(ctx))
        lib.spk_get_sizes(ctx, None, C.byref(nl), None, None, None)
        self._n = nl.value + (B.nrows if B is not None else 0)
        return f[:nl.value] if with_rhs else None

    def _set_operators_constrained(self, fn, grid, dof, k, B, with_rhs):
        """setOperatorsLaplace / ...3D with B="device": fn is the facade's entry point for the grid"""
        if B != "device":
            raise ValueError(f'B = {B!r}: a CSR block, None or "device"')
        n, m = dof * math.prod(grid), 2 * dof
        rhs = np.zeros((n if min(grid) >= 2 and n < 2 ** 31 else 1) + m) if with_rhs else None
        self._chk(fn(self.h, *grid, k.ctypes.data if k is not None else None, rhs.ctypes.data if with_rhs else None))
        ctx, nl = C.c_void_p(), C.c_int32()
        lib.SpkKSPGetContext(self.h, C.byref(ctx))
        lib.spk_get_sizes(ctx, None, C.byref(nl), None, None, None)
        self._n = nl.value + m
        return rhs[:nl.value + m] if with_rhs else None

    def setGrid(self, mx, my, mz=1):
        """The node grid behind the operator of setOperators (SpkKSPSetGrid; the role of KSPSetDM): what -pc_type mg
        coarsens.  setOperatorsLaplace / setOperatorsLaplace3D set it themselves."""
        self._chk(lib.SpkKSPSetGrid(self.h, mx, my, mz))

    def setFromOptions(self, options):
        """options: PETSc-style string or list, e.g. '-ksp_type fgmres -ksp_rtol 1e-8'."""
        args = options.split() if isinstance(options, str) else list(options)
        arr = (C.c_char_p * max(len(args), 1))(*[a.encode() for a in args])
        self._chk(lib.SpkKSPSetFromOptions(self.h, len(args), arr))

    def setUp(self):
        self._chk(lib.SpkKSPSetUp(self.h))

    def solve(self, b, x=None):
        b = np.ascontiguousarray(b, np.float64)
        assert b.shape == (self._n,)
        x = np.zeros_like(b) if x is None else x
        self._chk(lib.SpkKSPSolve(self.h, b, x))
        return x

    def getIterationNumber(self):
        v = C.c_int32()
        lib.SpkKSPGetIterationNumber(self.h, C.byref(v))
        return v.value

    def getConvergedReason(self):
        v = C.c_int32()
        lib.SpkKSPGetConvergedReason(self.h, C.byref(v))
        return v.value

    def getResidualNorm(self):
        v = C.c_double()
        lib.SpkKSPGetResidualNorm(self.h, C.byref(v))
        return v.value

    def getSolveTime(self):
        v = C.c_double()
        lib.SpkKSPGetSolveTime(self.h, C.byref(v))
        return v.value

    def getConvergenceHistory(self):
        p, n = C.POINTER(C.c_double)(), C.c_int32()
        lib.SpkKSPGetResidualHistory(self.h, C.byref(p), C.byref(n))
        return np.array([p[i] for i in range(n.value)])

    def getOptions(self):
        o, pc, sf = Opts(), C.c_int32(), C.c_int32()
        lib.SpkKSPGetOptions(self.h, C.byref(o), C.byref(pc), C.byref(sf))
        return o, pc.value, sf.value

    def getAMGOptions(self, fieldsplit0=False):
        """(options dict, selected) of the plain (-pc_type gamg) or the -fieldsplit_0_ multigrid option set."""
        o, sel = AmgOpts(), C.c_int32()
        self._chk(lib.SpkKSPGetAMGOptions(self.h, 1 if fieldsplit0 else 0, C.byref(o), C.byref(sel)))
        return amg_opts_dict(o), bool(sel.value)

    def getAMGReuse(self, fieldsplit0=False):
        """-pc_gamg_reuse_interpolation (or its -fieldsplit_0_ form) as read."""
        v = C.c_int32()
        self._chk(lib.SpkKSPGetAMGReuse(self.h, 1 if fieldsplit0 else 0, C.byref(v)))
        return bool(v.value)

    def getSchurPre(self):
        """(-pc_fieldsplit_schur_precondition, -fieldsplit_1_pc_type) as they resolve: ('selfp' | 'full', 'jacobi' | 'cholesky')."""
        p, d = C.c_int32(), C.c_int32()
        self._chk(lib.SpkKSPGetSchurPre(self.h, C.byref(p), C.byref(d)))
        return {v: k for k, v in _SCHUR_PRES.items()}[p.value], "cholesky" if d.value else "jacobi"

    def getType(self):
        """-ksp_type as set: 'fgmres', 'minres', 'pipecg', 'pipecgrr', or '' before setFromOptions gave one."""
        t, n = C.c_char_p(), C.c_int32()
        self._chk(lib.SpkKSPGetType(self.h, C.byref(t), C.byref(n)))
        return t.value.decode()

    def getNormType(self):
        """-ksp_norm_type as set: 'unpreconditioned' or 'natural'."""
        t, n = C.c_char_p(), C.c_int32()
        self._chk(lib.SpkKSPGetType(self.h, C.byref(t), C.byref(n)))
        return {v: k for k, v in _NORMS.items()}[n.value]

    def destroy(self):
        if self.h:
            lib.SpkKSPDestroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.destroy()
