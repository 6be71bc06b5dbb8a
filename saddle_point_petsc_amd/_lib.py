"""ctypes binding of libspk.so (include/spk.h, spk_ksp.h, spk_assembly.h).

The library is built in-tree by `make -C saddle_point_petsc_amd/csrc` (or
`__graft_entry__.build()`).  There is NO fallback: if libspk.so is missing the
import fails, and without a GPU `spk_create` fails -- nothing here computes on
the CPU.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libspk.so")

i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")


class SpkError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libspk error {code}: {msg}")
        self.code = code


class Opts(C.Structure):
    _fields_ = [
        ("restart", C.c_int32), ("max_it", C.c_int32), ("rtol", C.c_double),
        ("abstol", C.c_double), ("dtol", C.c_double), ("guess_nonzero", C.c_int32),
        ("orthog", C.c_int32), ("check_every", C.c_int32), ("fused", C.c_int32),
        ("cgs_refine", C.c_int32), ("single_reduce", C.c_int32), ("iteration_form", C.c_int32),
        ("basis_precision", C.c_int32),
    ]


class Result(C.Structure):
    _fields_ = [
        ("its", C.c_int32), ("reason", C.c_int32), ("rnorm", C.c_double),
        ("rnorm0", C.c_double), ("hist_len", C.c_int32), ("cycles", C.c_int32),
        ("solve_seconds", C.c_double),
    ]


ALLREDUCE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int)
EXCHANGE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_double), C.c_int64)
ALLGATHER_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)


class HostComm(C.Structure):
    _fields_ = [("user", C.c_void_p), ("allreduce", ALLREDUCE_CB), ("exchange", EXCHANGE_CB),
                ("allgather", ALLGATHER_CB)]


class CommInfo(C.Structure):
    """spk_comm_info (include/spk.h)."""
    _fields_ = [
        ("rank", C.c_int32), ("nranks", C.c_int32), ("peer_enabled", C.c_int32), ("window_tier", C.c_int32),
        ("self_test_ok", C.c_int32), ("halo_mode", C.c_int32), ("halo_fused", C.c_int32), ("device", C.c_int32),
        ("n_allreduce_fused", C.c_int64), ("n_allreduce_kernel", C.c_int64), ("n_allreduce_inner", C.c_int64),
        ("n_halo_fused", C.c_int64), ("n_halo_kernel", C.c_int64), ("n_halo_inner", C.c_int64),
        ("wait_ticks", C.c_uint64 * 4), ("wait_count", C.c_uint64 * 4),
        ("backend", C.c_char * 32), ("inner_backend", C.c_char * 32), ("why", C.c_char * 256),
    ]


AMG_MAX_LEVELS = 16


class AmgOpts(C.Structure):
    """spk_amg_opts (include/spk.h)."""
    _fields_ = [
        ("max_levels", C.c_int32), ("coarse_eq_limit", C.c_int32), ("nsmooths", C.c_int32), ("smoother", C.c_int32),
        ("threshold", C.c_double), ("smooth_its", C.c_int32), ("block_size", C.c_int32), ("esteig", C.c_double * 4),
        ("richardson_scale", C.c_double), ("setup", C.c_int32),
        ("coarsening", C.c_int32), ("grid", C.c_int32 * 3), ("transfer", C.c_int32), ("sides", C.c_int32),
        ("cycle", C.c_int32), ("tail", C.c_int32), ("tail_rows", C.c_int32), ("galerkin", C.c_int32),
        ("op", C.c_int32), ("lanczos", C.c_int32), ("precision", C.c_int32),
    ]


class AmgInfo(C.Structure):
    """spk_amg_info (include/spk.h)."""
    _fields_ = [
        ("levels", C.c_int32), ("block_size", C.c_int32), ("rows", C.c_int32 * AMG_MAX_LEVELS),
        ("nnz", C.c_int64 * AMG_MAX_LEVELS), ("lambda_max", C.c_double * AMG_MAX_LEVELS),
        ("operator_complexity", C.c_double), ("setup_seconds", C.c_double), ("setup", C.c_int32),
        ("coarsening", C.c_int32), ("dims", (C.c_int32 * 3) * AMG_MAX_LEVELS), ("sides", C.c_int32),
        ("cycle", C.c_int32), ("tail_first", C.c_int32), ("tail_launches", C.c_int32), ("galerkin", C.c_int32),
        ("op", C.c_int32), ("lanczos", C.c_int32), ("ritz_readbacks", C.c_int32),
        ("precision", C.c_int32),
    ]


class MatCSR(C.Structure):
    _fields_ = [
        ("row_begin", C.c_int64), ("nrows_local", C.c_int32), ("pad", C.c_int32),
        ("ncols_global", C.c_int64), ("rowptr", C.c_void_p), ("colidx", C.c_void_p),
        ("val", C.c_void_p),
    ]


class DebugMdotOpts(C.Structure):
    """spk_debug_mdot_opts (include/spk.h)."""
    _fields_ = [("n", C.c_int64), ("n_dot", C.c_int64), ("nv", C.c_int32), ("nv2", C.c_int32), ("split", C.c_int32),
                ("done", C.c_int32), ("pad", C.c_double)]


class DebugMaxpyOpts(C.Structure):
    """spk_debug_maxpy_opts (include/spk.h)."""
    _fields_ = [("n", C.c_int64), ("n_dot", C.c_int64), ("n_bd", C.c_int64), ("sign", C.c_double), ("pad", C.c_double),
                ("nv", C.c_int32), ("nv_live", C.c_int32), ("want_norm", C.c_int32), ("m", C.c_int32), ("bd_mode", C.c_int32),
                ("w1side", C.c_int32), ("pyth", C.c_int32), ("done", C.c_int32)]


class DebugHeadOpts(C.Structure):
    """spk_debug_head_opts (include/spk.h)."""
    _fields_ = [("nl", C.c_int64), ("m", C.c_int32), ("packed", C.c_int32), ("fact", C.c_int32), ("jacobi", C.c_int32),
                ("want_wl", C.c_int32), ("reserved", C.c_int32), ("pad", C.c_double)]


def hip_runtimes_mapped():
    """Paths of every libamdhip64 mapped into this process (two = two HIP runtimes: the second finds no device)."""
    try:
        with open("/proc/self/maps") as fh:
            return sorted({ln.split()[-1] for ln in fh if "libamdhip64" in ln})
    except OSError:
        return []


def _preload_hip_runtime():
    """ONE HIP runtime per process whatever the import order.  The torch wheel carries a private libamdhip64.so (SONAME
    libamdhip64.so.7, the name libspk.so needs).  Loaded first, it satisfies libspk's dependency by soname; loaded SECOND --
    `import saddle_point_petsc_amd` before `import torch` -- the process used to map two runtimes, and the second one found
    no device ("no ROCm-capable device").  So where torch is installed its copy is mapped here, before libspk.so, without
    importing torch; a later `import torch` finds it already loaded.  SPK_HIP_RUNTIME=system keeps /opt/rocm's."""
    if os.environ.get("SPK_HIP_RUNTIME") == "system":
        return None
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return None
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if not os.path.exists(path):
        return None
    try:
        return C.CDLL(path, mode=C.RTLD_GLOBAL)
    except OSError:
        return None


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
            "(hipcc, gfx950).  saddle_point_petsc_amd has no CPU fallback.")
    global _hip_preloaded
    _hip_preloaded = _preload_hip_runtime()
    L = C.CDLL(LIB_PATH)
    rts = hip_runtimes_mapped()
    if len(rts) > 1:
        raise ImportError("two HIP runtimes are mapped into this process (" + ", ".join(rts) + "): libspk.so would not find the "
                          "GPU.  Import saddle_point_petsc_amd before anything else that loads a HIP runtime of its own, or set "
                          "LD_LIBRARY_PATH so that both resolve libamdhip64.so.7 to the same file.")
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    L.spk_version.restype = C.c_int
    L.spk_last_error.restype = C.c_char_p
    L.spk_last_error.argtypes = [vp]
    L.spk_default_opts.argtypes = [C.POINTER(Opts)]
    L.spk_default_opts.restype = None
    L.spk_create.argtypes = [C.POINTER(vp), C.c_int]
    L.spk_destroy.argtypes = [vp]
    L.spk_comm_unique_id.argtypes = [C.c_char_p]
    L.spk_comm_init_rccl.argtypes = [vp, C.c_int, C.c_int, C.c_char_p]
    L.spk_comm_init_host.argtypes = [vp, C.c_int, C.c_int, C.POINTER(HostComm)]
    L.spk_local_group_create.argtypes = [C.POINTER(vp), C.c_int]
    L.spk_local_group_destroy.argtypes = [vp]
    L.spk_comm_init_local.argtypes = [vp, vp, C.c_int]
    L.spk_comm_enable_peer.argtypes = [vp, C.POINTER(i32)]
    L.spk_comm_backend.restype = C.c_char_p
    L.spk_comm_backend.argtypes = [vp]
    L.spk_comm_get_info.argtypes = [vp, C.POINTER(CommInfo)]
    L.spk_debug_peer_allreduce_loopback.argtypes = [vp, C.c_int, C.c_int, C.c_int, f64p, f64p]
    L.spk_debug_finish_timeout.argtypes = [vp, C.c_int]
    L.spk_debug_set_wait_bound.argtypes = [vp, C.c_uint32]
    L.spk_debug_wave_sums.argtypes = [vp, C.c_int, f64p, f64p]
    L.spk_debug_vec_shape.argtypes = [vp, i64, i32p]
    L.spk_debug_mdot.argtypes = [vp, C.POINTER(DebugMdotOpts), vp, vp, f64p, f64p]
    L.spk_debug_mdot_f32.argtypes = [vp, C.POINTER(DebugMdotOpts), vp, vp, f64p, f64p]
    L.spk_debug_maxpy.argtypes = [vp, C.POINTER(DebugMaxpyOpts), vp, f64p, f64p, vp, vp, vp, f64p, vp, vp]
    L.spk_debug_cycle_norm.argtypes = [vp, i64, i64, i64, i32, dbl, f64p, vp, vp, vp, f64p, vp]
    L.spk_debug_schur_w.argtypes = [vp, i64, i32, i32, i32, dbl, f64p, f64p, f64p, vp, vp, f64p]
    L.spk_debug_pack_bd.argtypes = [vp, i64, i32, f64p, vp, C.POINTER(i32)]
    L.spk_debug_cycle_head.argtypes = [vp, C.POINTER(DebugHeadOpts), f64p, f64p, vp, f64p, vp, vp, vp, f64p, vp, vp]
    L.spk_debug_gs_stamps.argtypes = [vp, np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")]
    L.spk_debug_time_products.argtypes = [vp, C.c_int32]
    L.spk_get_product_timing.argtypes = [vp, C.POINTER(C.c_int32)] + [C.POINTER(C.c_double)] * 4 + [C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.spk_set_block.argtypes = [vp, C.c_int, i64, i32, i64, i32p, i32p, f64p]
    L.spk_set_block_laplace.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp]
    L.spk_assemble_laplace_csr.argtypes = [vp, C.c_int, C.c_int, i64, i64, vp, C.c_int, C.c_int, i32p, i32p, f64p, vp]
    L.spk_set_block_laplace3d.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp]
    L.spk_assemble_laplace3d_csr.argtypes = [vp, C.c_int, C.c_int, C.c_int, i64, i64, vp, C.c_int, C.c_int, i32p, i32p, f64p, vp]
    L.spk_get_assembly_seconds.argtypes = [vp, C.POINTER(dbl)]
    L.spk_set_block_constraints.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    L.spk_assemble_constraints_csr.argtypes = [vp, C.c_int, C.c_int, C.c_int, i64, i64, i32p, f64p, i32p, i32p, f64p,
                                               C.POINTER(i32), C.POINTER(i32), i32p, i64]
    L.spk_host_constraints_csr.argtypes = [C.c_int, C.c_int, C.c_int, i64, i64, i32p, f64p, i32p, i32p, f64p,
                                           C.POINTER(i32), C.POINTER(i32), i32p, i64]
    L.spk_get_constraints_seconds.argtypes = [vp, C.POINTER(dbl)]
    L.spk_pc_setup.argtypes = [vp, C.c_int, C.c_int]
    L.spk_pc_set_inner.argtypes = [vp, C.c_int, C.c_double]
    L.spk_default_amg_opts.argtypes = [C.POINTER(AmgOpts)]
    L.spk_default_amg_opts.restype = None
    L.spk_pc_set_amg.argtypes = [vp, C.POINTER(AmgOpts)]
    L.spk_get_amg_info.argtypes = [vp, C.POINTER(AmgInfo)]
    L.spk_get_amg_level.argtypes = [vp, C.c_int, C.c_int, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), vp, vp, vp]
    L.spk_get_amg_aggregates.argtypes = [vp, C.c_int, C.POINTER(i32), vp]
    L.spk_debug_amg_transfer.argtypes = [vp, C.c_int, C.c_int, C.c_int, i64, f64p, f64p, f64p]
    L.spk_debug_amg_operator.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, f64p, C.c_void_p, C.c_void_p, f64p]
    L.spk_debug_amg_operator_f32.argtypes = [vp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.spk_debug_amg_transfer_f32.argtypes = [vp, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.spk_debug_amg_lanczos.argtypes = [vp, C.c_int, C.c_int, C.POINTER(i32), f64p, f64p]
    L.spk_amg_build_host.argtypes = [i32, i32p, i32p, f64p, C.POINTER(AmgOpts), C.POINTER(vp)]
    L.spk_amg_refresh_host.argtypes = [vp, vp]
    L.spk_amg_destroy_host.argtypes = [vp]
    L.spk_pc_set_amg_reuse.argtypes = [vp, C.c_int]
    L.spk_get_amg_reuse_info.argtypes = [vp, C.POINTER(i32), C.POINTER(dbl)]
    L.spk_amg_host_info.argtypes = [vp, C.POINTER(AmgInfo)]
    L.spk_amg_host_level.argtypes = [vp, C.c_int, C.c_int, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), vp, vp, vp]
    L.spk_amg_host_aggregates.argtypes = [vp, C.c_int, C.POINTER(i32), vp]
    L.spk_amg_cycle_steps.argtypes = [i32, i32, C.POINTER(i64), vp]
    L.spk_amg_stencil_children.argtypes = [vp, vp, i32, C.POINTER(i32), vp, vp]
    L.spk_pc_set_schur_pre.argtypes = [vp, C.c_int]
    L.spk_get_schur_matrix.argtypes = [vp, f64p]
    L.spk_get_schur_setup_seconds.argtypes = [vp, C.POINTER(dbl)]
    L.spk_get_schur_diag.argtypes = [vp, f64p]
    L.spk_get_jacobi_diag.argtypes = [vp, f64p]
    L.spk_get_bd_planes.argtypes = [vp, C.POINTER(i32)]
    L.spk_get_constraint_layout.argtypes = [vp] + [C.POINTER(i32)] * 7
    L.spk_mult.argtypes = [vp, f64p, f64p, C.c_int]
    L.spk_pc_apply.argtypes = [vp, f64p, f64p, C.c_int]
    L.spk_fgmres.argtypes = [vp, f64p, f64p, C.c_int, C.POINTER(Opts), C.POINTER(Result), vp, i32]
    L.spk_minres.argtypes = [vp, vp, vp, C.c_int, C.POINTER(Opts), C.c_int, C.POINTER(Result), vp, i32]
    L.spk_pipecg.argtypes = [vp, vp, vp, C.c_int, C.POINTER(Opts), C.c_int, C.POINTER(Result), vp, i32]
    L.spk_pipecgrr.argtypes = [vp, vp, vp, C.c_int, C.POINTER(Opts), C.c_int, C.POINTER(Result), vp, i32, C.POINTER(i32)]
    L.spk_pipecgrr_set_tau.argtypes = [vp, dbl]
    L.spk_vec_create.argtypes = [vp, i64, C.POINTER(vp)]
    L.spk_vec_destroy.argtypes = [vp, vp]
    L.spk_vec_set.argtypes = [vp, vp, f64p, i64]
    L.spk_vec_get.argtypes = [vp, vp, f64p, i64]
    L.spk_get_sizes.argtypes = [vp, C.POINTER(i64), C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), C.POINTER(i32)]
    L.spk_kernel_mdot.argtypes = [vp, i64, i32, f64p, i64, f64p, f64p]
    L.spk_kernel_maxpy.argtypes = [vp, i64, i32, f64p, f64p, i64, f64p, C.POINTER(dbl)]
    L.spk_time_spmv.argtypes = [vp, C.c_int, C.c_int, C.POINTER(dbl)]
    L.spk_get_spmv_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i64)]
    L.spk_debug_dict_layout.argtypes = [vp, C.POINTER(i32)]
    L.spk_get_iteration_form.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.spk_get_gs_launch.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.spk_get_basis_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i64)]
    L.spk_get_spmv_models.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i32), C.POINTER(i32)]
    L.spk_time_kernel.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(dbl)]
    L.spk_partition_slab.argtypes = [i64, i64, C.c_int, C.c_int, C.POINTER(i64), C.POINTER(i64)]
    L.spk_partition_split.argtypes = [i64, i32, i32p, i32p, f64p] + [vp] * 7 + [C.POINTER(i64), C.POINTER(i64), C.POINTER(i32)]
    # assembly
    L.SpkAssemblySizes.argtypes = [C.c_int, C.c_int, C.POINTER(i64), C.POINTER(i64)]
    L.SpkAssemblySlabNnz.restype = i64
    L.SpkAssemblySlabNnz.argtypes = [C.c_int, C.c_int, i64, i64]
    L.SpkAssembleOperator_Laplace.argtypes = [C.c_int, C.c_int, i64, i64, i32p, i32p, f64p, vp, C.c_int, C.c_int]
    L.SpkAssembleOperator_LaplaceKappa.argtypes = [C.c_int, C.c_int, i64, i64, vp, i32p, i32p, f64p, vp, C.c_int, C.c_int]
    L.SpkAssemblyRowPointers.argtypes = [C.c_int, C.c_int, i64, i64, i32p]
    L.SpkAssemblyCheckKappa.argtypes = [C.c_int, C.c_int, vp]
    L.SpkConstraintsSlabNnz.restype = i64
    L.SpkConstraintsSlabNnz.argtypes = [C.c_int, C.c_int, i64, i64]
    L.SpkAssembleOperator_Constraints.argtypes = [C.c_int, C.c_int, i64, i64, i32p, i32p, f64p]
    L.SpkAssembleRHS_Constraints.argtypes = [f64p]
    L.SpkAssemblySizes3D.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(i64), C.POINTER(i64)]
    L.SpkAssemblySlabNnz3D.restype = i64
    L.SpkAssemblySlabNnz3D.argtypes = [C.c_int, C.c_int, C.c_int, i64, i64]
    L.SpkAssembleOperator_Laplace3D.argtypes = [C.c_int, C.c_int, C.c_int, i64, i64, i32p, i32p, f64p, vp, C.c_int, C.c_int]
    L.SpkAssembleOperator_Laplace3DKappa.argtypes = [C.c_int, C.c_int, C.c_int, i64, i64, vp, i32p, i32p, f64p, vp, C.c_int, C.c_int]
    L.SpkAssemblyRowPointers3D.argtypes = [C.c_int, C.c_int, C.c_int, i64, i64, i32p]
    L.SpkAssemblyCheckKappa3D.argtypes = [C.c_int, C.c_int, C.c_int, vp]
    L.SpkConstraintsSlabNnz3D.restype = i64
    L.SpkConstraintsSlabNnz3D.argtypes = [C.c_int, C.c_int, C.c_int, i64, i64]
    L.SpkAssembleOperator_Constraints3D.argtypes = [C.c_int, C.c_int, C.c_int, i64, i64, i32p, i32p, f64p]
    L.SpkAssembleRHS_Constraints3D.argtypes = [f64p]
    L.SpkDivergenceSlabNnz3D.restype = i64
    L.SpkDivergenceSlabNnz3D.argtypes = [C.c_int, C.c_int, C.c_int, i64, i64]
    L.SpkAssembleOperator_Divergence3D.argtypes = [C.c_int, C.c_int, C.c_int, i64, i64, i32p, i32p, f64p]
    L.SpkWriteVTK.argtypes = [C.c_int, C.c_int, f64p, C.c_char_p]
    L.SpkFormStressOperatorQ12D.argtypes = [f64p, f64p, f64p]
    L.SpkFormLaplaceRHSQ12D.argtypes = [f64p, f64p]
    L.SpkFormStressOperatorQ13D.argtypes = [f64p, C.c_double, f64p, f64p]
    # KSP facade
    L.SpkKSPCreate.argtypes = [C.c_int, C.POINTER(vp)]
    L.SpkKSPSetCommRCCL.argtypes = [vp, C.c_int, C.c_int, C.c_char_p]
    L.SpkKSPSetOperators.argtypes = [vp, C.POINTER(MatCSR), C.POINTER(MatCSR)]
    L.SpkKSPSetOperatorsLaplace.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(MatCSR), vp]
    L.SpkKSPSetOperatorsLaplace3D.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.POINTER(MatCSR), vp]
    L.SpkKSPSetOperatorsLaplaceConstrained.argtypes = [vp, C.c_int, C.c_int, vp, vp]
    L.SpkKSPSetOperatorsLaplaceConstrained3D.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.SpkKSPSetGrid.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.SpkKSPSetFromOptions.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p)]
    L.SpkKSPSetUp.argtypes = [vp]
    L.SpkKSPSolve.argtypes = [vp, f64p, f64p]
    L.SpkKSPDestroy.argtypes = [C.POINTER(vp)]
    L.SpkKSPGetIterationNumber.argtypes = [vp, C.POINTER(i32)]
    L.SpkKSPGetConvergedReason.argtypes = [vp, C.POINTER(i32)]
    L.SpkKSPGetResidualNorm.argtypes = [vp, C.POINTER(dbl)]
    L.SpkKSPGetResidualHistory.argtypes = [vp, C.POINTER(C.POINTER(dbl)), C.POINTER(i32)]
    L.SpkKSPGetSolveTime.argtypes = [vp, C.POINTER(dbl)]
    L.SpkKSPGetOptions.argtypes = [vp, C.POINTER(Opts), C.POINTER(i32), C.POINTER(i32)]
    L.SpkKSPGetContext.argtypes = [vp, C.POINTER(vp)]
    L.SpkKSPGetAMGOptions.argtypes = [vp, C.c_int, C.POINTER(AmgOpts), C.POINTER(i32)]
    L.SpkKSPGetAMGReuse.argtypes = [vp, C.c_int, C.POINTER(i32)]
    L.SpkKSPGetType.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(i32)]
    L.SpkKSPGetSchurPre.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.SpkKSPGetError.restype = C.c_char_p
    L.SpkKSPGetError.argtypes = [vp]
    L.SpkKSPConvergedReasonName.restype = C.c_char_p
    L.SpkKSPConvergedReasonName.argtypes = [i32]
    return L


_hip_preloaded = None
lib = _load()
