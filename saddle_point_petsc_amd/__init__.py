"""saddle_point_petsc_amd -- MI355X-native replacement for the KSPSolve hot path
of p-m-mueller/saddle_point_petsc (FGMRES + Schur fieldsplit on
[A B^T; B 0]).  The product is the C-ABI library libspk.so (include/spk.h);
this package is its ctypes front end plus the host-side mirror of the
reference's call site.  No CPU fallback: importing needs the built library and
solving needs a GPU."""
from ._lib import lib, SpkError, LIB_PATH  # noqa: F401
from .csr import CSR  # noqa: F401
from .assembly import (  # noqa: F401
    AssembleOperator_Laplace, AssembleOperator_Constraints, FormStressOperatorQ12D,
    FormLaplaceRHSQ12D, grid_sizes, partition_slab, WriteVTK, slab_row_pointers, element_kappa,
    AssembleOperator_Laplace3D, AssembleOperator_Constraints3D, AssembleOperator_Divergence3D, partition_slab3d,
    FormStressOperatorQ13D, slab_row_pointers3d, element_kappa3d,
)
from .solver import (  # noqa: F401
    Context, KSP, LocalGroup, default_opts, unique_id,
    PC_NONE, PC_JACOBI, PC_SCHUR, SCHUR_DIAG, SCHUR_LOWER, SCHUR_UPPER, SCHUR_FULL,
    BLOCK_A00, BLOCK_A10, MEM_HOST, MEM_DEVICE, NORM_UNPRECONDITIONED, NORM_NATURAL, DIVERGED_INDEFINITE_PC,
    DIVERGED_INDEFINITE_MAT, PIPECGRR_TAU_DEFAULT, SCHUR_PRE_SELFP_DIAG, SCHUR_PRE_FULL,
    AmgHierarchy, amg_opts, AMG_CHEBYSHEV, AMG_RICHARDSON, AMG_SETUP_HOST, AMG_SETUP_DEVICE, AMG_COARSEN_AGGREGATION, AMG_COARSEN_GRID,
    AMG_TRANSFER_MATRIX_FREE, AMG_TRANSFER_STORED, AMG_SIDES_ODD, AMG_SIDES_ANY, AMG_OP, AMG_PROLONG, AMG_TENTATIVE, AMG_COARSE_INV,
    AMG_CYCLE_V, AMG_CYCLE_W, AMG_TAIL_AUTO, AMG_TAIL_LAUNCHES, AMG_TAIL_FUSED, amg_cycle_steps,
    AMG_STEP_PRE0, AMG_STEP_PRE, AMG_STEP_DOWN, AMG_STEP_COARSE, AMG_STEP_UP, AMG_STEP_POST,
    AMG_GALERKIN_PRODUCTS, AMG_GALERKIN_STENCIL, AMG_OPERATOR_CSR, AMG_OPERATOR_STENCIL, amg_stencil_children,
    AMG_LANCZOS_STEPWISE, AMG_LANCZOS_RESIDENT, AMG_PRECISION_DOUBLE, AMG_PRECISION_SINGLE,
)
