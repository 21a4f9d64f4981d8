"""ctypes binding of include/cvr_amd.h (libcvr_amd.so).  Mirrors the reference's call sequence
(main, spmv.cpp:1771-1938): load -> create/preprocess (pre_processing) -> spmv (spmv_compute_kernel) -> verdict."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_IO, ERR_NOMEM, ERR_STATE, ERR_INTERNAL = 0, -1, -2, -3, -4, -5, -6, -7
MM_REFCOMPAT, MM_STRICT = 0, 1


_torch_first = None      # was torch already imported when libcvr_amd.so was loaded?


class CvrError(RuntimeError):
    def __init__(self, code, where):
        import sys as _sys
        self.code = code
        hint = ""
        if code == ERR_NO_DEVICE and _torch_first is False and "torch" in _sys.modules:
            hint = (" -- PyTorch was imported AFTER libcvr_amd.so: two copies of the HIP runtime share the process and the second one"
                    " finds no GPU; import torch first (or set CVR_TORCH_PRELOAD=1)")
        super().__init__(f"{where}: error {code}: {last_error()}{hint}")


class CsrView(C.Structure):
    _fields_ = [("nrows", C.c_int64), ("ncols", C.c_int64), ("row_ptr", C.c_void_p), ("col_idx", C.c_void_p),
                ("vals", C.c_void_p), ("is_f32", C.c_int32), ("arrays_on_device", C.c_int32)]


class Options(C.Structure):
    _fields_ = [("device", C.c_int32), ("steps_per_chunk", C.c_int32), ("split_threshold", C.c_int64),
                ("xcd_swizzle", C.c_int32), ("x_window", C.c_int32), ("waves_per_block", C.c_int32),
                ("col_panels", C.c_int32), ("value_dict", C.c_int32), ("col_phases", C.c_int32), ("hub_table", C.c_int32), ("narrow_cols", C.c_int32),
                ("hub_reorder", C.c_int32), ("row_tags16", C.c_int32), ("row_bands", C.c_int32), ("piece_max", C.c_int32), ("interleave", C.c_int32), ("gang", C.c_int32), ("nvec", C.c_int32), ("reserved", C.c_int32 * 2)]

    # cvr_options.mutable_values took reserved[0] in C (include/cvr_amd.h); the Python struct keeps the two-word `reserved` field of the
    # same bytes, and the option reads and writes its first word
    @property
    def mutable_values(self):
        return self.reserved[0]

    @mutable_values.setter
    def mutable_values(self, v):
        self.reserved[0] = int(v)

    # cvr_options.transpose took reserved[1], the last reserved word: the handle of A^T built on the device from A's CSR
    @property
    def transpose(self):
        return self.reserved[1]

    @transpose.setter
    def transpose(self, v):
        self.reserved[1] = int(v)


class Timing(C.Structure):
    _fields_ = [("iters", C.c_int32), ("mean_s", C.c_double), ("min_s", C.c_double), ("max_s", C.c_double),
                ("total_s", C.c_double), ("h2d_s", C.c_double), ("d2h_s", C.c_double), ("median_s", C.c_double),
                ("step_mean_s", C.c_double), ("step_min_s", C.c_double), ("step_median_s", C.c_double), ("step_max_s", C.c_double),
                ("gather_mean_s", C.c_double)]


class Info(C.Structure):
    _fields_ = [("nrows", C.c_int64), ("ncols", C.c_int64), ("nnz", C.c_int64), ("is_f32", C.c_int32),
                ("steps_per_chunk", C.c_int32), ("nchunks", C.c_int64), ("nslots", C.c_int64), ("nshared", C.c_int64),
                ("image_bytes", C.c_int64), ("yext_elems", C.c_int64), ("x_elems", C.c_int64),
                ("plan_s", C.c_double), ("upload_s", C.c_double), ("convert_s", C.c_double),
                ("col_panels", C.c_int32), ("value_dict", C.c_int32), ("col_phases", C.c_int32), ("waves_per_block", C.c_int32),
                ("x_window", C.c_int32), ("lds_bytes", C.c_int32), ("nsegments", C.c_int64), ("chunk_row_cap", C.c_int64), ("near_diagonal_share", C.c_double), ("hub_entries", C.c_int32), ("narrow_cols", C.c_int32), ("hub_reorder", C.c_int32), ("row_tags16", C.c_int32), ("hub_share", C.c_double),
                ("hub_select_s", C.c_double), ("probe_s", C.c_double), ("dict_s", C.c_double), ("preprocess_wall_s", C.c_double), ("row_bands", C.c_int32), ("piece_max", C.c_int32), ("spmv_launches", C.c_int32), ("preprocess_fused", C.c_int32), ("interleave", C.c_int32), ("gang", C.c_int32)]


class CgOptions(C.Structure):
    """cvr_cg_options"""
    _fields_ = [("max_iters", C.c_int32), ("check_every", C.c_int32), ("rtol", C.c_double), ("minv_dev", C.c_void_p), ("reserved", C.c_int32 * 4)]


class CgResult(C.Structure):
    """cvr_cg_result"""
    _fields_ = [("iterations", C.c_int32), ("status", C.c_int32), ("spmv_count", C.c_int32), ("reserved", C.c_int32),
                ("residual_norm", C.c_double), ("b_norm", C.c_double), ("seconds", C.c_double)]


CG_CONVERGED, CG_MAX_ITERS, CG_BREAKDOWN = 0, 1, 2


class PrecondInfo(C.Structure):
    """cvr_precond_info"""
    _fields_ = [("n", C.c_int64), ("block_size", C.c_int32), ("is_f32", C.c_int32), ("nblocks", C.c_int64), ("identity_blocks", C.c_int64),
                ("device", C.c_int32), ("reserved", C.c_int32)]


PRECOND_MAX_BLOCK = 32      # include/cvr_amd.h: CVR_PRECOND_MAX_BLOCK
CHEBYSHEV_MAX_DEGREE = 16   # include/cvr_amd.h: CVR_CHEBYSHEV_MAX_DEGREE
CHEBYSHEV_LMAX_FACTOR = 1.1  # include/cvr_amd.h: CVR_CHEBYSHEV_LMAX_FACTOR


class ChebyshevInfo(C.Structure):
    """cvr_chebyshev_info"""
    _fields_ = [("degree", C.c_int32), ("is_f32", C.c_int32), ("lmin", C.c_double), ("lmax", C.c_double),
                ("a", C.c_double * CHEBYSHEV_MAX_DEGREE), ("b", C.c_double * CHEBYSHEV_MAX_DEGREE)]


class Ilu0Info(C.Structure):
    """cvr_ilu0_info"""
    _fields_ = [("n", C.c_int64), ("nnz", C.c_int64), ("levels_lower", C.c_int32), ("levels_upper", C.c_int32), ("launches_lower", C.c_int32),
                ("launches_upper", C.c_int32), ("max_level_width", C.c_int32), ("lanes_per_row", C.c_int32), ("wide_threshold", C.c_int32),
                ("is_f32", C.c_int32), ("reserved", C.c_int32 * 8)]


ILU0_MAX_SWEEPS = 64        # include/cvr_amd.h: CVR_ILU0_MAX_SWEEPS


class Ilu0JacobiInfo(C.Structure):
    """cvr_ilu0_jacobi_info"""
    _fields_ = [("n", C.c_int64), ("nnz", C.c_int64), ("sweeps", C.c_int32), ("launches_per_apply", C.c_int32), ("lanes_per_row", C.c_int32),
                ("levels_lower", C.c_int32), ("levels_upper", C.c_int32), ("is_f32", C.c_int32), ("reserved", C.c_int32 * 8)]


class McSgsInfo(C.Structure):
    """cvr_mcsgs_info"""
    _fields_ = [("n", C.c_int64), ("nnz", C.c_int64), ("ncolors", C.c_int32), ("rounds", C.c_int32), ("launches_per_apply", C.c_int32),
                ("lanes_per_row", C.c_int32), ("max_color_rows", C.c_int32), ("min_color_rows", C.c_int32), ("is_f32", C.c_int32),
                ("reserved", C.c_int32 * 8)]


FSAI_MAX_ROW = 32           # include/cvr_amd.h: CVR_FSAI_MAX_ROW


class FsaiInfo(C.Structure):
    """cvr_fsai_info"""
    _fields_ = [("n", C.c_int64), ("nnz", C.c_int64), ("max_row", C.c_int32), ("lanes_per_row", C.c_int32), ("truncated_rows", C.c_int64),
                ("is_f32", C.c_int32), ("reserved", C.c_int32 * 9)]


AMG_MAX_LEVELS = 16         # include/cvr_amd.h: CVR_AMG_MAX_LEVELS
AMG_MAX_COARSE = 256        # include/cvr_amd.h: CVR_AMG_MAX_COARSE


class AmgOptions(C.Structure):
    """cvr_amg_options"""
    _fields_ = [("max_levels", C.c_int32), ("coarse_size", C.c_int32), ("sweeps", C.c_int32), ("reserved0", C.c_int32), ("strength", C.c_double),
                ("coarse_scale", C.c_double), ("reserved", C.c_int32 * 8)]


class AmgInfo(C.Structure):
    """cvr_amg_info"""
    _fields_ = [("levels", C.c_int32), ("coarse_direct", C.c_int32), ("sweeps", C.c_int32), ("is_f32", C.c_int32), ("max_levels", C.c_int32),
                ("coarse_size", C.c_int32), ("strength", C.c_double), ("coarse_scale", C.c_double), ("operator_complexity", C.c_double),
                ("n", C.c_int64 * AMG_MAX_LEVELS), ("nnz", C.c_int64 * AMG_MAX_LEVELS), ("reserved", C.c_int32 * 8)]


class AmgSmoothedInfo(C.Structure):
    """cvr_amg_smoothed_info"""
    _fields_ = [("smoothed", C.c_int32), ("products_per_apply", C.c_int32), ("omega", C.c_double), ("p_nnz", C.c_int64 * AMG_MAX_LEVELS),
                ("reserved", C.c_int32 * 8)]


class AmgMis2Info(C.Structure):
    """cvr_amg_mis2_info"""
    _fields_ = [("mis2", C.c_int32), ("reserved0", C.c_int32), ("rounds", C.c_int32 * AMG_MAX_LEVELS), ("reserved", C.c_int32 * 8)]


AMG_SETUP_PLAIN, AMG_SETUP_SMOOTHED, AMG_SETUP_MIS2 = 0, 1, 2          # include/cvr_amd.h: CVR_AMG_SETUP_*
AMG_SETUPS = {"plain": AMG_SETUP_PLAIN, "smoothed": AMG_SETUP_SMOOTHED, "mis2": AMG_SETUP_MIS2}


class AmgBlockInfo(C.Structure):
    """cvr_amg_block_info"""
    _fields_ = [("nvec", C.c_int32), ("setup", C.c_int32), ("buffer_bytes", C.c_int64), ("reserved", C.c_int32 * 8)]


class SpGemmInfo(C.Structure):
    """cvr_spgemm_info_t"""
    _fields_ = [("nrows", C.c_int64), ("ncols", C.c_int64), ("inner", C.c_int64), ("nnz", C.c_int64), ("products", C.c_int64), ("max_row_products", C.c_int64),
                ("rows_empty", C.c_int64), ("rows_group", C.c_int64), ("rows_block", C.c_int64), ("rows_spill", C.c_int64), ("group_limit", C.c_int64),
                ("block_limit", C.c_int64), ("is_f32", C.c_int32), ("lanes_per_row", C.c_int32), ("symbolic_s", C.c_double), ("numeric_s", C.c_double)]


GMRES_MAX_RESTART = 64      # include/cvr_amd.h: CVR_GMRES_MAX_RESTART
APPLY_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)      # cvr_apply_fn: (ctx, v_dev, z_dev, n, stream) -> int


class LsqrInfo(C.Structure):
    """cvr_lsqr_info"""
    _fields_ = [("arnorm", C.c_double), ("anorm", C.c_double), ("stop_test", C.c_int32), ("reserved", C.c_int32)]


class MinresInfo(C.Structure):
    """cvr_minres_info"""
    _fields_ = [("anorm", C.c_double), ("acond", C.c_double), ("reserved", C.c_int32 * 2)]


EIG_MAX_NCV = 64            # include/cvr_amd.h: CVR_EIG_MAX_NCV
EIG_LARGEST, EIG_SMALLEST = 0, 1
EIG_CONVERGED, EIG_MAX_RESTARTS, EIG_BREAKDOWN, EIG_INVARIANT = 0, 1, 2, 3
EIG_EPS23 = 3.666852862501036e-11   # include/cvr_amd.h: CVR_EIG_EPS23


class EigOptions(C.Structure):
    """cvr_eig_options"""
    _fields_ = [("nev", C.c_int32), ("ncv", C.c_int32), ("which", C.c_int32), ("max_restarts", C.c_int32), ("tol", C.c_double), ("reserved", C.c_int32 * 4)]


class EigResult(C.Structure):
    """cvr_eig_result"""
    _fields_ = [("nconv", C.c_int32), ("status", C.c_int32), ("restarts", C.c_int32), ("spmv_count", C.c_int32), ("seconds", C.c_double),
                ("max_estimate", C.c_double)]


SVD_MAX_NCV = 64            # include/cvr_amd.h: CVR_SVD_MAX_NCV


class SvdOptions(C.Structure):
    """cvr_svd_options"""
    _fields_ = [("nev", C.c_int32), ("ncv", C.c_int32), ("max_restarts", C.c_int32), ("reserved0", C.c_int32), ("tol", C.c_double), ("reserved", C.c_int32 * 4)]


class SvdResult(C.Structure):
    """cvr_svd_result (status: EIG_CONVERGED, EIG_MAX_RESTARTS, EIG_BREAKDOWN or EIG_INVARIANT)"""
    _fields_ = [("nconv", C.c_int32), ("status", C.c_int32), ("restarts", C.c_int32), ("spmv_count", C.c_int32), ("seconds", C.c_double),
                ("max_estimate", C.c_double)]


LOBPCG_MAX_BLOCK = 8        # include/cvr_amd.h: CVR_LOBPCG_MAX_BLOCK
EIG_MAX_ITERS = 4           # include/cvr_amd.h: CVR_EIG_MAX_ITERS (cvr_lobpcg only)


class LobpcgOptions(C.Structure):
    """cvr_lobpcg_options"""
    _fields_ = [("nev", C.c_int32), ("which", C.c_int32), ("max_iters", C.c_int32), ("reserved0", C.c_int32), ("tol", C.c_double), ("reserved", C.c_int32 * 4)]


class LobpcgResult(C.Structure):
    """cvr_lobpcg_result"""
    _fields_ = [("nconv", C.c_int32), ("status", C.c_int32), ("iterations", C.c_int32), ("spmv_count", C.c_int32), ("precond_applies", C.c_int32),
                ("restarts_without_p", C.c_int32), ("seconds", C.c_double), ("max_rel_residual", C.c_double)]


class MmMatrix(C.Structure):
    _fields_ = [("nrows", C.c_int64), ("ncols", C.c_int64), ("nnz", C.c_int64), ("ref_numRows", C.c_int64),
                ("ref_numCols", C.c_int64), ("ref_nItems", C.c_int64), ("ref_nItemsRaw", C.c_int64),
                ("row_ptr", C.POINTER(C.c_int64)), ("col_idx", C.POINTER(C.c_int32)), ("vals", C.POINTER(C.c_double))]


# every symbol include/cvr_amd.h declares (tests check the library exports all of them)
SYMBOLS = ["cvr_default_options", "cvr_last_error", "cvr_version", "cvr_device_count", "cvr_create", "cvr_preprocess",
           "cvr_get_info", "cvr_destroy", "cvr_spmv", "cvr_spmv_device", "cvr_spmv_device_repeat", "cvr_spmm_device", "cvr_spmm", "cvr_spmm_supported",
           "cvr_spmv_scaled_device", "cvr_spmv_scaled", "cvr_cg_default_options", "cvr_cg_device", "cvr_cg", "cvr_cg_multi_device", "cvr_cg_multi", "cvr_bicgstab_device", "cvr_bicgstab", "cvr_gmres_device", "cvr_gmres",
           "cvr_precond_block_jacobi", "cvr_precond_get_info", "cvr_precond_export", "cvr_precond_apply_device", "cvr_precond_destroy", "cvr_pcg_device", "cvr_pcg",
           "cvr_precond_chebyshev", "cvr_precond_chebyshev_info", "cvr_chebyshev_bounds",
           "cvr_precond_ilu0", "cvr_precond_ilu0_info", "cvr_precond_ilu0_export", "cvr_ilu0_levels_host",
           "cvr_precond_ilu0_jacobi", "cvr_precond_ilu0_jacobi_info",
           "cvr_precond_fsai", "cvr_precond_fsai_info", "cvr_precond_fsai_export", "cvr_fsai_factor_host",
           "cvr_amg_default_options", "cvr_precond_amg", "cvr_precond_amg_info", "cvr_precond_amg_export_level", "cvr_amg_setup_host", "cvr_amg_hierarchy_info",
           "cvr_amg_hierarchy_export_level", "cvr_amg_hierarchy_destroy",
           "cvr_precond_amg_smoothed", "cvr_amg_smoothed_setup_host", "cvr_precond_amg_smoothed_info", "cvr_amg_hierarchy_smoothed_info",
           "cvr_precond_amg_export_prolongator", "cvr_amg_hierarchy_export_prolongator",
           "cvr_precond_amg_mis2", "cvr_amg_mis2_setup_host", "cvr_precond_amg_mis2_info", "cvr_amg_hierarchy_mis2_info", "cvr_amg_mis2_aggregate_host",
           "cvr_amg_mis2_aggregate_device", "cvr_precond_amg_block", "cvr_precond_amg_block_info",
           "cvr_color_host", "cvr_color_device", "cvr_precond_mcsgs", "cvr_precond_mcsgs_info", "cvr_precond_mcsgs_export",
           "cvr_spgemm_create", "cvr_spgemm_get_info", "cvr_spgemm_csr_device", "cvr_spgemm_export", "cvr_spgemm_numeric_device", "cvr_spgemm_destroy", "cvr_spgemm_host",
           "cvr_precond_apply_multi_device", "cvr_pcg_multi_device", "cvr_pcg_multi",
           "cvr_pbicgstab_device", "cvr_pbicgstab", "cvr_pgmres_device", "cvr_pgmres", "cvr_fgmres_device", "cvr_fgmres", "cvr_lsqr_device", "cvr_lsqr", "cvr_minres_device", "cvr_minres",
           "cvr_eig_default_options", "cvr_eigsh_device", "cvr_eigsh", "cvr_sym_eig_host",
           "cvr_lobpcg_default_options", "cvr_lobpcg_device", "cvr_lobpcg",
           "cvr_svd_default_options", "cvr_svds_device", "cvr_svds", "cvr_svd_host",
           "cvr_update_values_device", "cvr_update_values", "cvr_update_values_supported", "cvr_x_device", "cvr_y_device", "cvr_stream",
           "cvr_spmv_bench", "cvr_debug_phase_clocks", "cvr_device_copy_bench", "cvr_export_image", "cvr_export_gang", "cvr_comm_info", "cvr_plan_bound", "cvr_plan_chunks", "cvr_plan_selfcheck", "cvr_power_step_selfcheck", "cvr_mm_read", "cvr_mm_free", "cvr_mm_write_bin", "cvr_mm_read_bin",
           "cvr_fill_x", "cvr_csr_spmv_host", "cvr_verdict",
           "cvr_tune_steps", "cvr_tune", "cvr_auto_panels", "cvr_power_iteration", "cvr_comm_unique_id", "cvr_comm_create", "cvr_comm_destroy", "cvr_comm_all_gather", "cvr_spmv_gather_repeat",
           "cvr_source_key_of", "cvr_mm_write_bin_keyed", "cvr_mm_read_bin_keyed", "cvr_mm_read_cached", "cvr_save_image", "cvr_load_image",
           "cvr_row_partition", "cvr_row_partition_cost", "cvr_create_multi", "cvr_preprocess_multi", "cvr_spmv_multi", "cvr_multi_shards", "cvr_multi_info", "cvr_multi_uses_rccl", "cvr_destroy_multi", "cvr_multi_from_handles", "cvr_multi_handle"]


def lib_path():
    return os.path.join(_HERE, "libcvr_amd.so")


def lib():
    """Loads libcvr_amd.so; raises if it is not built -- there is no fallback."""
    global _lib
    if _lib is None:
        p = lib_path()
        if not os.path.exists(p):
            raise ImportError(f"{p} is missing: build it with `make -C cvr_amd/csrc` (or __graft_entry__.build())")
        # A process that also uses PyTorch must load torch FIRST: its wheel carries its own copy of the HIP runtime, and whichever
        # copy is loaded second finds no GPU.  The order is the caller's (importing torch here would put a second
        # runtime into processes that never wanted one: the CSR comparators and rocprofv3 crash on that); what this module does is
        # say so when it sees the wrong order behind a "no device" error (CvrError), and CVR_TORCH_PRELOAD=1 imports torch here.
        import sys as _sys
        global _torch_first
        if "torch" not in _sys.modules and os.environ.get("CVR_TORCH_PRELOAD"):      # opt-in: a caller that will import torch later
            try:
                import torch  # noqa: F401
            except Exception:  # noqa: BLE001
                pass
        _torch_first = "torch" in _sys.modules
        L = C.CDLL(p)
        L.cvr_last_error.restype = C.c_char_p
        L.cvr_version.restype = C.c_char_p
        L.cvr_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(CsrView), C.POINTER(Options)]
        L.cvr_preprocess.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        L.cvr_get_info.argtypes = [C.c_void_p, C.POINTER(Info)]
        L.cvr_destroy.argtypes = [C.c_void_p]
        L.cvr_spmv.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(Timing)]
        L.cvr_spmv_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cvr_spmv_device_repeat.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.cvr_spmm_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        L.cvr_spmm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.POINTER(Timing)]
        L.cvr_spmm_supported.argtypes = [C.c_void_p]
        L.cvr_spmv_scaled_device.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
        L.cvr_spmv_scaled.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_double, C.c_void_p]
        L.cvr_cg_default_options.argtypes = [C.POINTER(CgOptions)]
        L.cvr_cg_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CgOptions), C.POINTER(CgResult), C.c_void_p]
        L.cvr_cg.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CgOptions), C.POINTER(CgResult)]
        L.cvr_cg_multi_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(CgOptions), C.POINTER(CgResult), C.c_void_p]
        L.cvr_cg_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(CgOptions), C.POINTER(CgResult)]
        L.cvr_bicgstab_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CgOptions), C.POINTER(CgResult), C.c_void_p]
        L.cvr_bicgstab.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CgOptions), C.POINTER(CgResult)]
        L.cvr_gmres_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(CgOptions), C.POINTER(CgResult), C.c_void_p]
        L.cvr_gmres.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(CgOptions), C.POINTER(CgResult)]
        L.cvr_precond_block_jacobi.argtypes = [C.POINTER(C.c_void_p), C.POINTER(CsrView), C.c_int32, C.c_int32, C.c_void_p]
        L.cvr_precond_get_info.argtypes = [C.c_void_p, C.POINTER(PrecondInfo)]
        L.cvr_precond_export.argtypes = [C.c_void_p, C.c_void_p]
        L.cvr_precond_apply_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cvr_precond_destroy.argtypes = [C.c_void_p]
        L.cvr_pcg_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CgOptions), C.POINTER(CgResult), C.c_void_p]
        L.cvr_pcg.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CgOptions), C.POINTER(CgResult)]
        L.cvr_precond_chebyshev.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int32, C.c_double, C.c_double]
        L.cvr_precond_chebyshev_info.argtypes = [C.c_void_p, C.POINTER(ChebyshevInfo)]
        L.cvr_chebyshev_bounds.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p]
        L.cvr_precond_ilu0.argtypes = [C.POINTER(C.c_void_p), C.POINTER(CsrView), C.c_int32, C.c_void_p]
        L.cvr_precond_ilu0_info.argtypes = [C.c_void_p, C.POINTER(Ilu0Info)]
        L.cvr_precond_ilu0_export.argtypes = [C.c_void_p, C.c_void_p]
        L.cvr_ilu0_levels_host.argtypes = [C.POINTER(CsrView), C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.cvr_precond_ilu0_jacobi.argtypes = [C.POINTER(C.c_void_p), C.POINTER(CsrView), C.c_int32, C.c_int32, C.c_void_p]
        L.cvr_precond_ilu0_jacobi_info.argtypes = [C.c_void_p, C.POINTER(Ilu0JacobiInfo)]
        L.cvr_precond_fsai.argtypes = [C.POINTER(C.c_void_p), C.POINTER(CsrView), C.c_int32, C.c_void_p]
        L.cvr_precond_fsai_info.argtypes = [C.c_void_p, C.POINTER(FsaiInfo)]
        L.cvr_precond_fsai_export.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cvr_fsai_factor_host.argtypes = [C.POINTER(CsrView), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        L.cvr_amg_default_options.argtypes = [C.POINTER(AmgOptions)]
        L.cvr_precond_amg.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(CsrView), C.POINTER(AmgOptions), C.c_void_p]
        L.cvr_precond_amg_info.argtypes = [C.c_void_p, C.POINTER(AmgInfo)]
        L.cvr_precond_amg_export_level.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6
        L.cvr_amg_setup_host.argtypes = [C.POINTER(C.c_void_p), C.POINTER(CsrView), C.POINTER(AmgOptions), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
        L.cvr_amg_hierarchy_info.argtypes = [C.c_void_p, C.POINTER(AmgInfo)]
        L.cvr_spgemm_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(CsrView), C.POINTER(CsrView), C.c_int32, C.c_void_p]
        L.cvr_spgemm_get_info.argtypes = [C.c_void_p, C.POINTER(SpGemmInfo)]
        L.cvr_spgemm_csr_device.argtypes = [C.c_void_p, C.POINTER(CsrView)]
        L.cvr_spgemm_export.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cvr_spgemm_numeric_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cvr_spgemm_destroy.argtypes = [C.c_void_p]
        L.cvr_spgemm_host.argtypes = [C.POINTER(CsrView), C.POINTER(CsrView), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        L.cvr_amg_hierarchy_export_level.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6
        L.cvr_amg_hierarchy_destroy.argtypes = [C.c_void_p]
        L.cvr_precond_amg_smoothed.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(CsrView), C.POINTER(AmgOptions), C.c_double, C.c_void_p]
        L.cvr_amg_smoothed_setup_host.argtypes = [C.POINTER(C.c_void_p), C.POINTER(CsrView), C.POINTER(AmgOptions), C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
        L.cvr_precond_amg_smoothed_info.argtypes = [C.c_void_p, C.POINTER(AmgSmoothedInfo)]
        L.cvr_amg_hierarchy_smoothed_info.argtypes = [C.c_void_p, C.POINTER(AmgSmoothedInfo)]
        L.cvr_precond_amg_export_prolongator.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cvr_amg_hierarchy_export_prolongator.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cvr_precond_amg_mis2.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(CsrView), C.POINTER(AmgOptions), C.c_double, C.c_void_p]
        L.cvr_amg_mis2_setup_host.argtypes = [C.POINTER(C.c_void_p), C.POINTER(CsrView), C.POINTER(AmgOptions), C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
        L.cvr_precond_amg_mis2_info.argtypes = [C.c_void_p, C.POINTER(AmgMis2Info)]
        L.cvr_amg_hierarchy_mis2_info.argtypes = [C.c_void_p, C.POINTER(AmgMis2Info)]
        L.cvr_precond_amg_block.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(CsrView), C.POINTER(AmgOptions), C.c_int32, C.c_double, C.c_int32, C.c_void_p]
        L.cvr_precond_amg_block_info.argtypes = [C.c_void_p, C.POINTER(AmgBlockInfo)]
        L.cvr_amg_mis2_aggregate_host.argtypes = [C.POINTER(CsrView), C.c_double, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        L.cvr_amg_mis2_aggregate_device.argtypes = [C.POINTER(CsrView), C.c_double, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int, C.c_void_p]
        L.cvr_color_host.argtypes = [C.POINTER(CsrView), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.cvr_color_device.argtypes = [C.POINTER(CsrView), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.cvr_precond_mcsgs.argtypes = [C.POINTER(C.c_void_p), C.POINTER(CsrView), C.c_int32, C.c_void_p]
        L.cvr_precond_mcsgs_info.argtypes = [C.c_void_p, C.POINTER(McSgsInfo)]
        L.cvr_precond_mcsgs_export.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cvr_precond_apply_multi_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        L.cvr_pcg_multi_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(CgOptions), C.POINTER(CgResult), C.c_void_p]
        L.cvr_pcg_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(CgOptions), C.POINTER(CgResult)]
        L.cvr_pbicgstab_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CgOptions), C.POINTER(CgResult), C.c_void_p]
        L.cvr_pbicgstab.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CgOptions), C.POINTER(CgResult)]
        L.cvr_pgmres_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(CgOptions), C.POINTER(CgResult), C.c_void_p]
        L.cvr_pgmres.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(CgOptions), C.POINTER(CgResult)]
        L.cvr_fgmres_device.argtypes = [C.c_void_p, C.c_void_p, APPLY_FN, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(CgOptions), C.POINTER(CgResult), C.c_void_p]
        L.cvr_fgmres.argtypes = [C.c_void_p, C.c_void_p, APPLY_FN, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(CgOptions), C.POINTER(CgResult)]
        L.cvr_lsqr_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.POINTER(CgOptions), C.POINTER(CgResult), C.POINTER(LsqrInfo), C.c_void_p]
        L.cvr_lsqr.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.POINTER(CgOptions), C.POINTER(CgResult), C.POINTER(LsqrInfo)]
        L.cvr_minres_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.POINTER(CgOptions), C.POINTER(CgResult), C.POINTER(MinresInfo), C.c_void_p]
        L.cvr_minres.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.POINTER(CgOptions), C.POINTER(CgResult), C.POINTER(MinresInfo)]
        L.cvr_eig_default_options.argtypes = [C.POINTER(EigOptions)]
        L.cvr_eigsh_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(EigOptions), C.POINTER(EigResult), C.c_void_p]
        L.cvr_eigsh.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(EigOptions), C.POINTER(EigResult)]
        L.cvr_sym_eig_host.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
        L.cvr_svd_default_options.argtypes = [C.POINTER(SvdOptions)]
        L.cvr_svds_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(SvdOptions),
                                      C.POINTER(SvdResult), C.c_void_p]
        L.cvr_svds.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(SvdOptions),
                               C.POINTER(SvdResult)]
        L.cvr_svd_host.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.cvr_lobpcg_default_options.argtypes = [C.POINTER(LobpcgOptions)]
        L.cvr_lobpcg_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(LobpcgOptions), C.POINTER(LobpcgResult), C.c_void_p]
        L.cvr_lobpcg.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(LobpcgOptions), C.POINTER(LobpcgResult)]
        L.cvr_update_values_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.cvr_update_values.argtypes = [C.c_void_p, C.c_void_p]
        L.cvr_update_values_supported.argtypes = [C.c_void_p]
        for f in ("cvr_cg_default_options", "cvr_eig_default_options", "cvr_svd_default_options", "cvr_lobpcg_default_options"):
            getattr(L, f).restype = None
        for f in ("cvr_x_device", "cvr_y_device", "cvr_stream"):
            getattr(L, f).argtypes = [C.c_void_p]
            getattr(L, f).restype = C.c_void_p
        L.cvr_spmv_bench.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.cvr_debug_phase_clocks.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        L.cvr_export_image.argtypes = [C.c_void_p] * 5
        L.cvr_export_gang.argtypes = [C.c_void_p] * 3
        L.cvr_device_copy_bench.argtypes = [C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_double)]
        L.cvr_plan_selfcheck.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cvr_plan_selfcheck.restype = C.c_int
        L.cvr_power_step_selfcheck.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cvr_plan_bound.argtypes = [C.c_int64, C.c_int64, C.c_int32]
        L.cvr_plan_bound.restype = C.c_int64
        L.cvr_plan_chunks.argtypes = [C.c_int64, C.c_void_p, C.c_int32, C.c_int64] + [C.c_void_p] * 4
        L.cvr_plan_chunks.restype = C.c_int64
        L.cvr_mm_read.argtypes = [C.c_char_p, C.c_int, C.POINTER(MmMatrix)]
        L.cvr_mm_free.argtypes = [C.POINTER(MmMatrix)]
        L.cvr_mm_write_bin.argtypes = [C.c_char_p, C.POINTER(MmMatrix)]
        L.cvr_mm_read_bin.argtypes = [C.c_char_p, C.POINTER(MmMatrix)]
        L.cvr_fill_x.argtypes = [C.c_void_p, C.c_int64, C.c_int]
        L.cvr_csr_spmv_host.argtypes = [C.c_int64] + [C.c_void_p] * 5 + [C.c_int]
        L.cvr_verdict.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.cvr_verdict.restype = C.c_int64
        L.cvr_tune_steps.argtypes = [C.POINTER(CsrView), C.POINTER(Options), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.cvr_tune.argtypes = [C.POINTER(CsrView), C.POINTER(Options), C.POINTER(Options), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.cvr_auto_panels.argtypes = [C.POINTER(CsrView), C.POINTER(C.c_double)]
        L.cvr_power_iteration.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p]
        L.cvr_comm_unique_id.argtypes = [C.c_void_p]
        L.cvr_comm_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.cvr_comm_destroy.argtypes = [C.c_void_p]
        L.cvr_comm_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.cvr_comm_all_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
        L.cvr_spmv_gather_repeat.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                             C.c_int64, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.cvr_multi_handle.argtypes = [C.c_void_p, C.c_int32]
        L.cvr_multi_handle.restype = C.c_void_p
        L.cvr_multi_from_handles.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int32]
        L.cvr_source_key_of.argtypes = [C.c_char_p, C.c_int, C.POINTER(SourceKey)]
        L.cvr_mm_write_bin_keyed.argtypes = [C.c_char_p, C.POINTER(MmMatrix), C.POINTER(SourceKey)]
        L.cvr_mm_read_bin_keyed.argtypes = [C.c_char_p, C.POINTER(SourceKey), C.POINTER(MmMatrix)]
        L.cvr_mm_read_cached.argtypes = [C.c_char_p, C.c_int, C.POINTER(MmMatrix), C.POINTER(C.c_int)]
        L.cvr_save_image.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(SourceKey)]
        L.cvr_load_image.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.POINTER(SourceKey), C.POINTER(Options), C.POINTER(C.c_double)]
        L.cvr_row_partition.argtypes = [C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
        L.cvr_row_partition.restype = C.c_int64
        L.cvr_row_partition_cost.argtypes = [C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        L.cvr_row_partition_cost.restype = C.c_int64
        L.cvr_create_multi.argtypes = [C.POINTER(C.c_void_p), C.POINTER(CsrView), C.POINTER(Options), C.c_void_p, C.c_int32]
        L.cvr_preprocess_multi.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        L.cvr_spmv_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(Timing)]
        L.cvr_multi_shards.argtypes = [C.c_void_p]
        L.cvr_multi_uses_rccl.argtypes = [C.c_void_p]
        L.cvr_multi_info.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Info), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        L.cvr_destroy_multi.argtypes = [C.c_void_p]
        _lib = L
    return _lib


ROW_COST_MILLI_DEFAULT = 1250      # include/cvr_amd.h: CVR_ROW_COST_MILLI_DEFAULT


def row_partition(row_ptr, nparts, row_cost_milli=0):
    """cvr_row_partition_cost: bounds[nparts + 1] of contiguous row blocks cut at row boundaries with balanced cost = non-zeros +
    row_cost_milli / 1000 per row (0: balanced non-zeros, the reference's rule = cvr_row_partition).  Host only."""
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
    bounds = np.zeros(nparts + 1, dtype=np.int64)
    rc = lib().cvr_row_partition_cost(len(rp) - 1, rp.ctypes.data, nparts, int(row_cost_milli), bounds.ctypes.data)
    if rc < 0:
        raise CvrError(int(rc), "cvr_row_partition_cost")
    return bounds


def _host_view(rp, ci, vals=None, shape=None):
    """(view, keep) of host CSR arrays: a CsrView of a square matrix of len(rp) - 1 rows, or of shape = (nrows, ncols), over the arrays made contiguous
    in the ABI's types (vals: float32 stays, anything else becomes float64; None: the pattern alone), and `keep` = (rp, ci[, vals]), those arrays.
    The view holds raw pointers into them and no reference: whoever passes the view to C holds `keep` until that call has returned.  Raises the
    ValueError of a short row_ptr, col_idx or vals; loads no library."""
    rp = np.ascontiguousarray(rp, dtype=np.int64)
    ci = np.ascontiguousarray(ci, dtype=np.int32)
    nrows, ncols = (len(rp) - 1,) * 2 if shape is None else shape
    if vals is None:
        return CsrView(nrows, ncols, rp.ctypes.data, ci.ctypes.data, None, 0, 0), (rp, ci)
    f32 = np.asarray(vals).dtype == np.float32
    va = np.ascontiguousarray(vals, dtype=np.float32 if f32 else np.float64)
    if len(rp) != nrows + 1:
        raise ValueError("row_ptr must have nrows + 1 entries")
    if nrows > 0 and (len(ci) < rp[-1] or len(va) < rp[-1]):
        raise ValueError(f"col_idx / vals hold {len(ci)} / {len(va)} entries, row_ptr[nrows] = {int(rp[-1])}")
    return CsrView(int(nrows), int(ncols), rp.ctypes.data, ci.ctypes.data, va.ctypes.data, int(f32), 0), (rp, ci, va)


def _device_view(n, row_ptr_dev, col_idx_dev, vals_dev, is_f32=False):
    """the CsrView of a square matrix of n rows whose CSR arrays are the caller's, in a device's memory (raw pointers)"""
    return CsrView(n, n, row_ptr_dev, col_idx_dev, vals_dev, int(bool(is_f32)), 1)


def ilu0_levels_host(rp, ci):
    """cvr_ilu0_levels_host: (lower_level, upper_level, n_lower, n_upper) of a square CSR pattern with sorted rows and a diagonal in every row -- the
    level of each row in the L and the U sweep of Precond.ilu0, and the number of levels of each.  Host only."""
    view, keep = _host_view(rp, ci)
    n = view.nrows
    lo, up = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
    nlo, nup = C.c_int32(), C.c_int32()
    rc = lib().cvr_ilu0_levels_host(C.byref(view), lo.ctypes.data, up.ctypes.data, C.byref(nlo), C.byref(nup))
    if rc:
        raise CvrError(rc, "cvr_ilu0_levels_host")
    return lo[:n], up[:n], nlo.value, nup.value


def _color(call, name, n, view):
    color, perm, ptr = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32), np.zeros(n + 1, dtype=np.int32)
    nc, rounds = C.c_int32(), C.c_int32()
    rc = call(view, color.ctypes.data, perm.ctypes.data, ptr.ctypes.data, C.byref(nc), C.byref(rounds))
    if rc:
        raise CvrError(rc, name)
    return color[:n], perm[:n], ptr[: nc.value + 1], nc.value, rounds.value


def color_host(rp, ci):
    """cvr_color_host: (color, perm, color_ptr, ncolors, rounds) of a square CSR pattern with sorted rows, a diagonal in every row and a structurally
    symmetric off-diagonal pattern -- the colouring by rounds on hashed keys (greedy first-fit in descending key order), the rows ordered by
    (colour, row) and where each colour begins in that order.  Host only."""
    view, keep = _host_view(rp, ci)
    return _color(lambda v, *a: lib().cvr_color_host(C.byref(v), *a), "cvr_color_host", view.nrows, view)


def color_device(rp, ci, device=0, on_device=False, n=None):
    """cvr_color_device: the same on `device`, from host arrays, or (on_device: rp and ci are raw pointers, n the number of rows) from arrays in the
    device's memory; the outputs are host arrays either way"""
    view, keep = (_device_view(n, rp, ci, None), None) if on_device else _host_view(rp, ci)
    return _color(lambda v, *a: lib().cvr_color_device(C.byref(v), int(device), None, *a), "cvr_color_device", view.nrows, view)


def fsai_factor_host(rp, ci, vals):
    """cvr_fsai_factor_host: (row_ptr, col_idx, wa, wb, bad_row) of the FSAI factor W of a square CSR matrix with sorted rows and a diagonal in every
    row -- what Precond.fsai computes on the device, in host code (the type is vals' dtype, float32 or else float64).  bad_row is None, or the lowest
    row whose pivot is not finite or not > 0: the arrays then hold the rows before it.  Host only."""
    view, keep = _host_view(rp, ci, vals)
    n, dtype = view.nrows, keep[2].dtype
    room = max(int(keep[0][-1]), 1) if n > 0 else 1
    wrp, wci = np.zeros(n + 1, dtype=np.int64), np.zeros(room, dtype=np.int32)
    wa, wb = np.zeros(room, dtype=dtype), np.zeros(room, dtype=dtype)
    bad = C.c_int64(-1)
    rc = lib().cvr_fsai_factor_host(C.byref(view), wrp.ctypes.data, wci.ctypes.data, wa.ctypes.data, wb.ctypes.data, C.byref(bad))
    if rc and not (rc == ERR_STATE and bad.value >= 0):
        raise CvrError(rc, "cvr_fsai_factor_host")
    nnz = int(wrp[n])
    return wrp, wci[:nnz], wa[:nnz], wb[:nnz], (None if bad.value < 0 else int(bad.value))


def amg_options(**kw):
    """cvr_amg_default_options with the given fields replaced (max_levels, coarse_size, sweeps, strength, coarse_scale)"""
    o = AmgOptions()
    lib().cvr_amg_default_options(C.byref(o))
    for k, v in kw.items():
        if k not in dict(AmgOptions._fields_):
            raise TypeError(f"cvr_amg_options has no field {k}")
        setattr(o, k, v)
    return o


def _amg_setup(setup):
    """CVR_AMG_SETUP_* of Precond.amg_block's `setup`: a name of AMG_SETUPS, or the number itself"""
    if not isinstance(setup, str):
        return setup
    if setup not in AMG_SETUPS:
        raise ValueError(f"setup = {setup!r}: one of {sorted(AMG_SETUPS)}")
    return AMG_SETUPS[setup]


class AmgLevel:
    """one exported level: row_ptr, col_idx, vals, dinv, agg (None on the coarsest level) and winv (the n x n inverse of a directly solved coarsest
    level, else None)"""

    def __init__(self, n, rp, ci, va, dinv, agg, winv):
        self.n, self.rp, self.ci, self.va, self.dinv, self.agg, self.winv = n, rp, ci, va, dinv, agg, winv


def _amg_export(call, obj, info, level, dtype):
    """the arrays of one level through cvr_precond_amg_export_level or cvr_amg_hierarchy_export_level"""
    n, nnz, last = int(info.n[level]), int(info.nnz[level]), level == info.levels - 1
    rp, ci, va = np.zeros(n + 1, dtype=np.int64), np.zeros(nnz, dtype=np.int32), np.zeros(nnz, dtype=dtype)
    dinv = np.zeros(n, dtype=dtype)
    agg = None if last else np.zeros(n, dtype=np.int32)
    winv = np.zeros((n, n), dtype=dtype) if last and info.coarse_direct else None
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None          # noqa: E731
    rc = call(obj, level, rp.ctypes.data, ptr(ci), ptr(va), ptr(dinv), ptr(agg), ptr(winv))
    if rc:
        raise CvrError(rc, "cvr_amg export_level")
    return AmgLevel(n, rp, ci, va, dinv, agg, winv)


def amg_setup_host(rp, ci, vals, **options):
    """cvr_amg_setup_host: (AmgInfo, [AmgLevel, ...]) of the AMG hierarchy of a square CSR matrix with sorted rows and a diagonal in every row -- what
    Precond.amg builds, in host code (the type is vals' dtype, float32 or else float64; options as amg_options).  A diagonal entry or a pivot of the
    coarsest matrix that is not finite or not > 0 raises CvrError (ERR_STATE) with .bad = (level, row).  Host only."""
    return _amg_hierarchy_host("cvr_amg_setup_host", rp, ci, vals, options)


class AmgProlongator:
    """one exported prolongator P_l: n x nc in CSR (row_ptr, col_idx, vals)"""

    def __init__(self, n, nc, rp, ci, va):
        self.n, self.nc, self.rp, self.ci, self.va = n, nc, rp, ci, va


def _amg_export_prolongator(call, obj, info, sinfo, level, dtype):
    """P of one level through cvr_precond_amg_export_prolongator or cvr_amg_hierarchy_export_prolongator; the sizes from the two infos"""
    n, nnz = int(info.n[level]), int(sinfo.p_nnz[level])
    rp, ci, va = np.zeros(n + 1, dtype=np.int64), np.zeros(nnz, dtype=np.int32), np.zeros(nnz, dtype=dtype)
    rc = call(obj, level, rp.ctypes.data, ci.ctypes.data if nnz else None, va.ctypes.data if nnz else None)
    if rc:
        raise CvrError(rc, "cvr_amg export_prolongator")
    return AmgProlongator(n, int(info.n[level + 1]), rp, ci, va)


def amg_smoothed_setup_host(rp, ci, vals, omega=0.0, **options):
    """cvr_amg_smoothed_setup_host: (AmgInfo, AmgSmoothedInfo, [AmgLevel, ...], [AmgProlongator, ...]) of the smoothed-aggregation hierarchy of a
    square CSR matrix with sorted rows and a diagonal in every row -- what Precond.amg_smoothed builds, in host code.  omega = 0.0: the default 4/3.
    Errors as amg_setup_host.  Host only."""
    return _amg_hierarchy_host("cvr_amg_smoothed_setup_host", rp, ci, vals, options, omega)[:4]


def amg_mis2_setup_host(rp, ci, vals, omega=0.0, **options):
    """cvr_amg_mis2_setup_host: (AmgInfo, AmgSmoothedInfo, [AmgLevel, ...], [AmgProlongator, ...], AmgMis2Info) of the smoothed-aggregation hierarchy
    with the MIS(2) aggregation -- what Precond.amg_mis2 builds, in host code.  Errors as amg_smoothed_setup_host.  Host only."""
    return _amg_hierarchy_host("cvr_amg_mis2_setup_host", rp, ci, vals, options, omega)


def amg_mis2_aggregate_host(rp, ci, vals, strength=0.08):
    """cvr_amg_mis2_aggregate_host: (agg as int32, nc, rounds) of the MIS(2) aggregation of a square CSR matrix with sorted rows and a diagonal entry
    in every row.  Host only."""
    view, keep = _host_view(rp, ci, vals)
    agg, nc, rounds = np.full(view.nrows, -1, dtype=np.int32), C.c_int64(-1), C.c_int32(-1)
    rc = lib().cvr_amg_mis2_aggregate_host(C.byref(view), float(strength), agg.ctypes.data, C.byref(nc), C.byref(rounds))
    if rc:
        raise CvrError(rc, "cvr_amg_mis2_aggregate_host")
    return agg, nc.value, rounds.value


def amg_mis2_aggregate_device(n, row_ptr_dev, col_idx_dev, vals_dev, agg_dev, is_f32=False, strength=0.08, device=0, stream=None):
    """cvr_amg_mis2_aggregate_device: (nc, rounds); agg_dev receives n int32 values.  CSR arrays and agg_dev in the memory of `device` (raw pointers)"""
    nc, rounds = C.c_int64(-1), C.c_int32(-1)
    view = _device_view(n, row_ptr_dev, col_idx_dev, vals_dev, is_f32)
    rc = lib().cvr_amg_mis2_aggregate_device(C.byref(view), float(strength), agg_dev, C.byref(nc), C.byref(rounds), int(device), stream)
    if rc:
        raise CvrError(rc, "cvr_amg_mis2_aggregate_device")
    return nc.value, rounds.value


def _amg_hierarchy_host(entry, rp, ci, vals, options, *omega):
    """the host set-up through `entry` and everything its hierarchy exports: (info, levels) of cvr_amg_setup_host; with omega, of
    cvr_amg_smoothed_setup_host or cvr_amg_mis2_setup_host, (info, sinfo, levels, prolongators, minfo)"""
    view, keep = _host_view(rp, ci, vals)
    L, dtype = lib(), keep[2].dtype
    opt = amg_options(**options)
    h, bad_level, bad_row = C.c_void_p(), C.c_int32(-1), C.c_int64(-1)
    rc = getattr(L, entry)(C.byref(h), C.byref(view), C.byref(opt), *map(float, omega), C.byref(bad_level), C.byref(bad_row))
    if rc:
        e = CvrError(rc, entry)
        e.bad = (bad_level.value, bad_row.value) if bad_level.value >= 0 else None
        raise e
    try:
        info, sinfo, minfo = AmgInfo(), AmgSmoothedInfo(), AmgMis2Info()
        rc = L.cvr_amg_hierarchy_info(h, C.byref(info))
        if omega:
            rc = rc or L.cvr_amg_hierarchy_smoothed_info(h, C.byref(sinfo)) or L.cvr_amg_hierarchy_mis2_info(h, C.byref(minfo))
        if rc:
            raise CvrError(rc, "cvr_amg_hierarchy_info")
        levels = [_amg_export(L.cvr_amg_hierarchy_export_level, h, info, l, dtype) for l in range(info.levels)]
        if not omega:
            return info, levels
        return info, sinfo, levels, [_amg_export_prolongator(L.cvr_amg_hierarchy_export_prolongator, h, info, sinfo, l, dtype) for l in range(info.levels - 1)], minfo
    finally:
        L.cvr_amg_hierarchy_destroy(h)


def spgemm_host(a_csr, b_csr):
    """cvr_spgemm_host: (row_ptr, col_idx, vals) of C = A B for two (nrows, ncols, row_ptr, col_idx, vals) tuples of host arrays of one dtype (float32
    or else float64) -- what SpGemm computes on the device, in host code, by the two calls of the ABI.  B's rows must be strictly ascending in
    column: a violation raises CvrError (ERR_INVALID) with .bad_row.  Host only."""
    va_, keep_a = _host_view(*a_csr[2:], shape=a_csr[:2])
    vb_, keep_b = _host_view(*b_csr[2:], shape=b_csr[:2])
    m = va_.nrows
    crp, bad = np.zeros(m + 1, dtype=np.int64), C.c_int64(-1)

    def call(ci_ptr, va_ptr):
        rc = lib().cvr_spgemm_host(C.byref(va_), C.byref(vb_), crp.ctypes.data, ci_ptr, va_ptr, C.byref(bad))
        if rc:
            e = CvrError(rc, "cvr_spgemm_host")
            e.bad_row = None if bad.value < 0 else int(bad.value)
            raise e
    call(None, None)
    nnz = int(crp[m])
    cci, cva = np.zeros(max(nnz, 1), dtype=np.int32), np.zeros(max(nnz, 1), dtype=keep_a[2].dtype)
    call(cci.ctypes.data, cva.ctypes.data)
    return crp, cci[:nnz], cva[:nnz]


class SpGemm:
    """cvr_spgemm: C = A B in CSR on one GPU, bit for bit tests/spgemm_model.py.  The object owns C and copies of the two patterns."""

    def __init__(self):
        self._g = C.c_void_p()

    @classmethod
    def create(cls, a_csr, b_csr, device=0, stream=None):
        """from two (nrows, ncols, row_ptr, col_idx, vals) tuples of host arrays of one dtype; A may be unsorted with duplicates, B's rows must
        be strictly ascending in column"""
        va_, keep_a = _host_view(*a_csr[2:], shape=a_csr[:2])
        vb_, keep_b = _host_view(*b_csr[2:], shape=b_csr[:2])
        return cls._from_views(va_, vb_, device, stream)

    @classmethod
    def from_device(cls, a_dev, b_dev, is_f32=False, device=0, stream=None):
        """from two (nrows, ncols, row_ptr_dev, col_idx_dev, vals_dev) tuples of raw pointers into the memory of `device` (as CvrMatrix.from_device)"""
        va_ = CsrView(a_dev[0], a_dev[1], a_dev[2], a_dev[3], a_dev[4], int(bool(is_f32)), 1)
        vb_ = CsrView(b_dev[0], b_dev[1], b_dev[2], b_dev[3], b_dev[4], int(bool(is_f32)), 1)
        return cls._from_views(va_, vb_, device, stream)

    @classmethod
    def _from_views(cls, va_, vb_, device, stream):
        self = cls()
        rc = lib().cvr_spgemm_create(C.byref(self._g), C.byref(va_), C.byref(vb_), device, stream)
        if rc:
            self._g = C.c_void_p()
            raise CvrError(rc, "cvr_spgemm_create")
        self.dtype = np.float32 if self.info().is_f32 else np.float64
        return self

    def info(self):
        """cvr_spgemm_get_info: a SpGemmInfo"""
        info = SpGemmInfo()
        rc = lib().cvr_spgemm_get_info(self._g, C.byref(info))
        if rc:
            raise CvrError(rc, "cvr_spgemm_get_info")
        return info

    def csr_device(self):
        """cvr_spgemm_csr_device: (nrows, ncols, row_ptr_dev, col_idx_dev, vals_dev) of C, owned by this object: the arguments of
        CvrMatrix.from_device and of the *_from_device constructors"""
        v = CsrView()
        rc = lib().cvr_spgemm_csr_device(self._g, C.byref(v))
        if rc:
            raise CvrError(rc, "cvr_spgemm_csr_device")
        return v.nrows, v.ncols, v.row_ptr, v.col_idx, v.vals

    def export(self):
        """cvr_spgemm_export: (row_ptr, col_idx, vals) of C as host arrays"""
        i = self.info()
        rp, ci, va = np.zeros(i.nrows + 1, dtype=np.int64), np.zeros(i.nnz, dtype=np.int32), np.zeros(i.nnz, dtype=self.dtype)
        rc = lib().cvr_spgemm_export(self._g, rp.ctypes.data, ci.ctypes.data if i.nnz else None, va.ctypes.data if i.nnz else None)
        if rc:
            raise CvrError(rc, "cvr_spgemm_export")
        return rp, ci, va

    def numeric(self, a_vals_ptr, b_vals_ptr, stream=None):
        """cvr_spgemm_numeric_device: the numeric step again, asynchronously, with new device value arrays of A and B (same patterns, indexed like
        the arrays at creation), into the existing C"""
        rc = lib().cvr_spgemm_numeric_device(self._g, a_vals_ptr, b_vals_ptr, stream)
        if rc:
            raise CvrError(rc, "cvr_spgemm_numeric_device")

    def close(self):
        if getattr(self, "_g", None) and self._g.value:
            lib().cvr_spgemm_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def last_error():
    return lib().cvr_last_error().decode()


def version():
    return lib().cvr_version().decode()


def device_count():
    return lib().cvr_device_count()


def device_copy_gbs(device=0, nbytes=1 << 30, iters=20):
    """measured read+write rate of a streaming copy kernel (GB/s): the achievable-HBM yardstick"""
    g = C.c_double()
    rc = lib().cvr_device_copy_bench(device, nbytes, iters, C.byref(g))
    if rc:
        raise CvrError(rc, "cvr_device_copy_bench")
    return g.value


class SourceKey(C.Structure):
    _fields_ = [("size", C.c_int64), ("mtime_ns", C.c_int64), ("hash", C.c_uint64), ("mode", C.c_int32), ("reserved", C.c_int32)]


def source_key(path, mode=MM_REFCOMPAT):
    k = SourceKey()
    rc = lib().cvr_source_key_of(os.fsencode(path), mode, C.byref(k))
    if rc:
        raise CvrError(rc, f"cvr_source_key_of({path})")
    return k


def load_mm(path, mode=MM_REFCOMPAT, cache=None):
    """cvr_mm_read -> dict(nrows, ncols, nnz, ref_*, row_ptr int64, col_idx int32, vals float64) (numpy copies).
    cache=True: through the keyed cache beside the file (cvr_mm_read_cached: <path>.ref.csrbin / .strict.csrbin, read only while
    its key -- size, mtime, hash of the first and last MiB -- is the file's); out["cache_hit"] says which.
    cache=<path>: an UNKEYED binary image; read when it exists, written after a text parse otherwise (the caller answers for
    its freshness)."""
    m = MmMatrix()
    hit = None
    if cache is True:
        h = C.c_int()
        rc = lib().cvr_mm_read_cached(os.fsencode(path), mode, C.byref(m), C.byref(h))
        if rc:
            raise CvrError(rc, f"cvr_mm_read_cached({path})")
        hit = bool(h.value)
    elif cache and os.path.exists(cache):
        rc = lib().cvr_mm_read_bin(os.fsencode(cache), C.byref(m))
        if rc:
            raise CvrError(rc, f"cvr_mm_read_bin({cache})")
    else:
        rc = lib().cvr_mm_read(os.fsencode(path), mode, C.byref(m))
        if rc:
            raise CvrError(rc, f"cvr_mm_read({path})")
        if cache and lib().cvr_mm_write_bin(os.fsencode(cache), C.byref(m)):
            raise CvrError(ERR_IO, f"cvr_mm_write_bin({cache})")
    n = max(m.ref_nItems, m.nnz)
    out = dict(nrows=m.nrows, ncols=m.ncols, nnz=m.nnz, ref_numRows=m.ref_numRows, ref_numCols=m.ref_numCols,
               ref_nItems=m.ref_nItems, ref_nItemsRaw=m.ref_nItemsRaw,
               row_ptr=np.ctypeslib.as_array(m.row_ptr, shape=(m.nrows + 1,)).copy(),
               col_idx=np.ctypeslib.as_array(m.col_idx, shape=(max(n, 1),))[:n].copy(),
               vals=np.ctypeslib.as_array(m.vals, shape=(max(n, 1),))[:n].copy())
    lib().cvr_mm_free(C.byref(m))
    if hit is not None:
        out["cache_hit"] = hit
    return out


def sym_eig_host(a, vectors=True):
    """all eigenpairs of the symmetric matrix a (m x m, m <= EIG_MAX_NCV) by cvr_sym_eig_host: only a[i, j] with i >= j is read.  Returns (w ascending,
    Z with the eigenvector of w[c] in column c), or w alone without vectors."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError("a must be a square matrix")
    m = a.shape[0]
    col = np.asfortranarray(a)          # element (i, j) at i + j * m
    w = np.zeros(max(m, 1))
    z = np.zeros((m, m), order="F") if vectors else None
    rc = lib().cvr_sym_eig_host(m, col.ctypes.data, max(m, 1), w.ctypes.data, None if z is None else z.ctypes.data, max(m, 1))
    if rc:
        raise CvrError(rc, "cvr_sym_eig_host")
    return (w[:m], z) if vectors else w[:m]


def svd_host(b, vectors=True):
    """the singular value decomposition of b (p x q, p <= q <= SVD_MAX_NCV + 1) by cvr_svd_host.  Returns (s descending, Q of shape (p, p), P of shape
    (q, p)) with b = Q diag(s) P^T, or s alone without vectors."""
    b = np.asarray(b, dtype=np.float64)
    if b.ndim != 2:
        raise ValueError("b must be a matrix")
    p, q = b.shape
    col = np.asfortranarray(b)          # element (i, j) at i + j * p
    s = np.zeros(max(p, 1))
    Q = np.zeros((p, p), order="F") if vectors else None
    P = np.zeros((q, p), order="F") if vectors else None
    rc = lib().cvr_svd_host(p, q, col.ctypes.data, max(p, 1), s.ctypes.data, None if Q is None else Q.ctypes.data, max(p, 1),
                            None if P is None else P.ctypes.data, max(q, 1))
    if rc:
        raise CvrError(rc, "cvr_svd_host")
    return (s[:p], Q, P) if vectors else s[:p]


def fill_x(n, mode=0):
    x = np.empty(n, dtype=np.float64)
    lib().cvr_fill_x(x.ctypes.data, n, mode)
    return x


def csr_spmv_host(row_ptr, col_idx, vals, x, nthreads=1):
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
    ci = np.ascontiguousarray(col_idx, dtype=np.int32)
    va = np.ascontiguousarray(vals, dtype=np.float64)
    xx = np.ascontiguousarray(x, dtype=np.float64)
    y = np.zeros(len(rp) - 1, dtype=np.float64)
    lib().cvr_csr_spmv_host(len(rp) - 1, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, xx.ctypes.data, y.ctypes.data, nthreads)
    return y


def verdict(y, yref, n):
    y = np.ascontiguousarray(y, dtype=np.float64)
    yref = np.ascontiguousarray(yref, dtype=np.float64)
    return lib().cvr_verdict(y.ctypes.data, yref.ctypes.data, n)


def plan_chunks(row_ptr, S, thr=0):
    """host planner only (runs without a GPU): dict(nz_begin[n+1], row_first[n], nseg[n], pad_cnt[n])"""
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
    nrows = len(rp) - 1
    bound = lib().cvr_plan_bound(nrows, int(rp[-1] - rp[0]) if nrows else 0, S)
    nzb = np.zeros(bound + 1, dtype=np.int64)
    rf, ns, pc = (np.zeros(bound, dtype=np.int64) for _ in range(3))
    n = lib().cvr_plan_chunks(nrows, rp.ctypes.data, S, thr, nzb.ctypes.data, rf.ctypes.data, ns.ctypes.data, pc.ctypes.data)
    if n < 0:
        raise CvrError(n, "cvr_plan_chunks")
    return dict(nz_begin=nzb[: n + 1].copy(), row_first=rf[:n].copy(), nseg=ns[:n].copy(), pad_cnt=pc[:n].copy())


def plan_selfcheck(row_ptr, S, thr=0, max_rows=0, device=0):
    """plans row_ptr on the device and on the host and compares the plans field by field (raises CvrError if they differ);
    returns dict(host_s, device_s, nchunks)"""
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
    hs, ds, n = C.c_double(), C.c_double(), C.c_int64()
    rc = lib().cvr_plan_selfcheck(device, len(rp) - 1, rp.ctypes.data, S, thr, max_rows, C.addressof(hs), C.addressof(ds), C.addressof(n))
    if rc:
        raise CvrError(rc, "cvr_plan_selfcheck")
    return dict(host_s=hs.value, device_s=ds.value, nchunks=n.value)


def power_step_selfcheck(n, is_f32, x_ptr, y_ptr, partial_ptr, prev_ptr=None, bounds=None, max_rows=0, dense_ptr=None, stream=None, device=0):
    """one power-iteration step's vector work on the caller's device arrays (cvr_power_step_selfcheck): x_ptr is updated in place, partial_ptr
    (3 * 1024 doubles) receives the step's partial sums; bounds (nparts + 1 row offsets): y_ptr is the padded all-gather layout of nparts * max_rows
    values and dense_ptr, if given, receives y in row order.  Returns the sums (x.y, y.y, x.x) as three float64."""
    b = None if bounds is None else np.ascontiguousarray(bounds, dtype=np.int64)
    sums = np.zeros(3, dtype=np.float64)
    rc = lib().cvr_power_step_selfcheck(device, n, int(is_f32), x_ptr, y_ptr, prev_ptr, partial_ptr, None if b is None else b.ctypes.data,
                                        0 if b is None else len(b) - 1, max_rows, dense_ptr, sums.ctypes.data, stream)
    if rc:
        raise CvrError(rc, "cvr_power_step_selfcheck")
    return sums


def auto_panels(nrows, ncols, row_ptr, col_idx, is_f32=False):
    """(column panels cvr_create would choose, estimated L2 miss share of the x gathers); host only"""
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
    ci = np.ascontiguousarray(col_idx, dtype=np.int32)
    view = CsrView(nrows, ncols, rp.ctypes.data, ci.ctypes.data, None, int(is_f32))
    miss = C.c_double()
    P = lib().cvr_auto_panels(C.byref(view), C.byref(miss))
    if P < 0:
        raise CvrError(P, "cvr_auto_panels")
    return P, miss.value


COMM_ID_BYTES = 128


def comm_unique_id():
    """128 bytes from rank 0 that every rank passes to Comm() (hand them over with torch.distributed, a file, ...)"""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = lib().cvr_comm_unique_id(buf)
    if rc:
        raise CvrError(rc, "cvr_comm_unique_id")
    return buf.raw


class Comm:
    """RCCL communicator of the row-sharded SpMV, one rank per process and GPU (cvr_comm_create; collective)"""

    def __init__(self, unique_id, nranks, rank, device):
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError("unique_id must be the 128 bytes of comm_unique_id()")
        self._c = C.c_void_p()
        self.nranks, self.rank, self.device = nranks, rank, device
        rc = lib().cvr_comm_create(C.byref(self._c), unique_id, nranks, rank, device)
        if rc:
            raise CvrError(rc, "cvr_comm_create")

    def info(self):
        """(ranks, this rank, RCCL version) as the library reports them for this communicator (cvr_comm_info); -1 where it cannot say"""
        n, r, v = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        rc = lib().cvr_comm_info(self._c, C.byref(n), C.byref(r), C.byref(v))
        if rc:
            raise CvrError(rc, "cvr_comm_info")
        return n.value, r.value, v.value

    def all_gather(self, send_ptr, recv_ptr, count, is_f32=False, stream=None):
        rc = lib().cvr_comm_all_gather(self._c, send_ptr, recv_ptr, count, int(is_f32), stream)
        if rc:
            raise CvrError(rc, "cvr_comm_all_gather")

    def close(self):
        if self._c:
            lib().cvr_comm_destroy(self._c)
            self._c = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Precond:
    """A preconditioner the library owns (cvr_precond): built once, applied on the device, handed to CvrMatrix.pcg()."""

    def __init__(self):
        self._p = C.c_void_p()
        self.info = PrecondInfo()

    @classmethod
    def _build(cls, entry, *args, matrix=None):
        """the object of one constructor of the ABI, entry(&p, *args).  A view among args points into arrays its maker returned beside it (_host_view's
        `keep`): the calling constructor holds them in a local until this returns.  matrix: the CvrMatrix the object borrows, kept alive with it."""
        self = cls()
        rc = getattr(lib(), entry)(C.byref(self._p), *args)
        if rc:
            self._p = C.c_void_p()
            raise CvrError(rc, entry)
        lib().cvr_precond_get_info(self._p, C.byref(self.info))
        self.dtype = np.float32 if self.info.is_f32 else np.float64
        if matrix is not None:
            self._matrix = matrix
        return self

    def _info(self, entry, struct_type):
        """one info call of the ABI, entry(p, &info): the filled struct_type"""
        info = struct_type()
        rc = getattr(lib(), entry)(self._p, C.byref(info))
        if rc:
            raise CvrError(rc, entry)
        return info

    @classmethod
    def block_jacobi(cls, rp, ci, vals, block_size, device=0):
        """cvr_precond_block_jacobi from host CSR arrays of a square matrix (n = len(rp) - 1; the type is vals' dtype, float32 or else float64)"""
        view, keep = _host_view(rp, ci, vals)
        return cls._build("cvr_precond_block_jacobi", C.byref(view), int(block_size), int(device), None)

    @classmethod
    def block_jacobi_from_device(cls, n, row_ptr_dev, col_idx_dev, vals_dev, block_size, is_f32=False, device=0):
        """the same from CSR arrays in the memory of `device` (raw pointers, as CvrMatrix.from_device)"""
        view = _device_view(n, row_ptr_dev, col_idx_dev, vals_dev, is_f32)
        return cls._build("cvr_precond_block_jacobi", C.byref(view), int(block_size), int(device), None)

    @classmethod
    def chebyshev(cls, matrix, degree, lmin, lmax):
        """cvr_precond_chebyshev: z = p_degree(A) r, the Chebyshev polynomial for a spectrum in [lmin, lmax], applied through `matrix`'s own SpMV.  The
        object borrows the CvrMatrix (kept alive here; close the object before the matrix) and serves one stream at a time."""
        return cls._build("cvr_precond_chebyshev", matrix._h, int(degree), float(lmin), float(lmax), matrix=matrix)

    def chebyshev_info(self):
        """cvr_precond_chebyshev_info: dict(degree, is_f32, lmin, lmax, a, b) with the degree coefficients a[k], b[k] (a[0] = 0, b[0] = c0) as fp64 arrays"""
        ci = self._info("cvr_precond_chebyshev_info", ChebyshevInfo)
        return dict(degree=ci.degree, is_f32=ci.is_f32, lmin=ci.lmin, lmax=ci.lmax, a=np.array(ci.a[: ci.degree], dtype=np.float64),
                    b=np.array(ci.b[: ci.degree], dtype=np.float64))

    @classmethod
    def ilu0(cls, rp, ci, vals, device=0):
        """cvr_precond_ilu0 from host CSR arrays of a square matrix whose rows are sorted, without duplicates and with a diagonal entry each
        (n = len(rp) - 1; the type is vals' dtype, float32 or else float64).  Serves one stream at a time."""
        view, keep = _host_view(rp, ci, vals)
        return cls._build("cvr_precond_ilu0", C.byref(view), int(device), None)

    @classmethod
    def ilu0_from_device(cls, n, row_ptr_dev, col_idx_dev, vals_dev, is_f32=False, device=0):
        """the same from CSR arrays in the memory of `device` (raw pointers, as CvrMatrix.from_device)"""
        view = _device_view(n, row_ptr_dev, col_idx_dev, vals_dev, is_f32)
        return cls._build("cvr_precond_ilu0", C.byref(view), int(device), None)

    @classmethod
    def ilu0_jacobi(cls, rp, ci, vals, sweeps, device=0):
        """cvr_precond_ilu0_jacobi from host CSR arrays, read as Precond.ilu0 reads them: the same ILU(0) factors, each triangular solve of the apply
        replaced by `sweeps` (1 .. ILU0_MAX_SWEEPS) Jacobi sweeps -- 2 * sweeps launches per apply whatever the level structure.  Kind 2: pcg,
        pbicgstab and pgmres take it as they take Precond.ilu0's.  Serves one stream at a time."""
        view, keep = _host_view(rp, ci, vals)
        return cls._build("cvr_precond_ilu0_jacobi", C.byref(view), int(sweeps), int(device), None)

    @classmethod
    def ilu0_jacobi_from_device(cls, n, row_ptr_dev, col_idx_dev, vals_dev, sweeps, is_f32=False, device=0):
        """the same from CSR arrays in the memory of `device` (raw pointers, as CvrMatrix.from_device)"""
        view = _device_view(n, row_ptr_dev, col_idx_dev, vals_dev, is_f32)
        return cls._build("cvr_precond_ilu0_jacobi", C.byref(view), int(sweeps), int(device), None)

    def ilu0_jacobi_info(self):
        """cvr_precond_ilu0_jacobi_info: an Ilu0JacobiInfo (n, nnz, sweeps, launches_per_apply, lanes_per_row, levels_*, is_f32)"""
        return self._info("cvr_precond_ilu0_jacobi_info", Ilu0JacobiInfo)

    def ilu0_info(self):
        """cvr_precond_ilu0_info: an Ilu0Info (n, nnz, levels_*, launches_*, max_level_width, lanes_per_row, wide_threshold, is_f32)"""
        return self._info("cvr_precond_ilu0_info", Ilu0Info)

    def ilu0_export(self):
        """cvr_precond_ilu0_export: nnz values of the object's dtype in the CSR's own positions -- L strictly below the diagonal (without its unit
        diagonal), U from the diagonal up"""
        out = np.zeros(self.ilu0_info().nnz, dtype=self.dtype)
        if out.size:
            rc = lib().cvr_precond_ilu0_export(self._p, out.ctypes.data)
            if rc:
                raise CvrError(rc, "cvr_precond_ilu0_export")
        return out

    @classmethod
    def mcsgs(cls, rp, ci, vals, device=0):
        """cvr_precond_mcsgs from host CSR arrays of a square matrix whose rows are sorted, without duplicates and with a diagonal entry each, and
        whose off-diagonal pattern is structurally symmetric (n = len(rp) - 1; the type is vals' dtype, float32 or else float64): multicolour
        symmetric Gauss-Seidel, 2 * ncolors launches per apply.  Serves one stream at a time."""
        view, keep = _host_view(rp, ci, vals)
        return cls._build("cvr_precond_mcsgs", C.byref(view), int(device), None)

    @classmethod
    def mcsgs_from_device(cls, n, row_ptr_dev, col_idx_dev, vals_dev, is_f32=False, device=0):
        """the same from CSR arrays in the memory of `device` (raw pointers, as CvrMatrix.from_device)"""
        view = _device_view(n, row_ptr_dev, col_idx_dev, vals_dev, is_f32)
        return cls._build("cvr_precond_mcsgs", C.byref(view), int(device), None)

    def mcsgs_info(self):
        """cvr_precond_mcsgs_info: a McSgsInfo (n, nnz, ncolors, rounds, launches_per_apply, lanes_per_row, max_color_rows, min_color_rows, is_f32)"""
        return self._info("cvr_precond_mcsgs_info", McSgsInfo)

    def mcsgs_export(self):
        """cvr_precond_mcsgs_export: (color, perm, color_ptr) of the object's colouring as int32 arrays"""
        i = self.mcsgs_info()
        color, perm, ptr = np.zeros(max(i.n, 1), dtype=np.int32), np.zeros(max(i.n, 1), dtype=np.int32), np.zeros(i.ncolors + 1, dtype=np.int32)
        rc = lib().cvr_precond_mcsgs_export(self._p, color.ctypes.data, perm.ctypes.data, ptr.ctypes.data)
        if rc:
            raise CvrError(rc, "cvr_precond_mcsgs_export")
        return color[: i.n], perm[: i.n], ptr

    @classmethod
    def fsai(cls, rp, ci, vals, device=0):
        """cvr_precond_fsai from host CSR arrays of a symmetric positive definite matrix whose rows are sorted, without duplicates and with a
        diagonal entry each; only the entries with column <= row are read (n = len(rp) - 1; the type is vals' dtype, float32 or else float64).
        Serves one stream at a time."""
        view, keep = _host_view(rp, ci, vals)
        return cls._build("cvr_precond_fsai", C.byref(view), int(device), None)

    @classmethod
    def fsai_from_device(cls, n, row_ptr_dev, col_idx_dev, vals_dev, is_f32=False, device=0):
        """the same from CSR arrays in the memory of `device` (raw pointers, as CvrMatrix.from_device)"""
        view = _device_view(n, row_ptr_dev, col_idx_dev, vals_dev, is_f32)
        return cls._build("cvr_precond_fsai", C.byref(view), int(device), None)

    def fsai_info(self):
        """cvr_precond_fsai_info: an FsaiInfo (n, nnz of W, max_row, lanes_per_row, truncated_rows, is_f32)"""
        return self._info("cvr_precond_fsai_info", FsaiInfo)

    def fsai_export(self):
        """cvr_precond_fsai_export: (row_ptr, col_idx, wa, wb) of W -- its own CSR pattern (A's lower triangle, a row's CVR_FSAI_MAX_ROW entries
        nearest the diagonal at most) and the two value arrays of the object's dtype: z = Wb^T (Wa r)"""
        i = self.fsai_info()
        rp, ci = np.zeros(i.n + 1, dtype=np.int64), np.zeros(i.nnz, dtype=np.int32)
        wa, wb = np.zeros(i.nnz, dtype=self.dtype), np.zeros(i.nnz, dtype=self.dtype)
        rc = lib().cvr_precond_fsai_export(self._p, rp.ctypes.data, ci.ctypes.data if i.nnz else None, wa.ctypes.data if i.nnz else None,
                                           wb.ctypes.data if i.nnz else None)
        if rc:
            raise CvrError(rc, "cvr_precond_fsai_export")
        return rp, ci, wa, wb

    @classmethod
    def amg(cls, matrix, rp, ci, vals, **options):
        """cvr_precond_amg: one V-cycle of plain aggregation AMG for the symmetric positive definite `matrix` (a CvrMatrix, borrowed for level 0's
        products and kept alive here; close the object before the matrix), from host CSR arrays of the same matrix whose rows are sorted, without
        duplicates and with a diagonal entry each.  options: max_levels, coarse_size, sweeps, strength, coarse_scale.  Serves one stream at a time."""
        view, keep = _host_view(rp, ci, vals)
        opt = amg_options(**options)
        return cls._build("cvr_precond_amg", matrix._h, C.byref(view), C.byref(opt), None, matrix=matrix)

    @classmethod
    def amg_from_device(cls, matrix, n, row_ptr_dev, col_idx_dev, vals_dev, is_f32=False, **options):
        """the same from CSR arrays in the memory of the matrix's device (raw pointers, as CvrMatrix.from_device)"""
        view, opt = _device_view(n, row_ptr_dev, col_idx_dev, vals_dev, is_f32), amg_options(**options)
        return cls._build("cvr_precond_amg", matrix._h, C.byref(view), C.byref(opt), None, matrix=matrix)

    @classmethod
    def amg_smoothed(cls, matrix, rp, ci, vals, omega=0.0, **options):
        """cvr_precond_amg_smoothed: Precond.amg with the smoothed prolongator P = (I - omega D^-1 A) T and the Galerkin coarse operators P^T A P,
        built on the device by the SpGEMM; omega = 0.0: the default 4/3, else 0 < omega < 2.  The same kind of object (kind 4) for the same calls."""
        view, keep = _host_view(rp, ci, vals)
        opt = amg_options(**options)
        return cls._build("cvr_precond_amg_smoothed", matrix._h, C.byref(view), C.byref(opt), float(omega), None, matrix=matrix)

    @classmethod
    def amg_smoothed_from_device(cls, matrix, n, row_ptr_dev, col_idx_dev, vals_dev, is_f32=False, omega=0.0, **options):
        """the same from CSR arrays in the memory of the matrix's device (raw pointers, as CvrMatrix.from_device)"""
        view, opt = _device_view(n, row_ptr_dev, col_idx_dev, vals_dev, is_f32), amg_options(**options)
        return cls._build("cvr_precond_amg_smoothed", matrix._h, C.byref(view), C.byref(opt), float(omega), None, matrix=matrix)

    @classmethod
    def amg_mis2(cls, matrix, rp, ci, vals, omega=0.0, **options):
        """cvr_precond_amg_mis2: Precond.amg_smoothed with the MIS(2) aggregation, the whole level loop on the device; the same kind of object
        (kind 4, smoothed) for the same calls."""
        view, keep = _host_view(rp, ci, vals)
        opt = amg_options(**options)
        return cls._build("cvr_precond_amg_mis2", matrix._h, C.byref(view), C.byref(opt), float(omega), None, matrix=matrix)

    @classmethod
    def amg_mis2_from_device(cls, matrix, n, row_ptr_dev, col_idx_dev, vals_dev, is_f32=False, omega=0.0, **options):
        """the same from CSR arrays in the memory of the matrix's device (raw pointers, as CvrMatrix.from_device)"""
        view, opt = _device_view(n, row_ptr_dev, col_idx_dev, vals_dev, is_f32), amg_options(**options)
        return cls._build("cvr_precond_amg_mis2", matrix._h, C.byref(view), C.byref(opt), float(omega), None, matrix=matrix)

    @classmethod
    def amg_block(cls, matrix, rp, ci, vals, nvec, setup="plain", omega=0.0, **options):
        """cvr_precond_amg_block: the kind-4 object of Precond.amg (setup="plain"; omega is ignored), Precond.amg_smoothed ("smoothed") or
        Precond.amg_mis2 ("mis2") -- the same hierarchy byte for byte -- built for blocks of up to nvec = K columns, 1 .. 8: apply_multi and
        CvrMatrix.pcg_multi / pcg_multi_host take it for 1 <= nvec <= K, one V-cycle for all columns.  For K >= 2 `matrix` must have the plain
        layout (nvec >= 2 at creation).  apply, pcg and pcg_host take it as any kind-4 object."""
        view, keep = _host_view(rp, ci, vals)
        opt, setup = amg_options(**options), _amg_setup(setup)
        return cls._build("cvr_precond_amg_block", matrix._h, C.byref(view), C.byref(opt), int(setup), float(omega), int(nvec), None, matrix=matrix)

    @classmethod
    def amg_block_from_device(cls, matrix, n, row_ptr_dev, col_idx_dev, vals_dev, nvec, is_f32=False, setup="plain", omega=0.0, **options):
        """the same from CSR arrays in the memory of the matrix's device (raw pointers, as CvrMatrix.from_device)"""
        view, opt, setup = _device_view(n, row_ptr_dev, col_idx_dev, vals_dev, is_f32), amg_options(**options), _amg_setup(setup)
        return cls._build("cvr_precond_amg_block", matrix._h, C.byref(view), C.byref(opt), int(setup), float(omega), int(nvec), None, matrix=matrix)

    def amg_block_info(self):
        """cvr_precond_amg_block_info: an AmgBlockInfo (nvec = K, setup, buffer_bytes); CvrError on an object built another way"""
        return self._info("cvr_precond_amg_block_info", AmgBlockInfo)

    def amg_mis2_info(self):
        """cvr_precond_amg_mis2_info: an AmgMis2Info (mis2, the MIS rounds of every level); all zero of a kind-4 object built another way"""
        return self._info("cvr_precond_amg_mis2_info", AmgMis2Info)

    def amg_smoothed_info(self):
        """cvr_precond_amg_smoothed_info: an AmgSmoothedInfo (smoothed, omega, products_per_apply, p_nnz of every level); all zero of a plain object"""
        return self._info("cvr_precond_amg_smoothed_info", AmgSmoothedInfo)

    def amg_export_prolongator(self, level):
        """cvr_precond_amg_export_prolongator: an AmgProlongator (row_ptr, col_idx, vals of P_l, n x nc) of level 0 .. levels - 2"""
        return _amg_export_prolongator(lib().cvr_precond_amg_export_prolongator, self._p, self.amg_info(), self.amg_smoothed_info(), level, self.dtype)

    def amg_info(self):
        """cvr_precond_amg_info: an AmgInfo (levels, coarse_direct, the options, operator_complexity, n and nnz of every level)"""
        return self._info("cvr_precond_amg_info", AmgInfo)

    def amg_export_level(self, level):
        """cvr_precond_amg_export_level: an AmgLevel (row_ptr, col_idx, vals, dinv, agg, winv) of level 0 .. levels - 1"""
        return _amg_export(lib().cvr_precond_amg_export_level, self._p, self.amg_info(), level, self.dtype)

    def export(self):
        """the inverse blocks W as an array of shape (nblocks, block_size, block_size) of the object's dtype, each block row-major"""
        bs = self.info.block_size
        out = np.zeros((self.info.nblocks, bs, bs), dtype=self.dtype)
        if out.size:
            rc = lib().cvr_precond_export(self._p, out.ctypes.data)
            if rc:
                raise CvrError(rc, "cvr_precond_export")
        return out

    def apply(self, r_ptr, z_ptr, stream=None):
        """asynchronous z = M^-1 r on device arrays of n values (cvr_precond_apply_device); r_ptr != z_ptr"""
        rc = lib().cvr_precond_apply_device(self._p, r_ptr, z_ptr, stream)
        if rc:
            raise CvrError(rc, "cvr_precond_apply_device")

    def apply_multi(self, R_ptr, ldr, Z_ptr, ldz, nvec, stream=None):
        """asynchronous Z = M^-1 R on row-major device blocks of n rows of ldr / ldz values, 1 <= nvec <= 8 columns
        (cvr_precond_apply_multi_device); column c of Z is bit for bit apply()'s z for column c of R; the blocks must not overlap.  Takes
        block-Jacobi objects and, for nvec up to the width they were built for, Precond.amg_block's"""
        rc = lib().cvr_precond_apply_multi_device(self._p, R_ptr, ldr, Z_ptr, ldz, nvec, stream)
        if rc:
            raise CvrError(rc, "cvr_precond_apply_multi_device")

    def close(self):
        if getattr(self, "_p", None) and self._p.value:
            lib().cvr_precond_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def _which(which):
    """EIG_LARGEST / EIG_SMALLEST of an eigensolver's `which`"""
    try:
        return {"LA": EIG_LARGEST, "SA": EIG_SMALLEST}[which]
    except KeyError:
        raise ValueError(f"which = {which!r}: must be 'LA' or 'SA'") from None


def _returned_count(res, nev):
    """how many pairs or triplets an EigResult / SvdResult stands for: nev, less at EIG_INVARIANT (nconv) and 0 at EIG_BREAKDOWN"""
    return 0 if res.status == EIG_BREAKDOWN else res.nconv if res.status == EIG_INVARIANT else int(nev)


class CvrMatrix:
    """One matrix (or row shard) resident on one GPU: cvr_create + cvr_preprocess, then spmv()."""

    def __init__(self, nrows, ncols, row_ptr, col_idx, vals, device=0, steps_per_chunk=0, split_threshold=0,
                 xcd_swizzle=-1, x_window=-1, keep_csr=False, debug_col_mask=0,
                 col_panels=-1, value_dict=-1, tune_steps=False, waves_per_block=0, col_phases=-1, hub_table=-1, narrow_cols=-1, hub_reorder=-1,
                 row_tags16=-1, row_bands=-1, piece_max=-1, interleave=-1, gang=-1, nvec=0, mutable_values=0, transpose=0):
        """transpose=1: the handle of A^T, built on the device from this CSR of A (cvr_options.transpose): nrows / ncols of the object are
        A's ncols / nrows, x has nrows(A) values, y ncols(A); update_values takes values indexed like A's vals.
        mutable_values=1: the handle takes new values of the same pattern later (update_values, update_values_device; no value dictionary).
        tune_steps: choose steps_per_chunk by measurement first (cvr_tune_steps; its cost is self.tuning_s).
        nvec >= 2: the plain layout, for spmm() / spmm_device() with up to that many vectors at once (cvr_options.nvec).
        debug_col_mask is a profiling knob (tools/sweep.py): it travels through the environment (CVR_DEBUG_COL_MASK), not through cvr_options."""
        self._h = C.c_void_p()
        self.tuning_s = 0.0
        rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
        ci = np.ascontiguousarray(col_idx, dtype=np.int32)
        self.f32 = np.asarray(vals).dtype == np.float32
        self.dtype = np.float32 if self.f32 else np.float64
        va = np.ascontiguousarray(vals, dtype=self.dtype)
        if len(rp) != nrows + 1:
            raise ValueError("row_ptr must have nrows + 1 entries")
        if nrows > 0 and rp[0] < 0:
            raise ValueError("row_ptr[0] < 0")
        if nrows > 0 and (len(ci) < rp[-1] or len(va) < rp[-1]):      # the library reads row_ptr[nrows] entries of both
            raise ValueError(f"col_idx / vals hold {len(ci)} / {len(va)} entries, row_ptr[nrows] = {int(rp[-1])}")
        view = CsrView(nrows, ncols, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, int(self.f32))
        self._build(view, nrows, ncols, device, steps_per_chunk, split_threshold, xcd_swizzle, x_window, keep_csr,
                    debug_col_mask, col_panels, value_dict, tune_steps, waves_per_block, col_phases, hub_table, narrow_cols, hub_reorder,
                    row_tags16, row_bands, piece_max, interleave, gang, nvec, mutable_values, transpose)

    def save_image(self, path, key=None):
        """cvr_save_image: the converted image on disk, keyed by `key` (capi.source_key of the .mtx file; None = no source key),
        the options and the device geometry"""
        rc = lib().cvr_save_image(self._h, os.fsencode(path), C.byref(key) if key is not None else None)
        if rc:
            raise CvrError(rc, "cvr_save_image")

    @classmethod
    def from_image(cls, path, key=None, device=0, nvec=0, mutable_values=0, transpose=0, **options):
        """cvr_load_image: a handle from a saved image (CvrError with code ERR_STATE when the file was written for another source,
        other options -- nvec among them --, another device geometry or library version)"""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        self.tuning_s = 0.0
        opt = Options()
        lib().cvr_default_options(C.byref(opt))
        opt.device = device
        opt.nvec = nvec
        opt.mutable_values = mutable_values
        opt.transpose = transpose
        for k, v in options.items():
            setattr(opt, k, v)
        sec = C.c_double()
        rc = lib().cvr_load_image(C.byref(self._h), os.fsencode(path), C.byref(key) if key is not None else None, C.byref(opt), C.byref(sec))
        if rc:
            self._h = C.c_void_p()
            raise CvrError(rc, "cvr_load_image")
        self.load_s = self.preprocess_s = sec.value
        self.info = Info()
        lib().cvr_get_info(self._h, C.byref(self.info))
        self.nrows, self.ncols = self.info.nrows, self.info.ncols
        self.f32 = bool(self.info.is_f32)
        self.dtype = np.float32 if self.f32 else np.float64
        return self

    @classmethod
    def from_device(cls, nrows, ncols, row_ptr_dev, col_idx_dev, vals_dev, is_f32=False, device=0, steps_per_chunk=0,
                    split_threshold=0, keep_csr=False, col_panels=-1, value_dict=-1, tune_steps=False, hub_table=-1, hub_reorder=-1, interleave=-1, gang=-1, nvec=0, mutable_values=0,
                    transpose=0):
        """CSR arrays already in the memory of `device` (raw pointers: int64 row_ptr[nrows+1], int32 col_idx, fp64/fp32 vals),
        e.g. the .data_ptr() of torch tensors: cvr_csr_view.arrays_on_device = 1 (transpose=1: the handle of A^T, as in __init__)"""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        self.tuning_s = 0.0
        self.f32 = bool(is_f32)
        self.dtype = np.float32 if self.f32 else np.float64
        view = CsrView(nrows, ncols, row_ptr_dev, col_idx_dev, vals_dev, int(self.f32), 1)
        self._build(view, nrows, ncols, device, steps_per_chunk, split_threshold, -1, -1, keep_csr, 0, col_panels, value_dict, tune_steps,
                    hub_table=hub_table, hub_reorder=hub_reorder, interleave=interleave, gang=gang, nvec=nvec, mutable_values=mutable_values,
                    transpose=transpose)
        return self

    def _build(self, view, nrows, ncols, device, steps_per_chunk, split_threshold, xcd_swizzle, x_window, keep_csr,
               debug_col_mask, col_panels, value_dict, tune_steps, waves_per_block=0, col_phases=-1, hub_table=-1, narrow_cols=-1, hub_reorder=-1,
               row_tags16=-1, row_bands=-1, piece_max=-1, interleave=-1, gang=-1, nvec=0, mutable_values=0, transpose=0):
        opt = Options()
        lib().cvr_default_options(C.byref(opt))
        opt.device, opt.steps_per_chunk, opt.split_threshold = device, steps_per_chunk, split_threshold
        opt.xcd_swizzle, opt.x_window, opt.col_panels, opt.value_dict = xcd_swizzle, x_window, col_panels, value_dict
        opt.waves_per_block, opt.col_phases, opt.hub_table, opt.narrow_cols = waves_per_block, col_phases, hub_table, narrow_cols
        opt.hub_reorder, opt.row_tags16, opt.row_bands, opt.piece_max = hub_reorder, row_tags16, row_bands, piece_max
        opt.interleave = interleave
        opt.gang = gang
        opt.nvec = nvec
        opt.mutable_values = mutable_values
        opt.transpose = transpose
        # profiling knobs (tools/sweep.py): cvr_create / cvr_tune read them from the environment.  Only a knob the caller passed is
        # touched, and what the environment held before comes back once the handle exists (a value the user exported stays theirs).
        saved = {}
        for name, val in (("CVR_DEBUG_COL_MASK", debug_col_mask),):
            if val:
                saved[name] = os.environ.get(name)
                os.environ[name] = str(int(val))
        try:
            self._create(view, nrows, ncols, opt, tune_steps, steps_per_chunk, keep_csr)
        finally:
            for name, old in saved.items():
                if old is None:
                    os.environ.pop(name, None)
                else:
                    os.environ[name] = old

    def _create(self, view, nrows, ncols, opt, tune_steps, steps_per_chunk, keep_csr):
        if tune_steps and steps_per_chunk == 0:          # the layout by measurement (cvr_tune): S, chunks per workgroup, x window, column phases
            best, best_t, tun = Options(), C.c_double(), C.c_double()
            rc = lib().cvr_tune(C.byref(view), C.byref(opt), C.byref(best), C.byref(best_t), C.byref(tun))
            if rc:
                raise CvrError(rc, "cvr_tune")
            opt, self.tuning_s = best, tun.value
        rc = lib().cvr_create(C.byref(self._h), C.byref(view), C.byref(opt))
        if rc:
            self._h = C.c_void_p()
            raise CvrError(rc, "cvr_create")
        sec = C.c_double()
        rc = lib().cvr_preprocess(self._h, int(keep_csr), C.byref(sec))
        if rc:
            err = CvrError(rc, "cvr_preprocess")
            self.close()
            raise err
        self.preprocess_s = sec.value
        self.info = Info()
        lib().cvr_get_info(self._h, C.byref(self.info))
        self.nrows, self.ncols = self.info.nrows, self.info.ncols          # (the handle's: A^T's with transpose=1)

    def spmv(self, x, iters=1):
        """y = A x through host buffers; returns (y, Timing)"""
        x = np.ascontiguousarray(x, dtype=self.dtype)
        if len(x) < self.ncols:
            raise ValueError("x is shorter than ncols")
        y = np.zeros(max(self.nrows, 1), dtype=self.dtype)
        t = Timing()
        rc = lib().cvr_spmv(self._h, x.ctypes.data, y.ctypes.data, iters, C.byref(t))
        if rc:
            raise CvrError(rc, "cvr_spmv")
        return y[: self.nrows], t

    def spmv_device(self, x_ptr, y_ptr, stream=None, repeat=1):
        """asynchronous launch(es) on caller-owned device buffers (x_ext: ncols+1 values, last one 0; y_ext)"""
        if repeat == 1:
            rc = lib().cvr_spmv_device(self._h, x_ptr, y_ptr, stream)
        else:
            rc = lib().cvr_spmv_device_repeat(self._h, x_ptr, y_ptr, stream, repeat)
        if rc:
            raise CvrError(rc, "cvr_spmv_device")

    def spmv_scaled(self, x, y, alpha=1.0, beta=0.0):
        """y = alpha A x + beta y through host buffers (cvr_spmv_scaled): returns the new y (nrows values of the handle's dtype); x may be
        None when alpha == 0, y is not read when beta == 0"""
        xa = None if x is None else np.ascontiguousarray(x, dtype=self.dtype)
        if xa is not None and len(xa) < self.ncols:
            raise ValueError("x is shorter than ncols")
        out = np.zeros(max(self.nrows, 1), dtype=self.dtype)
        if y is not None:
            ya = np.asarray(y, dtype=self.dtype)
            if len(ya) < self.nrows:
                raise ValueError("y is shorter than nrows")
            out[: self.nrows] = ya[: self.nrows]
        rc = lib().cvr_spmv_scaled(self._h, float(alpha), None if xa is None else xa.ctypes.data, float(beta), out.ctypes.data)
        if rc:
            raise CvrError(rc, "cvr_spmv_scaled")
        return out[: self.nrows]

    def spmv_scaled_device(self, x_ptr, y_ptr, alpha, beta, stream=None):
        """asynchronous y = alpha A x + beta y on caller-owned device buffers (cvr_spmv_scaled_device; buffers as spmv_device, the first
        nrows values of y_ext are y); x_ptr may be None when alpha == 0"""
        rc = lib().cvr_spmv_scaled_device(self._h, float(alpha), x_ptr, float(beta), y_ptr, stream)
        if rc:
            raise CvrError(rc, "cvr_spmv_scaled_device")

    def _cg_options(self, rtol, max_iters, check_every, minv_ptr):
        opt = CgOptions()
        lib().cvr_cg_default_options(C.byref(opt))
        if rtol is not None:
            opt.rtol = float(rtol)
        if max_iters is not None:
            opt.max_iters = int(max_iters)
        opt.check_every = int(check_every)
        opt.minv_dev = minv_ptr
        return opt

    def _solve(self, symbol, opt, head, tail=(), out=()):
        """one single-vector solver call: symbol(handle, *head, &opt, &res, *&out, *tail) with the solver's further out-structs; returns the CgResult"""
        res = CgResult()
        rc = getattr(lib(), symbol)(self._h, *head, C.byref(opt), C.byref(res), *map(C.byref, out), *tail)
        if rc:
            raise CvrError(rc, symbol)
        return res

    def _solve_multi(self, symbol, opt, nvec, head, tail=()):
        """one batched solver call: symbol(handle, *head, &opt, res[nvec], *tail); returns the list of CgResult"""
        res = (CgResult * max(int(nvec), 1))()
        rc = getattr(lib(), symbol)(self._h, *head, C.byref(opt), res, *tail)
        if rc:
            raise CvrError(rc, symbol)
        return list(res)

    def _host_vectors(self, b, x0, x_len="nrows"):
        """a host solver's b, contiguous in the handle's type, and its x: x0 (None: zero) in a new array of at least one value; x has nrows values,
        or x_len = "ncols" of them"""
        b = np.ascontiguousarray(b, dtype=self.dtype)
        if len(b) < self.nrows:
            raise ValueError("b is shorter than nrows")
        n = getattr(self, x_len)
        x = np.zeros(max(n, 1), dtype=self.dtype)
        if x0 is not None:
            x0 = np.asarray(x0, dtype=self.dtype)
            if len(x0) < n:
                raise ValueError(f"x0 is shorter than {x_len}")
            x[:n] = x0[:n]
        return b, x

    def _gmres_options(self, name, options, minv):
        rtol, max_iters, check_every = options.pop("rtol", None), options.pop("max_iters", None), options.pop("check_every", 0)
        if options:
            raise TypeError(f"{name}: unknown options {sorted(options)}")
        return self._cg_options(rtol, max_iters, check_every, None if minv is None else minv.data_ptr())

    def cg(self, b_ptr, x_ptr, rtol=None, max_iters=None, check_every=0, minv_ptr=None, stream=None):
        """solves A x = b for a symmetric positive definite A by conjugate gradients on the device (cvr_cg_device): b_ptr and x_ptr are
        device arrays of nrows values (x: the start vector in, the solution out), minv_ptr an optional diagonal preconditioner (nrows
        values, z = minv .* r); rtol / max_iters None: the library's defaults.  Returns the CgResult (iterations, status = CG_*,
        spmv_count, residual_norm, b_norm, seconds); synchronises the stream."""
        return self._solve("cvr_cg_device", self._cg_options(rtol, max_iters, check_every, minv_ptr), (b_ptr, x_ptr), (stream,))

    def cg_host(self, b, x0=None, rtol=None, max_iters=None, check_every=0, minv_ptr=None):
        """the same through host arrays (cvr_cg): b and the start vector x0 (None: zero) of nrows values; minv_ptr stays a device
        pointer.  Returns (x, CgResult)."""
        b, x = self._host_vectors(b, x0)
        res = self._solve("cvr_cg", self._cg_options(rtol, max_iters, check_every, minv_ptr), (b.ctypes.data, x.ctypes.data))
        return x[: self.nrows], res

    def pcg(self, precond, b_ptr, x_ptr, rtol=None, max_iters=None, check_every=0, stream=None):
        """conjugate gradients preconditioned by a Precond object (cvr_pcg_device): z = M^-1 r by its apply in place of a diagonal;
        the arguments and the CgResult are cg's.  With block_size = 1 the result is bit for bit cg's with minv = the exported W."""
        return self._solve("cvr_pcg_device", self._cg_options(rtol, max_iters, check_every, None), (precond._p, b_ptr, x_ptr), (stream,))

    def pcg_host(self, precond, b, x0=None, rtol=None, max_iters=None, check_every=0):
        """the same through host arrays (cvr_pcg): b and the start vector x0 (None: zero) of nrows values.  Returns (x, CgResult)."""
        b, x = self._host_vectors(b, x0)
        res = self._solve("cvr_pcg", self._cg_options(rtol, max_iters, check_every, None), (precond._p, b.ctypes.data, x.ctypes.data))
        return x[: self.nrows], res

    def cg_multi(self, B_ptr, ldb, X_ptr, ldx, nvec, rtol=None, max_iters=None, check_every=0, minv_ptr=None, stream=None):
        """solves A X = B for 1 <= nvec <= 8 right-hand sides at once by conjugate gradients on the device (cvr_cg_multi_device): B_ptr and
        X_ptr are row-major device blocks of nrows rows of ldb / ldx values (X: the start block in, the solutions out), minv_ptr one
        preconditioner for all columns.  Column j is bit for bit cg()'s result for B[:, j] and X[:, j].  Needs a handle of the plain layout
        (nvec >= 2 at creation) unless nvec == ldb == ldx == 1.  Returns a list of nvec CgResult; synchronises the stream."""
        return self._solve_multi("cvr_cg_multi_device", self._cg_options(rtol, max_iters, check_every, minv_ptr), nvec, (B_ptr, ldb, X_ptr, ldx, nvec), (stream,))

    def _host_blocks(self, B, X0):
        """a host block solver's B, contiguous in the handle's type with exactly nrows rows, and its X: X0 (None: zero) in a new array"""
        B = np.ascontiguousarray(B, dtype=self.dtype)
        if B.ndim != 2 or B.shape[0] < self.nrows:
            raise ValueError("B must be 2-D with at least nrows rows")
        B = np.ascontiguousarray(B[: self.nrows])
        k = B.shape[1]
        X = np.zeros((max(self.nrows, 1), k), dtype=self.dtype)
        if X0 is not None:
            X0 = np.asarray(X0, dtype=self.dtype)
            if X0.ndim != 2 or X0.shape[0] < self.nrows or X0.shape[1] != k:
                raise ValueError("X0 must have B's shape")
            X[: self.nrows] = X0[: self.nrows]
        return B, X, k

    def cg_multi_host(self, B, X0=None, rtol=None, max_iters=None, check_every=0, minv_ptr=None):
        """the same through host arrays (cvr_cg_multi): B and the start block X0 (None: zero) of shape (nrows, nvec); minv_ptr stays a
        device pointer.  Returns (X of shape (nrows, nvec), list of CgResult)."""
        B, X, k = self._host_blocks(B, X0)
        res = self._solve_multi("cvr_cg_multi", self._cg_options(rtol, max_iters, check_every, minv_ptr), k, (B.ctypes.data, X.ctypes.data, k))
        return X[: self.nrows], res

    def pcg_multi(self, precond, B_ptr, ldb, X_ptr, ldx, nvec, rtol=None, max_iters=None, check_every=0, stream=None):
        """cg_multi preconditioned by a Precond object (cvr_pcg_multi_device): Z = M^-1 R by its k-wide apply in place of a diagonal; the
        blocks and the list of nvec CgResult are cg_multi's.  Column j is bit for bit pcg()'s result for B[:, j] and X[:, j].  Takes block-Jacobi
        objects and, for nvec up to the width they were built for, Precond.amg_block's (one V-cycle per step for all columns)."""
        return self._solve_multi("cvr_pcg_multi_device", self._cg_options(rtol, max_iters, check_every, None), nvec, (precond._p, B_ptr, ldb, X_ptr, ldx, nvec), (stream,))

    def pcg_multi_host(self, precond, B, X0=None, rtol=None, max_iters=None, check_every=0):
        """the same through host arrays (cvr_pcg_multi): B and the start block X0 (None: zero) of shape (nrows, nvec), for the objects pcg_multi
        takes.  Returns (X of shape (nrows, nvec), list of CgResult)."""
        B, X, k = self._host_blocks(B, X0)
        res = self._solve_multi("cvr_pcg_multi", self._cg_options(rtol, max_iters, check_every, None), k, (precond._p, B.ctypes.data, X.ctypes.data, k))
        return X[: self.nrows], res

    def bicgstab(self, b_ptr, x_ptr, rtol=None, max_iters=None, check_every=0, minv_ptr=None, stream=None):
        """solves A x = b for a nonsymmetric A by right-preconditioned BiCGSTAB on the device (cvr_bicgstab_device): the arguments and the
        CgResult are cg's (minv_ptr: p^ = minv .* p, s^ = minv .* s; a stop at the half step counts as one iteration; two SpMVs per
        step); synchronises the stream."""
        return self._solve("cvr_bicgstab_device", self._cg_options(rtol, max_iters, check_every, minv_ptr), (b_ptr, x_ptr), (stream,))

    def bicgstab_host(self, b, x0=None, rtol=None, max_iters=None, check_every=0, minv_ptr=None):
        """the same through host arrays (cvr_bicgstab): b and the start vector x0 (None: zero) of nrows values; minv_ptr stays a device
        pointer.  Returns (x, CgResult)."""
        b, x = self._host_vectors(b, x0)
        res = self._solve("cvr_bicgstab", self._cg_options(rtol, max_iters, check_every, minv_ptr), (b.ctypes.data, x.ctypes.data))
        return x[: self.nrows], res

    def pbicgstab(self, precond, b_ptr, x_ptr, rtol=None, max_iters=None, check_every=0, stream=None):
        """BiCGSTAB preconditioned by a Precond object (cvr_pbicgstab_device): p^ = M^-1 p and s^ = M^-1 s by its apply in place of a diagonal;
        the arguments and the CgResult are bicgstab's.  With block_size = 1 the result is bit for bit bicgstab's with minv = the exported W."""
        return self._solve("cvr_pbicgstab_device", self._cg_options(rtol, max_iters, check_every, None), (precond._p, b_ptr, x_ptr), (stream,))

    def pbicgstab_host(self, precond, b, x0=None, rtol=None, max_iters=None, check_every=0):
        """the same through host arrays (cvr_pbicgstab): b and the start vector x0 (None: zero) of nrows values.  Returns (x, CgResult)."""
        b, x = self._host_vectors(b, x0)
        res = self._solve("cvr_pbicgstab", self._cg_options(rtol, max_iters, check_every, None), (precond._p, b.ctypes.data, x.ctypes.data))
        return x[: self.nrows], res

    def lsqr(self, at, b_ptr, x_ptr, damp=0.0, rtol=None, max_iters=None, check_every=0, stream=None):
        """min ||b - A x||_2 (damp > 0: with the Tikhonov term damp^2 ||x - x0||^2) by LSQR on the device (cvr_lsqr_device) for A of any shape:
        `at` is a CvrMatrix of A^T (transpose=1 on the same CSR; self for a square symmetric A), b_ptr a device array of nrows values, x_ptr one
        of ncols values (the start vector in, the solution out).  Returns (CgResult, LsqrInfo); synchronises the stream."""
        info = LsqrInfo()
        res = self._solve("cvr_lsqr_device", self._cg_options(rtol, max_iters, check_every, None), (at._h, b_ptr, x_ptr, float(damp)), (stream,), (info,))
        return res, info

    def lsqr_host(self, at, b, x0=None, damp=0.0, rtol=None, max_iters=None, check_every=0):
        """the same through host arrays (cvr_lsqr): b of nrows values and the start vector x0 (None: zero) of ncols values.  Returns
        (x, CgResult, LsqrInfo)."""
        (b, x), info = self._host_vectors(b, x0, "ncols"), LsqrInfo()
        res = self._solve("cvr_lsqr", self._cg_options(rtol, max_iters, check_every, None), (at._h, b.ctypes.data, x.ctypes.data, float(damp)), out=(info,))
        return x[: self.ncols], res, info

    def minres(self, b_ptr, x_ptr, shift=0.0, rtol=None, max_iters=None, check_every=0, minv_ptr=None, stream=None):
        """solves (A - shift I) x = b for a symmetric A, indefinite ones included, by MINRES on the device (cvr_minres_device): the arguments are
        cg's (minv_ptr: an optional positive diagonal preconditioner).  Returns (CgResult, MinresInfo); synchronises the stream."""
        info = MinresInfo()
        res = self._solve("cvr_minres_device", self._cg_options(rtol, max_iters, check_every, minv_ptr), (b_ptr, x_ptr, float(shift)), (stream,), (info,))
        return res, info

    def minres_host(self, b, x0=None, shift=0.0, rtol=None, max_iters=None, check_every=0, minv_ptr=None):
        """the same through host arrays (cvr_minres): b and the start vector x0 (None: zero) of nrows values; minv_ptr stays a device pointer.
        Returns (x, CgResult, MinresInfo)."""
        (b, x), info = self._host_vectors(b, x0), MinresInfo()
        res = self._solve("cvr_minres", self._cg_options(rtol, max_iters, check_every, minv_ptr), (b.ctypes.data, x.ctypes.data, float(shift)), out=(info,))
        return x[: self.nrows], res, info

    def _eig_options(self, nev, which, ncv, tol, max_restarts):
        opt = EigOptions()
        lib().cvr_eig_default_options(C.byref(opt))
        opt.which = _which(which)
        opt.nev, opt.ncv, opt.tol, opt.max_restarts = int(nev), int(ncv), float(tol), int(max_restarts)
        return opt

    def _start_vector(self, v0, n, seed, what):
        """a start vector of n values on the host: v0, or a standard normal one from `seed`; `what` names n in the error"""
        if v0 is None:
            return np.random.default_rng(seed).standard_normal(max(n, 1)).astype(self.dtype)
        v0 = np.ascontiguousarray(v0, dtype=self.dtype)
        if len(v0) < n:
            raise ValueError(f"v0 is shorter than {what}")
        return v0

    def eigsh(self, nev, which="LA", ncv=0, tol=1e-8, v0=None, max_restarts=100, vectors=True, stream=None):
        """the nev algebraically largest ("LA") or smallest ("SA") eigenvalues of a symmetric A and their eigenvectors by thick-restart Lanczos on the
        device (cvr_eigsh_device).  v0: a torch device array of nrows values of the handle's type (anything with data_ptr()), or None: a seeded
        numpy vector, copied up.  Returns (evals: numpy, ascending; evecs: a torch device array of shape (count, nrows) whose row c is the vector of
        evals[c], or None without vectors; EigResult); count is nev, less at EIG_INVARIANT (nconv) and 0 at EIG_BREAKDOWN.  Synchronises the stream."""
        import torch
        opt, res = self._eig_options(nev, which, ncv, tol, max_restarts), EigResult()
        tdt = torch.float32 if self.dtype == np.float32 else torch.float64
        if v0 is None:
            v0 = torch.from_numpy(self._start_vector(None, self.nrows, 20261019, "nrows")).to("cuda")
        n = max(self.nrows, 1)
        evals = np.zeros(max(int(nev), 1))
        evecs = torch.zeros((max(int(nev), 1), n), dtype=tdt, device="cuda") if vectors else None
        torch.cuda.synchronize()
        rc = lib().cvr_eigsh_device(self._h, v0.data_ptr(), evals.ctypes.data, None if evecs is None else evecs.data_ptr(), n, C.byref(opt), C.byref(res), stream)
        if rc:
            raise CvrError(rc, "cvr_eigsh_device")
        count = _returned_count(res, nev)
        return evals[:count], (None if evecs is None else evecs[:count, : self.nrows]), res

    def eigsh_host(self, nev, which="LA", ncv=0, tol=1e-8, v0=None, max_restarts=100, vectors=True):
        """the same through host arrays (cvr_eigsh).  Returns (evals, evecs: numpy of shape (nrows, count) with the vector of evals[c] in column c, or
        None without vectors; EigResult)."""
        opt, res = self._eig_options(nev, which, ncv, tol, max_restarts), EigResult()
        v0 = self._start_vector(v0, self.nrows, 20261019, "nrows")
        n = max(self.nrows, 1)
        evals = np.zeros(max(int(nev), 1))
        evecs = np.zeros((max(int(nev), 1), n), dtype=self.dtype) if vectors else None
        rc = lib().cvr_eigsh(self._h, v0.ctypes.data, evals.ctypes.data, None if evecs is None else evecs.ctypes.data, n, C.byref(opt), C.byref(res))
        if rc:
            raise CvrError(rc, "cvr_eigsh")
        count = _returned_count(res, nev)
        return evals[:count], (None if evecs is None else evecs[:count, : self.nrows].T), res

    def _svd_options(self, nev, ncv, tol, max_restarts):
        opt = SvdOptions()
        lib().cvr_svd_default_options(C.byref(opt))
        opt.nev, opt.ncv, opt.tol, opt.max_restarts = int(nev), int(ncv), float(tol), int(max_restarts)
        return opt

    def svds(self, at, v0=None, nev=1, ncv=0, tol=1e-8, max_restarts=100, vectors=True, stream=None):
        """the nev largest singular values of A, of any shape, and their vectors by thick-restart Golub-Kahan-Lanczos on the device (cvr_svds_device).
        `at` is a CvrMatrix of A^T (transpose=1 on the same CSR; self for a symmetric A), as in lsqr.  v0: a torch device array of ncols values of
        the handle's type (anything with data_ptr()), or None: a seeded numpy vector, copied up.  Returns (svals: numpy, descending; U: a torch
        device array of shape (count, nrows) whose row c is the left vector of svals[c]; V: the same of shape (count, ncols) with the right ones;
        both None without vectors; SvdResult); count is nev, less at EIG_INVARIANT (nconv) and 0 at EIG_BREAKDOWN.  Synchronises the stream."""
        import torch
        opt, res = self._svd_options(nev, ncv, tol, max_restarts), SvdResult()
        tdt = torch.float32 if self.dtype == np.float32 else torch.float64
        if v0 is None:
            v0 = torch.from_numpy(self._start_vector(None, self.ncols, 20261021, "ncols")).to("cuda")
        nr, nc, cols = max(self.nrows, 1), max(self.ncols, 1), max(int(nev), 1)
        svals = np.zeros(cols)
        U = torch.zeros((cols, nr), dtype=tdt, device="cuda") if vectors else None
        V = torch.zeros((cols, nc), dtype=tdt, device="cuda") if vectors else None
        torch.cuda.synchronize()
        rc = lib().cvr_svds_device(self._h, at._h, v0.data_ptr(), svals.ctypes.data, None if U is None else U.data_ptr(), nr,
                                   None if V is None else V.data_ptr(), nc, C.byref(opt), C.byref(res), stream)
        if rc:
            raise CvrError(rc, "cvr_svds_device")
        count = _returned_count(res, nev)
        return svals[:count], (None if U is None else U[:count, : self.nrows]), (None if V is None else V[:count, : self.ncols]), res

    def svds_host(self, at, v0=None, nev=1, ncv=0, tol=1e-8, max_restarts=100, vectors=True):
        """the same through host arrays (cvr_svds).  Returns (svals; U: numpy of shape (nrows, count) with the left vector of svals[c] in column c; V:
        the same of shape (ncols, count); both None without vectors; SvdResult)."""
        opt, res = self._svd_options(nev, ncv, tol, max_restarts), SvdResult()
        v0 = self._start_vector(v0, self.ncols, 20261021, "ncols")
        nr, nc, cols = max(self.nrows, 1), max(self.ncols, 1), max(int(nev), 1)
        svals = np.zeros(cols)
        U = np.zeros((cols, nr), dtype=self.dtype) if vectors else None
        V = np.zeros((cols, nc), dtype=self.dtype) if vectors else None
        rc = lib().cvr_svds(self._h, at._h, v0.ctypes.data, svals.ctypes.data, None if U is None else U.ctypes.data, nr,
                            None if V is None else V.ctypes.data, nc, C.byref(opt), C.byref(res))
        if rc:
            raise CvrError(rc, "cvr_svds")
        count = _returned_count(res, nev)
        return svals[:count], (None if U is None else U[:count, : self.nrows].T), (None if V is None else V[:count, : self.ncols].T), res

    def _lobpcg_options(self, nev, which, tol, max_iters):
        opt = LobpcgOptions()
        lib().cvr_lobpcg_default_options(C.byref(opt))
        opt.which = _which(which)
        opt.nev, opt.tol, opt.max_iters = int(nev), float(tol), int(max_iters)
        return opt

    def lobpcg(self, X, precond=None, which="SA", tol=1e-8, max_iters=200, stream=None):
        """the X.shape[0] (1 .. LOBPCG_MAX_BLOCK) algebraically smallest ("SA") or largest ("LA") eigenvalues of a symmetric A and their eigenvectors by
        LOBPCG on the device (cvr_lobpcg_device), with an optional Precond of any kind ("SA" only).  X: a contiguous torch device array of shape
        (nev, ld), ld >= nrows, of the handle's type: row c carries column c of the start block in and the eigenvector of evals[c] out (the C ABI's
        column-major block with ldx = ld).  Returns (evals: numpy, ascending; resnorms: numpy; LobpcgResult); at EIG_BREAKDOWN both are empty and X is
        unchanged.  Synchronises the stream."""
        if X.dim() != 2 or not X.is_contiguous():
            raise ValueError("X must be a contiguous (nev, ld) array")
        nev, ld = int(X.shape[0]), int(X.shape[1])
        opt, res = self._lobpcg_options(nev, which, tol, max_iters), LobpcgResult()
        evals, resn = np.zeros(max(nev, 1)), np.zeros(max(nev, 1))
        import torch
        torch.cuda.synchronize()
        rc = lib().cvr_lobpcg_device(self._h, None if precond is None else precond._p, X.data_ptr(), ld, evals.ctypes.data, resn.ctypes.data, C.byref(opt),
                                     C.byref(res), stream)
        if rc:
            raise CvrError(rc, "cvr_lobpcg_device")
        count = 0 if res.status == EIG_BREAKDOWN else nev
        return evals[:count], resn[:count], res

    def lobpcg_host(self, X, precond=None, which="SA", tol=1e-8, max_iters=200):
        """the same through a host array (cvr_lobpcg).  X: numpy of shape (nrows, nev), column c the start vector of pair c.  Returns (evals, X: the
        eigenvectors in the same shape, resnorms, LobpcgResult); at EIG_BREAKDOWN evals and resnorms are empty and X is the start block."""
        X = np.asarray(X, dtype=self.dtype)
        if X.ndim != 2 or X.shape[0] < self.nrows:
            raise ValueError("X must have shape (nrows, nev)")
        nev = int(X.shape[1])
        blk = np.ascontiguousarray(X[: self.nrows].T)          # row c = column c of the block
        opt, res = self._lobpcg_options(nev, which, tol, max_iters), LobpcgResult()
        evals, resn = np.zeros(max(nev, 1)), np.zeros(max(nev, 1))
        rc = lib().cvr_lobpcg(self._h, None if precond is None else precond._p, blk.ctypes.data, max(self.nrows, 1), evals.ctypes.data, resn.ctypes.data,
                              C.byref(opt), C.byref(res))
        if rc:
            raise CvrError(rc, "cvr_lobpcg")
        count = 0 if res.status == EIG_BREAKDOWN else nev
        return evals[:count], blk.T, resn[:count], res

    def gmres(self, b, x0=None, restart=30, minv=None, stream=None, **options):
        """solves A x = b for any nonsingular A by restarted GMRES(restart) on the device (cvr_gmres_device).  b, x0 and minv are torch device
        arrays (anything with data_ptr() and new_zeros()) of nrows values of the handle's type: x0 is the start vector and is overwritten with the
        solution (None: a new zero array), minv the optional right preconditioner.  options: rtol, max_iters (None: the library's defaults),
        check_every.  Returns (x, CgResult); synchronises the stream."""
        opt = self._gmres_options("gmres", options, minv)
        x = b.new_zeros(max(self.nrows, 1)) if x0 is None else x0
        res = self._solve("cvr_gmres_device", opt, (b.data_ptr(), x.data_ptr(), int(restart)), (stream,))
        return (x[: self.nrows] if x0 is None else x), res

    def gmres_host(self, b, x0=None, restart=30, minv=None, **options):
        """the same through host arrays (cvr_gmres): b and the start vector x0 (None: zero) of nrows values; minv stays a device array.
        Returns (x, CgResult)."""
        opt = self._gmres_options("gmres_host", options, minv)
        b, x = self._host_vectors(b, x0)
        return x[: self.nrows], self._solve("cvr_gmres", opt, (b.ctypes.data, x.ctypes.data, int(restart)))

    def pgmres(self, precond, b, x0=None, restart=30, stream=None, **options):
        """restarted GMRES(restart) preconditioned by a Precond object (cvr_pgmres_device): z = M^-1 v by its apply in place of a diagonal; b, x0,
        the options and the return value are gmres's.  With block_size = 1 the result is bit for bit gmres's with minv = the exported W."""
        opt = self._gmres_options("pgmres", options, None)
        x = b.new_zeros(max(self.nrows, 1)) if x0 is None else x0
        res = self._solve("cvr_pgmres_device", opt, (precond._p, b.data_ptr(), x.data_ptr(), int(restart)), (stream,))
        return (x[: self.nrows] if x0 is None else x), res

    def pgmres_host(self, precond, b, x0=None, restart=30, **options):
        """the same through host arrays (cvr_pgmres): b and the start vector x0 (None: zero) of nrows values.  Returns (x, CgResult)."""
        opt = self._gmres_options("pgmres_host", options, None)
        b, x = self._host_vectors(b, x0)
        return x[: self.nrows], self._solve("cvr_pgmres", opt, (precond._p, b.ctypes.data, x.ctypes.data, int(restart)))

    def _fgmres(self, symbol, name, precond, apply, head, tail, options):
        """one cvr_fgmres* call: the Python `apply` wrapped in an APPLY_FN that lives as long as the call; an exception it raises becomes the return
        code 1 and is raised again behind the C call"""
        opt = self._gmres_options(name, options, None)
        raised = []

        def trampoline(_ctx, v_ptr, z_ptr, n, stream):
            try:
                return int(apply(v_ptr, z_ptr, n, stream) or 0)
            except BaseException as e:  # noqa: BLE001
                raised.append(e)
                return 1

        fn = APPLY_FN(trampoline) if apply is not None else APPLY_FN()
        try:
            return self._solve(symbol, opt, (None if precond is None else precond._p, fn, None) + head, tail)
        except CvrError:
            if raised:
                raise raised[0]
            raise

    def fgmres(self, b, restart=30, precond=None, apply=None, x0=None, stream=None, **options):
        """flexible restarted GMRES(restart) on the device (cvr_fgmres_device): z_j = M_j^-1 v_j is kept for every column and x = x0 + Z y, so the
        preconditioner may be any kind of Precond (`precond`), or a Python callable `apply(v_ptr, z_ptr, n, stream) -> int` that leaves z = M^-1 v
        complete in stream order on `stream` (raw device pointers of n values of the handle's type; its k-th call belongs to step k; a non-zero
        return or an exception ends the solve, the exception is raised again here), or neither (then bit for bit gmres without minv).  b, x0, the
        options (rtol, max_iters, check_every) and the return value are gmres's."""
        x = b.new_zeros(max(self.nrows, 1)) if x0 is None else x0
        res = self._fgmres("cvr_fgmres_device", "fgmres", precond, apply, (b.data_ptr(), x.data_ptr(), int(restart)), (stream,), options)
        return (x[: self.nrows] if x0 is None else x), res

    def fgmres_host(self, b, restart=30, precond=None, apply=None, x0=None, **options):
        """the same through host arrays (cvr_fgmres): b and the start vector x0 (None: zero) of nrows values; `apply` still gets device pointers and
        the handle's stream.  Returns (x, CgResult)."""
        b, x = self._host_vectors(b, x0)
        return x[: self.nrows], self._fgmres("cvr_fgmres", "fgmres_host", precond, apply, (b.ctypes.data, x.ctypes.data, int(restart)), (), options)

    def spmm(self, X, iters=1):
        """Y = A X for the k columns of X (host array of shape (ncols, k)) in one pass per block of 8 (cvr_spmm); returns (Y of shape
        (nrows, k), Timing).  Needs a handle of the plain layout (nvec >= 2 at creation) unless k == 1."""
        X = np.ascontiguousarray(X, dtype=self.dtype)
        if X.ndim != 2 or X.shape[0] < self.ncols:
            raise ValueError("X must be 2-D with at least ncols rows")
        X = np.ascontiguousarray(X[: self.ncols])
        k = X.shape[1]
        Y = np.zeros((max(self.nrows, 1), k), dtype=self.dtype)
        t = Timing()
        rc = lib().cvr_spmm(self._h, X.ctypes.data, Y.ctypes.data, k, iters, C.byref(t))
        if rc:
            raise CvrError(rc, "cvr_spmm")
        return Y[: self.nrows], t

    def spmm_device(self, X_ptr, ldx, Y_ptr, ldy, nvec, stream=None):
        """asynchronous Y = A X on caller-owned device buffers (cvr_spmm_device): X_ptr = x_elems rows of ldx values (row ncols zero),
        Y_ptr = yext_elems rows of ldy values"""
        rc = lib().cvr_spmm_device(self._h, X_ptr, ldx, Y_ptr, ldy, nvec, stream)
        if rc:
            raise CvrError(rc, "cvr_spmm_device")

    @property
    def spmm_supported(self):
        """True: spmm_device takes any number of vectors (the plain layout); False: only one of stride 1"""
        return bool(lib().cvr_spmm_supported(self._h))

    def update_values(self, vals):
        """new values of the same pattern from host memory (cvr_update_values): vals indexed like the creation's vals (row_ptr[nrows]
        elements); returns when the image holds them"""
        vals = np.ascontiguousarray(vals, dtype=self.dtype)
        rc = lib().cvr_update_values(self._h, vals.ctypes.data)
        if rc:
            raise CvrError(rc, "cvr_update_values")

    def update_values_device(self, vals_ptr, stream=None):
        """asynchronous update from a device array of the handle's device (cvr_update_values_device), ordered like spmv_device"""
        rc = lib().cvr_update_values_device(self._h, vals_ptr, stream)
        if rc:
            raise CvrError(rc, "cvr_update_values_device")

    def update_values_supported(self):
        """True: the handle takes update_values / update_values_device (mutable_values, no kept CSR)"""
        return bool(lib().cvr_update_values_supported(self._h))

    def spmv_gather(self, comm, x_ptr, y_ptrs, yall_ptrs, max_rows, steps, stream=None, overlap=False):
        """`steps` sharded SpMVs, each followed by the all-gather of this rank's y slice over RCCL, looped inside the
        library (cvr_spmv_gather_repeat; overlap: gather of step k under the SpMV of step k+1); returns the index of
        the buffers holding the last step"""
        ys = (C.c_void_p * 2)(*y_ptrs)
        yalls = (C.c_void_p * 2)(*yall_ptrs)
        last = C.c_int()
        rc = lib().cvr_spmv_gather_repeat(self._h, comm._c, x_ptr, ys, yalls, max_rows, steps, int(overlap), stream, C.byref(last))
        if rc:
            raise CvrError(rc, "cvr_spmv_gather_repeat")
        return last.value

    def power_iteration(self, x_ptr, iters, comm=None, bounds=None, stream=None):
        """x <- A x / ||A x||, `iters` times on the device (cvr_power_iteration); returns (Rayleigh quotient, seconds per iteration)"""
        lam, sec = C.c_double(), C.c_double()
        b = None if bounds is None else np.ascontiguousarray(bounds, dtype=np.int64)
        rc = lib().cvr_power_iteration(self._h, None if comm is None else comm._c, None if b is None else b.ctypes.data, iters, x_ptr,
                                       C.byref(lam), C.byref(sec), stream)
        if rc:
            raise CvrError(rc, "cvr_power_iteration")
        return lam.value, sec.value

    def chebyshev_bounds(self, power_iters=20, eig_ratio=30.0, stream=None):
        """(lmin, lmax) for Precond.chebyshev from `power_iters` power steps (cvr_chebyshev_bounds): lmax = 1.1 * the Rayleigh quotient,
        lmin = lmax / eig_ratio; synchronises the stream"""
        lo, hi = C.c_double(), C.c_double()
        rc = lib().cvr_chebyshev_bounds(self._h, int(power_iters), float(eig_ratio), C.byref(lo), C.byref(hi), stream)
        if rc:
            raise CvrError(rc, "cvr_chebyshev_bounds")
        return lo.value, hi.value

    def bench(self, warmup, iters):
        s = C.c_double()
        rc = lib().cvr_spmv_bench(self._h, warmup, iters, C.byref(s))
        if rc:
            raise CvrError(rc, "cvr_spmv_bench")
        return s.value

    def phase_clocks(self):
        """diagnostics (CVR_DEBUG=phase_clocks at creation): [workgroups][16 wavefronts][8] uint64 stamps of the last SpMV (cvr_debug_phase_clocks)"""
        n = C.c_int64()
        rc = lib().cvr_debug_phase_clocks(self._h, None, 0, C.byref(n))
        if rc:
            raise CvrError(rc, "cvr_debug_phase_clocks")
        out = np.zeros(n.value, dtype=np.uint64)
        rc = lib().cvr_debug_phase_clocks(self._h, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n))
        if rc:
            raise CvrError(rc, "cvr_debug_phase_clocks")
        return out.reshape(-1, 16, 8)

    @property
    def x_device(self):
        return lib().cvr_x_device(self._h)

    @property
    def y_device(self):
        return lib().cvr_y_device(self._h)

    @property
    def stream(self):
        return lib().cvr_stream(self._h)

    def export_image(self):
        i = self.info
        gb = (1280 if i.value_dict else (1536 if self.f32 else 2560) if i.narrow_cols else 2048 if self.f32 else 3072) + (512 if i.row_tags16 else 0)
        image = np.zeros(i.nchunks * (i.steps_per_chunk // 4) * gb, dtype=np.uint8)
        desc = np.zeros((i.nchunks, 4), dtype=np.uint32)
        target = np.zeros((i.nchunks, 64), dtype=np.uint8)
        shared = np.zeros((i.nshared, 3), dtype=np.int64)
        rc = lib().cvr_export_image(self._h, image.ctypes.data, desc.ctypes.data, target.ctypes.data, shared.ctypes.data)
        if rc:
            raise CvrError(rc, "cvr_export_image")
        out = dict(image=image, desc=desc, target=target, shared=shared)
        if i.gang:                      # gang chunks: the groups' first columns and the gangs' group counts
            gbase = np.zeros(i.nchunks * (i.steps_per_chunk // 4), dtype=np.uint32)
            desc2 = np.zeros((i.nchunks, 2), dtype=np.uint32)
            rc = lib().cvr_export_gang(self._h, gbase.ctypes.data, desc2.ctypes.data)
            if rc:
                raise CvrError(rc, "cvr_export_gang")
            out.update(gbase=gbase, desc2=desc2)
        return out

    def close(self):
        if self._h:
            lib().cvr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiMatrix:
    """One matrix over several GPUs of this process (cvr_create_multi): rows sharded, x replicated, y all-gathered inside the
    library.  devices may name one GPU several times (copies then stand in for RCCL)."""

    def __init__(self, nrows, ncols, row_ptr, col_idx, vals, devices, **options):
        self._m = C.c_void_p()
        rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
        ci = np.ascontiguousarray(col_idx, dtype=np.int32)
        self.f32 = np.asarray(vals).dtype == np.float32
        self.dtype = np.float32 if self.f32 else np.float64
        va = np.ascontiguousarray(vals, dtype=self.dtype)
        if len(rp) != nrows + 1:
            raise ValueError("row_ptr must have nrows + 1 entries")
        view = CsrView(nrows, ncols, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, int(self.f32))
        opt = Options()
        lib().cvr_default_options(C.byref(opt))
        for k, v in options.items():
            setattr(opt, k, v)
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        rc = lib().cvr_create_multi(C.byref(self._m), C.byref(view), C.byref(opt), devs.ctypes.data, len(devs))
        if rc:
            self._m = C.c_void_p()
            raise CvrError(rc, "cvr_create_multi")
        sec = C.c_double()
        rc = lib().cvr_preprocess_multi(self._m, 0, C.byref(sec))
        if rc:
            err = CvrError(rc, "cvr_preprocess_multi")
            self.close()
            raise err
        self.preprocess_s = sec.value
        self.nrows, self.ncols = nrows, ncols
        self.shards = lib().cvr_multi_shards(self._m)
        self.uses_rccl = bool(lib().cvr_multi_uses_rccl(self._m))

    def shard_info(self, p):
        info, b, e, d = Info(), C.c_int64(), C.c_int64(), C.c_int32()
        rc = lib().cvr_multi_info(self._m, p, C.byref(info), C.byref(b), C.byref(e), C.byref(d))
        if rc:
            raise CvrError(rc, "cvr_multi_info")
        return info, b.value, e.value, d.value

    def spmv(self, x, iters=1):
        x = np.ascontiguousarray(x, dtype=self.dtype)
        if len(x) < self.ncols:
            raise ValueError("x is shorter than ncols")
        y = np.zeros(max(self.nrows, 1), dtype=self.dtype)
        t = Timing()
        rc = lib().cvr_spmv_multi(self._m, x.ctypes.data, y.ctypes.data, iters, C.byref(t))
        if rc:
            raise CvrError(rc, "cvr_spmv_multi")
        return y[: self.nrows], t

    def close(self):
        if self._m:
            lib().cvr_destroy_multi(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
