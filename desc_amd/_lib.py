"""ctypes binding of libdesc_amd.so -- the C ABI declared in include/desc_amd.h.

There is no CPU fallback: if the shared library is missing, or no HIP device is
visible when a solver handle is created, the call raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DESC_AMD_LIB", os.path.join(HERE, "libdesc_amd.so"))   # override: diagnostic builds only

DESC_OK = 0
STEP_CONSTANT, STEP_PIECEWISE, STEP_HYBRID, STEP_EXTERNAL = 0, 1, 2, 3
MEM_HOST, MEM_DEVICE = 0, 1
BUILD_HOST, BUILD_DEVICE = 0, 1

# every symbol include/desc_amd.h declares (tests check that the library exports them)
EXPORTS = [
    "desc_last_error", "desc_version", "desc_device_count", "desc_problem_upload", "desc_problem_free",
    "desc_spectral_run_dev", "desc_gcw_run_dev", "desc_cemp_run_dev", "desc_refine_run_dev", "desc_pgd_create_dev",
    "desc_structure_build", "desc_structure_import", "desc_structure_get", "desc_structure_sizes",
    "desc_structure_host_exports", "desc_structure_free",
    "desc_sample_key", "desc_params_default",
    "desc_pgd_create", "desc_pgd_destroy", "desc_pgd_run", "desc_pgd_run_traced", "desc_pgd_reset", "desc_pgd_iterate",
    "desc_pgd_iterate_timed", "desc_pgd_sync", "desc_pgd_download", "desc_pgd_get_s0",
    "desc_pgd_sizes", "desc_pgd_layout_stats", "desc_pgd_kernel_name", "desc_pgd_solve", "desc_selftest_group_sum",
    "desc_pgd_create_shard", "desc_pgd_shard_info", "desc_pgd_shard_bind", "desc_pgd_shard_colsum", "desc_pgd_shard_sweep",
    "desc_pgd_shard_finish", "desc_pgd_shard_objective", "desc_pgd_shard_set_collectives", "desc_pgd_shard_start",
    "desc_pgd_shard_iterate", "desc_pgd_shard_run", "desc_pgd_stopped", "desc_device_synchronize", "desc_memcpy_d2h", "desc_memcpy_h2d", "desc_debug_band_plan", "desc_debug_spmm_variants", "desc_debug_wg_clock", "desc_debug_wg_plan", "desc_debug_last_sweep", "desc_debug_shard_layout", "desc_trim_memory", "desc_spectral_run", "desc_cemp_run", "desc_refine_run",
    "desc_marshal_edges", "desc_marshal_rij", "desc_mst_run", "desc_mst_run_dev", "desc_mpls_run", "desc_mpls_run_dev",
    "desc_irls_run", "desc_irls_run_dev", "desc_lp_params_default", "desc_lp_sij_run", "desc_lp_sij_run_dev",
    "desc_pgd_ext_begin", "desc_pgd_ext_grad", "desc_pgd_ext_apply", "desc_pgd_ext_laps",
    "desc_pgd_batch_create", "desc_pgd_batch_sizes", "desc_pgd_batch_get_structure", "desc_pgd_batch_get_s0", "desc_pgd_batch_run",
    "desc_pgd_batch_destroy", "desc_pgd_batch_concat",
    "desc_pgd_batch_create_where", "desc_pgd_batch_built_where", "desc_pgd_batch_max_codeg", "desc_pgd_batch_build_laps", "desc_test_batch_plan",
    "desc_gcw_batch_max_n", "desc_gcw_batch_create", "desc_gcw_batch_sizes", "desc_gcw_batch_csr", "desc_gcw_batch_run", "desc_gcw_batch_destroy",
    "desc_gcw_batch_create_where", "desc_gcw_batch_streamed_max_n",
    "desc_cemp_batch_max_degree", "desc_cemp_batch_create", "desc_cemp_batch_sizes", "desc_cemp_batch_get_samples", "desc_cemp_batch_run",
    "desc_cemp_batch_destroy", "desc_mst_batch_max_n", "desc_mst_batch_check", "desc_mst_batch_run",
    "desc_refine_batch_max_n", "desc_refine_batch_create", "desc_refine_batch_sizes", "desc_refine_batch_run", "desc_refine_batch_destroy",
    "desc_mpls_batch_max_n", "desc_mpls_batch_run",
    "desc_irls_batch_max_n", "desc_irls_batch_create", "desc_irls_batch_sizes", "desc_irls_batch_run", "desc_irls_batch_destroy",
    "desc_irls_tree_sequence",
    "desc_lp_batch_plan", "desc_lp_batch_create", "desc_lp_batch_sizes", "desc_lp_batch_get_samples", "desc_lp_batch_run", "desc_lp_batch_destroy",
    "desc_models_key", "desc_models_batch_max_n", "desc_models_batch_create", "desc_models_batch_sizes", "desc_models_batch_fetch",
    "desc_models_batch_destroy", "desc_test_models_uniform", "desc_test_models_normal",
    "desc_align_batch_create", "desc_align_batch_sizes", "desc_align_batch_run", "desc_align_batch_destroy", "desc_test_align_project",
    "desc_problem_batch_create", "desc_problem_batch_from_models", "desc_problem_batch_sizes", "desc_problem_batch_fetch",
    "desc_problem_batch_built_where", "desc_problem_batch_bytes", "desc_problem_batch_destroy",
    "desc_gcw_batch_create_on", "desc_refine_batch_create_on", "desc_pgd_batch_create_on",
    "desc_gcw_batch_bytes", "desc_refine_batch_bytes", "desc_pgd_batch_bytes",
    "desc_cemp_batch_create_on", "desc_irls_batch_create_on", "desc_mst_batch_run_on", "desc_cemp_batch_bytes", "desc_irls_batch_bytes",
    "desc_test_laa_r2q", "desc_test_laa_q2r", "desc_test_laa_edge_log", "desc_test_laa_rhs", "desc_test_laa_pcg", "desc_test_laa_node_update",
    "desc_test_irls_node_update", "desc_test_laa_weights", "desc_test_irls_weights", "desc_test_laa_quantile", "desc_test_irls_project",
    "desc_test_irls_pd_stage", "desc_test_irls_pd_solve",
    "desc_test_spectral_weights", "desc_test_spectral_row_wsum", "desc_test_spectral_assemble", "desc_test_spectral_spmm", "desc_test_spectral_gram",
    "desc_test_spectral_residual", "desc_test_spectral_combine", "desc_test_small_jacobi", "desc_test_small_ortho", "desc_test_small_project",
    "desc_test_small_ritz_tail",
]

I32P = C.POINTER(C.c_int32)
I64P = C.POINTER(C.c_int64)
F64P = C.POINTER(C.c_double)


class Problem(C.Structure):
    _fields_ = [("n", C.c_int64), ("m", C.c_int64), ("ind_i", I32P), ("ind_j", I32P), ("rij", F64P)]


class StructureView(C.Structure):
    _fields_ = [("n", C.c_int64), ("m", C.c_int64), ("m_pos", C.c_int64), ("m_cycle", C.c_int64),
                ("n_sample", C.c_int32), ("max_cnt", C.c_int32),
                ("codeg", I32P), ("pos_edge", I32P), ("cum_ind", I64P),
                ("k", I32P), ("e_jk", I32P), ("e_ki", I32P), ("ikj", I32P), ("jki", I32P)]


class StructureInfo(C.Structure):
    _fields_ = [("n", C.c_int64), ("m", C.c_int64), ("m_pos", C.c_int64), ("m_cycle", C.c_int64),
                ("n_sample", C.c_int32), ("max_cnt", C.c_int32), ("built_where", C.c_int32),
                ("host_resident", C.c_int32), ("ms_build", C.c_double)]


class Params(C.Structure):
    _fields_ = [("iters", C.c_int32), ("step_kind", C.c_int32), ("lr", C.c_double),
                ("beta1", C.c_double), ("beta2", C.c_double), ("decay_interval", C.c_double),
                ("hybrid_strategy", C.c_int32), ("t0", C.c_int32), ("patience", C.c_int32),
                ("stop_tol", C.c_double), ("n_sample_min", C.c_int32), ("seed", C.c_uint64),
                ("verbose", C.c_int32), ("device", C.c_int32), ("build_where", C.c_int32),
                ("check_every", C.c_int32), ("progress", C.c_void_p), ("progress_user", C.c_void_p)]


PROGRESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_double, C.c_double)


class Result(C.Structure):
    _fields_ = [("s_vec", F64P), ("obj_trace", F64P), ("avg_change_trace", F64P), ("w", F64P),
                ("adam_m", F64P), ("adam_v", F64P), ("iters_run", C.c_int32), ("t_end", C.c_int32),
                ("ms_structure", C.c_double), ("ms_upload", C.c_double), ("ms_cycle_d", C.c_double),
                ("ms_pgd", C.c_double), ("ms_total", C.c_double)]


class BatchResult(C.Structure):
    _fields_ = [("s_vec", F64P), ("obj_trace", F64P), ("avg_change_trace", F64P), ("w", F64P), ("adam_m", F64P), ("adam_v", F64P),
                ("iters_run", I32P), ("t_end", I32P), ("ms_structure", C.c_double), ("ms_upload", C.c_double), ("ms_cycle_d", C.c_double),
                ("ms_pgd", C.c_double), ("ms_total", C.c_double)]


class ShardInfo(C.Structure):
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("t_len", C.c_int64), ("t_part", C.c_int64), ("slice_len", C.c_int64),
                ("seg_lo", C.c_int64), ("seg_hi", C.c_int64), ("cyc_lo", C.c_int64), ("cyc_hi", C.c_int64),
                ("m_pos", C.c_int64), ("m_cycle", C.c_int64), ("xparts", C.c_int32), ("reserved", C.c_int32)]


RS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p)     # ncclReduceScatter
AG_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p)              # ncclAllGather


class Collectives(C.Structure):
    _fields_ = [("comm", C.c_void_p), ("reduce_scatter", C.c_void_p), ("all_gather", C.c_void_p)]


class SpectralInfo(C.Structure):
    _fields_ = [("iters", C.c_int32), ("products", C.c_int32), ("converged", C.c_int32), ("reserved", C.c_int32), ("residual", C.c_double),
                ("eigenvalues", C.c_double * 3), ("ms_total", C.c_double)]


class GcwBatchTimings(C.Structure):
    _fields_ = [("ms_structure", C.c_double), ("ms_upload", C.c_double), ("ms_eig", C.c_double), ("ms_project", C.c_double),
                ("ms_total", C.c_double)]


class CempBatchTimings(C.Structure):
    _fields_ = [("ms_structure", C.c_double), ("ms_upload", C.c_double), ("ms_build", C.c_double), ("ms_rounds", C.c_double),
                ("ms_total", C.c_double)]


class MstBatchTimings(C.Structure):
    _fields_ = [("ms_structure", C.c_double), ("ms_upload", C.c_double), ("ms_tree", C.c_double), ("ms_propagate", C.c_double),
                ("ms_total", C.c_double)]


class RefineBatchTimings(C.Structure):
    _fields_ = [("ms_structure", C.c_double), ("ms_upload", C.c_double), ("ms_input", C.c_double), ("ms_refine", C.c_double),
                ("ms_total", C.c_double)]


class MplsBatchTimings(C.Structure):
    _fields_ = [("ms_setup", C.c_double), ("ms_input", C.c_double), ("ms_loop", C.c_double), ("ms_download", C.c_double),
                ("ms_total", C.c_double)]


class IrlsBatchTimings(C.Structure):
    _fields_ = [("ms_structure", C.c_double), ("ms_upload", C.c_double), ("ms_project", C.c_double), ("ms_solve", C.c_double),
                ("ms_total", C.c_double)]


class LpBatchTimings(C.Structure):
    _fields_ = [("ms_structure", C.c_double), ("ms_upload", C.c_double), ("ms_build", C.c_double), ("ms_loop", C.c_double),
                ("ms_total", C.c_double)]


class ModelSpec(C.Structure):
    _fields_ = [("kind", C.c_int32), ("n", C.c_int32), ("p", C.c_double), ("q", C.c_double), ("p_node_crpt", C.c_double),
                ("p_edge_crpt", C.c_double), ("sigma", C.c_double), ("sigma_in", C.c_double), ("sigma_out", C.c_double),
                ("mode", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64)]


class ModelsBatchTimings(C.Structure):
    _fields_ = [("ms_graph", C.c_double), ("ms_nodes", C.c_double), ("ms_edges", C.c_double), ("ms_copy", C.c_double),
                ("ms_total", C.c_double)]


class AlignBatchTimings(C.Structure):
    _fields_ = [("ms_upload", C.c_double), ("ms_align", C.c_double), ("ms_copy", C.c_double), ("ms_total", C.c_double)]


class RefineInfo(C.Structure):
    _fields_ = [("iters", C.c_int32), ("cg_iters", C.c_int32), ("verbose", C.c_int32), ("cg_unconverged", C.c_int32),
                ("score", C.c_double), ("ms_total", C.c_double), ("cg_residual", C.c_double)]


class MplsParams(C.Structure):
    _fields_ = [("cemp_beta", F64P), ("n_cemp_beta", C.c_int32), ("cemp_max_iter", C.c_int32), ("nsample", C.c_int32), ("verbose", C.c_int32),
                ("seed", C.c_uint64), ("stop_threshold", C.c_double), ("max_iter", C.c_int32), ("n_beta", C.c_int32), ("beta", F64P),
                ("tau", F64P), ("alpha", F64P), ("n_tau", C.c_int32), ("n_alpha", C.c_int32)]


class MplsInfo(C.Structure):
    _fields_ = [("iters", C.c_int32), ("cg_iters", C.c_int32), ("cg_unconverged", C.c_int32), ("reserved", C.c_int32), ("m_pos", C.c_int64),
                ("score", C.c_double), ("cg_residual", C.c_double), ("ms_cemp", C.c_double), ("ms_mst", C.c_double), ("ms_loop", C.c_double),
                ("ms_total", C.c_double)]


class IrlsParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("max_iter_l1", C.c_int32), ("max_iter_irls", C.c_int32), ("verbose", C.c_int32), ("sigma_deg", C.c_double),
                ("R_init", F64P), ("order", I32P)]


class IrlsInfo(C.Structure):
    _fields_ = [("comp_nodes", C.c_int64), ("comp_edges", C.c_int64), ("l1_iters", C.c_int32), ("irls_iters", C.c_int32),
                ("l1_score", C.c_double), ("irls_score", C.c_double), ("pd_steps", C.c_int32), ("pd_ill", C.c_int32), ("pd_stuck", C.c_int32),
                ("warned_edges", C.c_int32), ("cg_iters_l1", C.c_int32), ("cg_iters_irls", C.c_int32), ("cg_unconverged", C.c_int32),
                ("pd_solves", C.c_int32), ("cg_residual", C.c_double), ("ms_project", C.c_double), ("ms_components", C.c_double),
                ("ms_tree", C.c_double), ("ms_l1", C.c_double), ("ms_l1_pcg", C.c_double), ("ms_irls", C.c_double), ("ms_total", C.c_double)]


class LpParams(C.Structure):
    _fields_ = [("nsample", C.c_int32), ("check_every", C.c_int32), ("seed", C.c_uint64), ("tol", C.c_double), ("max_iter", C.c_int32),
                ("restart", C.c_int32), ("verbose", C.c_int32), ("reserved", C.c_int32), ("pos_out", I32P)]


class LpInfo(C.Structure):
    _fields_ = [("nsample", C.c_int32), ("iters", C.c_int32), ("restarts", C.c_int32), ("converged", C.c_int32), ("m_pos", C.c_int64),
                ("rows", C.c_int64), ("viol", C.c_double), ("pobj", C.c_double), ("dobj", C.c_double), ("ms_samples", C.c_double),
                ("ms_transpose", C.c_double), ("ms_loop", C.c_double), ("ms_col", C.c_double), ("ms_row", C.c_double), ("ms_total", C.c_double)]


IRLS_GM, IRLS_L12 = 0, 1
ERR_INVALID, ERR_HIP, ERR_TOO_LARGE, ERR_STATE = -1, -2, -3, -4


class DescError(RuntimeError):
    """Carries the C return code (``code``): callers branch on it, not on the message text."""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


_lib = None


def load():
    """Load libdesc_amd.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DescError(
            f"{LIB_PATH} is missing: build it with `python -m desc_amd.build` (hipcc, gfx950). "
            "The DESC_PGD hot path has no CPU fallback.")
    # PyTorch bundles a ROCm runtime with the same sonames as /opt/rocm; a process can hold only
    # one copy and torch needs its own.  Callers that use torch next to this library (the
    # multi-GPU driver) import torch first, or set DESC_AMD_PRELOAD_TORCH=1.
    if os.environ.get("DESC_AMD_PRELOAD_TORCH") == "1":
        import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    L.desc_last_error.restype = C.c_char_p
    L.desc_version.restype = C.c_char_p
    L.desc_pgd_kernel_name.restype = C.c_char_p
    L.desc_pgd_kernel_name.argtypes = [C.c_void_p]
    L.desc_sample_key.restype = C.c_uint64
    L.desc_sample_key.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
    L.desc_params_default.argtypes = [C.POINTER(Params)]
    L.desc_params_default.restype = None
    L.desc_structure_build.argtypes = [C.POINTER(Problem), C.c_int32, C.c_uint64, C.c_int32, C.c_int32,
                                       C.POINTER(C.c_void_p)]
    L.desc_structure_import.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int32, I32P, I64P, I32P, I32P,
                                        I32P, I32P, I32P, C.POINTER(C.c_void_p)]
    L.desc_structure_get.argtypes = [C.c_void_p, C.POINTER(StructureView)]
    L.desc_structure_sizes.argtypes = [C.c_void_p, C.POINTER(StructureInfo)]
    L.desc_structure_host_exports.restype = C.c_int64
    L.desc_structure_host_exports.argtypes = []
    L.desc_structure_free.argtypes = [C.c_void_p]
    L.desc_structure_free.restype = None
    L.desc_pgd_create.argtypes = [C.POINTER(Problem), C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    L.desc_pgd_destroy.argtypes = [C.c_void_p]
    L.desc_pgd_destroy.restype = None
    L.desc_pgd_run.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Result)]
    L.desc_pgd_run_traced.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Params), F64P, C.c_double, C.c_int32, F64P, F64P, C.POINTER(Result)]
    L.desc_pgd_reset.argtypes = [C.c_void_p, C.POINTER(Params)]
    L.desc_pgd_iterate.argtypes = [C.c_void_p, C.c_int32]
    L.desc_pgd_iterate_timed.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.desc_pgd_sync.argtypes = [C.c_void_p]
    L.desc_pgd_download.argtypes = [C.c_void_p, C.POINTER(Result)]
    L.desc_pgd_ext_begin.argtypes = [C.c_void_p, C.POINTER(Params)]
    L.desc_pgd_ext_grad.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    L.desc_pgd_ext_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, F64P, F64P, I32P]
    L.desc_pgd_ext_laps.argtypes = [C.c_void_p, F64P]
    L.desc_pgd_get_s0.argtypes = [C.c_void_p, F64P]
    L.desc_pgd_sizes.argtypes = [C.c_void_p, I64P, I64P, I64P, I32P]
    L.desc_pgd_solve.argtypes = [C.POINTER(Problem), C.POINTER(Params), C.POINTER(Result)]
    L.desc_marshal_edges.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64, I32P, I32P, I64P, I32P]
    L.desc_marshal_rij.argtypes = [F64P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, I64P, F64P]
    L.desc_pgd_create_shard.argtypes = [C.POINTER(Problem), C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.desc_pgd_shard_info.argtypes = [C.c_void_p, C.POINTER(ShardInfo)]
    L.desc_pgd_shard_bind.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.desc_pgd_shard_colsum.argtypes = [C.c_void_p]
    L.desc_pgd_shard_sweep.argtypes = [C.c_void_p]
    L.desc_pgd_shard_finish.argtypes = [C.c_void_p, C.c_int32]
    L.desc_pgd_shard_objective.argtypes = [C.c_void_p, C.c_int32]
    L.desc_pgd_stopped.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.desc_pgd_shard_set_collectives.argtypes = [C.c_void_p, C.POINTER(Collectives)]
    L.desc_pgd_shard_start.argtypes = [C.c_void_p, C.POINTER(Params)]
    L.desc_pgd_shard_iterate.argtypes = [C.c_void_p, C.c_int32]
    L.desc_pgd_shard_run.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Result)]
    L.desc_debug_band_plan.argtypes = [C.POINTER(Problem), C.c_void_p, C.c_int32, C.c_int32, C.c_int32, I64P]
    L.desc_debug_spmm_variants.argtypes = [C.c_void_p, C.c_int32, F64P]
    L.desc_debug_wg_clock.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int32]
    L.desc_debug_wg_plan.argtypes = [C.c_void_p, I64P, C.c_int32]
    L.desc_pgd_layout_stats.argtypes = [C.c_void_p, I64P, C.c_int32]
    L.desc_debug_last_sweep.restype = C.c_char_p
    L.desc_debug_last_sweep.argtypes = [C.c_void_p]
    L.desc_debug_shard_layout.argtypes = [C.c_void_p, I32P, I32P, I32P, I32P]
    L.desc_trim_memory.restype = C.c_int64
    L.desc_trim_memory.argtypes = []
    L.desc_device_synchronize.argtypes = [C.c_int32]
    L.desc_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.desc_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.desc_spectral_run.argtypes = [C.POINTER(Problem), F64P, C.c_int32, C.c_double, C.c_int32, C.c_int32, F64P,
                                    C.POINTER(SpectralInfo)]
    L.desc_problem_upload.argtypes = [C.POINTER(Problem), C.c_int32, C.POINTER(C.c_void_p)]
    L.desc_problem_free.argtypes = [C.c_void_p]
    L.desc_problem_free.restype = None
    L.desc_spectral_run_dev.argtypes = [C.c_void_p, F64P, C.c_int32, C.c_double, C.c_int32, F64P, C.POINTER(SpectralInfo)]
    L.desc_gcw_run_dev.argtypes = [C.c_void_p, F64P, C.c_double, C.c_int32, F64P, C.POINTER(SpectralInfo)]
    L.desc_cemp_run_dev.argtypes = [C.c_void_p, F64P, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, F64P, C.POINTER(C.c_double)]
    L.desc_refine_run_dev.argtypes = [C.c_void_p, F64P, F64P, C.c_double, C.c_int32, F64P, C.POINTER(RefineInfo)]
    L.desc_pgd_create_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.desc_cemp_run.argtypes = [C.POINTER(Problem), F64P, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, F64P,
                                C.POINTER(C.c_double)]
    L.desc_refine_run.argtypes = [C.POINTER(Problem), F64P, F64P, C.c_double, C.c_int32, C.c_int32, F64P, C.POINTER(RefineInfo)]
    L.desc_mst_run.argtypes = [C.POINTER(Problem), F64P, C.c_int32, F64P, I32P]
    L.desc_mst_run_dev.argtypes = [C.c_void_p, F64P, F64P, I32P]
    L.desc_mpls_run.argtypes = [C.POINTER(Problem), C.POINTER(MplsParams), C.c_int32, F64P, F64P, F64P, C.POINTER(MplsInfo)]
    L.desc_mpls_run_dev.argtypes = [C.c_void_p, C.POINTER(MplsParams), F64P, F64P, F64P, C.POINTER(MplsInfo)]
    L.desc_irls_run.argtypes = [C.POINTER(Problem), C.POINTER(IrlsParams), C.c_int32, F64P, F64P, C.POINTER(IrlsInfo)]
    L.desc_irls_run_dev.argtypes = [C.c_void_p, C.POINTER(IrlsParams), F64P, F64P, C.POINTER(IrlsInfo)]
    L.desc_lp_params_default.argtypes = [C.POINTER(LpParams)]
    L.desc_lp_params_default.restype = None
    L.desc_lp_sij_run.argtypes = [C.POINTER(Problem), C.POINTER(LpParams), C.c_int32, F64P, F64P, I32P, C.POINTER(LpInfo)]
    L.desc_lp_sij_run_dev.argtypes = [C.c_void_p, C.POINTER(LpParams), F64P, F64P, I32P, C.POINTER(LpInfo)]
    L.desc_pgd_batch_create.argtypes = [C.POINTER(Problem), C.c_int32, C.POINTER(Params), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p)]
    L.desc_pgd_batch_create_where.argtypes = [C.POINTER(Problem), C.c_int32, C.POINTER(Params), C.POINTER(C.c_uint64), C.c_int32, C.POINTER(C.c_void_p)]
    L.desc_pgd_batch_built_where.argtypes = [C.c_void_p]
    L.desc_pgd_batch_built_where.restype = C.c_int32
    L.desc_pgd_batch_max_codeg.argtypes = []
    L.desc_pgd_batch_max_codeg.restype = C.c_int32
    L.desc_pgd_batch_build_laps.argtypes = [C.c_void_p, F64P]
    L.desc_test_batch_plan.argtypes = [I32P, C.c_int32, C.c_int32, I64P]
    L.desc_pgd_batch_sizes.argtypes = [C.c_void_p, I32P, I64P, I64P, I32P]
    L.desc_pgd_batch_get_structure.argtypes = [C.c_void_p, C.c_int32, C.POINTER(StructureView)]
    L.desc_pgd_batch_get_s0.argtypes = [C.c_void_p, F64P]
    L.desc_pgd_batch_run.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(BatchResult)]
    L.desc_pgd_batch_destroy.argtypes = [C.c_void_p]
    L.desc_pgd_batch_destroy.restype = None
    L.desc_pgd_batch_concat.argtypes = [C.POINTER(C.c_void_p), C.c_int32, I64P, I64P, I64P, I32P, I32P, I32P, I32P, I32P, I32P]
    L.desc_gcw_batch_max_n.restype = C.c_int32
    L.desc_gcw_batch_max_n.argtypes = []
    L.desc_gcw_batch_create.argtypes = [C.POINTER(Problem), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.desc_gcw_batch_streamed_max_n.restype = C.c_int32
    L.desc_gcw_batch_streamed_max_n.argtypes = []
    L.desc_gcw_batch_create_where.argtypes = [C.POINTER(Problem), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.desc_gcw_batch_sizes.argtypes = [C.c_void_p, I32P, I64P, I64P]
    L.desc_gcw_batch_csr.argtypes = [C.POINTER(Problem), C.c_int32, I64P, I64P, I32P, I32P, I32P]
    L.desc_gcw_batch_run.argtypes = [C.c_void_p, F64P, F64P, C.c_int32, C.c_double, C.c_int32, F64P, C.POINTER(SpectralInfo),
                                     C.POINTER(GcwBatchTimings)]
    L.desc_gcw_batch_destroy.argtypes = [C.c_void_p]
    L.desc_gcw_batch_destroy.restype = None
    L.desc_cemp_batch_max_degree.restype = C.c_int32
    L.desc_cemp_batch_max_degree.argtypes = []
    L.desc_cemp_batch_create.argtypes = [C.POINTER(Problem), C.c_int32, C.c_int32, C.c_uint64, C.POINTER(C.c_uint64), C.c_int32,
                                         C.POINTER(C.c_void_p)]
    L.desc_cemp_batch_sizes.argtypes = [C.c_void_p, I32P, I64P, I64P]
    L.desc_cemp_batch_get_samples.argtypes = [C.c_void_p, I32P, I32P, F64P, C.POINTER(C.c_uint8)]
    L.desc_cemp_batch_run.argtypes = [C.c_void_p, F64P, C.c_int32, C.c_int32, F64P, C.POINTER(CempBatchTimings)]
    L.desc_cemp_batch_destroy.argtypes = [C.c_void_p]
    L.desc_cemp_batch_destroy.restype = None
    L.desc_mst_batch_max_n.restype = C.c_int32
    L.desc_mst_batch_max_n.argtypes = []
    L.desc_mst_batch_check.argtypes = [C.POINTER(Problem), C.c_int32]
    L.desc_mst_batch_run.argtypes = [C.POINTER(Problem), C.c_int32, F64P, C.c_int32, F64P, I32P, C.POINTER(MstBatchTimings)]
    L.desc_refine_batch_max_n.restype = C.c_int32
    L.desc_refine_batch_max_n.argtypes = []
    L.desc_refine_batch_create.argtypes = [C.POINTER(Problem), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.desc_refine_batch_sizes.argtypes = [C.c_void_p, I32P, I64P, I64P]
    L.desc_refine_batch_run.argtypes = [C.c_void_p, F64P, F64P, C.c_double, C.c_int32, F64P, C.POINTER(RefineInfo), C.POINTER(RefineBatchTimings)]
    L.desc_refine_batch_destroy.argtypes = [C.c_void_p]
    L.desc_refine_batch_destroy.restype = None
    L.desc_mpls_batch_max_n.restype = C.c_int32
    L.desc_mpls_batch_max_n.argtypes = []
    L.desc_mpls_batch_run.argtypes = [C.c_void_p, F64P, F64P, C.c_double, C.c_int32, F64P, C.c_int32, F64P, C.c_int32, F64P, C.c_int32, F64P,
                                      C.POINTER(MplsInfo), C.POINTER(MplsBatchTimings)]
    L.desc_irls_batch_max_n.restype = C.c_int32
    L.desc_irls_batch_max_n.argtypes = []
    L.desc_irls_batch_create.argtypes = [C.POINTER(Problem), C.c_int32, C.POINTER(I32P), C.c_int32, C.POINTER(C.c_void_p)]
    L.desc_irls_batch_sizes.argtypes = [C.c_void_p, I32P, I64P, I64P]
    L.desc_irls_batch_run.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_int32, F64P, F64P, C.POINTER(IrlsInfo),
                                      C.POINTER(IrlsBatchTimings)]
    L.desc_irls_batch_destroy.argtypes = [C.c_void_p]
    L.desc_irls_batch_destroy.restype = None
    L.desc_irls_tree_sequence.argtypes = [C.POINTER(Problem), I32P, I32P, I64P]
    L.desc_lp_batch_plan.argtypes = [C.POINTER(Problem), C.c_int32, I32P, I32P, I64P, I64P, I64P, I32P, I32P]
    L.desc_lp_batch_create.argtypes = [C.POINTER(Problem), C.c_int32, I32P, C.POINTER(C.c_uint64), C.c_int32, C.POINTER(C.c_void_p)]
    L.desc_lp_batch_sizes.argtypes = [C.c_void_p, I32P, I64P, I64P, I32P, I64P, I64P, I64P]
    L.desc_lp_batch_get_samples.argtypes = [C.c_void_p, I32P, I32P]
    L.desc_lp_batch_run.argtypes = [C.c_void_p, C.POINTER(LpParams), F64P, F64P, C.POINTER(LpInfo), C.POINTER(LpBatchTimings)]
    L.desc_lp_batch_destroy.argtypes = [C.c_void_p]
    L.desc_lp_batch_destroy.restype = None
    L.desc_models_key.restype = C.c_uint64
    L.desc_models_key.argtypes = [C.c_uint64] * 5
    L.desc_models_batch_max_n.restype = C.c_int32
    L.desc_models_batch_max_n.argtypes = []
    L.desc_models_batch_create.argtypes = [C.POINTER(ModelSpec), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.desc_models_batch_sizes.argtypes = [C.c_void_p, I64P]
    L.desc_models_batch_fetch.argtypes = [C.c_void_p, I32P, I32P, F64P, F64P, F64P, F64P, C.POINTER(C.c_uint8), C.POINTER(ModelsBatchTimings)]
    L.desc_models_batch_destroy.argtypes = [C.c_void_p]
    L.desc_models_batch_destroy.restype = None
    L.desc_test_models_uniform.argtypes = [C.c_uint64] * 4 + [C.c_int64, C.c_uint64, C.c_int32, F64P]
    L.desc_test_models_normal.argtypes = [C.c_uint64] * 4 + [C.c_int64, C.c_uint64, C.c_int32, F64P]
    L.desc_align_batch_create.argtypes = [I32P, F64P, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.desc_align_batch_sizes.argtypes = [C.c_void_p, I32P, I64P]
    L.desc_align_batch_run.argtypes = [C.c_void_p, F64P, F64P, F64P, F64P, F64P, F64P, C.POINTER(AlignBatchTimings)]
    L.desc_align_batch_destroy.argtypes = [C.c_void_p]
    L.desc_align_batch_destroy.restype = None
    L.desc_test_align_project.argtypes = [F64P, C.c_int64, C.c_int32, F64P]
    L.desc_problem_batch_create.argtypes = [C.POINTER(Problem), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.desc_problem_batch_from_models.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.desc_problem_batch_sizes.argtypes = [C.c_void_p, I32P, I64P, I64P]
    L.desc_problem_batch_fetch.argtypes = [C.c_void_p, I32P, I32P, F64P, I32P, I32P, I32P]
    L.desc_problem_batch_built_where.argtypes = [C.c_void_p]
    L.desc_problem_batch_built_where.restype = C.c_int32
    L.desc_problem_batch_destroy.argtypes = [C.c_void_p]
    L.desc_problem_batch_destroy.restype = None
    L.desc_gcw_batch_create_on.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    L.desc_refine_batch_create_on.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.desc_pgd_batch_create_on.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(C.c_uint64), C.c_int32, C.POINTER(C.c_void_p)]
    L.desc_cemp_batch_create_on.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_void_p)]
    L.desc_irls_batch_create_on.argtypes = [C.c_void_p, C.POINTER(I32P), C.POINTER(C.c_void_p)]
    L.desc_mst_batch_run_on.argtypes = [C.c_void_p, F64P, F64P, I32P, C.POINTER(MstBatchTimings), I64P]
    for kind in ("problem", "gcw", "refine", "pgd", "cemp", "irls"):
        getattr(L, f"desc_{kind}_batch_bytes").argtypes = [C.c_void_p, I64P, I64P]
    L.desc_test_laa_r2q.argtypes = [F64P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, F64P]
    L.desc_test_laa_q2r.argtypes = [F64P, C.c_int64, C.c_int32, F64P]
    L.desc_test_laa_edge_log.argtypes = [C.c_void_p, F64P, F64P, C.c_int64, F64P]
    L.desc_test_laa_rhs.argtypes = [C.c_void_p, F64P, F64P, C.c_int64, F64P, F64P]
    L.desc_test_laa_pcg.argtypes = [C.c_void_p, C.c_int32, F64P, F64P, F64P, C.c_int64, I32P, F64P, I32P, F64P, F64P, I32P, I32P, F64P]
    L.desc_test_laa_node_update.argtypes = [F64P, F64P, C.c_int64, C.c_int32, F64P, F64P, F64P]
    L.desc_test_irls_node_update.argtypes = [F64P, F64P, C.c_int64, C.c_int32, F64P, F64P]
    L.desc_test_laa_weights.argtypes = [F64P, C.c_int64, C.c_double, C.c_int32, F64P]
    L.desc_test_irls_weights.argtypes = [C.c_void_p, F64P, F64P, C.c_int64, C.c_int32, C.c_double, F64P]
    L.desc_test_laa_quantile.argtypes = [F64P, C.c_int64, C.c_double, C.c_int64, C.c_int32, F64P]
    L.desc_test_irls_project.argtypes = [F64P, I32P, C.c_int64, C.c_int64, C.c_int32, F64P, I32P, I32P, F64P]
    L.desc_test_irls_pd_stage.argtypes = [C.c_void_p, C.c_int32, F64P, F64P, F64P, I32P, C.c_int64, C.c_int64, F64P, F64P, F64P]
    L.desc_test_irls_pd_solve.argtypes = [C.c_void_p, F64P, C.c_int64, C.c_int64, C.c_int32, F64P, F64P, I32P, F64P, C.c_int32, I32P]
    L.desc_test_spectral_weights.argtypes = [F64P, C.c_int64, C.c_int32, F64P]
    L.desc_test_spectral_row_wsum.argtypes = [C.c_void_p, F64P, C.c_int64, C.c_int32, F64P]
    L.desc_test_spectral_assemble.argtypes = [C.c_void_p, F64P, F64P, C.c_int64, C.c_int32, F64P]
    L.desc_test_spectral_spmm.argtypes = [C.c_void_p, F64P, F64P, F64P, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, F64P]
    L.desc_test_spectral_gram.argtypes = [F64P, F64P, C.c_int64, C.c_int32, C.c_int32, F64P, F64P]
    L.desc_test_spectral_residual.argtypes = [F64P, F64P, C.c_int64, F64P, F64P, C.c_int32, C.c_int32, F64P]
    L.desc_test_spectral_combine.argtypes = [F64P, C.c_int64, F64P, C.c_int32, C.c_int32, F64P]
    L.desc_test_small_jacobi.argtypes = [C.c_int32, F64P, F64P, F64P]
    L.desc_test_small_ortho.argtypes = [F64P, F64P, F64P, I32P]
    L.desc_test_small_project.argtypes = [F64P, C.c_int64, F64P]
    L.desc_test_small_ritz_tail.argtypes = [F64P, F64P, C.c_int64, F64P]
    _lib = L
    return L


# ---- DESC_DEBUG_GUARD=1 (diagnostics; tests/conftest.py turns it on): every buffer this module hands to the library to be
# written is fenced by 64 bytes of guard words on both sides, and every fence still alive is verified after each native call --
# a write past a caller buffer (or a late write into an older one) is reported at the call that made it.
GUARD = os.environ.get("DESC_DEBUG_GUARD") == "1"
_FENCE = 64
_FENCE_BYTE = 0xA5
_fences = []          # weak references to the fenced base arrays


def out_buffer(count, dtype=np.float64):
    """Zeroed output buffer for the library to fill (count >= 1 elements)."""
    count = max(int(count), 1)
    if not GUARD:
        return np.zeros(count, dtype=dtype)
    import weakref
    nbytes = count * np.dtype(dtype).itemsize
    base = np.zeros(nbytes + 2 * _FENCE, dtype=np.uint8)
    base[:_FENCE] = _FENCE_BYTE
    base[_FENCE + nbytes:] = _FENCE_BYTE
    _fences.append(weakref.ref(base))
    return base[_FENCE:_FENCE + nbytes].view(dtype)


def verify_guards():
    """Check the fences of every live guarded buffer; raises DescError(ERR_STATE) naming the damaged side."""
    if not _fences:
        return
    live = []
    for r in _fences:
        base = r()
        if base is None:
            continue
        live.append(r)
        lo, hi = base[:_FENCE], base[base.size - _FENCE:]
        if (lo != _FENCE_BYTE).any() or (hi != _FENCE_BYTE).any():
            side = "before" if (lo != _FENCE_BYTE).any() else "after"
            raise DescError(f"DESC_DEBUG_GUARD: native code wrote {side} a caller buffer of {base.size - 2 * _FENCE} bytes", ERR_STATE)
    _fences[:] = live


def check(rc):
    if GUARD:
        verify_guards()
    if rc != DESC_OK:
        raise DescError(f"desc_amd error {rc}: {load().desc_last_error().decode()}", rc)


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def default_params():
    p = Params()
    load().desc_params_default(C.byref(p))
    return p


class ProblemArrays:
    """Keeps the NumPy buffers behind a desc_problem alive."""

    def __init__(self, n, ind_i, ind_j, rij=None):
        self.ind_i = np.ascontiguousarray(ind_i, dtype=np.int32)
        self.ind_j = np.ascontiguousarray(ind_j, dtype=np.int32)
        self.rij = None if rij is None else np.ascontiguousarray(rij, dtype=np.float64).reshape(-1)
        m = self.ind_i.shape[0]
        self.n, self.m = int(n), int(m)
        if self.rij is not None and self.rij.shape[0] != 9 * m:
            raise ValueError("rij must hold m*9 doubles")
        self.c = Problem(int(n), m, ptr(self.ind_i, I32P), ptr(self.ind_j, I32P), ptr(self.rij, F64P))


class DeviceProblem:
    """Owner of a desc_device_problem*: Ind / RijMat / CSR index resident in HBM, shared by every stage of DESC()."""

    def __init__(self, prob: ProblemArrays, device=0):
        h = C.c_void_p()
        check(load().desc_problem_upload(C.byref(prob.c), device, C.byref(h)))
        self.handle, self.prob, self.device = h, prob, device
        self.n, self.m = prob.n, prob.m

    def free(self):
        if self.handle:
            load().desc_problem_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _view_arrays(v: StructureView):
    def arr(p, count, dt):
        if count == 0:
            return np.zeros(0, dtype=dt)
        return np.ctypeslib.as_array(p, shape=(count,)).copy()

    return dict(n=v.n, m=v.m, m_pos=v.m_pos, m_cycle=v.m_cycle, n_sample=v.n_sample, max_cnt=v.max_cnt,
                codeg=arr(v.codeg, v.m, np.int32), pos_edge=arr(v.pos_edge, v.m_pos, np.int32),
                cum_ind=arr(v.cum_ind, v.m_pos + 1, np.int64), k=arr(v.k, v.m_cycle, np.int32),
                e_jk=arr(v.e_jk, v.m_cycle, np.int32), e_ki=arr(v.e_ki, v.m_cycle, np.int32),
                ikj=arr(v.ikj, v.m_cycle, np.int32), jki=arr(v.jki, v.m_cycle, np.int32))


class Structure:
    """Owner of a desc_structure*."""

    def __init__(self, handle):
        self.handle = handle

    @classmethod
    def build(cls, prob: ProblemArrays, n_sample_min=30, seed=0, where=BUILD_HOST, device=0):
        h = C.c_void_p()
        check(load().desc_structure_build(C.byref(prob.c), n_sample_min, seed, where, device, C.byref(h)))
        return cls(h)

    @classmethod
    def from_arrays(cls, n, m, n_sample, pos_edge, cum_ind, k, e_jk, e_ki, ikj, jki):
        a = [np.ascontiguousarray(x, dtype=np.int32) for x in (pos_edge, k, e_jk, e_ki, ikj, jki)]
        cum = np.ascontiguousarray(cum_ind, dtype=np.int64)
        h = C.c_void_p()
        check(load().desc_structure_import(int(n), int(m), a[0].shape[0], int(n_sample), ptr(a[0], I32P),
                                           ptr(cum, I64P), ptr(a[1], I32P), ptr(a[2], I32P), ptr(a[3], I32P),
                                           ptr(a[4], I32P), ptr(a[5], I32P), C.byref(h)))
        return cls(h)

    def arrays(self):
        v = StructureView()
        check(load().desc_structure_get(self.handle, C.byref(v)))
        return _view_arrays(v)

    def sizes(self):
        """O(1): never exports a device-built structure to the host (desc_structure_sizes)."""
        v = StructureInfo()
        check(load().desc_structure_sizes(self.handle, C.byref(v)))
        return dict(n=v.n, m=v.m, m_pos=v.m_pos, m_cycle=v.m_cycle, n_sample=v.n_sample, max_cnt=v.max_cnt,
                    built_where=v.built_where, host_resident=bool(v.host_resident), ms_build=v.ms_build)

    def free(self):
        if self.handle:
            load().desc_structure_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _problem_array(probs):
    """The desc_problem array of a list of ProblemArrays (one spare entry for an empty list: ctypes has no array of length 0)."""
    return (Problem * max(len(probs), 1))(*[q.c for q in probs])


def _seeds_array(seeds, B):
    """Per-problem sampling seeds as a uint64 array, or None."""
    if seeds is None:
        return None
    if len(seeds) != B:
        raise ValueError(f"seeds must hold one entry per problem ({B}), not {len(seeds)}")
    return (C.c_uint64 * max(B, 1))(*[int(x) for x in seeds])


def _split_R(R, node_off):
    """The per-problem (3,3,n_b) Fortran-ordered views of the concatenated rotations."""
    return [R[9 * int(n0):9 * int(n1)].reshape((3, 3, int(n1 - n0)), order="F") for n0, n1 in zip(node_off[:-1], node_off[1:])]


def _timings(tm):
    """The ms_* fields of a timings (or result) structure as a dict."""
    return {name: getattr(tm, name) for name, _ in tm._fields_ if name.startswith("ms_")}


class _BatchHandle:
    """Base of the owners of a batched handle desc_<_kind>_batch*.  A subclass's constructor calls _open with the arguments of its
    create call that stand between ``count`` and ``out``; Batch, whose offsets are others, also overrides _read_sizes, and names
    another create call."""
    _kind = None
    _create = "create"
    handle = None

    def _export(self, name):
        return getattr(load(), f"desc_{self._kind}_batch_{name}")

    def _open(self, probs, *create_args):
        self.probs = list(probs)                     # keeps the NumPy buffers alive
        self.count = B = len(self.probs)
        h = C.c_void_p()
        check(self._export(self._create)(_problem_array(self.probs), B, *create_args, C.byref(h)))
        self.handle = h
        self._read_sizes(B)

    def _open_on(self, pset, *create_args):
        """As _open on a resident ProblemBatch: desc_<_kind>_batch_create_on; the handle keeps the set's device arrays alive."""
        if not pset.handle:
            raise ValueError("the ProblemBatch is closed")
        self.probs = pset.probs                      # the set's host mirror (endpoints; rotations only where they are on the host)
        self.count = B = len(pset)
        h = C.c_void_p()
        check(self._export("create_on")(pset.handle, *create_args, C.byref(h)))
        self.handle = h
        self._read_sizes(B)

    def bytes(self):
        """(h2d, d2h): the bytes the handle's device half copied up through its create and down (desc_<_kind>_batch_bytes)."""
        up, down = C.c_int64(), C.c_int64()
        check(self._export("bytes")(self.handle, C.byref(up), C.byref(down)))
        return int(up.value), int(down.value)

    def _read_sizes(self, B):
        no, eo = np.zeros(B + 1, dtype=np.int64), np.zeros(B + 1, dtype=np.int64)
        check(self._export("sizes")(self.handle, None, ptr(no, I64P), ptr(eo, I64P)))
        self.node_off, self.edge_off = no, eo
        self.n, self.m = int(no[B]), int(eo[B])

    def destroy(self):
        if self.handle:
            self._export("destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Batch(_BatchHandle):
    """Owner of a desc_pgd_batch*: B independent problems behind one another in one set of device arrays (desc_pgd_batch_*).
    ``probs`` is a sequence of ProblemArrays; ``seeds`` an optional sequence of per-problem sampling seeds; ``where`` the builder
    of the cycle structure (BUILD_HOST, or BUILD_DEVICE: desc_pgd_batch_create_where).  ``built_where`` is the builder that made the
    handle: BUILD_HOST also where a batch outside the device builder's staging caps fell back to the host."""

    _kind = "pgd"
    _create = "create_where"
    BUILD_LAPS = ("codeg", "plan", "compact", "sample", "mirror")

    def __init__(self, probs, params: Params, seeds=None, where=BUILD_HOST, on=None):
        if on is not None:                           # a resident ProblemBatch: probs is not read
            self._open_on(on, C.byref(params), _seeds_array(seeds, len(on)), int(where))
        else:
            probs = list(probs)
            self._open(probs, C.byref(params), _seeds_array(seeds, len(probs)), int(where))
        self.built_where = int(self._export("built_where")(self.handle))

    def build_laps(self):
        """Device time (ms) of the device builder's five launches, by name; zeros for a host-built handle."""
        out = np.zeros(len(self.BUILD_LAPS))
        check(load().desc_pgd_batch_build_laps(self.handle, ptr(out, F64P)))
        return dict(zip(self.BUILD_LAPS, out.tolist()))

    def _read_sizes(self, B):
        eo, co, ns = np.zeros(B + 1, dtype=np.int64), np.zeros(B + 1, dtype=np.int64), np.zeros(max(B, 1), dtype=np.int32)
        check(self._export("sizes")(self.handle, None, ptr(eo, I64P), ptr(co, I64P), ptr(ns, I32P)))
        self.edge_off, self.cycle_off, self.n_sample = eo, co, ns[:B]
        self.m, self.m_cycle = int(eo[B]), int(co[B])

    def structure(self, b):
        v = StructureView()
        check(load().desc_pgd_batch_get_structure(self.handle, b, C.byref(v)))
        return _view_arrays(v)

    def s0(self):
        """S0_long of every problem (a list of per-problem vectors)."""
        out = out_buffer(self.m_cycle)
        check(load().desc_pgd_batch_get_s0(self.handle, ptr(out, F64P)))
        return [out[self.cycle_off[b]:self.cycle_off[b + 1]] for b in range(self.count)]

    def run(self, params: Params, want_w=False, adam=None):
        """One batched run.  adam: (m_t, v_t), two writable contiguous float64 arrays of cycle_off[count] entries, read when
        params.t0 > 0 and written.  Returns a list of per-problem dicts (views of the concatenated buffers) and the call's timings."""
        B, iters = self.count, int(params.iters)
        bufs = dict(s_vec=out_buffer(self.m), obj=out_buffer(B * iters), avg=out_buffer(B * iters), iters_run=out_buffer(B, np.int32),
                    t_end=out_buffer(B, np.int32))
        r = BatchResult()
        r.s_vec, r.obj_trace, r.avg_change_trace = ptr(bufs["s_vec"], F64P), ptr(bufs["obj"], F64P), ptr(bufs["avg"], F64P)
        r.iters_run, r.t_end = ptr(bufs["iters_run"], I32P), ptr(bufs["t_end"], I32P)
        if want_w:
            bufs["w"] = out_buffer(self.m_cycle)
            r.w = ptr(bufs["w"], F64P)
        if adam is not None:
            for a in adam:
                if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.flags.writeable
                        and (a.size == self.m_cycle or self.m_cycle == 0)):
                    raise ValueError(f"Adam state must be two writable contiguous float64 arrays of {self.m_cycle} entries (all problems' cycles)")
            r.adam_m, r.adam_v = ptr(adam[0], F64P), ptr(adam[1], F64P)
        check(load().desc_pgd_batch_run(self.handle, C.byref(params), C.byref(r)))
        outs = []
        for b in range(B):
            e0, e1, c0, c1 = self.edge_off[b], self.edge_off[b + 1], self.cycle_off[b], self.cycle_off[b + 1]
            it = int(bufs["iters_run"][b])
            o = dict(S_vec=bufs["s_vec"][e0:e1], obj=bufs["obj"][b * iters:b * iters + it], avg=bufs["avg"][b * iters:b * iters + it],
                     iters_run=it, t_end=int(bufs["t_end"][b]), n_sample=int(self.n_sample[b]))
            if want_w:
                o["w"] = bufs["w"][c0:c1]
            if adam is not None:
                o["adam_m"], o["adam_v"] = adam[0][c0:c1], adam[1][c0:c1]
            outs.append(o)
        return outs, _timings(r)


def pgd_batch_max_codeg():
    """desc_pgd_batch_max_codeg: the largest codegree the batched device structure builder stages."""
    return int(load().desc_pgd_batch_max_codeg())


def batch_plan(hist, n_sample_min=30):
    """desc_test_batch_plan: the device builder's plan rule on a histogram of codegrees (hist[c], c = 0 .. n), on the host."""
    hist = np.ascontiguousarray(hist, dtype=np.int32)
    out = np.zeros(5, dtype=np.int64)
    check(load().desc_test_batch_plan(ptr(hist, I32P), hist.shape[0] - 1, int(n_sample_min), ptr(out, I64P)))
    return dict(zip(("m_pos", "max_codeg", "n_sample", "m_cycle", "max_cnt"), (int(x) for x in out)))


def gcw_batch_max_n():
    """desc_gcw_batch_max_n: the largest problem (nodes) the batched eigen-solve takes."""
    return int(load().desc_gcw_batch_max_n())


def gcw_batch_streamed_max_n():
    """desc_gcw_batch_streamed_max_n: the largest problem (nodes) the batched eigen-solve takes with its blocks streamed through LDS."""
    return int(load().desc_gcw_batch_streamed_max_n())


GCW_EIG = {"lds": 0, "streamed": 1, "auto": 2}       # DESC_GCW_EIG_*
GCW_EIG_RAN = ("lds", "streamed")                    # desc_spectral_info.reserved of a batched run


def gcw_eig_mode(eig):
    """The DESC_GCW_EIG_* value of ``eig``; ValueError naming the three values for anything else."""
    if not isinstance(eig, str) or eig not in GCW_EIG:
        raise ValueError(f'eig must be "lds", "streamed" or "auto", not {eig!r}')
    return GCW_EIG[eig]


class GcwBatch(_BatchHandle):
    """Owner of a desc_gcw_batch*: the Spectral / GCW eigen-solve of B small problems in one launch (desc_gcw_batch_*).
    ``probs`` is a sequence of ProblemArrays.  ``eig``: ``"lds"`` (the four blocks in LDS, up to gcw_batch_max_n() nodes),
    ``"streamed"`` (the blocks in global memory, one staging block in LDS, up to gcw_batch_streamed_max_n() nodes) or ``"auto"``
    (each problem by its own n: at most two launches).  The handle may be run any number of times."""

    _kind = "gcw"
    _create = "create_where"

    def __init__(self, probs, device=0, eig="lds", on=None):
        if on is not None:                           # a resident ProblemBatch: probs and device are not read
            self._open_on(on, gcw_eig_mode(eig))
        else:
            self._open(probs, int(device), gcw_eig_mode(eig))

    def run(self, s_vec=None, weights=None, normalize_rows=False, tol=1e-13, max_iters=500):
        """One batched eigen-solve.  s_vec: the concatenated S_vec (GCW mode); weights: concatenated host weights; neither: Spectral.
        Returns a list of per-problem (R (3,3,n_b) Fortran-ordered, info dict) and the call's timings."""
        B = self.count
        vec = None
        for name, v in (("s_vec", s_vec), ("weights", weights)):
            if v is None:
                continue
            vec = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
            if vec.size != self.m:
                raise ValueError(f"{name} must hold {self.m} entries (all problems' edges behind one another), not {vec.size}")
        R = out_buffer(9 * self.n)
        infos = (SpectralInfo * max(B, 1))()
        tm = GcwBatchTimings()
        check(load().desc_gcw_batch_run(self.handle, ptr(vec, F64P) if s_vec is not None else None,
                                        ptr(vec, F64P) if s_vec is None and weights is not None else None, 1 if normalize_rows else 0,
                                        tol, max_iters, ptr(R, F64P), infos, C.byref(tm)))
        outs = [(Rb, dict(iters=i.iters, products=i.products, converged=bool(i.converged), residual=i.residual,
                          eigenvalues=list(i.eigenvalues), ms_total=i.ms_total, eig=GCW_EIG_RAN[i.reserved]))
                for Rb, i in zip(_split_R(R, self.node_off), infos)]
        return outs, _timings(tm)


def cemp_batch_max_degree():
    """desc_cemp_batch_max_degree: the longest CSR row (neighbours of one node) the batched CEMP sampler stages."""
    return int(load().desc_cemp_batch_max_degree())


class CempBatch(_BatchHandle):
    """Owner of a desc_cemp_batch*: CEMP on B small problems in one GPU pass (desc_cemp_batch_*).  ``probs`` is a sequence of
    ProblemArrays; ``seeds`` an optional sequence of per-problem sampling seeds.  Sampling, S0 and the initial means are computed here;
    the handle may be run any number of times.  ``on``: a resident ProblemBatch to create the handle on (desc_cemp_batch_create_on)."""

    _kind = "cemp"

    def __init__(self, probs, nsample, seed=0, seeds=None, device=0, on=None):
        self.nsample = int(nsample)
        if on is not None:                           # a resident ProblemBatch: probs and device are not read
            self._open_on(on, self.nsample, int(seed), _seeds_array(seeds, len(on)))
        else:
            probs = list(probs)
            self._open(probs, self.nsample, int(seed), _seeds_array(seeds, len(probs)), int(device))

    def samples(self):
        """What create sampled, per problem: a list of dicts e_jk / e_ki (m_b x nsample local edge ids, -1 without a cycle), s0
        (m_b x nsample), has_cycle (m_b bools)."""
        mc = self.m * self.nsample
        ejk, eki, s0, hc = out_buffer(mc, np.int32), out_buffer(mc, np.int32), out_buffer(mc), out_buffer(self.m, np.uint8)
        check(load().desc_cemp_batch_get_samples(self.handle, ptr(ejk, I32P), ptr(eki, I32P), ptr(s0, F64P), ptr(hc, C.POINTER(C.c_uint8))))
        outs = []
        for b in range(self.count):
            e0, e1 = int(self.edge_off[b]), int(self.edge_off[b + 1])
            sl = slice(e0 * self.nsample, e1 * self.nsample)
            outs.append(dict(e_jk=ejk[sl].reshape(e1 - e0, self.nsample), e_ki=eki[sl].reshape(e1 - e0, self.nsample),
                             s0=s0[sl].reshape(e1 - e0, self.nsample), has_cycle=hc[e0:e1].astype(bool)))
        return outs

    def run(self, beta, max_iter):
        """The rounds (CEMP.m:107-128) from the initial means.  Returns a list of per-problem S_vec (library's edge order; views of one
        buffer) and the call's timings."""
        b = np.ascontiguousarray(beta, dtype=np.float64).reshape(-1)
        S = out_buffer(self.m)
        tm = CempBatchTimings()
        check(load().desc_cemp_batch_run(self.handle, ptr(b, F64P), b.shape[0], int(max_iter), ptr(S, F64P), C.byref(tm)))
        outs = [S[int(self.edge_off[k]):int(self.edge_off[k + 1])] for k in range(self.count)]
        return outs, _timings(tm)

    def mpls_run(self, s_vec, R_init, stop_threshold, max_iter, beta, tau, alpha):
        """The MPLS loop (MPLS.m:196-254) of every problem in one launch, on the handle's samples (desc_mpls_batch_run).  s_vec: the
        concatenated SVec (library's edge order, what ``run`` returned); R_init: the concatenated 9 n_b doubles per problem (3 x 3 x n_b
        column-major); beta / tau / alpha: MPLS_parameters.reweighting / .thresholding / .cycle_info_ratio.  Returns a list of per-problem
        (R_est (3,3,n_b) Fortran-ordered, info dict with mpls_run's keys) and the call's timings."""
        B = self.count
        S = np.ascontiguousarray(s_vec, dtype=np.float64).reshape(-1)
        Ri = np.ascontiguousarray(R_init, dtype=np.float64).reshape(-1)
        if S.size != self.m:
            raise ValueError(f"s_vec must hold {self.m} entries (all problems' edges behind one another), not {S.size}")
        if Ri.size != 9 * self.n:
            raise ValueError(f"R_init must hold {9 * self.n} entries (all problems' 3 x 3 x n blocks behind one another), not {Ri.size}")
        vec = [np.ascontiguousarray(np.atleast_1d(np.asarray(v, dtype=np.float64)).reshape(-1)) for v in (beta, tau, alpha)]
        R = out_buffer(9 * self.n)
        infos = (MplsInfo * max(B, 1))()
        tm = MplsBatchTimings()
        check(load().desc_mpls_batch_run(self.handle, ptr(S, F64P), ptr(Ri, F64P), float(stop_threshold), int(max_iter),
                                         ptr(vec[0], F64P), vec[0].size, ptr(vec[1], F64P), vec[1].size, ptr(vec[2], F64P), vec[2].size,
                                         ptr(R, F64P), infos, C.byref(tm)))
        outs = [(Rb, dict(iters=i.iters, cg_iters=i.cg_iters, cg_unconverged=i.cg_unconverged, m_pos=i.m_pos, score=i.score,
                          cg_residual=i.cg_residual, ms_loop=i.ms_loop, ms_total=i.ms_total))
                for Rb, i in zip(_split_R(R, self.node_off), infos)]
        return outs, _timings(tm)


def mst_batch_max_n():
    """desc_mst_batch_max_n: the largest problem (nodes) the batched tree kernel takes."""
    return int(load().desc_mst_batch_max_n())


def mst_batch_check(probs):
    """desc_mst_batch_check on a sequence of ProblemArrays: the size cap and connectivity of every problem (host only; raises DescError).
    The rotations are not read: index-only problems (a ProblemBatch's mirror) are taken."""
    probs = list(probs)
    check(load().desc_mst_batch_check(_problem_array(probs), len(probs)))


def mst_batch_run(probs, s_vec, device=0):
    """desc_mst_batch_run on a sequence of ProblemArrays and the concatenated S_vec (library's edge order) -> a list of per-problem
    (R (3,3,n_b) Fortran-ordered, tree edge ids ascending (n_b - 1,), sorted order) and the call's timings."""
    probs = list(probs)
    B = len(probs)
    arr = _problem_array(probs)
    S = np.ascontiguousarray(s_vec, dtype=np.float64).reshape(-1)
    no = np.concatenate([[0], np.cumsum([q.n for q in probs], dtype=np.int64)]).astype(np.int64)
    if S.size != sum(q.m for q in probs):
        raise ValueError("s_vec must hold one entry per edge of the batch")
    R = out_buffer(9 * int(no[B]))
    T = out_buffer(max(int(no[B]) - B, 1), np.int32)
    tm = MstBatchTimings()
    check(load().desc_mst_batch_run(arr, B, ptr(S, F64P), int(device), ptr(R, F64P), ptr(T, I32P), C.byref(tm)))
    outs = [(Rb, T[int(no[b]) - b:int(no[b + 1]) - b - 1].copy()) for b, Rb in enumerate(_split_R(R, no))]
    return outs, _timings(tm)


def mst_batch_run_on(pset, s_vec, return_bytes=False):
    """desc_mst_batch_run_on: mst_batch_run on a resident ProblemBatch, on its device.  ``return_bytes``: also the call's (h2d, d2h)."""
    if not pset.handle:
        raise ValueError("the ProblemBatch is closed")
    B, no = len(pset), pset.node_off
    S = np.ascontiguousarray(s_vec, dtype=np.float64).reshape(-1)
    if S.size != pset.m:
        raise ValueError("s_vec must hold one entry per edge of the batch")
    R = out_buffer(9 * int(no[B]))
    T = out_buffer(max(int(no[B]) - B, 1), np.int32)
    tm = MstBatchTimings()
    moved = np.zeros(2, dtype=np.int64)
    check(load().desc_mst_batch_run_on(pset.handle, ptr(S, F64P), ptr(R, F64P), ptr(T, I32P), C.byref(tm), ptr(moved, I64P)))
    outs = [(Rb, T[int(no[b]) - b:int(no[b + 1]) - b - 1].copy()) for b, Rb in enumerate(_split_R(R, no))]
    if return_bytes:
        return outs, _timings(tm), (int(moved[0]), int(moved[1]))
    return outs, _timings(tm)


def refine_batch_max_n():
    """desc_refine_batch_max_n: the largest problem (nodes) the batched refinement takes."""
    return int(load().desc_refine_batch_max_n())


def mpls_batch_max_n():
    """desc_mpls_batch_max_n: the largest problem (nodes) the batched MPLS loop takes (the batched refinement's cap)."""
    return int(load().desc_mpls_batch_max_n())


class RefineBatch(_BatchHandle):
    """Owner of a desc_refine_batch*: the DESC refinement tail of B small problems in one launch (desc_refine_batch_*).
    ``probs`` is a sequence of ProblemArrays.  The handle may be run any number of times."""

    _kind = "refine"

    def __init__(self, probs, device=0, on=None):
        if on is not None:                           # a resident ProblemBatch: probs and device are not read
            self._open_on(on)
        else:
            self._open(probs, int(device))

    def run(self, s_vec, R_init, stop_threshold=1e-3, max_iters=100):
        """One batched refinement.  s_vec: the concatenated S_vec (library's edge order); R_init: the concatenated 9 n_b doubles per
        problem (3 x 3 x n_b column-major).  Returns a list of per-problem (R (3,3,n_b) Fortran-ordered, info dict with refine_run's
        keys) and the call's timings."""
        B = self.count
        S = np.ascontiguousarray(s_vec, dtype=np.float64).reshape(-1)
        Ri = np.ascontiguousarray(R_init, dtype=np.float64).reshape(-1)
        if S.size != self.m:
            raise ValueError(f"s_vec must hold {self.m} entries (all problems' edges behind one another), not {S.size}")
        if Ri.size != 9 * self.n:
            raise ValueError(f"R_init must hold {9 * self.n} entries (all problems' 3 x 3 x n blocks behind one another), not {Ri.size}")
        R = out_buffer(9 * self.n)
        infos = (RefineInfo * max(B, 1))()
        tm = RefineBatchTimings()
        check(load().desc_refine_batch_run(self.handle, ptr(S, F64P), ptr(Ri, F64P), stop_threshold, int(max_iters), ptr(R, F64P), infos,
                                           C.byref(tm)))
        outs = [(Rb, dict(iters=i.iters, cg_iters=i.cg_iters, score=i.score, ms_total=i.ms_total, cg_unconverged=i.cg_unconverged,
                          cg_residual=i.cg_residual)) for Rb, i in zip(_split_R(R, self.node_off), infos)]
        return outs, _timings(tm)


def irls_batch_max_n():
    """desc_irls_batch_max_n: the largest problem (nodes) the batched IRLS takes."""
    return int(load().desc_irls_batch_max_n())


def irls_tree_sequence(prob, order=None):
    """desc_irls_tree_sequence (host only): the spanning-tree start of BoxMedianSO3Graph.m:79-114 over the edges of ``prob`` in the
    caller's row order (``order``: marshal_edges' perm, or None) -> (edges, dirs, reached): per reached node, in the order the
    reference sets them, the sorted edge id and 0 (Q(j) from Q(i)) or 1 (Q(i) from Q(j)); ``reached`` == n iff the graph is connected."""
    od = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    if od is not None and od.size != prob.m:
        raise ValueError("order must have m entries")
    seq = out_buffer(max(prob.n - 1, 1), np.int32)
    reached = C.c_int64(0)
    check(load().desc_irls_tree_sequence(C.byref(prob.c), ptr(od, I32P), ptr(seq, I32P), C.byref(reached)))
    seq = seq[:max(int(reached.value) - 1, 0)]
    return seq >> 1, seq & 1, int(reached.value)


class IrlsBatch(_BatchHandle):
    """Owner of a desc_irls_batch*: IRLS_GM / IRLS_L12 of B small connected problems in two launches (desc_irls_batch_*).  ``probs`` is a
    sequence of ProblemArrays, ``orders`` an optional sequence of per-problem row orders (marshal_edges' perm, or None).  The handle may
    be run any number of times, in either mode.  ``on``: a resident ProblemBatch to create the handle on (desc_irls_batch_create_on)."""

    _kind = "irls"

    def __init__(self, probs, orders=None, device=0, on=None):
        probs = on.probs if on is not None else list(probs)          # a resident ProblemBatch: its index mirror gives the sizes
        B = len(probs)
        arr = None
        if orders is not None:
            if len(orders) != B:
                raise ValueError(f"orders must hold one entry per problem ({B}), not {len(orders)}")
            self._orders = [None if o is None else np.ascontiguousarray(o, dtype=np.int32) for o in orders]     # kept alive over create
            for q, o in zip(probs, self._orders):
                if o is not None and o.size != q.m:
                    raise ValueError("an order must have one entry per edge of its problem")
            arr = (I32P * max(B, 1))(*[ptr(o, I32P) for o in self._orders])
        if on is not None:
            self._open_on(on, arr)
        else:
            self._open(probs, arr, int(device))

    def run(self, mode, sigma_deg=5.0, max_iter_l1=10, max_iter_irls=100):
        """One batched run -> a list of per-problem (R, R_l1 (3,3,n_b) Fortran-ordered, info dict with irls_run's keys) and the call's
        timings."""
        B = self.count
        R, R1 = out_buffer(9 * self.n), out_buffer(9 * self.n)
        infos = (IrlsInfo * max(B, 1))()
        tm = IrlsBatchTimings()
        check(load().desc_irls_batch_run(self.handle, int(mode), float(sigma_deg), int(max_iter_l1), int(max_iter_irls), ptr(R, F64P),
                                         ptr(R1, F64P), infos, C.byref(tm)))
        outs = [(Rb, R1b, {k: getattr(i, k) for k, _ in IrlsInfo._fields_})
                for Rb, R1b, i in zip(_split_R(R, self.node_off), _split_R(R1, self.node_off), infos)]
        return outs, _timings(tm)


def _nsample_array(nsample, B):
    """``nsample`` of a batched LP call -- None (the rule for every problem), one int or a sequence of B ints -- as an int32 array, or
    None."""
    if nsample is None:
        return None
    if np.ndim(nsample) == 0:
        nsample = [nsample] * B
    if len(nsample) != B:
        raise ValueError(f"nsample must hold one entry per problem ({B}), not {len(nsample)}")
    return np.ascontiguousarray([0 if v is None else int(v) for v in nsample], dtype=np.int32).reshape(-1)


def lp_batch_plan(probs, nsample=None):
    """desc_lp_batch_plan on a sequence of ProblemArrays: what desc_lp_batch_create decides on the host (no device; raises DescError with
    create's refusals) -> dict of nsample, m_pos, ncol, nrow (B entries) and var_off, row_off (B + 1)."""
    probs = list(probs)
    B = len(probs)
    ns = _nsample_array(nsample, B)
    i32 = lambda k: np.zeros(max(k, 1), dtype=np.int32)
    i64 = lambda k: np.zeros(max(k, 1), dtype=np.int64)
    out = dict(nsample=i32(B), m_pos=i64(B), var_off=i64(B + 1), row_off=i64(B + 1), ncol=i32(B), nrow=i32(B))
    check(load().desc_lp_batch_plan(_problem_array(probs), B, ptr(ns, I32P), ptr(out["nsample"], I32P), ptr(out["m_pos"], I64P),
                                    ptr(out["var_off"], I64P), ptr(out["row_off"], I64P), ptr(out["ncol"], I32P), ptr(out["nrow"], I32P)))
    return {k: v[:B + 1 if k.endswith("_off") else B] for k, v in out.items()}


class LpBatch(_BatchHandle):
    """Owner of a desc_lp_batch*: the LP of linprog_sij for B small problems at once (desc_lp_batch_*).  ``probs`` is a sequence of
    ProblemArrays; ``nsample`` None (the rule of linprog_sij.m:43, per problem), one int or a sequence of B ints; ``seeds`` an optional
    sequence of per-problem sampling seeds.  Samples, S0Mat and the transposed incidence are built here; the handle may be run any
    number of times with other parameters."""

    _kind = "lp"

    def __init__(self, probs, nsample=None, seeds=None, device=0):
        probs = list(probs)
        self._open(probs, ptr(_nsample_array(nsample, len(probs)), I32P), _seeds_array(seeds, len(probs)), int(device))

    def _read_sizes(self, B):
        no, eo, vo, ro = (np.zeros(B + 1, dtype=np.int64) for _ in range(4))
        ns, mp = np.zeros(max(B, 1), dtype=np.int32), np.zeros(max(B, 1), dtype=np.int64)
        check(self._export("sizes")(self.handle, None, ptr(no, I64P), ptr(eo, I64P), ptr(ns, I32P), ptr(mp, I64P), ptr(vo, I64P), ptr(ro, I64P)))
        self.node_off, self.edge_off, self.var_off, self.row_off, self.nsample, self.m_pos = no, eo, vo, ro, ns[:B], mp[:B]
        self.n, self.m = int(no[B]), int(eo[B])

    def sizes(self):
        """Per problem: nsample, m_pos, the offset of its variables and of its cycles in the batch's arrays."""
        return [dict(nsample=int(self.nsample[b]), m_pos=int(self.m_pos[b]), var_off=int(self.var_off[b]), row_off=int(self.row_off[b]))
                for b in range(self.count)]

    def samples(self):
        """What create sampled, per problem: a list of dicts pos_edges (m_pos 0-based sorted edge ids: the LP's variables) and k
        (m_pos x nsample sampled third nodes, 1-based), as lp_sij_run returns them."""
        MP, MC = int(self.var_off[self.count]), int(self.row_off[self.count])
        pos, k = out_buffer(MP, np.int32), out_buffer(MC, np.int32)
        check(load().desc_lp_batch_get_samples(self.handle, ptr(pos, I32P), ptr(k, I32P)))
        return [dict(pos_edges=pos[int(self.var_off[b]):int(self.var_off[b + 1])].copy(),
                     k=k[int(self.row_off[b]):int(self.row_off[b + 1])].reshape(int(self.m_pos[b]), int(self.nsample[b])))
                for b in range(self.count)]

    def run(self, params=None, want_y=False):
        """One batched run of the loop.  params: LpParams (tol, max_iter, check_every and restart are read; None: the defaults).
        Returns a list of per-problem (S_vec (m_b,) in sorted edge order, y (m_pos, nsample, 2) or None, info dict with lp_sij_run's
        keys) and the call's timings."""
        B = self.count
        MC = int(self.row_off[B])
        p = params if params is not None else default_lp_params()
        S = out_buffer(self.m)
        y = out_buffer(2 * MC) if want_y else None
        infos = (LpInfo * max(B, 1))()
        tm = LpBatchTimings()
        check(load().desc_lp_batch_run(self.handle, C.byref(p), ptr(S, F64P), ptr(y, F64P), infos, C.byref(tm)))
        outs = []
        for b in range(B):
            yb = None
            if want_y:
                yb = y[2 * int(self.row_off[b]):2 * int(self.row_off[b + 1])].reshape(int(self.m_pos[b]), int(self.nsample[b]), 2)
            outs.append((S[int(self.edge_off[b]):int(self.edge_off[b + 1])], yb, {name: getattr(infos[b], name) for name, _ in LpInfo._fields_}))
        return outs, _timings(tm)


MODELS_KIND_UNIFORM, MODELS_KIND_NONUNIFORM = 0, 1
MODELS_UNIFORM, MODELS_SELF_CONSISTENT, MODELS_ADV = 0, 1, 2
# DESC_MODELS_STREAM_*
MODELS_STREAMS = dict(edge=1, rorig=2, rcorr=3, corrupt=4, noise=5, haar=6, node=7, select=8, r0=9)


def models_batch_max_n():
    """desc_models_batch_max_n: the largest n the batched generator draws."""
    return int(load().desc_models_batch_max_n())


def models_key(seed, stream, sub, id, c):
    """desc_models_key: the generator's 64-bit key of (seed, stream, sub, id, component)."""
    return int(load().desc_models_key(int(seed), int(stream), int(sub), int(id), int(c)))


class ModelsBatch(_BatchHandle):
    """Owner of a desc_models_batch*: B synthetic problems drawn on the GPU (desc_models_batch_*).  ``specs`` is a sequence of
    ModelSpec.  Create runs the graph pass: ``m_per`` holds the problems' edge counts, ``node_off`` / ``edge_off`` their offsets in the
    concatenated arrays ``fetch`` returns."""

    _kind = "models"

    def __init__(self, specs, device=0):
        self.device = int(device)
        self.specs = list(specs)
        self.count = B = len(self.specs)
        arr = (ModelSpec * max(B, 1))(*self.specs)
        h = C.c_void_p()
        check(load().desc_models_batch_create(arr, B, int(device), C.byref(h)))
        self.handle = h
        m_per = np.zeros(max(B, 1), dtype=np.int64)
        check(load().desc_models_batch_sizes(self.handle, ptr(m_per, I64P)))
        self.m_per = m_per[:B]
        self.node_off = np.concatenate([[0], np.cumsum([s.n for s in self.specs], dtype=np.int64)]).astype(np.int64)
        self.edge_off = np.concatenate([[0], np.cumsum(self.m_per, dtype=np.int64)]).astype(np.int64)
        self.n, self.m = int(self.node_off[B]), int(self.edge_off[B])

    FIELDS = ("ind_i", "ind_j", "rij", "rij_orig", "r_orig", "err_vec", "corrupted")

    def fetch(self, only=None):
        """The node, selection and edge passes and the copy-back: a dict of the concatenated arrays ind_i / ind_j (int32, 0-based), rij /
        rij_orig (9 m), r_orig (9 n), err_vec (m), corrupted (m, uint8) -- and the call's timings.  ``only``: the names to copy back
        (default: all of them)."""
        N, M = self.n, self.m
        sizes = dict(ind_i=M, ind_j=M, rij=9 * M, rij_orig=9 * M, r_orig=9 * N, err_vec=M, corrupted=M)
        types = dict(ind_i=(np.int32, I32P), ind_j=(np.int32, I32P), corrupted=(np.uint8, C.POINTER(C.c_uint8)))
        names = self.FIELDS if only is None else [k for k in self.FIELDS if k in only]
        out = {k: out_buffer(sizes[k], types.get(k, (np.float64,))[0]) for k in names}
        tm = ModelsBatchTimings()
        check(load().desc_models_batch_fetch(self.handle, *[ptr(out.get(k), types.get(k, (None, F64P))[1]) for k in self.FIELDS], C.byref(tm)))
        return {k: v[:sizes[k]] for k, v in out.items()}, _timings(tm)


def hook_models_draws(seed, stream, sub, id0, count, c, normal=False, device=0):
    """desc_test_models_uniform / _normal: the device's draws of component c for ids id0 .. id0 + count - 1."""
    out = out_buffer(count)
    fn = load().desc_test_models_normal if normal else load().desc_test_models_uniform
    check(fn(int(seed), int(stream), int(sub), int(id0), int(count), int(c), int(device), ptr(out, F64P)))
    return out[:int(count)]


class AlignBatch(_BatchHandle):
    """Owner of a desc_align_batch*: the ground-truth rotations of B problems resident on the GPU (desc_align_batch_*).  ``n`` holds the
    problems' node counts, ``R_gt`` their 3x3xn_b column-major blocks behind one another (9 * sum(n) doubles).  ``run`` scores one set of
    estimates against them and may be called any number of times."""

    _kind = "align"

    def __init__(self, n, R_gt, device=0):
        self.n_per = np.ascontiguousarray(n, dtype=np.int32).reshape(-1)
        self.count = B = int(self.n_per.shape[0])
        self.R_gt = np.ascontiguousarray(R_gt, dtype=np.float64).reshape(-1)
        if self.R_gt.shape[0] != 9 * int(np.maximum(self.n_per, 0).sum(dtype=np.int64)):
            raise ValueError("R_gt must hold 9 * sum(n) doubles")
        n_arr = self.n_per if B else np.zeros(1, dtype=np.int32)
        gt = self.R_gt if self.R_gt.shape[0] else np.zeros(1)
        h = C.c_void_p()
        check(load().desc_align_batch_create(ptr(n_arr, I32P), ptr(gt, F64P), B, int(device), C.byref(h)))
        self.handle = h
        no, cnt = np.zeros(B + 1, dtype=np.int64), C.c_int32()
        check(load().desc_align_batch_sizes(self.handle, C.byref(cnt), ptr(no, I64P)))
        self.node_off, self.n = no, int(no[B])

    def run(self, R_est, rotations=True):
        """One batched alignment of R_est (9 * n doubles, the problems behind one another).  Returns a dict of the concatenated arrays
        R_out (9 n; None without ``rotations``), R_align (9 B), err (n, degrees), mean_error and median_error (B) -- and the call's timings."""
        B, N = self.count, self.n
        est = np.ascontiguousarray(R_est, dtype=np.float64).reshape(-1)
        if est.shape[0] != 9 * N:
            raise ValueError(f"R_est must hold 9 * {N} doubles, not {est.shape[0]}")
        out = dict(R_out=out_buffer(9 * N) if rotations else None, R_align=out_buffer(9 * B), err=out_buffer(N), mean_error=out_buffer(B),
                   median_error=out_buffer(B))
        tm = AlignBatchTimings()
        check(load().desc_align_batch_run(self.handle, ptr(est if N else np.zeros(1), F64P), ptr(out["R_out"], F64P), ptr(out["R_align"], F64P),
                                          ptr(out["err"], F64P), ptr(out["mean_error"], F64P), ptr(out["median_error"], F64P), C.byref(tm)))
        sizes = dict(R_out=9 * N, R_align=9 * B, err=N, mean_error=B, median_error=B)
        return {k: (None if v is None else v[:sizes[k]]) for k, v in out.items()}, _timings(tm)


def hook_align_project(A, device=0):
    """desc_test_align_project: the projection behind R_align of count column-major blocks (count x 9) -> count x 9."""
    A = np.ascontiguousarray(A, dtype=np.float64).reshape(-1, 9)
    out = out_buffer(A.size)
    check(load().desc_test_align_project(ptr(A if A.size else np.zeros(9), F64P), A.shape[0], int(device), ptr(out, F64P)))
    return out[:A.size].reshape(-1, 9)


CSR_WHERE = {"host": BUILD_HOST, "device": BUILD_DEVICE}


class ProblemBatch(_BatchHandle):
    """Owner of a desc_problem_batch*: the problems of B instances validated, laid out and uploaded once (desc_problem_batch_*), for
    every batched handle created ``on=`` it.  ``probs`` is a sequence of ProblemArrays (kept: the host mirror); ``csr``: ``"host"`` or
    ``"device"``, the builder of the per-problem CSR.  ``ProblemBatch.from_models(models_handle)`` takes a generator's problems on the
    device; its mirror holds the endpoints, and the rotations once ``host_problems()`` has fetched them.  ``close()`` drops this
    reference: handles created on the set keep its device arrays alive."""

    _kind = "problem"

    def __init__(self, probs, device=0, csr="host"):
        if not isinstance(csr, str) or csr not in CSR_WHERE:
            raise ValueError(f"csr must be 'host' or 'device', not {csr!r}")
        self.device = int(device)
        self._has_rij = True
        self._open(probs, self.device, CSR_WHERE[csr])
        self.built_where = int(self._export("built_where")(self.handle))

    @classmethod
    def from_models(cls, models: "ModelsBatch"):
        self = cls.__new__(cls)
        h = C.c_void_p()
        check(load().desc_problem_batch_from_models(models.handle, C.byref(h)))
        self.handle, self.device, self.count = h, int(models.device), models.count
        self._read_sizes(self.count)
        ii, jj = out_buffer(self.m, np.int32), out_buffer(self.m, np.int32)
        check(load().desc_problem_batch_fetch(self.handle, ptr(ii, I32P), ptr(jj, I32P), None, None, None, None))     # the host mirror: no copy
        self.probs = [ProblemArrays(int(self.node_off[b + 1] - self.node_off[b]), ii[self.edge_off[b]:self.edge_off[b + 1]],
                                    jj[self.edge_off[b]:self.edge_off[b + 1]]) for b in range(self.count)]
        self._has_rij = self.count == 0
        self.built_where = int(self._export("built_where")(self.handle))
        return self

    def __len__(self):
        return self.count

    def fetch(self, rij=False, csr=False):
        """The set's arrays through desc_problem_batch_fetch: dict(ind_i, ind_j[, rij][, rowptr, adj, adj_eid]), batch-long."""
        if not self.handle:
            raise ValueError("the ProblemBatch is closed")
        sizes = dict(ind_i=self.m, ind_j=self.m)
        if rij:
            sizes["rij"] = 9 * self.m
        if csr:
            sizes.update(rowptr=self.n + self.count, adj=2 * self.m, adj_eid=2 * self.m)
        out = {k: out_buffer(n, np.float64 if k == "rij" else np.int32) for k, n in sizes.items()}
        check(load().desc_problem_batch_fetch(self.handle, *[ptr(out.get(k), F64P if k == "rij" else I32P)
                                                             for k in ("ind_i", "ind_j", "rij", "rowptr", "adj", "adj_eid")]))
        return {k: v[:sizes[k]] for k, v in out.items()}

    def host_problems(self):
        """The host mirror with rotations (a list of ProblemArrays); a generated set fetches them once, here."""
        if not self._has_rij:
            rij = self.fetch(rij=True)["rij"]
            self.probs = [ProblemArrays(q.n, q.ind_i, q.ind_j, rij[9 * int(self.edge_off[b]):9 * int(self.edge_off[b + 1])])
                          for b, q in enumerate(self.probs)]
            self._has_rij = True
        return self.probs

    close = _BatchHandle.destroy

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def gcw_batch_csr(probs):
    """desc_gcw_batch_csr on a sequence of ProblemArrays: the per-problem CSR the batched eigen-solve uploads (host only)."""
    probs = list(probs)
    B = len(probs)
    arr = _problem_array(probs)
    no, eo = np.zeros(B + 1, dtype=np.int64), np.zeros(B + 1, dtype=np.int64)
    L = load()
    check(L.desc_gcw_batch_csr(arr, B, ptr(no, I64P), ptr(eo, I64P), None, None, None))
    N, M = int(no[B]), int(eo[B])
    rowptr, adj, eid = out_buffer(N + B, np.int32), out_buffer(2 * M, np.int32), out_buffer(2 * M, np.int32)
    check(L.desc_gcw_batch_csr(arr, B, ptr(no, I64P), ptr(eo, I64P), ptr(rowptr, I32P), ptr(adj, I32P), ptr(eid, I32P)))
    return dict(node_off=no, edge_off=eo, rowptr=rowptr[:N + B], adj=adj[:2 * M], adj_eid=eid[:2 * M])


def batch_concat(structures):
    """desc_pgd_batch_concat on a list of Structure objects: the host part of the batch set-up (offsets and globalised index arrays)."""
    B = len(structures)
    hs = (C.c_void_p * max(B, 1))(*[s.handle for s in structures])
    eo, co, so = (np.zeros(B + 1, dtype=np.int64) for _ in range(3))
    L = load()
    check(L.desc_pgd_batch_concat(hs, B, ptr(eo, I64P), ptr(co, I64P), ptr(so, I64P), None, None, None, None, None, None))
    mp, mc = int(so[B]), int(co[B])
    pos, cum = out_buffer(mp, np.int32), out_buffer(mp + 1, np.int32)
    ejk, eki, ikj, jki = (out_buffer(mc, np.int32) for _ in range(4))
    check(L.desc_pgd_batch_concat(hs, B, ptr(eo, I64P), ptr(co, I64P), ptr(so, I64P), ptr(pos, I32P), ptr(cum, I32P), ptr(ejk, I32P),
                                  ptr(eki, I32P), ptr(ikj, I32P), ptr(jki, I32P)))
    return dict(edge_off=eo, cycle_off=co, seg_off=so, pos_edge=pos[:mp], cum=cum[:mp + 1], e_jk=ejk[:mc], e_ki=eki[:mc], ikj=ikj[:mc],
                jki=jki[:mc])


def validate_step(step, m_cycle, like=None):
    """What a GetStep callback returned (DESC_PGD.m:207), checked before it reaches the library: a float64 vector of m_cycle entries --
    a NumPy array, or, when the gradient was handed out as the torch tensor `like`, a tensor on the same device.  Returns it contiguous
    and flat.  ValueError otherwise; whether the values are finite is the caller's business, as in the reference."""
    if like is not None:
        import torch
        if not isinstance(step, torch.Tensor):
            raise ValueError(f"GetStep was given a torch tensor and must return one, not {type(step).__name__}")
        if step.dtype != like.dtype:
            raise ValueError(f"GetStep must return a {like.dtype} tensor, not {step.dtype}")
        if step.device != like.device:
            raise ValueError(f"GetStep must return a tensor on {like.device}, not on {step.device}")
        if step.numel() != m_cycle:
            raise ValueError(f"GetStep must return m_cycle = {m_cycle} entries, not {step.numel()}")
        return step.detach().reshape(-1).contiguous()
    if not isinstance(step, np.ndarray):
        raise ValueError(f"GetStep must return a NumPy array of m_cycle = {m_cycle} float64 entries, not {type(step).__name__}")
    if step.dtype != np.float64:
        raise ValueError(f"GetStep must return a float64 array, not {step.dtype}")
    if step.size != m_cycle:
        raise ValueError(f"GetStep must return m_cycle = {m_cycle} entries, not {step.size}")
    return np.ascontiguousarray(step).reshape(-1)


def torch_for_device_mode():
    """torch for a plugin with ``device_tensors = True``.  PyTorch bundles its own ROCm runtime and a process can hold only one: torch
    has to be imported before this library is loaded (see load()).  DescError when that is no longer possible, when torch is not
    installed, or when it sees no GPU."""
    import sys
    if "torch" not in sys.modules and _lib is not None:
        raise DescError("a plugin with device_tensors = True needs torch, and torch must be imported before libdesc_amd.so is loaded: "
                        "import torch first (or set DESC_AMD_PRELOAD_TORCH=1)", ERR_STATE)
    try:
        import torch
    except ImportError as e:
        raise DescError(f"a plugin with device_tensors = True needs torch, which cannot be imported ({e}); "
                        "without it the plugin runs in the NumPy mode (device_tensors = False)", ERR_STATE) from None
    if not torch.cuda.is_available():
        raise DescError("a plugin with device_tensors = True needs a GPU that torch can see (torch.cuda.is_available() is False)", ERR_HIP)
    return torch


class Solver:
    """Owner of a desc_pgd* (problem + structure resident in HBM)."""

    def __init__(self, prob, structure: Structure, device=0, rank=0, world=1):
        h = C.c_void_p()
        if isinstance(prob, DeviceProblem):        # rotations and edge list already in HBM
            check(load().desc_pgd_create_dev(prob.handle, structure.handle, rank, world, C.byref(h)))
        else:
            check(load().desc_pgd_create_shard(C.byref(prob.c), structure.handle, device, rank, world, C.byref(h)))
        self.handle = h
        m, mp, mc, mx = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
        check(load().desc_pgd_sizes(h, C.byref(m), C.byref(mp), C.byref(mc), C.byref(mx)))
        self.m, self.m_pos, self.m_cycle, self.max_cnt = m.value, mp.value, mc.value, mx.value

    def kernel_name(self):
        return load().desc_pgd_kernel_name(self.handle).decode()

    def layout_stats(self):
        out = np.zeros(10, dtype=np.int64)
        k = load().desc_pgd_layout_stats(self.handle, ptr(out, I64P), 10)
        if k < 0:
            check(k)
        return dict(zip(("colsum_entries", "pieces", "bands", "piece_row_entries", "cycles", "segments",
                         "colsum_cl", "colsum_long", "colsum_nodes", "colsum_fx_bits"), (int(x) for x in out[:k])))

    def last_sweep(self):
        """Name + template arguments of the sweep kernel launched last (diagnostics)."""
        return load().desc_debug_last_sweep(self.handle).decode()

    def shard_layout(self):
        """The exchange layout (diagnostics): xpos, spos (2m each), xt and slot_ab ((owned segments, 2) each)."""
        info = self.shard_info()
        nsl = int(info.seg_hi - info.seg_lo)
        xpos, spos = out_buffer(2 * self.m, np.int32), out_buffer(2 * self.m, np.int32)
        xt, sab = out_buffer(2 * nsl, np.int32), out_buffer(2 * nsl, np.int32)
        check(load().desc_debug_shard_layout(self.handle, ptr(xpos, I32P), ptr(spos, I32P), ptr(xt, I32P), ptr(sab, I32P)))
        return dict(xpos=xpos[:2 * self.m], spos=spos[:2 * self.m], xt=xt[:2 * nsl].reshape(-1, 2), slot_ab=sab[:2 * nsl].reshape(-1, 2))

    def s0(self):
        out = out_buffer(self.m_cycle)
        check(load().desc_pgd_get_s0(self.handle, ptr(out, F64P)))
        return out[:self.m_cycle]

    def _result(self, iters, want_w=False, adam=None):
        bufs = dict(s_vec=out_buffer(self.m), obj=out_buffer(iters), avg=out_buffer(iters))
        r = Result()
        r.s_vec = ptr(bufs["s_vec"], F64P)
        r.obj_trace = ptr(bufs["obj"], F64P)
        r.avg_change_trace = ptr(bufs["avg"], F64P)
        if want_w:
            bufs["w"] = out_buffer(self.m_cycle)
            r.w = ptr(bufs["w"], F64P)
        if adam is not None:
            # the library reads AND writes m_cycle doubles through these pointers (HybridGradient.m_t / v_t)
            for a in adam:
                if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.flags.writeable
                        and (a.size == self.m_cycle or self.m_cycle == 0)):
                    raise ValueError(f"Adam state must be two writable contiguous float64 arrays of m_cycle = {self.m_cycle} entries")
            bufs["adam_m"], bufs["adam_v"] = adam
            r.adam_m = ptr(bufs["adam_m"], F64P)
            r.adam_v = ptr(bufs["adam_v"], F64P)
        return r, bufs

    def _pack(self, r, bufs):
        it = r.iters_run
        out = dict(S_vec=bufs["s_vec"][:self.m], obj=bufs["obj"][:it], avg=bufs["avg"][:it], iters_run=it,
                   t_end=r.t_end, ms_upload=r.ms_upload, ms_cycle_d=r.ms_cycle_d, ms_pgd=r.ms_pgd,
                   ms_total=r.ms_total, ms_structure=r.ms_structure)
        if "w" in bufs:
            out["w"] = bufs["w"][:self.m_cycle]
        if "adam_m" in bufs:
            out["adam_m"], out["adam_v"] = bufs["adam_m"], bufs["adam_v"]
        return out

    def run(self, params: Params, want_w=False, adam=None):
        r, bufs = self._result(params.iters, want_w, adam)
        check(load().desc_pgd_run(self.handle, C.byref(params), C.byref(r)))
        return self._pack(r, bufs)

    def run_traced(self, params: Params, dprob, err_vec, gcw_tol=1e-13, gcw_max_iters=500, adam=None):
        """desc_pgd_run_traced (params.make_plots = true, DESC_PGD.m:235-239): the run plus svec_errors and the GCW estimate
        of every iteration, R_est_all (iters_run, 3, 3, n)."""
        r, bufs = self._result(params.iters, adam=adam)
        n = dprob.n
        ev = np.ascontiguousarray(err_vec, dtype=np.float64).reshape(-1)
        if ev.size != self.m:
            raise ValueError("err_vec must have m entries")
        se = out_buffer(params.iters); Rall = out_buffer(max(params.iters, 1) * 9 * max(n, 1))
        check(load().desc_pgd_run_traced(self.handle, dprob.handle, C.byref(params), ptr(ev, F64P), gcw_tol, gcw_max_iters,
                                         ptr(se, F64P), ptr(Rall, F64P), C.byref(r)))
        out = self._pack(r, bufs)
        k = out["iters_run"]
        out["svec_errors"] = se[:k]
        out["R_est_all"] = Rall[:k * 9 * n].reshape(k, 9 * n).reshape((k, n, 3, 3)).transpose(0, 3, 2, 1)     # (t, r, c, node) from 3 x 3 x n column-major
        return out

    # ---- caller-supplied step rule (desc_pgd_ext_*): the iteration cut at DESC_PGD.m:207
    def ext_begin(self, params: Params):
        self._iters_cap = params.iters
        check(load().desc_pgd_ext_begin(self.handle, C.byref(params)))

    def ext_grad(self, out, where=MEM_HOST):
        """grad_long of the current iterate into `out`: a float64 NumPy array of m_cycle entries, or (where=MEM_DEVICE) a device address."""
        check(load().desc_pgd_ext_grad(self.handle, C.c_void_p(out.ctypes.data if isinstance(out, np.ndarray) else int(out)), where))

    def ext_apply(self, step, where=MEM_HOST):
        """Finish the iteration with `step` (as ext_grad's `out`) -> (average_change, objective, stopped)."""
        avg, obj, stop = C.c_double(), C.c_double(), C.c_int32()
        check(load().desc_pgd_ext_apply(self.handle, C.c_void_p(step.ctypes.data if isinstance(step, np.ndarray) else int(step)), where,
                                        C.byref(avg), C.byref(obj), C.byref(stop)))
        return avg.value, obj.value, bool(stop.value)

    def ext_laps(self):
        """Device milliseconds of the last gradient pass, apply pass, objective + stop rule."""
        out = np.zeros(3)
        check(load().desc_pgd_ext_laps(self.handle, ptr(out, F64P)))
        return tuple(float(x) for x in out)

    def run_external(self, params: Params, get_step, device_tensors=False, device=0, want_w=False, progress=None, after_step=None):
        """The PGD loop (DESC_PGD.m:182-257) around a step rule the library does not know: per iteration the gradient pass, then
        ``step = get_step(grad_long)`` (:207), then the apply pass with the objective and the stop rule.  ``get_step`` is called exactly
        iters_run times.  ``grad_long`` and the step are in the reference's cycle order (segment l at cum_ind[l] .. cum_ind[l+1]).

        Default mode: ``grad_long`` is a fresh float64 NumPy array and a NumPy array comes back -- 2 x 8 m_cycle bytes cross PCIe per
        iteration: slow, always available.  ``device_tensors``: ``grad_long`` is a float64 torch tensor on ``cuda:<device>`` that the
        gradient pass wrote in place (read-only for the callback; it is overwritten by the next iteration) and the returned tensor is
        read in place after torch's current stream has been synchronised: no per-cycle data leaves the device.

        progress(it, average_change, objective) and after_step(it) are called after every applied step."""
        p = Params.from_buffer_copy(params)
        p.step_kind = STEP_EXTERNAL
        p.progress = None; p.progress_user = None; p.verbose = 0
        mc = self.m_cycle
        torch = grad_t = None
        if device_tensors:
            torch = torch_for_device_mode()
            dev = torch.device("cuda", device)
            grad_t = torch.empty(max(mc, 1), dtype=torch.float64, device=dev)[:mc]
        else:
            grad_buf = out_buffer(mc)
        import time
        t0 = time.perf_counter()
        self.ext_begin(p)
        calls = 0
        for it in range(1, p.iters + 1):
            if device_tensors:
                self.ext_grad(grad_t.data_ptr(), MEM_DEVICE)
                step = get_step(grad_t)
                calls += 1
                step = validate_step(step, mc, like=grad_t)
                torch.cuda.current_stream(dev).synchronize()          # the step must be complete: the library orders only its own stream
                avg, obj, stopped = self.ext_apply(step.data_ptr(), MEM_DEVICE)
            else:
                self.ext_grad(grad_buf, MEM_HOST)
                step = get_step(grad_buf[:mc].copy())                 # value semantics, as MATLAB's: a plugin may keep what it is given
                calls += 1
                step = validate_step(step, mc)
                avg, obj, stopped = self.ext_apply(step, MEM_HOST)
            if progress is not None:
                progress(it, avg, obj)
            if after_step is not None:
                after_step(it)                                        # :235-239 come before the stop test of the same iteration
            if stopped:
                break
        out = self.download(want_w=want_w)
        out["ms_total"] = (time.perf_counter() - t0) * 1e3
        out["calls"] = calls
        return out

    def reset(self, params: Params):
        self._iters_cap = params.iters
        check(load().desc_pgd_reset(self.handle, C.byref(params)))

    def iterate(self, n):
        check(load().desc_pgd_iterate(self.handle, n))

    def iterate_timed(self, n, per_kernel=False):
        ms, mk = C.c_float(), C.c_float()
        check(load().desc_pgd_iterate_timed(self.handle, n, C.byref(ms), C.byref(mk) if per_kernel else None))
        return ms.value, (mk.value if per_kernel else None)

    def sync(self):
        check(load().desc_pgd_sync(self.handle))

    def download(self, want_w=False):
        r, bufs = self._result(getattr(self, "_iters_cap", 1), want_w)
        check(load().desc_pgd_download(self.handle, C.byref(r)))
        return self._pack(r, bufs)

    # ---- multi-GPU pieces (see desc_amd/sharded.py)
    def shard_info(self):
        info = ShardInfo()
        check(load().desc_pgd_shard_info(self.handle, C.byref(info)))
        return info

    def shard_bind(self, t_send_ptr, t_recv_ptr, sall_ptr, stream_ptr=None):
        check(load().desc_pgd_shard_bind(self.handle, t_send_ptr, t_recv_ptr, sall_ptr, stream_ptr))

    def shard_colsum(self):
        check(load().desc_pgd_shard_colsum(self.handle))

    def shard_sweep(self):
        check(load().desc_pgd_shard_sweep(self.handle))

    def shard_finish(self, initial=0):
        check(load().desc_pgd_shard_finish(self.handle, initial))

    def shard_objective(self, phase):
        check(load().desc_pgd_shard_objective(self.handle, phase))

    # fused protocol: whole iterations enqueued from C (collectives = function pointers, e.g. RCCL's)
    def shard_set_collectives(self, comm=None, reduce_scatter=None, all_gather=None):
        c = Collectives(comm, C.cast(reduce_scatter, C.c_void_p) if reduce_scatter is not None else None,
                        C.cast(all_gather, C.c_void_p) if all_gather is not None else None)
        self._coll_keepalive = (reduce_scatter, all_gather)
        check(load().desc_pgd_shard_set_collectives(self.handle, C.byref(c)))

    def shard_start(self, params: Params):
        self._iters_cap = params.iters
        check(load().desc_pgd_shard_start(self.handle, C.byref(params)))

    def shard_iterate(self, n):
        check(load().desc_pgd_shard_iterate(self.handle, n))

    def shard_run(self, params: Params):
        r, bufs = self._result(params.iters)
        check(load().desc_pgd_shard_run(self.handle, C.byref(params), C.byref(r)))
        return self._pack(r, bufs)

    def stopped(self):
        f = C.c_int32()
        check(load().desc_pgd_stopped(self.handle, C.byref(f)))
        return bool(f.value)

    def destroy(self):
        if self.handle:
            load().desc_pgd_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


DTYPE_CODES = {np.dtype(np.float64): 0, np.dtype(np.int64): 1, np.dtype(np.int32): 2}      # DESC_DTYPE_*


def marshal_edges_native(Ind):
    """desc_marshal_edges: m x 2 array of 1-based node ids (float64 / int64 / int32, any strides) -> (n, ind_i, ind_j, sorted)."""
    if Ind.dtype not in DTYPE_CODES:
        Ind = Ind.astype(np.int64 if np.issubdtype(Ind.dtype, np.integer) else np.float64)
    m = Ind.shape[0]
    ii = np.empty(m, dtype=np.int32)
    jj = np.empty(m, dtype=np.int32)
    n, srt = C.c_int64(0), C.c_int32(0)
    item = Ind.dtype.itemsize
    check(load().desc_marshal_edges(C.c_void_p(Ind.ctypes.data), DTYPE_CODES[Ind.dtype], m, Ind.strides[0] // item, Ind.strides[1] // item,
                                    ptr(ii, I32P), ptr(jj, I32P), C.byref(n), C.byref(srt)))
    return int(n.value), ii, jj, bool(srt.value)


def marshal_rij_native(R, perm=None):
    """desc_marshal_rij: (3, 3, m) float64 array with any strides (+ edge permutation) -> the ABI's (m * 9,) buffer."""
    m = R.shape[2]
    out = np.empty(9 * m, dtype=np.float64)
    pp = None if perm is None else np.ascontiguousarray(perm, dtype=np.int64)
    check(load().desc_marshal_rij(ptr(R, F64P), m, R.strides[0] // 8, R.strides[1] // 8, R.strides[2] // 8, ptr(pp, I64P), ptr(out, F64P)))
    return out


def solve(prob: ProblemArrays, params: Params, want_w=False):
    """One-shot desc_pgd_solve: structure build + layout + run + download in one C call."""
    r = Result()
    bufs = dict(s_vec=out_buffer(prob.m), obj=out_buffer(params.iters), avg=out_buffer(params.iters))
    r.s_vec = ptr(bufs["s_vec"], F64P)
    r.obj_trace = ptr(bufs["obj"], F64P)
    r.avg_change_trace = ptr(bufs["avg"], F64P)
    check(load().desc_pgd_solve(C.byref(prob.c), C.byref(params), C.byref(r)))
    it = r.iters_run
    return dict(S_vec=bufs["s_vec"][:prob.m], obj=bufs["obj"][:it], avg=bufs["avg"][:it], iters_run=it, t_end=r.t_end,
                ms_upload=r.ms_upload, ms_cycle_d=r.ms_cycle_d, ms_pgd=r.ms_pgd, ms_total=r.ms_total, ms_structure=r.ms_structure)


def spectral_run(prob, weights=None, normalize_rows=False, tol=1e-13, max_iters=500, device=0):
    """desc_spectral_run[_dev] -> (R (3,3,n) Fortran-ordered, info dict).  prob: ProblemArrays or DeviceProblem."""
    n = prob.n
    R = out_buffer(9 * n)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    if w is not None and w.size != prob.m:
        raise ValueError("weights must have m entries")
    info = SpectralInfo()
    if isinstance(prob, DeviceProblem):
        check(load().desc_spectral_run_dev(prob.handle, ptr(w, F64P), 1 if normalize_rows else 0, tol, max_iters, ptr(R, F64P), C.byref(info)))
    else:
        check(load().desc_spectral_run(C.byref(prob.c), ptr(w, F64P), 1 if normalize_rows else 0, tol, max_iters, device,
                                       ptr(R, F64P), C.byref(info)))
    return R[:9 * n].reshape((3, 3, n), order="F"), dict(iters=info.iters, products=info.products, converged=bool(info.converged), residual=info.residual,
                                                        eigenvalues=list(info.eigenvalues), ms_total=info.ms_total)


def gcw_run(dprob: DeviceProblem, s_vec, tol=1e-13, max_iters=500):
    """desc_gcw_run_dev: GCW with the weights formed on the device from S_vec -> (R (3,3,n), info)."""
    n = dprob.n
    R = out_buffer(9 * n)
    S = np.ascontiguousarray(s_vec, dtype=np.float64)
    if S.size != dprob.m:
        raise ValueError("s_vec must have m entries")
    info = SpectralInfo()
    check(load().desc_gcw_run_dev(dprob.handle, ptr(S, F64P), tol, max_iters, ptr(R, F64P), C.byref(info)))
    return R[:9 * n].reshape((3, 3, n), order="F"), dict(iters=info.iters, products=info.products, converged=bool(info.converged), residual=info.residual,
                                                        eigenvalues=list(info.eigenvalues), ms_total=info.ms_total)


def cemp_run(prob, beta, max_iter, nsample, seed=0, device=0):
    b = np.ascontiguousarray(beta, dtype=np.float64).reshape(-1)
    S = out_buffer(prob.m)
    ms = C.c_double()
    L = load()
    if isinstance(prob, DeviceProblem):
        check(L.desc_cemp_run_dev(prob.handle, ptr(b, F64P), b.shape[0], int(max_iter), int(nsample), int(seed), ptr(S, F64P), C.byref(ms)))
    else:
        check(L.desc_cemp_run(C.byref(prob.c), ptr(b, F64P), b.shape[0], int(max_iter), int(nsample), int(seed), device, ptr(S, F64P),
                              C.byref(ms)))
    return S[:prob.m], ms.value


def refine_run(prob, s_vec, R_init, stop_threshold=1e-3, max_iters=100, device=0, verbose=False):
    """desc_refine_run[_dev] -> (R (3,3,n), info)."""
    n = prob.n
    S = np.ascontiguousarray(s_vec, dtype=np.float64)
    Ri = np.ascontiguousarray(np.asarray(R_init, dtype=np.float64).reshape(-1, order="F"))
    Ro = out_buffer(9 * n)
    if S.size != prob.m or Ri.size != 9 * n:
        raise ValueError("s_vec must have m entries and R_init 3 x 3 x n")
    info = RefineInfo(); info.verbose = 1 if verbose else 0
    L = load()
    if isinstance(prob, DeviceProblem):
        check(L.desc_refine_run_dev(prob.handle, ptr(S, F64P), ptr(Ri, F64P), stop_threshold, max_iters, ptr(Ro, F64P), C.byref(info)))
    else:
        check(L.desc_refine_run(C.byref(prob.c), ptr(S, F64P), ptr(Ri, F64P), stop_threshold, max_iters, device, ptr(Ro, F64P), C.byref(info)))
    return Ro[:9 * n].reshape((3, 3, n), order="F"), dict(iters=info.iters, cg_iters=info.cg_iters, score=info.score, ms_total=info.ms_total,
                                                        cg_unconverged=info.cg_unconverged, cg_residual=info.cg_residual)


def mst_run(prob, s_vec, device=0):
    """desc_mst_run[_dev] -> (R (3,3,n), tree edge indices ascending (n - 1,), sorted order)."""
    n = prob.n
    S = np.ascontiguousarray(s_vec, dtype=np.float64).reshape(-1)
    if S.size != prob.m:
        raise ValueError("s_vec must have m entries")
    R = out_buffer(9 * n)
    T = out_buffer(max(n - 1, 1), np.int32)
    L = load()
    if isinstance(prob, DeviceProblem):
        check(L.desc_mst_run_dev(prob.handle, ptr(S, F64P), ptr(R, F64P), ptr(T, I32P)))
    else:
        check(L.desc_mst_run(C.byref(prob.c), ptr(S, F64P), device, ptr(R, F64P), ptr(T, I32P)))
    return R[:9 * n].reshape((3, 3, n), order="F"), T[:n - 1].copy()


def mpls_run(prob, cemp_beta, cemp_max_iter, nsample, stop_threshold, max_iter, beta, tau, alpha, seed=0, device=0, verbose=False):
    """desc_mpls_run[_dev] -> (R_est (3,3,n), R_init (3,3,n), CEMP's SVec (m,), info dict); sorted edge order."""
    n, m = prob.n, prob.m
    vec = [np.ascontiguousarray(np.atleast_1d(np.asarray(v, dtype=np.float64)).reshape(-1)) for v in (cemp_beta, beta, tau, alpha)]
    if any(v.size == 0 for v in vec):
        raise ValueError("the reweighting / thresholding / cycle_info_ratio vectors need at least one entry")
    p = MplsParams(ptr(vec[0], F64P), vec[0].size, int(cemp_max_iter), int(nsample), 1 if verbose else 0, int(seed), float(stop_threshold),
                   int(max_iter), vec[1].size, ptr(vec[1], F64P), ptr(vec[2], F64P), ptr(vec[3], F64P), vec[2].size, vec[3].size)
    R_est, R_init, S = out_buffer(9 * n), out_buffer(9 * n), out_buffer(m)
    info = MplsInfo()
    L = load()
    if isinstance(prob, DeviceProblem):
        check(L.desc_mpls_run_dev(prob.handle, C.byref(p), ptr(R_est, F64P), ptr(R_init, F64P), ptr(S, F64P), C.byref(info)))
    else:
        check(L.desc_mpls_run(C.byref(prob.c), C.byref(p), device, ptr(R_est, F64P), ptr(R_init, F64P), ptr(S, F64P), C.byref(info)))
    shape = lambda R: R[:9 * n].reshape((3, 3, n), order="F")      # noqa: E731
    return shape(R_est), shape(R_init), S[:m], dict(iters=info.iters, cg_iters=info.cg_iters, cg_unconverged=info.cg_unconverged, m_pos=info.m_pos,
                                                    score=info.score, cg_residual=info.cg_residual, ms_cemp=info.ms_cemp, ms_mst=info.ms_mst,
                                                    ms_loop=info.ms_loop, ms_total=info.ms_total)


def irls_run(prob, mode, max_iter_l1=10, max_iter_irls=100, sigma_deg=5.0, R_init=None, order=None, device=0, verbose=False):
    """desc_irls_run[_dev] -> (R (3,3,n), R_l1 (3,3,n), info dict); sorted edge order, NaN outside the largest component.
    order: the caller's 0-based row of every sorted edge (marshal_edges' perm), or None."""
    n, m = prob.n, prob.m
    Ri = None if R_init is None else np.ascontiguousarray(np.asarray(R_init, dtype=np.float64).reshape(-1, order="F"))
    if Ri is not None and Ri.size != 9 * n:
        raise ValueError("Rinit must be 3 x 3 x n")
    od = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    if od is not None and od.size != m:
        raise ValueError("order must have m entries")
    p = IrlsParams(int(mode), int(max_iter_l1), int(max_iter_irls), 1 if verbose else 0, float(sigma_deg), ptr(Ri, F64P), ptr(od, I32P))
    R, R1 = out_buffer(9 * n), out_buffer(9 * n)
    info = IrlsInfo()
    L = load()
    if isinstance(prob, DeviceProblem):
        check(L.desc_irls_run_dev(prob.handle, C.byref(p), ptr(R, F64P), ptr(R1, F64P), C.byref(info)))
    else:
        check(L.desc_irls_run(C.byref(prob.c), C.byref(p), device, ptr(R, F64P), ptr(R1, F64P), C.byref(info)))
    shape = lambda a: a[:9 * n].reshape((3, 3, n), order="F")      # noqa: E731
    return shape(R), shape(R1), {k: getattr(info, k) for k, _ in IrlsInfo._fields_}


def default_lp_params():
    p = LpParams()
    load().desc_lp_params_default(C.byref(p))
    return p


def lp_sij_run(prob, params=None, device=0, want_y=False, want_k=True):
    """desc_lp_sij_run[_dev] -> (S_vec (m,), y (m_pos, nsample, 2) or None, k (m_pos, nsample) 1-based or None, info dict); sorted edge order.
    With want_k the info dict also holds "pos_edges", the 0-based (sorted) edge ids of the LP's variables.
    prob: ProblemArrays or DeviceProblem; params: LpParams (None: the defaults)."""
    m = prob.m
    p = params if params is not None else default_lp_params()
    L = load()
    S = out_buffer(m)
    info = LpInfo()

    def call(pp, y, k):
        if isinstance(prob, DeviceProblem):
            check(L.desc_lp_sij_run_dev(prob.handle, C.byref(pp), ptr(S, F64P), ptr(y, F64P), ptr(k, I32P), C.byref(info)))
        else:
            check(L.desc_lp_sij_run(C.byref(prob.c), C.byref(pp), device, ptr(S, F64P), ptr(y, F64P), ptr(k, I32P), C.byref(info)))

    y = k = None
    ns = int(p.nsample)
    mp = m
    if want_y or want_k:                    # the buffers are sized by nsample and m_pos: a call without steps and outputs returns the sizes
        q = LpParams.from_buffer_copy(p)
        q.max_iter = 0
        call(q, None, None)
        ns, mp = int(info.nsample), int(info.m_pos)
    if want_y:
        y = out_buffer(2 * ns * mp)
    pos = None
    if want_k:
        k = out_buffer(ns * mp, np.int32)
        pos = out_buffer(mp, np.int32)
        p = LpParams.from_buffer_copy(p)
        p.pos_out = ptr(pos, I32P)
    call(p, y, k)
    out = {name: getattr(info, name) for name, _ in LpInfo._fields_}
    mp, ns = int(info.m_pos), int(info.nsample)
    if y is not None:
        y = y[:2 * ns * mp].reshape(mp, ns, 2)
    if k is not None:
        k = k[:ns * mp].reshape(mp, ns)
        out["pos_edges"] = pos[:mp].copy()
    return S[:m], y, k, out


def spmm_variants(dprob: DeviceProblem, reps=20):
    """desc_debug_spmm_variants: ms per block-SpMM product, vector-FMA vs v_mfma_f64_4x4x4 form (measurement hook)."""
    out = out_buffer(4)
    check(load().desc_debug_spmm_variants(dprob.handle, int(reps), ptr(out, F64P)))
    return dict(ms_valu=float(out[0]), ms_mfma=float(out[1]), max_abs_diff=float(out[2]), mfma_layout=int(out[3]))


def trim_memory():
    """Give the device blocks the library has parked for reuse back to the driver; returns the bytes released."""
    return int(load().desc_trim_memory())


def host_exports():
    """How often this process exported a device-built structure to host memory (diagnostics)."""
    return int(load().desc_structure_host_exports())


def device_count():
    rc = load().desc_device_count()
    if rc < 0:
        raise DescError(load().desc_last_error().decode())
    return rc


# ---- test hooks into the Lie-algebraic averaging core (desc_test_laa_* / desc_test_irls_*, include/desc_amd.h): one operation on
# NumPy arrays, launched as the library launches it.  Used by tests/test_gpu_laa_maps.py only.
def _f64(a, size=None):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    if size is not None and a.size != size:
        raise ValueError(f"expected {size} doubles, got {a.size}")
    return a


def hook_r2q(R, transpose=False, edge_grid=False, device=0):
    """R: (count, 9) column-major blocks -> (count, 4) quaternions."""
    R = _f64(R); count = R.size // 9
    Q = out_buffer(4 * count)
    check(load().desc_test_laa_r2q(ptr(R, F64P), count, int(bool(transpose)), int(bool(edge_grid)), device, ptr(Q, F64P)))
    return Q[:4 * count].reshape(count, 4)


def hook_q2r(Q, device=0):
    """Q: (n, 4) -> (n, 9) column-major blocks."""
    Q = _f64(Q); n = Q.size // 4
    R = out_buffer(9 * n)
    check(load().desc_test_laa_q2r(ptr(Q, F64P), n, device, ptr(R, F64P)))
    return R[:9 * n].reshape(n, 9)


def hook_edge_log(dprob: DeviceProblem, Q, QQ):
    m = dprob.m
    Q, QQ = _f64(Q, 4 * dprob.n), _f64(QQ, 4 * m)
    B = out_buffer(3 * m)
    check(load().desc_test_laa_edge_log(dprob.handle, ptr(Q, F64P), ptr(QQ, F64P), m, ptr(B, F64P)))
    return B[:3 * m].reshape(m, 3)


def hook_rhs(dprob: DeviceProblem, w, B):
    n, m = dprob.n, dprob.m
    w, B = _f64(w, m), _f64(B, 3 * m)
    rhs, diag = out_buffer(3 * n), out_buffer(n)
    check(load().desc_test_laa_rhs(dprob.handle, ptr(w, F64P), ptr(B, F64P), m, ptr(rhs, F64P), ptr(diag, F64P)))
    return rhs[:3 * n].reshape(n, 3), diag[:n]


def hook_pcg(dprob: DeviceProblem, w, rhs, diag, act=(1, 1, 1), w3=False):
    """-> dict(x (n, 3), bad (3,), rnorm (3,), bnorm (3,), total, unconverged, worst); rnorm / bnorm are squared norms."""
    n, m = dprob.n, dprob.m
    w, rhs, diag = _f64(w, 3 * m if w3 else m), _f64(rhs, 3 * n), _f64(diag, 3 * n if w3 else n)
    act = np.ascontiguousarray(act, dtype=np.int32)
    x, bad, rn, bn = out_buffer(3 * n), out_buffer(3, np.int32), out_buffer(3), out_buffer(3)
    tot, unc, worst = out_buffer(1, np.int32), out_buffer(1, np.int32), out_buffer(1)
    check(load().desc_test_laa_pcg(dprob.handle, int(bool(w3)), ptr(w, F64P), ptr(rhs, F64P), ptr(diag, F64P), m, ptr(act, I32P), ptr(x, F64P),
                                   ptr(bad, I32P), ptr(rn, F64P), ptr(bn, F64P), ptr(tot, I32P), ptr(unc, I32P), ptr(worst, F64P)))
    return dict(x=x[:3 * n].reshape(n, 3), bad=bad[:3].copy(), rnorm=rn[:3].copy(), bnorm=bn[:3].copy(), total=int(tot[0]),
                unconverged=int(unc[0]), worst=float(worst[0]))


def hook_node_update(x, Q, l1=False, device=0):
    """-> (Q_new (n, 4), Wv (n, 3) or None, score): score = sum of |x_v| over v >= 1, or its max for the L1 variant."""
    Q = _f64(Q); n = Q.size // 4
    x = _f64(x, 3 * n)
    Qo, sc = out_buffer(4 * n), out_buffer(1)
    if l1:
        check(load().desc_test_irls_node_update(ptr(x, F64P), ptr(Q, F64P), n, device, ptr(Qo, F64P), ptr(sc, F64P)))
        return Qo[:4 * n].reshape(n, 4), None, float(sc[0])
    Wv = out_buffer(3 * n)
    check(load().desc_test_laa_node_update(ptr(x, F64P), ptr(Q, F64P), n, device, ptr(Qo, F64P), ptr(Wv, F64P), ptr(sc, F64P)))
    return Qo[:4 * n].reshape(n, 4), Wv[:3 * n].reshape(n, 3), float(sc[0])


def hook_weights(x, thresh, device=0):
    x = _f64(x); m = x.size
    w = out_buffer(m)
    check(load().desc_test_laa_weights(ptr(x, F64P), m, float(thresh), device, ptr(w, F64P)))
    return w[:m]


def hook_irls_weights(dprob: DeviceProblem, x, B, mode, sigma):
    n, m = dprob.n, dprob.m
    x, B = _f64(x, 3 * n), _f64(B, 3 * m)
    w = out_buffer(m)
    check(load().desc_test_irls_weights(dprob.handle, ptr(x, F64P), ptr(B, F64P), m, int(mode), float(sigma), ptr(w, F64P)))
    return w[:m]


HOOK_QCAP = 1 << 20      # laa.hip's QCAP: the capacity the library itself passes to device_quantile (the hook refuses more)


def hook_quantile(x, p, cap=HOOK_QCAP, device=0):
    x = _f64(x)
    out = out_buffer(1)
    check(load().desc_test_laa_quantile(ptr(x, F64P), x.size, float(p), int(cap), device, ptr(out, F64P)))
    return float(out[0])


def hook_project(rij, order=None, only=-1, device=0):
    """rij: (m, 9) blocks Rij -> dict(P (m, 9), bad_row (-1: none), warn, info (5,))."""
    rij = _f64(rij); m = rij.size // 9
    od = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    P, bad, warn, info = out_buffer(9 * m), out_buffer(1, np.int32), out_buffer(1, np.int32), out_buffer(5)
    check(load().desc_test_irls_project(ptr(rij, F64P), ptr(od, I32P), m, int(only), device, ptr(P, F64P), ptr(bad, I32P), ptr(warn, I32P),
                                        ptr(info, F64P)))
    return dict(P=P[:9 * m].reshape(m, 9), bad_row=int(bad[0]), warn=int(warn[0]), info=info[:5].copy())


# ---- test hooks into the primal-dual L1 solver (desc_test_irls_pd_*, include/desc_amd.h).  Used by tests/test_gpu_pd_kernels.py and
# tests/test_gpu_pd_solver.py only.
PD_STAGES = ("absmax", "init", "gather0", "gather1", "gather2", "pre", "dir", "resid", "resid_trial", "accept")      # DESC_TEST_PD_*
PD_EDGE = ("y", "Ax", "u", "f1", "f2", "l1", "l2", "w2", "s1", "s2", "sx", "ev1", "ev2", "Adx", "du", "d1", "d2")    # m x 3 each
PD_NODE = ("x", "Atv", "w1p", "dg", "dx", "Atdv")                                                                    # n x 3 each
PD_RG = 256                                                                                                          # irls_math.h
PD_TRACE = ("part", "bad", "s", "trials", "verdict", "sdg", "tau", "resnorm")


def hook_pd_stage(dprob: DeviceProblem, stage, state, part, tau=(1, 1, 1), s=(0, 0, 0), ymax=(0, 0, 0), act=(1, 1, 1)):
    """One kernel of the primal-dual solver on a snapshot.  state: dict of the PD_EDGE (m, 3) and PD_NODE (n, 3) arrays; part: (PD_RG, 6)
    as the launch finds it.  -> (dict of all arrays after the launch, part (PD_RG * 6,) raw: [PD_RG][K] from its start)."""
    n, m = dprob.n, dprob.m
    edge = np.concatenate([_f64(state[k], 3 * m) for k in PD_EDGE])
    node = np.concatenate([_f64(state[k], 3 * n) for k in PD_NODE])
    eb, nb, pb = out_buffer(edge.size), out_buffer(node.size), out_buffer(6 * PD_RG)
    eb[:] = edge; nb[:] = node; pb[:] = _f64(part, 6 * PD_RG)
    sc = [np.ascontiguousarray(v, dtype=np.float64).reshape(3) for v in (tau, s, ymax)]
    act = np.ascontiguousarray(act, dtype=np.int32).reshape(3)
    check(load().desc_test_irls_pd_stage(dprob.handle, PD_STAGES.index(stage), ptr(sc[0], F64P), ptr(sc[1], F64P), ptr(sc[2], F64P),
                                         ptr(act, I32P), m, n, ptr(eb, F64P), ptr(nb, F64P), ptr(pb, F64P)))
    out = {k: eb[3 * m * t:3 * m * (t + 1)].reshape(m, 3).copy() for t, k in enumerate(PD_EDGE)}
    out.update({k: nb[3 * n * t:3 * n * (t + 1)].reshape(n, 3).copy() for t, k in enumerate(PD_NODE)})
    return out, pb[:6 * PD_RG].copy()


def hook_pd_solve(dprob: DeviceProblem, B, pdmaxiter):
    """The whole primal-dual solve of B (m, 3) -> dict(x, u, l1, l2, Ax, Atv, steps, ill, stuck, solves, cg_total, cg_unconverged,
    trace (records, 3, 8): the fields of PD_TRACE per step (record 0: the start) and coordinate)."""
    n, m = dprob.n, dprob.m
    B = _f64(B, 3 * m)
    cap = int(pdmaxiter) + 1
    x, st, cnt = out_buffer(3 * n), out_buffer(12 * m + 3 * n), out_buffer(6, np.int32)
    tr, tl = out_buffer(24 * max(cap, 1)), out_buffer(1, np.int32)
    check(load().desc_test_irls_pd_solve(dprob.handle, ptr(B, F64P), m, n, int(pdmaxiter), ptr(x, F64P), ptr(st, F64P), ptr(cnt, I32P),
                                         ptr(tr, F64P), max(cap, 0), ptr(tl, I32P)))
    out = dict(x=x[:3 * n].reshape(n, 3).copy(), Atv=st[12 * m:12 * m + 3 * n].reshape(n, 3).copy())
    for t, k in enumerate(("u", "l1", "l2", "Ax")):
        out[k] = st[3 * m * t:3 * m * (t + 1)].reshape(m, 3).copy()
    out.update(zip(("steps", "ill", "stuck", "solves", "cg_total", "cg_unconverged"), (int(v) for v in cnt[:6])))
    out["trace"] = tr[:24 * int(tl[0])].reshape(-1, 3, 8).copy()
    return out


# ---- test hooks into the Spectral / GCW eigen-solve (desc_test_spectral_* / desc_test_small_*, include/desc_amd.h).  Used by
# tests/test_gpu_spectral_kernels.py and tests/test_spectral_host.py only.  grid = 0: the product path's grid rule.
SPECTRAL_BW = 6          # spectral.hip's BW: columns of the iterated block


def hook_spectral_weights(S, device=0):
    S = _f64(S); m = S.size
    w = out_buffer(m)
    check(load().desc_test_spectral_weights(ptr(S, F64P), m, device, ptr(w, F64P)))
    return w[:m].copy()


def hook_spectral_row_wsum(dprob: DeviceProblem, w=None, grid=0):
    w = None if w is None else _f64(w, dprob.m)
    deg = out_buffer(dprob.n)
    check(load().desc_test_spectral_row_wsum(dprob.handle, ptr(w, F64P), dprob.m, int(grid), ptr(deg, F64P)))
    return deg[:dprob.n].copy()


def hook_spectral_assemble(dprob: DeviceProblem, w=None, dinv=None, grid=0):
    """-> (9, 2m): component q = r + 3k of CSR slot t at [q, t], as the library stores the blocks."""
    m = dprob.m
    w = None if w is None else _f64(w, m)
    dinv = None if dinv is None else _f64(dinv, dprob.n)
    blocks = out_buffer(18 * m)
    check(load().desc_test_spectral_assemble(dprob.handle, ptr(w, F64P), ptr(dinv, F64P), m, int(grid), ptr(blocks, F64P)))
    return blocks[:18 * m].reshape(9, 2 * m).copy()


def hook_spectral_spmm(dprob: DeviceProblem, blocks, x, z, alpha, s1, s2, z_is_y=False, form=0, grid=0):
    """y = alpha A x + s1 x + s2 z -> (3n, 6); blocks as hook_spectral_assemble returns them."""
    rows = 3 * dprob.n
    blocks, x, z = _f64(blocks, 18 * dprob.m), _f64(x, rows * SPECTRAL_BW), _f64(z, rows * SPECTRAL_BW)
    if blocks.size == 0:
        blocks = np.zeros(1)
    y = out_buffer(rows * SPECTRAL_BW)
    check(load().desc_test_spectral_spmm(dprob.handle, ptr(blocks, F64P), ptr(x, F64P), ptr(z, F64P), int(bool(z_is_y)), int(form), int(grid),
                                         float(alpha), float(s1), float(s2), ptr(y, F64P)))
    return y[:rows * SPECTRAL_BW].reshape(rows, SPECTRAL_BW).copy()


def hook_spectral_gram(X, Y, grid=0, device=0):
    """-> (X'Y, Y'Y), 6 x 6 each."""
    X = _f64(X); rows = X.size // SPECTRAL_BW
    Y = _f64(Y, X.size)
    G1, G2 = out_buffer(36), out_buffer(36)
    check(load().desc_test_spectral_gram(ptr(X, F64P), ptr(Y, F64P), rows, int(grid), device, ptr(G1, F64P), ptr(G2, F64P)))
    return G1[:36].reshape(6, 6).copy(), G2[:36].reshape(6, 6).copy()


def hook_spectral_residual(X, Y, Z3, theta, grid=0, device=0):
    """-> r2 (3,): |Y z_c - theta_c X z_c|^2 for the columns z_c of Z3 (6 x 3)."""
    X = _f64(X); rows = X.size // SPECTRAL_BW
    Y, Z3, theta = _f64(Y, X.size), _f64(Z3, 18), _f64(theta, 3)
    r2 = out_buffer(3)
    check(load().desc_test_spectral_residual(ptr(X, F64P), ptr(Y, F64P), rows, ptr(Z3, F64P), ptr(theta, F64P), int(grid), device, ptr(r2, F64P)))
    return r2[:3].copy()


def hook_spectral_combine(Y, Cm, grid=0, device=0):
    Y = _f64(Y); rows = Y.size // SPECTRAL_BW
    Cm = _f64(Cm, 36)
    Xn = out_buffer(Y.size)
    check(load().desc_test_spectral_combine(ptr(Y, F64P), rows, ptr(Cm, F64P), int(grid), device, ptr(Xn, F64P)))
    return Xn[:Y.size].reshape(rows, SPECTRAL_BW).copy()


def hook_small_jacobi(A):
    """-> (w descending, V with the eigenvectors in its columns)."""
    A = np.asarray(A, dtype=np.float64); N = A.shape[0]
    a = _f64(A, N * N)
    w, V = out_buffer(N), out_buffer(N * N)
    check(load().desc_test_small_jacobi(N, ptr(a, F64P), ptr(w, F64P), ptr(V, F64P)))
    return w[:N].copy(), V[:N * N].reshape(N, N).copy()


def hook_small_ortho(G, Z=None):
    """-> (ok, C 6 x 6)."""
    G = _f64(G, 36)
    Z = None if Z is None else _f64(Z, 36)
    Cm, ok = out_buffer(36), out_buffer(1, np.int32)
    check(load().desc_test_small_ortho(ptr(G, F64P), ptr(Z, F64P), ptr(Cm, F64P), ptr(ok, I32P)))
    return bool(ok[0]), Cm[:36].reshape(6, 6).copy()


def hook_small_project(M):
    """M: (count, 3, 3) -> their projections onto SO(3), (count, 3, 3)."""
    M = _f64(M); count = M.size // 9
    R = out_buffer(9 * count)
    check(load().desc_test_small_project(ptr(M, F64P), count, ptr(R, F64P)))
    return R[:9 * count].reshape(count, 3, 3).copy()


def hook_small_ritz_tail(V, dinv=None):
    """V: (3n, 3) -> R (3, 3, n) Fortran-ordered."""
    V = _f64(V); n = V.size // 9
    dinv = None if dinv is None else _f64(dinv, n)
    R = out_buffer(9 * n)
    check(load().desc_test_small_ritz_tail(ptr(V, F64P), ptr(dinv, F64P), n, ptr(R, F64P)))
    return R[:9 * n].reshape((3, 3, n), order="F").copy()
