"""ctypes binding of liblsfm_hip.so (C ABI: include/lsfm.h).

This module is plumbing only: every numerical step runs in the hand-written HIP library.  There is no CPU
fallback -- importing works anywhere, but creating a Context without a usable MI355X (or without the built
library) raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblsfm_hip.so")
_LIB = None

LSFM_OK = 0
LSFM_NOT_CONVERGED = 1


class LsfmMap(C.Structure):
    _fields_ = [("Ref", C.c_int), ("FRef", C.c_int), ("m", C.c_int), ("n", C.c_int), ("nU", C.c_int), ("nW", C.c_int),
                ("ScaP", C.c_int), ("Fix", C.c_int), ("Sign", C.c_int), ("FScaP", C.c_int), ("FFix", C.c_int),
                ("stno", C.POINTER(C.c_int)), ("stVal", C.POINTER(C.c_double)),
                ("U", C.POINTER(C.c_double)), ("Ui", C.POINTER(C.c_int)), ("Uj", C.POINTER(C.c_int)),
                ("W", C.POINTER(C.c_double)), ("photo", C.POINTER(C.c_int)), ("feature", C.POINTER(C.c_int)),
                ("V", C.POINTER(C.c_double)), ("FBlock", C.POINTER(C.c_int)), ("pose_origin", C.POINTER(C.c_int))]


class LsfmStats(C.Structure):
    _fields_ = [("t_total_ms", C.c_double), ("t_transform_ms", C.c_double), ("t_join_ms", C.c_double),
                ("t_schur_ms", C.c_double), ("t_pcg_ms", C.c_double), ("t_backsub_ms", C.c_double),
                ("pcg_iterations", C.c_long), ("spmv_launches", C.c_long), ("spmv_ms", C.c_double),
                ("spmv_bytes", C.c_double), ("spmv_nnzb_upper_last", C.c_long), ("spmv_rows_last", C.c_long),
                ("max_rel_residual", C.c_double), ("levels", C.c_int), ("joins", C.c_int), ("transforms", C.c_int),
                ("not_converged", C.c_int), ("schur_launches", C.c_long), ("trf_launches", C.c_long),
                ("schur_ms", C.c_double), ("schur_bytes", C.c_double), ("trf_ms", C.c_double), ("trf_bytes", C.c_double),
                ("schur_flops", C.c_double), ("upload_ms", C.c_double), ("attempts", C.c_int),
                ("s_digest", C.c_ulonglong), ("factor_digest", C.c_ulonglong), ("dist_solves", C.c_int), ("dist_work_total", C.c_double), ("dist_work_shared", C.c_double), ("refactor_mismatch", C.c_int), ("s_rebuild_mismatch", C.c_int), ("small_levels", C.c_int), ("t_small_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class LsfmError(RuntimeError):
    pass


# include/lsfm.h lsfm_allreduce_fn: (user, offset_bytes, count, dtype, hip_stream) -> 0 on success
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p)
LSFM_DTYPE_F64, LSFM_DTYPE_I64 = 0, 1
JOINT_GATE_MAX = 2048                   # include/lsfm.h LSFM_JOINT_GATE_MAX
JOINT_GATE_TAU = 11.344866730144373     # chi^2_3 at 0.99: the default tau of feature_pair_joint_gate and -jgate


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise LsfmError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        P = C.POINTER
        dp, ip, vp = P(C.c_double), P(C.c_int), C.c_void_p
        L.lsfm_context_create.argtypes = [C.c_int, C.c_size_t, P(vp)]
        L.lsfm_context_destroy.argtypes = [vp]
        L.lsfm_context_destroy.restype = None
        L.lsfm_set_pcg.argtypes = [vp, C.c_double, C.c_int]
        L.lsfm_set_precision.argtypes = [vp, C.c_int]
        L.lsfm_set_small_solve.argtypes = [vp, C.c_int]
        L.lsfm_set_spmv_variant.argtypes = [vp, C.c_int]
        L.lsfm_set_covcols_panel.argtypes = [vp, C.c_int]
        L.lsfm_last_error.argtypes = [vp]
        L.lsfm_last_error.restype = C.c_char_p
        L.lsfm_stream.argtypes = [vp]
        L.lsfm_stream.restype = vp
        L.lsfm_map_release.argtypes = [P(LsfmMap)]
        L.lsfm_map_release.restype = None
        L.lsfm_transform_stereo.argtypes = [vp, P(LsfmMap), C.c_int, P(LsfmMap)]
        L.lsfm_transform_mono.argtypes = [vp, P(LsfmMap), C.c_int, C.c_int, C.c_int, P(LsfmMap)]
        L.lsfm_join_stereo.argtypes = [vp, P(LsfmMap), P(LsfmMap), P(LsfmMap), dp, dp]
        L.lsfm_join_mono.argtypes = [vp, P(LsfmMap), P(LsfmMap), P(LsfmMap), dp, dp]
        L.lsfm_solve_stereo.argtypes = [vp, dp, dp, dp, dp, dp, dp, ip, ip, ip, ip, C.c_int, C.c_int, C.c_int, C.c_int, dp]
        L.lsfm_solve_mono.argtypes = [vp, dp, dp, dp, dp, dp, dp, ip, ip, ip, ip, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, dp]
        L.lsfm_tree_upload.argtypes = [vp, P(LsfmMap), C.c_int, C.c_int, P(vp)]
        L.lsfm_tree_run.argtypes = [vp, vp, P(LsfmStats)]
        L.lsfm_tree_set_final_reanchor.argtypes = [vp, C.c_int]
        L.lsfm_tree_set_plans.argtypes = [vp, C.c_int]
        L.lsfm_tree_export_size.argtypes = [vp, vp]
        L.lsfm_tree_export_size.restype = C.c_size_t
        L.lsfm_tree_export_dev.argtypes = [vp, vp, vp, C.c_size_t]
        L.lsfm_packed_size.argtypes = [vp]
        L.lsfm_packed_size.restype = C.c_size_t
        L.lsfm_tree_upload_dev.argtypes = [vp, P(vp), C.c_int, C.c_int, P(vp)]
        L.lsfm_tree_reload_dev.argtypes = [vp, vp, P(vp), C.c_int]
        L.lsfm_tree_set_comm.argtypes = [vp, C.c_int, C.c_int, ALLREDUCE_FN, vp, vp, C.c_size_t]
        L.lsfm_tree_set_comm_blocks.argtypes = [vp, C.c_int]
        L.lsfm_tree_export_slice_sizes.argtypes = [vp, vp, C.c_int, P(C.c_size_t)]
        L.lsfm_tree_export_slice_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t]
        L.lsfm_tree_download.argtypes = [vp, vp, P(LsfmMap)]
        L.lsfm_tree_set_stop_level.argtypes = [vp, C.c_int]
        L.lsfm_tree_node_count.argtypes = [vp, vp]
        L.lsfm_tree_download_node.argtypes = [vp, vp, C.c_int, P(LsfmMap)]
        L.lsfm_tree_download_state.argtypes = [vp, vp, ip, ip, ip, dp, C.c_size_t]
        L.lsfm_tree_free.argtypes = [vp, vp]
        L.lsfm_tree_free.restype = None
        L.lsfm_divide_conquer.argtypes = [vp, P(LsfmMap), C.c_int, C.c_int, P(LsfmMap), P(LsfmStats)]
        L.lsfm_read_localmap.argtypes = [C.c_char_p, C.c_int, P(LsfmMap)]
        L.lsfm_write_localmap.argtypes = [C.c_char_p, C.c_int, P(LsfmMap)]
        L.lsfm_read_localmaps.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, P(LsfmMap), P(C.c_int)]
        L.lsfm_write_mapset.argtypes = [C.c_char_p, P(LsfmMap), C.c_int, C.c_int]
        L.lsfm_mapset_info.argtypes = [C.c_char_p, P(C.c_int), P(C.c_int)]
        L.lsfm_read_mapset.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, P(LsfmMap)]
        L.lsfm_save_state_bin.argtypes = [C.c_char_p, P(C.c_double), P(C.c_int), C.c_int]
        L.lsfm_save_state.argtypes = [C.c_char_p, dp, ip, C.c_int]
        L.lsfm_save_poses.argtypes = [C.c_char_p, C.c_char_p, ip, dp, C.c_int]
        L.lsfm_schur_pattern.argtypes = [vp, ip, ip, ip, ip, C.c_int, C.c_int, C.c_int, C.c_int, ip, ip, C.c_int, ip]
        L.lsfm_symbolic_analyse.argtypes = [C.c_int, ip, ip, ip, C.c_int, ip, ip, ip, C.c_int, ip, dp]
        L.lsfm_inverse_v.argtypes = [vp, dp, C.c_int, C.c_int]
        L.lsfm_selftest_vinv.argtypes = [vp, dp, dp, C.c_int, C.c_int, dp, dp]
        L.lsfm_gn_polish.argtypes = [vp, P(LsfmMap), C.c_int, C.c_int, P(LsfmMap), C.c_int, dp, dp, ip]
        L.lsfm_gn_polish_robust.argtypes = [vp, P(LsfmMap), C.c_int, C.c_int, P(LsfmMap), C.c_int, C.c_int, C.c_double, dp, dp, ip, dp, dp]
        L.lsfm_map_chi2.argtypes = [vp, P(LsfmMap), C.c_int, C.c_int, P(LsfmMap), dp, ip]
        L.lsfm_map_feature_chi2.argtypes = [vp, P(LsfmMap), C.c_int, C.c_int, P(LsfmMap), dp, dp]
        L.lsfm_gn_polish_robust_features.argtypes = [vp, P(LsfmMap), C.c_int, C.c_int, P(LsfmMap), C.c_int, C.c_int, C.c_double, dp, dp, ip, dp, dp]
        L.lsfm_gn_linearise.argtypes = [vp, P(LsfmMap), C.c_int, C.c_int, P(LsfmMap), dp, P(LsfmMap), dp, dp]
        L.lsfm_gn_linearise_timed.argtypes = [vp, P(LsfmMap), C.c_int, C.c_int, P(LsfmMap), dp, P(LsfmMap), dp, dp, dp, ip]
        L.lsfm_gn_linearise_features.argtypes = [vp, P(LsfmMap), C.c_int, C.c_int, P(LsfmMap), dp, dp, P(LsfmMap), dp, dp]
        L.lsfm_gn_linearise_features_timed.argtypes = [vp, P(LsfmMap), C.c_int, C.c_int, P(LsfmMap), dp, dp, P(LsfmMap), dp, dp, dp, ip]
        L.lsfm_solve_features.argtypes = [vp, dp, dp, dp, dp, dp, dp, C.c_int, C.c_int, ip, ip]
        L.lsfm_map_covariance.argtypes = [vp, P(LsfmMap), C.c_int, dp, dp, dp, C.c_int, ip]
        L.lsfm_map_covariance_timed.argtypes = [vp, P(LsfmMap), C.c_int, dp, dp, dp, C.c_int, ip, dp]
        L.lsfm_save_covariances.argtypes = [C.c_char_p, C.c_char_p, ip, C.c_int, C.c_int, dp, dp]
        L.lsfm_read_covariances.argtypes = [C.c_char_p, C.c_int, ip, dp, C.c_int, ip]
        L.lsfm_map_covariance_columns.argtypes = [vp, P(LsfmMap), C.c_int, ip, C.c_int, dp, dp, dp, ip, dp]
        L.lsfm_map_covariance_columns_timed.argtypes = [vp, P(LsfmMap), C.c_int, ip, C.c_int, dp, dp, dp, ip, dp, dp]
        L.lsfm_map_covariance_feature_columns.argtypes = [vp, P(LsfmMap), C.c_int, ip, C.c_int, dp, dp, dp, ip, dp]
        L.lsfm_map_covariance_feature_columns_timed.argtypes = [vp, P(LsfmMap), C.c_int, ip, C.c_int, dp, dp, dp, ip, dp, dp]
        L.lsfm_map_feature_pair_gate.argtypes = [vp, P(LsfmMap), C.c_int, ip, C.c_int, dp, dp, ip, dp]
        L.lsfm_map_feature_pair_gate_timed.argtypes = [vp, P(LsfmMap), C.c_int, ip, C.c_int, dp, dp, ip, dp, dp]
        L.lsfm_map_merge_features.argtypes = [vp, P(LsfmMap), C.c_int, ip, C.c_int, P(LsfmMap), dp, ip, ip, ip, dp]
        L.lsfm_map_merge_features_timed.argtypes = [vp, P(LsfmMap), C.c_int, ip, C.c_int, P(LsfmMap), dp, ip, ip, ip, dp, dp]
        L.lsfm_map_feature_pair_joint_gate.argtypes = [vp, P(LsfmMap), C.c_int, ip, C.c_int, ip, C.c_double, ip, dp, dp, dp, ip, ip, dp, ip, dp]
        L.lsfm_map_feature_pair_joint_gate_timed.argtypes = [vp, P(LsfmMap), C.c_int, ip, C.c_int, ip, C.c_double, ip, dp, dp, dp, ip, ip, dp, ip, dp, dp]
        L.lsfm_selftest_pair_select.argtypes = [vp, C.c_int, dp, dp, ip, ip, C.c_double, ip, dp, dp, ip, ip]
        L.lsfm_save_joint_gate.argtypes = [C.c_char_p, ip, C.c_int, ip, dp, dp, C.c_int, C.c_int, C.c_double]
        L.lsfm_read_joint_gate.argtypes = [C.c_char_p, ip, ip, dp, dp, C.c_int, ip, dp]
        L.lsfm_merge_structure.argtypes = [P(LsfmMap), ip, C.c_int, ip, ip, ip, ip, ip, ip, C.c_int, ip, C.c_char_p, C.c_int]
        llp = P(C.c_longlong)
        L.lsfm_map_feature_pair_candidates.argtypes = [vp, P(LsfmMap), dp, C.c_double, C.c_double, ip, dp, dp, C.c_longlong, llp]
        L.lsfm_map_feature_pair_candidates_timed.argtypes = [vp, P(LsfmMap), dp, C.c_double, C.c_double, ip, dp, dp, C.c_longlong, llp, dp, llp]
        L.lsfm_save_pair_list.argtypes = [C.c_char_p, ip, C.c_longlong]
        L.lsfm_read_pair_list.argtypes = [C.c_char_p, ip, C.c_longlong, llp]
        L.lsfm_save_merge_report.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_double, ip]
        L.lsfm_read_merge_report.argtypes = [C.c_char_p, ip, ip, ip, dp, ip, C.c_int]
        L.lsfm_save_cov_columns.argtypes = [C.c_char_p, ip, C.c_int, ip, C.c_int, dp]
        L.lsfm_read_cov_columns.argtypes = [C.c_char_p, ip, ip, dp, C.c_int, ip]
        L.lsfm_save_pair_gate.argtypes = [C.c_char_p, ip, C.c_int, dp, dp]
        L.lsfm_read_pair_gate.argtypes = [C.c_char_p, ip, ip, dp, dp, C.c_int, ip]
        L.lsfm_map_marginalise.argtypes = [vp, P(LsfmMap), P(C.c_ubyte), P(LsfmMap)]
        L.lsfm_map_marginalise_timed.argtypes = [vp, P(LsfmMap), P(C.c_ubyte), P(LsfmMap), dp]
        ub = P(C.c_ubyte)
        L.lsfm_map_marginalise_poses.argtypes = [vp, P(LsfmMap), C.c_int, ub, ub, P(LsfmMap)]
        L.lsfm_map_marginalise_poses_timed.argtypes = [vp, P(LsfmMap), C.c_int, ub, ub, P(LsfmMap), dp, ip]
        L.lsfm_marg_pose_structure.argtypes = [P(LsfmMap), C.c_int, ub, ub, ub, ip, ip, ip, C.c_int, ip, ip, ip, C.c_int, ip, C.c_char_p, C.c_int]
        L.lsfm_gn_structure.argtypes = [P(LsfmMap), C.c_int, C.c_int, P(LsfmMap), C.c_int, C.c_int, ip, ip, ip, ip, ip, C.c_int, ip, ip, C.c_int, ip, ip, ip,
                                        C.c_int, ip, ip, C.c_int, ip, ip, ip, ip, C.c_int, C.c_char_p, C.c_int]
        L.lsfm_tree_export_reduced_size.argtypes = [vp, vp, ip, C.c_int, P(C.c_size_t)]
        L.lsfm_tree_export_reduced_dev.argtypes = [vp, vp, ip, C.c_int, vp, C.c_size_t]
        L.lsfm_tree_export_reduced_dev_timed.argtypes = [vp, vp, ip, C.c_int, vp, C.c_size_t, dp]
        L.lsfm_spmv_bench.argtypes = [vp, C.c_int, ip, ip, dp, dp, dp, C.c_int, dp, dp]
        L.lsfm_wstream_bench.argtypes = [vp, C.c_longlong, C.c_int, C.c_int, dp]
        L.lsfm_selftest_prims.argtypes = [vp, C.c_int, C.c_uint]
        L.lsfm_selftest_chol.argtypes = [vp, C.c_int, ip, ip, dp, ip, P(C.c_ubyte), ip, C.c_int, dp, C.c_int, C.c_int, dp, dp, ip, ip, ip, dp, dp, dp,
                                         C.c_int, ip]
        L.lsfm_selftest_cc_sweeps.argtypes = [vp, C.c_int, ip, ip, dp, ip, P(C.c_ubyte), dp, C.c_int, dp, dp, dp, ip, dp, dp, ip]
        L.lsfm_selftest_transform.argtypes = [vp, P(LsfmMap), C.c_int, C.c_int, ip, ip, ip, C.c_int, P(LsfmMap)]
        L.lsfm_selftest_small.argtypes = [vp, C.c_int, ip, ip, ip, ub, dp, ip, ip, dp, ip, ip, C.c_int, dp, dp, dp, dp, ub, C.c_int, dp, dp, ip, dp]
        _LIB = L
    return _LIB


EXPORTS = ["lsfm_context_create", "lsfm_context_destroy", "lsfm_set_pcg", "lsfm_set_precision", "lsfm_set_small_solve", "lsfm_set_spmv_variant", "lsfm_set_covcols_panel", "lsfm_last_error", "lsfm_stream",
           "lsfm_map_release", "lsfm_transform_stereo", "lsfm_transform_mono", "lsfm_join_stereo", "lsfm_join_mono",
           "lsfm_solve_stereo", "lsfm_solve_mono", "lsfm_tree_upload", "lsfm_tree_run", "lsfm_tree_set_final_reanchor",
           "lsfm_tree_download", "lsfm_tree_set_stop_level", "lsfm_tree_node_count", "lsfm_tree_download_node", "lsfm_tree_download_state", "lsfm_tree_set_plans", "lsfm_tree_export_size", "lsfm_tree_export_dev", "lsfm_packed_size",
           "lsfm_tree_upload_dev", "lsfm_tree_reload_dev", "lsfm_tree_set_comm", "lsfm_tree_set_comm_blocks", "lsfm_tree_export_slice_sizes", "lsfm_tree_export_slice_dev",
           "lsfm_tree_free", "lsfm_divide_conquer", "lsfm_read_localmap", "lsfm_read_localmaps", "lsfm_write_localmap", "lsfm_write_mapset", "lsfm_mapset_info", "lsfm_mapset_stamp", "lsfm_read_mapset", "lsfm_save_state_bin", "lsfm_save_state", "lsfm_save_poses", "lsfm_gn_polish",
           "lsfm_gn_polish_robust", "lsfm_map_chi2", "lsfm_map_feature_chi2", "lsfm_gn_polish_robust_features", "lsfm_gn_linearise", "lsfm_gn_linearise_timed",
           "lsfm_gn_linearise_features", "lsfm_gn_linearise_features_timed",
           "lsfm_spmv_bench", "lsfm_wstream_bench", "lsfm_selftest_prims", "lsfm_selftest_chol", "lsfm_selftest_cc_sweeps", "lsfm_selftest_transform", "lsfm_selftest_small", "lsfm_schur_pattern", "lsfm_symbolic_analyse", "lsfm_inverse_v", "lsfm_selftest_vinv", "lsfm_solve_features",
           "lsfm_map_covariance", "lsfm_map_covariance_timed",
           "lsfm_save_covariances", "lsfm_read_covariances",
           "lsfm_map_covariance_columns", "lsfm_map_covariance_columns_timed", "lsfm_save_cov_columns", "lsfm_read_cov_columns",
           "lsfm_map_covariance_feature_columns", "lsfm_map_covariance_feature_columns_timed", "lsfm_map_feature_pair_gate", "lsfm_map_feature_pair_gate_timed", "lsfm_save_pair_gate", "lsfm_read_pair_gate",
           "lsfm_map_merge_features", "lsfm_map_merge_features_timed", "lsfm_merge_structure", "lsfm_save_merge_report", "lsfm_read_merge_report",
           "lsfm_map_feature_pair_candidates", "lsfm_map_feature_pair_candidates_timed", "lsfm_save_pair_list", "lsfm_read_pair_list",
           "lsfm_map_feature_pair_joint_gate", "lsfm_map_feature_pair_joint_gate_timed", "lsfm_selftest_pair_select", "lsfm_save_joint_gate", "lsfm_read_joint_gate",
           "lsfm_map_marginalise", "lsfm_map_marginalise_timed", "lsfm_tree_export_reduced_size", "lsfm_tree_export_reduced_dev",
           "lsfm_tree_export_reduced_dev_timed", "lsfm_map_marginalise_poses", "lsfm_map_marginalise_poses_timed", "lsfm_marg_pose_structure", "lsfm_gn_structure"]


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype).reshape(-1)


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


class HostMap:
    """A map in the reference layout whose arrays are owned by numpy; `.c` is the lsfm_map view."""

    def __init__(self, d):
        g = d if isinstance(d, dict) else d.__dict__
        self.stno = _c(g["stno"], np.int32); self.stVal = _c(g["stVal"], np.float64)
        self.U = _c(g["U"], np.float64); self.Ui = _c(g["Ui"], np.int32); self.Uj = _c(g["Uj"], np.int32)
        self.W = _c(g["W"], np.float64); self.photo = _c(g["photo"], np.int32); self.feature = _c(g["feature"], np.int32)
        self.V = _c(g["V"], np.float64); self.FBlock = _c(g["FBlock"], np.int32)
        c = LsfmMap()
        c.Ref = int(g["Ref"]); c.FRef = int(g.get("FRef", g["Ref"])); c.m = int(g["m"]); c.n = int(g["n"])
        c.nU = len(self.Ui); c.nW = len(self.photo)
        c.ScaP = int(g.get("ScaP", 0)); c.Fix = int(g.get("Fix", 0)); c.Sign = int(g.get("Sign", 1))
        c.FScaP = int(g.get("FScaP", c.ScaP)); c.FFix = int(g.get("FFix", c.Fix))
        c.stno = _ptr(self.stno, C.c_int); c.stVal = _ptr(self.stVal, C.c_double)
        c.U = _ptr(self.U, C.c_double); c.Ui = _ptr(self.Ui, C.c_int); c.Uj = _ptr(self.Uj, C.c_int)
        c.W = _ptr(self.W, C.c_double); c.photo = _ptr(self.photo, C.c_int); c.feature = _ptr(self.feature, C.c_int)
        c.V = _ptr(self.V, C.c_double); c.FBlock = _ptr(self.FBlock, C.c_int)
        if g.get("pose_origin") is not None:
            self.pose_origin = _c(g["pose_origin"], np.int32)
            c.pose_origin = _ptr(self.pose_origin, C.c_int)
        self.c = c


def _arr(ptr, n, dtype):
    if n == 0:
        return np.zeros(0, dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True)


def map_to_dict(g: LsfmMap, release=True):
    r = 6 * g.m + 3 * g.n
    d = dict(Ref=g.Ref, FRef=g.FRef, m=g.m, n=g.n, nU=g.nU, nW=g.nW, ScaP=g.ScaP, Fix=g.Fix, Sign=g.Sign,
             FScaP=g.FScaP, FFix=g.FFix,
             stno=_arr(g.stno, r, np.int32), stVal=_arr(g.stVal, r, np.float64),
             U=_arr(g.U, 36 * g.nU, np.float64).reshape(-1, 36), Ui=_arr(g.Ui, g.nU, np.int32), Uj=_arr(g.Uj, g.nU, np.int32),
             W=_arr(g.W, 18 * g.nW, np.float64).reshape(-1, 18), photo=_arr(g.photo, g.nW, np.int32),
             feature=_arr(g.feature, g.nW, np.int32), V=_arr(g.V, 9 * g.n, np.float64).reshape(-1, 9),
             FBlock=_arr(g.FBlock, g.n, np.int32))
    if g.pose_origin:
        d["pose_origin"] = _arr(g.pose_origin, g.m, np.int32)
    if release:
        lib().lsfm_map_release(C.byref(g))
    return d


def _gn_args(maps, G):
    """The arguments of the GN entry points: the local maps as lsfm_map views, the global state x (stVal a copy the call may update),
    and what must stay alive while they are used."""
    hms = [HostMap(d) for d in maps]
    arr = (LsfmMap * len(hms))(*[h.c for h in hms])
    x = LsfmMap()
    stno = _c(G["stno"], np.int32)
    st = np.array(np.asarray(G["stVal"], np.float64), copy=True)
    x.m, x.n, x.Ref, x.FRef = int(G["m"]), int(G["n"]), int(G["Ref"]), int(G.get("FRef", G["Ref"]))
    x.ScaP, x.Fix, x.Sign = int(G.get("ScaP", 0)), int(G.get("Fix", 0)), int(G.get("Sign", 1))
    x.FScaP, x.FFix = int(G.get("FScaP", x.ScaP)), int(G.get("FFix", x.Fix))
    x.stno, x.stVal = _ptr(stno, C.c_int), _ptr(st, C.c_double)
    org = None
    if G.get("pose_origin") is not None:
        org = _c(G["pose_origin"], np.int32)
        x.pose_origin = _ptr(org, C.c_int)
    return hms, arr, x, (stno, st, org)


class Context:
    """One per GPU.  Raises LsfmError when no HIP device is usable (the library has no CPU path)."""

    def __init__(self, device=0, arena_bytes=0):
        self._h = C.c_void_p()
        rc = lib().lsfm_context_create(int(device), int(arena_bytes), C.byref(self._h))
        if rc != 0:
            self._h = None
            raise LsfmError(f"lsfm_context_create failed (rc={rc}): no usable HIP device -- there is no CPU fallback")

    def close(self):
        if self._h:
            lib().lsfm_context_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            raise LsfmError(f"{what} failed (rc={rc}): {lib().lsfm_last_error(self._h).decode()}")
        return rc

    def set_pcg(self, rel_tol=1e-12, max_steps=0):
        """Stopping rule of the refinement (relative residual) and the most steps a system may take (0: the default, 50)."""
        self._check(lib().lsfm_set_pcg(self._h, float(rel_tol), int(max_steps)), "lsfm_set_pcg")

    def set_precision(self, mixed):
        """False: fp64 throughout.  True: the Cholesky preconditioner kept and applied in fp32, residual correction in fp64."""
        self._check(lib().lsfm_set_precision(self._h, 1 if mixed else 0), "lsfm_set_precision")

    def set_small_solve(self, max_poses=5):
        """Levels whose camera systems have at most `max_poses` poses are solved by the one-launch dense path (0: none; at most 16;
        default 5); the others, and everything in feature-sharded runs, by the sparse pipeline.  The tests compare the two."""
        self._check(lib().lsfm_set_small_solve(self._h, int(max_poses)), "lsfm_set_small_solve")

    def set_spmv_variant(self, variant):
        """0: by size (default); 1: always the kernel that streams the upper blocks once; 2: always the row-sorted list."""
        self._check(lib().lsfm_set_spmv_variant(self._h, int(variant)), "lsfm_set_spmv_variant")

    def set_covcols_panel(self, variant):
        """covariance_columns, a supernode group's panel product: 0 the default; 1 lane per column; 2 on the MFMA unit."""
        self._check(lib().lsfm_set_covcols_panel(self._h, int(variant)), "lsfm_set_covcols_panel")

    def stream(self):
        return lib().lsfm_stream(self._h)

    def tree_reload_dev(self, tree, dev_ptrs):
        """New values (same structure) for the resident inputs of a tree made by tree_upload_dev; plans are kept."""
        arr = (C.c_void_p * len(dev_ptrs))(*[C.c_void_p(int(p)) for p in dev_ptrs])
        self._check(lib().lsfm_tree_reload_dev(self._h, tree, arr, len(dev_ptrs)), "lsfm_tree_reload_dev")

    # ---- the reference's three scheduler-facing methods -------------------------------------------------
    def transform(self, d, mono, Ref, ScaP=0, Fix=0):
        hm = HostMap(d)
        out = LsfmMap()
        if mono:
            rc = lib().lsfm_transform_mono(self._h, C.byref(hm.c), int(Ref), int(ScaP), int(Fix), C.byref(out))
        else:
            rc = lib().lsfm_transform_stereo(self._h, C.byref(hm.c), int(Ref), C.byref(out))
        self._check(rc, "lsfm_transform")
        return map_to_dict(out)

    def join(self, dEnd, dCur, mono):
        """Returns (joint dict with solved state, eP, eF, rc)."""
        he, hc = HostMap(dEnd), HostMap(dCur)
        out = LsfmMap()
        m = he.c.m + hc.c.m - (2 if mono else 0)
        eP = np.zeros(6 * m)
        eF = np.zeros(3 * (he.c.n + hc.c.n))
        fn = lib().lsfm_join_mono if mono else lib().lsfm_join_stereo
        rc = self._check(fn(self._h, C.byref(he.c), C.byref(hc.c), C.byref(out), _ptr(eP, C.c_double), _ptr(eF, C.c_double)),
                         "lsfm_join")
        j = map_to_dict(out)
        return j, eP, eF[:3 * j["n"]], rc

    def solve(self, j, eP, eF, mono, sa=None, x0=None):
        m, n = int(j["m"]), int(j["n"])
        st = np.zeros(6 * m + 3 * n)
        U = _c(j["U"], np.float64); W = _c(j["W"], np.float64); V = _c(j["V"], np.float64)
        Ui = _c(j["Ui"], np.int32); Uj = _c(j["Uj"], np.int32); ph = _c(j["photo"], np.int32); fe = _c(j["feature"], np.int32)
        eP = _c(eP, np.float64); eF = _c(eF, np.float64)
        x0p = _ptr(_c(x0, np.float64), C.c_double) if x0 is not None else None
        d, i = C.c_double, C.c_int
        if mono:
            rc = lib().lsfm_solve_mono(self._h, _ptr(st, d), _ptr(eF, d), _ptr(eP, d), _ptr(U, d), _ptr(W, d), _ptr(V, d),
                                       _ptr(Ui, i), _ptr(Uj, i), _ptr(ph, i), _ptr(fe, i), m, n, len(Ui), len(ph),
                                       sa[0], sa[1], sa[2], sa[3], sa[4], x0p)
        else:
            rc = lib().lsfm_solve_stereo(self._h, _ptr(st, d), _ptr(eF, d), _ptr(eP, d), _ptr(U, d), _ptr(W, d), _ptr(V, d),
                                         _ptr(Ui, i), _ptr(Uj, i), _ptr(ph, i), _ptr(fe, i), m, n, len(Ui), len(ph), x0p)
        self._check(rc, "lsfm_solve")
        return st, rc

    # ---- the scheduler --------------------------------------------------------------------------------
    def tree_upload(self, maps, mono):
        hms = [HostMap(m) for m in maps]
        arr = (LsfmMap * len(hms))(*[h.c for h in hms])
        t = C.c_void_p()
        self._check(lib().lsfm_tree_upload(self._h, arr, len(hms), int(mono), C.byref(t)), "lsfm_tree_upload")
        return t

    def tree_run(self, tree):
        st = LsfmStats()
        rc = self._check(lib().lsfm_tree_run(self._h, tree, C.byref(st)), "lsfm_tree_run")
        return st.as_dict(), rc

    def tree_download(self, tree):
        out = LsfmMap()
        self._check(lib().lsfm_tree_download(self._h, tree, C.byref(out)), "lsfm_tree_download")
        return map_to_dict(out)

    # ---- level checkpoint / resume (include/lsfm.h) ------------------------------------------------------
    def tree_set_stop_level(self, tree, levels):
        """The next runs of `tree` end after `levels` tree levels (0: the whole tree)."""
        if lib().lsfm_tree_set_stop_level(tree, int(levels)):
            raise LsfmError("lsfm_tree_set_stop_level: bad argument")

    def tree_node_count(self, tree):
        return int(lib().lsfm_tree_node_count(self._h, tree))

    def tree_download_node(self, tree, k):
        """Node k of the level the last run ended at, as a map dict that tree_upload takes back (FRef, FScaP, FFix, pose_origin)."""
        out = LsfmMap()
        self._check(lib().lsfm_tree_download_node(self._h, tree, int(k), C.byref(out)), "lsfm_tree_download_node")
        return map_to_dict(out)

    def tree_download_state(self, tree):
        """(m, n, stno, stVal) of the final map: the state vector without the information blocks."""
        m, n = C.c_int(0), C.c_int(0)
        self._check(lib().lsfm_tree_download_state(self._h, tree, C.byref(m), C.byref(n), None, None, 0), "lsfm_tree_download_state")
        r = 6 * m.value + 3 * n.value
        stno = np.zeros(r, np.int32); stVal = np.zeros(r)
        self._check(lib().lsfm_tree_download_state(self._h, tree, C.byref(m), C.byref(n), _ptr(stno, C.c_int), _ptr(stVal, C.c_double), r),
                    "lsfm_tree_download_state")
        return m.value, n.value, stno, stVal

    def tree_free(self, tree):
        lib().lsfm_tree_free(self._h, tree)

    def tree_set_plans(self, tree, on):
        lib().lsfm_tree_set_plans(tree, int(on))

    def tree_set_final_reanchor(self, tree, on):
        lib().lsfm_tree_set_final_reanchor(tree, int(on))

    # ---- device-resident hand-off of a tree node (multi-GPU sub-tree sharding) ---------------------------
    def tree_export_size(self, tree):
        return int(lib().lsfm_tree_export_size(self._h, tree))

    def tree_export_dev(self, tree, dev_ptr, cap):
        """Packs the final map of a finished tree into caller-owned device memory (e.g. a torch uint8 CUDA tensor)."""
        self._check(lib().lsfm_tree_export_dev(self._h, tree, C.c_void_p(int(dev_ptr)), int(cap)), "lsfm_tree_export_dev")

    def tree_upload_dev(self, dev_ptrs, mono):
        """A new tree whose resident inputs are the packed maps at the given device addresses (no host copy)."""
        arr = (C.c_void_p * len(dev_ptrs))(*[C.c_void_p(int(p)) for p in dev_ptrs])
        t = C.c_void_p()
        self._check(lib().lsfm_tree_upload_dev(self._h, arr, len(dev_ptrs), int(mono), C.byref(t)), "lsfm_tree_upload_dev")
        return t

    def tree_export_reduced_size(self, tree, keep_ids):
        """Bytes of the reduced pack of a finished tree's final map: every feature whose label is not in keep_ids marginalised out."""
        ids = _c(keep_ids, np.int32)
        n = C.c_size_t(0)
        self._check(lib().lsfm_tree_export_reduced_size(self._h, tree, _ptr(ids, C.c_int) if len(ids) else None, len(ids), C.byref(n)),
                    "lsfm_tree_export_reduced_size")
        return int(n.value)

    def tree_export_reduced_dev(self, tree, keep_ids, dev_ptr, cap, times=False):
        """Packs the final map of a finished tree, reduced to the features in keep_ids (any order; unknown ids are ignored), into
        caller-owned device memory: the format of tree_export_dev, taken by tree_upload_dev unchanged.  The result stays intact.
        times: returns {"structure_ms", "partition_ms", "vinv_ms", "values_ms", "emit_ms"} by HIP events."""
        ids = _c(keep_ids, np.int32)
        t = np.zeros(5)
        self._check(lib().lsfm_tree_export_reduced_dev_timed(self._h, tree, _ptr(ids, C.c_int) if len(ids) else None, len(ids),
                                                             C.c_void_p(int(dev_ptr)), int(cap), _ptr(t, C.c_double) if times else None),
                    "lsfm_tree_export_reduced_dev")
        if times:
            return dict(zip(("structure_ms", "partition_ms", "vinv_ms", "values_ms", "emit_ms"), t.tolist()))

    # ---- feature-sharded joins (the top of the tree over several GPUs) -----------------------------------
    def tree_export_slice_sizes(self, tree, nslices):
        sizes = (C.c_size_t * nslices)()
        self._check(lib().lsfm_tree_export_slice_sizes(self._h, tree, int(nslices), sizes), "lsfm_tree_export_slice_sizes")
        return [int(v) for v in sizes]

    def tree_export_slice_dev(self, tree, nslices, slice_, dev_ptr, cap):
        """Pack `slice_` (features with feat_id % nslices == slice_, all poses and U blocks) of a finished tree's final map."""
        self._check(lib().lsfm_tree_export_slice_dev(self._h, tree, int(nslices), int(slice_), C.c_void_p(int(dev_ptr)), int(cap)),
                    "lsfm_tree_export_slice_dev")

    def tree_set_comm(self, tree, rank, world, fn, dev_ptr, dev_bytes):
        """fn: an ALLREDUCE_FN instance (the caller keeps it alive as long as the tree runs); None / world <= 1: off."""
        cb = fn if fn is not None else C.cast(None, ALLREDUCE_FN)
        self._check(lib().lsfm_tree_set_comm(tree, int(rank), int(world), cb, None, C.c_void_p(int(dev_ptr) if dev_ptr else None),
                                             int(dev_bytes)), "lsfm_tree_set_comm")

    def tree_set_comm_blocks(self, tree, block_maps):
        """block_maps = 2^k > 0: the pose-side factorisation of the feature-sharded tree is distributed by block ownership; 0: replicated."""
        self._check(lib().lsfm_tree_set_comm_blocks(tree, int(block_maps)), "lsfm_tree_set_comm_blocks")

    def divide_conquer(self, maps, mono, final_reanchor=True):
        t = self.tree_upload(maps, mono)
        if not final_reanchor:
            lib().lsfm_tree_set_final_reanchor(t, 0)
        try:
            stats, rc = self.tree_run(t)
            out = self.tree_download(t)
        finally:
            self.tree_free(t)
        return out, stats, rc

    def gn_polish(self, maps, mono, G, iters):
        """lsfm_gn_polish: `iters` Gauss-Newton steps of the map-joining objective over all local maps from the global state G (a map
        dict: stno, stVal, m, n, Ref; Mono: ScaP, Fix; e.g. what divide_conquer returned).  No reference counterpart (parity unpinned).
        Returns (stVal, obj[iters + 1], gnorm[iters + 1], halvings[iters], rc)."""
        hms, arr, x, keep = _gn_args(maps, G)
        st = keep[1]
        obj, gn, hv = np.zeros(iters + 1), np.zeros(iters + 1), np.zeros(max(iters, 1), np.int32)
        rc = lib().lsfm_gn_polish(self._h, arr, len(hms), int(mono), C.byref(x), int(iters), _ptr(obj, C.c_double), _ptr(gn, C.c_double), _ptr(hv, C.c_int))
        if rc < 0:
            self._check(rc, "lsfm_gn_polish")
        return st, obj, gn, hv[:iters], rc

    def map_chi2(self, maps, mono, G):
        """lsfm_map_chi2: chi^2_k = r_k^T I_k r_k of every local map at the global state G (the terms of gn_polish's objective) and
        dof_k = 6 m_k + 3 n_k.  Deterministic.  No reference counterpart.  Returns (chi2 [N], dof [N])."""
        hms, arr, x, keep = _gn_args(maps, G)
        chi2, dof = np.zeros(len(hms)), np.zeros(len(hms), np.int32)
        self._check(lib().lsfm_map_chi2(self._h, arr, len(hms), int(mono), C.byref(x), _ptr(chi2, C.c_double), _ptr(dof, C.c_int)), "lsfm_map_chi2")
        return chi2, dof

    def gn_polish_robust(self, maps, mono, G, iters, kind, c):
        """lsfm_gn_polish_robust: gn_polish with whole local maps down-weighted by an M-estimator on s_k = chi2_k / dof_k (IRLS);
        kind 0 none (= gn_polish), 1 / "huber", 2 / "cauchy"; c > 0 the threshold.  No reference counterpart.
        Returns (stVal, obj[iters + 1] (G per iterate), gnorm[iters + 1], halvings[iters], chi2 [N], weight [N], rc)."""
        kind = {"none": 0, "huber": 1, "cauchy": 2}.get(kind, kind)
        hms, arr, x, keep = _gn_args(maps, G)
        st = keep[1]
        obj, gn, hv = np.zeros(iters + 1), np.zeros(iters + 1), np.zeros(max(iters, 1), np.int32)
        chi2, w = np.zeros(len(hms)), np.zeros(len(hms))
        rc = lib().lsfm_gn_polish_robust(self._h, arr, len(hms), int(mono), C.byref(x), int(iters), int(kind), float(c), _ptr(obj, C.c_double),
                                         _ptr(gn, C.c_double), _ptr(hv, C.c_int), _ptr(chi2, C.c_double), _ptr(w, C.c_double))
        if rc < 0:
            self._check(rc, "lsfm_gn_polish_robust")
        return st, obj, gn, hv[:iters], chi2, w, rc

    def map_feature_chi2(self, maps, mono, G):
        """lsfm_map_feature_chi2: c_kf = g_f^T V_f^-1 g_f, the chi^2 (3 dof) of feature f of local map k given the map's poses, at the
        global state G, and pose_chi2_k = chi2_k - sum_f c_kf.  Deterministic.  No reference counterpart.  Returns (list of arrays, one
        per map in the map's feature order, pose_chi2 [N])."""
        hms, arr, x, keep = _gn_args(maps, G)
        ns = [int(h.c.n) for h in hms]
        fchi2, pose = np.zeros(max(sum(ns), 1)), np.zeros(len(hms))
        self._check(lib().lsfm_map_feature_chi2(self._h, arr, len(hms), int(mono), C.byref(x), _ptr(fchi2, C.c_double), _ptr(pose, C.c_double)),
                    "lsfm_map_feature_chi2")
        return np.split(fchi2[:sum(ns)], np.cumsum(ns)[:-1]), pose

    def gn_polish_robust_features(self, maps, mono, G, iters, kind, c):
        """lsfm_gn_polish_robust_features: gn_polish with single features of single local maps down-weighted by an M-estimator on
        s_kf = c_kf / 3 (IRLS on the maps I_k(w)); kind 0 none (= gn_polish), 1 / "huber", 2 / "cauchy"; c > 0.  On Monocular sets prefer
        Huber.  No reference counterpart.  Returns (stVal, obj[iters + 1] (G per iterate), gnorm[iters + 1],
        halvings[iters], fchi2, fweight (lists of arrays per map, at the returned state), rc)."""
        kind = {"none": 0, "huber": 1, "cauchy": 2}.get(kind, kind)
        hms, arr, x, keep = _gn_args(maps, G)
        st = keep[1]
        ns = [int(h.c.n) for h in hms]
        obj, gn, hv = np.zeros(iters + 1), np.zeros(iters + 1), np.zeros(max(iters, 1), np.int32)
        fchi2, fw = np.zeros(max(sum(ns), 1)), np.zeros(max(sum(ns), 1))
        rc = lib().lsfm_gn_polish_robust_features(self._h, arr, len(hms), int(mono), C.byref(x), int(iters), int(kind), float(c), _ptr(obj, C.c_double),
                                                  _ptr(gn, C.c_double), _ptr(hv, C.c_int), _ptr(fchi2, C.c_double), _ptr(fw, C.c_double))
        if rc < 0:
            self._check(rc, "lsfm_gn_polish_robust_features")
        cut = np.cumsum(ns)[:-1]
        return st, obj, gn, hv[:iters], np.split(fchi2[:sum(ns)], cut), np.split(fw[:sum(ns)], cut), rc

    def gn_linearise(self, maps, mono, G, weight=None, want_b=False, timed=False, feature_weight=None):
        """lsfm_gn_linearise: the joint map of the local maps linearised at the global state G (as gn_polish takes it; read only) --
        H = sum_k w_k J_k^T I_k J_k as U / W / V with every block once, the matrix a step of gn_polish[_robust] solves with at G.
        weight [N] or None (all 1): e.g. what gn_polish_robust returned.  No reference counterpart.  Returns (map dict of the form
        tree_download returns, F = sum_k w_k chi2_k, b = sum_k w_k J_k^T I_k r_k or None); timed: also ({"assembly_ms",
        "coalesce_w_ms", "coalesce_u_ms"} by HIP events, {"NWJ", "nW", "NUJ", "nU"}: blocks of the working form / of the map).
        feature_weight (None: the call above): lsfm_gn_linearise_features -- weights w_kf in [0, 1] of the features' conditional terms, a
        list of per-map arrays as gn_polish_robust_features returns them or one flat array [sum n_k]; the maps are then I_k(w_k.), H
        the matrix of a feature-robust step at those weights, F = sum_k w_k (pose_chi2_k + sum_f w_kf c_kf), U also holds the blocks of
        poses that see a common feature, and timed gains "chi2_fill_ms" (the chi^2 pass + the correction of U) ahead of the others."""
        hms, arr, x, keep = _gn_args(maps, G)
        w = _c(weight, np.float64) if weight is not None else None
        if w is not None and len(w) != len(hms):
            raise LsfmError(f"gn_linearise: {len(w)} weights for {len(hms)} maps")
        fw = None
        if feature_weight is not None:
            ns = [int(h.c.n) for h in hms]
            if isinstance(feature_weight, (list, tuple)) and len(feature_weight) and np.ndim(feature_weight[0]) > 0:
                if len(feature_weight) != len(hms) or any(np.size(a) != n for a, n in zip(feature_weight, ns)):
                    raise LsfmError(f"gn_linearise: feature weights of sizes {[int(np.size(a)) for a in feature_weight]} for maps of {ns} features")
                fw = _c(np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in feature_weight]), np.float64)
            else:
                fw = _c(feature_weight, np.float64)
                if len(fw) != sum(ns):
                    raise LsfmError(f"gn_linearise: {len(fw)} feature weights for {sum(ns)} feature instances")
            if len(fw) == 0:
                fw = np.zeros(1)  # (no feature at all: the pointer must still be one)
        out = LsfmMap()
        F = C.c_double(0.0)
        b = np.zeros(6 * x.m + 3 * x.n) if want_b else None
        names = ("assembly_ms", "coalesce_w_ms", "coalesce_u_ms")
        if fw is not None:
            names = ("chi2_fill_ms",) + names
        t, cnt = np.zeros(len(names)), np.zeros(4, np.int32)
        head = (self._h, arr, len(hms), int(mono), C.byref(x), _ptr(w, C.c_double) if w is not None else None)
        tail = (C.byref(out), C.byref(F), _ptr(b, C.c_double) if want_b else None, _ptr(t, C.c_double) if timed else None, _ptr(cnt, C.c_int) if timed else None)
        if fw is None:
            self._check(lib().lsfm_gn_linearise_timed(*head, *tail), "lsfm_gn_linearise")
        else:
            self._check(lib().lsfm_gn_linearise_features_timed(*head, _ptr(fw, C.c_double), *tail), "lsfm_gn_linearise_features")
        d = map_to_dict(out)
        if timed:
            return d, F.value, b, dict(zip(names, t.tolist())), dict(zip(("NWJ", "nW", "NUJ", "nU"), cnt.tolist()))
        return d, F.value, b

    def inverse_v(self, V):
        """lsfm_inverse_v (the reference's pba_inverseV, Imp.cpp:3022): V^-1 of the 3x3 feature blocks, [n, 9]."""
        IV = np.array(np.asarray(V, np.float64).reshape(-1), copy=True)
        n = IV.size // 9
        self._check(lib().lsfm_inverse_v(self._h, _ptr(IV, C.c_double), 0, n), "lsfm_inverse_v")
        return IV.reshape(n, 9)

    def selftest_vinv(self, V, eb, skip=0):
        """lsfm_selftest_vinv: K7 (k_vinv) alone on V [n, 9], eb [n, 3]; skip = 1 puts the device arrays 8 bytes off a 16-byte
        boundary.  Returns (IV [n, 9], LY [n, 9]: the factor of V^-1 and L^T eb, as the Schur kernels read them)."""
        V = _c(np.asarray(V, np.float64).reshape(-1), np.float64); eb = _c(np.asarray(eb, np.float64).reshape(-1), np.float64)
        n = V.size // 9
        if V.size != 9 * n or eb.size != 3 * n:
            raise LsfmError("selftest_vinv: V [n, 9] and eb [n, 3]")
        IV = np.zeros(9 * n); LY = np.zeros(9 * n)
        self._check(lib().lsfm_selftest_vinv(self._h, _ptr(V, C.c_double), _ptr(eb, C.c_double), n, int(skip), _ptr(IV, C.c_double), _ptr(LY, C.c_double)),
                    "lsfm_selftest_vinv")
        return IV.reshape(n, 9), LY.reshape(n, 9)

    def solve_features(self, j, IV, eb, dpa):
        """lsfm_solve_features (the reference's pba_solveFeatures, Imp.cpp:2980): the features' back-substitution for the given pose
        values dpa[6m] on the system of joint-map dict j."""
        m, n = int(j["m"]), int(j["n"])
        W = _c(j["W"], np.float64); ph = _c(j["photo"], np.int32); fe = _c(j["feature"], np.int32)
        cnt = np.bincount(fe, minlength=n).astype(np.int32)
        IV = _c(IV, np.float64); eb = _c(eb, np.float64); dpa = _c(dpa, np.float64)
        dpb = np.zeros(3 * n)
        self._check(lib().lsfm_solve_features(self._h, _ptr(W, C.c_double), _ptr(IV, C.c_double), None, _ptr(eb, C.c_double), _ptr(dpa, C.c_double),
                                              _ptr(dpb, C.c_double), m, n, _ptr(cnt, C.c_int), _ptr(ph, C.c_int)), "lsfm_solve_features")
        return dpb

    def schur_pattern(self, j):
        """Upper block pattern (rowptr, colidx) of the camera system of a joint map dict, as the device builds it."""
        m, n = int(j["m"]), int(j["n"])
        Ui = _c(j["Ui"], np.int32); Uj = _c(j["Uj"], np.int32); ph = _c(j["photo"], np.int32); fe = _c(j["feature"], np.int32)
        cap = m * (m + 1) // 2
        rowptr = np.zeros(m + 1, np.int32)
        colidx = np.zeros(max(cap, 1), np.int32)
        nnzb = C.c_int(0)
        self._check(lib().lsfm_schur_pattern(self._h, _ptr(Ui, C.c_int), _ptr(Uj, C.c_int), _ptr(ph, C.c_int), _ptr(fe, C.c_int), m, n,
                                             len(Ui), len(ph), _ptr(rowptr, C.c_int), _ptr(colidx, C.c_int), cap, C.byref(nnzb)),
                    "lsfm_schur_pattern")
        return rowptr, colidx[:nnzb.value].copy()

    def covariance_raw(self, d, mono, pairs=False, cap_blocks=None, times=False):
        """lsfm_map_covariance(_timed) as it is: (rc, pose [m,6,6], feature [n,3,3], pair blocks [nnzb,6,6] or None, nnzb, times[4] or None).
        rc < 0 is returned, not raised (tests of the argument checks); cap_blocks: room for pair blocks (default: m (m + 1) / 2)."""
        h = HostMap(d)
        m, n = h.c.m, h.c.n
        pose = np.zeros((m, 6, 6))
        feat = np.zeros((n, 3, 3))
        cap = m * (m + 1) // 2 if cap_blocks is None else int(cap_blocks)
        pair = np.zeros((max(cap, 1), 6, 6)) if pairs else None
        nnzb = C.c_int(0)
        t = np.zeros(4) if times else None
        rc = lib().lsfm_map_covariance_timed(self._h, C.byref(h.c), int(mono), _ptr(pose, C.c_double), _ptr(feat, C.c_double),
                                             _ptr(pair, C.c_double) if pairs else None, cap if pairs else 0, C.byref(nnzb),
                                             _ptr(t, C.c_double) if times else None)
        return rc, pose, feat, (pair[:nnzb.value].copy() if pairs else None), nnzb.value, t

    def covariance(self, d, mono, pairs=False):
        """lsfm_map_covariance: marginal covariances of the map dict d's information matrix [U W; W^T V] (Mono: with the gauge of
        lsfm_solve_mono held fixed -- rows / columns of the pose Ref and scalar Fix of pose ScaP, reported as 0).  No reference
        counterpart.  Returns {"pose": (m,6,6), "feature": (n,3,3)} and, with pairs, "pairs": (rowptr, colidx, blocks) -- Sigma_pq on
        the upper block pattern of the camera system (lsfm_schur_pattern's order).  Raises LsfmError on a non-zero status (> 0: a
        pivot had to be floored, the result would not be the inverse)."""
        rowptr = colidx = None
        cap = 0
        if pairs:
            rowptr, colidx = self.schur_pattern(d)
            cap = len(colidx)
        rc, pose, feat, blocks, _, _ = self.covariance_raw(d, mono, pairs=pairs, cap_blocks=cap)
        self._check(rc, "lsfm_map_covariance")
        if rc != 0:
            raise LsfmError(f"lsfm_map_covariance: {rc} pivot(s) floored -- the information matrix is too close to singular")
        out = {"pose": pose, "feature": feat}
        if pairs:
            out["pairs"] = (rowptr, colidx, blocks)
        return out

    def covariance_columns_raw(self, d, mono, poses, features=False, joint=False, times=False):
        """lsfm_map_covariance_columns(_timed) as it is: (rc, pose [k,m,6,6], feature [k,n,3,6] or None, joint [6k,6k] or None, steps,
        last_corr [k], times[4] or None).  rc is returned, not raised (tests of the argument checks and statuses)."""
        h = HostMap(d)
        m, n = h.c.m, h.c.n
        q = _c(poses, np.int32)
        k = len(q)
        pose = np.zeros((k, m, 6, 6))
        feat = np.zeros((k, n, 3, 6)) if features else None
        jt = np.zeros((6 * k, 6 * k)) if joint else None
        steps = C.c_int(0)
        corr = np.zeros(max(k, 1))
        t = np.zeros(4) if times else None
        rc = lib().lsfm_map_covariance_columns_timed(self._h, C.byref(h.c), int(mono), _ptr(q, C.c_int) if k else None, k, _ptr(pose, C.c_double),
                                                     _ptr(feat, C.c_double) if features else None, _ptr(jt, C.c_double) if joint else None,
                                                     C.byref(steps), _ptr(corr, C.c_double), _ptr(t, C.c_double) if times else None)
        return rc, pose, feat, jt, steps.value, corr[:k], t

    def covariance_columns(self, d, mono, poses, features=False, joint=False):
        """lsfm_map_covariance_columns: the whole columns of Sigma = I^-1 of map dict d for the poses `poses` (indices into d's pose
        order, distinct) -- every block Sigma_{p,q}, on and off the camera system's pattern, solved side by side against one factor
        and refined in fp64 (Mono: the gauge of covariance()).  No reference counterpart.  Returns {"pose": (k,m,6,6) with [a, p] =
        Sigma_{p, poses[a]}, "feature": (k,n,3,6) or None, "joint": (6k,6k) exactly symmetric or None, "steps", "last_corr": (k,),
        "converged"}.  Raises LsfmError on an error or floored pivots; a refinement that ran out of steps is reported by "converged" (an extra key).
        The status 1 means both "not converged" and "one pivot floored": the two are told apart by steps (0: floored, nothing written)."""
        rc, pose, feat, jt, steps, corr, _ = self.covariance_columns_raw(d, mono, poses, features=features, joint=joint)
        self._check(rc, "lsfm_map_covariance_columns")
        if rc > 0 and steps == 0:
            raise LsfmError(f"lsfm_map_covariance_columns: {rc} pivot(s) floored -- the information matrix is too close to singular")
        return {"pose": pose, "feature": feat, "joint": jt, "steps": steps, "last_corr": corr, "converged": rc == 0}

    def covariance_feature_columns_raw(self, d, mono, feats, poses=True, features=False, joint=False, times=False):
        """lsfm_map_covariance_feature_columns(_timed) as it is: (rc, pose [k,m,6,3] or None, feature [k,n,3,3] or None, joint [3k,3k] or
        None, steps, last_corr [k], times[4] or None).  rc is returned, not raised (tests of the argument checks and statuses)."""
        h = HostMap(d)
        m, n = h.c.m, h.c.n
        q = _c(feats, np.int32)
        k = len(q)
        pose = np.zeros((k, m, 6, 3)) if poses else None
        feat = np.zeros((k, n, 3, 3)) if features else None
        jt = np.zeros((3 * k, 3 * k)) if joint else None
        steps = C.c_int(0)
        corr = np.zeros(max(k, 1))
        t = np.zeros(4) if times else None
        rc = lib().lsfm_map_covariance_feature_columns_timed(self._h, C.byref(h.c), int(mono), _ptr(q, C.c_int) if k else None, k,
                                                             _ptr(pose, C.c_double) if poses else None, _ptr(feat, C.c_double) if features else None,
                                                             _ptr(jt, C.c_double) if joint else None, C.byref(steps), _ptr(corr, C.c_double),
                                                             _ptr(t, C.c_double) if times else None)
        return rc, pose, feat, jt, steps.value, corr[:k], t

    def covariance_feature_columns(self, d, mono, feats, poses=True, features=False, joint=False):
        """lsfm_map_covariance_feature_columns: the whole columns of Sigma = I^-1 of map dict d for the features `feats` (indices into
        d's feature order, distinct), three columns per feature through covariance_columns' sweeps and refinement.  No reference
        counterpart.  Returns {"pose": (k,m,6,3) with [a, p] = Sigma_{p, feats[a]} or None, "feature": (k,n,3,3) with [a, g] =
        Sigma_{g, feats[a]} or None, "joint": (3k,3k) exactly symmetric or None, "steps", "last_corr": (k,), "converged"}.  Errors and
        statuses as covariance_columns."""
        rc, pose, feat, jt, steps, corr, _ = self.covariance_feature_columns_raw(d, mono, feats, poses=poses, features=features, joint=joint)
        self._check(rc, "lsfm_map_covariance_feature_columns")
        if rc > 0 and steps == 0:
            raise LsfmError(f"lsfm_map_covariance_feature_columns: {rc} pivot(s) floored -- the information matrix is too close to singular")
        return {"pose": pose, "feature": feat, "joint": jt, "steps": steps, "last_corr": corr, "converged": rc == 0}

    def feature_pair_gate_raw(self, d, mono, pairs, d2=True, cov=True, times=False):
        """lsfm_map_feature_pair_gate(_timed) as it is: (rc, d2 [K] or None, cov_diff [K,3,3] or None, steps, last_corr [K], times[4] or
        None) for pairs [K, 2] of feature indices.  rc is returned, not raised."""
        h = HostMap(d)
        pr = _c(pairs, np.int32)
        K = len(pr) // 2
        dd = np.zeros(max(K, 1)) if d2 else None
        cv = np.zeros((max(K, 1), 3, 3)) if cov else None
        steps = C.c_int(0)
        corr = np.zeros(max(K, 1))
        t = np.zeros(4) if times else None
        rc = lib().lsfm_map_feature_pair_gate_timed(self._h, C.byref(h.c), int(mono), _ptr(pr, C.c_int) if K else None, K,
                                                    _ptr(dd, C.c_double) if d2 else None, _ptr(cv, C.c_double) if cov else None, C.byref(steps),
                                                    _ptr(corr, C.c_double), _ptr(t, C.c_double) if times else None)
        return rc, (dd[:K] if d2 else None), (cv[:K] if cov else None), steps.value, corr[:K], t

    def feature_pair_gate(self, d, mono, pairs):
        """lsfm_map_feature_pair_gate: for every pair (f, g) of pairs [K, 2] (indices into map dict d's feature order, f != g) the exact
        Sigma_d = Var(x_f - x_g) of Sigma = I^-1, cross-covariance included, and d^2 = (x_f - x_g)^T Sigma_d^-1 (x_f - x_g) at d's
        estimates -- the gate of "are f and g the same point".  Three columns per pair, no cancelling sum of marginals.  No reference
        counterpart.  Returns {"d2": (K,) (NaN where Sigma_d is not positive definite), "cov_diff": (K,3,3), "steps", "last_corr": (K,),
        "converged"}.  Errors and statuses as covariance_columns."""
        rc, dd, cv, steps, corr, _ = self.feature_pair_gate_raw(d, mono, pairs)
        self._check(rc, "lsfm_map_feature_pair_gate")
        if rc > 0 and steps == 0:
            raise LsfmError(f"lsfm_map_feature_pair_gate: {rc} pivot(s) floored -- the information matrix is too close to singular")
        return {"d2": dd, "cov_diff": cv, "steps": steps, "last_corr": corr, "converged": rc == 0}

    def merge_features_raw(self, d, mono, pairs, times=False):
        """lsfm_map_merge_features(_timed) as it is: (rc, map dict or None, d2, dof, rep [n], steps, last_corr, times[5] or None) for pairs
        [K, 2] of feature indices.  rc is returned, not raised; the map is None where the call wrote none."""
        h = HostMap(d)
        pr = _c(pairs, np.int32)
        K = len(pr) // 2
        out = LsfmMap()
        d2, corr = C.c_double(0.0), C.c_double(0.0)
        dof, steps = C.c_int(0), C.c_int(0)
        rep = np.zeros(max(h.c.n, 1), np.int32)
        t = np.zeros(5) if times else None
        rc = lib().lsfm_map_merge_features_timed(self._h, C.byref(h.c), int(mono), _ptr(pr, C.c_int) if K else None, K, C.byref(out), C.byref(d2),
                                                 C.byref(dof), _ptr(rep, C.c_int), C.byref(steps), C.byref(corr), _ptr(t, C.c_double) if times else None)
        g = map_to_dict(out) if bool(out.stno) else None
        return rc, g, d2.value, dof.value, rep[:h.c.n], steps.value, corr.value, t

    def merge_features(self, d, mono, pairs):
        """lsfm_map_merge_features: map dict d with x_f = x_g declared for every pair (f, g) of pairs [K, 2] (indices into d's feature
        order) -- the exact constrained Gaussian, again a map (U unchanged, V' and W' the classes' sums, the state re-estimated through the
        merged map's camera system) -- and the joint compatibility D^2 of all pairs with dof = 3 (features removed).  No reference
        counterpart.  Returns dict(map, d2, dof, rep [n] (output feature of every input feature), steps, last_corr, converged).  Errors
        and statuses as covariance_columns."""
        rc, g, d2, dof, rep, steps, corr, _ = self.merge_features_raw(d, mono, pairs)
        self._check(rc, "lsfm_map_merge_features")
        if rc > 0 and steps == 0:
            raise LsfmError(f"lsfm_map_merge_features: {rc} pivot(s) floored -- the merged information matrix is too close to singular")
        return dict(map=g, d2=d2, dof=dof, rep=rep, steps=steps, last_corr=corr, converged=rc == 0)

    def feature_pair_candidates_raw(self, d, radius, feat_cov=None, tau=None, cap=None, dist2=True, q=None, times=False):
        """lsfm_map_feature_pair_candidates(_timed) as it is: (rc, count, pairs [min(count, cap), 2] or None, dist2 or None, q or None,
        times[4] or None, info[4] or None).  cap None: the sizing call (pairs NULL, cap 0).  q None: asked for exactly when feat_cov is
        given.  rc is returned, not raised; the arrays come back whole up to cap where the call refused, so a test sees what was
        written."""
        h = HostMap(d)
        fc = None
        if feat_cov is not None:
            fc = _c(feat_cov, np.float64)
            if len(fc) != 9 * h.c.n:
                raise LsfmError(f"feature_pair_candidates: {len(fc)} covariance entries for {h.c.n} features")
        if q is None:
            q = fc is not None
        sizing = cap is None
        cap = 0 if sizing else int(cap)
        pr = None if sizing else np.full((max(cap, 1), 2), -1, np.int32)
        dd = np.full(max(cap, 1), -1.0) if (dist2 and not sizing) else None
        qq = np.full(max(cap, 1), -1.0) if (q and not sizing) else None
        cnt = C.c_longlong(0)
        t = np.zeros(4) if times else None
        inf = np.zeros(4, np.int64) if times else None
        rc = lib().lsfm_map_feature_pair_candidates_timed(self._h, C.byref(h.c), _ptr(fc, C.c_double) if fc is not None else None, float(radius),
                                                          float(tau) if tau is not None else 0.0, _ptr(pr, C.c_int) if pr is not None else None,
                                                          _ptr(dd, C.c_double) if dd is not None else None, _ptr(qq, C.c_double) if qq is not None else None,
                                                          cap, C.byref(cnt), _ptr(t, C.c_double) if times else None,
                                                          _ptr(inf, C.c_longlong) if times else None)
        k = min(cnt.value, cap) if rc == 0 else cap
        return (rc, cnt.value, pr[:k] if pr is not None else None, dd[:k] if dd is not None else None, qq[:k] if qq is not None else None, t, inf)

    def feature_pair_candidates(self, d, radius, feat_cov=None, tau=None):
        """lsfm_map_feature_pair_candidates: every pair f < g of map dict d's features (indices into its feature order) that lie within
        `radius` of each other and, with feat_cov [n, 3, 3] (covariance(d, mono)["feature"]) and tau, whose bound q = 1/2 d^T (Sigma_ff +
        Sigma_gg)^-1 d is <= tau.  q never exceeds the gate's d^2, so no pair feature_pair_gate would accept at tau is lost; a pair whose
        sum of blocks is not positive definite is kept with q = NaN.  Sizes, then fills: two calls.  No reference counterpart.  Returns
        dict(pairs [K, 2] int32 sorted by (f, g), dist2 [K], q [K] or None)."""
        if (feat_cov is None) != (tau is None):
            raise LsfmError("feature_pair_candidates: feat_cov and tau go together")
        rc, count, _, _, _, _, _ = self.feature_pair_candidates_raw(d, radius, feat_cov, tau)
        self._check(rc, "lsfm_map_feature_pair_candidates")
        rc, count, pr, dd, qq, _, _ = self.feature_pair_candidates_raw(d, radius, feat_cov, tau, cap=count)
        self._check(rc, "lsfm_map_feature_pair_candidates")
        return dict(pairs=pr[:count], dist2=dd[:count], q=qq[:count] if qq is not None else None)

    def feature_pair_joint_gate_raw(self, d, mono, pairs, tau=None, order=None, want_C=False, times=False):
        """lsfm_map_feature_pair_joint_gate(_timed) as it is: (rc, dict(status [K], delta [K], d2 [K], C [3K,3K] or None, accepted, implied,
        D2, steps, last_corr [K]), times[6] or None) for pairs [K, 2] of feature indices.  rc is returned, not raised."""
        h = HostMap(d)
        pr = _c(pairs, np.int32)
        K = len(pr) // 2
        k1 = max(K, 1)
        od = _c(order, np.int32) if order is not None else None
        if od is not None and len(od) != K:
            raise LsfmError(f"feature_pair_joint_gate: an order of {len(od)} entries for {K} pairs")
        st, dl, dd, corr = np.zeros(k1, np.int32), np.zeros(k1), np.zeros(k1), np.zeros(k1)
        Cm = np.zeros((3 * K, 3 * K)) if (want_C and 1 <= K <= JOINT_GATE_MAX) else None
        acc, imp, steps, D2 = C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0.0)
        t = np.zeros(6) if times else None
        rc = lib().lsfm_map_feature_pair_joint_gate_timed(self._h, C.byref(h.c), int(mono), _ptr(pr, C.c_int) if K else None, K,
                                                          _ptr(od, C.c_int) if od is not None and K else None, float(JOINT_GATE_TAU if tau is None else tau),
                                                          _ptr(st, C.c_int), _ptr(dl, C.c_double), _ptr(dd, C.c_double),
                                                          _ptr(Cm, C.c_double) if Cm is not None else None, C.byref(acc), C.byref(imp), C.byref(D2),
                                                          C.byref(steps), _ptr(corr, C.c_double), _ptr(t, C.c_double) if times else None)
        return rc, dict(status=st[:K], delta=dl[:K], d2=dd[:K], C=Cm, accepted=acc.value, implied=imp.value, D2=D2.value, steps=steps.value,
                        last_corr=corr[:K]), t

    def feature_pair_joint_gate(self, d, mono, pairs, tau=None, order=None, want_C=False):
        """lsfm_map_feature_pair_joint_gate: which of the pairs [K, 2] (indices into map dict d's feature order) are compatible TOGETHER.  In
        `order` (a permutation of 0..K-1; None: ascending individual d2) a pair already connected by the accepted pairs is implied (status
        2, delta 0); otherwise delta = its d^2 conditioned on the accepted pairs, accepted (status 1) iff delta <= tau (None: chi^2_3 at
        0.99; inf accepts every independent pair), else status 0.  D2 = the sum of delta over the accepted pairs = their joint compatibility
        with 3 accepted degrees of freedom, what merge_features reports for exactly those pairs.  No reference counterpart.  Returns
        dict(status, delta, d2, C (the joint matrix A Sigma A^T, with want_C), accepted, implied, D2, dof, steps, last_corr, converged).
        Errors and statuses as feature_pair_gate."""
        rc, out, _ = self.feature_pair_joint_gate_raw(d, mono, pairs, tau, order, want_C)
        self._check(rc, "lsfm_map_feature_pair_joint_gate")
        if rc > 0 and out["steps"] == 0:
            raise LsfmError(f"lsfm_map_feature_pair_joint_gate: {rc} pivot(s) floored -- the information matrix is too close to singular")
        out["dof"] = 3 * out["accepted"]
        out["converged"] = rc == 0
        return out

    def selftest_pair_select(self, Cm, d, ends, tau, order=None, raw=False):
        """lsfm_selftest_pair_select: the selection of feature_pair_joint_gate alone on the caller's symmetric matrix Cm [3K, 3K], d [3K]
        and the pairs' endpoints ends [K, 2] (any labels).  Returns dict(status, delta, D2, accepted, implied); raw: (rc, dict)."""
        en = _c(ends, np.int32)
        K = len(en) // 2
        cm, dv = _c(Cm, np.float64), _c(d, np.float64)
        if len(cm) != 9 * K * K or len(dv) != 3 * K:
            raise LsfmError(f"selftest_pair_select: {len(cm)} matrix and {len(dv)} vector entries for {K} pairs")
        od = _c(order, np.int32) if order is not None else None
        if od is not None and len(od) != K:
            raise LsfmError(f"selftest_pair_select: an order of {len(od)} entries for {K} pairs")
        st, dl = np.zeros(max(K, 1), np.int32), np.zeros(max(K, 1))
        acc, imp, D2 = C.c_int(0), C.c_int(0), C.c_double(0.0)
        rc = lib().lsfm_selftest_pair_select(self._h, K, _ptr(cm, C.c_double), _ptr(dv, C.c_double), _ptr(en, C.c_int),
                                             _ptr(od, C.c_int) if od is not None else None, float(tau), _ptr(st, C.c_int), _ptr(dl, C.c_double),
                                             C.byref(D2), C.byref(acc), C.byref(imp))
        out = dict(status=st[:K], delta=dl[:K], D2=D2.value, accepted=acc.value, implied=imp.value)
        if raw:
            return rc, out
        self._check(rc, "lsfm_selftest_pair_select")
        return out

    def marginalise(self, d, drop, times=False):
        """lsfm_map_marginalise: the map dict d with every feature f that has drop[f] != 0 marginalised out (U' = U - sum W_f V_f^-1
        W_f^T over the dropped features), in canonical form: kept features in their order with V / W / photo unchanged, one U block
        per pose pair sorted by (Ui, Uj).  No reference counterpart.  Returns a map dict of the form tree_download returns; times:
        also {"structure_ms", "values_ms", "emit_ms"} by HIP events."""
        h = HostMap(d)
        fl = np.ascontiguousarray(np.asarray(drop).astype(bool), dtype=np.uint8).reshape(-1)
        if len(fl) != h.c.n:
            raise LsfmError(f"marginalise: {len(fl)} flags for {h.c.n} features")
        out = LsfmMap()
        t = np.zeros(3)
        self._check(lib().lsfm_map_marginalise_timed(self._h, C.byref(h.c), _ptr(fl, C.c_ubyte), C.byref(out), _ptr(t, C.c_double) if times else None),
                    "lsfm_map_marginalise")
        g = map_to_dict(out)
        if times:
            return g, dict(zip(("structure_ms", "values_ms", "emit_ms"), t.tolist()))
        return g

    def marginalise_poses(self, d, mono, keep_pose, drop_feat=None, times=False, info=False):
        """lsfm_map_marginalise_poses: the map dict d with every pose p that has keep_pose[p] == 0 marginalised out (U'_KK = U1_KK - U1_KD
        U1_DD^-1 U1_DK), after the features that go with them (drop_feat None: exactly the features a dropped pose sees; flags: those and
        more), in canonical form with the kept poses renumbered in their order.  The Ref pose (Mono: and the ScaP pose) must be kept.  No
        reference counterpart.  Returns a map dict of the form tree_download returns; times: also {"stage_a_ms", "structure_ms",
        "factor_ms", "sweeps_ms", "syrk_emit_ms"} by HIP events; info: also a dict by MARG_POSES_INFO.  Raises LsfmError on an error or
        floored pivots."""
        h = HostMap(d)
        kp = np.ascontiguousarray(np.asarray(keep_pose).astype(bool), dtype=np.uint8).reshape(-1)
        if len(kp) != h.c.m:
            raise LsfmError(f"marginalise_poses: {len(kp)} flags for {h.c.m} poses")
        fl = None
        if drop_feat is not None:
            fl = np.ascontiguousarray(np.asarray(drop_feat).astype(bool), dtype=np.uint8).reshape(-1)
            if len(fl) != h.c.n:
                raise LsfmError(f"marginalise_poses: {len(fl)} flags for {h.c.n} features")
        out = LsfmMap()
        t = np.zeros(5)
        inf = np.zeros(8, np.int32)
        rc = self._check(lib().lsfm_map_marginalise_poses_timed(self._h, C.byref(h.c), int(mono), _ptr(kp, C.c_ubyte), _ptr(fl, C.c_ubyte) if fl is not None else None,
                                                                C.byref(out), _ptr(t, C.c_double), _ptr(inf, C.c_int)), "lsfm_map_marginalise_poses")
        if rc != 0:
            raise LsfmError(f"lsfm_map_marginalise_poses: {rc} pivot(s) floored -- the dropped poses' own system is too close to singular")
        res = [map_to_dict(out)]
        if times:
            res.append(dict(zip(("stage_a_ms", "structure_ms", "factor_ms", "sweeps_ms", "syrk_emit_ms"), t.tolist())))
        if info:
            res.append(dict(zip(MARG_POSES_INFO, (int(v) for v in inf))))
        return res[0] if len(res) == 1 else tuple(res)

    def spmv_bench(self, rowptr, colidx, val, x, reps=20):
        rowptr = _c(rowptr, np.int32); colidx = _c(colidx, np.int32); val = _c(val, np.float64); x = _c(x, np.float64)
        m = len(rowptr) - 1
        y = np.zeros(6 * m)
        ms, by = C.c_double(), C.c_double()
        self._check(lib().lsfm_spmv_bench(self._h, m, _ptr(rowptr, C.c_int), _ptr(colidx, C.c_int), _ptr(val, C.c_double),
                                          _ptr(x, C.c_double), _ptr(y, C.c_double), int(reps), C.byref(ms), C.byref(by)),
                    "lsfm_spmv_bench")
        return y, ms.value, by.value


def _wstream(self, nblocks, mode, reps=10):
    """ms per launch of the W access-pattern copy (lsfm_wstream_bench)."""
    ms = C.c_double()
    self._check(lib().lsfm_wstream_bench(self._h, int(nblocks), int(mode), int(reps), C.byref(ms)), "lsfm_wstream_bench")
    return ms.value


Context.wstream_bench = _wstream


def _selftest_prims(self, cases=64, seed=1):
    """The library's own fill / small-copy kernels against the host (lsfm_selftest_prims); raises LsfmError on the first mismatch."""
    self._check(lib().lsfm_selftest_prims(self._h, int(cases), int(seed)), "lsfm_selftest_prims")


Context.selftest_prims = _selftest_prims

SELFTEST_CHOL_INFO = ("blocks", "leaf_tasks", "leaf_columns", "task0_outer", "groups", "group_levels", "fused_levels", "split_levels", "max_rows_below",
                      "d_err", "floored")


def _selftest_chol(self, rowptr, colidx, val, r, origin=None, fixed=None, pose_seg=None, nseg=1, mode=0):
    """lsfm_selftest_chol: the device Cholesky factor of the symmetric positive definite block matrix (rowptr, colidx, val: upper
    block CSR, diagonal block first and full) and one unrefined application of it per right-hand side r[nrhs, 6 m], in order.
    mode bit 0: the first right-hand side's forward substitution rides on the factorisation; bit 1: fp32 sweeps.  Returns dict(z
    [nrhs, 6 m], dot [nrhs, nseg], perm, colptr, rowidx, L [blocks, 6, 6], Dinv [m, 6, 6], dscale [6 m], info: dict by
    SELFTEST_CHOL_INFO)."""
    rowptr = _c(rowptr, np.int32); colidx = _c(colidx, np.int32); val = _c(val, np.float64)
    m = len(rowptr) - 1
    if m < 1 or len(colidx) != rowptr[-1] or len(val) != 36 * len(colidx):
        raise LsfmError("selftest_chol: rowptr / colidx / val do not fit together")
    r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1, 6 * m)
    nrhs = r.shape[0]
    org = _c(origin, np.int32) if origin is not None else None
    fx = np.ascontiguousarray(np.asarray(fixed).astype(bool), dtype=np.uint8).reshape(-1) if fixed is not None else None
    seg = _c(pose_seg, np.int32) if pose_seg is not None else np.zeros(m, np.int32)
    if (org is not None and len(org) != m) or (fx is not None and len(fx) != 6 * m) or len(seg) != m:
        raise LsfmError("selftest_chol: origin / fixed / pose_seg do not fit m")
    cap = int(symbolic_analyse(rowptr, colidx, org)["info"][0])
    z = np.zeros((nrhs, 6 * m)); dot = np.zeros((nrhs, int(nseg)))
    perm = np.zeros(m, np.int32); colptr = np.zeros(m + 1, np.int32); rowidx = np.zeros(cap, np.int32)
    Lb = np.zeros((cap, 6, 6)); Dinv = np.zeros((m, 6, 6)); dscale = np.zeros(6 * m)
    info = np.zeros(16, np.int32)
    rc = lib().lsfm_selftest_chol(self._h, m, _ptr(rowptr, C.c_int), _ptr(colidx, C.c_int), _ptr(val, C.c_double),
                                  _ptr(org, C.c_int) if org is not None else None, _ptr(fx, C.c_ubyte) if fx is not None else None,
                                  _ptr(seg, C.c_int), int(nseg), _ptr(r, C.c_double), nrhs, int(mode), _ptr(z, C.c_double), _ptr(dot, C.c_double),
                                  _ptr(perm, C.c_int), _ptr(colptr, C.c_int), _ptr(rowidx, C.c_int), _ptr(Lb, C.c_double), _ptr(Dinv, C.c_double),
                                  _ptr(dscale, C.c_double), cap, _ptr(info, C.c_int))
    self._check(rc, "lsfm_selftest_chol")
    return dict(z=z, dot=dot, perm=perm, colptr=colptr, rowidx=rowidx, L=Lb, Dinv=Dinv, dscale=dscale,
                info=dict(zip(SELFTEST_CHOL_INFO, (int(v) for v in info))))


Context.selftest_chol = _selftest_chol

SELFTEST_CC_SWEEPS_INFO = ("leaf_tasks", "groups", "group_levels", "max_rows_below", "width_mask", "fwd_task_launches", "fwd_group_launches",
                           "fwd_panel_launches", "bwd_panel_launches", "panel", "d_err", "floored")


def _selftest_cc_sweeps(self, rowptr, colidx, val, B, origin=None, fixed=None, X=None):
    """lsfm_selftest_cc_sweeps: the columns calls' side-by-side sweeps, UNREFINED, against the device Cholesky factor of the block
    matrix (rowptr, colidx, val: as selftest_chol) on the right-hand sides B[6 m, R] (caller's numbering, unscaled, 1 <= R <= 192),
    with the panel version of set_covcols_panel.  X[6 m, R] (optional): y = B - S X by one launch of the residual kernel.  Returns
    dict(x [6 m, R], fwd [6 m, R] (the slab after the forward sweep: elimination order, scaled), perm, dscale, y (None without X),
    info: dict by SELFTEST_CC_SWEEPS_INFO)."""
    rowptr = _c(rowptr, np.int32); colidx = _c(colidx, np.int32); val = _c(val, np.float64)
    m = len(rowptr) - 1
    if m < 1 or len(colidx) != rowptr[-1] or len(val) != 36 * len(colidx):
        raise LsfmError("selftest_cc_sweeps: rowptr / colidx / val do not fit together")
    B = np.ascontiguousarray(B, dtype=np.float64)
    if B.ndim != 2 or B.shape[0] != 6 * m:
        raise LsfmError("selftest_cc_sweeps: B is not [6 m, R]")
    R = B.shape[1]
    org = _c(origin, np.int32) if origin is not None else None
    fx = np.ascontiguousarray(np.asarray(fixed).astype(bool), dtype=np.uint8).reshape(-1) if fixed is not None else None
    if (org is not None and len(org) != m) or (fx is not None and len(fx) != 6 * m):
        raise LsfmError("selftest_cc_sweeps: origin / fixed do not fit m")
    Xc = y = None
    if X is not None:
        Xc = np.ascontiguousarray(X, dtype=np.float64)
        if Xc.shape != B.shape:
            raise LsfmError("selftest_cc_sweeps: X is not shaped like B")
        y = np.zeros_like(B)
    x = np.zeros_like(B); fwd = np.zeros_like(B)
    perm = np.zeros(m, np.int32); dscale = np.zeros(6 * m)
    info = np.zeros(16, np.int32)
    rc = lib().lsfm_selftest_cc_sweeps(self._h, m, _ptr(rowptr, C.c_int), _ptr(colidx, C.c_int), _ptr(val, C.c_double),
                                       _ptr(org, C.c_int) if org is not None else None, _ptr(fx, C.c_ubyte) if fx is not None else None,
                                       _ptr(B, C.c_double), R, _ptr(Xc, C.c_double) if Xc is not None else None, _ptr(x, C.c_double),
                                       _ptr(fwd, C.c_double), _ptr(perm, C.c_int), _ptr(dscale, C.c_double),
                                       _ptr(y, C.c_double) if y is not None else None, _ptr(info, C.c_int))
    self._check(rc, "lsfm_selftest_cc_sweeps")
    return dict(x=x, fwd=fwd, perm=perm, dscale=dscale, y=y, info=dict(zip(SELFTEST_CC_SWEEPS_INFO, (int(v) for v in info))))


Context.selftest_cc_sweeps = _selftest_cc_sweeps


def _selftest_transform(self, dicts, mono, targets, alias=False):
    """lsfm_selftest_transform: the maps as ONE batch through the batched transform, as a tree level calls it.  targets: per map None
    or a negative number (passed through), the new reference pose's id (Stereo), or (Ref, ScaP, Fix) (Mono).  alias: the W blocks of
    passed-through maps stay in the transform's input (alias_passthrough) and are read from there.  Returns the list of result dicts."""
    hms = [HostMap(d) for d in dicts]
    N = len(hms)
    if N < 1 or len(targets) != N:
        raise LsfmError("selftest_transform: one target per map")
    t = np.zeros((3, N), np.int32)
    for b, tg in enumerate(targets):
        t[:, b] = (-1, 0, 0) if tg is None else (tuple(tg) + (0, 0))[:3] if isinstance(tg, (tuple, list)) else (int(tg), 0, 0)
    arr = (LsfmMap * N)(*[h.c for h in hms])
    out = (LsfmMap * N)()
    rc = lib().lsfm_selftest_transform(self._h, arr, N, int(bool(mono)), _ptr(t[0], C.c_int), _ptr(t[1], C.c_int), _ptr(t[2], C.c_int),
                                       int(bool(alias)), out)
    self._check(rc, "lsfm_selftest_transform")
    return [map_to_dict(out[b]) for b in range(N)]


Context.selftest_transform = _selftest_transform


def _selftest_small(self, B, strips=0, active=None, fixed=None, x0=None, prefill=None):
    """lsfm_selftest_small: the systems of B -- dict(pose_off, feat_off, u_off [G + 1]; U, Ui, Uj, W, photo, feature, V, ea, eb in the
    batch's numbering) -- through ONE launch of the dense small-system kernel, at the instance of `strips` 16-row strips (0: that of
    the largest system).  active [G], fixed [6 M], x0 [6 M]: optional.  prefill: (x_pose, x_feat) as they are before the launch
    (default: NaN, so that what the kernel did not write shows).  Returns (x_pose, x_feat, status [2], max_rel)."""
    po, fo, uo = (_c(B[k], np.int32) for k in ("pose_off", "feat_off", "u_off"))
    G = len(po) - 1
    if G < 1 or len(fo) != G + 1 or len(uo) != G + 1:
        raise LsfmError("selftest_small: pose_off / feat_off / u_off must have one entry per system and one more")
    M, NF, NU = int(po[-1]), int(fo[-1]), int(uo[-1])
    U = _c(B["U"], np.float64); Ui = _c(B["Ui"], np.int32); Uj = _c(B["Uj"], np.int32)
    W = _c(B["W"], np.float64); ph = _c(B["photo"], np.int32); fe = _c(B["feature"], np.int32); V = _c(B["V"], np.float64)
    ea = _c(B["ea"], np.float64); eb = _c(B["eb"], np.float64)
    nW = len(ph)
    if (len(U), len(Ui), len(Uj)) != (36 * NU, NU, NU) or (len(W), len(fe)) != (18 * nW, nW) or (len(V), len(ea), len(eb)) != (9 * NF, 6 * M, 3 * NF):
        raise LsfmError("selftest_small: the arrays do not fit the offsets")
    flags = lambda a, n, what: None if a is None else _fit(np.ascontiguousarray(np.asarray(a).astype(bool), dtype=np.uint8).reshape(-1), n, what)
    act, fx = flags(active, G, "active"), flags(fixed, 6 * M, "fixed")
    x0 = None if x0 is None else _fit(_c(x0, np.float64), 6 * M, "x0")
    if prefill is None:
        xp, xf = np.full(6 * M, np.nan), np.full(3 * NF, np.nan)
    else:
        xp, xf = _fit(np.array(_c(prefill[0], np.float64)), 6 * M, "prefill"), _fit(np.array(_c(prefill[1], np.float64)), 3 * NF, "prefill")
    st = np.zeros(2, np.int32)
    mr = C.c_double()
    d, i, opt = C.c_double, C.c_int, lambda a, t: None if a is None else _ptr(a, t)
    rc = lib().lsfm_selftest_small(self._h, G, _ptr(po, i), _ptr(fo, i), _ptr(uo, i), opt(act, C.c_ubyte), _ptr(U, d), _ptr(Ui, i), _ptr(Uj, i),
                                   _ptr(W, d), _ptr(ph, i), _ptr(fe, i), nW, _ptr(V, d), _ptr(ea, d), _ptr(eb, d), opt(x0, d), opt(fx, C.c_ubyte),
                                   int(strips), _ptr(xp, d), _ptr(xf, d), _ptr(st, i), C.byref(mr))
    self._check(rc, "lsfm_selftest_small")
    return xp, xf, st, mr.value


def _fit(a, n, what):
    if len(a) != n:
        raise LsfmError(f"selftest_small: {what} has {len(a)} entries, not {n}")
    return a


Context.selftest_small = _selftest_small


def symbolic_analyse(rowptr, colidx, origin=None, reps=1):
    """Host-only: ordering + symbolic block Cholesky of a camera system's upper block pattern (no device needed).
    Returns dict(perm, colptr, rowidx, info, ms)."""
    rowptr = _c(rowptr, np.int32); colidx = _c(colidx, np.int32)
    m = len(rowptr) - 1
    org = _c(origin, np.int32) if origin is not None else None
    info = np.zeros(8, np.int32)
    perm = np.zeros(m, np.int32); colptr = np.zeros(m + 1, np.int32)
    ms = C.c_double()
    lib().lsfm_symbolic_analyse(m, _ptr(rowptr, C.c_int), _ptr(colidx, C.c_int), _ptr(org, C.c_int) if org is not None else None, 1,
                                _ptr(perm, C.c_int), _ptr(colptr, C.c_int), None, 0, _ptr(info, C.c_int), None)
    rowidx = np.zeros(max(int(info[0]), 1), np.int32)
    rc = lib().lsfm_symbolic_analyse(m, _ptr(rowptr, C.c_int), _ptr(colidx, C.c_int), _ptr(org, C.c_int) if org is not None else None, int(reps),
                                     _ptr(perm, C.c_int), _ptr(colptr, C.c_int), _ptr(rowidx, C.c_int), len(rowidx), _ptr(info, C.c_int), C.byref(ms))
    if rc:
        raise LsfmError(f"lsfm_symbolic_analyse failed (rc={rc}): malformed pattern")
    return dict(perm=perm, colptr=colptr, rowidx=rowidx[:int(info[0])], info=info, ms=ms.value)


MARG_POSES_INFO = ("dropped", "boundary", "components", "blocks", "chunks", "leaf_tasks", "groups", "group_levels")


def marg_pose_structure(d, mono, keep_pose, drop_feat=None):
    """Host-only (lsfm_marg_pose_structure): what lsfm_map_marginalise_poses makes of the labels of map dict d and the flags, without
    a device.  Returns dict(drop [n] bool, comp [m] (component of a dropped pose, -1: kept), nptr / nidx (N(c) as a CSR, the input's pose
    indices), bd, Ui / Uj (the pattern of U' in the output's numbering), info [8]).  Raises LsfmError with the library's reason."""
    h = HostMap(d)
    m, n = h.c.m, h.c.n
    kp = None if keep_pose is None else np.ascontiguousarray(np.asarray(keep_pose).astype(bool), dtype=np.uint8).reshape(-1)
    fl = None if drop_feat is None else np.ascontiguousarray(np.asarray(drop_feat).astype(bool), dtype=np.uint8).reshape(-1)
    if (kp is not None and len(kp) != m) or (fl is not None and len(fl) != n):
        raise LsfmError("marg_pose_structure: the flags do not fit the map")
    info = np.zeros(8, np.int32)
    why = C.create_string_buffer(512)
    ub = C.c_ubyte
    args = (C.byref(h.c), int(mono), _ptr(kp, ub) if kp is not None else None, _ptr(fl, ub) if fl is not None else None)
    rc = lib().lsfm_marg_pose_structure(*args, None, None, None, None, 0, None, None, None, 0, _ptr(info, C.c_int), why, len(why))
    if rc:
        raise LsfmError(f"lsfm_marg_pose_structure failed (rc={rc}): {why.value.decode()}")
    drop = np.zeros(max(n, 1), np.uint8); comp = np.zeros(m, np.int32); nptr = np.zeros(m + 1, np.int32); bd = np.zeros(m, np.int32)
    nidx = np.zeros(max(int(info[4]), 1), np.int32); Ui = np.zeros(max(int(info[3]), 1), np.int32); Uj = np.zeros_like(Ui)
    rc = lib().lsfm_marg_pose_structure(*args, _ptr(drop, ub), _ptr(comp, C.c_int), _ptr(nptr, C.c_int), _ptr(nidx, C.c_int), len(nidx), _ptr(bd, C.c_int),
                                        _ptr(Ui, C.c_int), _ptr(Uj, C.c_int), len(Ui), _ptr(info, C.c_int), why, len(why))
    if rc:
        raise LsfmError(f"lsfm_marg_pose_structure failed (rc={rc}): {why.value.decode()}")
    nc = int(info[2])
    return dict(drop=drop[:n].astype(bool), comp=comp, nptr=nptr[:nc + 1].copy(), nidx=nidx[:int(info[4])].copy(), bd=bd[:int(info[1])].copy(),
                Ui=Ui[:int(info[3])].copy(), Uj=Uj[:int(info[3])].copy(), info=info)


MERGE_STRUCTURE_INFO = ("n", "nW", "classes", "removed", "summed_blocks")


def merge_structure(d, pairs):
    """Host-only (lsfm_merge_structure): what lsfm_map_merge_features makes of the index arrays of map dict d and the pairs [K, 2], without
    a device.  Returns dict(rep [n], photo / feature [nW'], FBlock [n'], sptr [nW' + 1] / sidx [nW] (the sources of every output W block),
    info (by MERGE_STRUCTURE_INFO)).  Raises LsfmError with the library's reason."""
    h = HostMap(d)
    pr = _c(pairs, np.int32)
    K = len(pr) // 2
    info = np.zeros(8, np.int32)
    why = C.create_string_buffer(512)
    p = lambda a: _ptr(a, C.c_int)
    head = (C.byref(h.c), p(pr) if K else None, K)
    rc = lib().lsfm_merge_structure(*head, None, None, None, None, None, None, 0, p(info), why, len(why))
    if rc:
        raise LsfmError(f"lsfm_merge_structure failed (rc={rc}): {why.value.decode()}")
    v = dict(zip(MERGE_STRUCTURE_INFO, (int(i) for i in info)))
    n, nW = h.c.n, h.c.nW
    cap = max(nW, 1)
    rep, photo, feature, FBlock = np.zeros(max(n, 1), np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(max(n, 1), np.int32)
    sptr, sidx = np.zeros(cap + 1, np.int32), np.zeros(cap, np.int32)
    rc = lib().lsfm_merge_structure(*head, p(rep), p(photo), p(feature), p(FBlock), p(sptr), p(sidx), cap, p(info), why, len(why))
    if rc:
        raise LsfmError(f"lsfm_merge_structure failed (rc={rc}): {why.value.decode()}")
    return dict(rep=rep[:n], photo=photo[:v["nW"]], feature=feature[:v["nW"]], FBlock=FBlock[:v["n"]], sptr=sptr[:v["nW"] + 1], sidx=sidx[:nW], info=v)


GN_STRUCTURE_INFO = ("M", "NFG", "P", "FI", "NUJ", "NWJ", "nU", "nW", "slots", "contributors")


def gn_structure(maps, mono, G, slots=False, coalesce=False):
    """Host-only (lsfm_gn_structure): the joint system that the Gauss-Newton calls build from the labels of the local map dicts `maps` and
    the global state G, without a device.  Returns dict(info (by GN_STRUCTURE_INFO), map_hubs [N, 3] (nh, Ref pose, ScaP pose), wdst, fptrJ,
    photoJ, UiJ / UjJ (the working form), photo / feature / FBlock / Ui / Uj (coalesced; empty without `coalesce`), slot_map / slot_a /
    slot_b / slot_count (the correction slots; empty without `slots`)).  Raises LsfmError with the library's reason."""
    hms, arr, x, keep = _gn_args(maps, G)
    N = len(hms)
    info = np.zeros(10, np.int32)
    why = C.create_string_buffer(512)
    head = (arr, N, 1 if mono else 0, C.byref(x), int(bool(slots)), int(bool(coalesce)), _ptr(info, C.c_int))
    rc = lib().lsfm_gn_structure(*head, None, None, None, None, 0, None, None, 0, None, None, None, 0, None, None, 0, None, None, None, None, 0, why, len(why))
    if rc:
        raise LsfmError(f"lsfm_gn_structure failed (rc={rc}): {why.value.decode()}")
    v = dict(zip(GN_STRUCTURE_INFO, (int(i) for i in info)))
    z = lambda n: np.zeros(max(n, 1), np.int32)
    hubs, wdst, fptrJ, photoJ, UiJ, UjJ = z(3 * N), z(v["FI"]), z(v["NFG"] + 1), z(v["NWJ"]), z(v["NUJ"]), z(v["NUJ"])
    photo, feature, FBlock, Ui, Uj = z(v["nW"]), z(v["nW"]), z(v["NFG"]), z(v["nU"]), z(v["nU"])
    sm, sa, sb, sc = z(v["slots"]), z(v["slots"]), z(v["slots"]), z(v["slots"])
    p = lambda a: _ptr(a, C.c_int)
    rc = lib().lsfm_gn_structure(*head, p(hubs), p(wdst), p(fptrJ), p(photoJ), len(photoJ), p(UiJ), p(UjJ), len(UiJ), p(photo), p(feature), p(FBlock),
                                 len(photo), p(Ui), p(Uj), len(Ui), p(sm), p(sa), p(sb), p(sc), len(sm), why, len(why))
    if rc:
        raise LsfmError(f"lsfm_gn_structure failed (rc={rc}): {why.value.decode()}")
    return dict(info=v, map_hubs=hubs.reshape(N, 3), wdst=wdst[:v["FI"]], fptrJ=fptrJ, photoJ=photoJ[:v["NWJ"]], UiJ=UiJ[:v["NUJ"]], UjJ=UjJ[:v["NUJ"]],
                photo=photo[:v["nW"]], feature=feature[:v["nW"]], FBlock=FBlock[:v["NFG"] if coalesce else 0], Ui=Ui[:v["nU"]], Uj=Uj[:v["nU"]],
                slot_map=sm[:v["slots"]], slot_a=sa[:v["slots"]], slot_b=sb[:v["slots"]], slot_count=sc[:v["slots"]])


LSFM_NODE_MAGIC = 1279870541  # first token of the tree-node trailer of a local-map file (lsfm_io.cpp)


def read_localmap(path, mono):
    g = LsfmMap()
    rc = lib().lsfm_read_localmap(str(path).encode(), int(mono), C.byref(g))
    if rc:
        raise LsfmError(f"lsfm_read_localmap({path}) failed (rc={rc})")
    return map_to_dict(g)


def write_localmap(path, d, mono):
    """A map dict (local map, joint map or final map with its information matrix) in the local-map text format."""
    hm = HostMap(d)
    rc = lib().lsfm_write_localmap(str(path).encode(), int(mono), C.byref(hm.c))
    if rc:
        raise LsfmError(f"lsfm_write_localmap({path}) failed (rc={rc})")


def write_mapset(path, maps, mono):
    """Binary cache of a set of maps (list of map dicts): one file, read back bit for bit by read_mapset."""
    hms = [HostMap(d) for d in maps]
    arr = (LsfmMap * len(hms))(*[h.c for h in hms])
    rc = lib().lsfm_write_mapset(str(path).encode(), arr, len(hms), int(mono))
    if rc:
        raise LsfmError(f"lsfm_write_mapset({path}) failed (rc={rc})")


def mapset_info(path):
    """(N, mono) of a binary cache; None when the file is missing or not a cache."""
    n, mono = C.c_int(0), C.c_int(0)
    if lib().lsfm_mapset_info(str(path).encode(), C.byref(n), C.byref(mono)):
        return None
    return n.value, bool(mono.value)


def read_mapset(path, mono, first=0, count=None, threads=0):
    info = mapset_info(path)
    if info is None:
        raise LsfmError(f"{path}: not a map-set cache")
    if count is None:
        count = info[0] - first
    arr = (LsfmMap * max(count, 1))()
    rc = lib().lsfm_read_mapset(str(path).encode(), int(mono), int(first), int(count), int(threads), arr)
    if rc:
        raise LsfmError(f"lsfm_read_mapset({path}) failed (rc={rc})")
    return [map_to_dict(arr[k]) for k in range(count)]


def read_localmaps(directory, count, mono, first=1, threads=0):
    """localmap_<first>.txt ... of a directory, parsed on `threads` host threads (0: one per core)."""
    arr = (LsfmMap * count)()
    bad = C.c_int(0)
    rc = lib().lsfm_read_localmaps(str(directory).encode(), int(first), int(count), int(mono), int(threads), arr, C.byref(bad))
    if rc:
        raise LsfmError(f"lsfm_read_localmaps({directory}) failed at localmap_{bad.value}.txt (rc={rc})")
    return [map_to_dict(arr[k]) for k in range(count)]


def save_covariances(pose_path, feat_path, d, pose_cov, feat_cov):
    """lsfm_save_covariances: the -cov / -covf files of map dict d (either path may be None)."""
    stno = _c(d["stno"], np.int32)
    pc = _c(pose_cov, np.float64)
    fc = _c(feat_cov if feat_cov is not None else np.zeros(0), np.float64)
    rc = lib().lsfm_save_covariances(pose_path.encode() if pose_path else None, feat_path.encode() if feat_path else None, _ptr(stno, C.c_int),
                                     int(d["m"]), int(d["n"]), _ptr(pc, C.c_double), _ptr(fc, C.c_double))
    if rc != 0:
        raise LsfmError(f"lsfm_save_covariances failed (rc={rc})")


def read_covariances(path, k, cap=None):
    """lsfm_read_covariances: a -cov (k = 6) / -covf (k = 3) file as (ids [count], blocks [count, k, k])."""
    if cap is None:
        with open(path) as f:
            cap = sum(1 for line in f if line.strip())
    ids = np.zeros(max(cap, 1), np.int32)
    cov = np.zeros((max(cap, 1), k, k))
    cnt = C.c_int(0)
    rc = lib().lsfm_read_covariances(path.encode(), int(k), _ptr(ids, C.c_int), _ptr(cov, C.c_double), int(cap), C.byref(cnt))
    if rc != 0:
        raise LsfmError(f"lsfm_read_covariances({path}) failed (rc={rc})")
    return ids[:cnt.value].copy(), cov[:cnt.value].copy()


def save_cov_columns(path, d, poses, pose_cols):
    """lsfm_save_cov_columns: the -covcols file of map dict d for pose_cols [k, m, 6, 6] as covariance_columns gives it for `poses`."""
    stno = _c(d["stno"], np.int32)
    q = _c(poses, np.int32)
    pc = _c(pose_cols, np.float64)
    rc = lib().lsfm_save_cov_columns(path.encode(), _ptr(stno, C.c_int), int(d["m"]), _ptr(q, C.c_int), len(q), _ptr(pc, C.c_double))
    if rc != 0:
        raise LsfmError(f"lsfm_save_cov_columns failed (rc={rc})")


def read_cov_columns(path, cap=None):
    """lsfm_read_cov_columns: a -covcols file as (ids_q [count], ids_p [count], blocks [count, 6, 6])."""
    if cap is None:
        with open(path) as f:
            cap = sum(1 for line in f if line.strip())
    iq = np.zeros(max(cap, 1), np.int32)
    ip_ = np.zeros(max(cap, 1), np.int32)
    blk = np.zeros((max(cap, 1), 6, 6))
    cnt = C.c_int(0)
    rc = lib().lsfm_read_cov_columns(path.encode(), _ptr(iq, C.c_int), _ptr(ip_, C.c_int), _ptr(blk, C.c_double), int(cap), C.byref(cnt))
    if rc != 0:
        raise LsfmError(f"lsfm_read_cov_columns({path}) failed (rc={rc})")
    return iq[:cnt.value].copy(), ip_[:cnt.value].copy(), blk[:cnt.value].copy()


def save_pair_gate(path, ids, d2, cov_diff):
    """lsfm_save_pair_gate: the -gateout file for the pairs' feature labels ids [K, 2], d2 [K] and cov_diff [K, 3, 3] as
    feature_pair_gate gives them."""
    i = _c(ids, np.int32)
    dd = _c(d2, np.float64)
    cv = _c(cov_diff, np.float64)
    if len(i) != 2 * len(dd) or len(cv) != 9 * len(dd):
        raise LsfmError(f"save_pair_gate: {len(i)} ids, {len(dd)} d2 and {len(cv)} covariance entries do not belong together")
    rc = lib().lsfm_save_pair_gate(path.encode(), _ptr(i, C.c_int), len(dd), _ptr(dd, C.c_double), _ptr(cv, C.c_double))
    if rc != 0:
        raise LsfmError(f"lsfm_save_pair_gate failed (rc={rc})")


def read_pair_gate(path, cap=None):
    """lsfm_read_pair_gate: a -gateout file as (ids [count, 2], d2 [count], cov_diff [count, 3, 3])."""
    if cap is None:
        with open(path) as f:
            cap = sum(1 for line in f if line.strip())
    jf = np.zeros(max(cap, 1), np.int32)
    jg = np.zeros(max(cap, 1), np.int32)
    dd = np.zeros(max(cap, 1))
    cv = np.zeros((max(cap, 1), 3, 3))
    cnt = C.c_int(0)
    rc = lib().lsfm_read_pair_gate(path.encode(), _ptr(jf, C.c_int), _ptr(jg, C.c_int), _ptr(dd, C.c_double), _ptr(cv, C.c_double), int(cap), C.byref(cnt))
    if rc != 0:
        raise LsfmError(f"lsfm_read_pair_gate({path}) failed (rc={rc})")
    k = cnt.value
    return np.stack([jf[:k], jg[:k]], axis=1), dd[:k].copy(), cv[:k].copy()


def save_pair_list(path, ids):
    """lsfm_save_pair_list: a pair list -- the input of -gate and -merge, the output of -cand -- for the feature labels ids [K, 2]."""
    i = _c(ids, np.int32)
    if len(i) % 2:
        raise LsfmError(f"save_pair_list: {len(i)} ids are not pairs")
    rc = lib().lsfm_save_pair_list(path.encode(), _ptr(i, C.c_int) if len(i) else None, len(i) // 2)
    if rc != 0:
        raise LsfmError(f"lsfm_save_pair_list failed (rc={rc})")


def read_pair_list(path, cap=None):
    """lsfm_read_pair_list: a pair list as ids [count, 2] int32; cap None: sized by a first call."""
    cnt = C.c_longlong(0)
    if cap is None:
        rc = lib().lsfm_read_pair_list(path.encode(), None, 0, C.byref(cnt))
        if rc != 0 and not (rc == -1 and cnt.value > 0):
            raise LsfmError(f"lsfm_read_pair_list({path}) failed (rc={rc})")
        cap = cnt.value
    ids = np.zeros((max(int(cap), 1), 2), np.int32)
    rc = lib().lsfm_read_pair_list(path.encode(), _ptr(ids, C.c_int), int(cap), C.byref(cnt))
    if rc != 0:
        raise LsfmError(f"lsfm_read_pair_list({path}) failed (rc={rc})")
    return ids[:cnt.value].copy()


def save_merge_report(path, ids, removed, dof, d2):
    """lsfm_save_merge_report: the -mergeout file for ids [K, 3] (the labels of each pair's two features and of the feature both became),
    the number of features removed, dof and D^2 as merge_features gives them."""
    i = _c(ids, np.int32)
    if len(i) % 3 or not len(i):
        raise LsfmError(f"save_merge_report: {len(i)} ids are not K > 0 triples")
    rc = lib().lsfm_save_merge_report(path.encode(), len(i) // 3, int(removed), int(dof), float(d2), _ptr(i, C.c_int))
    if rc != 0:
        raise LsfmError(f"lsfm_save_merge_report failed (rc={rc})")


def read_merge_report(path, cap=None):
    """lsfm_read_merge_report: a -mergeout file as dict(K, removed, dof, d2, ids [K, 3])."""
    if cap is None:
        with open(path) as f:
            cap = sum(1 for line in f if line.strip())
    ids = np.zeros((max(cap, 1), 3), np.int32)
    K, rem, dof, d2 = C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0.0)
    rc = lib().lsfm_read_merge_report(path.encode(), C.byref(K), C.byref(rem), C.byref(dof), C.byref(d2), _ptr(ids, C.c_int), int(cap))
    if rc != 0:
        raise LsfmError(f"lsfm_read_merge_report({path}) failed (rc={rc})")
    return dict(K=K.value, removed=rem.value, dof=dof.value, d2=d2.value, ids=ids[:K.value].copy())


def save_joint_gate(path, ids, status, d2, delta, D2):
    """lsfm_save_joint_gate: the -jgateout file for the pairs' feature labels ids [K, 2] and status / d2 / delta [K], D2 as
    feature_pair_joint_gate gives them (the counts of the head are taken from status)."""
    i, st = _c(ids, np.int32), _c(status, np.int32)
    dd, dl = _c(d2, np.float64), _c(delta, np.float64)
    K = len(st)
    if K < 1 or len(i) != 2 * K or len(dd) != K or len(dl) != K:
        raise LsfmError(f"save_joint_gate: {len(i)} ids, {K} statuses, {len(dd)} d2 and {len(dl)} delta do not belong together")
    rc = lib().lsfm_save_joint_gate(path.encode(), _ptr(i, C.c_int), K, _ptr(st, C.c_int), _ptr(dd, C.c_double), _ptr(dl, C.c_double),
                                    int(np.sum(st == 1)), int(np.sum(st == 2)), float(D2))
    if rc != 0:
        raise LsfmError(f"lsfm_save_joint_gate failed (rc={rc})")


def read_joint_gate(path, cap=None):
    """lsfm_read_joint_gate: a -jgateout file as dict(K, accepted, implied, dof, D2, ids [K, 2], status, d2, delta [K])."""
    if cap is None:
        with open(path) as f:
            cap = sum(1 for line in f if line.strip())
    k1 = max(cap, 1)
    ids, st, dd, dl = np.zeros((k1, 2), np.int32), np.zeros(k1, np.int32), np.zeros(k1), np.zeros(k1)
    head = np.zeros(4, np.int32)
    D2 = C.c_double(0.0)
    rc = lib().lsfm_read_joint_gate(path.encode(), _ptr(ids, C.c_int), _ptr(st, C.c_int), _ptr(dd, C.c_double), _ptr(dl, C.c_double), int(cap),
                                    _ptr(head, C.c_int), C.byref(D2))
    if rc != 0:
        raise LsfmError(f"lsfm_read_joint_gate({path}) failed (rc={rc})")
    K = int(head[0])
    return dict(K=K, accepted=int(head[1]), implied=int(head[2]), dof=int(head[3]), D2=D2.value, ids=ids[:K].copy(), status=st[:K].copy(),
                d2=dd[:K].copy(), delta=dl[:K].copy())
