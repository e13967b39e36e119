"""ctypes binding of libccvpe_hip.so (include/ccvpe.h).  No fallback: a missing library is an error."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libccvpe_hip.so")

OK = 0
VARIANT_ID = {"vigor": 0, "vigor_ori_prior": 1, "kitti": 2, "oxford": 3}


class Config(C.Structure):
    _fields_ = [("variant", C.c_int32), ("circular_padding", C.c_int32), ("ori_noise", C.c_float),
                ("device", C.c_int32), ("micro_batch", C.c_int32), ("reserved", C.c_int32 * 3)]


class Outputs(C.Structure):
    _fields_ = [("logits_flattened", C.c_void_p), ("heatmap", C.c_void_p), ("ori", C.c_void_p),
                ("matching_score", C.c_void_p * 6)]


class Pose(C.Structure):
    _fields_ = [("index", C.c_int32), ("prob", C.c_float), ("cos_v", C.c_float), ("sin_v", C.c_float),
                ("angle_deg", C.c_float)]


# every symbol include/ccvpe.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("ccvpe_last_error", C.c_char_p, []),
    ("ccvpe_version", C.c_char_p, []),
    ("ccvpe_launch_count", C.c_uint64, []),
    ("ccvpe_create", C.c_int, [C.POINTER(Config), C.POINTER(C.c_void_p)]),
    ("ccvpe_destroy", C.c_int, [C.c_void_p]),
    ("ccvpe_set_weight", C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int32]),
    ("ccvpe_skip_weight", C.c_int, [C.c_void_p, C.c_char_p]),
    ("ccvpe_finalize_weights", C.c_int, [C.c_void_p]),
    ("ccvpe_save_packed", C.c_int, [C.c_void_p, C.c_char_p]),
    ("ccvpe_load_packed", C.c_int, [C.c_void_p, C.c_char_p]),
    ("ccvpe_pack_switches", C.c_char_p, []),
    ("ccvpe_import_tuning", C.c_int, [C.c_void_p, C.c_char_p]),
    ("ccvpe_export_tuning", C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("ccvpe_tuning_generation", C.c_int, [C.c_void_p]),
    ("ccvpe_max_micro_batch", C.c_int, [C.c_int32, C.c_float, C.c_int32, C.c_int32]),
    ("ccvpe_output_channels", C.c_int, [C.c_void_p, C.c_int32]),
    ("ccvpe_workspace_bytes", C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    ("ccvpe_forward", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                C.POINTER(Outputs), C.c_void_p]),
    ("ccvpe_postprocess", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    ("ccvpe_postprocess_rows", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    ("ccvpe_postprocess_topk", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                         C.c_void_p]),
    ("ccvpe_eval_metrics", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    ("ccvpe_aerial_cache_bytes", C.c_size_t, [C.c_void_p, C.c_int32]),
    ("ccvpe_encode_aerial", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    ("ccvpe_forward_cached", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                       C.POINTER(Outputs), C.c_void_p]),
    ("ccvpe_localize", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    ("ccvpe_localize_cached", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                        C.c_void_p]),
    ("ccvpe_localize_topk", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_void_p, C.c_void_p]),
    ("ccvpe_localize_topk_cached", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_void_p, C.c_void_p]),
    ("ccvpe_forward_cached_indexed", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                               C.c_int32, C.POINTER(Outputs), C.c_void_p]),
    ("ccvpe_localize_cached_indexed", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                                C.c_int32, C.c_void_p, C.c_void_p]),
    ("ccvpe_localize_topk_cached_indexed", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                                     C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    ("ccvpe_ground_cache_bytes", C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    ("ccvpe_encode_ground", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    ("ccvpe_localize_region", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_localize_prior", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                                       C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    ("ccvpe_localize_prior_cached_indexed", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                                      C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    ("ccvpe_postprocess_prior", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_void_p]),
    ("ccvpe_localize_region_prior", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    ("ccvpe_track_update", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_track_update_cached_indexed", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                                    C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_track_update_logits", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    ("ccvpe_track_predict", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    ("ccvpe_track_predict_affine", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
    ("ccvpe_track_smooth_work_bytes", C.c_size_t, [C.c_int32]),
    ("ccvpe_track_smooth", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_track_smooth_affine_work_bytes", C.c_size_t, [C.c_int32]),
    ("ccvpe_track_smooth_affine", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_track_link_work_bytes", C.c_size_t, [C.c_int32, C.c_int32]),
    ("ccvpe_track_link", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_track_viterbi_work_bytes", C.c_size_t, [C.c_int32]),
    ("ccvpe_track_viterbi", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                      C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_track_viterbi_back", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                           C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_track_viterbi_affine", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                             C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_track_viterbi_back_affine", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                                  C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_localize_summary", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                                         C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_localize_summary_cached_indexed", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                                        C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p]),
    ("ccvpe_postprocess_summary", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_belief_summary", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    ("ccvpe_localize_heading", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                                         C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_localize_heading_cached_indexed", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                                        C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_postprocess_heading", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_heading_prior_map", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_void_p]),
    ("ccvpe_localize_heading_prior", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                                               C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_localize_heading_prior_cached_indexed", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                                              C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                                              C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                              C.c_void_p]),
    ("ccvpe_heading_predict", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_track_joint_work_bytes", C.c_size_t, [C.c_int32, C.c_int32]),
    ("ccvpe_track_joint_predict", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                            C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_track_joint_predict_affine", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                                   C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p]),
    ("ccvpe_track_joint_update_logits", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                                  C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_track_joint_smooth_work_bytes", C.c_size_t, [C.c_int32, C.c_int32]),
    ("ccvpe_track_joint_smooth", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_track_joint_viterbi_work_bytes", C.c_size_t, [C.c_int32, C.c_int32]),
    ("ccvpe_track_joint_viterbi", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                            C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_track_joint_viterbi_back", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                 C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                                 C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_belief_credible", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    ("ccvpe_postprocess_credible", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_localize_credible", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_localize_credible_cached_indexed", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                                         C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_preprocess",C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                   C.POINTER(C.c_float * 3), C.POINTER(C.c_float * 3), C.c_void_p, C.c_void_p]),
    ("ccvpe_preprocess_resize", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                          C.POINTER(C.c_float * 3), C.POINTER(C.c_float * 3), C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ccvpe_preprocess_affine", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.c_int32,
                                          C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float * 3), C.POINTER(C.c_float * 3),
                                          C.c_void_p, C.c_void_p]),
    ("ccvpe_preprocess_window_resize", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                                 C.c_int32, C.c_int32, C.POINTER(C.c_float * 3), C.POINTER(C.c_float * 3), C.c_void_p,
                                                 C.c_void_p, C.c_void_p]),
    ("ccvpe_set_debug", C.c_int, [C.c_void_p, C.c_int32]),
    ("ccvpe_set_streams", C.c_int, [C.c_void_p, C.c_int32]),
    ("ccvpe_read_tap", C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                 C.POINTER(C.c_int32 * 4)]),
    ("ccvpe_debug_dump_plan", C.c_int, [C.c_void_p, C.c_char_p]),
    ("ccvpe_profile_forward", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                        C.POINTER(Outputs), C.c_void_p]),
    ("ccvpe_profile_row", C.c_int, [C.c_void_p, C.c_int32, C.c_char_p, C.c_size_t, C.POINTER(C.c_float),
                                    C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("ccvpe_profile_row_issued", C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_double)]),
    ("ccvpe_op_num_tiles", C.c_int, []),
    ("ccvpe_op_tile_name", C.c_char_p, [C.c_int32]),
    ("ccvpe_op_conv2d", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                  C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.c_void_p]),
    ("ccvpe_op_conv2d_ex", C.c_int, [C.c_void_p, C.c_void_p]),
    ("ccvpe_op_level1", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    ("ccvpe_op_deconv_k2s2", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                       C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    ("ccvpe_op_pose_rows", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
]


IMAGENET_MEAN = (0.485, 0.456, 0.406)   # train_VIGOR.py:60
IMAGENET_STD = (0.229, 0.224, 0.225)


def preprocess(img_u8_hwc, shift=None, crop_w=None, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """uint8 [B,H,W,3] cuda tensor -> float32 NCHW [B,3,H,crop_w] (ToTensor + Normalize + roll + FoV crop)."""
    import torch
    lib = load()
    assert img_u8_hwc.is_cuda and img_u8_hwc.dtype == torch.uint8 and img_u8_hwc.dim() == 4 and img_u8_hwc.shape[3] == 3
    img = img_u8_hwc.contiguous()
    B, H, W, _ = img.shape
    crop_w = W if crop_w is None else int(crop_w)
    out = torch.empty((B, 3, H, crop_w), dtype=torch.float32, device=img.device)
    sh = None
    if shift is not None:
        sh = torch.as_tensor(shift, dtype=torch.int32, device=img.device).contiguous()
        assert sh.numel() == B
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    stream = torch.cuda.current_stream(img.device).cuda_stream
    rc = lib.ccvpe_preprocess(C.c_void_p(img.data_ptr()), B, H, W, C.c_void_p(sh.data_ptr()) if sh is not None else None,
                              crop_w, C.byref(m), C.byref(s), C.c_void_p(out.data_ptr()), C.c_void_p(stream))
    check(rc, "ccvpe_preprocess")
    return out


def preprocess_resize(img_u8_hwc, out_hw, shift=None, crop_w=None, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """uint8 [B,H,W,3] cuda tensor as decoded -> PIL-exact bilinear resize to out_hw -> float32 NCHW [B,3,OH,crop_w]
    (transforms.Resize + ToTensor + Normalize + roll + FoV crop, train_VIGOR.py:57-70, datasets.py:118, train_VIGOR.py:272-273)."""
    import torch
    lib = load()
    assert img_u8_hwc.is_cuda and img_u8_hwc.dtype == torch.uint8 and img_u8_hwc.dim() == 4 and img_u8_hwc.shape[3] == 3
    img = img_u8_hwc.contiguous()
    B, H, W, _ = img.shape
    OH, OW = int(out_hw[0]), int(out_hw[1])
    crop_w = OW if crop_w is None else int(crop_w)
    out = torch.empty((B, 3, OH, crop_w), dtype=torch.float32, device=img.device)
    scratch = torch.empty((B, H, OW, 3), dtype=torch.uint8, device=img.device) if W != OW else None
    sh = None
    if shift is not None:
        sh = torch.as_tensor(shift, dtype=torch.int32, device=img.device).contiguous()
        assert sh.numel() == B
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    stream = torch.cuda.current_stream(img.device).cuda_stream
    rc = lib.ccvpe_preprocess_resize(C.c_void_p(img.data_ptr()), B, H, W, OH, OW, C.c_void_p(sh.data_ptr()) if sh is not None else None,
                                     crop_w, C.byref(m), C.byref(s), C.c_void_p(scratch.data_ptr()) if scratch is not None else None,
                                     C.c_void_p(out.data_ptr()), C.c_void_p(stream))
    check(rc, "ccvpe_preprocess_resize")
    return out


RESAMPLE = {"nearest": 0, "bilinear": 2}   # CCVPE_RESAMPLE_* = PIL.Image.NEAREST / BILINEAR


def preprocess_affine(img_u8_hwc, matrices, filters, crop, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """uint8 [B,H,W,3] cuda tensor -> chain of PIL affine resamplings (matrices [B,n,6] float64 PIL `data` tuples, filters [n] of
    "nearest" / "bilinear" or PIL's 0 / 2) -> crop = (top, left, out_h, out_w) of the last canvas -> ToTensor + Normalize ->
    float32 NCHW [B,3,out_h,out_w] (ccvpe_preprocess_affine; KITTI datasets.py:577-598)."""
    import torch
    lib = load()
    assert img_u8_hwc.is_cuda and img_u8_hwc.dtype == torch.uint8 and img_u8_hwc.dim() == 4 and img_u8_hwc.shape[3] == 3
    img = img_u8_hwc.contiguous()
    B, H, W, _ = img.shape
    mat = torch.as_tensor(matrices, dtype=torch.float64).to(img.device).contiguous()
    n = len(filters)
    assert mat.shape == (B, n, 6), (tuple(mat.shape), B, n)
    flt = (C.c_int32 * n)(*[RESAMPLE[f] if isinstance(f, str) else int(f) for f in filters])
    top, left, out_h, out_w = (int(v) for v in crop)
    out = torch.empty((B, 3, max(out_h, 0), max(out_w, 0)), dtype=torch.float32, device=img.device)
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    stream = torch.cuda.current_stream(img.device).cuda_stream
    rc = lib.ccvpe_preprocess_affine(C.c_void_p(img.data_ptr()), B, H, W, C.c_void_p(mat.data_ptr()), flt, n, top, left, out_h, out_w,
                                     C.byref(m), C.byref(s), C.c_void_p(out.data_ptr()), C.c_void_p(stream))
    check(rc, "ccvpe_preprocess_affine")
    return out


def preprocess_window_resize(map_u8_hwc, origins, win_hw, out_hw, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """ONE uint8 map [map_h,map_w,3] cuda tensor -> per sample the win_hw window at origins[b] = (x0, y0) (zeros outside the map,
    PIL crop) -> PIL-exact bilinear resize to out_hw -> ToTensor + Normalize -> float32 NCHW [B,3,out_h,out_w]
    (ccvpe_preprocess_window_resize; Oxford datasets.py:306-321)."""
    import torch
    lib = load()
    assert map_u8_hwc.is_cuda and map_u8_hwc.dtype == torch.uint8 and map_u8_hwc.dim() == 3 and map_u8_hwc.shape[2] == 3
    mp = map_u8_hwc.contiguous()
    org = torch.as_tensor(origins, dtype=torch.int32).reshape(-1, 2).to(mp.device).contiguous()
    B = org.shape[0]
    win_h, win_w = int(win_hw[0]), int(win_hw[1])
    out_h, out_w = int(out_hw[0]), int(out_hw[1])
    out = torch.empty((B, 3, max(out_h, 0), max(out_w, 0)), dtype=torch.float32, device=mp.device)
    scratch = torch.empty((max(B * win_h * out_w * 3, 1),), dtype=torch.uint8, device=mp.device)
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    stream = torch.cuda.current_stream(mp.device).cuda_stream
    rc = lib.ccvpe_preprocess_window_resize(C.c_void_p(mp.data_ptr()), mp.shape[0], mp.shape[1], C.c_void_p(org.data_ptr()), B, win_h, win_w,
                                            out_h, out_w, C.byref(m), C.byref(s), C.c_void_p(scratch.data_ptr()), C.c_void_p(out.data_ptr()),
                                            C.c_void_p(stream))
    check(rc, "ccvpe_preprocess_window_resize")
    return out


def op_conv2d(x_nhwc, w, bias=None, stride=1, pad=0, act=0, tile=0, iters=0):
    """Kernel-level hook: x [B,H,W,Cin] cuda fp32, w [Cout,Cin,KH,KW], returns (out NHWC, mean ms or None)."""
    import torch
    lib = load()
    B, H, W, Cin = x_nhwc.shape
    Cout, _, KH, KW = w.shape
    OH = (H + 2 * pad - KH) // stride + 1
    OW = (W + 2 * pad - KW) // stride + 1
    out = torch.empty((B, OH, OW, Cout), dtype=torch.float32, device=x_nhwc.device)
    x_nhwc = x_nhwc.contiguous()
    w = w.contiguous().float()
    b = bias.contiguous().float() if bias is not None else None
    ms = C.c_float(0.0)
    stream = torch.cuda.current_stream(x_nhwc.device).cuda_stream
    rc = lib.ccvpe_op_conv2d(C.c_void_p(x_nhwc.data_ptr()), B, H, W, Cin, C.c_void_p(w.data_ptr()),
                             C.c_void_p(b.data_ptr()) if b is not None else None, Cout, KH, KW, stride, pad, act, tile,
                             C.c_void_p(out.data_ptr()), iters, C.byref(ms), C.c_void_p(stream))
    check(rc, "ccvpe_op_conv2d")
    return out, (ms.value if iters > 0 else None)


class OpConvDst(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("ld", C.c_int32), ("coff", C.c_int32)]


class OpConvDesc(C.Structure):   # ccvpe_op_conv_desc
    _fields_ = [("x", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32), ("in_ld", C.c_int32),
                ("w", C.c_void_p), ("bias", C.c_void_p),
                ("Cout", C.c_int32), ("KH", C.c_int32), ("KW", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32), ("act", C.c_int32),
                ("tile", C.c_int32), ("mode", C.c_int32),
                ("gate", C.c_void_p), ("resid", C.c_void_p), ("resid_ld", C.c_int32), ("ndst", C.c_int32), ("dst", OpConvDst * 3),
                ("iters", C.c_int32), ("ms", C.POINTER(C.c_float)),
                ("ran_tile", C.POINTER(C.c_int32)), ("ran_split", C.POINTER(C.c_int32)), ("requested_runs", C.POINTER(C.c_int32))]


def op_conv2d_ex(x_nhwc, w, bias=None, stride=1, pad=0, act=0, tile=0, gate=None, resid=None, dsts=None, deconv=False):
    """Kernel-level hook for the forms the plans launch (ccvpe_op_conv2d_ex).  x [B,H,W,in_ld] cuda fp32 with in_ld >= Cin (the
    weight's input channels; the rest of a pixel is never read); w [Cout,Cin,KH,KW], or [Cin,Cout,2,2] with deconv=True
    (ConvTranspose2d k2 s2: 2H x 2W output pixels); gate [B,Cin]; resid [B,OH,OW,resid_ld]; dsts: up to three (tensor
    [B,OH',OW',ld], coff) pairs the caller allocated - the result lands in channels [coff, coff + Cout) of each, nothing else is
    written; None: one dense output.  Returns (outs, ran_name, ran_split, requested_runs): the destination tensors, the name of the
    tile that ran, the split code the launcher recorded (1: K whole, S: slabs + reduce launch, 64 + S: self-reducing, 255: tail
    split) and whether the requested tile takes this launch (1 / 0; -1 for tile 0)."""
    import torch
    lib = load()
    x = x_nhwc.contiguous()
    B, H, W, in_ld = x.shape
    w = w.contiguous().float()
    if deconv:
        Cin, Cout, KH, KW = w.shape
        OH, OW = 2 * H, 2 * W
    else:
        Cout, Cin, KH, KW = w.shape
        OH = (H + 2 * pad - KH) // stride + 1
        OW = (W + 2 * pad - KW) // stride + 1
    if dsts is None:
        dsts = [(torch.empty((B, OH, OW, Cout), dtype=torch.float32, device=x.device), 0)]
    b = bias.contiguous().float() if bias is not None else None
    keep = [x, w, b]
    d = OpConvDesc()
    d.x = x.data_ptr(); d.B, d.H, d.W, d.Cin, d.in_ld = B, H, W, Cin, in_ld
    d.w = w.data_ptr(); d.bias = b.data_ptr() if b is not None else None
    d.Cout, d.KH, d.KW, d.stride, d.pad, d.act, d.tile, d.mode = Cout, KH, KW, (2 if deconv else stride), pad, act, tile, (1 if deconv else 0)
    if gate is not None:
        g = gate.contiguous().float()
        assert tuple(g.shape) == (B, Cin), tuple(g.shape)
        keep.append(g)
        d.gate = g.data_ptr()
    if resid is not None:
        assert resid.is_contiguous() and resid.dtype == torch.float32 and tuple(resid.shape[:3]) == (B, OH, OW)
        d.resid = resid.data_ptr(); d.resid_ld = resid.shape[3]
    assert 1 <= len(dsts) <= 3
    d.ndst = len(dsts)
    for i, (t, coff) in enumerate(dsts):
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and tuple(t.shape[:3]) == (B, OH, OW), tuple(t.shape)
        d.dst[i].ptr = t.data_ptr(); d.dst[i].ld = t.shape[3]; d.dst[i].coff = coff
    ran_tile, ran_split, runs = C.c_int32(0), C.c_int32(0), C.c_int32(-2)
    d.ran_tile, d.ran_split, d.requested_runs = C.pointer(ran_tile), C.pointer(ran_split), C.pointer(runs)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    rc = lib.ccvpe_op_conv2d_ex(C.byref(d), C.c_void_p(stream))
    check(rc, "ccvpe_op_conv2d_ex")
    return [t for t, _ in dsts], lib.ccvpe_op_tile_name(ran_tile.value).decode(), ran_split.value, runs.value


def op_level1(x_nhwc, wd, bd, wa, ba, wt, bt, score=False, tile=1, max_wg=0):
    """Kernel-level hook: the fused last decoder level on its own.  x [B,h,w,Cin] cuda fp32 in the reference's channel order (channel 0
    the score channel when `score`), wd [Cin,16,2,2], bd [16], wa [16,16,3,3], ba [16], wt [Cout,16,3,3], bt [Cout]; tile 0 = 16 x 16
    output tiles, 1 = 32 x 16 where the width allows; max_wg (>= 8) caps the grid so that workgroups loop over tiles.  Returns (out NCHW [B,Cout,2h,2w], the tile that ran)."""
    import torch
    lib = load()
    B, h, w, Cin = x_nhwc.shape
    Cout = wt.shape[0]
    x = x_nhwc.float()
    if score:   # the plan's layout: [score, 7 unused, descriptors]
        x = torch.cat([x[..., :1], x.new_zeros((B, h, w, 7)), x[..., 1:]], dim=-1)
    x = x.contiguous()
    ws = [t.detach().float().contiguous() for t in (wd, bd, wa, ba, wt, bt)]
    out = torch.empty((B, Cout, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    rc = lib.ccvpe_op_level1(C.c_void_p(x.data_ptr()), B, 2 * h, 2 * w, Cin, 1 if score else 0, *[C.c_void_p(t.data_ptr()) for t in ws],
                             Cout, tile | (max_wg << 8), C.c_void_p(out.data_ptr()), C.c_void_p(stream))
    check(rc, "ccvpe_op_level1")
    return out, rc


def op_deconv_k2s2(x_nhwc, w, bias, dst, coff=0, cw=None):
    """Kernel-level hook: deconv_k2s2_kernel on its own (ccvpe_op_deconv_k2s2).  x [B,H,W,in_ld] cuda fp32 with in_ld >= Cin, w
    [Cin,Cout,2,2], bias [Cout] or None; the result lands in channels [coff, coff + cw) of dst [B,2H,2W,ld] (cw >= Cout, default Cout:
    the channels past Cout are written as zeros), nothing else of dst is written.  Returns the taps a workgroup held (4 or 2)."""
    import torch
    lib = load()
    x = x_nhwc.contiguous()
    B, H, W, in_ld = x.shape
    w = w.detach().float().contiguous()
    Cin, Cout = w.shape[0], w.shape[1]
    b = bias.detach().float().contiguous() if bias is not None else None
    assert dst.is_cuda and dst.is_contiguous() and dst.dtype == torch.float32 and tuple(dst.shape[:3]) == (B, 2 * H, 2 * W), tuple(dst.shape)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    rc = lib.ccvpe_op_deconv_k2s2(C.c_void_p(x.data_ptr()), B, H, W, Cin, in_ld, C.c_void_p(w.data_ptr()),
                                  C.c_void_p(b.data_ptr()) if b is not None else None, Cout, C.c_void_p(dst.data_ptr()), dst.shape[3], coff,
                                  Cout if cw is None else cw, C.c_void_p(stream))
    check(rc, "ccvpe_op_deconv_k2s2")
    return rc


def op_pose_rows(handle, logits, ori):
    """Kernel-level hook: the tail of the plain pose plan (ccvpe_localize behind its decoders) on logits [B, 512*512] and ori
    [B, 2, 512, 512] (cuda fp32) the caller holds, on a model's handle.  Returns rows [B, 5]."""
    import torch
    lib = load()
    logits, ori = logits.detach().float().contiguous(), ori.detach().float().contiguous()
    B = logits.shape[0]
    rows = torch.empty((B, 5), dtype=torch.float32, device=logits.device)
    stream = torch.cuda.current_stream(logits.device).cuda_stream
    check(lib.ccvpe_op_pose_rows(handle, C.c_void_p(logits.data_ptr()), C.c_void_p(ori.data_ptr()), B, C.c_void_p(rows.data_ptr()),
                                 C.c_void_p(stream)), "ccvpe_op_pose_rows")
    return rows


_lib = None


def library_digest() -> str:
    """Digest of the library that load() binds: the in-tree sources, or the file CCVPE_LIB_PATH names."""
    override = os.environ.get("CCVPE_LIB_PATH")
    if override:
        import hashlib
        h = hashlib.sha256()
        with open(override, "rb") as fh:
            for chunk in iter(lambda: fh.read(1 << 20), b""):
                h.update(chunk)
        return h.hexdigest()
    from . import build as _build
    return _build._digest()


def load() -> C.CDLL:
    """dlopen the in-tree library and bind every entry point; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: it ships its own HIP runtime, and the library must bind to the runtime the process's device memory and streams come
    # from.  Loaded before torch, libccvpe_hip.so pulls in the system runtime and ccvpe_create then sees no device
    # (`python __graft_entry__.py smoke`: build() loads the library, smoke() imported torch afterwards).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    override = os.environ.get("CCVPE_LIB_PATH")   # diagnostics: load an alternative build of the same ABI
    if override:
        lib = C.CDLL(override)
        for name, res, args in SYMBOLS:
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib
    try:   # rebuild when the sources are newer than the library (hipcc cross-compiles in seconds)
        from . import build as _build
        if not _build.is_current():
            _build.build(verbose=False)
    except Exception as e:  # noqa: BLE001 - no hipcc here: fall through to whatever library exists
        if os.path.exists(LIB_PATH):
            import warnings
            warnings.warn(f"libccvpe_hip.so may be stale and could not be rebuilt: {e}")
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -m ccvpe_amd.build` (hipcc, gfx950). "
            "ccvpe_amd has no CPU or PyTorch fallback for the forward pass.")
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class CcvpeError(RuntimeError):
    pass


def check(rc: int, what: str) -> None:
    if rc < 0:
        msg = load().ccvpe_last_error()
        raise CcvpeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
