"""
ctypes binding of libannchor_hip.so (include/annchor_hip.h).

The product path is the HIP library; there is no CPU implementation behind this
module.  Importing works without a GPU (so that the host logic can be tested), but
creating an `Engine` fails loudly when the library or a device is missing.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ANNCHOR_HIP_LIB", os.path.join(_HERE, "libannchor_hip.so"))   # override: profiling builds

# field ids (include/annchor_hip.h)
F_D, F_A, F_SID, F_IJS, F_I_PTR, F_I_IDX, F_FEATURES, F_NCM, F_RA, F_LABELS, F_THRESH, F_PROB, F_CAND, F_NEXT, F_DAD = range(1, 16)
_FIELD_DTYPE = {
    F_D: np.float64, F_A: np.int64, F_SID: np.uint64, F_IJS: np.int64, F_I_PTR: np.int64, F_I_IDX: np.int64,
    F_FEATURES: np.float64, F_NCM: np.uint8, F_RA: np.float64, F_LABELS: np.int64, F_THRESH: np.float64,
    F_PROB: np.float64, F_CAND: np.int64, F_NEXT: np.int64, F_DAD: np.float64,
}

METRIC_LEVENSHTEIN, METRIC_EUCLIDEAN_F32, METRIC_EUCLIDEAN_F64, METRIC_WASSERSTEIN = 1, 2, 3, 4
METRIC_COSINE_F32, METRIC_COSINE_F64 = 5, 6
METRIC_DTW_F32, METRIC_DTW_F64 = 7, 8
METRIC_FRECHET_F32, METRIC_FRECHET_F64 = 9, 10
METRIC_HAUSDORFF_F32, METRIC_HAUSDORFF_F64 = 11, 12
METRIC_ERP_F32, METRIC_ERP_F64 = 13, 14
METRIC_EMD_POINTS_F32, METRIC_EMD_POINTS_F64 = 15, 16
METRIC_JACCARD_TOKENS, METRIC_JACCARD_BITS = 17, 18
METRIC_WEIGHTED_LEVENSHTEIN = 19
METRIC_MSM_F32, METRIC_MSM_F64 = 20, 21
METRIC_TWE_F32, METRIC_TWE_F64 = 22, 23
METRIC_AFFINE_GAP = 24
METRIC_EDR_F32, METRIC_EDR_F64 = 25, 26
METRIC_LCSS_F32, METRIC_LCSS_F64 = 27, 28
METRIC_OSA = 29

# annchor_radius_fetch: which list; annchor_radius_rows: (row, 64-column chunk) entries one call takes (csrc/radius.hip)
RADIUS_EVAL, RADIUS_SURE, RADIUS_KEPT = 0, 1, 2
RADIUS_CHUNK_COLS = 64
RADIUS_TABLE_MAX = 1 << 23

# every entry point declared in include/annchor_hip.h: name -> (restype, argtypes)
_vp, _i32, _i64, _dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
_SIGNATURES = {
    "annchor_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_vp)]),
    "annchor_destroy": (None, [_vp]),
    "annchor_release_parked": (ctypes.c_int, []),
    "annchor_parked_bytes": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_i64)]),
    "annchor_last_error": (ctypes.c_char_p, [_vp]),
    "annchor_create_error": (ctypes.c_char_p, []),
    "annchor_device_name": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_int]),
    "annchor_device_pci_bus_id": (ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_int]),
    "annchor_device_mem_info": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    "annchor_synchronize": (ctypes.c_int, [_vp]),
    "annchor_lev_persist_state": (ctypes.c_int, [ctypes.c_int]),
    "annchor_last_kernel_ms": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_float)]),
    "annchor_set_strings": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32]),
    "annchor_set_strings_u16": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32]),
    "annchor_set_points_f32": (ctypes.c_int, [_vp, _vp, _i64, _i32]),
    "annchor_set_points_f64": (ctypes.c_int, [_vp, _vp, _i64, _i32]),
    "annchor_set_points_cosine_f32": (ctypes.c_int, [_vp, _vp, _i64, _i32]),
    "annchor_set_points_cosine_f64": (ctypes.c_int, [_vp, _vp, _i64, _i32]),
    "annchor_set_series_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32]),
    "annchor_set_series_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32]),
    "annchor_set_series_nd_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _i32]),
    "annchor_set_series_nd_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _i32]),
    "annchor_set_edr_series_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _dbl, _i32]),
    "annchor_set_edr_series_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _dbl, _i32]),
    "annchor_set_lcss_series_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _dbl, _i32]),
    "annchor_set_lcss_series_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _dbl, _i32]),
    "annchor_set_curves_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32]),
    "annchor_set_curves_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32]),
    "annchor_set_erp_series_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _dbl]),
    "annchor_set_erp_series_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _dbl]),
    "annchor_set_msm_series_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _dbl]),
    "annchor_set_msm_series_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _dbl]),
    "annchor_set_twe_series_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _dbl, _dbl]),
    "annchor_set_twe_series_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _dbl, _dbl]),
    "annchor_set_coded_strings": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp]),
    "annchor_set_coded_strings_affine": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _dbl]),
    "annchor_set_coded_strings_osa": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _dbl]),
    "annchor_set_point_sets_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32]),
    "annchor_set_point_sets_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32]),
    "annchor_set_clouds_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32]),
    "annchor_set_clouds_f64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32]),
    "annchor_set_token_sets": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64]),
    "annchor_set_bitsets": (ctypes.c_int, [_vp, _vp, _i64, _i32]),
    "annchor_set_histograms": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "annchor_set_histograms_wide": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "annchor_set_opaque": (ctypes.c_int, [_vp, _i64]),
    "annchor_metric_pairs": (ctypes.c_int, [_vp, _vp, _i64, _vp]),
    "annchor_brute_force": (ctypes.c_int, [_vp, _i32, _vp, _vp]),
    "annchor_pick_anchors_maxmin": (ctypes.c_int, [_vp, _i32, _i64]),
    "annchor_pick_anchors_selected": (ctypes.c_int, [_vp, _vp, _i32]),
    "annchor_set_anchor_distances": (ctypes.c_int, [_vp, _vp, _i32, _vp, _i32]),
    "annchor_build_locality": (ctypes.c_int, [_vp, _i32, _i32, _i32, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    "annchor_build_query_locality": (ctypes.c_int, [_vp, _i64, _i32, _i32, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    "annchor_compute_features": (ctypes.c_int, [_vp]),
    "annchor_count_uncomputed": (ctypes.c_int, [_vp, ctypes.POINTER(_i64)]),
    "annchor_kth_uncomputed_dad": (ctypes.c_int, [_vp, _vp, _i32, _vp]),
    "annchor_bin_counts": (ctypes.c_int, [_vp, _vp, _i32, _vp]),
    "annchor_sampler_stats": (ctypes.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "annchor_select_by_rank": (ctypes.c_int, [_vp, _vp, _i32, _vp, _vp, _i64, _vp]),
    "annchor_sample_pairs": (ctypes.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "annchor_sample_pairs_device": (ctypes.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _i64]),
    "annchor_hash_sample_pairs_device": (ctypes.c_int, [_vp, _vp, _i32, _vp, _vp, ctypes.c_uint64, _vp]),
    "annchor_download_samples": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "annchor_fit_regression_device": (ctypes.c_int, [_vp, _vp, _i32, _i32, _i32]),
    "annchor_fit_errors_device": (ctypes.c_int, [_vp]),
    "annchor_model_download": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "annchor_errors_download": (ctypes.c_int, [_vp, _vp, _i64]),
    "annchor_model_download_with_errors": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, ctypes.POINTER(_i64)]),
    "annchor_sample_pairs_device_draw": (ctypes.c_int, [_vp, _vp, _i32, _vp, _vp, ctypes.c_uint32, ctypes.POINTER(_i64), ctypes.POINTER(_i32)]),
    "annchor_legacy_choice_ranks_device": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp, _vp, _i32, _vp, ctypes.POINTER(_i32)]),
    "annchor_hash_sample": (ctypes.c_int, [_vp, _vp, _i32, _vp, _vp, ctypes.c_uint64, _vp, ctypes.POINTER(_i64)]),
    "annchor_hash_sample_pairs": (ctypes.c_int, [_vp, _vp, _i32, _vp, _vp, ctypes.c_uint64, _vp, _vp, _vp, ctypes.POINTER(_i64)]),
    "annchor_legacy_prefetch": (ctypes.c_int, [ctypes.c_uint32, _i64]),
    "annchor_legacy_generate": (ctypes.c_int, [ctypes.c_uint32, _i64]),
    "annchor_legacy_generate_at_next_wait": (ctypes.c_int, [_vp, ctypes.c_uint32, _i64, _i64]),
    "annchor_legacy_choice_ranks": (ctypes.c_int, [ctypes.c_uint32, _vp, _vp, _i32, _vp, _vp]),
    "annchor_legacy_choice_begin": (ctypes.c_int, [ctypes.c_uint32, _vp, _vp, _i32, ctypes.POINTER(_vp)]),
    "annchor_legacy_choice_end": (ctypes.c_int, [_vp, _vp, _vp]),
    "annchor_ols_bins": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp]),
    "annchor_gather_features": (ctypes.c_int, [_vp, _vp, _i64, _vp]),
    "annchor_evaluate_samples": (ctypes.c_int, [_vp, _vp, _i64, _vp]),
    "annchor_set_samples": (ctypes.c_int, [_vp, _vp, _i64, _vp]),
    "annchor_predict_merge": (ctypes.c_int, [_vp, _vp, _i32, _vp, _vp, _i32, _i32, _vp]),
    "annchor_merge_host_prediction": (ctypes.c_int, [_vp, _vp, _i32, _i32]),
    "annchor_set_labels": (ctypes.c_int, [_vp, _vp]),
    "annchor_select_candidates": (ctypes.c_int, [_vp, _i32, _i32, _vp, _vp, _i32, _i64, _i32,
                                                 ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    "annchor_select_prepare": (ctypes.c_int, [_vp, _i32, _i32]),
    "annchor_mark_candidates": (ctypes.c_int, [_vp]),
    "annchor_refine_candidates": (ctypes.c_int, [_vp]),
    "annchor_park_refine": (ctypes.c_int, [_vp, _i32]),
    "annchor_set_refined": (ctypes.c_int, [_vp, _vp, _i64]),
    "annchor_update_bounds": (ctypes.c_int, [_vp]),
    "annchor_update_bounds_prepare": (ctypes.c_int, [_vp]),
    "annchor_overlap_stats": (ctypes.c_int, [_vp, _vp]),
    "annchor_neighbor_graph": (ctypes.c_int, [_vp, _i32, _vp, _vp]),
    "annchor_stream_bind": (ctypes.c_int, [_vp, _vp, _i64, _i32, _i64, _i32]),
    "annchor_stream_anchor_round": (ctypes.c_int, [_vp, _vp, _i32, _i32, ctypes.POINTER(_dbl), ctypes.POINTER(_i64)]),
    "annchor_stream_get_row": (ctypes.c_int, [_vp, _i64, _vp]),
    "annchor_stream_order": (ctypes.c_int, [_vp, _i32] + [ctypes.POINTER(_vp)] * 6 + [ctypes.POINTER(_i64), ctypes.POINTER(_i32),
                                                                                   ctypes.POINTER(_i32)]),
    "annchor_stream_knn": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _dbl, _i32, _i32, _vp,
                                          _vp, _vp, ctypes.POINTER(_i64)]),
    "annchor_stream_knn_begin": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                                                ctypes.POINTER(_vp), ctypes.POINTER(_i64)]),
    "annchor_stream_knn_join": (ctypes.c_int, [_vp, _vp, _i32, ctypes.POINTER(_vp), ctypes.POINTER(_i64)]),
    "annchor_stream_join_rev_begin": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_i64)]),
    "annchor_stream_order_begin": (ctypes.c_int, [_vp, _i32, _i32, _i32, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_i64)]),
    "annchor_stream_order_end": (ctypes.c_int, [_vp] + [ctypes.POINTER(_vp)] * 6 + [ctypes.POINTER(_i64), ctypes.POINTER(_i32),
                                                                                       ctypes.POINTER(_i32)]),
    "annchor_stream_last_counts": (ctypes.c_int, [_vp, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    "annchor_stream_last_kernel": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(_i64)]),
    "annchor_stream_last_tile_kernels": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "annchor_stream_budget": (ctypes.c_int, [_i32, _dbl, _i32, ctypes.POINTER(_i32), ctypes.POINTER(_i32), ctypes.POINTER(_i32)]),
    "annchor_stream_knn_end": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.POINTER(_i64)]),
    "annchor_stream_knn_run": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _dbl, _i32, _i32,
                                               ctypes.POINTER(_i64)]),
    "annchor_stream_knn_fetch": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "annchor_stream_query": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _dbl, _vp, _vp,
                                            ctypes.POINTER(_i64)]),
    "annchor_stream_bind_f64": (ctypes.c_int, [_vp, _vp, _i64, _i32, _i64, _vp, _vp, ctypes.POINTER(_vp)]),
    "annchor_stream_rerank64": (ctypes.c_int, [_vp, _i32, _vp, _vp]),
    "annchor_stream_query64": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _dbl, _vp, _i64, _i64,
                                              _vp, _vp, ctypes.POINTER(_i64)]),
    "annchor_stream_last_rerank64": (ctypes.c_int, [_vp, ctypes.POINTER(_i64), ctypes.POINTER(ctypes.c_int32)]),
    "annchor_stream_order_classes": (ctypes.c_int, [_vp, _vp, _i32, _vp, ctypes.POINTER(_i64), ctypes.POINTER(_i32), ctypes.POINTER(_i32)]),
    "annchor_stream_enemies": (ctypes.c_int, [_vp, _i32, _dbl, _vp, _vp, ctypes.POINTER(_i64)]),
    "annchor_stream_join_tables": (ctypes.c_int, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "annchor_stream_hip_stream": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "annchor_stream_anchor_begin": (ctypes.c_int, [_vp, _i32, _i64, _i32, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_i64)]),
    "annchor_stream_anchor_step": (ctypes.c_int, [_vp, _vp, _i32, _i32]),
    "annchor_stream_anchor_end": (ctypes.c_int, [_vp, _vp, _vp]),
    "annchor_stream_rows_begin": (ctypes.c_int, [_vp, _i32, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_i64)]),
    "annchor_stream_rows_end": (ctypes.c_int, [_vp, _i32, _vp]),
    "annchor_stream_anchor_dists_begin": (ctypes.c_int, [_vp, _i32, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_i64)]),
    "annchor_stream_lists_all": (ctypes.c_int, [_vp, _i32, _i64, ctypes.POINTER(_vp)]),
    "annchor_stream_route_begin": (ctypes.c_int, [_vp, _i32, _vp, _vp, ctypes.POINTER(_vp), _vp, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    "annchor_stream_route_recv": (ctypes.c_int, [_vp, _i64, ctypes.POINTER(_vp)]),
    "annchor_comm_unique_id": (ctypes.c_int, [_vp]),
    "annchor_comm_init": (ctypes.c_int, [_vp, _vp, _i32, _i32]),
    "annchor_comm_destroy": (ctypes.c_int, [_vp]),
    "annchor_comm_set_timeout": (ctypes.c_int, [_vp, ctypes.c_double]),
    "annchor_comm_preflight": (ctypes.c_int, [_vp, ctypes.c_double]),
    "annchor_comm_init_side": (ctypes.c_int, [_vp, _vp]),
    "annchor_comm_allgather_begin": (ctypes.c_int, [_vp, _vp, _vp, _i64]),
    "annchor_comm_side_join": (ctypes.c_int, [_vp]),
    "annchor_comm_allgather": (ctypes.c_int, [_vp, _vp, _vp, _i64]),
    "annchor_comm_alltoall_records": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i32]),
    "annchor_stream_anchor_rounds": (ctypes.c_int, [_vp, _i32]),
    "annchor_stream_route_end": (ctypes.c_int, [_vp, _i64, _i64, _vp, _vp]),
    "annchor_stream_graph_device": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_i64), ctypes.POINTER(_i32)]),
    "annchor_device_alloc": (ctypes.c_int, [_vp, _i64, ctypes.POINTER(_vp)]),
    "annchor_device_free": (ctypes.c_int, [_vp, _vp]),
    "annchor_device_copy": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i32]),
    "annchor_enemies_candidates": (ctypes.c_int, [_vp, _vp, _i32, _i32, ctypes.POINTER(_i64)]),
    "annchor_enemies_predict": (ctypes.c_int, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "annchor_enemies_first": (ctypes.c_int, [_vp, _i32, _i32, _i32, _vp, _i64, ctypes.POINTER(_i64)]),
    "annchor_enemies_set_exact": (ctypes.c_int, [_vp, _vp, _i64]),
    "annchor_enemies_graph": (ctypes.c_int, [_vp, _i32, _vp, _vp]),
    "annchor_enemies_download": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "annchor_radius_count": (ctypes.c_int, [_vp, _dbl, _dbl, _i32, _i32, _vp, _vp]),
    "annchor_radius_rows": (ctypes.c_int, [_vp, _i64, _i64, _i64, _i64, _i64, _i32, ctypes.POINTER(_i64), ctypes.POINTER(_i64),
                                           ctypes.POINTER(_i64)]),
    "annchor_radius_fetch": (ctypes.c_int, [_vp, _i32, _vp, _vp]),
    "annchor_radius_query_count": (ctypes.c_int, [_vp, _i64, _dbl, _dbl, _i32, _i32, _vp, _vp]),
    "annchor_radius_query_rows": (ctypes.c_int, [_vp, _i64, _i64, _i64, _i64, _i64, _i64, _i32, ctypes.POINTER(_i64), ctypes.POINTER(_i64),
                                                 ctypes.POINTER(_i64)]),
    "annchor_dbscan_begin": (ctypes.c_int, [_vp, _i32]),
    "annchor_dbscan_absorb": (ctypes.c_int, [_vp, ctypes.POINTER(_i64)]),
    "annchor_dbscan_edges": (ctypes.c_int, [_vp, _vp, _i64]),
    "annchor_dbscan_finish": (ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(_i64)]),
    "annchor_knn_exact_begin": (ctypes.c_int, [_vp, _i32, _vp, _dbl, _i32, _vp]),
    "annchor_knn_exact_rows": (ctypes.c_int, [_vp, _i64, _i64, _i64, _i64, _i64, _i32, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    "annchor_knn_exact_fetch": (ctypes.c_int, [_vp, _vp]),
    "annchor_knn_exact_edges": (ctypes.c_int, [_vp, _vp, _vp, _i64]),
    "annchor_knn_exact_finish": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32]),
    "annchor_graph_to_coo": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, ctypes.POINTER(_i64)]),
    "annchor_field_size": (ctypes.c_int, [_vp, _i32, ctypes.POINTER(_i64)]),
    "annchor_download": (ctypes.c_int, [_vp, _i32, _vp, _i64]),
    "annchor_upload": (ctypes.c_int, [_vp, _i32, _vp, _i64]),
    "annchor_prof_enable": (ctypes.c_int, [_vp, _i32]),
    "annchor_prof_reset": (ctypes.c_int, [_vp]),
    "annchor_prof_get": (ctypes.c_int, [_vp, _i32, _vp, _vp, _vp, _vp]),
}

_lib = None


class NativeError(RuntimeError):
    pass


def exported_symbols():
    return sorted(_SIGNATURES)


def load_library():
    """Load libannchor_hip.so and bind every declared entry point (no GPU needed)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                "libannchor_hip.so is not built (%s).  Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `python annchor_amd/build.py`; there is no CPU fallback." % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def release_parked_contexts():
    """Free the runtime shells (stream, pinned staging, device slab) that destroyed engines left
    parked for the next one; returns how many there were."""
    return int(load_library().annchor_release_parked())


PAIR_BYTES = 130            # device memory per candidate pair of the pair-list form (with scratch)
PAIR_LIST_MAX = (1 << 30) - 1   # int32 positions into the per-point index (two entries per pair)


def pairlist_point_limit(device=0):
    """Largest data set whose complete pair list (nx (nx - 1) / 2 candidates, the worst case of the locality filter) the
    pair-list form will materialise on `device`: bounded by the int32 pair positions (2^30 pairs: 46 341 points) and by
    80 % of the device's free memory at PAIR_BYTES per pair.  None when no device can be asked.  Blocks this process keeps
    parked for reuse count as free -- they are NOT handed back to the driver here: a gigabyte request that follows the release
    of tens of gigabytes waited ~1.5 s on this stack (every second fit of 100 000 points, tools/lev100k_profile.py)."""
    f, t, parked = _i64(), _i64(), _i64()
    try:
        if load_library().annchor_device_mem_info(int(device), ctypes.byref(f), ctypes.byref(t)) != 0:
            return None
        if load_library().annchor_parked_bytes(int(device), ctypes.byref(parked)) != 0:
            return None
    except NativeError:
        return None
    pairs = min(PAIR_LIST_MAX, int(0.8 * (f.value + parked.value) / PAIR_BYTES))
    return int((1 + (1 + 8 * pairs) ** 0.5) // 2)


def bind_to_device_numa(device=0):
    """Restrict this process (and the threads it starts from now on) to the CPUs of the NUMA node
    the GPU hangs off -- what `numactl --cpunodebind` does for a launcher.  Call it before the first
    Annchor / Engine is created.  On the MI355X box the C2 fit takes 5.25 ms from the GPU's node and
    5.57 ms from the other one.  Returns a description, or None when the topology cannot be read."""
    import os

    buf = ctypes.create_string_buffer(64)
    try:
        if load_library().annchor_device_pci_bus_id(int(device), buf, 64) != 0:
            return None
        bus = buf.value.decode().lower()
        with open("/sys/bus/pci/devices/%s/numa_node" % bus) as fh:
            node = int(fh.read())
        if node < 0:
            return None
        with open("/sys/devices/system/node/node%d/cpulist" % node) as fh:
            cpus = set()
            for part in fh.read().strip().split(","):
                lo, _, hi = part.partition("-")
                cpus.update(range(int(lo), int(hi or lo) + 1))
        cpus &= os.sched_getaffinity(0)
        if not cpus:
            return None
        os.sched_setaffinity(0, cpus)
        return "NUMA node %d of GPU %s (%d CPUs)" % (node, bus, len(cpus))
    except (OSError, ValueError, AttributeError):
        return None


def stream_budget(n_tiles, p_work, join_passes):
    """(total, tile_phase, per_pass): the streamed form's per-row-tile work budget and its split
    between the tile phase and the join passes (include/annchor_hip.h: annchor_stream_budget)."""
    T, tp, pp = _i32(), _i32(), _i32()
    rc = load_library().annchor_stream_budget(int(n_tiles), float(p_work), int(join_passes), ctypes.byref(T), ctypes.byref(tp),
                                              ctypes.byref(pp))
    if rc != 0:
        raise NativeError("annchor_stream_budget failed (%d)" % rc)
    return T.value, tp.value, pp.value


# A stream is produced AHEAD of its draw only up to this many 32-bit words (1 GB): the ahead-of-time size is a bound from the
# point count (1.5 x nx (nx - 1) / 2 -- 7.5 x 10^9 words for the thinned lists of 10^5 points, most of which the draw would never
# read); beyond it the draw itself generates what it consumes, sized from the real bin populations (annchor_legacy_choice_ranks).
LEGACY_EAGER_MAX_DRAWS = 1 << 28


def comm_unique_id():
    """128 bytes from which the ranks of a job build their in-library RCCL communicator (call on ONE rank, hand the bytes
    to the others by any means: Engine.comm_init)."""
    buf = (ctypes.c_uint8 * 128)()
    rc = load_library().annchor_comm_unique_id(buf)
    if rc != 0:
        raise NativeError("annchor_comm_unique_id failed (%d): RCCL not loadable?" % rc)
    return bytes(buf)


def legacy_prefetch(seed, ndraws):
    """Begin producing the legacy MT19937 stream of `seed` on a background thread."""
    if 0 <= seed < 2 ** 32 and 0 < ndraws <= LEGACY_EAGER_MAX_DRAWS:
        rc = load_library().annchor_legacy_prefetch(int(seed), int(ndraws))
        if rc != 0:
            raise NativeError("annchor_legacy_prefetch failed (%d)" % rc)


def legacy_generate(seed, ndraws):
    """Produce the legacy MT19937 stream of `seed` on the calling thread (returns when it is there)."""
    if 0 <= seed < 2 ** 32 and 0 < ndraws <= LEGACY_EAGER_MAX_DRAWS:
        rc = load_library().annchor_legacy_generate(int(seed), int(ndraws))
        if rc != 0:
            raise NativeError("annchor_legacy_generate failed (%d)" % rc)


def lev_persist_state(set=-1):
    """The picker's persistent anchor launch: 1 armed, 0 switched off (the library does that itself after two launches that gave
    up -- a GPU shared with another process); set=1 re-arms, set=0 switches it off."""
    return int(load_library().annchor_lev_persist_state(int(set)))


def legacy_choice_ranks(seed, counts, want):
    """np.random.seed(seed); per bin np.random.permutation(counts[b])[:want[b]] (or the whole
    bin when it is smaller) -- NumPy's legacy stream, generated by the library's host code."""
    lib = load_library()
    counts, want = _c(counts, np.int64), _c(want, np.int64)
    out = np.zeros(int(np.minimum(counts, want).sum()), dtype=np.int64)
    n_out = np.zeros(len(counts), dtype=np.int64)
    rc = lib.annchor_legacy_choice_ranks(int(seed) & 0xFFFFFFFF, _ptr(counts), _ptr(want), len(counts), _ptr(out), _ptr(n_out))
    if rc != 0:
        raise NativeError("annchor_legacy_choice_ranks failed (%d)" % rc)
    return np.split(out, np.cumsum(n_out)[:-1])


_DGELSD = None


def _dgelsd_pointer():
    """Address of scipy's Fortran dgelsd (the routine scipy.linalg.lapack.dgelsd wraps), or 0."""
    global _DGELSD
    if _DGELSD is None:
        try:
            from scipy.linalg import cython_lapack
            cap = cython_lapack.__pyx_capi__["dgelsd"]
            api = ctypes.pythonapi
            api.PyCapsule_GetName.restype, api.PyCapsule_GetName.argtypes = ctypes.c_char_p, [ctypes.py_object]
            api.PyCapsule_GetPointer.restype, api.PyCapsule_GetPointer.argtypes = ctypes.c_void_p, [ctypes.py_object, ctypes.c_char_p]
            _DGELSD = api.PyCapsule_GetPointer(cap, api.PyCapsule_GetName(cap)) or 0
        except Exception:  # noqa: BLE001 -- no scipy.linalg.cython_lapack: the Python path does the work
            _DGELSD = 0
    return _DGELSD


def ols_bins(Xs, ys, cuts):
    """Per-partition OLS pieces (coef, xmean, ymean, status) for samples grouped by partition; Xs is
    the (n, nf) design matrix in column-major order, ys the targets, cuts the partition boundaries.
    None when scipy's LAPACK pointer is not available."""
    ptr = _dgelsd_pointer()
    if not ptr:
        return None
    n, nf = Xs.shape
    Xf = np.asfortranarray(Xs, dtype=np.float64)
    ys = _c(ys, np.float64)
    cuts = _c(cuts, np.int64)
    nb = len(cuts) - 1
    coef, xm = np.zeros((nb, nf)), np.zeros((nb, nf))
    ym, status = np.zeros(nb), np.zeros(nb, dtype=np.int32)
    rc = load_library().annchor_ols_bins(ptr, _ptr(Xf), _ptr(ys), n, nf, _ptr(cuts), nb, _ptr(coef), _ptr(xm), _ptr(ym), _ptr(status))
    if rc != 0:
        raise NativeError("annchor_ols_bins failed (%d)" % rc)
    return coef, xm, ym, status


def legacy_choice_begin(seed, counts, want):
    """legacy_choice_ranks on the library's persistent worker thread: returns a ticket at once."""
    lib = load_library()
    counts, want = _c(counts, np.int64), _c(want, np.int64)
    t = _vp()
    rc = lib.annchor_legacy_choice_begin(int(seed) & 0xFFFFFFFF, _ptr(counts), _ptr(want), len(counts), ctypes.byref(t))
    if rc != 0:
        raise NativeError("annchor_legacy_choice_begin failed (%d)" % rc)
    return (t, int(np.minimum(counts, want).sum()), len(counts))


def legacy_choice_end(ticket):
    """Wait for legacy_choice_begin's draw; same return value as legacy_choice_ranks."""
    t, total, nbins = ticket
    out = np.zeros(total, dtype=np.int64)
    n_out = np.zeros(nbins, dtype=np.int64)
    rc = load_library().annchor_legacy_choice_end(t, _ptr(out), _ptr(n_out))
    if rc != 0:
        raise NativeError("annchor_legacy_choice_ranks failed (%d)" % rc)
    return np.split(out, np.cumsum(n_out)[:-1])


class GraphBuffers:
    """The result arrays of a large graph build -- int64 [rows, k] and float64 [rows, k] -- allocated AND touched on a
    helper thread while the GPU works.  A fresh NumPy array is untouched virtual memory: the device-to-host copy that
    fills it first has to fault every page in (240 MB at N = 10^6: 14 ms of page faults around a 4 ms copy at the 56 GB/s
    this host's PCIe link delivers).  The sizes are known when fit() starts, the host has nothing to do during the tile phase,
    and ctypes releases the GIL around the library calls: the faults move off the critical path."""

    def __init__(self, rows, k):
        import threading

        self.rows, self.k = int(rows), int(k)
        self.idx = self.dist = None
        self._t = threading.Thread(target=self._make, daemon=True)
        self._t.start()

    def _make(self):
        idx = np.empty((self.rows, self.k), dtype=np.int64)
        dist = np.empty((self.rows, self.k), dtype=np.float64)
        idx.fill(0)
        dist.fill(0.0)
        self.idx, self.dist = idx, dist

    def take(self, rows, k):
        """(idx, dist) if the shape matches, else fresh arrays."""
        self._t.join()
        if self.idx is not None and (self.rows, self.k) == (int(rows), int(k)):
            return self.idx, self.dist
        return np.empty((int(rows), int(k)), dtype=np.int64), np.empty((int(rows), int(k)), dtype=np.float64)


class Engine:
    """One device context (one GPU).  All pipeline state lives in HBM inside it."""

    def __init__(self, device=0):
        self.lib = load_library()
        h = _vp()
        rc = self.lib.annchor_create(int(device), ctypes.byref(h))
        if rc != 0:
            raise NativeError("annchor_create(device=%d) failed (%d): %s -- the HIP path is the only path; "
                              "no CPU fallback exists." % (device, rc, self.lib.annchor_create_error().decode()))
        self.h = h
        self.device = device
        self.nx = 0
        self.metric = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.annchor_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise NativeError("libannchor_hip error %d: %s" % (rc, self.lib.annchor_last_error(self.h).decode()))

    def device_name(self):
        buf = ctypes.create_string_buffer(256)
        self._chk(self.lib.annchor_device_name(self.h, buf, 256))
        return buf.value.decode()

    def synchronize(self):
        self._chk(self.lib.annchor_synchronize(self.h))

    def last_kernel_ms(self):
        ms = ctypes.c_float()
        self._chk(self.lib.annchor_last_kernel_ms(self.h, ctypes.byref(ms)))
        return ms.value

    # ------------------------------------------------------------ data set
    def set_strings(self, codes, offs, lens, alphabet):
        offs, lens = _c(offs, np.int64), _c(lens, np.int32)
        if np.asarray(codes).dtype == np.uint16:   # more than 256 distinct symbols: 16-bit codes
            codes = _c(codes, np.uint16)
            self._chk(self.lib.annchor_set_strings_u16(self.h, _ptr(codes), _ptr(offs), _ptr(lens), len(lens), int(alphabet)))
        else:
            codes = _c(codes, np.uint8)
            self._chk(self.lib.annchor_set_strings(self.h, _ptr(codes), _ptr(offs), _ptr(lens), len(lens), int(alphabet)))
        self.nx, self.metric = len(lens), METRIC_LEVENSHTEIN

    def set_points(self, X, cosine=False):
        X = np.asarray(X)
        if X.dtype == np.float32:
            X = _c(X, np.float32)
            fn = self.lib.annchor_set_points_cosine_f32 if cosine else self.lib.annchor_set_points_f32
            self._chk(fn(self.h, _ptr(X), X.shape[0], X.shape[1]))
            self.metric = METRIC_COSINE_F32 if cosine else METRIC_EUCLIDEAN_F32
        else:
            X = _c(X, np.float64)
            fn = self.lib.annchor_set_points_cosine_f64 if cosine else self.lib.annchor_set_points_f64
            self._chk(fn(self.h, _ptr(X), X.shape[0], X.shape[1]))
            self.metric = METRIC_COSINE_F64 if cosine else METRIC_EUCLIDEAN_F64
        self.nx = X.shape[0]

    def _set_pool(self, name, values, offs, lens, extra, metric_f32, metric_f64, *more):
        """The ragged pool of set_series, set_series_nd, set_edr_series, set_lcss_series, set_curves, set_point_sets, set_erp_series,
        set_msm_series, set_twe_series and set_clouds:
        annchor_set_<name>_f32 for float32 values, _f64 for anything else; `extra` is the entry point's integer argument (None: it
        has none), `more` what follows it."""
        offs, lens = _c(offs, np.int64), _c(lens, np.int32)
        f32 = np.asarray(values).dtype == np.float32
        values = _c(values, np.float32 if f32 else np.float64)
        fn = getattr(self.lib, "annchor_set_%s_%s" % (name, "f32" if f32 else "f64"))
        more = more if extra is None else (int(extra),) + more
        self._chk(fn(self.h, _ptr(values), _ptr(offs), _ptr(lens), len(lens), *more))
        self.nx, self.metric = len(lens), metric_f32 if f32 else metric_f64

    def set_series(self, values, offs, lens, window=None):
        """Time series for dynamic time warping: pooled values (float32 or float64), int64 offsets, int32 lengths;
        window None: unconstrained, else the Sakoe-Chiba half width."""
        self._set_pool("series", values, offs, lens, -1 if window is None else window, METRIC_DTW_F32, METRIC_DTW_F64)

    def set_series_nd(self, values, offs, lens, dim, window=None):
        """Series of `dim` coordinates per point for dynamic time warping: the points end to end (float32 or float64); int64
        offsets and int32 lengths counted in points; window as set_series takes it."""
        self._set_pool("series_nd", values, offs, lens, dim, METRIC_DTW_F32, METRIC_DTW_F64, -1 if window is None else int(window))

    def set_edr_series(self, values, offs, lens, dim, eps, normalize=False):
        """Series for the edit distance on real sequences: the points end to end (float32 or float64), `dim` coordinates each;
        int64 offsets and int32 lengths counted in points; `eps` the matching threshold per coordinate, a finite float >= 0;
        normalize: divide the edit count by the longer member's length."""
        self._set_pool("edr_series", values, offs, lens, dim, METRIC_EDR_F32, METRIC_EDR_F64, float(eps), int(bool(normalize)))

    def set_lcss_series(self, values, offs, lens, dim, eps, delta=None):
        """Series for the longest-common-subsequence distance: the points end to end (float32 or float64), `dim` coordinates
        each; int64 offsets and int32 lengths counted in points; `eps` the matching threshold per coordinate, a finite float
        >= 0; delta None: matched points may be any time apart, else at most `delta` steps."""
        self._set_pool("lcss_series", values, offs, lens, dim, METRIC_LCSS_F32, METRIC_LCSS_F64, float(eps),
                       -1 if delta is None else int(delta))

    def set_curves(self, values, offs, lens, dim):
        """Curves for the discrete Frechet distance: the points end to end (float32 or float64), `dim` coordinates each;
        int64 offsets and int32 lengths counted in points."""
        self._set_pool("curves", values, offs, lens, dim, METRIC_FRECHET_F32, METRIC_FRECHET_F64)

    def set_erp_series(self, values, offs, lens, dim, gap=0.0):
        """Series for the edit distance with real penalty: the points end to end (float32 or float64), `dim` coordinates each;
        int64 offsets and int32 lengths counted in points; `gap` the gap value, a finite float."""
        self._set_pool("erp_series", values, offs, lens, dim, METRIC_ERP_F32, METRIC_ERP_F64, float(gap))

    def set_msm_series(self, values, offs, lens, c=1.0):
        """Univariate series for Move-Split-Merge: pooled values (float32 or float64), int64 offsets, int32 lengths; `c` the cost of
        a split or merge, a finite float above 0."""
        self._set_pool("msm_series", values, offs, lens, None, METRIC_MSM_F32, METRIC_MSM_F64, float(c))

    def set_twe_series(self, values, offs, lens, dim, nu=0.001, lam=1.0):
        """Series for the time warp edit distance: the points end to end (float32 or float64), `dim` coordinates each; int64
        offsets and int32 lengths counted in points; `nu` the stiffness and `lam` the penalty of a delete, finite floats >= 0."""
        self._set_pool("twe_series", values, offs, lens, dim, METRIC_TWE_F32, METRIC_TWE_F64, float(nu), float(lam))

    def set_coded_strings(self, codes, offs, lens, substitution, indel):
        """Strings for the weighted Levenshtein distance: uint8 dense codes below A, int64 offsets and int32 lengths counted in
        symbols (a string may be empty); `substitution` float64 [A, A], `indel` float64 [A]."""
        codes, offs, lens = _c(codes, np.uint8), _c(offs, np.int64), _c(lens, np.int32)
        substitution, indel = _c(substitution, np.float64), _c(indel, np.float64)
        A = indel.size
        assert indel.ndim == 1 and substitution.shape == (A, A), "substitution must be [A, A] and indel [A]"
        if codes.size == 0:
            codes = np.zeros(1, dtype=np.uint8)
        self._chk(self.lib.annchor_set_coded_strings(self.h, _ptr(codes), _ptr(offs), _ptr(lens), len(lens), A, _ptr(substitution),
                                                     _ptr(indel)))
        self.nx, self.metric = len(lens), METRIC_WEIGHTED_LEVENSHTEIN

    def set_coded_strings_affine(self, codes, offs, lens, substitution, extend, open):
        """Strings for the affine-gap alignment distance: codes, offsets, lengths and `substitution` as set_coded_strings takes them
        (0 .. 1024 symbols per string); `extend` float64 [A], the cost of each symbol inside a gap; `open` the cost of opening a
        gap, a finite float >= 0."""
        codes, offs, lens = _c(codes, np.uint8), _c(offs, np.int64), _c(lens, np.int32)
        substitution, extend = _c(substitution, np.float64), _c(extend, np.float64)
        A = extend.size
        assert extend.ndim == 1 and substitution.shape == (A, A), "substitution must be [A, A] and extend [A]"
        if codes.size == 0:
            codes = np.zeros(1, dtype=np.uint8)
        self._chk(self.lib.annchor_set_coded_strings_affine(self.h, _ptr(codes), _ptr(offs), _ptr(lens), len(lens), A,
                                                            _ptr(substitution), _ptr(extend), float(open)))
        self.nx, self.metric = len(lens), METRIC_AFFINE_GAP

    def set_coded_strings_osa(self, codes, offs, lens, substitution, indel, transpose):
        """Strings for optimal string alignment: codes, offsets, lengths, `substitution` and `indel` as set_coded_strings takes
        them (0 .. 1024 symbols per string); `transpose` the cost of swapping two adjacent symbols, a float >= 0, +inf for "no
        transpositions"."""
        codes, offs, lens = _c(codes, np.uint8), _c(offs, np.int64), _c(lens, np.int32)
        substitution, indel = _c(substitution, np.float64), _c(indel, np.float64)
        A = indel.size
        assert indel.ndim == 1 and substitution.shape == (A, A), "substitution must be [A, A] and indel [A]"
        if codes.size == 0:
            codes = np.zeros(1, dtype=np.uint8)
        self._chk(self.lib.annchor_set_coded_strings_osa(self.h, _ptr(codes), _ptr(offs), _ptr(lens), len(lens), A,
                                                         _ptr(substitution), _ptr(indel), float(transpose)))
        self.nx, self.metric = len(lens), METRIC_OSA

    def set_point_sets(self, values, offs, lens, dim):
        """Point sets for the Hausdorff distance: the points end to end (float32 or float64), `dim` coordinates each; int64
        offsets and int32 lengths counted in points."""
        self._set_pool("point_sets", values, offs, lens, dim, METRIC_HAUSDORFF_F32, METRIC_HAUSDORFF_F64)

    def set_clouds(self, values, offs, lens, dim):
        """Point clouds for the earth mover's distance: the points end to end (float32 or float64), `dim` coordinates each; int64
        offsets and int32 lengths counted in points."""
        self._set_pool("clouds", values, offs, lens, dim, METRIC_EMD_POINTS_F32, METRIC_EMD_POINTS_F64)

    def set_token_sets(self, codes, offs, lens):
        """Sets of integers for the Jaccard distance, tokens form: int32 codes, non-negative and strictly ascending within a member;
        int64 offsets and int32 sizes counted in codes.  A member may be empty."""
        codes, offs, lens = _c(codes, np.int32), _c(offs, np.int64), _c(lens, np.int32)
        if codes.size == 0:
            codes = np.zeros(1, dtype=np.int32)
        self._chk(self.lib.annchor_set_token_sets(self.h, _ptr(codes), _ptr(offs), _ptr(lens), len(lens)))
        self.nx, self.metric = len(lens), METRIC_JACCARD_TOKENS

    def set_bitsets(self, words, nbits):
        """Sets of integers for the Jaccard distance, bits form: uint32 [nx, W], W = ceil(nbits / 32) rounded up to a multiple of 4;
        bit p of a member is bit p % 32 of word p // 32, the bits from nbits on are zero."""
        words = _c(words, np.uint32)
        W = (-(-max(int(nbits), 1) // 32) + 3) // 4 * 4
        assert words.ndim == 2 and words.shape[1] == W, "words must be [nx, %d] for %d bits" % (W, nbits)
        self._chk(self.lib.annchor_set_bitsets(self.h, _ptr(words), words.shape[0], int(nbits)))
        self.nx, self.metric = words.shape[0], METRIC_JACCARD_BITS

    def set_histograms(self, X, cost, wide=False):
        X, cost = _c(X, np.float64), _c(cost, np.float64)
        assert cost.shape == (X.shape[1], X.shape[1]), "cost_matrix must be [nbins, nbins]"
        fn = self.lib.annchor_set_histograms_wide if wide else self.lib.annchor_set_histograms
        self._chk(fn(self.h, _ptr(X), X.shape[0], X.shape[1], _ptr(cost)))
        self.nx, self.metric = X.shape[0], METRIC_WASSERSTEIN

    def set_opaque(self, nx):
        self._chk(self.lib.annchor_set_opaque(self.h, int(nx)))
        self.nx, self.metric = int(nx), 0

    # ----------------------------------------------------------- metric (a2)
    def metric_pairs(self, IJ):
        IJ = _c(IJ, np.int64).reshape(-1, 2)
        out = np.zeros(IJ.shape[0], dtype=np.float64)
        self._chk(self.lib.annchor_metric_pairs(self.h, _ptr(IJ), IJ.shape[0], _ptr(out)))
        return out

    def brute_force(self, k):
        idx = np.zeros((self.nx, k), dtype=np.int64)
        dist = np.zeros((self.nx, k), dtype=np.float64)
        self._chk(self.lib.annchor_brute_force(self.h, int(k), _ptr(idx), _ptr(dist)))
        return idx, dist

    # -------------------------------------------------------------- anchors
    def pick_anchors_maxmin(self, na, first):
        self._chk(self.lib.annchor_pick_anchors_maxmin(self.h, int(na), int(first)))

    def pick_anchors_selected(self, A):
        A = _c(A, np.int64)
        self._chk(self.lib.annchor_pick_anchors_selected(self.h, _ptr(A), len(A)))

    def set_anchor_distances(self, D, A):
        D = _c(D, np.float64)
        A = _c(A, np.int64).reshape(-1)
        if D.ndim != 2 or D.shape[0] != self.nx:
            raise ValueError("anchor distances must be [nx=%d, n_anchors], got %r" % (self.nx, D.shape))
        self._chk(self.lib.annchor_set_anchor_distances(self.h, _ptr(D), D.shape[1], _ptr(A) if len(A) else None, len(A)))

    # ------------------------------------------------------------- pipeline
    def build_locality(self, locality, loc_thresh, loc_min):
        n, m = _i64(), _i64()
        self._chk(self.lib.annchor_build_locality(self.h, int(locality), int(loc_thresh), int(loc_min),
                                                  ctypes.byref(n), ctypes.byref(m)))
        return n.value, m.value

    def build_query_locality(self, nx_base, locality, loc_thresh):
        n, m = _i64(), _i64()
        self._chk(self.lib.annchor_build_query_locality(self.h, int(nx_base), int(locality), int(loc_thresh),
                                                        ctypes.byref(n), ctypes.byref(m)))
        return n.value, m.value

    def compute_features(self):
        self._chk(self.lib.annchor_compute_features(self.h))

    def count_uncomputed(self):
        n = _i64()
        self._chk(self.lib.annchor_count_uncomputed(self.h, ctypes.byref(n)))
        return n.value

    def sampler_stats(self, iq1, iq3, n_partitions):
        """(q1, q3, edges or None, counts or None): the two quantiles and -- when the library could chain them on the device --
        the bin edges and populations of a sampling step, in one host wait."""
        ks = np.array([iq1, iq3], dtype=np.int64)
        q = np.empty(2, dtype=np.float64)
        edges = np.empty(n_partitions + 1, dtype=np.float64)
        counts = np.empty(n_partitions, dtype=np.int64)
        fused = ctypes.c_int32(0)
        self._chk(self.lib.annchor_sampler_stats(self.h, _ptr(ks), int(n_partitions), _ptr(q), _ptr(edges), _ptr(counts),
                                                 ctypes.byref(fused)))
        if fused.value:
            return q[0], q[1], edges, counts
        return q[0], q[1], None, None

    def kth_uncomputed_dad(self, ks):
        ks = _c(ks, np.int64)
        out = np.zeros(len(ks), dtype=np.float64)
        self._chk(self.lib.annchor_kth_uncomputed_dad(self.h, _ptr(ks), len(ks), _ptr(out)))
        return out

    def bin_counts(self, bins):
        bins = _c(bins, np.float64)
        out = np.zeros(len(bins) - 1, dtype=np.int64)
        self._chk(self.lib.annchor_bin_counts(self.h, _ptr(bins), len(bins) - 1, _ptr(out)))
        return out

    def select_by_rank(self, bins, bin_of, ranks):
        bins, bin_of, ranks = _c(bins, np.float64), _c(bin_of, np.int32), _c(ranks, np.int64)
        out = np.zeros(len(ranks), dtype=np.int64)
        self._chk(self.lib.annchor_select_by_rank(self.h, _ptr(bins), len(bins) - 1, _ptr(bin_of), _ptr(ranks),
                                                  len(ranks), _ptr(out)))
        return out

    def sample_pairs(self, bins, counts, bin_of, ranks):
        """select_by_rank + gather_features + evaluate_samples in one call (device metric only)."""
        bins, counts = _c(bins, np.float64), _c(counts, np.int64)
        bin_of, ranks = _c(bin_of, np.int32), _c(ranks, np.int64)
        m = len(ranks)
        pos, feats, y = np.empty(m, dtype=np.int64), np.empty((m, 4), dtype=np.float64), np.empty(m, dtype=np.float64)
        self._chk(self.lib.annchor_sample_pairs(self.h, _ptr(bins), len(bins) - 1, _ptr(counts), _ptr(bin_of), _ptr(ranks), m,
                                                _ptr(pos), _ptr(feats), _ptr(y)))
        return pos, feats, y

    # ---- the iteration's models fitted on the device (csrc/model.hip): no host round trip between the stages
    def sample_pairs_device(self, bins, counts, bin_of, ranks):
        bins, counts = _c(bins, np.float64), _c(counts, np.int64)
        bin_of, ranks = _c(bin_of, np.int32), _c(ranks, np.int64)
        self._chk(self.lib.annchor_sample_pairs_device(self.h, _ptr(bins), len(bins) - 1, _ptr(counts), _ptr(bin_of), _ptr(ranks), len(ranks)))
        return len(ranks)

    def hash_sample_pairs_device(self, bins, counts, want, seed_key):
        bins, counts, want = _c(bins, np.float64), _c(counts, np.int64), _c(want, np.int64)
        m = _i64()
        self._chk(self.lib.annchor_hash_sample_pairs_device(self.h, _ptr(bins), len(bins) - 1, _ptr(counts), _ptr(want),
                                                            ctypes.c_uint64(int(seed_key)), ctypes.byref(m)))
        return int(m.value)

    def download_samples(self, m, predict=True):
        """(positions, feature rows, distances, unclipped predictions) of the device-resident sample."""
        pos, feats, y = np.empty(m, dtype=np.int64), np.empty((m, 4), dtype=np.float64), np.empty(m, dtype=np.float64)
        sp = np.empty(m, dtype=np.float64) if predict else None
        self._chk(self.lib.annchor_download_samples(self.h, _ptr(pos), _ptr(feats), _ptr(y), _ptr(sp)))
        return pos, feats, y, sp

    def fit_regression_device(self, bins, first, is_metric):
        bins = _c(bins, np.float64)
        self._chk(self.lib.annchor_fit_regression_device(self.h, _ptr(bins), len(bins) - 1, int(first), int(is_metric)))

    def fit_errors_device(self):
        self._chk(self.lib.annchor_fit_errors_device(self.h))

    def model_download(self, nb, with_errors=True):
        """(W [nb, 3], c [nb], status [nb], err_ptr [nb + 1] or None, flags [3]); waits; clears the sticky flags."""
        W, c = np.zeros((nb, 3)), np.zeros(nb)
        status, flags = np.zeros(nb, dtype=np.int32), np.zeros(3, dtype=np.int32)
        ep = np.zeros(nb + 1, dtype=np.int64) if with_errors else None
        self._chk(self.lib.annchor_model_download(self.h, _ptr(W), _ptr(c), _ptr(status), _ptr(ep), _ptr(flags)))
        return W, c, status, ep, flags

    def model_download_with_errors(self, nb, cap):
        """model_download + errors_download behind one wait: (W, c, status, err_ptr, flags, errs or None)."""
        W, c = np.zeros((nb, 3)), np.zeros(nb)
        status, flags = np.zeros(nb, dtype=np.int32), np.zeros(3, dtype=np.int32)
        ep = np.zeros(nb + 1, dtype=np.int64)
        errs = np.empty(int(cap), dtype=np.float64)
        n = _i64()
        self._chk(self.lib.annchor_model_download_with_errors(self.h, _ptr(W), _ptr(c), _ptr(status), _ptr(ep), _ptr(flags), _ptr(errs),
                                                             int(cap), ctypes.byref(n)))
        return W, c, status, ep, flags, (errs[:n.value] if n.value >= 0 else None)

    def errors_download(self, n):
        out = np.empty(int(n), dtype=np.float64)
        self._chk(self.lib.annchor_errors_download(self.h, _ptr(out), int(n)))
        return out

    def sample_pairs_device_draw(self, bins, counts, want, seed):
        """The legacy draw + the sampling step in one call, the draw's trace on the device: (taken, number of samples)."""
        bins, counts, want = _c(bins, np.float64), _c(counts, np.int64), _c(want, np.int64)
        n, taken = _i64(), _i32()
        self._chk(self.lib.annchor_sample_pairs_device_draw(self.h, _ptr(bins), len(bins) - 1, _ptr(counts), _ptr(want), int(seed),
                                                           ctypes.byref(n), ctypes.byref(taken)))
        return bool(taken.value), int(n.value)

    def legacy_choice_ranks_device(self, seed, counts, want):
        """legacy_choice_ranks through the device-side trace (tests): list of per-bin rank arrays, or None when not applicable."""
        counts, want = _c(counts, np.int64), _c(want, np.int64)
        n_out = np.minimum(counts, want)
        out = np.full(int(n_out.sum()), -1, dtype=np.int64)
        taken = _i32()
        self._chk(self.lib.annchor_legacy_choice_ranks_device(self.h, int(seed), _ptr(counts), _ptr(want), len(counts), _ptr(out),
                                                             ctypes.byref(taken)))
        if not taken.value:
            return None
        offs = np.concatenate([[0], np.cumsum(n_out)])
        return [out[offs[b]:offs[b + 1]] for b in range(len(counts))]

    def hash_sample(self, bins, counts, want, seed_key):
        """Hashed stratified choice (annchor_hash_sample): positions of the samples, partition by partition."""
        bins, counts, want = _c(bins, np.float64), _c(counts, np.int64), _c(want, np.int64)
        out = np.empty(int(np.minimum(counts, want).sum()), dtype=np.int64)
        n = _i64()
        self._chk(self.lib.annchor_hash_sample(self.h, _ptr(bins), len(bins) - 1, _ptr(counts), _ptr(want), int(seed_key) & (2 ** 64 - 1),
                                               _ptr(out), ctypes.byref(n)))
        return out[:n.value]

    def hash_sample_pairs(self, bins, counts, want, seed_key):
        """hash_sample + gather_features + evaluate_samples in one call (device metric only)."""
        bins, counts, want = _c(bins, np.float64), _c(counts, np.int64), _c(want, np.int64)
        m = int(np.minimum(counts, want).sum())
        pos, feats, y = np.empty(m, dtype=np.int64), np.empty((m, 4), dtype=np.float64), np.empty(m, dtype=np.float64)
        n = _i64()
        self._chk(self.lib.annchor_hash_sample_pairs(self.h, _ptr(bins), len(bins) - 1, _ptr(counts), _ptr(want), int(seed_key) & (2 ** 64 - 1),
                                                     _ptr(pos), _ptr(feats), _ptr(y), ctypes.byref(n)))
        return pos[:n.value], feats[:n.value], y[:n.value]

    def gather_features(self, pos):
        pos = _c(pos, np.int64)
        out = np.zeros((len(pos), 4), dtype=np.float64)
        self._chk(self.lib.annchor_gather_features(self.h, _ptr(pos), len(pos), _ptr(out)))
        return out

    def evaluate_samples(self, pos):
        pos = _c(pos, np.int64)
        out = np.zeros(len(pos), dtype=np.float64)
        self._chk(self.lib.annchor_evaluate_samples(self.h, _ptr(pos), len(pos), _ptr(out)))
        return out

    def set_samples(self, pos, y):
        pos, y = _c(pos, np.int64), _c(y, np.float64)
        self._chk(self.lib.annchor_set_samples(self.h, _ptr(pos), len(pos), _ptr(y)))

    def predict_merge(self, bins, W, c, first, is_metric, n_samples):
        bins, W, c = _c(bins, np.float64), _c(W, np.float64), _c(c, np.float64)
        sp = np.zeros(n_samples, dtype=np.float64)
        self._chk(self.lib.annchor_predict_merge(self.h, _ptr(bins), len(bins) - 1, _ptr(W), _ptr(c), int(first),
                                                 int(is_metric), _ptr(sp)))
        return sp

    def n_pairs(self):
        return self.field_size(F_NCM)

    def merge_host_prediction(self, pred, first, is_metric):
        pred = _c(pred, np.float64).reshape(-1)
        if pred.shape[0] != self.n_pairs():
            raise ValueError("regression.predict returned %d values for %d candidate pairs" % (pred.shape[0], self.n_pairs()))
        self._chk(self.lib.annchor_merge_host_prediction(self.h, _ptr(pred), int(first), int(is_metric)))

    def set_labels(self, labels):
        labels = _c(labels, np.int64).reshape(-1)
        if labels.shape[0] != self.n_pairs():
            raise ValueError("error_predictor.predict returned %d labels for %d candidate pairs" % (labels.shape[0], self.n_pairs()))
        if labels.size and (labels.min() < 0 or labels.max() >= 255):
            raise ValueError("error labels must lie in 0..254 (got %d..%d)" % (labels.min(), labels.max()))
        self._chk(self.lib.annchor_set_labels(self.h, _ptr(labels)))

    def select_candidates(self, n_neighbors, nmin, errs_list, n_refine, lookahead, n_labels=None):
        """errs_list None: the residual lists fit_errors_device left on the device (n_labels of them)."""
        nc, nn = _i64(), _i64()
        if errs_list is None:
            self._chk(self.lib.annchor_select_candidates(self.h, int(n_neighbors), int(nmin), None, None, int(n_labels), int(n_refine),
                                                         int(lookahead), ctypes.byref(nc), ctypes.byref(nn)))
            return nc.value, nn.value
        ptr = np.zeros(len(errs_list) + 1, dtype=np.int64)
        np.cumsum([len(e) for e in errs_list], out=ptr[1:])
        errs = _c(np.concatenate(errs_list) if len(errs_list) else np.zeros(0), np.float64)
        self._chk(self.lib.annchor_select_candidates(self.h, int(n_neighbors), int(nmin), _ptr(errs), _ptr(ptr),
                                                     len(errs_list), int(n_refine), int(lookahead),
                                                     ctypes.byref(nc), ctypes.byref(nn)))
        return nc.value, nn.value

    def select_prepare(self, n_neighbors, nmin):
        """Thresholds + guarantee_nmin of the next select_candidates, launched ahead (no host wait)."""
        self._chk(self.lib.annchor_select_prepare(self.h, int(n_neighbors), int(nmin)))

    def mark_candidates(self):
        self._chk(self.lib.annchor_mark_candidates(self.h))

    def refine_candidates(self):
        self._chk(self.lib.annchor_refine_candidates(self.h))

    def park_refine(self, action):
        """1: the next sampler_stats call queues the refinement launch behind its download; 2: launch it now if still parked."""
        self._chk(self.lib.annchor_park_refine(self.h, int(action)))

    def set_refined(self, exact):
        exact = _c(exact, np.float64)
        self._chk(self.lib.annchor_set_refined(self.h, _ptr(exact), len(exact)))

    def update_bounds(self):
        self._chk(self.lib.annchor_update_bounds(self.h))

    def update_bounds_prepare(self):
        """update_bounds' mask-only prefix on the side stream (a no-op on an engine created with ANNCHOR_FIT_OVERLAP=0)."""
        self._chk(self.lib.annchor_update_bounds_prepare(self.h))

    def overlap_stats(self):
        """(the engine uses a side stream, calls of update_bounds that found their lists prepared): host state, no wait."""
        out = np.zeros(2, dtype=np.int64)
        self._chk(self.lib.annchor_overlap_stats(self.h, _ptr(out)))
        return bool(out[0]), int(out[1])

    def neighbor_graph(self, k):
        idx = np.zeros((self.nx, k), dtype=np.int64)
        dist = np.zeros((self.nx, k), dtype=np.float64)
        self._chk(self.lib.annchor_neighbor_graph(self.h, int(k), _ptr(idx), _ptr(dist)))
        return idx, dist

    # ------------------------------------------------------- streamed form
    def stream_bind(self, X, global_base=0, device_ptr=None, shape=None):
        """Bind this rank's rows: a float32 NumPy array, or a raw device pointer + shape."""
        if device_ptr is not None:
            n, d = shape
            self._chk(self.lib.annchor_stream_bind(self.h, device_ptr, int(n), int(d), int(global_base), 1))
        else:
            X = _c(X, np.float32)
            n, d = X.shape
            self._chk(self.lib.annchor_stream_bind(self.h, _ptr(X), n, d, int(global_base), 0))
        self.nx, self.metric = int(n), METRIC_EUCLIDEAN_F32
        self._stream_dim = int(d)

    def stream_bind_f64(self, X, global_base=0, centre=None):
        """Bind float64 rows: they stay resident in float64; their centred float32 copy becomes the bound rows of stream_bind.
        centre: float64 [dim] to subtract (queries: the data set's), None = the column means.  Returns (centre, device pointer
        of the float64 rows)."""
        X = _c(X, np.float64)
        n, d = X.shape
        cin = _c(centre, np.float64) if centre is not None else None
        if cin is not None and cin.shape != (d,):
            raise ValueError("centre must be float64 [%d]" % d)
        cout, rows = np.empty(d, dtype=np.float64), _vp()
        self._chk(self.lib.annchor_stream_bind_f64(self.h, _ptr(X), n, d, int(global_base), _ptr(cin), _ptr(cout), ctypes.byref(rows)))
        self.nx, self.metric = int(n), METRIC_EUCLIDEAN_F32
        self._stream_dim = int(d)
        return cout, rows.value

    def stream_rerank64(self, k, n_local, out=None):
        """After stream_knn(..., fetch=False) with longer lists: the float64 re-rank, guard and repair; (idx int64, dist float64)
        [n_local, k] in the bound rows' own order, column 0 = self."""
        if out is not None:
            idx, dist = out.take(n_local, k)
        else:
            idx = np.empty((int(n_local), int(k)), dtype=np.int64)
            dist = np.empty((int(n_local), int(k)), dtype=np.float64)
        self._chk(self.lib.annchor_stream_rerank64(self.h, int(k), _ptr(idx), _ptr(dist)))
        return idx, dist

    def stream_query64(self, cols, n_all, nt_all, n_anchors, dim_padded, nn, nn_search, p_work, rows64, n_data, data_base=0):
        """stream_query for queries bound with stream_bind_f64: nn_search entries searched in float32, nn kept after the float64
        re-rank against the data set's float64 rows (device pointer rows64)."""
        idx = np.empty((self.nx, nn), dtype=np.int64)
        dist = np.empty((self.nx, nn), dtype=np.float64)
        ev = _i64()
        self._chk(self.lib.annchor_stream_query64(self.h, cols["Xs"], cols["rs"], cols["perm"], cols["lo"], cols["hi"], cols["mid"],
                                                  int(n_all), int(nt_all), int(n_anchors), int(dim_padded), int(nn), int(nn_search),
                                                  float(p_work), rows64, int(n_data), int(data_base), _ptr(idx), _ptr(dist), ctypes.byref(ev)))
        return idx, dist, ev.value

    def stream_last_rerank64(self):
        """(rows the last float64 re-rank's guard flagged, whether they were repaired against every column)."""
        a, b = _i64(), ctypes.c_int32()
        self._chk(self.lib.annchor_stream_last_rerank64(self.h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), bool(b.value)

    def stream_anchor_round(self, anchor_vec, rnd, n_anchors):
        v = _c(anchor_vec, np.float32)
        mx, arg = _dbl(), _i64()
        self._chk(self.lib.annchor_stream_anchor_round(self.h, _ptr(v), int(rnd), int(n_anchors), ctypes.byref(mx), ctypes.byref(arg)))
        return mx.value, arg.value

    def stream_get_row(self, local_idx):
        out = np.zeros(self._stream_dim, dtype=np.float32)
        self._chk(self.lib.annchor_stream_get_row(self.h, int(local_idx), _ptr(out)))
        return out

    def stream_order(self, min_tiles=0):
        ptrs = [_vp() for _ in range(6)]
        n_pad, nt, dimp = _i64(), _i32(), _i32()
        self._chk(self.lib.annchor_stream_order(self.h, int(min_tiles), *[ctypes.byref(p) for p in ptrs], ctypes.byref(n_pad),
                                                ctypes.byref(nt), ctypes.byref(dimp)))
        names = ("Xs", "rs", "perm", "lo", "hi", "mid")
        return {k: p.value for k, p in zip(names, ptrs)}, n_pad.value, nt.value, dimp.value

    def stream_order_begin(self, min_tiles, tile_begin, tile_count):
        """The level sorts of the k-d order restricted to the caller's tile range; (device pointer of its slice of the order,
        the all-gather target, bytes per rank)."""
        ol, oa, nb = _vp(), _vp(), _i64()
        self._chk(self.lib.annchor_stream_order_begin(self.h, int(min_tiles), int(tile_begin), int(tile_count), ctypes.byref(ol), ctypes.byref(oa),
                                                      ctypes.byref(nb)))
        return ol.value, oa.value, nb.value

    def stream_order_end(self):
        ptrs = [_vp() for _ in range(6)]
        n_pad, nt, dimp = _i64(), _i32(), _i32()
        self._chk(self.lib.annchor_stream_order_end(self.h, *[ctypes.byref(p) for p in ptrs], ctypes.byref(n_pad), ctypes.byref(nt),
                                                    ctypes.byref(dimp)))
        names = ("Xs", "rs", "perm", "lo", "hi", "mid")
        return {k: p.value for k, p in zip(names, ptrs)}, n_pad.value, nt.value, dimp.value

    def stream_knn(self, ptrs, n_all, nt_all, n_anchors, dim_padded, tile_begin, tile_count, k, p_work, n_local=None, join_passes=0, join_extra=0,
                   out=None, fetch=True):
        """n_local given: graph rows come back in the bound shard's own row order ([n_local, k],
        row_ids is None); otherwise in tile order with row_ids (global id per row, -1 = padding).  out: GraphBuffers.
        fetch=False: the graph stays on the device for stream_rerank64; returns the tile evaluations alone."""
        rows = tile_count * 128 if n_local is None else int(n_local)
        row_ids = np.zeros(rows, dtype=np.int64) if n_local is None else None
        ev = _i64()
        self._chk(self.lib.annchor_stream_knn_run(self.h, ptrs["Xs"], ptrs["rs"], ptrs["perm"], ptrs["lo"], ptrs["hi"], ptrs["mid"], int(n_all),
                                                  int(nt_all), int(n_anchors), int(dim_padded), int(tile_begin), int(tile_count),
                                                  int(k), float(p_work), int(join_passes), int(join_extra), ctypes.byref(ev)))
        if not fetch:
            return ev.value
        # (the result arrays only now: at N = 8 x 10^6 the helper thread needs longer for its 1.9 GB than the anchor rounds and
        # the ordering take)
        if out is not None:
            idx, dist = out.take(rows, k)
        else:
            idx = np.empty((rows, k), dtype=np.int64)
            dist = np.empty((rows, k), dtype=np.float64)
        self._chk(self.lib.annchor_stream_knn_fetch(self.h, _ptr(row_ids) if row_ids is not None else None, _ptr(idx), _ptr(dist)))
        return row_ids, idx, dist, ev.value

    def stream_knn_begin(self, ptrs, n_all, nt_all, n_anchors, dim_padded, tile_begin, tile_count, k, tile_budget):
        """Tile phase of a row-sharded build (tile_budget column tiles per row tile: stream_budget);
        returns (device pointer, bytes) of this rank's lists."""
        lp, nb = _vp(), _i64()
        self._chk(self.lib.annchor_stream_knn_begin(self.h, ptrs["Xs"], ptrs["rs"], ptrs["perm"], ptrs["lo"], ptrs["hi"], ptrs["mid"],
                                                    int(n_all), int(nt_all), int(n_anchors), int(dim_padded), int(tile_begin),
                                                    int(tile_count), int(k), int(tile_budget), ctypes.byref(lp), ctypes.byref(nb)))
        self._knn_shape = (int(tile_count), int(k))
        return lp.value, nb.value

    def stream_knn_join(self, lists_all, per_pass):
        """One join pass against the all-gathered lists; returns (device pointer of the new local lists,
        list entries the pass replaced)."""
        lp, upd = _vp(), _i64()
        self._chk(self.lib.annchor_stream_knn_join(self.h, lists_all, int(per_pass), ctypes.byref(lp), ctypes.byref(upd)))
        return lp.value, upd.value

    def stream_join_rev_begin(self, lists_all):
        """Reverse neighbour lists of this rank's columns from the all-gathered lists; (device pointer of the slice, the gather target, bytes per rank)."""
        rl, ra, nb = _vp(), _vp(), _i64()
        self._chk(self.lib.annchor_stream_join_rev_begin(self.h, lists_all, ctypes.byref(rl), ctypes.byref(ra), ctypes.byref(nb)))
        return rl.value, ra.value, nb.value

    def stream_knn_end(self, n_local=None):
        tile_count, k = self._knn_shape
        rows = tile_count * 128 if n_local is None else int(n_local)
        row_ids = np.zeros(rows, dtype=np.int64) if n_local is None else None
        idx = np.empty((rows, k), dtype=np.int64)
        dist = np.empty((rows, k), dtype=np.float64)
        ev = _i64()
        self._chk(self.lib.annchor_stream_knn_end(self.h, _ptr(row_ids) if row_ids is not None else None, _ptr(idx), _ptr(dist),
                                                  ctypes.byref(ev)))
        return row_ids, idx, dist, ev.value

    # ---- row-sharded builds: device-resident exchange buffers (include/annchor_hip.h, csrc/sharded.hip)
    def hip_stream(self):
        """The context's hipStream_t (an integer address): collectives are ordered on it."""
        p = _vp()
        self._chk(self.lib.annchor_stream_hip_stream(self.h, ctypes.byref(p)))
        return p.value or 0

    def stream_anchor_begin(self, n_anchors, first_global, world=1):
        """(candidate pointer, gathered pointer, bytes per candidate): this rank's candidate record for the first anchor
        and the all-gather target of the rounds (device memory)."""
        p, g, nb = _vp(), _vp(), _i64()
        self._chk(self.lib.annchor_stream_anchor_begin(self.h, int(n_anchors), int(first_global), int(world), ctypes.byref(p), ctypes.byref(g),
                                                       ctypes.byref(nb)))
        return p.value, g.value, nb.value

    def stream_anchor_step(self, gathered, world, rnd):
        self._chk(self.lib.annchor_stream_anchor_step(self.h, gathered, int(world), int(rnd)))

    def legacy_generate_at_next_wait(self, seed, ndraws, chunk=0):
        """The legacy MT19937 stream of `seed` on this thread at the context's next host waits, `chunk` words per wait (returns at once)."""
        if 0 <= seed < 2 ** 32 and 0 < ndraws <= LEGACY_EAGER_MAX_DRAWS:
            self._chk(self.lib.annchor_legacy_generate_at_next_wait(self.h, int(seed), int(ndraws), int(chunk)))

    def stream_anchor_rounds(self, n_anchors):
        """All max-min rounds in one call (collectives from inside the library when the context has a communicator)."""
        self._chk(self.lib.annchor_stream_anchor_rounds(self.h, int(n_anchors)))

    # ---- in-library RCCL (csrc/comm.hip)
    def comm_init(self, unique_id, world, rank):
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        self._chk(self.lib.annchor_comm_init(self.h, buf, int(world), int(rank)))

    def comm_destroy(self):
        self._chk(self.lib.annchor_comm_destroy(self.h))

    def comm_set_timeout(self, seconds):
        self._chk(self.lib.annchor_comm_set_timeout(self.h, float(seconds)))

    def comm_preflight(self, seconds=60.0):
        self._chk(self.lib.annchor_comm_preflight(self.h, float(seconds)))

    def comm_init_side(self, unique_id):
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        self._chk(self.lib.annchor_comm_init_side(self.h, buf))

    def comm_allgather_begin(self, send, recv, nbytes):
        self._chk(self.lib.annchor_comm_allgather_begin(self.h, send, recv, int(nbytes)))

    def comm_side_join(self):
        self._chk(self.lib.annchor_comm_side_join(self.h))

    def comm_allgather(self, send, recv, nbytes):
        self._chk(self.lib.annchor_comm_allgather(self.h, send, recv, int(nbytes)))

    def comm_alltoall_records(self, send, send_counts, recv, recv_counts, words):
        sc, rc = _c(send_counts, np.int64), _c(recv_counts, np.int64)
        self._chk(self.lib.annchor_comm_alltoall_records(self.h, send, _ptr(sc), recv, _ptr(rc), int(words)))

    def stream_anchor_end(self, n_anchors):
        A = np.empty(int(n_anchors), dtype=np.int64)
        V = np.empty((int(n_anchors), self._stream_dim), dtype=np.float32)
        self._chk(self.lib.annchor_stream_anchor_end(self.h, _ptr(A), _ptr(V)))
        return A, V

    def stream_rows_begin(self, counts):
        counts = _c(counts, np.int64)
        s, r, nb = _vp(), _vp(), _i64()
        self._chk(self.lib.annchor_stream_rows_begin(self.h, len(counts), _ptr(counts), ctypes.byref(s), ctypes.byref(r), ctypes.byref(nb)))
        return s.value, r.value, nb.value

    def stream_anchor_dists_begin(self, counts):
        """Send / receive buffers and bytes per rank of the all-gather of the ranks' own anchor distances."""
        counts = _c(counts, np.int64)
        s, r, nb = _vp(), _vp(), _i64()
        self._chk(self.lib.annchor_stream_anchor_dists_begin(self.h, len(counts), _ptr(counts), ctypes.byref(s), ctypes.byref(r),
                                                             ctypes.byref(nb)))
        return s.value, r.value, nb.value

    def stream_rows_end(self, counts):
        counts = _c(counts, np.int64)
        self._chk(self.lib.annchor_stream_rows_end(self.h, len(counts), _ptr(counts)))
        self.nx = int(counts.sum())

    def stream_lists_all(self, world, bytes_per_rank):
        p = _vp()
        self._chk(self.lib.annchor_stream_lists_all(self.h, int(world), int(bytes_per_rank), ctypes.byref(p)))
        return p.value

    def stream_route_begin(self, starts, bases):
        """Finish the build begun with stream_knn_begin; (send pointer, records per destination rank, int64 words per
        record, tile evaluations)."""
        starts, bases = _c(starts, np.int64), _c(bases, np.int64)
        world = len(bases)
        send, words, ev = _vp(), _i64(), _i64()
        counts = np.zeros(world, dtype=np.int64)
        self._chk(self.lib.annchor_stream_route_begin(self.h, world, _ptr(starts), _ptr(bases), ctypes.byref(send), _ptr(counts),
                                                      ctypes.byref(words), ctypes.byref(ev)))
        return send.value, counts, words.value, ev.value

    def stream_route_recv(self, n_recv):
        p = _vp()
        self._chk(self.lib.annchor_stream_route_recv(self.h, int(n_recv), ctypes.byref(p)))
        return p.value

    def stream_route_end(self, n_recv, rows_padded, n_own, k, out=None):
        if out is not None:
            idx, dist = out.take(n_own, k)
        else:
            idx = np.empty((int(n_own), int(k)), dtype=np.int64)
            dist = np.empty((int(n_own), int(k)), dtype=np.float64)
        self._chk(self.lib.annchor_stream_route_end(self.h, int(n_recv), int(rows_padded), _ptr(idx), _ptr(dist)))
        return idx, dist

    def stream_graph_device(self):
        """(idx pointer, dist pointer, rows_padded, k) of the graph rows stream_route_end left on the device."""
        pi, pd, rows, k = _vp(), _vp(), _i64(), _i32()
        self._chk(self.lib.annchor_stream_graph_device(self.h, ctypes.byref(pi), ctypes.byref(pd), ctypes.byref(rows), ctypes.byref(k)))
        return pi.value, pd.value, rows.value, k.value

    def stream_query(self, cols, n_all, nt_all, n_anchors, dim_padded, nn, p_work):
        """nn nearest data rows of every (bound + ordered) query row; cols = the data set's column arrays."""
        idx = np.empty((self.nx, nn), dtype=np.int64)
        dist = np.empty((self.nx, nn), dtype=np.float64)
        ev = _i64()
        self._chk(self.lib.annchor_stream_query(self.h, cols["Xs"], cols["rs"], cols["perm"], cols["lo"], cols["hi"], cols["mid"],
                                                int(n_all), int(nt_all), int(n_anchors), int(dim_padded), int(nn), float(p_work),
                                                _ptr(idx), _ptr(dist), ctypes.byref(ev)))
        return idx, dist, ev.value

    def stream_order_classes(self, codes, n_classes, anchor_vectors=None):
        """Class-pure tiles of the (bound, anchor-swept) rows: k-d order, stably sorted by label code, every class padded to whole
        tiles.  codes: int32 label codes 0 .. n_classes - 1; anchor_vectors [n_anchors, dim]: centre of the fp16 split copy.
        Returns (n_pad, n_tiles, dim_padded) of the class-padded order."""
        codes = _c(codes, np.int32)
        if codes.shape != (self.nx,):
            raise ValueError("one label code per bound row")
        av = _c(anchor_vectors, np.float32) if anchor_vectors is not None else None
        n_pad, nt, dimp = _i64(), _i32(), _i32()
        self._chk(self.lib.annchor_stream_order_classes(self.h, _ptr(codes), int(n_classes), _ptr(av), ctypes.byref(n_pad), ctypes.byref(nt),
                                                        ctypes.byref(dimp)))
        return n_pad.value, nt.value, dimp.value

    def stream_enemies(self, nn, p_work):
        """nn nearest rows of another label of every row (after stream_order_classes): (idx int64 [n, nn], dist float64 [n, nn],
        tile evaluations)."""
        idx = np.empty((self.nx, nn), dtype=np.int64)
        dist = np.empty((self.nx, nn), dtype=np.float64)
        ev = _i64()
        self._chk(self.lib.annchor_stream_enemies(self.h, int(nn), float(p_work), _ptr(idx), _ptr(dist), ctypes.byref(ev)))
        return idx, dist, ev.value

    def stream_last_counts(self):
        """(tile evaluations of the tile phase, 128-column runs of the join passes) of the last build."""
        a, b = _i64(), _i64()
        self._chk(self.lib.annchor_stream_last_counts(self.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def stream_last_kernel(self, with_guard=False):
        """Kernel of the last build's tile phase: 0 exact float32 tile GEMMs, 1 split-fp16; with_guard: also the number of
        rows the split kernel flagged as ill-conditioned (more than 1 in 200 repeats the tile phase on the exact kernel)."""
        k, g = ctypes.c_int32(), _i64()
        self._chk(self.lib.annchor_stream_last_kernel(self.h, ctypes.byref(k), ctypes.byref(g)))
        return (int(k.value), int(g.value)) if with_guard else int(k.value)

    def stream_last_tile_kernels(self):
        """(two_stage, repaired) of the last build's tile phase: k_st_knnh ran behind the warm-up; flagged rows were repaired exactly."""
        a, b = ctypes.c_int32(), ctypes.c_int32()
        self._chk(self.lib.annchor_stream_last_tile_kernels(self.h, ctypes.byref(a), ctypes.byref(b)))
        return bool(a.value), bool(b.value)

    def stream_join_tables(self, gathered, world, n_anchors, n_tiles, joined):
        self._chk(self.lib.annchor_stream_join_tables(self.h, gathered, int(world), int(n_anchors), int(n_tiles), joined))

    def device_alloc(self, nbytes):
        p = _vp()
        self._chk(self.lib.annchor_device_alloc(self.h, int(nbytes), ctypes.byref(p)))
        return p.value

    def device_free(self, dptr):
        self._chk(self.lib.annchor_device_free(self.h, dptr))

    def device_copy(self, dst, src, nbytes, kind):
        self._chk(self.lib.annchor_device_copy(self.h, dst, src, int(nbytes), {"h2d": 1, "d2h": 2, "d2d": 3}[kind]))

    # ---- nearest enemies (csrc/enemies.hip)
    def enemies_candidates(self, codes, loc_thresh, loc_min):
        codes = _c(codes, np.int32)
        n = _i64()
        self._chk(self.lib.annchor_enemies_candidates(self.h, _ptr(codes), int(loc_thresh), int(loc_min), ctypes.byref(n)))
        self._n_enemy_pairs = n.value
        return n.value

    def enemies_predict(self, bins=None, W=None, c=None, pred=None):
        if pred is not None:
            pred = _c(pred, np.float64).reshape(-1)
            if pred.shape[0] != self._n_enemy_pairs:
                raise ValueError("regression.predict returned %d values for %d enemy pairs" % (pred.shape[0], self._n_enemy_pairs))
            self._chk(self.lib.annchor_enemies_predict(self.h, None, 0, None, None, _ptr(pred)))
            return
        bins, W, c = _c(bins, np.float64), _c(W, np.float64), _c(c, np.float64)
        self._chk(self.lib.annchor_enemies_predict(self.h, _ptr(bins), len(bins) - 1, _ptr(W), _ptr(c), None))

    def enemies_first(self, first, nn, evaluate):
        """evaluate: the todo pairs are evaluated on the device, returns their number; otherwise returns them (int64 [m, 2])."""
        m = _i64()
        if evaluate:
            self._chk(self.lib.annchor_enemies_first(self.h, int(first), int(nn), 1, None, 0, ctypes.byref(m)))
            return m.value
        cap = self.nx * int(first)
        todo = np.empty((cap, 2), dtype=np.int64)
        self._chk(self.lib.annchor_enemies_first(self.h, int(first), int(nn), 0, _ptr(todo), cap, ctypes.byref(m)))
        return todo[:m.value]

    def enemies_set_exact(self, exact):
        exact = _c(exact, np.float64)
        self._chk(self.lib.annchor_enemies_set_exact(self.h, _ptr(exact), len(exact)))

    def enemies_graph(self, nn):
        idx = np.empty((self.nx, nn), dtype=np.int64)
        dist = np.empty((self.nx, nn), dtype=np.float64)
        self._chk(self.lib.annchor_enemies_graph(self.h, int(nn), _ptr(idx), _ptr(dist)))
        return idx, dist

    def enemies_download(self):
        """(IJs_new [n, 2], features [n, 4], RA [n], ncm bool [n], I_ptr [nx + 1], I_idx [2 n]) of the enemy pairs."""
        n = self._n_enemy_pairs
        ij, feats = np.empty((n, 2), dtype=np.int64), np.empty((n, 4), dtype=np.float64)
        RA, ncm = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.uint8)
        ptr, idx = np.empty(self.nx + 1, dtype=np.int64), np.empty(2 * n, dtype=np.int64)
        self._chk(self.lib.annchor_enemies_download(self.h, _ptr(ij), _ptr(feats), _ptr(RA), _ptr(ncm), _ptr(ptr), _ptr(idx)))
        return ij, feats, RA, ncm.astype(bool), ptr, idx

    # ---------------------------------------------------- fixed-radius graph (csrc/radius.hip)
    def radius_count(self, r, rtol, connectivity, use_bounds):
        """Per-row numbers of EVAL and SURE pairs (int64 [nx] each) of all pairs i < j; fixes (r, rtol, mode, use_bounds) for
        radius_rows."""
        row_eval = np.zeros(self.nx, dtype=np.int64)
        row_sure = np.zeros(self.nx, dtype=np.int64)
        self._chk(self.lib.annchor_radius_count(self.h, float(r), float(rtol), 1 if connectivity else 0, 1 if use_bounds else 0,
                                                _ptr(row_eval), _ptr(row_sure)))
        return row_eval, row_sure

    def radius_rows(self, row_begin, row_end, col_begin, col_end, max_pairs=0, evaluate=False):
        """(n_eval, n_sure, n_kept) of the range; n_kept = -1: more than max_pairs candidates, nothing was emitted."""
        ne, ns, nk = _i64(), _i64(), _i64()
        self._chk(self.lib.annchor_radius_rows(self.h, int(row_begin), int(row_end), int(col_begin), int(col_end), int(max_pairs),
                                               1 if evaluate else 0, ctypes.byref(ne), ctypes.byref(ns), ctypes.byref(nk)))
        return ne.value, ns.value, nk.value

    def radius_query_count(self, nx_data, r, rtol, connectivity, use_bounds):
        """The engine holds nx_data data points followed by nq queries: per-query numbers of EVAL and SURE pairs (int64 [nq]
        each) over the whole rectangle; fixes (r, rtol, mode, use_bounds) for radius_query_rows."""
        nq = max(self.nx - int(nx_data), 0)
        row_eval = np.zeros(nq, dtype=np.int64)
        row_sure = np.zeros(nq, dtype=np.int64)
        self._chk(self.lib.annchor_radius_query_count(self.h, int(nx_data), float(r), float(rtol), 1 if connectivity else 0,
                                                      1 if use_bounds else 0, _ptr(row_eval), _ptr(row_sure)))
        return row_eval, row_sure

    def radius_query_rows(self, nx_data, q_begin, q_end, col_begin, col_end, max_pairs=0, evaluate=False):
        """(n_eval, n_sure, n_kept) of the queries [q_begin, q_end) against the data columns [col_begin, col_end); n_kept = -1:
        more than max_pairs candidates, nothing was emitted.  radius_fetch then returns rows (j, nx_data + q)."""
        ne, ns, nk = _i64(), _i64(), _i64()
        self._chk(self.lib.annchor_radius_query_rows(self.h, int(nx_data), int(q_begin), int(q_end), int(col_begin), int(col_end),
                                                     int(max_pairs), 1 if evaluate else 0, ctypes.byref(ne), ctypes.byref(ns),
                                                     ctypes.byref(nk)))
        return ne.value, ns.value, nk.value

    def radius_fetch(self, which, n, distances=False):
        """List `which` (RADIUS_EVAL / RADIUS_SURE / RADIUS_KEPT) of the last radius_rows: int64 [n, 2] and, when asked, float64 [n]."""
        ij = np.zeros((int(n), 2), dtype=np.int64)
        d = np.zeros(int(n), dtype=np.float64) if distances else None
        self._chk(self.lib.annchor_radius_fetch(self.h, int(which), _ptr(ij), _ptr(d)))
        return (ij, d) if distances else ij

    # ---------------------------------------------------- DBSCAN on the radius lists (csrc/dbscan.hip)
    def dbscan_begin(self, min_samples):
        """Zero the degrees and empty the device edge list for the engine's nx points."""
        self._chk(self.lib.annchor_dbscan_begin(self.h, int(min_samples)))

    def dbscan_absorb(self):
        """Append the kept and sure pairs of the last radius_rows to the edge list, device to device; returns their number."""
        n = _i64()
        self._chk(self.lib.annchor_dbscan_absorb(self.h, ctypes.byref(n)))
        return n.value

    def dbscan_edges(self, ij):
        """Append host edges (int64 [n, 2], each unordered pair once) to the edge list."""
        ij = _c(ij, np.int64).reshape(-1, 2)
        self._chk(self.lib.annchor_dbscan_edges(self.h, _ptr(ij), len(ij)))

    def dbscan_finish(self):
        """(labels int32 [nx], core uint8 [nx], n_clusters) of the edge list as it stands."""
        labels = np.empty(self.nx, dtype=np.int32)
        core = np.empty(self.nx, dtype=np.uint8)
        n = _i64()
        self._chk(self.lib.annchor_dbscan_finish(self.h, _ptr(labels), _ptr(core), ctypes.byref(n)))
        return labels, core, n.value

    # ---------------------------------------------------- exact k-NN graph from per-row radii (csrc/knnexact.hip)
    def knn_exact_begin(self, k, u, rtol, use_bounds):
        """Upload the rows' radii (float64 [nx], >= 0, +inf: unknown), empty the entry list; returns the per-row numbers of
        EVAL pairs (int64 [nx]) of all pairs i < j and fixes (k, u, rtol, use_bounds) for knn_exact_rows."""
        u = _c(u, np.float64).reshape(-1)
        if len(u) != self.nx:
            raise ValueError("radii must be [nx=%d], got %r" % (self.nx, u.shape))
        row_eval = np.zeros(self.nx, dtype=np.int64)
        self._chk(self.lib.annchor_knn_exact_begin(self.h, int(k), _ptr(u), float(rtol), 1 if use_bounds else 0, _ptr(row_eval)))
        self._knn_exact_k = int(k)
        return row_eval

    def knn_exact_rows(self, row_begin, row_end, col_begin, col_end, max_pairs=0, evaluate=False):
        """(n_eval, n_entries) of the range; n_entries = -1: more than max_pairs candidates, nothing was emitted.  evaluate: the
        device metric runs on the candidates and they are absorbed (n_entries: the directed entries added)."""
        ne, nn = _i64(), _i64()
        self._chk(self.lib.annchor_knn_exact_rows(self.h, int(row_begin), int(row_end), int(col_begin), int(col_end), int(max_pairs),
                                                  1 if evaluate else 0, ctypes.byref(ne), ctypes.byref(nn)))
        return ne.value, nn.value

    def knn_exact_fetch(self, n):
        """The candidates of the last knn_exact_rows: int64 [n, 2], row-major, ascending column inside a row."""
        ij = np.zeros((int(n), 2), dtype=np.int64)
        self._chk(self.lib.annchor_knn_exact_fetch(self.h, _ptr(ij)))
        return ij

    def knn_exact_edges(self, ij, d):
        """Absorb host-evaluated candidates (int64 [n, 2], float64 [n]; each unordered pair once) under the directed tests."""
        ij, d = _c(ij, np.int64).reshape(-1, 2), _c(d, np.float64).reshape(-1)
        if len(ij) != len(d):
            raise ValueError("%d candidates with %d distances" % (len(ij), len(d)))
        self._chk(self.lib.annchor_knn_exact_edges(self.h, _ptr(ij), _ptr(d), len(ij)))

    def knn_exact_finish(self, row_cap=0):
        """(idx int64 [nx, k], dist float64 [nx, k], row_entries int64 [nx]) of the entry list as it stands.  row_cap: slots of a
        row the selection keeps in LDS (0: as many as fit)."""
        k = getattr(self, "_knn_exact_k", 1)   # (without a begin the call below is refused with the library's own message)
        idx = np.zeros((self.nx, k), dtype=np.int64)
        dist = np.zeros((self.nx, k), dtype=np.float64)
        rows = np.zeros(self.nx, dtype=np.int64)
        self._chk(self.lib.annchor_knn_exact_finish(self.h, _ptr(idx), _ptr(dist), _ptr(rows), int(row_cap)))
        return idx, dist, rows

    def graph_to_coo(self, idx, dist):
        """Symmetric COO (rows, cols, vals) of a k-NN graph, every cell once, vals = distance + eps."""
        idx, dist = _c(idx, np.int64), _c(dist, np.float64)
        nx, k = idx.shape
        rows, cols = np.empty(2 * nx * k, dtype=np.int64), np.empty(2 * nx * k, dtype=np.int64)
        vals = np.empty(2 * nx * k, dtype=np.float64)
        nnz = _i64()
        self._chk(self.lib.annchor_graph_to_coo(self.h, _ptr(idx), _ptr(dist), nx, k, _ptr(rows), _ptr(cols), _ptr(vals), ctypes.byref(nnz)))
        n = nnz.value
        return rows[:n], cols[:n], vals[:n]

    # ---------------------------------------------------------- state access
    def field_size(self, field):
        n = _i64()
        self._chk(self.lib.annchor_field_size(self.h, int(field), ctypes.byref(n)))
        return n.value

    def download(self, field):
        n = self.field_size(field)
        out = np.zeros(n, dtype=_FIELD_DTYPE[field])
        if n:
            self._chk(self.lib.annchor_download(self.h, int(field), _ptr(out), n))
        return out

    def upload(self, field, arr):
        arr = _c(arr, _FIELD_DTYPE[field]).reshape(-1)
        self._chk(self.lib.annchor_upload(self.h, int(field), _ptr(arr), arr.size))

    # ------------------------------------------------------------ profiling
    def prof_enable(self, on=True):
        """on: False/0 off, True/1 every kernel family, 2 the metric kernels only."""
        self._chk(self.lib.annchor_prof_enable(self.h, int(on)))

    def prof_reset(self):
        self._chk(self.lib.annchor_prof_reset(self.h))

    def prof_get(self):
        cap = 64
        names = (ctypes.c_char_p * cap)()
        ms = np.zeros(cap, dtype=np.float64)
        launches = np.zeros(cap, dtype=np.int64)
        alg = np.zeros(cap, dtype=np.float64)
        n = self.lib.annchor_prof_get(self.h, cap, names, _ptr(ms), _ptr(launches), _ptr(alg))
        if n < 0:
            self._chk(n)
        return {names[i].decode(): dict(ms=float(ms[i]), launches=int(launches[i]), alg_bytes=float(alg[i]))
                for i in range(n)}
