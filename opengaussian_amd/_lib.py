"""ctypes binding of libogs_hip.so (C ABI: include/ogs_raster.h, include/ogs_kmeans.h, ...).

The product path has NO CPU fallback: if the HIP library is missing or fails to load, ``lib()`` raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# OGS_LIB_PATH: another build of the same library (A-B timing of two kernel versions on one box); never a fallback
LIB_PATH = os.environ.get("OGS_LIB_PATH") or os.path.join(_HERE, "lib", "libogs_hip.so")

_f32p = C.POINTER(C.c_float)
_vp = C.c_void_p


class OgsRasterFwdArgs(C.Structure):
    _fields_ = [
        ("P", C.c_int32), ("W", C.c_int32), ("H", C.c_int32), ("C", C.c_int32),
        ("sh_degree", C.c_int32), ("sh_coeffs", C.c_int32),
        ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("scale_modifier", C.c_float),
        ("prefiltered", C.c_int32), ("debug", C.c_int32),
        ("bg", _vp), ("means3D", _vp), ("colors_precomp", _vp), ("shs", _vp), ("opacities", _vp),
        ("scales", _vp), ("rotations", _vp), ("cov3D_precomp", _vp),
        ("viewmatrix", _vp), ("projmatrix", _vp), ("campos", _vp),
        ("out_color", _vp), ("out_depth", _vp), ("out_alpha", _vp), ("radii", _vp),
        ("geom_buffer", _vp), ("geom_tmp", _vp), ("image_buffer", _vp), ("point_list", _vp),
        ("binning_tmp", _vp), ("sorted_rec", _vp), ("quad_list", _vp), ("group_ids", _vp), ("num_groups", C.c_int32),
        ("full_binning", C.c_int32),
        ("bwd_clear", _vp), ("bwd_clear_bytes", C.c_size_t),
    ]


class OgsRasterBwdArgs(C.Structure):
    _fields_ = [
        ("P", C.c_int32), ("W", C.c_int32), ("H", C.c_int32), ("C", C.c_int32),
        ("sh_degree", C.c_int32), ("sh_coeffs", C.c_int32),
        ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("scale_modifier", C.c_float),
        ("debug", C.c_int32), ("num_rendered", C.c_int32), ("geom_channels", C.c_int32),
        ("bg", _vp), ("means3D", _vp), ("colors_precomp", _vp), ("shs", _vp), ("opacities", _vp),
        ("scales", _vp), ("rotations", _vp), ("cov3D_precomp", _vp),
        ("viewmatrix", _vp), ("projmatrix", _vp), ("campos", _vp),
        ("radii", _vp), ("out_alpha", _vp), ("dL_dcolor", _vp), ("dL_ddepth", _vp), ("dL_dalpha", _vp),
        ("geom_buffer", _vp), ("image_buffer", _vp), ("point_list", _vp), ("sorted_rec", _vp), ("quad_list", _vp), ("bwd_tmp", _vp),
        ("dL_dmeans2D", _vp), ("dL_dcolors", _vp), ("dL_dopacity", _vp), ("dL_dmeans3D", _vp),
        ("dL_dcov3D", _vp), ("dL_dsh", _vp), ("dL_dscales", _vp), ("dL_drotations", _vp), ("num_groups", C.c_int32), ("dL_dsh_rgb", _vp),
        ("bwd_tmp_is_clear", C.c_int32),
        ("dL_dviewmatrix", _vp), ("dL_dprojmatrix", _vp), ("dL_dcampos", _vp), ("pose_tmp", _vp),
    ]


class OgsAdamTensor(C.Structure):
    _fields_ = [("param", _vp), ("grad", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp), ("numel", C.c_int64),
                ("lr", C.c_double), ("step", C.c_int64)]


class OgsRowTensor(C.Structure):
    _fields_ = [("src", _vp), ("dst", _vp), ("width", C.c_int32), ("zero_new", C.c_int32)]


class OgsDensifyArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("grad_accum", _vp), ("denom", _vp), ("scaling", _vp), ("opacity", _vp),
                ("max_grad", C.c_float), ("min_opacity", C.c_float), ("extent", C.c_float), ("percent_dense", C.c_float),
                ("prune_world_size", C.c_int32)]


class OgsGroupStatsArgs(C.Structure):
    _fields_ = [("labels", _vp), ("num_labels", C.c_int32), ("alpha_threshold", C.c_float), ("max_alpha", _vp),
                ("count", _vp), ("feat_sum", _vp), ("stats_tmp", _vp)]


class OgsLabelMapArgs(C.Structure):
    """include/ogs_query.h: labels in, the four [H, W] maps out."""
    _fields_ = [("labels", _vp), ("num_labels", C.c_int32), ("out_label", _vp), ("out_weight", _vp), ("out_second", _vp),
                ("out_alpha", _vp)]


class OgsLabelVotesArgs(C.Structure):
    """include/ogs_query.h: a label image in, the [R, L + 1] fixed-point table accumulated into."""
    _fields_ = [("pixel_labels", _vp), ("num_labels", C.c_int32), ("rows", _vp), ("num_rows", C.c_int32), ("votes", _vp)]


class OgsFeatureVotesArgs(C.Structure):
    """include/ogs_query.h: a feature image in, the [R, D + 1] fixed-point table accumulated into."""
    _fields_ = [("features", _vp), ("num_channels", C.c_int32), ("valid", _vp), ("rows", _vp), ("num_rows", C.c_int32),
                ("votes", _vp)]


class OgsFeatureMapArgs(C.Structure):
    """include/ogs_query.h: a feature table [R, D] in, the rendered map (and the alpha) out."""
    _fields_ = [("features", _vp), ("num_channels", C.c_int32), ("rows", _vp), ("num_rows", C.c_int32),
                ("channels_last", C.c_int32), ("out_map", _vp), ("out_alpha", _vp)]


class OgsRawModel(C.Structure):
    """include/ogs_model.h: the reference model's raw parameters."""
    _fields_ = [("features_dc", _vp), ("features_rest", _vp), ("scaling", _vp), ("rotation", _vp), ("opacity", _vp)]


class OgsRawModelGrads(C.Structure):
    _fields_ = [("features_dc", _vp), ("features_rest", _vp), ("scaling", _vp), ("rotation", _vp), ("opacity", _vp)]


# name -> (restype, argtypes); also the list the symbol-export test checks against the headers
SIGNATURES = {
    "ogs_version": (C.c_int, []),
    "ogs_last_error": (C.c_char_p, []),
    "ogs_raster_geom_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "ogs_raster_geom_tmp_bytes": (C.c_size_t, [C.c_int32]),
    "ogs_raster_image_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "ogs_raster_image_bytes_grouped": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "ogs_raster_binning_tmp_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "ogs_raster_backward_tmp_bytes": (C.c_size_t, [C.c_int32]),
    "ogs_raster_backward_pose_tmp_bytes": (C.c_size_t, [C.c_int32]),
    "ogs_pose_partial_chunk": (C.c_int, []),
    "ogs_raster_sorted_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "ogs_raster_quad_list_bytes": (C.c_size_t, [C.c_int64]),
    "ogs_raster_forward_geometry": (C.c_int, [C.POINTER(OgsRasterFwdArgs), _vp, C.POINTER(C.c_int64)]),
    "ogs_raster_forward_render": (C.c_int, [C.POINTER(OgsRasterFwdArgs), C.c_int64, _vp]),
    "ogs_raster_read_num_rendered_async": (C.c_int, [C.POINTER(OgsRasterFwdArgs), _vp, _vp]),
    "ogs_raster_forward_render_deferred": (C.c_int, [C.POINTER(OgsRasterFwdArgs), C.c_int64, _vp]),
    "ogs_raster_read_num_emitted": (C.c_int, [C.POINTER(OgsRasterFwdArgs), _vp, C.POINTER(C.c_uint32)]),
    "ogs_raster_stats_image_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "ogs_raster_stats_tmp_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "ogs_raster_forward_group_stats": (C.c_int, [C.POINTER(OgsRasterFwdArgs), C.POINTER(OgsGroupStatsArgs), C.c_int64, _vp]),
    "ogs_raster_backward": (C.c_int, [C.POINTER(OgsRasterBwdArgs), _vp]),
    "ogs_raster_tiny_max_points": (C.c_size_t, []),
    "ogs_raster_tile_sort_capacity": (C.c_size_t, [C.c_int32]),
    "ogs_raster_tile_sort_debug": (C.c_int, [C.c_int32]),
    "ogs_raster_tile_count_debug": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "ogs_raster_tile_count_trip": (C.c_size_t, []),
    "ogs_raster_tile_place_debug": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "ogs_raster_forward_tiny": (C.c_int, [C.POINTER(OgsRasterFwdArgs), _vp]),
    "ogs_raster_forward_reblend": (C.c_int, [C.POINTER(OgsRasterFwdArgs), _vp]),
    "ogs_raster_compact_kept": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ogs_mark_visible": (C.c_int, [C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "ogs_sh_grad_from_views": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "ogs_raster_export_binning": (C.c_int, [C.POINTER(OgsRasterFwdArgs), C.c_int64, _vp, _vp, _vp, _vp]),
    "ogs_selftest_wave_fold16": (C.c_int, [_vp, _vp, _vp]),
    "ogs_selftest_mfma_rank1": (C.c_int, [_vp, _vp, _vp, C.c_int32, _vp, _vp, _vp]),
    "ogs_selftest_tile_order": (C.c_int, [_vp, C.c_int64, _vp, _vp]),
    "ogs_selftest_radix_tmp_bytes": (C.c_size_t, [C.c_int64]),
    "ogs_selftest_radix_sort": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]),
    "ogs_selftest_scan_tmp_bytes": (C.c_size_t, [C.c_int64]),
    "ogs_selftest_scan_u32": (C.c_int, [_vp, _vp, _vp, C.c_int64, _vp, _vp, _vp, _vp]),
    "ogs_raster_forward_geometry_raw": (C.c_int, [C.POINTER(OgsRasterFwdArgs), C.POINTER(OgsRawModel), _vp,
                                                  C.POINTER(C.c_int64)]),
    "ogs_raster_forward_tiny_raw": (C.c_int, [C.POINTER(OgsRasterFwdArgs), C.POINTER(OgsRawModel), _vp]),
    "ogs_raster_backward_raw": (C.c_int, [C.POINTER(OgsRasterBwdArgs), C.POINTER(OgsRawModel), C.POINTER(OgsRawModelGrads), _vp]),
    "ogs_model_activate": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(OgsRawModel), _vp, _vp, _vp, _vp, _vp]),
    "ogs_check_async_status": (C.c_int, []),
    "ogs_prof_enable": (C.c_int, [C.c_int]),
    "ogs_prof_filter": (C.c_int, [C.c_char_p]),
    "ogs_prof_collect": (C.c_int, [C.c_char_p, C.c_size_t]),
    "ogs_kmeans_tmp_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "ogs_kmeans_lloyd": (C.c_int, [_vp, C.c_int64, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                   _vp, C.c_int64, _vp, _vp]),
    "ogs_kmeans_assign": (C.c_int, [_vp, C.c_int64, C.c_int32, _vp, C.c_int32, _vp, C.c_int64, _vp]),
    "ogs_mask_feature_sums": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _vp, _vp]),
    "ogs_mask_feature_sqdev": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int64, _vp, _vp]),
    "ogs_mask_feature_sums_backward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int64, _vp, _vp, _vp]),
    "ogs_mask_cohesion": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int64, _vp, _vp]),
    "ogs_mask_cohesion_backward": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int64, _vp, _vp, _vp]),
    "ogs_label_feature_sums": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _vp, _vp]),
    "ogs_label_feature_sqdev": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int64, _vp, _vp]),
    "ogs_label_feature_sums_backward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int64, _vp, _vp, _vp]),
    "ogs_label_cohesion": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int64, _vp, _vp]),
    "ogs_label_cohesion_backward": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int64, _vp, _vp, _vp]),
    "ogs_separation_loss": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]),
    "ogs_adam_step": (C.c_int, [C.POINTER(OgsAdamTensor), C.c_int32, C.c_double, C.c_double, C.c_double, _vp]),
    "ogs_rows_gather": (C.c_int, [C.POINTER(OgsRowTensor), C.c_int32, _vp, _vp, C.c_int64, _vp]),
    "ogs_densify_tmp_bytes": (C.c_size_t, [C.c_int32]),
    "ogs_densify_plan": (C.c_int, [C.POINTER(OgsDensifyArgs), _vp, C.POINTER(C.c_uint32), _vp]),
    "ogs_densify_map": (C.c_int, [C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "ogs_densify_split_children": (C.c_int, [C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ogs_densify_stats": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ogs_kmeans_accumulate": (C.c_int, [_vp, C.c_int64, C.c_int32, _vp, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "ogs_kmeans_update": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "ogs_kmeans_gather": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, _vp, _vp]),
    "ogs_refine_wave_table_capacity": (C.c_size_t, []),
    "ogs_refine_wave_max_pixels": (C.c_size_t, []),
    "ogs_refine_block_scratch_words": (C.c_size_t, [C.c_int32]),
    "ogs_refine_visibility": (C.c_int, [C.c_int32, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_float, C.c_float, _vp,
                                        C.c_float, C.c_float, _vp, _vp]),
    "ogs_refine_footprint_labels": (C.c_int, [C.c_int32, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp,
                                              _vp]),
    "ogs_refine_footprint_labels_block": (C.c_int, [C.c_int32, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _vp,
                                                    _vp, _vp, _vp]),
    "ogs_refine_vote": (C.c_int, [C.c_int64, C.c_int32, _vp, _vp, _vp]),
    "ogs_refine_expand": (C.c_int, [C.c_int32, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp,
                                    C.c_int32, _vp]),
    "ogs_refine_finalize": (C.c_int, [C.c_int64, C.c_int32, _vp, _vp, _vp, C.c_int32, C.c_float, _vp, _vp]),
    "ogs_loss_photometric_tmp_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "ogs_loss_photometric_forward": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_float, _vp, _vp, _vp]),
    "ogs_loss_photometric_backward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_float, C.c_int32, C.c_int32, C.c_int32, _vp,
                                                _vp]),
    "ogs_loss_masked_tmp_bytes": (C.c_size_t, []),
    "ogs_loss_masked_forward": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _vp, _vp, _vp]),
    "ogs_loss_masked_backward": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _vp, _vp, _vp,
                                           _vp]),
    "ogs_knn_tile_points": (C.c_size_t, []),
    "ogs_knn_group_ksum": (C.c_int, [C.c_int64, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ogs_knn_box_points": (C.c_size_t, []),
    "ogs_knn_max_k": (C.c_size_t, []),
    "ogs_knn_neighbors_tmp_bytes": (C.c_size_t, [C.c_int64]),
    "ogs_knn_neighbors": (C.c_int, [C.c_int64, _vp, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_size_t, _vp]),
    "ogs_knn_index_bytes": (C.c_size_t, [C.c_int64]),
    "ogs_knn_index_build_tmp_bytes": (C.c_size_t, [C.c_int64]),
    "ogs_knn_index_build": (C.c_int, [C.c_int64, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp]),
    "ogs_knn_query_tmp_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "ogs_knn_query": (C.c_int, [C.c_int64, _vp, C.c_int64, _vp, C.c_int32, _vp, _vp, _vp, C.c_size_t, _vp]),
    "ogs_knn_aggregate": (C.c_int, [C.c_int64, C.c_int32, C.c_int64, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "ogs_knn_transpose_chunk": (C.c_size_t, []),
    "ogs_knn_transpose_tmp_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int64]),
    "ogs_knn_transpose": (C.c_int, [C.c_int64, C.c_int32, C.c_int64, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "ogs_knn_aggregate_t_tmp_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int64, C.c_int32]),
    "ogs_knn_aggregate_t": (C.c_int, [C.c_int64, C.c_int32, C.c_int64, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t,
                                      _vp]),
    "ogs_knn_edge_dots": (C.c_int, [C.c_int64, C.c_int32, C.c_int64, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "ogs_knn_smoothness_fwd_tmp_bytes": (C.c_size_t, [C.c_int64]),
    "ogs_knn_smoothness_fwd": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "ogs_knn_smoothness_bwd_tmp_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "ogs_knn_smoothness_bwd": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                         C.c_size_t, _vp]),
    "ogs_knn_components_tmp_bytes": (C.c_size_t, [C.c_int64]),
    "ogs_knn_components": (C.c_int, [C.c_int64, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "ogs_knn_radius_count_tmp_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "ogs_knn_radius_count": (C.c_int, [C.c_int64, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "ogs_knn_dbscan_tmp_bytes": (C.c_size_t, [C.c_int64]),
    "ogs_knn_dbscan": (C.c_int, [C.c_int64, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "ogs_kmeans_wide_row_tile": (C.c_size_t, []),
    "ogs_kmeans_wide_centre_tile": (C.c_size_t, []),
    "ogs_kmeans_wide_dim_step": (C.c_size_t, []),
    "ogs_kmeans_wide_stage": (C.c_size_t, []),
    "ogs_kmeans_wide_max_dim": (C.c_size_t, []),
    "ogs_kmeans_wide_max_k": (C.c_size_t, []),
    "ogs_kmeans_wide_tmp_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "ogs_kmeans_wide_assign": (C.c_int, [_vp, C.c_int64, C.c_int32, _vp, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_size_t, _vp]),
    "ogs_kmeans_wide_update": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, _vp, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_size_t,
                                         _vp]),
    "ogs_kmeans_wide_inertia": (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, C.c_size_t, _vp]),
    "ogs_kmeans_wide_lloyd": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp,
                                        _vp, C.c_size_t, _vp]),
    "ogs_kmeans_wide_seed_rows": (C.c_size_t, []),
    "ogs_kmeans_wide_seed_tmp_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "ogs_kmeans_wide_seed": (C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, _vp, _vp, _vp, _vp,
                                       _vp, _vp, C.c_size_t, _vp]),
    "ogs_query_max_leaves": (C.c_size_t, []),
    "ogs_query_max_top": (C.c_size_t, []),
    "ogs_query_max_classes": (C.c_size_t, []),
    "ogs_query_confusion_block": (C.c_size_t, []),
    "ogs_query_split_block": (C.c_size_t, []),
    "ogs_query_split_tmp_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "ogs_query_select": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, C.c_int32, C.c_float, C.c_float,
                                   C.c_int32, _vp, _vp, _vp, _vp]),
    "ogs_query_classify": (C.c_int, [C.c_int64, _vp, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]),
    "ogs_query_confusion": (C.c_int, [C.c_int64, _vp, _vp, _vp, C.c_int32, _vp, _vp]),
    "ogs_query_split_count": (C.c_int, [C.c_int64, _vp, C.c_int32, _vp, _vp, C.c_int32, _vp, _vp]),
    "ogs_query_split_scan": (C.c_int, [C.c_int64, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "ogs_query_split_scatter": (C.c_int, [C.c_int64, _vp, C.c_int32, _vp, _vp, C.c_int32, _vp, _vp, _vp, C.c_int64, _vp]),
    "ogs_raster_label_map": (C.c_int, [C.POINTER(OgsRasterFwdArgs), C.POINTER(OgsLabelMapArgs), _vp]),
    "ogs_label_map_tile_capacity": (C.c_size_t, []),
    "ogs_raster_label_votes": (C.c_int, [C.POINTER(OgsRasterFwdArgs), C.POINTER(OgsLabelVotesArgs), _vp]),
    "ogs_label_votes_quadrant_capacity": (C.c_size_t, []),
    "ogs_label_votes_fold_columns": (C.c_size_t, []),
    "ogs_raster_feature_votes": (C.c_int, [C.POINTER(OgsRasterFwdArgs), C.POINTER(OgsFeatureVotesArgs), _vp]),
    "ogs_feature_votes_fold_columns": (C.c_size_t, []),
    "ogs_feature_votes_block_columns": (C.c_size_t, []),
    "ogs_raster_feature_map": (C.c_int, [C.POINTER(OgsRasterFwdArgs), C.POINTER(OgsFeatureMapArgs), _vp]),
    "ogs_feature_map_fold_columns": (C.c_size_t, []),
    "ogs_feature_map_block_columns": (C.c_size_t, []),
}

_lib = None


class OgsError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load libogs_hip.so once.  Raises (loudly) when it is missing: there is no CPU fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OgsError(f"{LIB_PATH} not found -- build it with `python -m opengaussian_amd.build` "
                           "(the product path has no CPU fallback)")
        # torch first: its wheel carries a HIP runtime of its own (soname libamdhip64.so.7, which satisfies this library's
        # NEEDED entry once it is loaded).  Loaded the other way round the process ends up with TWO runtimes, and the one that
        # initialises second finds no device -- build() followed by smoke() in one process did that.
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        raise OgsError(f"{what} failed (code {rc}): {lib().ogs_last_error().decode()}")


def prof_filter(prefix: str):
    """mode 2 of prof_enable brackets the kernels whose name starts with `prefix` (default "blend_")."""
    check(lib().ogs_prof_filter(prefix.encode()), "ogs_prof_filter")


def prof_enable(mode):
    """0/False: off, 1/True: every launch, 2: only the blend kernels (cheap enough for a timed region)."""
    check(lib().ogs_prof_enable(int(mode)), "ogs_prof_enable")


def prof_collect() -> dict:
    """{kernel name: {"calls": n, "total_ms": t}} for launches since prof_enable(True)."""
    import json
    buf = C.create_string_buffer(1 << 16)
    check(lib().ogs_prof_collect(buf, len(buf)), "ogs_prof_collect")
    return json.loads(buf.value.decode())


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else t.data_ptr()


def mark_written(*tensors):
    """Tell torch that a kernel wrote these tensors through their raw pointers: bump each one's version counter, as an in-place
    torch op would.  The counter is shared by a tensor, its ``detach()`` aliases and its views, so everything keyed on
    ``(data_ptr, _version)`` -- the kept passes and images, the tiled background, ``CameraPose`` -- and autograd's saved-tensor
    check see the write.  Every public call that writes a caller-visible tensor through ``data_ptr()`` calls this after it has
    enqueued its launches, for exactly the tensors it wrote (DESIGN.md section 3b lists them).  Host bookkeeping only: no
    launch, no synchronisation.  ``None`` entries are skipped; leaves that require grad are fine, in either grad mode."""
    import torch
    written = [t for t in tensors if t is not None]
    if written:
        with torch.no_grad():
            torch.autograd.graph.increment_version(written)
