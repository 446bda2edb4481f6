"""The C ABI of libpings_hip.so, declared once for ctypes: a mirror of include/pings_hip.h and nothing else.

`_lib.lib()` applies `SIGNATURES` when it loads the library and refuses a library whose `pings_abi_version()` is not
`ABI_VERSION`.  tests/test_abi.py checks every name, type, struct layout and constant here against the header, so a
change of the header is made here in the same commit.
"""
from __future__ import annotations

import ctypes as C

ABI_VERSION = 11                                                  # PINGS_ABI_VERSION

RASTER_SURFEL, RASTER_3DGS, RASTER_2DGS = 0, 1, 2                 # PINGS_RASTER_*: pings_raster_settings.mode
HEAD_COLOR, HEAD_SEMANTIC = 0, 1                                  # PINGS_HEAD_*: pings_head_reduce mode
REG_SINGULAR, REG_ILL_CONDITIONED, REG_NONFINITE = 1, 2, 4        # PINGS_REG_*: pings_reg_solve_checked status bits
REG_F_NORMALS, REG_F_DIV_GRAD, REG_F_WEIGHTED = 1, 2, 4           # PINGS_REG_F_*: pings_reg_loop_args.flags
REG_COLOR_PHOTO, REG_COLOR_CONSIST = 1, 2                         # PINGS_REG_COLOR_*: pings_reg_color_args.mode
MC_ALLOW_DEGENERATE, MC_ASCENT = 1, 2                             # PINGS_MC_*: pings_mc_count / pings_mc_emit flags
ADAMW_MAX_JOBS, ADAMW_CHUNK = 48, 4096                            # PINGS_ADAMW_*: tensors per launch, elements per item
EVAL_VIEW_RECORD, EVAL_PAIR_RECORD = 9, 12                        # PINGS_EVAL_*_RECORD: doubles per record
EVAL_EXTENT = 1                                                   # PINGS_EVAL_EXTENT: status bit of the eval grids
MESH_SAMPLE_UNIT_BITS, MESH_SAMPLE_SUM_BITS = 32, 62              # area quantum 2^-32 m^2; F * cap <= 2^62 quanta
MESH_SAMPLE_INDEX, MESH_SAMPLE_NONFINITE, MESH_SAMPLE_AREA_CAP = 16, 32, 64   # status bits of pings_mesh_sample
LOOP_MAX_R, LOOP_MAX_S, LOOP_MAX_D = 32, 128, 16                  # PINGS_LOOP_MAX_*: limits of the pings_loop_* entries
LOOP_MAX_Q, LOOP_MAX_C = 16, 65536                                # poses / queries per call, candidates per search
LIDAR_MAX_CAMS, LIDAR_MAX_LIDARS = 8, 8                           # PINGS_LIDAR_MAX_*: cameras per launch, other LiDARs
CAMFRONT_MAX_MAPS, CAMFRONT_TILE_W, CAMFRONT_TILE_H = 32, 128, 32    # PINGS_CAMFRONT_*: maps per launch, workgroup tile
CAMFRONT_RGB_U8, CAMFRONT_RGB_F32, CAMFRONT_NORMAL, CAMFRONT_DEPTH, CAMFRONT_SKY = 0, 1, 2, 3, 4   # pings_camfront_map.kind
CAMFRONT_FIT_RECORD, CAMFRONT_MIN_FIT = 5, 100                    # doubles per fit record; no fit at this many pixels or fewer
CAMFRONT_FULL = 2                                                 # status bit of pings_camfront_voxel_average
TSDF_BLOCK = 8                                                    # PINGS_TSDF_BLOCK: voxels per block edge
TSDF_EXTENT, TSDF_TABLE_FULL = 1, 2                               # PINGS_TSDF_*: status bits of pings_tsdf_touch
TSDF_POINTS_SCALE_BITS, TSDF_POINTS_COUNT_SHIFT = 22, 44          # a scan's sample is rint(t * 2^22); count << 44 | sum
TSDF_POINTS_MAX = 1048575                                         # points per scan: the count field holds 20 bits
TSDF_SDF_POINT, TSDF_SDF_RAY = 0, 1                               # PINGS_TSDF_SDF_*: sdf_mode of pings_tsdf_points_*
PGO_PRIOR, PGO_CHAIN, PGO_LOOP = 0, 1, 2                          # PINGS_PGO_*: pings_pgo_args.kind
PGO_ST_NEAR_PI, PGO_ST_NOT_POSDEF, PGO_ST_NONFINITE, PGO_ST_CONVERGED, PGO_ST_LAMBDA_MAX = 1, 2, 4, 8, 16   # status bits
PGO_RECORD = 8                                                    # PINGS_PGO_RECORD: doubles per trial record

vp = C.c_void_p     # device pointers and the hipStream_t travel as integers (tensor.data_ptr())
i32, i64, f32, f64, sz = C.c_int, C.c_int64, C.c_float, C.c_double, C.c_size_t


# ---------------------------------------------------------------- struct mirrors: pings_<snake_case of the class name>
class RasterSettings(C.Structure):
    _fields_ = [
        ("image_height", C.c_int32), ("image_width", C.c_int32),
        ("mode", C.c_int32), ("front_only", C.c_int32),
        ("tanfovx", C.c_double), ("tanfovy", C.c_double), ("scale_modifier", C.c_double),
        ("bg", C.c_void_p), ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p),
        ("projmatrix_raw", C.c_void_p), ("prcppoint", C.c_void_p),
    ]


class KnnMap(C.Structure):
    _fields_ = [
        ("table", C.c_void_p), ("buffer_size", C.c_int64), ("neural_points", C.c_void_p),
        ("point_ts_create", C.c_void_p), ("travel_dist", C.c_void_p), ("cur_ts", C.c_int32),
        ("time_filtering", C.c_int32), ("diff_travel_dist_local", C.c_float),
        ("free_mask", C.c_void_p), ("valid_mask", C.c_void_p),
        ("use_free_mask", C.c_int32), ("use_valid_mask", C.c_int32),
        ("global2local", C.c_void_p), ("neighbor_dx", C.c_void_p), ("K", C.c_int32), ("nn_k", C.c_int32),
        ("resolution", C.c_float), ("max_valid_dist2", C.c_float),
        ("compact", C.c_void_p), ("compact_mask", C.c_uint32),
        ("blocks", C.c_void_p), ("block_records", C.c_void_p), ("blocks_ok", C.c_void_p), ("block_mask", C.c_uint32),
    ]


class QfTables(C.Structure):
    _fields_ = [("geo_features", C.c_void_p), ("color_features", C.c_void_p), ("Fg", C.c_int32), ("Fc", C.c_int32),
                ("points", C.c_void_p), ("orientations", C.c_void_p), ("certainties", C.c_void_p),
                ("after_pgo", C.c_int32), ("weighted_first", C.c_int32)]


class SdfDecoder(C.Structure):
    _fields_ = [("W1", C.c_void_p), ("b1", C.c_void_p), ("W2", C.c_void_p), ("b2", C.c_void_p),
                ("hidden", C.c_int32), ("feat_dim", C.c_int32), ("sdf_scale", C.c_float),
                ("weighted_first", C.c_int32)]


class ColorDecoder(C.Structure):
    _fields_ = [("W1", C.c_void_p), ("b1", C.c_void_p), ("W2", C.c_void_p), ("b2", C.c_void_p),
                ("hidden", C.c_int32), ("feat_dim", C.c_int32), ("channels", C.c_int32),
                ("weighted_first", C.c_int32)]


class MlpJob(C.Structure):
    _fields_ = [("x", C.c_void_p), ("IN", C.c_int32), ("OUT", C.c_int32), ("W1", C.c_void_p), ("b1", C.c_void_p),
                ("W2", C.c_void_p), ("b2", C.c_void_p), ("y", C.c_void_p), ("dL_dy", C.c_void_p), ("dL_dx", C.c_void_p),
                ("dL_dW1", C.c_void_p), ("dL_db1", C.c_void_p), ("dL_dW2", C.c_void_p), ("dL_db2", C.c_void_p)]


class SpawnParams(C.Structure):
    _fields_ = [("n", C.c_int), ("k", C.c_int), ("scale_dim", C.c_int), ("surfel", C.c_int),
                ("color_residual", C.c_int), ("alpha_filter_on", C.c_int), ("scale_filter_on", C.c_int),
                ("displacement_range", C.c_float), ("unit_scale", C.c_float), ("max_scale", C.c_float),
                ("scale_filter_thr", C.c_float)]


class GatherJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("row_bytes", C.c_int64), ("rows", C.c_int64)]


class ImageLossParams(C.Structure):
    _fields_ = [("H", C.c_int), ("W", C.c_int), ("v_min", C.c_int), ("v_max", C.c_int), ("depth_min", C.c_float),
                ("depth_max", C.c_float), ("min_accu_alpha", C.c_float), ("inverse_depth", C.c_int),
                ("consist_mode", C.c_int)]


class RegLoopArgs(C.Structure):
    _fields_ = [("n", C.c_int64), ("flags", C.c_int32), ("iter", C.c_int32), ("trace_cap", C.c_int32),
                ("min_grad", C.c_float), ("max_grad", C.c_float), ("max_std", C.c_float), ("gm_dist", C.c_float),
                ("gm_grad", C.c_float), ("lm_lambda", C.c_float)] + \
               [(k, C.c_void_p) for k in ("src", "cur", "sdf", "grad", "std", "mask", "label", "normals", "valid",
                                          "part", "T", "delta", "record", "trace")]


class RegColorArgs(C.Structure):
    _fields_ = [("src_color", C.c_void_p), ("color_pred", C.c_void_p), ("color_jac", C.c_void_p),
                ("channels", C.c_int32), ("mode", C.c_int32), ("photo_weight", C.c_float), ("photo_part", C.c_void_p)]


class GaussLossArgs(C.Structure):
    _fields_ = [("P", C.c_int64), ("Na", C.c_int64), ("cap", C.c_int64), ("R", C.c_int32), ("ncols", C.c_int32),
                ("scale_cols", C.c_int32), ("flags", C.c_int32), ("min_alpha", C.c_float),
                ("contrib_thr", C.c_float), ("shift_range", C.c_float), ("grad_min", C.c_float),
                ("grad_max", C.c_float), ("inv_voxel_pow", C.c_float), ("n_inject", C.c_int64)] + \
               [(n, vp) for n in ("alpha_all", "visible", "contrib", "free_mask", "xyz", "rot", "scale", "alpha", "seed",
                                  "inject_idx", "randn", "keys", "part", "meta", "idx", "normal", "queries", "label",
                                  "sdf", "grad", "nn", "valid", "losses", "counts", "g", "ds", "v", "dn", "dq",
                                  "d_xyz", "d_rot", "d_scale", "d_alpha", "d_alpha_all")]


class SdfHvpArgs(C.Structure):
    _fields_ = [("W1", vp), ("b1", vp), ("W2", vp), ("b2", vp), ("H", C.c_int32), ("F", C.c_int32),
                ("scale", C.c_float), ("after_pgo", C.c_int32), ("features", vp), ("points", vp),
                ("orientations", vp), ("gpoints", vp), ("queries", vp), ("B", C.c_int64), ("nnk", C.c_int32),
                ("idx", vp), ("gidx", vp), ("v", vp), ("ds", vp), ("grad_x", vp), ("out", vp)]


class SdfLossArgs(C.Structure):
    _fields_ = [("B", C.c_int64), ("cap", C.c_int64), ("k", C.c_int32), ("C", C.c_int32), ("d", C.c_int32),
                ("flags", C.c_int32), ("sigma", C.c_float), ("eik_band", C.c_float), ("col_band", C.c_float)] + \
               [(n, vp) for n in ("coord", "label", "weight", "color_label", "w", "s", "c", "g", "idx", "xsel", "meta",
                                  "part", "sdf_pred", "losses", "counts", "gl", "g_pred", "d_s", "d_g", "d_c")]


class SemLossArgs(C.Structure):
    _fields_ = [("B", C.c_int64), ("k", C.c_int32), ("S", C.c_int32), ("d", C.c_int32), ("flags", C.c_int32)] + \
               [(n, vp) for n in ("raw", "w", "label", "selected", "scratch", "loss", "counts", "gl", "d_raw")]


class AdamwJob(C.Structure):
    _fields_ = [("p", vp), ("g", vp), ("m", vp), ("v", vp), ("n", C.c_int64)] + \
               [(n, C.c_float) for n in ("decay", "beta1", "beta2", "one_minus_beta1", "one_minus_beta2", "step_size",
                                         "bc2_sqrt", "eps")]


class CameraPoseArgs(C.Structure):
    _fields_ = [(n, vp) for n in ("R", "T", "projection_matrix", "world_view_transform", "full_proj_transform",
                                  "camera_center", "cam_trans_delta", "cam_rot_delta", "out")] + \
               [(n, C.c_int64) for n in ("R_s0", "R_s1", "T_s", "proj_s0", "proj_s1", "wvt_s0", "wvt_s1", "fpt_s0",
                                         "fpt_s1", "center_s")] + [("converged_threshold", C.c_double)]


class PoolSampleArgs(C.Structure):
    _fields_ = [("P", C.c_int64)] + \
               [(n, C.c_int32) for n in ("surface_sample_n", "free_front_n", "free_behind_n", "color_channels",
                                         "dist_weight_on", "behind_dropoff_on", "sem_is_i64", "reserved")] + \
               [(n, C.c_double) for n in ("surface_sample_range", "free_sample_begin_ratio", "free_sample_end_dist",
                                          "dist_weight_scale", "max_range")] + \
               [(n, vp) for n in ("points", "normal", "sem", "color", "noise_surface", "noise_front", "noise_behind",
                                  "coord", "sdf_label", "weight", "out_normal", "out_sem", "out_color")]


class PoolAppendArgs(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n", "m", "capacity")] + \
               [(n, C.c_int32) for n in ("frame_id", "color_channels", "pose_is_f64", "reserved")] + \
               [(n, vp) for n in ("pose", "coord", "sdf_label", "weight", "sem", "color", "normal", "global_coord_pool",
                                  "sdf_label_pool", "weight_pool", "time_pool", "sem_label_pool", "color_pool",
                                  "normal_label_pool")]


class PoolSelectArgs(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n", "capacity")] + \
               [(n, C.c_int32) for n in ("color_channels", "pose_is_f64", "select_all", "reserved")] + \
               [("thr", C.c_double)] + \
               [(n, vp) for n in ("pose", "coord", "sdf_label", "color", "normal", "scratch", "out_points", "out_color",
                                  "out_normal")]


class LidarCam(C.Structure):
    _fields_ = [(n, vp) for n in ("image", "K", "T", "keys", "src", "l0", "l1", "l2", "l3")] + \
               [("H", C.c_int32), ("W", C.c_int32)]


class CamfrontMap(C.Structure):
    _fields_ = [(n, vp) for n in ("src", "l0", "l1", "l2", "l3")] + \
               [(n, C.c_int64) for n in ("stride_c", "stride_y", "stride_x")] + \
               [(n, C.c_int32) for n in ("H", "W", "kind", "reserved")]


class PgoArgs(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_nodes", "n_factors", "n_loops", "n_entries")] + \
               [("chunk", C.c_int32), ("iteration", C.c_int32), ("rel_tol", C.c_double)] + \
               [(n, vp) for n in ("fi", "fj", "kind", "lcol", "loop_f", "node_off", "node_ent", "Z", "W", "X", "state", "record",
                                  "status", "scratch")]


# ---------------------------------------------------------------- entry points: {name: (restype, argtypes)}
SIGNATURES = {
    # general
    "pings_abi_version": (i32, []),
    "pings_last_error": (C.c_char_p, []),
    "pings_prof_enable": (i32, [i32]),
    "pings_prof_only": (i32, [C.c_char_p]),
    "pings_prof_report": (i32, [C.c_char_p, sz]),
    # fused SSIM
    "pings_ssim_partials_count": (sz, [i32, i32, i32]),
    "pings_ssim_forward": (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]),
    "pings_ssim_backward": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp]),
    # Gaussian(-surfel) rasteriser
    "pings_raster_mark_visible": (i32, [vp, i32, C.POINTER(RasterSettings), vp, vp]),
    "pings_raster_geom_bytes": (sz, [i32, i32, i32]),
    "pings_raster_binning_bytes": (sz, [i64, i32, i32]),
    "pings_raster_image_bytes": (sz, [i32, i32]),
    "pings_raster_preprocess": (i32, [C.POINTER(RasterSettings), i32, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i64),
                                      C.POINTER(i32), vp]),
    "pings_raster_preprocess_dyn": (i32, [C.POINTER(RasterSettings), i32, vp, vp, vp, vp, vp, vp, vp, vp, i32,
                                          C.POINTER(vp), i32, C.POINTER(i32), C.POINTER(i64), C.POINTER(i32), vp]),
    "pings_raster_render": (i32, [C.POINTER(RasterSettings), i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp]),
    "pings_raster_tile_sort_bytes": (sz, [i64, C.POINTER(i32)]),
    "pings_raster_tile_sort": (i32, [vp, i64, i32, i32, vp, vp, vp, i32, vp]),
    "pings_raster_scan_bytes": (sz, [i64]),
    "pings_raster_scan_u32": (i32, [vp, i64, i32, i32, vp, vp, sz, vp]),
    "pings_raster_backward_bytes": (sz, [i32, i64]),
    "pings_raster_backward": (i32, [C.POINTER(RasterSettings), i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                    vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp]),
    "pings_raster_debug_lists": (i32, [vp, i64, i32, i32, vp, vp, vp]),
    "pings_raster_debug_image": (i32, [vp, i32, i32, vp, vp, vp]),
    "pings_raster_debug_occlusion": (i32, [vp, i32, i32, i32, vp, vp, C.POINTER(C.c_int32), vp]),
    "pings_raster_rank_bucket": (i32, [vp, i64, i32, C.c_uint32, vp]),
    "pings_raster_debug_bin_plan": (i32, [C.POINTER(i32), C.POINTER(C.c_uint32)]),
    "pings_raster_debug_interior": (i32, [vp, vp, i64, f32, f32, f32, f32, vp]),
    # 2D Gaussian splatting rasteriser
    "pings_raster2d_geom_bytes": (sz, [i32, i32, i32]),
    "pings_raster2d_binning_bytes": (sz, [i64, i32, i32]),
    "pings_raster2d_image_bytes": (sz, [i32, i32]),
    "pings_raster2d_preprocess": (i32, [C.POINTER(RasterSettings), i32, vp, vp, vp, vp, vp, vp, vp, vp, i32,
                                        C.POINTER(vp), i32, C.POINTER(i32), C.POINTER(i64), vp]),
    "pings_raster2d_render": (i32, [C.POINTER(RasterSettings), i32, i64, vp, vp, vp, vp, vp, vp]),
    "pings_raster2d_backward_bytes": (sz, [i32, i64]),
    "pings_raster2d_backward": (i32, [C.POINTER(RasterSettings), i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                      vp, vp, vp, vp]),
    "pings_raster2d_debug_lists": (i32, [vp, i64, i32, i32, vp, vp, vp]),
    "pings_raster2d_debug_image": (i32, [vp, i32, i32, vp, vp, vp, vp]),
    # neural-point kNN, query_feature, SDF decode
    "pings_knn_compact_entries": (sz, [i64]),
    "pings_knn_compact_build": (i32, [vp, i64, vp, sz, vp]),
    "pings_knn_blocks_entries": (sz, [i64]),
    "pings_knn_blocks_build": (i32, [C.POINTER(KnnMap), i64, i64, i32, vp, sz, vp, vp, vp]),
    "pings_knn_search": (i32, [C.POINTER(KnnMap), vp, i64, vp, vp, vp, vp, vp]),
    "pings_knn_cells": (i32, [C.POINTER(KnnMap), vp, i64, i64, vp, vp, vp]),
    "pings_query_feature_forward": (i32, [C.POINTER(KnnMap), C.POINTER(QfTables), vp, i64, vp, vp, vp, vp, vp, vp, vp,
                                          vp, vp, vp, vp, vp]),
    "pings_query_feature_accumulate": (i32, [vp, vp, i64, vp, vp]),
    "pings_query_feature_scratch_bytes": (sz, [i64, i32, i64]),
    "pings_query_feature_backward": (i32, [C.POINTER(QfTables), vp, vp, i64, i32, vp, vp, vp, vp, vp, vp, i64, vp, vp,
                                           vp, vp, vp]),
    "pings_query_feature_double_backward": (i32, [C.POINTER(QfTables), vp, vp, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp,
                                                  i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "pings_rows_scatter_add_scratch_bytes": (sz, [i64, i64]),
    "pings_rows_scatter_add": (i32, [vp, i64, vp, i64, i32, vp, vp, i64, vp, vp, vp]),
    "pings_rows_plan_bytes": (sz, [i64, i64]),
    "pings_rows_plan_build": (i32, [vp, i64, i64, vp, vp]),
    "pings_rows_plan_apply": (i32, [vp, i64, i64, vp, i64, i32, vp, vp, vp]),
    "pings_sdf_forward": (i32, [C.POINTER(KnnMap), C.POINTER(SdfDecoder), vp, vp, vp, vp, i32, vp, i64, vp, vp, vp, vp,
                                vp, vp, vp, vp, vp]),
    "pings_sdf_plan": (i32, [i32, i32, i32, i32, i32, i32, C.POINTER(C.c_int32)]),
    "pings_color_forward": (i32, [C.POINTER(ColorDecoder), vp, i64, vp, vp, i32, vp, i64, vp, i32, vp, vp, vp]),
    "pings_sdf_backward_scratch_bytes": (sz, [i64, i32, i32, i32, i64]),
    "pings_sdf_double_backward": (i32, [C.POINTER(SdfDecoder), vp, i64, vp, vp, vp, i32, vp, i64, i32, vp, vp, vp, vp,
                                        vp, vp, vp, vp, vp, vp, vp]),
    "pings_sdf_backward": (i32, [C.POINTER(SdfDecoder), vp, i64, vp, vp, i32, vp, i64, i32, vp, vp, vp, vp, vp, vp, vp,
                                 vp, vp, vp]),
    # decoder MLP
    "pings_mlp_backward_scratch_bytes": (sz, [i32, i32, i32]),
    "pings_mlp_forward": (i32, [vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp]),
    "pings_mlp_backward": (i32, [vp, vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "pings_mlp_double_backward_supported": (i32, [i32, i32, i32]),
    "pings_mlp_double_backward": (i32, [vp, vp, vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "pings_mlp_forward_grouped": (i32, [C.POINTER(MlpJob), i32, i64, vp]),
    "pings_mlp_forward_grouped_dyn": (i32, [C.POINTER(MlpJob), i32, i64, vp, vp]),
    "pings_mlp_backward_grouped_scratch_bytes": (sz, [C.POINTER(MlpJob), i32]),
    "pings_mlp_backward_grouped": (i32, [C.POINTER(MlpJob), i32, i64, vp, vp]),
    # exposure correction
    "pings_exposure_forward": (i32, [vp, vp, vp, i64, vp, vp]),
    "pings_exposure_backward_scratch_bytes": (sz, []),
    "pings_exposure_backward": (i32, [vp, vp, vp, i64, vp, vp, vp, vp, vp]),
    # finite-difference SDF gradient
    "pings_stencil_points": (i32, [vp, i64, f32, i32, vp, vp]),
    "pings_stencil_gradient": (i32, [vp, vp, i64, f32, i32, vp, vp]),
    "pings_stencil_gradient_backward": (i32, [vp, i64, f32, i32, vp, vp, vp]),
    # spawn_gaussians
    "pings_spawn_gather": (i32, [i32, vp, vp, vp, vp, vp, vp, i32, vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp,
                                 vp, vp]),
    "pings_spawn_gather_dyn": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, i32, vp, i32, i32, i32, vp, vp, vp, vp,
                                     vp, vp, vp, vp]),
    "pings_spawn_plan_dyn": (i32, [C.POINTER(SpawnParams), vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "pings_spawn_forward_dyn": (i32, [C.POINTER(SpawnParams), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                      vp, vp, vp, vp, vp, vp, vp]),
    "pings_spawn_gather_backward": (i32, [i32, vp, vp, i32, i32, vp, i32, i32, vp, vp, vp]),
    "pings_spawn_plan_scratch_bytes": (sz, [i64]),
    "pings_spawn_plan": (i32, [C.POINTER(SpawnParams), vp, vp, vp, vp, vp, vp, vp]),
    "pings_spawn_forward": (i32, [C.POINTER(SpawnParams), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                  vp, vp, vp, vp]),
    "pings_spawn_backward": (i32, [C.POINTER(SpawnParams), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                   vp, vp, vp, vp, vp, vp]),
    # neural-point map maintenance
    "pings_voxel_downsample_scratch_bytes": (sz, [i64]),
    "pings_voxel_downsample": (i32, [vp, i64, f32, vp, vp, C.POINTER(i64), vp]),
    "pings_voxel_downsample_min_value": (i32, [vp, vp, i64, f32, vp, vp, C.POINTER(i64), vp]),
    "pings_map_prune_mask": (i32, [i64, vp, i64, i32, vp, vp, f32, f32, vp, vp, vp]),
    "pings_map_adjust": (i32, [i64, vp, vp, vp, vp, i32, vp, i32, i64, vp, vp]),
    "pings_map_rehash": (i32, [vp, vp, i64, f32, i64, vp, vp, vp]),
    "pings_map_update_scratch_bytes": (sz, [i64, i64]),
    "pings_map_update": (i32, [vp, vp, i64, f64, i64, vp, i64, vp, i32, f32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                               vp, vp, C.POINTER(i64), vp]),
    "pings_map_reset_local_scratch_bytes": (sz, [i64]),
    "pings_map_reset_local": (i32, [i64, vp, vp, vp, vp, i32, i32, i32, f32, i32, vp, i32, f64, f64, vp, vp, vp, vp, vp,
                                    C.POINTER(i64), vp]),
    "pings_mask_rows_scratch_bytes": (sz, [i64]),
    "pings_mask_rows": (i32, [vp, i64, vp, vp, C.POINTER(i64), vp]),
    "pings_gather_rows_multi": (i32, [C.POINTER(GatherJob), i32, vp, vp]),
    "pings_gather_rows": (i32, [vp, i64, vp, i64, vp, vp]),
    "pings_scatter_rows": (i32, [vp, i64, vp, i64, vp, vp]),
    # depth2normal
    "pings_depth2normal_forward": (i32, [vp, vp, vp, i32, i32, f32, f32, f32, f32, f32, vp, vp]),
    "pings_depth2normal_backward_scratch_bytes": (sz, [i32, i32]),
    "pings_depth2normal_backward": (i32, [vp, vp, vp, i32, i32, f32, f32, f32, f32, f32, vp, vp, vp, vp]),
    # image-space losses
    "pings_image_losses_scratch_bytes": (sz, []),
    "pings_image_losses_forward": (i32, [C.POINTER(ImageLossParams), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "pings_image_losses_backward": (i32, [C.POINTER(ImageLossParams), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                          vp, vp, vp, vp]),
    # colour / semantic heads
    "pings_head_reduce": (i32, [vp, vp, i64, i32, i32, i32, vp, vp, vp]),
    # tracker registration
    "pings_reg_normal_equations_scratch_bytes": (sz, []),
    "pings_reg_normal_equations": (i32, [vp, vp, vp, vp, i64, vp, vp, vp]),
    "pings_reg_solve": (i32, [vp, f32, vp, vp, vp]),
    "pings_reg_solve_checked": (i32, [vp, f32, vp, vp, vp, C.POINTER(i32), vp]),
    # device-resident odometry loop
    "pings_reg_partials": (i32, [i64]),
    "pings_reg_transform": (i32, [C.POINTER(RegLoopArgs), vp]),
    "pings_reg_assemble": (i32, [C.POINTER(RegLoopArgs), vp]),
    "pings_reg_step": (i32, [C.POINTER(RegLoopArgs), vp]),
    "pings_reg_assemble_color": (i32, [C.POINTER(RegLoopArgs), C.POINTER(RegColorArgs), vp]),
    "pings_reg_read_record": (i32, [vp, vp, vp]),
    # Gaussian-space loss block
    "pings_gauss_loss_select": (i32, [C.POINTER(GaussLossArgs), vp]),
    "pings_gauss_loss_prepare": (i32, [C.POINTER(GaussLossArgs), vp]),
    "pings_gauss_loss_reduce": (i32, [C.POINTER(GaussLossArgs), vp]),
    "pings_gauss_loss_backward_rows": (i32, [C.POINTER(GaussLossArgs), vp]),
    "pings_gauss_loss_backward_scatter": (i32, [C.POINTER(GaussLossArgs), vp]),
    "pings_sdf_hvp_x": (i32, [C.POINTER(SdfHvpArgs), vp]),
    # SDF-sample loss block
    "pings_sdf_loss_select": (i32, [C.POINTER(SdfLossArgs), vp]),
    "pings_sdf_loss_reduce": (i32, [C.POINTER(SdfLossArgs), vp]),
    "pings_sdf_loss_backward": (i32, [C.POINTER(SdfLossArgs), vp]),
    "pings_sdf_loss_partials": (i32, [i64, i64]),
    # semantic loss block
    "pings_sem_loss_scratch_bytes": (sz, [i64]),
    "pings_sem_loss_forward": (i32, [C.POINTER(SemLossArgs), vp]),
    "pings_sem_loss_backward": (i32, [C.POINTER(SemLossArgs), vp]),
    # marching cubes
    "pings_mc_scratch_bytes": (sz, [i64, i64, i64]),
    "pings_mc_count": (i32, [vp, vp, i64, i64, i64, f32, i32, vp, C.POINTER(i64), vp]),
    "pings_mc_emit": (i32, [vp, vp, i64, i64, i64, f32, i32, vp, i64, i64, vp, vp, vp, vp]),
    # mesh finishing
    "pings_mesh_weld_scratch_bytes": (sz, [i64, i64]),
    "pings_mesh_weld": (i32, [vp, i64, vp, i64, vp, vp, vp, vp, vp, C.POINTER(i64), vp]),
    "pings_mesh_clusters_scratch_bytes": (sz, [i64]),
    "pings_mesh_clusters": (i32, [vp, i64, i64, vp, vp, vp, C.POINTER(i64), vp]),
    "pings_mesh_drop_small_scratch_bytes": (sz, [i64]),
    "pings_mesh_drop_small": (i32, [vp, i64, vp, vp, i64, vp, vp, C.POINTER(i64), vp]),
    "pings_mesh_vertex_normals_scratch_bytes": (sz, [i64, i64]),
    "pings_mesh_vertex_normals": (i32, [vp, i64, vp, i64, vp, vp, vp]),
    "pings_mesh_compact_vertices_scratch_bytes": (sz, [i64, i64]),
    "pings_mesh_compact_vertices": (i32, [vp, i64, vp, i64, vp, vp, vp, vp, vp, C.POINTER(i64), vp]),
    # labelled meshes
    "pings_mesh_label_colors": (i32, [vp, i64, vp, vp, i64, vp, vp, vp, vp]),
    "pings_mesh_remove_vertices_scratch_bytes": (sz, [i64, i64]),
    "pings_mesh_remove_vertices": (i32, [vp, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i64), vp]),
    # mesh surface sampling
    "pings_mesh_sample_scratch_bytes": (sz, [i64]),
    "pings_mesh_sample": (i32, [vp, i64, vp, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp]),
    # fused AdamW
    "pings_adamw_step": (i32, [C.POINTER(AdamwJob), i32, C.POINTER(i32), vp]),
    # view evaluation
    "pings_eval_view_metrics_scratch_bytes": (sz, [i64]),
    "pings_eval_view_metrics": (i32, [vp, vp, i32, i64, vp, vp, vp, f32, f32, f32, i32, vp, vp, vp, vp]),
    "pings_eval_backproject_scratch_bytes": (sz, [i64]),
    "pings_eval_backproject": (i32, [vp, vp, vp, i32, i32, C.POINTER(f64), C.POINTER(f64), f64, f32, i32, vp, vp, vp,
                                     vp, vp]),
    "pings_eval_voxel_scratch_bytes": (sz, [i64]),
    "pings_eval_voxel_centroids": (i32, [vp, i64, vp, f64, vp, vp, vp, vp, vp]),
    "pings_eval_nn_scratch_bytes": (sz, [i64]),
    "pings_eval_nn_build": (i32, [vp, i64, vp, f64, vp, vp, vp]),
    "pings_eval_nn_query": (i32, [vp, i64, vp, vp, i64, f64, f64, vp, vp, vp]),
    "pings_eval_pair_reduce": (i32, [vp, i64, vp, vp, i64, vp, f64, f64, vp, vp, vp]),
    # camera pose
    "pings_camera_update_pose": (i32, [C.POINTER(CameraPoseArgs), vp]),
    "pings_camera_set_pose": (i32, [vp, i32, i64, i64, vp, i64, i64, vp, vp]),
    # SDF training-sample pool
    "pings_pool_sample": (i32, [C.POINTER(PoolSampleArgs), vp]),
    "pings_pool_draw": (i32, [C.POINTER(GatherJob), i32, vp, i64, vp, i64, vp, i64, vp, i64, i64, vp, vp]),
    "pings_pool_ts_range": (i32, [vp, i32, i64, vp, vp]),
    "pings_pool_transform": (i32, [i64, vp, vp, i32, vp, i32, i64, vp, vp]),
    "pings_pool_window_scratch_bytes": (sz, [i64]),
    "pings_pool_window_count": (i32, [vp, i64, vp, f32, i32, vp, C.POINTER(i64), vp]),
    "pings_pool_window": (i32, [vp, i64, vp, f32, i32, vp, vp, i64, vp]),
    # the pool part of Mapper.process_frame
    "pings_pool_append": (i32, [C.POINTER(PoolAppendArgs), vp]),
    "pings_pool_discard_mark": (i32, [vp, i64, i64, vp, vp, vp]),
    "pings_pool_compact_scratch_bytes": (sz, [i64]),
    "pings_pool_compact_count": (i32, [vp, i64, i64, vp, C.POINTER(i64), vp]),
    "pings_pool_compact": (i32, [C.POINTER(GatherJob), i32, vp, i64, vp, vp]),
    "pings_pool_select_scratch_bytes": (sz, [i64]),
    "pings_pool_select_count": (i32, [vp, i64, f64, vp, C.POINTER(i64), vp]),
    "pings_pool_select_update": (i32, [C.POINTER(PoolSelectArgs), vp]),
    # frame-time point tests
    "pings_frame_new_scratch_bytes": (sz, [i64]),
    "pings_frame_new_count": (i32, [C.POINTER(KnnMap), vp, i64, vp, vp, i64, f64, f64, f64, vp, C.POINTER(i64), vp]),
    "pings_frame_new_rows": (i32, [vp, i64, i64, vp, i64, vp]),
    "pings_frame_static_mask": (i32, [vp, vp, vp, i64, f64, f64, f64, vp, vp, vp]),
    "pings_frame_valid_scatter": (i32, [vp, i64, vp, vp, f64, i64, vp, i64, i64, vp, vp, vp]),
    # loop-closure context
    "pings_loop_context_scratch_bytes": (sz, [i64, i32, i32, i32, i32]),
    "pings_loop_context_build": (i32, [vp, i64, vp, i32, vp, i32, i32, i32, f64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                       vp]),
    "pings_loop_ring_key": (i32, [vp, i32, i32, i32, vp, vp]),
    "pings_loop_virtual_poses": (i32, [vp, vp, i32, f64, vp, vp, vp, vp, vp]),
    "pings_loop_search": (i32, [vp, vp, i64, vp, i32, vp, vp, i32, i32, i32, i32, i32, f64, vp, vp, vp, vp]),
    "pings_loop_context_distance": (i32, [vp, vp, i32, i32, i32, vp, vp]),
    "pings_loop_read_record": (i32, [vp, vp, vp, vp]),
    # LiDAR frame front-end
    "pings_lidar_crop": (i32, [vp, i64, i64, f64, f64, f64, f64, i32, vp, vp]),
    "pings_lidar_deskew_scratch_bytes": (sz, []),
    "pings_lidar_deskew": (i32, [vp, i64, i64, vp, i32, vp, i32, f64, vp, i32, i32, C.POINTER(f64), C.POINTER(f64), vp,
                                 vp]),
    "pings_lidar_slerp_pose": (i32, [vp, i32, f64, vp, i32, i32, vp, i32, vp]),
    "pings_lidar_project": (i32, [vp, i64, i64, C.POINTER(LidarCam), i32, f64, f64, vp, i64, vp, i64, vp, i32, vp]),
    "pings_lidar_depth_pyramid": (i32, [C.POINTER(LidarCam), i32, vp]),
    # camera frame front-end
    "pings_camfront_pyramid": (i32, [C.POINTER(CamfrontMap), i32, C.POINTER(i32), vp]),
    "pings_camfront_align_scratch_bytes": (sz, []),
    "pings_camfront_align": (i32, [vp, vp, i64, f64, f64, vp, vp, vp]),
    "pings_camfront_cloud_scratch_bytes": (sz, [i64]),
    "pings_camfront_mono_cloud": (i32, [vp, vp, i32, i32, vp, C.POINTER(f64), C.POINTER(f64), f64, f64, f64, i32, vp, vp,
                                        vp, vp, vp, vp]),
    "pings_camfront_voxel_scratch_bytes": (sz, [i64]),
    "pings_camfront_voxel_average": (i32, [vp, i64, vp, f64, vp, vp, i64, vp, vp, vp, vp]),
    # sparse TSDF fusion
    "pings_tsdf_table_insert": (i32, [vp, i64, vp, vp, i64, vp, vp]),
    "pings_tsdf_touch": (i32, [vp, i32, i32, C.POINTER(f64), C.POINTER(f64), C.POINTER(f64), f64, f64, f32, f32, i32, i32,
                               vp, vp, vp, i64, i64, vp, vp, vp, C.POINTER(i64), vp]),
    "pings_tsdf_assign_scratch_bytes": (sz, [i64]),
    "pings_tsdf_assign": (i32, [vp, i64, i64, i64, vp, vp, vp, i64, vp, vp, vp, vp, vp]),
    "pings_tsdf_update": (i32, [vp, vp, i32, i32, C.POINTER(f64), C.POINTER(f64), C.POINTER(f64), f64, f64, f32, f32, vp,
                                i64, vp, vp, i64, i64, vp, vp, vp, vp]),
    "pings_tsdf_densify": (i32, [vp, vp, i64, i64, vp, vp, vp, C.POINTER(i64), i64, i64, i64, f32, vp, vp, vp, vp]),
    "pings_tsdf_vertices": (i32, [vp, i64, vp, vp, C.POINTER(i64), i64, i64, i64, C.POINTER(f64), f64, vp, vp, vp]),
    # LiDAR scans into the TSDF volume
    "pings_tsdf_points_touch": (i32, [vp, i64, vp, C.POINTER(f64), f64, f64, f32, f32, i32, i32, vp, vp, vp, vp, i64, i64,
                                      vp, vp, vp, C.POINTER(i64), vp]),
    "pings_tsdf_points_accumulate": (i32, [vp, vp, i64, vp, C.POINTER(f64), f64, f64, f32, f32, i32, i32, i32, vp, vp, vp,
                                           vp, i64, i64, vp, vp]),
    "pings_tsdf_points_apply": (i32, [vp, i64, vp, i64, i64, vp, i32, f32, vp, vp, vp, vp]),
    # pose-graph optimisation
    "pings_pgo_scratch_bytes": (sz, [i64, i64, i64, i32]),
    "pings_pgo_cost": (i32, [C.POINTER(PgoArgs), vp, vp, vp]),
    "pings_pgo_iteration": (i32, [C.POINTER(PgoArgs), vp]),
    "pings_pgo_read_record": (i32, [vp, vp, vp]),
    "pings_pgo_pose_diff": (i32, [vp, vp, i64, vp, vp, vp]),
}
