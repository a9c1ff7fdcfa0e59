"""ctypes binding of libdefslam_hip.so (the C ABI in include/defslam_hip.h) and of the lab build
libdefslam_hip_lab.so (the same ABI + include/defslam_hip_debug.h: test hooks, timers, A/B solver switches).

Both are built in-tree by `__graft_entry__.build()` / `make -C defslam_amd/csrc`.
There is no CPU fallback: if the shared object is missing, importing a symbol raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# The in-tree libraries, always: neither this binding nor the .so reads environment variables (tools that A/B two builds assign
# _lib.LIB_PATH / _lib.LAB_LIB_PATH before the first load()).
LIB_PATH = os.path.join(_HERE, "lib", "libdefslam_hip.so")
LAB_LIB_PATH = os.path.join(_HERE, "lib", "libdefslam_hip_lab.so")

DSH_OK = 0
DSH_ERR_ARG = 1
DSH_ERR_STATE = 3
DSH_TRACE_STRIDE = 8
DSH_MAX_ITERS = 64

c_double_p = C.POINTER(C.c_double)
c_float_p = C.POINTER(C.c_float)
c_i32_p = C.POINTER(C.c_int32)
c_u8_p = C.POINTER(C.c_uint8)


class SftFrameC(C.Structure):
    _fields_ = [
        ("Tcw", c_float_p),
        ("K", C.c_double * 4),
        ("n_frame", C.c_int32),
        ("M", C.c_int32),
        ("obs_nodes", c_i32_p),
        ("obs_bary", c_double_p),
        ("obs_uv", c_double_p),
        ("obs_invsig2", c_double_p),
        ("xyz", c_double_p),
        ("reg_lap", C.c_double),
        ("reg_inex", C.c_double),
        ("reg_temp", C.c_double),
        ("neighbour_layers", C.c_int32),
        ("max_iters", C.c_int32),
    ]


class SftResultC(C.Structure):
    _fields_ = [
        ("Tcw", c_float_p),
        ("pose7", c_double_p),
        ("xyz", c_double_p),
        ("chi2_obs", c_double_p),
        ("outlier", c_u8_p),
        ("mappoint_xyz", c_float_p),
        ("rep_error", C.c_double),
        ("inliers", C.c_int32),
        ("iters", C.c_int32),
        ("trials", C.c_int32),
        ("dim", C.c_int32),
        ("half_bandwidth", C.c_int32),
        ("status", C.c_int32),
        ("trace", c_double_p),
    ]


class SchwarpProblemC(C.Structure):
    pass


class BbsC(C.Structure):
    _fields_ = [("umin", C.c_double), ("umax", C.c_double), ("nptsu", C.c_int32), ("vmin", C.c_double), ("vmax", C.c_double),
                ("nptsv", C.c_int32), ("valdim", C.c_int32)]


# the pointer members are declared void*: the mirror fills them with plain addresses (base of a pooled array + offset), which costs a
# fraction of a typed ctypes pointer per field
SchwarpProblemC._fields_ = [("bbs", BbsC), ("P", C.c_int32), ("kp1", C.c_void_p), ("kp2", C.c_void_p), ("invsig", C.c_void_p), ("fx_slot", C.c_double),
                            ("fy_slot", C.c_double), ("lam", C.c_double), ("fx", C.c_float), ("fy", C.c_float), ("max_iters", C.c_int32), ("x", C.c_void_p),
                            ("diff", C.c_void_p), ("drop", C.c_void_p), ("info", C.c_int32 * 2), ("costs", C.c_double * 2), ("init_lambda", C.c_double), ("init_ok", C.c_int32)]



class SchwarpStoreC(C.Structure):
    _fields_ = [("point_id", C.c_void_p), ("idx2", C.c_void_p), ("tag", C.c_int32)]


class TrackFrameC(C.Structure):
    _fields_ = [("Tcw", c_float_p), ("Ow", C.c_float * 3), ("K", C.c_float * 4), ("bounds", C.c_float * 4), ("grid_cols", C.c_int32),
                ("grid_rows", C.c_int32), ("levels", C.c_int32), ("scale_factors", c_float_p), ("log_scale_factor", C.c_float), ("N", C.c_int32),
                ("kp", c_float_p), ("octave", c_i32_p), ("desc", c_u8_p), ("state", c_u8_p)]


class TrackProblemC(C.Structure):
    _fields_ = [("frame", TrackFrameC), ("mode", C.c_int32), ("th", C.c_float), ("Q", C.c_int32), ("xyz", c_float_p), ("octave", c_i32_p),
                ("normal", c_float_p), ("max_distance", c_float_p), ("desc", c_u8_p), ("skip", c_u8_p), ("match", c_i32_p), ("in_view", c_u8_p),
                ("level", c_i32_p), ("uv", c_float_p), ("view_cos", c_float_p), ("nmatches", C.c_int32), ("rescans", C.c_int32)]


DSH_TRACK_FRAME = 0
DSH_TRACK_LOCAL = 1


class MpKeyFrameC(C.Structure):
    _fields_ = [("Ow", C.c_float * 3), ("N", C.c_int32), ("desc", c_u8_p), ("octave", c_i32_p), ("levels", C.c_int32),
                ("scale_factors", c_float_p), ("bad", C.c_int32)]


DSH_MP_DESCRIPTOR = 1
DSH_MP_NORMAL_DEPTH = 2
DSH_MP_NO_OBS = 1
DSH_MP_NO_GOOD_DESC = 2
DSH_MP_MAX_OBS = 65535


class MpdbDescC(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("point_capacity", C.c_int32), ("keyframe_capacity", C.c_int32), ("observation_capacity", C.c_int64)]


DSH_MPDB_POSITION = 1
DSH_MPDB_NORMAL_DEPTH = 2
DSH_MPDB_DESCRIPTOR = 4


class TrackCloseCountsC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("matches_inliers", "matches_outliers", "to_match_local", "observed", "inliers", "outliers",
                                         "local_map_points", "n_moved")]


class TrackEndCountsC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("cleaned", "dropped", "kept")]


class PoseOnlyProblemC(C.Structure):
    _fields_ = [("Tcw", c_float_p), ("K", C.c_float * 4), ("N", C.c_int32), ("kp", c_float_p), ("octave", c_i32_p), ("levels", C.c_int32),
                ("inv_level_sigma2", c_float_p), ("frame_points", c_i32_p), ("outlier", c_u8_p), ("Tcw_out", C.c_float * 16),
                ("pose", C.c_double * 7), ("n_initial", C.c_int32), ("n_bad", C.c_int32), ("n_good", C.c_int32), ("rounds", C.c_int32),
                ("iters", C.c_int32 * 4), ("trials", C.c_int32 * 4), ("bad", C.c_int32 * 4), ("chi2", C.c_double * 4)]


class TrackSftFrameC(C.Structure):
    _fields_ = [("Tcw", c_float_p), ("K", C.c_double * 4), ("N", C.c_int32), ("kp", c_float_p), ("octave", c_i32_p), ("levels", C.c_int32),
                ("inv_level_sigma2", c_float_p), ("frame_points", c_i32_p), ("outlier", c_u8_p), ("xyz", c_double_p), ("reg_lap", C.c_double),
                ("reg_inex", C.c_double), ("reg_temp", C.c_double), ("neighbour_layers", C.c_int32), ("max_iters", C.c_int32)]


class TrackSftTableC(C.Structure):
    _fields_ = [("capacity", C.c_int32), ("M", C.c_int32), ("points_obs", C.c_int32), ("kp_index", c_i32_p), ("point_id", c_i32_p),
                ("nodes", c_i32_p), ("bary", c_double_p), ("uv", c_double_p), ("invsig2", c_double_p)]


class KfKeypointsC(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("N", C.c_int32), ("kp", c_float_p)]


class SurfaceGridC(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("bbs", C.POINTER(BbsC)), ("depth_ctrl", c_double_p), ("Twc", c_float_p), ("xs", C.c_int32), ("ys", C.c_int32)]


class TemplateSwitchCountsC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_new", "first_id", "n_moved", "n_masked", "n_embedded", "n_points")]


class TemplateSwitchInputC(C.Structure):
    _fields_ = [("kfdb", C.c_void_p), ("slot", C.c_int32), ("kf", C.POINTER(KfKeypointsC)), ("surface_pts", c_float_p), ("Twc", c_float_p)]


class AnchorListsC(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("anchor_capacity", "pair_capacity", "query_capacity")] + [("max_matrix_bytes", C.c_int64)] +
                [(n, c_i32_p) for n in ("anchor_slot", "anchor_count", "anchor_pairs", "pair_ptr", "pair_idx1", "pair_idx2", "pair_point")] +
                [("pair_own", c_u8_p)] + [(n, c_i32_p) for n in ("query_ptr", "query_idx1", "query_point")] + [("has", c_u8_p)] +
                [(n, C.c_int32) for n in ("n_anchors", "n_pairs", "n_queries", "n_no_ref")])


DSH_MP_NO_REF = 4
DSH_MP_SKIPPED_BAD = 8
DSH_UPKEEP_IDS = 0
DSH_UPKEEP_EMBEDDED = 1


class KeyframeProcessInputC(C.Structure):
    _fields_ = [("kfdb", C.c_void_p), ("slot", C.c_int32)]


class KeyframeProcessCountsC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_empty", "n_bad", "n_added", "n_recent", "n_no_good_desc", "n_no_ref")] + [("first_record", C.c_int64)]


class PointUpkeepInputC(C.Structure):
    _fields_ = [("kfdb", C.c_void_p), ("what", C.c_int32), ("select", C.c_int32), ("n", C.c_int32), ("ids", c_i32_p)]


class PointUpkeepCountsC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_selected", "n_no_obs", "n_no_good_desc", "n_no_ref", "n_bad")]


class PointEraseCountsC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_found", "n_ref_moved", "n_set_bad", "n_records", "n_entries")]


class KeyframeRegisterInputC(C.Structure):
    _fields_ = [("kfdb", C.c_void_p), ("slot", C.c_int32), ("N", C.c_int32), ("surface_pts", c_float_p), ("Twc", c_float_p), ("u", c_double_p),
                ("nu", C.c_int64), ("chi_limit", C.c_double), ("check_chi", C.c_int32)]


class KeyframeRegisterResultC(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("n_pairs", "n_empty", "n_bad", "n_no_facet", "n_no_snapshot", "registered", "stream_status")] +
                [("consumed", C.c_int64), ("sim3", C.c_double * 8), ("s22", C.c_double), ("info", C.c_double * 8), ("Tcw_new", C.c_float * 16),
                 ("Ow_new", C.c_float * 3)])


class KeyframePoseInputC(C.Structure):
    _fields_ = [("kfdb", C.c_void_p), ("slot", C.c_int32), ("Tcw", c_float_p)]


class KeyframeSurfaceInfoC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("N", "n_normals", "enough_normals", "has_depth")] + [("grid", BbsC)]


class SurfaceTakeInputC(C.Structure):
    _fields_ = [("ddb", C.c_void_p), ("n", C.c_int32), ("sel", c_i32_p), ("slot", c_i32_p), ("idx", c_i32_p)]


class KeyframeSfnInputC(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("slot", C.c_int32), ("bbs", C.POINTER(BbsC)), ("bending_weight", C.c_double), ("mean_depth", C.c_double)]


class KeyframeSfnResultC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_sites", "n_empty", "n_bad", "n_no_normal", "n_nan", "ok")]


class KeyframeCreateInputC(C.Structure):
    _fields_ = [("kfdb", C.c_void_p), ("kf", C.POINTER(MpKeyFrameC)), ("Tcw", c_float_p), ("points", c_i32_p), ("kpn", c_float_p)]


class KeyframeCreateResultC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("slot", "n_held", "n_snapshot")] + [("Ow", C.c_float * 3)]


class KeyframeConnectionsC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_counted", "n_connected", "parent", "parent_set", "max_weight", "max_kf")]


class KeyframeViewC(C.Structure):
    _fields_ = ([("N", C.c_int32), ("kp_px", c_float_p)] +
                [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "mnMinX", "mnMaxX", "mnMinY", "mnMaxY")] +
                [("grid_cols", C.c_int32), ("grid_rows", C.c_int32), ("warp_grid", BbsC)])


class WarpPairInputC(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("kfdb", C.c_void_p), ("ddb", C.c_void_p), ("slot", C.c_int32), ("anchor", C.c_int32), ("tag", C.c_int32),
                ("lam", C.c_double), ("min_pairs", C.c_int32), ("max_iters", C.c_int32), ("radius", C.c_float), ("th_low", C.c_int32),
                ("n_pairs", C.c_int32), ("pair_idx1", c_i32_p), ("pair_idx2", c_i32_p), ("n_queries", C.c_int32), ("query_idx1", c_i32_p)]


class WarpPairResultC(C.Structure):
    _fields_ = ([("x", c_double_p), ("pair_state", c_u8_p), ("query_state", c_u8_p), ("query_match", c_i32_p), ("query_point", c_i32_p),
                 ("query_added", c_u8_p), ("init_ok", C.c_int32), ("fitted", C.c_int32), ("info", C.c_int32 * 2), ("costs", C.c_double * 2),
                 ("first_record", C.c_int64)] +
                [(n, C.c_int32) for n in ("n_filtered", "n_matched", "n_appended", "n_list", "n_skipped", "n_dropped", "n_kept", "n_stored", "rounds")] +
                [("erase", PointEraseCountsC)])


class OrbConfigC(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("levels", C.c_int32), ("scale_factor", C.c_float),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32), ("capacity", C.c_int32), ("pattern", c_i32_p)]


DIFFPROP_FIELDS = ["I1u", "I1v", "I2u", "I2v", "J12a", "J12b", "J12c", "J12d", "J21a", "J21b", "J21c", "J21d",
                   "H12uux", "H12uuy", "H12uvx", "H12uvy", "H12vvx", "H12vvy"]


# Every symbol include/defslam_hip.h declares (checked by tests/test_abi.py).
EXPORTED_SYMBOLS = [
    "dsh_create", "dsh_destroy", "dsh_last_error", "dsh_stream", "dsh_synchronize",
    "dsh_template_build", "dsh_template_set", "dsh_template_dims", "dsh_template_get", "dsh_template_embed",
    "dsh_sft_solve", "dsh_sft_batch_upload", "dsh_sft_batch_run", "dsh_sft_batch_download",
    "dsh_sft_batch_counts", "dsh_sft_batch_problem_info",
    "dsh_bbs_eval", "dsh_bbs_coloc", "dsh_normals_estimate", "dsh_schwarp_eval", "dsh_schwarp_fit", "dsh_schwarp_fit_batch",
    "dsh_sfn_estimate", "dsh_bbs_bending", "dsh_warp_initialize", "dsh_search_by_schwarp",
    "dsh_template_embed_device", "dsh_scale_min_median", "dsh_optimize_horn", "dsh_surface_register",
    "dsh_comm_unique_id", "dsh_comm_create", "dsh_comm_destroy", "dsh_sft_shared_solve", "dsh_sft_shared_solve_group", "dsh_sft_connected_solve", "dsh_sft_connected_solve_group",
    "dsh_diffdb_create", "dsh_diffdb_destroy", "dsh_diffdb_clear", "dsh_diffdb_count", "dsh_diffdb_append", "dsh_schwarp_fit_batch_store",
    "dsh_normals_estimate_db", "dsh_sfn_estimate_db",
    "dsh_search_by_projection_batch", "dsh_search_by_projection_frame", "dsh_search_by_projection_local",
    "dsh_kfdb_create", "dsh_kfdb_destroy", "dsh_kfdb_clear", "dsh_kfdb_add", "dsh_kfdb_set_bad", "dsh_kfdb_count", "dsh_mappoint_update",
    "dsh_mpdb_create", "dsh_mpdb_destroy", "dsh_mpdb_clear", "dsh_mpdb_point_count", "dsh_mpdb_keyframe_count", "dsh_mpdb_add_points",
    "dsh_mpdb_update_points", "dsh_mpdb_set_points_bad", "dsh_mpdb_add_observations", "dsh_mpdb_erase_observations", "dsh_mpdb_add_keyframe",
    "dsh_mpdb_set_keyframe_point", "dsh_mpdb_set_keyframe_parent", "dsh_mpdb_set_keyframe_bad",
    "dsh_local_map_update", "dsh_local_map_points", "dsh_local_map_search",
    "dsh_trackstate_set_embedding", "dsh_trackstate_clear_embedding", "dsh_trackstate_set_counters", "dsh_trackstate_get",
    "dsh_trackstate_seed_local_points", "dsh_trackstate_repose", "dsh_trackstate_cull", "dsh_track_close_frame",
    "dsh_track_end_frame", "dsh_track_last_frame", "dsh_motion_model_search",
    "dsh_track_pose_only", "dsh_track_pose_only_batch",
    "dsh_track_sft_observations", "dsh_track_sft",
    "dsh_surface_vertices", "dsh_need_new_template", "dsh_template_switch", "dsh_point_store_get_points", "dsh_point_store_get_embedding",
    "dsh_point_store_add_observations_indexed", "dsh_point_store_set_reference_keyframes", "dsh_point_store_get_reference_keyframes", "dsh_keyframe_anchors",
    "dsh_keyframe_process_new", "dsh_point_store_upkeep",
    "dsh_point_store_erase_observations", "dsh_point_store_set_bad", "dsh_point_store_cull", "dsh_point_store_get_observations",
    "dsh_point_store_get_keyframe_table",
    "dsh_keyframe_snapshot_positions", "dsh_keyframe_get_snapshot", "dsh_keyframe_register_clouds", "dsh_keyframe_register",
    "dsh_keyframe_set_pose", "dsh_keyframe_get_centre",
    "dsh_keyframe_surface_init", "dsh_keyframe_surface_set_depth", "dsh_keyframe_surface_set_points", "dsh_keyframe_surface_set_normals",
    "dsh_keyframe_surface_take_normals", "dsh_keyframe_surface_gather", "dsh_keyframe_surface_get", "dsh_keyframe_surface_vertices",
    "dsh_keyframe_sfn", "dsh_keyframe_surface_state",
    "dsh_track_keyframe_candidate", "dsh_keyframe_create", "dsh_keyframe_update_connections",
    "dsh_keyframe_set_view", "dsh_keyframe_get_view", "dsh_keyframe_warp_pair",
    "dsh_orb_create", "dsh_orb_destroy", "dsh_orb_level_sizes", "dsh_orb_detect", "dsh_orb_describe", "dsh_orb_get_plane",
]
DSH_COMM_ID_BYTES = 128

# include/defslam_hip_debug.h: only libdefslam_hip_lab.so exports these
LAB_SYMBOLS = ["dsh_lab_set_option", "dsh_lab_sft_run_timed", "dsh_lab_sft_assemble_timed", "dsh_lab_sft_phase_ms", "dsh_lab_sft_step_trace",
               "dsh_lab_sft_system", "dsh_lab_sft_solver_info", "dsh_lab_sft_wave_check", "dsh_lab_sft_dump", "dsh_lab_sft_rounds_timed",
               "dsh_lab_sft_factor_check"]

_lib = None
_lab = None


def load() -> C.CDLL:
    """Load the product library; raises OSError when it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        _lib = _bind(LIB_PATH, lab=False)
    return _lib


def load_lab() -> C.CDLL:
    """Load the lab build (product ABI + the measurement / debugging entry points)."""
    global _lab
    if _lab is None:
        _lab = _bind(LAB_LIB_PATH, lab=True)
    return _lab


def _bind(path: str, lab: bool) -> C.CDLL:
    if not os.path.exists(path):
        raise OSError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      f"(or `make -C defslam_amd/csrc`). There is no CPU fallback.")
    L = C.CDLL(path)
    vp = C.c_void_p
    L.dsh_create.argtypes = [C.POINTER(vp), C.c_int]
    L.dsh_destroy.argtypes = [vp]
    L.dsh_last_error.argtypes = [vp]
    L.dsh_last_error.restype = C.c_char_p
    L.dsh_stream.argtypes = [vp]
    L.dsh_stream.restype = vp
    L.dsh_synchronize.argtypes = [vp]
    L.dsh_template_build.argtypes = [vp, C.c_int, c_double_p, C.c_int, c_i32_p]
    L.dsh_template_set.argtypes = [vp, C.c_int, c_double_p, c_u8_p, c_i32_p, c_i32_p, c_double_p, c_double_p, C.c_int, c_i32_p,
                                   c_double_p, C.c_double]
    L.dsh_template_dims.argtypes = [vp, c_i32_p, c_i32_p, c_i32_p]
    L.dsh_template_get.argtypes = [vp, c_u8_p, c_i32_p, c_i32_p, c_double_p, c_double_p, c_i32_p, c_double_p, c_double_p]
    L.dsh_template_embed.argtypes = [vp, C.c_int, c_float_p, c_i32_p, c_i32_p, c_float_p]
    L.dsh_sft_solve.argtypes = [vp, C.POINTER(SftFrameC), C.POINTER(SftResultC)]
    L.dsh_sft_batch_upload.argtypes = [vp, C.c_int, C.POINTER(SftFrameC)]
    L.dsh_sft_batch_run.argtypes = [vp]
    L.dsh_sft_batch_download.argtypes = [vp, C.c_int, C.POINTER(SftResultC)]
    L.dsh_sft_batch_counts.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.dsh_sft_batch_problem_info.argtypes = [vp, C.c_int, C.POINTER(C.c_int64), c_i32_p]
    L.dsh_bbs_eval.argtypes = [vp, C.POINTER(BbsC), c_double_p, c_double_p, c_double_p, C.c_int, C.c_int, C.c_int, c_double_p, c_u8_p]
    L.dsh_bbs_coloc.argtypes = [vp, C.POINTER(BbsC), c_double_p, c_double_p, C.c_int, C.c_int, C.c_int, c_i32_p, c_double_p, c_i32_p]
    L.dsh_normals_estimate.argtypes = [vp, C.c_int, c_i32_p, c_float_p, c_u8_p, c_float_p, c_u8_p, c_float_p, c_u8_p, c_float_p,
                                       c_double_p, c_double_p, c_i32_p, c_float_p, c_float_p, c_u8_p, c_i32_p]
    L.dsh_schwarp_eval.argtypes = [vp, C.POINTER(BbsC), C.c_int, c_float_p, c_float_p, c_float_p, C.c_double, C.c_double, C.c_double, c_double_p,
                                   c_double_p, c_double_p]
    L.dsh_schwarp_fit.argtypes = [vp, C.POINTER(BbsC), C.c_int, c_float_p, c_float_p, c_float_p, C.c_double, C.c_double, C.c_double, C.c_float,
                                  C.c_float, C.c_int, c_double_p, c_float_p, c_u8_p, c_i32_p, c_double_p]
    L.dsh_schwarp_fit_batch.argtypes = [vp, C.c_int, C.POINTER(SchwarpProblemC)]
    L.dsh_diffdb_create.argtypes = [vp, C.c_int64, C.POINTER(vp)]
    L.dsh_diffdb_destroy.argtypes = [vp]
    L.dsh_diffdb_clear.argtypes = [vp]
    L.dsh_diffdb_count.argtypes = [vp]
    L.dsh_diffdb_count.restype = C.c_int64
    L.dsh_diffdb_append.argtypes = [vp, C.c_int, c_float_p, c_i32_p, c_i32_p, c_i32_p]
    L.dsh_schwarp_fit_batch_store.argtypes = [vp, C.c_int, C.POINTER(SchwarpProblemC), C.POINTER(SchwarpStoreC), vp]
    L.dsh_normals_estimate_db.argtypes = [vp, vp, C.c_int, c_i32_p, c_float_p, c_u8_p, c_float_p, c_double_p, c_double_p, c_i32_p, c_float_p, c_i32_p,
                                          C.c_int32, c_i32_p, c_i32_p, c_i32_p, c_i32_p, c_float_p, c_u8_p]
    L.dsh_sfn_estimate.argtypes = [vp, C.POINTER(BbsC), C.c_int, c_double_p, c_double_p, c_float_p, C.c_double, C.c_double, C.c_int, c_double_p, c_double_p,
                                   c_double_p, c_double_p, c_float_p, c_i32_p]
    L.dsh_sfn_estimate_db.argtypes = [vp, C.POINTER(BbsC), vp, C.c_int, c_i32_p, c_double_p, c_double_p, C.c_double, C.c_double, C.c_int, c_double_p, c_double_p,
                                      c_double_p, c_double_p, c_float_p, c_i32_p]
    L.dsh_bbs_bending.argtypes = [C.POINTER(BbsC), C.c_double, c_double_p]
    L.dsh_search_by_schwarp.argtypes = [vp, C.POINTER(BbsC), c_double_p, C.c_int, c_float_p, c_u8_p, c_float_p, c_float_p, C.c_int, C.c_int, C.c_int, c_float_p,
                                        c_u8_p, c_u8_p, C.c_float, C.c_int, c_i32_p, c_i32_p]
    L.dsh_warp_initialize.argtypes = [vp, C.POINTER(BbsC), C.c_int, c_float_p, c_float_p, C.c_double, c_double_p, c_i32_p]
    c_i64_p = C.POINTER(C.c_int64)
    L.dsh_template_embed_device.argtypes = [vp, C.c_int, c_float_p, c_i32_p, c_i32_p, c_float_p]
    L.dsh_scale_min_median.argtypes = [vp, C.c_int, c_float_p, c_float_p, c_double_p, C.c_int64, c_float_p, c_i64_p, c_i32_p]
    L.dsh_optimize_horn.argtypes = [vp, C.c_int, c_float_p, c_float_p, c_double_p, C.c_double, C.c_double, c_i32_p, c_double_p]
    L.dsh_surface_register.argtypes = [vp, C.c_int, c_float_p, c_float_p, c_double_p, C.c_int64, c_float_p, C.c_double, C.c_int, c_i32_p, c_double_p,
                                       c_double_p, c_float_p, c_double_p]
    L.dsh_comm_unique_id.argtypes = [vp]
    L.dsh_comm_create.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.dsh_comm_destroy.argtypes = [vp]
    L.dsh_sft_shared_solve.argtypes = [vp, vp, C.POINTER(SftFrameC), C.POINTER(SftResultC)]
    L.dsh_sft_shared_solve_group.argtypes = [C.c_int, C.POINTER(vp), C.POINTER(SftFrameC), C.POINTER(SftResultC)]
    L.dsh_sft_connected_solve.argtypes = [vp, vp, C.POINTER(SftFrameC), C.POINTER(SftResultC)]
    L.dsh_sft_connected_solve_group.argtypes = [vp, vp, C.POINTER(SftFrameC), C.POINTER(SftResultC)]
    L.dsh_search_by_projection_batch.argtypes = [vp, C.c_int, C.POINTER(TrackProblemC)]
    L.dsh_search_by_projection_frame.argtypes = [vp, C.POINTER(TrackFrameC), C.c_int, c_float_p, c_i32_p, c_u8_p, C.c_float, c_i32_p, c_i32_p]
    L.dsh_search_by_projection_local.argtypes = [vp, C.POINTER(TrackFrameC), C.c_int, c_float_p, c_float_p, c_float_p, c_u8_p, c_u8_p, C.c_float,
                                                 c_i32_p, c_u8_p, c_i32_p, c_i32_p]
    L.dsh_kfdb_create.argtypes = [vp, C.c_int32, C.POINTER(vp)]
    L.dsh_kfdb_destroy.argtypes = [vp]
    L.dsh_kfdb_clear.argtypes = [vp]
    L.dsh_kfdb_add.argtypes = [vp, C.POINTER(MpKeyFrameC), c_i32_p]
    L.dsh_kfdb_set_bad.argtypes = [vp, C.c_int32, C.c_int32]
    L.dsh_kfdb_count.argtypes = [vp]
    L.dsh_mappoint_update.argtypes = [vp, vp, C.c_int, c_float_p, c_i32_p, c_i32_p, c_i32_p, c_i32_p, C.c_int32, c_u8_p, c_i32_p, c_float_p,
                                      c_float_p, c_float_p, c_i32_p]
    i32 = C.c_int32
    L.dsh_mpdb_create.argtypes = [C.POINTER(MpdbDescC), C.POINTER(vp)]
    L.dsh_mpdb_destroy.argtypes = [vp]
    L.dsh_mpdb_clear.argtypes = [vp]
    L.dsh_mpdb_point_count.argtypes = [vp]
    L.dsh_mpdb_keyframe_count.argtypes = [vp]
    L.dsh_mpdb_add_points.argtypes = [vp, C.c_int, c_float_p, c_float_p, c_float_p, c_u8_p, c_u8_p, c_i32_p]
    L.dsh_mpdb_update_points.argtypes = [vp, C.c_int, c_i32_p, i32, c_float_p, c_float_p, c_float_p, c_u8_p]
    L.dsh_mpdb_set_points_bad.argtypes = [vp, C.c_int, c_i32_p, c_u8_p]
    L.dsh_mpdb_add_observations.argtypes = [vp, C.c_int, c_i32_p, c_i32_p]
    L.dsh_mpdb_erase_observations.argtypes = [vp, C.c_int, c_i32_p, c_i32_p]
    L.dsh_mpdb_add_keyframe.argtypes = [vp, i32, c_i32_p, i32, i32, c_i32_p]
    L.dsh_mpdb_set_keyframe_point.argtypes = [vp, i32, i32, i32]
    L.dsh_mpdb_set_keyframe_parent.argtypes = [vp, i32, i32]
    L.dsh_mpdb_set_keyframe_bad.argtypes = [vp, i32, i32]
    L.dsh_local_map_update.argtypes = [vp, C.c_int, c_i32_p, c_u8_p, i32, c_i32_p, c_i32_p, c_i32_p, c_i32_p, c_i32_p, c_i32_p]
    L.dsh_local_map_points.argtypes = [vp, i32, c_i32_p, c_i32_p]
    L.dsh_local_map_search.argtypes = [vp, C.POINTER(TrackFrameC), C.c_float, i32, c_i32_p, c_i32_p, c_u8_p, c_i32_p, c_float_p, c_float_p, c_i32_p]
    L.dsh_trackstate_set_embedding.argtypes = [vp, C.c_int, c_i32_p, c_i32_p, c_double_p]
    L.dsh_trackstate_clear_embedding.argtypes = [vp]
    L.dsh_trackstate_set_counters.argtypes = [vp, C.c_int, c_i32_p, c_i32_p, c_i32_p]
    L.dsh_trackstate_get.argtypes = [vp, C.c_int, c_i32_p, c_i32_p, c_i32_p, c_i32_p, c_float_p]
    L.dsh_trackstate_seed_local_points.argtypes = [vp, C.c_int, c_i32_p]
    L.dsh_trackstate_repose.argtypes = [vp, C.c_int, c_double_p, c_i32_p]
    L.dsh_trackstate_cull.argtypes = [vp, C.c_int, c_i32_p, c_i32_p, i32, c_u8_p]
    L.dsh_track_close_frame.argtypes = [vp, C.POINTER(TrackFrameC), C.c_int, c_i32_p, c_u8_p, C.c_int, c_double_p, i32, C.POINTER(TrackCloseCountsC)]
    L.dsh_track_end_frame.argtypes = [vp, C.c_int, c_i32_p, c_u8_p, c_i32_p, c_i32_p, c_u8_p, C.POINTER(TrackEndCountsC)]
    L.dsh_track_last_frame.argtypes = [vp, i32, c_i32_p, c_i32_p, c_i32_p]
    L.dsh_motion_model_search.argtypes = [vp, C.POINTER(TrackFrameC), C.c_float, C.c_float, i32, c_i32_p, c_i32_p, c_i32_p, c_float_p]
    L.dsh_track_pose_only.argtypes = [vp, C.POINTER(PoseOnlyProblemC)]
    L.dsh_track_pose_only_batch.argtypes = [vp, C.c_int, C.POINTER(PoseOnlyProblemC)]
    L.dsh_track_sft_observations.argtypes = [vp, C.POINTER(TrackSftFrameC), C.POINTER(TrackSftTableC)]
    L.dsh_track_sft.argtypes = [vp, C.POINTER(TrackSftFrameC), i32, C.POINTER(TrackSftTableC), C.POINTER(SftResultC)]
    L.dsh_surface_vertices.argtypes = [C.POINTER(SurfaceGridC), c_double_p]
    L.dsh_need_new_template.argtypes = [vp, i32, C.POINTER(KfKeypointsC), c_i32_p, c_u8_p]
    L.dsh_template_switch.argtypes = [vp, C.POINTER(TemplateSwitchInputC), c_i32_p, C.POINTER(TemplateSwitchCountsC)]
    L.dsh_point_store_get_points.argtypes = [vp, C.c_int, c_i32_p, c_float_p, c_float_p, c_float_p, c_u8_p, c_u8_p]
    L.dsh_point_store_get_embedding.argtypes = [vp, C.c_int, c_i32_p, c_i32_p, c_double_p]
    L.dsh_point_store_add_observations_indexed.argtypes = [vp, C.c_int, c_i32_p, c_i32_p, c_i32_p]
    L.dsh_point_store_set_reference_keyframes.argtypes = [vp, C.c_int, c_i32_p, c_i32_p]
    L.dsh_point_store_get_reference_keyframes.argtypes = [vp, C.c_int, c_i32_p, c_i32_p]
    L.dsh_keyframe_anchors.argtypes = [vp, i32, i32, C.POINTER(AnchorListsC)]
    L.dsh_keyframe_process_new.argtypes = [vp, C.POINTER(KeyframeProcessInputC), c_u8_p, c_i32_p, C.POINTER(KeyframeProcessCountsC)]
    L.dsh_point_store_upkeep.argtypes = [vp, C.POINTER(PointUpkeepInputC), c_i32_p, C.POINTER(PointUpkeepCountsC)]
    L.dsh_point_store_erase_observations.argtypes = [vp, C.c_int, c_i32_p, c_i32_p, i32, c_u8_p, C.POINTER(PointEraseCountsC)]
    L.dsh_point_store_set_bad.argtypes = [vp, C.c_int, c_i32_p, C.POINTER(PointEraseCountsC)]
    L.dsh_point_store_cull.argtypes = [vp, C.c_int, c_i32_p, c_i32_p, i32, c_u8_p, C.POINTER(PointEraseCountsC)]
    L.dsh_point_store_get_observations.argtypes = [vp, C.c_int, c_i32_p, c_i32_p, i32, c_i32_p, c_i32_p, c_i32_p]
    L.dsh_point_store_get_keyframe_table.argtypes = [vp, i32, i32, c_i32_p]
    L.dsh_keyframe_snapshot_positions.argtypes = [vp, i32, c_i32_p]
    L.dsh_keyframe_get_snapshot.argtypes = [vp, i32, i32, c_i32_p, c_float_p]
    L.dsh_keyframe_register_clouds.argtypes = [vp, C.POINTER(KeyframeRegisterInputC), c_i32_p, c_float_p, c_float_p, C.POINTER(KeyframeRegisterResultC)]
    L.dsh_keyframe_register.argtypes = [vp, C.POINTER(KeyframeRegisterInputC), c_i32_p, c_float_p, C.POINTER(KeyframeRegisterResultC)]
    L.dsh_keyframe_set_pose.argtypes = [vp, C.POINTER(KeyframePoseInputC), c_float_p]
    L.dsh_keyframe_get_centre.argtypes = [vp, C.POINTER(KeyframePoseInputC), c_float_p]
    L.dsh_keyframe_surface_init.argtypes = [vp, i32, i32, c_float_p]
    L.dsh_keyframe_surface_set_depth.argtypes = [vp, i32, C.POINTER(BbsC), c_double_p]
    L.dsh_keyframe_surface_set_points.argtypes = [vp, i32, i32, c_i32_p, c_float_p]
    L.dsh_keyframe_surface_set_normals.argtypes = [vp, i32, c_i32_p, c_i32_p, c_float_p, c_i32_p]
    L.dsh_keyframe_surface_take_normals.argtypes = [vp, C.POINTER(SurfaceTakeInputC), c_i32_p]
    L.dsh_keyframe_surface_gather.argtypes = [vp, i32, c_i32_p, c_i32_p, c_float_p, c_u8_p, c_float_p]
    L.dsh_keyframe_surface_get.argtypes = [vp, i32, i32, c_float_p, c_u8_p, c_float_p, c_float_p, c_double_p, C.POINTER(KeyframeSurfaceInfoC)]
    L.dsh_keyframe_surface_vertices.argtypes = [vp, i32, c_float_p, i32, i32, c_double_p]
    L.dsh_keyframe_surface_state.argtypes = [vp, i32]
    L.dsh_keyframe_sfn.argtypes = [vp, C.POINTER(KeyframeSfnInputC), c_double_p, c_double_p, c_float_p, C.POINTER(KeyframeSfnResultC)]
    L.dsh_track_keyframe_candidate.argtypes = [vp, i32, c_i32_p, c_i32_p]
    L.dsh_keyframe_create.argtypes = [vp, C.POINTER(KeyframeCreateInputC), C.POINTER(KeyframeCreateResultC)]
    L.dsh_keyframe_update_connections.argtypes = [vp, i32, i32, i32, c_i32_p, c_i32_p, c_i32_p, c_i32_p, C.POINTER(KeyframeConnectionsC)]
    L.dsh_keyframe_set_view.argtypes = [vp, i32, C.POINTER(KeyframeViewC)]
    L.dsh_keyframe_get_view.argtypes = [vp, i32, C.POINTER(KeyframeViewC), c_float_p]
    L.dsh_keyframe_warp_pair.argtypes = [vp, C.POINTER(WarpPairInputC), C.POINTER(WarpPairResultC)]
    L.dsh_orb_create.argtypes = [C.POINTER(OrbConfigC), C.POINTER(vp)]
    L.dsh_orb_destroy.argtypes = [vp]
    L.dsh_orb_level_sizes.argtypes = [vp, c_i32_p, c_float_p]
    L.dsh_orb_detect.argtypes = [vp, c_u8_p, C.c_int64, c_i32_p, c_i32_p]
    L.dsh_orb_describe.argtypes = [vp, i32, c_i32_p, c_float_p, c_float_p, c_u8_p]
    L.dsh_orb_get_plane.argtypes = [vp, i32, i32, c_u8_p]
    for name in EXPORTED_SYMBOLS:
        fn = getattr(L, name)
        if name not in ("dsh_last_error", "dsh_stream"):
            fn.restype = C.c_int
    if lab:
        L.dsh_lab_set_option.argtypes = [vp, C.c_char_p, C.c_int]
        L.dsh_lab_sft_run_timed.argtypes = [vp, C.c_int, c_double_p]
        L.dsh_lab_sft_assemble_timed.argtypes = [vp, C.c_int, c_double_p]
        L.dsh_lab_sft_phase_ms.argtypes = [vp, C.c_int, c_double_p]
        L.dsh_lab_sft_step_trace.argtypes = [vp, C.c_int, c_double_p]
        L.dsh_lab_sft_system.argtypes = [vp, C.c_int, C.c_int32, c_double_p, c_double_p, c_double_p]
        L.dsh_lab_sft_solver_info.argtypes = [vp, C.c_int, c_i32_p]
        L.dsh_lab_sft_wave_check.argtypes = [vp, C.c_double, C.c_int, C.c_int, c_double_p, c_double_p, c_i32_p, c_double_p]
        L.dsh_lab_sft_dump.argtypes = [vp, C.c_int, C.c_int, C.c_int64, c_double_p]
        L.dsh_lab_sft_rounds_timed.argtypes = [vp, c_double_p, c_i32_p]
        L.dsh_lab_sft_factor_check.argtypes = [vp, c_double_p, c_u8_p, C.c_int, c_double_p, c_i32_p]
        for name in LAB_SYMBOLS:
            getattr(L, name).restype = C.c_int
    return L


class HipEvents:
    """Two HIP events on a caller-chosen stream (libamdhip64 through ctypes): how bench.py times the launches of the
    PRODUCT library on the stream it launches on (dsh_stream) without any timing entry point in the ABI."""

    def __init__(self):
        self._hip = C.CDLL("libamdhip64.so")
        self._hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        self._hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self._hip.hipEventSynchronize.argtypes = [C.c_void_p]
        self._hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self._hip.hipEventDestroy.argtypes = [C.c_void_p]
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        for e in (self.e0, self.e1):
            if self._hip.hipEventCreate(C.byref(e)) != 0:
                raise OSError("hipEventCreate failed")

    def start(self, stream: int):
        if self._hip.hipEventRecord(self.e0, C.c_void_p(stream)) != 0:
            raise OSError("hipEventRecord failed")

    def stop_ms(self, stream: int) -> float:
        ms = C.c_float()
        if (self._hip.hipEventRecord(self.e1, C.c_void_p(stream)) != 0 or self._hip.hipEventSynchronize(self.e1) != 0
                or self._hip.hipEventElapsedTime(C.byref(ms), self.e0, self.e1) != 0):
            raise OSError("HIP event timing failed")
        return float(ms.value)

    def close(self):
        for e in (self.e0, self.e1):
            if e:
                self._hip.hipEventDestroy(e)
        self.e0 = self.e1 = None


HIP_DEVICE_ATTRIBUTE_MULTIPROCESSOR_COUNT = 63   # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h)


def device_cus(device: int = 0) -> int:
    """Compute units of a HIP device (libamdhip64 through ctypes): what the library sizes its launches by (dsh_create)."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipDeviceGetAttribute.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int]
    n = C.c_int(0)
    if hip.hipDeviceGetAttribute(C.byref(n), HIP_DEVICE_ATTRIBUTE_MULTIPROCESSOR_COUNT, int(device)) != 0 or n.value <= 0:
        raise OSError("hipDeviceGetAttribute(hipDeviceAttributeMultiprocessorCount) failed")
    return int(n.value)
