"""Host-side mirror of the map point store and the local map (include/defslam_hip.h: dsh_mpdb_*, dsh_local_map_*):

  * Tracking::UpdateLocalMap = Tracking::UpdateLocalKeyFrames (Thirdparty/ORBSLAM_2/src/Tracking.cc:1510-1629) +
    DefTracking::UpdateLocalPoints (Modules/Tracking/DefTracking.cc:426-454);
  * Tracking::SearchLocalPoints (Tracking.cc:1405-1470) with the resident local points as queries;
  * the back half of DefTracking::TrackLocalMap (DefTracking.cc:253-339) on the store's per-point tracking state (dsh_trackstate_*,
    dsh_track_close_frame): the position write-back of DefPoseOptimization, the counting loops, LocalMapping::MapPointCulling;
  * the end of a tracked frame in DefTracking::Track (CleanMatches, the outlier drop, mLastFrame: DefTracking.cc:169-172, :185-191, :211)
    and the next frame's TrackWithMotionModel (:342-375) with the resident last-frame list as queries (dsh_track_end_frame,
    dsh_motion_model_search);
  * DefLocalMapping::updateTemplate and needNewTemplate (Modules/Mapping/DefLocalMapping.cc:138-153, :355-404) on the store
    (dsh_template_switch, dsh_need_new_template): the occupancy mask, the new map points, the embedding in the new template;
  * what SchwarpDatabase::add (Modules/Mapping/SchwarpDatabase.cc:61-106) and DefORBmatcher::searchBySchwarp
    (Modules/Matching/DefORBmatcher.cc:200-211) read of the map for a new keyframe (dsh_keyframe_anchors): its anchor keyframes, the
    matched key point indices and the search queries per anchor;
  * LocalMapping::ProcessNewKeyFrame's loop (Thirdparty/ORBSLAM_2/src/LocalMapping.cc:142-165) and the upkeep of DefMapPoint::Repose
    (Modules/Common/DefMapPoint.cc:122-126) with the observation lists read from the store's log (dsh_keyframe_process_new,
    dsh_point_store_upkeep): AddObservation, UpdateNormalAndDepth, ComputeDistinctiveDescriptors, results written into the store;
  * MapPoint::EraseObservation (MapPoint.cc:122-148), DefMapPoint::setBadFlag (DefMapPoint.cc:76-94) and LocalMapping::MapPointCulling
    (LocalMapping.cc:173-199) in full on the store's log and tables (dsh_point_store_erase_observations, dsh_point_store_set_bad,
    dsh_point_store_cull), with the read-backs of a point's observations and a keyframe's table;
  * DefKeyFrame's PosesKeyframes snapshot (Modules/Common/DefKeyFrame.cc:60-74) and SurfaceRegistration::registerSurfaces
    (Modules/Mapping/SurfaceRegistration.cc:48-153) with the clouds selected from the store and the snapshot, Surface::applyScale and the
    camera centre of KeyFrame::SetPose written into the keyframe store (dsh_keyframe_snapshot_positions, dsh_keyframe_register,
    dsh_keyframe_set_pose);
  * DefTracking::CreateNewKeyFrame (Modules/Tracking/DefTracking.cc:696-707) in one call on both stores, with the table taken on the
    device from the keyframe candidate the end of the frame left there, and KeyFrame::UpdateConnections
    (Thirdparty/ORBSLAM_2/src/KeyFrame.cc:326-419) over the observation log, which gives the keyframe its parent
    (dsh_track_keyframe_candidate, dsh_keyframe_create, dsh_keyframe_update_connections);
  * the per-anchor body of SchwarpDatabase::add (SchwarpDatabase.cc:107-117): DefORBmatcher::findbyWarp and
    SchwarpDatabase::calculateSchwarps with the key points, descriptor rows and tables read from the stores
    (dsh_keyframe_set_view, dsh_keyframe_warp_pair).

The map points, who observes whom, and the keyframes' point tables and spanning tree stay in HBM (MapPointStore); the work runs on the
device (localmap_kernels.hip, track_kernels.hip), there is no CPU fallback.  Where the reference iterates pointer-ordered containers the
order here is the index: keyframes by ascending slot, points by ascending id.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from .sft import Context, _ptr
from .track import TrackFrame

POSITION = _lib.DSH_MPDB_POSITION
NORMAL_DEPTH = _lib.DSH_MPDB_NORMAL_DEPTH
DESCRIPTOR = _lib.DSH_MPDB_DESCRIPTOR


@dataclass
class LocalMap:
    """What dsh_local_map_update returns."""
    frame_bad: np.ndarray               # (N,) bool: the frame held a bad point there (the reference nulls the entry)
    local_kf: np.ndarray                # mvpLocalKeyFrames as slots
    votes: np.ndarray                   # the votes of its first n_voted entries
    ref_kf: int                         # pKFmax, or -1: leave mpReferenceKF as it is
    n_local_points: int                 # len(mvpLocalMapPoints); the ids stay on the device (MapPointStore.local_points)


@dataclass
class LocalSearch:
    """What dsh_local_map_search returns, per local point in ascending id."""
    local_ids: np.ndarray
    match: np.ndarray                   # key point index or -1
    in_view: np.ndarray                 # mbTrackInView
    level: np.ndarray                   # mnTrackScaleLevel
    uv: np.ndarray                      # (Q,2) mTrackProjX, mTrackProjY
    view_cos: np.ndarray                # mTrackViewCos
    nmatches: int


@dataclass
class PointState:
    """What dsh_trackstate_get returns, per id asked for."""
    visible: np.ndarray                 # mnVisible
    found: np.ndarray                   # mnFound
    n_obs: np.ndarray                   # MapPoint::nObs (stale after the point became bad, like the reference)
    xyz: np.ndarray                     # (n,3) float32 mWorldPos


@dataclass
class CloseCounts:
    """What dsh_track_close_frame returns (DefTracking.cc:253-328)."""
    matches_inliers: int                # mnMatchesInliers: decides whether the tracking succeeded
    matches_outliers: int               # mnMatchesOutliers
    to_match_local: int                 # DefnToMatchLOCAL
    observed: int                       # observedFrame
    inliers: int                        # mI  } the Matches.txt row
    outliers: int                       # mO  }
    local_map_points: int               # numberLocalMapPoints
    n_moved: int                        # points the repose moved


@dataclass
class EndFrame:
    """What dsh_track_end_frame returns (DefTracking.cc:169-172, :185-191, :211)."""
    points: np.ndarray                  # (N,) mvpMapPoints after CleanMatches: what CreateNewKeyFrame copies, outliers included
    outlier: np.ndarray                 # (N,) bool mvbOutlier after CleanMatches
    cleaned: int                        # entries CleanMatches emptied
    dropped: int                        # outliers emptied afterwards
    kept: int                           # entries of the resident last-frame list that hold a point


@dataclass
class LastFrame:
    """The resident last-frame list (dsh_track_last_frame)."""
    ids: np.ndarray                     # (N,) the point each key point of the last frame holds, or -1
    octave: np.ndarray                  # (N,) its octave, -1 where the entry is empty


@dataclass
class MotionModelSearch:
    """What dsh_motion_model_search returns (DefTracking::TrackWithMotionModel from the store)."""
    frame_points: np.ndarray            # (N,) mvpMapPoints of the current frame as ids or -1
    match: np.ndarray                   # (N_last,) the key point each last-frame entry took, or -1
    nmatches: int
    th_used: float                      # th or th_wide: the search that produced the result
    ok: bool                            # TrackWithMotionModel's return value (nmatches >= 15, :373)


@dataclass
class PoseOnlyFrame:
    """What dsh_track_pose_only reads of a frame (ORB_SLAM2::Optimizer::poseOptimization, monocular)."""
    Tcw: np.ndarray                     # (4,4) float32 mTcw
    K: np.ndarray                       # fx, fy, cx, cy
    kp: np.ndarray                      # (N,2) float32 mvKeysUn
    octave: np.ndarray                  # (N,) mvKeysUn[i].octave
    inv_level_sigma2: np.ndarray        # (levels,) float32 mvInvLevelSigma2
    frame_points: np.ndarray            # (N,) mvpMapPoints as ids or -1
    outlier: Optional[np.ndarray] = None   # (N,) mvbOutlier on entry (None: all False); kept where no point is held


@dataclass
class PoseOnly:
    """What dsh_track_pose_only returns."""
    outlier: np.ndarray                 # (N,) bool mvbOutlier: written where a point is held
    Tcw: np.ndarray                     # (4,4) float32: the pose SetPose receives; the input pose when n_initial < 3
    pose: np.ndarray                    # (7,) t, q (x y z w) of the recovered SE3Quat
    n_initial: int
    n_bad: int                          # nBad of the last round run
    n_good: int                         # the return value
    rounds: int                         # 0, 1 or 4
    iters: np.ndarray                   # (4,) outer iterations per round
    trials: np.ndarray                  # (4,) damping trials per round
    bad: np.ndarray                     # (4,) nBad after each round
    chi2: np.ndarray                    # (4,) active robust chi2 of the last accepted state per round


@dataclass
class SftObservations:
    """What dsh_track_sft_observations returns: the observation table of DefPoseOptimization (DefOptimizer.cc:293-361), by key point."""
    kp_index: np.ndarray                # (M,) the key point of each row, ascending
    point_id: np.ndarray                # (M,) the point it holds
    nodes: np.ndarray                   # (M,3) int32: obs_nodes, the store's bytes
    bary: np.ndarray                    # (M,3) float64: obs_bary, the store's bytes
    uv: np.ndarray                      # (M,2) float64: the float32 key point
    invsig2: np.ndarray                 # (M,) float64: the float32 mvInvLevelSigma2[octave]
    points_obs: int                     # Points_Obs: key points that hold a point and are no outlier, bad points included


@dataclass
class TrackSft:
    """What dsh_track_sft returns: the result of dsh_sft_solve on the table, and mvbOutlier of the frame."""
    outlier: np.ndarray                 # (N,) bool mvbOutlier: written at table.kp_index, kept elsewhere
    table: SftObservations
    Tcw: np.ndarray                     # (4,4) float32: the pose SetPose receives
    pose7: np.ndarray                   # (7,) t, q (x y z w)
    xyz: np.ndarray                     # (n,3) float64 node positions
    chi2_obs: np.ndarray                # (M,) per row
    row_outlier: np.ndarray             # (M,) bool per row
    mappoint_xyz: np.ndarray            # (M,3) float32 per row
    rep_error: float                    # NaN when the table is empty
    inliers: int
    iters: int
    trials: int
    dim: int
    half_bandwidth: int
    status: int


@dataclass
class StoredPoints:
    """What dsh_point_store_get_points returns, per id asked for."""
    xyz: np.ndarray                     # (n,3) float32 mWorldPos
    normal: np.ndarray                  # (n,3) float32 mNormalVector
    max_distance: np.ndarray            # (n,) float32 mfMaxDistance
    desc: np.ndarray                    # (n,32) uint8 mDescriptor
    bad: np.ndarray                     # (n,) bool


@dataclass
class KeyFramePoints:
    """What the occupancy mask reads of a keyframe (dsh_kf_keypoints)."""
    rows: int                           # imGray.rows
    cols: int                           # imGray.cols
    kp: np.ndarray                      # (N,2) float32 mvKeysUn[i].pt

    def c(self, keep: list) -> _lib.KfKeypointsC:
        kp = np.ascontiguousarray(self.kp, np.float32).reshape(-1, 2)
        keep.append(kp)
        return _lib.KfKeypointsC(int(self.rows), int(self.cols), int(kp.shape[0]), _ptr(kp, C.c_float))


@dataclass
class TemplateSwitch:
    """What dsh_template_switch returns (DefLocalMapping::updateTemplate on the store)."""
    n_new: int                          # points created: ids first_id .. first_id + n_new - 1
    first_id: int
    n_moved: int                        # key points that hold a point that is not bad
    n_masked: int                       # empty key points inside the occupancy mask
    n_embedded: int                     # points with a facet afterwards
    n_points: int                       # the store's size afterwards
    new_idx: np.ndarray                 # (n_new,) the key point of each new point


@dataclass
class KeyframeAnchors:
    """What dsh_keyframe_anchors returns: the anchors by ascending slot, the pairs and queries of the anchors that reached min_pairs as CSR."""
    anchor_slot: np.ndarray             # (A,) the reference keyframes of the new keyframe's points
    anchor_count: np.ndarray            # (A,) countKFMatches
    anchor_pairs: np.ndarray            # (A,) len(vMatchedIndices), below min_pairs or not
    pair_ptr: np.ndarray                # (A+1,)
    pair_idx1: np.ndarray               # key point in the anchor
    pair_idx2: np.ndarray               # key point in the new keyframe
    pair_point: np.ndarray              # the shared point
    pair_own: np.ndarray                # bool: the anchor is the point's reference keyframe (its record is stored after the fit)
    query_ptr: np.ndarray               # (A+1,)
    query_idx1: np.ndarray              # entries of the anchor's table that searchBySchwarp looks for in the new keyframe
    query_point: np.ndarray
    has: np.ndarray                     # (N,) bool: the new keyframe's entry holds a point
    n_no_ref: int                       # entries whose point has no reference keyframe

    def pairs(self, a: int):
        """vMatchedIndices of anchor a: (idx1, idx2) rows."""
        s = slice(self.pair_ptr[a], self.pair_ptr[a + 1])
        return np.stack([self.pair_idx1[s], self.pair_idx2[s]], 1)

    def queries(self, a: int) -> np.ndarray:
        return self.query_idx1[self.query_ptr[a]:self.query_ptr[a + 1]]


@dataclass
class NewKeyframe:
    """What dsh_keyframe_process_new returns (LocalMapping::ProcessNewKeyFrame's loop on the stores)."""
    action: np.ndarray                  # (N,) KF_EMPTY, KF_BAD_POINT, KF_ADDED or KF_RECENT per table entry
    added: np.ndarray                   # (n_added,) the points that got the observation and the upkeep, by ascending entry
    n_empty: int
    n_bad: int
    n_added: int
    n_recent: int                       # entries for the caller's mlpRecentAddedMapPoints
    n_no_good_desc: int                 # added points whose observing keyframes are all bad: descriptor unchanged
    n_no_ref: int                       # added points without a reference keyframe: normal and range unchanged
    first_record: int                   # log position of the first record appended


@dataclass
class Upkeep:
    """What dsh_point_store_upkeep returns."""
    status: Optional[np.ndarray]        # (n,) UPKEEP_* flags per id; None for the embedded selection
    n_selected: int                     # points the selection names that are not bad
    n_no_obs: int
    n_no_good_desc: int
    n_no_ref: int
    n_bad: int                          # ids that name a bad point


@dataclass
class EraseCounts:
    """dsh_point_erase_counts."""
    n_found: int                        # pairs whose record was live (erase_observations_full only)
    n_ref_moved: int                    # points whose reference keyframe changed
    n_set_bad: int                      # points setBadFlag ran on
    n_records: int                      # log records blanked, the pairs' own included
    n_entries: int                      # table entries written to -1, once per record that names them


@dataclass
class ObservationErase:
    """What dsh_point_store_erase_observations returns."""
    status: np.ndarray                  # (n,) ERASE_NOT_STORED, ERASE_DONE or ERASE_SET_BAD per pair
    counts: EraseCounts


@dataclass
class PointCull:
    """What dsh_point_store_cull returns."""
    action: np.ndarray                  # (n,) CULL_* per entry of mlpRecentAddedMapPoints
    counts: EraseCounts


@dataclass
class PointObservations:
    """What dsh_point_store_get_observations returns: MapPoint::GetObservations of the ids as a CSR by ascending slot."""
    ptr: np.ndarray                     # (n+1,)
    slots: np.ndarray                   # the observing keyframes
    idx: np.ndarray                     # the key point index in each, -1: added without one

    def of(self, i: int) -> dict:
        """mObservations of the i-th id asked for: {slot: idx} in slot order."""
        s = slice(self.ptr[i], self.ptr[i + 1])
        return dict(zip(self.slots[s].tolist(), self.idx[s].tolist()))


@dataclass
class KeyframeClouds:
    """What dsh_keyframe_register_clouds returns: the pairs of SurfaceRegistration.cc:60-104 in ascending entry order."""
    pair_idx: np.ndarray                # (n_pairs,) the table entry of each pair
    cloud_surface: np.ndarray           # (n_pairs,3) float32 cloud2pc: the surface points in world coordinates
    cloud_map: np.ndarray               # (n_pairs,3) float32 cloud1pc: PosesKeyframes of the points
    n_pairs: int
    n_empty: int                        # entries without a point
    n_bad: int                          # entries whose point is bad
    n_no_facet: int                     # entries whose point has no facet now
    n_no_snapshot: int                  # entries whose point has no snapshot for this keyframe


@dataclass
class KeyframeRegistration:
    """What dsh_keyframe_register returns (SurfaceRegistration::registerSurfaces from the stores)."""
    pair_idx: np.ndarray
    n_pairs: int
    n_empty: int
    n_bad: int
    n_no_facet: int
    n_no_snapshot: int
    registered: bool
    stream_status: int                  # 1: the stream u is shorter than the reference's draws
    consumed: int                       # draws of u the reference makes
    sim3: np.ndarray                    # (8,) qx qy qz qw tx ty tz s
    s22: float                          # the recovered scale
    info: np.ndarray                    # (8,) as dsh_surface_register
    Tcw_new: np.ndarray                 # (4,4) float32: the pose SetPose receives
    Ow_new: np.ndarray                  # (3,) float32: its camera centre
    surface_scaled: Optional[np.ndarray]   # (N,3) float32 Surface::applyScale of the surface points; None when not registered


@dataclass
class KeyframeSurface:
    """What dsh_keyframe_surface_get returns: the resident defSLAM::Surface of a keyframe."""
    normals: np.ndarray                 # (N,3) float32 SurfacePoint::Normal, zeros where none was set
    has_normal: np.ndarray              # (N,) bool SurfacePoint::NormalOn
    pts: np.ndarray                     # (N,3) float32 SurfacePoint::x3D
    kpn: np.ndarray                     # (N,2) float32 mpKeypointNorm
    ctrl: Optional[np.ndarray]          # (nptsu * nptsv,) float64 nodesDepth_; None without a depth spline
    bbs: object                         # nrsfm.Bbs of the depth spline; None without one
    n_normals: int                      # numberofNormals_
    enough_normals: bool                # Surface::enoughNormals


@dataclass
class SurfaceGather:
    """What dsh_keyframe_surface_gather returns: x0 / has_x0 / ref_uv of a normal solve."""
    normal_xy: np.ndarray               # (n,2) float32 Ni(0), Ni(1); zeros without a normal
    has: np.ndarray                     # (n,) uint8 Surface::getNormalSurfacePoint's return value
    uv: np.ndarray                      # (n,2) float32 mpKeypointNorm


@dataclass
class KeyframeSfn:
    """What dsh_keyframe_sfn returns (ShapeFromNormals::estimate of a keyframe from the store)."""
    ok: bool
    n_sites: int
    n_empty: int                        # entries without a point
    n_bad: int                          # entries whose point is bad
    n_no_normal: int                    # entries without a normal
    n_nan: int                          # entries whose normal has a NaN component
    ctrl_raw: np.ndarray                # (nptsu * nptsv,) float64 the control points before the scaling
    ctrl: Optional[np.ndarray]          # the scaled control points, None when not ok
    pts: Optional[np.ndarray]           # (N,3) float32 the surface points, None when not ok


# dsh_point_store_erase_observations: what became of a pair
ERASE_NOT_STORED, ERASE_DONE, ERASE_SET_BAD = 0, 1, 2

# dsh_keyframe_process_new: what became of a table entry
KF_EMPTY, KF_BAD_POINT, KF_ADDED, KF_RECENT = 0, 1, 2, 3
# dsh_point_store_upkeep: the parts to update, and the status flags per point
UPKEEP_DESCRIPTOR, UPKEEP_NORMAL_DEPTH, UPKEEP_BOTH = _lib.DSH_MP_DESCRIPTOR, _lib.DSH_MP_NORMAL_DEPTH, _lib.DSH_MP_DESCRIPTOR | _lib.DSH_MP_NORMAL_DEPTH
UPKEEP_NO_OBS, UPKEEP_NO_GOOD_DESC, UPKEEP_NO_REF, UPKEEP_SKIPPED_BAD = (_lib.DSH_MP_NO_OBS, _lib.DSH_MP_NO_GOOD_DESC, _lib.DSH_MP_NO_REF,
                                                                         _lib.DSH_MP_SKIPPED_BAD)

# dsh_trackstate_cull: what became of an entry of mlpRecentAddedMapPoints
CULL_STAYS, CULL_WAS_BAD, CULL_SET_BAD, CULL_OLD = 0, 1, 2, 3


@dataclass
class KeyframeCreation:
    """What dsh_keyframe_create returns (DefTracking::CreateNewKeyFrame on the two stores)."""
    slot: int                           # of the new keyframe, in both stores
    n_held: int                         # table entries that hold a point
    n_snapshot: int                     # entries whose position was taken (DefKeyFrame.cc:60-74)
    Ow: np.ndarray                      # (3,) float32 the camera centre written


@dataclass
class KeyframeConnections:
    """What dsh_keyframe_update_connections returns (KeyFrame::UpdateConnections, KeyFrame.cc:326-419)."""
    counted_kf: np.ndarray              # mConnectedKeyFrameWeights: the keyframes with a weight > 0 by ascending slot
    counted_w: np.ndarray               # their weights
    ordered_kf: np.ndarray              # mvpOrderedConnectedKeyFrames: descending weight, among equals descending slot
    ordered_w: np.ndarray               # mvOrderedWeights
    parent: int                         # the keyframe's parent after the call, -1: none
    parent_set: bool                    # this call set it (the first connection)
    max_weight: int                     # nmax
    max_kf: int                         # pKFmax, -1 when no weight is positive


@dataclass
class KeyframeView:
    """What warp_pair reads of a keyframe beyond its Surface (dsh_keyframe_view)."""
    kp_px: np.ndarray                   # (N,2) float32 mvKeysUn[i].pt
    K: tuple                            # fx, fy, cx, cy
    bounds: tuple                       # mnMinX, mnMaxX, mnMinY, mnMaxY
    grid_cols: int
    grid_rows: int
    warp_grid: object                   # nrsfm.Bbs: umin, umax, NCu, vmin, vmax, NCv, valdim


WARP_NO_MATCH, WARP_FILTERED, WARP_UNFITTED, WARP_SKIPPED, WARP_DROPPED, WARP_KEPT, WARP_STORED = range(7)


@dataclass
class WarpPair:
    """One anchor of SchwarpDatabase::add (dsh_keyframe_warp_pair)."""
    x: np.ndarray                       # (2 NCu NCv,) the fitted warp, or the initialisation when not fitted
    init_ok: bool
    fitted: bool
    info: np.ndarray                    # iterations, accepted steps
    costs: np.ndarray                   # initial, final
    pair_state: np.ndarray              # WARP_* per pair
    query_state: np.ndarray             # WARP_* per query
    query_match: np.ndarray             # idx2 or -1
    query_point: np.ndarray             # the point a matched query registered, -1: none
    query_added: np.ndarray             # bool: the query's observation record was appended
    first_record: int
    counts: dict                        # n_filtered, n_matched, n_appended, n_list, n_skipped, n_dropped, n_kept, n_stored, rounds
    erase: dict                         # n_found, n_ref_moved, n_set_bad, n_records, n_entries


def _i32(a):
    return np.ascontiguousarray(a, np.int32).reshape(-1)


class MapPointStore:
    """dsh_mpdb: map points, observations and keyframe tables resident in HBM."""

    def __init__(self, ctx: Context, points: int = 4096, keyframes: int = 64, observations: int = 1 << 16):
        self._ctx, self._h = ctx, None
        self._n_last = 0                                       # length of the resident last-frame list (the N of the last end_frame)
        self._kf_n = []                                        # key points per keyframe slot
        d = _lib.MpdbDescC(ctx._h, int(points), int(keyframes), int(observations))
        h = C.c_void_p()
        ctx._check(ctx._L.dsh_mpdb_create(C.byref(d), C.byref(h)), "dsh_mpdb_create")
        self._h = h

    def close(self):
        if self._h is not None:
            self._ctx._L.dsh_mpdb_destroy(self._h)
            self._h = None

    __del__ = close

    def _call(self, name, *args):
        self._ctx._check(getattr(self._ctx._L, name)(self._h, *args), name)

    def clear(self):
        self._call("dsh_mpdb_clear")
        self._n_last = 0
        self._kf_n = []

    @property
    def n_points(self) -> int:
        return int(self._ctx._L.dsh_mpdb_point_count(self._h))

    @property
    def n_keyframes(self) -> int:
        return int(self._ctx._L.dsh_mpdb_keyframe_count(self._h))

    # ---- points ----
    def add_points(self, xyz, normal, max_distance, desc, bad=None) -> int:
        """Returns the id of the first new point; the others follow."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = xyz.shape[0]
        nrm = np.ascontiguousarray(normal, np.float32).reshape(n, 3)
        md = np.ascontiguousarray(max_distance, np.float32).reshape(n)
        ds = np.ascontiguousarray(desc, np.uint8).reshape(n, 32)
        b = None if bad is None else np.ascontiguousarray(bad, np.uint8).reshape(n)
        first = C.c_int32(-1)
        self._call("dsh_mpdb_add_points", n, _ptr(xyz, C.c_float), _ptr(nrm, C.c_float), _ptr(md, C.c_float), _ptr(ds, C.c_uint8), _ptr(b, C.c_uint8),
                   C.byref(first))
        return int(first.value)

    def update_points(self, ids, xyz=None, normal=None, max_distance=None, desc=None):
        """Overwrite what is given: xyz (the RecalculatePosition write-back), normal with max_distance, desc."""
        ids = _i32(ids)
        n = ids.shape[0]
        what = (POSITION if xyz is not None else 0) | (NORMAL_DEPTH if normal is not None else 0) | (DESCRIPTOR if desc is not None else 0)
        xyz = None if xyz is None else np.ascontiguousarray(xyz, np.float32).reshape(n, 3)
        nrm = None if normal is None else np.ascontiguousarray(normal, np.float32).reshape(n, 3)
        md = None if max_distance is None else np.ascontiguousarray(max_distance, np.float32).reshape(n)
        ds = None if desc is None else np.ascontiguousarray(desc, np.uint8).reshape(n, 32)
        self._call("dsh_mpdb_update_points", n, _ptr(ids, C.c_int32), what, _ptr(xyz, C.c_float), _ptr(nrm, C.c_float), _ptr(md, C.c_float),
                   _ptr(ds, C.c_uint8))

    def set_points_bad(self, ids, bad=None):
        ids = _i32(ids)
        b = None if bad is None else np.ascontiguousarray(bad, np.uint8).reshape(ids.shape[0])
        self._call("dsh_mpdb_set_points_bad", ids.shape[0], _ptr(ids, C.c_int32), _ptr(b, C.c_uint8))

    # ---- observations ----
    def add_observations(self, point_ids, keyframe_slots, idx=None):
        """MapPoint::AddObservation; idx: the key point index of each observation in its keyframe (needed by keyframe_anchors)."""
        p, k = _i32(point_ids), _i32(keyframe_slots)
        if idx is None:
            self._call("dsh_mpdb_add_observations", p.shape[0], _ptr(p, C.c_int32), _ptr(k, C.c_int32))
        else:
            i = _i32(idx)
            self._call("dsh_point_store_add_observations_indexed", p.shape[0], _ptr(p, C.c_int32), _ptr(k, C.c_int32), _ptr(i, C.c_int32))

    def erase_observations(self, point_ids, keyframe_slots):
        p, k = _i32(point_ids), _i32(keyframe_slots)
        self._call("dsh_mpdb_erase_observations", p.shape[0], _ptr(p, C.c_int32), _ptr(k, C.c_int32))

    def set_reference_keyframes(self, ids, slots):
        """MapPoint::GetReferenceKeyFrame of ids: a slot each, or -1."""
        ids, sl = _i32(ids), _i32(slots)
        self._call("dsh_point_store_set_reference_keyframes", ids.shape[0], _ptr(ids, C.c_int32), _ptr(sl, C.c_int32))

    def get_reference_keyframes(self, ids=None) -> np.ndarray:
        ids = np.arange(self.n_points, dtype=np.int32) if ids is None else _i32(ids)
        out = np.full(max(ids.shape[0], 1), -1, np.int32)
        self._call("dsh_point_store_get_reference_keyframes", ids.shape[0], _ptr(ids, C.c_int32), _ptr(out, C.c_int32))
        return out[:ids.shape[0]]

    # ---- keyframes ----
    def add_keyframe(self, points, parent: int = -1, bad: bool = False) -> int:
        t = _i32(points)
        slot = C.c_int32(-1)
        self._call("dsh_mpdb_add_keyframe", t.shape[0], _ptr(t, C.c_int32), int(parent), 1 if bad else 0, C.byref(slot))
        self._kf_n.append(t.shape[0])
        return int(slot.value)

    def set_keyframe_point(self, slot: int, idx: int, point_id: int):
        self._call("dsh_mpdb_set_keyframe_point", int(slot), int(idx), int(point_id))

    def set_keyframe_parent(self, slot: int, parent: int):
        self._call("dsh_mpdb_set_keyframe_parent", int(slot), int(parent))

    def set_keyframe_bad(self, slot: int, bad: bool = True):
        self._call("dsh_mpdb_set_keyframe_bad", int(slot), 1 if bad else 0)

    # ---- the local map ----
    def update_local_map(self, frame_points) -> LocalMap:
        """Tracking::UpdateLocalMap for a frame whose mvpMapPoints are frame_points (ids or -1)."""
        fp = _i32(frame_points)
        N, K = fp.shape[0], max(self.n_keyframes, 1)
        fb = np.zeros(N, np.uint8)
        kf, votes = np.full(K, -1, np.int32), np.zeros(K, np.int32)
        nv, nk, ref, npts = C.c_int32(0), C.c_int32(0), C.c_int32(-1), C.c_int32(0)
        self._call("dsh_local_map_update", N, _ptr(fp, C.c_int32), _ptr(fb, C.c_uint8), K, _ptr(kf, C.c_int32), _ptr(votes, C.c_int32), C.byref(nv),
                   C.byref(nk), C.byref(ref), C.byref(npts))
        return LocalMap(frame_bad=fb.astype(bool), local_kf=kf[:nk.value].copy(), votes=votes[:nv.value].copy(), ref_kf=int(ref.value),
                        n_local_points=int(npts.value))

    def local_points(self, n: int) -> np.ndarray:
        """The resident local point ids of the last update (n = LocalMap.n_local_points)."""
        ids = np.zeros(max(int(n), 1), np.int32)
        got = C.c_int32(0)
        self._call("dsh_local_map_points", int(n), _ptr(ids, C.c_int32), C.byref(got))
        return ids[:got.value].copy()

    def search_local_points(self, frame: TrackFrame, n_local_points: int, th: float = 3.0) -> LocalSearch:
        """Tracking::SearchLocalPoints from the store; frame.state as for the local-map search (track.local_points_search)."""
        keep = []
        f = frame.c(keep)
        Q = int(n_local_points)
        m = max(Q, 1)
        ids, match = np.zeros(m, np.int32), np.full(m, -1, np.int32)
        iv, lev, uv, vc = np.zeros(m, np.uint8), np.zeros(m, np.int32), np.zeros((m, 2), np.float32), np.zeros(m, np.float32)
        nm = C.c_int32(0)
        self._call("dsh_local_map_search", C.byref(f), float(th), Q, _ptr(ids, C.c_int32), _ptr(match, C.c_int32), _ptr(iv, C.c_uint8),
                   _ptr(lev, C.c_int32), _ptr(uv, C.c_float), _ptr(vc, C.c_float), C.byref(nm))
        return LocalSearch(local_ids=ids[:Q], match=match[:Q], in_view=iv[:Q].astype(bool), level=lev[:Q], uv=uv[:Q], view_cos=vc[:Q],
                           nmatches=int(nm.value))

    # ---- the per-point tracking state and the end of a tracked frame ----
    def set_embedding(self, ids, nodes, bary=None):
        """DefMapPoint::SetFacet + SetCoordinates: nodes (n,3) ascending node indices (-1 -1 -1 removes the facet), bary (n,3) in that order."""
        ids = _i32(ids)
        n = ids.shape[0]
        nd = np.ascontiguousarray(nodes, np.int32).reshape(n, 3)
        b = None if bary is None else np.ascontiguousarray(bary, np.float64).reshape(n, 3)
        self._call("dsh_trackstate_set_embedding", n, _ptr(ids, C.c_int32), _ptr(nd, C.c_int32), _ptr(b, C.c_double))

    def clear_embedding(self):
        """DefMap::clearTemplate: every point loses its facet."""
        self._call("dsh_trackstate_clear_embedding")

    def set_counters(self, ids, visible, found):
        ids = _i32(ids)
        v, f = _i32(visible), _i32(found)
        self._call("dsh_trackstate_set_counters", ids.shape[0], _ptr(ids, C.c_int32), _ptr(v, C.c_int32), _ptr(f, C.c_int32))

    def get_state(self, ids=None) -> PointState:
        """mnVisible, mnFound, nObs and the position of ids (None: every point of the store)."""
        ids = np.arange(self.n_points, dtype=np.int32) if ids is None else _i32(ids)
        n = ids.shape[0]
        m = max(n, 1)
        v, f, o, x = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros((m, 3), np.float32)
        self._call("dsh_trackstate_get", n, _ptr(ids, C.c_int32), _ptr(v, C.c_int32), _ptr(f, C.c_int32), _ptr(o, C.c_int32), _ptr(x, C.c_float))
        return PointState(visible=v[:n], found=f[:n], n_obs=o[:n], xyz=x[:n])

    def seed_local_points(self, ids):
        """DefTracking::MonocularInitialization: the local list and the reference list become ids (ascending)."""
        ids = _i32(ids)
        self._call("dsh_trackstate_seed_local_points", ids.shape[0], _ptr(ids, C.c_int32))

    def repose(self, node_xyz) -> int:
        """DefOptimizer.cc:568-576: every point that is not bad and has a facet moves to its barycentric position; returns how many."""
        x = np.ascontiguousarray(node_xyz, np.float64).reshape(-1, 3)
        moved = C.c_int32(0)
        self._call("dsh_trackstate_repose", x.shape[0], _ptr(x, C.c_double), C.byref(moved))
        return int(moved.value)

    def cull(self, ids, first_kf, current_kf: int) -> np.ndarray:
        """LocalMapping::MapPointCulling over ids (mnFirstKFid in first_kf): CULL_* per entry; CULL_SET_BAD points are bad in the store."""
        ids, fk = _i32(ids), _i32(first_kf)
        act = np.zeros(max(ids.shape[0], 1), np.uint8)
        self._call("dsh_trackstate_cull", ids.shape[0], _ptr(ids, C.c_int32), _ptr(fk, C.c_int32), int(current_kf), _ptr(act, C.c_uint8))
        return act[:ids.shape[0]]

    def close_frame(self, frame: TrackFrame, frame_points, outlier, node_xyz=None, only_tracking: bool = False) -> CloseCounts:
        """The rest of DefTracking::TrackLocalMap after the optimisation: frame carries the pose after SetPose (only Tcw, Ow, K and bounds are
        read), frame_points / outlier are mvpMapPoints (ids or -1) / mvbOutlier, node_xyz the optimised nodes (None: no position changes)."""
        keep = []
        f = frame.c(keep)
        fp = _i32(frame_points)
        out = np.ascontiguousarray(outlier, np.uint8).reshape(fp.shape[0])
        x = None if node_xyz is None else np.ascontiguousarray(node_xyz, np.float64).reshape(-1, 3)
        cc = _lib.TrackCloseCountsC()
        self._call("dsh_track_close_frame", C.byref(f), fp.shape[0], _ptr(fp, C.c_int32), _ptr(out, C.c_uint8), 0 if x is None else x.shape[0],
                   _ptr(x, C.c_double), 1 if only_tracking else 0, C.byref(cc))
        return CloseCounts(**{n: int(getattr(cc, n)) for n, _ in _lib.TrackCloseCountsC._fields_})

    # ---- the end of a frame and the next frame's motion-model search ----
    def end_frame(self, frame_points, outlier, octave) -> EndFrame:
        """CleanMatches, the outlier drop and mLastFrame = Frame(*mCurrentFrame): frame_points / outlier / octave are mvpMapPoints (ids or
        -1) / mvbOutlier / mvKeys[i].octave; the result of the two loops stays in the store as the last-frame list."""
        fp = _i32(frame_points)
        N = fp.shape[0]
        out = np.ascontiguousarray(outlier, np.uint8).reshape(N)
        oc = _i32(octave).reshape(N)
        m = max(N, 1)
        pts, flag = np.full(m, -1, np.int32), np.zeros(m, np.uint8)
        cc = _lib.TrackEndCountsC()
        self._call("dsh_track_end_frame", N, _ptr(fp, C.c_int32), _ptr(out, C.c_uint8), _ptr(oc, C.c_int32), _ptr(pts, C.c_int32), _ptr(flag, C.c_uint8),
                   C.byref(cc))
        self._n_last = N
        return EndFrame(points=pts[:N], outlier=flag[:N].astype(bool), cleaned=int(cc.cleaned), dropped=int(cc.dropped), kept=int(cc.kept))

    def last_frame(self, capacity: int = 8192) -> LastFrame:
        """The resident last-frame list (capacity: at least its length; a frame has at most 8192 key points)."""
        m = max(int(capacity), 1)
        ids, oc = np.full(m, -1, np.int32), np.full(m, -1, np.int32)
        n = C.c_int32(0)
        self._call("dsh_track_last_frame", int(capacity), _ptr(ids, C.c_int32), _ptr(oc, C.c_int32), C.byref(n))
        return LastFrame(ids=ids[:n.value].copy(), octave=oc[:n.value].copy())

    def keyframe_candidate(self, capacity: int = 8192) -> np.ndarray:
        """The resident keyframe candidate: the ids of the last end_frame after CleanMatches alone, outliers still held."""
        m = max(int(capacity), 1)
        ids = np.full(m, -1, np.int32)
        n = C.c_int32(0)
        self._call("dsh_track_keyframe_candidate", int(capacity), _ptr(ids, C.c_int32), C.byref(n))
        return ids[:n.value].copy()

    def motion_model_search(self, frame: TrackFrame, th: float = 20.0, th_wide: float = 25.0, min_matches: int = 20) -> MotionModelSearch:
        """DefTracking::TrackWithMotionModel after SetPose, with the resident last-frame list (of the preceding end_frame) as LastFrame;
        frame.state is not read."""
        keep = []
        f = frame.c(keep)
        N, NL = int(f.N), self._n_last
        fp, match = np.full(max(N, 1), -1, np.int32), np.full(max(NL, 1), -1, np.int32)
        nm, used = C.c_int32(0), C.c_float(0.0)
        self._call("dsh_motion_model_search", C.byref(f), float(th), float(th_wide), int(min_matches), _ptr(fp, C.c_int32), _ptr(match, C.c_int32),
                   C.byref(nm), C.byref(used))
        return MotionModelSearch(frame_points=fp[:N], match=match[:NL], nmatches=int(nm.value), th_used=float(used.value), ok=nm.value >= 15)

    # ---- the rigid pose-only optimisation (the else branch of TrackLocalMap) ----
    def pose_only_batch(self, frames, _single: bool = False) -> list:
        """ORB_SLAM2::Optimizer::poseOptimization for each PoseOnlyFrame of `frames` against the store's positions, in one launch."""
        B = len(frames)
        probs = (_lib.PoseOnlyProblemC * max(B, 1))()
        keep = []
        for p, f in zip(probs, frames):
            fp = _i32(f.frame_points)
            N = fp.shape[0]
            T = np.ascontiguousarray(f.Tcw, np.float32).reshape(16)
            kp = np.ascontiguousarray(f.kp, np.float32).reshape(N, 2)
            oc = _i32(f.octave).reshape(N)
            sg = np.ascontiguousarray(f.inv_level_sigma2, np.float32).reshape(-1)
            fl = np.zeros(max(N, 1), np.uint8)
            if f.outlier is not None:
                fl[:N] = np.asarray(f.outlier, bool).reshape(N)
            keep.append((T, kp, oc, sg, fp, fl))
            p.Tcw, p.kp, p.octave = _ptr(T, C.c_float), _ptr(kp, C.c_float), _ptr(oc, C.c_int32)
            p.K = (C.c_float * 4)(*[float(v) for v in np.asarray(f.K).reshape(4)])
            p.N, p.levels = N, int(sg.shape[0])
            p.inv_level_sigma2, p.frame_points, p.outlier = _ptr(sg, C.c_float), _ptr(fp, C.c_int32), _ptr(fl, C.c_uint8)
        if _single:
            self._call("dsh_track_pose_only", C.byref(probs[0]))
        else:
            self._call("dsh_track_pose_only_batch", B, probs)
        return [PoseOnly(outlier=k[5][:int(p.N)].astype(bool), Tcw=np.array(p.Tcw_out, np.float32).reshape(4, 4), pose=np.array(p.pose, float),
                         n_initial=int(p.n_initial), n_bad=int(p.n_bad), n_good=int(p.n_good), rounds=int(p.rounds),
                         iters=np.array(p.iters, np.int32), trials=np.array(p.trials, np.int32), bad=np.array(p.bad, np.int32),
                         chi2=np.array(p.chi2, float)) for p, k in zip(probs[:B], keep)]

    def pose_only(self, Tcw, K, kp, octave, inv_level_sigma2, frame_points, outlier=None) -> PoseOnly:
        """One frame: Tcw (4,4) float32, K = fx fy cx cy, kp (N,2) mvKeysUn, octave (N,), inv_level_sigma2 (levels,), frame_points (N,)
        ids or -1.  The positions are the store's; nothing of the store changes."""
        return self.pose_only_batch([PoseOnlyFrame(Tcw, K, kp, octave, inv_level_sigma2, frame_points, outlier)], _single=True)[0]

    # ---- Shape-from-Template of a tracked frame (the if branch of TrackLocalMap) ----
    def _sft_frame(self, kp, octave, inv_level_sigma2, frame_points, outlier, keep: list) -> _lib.TrackSftFrameC:
        fp = _i32(frame_points)
        N = fp.shape[0]
        kp = np.ascontiguousarray(kp, np.float32).reshape(N, 2)
        oc = _i32(octave).reshape(N)
        sg = np.ascontiguousarray(inv_level_sigma2, np.float32).reshape(-1)
        fl = np.zeros(max(N, 1), np.uint8)
        if outlier is not None:
            fl[:N] = np.asarray(outlier, bool).reshape(N)
        keep += [fp, kp, oc, sg, fl]
        f = _lib.TrackSftFrameC()
        f.N, f.levels = N, int(sg.shape[0])
        f.kp, f.octave, f.inv_level_sigma2 = _ptr(kp, C.c_float), _ptr(oc, C.c_int32), _ptr(sg, C.c_float)
        f.frame_points, f.outlier = _ptr(fp, C.c_int32), _ptr(fl, C.c_uint8)
        return f

    @staticmethod
    def _sft_table(N: int, keep: list) -> _lib.TrackSftTableC:
        m = max(int(N), 1)
        a = dict(kp_index=np.zeros(m, np.int32), point_id=np.zeros(m, np.int32), nodes=np.zeros((m, 3), np.int32), bary=np.zeros((m, 3)),
                 uv=np.zeros((m, 2)), invsig2=np.zeros(m))
        keep.append(a)
        return _lib.TrackSftTableC(int(N), 0, 0, _ptr(a["kp_index"], C.c_int32), _ptr(a["point_id"], C.c_int32), _ptr(a["nodes"], C.c_int32),
                                   _ptr(a["bary"], C.c_double), _ptr(a["uv"], C.c_double), _ptr(a["invsig2"], C.c_double))

    @staticmethod
    def _sft_rows(t: _lib.TrackSftTableC, a: dict) -> SftObservations:
        M = int(t.M)
        return SftObservations(**{k: v[:M].copy() for k, v in a.items()}, points_obs=int(t.points_obs))

    def sft_observations(self, kp, octave, inv_level_sigma2, frame_points, outlier=None) -> SftObservations:
        """The observation table DefPoseOptimization builds of a frame (DefOptimizer.cc:293-361), selected on the device from the facets
        and barycentrics the store holds: kp (N,2) mvKeysUn, octave (N,), inv_level_sigma2 (levels,), frame_points (N,) ids or -1,
        outlier (N,) mvbOutlier on entry (None: all False).  Nothing changes."""
        keep: list = []
        f = self._sft_frame(kp, octave, inv_level_sigma2, frame_points, outlier, keep)
        t = self._sft_table(f.N, keep)
        self._call("dsh_track_sft_observations", C.byref(f), C.byref(t))
        return self._sft_rows(t, keep[-1])

    def sft(self, Tcw, K, kp, octave, inv_level_sigma2, frame_points, node_xyz, outlier=None, write_back: bool = True, RegLap: float = 5000.0,
            RegInex: float = 5000.0, RegTemp: float = 0.0, NeighboursLayers: int = 1, max_iters: int = 50) -> TrackSft:
        """Optimizer::DefPoseOptimization of a frame against the store: the table of sft_observations, then dsh_sft_solve's path on it
        with Tcw (4,4) float32, K = fx fy cx cy and node_xyz (n,3) the current node positions.  write_back moves every point that is not
        bad and has a facet to its position on the optimised nodes (DefOptimizer.cc:568-576); close the frame with node_xyz=None then."""
        keep: list = []
        f = self._sft_frame(kp, octave, inv_level_sigma2, frame_points, outlier, keep)
        N = int(f.N)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        x = np.ascontiguousarray(node_xyz, np.float64).reshape(-1, 3)
        keep += [T, x]
        f.Tcw, f.xyz = _ptr(T, C.c_float), _ptr(x, C.c_double)
        f.K = (C.c_double * 4)(*[float(v) for v in np.asarray(K).reshape(4)])
        f.reg_lap, f.reg_inex, f.reg_temp = float(RegLap), float(RegInex), float(RegTemp)
        f.neighbour_layers, f.max_iters = int(NeighboursLayers), int(max_iters)
        t = self._sft_table(N, keep)
        m = max(N, 1)
        b = dict(Tcw=np.zeros((4, 4), np.float32), pose7=np.zeros(7), xyz=np.zeros((x.shape[0], 3)), chi2=np.zeros(m), outl=np.zeros(m, np.uint8),
                 mp=np.zeros((m, 3), np.float32))
        r = _lib.SftResultC()
        r.Tcw, r.pose7, r.xyz = _ptr(b["Tcw"], C.c_float), _ptr(b["pose7"], C.c_double), _ptr(b["xyz"], C.c_double)
        r.chi2_obs, r.outlier, r.mappoint_xyz = _ptr(b["chi2"], C.c_double), _ptr(b["outl"], C.c_uint8), _ptr(b["mp"], C.c_float)
        self._call("dsh_track_sft", C.byref(f), 1 if write_back else 0, C.byref(t), C.byref(r))
        rows = self._sft_rows(t, keep[-1])
        M = rows.kp_index.shape[0]
        return TrackSft(outlier=keep[4][:N].astype(bool), table=rows, Tcw=b["Tcw"], pose7=b["pose7"], xyz=b["xyz"], chi2_obs=b["chi2"][:M],
                        row_outlier=b["outl"][:M].astype(bool), mappoint_xyz=b["mp"][:M], rep_error=float(r.rep_error), inliers=int(r.inliers),
                        iters=int(r.iters), trials=int(r.trials), dim=int(r.dim), half_bandwidth=int(r.half_bandwidth), status=int(r.status))

    # ---- the template switch ----
    def get_points(self, ids=None) -> StoredPoints:
        """Position, normal, max distance, descriptor and bad flag of ids (None: every point of the store)."""
        ids = np.arange(self.n_points, dtype=np.int32) if ids is None else _i32(ids)
        n = ids.shape[0]
        m = max(n, 1)
        x, nr, md = np.zeros((m, 3), np.float32), np.zeros((m, 3), np.float32), np.zeros(m, np.float32)
        d, b = np.zeros((m, 32), np.uint8), np.zeros(m, np.uint8)
        self._call("dsh_point_store_get_points", n, _ptr(ids, C.c_int32), _ptr(x, C.c_float), _ptr(nr, C.c_float), _ptr(md, C.c_float), _ptr(d, C.c_uint8),
                   _ptr(b, C.c_uint8))
        return StoredPoints(xyz=x[:n], normal=nr[:n], max_distance=md[:n], desc=d[:n], bad=b[:n].astype(bool))

    def get_embedding(self, ids=None):
        """(nodes (n,3) int32, bary (n,3) float64) of ids (None: every point of the store); nodes -1 -1 -1: no facet."""
        ids = np.arange(self.n_points, dtype=np.int32) if ids is None else _i32(ids)
        n = ids.shape[0]
        m = max(n, 1)
        nd, b = np.full((m, 3), -1, np.int32), np.zeros((m, 3), np.float64)
        self._call("dsh_point_store_get_embedding", n, _ptr(ids, C.c_int32), _ptr(nd, C.c_int32), _ptr(b, C.c_double))
        return nd[:n], b[:n]

    def need_new_template(self, slot: int, kf: KeyFramePoints):
        """DefLocalMapping::needNewTemplate on keyframe `slot`: (newPoints, candidate (N,) bool); the caller compares the count with
        pointsToTemplate_."""
        keep = []
        k = kf.c(keep)
        cand = np.zeros(max(k.N, 1), np.uint8)
        n = C.c_int32(0)
        self._call("dsh_need_new_template", int(slot), C.byref(k), C.byref(n), _ptr(cand, C.c_uint8))
        return int(n.value), cand[:k.N].astype(bool)

    def switch_template(self, kf_store, slot: int, kf: KeyFramePoints, surface_pts, Twc) -> TemplateSwitch:
        """DefLocalMapping::updateTemplate for the reference keyframe `slot` (the same slot in kf_store, a mappoint.KeyFrameStore): the
        context's template must have been built just before (sft.surface_vertices, Context.template_build).  surface_pts (N,3) float32 is
        Surface::get3DSurfacePoint per key point, Twc (4,4) float32 the keyframe's GetPoseInverse()."""
        keep = []
        k = kf.c(keep)
        sp = None if surface_pts is None else np.ascontiguousarray(surface_pts, np.float32).reshape(-1, 3)   # None: the resident ones
        T = np.ascontiguousarray(Twc, np.float32).reshape(16)
        inp = _lib.TemplateSwitchInputC(kf_store._h if kf_store is not None else None, int(slot), C.pointer(k), _ptr(sp, C.c_float), _ptr(T, C.c_float))
        idx = np.zeros(max(k.N, 1), np.int32)
        cc = _lib.TemplateSwitchCountsC()
        self._call("dsh_template_switch", C.byref(inp), _ptr(idx, C.c_int32), C.byref(cc))
        return TemplateSwitch(new_idx=idx[:cc.n_new].copy(), **{n: int(getattr(cc, n)) for n, _ in _lib.TemplateSwitchCountsC._fields_})

    # ---- the mapping thread: anchors of a new keyframe ----
    def keyframe_anchors(self, slot: int, min_pairs: int = 20, max_matrix_bytes: int = 0) -> KeyframeAnchors:
        """What SchwarpDatabase::add reads of the map for the new keyframe `slot`.  Every live observation must carry its key point
        index (add_observations(..., idx=...)).  max_matrix_bytes bounds the device's anchors x N matrix (0: the library's default)."""
        N = self._kf_n[slot] if 0 <= int(slot) < len(self._kf_n) else 0
        ca, cp, cq = max(self.n_keyframes, 1), 4 * max(N, 1), 16 * max(N, 1)
        has = np.zeros(max(N, 1), np.uint8)
        while True:
            a = {n: np.zeros(ca, np.int32) for n in ("anchor_slot", "anchor_count", "anchor_pairs")}
            a.update({n: np.zeros(ca + 1, np.int32) for n in ("pair_ptr", "query_ptr")})
            a.update({n: np.zeros(max(cp, 1), np.int32) for n in ("pair_idx1", "pair_idx2", "pair_point")})
            a.update({n: np.zeros(max(cq, 1), np.int32) for n in ("query_idx1", "query_point")})
            own = np.zeros(max(cp, 1), np.uint8)
            r = _lib.AnchorListsC(anchor_capacity=ca, pair_capacity=cp, query_capacity=cq, max_matrix_bytes=int(max_matrix_bytes),
                                  pair_own=_ptr(own, C.c_uint8), has=_ptr(has, C.c_uint8), **{n: _ptr(v, C.c_int32) for n, v in a.items()})
            rc = self._ctx._L.dsh_keyframe_anchors(self._h, int(slot), int(min_pairs), C.byref(r))
            if rc == _lib.DSH_ERR_ARG and (r.n_anchors > ca or r.n_pairs > cp or r.n_queries > cq):   # a list did not fit: the needed sizes came back
                ca, cp, cq = max(ca, r.n_anchors), max(cp, r.n_pairs), max(cq, r.n_queries)
                continue
            self._ctx._check(rc, "dsh_keyframe_anchors")
            break
        A, npair, nq = r.n_anchors, r.n_pairs, r.n_queries
        return KeyframeAnchors(anchor_slot=a["anchor_slot"][:A], anchor_count=a["anchor_count"][:A], anchor_pairs=a["anchor_pairs"][:A],
                               pair_ptr=a["pair_ptr"][:A + 1], pair_idx1=a["pair_idx1"][:npair], pair_idx2=a["pair_idx2"][:npair],
                               pair_point=a["pair_point"][:npair], pair_own=own[:npair].astype(bool), query_ptr=a["query_ptr"][:A + 1],
                               query_idx1=a["query_idx1"][:nq], query_point=a["query_point"][:nq], has=has[:N].astype(bool),
                               n_no_ref=int(r.n_no_ref))

    # ---- the mapping thread: the map point upkeep of a new keyframe and of Repose ----
    def process_new_keyframe(self, kf_store, slot: int) -> NewKeyframe:
        """LocalMapping::ProcessNewKeyFrame's loop for keyframe `slot` (the same slot in kf_store, a mappoint.KeyFrameStore): every point
        of its table that does not observe it yet gets the observation, then UpdateNormalAndDepth and ComputeDistinctiveDescriptors over
        its observations by ascending slot, written into the store.  Every live observation must carry its key point index."""
        N = self._kf_n[slot] if 0 <= int(slot) < len(self._kf_n) else 0
        inp = _lib.KeyframeProcessInputC(kf_store._h if kf_store is not None else None, int(slot))
        act, added = np.zeros(max(N, 1), np.uint8), np.full(max(N, 1), -1, np.int32)
        cc = _lib.KeyframeProcessCountsC()
        self._call("dsh_keyframe_process_new", C.byref(inp), _ptr(act, C.c_uint8), _ptr(added, C.c_int32), C.byref(cc))
        return NewKeyframe(action=act[:N], added=added[:cc.n_added].copy(), **{n: int(getattr(cc, n)) for n, _ in _lib.KeyframeProcessCountsC._fields_})

    def upkeep(self, kf_store, ids=None, what: int = UPKEEP_BOTH, embedded: bool = False) -> Upkeep:
        """The map point upkeep on the store: the parts `what` names of the distinct points ids, or (embedded) of every point that is not
        bad and has a facet -- DefMapPoint::Repose's UpdateNormalAndDepth after switch_template with what=UPKEEP_NORMAL_DEPTH."""
        ids = np.zeros(0, np.int32) if ids is None else _i32(ids)
        n = 0 if embedded else ids.shape[0]
        inp = _lib.PointUpkeepInputC(kf_store._h if kf_store is not None else None, int(what),
                                     _lib.DSH_UPKEEP_EMBEDDED if embedded else _lib.DSH_UPKEEP_IDS, n, _ptr(ids, C.c_int32))
        st = np.zeros(max(n, 1), np.int32)
        cc = _lib.PointUpkeepCountsC()
        self._call("dsh_point_store_upkeep", C.byref(inp), _ptr(st, C.c_int32), C.byref(cc))
        return Upkeep(status=None if embedded else st[:n], **{f: int(getattr(cc, f)) for f, _ in _lib.PointUpkeepCountsC._fields_})

    # ---- the mapping thread: erasing observations and culling points ----
    def _erase_counts(self, cc) -> EraseCounts:
        return EraseCounts(**{f: int(getattr(cc, f)) for f, _ in _lib.PointEraseCountsC._fields_})

    def erase_observations_full(self, points, slots, erase_match: bool = False) -> ObservationErase:
        """MapPoint::EraseObservation of the pairs (distinct points): the record, nObs, the reference keyframe when it was the erased one,
        and setBadFlag when nObs falls to 2; erase_match adds KeyFrame::EraseMapPointMatch of the record's key point (the Schwarp fit's drop)."""
        p, k = _i32(points), _i32(slots)
        st = np.zeros(max(p.shape[0], 1), np.uint8)
        cc = _lib.PointEraseCountsC()
        self._call("dsh_point_store_erase_observations", p.shape[0], _ptr(p, C.c_int32), _ptr(k, C.c_int32), 1 if erase_match else 0,
                   _ptr(st, C.c_uint8), C.byref(cc))
        return ObservationErase(status=st[:p.shape[0]], counts=self._erase_counts(cc))

    def set_bad_full(self, ids) -> EraseCounts:
        """DefMapPoint::setBadFlag of the distinct points: the flag, their observation records and the table entries those name."""
        ids = _i32(ids)
        cc = _lib.PointEraseCountsC()
        self._call("dsh_point_store_set_bad", ids.shape[0], _ptr(ids, C.c_int32), C.byref(cc))
        return self._erase_counts(cc)

    def cull_full(self, ids, first_kf, current_kf: int) -> PointCull:
        """LocalMapping::MapPointCulling over ids: cull()'s decisions, with setBadFlag in full for the CULL_SET_BAD points."""
        ids, fk = _i32(ids), _i32(first_kf)
        act = np.zeros(max(ids.shape[0], 1), np.uint8)
        cc = _lib.PointEraseCountsC()
        self._call("dsh_point_store_cull", ids.shape[0], _ptr(ids, C.c_int32), _ptr(fk, C.c_int32), int(current_kf), _ptr(act, C.c_uint8), C.byref(cc))
        return PointCull(action=act[:ids.shape[0]], counts=self._erase_counts(cc))

    def observations(self, ids=None) -> PointObservations:
        """MapPoint::GetObservations of ids (None: every point of the store), by ascending slot."""
        ids = np.arange(self.n_points, dtype=np.int32) if ids is None else _i32(ids)
        n, cap = ids.shape[0], max(4 * ids.shape[0], 64)
        while True:
            ptr, sl, ix = np.zeros(n + 1, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
            total = C.c_int32(0)
            rc = self._ctx._L.dsh_point_store_get_observations(self._h, n, _ptr(ids, C.c_int32), _ptr(ptr, C.c_int32), cap, _ptr(sl, C.c_int32),
                                                               _ptr(ix, C.c_int32), C.byref(total))
            if rc == _lib.DSH_ERR_ARG and total.value > cap:   # the lists did not fit: the needed size came back
                cap = int(total.value)
                continue
            self._ctx._check(rc, "dsh_point_store_get_observations")
            return PointObservations(ptr=ptr, slots=sl[:total.value].copy(), idx=ix[:total.value].copy())

    # ---- the mapping thread: surface registration of a keyframe ----
    def _kf_len(self, slot: int) -> int:
        return self._kf_n[slot] if 0 <= int(slot) < len(self._kf_n) else 0

    def snapshot_positions(self, slot: int) -> int:
        """DefKeyFrame's constructor loop (DefKeyFrame.cc:60-74) for keyframe `slot`: the position of every point it holds that is not
        bad and has a facet is kept as PosesKeyframes; returns how many entries were taken.  Once per keyframe."""
        n = C.c_int32(0)
        self._call("dsh_keyframe_snapshot_positions", int(slot), C.byref(n))
        return int(n.value)

    def get_snapshot(self, slot: int):
        """(point (N,) int32, xyz (N,3) float32) of keyframe `slot`: per table entry the point whose position was taken, or -1."""
        N = self._kf_len(slot)
        pt, x = np.full(max(N, 1), -1, np.int32), np.zeros((max(N, 1), 3), np.float32)
        self._call("dsh_keyframe_get_snapshot", int(slot), N, _ptr(pt, C.c_int32), _ptr(x, C.c_float))
        return pt[:N], x[:N]

    def _register_input(self, kf_store, slot, surface_pts, Twc, u, chi_limit, check_chi, keep: list) -> _lib.KeyframeRegisterInputC:
        # surface_pts None: the keyframe's resident surface points (surface_init)
        sp = None if surface_pts is None else np.ascontiguousarray(surface_pts, np.float32).reshape(-1, 3)
        T = np.ascontiguousarray(Twc, np.float32).reshape(16)
        uu = None if u is None else np.ascontiguousarray(u, np.float64).reshape(-1)
        keep += [sp, T, uu]
        return _lib.KeyframeRegisterInputC(kf_store._h if kf_store is not None else None, int(slot), self._kf_len(slot) if sp is None else int(sp.shape[0]), _ptr(sp, C.c_float),
                                           _ptr(T, C.c_float), _ptr(uu, C.c_double), 0 if uu is None else uu.shape[0], float(chi_limit),
                                           int(bool(check_chi)))

    @staticmethod
    def _register_counts(r) -> dict:
        return {n: int(getattr(r, n)) for n in ("n_pairs", "n_empty", "n_bad", "n_no_facet", "n_no_snapshot")}

    def register_clouds(self, slot: int, surface_pts, Twc) -> KeyframeClouds:
        """The two clouds of SurfaceRegistration::registerSurfaces (:60-104) for keyframe `slot`: surface_pts (N,3) float32 is
        Surface::get3DSurfacePoint per key point, Twc (4,4) float32 the keyframe's GetPoseInverse().  Nothing changes."""
        keep: list = []
        inp = self._register_input(None, slot, surface_pts, Twc, None, 0.0, True, keep)
        m = max(int(inp.N), 1)
        idx, a, b = np.zeros(m, np.int32), np.zeros((m, 3), np.float32), np.zeros((m, 3), np.float32)
        r = _lib.KeyframeRegisterResultC()
        self._call("dsh_keyframe_register_clouds", C.byref(inp), _ptr(idx, C.c_int32), _ptr(a, C.c_float), _ptr(b, C.c_float), C.byref(r))
        n = int(r.n_pairs)
        return KeyframeClouds(pair_idx=idx[:n].copy(), cloud_surface=a[:n].copy(), cloud_map=b[:n].copy(), **self._register_counts(r))

    def register_surface(self, kf_store, slot: int, surface_pts, Twc, u, chi_limit: float, check_chi: bool = True) -> KeyframeRegistration:
        """SurfaceRegistration::registerSurfaces for keyframe `slot` from the stores: the clouds of register_clouds, the registration of
        register.registerSurfaces on them (u: the rand() stream), and when it registers Surface::applyScale of surface_pts and the new
        camera centre written into kf_store (a mappoint.KeyFrameStore, or None).  A refusal that still reports the counts (more than
        8000 pairs, a stream that is too short) raises DshError with them in its `result` attribute."""
        keep: list = []
        inp = self._register_input(kf_store, slot, surface_pts, Twc, u, chi_limit, check_chi, keep)
        N = int(inp.N)
        idx, sc = np.zeros(max(N, 1), np.int32), np.zeros((max(N, 1), 3), np.float32)
        r = _lib.KeyframeRegisterResultC()
        rc = self._ctx._L.dsh_keyframe_register(self._h, C.byref(inp), _ptr(idx, C.c_int32), _ptr(sc, C.c_float), C.byref(r))
        reg = bool(r.registered)
        info = np.array(r.info, float)
        res = KeyframeRegistration(pair_idx=idx[:int(r.n_pairs)].copy() if rc == _lib.DSH_OK else np.zeros(0, np.int32), registered=reg,
                                   stream_status=int(r.stream_status), consumed=int(r.consumed), sim3=np.array(r.sim3, float), s22=float(r.s22),
                                   info=info, Tcw_new=np.array(r.Tcw_new, np.float32).reshape(4, 4), Ow_new=np.array(r.Ow_new, np.float32),
                                   surface_scaled=sc[:N].copy() if reg else None, **self._register_counts(r))
        try:
            self._ctx._check(rc, "dsh_keyframe_register")
        except Exception as e:
            e.result = res
            raise
        return res

    def set_keyframe_pose(self, kf_store, slot: int, Tcw) -> np.ndarray:
        """KeyFrame::SetPose for keyframe `slot` of kf_store: its camera centre becomes that of Tcw (4,4) float32; returns the centre."""
        T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        inp = _lib.KeyframePoseInputC(kf_store._h if kf_store is not None else None, int(slot), _ptr(T, C.c_float))
        Ow = np.zeros(3, np.float32)
        self._call("dsh_keyframe_set_pose", C.byref(inp), _ptr(Ow, C.c_float))
        return Ow

    def keyframe_centre(self, kf_store, slot: int) -> np.ndarray:
        """The camera centre kf_store holds for keyframe `slot`."""
        inp = _lib.KeyframePoseInputC(kf_store._h if kf_store is not None else None, int(slot), None)
        Ow = np.zeros(3, np.float32)
        self._call("dsh_keyframe_get_centre", C.byref(inp), _ptr(Ow, C.c_float))
        return Ow

    # ---- the mapping thread: the resident Surface of a keyframe ----
    def surface_init(self, slot: int, kpn):
        """Surface(N) of DefKeyFrame's constructor for keyframe `slot`, with mpKeypointNorm kpn (N,2) float32.  Once per keyframe."""
        k = np.ascontiguousarray(kpn, np.float32).reshape(-1, 2)
        self._call("dsh_keyframe_surface_init", int(slot), int(k.shape[0]), _ptr(k, C.c_float))

    def surface_set_depth(self, slot: int, bbs, ctrl):
        """Surface::saveArray: the depth spline of keyframe `slot` (bbs: nrsfm.Bbs, ctrl (nptsu * nptsv,) float64)."""
        b = bbs.c()
        x = np.ascontiguousarray(ctrl, np.float64).reshape(-1)
        if x.shape[0] != bbs.nptsu * bbs.nptsv:
            raise ValueError("ctrl does not have nptsu * nptsv entries")
        self._call("dsh_keyframe_surface_set_depth", int(slot), C.byref(b), _ptr(x, C.c_double))

    def surface_set_points(self, slot: int, idx, pts):
        """Surface::set3DSurfacePoint from the host: pts (n,3) float32 for the distinct key points idx of keyframe `slot`."""
        i, x = _i32(idx), np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
        if i.shape[0] != x.shape[0]:
            raise ValueError("idx and pts differ in length")
        self._call("dsh_keyframe_surface_set_points", int(slot), i.shape[0], _ptr(i, C.c_int32), _ptr(x, C.c_float))

    def surface_set_normals(self, slots, idx, normals) -> np.ndarray:
        """Surface::setNormalSurfacePoint in call order for the targets (slots[j], idx[j]) with normals (n,3) float32; returns each target
        keyframe's n_normals after the call."""
        s, i, x = _i32(slots), _i32(idx), np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if not s.shape[0] == i.shape[0] == x.shape[0]:
            raise ValueError("slots, idx and normals differ in length")
        nn = np.zeros(max(s.shape[0], 1), np.int32)
        self._call("dsh_keyframe_surface_set_normals", s.shape[0], _ptr(s, C.c_int32), _ptr(i, C.c_int32), _ptr(x, C.c_float), _ptr(nn, C.c_int32))
        return nn[:s.shape[0]]

    def surface_take_normals(self, diff_db, sel, slots, idx) -> np.ndarray:
        """The same with normal j picked on the device from the last normal solve of diff_db (nrsfm.DiffDatabase): sel >= 0 is normal_ref
        of that point, sel < 0 record -1 - sel."""
        q, s, i = _i32(sel), _i32(slots), _i32(idx)
        if not q.shape[0] == s.shape[0] == i.shape[0]:
            raise ValueError("sel, slots and idx differ in length")
        nn = np.zeros(max(s.shape[0], 1), np.int32)
        inp = _lib.SurfaceTakeInputC(diff_db._h if diff_db is not None else None, s.shape[0], _ptr(q, C.c_int32), _ptr(s, C.c_int32), _ptr(i, C.c_int32))
        self._call("dsh_keyframe_surface_take_normals", C.byref(inp), _ptr(nn, C.c_int32))
        return nn[:s.shape[0]]

    def surface_gather(self, slots, idx) -> SurfaceGather:
        """x0 / has_x0 / ref_uv of a normal solve for the targets (slots[j], idx[j])."""
        s, i = _i32(slots), _i32(idx)
        if s.shape[0] != i.shape[0]:
            raise ValueError("slots and idx differ in length")
        n = s.shape[0]
        m = max(n, 1)
        nxy, has, uv = np.zeros((m, 2), np.float32), np.zeros(m, np.uint8), np.zeros((m, 2), np.float32)
        self._call("dsh_keyframe_surface_gather", n, _ptr(s, C.c_int32), _ptr(i, C.c_int32), _ptr(nxy, C.c_float), _ptr(has, C.c_uint8), _ptr(uv, C.c_float))
        return SurfaceGather(normal_xy=nxy[:n], has=has[:n], uv=uv[:n])

    def surface_get(self, slot: int) -> KeyframeSurface:
        """The resident Surface of keyframe `slot`, read back."""
        from .nrsfm import Bbs
        N = self._kf_len(slot)
        m = max(N, 1)
        nr, has, pts, kpn = np.zeros((m, 3), np.float32), np.zeros(m, np.uint8), np.zeros((m, 3), np.float32), np.zeros((m, 2), np.float32)
        ctrl = np.zeros(512, np.float64)
        info = _lib.KeyframeSurfaceInfoC()
        self._call("dsh_keyframe_surface_get", int(slot), N, _ptr(nr, C.c_float), _ptr(has, C.c_uint8), _ptr(pts, C.c_float), _ptr(kpn, C.c_float),
                   _ptr(ctrl, C.c_double), C.byref(info))
        g = info.grid
        bbs = Bbs(g.umin, g.umax, g.nptsu, g.vmin, g.vmax, g.nptsv, g.valdim) if info.has_depth else None
        return KeyframeSurface(normals=nr[:N], has_normal=has[:N].astype(bool), pts=pts[:N], kpn=kpn[:N],
                               ctrl=ctrl[:g.nptsu * g.nptsv].copy() if info.has_depth else None, bbs=bbs, n_normals=int(info.n_normals),
                               enough_normals=bool(info.enough_normals))

    def sfn(self, slot: int, bbs, bending_weight: float, mean_depth: float) -> KeyframeSfn:
        """ShapeFromNormals::estimate of keyframe `slot` from the store: obtainM's selection on the device, the stages of
        nrsfm.ShapeFromNormals on its sites; when ok the surface points and the depth spline of the keyframe are the new ones."""
        b = bbs.c()
        N, Nc = self._kf_len(slot), bbs.nptsu * bbs.nptsv
        raw, ctrl, pts = np.zeros(Nc, np.float64), np.zeros(Nc, np.float64), np.zeros((max(N, 1), 3), np.float32)
        inp = _lib.KeyframeSfnInputC(self._ctx._h, int(slot), C.pointer(b), float(bending_weight), float(mean_depth))
        r = _lib.KeyframeSfnResultC()
        self._call("dsh_keyframe_sfn", C.byref(inp), _ptr(raw, C.c_double), _ptr(ctrl, C.c_double), _ptr(pts, C.c_float), C.byref(r))
        ok = bool(r.ok)
        return KeyframeSfn(ok=ok, ctrl_raw=raw, ctrl=ctrl if ok else None, pts=pts[:N] if ok else None,
                           **{n: int(getattr(r, n)) for n in ("n_sites", "n_empty", "n_bad", "n_no_normal", "n_nan")})

    def surface_state(self, slot: int) -> int:
        """0: keyframe `slot` has no resident Surface, 1: a Surface, 2: a Surface with a depth spline; -1: no such keyframe."""
        return int(self._ctx._L.dsh_keyframe_surface_state(self._h, int(slot)))

    def surface_vertices(self, slot: int, Twc, xs: int, ys: int) -> np.ndarray:
        """Surface::getVertex of keyframe `slot` with its resident depth spline: (xs * ys, 3) float64 in world coordinates."""
        T = np.ascontiguousarray(Twc, np.float32).reshape(16)
        out = np.zeros((max(int(xs) * int(ys), 1), 3), np.float64)
        self._call("dsh_keyframe_surface_vertices", int(slot), _ptr(T, C.c_float), int(xs), int(ys), _ptr(out, C.c_double))
        return out[:int(xs) * int(ys)]

    def keyframe_table(self, slot: int) -> np.ndarray:
        """KeyFrame::GetMapPointMatches of keyframe `slot` as ids or -1."""
        N = self._kf_n[slot] if 0 <= int(slot) < len(self._kf_n) else 0
        t = np.full(max(N, 1), -1, np.int32)
        self._call("dsh_point_store_get_keyframe_table", int(slot), N, _ptr(t, C.c_int32))
        return t[:N]

    # ---- a new keyframe: creation and covisibility connections ----
    def create_keyframe(self, kf_store, kf, Tcw, points=None, kpn=None) -> KeyframeCreation:
        """DefTracking::CreateNewKeyFrame on both stores in one call: kf (a mappoint.MpKeyFrame; Ow and bad are not read) goes into
        kf_store with the camera centre of Tcw (4,4) float32, the table `points` (ids or -1; None: the resident keyframe candidate of
        the last end_frame) into this store, the PosesKeyframes snapshot is taken, and with kpn (N,2) float32 the Surface is
        initialised.  The state afterwards is that of kf_store.add, add_keyframe, snapshot_positions and surface_init."""
        desc = np.ascontiguousarray(kf.desc, np.uint8).reshape(-1, 32)
        octave = _i32(kf.octave)
        sf = np.ascontiguousarray(kf.scale_factors, np.float32).reshape(-1)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        N = int(desc.shape[0])
        t = None if points is None else _i32(points)
        k = None if kpn is None else np.ascontiguousarray(kpn, np.float32).reshape(-1, 2)
        if octave.shape[0] != N or (t is not None and t.shape[0] != N) or (k is not None and k.shape[0] != N):
            raise ValueError("desc, octave, points and kpn differ in length")
        if N == 0:   # an empty array has no address: give the call one it does not read
            t = None if t is None else np.full(1, -1, np.int32)
            k = None if k is None else np.zeros((1, 2), np.float32)
        c = _lib.MpKeyFrameC()
        c.N = N
        c.desc, c.octave = _ptr(desc, C.c_uint8), _ptr(octave, C.c_int32)
        c.levels, c.scale_factors = int(sf.shape[0]), _ptr(sf, C.c_float)
        inp = _lib.KeyframeCreateInputC(kf_store._h if kf_store is not None else None, C.pointer(c), _ptr(T, C.c_float), _ptr(t, C.c_int32),
                                        _ptr(k, C.c_float))
        r = _lib.KeyframeCreateResultC()
        self._call("dsh_keyframe_create", C.byref(inp), C.byref(r))
        self._kf_n.append(N)
        return KeyframeCreation(slot=int(r.slot), n_held=int(r.n_held), n_snapshot=int(r.n_snapshot), Ow=np.array(r.Ow, np.float32))

    def update_connections(self, slot: int, th: int = 100) -> KeyframeConnections:
        """KeyFrame::UpdateConnections of keyframe `slot` from the observation log; on the first call that finds a connection the
        keyframe's parent in the store becomes the first ordered keyframe (not for slot 0)."""
        K = max(self.n_keyframes, 1)
        ck, cw, ok, ow = (np.zeros(K, np.int32) for _ in range(4))
        r = _lib.KeyframeConnectionsC()
        self._call("dsh_keyframe_update_connections", int(slot), int(th), K, _ptr(ck, C.c_int32), _ptr(cw, C.c_int32), _ptr(ok, C.c_int32),
                   _ptr(ow, C.c_int32), C.byref(r))
        nc, no = int(r.n_counted), int(r.n_connected)
        return KeyframeConnections(counted_kf=ck[:nc].copy(), counted_w=cw[:nc].copy(), ordered_kf=ok[:no].copy(), ordered_w=ow[:no].copy(),
                                   parent=int(r.parent), parent_set=bool(r.parent_set), max_weight=int(r.max_weight), max_kf=int(r.max_kf))

    # ---- the mapping thread: one anchor of SchwarpDatabase::add ----
    def set_view(self, slot: int, view: KeyframeView):
        """The pixel key points, camera, image bounds, image grid and warp grid of keyframe `slot`.  Once per keyframe, after surface_init."""
        px = np.ascontiguousarray(view.kp_px, np.float32).reshape(-1, 2)
        v = _lib.KeyframeViewC(int(px.shape[0]), _ptr(px if px.shape[0] else np.zeros((1, 2), np.float32), C.c_float), *[float(a) for a in view.K],
                               *[float(a) for a in view.bounds], int(view.grid_cols), int(view.grid_rows), view.warp_grid.c())
        self._call("dsh_keyframe_set_view", int(slot), C.byref(v))

    def get_view(self, slot: int) -> KeyframeView:
        from .nrsfm import Bbs
        N = self._kf_len(slot)
        px = np.zeros((max(N, 1), 2), np.float32)
        v = _lib.KeyframeViewC()
        self._call("dsh_keyframe_get_view", int(slot), C.byref(v), _ptr(px, C.c_float))
        g = v.warp_grid
        return KeyframeView(kp_px=px[:N], K=(v.fx, v.fy, v.cx, v.cy), bounds=(v.mnMinX, v.mnMaxX, v.mnMinY, v.mnMaxY), grid_cols=int(v.grid_cols),
                            grid_rows=int(v.grid_rows), warp_grid=Bbs(g.umin, g.umax, g.nptsu, g.vmin, g.vmax, g.nptsv, g.valdim))

    def warp_pair(self, kf_store, diff_db, slot: int, anchor: int, pair_idx1, pair_idx2, query_idx1, lam: float, tag: Optional[int] = None,
                  min_pairs: int = 20, max_iters: int = 3, radius: float = 2.0, th_low: int = 50) -> WarpPair:
        """DefORBmatcher::findbyWarp and SchwarpDatabase::calculateSchwarps for new keyframe `slot` and anchor keyframe `anchor`, every
        key point array read from the stores: pair_idx1 / pair_idx2 are the matched key points (anchor, slot) as anchors() lists them,
        query_idx1 the anchor's key points to search for, ascending.  The DiffProp records go into diff_db (nrsfm.DiffDatabase) under
        the point ids of the store with `tag` (default: slot).  x has the 2 NCu NCv entries of the anchor's warp grid."""
        i1, i2, q1 = _i32(pair_idx1), _i32(pair_idx2), _i32(query_idx1)
        if i1.shape[0] != i2.shape[0]:
            raise ValueError("pair_idx1 and pair_idx2 differ in length")
        P, Q = int(i1.shape[0]), int(q1.shape[0])
        m = max(Q, 1)
        x = np.zeros(512, np.float64)                             # room for the 256 control points the call accepts
        ps, qs, qa = np.zeros(max(P, 1), np.uint8), np.zeros(m, np.uint8), np.zeros(m, np.uint8)
        qm, qp = np.full(m, -1, np.int32), np.full(m, -1, np.int32)
        inp = _lib.WarpPairInputC(self._ctx._h, kf_store._h if kf_store is not None else None, diff_db._h if diff_db is not None else None, int(slot),
                                  int(anchor), int(slot if tag is None else tag), float(lam), int(min_pairs), int(max_iters), float(radius), int(th_low),
                                  P, _ptr(i1 if P else np.zeros(1, np.int32), C.c_int32), _ptr(i2 if P else np.zeros(1, np.int32), C.c_int32), Q,
                                  _ptr(q1 if Q else np.zeros(1, np.int32), C.c_int32))
        r = _lib.WarpPairResultC(_ptr(x, C.c_double), _ptr(ps, C.c_uint8), _ptr(qs, C.c_uint8), _ptr(qm, C.c_int32), _ptr(qp, C.c_int32), _ptr(qa, C.c_uint8))
        self._call("dsh_keyframe_warp_pair", C.byref(inp), C.byref(r))
        v = _lib.KeyframeViewC()
        self._call("dsh_keyframe_get_view", int(anchor), C.byref(v), None)   # the anchor's grid, from the host mirror
        x = x[:2 * v.warp_grid.nptsu * v.warp_grid.nptsv].copy()
        return WarpPair(x=x, init_ok=bool(r.init_ok), fitted=bool(r.fitted), info=np.array(r.info, np.int32), costs=np.array(r.costs, np.float64),
                        pair_state=ps[:P], query_state=qs[:Q], query_match=qm[:Q], query_point=qp[:Q], query_added=qa[:Q].astype(bool),
                        first_record=int(r.first_record),
                        counts={n: int(getattr(r, n)) for n in ("n_filtered", "n_matched", "n_appended", "n_list", "n_skipped", "n_dropped", "n_kept", "n_stored", "rounds")},
                        erase={n: int(getattr(r.erase, n)) for n in ("n_found", "n_ref_moved", "n_set_bad", "n_records", "n_entries")})
