"""Host-side mirror of the tracking searches (include/defslam_hip.h: dsh_search_by_projection_*) and the two steps of DefSLAM's
per-frame tracking that produce the SfT problem's observations:

  * DefTracking::TrackWithMotionModel (Modules/Tracking/DefTracking.cc:342-375): frame-to-frame search with th = 20, again with
    th = 25 when fewer than 20 points matched, failure below 15 matches.
  * DefTracking::TrackLocalMap -> Tracking::SearchLocalPoints (DefTracking.cc:234-250, Tracking.cc:1405-1470): local-map search
    with th = 3 on the state the first search left.

Both run on the device (track_kernels.hip); there is no CPU fallback.  Key point state: 0 no map point, 1 a map point with
observations, 2 a map point without observations.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from .sft import Context, _ptr

FRAME_GRID_COLS = 64
FRAME_GRID_ROWS = 48
TH_HIGH = 75          # ORBmatcher.cc:35 (ORB-SLAM2 has 100)


def orb_pyramid(levels: int = 8, scale_factor: float = 1.2):
    """ORBextractor's mvScaleFactor (float32 products, ORBextractor.cc) and Frame::mfLogScaleFactor = log(float scale factor)."""
    sf = np.ones(levels, np.float32)
    f = np.float32(scale_factor)
    for i in range(1, levels):
        sf[i] = np.float32(sf[i - 1] * f)
    return sf, np.float32(np.log(np.float64(f)))


def camera_center(Tcw: np.ndarray) -> np.ndarray:
    """Frame::mOw = -Rcw^T tcw (Frame::UpdatePoseMatrices) from the float32 pose: accumulated in double, rounded to float32."""
    T = np.asarray(Tcw, np.float32).astype(np.float64)
    R, t = T[:3, :3], T[:3, 3]
    return np.array([-(R[0, k] * t[0] + R[1, k] * t[1] + R[2, k] * t[2]) for k in range(3)], np.float64).astype(np.float32)


@dataclass
class TrackFrame:
    """The members of ORB_SLAM2::Frame the searches read."""
    Tcw: np.ndarray                     # (4,4) float32 mTcw
    K: np.ndarray                       # (4,) float32 fx, fy, cx, cy
    bounds: np.ndarray                  # (4,) float32 mnMinX, mnMaxX, mnMinY, mnMaxY
    kp: np.ndarray                      # (N,2) float32 mvKeysUn
    octave: np.ndarray                  # (N,) int32
    desc: np.ndarray                    # (N,32) uint8
    scale_factors: np.ndarray           # (levels,) float32
    log_scale_factor: float
    state: Optional[np.ndarray] = None  # (N,) uint8, zeros when None
    Ow: Optional[np.ndarray] = None     # (3,) float32 mOw, camera_center(Tcw) when None
    grid: tuple = (FRAME_GRID_COLS, FRAME_GRID_ROWS)

    def arrays(self):
        N = int(np.asarray(self.kp).reshape(-1, 2).shape[0])
        st = np.zeros(N, np.uint8) if self.state is None else self.state
        Ow = camera_center(self.Tcw) if self.Ow is None else self.Ow
        return dict(Tcw=np.ascontiguousarray(self.Tcw, np.float32).reshape(4, 4), kp=np.ascontiguousarray(self.kp, np.float32).reshape(-1, 2),
                    octave=np.ascontiguousarray(self.octave, np.int32), desc=np.ascontiguousarray(self.desc, np.uint8).reshape(-1, 32),
                    state=np.ascontiguousarray(st, np.uint8), sf=np.ascontiguousarray(self.scale_factors, np.float32),
                    Ow=np.asarray(Ow, np.float32), K=np.asarray(self.K, np.float32), bounds=np.asarray(self.bounds, np.float32))

    def c(self, keep: list) -> _lib.TrackFrameC:
        a = self.arrays()
        keep.append(a)
        f = _lib.TrackFrameC()
        f.Tcw = _ptr(a["Tcw"], C.c_float)
        f.Ow[:] = [float(x) for x in a["Ow"]]
        f.K[:] = [float(x) for x in a["K"]]
        f.bounds[:] = [float(x) for x in a["bounds"]]
        f.grid_cols, f.grid_rows = int(self.grid[0]), int(self.grid[1])
        f.levels = int(a["sf"].shape[0])
        f.scale_factors = _ptr(a["sf"], C.c_float)
        f.log_scale_factor = float(self.log_scale_factor)
        f.N = int(a["kp"].shape[0])
        f.kp = _ptr(a["kp"], C.c_float)
        f.octave = _ptr(a["octave"], C.c_int32)
        f.desc = _ptr(a["desc"], C.c_uint8)
        f.state = _ptr(a["state"], C.c_uint8)
        return f


@dataclass
class FrameQueries:
    """Frame to frame: the last frame's map points that are present and not outliers, in last-frame index order."""
    xyz: np.ndarray                     # (Q,3) float32 world positions
    octave: np.ndarray                  # (Q,) LastFrame.mvKeys[i].octave
    desc: np.ndarray                    # (Q,32) uint8


@dataclass
class LocalQueries:
    """Local map: mvpLocalMapPoints in its order."""
    xyz: np.ndarray                     # (Q,3) float32
    normal: np.ndarray                  # (Q,3) float32 GetNormal()
    max_distance: np.ndarray            # (Q,) float32 mfMaxDistance
    desc: np.ndarray                    # (Q,32) uint8
    skip: Optional[np.ndarray] = None   # (Q,) already matched in this frame or bad


@dataclass
class SearchResult:
    match: np.ndarray                   # (Q,) int32 key point index or -1
    nmatches: int
    rescans: int
    in_view: np.ndarray = field(default=None)
    level: np.ndarray = field(default=None)
    uv: np.ndarray = field(default=None)
    view_cos: np.ndarray = field(default=None)


def search_batch(ctx: Context, items: Sequence[tuple]) -> List[SearchResult]:
    """items: (TrackFrame, FrameQueries or LocalQueries, th) per search; one upload, three launches, one download."""
    B = len(items)
    probs = (_lib.TrackProblemC * max(B, 1))()
    keep, outs = [], []
    for i, (fr, qs, th) in enumerate(items):
        p = probs[i]
        p.frame = fr.c(keep)
        p.th = float(th)
        xyz = np.ascontiguousarray(qs.xyz, np.float32).reshape(-1, 3)
        Q = xyz.shape[0]
        desc = np.ascontiguousarray(qs.desc, np.uint8).reshape(-1, 32)
        o = dict(match=np.full(Q, -1, np.int32))
        keep.append((xyz, desc))
        p.Q, p.xyz, p.desc, p.match = Q, _ptr(xyz, C.c_float), _ptr(desc, C.c_uint8), _ptr(o["match"], C.c_int32)
        if isinstance(qs, LocalQueries):
            nrm = np.ascontiguousarray(qs.normal, np.float32).reshape(-1, 3)
            md = np.ascontiguousarray(qs.max_distance, np.float32)
            skip = None if qs.skip is None else np.ascontiguousarray(qs.skip, np.uint8)
            keep.append((nrm, md, skip))
            o.update(in_view=np.zeros(Q, np.uint8), level=np.zeros(Q, np.int32), uv=np.zeros((Q, 2), np.float32), view_cos=np.zeros(Q, np.float32))
            p.mode = _lib.DSH_TRACK_LOCAL
            p.normal, p.max_distance, p.skip = _ptr(nrm, C.c_float), _ptr(md, C.c_float), _ptr(skip, C.c_uint8)
            p.in_view, p.level = _ptr(o["in_view"], C.c_uint8), _ptr(o["level"], C.c_int32)
            p.uv, p.view_cos = _ptr(o["uv"], C.c_float), _ptr(o["view_cos"], C.c_float)
        else:
            oc = np.ascontiguousarray(qs.octave, np.int32)
            keep.append(oc)
            p.mode = _lib.DSH_TRACK_FRAME
            p.octave = _ptr(oc, C.c_int32)
        outs.append(o)
    ctx._check(ctx._L.dsh_search_by_projection_batch(ctx._h, B, probs), "dsh_search_by_projection_batch")
    res = []
    for i, o in enumerate(outs):
        r = SearchResult(match=o["match"], nmatches=int(probs[i].nmatches), rescans=int(probs[i].rescans))
        r.in_view = o["in_view"].astype(bool) if "in_view" in o else None
        r.level, r.uv, r.view_cos = o.get("level"), o.get("uv"), o.get("view_cos")
        res.append(r)
    return res


def SearchByProjectionFrame(ctx: Context, frame: TrackFrame, qs: FrameQueries, th: float) -> SearchResult:
    """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, true) (ORBmatcher.cc:1360-1510)."""
    return search_batch(ctx, [(frame, qs, th)])[0]


def SearchByProjectionLocal(ctx: Context, frame: TrackFrame, qs: LocalQueries, th: float = 3.0) -> SearchResult:
    """isInFrustum(pMP, 0.5) + ORBmatcher(0.8).SearchByProjection(F, vpMapPoints, th) (Tracking.cc:1440-1468, ORBmatcher.cc:42-136)."""
    return search_batch(ctx, [(frame, qs, th)])[0]


def assigned_state(state: np.ndarray, match: np.ndarray) -> np.ndarray:
    """Key point state after a search: every assigned key point holds a map point with observations (state 1)."""
    st = np.array(state, np.uint8, copy=True)
    m = np.asarray(match)
    st[m[m >= 0]] = 1
    return st


@dataclass
class MotionModelResult:
    match: np.ndarray                   # (Q,) key point of each last-frame map point, -1
    nmatches: int
    ok: bool                            # TrackWithMotionModel's return value (nmatches >= 15)
    th: float                           # the window factor of the search that produced match (20 or 25)
    state: np.ndarray                   # (N,) the frame's key point state afterwards
    rescans: int = 0


def motion_model_search(ctx: Context, frame: TrackFrame, qs: FrameQueries) -> MotionModelResult:
    """DefTracking::TrackWithMotionModel (DefTracking.cc:342-375) from the pose the caller set (mCurrentFrame->SetPose(mLastFrame.mTcw)):
    the frame's map points are cleared (:353), searched with th = 20, cleared and searched again with th = 25 when fewer than 20
    matched; fewer than 15 matches is a failure."""
    N = np.asarray(frame.kp).reshape(-1, 2).shape[0]
    f = TrackFrame(**{**frame.__dict__, "state": np.zeros(N, np.uint8)})
    th = 20.0
    r = SearchByProjectionFrame(ctx, f, qs, th)
    rescans = r.rescans
    if r.nmatches < 20:
        th = 25.0
        r = SearchByProjectionFrame(ctx, f, qs, th)
        rescans += r.rescans
    return MotionModelResult(match=r.match, nmatches=r.nmatches, ok=r.nmatches >= 15, th=th, state=assigned_state(f.state, r.match), rescans=rescans)


def local_points_search(ctx: Context, frame: TrackFrame, state: np.ndarray, qs: LocalQueries, th: float = 3.0):
    """Tracking::SearchLocalPoints (Tracking.cc:1405-1470) on the state the motion-model search left: returns (SearchResult, new state).
    qs.skip marks the local points already matched in this frame or bad (the caller's bookkeeping of :1408-1451)."""
    f = TrackFrame(**{**frame.__dict__, "state": np.asarray(state, np.uint8)})
    r = SearchByProjectionLocal(ctx, f, qs, th)
    return r, assigned_state(state, r.match)
