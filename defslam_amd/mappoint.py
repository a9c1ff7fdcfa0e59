"""Host-side mirror of the map point upkeep (include/defslam_hip.h: dsh_kfdb_*, dsh_mappoint_update):

  * MapPoint::ComputeDistinctiveDescriptors (Thirdparty/ORBSLAM_2/src/MapPoint.cc:257-325): the observed descriptor with the least
    median Hamming distance to the others, over the observations whose keyframe is not bad;
  * MapPoint::UpdateNormalAndDepth (MapPoint.cc:348-391): the mean viewing direction over all observations and the scale-invariance
    distance range from the reference keyframe;
  * LocalMapping::ProcessNewKeyFrame's loop (LocalMapping.cc:142-161) that calls both for the map points of a new keyframe.

The keyframes' descriptor rows stay in HBM (KeyFrameStore); the work runs on the device (mappoint_kernels.hip), there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .sft import Context, _ptr

DESCRIPTOR = _lib.DSH_MP_DESCRIPTOR
NORMAL_DEPTH = _lib.DSH_MP_NORMAL_DEPTH
BOTH = DESCRIPTOR | NORMAL_DEPTH
NO_OBS = _lib.DSH_MP_NO_OBS
NO_GOOD_DESC = _lib.DSH_MP_NO_GOOD_DESC


@dataclass
class MpKeyFrame:
    """The members of ORB_SLAM2::KeyFrame the upkeep reads (fixed once the keyframe is inserted)."""
    Ow: np.ndarray                      # (3,) float32 GetCameraCenter()
    desc: np.ndarray                    # (N,32) uint8 mDescriptors
    octave: np.ndarray                  # (N,) int32 mvKeysUn[j].octave
    scale_factors: np.ndarray           # (levels,) float32 mvScaleFactors
    bad: bool = False                   # isBad()


class KeyFrameStore:
    """dsh_kfdb: every keyframe's descriptor rows, octaves, camera centre and pyramid, copied to HBM once when it is added."""

    def __init__(self, ctx: Context, capacity: int = 64):
        self._ctx, self._h = ctx, None
        h = C.c_void_p()
        ctx._check(ctx._L.dsh_kfdb_create(ctx._h, int(capacity), C.byref(h)), "dsh_kfdb_create")
        self._h = h

    def close(self):
        if self._h is not None:
            self._ctx._L.dsh_kfdb_destroy(self._h)
            self._h = None

    __del__ = close

    def add(self, kf: MpKeyFrame) -> int:
        desc = np.ascontiguousarray(kf.desc, np.uint8).reshape(-1, 32)
        octave = np.ascontiguousarray(kf.octave, np.int32).reshape(-1)
        sf = np.ascontiguousarray(kf.scale_factors, np.float32).reshape(-1)
        c = _lib.MpKeyFrameC()
        c.Ow[:] = [float(x) for x in np.asarray(kf.Ow, np.float32).reshape(3)]
        c.N = int(desc.shape[0])
        c.desc, c.octave = _ptr(desc, C.c_uint8), _ptr(octave, C.c_int32)
        c.levels, c.scale_factors = int(sf.shape[0]), _ptr(sf, C.c_float)
        c.bad = 1 if kf.bad else 0
        slot = C.c_int32(-1)
        self._ctx._check(self._ctx._L.dsh_kfdb_add(self._h, C.byref(c), C.byref(slot)), "dsh_kfdb_add")
        return int(slot.value)

    def set_bad(self, slot: int, bad: bool = True):
        self._ctx._check(self._ctx._L.dsh_kfdb_set_bad(self._h, int(slot), 1 if bad else 0), "dsh_kfdb_set_bad")

    def clear(self):
        self._ctx._check(self._ctx._L.dsh_kfdb_clear(self._h), "dsh_kfdb_clear")

    def __len__(self):
        return int(self._ctx._L.dsh_kfdb_count(self._h))


def obs_csr(obs: Sequence[Sequence[Tuple[int, int]]]):
    """Per point a list of (store slot, key point index) in the reference's iteration order -> (obs_ptr, obs_kf, obs_idx)."""
    ptr = np.zeros(len(obs) + 1, np.int32)
    ptr[1:] = np.cumsum([len(o) for o in obs])
    flat = [x for o in obs for x in o]
    kf = np.array([s for s, _ in flat], np.int32)
    idx = np.array([j for _, j in flat], np.int32)
    return ptr, kf, idx


@dataclass
class UpdateResult:
    desc: np.ndarray                    # (P,32) uint8: the input where no descriptor was elected
    best: np.ndarray                    # (P,) int32 observation index of the elected descriptor, -1
    normal: np.ndarray                  # (P,3) float32 mNormalVector: the input where not written
    max_distance: np.ndarray            # (P,) float32 mfMaxDistance
    min_distance: np.ndarray            # (P,) float32 mfMinDistance
    status: np.ndarray                  # (P,) int32 NO_OBS | NO_GOOD_DESC


def update(ctx: Context, store: KeyFrameStore, xyz, obs, ref_kf, what: int = BOTH, desc=None, normal=None, max_distance=None,
           min_distance=None) -> UpdateResult:
    """dsh_mappoint_update.  obs: a list of (slot, index) lists or a CSR triple (obs_ptr, obs_kf, obs_idx).  desc / normal / distances are
    the points' current values (zeros when None): what the call does not write comes back unchanged."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    P = xyz.shape[0]
    ptr, kf, idx = obs if isinstance(obs, tuple) else obs_csr(obs)
    ptr, kf, idx = (np.ascontiguousarray(a, np.int32) for a in (ptr, kf, idx))
    ref = np.ascontiguousarray(ref_kf, np.int32).reshape(-1)
    r = UpdateResult(desc=np.zeros((P, 32), np.uint8) if desc is None else np.array(desc, np.uint8).reshape(P, 32),
                     best=np.full(P, -1, np.int32),
                     normal=np.zeros((P, 3), np.float32) if normal is None else np.array(normal, np.float32).reshape(P, 3),
                     max_distance=np.zeros(P, np.float32) if max_distance is None else np.array(max_distance, np.float32).reshape(P),
                     min_distance=np.zeros(P, np.float32) if min_distance is None else np.array(min_distance, np.float32).reshape(P),
                     status=np.zeros(P, np.int32))
    d, g = bool(what & DESCRIPTOR), bool(what & NORMAL_DEPTH)
    ctx._check(ctx._L.dsh_mappoint_update(ctx._h, store._h if store is not None else None, P, _ptr(xyz, C.c_float), _ptr(ptr, C.c_int32),
                                          _ptr(kf, C.c_int32), _ptr(idx, C.c_int32), _ptr(ref, C.c_int32), int(what),
                                          _ptr(r.desc, C.c_uint8) if d else None, _ptr(r.best, C.c_int32) if d else None,
                                          _ptr(r.normal, C.c_float) if g else None, _ptr(r.max_distance, C.c_float) if g else None,
                                          _ptr(r.min_distance, C.c_float) if g else None, _ptr(r.status, C.c_int32)), "dsh_mappoint_update")
    return r


@dataclass
class MapPoint:
    """The members of ORB_SLAM2::MapPoint the upkeep reads and writes."""
    xyz: np.ndarray                             # (3,) float32 mWorldPos
    ref_kf: int                                 # mpRefKF (store slot)
    obs: Dict[int, int] = field(default_factory=dict)   # mObservations: slot -> key point index
    desc: np.ndarray = field(default_factory=lambda: np.zeros(32, np.uint8))
    normal: np.ndarray = field(default_factory=lambda: np.zeros(3, np.float32))
    max_distance: float = 0.0
    min_distance: float = 0.0
    bad: bool = False


def obs_in_order(mp: MapPoint, order: Optional[Sequence[int]] = None) -> List[Tuple[int, int]]:
    """mObservations in the reference's iteration order: std::map<KeyFrame*, size_t> orders by keyframe address, which the caller
    models with order[slot] (a rank per slot); by slot when None."""
    key = (lambda s: s) if order is None else (lambda s: order[s])
    return sorted(mp.obs.items(), key=lambda kv: key(kv[0]))


def update_points(ctx: Context, store: KeyFrameStore, points: Sequence[MapPoint], what: int = BOTH, order=None) -> UpdateResult:
    """One batched update of MapPoint objects (CreateNewMapPoints, MonocularInitialization, Repose): writes the results back."""
    if not points:
        return None
    res = update(ctx, store, np.stack([np.asarray(p.xyz, np.float32) for p in points]), [obs_in_order(p, order) for p in points],
                 [p.ref_kf for p in points], what, desc=np.stack([p.desc for p in points]), normal=np.stack([p.normal for p in points]),
                 max_distance=[p.max_distance for p in points], min_distance=[p.min_distance for p in points])
    for i, p in enumerate(points):
        p.desc = res.desc[i].copy()
        p.normal = res.normal[i].copy()
        p.max_distance, p.min_distance = res.max_distance[i], res.min_distance[i]
    return res


def process_new_keyframe(ctx: Context, store: KeyFrameStore, slot: int, matches: Sequence[Optional[MapPoint]], order=None):
    """LocalMapping::ProcessNewKeyFrame's loop (LocalMapping.cc:142-161) for the keyframe in `slot` with mvpMapPoints = matches: bad points
    are skipped; a point that does not observe the keyframe yet gets AddObservation(pKF, i) and is updated (UpdateNormalAndDepth, then
    ComputeDistinctiveDescriptors), in one batch after the loop -- the points do not interact, so the batch is exact; a point that already
    observes it (its second key point in this keyframe, or a point the tracking inserted) goes to the recently-added list instead.
    Returns (updated points, recently added points)."""
    updated, recent = [], []
    for i, mp in enumerate(matches):
        if mp is None or mp.bad:
            continue
        if slot not in mp.obs:
            mp.obs[slot] = i
            updated.append(mp)
        else:
            recent.append(mp)
    update_points(ctx, store, updated, BOTH, order)
    return updated, recent
