"""TEST INFRASTRUCTURE ONLY: sequential restatement of the two tracking searches (the checker of dsh_search_by_projection_*).

Plain Python, one query at a time, explicit np.float32 scalars, statement by statement after the reference:
  ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono) ..... Thirdparty/ORBSLAM_2/src/ORBmatcher.cc:1360-1510 (monocular)
  ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>, th) ....... ORBmatcher.cc:42-136, RadiusByViewingCos :138-143
  Tracking::SearchLocalPoints ........................................... Tracking.cc:1405-1470
  Frame::isInFrustum .................................................... Frame.cc:338-390
  MapPoint::PredictScale ................................................ MapPoint.cc:422-437
  Frame::GetFeaturesInArea / PosInGrid / AssignFeaturesToGrid ........... Frame.cc:421-480, 484-496, 296-308
The grid is the reference's: a list of index lists per cell, filled in key point order, walked column by column.
OpenCV arithmetic is restated as include/defslam_hip.h states it (float32 3-term products with tcw added in double; cv::norm and
cv::Mat::dot in double).  Nothing in defslam_amd/ imports this module.
"""
from __future__ import annotations

import math

import numpy as np

f32 = np.float32
TH_HIGH = 75                       # ORBmatcher.cc:35
NN_RATIO = f32(0.8)                # ORBmatcher matcher(0.8, false), Tracking.cc:1460


def _round(x):
    """C round(): half away from zero (exact in double for a float32 argument)."""
    x = float(x)
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def _desc_ints(desc):
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    return [int.from_bytes(row.tobytes(), "little") for row in d]


class RefFrame:
    """The members of ORB_SLAM2::Frame the searches read (float32 where the reference is float)."""

    def __init__(self, Tcw, K, bounds, kp, octave, desc, scale_factors, log_scale_factor, Ow, grid=(64, 48)):
        T = np.asarray(Tcw, np.float32).reshape(4, 4)
        self.R = [[f32(T[i, k]) for k in range(3)] for i in range(3)]
        self.t = [f32(T[i, 3]) for i in range(3)]
        self.Ow = [f32(x) for x in np.asarray(Ow, np.float32)]
        self.fx, self.fy, self.cx, self.cy = (f32(x) for x in np.asarray(K, np.float32))
        self.minX, self.maxX, self.minY, self.maxY = (f32(x) for x in np.asarray(bounds, np.float32))
        self.cols, self.rows = int(grid[0]), int(grid[1])
        # Frame.cc:97-98
        self.winv = f32(f32(self.cols) / f32(self.maxX - self.minX))
        self.hinv = f32(f32(self.rows) / f32(self.maxY - self.minY))
        kp = np.asarray(kp, np.float32).reshape(-1, 2)
        self.kx = [f32(x) for x in kp[:, 0]]
        self.ky = [f32(y) for y in kp[:, 1]]
        self.oct = [int(o) for o in np.asarray(octave)]
        self.desc = _desc_ints(desc)
        self.sf = [f32(s) for s in np.asarray(scale_factors, np.float32)]
        self.levels = len(self.sf)
        self.logsf = f32(log_scale_factor)
        self.N = len(self.kx)
        # AssignFeaturesToGrid (Frame.cc:296-308) with PosInGrid (Frame.cc:484-496)
        self.grid = [[[] for _ in range(self.rows)] for _ in range(self.cols)]
        for i in range(self.N):
            px = _round(f32(f32(self.kx[i] - self.minX) * self.winv))
            py = _round(f32(f32(self.ky[i] - self.minY) * self.hinv))
            if px < 0 or px >= self.cols or py < 0 or py >= self.rows:
                continue
            self.grid[px][py].append(i)

    def cam(self, x, y, z):
        """Rcw * x3Dw + tcw of float cv::Mats (see the module docstring)."""
        out = []
        for k in range(3):
            s = f32(f32(self.R[k][0] * x) + f32(self.R[k][1] * y))
            s = f32(s + f32(self.R[k][2] * z))
            out.append(f32(float(s) + float(self.t[k])))
        return out

    def features_in_area(self, x, y, r, minLevel, maxLevel):
        """Frame::GetFeaturesInArea (Frame.cc:421-480)."""
        v = []
        nMinCellX = max(0, int(math.floor(f32(f32(f32(x - self.minX) - r) * self.winv))))
        if nMinCellX >= self.cols:
            return v
        nMaxCellX = min(self.cols - 1, int(math.ceil(f32(f32(f32(x - self.minX) + r) * self.winv))))
        if nMaxCellX < 0:
            return v
        nMinCellY = max(0, int(math.floor(f32(f32(f32(y - self.minY) - r) * self.hinv))))
        if nMinCellY >= self.rows:
            return v
        nMaxCellY = min(self.rows - 1, int(math.ceil(f32(f32(f32(y - self.minY) + r) * self.hinv))))
        if nMaxCellY < 0:
            return v
        bCheckLevels = (minLevel > 0) or (maxLevel >= 0)
        for ix in range(nMinCellX, nMaxCellX + 1):
            for iy in range(nMinCellY, nMaxCellY + 1):
                for j in self.grid[ix][iy]:
                    if bCheckLevels:
                        if self.oct[j] < minLevel:
                            continue
                        if maxLevel >= 0 and self.oct[j] > maxLevel:
                            continue
                    distx = f32(self.kx[j] - x)
                    disty = f32(self.ky[j] - y)
                    if abs(distx) < r and abs(disty) < r:
                        v.append(j)
        return v


def search_frame(fr: RefFrame, state, xyz, octave, desc, th):
    """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, true).  state: per key point 0 / 1 / 2 (include/defslam_hip.h).
    Returns (match[Q], nmatches, state afterwards)."""
    mp = [int(s) for s in state]
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    qd = _desc_ints(desc)
    th = f32(th)
    match = np.full(xyz.shape[0], -1, np.int32)
    nmatches = 0
    for i in range(xyz.shape[0]):
        xc, yc, zc = fr.cam(f32(xyz[i, 0]), f32(xyz[i, 1]), f32(xyz[i, 2]))
        invzc = f32(1.0 / float(zc))                                   # :1393 double 1.0 / float, stored as float
        if invzc < 0:
            continue
        u = f32(f32(fr.fx * xc) * invzc) + fr.cx
        v = f32(f32(fr.fy * yc) * invzc) + fr.cy
        if u != u or v != v:                                           # NaN (z == 0): outside by contract
            continue
        if u < fr.minX or u > fr.maxX:
            continue
        if v < fr.minY or v > fr.maxY:
            continue
        nLastOctave = int(octave[i])
        radius = f32(th * fr.sf[nLastOctave])
        vIndices2 = fr.features_in_area(u, v, radius, nLastOctave - 1, nLastOctave + 1)
        if not vIndices2:
            continue
        bestDist, bestIdx2 = 256, -1
        for i2 in vIndices2:
            if mp[i2] == 1:                                            # a map point with observations
                continue
            dist = (qd[i] ^ fr.desc[i2]).bit_count()
            if dist < bestDist:
                bestDist, bestIdx2 = dist, i2
        if bestDist <= TH_HIGH:
            if mp[bestIdx2]:                                           # :1462
                continue
            mp[bestIdx2] = 1
            match[i] = bestIdx2
            nmatches += 1
    return match, nmatches, np.asarray(mp, np.uint8)


def is_in_frustum(fr: RefFrame, P, Pn, max_distance, viewingCosLimit=f32(0.5)):
    """Frame::isInFrustum (Frame.cc:338-390) + MapPoint::PredictScale (MapPoint.cc:422-437).  Returns None or (u, v, level, viewCos)."""
    x, y, z = (f32(a) for a in P)
    PcX, PcY, PcZ = fr.cam(x, y, z)
    if PcZ < f32(0.0):
        return None
    invz = f32(f32(1.0) / PcZ)
    u = f32(f32(fr.fx * PcX) * invz) + fr.cx
    v = f32(f32(fr.fy * PcY) * invz) + fr.cy
    if u != u or v != v:
        return None
    if u < fr.minX or u > fr.maxX:
        return None
    if v < fr.minY or v > fr.maxY:
        return None
    # maxDistance / minDistance are read and never used in DefSLAM's isInFrustum: no distance-range test
    PO = [f32(x - fr.Ow[0]), f32(y - fr.Ow[1]), f32(z - fr.Ow[2])]
    dist = f32(math.sqrt(float(PO[0]) * float(PO[0]) + float(PO[1]) * float(PO[1]) + float(PO[2]) * float(PO[2])))   # cv::norm
    n = [f32(a) for a in Pn]
    dot = float(PO[0]) * float(n[0]) + float(PO[1]) * float(n[1]) + float(PO[2]) * float(n[2])                    # cv::Mat::dot
    viewCos = f32(dot / float(dist))
    if viewCos < viewingCosLimit:
        return None
    ratio = f32(f32(max_distance) / dist)
    nScale = int(math.ceil(math.log(float(ratio)) / float(fr.logsf)))
    if nScale < 0:
        nScale = 0
    elif nScale >= fr.levels:
        nScale = fr.levels - 1
    return u, v, nScale, viewCos


def search_local(fr: RefFrame, state, xyz, normal, max_distance, desc, skip, th):
    """Tracking::SearchLocalPoints' isInFrustum pass (Tracking.cc:1440-1456) and ORBmatcher(0.8).SearchByProjection(F, points, th).
    Returns (match, nmatches, state afterwards, in_view, level, uv, viewCos)."""
    mp = [int(s) for s in state]
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    normal = np.asarray(normal, np.float32).reshape(-1, 3)
    Q = xyz.shape[0]
    qd = _desc_ints(desc)
    th = f32(th)
    in_view = np.zeros(Q, bool)
    level = np.zeros(Q, np.int32)
    uv = np.zeros((Q, 2), np.float32)
    vcos = np.zeros(Q, np.float32)
    for q in range(Q):
        if skip is not None and skip[q]:
            continue
        r = is_in_frustum(fr, xyz[q], normal[q], max_distance[q])
        if r is not None:
            in_view[q] = True
            uv[q] = r[0], r[1]
            level[q] = r[2]
            vcos[q] = r[3]
    match = np.full(Q, -1, np.int32)
    nmatches = 0
    bFactor = th != f32(1.0)
    for q in range(Q):
        if not in_view[q]:
            continue
        nPredictedLevel = int(level[q])
        r = f32(2.5) if float(vcos[q]) > 0.998 else f32(4.0)           # RadiusByViewingCos
        if bFactor:
            r = f32(r * th)
        vIndices = fr.features_in_area(uv[q, 0], uv[q, 1], f32(r * fr.sf[nPredictedLevel]), nPredictedLevel - 1, nPredictedLevel)
        if not vIndices:
            continue
        bestDist, bestLevel, bestDist2, bestLevel2, bestIdx = 256, -1, 256, -1, -1
        for idx in vIndices:
            if mp[idx] == 1:
                continue
            dist = (qd[q] ^ fr.desc[idx]).bit_count()
            if dist < bestDist:
                bestDist2, bestDist = bestDist, dist
                bestLevel2, bestLevel = bestLevel, fr.oct[idx]
                bestIdx = idx
            elif dist < bestDist2:
                bestLevel2 = fr.oct[idx]
                bestDist2 = dist
        if bestDist <= TH_HIGH:
            if bestLevel == bestLevel2 and f32(bestDist) > f32(NN_RATIO * f32(bestDist2)):
                continue
            mp[bestIdx] = 1                                            # F.mvpMapPoints[bestIdx] = pMP (overwrites)
            match[q] = bestIdx
            nmatches += 1
    return match, nmatches, np.asarray(mp, np.uint8), in_view, level, uv, vcos


def ref_frame(tf) -> RefFrame:
    """RefFrame of a defslam_amd.track.TrackFrame."""
    a = tf.arrays()
    return RefFrame(a["Tcw"], a["K"], a["bounds"], a["kp"], a["octave"], a["desc"], a["sf"], tf.log_scale_factor, a["Ow"], tf.grid)


def motion_model(tf, xyz, octave, desc):
    """DefTracking::TrackWithMotionModel (DefTracking.cc:342-375): (match, nmatches, th, state)."""
    fr = ref_frame(tf)
    zero = np.zeros(fr.N, np.uint8)
    m, n, st = search_frame(fr, zero, xyz, octave, desc, 20)
    th = 20
    if n < 20:
        m, n, st = search_frame(fr, zero, xyz, octave, desc, 25)
        th = 25
    return m, n, th, st
