"""The ORB feature front end on the device (include/defslam_hip.h: dsh_orb_*): ORB_SLAM2::ORBextractor::operator() as two device stages,
detect and describe, with the caller's DistributeOctTree between them.  The OpenCV steps are readings stated in the header, not verified
against an OpenCV build."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .sft import DshError, _ptr


def features_per_level(n_features: int, levels: int, scale_factor: float) -> list:
    """mnFeaturesPerLevel (ORBextractor.cc:436-446), float32 as the reference computes it."""
    f32 = np.float32
    factor = f32(1.0) / f32(scale_factor)
    wanted = f32(n_features) * (f32(1.0) - factor) / (f32(1.0) - f32(float(factor) ** levels))
    out, total = [], 0
    for _ in range(levels - 1):
        out.append(int(np.rint(wanted)))
        total += out[-1]
        wanted = f32(wanted * factor)
    out.append(max(n_features - total, 0))
    return out


class OrbExtractor:
    def __init__(self, ctx, width, height, pattern, levels=8, scale_factor=1.2, ini_th=20, min_th=7, capacity=8192, n_features=1000):
        self._ctx = ctx
        self._L = ctx._L
        self.width, self.height, self.levels, self.capacity, self.n_features = int(width), int(height), int(levels), int(capacity), int(n_features)
        self.scale_factor = float(scale_factor)
        pattern = np.ascontiguousarray(pattern, np.int32).reshape(-1)
        if pattern.size != 1024:
            raise ValueError("pattern: 512 points (x, y)")
        cfg = _lib.OrbConfigC(ctx._h, self.width, self.height, self.levels, self.scale_factor, int(ini_th), int(min_th), self.capacity,
                              _ptr(pattern, C.c_int32))
        h = C.c_void_p()
        self._h = None
        ctx._check(self._L.dsh_orb_create(C.byref(cfg), C.byref(h)), "dsh_orb_create")
        self._h = h
        wh = np.zeros((self.levels, 2), np.int32)
        sf = np.zeros(self.levels, np.float32)
        ctx._check(self._L.dsh_orb_level_sizes(self._h, _ptr(wh, C.c_int32), _ptr(sf, C.c_float)), "dsh_orb_level_sizes")
        self._wh, self._sf = wh, sf

    def close(self):
        if self._h is not None:
            self._L.dsh_orb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def level_sizes(self):
        """(levels x 2 int32: width, height), (levels float32: the scale factor of each level)."""
        return self._wh.copy(), self._sf.copy()

    def detect(self, image):
        """The candidates of every level: a list of (n_l x 3) int32 arrays x, y, response, in the reference's order.  A level with more
        than `capacity` candidates raises DshError; its `counts` holds the true counts."""
        image = np.asarray(image)
        if image.dtype != np.uint8 or image.shape != (self.height, self.width) or image.strides[1] != 1 or image.strides[0] < self.width:
            raise ValueError("image: uint8, height x width, rows contiguous")
        counts = np.zeros(self.levels, np.int32)
        cand = np.zeros((self.levels, self.capacity, 3), np.int32)
        rc = self._L.dsh_orb_detect(self._h, C.cast(image.ctypes.data, _lib.c_u8_p), image.strides[0], _ptr(counts, C.c_int32), _ptr(cand, C.c_int32))
        if rc != _lib.DSH_OK:
            e = DshError(f"dsh_orb_detect: status {rc}: {self._L.dsh_last_error(self._ctx._h).decode()}")
            e.status, e.counts = rc, counts
            raise e
        return [cand[l, :counts[l]].copy() for l in range(self.levels)]

    def describe(self, level, xy):
        """Angles (degrees, float32) and 32-byte descriptors of key points given by level and position in level pixels."""
        level = np.ascontiguousarray(level, np.int32).reshape(-1)
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        n = level.shape[0]
        if xy.shape[0] != n:
            raise ValueError("level and xy differ in length")
        angle = np.zeros(n, np.float32)
        desc = np.zeros((n, 32), np.uint8)
        self._ctx._check(self._L.dsh_orb_describe(self._h, n, _ptr(level, C.c_int32), _ptr(xy, C.c_float), _ptr(angle, C.c_float), _ptr(desc, C.c_uint8)),
                         "dsh_orb_describe")
        return angle, desc

    def plane(self, level, blurred):
        """The level with its 19-pixel frame (blurred false), or the blurred plane 3 pixels beyond the level."""
        w, h = self._wh[level]
        m = 3 if blurred else 19
        out = np.zeros((h + 2 * m, w + 2 * m), np.uint8)
        self._ctx._check(self._L.dsh_orb_get_plane(self._h, int(level), 1 if blurred else 0, _ptr(out, C.c_uint8)), "dsh_orb_get_plane")
        return out

    def extract(self, image, distribute):
        """The whole of operator(): detect, the caller's distribute(level, candidates, n_wanted) -> indices into the level's candidates,
        describe.  Returns a dict of arrays ordered by level: pt (image pixels), octave, size, angle, response, desc."""
        cand = self.detect(image)
        wanted = features_per_level(self.n_features, self.levels, self.scale_factor)
        lv, xy, resp = [], [], []
        for l in range(self.levels):
            idx = np.asarray(distribute(l, cand[l], wanted[l]), np.int64).reshape(-1)
            sel = cand[l][idx]
            lv.append(np.full(sel.shape[0], l, np.int32))
            xy.append(sel[:, :2].astype(np.float32))
            resp.append(sel[:, 2].astype(np.float32))
        lv, xy, resp = np.concatenate(lv), np.concatenate(xy).reshape(-1, 2), np.concatenate(resp)
        angle, desc = self.describe(lv, xy)
        sf = self._sf[lv]
        pt = np.where((lv > 0)[:, None], xy * sf[:, None], xy).astype(np.float32)     # pt *= scale for l > 0 (:1108-1113)
        size = (np.float32(31.0) * sf).astype(np.int32).astype(np.float32)             # (int)(PATCH_SIZE * sf[l]) (:841)
        return dict(pt=pt, octave=lv, size=size, angle=angle, response=resp, desc=desc)
