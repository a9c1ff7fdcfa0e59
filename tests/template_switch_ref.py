"""TEST INFRASTRUCTURE ONLY: sequential restatement of the template switch (the checker of dsh_need_new_template, dsh_template_switch
and dsh_surface_vertices) on top of tests/track_close_ref.py (the host mirror TrackRefMap) and tests/mappoint_ref.py
(UpdateNormalAndDepth).

Plain Python, statement by statement after the reference:
  DefLocalMapping::updateTemplate ............. Modules/Mapping/DefLocalMapping.cc:138-153
  DefLocalMapping::CreateNewMapPoints ......... DefLocalMapping.cc:240-347
  DefLocalMapping::needNewTemplate ............ DefLocalMapping.cc:355-404
  DefMap::clearTemplate ....................... Modules/Common/DefMap.cc:67-82
  TriangularMesh::TriangularMesh .............. Modules/Template/TriangularMesh.cc:57-89
  Surface::getVertex .......................... Modules/Mapping/Surface.cc:125-161
The occupancy mask is built as an image: the held pixels, then the k x k box with BORDER_REFLECT_101 read pixel by pixel (the reading of
cv::filter2D + cv::threshold that include/defslam_hip.h states).  masked_by_interval is the form the device uses; the CPU test holds the
two against each other.  The embedding itself is not restated here: the caller passes the host routine (Context.template_embed).
Nothing in defslam_amd/ imports this module.
"""
from __future__ import annotations

import numpy as np

import mappoint_ref as M
import track_close_ref as T

f32 = np.float32
COUNT_NAMES = ("n_new", "first_id", "n_moved", "n_masked", "n_embedded", "n_points")


class RefKfData:
    """The keyframe store's side of a keyframe, as mappoint_ref reads it."""

    def __init__(self, Ow, desc, octave, scale_factors, bad=False):
        self.Ow = np.asarray(Ow, np.float32).reshape(3)
        self.desc = np.asarray(desc, np.uint8).reshape(-1, 32)
        self.octave = np.asarray(octave, np.int32).reshape(-1)
        self.scale_factors = np.asarray(scale_factors, np.float32).reshape(-1)
        self.bad = bool(bad)


def pixel(kp):
    """mask.at<char>(pt.y, pt.x): the float to int conversion truncates toward zero -> (y, x)."""
    return int(f32(kp[1])), int(f32(kp[0]))


def reflect101(p, n):
    """BORDER_REFLECT_101 for a window shorter than the axis."""
    if p < 0:
        return -p
    if p >= n:
        return 2 * (n - 1) - p
    return p


def kernel_of(cols):
    k = cols // 20
    return k, k // 2


def box_mask(rows, cols, held_pixels):
    """mask != 0 after filter2D (k x k ones, anchor k / 2, BORDER_REFLECT_101) and threshold > 1, as a (rows, cols) bool image: a pixel is
    set when its reflected window holds at least one held pixel.  The box is separable and so is the reflection."""
    k, a = kernel_of(cols)
    assert 2 <= k < rows and k < cols
    src = np.zeros((rows, cols), bool)
    for y, x in held_pixels:
        src[y, x] = True
    ix = np.array([[reflect101(x + d, cols) for d in range(-a, k - a)] for x in range(cols)])       # (cols, k)
    iy = np.array([[reflect101(y + d, rows) for d in range(-a, k - a)] for y in range(rows)])       # (rows, k)
    along_x = src[:, ix].any(axis=2)                                                                 # (rows, cols)
    return along_x[iy, :].any(axis=1)                                                                # (rows, cols)


def interval(x, k, a, n):
    """The source pixels [L, H] the window of pixel x reads along an axis of n pixels (include/defslam_hip.h)."""
    lo, hi = x - a, x + k - 1 - a
    L, H = max(lo, 0), min(hi, n - 1)
    if lo < 0:
        H = max(H, -lo)
    if hi > n - 1:
        L = min(L, 2 * (n - 1) - hi)
    return L, H


def masked_by_interval(rows, cols, held_pixels, y, x):
    k, a = kernel_of(cols)
    Lx, Hx = interval(x, k, a, cols)
    Ly, Hy = interval(y, k, a, rows)
    return any(Lx <= px <= Hx and Ly <= py <= Hy for py, px in held_pixels)


def to_world(Twc, s):
    """x3wh = Twc * x3ch of float32 cv::Mat: the four products of a row summed left to right in float32."""
    T = np.asarray(Twc, np.float32).reshape(4, 4)
    x, y, z, w = f32(s[0]), f32(s[1]), f32(s[2]), f32(1)
    return np.array([f32(f32(f32(T[r, 0] * x) + f32(T[r, 1] * y)) + f32(T[r, 2] * z)) + f32(T[r, 3] * w) for r in range(3)], np.float32)


class TemplateRefMap(T.TrackRefMap):
    """TrackRefMap with the template switch of the mapping thread."""

    def held_pixels(self, slot, kp):
        """:249-259 / :363-373: the pixels of the key points that hold a point that is not bad."""
        return [pixel(kp[i]) for i, p in enumerate(self.kfs[slot].table) if p >= 0 and not self.points[p].bad]

    def need_new_template(self, slot, rows, cols, kp):
        """DefLocalMapping::needNewTemplate: (newPoints, candidate flags)."""
        mask = box_mask(rows, cols, self.held_pixels(slot, kp))
        cand = np.zeros(len(self.kfs[slot].table), bool)
        for i, p in enumerate(self.kfs[slot].table):                        # :386-398
            if p < 0 and not mask[pixel(kp[i])]:
                cand[i] = True
        return int(cand.sum()), cand

    def switch_template(self, kfs, slot, rows, cols, kp, surface_pts, Twc, embed, rest_xyz):
        """DefLocalMapping::updateTemplate on the mirror with the keyframe store's side kfs (RefKfData per slot).
        embed(pts) -> (facet id, nodes, float32 barycentrics) is the host embedding in the new template, rest_xyz its nodes.
        Returns the counts (COUNT_NAMES), new_idx, and pre_embed: the positions the embedding was fed (every point, bad ones too)."""
        c = dict.fromkeys(COUNT_NAMES, 0)
        self.clear_embedding()                                              # DefMap::clearTemplate
        mask = box_mask(rows, cols, self.held_pixels(slot, kp))             # :245-271
        c["first_id"] = len(self.points)
        new_idx = []
        table = self.kfs[slot].table
        for i in range(len(table)):                                         # :273-345
            p = table[i]
            if p >= 0:
                if self.points[p].bad:
                    continue
                self.points[p].xyz = to_world(Twc, surface_pts[i])          # SetWorldPos
                c["n_moved"] += 1
            else:
                if mask[pixel(kp[i])]:
                    c["n_masked"] += 1
                    continue
                x3w = to_world(Twc, surface_pts[i])
                q = self.add_point(xyz=x3w, desc=kfs[slot].desc[i])         # new DefMapPoint(x3w, referenceKF_, mpMap)
                assert self.add_observation(q, slot)                        # :337
                table[i] = q                                                # :338
                pt = self.points[q]                                         # :340-341: one observation elects its descriptor
                pt.normal, pt.max_distance, _ = M.update_normal_and_depth(kfs, x3w, [(slot, i)], slot)
                new_idx.append(i)
        c["n_new"] = len(new_idx)
        c["n_points"] = len(self.points)
        pre_embed = np.array([pt.xyz for pt in self.points], np.float32).reshape(-1, 3)
        ids = [p for p, pt in enumerate(self.points) if not pt.bad]         # Map::GetAllMapPoints holds no bad point
        if ids:
            fid, nodes, bary = embed(pre_embed[ids])                        # calculateFeaturesCoordinates
            for n, p in enumerate(ids):
                if fid[n] < 0:
                    continue
                order = np.argsort(nodes[n], kind="stable")                 # std::set<Node*> order
                self.set_embedding(p, nodes[n][order], np.asarray(bary[n], np.float32)[order].astype(np.float64))
                c["n_embedded"] += 1
        self.repose(rest_xyz)                                               # Repose -> RecalculatePosition of every point with a facet
        return c, np.array(new_idx, np.int32), pre_embed


def surface_vertices(bbs, depth, Twc, xs, ys):
    """Surface::getVertex + the Node positions: depth(u, v) -> d evaluates the keyframe's depth spline in double.
    Returns (world (xs * ys, 3) float64, camera (xs * ys, 3) float32)."""
    umin, umax, _, vmin, vmax, _, _ = bbs
    t = 0.03
    u = np.array([np.float64((umax - umin - 2 * t) * x) / (xs - 1) + (umin + t) for x in range(xs) for _ in range(ys)])
    v = np.array([np.float64((vmax - vmin - 2 * t) * j) / (ys - 1) + (vmin + t) for _ in range(xs) for j in range(ys)])
    d = np.asarray(depth(u, v), np.float64).reshape(-1)
    cam = np.stack([(u * d).astype(np.float32), (v * d).astype(np.float32), d.astype(np.float32)], 1)
    world = np.array([to_world(Twc, s) for s in cam], np.float32).astype(np.float64)
    return world, cam


def scene_kf_data(sc):
    return [RefKfData(sc["kf_Ow"][k], sc["kf_desc"][k], sc["kf_octave"][k], sc["scale_factors"], sc["kf_bad"][k]) for k in range(sc["tables"].shape[0])]


def scene_to_ref(sc, embed=True):
    return T.scene_to_ref(sc, embed, cls=TemplateRefMap)
