"""TEST INFRASTRUCTURE ONLY: the images, sampling patterns and cases of the ORB front end's tests, from seeded NumPy, and the
restatement's results per case, computed once per process."""
import functools

import numpy as np

import orb_ref as R

# name: width, height, levels (scale factor 1.2, thresholds 20 and 7) -- the smallest shapes at which the kernels can go wrong: one cell; a
# 65-wide cell; 2 x 2 cells of 30; three levels; the skipped last cell column and row; the default frame
CASES = {
    "one_cell": (62, 62, 1),
    "wide_cell": (91, 62, 1),
    "four_cells": (92, 93, 1),
    "three_levels": (123, 100, 3),
    "skipped_column": (813, 62, 1),
    "skipped_row": (94, 903, 1),
    "default": (640, 480, 8),
}
SCALE, INI_TH, MIN_TH = 1.2, 20, 7

KINDS = ("shapes", "noise", "flat", "faint")


def _draw_shapes(rng, w, h, base, levels, n_shapes):
    """Random filled rectangles and triangles, each at one of `levels`, over a constant `base`."""
    img = np.full((h, w), base, np.int32)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(n_shapes):
        g = int(levels[rng.integers(len(levels))])
        if rng.integers(2):
            x0, y0 = int(rng.integers(-5, w - 5)), int(rng.integers(-5, h - 5))
            x1, y1 = x0 + int(rng.integers(6, max(8, w // 3))), y0 + int(rng.integers(6, max(8, h // 3)))
            img[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = g
        else:
            p = np.stack([rng.integers(-5, w + 5, 3), rng.integers(-5, h + 5, 3)], 1).astype(np.int64)
            e = [(p[(i + 1) % 3] - p[i]) for i in range(3)]
            s = [e[i][0] * (yy - p[i][1]) - e[i][1] * (xx - p[i][0]) for i in range(3)]
            inside = ((s[0] >= 0) & (s[1] >= 0) & (s[2] >= 0)) | ((s[0] <= 0) & (s[1] <= 0) & (s[2] <= 0))
            img[inside] = g
    return img


def image(kind, w, h, seed=0):
    """uint8, h x w.  shapes: rectangles and triangles at random grey levels plus noise of +-2; noise: uniform 0 .. 255; flat: constant;
    faint: shapes at the grey levels 100, 110 and 117 plus noise of +-1, so that no two pixels differ by more than 19."""
    rng = np.random.default_rng([seed, w, h, KINDS.index(kind)])
    n_shapes = max(6, w * h // 600)
    if kind == "shapes":
        img = _draw_shapes(rng, w, h, 128, np.arange(10, 246), n_shapes) + rng.integers(-2, 3, (h, w))
    elif kind == "noise":
        img = rng.integers(0, 256, (h, w))
    elif kind == "flat":
        img = np.full((h, w), 93)
    elif kind == "faint":
        img = _draw_shapes(rng, w, h, 100, np.array([100, 110, 117]), n_shapes) + rng.integers(-1, 2, (h, w))
    else:
        raise ValueError(kind)
    return np.clip(img, 0, 255).astype(np.uint8)


def pattern(seed=0, corners=False):
    """512 points (256 pairs), int32 x, y with |x|, |y| <= 13; corners: the first four are (+-13, +-13)."""
    rng = np.random.default_rng([seed, 31])
    p = rng.integers(-13, 14, (512, 2)).astype(np.int32)
    if corners:
        p[:4] = [[13, 13], [-13, 13], [13, -13], [-13, -13]]
    return p


def top_n(level, cand, n_wanted):
    """A stand-in for DistributeOctTree: the n_wanted candidates of largest response, ties by position in the list, in list order."""
    order = np.argsort(-cand[:, 2], kind="stable")[:n_wanted]
    return np.sort(order)


@functools.lru_cache(maxsize=None)
def reference(case, kind):
    """The restatement on one case and image kind: image, pyramid, candidates per level.  Shared and never modified."""
    w, h, levels = CASES[case]
    img = image(kind, w, h)
    pyr = R.pyramid(img, levels, SCALE)
    cand = R.detect(img, levels, SCALE, INI_TH, MIN_TH, pyr)
    return dict(image=img, pyr=pyr, cand=cand, levels=levels)


def describe_points(case, kind):
    """The key points the describe tests use: per level the first 300 candidates, the eight positions exactly 16 pixels from the edges
    (corners and edge centres) and a 12 x 10 grid of fractional positions over the admissible range.  level (n), xy (n x 2 float32)."""
    ref = reference(case, kind)
    lv, xy = [], []
    for l, (level, _, _) in enumerate(ref["pyr"]):
        h, w = level.shape
        x1, y1 = w - 17, h - 17
        edge = [(16, 16), (x1, 16), (16, y1), (x1, y1), (16, h // 2), (x1, h // 2), (w // 2, 16), (w // 2, y1)]
        gx, gy = np.meshgrid(np.linspace(16, x1, 12), np.linspace(16, y1, 10))
        pts = np.concatenate([ref["cand"][l][:300, :2].astype(np.float32), np.array(edge, np.float32),
                              np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)])
        pts[:, 0] = np.clip(pts[:, 0], 16, x1)           # a float32 grid end may round just outside
        pts[:, 1] = np.clip(pts[:, 1], 16, y1)
        lv.append(np.full(len(pts), l, np.int32))
        xy.append(pts)
    return np.concatenate(lv), np.concatenate(xy)


@functools.lru_cache(maxsize=None)
def described(case, kind):
    """The restatement's angles, descriptors and fragile-bit masks of describe_points with the (+-13, +-13) pattern."""
    lv, xy = describe_points(case, kind)
    return (lv, xy) + R.describe(reference(case, kind)["pyr"], pattern(corners=True), lv, xy)
