"""TEST INFRASTRUCTURE ONLY: the ORB front end restated in NumPy, step by step as include/defslam_hip.h defines it (ORBextractor.cc
:1047-1118).  The OpenCV steps are readings of OpenCV's documented behaviour in integers or single float32 operations, not verified
against an OpenCV build; tests/test_orb_cpu.py pins each against an independent formulation.  The device is held to this file exactly."""
import numpy as np

f32 = np.float32
PATCH_SIZE, HALF_PATCH_SIZE, EDGE_THRESHOLD, W_CELL = 31, 15, 19, 30
BLUR_MARGIN = 3
BLUR_Q = np.array([18, 34, 49, 55, 49, 34, 18], np.int64)
# the radius-3 circle of 16, (dx, dy), contiguous
CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


def cv_round(v):
    return np.rint(v).astype(np.int64)


# ---- scale table, level sizes, features per level ------------------------------------------------------------------------------------
def scale_table(levels, scale_factor):
    sf = np.zeros(levels, f32)
    sf[0] = 1.0
    for l in range(1, levels):
        sf[l] = sf[l - 1] * f32(scale_factor)
    return sf, (f32(1.0) / sf).astype(f32)


def level_sizes(w0, h0, levels, scale_factor):
    _, inv = scale_table(levels, scale_factor)
    return [(int(cv_round(f32(w0) * inv[l])), int(cv_round(f32(h0) * inv[l]))) for l in range(levels)]


def features_per_level(n_features, levels, scale_factor):
    factor = f32(1.0) / f32(scale_factor)
    wanted = f32(n_features) * (f32(1.0) - factor) / (f32(1.0) - f32(float(factor) ** levels))
    out = []
    for _ in range(levels - 1):
        out.append(int(cv_round(wanted)))
        wanted = f32(wanted * factor)
    return out + [max(n_features - sum(out), 0)]


# ---- pyramid -------------------------------------------------------------------------------------------------------------------------
def resize_taps(src, dst):
    """Per destination index: the first tap's index, the float fraction, and the fixed-point taps c0, c1 (11 bits)."""
    sc = np.float64(src) / np.float64(dst)
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * sc - 0.5).astype(f32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(f32)).astype(f32)
    lo, hi = s < 0, s >= src - 1
    s = np.where(lo, 0, np.where(hi, src - 1, s))
    f = np.where(lo | hi, f32(0), f).astype(f32)
    c0 = cv_round((f32(1.0) - f) * f32(2048))
    c1 = cv_round(f * f32(2048))
    return s, f, c0, c1


def resize(img, dw, dh):
    """INTER_LINEAR on 8-bit data, the fixed-point path."""
    h, w = img.shape
    sx, _, a0, a1 = resize_taps(w, dw)
    sy, _, b0, b1 = resize_taps(h, dh)
    sx1, sy1 = np.minimum(sx + 1, w - 1), np.minimum(sy + 1, h - 1)
    S = img.astype(np.int64)
    hrow = S[:, sx] * a0[None, :] + S[:, sx1] * a1[None, :]            # h x dw
    h0, h1 = hrow[sy], hrow[sy1]
    D = (((b0[:, None] * (h0 >> 4)) >> 16) + ((b1[:, None] * (h1 >> 4)) >> 16) + 2) >> 2
    return D.astype(np.uint8)


def resize_float(img, dw, dh):
    """The independent formulation: float64 bilinear interpolation with the same taps' positions and fractions."""
    h, w = img.shape
    sx, fx, _, _ = resize_taps(w, dw)
    sy, fy, _, _ = resize_taps(h, dh)
    sx1, sy1 = np.minimum(sx + 1, w - 1), np.minimum(sy + 1, h - 1)
    S = img.astype(np.float64)
    fx, fy = fx.astype(np.float64)[None, :], fy.astype(np.float64)[:, None]
    top = S[sy][:, sx] * (1 - fx) + S[sy][:, sx1] * fx
    bot = S[sy1][:, sx] * (1 - fx) + S[sy1][:, sx1] * fx
    return top * (1 - fy) + bot * fy


def frame(img, margin=EDGE_THRESHOLD):
    """BORDER_REFLECT_101 around the level itself."""
    return np.pad(img, margin, mode="reflect")


def blur_plane(framed):
    """The blurred plane, 3 pixels beyond the level on every side, from the framed level: row pass, column pass, exact integers."""
    F = framed.astype(np.int64)
    m = EDGE_THRESHOLD - BLUR_MARGIN                     # the blurred plane's origin inside the frame
    H, Wd = F.shape[0] - 2 * m, F.shape[1] - 2 * m
    rows = sum(BLUR_Q[i] * F[:, m - 3 + i:m - 3 + i + Wd] for i in range(7))           # all frame rows x Wd
    s = sum(BLUR_Q[j] * rows[m - 3 + j:m - 3 + j + H] for j in range(7))
    return np.minimum(255, (s + 32768) >> 16).astype(np.uint8)


def pyramid(image, levels, scale_factor):
    """Per level: (the level, the framed level, the blurred plane)."""
    sizes = level_sizes(image.shape[1], image.shape[0], levels, scale_factor)
    out = []
    for l, (w, h) in enumerate(sizes):
        lv = np.ascontiguousarray(image) if l == 0 else resize(out[-1][0], w, h)
        assert lv.shape == (h, w)
        fr = frame(lv)
        out.append((lv, fr, blur_plane(fr)))
    return out


# ---- FAST ----------------------------------------------------------------------------------------------------------------------------
def fast_m(img):
    """M(p) for every pixel at least 3 inside img: shape (h - 6, w - 6), int."""
    I = img.astype(np.int64)
    h, w = I.shape
    c = I[3:h - 3, 3:w - 3]
    d = np.stack([I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c for dx, dy in CIRCLE])
    best = np.full(c.shape, -256, np.int64)
    for sign in (1, -1):
        e = sign * d
        for k in range(16):
            arc = e[[(k + i) % 16 for i in range(9)]].min(0)
            best = np.maximum(best, arc)
    return best


def suppress(M, th):
    """The corners of a cell's detection region M at threshold th that survive the 3 x 3 suppression confined to the region."""
    corner = M > th
    resp = np.where(corner, M - 1, 0)
    p = np.pad(resp, 1)
    h, w = M.shape
    keep = corner.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= resp > p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return keep, resp


def cells(w, h):
    """The cells of a level of w x h: (i, j, iniX, iniY, maxX, maxY) of those that run, and the (i, j) the reference skips."""
    minB, maxBX, maxBY = EDGE_THRESHOLD - 3, w - EDGE_THRESHOLD + 3, h - EDGE_THRESHOLD + 3
    width, height = f32(maxBX - minB), f32(maxBY - minB)
    nCols, nRows = int(width / f32(W_CELL)), int(height / f32(W_CELL))
    wCell, hCell = int(np.ceil(width / f32(nCols))), int(np.ceil(height / f32(nRows)))
    run, skipped = [], []
    for i in range(nRows):
        iniY = minB + i * hCell
        if iniY >= maxBY - 3:
            skipped += [(i, j) for j in range(nCols)]
            continue
        maxY = min(iniY + hCell + 6, maxBY)
        for j in range(nCols):
            iniX = minB + j * wCell
            if iniX >= maxBX - 6:
                skipped.append((i, j))
                continue
            run.append((i, j, iniX, iniY, min(iniX + wCell + 6, maxBX), maxY))
    return run, skipped, (nCols, nRows, wCell, hCell)


def detect_level(level, ini_th, min_th, per_cell=False):
    """Candidates of one level, (n x 3) int: x, y, response, in the reference's order.  M is a function of the pixel alone (its circle lies
    inside the cell's sub-image), so it is computed once per level; per_cell=True computes it from each sub-image instead."""
    h, w = level.shape
    M_all = None if per_cell else fast_m(level)
    out, retried = [], 0
    for (_, _, x0, y0, x1, y1) in cells(w, h)[0]:
        if x1 - x0 < 7 or y1 - y0 < 7:
            continue
        M = fast_m(level[y0:y1, x0:x1]) if per_cell else M_all[y0:y1 - 6, x0:x1 - 6]
        keep, resp = suppress(M, ini_th)
        if not keep.any():
            retried += 1
            keep, resp = suppress(M, min_th)
        ys, xs = np.nonzero(keep)                        # raster order
        out.append(np.stack([xs + x0 + 3, ys + y0 + 3, resp[ys, xs]], 1))
    cand = np.concatenate(out) if out else np.zeros((0, 3), np.int64)
    return cand.astype(np.int32).reshape(-1, 3), retried


def detect(image, levels, scale_factor, ini_th, min_th, pyr=None):
    pyr = pyr or pyramid(image, levels, scale_factor)
    return [detect_level(p[0], ini_th, min_th)[0] for p in pyr]


# ---- angle ---------------------------------------------------------------------------------------------------------------------------
def umax_table():
    """ORBextractor.cc:454-469."""
    umax = [0] * (HALF_PATCH_SIZE + 1)
    vmax = int(np.floor(f32(HALF_PATCH_SIZE) * np.sqrt(f32(2.0)) / f32(2) + f32(1)))
    vmin = int(np.ceil(f32(HALF_PATCH_SIZE) * np.sqrt(f32(2.0)) / f32(2)))
    hp2 = float(HALF_PATCH_SIZE * HALF_PATCH_SIZE)
    for v in range(vmax + 1):
        umax[v] = int(cv_round(np.sqrt(hp2 - v * v)))
    v0 = 0
    for v in range(HALF_PATCH_SIZE, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return umax


UMAX = umax_table()
_DEG = f32(180.0 / np.pi)
_P1, _P3, _P5, _P7 = (f32(p) * _DEG for p in (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128))


def fast_atan2(y, x):
    """cv::fastAtan2 read as the scalar polynomial; float32 arrays in, degrees out."""
    y, x = np.asarray(y, f32), np.asarray(x, f32)
    ax, ay = np.abs(x), np.abs(y)
    eps = f32(np.finfo(np.float64).eps)
    big = ax >= ay
    c = (np.where(big, ay, ax) / (np.where(big, ax, ay) + eps)).astype(f32)
    c2 = (c * c).astype(f32)
    a = ((((_P7 * c2 + _P5) * c2 + _P3) * c2 + _P1) * c).astype(f32)
    a = np.where(big, a, f32(90.0) - a).astype(f32)
    a = np.where(x < 0, f32(180.0) - a, a).astype(f32)
    a = np.where(y < 0, f32(360.0) - a, a).astype(f32)
    return a


def moments(framed, cx, cy):
    """m_10, m_01 of the circular patch centred at the level pixel (cx, cy)."""
    m10 = m01 = 0
    for v in range(-HALF_PATCH_SIZE, HALF_PATCH_SIZE + 1):
        d = UMAX[abs(v)]
        row = framed[cy + v + EDGE_THRESHOLD, cx - d + EDGE_THRESHOLD:cx + d + 1 + EDGE_THRESHOLD].astype(np.int64)
        m10 += int((np.arange(-d, d + 1) * row).sum())
        m01 += v * int(row.sum())
    return m10, m01


def ic_angle(framed, xy):
    """Angles of key points xy (n x 2 float32, level pixels) on the unblurred framed level."""
    c = cv_round(np.asarray(xy, f32))
    m = np.array([moments(framed, int(x), int(y)) for x, y in c], np.int64).reshape(-1, 2)
    return fast_atan2(m[:, 1].astype(f32), m[:, 0].astype(f32))


# ---- descriptor ----------------------------------------------------------------------------------------------------------------------
FRAGILE = 0.5 - 1e-4


def rotated_pattern(pattern, angle):
    """Row and column offsets of every pattern point for every angle (n x 512 ints each) and which samples are fragile."""
    ang = (np.asarray(angle, f32) * f32(np.pi / np.float64(f32(180.0)))).astype(f32)
    a = np.cos(ang.astype(np.float64)).astype(f32)[:, None]
    b = np.sin(ang.astype(np.float64)).astype(f32)[:, None]
    px, py = pattern[:, 0].astype(f32)[None, :], pattern[:, 1].astype(f32)[None, :]
    vr = ((px * b).astype(f32) + (py * a).astype(f32)).astype(f32)
    vc = ((px * a).astype(f32) - (py * b).astype(f32)).astype(f32)
    fragile = (np.abs(vr - np.rint(vr)) > FRAGILE) | (np.abs(vc - np.rint(vc)) > FRAGILE)
    return cv_round(vr), cv_round(vc), fragile


def describe_level(framed, blurred, pattern, xy):
    """angle (n float32), descriptors (n x 32 uint8), fragile bits (n x 32 uint8 masks) of key points xy of one level."""
    xy = np.asarray(xy, f32).reshape(-1, 2)
    angle = ic_angle(framed, xy)
    c = cv_round(xy)
    r, col, frag = rotated_pattern(np.asarray(pattern).reshape(512, 2), angle)
    s = blurred[c[:, 1:2] + r + BLUR_MARGIN, c[:, 0:1] + col + BLUR_MARGIN].astype(np.int64)   # n x 512
    bits = (s[:, 0::2] < s[:, 1::2]).astype(np.uint8)                                           # n x 256, bit 8 i + k
    fbits = (frag[:, 0::2] | frag[:, 1::2]).astype(np.uint8)
    return angle, np.packbits(bits, axis=1, bitorder="little"), np.packbits(fbits, axis=1, bitorder="little")


def describe(pyr, pattern, level, xy):
    level = np.asarray(level, np.int64).reshape(-1)
    xy = np.asarray(xy, f32).reshape(-1, 2)
    angle, desc, frag = np.zeros(len(level), f32), np.zeros((len(level), 32), np.uint8), np.zeros((len(level), 32), np.uint8)
    for l in np.unique(level):
        m = level == l
        angle[m], desc[m], frag[m] = describe_level(pyr[l][1], pyr[l][2], pattern, xy[m])
    return angle, desc, frag


def extract(image, pattern, distribute, levels=8, scale_factor=1.2, ini_th=20, min_th=7, n_features=1000, pyr=None, cand=None):
    """The whole of operator() with the caller's distribute(level, candidates, n_wanted) -> indices; arrays ordered by level.  pyr and
    cand: the pyramid and the candidates of this image when the caller has them already."""
    pyr = pyr or pyramid(image, levels, scale_factor)
    cand = cand or detect(image, levels, scale_factor, ini_th, min_th, pyr)
    wanted = features_per_level(n_features, levels, scale_factor)
    sf, _ = scale_table(levels, scale_factor)
    lv, xy, resp = [], [], []
    for l in range(levels):
        sel = cand[l][np.asarray(distribute(l, cand[l], wanted[l]), np.int64).reshape(-1)]
        lv.append(np.full(len(sel), l, np.int32))
        xy.append(sel[:, :2].astype(f32))
        resp.append(sel[:, 2].astype(f32))
    lv, xy, resp = np.concatenate(lv), np.concatenate(xy).reshape(-1, 2), np.concatenate(resp)
    angle, desc, frag = describe(pyr, pattern, lv, xy)
    s = sf[lv]
    pt = np.where((lv > 0)[:, None], xy * s[:, None], xy).astype(f32)
    size = (f32(PATCH_SIZE) * s).astype(np.int32).astype(f32)
    return dict(pt=pt, octave=lv, size=size, angle=angle, response=resp, desc=desc, fragile=frag)
