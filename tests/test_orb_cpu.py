"""The restatement of the ORB front end (tests/orb_ref.py) against independent formulations, and the argument checks of the new entry
points on a host-only context.  The OpenCV steps are readings (include/defslam_hip.h) that no OpenCV build was available to verify; each is
pinned here by a brute-force definition or a float computation.  Measured on this file's inputs: resize against float bilinear 0.77 grey
levels (bound 1), blur against the float Gaussian 1.88 (recorded, not bounded), angle against arctan2 0.0096 degrees (bound 0.3),
fragile bits at most 0.12 % of a case's bits (bound 1 %)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import orb_ref as R
import orb_scenes as S
from conftest import ROOT


# ---- FAST ----------------------------------------------------------------------------------------------------------------------------
def brute_corner(img, x, y, t):
    """The definition: some arc of 9 contiguous circle pixels is all brighter than I(p) + t or all darker than I(p) - t."""
    v = int(img[y, x])
    ring = [int(img[y + dy, x + dx]) for dx, dy in R.CIRCLE]
    for k in range(16):
        arc = [ring[(k + i) % 16] for i in range(9)]
        if all(a > v + t for a in arc) or all(a < v - t for a in arc):
            return True
    return False


def brute_response(img, x, y):
    """The largest t at which p is still a corner, -1 if it is none at t = 0."""
    t = -1
    while t < 255 and brute_corner(img, x, y, t + 1):
        t += 1
    return t


def brute_cell(sub, th):
    """cv::FAST with suppression on one sub-image, by loops: (x, y, response) in raster order."""
    h, w = sub.shape
    resp = np.zeros((h, w), np.int64)
    for y in range(3, h - 3):
        for x in range(3, w - 3):
            if brute_corner(sub, x, y, th):
                resp[y, x] = brute_response(sub, x, y)
    out = []
    for y in range(3, h - 3):
        for x in range(3, w - 3):
            if brute_corner(sub, x, y, th) and all(resp[y, x] > resp[y + dy, x + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy):
                out.append((x, y, resp[y, x]))
    return out


def brute_level(level, ini_th, min_th):
    out = []
    for (i, j, x0, y0, x1, y1) in R.cells(level.shape[1], level.shape[0])[0]:
        sub = level[y0:y1, x0:x1]
        found = brute_cell(sub, ini_th) or brute_cell(sub, min_th)
        out += [(x + x0, y + y0, r) for x, y, r in found]
    return np.array(out, np.int32).reshape(-1, 3)


def test_fast_score_on_patches_equals_the_arc_definition():
    rng = np.random.default_rng(5)
    n_corner = 0
    for trial in range(400):
        if trial % 2:
            p = rng.integers(0, 256, (7, 7))
        else:   # a ring with one arc of random length pushed to one side of the centre
            p = rng.integers(90, 111, (7, 7))
            k0, length, delta = rng.integers(16), rng.integers(6, 14), int(rng.integers(5, 120)) * (1 if rng.integers(2) else -1)
            for i in range(length):
                dx, dy = R.CIRCLE[(k0 + i) % 16]
                p[3 + dy, 3 + dx] = np.clip(p[3 + dy, 3 + dx] + delta, 0, 255)
        p = p.astype(np.uint8)
        M = int(R.fast_m(p)[0, 0])
        r = brute_response(p, 3, 3)
        assert (r == M - 1) if M > 0 else (r == -1), (trial, M, r)
        for t in (0, 7, 20, 100):
            assert brute_corner(p, 3, 3, t) == (M > t)
        n_corner += M > 7
    assert n_corner >= 50


def test_detection_on_a_level_equals_the_loops_per_cell():
    level = S.image("shapes", 97, 71, seed=3)
    want = brute_level(level, S.INI_TH, S.MIN_TH)
    got, retried = R.detect_level(level, S.INI_TH, S.MIN_TH)
    per_cell, _ = R.detect_level(level, S.INI_TH, S.MIN_TH, per_cell=True)
    assert len(want) >= 5 and got.tolist() == want.tolist() and per_cell.tolist() == want.tolist()
    faint = S.image("faint", 97, 71, seed=3)
    assert brute_level(faint, S.INI_TH, S.MIN_TH).tolist() == R.detect_level(faint, S.INI_TH, S.MIN_TH)[0].tolist()


def test_faint_images_are_found_by_the_low_threshold_alone():
    for case in S.CASES:
        ref = S.reference(case, "faint")
        for (level, _, _), cand in zip(ref["pyr"], ref["cand"]):
            assert len(R.detect_level(level, S.INI_TH, S.INI_TH)[0]) == 0          # nothing at ini_th in any cell
            assert len(cand) > 0 and cand[:, 2].max() < S.INI_TH
        assert all(len(c) == 0 for c in S.reference(case, "flat")["cand"])


def test_suppression_stops_at_cell_boundaries():
    """92 wide: two cell columns whose detection regions are [19, 49) and [49, 79).  A bright bar of two pixels has two equal corners side
    by side: inside one region neither survives the strict comparison, across the boundary both do, as in the reference."""
    img = np.full((93, 92), 60, np.uint8)
    img[30, 48:50] = 200      # across the boundary
    img[60, 30:32] = 200      # inside the first cell
    run, skipped, (nCols, nRows, wCell, hCell) = R.cells(92, 93)
    assert (nCols, wCell) == (2, 30) and [c[2] + 3 for c in run[:2]] == [19, 49]
    cand = R.detect_level(img, S.INI_TH, S.MIN_TH)[0].tolist()
    assert [48, 30, 139] in cand and [49, 30, 139] in cand
    assert not any(c[1] == 60 for c in cand)
    assert cand == brute_level(img, S.INI_TH, S.MIN_TH).tolist()


def test_cell_arithmetic_and_skipped_cells():
    expect = {62: (1, 30), 91: (1, 59), 92: (2, 30), 123: (3, 31), 813: (26, 31)}
    for w, (nCols, wCell) in expect.items():
        run, skipped, (nc, nr, wc, hc) = R.cells(w, 62)
        assert (nc, wc) == (nCols, wCell) and nr == 1
        assert max(c[4] - c[2] for c in run) <= 65
        if w == 91:
            assert run[0][4] - run[0][2] == 59
        if w == 813:          # the last column: iniX = 791 = maxBX - 6
            assert skipped == [(0, 25)] and len(run) == 25
        else:
            assert not skipped
        # the detection regions tile the columns without overlap
        edges = [(c[2] + 3, c[4] - 3) for c in run]
        assert all(a[1] == b[0] for a, b in zip(edges, edges[1:]))
    run, skipped, (nc, nr, wc, hc) = R.cells(94, 903)
    assert (nr, hc) == (29, 31) and skipped == [(28, 0), (28, 1)] and len(run) == 56      # iniY = 884 = maxBY - 3
    # the cases of the GPU tests reach both skip branches
    assert R.cells(*S.CASES["skipped_column"][:2])[1] and R.cells(*S.CASES["skipped_row"][:2])[1]


# ---- pyramid -------------------------------------------------------------------------------------------------------------------------
def test_level_sizes_follow_the_float_scale_table():
    assert R.level_sizes(640, 480, 8, 1.2) == [(640, 480), (533, 400), (444, 333), (370, 278), (309, 231), (257, 193), (214, 161), (179, 134)]


def test_resize_is_within_one_grey_level_of_float_bilinear():
    img = S.image("noise", 97, 71)
    worst = 0.0
    for dw, dh in ((81, 59), (80, 60), (62, 62), (97, 71), (49, 36)):
        d = np.abs(R.resize(img, dw, dh).astype(np.float64) - R.resize_float(img, dw, dh)).max()
        worst = max(worst, d)
    print("resize against float bilinear:", worst)
    assert worst <= 1.0
    assert R.resize(img, 97, 71).tobytes() == img.tobytes()


def test_blur_equals_the_49_tap_integer_sum():
    img = S.image("noise", 70, 64)
    fr = R.frame(img)
    got = R.blur_plane(fr)
    assert got.shape == (70, 76)
    F = fr.astype(np.int64)
    q2 = np.outer(R.BLUR_Q, R.BLUR_Q)
    assert q2.sum() == 257 * 257
    want = np.zeros(got.shape, np.int64)
    for y in range(got.shape[0]):
        for x in range(got.shape[1]):
            want[y, x] = min(255, (int((q2 * F[y + 13:y + 20, x + 13:x + 20]).sum()) + 32768) >> 16)
    assert got.tolist() == want.tolist()
    # the weights: cvRound(k * 256) of the normalised Gaussian of sigma 2; the deviation from the float Gaussian is recorded, not bounded
    k = np.exp(-(np.arange(-3, 4) ** 2) / 8.0)
    k /= k.sum()
    assert np.rint(k * 256).astype(int).tolist() == R.BLUR_Q.tolist()
    flt = np.zeros(got.shape)
    k2 = np.outer(k, k)
    for y in range(got.shape[0]):
        for x in range(got.shape[1]):
            flt[y, x] = (k2 * F[y + 13:y + 20, x + 13:x + 20]).sum()
    print("blur against the float Gaussian:", np.abs(got - flt).max())
    # the frame is BORDER_REFLECT_101 of the level itself
    assert fr[19:-19, 19:-19].tobytes() == img.tobytes() and fr[0, 19:-19].tolist() == img[19].tolist() and fr[19:-19, -1].tolist() == img[:, -20].tolist()


# ---- angle and descriptor ------------------------------------------------------------------------------------------------------------
def test_umax_and_the_angle_polynomial():
    assert R.UMAX == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
    rng = np.random.default_rng(11)
    m = rng.integers(-200000, 200001, (200000, 2))
    m[:8] = [[0, 0], [1, 0], [0, 1], [-1, 0], [0, -1], [5, 5], [-5, 5], [5, -5]]
    got = R.fast_atan2(m[:, 1].astype(np.float32), m[:, 0].astype(np.float32)).astype(np.float64)
    want = np.degrees(np.arctan2(m[:, 1], m[:, 0])) % 360.0
    err = np.abs(got - want)
    err = np.minimum(err, 360.0 - err)
    print("angle against arctan2:", err.max())
    assert err.max() <= 0.3
    assert got[0] == 0.0 and got.min() >= 0.0 and got.max() <= 360.0


def test_moments_are_those_of_the_reference_loop():
    ref = S.reference("one_cell", "noise")
    fr = ref["pyr"][0][1]
    img = ref["image"].astype(np.int64)
    for cx, cy in ((16, 16), (45, 30), (31, 45)):
        m01 = m10 = 0
        for u in range(-15, 16):
            m10 += u * img[cy, cx + u]
        for v in range(1, 16):
            v_sum = 0
            for u in range(-R.UMAX[v], R.UMAX[v] + 1):
                plus, minus = img[cy + v, cx + u], img[cy - v, cx + u]
                v_sum += plus - minus
                m10 += u * (plus + minus)
            m01 += v * v_sum
        assert R.moments(fr, cx, cy) == (m10, m01)


def test_descriptor_equals_the_scalar_loop():
    lv, xy, angle, desc, frag = S.described("four_cells", "noise")
    _, fr, bl = S.reference("four_cells", "noise")["pyr"][0]
    pat = S.pattern(corners=True)
    for i in (0, 150, len(lv) - 1):
        ang = np.float32(angle[i]) * np.float32(np.pi / 180.0)
        a, b = np.float32(np.cos(np.float64(ang))), np.float32(np.sin(np.float64(ang)))
        cx, cy = int(np.rint(xy[i, 0])), int(np.rint(xy[i, 1]))

        def value(idx):
            px, py = np.float32(pat[idx, 0]), np.float32(pat[idx, 1])
            r = int(np.rint(np.float32(np.float32(px * b) + np.float32(py * a))))
            c = int(np.rint(np.float32(np.float32(px * a) - np.float32(py * b))))
            return int(bl[cy + r + 3, cx + c + 3])

        for byte in range(32):
            val = 0
            for k in range(8):
                val |= (value(16 * byte + 2 * k) < value(16 * byte + 2 * k + 1)) << k
            assert val == desc[i, byte], (i, byte)


def test_fragile_bits_stay_below_one_percent_in_every_device_case():
    """The condition that keeps the mask of the device tests from hiding a failure."""
    worst = 0.0
    for case in S.CASES:
        for kind in ("shapes", "noise"):
            lv, xy, angle, desc, frag = S.described(case, kind)
            assert len(lv) >= 100
            share = float(np.unpackbits(frag).mean())
            worst = max(worst, share)
            assert share <= 0.01, (case, kind, share)
    print("largest fragile-bit share:", worst)


# ---- the header's refusals on a host-only context ------------------------------------------------------------------------------------
def test_new_entry_points_name_no_context_type_in_their_parameters():
    header = open(os.path.join(ROOT, "include", "defslam_hip.h")).read()
    protos = dict(re.findall(r"\b(dsh_orb_[a-z_]+)\s*\(([^)]*)\)", header))
    assert sorted(protos) == ["dsh_orb_create", "dsh_orb_describe", "dsh_orb_destroy", "dsh_orb_detect", "dsh_orb_get_plane", "dsh_orb_level_sizes"]
    assert not any(re.search(r"\b(dsh_ctx|dsh_diffdb|dsh_kfdb|dsh_comm)\b", p) for p in protos.values())
    assert "not verified against an opencv build" in " ".join(header.lower().split())


def test_entry_points_refuse_malformed_arguments_and_a_host_only_context(host_ctx):
    from defslam_amd import _lib
    L, h = host_ctx._L, host_ctx._h
    ARG, NODEV = _lib.DSH_ERR_ARG, 4
    pat = np.ascontiguousarray(S.pattern())

    def create(**kw):
        a = dict(ctx=h, width=100, height=80, levels=2, scale_factor=1.2, ini_th_fast=20, min_th_fast=7, capacity=64,
                 pattern=pat.ctypes.data_as(_lib.c_i32_p))
        a.update(kw)
        cfg = _lib.OrbConfigC(*[a[n] for n, _ in _lib.OrbConfigC._fields_])
        out = C.c_void_p()
        rc = L.dsh_orb_create(C.byref(cfg), C.byref(out))
        return rc, out, L.dsh_last_error(h).decode()

    far = pat.copy()
    far[7] = (14, 13)                                                   # 365 > 342
    edge = pat.copy()
    edge[7] = (18, 4)                                                   # 340: allowed
    for kw, word in ((dict(pattern=None), "pattern"), (dict(levels=0), "levels"), (dict(levels=33), "levels"), (dict(scale_factor=1.0), "scale_factor"),
                     (dict(min_th_fast=0), "thresholds"), (dict(min_th_fast=21), "thresholds"), (dict(ini_th_fast=256), "thresholds"),
                     (dict(capacity=0), "capacity"), (dict(width=61), "62"), (dict(levels=3), "level 2"), (dict(height=73, levels=2), "level 1"),
                     (dict(pattern=far.ctypes.data_as(_lib.c_i32_p)), "pattern point 7")):
        rc, out, msg = create(**kw)
        assert rc == ARG and word in msg and not out.value, (kw, rc, msg)
    assert L.dsh_orb_create(None, None) == ARG
    rc, orb, msg = create(pattern=edge.ctypes.data_as(_lib.c_i32_p))
    assert rc == _lib.DSH_OK and orb.value, msg                         # the create is host logic: it works without a device
    try:
        wh, sf = np.zeros((2, 2), np.int32), np.zeros(2, np.float32)
        assert L.dsh_orb_level_sizes(orb, wh.ctypes.data_as(_lib.c_i32_p), sf.ctypes.data_as(_lib.c_float_p)) == _lib.DSH_OK
        assert [tuple(r) for r in wh.tolist()] == R.level_sizes(100, 80, 2, 1.2) and sf.tobytes() == R.scale_table(2, 1.2)[0].tobytes()
        assert L.dsh_orb_level_sizes(orb, None, None) == ARG

        img = np.zeros((80, 100), np.uint8)
        counts, cand = np.zeros(2, np.int32), np.zeros((2, 64, 3), np.int32)
        p_img, p_counts, p_cand = img.ctypes.data_as(_lib.c_u8_p), counts.ctypes.data_as(_lib.c_i32_p), cand.ctypes.data_as(_lib.c_i32_p)

        def status(rc, code, word):
            msg = L.dsh_last_error(h).decode()
            assert rc == code and word in msg, (rc, msg)

        status(L.dsh_orb_detect(orb, None, 100, p_counts, p_cand), ARG, "NULL")
        status(L.dsh_orb_detect(orb, p_img, 99, p_counts, p_cand), ARG, "row_stride")
        status(L.dsh_orb_detect(orb, p_img, 100, p_counts, p_cand), NODEV, "host-only")

        lv, xy = np.array([0, 1], np.int32), np.array([[16, 16], [66, 50]], np.float32)       # level 1 is 83 x 67
        angle, desc = np.zeros(2, np.float32), np.zeros((2, 32), np.uint8)

        def describe(lv, xy, n=2):
            return L.dsh_orb_describe(orb, n, lv.ctypes.data_as(_lib.c_i32_p), xy.ctypes.data_as(_lib.c_float_p), angle.ctypes.data_as(_lib.c_float_p),
                                      desc.ctypes.data_as(_lib.c_u8_p))

        status(describe(lv, xy), NODEV, "host-only")
        status(describe(np.array([0, 2], np.int32), xy), ARG, "key point 1 has a level")
        status(describe(lv, np.array([[15.4, 16], [66, 50]], np.float32)), ARG, "key point 0 lies less than 16")
        status(describe(lv, np.array([[16, 16], [66.6, 50]], np.float32)), ARG, "key point 1 lies less than 16")
        status(describe(lv, np.array([[16, 16], [66, np.nan]], np.float32)), ARG, "key point 1")
        status(describe(lv, xy, n=-1), ARG, "N outside")
        status(L.dsh_orb_describe(orb, 2, None, None, None, None), ARG, "NULL")

        out = np.zeros((118, 138), np.uint8)
        status(L.dsh_orb_get_plane(orb, 2, 0, out.ctypes.data_as(_lib.c_u8_p)), ARG, "level")
        status(L.dsh_orb_get_plane(orb, 0, 0, None), ARG, "NULL")
        status(L.dsh_orb_get_plane(orb, 0, 0, out.ctypes.data_as(_lib.c_u8_p)), NODEV, "host-only")
    finally:
        assert L.dsh_orb_destroy(orb) == _lib.DSH_OK
    assert L.dsh_orb_destroy(None) == ARG


def test_an_extractor_outlives_its_context():
    from defslam_amd import _lib, sft
    ctx = sft.Context(-1)
    pat = np.ascontiguousarray(S.pattern())
    cfg = _lib.OrbConfigC(ctx._h, 100, 80, 1, 1.2, 20, 7, 64, pat.ctypes.data_as(_lib.c_i32_p))
    orb = C.c_void_p()
    assert ctx._L.dsh_orb_create(C.byref(cfg), C.byref(orb)) == _lib.DSH_OK
    L = ctx._L
    ctx.close()
    wh, sf = np.zeros(2, np.int32), np.zeros(1, np.float32)
    assert L.dsh_orb_level_sizes(orb, wh.ctypes.data_as(_lib.c_i32_p), sf.ctypes.data_as(_lib.c_float_p)) == _lib.DSH_ERR_ARG
    assert L.dsh_orb_detect(orb, None, 0, None, None) == _lib.DSH_ERR_ARG
    assert L.dsh_orb_destroy(orb) == _lib.DSH_OK


def test_features_per_level_match_the_binding():
    from defslam_amd import orb
    for n, levels, s in ((1000, 8, 1.2), (1500, 3, 1.2), (500, 1, 1.5), (2000, 8, 1.1)):
        assert orb.features_per_level(n, levels, s) == R.features_per_level(n, levels, s)
        assert sum(R.features_per_level(n, levels, s)) == n
