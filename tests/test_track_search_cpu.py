"""CPU tests of the tracking searches: the restatement (tests/track_search_ref.py) on hand-built scenes with known answers, and the
ABI's refusals (host-only context, bad arguments) without a GPU."""
import numpy as np
import pytest

import track_search_ref as R


K_ISO, BOUNDS_ISO = (500, 500, 320, 240), (0, 640, 0, 480)
# a dyadic anisotropic camera whose undistorted image area starts at negative coordinates: (X, Y, 1) with X, Y multiples of 1/1024 projects
# exactly to (512 X + 300.5, 256 Y + 140.25); columns are 720 / 64 = 11.25 px wide, rows 288 / 48 = 6 px high
K_DY, BOUNDS_DY = (512, 256, 300.5, 140.25), (-8, 712, -4, 284)


def hand_frame(kp, octave, state=None, desc=None, levels=8, K=K_ISO, bounds=BOUNDS_ISO):
    """Identity pose, 640 x 480, fx = fy = 500: a point (X, Y, 1) with dyadic X, Y projects exactly to (500 X + 320, 500 Y + 240).
    K, bounds: another pinhole (fx, fy, cx, cy) and image area (mnMinX, mnMaxX, mnMinY, mnMaxY)."""
    from defslam_amd import track
    kp = np.asarray(kp, np.float32).reshape(-1, 2)
    N = kp.shape[0]
    sf, logsf = track.orb_pyramid(levels)
    return track.TrackFrame(Tcw=np.eye(4, dtype=np.float32), K=np.array(K, np.float32), bounds=np.array(bounds, np.float32),
                            kp=kp, octave=np.asarray(octave, np.int32), desc=np.zeros((N, 32), np.uint8) if desc is None else desc,
                            scale_factors=sf, log_scale_factor=float(logsf), state=np.zeros(N, np.uint8) if state is None else np.asarray(state, np.uint8))


def desc_with_dist(d):
    """A descriptor at Hamming distance d from the all-zero one."""
    out = np.zeros(32, np.uint8)
    for b in range(d):
        out[b // 8] |= np.uint8(1 << (b % 8))
    return out


U, V = np.float32(382.5), np.float32(271.25)   # projection of (0.125, 0.0625, 1)
P0 = np.array([[0.125, 0.0625, 1.0]], np.float32)


def test_frame_conflict_is_resolved_in_query_order():
    """Two queries want key point 0 (distance 3); the first takes it, the second falls back to key point 1 (distance 10)."""
    tf = hand_frame([[U + 1, V], [U - 2, V]], [0, 0], desc=np.stack([desc_with_dist(3), desc_with_dist(10)]))
    fr = R.ref_frame(tf)
    xyz = np.repeat(P0, 2, 0)
    m, n, st = R.search_frame(fr, tf.state, xyz, [0, 0], np.zeros((2, 32), np.uint8), 20)
    assert m.tolist() == [0, 1] and n == 2 and st.tolist() == [1, 1]


def test_frame_drops_a_best_with_a_map_point_and_local_overwrites_it():
    """Key point 0 (state 2: a map point without observations) is the best of both searches: frame to frame drops the match
    (ORBmatcher.cc:1462), the local map overwrites the key point's map point."""
    tf = hand_frame([[U + 1, V], [U - 1, V]], [0, 0], state=[2, 0], desc=np.stack([desc_with_dist(2), desc_with_dist(9)]))
    fr = R.ref_frame(tf)
    m, n, _ = R.search_frame(fr, tf.state, P0, [0], np.zeros((1, 32), np.uint8), 20)
    assert m.tolist() == [-1] and n == 0
    nrm = np.array([[0.125, 0.0625, 1.0]], np.float32) / np.float32(np.linalg.norm([0.125, 0.0625, 1.0]))
    m, n, st, iv, lev, uv, vc = R.search_local(fr, tf.state, P0, nrm, [1.0], np.zeros((1, 32), np.uint8), None, 3)
    assert iv[0] and lev[0] == 0 and m.tolist() == [0] and n == 1 and st.tolist() == [1, 0]


@pytest.mark.parametrize("d1,d2,ok", [(4, 5, True), (5, 6, False), (8, 10, True), (0, 0, True), (75, 256, True), (76, 256, False)])
def test_local_ratio_test_on_its_boundary(d1, d2, ok):
    """bestDist > 0.8f * bestDist2 rejects only strictly: 4 vs 0.8f * 5 == 4.0f and 8 vs 0.8f * 10 == 8.0f pass; TH_HIGH = 75 is
    inclusive.  Both candidates on the predicted level (a second best on another level never rejects)."""
    kps = [[U + 1, V]] + ([[U - 1, V]] if d2 < 256 else [])
    descs = [desc_with_dist(d1)] + ([desc_with_dist(d2)] if d2 < 256 else [])
    tf = hand_frame(kps, [0] * len(kps), desc=np.stack(descs))
    fr = R.ref_frame(tf)
    nrm = P0 / np.float32(np.linalg.norm(P0))
    m, n, *_ = R.search_local(fr, tf.state, P0, nrm, [1.0], np.zeros((1, 32), np.uint8), None, 3)
    assert (m[0] == 0) == ok


def test_window_edge_is_strict():
    """|dx| == r is outside the window (Frame.cc:471 fabs(distx) < r); th = 20 at octave 0 gives r = 20 exactly."""
    tf = hand_frame([[U + 20, V], [U, V - 20], [U + 19.75, V - 19.75]], [0, 0, 0])
    fr = R.ref_frame(tf)
    assert fr.features_in_area(U, V, np.float32(20), -1, 1) == [2]
    m, n, _ = R.search_frame(fr, tf.state, P0, [0], np.zeros((1, 32), np.uint8), 20)
    assert m.tolist() == [2]


def test_octave_window_limits():
    """Frame to frame searches octaves [o - 1, o + 1]; the local map [level - 1, level]."""
    tf = hand_frame([[U + 1, V], [U + 2, V], [U + 3, V], [U + 4, V]], [0, 1, 3, 4])
    fr = R.ref_frame(tf)
    assert fr.features_in_area(U, V, np.float32(20), 1, 3) == [1, 2]
    assert fr.features_in_area(U, V, np.float32(20), 2, 3) == [2]


def test_no_distance_range_test_in_is_in_frustum():
    """A point 10 times beyond 1.2 * mfMaxDistance is still in view (DefSLAM's isInFrustum never uses the range); its level clamps
    to 0."""
    tf = hand_frame([[U, V]], [0])
    fr = R.ref_frame(tf)
    nrm = P0 / np.float32(np.linalg.norm(P0))
    r = R.is_in_frustum(fr, P0[0], nrm[0], np.float32(0.1))
    assert r is not None and r[2] == 0 and r[0] == U and r[1] == V


def test_grid_cell_edges_follow_pos_in_grid():
    """PosInGrid rounds half away from zero: x = 5.0 (cell width 10) is cell 1, x = 4.99 is cell 0; x = 635.0 is 63.5 -> 64,
    outside the grid, so the key point is in no cell (the reference never returns it)."""
    tf = hand_frame([[5.0, 100.0], [4.99, 100.0], [635.0, 100.0]], [0, 0, 0])
    fr = R.ref_frame(tf)
    assert 0 in fr.grid[1][10] and 1 in fr.grid[0][10]
    assert all(2 not in fr.grid[ix][iy] for ix in range(64) for iy in range(48))


def test_tie_goes_to_the_first_in_visiting_order():
    """Equal distances: the first in (column, row, index) order wins, not the lower index."""
    tf = hand_frame([[U + 10, V], [U - 10, V]], [0, 0], desc=np.stack([desc_with_dist(5), desc_with_dist(5)]))
    fr = R.ref_frame(tf)
    m, *_ = R.search_frame(fr, tf.state, P0, [0], np.zeros((1, 32), np.uint8), 20)
    assert m.tolist() == [1]   # key point 1 lies in a lower grid column


def test_host_only_context_has_no_device(host_ctx):
    from defslam_amd import sft, track
    tf = hand_frame([[U, V]], [0])
    with pytest.raises(sft.DshError, match="status 4"):
        track.SearchByProjectionFrame(host_ctx, tf, track.FrameQueries(xyz=P0, octave=[0], desc=np.zeros((1, 32), np.uint8)), 20)


@pytest.mark.parametrize("what", ["N", "octave", "state", "levels", "grid", "query_octave", "th", "mode"])
def test_bad_arguments_are_refused(host_ctx, what):
    import ctypes as C
    from defslam_amd import _lib, sft, track
    n_kp = 8193 if what == "N" else 1
    kp = np.tile(np.array([[U, V]], np.float32), (n_kp, 1))
    tf = hand_frame(kp, [0] * n_kp)
    if what == "octave":
        tf.octave = np.array([200], np.int32)
    if what == "state":
        tf.state = np.array([3], np.uint8)
    if what == "levels":
        tf.scale_factors = np.ones(33, np.float32)
    if what == "grid":
        tf.grid = (100, 100)
    items = [(tf, track.FrameQueries(xyz=P0, octave=[8 if what == "query_octave" else 0], desc=np.zeros((1, 32), np.uint8)), 0.0 if what == "th" else 20)]
    if what == "mode":
        keep = []
        p = _lib.TrackProblemC()
        p.frame = tf.c(keep)
        p.mode = 7
        p.th = 20.0
        rc = host_ctx._L.dsh_search_by_projection_batch(host_ctx._h, 1, C.byref(p))
        assert rc == 1
        return
    with pytest.raises(sft.DshError, match="status 1"):
        track.search_batch(host_ctx, items)


@pytest.mark.parametrize("bounds,inside", [((382.5, 640, 0, 480), True), ((0, 382.5, 0, 480), True), ((0, 640, 271.25, 480), True),
                                           ((0, 640, 0, 271.25), True), ((382.75, 640, 0, 480), False), ((0, 382.25, 0, 480), False),
                                           ((0, 640, 271.5, 480), False), ((0, 640, 0, 271.0), False)])
def test_image_bounds_are_inclusive(bounds, inside):
    """Frame.cc:360-363 / ORBmatcher.cc:1405-1408 reject only u < mnMinX, u > mnMaxX (v likewise): a projection on the bound is in."""
    from defslam_amd import track
    tf = hand_frame([[U, V]], [0])
    tf = track.TrackFrame(**{**tf.__dict__, "bounds": np.asarray(bounds, np.float32)})
    fr = R.ref_frame(tf)
    nrm = P0 / np.float32(np.linalg.norm(P0))
    assert (R.is_in_frustum(fr, P0[0], nrm[0], np.float32(1.0)) is not None) == inside


# ---- the same known answers at fx != fy with image bounds that start below zero (K_DY, BOUNDS_DY) ---------------------------------------
UD, VD = np.float32(364.5), np.float32(156.25)   # projection of P0 = (0.125, 0.0625, 1): 512 / 8 + 300.5, 256 / 16 + 140.25
# on the four bounds: (-8, -4) and (712, 284) are the projections of (-617 / 1024, -577 / 1024, 1) and (823 / 1024, 575 / 1024, 1)
P_MIN = np.array([[-617.0 / 1024, -577.0 / 1024, 1.0]], np.float32)
P_MAX = np.array([[823.0 / 1024, 575.0 / 1024, 1.0]], np.float32)
# in the image only with fx on x and fy on y: v = 256 / 2 + 140.25 = 268.25 (swapped 396.25 > 284) -- and the other way round: u = 812.5 > 712
# (swapped: 556.5, 204.25, inside)
P_ONLY_UNSWAPPED = np.array([[0.125, 0.5, 1.0]], np.float32)
P_ONLY_SWAPPED = np.array([[1.0, 0.125, 1.0]], np.float32)


def dyadic_frame(kp, octave, **kw):
    return hand_frame(kp, octave, K=K_DY, bounds=BOUNDS_DY, **kw)


def test_dyadic_camera_projects_with_fx_on_x_and_fy_on_y():
    """P0 lands on (364.5, 156.25), not on the swapped (332.5, 172.25); a point that only the right assignment of fx and fy puts into
    the image is in view and matched, one that only the swapped assignment would put there is not."""
    nrm = lambda P: P / np.float32(np.linalg.norm(P))
    zero = np.zeros((1, 32), np.uint8)
    tf = dyadic_frame([[UD, VD], [332.5, 172.25]], [0, 0])
    fr = R.ref_frame(tf)
    r = R.is_in_frustum(fr, P0[0], nrm(P0)[0], np.float32(1.0))
    assert r is not None and r[0] == UD and r[1] == VD
    m, n, _ = R.search_frame(fr, tf.state, P0, [0], zero, 3)           # r = 3 px: only the key point at the projection
    assert m.tolist() == [0]
    tf = dyadic_frame([[364.5, 268.25], [556.5, 204.25]], [0, 0])
    fr = R.ref_frame(tf)
    r = R.is_in_frustum(fr, P_ONLY_UNSWAPPED[0], nrm(P_ONLY_UNSWAPPED)[0], np.float32(1.0))
    assert r is not None and (r[0], r[1]) == (np.float32(364.5), np.float32(268.25))
    assert R.search_frame(fr, tf.state, P_ONLY_UNSWAPPED, [0], zero, 20)[0].tolist() == [0]
    assert R.is_in_frustum(fr, P_ONLY_SWAPPED[0], nrm(P_ONLY_SWAPPED)[0], np.float32(1.0)) is None
    assert R.search_frame(fr, tf.state, P_ONLY_SWAPPED, [0], zero, 20)[0].tolist() == [-1]


def test_dyadic_window_edge_is_strict():
    """|dx| == r is outside at fx != fy as well; the window is a square in pixels, not in normalised coordinates."""
    tf = dyadic_frame([[UD + 20, VD], [UD, VD - 20], [UD + 19.75, VD - 19.75]], [0, 0, 0])
    fr = R.ref_frame(tf)
    assert fr.features_in_area(UD, VD, np.float32(20), -1, 1) == [2]
    m, n, _ = R.search_frame(fr, tf.state, P0, [0], np.zeros((1, 32), np.uint8), 20)
    assert m.tolist() == [2]


DYADIC_BOUND_CASES = [(P_MIN, (-8, 712, -4, 284), True), (P_MIN, (-7.75, 712, -4, 284), False), (P_MIN, (-8, 712, -3.75, 284), False),
                      (P_MAX, (-8, 712, -4, 284), True), (P_MAX, (-8, 711.75, -4, 284), False), (P_MAX, (-8, 712, -4, 283.75), False)]


@pytest.mark.parametrize("P,bounds,inside", DYADIC_BOUND_CASES)
def test_dyadic_image_bounds_are_inclusive_at_negative_minima(P, bounds, inside):
    """A projection exactly on mnMinX = -8 / mnMinY = -4 (and on the maxima) is in; a quarter pixel beyond is out."""
    tf = hand_frame([[UD, VD]], [0], K=K_DY, bounds=bounds)
    fr = R.ref_frame(tf)
    nrm = P / np.float32(np.linalg.norm(P))
    assert (R.is_in_frustum(fr, P[0], nrm[0], np.float32(1.0)) is not None) == inside


def test_dyadic_grid_cells_around_a_negative_minimum_bound():
    """PosInGrid measures from mnMinX = -8, mnMinY = -4.  Rows are 6 px high: y = -1 is (y + 4) / 6 = 0.5 -> row 1 (half away from zero), y = -1.01
    row 0.  Key points left of the image: x = -9 is column round(-1 / 11.25) = 0 -- the reference keeps it, in column 0 --, x = -14 is column
    round(-6 / 11.25) = -1, in no cell.  Inside, x = -7 is column 0 and x = 4 column round(12 / 11.25) = 1."""
    tf = dyadic_frame([[100.0, -1.0], [100.0, -1.01], [-9.0, 50.0], [-14.0, 50.0], [-7.0, 50.0], [4.0, 50.0]], [0] * 6)
    fr = R.ref_frame(tf)
    col = round(108.0 / 11.25)
    assert 0 in fr.grid[col][1] and 1 in fr.grid[col][0]
    assert fr.grid[0][9] == [2, 4] and fr.grid[1][9] == [5]
    assert all(3 not in fr.grid[ix][iy] for ix in range(64) for iy in range(48))
    # the search finds the key points on both sides of the bound: the projection (-8, 50) of (-617 / 1024, -90.25 / 256, 1) is on mnMinX
    P = np.array([[-617.0 / 1024, -90.25 / 256, 1.0]], np.float32)
    assert fr.features_in_area(np.float32(-8), np.float32(50), np.float32(20), -1, 1) == [2, 4, 5]
    descs = np.stack([desc_with_dist(d) for d in (0, 0, 7, 1, 9, 20)])
    tf = dyadic_frame(tf.kp, tf.octave, desc=descs)
    m, n, _ = R.search_frame(R.ref_frame(tf), tf.state, P, [0], np.zeros((1, 32), np.uint8), 20)
    assert m.tolist() == [2]   # the key point outside the image wins (distance 7); the better one at x = -14 (distance 1) is in no cell
