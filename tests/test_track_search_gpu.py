"""GPU tests of the tracking searches (dsh_search_by_projection_*): bit-exact match indices (and the local map's in_view, level,
projection and viewCos) against the sequential restatement tests/track_search_ref.py."""
import numpy as np
import pytest

import track_search_ref as R
import operating_points as op
from test_track_search_cpu import (DYADIC_BOUND_CASES, K_DY, P0, P_ONLY_SWAPPED, P_ONLY_UNSWAPPED, U, UD, V, VD, desc_with_dist, dyadic_frame,
                                   hand_frame)

pytestmark = pytest.mark.gpu


def check_frame(ctx, tf, fq, th):
    from defslam_amd import track
    g = track.SearchByProjectionFrame(ctx, tf, fq, th)
    m, n, _ = R.search_frame(R.ref_frame(tf), tf.arrays()["state"], fq.xyz, fq.octave, fq.desc, th)
    np.testing.assert_array_equal(g.match, m)
    assert g.nmatches == n
    return g


def check_local(ctx, tf, lq, th=3):
    from defslam_amd import track
    g = track.SearchByProjectionLocal(ctx, tf, lq, th)
    m, n, _, iv, lev, uv, vc = R.search_local(R.ref_frame(tf), tf.arrays()["state"], lq.xyz, lq.normal, lq.max_distance, lq.desc, lq.skip, th)
    np.testing.assert_array_equal(g.in_view, iv)
    np.testing.assert_array_equal(g.level[iv], lev[iv])
    np.testing.assert_array_equal(g.uv[iv], uv[iv])
    np.testing.assert_array_equal(g.view_cos[iv], vc[iv])
    np.testing.assert_array_equal(g.match, m)
    assert g.nmatches == n
    return g


@pytest.mark.parametrize("seed,n_kp,n_q,state_mix", [(0, 1200, 400, False), (1, 1200, 400, True), (2, 2000, 1500, False), (3, 2000, 1500, True),
                                                     (4, 300, 60, True), (5, 8000, 1200, False)])
def test_frame_to_frame_matches_the_restatement(gpu_ctx, seed, n_kp, n_q, state_mix):
    from defslam_amd import synth
    sc = synth.make_track_scene(seed, n_kp=n_kp, n_frame_q=n_q, n_local_q=0, state_mix=state_mix, n_clusters=6 + seed)
    g20 = check_frame(gpu_ctx, sc["frame"], sc["fq"], 20)
    g25 = check_frame(gpu_ctx, sc["frame"], sc["fq"], 25)
    assert g20.nmatches > 0.3 * len(g20.match) and g25.nmatches > 0


@pytest.mark.parametrize("seed,n_kp,n_q,state_mix", [(0, 1200, 300, False), (1, 1200, 300, True), (2, 2000, 1500, True), (3, 2000, 1000, False),
                                                     (6, 500, 80, True)])
def test_local_map_matches_the_restatement(gpu_ctx, seed, n_kp, n_q, state_mix):
    from defslam_amd import synth
    sc = synth.make_track_scene(seed, n_kp=n_kp, n_frame_q=0, n_local_q=n_q, state_mix=state_mix, n_clusters=6 + seed)
    g3 = check_local(gpu_ctx, sc["frame"], sc["lq"], 3)
    g5 = check_local(gpu_ctx, sc["frame"], sc["lq"], 5)
    assert g3.nmatches > 0 and g5.nmatches > 0 and g3.in_view.sum() > 0.3 * len(g3.match)


def test_adversarial_conflicts_need_phase_b_rescans_and_still_match(gpu_ctx):
    """Clusters of near-identical key points wanted by many queries exhaust the stored keys: phase B walks windows again."""
    from defslam_amd import synth
    sc = synth.make_track_scene(11, n_kp=1500, n_frame_q=300, n_local_q=300, n_clusters=30)
    g = check_frame(gpu_ctx, sc["frame"], sc["fq"], 20)
    assert g.rescans > 0
    check_local(gpu_ctx, sc["frame"], sc["lq"], 3)


def test_hand_built_boundaries_on_the_device(gpu_ctx):
    """The CPU tests' known answers, on the device: conflict order, drop vs overwrite of a state-2 key point, window edge, ties."""
    from defslam_amd import track
    zero = np.zeros((2, 32), np.uint8)
    tf = hand_frame([[U + 1, V], [U - 2, V]], [0, 0], desc=np.stack([desc_with_dist(3), desc_with_dist(10)]))
    assert check_frame(gpu_ctx, tf, track.FrameQueries(np.repeat(P0, 2, 0), [0, 0], zero), 20).match.tolist() == [0, 1]
    tf = hand_frame([[U + 1, V], [U - 1, V]], [0, 0], state=[2, 0], desc=np.stack([desc_with_dist(2), desc_with_dist(9)]))
    assert check_frame(gpu_ctx, tf, track.FrameQueries(P0, [0], zero[:1]), 20).match.tolist() == [-1]
    nrm = P0 / np.float32(np.linalg.norm(P0))
    assert check_local(gpu_ctx, tf, track.LocalQueries(P0, nrm, np.array([1.0], np.float32), zero[:1]), 3).match.tolist() == [0]
    tf = hand_frame([[U + 20, V], [U, V - 20], [U + 19.75, V - 19.75]], [0, 0, 0])
    assert check_frame(gpu_ctx, tf, track.FrameQueries(P0, [0], zero[:1]), 20).match.tolist() == [2]
    tf = hand_frame([[U + 10, V], [U - 10, V]], [0, 0], desc=np.stack([desc_with_dist(5), desc_with_dist(5)]))
    assert check_frame(gpu_ctx, tf, track.FrameQueries(P0, [0], zero[:1]), 20).match.tolist() == [1]
    for d1, d2, ok in [(4, 5, True), (5, 6, False), (8, 10, True), (75, 256, True), (76, 256, False)]:
        kps = [[U + 1, V]] + ([[U - 1, V]] if d2 < 256 else [])
        descs = [desc_with_dist(d1)] + ([desc_with_dist(d2)] if d2 < 256 else [])
        tf = hand_frame(kps, [0] * len(kps), desc=np.stack(descs))
        g = check_local(gpu_ctx, tf, track.LocalQueries(P0, nrm, np.array([1.0], np.float32), zero[:1]), 3)
        assert (g.match[0] == 0) == ok
    # no distance-range test: far beyond 1.2 * mfMaxDistance, still in view at level 0
    tf = hand_frame([[U, V]], [0])
    g = check_local(gpu_ctx, tf, track.LocalQueries(P0, nrm, np.array([0.1], np.float32), zero[:1]), 3)
    assert g.in_view[0] and g.level[0] == 0


def test_motion_model_retries_with_a_wider_window(gpu_ctx):
    """30 points whose key points lie 22 px away: th = 20 (r = 20) finds none, th = 25 finds all (DefTracking.cc:363-369)."""
    from defslam_amd import track
    i = np.arange(30)
    X, Y = ((i % 6 - 3) / 8).astype(np.float32), ((i // 6 - 2) / 8).astype(np.float32)   # 62.5 px apart: one key point per window
    xyz = np.stack([X, Y, np.ones(30, np.float32)], 1)
    kp = np.stack([500 * X + 320 + 22, 500 * Y + 240], 1).astype(np.float32)
    tf = hand_frame(kp, np.zeros(30))
    qs = track.FrameQueries(xyz, np.zeros(30, np.int32), np.zeros((30, 32), np.uint8))
    r = track.motion_model_search(gpu_ctx, tf, qs)
    m, n, th, st = R.motion_model(tf, xyz, qs.octave, qs.desc)
    assert r.th == th == 25 and r.nmatches == n == 30 and r.ok
    np.testing.assert_array_equal(r.match, m)
    np.testing.assert_array_equal(r.state, st)
    few = track.motion_model_search(gpu_ctx, tf, track.FrameQueries(xyz[:12], qs.octave[:12], qs.desc[:12]))
    assert few.th == 25 and few.nmatches == 12 and not few.ok


def test_batch_equals_single_calls(gpu_ctx):
    """Frames of different sizes and both modes in one batch give what each gives alone, bit for bit; Q = 0 and N = 0 included."""
    from defslam_amd import track, synth
    items = []
    for s, (n_kp, nq) in enumerate([(1200, 400), (300, 50), (2000, 1500), (700, 0), (0, 40)]):
        sc = synth.make_track_scene(20 + s, n_kp=max(n_kp, 1), n_frame_q=nq, n_local_q=max(nq // 2, 0), state_mix=s % 2 == 1)
        f = sc["frame"]
        if n_kp == 0:
            f = track.TrackFrame(**{**f.__dict__, "kp": np.zeros((0, 2), np.float32), "octave": np.zeros(0, np.int32),
                                    "desc": np.zeros((0, 32), np.uint8), "state": np.zeros(0, np.uint8)})
        items.append((f, sc["fq"], 20))
        items.append((f, sc["lq"], 3))
    batch = track.search_batch(gpu_ctx, items)
    for (f, qs, th), b in zip(items, batch):
        one = track.search_batch(gpu_ctx, [(f, qs, th)])[0]
        np.testing.assert_array_equal(b.match, one.match)
        assert b.nmatches == one.nmatches
        if isinstance(qs, track.LocalQueries):
            np.testing.assert_array_equal(b.in_view, one.in_view)
            np.testing.assert_array_equal(b.level, one.level)
            check_local(gpu_ctx, f, qs, th)
        else:
            check_frame(gpu_ctx, f, qs, th)
    assert track.search_batch(gpu_ctx, []) == []


def test_empty_queries_and_empty_frame(gpu_ctx):
    from defslam_amd import track
    tf = hand_frame([[U, V]], [0])
    r = track.SearchByProjectionFrame(gpu_ctx, tf, track.FrameQueries(np.zeros((0, 3), np.float32), np.zeros(0, np.int32), np.zeros((0, 32), np.uint8)), 20)
    assert r.match.shape == (0,) and r.nmatches == 0
    empty = hand_frame(np.zeros((0, 2), np.float32), np.zeros(0))
    r = check_frame(gpu_ctx, empty, track.FrameQueries(P0, [0], np.zeros((1, 32), np.uint8)), 20)
    assert r.match.tolist() == [-1]


def test_chain_sft_search_sft(gpu_ctx, oracle_mod):
    """SfT on frame t -> search on frame t+1 from dsh_sft_result.mappoint_xyz -> SfT on frame t+1.  The device chain (device search,
    device SfT) against the reference chain (the restatement's matches, the CPU oracle's SfT): equal matches, equal LM iterations and
    inliers, vertices to 1e-7."""
    from defslam_amd import sft, synth, track
    tmpl, fr = synth.make_problem("smoke", 1)
    gpu_ctx.template_build(tmpl.xyz0, tmpl.facets)
    f = sft.frame_from_synth(fr)
    sft.DefPoseOptimization(gpu_ctx, f, synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    keep = ~f.mvbOutlier
    mp = f.mappoints[keep]
    sc = synth.make_track_scene(7, n_kp=1200, n_frame_q=0, n_local_q=0, mappoint_xyz=mp, Tcw=f.Tcw)
    # the queries are the inlier map points in observation order; the current frame starts at the last pose (DefTracking.cc:350)
    tf = track.TrackFrame(**{**sc["frame"].__dict__, "Tcw": f.Tcw, "Ow": None})
    rng = np.random.default_rng(3)
    pdesc = np.zeros((mp.shape[0], 32), np.uint8)
    kpd = sc["frame"].desc
    for i in range(mp.shape[0]):   # the point's descriptor: its key point's, a few bits off
        j = sc["kp_of_point"][i]
        pdesc[i] = kpd[j] if j >= 0 else rng.integers(0, 256, 32, dtype=np.uint8)
    koct = np.where(sc["kp_of_point"] >= 0, tf.octave[np.maximum(sc["kp_of_point"], 0)], 0).astype(np.int32)   # LastFrame.mvKeys[i].octave
    qs = track.FrameQueries(mp, koct, pdesc)
    r = track.motion_model_search(gpu_ctx, tf, qs)
    m, n, th, _ = R.motion_model(tf, mp, qs.octave, qs.desc)
    np.testing.assert_array_equal(r.match, m)
    assert r.ok and r.nmatches == n
    sel = np.nonzero(r.match >= 0)[0]
    src = np.nonzero(keep)[0][sel]

    def frame_t1(match_sel):
        f1 = sft.frame_from_synth(fr)
        f1.Tcw = f.Tcw.copy()
        f1.nodes_xyz = f.nodes_xyz.copy()
        f1.obs_nodes, f1.obs_bary = fr.obs_nodes[src], fr.obs_bary[src]
        f1.obs_uv = tf.kp[match_sel].astype(np.float64)
        f1.obs_invsig2 = fr.obs_invsig2[src]
        return f1

    a, b = frame_t1(r.match[sel]), frame_t1(m[sel])
    ia = sft.DefPoseOptimization(gpu_ctx, a, synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    tc = oracle_mod.template_build(tmpl.xyz0, tmpl.facets)
    ro = oracle_mod.sft_solve(tc, b.Tcw, b.K, b.N, b.obs_nodes, b.obs_bary, b.obs_uv, b.obs_invsig2, b.nodes_xyz, synth.REG_LAP, synth.REG_INEX,
                              synth.REG_TEMP)
    assert a.iters == ro.iters and ia == ro.ret, (a.iters, ro.iters, ia, ro.ret)
    assert float(np.abs(a.nodes_xyz - ro.xyz).max()) < 1e-7


def _with_bounds(tf, bounds):
    from defslam_amd import track
    return track.TrackFrame(**{**tf.__dict__, "bounds": np.asarray(bounds, np.float32)})


def test_image_bounds_are_inclusive_on_the_device(gpu_ctx):
    """u == mnMinX / mnMaxX and v == mnMinY / mnMaxY are inside (Frame.cc:360-363, ORBmatcher.cc:1405-1408 reject only u < min and
    u > max); a quarter pixel beyond is outside.  Both searches, projection (382.5, 271.25) exact."""
    from defslam_amd import track
    zero = np.zeros((1, 32), np.uint8)
    nrm = P0 / np.float32(np.linalg.norm(P0))
    lq = track.LocalQueries(P0, nrm, np.array([1.0], np.float32), zero)
    fq = track.FrameQueries(P0, [0], zero)
    for bounds, inside in [([U, 640, 0, 480], True), ([0, U, 0, 480], True), ([0, 640, V, 480], True), ([0, 640, 0, V], True),
                           ([U + 0.25, 640, 0, 480], False), ([0, U - 0.25, 0, 480], False), ([0, 640, V + 0.25, 480], False), ([0, 640, 0, V - 0.25], False)]:
        # the key point inside the image towards its centre (4 px from a max bound: closer ones round to the column / row past the grid)
        kx = U + (0.125 if bounds[0] == U else -4.0 if bounds[1] in (U, U - 0.25) else 0.0)
        ky = V + (0.125 if bounds[2] == V else -4.0 if bounds[3] in (V, V - 0.25) else 0.0)
        tf = _with_bounds(hand_frame([[kx, ky]], [0]), bounds)
        assert (check_frame(gpu_ctx, tf, fq, 20).match[0] == 0) == inside, bounds
        g = check_local(gpu_ctx, tf, lq, 3)
        assert bool(g.in_view[0]) == inside and (g.match[0] == 0) == inside, bounds


def test_grid_cell_edges_on_the_device(gpu_ctx):
    """PosInGrid on the device: x = 5.0 rounds to column 1, x = 4.99 to column 0, so with equal distances key point 1 (x = 4.99) is
    visited first and wins although its index is higher; a key point at x = 635.0 (column 63.5 -> 64) is in no cell and never found."""
    from defslam_amd import track
    zero = np.zeros((1, 32), np.uint8)
    X = np.float32((5.0 - 320.0) / 500.0)
    q = np.array([[X, 0.0625, 1.0]], np.float32)
    tf = hand_frame([[5.0, V], [4.99, V]], [0, 0], desc=np.stack([desc_with_dist(3), desc_with_dist(3)]))
    assert check_frame(gpu_ctx, tf, track.FrameQueries(q, [0], zero), 20).match.tolist() == [1]
    X2 = np.float32((634.0 - 320.0) / 500.0)
    tf = hand_frame([[635.0, V], [634.0 - 15.0, V]], [0, 0], desc=np.stack([desc_with_dist(0), desc_with_dist(40)]))
    assert check_frame(gpu_ctx, tf, track.FrameQueries(np.array([[X2, 0.0625, 1.0]], np.float32), [0], zero), 20).match.tolist() == [1]


def test_octave_windows_on_the_device(gpu_ctx):
    """Frame to frame searches octaves [o - 1, o + 1], the local map [level - 1, level]: better key points one octave outside are not
    candidates."""
    from defslam_amd import track
    zero = np.zeros((1, 32), np.uint8)
    descs = np.stack([desc_with_dist(d) for d in (1, 5, 6, 2, 3)])
    tf = hand_frame([[U + 1, V], [U + 2, V], [U + 3, V], [U + 4, V], [U + 5, V]], [0, 1, 3, 4, 2], desc=descs)
    assert check_frame(gpu_ctx, tf, track.FrameQueries(P0, [2], zero), 20).match.tolist() == [4]    # octave 2: [1, 3] -> key point 4 (d 3)
    assert check_frame(gpu_ctx, tf, track.FrameQueries(P0, [4], zero), 20).match.tolist() == [3]    # octave 4: [3, 5] -> key point 3 (d 2)
    nrm = P0 / np.float32(np.linalg.norm(P0))
    dist = float(np.linalg.norm(P0.astype(np.float64)))
    maxd = np.array([dist * 1.2 ** 2.5], np.float32)                                                 # predicted level 3: window [2, 3]
    g = check_local(gpu_ctx, tf, track.LocalQueries(P0, nrm, maxd, zero), 3)
    assert g.level[0] == 3 and g.match.tolist() == [4]


def test_a_window_over_the_candidate_limit_is_refused(gpu_ctx):
    """More than 4096 candidates in one query's window is DSH_ERR_ARG (a clean refusal, not a truncated search); 4096 are fine."""
    from defslam_amd import sft, track
    zero = np.zeros((1, 32), np.uint8)
    fq = track.FrameQueries(P0, [0], zero)
    tf = hand_frame(np.tile(np.array([[U + 1, V]], np.float32), (4097, 1)), np.zeros(4097))
    with pytest.raises(sft.DshError, match="status 1.*4096 candidates"):
        track.SearchByProjectionFrame(gpu_ctx, tf, fq, 20)
    tf = hand_frame(np.tile(np.array([[U + 1, V]], np.float32), (4096, 1)), np.zeros(4096))
    assert check_frame(gpu_ctx, tf, fq, 20).match.tolist() == [0]


# ---- other cameras, image bounds and poses (tests/operating_points.py) -----------------------------------------------------------------------
# (camera, world, image bounds or None for (0, width, 0, height), seed)
MOVED_SCENES = [("hamlyn", "oblique", None, 31), ("tall", "turn_y", None, 32), ("webcam", "turn_x", None, 33), ("hamlyn", "turn_z", (-12.3, 707.7, -7.6, 280.4), 34),
                ("tall", "oblique", None, 35)]
_SCENES = {}


def moved_scene(camera, world, bounds, seed):
    """make_track_scene in a camera of the reference's settings files (fx != fy) and its image area, then the whole scene moved by a world:
    points G x and normals R n as float32, the pose Tcw G^-1 as float32 (Ow follows from it).  Built once per scene and shared."""
    key = (camera, world, bounds, seed)
    if key not in _SCENES:
        from defslam_amd import synth, track
        fx, fy, cx, cy, w, h = op.CAMERAS[camera]
        sc = synth.make_track_scene(seed, n_kp=1200, n_frame_q=400, n_local_q=300, state_mix=seed % 2 == 1, camera=(fx, fy, cx, cy),
                                    bounds=(0.0, float(w), 0.0, float(h)) if bounds is None else bounds)
        G = op.world_matrix(world)
        mv = lambda x: (np.asarray(x, np.float64) @ G[:3, :3].T + G[:3, 3]).astype(np.float32)
        tf = track.TrackFrame(**{**sc["frame"].__dict__, "Tcw": op.move_pose(G, sc["frame"].Tcw), "Ow": None})
        assert op.quaternion_branch(tf.Tcw) == op.WORLD_BRANCH[world] and tf.K[0] != tf.K[1]
        fq = track.FrameQueries(xyz=mv(sc["fq"].xyz), octave=sc["fq"].octave, desc=sc["fq"].desc)
        lq = sc["lq"]
        lq = track.LocalQueries(xyz=mv(lq.xyz), normal=(lq.normal.astype(np.float64) @ G[:3, :3].T).astype(np.float32), max_distance=lq.max_distance, desc=lq.desc,
                                skip=lq.skip)
        _SCENES[key] = (tf, fq, lq)
    return _SCENES[key]


@pytest.mark.parametrize("camera,world,bounds,seed", MOVED_SCENES, ids=[f"{c}-{w}" + ("-negative-bounds" if b else "") for c, w, b, _ in MOVED_SCENES])
def test_both_searches_at_other_cameras_bounds_and_poses(gpu_ctx, camera, world, bounds, seed):
    """fx > fy and fy > fx, image areas other than 640 x 480 (one that starts at a negative non-integer minimum), poses far from identity:
    both searches at both thresholds, every output bit-exact against the restatement; and they do find the scene's matches."""
    tf, fq, lq = moved_scene(camera, world, bounds, seed)
    g20 = check_frame(gpu_ctx, tf, fq, 20)
    g25 = check_frame(gpu_ctx, tf, fq, 25)
    assert g20.nmatches > 0.3 * len(g20.match) and g25.nmatches > 0
    g3 = check_local(gpu_ctx, tf, lq, 3)
    g5 = check_local(gpu_ctx, tf, lq, 5)
    assert g3.nmatches > 0 and g5.nmatches > 0 and g3.in_view.sum() > 0.3 * len(g3.match)


def test_batch_of_frames_with_different_cameras_and_bounds(gpu_ctx):
    """One batch whose frames differ in camera, image bounds and pose (a kernel that took problem 0's camera or bounds for all fails):
    every problem gives what it gives alone, bit for bit, and what the restatement gives."""
    from defslam_amd import track
    items = []
    for camera, world, bounds, seed in MOVED_SCENES[:4]:
        tf, fq, lq = moved_scene(camera, world, bounds, seed)
        items += [(tf, fq, 20), (tf, lq, 3)]
    items = items[1:] + items[:1]                                   # neither sorted by frame nor by mode
    batch = track.search_batch(gpu_ctx, items)
    for (f, qs, th), b in zip(items, batch):
        one = track.search_batch(gpu_ctx, [(f, qs, th)])[0]
        np.testing.assert_array_equal(b.match, one.match)
        assert b.nmatches == one.nmatches and b.nmatches > 0
        if isinstance(qs, track.LocalQueries):
            np.testing.assert_array_equal(b.in_view, one.in_view)
            np.testing.assert_array_equal(b.level, one.level)
            np.testing.assert_array_equal(b.uv, one.uv)
            m, n, *_ = R.search_local(R.ref_frame(f), f.arrays()["state"], qs.xyz, qs.normal, qs.max_distance, qs.desc, qs.skip, th)
        else:
            m, n, _ = R.search_frame(R.ref_frame(f), f.arrays()["state"], qs.xyz, qs.octave, qs.desc, th)
        np.testing.assert_array_equal(b.match, m)
        assert b.nmatches == n


def test_dyadic_anisotropic_camera_on_the_device(gpu_ctx):
    """The known answers of test_track_search_cpu.py at fx = 512, fy = 256 and image bounds (-8, 712, -4, 284), on the device: fx on x and fy
    on y (a point only the right assignment puts into the image; one only the swapped assignment would), the strict window edge, inclusive
    bounds at negative minima, grid cells on both sides of a negative minimum bound."""
    from defslam_amd import track
    zero = np.zeros((1, 32), np.uint8)
    nrm = lambda P: P / np.float32(np.linalg.norm(P))
    one = np.array([1.0], np.float32)
    tf = dyadic_frame([[UD, VD], [332.5, 172.25]], [0, 0])
    assert check_frame(gpu_ctx, tf, track.FrameQueries(P0, [0], zero), 3).match.tolist() == [0]
    g = check_local(gpu_ctx, tf, track.LocalQueries(P0, nrm(P0), one, zero), 1)
    assert g.in_view[0] and g.uv[0].tolist() == [UD, VD] and g.match.tolist() == [0]
    tf = dyadic_frame([[364.5, 268.25], [556.5, 204.25]], [0, 0])
    assert check_frame(gpu_ctx, tf, track.FrameQueries(P_ONLY_UNSWAPPED, [0], zero), 20).match.tolist() == [0]
    assert check_frame(gpu_ctx, tf, track.FrameQueries(P_ONLY_SWAPPED, [0], zero), 20).match.tolist() == [-1]
    g = check_local(gpu_ctx, tf, track.LocalQueries(np.concatenate([P_ONLY_UNSWAPPED, P_ONLY_SWAPPED]), np.concatenate([nrm(P_ONLY_UNSWAPPED), nrm(P_ONLY_SWAPPED)]),
                                                    np.array([1.0, 1.0], np.float32), np.zeros((2, 32), np.uint8)), 3)
    assert g.in_view.tolist() == [True, False] and g.uv[0].tolist() == [364.5, 268.25] and g.match.tolist() == [0, -1]
    tf = dyadic_frame([[UD + 20, VD], [UD, VD - 20], [UD + 19.75, VD - 19.75]], [0, 0, 0])
    assert check_frame(gpu_ctx, tf, track.FrameQueries(P0, [0], zero), 20).match.tolist() == [2]
    for P, bounds, inside in DYADIC_BOUND_CASES:
        # the key point 6 / 4 px inside the image from the projection (closer to a max bound it would round to the column / row past the grid:
        # columns are 11.25 px wide, rows 6 px high; the local search looks 7.5 px far)
        kx = float(np.float32(512) * P[0, 0] + np.float32(300.5)) + (6.0 if P[0, 0] < 0 else -6.0)
        ky = float(np.float32(256) * P[0, 1] + np.float32(140.25)) + (4.0 if P[0, 1] < 0 else -4.0)
        tf = hand_frame([[kx, ky]], [0], K=K_DY, bounds=bounds)
        assert (check_frame(gpu_ctx, tf, track.FrameQueries(P, [0], zero), 20).match[0] == 0) == inside, bounds
        g = check_local(gpu_ctx, tf, track.LocalQueries(P, nrm(P), one, zero), 3)
        assert bool(g.in_view[0]) == inside and (g.match[0] == 0) == inside, bounds
    descs = np.stack([desc_with_dist(d) for d in (0, 0, 7, 1, 9, 20)])
    tf = dyadic_frame([[100.0, -1.0], [100.0, -1.01], [-9.0, 50.0], [-14.0, 50.0], [-7.0, 50.0], [4.0, 50.0]], [0] * 6, desc=descs)
    P = np.array([[-617.0 / 1024, -90.25 / 256, 1.0]], np.float32)          # projects to (-8, 50): on mnMinX
    assert check_frame(gpu_ctx, tf, track.FrameQueries(P, [0], zero), 20).match.tolist() == [2]
    # rows around y = -1: equal distances, the key point in the lower row (y = -1.01, row 0) is visited first and wins
    Pr = np.array([[(100.0 - 300.5) / 512, (-1.0 - 140.25) / 256, 1.0]], np.float32)
    tf = dyadic_frame([[100.0, -1.0], [100.0, -1.01]], [0, 0], desc=np.stack([desc_with_dist(3), desc_with_dist(3)]))
    assert check_frame(gpu_ctx, tf, track.FrameQueries(Pr, [0], zero), 20).match.tolist() == [1]
