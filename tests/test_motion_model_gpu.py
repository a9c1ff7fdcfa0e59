"""GPU tests of dsh_track_end_frame, dsh_track_last_frame and dsh_motion_model_search: every output -- the end-of-frame outputs and
counts, the resident list, frame_points, match, nmatches, th_used -- equals the sequential restatement tests/motion_model_ref.py run on a
host mirror of the same calls, and match equals dsh_search_by_projection_frame fed with the same queries packed on the host, bit for
bit.  Integers: no tolerance anywhere.  About 300 key points on the default 64 x 48 grid; last frames of 0, 1, 63, 64, 65, 130 and 1025
key points put the gather's ordered compaction across lane, wavefront and workgroup boundaries."""
import numpy as np
import pytest

import motion_model_ref as M
import track_search_ref as R
from test_motion_model_cpu import LENGTHS, make_scene
from test_track_close_gpu import BothT, check_state

pytestmark = pytest.mark.gpu


class BothM(BothT):
    """The same end of frame or search on the store and on the host mirror (a MotionRefMap), compared output by output."""

    def check_list(self):
        g = self.st.last_frame()
        ids, oc = self.rm.last_frame()
        assert np.array_equal(g.ids, ids) and np.array_equal(g.octave, oc)
        return g

    def end(self, points, outlier, octave):
        g = self.st.end_frame(points, outlier, octave)
        r = self.rm.end_frame(points, outlier, octave)
        assert np.array_equal(g.points, r["points"]) and np.array_equal(g.outlier, r["outlier"])
        assert (g.cleaned, g.dropped, g.kept) == (r["cleaned"], r["dropped"], r["kept"])
        self.check_list()
        return g

    def mm(self, frame, **kw):
        g = self.st.motion_model_search(frame, **kw)
        r = self.rm.motion_model_search(frame, **kw)
        assert np.array_equal(g.frame_points, r["frame_points"]) and np.array_equal(g.match, r["match"])
        assert g.nmatches == r["nmatches"] and g.th_used == r["th_used"] and g.ok == r["ok"]
        return g


def fill_from_scene(st, sc):
    """What test_track_close_gpu.both_from_scene puts into a fresh store, into an empty one (a new store, or one that was cleared)."""
    st.add_points(sc["xyz"], sc["normal"], sc["max_distance"], sc["desc"], sc["bad"])
    for k in range(sc["tables"].shape[0]):
        assert st.add_keyframe(sc["tables"][k], sc["parents"][k], sc["kf_bad"][k]) == k
    st.add_observations(sc["obs_point"], sc["obs_kf"])
    P = sc["xyz"].shape[0]
    st.set_counters(np.arange(P), sc["visible"], sc["found"])
    st.set_embedding(np.arange(P), sc["nodes"], sc["bary"])


def both_from_scene(ctx, sc, **caps):
    from defslam_amd import localmap
    st = localmap.MapPointStore(ctx, **caps)
    fill_from_scene(st, sc)
    return BothM(st, M.scene_to_ref(sc))


@pytest.fixture(scope="module")
def scene():
    return make_scene()


def hand_both(ctx):
    from defslam_amd import localmap
    rm = M.hand_map()
    st = localmap.MapPointStore(ctx, points=2, keyframes=1, observations=2)        # tiny: every array grows
    rm.fill(st)
    for p in range(len(rm.points)):
        if rm.nodes[p] is not None:
            st.set_embedding([p], [rm.nodes[p]], [rm.bary[p]])
    return BothM(st, rm)


# ---- the hand-built case ---------------------------------------------------------------------------------------------------------------

def test_hand_built_case_with_a_query_without_observations(gpu_ctx):
    """p0 loses its only observation after the frame ended (n_obs == 0, not bad): its pick does not block key point 0, p1 takes the key
    point again, frame_points holds the last writer and nmatches counts both."""
    both = hand_both(gpu_ctx)
    fr = M.hand_frame()
    g = both.end(M.HAND_LAST_POINTS, M.HAND_LAST_OUTLIER, M.HAND_LAST_OCTAVE)
    assert g.points.tolist() == M.HAND_END["points"] and g.outlier.astype(int).tolist() == M.HAND_END["outlier"]
    assert (g.cleaned, g.dropped, g.kept) == (M.HAND_END["cleaned"], M.HAND_END["dropped"], M.HAND_END["kept"])
    lf = both.check_list()
    assert lf.ids.tolist() == M.HAND_LIST[0] and lf.octave.tolist() == M.HAND_LIST[1]
    g = both.mm(fr, min_matches=2)                                                   # everybody observed: p0 blocks key point 0
    assert g.frame_points.tolist() == M.HAND_BLOCKING_FRAME_POINTS and g.match.tolist() == M.HAND_BLOCKING_MATCH
    assert g.nmatches == M.HAND_BLOCKING_NMATCHES and g.th_used == 20.0
    both.forget([(0, 0)])
    both.set_bad([3])
    assert both.st.get_state([0]).n_obs.tolist() == [0]
    g = both.mm(fr, min_matches=2)
    assert g.frame_points.tolist() == M.HAND_FRAME_POINTS and g.match.tolist() == M.HAND_MATCH
    assert g.nmatches == M.HAND_NMATCHES and g.th_used == 20.0
    g = both.mm(fr)                                                                  # 3 < 20: the gated wide pass runs
    assert g.match.tolist() == M.HAND_MATCH and g.nmatches == M.HAND_NMATCHES and g.th_used == 25.0 and not g.ok
    both.check_list()                                                                # a search does not change the list
    both.st.close()


# ---- generated scenes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [0] + LENGTHS)
def test_every_length_equals_the_restatement_and_the_packed_call(gpu_ctx, scene, L):
    """end_frame, the list, the default search, and the search at th 20 and at th 25 alone (min_matches = 0: no retry), each against the
    restatement and against dsh_search_by_projection_frame with the same queries packed on the host: every kept query has observations
    after end_frame, so the two searches must agree bit for bit."""
    from defslam_amd import track
    both = both_from_scene(gpu_ctx, scene, points=16, keyframes=2, observations=64)
    pts, out, octs = M.make_last_frame(scene, L) if L else (np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, np.int32))
    e = both.end(pts, out, octs)
    fr = scene["frame"]
    g = both.mm(fr)
    assert g.match.shape == (L,)
    if L == 0:
        assert g.nmatches == 0 and g.th_used == 25.0 and (g.frame_points == -1).all()
    if L >= 130:
        assert e.cleaned > 0 and e.dropped > 0 and g.nmatches >= 20 and g.th_used == 20.0
    idx, xyz, octave, desc = both.rm.last_frame_queries()
    assert len(idx) <= e.kept
    empty = track.TrackFrame(**{**fr.__dict__, "state": None})
    for th in (20.0, 25.0):
        s = both.mm(fr, th=th, th_wide=th + 5.0, min_matches=0)
        assert s.th_used == th
        h = track.SearchByProjectionFrame(gpu_ctx, empty, track.FrameQueries(xyz, octave, desc), th)
        assert s.match[idx].tobytes() == h.match.tobytes() and s.nmatches == h.nmatches
        assert (np.delete(s.match, idx) == -1).all()
    check_state(both.st, both.rm)                                                    # neither call touches a point
    both.st.close()


@pytest.mark.parametrize("target,used", [(19, 25.0), (20, 20.0)])
def test_retry_boundary(gpu_ctx, scene, target, used):
    """The last frame trimmed on the restatement until the narrow search finds exactly 19, and exactly 20: the first comes back with the
    fresh search at th_wide, the second with the narrow result."""
    both = both_from_scene(gpu_ctx, scene)
    pts, out, octs = M.make_last_frame(scene, 130)
    rm = both.rm
    rm.end_frame(pts, out, octs)
    gone = M.trim_to_narrow_count(rm, scene["frame"], target)
    pts = pts.copy()
    pts[gone] = -1
    fr = R.ref_frame(scene["frame"])
    assert rm.search_by_projection(fr, 20)[2] == target                              # on the CPU, before the device call
    wide = rm.search_by_projection(fr, 25)
    both.end(pts, out, octs)
    g = both.mm(scene["frame"])
    assert g.th_used == used and g.nmatches == (wide[2] if used == 25.0 else target)
    if used == 25.0:
        assert np.array_equal(g.match, wide[1]) and np.array_equal(g.frame_points, wide[0])
    both.st.close()


def test_filters_follow_the_store(gpu_ctx, scene):
    """A point set bad, moved or re-described, an observation erased and the template cleared between end_frame and the search change
    the result as the restatement says: the queries are gathered at call time."""
    both = both_from_scene(gpu_ctx, scene)
    both.end(*M.make_last_frame(scene, 130))
    g0 = both.mm(scene["frame"])
    taken = both.rm.last_frame()[0][g0.match >= 0]
    both.set_bad(taken[:5].tolist())
    g1 = both.mm(scene["frame"])
    assert g1.nmatches < g0.nmatches and not np.isin(taken[:5], g1.frame_points).any()
    both.embed(taken[5:8], np.full((3, 3), -1, np.int32), np.zeros((3, 3)))          # three facets removed
    g2 = both.mm(scene["frame"])
    assert g2.nmatches < g1.nmatches and not np.isin(taken[5:8], g2.frame_points).any()
    both.move(taken[8:10].tolist(), np.array([both.rm.points[p].xyz for p in taken[8:10]]) + np.float32(0.5))
    both.mm(scene["frame"])
    both.st.clear_embedding()
    both.rm.clear_embedding()
    g3 = both.mm(scene["frame"])
    assert g3.nmatches == 0 and g3.th_used == 25.0 and (g3.match == -1).all()
    both.check_list()
    both.st.close()


def run_four_frames(both, sc):
    """motion_model_search -> update_local_map -> search_local_points -> close_frame with a repose -> end_frame, four times; every step is
    compared with the restatement inside `both`.  Returns the bytes of every output."""
    from defslam_amd import track
    rng = np.random.default_rng(99)
    N = sc["frame_points"].shape[0]
    koct = sc["frame"].arrays()["octave"]
    both.end(*M.make_last_frame(sc, 130))                                            # MonocularInitialization's call (DefTracking.cc:637)
    blob = []
    for t in range(4):
        fr = sc["frame_after"] if t % 2 else sc["frame"]
        g = both.mm(fr)
        assert g.nmatches > 0
        fp = g.frame_points
        u, _ = both.update(fp)
        s = both.search(track.TrackFrame(**{**fr.__dict__, "state": (fp >= 0).astype(np.uint8)}), u.n_local_points)
        final = np.where(u.frame_bad, -1, fp)                                        # Tracking.cc:1527-1530
        matched = s.match >= 0
        final[s.match[matched]] = s.local_ids[matched]                               # the search's matches join the frame
        out = ((final >= 0) & (rng.uniform(size=N) < 0.15)).astype(np.uint8)
        c = both.close(fr, final, out, sc["node_xyz"] + rng.normal(0, 1e-3, sc["node_xyz"].shape))
        e = both.end(final, out, koct)
        assert e.kept > 0
        lf = both.st.last_frame()
        st = check_state(both.st, both.rm)
        blob += [g.frame_points.tobytes(), g.match.tobytes(), np.array([g.nmatches, int(g.th_used)] + list(c.values()), np.int32).tobytes(),
                 e.points.tobytes(), e.outlier.tobytes(), np.array([e.cleaned, e.dropped, e.kept], np.int32).tobytes(), lf.ids.tobytes(),
                 lf.octave.tobytes(), st.xyz.tobytes(), st.visible.tobytes(), st.found.tobytes()]
    return b"".join(blob)


def test_four_chained_frames_twice_on_one_store(gpu_ctx, scene):
    from defslam_amd import sft
    both = both_from_scene(gpu_ctx, scene, points=16, keyframes=2, observations=64)
    first = run_four_frames(both, scene)
    both.st.clear()                                                                  # a reset forgets the list too
    with pytest.raises(sft.DshError, match="status 1: dsh_motion_model_search: no resident last-frame list"):
        both.st.motion_model_search(scene["frame"])
    with pytest.raises(sft.DshError, match="status 1: dsh_track_last_frame: no resident last-frame list"):
        both.st.last_frame()
    fill_from_scene(both.st, scene)
    both.rm = M.scene_to_ref(scene)
    assert run_four_frames(both, scene) == first
    both.st.close()


def test_refusals_on_a_live_store_change_nothing(gpu_ctx, scene):
    """No list before the first end_frame; then ids outside the store, N outside 0 .. 8192, an octave outside 0 .. 127 or beyond the
    frame's levels, NULL arrays: DSH_ERR_ARG naming the entry, and the list and every point are as before."""
    import ctypes as C
    from defslam_amd import sft, track
    both = both_from_scene(gpu_ctx, scene)
    st, fr = both.st, scene["frame"]
    with pytest.raises(sft.DshError, match="status 1: dsh_motion_model_search: no resident last-frame list"):
        st.motion_model_search(fr)
    both.end(*M.make_last_frame(scene, 65))
    before, lf = check_state(st, both.rm), both.check_list()
    P = scene["xyz"].shape[0]
    N = fr.arrays()["kp"].shape[0]
    few = track.TrackFrame(**{**fr.__dict__, "scale_factors": fr.arrays()["sf"][:2]})   # two levels: the list holds higher octaves
    assert lf.octave.max() >= 2
    for call, word in ((lambda: st.end_frame([P], [0], [0]), r"frame_points\[0\]"), (lambda: st.end_frame([0, -2], [0, 0], [0, 0]), r"frame_points\[1\]"),
                       (lambda: st.end_frame(np.full(8193, -1), np.zeros(8193), np.zeros(8193)), "N outside"),
                       (lambda: st.end_frame([0, 1], [0, 0], [0, 128]), r"octave\[1\]"), (lambda: st.end_frame([0], [0], [-1]), r"octave\[0\]"),
                       (lambda: st.last_frame(64), "capacity"),
                       (lambda: st.motion_model_search(fr, th=0.0), "positive finite"), (lambda: st.motion_model_search(fr, th_wide=float("nan")), "positive finite"),
                       (lambda: st.motion_model_search(fr, min_matches=-1), "min_matches"),
                       (lambda: st.motion_model_search(few), "levels-1"),
                       (lambda: st.motion_model_search(track.TrackFrame(**{**fr.__dict__, "grid": (200, 200)})), "grid")):
        with pytest.raises(sft.DshError, match="status 1: dsh_(track_end_frame|track_last_frame|motion_model_search): .*" + word):
            call()
    L = gpu_ctx._L
    z = np.zeros(N, np.int32)
    zi = z.ctypes.data_as(C.POINTER(C.c_int32))
    keep = []
    assert L.dsh_track_end_frame(st._h, 1, zi, None, zi, None, None, None) == 1
    assert L.dsh_track_end_frame(st._h, 1, None, None, None, None, None, None) == 1
    assert L.dsh_motion_model_search(st._h, None, 20.0, 25.0, 20, zi, None, None, None) == 1
    assert L.dsh_motion_model_search(st._h, C.byref(fr.c(keep)), 20.0, 25.0, 20, None, None, None, None) == 1
    after = check_state(st, both.rm)
    assert before.xyz.tobytes() == after.xyz.tobytes() and before.found.tolist() == after.found.tolist()
    both.check_list()
    both.mm(fr)                                                                      # and it still works
    assert L.dsh_motion_model_search(st._h, C.byref(fr.c(keep)), 20.0, 25.0, 20, zi, None, None, None) == 0   # match, nmatches, th_used may be NULL
    both.st.close()
