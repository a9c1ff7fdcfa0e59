"""GPU tests of the per-point tracking state of the map point store and of dsh_track_close_frame: after every sequence of calls the
state of ALL points (mnVisible, mnFound, nObs, and the positions as bytes) and the counts equal the sequential restatement
tests/track_close_ref.py run on a host mirror of the same mutations.  Integers and bytes: no tolerance anywhere."""
import numpy as np
import pytest

import track_close_ref as T
from test_local_map_gpu import Both, check_update, store_from_scene
from test_track_close_cpu import SCENES, make_scene

pytestmark = pytest.mark.gpu


def counts_dict(c):
    return {k: getattr(c, k) for k in T.COUNT_NAMES}


def check_state(store, rm):
    """get_state of all points against the mirror."""
    g = store.get_state()
    v, f, o, x = rm.track_state()
    np.testing.assert_array_equal(g.visible, v)
    np.testing.assert_array_equal(g.found, f)
    np.testing.assert_array_equal(g.n_obs, o)
    assert g.xyz.tobytes() == x.tobytes()
    return g


class BothT(Both):
    """The same mutation or frame step on the store and on the host mirror (a TrackRefMap)."""

    def add_points(self, xyz, normal, md, desc):
        ids = super().add_points(xyz, normal, md, desc)
        return ids

    def set_bad(self, ids):
        self.st.set_points_bad(ids)
        for p in ids:
            self.rm.set_bad(int(p))

    def embed(self, ids, nodes, bary):
        self.st.set_embedding(ids, nodes, bary)
        for i, p in enumerate(ids):
            self.rm.set_embedding(int(p), nodes[i], bary[i])

    def counters(self, ids, visible, found):
        self.st.set_counters(ids, visible, found)
        for i, p in enumerate(ids):
            self.rm.set_counters(int(p), visible[i], found[i])

    def update(self, frame_points):
        return check_update(self.st, self.rm, frame_points)

    def search(self, frame, n_local_points):
        g = self.st.search_local_points(frame, n_local_points)
        r = self.rm.search_local_points(frame)
        np.testing.assert_array_equal(g.match, r["match"])
        np.testing.assert_array_equal(g.in_view, r["in_view"])
        return g

    def close(self, frame, frame_points, outlier, node_xyz=None, only_tracking=False):
        g = counts_dict(self.st.close_frame(frame, frame_points, outlier, node_xyz, only_tracking))
        r = self.rm.close_frame(frame, frame_points, outlier, node_xyz, only_tracking)
        assert g == r
        return g

    def cull(self, ids, first_kf, current_kf):
        g = self.st.cull(ids, first_kf, current_kf)
        r = self.rm.cull(ids, first_kf, current_kf)
        np.testing.assert_array_equal(g, r)
        return g


def both_from_scene(ctx, sc, scene_to_ref=T.scene_to_ref, **caps):
    st = store_from_scene(ctx, sc, **caps)
    P = sc["xyz"].shape[0]
    st.set_counters(np.arange(P), sc["visible"], sc["found"])
    st.set_embedding(np.arange(P), sc["nodes"], sc["bary"])
    return BothT(st, scene_to_ref(sc))


# ---- the hand-built map ----------------------------------------------------------------------------------------------------------------

def hand_both(ctx):
    from defslam_amd import localmap
    rm = T.hand_map(erased=False)
    st = localmap.MapPointStore(ctx, points=2, keyframes=1, observations=2)        # tiny: every array grows, the new ones too
    rm.fill(st)
    both = BothT(st, rm)
    for p in range(6):
        if rm.nodes[p] is not None:
            st.set_embedding([p], [rm.nodes[p]], [rm.bary[p]])
    both.forget([(5, 0), (5, 0)])                                                   # the device sees the erase itself; the second finds nothing
    return both


@pytest.mark.parametrize("only_tracking", [False, True])
def test_hand_built_map_first_frame(gpu_ctx, only_tracking):
    both = hand_both(gpu_ctx)
    fr = T.hand_frame()
    g, _ = both.update(T.HAND_FRAME_POINTS)
    assert both.st.local_points(g.n_local_points).tolist() == T.HAND_FIRST_LIST
    both.search(fr, g.n_local_points)
    both.set_bad([3])
    c = both.close(fr, T.HAND_FRAME_POINTS, T.HAND_OUTLIER, T.HAND_NODES_AFTER, only_tracking)
    assert c == (T.HAND_COUNTS_ONLY_TRACKING if only_tracking else T.HAND_COUNTS)
    s = check_state(both.st, both.rm)
    assert s.visible.tolist() == T.HAND_VISIBLE and s.found.tolist() == T.HAND_FOUND and s.n_obs.tolist() == T.HAND_N_OBS
    assert s.xyz.tobytes() == T.HAND_XYZ_AFTER.tobytes()
    both.st.close()


def test_hand_built_map_second_frame_previous_list_and_cull(gpu_ctx):
    both = hand_both(gpu_ctx)
    fr = T.hand_frame()
    g, _ = both.update(T.HAND_FRAME_POINTS)
    both.search(fr, g.n_local_points)
    both.set_bad([3])
    both.close(fr, T.HAND_FRAME_POINTS, T.HAND_OUTLIER, T.HAND_NODES_AFTER)
    both.set_kf_bad(1)
    g, _ = both.update([0])
    assert both.st.local_points(g.n_local_points).tolist() == T.HAND_SECOND_LIST
    both.search(fr, g.n_local_points)
    c = both.close(fr, [0], [0])                                                    # node_xyz = NULL: every position stays
    assert c["local_map_points"] == T.HAND_SECOND_LOCAL_MAP_POINTS != T.HAND_SECOND_WRONG_LIST_COUNT and c["n_moved"] == 0
    assert check_state(both.st, both.rm).xyz.tobytes() == T.HAND_XYZ_AFTER.tobytes()
    both.counters([1], [5], [1])
    assert both.cull(np.arange(6), T.HAND_FIRST_KF, T.HAND_CURRENT_KF).tolist() == T.HAND_ACTIONS
    g, _ = both.update([0, 1, 2, 3, 4, 5])                                          # the bad flags as the next update sees them
    assert g.frame_bad.tolist() == [False, True, False, True, False, False]
    check_state(both.st, both.rm)                                                   # n_obs of the culled point stayed
    both.st.close()


def test_seed_clear_embedding_and_a_cleared_store(gpu_ctx):
    both = hand_both(gpu_ctx)
    fr = T.hand_frame()
    assert counts_dict(both.st.close_frame(fr, [], []))["local_map_points"] == 0   # before any update or seed: the list is empty
    both.st.seed_local_points([0, 4, 5])
    both.rm.seed_local_points([0, 4, 5])
    assert both.st.local_points(3).tolist() == [0, 4, 5]
    assert both.close(fr, [], [])["local_map_points"] == 3
    assert both.st.repose(T.HAND_NODES_AFTER) == both.rm.repose(T.HAND_NODES_AFTER) == 5
    check_state(both.st, both.rm)
    both.st.clear_embedding()
    both.rm.clear_embedding()
    c = both.close(fr, [0], [0], T.HAND_NODES_AFTER)
    assert c["to_match_local"] == 0 and c["local_map_points"] == 0 and c["n_moved"] == 0
    assert both.st.repose(np.zeros((0, 3))) == 0                                   # no facet left: any template will do
    check_state(both.st, both.rm)
    both.st.clear()                                                                 # a reset forgets the new state too
    assert both.st.n_points == 0 and counts_dict(both.st.close_frame(fr, [], [])) == dict.fromkeys(T.COUNT_NAMES, 0)
    first = both.st.add_points(np.zeros((2, 3)), np.zeros((2, 3)), np.ones(2), np.zeros((2, 32), np.uint8))
    s = both.st.get_state()
    assert first == 0 and s.visible.tolist() == [1, 1] and s.found.tolist() == [1, 1] and s.n_obs.tolist() == [0, 0]
    assert both.st.repose(np.zeros((0, 3))) == 0
    both.st.close()


# ---- generated scenes ------------------------------------------------------------------------------------------------------------------

CASES = [(name, None) for name in sorted(SCENES)] + [("p1050", n) for n in (1, 63, 64, 65)]


@pytest.mark.parametrize("name,N", CASES)
def test_generated_frame_equals_the_restatement(gpu_ctx, name, N):
    """update -> search -> close on a second frame, so that the reference list is the first frame's and holds points that became bad;
    then the culling, seen through the next update's frame_bad."""
    sc = make_scene(name)
    both = both_from_scene(gpu_ctx, sc, points=16, keyframes=2, observations=64)
    both.update(T.previous_frame_points(sc))
    both.set_bad(sc["late_bad"].tolist())
    g, _ = both.update(sc["frame_points"])
    both.search(sc["frame"], g.n_local_points)
    n = sc["final_points"].shape[0] if N is None else N
    c = both.close(sc["frame_after"], sc["final_points"][:n], sc["outlier"][:n], sc["node_xyz"])
    rm = both.rm
    assert rm.reference_points != rm.local_points                                   # the two lists differ ...
    if name != "p30":                                                               # ... and so would the count (six keyframes are all local)
        assert rm.frustum_count(T.R.ref_frame(sc["frame_after"]), rm.local_points)[0] != c["local_map_points"]
    assert c["n_moved"] > 0 and 0 < c["local_map_points"] < len(rm.reference_points)
    check_state(both.st, rm)
    ids, first_kf = T.cull_list(sc)
    act = both.cull(ids, first_kf, sc["current_kf"])
    assert sorted(set(act.tolist())) == [0, 1, 2, 3]
    g, _ = both.update(ids)
    np.testing.assert_array_equal(g.frame_bad, np.array([rm.points[p].bad for p in ids]))
    check_state(both.st, rm)
    both.st.close()


def test_close_without_nodes_leaves_every_position(gpu_ctx):
    sc = make_scene("p30")
    both = both_from_scene(gpu_ctx, sc)
    before = both.st.get_state().xyz.tobytes()
    g, _ = both.update(sc["frame_points"])
    both.search(sc["frame"], g.n_local_points)
    c = both.close(sc["frame_after"], sc["final_points"], sc["outlier"], None, only_tracking=True)
    assert c["n_moved"] == 0 and c["matches_inliers"] == int(((sc["final_points"] >= 0) & (sc["outlier"] == 0)).sum())
    assert both.st.get_state().xyz.tobytes() == before
    check_state(both.st, both.rm)
    both.st.close()


def test_repose_chained_with_the_solver(gpu_ctx):
    """dsh_sft_solve on the smoke problem, then repose with dsh_sft_result.xyz over a store whose points carry the frame's obs_nodes /
    obs_bary: the observed points get mappoint_xyz byte for byte, the unobserved facet points the restatement's positions."""
    from defslam_amd import localmap, sft, synth
    tmpl, fr = synth.make_problem("smoke", 0)
    ctx = sft.Context(0)
    ctx.template_build(tmpl.xyz0, tmpl.facets)
    f = sft.frame_from_synth(fr)
    sft.DefPoseOptimization(ctx, f, synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    M = fr.obs_nodes.shape[0]
    rng = np.random.default_rng(5)
    extra = 70
    nodes = np.concatenate([fr.obs_nodes, np.sort(tmpl.facets[rng.integers(0, tmpl.facets.shape[0], extra)], axis=1)]).astype(np.int32)
    bary = np.concatenate([fr.obs_bary, rng.dirichlet((1.0, 1.0, 1.0), extra)])
    P = M + extra
    rm = T.TrackRefMap()
    for p in range(P):
        rm.add_point(xyz=(0, 0, 1))
        rm.set_embedding(p, nodes[p], bary[p])
    rm.set_embedding(P - 1, None)                                                   # one point without a facet, one bad
    rm.set_bad(P - 2)
    st = localmap.MapPointStore(ctx, points=64)
    rm.fill(st)
    st.set_embedding(np.arange(P - 1), nodes[:P - 1], bary[:P - 1])
    assert st.repose(f.nodes_xyz) == rm.repose(f.nodes_xyz) == P - 2
    g = check_state(st, rm)
    assert g.xyz[:M].tobytes() == np.ascontiguousarray(f.mappoints, np.float32).tobytes()
    assert g.xyz[P - 2:].tobytes() == np.array([[0, 0, 1], [0, 0, 1]], np.float32).tobytes()
    st.close()
    ctx.close()


def test_eight_frames_with_mutations_in_between_twice(gpu_ctx):
    """Eight frames; between them points are added (their state starts at 1 / 1 / 0 / no facet), embedded, moved, set bad, observations
    added and erased, counters overwritten, the template cleared once, points culled.  Every frame equals the restatement on a host
    mirror, and two runs on fresh stores give identical bytes."""
    from defslam_amd import synth, track
    runs = []
    for _ in range(2):
        sc = synth.make_track_close_scene(5, n_kf=20, n_kp=200, obs_per_point=6, n_frame_kp=500)
        both = both_from_scene(gpu_ctx, sc, points=16, keyframes=2, observations=64)
        rm = both.rm
        rng = np.random.default_rng(77)
        N = sc["frame_points"].shape[0]
        n_nodes = sc["node_xyz"].shape[0]
        facets = sc["template"].facets
        blob = []
        for t in range(8):
            P, K = len(rm.points), len(rm.kfs)
            new = both.add_points(rng.uniform(-0.3, 0.3, (5, 3)).astype(np.float32) + np.array([0, 0, 1], np.float32),
                                  np.tile(np.array([0, 0, 1], np.float32), (5, 1)), rng.uniform(0.5, 3, 5).astype(np.float32),
                                  rng.integers(0, 256, (5, 32), dtype=np.uint8))
            both.embed(new[:4], np.sort(facets[rng.integers(0, facets.shape[0], 4)], axis=1).astype(np.int32), rng.dirichlet((1.0, 1.0, 1.0), 4))
            both.observe([(p, K - 1) for p in new[:3]])
            ids = rng.choice(P, 8, replace=False)
            both.move(ids, np.array([rm.points[p].xyz for p in ids]) + rng.normal(0, 1e-3, (8, 3)).astype(np.float32))
            both.set_bad(rng.choice(P, 2, replace=False).tolist())
            have = [(p, k) for p in rng.choice(P, 20, replace=False).tolist() for k in list(rm.points[p].obs)[:1]]
            both.forget(have[:8] + [(int(new[4]), 0)])                              # and one pair that is not there
            if t == 3:
                ids = rng.choice(P, 10, replace=False)
                both.counters(ids, rng.integers(1, 30, 10).astype(np.int32), rng.integers(0, 10, 10).astype(np.int32))
                both.embed(ids[:3], np.full((3, 3), -1, np.int32), np.zeros((3, 3)))   # three facets removed
            if t == 5:
                both.st.clear_embedding()
                rm.clear_embedding()
            fp = np.full(N, -1, np.int32)
            held = rng.choice(len(rm.points), 120, replace=False)
            fp[rng.choice(N, 120, replace=False)] = held
            fp[rng.choice(np.nonzero(fp < 0)[0], 4, replace=False)] = held[:4]         # held twice
            g, _ = both.update(fp)
            fr = track.TrackFrame(**{**sc["frame"].__dict__, "state": (fp >= 0).astype(np.uint8)})
            s = both.search(fr, g.n_local_points)
            final = np.where(g.frame_bad, -1, fp)                                      # Tracking.cc:1527-1530
            matched = s.match >= 0
            final[s.match[matched]] = s.local_ids[matched]                             # the search's matches join the frame
            out = ((final >= 0) & (rng.uniform(size=N) < 0.2)).astype(np.uint8)
            nodes_t = sc["node_xyz"] + rng.normal(0, 1e-3, (n_nodes, 3))
            c = both.close(sc["frame_after"] if t % 2 else fr, final, out, nodes_t if t != 6 else None, only_tracking=(t == 4))
            recent = np.arange(max(0, len(rm.points) - 40), len(rm.points), dtype=np.int32)
            act = both.cull(recent, rng.integers(K - 4, K + 1, recent.shape[0]).astype(np.int32), K)
            st8 = check_state(both.st, rm)
            blob += [np.array(list(c.values()), np.int32).tobytes(), act.tobytes(), st8.visible.tobytes(), st8.found.tobytes(), st8.n_obs.tobytes(),
                     st8.xyz.tobytes()]
        assert both.st.n_points == sc["xyz"].shape[0] + 40
        both.st.close()
        runs.append(b"".join(blob))
    assert runs[0] == runs[1]


def test_refusals_on_a_live_store_store_nothing(gpu_ctx):
    """An id outside, an id repeated, a node index >= n_nodes, descending nodes, NULL arrays: DSH_ERR_ARG naming the entry, and the store
    answers as before."""
    import ctypes as C
    from defslam_amd import _lib, sft
    both = hand_both(gpu_ctx)
    st, fr = both.st, T.hand_frame()
    before = check_state(st, both.rm)
    b3, n3 = np.array([[0.2, 0.3, 0.5]]), np.array([[0, 1, 2]], np.int32)
    for call in (lambda: st.set_embedding([6], n3, b3), lambda: st.set_embedding([1, 1], np.tile(n3, (2, 1)), np.tile(b3, (2, 1))),
                 lambda: st.set_embedding([0], [[2, 1, 3]], b3),                       # descending
                 lambda: st.set_embedding([0], [[1, 1, 3]], b3),                       # not distinct
                 lambda: st.set_embedding([0], [[-1, 1, 3]], b3),
                 lambda: st.set_embedding([0], n3, None),                              # bary NULL with a facet to set
                 lambda: st.set_counters([6], [1], [1]), lambda: st.set_counters([2, 2], [1, 1], [1, 1]),
                 lambda: st.get_state([0, 6]), lambda: st.get_state([3, 3]),
                 lambda: st.seed_local_points([6]), lambda: st.seed_local_points([2, 1]), lambda: st.seed_local_points([1, 1]),
                 lambda: st.repose(T.HAND_NODES_AFTER[:3]),                            # the store holds node 3
                 lambda: st.cull([6], [0], 3), lambda: st.cull([0, 0], [0, 0], 3),
                 lambda: st.close_frame(fr, [6], [0]), lambda: st.close_frame(fr, [-2], [0]),
                 lambda: st.close_frame(fr, [0], [0], T.HAND_NODES_AFTER[:3])):
        with pytest.raises(sft.DshError, match="status 1: dsh_track"):
            call()
    L = gpu_ctx._L
    z = np.zeros(1, np.int32)
    zi = z.ctypes.data_as(C.POINTER(C.c_int32))
    keep = []
    cc = _lib.TrackCloseCountsC()
    assert L.dsh_trackstate_set_counters(st._h, 1, zi, None, zi) == 1
    assert L.dsh_trackstate_cull(st._h, 1, zi, None, 3, None) == 1
    assert L.dsh_track_close_frame(st._h, C.byref(fr.c(keep)), 1, zi, None, 0, None, 0, C.byref(cc)) == 1
    assert L.dsh_track_close_frame(st._h, C.byref(fr.c(keep)), 0, None, None, 0, None, 0, None) == 1
    after = check_state(st, both.rm)
    assert before.xyz.tobytes() == after.xyz.tobytes() and before.found.tolist() == after.found.tolist()
    # and it still works: the largest stored node index follows a facet that is removed
    st.set_embedding([1, 4, 5], np.full((3, 3), -1, np.int32))
    for p in (1, 4, 5):
        both.rm.set_embedding(p, None)
    assert st.repose(T.HAND_NODES_AFTER[:3]) == both.rm.repose(T.HAND_NODES_AFTER[:3]) == 2
    check_state(st, both.rm)
    st.close()
