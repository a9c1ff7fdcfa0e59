"""GPU tests of the map point store and the local map (dsh_mpdb_*, dsh_local_map_*): every output of dsh_local_map_update equals the
sequential restatement tests/local_map_ref.py exactly (integers: no tolerance), dsh_local_map_search equals the existing local-map
search fed with the same queries gathered on the host, bit for bit, and its matches equal tests/track_search_ref.py."""
import ctypes as C

import numpy as np
import pytest

import local_map_ref as LM
from test_local_map_cpu import ARG, OK, check_expected, scene_to_ref

pytestmark = pytest.mark.gpu


def store_from_scene(ctx, sc, **caps):
    from defslam_amd import localmap
    st = localmap.MapPointStore(ctx, **caps)
    st.add_points(sc["xyz"], sc["normal"], sc["max_distance"], sc["desc"], sc["bad"])
    for k in range(sc["tables"].shape[0]):
        assert st.add_keyframe(sc["tables"][k], sc["parents"][k], sc["kf_bad"][k]) == k
    st.add_observations(sc["obs_point"], sc["obs_kf"])
    return st


def check_update(store, rm, frame_points):
    """One dsh_local_map_update against the restatement: frame_bad, the list, the votes, ref_kf, the local ids -- all exact."""
    g = store.update_local_map(frame_points)
    r = rm.update_local_map(frame_points)
    np.testing.assert_array_equal(g.frame_bad, r["frame_bad"])
    np.testing.assert_array_equal(g.local_kf, r["local_kf"])
    np.testing.assert_array_equal(g.votes, r["votes"])
    assert g.ref_kf == r["ref_kf"]
    assert g.n_local_points == len(r["local_points"])
    np.testing.assert_array_equal(store.local_points(g.n_local_points), r["local_points"])
    return g, r


def check_search(ctx, store, rm, frame, n_local_points, th=3.0):
    """dsh_local_map_search against (a) dsh_search_by_projection_batch with the queries gathered on the host, every output bit for bit,
    and (b) the sequential restatement of the search."""
    from defslam_amd import track
    g = store.search_local_points(frame, n_local_points, th)
    ids, xyz, nrm, md, desc, skip = rm.queries()
    np.testing.assert_array_equal(g.local_ids, ids)
    h = track.SearchByProjectionLocal(ctx, frame, track.LocalQueries(xyz, nrm, md, desc, skip), th)
    for a, b in ((g.match, h.match), (g.in_view, h.in_view), (g.level, h.level), (g.uv, h.uv), (g.view_cos, h.view_cos)):
        assert a.tobytes() == b.tobytes()
    assert g.nmatches == h.nmatches
    r = rm.search_local_points(frame, th)
    np.testing.assert_array_equal(g.match, r["match"])
    assert g.nmatches == r["nmatches"]
    return g


SIZES = {"default": dict(n_kf=30, n_kp=1200, obs_per_point=8),            # the reference's size: about 30 keyframes x 1200 key points
         "kf300": dict(n_kf=300, n_kp=400, obs_per_point=8),
         "obs600": dict(n_kf=700, n_kp=200, obs_per_point=600)}             # 300 .. 700 observations per point, 600 nominal


@pytest.mark.parametrize("size", sorted(SIZES))
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_update_equals_the_restatement_on_generated_scenes(gpu_ctx, seed, size):
    from defslam_amd import synth
    sc = synth.make_local_map_scene(seed, **SIZES[size])
    if size == "obs600":
        assert np.bincount(sc["obs_point"]).max() >= 500
    rm = scene_to_ref(sc)
    st = store_from_scene(gpu_ctx, sc)
    g, _ = check_update(st, rm, sc["frame_points"])
    assert g.ref_kf >= 0 and g.frame_bad.any() and len(g.votes) > 0 and g.n_local_points > 0
    g2, _ = check_update(st, rm, sc["frame_points"])               # again: the same answer from the same state
    np.testing.assert_array_equal(g.local_kf, g2.local_kf)
    check_search(gpu_ctx, st, rm, sc["frame"], g.n_local_points)
    st.close()


@pytest.mark.parametrize("name", sorted(LM.hand_maps()))
def test_hand_built_maps_on_the_device(gpu_ctx, name):
    from defslam_amd import localmap
    rm, frame_points, want = LM.hand_maps()[name]
    if name == "erased_observation":                                # the device must see the erase itself, not a log without the pair
        assert rm.add_observation(1, 2)
    st = localmap.MapPointStore(gpu_ctx, points=2, keyframes=1, observations=2)        # tiny: every array grows
    rm.fill(st)
    if name == "erased_observation":
        st.erase_observations([1], [2])
        rm.erase_observation(1, 2)
    g, r = check_update(st, rm, frame_points)
    check_expected(r, want)
    assert g.local_kf.tolist() == want["local_kf"] and g.votes.tolist() == want["votes"] and g.ref_kf == want["ref_kf"]
    st.close()


def test_no_votes_keeps_the_previous_list_on_the_device(gpu_ctx):
    from defslam_amd import localmap
    rm, frame_points, want = LM.hand_maps()["parent_break"]
    st = localmap.MapPointStore(gpu_ctx, points=8, keyframes=8, observations=8)
    rm.fill(st)
    g0 = st.update_local_map([-1, -1])                              # before any vote: no list at all
    assert g0.local_kf.tolist() == [] and g0.ref_kf == -1 and g0.n_local_points == 0
    rm.update_local_map([-1, -1])
    check_update(st, rm, frame_points)
    st.set_points_bad([2])
    rm.points[2].bad = True
    for fp in ([-1, -1, -1], [], [2]):
        g, _ = check_update(st, rm, fp)
        assert g.local_kf.tolist() == want["local_kf"] and g.ref_kf == -1 and len(g.votes) == 0
        assert st.local_points(g.n_local_points).tolist() == [0, 3, 4]
    st.clear()                                                      # a reset forgets the list too
    assert st.n_points == 0 and st.n_keyframes == 0
    assert st.update_local_map([]).local_kf.tolist() == []
    st.close()


class Both:
    """The same mutation on the store and on the host mirror."""

    def __init__(self, store, rm):
        self.st, self.rm = store, rm

    def add_points(self, xyz, normal, md, desc):
        first = self.st.add_points(xyz, normal, md, desc)
        assert first == len(self.rm.points)
        for i in range(len(xyz)):
            self.rm.add_point(xyz[i], normal[i], md[i], desc[i])
        return list(range(first, first + len(xyz)))

    def move(self, ids, xyz):
        self.st.update_points(ids, xyz=xyz)
        for p, x in zip(ids, xyz):
            self.rm.points[p].xyz = np.asarray(x, np.float32)

    def redescribe(self, ids, normal, md, desc):
        self.st.update_points(ids, normal=normal, max_distance=md, desc=desc)
        for i, p in enumerate(ids):
            self.rm.points[p].normal, self.rm.points[p].max_distance, self.rm.points[p].desc = normal[i], np.float32(md[i]), desc[i]

    def set_bad(self, ids):
        self.st.set_points_bad(ids)
        for p in ids:
            self.rm.points[p].bad = True

    def observe(self, pairs):
        self.st.add_observations([p for p, _ in pairs], [k for _, k in pairs])
        for p, k in pairs:
            assert self.rm.add_observation(p, k)

    def forget(self, pairs):
        self.st.erase_observations([p for p, _ in pairs], [k for _, k in pairs])
        for p, k in pairs:
            self.rm.erase_observation(p, k)

    def add_keyframe(self, table, parent):
        k = self.st.add_keyframe(table, parent)
        assert k == self.rm.add_keyframe(table, parent)
        return k

    def set_table(self, k, idx, p):
        self.st.set_keyframe_point(k, idx, p)
        self.rm.kfs[k].table[idx] = p

    def set_parent(self, k, parent):
        self.st.set_keyframe_parent(k, parent)
        self.rm.kfs[k].parent = parent

    def set_kf_bad(self, k, bad=True):
        self.st.set_keyframe_bad(k, bad)
        self.rm.kfs[k].bad = bad


def test_a_sequence_of_frames_with_the_store_mutated_in_between(gpu_ctx):
    """24 frames; between them points are added, moved, re-described and set bad, observations added and erased, a keyframe added,
    another set bad, parents changed, table entries set and cleared.  Every frame equals the restatement run on a host mirror of the
    same mutations: the log, the erase, the growth of every array and the persistence of the previous list."""
    from defslam_amd import synth, track
    sc = synth.make_local_map_scene(5, n_kf=25, n_kp=300, obs_per_point=6, n_frame_kp=600)
    rm = scene_to_ref(sc)
    st = store_from_scene(gpu_ctx, sc, points=16, keyframes=2, observations=64)
    both = Both(st, rm)
    rng = np.random.default_rng(99)
    N = sc["frame_points"].shape[0]
    searched = 0
    for t in range(24):
        P, K = len(rm.points), len(rm.kfs)
        # --- mutations ---
        new = both.add_points(rng.uniform(-0.3, 0.3, (5, 3)).astype(np.float32) + np.array([0, 0, 1], np.float32),
                              np.tile(np.array([0, 0, 1], np.float32), (5, 1)), rng.uniform(0.5, 3, 5).astype(np.float32),
                              rng.integers(0, 256, (5, 32), dtype=np.uint8))
        last = K - 1
        free = [j for j, p in enumerate(rm.kfs[last].table) if p < 0][:5]
        for j, p in zip(free, new):                                  # the tracking inserts them into the newest keyframe's table ...
            both.set_table(last, j, p)
        both.observe([(p, last) for p in new[:3]])                   # ... and only some observe it yet
        ids = rng.choice(P, 12, replace=False)
        both.move(ids, np.array([rm.points[p].xyz for p in ids]) + rng.normal(0, 1e-3, (12, 3)).astype(np.float32))
        if t % 3 == 0:
            ids = rng.choice(P, 6, replace=False)
            nr = rng.normal(size=(6, 3))
            both.redescribe(ids, (nr / np.linalg.norm(nr, axis=1)[:, None]).astype(np.float32), rng.uniform(0.5, 3, 6).astype(np.float32),
                            rng.integers(0, 256, (6, 32), dtype=np.uint8))
        both.set_bad(rng.choice(P, 2, replace=False).tolist())
        fresh = set()
        while len(fresh) < 20:
            p, k = int(rng.integers(0, P)), int(rng.integers(0, K))
            if k not in rm.points[p].obs:
                fresh.add((p, k))
        both.observe(sorted(fresh))
        have = [(p, k) for p in rng.choice(P, 40, replace=False).tolist() for k in list(rm.points[p].obs)[:1]]
        both.forget(have[:15] + [(0, K - 1)] * (0 if (K - 1) in rm.points[0].obs else 1))     # and one pair that is not there: no change
        if t >= 12:
            both.observe(have[:3])                                   # an erased pair comes back as a new record
        if t == 5:
            both.add_keyframe(rng.choice(np.concatenate([np.arange(P), np.full(P, -1)]), 300).astype(np.int32), parent=K - 1)
        if t == 8:
            both.set_kf_bad(int(rm.local_kf[0]))                    # a keyframe of the current list
        if t == 11:
            both.set_parent(K - 1, 1)
            both.set_parent(2, K - 1)                                # a parent later in slot order
        if t == 17:
            both.set_kf_bad(int(rm.local_kf[0]), False)
            both.set_table(3, 0, -1)
        # --- the frame ---
        fp = np.full(N, -1, np.int32)
        if t not in (14, 20):                                        # two frames hold nothing: the previous list persists
            lo = int(rng.integers(0, max(1, len(rm.points) - 600)))
            held = rng.choice(np.arange(lo, min(lo + 600, len(rm.points))), 150, replace=False)
            fp[rng.choice(N, 150, replace=False)] = held
            fp[rng.choice(np.nonzero(fp < 0)[0], 4, replace=False)] = held[:4]      # held twice
        g, r = check_update(st, rm, fp)
        if t in (14, 20):
            assert g.ref_kf == -1 and len(g.votes) == 0 and len(g.local_kf) > 0
        if t % 6 == 2:
            fr = track.TrackFrame(**{**sc["frame"].__dict__, "state": (fp >= 0).astype(np.uint8)})
            check_search(gpu_ctx, st, rm, fr, g.n_local_points)
            searched += 1
    assert searched == 4 and len(rm.kfs) == 26 and st.n_points == len(rm.points) == sc["xyz"].shape[0] + 24 * 5
    st.close()


def test_two_identical_calls_give_identical_bytes(gpu_ctx):
    from defslam_amd import synth
    sc = synth.make_local_map_scene(4, n_kf=40, n_kp=600, obs_per_point=8)
    st = store_from_scene(gpu_ctx, sc)
    outs = []
    for _ in range(2):
        g = st.update_local_map(sc["frame_points"])
        s = st.search_local_points(sc["frame"], g.n_local_points)
        outs.append(b"".join(a.tobytes() for a in (g.frame_bad, g.local_kf, g.votes, st.local_points(g.n_local_points), s.local_ids, s.match, s.in_view,
                                                   s.level, s.uv, s.view_cos)) + bytes([g.ref_kf & 255, s.nmatches & 255]))
    assert outs[0] == outs[1]
    assert s.nmatches > 0 and s.in_view.sum() > 0
    st.close()


def test_refusals_on_a_live_store_store_nothing(gpu_ctx):
    """Against a store that holds something: ids and slots outside it, an index >= N, NULL arrays, a pair that is stored or repeated in
    the batch, a short capacity -- DSH_ERR_ARG with a message, and the store answers as before."""
    from defslam_amd import localmap, sft
    rm, frame_points, want = LM.hand_maps()["parent_break"]
    st = localmap.MapPointStore(gpu_ctx, points=8, keyframes=8, observations=8)
    rm.fill(st)
    z3, z1, d = np.zeros((1, 3), np.float32), np.ones(1, np.float32), np.zeros((1, 32), np.uint8)
    for call in (lambda: st.add_observations([0, 0], [1, 1]),                  # repeated in the batch
                 lambda: st.add_observations([0], [0]),                        # stored already
                 lambda: st.add_observations([6], [0]), lambda: st.add_observations([0], [6]),
                 lambda: st.erase_observations([0], [6]),
                 lambda: st.update_points([1, 1], xyz=np.zeros((2, 3))),       # repeated id
                 lambda: st.update_points([6], xyz=z3), lambda: st.set_points_bad([-1]),
                 lambda: st.add_keyframe([6]), lambda: st.add_keyframe([0], parent=6),
                 lambda: st.set_keyframe_point(0, 1, 0),                       # index >= N
                 lambda: st.set_keyframe_point(6, 0, 0), lambda: st.set_keyframe_point(0, 0, 6),
                 lambda: st.set_keyframe_parent(2, 2), lambda: st.set_keyframe_parent(2, 6), lambda: st.set_keyframe_bad(6),
                 lambda: st.update_local_map([6]), lambda: st.local_points(-1)):
        with pytest.raises(sft.DshError, match="status 1: dsh_"):
            call()
    L = gpu_ctx._L
    fp = np.array(frame_points, np.int32)
    kf = np.zeros(8, np.int32)
    p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.dsh_local_map_update(st._h, 2, p32(fp), None, 5, p32(kf), None, None, None, None, None) == ARG      # 6 keyframes need 6 entries
    assert L.dsh_local_map_update(st._h, 2, p32(fp), None, 0, None, None, None, None, None, None) == OK          # no list asked for
    assert st.n_points == 6 and st.n_keyframes == 6
    g, r = check_update(st, rm, frame_points)
    check_expected(r, want)
    with pytest.raises(sft.DshError, match="capacity"):
        st.search_local_points(LM_frame(), g.n_local_points - 1)
    st.close()


def LM_frame():
    from test_track_search_cpu import hand_frame
    return hand_frame([[100, 100], [300, 200]], [0, 1])
