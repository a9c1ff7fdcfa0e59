"""CPU tests of closing a tracked frame on the map point store: the restatement (tests/track_close_ref.py) on a hand-built map with the
expected numbers written out, the scene generator and what its scenes exercise, and the ABI of dsh_trackstate_* / dsh_track_close_frame
without a GPU (symbols, host-only refusals and their order, a detached store)."""
import ctypes as C

import numpy as np
import pytest

import track_close_ref as T

OK, ARG, NODEV = 0, 1, 4
NEW_ENTRIES = ["dsh_trackstate_set_embedding", "dsh_trackstate_clear_embedding", "dsh_trackstate_set_counters", "dsh_trackstate_get",
               "dsh_trackstate_seed_local_points", "dsh_trackstate_repose", "dsh_trackstate_cull", "dsh_track_close_frame"]

# the generated scenes the GPU tests run (tests/test_track_close_gpu.py), seeds picked so that every branch is exercised (checked below)
SCENES = {"p30": (3, dict(n_kf=6, n_kp=64)),                            # P about 30: one partial wavefront
          "p1050": (1, dict(n_kf=30, n_kp=300, obs_per_point=6)),       # P just above LM_CHUNK = 1024
          "default": (2, dict())}                                       # 30 keyframes x 1200 key points, 8 observations per point


def make_scene(name):
    from defslam_amd import synth
    seed, kw = SCENES[name]
    return synth.make_track_close_scene(seed, **kw)


# ---- the restatement on the hand-built map -------------------------------------------------------------------------------------------

def first_hand_frame(rm, only_tracking=False):
    fr = T.hand_frame()
    got = rm.update_local_map(T.HAND_FRAME_POINTS)
    assert got["local_points"].tolist() == T.HAND_FIRST_LIST and rm.reference_points == []
    rm.search_local_points(fr)
    rm.set_bad(3)                                                       # culled by the mapping thread meanwhile: nObs stays 2
    return rm.close_frame(fr, T.HAND_FRAME_POINTS, T.HAND_OUTLIER, T.HAND_NODES_AFTER, only_tracking)


def test_restatement_first_frame_of_the_hand_built_map():
    """Every branch of the loops once: held twice and inlier at both (found += 2, two votes for mnMatchesInliers), an outlier, an inlier
    without a facet (no DefnToMatchLOCAL), a bad point with a stale nObs (IncreaseFound and mnMatchesInliers, not observedFrame; it
    does not move), an inlier with nObs == 0 (IncreaseFound only, but it is observed), a query in view (visible += 1); the reference
    list is still empty."""
    rm = T.hand_map()
    assert first_hand_frame(rm) == T.HAND_COUNTS
    v, f, o, x = rm.track_state()
    assert v.tolist() == T.HAND_VISIBLE and f.tolist() == T.HAND_FOUND and o.tolist() == T.HAND_N_OBS
    assert x.tobytes() == T.HAND_XYZ_AFTER.tobytes()
    assert rm.points[3].bad and rm.points[3].n_obs == 2                        # the stale nObs


def test_restatement_only_tracking_counts_every_inlier():
    assert first_hand_frame(T.hand_map(), only_tracking=True) == T.HAND_COUNTS_ONLY_TRACKING


def test_restatement_second_frame_counts_against_the_previous_list_and_culls():
    rm = T.hand_map()
    first_hand_frame(rm)
    fr = T.hand_frame()
    rm.kfs[1].bad = True
    got = rm.update_local_map([0])
    assert got["local_points"].tolist() == T.HAND_SECOND_LIST and rm.reference_points == T.HAND_FIRST_LIST
    rm.search_local_points(fr)
    c = rm.close_frame(fr, [0], [0])                                    # no nodes: nothing moves
    assert c["local_map_points"] == T.HAND_SECOND_LOCAL_MAP_POINTS and c["n_moved"] == 0
    assert rm.left_out == dict(bad=1, no_facet=1, out_of_frustum=1)
    assert rm.frustum_count(T.R.ref_frame(fr), rm.local_points)[0] == T.HAND_SECOND_WRONG_LIST_COUNT
    assert rm.track_state()[3].tobytes() == T.HAND_XYZ_AFTER.tobytes()
    assert rm.track_state()[0].tolist() == [4, 2, 3, 2, 2, 2] and rm.track_state()[1].tolist() == [4, 1, 2, 2, 2, 1]
    rm.set_counters(1, 5, 1)
    assert rm.cull(range(6), T.HAND_FIRST_KF, T.HAND_CURRENT_KF).tolist() == T.HAND_ACTIONS
    assert [p.bad for p in rm.points] == [False, True, False, True, False, False] and rm.points[1].n_obs == 1


def test_restatement_seed_clear_embedding_and_erase():
    rm = T.hand_map(erased=False)
    assert rm.points[5].n_obs == 2
    rm.erase_observation(5, 0)
    rm.erase_observation(5, 0)                                          # a pair that is not there: no change
    assert rm.points[5].n_obs == 1
    rm.seed_local_points([0, 4, 5])
    assert rm.local_points == [0, 4, 5] and rm.reference_points == [0, 4, 5]
    fr = T.hand_frame()
    assert rm.close_frame(fr, [], [])["local_map_points"] == 3
    rm.clear_embedding()
    c = rm.close_frame(fr, [0], [0], T.HAND_NODES_AFTER)
    assert c["to_match_local"] == 0 and c["local_map_points"] == 0 and c["n_moved"] == 0 and c["matches_inliers"] == 1


# ---- the generator -------------------------------------------------------------------------------------------------------------------

def test_scene_generator_is_deterministic_and_extends_the_local_map_scene():
    from defslam_amd import synth
    kw = dict(n_kf=12, n_kp=100, obs_per_point=5)
    a, b, base = synth.make_track_close_scene(3, **kw), synth.make_track_close_scene(3, **kw), synth.make_local_map_scene(3, **kw)
    for k in ("xyz", "normal", "nodes", "bary", "late_bad", "visible", "found", "first_kf", "node_xyz", "final_points", "outlier", "frame_points"):
        np.testing.assert_array_equal(a[k], b[k])
    np.testing.assert_array_equal(a["frame_after"].Tcw, b["frame_after"].Tcw)
    for k in ("xyz", "max_distance", "desc", "bad", "tables", "parents", "kf_bad", "frame_points"):
        np.testing.assert_array_equal(a[k], base[k])
    has = a["nodes"][:, 0] >= 0
    assert has.any() and (~has).any() and (a["nodes"][~has] == -1).all()
    assert (np.diff(a["nodes"][has], axis=1) > 0).all() and a["nodes"].max() < a["node_xyz"].shape[0]
    np.testing.assert_allclose(a["bary"][has].sum(1), 1.0, atol=1e-12)
    # the embedding reproduces the points the scene drew from the template
    pos = (a["bary"][has][:, :, None] * a["template_xyz"][a["nodes"][has]]).sum(1)
    np.testing.assert_allclose(pos, a["xyz"][has], atol=1e-6)
    assert not np.array_equal(a["frame_after"].Tcw, a["frame"].Tcw) and 0 < np.abs(a["node_xyz"] - a["template_xyz"]).max() < 0.02
    assert (a["found"] <= a["visible"]).all() and a["found"].min() >= 1


@pytest.mark.parametrize("name", sorted(SCENES))
def test_generated_scenes_exercise_every_branch_on_the_restatement(name):
    """A condition on the inputs of the GPU tests, checked on the restatement alone."""
    sc = make_scene(name)
    rm = T.scene_to_ref(sc)
    found0 = rm.track_state()[1]
    c = T.run_generated_frame(rm, sc)
    assert all(c[k] > 0 for k in T.COUNT_NAMES if k != "n_moved"), c
    assert c["n_moved"] > 0 and c["matches_inliers"] != c["inliers"]
    assert 0 < c["local_map_points"] < len(rm.reference_points)
    assert all(v > 0 for v in rm.left_out.values()), rm.left_out
    assert (rm.track_state()[1] - found0).max() >= 2                    # held twice, inlier at both key points
    assert rm.reference_points != rm.local_points                      # the previous list is another one
    fp, out = sc["final_points"], sc["outlier"]
    held = fp[fp >= 0]
    assert sc["bad"][held].any() and (rm.track_state()[2][held] == 0).any() and (sc["nodes"][held, 0] < 0).any()
    ids, first_kf = T.cull_list(sc)
    assert sorted(set(rm.cull(ids, first_kf, sc["current_kf"]).tolist())) == [0, 1, 2, 3]


@pytest.mark.parametrize("name", ["default", "p1050"])
def test_generated_scenes_tell_the_previous_list_from_the_current_one(name):
    """Where the map has more keyframes than one local map holds, the previous frame's list is not the current one plus the points
    that became bad, and numberLocalMapPoints taken against the wrong list would be another number."""
    sc = make_scene(name)
    rm = T.scene_to_ref(sc)
    c = T.run_generated_frame(rm, sc)
    assert set(rm.reference_points) - set(rm.local_points) - set(sc["late_bad"].tolist())
    assert rm.frustum_count(T.R.ref_frame(sc["frame_after"]), rm.local_points)[0] != c["local_map_points"]


# ---- the ABI without a GPU -----------------------------------------------------------------------------------------------------------

def test_new_symbols_are_bound_and_outside_the_counted_prefixes():
    from defslam_amd import _lib, localmap
    L = _lib.load()
    for n in NEW_ENTRIES:
        assert n in _lib.EXPORTED_SYMBOLS and getattr(L, n).argtypes is not None, n
        assert not n.startswith("dsh_mpdb_") and not n.startswith("dsh_local_map_")
    assert len([n for n in _lib.EXPORTED_SYMBOLS if n.startswith("dsh_trackstate_")]) == 7
    assert C.sizeof(_lib.TrackCloseCountsC) == 32
    for m in ("set_embedding", "clear_embedding", "set_counters", "get_state", "seed_local_points", "repose", "cull", "close_frame"):
        assert callable(getattr(localmap.MapPointStore, m))
    assert [f for f in localmap.CloseCounts.__dataclass_fields__] == list(T.COUNT_NAMES)


def _entry_rows(keep):
    """(name, well-formed arguments, malformed arguments) after the store handle, for an EMPTY store (a host-only store stays empty)."""
    from test_track_search_cpu import hand_frame
    from defslam_amd import _lib
    f = hand_frame([[10, 10]], [0]).c(keep)
    nopose = hand_frame([[10, 10]], [0]).c(keep)
    nopose.Tcw = None
    a = dict(z=np.zeros(1, np.int32), n3=np.array([0, 1, 2], np.int32), b3=np.ones(3), x3=np.zeros(3), u1=np.zeros(1, np.uint8))
    keep.append(a)
    p = lambda x, t: x.ctypes.data_as(C.POINTER(t))
    zi, n3, b3, x3, u1 = p(a["z"], C.c_int32), p(a["n3"], C.c_int32), p(a["b3"], C.c_double), p(a["x3"], C.c_double), p(a["u1"], C.c_uint8)
    cc = _lib.TrackCloseCountsC()
    keep.append(cc)
    return [
        ("dsh_trackstate_set_embedding", (0, None, None, None), (1, zi, n3, b3)),                                   # id 0 outside
        ("dsh_trackstate_set_embedding", (0, None, None, None), (1, None, n3, b3)),                                 # NULL with n > 0
        ("dsh_trackstate_set_embedding", (0, None, None, None), (-1, None, None, None)),
        ("dsh_trackstate_clear_embedding", (), None),
        ("dsh_trackstate_set_counters", (0, None, None, None), (1, zi, zi, zi)),
        ("dsh_trackstate_set_counters", (0, None, None, None), (1, None, None, None)),
        ("dsh_trackstate_get", (0, None, None, None, None, None), (1, zi, None, None, None, None)),
        ("dsh_trackstate_get", (0, None, None, None, None, None), (1, None, None, None, None, None)),
        ("dsh_trackstate_seed_local_points", (0, None), (1, zi)),
        ("dsh_trackstate_seed_local_points", (0, None), (1, None)),
        ("dsh_trackstate_repose", (0, None, None), (-1, None, None)),
        ("dsh_trackstate_repose", (1, x3, None), (1, None, None)),                                                  # nodes NULL with n_nodes > 0
        ("dsh_trackstate_cull", (0, None, None, 3, None), (1, zi, zi, 3, u1)),
        ("dsh_trackstate_cull", (0, None, None, 3, None), (1, None, None, 3, None)),
        ("dsh_track_close_frame", (C.byref(f), 0, None, None, 0, None, 0, C.byref(cc)), (C.byref(f), 1, zi, u1, 0, None, 0, C.byref(cc))),   # id 0 outside
        ("dsh_track_close_frame", (C.byref(f), 0, None, None, 1, x3, 0, C.byref(cc)), (C.byref(f), 1, None, None, 0, None, 0, C.byref(cc))),  # NULL with N > 0
        ("dsh_track_close_frame", (C.byref(f), 0, None, None, 0, None, 1, C.byref(cc)), (None, 0, None, None, 0, None, 0, C.byref(cc))),      # frame NULL
        ("dsh_track_close_frame", (C.byref(f), 0, None, None, 0, None, 0, C.byref(cc)), (C.byref(nopose), 0, None, None, 0, None, 0, C.byref(cc))),
        ("dsh_track_close_frame", (C.byref(f), 0, None, None, 0, None, 0, C.byref(cc)), (C.byref(f), 0, None, None, 0, None, 0, None)),       # out NULL
    ]


def test_host_only_status_of_every_new_entry_point(host_ctx):
    """On a host-only context a malformed call is DSH_ERR_ARG with a message naming the entry, a well-formed one DSH_ERR_NO_DEVICE saying
    "host-only" -- arguments first, then the device; a NULL store is DSH_ERR_ARG."""
    from test_local_map_cpu import _raw_store
    L = host_ctx._L
    msg = lambda: L.dsh_last_error(host_ctx._h).decode()
    rc, h = _raw_store(L, host_ctx._h)
    assert rc == OK and h
    keep = []
    rows = _entry_rows(keep)
    assert {r[0] for r in rows} == set(NEW_ENTRIES)
    for name, good, bad in rows:
        fn = getattr(L, name)
        assert fn(h, *good) == NODEV, (name, msg())
        assert "host-only" in msg() and name in msg(), (name, msg())
        assert fn(None, *good) == ARG, (name, "NULL store")
        if bad is not None:
            assert fn(h, *bad) == ARG, (name, "malformed")
            assert name in msg(), (name, msg())
            assert fn(None, *bad) == ARG, (name, "NULL store")
    assert L.dsh_mpdb_point_count(h) == 0
    assert L.dsh_mpdb_destroy(h) == OK


def test_a_detached_store_refuses_every_new_entry():
    from defslam_amd import sft
    from test_local_map_cpu import _raw_store
    ctx = sft.Context(-1)
    L = ctx._L
    rc, h = _raw_store(L, ctx._h)
    assert rc == OK
    ctx.close()                                    # dsh_destroy detaches the store
    keep = []
    for name, good, bad in _entry_rows(keep):
        for args in (good, bad):
            if args is not None:
                assert getattr(L, name)(h, *args) == ARG, name
    assert L.dsh_mpdb_destroy(h) == OK
