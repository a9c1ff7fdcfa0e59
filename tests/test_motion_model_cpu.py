"""CPU tests of the end of a frame and the motion-model search on the map point store: the restatement (tests/motion_model_ref.py) on a
hand-built case with the expected numbers written out, its agreement with tests/track_search_ref.py where the two searches must agree,
the retry boundary, and the ABI of dsh_track_end_frame / dsh_track_last_frame / dsh_motion_model_search without a GPU (symbols, every
host-only refusal and its order, a detached store)."""
import ctypes as C

import numpy as np
import pytest

import motion_model_ref as M
import track_search_ref as R

OK, ARG, NODEV = 0, 1, 4
NEW_ENTRIES = ["dsh_track_end_frame", "dsh_track_last_frame", "dsh_motion_model_search"]
LENGTHS = [1, 63, 64, 65, 130, 1025]                 # last-frame lengths of the GPU tests: lane, wavefront and workgroup boundaries of the gather
SCENE = (4, dict(n_kf=12, n_kp=200, obs_per_point=6, n_frame_kp=300))   # about 300 key points on the default 64 x 48 grid


def make_scene():
    from defslam_amd import synth
    seed, kw = SCENE
    return synth.make_track_close_scene(seed, **kw)


# ---- the restatement on the hand-built case ----------------------------------------------------------------------------------------------

def hand_after_end_frame():
    rm = M.hand_map()
    e = rm.end_frame(M.HAND_LAST_POINTS, M.HAND_LAST_OUTLIER, M.HAND_LAST_OCTAVE)
    return rm, e


def test_restatement_end_frame_of_the_hand_built_case():
    """CleanMatches empties the entry of the point nobody observes and clears its flag, the outputs keep the outlier with its point, the
    drop removes it from the list and leaves its flag, and the list carries -1 for the octave of an empty entry."""
    rm, e = hand_after_end_frame()
    assert e["points"].tolist() == M.HAND_END["points"] and e["outlier"].astype(int).tolist() == M.HAND_END["outlier"]
    assert (e["cleaned"], e["dropped"], e["kept"]) == (M.HAND_END["cleaned"], M.HAND_END["dropped"], M.HAND_END["kept"])
    ids, oc = rm.last_frame()
    assert ids.tolist() == M.HAND_LIST[0] and oc.tolist() == M.HAND_LIST[1]
    assert rm.last_outlier[6] and rm.last_points[6] == -1                # the dropped outlier keeps its flag


def test_restatement_clean_matches_reads_the_stale_n_obs():
    """A bad point keeps nObs, so CleanMatches leaves its entry (there is no isBad test); the search skips it later."""
    rm = M.hand_map()
    rm.set_bad(1)
    e = rm.end_frame(M.HAND_LAST_POINTS, M.HAND_LAST_OUTLIER, M.HAND_LAST_OCTAVE)
    assert e["points"][1] == 1 and rm.last_points[1] == 1
    r = rm.motion_model_search(M.hand_frame(), min_matches=0)
    assert r["match"][1] == -1 and 1 not in r["frame_points"].tolist()


def test_restatement_a_query_without_observations_does_not_block_its_key_point():
    rm, _ = hand_after_end_frame()
    fr = M.hand_frame()
    r = rm.motion_model_search(fr, min_matches=2)
    assert r["frame_points"].tolist() == M.HAND_BLOCKING_FRAME_POINTS and r["match"].tolist() == M.HAND_BLOCKING_MATCH
    assert r["nmatches"] == M.HAND_BLOCKING_NMATCHES and r["th_used"] == 20.0
    rm.erase_observation(0, 0)                                           # n_obs == 0 and not bad: unreachable through the reference's erase rule
    rm.set_bad(3)
    assert rm.points[0].n_obs == 0
    r = rm.motion_model_search(fr, min_matches=2)
    assert r["frame_points"].tolist() == M.HAND_FRAME_POINTS and r["match"].tolist() == M.HAND_MATCH
    assert r["nmatches"] == M.HAND_NMATCHES == 1 + sum(p >= 0 for p in M.HAND_FRAME_POINTS) and r["th_used"] == 20.0
    r = rm.motion_model_search(fr)                                       # 3 < 20: the wide search; the same matches here
    assert r["match"].tolist() == M.HAND_MATCH and r["th_used"] == 25.0 and not r["ok"]
    ids, _ = rm.last_frame()
    assert ids.tolist() == M.HAND_LIST[0]                                # a search does not change the list


def test_restatement_empty_and_missing_last_frame():
    rm = M.hand_map()
    assert rm.last_points is None
    rm.end_frame([], [], [])
    r = rm.motion_model_search(M.hand_frame())
    assert r["nmatches"] == 0 and r["th_used"] == 25.0 and r["match"].shape == (0,) and r["frame_points"].tolist() == [-1, -1, -1]
    assert rm.motion_model_search(M.hand_frame(), min_matches=0)["th_used"] == 20.0


# ---- generated scenes --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [65, 130, 1025])
def test_restatement_agrees_with_the_packed_search_when_every_query_has_observations(L):
    """After end_frame every kept entry has n_obs >= 1, so DefORBmatcher's copy and ORBmatcher::SearchByProjection agree (no key point
    enters with a map point): the same queries through track_search_ref.motion_model give the same matches, count and th."""
    sc = make_scene()
    rm = M.scene_to_ref(sc)
    e = rm.end_frame(*M.make_last_frame(sc, L))
    idx, xyz, octave, desc = rm.last_frame_queries()
    assert all(rm.points[rm.last_points[i]].n_obs > 0 for i in idx) and 0 < len(idx) <= e["kept"]
    if L >= 130:
        assert e["cleaned"] > 0 and len(idx) < e["kept"]              # CleanMatches had work, and so has the search's own filter
    r = rm.motion_model_search(sc["frame"])
    m, n, th, st = R.motion_model(sc["frame"], xyz, octave, desc)
    np.testing.assert_array_equal(r["match"][idx], m)
    assert r["nmatches"] == n and r["th_used"] == th
    assert (np.delete(r["match"], idx) == -1).all()
    np.testing.assert_array_equal(r["frame_points"] >= 0, st == 1)


def test_generated_last_frames_exercise_every_filter():
    """A condition on the inputs of the GPU tests, checked on the restatement alone."""
    sc = make_scene()
    rm = M.scene_to_ref(sc)
    pts, out, octs = M.make_last_frame(sc, 1025)
    e = rm.end_frame(pts, out, octs)
    assert e["cleaned"] > 0 and e["dropped"] > 0 and (pts < 0).any()
    kept = [p for p in rm.last_points if p >= 0]
    assert any(rm.points[p].bad for p in kept) and any(rm.nodes[p] is None for p in kept)
    r = rm.motion_model_search(sc["frame"])
    assert r["nmatches"] >= 30 and r["th_used"] == 20.0
    assert M.make_last_frame(sc, 1)[0][0] >= 0


def test_retry_boundary_on_the_restatement():
    """19 narrow matches: the result is the fresh search at th_wide; 20: the narrow result stays."""
    sc = make_scene()
    for target, used in ((19, 25.0), (20, 20.0)):
        rm = M.scene_to_ref(sc)
        rm.end_frame(*M.make_last_frame(sc, 130))
        assert M.trim_to_narrow_count(rm, sc["frame"], target)
        fr = R.ref_frame(sc["frame"])
        assert rm.search_by_projection(fr, 20)[2] == target
        r = rm.motion_model_search(sc["frame"])
        assert r["th_used"] == used
        fp, match, n = rm.search_by_projection(fr, used)
        assert r["nmatches"] == n and r["match"].tolist() == match.tolist() and r["frame_points"].tolist() == fp.tolist()


# ---- the ABI without a GPU ---------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_bound_declared_and_wrapped():
    import os
    from defslam_amd import _lib, localmap
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "defslam_hip.h")).read()
    for n in NEW_ENTRIES:
        assert n in _lib.EXPORTED_SYMBOLS and getattr(L, n).argtypes is not None, n
        assert f"int {n}(dsh_mpdb* db" in header, n
    assert "} dsh_track_end_counts;" in header and C.sizeof(_lib.TrackEndCountsC) == 12
    for m in ("end_frame", "motion_model_search", "last_frame"):
        assert callable(getattr(localmap.MapPointStore, m))
    assert list(localmap.EndFrame.__dataclass_fields__) == ["points", "outlier", "cleaned", "dropped", "kept"]
    assert list(localmap.MotionModelSearch.__dataclass_fields__) == ["frame_points", "match", "nmatches", "th_used", "ok"]


def _rows(keep):
    """(name, arguments after the store handle, expected status, a word of the message) for an EMPTY store on a host-only context."""
    from defslam_amd import _lib
    f = M.hand_frame().c(keep)

    def frame(**kw):
        g = M.hand_frame().c(keep)
        for k, v in kw.items():
            setattr(g, k, v)
        return C.byref(g)

    a = dict(z=np.zeros(4, np.int32), m1=np.full(4, -1, np.int32), o128=np.full(1, 128, np.int32), om=np.full(1, -1, np.int32), u=np.zeros(4, np.uint8),
             fl=np.zeros(1, np.float32), m2=np.array([-1, -2], np.int32))
    keep.append(a)
    p = lambda x, t: x.ctypes.data_as(C.POINTER(t))
    z, m1, o128, om, u = p(a["z"], C.c_int32), p(a["m1"], C.c_int32), p(a["o128"], C.c_int32), p(a["om"], C.c_int32), p(a["u"], C.c_uint8)
    m2 = p(a["m2"], C.c_int32)
    cc = _lib.TrackEndCountsC()
    keep.append(cc)
    nan, inf = float("nan"), float("inf")
    end, last, mm = "dsh_track_end_frame", "dsh_track_last_frame", "dsh_motion_model_search"
    return [
        (end, (0, None, None, None, None, None, None), NODEV, "host-only"),
        (end, (1, m1, u, z, m1, u, C.byref(cc)), NODEV, "host-only"),
        (end, (1, z, u, z, None, None, None), ARG, "frame_points[0]"),                     # id 0 outside the empty store
        (end, (2, m2, u, z, None, None, None), ARG, "frame_points[1]"),                    # neither -1 nor an id
        (end, (-1, None, None, None, None, None, None), ARG, "N outside"),
        (end, (8193, m1, u, z, None, None, None), ARG, "N outside"),
        (end, (1, m1, u, o128, None, None, None), ARG, "octave[0]"),
        (end, (1, m1, u, om, None, None, None), ARG, "octave[0]"),
        (end, (1, None, u, z, None, None, None), ARG, "NULL"),
        (end, (1, m1, None, z, None, None, None), ARG, "NULL"),
        (end, (1, m1, u, None, None, None, None), ARG, "NULL"),
        (last, (0, None, None, None), NODEV, "host-only"),
        (last, (-1, None, None, None), ARG, "capacity"),
        (mm, (C.byref(f), 20.0, 25.0, 20, z, None, None, None), NODEV, "host-only"),
        (mm, (C.byref(f), 20.0, 25.0, 0, z, z, z, p(a["fl"], C.c_float)), NODEV, "host-only"),
        (mm, (frame(state=None), 20.0, 25.0, 20, z, None, None, None), NODEV, "host-only"),     # state is not read
        (mm, (None, 20.0, 25.0, 20, z, None, None, None), ARG, "frame is NULL"),
        (mm, (frame(N=-1), 20.0, 25.0, 20, z, None, None, None), ARG, "N outside"),
        (mm, (frame(N=8193), 20.0, 25.0, 20, z, None, None, None), ARG, "N outside"),
        (mm, (frame(Tcw=None), 20.0, 25.0, 20, z, None, None, None), ARG, "Tcw"),
        (mm, (frame(grid_cols=200, grid_rows=200), 20.0, 25.0, 20, z, None, None, None), ARG, "grid"),
        (mm, (frame(levels=33), 20.0, 25.0, 20, z, None, None, None), ARG, "levels"),
        (mm, (frame(kp=None), 20.0, 25.0, 20, z, None, None, None), ARG, "key point arrays"),
        (mm, (C.byref(f), 0.0, 25.0, 20, z, None, None, None), ARG, "positive finite"),
        (mm, (C.byref(f), nan, 25.0, 20, z, None, None, None), ARG, "positive finite"),
        (mm, (C.byref(f), 20.0, -1.0, 20, z, None, None, None), ARG, "positive finite"),
        (mm, (C.byref(f), 20.0, inf, 20, z, None, None, None), ARG, "positive finite"),
        (mm, (C.byref(f), 20.0, 25.0, -1, z, None, None, None), ARG, "min_matches"),
        (mm, (C.byref(f), 20.0, 25.0, 20, None, None, None, None), ARG, "frame_points is NULL"),
    ]


def test_host_only_status_of_every_refusal(host_ctx):
    """On a host-only context a malformed call is DSH_ERR_ARG with a message naming the entry point and the entry, a well-formed one
    DSH_ERR_NO_DEVICE saying "host-only" -- arguments first, then the device; a NULL store is DSH_ERR_ARG."""
    from test_local_map_cpu import _raw_store
    L = host_ctx._L
    msg = lambda: L.dsh_last_error(host_ctx._h).decode()
    rc, h = _raw_store(L, host_ctx._h)
    assert rc == OK and h
    keep = []
    rows = _rows(keep)
    assert {r[0] for r in rows} == set(NEW_ENTRIES)
    for name, args, want, word in rows:
        fn = getattr(L, name)
        assert fn(h, *args) == want, (name, args, msg())
        assert name in msg() and word in msg(), (name, word, msg())
        assert fn(None, *args) == ARG, (name, "NULL store")
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
    for name, args, _, _ in _rows(keep):
        assert getattr(L, name)(h, *args) == ARG, name
    assert L.dsh_mpdb_destroy(h) == OK
