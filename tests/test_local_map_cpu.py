"""CPU tests of the local map: the restatement (tests/local_map_ref.py) on hand-built maps with the expected lists written out, the
scene generator, and the ABI of the map point store without a GPU (host-only refusals, order of checks, lifetime, symbols)."""
import ctypes as C

import numpy as np
import pytest

import local_map_ref as LM

OK, ARG, NODEV = 0, 1, 4


def check_expected(got, want):
    assert got["local_kf"].tolist() == want["local_kf"]
    assert got["votes"].tolist() == want["votes"]
    assert got["n_voted"] == len(want["votes"])
    assert got["ref_kf"] == want["ref_kf"]
    assert got["local_points"].tolist() == want["local_points"]
    assert np.nonzero(got["frame_bad"])[0].tolist() == want["frame_bad"]


@pytest.mark.parametrize("name", sorted(LM.hand_maps()))
def test_restatement_on_hand_built_maps(name):
    """The parent break, a bad parent that is still appended, the > 80 stop (at the first test with 95 voted keyframes, and while
    expanding), a vote tie that goes to the lower slot, a point held twice that votes twice, all voted keyframes bad, an erased
    observation, a table ahead of the observations, bad points in the frame and in a table."""
    rm, frame_points, want = LM.hand_maps()[name]
    check_expected(rm.update_local_map(frame_points), want)


def test_restatement_no_votes_keeps_the_previous_list_and_rebuilds_the_points():
    """Tracking.cc:1534 returns before mvpLocalKeyFrames.clear(); UpdateLocalPoints runs regardless, on the old list and the new flags."""
    rm, frame_points, want = LM.hand_maps()["parent_break"]
    check_expected(rm.update_local_map(frame_points), want)
    rm.points[2].bad = True
    for fp in ([-1, -1, -1], [], [2]):            # nothing held; an empty frame; only a bad point held (it does not vote)
        got = rm.update_local_map(fp)
        assert got["local_kf"].tolist() == want["local_kf"] and got["ref_kf"] == -1 and got["n_voted"] == 0 and got["votes"].tolist() == []
        assert got["local_points"].tolist() == [0, 3, 4]
        assert got["frame_bad"].tolist() == [p == 2 for p in fp]


def test_restatement_skip_is_bad_or_held_by_the_frame():
    rm, _, _ = LM.hand_maps()["tie_and_twice"]
    rm.points[0].bad = True                       # bad after it got into a table: it is no local point at all
    rm.update_local_map([1, 2, 2, -1])
    ids, _, _, _, _, skip = rm.queries()
    assert ids.tolist() == [1, 2, 3] and skip.tolist() == [1, 1, 0]


def test_scene_generator_is_deterministic_and_has_what_it_promises():
    from defslam_amd import synth
    a = synth.make_local_map_scene(3, n_kf=40, n_kp=200, obs_per_point=6, n_frame_kp=500)
    b = synth.make_local_map_scene(3, n_kf=40, n_kp=200, obs_per_point=6, n_frame_kp=500)
    for k in ("xyz", "normal", "max_distance", "desc", "bad", "tables", "parents", "kf_bad", "obs_point", "obs_kf", "frame_points"):
        np.testing.assert_array_equal(a[k], b[k])
    P, n_kf = a["xyz"].shape[0], a["tables"].shape[0]
    assert a["tables"].shape == (40, 200) and a["tables"].max() < P and a["tables"].min() == -1
    # every observation is in the table of its keyframe; the last keyframe has a table and no observation yet
    for p, k in zip(a["obs_point"][:500], a["obs_kf"][:500]):
        assert p in a["tables"][k]
    assert (a["tables"][-1] >= 0).sum() > 0 and not (a["obs_kf"] == n_kf - 1).any()
    pairs = set(zip(a["obs_point"].tolist(), a["obs_kf"].tolist()))
    assert len(pairs) == a["obs_point"].shape[0]
    # a spanning tree with branches: parents precede, slot 0 is the root, some keyframe has two children
    assert a["parents"][0] == -1 and all(0 <= a["parents"][k] < k for k in range(1, n_kf))
    assert np.bincount(a["parents"][1:]).max() >= 2
    assert a["kf_bad"].any() and a["bad"].any()
    fp = a["frame_points"]
    held = fp[fp >= 0]
    assert held.shape[0] > 20 and np.unique(held).shape[0] < held.shape[0] and a["bad"][held].any()
    np.testing.assert_array_equal(a["frame"].state, (fp >= 0).astype(np.uint8))


def scene_to_ref(sc):
    """A make_local_map_scene dict as a RefMap."""
    rm = LM.RefMap()
    for p in range(sc["xyz"].shape[0]):
        rm.add_point(sc["xyz"][p], sc["normal"][p], sc["max_distance"][p], sc["desc"][p], sc["bad"][p])
    for k in range(sc["tables"].shape[0]):
        rm.add_keyframe(sc["tables"][k], sc["parents"][k], sc["kf_bad"][k])
    for p, k in zip(sc["obs_point"].tolist(), sc["obs_kf"].tolist()):
        assert rm.add_observation(p, k)
    return rm


def test_restatement_on_a_generated_scene_is_consistent():
    from defslam_amd import synth
    sc = synth.make_local_map_scene(1, n_kf=30, n_kp=300, obs_per_point=6, n_frame_kp=600)
    rm = scene_to_ref(sc)
    got = rm.update_local_map(sc["frame_points"])
    assert got["n_voted"] > 3 and got["ref_kf"] >= 0 and not sc["kf_bad"][got["ref_kf"]]
    assert len(set(got["local_kf"].tolist())) == len(got["local_kf"])
    assert got["frame_bad"].sum() > 0 and got["votes"].sum() > 0
    # the votes are the observations of the held good points, with multiplicity
    fp = sc["frame_points"]
    mult = np.bincount(fp[(fp >= 0) & ~sc["bad"][np.maximum(fp, 0)]], minlength=sc["xyz"].shape[0])
    v = np.zeros(sc["tables"].shape[0], np.int64)
    np.add.at(v, sc["obs_kf"], mult[sc["obs_point"]])
    voted = [k for k in range(v.shape[0]) if v[k] > 0 and not sc["kf_bad"][k]]
    assert got["local_kf"][:got["n_voted"]].tolist() == voted and got["votes"].tolist() == v[voted].tolist()
    assert np.all(np.diff(got["local_points"]) > 0) and not sc["bad"][got["local_points"]].any()


# ---- the ABI without a GPU -------------------------------------------------------------------------------------------------------

def test_new_symbols_are_bound():
    from defslam_amd import _lib, localmap
    L = _lib.load()
    names = [n for n in _lib.EXPORTED_SYMBOLS if n.startswith("dsh_mpdb_") or n.startswith("dsh_local_map_")]
    assert len(names) == 17
    for n in names:
        assert getattr(L, n).argtypes is not None, n
    assert localmap.MapPointStore and localmap.POSITION == 1 and localmap.NORMAL_DEPTH == 2 and localmap.DESCRIPTOR == 4


def _raw_store(L, ctx_h, points=8, keyframes=4, observations=16):
    from defslam_amd import _lib
    d = _lib.MpdbDescC(ctx_h, points, keyframes, observations)
    h = C.c_void_p()
    return L.dsh_mpdb_create(C.byref(d), C.byref(h)), h


def _entry_rows(keep):
    """(name, well-formed arguments, malformed arguments) after the store handle, for an EMPTY store.  A host-only store stays empty
    (every mutation is refused), so an entry that names an existing keyframe has no well-formed call there: None."""
    from test_track_search_cpu import hand_frame
    f = hand_frame([[10, 10]], [0]).c(keep)
    i32 = lambda *v: np.array(v, np.int32)
    a = dict(z=i32(0), f3=np.zeros(3, np.float32), f1=np.zeros(1, np.float32), d=np.zeros(32, np.uint8))
    keep.append(a)
    p = lambda x, t: x.ctypes.data_as(C.POINTER(t))
    zi, f3, f1, d = p(a["z"], C.c_int32), p(a["f3"], C.c_float), p(a["f1"], C.c_float), p(a["d"], C.c_uint8)
    return [
        ("dsh_mpdb_add_points", (0, None, None, None, None, None, None), (1, None, f3, f1, d, None, None)),                 # xyz NULL with n > 0
        ("dsh_mpdb_update_points", (0, None, 1, None, None, None, None), (1, zi, 1, f3, None, None, None)),                 # id 0 outside
        ("dsh_mpdb_update_points", (0, None, 7, None, None, None, None), (0, None, 0, None, None, None, None)),             # empty mask
        ("dsh_mpdb_set_points_bad", (0, None, None), (1, zi, None)),                                                        # id 0 outside
        ("dsh_mpdb_add_observations", (0, None, None), (1, zi, zi)),                                                        # outside
        ("dsh_mpdb_add_observations", (0, None, None), (1, None, zi)),                                                      # NULL with n > 0
        ("dsh_mpdb_erase_observations", (0, None, None), (1, zi, zi)),
        ("dsh_mpdb_add_keyframe", (0, None, -1, 0, None), (0, None, 0, 0, None)),                                           # parent outside
        ("dsh_mpdb_add_keyframe", (0, None, -1, 0, None), (1, None, -1, 0, None)),                                          # table NULL
        ("dsh_mpdb_add_keyframe", (0, None, -1, 0, None), (1, zi, -1, 0, None)),                                            # table entry outside
        ("dsh_mpdb_set_keyframe_point", None, (0, 0, -1)),
        ("dsh_mpdb_set_keyframe_parent", None, (0, -1)),
        ("dsh_mpdb_set_keyframe_bad", None, (0, 1)),
        ("dsh_local_map_update", (0, None, None, 0, None, None, None, None, None, None), (1, None, None, 0, None, None, None, None, None, None)),
        ("dsh_local_map_update", (0, None, None, 0, None, None, None, None, None, None), (1, zi, None, 0, None, None, None, None, None, None)),
        ("dsh_local_map_points", (0, None, None), (-1, None, None)),
        ("dsh_local_map_search", (C.byref(f), 3.0, 0, None, None, None, None, None, None, None),
         (C.byref(f), 0.0, 0, None, None, None, None, None, None, None)),                                                    # th
        ("dsh_local_map_search", (C.byref(f), 3.0, 0, None, None, None, None, None, None, None),
         (None, 3.0, 0, None, None, None, None, None, None, None)),                                                          # frame NULL
    ]


def test_host_only_status_of_every_new_entry_point(host_ctx):
    """The discipline of test_abi_and_host's table for the entries that take the store alone: on a host-only context a malformed call
    is DSH_ERR_ARG with a message, a well-formed one DSH_ERR_NO_DEVICE saying "host-only" -- arguments first, then the device."""
    from defslam_amd import _lib
    L = host_ctx._L
    msg = lambda: L.dsh_last_error(host_ctx._h).decode()
    # the life cycle works without a device: the store holds no arrays there
    d = _lib.MpdbDescC(host_ctx._h, 0, 4, 16)
    h = C.c_void_p()
    assert L.dsh_mpdb_create(C.byref(d), C.byref(h)) == ARG and "dsh_mpdb_create" in msg() and not h
    assert L.dsh_mpdb_create(None, C.byref(h)) == ARG
    d_null = _lib.MpdbDescC(None, 8, 4, 16)
    assert L.dsh_mpdb_create(C.byref(d_null), C.byref(h)) == ARG
    rc, h = _raw_store(L, host_ctx._h)
    assert rc == OK and h
    assert L.dsh_mpdb_point_count(h) == 0 and L.dsh_mpdb_keyframe_count(h) == 0
    assert L.dsh_mpdb_point_count(None) == -1 and L.dsh_mpdb_keyframe_count(None) == -1
    assert L.dsh_mpdb_clear(h) == OK and L.dsh_mpdb_clear(None) == ARG
    keep = []
    rows = _entry_rows(keep)
    covered = {r[0] for r in rows} | {"dsh_mpdb_create", "dsh_mpdb_destroy", "dsh_mpdb_clear", "dsh_mpdb_point_count", "dsh_mpdb_keyframe_count"}
    assert covered == {n for n in _lib.EXPORTED_SYMBOLS if n.startswith("dsh_mpdb_") or n.startswith("dsh_local_map_")}
    for name, good, bad in rows:
        fn = getattr(L, name)
        if good is not None:
            assert fn(h, *good) == NODEV, (name, msg())
            assert "host-only" in msg() and name in msg(), (name, msg())
        assert fn(h, *bad) == ARG, (name, "malformed")
        assert name in msg(), (name, msg())
        assert fn(None, *bad) == ARG, (name, "NULL store")
    assert L.dsh_mpdb_point_count(h) == 0 and L.dsh_mpdb_keyframe_count(h) == 0        # nothing was stored
    assert L.dsh_mpdb_destroy(h) == OK and L.dsh_mpdb_destroy(None) == ARG


@pytest.mark.parametrize("store_first", [True, False])
def test_lifetime_destroy_in_either_order_and_a_detached_store_refuses(store_first):
    from defslam_amd import sft
    ctx = sft.Context(-1)
    L = ctx._L
    rc, h = _raw_store(L, ctx._h)
    assert rc == OK
    if store_first:
        assert L.dsh_mpdb_destroy(h) == OK
        ctx.close()
        return
    ctx.close()                                    # dsh_destroy detaches the store
    keep = []
    for name, good, bad in _entry_rows(keep):
        for args in (good, bad):
            if args is not None:
                assert getattr(L, name)(h, *args) == ARG, name
    assert L.dsh_mpdb_clear(h) == ARG
    assert L.dsh_mpdb_point_count(h) == 0
    assert L.dsh_mpdb_destroy(h) == OK
