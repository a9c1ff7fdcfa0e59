"""CPU tests of the erase on the resident map point store (dsh_point_store_erase_observations, dsh_point_store_set_bad,
dsh_point_store_cull, dsh_point_store_get_observations, dsh_point_store_get_keyframe_table): the binding, every refusal an empty store
on a host-only context can reach, and the restatement tests/point_erase_ref.py against hand-written cases.  Every value is exact."""
import ctypes as C
import os

import numpy as np

import point_erase_ref as PE
import track_close_ref as T

OK, ARG, STATE, NODEV = 0, 1, 3, 4
NEW_ENTRIES = ("dsh_point_store_erase_observations", "dsh_point_store_set_bad", "dsh_point_store_cull", "dsh_point_store_get_observations",
               "dsh_point_store_get_keyframe_table")


def test_new_symbols_are_declared_exported_and_bound():
    from defslam_amd import _lib, localmap
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "defslam_hip.h")).read()
    for n in NEW_ENTRIES:
        assert n in _lib.EXPORTED_SYMBOLS and getattr(L, n).argtypes is not None, n
        assert f"int {n}(dsh_mpdb* db" in header, n
    assert "} dsh_point_erase_counts;" in header and C.sizeof(_lib.PointEraseCountsC) == 20
    assert [f for f, _ in _lib.PointEraseCountsC._fields_] == list(PE.COUNT_NAMES) == list(localmap.EraseCounts.__dataclass_fields__)
    for m in ("erase_observations_full", "set_bad_full", "cull_full", "observations", "keyframe_table"):
        assert callable(getattr(localmap.MapPointStore, m))
    assert (localmap.ERASE_NOT_STORED, localmap.ERASE_DONE, localmap.ERASE_SET_BAD) == (0, 1, 2)
    # the old entry points stay and point to the new ones
    for n in ("dsh_mpdb_erase_observations", "dsh_mpdb_set_points_bad", "dsh_trackstate_cull"):
        assert n in _lib.EXPORTED_SYMBOLS


def _rows(keep):
    """(entry, arguments after the store handle, part of the message, the counts struct or None) for an EMPTY store: each row is
    well-formed up to the argument it names."""
    from defslam_amd import _lib
    i32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    u8p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    one, two, rep, neg = np.zeros(1, np.int32), np.array([0, 1], np.int32), np.array([3, 5, 3], np.int32), np.array([-1], np.int32)
    act, ptr, tot = np.zeros(4, np.uint8), np.zeros(4, np.int32), np.zeros(1, np.int32)
    keep += [one, two, rep, neg, act, ptr, tot]
    cc = _lib.PointEraseCountsC(7, 7, 7, 7, 7)
    keep.append(cc)
    c = C.byref(cc)
    E, S, U, G, K = NEW_ENTRIES
    return cc, [
        (E, (0, None, None, 0, None, None), "out is NULL"),
        (E, (-1, None, None, 0, None, c), "n < 0"),
        (E, (1, None, i32p(one), 0, None, c), "point id array is NULL"),
        (E, (1, i32p(one), None, 0, None, c), "keyframe_slots is NULL"),
        (E, (3, i32p(rep), i32p(rep), 1, None, c), "point id 3 repeated in the batch"),
        (E, (1, i32p(one), i32p(one), 0, None, c), "point id 0 outside the store"),
        (E, (1, i32p(neg), i32p(one), 0, None, c), "point id -1 outside the store"),
        (S, (0, None, None), "out is NULL"),
        (S, (-1, None, c), "n < 0"),
        (S, (2, None, c), "point id array is NULL"),
        (S, (3, i32p(rep), c), "point id 3 repeated in the batch"),
        (S, (2, i32p(two), c), "point id 0 outside the store"),
        (U, (0, None, None, 0, None, None), "out is NULL"),
        (U, (-1, None, None, 0, None, c), "n < 0"),
        (U, (1, None, i32p(one), 3, u8p(act), c), "point id array is NULL"),
        (U, (3, i32p(rep), i32p(rep), 3, u8p(act), c), "point id 3 repeated in the batch"),
        (U, (1, i32p(one), i32p(one), 3, u8p(act), c), "point id 0 outside the store"),
        (G, (-1, None, i32p(ptr), 4, i32p(ptr), i32p(ptr), i32p(tot)), "n < 0"),
        (G, (1, None, i32p(ptr), 4, i32p(ptr), i32p(ptr), i32p(tot)), "point id array is NULL"),
        (G, (3, i32p(rep), i32p(ptr), 4, i32p(ptr), i32p(ptr), i32p(tot)), "point id 3 repeated in the batch"),
        (G, (1, i32p(one), i32p(ptr), 4, i32p(ptr), i32p(ptr), i32p(tot)), "point id 0 outside the store"),
        (G, (0, None, None, 4, i32p(ptr), i32p(ptr), i32p(tot)), "obs_ptr or n_total is NULL"),
        (G, (0, None, i32p(ptr), 4, i32p(ptr), i32p(ptr), None), "obs_ptr or n_total is NULL"),
        (G, (0, None, i32p(ptr), -1, i32p(ptr), i32p(ptr), i32p(tot)), "capacity < 0"),
        (G, (0, None, i32p(ptr), 4, None, i32p(ptr), i32p(tot)), "slots or idx is NULL"),
        (K, (0, 4, i32p(ptr)), "slot outside the store"),
        (K, (-1, 4, i32p(ptr)), "slot outside the store"),
    ]


def test_refusals_on_a_host_only_context_leave_the_counts_unwritten(host_ctx):
    """Arguments first: DSH_ERR_ARG with a message that names the entry and the counts as the caller left them; valid arguments reach the
    device gate and get DSH_ERR_NO_DEVICE, the counts still unwritten."""
    from defslam_amd import _lib
    from test_local_map_cpu import _raw_store
    L = host_ctx._L
    msg = lambda: L.dsh_last_error(host_ctx._h).decode()
    rc, h = _raw_store(L, host_ctx._h)
    assert rc == OK and h
    keep = []
    cc, rows = _rows(keep)
    assert {r[0] for r in rows} == set(NEW_ENTRIES)
    for name, args, part in rows:
        assert getattr(L, name)(h, *args) == ARG, (name, part)
        assert name in msg() and part in msg(), (name, part, msg())
        assert getattr(L, name)(None, *args) == ARG, (name, "NULL store")
        assert [getattr(cc, f) for f in PE.COUNT_NAMES] == [7] * 5, (name, part)
    c = C.byref(cc)
    ptr, tot = np.zeros(1, np.int32), np.full(1, 9, np.int32)
    i32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.dsh_point_store_erase_observations(h, 0, None, None, 1, None, c) == NODEV and "host-only" in msg()
    assert L.dsh_point_store_set_bad(h, 0, None, c) == NODEV
    assert L.dsh_point_store_cull(h, 0, None, None, 5, None, c) == NODEV
    assert L.dsh_point_store_get_observations(h, 0, None, i32p(ptr), 0, None, None, i32p(tot)) == NODEV and tot[0] == 9
    assert [getattr(cc, f) for f in PE.COUNT_NAMES] == [7] * 5
    assert L.dsh_mpdb_destroy(h) == OK


def test_a_detached_store_refuses_every_entry():
    from defslam_amd import _lib, sft
    from test_local_map_cpu import _raw_store
    ctx = sft.Context(-1)
    L = ctx._L
    rc, h = _raw_store(L, ctx._h)
    assert rc == OK
    ctx.close()
    cc = _lib.PointEraseCountsC()
    ptr = np.zeros(2, np.int32)
    p = ptr.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.dsh_point_store_erase_observations(h, 0, None, None, 0, None, C.byref(cc)) == ARG
    assert L.dsh_point_store_set_bad(h, 0, None, C.byref(cc)) == ARG
    assert L.dsh_point_store_cull(h, 0, None, None, 0, None, C.byref(cc)) == ARG
    assert L.dsh_point_store_get_observations(h, 0, None, p, 0, None, None, p) == ARG
    assert L.dsh_point_store_get_keyframe_table(h, 0, 0, None) == ARG
    assert L.dsh_mpdb_destroy(h) == OK


# ---- the restatement against hand-written cases ----------------------------------------------------------------------------------------------

def _four_obs_point(ref):
    rm = PE.EraseRefMap()
    for _ in range(5):
        rm.add_keyframe([-1] * 4)
    p = rm.add_point(ref=ref)
    for kf in (3, 1, 4, 2):                                           # arrival order is not slot order
        rm.kfs[kf].table[kf % 4] = p
        rm.add_observation(p, kf, kf % 4)
    return rm, p


def test_erasing_the_reference_keyframe_of_a_four_observation_point_moves_it_to_the_lowest_remaining_slot():
    rm, p = _four_obs_point(ref=3)
    status, c = rm.erase_observations([p], [3])
    mp = rm.points[p]
    assert status.tolist() == [1] and mp.ref == 1 and mp.n_obs == 3 and not mp.bad
    assert dict(rm.observations(p)) == {1: 1, 2: 2, 4: 0}
    assert c == dict(n_found=1, n_ref_moved=1, n_set_bad=0, n_records=1, n_entries=0)
    assert rm.kfs[3].table[3] == p                           # EraseObservation alone leaves the keyframe's table
    # erasing a keyframe that is not the reference leaves it
    rm, p = _four_obs_point(ref=3)
    status, c = rm.erase_observations([p], [1], erase_match=True)
    assert status.tolist() == [1] and rm.points[p].ref == 3 and c["n_ref_moved"] == 0 and c["n_entries"] == 1
    assert rm.kfs[1].table[1] == -1


def test_three_to_two_observations_cascades_and_leaves_n_obs_at_two():
    rm, p = _four_obs_point(ref=2)
    rm.erase_observations([p], [4])
    status, c = rm.erase_observations([p], [2])
    mp = rm.points[p]
    assert status.tolist() == [2] and mp.bad and mp.n_obs == 2 and dict(rm.observations(p)) == {}
    assert mp.ref == 1                                          # moved before the cascade, on the records the cascade removed
    assert c == dict(n_found=1, n_ref_moved=1, n_set_bad=1, n_records=3, n_entries=2)
    assert [rm.kfs[kf].table[kf % 4] for kf in (1, 2, 3, 4)] == [-1, p, -1, p]   # the cascade's entries; the pairs' own stay
    # the only observation: the reference keyframe stays where the reference would read end()
    rm = PE.EraseRefMap()
    rm.add_keyframe([0])
    rm.add_point(ref=0)
    rm.add_observation(0, 0, 0)
    status, c = rm.erase_observations([0], [0])
    assert status.tolist() == [2] and rm.points[0].ref == 0 and rm.points[0].n_obs == 0 and c["n_ref_moved"] == 0


def test_a_pair_that_is_not_stored_changes_nothing():
    rm, p = _four_obs_point(ref=3)
    before = rm.state()
    status, c = rm.erase_observations([p], [0], erase_match=True)
    assert status.tolist() == [0] and c == PE.zero_counts()
    after = rm.state()
    assert all(np.array_equal(before[n], after[n]) for n in ("bad", "n_obs", "ref")) and before["obs"] == after["obs"] and before["tables"] == after["tables"]


def test_the_small_scene_is_what_its_docstring_says():
    rm, (pts, slots) = PE.small_scene()
    assert len(rm.kfs) == 3 and all(len(kf.table) == 8 for kf in rm.kfs) and len(rm.points) == 6
    status, c = rm.erase_observations(pts, slots, erase_match=True)
    s = rm.state()
    assert status.tolist() == [2, 2, 2, 2, 2, 0]
    assert s["ref"].tolist() == [1, 2, 2, 1, 0, 0] and s["n_obs"].tolist() == [2, 2, 0, 2, 2, 2] and s["bad"].tolist() == [True] * 5 + [False]
    assert s["obs"][:5] == [{}] * 5 and s["obs"][5] == {0: 6, 1: 6}
    assert s["tables"][1][5] == -1 and s["tables"][0][3] == -1 and s["tables"][0][4] == -1
    assert c == dict(n_found=5, n_ref_moved=2, n_set_bad=5, n_records=13, n_entries=13)
    rm2, _ = PE.small_scene()
    rm2.erase_observations(pts, slots, erase_match=False)
    assert rm2.state()["tables"][0][3] == 4                            # kept without erase_match


def test_cull_decisions_equal_track_close_ref_on_the_same_counters():
    """found / visible = 2 / 5 is 0.4f exactly and stays; 1 / 3 goes; a bad point leaves the list untouched."""
    counters = [(2, 5), (1, 3), (39, 100), (40, 100), (1, 1), (0, 1), (3, 3), (0, 0), (7, 0)]
    first_kf = [9, 9, 9, 9, 7, 7, 6, 9, 9]
    rm, tr = PE.EraseRefMap(), T.TrackRefMap()
    rm.add_keyframe([-1] * 16)
    tr.add_keyframe([-1] * 16)
    for p, (f, v) in enumerate(counters + [(0, 9)]):
        bad = p == len(counters)
        rm.add_point(bad=bad, found=f, visible=v)
        tr.add_point(bad=bad)
        tr.set_counters(p, v, f)
        rm.add_observation(p, 0, p)
        rm.kfs[0].table[p] = p
    ids = list(range(len(counters) + 1))
    action, c = rm.cull(ids, first_kf + [9], 10)
    assert action.tolist() == tr.cull(ids, first_kf + [9], 10).tolist()
    assert action[0] == 0 and action[1] == 2 and action[-1] == 1 and action[4] == 3
    gone = [p for p in ids if action[p] == 2]
    assert c == dict(n_found=0, n_ref_moved=0, n_set_bad=len(gone), n_records=len(gone), n_entries=len(gone))
    for p in ids:
        assert rm.points[p].bad == tr.points[p].bad
        assert rm.points[p].n_obs == 1                               # setBadFlag leaves nObs
        assert (dict(rm.observations(p)) == {}) == (action[p] == 2) and (rm.kfs[0].table[p] == -1) == (action[p] == 2)
