"""CPU tests of dsh_keyframe_process_new and dsh_point_store_upkeep: the binding, the order of checks on a host-only context with every
refusal an empty store can reach, and the store model tests/keyframe_insert_ref.py against the sequential restatement
tests/mappoint_ref.py (process_new_keyframe on MapPoint-like objects) on random scenes.  Every compared value is exact."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import keyframe_insert_ref as KI
import mappoint_ref as R

OK, ARG, STATE, NODEV = 0, 1, 3, 4
NEW_ENTRIES = ("dsh_keyframe_process_new", "dsh_point_store_upkeep")


def test_new_symbols_are_bound_and_outside_the_pinned_prefixes():
    from defslam_amd import _lib, localmap
    L = _lib.load()
    for n in NEW_ENTRIES:
        assert n in _lib.EXPORTED_SYMBOLS and getattr(L, n).argtypes is not None, n
        for prefix in ("dsh_mpdb_", "dsh_local_map_", "dsh_trackstate_", "dsh_kfdb_"):
            assert not n.startswith(prefix), n
    assert C.sizeof(_lib.KeyframeProcessInputC) == 16 and C.sizeof(_lib.KeyframeProcessCountsC) == 32
    assert C.sizeof(_lib.PointUpkeepInputC) == 32 and C.sizeof(_lib.PointUpkeepCountsC) == 20
    assert (_lib.DSH_MP_NO_REF, _lib.DSH_MP_SKIPPED_BAD, _lib.DSH_UPKEEP_IDS, _lib.DSH_UPKEEP_EMBEDDED) == (4, 8, 0, 1)
    assert (KI.NO_OBS, KI.NO_GOOD_DESC, KI.NO_REF, KI.SKIPPED_BAD) == (_lib.DSH_MP_NO_OBS, _lib.DSH_MP_NO_GOOD_DESC, _lib.DSH_MP_NO_REF,
                                                                       _lib.DSH_MP_SKIPPED_BAD)
    assert (KI.EMPTY, KI.BAD_POINT, KI.ADDED, KI.RECENT) == (localmap.KF_EMPTY, localmap.KF_BAD_POINT, localmap.KF_ADDED, localmap.KF_RECENT)
    for m in ("process_new_keyframe", "upkeep"):
        assert callable(getattr(localmap.MapPointStore, m))


def _rows(keep):
    """(entry, arguments after the store handle, part of the message) for an EMPTY store, in the order of the checks: each row is
    well-formed up to the argument it names."""
    from defslam_amd import _lib
    i32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    ids0, ids00 = np.zeros(1, np.int32), np.zeros(2, np.int32)
    keep += [ids0, ids00]
    pc, uc = _lib.KeyframeProcessCountsC(), _lib.PointUpkeepCountsC()
    fake = C.c_void_p(1)   # never dereferenced: the checks that come first refuse
    pin = lambda slot, kfdb=None: _lib.KeyframeProcessInputC(kfdb, slot)
    uin = lambda what=3, select=0, n=0, ids=None, kfdb=None: _lib.PointUpkeepInputC(kfdb, what, select, n, ids)
    rows = [
        ("dsh_keyframe_process_new", (None, None, None, C.byref(pc)), "in is NULL"),
        ("dsh_keyframe_process_new", (pin(0), None, None, None), "out is NULL"),
        ("dsh_keyframe_process_new", (pin(0, fake), None, None, C.byref(pc)), "slot outside the store"),
        ("dsh_keyframe_process_new", (pin(-1, fake), None, None, C.byref(pc)), "slot outside the store"),
        ("dsh_point_store_upkeep", (None, None, C.byref(uc)), "in is NULL"),
        ("dsh_point_store_upkeep", (uin(), None, None), "out is NULL"),
        ("dsh_point_store_upkeep", (uin(what=0, kfdb=fake), None, C.byref(uc)), "what is not a non-empty mask"),
        ("dsh_point_store_upkeep", (uin(what=4, kfdb=fake), None, C.byref(uc)), "what is not a non-empty mask"),
        ("dsh_point_store_upkeep", (uin(select=2, kfdb=fake), None, C.byref(uc)), "select is neither"),
        ("dsh_point_store_upkeep", (uin(n=-1, kfdb=fake), None, C.byref(uc)), "n < 0"),
        ("dsh_point_store_upkeep", (uin(n=1, kfdb=fake), None, C.byref(uc)), "array is NULL"),
        ("dsh_point_store_upkeep", (uin(n=1, ids=i32p(ids0), kfdb=fake), None, C.byref(uc)), "point id 0 outside the store"),
        ("dsh_point_store_upkeep", (uin(n=2, ids=i32p(ids00), kfdb=fake), None, C.byref(uc)), "outside the store"),
        ("dsh_point_store_upkeep", (uin(), None, C.byref(uc)), "kfdb is NULL"),
        ("dsh_point_store_upkeep", (uin(select=1), None, C.byref(uc)), "kfdb is NULL"),
        ("dsh_point_store_upkeep", (uin(what=2, select=1, n=7), None, C.byref(uc)), "kfdb is NULL"),   # ids ignored with DSH_UPKEEP_EMBEDDED
    ]
    keep.append(rows)
    return rows


def test_order_of_checks_on_a_host_only_context(host_ctx):
    """Arguments first, each DSH_ERR_ARG with a message that names the entry, and nothing changed.  A keyframe store cannot exist on a
    host-only context (its create is the device gate), so the refusal that follows the arguments there is the NULL keyframe store."""
    from test_local_map_cpu import _raw_store
    L = host_ctx._L
    msg = lambda: L.dsh_last_error(host_ctx._h).decode()
    rc, h = _raw_store(L, host_ctx._h)
    assert rc == OK and h
    keep = []
    rows = _rows(keep)
    assert {r[0] for r in rows} == set(NEW_ENTRIES)
    for name, args, part in rows:
        a = [C.byref(x) if isinstance(x, C.Structure) else x for x in args]
        assert getattr(L, name)(h, *a) == ARG, (name, part)
        assert name in msg() and part in msg(), (name, part, msg())
        assert getattr(L, name)(None, *a) == ARG, (name, "NULL store")
    kf = C.c_void_p()
    assert L.dsh_kfdb_create(host_ctx._h, 4, C.byref(kf)) == NODEV and not kf
    assert L.dsh_mpdb_point_count(h) == 0 and L.dsh_mpdb_keyframe_count(h) == 0
    assert L.dsh_mpdb_destroy(h) == OK


def test_a_detached_store_refuses_both_entries():
    from defslam_amd import sft
    from test_local_map_cpu import _raw_store
    ctx = sft.Context(-1)
    L = ctx._L
    rc, h = _raw_store(L, ctx._h)
    assert rc == OK
    ctx.close()                                    # dsh_destroy detaches the store
    keep = []
    for name, args, _ in _rows(keep):
        a = [C.byref(x) if isinstance(x, C.Structure) else x for x in args]
        assert getattr(L, name)(h, *a) == ARG, name
    assert L.dsh_mpdb_destroy(h) == OK


# ---- the store model against the restatement -----------------------------------------------------------------------------------------

def _objects(m):
    """MapPoint-like objects of tests/mappoint_ref.py from the model's state."""
    return [SimpleNamespace(xyz=pt.xyz.copy(), ref_kf=pt.ref, obs=dict(pt.obs), desc=pt.desc.copy(), normal=pt.normal.copy(),
                            max_distance=pt.max_distance, min_distance=pt.min_distance, bad=pt.bad) for pt in m.points]


@pytest.mark.parametrize("seed", range(6))
def test_model_equals_the_restatement_on_random_scenes(seed):
    """The model's process_new_keyframe against mappoint_ref.process_new_keyframe: the same points updated and recent, in the same order,
    and every mutated field of every point equal as bytes.  The scenes hold a point in two entries, a point that observes the new
    keyframe already, bad points, bad keyframes and reference keyframes outside the observations."""
    m, slot = KI.random_model(seed, K=7, N=8, P=24)
    for pt in m.points:
        pt.ref = max(pt.ref, 0)                   # the restatement has no "no reference keyframe"
    pts = _objects(m)
    table = m.kfs[slot].table
    assert len({p for p in table if p >= 0}) < len([p for p in table if p >= 0])     # a point held twice
    updated, recent = R.process_new_keyframe(m.kfs, slot, [None if p < 0 else pts[p] for p in table])
    action, added, status = m.process_new_keyframe(slot)
    where = {id(o): p for p, o in enumerate(pts)}
    assert [where[id(x)] for x in updated] == added
    assert [where[id(x)] for x in recent] == [p for p, a in zip(table, action) if a == KI.RECENT]
    assert [a == KI.BAD_POINT for a in action] == [p >= 0 and m.points[p].bad for p in table]
    assert KI.RECENT in action and KI.ADDED in action
    for p, o in enumerate(pts):
        assert o.obs == dict(m.observations(p)) and len(o.obs) == m.points[p].n_obs, p
        assert o.desc.tobytes() == m.points[p].desc.tobytes(), p
        assert np.asarray(o.normal, np.float32).tobytes() == m.points[p].normal.tobytes(), p
        assert np.float32(o.max_distance).tobytes() == m.points[p].max_distance.tobytes() and np.float32(o.min_distance).tobytes() == m.points[p].min_distance.tobytes(), p
    assert all((s & KI.NO_OBS) == 0 for s in status)
    # a second pass adds nothing
    before = m.point_arrays()
    action2, added2, _ = m.process_new_keyframe(slot)
    assert added2 == [] and all(a != KI.ADDED for a in action2)
    assert all(before[k].tobytes() == m.point_arrays()[k].tobytes() for k in before)


def test_model_does_not_depend_on_the_order_of_the_log():
    a, slot = KI.random_model(3, shuffle=True)
    b, _ = KI.random_model(3, shuffle=False)
    assert [r[:3] for r in a.log] != [r[:3] for r in b.log] and sorted(r[:3] for r in a.log) == sorted(r[:3] for r in b.log)
    assert a.process_new_keyframe(slot) == b.process_new_keyframe(slot)
    assert all(v.tobytes() == b.point_arrays()[k].tobytes() for k, v in a.point_arrays().items())


def test_model_statuses():
    """A bad point is skipped; no observation, every keyframe bad and no reference keyframe each leave what the contract says."""
    m, slot = KI.random_model(1, K=4, N=6, P=10, p_bad_kf=0.0, p_bad_point=0.0)
    p = next(p for p in range(10) if len(m.observations(p)) >= 2)
    before = {k: v[p].copy() for k, v in m.point_arrays().items() if k != "bad"}
    m.points[p].bad = True
    assert m.upkeep([p]) == [KI.SKIPPED_BAD] and all(before[k].tobytes() == m.point_arrays()[k][p].tobytes() for k in before)
    m.points[p].bad = False
    for s, _ in m.observations(p):
        m.kfs[s].bad = True
    m.points[p].ref = m.observations(p)[0][0]
    assert m.upkeep([p]) == [KI.NO_GOOD_DESC]
    after = {k: v[p].copy() for k, v in m.point_arrays().items()}
    assert after["desc"].tobytes() == before["desc"].tobytes() and after["normal"].tobytes() != before["normal"].tobytes()
    m.points[p].ref = -1
    m.kfs[m.observations(p)[0][0]].bad = False
    m.points[p].normal = before["normal"]
    assert m.upkeep([p]) == [KI.NO_REF]
    assert m.points[p].normal.tobytes() == before["normal"].tobytes() and m.points[p].desc.tobytes() == m.kfs[m.observations(p)[0][0]].desc[m.observations(p)[0][1]].tobytes()
    for s, _ in m.observations(p):
        m.erase_observation(p, s)
    assert m.upkeep([p]) == [KI.NO_OBS] and m.points[p].n_obs == 0
