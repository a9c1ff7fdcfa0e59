"""CPU tests of the surface registration of a keyframe from the resident stores (dsh_keyframe_snapshot_positions, dsh_keyframe_get_snapshot,
dsh_keyframe_register_clouds, dsh_keyframe_register, dsh_keyframe_set_pose, dsh_keyframe_get_centre): the binding, the header's
constraint on the new prototypes, the order of checks on a host-only context, the restatement tests/surface_register_ref.py against a
second transcription of SurfaceRegistration.cc:60-104 on MapPoint-like objects, and the oracle's verdicts on the scene the GPU test
registers.  Integers and bytes are compared exactly."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import surface_register_ref as SR
from conftest import ROOT
from template_switch_ref import to_world

OK, ARG, STATE, NODEV = 0, 1, 3, 4
NEW_ENTRIES = ("dsh_keyframe_snapshot_positions", "dsh_keyframe_get_snapshot", "dsh_keyframe_register_clouds", "dsh_keyframe_register",
               "dsh_keyframe_set_pose", "dsh_keyframe_get_centre")
REGISTER_PAIRS = (14, 15, 40, 300)                   # the pair counts test_surface_register_store_gpu registers


def register_scene(n_pairs):
    return SR.make_scene(max(64, 2 * n_pairs), seed=3, n_pairs=n_pairs)


def test_new_symbols_are_bound():
    from defslam_amd import _lib, localmap
    L = _lib.load()
    for n in NEW_ENTRIES:
        assert n in _lib.EXPORTED_SYMBOLS and getattr(L, n).argtypes is not None, n
    assert C.sizeof(_lib.KeyframeRegisterInputC) == 64 and C.sizeof(_lib.KeyframeRegisterResultC) == 256
    assert _lib.KeyframeRegisterResultC.consumed.offset == 32 and _lib.KeyframeRegisterResultC.Tcw_new.offset == 176
    assert C.sizeof(_lib.KeyframePoseInputC) == 24
    for m in ("snapshot_positions", "get_snapshot", "register_clouds", "register_surface", "set_keyframe_pose", "keyframe_centre"):
        assert callable(getattr(localmap.MapPointStore, m))


def test_new_prototypes_stay_out_of_the_host_only_table():
    """tests/test_abi_and_host.py lists every dsh_name( of the header whose text up to the next ')' names a context, a DiffProp store, a
    keyframe store or a communicator, and wants a table row for each: the new entries take the point store alone and name the keyframe
    store in their input struct, so none of them may land in that set -- by a prototype or by a comment."""
    header = open(os.path.join(ROOT, "include", "defslam_hip.h")).read()
    takes = set(re.findall(r"\b(dsh_[a-z0-9_]+)\s*\((?:[^)]*\b(?:dsh_ctx|dsh_diffdb|dsh_kfdb|dsh_comm)\b)", header))
    assert not takes & set(NEW_ENTRIES), takes & set(NEW_ENTRIES)
    declared = set(re.findall(r"\b(dsh_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_ENTRIES) <= declared
    assert "so the store has no pose update" not in header and "dsh_keyframe_set_pose is the call" in header


def _rows(keep):
    """(entry, arguments after the store handle, part of the message) for an EMPTY store, in the order of the checks."""
    from defslam_amd import _lib
    f = np.zeros(16, np.float32)
    keep.append(f)
    fp = f.ctypes.data_as(C.POINTER(C.c_float))
    nan = np.full(16, np.nan, np.float32)
    keep.append(nan)
    nanp = nan.ctypes.data_as(C.POINTER(C.c_float))
    ip = np.zeros(4, np.int32)
    keep.append(ip)
    ipp = ip.ctypes.data_as(C.POINTER(C.c_int32))
    res = _lib.KeyframeRegisterResultC()
    fake = C.c_void_p(1)                                # never dereferenced: the checks that come first refuse
    rin = lambda slot=0, N=0, kfdb=None: _lib.KeyframeRegisterInputC(kfdb, slot, N, fp, fp, None, 0, 0.05, 1)
    pin = lambda slot=0, kfdb=fake, T=fp: _lib.KeyframePoseInputC(kfdb, slot, T)
    rows = [
        ("dsh_keyframe_snapshot_positions", (0, None), "slot outside the store"),
        ("dsh_keyframe_snapshot_positions", (-1, ipp), "slot outside the store"),
        ("dsh_keyframe_get_snapshot", (0, 8, ipp, fp), "slot outside the store"),
        ("dsh_keyframe_register_clouds", (None, None, None, None, C.byref(res)), "in is NULL"),
        ("dsh_keyframe_register_clouds", (rin(), None, None, None, None), "out is NULL"),
        ("dsh_keyframe_register_clouds", (rin(0, 0, fake), None, None, None, C.byref(res)), "slot outside the store"),
        ("dsh_keyframe_register", (None, None, None, C.byref(res)), "in is NULL"),
        ("dsh_keyframe_register", (rin(), None, None, None), "out is NULL"),
        ("dsh_keyframe_register", (rin(-1, 0, fake), None, None, C.byref(res)), "slot outside the store"),
        ("dsh_keyframe_set_pose", (None, None), "in is NULL"),
        ("dsh_keyframe_set_pose", (pin(kfdb=None), None), "kfdb is NULL"),
        ("dsh_keyframe_set_pose", (pin(T=None), None), "Tcw is NULL"),
        ("dsh_keyframe_get_centre", (None, fp), "in is NULL"),
        ("dsh_keyframe_get_centre", (pin(kfdb=None), fp), "kfdb is NULL"),
        ("dsh_keyframe_get_centre", (pin(), None), "Ow is NULL"),
        # a handle that is no store of this context is refused before anything of it is read, and so is a pose that is not finite
        ("dsh_keyframe_set_pose", (pin(), None), "belongs to another context or was detached"),
        ("dsh_keyframe_get_centre", (pin(), fp), "belongs to another context or was detached"),
        ("dsh_keyframe_set_pose", (pin(T=nanp), None), "Tcw is not finite"),
    ]
    keep.append(rows)
    return rows


def test_order_of_checks_on_a_host_only_context(host_ctx):
    """Arguments first, each DSH_ERR_ARG with a message that names the entry, and nothing written.  Every new entry names a keyframe of
    the store, and a host-only store stays empty (its mutations are refused), so no call on it is well-formed: the refusal that follows
    the arguments, DSH_ERR_NO_DEVICE saying "host-only", is what dsh_kfdb_create and dsh_mpdb_add_keyframe answer there."""
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
    assert L.dsh_kfdb_create(host_ctx._h, 4, C.byref(kf)) == NODEV and not kf and "host-only" in msg()
    assert L.dsh_mpdb_add_keyframe(h, 0, None, -1, 0, None) == NODEV and "host-only" in msg()
    assert L.dsh_mpdb_keyframe_count(h) == 0
    assert L.dsh_mpdb_destroy(h) == OK


def test_a_detached_store_refuses_every_entry():
    from defslam_amd import sft
    from test_local_map_cpu import _raw_store
    ctx = sft.Context(-1)
    L = ctx._L
    rc, h = _raw_store(L, ctx._h)
    assert rc == OK
    ctx.close()                                        # dsh_destroy detaches the store
    keep = []
    for name, args, _ in _rows(keep):
        a = [C.byref(x) if isinstance(x, C.Structure) else x for x in args]
        assert getattr(L, name)(h, *a) == ARG, name
    assert L.dsh_mpdb_destroy(h) == OK


# ---- the restatement against a second transcription --------------------------------------------------------------------------------------

class _MP:
    """A DefMapPoint as SurfaceRegistration.cc reads it."""

    def __init__(self, xyz, bad, facet):
        self.mWorldPos, self.bad, self.facet, self.PosesKeyframes, self.covNorm = xyz, bad, facet, {}, True

    def isBad(self):
        return self.bad

    def getFacet(self):
        return self.facet


def _transcription(kf, mvpMapPoints, surface, Twc):
    """SurfaceRegistration.cc:60-104, line by line, on objects: (cloud1pc, cloud2pc, the key points that made a pair)."""
    cloud1pc, cloud2pc, which = [], [], []
    for i in range(len(mvpMapPoints)):
        pMP = mvpMapPoints[i]
        if pMP:
            if pMP.isBad():
                continue
            if pMP.getFacet():
                if not pMP.covNorm:
                    continue
                x3Dy = pMP.PosesKeyframes.get(kf)      # operator[] of the unordered_map: an empty cv::Mat when absent
                if x3Dy is None:
                    continue
                cloud1pc.append([x3Dy[0], x3Dy[1], x3Dy[2]])
                x3DKf = to_world(Twc, surface[i])
                cloud2pc.append([x3DKf[0], x3DKf[1], x3DKf[2]])
                which.append(i)
    return np.array(cloud1pc, np.float32).reshape(-1, 3), np.array(cloud2pc, np.float32).reshape(-1, 3), which


def _objects(model):
    return [_MP(pt.xyz.copy(), pt.bad, model.facet.get(p)) for p, pt in enumerate(model.points)]


@pytest.mark.parametrize("N,seed,hold", [(40, 0, 0.5), (64, 1, 0.7), (257, 2, 0.5), (33, 3, 0.3), (20, 4, 0.5), (64, 5, 1.0), (64, 6, 0.0)])
def test_restatement_equals_the_transcription_on_random_scenes(N, seed, hold):
    sc = SR.make_scene(N, seed, hold=hold)
    m, slot = sc["model"], sc["slot"]
    objs = _objects(m)
    # DefKeyFrame.cc:60-74 on the objects, and the model's
    for p in m.kfs[slot].table:
        if p >= 0 and not objs[p].isBad() and objs[p].getFacet():
            objs[p].PosesKeyframes["kf"] = objs[p].mWorldPos.copy()
    taken = m.snapshot_positions(slot)
    assert taken == sum(p >= 0 and not m.points[p].bad and p in m.facet for p in m.kfs[slot].table)
    with pytest.raises(SR.SnapshotTaken):
        m.snapshot_positions(slot)
    # the scene's mutations after the snapshot, on both
    SR.apply_after(m, sc)
    for p, (o, pt) in enumerate(zip(objs, m.points)):
        o.mWorldPos, o.bad, o.facet = pt.xyz.copy(), pt.bad, m.facet.get(p)
    c, idx, surf, mp = m.select(slot, sc["surface_pts"], sc["Twc"])
    c1, c2, which = _transcription("kf", [objs[p] if p >= 0 else None for p in m.kfs[slot].table], sc["surface_pts"], sc["Twc"])
    assert idx.tolist() == which and mp.tobytes() == c1.tobytes() and surf.tobytes() == c2.tobytes()
    assert sum(c.values()) == N and c["n_pairs"] == len(which)
    if N >= 32 and 0 < hold < 1:                       # the specials are there and do what they promise
        r = sc["roles"]
        assert c["n_no_snapshot"] >= 1 and c["n_bad"] >= 1 and c["n_no_facet"] >= 1
        assert r.index("dup") in which and r.index("move_to") in which and r.index("move_from") not in which and r.index("add_to") not in which
        moved = np.array([m.points[m.kfs[slot].table[i]].xyz for i in which], np.float32)
        assert (np.abs(moved - mp).max(axis=1) > 0).all()   # a cloud read from the current positions would differ in every pair


@pytest.mark.parametrize("n_pairs", REGISTER_PAIRS)
def test_pair_count_scenes_have_exactly_that_many_pairs(n_pairs):
    sc = register_scene(n_pairs)
    m = sc["model"]
    m.snapshot_positions(sc["slot"])
    SR.apply_after(m, sc)
    c = m.select(sc["slot"], sc["surface_pts"], sc["Twc"])[0]
    assert c["n_pairs"] == n_pairs and c["n_no_snapshot"] == 1 and c["n_bad"] == 2 and c["n_no_facet"] == 2
    assert SR.consumed(n_pairs, sc["u"]) is not None and SR.consumed(n_pairs, sc["u"][:n_pairs]) is None


def test_erasures_leave_the_snapshot_and_empty_the_entries_their_records_name():
    """The restatement's side of the GPU test of dsh_point_store_set_bad, the erase and the cull after a snapshot: setBadFlag writes -1
    into the entries the point's records name, so those count as empty, not as bad; PosesKeyframes is never touched."""
    sc = register_scene(40)
    m, slot = sc["model"], sc["slot"]
    pick = SR.add_erase_fixture(sc)
    pt = {n: m.kfs[slot].table[i] for n, i in pick.items()}
    m.snapshot_positions(slot)
    SR.apply_after(m, sc)
    snap = {k: v.copy() for k, v in m.snap.items()}
    c0 = m.select(slot, sc["surface_pts"], sc["Twc"])[0]
    m.set_bad([pt["set_bad"], pt["twice"]])
    assert m.erase_observations([pt["erase_cascade"], pt["erase_keep"]], [slot, slot])[0].tolist() == [2, 1]
    assert m.erase_observations([pt["erase_match"]], [slot], erase_match=True)[0].tolist() == [1]
    assert m.cull([pt["cull"], pt["erase_keep"]], [0, 0], 1)[0].tolist() == [2, 0]
    t = m.kfs[slot].table
    assert [t[pick[n]] for n in SR.ERASE_PICKS] == [-1, pt["erase_cascade"], -1, pt["erase_keep"], -1, -1]
    assert t[sc["roles"].index("dup")] == pt["twice"] and m.points[pt["twice"]].bad and not m.points[pt["erase_match"]].bad
    assert snap.keys() == m.snap.keys() and all(snap[k].tobytes() == m.snap[k].tobytes() for k in snap)
    c, idx, _, _ = m.select(slot, sc["surface_pts"], sc["Twc"])
    assert (c["n_pairs"], c["n_empty"], c["n_bad"]) == (c0["n_pairs"] - 6, c0["n_empty"] + 4, c0["n_bad"] + 2)
    assert pick["erase_keep"] in idx


def test_centre_of_set_pose_is_within_one_ulp_of_float64():
    """A sanity check only: the float32 expression against -R^T t in float64."""
    rng = np.random.default_rng(0)
    for _ in range(50):
        q, _r = np.linalg.qr(rng.standard_normal((3, 3)))
        T = np.eye(4, dtype=np.float32)
        T[:3, :3], T[:3, 3] = q, rng.uniform(-2, 2, 3)
        want = -(T[:3, :3].astype(np.float64).T @ T[:3, 3].astype(np.float64))
        got = SR.centre_of(T)
        mag = np.abs(T[:3, :3].astype(np.float64)).T @ np.abs(T[:3, 3].astype(np.float64))
        assert (np.abs(got - want) <= np.spacing(mag.astype(np.float32)) * 1.5).all()
    s = SR.apply_scale(np.array([[1.5, -2.25, 3.0]], np.float32), 1.1)
    assert s.dtype == np.float32 and s.tobytes() == np.array([[1.5 * 1.1, -2.25 * 1.1, 3.0 * 1.1]]).astype(np.float32).tobytes()


def test_the_registered_scene_is_acceptable_at_0_05_and_not_at_1e_6(oracle_mod):
    """The GPU test's verdicts are the reference's own: on the clouds of its "registers" scene the oracle's OptimizeHorn is acceptable
    with chi_limit 0.05 and not with 1e-6."""
    sc = register_scene(40)
    m = sc["model"]
    m.snapshot_positions(sc["slot"])
    SR.apply_after(m, sc)
    c, _, surf, mp = m.select(sc["slot"], sc["surface_pts"], sc["Twc"])
    assert c["n_pairs"] == 40
    o = oracle_mod.scale_min_median(surf, mp, sc["u"])
    assert o["status"] == 0 and o["consumed"] == SR.consumed(c["n_pairs"], sc["u"])
    start = [0, 0, 0, 1, 0, 0, 0, float(np.float32(o["scale"]))]
    assert oracle_mod.optimize_horn(surf, mp, start, chi=0.05 ** 2)["ok"]
    assert not oracle_mod.optimize_horn(surf, mp, start, chi=1e-6 ** 2)["ok"]
