"""GPU tests of dsh_track_keyframe_candidate, dsh_keyframe_create and dsh_keyframe_update_connections against the restatement
(tests/keyframe_create_ref.py) and against the four calls the creation stands for.  Everything is exact."""
import numpy as np
import pytest

import keyframe_create_ref as KC
import keyframe_insert_ref as KI
import local_map_ref as LM
from store_model import store_state

pytestmark = pytest.mark.gpu

NODES, BARY = np.array([0, 1, 2], np.int32), np.array([0.2, 0.3, 0.5])


def stores(ctx, m, small=True):
    """The model in a fresh pair of stores; small: every capacity starts at 1, so the arrays grow on the way."""
    from defslam_amd import localmap, mappoint
    st = localmap.MapPointStore(ctx, points=1, keyframes=1, observations=1) if small else localmap.MapPointStore(ctx)
    appearance = bool(m.kfs) and all(k.has_appearance for k in m.kfs)
    ks = mappoint.KeyFrameStore(ctx, 1) if appearance or not m.kfs else None
    m.fill(st, ks)
    ids = sorted(m.facet)
    if ids:
        st.set_embedding(ids, np.tile(NODES, (len(ids), 1)), np.tile(BARY, (len(ids), 1)))
    return st, ks


def mp_keyframe(d):
    from defslam_amd import mappoint
    return mappoint.MpKeyFrame(np.zeros(3, np.float32), d["desc"], d["octave"], d["scale_factors"])


def everything(st, ks, slot, kpn):
    """What the issue names of a new keyframe, as bytes and lists."""
    pt, xyz = st.get_snapshot(slot)
    out = dict(table=st.keyframe_table(slot).tolist(), snap_point=pt.tolist(), snap_xyz=xyz.tobytes(), centre=st.keyframe_centre(ks, slot).tobytes(),
               surface_state=st.surface_state(slot), n_kf=(st.n_keyframes, len(ks)))
    if kpn:
        s = st.surface_get(slot)
        out.update(normals=s.normals.tobytes(), has=s.has_normal.tolist(), pts=s.pts.tobytes(), kpn=s.kpn.tobytes(), n_normals=s.n_normals, depth=s.ctrl is None)
    return out


def upkeep_of(st, ks, slot):
    """process_new_keyframe and the upkeep of the points it added, then the whole store."""
    r = st.process_new_keyframe(ks, slot)
    u = st.upkeep(ks, ids=r.added if len(r.added) else [0])
    g = st.get_points()
    s = store_state(st)
    return dict(action=r.action.tolist(), added=r.added.tolist(), counts=(r.n_empty, r.n_bad, r.n_added, r.n_recent, r.n_no_good_desc, r.n_no_ref),
                status=u.status.tolist(), desc=g.desc.tobytes(), normal=g.normal.tobytes(), maxd=g.max_distance.tobytes(), n_obs=s["n_obs"].tolist(), obs=s["obs"],
                tables=s["tables"])


@pytest.mark.parametrize("N,source,kpn", [(0, "points", True), (0, "candidate", False), (1, "points", False), (1, "candidate", True), (70, "points", True),
                                          (70, "candidate", True), (300, "points", False), (300, "candidate", True), (1200, "points", True),
                                          (1200, "candidate", False)])
def test_create_equals_the_four_calls_and_the_restatement(gpu_ctx, N, source, kpn):
    m, d = KC.create_scene(N, seed=N)
    a, ka = stores(gpu_ctx, m)
    b, kb = stores(gpu_ctx, m)
    fp, octave = d["frame_points"], d["octave"]
    cand = m.end_frame_candidate(fp)
    if source == "candidate":
        ea, eb = a.end_frame(fp, d["outlier"], octave), b.end_frame(fp, d["outlier"], octave)
        assert ea.points.tolist() == eb.points.tolist() == cand == a.keyframe_candidate().tolist()
        if N >= 70:   # the frame has cleaned entries and outliers: the outliers are IN the candidate, the cleaned entries are -1
            assert any(f >= 0 and c < 0 for f, c in zip(fp, cand)) and any(o and c >= 0 for o, c in zip(d["outlier"], cand))
            assert a.last_frame().ids.tolist() != cand
    points = None if source == "candidate" else cand
    K0 = a.n_keyframes
    r = a.create_keyframe(ka, mp_keyframe(d), d["Tcw"], points=points, kpn=d["kpn"] if kpn else None)
    want = m.create(d["desc"], octave, d["scale_factors"], d["Tcw"], points=points, kpn=d["kpn"] if kpn else None)
    assert (r.slot, r.n_held, r.n_snapshot) == (want["slot"], want["n_held"], want["n_snapshot"]) and r.slot == K0
    assert r.Ow.tobytes() == want["Ow"].tobytes()
    # the four calls on the second pair
    from defslam_amd import mappoint
    assert kb.add(mappoint.MpKeyFrame(want["Ow"], d["desc"], octave, d["scale_factors"])) == K0
    assert b.add_keyframe(np.array(cand, np.int32)) == K0
    assert b.snapshot_positions(K0) == want["n_snapshot"]
    if kpn:
        b.surface_init(K0, d["kpn"])
    ga, gb = everything(a, ka, K0, kpn), everything(b, kb, K0, kpn)
    assert ga == gb
    # ... and the restatement
    pt, xyz = m.get_snapshot(K0)
    assert ga["table"] == cand and ga["snap_point"] == pt.tolist() and ga["snap_xyz"] == xyz.tobytes() and ga["centre"] == want["Ow"].tobytes()
    assert ga["surface_state"] == (1 if kpn else 0) and ga["n_kf"] == (K0 + 1, K0 + 1)
    if kpn:
        assert ga["kpn"] == d["kpn"].tobytes() and ga["n_normals"] == 0 and not any(ga["has"]) and ga["pts"] == bytes(12 * N) == ga["normals"] and ga["depth"]
    if source == "candidate":
        assert a.keyframe_candidate().tolist() == cand           # not consumed
    # no observation was added; the upkeep that follows is the same on both pairs
    assert store_state(a)["obs"] == m.state()["obs"]
    assert upkeep_of(a, ka, K0) == upkeep_of(b, kb, K0)
    # the mirrors: a second snapshot and a second Surface are refused, as after the four calls
    from defslam_amd.sft import DshError
    with pytest.raises(DshError, match="status 3"):
        a.snapshot_positions(K0)
    if kpn:
        with pytest.raises(DshError, match="status 3"):
            a.surface_init(K0, d["kpn"])
    for s in (a, b, ka, kb):
        s.close()


def test_two_keyframes_from_one_candidate(gpu_ctx):
    m, d = KC.create_scene(70, seed=5)
    a, ka = stores(gpu_ctx, m)
    cand = m.end_frame_candidate(d["frame_points"])
    a.end_frame(d["frame_points"], d["outlier"], d["octave"])
    for k in range(2):
        r = a.create_keyframe(ka, mp_keyframe(d), d["Tcw"], kpn=d["kpn"])
        want = m.create(d["desc"], d["octave"], d["scale_factors"], d["Tcw"], kpn=d["kpn"])
        assert (r.slot, r.n_held, r.n_snapshot) == (want["slot"], want["n_held"], want["n_snapshot"]) == (2 + k, want["n_held"], want["n_snapshot"])
        assert a.keyframe_table(r.slot).tolist() == cand and a.get_snapshot(r.slot)[0].tolist() == m.get_snapshot(r.slot)[0].tolist()
    assert a.n_keyframes == len(ka) == 4
    a.clear()                                                    # forgets the candidate with the last-frame list
    from defslam_amd.sft import DshError
    with pytest.raises(DshError, match="no resident keyframe candidate"):
        a.keyframe_candidate()
    a.close()
    ka.close()


def test_create_refusals_leave_both_stores_unchanged(gpu_ctx):
    from defslam_amd import localmap, mappoint, sft
    from defslam_amd.sft import DshError
    m, d = KC.create_scene(6, seed=3)
    a, ka = stores(gpu_ctx, m, small=False)
    kf, T = mp_keyframe(d), d["Tcw"]
    P = a.n_points
    other = mappoint.KeyFrameStore(gpu_ctx, 4)                   # holds no keyframe: another count than the point store
    ctx2 = sft.Context(0)
    foreign = mappoint.KeyFrameStore(ctx2, 4)
    foreign.add(mp_keyframe(d)), foreign.add(mp_keyframe(d))

    def with_kf(**over):
        k = dict(desc=d["desc"], octave=d["octave"], scale_factors=d["scale_factors"])
        k.update(over)
        return mappoint.MpKeyFrame(np.zeros(3, np.float32), k["desc"], k["octave"], k["scale_factors"])
    nan_T, big_T = T.copy(), T.copy()
    nan_T[1, 2] = np.nan
    big_T[:3, :] = np.float32(3e38)
    nan_kpn = d["kpn"].copy()
    nan_kpn[2, 1] = np.inf
    ok_pts = np.full(6, -1, np.int32)
    cases = [("no candidate", lambda: a.create_keyframe(ka, kf, T), "no resident keyframe candidate"),
             ("id outside", lambda: a.create_keyframe(ka, kf, T, points=[0, P, -1, -1, -1, -1]), "table entry 1 is neither -1 nor a point of the store"),
             ("id below", lambda: a.create_keyframe(ka, kf, T, points=[0, -2, -1, -1, -1, -1]), "table entry 1"),
             ("kfdb NULL", lambda: a.create_keyframe(None, kf, T, points=ok_pts), "kfdb is NULL"),
             ("another context", lambda: a.create_keyframe(foreign, kf, T, points=ok_pts), "belongs to another context or was detached"),
             ("another count", lambda: a.create_keyframe(other, kf, T, points=ok_pts), "the new slot must be the same in both"),
             ("octave", lambda: a.create_keyframe(ka, with_kf(octave=[0, 1, 128, 0, 0, 0]), T, points=ok_pts), "octave outside 0 .. 127"),
             ("levels", lambda: a.create_keyframe(ka, with_kf(scale_factors=np.ones(33, np.float32)), T, points=ok_pts), "levels outside 1 .. 32"),
             ("Tcw", lambda: a.create_keyframe(ka, kf, nan_T, points=ok_pts), "Tcw is not finite"),
             ("centre", lambda: a.create_keyframe(ka, kf, big_T, points=ok_pts), "camera centre not finite"),
             ("kpn", lambda: a.create_keyframe(ka, kf, T, points=ok_pts, kpn=nan_kpn), "key point 2 is not finite"),
             ("N", lambda: a.create_keyframe(ka, mappoint.MpKeyFrame(np.zeros(3, np.float32), np.zeros((8193, 32), np.uint8), np.zeros(8193, np.int32), np.ones(1, np.float32)),
                                             T, points=np.full(8193, -1, np.int32)), "N outside 0 .. 8192")]
    for name, call, words in cases + [("candidate length", lambda: a.create_keyframe(ka, kf, T), "the resident keyframe candidate has 5 entries, kf->N is 6")]:
        if name == "candidate length":                           # from here on there is a candidate, of another length
            a.end_frame(np.full(5, -1, np.int32), np.zeros(5, np.uint8), np.zeros(5, np.int32))
        with pytest.raises(DshError) as e:
            call()
        assert "dsh_keyframe_create: status 1" in str(e.value) and words in str(e.value), (name, str(e.value))
        assert (a.n_keyframes, len(ka), len(other), len(foreign)) == (2, 2, 0, 2), name
    ctx2.close()                                                 # a keyframe store whose context is gone is detached: the same refusal
    with pytest.raises(DshError) as e:
        a.create_keyframe(foreign, kf, T, points=ok_pts)
    assert "dsh_keyframe_create: status 1" in str(e.value) and "belongs to another context or was detached" in str(e.value)
    assert (a.n_keyframes, len(ka)) == (2, 2)
    # and the stores still work
    assert a.create_keyframe(ka, kf, T, points=ok_pts).slot == 2
    for s in (a, ka, other, foreign):
        s.close()


# ---- connections ---------------------------------------------------------------------------------------------------------------------------

def connect(st, m, slot, th):
    got, want = KC.connections_of(st.update_connections(slot, th)), m.update_connections(slot, th)
    assert got == want, (slot, th, got, want)
    return got


@pytest.mark.parametrize("name", sorted(KC.hand_cases()))
def test_hand_cases_on_the_device(gpu_ctx, name):
    m, slot, th = KC.hand_cases()[name]
    st, _ = stores(gpu_ctx, m)
    connect(st, m, slot, th)
    connect(st, m, slot, th)                                     # the second call: the parent is read back from the device, not set again
    st.close()


def test_second_call_and_preset_parent_on_the_device(gpu_ctx):
    m, slot, th = KC.hand_cases()["equal_connected"]
    st, _ = stores(gpu_ctx, m)
    assert connect(st, m, slot, th)["parent"] == 3
    new = [(p, 0) for p in (0, 1, 3)] + [(3, 2)]
    for p, k in new:
        assert m.add_observation(p, k)
    st.add_observations([p for p, _ in new], [k for _, k in new])
    r = connect(st, m, slot, th)
    assert r["ordered_kf"] == [0, 3, 1] and r["parent"] == 3 and not r["parent_set"]
    st.close()
    m, slot, th = KC.hand_cases()["th_met"]
    st, _ = stores(gpu_ctx, m)
    st.set_keyframe_parent(slot, 2)                              # ChangeParent leaves mbFirstConnection alone: the first connection overwrites it
    m.kfs[slot].parent = 2
    r = connect(st, m, slot, th)
    assert r["parent_set"] and r["parent"] == 0
    assert KC.connections_of(st.update_connections(slot, th))["parent"] == 0   # read back from the device
    st.close()


@pytest.mark.parametrize("seed,K,N,P,max_obs,ths,equal", [
    # K old keyframes and the new one: the store holds 2, 65 and 300 (one keyframe alone is the hand case "alone")
    (0, 1, 5, 4, 3, (1, 2), False),
    (2, 64, 70, 50, 40, (1, 2, 100), False),                     # the ordering crosses a wavefront
    (3, 299, 1200, 900, 40, (1, 3, 100), False),                 # ... and a workgroup; a log of several grid strides with blanked records
    (4, 299, 64, 8, 299, (1, 1000), True),                       # all weights equal: the order is by slot alone
    (11, 8200, 40, 60, 400, (2,), False),                        # more keyframes than a pass of the histogram holds
])
def test_random_scenes_on_the_device(gpu_ctx, seed, K, N, P, max_obs, ths, equal):
    m, slot = KC.random_connections(seed, K, N, P, max_obs, p_bad=0.0 if equal else 0.05, equal=equal)
    st, _ = stores(gpu_ctx, m, small=K < 1000)
    for th in ths:
        r = connect(st, m, slot, th)
    if K == 8200:
        assert max(r["counted_kf"]) >= 8192 and len(r["ordered_kf"]) > 1000
    assert st.n_keyframes == K + 1
    if K == 299 and not equal:
        assert len(m.log) > 4096 and any(not rec[3] for rec in m.log) and len(r["counted_kf"]) > 256
    if equal:
        assert r["ordered_kf"] == [r["max_kf"]] == [0]          # th above every weight: the fallback, the lowest slot
        assert KC.connections_of(st.update_connections(slot, 1))["ordered_kf"] == list(range(K - 1, -1, -1))
    st.close()


def test_connections_refusals(gpu_ctx):
    from defslam_amd import _lib
    from defslam_amd.sft import DshError, _ptr
    import ctypes as C
    m, slot, th = KC.hand_cases()["th_met"]
    st, _ = stores(gpu_ctx, m)
    for call, words in ((lambda: st.update_connections(4), "slot outside the store"), (lambda: st.update_connections(-1), "slot outside the store"),
                        (lambda: st.update_connections(slot, 0), "th < 1")):
        with pytest.raises(DshError, match="status 1") as e:
            call()
        assert words in str(e.value)
    buf = np.zeros(8, np.int32)
    L = gpu_ctx._L
    assert L.dsh_keyframe_update_connections(st._h, slot, 3, 3, _ptr(buf, C.c_int32), None, None, None, None) == _lib.DSH_ERR_ARG   # capacity 3 < 4 keyframes
    assert b"capacity is smaller" in L.dsh_last_error(gpu_ctx._h)
    assert L.dsh_keyframe_update_connections(st._h, slot, 3, 0, None, None, None, None, None) == _lib.DSH_OK                         # no list: no capacity needed
    assert KC.connections_of(st.update_connections(slot, 3))["parent"] == 0                                                        # which set the parent
    st.close()


def test_the_limit_of_65535_keyframes(gpu_ctx):
    """The store may hold 65535 keyframes: a slot fits 16 bits beside a weight in the ordering's key.  Both stores are filled to the
    limit through dsh_keyframe_create (empty keyframes but a few; the last one, slot 65534, holds the table), the connections of the
    last slot equal the restatement -- keyframes 0 and 65533 among the connected, ties at both ends -- the 65536th creation is refused
    with both counts unchanged, and a store pushed past the limit through dsh_mpdb_add_keyframe refuses the connections."""
    from defslam_amd import localmap, mappoint
    from defslam_amd.sft import DshError
    LIMIT, P = 65535, 24
    rng = np.random.default_rng(65535)
    slot = LIMIT - 1
    table = [int(p) for p in rng.integers(0, P, 40)] + [-1, 0, 0]
    m = KC.topology(LIMIT, P, {slot: table}, bad_points=(5,))
    observers = {0: range(0, 12), 1: range(0, 12), 63: range(3, 9), 64: range(2, 20), 255: range(10, 14), 256: range(0, 24), 8191: range(4, 16), 8192: range(4, 16),
                 30000: range(7, 8), 65533: range(0, 24), slot: range(0, 6)}
    pairs = [(p, k) for k, ps in observers.items() for p in ps]
    for p, k in pairs:
        assert m.add_observation(p, k)
    m.erase_observation(3, 64)
    st, ks = localmap.MapPointStore(gpu_ctx, points=P, keyframes=1024), mappoint.KeyFrameStore(gpu_ctx, 1024)
    st.add_points(np.zeros((P, 3), np.float32), np.tile(np.float32([0, 0, 1]), (P, 1)), np.ones(P, np.float32), np.zeros((P, 32), np.uint8),
                  np.array([pt.bad for pt in m.points], np.uint8))
    T = np.eye(4, dtype=np.float32)
    empty = mappoint.MpKeyFrame(np.zeros(3, np.float32), np.zeros((0, 32), np.uint8), np.zeros(0, np.int32), np.ones(1, np.float32))
    for k in range(slot):
        st.create_keyframe(ks, empty, T, points=[])
    N = len(table)
    last = mappoint.MpKeyFrame(np.zeros(3, np.float32), np.zeros((N, 32), np.uint8), np.zeros(N, np.int32), np.ones(1, np.float32))
    assert st.create_keyframe(ks, last, T, points=table).slot == slot and (st.n_keyframes, len(ks)) == (LIMIT, LIMIT)
    st.add_observations([p for p, _ in pairs], [k for _, k in pairs])
    st.erase_observations([3], [64])
    with pytest.raises(DshError) as e:
        st.create_keyframe(ks, empty, T, points=[])
    assert "dsh_keyframe_create: status 1" in str(e.value) and "holds 65535 keyframes already" in str(e.value)
    assert (st.n_keyframes, len(ks)) == (LIMIT, LIMIT)
    first = connect(st, m, slot, 1)
    assert first["parent_set"] and 0 in first["ordered_kf"] and 65533 in first["ordered_kf"] and first["max_kf"] == 256 and first["parent"] == 65533
    assert len(set(first["ordered_w"])) < len(first["ordered_w"])                # ties: among equals the higher slot comes first
    connect(st, m, slot, first["max_weight"] + 1)                                # nobody reaches th: (nmax, pKFmax), the LOWER of 256 and 65533
    connect(st, m, 0, 1)                                                         # slot 0 holds nothing
    assert st.add_keyframe([]) == LIMIT                                          # past the limit, behind the creation's back
    for call, words in ((lambda: st.update_connections(slot, 1), "dsh_keyframe_update_connections: status 1: dsh_keyframe_update_connections: the store holds more than 65535 keyframes"),
                        (lambda: st.create_keyframe(ks, empty, T, points=[]), "dsh_keyframe_create: status 1")):
        with pytest.raises(DshError) as e:
            call()
        assert words in str(e.value), str(e.value)
    assert (st.n_keyframes, len(ks)) == (LIMIT + 1, LIMIT)
    st.close()
    ks.close()


# ---- the chain -----------------------------------------------------------------------------------------------------------------------------

class ChainModel(KC.CreateModel, LM.RefMap, KI.StoreModel):
    pass


def test_chain_from_end_frame_to_the_next_local_map(gpu_ctx):
    """end_frame -> create_keyframe -> process_new_keyframe -> update_connections -> update_local_map of a next frame: the one place the
    parent is read.  The same scene with the parent set through set_keyframe_parent from the restatement gives the same list."""
    m, d = KC.create_scene(300, seed=9, K_old=6, N_old=40, P=200, cls=ChainModel)
    a, ka = stores(gpu_ctx, m)
    b, kb = stores(gpu_ctx, m)
    m.end_frame_candidate(d["frame_points"])
    for st, ks in ((a, ka), (b, kb)):
        st.end_frame(d["frame_points"], d["outlier"], d["octave"])
        slot = st.create_keyframe(ks, mp_keyframe(d), d["Tcw"], kpn=d["kpn"]).slot
        r = st.process_new_keyframe(ks, slot)
    assert m.create(d["desc"], d["octave"], d["scale_factors"], d["Tcw"], kpn=d["kpn"])["slot"] == slot == 6
    _, added, _ = m.process_new_keyframe(slot)
    assert r.added.tolist() == added and len(added) > 50
    want = m.update_connections(slot, 15)
    assert KC.connections_of(a.update_connections(slot, 15)) == want and want["parent_set"] and 0 <= want["parent"] < 6
    # the next frame sees points of the parent only: the new keyframe enters the list as the parent's child, and only so
    nxt = [p for p in m.kfs[want["parent"]].table if not m.points[p].bad and list(m.points[p].obs) == [want["parent"]]][:8]
    assert nxt and slot not in b.update_local_map(nxt).local_kf.tolist()
    b.set_keyframe_parent(slot, want["parent"])
    la, lb, lm = a.update_local_map(nxt), b.update_local_map(nxt), m.update_local_map(nxt)
    assert la.local_kf.tolist() == lb.local_kf.tolist() == lm["local_kf"].tolist() and slot in la.local_kf.tolist()
    assert la.votes.tolist() == lb.votes.tolist() == lm["votes"].tolist() and la.ref_kf == lb.ref_kf == lm["ref_kf"]
    for s in (a, b, ka, kb):
        s.close()
