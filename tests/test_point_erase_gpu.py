"""GPU tests of the erase on the resident map point store: dsh_point_store_erase_observations, dsh_point_store_set_bad,
dsh_point_store_cull and the read-backs dsh_point_store_get_observations, dsh_point_store_get_keyframe_table.  The state of the store --
observations(), keyframe_table(), get_points().bad, get_state().n_obs, get_reference_keyframes() -- and the status, action and counts of
every call equal (==) the sequential restatement tests/point_erase_ref.py.  Integers: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import anchor_pairs_ref as AR
import keyframe_insert_ref as KI
import local_map_ref as LM
import point_erase_ref as PE
from store_model import assert_state

pytestmark = pytest.mark.gpu

OK, ARG, STATE = 0, 1, 3


def store_from(ctx, rm, **caps):
    from defslam_amd import localmap
    st = localmap.MapPointStore(ctx, **caps)
    rm.fill(st)
    return st


def erase_both(st, rm, pts, slots, erase_match, what=""):
    g = st.erase_observations_full(pts, slots, erase_match=erase_match)
    status, c = rm.erase_observations(pts, slots, erase_match=erase_match)
    assert g.status.tolist() == status.tolist(), (what, g.status, status)
    PE.assert_counts(g.counts, c, what)
    assert_state(st, rm, what)
    return g


def set_bad_both(st, rm, ids, what=""):
    PE.assert_counts(st.set_bad_full(ids), rm.set_bad(ids), what)
    assert_state(st, rm, what)


def cull_both(st, rm, ids, first_kf, current_kf, what=""):
    g = st.cull_full(ids, first_kf, current_kf)
    action, c = rm.cull(ids, first_kf, current_kf)
    assert g.action.tolist() == action.tolist(), (what, g.action, action)
    PE.assert_counts(g.counts, c, what)
    assert_state(st, rm, what)
    return g


@pytest.mark.parametrize("erase_match", [True, False])
def test_small_scene_every_case_in_one_batch(gpu_ctx, erase_match):
    """3 keyframes of 8 key points, 6 points (point_erase_ref.small_scene; tests/test_point_erase_cpu.py pins what it holds): the move of
    the reference keyframe and its absence, the cascade at 3 -> 2, the only observation, an entry that holds another point under the
    pair and under the cascade, a bad point with records, a pair that is not stored; then the same call again, which finds nothing."""
    rm, (pts, slots) = PE.small_scene()
    st = store_from(gpu_ctx, rm, points=2, keyframes=1, observations=4)
    assert_state(st, rm, "before")
    g = erase_both(st, rm, pts, slots, erase_match, "first")
    assert g.status.tolist() == [2, 2, 2, 2, 2, 0] and g.counts.n_ref_moved == 2 and g.counts.n_records == 13
    assert st.get_reference_keyframes().tolist() == [1, 2, 2, 1, 0, 0]
    assert st.keyframe_table(0)[3] == (-1 if erase_match else 4) and st.keyframe_table(1)[5] == -1
    g = erase_both(st, rm, pts, slots, erase_match, "second")
    assert g.status.tolist() == [0] * 6 and [getattr(g.counts, n) for n in PE.COUNT_NAMES] == [0] * 5
    st.close()


def test_a_log_that_spans_several_workgroups_of_the_sweep(gpu_ctx):
    """A few thousand records added in shuffled order.  setBadFlag of the points whose records lie at the first and the last position of
    the log and on both sides of the workgroup boundaries of the sweep (256 records per workgroup); then an erase batch in which the
    lowest remaining slot of some points arrived last, with and without a cascade."""
    rm = PE.long_scene()
    R = len(rm.log)
    assert 2500 <= R <= 6000
    edge = [0, R - 1, 255, 256, 511, 512, 1023, 1024]
    doomed = sorted({rm.log[r][0] for r in edge})
    # points whose last record in the log has their lowest slot: their reference keyframe becomes the highest slot, which the batch erases
    last = {}
    for r, (p, kf, _, _) in enumerate(rm.log):
        last[p] = kf
    late = [p for p, mp in enumerate(rm.points) if p not in doomed and len(mp.obs) >= 2 and last[p] == min(mp.obs)]
    assert sum(1 for p in late if len(rm.points[p].obs) >= 4) >= 5 and sum(1 for p in late if len(rm.points[p].obs) <= 3) >= 5
    for p in late:
        rm.points[p].ref = max(rm.points[p].obs)
    st = store_from(gpu_ctx, rm, points=16, keyframes=2, observations=64)
    set_bad_both(st, rm, doomed, "edges")
    rng = np.random.default_rng(5)
    others = [int(p) for p in rng.permutation(len(rm.points))[:200] if p not in late and p not in doomed]
    pts = late + others
    slots = [max(rm.points[p].obs) for p in late] + [int(rng.integers(0, len(rm.kfs))) for _ in others]
    before = [rm.points[p].ref for p in late]
    g = erase_both(st, rm, pts, slots, True, "late")
    assert all(rm.points[p].ref == last[p] != b for p, b in zip(late, before))
    assert g.counts.n_ref_moved >= len(late) and 0 < g.counts.n_set_bad < g.counts.n_found < len(pts)
    st.close()


def test_a_log_that_had_grown_and_holds_blanks_and_the_mirror_afterwards(gpu_ctx):
    """The store starts with room for 8 records and grows; a first batch leaves blanks, then pairs it erased -- by name and by cascade --
    are added again and get fresh records, a pair that is still live is refused, and a second batch runs over the blanks."""
    rm = PE.long_scene(seed=11, K=12, N=64, P=120)
    st = store_from(gpu_ctx, rm, points=4, keyframes=1, observations=8)
    rng = np.random.default_rng(2)
    pts = [int(p) for p in rng.permutation(len(rm.points))[:60]]
    slots = [min(rm.points[p].obs) if i % 3 else int(rng.integers(0, 12)) for i, p in enumerate(pts)]
    before = {p: dict(rm.points[p].obs) for p in pts}
    g = erase_both(st, rm, pts, slots, True, "first batch")
    assert g.counts.n_set_bad > 0 and g.counts.n_records > g.counts.n_found > 0
    named = [(p, s) for p, s, c in zip(pts, slots, g.status) if c != 0]
    cascaded = [(p, s) for p, c in zip(pts, g.status) if c == 2 for s in before[p] if (p, s) not in named]
    assert named and cascaded
    again = named[:10] + cascaded[:10]
    idx = [before[p][s] for p, s in again]
    R0 = len(rm.log)
    st.add_observations([p for p, _ in again], [s for _, s in again], idx=idx)        # accepted: the mirror dropped the keys
    for (p, s), i in zip(again, idx):
        assert rm.add_observation(p, s, i)
    assert len(rm.log) == R0 + len(again)
    assert_state(st, rm, "added again")
    live = next((p, s) for p, mp in enumerate(rm.points) for s in mp.obs)
    L = gpu_ctx._L
    i32 = lambda v: np.array([v], np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    assert L.dsh_point_store_add_observations_indexed(st._h, 1, i32(live[0]), i32(live[1]), i32(0)) == ARG   # still live: still refused
    assert_state(st, rm, "after the refused add")
    pts2 = [int(p) for p in rng.permutation(len(rm.points))[:50]]
    slots2 = [int(rng.integers(0, 12)) for _ in pts2]
    erase_both(st, rm, pts2, slots2, False, "second batch")
    set_bad_both(st, rm, [p for p, _ in again[:6]], "set bad over fresh records")
    st.close()


def test_read_back_of_points_with_more_than_one_wavefront_of_observations(gpu_ctx):
    """70 keyframes of 4 key points.  Points observed by 70, 65, 64, 1 and 0 keyframes and a few ordinary ones, the records added in
    shuffled order; an erase batch first leaves blanks in the log, one of them inside the list of 65.  The rank by slot then runs over
    lists of more than, exactly and less than a wavefront of 64 observations."""
    K = 70
    rm = PE.EraseRefMap()
    for _ in range(K):
        rm.add_keyframe([-1] * 4)
    # point -> (key point index, keyframes): 0 all 70; 1 has 66 and loses one; 2 has 64; 3 one; 4 none; 5 .. 8 ordinary, in entry 3
    seen = {0: (0, range(K)), 1: (1, range(66)), 2: (2, range(6, K)), 3: (3, [50]), 4: (3, []), 5: (3, [0, 10, 20, 30, 40]), 6: (3, [1, 11, 21]),
            7: (3, [2, 12, 22, 32]), 8: (3, [3, 13])}
    pairs = []
    for p, (i, kfs) in seen.items():
        assert rm.add_point(ref=min(kfs, default=-1)) == p
        for kf in kfs:
            assert rm.kfs[kf].table[i] == -1
            rm.kfs[kf].table[i] = p
            pairs.append((p, kf, i))
    for j in np.random.default_rng(17).permutation(len(pairs)):
        rm.add_observation(*pairs[int(j)])
    st = store_from(gpu_ctx, rm, points=4, keyframes=2, observations=32)
    g = erase_both(st, rm, [1, 5, 6], [30, 20, 11], True, "blanks")      # point 6 goes from 3 to 2 observations: bad, all its records blank
    assert g.status.tolist() == [1, 1, 2] and g.counts.n_records == 5
    want = [len(rm.observations(p)) for p in range(9)]
    assert want == [70, 65, 64, 1, 0, 4, 0, 4, 2]
    for ids in (list(range(9)), [8, 2, 4, 0, 6, 1], [1]):
        o = st.observations(ids)
        assert o.ptr.tolist() == np.concatenate([[0], np.cumsum([want[p] for p in ids])]).tolist(), ids
        assert len(o.slots) == len(o.idx) == o.ptr[-1]
        for i, p in enumerate(ids):
            assert o.of(i) == dict(rm.observations(p)), (ids, p)
    st.close()


def test_cull_equals_trackstate_cull_and_erases_the_records(gpu_ctx):
    rm = PE.long_scene(seed=4, K=10, N=160, P=300)
    rm.points[7].found, rm.points[7].visible = 2, 5          # 0.4f exactly: stays
    rm.points[8].found, rm.points[8].visible = 1, 3
    rm.points[9].bad = True                                       # already bad: action 1, its records stay
    st, twin = store_from(gpu_ctx, rm), store_from(gpu_ctx, rm)
    rng = np.random.default_rng(8)
    ids = [7, 8, 9] + [int(p) for p in rng.permutation(np.arange(10, 300))[:150]]
    first_kf = [9, 9, 9] + [int(v) for v in rng.integers(5, 10, len(ids) - 3)]      # the three named points are young
    n_obs = st.get_state().n_obs.copy()
    held = {p: dict(rm.points[p].obs) for p in ids}
    g = cull_both(st, rm, ids, first_kf, 10, "cull")
    assert g.action.tolist() == twin.cull(ids, first_kf, 10).tolist()
    assert g.action[0] == 0 and g.action[1] == 2 and g.action[2] == 1 and set(g.action.tolist()) == {0, 1, 2, 3}
    assert st.get_points().bad.tolist() == twin.get_points().bad.tolist()
    assert st.get_state().n_obs.tolist() == n_obs.tolist()             # setBadFlag leaves nObs
    o = st.observations(ids)
    for i, p in enumerate(ids):
        assert o.of(i) == ({} if g.action[i] == 2 else held[p]), p
        if g.action[i] == 2:
            assert all(st.keyframe_table(s)[j] == -1 for s, j in held[p].items())
    assert held[9] and g.counts.n_found == 0 and g.counts.n_set_bad == int((g.action == 2).sum())
    assert g.counts.n_records == g.counts.n_entries == sum(len(held[p]) for i, p in enumerate(ids) if g.action[i] == 2)
    st.close()
    twin.close()


class AllRefMap(PE.EraseRefMap, KI.StoreModel, AR.AnchorRefMap, LM.RefMap):
    """One model object with the four restatements that the mapping thread's calls are checked against."""


def _model_stores(ctx, seed, **kw):
    """A keyframe_insert_ref scene as a model that every restatement runs on, with its two stores."""
    from defslam_amd import localmap, mappoint
    rm, slot = KI.random_model(seed, cls=AllRefMap, **kw)
    rng = np.random.default_rng(seed + 100)
    for mp in rm.points:
        mp.found, mp.visible = int(rng.integers(1, 8)), int(rng.integers(1, 12))
    ks, st = mappoint.KeyFrameStore(ctx, 2), localmap.MapPointStore(ctx, points=8, keyframes=2, observations=16)
    rm.fill(st, ks)
    return slot, ks, st, rm, rng


def test_seeded_random_sequence_of_the_three_calls_between_adds_and_new_keyframes(gpu_ctx):
    """5 keyframes of 40 key points, 60 points: eight random batches of the three calls, each followed by add_observations(idx=...) and
    by process_new_keyframe on a random keyframe; every array is compared after every step."""
    slot, ks, st, rm, rng = _model_stores(gpu_ctx, 21, K=4, N=40, P=60, p_bad_point=0.05)
    K, P = len(rm.kfs), len(rm.points)
    assert K == 5 and P == 60 and all(len(kf.table) == 40 for kf in rm.kfs)
    assert_state(st, rm, "start")
    for step in range(8):
        ids = [int(p) for p in rng.permutation(P)[:int(rng.integers(1, 25))]]
        kind = step % 3
        if kind == 0:
            slots = [int(rng.choice(sorted(rm.points[p].obs))) if rm.points[p].obs and rng.random() < 0.8 else int(rng.integers(0, K))
                     for p in ids]
            erase_both(st, rm, ids, slots, bool(rng.integers(0, 2)), f"step {step} erase")
        elif kind == 1:
            cull_both(st, rm, ids, [int(v) for v in rng.integers(0, 6, len(ids))], 5, f"step {step} cull")
        else:
            set_bad_both(st, rm, ids[:4], f"step {step} set bad")
        new = []
        for p in rng.permutation(P)[:10]:
            p, s = int(p), int(rng.integers(0, K))
            if s not in rm.points[p].obs:
                new.append((p, s, int(rng.integers(0, 40))))
        if new:
            st.add_observations([a for a, _, _ in new], [b for _, b, _ in new], idx=[c for _, _, c in new])
            for a, b, c in new:
                assert rm.add_observation(a, b, c)
            assert_state(st, rm, f"step {step} add")
        s = int(rng.integers(0, K))
        g = st.process_new_keyframe(ks, s)
        action, added, _ = rm.process_new_keyframe(s)
        assert g.action.tolist() == action and g.added.tolist() == added, f"step {step} new keyframe"
        assert_state(st, rm, f"step {step} new keyframe")
    assert any(mp.bad for mp in rm.points) and any(not mp.bad and mp.obs for mp in rm.points)
    st.close()
    ks.close()


def test_downstream_calls_after_a_cull_and_a_drop_batch_equal_their_restatements(gpu_ctx):
    """The drift this closes: after MapPointCulling and the drops of one fit, the local map, the anchor lists and ProcessNewKeyFrame of
    the store equal local_map_ref, anchor_pairs_ref and keyframe_insert_ref run on the restated state."""
    slot, ks, st, rm, rng = _model_stores(gpu_ctx, 33, K=6, N=40, P=80, p_obs=0.8, p_bad_point=0.05)
    P = len(rm.points)
    for p, mp in enumerate(rm.points):                                # every point has a reference keyframe it observes, where it has any
        if mp.obs:
            mp.ref = sorted(mp.obs)[p % len(mp.obs)]
    st.set_reference_keyframes(np.arange(P), [mp.ref for mp in rm.points])
    ids = [int(p) for p in rng.permutation(P)[:40]]
    g = cull_both(st, rm, ids, [int(v) for v in rng.integers(0, 6, len(ids))], 6, "cull")
    assert g.counts.n_set_bad > 0 and g.counts.n_records > 0
    KF2 = 2                                                            # the drops of one fit: distinct points that observe KF2
    dropped = [p for p, mp in enumerate(rm.points) if KF2 in mp.obs][::2]
    g = erase_both(st, rm, dropped, [KF2] * len(dropped), True, "drop")
    assert g.counts.n_found == len(dropped) > 3 and g.counts.n_ref_moved > 0
    # Tracking::UpdateLocalMap
    frame_points = rm.kfs[slot].table
    want = rm.update_local_map(frame_points)
    got = st.update_local_map(frame_points)
    assert got.frame_bad.tolist() == want["frame_bad"].tolist() and got.local_kf.tolist() == want["local_kf"].tolist()
    assert got.votes.tolist() == want["votes"].tolist() and got.ref_kf == want["ref_kf"]
    assert st.local_points(got.n_local_points).tolist() == want["local_points"].tolist()
    # SchwarpDatabase::add
    for s in (slot, KF2):
        AR.assert_equal(st.keyframe_anchors(s, 1), rm.keyframe_anchors(s, 1))
    # LocalMapping::ProcessNewKeyFrame
    for s in (slot, KF2):
        g = st.process_new_keyframe(ks, s)
        action, added, _ = rm.process_new_keyframe(s)
        assert g.action.tolist() == action and g.added.tolist() == added
    w = rm.point_arrays()
    gp = st.get_points()
    for k in ("normal", "max_distance", "desc"):
        assert getattr(gp, k).tobytes() == w[k].tobytes(), k
    assert_state(st, rm, "after the new keyframes")
    st.close()
    ks.close()


def test_state_refusal_while_an_unindexed_live_record_exists(gpu_ctx):
    from defslam_amd import _lib
    rm, (pts, slots) = PE.small_scene()
    st = store_from(gpu_ctx, rm)
    st.add_observations([5], [2])                                      # without a key point index
    L, msg = gpu_ctx._L, lambda: gpu_ctx._L.dsh_last_error(gpu_ctx._h).decode()
    i32 = lambda v: np.array(v, np.int32)
    p, s, act = i32(pts), i32(slots), np.zeros(6, np.uint8)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    cc = _lib.PointEraseCountsC(7, 7, 7, 7, 7)
    assert L.dsh_point_store_erase_observations(st._h, 6, ip(p), ip(s), 1, None, C.byref(cc)) == STATE and "without a key point index" in msg()
    assert L.dsh_point_store_set_bad(st._h, 6, ip(p), C.byref(cc)) == STATE and "dsh_point_store_set_bad" in msg()
    assert L.dsh_point_store_cull(st._h, 6, ip(p), ip(s), 9, act.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(cc)) == STATE
    assert [getattr(cc, n) for n in PE.COUNT_NAMES] == [7] * 5
    assert rm.add_observation(5, 2)                                    # the read-backs work and report -1
    assert_state(st, rm, "nothing changed")
    assert st.observations([5]).of(0) == {0: 6, 1: 6, 2: -1}
    st.erase_observations([5], [2])                                    # the old erase takes it out of the count
    assert rm.erase_observation(5, 2)
    erase_both(st, rm, pts, slots, True, "after the unindexed record left")
    st.close()


def test_empty_batches_and_a_capacity_that_is_too_small(gpu_ctx):
    from defslam_amd import _lib
    rm, _ = PE.small_scene()
    st = store_from(gpu_ctx, rm)
    L = gpu_ctx._L
    for call in (lambda c: L.dsh_point_store_erase_observations(st._h, 0, None, None, 1, None, c), lambda c: L.dsh_point_store_set_bad(st._h, 0, None, c),
                 lambda c: L.dsh_point_store_cull(st._h, 0, None, None, 3, None, c)):
        cc = _lib.PointEraseCountsC(7, 7, 7, 7, 7)
        assert call(C.byref(cc)) == OK and [getattr(cc, n) for n in PE.COUNT_NAMES] == [0] * 5
    assert_state(st, rm, "empty batches")
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    ids, ptr, sl, ix, tot = np.arange(6, dtype=np.int32), np.full(7, -7, np.int32), np.full(16, -7, np.int32), np.full(16, -7, np.int32), np.zeros(1, np.int32)
    assert L.dsh_point_store_get_observations(st._h, 6, ip(ids), ip(ptr), 14, ip(sl), ip(ix), ip(tot)) == ARG
    assert tot[0] == 15 and "capacity 14 is too small" in L.dsh_last_error(gpu_ctx._h).decode()
    assert (ptr == -7).all() and (sl == -7).all() and (ix == -7).all()
    assert L.dsh_point_store_get_observations(st._h, 6, ip(ids), ip(ptr), 15, ip(sl), ip(ix), ip(tot)) == OK
    assert tot[0] == 15 and ptr.tolist() == [0, 3, 6, 7, 10, 13, 15] and sl[:15].tolist() == [0, 1, 2, 0, 1, 2, 2, 0, 1, 2, 0, 1, 2, 0, 1]
    assert ix[:15].tolist() == [0, 0, 0, 1, 5, 1, 2, 3, 3, 3, 4, 4, 4, 6, 6] and sl[15] == -7
    assert L.dsh_point_store_get_observations(st._h, 0, None, ip(ptr), 0, None, None, ip(tot)) == OK and tot[0] == 0 and ptr[0] == 0
    tab = np.full(8, -7, np.int32)
    assert L.dsh_point_store_get_keyframe_table(st._h, 1, 7, ip(tab)) == ARG and (tab == -7).all()
    assert L.dsh_point_store_get_keyframe_table(st._h, 1, 8, ip(tab)) == OK and tab.tolist() == rm.kfs[1].table
    assert L.dsh_point_store_get_keyframe_table(st._h, 3, 8, ip(tab)) == ARG
    # refusals that need a stored point: a slot outside the store, a repeated point; nothing changes
    cc = _lib.PointEraseCountsC(7, 7, 7, 7, 7)
    p, s = np.array([0, 1], np.int32), np.array([0, 3], np.int32)
    assert L.dsh_point_store_erase_observations(st._h, 2, ip(p), ip(s), 0, None, C.byref(cc)) == ARG
    assert "pair 1: keyframe slot outside the store" in L.dsh_last_error(gpu_ctx._h).decode()
    p = np.array([2, 4, 2], np.int32)
    assert L.dsh_point_store_set_bad(st._h, 3, ip(p), C.byref(cc)) == ARG and "point id 2 repeated in the batch" in L.dsh_last_error(gpu_ctx._h).decode()
    assert [getattr(cc, n) for n in PE.COUNT_NAMES] == [7] * 5
    assert_state(st, rm, "after the refusals")
    st.close()
