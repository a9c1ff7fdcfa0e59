"""GPU tests of dsh_keyframe_process_new and dsh_point_store_upkeep.  Every compared value is exact: integers, or float32 bit patterns
compared as bytes; there are no tolerances.  The yardsticks are the store model tests/keyframe_insert_ref.py, which drives the sequential
restatement tests/mappoint_ref.py by ascending slot, and the existing dsh_mappoint_update fed an ascending-slot CSR.

The big scene (keyframe_insert_ref.big_scene) has 132 keyframes with 6 key points each and more than 24 000 log records, so the log
kernels stride; its points reach every lane-group class (8, 16, 32, 64 lanes), the small/large hand-over (64 / 65 observations) and one,
two and three blocks of 64 election rows (64, 128, 129)."""
import ctypes as C

import numpy as np
import pytest

import keyframe_insert_ref as KI

pytestmark = pytest.mark.gpu

OK, ARG, STATE = 0, 1, 3


def stores_from(ctx, m, **caps):
    from defslam_amd import localmap, mappoint
    ks = mappoint.KeyFrameStore(ctx, 2)                                             # it grows, the resident octaves and pyramids too
    st = localmap.MapPointStore(ctx, **caps)
    m.fill(st, ks)
    return ks, st


def check_store(st, m):
    """dsh_point_store_get_points of EVERY point and n_obs against the model."""
    g, w = st.get_points(), m.point_arrays()
    for k in ("xyz", "normal", "max_distance", "desc"):
        assert getattr(g, k).tobytes() == w[k].tobytes(), k
    assert g.bad.tolist() == w["bad"].tolist()
    assert st.get_state().n_obs.tolist() == m.state()["n_obs"].tolist()
    return g


def process_both(st, ks, m, slot):
    """One keyframe on the store and on the model: actions, added points in order, counts."""
    g = st.process_new_keyframe(ks, slot)
    action, added, status = m.process_new_keyframe(slot)
    assert g.action.tolist() == action and g.added.tolist() == added
    assert (g.n_empty, g.n_bad, g.n_added, g.n_recent) == tuple(action.count(a) for a in (KI.EMPTY, KI.BAD_POINT, KI.ADDED, KI.RECENT))
    assert g.n_no_good_desc == sum(1 for s in status if s & KI.NO_GOOD_DESC) and g.n_no_ref == sum(1 for s in status if s & KI.NO_REF)
    assert g.first_record == len(m.log) - len(added)
    return g


def test_big_scene_every_count_class_log_order_and_the_second_call(gpu_ctx):
    """Cases 2-5, 7 and 10 of the issue on one store: observation counts 1, 2, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129 after the add;
    records appended by descending slot with blanked ones in between and a pair erased and added again with another index; a point held
    twice, a point already observing, a bad point, an empty entry; four bad keyframes in the election; a reference keyframe that is not
    observed and a reference of -1; then every call once more, which adds nothing and changes nothing."""
    from defslam_amd import sft
    m, nm = KI.big_scene()
    assert len(m.log) >= 24000 and len(m.kfs) == 132 and all(len(k.table) == 6 for k in m.kfs)
    assert sum(1 for r in m.log if not r[3]) >= 20
    ks, st = stores_from(gpu_ctx, m, points=8, keyframes=4, observations=64)
    check_store(st, m)
    before = st.get_points()
    gA = process_both(st, ks, m, nm["A"])
    gB = process_both(st, ks, m, nm["B"])
    assert gA.n_added == gB.n_added == 6 and gB.n_no_ref == 1
    assert sorted(len(m.observations(p)) for p in nm["count_pts"]) == [1, 2, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129]
    p, s, j = nm["again"]
    assert dict(m.observations(p))[s] == j
    g = check_store(st, m)
    # the point with two observations: both medians are 0, the lower slot wins although its record is not the last
    p2 = nm["count_pts"][1]
    (s0, j0), (s1, _) = m.observations(p2)
    assert s1 == nm["A"] and not m.kfs[s0].bad and g.desc[p2].tobytes() == m.kfs[s0].desc[j0].tobytes()
    # the reference of -1 left normal and range alone and elected a descriptor
    p9 = nm["count_pts"][8]
    assert g.normal[p9].tobytes() == before.normal[p9].tobytes() and g.max_distance[p9] == before.max_distance[p9]
    assert g.desc[p9].tobytes() != before.desc[p9].tobytes()
    gC = process_both(st, ks, m, nm["C"])
    assert gC.action.tolist() == [KI.ADDED, KI.RECENT, KI.BAD_POINT, KI.EMPTY, KI.RECENT, KI.ADDED] and gC.added.tolist() == [nm["twice"], nm["all_bad"]]
    g = check_store(st, m)
    assert g.desc[nm["already"]].tobytes() == before.desc[nm["already"]].tobytes()   # action 3: its stale descriptor is untouched
    assert g.desc[nm["all_bad"]].tobytes() == m.kfs[nm["C"]].desc[5].tobytes()         # the one good keyframe it observes now
    # the mirror knows the records: adding one again is refused, erasing it works, the anchors see them
    with pytest.raises(sft.DshError, match="already observes"):
        st.add_observations([nm["twice"]], [nm["C"]], idx=[0])
    a = st.keyframe_anchors(nm["C"], 0)
    assert a.n_no_ref == 0 and a.anchor_slot.shape[0] >= 1 and (a.pair_idx2[a.pair_point == nm["twice"]] == 0).all()
    # a second call on each slot
    for slot in (nm["A"], nm["B"], nm["C"]):
        g2 = process_both(st, ks, m, slot)
        assert g2.n_added == 0 and KI.ADDED not in g2.action.tolist()
    check_store(st, m)
    st.erase_observations([nm["twice"]], [nm["C"]])
    m.erase_observation(nm["twice"], nm["C"])
    g3 = process_both(st, ks, m, nm["C"])
    assert g3.added.tolist() == [nm["twice"]]
    check_store(st, m)
    # the upkeep by ids on the same store: a point without observations, a bad one, the large ones again, descriptor or geometry alone
    ids = [nm["no_obs"], nm["bad_point"], nm["plain"]] + nm["count_pts"]
    for what in (KI.DESCRIPTOR, KI.NORMAL_DEPTH, KI.BOTH):
        u = st.upkeep(ks, ids, what=what)
        want = m.upkeep(ids, what)
        assert u.status.tolist() == want and want[:2] == [KI.NO_OBS, KI.SKIPPED_BAD]
        assert (u.n_selected, u.n_no_obs, u.n_bad, u.n_no_ref) == (len(ids) - 1, 1, 1, 1)
        check_store(st, m)
    st.close()
    ks.close()


def test_strides_of_the_work_lists_and_ties_in_every_class(gpu_ctx):
    """More than 4096 selected points, so a wavefront of the sort kernel takes a second point, and more than 1024 blocks of large
    points, so a wavefront of the large kernel takes a second block.  Case 6 of the issue in every class: points with 12, 24, 48 and 124
    observations whose rows alternate between two descriptors -- every median is 0, within a lane group and across the two blocks of
    the large path, and the lowest slot wins although the highest holds the other descriptor."""
    m, nm = KI.big_scene(fillers=350, singles=4200, ties=(12, 24, 48, 124))
    ks, st = stores_from(gpu_ctx, m)
    ids = list(range(len(m.points)))
    large = [p for p in ids if not m.points[p].bad and len(m.observations(p)) > 64]
    assert len(ids) > 4096 and sum(1 + -(-sum(1 for s, _ in m.observations(p) if not m.kfs[s].bad) // 64) for p in large) > 1024
    u = st.upkeep(ks, ids)
    assert u.status.tolist() == m.upkeep(ids) and u.n_selected == len(ids) - u.n_bad
    g = check_store(st, m)
    for p, slots, two in nm["ties"]:
        assert [s for s, _ in m.observations(p)] == slots and len(slots) % 2 == 0 and g.desc[p].tobytes() == two[0].tobytes() != two[1].tobytes()
    # the embedded selection over the same long store: every point gets a facet first
    st.set_embedding(ids, np.tile(np.int32([0, 1, 2]), (len(ids), 1)), np.tile([1.0, 0.0, 0.0], (len(ids), 1)))
    e = st.upkeep(ks, what=KI.NORMAL_DEPTH, embedded=True)
    assert e.n_selected == sum(1 for p in ids if not m.points[p].bad) > 4096
    m.upkeep(ids, KI.NORMAL_DEPTH)
    check_store(st, m)
    st.close()
    ks.close()


@pytest.mark.parametrize("table", [[], [4]])
def test_keyframes_with_no_and_one_key_point(gpu_ctx, table):
    m, slot = KI.random_model(11, K=5, N=6, P=12, new_table=table)
    ks, st = stores_from(gpu_ctx, m)
    m.points[4].bad = False
    st.set_points_bad([4], [0])
    g = process_both(st, ks, m, slot)
    assert g.n_added == len(table)
    check_store(st, m)
    st.close()
    ks.close()


def wide_table(n):
    """A table of n entries over n + 10 points: every ninth entry empty, the point of entry 3 again in entry 66 and in the entry before
    the last, the point of entry 70 % n again in the last."""
    t = [int(p) for p in np.random.default_rng(n).permutation(n + 10)[:n]]
    for i in range(8, n, 9):
        t[i] = -1
    t[66], t[n - 2], t[n - 1] = t[3], t[3], t[70 % n]
    return t


@pytest.mark.parametrize("n", [70, 300])
def test_a_table_that_crosses_the_wavefronts_and_tiles_of_the_classify_kernel(gpu_ctx, n):
    """A new keyframe of 70 and one of 300 key points: the ordered compaction of the added entries runs over more than one wavefront and
    more than one tile of 256 entries.  Added entries lie on both sides of entry 64 and of entry 256; a point is held by three entries,
    some are bad, one observes the keyframe already."""
    table = wide_table(n)
    m, slot = KI.random_model(40 + n, K=6, N=40, P=n + 10, p_bad_point=0.1, new_table=table)
    ks, st = stores_from(gpu_ctx, m, points=8, keyframes=2, observations=16)
    R0 = len(m.log)
    g = process_both(st, ks, m, slot)
    action = g.action.tolist()
    added_at = [i for i, a in enumerate(action) if a == KI.ADDED]
    for edge in (64, 256)[:1 if n == 70 else 2]:
        assert {edge - 1, edge, edge + 1} & set(added_at) and min(added_at) < edge - 1 and max(added_at) > edge + 1
    assert action.count(KI.BAD_POINT) >= 3 and action.count(KI.EMPTY) == len(range(8, n, 9)) and action[1] == KI.RECENT
    assert not m.points[table[3]].bad and action[3] == KI.ADDED and action[66] == action[n - 2] == KI.RECENT
    # the records the call appended, in entry order, and every point's observations read back
    assert [(r[0], r[1], r[2]) for r in m.log[R0:]] == [(table[i], slot, i) for i in added_at] and g.added.tolist() == [table[i] for i in added_at]
    o = st.observations()
    for p in range(n + 10):
        assert list(o.of(p).items()) == sorted(m.observations(p)), p
    assert st.keyframe_table(slot).tolist() == table
    check_store(st, m)
    g2 = process_both(st, ks, m, slot)                                   # again: nothing is added, the added entries are recent now
    assert g2.n_added == 0 and g2.n_recent == g.n_recent + g.n_added
    check_store(st, m)
    st.close()
    ks.close()


def test_bad_keyframes_some_all_and_the_statuses_by_id(gpu_ctx):
    """Case 5: the election skips bad keyframes, the normal does not; with every observing keyframe bad the descriptor stays and the
    geometry is still computed.  Case 7: no reference keyframe.  The point store's flag is the one read, not the keyframe store's."""
    m, slot = KI.random_model(5, K=9, N=6, P=14, p_bad_kf=0.0, p_bad_point=0.0, p_obs=0.8)
    ks, st = stores_from(gpu_ctx, m)
    p = max(range(14), key=lambda q: len(m.observations(q)))
    obs = m.observations(p)
    assert len(obs) >= 3
    m.points[p].ref = obs[0][0]
    st.set_reference_keyframes([p], [obs[0][0]])
    ids = list(range(14))
    for n_bad in (1, len(obs)):
        for s, _ in obs[:n_bad]:
            m.kfs[s].bad = True
            st.set_keyframe_bad(s, True)                                             # the keyframe store is not told
        before = st.get_points([p])
        u = st.upkeep(ks, ids)
        assert u.status.tolist() == m.upkeep(ids)
        assert bool(u.status[p] & KI.NO_GOOD_DESC) == (n_bad == len(obs)) and u.n_no_good_desc >= (n_bad == len(obs))
        g = check_store(st, m)
        if n_bad == len(obs):
            assert g.desc[p].tobytes() == before.desc[0].tobytes()
    m.points[p].ref = -1
    st.set_reference_keyframes([p], [-1])
    u = st.upkeep(ks, [p], what=KI.NORMAL_DEPTH)
    assert u.status.tolist() == m.upkeep([p], KI.NORMAL_DEPTH) == [KI.NO_GOOD_DESC | KI.NO_REF] and u.n_no_ref == 1
    check_store(st, m)
    st.close()
    ks.close()


def test_the_log_grows_inside_the_call(gpu_ctx):
    """Case 8: observation_capacity smaller than the records the call appends."""
    from defslam_amd import sft
    m, slot = KI.random_model(2, K=1, N=6, P=8, p_obs=0.5, p_bad_point=0.0, new_table=[0, 1, 2, 3, 4, 5])
    live = sum(1 for r in m.log if r[3])
    ks, st = stores_from(gpu_ctx, m, points=8, keyframes=2, observations=max(live, 1))
    g = process_both(st, ks, m, slot)
    assert g.n_added == 5 and g.action.tolist()[1] == KI.RECENT and live >= 1          # the store had room for no record more
    check_store(st, m)
    st.erase_observations([0], [slot])
    m.erase_observation(0, slot)
    with pytest.raises(sft.DshError, match="already observes"):
        st.add_observations([2], [slot], idx=[2])
    assert process_both(st, ks, m, slot).added.tolist() == [0]
    check_store(st, m)
    st.close()
    ks.close()


def test_equals_the_three_call_path(gpu_ctx):
    """Case 9: two stores with the same scene; one through dsh_point_store_add_observations_indexed, dsh_mappoint_update with an
    ascending-slot CSR and dsh_mpdb_update_points, one through dsh_keyframe_process_new.  Every point, n_obs, the anchors' lists and the
    local map's votes are identical."""
    from defslam_amd import mappoint
    m, slot = KI.random_model(21, K=40, N=6, P=60, p_obs=0.9, p_bad_point=0.05, p_bad_kf=0.1)
    for pt in m.points:
        pt.ref = max(pt.ref, 0)                                                     # dsh_mappoint_update needs a reference keyframe
    ks, new = stores_from(gpu_ctx, m)
    ks2, old = stores_from(gpu_ctx, m)
    g = new.process_new_keyframe(ks, slot)
    # today's path, decided on the host objects
    table, seen, add = m.kfs[slot].table, set(), []
    for i, p in enumerate(table):
        if p >= 0 and not m.points[p].bad and not m.live(p, slot) and p not in seen:
            seen.add(p)
            add.append((p, i))
    assert g.added.tolist() == [p for p, _ in add] and len(add) >= 3
    old.add_observations([p for p, _ in add], [slot] * len(add), idx=[i for _, i in add])
    for p, i in add:
        assert m.add_observation(p, slot, i)
    ids = [p for p, _ in add]
    cur = old.get_points(ids)
    u = mappoint.update(gpu_ctx, ks2, cur.xyz, [m.observations(p) for p in ids], [m.points[p].ref for p in ids], desc=cur.desc, normal=cur.normal,
                        max_distance=cur.max_distance)
    old.update_points(ids, normal=u.normal, max_distance=u.max_distance, desc=u.desc)
    a, b = new.get_points(), old.get_points()
    for k in ("xyz", "normal", "max_distance", "desc", "bad"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    assert new.get_state().n_obs.tolist() == old.get_state().n_obs.tolist() == m.state()["n_obs"].tolist()
    x, y = new.keyframe_anchors(slot, 1), old.keyframe_anchors(slot, 1)
    for k in x.__dataclass_fields__:
        assert np.asarray(getattr(x, k)).tolist() == np.asarray(getattr(y, k)).tolist(), k
    assert x.pair_point.shape[0] > 0 and x.anchor_slot.shape[0] > 1
    fp = np.array(table, np.int32)
    la, lb = new.update_local_map(fp), old.update_local_map(fp)
    assert la.votes.tolist() == lb.votes.tolist() and la.local_kf.tolist() == lb.local_kf.tolist() and la.ref_kf == lb.ref_kf
    assert slot in la.local_kf.tolist() and la.n_local_points == lb.n_local_points
    for s_ in (new, old):
        s_.close()
    ks.close()
    ks2.close()


def test_embedded_upkeep_after_a_template_switch(gpu_ctx):
    """Case 11: DSH_UPKEEP_EMBEDDED with DSH_MP_NORMAL_DEPTH after switch_template equals the caller-side path -- positions read back,
    dsh_mappoint_update with DSH_MP_NORMAL_DEPTH, dsh_mpdb_update_points -- and the model.  Then ids that repeat or leave the store."""
    from defslam_amd import localmap, mappoint, sft, synth
    ctx = sft.Context(0)                                                             # its own context: the test replaces the template
    m, _ = KI.random_model(31, K=5, N=6, P=16, p_obs=0.7, p_bad_kf=0.2)
    for p in range(3):
        m.points[p].xyz = np.float32([50, 50, 5])                                    # outside the template unless the keyframe moves them
    r = 2
    xs = ys = 7
    gx, gy = np.meshgrid(np.linspace(-3, 3, xs), np.linspace(-3, 3, ys), indexing="ij")
    nodes = np.stack([gx.ravel(), gy.ravel(), np.full(xs * ys, 5.0)], 1)
    ctx.template_build(nodes, synth.regular_triangulation(xs, ys))
    rng = np.random.default_rng(0)
    kf = localmap.KeyFramePoints(48, 64, np.float32([[5 + 9 * i, 7 + 6 * i] for i in range(6)]))
    surf = np.concatenate([rng.uniform(-2, 2, (6, 2)), np.full((6, 1), 5.0)], 1).astype(np.float32)
    stores = [stores_from(ctx, m) for _ in range(2)]
    sw = [st.switch_template(ks, r, kf, surf, np.eye(4, dtype=np.float32)) for ks, st in stores]
    assert sw[0].n_embedded == sw[1].n_embedded >= 3 and sw[0].new_idx.tolist() == sw[1].new_idx.tolist()
    (ks, st), (ks2, st2) = stores
    # the model follows the switch from the store's own read-backs
    pts, ref = st.get_points(), st.get_reference_keyframes()
    for j, i in enumerate(sw[0].new_idx.tolist()):
        q = m.add_point(pts.xyz[sw[0].first_id + j], pts.normal[sw[0].first_id + j], pts.max_distance[sw[0].first_id + j], pts.desc[sw[0].first_id + j], ref=r)
        assert q == sw[0].first_id + j and ref[q] == r
        assert m.add_observation(q, r, i)
        m.kfs[r].table[i] = q
    for p in range(len(m.points)):
        m.points[p].xyz = pts.xyz[p].copy()
    has_facet = (st.get_embedding()[0][:, 0] >= 0).tolist()
    ids = m.embedded_ids(has_facet)
    assert 0 < len(ids) < len(m.points) and sw[0].n_embedded == len(ids)
    u = st.upkeep(ks, what=KI.NORMAL_DEPTH, embedded=True)
    want = m.upkeep(ids, KI.NORMAL_DEPTH)
    assert u.status is None and u.n_selected == len(ids) and u.n_bad == 0
    assert (u.n_no_obs, u.n_no_ref) == (sum(1 for s in want if s & KI.NO_OBS), sum(1 for s in want if s & KI.NO_REF))
    check_store(st, m)
    # the caller-side path on the second store
    work = [p for p in ids if m.observations(p) and m.points[p].ref >= 0]
    xyz = st2.get_state(work).xyz
    cur = st2.get_points(work)
    res = mappoint.update(ctx, ks2, xyz, [m.observations(p) for p in work], [m.points[p].ref for p in work], what=mappoint.NORMAL_DEPTH, normal=cur.normal,
                          max_distance=cur.max_distance)
    st2.update_points(work, normal=res.normal, max_distance=res.max_distance)
    a, b = st.get_points(), st2.get_points()
    for k in ("xyz", "normal", "max_distance", "desc", "bad"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    for bad_ids, part in (([1, 1], "repeated"), ([0, len(m.points)], "outside the store"), ([-1], "outside the store")):
        with pytest.raises(sft.DshError, match=part):
            st.upkeep(ks, bad_ids)
    check_store(st, m)
    for ks_, st_ in stores:
        st_.close()
        ks_.close()
    ctx.close()


def test_refusals_that_need_stored_data(gpu_ctx):
    """Case 12 and the keyframe store's own refusals: decided on the host mirrors, nothing changed."""
    from defslam_amd import _lib, localmap, mappoint, sft
    m, slot = KI.random_model(4, K=4, N=6, P=10)
    ks, st = stores_from(gpu_ctx, m)
    L = gpu_ctx._L
    msg = lambda: L.dsh_last_error(gpu_ctx._h).decode()
    pc, uc = _lib.KeyframeProcessCountsC(), _lib.PointUpkeepCountsC()

    def both(kfdb, want, part):
        pin = _lib.KeyframeProcessInputC(kfdb, slot)
        assert L.dsh_keyframe_process_new(st._h, C.byref(pin), None, None, C.byref(pc)) == want and "dsh_keyframe_process_new" in msg() and part in msg(), msg()
        uin = _lib.PointUpkeepInputC(kfdb, 3, _lib.DSH_UPKEEP_EMBEDDED, 0, None)
        assert L.dsh_point_store_upkeep(st._h, C.byref(uin), None, C.byref(uc)) == want and "dsh_point_store_upkeep" in msg() and part in msg(), msg()
    both(None, ARG, "kfdb is NULL")
    # a live record without a key point index
    free = next(p for p in range(10) if not m.live(p, 0))
    st.add_observations([free], [0])
    both(ks._h, STATE, "without a key point index")
    st.erase_observations([free], [0])
    assert m.add_observation(free, 0, 0)                                             # the blanked record stays in the log
    m.erase_observation(free, 0)
    # fewer keyframes than the point store, then an N that differs
    short = mappoint.KeyFrameStore(gpu_ctx, 2)
    k0 = m.kfs[0]
    short.add(mappoint.MpKeyFrame(k0.Ow, k0.desc, k0.octave, k0.scale_factors))
    both(short._h, ARG, "fewer keyframes")
    for k in m.kfs[1:-1]:
        short.add(mappoint.MpKeyFrame(k.Ow, k.desc, k.octave, k.scale_factors))
    k = m.kfs[-1]
    short.add(mappoint.MpKeyFrame(k.Ow, k.desc[:-1], k.octave[:-1], k.scale_factors))
    both(short._h, ARG, "keyframe %d has another N" % slot)
    short.close()
    # an octave >= levels anywhere in the keyframe store
    over = mappoint.KeyFrameStore(gpu_ctx, 2)
    for s, k in enumerate(m.kfs):
        over.add(mappoint.MpKeyFrame(k.Ow, k.desc, np.where(np.arange(len(k.octave)) == 2, len(k.scale_factors), k.octave) if s == 1 else k.octave,
                                     k.scale_factors))
    both(over._h, ARG, "keyframe 1 has an octave >= levels")
    over.close()
    # another context's keyframe store
    ctx2 = sft.Context(0)
    other = mappoint.KeyFrameStore(ctx2, 2)
    both(other._h, ARG, "another context")
    other.close()
    ctx2.close()
    check_store(st, m)                                                               # nothing changed
    process_both(st, ks, m, slot)
    check_store(st, m)
    st.close()
    ks.close()
