"""GPU tests of dsh_keyframe_anchors and the two store fields it reads (dsh_point_store_add_observations_indexed,
dsh_point_store_set_reference_keyframes / dsh_point_store_get_reference_keyframes): every output -- the anchors with their counts, the
pair and query lists, the own flags, has, n_no_ref -- equals (==) the sequential restatement tests/anchor_pairs_ref.py on the same map.
Integers: no tolerance anywhere.  The maps (anchor_pairs_ref.SCENES; tests/test_anchor_pairs_cpu.py checks that each holds every case):
70 key points and 5 keyframes (a wavefront boundary), 300 key points (a workgroup boundary of the ordered compaction), 76 keyframes with
at least 70 anchors (the anchor compaction crosses a ballot word).  Also here, because a host-only store stays empty: the refusals that
need a stored keyframe, point or record."""
import ctypes as C

import numpy as np
import pytest

import anchor_pairs_ref as A

pytestmark = pytest.mark.gpu

OK, ARG, STATE = 0, 1, 3


def store_from(ctx, rm, **caps):
    from defslam_amd import localmap
    st = localmap.MapPointStore(ctx, **caps)
    rm.fill(st, batches=3)
    return st


@pytest.fixture(scope="module")
def scenes():
    """Each map once, with the restatement's result: shared and left unchanged."""
    out = {}
    for name, (make, min_pairs) in A.SCENES.items():
        rm = make()
        out[name] = (rm, min_pairs, rm.keyframe_anchors(len(rm.kfs) - 1, min_pairs))
    return out


@pytest.mark.parametrize("name", sorted(A.SCENES))
def test_every_output_equals_the_restatement(gpu_ctx, scenes, name):
    """The store starts tiny, so points, keyframes, tables and the log (with the indices beside it) all grow between the adds and the
    call.  Then the same call with the anchors forced into chunks of three and of one, and with min_pairs 0 (every anchor listed,
    a == slot among them)."""
    rm, min_pairs, want = scenes[name]
    st = store_from(gpu_ctx, rm, points=2, keyframes=1, observations=2)
    slot = len(rm.kfs) - 1
    N = len(rm.kfs[slot].table)
    assert st.get_reference_keyframes().tolist() == rm.state()["ref"].tolist()
    g = st.keyframe_anchors(slot, min_pairs)
    A.assert_equal(g, want)
    for rows in (3, 1):
        A.assert_equal(st.keyframe_anchors(slot, min_pairs, max_matrix_bytes=4 * N * rows), want)
    all_listed = rm.keyframe_anchors(slot, 0)
    A.assert_equal(st.keyframe_anchors(slot, 0), all_listed)
    A.assert_equal(st.keyframe_anchors(slot, 0, max_matrix_bytes=4 * N * 2), all_listed)
    a = all_listed["anchor_slot"].index(slot)
    ps = slice(all_listed["pair_ptr"][a], all_listed["pair_ptr"][a + 1])
    assert all_listed["pair_idx1"][ps] == all_listed["pair_idx2"][ps] != []
    st.close()


def test_min_pairs_boundary(gpu_ctx):
    """Anchors with exactly min_pairs - 1 and min_pairs pairs: the first keeps its entry and contributes nothing."""
    m = 20
    rm = A.threshold_map(m)
    st = store_from(gpu_ctx, rm)
    g = st.keyframe_anchors(2, m)
    A.assert_equal(g, rm.keyframe_anchors(2, m))
    assert g.anchor_pairs.tolist() == [m - 1, m] and g.pair_ptr.tolist() == [0, 0, m] and not g.pair_own[0] and g.pair_own[1:].all()
    A.assert_equal(st.keyframe_anchors(2, m - 1), rm.keyframe_anchors(2, m - 1))
    A.assert_equal(st.keyframe_anchors(2, m + 1), rm.keyframe_anchors(2, m + 1))
    st.close()


def test_mutations_after_the_first_call_are_seen(gpu_ctx, scenes):
    """The call keeps nothing: a bad flag, an erased record, a new observation and a changed reference keyframe show in the next one; an
    older keyframe as `slot` works too, and so does an empty keyframe."""
    rm = A.SCENES["n70_k5"][0]()
    st = store_from(gpu_ctx, rm)
    slot = len(rm.kfs) - 1
    A.assert_equal(st.keyframe_anchors(slot, 5), rm.keyframe_anchors(slot, 5))
    held = [p for p in rm.kfs[slot].table if p >= 0 and not rm.points[p].bad and slot in rm.points[p].obs]
    rm.points[held[0]].bad = True
    st.set_points_bad([held[0]])
    rm.erase_observation(held[1], slot)
    st.erase_observations([held[1]], [slot])
    late = next(i for i, p in enumerate(rm.kfs[slot].table) if p >= 0 and not rm.points[p].bad and not any(r[:2] == [p, slot] for r in rm.log))
    assert rm.add_observation(rm.kfs[slot].table[late], slot, late)
    st.add_observations([rm.kfs[slot].table[late]], [slot], idx=[late])
    rm.points[held[2]].ref = 0 if rm.points[held[2]].ref != 0 else 1
    st.set_reference_keyframes([held[2]], [rm.points[held[2]].ref])
    assert st.get_reference_keyframes([held[2], held[3]]).tolist() == [rm.points[held[2]].ref, rm.points[held[3]].ref]
    A.assert_equal(st.keyframe_anchors(slot, 5), rm.keyframe_anchors(slot, 5))
    A.assert_equal(st.keyframe_anchors(1, 2), rm.keyframe_anchors(1, 2))
    e = rm.add_keyframe([])
    assert st.add_keyframe(np.zeros(0, np.int32)) == e
    g = st.keyframe_anchors(e, 0)
    A.assert_equal(g, rm.keyframe_anchors(e, 0))
    assert g.anchor_slot.shape == (0,) and g.pair_ptr.tolist() == [0] and g.query_ptr.tolist() == [0]
    st.close()


def raw_lists(ca, cp, cq):
    from defslam_amd import _lib
    a = {n: np.full(max(c, 1) + 1, -7, np.int32) for n, c in (("anchor_slot", ca), ("anchor_count", ca), ("anchor_pairs", ca), ("pair_ptr", ca),
                                                                ("query_ptr", ca), ("pair_idx1", cp), ("pair_idx2", cp), ("pair_point", cp),
                                                                ("query_idx1", cq), ("query_point", cq))}
    own = np.full(max(cp, 1), 9, np.uint8)
    r = _lib.AnchorListsC(anchor_capacity=ca, pair_capacity=cp, query_capacity=cq, pair_own=own.ctypes.data_as(C.POINTER(C.c_uint8)),
                          **{n: v.ctypes.data_as(C.POINTER(C.c_int32)) for n, v in a.items()})
    return r, a, own


def test_refusals_that_need_a_filled_store(gpu_ctx, scenes):
    """Lists that do not fit: DSH_ERR_ARG, the needed sizes reported and no array written.  An index outside the keyframe, a repeated id,
    a slot outside the store: DSH_ERR_ARG and nothing stored."""
    from defslam_amd import sft
    rm, min_pairs, want = scenes["n70_k5"]
    st = store_from(gpu_ctx, rm)
    L, slot = gpu_ctx._L, len(rm.kfs) - 1
    msg = lambda: L.dsh_last_error(gpu_ctx._h).decode()
    A_, NP, NQ = len(want["anchor_slot"]), len(want["pair_idx1"]), len(want["query_idx1"])
    assert NP > 1 and NQ > 1
    for ca, cp, cq in ((A_ - 1, NP, NQ), (A_, NP - 1, NQ), (A_, NP, NQ - 1), (0, 0, 0)):
        r, a, own = raw_lists(ca, cp, cq)
        assert L.dsh_keyframe_anchors(st._h, slot, min_pairs, C.byref(r)) == ARG and "do not fit" in msg()
        assert (r.n_anchors, r.n_pairs, r.n_queries) == (A_, NP, NQ)
        assert all((v == -7).all() for v in a.values()) and (own == 9).all()
    r, a, own = raw_lists(A_, NP, NQ)                                                # exactly enough
    assert L.dsh_keyframe_anchors(st._h, slot, min_pairs, C.byref(r)) == OK
    assert a["pair_idx1"][:NP].tolist() == want["pair_idx1"] and a["query_ptr"][:A_ + 1].tolist() == want["query_ptr"]
    r, a, own = raw_lists(A_, NP, NQ)
    r.pair_idx2 = None
    assert L.dsh_keyframe_anchors(st._h, slot, min_pairs, C.byref(r)) == ARG and "NULL" in msg()
    r, a, own = raw_lists(A_, NP, NQ)
    r.pair_capacity = -1
    assert L.dsh_keyframe_anchors(st._h, slot, min_pairs, C.byref(r)) == ARG and "capacity" in msg()
    r, a, own = raw_lists(A_, NP, NQ)
    assert L.dsh_keyframe_anchors(st._h, slot + 1, min_pairs, C.byref(r)) == ARG and "slot outside" in msg()
    assert L.dsh_keyframe_anchors(st._h, slot, -1, C.byref(r)) == ARG and "min_pairs" in msg()
    free = next(p for p in range(len(rm.points)) if not any(r[:2] == [p, 0] for r in rm.log))
    n0 = len(rm.kfs[0].table)
    for idx in (n0, -1):
        with pytest.raises(sft.DshError, match="index outside the keyframe's key points"):
            st.add_observations([free], [0], idx=[idx])
    with pytest.raises(sft.DshError, match="slot outside the store"):
        st.add_observations([free], [slot + 1], idx=[0])
    with pytest.raises(sft.DshError, match="repeated in the batch"):
        st.add_observations([free, free], [0, 0], idx=[0, 1])
    with pytest.raises(sft.DshError, match="repeated in the batch"):
        st.set_reference_keyframes([3, 3], [0, 1])
    with pytest.raises(sft.DshError, match="neither -1 nor a slot"):
        st.set_reference_keyframes([3], [slot + 1])
    with pytest.raises(sft.DshError, match="repeated in the batch"):
        st.get_reference_keyframes([3, 3])
    assert st.get_reference_keyframes().tolist() == rm.state()["ref"].tolist()     # nothing was stored
    A.assert_equal(st.keyframe_anchors(slot, min_pairs), want)
    st.close()


def test_records_without_an_index_are_a_state_error(gpu_ctx):
    """A store that has only ever used dsh_mpdb_add_observations: DSH_ERR_STATE, nothing written.  One such record among indexed ones is
    enough; erasing it, or clearing the store, lifts the refusal."""
    from defslam_amd import localmap
    rm = A.threshold_map(4)
    L = gpu_ctx._L
    st = localmap.MapPointStore(gpu_ctx)
    P = len(rm.points)
    z = np.zeros((P, 3), np.float32)
    st.add_points(z, z, np.ones(P, np.float32), np.zeros((P, 32), np.uint8))
    for kf in rm.kfs:
        st.add_keyframe(np.array(kf.table, np.int32))
    log = np.array(rm.log, np.int32)                                                 # no erased record in this map
    st.add_observations(log[:, 0], log[:, 1])
    st.set_reference_keyframes(np.arange(P), rm.state()["ref"])
    r, a, own = raw_lists(8, 64, 64)
    assert L.dsh_keyframe_anchors(st._h, 2, 4, C.byref(r)) == STATE
    assert f"{len(rm.log)} live observation records without a key point index" in L.dsh_last_error(gpu_ctx._h).decode()
    assert all((v == -7).all() for v in a.values()) and (own == 9).all() and r.n_anchors == 0
    st.clear()
    rm.fill(st, batches=3)
    A.assert_equal(st.keyframe_anchors(2, 4), rm.keyframe_anchors(2, 4))
    q = rm.add_point(ref=0)
    st.add_points(np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), [1.0], np.zeros((1, 32), np.uint8))
    st.add_observations([q], [0])                                                    # the old call: no index
    assert L.dsh_keyframe_anchors(st._h, 2, 4, C.byref(r)) == STATE
    st.erase_observations([q], [0])                                                  # erasing the record takes it out of the count
    A.assert_equal(st.keyframe_anchors(2, 4), rm.keyframe_anchors(2, 4))
    st.close()


def test_points_of_a_template_switch_carry_both_fields(ctx_switch):
    """After dsh_template_switch the created points have the switch's keyframe as reference keyframe and their observation records the
    key point new_idx: a later keyframe that observes them pairs them with idx1 == new_idx."""
    from defslam_amd import localmap
    from test_template_switch_cpu import make_scene
    from test_template_switch_gpu import build_template, kf_store_from_scene
    ctx = ctx_switch
    sc, (xs, ys) = make_scene("last")
    P, r = sc["xyz"].shape[0], sc["ref_slot"]
    rm = A.AnchorRefMap()
    st = localmap.MapPointStore(ctx, points=2, keyframes=1, observations=2)
    st.add_points(sc["xyz"], sc["normal"], sc["max_distance"], sc["desc"], sc["bad"])
    for p in range(P):
        rm.add_point(bad=sc["bad"][p])
    for k in range(sc["tables"].shape[0]):
        assert st.add_keyframe(sc["tables"][k], sc["parents"][k], sc["kf_bad"][k]) == rm.add_keyframe(sc["tables"][k]) == k
    idx = []
    for p, k in zip(sc["obs_point"], sc["obs_kf"]):                                  # the scene's observations: the entry that holds the point, else 0
        hit = np.nonzero(sc["tables"][k] == p)[0]
        idx.append(int(hit[0]) if len(hit) else 0)
        assert rm.add_observation(int(p), int(k), idx[-1])
    st.add_observations(sc["obs_point"], sc["obs_kf"], idx=idx)
    ks = kf_store_from_scene(ctx, sc)
    build_template(ctx, sc, xs, ys)
    g = st.switch_template(ks, r, localmap.KeyFramePoints(sc["rows"], sc["cols"], sc["kp"]), sc["surface_pts"], sc["Twc"])
    assert g.n_new >= 10
    new = np.arange(g.first_id, g.n_points)
    assert st.get_reference_keyframes(new).tolist() == [r] * g.n_new
    assert (st.get_reference_keyframes(np.arange(P)) == -1).all()
    for p, i in zip(new, g.new_idx):                                                 # the mirror follows the switch
        assert rm.add_point(ref=r) == p
        rm.kfs[r].table[int(i)] = int(p)
        assert rm.add_observation(int(p), r, int(i))
    n2 = g.n_new + 7                                                                 # a later keyframe that observes the new points, reversed
    table = np.full(n2, -1, np.int32)
    table[:g.n_new] = new[::-1]
    k2 = st.add_keyframe(table)
    assert rm.add_keyframe(table) == k2
    for i in range(g.n_new):
        assert rm.add_observation(int(table[i]), k2, i)
    st.add_observations(table[:g.n_new], [k2] * g.n_new, idx=np.arange(g.n_new))
    got = st.keyframe_anchors(k2, min_pairs=10)
    A.assert_equal(got, rm.keyframe_anchors(k2, 10))
    assert got.anchor_slot.tolist() == [r] and got.anchor_count.tolist() == [g.n_new]
    assert got.pair_idx1.tolist() == g.new_idx[::-1].tolist() and got.pair_idx2.tolist() == list(range(g.n_new)) and got.pair_own.all()
    ks.close()
    st.close()


@pytest.fixture(scope="module")
def ctx_switch():
    """A context of its own: the template switch replaces the context's template."""
    from defslam_amd import sft
    c = sft.Context(0)
    yield c
    c.close()
