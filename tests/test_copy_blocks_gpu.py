"""GPU tests of the empty paths of the one-copy blocks (UpBlock / DownBlock of defslam_amd/csrc/dsh_ctx.h) that no other test reaches: a
download block without a slice, one with a single slice among absent ones, a search without queries, an early return in front of the
blocks, an upload block whose unselected slices are empty; and of what a block hands out to the caller: one output among absent ones with
guard entries behind it, lists shorter than their capacity, a refusal after the download that leaves every array, optional outputs that
are null.  Through ctypes where the Python wrapper always passes arrays.  The store is
tiny: 4 points, 1 keyframe of 3 key points, 2 observations.  (dsh_local_map_update with N = 0 against the restatement is
tests/test_local_map_gpu.py::test_no_votes_keeps_the_previous_list_on_the_device.)  Also the refusal messages that need a stored point
or keyframe, as literal strings (the others: tests/test_refusal_messages_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import track_close_ref as T
from test_local_map_gpu import check_search, check_update
from test_track_close_gpu import check_state

pytestmark = pytest.mark.gpu

OK, ARG = 0, 1


def tiny(ctx):
    """The store and its host mirror: points 0 and 1 are observed by (and in the table of) keyframe 0, points 2 and 3 by nothing."""
    from defslam_amd import localmap
    rm = T.TrackRefMap()
    nrm = np.array([0.1, 0.2, 1.0]) / np.linalg.norm([0.1, 0.2, 1.0])
    rng = np.random.default_rng(5)
    for xyz in ([0.0, 0.0, 2.0], [0.1, 0.0, 2.0], [-0.1, 0.1, 2.0], [0.0, -0.1, 3.0]):
        rm.add_point(np.float32(xyz), np.float32(nrm), 4.0, rng.integers(0, 256, 32).astype(np.uint8))
    rm.add_keyframe([0, 1, -1])
    assert rm.add_observation(0, 0)
    assert rm.add_observation(1, 0)
    st = localmap.MapPointStore(ctx, points=4, keyframes=1, observations=2)
    rm.fill(st)
    assert st.n_points == 4 and st.n_keyframes == 1
    return st, rm


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def test_get_without_outputs_and_with_one(gpu_ctx):
    st, rm = tiny(gpu_ctx)
    L = gpu_ctx._L
    ids = np.arange(4, dtype=np.int32)
    assert L.dsh_trackstate_get(st._h, 4, p32(ids), None, None, None, None) == OK           # nothing to write
    n_obs = np.full(6, -7, np.int32)                                                          # two guard entries behind the four
    assert L.dsh_trackstate_get(st._h, 4, p32(ids), None, None, p32(n_obs), None) == OK
    assert n_obs.tolist() == [1, 1, 0, 0, -7, -7]
    assert ids.tolist() == [0, 1, 2, 3]
    check_state(st, rm)
    st.close()


def test_search_without_local_points_still_sees_the_frames_own_points(gpu_ctx):
    st, rm = tiny(gpu_ctx)
    g, _ = check_update(st, rm, [2, 3, 2])                                                    # points without observations: no vote, no list
    assert g.n_local_points == 0
    before = st.get_state().visible.copy()
    s = st.search_local_points(T.hand_frame(), 0)
    rm.search_local_points(T.hand_frame())
    assert s.nmatches == 0 and s.match.shape == (0,)
    assert (st.get_state().visible - before).tolist() == [0, 0, 2, 1]                         # one per key point that holds the point
    check_state(st, rm)
    st.close()


def test_repose_on_an_empty_store_moves_nothing(gpu_ctx):
    from defslam_amd import localmap
    st = localmap.MapPointStore(gpu_ctx, points=4, keyframes=1, observations=2)
    assert st.n_points == 0 and st.repose(T.HAND_NODES_AFTER) == 0
    st.close()


def test_a_descriptor_update_alone_leaves_positions_normals_and_depth_ranges(gpu_ctx):
    """xyz read back as bytes; normal and max distance through the search, whose view_cos and in_view come from them bit for bit."""
    st, rm = tiny(gpu_ctx)
    xyz = st.get_state().xyz.tobytes()
    desc = np.random.default_rng(6).integers(0, 256, (2, 32)).astype(np.uint8)
    st.update_points([3, 1], desc=desc)
    rm.points[3].desc, rm.points[1].desc = desc[0], desc[1]
    assert st.get_state().xyz.tobytes() == xyz
    g, _ = check_update(st, rm, [0])
    assert g.n_local_points == 2
    s = check_search(gpu_ctx, st, rm, T.hand_frame(), g.n_local_points)
    assert s.local_ids.tolist() == [0, 1] and s.in_view.tolist() == [False, True] and s.view_cos[1] > 0.5
    check_state(st, rm)
    st.close()


def test_refusal_messages_that_need_a_filled_store(gpu_ctx):
    from defslam_amd import _lib
    st, rm = tiny(gpu_ctx)
    L = gpu_ctx._L
    msg = lambda: L.dsh_last_error(gpu_ctx._h).decode()
    i32 = lambda *v: np.array(v, np.int32)
    pts, slot_out, pt_out, rep = i32(2, 3), i32(0, 1), i32(2, 4), i32(2, 1, 2)
    for name in ("dsh_mpdb_add_observations", "dsh_mpdb_erase_observations"):
        assert getattr(L, name)(st._h, 2, p32(pts), p32(slot_out)) == ARG and msg() == name + ": pair 1: keyframe slot outside the store"
        assert getattr(L, name)(st._h, 2, p32(pt_out), p32(i32(0, 0))) == ARG and msg() == name + ": pair 1: point id outside the store"
    assert L.dsh_mpdb_set_points_bad(st._h, 3, p32(rep), None) == ARG and msg() == "dsh_mpdb_set_points_bad: point id 2 repeated in the batch"
    check_state(st, rm)                                                                       # nothing was stored
    st.close()
    kf = C.c_void_p()
    assert L.dsh_kfdb_create(gpu_ctx._h, 2, C.byref(kf)) == OK
    assert L.dsh_kfdb_add(kf, None, None) == ARG and msg() == "dsh_kfdb_add: keyframe is NULL"
    assert L.dsh_kfdb_set_bad(kf, -1, 1) == ARG and msg() == "dsh_kfdb_set_bad: slot outside the store"
    assert L.dsh_kfdb_count(kf) == 0 and L.dsh_kfdb_destroy(kf) == OK


def pu8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def pf32(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def pf64(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def guarded(n, dtype, guard):
    """An output array of n entries and two guard entries behind them."""
    return np.full(n + 2, guard, dtype)


def test_one_output_among_absent_ones(gpu_ctx):
    """dsh_point_store_get_points and dsh_point_store_get_embedding with one output at a time: its values are those of the full call, the
    two entries behind the n asked for keep their guard value, and a call without any output is OK."""
    st, rm = tiny(gpu_ctx)
    st.set_embedding([1, 3], [[0, 1, 2], [1, 2, 3]], [[0.5, 0.25, 0.25], [0.25, 0.25, 0.5]])
    L = gpu_ctx._L
    ids = np.array([3, 0, 1], np.int32)
    full = st.get_points(ids)
    nodes, bary = st.get_embedding(ids)
    assert nodes.tolist() == [[1, 2, 3], [-1, -1, -1], [0, 1, 2]] and bary[2].tolist() == [0.5, 0.25, 0.25]
    assert L.dsh_point_store_get_points(st._h, 3, p32(ids), None, None, None, None, None) == OK
    assert L.dsh_point_store_get_embedding(st._h, 3, p32(ids), None, None) == OK
    outs = [(0, 3, np.float32, pf32, full.xyz), (1, 3, np.float32, pf32, full.normal), (2, 1, np.float32, pf32, full.max_distance),
            (3, 32, np.uint8, pu8, full.desc), (4, 1, np.uint8, pu8, full.bad)]
    for at, width, dtype, ptr, want in outs:
        a = guarded(3, dtype, 77).repeat(width)
        args = [None] * 5
        args[at] = ptr(a)
        assert L.dsh_point_store_get_points(st._h, 3, p32(ids), *args) == OK
        assert a[:3 * width].tobytes() == np.ascontiguousarray(want).astype(dtype).tobytes(), at
        assert (a[3 * width:] == 77).all(), at
    nd = guarded(3, np.int32, -7).repeat(3)
    assert L.dsh_point_store_get_embedding(st._h, 3, p32(ids), p32(nd), None) == OK
    assert nd[:9].tolist() == nodes.reshape(-1).tolist() and (nd[9:] == -7).all()
    b = guarded(3, np.float64, -7.0).repeat(3)
    assert L.dsh_point_store_get_embedding(st._h, 3, p32(ids), None, pf64(b)) == OK
    assert b[:9].tobytes() == bary.tobytes() and (b[9:] == -7.0).all()
    assert ids.tolist() == [3, 0, 1]
    st.close()


def test_local_map_lists_shorter_than_their_capacity(gpu_ctx):
    """dsh_local_map_update with kf_capacity above the keyframe count: the entries of local_kf / local_votes behind n_local_kf / n_voted
    keep their guard value."""
    st, rm = tiny(gpu_ctx)
    L = gpu_ctx._L
    want = rm.update_local_map([0, 1, 2])
    fp = np.array([0, 1, 2], np.int32)
    fb = guarded(3, np.uint8, 9)
    kf, votes = np.full(5, -7, np.int32), np.full(5, -7, np.int32)
    nv, nk, ref, npts = C.c_int32(-1), C.c_int32(-1), C.c_int32(-5), C.c_int32(-1)
    assert L.dsh_local_map_update(st._h, 3, p32(fp), pu8(fb), 5, p32(kf), p32(votes), C.byref(nv), C.byref(nk), C.byref(ref), C.byref(npts)) == OK
    assert nk.value == len(want["local_kf"]) == 1 and nv.value == len(want["votes"]) == 1
    assert kf.tolist() == list(want["local_kf"]) + [-7] * 4 and votes.tolist() == list(want["votes"]) + [-7] * 4
    assert fb.tolist() == [int(b) for b in want["frame_bad"]] + [9, 9]
    assert ref.value == want["ref_kf"] and npts.value == len(want["local_points"])
    check_state(st, rm)
    st.close()


def test_observation_lists_with_room_to_spare_and_without_enough(gpu_ctx):
    """dsh_point_store_get_observations: with capacity above the total, slots / idx behind n_total and obs_ptr behind its n + 1 entries
    keep their guard value; with capacity one below the total the call is refused, n_total is set and no array is touched."""
    st, rm = tiny(gpu_ctx)
    L = gpu_ctx._L
    msg = lambda: L.dsh_last_error(gpu_ctx._h).decode()
    ids = np.array([1, 2, 0], np.int32)
    full = st.observations(ids)
    assert full.ptr.tolist() == [0, 1, 1, 2] and full.slots.tolist() == [0, 0]
    ptr, sl, ix = np.full(6, -7, np.int32), np.full(5, -7, np.int32), np.full(5, -7, np.int32)
    total = C.c_int32(-1)
    assert L.dsh_point_store_get_observations(st._h, 3, p32(ids), p32(ptr), 5, p32(sl), p32(ix), C.byref(total)) == OK
    assert total.value == 2
    assert ptr.tolist() == [0, 1, 1, 2, -7, -7]
    assert sl.tolist() == full.slots.tolist() + [-7] * 3 and ix.tolist() == full.idx.tolist() + [-7] * 3
    ptr[:], sl[:], ix[:] = -7, -7, -7
    total = C.c_int32(-1)
    assert L.dsh_point_store_get_observations(st._h, 3, p32(ids), p32(ptr), 1, p32(sl), p32(ix), C.byref(total)) == ARG
    assert msg() == "dsh_point_store_get_observations: capacity 1 is too small for the 2 observations of the points"
    assert total.value == 2
    assert (ptr == -7).all() and (sl == -7).all() and (ix == -7).all()
    check_state(st, rm)
    st.close()


def test_anchor_lists_that_do_not_fit_leave_the_arrays(gpu_ctx):
    """dsh_keyframe_anchors with a pair capacity one below the need: refused, the needed sizes are set and no array is touched.  The tiny
    store's observations carry no key point index, so the store here is the smallest with an anchor: two keyframes that hold the same
    two points."""
    from defslam_amd import _lib, localmap
    from store_model import MapModel
    m = MapModel()
    for _ in range(2):
        m.add_point(ref=0)
    for s in range(2):
        m.add_keyframe([0, 1])
        for i in range(2):
            assert m.add_observation(i, s, i)
    st = localmap.MapPointStore(gpu_ctx, points=2, keyframes=2, observations=4)
    m.fill(st)
    L = gpu_ctx._L
    full = st.keyframe_anchors(1, 0)
    A, npair, nq = len(full.anchor_slot), len(full.pair_idx1), len(full.query_idx1)
    assert A == 1 and npair == 2 and full.pair_ptr.tolist() == [0, 2]
    i32 = {n: np.full(4, -7, np.int32) for n in ("anchor_slot", "anchor_count", "anchor_pairs", "pair_ptr", "pair_idx1", "pair_idx2", "pair_point",
                                                    "query_ptr", "query_idx1", "query_point")}
    own, has = np.full(4, 9, np.uint8), np.full(4, 9, np.uint8)
    r = _lib.AnchorListsC(anchor_capacity=3, pair_capacity=npair - 1, query_capacity=4, max_matrix_bytes=0, pair_own=pu8(own), has=pu8(has),
                          **{n: p32(v) for n, v in i32.items()})
    assert L.dsh_keyframe_anchors(st._h, 1, 0, C.byref(r)) == ARG
    assert L.dsh_last_error(gpu_ctx._h).decode() == ("dsh_keyframe_anchors: the lists do not fit: %d anchors, %d pairs and %d queries are needed "
                                                     "(n_anchors, n_pairs, n_queries of out)" % (A, npair, nq))
    assert (r.n_anchors, r.n_pairs, r.n_queries) == (A, npair, nq)
    assert all((v == -7).all() for v in i32.values()) and (own == 9).all() and (has == 9).all()
    st.close()


def test_repose_and_end_frame_without_their_optional_outputs(gpu_ctx):
    """dsh_trackstate_repose with n_moved null and dsh_track_end_frame with points_out, outlier_out and out null."""
    st, rm = tiny(gpu_ctx)
    L = gpu_ctx._L
    for p, nodes, bary in ((0, (0, 1, 2), (0.5, 0.25, 0.25)), (3, (1, 2, 3), (0.25, 0.25, 0.5))):
        st.set_embedding([p], [nodes], [bary])
        rm.set_embedding(p, nodes, bary)
    x = np.ascontiguousarray(T.HAND_NODES_AFTER, np.float64)
    assert L.dsh_trackstate_repose(st._h, 4, pf64(x), None) == OK
    assert rm.repose(T.HAND_NODES_AFTER) == 2
    g = check_state(st, rm)
    assert g.xyz[0].tolist() == [-0.0625, -0.0625, 1.0078125]
    fp, out, octave = np.array([0, 1, 2, -1], np.int32), np.array([0, 1, 0, 0], np.uint8), np.array([0, 1, 2, 3], np.int32)
    assert L.dsh_track_end_frame(st._h, 4, p32(fp), pu8(out), p32(octave), None, None, None) == OK
    last = st.last_frame(4)                                                                   # point 1 was an outlier, point 2 has no observation
    assert last.ids.tolist() == [0, -1, -1, -1] and last.octave.tolist() == [0, -1, -1, -1]
    assert fp.tolist() == [0, 1, 2, -1] and out.tolist() == [0, 1, 0, 0]
    check_state(st, rm)
    st.close()
