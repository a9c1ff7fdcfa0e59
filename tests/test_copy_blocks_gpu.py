"""GPU tests of the empty paths of the one-copy blocks (UpBlock / DownBlock of defslam_amd/csrc/dsh_ctx.h) that no other test reaches: a
download block without a slice, one with a single slice among absent ones, a search without queries, an early return in front of the
blocks, an upload block whose unselected slices are empty.  Through ctypes where the Python wrapper always passes arrays.  The store is
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
