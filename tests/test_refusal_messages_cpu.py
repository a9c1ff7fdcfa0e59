"""The refusal messages of the validators that the map point store's entry points share (defslam_amd/csrc/mpdb_store.h, dsh_ctx.h), as
literal strings: the entry points keep their own wording ("table entry 1" against "frame_points[1]") through the shared checks.  A store
created on a host-only context checks arguments before it refuses, but it stays empty and a keyframe store cannot be created there at
all, so the messages that need a stored point or keyframe (a keyframe slot outside the store, an id repeated in a batch, dsh_kfdb_*) are
asserted the same way on a device: tests/test_copy_blocks_gpu.py::test_refusal_messages_that_need_a_filled_store."""
import ctypes as C

import numpy as np
import pytest

ARG = 1
BIG = (1 << 20) + 1


def _rows(keep):
    """(entry point, arguments after the store handle, dsh_last_error) for an EMPTY store."""
    from test_track_search_cpu import hand_frame
    from defslam_amd import _lib
    f = C.byref(hand_frame([[10, 10]], [0]).c(keep))
    a = dict(t=np.array([-1, 0], np.int32), z=np.zeros(1, np.int32), u=np.zeros(2, np.uint8))
    cc = _lib.TrackCloseCountsC()
    keep += [a, cc]
    t, z, u = a["t"].ctypes.data_as(_lib.c_i32_p), a["z"].ctypes.data_as(_lib.c_i32_p), a["u"].ctypes.data_as(_lib.c_u8_p)
    update = lambda N, fp: (N, fp, None, 0, None, None, None, None, None, None)
    close = lambda N, fp, out: (f, N, fp, out, 0, None, 0, C.byref(cc))
    return [
        ("dsh_local_map_update", update(2, t), "dsh_local_map_update: frame_points[1] is neither -1 nor a point of the store"),
        ("dsh_local_map_update", update(-1, None), "dsh_local_map_update: N outside 0 .. 2^20"),
        ("dsh_local_map_update", update(BIG, None), "dsh_local_map_update: N outside 0 .. 2^20"),
        ("dsh_track_close_frame", close(2, t, u), "dsh_track_close_frame: frame_points[1] is neither -1 nor a point of the store"),
        ("dsh_track_close_frame", close(-1, None, None), "dsh_track_close_frame: N outside 0 .. 2^20"),
        ("dsh_track_close_frame", close(BIG, None, None), "dsh_track_close_frame: N outside 0 .. 2^20"),
        ("dsh_mpdb_add_keyframe", (2, t, -1, 0, None), "dsh_mpdb_add_keyframe: table entry 1 is neither -1 nor a point of the store"),
        ("dsh_mpdb_add_keyframe", (-1, None, -1, 0, None), "dsh_mpdb_add_keyframe: N outside 0 .. 2^20"),
        ("dsh_mpdb_add_keyframe", (BIG, None, -1, 0, None), "dsh_mpdb_add_keyframe: N outside 0 .. 2^20"),
        ("dsh_mpdb_add_observations", (1, z, z), "dsh_mpdb_add_observations: pair 0: point id outside the store"),
        ("dsh_mpdb_erase_observations", (1, z, z), "dsh_mpdb_erase_observations: pair 0: point id outside the store"),
        ("dsh_mpdb_set_points_bad", (1, None, None), "dsh_mpdb_set_points_bad: point id array is NULL"),
    ]


@pytest.mark.parametrize("n", [8001, 8000])
def test_surface_registration_refuses_more_than_8000_pairs(host_ctx, n):
    """kMaxPairs of dsh_register.cpp (smm_finish_kernel keeps two floats per pair in LDS): the argument check comes before the device
    entry, so 8001 pairs are DSH_ERR_ARG on a host-only context too, and 8000 pass it and reach "no GPU"."""
    from defslam_amd import _lib
    L = host_ctx._L
    a = np.ones((n, 3), np.float32)
    u = np.ones(n)      # no candidate: nothing but the stream's first n numbers would be read
    fp, dp = a.ctypes.data_as(_lib.c_float_p), u.ctypes.data_as(_lib.c_double_p)
    scale, consumed, status, reg, s22 = C.c_float(-1), C.c_int64(-1), C.c_int32(-1), C.c_int32(-1), C.c_double(-1)
    Twc, Tcw, sim3 = np.eye(4, dtype=np.float32), np.zeros(16, np.float32), np.zeros(8)
    calls = [
        ("dsh_scale_min_median", lambda: L.dsh_scale_min_median(host_ctx._h, n, fp, fp, dp, n, C.byref(scale), C.byref(consumed), C.byref(status)),
         "dsh_scale_min_median: bad argument (1 <= n <= 8000)"),
        ("dsh_surface_register", lambda: L.dsh_surface_register(host_ctx._h, n, fp, fp, dp, n, Twc.ctypes.data_as(_lib.c_float_p), 0.05, 1, C.byref(reg),
                                                                sim3.ctypes.data_as(_lib.c_double_p), C.byref(s22), Tcw.ctypes.data_as(_lib.c_float_p), None),
         "dsh_surface_register: bad argument (n <= 8000)"),
    ]
    for name, call, refusal in calls:
        rc = call()
        msg = L.dsh_last_error(host_ctx._h).decode()
        if n > 8000:
            assert rc == ARG and msg == refusal
        else:
            assert rc == 4 and msg == name + ": host-only context, no GPU (there is no CPU fallback)"      # DSH_ERR_NO_DEVICE
    assert (scale.value, consumed.value, status.value, s22.value) == (-1, -1, -1, -1) and not sim3.any() and not Tcw.any()
    assert reg.value == (-1 if n > 8000 else 0)


@pytest.mark.parametrize("row", range(12))
def test_refusal_message_on_a_host_only_store(host_ctx, row):
    from test_local_map_cpu import _raw_store
    L = host_ctx._L
    rc, h = _raw_store(L, host_ctx._h)
    assert rc == 0 and h
    keep = []
    name, args, want = _rows(keep)[row]
    assert getattr(L, name)(h, *args) == ARG
    assert L.dsh_last_error(host_ctx._h).decode() == want
    assert L.dsh_mpdb_point_count(h) == 0 and L.dsh_mpdb_keyframe_count(h) == 0
    assert L.dsh_mpdb_destroy(h) == 0
