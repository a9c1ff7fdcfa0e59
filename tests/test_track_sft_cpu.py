"""CPU tests of the observation selection of dsh_track_sft: the NumPy restatement tests/track_sft_ref.py on constructed cases, one per
branch of DefOptimizer.cc:293-361, and on generated scenes, where it must return the synth frame's own rows; the ABI of the two new
entries and every refusal that needs no device, on host-only contexts."""
import ctypes as C
import os

import numpy as np
import pytest

import track_sft_ref as R

OK, ARG, STATE, NODEV = 0, 1, 3, 4
NEW_ENTRIES = ("dsh_track_sft_observations", "dsh_track_sft")


# ---- constructed cases: one per branch -------------------------------------------------------------------------------------------------

def hand_model():
    """p0, p1 with a facet; p2 bad with a facet; p3 without a facet."""
    m = R.SftModel()
    m.add_point(nodes=(0, 1, 2), bary=(0.5, 0.25, 0.25))
    m.add_point(nodes=(1, 2, 3), bary=(0.25, 0.5, 0.25))
    m.add_point(nodes=(0, 1, 2), bary=(0.25, 0.25, 0.5), bad=True)
    m.add_point()
    return m


HAND_KP = np.array([[10, 20], [30, 40], [50, 60], [70, 80], [90, 100]], np.float32) + np.float32(0.3)
HAND_OCT = [0, 1, 2, 3, 4]


def hand_select(frame_points, outlier):
    return R.select(hand_model(), HAND_KP, HAND_OCT, R.INV_LEVEL_SIGMA2, frame_points, outlier)


def test_a_hole_gives_no_row_and_does_not_count():
    t = hand_select([0, -1, 1, -1, -1], [0, 0, 0, 0, 0])
    assert t.kp_index.tolist() == [0, 2] and t.point_id.tolist() == [0, 1] and t.points_obs == 2


def test_an_outlier_on_entry_gives_no_row_and_does_not_count():
    t = hand_select([0, 1, -1, -1, -1], [1, 0, 0, 0, 0])
    assert t.kp_index.tolist() == [1] and t.points_obs == 1


def test_a_bad_point_gives_no_row_but_counts():
    t = hand_select([0, 2, -1, -1, -1], [0, 0, 0, 0, 0])
    assert t.kp_index.tolist() == [0] and t.points_obs == 2


def test_a_point_without_a_facet_gives_no_row_but_counts():
    t = hand_select([3, 1, -1, -1, -1], [0, 0, 0, 0, 0])
    assert t.kp_index.tolist() == [1] and t.points_obs == 2


def test_an_id_held_twice_gives_a_row_each_in_key_point_order():
    t = hand_select([1, 0, -1, 1, 0], [0, 0, 0, 0, 1])
    assert t.kp_index.tolist() == [0, 1, 3] and t.point_id.tolist() == [1, 0, 1] and t.points_obs == 3
    assert t.nodes.tolist() == [[1, 2, 3], [0, 1, 2], [1, 2, 3]]
    assert t.bary.tolist() == [[0.25, 0.5, 0.25], [0.5, 0.25, 0.25], [0.25, 0.5, 0.25]]
    # the float32 key point and the float32 level weight, widened
    assert t.uv.dtype == np.float64 and t.uv.tobytes() == HAND_KP[[0, 1, 3]].astype(np.float64).tobytes()
    assert t.invsig2.tobytes() == R.INV_LEVEL_SIGMA2[[0, 1, 3]].astype(np.float64).tobytes()


def test_points_obs_against_m_and_the_empty_frame():
    t = hand_select([0, 1, 2, 3, 2], [0, 1, 0, 0, 1])
    assert (len(t.kp_index), t.points_obs) == (1, 3)
    t = R.select(hand_model(), np.zeros((0, 2), np.float32), [], R.INV_LEVEL_SIGMA2, [], [])
    assert (len(t.kp_index), t.points_obs) == (0, 0) and t.nodes.shape == (0, 3) and t.uv.shape == (0, 2)
    t = R.select(R.SftModel(), HAND_KP, HAND_OCT, R.INV_LEVEL_SIGMA2, [-1] * 5, None)
    assert (len(t.kp_index), t.points_obs) == (0, 0)


def test_the_scatter_writes_the_rows_and_keeps_the_rest():
    t = hand_select([1, 0, -1, 1, 0], [0, 0, 1, 0, 1])
    assert R.scatter([0, 0, 1, 0, 1], t, [1, 0, 1]).tolist() == [True, False, True, True, True]


# ---- generated scenes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(), dict(twice=False), dict(partial=True, seed=3), dict(N=1200, n_rows=450, seed=5, free_points=40)],
                         ids=["default", "no_twice", "partial", "default_size"])
def test_generated_scene_returns_the_synth_frames_own_rows(kw):
    sc = R.make_scene(**kw)
    fr = sc.synth
    for a in (fr.obs_uv, fr.obs_invsig2, fr.obs_bary):                       # what lets the float32 frame carry them exactly
        assert a.dtype == np.float64 and np.array_equal(a, a.astype(np.float32).astype(np.float64))
    assert set(np.unique(fr.obs_invsig2)) <= set(R.INV_LEVEL_SIGMA2.astype(np.float64))
    held = np.nonzero(sc.frame_points >= 0)[0]
    assert not np.array_equal(sc.frame_points[held], np.sort(sc.frame_points[held]))          # shuffled
    assert (sc.frame_points < 0).any() and sc.outlier.sum() == 5
    t = R.select(sc.model, sc.kp, sc.octave, R.INV_LEVEL_SIGMA2, sc.frame_points, sc.outlier)
    R.assert_table(t, R.expected_table(sc), str(kw))
    M = len(sc.rows) + (sc.twice >= 0)
    assert len(t.kp_index) == M and t.points_obs == M + 3 + 4 and (np.diff(t.kp_index) > 0).all()
    if kw.get("partial"):
        assert (t.nodes % 10).max() < 5


# ---- the ABI without a GPU -------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_bound_declared_and_wrapped():
    from defslam_amd import _lib, localmap
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "defslam_hip.h")).read()
    for n in NEW_ENTRIES:
        assert n in _lib.EXPORTED_SYMBOLS and getattr(L, n).argtypes is not None, n
        assert f"int {n}(dsh_mpdb* db" in header, n
    # the C layout on an LP64 target
    assert "} dsh_track_sft_frame;" in header and C.sizeof(_lib.TrackSftFrameC) == 136 and _lib.TrackSftFrameC.xyz.offset == 96
    assert "} dsh_track_sft_table;" in header and C.sizeof(_lib.TrackSftTableC) == 64 and _lib.TrackSftTableC.kp_index.offset == 16
    for m in ("sft_observations", "sft"):
        assert callable(getattr(localmap.MapPointStore, m))
    assert list(localmap.SftObservations.__dataclass_fields__) == ["kp_index", "point_id", "nodes", "bary", "uv", "invsig2", "points_obs"]


def _frame(keep, **kw):
    from defslam_amd import _lib
    a = dict(T=np.eye(4, dtype=np.float32), kp=np.zeros((4, 2), np.float32), oct=np.zeros(4, np.int32), sig=np.ones(8, np.float32),
             fp=np.full(4, -1, np.int32), out=np.ones(4, np.uint8), xyz=np.zeros((100, 3)))
    keep.append(a)
    f = _lib.TrackSftFrameC()
    ptr = lambda x, t: x.ctypes.data_as(C.POINTER(t))
    f.Tcw, f.kp, f.octave, f.inv_level_sigma2 = ptr(a["T"], C.c_float), ptr(a["kp"], C.c_float), ptr(a["oct"], C.c_int32), ptr(a["sig"], C.c_float)
    f.frame_points, f.outlier, f.xyz = ptr(a["fp"], C.c_int32), ptr(a["out"], C.c_uint8), ptr(a["xyz"], C.c_double)
    f.K = (C.c_double * 4)(500, 500, 320, 240)
    f.N, f.levels, f.neighbour_layers, f.max_iters = 4, 8, 1, 50
    f.reg_lap, f.reg_inex, f.reg_temp = 700.0, 12000.0, 0.05
    for k, v in kw.items():
        if k in ("fp", "oct"):
            a[k][:] = v
        else:
            setattr(f, k, v)
    keep.append(f)
    return f


def _rows(keep):
    """(name, arguments after the store handle, expected status, a word of the message, the frame, the table, the result) for an EMPTY
    store on a host-only context that has a template."""
    from defslam_amd import _lib
    obs, sft = NEW_ENTRIES
    rows = []

    def out_structs():
        t, r = _lib.TrackSftTableC(), _lib.SftResultC()
        t.capacity, t.M, t.points_obs, r.inliers = 4, -7, -7, -7            # a refusal writes nothing
        keep.extend([t, r])
        return t, r

    def both(want, word, solve_only=False, **kw):
        for name in NEW_ENTRIES:
            f = _frame(keep, **kw)
            t, r = out_structs()
            if name == obs:
                rows.append((obs, (C.byref(f), C.byref(t)), NODEV if solve_only else want, "host-only" if solve_only else word, f, t, r))
            else:
                rows.append((sft, (C.byref(f), 1, C.byref(t), C.byref(r)), want, word, f, t, r))

    both(NODEV, "host-only")
    both(NODEV, "host-only", N=0, kp=None, octave=None, frame_points=None, outlier=None)
    both(NODEV, "host-only", oct=99)                                  # an octave is read only where a point is held
    both(ARG, "N outside", N=-1)
    both(ARG, "N outside", N=8193)
    both(ARG, "levels outside", levels=0)
    both(ARG, "levels outside", levels=33)
    both(ARG, "inv_level_sigma2 is NULL", inv_level_sigma2=None)
    both(ARG, "NULL", kp=None)
    both(ARG, "NULL", octave=None)
    both(ARG, "NULL", frame_points=None)
    both(ARG, "NULL", outlier=None)
    both(ARG, "frame_points[0]", fp=0)                                # id 0 outside the empty store
    both(ARG, "frame_points[0]", fp=-2)
    both(ARG, "Tcw or xyz is NULL", solve_only=True, Tcw=None)
    both(ARG, "Tcw or xyz is NULL", solve_only=True, xyz=None)
    both(ARG, "max_iters outside", solve_only=True, max_iters=65)
    f = _frame(keep)
    t, r = out_structs()
    rows.append((obs, (None, C.byref(t)), ARG, "f is NULL", None, t, r))
    rows.append((obs, (C.byref(f), None), ARG, "t is NULL", f, t, r))
    rows.append((sft, (None, 1, C.byref(t), C.byref(r)), ARG, "f is NULL", None, t, r))
    rows.append((sft, (C.byref(f), 1, C.byref(t), None), ARG, "r is NULL", f, t, r))
    rows.append((sft, (C.byref(f), 1, None, C.byref(r)), NODEV, "host-only", f, t, r))    # the table is optional
    return rows


def _template_ctx():
    from defslam_amd import sft, synth
    ctx = sft.Context(-1)
    tmpl = synth.make_grid_template(10, 10)
    ctx.template_build(tmpl.xyz0, tmpl.facets)
    return ctx


def test_host_only_status_of_every_refusal():
    """On a host-only context a malformed call is DSH_ERR_ARG with a message naming the entry point and the argument and writes
    nothing, a well-formed one DSH_ERR_NO_DEVICE saying "host-only" -- arguments first, then the device; a NULL store is DSH_ERR_ARG."""
    from test_local_map_cpu import _raw_store
    ctx = _template_ctx()
    L = ctx._L
    msg = lambda: L.dsh_last_error(ctx._h).decode()
    rc, h = _raw_store(L, ctx._h)
    assert rc == OK and h
    keep = []
    rows = _rows(keep)
    assert {r[0] for r in rows} == set(NEW_ENTRIES)
    for name, args, want, word, f, t, r in rows:
        fn = getattr(L, name)
        assert fn(h, *args) == want, (name, word, msg())
        assert msg().startswith(name + ": ") and word in msg(), (name, word, msg())
        assert fn(None, *args) == ARG, (name, "NULL store")
        assert (t.M, t.points_obs, r.inliers) == (-7, -7, -7), (name, word)
        if f is not None and f.outlier:
            assert bytes(f.outlier[0:4]) == b"\x01" * 4, (name, word)
    assert L.dsh_mpdb_point_count(h) == 0
    assert L.dsh_mpdb_destroy(h) == OK
    ctx.close()


def test_no_template_is_a_state_error_behind_the_argument_checks():
    from defslam_amd import sft
    from test_local_map_cpu import _raw_store
    ctx = sft.Context(-1)
    L = ctx._L
    rc, h = _raw_store(L, ctx._h)
    assert rc == OK
    keep = []
    for name, args, want, word, *_ in _rows(keep):
        rc = getattr(L, name)(h, *args)
        assert rc == (ARG if want == ARG else STATE), (name, word)
        if rc == STATE:
            assert L.dsh_last_error(ctx._h).decode() == name + ": no template"
    assert L.dsh_mpdb_destroy(h) == OK
    ctx.close()


def test_a_detached_store_refuses_every_new_entry():
    from test_local_map_cpu import _raw_store
    ctx = _template_ctx()
    L = ctx._L
    rc, h = _raw_store(L, ctx._h)
    assert rc == OK
    ctx.close()                                    # dsh_destroy detaches the store
    keep = []
    for name, args, *_ in _rows(keep):
        assert getattr(L, name)(h, *args) == ARG, name
    assert L.dsh_mpdb_destroy(h) == OK
