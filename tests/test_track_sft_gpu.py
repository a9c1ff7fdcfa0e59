"""GPU tests of dsh_track_sft_observations and dsh_track_sft.
The selection alone: every array of the table byte for byte against the NumPy restatement tests/track_sft_ref.py, at frame sizes around
the wavefront, the tile and the workgroup's share, and at the largest frame.
The solve: every field of the result byte for byte dsh_sft_solve on the restatement's table on the same context, mvbOutlier the scatter
of its flags, the store's positions those of a twin store after repose(result.xyz) and nothing else of the store changed.  Integers
and bytes: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import store_model
import track_sft_ref as R

pytestmark = pytest.mark.gpu

REGS = dict(full=(700.0, 12000.0, 0.05), partial=(700.0, 12000.0, 0.05), reg_temp0=(700.0, 12000.0, 0.0))
SCENES = dict(full=dict(seed=0), partial=dict(seed=3, partial=True), reg_temp0=dict(seed=1))
_CASE = {}


def case(name):
    """scene and the restatement's table of a solve case: computed once, shared, not modified."""
    if name not in _CASE:
        sc = R.make_scene(N=300, n_rows=150, **SCENES[name])
        _CASE[name] = (sc, R.select(sc.model, sc.kp, sc.octave, R.INV_LEVEL_SIGMA2, sc.frame_points, sc.outlier))
    return _CASE[name]


def store_of(ctx, model):
    from defslam_amd import localmap
    st = localmap.MapPointStore(ctx, points=64)
    model.fill(st)
    return st


def use_template(ctx, tmpl):
    ctx.template_build(tmpl.xyz0, tmpl.facets)


def snapshot(st):
    """Everything the store holds per point, as bytes."""
    p, s, (nd, b) = st.get_points(), st.get_state(), st.get_embedding()
    return dict(xyz=p.xyz.tobytes(), normal=p.normal.tobytes(), max_distance=p.max_distance.tobytes(), desc=p.desc.tobytes(), bad=p.bad.tobytes(),
                visible=s.visible.tobytes(), found=s.found.tobytes(), n_obs=s.n_obs.tobytes(), nodes=nd.tobytes(), bary=b.tobytes())


def call_sft(st, sc, regs, write_back, outlier=None, xyz=None):
    return st.sft(sc.Tcw, sc.K, sc.kp, sc.octave, R.INV_LEVEL_SIGMA2, sc.frame_points, sc.xyz if xyz is None else xyz,
                  outlier=sc.outlier if outlier is None else outlier, write_back=write_back, RegLap=regs[0], RegInex=regs[1], RegTemp=regs[2])


def solve_on_table(ctx, sc, t, regs):
    """dsh_sft_solve on a host table."""
    from defslam_amd import sft
    f = sft.Frame(Tcw=sc.Tcw.copy(), K=sc.K.copy(), N=len(sc.frame_points), obs_nodes=t.nodes, obs_bary=t.bary, obs_uv=t.uv, obs_invsig2=t.invsig2,
                  nodes_xyz=sc.xyz.copy())
    inl = ctx.prepare_solve(f, *regs)()
    return f, inl


RESULT_ARRAYS = (("Tcw", "Tcw"), ("pose7", "pose7"), ("xyz", "nodes_xyz"), ("chi2_obs", "chi2_obs"), ("row_outlier", "mvbOutlier"),
                 ("mappoint_xyz", "mappoints"))
RESULT_SCALARS = (("iters", "iters"), ("trials", "trials"), ("dim", "dim"), ("half_bandwidth", "half_bandwidth"), ("status", "status"))


def assert_result(g, f, inl, what):
    for a, b in RESULT_ARRAYS:
        x, y = np.ascontiguousarray(getattr(g, a)), np.ascontiguousarray(getattr(f, b))
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, a)
    for a, b in RESULT_SCALARS:
        assert getattr(g, a) == getattr(f, b), (what, a, getattr(g, a), getattr(f, b))
    assert g.inliers == inl, (what, g.inliers, inl)
    assert np.float64(g.rep_error).tobytes() == np.float64(f.rep_error_f64).tobytes(), (what, g.rep_error, f.rep_error_f64)


# ---- the selection alone ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def selection_store(gpu_ctx):
    """A few hundred points: rows, bad points, points without a facet, points nobody holds."""
    sc = R.make_scene(N=300, n_rows=200, seed=7, n_bad=20, n_no_facet=25, free_points=40)
    use_template(gpu_ctx, sc.tmpl)
    st = store_of(gpu_ctx, sc.model)
    yield st, sc.model
    st.close()


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 255, 256, 257, 513, 8192])
def test_selection_equals_the_restatement(selection_store, N):
    st, model = selection_store
    P = len(model.points)
    for rate in (0.0, 0.5, 1.0):
        rng = np.random.default_rng(100 * N + int(10 * rate))
        fp = np.where(rng.uniform(size=N) < rate, rng.integers(0, P, N), -1).astype(np.int32)
        out = rng.uniform(size=N) < 0.2
        octave = np.where(fp >= 0, rng.integers(0, R.LEVELS, N), 99).astype(np.int32)
        kp = np.stack([rng.uniform(0, 640, N), rng.uniform(0, 480, N)], 1).astype(np.float32)
        ref = R.select(model, kp, octave, R.INV_LEVEL_SIGMA2, fp, out)
        got = st.sft_observations(kp, octave, R.INV_LEVEL_SIGMA2, fp, out)
        print(f"N {N} rate {rate}: M {len(got.kp_index)} (ref {len(ref.kp_index)}) points_obs {got.points_obs} (ref {ref.points_obs})")
        R.assert_table(got, ref, (N, rate))
        if rate == 0.0:
            assert len(got.kp_index) == 0 and got.points_obs == 0
        elif N >= 63:
            assert 0 < len(got.kp_index) < got.points_obs <= N                 # bad points and points without a facet were held


# ---- the solve ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SCENES))
def test_solve_equals_sft_solve_on_the_table_and_moves_the_points(gpu_ctx, name):
    sc, t = case(name)
    regs = REGS[name]
    R.assert_table(t, R.expected_table(sc), name)
    assert 140 <= len(t.kp_index) <= 160 and sc.twice >= 0
    use_template(gpu_ctx, sc.tmpl)
    f, inl = solve_on_table(gpu_ctx, sc, t, regs)
    if name == "partial":
        assert f.dim < 6 + 3 * sc.tmpl.n                                       # the active set is a strict subset of the nodes
    else:
        assert f.dim == 6 + 3 * sc.tmpl.n
    st, twin = store_of(gpu_ctx, sc.model), store_of(gpu_ctx, sc.model)
    before = snapshot(st)
    # without write_back: the result, the flags, and a store that has not changed
    g = call_sft(st, sc, regs, write_back=False)
    print(f"{name}: M {len(t.kp_index)} iters {g.iters} trials {g.trials} inliers {g.inliers} dim {g.dim} rep_error {g.rep_error:.4f}")
    R.assert_table(g.table, t, name)
    assert_result(g, f, inl, name)
    want_flags = R.scatter(sc.outlier, t, f.mvbOutlier)
    assert np.array_equal(g.outlier, want_flags), name
    assert g.outlier[sc.outlier].all() and g.iters > 0 and 0 < g.inliers <= len(t.kp_index)
    assert snapshot(st) == before, name
    store_model.assert_state(st, sc.model, name)
    # with write_back: the same numbers again, the positions of the twin after repose(result.xyz), nothing else
    g2 = call_sft(st, sc, regs, write_back=True)
    assert_result(g2, f, inl, name + " second call")
    assert np.array_equal(g2.outlier, want_flags), name
    moved = twin.repose(g.xyz)
    assert moved == sum(1 for p, pt in enumerate(sc.model.points) if not pt.bad and sc.model.nodes[p] is not None)
    after, want = snapshot(st), snapshot(twin)
    assert after["xyz"] == want["xyz"] and after["xyz"] != before["xyz"], name
    assert {k: v for k, v in after.items() if k != "xyz"} == {k: v for k, v in before.items() if k != "xyz"}, name
    store_model.assert_state(st, sc.model, name)
    st.close()
    twin.close()


def test_close_frame_without_nodes_after_the_write_back(gpu_ctx):
    """close_frame(node_xyz=None) behind sft(write_back) counts what close_frame(node_xyz) counts on a twin that was not written back;
    n_moved is the exception, the points moved inside sft."""
    from defslam_amd import track
    sc, t = case("full")
    regs = REGS["full"]
    use_template(gpu_ctx, sc.tmpl)
    st, twin = store_of(gpu_ctx, sc.model), store_of(gpu_ctx, sc.model)
    P = len(sc.model.points)
    for s in (st, twin):
        s.seed_local_points(np.arange(P))
    g = call_sft(st, sc, regs, write_back=True)
    sf, logsf = track.orb_pyramid(R.LEVELS)
    N = len(sc.frame_points)
    fr = track.TrackFrame(Tcw=g.Tcw, K=np.asarray(sc.K, np.float32), bounds=np.array([0, 640, 0, 480], np.float32), kp=sc.kp,
                          octave=np.where(sc.frame_points >= 0, sc.octave, 0), desc=np.zeros((N, 32), np.uint8), scale_factors=sf,
                          log_scale_factor=float(logsf))
    a = st.close_frame(fr, sc.frame_points, g.outlier, None)
    b = twin.close_frame(fr, sc.frame_points, g.outlier, g.xyz)
    for n in a.__dataclass_fields__:
        if n != "n_moved":
            assert getattr(a, n) == getattr(b, n), (n, a, b)
    assert a.n_moved == 0 and b.n_moved > 0 and a.matches_inliers > 0 and a.local_map_points > 0
    assert snapshot(st) == snapshot(twin)
    st.close()
    twin.close()


def test_no_row_returns_the_input(gpu_ctx):
    """M == 0 (every key point that holds a point is an outlier on entry): DSH_OK, zeros, NaN, the input pose and nodes, the flags and the
    store untouched."""
    sc, _ = case("full")
    use_template(gpu_ctx, sc.tmpl)
    st = store_of(gpu_ctx, sc.model)
    before = snapshot(st)
    flags = sc.frame_points >= 0
    T = sc.Tcw.copy()
    T[0, 3] = np.float32(0.015625)
    xyz = sc.xyz + 0.25
    g = st.sft(T, sc.K, sc.kp, sc.octave, R.INV_LEVEL_SIGMA2, sc.frame_points, xyz, outlier=flags, write_back=True)
    assert (g.inliers, g.iters, g.trials, g.dim, g.half_bandwidth, g.status) == (0, 0, 0, 0, 0, 0) and np.isnan(g.rep_error)
    assert len(g.table.kp_index) == 0 and g.table.points_obs == 0
    assert g.Tcw.tobytes() == T.tobytes() and g.xyz.tobytes() == xyz.tobytes()
    assert np.array_equal(g.pose7, [0.015625, 0, 0, 0, 0, 0, 1])
    assert np.array_equal(g.outlier, flags) and snapshot(st) == before
    g = st.sft(T, sc.K, np.zeros((0, 2)), [], R.INV_LEVEL_SIGMA2, [], xyz)      # an empty frame
    assert g.iters == 0 and np.isnan(g.rep_error) and g.xyz.tobytes() == xyz.tobytes() and snapshot(st) == before
    st.close()


def test_refusals_that_need_points_in_the_store(gpu_ctx):
    """A stale embedding is refused by the packer and the message names the key point; a stored node index outside the template, an
    octave outside the levels where a point is held, an id outside the store and a table without room are refused by name; nothing of
    the store or the flags changes."""
    from defslam_amd import _lib
    sc, t = case("full")
    regs = REGS["full"]
    use_template(gpu_ctx, sc.tmpl)
    st = store_of(gpu_ctx, sc.model)
    orig = snapshot(st)
    m = int(np.nonzero(t.point_id != 0)[0][17])                             # not the id held twice
    i, p = int(t.kp_index[m]), int(t.point_id[m])
    nodes, bary = st.get_embedding([p])
    st.set_embedding([p], [[0, 55, 99]], bary)                             # three nodes of the 10 x 10 grid that share no edge
    before = snapshot(st)
    with pytest.raises(Exception, match=rf"dsh_track_sft: .*observation {m}: its nodes are not joined.*\(key point {i}\)"):
        call_sft(st, sc, regs, write_back=True)
    assert snapshot(st) == before
    got = st.sft_observations(sc.kp, sc.octave, R.INV_LEVEL_SIGMA2, sc.frame_points, sc.outlier)      # the selection does not judge it
    assert got.nodes[m].tolist() == [0, 55, 99]
    st.set_embedding([p], [[0, 1, 100]], bary)
    for fn in (lambda: call_sft(st, sc, regs, write_back=True),
               lambda: st.sft_observations(sc.kp, sc.octave, R.INV_LEVEL_SIGMA2, sc.frame_points, sc.outlier)):
        with pytest.raises(Exception, match=r"dsh_track_sft\w*: a stored node index \(100\) is >= the 100 nodes"):
            fn()
    st.set_embedding([p], nodes, bary)
    oc = sc.octave.copy()
    assert (oc[sc.frame_points < 0] == 99).all()                            # not read where no point is held
    oc[i] = R.LEVELS
    with pytest.raises(Exception, match=rf"dsh_track_sft_observations: octave\[{i}\] outside"):
        st.sft_observations(sc.kp, oc, R.INV_LEVEL_SIGMA2, sc.frame_points, sc.outlier)
    fp = sc.frame_points.copy()
    fp[i] = st.n_points
    with pytest.raises(Exception, match=rf"dsh_track_sft: frame_points\[{i}\]"):
        st.sft(sc.Tcw, sc.K, sc.kp, sc.octave, R.INV_LEVEL_SIGMA2, fp, sc.xyz, outlier=sc.outlier)
    # a table with room for one row: refused, nothing written; without arrays the counts alone come back
    keep = []
    f = st._sft_frame(sc.kp, sc.octave, R.INV_LEVEL_SIGMA2, sc.frame_points, sc.outlier, keep)
    tab = st._sft_table(len(sc.frame_points), keep)
    tab.capacity, tab.M = 1, -7
    L = gpu_ctx._L
    assert L.dsh_track_sft_observations(st._h, C.byref(f), C.byref(tab)) == _lib.DSH_ERR_ARG and tab.M == -7
    assert "capacity (1) < M" in L.dsh_last_error(gpu_ctx._h).decode()
    bare = _lib.TrackSftTableC()
    assert L.dsh_track_sft_observations(st._h, C.byref(f), C.byref(bare)) == _lib.DSH_OK and (bare.M, bare.points_obs) == (len(t.kp_index), t.points_obs)
    assert snapshot(st) == orig
    st.close()
