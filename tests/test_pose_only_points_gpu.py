"""GPU tests of dsh_track_pose_only and dsh_track_pose_only_batch at the operating points of tests/pose_only_points.py: cameras with
fx / fy = 1.8 and its inverse, worlds in which the frame's pose enters through each non-trace branch of the matrix -> quaternion
conversion with a small w, scenes 0.15 x and 8 x the size, sigma tables of 1, 8 and 32 levels, points behind the camera.  Against the
"device"-order restatement of tests/pose_only_ref.py, exactly as tests/test_pose_only_gpu.py compares its cases (its check()), with the
tolerances measured for these points (tests/test_pose_only_points_cpu.py, which has also checked every point's eligibility); against the
known pose without the restatement; and as one mixed batch, forwards and backwards, in which every problem has its own K, its own table
and its own N."""
import numpy as np
import pytest

import pose_only_points as PP
import pose_only_ref as R
import store_model
from test_pose_only_gpu import check, frame_of, store_of

pytestmark = pytest.mark.gpu

_REF = {}


def case(name):
    """model, frame and the "device"-order restatement of a point, every flag set on entry: computed once, shared, not modified."""
    if name not in _REF:
        model, fr, _ = PP.build(name)
        _REF[name] = (model, fr, R.solve(model, fr, "device", outlier=np.ones(len(fr.frame_points), bool)))
    return _REF[name]


def check_point(g, name, what=""):
    pt, (_, fr, ref) = PP.POINTS[name], case(name)
    print(f"{what}{name}: world {pt.world} branch {PP.quaternion_branch(fr.Tcw)} raw w {ref.stats['start_raw_w']:+.4f} | iters {g.iters.tolist()} "
          f"(restatement {[r.iters for r in ref.rounds]}) trials {g.trials.tolist()} (restatement {[r.trials for r in ref.rounds]})")
    check(g, ref, what + name, pose_tol=PP.POSE_TOL[pt.z0], chi2_rtol=PP.CHI2_RTOL)


def merged(names):
    """The points `names` against ONE store: their models one after the other, each frame's ids moved behind the earlier ones', every
    flag set on entry."""
    from defslam_amd import localmap
    model, frames = store_model.MapModel(), []
    for n in names:
        m, fr, _ = case(n)
        base = len(model.points)
        for p in m.points:
            model.add_point(xyz=p.xyz, bad=p.bad)
        fp = np.where(fr.frame_points >= 0, fr.frame_points + base, -1).astype(np.int32)
        frames.append(localmap.PoseOnlyFrame(fr.Tcw, fr.K, fr.kp, fr.octave, fr.inv_level_sigma2, fp, np.ones(len(fp), bool)))
    return model, frames


def raw(results):
    return [b"".join(np.ascontiguousarray(getattr(r, f)).tobytes() for f in r.__dataclass_fields__) for r in results]


@pytest.mark.parametrize("name", PP.POINT_NAMES)
def test_single_call_equals_the_restatement(gpu_ctx, name):
    """Flags, counts, rounds, iterations, trials and bad per round exactly; pose and chi2 within 16 x the measured reassociation noise of
    the point's scale; Tcw_out within one float32 ulp; the store unchanged.  behind_camera is one of the points."""
    model, fr, _ = case(name)
    st = store_of(gpu_ctx, model)
    before = (st.get_points(), st.get_state())
    g = st.pose_only(fr.Tcw, fr.K, fr.kp, fr.octave, fr.inv_level_sigma2, fr.frame_points, outlier=np.ones(len(fr.frame_points), bool))
    check_point(g, name)
    for a, b in zip(before, (st.get_points(), st.get_state())):
        for f in a.__dataclass_fields__:
            assert np.array_equal(getattr(a, f), getattr(b, f)), (name, f)
    store_model.assert_state(st, model, name)
    st.close()


@pytest.mark.parametrize("name", list(PP.NOISE_FREE))
def test_noise_free_matches_give_the_known_pose(gpu_ctx, name):
    """Not through the restatement: for each world and scale Tcw_out is the known moved pose [R | z0 t] G^-1 to 10 x the float32 spacing
    of its entries.  A mistake that the kernel and the restatement share in what shapes the converged pose -- the rotation by a
    quaternion with a small w, the Jacobian at fx != fy, the float32 matrix of the result -- does not pass here; one in the conversion of
    the start pose is optimised away, which is why the next test looks at that conversion alone."""
    model, fr, want = PP.build_noise_free(name)
    want = want.astype(np.float32)
    st = store_of(gpu_ctx, model)
    g = st.pose_only(fr.Tcw, fr.K, fr.kp, fr.octave, fr.inv_level_sigma2, fr.frame_points)
    st.close()
    err, bound = np.abs(g.Tcw - want), 10 * np.spacing(np.abs(want).astype(np.float32))
    print(f"{name}: branch {PP.quaternion_branch(fr.Tcw)}, largest error / bound {float((err / bound).max()):.3f}, largest error {float(err.max()):.3e}")
    assert PP.quaternion_branch(fr.Tcw) == PP.WORLD_BRANCH[PP.NOISE_FREE[name].world]
    assert (g.n_initial, g.n_good, g.rounds) == (80, 80, 4), name
    assert (err <= bound).all(), (name, float((err / bound).max()))


def test_the_start_pose_conversion_against_scipy(gpu_ctx):
    """Not through the restatement either: with two held key points the call returns before it optimises and `pose` is the frame's
    pose as the kernel converted it.  For the start pose of every point and every noise-free case, in one batch: the translation's
    float32 values, and scipy's quaternion of the same matrix with w >= 0, to 4e-7 (the entries are float32, so the matrix is a
    rotation to that; tests/test_pose_only_points_cpu.py compares the restatement in the same way).  The noise-free test above does
    not see this conversion: a wrong start is optimised away."""
    from defslam_amd import localmap
    from scipy.spatial.transform import Rotation
    model = store_model.MapModel()
    for x in ((0.1, 0.2, 4.0), (-0.3, 0.1, 5.0)):
        model.add_point(xyz=x)
    poses = {n: PP.build(n)[1].Tcw for n in PP.POINT_NAMES}
    poses.update({n: PP.build(PP.NOISE_FREE[n])[1].Tcw for n in PP.NOISE_FREE})
    K, kp, oc, fp = np.array(PP.CAMERAS["hamlyn"][:4], np.float32), np.full((2, 2), 100, np.float32), np.zeros(2, np.int32), np.arange(2, dtype=np.int32)
    st = store_of(gpu_ctx, model)
    res = st.pose_only_batch([localmap.PoseOnlyFrame(T, K, kp, oc, R.sigma_table(), fp) for T in poses.values()])
    st.close()
    branches = set()
    for (n, T), g in zip(poses.items(), res):
        q = Rotation.from_matrix(T[:3, :3].astype(float)).as_quat()
        q = q if q[3] >= 0 else -q
        print(f"{n}: branch {PP.quaternion_branch(T)}, w {g.pose[6]:.4f}, largest difference to scipy {np.abs(g.pose[3:] - q).max():.2e}")
        assert g.rounds == 0 and g.n_initial == 2 and np.array_equal(g.Tcw, T), n
        assert g.pose[:3].tolist() == [float(v) for v in T[:3, 3]] and g.pose[6] >= 0, n
        assert np.abs(g.pose[3:] - q).max() < 4e-7, (n, g.pose[3:], q)
        branches.add(PP.quaternion_branch(T))
    assert branches == {"trace", 0, 1, 2}


def test_a_mixed_batch_forwards_and_backwards(gpu_ctx):
    """Every point in one call against one store, interleaved: each problem has its own K, its own table (1, 8 or 32 levels) and its own
    N, and the one with n_initial < 3 is in the middle.  The batch is byte for byte its single calls, a second run byte for byte the
    first, each result equals its own restatement, and problem b of the batch in reverse order is byte for byte problem B - 1 - b of
    the forward one: no problem reads another's table, key points or K, or those of problem 0."""
    names = PP.plan()
    B = len(names)
    model, frames = merged(names)
    assert len({f.inv_level_sigma2.tobytes() for f in frames}) >= 5 and len({tuple(f.K.tolist()) for f in frames}) == 5
    assert {len(f.inv_level_sigma2) for f in frames} == {1, 8, 32} and len({len(f.frame_points) for f in frames}) >= 6
    st = store_of(gpu_ctx, model)
    first = st.pose_only_batch(frames)
    again = st.pose_only_batch(frames)
    single = [st.pose_only(f.Tcw, f.K, f.kp, f.octave, f.inv_level_sigma2, f.frame_points, f.outlier) for f in frames]
    back = st.pose_only_batch(frames[::-1])
    store_model.assert_state(st, model, "mixed batch")
    st.close()
    assert raw(first) == raw(again)
    for b, n in enumerate(names):
        assert raw(first)[b] == raw(single)[b], (b, n)
        assert raw(back)[B - 1 - b] == raw(first)[b], (b, n)
        check_point(first[b], n, f"batch[{b}] ")
    k = names.index("turn_y_held2")
    assert 0 < k < B - 1 and first[k].n_initial == 2 and first[k].rounds == 0 and [r.rounds for r in first].count(0) == 1


def test_octaves_at_the_edge_of_the_table(gpu_ctx):
    """octave = levels - 1 on every held key point of a 32-level table, and a table of one level (every octave 0), each as the second
    problem of a batch behind one with another table: equal to the restatement.  There octave = levels on a hole is not read, and on a
    held key point it is refused by name."""
    for names in (["turn_z_one_level", "turn_x_top_octave"], ["turn_y_big_32_levels", "turn_z_one_level"]):
        model, frames = merged(names)
        f = frames[1]
        levels = len(f.inv_level_sigma2)
        held = f.frame_points >= 0
        assert (f.octave[held] == levels - 1).all() and levels in (1, PP.PO_MAX_LEVELS) and levels != len(frames[0].inv_level_sigma2)
        st = store_of(gpu_ctx, model)
        plain = st.pose_only_batch(frames)
        check_point(plain[1], names[1], "second of two: ")
        oc = f.octave.copy()
        oc[~held] = levels                                                   # past the table's end, and the batch's when it is the last
        oc[np.nonzero(~held)[0][0]] = 99
        f.octave = oc
        assert raw(st.pose_only_batch(frames)) == raw(plain), names
        i = int(np.nonzero(held)[0][-1])
        oc[i] = levels
        with pytest.raises(Exception, match=rf"dsh_track_pose_only_batch: problem 1: octave\[{i}\] outside"):
            st.pose_only_batch(frames)
        st.close()
