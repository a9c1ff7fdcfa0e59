"""GPU tests of dsh_track_pose_only and dsh_track_pose_only_batch against the "device"-order restatement of tests/pose_only_ref.py.
Exact: the flags, n_initial, n_bad, n_good, rounds, and iters, trials and bad per round.  Within POSE_TOL / CHI2_RTOL (16 x the
reassociation noise of the reference itself, measured by tests/test_pose_only_cpu.py): pose and chi2.  Within one float32 ulp per entry:
Tcw_out.  Every case runs against a store with holes in frame_points, at least three octaves, bad points that still take part and one
id held by two key points; the cases and their seeds are GPU_CASES of the restatement, for each of which the CPU test has checked
that the two summation orders agree on every decision."""
import numpy as np
import pytest

import pose_only_ref as R
import store_model

pytestmark = pytest.mark.gpu

_REF = {}


def case(name):
    """model, frame and the "device"-order restatement of a case: computed once, shared, not modified."""
    if name not in _REF:
        model, fr, _ = R.make_case(**R.GPU_CASES[name])
        _REF[name] = (model, fr, R.solve(model, fr, "device", outlier=np.ones(len(fr.frame_points), bool)))
    return _REF[name]


def store_of(ctx, model):
    from defslam_amd import localmap
    st = localmap.MapPointStore(ctx, points=64)
    model.fill(st)
    return st


def frame_of(fr, outlier=None):
    from defslam_amd import localmap
    return localmap.PoseOnlyFrame(fr.Tcw, fr.K, fr.kp, fr.octave, fr.inv_level_sigma2, fr.frame_points, outlier)


def check(g, ref, name, pose_tol=R.POSE_TOL, chi2_rtol=R.CHI2_RTOL):
    """A result against the restatement's; tests/test_pose_only_points_gpu.py passes the tolerances measured for its points."""
    print(f"{name}: n_initial {g.n_initial} rounds {g.rounds} iters {g.iters.tolist()} trials {g.trials.tolist()} bad {g.bad.tolist()} | "
          f"pose diff {np.abs(g.pose - ref.pose).max():.3e} (tol {pose_tol:.3e})")
    nr = len(ref.rounds)
    assert (g.n_initial, g.n_bad, g.n_good, g.rounds) == (ref.n_initial, ref.n_bad, ref.n_good, nr), name
    assert g.iters.tolist() == [r.iters for r in ref.rounds] + [0] * (4 - nr), name
    assert g.trials.tolist() == [r.trials for r in ref.rounds] + [0] * (4 - nr), name
    assert g.bad.tolist() == [r.bad for r in ref.rounds] + [0] * (4 - nr), name
    assert np.array_equal(g.outlier, ref.outlier), name
    assert np.abs(g.pose - ref.pose).max() <= pose_tol, (name, np.abs(g.pose - ref.pose).max())
    for k, r in enumerate(ref.rounds):
        assert abs(g.chi2[k] - r.chi2) <= chi2_rtol * max(r.chi2, 1.0), (name, k, g.chi2[k], r.chi2)
    assert (g.chi2[nr:] == 0).all(), name
    assert np.abs(g.Tcw.view(np.int32).astype(np.int64) - ref.Tcw.view(np.int32)).max() <= 1, name
    if nr == 0:
        assert np.array_equal(g.Tcw, ref.Tcw), name                      # the input pose, bit for bit


@pytest.mark.parametrize("name", list(R.GPU_CASES))
def test_single_call_equals_the_restatement(gpu_ctx, name):
    """The entries without a point keep the caller's flag (all ones on entry), the others are written."""
    model, fr, ref = case(name)
    st = store_of(gpu_ctx, model)
    before = (st.get_points(), st.get_state())
    g = st.pose_only(fr.Tcw, fr.K, fr.kp, fr.octave, fr.inv_level_sigma2, fr.frame_points, outlier=np.ones(len(fr.frame_points), bool))
    check(g, ref, name)
    # the store is unchanged: positions, counters and lists read back equal
    for a, b in zip(before, (st.get_points(), st.get_state())):
        for f in a.__dataclass_fields__:
            assert np.array_equal(getattr(a, f), getattr(b, f)), (name, f)
    store_model.assert_state(st, model, name)
    st.close()


def test_a_batch_equals_its_single_calls_and_itself(gpu_ctx):
    """Three problems with different N against one store, the middle one with n_initial < 3: byte for byte the three single calls, and
    a second run of the batch byte for byte the first."""
    names = ["held65", "held2", "outliers20"]
    model, frames = store_model.MapModel(), []
    for n in names:
        m, fr, _ = R.make_case(**R.GPU_CASES[n])
        base = len(model.points)
        for pt in m.points:
            model.add_point(xyz=pt.xyz, bad=pt.bad)
        fp = np.where(fr.frame_points >= 0, fr.frame_points + base, -1).astype(np.int32)
        frames.append(R.Frame(fr.Tcw, fr.K, fr.kp, fr.octave, fr.inv_level_sigma2, fp))
    st = store_of(gpu_ctx, model)

    def raw(results):
        return [b"".join(np.ascontiguousarray(getattr(r, f)).tobytes() for f in r.__dataclass_fields__) for r in results]

    first = st.pose_only_batch([frame_of(f) for f in frames])
    again = st.pose_only_batch([frame_of(f) for f in frames])
    single = [st.pose_only(f.Tcw, f.K, f.kp, f.octave, f.inv_level_sigma2, f.frame_points) for f in frames]
    assert raw(first) == raw(again) and raw(first) == raw(single)
    assert [r.rounds for r in first] == [4, 0, 4] and first[1].n_initial == 2
    for n, g in zip(names, first):                                       # and each equals its own case's restatement
        ref = case(n)[2]
        g.outlier = g.outlier | (case(n)[1].frame_points < 0)            # case() ran with every flag set on entry
        check(g, ref, "batch " + n)
    st.close()


def test_refusals_that_need_a_point_in_the_store(gpu_ctx):
    """An octave outside the levels is refused where a point is held and not read where none is; an id outside the store is named."""
    from defslam_amd import localmap
    model, fr, _ = case("held9")
    st = store_of(gpu_ctx, model)
    i, hole = int(np.nonzero(fr.frame_points >= 0)[0][0]), int(np.nonzero(fr.frame_points < 0)[0][0])
    oc = fr.octave.copy()
    oc[hole] = 99
    g = st.pose_only(fr.Tcw, fr.K, fr.kp, oc, fr.inv_level_sigma2, fr.frame_points)
    assert g.n_initial == 9
    oc[i] = R.LEVELS
    with pytest.raises(Exception, match=rf"dsh_track_pose_only: octave\[{i}\] outside"):
        st.pose_only(fr.Tcw, fr.K, fr.kp, oc, fr.inv_level_sigma2, fr.frame_points)
    fp = fr.frame_points.copy()
    fp[i] = st.n_points
    with pytest.raises(Exception, match=rf"dsh_track_pose_only_batch: problem 1: frame_points\[{i}\]"):
        st.pose_only_batch([frame_of(fr), localmap.PoseOnlyFrame(fr.Tcw, fr.K, fr.kp, fr.octave, fr.inv_level_sigma2, fp)])
    assert st.pose_only_batch([]) == []
    st.close()


def test_a_point_behind_the_camera_returns_a_status(gpu_ctx):
    """Not covered numerically: a point at and one behind the camera plane give non-finite or meaningless residuals; the call returns
    and the counts stay consistent."""
    model, fr, _ = R.make_case(**R.GPU_CASES["held10"])
    held = np.nonzero(fr.frame_points >= 0)[0]
    T = np.eye(4, dtype=np.float32)
    model.points[int(fr.frame_points[held[0]])].xyz[:] = (0.5, 0.5, 0.0)
    model.points[int(fr.frame_points[held[1]])].xyz[:] = (0.5, 0.5, -2.0)
    st = store_of(gpu_ctx, model)
    g = st.pose_only(T, fr.K, fr.kp, fr.octave, fr.inv_level_sigma2, fr.frame_points)
    assert g.n_initial == 10 and g.rounds == 4 and 0 <= g.n_bad <= 10 and g.n_good == 10 - g.n_bad
    st.close()
