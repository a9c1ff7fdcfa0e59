"""GPU parity tests of the SfT solve away from the one synthetic camera, pose and weight triple (tests/operating_points.py): cameras with
fx != fy, poses that enter through every branch of the matrix -> quaternion conversion, other regulariser weights (RegTemp = 0 among
them), scene scales 0.15 and 8, clean and heavily contaminated matches, other key point counts -- in the normal equations, latency mode,
the throughput shape (camera, weights and key point count differing from problem to problem inside one batch), the wide-band solvers
and with 0 / 1 / 2 neighbour layers.  Every comparison is the strict one of test_sft_gpu.py's _compare: tests/test_operating_points_cpu.py
holds every problem solved here to the eligibility conditions, so there is no relaxed case."""
import numpy as np
import pytest

import operating_points as op
from conftest import oracle_args
from test_sft_gpu import _compare, _solve_gpu, rounds_ctx  # noqa: F401  (rounds_ctx: the fixture)

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _oracle(oracle_mod, key, tmpl, fr, regs, layers=1):
    """oracle.sft_solve (ldlt_mode 1) of a problem, computed once per key and shared between tests."""
    if key not in _ORACLE:
        tc, args = oracle_args(oracle_mod, tmpl, fr, regs=regs)
        _ORACLE[key] = oracle_mod.sft_solve(*args, layers=layers, ldlt_mode=1)
    return _ORACLE[key]


def _fr_like(fr):
    return dict(Tcw=fr.Tcw, K=fr.K, n_frame=fr.n_frame, obs_nodes=fr.obs_nodes, obs_bary=fr.obs_bary, obs_uv=fr.obs_uv, obs_invsig2=fr.obs_invsig2, xyz=fr.xyz)


def _compare_all(f, inl, r, z0):
    """_compare, the float32 pose the caller gets back and the per-observation errors."""
    _compare(f, inl, r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret, scene_scale=z0)
    assert f.trials == r.trials and f.dim == r.dims[0]
    np.testing.assert_allclose(f.Tcw, r.Tcw, rtol=0, atol=2e-7 * max(1.0, float(np.abs(r.Tcw[:3, 3]).max())))
    np.testing.assert_allclose(f.chi2_obs, r.chi2_obs, rtol=1e-8, atol=1e-12)


@pytest.mark.parametrize("case", op.NORMAL_EQ_CASES)
@pytest.mark.parametrize("shape,m,pid", [((10, 10), 300, 1), ((25, 20), 1000, 2), ((6, 17), 120, 3), ((8, 30), 400, 4), ((6, 41), 400, 5)])
def test_normal_equations_match_oracle_at_other_operating_points(lab_ctx, oracle_mod, shape, m, pid, case):
    """test_normal_equations_match_oracle (its five shapes select the record placement classes) at fx > fy with an oblique pose and the webcam
    weights, and at fy > fx with a pose near a half turn about y and RegTemp = 0: one linearisation each."""
    from defslam_amd import sft
    tmpl, fr, regs = op.make_problem(case, *shape, m, pid)
    rng = np.random.default_rng(pid)
    fr.xyz = fr.xyz + rng.normal(scale=0.002, size=fr.xyz.shape)   # non-trivial curvature / stretch residuals
    tc, args = oracle_args(oracle_mod, tmpl, fr, regs=regs)
    Ho, bo, chio = oracle_mod.sft_system(*args)
    lab_ctx.template_build(tmpl.xyz0, tmpl.facets)
    lab_ctx.batch_upload([sft.frame_from_synth(fr)], *regs)
    Hg, bg, chig = lab_ctx.debug_system(0, Ho.shape[0])
    assert chig == pytest.approx(chio, rel=1e-12)
    np.testing.assert_allclose(Hg, Ho, rtol=1e-9, atol=1e-11 * np.abs(Ho).max())
    np.testing.assert_allclose(bg, bo, rtol=1e-9, atol=1e-11 * np.abs(bo).max())
    np.testing.assert_array_equal(np.abs(Hg) > 0, np.abs(Ho) > 0)


@pytest.mark.parametrize("case", op.CASE_NAMES)
def test_latency_mode_matches_oracle_on_every_case(gpu_ctx, oracle_mod, case):
    """DefPoseOptimization of one frame (9 x 14 mesh, 420 matches) against the oracle at every named operating point."""
    c = op.CASES[case]
    tmpl, fr, regs = op.make_problem(c, *op.MESH)
    r = _oracle(oracle_mod, ("latency", case), tmpl, fr, regs)
    f, inl = _solve_gpu(gpu_ctx, tmpl.xyz0, tmpl.facets, _fr_like(fr), regs)
    _compare_all(f, inl, r, c.z0)


@pytest.mark.parametrize("world,z0", op.BATCH_PLACEMENTS, ids=[f"{w}-z0={z:g}" for w, z in op.BATCH_PLACEMENTS])
def test_throughput_shape_with_cameras_weights_and_key_point_counts_mixed_in_one_batch(rounds_ctx, oracle_mod, world, z0):
    """Two problems per compute unit on the 9 x 14 mesh, as rounds of phase kernels to the end and with the product's tail kernel.  Problem b
    belongs to case batch_plan[b] -- interleaved, not sorted -- and takes that case's camera (five pinholes, fx > fy, fy > fx), weights (four
    triples, RegTemp = 0 among them), noise and key point count; the batch's one template fixes the placement and the scale, so these are the
    parameter of the test (poses through the trace branch and both half-turn branches of the other axes, scales 1, 0.15 and 8).  A kernel that
    took problem 0's camera or weights for every problem fails here.  Per case: two of its problems against the oracle; every one of its
    problems (identical inputs) against the same frame solved alone in latency mode, to 1e-9 relative; two runs bit-identical."""
    from defslam_amd import _lib, sft
    B = 2 * _lib.device_cus(0)
    plan = op.batch_plan(B)
    probs = {name: op.batch_problem(world, z0, name) for name in op.CASE_NAMES}
    tmpl = probs[op.CASE_NAMES[0]][0]
    for t, _, _ in probs.values():
        np.testing.assert_array_equal(t.xyz0, tmpl.xyz0)            # one template for the batch
    assert len({tuple(fr.K) for _, fr, _ in probs.values()}) == len(op.CAMERAS) and len({regs for _, _, regs in probs.values()}) == len(op.WEIGHTS)
    rounds_ctx.template_build(tmpl.xyz0, tmpl.facets)
    frames = []
    for name in plan:
        f = sft.frame_from_synth(probs[name][1])
        f.regs = probs[name][2]
        frames.append(f)
    rounds_ctx.batch_upload(frames, 1.0, 1.0, 1.0, 1, 50)            # the call's weights are nobody's: every frame brings its own
    assert int(rounds_ctx.problem_info(0)[1][7]) == 1, "two problems per CU must run as rounds of phase kernels (one wavefront per problem)"
    snaps = []
    for _ in range(2):
        rounds_ctx.batch_run()
        inl = rounds_ctx.batch_download()
        snaps.append([(int(i), f.iters, f.trials, f.status, f.nodes_xyz.copy(), f.pose7.copy(), f.chi2_obs.copy(), f.mvbOutlier.copy(), f.trace.copy(), f.Tcw.copy())
                      for i, f in zip(inl, frames)])
    for a, b in zip(*snaps):
        assert a[:4] == b[:4]
        for u, v in zip(a[4:], b[4:]):
            np.testing.assert_array_equal(u, v)
    inl = [s[0] for s in snaps[1]]
    for name in op.CASE_NAMES:
        _, fr, regs = probs[name]
        members = [b for b in range(B) if plan[b] == name]
        assert len(members) >= 2
        r = _oracle(oracle_mod, ("batch", world, z0, name), tmpl, fr, regs)
        for b in (members[0], members[-1]):
            _compare_all(frames[b], inl[b], r, z0)
        one, i1 = _solve_gpu(rounds_ctx, tmpl.xyz0, tmpl.facets, _fr_like(fr), regs)      # alone: latency mode
        for b in members:
            f = frames[b]
            assert (inl[b], f.iters, f.trials) == (i1, one.iters, one.trials), (name, b)
            np.testing.assert_array_equal(f.trace[:, [2, 6]], one.trace[:, [2, 6]])
            np.testing.assert_array_equal(f.mvbOutlier, one.mvbOutlier)
            assert np.abs(f.nodes_xyz - one.nodes_xyz).max() <= 1e-9 * np.abs(one.nodes_xyz).max(), (name, b)
            np.testing.assert_array_equal(f.nodes_xyz, frames[members[0]].nodes_xyz)      # identical inputs, identical bits, wherever they sit in the batch
            np.testing.assert_array_equal(f.pose7, frames[members[0]].pose7)


@pytest.mark.parametrize("rows,cols,m,pid", op.WIDE, ids=["6x41", "5x45"])
def test_wide_bands_at_another_operating_point(lab_ctx, oracle_mod, rows, cols, m, pid):
    """Half-bandwidth 248 (the two-sided / wide tile solver) and 272 (the row-major fallback) at fx != fy, a pose near a half turn about x and
    the webcam weights, through the library's defaults against the oracle.  6 x 41 also with the lab's "split" on and off, each against the
    oracle and against each other as test_two_sided_factorisation_follows_the_undivided_one_and_the_oracle compares them: iterations, trials,
    accept flags, outliers and inliers identical, numbers to 1e-9 -- the two-sided factorisation eliminates in another order, so the floats
    are equal to rounding, not bit for bit (measured on an MI355X: vertices differ by 3.1e-14, the pose by 2.2e-13)."""
    c = op.CASES[op.WIDE_CASE]
    tmpl, fr, regs = op.make_problem(c, rows, cols, m, pid)
    r = _oracle(oracle_mod, ("wide", rows, cols), tmpl, fr, regs)
    f, inl = _solve_gpu(lab_ctx, tmpl.xyz0, tmpl.facets, _fr_like(fr), regs)
    assert (128 < f.half_bandwidth <= 256) == (cols == 41) and (f.half_bandwidth > 256) == (cols == 45)
    _compare_all(f, inl, r, c.z0)
    if cols != 41:
        return
    runs = {}
    try:
        for split in (1, 0):
            lab_ctx.set_option("split", split)
            runs[split] = _solve_gpu(lab_ctx, tmpl.xyz0, tmpl.facets, _fr_like(fr), regs)
            assert lab_ctx.solver_info(0)["split"] == split
    finally:
        lab_ctx.set_option("split", 2)                                  # the library's default
    (s1, inl_s), (u, inl_u) = runs[1], runs[0]
    _compare_all(u, inl_u, r, c.z0)
    _compare_all(s1, inl_s, r, c.z0)
    assert (inl_s, s1.iters, s1.trials) == (inl_u, u.iters, u.trials)
    np.testing.assert_array_equal(s1.trace[:, 6:], u.trace[:, 6:])
    np.testing.assert_array_equal(s1.mvbOutlier, u.mvbOutlier)
    np.testing.assert_allclose(s1.trace[:, :6], u.trace[:, :6], rtol=1e-7)
    np.testing.assert_allclose(s1.nodes_xyz, u.nodes_xyz, rtol=0, atol=1e-9 * np.abs(u.nodes_xyz).max())
    np.testing.assert_allclose(s1.pose7, u.pose7, rtol=0, atol=1e-9)


def test_neighbour_layers_on_a_partial_view(gpu_ctx, oracle_mod):
    """NeighboursLayers 0, 1, 2 on a frame that sees seven of the fourteen columns: without the ring of neighbours fewer nodes are optimised
    (a smaller system), layer 0 and layer 1 each against the oracle, and 2 gives the bits of 1 (the reference adds one ring for any value
    >= 1)."""
    rows, cols, m, pid, kc = op.LAYERS_VIEW
    c = op.CASES[op.LAYERS_CASE]
    tmpl, fr, regs = op.make_problem(c, rows, cols, m, pid, keep_cols=kc)
    out = {}
    for layers in (0, 1, 2):
        out[layers] = _solve_gpu(gpu_ctx, tmpl.xyz0, tmpl.facets, _fr_like(fr), regs, layers=layers)
    for layers in (0, 1):
        r = _oracle(oracle_mod, ("layers", layers), tmpl, fr, regs, layers=layers)
        _compare_all(out[layers][0], out[layers][1], r, c.z0)
    assert out[0][0].dim < out[1][0].dim < 6 + 3 * tmpl.n
    (f1, i1), (f2, i2) = out[1], out[2]
    assert (i1, f1.iters, f1.trials, f1.dim) == (i2, f2.iters, f2.trials, f2.dim)
    for k in ("nodes_xyz", "pose7", "chi2_obs", "mvbOutlier", "trace", "Tcw"):
        np.testing.assert_array_equal(getattr(f1, k), getattr(f2, k))
    unseen = [col + cols * r_ for r_ in range(rows) for col in range(kc + 1, cols)]
    np.testing.assert_array_equal(out[0][0].nodes_xyz[unseen], fr.xyz[unseen])     # fixed vertices come back bit-identical
