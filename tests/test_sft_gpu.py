"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI, against
the CPU oracle on the same seeded inputs, against the committed golden vectors, and through
size-independent properties at the full BASELINE.json sizes.

Tolerance (north_star): mesh-vertex positions and camera pose within 1e-4 relative of the CPU path;
we assert 1e-7 / 1e-8 -- the HIP path follows the oracle's accept/reject sequence exactly and differs only
by summation order and FMA contraction.  Indexing, iteration counts, trial counts and outlier flags are
compared exactly.
"""
import glob
import os

import numpy as np
import pytest

from conftest import oracle_args

pytestmark = pytest.mark.gpu

GOLDEN = sorted(p for p in glob.glob(os.path.join(os.path.dirname(__file__), "golden", "sft_*.npz")) if "sft_C5_" not in os.path.basename(p))
# full-size stress problems (BASELINE configs[4]): outputs of the C oracle, inputs regenerated from the seeds (make_golden_c5.py)
GOLDEN_C5 = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "sft_C5_p*.npz")))
VERT_TOL = 1e-7
POSE_TOL = 1e-8


def _solve_gpu(ctx, tmpl_xyz0, facets, fr_like, regs, layers=1, max_iters=50):
    from defslam_amd import sft
    ctx.template_build(tmpl_xyz0, facets)
    f = sft.Frame(Tcw=np.array(fr_like["Tcw"], np.float32), K=np.array(fr_like["K"], float), N=int(fr_like["n_frame"]),
                  obs_nodes=fr_like["obs_nodes"], obs_bary=fr_like["obs_bary"], obs_uv=fr_like["obs_uv"], obs_invsig2=fr_like["obs_invsig2"],
                  nodes_xyz=np.array(fr_like["xyz"], float))
    inl = sft.DefPoseOptimization(ctx, f, regs[0], regs[1], regs[2], layers, max_iters)
    return f, inl


def _compare(f, inl, r_xyz, r_pose7, r_trace, r_outlier, r_rep, r_inl, scene_scale=1.0):
    """scene_scale: the translation of the pose is in scene units, so its bound is POSE_TOL * max(1, scene scale)."""
    assert f.status == 0
    assert f.iters == r_trace.shape[0]
    np.testing.assert_array_equal(f.trace[:, 2], r_trace[:, 2])      # trials per iteration
    np.testing.assert_array_equal(f.trace[:, 6], r_trace[:, 6])      # accepted flags
    np.testing.assert_allclose(f.trace[:, [0, 1, 3, 4]], r_trace[:, [0, 1, 3, 4]], rtol=1e-8)
    scale = np.abs(r_xyz).max()
    assert np.abs(f.nodes_xyz - r_xyz).max() <= VERT_TOL * scale
    assert np.abs(f.pose7[3:] - r_pose7[3:]).max() <= POSE_TOL
    assert np.abs(f.pose7[:3] - r_pose7[:3]).max() <= POSE_TOL * max(1.0, scene_scale)
    np.testing.assert_array_equal(f.mvbOutlier, np.asarray(r_outlier, bool))
    assert inl == r_inl
    assert f.rep_error_f64 == pytest.approx(r_rep, rel=1e-9)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_hip_matches_golden_vectors(gpu_ctx, path):
    g = np.load(path)
    f, inl = _solve_gpu(gpu_ctx, g["xyz0"], g["facets"], g, tuple(g["regs"]), int(g["layers"]))
    _compare(f, inl, g["out_xyz"], g["out_pose7"], g["out_trace"], g["out_outlier"], float(g["out_rep_error"]), int(g["out_inliers"]))
    np.testing.assert_allclose(f.chi2_obs, g["out_chi2_obs"], rtol=1e-8, atol=1e-12)


@pytest.mark.parametrize("path", GOLDEN_C5, ids=[os.path.basename(p) for p in GOLDEN_C5])
def test_hip_matches_golden_vectors_full_size_c5(gpu_ctx, path):
    """BASELINE.json configs[4] per problem: 2000-node template (40x50), 4000 matches, D = 6006, half-bandwidth 248 -> the wide
    tile solver at full size against the C oracle's dense solve (15 minutes of CPU per problem, done once in the build
    container: tests/golden/make_golden_c5.py).  Same LM trajectory, vertices / pose / per-observation chi2 / outliers."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden_c5 import input_digest
    from defslam_amd import synth
    g = np.load(path)
    pid = int(g["problem_id"])
    tmpl, fr = synth.make_problem("C5", pid)
    assert input_digest(tmpl, fr) == str(g["input_sha256"]), "defslam_amd/synth.py no longer generates the inputs this fixture was computed for"
    f, inl = _solve_gpu(gpu_ctx, tmpl.xyz0, tmpl.facets, dict(Tcw=fr.Tcw, K=fr.K, n_frame=fr.n_frame, obs_nodes=fr.obs_nodes, obs_bary=fr.obs_bary,
                                                              obs_uv=fr.obs_uv, obs_invsig2=fr.obs_invsig2, xyz=fr.xyz), tuple(g["regs"]))
    assert f.dim == int(g["out_dims"][0]) == 6006 and 128 < f.half_bandwidth <= 256
    _compare(f, inl, g["out_xyz"], g["out_pose7"], g["out_trace"], g["out_outlier"], float(g["out_rep_error"]), int(g["out_inliers"]))
    assert f.trials == int(g["out_trials"])
    np.testing.assert_allclose(f.chi2_obs, g["out_chi2_obs"], rtol=1e-7, atol=1e-12)
    np.testing.assert_allclose(f.Tcw, g["out_Tcw"], atol=2e-7)


def test_c5_batch_of_16_equals_singles_bit_for_bit(gpu_ctx):
    """BASELINE.json configs[4]: 16 concurrent 2000-node x 4000-match problems in ONE launch give, problem by problem, exactly
    the bits of 16 one-at-a-time solves (and problems 0/1 of them are the oracle-checked fixtures above)."""
    from defslam_amd import sft, synth
    rows, cols, m = synth.CONFIGS["C5"]
    tmpl = synth.make_grid_template(rows, cols)
    gpu_ctx.template_build(tmpl.xyz0, tmpl.facets)
    frames = [sft.frame_from_synth(synth.make_frame(tmpl, m, p)) for p in range(16)]
    inl = sft.DefPoseOptimizationBatch(gpu_ctx, frames, synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    assert all(f.status == 0 for f in frames)
    for p in range(16):
        one = sft.frame_from_synth(synth.make_frame(tmpl, m, p))
        i1 = sft.DefPoseOptimization(gpu_ctx, one, synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
        assert (i1, one.iters, one.trials) == (inl[p], frames[p].iters, frames[p].trials)
        np.testing.assert_array_equal(one.nodes_xyz, frames[p].nodes_xyz)
        np.testing.assert_array_equal(one.pose7, frames[p].pose7)
        np.testing.assert_array_equal(one.mvbOutlier, frames[p].mvbOutlier)
        np.testing.assert_array_equal(one.chi2_obs, frames[p].chi2_obs)
        assert one.rep_error_f64 == frames[p].rep_error_f64
    for path in GOLDEN_C5:   # the batch members with a fixture agree with the oracle as well
        g = np.load(path)
        f = frames[int(g["problem_id"])]
        assert f.iters == int(g["out_iters"]) and f.trials == int(g["out_trials"])
        assert np.abs(f.nodes_xyz - g["out_xyz"]).max() <= VERT_TOL * np.abs(g["out_xyz"]).max()


def test_benched_shape_matches_oracle_under_load(gpu_ctx, oracle_mod):
    """The configuration bench.py reports, checked against the oracle where it runs: the PRODUCT library, >= 1024 C2 problems in one
    batch (so that the throughput shape is chosen: rounds of LIN / FACTOR / TRIAL phase kernels with ONE wavefront per factorisation,
    four factorisations resident per CU -- asserted through dsh_sft_batch_problem_info: wavefronts per problem == 1), every compute unit
    loaded with other problems while the sampled ones are solved.  Sampled ids: first, last, middle, and neighbours in the work lists the
    persistent workgroups pull from; LM trajectory, vertices, pose, outliers against oracle.sft_solve through _compare.  The run is
    repeated three times and must reproduce itself bit for bit (the order in which the workgroups pull problems varies, the results must not)."""
    from defslam_amd import sft, synth
    B = 1024
    rows, cols, m = synth.CONFIGS["C2"]
    tmpl = synth.make_grid_template(rows, cols)
    gpu_ctx.template_build(tmpl.xyz0, tmpl.facets)
    regs = (synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    syn = [synth.make_frame(tmpl, m, p) for p in range(B)]
    frames = [sft.frame_from_synth(fr) for fr in syn]
    gpu_ctx.batch_upload(frames, *regs, 1, 50)
    _, counts = gpu_ctx.problem_info(0)
    assert int(counts[7]) == 1, "a batch of 1024 C2 problems must run as rounds of phase kernels (one wavefront per factorisation)"
    snaps = []
    for _ in range(3):
        gpu_ctx.batch_run()
        inl = gpu_ctx.batch_download()
        snaps.append([(int(i), f.iters, f.trials, f.nodes_xyz.copy(), f.pose7.copy(), f.chi2_obs.copy(), f.mvbOutlier.copy(), f.trace.copy())
                      for i, f in zip(inl, frames)])
    for rep in (1, 2):
        for p in range(B):
            a, b = snaps[0][p], snaps[rep][p]
            assert a[:3] == b[:3], (rep, p)
            for u, v in zip(a[3:], b[3:]):
                np.testing.assert_array_equal(u, v)
    tc = oracle_mod.template_build(tmpl.xyz0, tmpl.facets)
    ids = [0, 1, 2, 3, 255, 256, 257, 510, 511, 512, 513, 767, 768, 1000, 1022, 1023]
    for p in ids:
        fr = syn[p]
        r = oracle_mod.sft_solve(tc, fr.Tcw, fr.K, fr.n_frame, fr.obs_nodes, fr.obs_bary, fr.obs_uv, fr.obs_invsig2, fr.xyz, *regs, ldlt_mode=1)
        _compare(frames[p], snaps[2][p][0], r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret)
        assert frames[p].trials == r.trials


# batch sizes at the hand-over points, from the device's CU count (on 256 CUs: 65, 86, 129 and 300 problems -- the test ids)
LAUNCH_SHAPES = {
    "three_lanes": (lambda cus: cus // 4 + 1, 8),
    "two_lanes": (lambda cus: cus // 3 + 1, 8),
    "rounds_just_above_half": (lambda cus: cus // 2 + 1, 1),
    "rounds_tail_alone": (lambda cus: (cus * 75 + 63) // 64, 1),
}


@pytest.mark.parametrize("shape", list(LAUNCH_SHAPES), ids=["65-8", "86-8", "129-1", "300-1"])
def test_launch_shapes_between_latency_mode_and_rounds(gpu_ctx, oracle_mod, shape):
    """The hand-over points of r06 in the PRODUCT library, from the device's CU count: CUs / 4 + 1 problems = three speculative
    lanes per problem (the device holds 3 x B workgroups, not 4 x), CUs / 3 + 1 = two lanes, CUs / 2 + 1 and about 1.17 x CUs = the throughput
    shape with the tail kernel alone (until r05: one workgroup per problem of the persistent kernel).  A ragged batch on the 9 x 14 mesh,
    sampled ids against the oracle, two runs bit-identical."""
    from defslam_amd import _lib, sft, synth
    cus = _lib.device_cus(0)
    B, waves = LAUNCH_SHAPES[shape][0](cus), LAUNCH_SHAPES[shape][1]
    lanes = 4 if 4 * B <= cus else (3 if 3 * B <= cus else (2 if 2 * B <= cus else 1))
    assert lanes == {"three_lanes": 3, "two_lanes": 2}.get(shape, 1)
    tmpl = synth.make_grid_template(9, 14)
    gpu_ctx.template_build(tmpl.xyz0, tmpl.facets)
    regs = (synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    syn = []
    for p in range(B):
        fr = synth.make_frame(tmpl, 380 + 10 * (p % 5), p)
        if p % 4 == 2:   # a partial view: another active set, another dimension in the same batch
            keep = [c + 14 * r for r in range(9) for c in range(13)]
            sel = np.all(np.isin(fr.obs_nodes, keep), axis=1)
            for k in ["obs_nodes", "obs_bary", "obs_uv", "obs_invsig2"]:
                setattr(fr, k, getattr(fr, k)[sel])
        syn.append(fr)
    frames = [sft.frame_from_synth(fr) for fr in syn]
    gpu_ctx.batch_upload(frames, *regs, 1, 50)
    assert int(gpu_ctx.problem_info(0)[1][7]) == waves
    snaps = []
    for _ in range(2):
        gpu_ctx.batch_run()
        inl = gpu_ctx.batch_download()
        snaps.append([(int(i), f.iters, f.trials, f.nodes_xyz.copy(), f.pose7.copy()) for i, f in zip(inl, frames)])
    for a, b in zip(*snaps):
        assert a[:3] == b[:3]
        np.testing.assert_array_equal(a[3], b[3])
        np.testing.assert_array_equal(a[4], b[4])
    tc = oracle_mod.template_build(tmpl.xyz0, tmpl.facets)
    for p in (0, 1, 2, B // 2, B - 2, B - 1):
        fr = syn[p]
        r = oracle_mod.sft_solve(tc, fr.Tcw, fr.K, fr.n_frame, fr.obs_nodes, fr.obs_bary, fr.obs_uv, fr.obs_invsig2, fr.xyz, *regs, ldlt_mode=1)
        _compare(frames[p], snaps[1][p][0], r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret)


@pytest.mark.parametrize("lab", [False, True], ids=["product", "lab"])
def test_launch_shapes_in_turn_on_one_context_equal_fresh_contexts(request, lab):
    """One context takes the launch shapes one after the other -- tail kernel alone, latency mode with four lanes, three lanes, rounds + tail
    on the 9 x 14 mesh, then another template whose single problem is promoted and cut (C2), then the first shape again -- so every upload
    lays its arena out over what another shape left and replaces the plan the run functions read.  Every step: the expected shape
    (dsh_sft_batch_problem_info; in the lab build also lanes, cut and tile mode), and results bit for bit those of the same upload on a
    context created for it."""
    from defslam_amd import _lib, sft, synth
    ctx = request.getfixturevalue("lab_ctx" if lab else "gpu_ctx")
    cus = _lib.device_cus(0)
    regs = (synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    mesh = synth.make_grid_template(9, 14)
    c2 = synth.make_grid_template(*synth.CONFIGS["C2"][:2])

    def ragged(B):   # the frames of test_launch_shapes_between_latency_mode_and_rounds
        syn = []
        for p in range(B):
            fr = synth.make_frame(mesh, 380 + 10 * (p % 5), p)
            if p % 4 == 2:   # a partial view: another active set, another dimension in the same batch
                keep = [c + 14 * r for r in range(9) for c in range(13)]
                sel = np.all(np.isin(fr.obs_nodes, keep), axis=1)
                for k in ["obs_nodes", "obs_bary", "obs_uv", "obs_invsig2"]:
                    setattr(fr, k, getattr(fr, k)[sel])
            syn.append(fr)
        return syn

    syn_all = ragged(2 * cus)
    # (template, synthetic frames, wavefronts per problem reported, lanes, (tile mode, cut) of problem 0)
    steps = [(mesh, syn_all[:cus // 2 + 1], 1, 1, (1, 0)), (mesh, syn_all[:1], 8, 4, (1, 0)), (mesh, syn_all[:cus // 4 + 1], 8, 3, (1, 0)),
             (mesh, syn_all, 1, 1, (1, 0)), (c2, [synth.make_frame(c2, synth.CONFIGS["C2"][2], 7)], 8, 4, (2, 1)), (mesh, syn_all[:cus // 2 + 1], 1, 1, (1, 0))]

    def solve(c, tmpl, syn, waves, lanes, solver):
        B = len(syn)
        assert lanes == (1 if waves == 1 else 4 if 4 * B <= cus else 3 if 3 * B <= cus else 2 if 2 * B <= cus else 1)   # DESIGN 4.0, this device
        c.template_build(tmpl.xyz0, tmpl.facets)
        frames = [sft.frame_from_synth(fr) for fr in syn]
        c.batch_upload(frames, *regs, 1, 50)
        assert int(c.problem_info(0)[1][7]) == waves
        if lab:
            info = c.solver_info(0)
            assert (info["lanes"], info["tile_mode"], info["split"]) == (lanes,) + solver
        c.batch_run()
        return c.batch_download(), frames

    for step, (tmpl, syn, waves, lanes, solver) in enumerate(steps):
        inl, frames = solve(ctx, tmpl, syn, waves, lanes, solver)
        fresh = sft.Context(0, lab=lab)
        try:
            inl_f, frames_f = solve(fresh, tmpl, syn, waves, lanes, solver)
        finally:
            fresh.close()
        assert list(inl) == list(inl_f), step
        for p, (a, b) in enumerate(zip(frames, frames_f)):
            assert (a.iters, a.trials, a.status) == (b.iters, b.trials, b.status), (step, p)
            for k in ("nodes_xyz", "pose7", "chi2_obs", "mvbOutlier", "trace"):
                np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=f"step {step}, problem {p}, {k}")


@pytest.fixture(params=[0, -1], ids=["rounds_to_the_end", "product_default_tail"])
def rounds_ctx(request, lab_ctx):
    """Both ways the throughput shape ends a step.  tail = 0: the rounds of phase kernels run to the END of every problem (the one-wavefront
    solver of the rounds on small, ragged, failing and budgeted problems).  tail = -1: the PRODUCT default -- the last problems of a step, from
    the automatic threshold downwards (on a 256-CU device ALL of a 512-problem batch), go to sftb_tail_kernel: the same edge cases through the
    eight-wavefront solver, the tail kernel's own linearisation / trial loop and its budget and failure exits."""
    lab_ctx.set_option("tail", request.param)
    yield lab_ctx
    lab_ctx.set_option("tail", -1)


def test_tail_kernel_finishes_what_the_rounds_leave_like_the_rounds_would(lab_ctx, oracle_mod):
    """sftb_tail_kernel: once at most two problems per CU are still running, each of them gets a workgroup that runs it to its end from the
    controller record the rounds left (linearisations and trials: the code of LIN / TRIAL; factorisation: the eight-wavefront register-window
    solver).  A ragged batch of 1100 problems (every third sees part of the template; the rounds run until 512 are left) with the tail kernel and
    with rounds to the end: identical LM trajectories, outliers and inlier counts, vertices to 1e-9 relative; sampled ids against the oracle;
    two runs with the tail kernel bit-identical (where the rounds end is decided on the device, not by the host's launch groups)."""
    from defslam_amd import sft, synth
    B = 1100
    tmpl = synth.make_grid_template(9, 14)
    lab_ctx.template_build(tmpl.xyz0, tmpl.facets)
    regs = (synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    syn = []
    for p in range(B):
        fr = synth.make_frame(tmpl, 420, p)
        if p % 3 == 1:   # a partial view: no observation on the last column(s) of the template
            keep = [c + 14 * r for r in range(9) for c in range(14 - 1 - (p % 2))]
            sel = np.all(np.isin(fr.obs_nodes, keep), axis=1)
            for k in ["obs_nodes", "obs_bary", "obs_uv", "obs_invsig2"]:
                setattr(fr, k, getattr(fr, k)[sel])
        syn.append(fr)
    runs = {}
    for key, tail in (("rounds", 0), ("tail", 2), ("tail2", 2)):
        lab_ctx.set_option("tail", tail)
        frames = [sft.frame_from_synth(fr) for fr in syn]
        lab_ctx.batch_upload(frames, *regs, 1, 50)
        _, counts = lab_ctx.problem_info(0)
        assert int(counts[7]) == 1
        lab_ctx.batch_run()
        inl = lab_ctx.batch_download()
        runs[key] = (frames, [int(i) for i in inl])
        if tail:
            ph, nr = lab_ctx.rounds_timed()
            assert ph["tail"] > 0.0 and nr >= 1, (ph, nr)            # both parts of the step ran
    lab_ctx.set_option("tail", -1)
    fr_r, in_r = runs["rounds"]
    fr_t, in_t = runs["tail"]
    fr_u, in_u = runs["tail2"]
    assert in_r == in_t == in_u
    for a, b, c in zip(fr_r, fr_t, fr_u):
        assert (a.iters, a.trials) == (b.iters, b.trials)
        np.testing.assert_array_equal(a.trace[:a.iters, [2, 6]], b.trace[:b.iters, [2, 6]])
        np.testing.assert_array_equal(a.mvbOutlier, b.mvbOutlier)
        assert np.abs(a.nodes_xyz - b.nodes_xyz).max() <= 1e-9 * np.abs(a.nodes_xyz).max()
        np.testing.assert_array_equal(b.nodes_xyz, c.nodes_xyz)
        np.testing.assert_array_equal(b.pose7, c.pose7)
    tc = oracle_mod.template_build(tmpl.xyz0, tmpl.facets)
    for p in (0, 1, 2, 511, 512, 700, 1099):
        fr = syn[p]
        r = oracle_mod.sft_solve(tc, fr.Tcw, fr.K, fr.n_frame, fr.obs_nodes, fr.obs_bary, fr.obs_uv, fr.obs_invsig2, fr.xyz, *regs, ldlt_mode=1)
        _compare(fr_t[p], in_t[p], r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret)


@pytest.mark.parametrize("shape,m", [((3, 3), 60), ((5, 6), 200), ((7, 7), 300), ((10, 10), 300), ((9, 14), 420)])
def test_rounds_of_phase_kernels_on_small_and_ragged_problems(rounds_ctx, oracle_mod, shape, m):
    """The throughput shape (LIN / FACTOR / TRIAL rounds, one wavefront per factorisation) away from the benched size: block-row counts
    below, at and just above the 8-tile window (2, 6, 10, 19, 24 block rows), active blocks that are not a multiple of the tile size, and
    -- every third problem sees only part of the template -- different dimensions inside one batch.  512 problems per batch (the smallest
    batch that takes this shape on a 256-CU device), 56 of them against the oracle."""
    from defslam_amd import sft, synth
    B = 512
    rows, cols = shape
    tmpl = synth.make_grid_template(rows, cols)
    rounds_ctx.template_build(tmpl.xyz0, tmpl.facets)
    regs = (synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    syn = []
    for p in range(B):
        fr = synth.make_frame(tmpl, m, p)
        if p % 3 == 1 and cols > 3:
            keep = [c + cols * r for r in range(rows) for c in range(cols - 1 - (p % 2))]
            sel = np.all(np.isin(fr.obs_nodes, keep), axis=1)
            for k in ["obs_nodes", "obs_bary", "obs_uv", "obs_invsig2"]:
                setattr(fr, k, getattr(fr, k)[sel])
        syn.append(fr)
    frames = [sft.frame_from_synth(fr) for fr in syn]
    rounds_ctx.batch_upload(frames, *regs, 1, 50)
    _, counts = rounds_ctx.problem_info(0)
    assert int(counts[7]) == 1, "512 narrow-band problems must run as rounds of phase kernels"
    rounds_ctx.batch_run()
    inl = rounds_ctx.batch_download()
    tc = oracle_mod.template_build(tmpl.xyz0, tmpl.facets)
    dims = set()
    relaxed = []
    for p in list(range(0, 48)) + [255, 256, 257, 300, 301, 509, 510, 511]:
        fr = syn[p]
        r = oracle_mod.sft_solve(tc, fr.Tcw, fr.K, fr.n_frame, fr.obs_nodes, fr.obs_bary, fr.obs_uv, fr.obs_invsig2, fr.xyz, *regs, ldlt_mode=1)
        f = frames[p]
        # Terminal stagnation: once an iteration needs >= 8 dampings in a row (lambda grown by > 2^28 within it) the trial steps are below
        # one ulp of the state, the gain ratio is rounding noise and accept / reject -- and with it "ten rejections: stop" against "one more
        # iteration" -- is a coin toss.  Measured on the 512 3x3 problems (tools/diag/rounds_small_mesh.py): 29 differ from the oracle there
        # and nowhere else, the eight-wavefront latency kernel differs from the oracle just as often (on other problems), the one-wavefront
        # and four-wavefront solutions of the same system agree to 1.4e-11 (damping 1e-5) ... 2e-16 (damping 1e18), final states to 1.2e-12.
        # So: strict up to the first such iteration of either side; the final state, outliers and inliers always.
        heavy = [int(np.argmax(t[:, 2] >= 8)) if (t[:, 2] >= 8).any() else len(t) for t in (r.trace, f.trace)]
        k = min(heavy)
        if k >= len(r.trace) and k >= len(f.trace):
            _compare(f, int(inl[p]), r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret)
        else:
            relaxed.append(p)
            assert f.status == 0 and abs(f.iters - r.trace.shape[0]) <= 1 and f.iters > k
            np.testing.assert_array_equal(f.trace[:k, [2, 6]], r.trace[:k, [2, 6]])
            np.testing.assert_allclose(f.trace[:k, [0, 1, 3, 4]], r.trace[:k, [0, 1, 3, 4]], rtol=1e-8)
            np.testing.assert_allclose(f.trace[k, [0, 1]], r.trace[k, [0, 1]], rtol=1e-8)   # chi2 and damping at the start of that iteration
            assert np.abs(f.nodes_xyz - r.xyz).max() <= VERT_TOL * np.abs(r.xyz).max() and np.abs(f.pose7 - r.pose7).max() <= POSE_TOL
            np.testing.assert_array_equal(f.mvbOutlier, np.asarray(r.outlier, bool))
            assert int(inl[p]) == r.ret and f.rep_error_f64 == pytest.approx(r.rep_error, rel=1e-9)
        assert f.dim == r.dims[0]
        dims.add(f.dim)
    if cols > 3:
        assert len(dims) >= 2
        assert not relaxed, relaxed          # only the 3x3 mesh (27 unknowns, 60 matches) runs into the stagnation phase
    else:
        assert len(relaxed) <= 12, relaxed


def test_rounds_of_phase_kernels_when_the_camera_records_do_not_fit_lds(rounds_ctx, oracle_mod):
    """The benched template with four times the observations (4000 matches): the camera records of placement class 3 (five doubles per
    observation) no longer fit the LDS budget of the LIN kernel next to the other record classes, the upload falls back to class 2 (128-byte
    records in the workspace) -- same throughput shape, same results."""
    from defslam_amd import sft, synth
    B = 512
    rows, cols, _ = synth.CONFIGS["C2"]
    tmpl = synth.make_grid_template(rows, cols)
    rounds_ctx.template_build(tmpl.xyz0, tmpl.facets)
    regs = (synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    syn = [synth.make_frame(tmpl, 4000, p) for p in range(B)]
    frames = [sft.frame_from_synth(fr) for fr in syn]
    rounds_ctx.batch_upload(frames, *regs, 1, 50)
    assert int(rounds_ctx.problem_info(0)[1][7]) == 1
    rounds_ctx.batch_run()
    inl = rounds_ctx.batch_download()
    tc = oracle_mod.template_build(tmpl.xyz0, tmpl.facets)
    for p in (0, 255, 511):
        fr = syn[p]
        r = oracle_mod.sft_solve(tc, fr.Tcw, fr.K, fr.n_frame, fr.obs_nodes, fr.obs_bary, fr.obs_uv, fr.obs_invsig2, fr.xyz, *regs, ldlt_mode=1)
        _compare(frames[p], int(inl[p]), r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret)


def test_rounds_of_phase_kernels_with_failing_factorisations(rounds_ctx, oracle_mod):
    """Problems whose normal equations are not positive definite (observations with NEGATIVE information: H = sum w J^T J is indefinite) among
    healthy ones in one batch of the throughput shape: the one-wavefront Cholesky reports the non-positive pivot, the trial counts as failed
    (g2o: `_solver->solve` returns false, the step is rejected, optimization_algorithm_levenberg.cpp:103-113), the state is restored, status
    bit 0 is set -- and the neighbours of such a problem in the batch index are solved as if it were not there.  (With 512 problems every FACTOR
    wave of a 256-CU device gets one problem per launch, and which wave pulls which problem is decided at run time: the sequences inside one
    wave -- a failed problem behind and in front of healthy ones -- are test_factor_waves_gpu.py's.)"""
    from defslam_amd import sft, synth
    B = 512
    tmpl = synth.make_grid_template(10, 10)
    rounds_ctx.template_build(tmpl.xyz0, tmpl.facets)
    regs = (synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    syn = [synth.make_frame(tmpl, 300, p) for p in range(B)]
    poisoned = (3, 77, 300, 511)
    for p in poisoned:
        syn[p].obs_invsig2 = -50.0 * np.abs(syn[p].obs_invsig2)
    frames = [sft.frame_from_synth(fr) for fr in syn]
    rounds_ctx.batch_upload(frames, *regs, 1, 50)
    assert int(rounds_ctx.problem_info(0)[1][7]) == 1
    rounds_ctx.batch_run()
    inl = rounds_ctx.batch_download()
    tc = oracle_mod.template_build(tmpl.xyz0, tmpl.facets)
    for p in list(poisoned) + [2, 4, 76, 78, 299, 301, 510, 0, 1]:
        fr = syn[p]
        r = oracle_mod.sft_solve(tc, fr.Tcw, fr.K, fr.n_frame, fr.obs_nodes, fr.obs_bary, fr.obs_uv, fr.obs_invsig2, fr.xyz, *regs, ldlt_mode=1)
        f = frames[p]
        if p in poisoned:
            # An indefinite problem has no trajectory to compare: whether H + lambda I passes the Cholesky at a given damping hangs on the last
            # bits of a pivot, and from the first such difference on the two runs are different problems.  What is defined: the first
            # linearisation (chi2, the damping it starts from), that its first factorisation fails in both, that the failure is reported, and
            # that the solve terminates with finite numbers.
            assert f.status & 1, "a failed factorisation must be reported"
            assert 1 <= f.iters <= 50 and f.trials >= f.iters
            np.testing.assert_allclose(f.trace[0, [0, 1]], r.trace[0, [0, 1]], rtol=1e-8)
            assert f.trace[0, 7] == 0 and r.trace[0, 7] == 0
            assert np.isfinite(f.nodes_xyz).all() and np.isfinite(f.pose7).all()
        else:
            _compare(f, int(inl[p]), r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret)


@pytest.mark.parametrize("max_iters", [0, 1, 3])
def test_rounds_of_phase_kernels_with_an_iteration_budget(rounds_ctx, oracle_mod, max_iters):
    """The throughput shape when the caller's iteration budget ends the solve: 0 (classification of the initial state only -- the batch never
    enters a LIN / FACTOR round), 1 and 3 iterations (problems stop on the budget in different rounds, each with its own number of rejected
    dampings).  512 problems on the 10 x 10 mesh, 24 of them against the oracle with the same budget."""
    from defslam_amd import sft, synth
    B = 512
    tmpl = synth.make_grid_template(10, 10)
    rounds_ctx.template_build(tmpl.xyz0, tmpl.facets)
    regs = (synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    syn = [synth.make_frame(tmpl, 300, p) for p in range(B)]
    frames = [sft.frame_from_synth(fr) for fr in syn]
    rounds_ctx.batch_upload(frames, *regs, 1, max_iters)
    _, counts = rounds_ctx.problem_info(0)
    assert int(counts[7]) == 1
    rounds_ctx.batch_run()
    inl = rounds_ctx.batch_download()
    tc = oracle_mod.template_build(tmpl.xyz0, tmpl.facets)
    zero_it = []
    for p in list(range(16)) + [255, 256, 257, 509, 510, 511, 300, 301]:
        fr = syn[p]
        r = oracle_mod.sft_solve(tc, fr.Tcw, fr.K, fr.n_frame, fr.obs_nodes, fr.obs_bary, fr.obs_uv, fr.obs_invsig2, fr.xyz, *regs, max_iters=max_iters, ldlt_mode=1)
        f = frames[p]
        assert f.iters == r.trace.shape[0] <= max_iters
        if max_iters == 0:
            # Outside the reference's behaviour (it always runs optimize(50)): no edge error is ever computed, the oracle's edges hold zeros,
            # every observation is an inlier; the same in every launch shape (the one-problem latency path below).
            assert f.status == 0 and f.trials == 0
            np.testing.assert_array_equal(f.nodes_xyz, fr.xyz)            # nothing moved
            np.testing.assert_array_equal(f.mvbOutlier, np.asarray(r.outlier, bool))
            assert not f.mvbOutlier.any() and int(inl[p]) == r.ret == fr.obs_nodes.shape[0]
            assert f.rep_error_f64 == pytest.approx(r.rep_error, rel=1e-9)
            zero_it.append((p, f.mvbOutlier.copy(), f.chi2_obs.copy(), f.rep_error_f64, int(inl[p])))
        else:
            _compare(f, int(inl[p]), r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret)
            assert f.trials == r.trials
    for p, outl, chi2, rep, n_in in zero_it[:4]:
        fr = syn[p]
        f1, i1 = _solve_gpu(rounds_ctx, tmpl.xyz0, tmpl.facets, dict(Tcw=fr.Tcw, K=fr.K, n_frame=fr.n_frame, obs_nodes=fr.obs_nodes, obs_bary=fr.obs_bary,
                                                                  obs_uv=fr.obs_uv, obs_invsig2=fr.obs_invsig2, xyz=fr.xyz), regs, 1, 0)
        np.testing.assert_array_equal(f1.mvbOutlier, outl)
        np.testing.assert_array_equal(f1.chi2_obs, chi2)
        assert (f1.rep_error_f64, i1, f1.iters, f1.trials) == (rep, n_in, 0, 0)


@pytest.mark.parametrize("cfg,pid", [("smoke", 0), ("smoke", 7), ("C2", 0), ("W12", 1), ("W16", 2), ("B272", 3)])
def test_hip_matches_oracle_seeded(gpu_ctx, oracle_mod, cfg, pid):
    from defslam_amd import synth
    tmpl, fr = synth.make_problem(cfg, pid)
    tc, args = oracle_args(oracle_mod, tmpl, fr)
    r = oracle_mod.sft_solve(*args, ldlt_mode=1)
    f, inl = _solve_gpu(gpu_ctx, tmpl.xyz0, tmpl.facets, dict(Tcw=fr.Tcw, K=fr.K, n_frame=fr.n_frame, obs_nodes=fr.obs_nodes, obs_bary=fr.obs_bary,
                                                              obs_uv=fr.obs_uv, obs_invsig2=fr.obs_invsig2, xyz=fr.xyz),
                    (synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP))
    _compare(f, inl, r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret)
    # float32 boundaries: pose matrix and map points
    np.testing.assert_allclose(f.Tcw, r.Tcw, atol=2e-7)
    assert f.dim == r.dims[0]


@pytest.mark.parametrize("shape,m,pid", [((10, 10), 300, 1), ((25, 20), 1000, 2), ((6, 17), 120, 3), ((8, 30), 400, 4), ((6, 41), 400, 5)])
def test_normal_equations_match_oracle(lab_ctx, oracle_mod, shape, m, pid):
    """Residuals + Jacobians + H/b assembly in isolation, through the lab hook dsh_lab_sft_system."""
    gpu_ctx = lab_ctx
    from defslam_amd import sft, synth
    tmpl = synth.make_grid_template(*shape)
    fr = synth.make_frame(tmpl, m, pid)
    rng = np.random.default_rng(pid)
    fr.xyz = fr.xyz + rng.normal(scale=0.002, size=fr.xyz.shape)   # non-trivial curvature / stretch residuals
    tc, args = oracle_args(oracle_mod, tmpl, fr)
    Ho, bo, chio = oracle_mod.sft_system(*args)
    gpu_ctx.template_build(tmpl.xyz0, tmpl.facets)
    gpu_ctx.batch_upload([sft.frame_from_synth(fr)], synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    Hg, bg, chig = gpu_ctx.debug_system(0, Ho.shape[0])
    assert chig == pytest.approx(chio, rel=1e-12)
    np.testing.assert_allclose(Hg, Ho, rtol=1e-9, atol=1e-11 * np.abs(Ho).max())
    np.testing.assert_allclose(bg, bo, rtol=1e-9, atol=1e-11 * np.abs(bo).max())
    # structure: identical sparsity pattern (bit-exact indexing of which node pairs interact)
    np.testing.assert_array_equal(np.abs(Hg) > 0, np.abs(Ho) > 0)


def test_partial_view_keeps_unseen_nodes_fixed(gpu_ctx, oracle_mod):
    from defslam_amd import synth
    tmpl = synth.make_grid_template(12, 12)
    fr = synth.make_frame(tmpl, 800, 9)
    keep = [c + 12 * r for r in range(6) for c in range(6)]
    sel = np.all(np.isin(fr.obs_nodes, keep), axis=1)
    for k in ["obs_nodes", "obs_bary", "obs_uv", "obs_invsig2"]:
        setattr(fr, k, getattr(fr, k)[sel])
    tc, args = oracle_args(oracle_mod, tmpl, fr)
    r = oracle_mod.sft_solve(*args)
    f, inl = _solve_gpu(gpu_ctx, tmpl.xyz0, tmpl.facets, dict(Tcw=fr.Tcw, K=fr.K, n_frame=fr.n_frame, obs_nodes=fr.obs_nodes, obs_bary=fr.obs_bary,
                                                              obs_uv=fr.obs_uv, obs_invsig2=fr.obs_invsig2, xyz=fr.xyz),
                    (synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP))
    _compare(f, inl, r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret)
    moved = np.abs(f.nodes_xyz - fr.xyz).max(axis=1) > 0
    assert f.dim == r.dims[0] < 6 + 3 * tmpl.n
    far = [c + 12 * r_ for r_ in range(8, 12) for c in range(8, 12)]
    assert not moved[far].any()                      # fixed vertices are returned bit-identical


@pytest.mark.parametrize("shape,cols_kept", [((6, 41), 30), ((8, 30), 24)])
def test_partial_view_on_a_wide_band_template(gpu_ctx, oracle_mod, shape, cols_kept):
    """The wide tile solver (half-bandwidth > 128) with a partially observed template: fewer active nodes than the template has,
    an active block whose size is not a multiple of the tile size, tile rows near the end of the matrix with short bands."""
    from defslam_amd import synth
    rows, cols = shape
    tmpl = synth.make_grid_template(rows, cols)
    fr = synth.make_frame(tmpl, 700, 11)
    keep = [c + cols * r for r in range(rows) for c in range(cols_kept)]
    sel = np.all(np.isin(fr.obs_nodes, keep), axis=1)
    for k in ["obs_nodes", "obs_bary", "obs_uv", "obs_invsig2"]:
        setattr(fr, k, getattr(fr, k)[sel])
    tc, args = oracle_args(oracle_mod, tmpl, fr)
    r = oracle_mod.sft_solve(*args, ldlt_mode=1)
    f, inl = _solve_gpu(gpu_ctx, tmpl.xyz0, tmpl.facets, dict(Tcw=fr.Tcw, K=fr.K, n_frame=fr.n_frame, obs_nodes=fr.obs_nodes, obs_bary=fr.obs_bary,
                                                              obs_uv=fr.obs_uv, obs_invsig2=fr.obs_invsig2, xyz=fr.xyz),
                    (synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP))
    assert f.half_bandwidth > 128 and f.dim == r.dims[0] < 6 + 3 * tmpl.n
    _compare(f, inl, r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret)


def test_warm_started_sequence(gpu_ctx, oracle_mod):
    """Frame-to-frame tracking: every frame starts from the previous result (float32 pose round trip)."""
    from defslam_amd import sft, synth
    tmpl = synth.make_grid_template(10, 10)
    tc = oracle_mod.template_build(tmpl.xyz0, tmpl.facets)
    gpu_ctx.template_build(tmpl.xyz0, tmpl.facets)
    Tg, xg = np.eye(4, dtype=np.float32), tmpl.xyz0.copy()
    To, xo = Tg.copy(), xg.copy()
    for k in range(4):
        fr = synth.make_frame(tmpl, 300, 20 + k, phase=0.2 * k, init_xyz=xg, init_Tcw=Tg)
        f = sft.frame_from_synth(fr)
        sft.DefPoseOptimization(gpu_ctx, f, synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
        r = oracle_mod.sft_solve(tc, To, fr.K, fr.n_frame, fr.obs_nodes, fr.obs_bary, fr.obs_uv, fr.obs_invsig2, xo,
                                 synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
        assert f.iters == r.iters
        assert np.abs(f.nodes_xyz - r.xyz).max() < 1e-7
        np.testing.assert_allclose(f.Tcw, r.Tcw, atol=2e-7)
        Tg, xg, To, xo = f.Tcw, f.nodes_xyz, r.Tcw, r.xyz


def test_seq100_tracking_sequence_against_the_oracle_every_10th_frame(gpu_ctx, oracle_mod):
    """SEQ100 (the runnable substitute of the Mandala sequences, BASELINE configs[2]): 100 frames of the C2 workload
    (500-node template, 1000 matches per frame) with temporally smooth deformation and camera motion, every frame tracked from
    the previous result through the one-shot call dsh_sft_solve (float32 pose round trip, DefTracking.cc:350).  Every 10th
    frame the oracle solves the same frame from the same previous state: same LM trajectory, vertices, pose, outliers."""
    from defslam_amd import sft, synth
    rows, cols, m = synth.CONFIGS[synth.SEQ100["config"]]
    n_frames = synth.SEQ100["n_frames"]
    tmpl = synth.make_grid_template(rows, cols)
    tc = oracle_mod.template_build(tmpl.xyz0, tmpl.facets)
    gpu_ctx.template_build(tmpl.xyz0, tmpl.facets)
    regs = (synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    T, x = np.eye(4, dtype=np.float32), tmpl.xyz0.copy()
    checked = 0
    total_iters = 0
    for k in range(n_frames):
        fr = synth.make_sequence_frame(tmpl, m, k, n_frames, synth.SEQ100["seq_id"], init_xyz=x, init_Tcw=T)
        f = sft.frame_from_synth(fr)
        call = gpu_ctx.prepare_solve(f, *regs, 1, 50)
        inl = call()
        assert f.status == 0 and f.iters >= 1
        total_iters += f.iters
        if k % 10 == 0 or k == n_frames - 1:
            r = oracle_mod.sft_solve(tc, T, fr.K, fr.n_frame, fr.obs_nodes, fr.obs_bary, fr.obs_uv, fr.obs_invsig2, x, *regs, ldlt_mode=1)
            _compare(f, inl, r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret)
            np.testing.assert_allclose(f.Tcw, r.Tcw, atol=2e-7)
            checked += 1
        assert inl > 0.85 * m                       # tracking holds: the 5 % synthetic outliers and little else are rejected
        T, x = f.Tcw.copy(), f.nodes_xyz.copy()
    assert checked == 11
    # warm starts converge in fewer iterations than the cold first frame of the workload (about 10)
    assert total_iters / n_frames < 10


@pytest.mark.parametrize("shape", [(10, 10), (6, 41)], ids=["narrow", "wide-band"])
def test_batch_equals_single_and_is_reproducible(gpu_ctx, shape):
    """Independent problems in one launch give bit-identical results to one-at-a-time solves, run after run (register-window
    tile solver and, for the 6x41 template with half-bandwidth 248, the left-looking wide tile solver; mixed match counts)."""
    from defslam_amd import sft, synth
    tmpl = synth.make_grid_template(*shape)
    gpu_ctx.template_build(tmpl.xyz0, tmpl.facets)
    frames = [sft.frame_from_synth(synth.make_frame(tmpl, 200 + 10 * p, p)) for p in range(9)]
    inl = sft.DefPoseOptimizationBatch(gpu_ctx, frames, synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    xyz_a = [f.nodes_xyz.copy() for f in frames]
    gpu_ctx.batch_run()
    inl2 = gpu_ctx.batch_download()
    assert inl == inl2
    for f, xa in zip(frames, xyz_a):
        np.testing.assert_array_equal(f.nodes_xyz, xa)
    for p in [0, 4, 8]:
        f1 = sft.frame_from_synth(synth.make_frame(tmpl, 200 + 10 * p, p))
        i1 = sft.DefPoseOptimization(gpu_ctx, f1, synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
        assert i1 == inl[p]
        np.testing.assert_array_equal(f1.nodes_xyz, xyz_a[p])
        np.testing.assert_array_equal(f1.pose7, frames[p].pose7)


def test_one_batch_may_mix_solvers(gpu_ctx):
    """Problems of one batch choose their solver by their own half-bandwidth: a partially observed frame of the 8x30 template falls
    below 128 (register-window tiles), a fuller view stays above (wide tiles).  Both in one launch = each alone, bit for bit."""
    from defslam_amd import sft, synth
    tmpl = synth.make_grid_template(8, 30)
    gpu_ctx.template_build(tmpl.xyz0, tmpl.facets)

    def frame(cols_kept, pid):
        fr = synth.make_frame(tmpl, 700, pid)
        keep = [c + 30 * r for r in range(8) for c in range(cols_kept)]
        sel = np.all(np.isin(fr.obs_nodes, keep), axis=1)
        for k in ["obs_nodes", "obs_bary", "obs_uv", "obs_invsig2"]:
            setattr(fr, k, getattr(fr, k)[sel])
        return sft.frame_from_synth(fr)

    batch = [frame(17, 1), frame(24, 2), frame(30, 3), frame(12, 4)]
    sft.DefPoseOptimizationBatch(gpu_ctx, batch, synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    kinds = [f.half_bandwidth > 128 for f in batch]
    assert any(kinds) and not all(kinds)
    for f, (cols_kept, pid) in zip(batch, [(17, 1), (24, 2), (30, 3), (12, 4)]):
        one = frame(cols_kept, pid)
        sft.DefPoseOptimization(gpu_ctx, one, synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
        assert (one.iters, one.trials, one.half_bandwidth) == (f.iters, f.trials, f.half_bandwidth)
        np.testing.assert_array_equal(one.nodes_xyz, f.nodes_xyz)
        np.testing.assert_array_equal(one.pose7, f.pose7)


@pytest.mark.parametrize("cfg,pid", [("smoke", 3), ("C2", 5)])
def test_four_wavefront_launch_shape_matches_eight(lab_ctx, oracle_mod, cfg, pid):
    """The throughput launch shape (4 wavefronts per problem, two ring rows per wave, chosen by the library once a batch
    holds >= 2 problems per CU) and the barrier version of the 8-wavefront shape run the same factorisation as the default
    (8 wavefronts, barrier-free dataflow steps): same LM trajectory as the oracle, vertices equal to rounding."""
    from defslam_amd import sft, synth
    gpu_ctx = lab_ctx
    tmpl, fr = synth.make_problem(cfg, pid)
    gpu_ctx.template_build(tmpl.xyz0, tmpl.facets)
    out = {}
    try:
        for nw, df in (("8", "1"), ("4", "1"), ("8", "0")):
            gpu_ctx.set_option("waves", int(nw))      # applied by the next dsh_sft_batch_upload
            gpu_ctx.set_option("dataflow", int(df))   # barrier-free steps (default) or the barrier version (lab build only)
            f = sft.frame_from_synth(fr)
            inl = sft.DefPoseOptimization(gpu_ctx, f, synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
            out[nw + df] = (f, inl)
    finally:
        gpu_ctx.set_option("waves", 0)
        gpu_ctx.set_option("dataflow", 1)
    f8, i8 = out["81"]
    f4, i4 = out["41"]
    fb, ib = out["80"]
    assert ib == i8 and fb.iters == f8.iters and fb.trials == f8.trials
    assert np.abs(fb.nodes_xyz - f8.nodes_xyz).max() < 1e-10 * np.abs(f8.nodes_xyz).max()
    assert i4 == i8 and f4.iters == f8.iters and f4.trials == f8.trials
    np.testing.assert_array_equal(f4.mvbOutlier, f8.mvbOutlier)
    assert np.abs(f4.nodes_xyz - f8.nodes_xyz).max() < 1e-10 * np.abs(f8.nodes_xyz).max()
    np.testing.assert_allclose(f4.trace, f8.trace, rtol=1e-8, atol=1e-12)
    tc, args = oracle_args(oracle_mod, tmpl, fr)
    r = oracle_mod.sft_solve(*args, ldlt_mode=1)
    assert f4.iters == r.iters
    assert np.abs(f4.nodes_xyz - r.xyz).max() < 1e-9 * np.abs(r.xyz).max()


@pytest.mark.parametrize("waves", ["8", "4"])
def test_dataflow_steps_equal_barrier_steps_bit_for_bit_under_load(lab_ctx, waves):
    """The barrier-free factor steps hand tiles over through LDS flags; a missed dependency shows up as a (rare, load
    dependent) difference.  Many more problems than CUs, both launch shapes, compared bit for bit with the barrier
    version (same arithmetic order).  Regression test for the per-parity X flags (a wave one step ahead must not
    satisfy a reader of the previous step)."""
    from defslam_amd import sft, synth
    gpu_ctx = lab_ctx
    tmpl = synth.make_grid_template(12, 14)
    gpu_ctx.template_build(tmpl.xyz0, tmpl.facets)
    B = 900
    gpu_ctx.set_option("waves", int(waves))

    def run(df):
        gpu_ctx.set_option("dataflow", int(df))
        frames = [sft.frame_from_synth(synth.make_frame(tmpl, 260 + (p % 7) * 20, p)) for p in range(B)]
        inl = sft.DefPoseOptimizationBatch(gpu_ctx, frames, synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
        return np.stack([f.nodes_xyz for f in frames]), np.array([f.trials for f in frames]), np.array(inl)

    try:
        ref = run("0")
        for _ in range(2):
            cur = run("1")
            np.testing.assert_array_equal(cur[1], ref[1])
            np.testing.assert_array_equal(cur[2], ref[2])
            np.testing.assert_array_equal(cur[0], ref[0])
    finally:
        gpu_ctx.set_option("waves", 0)
        gpu_ctx.set_option("dataflow", 1)


def test_mappoint_writeback_float32(gpu_ctx):
    from defslam_amd import sft, synth
    tmpl, fr = synth.make_problem("smoke", 2)
    gpu_ctx.template_build(tmpl.xyz0, tmpl.facets)
    f = sft.frame_from_synth(fr)
    sft.DefPoseOptimization(gpu_ctx, f, synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    exp = (fr.obs_bary[:, :, None] * f.nodes_xyz[fr.obs_nodes]).sum(1)
    np.testing.assert_allclose(f.mappoints, exp.astype(np.float32), atol=1e-7)


@pytest.mark.parametrize("cfg", ["C2", "C5"])
def test_full_size_properties(gpu_ctx, cfg):
    """BASELINE.json sizes (C2: 500 nodes x 1000 matches, C5: 2000 x 4000): properties that need no oracle run.
    (1) every accepted step lowers the robust cost and the controller never reports a failed factorisation,
    (2) rigid-motion equivariance: moving template + camera by the same rigid transform leaves image-space
        quantities (chi2 trace, reprojection error, outliers) unchanged and moves the vertices rigidly."""
    from scipy.spatial.transform import Rotation
    from defslam_amd import sft, synth
    tmpl, fr = synth.make_problem(cfg, 1)
    gpu_ctx.template_build(tmpl.xyz0, tmpl.facets)
    f = sft.frame_from_synth(fr)
    inl = sft.DefPoseOptimization(gpu_ctx, f, synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    assert f.status == 0 and f.iters >= 3
    acc = f.trace[:, 6] == 1
    assert (f.trace[acc, 3] < f.trace[acc, 0]).all()
    assert (np.diff(f.trace[:, 0]) <= 1e-9 * f.trace[0, 0]).all()
    assert 0.8 * fr.obs_nodes.shape[0] < inl <= fr.obs_nodes.shape[0]
    # rigid transform G: x' = Rg x + tg ; camera Tcw' = Tcw * G^-1
    Rg = Rotation.from_rotvec([0.2, -0.1, 0.3]).as_matrix()
    tg = np.array([0.3, -0.2, 0.5])
    xyz0p = tmpl.xyz0 @ Rg.T + tg
    G = np.eye(4)
    G[:3, :3], G[:3, 3] = Rg, tg
    Tp = (fr.Tcw.astype(float) @ np.linalg.inv(G))
    gpu_ctx.template_build(xyz0p, tmpl.facets)
    f2 = sft.frame_from_synth(fr)
    f2.nodes_xyz = xyz0p.copy()
    f2.Tcw = Tp.astype(np.float32)
    inl2 = sft.DefPoseOptimization(gpu_ctx, f2, synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    # the float32 pose boundary perturbs the start by ~1e-7, so compare to 1e-4 (the north-star tolerance)
    assert f2.iters == f.iters
    np.testing.assert_allclose(f2.trace[:, 0], f.trace[:, 0], rtol=1e-4)
    assert inl2 == inl
    back = (f2.nodes_xyz - tg) @ Rg
    assert np.abs(back - f.nodes_xyz).max() < 1e-4 * np.abs(f.nodes_xyz).max()


@pytest.mark.parametrize("cfg,pid", [("W16", 3), ("W12", 4)])
def test_wide_tile_solver_agrees_with_the_band_solver(lab_ctx, cfg, pid):
    """Half-bandwidths 128 < kd <= 256 run the left-looking MFMA tile factorisation (sft_wide.h); the lab option "wide_off" selects the
    row-major band solver for the same problem.  Both are Cholesky factorisations of the same matrix in different summation
    orders: identical Levenberg-Marquardt trajectories, vertices to 1e-9."""
    from defslam_amd import sft, synth
    gpu_ctx = lab_ctx
    tmpl, fr = synth.make_problem(cfg, pid)
    gpu_ctx.template_build(tmpl.xyz0, tmpl.facets)
    fw = sft.frame_from_synth(fr)
    inl_w = sft.DefPoseOptimization(gpu_ctx, fw, synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    _, counts = gpu_ctx.problem_info(0)
    assert 128 < counts[6] <= 256
    gpu_ctx.set_option("wide_off", 1)
    try:
        fb = sft.frame_from_synth(fr)
        inl_b = sft.DefPoseOptimization(gpu_ctx, fb, synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    finally:
        gpu_ctx.set_option("wide_off", 0)
    assert fw.status == 0 and fb.status == 0
    assert (fw.iters, fw.trials, inl_w) == (fb.iters, fb.trials, inl_b)
    np.testing.assert_allclose(fw.trace[:fw.iters, :6], fb.trace[:fb.iters, :6], rtol=1e-7)
    np.testing.assert_allclose(fw.nodes_xyz, fb.nodes_xyz, rtol=0, atol=1e-9 * np.abs(fb.nodes_xyz).max())
    np.testing.assert_allclose(fw.pose7, fb.pose7, rtol=0, atol=1e-9)


def test_assembly_only_launches_leave_the_batch_intact(lab_ctx):
    """dsh_lab_sft_assemble_timed (measurement aid of the assembly roofline, lab build) runs a kernel of its own that does one
    linearisation + assembly per problem on the batch's buffers: a full run afterwards gives the same results bit for bit."""
    from defslam_amd import sft, synth
    gpu_ctx = lab_ctx
    tmpl, _ = synth.make_problem("smoke", 0)
    gpu_ctx.template_build(tmpl.xyz0, tmpl.facets)
    frames = [sft.frame_from_synth(synth.make_frame(tmpl, 300, p)) for p in range(6)]
    gpu_ctx.batch_upload(frames, synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    with pytest.raises(sft.DshError):
        gpu_ctx.batch_assemble_timed(1)          # nothing has run yet: H has no zero pattern to keep
    gpu_ctx.batch_run()
    gpu_ctx.batch_download()
    ref = [(f.nodes_xyz.copy(), f.pose7.copy(), f.iters, f.trials) for f in frames]
    ms = gpu_ctx.batch_assemble_timed(3)
    assert ms > 0
    with pytest.raises(sft.DshError):
        gpu_ctx.batch_download()                 # the assembly passes invalidated the run
    gpu_ctx.batch_run()
    gpu_ctx.batch_download()
    for f, (x, q, it, tr) in zip(frames, ref):
        assert (f.iters, f.trials) == (it, tr)
        np.testing.assert_array_equal(f.nodes_xyz, x)
        np.testing.assert_array_equal(f.pose7, q)


@pytest.mark.parametrize("cfg,pids,iters", [("smoke", (0, 1, 2, 3, 4, 5), 10), ("C2", (0, 5), 10), ("W16", (0, 1), 6), ("B272", (0,), 5), ("C5", (0,), 4), ("smoke", (7,), 1)])
def test_speculative_damping_trials_are_bit_identical(lab_ctx, cfg, pids, iters):
    """Latency mode (sft_spec_kernel): K workgroups per problem run K consecutive dampings of the rejection chain side by side
    and the next launch replays the Levenberg-Marquardt controller over them in trial order.  Same arithmetic on the same
    state: vertices, pose, per-observation errors, classification and the whole iteration trace equal the one-workgroup
    kernel bit for bit, for every lane count, tile mode (banded MFMA tiles, wide tiles) and for several problems per launch."""
    from defslam_amd import sft, synth
    ctx = lab_ctx
    runs = {}
    ctx.set_option("split", 0)     # the two-sided factorisation of wide bands eliminates in another order: its own test below
    try:
        for K in (1, 2, 3, 4):
            ctx.set_option("speculate", K)
            frames = []
            for pid in pids:
                tmpl, fr = synth.make_problem(cfg, pid)
                if not frames:
                    ctx.template_build(tmpl.xyz0, tmpl.facets)
                frames.append(sft.frame_from_synth(fr))
            inl = sft.DefPoseOptimizationBatch(ctx, frames, synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP, max_iters=iters)
            runs[K] = (frames, inl)
    finally:
        ctx.set_option("speculate", 0)
        ctx.set_option("split", 2)
    f1, i1 = runs[1]
    assert sum(f.trials for f in f1) > sum(f.iters for f in f1) or iters == 1   # the cases do reject trials
    for K in (2, 3, 4):
        fk, ik = runs[K]
        assert ik == i1
        for a, b in zip(fk, f1):
            assert (a.iters, a.trials, a.status) == (b.iters, b.trials, b.status)
            np.testing.assert_array_equal(a.trace, b.trace)
            np.testing.assert_array_equal(a.nodes_xyz, b.nodes_xyz)
            np.testing.assert_array_equal(a.pose7, b.pose7)
            np.testing.assert_array_equal(a.chi2_obs, b.chi2_obs)
            np.testing.assert_array_equal(a.mvbOutlier, b.mvbOutlier)
            np.testing.assert_array_equal(a.mappoints, b.mappoints)
            assert a.rep_error_f64 == b.rep_error_f64


@pytest.mark.parametrize("cfg,pids,iters", [("W16", (0, 3), 50), ("W12", (1, 4), 50), ("C5", (0,), 6), ("C2", (0, 7), 50)])
def test_two_sided_factorisation_follows_the_undivided_one_and_the_oracle(lab_ctx, oracle_mod, cfg, pids, iters):
    """Latency mode, wide band (128 < kd <= 256): the band ordering is cut at a separator of one bandwidth, two workgroups eliminate the two
    halves at the same time (the second one in reversed order), the separator + camera system is the sum of their Schur contributions
    (sft_wide.h, SftPart).  The library's default (option "split" = 2) also takes a NARROW band that is long enough this way -- C2: the
    left-looking wide-tile code on two workgroups beats the register-window solver on one (4.1 against 4.5 ms per frame).  The same Cholesky factorisation in another elimination order: the Levenberg-Marquardt trajectory (iterations,
    damping trials, accepted steps) is the undivided solver's and the oracle's, numbers agree to rounding.  A CONNECTED mesh: every
    curvature, stretching and observation edge that crosses the cut is in the system (nothing is dropped at the cut)."""
    from defslam_amd import sft, synth
    ctx = lab_ctx
    res = {}
    try:
        narrow = cfg == "C2"
        for split in (1, 0):
            ctx.set_option("split", (2 if narrow else 1) if split else 0)
            frames = []
            for pid in pids:
                tmpl, fr = synth.make_problem(cfg, pid)
                if not frames:
                    ctx.template_build(tmpl.xyz0, tmpl.facets)
                frames.append((sft.frame_from_synth(fr), fr, tmpl))
            inl = sft.DefPoseOptimizationBatch(ctx, [f for f, _, _ in frames], synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP, max_iters=iters)
            info = ctx.solver_info(0)
            assert info["tile_mode"] == (2 if (split or not narrow) else 1) and info["lanes"] >= 2 and info["split"] == split
            if split:
                _, counts = ctx.problem_info(0)
                Dn, kd = counts[5] - 6, counts[6]
                assert info["s"] >= kd and info["s"] % 16 == 0 and info["c0"] % 16 == 0 and info["c0"] > 0
                assert info["n1p"] - info["pad"] == Dn - info["c0"] - info["s"] and 0 <= info["pad"] < 16     # the three pieces tile the unknowns
            res[split] = (frames, inl)
    finally:
        ctx.set_option("split", 2)                                  # the library's default
    (fs, inl_s), (fu, inl_u) = res[1], res[0]
    assert inl_s == inl_u
    for (a, fr, tmpl), (b, _, _) in zip(fs, fu):
        assert a.status == 0 and b.status == 0
        assert (a.iters, a.trials) == (b.iters, b.trials)
        np.testing.assert_allclose(a.trace[:a.iters, :6], b.trace[:b.iters, :6], rtol=1e-7)
        np.testing.assert_array_equal(a.trace[:a.iters, 6:], b.trace[:b.iters, 6:])
        np.testing.assert_allclose(a.nodes_xyz, b.nodes_xyz, rtol=0, atol=1e-9 * np.abs(b.nodes_xyz).max())
        np.testing.assert_allclose(a.pose7, b.pose7, rtol=0, atol=1e-9)
        np.testing.assert_array_equal(a.mvbOutlier, b.mvbOutlier)
    if cfg != "C5":   # (the oracle's dense LDLT of the 2000-node problem takes minutes: its golden fixtures cover C5)
        for k, (a, fr, tmpl) in enumerate(fs):
            tc, args = oracle_args(oracle_mod, tmpl, fr)
            r = oracle_mod.sft_solve(*args)
            _compare(a, inl_s[k], r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret)


def test_changing_view_sequence_through_the_graph_cache(gpu_ctx, oracle_mod):
    """Seventy frames that each see a different 6x6 window of a 14x14 template: every frame has its own active set, the 65th evicts
    the graph cache while the device may still hold the previous batch.  The last frames are checked against the oracle."""
    from defslam_amd import sft, synth
    tmpl = synth.make_grid_template(14, 14)
    gpu_ctx.template_build(tmpl.xyz0, tmpl.facets)
    base = synth.make_frame(tmpl, 900, 3)
    views = [(r, c) for r in range(9) for c in range(9)][:70]
    for n, (r0, c0) in enumerate(views):
        keep = [c + 14 * r for r in range(r0, r0 + 6) for c in range(c0, c0 + 6)]
        sel = np.all(np.isin(base.obs_nodes, keep), axis=1)
        fr = synth.make_frame(tmpl, 900, 3)
        for k in ["obs_nodes", "obs_bary", "obs_uv", "obs_invsig2"]:
            setattr(fr, k, getattr(base, k)[sel])
        f = sft.frame_from_synth(fr)
        inl = sft.DefPoseOptimization(gpu_ctx, f, synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
        assert f.status == 0
        if n >= 66:
            tc, args = oracle_args(oracle_mod, tmpl, fr)
            r = oracle_mod.sft_solve(*args)
            _compare(f, inl, r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret)


@pytest.mark.parametrize("cfg,batch", [("W16", 1), ("W12", 3), ("C5", 1), ("W16", 40)])
def test_helper_workgroups_of_the_two_sided_factorisation_do_not_change_a_bit(lab_ctx, oracle_mod, cfg, batch):
    """Wide bands in latency mode: helper workgroups form the far products of a part's block columns on other CUs (sft_wide.h: factor_part,
    factor_wide_helper).  The owner takes a helper's column when it is there and forms it itself -- same routine, same order -- when it is not, so
    every setting must give the SAME BITS: no helpers (the owner is factor_wide), one to three per part with four or two lanes, and a launch with
    several times more workgroups than the device has CUs (40 problems x 4 lanes x 2 parts x 4 roles: helpers that start late or never, owners that
    fall back, helpers that skip).  The first problem also against the oracle (not the full-size C5: its dense CPU solve takes minutes and
    test_hip_matches_golden_vectors_full_size_c5 holds that comparison)."""
    from defslam_amd import sft, synth
    rows, cols, m = synth.CONFIGS[cfg]
    tmpl = synth.make_grid_template(rows, cols)
    lab_ctx.template_build(tmpl.xyz0, tmpl.facets)
    regs = (synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    syn = [synth.make_frame(tmpl, m, p) for p in range(batch)]
    ref = None
    # (lanes, helpers, wavefronts of a FACTOR workgroup: the sixteen-wavefront variant -- sft_part_factor_kernel, one live row per wave -- is a lab
    # build's A/B and has to give the same bits as well)
    settings = [(4, 0, 8), (4, 3, 8), (4, 1, 8), (2, 2, 8), (4, -1, 8), (4, 3, 16), (4, 1, 16)] if batch < 8 else [(4, 0, 8), (4, 3, 8), (2, 3, 8), (2, 3, 16)]
    try:
        for K, nh, ow in settings:
            lab_ctx.set_option("speculate", K)
            lab_ctx.set_option("helpers", nh)
            lab_ctx.set_option("owner_waves", ow)
            frames = [sft.frame_from_synth(fr) for fr in syn]
            lab_ctx.batch_upload(frames, *regs, 1, 50)
            info = lab_ctx.solver_info(0)
            assert info["split"] == 1 and info["lanes"] == K and info["tile_mode"] == 2
            lab_ctx.batch_run()
            inl = lab_ctx.batch_download()
            res = [(int(i), f.iters, f.trials, f.nodes_xyz.copy(), f.pose7.copy(), f.chi2_obs.copy(), f.mvbOutlier.copy(), f.trace.copy()) for i, f in zip(inl, frames)]
            if ref is None:
                ref = res
                continue
            for p, (a, b) in enumerate(zip(ref, res)):
                assert a[:3] == b[:3], (K, nh, p)
                for u, v in zip(a[3:], b[3:]):
                    np.testing.assert_array_equal(u, v, err_msg=f"lanes {K}, helpers {nh}, {ow} wavefronts, problem {p}")
    finally:
        lab_ctx.set_option("speculate", 0)
        lab_ctx.set_option("helpers", -1)
        lab_ctx.set_option("owner_waves", 8)
    if cfg == "C5":
        return
    fr = syn[0]
    tc = oracle_mod.template_build(tmpl.xyz0, tmpl.facets)
    r = oracle_mod.sft_solve(tc, fr.Tcw, fr.K, fr.n_frame, fr.obs_nodes, fr.obs_bary, fr.obs_uv, fr.obs_invsig2, fr.xyz, *regs, ldlt_mode=1)
    a = ref[0]
    assert (a[1], a[2], a[0]) == (r.iters, r.trials, r.ret)
    assert np.abs(a[3] - r.xyz).max() <= 1e-7 * np.abs(r.xyz).max() and np.abs(a[4] - r.pose7).max() <= 1e-8
    np.testing.assert_array_equal(a[6], np.asarray(r.outlier, bool))
