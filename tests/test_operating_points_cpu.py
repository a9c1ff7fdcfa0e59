"""CPU tests: the comparators of the SfT solve (the C oracle and its NumPy restatement) are right away from the one synthetic camera,
pose and weight triple (tests/operating_points.py), by checks that share no code with the oracle -- central differences, scipy -- and
every problem the GPU tests solve at these points is eligible for an exact comparison of Levenberg-Marquardt trajectories."""
import ctypes as C

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import operating_points as op
from conftest import oracle_args


def _same(a, b, path=""):
    """Every array (and scalar) of two generator results, bit for bit."""
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            _same(a[k], b[k], f"{path}/{k}")
    elif hasattr(a, "__dict__") and not isinstance(a, np.ndarray):
        _same(vars(a), vars(b), path)
    elif a is None:
        assert b is None, path
    else:
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), path


def test_generator_defaults_are_the_default_stream():
    """The camera, image size and scale keywords of the generators default to the one operating point bench.py, the goldens and the C5
    digests were made at: a default call and a call that spells the defaults out return the same arrays, bit for bit."""
    from defslam_amd import synth
    K, size = (500.0, 500.0, 320.0, 240.0), (640, 480)
    assert (synth.CAMERA_K, synth.IMAGE_SIZE) == (K, size)
    for rows, cols in [(9, 14), (10, 10)]:
        t0 = synth.make_grid_template(rows, cols)
        t1 = synth.make_grid_template(rows, cols, seed=1234, z0=1.0, camera=K, image_size=size)
        _same(t0, t1, "template")
        for pid in (0, 7):
            _same(synth.make_frame(t0, 300, pid), synth.make_frame(t1, 300, pid, camera=K, image_size=size, scale=1.0), "frame")
    _same(synth.make_sequence_frame(t0, 100, 5), synth.make_frame(t1, 100, 100005, phase=2.0 * np.pi * 5 / 100 - 0.3 * 100005,
                                                                  gt_pose=synth.sequence_gt_pose(5, 100), camera=K, image_size=size, scale=1.0), "sequence frame")
    for seed in (0, 3):
        a = synth.make_track_scene(seed, n_kp=600, n_frame_q=120, n_local_q=90, state_mix=True)
        b = synth.make_track_scene(seed, n_kp=600, n_frame_q=120, n_local_q=90, state_mix=True, camera=K, bounds=(0.0, 640.0, 0.0, 480.0), scale=1.0)
        _same(a, b, "track scene")
    # and the keywords do something: another camera gives another frame in that camera
    c = op.CASES["hamlyn/oblique/default"]
    t2 = synth.make_grid_template(9, 14, camera=c.K, image_size=c.image_size)
    f2 = synth.make_frame(t2, 300, 0, camera=c.K, image_size=c.image_size)
    assert tuple(f2.K) == c.K and f2.obs_uv[:, 0].max() > 640 and f2.obs_uv[:, 1].max() < 288 + 3


def test_cases_are_about_a_dozen_and_move_every_axis():
    cs = list(op.CASES.values())
    assert 10 <= len(cs) <= 14 and "synth/identity/default" in op.CASES
    assert {c.camera for c in cs} == set(op.CAMERAS) and {c.weights for c in cs} == set(op.WEIGHTS) and {c.world for c in cs} == set(op.WORLDS)
    assert {c.z0 for c in cs} == {0.15, 1.0, 8.0} and {c.noise for c in cs} == set(op.NOISE) and {c.n_frame for c in cs} == {300, 1200, 5000}
    names = op.batch_plan(512)
    assert names[:12] != sorted(names[:12]) and set(names[:12]) == set(op.CASE_NAMES)      # interleaved, not sorted by case
    assert min(names.count(n) for n in op.CASE_NAMES) >= 42


# ---- the camera Jacobian and the roles of fx and fy ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["hamlyn/oblique/default", "tall/turn_y/switch"])
def test_camera_jacobian_is_the_true_derivative_at_another_camera_and_a_large_pose(oracle_mod, case):
    """test_oracle_sft.py::test_camera_jacobian_is_the_true_derivative_node_jacobian_is_not at fx != fy and a pose far from identity: the C
    oracle's camera gradient b_cam = -J_cam^T w e against central differences of the NumPy graph's observation cost along the six pose
    directions.  Several observations, so that both image rows and all six columns carry weight."""
    from oracle import sft_oracle_np as onp
    tmpl, fr, _ = op.make_problem(case, 4, 4, 6, 1)
    fr.obs_uv = fr.obs_uv + np.array([3.0, -2.0])                      # residuals of a few pixels in both rows
    tc, args = oracle_args(oracle_mod, tmpl, fr, regs=(0.0, 0.0, 0.0))
    H, b, chi = oracle_mod.sft_system(*args)

    def chi_at(delta6):
        g = onp.Graph(*args)
        g.apply(np.concatenate([delta6, np.zeros(g.D - 6)]))
        c_obs = g.chi2_parts(g.residuals())[0]
        assert (c_obs < g.dsqr).all()                                  # below the Huber threshold: the cost is the plain sum
        return c_obs.sum()

    grad = np.zeros(6)
    for k in range(6):
        d = np.zeros(6)
        d[k] = 1e-6
        grad[k] = (chi_at(d) - chi_at(-d)) / 2e-6
    assert np.abs(grad).min() > 1e-6 * np.abs(grad).max()                 # every direction is exercised
    np.testing.assert_allclose(-2 * b[:6], grad, rtol=2e-5, atol=1e-9 * np.abs(grad).max())


@pytest.mark.parametrize("case", ["hamlyn/oblique/default", "tall/turn_y/switch"])
def test_u_row_responds_to_fx_only_and_v_row_to_fy_only(oracle_mod, case):
    """Perturb fx alone and fy alone.  On the NumPy graph, by central differences: d e_u / d fx = -x / z and d e_u / d fy = 0, d e_v / d fy =
    -y / z and d e_v / d fx = 0, with (x, y, z) the camera-frame point from scipy's rotation of the float32 pose -- an fx / fy swap in the
    restatement's projection fails here.  On the C oracle: its per-observation chi2 = w (e_u^2 + e_v^2) moves with fx by 2 w e_u d e_u / d fx
    and with fy by 2 w e_v d e_v / d fy -- a swap in the oracle's projection fails here -- and its camera gradient moves with fx through the
    u-row alone: d b_cam / d fx = -w (J_u^T e_u)' with J_u proportional to fx, which a swap in its Jacobian fails."""
    from oracle import sft_oracle_np as onp
    tmpl, fr, _ = op.make_problem(case, 4, 4, 5, 2)
    tc, args = oracle_args(oracle_mod, tmpl, fr, regs=(0.0, 0.0, 0.0))
    T = fr.Tcw.astype(np.float64)
    pw = (fr.obs_bary[:, :, None] * fr.xyz[fr.obs_nodes]).sum(1)
    pc = Rotation.from_matrix(T[:3, :3]).apply(pw) + T[:3, 3]
    w = fr.obs_invsig2 / fr.n_frame

    def with_K(dfx, dfy):
        a = list(args)
        a[2] = np.asarray(fr.K, np.float64) + np.array([dfx, dfy, 0.0, 0.0])
        return a

    def e_np(dfx, dfy):
        return onp.Graph(*with_K(dfx, dfy)).residuals()[0]

    def oracle_at(dfx, dfy):
        a = with_K(dfx, dfy)
        H, b, chi = oracle_mod.sft_system(*a)
        return chi, b[:6]

    h = 1e-3
    e0 = e_np(0, 0)
    assert np.abs(e0).min() > 0.01 and (w * (e0 ** 2).sum(1) < 5.991).all()
    de_dfx = (e_np(h, 0) - e_np(-h, 0)) / (2 * h)
    de_dfy = (e_np(0, h) - e_np(0, -h)) / (2 * h)
    # (x, y, z) from scipy's own projection of the float32 matrix onto a rotation: it is orthonormal to 1e-7 only, so is the agreement
    np.testing.assert_allclose(de_dfx[:, 0], -pc[:, 0] / pc[:, 2], rtol=5e-6)
    np.testing.assert_allclose(de_dfy[:, 1], -pc[:, 1] / pc[:, 2], rtol=5e-6)
    assert np.abs(de_dfx[:, 0]).min() > 1e-3 and np.abs(de_dfy[:, 1]).min() > 1e-3
    np.testing.assert_array_equal(de_dfx[:, 1], 0.0)                   # the v-row does not know fx
    np.testing.assert_array_equal(de_dfy[:, 0], 0.0)                   # the u-row does not know fy
    # the C oracle: robust chi2 of the system (all observations below the Huber threshold, no regulariser)
    (cxp, bxp), (cxm, bxm) = oracle_at(h, 0), oracle_at(-h, 0)
    (cyp, byp), (cym, bym) = oracle_at(0, h), oracle_at(0, -h)
    assert (cxp - cxm) / (2 * h) == pytest.approx((2 * w * e0[:, 0] * de_dfx[:, 0]).sum(), rel=5e-6)
    assert (cyp - cym) / (2 * h) == pytest.approx((2 * w * e0[:, 1] * de_dfy[:, 1]).sum(), rel=5e-6)
    # its camera gradient b_cam = -sum w (J_u^T e_u + J_v^T e_v): J_u = fx j_u, J_v = fy j_v with j_* the NumPy graph's rows at unit focal length
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    nul = np.zeros_like(x)
    ju = np.stack([x * y / z**2, -(1 + x * x / z**2), y / z, -1 / z, nul, x / z**2], 1)
    jv = np.stack([1 + y * y / z**2, -x * y / z**2, -x / z, nul, -1 / z, y / z**2], 1)
    fx, fy = fr.K[0], fr.K[1]
    b0 = oracle_mod.sft_system(*args)[1][:6]
    np.testing.assert_allclose(b0, -((w * e0[:, 0])[:, None] * fx * ju + (w * e0[:, 1])[:, None] * fy * jv).sum(0), rtol=5e-6, atol=5e-6 * np.abs(b0).max())
    db_dfx = -((w * (e0[:, 0] + fx * de_dfx[:, 0]))[:, None] * ju).sum(0)
    db_dfy = -((w * (e0[:, 1] + fy * de_dfy[:, 1]))[:, None] * jv).sum(0)
    np.testing.assert_allclose((bxp - bxm) / (2 * h), db_dfx, rtol=5e-6, atol=5e-6 * np.abs(db_dfx).max())
    np.testing.assert_allclose((byp - bym) / (2 * h), db_dfy, rtol=5e-6, atol=5e-6 * np.abs(db_dfy).max())
    assert not np.allclose(db_dfx, db_dfy, rtol=1e-2)


# ---- the two oracles against each other on every case -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", op.CASE_NAMES)
def test_c_oracle_matches_numpy_restatement_on_every_case(oracle_mod, case):
    """7 x 9 mesh, 200 matches: identical trajectories, states to the tolerance of test_c_oracle_matches_numpy_restatement_live."""
    from oracle import sft_oracle_np as onp
    rows, cols, m = op.SMALL
    tmpl, fr, regs = op.make_problem(case, rows, cols, m)
    tc, args = oracle_args(oracle_mod, tmpl, fr, regs=regs)
    r = oracle_mod.sft_solve(*args)
    rn = onp.solve(*args)
    assert r.iters == rn["iters"] >= 3
    np.testing.assert_array_equal(r.trace[:, [2, 6]], rn["trace"][:, [2, 6]])
    np.testing.assert_allclose(r.xyz, rn["xyz"], atol=1e-11)
    np.testing.assert_allclose(r.pose7, rn["pose7"], atol=1e-11)
    np.testing.assert_array_equal(r.outlier.astype(bool), rn["outlier"])
    assert r.ret == rn["ret"]


# ---- the branches of the matrix -> quaternion conversion --------------------------------------------------------------------------------
def test_worlds_enter_through_all_four_quaternion_branches(oracle_mod):
    """Every world's float32 pose takes the branch the table says (by trace and largest diagonal entry), the five worlds hit all four
    branches, and sft_oracle_pose_from_f32 agrees with scipy on exactly these matrices (and keeps the float32 translation)."""
    L = oracle_mod.lib()
    out = (C.c_double * 7)()
    seen = set()
    for world in op.WORLDS:
        T = op.move_pose(op.world_matrix(world), np.eye(4, dtype=np.float32))
        R = T[:3, :3].astype(np.float64)
        br = "trace" if np.trace(R) > 0 else int(np.argmax(np.diag(R)))
        assert br == op.WORLD_BRANCH[world] == op.quaternion_branch(T), world
        if br != "trace":
            assert np.trace(R) < -0.9 and np.diag(R)[br] > 0.9            # far inside its branch
        seen.add(br)
        L.sft_oracle_pose_from_f32(np.ascontiguousarray(T).ctypes.data_as(C.POINTER(C.c_float)), out)
        p = np.array(out[:])
        q = Rotation.from_matrix(R).as_quat()
        q = q if q[3] >= 0 else -q
        assert abs(q[3]) > 0.01 or world in ("identity", "oblique")      # w stays off the sign flip
        np.testing.assert_allclose(p[3:], q, atol=5e-7)                  # float32 input
        assert abs(np.linalg.norm(p[3:]) - 1) < 1e-14
        np.testing.assert_array_equal(p[:3], T[:3, 3].astype(np.float64))
    assert seen == {"trace", 0, 1, 2}
    for name, c in op.CASES.items():                                     # the frames of the cases start in their world's branch
        _, fr, _ = op.make_problem(c, 4, 4, 10)
        assert op.quaternion_branch(fr.Tcw) == op.WORLD_BRANCH[c.world], name


# ---- eligibility of everything the GPU tests solve ----------------------------------------------------------------------------------------
def _eligible(oracle_mod, tmpl_xyz0, facets, fr, regs, layers):
    tc = oracle_mod.template_build(tmpl_xyz0, facets)
    args = (tc, fr.Tcw, fr.K, fr.n_frame, fr.obs_nodes, fr.obs_bary, fr.obs_uv, fr.obs_invsig2, fr.xyz) + tuple(regs)
    r0 = oracle_mod.sft_solve(*args, layers=layers, ldlt_mode=0)
    r1 = oracle_mod.sft_solve(*args, layers=layers, ldlt_mode=1)
    assert r0.iters == r1.iters >= 3, "fewer than three iterations, or the two factorisations of the oracle part ways"
    np.testing.assert_array_equal(r0.trace[:, [2, 6]], r1.trace[:, [2, 6]])       # trial counts and accept flags
    assert r1.trace[:, 2].max() < 8, "an iteration with >= 8 dampings: accept / reject is rounding noise from there on"
    assert abs(r1.pose7[6]) >= 0.01 and abs(r0.pose7[6]) >= 0.01, "q_w near the sign flip"
    assert r1.ret > fr.obs_nodes.shape[0] / 2 and r0.ret == r1.ret
    return r1


USES = op.uses()


@pytest.mark.parametrize("use", USES, ids=[f"{u[0]}-{u[1]}x{u[2]}-m{u[3]}-id{u[4]}-layers{u[5]}" + (f"-cols{u[6]}" if u[6] else "") for u in USES])
def test_every_problem_of_the_gpu_tests_is_eligible(oracle_mod, use):
    """The GPU tests at these operating points compare trajectories exactly and allow no relaxed case, so every problem they solve (same
    mesh, match count, problem id, layers) must have a trajectory that is not decided by rounding: the oracle's two factorisations give the
    same trial counts and accept flags, no iteration needs eight or more dampings, at least three iterations, |q_w| >= 0.01 at the end,
    more than half of the matches inliers.  A problem that fails is replaced by another id in tests/operating_points.py."""
    name, rows, cols, m, pid, layers, keep_cols = use
    tmpl, fr, regs = op.make_problem(name, rows, cols, m, pid, keep_cols=keep_cols)
    _eligible(oracle_mod, tmpl.xyz0, tmpl.facets, fr, regs, layers)


@pytest.mark.parametrize("world,z0", op.BATCH_PLACEMENTS)
@pytest.mark.parametrize("name", op.CASE_NAMES)
def test_every_problem_of_the_mixed_batches_is_eligible(oracle_mod, world, z0, name):
    """The members of the mixed batches of the throughput shape: every case's camera, weights, noise and key point count on the batch's
    template, placement and scale (operating_points.batch_problem).  Same conditions."""
    tmpl, fr, regs = op.batch_problem(world, z0, name)
    assert tuple(fr.K) == op.CASES[name].K and regs == op.CASES[name].regs and fr.n_frame == op.CASES[name].n_frame
    assert op.quaternion_branch(fr.Tcw) == op.WORLD_BRANCH[world]
    _eligible(oracle_mod, tmpl.xyz0, tmpl.facets, fr, regs, 1)


def test_the_partial_view_of_the_layers_test_has_a_smaller_dimension_without_the_ring(oracle_mod):
    rows, cols, m, pid, kc = op.LAYERS_VIEW
    tmpl, fr, regs = op.make_problem(op.LAYERS_CASE, rows, cols, m, pid, keep_cols=kc)
    tc, args = oracle_args(oracle_mod, tmpl, fr, regs=regs)
    d0, d1, d2 = (oracle_mod.sft_system(*args, layers=k)[0].shape[0] for k in (0, 1, 2))
    assert d0 < d1 == d2 < 6 + 3 * tmpl.n


def test_the_patches_problem_of_the_two_rank_test_is_eligible(oracle_mod):
    """test_patches_on_separate_ranks_equal_the_joint_solve_of_the_oracle at another operating point: the union of the patches."""
    from test_shared_camera_gpu import _joint_problem
    name, rows, cols, cuts, m, pid = op.SHARED_CASE
    tmpl, fr, facets, _, regs = _joint_problem(rows, cols, cuts, m, pid, name)
    _eligible(oracle_mod, tmpl.xyz0, facets, fr, regs, 1)
