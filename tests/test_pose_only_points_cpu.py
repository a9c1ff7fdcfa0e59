"""CPU tests that make the operating points of the pose-only optimisation (tests/pose_only_points.py) trustworthy: every point is
eligible for an exact comparison, the table reaches the branches it is there for, the restatement (tests/pose_only_ref.py) is right
in the new places independently of any kernel, and the tolerance of the GPU tests is the measured reassociation noise."""
import dataclasses
import os
import re

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import pose_only_points as PP
import pose_only_ref as R

_SOLVED = {}


def solved(name):
    """model, frame and the restatement in the "sequential" order and the "device" order with block 64, 128 and 256: once per point."""
    if name not in _SOLVED:
        model, fr, _ = PP.build(name)
        res = {"sequential": R.solve(model, fr, "sequential")}
        for block in (64, 128, 256):
            res[block] = R.solve(model, fr, "device", block=block)
        _SOLVED[name] = (model, fr, res)
    return _SOLVED[name]


# ---- the table ---------------------------------------------------------------------------------------------------------------------------

def test_the_table_holds_what_it_is_there_for():
    P = PP.POINTS
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "defslam_amd", "csrc", "poseonly_problem.h")).read()
    assert int(re.search(r"#define PO_BLOCK (\d+)", header).group(1)) == PP.PO_BLOCK
    assert int(re.search(r"#define PO_MAX_LEVELS (\d+)", header).group(1)) == PP.PO_MAX_LEVELS
    assert 12 <= len(P) <= 16
    c = P["control"]
    assert (c.camera, c.world, c.z0, c.levels, c.scale_factor) == ("synth", "identity", 1.0, 8, 1.2)
    assert {p.world for p in P.values()} == set(PP.WORLDS)
    assert {"hamlyn", "tall"} <= {p.camera for p in P.values()} and {p.z0 for p in P.values()} == set(PP.SCALES)
    assert {1, 8, PP.PO_MAX_LEVELS} <= {p.levels for p in P.values()} and any(p.scale_factor != 1.2 for p in P.values())
    turned = [p for p in P.values() if p.world.startswith("turn_")]
    assert any(p.args.get("outlier_share", 0) >= 0.2 for p in turned)
    assert {64, 65, PP.PO_BLOCK - 1, PP.PO_BLOCK, PP.PO_BLOCK + 1} <= {p.args["held"] for p in turned}     # a full wavefront / workgroup, one more
    assert {3, 9} <= {p.args["held"] for p in turned}
    assert all(p.args["N"] <= 400 and p.args["held"] <= PP.PO_BLOCK + 1 for p in P.values())
    assert P[PP.BEHIND].args["behind"] == 2
    order = PP.plan()
    assert sorted(order) == sorted(P) and order != sorted(order, key=lambda n: P[n].world) and order != sorted(order, key=lambda n: P[n].camera)
    assert 0 < order.index("turn_y_held2") < len(order) - 1                   # the problem with n_initial < 3 is in the middle
    assert (P[order[0]].levels, P[order[0]].camera) != (8, "synth")           # problem 0 of the batch has neither the usual table nor K


def test_the_defaults_of_make_case_are_the_old_frustum_and_table():
    """The camera and the sigma table are parameters now; a case that names neither carries FX, FY, CX, CY and sigma_table()."""
    _, fr, _ = R.make_case(**R.GPU_CASES["held9"])
    assert fr.K.tolist() == [R.FX, R.FY, R.CX, R.CY] and np.array_equal(fr.inv_level_sigma2, R.sigma_table())
    _, fr, _ = R.make_case(camera=PP.CAMERAS["tall"], sigma=R.sigma_table(3, 1.5), **R.GPU_CASES["held9"])
    assert fr.K.tolist() == [float(np.float32(v)) for v in PP.CAMERAS["tall"][:4]] and fr.octave.max() == 2
    held = fr.kp[fr.frame_points >= 0]
    assert (held[:, 0] < 288 + 30).all() and (held[:, 1] > 288 + 30).any()      # the key points fill the tall image


@pytest.mark.parametrize("name", PP.POINT_NAMES)
def test_every_point_is_eligible(name):
    """The "sequential" order and the "device" order with block 64, 128 and 256 agree on every decision: no accept / reject and no flag
    of the point is a coin flip at the rounding floor.  A seed that fails is replaced in the table, with a comment."""
    _, _, res = solved(name)
    want = R.decisions(res["sequential"])
    for block in (64, 128, 256):
        assert R.decisions(res[block]) == want, (name, block)
        assert np.array_equal(res[block].outlier, res["sequential"].outlier), (name, block)
        assert np.abs(res[block].Tcw.view(np.int32).astype(np.int64) - res["sequential"].Tcw.view(np.int32)).max() <= 1, (name, block)


def test_coverage_of_the_table():
    """What the points are there to reach, asserted on the restatement so that the table cannot quietly lose a branch."""
    print(f"\n{'point':24s} {'branch':>6s} {'raw w':>8s} {'|qw| end':>8s} {'huber <=/>':>11s} {'pivoted':>8s}  stops / iters / trials")
    stops, flipped, pivoted, huber_both = set(), [], 0, []
    for name, pt in PP.POINTS.items():
        _, fr, res = solved(name)
        r = res[256]
        branch, s = PP.quaternion_branch(fr.Tcw), r.stats
        assert branch == PP.WORLD_BRANCH[pt.world], (name, branch)
        start = R.pose_from_f32_matrix(fr.Tcw)
        assert start[6] >= 0 and abs(abs(s["start_raw_w"]) - start[6]) < 1e-6, name
        if pt.world.startswith("turn_"):
            assert start[6] >= 0.01 and abs(r.pose[6]) >= 0.01, (name, start[6], r.pose[6])           # off the coin flip at w = 0
            assert start[6] <= 0.2, (name, start[6])                                                  # and w is small, which is the point
        if s["start_raw_w"] < 0:
            flipped.append(name)
        if s["huber_below"] and s["huber_above"]:
            huber_both.append(name)
        pivoted += s["pivoted_solves"]
        stops |= {x.stop for x in r.rounds}
        print(f"{name:24s} {branch!s:>6s} {s['start_raw_w']:8.4f} {abs(r.pose[6]):8.4f} {s['huber_below']:6d}/{s['huber_above']:<4d} "
              f"{s['pivoted_solves']:3d}/{s['solves']:<4d}  {[x.stop for x in r.rounds]} {[x.iters for x in r.rounds]} {[x.trials for x in r.rounds]}")
    old = set()
    for kw in R.GPU_CASES.values():
        model, fr, _ = R.make_case(**kw)
        if kw["N"] <= 1200:
            old |= {x.stop for x in R.solve(model, fr, "device").rounds}
    print(f"stop reasons in POINTS: {sorted(stops)}; in GPU_CASES: {sorted(old)}")
    assert {"nbad", "rho", "iters"} <= stops
    # "qmax" occurs in the table (turn_x_at_optimum) and in no case of GPU_CASES; "empty" occurs in GPU_CASES (all_flagged) only
    assert "qmax" in stops and "qmax" not in old and "empty" in old and "empty" not in stops
    assert {PP.WORLD_BRANCH[PP.POINTS[n].world] for n in flipped} == {0, 1, 2}, flipped    # the flip runs behind each non-trace branch
    assert len(huber_both) >= 10 and pivoted > 0
    # a world's branch is a property of the world, not of a seed: the noise-free cases take it too
    for name, pt in PP.NOISE_FREE.items():
        assert PP.quaternion_branch(PP.build(pt)[1].Tcw) == PP.WORLD_BRANCH[pt.world], name


def test_behind_camera_has_two_points_at_negative_depth():
    model, fr, res = solved(PP.BEHIND)
    at_start = np.sort(PP.depths(model, fr, R.pose_from_f32_matrix(fr.Tcw)))
    at_end = np.sort(PP.depths(model, fr, res[256].pose))
    print(f"depths at the start {at_start[:3]}, at the final estimate {at_end[:3]}")
    assert (at_start[:2] <= -0.5).all() and np.isfinite(at_start).all() and at_start[2] > 0
    assert (at_end[:2] < 0).all() and at_end[2] > 0
    assert len(res[256].rounds) == 4 and all(r.iters >= 1 for r in res[256].rounds)


# ---- the restatement in the new places ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("camera,world", [("hamlyn", "turn_x"), ("tall", "turn_z"), ("hamlyn", "turn_y")])
def test_jacobian_against_central_differences_at_a_turned_pose(camera, world):
    """test_jacobian_against_central_differences of test_pose_only_cpu.py with fx / fy = 1.8 and its inverse, at a pose whose
    quaternion has a small w, one of the six points at negative depth."""
    rng = np.random.default_rng(2)
    K = [float(v) for v in PP.CAMERAS[camera][:4]]
    Xc = np.stack([rng.uniform(-2, 2, 6), rng.uniform(-1.5, 1.5, 6), rng.uniform(3, 8, 6)], 1)
    Xc[4] *= -0.5                                                              # behind the camera
    own = R.true_pose(rng)
    pose = R.pose_from_f32_matrix(PP.moved_pose(PP.Point(camera, world, 1.0, 8, 1.2), own).astype(np.float32))
    assert 0 <= pose[6] <= 0.2                                                 # a small w: the camera has turned by more than 157 degrees
    Rm, t = np.array(R.quat_to_R(pose[3:])).reshape(3, 3), np.array(pose[:3])
    X = (Xc - t) @ Rm                                                          # R' (x - t): the camera-frame points are Xc at `pose`
    uv, w = rng.uniform(0, 600, (6, 2)), np.ones(6)
    _, _, _, px, py, pz = R.edge_error(pose, K, X, uv, w)
    assert np.abs(np.stack([px, py, pz], 1) - Xc).max() < 1e-12 and pz[4] < -1
    A0, A1 = R.edge_jacobian(K, px, py, pz)
    h = 1e-6
    for d in range(6):
        dp, dm = [0.0] * 6, [0.0] * 6
        dp[d], dm[d] = h, -h
        ep, em = R.edge_error(R.exp_times(dp, pose), K, X, uv, w), R.edge_error(R.exp_times(dm, pose), K, X, uv, w)
        assert np.abs((ep[0] - em[0]) / (2 * h) - A0[d]).max() < 1e-5 * max(1.0, np.abs(A0[d]).max())
        assert np.abs((ep[1] - em[1]) / (2 * h) - A1[d]).max() < 1e-5 * max(1.0, np.abs(A1[d]).max())


@pytest.mark.parametrize("name", list(PP.NOISE_FREE))
def test_recovers_the_known_moved_pose_from_noise_free_matches(name):
    """For each world and scale: [R | z0 t] G^-1 to 10 x the float32 spacing of its entries, the bound of
    test_recovers_a_known_pose_from_noise_free_matches."""
    pt = PP.NOISE_FREE[name]
    model, fr, want = PP.build_noise_free(name)
    want = want.astype(np.float32)
    # the seed was chosen on the input alone: it is the first from its base whose known pose has no entry too small for the bound
    n = list(PP.NOISE_FREE).index(name) + 1
    for seed in range(100 * n, pt.args["seed"] + 1):
        p = dataclasses.replace(pt, args=dict(pt.args, seed=seed))
        assert PP.noise_free_entries_ok(p, PP.moved_pose(p, PP.build(p)[2])) == (seed == pt.args["seed"]), (name, seed)
    res = R.solve(model, fr)
    err = np.abs(res.Tcw - want)
    bound = 10 * np.spacing(np.abs(want).astype(np.float32))
    print(f"{name}: largest error / bound {float((err / bound).max()):.3f}, largest error {float(err.max()):.3e}")
    assert res.rounds[-1].bad == 0 and res.n_good == 80
    assert (err <= bound).all(), (name, float((err / bound).max()))


@pytest.mark.parametrize("branch", ["trace", 0, 1, 2])
def test_quaternion_round_trip_against_scipy(branch):
    """pose_from_f32_matrix(pose_to_f32_matrix(p)) at 20 rotations per branch of the conversion, angles up to 0.99 pi about each axis
    among them: the same rotation as scipy's, w >= 0, and the branch is the one intended."""
    rng = np.random.default_rng(5)
    rots = []
    if branch == "trace":
        rots += [Rotation.from_rotvec(a * np.eye(3)[k]) for k in range(3) for a in (0.0, 1e-9, 0.3, -0.6)]
        while len(rots) < 20:
            v = rng.normal(size=3)
            rots.append(Rotation.from_rotvec(v / np.linalg.norm(v) * rng.uniform(0, 2.0)))
    else:
        rots += [Rotation.from_rotvec(a * np.pi * np.eye(3)[branch]) for a in (0.99, -0.99, 0.9, 0.75, -0.8)]
        while len(rots) < 20:
            v = np.eye(3)[branch] + rng.uniform(-0.25, 0.25, 3)
            rots.append(Rotation.from_rotvec(v / np.linalg.norm(v) * rng.choice([-1, 1]) * rng.uniform(0.72, 0.995) * np.pi))
    raw_negative = 0
    for rot in rots:
        q = rot.as_quat()
        q = q if q[3] >= 0 else -q
        p = [0.5, -1.5, 2.5] + [float(v) for v in q]
        T = R.pose_to_f32_matrix(p)
        assert PP.quaternion_branch(T) == branch
        back = R.pose_from_f32_matrix(T)
        raw_negative += R.quat_from_R([float(v) for v in T[:3, :3].reshape(9)])[3] < 0
        assert back[:3] == p[:3] and back[6] >= 0
        # float32 entries: the rotation comes back to a few float32 ulp, and it is scipy's rotation of the same matrix
        assert np.abs(np.array(R.quat_to_R(back[3:])).reshape(3, 3) - rot.as_matrix()).max() < 4e-7
        sq = Rotation.from_matrix(T[:3, :3].astype(float)).as_quat()
        assert min(np.abs(np.array(back[3:]) - sq).max(), np.abs(np.array(back[3:]) + sq).max()) < 4e-7
    if branch != "trace":
        assert 0 < raw_negative < 20                                          # both signs of the raw w, so the flip runs and does not


# ---- the tolerance -----------------------------------------------------------------------------------------------------------------------

def test_tolerances_are_the_measured_reassociation_noise():
    """Per scene scale the largest |pose_sequential - pose_device| over the points (one number per scale, nothing normalised), and the
    largest relative chi2 difference over all rounds: not above the recorded constants, which are no more than twice the measurement;
    the GPU tolerance is 16 x the constant."""
    worst, worst_chi = {z: 0.0 for z in PP.SCALES}, 0.0
    for name, pt in PP.POINTS.items():
        _, _, res = solved(name)
        a, b = res["sequential"], res[256]
        d = float(np.abs(a.pose - b.pose).max())
        c = max([abs(x.chi2 - y.chi2) / max(x.chi2, 1.0) for x, y in zip(a.rounds, b.rounds)] or [0.0])
        print(f"{name:24s} z0 {pt.z0:5g}: |pose_sequential - pose_device| {d:.3e}, relative chi2 difference {c:.3e}")
        worst[pt.z0], worst_chi = max(worst[pt.z0], d), max(worst_chi, c)
    for z in PP.SCALES:
        print(f"z0 = {z:g}: measured {worst[z]:.3e}, recorded {PP.MEASURED_ORDER_NOISE[z]:.3e}, GPU tolerance {PP.POSE_TOL[z]:.3e}")
        assert worst[z] <= PP.MEASURED_ORDER_NOISE[z] <= 2 * worst[z], (z, worst[z])
        assert PP.POSE_TOL[z] == 16 * PP.MEASURED_ORDER_NOISE[z]
    print(f"chi2: measured {worst_chi:.3e}, recorded {PP.MEASURED_CHI2_NOISE:.3e}, GPU tolerance {PP.CHI2_RTOL:.3e}")
    assert worst_chi <= PP.MEASURED_CHI2_NOISE <= 2 * worst_chi and PP.CHI2_RTOL == 16 * PP.MEASURED_CHI2_NOISE
    assert (R.POSE_TOL, R.CHI2_RTOL) == (16 * 7.0e-16, 16 * 7.4e-15)          # those of the existing cases stay as they are
