"""The pose-only shim (integration/pose_only_hip.h) compiled against stand-in Frame / MapPoint types and run on the device: for a frame
of each case, the store way (PoseOptimizationStoreHIP: one call, mvbOutlier and the pose written back on the frame) and the host way (the
reference's optimiser written out as loops over the stand-in objects, positions read from them, sums in edge order) agree with the
restatement tests/pose_only_ref.py in the sense of tests/test_pose_only_gpu.py: the store way with the "device" order and the host way
with the "sequential" order, exactly in the return value, the flags and the counts per round, within POSE_TOL / CHI2_RTOL in pose and
chi2, within one float32 ulp in the frame's pose; and the two ways agree with each other in every decision."""
import os

import numpy as np
import pytest

import pose_only_ref as R
import shim_run
import store_model

INTEG = shim_run.INTEG
CASES = ["held2", "held9", "held65", "outliers20", "outlier_returns", "all_flagged"]


def test_shim_compiles_against_the_c_abi():
    shim_run.build()
    assert os.path.exists(shim_run.exe("poseonly_shim_test"))
    src = open(os.path.join(INTEG, "pose_only_hip.h")).read()
    assert "dsh_track_pose_only" in src and "PoseOptimizationStoreHIP" in src and "defslam_hip_debug.h" not in src and "dsh_lab" not in src


def write_frame(fr, entry, path):
    f32 = lambda v: " ".join(repr(float(x)) for x in np.asarray(v, np.float32).reshape(-1))
    N = len(fr.frame_points)
    with open(path, "w") as f:
        f.write(f"{N} {len(fr.inv_level_sigma2)} {f32(fr.K)}\n{f32(fr.Tcw)}\n{f32(fr.inv_level_sigma2)}\n")
        for i in range(N):
            f.write(f"{f32(fr.kp[i])} {int(fr.octave[i])} {int(fr.frame_points[i])} {int(entry[i])}\n")


def parse(path):
    out, way = {}, None
    for ln in open(path).read().splitlines():
        w = ln.split()
        if w[0] in ("dev", "host"):
            way = out.setdefault(w[0], {})
            way["ret"], way["n_initial"], way["rounds"] = (int(x) for x in w[1:])
        elif w[0] == "time_us":
            out["time_us"] = float(w[1])
        elif w[0] in ("iters", "trials", "bad", "flags"):
            way[w[0]] = [int(x) for x in w[1:]]
        elif w[0] in ("chi2", "pose"):
            way[w[0]] = np.array([float(x) for x in w[1:]])
        elif w[0] == "Tcw":
            way["Tcw"] = np.array([int(x) for x in w[1:]], np.uint32).view(np.float32).reshape(4, 4)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_store_way_host_way_and_restatement_agree(tmp_path, name):
    shim_run.build()
    model, fr, _ = R.make_case(**R.GPU_CASES[name])
    entry = np.arange(len(fr.frame_points)) % 3 == 0                     # mvbOutlier on entry: kept where no point is held
    scene, frame, dst = str(tmp_path / "scene.txt"), str(tmp_path / "frame.txt"), str(tmp_path / "out.txt")
    store_model.write_scene(model, scene)
    write_frame(fr, entry, frame)
    shim_run.run("poseonly_shim_test", scene, frame, dst)
    got = parse(dst)
    print(f"{name}: host way {got['time_us']:.0f} us")
    for way, order in (("dev", "device"), ("host", "sequential")):
        ref, g = R.solve(model, fr, order, outlier=entry), got[way]
        nr = len(ref.rounds)
        assert (g["ret"], g["n_initial"], g["rounds"]) == (ref.n_good, ref.n_initial, nr), (name, way)
        for key in ("iters", "trials", "bad"):
            assert g[key] == [getattr(r, key) for r in ref.rounds] + [0] * (4 - nr), (name, way, key)
        assert g["flags"] == ref.outlier.astype(int).tolist(), (name, way)
        assert np.abs(g["pose"] - ref.pose).max() <= R.POSE_TOL, (name, way, np.abs(g["pose"] - ref.pose).max())
        for k, r in enumerate(ref.rounds):
            assert abs(g["chi2"][k] - r.chi2) <= R.CHI2_RTOL * max(r.chi2, 1.0), (name, way, k)
        assert np.abs(g["Tcw"].view(np.int32).astype(np.int64) - ref.Tcw.view(np.int32)).max() <= 1, (name, way)
        if nr == 0:
            assert np.array_equal(g["Tcw"], np.asarray(fr.Tcw, np.float32).reshape(4, 4)), (name, way)
    for key in ("ret", "n_initial", "rounds", "iters", "trials", "bad", "flags"):
        assert got["dev"][key] == got["host"][key], (name, key)
