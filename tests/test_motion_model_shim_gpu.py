"""The motion-model shim (integration/motion_model_hip.h) compiled against stand-in types and run on the device: EndTrackedFrameHIP and
TrackWithMotionModelStoreHIP leave the stand-in frames exactly as the host's loops and SearchByProjectionHIP over a second copy of them
do, and both equal the sequential restatement (tests/motion_model_ref.py)."""
import os

import numpy as np
import pytest

import motion_model_ref as M
import track_close_ref as T
import shim_run

INTEG = shim_run.INTEG


def test_motion_model_shim_compiles_against_the_c_abi():
    shim_run.build()
    assert os.path.exists(shim_run.exe("motionmodel_shim_test"))
    src = open(os.path.join(INTEG, "motion_model_hip.h")).read()
    assert "defslam_hip_debug.h" not in src and "dsh_lab" not in src
    assert "dsh_search_by_projection" not in src and "world_pos" not in src       # nothing per map point is packed on the host


def mark_outliers(fp):
    """The driver's rule: every seventh held entry of a searched frame becomes an outlier."""
    out = np.zeros(fp.shape[0], np.uint8)
    held = np.nonzero(fp >= 0)[0]
    out[held[6::7]] = 1
    return out


@pytest.mark.gpu
def test_motion_model_shim_store_way_host_way_and_restatement_agree(tmp_path):
    from defslam_amd import synth
    shim_run.build()
    sc = synth.make_track_close_scene(1, n_kf=30, n_kp=300, obs_per_point=6, n_frame_kp=600)
    synth.write_local_map_scene(sc, tmp_path / "map.txt")
    synth.write_track_close_scene(sc, T.previous_frame_points(sc), tmp_path / "close.txt")
    r = shim_run.run("motionmodel_shim_test", tmp_path / "map.txt", tmp_path / "close.txt", tmp_path / "out.txt", "0")
    N = sc["final_points"].shape[0]
    tok = iter(open(tmp_path / "out.txt").read().split())
    ints = lambda n: [int(next(tok)) for _ in range(n)]

    def way():
        frames = [dict(end=ints(3), end_points=ints(N), end_outlier=ints(N))]
        for _ in range(2):
            f = dict(search=ints(2), points=ints(N), outlier=ints(N))
            f.update(end=ints(3), end_points=ints(N), end_outlier=ints(N))
            frames.append(f)
        return frames

    dev, host = way(), way()
    assert next(tok, None) is None
    assert dev == host                                                # mvpMapPoints, mvbOutlier and the counts of the two ways

    rm = M.scene_to_ref(sc)
    octave = sc["frame"].arrays()["octave"]
    fp, out = sc["final_points"], sc["outlier"]
    for t, f in enumerate(dev):
        if t > 0:
            if t == 2:
                for p in sc["late_bad"]:
                    rm.set_bad(int(p))
            s = rm.motion_model_search(sc["frame"] if t == 1 else sc["frame_after"])
            assert f["search"] == [s["nmatches"], int(s["th_used"])] and f["points"] == s["frame_points"].tolist()
            assert s["nmatches"] >= 20 and not any(f["outlier"])
            fp, out = s["frame_points"], mark_outliers(s["frame_points"])
        e = rm.end_frame(fp, out, octave)
        assert f["end"] == [e["cleaned"], e["dropped"], e["kept"]]
        # the frame after the outlier drop: the list's points; the flags are those after CleanMatches (a dropped outlier keeps its flag)
        assert f["end_points"] == rm.last_frame()[0].tolist() and f["end_outlier"] == e["outlier"].astype(int).tolist()
    assert dev[0]["end"][0] > 0 and all(f["end"][1] > 0 for f in dev)    # CleanMatches and the drop both had work
