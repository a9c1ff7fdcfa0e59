"""The local-map shim (integration/local_map_hip.h) compiled against stand-in KeyFrame / MapPoint / Frame types and run on the device:
UpdateLocalMapHIP and SearchLocalPointsStoreHIP change the stand-in objects exactly as the sequential restatements
(tests/local_map_ref.py, tests/track_search_ref.py) of the reference's calls do."""
import os

import numpy as np
import pytest

import shim_run
from test_local_map_cpu import scene_to_ref

INTEG = shim_run.INTEG
FRAME_ID = 7          # mnId of the driver's current frame


def test_local_map_shim_compiles_against_the_c_abi():
    shim_run.build()
    assert os.path.exists(shim_run.exe("localmap_shim_test"))
    src = open(os.path.join(INTEG, "local_map_hip.h")).read()
    assert "defslam_hip_debug.h" not in src and "dsh_lab" not in src


@pytest.mark.gpu
def test_local_map_shim_follows_the_reference_flow(tmp_path):
    from defslam_amd import synth, track
    shim_run.build()
    sc = synth.make_local_map_scene(21, n_kf=40, n_kp=500, obs_per_point=8, n_frame_kp=1000)
    synth.write_local_map_scene(sc, tmp_path / "in.txt")
    r = shim_run.run("localmap_shim_test", tmp_path / "in.txt", tmp_path / "out.txt", "0")
    P, K, N = sc["xyz"].shape[0], sc["tables"].shape[0], sc["frame_points"].shape[0]
    tok = iter(open(tmp_path / "out.txt").read().split())
    ints = lambda n: np.array([int(next(tok)) for _ in range(n)])
    n_kf, n_voted, ref, frame_ref = ints(4)
    local_kf, votes, frame_after_update = ints(n_kf), ints(n_voted), ints(N)
    n_pts = int(next(tok))
    local_pts, kf_stamp, pt_stamp = ints(n_pts), ints(K), ints(P)
    n2 = int(next(tok))
    loc = [(int(next(tok)), int(next(tok)), float(next(tok)), float(next(tok)), float(next(tok)), int(next(tok)), int(next(tok))) for _ in range(n_pts)]
    final = ints(N)
    host_way_equal = int(next(tok))

    # Tracking::UpdateLocalMap
    rm = scene_to_ref(sc)
    want = rm.update_local_map(sc["frame_points"])
    np.testing.assert_array_equal(local_kf, want["local_kf"])
    np.testing.assert_array_equal(votes, want["votes"])
    assert ref == frame_ref == want["ref_kf"] and want["ref_kf"] >= 0
    fp = np.where(want["frame_bad"], -1, sc["frame_points"])                  # Tracking.cc:1529
    assert want["frame_bad"].any()
    np.testing.assert_array_equal(frame_after_update, fp)
    np.testing.assert_array_equal(local_pts, want["local_points"])
    np.testing.assert_array_equal(kf_stamp, np.where(np.isin(np.arange(K), want["local_kf"]), FRAME_ID, 0))
    np.testing.assert_array_equal(pt_stamp, np.where(np.isin(np.arange(P), want["local_points"]), FRAME_ID, 0))
    # Tracking::SearchLocalPoints: a held point without observations is a candidate (state 2), as the shim's frame view says
    n_obs = np.bincount(sc["obs_point"], minlength=P)
    state = np.where(fp < 0, 0, np.where(n_obs[np.maximum(fp, 0)] > 0, 1, 2)).astype(np.uint8)
    s = rm.search_local_points(track.TrackFrame(**{**sc["frame"].__dict__, "state": state}), 3)
    assert n2 == s["nmatches"] and n2 > 0
    times_held = np.bincount(fp[fp >= 0], minlength=P)                        # the loop at :1408-1425 runs per key point of the frame
    held = times_held > 0
    assert times_held.max() == 2
    for q, (inv, lv, u, v, c, vis, seen_id) in enumerate(loc):
        p = want["local_points"][q]
        if held[p]:
            assert (inv, vis, seen_id) == (0, times_held[p], FRAME_ID)        # :1421-1424 once per holding key point, then skipped at :1449
            continue
        assert inv == int(s["in_view"][q]) and seen_id == 0 and vis == int(s["in_view"][q])
        if inv:
            assert (lv, np.float32(u), np.float32(v), np.float32(c)) == (s["level"][q], s["uv"][q, 0], s["uv"][q, 1], s["view_cos"][q])
    exp_final = fp.copy()
    m = s["match"]
    exp_final[m[m >= 0]] = want["local_points"][m >= 0]
    np.testing.assert_array_equal(final, exp_final)
    # the driver's cross-check: the host's std::map / std::set way over the same objects + SearchLocalPointsHIP gave the same
    assert host_way_equal == 1
