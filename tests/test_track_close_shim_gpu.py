"""The track-close shim (integration/track_close_hip.h) compiled against stand-in types and run on the device: CloseTrackedFrameHIP and
MapPointCullingHIP leave the stand-in objects exactly as the host's loops over a second copy of them do, and both equal the sequential
restatement (tests/track_close_ref.py)."""
import os

import numpy as np
import pytest

import track_close_ref as T
import shim_run

INTEG = shim_run.INTEG


def test_track_close_shim_compiles_against_the_c_abi():
    shim_run.build()
    assert os.path.exists(shim_run.exe("trackclose_shim_test"))
    src = open(os.path.join(INTEG, "track_close_hip.h")).read()
    assert "defslam_hip_debug.h" not in src and "dsh_lab" not in src


@pytest.mark.gpu
def test_track_close_shim_device_way_host_way_and_restatement_agree(tmp_path):
    from defslam_amd import synth
    shim_run.build()
    sc = synth.make_track_close_scene(1, n_kf=30, n_kp=300, obs_per_point=6, n_frame_kp=600)
    prev = T.previous_frame_points(sc)
    synth.write_local_map_scene(sc, tmp_path / "map.txt")
    synth.write_track_close_scene(sc, prev, tmp_path / "close.txt")
    r = shim_run.run("trackclose_shim_test", tmp_path / "map.txt", tmp_path / "close.txt", tmp_path / "out.txt", "0")
    P = sc["xyz"].shape[0]
    tok = iter(open(tmp_path / "out.txt").read().split())

    def way():
        head = [int(next(tok)) for _ in range(10)]
        recent = [int(next(tok)) for _ in range(head[9])]
        rows = [(np.float32(next(tok)), np.float32(next(tok)), np.float32(next(tok)), int(next(tok)), int(next(tok)), int(next(tok)), int(next(tok)))
                for _ in range(P)]
        return head, recent, rows

    dev = way()
    store = [(np.float32(next(tok)), np.float32(next(tok)), np.float32(next(tok)), int(next(tok)), int(next(tok)), int(next(tok))) for _ in range(P)]
    host = way()
    assert dev == host                                                # the objects of the two ways: counts, the list, every mutated field

    rm = T.scene_to_ref(sc)
    c = T.run_generated_frame(rm, sc)
    ids, first_kf = T.cull_list(sc)
    act = rm.cull(ids, first_kf, sc["current_kf"])
    head, recent, rows = dev
    assert head[:8] == [c[k] for k in T.COUNT_NAMES] and all(v > 0 for v in head[:8])
    assert head[8] == int((act == 2).sum()) > 0 and recent == ids[act == 0].tolist() and len(recent) > 0
    v, f, o, x = rm.track_state()
    assert np.array([r[:3] for r in rows], np.float32).tobytes() == x.tobytes()
    assert [r[3] for r in rows] == f.tolist() and [r[4] for r in rows] == v.tolist() and [r[5] for r in rows] == o.tolist()
    assert [bool(r[6]) for r in rows] == [p.bad for p in rm.points]
    # the store itself holds the same
    assert np.array([s[:3] for s in store], np.float32).tobytes() == x.tobytes()
    assert [s[3] for s in store] == f.tolist() and [s[4] for s in store] == v.tolist() and [s[5] for s in store] == o.tolist()
