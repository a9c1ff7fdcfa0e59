"""The point-erase shim (integration/point_erase_hip.h) compiled against stand-in KeyFrame / MapPoint types and run on the device: for one
culling of mlpRecentAddedMapPoints and the drops of one Schwarp fit, the store route (MapPointCullingStoreHIP, DropMatchesStoreHIP: one
call each, the reference's mutations written back on the objects) and the host route (the reference's loops over the objects) leave every
mutated field identical -- isBad, Observations(), the observation maps, GetReferenceKeyFrame, the mvpMapPoints of every keyframe and the
edited recent list -- and both equal the restatement (tests/point_erase_ref.py)."""
import os

import numpy as np
import pytest

import point_erase_ref as PE
import shim_run
import store_model

INTEG = shim_run.INTEG


def test_shim_compiles_against_the_c_abi():
    shim_run.build()
    assert os.path.exists(shim_run.exe("point_erase_shim_test"))
    src = open(os.path.join(INTEG, "point_erase_hip.h")).read()
    assert "dsh_point_store_cull" in src and "dsh_point_store_erase_observations" in src and "defslam_hip_debug.h" not in src and "dsh_lab" not in src


@pytest.mark.gpu
def test_store_route_host_route_and_restatement_agree(tmp_path):
    shim_run.build()
    rm = PE.long_scene(seed=9, K=8, N=48, P=70)
    rng = np.random.default_rng(9)
    P = len(rm.points)
    for p in (3, 11):
        rm.points[p].bad = True                                   # bad already: they leave the list, their records stay
    first_kf = [int(v) for v in rng.integers(4, 9, P)]
    recent = [int(p) for p in rng.permutation(P)[:40]]
    recent += [p for p in (3, 11) if p not in recent]
    KF2, current_kf = 5, 9
    dropped = [p for p, mp in enumerate(rm.points) if KF2 in mp.obs][::2]
    for p in dropped[:4]:
        rm.points[p].ref = KF2                                  # the drop moves their reference keyframe
    src, dst = str(tmp_path / "map.txt"), str(tmp_path / "out.txt")
    words = lambda v: " ".join(map(str, v))
    store_model.write_scene(rm, src, f"{current_kf}\n{words(first_kf)}\n{words([len(recent)] + recent)}\n{words([KF2, len(dropped)] + dropped)}\n")
    shim_run.run("point_erase_shim_test", src, dst)
    got = store_model.parse_dump(dst)
    assert set(got) == {("store", "cull"), ("store", "drop"), ("host", "cull"), ("host", "drop")}
    action, c = rm.cull(recent, [first_kf[p] for p in recent], current_kf)
    assert set(action.tolist()) == {0, 1, 2, 3} and c["n_records"] > 0
    stays = [p for p, a in zip(recent, action) if a == 0]
    want = store_model.dump_of(rm, stays)
    for route in ("store", "host"):
        assert got[(route, "cull")] == want, route
    status, c = rm.erase_observations(dropped, [KF2] * len(dropped), erase_match=True)
    assert c["n_ref_moved"] > 0 and c["n_set_bad"] > 0 and 1 in status.tolist() and 2 in status.tolist()
    want = store_model.dump_of(rm, stays)
    for route in ("store", "host"):
        assert got[(route, "drop")] == want, route
    assert got[("store", "drop")] != got[("store", "cull")]
