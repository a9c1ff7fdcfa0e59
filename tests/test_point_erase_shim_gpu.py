"""The point-erase shim (integration/point_erase_hip.h) compiled against stand-in KeyFrame / MapPoint types and run on the device: for one
culling of mlpRecentAddedMapPoints and the drops of one Schwarp fit, the store route (MapPointCullingStoreHIP, DropMatchesStoreHIP: one
call each, the reference's mutations written back on the objects) and the host route (the reference's loops over the objects) leave every
mutated field identical -- isBad, Observations(), the observation maps, GetReferenceKeyFrame, the mvpMapPoints of every keyframe and the
edited recent list -- and both equal the restatement (tests/point_erase_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

import point_erase_ref as PE
from conftest import ROOT

INTEG = os.path.join(ROOT, "integration")


def test_shim_compiles_against_the_c_abi():
    subprocess.run(["make", "-C", INTEG], check=True, capture_output=True)
    assert os.path.exists(os.path.join(INTEG, "build", "point_erase_shim_test"))
    src = open(os.path.join(INTEG, "point_erase_hip.h")).read()
    assert "dsh_point_store_cull" in src and "dsh_point_store_erase_observations" in src and "defslam_hip_debug.h" not in src and "dsh_lab" not in src


def write_map(path, rm, first_kf, current_kf, recent, KF2, dropped):
    with open(path, "w") as f:
        f.write(f"{len(rm.points)} {len(rm.kfs)}\n")
        for p, mp in enumerate(rm.points):
            f.write(f"{int(mp['mbBad'])} {mp['mpRefKF']} {mp['mnFound']} {mp['mnVisible']} {first_kf[p]}\n")
        for kf in rm.kfs:
            f.write(" ".join(map(str, [len(kf["mvpMapPoints"])] + kf["mvpMapPoints"])) + "\n")
        f.write(f"{len(rm.log)}\n" + "".join(f"{p} {s} {i}\n" for p, s, i in rm.log))
        f.write(" ".join(map(str, [current_kf, len(recent)] + recent)) + "\n")
        f.write(" ".join(map(str, [KF2, len(dropped)] + dropped)) + "\n")


def parse(path):
    """(route, step) -> dict(recent=[ids], pts={id: (bad, nObs, ref, {slot: idx})}, kfs={slot: table})"""
    out = {}
    for line in open(path):
        w = line.split()
        r = out.setdefault((w[0], w[1]), dict(recent=None, pts={}, kfs={}))
        if w[2] == "recent":
            r["recent"] = [int(x) for x in w[3:]]
        elif w[2] == "kf":
            r["kfs"][int(w[3])] = [int(x) for x in w[4:]]
        else:
            head, obs = line.split("|")
            h = head.split()
            r["pts"][int(h[3])] = (int(h[4]), int(h[5]), int(h[6]), {int(a.split(":")[0]): int(a.split(":")[1]) for a in obs.split()})
    return out


def restated(rm, recent):
    return dict(recent=list(recent), pts={p: (int(mp["mbBad"]), mp["nObs"], mp["mpRefKF"], rm.observations(p)) for p, mp in enumerate(rm.points)},
                kfs={s: list(kf["mvpMapPoints"]) for s, kf in enumerate(rm.kfs)})


@pytest.mark.gpu
def test_store_route_host_route_and_restatement_agree(tmp_path):
    subprocess.run(["make", "-C", INTEG], check=True, capture_output=True)
    rm = PE.long_scene(seed=9, K=8, N=48, P=70)
    rng = np.random.default_rng(9)
    P = len(rm.points)
    for p in (3, 11):
        rm.points[p]["mbBad"] = True                                   # bad already: they leave the list, their records stay
    first_kf = [int(v) for v in rng.integers(4, 9, P)]
    recent = [int(p) for p in rng.permutation(P)[:40]]
    recent += [p for p in (3, 11) if p not in recent]
    KF2, current_kf = 5, 9
    dropped = [p for p, mp in enumerate(rm.points) if KF2 in mp["mObservations"]][::2]
    for p in dropped[:4]:
        rm.points[p]["mpRefKF"] = KF2                                  # the drop moves their reference keyframe
    src, dst = str(tmp_path / "map.txt"), str(tmp_path / "out.txt")
    write_map(src, rm, first_kf, current_kf, recent, KF2, dropped)
    subprocess.run([os.path.join(INTEG, "build", "point_erase_shim_test"), src, dst], check=True, capture_output=True, timeout=60)
    got = parse(dst)
    assert set(got) == {("store", "cull"), ("store", "drop"), ("host", "cull"), ("host", "drop")}
    action, c = rm.cull(recent, [first_kf[p] for p in recent], current_kf)
    assert set(action.tolist()) == {0, 1, 2, 3} and c["n_records"] > 0
    stays = [p for p, a in zip(recent, action) if a == 0]
    want = restated(rm, stays)
    for route in ("store", "host"):
        assert got[(route, "cull")] == want, route
    status, c = rm.erase_observations(dropped, [KF2] * len(dropped), erase_match=True)
    assert c["n_ref_moved"] > 0 and c["n_set_bad"] > 0 and 1 in status.tolist() and 2 in status.tolist()
    want = restated(rm, stays)
    for route in ("store", "host"):
        assert got[(route, "drop")] == want, route
    assert got[("store", "drop")] != got[("store", "cull")]
