"""The keyframe-insert shim (integration/keyframe_insert_hip.h) compiled against stand-in KeyFrame / MapPoint types and run on the device:
for one new keyframe and one repose upkeep the store route (ProcessNewKeyFrameStoreHIP, ReposeUpkeepStoreHIP: one call each, results
written back on the objects) and the host route (the loop over the objects and dsh_mappoint_update) leave every mutated field of every
map point identical -- observations, nObs, descriptor, normal, max and min distance, the recent list -- and both equal the restatement
(tests/keyframe_insert_ref.py).  Floats are compared as bit patterns."""
import os
import subprocess

import numpy as np
import pytest

import keyframe_insert_ref as KI
from conftest import ROOT

INTEG = os.path.join(ROOT, "integration")


def test_shim_compiles_against_the_c_abi():
    subprocess.run(["make", "-C", INTEG], check=True, capture_output=True)
    assert os.path.exists(os.path.join(INTEG, "build", "keyframe_insert_shim_test"))
    src = open(os.path.join(INTEG, "keyframe_insert_hip.h")).read()
    assert "dsh_keyframe_process_new" in src and "dsh_point_store_upkeep" in src and "defslam_hip_debug.h" not in src and "dsh_lab" not in src


def write_map(path, m, slot, emb, emb_xyz):
    with open(path, "w") as f:
        f.write(f"{len(m.xyz)} {len(m.kfs)}\n")
        for p in range(len(m.xyz)):
            nums = [int(m.bad[p]), m.ref[p]] + [repr(float(v)) for v in m.xyz[p]] + [repr(float(v)) for v in m.normal[p]] + [repr(float(m.max_distance[p]))]
            f.write(" ".join(map(str, nums + m.desc[p].tolist())) + "\n")
        for s, k in enumerate(m.kfs):
            f.write(" ".join(map(str, [len(m.tables[s]), int(k.bad)] + [repr(float(v)) for v in k.Ow] + [len(k.scale_factors)] +
                                 [repr(float(v)) for v in k.scale_factors])) + "\n")
            for j, t in enumerate(m.tables[s]):
                f.write(" ".join(map(str, [int(k.octave[j]), t] + k.desc[j].tolist())) + "\n")
        f.write(f"{len(m.log)}\n" + "".join(f"{p} {s} {i} {int(live)}\n" for p, s, i, live in m.log))
        f.write(f"{slot} {len(emb)}\n" + "".join(f"{p} " + " ".join(repr(float(v)) for v in x) + "\n" for p, x in zip(emb, emb_xyz)))


def parse(path):
    """(route, step) -> dict(recent=[ids], pts={id: (n_obs, max bits, min bits, normal bits x 3, desc bytes, {slot: idx})})"""
    out = {}
    for line in open(path):
        w = line.split()
        r = out.setdefault((w[0], w[1]), dict(recent=None, pts={}))
        if w[2] == "recent":
            r["recent"] = [int(x) for x in w[3:]]
        else:
            head, obs = line.split("|")
            h = head.split()
            r["pts"][int(h[3])] = (int(h[4]), int(h[5]), int(h[6]), tuple(int(x) for x in h[7:10]), bytes(int(x) for x in h[10:42]),
                                   {int(a.split(":")[0]): int(a.split(":")[1]) for a in obs.split()})
    return out


def model_points(m):
    u32 = lambda v: int(np.float32(v).view(np.uint32))
    return {p: (m.n_obs[p], u32(m.max_distance[p]), u32(m.min_distance[p]), tuple(u32(v) for v in m.normal[p]), m.desc[p].tobytes(),
                dict(m.observations(p))) for p in range(len(m.xyz))}


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [3, 8])
def test_store_route_host_route_and_restatement_agree(tmp_path, seed):
    subprocess.run(["make", "-C", INTEG], check=True, capture_output=True)
    m, slot = KI.random_model(seed, K=8, N=6, P=20, p_obs=0.8)
    m.ref = [max(r, 0) for r in m.ref]                      # the host route's dsh_mappoint_update needs a reference keyframe
    m.erase_observation(*[(r[0], r[1]) for r in m.log if r[1] != slot][0])      # a blanked record in the log
    rng = np.random.default_rng(seed)
    emb = [int(p) for p in rng.permutation(20)[:9]]
    emb_xyz = (rng.normal(0, 1, (9, 3)) + [0, 0, 5]).astype(np.float32)
    src, dst = str(tmp_path / "map.txt"), str(tmp_path / "out.txt")
    write_map(src, m, slot, emb, emb_xyz)
    # the min distance the model starts from is what the objects start from
    for p in range(20):
        m.min_distance[p] = np.float32(0)
    subprocess.run([os.path.join(INTEG, "build", "keyframe_insert_shim_test"), src, dst], check=True, capture_output=True, timeout=60)
    got = parse(dst)
    assert set(got) == {("store", "new"), ("store", "repose"), ("host", "new"), ("host", "repose")}
    action, added, _ = m.process_new_keyframe(slot)
    recent = [p for p, a in zip(m.tables[slot], action) if a == KI.RECENT]
    assert len(added) >= 2 and recent
    want = model_points(m)
    for route in ("store", "host"):
        assert got[(route, "new")]["recent"] == recent, route
        assert got[(route, "new")]["pts"] == want, route
    # min = max / mvScaleFactors[levels - 1] in float, on the objects of the store route too
    p = added[0]
    sf = m.kfs[m.ref[p]].scale_factors
    assert np.float32(m.min_distance[p]) == np.float32(m.max_distance[p]) / sf[len(sf) - 1] and m.min_distance[p] > 0
    for q, x in zip(emb, emb_xyz):
        m.xyz[q] = x
    has_facet = [q in emb for q in range(20)]
    ids = m.embedded_ids(has_facet)
    assert 0 < len(ids) <= len(emb)
    m.upkeep(ids, KI.NORMAL_DEPTH)
    want = model_points(m)
    for route in ("store", "host"):
        assert got[(route, "repose")]["pts"] == want, route
    assert got[("store", "repose")]["pts"] != got[("store", "new")]["pts"]
