"""The keyframe-insert shim (integration/keyframe_insert_hip.h) compiled against stand-in KeyFrame / MapPoint types and run on the device:
for one new keyframe and one repose upkeep the store route (ProcessNewKeyFrameStoreHIP, ReposeUpkeepStoreHIP: one call each, results
written back on the objects) and the host route (the loop over the objects and dsh_mappoint_update) leave every mutated field of every
map point identical -- observations, nObs, descriptor, normal, max and min distance, the recent list -- and both equal the restatement
(tests/keyframe_insert_ref.py).  Floats are compared as bit patterns."""
import os

import numpy as np
import pytest

import keyframe_insert_ref as KI
import shim_run
import store_model

INTEG = shim_run.INTEG


def test_shim_compiles_against_the_c_abi():
    shim_run.build()
    assert os.path.exists(shim_run.exe("keyframe_insert_shim_test"))
    src = open(os.path.join(INTEG, "keyframe_insert_hip.h")).read()
    assert "dsh_keyframe_process_new" in src and "dsh_point_store_upkeep" in src and "defslam_hip_debug.h" not in src and "dsh_lab" not in src


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [3, 8])
def test_store_route_host_route_and_restatement_agree(tmp_path, seed):
    shim_run.build()
    m, slot = KI.random_model(seed, K=8, N=6, P=20, p_obs=0.8)
    for pt in m.points:
        pt.ref = max(pt.ref, 0)                             # the host route's dsh_mappoint_update needs a reference keyframe
    m.erase_observation(*[(r[0], r[1]) for r in m.log if r[1] != slot][0])      # a blanked record in the log
    rng = np.random.default_rng(seed)
    emb = [int(p) for p in rng.permutation(20)[:9]]
    emb_xyz = (rng.normal(0, 1, (9, 3)) + [0, 0, 5]).astype(np.float32)
    src, dst = str(tmp_path / "map.txt"), str(tmp_path / "out.txt")
    store_model.write_scene(m, src, f"{slot} {len(emb)}\n" + "".join(f"{p} " + " ".join(repr(float(v)) for v in x) + "\n" for p, x in zip(emb, emb_xyz)))
    shim_run.run("keyframe_insert_shim_test", src, dst)
    got = store_model.parse_dump(dst)
    assert set(got) == {("store", "new"), ("store", "repose"), ("host", "new"), ("host", "repose")}
    action, added, _ = m.process_new_keyframe(slot)
    recent = [p for p, a in zip(m.kfs[slot].table, action) if a == KI.RECENT]
    assert len(added) >= 2 and recent
    want = store_model.dump_of(m, recent)
    for route in ("store", "host"):
        assert got[(route, "new")] == want, route
    # min = max / mvScaleFactors[levels - 1] in float, on the objects of the store route too
    p = added[0]
    sf = m.kfs[m.points[p].ref].scale_factors
    assert np.float32(m.points[p].min_distance) == np.float32(m.points[p].max_distance) / sf[len(sf) - 1] and m.points[p].min_distance > 0
    for q, x in zip(emb, emb_xyz):
        m.points[q].xyz = x
    has_facet = [q in emb for q in range(20)]
    ids = m.embedded_ids(has_facet)
    assert 0 < len(ids) <= len(emb)
    m.upkeep(ids, KI.NORMAL_DEPTH)
    want = store_model.dump_of(m)
    for route in ("store", "host"):
        assert got[(route, "repose")] == want, route
    written = lambda step: [b[3:] for b in got[("store", step)]["bits"]]      # normal, max and min distance: not the position embed() sets
    assert written("repose") != written("new")
