"""The keyframe-create shim (integration/keyframe_create_hip.h) compiled against stand-in Frame / KeyFrame / MapPoint types and run on
the device: for the end of one tracked frame that becomes a keyframe, its map point upkeep and its connections, the store route
(EndTrackedFrameHIP with CreateNewKeyFrameStoreHIP, ProcessNewKeyFrameStoreHIP, UpdateConnectionsStoreHIP) and the host route (the
reference's loops written out over the objects) leave every mutated field identical -- the frame, the new keyframe's table, centre and
snapshot, the points, the connection members of every keyframe, parent and children -- and both equal the restatement
(tests/keyframe_create_ref.py).  Floats are compared as bit patterns."""
import copy
import os

import numpy as np
import pytest

import keyframe_create_ref as KC
import keyframe_insert_ref as KI
import shim_run
import store_model
from surface_register_ref import centre_of

INTEG = shim_run.INTEG


class Model(KC.CreateModel, KI.StoreModel):
    pass


def test_shim_compiles_against_the_c_abi():
    shim_run.build()
    assert os.path.exists(shim_run.exe("keyframe_create_shim_test"))
    src = open(os.path.join(INTEG, "keyframe_create_hip.h")).read()
    assert "dsh_keyframe_create" in src and "dsh_keyframe_update_connections" in src and "defslam_hip_debug.h" not in src and "dsh_lab" not in src


def parse_more(path):
    """The lines of the driver beyond StoreScene::dump -> {route: dict(frame, centre, snap, conn)}."""
    out = {}
    for ln in open(path).read().splitlines():
        w = ln.split()
        if len(w) < 3 or w[2] not in ("frame", "centre", "snap", "conn"):
            continue
        d = out.setdefault(w[0], {"conn": []})
        if w[2] == "frame":
            d["frame"] = [int(x) for x in w[3:]]
        elif w[2] == "centre":
            d["centre"] = [int(x) for x in w[3].split(":")]
        elif w[2] == "snap":
            d["snap"] = [tuple(int(x) for x in e.split(":")) for e in w[3:]]
        else:
            head, counted, ordered, children = " ".join(w[3:]).split("|")
            k, first, parent = (int(x) for x in head.split())
            assert k == len(d["conn"])
            pairs = lambda s: [tuple(int(x) for x in e.split(":")) for e in s.split()]
            d["conn"].append(dict(first=bool(first), parent=parent, counted=dict(pairs(counted)), ordered=pairs(ordered), children=[int(x) for x in children.split()]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("seed,th", [(3, 2), (8, 100)])
def test_store_route_host_route_and_restatement_agree(tmp_path, seed, th):
    shim_run.build()
    N = 60
    m, d = KC.create_scene(N, seed=seed, K_old=4, N_old=8, P=40, cls=Model)
    for pt in m.points:
        pt.ref = max(pt.ref, 0)                             # the host route's dsh_mappoint_update needs a reference keyframe
    scene = copy.deepcopy(m)                                # with the empty keyframe the driver constructs the new one in
    scene.add_keyframe([], Ow=np.zeros(3, np.float32), desc=np.zeros((0, 32), np.uint8), octave=np.zeros(0, np.int32), scale_factors=np.ones(1, np.float32))
    fl = lambda v: " ".join(repr(float(x)) for x in np.asarray(v, np.float32).reshape(-1))
    emb = sorted(m.facet)
    tail = f"{th} {len(emb)}\n" + " ".join(str(p) for p in emb) + f"\n{N}\n"
    for i in range(N):
        tail += f"{int(d['frame_points'][i])} {int(d['outlier'][i])} {int(d['octave'][i])} {fl(d['kpn'][i])} " + " ".join(str(int(b)) for b in d["desc"][i]) + "\n"
    tail += f"{len(d['scale_factors'])} {fl(d['scale_factors'])}\n{fl(d['Tcw'])}\n"
    src, dst = str(tmp_path / "map.txt"), str(tmp_path / "out.txt")
    store_model.write_scene(scene, src, tail)
    shim_run.run("keyframe_create_shim_test", src, dst)
    got, more = store_model.parse_dump(dst), parse_more(dst)
    assert set(got) == {("store", "kf"), ("host", "kf")} and set(more) == {"store", "host"}
    # the restatement
    cand = m.end_frame_candidate(d["frame_points"])
    slot = m.create(d["desc"], d["octave"], d["scale_factors"], d["Tcw"], kpn=d["kpn"])["slot"]
    action, added, _ = m.process_new_keyframe(slot)
    recent = [p for p, a in zip(m.kfs[slot].table, action) if a == KI.RECENT]
    con = m.update_connections(slot, th)
    assert slot == 4 and len(added) >= 5 and con["parent_set"] and (len(con["ordered_kf"]) > 1) == (th == 2)
    want = store_model.dump_of(m, recent)
    pt, xyz = m.get_snapshot(slot)
    conn = [dict(first=True, parent=k.parent, counted={}, ordered=[], children=[]) for k in m.kfs]
    conn[slot].update(first=False, counted=dict(zip(con["counted_kf"], con["counted_w"])), ordered=list(zip(con["ordered_kf"], con["ordered_w"])))
    conn[con["parent"]]["children"] = [slot]
    for k, w in zip(con["ordered_kf"], con["ordered_w"]):   # AddConnection on the listed keyframes
        conn[k].update(counted={slot: w}, ordered=[(slot, w)])
    want_more = dict(frame=[-1 if o else c for c, o in zip(cand, d["outlier"])], centre=centre_of(d["Tcw"]).view(np.uint32).tolist(),
                     snap=[(i, int(p)) + tuple(xyz[i].view(np.uint32).tolist()) for i, p in enumerate(pt) if p >= 0], conn=conn)
    assert want_more["snap"] and any(o and c >= 0 for c, o in zip(cand, d["outlier"]))
    for route in ("store", "host"):
        assert got[(route, "kf")] == want, route
        for k in want_more:
            assert more[route][k] == want_more[k], (route, k)
