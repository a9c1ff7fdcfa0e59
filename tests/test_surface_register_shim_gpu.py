"""The surface registration shim (integration/surface_register_store_hip.h) compiled against stand-in KeyFrame / MapPoint types and run on
the device: for one keyframe the store route (SnapshotKeyFrameStoreHIP, RegisterSurfacesStoreHIP: one call each, applyScale and SetPose
written back on the keyframe object) and the host route (DefKeyFrame's constructor loop, the walk of SurfaceRegistration.cc:60-104 over
the objects, dsh_surface_register on the host clouds) yield the same counts, the same Sim(3), scale and pose and leave the same surface
points, pose and camera centre on the keyframe, and both equal the restatement (tests/surface_register_ref.py).  Bit patterns."""
import os

import numpy as np
import pytest

import shim_run
import store_model
import surface_register_ref as SR
from test_surface_register_store_cpu import register_scene

INTEG = shim_run.INTEG


def test_shim_compiles_against_the_c_abi():
    shim_run.build()
    assert os.path.exists(shim_run.exe("surfreg_shim_test"))
    src = open(os.path.join(INTEG, "surface_register_store_hip.h")).read()
    assert "dsh_keyframe_snapshot_positions" in src and "dsh_keyframe_register" in src and "defslam_hip_debug.h" not in src and "dsh_lab" not in src


def _tail(sc, chi_limit, check_chi):
    fl = lambda v: " ".join(repr(float(x)) for x in np.asarray(v).reshape(-1))
    m = sc["model"]
    lines = [f"{sc['slot']} {chi_limit!r} {int(check_chi)}", fl(sc["Twc"])] + [fl(s) for s in sc["surface_pts"]]
    lines += [str(len(m.facet)), " ".join(str(p) for p in sorted(m.facet))]
    ops = []
    for op in sc["after"]:
        if op[0] == "move":
            ops += [f"move {p} {fl(x)}" for p, x in zip(op[1], op[2])]
        elif op[0] == "table":
            ops.append(f"table {op[1]} {op[2]}")
        else:
            ops.append(f"{op[0]} {op[1]}")
    lines += [str(len(ops))] + ops + [str(len(sc["u"])), " ".join(repr(float(v)) for v in sc["u"])]
    return "\n".join(lines) + "\n"


def _parse(path):
    out = {}
    for ln in open(path).read().splitlines():
        w = ln.split()
        out[(w[0], w[1])] = [int(x) for x in w[2:]]
    return out


def _f32(v):
    return np.array(v, np.uint32).view(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("n_pairs,chi_limit,check_chi", [(40, 0.05, True), (40, 1e-6, True), (40, 1e-6, False), (14, 0.05, True)])
def test_store_route_host_route_and_restatement_agree(tmp_path, n_pairs, chi_limit, check_chi):
    shim_run.build()
    sc = register_scene(n_pairs)
    m, slot = sc["model"], sc["slot"]
    src, dst = str(tmp_path / "map.txt"), str(tmp_path / "out.txt")
    store_model.write_scene(m, src, _tail(sc, chi_limit, check_chi))
    shim_run.run("surfreg_shim_test", src, dst)
    got = _parse(dst)
    kinds = ("taken", "counts", "sim3", "s22", "info", "Tcw_new", "kf_Tcw", "kf_Twc", "kf_Ow", "surface")
    for k in kinds:
        assert got[("store", k)] == got[("host", k)], k
    taken = m.snapshot_positions(slot)
    SR.apply_after(m, sc)
    c, idx, surf, mp = m.select(slot, sc["surface_pts"], sc["Twc"])
    registered = n_pairs >= 15 and (chi_limit > 1e-3 or not check_chi)
    assert got[("store", "taken")] == [taken]
    assert got[("store", "counts")] == [c[k] for k in SR.COUNT_NAMES] + [int(registered)] * 2
    Tcw = _f32(got[("store", "Tcw_new")]).reshape(4, 4)
    s22 = np.array(got[("store", "s22")], np.uint64).view(np.float64)[0]
    if registered:
        assert abs(s22 - 1.35) < 0.05                                               # the scene's similarity
        assert _f32(got[("store", "surface")]).tobytes() == SR.apply_scale(sc["surface_pts"], s22).tobytes()
        assert _f32(got[("store", "kf_Ow")]).tobytes() == SR.centre_of(Tcw).tobytes() == _f32(got[("store", "centre")]).tobytes()
        assert _f32(got[("store", "kf_Tcw")]).tobytes() == Tcw.tobytes()
        assert _f32(got[("store", "kf_Twc")]).reshape(4, 4)[:3, :3].tobytes() == np.ascontiguousarray(Tcw[:3, :3].T).tobytes()
    else:
        assert _f32(got[("store", "surface")]).tobytes() == sc["surface_pts"].tobytes()
        assert _f32(got[("store", "kf_Ow")]).tobytes() == _f32(got[("store", "centre")]).tobytes() == np.asarray(m.kfs[slot].Ow, np.float32).tobytes()
        assert _f32(got[("store", "kf_Twc")]).tobytes() == sc["Twc"].tobytes() and not Tcw.any()
