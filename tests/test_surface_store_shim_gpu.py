"""The resident-Surface shim (integration/surface_store_hip.h) compiled against stand-in KeyFrame / MapPoint types and run on the device:
one keyframe goes through the normals, Shape from Normals, the surface registration and the template switch by the store route
(InitSurfaceStoreHIP, twice ObtainK1K2StoreHIP, ShapeFromNormalsStoreHIP, RegisterSurfacesStoreHIP, UpdateTemplateHIP: no Surface and no
surface point on the host) and by the host route (a Surface per keyframe on the host, the normals downloaded and set in the reference's
order, obtainM's walk over the objects, dsh_sfn_estimate on host arrays, the same two shims uploading the host points, applyScale on the
host).  Both leave the same normals, flags, counts, surface points and depth spline in every keyframe, the same registration, pose and
template vertices, and the same map points after the switch.  Bit patterns."""
import os

import numpy as np
import pytest

import shim_run
import store_model
from surface_register_ref import RegisterModel

INTEG = shim_run.INTEG
BBS = (-0.6, 0.6, 13, -0.6, 0.6, 15)


def test_shim_compiles_against_the_c_abi():
    shim_run.build()
    assert os.path.exists(shim_run.exe("surfstore_shim_test"))
    src = open(os.path.join(INTEG, "surface_store_hip.h")).read()
    for name in ("dsh_keyframe_surface_init", "dsh_keyframe_surface_gather", "dsh_normals_estimate_db", "dsh_keyframe_surface_take_normals", "dsh_keyframe_sfn"):
        assert name in src
    for other in ("surface_register_store_hip.h", "template_switch_hip.h"):         # they serve a keyframe whose Surface is in the store
        assert "dsh_keyframe_surface_state" in open(os.path.join(INTEG, other)).read()
    assert "defslam_hip_debug.h" not in src and "dsh_lab" not in src


def make_scene(seed=0, n_points=100, N1=120, N2=150):
    """Three keyframes: slot 0 a small one, slot 1 the keyframe under test (the reference keyframe of every point, which it holds at a
    random entry), slot 2 the second keyframe of every DiffProp record.  Some entries of slot 1 are empty, one point is bad, and the
    records of a point go to key points of slot 2 that other records name too (the later normal stays).  The points lie in the world
    at depth 1.3 behind the keyframe's key points; the surface of the scene's normals is unrelated to them (check_chi is off)."""
    from defslam_amd import synth
    rng = np.random.default_rng(seed)
    g = synth.make_normals_scene(n_points=n_points, n_views=2, seed=seed + 3, nonref_frac=0.0)
    m = RegisterModel()
    entry = rng.permutation(N1)[:n_points]
    t1, t2 = [-1] * N1, [-1] * N2
    kpn = [rng.uniform(-0.4, 0.4, (5, 2)), rng.uniform(-0.4, 0.4, (N1, 2)), rng.uniform(-0.4, 0.4, (N2, 2))]
    Twc = np.eye(4)
    Twc[:3, :3], Twc[:3, 3] = synth._rodrigues(np.array([0.05, -0.03, 0.02])), [0.1, -0.05, 0.2]
    Twc = Twc.astype(np.float32)
    for p in range(n_points):
        cam = 1.3 * np.array([g["ref_uv"][p, 0], g["ref_uv"][p, 1], 1.0]) + rng.normal(0, 0.01, 3)
        m.add_point(xyz=Twc[:3, :3].astype(np.float64) @ cam + Twc[:3, 3], bad=p == 7, ref=1, desc=rng.integers(0, 256, 32, dtype=np.uint8))
        t1[entry[p]] = p
        kpn[1][entry[p]] = g["ref_uv"][p]
    levels, sf = 4, (1.2 ** np.arange(4)).astype(np.float32)
    for t, Ow in (([0, 1, -1, 2, -1], (0.0, 0.0, 0.0)), (t1, Twc[:3, 3]), (t2, (0.3, 0.0, 0.1))):
        m.add_keyframe(t, Ow=Ow, desc=rng.integers(0, 256, (len(t), 32), dtype=np.uint8), octave=rng.integers(0, levels, len(t)), scale_factors=sf)
    for p in range(n_points):
        assert m.add_observation(p, 1, int(entry[p]))
    R = g["recs"].shape[0]
    rec_point = np.repeat(np.arange(n_points), np.diff(g["rec_ptr"]))
    rec_idx2 = rng.integers(0, N2 // 2, R)                                           # half of slot 2: repeats
    order = rng.permutation(R)                                                      # the database groups them by point again
    todo = [p for p in rng.permutation(n_points).tolist() if p != 7][:n_points - 10]
    fl = lambda v: " ".join(repr(float(x)) for x in np.asarray(v, np.float32).reshape(-1))
    lines = [f"1 {BBS[0]!r} {BBS[1]!r} {BBS[2]} {BBS[3]!r} {BBS[4]!r} {BBS[5]} 0.001 1.0"]
    lines += [fl(x) for k in kpn for x in k]
    lines += [str(R)] + [f"{rec_point[r]} 2 {rec_idx2[r]} {fl(g['recs'][r])}" for r in order]
    lines += [str(len(todo)), " ".join(str(p) for p in todo)]
    rows, cols = 120, 160
    px = np.stack([kpn[1][:, 0] * 0.625 * cols + cols / 2, kpn[1][:, 1] * 0.625 * cols + rows / 2], 1)
    assert (px[:, 0] > 0).all() and (px[:, 0] < cols - 1).all() and (px[:, 1] > 0).all() and (px[:, 1] < rows - 1).all()
    facets = [p for p in range(n_points) if p % 9 != 4]                              # some points had no facet when the keyframe was made
    u = rng.random(n_points + n_points * n_points)
    lines += [f"{rows} {cols} 9 8 0.05 0", fl(Twc)] + [fl(x) for x in px]
    lines += [str(len(facets)), " ".join(str(p) for p in facets), str(len(u)), " ".join(repr(float(x)) for x in u)]
    return m, "\n".join(lines) + "\n", len(todo)


def _parse(path):
    out = {}
    for ln in open(path).read().splitlines():
        w = ln.split()
        key = (w[0], w[1]) if w[1] != "kf" else (w[0], "kf", int(w[2]), w[3])
        out[key] = [int(x) for x in (w[2:] if w[1] != "kf" else w[4:])]
    return out


@pytest.mark.gpu
def test_store_route_and_host_route_leave_the_same_surfaces(tmp_path):
    shim_run.build()
    m, tail, n_todo = make_scene()
    src, dst = str(tmp_path / "map.txt"), str(tmp_path / "out.txt")
    store_model.write_scene(m, src, tail)
    shim_run.run("surfstore_shim_test", src, dst)
    got = _parse(dst)
    assert got[("store", "sfn")] == got[("host", "sfn")]
    ret, n_sites, n_empty, n_bad, n_no_normal, n_nan, ok = got[("store", "sfn")]
    assert ret == ok == 1 and n_sites >= 50 and n_empty == 20 and n_bad == 1 and n_sites + n_no_normal == 99 and n_nan == 0
    solved, propagated = got[("store", "solved")]
    assert 50 <= solved <= n_sites and propagated >= 10
    for k in range(3):
        for kind in ("counts", "normal", "on", "x3D", "depth"):
            assert got[("store", "kf", k, kind)] == got[("host", "kf", k, kind)], (k, kind)
    assert got[("store", "kf", 1, "counts")] == [n_sites, 13 * 15] and got[("store", "kf", 0, "counts")] == [0, 0]
    n2, d2 = got[("store", "kf", 2, "counts")]
    assert d2 == 0 and 10 <= n2 == sum(got[("store", "kf", 2, "on")]) <= 75         # repeated targets were counted once
    x3D = np.array(got[("store", "kf", 1, "x3D")], np.uint32).view(np.float32).reshape(-1, 3)
    assert np.isfinite(x3D).all() and np.median(x3D[:, 2]) > 0
    # the registration and the switch: the store route read and scaled the resident Surface, the keyframe object held no surface point
    assert got[("store", "host_surface_points")] == [0]
    for kind in ("register", "sim3", "s22", "kf_Tcw", "kf_Twc", "vertices", "switch", "xyz", "point_normal", "max_distance", "nodes", "bary"):
        assert got[("store", kind)] == got[("host", kind)], kind
    ret, n_pairs, _, n_bad, n_no_facet, n_no_snapshot, registered = got[("store", "register")]
    assert ret == registered == 1 and n_pairs >= 80 and n_bad == 1 and n_no_facet + n_no_snapshot >= 1
    s22 = np.array(got[("store", "s22")], np.uint64).view(np.float64)[0]
    # No range for s22 follows from the scene: its normals come from an independent random plane per point (synth.make_normals_scene),
    # so the integrated surface is not the map's and the similarity found is arbitrary; check_chi is off for that reason.
    assert np.isfinite(s22) and s22 > 0
    n_new, _, n_moved, _, n_embedded, n_points = got[("store", "switch")]
    assert n_moved == 99 and n_points == 100 + n_new and n_embedded >= 1
