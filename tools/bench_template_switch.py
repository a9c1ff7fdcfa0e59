"""Cost of a template switch on the resident store (dsh_template_switch) against the route the calls before it offer.

  size       the reference's default: a 640 x 480 keyframe with 1200 key points on the default store of tools/bench_local_map.py (30
             keyframes x 1200 key points, 8 observations per point), a 10 x 10 template.  Two scenes: "default" (held key points all over
             the image: the 32-pixel boxes mask almost everything, few new points) and "exploring" (held key points in the left half)
  device     HIP events on dsh_stream around MapPointStore.switch_template (one upload, three launches, one download) and host wall time
             of the Python call: medians of --reps calls after three warm-up calls.  Every call runs on a store refilled from the scene
             (a switch changes the store: the new points are held afterwards); the refill is not timed
  composed   the same switch from the earlier calls: CreateNewMapPoints restated on the host (numpy: the mask as an image, the positions;
             dsh_mappoint_update for the new points' normal and depth), dsh_mpdb_add_points + dsh_mpdb_add_observations +
             dsh_mpdb_set_keyframe_point, dsh_mpdb_update_points of the moved points, dsh_trackstate_get of all positions,
             dsh_template_embed_device, dsh_trackstate_set_embedding, dsh_trackstate_repose.  Host wall time of the whole route
  bytes      what crosses PCIe per switch, both ways (computed from the sizes)
Prints one JSON object (and writes it to --out).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from defslam_amd import _lib, localmap, mappoint, nrsfm, sft, synth  # noqa: E402

SCENES = {"default": dict(half=False), "exploring": dict(half=True)}
SIZE = dict(rows=480, cols=640, n_kp=1200, n_kf=30, obs_per_point=8)
GRID = (10, 10)


def fill(st, sc):
    st.clear()
    st.add_points(sc["xyz"], sc["normal"], sc["max_distance"], sc["desc"], sc["bad"])
    for k in range(sc["tables"].shape[0]):
        st.add_keyframe(sc["tables"][k], sc["parents"][k], sc["kf_bad"][k])
    st.add_observations(sc["obs_point"], sc["obs_kf"])


def reflect101(p, n):
    return np.where(p < 0, -p, np.where(p >= n, 2 * (n - 1) - p, p))


def host_create_new_map_points(sc):
    """DefLocalMapping.cc:240-347 on arrays: (moved ids, their positions, new key point indices, their positions)."""
    r, rows, cols = sc["ref_slot"], sc["rows"], sc["cols"]
    table, bad = sc["tables"][r], sc["bad"]
    px, py = sc["kp"][:, 0].astype(np.int64), sc["kp"][:, 1].astype(np.int64)
    held = (table >= 0) & ~bad[np.maximum(table, 0)]
    k = cols // 20
    a = k // 2
    src = np.zeros((rows, cols), bool)
    src[py[held], px[held]] = True
    d = np.arange(-a, k - a)
    along_x = src[:, reflect101(np.arange(cols)[:, None] + d, cols)].any(axis=2)
    mask = along_x[reflect101(np.arange(rows)[:, None] + d, rows), :].any(axis=1)
    new = np.nonzero((table < 0) & ~mask[py, px])[0]
    T = sc["Twc"]
    s = sc["surface_pts"]
    w = np.stack([((T[i, 0] * s[:, 0] + T[i, 1] * s[:, 1]) + T[i, 2] * s[:, 2]) + T[i, 3] for i in range(3)], 1).astype(np.float32)
    hi = np.nonzero(held)[0]
    return table[hi], w[hi], new, w[new]


def composed_switch(ctx, st, ks, sc):
    r = sc["ref_slot"]
    moved_ids, moved_xyz, new_idx, new_xyz = host_create_new_map_points(sc)
    st.clear_embedding()
    n_new = new_idx.shape[0]
    if n_new:
        u = mappoint.update(ctx, ks, new_xyz, [[(r, int(i))] for i in new_idx], [r] * n_new)
        first = st.add_points(new_xyz, u.normal, u.max_distance, sc["kf_desc"][r][new_idx])
        st.add_observations(np.arange(first, first + n_new), np.full(n_new, r))
        for j, i in enumerate(new_idx):
            st.set_keyframe_point(r, int(i), first + j)
    uniq, last = np.unique(moved_ids[::-1], return_index=True)                      # a point held twice keeps the later position
    st.update_points(uniq, xyz=moved_xyz[::-1][last])
    P = st.n_points
    xyz = st.get_state().xyz
    good = np.nonzero(~np.concatenate([sc["bad"], np.zeros(P - sc["bad"].shape[0], bool)]))[0]
    fid, nodes, bary = ctx.template_embed_device(xyz[good])
    hit = fid >= 0
    order = np.argsort(nodes[hit], axis=1, kind="stable")
    st.set_embedding(good[hit], np.take_along_axis(nodes[hit], order, 1), np.take_along_axis(bary[hit], order, 1).astype(np.float64))
    st.repose(sc["nodes_new"])
    return dict(n_new=int(n_new), n_moved=int(moved_ids.shape[0]), n_embedded=int(hit.sum()), n_points=int(P))


def run_scene(ctx, ev, sc, reps):
    stream = ctx._L.dsh_stream(ctx._h)
    K = sc["tables"].shape[0]
    ks = mappoint.KeyFrameStore(ctx, K)
    for k in range(K):
        ks.add(mappoint.MpKeyFrame(sc["kf_Ow"][k], sc["kf_desc"][k], sc["kf_octave"][k], sc["scale_factors"], bool(sc["kf_bad"][k])))
    sc["nodes_new"] = nrsfm.surface_vertices(ctx, nrsfm.Bbs(*sc["bbs"]), sc["depth_ctrl"], sc["Twc"], *GRID)
    ctx.template_build(sc["nodes_new"], synth.regular_triangulation(*GRID))
    st = localmap.MapPointStore(ctx, points=sc["xyz"].shape[0] + sc["kp"].shape[0], keyframes=K, observations=sc["obs_point"].shape[0] + sc["kp"].shape[0])
    kf = localmap.KeyFramePoints(sc["rows"], sc["cols"], sc["kp"])
    ev_ms, wall_ms, comp_ms = [], [], []
    g = c = None
    for i in range(reps + 3):
        fill(st, sc)
        t0 = time.perf_counter()
        ev.start(stream)
        g = st.switch_template(ks, sc["ref_slot"], kf, sc["surface_pts"], sc["Twc"])
        e = ev.stop_ms(stream)
        t1 = time.perf_counter()
        fill(st, sc)
        t2 = time.perf_counter()
        c = composed_switch(ctx, st, ks, sc)
        t3 = time.perf_counter()
        if i >= 3:
            ev_ms.append(e)
            wall_ms.append(1e3 * (t1 - t0))
            comp_ms.append(1e3 * (t3 - t2))
    same = (g.n_new, g.n_moved, g.n_embedded, g.n_points) == (c["n_new"], c["n_moved"], c["n_embedded"], c["n_points"])
    N, P, n_nodes, F = int(sc["kp"].shape[0]), int(g.n_points), int(sc["nodes_new"].shape[0]), int(synth.regular_triangulation(*GRID).shape[0])
    out = dict(key_points=N, points_after=P, n_new=g.n_new, n_moved=g.n_moved, n_masked=g.n_masked, n_embedded=g.n_embedded, routes_agree=bool(same),
               device_event_us_median=1e3 * float(np.median(ev_ms)), device_wall_us_median=1e3 * float(np.median(wall_ms)),
               composed_wall_us_median=1e3 * float(np.median(comp_ms)))
    # the switch: key points, surface points, octaves, Twc, scale factors and the template up; the counts and new_idx down
    out["device_bytes_up"] = 8 * N + 12 * N + N + 64 + 128 + 24 * n_nodes + 12 * F + 4 * (n_nodes + 1) + 12 * F + 32
    out["device_bytes_down"] = 32 + 4 * N
    # the composed route: new points (xyz, normal, max distance, descriptor, ids), moved points (id, xyz), all positions down and up
    # again for the embedding, the embedding down (facet, nodes, float barycentrics) and up (id, nodes, double barycentrics)
    good = P - int(sc["bad"].sum())
    out["composed_bytes_up"] = g.n_new * (12 + 12 + 4 + 32 + 8 + 4) + g.n_moved * 16 + 12 * good + g.n_embedded * (4 + 12 + 24) + 24 * n_nodes
    out["composed_bytes_down"] = 12 * P + good * (4 + 12 + 12) + g.n_new * (12 + 4 + 4 + 32)
    st.close()
    ks.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scenes", default="default,exploring")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = sft.Context(0)
    ev = _lib.HipEvents()
    res = dict(tool="bench_template_switch", reps=a.reps, size=SIZE, grid=GRID)
    for name in a.scenes.split(","):
        sc = synth.make_template_switch_scene(400, **SIZE, **SCENES[name])                # the same map, the held key points placed differently
        res[name] = run_scene(ctx, ev, sc, a.reps)
    ev.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
