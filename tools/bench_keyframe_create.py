"""Timing of the creation of a keyframe on the resident stores and of its connections.
  create        dsh_keyframe_create of a keyframe of 1200 key points, about 600 held, from the resident keyframe candidate, against the
                four calls it stands for (dsh_kfdb_add, dsh_mpdb_add_keyframe with the table handed over from the host,
                dsh_keyframe_snapshot_positions, dsh_keyframe_surface_init) on a second pair of stores filled alike
  connections   dsh_keyframe_update_connections of a keyframe of 1200 key points in a map of 10, 100 and 1000 keyframes with 600
                observation records each, beside dsh_local_map_update of the same table on the same store (it makes the same sweep)
Host wall time around calls that end in a stream synchronise, the two sides of every comparison alternating in one loop, medians after
warm-up.  Kernel times come from a run of their own under rocprofv3 --kernel-trace --stats (the kernels are kc_*_kernel and
sr_snapshot_kernel).  Prints one JSON line.
    python tools/bench_keyframe_create.py [reps]                  (profiles/keyframe_create/README.md has the numbers)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import keyframe_create_ref as KC   # noqa: E402
from defslam_amd import localmap, mappoint, sft   # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
ctx = sft.Context(0)


def alternating(fns, n):
    """Every function once per round, n rounds after n / 10 warm-up rounds: {name: median / p10 / p90 in us}."""
    t = {k: [] for k in fns}
    for r in range(max(5, n // 10) + n):
        for k, fn in fns.items():
            a = time.perf_counter()
            fn()
            if r >= max(5, n // 10):
                t[k].append(time.perf_counter() - a)
    return {k: dict(median_us=float(np.median(v) * 1e6), p10_us=float(np.percentile(v, 10) * 1e6), p90_us=float(np.percentile(v, 90) * 1e6)) for k, v in t.items()}


# ---- creation: the one call against the four ----
N = 1200
m, d = KC.create_scene(N, seed=1, P=4000)
cand = np.array(m.end_frame_candidate(d["frame_points"]), np.int32)
nodes, bary = np.array([0, 1, 2], np.int32), np.array([0.2, 0.3, 0.5])


def pair():
    s, k = localmap.MapPointStore(ctx, points=4096, keyframes=1024), mappoint.KeyFrameStore(ctx, 1024)
    m.fill(s, k)
    ids = sorted(m.facet)
    s.set_embedding(ids, np.tile(nodes, (len(ids), 1)), np.tile(bary, (len(ids), 1)))
    s.end_frame(d["frame_points"], d["outlier"], d["octave"])
    return s, k


a, ka = pair()
b, kb = pair()
kf = mappoint.MpKeyFrame(np.zeros(3, np.float32), d["desc"], d["octave"], d["scale_factors"])
Ow = a.create_keyframe(ka, kf, d["Tcw"], kpn=d["kpn"]).Ow
kf4 = mappoint.MpKeyFrame(Ow, d["desc"], d["octave"], d["scale_factors"])


def one_call():
    return a.create_keyframe(ka, kf, d["Tcw"], kpn=d["kpn"]).slot


def four_calls():
    kb.add(kf4)
    s = b.add_keyframe(cand)                       # the hand-over of points_out: the table goes up from the host
    b.snapshot_positions(s)
    b.surface_init(s, d["kpn"])
    return s


four_calls()
sa, sb = one_call(), four_calls()
assert sa == sb and a.keyframe_table(sa).tolist() == b.keyframe_table(sb).tolist() and a.get_snapshot(sa)[1].tobytes() == b.get_snapshot(sb)[1].tobytes()
out = dict(reps=reps, create=dict(N=N, n_held=int((cand >= 0).sum()), **alternating(dict(keyframe_create=one_call, four_calls=four_calls), reps)))
out["ratio_create_over_four_calls"] = out["create"]["keyframe_create"]["median_us"] / out["create"]["four_calls"]["median_us"]
for s in (a, ka, b, kb):
    s.close()

# ---- connections beside the local map update of the same table ----
out["connections"] = []
for K in (10, 100, 1000):
    rng = np.random.default_rng(K)
    P = max(2000, 100 * K)
    st = localmap.MapPointStore(ctx, points=P, keyframes=K + 1, observations=600 * K + 1200)
    st.add_points(rng.normal(0, 1, (P, 3)).astype(np.float32), np.tile(np.float32([0, 0, 1]), (P, 1)), np.ones(P, np.float32), np.zeros((P, 32), np.uint8))
    for k in range(K):
        table = np.full(N, -1, np.int32)
        idx = rng.permutation(N)[:600]
        # a keyframe sees points near its own place in the map: the neighbours in slot order share some
        table[idx] = (rng.permutation(2000)[:600] + (k * (P - 2000)) // max(K - 1, 1)).astype(np.int32)
        assert st.add_keyframe(table) == k
        st.add_observations(table[idx], np.full(600, k, np.int32), idx=idx)
    table = np.full(N, -1, np.int32)
    table[rng.permutation(N)[:600]] = (rng.permutation(2000)[:600] + (P - 2000)).astype(np.int32)
    slot = st.add_keyframe(table)
    r = st.update_connections(slot, 100)
    t = alternating(dict(update_connections=lambda: st.update_connections(slot, 100), local_map_update=lambda: st.update_local_map(table)), reps)
    out["connections"].append(dict(K=K, records=600 * K, n_counted=len(r.counted_kf), n_connected=len(r.ordered_kf), **t))
    st.close()
print(json.dumps(out))
ctx.close()
