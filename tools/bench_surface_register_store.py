"""Timing of dsh_keyframe_register against dsh_surface_register on ready host clouds: a keyframe of N = 1200 key points with 600 pairs
(tests/surface_register_ref.make_scene), host wall time around calls that end in a stream synchronise.  Prints one JSON line.
    python tools/bench_surface_register_store.py [reps]                  (profiles/surface_register_store/README.md has the numbers)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import surface_register_ref as SR   # noqa: E402
from defslam_amd import localmap, mappoint, register, sft   # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
sc = SR.make_scene(1200, seed=7, n_pairs=600)
m, slot = sc["model"], sc["slot"]
ctx = sft.Context(0)
st = localmap.MapPointStore(ctx)
ks = mappoint.KeyFrameStore(ctx, 4)
SR.fill_store(m, st, ks)
t0 = time.perf_counter()
taken = st.snapshot_positions(slot)
t_snap_first = time.perf_counter() - t0
assert taken == m.snapshot_positions(slot)
SR.apply_after(m, sc, st)
c, idx, surf, mp = m.select(slot, sc["surface_pts"], sc["Twc"])
assert c["n_pairs"] == 600


def timed(fn, n):
    for _ in range(max(5, n // 10)):
        fn()
    t = []
    for _ in range(n):
        a = time.perf_counter()
        fn()
        t.append(time.perf_counter() - a)
    t = np.array(t) * 1e6
    return dict(median_us=float(np.median(t)), p10_us=float(np.percentile(t, 10)), p90_us=float(np.percentile(t, 90)))


store = lambda: st.register_surface(ks, slot, sc["surface_pts"], sc["Twc"], sc["u"], 0.05)
host = lambda: register.registerSurfaces(ctx, surf, mp, sc["u"], sc["Twc"], 0.05)
clouds = lambda: st.register_clouds(slot, sc["surface_pts"], sc["Twc"])
g, r = store(), host()
assert g.registered and r["registered"] and g.sim3.tobytes() == r["sim3"].tobytes()
out = dict(N=1200, n_pairs=600, reps=reps, snapshot_first_call_us=t_snap_first * 1e6, keyframe_register=timed(store, reps),
           surface_register_host_clouds=timed(host, reps), keyframe_register_clouds=timed(clouds, reps))
out["ratio_store_over_host"] = out["keyframe_register"]["median_us"] / out["surface_register_host_clouds"]["median_us"]
print(json.dumps(out))
ctx.close()
