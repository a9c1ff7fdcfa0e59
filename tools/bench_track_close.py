"""Cost of closing a tracked frame on the resident store (dsh_track_close_frame) against the host's way of ending the same frame.

  sizes      those of tools/bench_local_map.py: default (30 keyframes x 1200 key points, 8 observations per point), 300 keyframes, 500
             observations per point
  device     HIP events on dsh_stream around MapPointStore.close_frame (upload, at most three launches, the 32-byte download) and host wall
             time of the Python call: medians of --reps calls after three warm-up calls
  host       the integration driver (integration/build/trackclose_shim_test, a child process) times, over stand-in objects of the same
             scene: CloseTrackedFrameHIP (write-backs on the host objects included), and how the frame ended before the store held the
             embedding -- DefMapPoint::RecalculatePosition of every facet point on the host, dsh_mpdb_update_points of all of them, the loops
             of DefTracking.cc:253-319 over the pointer graph.  C++ wall times
  upload     bytes that travel up per frame, both ways (computed from the sizes)
Prints one JSON object (and writes it to --out).  The device time of the kernels alone comes from a kernel trace of this tool
(rocprofv3 --kernel-trace --stats, with --no-driver); --summarize-trace prints its per-kernel medians.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from defslam_amd import _lib, localmap, sft, synth  # noqa: E402

SIZES = {"default": dict(n_kf=30, n_kp=1200, obs_per_point=8),
         "kf300": dict(n_kf=300, n_kp=1200, obs_per_point=8),
         "obs500": dict(n_kf=600, n_kp=1200, obs_per_point=500)}
DRIVER = os.path.join(ROOT, "integration", "build", "trackclose_shim_test")


def previous_frame_points(sc):
    """What the frame before held: points from a third of the map earlier, so that its local list is another one."""
    fp = sc["frame_points"]
    return np.where(fp >= 0, np.maximum(fp - sc["xyz"].shape[0] // 3, 0), -1).astype(np.int32)


def fill(ctx, sc):
    st = localmap.MapPointStore(ctx)
    st.add_points(sc["xyz"], sc["normal"], sc["max_distance"], sc["desc"], sc["bad"])
    for k in range(sc["tables"].shape[0]):
        st.add_keyframe(sc["tables"][k], sc["parents"][k], sc["kf_bad"][k])
    st.add_observations(sc["obs_point"], sc["obs_kf"])
    P = sc["xyz"].shape[0]
    st.set_counters(np.arange(P), sc["visible"], sc["found"])
    st.set_embedding(np.arange(P), sc["nodes"], sc["bary"])
    return st


def device_leg(ctx, ev, sc, reps):
    stream = ctx._L.dsh_stream(ctx._h)
    st = fill(ctx, sc)
    st.update_local_map(previous_frame_points(sc))
    g = st.update_local_map(sc["frame_points"])
    st.search_local_points(sc["frame"], g.n_local_points, 3.0)
    call = lambda: st.close_frame(sc["frame_after"], sc["final_points"], sc["outlier"], sc["node_xyz"])
    for _ in range(3):
        call()
    ev_ms, wall_ms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        ev.start(stream)
        c = call()
        ev_ms.append(ev.stop_ms(stream))
        wall_ms.append(1e3 * (time.perf_counter() - t0))
    P, N, n_nodes = int(sc["xyz"].shape[0]), int(sc["final_points"].shape[0]), int(sc["node_xyz"].shape[0])
    out = dict(points=P, facet_points=int(c.n_moved), frame_keypoints=N, template_nodes=n_nodes, local_map_points=int(c.local_map_points),
               matches_inliers=int(c.matches_inliers), event_us_median=1e3 * float(np.median(ev_ms)), wall_us_median=1e3 * float(np.median(wall_ms)))
    # per frame, up: the pose block, 5 bytes per key point and 24 per node; the host's way sends an id and a position per facet point
    out["upload_bytes_close"] = 512 + 5 * N + 24 * n_nodes
    out["upload_bytes_positions"] = 16 * int(c.n_moved)
    st.close()
    return out


def driver_leg(sc, reps):
    with tempfile.TemporaryDirectory() as d:
        synth.write_local_map_scene(sc, os.path.join(d, "map.txt"))
        synth.write_track_close_scene(sc, previous_frame_points(sc), os.path.join(d, "close.txt"))
        r = subprocess.run(["timeout", "-k", "10", "300", DRIVER, os.path.join(d, "map.txt"), os.path.join(d, "close.txt"), os.path.join(d, "out.txt"), "0",
                            os.path.join(d, "t.json"), str(reps)], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"trackclose_shim_test failed ({r.returncode}): {r.stderr}")
        t = json.load(open(os.path.join(d, "t.json")))
    t["host_close_ms"] = t["host_repose_ms"] + t["host_upload_ms"] + t["host_loops_ms"]
    return t


def summarize_trace(path):
    """Per-kernel medians of a `rocprofv3 --kernel-trace --output-format csv` trace of this tool."""
    import csv
    import re
    durs = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            m = re.search(r"\b(tc_\w+|lm_\w+|trk_\w+)", row["Kernel_Name"])
            if m:
                durs.setdefault(m.group(1), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return [dict(kernel=k, calls=len(v), median_us=round(float(np.median(v)), 2), max_us=round(float(np.max(v)), 2)) for k, v in sorted(durs.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarize-trace", metavar="CSV", default="")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sizes", default="default,kf300,obs500")
    ap.add_argument("--no-driver", action="store_true", help="skip the integration driver (the host comparison)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.summarize_trace:
        for r in summarize_trace(a.summarize_trace):
            print(json.dumps(r))
        return
    ctx = sft.Context(0)
    ev = _lib.HipEvents()
    res = dict(tool="bench_track_close", reps=a.reps)
    for i, name in enumerate(a.sizes.split(",")):
        sc = synth.make_track_close_scene(300 + i, **SIZES[name])
        res[name] = device_leg(ctx, ev, sc, a.reps)
        if not a.no_driver:
            res[name]["driver"] = driver_leg(sc, a.reps)
    ev.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
