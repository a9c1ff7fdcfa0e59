"""Cost of the local map from the resident store (dsh_local_map_update, dsh_local_map_search) against the host's way of doing the same frame.

  sizes      default (30 keyframes x 1200 key points, 8 observations per point), 300 keyframes, 500 observations per point
  device     HIP events on dsh_stream around each call (upload, launches, download) and host wall time of the Python mirror: medians of
             --reps calls after three warm-up calls
  host       the integration driver (integration/build/localmap_shim_test, a child process) times, over stand-in objects of the same
             scene: (a) UpdateLocalKeyFrames + UpdateLocalPoints with std::map / std::set on the host, then SearchLocalPointsHIP, which
             re-packs and uploads every local point -- how the frame was done before the store; (b) UpdateLocalMapHIP +
             SearchLocalPointsStoreHIP.  Both are C++ wall times of whole calls, write-backs included
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
DRIVER = os.path.join(ROOT, "integration", "build", "localmap_shim_test")


def fill(ctx, sc):
    st = localmap.MapPointStore(ctx)
    st.add_points(sc["xyz"], sc["normal"], sc["max_distance"], sc["desc"], sc["bad"])
    for k in range(sc["tables"].shape[0]):
        st.add_keyframe(sc["tables"][k], sc["parents"][k], sc["kf_bad"][k])
    st.add_observations(sc["obs_point"], sc["obs_kf"])
    return st


def device_legs(ctx, ev, sc, reps):
    stream = ctx._L.dsh_stream(ctx._h)
    st = fill(ctx, sc)
    g = st.update_local_map(sc["frame_points"])
    legs = {}
    for name, call in (("update", lambda: st.update_local_map(sc["frame_points"])),
                       ("search", lambda: st.search_local_points(sc["frame"], g.n_local_points, 3.0))):
        for _ in range(3):
            call()
        ev_ms, wall_ms = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            ev.start(stream)
            r = call()
            ev_ms.append(ev.stop_ms(stream))
            wall_ms.append(1e3 * (time.perf_counter() - t0))
        legs[name] = dict(event_us_median=1e3 * float(np.median(ev_ms)), wall_us_median=1e3 * float(np.median(wall_ms)))
    legs["search"]["matches"] = r.nmatches
    N, Q = int(sc["frame_points"].shape[0]), int(g.n_local_points)
    held = sc["frame_points"][sc["frame_points"] >= 0]
    obs_of = np.bincount(sc["obs_point"], minlength=sc["xyz"].shape[0])
    out = dict(keyframes=int(sc["tables"].shape[0]), points=int(sc["xyz"].shape[0]), observations=int(sc["obs_point"].shape[0]), frame_keypoints=N,
               held_points=int(held.shape[0]), votes_cast=int(obs_of[held][~sc["bad"][held]].sum()), local_keyframes=int(len(g.local_kf)), local_points=Q,
               **legs)
    out["pair_event_us"] = legs["update"]["event_us_median"] + legs["search"]["event_us_median"]
    # per frame, up: the store way sends the frame's ids and key points; the re-pack way sends the key points and 64 bytes per local point
    # (position 12, normal 12, max distance 4, descriptor 32, skip flag 4) -- dsh_track.cpp also sends a 4-byte problem index per query
    frame_bytes = 256 + N * (8 + 4 + 32)
    out["upload_bytes_store"] = 4 * N + frame_bytes
    out["upload_bytes_repack"] = frame_bytes + Q * (12 + 12 + 4 + 4 + 32 + 4)
    st.close()
    return out


def driver_leg(sc, reps):
    with tempfile.TemporaryDirectory() as d:
        synth.write_local_map_scene(sc, os.path.join(d, "in.txt"))
        r = subprocess.run(["timeout", "-k", "10", "300", DRIVER, os.path.join(d, "in.txt"), os.path.join(d, "out.txt"), "0", os.path.join(d, "t.json"), str(reps)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"localmap_shim_test failed ({r.returncode}): {r.stderr}")
        t = json.load(open(os.path.join(d, "t.json")))
        t["host_way_equal"] = int(open(os.path.join(d, "out.txt")).read().split()[-1])
    t["host_frame_ms"] = t["host_update_ms"] + t["host_repack_search_ms"]
    t["store_frame_ms"] = t["store_update_ms"] + t["store_search_ms"]
    return t


def summarize_trace(path):
    """Per-kernel medians of a `rocprofv3 --kernel-trace --output-format csv` trace of this tool."""
    import csv
    import re
    durs = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            m = re.search(r"\b(lm_\w+|trk_\w+)", row["Kernel_Name"])
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
    res = dict(tool="bench_local_map", reps=a.reps)
    for i, name in enumerate(a.sizes.split(",")):
        sc = synth.make_local_map_scene(300 + i, **SIZES[name])
        res[name] = device_legs(ctx, ev, sc, a.reps)
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
