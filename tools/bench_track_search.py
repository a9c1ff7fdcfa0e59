"""Cost of the tracking searches (dsh_search_by_projection_*) on the device.

  per frame  TrackWithMotionModel's frame-to-frame search (th = 20) and SearchLocalPoints' local-map search (th = 3) of one frame,
             at the reference's default size (1200 key points, ~400 last-frame points, ~300 local points) and at 2000 key points /
             1500 queries: HIP events on dsh_stream around each call (upload, three launches, download) and host wall time
  batched    frames/s of B = 16 / 256 / 4096 frames per call (both searches of every frame, two calls)
  rescans    the fraction of queries phase B had to search again
Prints one JSON object (and writes it to --out).  The device time of the kernels alone comes from a kernel trace of this tool
(rocprofv3 --kernel-trace --stats); profiles/README.md lists both.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from defslam_amd import _lib, sft, synth, track  # noqa: E402


def scenes(n, n_kp, n_fq, n_lq, seed0=100):
    return [synth.make_track_scene(seed0 + i, n_kp=n_kp, n_frame_q=n_fq, n_local_q=n_lq) for i in range(n)]


def per_frame(ctx, ev, sc, reps):
    st = ctx._L.dsh_stream(ctx._h)
    out = {}
    for name, items in (("frame_th20", [(sc["frame"], sc["fq"], 20)]), ("local_th3", [(sc["frame"], sc["lq"], 3)])):
        for _ in range(3):
            track.search_batch(ctx, items)
        ev_ms, wall_ms = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            ev.start(st)
            r = track.search_batch(ctx, items)[0]
            ev_ms.append(ev.stop_ms(st))
            wall_ms.append(1e3 * (time.perf_counter() - t0))
        out[name] = dict(Q=int(len(r.match)), matches=r.nmatches, rescans=r.rescans, event_us_median=1e3 * float(np.median(ev_ms)),
                         wall_us_median=1e3 * float(np.median(wall_ms)))
    out["pair_event_us"] = out["frame_th20"]["event_us_median"] + out["local_th3"]["event_us_median"]
    out["pair_wall_us"] = out["frame_th20"]["wall_us_median"] + out["local_th3"]["wall_us_median"]
    return out


def batched(ctx, ev, pool, B, reps):
    st = ctx._L.dsh_stream(ctx._h)
    fr = [(pool[i % len(pool)]["frame"], pool[i % len(pool)]["fq"], 20) for i in range(B)]
    lo = [(pool[i % len(pool)]["frame"], pool[i % len(pool)]["lq"], 3) for i in range(B)]
    track.search_batch(ctx, fr)
    track.search_batch(ctx, lo)
    ev_ms, wall_s, resc, nq = [], [], 0, 0
    for _ in range(reps):
        t0 = time.perf_counter()
        ev.start(st)
        a = track.search_batch(ctx, fr)
        b = track.search_batch(ctx, lo)
        ev_ms.append(ev.stop_ms(st))
        wall_s.append(time.perf_counter() - t0)
        resc += sum(r.rescans for r in a + b)
        nq += sum(len(r.match) for r in a + b)
    return dict(B=B, frames_per_s_event=B / (1e-3 * float(np.median(ev_ms))), frames_per_s_wall=B / float(np.median(wall_s)), rescan_fraction=resc / max(nq, 1))


def summarize_trace(path):
    """Per-call kernel time from a `rocprofv3 --kernel-trace --output-format csv` trace of this tool: every call launches
    trk_cells_kernel, trk_search_kernel (when it has queries) and trk_resolve_kernel; grouped by the cells kernel's grid (B frames)."""
    import csv
    calls = []
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            dur = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
            if "trk_cells_kernel" in name:
                calls.append(dict(B=int(row["Grid_Size_X"]) // 1024, cells=dur, search=0.0, resolve=0.0))
            elif calls and "trk_search_kernel" in name:
                calls[-1]["search"] = dur
            elif calls and "trk_resolve_kernel" in name:
                calls[-1]["resolve"] = dur
    # the tool's order: 3 warm-up + reps calls per single-frame leg (default frame, default local, large frame, large local), then batches
    out, i, lead = [], 0, 0
    while lead < len(calls) and calls[lead]["B"] == 1:
        lead += 1
    n_leg = lead // 4
    for leg in ("default frame-to-frame", "default local map", "large frame-to-frame", "large local map"):
        seg = calls[i + 3:i + n_leg]
        i += n_leg
        med = {k: float(np.median([c[k] for c in seg])) for k in ("cells", "search", "resolve")}
        out.append(dict(leg=leg, calls=len(seg), **{k + "_us": round(v, 1) for k, v in med.items()}, total_us=round(sum(med.values()), 1)))
    by_b = {}
    for c in calls[i:]:
        by_b.setdefault(c["B"], []).append(c)
    for B, seg in sorted(by_b.items()):
        med = {k: float(np.median([c[k] for c in seg])) for k in ("cells", "search", "resolve")}
        out.append(dict(leg=f"batch of {B} frames", calls=len(seg), **{k + "_us": round(v, 1) for k, v in med.items()}, total_us=round(sum(med.values()), 1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarize-trace", metavar="CSV", default="", help="print the per-call kernel times of a kernel trace of this tool and exit")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch-reps", type=int, default=5)
    ap.add_argument("--batches", default="16,256,4096")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.summarize_trace:
        for r in summarize_trace(a.summarize_trace):
            print(json.dumps(r))
        return
    ctx = sft.Context(0)
    ev = _lib.HipEvents()
    res = dict(tool="bench_track_search")
    default = scenes(16, 1200, 400, 300)
    large = scenes(4, 2000, 1500, 1500, seed0=200)
    res["default_size"] = per_frame(ctx, ev, default[0], a.reps)
    res["large_size"] = per_frame(ctx, ev, large[0], a.reps)
    res["batched_default_size"] = [batched(ctx, ev, default, int(B), a.batch_reps) for B in a.batches.split(",")]
    resc = sum(r.rescans for s in default for r in track.search_batch(ctx, [(s["frame"], s["fq"], 20), (s["frame"], s["lq"], 3)]))
    nq = sum(len(s["fq"].xyz) + len(s["lq"].xyz) for s in default)
    res["rescan_fraction_default"] = resc / nq
    ev.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
