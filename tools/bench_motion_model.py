"""End-to-end cost of TrackWithMotionModel from the resident store (dsh_motion_model_search) against the host-packed way of the same
search, on one scene: 1200 key points in the current frame, a last frame of 1200 key points that holds about 400 points.

  store      MapPointStore.motion_model_search: one upload of the frame's key points, the gather from the store, the grid, the narrow
             search (the wide one is enqueued behind it and leaves at once), one download
  packed     what the frame did before: Python packs position, octave and descriptor of every query from host copies of the points
             (the filter of DefORBmatcher.cc:325-332 included, vectorised with numpy), then dsh_search_by_projection_frame uploads them with the frame
Both are timed by the host clock around the Python call (each call ends in a stream synchronise inside the library), in --rounds rounds
that alternate --reps calls of one and of the other after warm-up calls of both; per round the median, over the rounds the median and the
spread (min, max) of those medians.  The two ways must return the same matches; the tool checks that first and fails otherwise.
Prints one JSON object (and writes it to --out).  One process, no retry, and an alarm ends it after --timeout seconds.  The device time of the kernels alone comes from a kernel
trace of this tool (rocprofv3 --kernel-trace --stats, in a run of its own); --summarize-trace prints its per-kernel medians.
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from defslam_amd import localmap, sft, synth, track  # noqa: E402


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


def last_frame(sc, held=400):
    """The frame before: the scene's final frame, filled up to about `held` held key points with points the current frame has no key
    point for (they are searched and find nothing)."""
    rng = np.random.default_rng(11)
    fp = sc["final_points"].copy()
    free = np.nonzero(fp < 0)[0]
    more = max(0, held - int((fp >= 0).sum()))
    fp[rng.choice(free, min(more, free.shape[0]), replace=False)] = rng.integers(0, sc["xyz"].shape[0], min(more, free.shape[0]))
    return fp.astype(np.int32), sc["outlier"], sc["frame"].arrays()["octave"]


def packed_call(ctx, frame, host, ids, octave):
    """The host-packed way: the filter and the packing per query in Python, then the packed search."""
    held = np.nonzero(ids >= 0)[0]
    p = ids[held]
    ok = ~host["bad"][p] & (host["nodes"][p, 0] >= 0)
    keep, p = held[ok], p[ok]
    return keep, track.SearchByProjectionFrame(ctx, frame, track.FrameQueries(host["xyz"][p], octave[keep], host["desc"][p]), 20.0)


def summarize_trace(path):
    """Per-kernel medians of a `rocprofv3 --kernel-trace --output-format csv` trace of this tool."""
    import csv
    import re
    durs = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            m = re.search(r"\b(mm_\w+|trk_\w+)", row["Kernel_Name"])
            if m:
                durs.setdefault(m.group(1), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return [dict(kernel=k, calls=len(v), median_us=round(float(np.median(v)), 2), max_us=round(float(np.max(v)), 2)) for k, v in sorted(durs.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarize-trace", metavar="CSV", default="")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--store-only", action="store_true", help="time the store call alone (for a kernel trace)")
    ap.add_argument("--out", default="")
    ap.add_argument("--timeout", type=int, default=300, help="seconds after which the process ends itself")
    a = ap.parse_args()
    signal.alarm(a.timeout)
    if a.summarize_trace:
        for r in summarize_trace(a.summarize_trace):
            print(json.dumps(r))
        return
    sc = synth.make_track_close_scene(300)
    ctx = sft.Context(0)
    st = fill(ctx, sc)
    pts, out, octs = last_frame(sc)
    e = st.end_frame(pts, out, octs)
    lf = st.last_frame()
    frame = sc["frame"]
    empty = track.TrackFrame(**{**frame.__dict__, "state": None})
    host = dict(xyz=sc["xyz"], desc=sc["desc"], bad=sc["bad"], nodes=sc["nodes"])
    g = st.motion_model_search(frame)
    keep, h = packed_call(ctx, empty, host, lf.ids, lf.octave)
    if g.th_used != 20.0 or g.match[keep].tobytes() != h.match.tobytes() or g.nmatches != h.nmatches:
        raise SystemExit("the store call and the packed call disagree")
    ways = dict(store=lambda: st.motion_model_search(frame))
    if not a.store_only:
        ways["packed"] = lambda: packed_call(ctx, empty, host, lf.ids, lf.octave)
    for call in ways.values():
        for _ in range(20):
            call()
    med = {k: [] for k in ways}
    for _ in range(a.rounds):
        for k, call in ways.items():
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                call()
                t.append(1e6 * (time.perf_counter() - t0))
            med[k].append(float(np.median(t)))
    res = dict(tool="bench_motion_model", reps=a.reps, rounds=a.rounds, frame_keypoints=int(g.frame_points.shape[0]), last_frame_keypoints=int(lf.ids.shape[0]),
               held=int(e.kept), queries=len(keep), nmatches=int(g.nmatches), upload_bytes_store=768 + 44 * int(g.frame_points.shape[0]),
               upload_bytes_packed=512 + 44 * int(g.frame_points.shape[0]) + 68 * len(keep))   # two / one frame records, 44 per key point, 68 per query
    for k, v in med.items():
        res[k + "_us"] = dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1), rounds=[round(x, 1) for x in v])
    st.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
