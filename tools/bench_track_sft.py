"""End-to-end cost of Shape-from-Template of a tracked frame from the resident store (dsh_track_sft) against the path it replaces, at
two sizes: the reference's default (10 x 10 template, 1200 key points, about 450 rows) and C2 (25 x 20 template, 1200 key points, about
1000 rows).  Scenes of tests/track_sft_ref.py: holes, five outliers on entry, three bad points, four points without a facet, one id
held twice.

  parent     what a caller did before: a ready host table into dsh_sft_solve, the scatter of its flags, then close_frame(node_xyz),
             which moves the points.  The table is built before the clock starts (the parent builds it from host objects, which is not
             timed here); the whole-store get_embedding it needs once per template switch to be able to is timed on its own.
  store      MapPointStore.sft(write_back=True), then close_frame(node_xyz=None).
Both are timed by the host clock around the Python calls (each ends in a stream synchronise inside the library), --reps calls of each way
in --rounds alternating rounds after three warm-up calls; over all calls of a way the median and the spread (min, 10th and 90th
percentile, max).  The store way's node positions must equal the parent's bit for bit; the tool checks that first and fails otherwise.
Prints one JSON object per size (and appends them to --out).  One process, no retry, and an alarm ends it after --timeout seconds.  The
kernel time of the selection comes from a kernel trace of this tool (rocprofv3 --kernel-trace, in a run of its own, with --device-only);
--summarize-trace prints the kernel's calls and medians per grid size.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from defslam_amd import localmap, sft, synth, track  # noqa: E402

SIZES = dict(default=dict(rows=10, cols=10, N=1200, n_rows=450), C2=dict(rows=25, cols=20, N=1200, n_rows=1000))
REGS = (synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
KERNEL = "tf_select_kernel"


def summarize_trace(path):
    """Calls and median duration of the selection kernel per grid size in a `rocprofv3 --kernel-trace --output-format csv` trace."""
    import csv
    durs = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            if KERNEL in row["Kernel_Name"]:
                grid = int(row.get("Grid_Size_X", row.get("Grid_Size", 0))) // 256
                durs.setdefault(grid, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return [dict(kernel=KERNEL, workgroups=g, calls=len(v), median_us=round(float(np.median(v)), 2), min_us=round(float(np.min(v)), 2),
                 max_us=round(float(np.max(v)), 2)) for g, v in sorted(durs.items())]


def spread(t):
    t = np.asarray(t)
    return dict(median=round(float(np.median(t)), 1), min=round(float(t.min()), 1), p10=round(float(np.percentile(t, 10)), 1),
                p90=round(float(np.percentile(t, 90)), 1), max=round(float(t.max()), 1), calls=int(t.shape[0]))


def run_size(name, a):
    import track_sft_ref as R
    kw = SIZES[name]
    sc = R.make_scene(seed=0, **kw)
    ctx = sft.Context(0)
    ctx.template_build(sc.tmpl.xyz0, sc.tmpl.facets)
    st = localmap.MapPointStore(ctx)
    sc.model.fill(st)
    P, N = len(sc.model.points), len(sc.frame_points)
    st.seed_local_points(np.arange(P))
    t = R.select(sc.model, sc.kp, sc.octave, R.INV_LEVEL_SIGMA2, sc.frame_points, sc.outlier)
    sf, logsf = track.orb_pyramid(R.LEVELS)
    octave = np.where(sc.frame_points >= 0, sc.octave, 0)

    def close(Tcw, flags, node_xyz):
        fr = track.TrackFrame(Tcw=Tcw, K=np.asarray(sc.K, np.float32), bounds=np.array([0, 640, 0, 480], np.float32), kp=sc.kp, octave=octave,
                              desc=desc, scale_factors=sf, log_scale_factor=float(logsf))
        return st.close_frame(fr, sc.frame_points, flags, node_xyz)

    desc = np.zeros((N, 32), np.uint8)
    f = sft.Frame(Tcw=sc.Tcw.copy(), K=sc.K.copy(), N=N, obs_nodes=t.nodes, obs_bary=t.bary, obs_uv=t.uv, obs_invsig2=t.invsig2, nodes_xyz=sc.xyz.copy())
    solve = ctx.prepare_solve(f, *REGS)

    def parent():
        solve()                      # from the frame's pose and nodes as they were when the call was prepared
        return f.nodes_xyz, close(f.Tcw, R.scatter(sc.outlier, t, f.mvbOutlier), f.nodes_xyz)

    def store():
        g = st.sft(sc.Tcw, sc.K, sc.kp, sc.octave, R.INV_LEVEL_SIGMA2, sc.frame_points, sc.xyz, outlier=sc.outlier, write_back=True, RegLap=REGS[0],
                   RegInex=REGS[1], RegTemp=REGS[2])
        return g.xyz, close(g.Tcw, g.outlier, None)

    (xa, ca), (xb, cb) = parent(), store()
    if xa.tobytes() != xb.tobytes() or any(getattr(ca, k) != getattr(cb, k) for k in ca.__dataclass_fields__ if k != "n_moved"):
        raise SystemExit(f"{name}: the store way and the parent's path disagree")
    ways = dict(store=store) if a.device_only else dict(parent=parent, store=store, parent_get_embedding_per_switch=lambda: st.get_embedding())
    for call in ways.values():
        for _ in range(3):
            call()
    times = {k: [] for k in ways}
    for _ in range(a.rounds):
        for k, call in ways.items():
            for _ in range(max(a.reps // a.rounds, 1)):
                t0 = time.perf_counter()
                call()
                times[k].append(1e6 * (time.perf_counter() - t0))
    res = dict(tool="bench_track_sft", size=name, template_nodes=sc.tmpl.n, keypoints=N, rows=int(len(t.kp_index)), store_points=P, lm_iterations=int(f.iters),
               lm_trials=int(f.trials), inliers=int(ca.inliers), frame_upload_bytes_store_way=17 * N + 4 * R.LEVELS, table_download_bytes_store_way=8 + 68 * N,
               table_bytes_parent=60 * int(len(t.kp_index)), embedding_readback_bytes_per_switch=36 * P)
    for k, v in times.items():
        res[k + "_us"] = spread(v)
    st.close()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarize-trace", metavar="CSV", default="")
    ap.add_argument("--reps", type=int, default=40, help="timed calls of each way (at least 30 for a figure to report)")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--sizes", default="default,C2")
    ap.add_argument("--device-only", action="store_true", help="run the store way alone (for a kernel trace)")
    ap.add_argument("--out", default="")
    ap.add_argument("--timeout", type=int, default=300, help="seconds after which the process ends itself")
    a = ap.parse_args()
    signal.alarm(a.timeout)
    if a.summarize_trace:
        for r in summarize_trace(a.summarize_trace):
            print(json.dumps(r))
        return
    for name in a.sizes.split(","):
        line = json.dumps(run_size(name, a))
        print(line)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
