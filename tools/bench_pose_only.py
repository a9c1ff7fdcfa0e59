"""End-to-end cost of the rigid pose-only optimisation from the resident store (dsh_track_pose_only, dsh_track_pose_only_batch) against
the host path it replaces, on one store: frames of 1200 key points that hold 450 points (the reference's default size), 10 % of them
displaced grossly.

  device     MapPointStore.pose_only: one upload of the frame, one launch, one download; and pose_only_batch of 8 and of 64 frames
  host       what a caller of the store did before: dsh_point_store_get_points for the held ids, then the single-thread sequential
             restatement of the optimiser (tests/pose_only_ref.py, NumPy) on the positions read back.  The read-back alone is reported
             too: a compiled solver would replace the NumPy part, not the read-back.
All are timed by the host clock around the Python call (each call ends in a stream synchronise inside the library), in --rounds rounds
that alternate --reps calls of each way after warm-up calls; per round the median, over the rounds the median and the spread (min, max)
of those medians.  The device result must equal the restatement's decisions; the tool checks that first and fails otherwise.  Prints
one JSON object (and writes it to --out).  One process, no retry, and an alarm ends it after --timeout seconds.  The device time of the
kernel alone comes from a kernel trace of this tool (rocprofv3 --kernel-trace, in a run of its own, with --device-only);
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

from defslam_amd import localmap, sft  # noqa: E402

BATCHES = (8, 64)


def summarize_trace(path):
    """Calls and median duration of po_solve_kernel per grid size in a `rocprofv3 --kernel-trace --output-format csv` trace, and the
    number of other kernels between its first and its last call."""
    import csv
    durs, other, seen = {}, {}, False
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    last = max((i for i, r in enumerate(rows) if "po_solve_kernel" in r["Kernel_Name"]), default=-1)
    for i, row in enumerate(rows):
        if "po_solve_kernel" in row["Kernel_Name"]:
            seen = True
            grid = int(row.get("Grid_Size_X", row.get("Grid_Size", 0))) // 256
            durs.setdefault(grid, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        elif seen and i < last:
            name = row["Kernel_Name"].split("(")[0][:60]
            other[name] = other.get(name, 0) + 1
    return [dict(kernel="po_solve_kernel", problems=g, calls=len(v), median_us=round(float(np.median(v)), 2), min_us=round(float(np.min(v)), 2),
                 max_us=round(float(np.max(v)), 2)) for g, v in sorted(durs.items())] + [dict(other_kernels_between_its_calls=other)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarize-trace", metavar="CSV", default="")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device-only", action="store_true", help="time the device calls alone (for a kernel trace)")
    ap.add_argument("--out", default="")
    ap.add_argument("--timeout", type=int, default=300, help="seconds after which the process ends itself")
    a = ap.parse_args()
    signal.alarm(a.timeout)
    if a.summarize_trace:
        for r in summarize_trace(a.summarize_trace):
            print(json.dumps(r))
        return
    import pose_only_ref as R
    model, fr, _ = R.make_case(**R.GPU_CASES["default450of1200"])
    ctx = sft.Context(0)
    st = localmap.MapPointStore(ctx)
    model.fill(st)
    held = np.unique(fr.frame_points[fr.frame_points >= 0]).astype(np.int32)
    frame = localmap.PoseOnlyFrame(fr.Tcw, fr.K, fr.kp, fr.octave, fr.inv_level_sigma2, fr.frame_points)

    def host_call():
        xyz = np.zeros((st.n_points, 3), np.float32)
        xyz[held] = st.get_points(held).xyz
        return R.solve(None, fr, "sequential", xyz=xyz)

    g, h = st.pose_only(fr.Tcw, fr.K, fr.kp, fr.octave, fr.inv_level_sigma2, fr.frame_points), host_call()
    if (g.outlier.tobytes() != h.outlier.tobytes() or g.iters[:g.rounds].tolist() != [r.iters for r in h.rounds] or
            np.abs(g.pose - h.pose).max() > R.POSE_TOL):
        raise SystemExit("the device call and the host path disagree")
    ways = dict(device_1=lambda: st.pose_only_batch([frame]))
    for B in BATCHES:
        ways[f"device_{B}"] = lambda B=B: st.pose_only_batch([frame] * B)
    if not a.device_only:
        ways["host_readback"] = lambda: st.get_points(held)
        ways["host"] = host_call
    for call in ways.values():
        for _ in range(5):
            call()
    med = {k: [] for k in ways}
    for _ in range(a.rounds):
        for k, call in ways.items():
            t = []
            for _ in range(a.reps if k != "host" else max(a.reps // 10, 3)):
                t0 = time.perf_counter()
                call()
                t.append(1e6 * (time.perf_counter() - t0))
            med[k].append(float(np.median(t)))
    N = int(fr.frame_points.shape[0])
    res = dict(tool="bench_pose_only", reps=a.reps, rounds=a.rounds, keypoints=N, held=int(g.n_initial), n_good=int(g.n_good),
               lm_iterations=g.iters.tolist(), lm_trials=g.trials.tolist(), upload_bytes_per_frame=96 + 16 * N + 4 * len(fr.inv_level_sigma2),
               download_bytes_per_frame=N + 216, readback_bytes_host_path=12 * int(held.shape[0]))
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
