"""Cost of the map point upkeep (dsh_mappoint_update: ComputeDistinctiveDescriptors + UpdateNormalAndDepth) on the device.

Three sizes, 1200 map points each, every point observed by M distinct keyframes of a resident store of 600 keyframes x 1200 key points
(10 % bad):  M = 10 (the default sequence after 100 frames: a keyframe every 10th frame), M = 100, M = 500 (a long sequence).
Per size: HIP events on dsh_stream around each call (upload, launches, download) and host wall time, medians over --reps calls after 3
warm-up calls, and the Hamming pairs a call evaluates (sum over points of Me^2, Me = observations in keyframes that are not bad).
Prints one JSON object (and writes it to --out).  The device time of the kernels alone comes from a kernel trace of this tool
(rocprofv3 --kernel-trace --stats); --summarize-trace turns that trace into kernel time per call and Hamming pairs per second.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from defslam_amd import _lib, mappoint, sft, track  # noqa: E402

SIZES = (10, 100, 500)
P, K, N = 1200, 600, 1200


def make_store_data(seed=0):
    rng = np.random.default_rng(seed)
    sf, _ = track.orb_pyramid(8)
    desc = rng.integers(0, 256, (K, N, 32), dtype=np.uint8)
    kfs = [mappoint.MpKeyFrame(Ow=rng.uniform(-0.3, 0.3, 3).astype(np.float32), desc=desc[k], octave=rng.integers(0, 8, N).astype(np.int32),
                               scale_factors=sf, bad=bool(rng.uniform() < 0.1)) for k in range(K)]
    return kfs


def make_points(kfs, M, seed):
    """Point p observes M distinct keyframes through key point p of each (slot order)."""
    rng = np.random.default_rng(100 + seed)
    xyz = np.column_stack([rng.uniform(-1, 1, P), rng.uniform(-1, 1, P), rng.uniform(1.5, 4, P)]).astype(np.float32)
    obs = [[(int(s), p) for s in np.sort(rng.choice(K, M, replace=False))] for p in range(P)]
    ref = [o[0][0] for o in obs]
    pairs = sum(sum(1 for s, _ in o if not kfs[s].bad) ** 2 for o in obs)
    return xyz, mappoint.obs_csr(obs), ref, pairs


def kernels_per_call(M):
    """mpu_launch: points with M <= 64 take one packed kernel; larger ones the large and the finish kernel."""
    return 1 if M <= 64 else 2


def run(ctx, ev, st, kfs, M, reps):
    xyz, csr, ref, pairs = make_points(kfs, M, M)
    stream = ctx._L.dsh_stream(ctx._h)
    for _ in range(3):
        mappoint.update(ctx, st, xyz, csr, ref)
    ev_ms, wall_ms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        ev.start(stream)
        mappoint.update(ctx, st, xyz, csr, ref)
        ev_ms.append(ev.stop_ms(stream))
        wall_ms.append(1e3 * (time.perf_counter() - t0))
    return dict(points=P, observations=M, hamming_pairs=int(pairs), event_us_median=1e3 * float(np.median(ev_ms)),
                wall_us_median=float(1e3 * np.median(wall_ms)), calls=3 + reps, kernels_per_call=kernels_per_call(M))


def summarize_trace(path, bench_json):
    """Kernel time per call from a `rocprofv3 --kernel-trace --output-format csv` trace of this tool: the mpu_* kernels in launch order,
    cut into calls by the plan the tool's own output line records (calls and kernels per call of every size)."""
    import csv
    rows = []
    with open(path) as f:
        for row in csv.DictReader(f):
            if "mpu_" in row["Kernel_Name"]:
                rows.append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    rows.sort()
    plan = json.load(open(bench_json))["sizes"]
    out, i = [], 0
    for leg in plan:
        k, n = leg["kernels_per_call"], leg["calls"]
        per_call = [sum(d for _, d in rows[i + c * k:i + (c + 1) * k]) for c in range(3, n)]
        i += k * n
        med = float(np.median(per_call))
        out.append(dict(observations=leg["observations"], points=leg["points"], calls=len(per_call), kernel_us_median=round(med, 1),
                        hamming_pairs=leg["hamming_pairs"], hamming_pairs_per_s=leg["hamming_pairs"] / (1e-6 * med),
                        event_us_median=round(leg["event_us_median"], 1)))
    assert i == len(rows), (i, len(rows))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarize-trace", nargs=2, metavar=("CSV", "BENCH_JSON"), help="kernel time per call of a trace of this tool, then exit")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.summarize_trace:
        for r in summarize_trace(*a.summarize_trace):
            print(json.dumps(r))
        return
    ctx = sft.Context(0)
    ev = _lib.HipEvents()
    kfs = make_store_data()
    st = mappoint.KeyFrameStore(ctx, K)
    for kf in kfs:
        st.add(kf)
    res = dict(tool="bench_mappoint_upkeep", keyframes=K, key_points_per_keyframe=N, sizes=[run(ctx, ev, st, kfs, M, a.reps) for M in SIZES])
    st.close()
    ev.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
