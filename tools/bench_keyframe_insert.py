"""Cost of a new keyframe's map point upkeep on the resident stores (dsh_keyframe_process_new) against the three-call path it replaces
(dsh_point_store_add_observations_indexed, dsh_mappoint_update with a CSR the caller builds, dsh_mpdb_update_points), in the same run.

One size per M = 10 / 100 / 500: a store of 600 keyframes x 1200 key points (10 % bad) and 600 map points, every point observed by M
distinct old keyframes; the new keyframe (slot 600) has 1200 key points and holds the 600 points at its even entries.  Both paths add
the same 600 observations and update the same 600 points; after each timed call the 600 pairs are erased again, so every repetition
starts from the same live observations.  The log grows by 600 blanked records per call; only the store path scans the log, so the
growth weighs on it alone.  The two paths alternate within a repetition, so both run over the whole range of log lengths.
Per path: HIP events on dsh_stream around the call(s) and host wall time, medians over --reps after 3 warm-up repetitions.  The CSR
of the three-call path is built once, outside the timed region: the caller's walk over its host objects is NOT in its time.
Prints one JSON object (and writes it to --out).  --summarize-trace CSV sums a `rocprofv3 --kernel-trace --output-format csv` trace of
this tool per kernel name.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from defslam_amd import _lib, localmap, mappoint, sft, track  # noqa: E402

SIZES = (10, 100, 500)
P, K, N = 600, 600, 1200


def make_keyframes(seed=0):
    rng = np.random.default_rng(seed)
    sf, _ = track.orb_pyramid(8)
    return [mappoint.MpKeyFrame(Ow=rng.uniform(-0.3, 0.3, 3).astype(np.float32), desc=rng.integers(0, 256, (N, 32), dtype=np.uint8),
                                octave=rng.integers(0, 8, N).astype(np.int32), scale_factors=sf, bad=bool(k < K and rng.uniform() < 0.1))
            for k in range(K + 1)]


def make_store(ctx, kfs, M, seed):
    """-> (store, xyz, per point its old observations by ascending slot, reference keyframes)."""
    rng = np.random.default_rng(100 + seed)
    xyz = np.column_stack([rng.uniform(-1, 1, P), rng.uniform(-1, 1, P), rng.uniform(1.5, 4, P)]).astype(np.float32)
    obs = [[(int(s), p) for s in np.sort(rng.choice(K, M, replace=False))] for p in range(P)]
    st = localmap.MapPointStore(ctx, points=P, keyframes=K + 1, observations=P * (M + 1) + 64 * P)
    st.add_points(xyz, np.zeros((P, 3), np.float32), np.ones(P, np.float32), rng.integers(0, 256, (P, 32), dtype=np.uint8))
    empty = np.full(N, -1, np.int32)
    for k in range(K):
        st.add_keyframe(empty, bad=kfs[k].bad)
    table = empty.copy()
    table[0:2 * P:2] = np.arange(P)
    st.add_keyframe(table)
    flat = [(p, s, j) for p in range(P) for s, j in obs[p]]
    order = rng.permutation(len(flat))   # arrival order is not slot order
    st.add_observations([flat[i][0] for i in order], [flat[i][1] for i in order], idx=[flat[i][2] for i in order])
    ref = [o[0][0] for o in obs]
    st.set_reference_keyframes(np.arange(P), ref)
    return st, xyz, obs, ref


def run(ctx, ev, ks, kfs, M, reps):
    st, xyz, obs, ref = make_store(ctx, kfs, M, M)
    stream = ctx._L.dsh_stream(ctx._h)
    ids, slots, idx = np.arange(P, dtype=np.int32), np.full(P, K, np.int32), 2 * np.arange(P, dtype=np.int32)
    csr = mappoint.obs_csr([o + [(K, 2 * p)] for p, o in enumerate(obs)])   # ascending slot: the new keyframe is the last

    def store_path():
        g = st.process_new_keyframe(ks, K)
        assert g.n_added == P

    def three_calls():
        st.add_observations(ids, slots, idx=idx)
        u = mappoint.update(ctx, ks, xyz, csr, ref)
        st.update_points(ids, normal=u.normal, max_distance=u.max_distance, desc=u.desc)

    out = dict(points=P, observations_before=M, log_records=P * M)
    results = {}
    paths = (("store", store_path), ("three_calls", three_calls))
    times = {name: ([], []) for name, _ in paths}
    for rep in range(3 + reps):
        for name, fn in paths:
            t0 = time.perf_counter()
            ev.start(stream)
            fn()
            e = ev.stop_ms(stream)
            w = 1e3 * (time.perf_counter() - t0)
            if rep >= 3:
                times[name][0].append(e)
                times[name][1].append(w)
            if rep == 2 + reps:
                results[name] = st.get_points()
            st.erase_observations(ids, slots)
    for name, _ in paths:
        out[name] = dict(event_us_median=1e3 * float(np.median(times[name][0])), wall_us_median=1e3 * float(np.median(times[name][1])), calls=3 + reps)
    a, b = results["store"], results["three_calls"]
    out["identical"] = bool(a.desc.tobytes() == b.desc.tobytes() and a.normal.tobytes() == b.normal.tobytes() and
                            a.max_distance.tobytes() == b.max_distance.tobytes())
    out["store_over_three_calls_event"] = out["store"]["event_us_median"] / out["three_calls"]["event_us_median"]
    out["store_over_three_calls_wall"] = out["store"]["wall_us_median"] / out["three_calls"]["wall_us_median"]
    st.close()
    return out


def summarize_trace(path):
    import csv
    import re
    tot = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            full = row["Kernel_Name"]
            hit = re.search(r"\b((?:ki|mpu|lm|tc|an|ts)_\w+(?:<\d+>)?|__amd_rocclr_\w+)", full)
            name = hit.group(1) if hit else full
            n, t = tot.get(name, (0, 0.0))
            tot[name] = (n + 1, t + (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return [dict(kernel=k, launches=n, total_us=round(t, 1), mean_us=round(t / n, 2)) for k, (n, t) in sorted(tot.items(), key=lambda kv: -kv[1][1])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarize-trace", metavar="CSV", help="kernel time per kernel name of a trace of this tool, then exit")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.summarize_trace:
        for r in summarize_trace(a.summarize_trace):
            print(json.dumps(r))
        return
    ctx = sft.Context(0)
    ev = _lib.HipEvents()
    kfs = make_keyframes()
    ks = mappoint.KeyFrameStore(ctx, K + 1)
    for kf in kfs:
        ks.add(kf)
    res = dict(tool="bench_keyframe_insert", keyframes=K + 1, key_points_per_keyframe=N,
               sizes=[run(ctx, ev, ks, kfs, int(M), a.reps) for M in a.sizes.split(",")])
    ks.close()
    ev.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
