"""Cost of LocalMapping::MapPointCulling on the resident map point store (dsh_point_store_cull: decision, bad flags, observation records
and table entries in one call) against what the same state change needs without it: dsh_trackstate_cull for the decision and the flags,
dsh_mpdb_erase_observations for the records of the culled points, and one dsh_mpdb_set_keyframe_point per table entry -- the caller
knowing from its host objects which records and entries those are, which is NOT in that path's time.

The store: 200 keyframes x 1200 key points, 40 000 points with 5 observations each in 5 distinct keyframes (a log of 200 000 records in
shuffled order, every observation in a table entry of its own); the first 1200 points are mlpRecentAddedMapPoints, about 30 % of them
with found / visible < 0.4.  A cull is destructive, so every repetition builds two fresh stores with the same contents, one per path;
the stores of both paths are compared afterwards (bad flags, every table, the observations of the recent points; not n_obs, which
setBadFlag leaves and dsh_mpdb_erase_observations decrements).
Per path: HIP events on dsh_stream around the call(s) and host wall time, medians over --reps after one warm-up repetition.
Prints one JSON object (and writes it to --out).  --summarize-trace CSV sums a `rocprofv3 --kernel-trace --output-format csv` trace of
this tool per kernel name: the kernel time of a call.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from defslam_amd import _lib, localmap, sft  # noqa: E402

K, N, P, M, RECENT = 200, 1200, 40000, 5, 1200
CURRENT_KF = 10


def make_scene(seed=0):
    rng = np.random.default_rng(seed)
    p = np.repeat(np.arange(P, dtype=np.int32), M)
    n = np.arange(P * M)
    kf = (n % K).astype(np.int32)                     # the M observations of a point lie in M consecutive keyframes
    idx = (n // K).astype(np.int32)                   # every observation in an entry of its own: P * M / K = 1000 <= N
    tables = np.full((K, N), -1, np.int32)
    tables[kf, idx] = p
    order = rng.permutation(P * M)                    # arrival order is not slot order
    found, visible = np.ones(P, np.int32), np.ones(P, np.int32)
    low = rng.random(RECENT) < 0.3
    visible[:RECENT] = 10
    found[:RECENT] = np.where(low, rng.integers(0, 4, RECENT), rng.integers(4, 11, RECENT))
    first_kf = rng.integers(6, 11, RECENT).astype(np.int32)
    return dict(p=p[order], kf=kf[order], idx=idx[order], tables=tables, found=found, visible=visible, first_kf=first_kf, obs_kf=kf.reshape(P, M),
                obs_idx=idx.reshape(P, M))


def make_store(ctx, sc):
    st = localmap.MapPointStore(ctx, points=P, keyframes=K, observations=P * M)
    z = np.zeros((P, 3), np.float32)
    st.add_points(z, z, np.ones(P, np.float32), np.zeros((P, 32), np.uint8))
    for k in range(K):
        st.add_keyframe(sc["tables"][k])
    st.add_observations(sc["p"], sc["kf"], idx=sc["idx"])
    st.set_reference_keyframes(np.arange(P), sc["obs_kf"][:, 0])
    st.set_counters(np.arange(P), sc["visible"], sc["found"])
    return st


def state(st):
    ids = np.arange(RECENT)
    o = st.observations(ids)
    return (st.get_points().bad.tobytes(), b"".join(st.keyframe_table(k).tobytes() for k in range(K)),
            o.ptr.tobytes(), o.slots.tobytes(), o.idx.tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarize-trace", metavar="CSV", help="kernel time per kernel name of a trace of this tool, then exit")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.summarize_trace:
        from bench_keyframe_insert import summarize_trace
        for r in summarize_trace(a.summarize_trace):
            print(json.dumps(r))
        return
    ctx = sft.Context(0)
    ev = _lib.HipEvents()
    stream = ctx._L.dsh_stream(ctx._h)
    sc = make_scene()
    ids = np.arange(RECENT, dtype=np.int32)
    times = {"store": ([], []), "parent": ([], [])}
    info = {}
    for rep in range(1 + a.reps):
        sa, sb = make_store(ctx, sc), make_store(ctx, sc)

        def store_path():
            g = sa.cull_full(ids, sc["first_kf"], CURRENT_KF)
            info.update(n_set_bad=g.counts.n_set_bad, n_records=g.counts.n_records, n_entries=g.counts.n_entries)

        def parent_path():
            act = sb.cull(ids, sc["first_kf"], CURRENT_KF)
            gone = ids[act == localmap.CULL_SET_BAD]                 # the caller's walk over mObservations of the culled points
            sb.erase_observations(np.repeat(gone, M), sc["obs_kf"][gone].reshape(-1))
            for s, i in zip(sc["obs_kf"][gone].reshape(-1).tolist(), sc["obs_idx"][gone].reshape(-1).tolist()):
                sb.set_keyframe_point(s, i, -1)

        for name, fn in (("store", store_path), ("parent", parent_path)):
            t0 = time.perf_counter()
            ev.start(stream)
            fn()
            e = ev.stop_ms(stream)
            w = 1e3 * (time.perf_counter() - t0)
            if rep >= 1:
                times[name][0].append(e)
                times[name][1].append(w)
        if rep == a.reps:
            info["identical"] = state(sa) == state(sb)
        sa.close()
        sb.close()
    res = dict(tool="bench_point_erase", keyframes=K, key_points_per_keyframe=N, points=P, log_records=P * M, recent_points=RECENT, reps=a.reps, **info)
    for name in times:
        res[name] = dict(event_us_median=1e3 * float(np.median(times[name][0])), wall_us_median=1e3 * float(np.median(times[name][1])))
    res["store_over_parent_wall"] = res["store"]["wall_us_median"] / res["parent"]["wall_us_median"]
    ev.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
