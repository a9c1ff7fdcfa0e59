"""Cost of what SchwarpDatabase::add reads of the map for a new keyframe, from the resident store (dsh_keyframe_anchors) against the host
walk over the pointer graph, on one generated map: 1200 key points per keyframe, 300 keyframes, about 360 k observation records, the new
keyframe holding 700 points.

  c_call     the C call end to end through ctypes with preallocated lists: the launches and the one download
  store      AnchorPairsHIP of integration/anchor_pairs_hip.h in the compiled driver: the C call plus the lists as host objects
  host       the loops of SchwarpDatabase.cc:61-106 and DefORBmatcher.cc:200-211 over stand-in objects, in the same driver
c_call is timed by the host clock around the call (it ends in a stream synchronise inside the library), --reps calls after warm-up, the
median and the spread; store and host are the driver's medians over --driver-reps calls.  The three ways must agree: the driver's routes
are compared list by list, and the C call's totals with them.  Prints one JSON object (and writes it to --out).  One process and one
child, no retry, and an alarm ends it after --timeout seconds.  The device time of the kernels alone comes from a kernel trace of this
tool (rocprofv3 --kernel-trace --stats with --store-only, in a run of its own); --summarize-trace prints its per-kernel medians.
"""
import argparse
import ctypes as C
import json
import os
import signal
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from defslam_amd import _lib, localmap, sft  # noqa: E402

DRIVER = os.path.join(ROOT, "integration", "build", "anchor_pairs_shim_test")


def make_map(K=300, N=1200, own=40, span=30, held_recent=400, held_older=300, seed=5):
    """Keyframe r creates `own` points and the `span` keyframes from r on observe them, so a keyframe's table is full at own * span
    entries; the new keyframe K - 1 holds the newest held_recent points and held_older random older ones, and observes them all."""
    rng = np.random.default_rng(seed)
    ref = np.repeat(np.arange(K - 1), own).astype(np.int32)
    P = ref.shape[0]
    pt = np.repeat(np.arange(P), span)
    kf = ref[pt] + np.tile(np.arange(span), P)
    keep = kf < K - 1
    pt, kf = pt[keep], kf[keep]
    order = np.argsort(kf, kind="stable")
    pt, kf = pt[order], kf[order]
    idx = np.arange(kf.shape[0]) - np.searchsorted(kf, kf, side="left")
    tables = np.full((K, N), -1, np.int32)
    tables[kf, idx] = pt
    held = np.concatenate([np.arange(P - held_recent, P), rng.choice(P - held_recent, held_older, replace=False)])
    tables[K - 1, :held.shape[0]] = held
    log = np.column_stack([np.concatenate([pt, held]), np.concatenate([kf, np.full(held.shape[0], K - 1)]),
                           np.concatenate([idx, np.arange(held.shape[0])])]).astype(np.int32)
    return ref, tables, log


def fill(ctx, ref, tables, log):
    st = localmap.MapPointStore(ctx, points=ref.shape[0], keyframes=tables.shape[0], observations=log.shape[0])
    P = ref.shape[0]
    z = np.zeros((P, 3), np.float32)
    st.add_points(z, z, np.ones(P, np.float32), np.zeros((P, 32), np.uint8))
    for t in tables:
        st.add_keyframe(t)
    st.add_observations(log[:, 0], log[:, 1], idx=log[:, 2])
    st.set_reference_keyframes(np.arange(P), ref)
    return st


def write_map(path, ref, tables, log, min_pairs):
    """The scene file of integration/standin_store_scene.h without appearance, and the driver's tail: the newest keyframe, no drop."""
    P, K = ref.shape[0], tables.shape[0]
    n_obs = np.bincount(log[:, 0], minlength=P)
    with open(path, "w") as f:
        f.write(f"store_scene {P} {K} {log.shape[0]} 0\n")
        f.write("".join(f"0 0 1 0 0 1 1 0 0 {r} {n} 1 1" + " 0" * 32 + "\n" for r, n in zip(ref, n_obs)))
        for t in tables:
            f.write(f"{t.shape[0]} -1 0 " + " ".join(map(str, t)) + "\n")
        f.write("".join(f"{p} {k} {i} 1\n" for p, k, i in log))
        f.write(f"{K - 1} {min_pairs} -1 -1\n")


def summarize_trace(path):
    """Per-kernel medians of a `rocprofv3 --kernel-trace --output-format csv` trace of this tool."""
    import csv
    import re
    durs = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            m = re.search(r"\b(an_\w+)", row["Kernel_Name"])
            if m:
                durs.setdefault(m.group(1), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return [dict(kernel=k, calls=len(v), median_us=round(float(np.median(v)), 2), max_us=round(float(np.max(v)), 2)) for k, v in sorted(durs.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarize-trace", metavar="CSV", default="")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--driver-reps", type=int, default=50)
    ap.add_argument("--min-pairs", type=int, default=20)
    ap.add_argument("--store-only", action="store_true", help="time the C call alone (for a kernel trace)")
    ap.add_argument("--out", default="")
    ap.add_argument("--timeout", type=int, default=300, help="seconds after which the process ends itself")
    a = ap.parse_args()
    signal.alarm(a.timeout)
    if a.summarize_trace:
        for r in summarize_trace(a.summarize_trace):
            print(json.dumps(r))
        return
    ref, tables, log = make_map()
    slot = tables.shape[0] - 1
    ctx = sft.Context(0)
    st = fill(ctx, ref, tables, log)
    g = st.keyframe_anchors(slot, a.min_pairs)
    A, NP, NQ = g.anchor_slot.shape[0], g.pair_idx1.shape[0], g.query_idx1.shape[0]
    arrs = {n: np.zeros(max(c, 1), np.int32) for n, c in (("anchor_slot", A), ("anchor_count", A), ("anchor_pairs", A), ("pair_ptr", A + 1),
                                                          ("query_ptr", A + 1), ("pair_idx1", NP), ("pair_idx2", NP), ("pair_point", NP),
                                                          ("query_idx1", NQ), ("query_point", NQ))}
    own, has = np.zeros(max(NP, 1), np.uint8), np.zeros(tables.shape[1], np.uint8)
    r = _lib.AnchorListsC(anchor_capacity=A, pair_capacity=NP, query_capacity=NQ, pair_own=own.ctypes.data_as(C.POINTER(C.c_uint8)),
                          has=has.ctypes.data_as(C.POINTER(C.c_uint8)), **{n: v.ctypes.data_as(C.POINTER(C.c_int32)) for n, v in arrs.items()})
    fn, h = ctx._L.dsh_keyframe_anchors, st._h
    t = []
    for i in range(20 + a.reps):
        t0 = time.perf_counter()
        rc = fn(h, slot, a.min_pairs, C.byref(r))
        t.append(1e6 * (time.perf_counter() - t0))
        if rc != 0:
            raise SystemExit("dsh_keyframe_anchors failed: " + ctx._L.dsh_last_error(ctx._h).decode())
    t = np.array(t[20:])
    res = dict(tool="bench_anchor_pairs", reps=a.reps, keypoints=int(tables.shape[1]), keyframes=int(tables.shape[0]), points=int(ref.shape[0]),
               log_records=int(log.shape[0]), anchors=int(A), anchors_fitting=int((g.anchor_pairs >= a.min_pairs).sum()), pairs=int(NP), queries=int(NQ),
               download_bytes=int(16 + 12 * A + 8 * (A + 1) + 13 * NP + 8 * NQ + tables.shape[1]),
               c_call_us=dict(median=round(float(np.median(t)), 1), min=round(float(t.min()), 1), max=round(float(t.max()), 1)))
    st.close()
    ctx.close()
    if not a.store_only:
        with tempfile.TemporaryDirectory() as d:
            write_map(os.path.join(d, "map.txt"), ref, tables, log, a.min_pairs)
            subprocess.run([DRIVER, os.path.join(d, "map.txt"), os.path.join(d, "out.txt"), "0", str(a.driver_reps)], check=True, timeout=a.timeout)
            lines = open(os.path.join(d, "out.txt")).read().splitlines()
        store = [ln.split(" ", 1)[1] for ln in lines if ln.startswith("store ")]
        host = [ln.split(" ", 1)[1] for ln in lines if ln.startswith("host ")]
        if store != host or len([ln for ln in store if ln.startswith("lists anchor")]) != A:
            raise SystemExit("the store route, the host walk and the C call disagree")
        host_us, store_us = map(float, lines[-1].split()[1:])
        res.update(driver_reps=a.driver_reps, host_walk_us=host_us, store_route_us=store_us)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
