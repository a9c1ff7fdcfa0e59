"""Timing of one anchor of SchwarpDatabase::add on the resident stores: dsh_keyframe_warp_pair against the explicit-array sequence it
replaces (dsh_warp_initialize, dsh_schwarp_eval, dsh_search_by_schwarp, dsh_schwarp_fit_batch_store on host-gathered arrays), for the
same anchor in the same process.  Shape: 1200 key points per keyframe, 600 pairs, 300 queries, a 13 x 15 warp grid.
The call changes the stores, so every repetition runs on a freshly filled pair of stores; the time of the explicit-array sequence is
the sum of the host wall time of its four library calls (the gathers and the object bookkeeping between them, which the reference does
in C++ and this tool in numpy, are left out: the comparison favours the sequence).  Medians after two warm-up repetitions.  Kernel
times come from a run of their own under rocprofv3 --kernel-trace --stats (the new kernels are wp_*_kernel).  Prints one JSON line.
    python tools/bench_warp_pair.py [reps]                        (profiles/warp_pair/README.md has the numbers)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import warp_pair_ref as WP   # noqa: E402
from defslam_amd import nrsfm, sft, synth   # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 12
ctx = sft.Context(0)
sc = synth.make_warp_pair_scene(1200, 600, 300, seed=1, nu=13, nv=15, outliers=0.05)
A = sc["anchors"][0]
i1, i2, q1 = A["pair_idx1"], A["pair_idx2"], A["query_idx1"]

# the sequence's calls are timed where the library is entered
clock = {}
for name in ("WarpInitialize", "schwarp_eval", "searchBySchwarp", "calculateSchwarpsBatch"):
    def timed(*a, _f=getattr(nrsfm, name), _n=name, **k):
        t = time.perf_counter()
        r = _f(*a, **k)
        clock[_n] = clock.get(_n, 0.0) + time.perf_counter() - t
        return r
    setattr(nrsfm, name, timed)

new_t, seq_t, parts, counts = [], [], [], None
for rep in range(reps + 2):
    m = WP.build_model(sc)
    st, ks = WP.stores(ctx, sc, m)
    ddb_a, ddb_b = nrsfm.DiffDatabase(ctx, 4096), nrsfm.DiffDatabase(ctx, 4096)
    t = time.perf_counter()
    g = st.warp_pair(ks, ddb_a, len(m.kfs) - 1, 0, i1, i2, q1, sc["lam"])
    dt = time.perf_counter() - t
    clock.clear()
    r = WP.host_route(ctx, m, sc, 0, i1, i2, q1, ddb_b, len(m.kfs) - 1)
    assert g.x.tobytes() == r["x"].tobytes() and np.array_equal(g.pair_state, r["pair_state"]) and len(ddb_a) == len(ddb_b)
    if rep >= 2:
        new_t.append(dt)
        seq_t.append(sum(clock.values()))
        parts.append(dict(clock))
    counts = g.counts
    for s in (st, ks, ddb_a, ddb_b):
        s.close()
us = lambda v: dict(median_us=float(np.median(v) * 1e6), p10_us=float(np.percentile(v, 10) * 1e6), p90_us=float(np.percentile(v, 90) * 1e6))
out = dict(reps=reps, shape=dict(N=1200, n_pairs=600, n_queries=300, grid=[13, 15]), counts=counts, warp_pair=us(new_t), sequence=us(seq_t),
           sequence_calls={k: float(np.median([p[k] for p in parts]) * 1e6) for k in parts[0]})
out["ratio_warp_pair_over_sequence"] = out["warp_pair"]["median_us"] / out["sequence"]["median_us"]
print(json.dumps(out))
ctx.close()
