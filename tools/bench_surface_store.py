"""Timing of the resident Surface of a keyframe: dsh_keyframe_sfn against dsh_sfn_estimate on ready host arrays (the baseline), the
normal-writing and gathering calls, and the chain Shape from Normals -> registration -> template switch with resident inputs against
the same chain with explicit arrays.  A keyframe of N = 1200 key points with 600 sites on a 13 x 15 grid
(tests/surface_store_ref.make_surface_scene), host wall time around calls that end in a stream synchronise, the two sides of every
comparison alternating in one loop.  Prints one JSON line.
    python tools/bench_surface_store.py [reps]                  (profiles/surface_store/README.md has the numbers)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import surface_register_ref as SR   # noqa: E402
import surface_store_ref as SS   # noqa: E402
from defslam_amd import localmap, mappoint, nrsfm, sft, synth   # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
BW = 1e-3
ctx = sft.Context(0)


def alternating(fns, n):
    """Every function once per round, n rounds after n / 10 warm-up rounds: {name: median / p10 / p90 in us}."""
    t = {k: [] for k in fns}
    for r in range(max(5, n // 10) + n):
        for k, fn in fns.items():
            a = time.perf_counter()
            fn()
            if r >= max(5, n // 10):
                t[k].append(time.perf_counter() - a)
    return {k: dict(median_us=float(np.median(v) * 1e6), p10_us=float(np.percentile(v, 10) * 1e6), p90_us=float(np.percentile(v, 90) * 1e6)) for k, v in t.items()}


# ---- Shape from Normals of a keyframe: the store against ready host arrays ----
sc = SS.make_surface_scene(1200, seed=5, n_sites=600)
m, slot = sc["model"], sc["slot"]
st = localmap.MapPointStore(ctx)
SR.fill_store(m, st)
st.surface_init(slot, sc["kpn"])
m.surface_init(slot, sc["kpn"])
ents = np.array(sorted(sc["normals"]), np.int32)
slots = np.full(len(ents), slot, np.int32)
normals = np.array([sc["normals"][i] for i in ents], np.float32)
st.surface_set_normals(slots, ents, normals)
m.set_normals(slots, ents, normals)
st.set_bad_full(sc["emptied"])
m.set_bad(sc["emptied"])
c, w, u, v, nr = m.sfn_select(slot)
assert c["n_sites"] == 600
b = nrsfm.Bbs(*sc["bbs"])
kpn = sc["kpn"].astype(np.float64)
ua, va = kpn[:, 0].copy(), kpn[:, 1].copy()
resident = lambda: st.sfn(slot, b, BW, sc["mean_depth"])
host = lambda: nrsfm.ShapeFromNormals(ctx, b, u, v, nr, BW, sc["mean_depth"], ua, va)
g, h = resident(), host()
assert g.ok and h[0] and g.ctrl.tobytes() == h[2].tobytes() and g.pts.tobytes() == h[3].tobytes()
out = dict(N=1200, n_sites=600, grid=[13, 15], reps=reps)
out["sfn"] = alternating(dict(keyframe_sfn=resident, sfn_estimate_host_arrays=host), reps)
out["ratio_keyframe_sfn_over_sfn_estimate"] = out["sfn"]["keyframe_sfn"]["median_us"] / out["sfn"]["sfn_estimate_host_arrays"]["median_us"]
out["bookkeeping"] = alternating(dict(set_normals_600=lambda: st.surface_set_normals(slots, ents, normals), gather_600=lambda: st.surface_gather(slots, ents),
                                      get=lambda: st.surface_get(slot)), reps)
st.close()

# ---- the chain on one keyframe: SfN, registration, template switch; resident inputs against explicit arrays ----
# The template switch scene has the keyframe, its key points and a template; the switch creates points, so every round works on the
# same pair of stores and only the first switch of each creates many.  The keyframe's snapshot is taken once, before the rounds, so
# every round registers against the same map cloud, which is placed at 1.3 times the surface the normals give; the stream has eight candidates for scaleMinMedian, so 43 KB of it go up on both sides.
tsc = synth.make_template_switch_scene(1, n_kf=2, n_kp=1200, held_frac=0.5, obs_per_point=2, n_frame_kp=300, ctrl=(13, 15), ref_slot=-1)
r, N = tsc["ref_slot"], tsc["kp"].shape[0]
tb = nrsfm.Bbs(*tsc["bbs"])


def chain_stores():
    s = localmap.MapPointStore(ctx)
    s.add_points(tsc["xyz"], tsc["normal"], tsc["max_distance"], tsc["desc"], tsc["bad"])
    for j in range(tsc["tables"].shape[0]):
        assert s.add_keyframe(tsc["tables"][j], tsc["parents"][j], tsc["kf_bad"][j]) == j
    s.add_observations(tsc["obs_point"], tsc["obs_kf"])
    P = tsc["xyz"].shape[0]
    s.set_counters(np.arange(P), tsc["visible"], tsc["found"])
    s.set_embedding(np.arange(P), tsc["nodes"], tsc["bary"])
    k = mappoint.KeyFrameStore(ctx, 4)
    for j in range(tsc["tables"].shape[0]):
        k.add(mappoint.MpKeyFrame(tsc["kf_Ow"][j], tsc["kf_desc"][j], tsc["kf_octave"][j], tsc["scale_factors"], bool(tsc["kf_bad"][j])))
    return s, k


a, ka = chain_stores()
e, ke = chain_stores()
kf = localmap.KeyFramePoints(tsc["rows"], tsc["cols"], tsc["kp"])
gs = synth.make_sfn_scene(N, seed=3, with_normal_frac=1.0)                          # the surface the normals come from, and its key points
kpn_t = np.stack([gs["u_all"], gs["v_all"]], 1).astype(np.float32)
cb = nrsfm.Bbs(*gs["bbs"])
a.surface_init(r, kpn_t)
table = a.keyframe_table(r)
held = np.flatnonzero(table >= 0).astype(np.int32)
hn = gs["normals"][held].astype(np.float32)
a.surface_set_normals(np.full(len(held), r, np.int32), held, hn)
bad = a.get_points().bad
sites = np.array([i for i in held if not bad[table[i]]], np.int64)
su, sv, sn = kpn_t[sites, 0].astype(np.float64), kpn_t[sites, 1].astype(np.float64), gs["normals"][sites].astype(np.float32)
kua, kva = kpn_t[:, 0].astype(np.float64), kpn_t[:, 1].astype(np.float64)
nodes = nrsfm.surface_vertices(ctx, tb, tsc["depth_ctrl"], tsc["Twc"], 10, 10)
ctx.template_build(nodes, synth.regular_triangulation(10, 10))


# the map the keyframe is registered against: its points at 1.3 times the surface Shape from Normals will give, with a little noise
q0 = nrsfm.ShapeFromNormals(ctx, cb, su, sv, sn, BW, gs["mean_depth"], kua, kva)
assert q0[0]
T64 = tsc["Twc"].astype(np.float64)
world = q0[3].astype(np.float64) @ T64[:3, :3].T + T64[:3, 3]
placed = (1.3 * world[held] + np.random.default_rng(0).normal(0, 1e-3, (len(held), 3))).astype(np.float32)
for s in (a, e):
    s.update_points(table[held], xyz=placed)
n_pairs = a.snapshot_positions(r)
assert n_pairs == e.snapshot_positions(r) >= 15
stream = np.full(n_pairs + 8 * (n_pairs - 1), 0.9)                                  # a draw <= 0.25 makes a candidate, which draws n - 1 more
for j in range(8):
    stream[j * n_pairs] = 0.1
    stream[j * n_pairs + 1:(j + 1) * n_pairs] = np.random.default_rng(j).random(n_pairs - 1)
registered = []


def chain_resident():
    q = a.sfn(r, cb, BW, gs["mean_depth"])
    g = a.register_surface(ka, r, None, tsc["Twc"], stream, 0.05, check_chi=False)
    a.switch_template(ka, r, kf, None, tsc["Twc"])
    registered.append(g.registered)
    return q, g


def chain_explicit():
    q = nrsfm.ShapeFromNormals(ctx, cb, su, sv, sn, BW, gs["mean_depth"], kua, kva)
    g = e.register_surface(ke, r, q[3], tsc["Twc"], stream, 0.05, check_chi=False)
    e.switch_template(ke, r, kf, g.surface_scaled, tsc["Twc"])
    registered.append(g.registered)
    return q, g


(qa, ga), (qe, ge) = chain_resident(), chain_explicit()
assert qa.ok and qe[0] and qa.n_sites == len(sites) and qa.pts.tobytes() == qe[3].tobytes()
assert ga.registered and ge.registered and ga.sim3.tobytes() == ge.sim3.tobytes() and ga.n_pairs == n_pairs
assert a.surface_get(r).pts.tobytes() == ge.surface_scaled.tobytes()
assert a.get_points().xyz.tobytes() == e.get_points().xyz.tobytes()
out["chain"] = dict(N=int(N), n_sites=int(len(sites)), n_pairs=int(n_pairs), **alternating(dict(resident=chain_resident, explicit=chain_explicit), max(20, reps // 4)))
out["ratio_chain_resident_over_explicit"] = out["chain"]["resident"]["median_us"] / out["chain"]["explicit"]["median_us"]
assert all(registered)
print(json.dumps(out))
for s in (a, ka, e, ke):
    s.close()
ctx.close()
