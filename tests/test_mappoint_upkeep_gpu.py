"""GPU tests of the map point upkeep (dsh_kfdb_*, dsh_mappoint_update) against the sequential restatement tests/mappoint_ref.py:
bit-exact descriptors, elected indices, status, normals and depth ranges on a synthetic map whose observation counts cross every internal
boundary of the kernels, the `what` masks, batch independence, residency of the keyframe store, refusals, and the chain into the
local-map search."""
import ctypes as C

import numpy as np
import pytest

import mappoint_ref as R
import track_search_ref as TR

pytestmark = pytest.mark.gpu

LEVELS = 8
BIG_M = (1, 2, 3, 63, 64, 65, 127, 128, 129, 257, 1000, 4097)
FIELDS = ("desc", "best", "normal", "max_distance", "min_distance", "status")


def _flip(rng, d, n):
    bits = np.unpackbits(d)
    if n:
        bits[rng.choice(256, n, replace=False)] ^= 1
    return np.packbits(bits)


def _views(rng, base, M):
    """M per-view descriptors of one point: bit flips of its descriptor; one point in three draws its views from 2-3 near-duplicate
    patterns (equal rows: median ties)."""
    if rng.uniform() < 1 / 3:
        pats = [_flip(rng, base, int(rng.integers(0, 6))) for _ in range(int(rng.integers(2, 4)))]
        return [pats[int(rng.integers(0, len(pats)))].copy() for _ in range(M)]
    return [_flip(rng, base, int(rng.integers(0, 48))) for _ in range(M)]


def make_map(seed, n_kf=40, n_pts=1500, n_kp=2000):
    """40 keyframes (10 % bad) and 1500 points observed by 1 .. 40 of them, in a random keyframe order (the reference's map order by
    address); 15 % of the points have a reference keyframe that does not observe them; point 7 sits on a keyframe centre."""
    from defslam_amd import mappoint, track
    rng = np.random.default_rng(seed)
    sf, _ = track.orb_pyramid(LEVELS)
    Ow = np.column_stack([rng.uniform(-0.3, 0.3, n_kf), rng.uniform(-0.3, 0.3, n_kf), rng.uniform(-0.3, 0.0, n_kf)]).astype(np.float32)
    desc = rng.integers(0, 256, (n_kf, n_kp, 32), dtype=np.uint8)
    octave = rng.integers(0, LEVELS, (n_kf, n_kp)).astype(np.int32)
    bad = np.zeros(n_kf, bool)
    bad[rng.choice(n_kf, n_kf // 10, replace=False)] = True
    order = rng.permutation(n_kf)          # rank of each keyframe in the std::map order
    used = np.zeros(n_kf, np.int64)
    xyz = np.column_stack([rng.uniform(-1, 1, n_pts), rng.uniform(-1, 1, n_pts), rng.uniform(1.5, 4, n_pts)]).astype(np.float32)
    obs, ref = [], []
    for p in range(n_pts):
        M = int(rng.integers(1, n_kf + 1)) if rng.uniform() < 0.3 else int(rng.integers(1, 12))
        kfs = sorted(rng.choice(n_kf, M, replace=False).tolist(), key=lambda s: order[s])
        o = []
        for s, v in zip(kfs, _views(rng, rng.integers(0, 256, 32, dtype=np.uint8), M)):
            j = int(used[s])
            used[s] += 1
            desc[s, j] = v
            o.append((s, j))
        obs.append(o)
        ref.append(int(rng.integers(0, n_kf)) if rng.uniform() < 0.15 else kfs[int(rng.integers(0, M))])
    xyz[7] = Ow[obs[7][0][0]]                  # on a keyframe centre: the reference's NaN
    kf_list = [mappoint.MpKeyFrame(Ow=Ow[s], desc=desc[s], octave=octave[s], scale_factors=sf, bad=bool(bad[s])) for s in range(n_kf)]
    return kf_list, xyz, obs, ref


def make_big(seed, n_kf=4100, n_kp=16):
    """A second store of 4100 small keyframes for the large observation counts: point q observes BIG_M[q] distinct keyframes through
    key point q of each."""
    from defslam_amd import mappoint, track
    rng = np.random.default_rng(10_000 + seed)
    sf, _ = track.orb_pyramid(LEVELS)
    Ow = rng.uniform(-0.5, 0.5, (n_kf, 3)).astype(np.float32)
    desc = rng.integers(0, 256, (n_kf, n_kp, 32), dtype=np.uint8)
    octave = rng.integers(0, LEVELS, (n_kf, n_kp)).astype(np.int32)
    bad = rng.uniform(size=n_kf) < 0.1
    xyz = np.column_stack([rng.uniform(-1, 1, len(BIG_M)), rng.uniform(-1, 1, len(BIG_M)), rng.uniform(1.5, 4, len(BIG_M))]).astype(np.float32)
    obs, ref = [], []
    for q, M in enumerate(BIG_M):
        kfs = sorted(rng.choice(n_kf, M, replace=False).tolist())
        for s, v in zip(kfs, _views(rng, rng.integers(0, 256, 32, dtype=np.uint8), M)):
            desc[s, q] = v
        obs.append([(s, q) for s in kfs])
        ref.append(kfs[M // 2] if q % 3 else int(rng.integers(0, n_kf)))
    kf_list = [mappoint.MpKeyFrame(Ow=Ow[s], desc=desc[s], octave=octave[s], scale_factors=sf, bad=bool(bad[s])) for s in range(n_kf)]
    return kf_list, xyz, obs, ref


def fill(ctx, kfs, capacity=8, order=None):
    from defslam_amd import mappoint
    st = mappoint.KeyFrameStore(ctx, capacity)
    slots = {}
    for s in (range(len(kfs)) if order is None else order):
        slots[s] = st.add(kfs[s])
    return st, slots


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
    return np.array_equal(a, b)


def check(r, ref, what=3):
    keys = (["best", "desc"] if what & 1 else []) + (["normal", "max_distance", "min_distance"] if what & 2 else []) + ["status"]
    for k in keys:
        got, want = getattr(r, k), ref[k]
        if not same_bits(got, want):
            g2, w2 = np.asarray(got).reshape(len(got), -1), np.asarray(want).reshape(len(want), -1)
            eq = (g2 == w2) | (np.isnan(g2) & np.isnan(w2)) if g2.dtype.kind == "f" else g2 == w2
            bad = np.flatnonzero(~np.all(eq, axis=1))
            raise AssertionError(f"{k}: {len(bad)} points differ, first {bad[:5].tolist()}: {got[bad[:3]]} vs {want[bad[:3]]}")


@pytest.fixture(scope="module")
def small_map(gpu_ctx):
    kfs, xyz, obs, ref = make_map(0)
    st, _ = fill(gpu_ctx, kfs)
    yield kfs, xyz, obs, ref, st
    st.close()


@pytest.fixture(scope="module")
def big_map(gpu_ctx):
    kfs, xyz, obs, ref = make_big(0)
    st, _ = fill(gpu_ctx, kfs, capacity=64)
    yield kfs, xyz, obs, ref, st
    st.close()


def test_small_map_matches_the_restatement(gpu_ctx, small_map):
    from defslam_amd import mappoint
    kfs, xyz, obs, ref, st = small_map
    assert len(st) == len(kfs)
    r = mappoint.update(gpu_ctx, st, xyz, obs, ref)
    check(r, R.update_points(kfs, xyz, obs, ref))
    assert np.isnan(r.normal[7]).all()


def test_observation_counts_across_every_kernel_boundary(gpu_ctx, big_map):
    from defslam_amd import mappoint
    kfs, xyz, obs, ref, st = big_map
    assert [len(o) for o in obs] == list(BIG_M)
    r = mappoint.update(gpu_ctx, st, xyz, obs, ref)
    check(r, R.update_points(kfs, xyz, obs, ref))


def test_what_masks(gpu_ctx, small_map):
    from defslam_amd import mappoint
    kfs, xyz, obs, ref, st = small_map
    P = len(obs)
    d0 = np.random.default_rng(5).integers(0, 256, (P, 32), dtype=np.uint8)
    n0 = np.full((P, 3), 7.0, np.float32)
    m0 = np.full(P, 9.0, np.float32)
    g = mappoint.update(gpu_ctx, st, xyz, obs, ref, mappoint.NORMAL_DEPTH, desc=d0, normal=n0, max_distance=m0, min_distance=m0)
    assert np.array_equal(g.desc, d0) and (g.best == -1).all()
    check(g, R.update_points(kfs, xyz, obs, ref, 2), 2)
    d = mappoint.update(gpu_ctx, st, xyz, obs, ref, mappoint.DESCRIPTOR, desc=d0, normal=n0, max_distance=m0, min_distance=m0)
    assert np.array_equal(d.normal, n0) and np.array_equal(d.max_distance, m0) and np.array_equal(d.min_distance, m0)
    check(d, R.update_points(kfs, xyz, obs, ref, 1, desc=d0), 1)


def test_batches_are_independent(gpu_ctx, small_map, big_map):
    from defslam_amd import mappoint
    for kfs, xyz, obs, ref, st in (small_map, big_map):
        whole = mappoint.update(gpu_ctx, st, xyz, obs, ref)
        h = len(obs) // 2
        a = mappoint.update(gpu_ctx, st, xyz[:h], obs[:h], ref[:h])
        b = mappoint.update(gpu_ctx, st, xyz[h:], obs[h:], ref[h:])
        n = min(len(obs), 200)
        ones = [mappoint.update(gpu_ctx, st, xyz[i:i + 1], obs[i:i + 1], ref[i:i + 1]) for i in range(n)]
        for k in FIELDS:
            w = getattr(whole, k)
            assert same_bits(w, np.concatenate([getattr(a, k), getattr(b, k)])), k
            assert same_bits(w[:n], np.concatenate([getattr(o, k) for o in ones])), k


def test_store_residency(gpu_ctx, small_map):
    """The same keyframes in another slot order, or after a clear, give identical bits; set_bad changes only the election."""
    from defslam_amd import mappoint
    kfs, xyz, obs, ref, st = small_map
    base = mappoint.update(gpu_ctx, st, xyz, obs, ref)
    perm = np.random.default_rng(3).permutation(len(kfs)).tolist()
    st2, slots = fill(gpu_ctx, kfs, capacity=1, order=perm)
    r2 = mappoint.update(gpu_ctx, st2, xyz, [[(slots[s], j) for s, j in o] for o in obs], [slots[s] for s in ref])
    st2.clear()
    assert len(st2) == 0
    for s in range(len(kfs)):
        assert st2.add(kfs[s]) == s
    r3 = mappoint.update(gpu_ctx, st2, xyz, obs, ref)
    for k in FIELDS:
        assert same_bits(getattr(base, k), getattr(r2, k)), k
        assert same_bits(getattr(base, k), getattr(r3, k)), k
    flip = [s for s in range(len(kfs)) if not kfs[s].bad][:6]
    for s in flip:
        st2.set_bad(s)
    r4 = mappoint.update(gpu_ctx, st2, xyz, obs, ref)
    kfs4 = [mappoint.MpKeyFrame(**{**k.__dict__, "bad": k.bad or i in flip}) for i, k in enumerate(kfs)]
    check(r4, R.update_points(kfs4, xyz, obs, ref))
    for k in ("normal", "max_distance", "min_distance"):
        assert same_bits(getattr(base, k), getattr(r4, k)), k
    assert not np.array_equal(base.best, r4.best)
    st2.close()


def _raw(ctx, st, xyz, obs, ref, outs):
    from defslam_amd import mappoint
    ptr, kf, idx = mappoint.obs_csr(obs)
    a = [np.ascontiguousarray(x) for x in (np.asarray(xyz, np.float32), ptr, kf, idx, np.asarray(ref, np.int32))]

    def p(x, t):
        return x.ctypes.data_as(C.POINTER(t))
    return ctx._L.dsh_mappoint_update(ctx._h, st._h if st is not None else None, len(obs), p(a[0], C.c_float), p(a[1], C.c_int32), p(a[2], C.c_int32),
                                      p(a[3], C.c_int32), p(a[4], C.c_int32), 3, p(outs["desc"], C.c_uint8), p(outs["best"], C.c_int32),
                                      p(outs["normal"], C.c_float), p(outs["max"], C.c_float), p(outs["min"], C.c_float), p(outs["status"], C.c_int32))


def test_refusals_write_nothing(gpu_ctx, small_map):
    from defslam_amd import mappoint, sft, track
    kfs, xyz, obs, ref, st = small_map
    P = 4
    xyz, obs, ref = xyz[:P], [list(o) for o in obs[:P]], list(ref[:P])
    sf, _ = track.orb_pyramid(LEVELS)

    def outs():
        return dict(desc=np.full((P, 32), 0xAB, np.uint8), best=np.full(P, 77, np.int32), normal=np.full((P, 3), 5.0, np.float32),
                    max=np.full(P, 6.0, np.float32), min=np.full(P, 6.0, np.float32), status=np.full(P, 99, np.int32))

    def refused(st_, obs_, ref_):
        o = outs()
        assert _raw(gpu_ctx, st_, xyz, obs_, ref_, o) == 1
        fresh = outs()
        assert all(np.array_equal(o[k], fresh[k]) for k in o)

    o = outs()
    assert _raw(gpu_ctx, st, xyz, obs, ref, o) == 0 and not np.array_equal(o["normal"], outs()["normal"])
    refused(st, [obs[0] + [(len(kfs), 0)]] + obs[1:], ref)                                  # slot out of range
    refused(st, [obs[0] + [(obs[0][0][0], 1)]] + obs[1:], ref)                              # repeated slot
    refused(st, [[(obs[0][0][0], 2000)]] + obs[1:], ref)                                    # obs_idx >= N
    refused(st, obs, [len(kfs)] + ref[1:])                                                  # reference slot out of range
    # octave >= levels where the depth reads it
    odd = mappoint.KeyFrameStore(gpu_ctx, 2)
    s0 = odd.add(mappoint.MpKeyFrame(Ow=np.zeros(3, np.float32), desc=np.zeros((2, 32), np.uint8), octave=np.array([LEVELS, 0], np.int32),
                                     scale_factors=sf))
    s1 = odd.add(mappoint.MpKeyFrame(Ow=np.ones(3, np.float32), desc=np.zeros((1, 32), np.uint8), octave=np.array([0], np.int32), scale_factors=sf))
    refused(odd, [[(s0, 0)]] * P, [s0] * P)
    refused(odd, [[(s1, 0)]] * P, [s0] * P)                                                 # not observed: key point 0's octave
    assert _raw(gpu_ctx, odd, xyz, [[(s0, 1)]] * P, [s0] * P, outs()) == 0                  # key point 1 is fine
    odd.close()
    # a store of another context, then detached by dsh_destroy of that context
    other = sft.Context(0)
    ost = mappoint.KeyFrameStore(other, 4)
    ost.add(kfs[0])
    refused(ost, [[(0, 0)]] * P, [0] * P)
    other.close()
    refused(ost, [[(0, 0)]] * P, [0] * P)
    L = gpu_ctx._L
    assert L.dsh_kfdb_add(ost._h, None, None) == 1 and L.dsh_kfdb_set_bad(ost._h, 0, 1) == 1 and L.dsh_kfdb_clear(ost._h) == 1
    ost.close()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_chain_into_the_local_map_search(gpu_ctx, seed):
    """Upkeep outputs (descriptor, normal, max distance) feed local_points_search; the matches equal mappoint_ref -> search_local."""
    from defslam_amd import mappoint, synth, track
    sc = synth.make_track_scene(seed)
    tf, lq = sc["frame"], sc["lq"]
    rng = np.random.default_rng(50 + seed)
    Q = lq.xyz.shape[0]
    sf, _ = track.orb_pyramid(LEVELS)
    n_kf = 12
    Ow = np.column_stack([rng.uniform(-0.05, 0.05, n_kf), rng.uniform(-0.05, 0.05, n_kf), rng.uniform(-0.1, 0.0, n_kf)]).astype(np.float32)
    desc = rng.integers(0, 256, (n_kf, Q, 32), dtype=np.uint8)
    octave = rng.integers(0, 3, (n_kf, Q)).astype(np.int32)
    bad = np.zeros(n_kf, bool)
    bad[3] = True
    obs, ref = [], []
    for q in range(Q):
        kfs_q = sorted(rng.choice(n_kf, int(rng.integers(1, n_kf + 1)), replace=False).tolist())
        for s in kfs_q:
            desc[s, q] = _flip(rng, lq.desc[q], int(rng.integers(0, 12)))
        obs.append([(s, q) for s in kfs_q])
        ref.append(kfs_q[0])
    kfs = [mappoint.MpKeyFrame(Ow=Ow[s], desc=desc[s], octave=octave[s], scale_factors=sf, bad=bool(bad[s])) for s in range(n_kf)]
    st, _ = fill(gpu_ctx, kfs)
    up = mappoint.update(gpu_ctx, st, lq.xyz, obs, ref)
    want = R.update_points(kfs, lq.xyz, obs, ref)
    check(up, want)
    qs = track.LocalQueries(xyz=lq.xyz, normal=up.normal, max_distance=up.max_distance, desc=up.desc, skip=lq.skip)
    N = np.asarray(tf.kp).shape[0]
    res, _ = track.local_points_search(gpu_ctx, tf, np.zeros(N, np.uint8), qs)
    m, n, *_ = TR.search_local(TR.ref_frame(tf), np.zeros(N, np.uint8), lq.xyz, want["normal"], want["max_distance"], want["desc"], lq.skip, 3)
    assert np.array_equal(res.match, m) and res.nmatches == n and n > 0
    st.close()
