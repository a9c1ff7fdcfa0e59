"""The map point upkeep shim (integration/mappoint_upkeep_hip.h) compiled against stand-in KeyFrame / MapPoint types and run on the
device: ProcessNewKeyFrameHIP over a short keyframe sequence, then a Repose-style geometry-only update, leave every map point's
descriptor, normal, depth range and observations as the sequential restatement (tests/mappoint_ref.py) of the reference's calls does."""
import os

import numpy as np
import pytest

import mappoint_ref as R
import shim_run

INTEG = shim_run.INTEG
LEVELS = 8


def test_mappoint_shim_compiles_against_the_c_abi():
    shim_run.build()
    assert os.path.exists(shim_run.exe("mappoint_shim_test"))
    src = open(os.path.join(INTEG, "mappoint_upkeep_hip.h")).read()
    assert "defslam_hip_debug.h" not in src and "dsh_lab" not in src


def _flip(rng, d, n):
    bits = np.unpackbits(d)
    bits[rng.choice(256, n, replace=False)] ^= 1
    return np.packbits(bits)


@pytest.mark.gpu
def test_mappoint_shim_follows_the_reference_flow(tmp_path):
    from defslam_amd import mappoint, track
    shim_run.build()
    rng = np.random.default_rng(11)
    sf, _ = track.orb_pyramid(LEVELS)
    K, P, N = 12, 300, 400
    Ow = rng.uniform(-0.3, 0.3, (K, 3)).astype(np.float32)
    desc = rng.integers(0, 256, (K, N, 32), dtype=np.uint8)
    octave = rng.integers(0, LEVELS, (K, N)).astype(np.int32)
    bad = np.zeros(K, bool)
    bad[[2, 7]] = True
    kfs = [mappoint.MpKeyFrame(Ow=Ow[k], desc=desc[k], octave=octave[k], scale_factors=sf, bad=bool(bad[k])) for k in range(K)]
    xyz = np.column_stack([rng.uniform(-1, 1, P), rng.uniform(-1, 1, P), rng.uniform(1.5, 4, P)]).astype(np.float32)
    pdesc = rng.integers(0, 256, (P, 32), dtype=np.uint8)
    # map points start with one observation in their reference keyframe (0 or 1), key point p; one in ten has none yet
    ref = rng.integers(0, 2, P)
    init = [[] if p % 10 == 3 else [(int(ref[p]), p)] for p in range(P)]
    for p in range(P):
        desc[ref[p], p] = _flip(rng, pdesc[p], 3)
    # keyframes 2 .. 11 arrive in order; each sees a random third of the points at key point p (some twice: a second key point)
    steps = []
    for k in range(2, K):
        m = np.full(N, -1, np.int64)
        seen = rng.choice(P, P // 3, replace=False)
        m[seen] = seen
        for p in seen:
            desc[k, p] = _flip(rng, pdesc[p], int(rng.integers(0, 30)))
        dup = rng.choice(seen, 5, replace=False)
        m[P + np.arange(5)] = dup
        steps.append((k, m))
    moved = rng.choice(P, 40, replace=False)
    new_xyz = xyz[moved] + rng.uniform(-0.05, 0.05, (40, 3)).astype(np.float32)
    with open(tmp_path / "in.txt", "w") as f:
        f.write(f"{LEVELS} " + " ".join(repr(float(s)) for s in sf) + f"\n{K}\n")
        for k in range(K):
            f.write(" ".join(repr(float(v)) for v in Ow[k]) + f" {N} {int(bad[k])}\n")
            f.write("".join(f"{int(octave[k, j])} " + " ".join(str(int(b)) for b in desc[k, j]) + "\n" for j in range(N)))
        f.write(f"{P}\n")
        for p in range(P):
            f.write(" ".join(repr(float(v)) for v in xyz[p]) + f" {int(ref[p])} {len(init[p])} " + " ".join(f"{a} {b}" for a, b in init[p]) + "\n")
        f.write(f"{len(steps)}\n")
        for k, m in steps:
            f.write(f"{k} {N} " + " ".join(str(int(x)) for x in m) + "\n")
        f.write(f"{len(moved)}\n" + "".join(f"{int(p)} " + " ".join(repr(float(v)) for v in new_xyz[i]) + "\n" for i, p in enumerate(moved)))
    r = shim_run.run("mappoint_shim_test", tmp_path / "in.txt", tmp_path / "out.txt", "0")
    tok = iter(open(tmp_path / "out.txt").read().split())
    order = [int(next(tok)) for _ in range(K)]

    def read_dump():
        out = []
        for _ in range(P):
            n = int(next(tok))
            obs = [(int(next(tok)), int(next(tok))) for _ in range(n)]
            d = np.array([int(next(tok)) for _ in range(32)], np.uint8)
            nv = np.array([float(next(tok)) for _ in range(3)], np.float32)
            out.append((obs, d, nv, np.float32(float(next(tok))), np.float32(float(next(tok)))))
        return out
    after_steps, after_moves = read_dump(), read_dump()

    # the restatement of the same flow, keyframes in the driver's address order
    mps = [mappoint.MapPoint(xyz=xyz[p].copy(), ref_kf=int(ref[p]), obs=dict(init[p]), normal=np.zeros(3, np.float32)) for p in range(P)]
    for k, m in steps:
        matches = [None if x < 0 else mps[x] for x in m]
        R.process_new_keyframe(kfs, k, matches, order)

    def same(a, b):
        return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))

    def compare(dumped):
        for p, (obs, d, nv, mx, mn) in enumerate(dumped):
            mp = mps[p]
            assert obs == mappoint.obs_in_order(mp, order), p
            assert np.array_equal(d, mp.desc), p
            assert same(nv, mp.normal) and same(mx, mp.max_distance) and same(mn, mp.min_distance), (p, nv, mp.normal, mx, mp.max_distance)
    compare(after_steps)
    assert sum(len(o[0]) > 1 for o in after_steps) > P // 2
    for i, p in enumerate(moved):
        mps[p].xyz = new_xyz[i].copy()
        obs = mappoint.obs_in_order(mps[p], order)
        if obs:
            mps[p].normal, mps[p].max_distance, mps[p].min_distance = R.update_normal_and_depth(kfs, mps[p].xyz, obs, mps[p].ref_kf)
    compare(after_moves)
