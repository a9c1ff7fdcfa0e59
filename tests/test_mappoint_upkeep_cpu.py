"""CPU tests of the map point upkeep: the restatement (tests/mappoint_ref.py) against a brute-force election and on hand-built points
with known answers, and the ABI's refusals (bad arguments first, then no device) on a host-only context."""
import ctypes as C

import numpy as np
import pytest

import mappoint_ref as R

f32 = np.float32


def kf(Ow, desc, octave=None, bad=False, levels=8):
    from defslam_amd import mappoint, track
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    sf, _ = track.orb_pyramid(levels)
    return mappoint.MpKeyFrame(Ow=np.asarray(Ow, np.float32), desc=desc,
                               octave=np.zeros(desc.shape[0], np.int32) if octave is None else np.asarray(octave, np.int32), scale_factors=sf, bad=bad)


def desc_bits(bits):
    """A descriptor with the given bit positions set."""
    out = np.zeros(32, np.uint8)
    for b in bits:
        out[b // 8] |= np.uint8(1 << (b % 8))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_restated_election_matches_brute_force(seed):
    rng = np.random.default_rng(seed)
    for M in (1, 2, 3, 4, 5, 8, 17, 40):
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        flips = rng.random((M, 256)) < rng.choice([0.02, 0.1, 0.5])
        rows = np.packbits(np.unpackbits(base)[None, :] ^ flips, axis=1)
        if M > 3:
            rows[M // 2] = rows[0]   # a duplicate: equal rows, equal medians
        assert R.elect(rows) == R.elect_bruteforce(rows), (seed, M)


def test_one_and_two_observations():
    a, b = desc_bits([1, 2, 3]), desc_bits([200])
    kfs = [kf([0, 0, 0], [a]), kf([1, 0, 0], [b])]
    best, row = R.compute_distinctive_descriptors(kfs, [(0, 0)])
    assert best == 0 and (row == a).all()
    best, row = R.compute_distinctive_descriptors(kfs, [(1, 0), (0, 0)])   # M = 2: both medians are 0, the first wins
    assert best == 0 and (row == b).all()


def test_equal_medians_go_to_the_earliest_observation():
    """Rows 0 and 1 both have median 1 (distance 1 to each other); row 2 is far.  Iteration order decides: the earliest wins."""
    x, y, z = desc_bits([0]), desc_bits([0, 1]), desc_bits(range(100, 160))
    kfs = [kf([0, 0, 0], [z]), kf([0, 0, 1], [y]), kf([0, 1, 0], [x])]
    assert R.compute_distinctive_descriptors(kfs, [(2, 0), (1, 0), (0, 0)])[0] == 0
    assert R.compute_distinctive_descriptors(kfs, [(1, 0), (2, 0), (0, 0)])[0] == 0
    assert R.compute_distinctive_descriptors(kfs, [(0, 0), (1, 0), (2, 0)])[0] == 1


def test_bad_keyframe_leaves_the_election_but_counts_in_the_normal():
    far = desc_bits(range(0, 200))
    kfs = [kf([0, 0, 0], [desc_bits([5])]), kf([2, 0, 0], [far], bad=True), kf([0, 0, 2], [desc_bits([5, 6])])]
    xyz = np.array([1, 0, 1], np.float32)
    obs = [(0, 0), (1, 0), (2, 0)]
    best, row = R.compute_distinctive_descriptors(kfs, obs)
    assert best == 0                      # among the two good ones (M = 2): the first
    n3, mx, mn = R.update_normal_and_depth(kfs, xyz, obs, 0)
    n2, _, _ = R.update_normal_and_depth(kfs, xyz, [(0, 0), (2, 0)], 0)
    assert not np.array_equal(n3, n2)     # the bad keyframe's direction is in the sum, and n = 3
    # (1,0,1)/sqrt2 + (-1,0,1)/sqrt2 + (1,0,-1)/sqrt2, over 3: x = z = 1/(3 sqrt2)
    assert abs(float(n3[0]) - 1 / (3 * np.sqrt(2))) < 1e-6 and abs(float(n3[2]) - 1 / (3 * np.sqrt(2))) < 1e-6
    assert mx == f32(np.sqrt(2)) and mn == f32(mx / kfs[0].scale_factors[7])   # key point 0 of the reference keyframe: octave 0


def test_reference_keyframe_not_observed_uses_key_point_0():
    """observations[pRefKF] on the copy inserts pRefKF with index 0: key point 0's octave of the reference keyframe sets the range."""
    kfs = [kf([0, 0, 0], [desc_bits([1])] * 3, octave=[3, 0, 5]), kf([0, 0, 4], [desc_bits([2])])]
    xyz = np.array([0, 0, 1], np.float32)
    _, mx_absent, _ = R.update_normal_and_depth(kfs, xyz, [(1, 0)], 0)
    _, mx_present, _ = R.update_normal_and_depth(kfs, xyz, [(0, 2), (1, 0)], 0)
    sf = kfs[0].scale_factors
    assert mx_absent == f32(f32(1) * sf[3]) and mx_present == f32(f32(1) * sf[5])


def test_all_observations_in_bad_keyframes_leave_the_descriptor():
    kfs = [kf([0, 0, 0], [desc_bits([1])], bad=True), kf([0, 0, 3], [desc_bits([2])], bad=True)]
    old = desc_bits([9, 10])
    r = R.update_point(kfs, np.array([0, 0, 1], np.float32), [(0, 0), (1, 0)], 0, 3, desc=old)
    assert r["best"] == -1 and (r["desc"] == old).all() and r["status"] == 2
    assert np.isfinite(r["normal"]).all() and r["max_distance"] == f32(1)
    r = R.update_point(kfs, np.zeros(3, np.float32), [], 0, 3, desc=old)
    assert r["status"] == 1 and (r["desc"] == old).all() and r["best"] == -1


def test_point_on_a_keyframe_centre_gives_nan():
    kfs = [kf([1, 2, 3], [desc_bits([1])])]
    n, mx, mn = R.update_normal_and_depth(kfs, np.array([1, 2, 3], np.float32), [(0, 0)], 0)
    assert np.isnan(n).all() and mx == 0 and mn == 0


# ---- the ABI without a device ----------------------------------------------------------------------------------------------------

def _call(ctx, P=1, xyz=None, ptr=None, kf=None, idx=None, ref=None, what=3, desc=True, geom=True, store=None):
    from defslam_amd import _lib
    keep = []

    def arr(a, t, ct):
        if a is None:
            return None
        a = np.ascontiguousarray(a, t)
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(ct))
    xyz = np.zeros((max(P, 1), 3), np.float32) if xyz is None else xyz
    ptr = np.array([0] + [1] * P, np.int32) if ptr is None else ptr
    kf = np.zeros(max(P, 1), np.int32) if kf is None else kf
    idx = np.zeros(max(P, 1), np.int32) if idx is None else idx
    ref = np.zeros(max(P, 1), np.int32) if ref is None else ref
    out_d = np.zeros((max(P, 1), 32), np.uint8) if desc else None
    out_b = np.zeros(max(P, 1), np.int32)
    out_n = np.zeros((max(P, 1), 3), np.float32) if geom else None
    out_m = np.zeros(max(P, 1), np.float32) if geom else None
    out_s = np.zeros(max(P, 1), np.int32)
    return ctx._L.dsh_mappoint_update(ctx._h, store, P, arr(xyz, np.float32, C.c_float), arr(ptr, np.int32, C.c_int32), arr(kf, np.int32, C.c_int32),
                                      arr(idx, np.int32, C.c_int32), arr(ref, np.int32, C.c_int32), what, arr(out_d, np.uint8, C.c_uint8),
                                      arr(out_b, np.int32, C.c_int32), arr(out_n, np.float32, C.c_float), arr(out_m, np.float32, C.c_float),
                                      arr(out_m, np.float32, C.c_float), arr(out_s, np.int32, C.c_int32))


@pytest.mark.parametrize("bad", ["P", "what0", "what4", "no_desc", "no_geom", "ptr0", "ptr_dec", "too_many", "no_xyz"])
def test_bad_arguments_come_before_no_device(host_ctx, bad):
    kw = {}
    if bad == "P":
        kw = dict(P=-1)
    elif bad == "what0":
        kw = dict(what=0)
    elif bad == "what4":
        kw = dict(what=4)
    elif bad == "no_desc":
        kw = dict(what=1, desc=False)
    elif bad == "no_geom":
        kw = dict(what=2, geom=False)
    elif bad == "ptr0":
        kw = dict(ptr=np.array([1, 1], np.int32))
    elif bad == "ptr_dec":
        kw = dict(P=2, ptr=np.array([0, 2, 1], np.int32), kf=np.zeros(2, np.int32), idx=np.zeros(2, np.int32))
    elif bad == "too_many":
        kw = dict(ptr=np.array([0, 65536], np.int32), kf=np.arange(65536, dtype=np.int32), idx=np.zeros(65536, np.int32))
    elif bad == "no_xyz":
        from defslam_amd import _lib
        assert host_ctx._L.dsh_mappoint_update(host_ctx._h, None, 1, None, None, None, None, None, 3, None, None, None, None, None, None) == 1
        return
    assert _call(host_ctx, **kw) == 1


def test_host_only_context_has_no_device(host_ctx):
    from defslam_amd import mappoint, sft
    assert _call(host_ctx) == 4
    assert _call(host_ctx, what=2, desc=False) == 4
    assert _call(host_ctx, P=0) == 4
    with pytest.raises(sft.DshError, match="status 1"):
        mappoint.KeyFrameStore(host_ctx, 0)
    with pytest.raises(sft.DshError, match="status 4"):
        mappoint.KeyFrameStore(host_ctx, 16)
    with pytest.raises(sft.DshError, match="status 4"):
        mappoint.update(host_ctx, None, np.zeros((2, 3), np.float32), [[(0, 1)], []], [0, 0])


def test_store_entry_points_refuse_a_null_store(host_ctx):
    from defslam_amd import _lib
    L = host_ctx._L
    assert L.dsh_kfdb_add(None, None, None) == 1
    assert L.dsh_kfdb_set_bad(None, 0, 1) == 1
    assert L.dsh_kfdb_clear(None) == 1
    assert L.dsh_kfdb_destroy(None) == 1
    assert L.dsh_kfdb_count(None) == -1
