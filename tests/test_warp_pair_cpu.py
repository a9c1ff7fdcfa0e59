"""CPU tests of dsh_keyframe_set_view / dsh_keyframe_warp_pair: the two formulations of tests/warp_pair_ref.py -- the literal
transcription of the reference's loops and the elections the header states for the device -- agree on random maps and on the hand-made
cases; the filter's pairing of residuals; the float32 inverse sigma; and the order of checks of the new entries on a host-only context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import warp_pair_ref as WP
from conftest import ROOT

OK, ARG, STATE, NODEV = 0, 1, 3, 4
NEW_ENTRIES = ("dsh_keyframe_set_view", "dsh_keyframe_get_view", "dsh_keyframe_warp_pair")


def _random_map(seed):
    """An anchor (slot 0), two more keyframes, the new keyframe (slot 3): tables and records that need not agree -- points under two
    entries of the anchor, records whose index names an entry that holds another point, points anchored in the new keyframe, points with
    two or three observations -- and lists with repeated points, shared idx2 and entries on empty key points."""
    rng = np.random.default_rng(seed)
    m = WP.WarpPairRef()
    N, P = 24, 30
    for _ in range(4):
        m.add_keyframe([-1] * N)
    for p in range(P):
        m.add_point(ref=int(rng.choice([0, 0, 0, 1, 3])), bad=rng.uniform() < 0.05)
    for p in range(P):
        for k in rng.permutation(4)[:rng.integers(1, 5)]:
            i = int(rng.integers(0, N))
            if m.add_observation(p, int(k), i) and rng.uniform() < 0.85:
                m.kfs[int(k)].table[i] = p
    for k in (0, 3):                                                            # entries that hold a point without a record
        for i in rng.integers(0, N, 4):
            m.kfs[k].table[int(i)] = int(rng.integers(0, P))
    return m, rng, N


@pytest.mark.parametrize("seed", range(40))
def test_the_two_formulations_agree_on_random_maps(seed):
    m, rng, N = _random_map(seed)
    a, b = WP.clone(m), WP.clone(m)
    P, Q = 10, 8
    i1, i2 = rng.integers(0, N, P), rng.permutation(N)[:P]
    q1 = np.sort(rng.permutation(N)[:Q])
    filt = rng.uniform(size=P) < 0.3
    free = [j for j in range(N) if m.kfs[3].table[j] == -1 or j in i2[filt]]
    match = np.array([int(rng.choice(free)) if free and rng.uniform() < 0.7 else -1 for _ in range(Q)])   # several queries on one free key point
    ra, rb = a.filter_register_seq(0, 3, i1, i2, filt, q1, match), b.filter_register_par(0, 3, i1, i2, filt, q1, match)
    assert ra[0] == rb[0] and all(np.array_equal(x, y) for x, y in zip(ra[1:], rb[1:]))
    assert _same(a, b)
    assert [r[:3] for r in a.log] == [r[:3] for r in b.log]                     # the records in the same order
    kept = ra[0]
    drop = rng.uniform(size=len(kept)) < 0.4
    sa, stored_a, ca = a.records_drops_seq(0, 3, kept, drop)
    sb, stored_b, cb, rounds = b.records_drops_par(0, 3, kept, drop)
    assert np.array_equal(sa, sb), (sa, sb)
    assert stored_a == stored_b and ca == cb and rounds <= len(kept) + 1
    assert _same(a, b)


def _same(a, b):
    sa, sb = a.state(), b.state()
    return all(np.array_equal(sa[n], sb[n]) for n in ("bad", "n_obs", "ref")) and sa["obs"] == sb["obs"] and sa["tables"] == sb["tables"]


def _hand_map():
    """Anchor 0, lenders 1 and 2, new keyframe 3, six key points each.  p0 .. p3 observed by all four keyframes at entry p; p4 by the
    anchor and the new keyframe alone; p5 by the anchor alone."""
    m = WP.WarpPairRef()
    for _ in range(4):
        m.add_keyframe([-1] * 6)
    for p in range(6):
        m.add_point(ref=0)
        for k in ((0, 1, 2, 3) if p < 4 else (0, 3) if p == 4 else (0,)):
            m.add_observation(p, k, p)
            m.kfs[k].table[p] = p
    return m


def test_hand_made_cases_of_the_registration():
    # two queries (entries 4' and 5 of the anchor) on the free key point 5 of the new keyframe: the later one holds the entry, both get a record
    for route in ("filter_register_seq", "filter_register_par"):
        m = _hand_map()
        m.kfs[3].table[4] = -1                                                  # p4's entry: cleared as by the filter
        m.erase_observation(4, 3)
        kept, ps, qs, qp, qa = getattr(m, route)(0, 3, [0, 1], [0, 1], [False, True], [4, 5], [5, 5])
        assert kept == [(0, 0, 0), (4, 5, 2), (5, 5, 3)] and ps.tolist() == [WP.UNFITTED, WP.FILTERED]
        assert qp.tolist() == [4, 5] and qa.tolist() == [True, True] and m.kfs[3].table[5] == 5 and m.kfs[3].table[1] == -1
        assert m.live(1, 3) and m.points[4].obs[3] == 5 and m.points[5].obs[3] == 5     # the filtered pair keeps its record
        # a point under two entries of the anchor: the second query finds the record the first one added
        m = _hand_map()
        m.kfs[0].table[3] = 5
        kept, ps, qs, qp, qa = getattr(m, route)(0, 3, [0], [0], [False], [3, 5], [4, -1])
        assert qa.tolist() == [True, False] and qs.tolist() == [WP.UNFITTED, WP.NO_MATCH] and m.kfs[3].table[4] == 5
        # a query landing on the entry the filter just cleared
        m = _hand_map()
        kept, ps, qs, qp, qa = getattr(m, route)(0, 3, [1], [1], [True], [5], [1])
        assert m.kfs[3].table[1] == 5 and m.live(1, 3) and m.live(5, 3) and kept == [(5, 1, 1)]


def test_hand_made_cases_of_the_drops():
    for route in ("records_drops_seq", "records_drops_par"):
        # a shared idx2: the later entry finds the key point empty
        m = _hand_map()
        st = getattr(m, route)(0, 3, [(0, 0, 0), (1, 0, 1), (2, 2, 2)], [True, True, False])
        assert st[0].tolist() == [WP.DROPPED, WP.SKIPPED, WP.STORED] and st[1] == [(2, 2)] and not m.live(0, 3) and m.points[0].n_obs == 3
        # a drop that leaves two observations: setBadFlag, and the later entry that names the point through the anchor is skipped
        m = _hand_map()
        m.kfs[3].table[5] = 4                                                   # p4 under a second key point of the new keyframe
        st = getattr(m, route)(0, 3, [(4, 4, 0), (4, 5, 1), (3, 3, 2)], [True, False, False])
        assert st[0].tolist() == [WP.DROPPED, WP.SKIPPED, WP.STORED] and m.points[4].bad and not m.points[4].obs and m.kfs[0].table[4] == -1
        assert st[2]["n_set_bad"] == 1 and st[2]["n_found"] == 1 and st[2]["n_entries"] == 1
        # the chain: entry 0 sets p4 bad, so entry 1 (p1 == p4) never drops p0's record, so entry 2 stores
        m = _hand_map()
        m.kfs[3].table[5] = 0
        st = getattr(m, route)(0, 3, [(4, 4, 0), (4, 5, 1), (0, 0, 2)], [True, True, False])
        assert st[0].tolist() == [WP.DROPPED, WP.SKIPPED, WP.STORED] and m.live(0, 3)
        # a point anchored elsewhere is kept, not stored
        m = _hand_map()
        m.points[2].ref = 1
        st = getattr(m, route)(0, 3, [(2, 2, 0)], [False])
        assert st[0].tolist() == [WP.KEPT] and st[1] == []


def test_the_filter_pairs_neighbouring_residuals():
    """DefORBmatcher.cc:167-175 on [x_0 .. x_3, y_0 .. y_3]: match i is judged by entries 2i and 2i + 1."""
    # match 0 has x-residual 4 and match 1 x-residual 3: entries 0 and 1, so "match 0" goes (16 + 9 > 20) and match 1 stays
    assert WP.filter_flags(np.array([4.0, 3.0, 0, 0, 0, 0, 0, 0]), 4).tolist() == [True, False, False, False]
    # the y-residuals of matches 0 and 1 are entries 4 and 5: they are charged to match 2
    assert WP.filter_flags(np.array([0, 0, 0, 0, 4.0, 3.0, 0, 0]), 4).tolist() == [False, False, True, False]
    # both components of match 0 (entries 0 and 4) never meet: 3^2 + 0 and 4^2 + 0 stay below 20
    assert not WP.filter_flags(np.array([3.0, 0, 0, 0, 4.0, 0, 0, 0]), 4).any()
    # 25 <= 5.77^2: the block is not scaled; 36 > 5.77^2: every residual times sqrt(5.77 / 6)
    small, big = np.array([4.0, 3.0, 0, 0, 0, 0, 0, 0]), np.array([6.0, 0, 0, 0, 0, 0, 0, 0])
    assert np.array_equal(WP.corrected(small, 4), small)
    assert np.array_equal(WP.corrected(big, 4), big * np.sqrt(5.77 / np.sqrt(36.0)))
    assert WP.filter_flags(big, 4).tolist() == [True, False, False, False]      # 36 * 5.77 / 6 = 34.6 > 20
    # 4.6^2 = 21.16 > 20 alone, but in a block of |r|^2 = 84.64 it is scaled by 5.77 / 9.2: 13.3 and the match stays
    assert not WP.filter_flags(np.array([4.6, 0, 4.6, 0, 4.6, 0, 4.6, 0]), 4).any()


def test_inverse_sigma_is_float32_throughout():
    sf = (1.2 ** np.arange(8)).astype(np.float32)
    got = WP.inv_sigma(sf, np.arange(8))
    assert got.dtype == np.float32
    for o in range(8):
        s2 = np.float32(sf[o] * sf[o])
        assert got[o] == np.sqrt(np.float32(np.float32(1.0) / s2))


def test_the_scene_generator_and_its_map():
    from defslam_amd import synth
    sc = synth.make_warp_pair_scene(96, 20, 10, n_anchors=2, seed=1, nu=5, nv=6)
    m = WP.build_model(sc)
    assert len(m.kfs) == 5 and len(m.points) == 60
    A = sc["anchors"][1]
    assert np.all(np.diff(A["query_idx1"]) > 0) and len(set(A["pair_idx2"]) | set(sc["anchors"][0]["pair_idx2"])) == 40
    for i1, i2 in zip(A["pair_idx1"], A["pair_idx2"]):
        assert m.kfs[1].table[i1] == m.kfs[4].table[i2] >= 0
    named = np.concatenate([np.r_[a["pair_idx2"], a["query_idx2"]] for a in sc["anchors"]])
    assert np.array_equal(sc["px2"][named], (sc["kpn2"][named] * np.float32(sc["K"][:2]) + np.float32(sc["K"][2:])).astype(np.float32))


def test_new_prototypes_stay_out_of_the_host_only_table():
    header = open(os.path.join(ROOT, "include", "defslam_hip.h")).read()
    takes = set(re.findall(r"\b(dsh_[a-z0-9_]+)\s*\((?:[^)]*\b(?:dsh_ctx|dsh_diffdb|dsh_kfdb|dsh_comm)\b)", header))
    assert not takes & set(NEW_ENTRIES), takes & set(NEW_ENTRIES)


def test_order_of_checks_on_a_host_only_context(host_ctx):
    """Arguments first, each DSH_ERR_ARG with a message that names the entry.  A host-only store stays empty, so every entry names a
    keyframe that is not there; what a host-only context answers past the arguments is "host-only" (dsh_mpdb_add_keyframe, the call
    these entries need first)."""
    from defslam_amd import _lib
    from test_local_map_cpu import _raw_store
    L = host_ctx._L
    msg = lambda: L.dsh_last_error(host_ctx._h).decode()
    rc, h = _raw_store(L, host_ctx._h)
    assert rc == OK and h
    px = np.zeros((4, 2), np.float32)
    view = _lib.KeyframeViewC(4, px.ctypes.data_as(_lib.c_float_p), 500, 500, 320, 240, 0, 640, 0, 480, 64, 48, _lib.BbsC(0.0, 1.0, 5, 0.0, 1.0, 6, 2))
    idx = np.zeros(4, np.int32)
    ip = idx.ctypes.data_as(_lib.c_i32_p)
    inp = _lib.WarpPairInputC(host_ctx._h, None, None, 1, 0, 1, 1e-2, 20, 3, 2.0, 50, 4, ip, ip, 0, ip)
    res = _lib.WarpPairResultC()
    assert L.dsh_keyframe_set_view(h, 0, None) == ARG and "dsh_keyframe_set_view: view is NULL" in msg()
    assert L.dsh_keyframe_set_view(h, 0, C.byref(view)) == ARG and "dsh_keyframe_set_view: slot outside the store" in msg()
    assert L.dsh_keyframe_get_view(h, 0, None, None) == ARG and "dsh_keyframe_get_view: view is NULL" in msg()
    assert L.dsh_keyframe_get_view(h, 0, C.byref(view), None) == ARG and "slot outside the store" in msg()
    assert L.dsh_keyframe_warp_pair(h, None, C.byref(res)) == ARG and "dsh_keyframe_warp_pair: in is NULL" in msg()
    assert L.dsh_keyframe_warp_pair(h, C.byref(inp), None) == ARG and "out is NULL" in msg()
    assert L.dsh_keyframe_warp_pair(h, C.byref(inp), C.byref(res)) == ARG and "keyframe store is NULL" in msg()
    other = _lib.WarpPairInputC(None, None, None, 1, 0, 1, 1e-2, 20, 3, 2.0, 50, 4, ip, ip, 0, ip)
    assert L.dsh_keyframe_warp_pair(h, C.byref(other), C.byref(res)) == ARG and "not the context of the store" in msg()
    for name, args in (("dsh_keyframe_set_view", (0, C.byref(view))), ("dsh_keyframe_get_view", (0, C.byref(view), None)),
                       ("dsh_keyframe_warp_pair", (C.byref(inp), C.byref(res)))):
        assert getattr(L, name)(None, *args) == ARG, name
    assert L.dsh_mpdb_add_keyframe(h, 0, None, -1, 0, None) == NODEV and "host-only" in msg()
    assert L.dsh_mpdb_destroy(h) == OK
