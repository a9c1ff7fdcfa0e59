"""CPU tests of the restatement of a keyframe's creation and connections (tests/keyframe_create_ref.py) against independent brute
force, and of the refusals of dsh_track_keyframe_candidate, dsh_keyframe_create and dsh_keyframe_update_connections that need no
device, on a host-only context.  No GPU."""
import numpy as np
import pytest

import keyframe_create_ref as KC
from surface_register_ref import centre_of


def brute(m, slot, th):
    """UpdateConnections from the set of live (point, keyframe) pairs alone -> (weights, pKFmax pair, ordered pairs)."""
    pairs = {(r[0], r[1]) for r in m.log if r[3]}
    w = {}
    for p in m.kfs[slot].table:
        if p >= 0 and not m.points[p].bad:
            for q, k in pairs:
                if q == p and k != slot:
                    w[k] = w.get(k, 0) + 1
    best = (0, -1)
    for k in range(len(m.kfs)):
        if w.get(k, 0) > best[0]:
            best = (w[k], k)
    conn = [(v, k) for k, v in w.items() if v >= th] or ([best] if w else [])
    return w, best, sorted(conn)[::-1]


def check(m, slot, th):
    first, parent = m.first_connection[slot], m.kfs[slot].parent
    w, best, order = brute(m, slot, th)
    r = m.update_connections(slot, th)
    assert dict(zip(r["counted_kf"], r["counted_w"])) == w and r["counted_kf"] == sorted(w)
    assert (r["max_weight"], r["max_kf"]) == best
    assert list(zip(r["ordered_w"], r["ordered_kf"])) == order
    sets = bool(w) and first and slot != 0
    assert r["parent_set"] == sets and r["parent"] == (order[0][1] if sets else parent) == m.kfs[slot].parent
    assert m.first_connection[slot] == (first and not sets)
    return r


EXPECT = {   # the hand cases worked out by hand: (counted, ordered as (kf, w), parent)
    "branches": ({0: 2, 1: 3, 2: 1}, [(1, 3), (0, 2)], 1),
    "empty": ({}, [], -1),
    "no_table": ({}, [], -1),
    "alone": ({}, [], -1),
    "th_met": ({0: 3, 1: 2}, [(0, 3)], 0),
    "th_missed": ({0: 3, 1: 2}, [(0, 3)], 0),
    "fallback_two_maxima": ({0: 1, 1: 2, 3: 2}, [(1, 2)], 1),
    "equal_connected": ({0: 1, 1: 2, 3: 2}, [(3, 2), (1, 2)], 3),
    "slot0": ({1: 2, 2: 1}, [(1, 2), (2, 1)], -1),
}


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_hand_cases_reach_every_branch(name):
    m, slot, th = KC.hand_cases()[name]
    counted, ordered, parent = EXPECT[name]
    r = check(m, slot, th)
    assert dict(zip(r["counted_kf"], r["counted_w"])) == counted
    assert list(zip(r["ordered_kf"], r["ordered_w"])) == ordered
    assert r["parent"] == parent and r["parent_set"] == (parent >= 0)
    if name == "slot0":
        assert m.first_connection[0]                       # mnId == 0 keeps its flag
    if name in ("empty", "no_table", "alone"):
        assert m.first_connection[slot] and r["max_kf"] == -1 and r["max_weight"] == 0


def test_second_call_keeps_the_parent_and_recomputes_the_lists():
    m, slot, th = KC.hand_cases()["equal_connected"]
    assert check(m, slot, th)["parent"] == 3
    for p in (0, 1, 2, 3):                                 # keyframe 0 overtakes: it observes all four held points
        m.add_observation(p, 0)
    assert m.add_observation(3, 2)
    r = check(m, slot, th)
    assert r["ordered_kf"] == [0, 3, 1] and r["ordered_w"] == [4, 2, 2] and r["parent"] == 3 and not r["parent_set"]


def test_a_preset_parent_is_overwritten_by_the_first_connection():
    m, slot, th = KC.hand_cases()["th_met"]
    m.kfs[slot].parent = 2                                 # ChangeParent: mbFirstConnection stays true
    r = check(m, slot, th)
    assert r["parent_set"] and r["parent"] == 0 and m.kfs[slot].parent == 0


@pytest.mark.parametrize("seed,K,N,P,th", [(0, 1, 5, 4, 1), (1, 2, 9, 6, 2), (2, 12, 40, 30, 3), (3, 65, 70, 50, 100), (4, 30, 64, 20, 1), (5, 7, 0, 5, 1)])
def test_random_scenes_against_brute_force(seed, K, N, P, th):
    m, slot = KC.random_connections(seed, K, N, P, max_obs=9)
    check(m, slot, th)
    check(m, slot, max(th - 1, 1))                         # the second call: no parent any more


def test_all_weights_equal_orders_by_slot():
    m, slot = KC.random_connections(6, 9, 12, 5, max_obs=9, p_bad=0.0, equal=True)
    r = check(m, slot, 1)
    assert r["ordered_kf"] == list(range(8, -1, -1)) and len(set(r["ordered_w"])) == 1 and r["max_kf"] == 0 and r["parent"] == 8


def test_candidate_and_create():
    m = KC.topology(2, 5, {0: [0, 1], 1: [2]}, bad_points=(3,))
    for p, k in ((0, 0), (1, 0), (3, 1)):
        m.add_observation(p, k)
    m.facet = {0: (0, 1, 2), 3: (0, 1, 2), 2: (0, 1, 2)}
    cand = m.end_frame_candidate([0, 2, -1, 3, 1, 4])      # 2 and 4 have no observation: cleaned; 3 is bad and stays (no isBad test)
    assert cand == [0, -1, -1, 3, 1, -1]
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = (1, 2, 3)
    # appearance is all or nothing in a model: give the two old keyframes theirs
    for k in m.kfs:
        k.has_appearance, k.Ow, k.desc, k.octave, k.scale_factors = True, np.zeros(3, np.float32), np.zeros((len(k.table), 32), np.uint8), np.zeros(len(k.table), np.int32), np.ones(1, np.float32)
    r = m.create(np.zeros((6, 32), np.uint8), np.zeros(6, np.int32), np.ones(1, np.float32), T, kpn=np.zeros((6, 2), np.float32))
    assert r["slot"] == 2 and r["n_held"] == 3 and r["n_snapshot"] == 1          # 0: held, good, facet; 3: bad; 1: no facet
    assert r["Ow"].tobytes() == centre_of(T).tobytes() == np.float32([-1, -2, -3]).tobytes()
    assert m.kfs[2].table == cand and m.kfs[2].parent == -1 and not m.kfs[2].bad and m.first_connection[2]
    assert m.get_snapshot(2)[0].tolist() == [0, -1, -1, -1, -1, -1] and 2 in m.surface and m.candidate == cand   # not consumed
    assert not any(s == 2 for pt in m.points for s in pt.obs)                    # no observation is added


# ---- the refusals that need no device -------------------------------------------------------------------------------------------------------

def test_refusals_on_a_host_only_context(host_ctx):
    from defslam_amd import localmap, mappoint
    from defslam_amd.sft import DshError
    st = localmap.MapPointStore(host_ctx)
    kf = mappoint.MpKeyFrame(np.zeros(3, np.float32), np.zeros((2, 32), np.uint8), np.zeros(2, np.int32), np.ones(1, np.float32))
    T = np.eye(4, dtype=np.float32)
    for call, status, words in (
            (lambda: st.update_connections(0), 1, "dsh_keyframe_update_connections: slot outside the store"),
            (lambda: st.update_connections(-1), 1, "slot outside the store"),
            (lambda: st.create_keyframe(None, kf, T, points=[-1, -1]), 1, "dsh_keyframe_create: kfdb is NULL"),
            (lambda: st.keyframe_candidate(), 4, "dsh_track_keyframe_candidate: host-only"),
            (lambda: st.keyframe_candidate(-1), 1, "capacity < 0")):
        with pytest.raises(DshError) as e:
            call()
        assert f"status {status}" in str(e.value) and words in str(e.value), str(e.value)
    assert st.n_keyframes == 0
    L = host_ctx._L
    assert L.dsh_keyframe_create(st._h, None, None) == 1 and L.dsh_keyframe_create(None, None, None) == 1
    assert L.dsh_keyframe_update_connections(None, 0, 100, 0, None, None, None, None, None) == 1
    st.close()
