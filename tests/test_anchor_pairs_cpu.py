"""CPU tests of the anchor keyframes of a new keyframe: the restatement (tests/anchor_pairs_ref.py) against an independent brute force
over flat record arrays, the conditions the generated maps of the GPU tests must meet, and the ABI of the new entries without a GPU
(symbols, the refusals an empty host-only store can reach and their order, a detached store).  A host-only store stays empty -- every
mutation is refused -- so the refusals that need a stored keyframe, point or record (an index outside the keyframe, repeated ids,
lists that do not fit, live records without an index) are in tests/test_anchor_pairs_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import anchor_pairs_ref as A

OK, ARG, STATE, NODEV = 0, 1, 3, 4
NEW_ENTRIES = ["dsh_point_store_add_observations_indexed", "dsh_point_store_set_reference_keyframes", "dsh_point_store_get_reference_keyframes",
               "dsh_keyframe_anchors"]


def brute_force(rm, slot):
    """Per keyframe a with a vote: the multiset of (idx1, idx2, point, own) and the set of query entries, from flat arrays and sets
    instead of the per-point dictionaries: the live records are the log without its blanked records."""
    live = {(p, k): i for p, k, i, alive in rm.log if alive}
    assert live == {(p, k): i for p, pt in enumerate(rm.points) for k, i in pt.obs.items()}
    in_new = {p for (p, k) in live if k == slot}
    good = [p for p in rm.kfs[slot].table if p >= 0 and not rm.points[p].bad]
    votes = {}
    for p in good:
        if rm.points[p].ref >= 0:
            votes[rm.points[p].ref] = votes.get(rm.points[p].ref, 0) + 1
    out = {}
    for a in votes:
        sees_a = {p for (p, k) in live if k == a}
        pairs = sorted((live[(p, a)], live[(p, slot)], p, rm.points[p].ref == a) for p in good if p in in_new and p in sees_a)
        queries = {j for j, q in enumerate(rm.kfs[a].table) if q >= 0 and not rm.points[q].bad and q not in in_new}
        out[a] = (votes[a], pairs, queries)
    return out, sum(1 for p in good if rm.points[p].ref < 0)


def check_against_brute_force(rm, min_pairs):
    slot = len(rm.kfs) - 1
    r = rm.keyframe_anchors(slot, min_pairs)
    bf, n_no_ref = brute_force(rm, slot)
    assert r["anchor_slot"] == sorted(bf) and r["n_no_ref"] == n_no_ref
    assert r["has"] == [p >= 0 for p in rm.kfs[slot].table]
    for n, a in enumerate(r["anchor_slot"]):
        votes, pairs, queries = bf[a]
        assert r["anchor_count"][n] == votes and r["anchor_pairs"][n] == len(pairs)
        ps, qs = slice(r["pair_ptr"][n], r["pair_ptr"][n + 1]), slice(r["query_ptr"][n], r["query_ptr"][n + 1])
        got = list(zip(r["pair_idx1"][ps], r["pair_idx2"][ps], r["pair_point"][ps], r["pair_own"][ps]))
        if len(pairs) < min_pairs:
            assert got == [] and r["query_idx1"][qs] == []
            continue
        assert sorted(got) == pairs
        assert r["query_idx1"][qs] == sorted(queries)                         # ascending entries of the anchor's table
        assert [rm.kfs[a].table[j] for j in r["query_idx1"][qs]] == r["query_point"][qs]
        held = [i for i, p in enumerate(rm.kfs[slot].table) if p in set(r["pair_point"][ps])]
        assert [rm.kfs[slot].table[i] for i in held] == r["pair_point"][ps]      # in the order of the new keyframe's entries
    return r


@pytest.mark.parametrize("name", sorted(A.SCENES))
def test_restatement_against_the_brute_force_on_the_scenes_of_the_gpu_tests(name):
    make, min_pairs = A.SCENES[name]
    check_against_brute_force(make(), min_pairs)


@pytest.mark.parametrize("seed", range(6))
def test_restatement_against_the_brute_force_on_seeded_random_maps(seed):
    rng = np.random.default_rng(100 + seed)
    rm = A.make_map(50 + seed, int(rng.integers(20, 200)), int(rng.integers(2, 12)), int(rng.integers(4, 60)))
    check_against_brute_force(rm, int(rng.integers(0, 12)))


def test_the_generated_maps_hold_every_case_the_gpu_tests_need():
    """A condition on the inputs of the GPU tests, checked on the restatement alone."""
    for name, (make, min_pairs) in A.SCENES.items():
        rm = make()
        slot = len(rm.kfs) - 1
        table = rm.kfs[slot].table
        r = rm.keyframe_anchors(slot, min_pairs)
        held = [p for p in table if p >= 0]
        erased = {(p, k) for p, k, _, alive in rm.log if not alive}
        assert len(held) > len(set(held)), name                                                  # a point held by two entries
        assert any(rm.points[p].bad for p in held), name                                                # a bad point
        assert any((p, slot) in erased for p in held), name                                      # an erased record of (p, slot)
        assert any(k != slot and p in held for p, k in erased), name                             # and of (p, a)
        assert any(not rm.points[p].bad and slot not in rm.points[p].obs and (p, slot) not in erased for p in held), name  # does not observe the keyframe yet
        assert r["n_no_ref"] > 0, name
        assert slot in r["anchor_slot"], name                                                    # a == slot
        a = r["anchor_slot"].index(slot)
        ps = slice(r["pair_ptr"][a], r["pair_ptr"][a + 1])
        assert r["anchor_pairs"][a] < min_pairs or r["pair_idx1"][ps] == r["pair_idx2"][ps]
        assert 0 in r["pair_own"] and 1 in r["pair_own"], name                                   # shared with an anchor that is not its reference
        assert len(r["query_idx1"]) > 0, name
    r = A.SCENES["a70"][0]().keyframe_anchors(75, 3)
    assert len(r["anchor_slot"]) >= 70 and min(r["anchor_pairs"]) < 3 <= max(r["anchor_pairs"])
    r = A.SCENES["n70_k5"][0]().keyframe_anchors(4, 0)                                            # every anchor listed: a == slot is the last
    ps = slice(r["pair_ptr"][-2], r["pair_ptr"][-1])
    assert r["anchor_slot"][-1] == 4 and len(r["pair_idx1"][ps]) > 0 and r["pair_idx1"][ps] == r["pair_idx2"][ps]


def test_min_pairs_boundary_on_the_restatement():
    """An anchor with min_pairs - 1 pairs keeps its entry and contributes nothing; one with exactly min_pairs contributes all."""
    m = 20
    r = A.threshold_map(m).keyframe_anchors(2, m)
    assert r["anchor_slot"] == [0, 1] and r["anchor_count"] == [m - 1, m - 1] and r["anchor_pairs"] == [m - 1, m]
    assert r["pair_ptr"] == [0, 0, m] and r["query_ptr"] == [0, 0, 1]
    assert r["pair_own"] == [False] + [True] * (m - 1)                # point 0 belongs to keyframe 0 and is the first entry
    assert r["pair_idx1"][0] == m and r["pair_idx2"][0] == 0 and r["query_idx1"] == [m + 1]
    check_against_brute_force(A.threshold_map(m), m)


def test_a_dropped_match_leaves_the_lists_of_the_later_anchors():
    lists = [[(1, 5), (2, 6)], [(9, 5), (8, 7)], [(3, 5)]]
    assert A.drop_match(lists, 0, 5) == [[(1, 5), (2, 6)], [(8, 7)], []]
    assert A.drop_match(lists, 1, 5) == [[(1, 5), (2, 6)], [(9, 5), (8, 7)], []]


# ---- the ABI without a GPU ---------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_bound_declared_and_wrapped():
    from defslam_amd import _lib, localmap
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "defslam_hip.h")).read()
    for n in NEW_ENTRIES:
        assert n in _lib.EXPORTED_SYMBOLS and getattr(L, n).argtypes is not None, n
        assert f"int {n}(dsh_mpdb* db" in header, n
    assert "} dsh_anchor_lists;" in header and C.sizeof(_lib.AnchorListsC) == 136
    for m in ("set_reference_keyframes", "get_reference_keyframes", "keyframe_anchors"):
        assert callable(getattr(localmap.MapPointStore, m))
    assert "pair_own" in localmap.KeyframeAnchors.__dataclass_fields__


def _lists(keep, **over):
    from defslam_amd import _lib
    a = {n: np.zeros(4, np.int32) for n in ("anchor_slot", "anchor_count", "anchor_pairs", "pair_ptr", "pair_idx1", "pair_idx2", "pair_point",
                                             "query_ptr", "query_idx1", "query_point")}
    own = np.zeros(4, np.uint8)
    keep.append((a, own))
    kw = dict(anchor_capacity=2, pair_capacity=4, query_capacity=4, max_matrix_bytes=0, pair_own=own.ctypes.data_as(C.POINTER(C.c_uint8)),
              **{n: v.ctypes.data_as(C.POINTER(C.c_int32)) for n, v in a.items()})
    kw.update(over)
    r = _lib.AnchorListsC(**kw)
    keep.append(r)
    return C.byref(r)


def _rows(keep):
    """(name, arguments after the store handle, expected status, a word of the message) for an EMPTY store on a host-only context."""
    a = dict(z=np.zeros(2, np.int32), m1=np.full(2, -1, np.int32))
    keep.append(a)
    z, m1 = (a[n].ctypes.data_as(C.POINTER(C.c_int32)) for n in ("z", "m1"))
    add, st, gt, an = NEW_ENTRIES
    return [
        (add, (0, None, None, None), NODEV, "host-only"),
        (add, (-1, None, None, None), ARG, "n < 0"),
        (add, (1, None, z, z), ARG, "NULL"),
        (add, (1, z, None, z), ARG, "NULL"),
        (add, (1, z, z, None), ARG, "idx is NULL"),
        (add, (1, z, z, z), ARG, "point id outside the store"),
        (st, (0, None, None), NODEV, "host-only"),
        (st, (-1, None, None), ARG, "n < 0"),
        (st, (1, None, z), ARG, "NULL"),
        (st, (1, z, m1), ARG, "point id 0 outside the store"),
        (gt, (0, None, None), NODEV, "host-only"),
        (gt, (1, None, z), ARG, "NULL"),
        (gt, (1, z, z), ARG, "point id 0 outside the store"),
        (an, (0, 20, _lists(keep)), ARG, "slot outside the store"),                   # an empty store has no keyframe
        (an, (-1, 20, _lists(keep)), ARG, "slot outside the store"),
        (an, (0, 20, None), ARG, "out is NULL"),
    ]


def test_host_only_status_of_every_refusal(host_ctx):
    """On a host-only context a malformed call is DSH_ERR_ARG with a message naming the entry point, a well-formed one
    DSH_ERR_NO_DEVICE saying "host-only" -- arguments first, then the device; a NULL store is DSH_ERR_ARG."""
    from test_local_map_cpu import _raw_store
    L = host_ctx._L
    msg = lambda: L.dsh_last_error(host_ctx._h).decode()
    rc, h = _raw_store(L, host_ctx._h)
    assert rc == OK and h
    keep = []
    rows = _rows(keep)
    assert {r[0] for r in rows} == set(NEW_ENTRIES)
    for name, args, want, word in rows:
        fn = getattr(L, name)
        assert fn(h, *args) == want, (name, args, msg())
        assert name in msg() and word in msg(), (name, word, msg())
        assert fn(None, *args) == ARG, (name, "NULL store")
    assert L.dsh_mpdb_point_count(h) == 0
    assert L.dsh_mpdb_destroy(h) == OK


def test_a_detached_store_refuses_every_new_entry():
    from defslam_amd import sft
    from test_local_map_cpu import _raw_store
    ctx = sft.Context(-1)
    L = ctx._L
    rc, h = _raw_store(L, ctx._h)
    assert rc == OK
    ctx.close()                                    # dsh_destroy detaches the store
    keep = []
    for name, args, _, _ in _rows(keep):
        assert getattr(L, name)(h, *args) == ARG, name
    assert L.dsh_mpdb_destroy(h) == OK
