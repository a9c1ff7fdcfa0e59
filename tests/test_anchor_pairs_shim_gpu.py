"""The anchor shim (integration/anchor_pairs_hip.h) compiled against stand-in KeyFrame / MapPoint types and run on the device: for one
new keyframe the store route (AnchorPairsHIP, one call) and the host route (the reference's loops over the pointer graph) give the same
vMatchedIndices, own flags, query lists, has and n_no_ref, both equal the sequential restatement (tests/anchor_pairs_ref.py), and one
dropped match leaves the lists of the later anchors as the host's second walk does (DropMatchHIP)."""
import os

import pytest

import anchor_pairs_ref as A
import shim_run
import store_model

INTEG = shim_run.INTEG
MIN_PAIRS = 5


def test_anchor_shim_compiles_against_the_c_abi():
    shim_run.build()
    assert os.path.exists(shim_run.exe("anchor_pairs_shim_test"))
    src = open(os.path.join(INTEG, "anchor_pairs_hip.h")).read()
    assert "dsh_keyframe_anchors" in src and "defslam_hip_debug.h" not in src and "dsh_lab" not in src
    assert "anchor_pairs_hip.h" not in open(os.path.join(INTEG, "schwarp_database_hip.h")).read()


def ref_anchors(r, min_pairs, first=0):
    out = []
    for a in range(first, len(r["anchor_slot"])):
        ps, qs = slice(r["pair_ptr"][a], r["pair_ptr"][a + 1]), slice(r["query_ptr"][a], r["query_ptr"][a + 1])
        out.append((r["anchor_slot"][a], r["anchor_count"][a], r["anchor_pairs"][a], int(r["anchor_pairs"][a] >= min_pairs),
                    list(zip(r["pair_idx1"][ps], r["pair_idx2"][ps], map(int, r["pair_own"][ps]))), r["query_idx1"][qs]))
    return out


@pytest.mark.gpu
def test_anchor_shim_routes_agree_with_each_other_and_with_the_restatement(tmp_path):
    shim_run.build()
    rm = A.SCENES["n70_k5"][0]()
    slot = len(rm.kfs) - 1
    want = rm.keyframe_anchors(slot, MIN_PAIRS)
    anchors = ref_anchors(want, MIN_PAIRS)
    # the dropped match: a pair of a fitting anchor whose point a later fitting anchor pairs too
    points = [want["pair_point"][want["pair_ptr"][a]:want["pair_ptr"][a + 1]] for a in range(len(anchors))]
    drop = next((a, n) for a in range(len(anchors)) for n, p in enumerate(points[a]) if any(p in later for later in points[a + 1:]))
    point = want["pair_point"][want["pair_ptr"][drop[0]] + drop[1]]
    idx2 = anchors[drop[0]][4][drop[1]][1]
    store_model.write_scene(rm, tmp_path / "map.txt", f"{slot} {MIN_PAIRS} {drop[0]} {drop[1]}\n")
    shim_run.run("anchor_pairs_shim_test", tmp_path / "map.txt", tmp_path / "out.txt")
    got = {route: lists for (route, _), lists in store_model.parse_dump(tmp_path / "out.txt").items()}
    assert got["store"] == got["host"]
    assert got["store"]["anchors"] == anchors and got["store"]["has"] == [int(h) for h in want["has"]] and got["store"]["no_ref"] == want["n_no_ref"]
    # after the drop: (point, KF2) is erased and KF2's entry emptied; the later anchors' lists as a walk after the drop gives them
    assert got["store_drop"] == got["host_drop"]
    rm.erase_observation(point, slot)
    rm.kfs[slot].table[idx2] = -1
    again = rm.keyframe_anchors(slot, MIN_PAIRS)
    # the reference counts on its copy of :62, which still holds the point: the counts are the snapshot's, everything else a walk after the drop
    count = {a[0]: a[1] for a in anchors}
    later = [(a[0], count[a[0]]) + a[2:] for a in ref_anchors(again, MIN_PAIRS) if a[0] > anchors[drop[0]][0]]
    assert got["store_drop"]["anchors"] == later and later != anchors[drop[0] + 1:]
    lists = A.drop_match([[m[:2] for m in a[4]] for a in anchors], drop[0], idx2)
    assert lists[drop[0] + 1:] == [[m[:2] for m in a[4]] for a in later]
    # and a fresh call on the store after the same two mutations
    assert got["store_again"]["anchors"] == ref_anchors(again, MIN_PAIRS) and got["store_again"]["has"] == [int(h) for h in again["has"]]
