"""The anchor shim (integration/anchor_pairs_hip.h) compiled against stand-in KeyFrame / MapPoint types and run on the device: for one
new keyframe the store route (AnchorPairsHIP, one call) and the host route (the reference's loops over the pointer graph) give the same
vMatchedIndices, own flags, query lists, has and n_no_ref, both equal the sequential restatement (tests/anchor_pairs_ref.py), and one
dropped match leaves the lists of the later anchors as the host's second walk does (DropMatchHIP)."""
import os
import subprocess

import pytest

import anchor_pairs_ref as A
from conftest import ROOT

INTEG = os.path.join(ROOT, "integration")
MIN_PAIRS = 5


def test_anchor_shim_compiles_against_the_c_abi():
    subprocess.run(["make", "-C", INTEG], check=True, capture_output=True)
    assert os.path.exists(os.path.join(INTEG, "build", "anchor_pairs_shim_test"))
    src = open(os.path.join(INTEG, "anchor_pairs_hip.h")).read()
    assert "dsh_keyframe_anchors" in src and "defslam_hip_debug.h" not in src and "dsh_lab" not in src
    assert "anchor_pairs_hip.h" not in open(os.path.join(INTEG, "schwarp_database_hip.h")).read()


def write_map(path, rm, slot, min_pairs, drop_anchor, drop_pair):
    with open(path, "w") as f:
        f.write(f"{len(rm.bad)} {len(rm.tables)}\n")
        for b, r in zip(rm.bad, rm.ref):
            f.write(f"{int(b)} {r}\n")
        for t in rm.tables:
            f.write(" ".join(map(str, [len(t)] + t)) + "\n")
        f.write(f"{len(rm.log)}\n" + "".join(f"{p} {k} {i}\n" for p, k, i in rm.log))
        f.write(f"{len(rm.erased)}\n" + "".join(f"{p} {k}\n" for p, k in rm.erased))
        f.write(f"{slot} {min_pairs} {drop_anchor} {drop_pair}\n")


def parse(path):
    """route -> dict(anchors=[(slot, count, n_pairs, fits, [(idx1, idx2, own)], [j])], has=[..], no_ref=n)"""
    out = {}
    for line in open(path):
        w = line.split()
        r = out.setdefault(w[0], dict(anchors=[], has=None, no_ref=None))
        if w[1] == "anchor":
            pairs, queries = (part.split() for part in line.split("|")[1:])
            r["anchors"].append((int(w[2]), int(w[3]), int(w[4]), int(w[5]), [tuple(map(int, p.split(":"))) for p in pairs], list(map(int, queries))))
        elif w[1] == "has":
            r["has"] = [int(x) for x in w[2:]]
        else:
            r["no_ref"] = int(w[2])
    return out


def ref_anchors(r, min_pairs, first=0):
    out = []
    for a in range(first, len(r["anchor_slot"])):
        ps, qs = slice(r["pair_ptr"][a], r["pair_ptr"][a + 1]), slice(r["query_ptr"][a], r["query_ptr"][a + 1])
        out.append((r["anchor_slot"][a], r["anchor_count"][a], r["anchor_pairs"][a], int(r["anchor_pairs"][a] >= min_pairs),
                    list(zip(r["pair_idx1"][ps], r["pair_idx2"][ps], map(int, r["pair_own"][ps]))), r["query_idx1"][qs]))
    return out


@pytest.mark.gpu
def test_anchor_shim_routes_agree_with_each_other_and_with_the_restatement(tmp_path):
    subprocess.run(["make", "-C", INTEG], check=True, capture_output=True)
    exe = os.path.join(INTEG, "build", "anchor_pairs_shim_test")
    rm = A.SCENES["n70_k5"][0]()
    slot = len(rm.tables) - 1
    want = rm.keyframe_anchors(slot, MIN_PAIRS)
    anchors = ref_anchors(want, MIN_PAIRS)
    # the dropped match: a pair of a fitting anchor whose point a later fitting anchor pairs too
    points = [want["pair_point"][want["pair_ptr"][a]:want["pair_ptr"][a + 1]] for a in range(len(anchors))]
    drop = next((a, n) for a in range(len(anchors)) for n, p in enumerate(points[a]) if any(p in later for later in points[a + 1:]))
    point = want["pair_point"][want["pair_ptr"][drop[0]] + drop[1]]
    idx2 = anchors[drop[0]][4][drop[1]][1]
    write_map(tmp_path / "map.txt", rm, slot, MIN_PAIRS, *drop)
    subprocess.run([exe, str(tmp_path / "map.txt"), str(tmp_path / "out.txt")], check=True, timeout=120)
    got = parse(tmp_path / "out.txt")
    assert got["store"] == got["host"]
    assert got["store"]["anchors"] == anchors and got["store"]["has"] == [int(h) for h in want["has"]] and got["store"]["no_ref"] == want["n_no_ref"]
    # after the drop: (point, KF2) is erased and KF2's entry emptied; the later anchors' lists as a walk after the drop gives them
    assert got["store_drop"] == got["host_drop"]
    rm.erase_observation(point, slot)
    rm.tables[slot][idx2] = -1
    again = rm.keyframe_anchors(slot, MIN_PAIRS)
    # the reference counts on its copy of :62, which still holds the point: the counts are the snapshot's, everything else a walk after the drop
    count = {a[0]: a[1] for a in anchors}
    later = [(a[0], count[a[0]]) + a[2:] for a in ref_anchors(again, MIN_PAIRS) if a[0] > anchors[drop[0]][0]]
    assert got["store_drop"]["anchors"] == later and later != anchors[drop[0] + 1:]
    lists = A.drop_match([[m[:2] for m in a[4]] for a in anchors], drop[0], idx2)
    assert lists[drop[0] + 1:] == [[m[:2] for m in a[4]] for a in later]
    # and a fresh call on the store after the same two mutations
    assert got["store_again"]["anchors"] == ref_anchors(again, MIN_PAIRS) and got["store_again"]["has"] == [int(h) for h in again["has"]]
