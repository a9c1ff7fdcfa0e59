"""Sequential restatement of what the mapping thread reads of the map when a keyframe enters the Schwarp chain, over plain Python
containers, written from the reference's lines and not from the kernels:

  SchwarpDatabase::add              Modules/Mapping/SchwarpDatabase.cc:61-80 (the count per reference keyframe), :83-106 (vMatchedIndices)
  DefORBmatcher::searchBySchwarp    Modules/Matching/DefORBmatcher.cc:200-211 (the queries)
  SchwarpDatabase::calculateSchwarps  :288-298 (a dropped match erases (point, KF2); only the anchor's own points are stored)

Of the map (tests/store_model.py) those lines touch, per point, isBad(), GetReferenceKeyFrame() and mObservations (keyframe -> key point
index), and per keyframe mvpMapPoints.  Keyframes are slots, points ids, "null" is -1.  Where the reference iterates an
unordered_map<KeyFrame*, int> (its order is unspecified) the anchors are taken by ascending slot.  Also here: the generated maps the CPU
and GPU tests share."""
import numpy as np

from store_model import MapModel


class AnchorRefMap(MapModel):
    """The map with what the mapping thread reads of it for a new keyframe."""

    # ---- SchwarpDatabase::add up to the first fit ----
    def keyframe_anchors(self, slot, min_pairs=20):
        matches = self.kfs[slot].table                                # vpMapPointMatches (:62-63)
        count = {}                                                    # countKFMatches
        n_no_ref = 0
        for i in range(len(matches)):                                 # :68-80
            p = matches[i]
            if p == -1:
                continue
            if self.points[p].bad:
                continue
            refkf = self.points[p].ref
            if refkf < 0:                                             # no keyframe to count for: reported, not counted
                n_no_ref += 1
                continue
            if refkf not in count:
                count[refkf] = 0
            count[refkf] += 1
        out = dict(anchor_slot=[], anchor_count=[], anchor_pairs=[], pair_ptr=[0], pair_idx1=[], pair_idx2=[], pair_point=[], pair_own=[],
                   query_ptr=[0], query_idx1=[], query_point=[], has=[p != -1 for p in matches], n_no_ref=n_no_ref)
        for refkf in sorted(count):                                   # :83, by ascending slot
            matched = []                                              # vMatchedIndices
            for i in range(len(matches)):                             # :89-104
                p = matches[i]
                if p == -1:
                    continue
                if self.points[p].bad:
                    continue
                obs = self.points[p].obs
                if slot in obs and refkf in obs:                      # IsInKeyFrame of both
                    matched.append((obs[refkf], obs[slot], p, self.points[p].ref == refkf))
            out["anchor_slot"].append(refkf)
            out["anchor_count"].append(count[refkf])
            out["anchor_pairs"].append(len(matched))
            if len(matched) >= min_pairs:                             # :105-106
                for idx1, idx2, p, own in matched:
                    out["pair_idx1"].append(idx1)
                    out["pair_idx2"].append(idx2)
                    out["pair_point"].append(p)
                    out["pair_own"].append(own)                       # :296-298
                table = self.kfs[refkf].table
                for j in range(len(table)):                           # DefORBmatcher.cc:201-212
                    q = table[j]
                    if q == -1:
                        continue
                    if self.points[q].bad:
                        continue
                    if slot in self.points[q].obs:
                        continue
                    out["query_idx1"].append(j)
                    out["query_point"].append(q)
            out["pair_ptr"].append(len(out["pair_idx1"]))
            out["query_ptr"].append(len(out["query_idx1"]))
        return out


def drop_match(lists, a_from, idx2):
    """The one sequential effect between the anchors of a keyframe (:288-292): the fit of an anchor dropped the match at key point idx2
    of the new keyframe and erased (point, KF2), so the anchors behind a_from lose their pair with that idx2.  lists: per anchor a list
    of (idx1, idx2).  Returns the lists after the drop."""
    return [[m for m in l if not (a > a_from and m[1] == idx2)] for a, l in enumerate(lists)]


# ---- generated maps ----------------------------------------------------------------------------------------------------------------------

def make_map(seed, N, K, per_kf, extra_obs=2):
    """K - 1 earlier keyframes and the new keyframe K - 1 with N key points.  Every earlier keyframe creates per_kf points (it is their
    reference keyframe; a few get none) and observes some points of the others; the new keyframe holds most points once and a few
    twice, observes most of what it holds, creates a few points of its own (a == slot), and then some points become bad and some
    records are erased."""
    rng = np.random.default_rng(seed)
    rm = AnchorRefMap()
    new = K - 1
    sizes = [int(rng.integers(max(per_kf + 8, N // 2), max(per_kf + 8, N) + 1)) for _ in range(K - 1)] + [N]
    free = []
    for n in sizes:
        rm.add_keyframe([-1] * n)
        free.append(list(rng.permutation(n)))
    for k in range(K - 1):
        for _ in range(per_kf):
            p = rm.add_point(ref=-1 if rng.random() < 0.05 else k)
            i = int(free[k].pop())
            rm.kfs[k].table[i] = p
            assert rm.add_observation(p, k, i)
    P0 = len(rm.points)
    for p in range(P0):                                               # seen again by other earlier keyframes: shared, not owned
        for k in rng.permutation(K - 1)[:extra_obs]:
            k = int(k)
            if k in rm.points[p].obs or not free[k] or rng.random() < 0.4:
                continue
            i = int(free[k].pop())
            rm.kfs[k].table[i] = p
            assert rm.add_observation(p, k, i)
    held = [int(p) for p in rng.permutation(P0)[:min(P0, (3 * N) // 5)]]
    for n, p in enumerate(held):
        i = int(free[new].pop())
        rm.kfs[new].table[i] = p
        if n % 9 != 4:                                                # the others do not observe the keyframe yet
            assert rm.add_observation(p, new, i)
        if n % 11 == 3 and free[new]:                                 # held by a second entry; the observation keeps the first index
            rm.kfs[new].table[int(free[new].pop())] = p
    for _ in range(min(5, len(free[new]))):                           # the new keyframe's own points
        p = rm.add_point(ref=new)
        i = int(free[new].pop())
        rm.kfs[new].table[i] = p
        assert rm.add_observation(p, new, i)
    for p in rng.permutation(len(rm.points))[:max(2, len(rm.points) // 15)]:
        rm.points[int(p)].bad = True
    both = [p for p in held if new in rm.points[p].obs and len(rm.points[p].obs) > 1 and not rm.points[p].bad]
    for n, p in enumerate(both[:8]):
        if n % 2 == 0:
            rm.erase_observation(p, new)                              # a blanked record of (p, slot)
        else:
            rm.erase_observation(p, next(k for k in rm.points[p].obs if k != new))   # and of (p, a)
    return rm


def threshold_map(m):
    """Anchor 0 shares exactly m - 1 points with the new keyframe 2, anchor 1 exactly m; one point of anchor 0 is seen by anchor 1 too."""
    rm = AnchorRefMap()
    for n in (m + 3, m + 3, 2 * m + 3):
        rm.add_keyframe([-1] * n)
    j = 0
    for k, n in ((0, m - 1), (1, m - 1)):
        for i in range(n):
            p = rm.add_point(ref=k)
            rm.kfs[k].table[i] = p
            assert rm.add_observation(p, k, i)
            rm.kfs[2].table[j] = p
            assert rm.add_observation(p, 2, j)
            j += 1
    p = 0                                                             # owned by keyframe 0, the m-th pair of keyframe 1
    rm.kfs[1].table[m] = p
    assert rm.add_observation(p, 1, m)
    for k in (0, 1):                                                  # a query each: a point the new keyframe does not see
        q = rm.add_point(ref=k)
        rm.kfs[k].table[m + 1] = q
        assert rm.add_observation(q, k, m + 1)
    return rm


# (name, how to build it, min_pairs): the shapes of the GPU tests
SCENES = {
    "n70_k5": (lambda: make_map(1, 70, 5, 14, extra_obs=3), 20),                  # one wavefront boundary in the table
    "n300_k6": (lambda: make_map(2, 300, 6, 150), 20),                # one workgroup boundary in the ordered compaction
    "a70": (lambda: make_map(3, 400, 76, 6), 3),                      # at least 70 anchors: the anchor compaction crosses a ballot word
}


def assert_equal(g, r):
    """Every output of MapPointStore.keyframe_anchors equals the restatement's."""
    for n in ("anchor_slot", "anchor_count", "anchor_pairs", "pair_ptr", "pair_idx1", "pair_idx2", "pair_point", "pair_own", "query_ptr",
              "query_idx1", "query_point", "has"):
        got, want = np.asarray(getattr(g, n)).astype(np.int64), np.asarray(r[n]).astype(np.int64)
        assert got.shape == want.shape and (got == want).all(), (n, got, want)
    assert g.n_no_ref == r["n_no_ref"]
