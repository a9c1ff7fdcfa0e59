"""Sequential restatement of what the mapping thread reads of the map when a keyframe enters the Schwarp chain, over plain Python
containers, written from the reference's lines and not from the kernels:

  SchwarpDatabase::add              Modules/Mapping/SchwarpDatabase.cc:61-80 (the count per reference keyframe), :83-106 (vMatchedIndices)
  DefORBmatcher::searchBySchwarp    Modules/Matching/DefORBmatcher.cc:200-211 (the queries)
  SchwarpDatabase::calculateSchwarps  :288-298 (a dropped match erases (point, KF2); only the anchor's own points are stored)

A map here is what those lines touch: per point isBad(), GetReferenceKeyFrame() and mObservations (keyframe -> key point index), per
keyframe mvpMapPoints.  Keyframes are slots, points ids, "null" is -1.  Where the reference iterates an unordered_map<KeyFrame*, int>
(its order is unspecified) the anchors are taken by ascending slot.  Also here: the generated maps the CPU and GPU tests share, and the
replay of a map into a MapPointStore."""
import numpy as np


class AnchorRefMap:
    def __init__(self):
        self.bad = []          # MapPoint::isBad
        self.ref = []          # MapPoint::GetReferenceKeyFrame as a slot, -1: none
        self.obs = []          # MapPoint::mObservations: {keyframe: key point index}
        self.tables = []       # KeyFrame::mvpMapPoints: a point or -1 per key point
        self.log = []          # every AddObservation in call order (point, keyframe, index), for the replay
        self.erased = []       # every EraseObservation that found its record

    def add_point(self, ref=-1, bad=False):
        self.bad.append(bool(bad))
        self.ref.append(int(ref))
        self.obs.append({})
        return len(self.bad) - 1

    def add_keyframe(self, n):
        self.tables.append([-1] * int(n))
        return len(self.tables) - 1

    def add_observation(self, p, kf, idx):
        assert kf not in self.obs[p] and 0 <= idx < len(self.tables[kf])
        self.obs[p][kf] = int(idx)
        self.log.append((int(p), int(kf), int(idx)))

    def erase_observation(self, p, kf):
        if kf in self.obs[p]:
            del self.obs[p][kf]
            self.erased.append((int(p), int(kf)))

    # ---- SchwarpDatabase::add up to the first fit ----
    def keyframe_anchors(self, slot, min_pairs=20):
        matches = self.tables[slot]                                   # vpMapPointMatches (:62-63)
        count = {}                                                    # countKFMatches
        n_no_ref = 0
        for i in range(len(matches)):                                 # :68-80
            p = matches[i]
            if p == -1:
                continue
            if self.bad[p]:
                continue
            refkf = self.ref[p]
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
                if self.bad[p]:
                    continue
                if slot in self.obs[p] and refkf in self.obs[p]:      # IsInKeyFrame of both
                    matched.append((self.obs[p][refkf], self.obs[p][slot], p, self.ref[p] == refkf))
            out["anchor_slot"].append(refkf)
            out["anchor_count"].append(count[refkf])
            out["anchor_pairs"].append(len(matched))
            if len(matched) >= min_pairs:                             # :105-106
                for idx1, idx2, p, own in matched:
                    out["pair_idx1"].append(idx1)
                    out["pair_idx2"].append(idx2)
                    out["pair_point"].append(p)
                    out["pair_own"].append(own)                       # :296-298
                table = self.tables[refkf]
                for j in range(len(table)):                           # DefORBmatcher.cc:201-212
                    q = table[j]
                    if q == -1:
                        continue
                    if self.bad[q]:
                        continue
                    if slot in self.obs[q]:
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
        rm.add_keyframe(n)
        free.append(list(rng.permutation(n)))
    for k in range(K - 1):
        for _ in range(per_kf):
            p = rm.add_point(ref=-1 if rng.random() < 0.05 else k)
            i = int(free[k].pop())
            rm.tables[k][i] = p
            rm.add_observation(p, k, i)
    P0 = len(rm.bad)
    for p in range(P0):                                               # seen again by other earlier keyframes: shared, not owned
        for k in rng.permutation(K - 1)[:extra_obs]:
            k = int(k)
            if k in rm.obs[p] or not free[k] or rng.random() < 0.4:
                continue
            i = int(free[k].pop())
            rm.tables[k][i] = p
            rm.add_observation(p, k, i)
    held = [int(p) for p in rng.permutation(P0)[:min(P0, (3 * N) // 5)]]
    for n, p in enumerate(held):
        i = int(free[new].pop())
        rm.tables[new][i] = p
        if n % 9 != 4:                                                # the others do not observe the keyframe yet
            rm.add_observation(p, new, i)
        if n % 11 == 3 and free[new]:                                 # held by a second entry; the observation keeps the first index
            rm.tables[new][int(free[new].pop())] = p
    for _ in range(min(5, len(free[new]))):                           # the new keyframe's own points
        p = rm.add_point(ref=new)
        i = int(free[new].pop())
        rm.tables[new][i] = p
        rm.add_observation(p, new, i)
    for p in rng.permutation(len(rm.bad))[:max(2, len(rm.bad) // 15)]:
        rm.bad[int(p)] = True
    both = [p for p in held if new in rm.obs[p] and len(rm.obs[p]) > 1 and not rm.bad[p]]
    for n, p in enumerate(both[:8]):
        if n % 2 == 0:
            rm.erase_observation(p, new)                              # a blanked record of (p, slot)
        else:
            rm.erase_observation(p, next(k for k in rm.obs[p] if k != new))   # and of (p, a)
    return rm


def threshold_map(m):
    """Anchor 0 shares exactly m - 1 points with the new keyframe 2, anchor 1 exactly m; one point of anchor 0 is seen by anchor 1 too."""
    rm = AnchorRefMap()
    for n in (m + 3, m + 3, 2 * m + 3):
        rm.add_keyframe(n)
    j = 0
    for k, n in ((0, m - 1), (1, m - 1)):
        for i in range(n):
            p = rm.add_point(ref=k)
            rm.tables[k][i] = p
            rm.add_observation(p, k, i)
            rm.tables[2][j] = p
            rm.add_observation(p, 2, j)
            j += 1
    p = 0                                                             # owned by keyframe 0, the m-th pair of keyframe 1
    rm.tables[1][m] = p
    rm.add_observation(p, 1, m)
    for k in (0, 1):                                                  # a query each: a point the new keyframe does not see
        q = rm.add_point(ref=k)
        rm.tables[k][m + 1] = q
        rm.add_observation(q, k, m + 1)
    return rm


# (name, how to build it, min_pairs): the shapes of the GPU tests
SCENES = {
    "n70_k5": (lambda: make_map(1, 70, 5, 14, extra_obs=3), 20),                  # one wavefront boundary in the table
    "n300_k6": (lambda: make_map(2, 300, 6, 150), 20),                # one workgroup boundary in the ordered compaction
    "a70": (lambda: make_map(3, 400, 76, 6), 3),                      # at least 70 anchors: the anchor compaction crosses a ballot word
}


def fill_store(st, rm, batches=3):
    """Replay rm into an empty MapPointStore: points, keyframes with their tables, every observation ever added (in a few batches, with
    its index), the erasures, the reference keyframes."""
    P = len(rm.bad)
    z = np.zeros((P, 3), np.float32)
    st.add_points(z, z, np.ones(P, np.float32), np.zeros((P, 32), np.uint8), np.array(rm.bad, np.uint8))
    for k, t in enumerate(rm.tables):
        assert st.add_keyframe(np.array(t, np.int32)) == k
    log = np.array(rm.log, np.int32).reshape(-1, 3)
    for part in np.array_split(log, batches):
        if len(part):
            st.add_observations(part[:, 0], part[:, 1], idx=part[:, 2])
    if rm.erased:
        e = np.array(rm.erased, np.int32)
        st.erase_observations(e[:, 0], e[:, 1])
    st.set_reference_keyframes(np.arange(P), np.array(rm.ref, np.int32))


def assert_equal(g, r):
    """Every output of MapPointStore.keyframe_anchors equals the restatement's."""
    for n in ("anchor_slot", "anchor_count", "anchor_pairs", "pair_ptr", "pair_idx1", "pair_idx2", "pair_point", "pair_own", "query_ptr",
              "query_idx1", "query_point", "has"):
        got, want = np.asarray(getattr(g, n)).astype(np.int64), np.asarray(r[n]).astype(np.int64)
        assert got.shape == want.shape and (got == want).all(), (n, got, want)
    assert g.n_no_ref == r["n_no_ref"]
