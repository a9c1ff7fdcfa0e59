"""TEST INFRASTRUCTURE ONLY: the restatement of dsh_keyframe_process_new and dsh_point_store_upkeep on the model of the two resident stores.

On what the stores hold (tests/store_model.py) it drives tests/mappoint_ref.py one point at a time with the point's live observations by
ASCENDING SLOT, whatever order the records arrived in.  Nothing in defslam_amd/ imports this module.
"""
from __future__ import annotations

import numpy as np

import mappoint_ref as R
from store_model import MapModel

DESCRIPTOR, NORMAL_DEPTH, BOTH = 1, 2, 3
NO_OBS, NO_GOOD_DESC, NO_REF, SKIPPED_BAD = 1, 2, 4, 8
EMPTY, BAD_POINT, ADDED, RECENT = 0, 1, 2, 3


class StoreModel(MapModel):
    """The model of the two stores with the upkeep of a point and the insertion of a new keyframe."""

    # ---- the upkeep ----
    def upkeep_point(self, p, what=BOTH):
        """-> status; writes desc / normal / max_distance / min_distance of point p where the reference would."""
        pt = self.points[p]
        if pt.bad:
            return SKIPPED_BAD
        obs = self.observations(p)
        if not obs:
            return NO_OBS
        status = 0
        if all(self.kfs[s].bad for s, _ in obs):
            status |= NO_GOOD_DESC
        ref = pt.ref
        no_ref = ref < 0 or (ref not in dict(obs) and len(self.kfs[ref].table) == 0)
        if no_ref:
            status |= NO_REF
        if what & DESCRIPTOR:
            _, row = R.compute_distinctive_descriptors(self.kfs, obs)
            if row is not None:
                pt.desc = row
        if (what & NORMAL_DEPTH) and not no_ref:
            pt.normal, pt.max_distance, pt.min_distance = R.update_normal_and_depth(self.kfs, pt.xyz, obs, ref)
        return status

    def upkeep(self, ids, what=BOTH):
        return [self.upkeep_point(int(p), what) for p in ids]

    def embedded_ids(self, has_facet):
        return [p for p, pt in enumerate(self.points) if not pt.bad and has_facet[p]]

    def process_new_keyframe(self, slot):
        """LocalMapping.cc:142-165 -> (action per entry, added points, statuses of the added points)."""
        action, added, status = [], [], []
        for i, p in enumerate(self.kfs[slot].table):
            if p < 0:
                action.append(EMPTY)
            elif self.points[p].bad:
                action.append(BAD_POINT)
            elif self.live(p, slot):
                action.append(RECENT)
            else:
                assert self.add_observation(p, slot, i)
                status.append(self.upkeep_point(p))
                added.append(p)
                action.append(ADDED)
        return action, added, status


def random_model(seed, K=6, N=6, P=20, levels=4, p_obs=0.5, p_bad_kf=0.2, p_bad_point=0.1, p_no_ref=0.0, new_table=None, shuffle=True, cls=None):
    """K old keyframes with N key points each and P points that observe some of them, then a new keyframe whose table holds some of the
    points (one of them twice, one observing it already).  Records are appended in shuffled order, so log order and slot order differ."""
    rng = np.random.default_rng(seed)
    m = (cls or StoreModel)()                        # cls: a class that combines StoreModel with other restatements
    sf = (1.2 ** np.arange(levels)).astype(np.float32)
    for p in range(P):
        m.add_point(rng.normal(0, 1, 3).astype(np.float32) + np.float32([0, 0, 5]), rng.normal(0, 1, 3).astype(np.float32), np.float32(rng.uniform(1, 9)),
                    rng.integers(0, 256, 32, dtype=np.uint8), bad=rng.random() < p_bad_point)
    pairs = []
    for s in range(K):
        table = [-1] * N
        for j, p in enumerate(rng.permutation(P)[:N]):
            if rng.random() < p_obs:
                table[j] = int(p)
                pairs.append((int(p), s, j))
        m.add_keyframe(Ow=rng.normal(0, 1, 3).astype(np.float32), desc=rng.integers(0, 256, (N, 32), dtype=np.uint8), octave=rng.integers(0, levels, N),
                       scale_factors=sf, table=table, bad=rng.random() < p_bad_kf)
    perm = rng.permutation(len(pairs))
    if shuffle:
        pairs = [pairs[i] for i in perm]
    for p, s, j in pairs:
        assert m.add_observation(p, s, j)
    for p in range(P):
        seen = [s for s, _ in m.observations(p)]
        m.points[p].ref = -1 if (not seen and rng.random() < 0.5) or rng.random() < p_no_ref else int(rng.choice(seen)) if seen and rng.random() < 0.8 else int(rng.integers(0, K))
    if new_table is None:
        held = [int(p) for p in rng.permutation(P)[:max(N - 2, 1)]]
        new_table = (held + [held[0], -1])[:N] if N >= 3 else held[:N]
    slot = m.add_keyframe(Ow=rng.normal(0, 1, 3).astype(np.float32), desc=rng.integers(0, 256, (len(new_table), 32), dtype=np.uint8),
                          octave=rng.integers(0, levels, len(new_table)), scale_factors=sf, table=new_table)
    if len(new_table) >= 3 and new_table[1] >= 0 and new_table[1] != new_table[0]:
        assert m.add_observation(new_table[1], slot, 1)   # this point observes the new keyframe already
    return m, slot


# ---- the scene of the GPU tests: every width class, the large path, a log that strides ---------------------------------------------------

PRE_COUNTS = (0, 1, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128)   # observations before the add: 1, 2, 8, 9 ... 129 after it
BAD_SLOTS = (3, 10, 77, 100)
K_OLD, N_KP = 129, 6


def big_scene(seed=7, fillers=200, filler_obs=118, singles=0, ties=()):
    """129 old keyframes with 6 key points each, four of them bad, and three new keyframes A, B, C (slots 129, 130, 131):
      A, B   hold the twelve points of PRE_COUNTS, whose references are observed, not observed (key point 0 lends the octave) or -1
      C      holds a point twice, a point that observes C already, a bad point, an empty entry and a point whose old keyframes are all bad
    `fillers` further points with `filler_obs` observations each make the log long; `singles` points with one observation each make the
    selection long; per entry c of `ties` (even) a point with c observations in good keyframes whose rows alternate between two
    descriptors by slot rank, so every median is 0 and the lowest slot, which holds the first descriptor, must win.  The old records are appended by DESCENDING slot,
    the points interleaved; some records are blanked, one pair is erased and added again with another index.
    -> (model, dict of the named points and slots)"""
    rng = np.random.default_rng(seed)
    m = StoreModel()
    levels = 8
    sf = (1.2 ** np.arange(levels)).astype(np.float32)

    def point(bad=False):
        return m.add_point(rng.normal(0, 1, 3).astype(np.float32) + np.float32([0, 0, 6]), rng.normal(0, 1, 3).astype(np.float32),
                           np.float32(rng.uniform(1, 9)), rng.integers(0, 256, 32, dtype=np.uint8), bad=bad)
    pairs, names = [], {}

    def observe(p, slots):
        for s in slots:
            pairs.append((p, int(s), int(rng.integers(0, N_KP))))
    count_pts = []
    for c in PRE_COUNTS:
        p = point()
        observe(p, rng.permutation(K_OLD)[:c])
        count_pts.append(p)
    names["count_pts"] = count_pts
    for name, c, bad in (("twice", 3, False), ("already", 5, False), ("bad_point", 4, True), ("plain", 9, False), ("no_obs", 0, False)):
        names[name] = point(bad)
        observe(names[name], rng.permutation(K_OLD)[:c])
    names["all_bad"] = point()
    observe(names["all_bad"], BAD_SLOTS)
    fill = [point() for _ in range(fillers)]
    for p in fill:
        observe(p, rng.permutation(K_OLD)[:filler_obs])
    good_slots = [s_ for s_ in range(K_OLD) if s_ not in BAD_SLOTS]
    names["ties"] = []
    for t, c in enumerate(ties):
        p = point()
        slots = sorted(int(s_) for s_ in rng.permutation(good_slots)[:c])
        pairs.extend((p, s_, t) for s_ in slots)                    # key point t of each keyframe
        names["ties"].append((p, slots, rng.integers(0, 256, (2, 32), dtype=np.uint8)))
    names["singles"] = [point() for _ in range(singles)]
    for p in names["singles"]:
        observe(p, rng.permutation(K_OLD)[:1])
    # descending slot, the points interleaved
    pairs.sort(key=lambda r: (-r[1], rng.random()))
    tables = [[-1] * N_KP for _ in range(K_OLD)]
    for p, s_, j in pairs:
        if tables[s_][j] < 0:
            tables[s_][j] = p
    for s_ in range(K_OLD):
        m.add_keyframe(Ow=rng.normal(0, 1, 3).astype(np.float32), desc=rng.integers(0, 256, (N_KP, 32), dtype=np.uint8), octave=rng.integers(0, levels, N_KP),
                       scale_factors=sf, table=tables[s_], bad=s_ in BAD_SLOTS)
    for t, (p, slots, two) in enumerate(names["ties"]):
        for rank, s_ in enumerate(slots):
            m.kfs[s_].desc[t] = two[rank % 2]
    blank = set(int(i) for i in rng.permutation(len(pairs))[:60] if pairs[int(i)][0] in fill)
    # the pair erased and added again: a record of the point with 33 observations
    p33 = count_pts[PRE_COUNTS.index(32)]
    again = next(r for r in pairs if r[0] == p33)
    for i, (p, s_, j) in enumerate(pairs):
        if (p, s_, j) == again:
            assert m.add_observation(p, s_, (j + 1) % N_KP)
            m.erase_observation(p, s_)
            names["again"] = (p, s_, j)
        elif i in blank:
            assert m.add_observation(p, s_, j)
            m.erase_observation(p, s_)
        else:
            assert m.add_observation(p, s_, j)
    assert m.add_observation(*again)
    A = m.add_keyframe(Ow=rng.normal(0, 1, 3).astype(np.float32), desc=rng.integers(0, 256, (N_KP, 32), dtype=np.uint8), octave=rng.integers(0, levels, N_KP),
                       scale_factors=sf, table=count_pts[:6])
    B = m.add_keyframe(Ow=rng.normal(0, 1, 3).astype(np.float32), desc=rng.integers(0, 256, (N_KP, 32), dtype=np.uint8), octave=rng.integers(0, levels, N_KP),
                       scale_factors=sf, table=count_pts[6:])
    Ck = m.add_keyframe(Ow=rng.normal(0, 1, 3).astype(np.float32), desc=rng.integers(0, 256, (N_KP, 32), dtype=np.uint8), octave=rng.integers(0, levels, N_KP),
                        scale_factors=sf, table=[names["twice"], names["already"], names["bad_point"], -1, names["twice"], names["all_bad"]])
    assert m.add_observation(names["already"], Ck, 1)
    names.update(A=A, B=B, C=Ck)
    # reference keyframes: observed ones, the new keyframe itself (a point created from it), one that is not observed, and none
    for i, p in enumerate(count_pts):
        seen = [s_ for s_, _ in m.observations(p)]
        m.points[p].ref = (A if i < 6 else B) if not seen else seen[len(seen) // 2]
    m.points[count_pts[3]].ref = next(s_ for s_ in range(K_OLD) if s_ not in dict(m.observations(count_pts[3])))   # not observed
    m.points[count_pts[8]].ref = -1
    for name in ("twice", "already", "bad_point", "plain", "all_bad"):
        m.points[names[name]].ref = m.observations(names[name])[0][0]
    m.points[names["no_obs"]].ref = 0
    for p in fill + names["singles"] + [t[0] for t in names["ties"]]:
        m.points[p].ref = m.observations(p)[0][0]
    return m, names
