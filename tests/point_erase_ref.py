"""TEST INFRASTRUCTURE ONLY: sequential restatement of what takes a point out of the map, over dict-based objects, written from the
reference's lines and not from the kernels:

  MapPoint::EraseObservation, GetObservations, Observations, setBadFlag   Thirdparty/ORBSLAM_2/src/MapPoint.cc:122-180
  DefMapPoint::setBadFlag                                                 Modules/Common/DefMapPoint.cc:76-94
  KeyFrame::EraseMapPointMatch(const size_t&)                             Thirdparty/ORBSLAM_2/src/KeyFrame.cc:248-252
  LocalMapping::MapPointCulling                                           Thirdparty/ORBSLAM_2/src/LocalMapping.cc:173-199
  the drop of a Schwarp fit                                               Modules/Mapping/SchwarpDatabase.cc:288-292

Of a point of the map (tests/store_model.py) they touch bad (mbBad), ref (mpRefKF: a slot, -1: none), n_obs (nObs), found, visible and
obs (mObservations), a map from keyframe slot to key point index that is read in slot order (slot order stands for pointer order); of a
keyframe its table (mvpMapPoints), a list of ids or -1.  Also here: the counts the store reports and the scenes the CPU and GPU tests
share.  Nothing in defslam_amd/ imports this module."""
from __future__ import annotations

import numpy as np

from store_model import MapModel

f32 = np.float32
COUNT_NAMES = ("n_found", "n_ref_moved", "n_set_bad", "n_records", "n_entries")


def zero_counts():
    return dict.fromkeys(COUNT_NAMES, 0)


class EraseRefMap(MapModel):
    """The map with the reference's functions that take a point out of it."""

    # ---- the reference's functions ----
    def erase_map_point_match(self, kf, idx):                         # KeyFrame.cc:248-252: it does not look at the entry
        self.kfs[kf].table[idx] = -1

    def set_bad_flag(self, p, c):                                     # DefMapPoint.cc:76-94
        mp = self.points[p]
        mp.bad = True                                                 # :82
        obs, n_obs = dict(mp.obs), mp.n_obs                           # :83
        for kf in obs:                                                # :84 mObservations.clear(): the model blanks the records
            self.erase_observation(p, kf)
        mp.n_obs = n_obs                                              # and nObs stays
        for kf in sorted(obs):                                        # :86-91
            self.erase_map_point_match(kf, obs[kf])
            c["n_records"] += 1
            c["n_entries"] += 1
        c["n_set_bad"] += 1

    def map_point_erase_observation(self, p, kf, c):                  # MapPoint.cc:122-148 -> the status of the store
        mp = self.points[p]
        bad = False
        if kf not in mp.obs:                                          # :127
            return 0
        self.erase_observation(p, kf)                                 # :133 nObs--, :135 erase
        c["n_found"] += 1
        c["n_records"] += 1
        if mp.ref == kf:                                              # :137
            if mp.obs:                                                # begin() == end() is undefined in the reference: mpRefKF stays
                mp.ref = min(mp.obs)                                  # :138
                c["n_ref_moved"] += 1
        if mp.n_obs <= 2:                                             # :141
            bad = True
        if bad:
            self.set_bad_flag(p, c)                                   # :147
        return 2 if bad else 1

    # ---- the three calls of the store ----
    def erase_observations(self, points, slots, erase_match=False):
        """SchwarpDatabase.cc:288-292 per pair when erase_match: the index is read before the erase, as mapPoint2's idx2 is."""
        c, status = zero_counts(), []
        for p, kf in zip(points, slots):
            p, kf = int(p), int(kf)
            idx = self.points[p].obs.get(kf)
            status.append(self.map_point_erase_observation(p, kf, c))   # :290
            if erase_match and idx is not None:
                self.erase_map_point_match(kf, idx)                   # :291
                c["n_entries"] += 1
        return np.array(status, np.uint8), c

    def set_bad(self, ids):
        c = zero_counts()
        for p in ids:
            self.set_bad_flag(int(p), c)
        return c

    def cull(self, ids, first_kf, current_kf):                        # LocalMapping.cc:173-199
        c, action = zero_counts(), np.zeros(len(ids), np.uint8)
        for i, p in enumerate(ids):
            mp = self.points[int(p)]
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = f32(mp.found) / f32(mp.visible)               # MapPoint::GetFoundRatio, MapPoint.cc:251-255
            if mp.bad:                                                # :184
                action[i] = 1
            elif ratio < f32(0.40):                                   # :188
                self.set_bad_flag(int(p), c)                          # :191
                action[i] = 2
            elif int(current_kf) - int(first_kf[i]) >= 3:             # :194
                action[i] = 3
        return action, c


def assert_counts(got, want, what=""):
    assert {n: int(getattr(got, n)) for n in COUNT_NAMES} == want, (what, got, want)


# ---- scenes --------------------------------------------------------------------------------------------------------------------------------

def small_scene():
    """3 keyframes of 8 key points, 6 points -> (map, the erase batch (points, slots)).  With three keyframes every erase that finds its
    record ends at nObs <= 2 and cascades; the move without a cascade is in long_scene.
      p0  3 observations, mpRefKF = 0: erasing (p0, 0) moves it to 1, then nObs 3 -> 2 cascades over the records the move was decided on
      p1  3 observations, mpRefKF = 2: erasing (p1, 0) leaves it; the cascade meets its record in keyframe 1, which names entry 5, and
          entry 5 holds p3: nulled all the same
      p2  1 observation (keyframe 2), mpRefKF = 2: erasing it leaves mpRefKF (nothing remains) and cascades over nothing
      p3  3 observations, mpRefKF = 1: erasing (p3, 0), whose entry 3 of keyframe 0 holds p4, not p3 -- nulled with erase_match, kept
          without
      p4  bad already, 3 records left, mpRefKF = 1: erasing (p4, 1) moves it to 0 and cascades over the other two
      p5  observes keyframes 0 and 1 only: (p5, 2) is not stored"""
    rm = EraseRefMap()
    for t in range(3):
        rm.add_keyframe([-1] * 8)
    refs = (0, 2, 2, 1, 1, 0)
    for p in range(6):
        rm.add_point(ref=refs[p], bad=p == 4)
    T = [kf.table for kf in rm.kfs]
    obs = [(0, 0, 0), (0, 1, 0), (0, 2, 0),
           (1, 0, 1), (1, 1, 5), (1, 2, 1),
           (2, 2, 2),
           (3, 0, 3), (3, 1, 3), (3, 2, 3),
           (4, 0, 4), (4, 1, 4), (4, 2, 4),
           (5, 0, 6), (5, 1, 6)]
    for p, kf, idx in obs:
        T[kf][idx] = p
    T[1][5] = 3      # the entry p1's record names holds another point
    T[0][3] = 4      # and so does the entry p3's record names
    order = [9, 2, 14, 0, 7, 5, 11, 3, 12, 1, 8, 4, 10, 6, 13]   # arrival order differs from slot order
    assert sorted(order) == list(range(len(obs)))
    for i in order:
        assert rm.add_observation(*obs[i])
    return rm, ([0, 1, 2, 3, 4, 5], [0, 0, 2, 0, 1, 2])


def long_scene(seed=3, K=40, N=128, P=700):
    """A log of a few thousand records in shuffled order over K keyframes of N key points; every point observes 1 .. 9 keyframes."""
    rng = np.random.default_rng(seed)
    rm = EraseRefMap()
    for _ in range(K):
        rm.add_keyframe([-1] * N)
    free = [list(rng.permutation(N)) for _ in range(K)]
    pairs = []
    for p in range(P):
        rm.add_point(found=int(rng.integers(1, 10)), visible=int(rng.integers(1, 12)))
        for kf in rng.permutation(K)[:int(rng.integers(1, 10))]:
            kf = int(kf)
            if free[kf]:
                i = int(free[kf].pop())
                pairs.append((p, kf, i))
                rm.kfs[kf].table[i] = p
    for i in rng.permutation(len(pairs)):
        assert rm.add_observation(*pairs[int(i)])
    for p, mp in enumerate(rm.points):
        seen = sorted(mp.obs)
        mp.ref = seen[int(rng.integers(0, len(seen)))] if seen else -1
    return rm
