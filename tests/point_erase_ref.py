"""TEST INFRASTRUCTURE ONLY: sequential restatement of what takes a point out of the map, over dict-based objects, written from the
reference's lines and not from the kernels:

  MapPoint::EraseObservation, GetObservations, Observations, setBadFlag   Thirdparty/ORBSLAM_2/src/MapPoint.cc:122-180
  DefMapPoint::setBadFlag                                                 Modules/Common/DefMapPoint.cc:76-94
  KeyFrame::EraseMapPointMatch(const size_t&)                             Thirdparty/ORBSLAM_2/src/KeyFrame.cc:248-252
  LocalMapping::MapPointCulling                                           Thirdparty/ORBSLAM_2/src/LocalMapping.cc:173-199
  the drop of a Schwarp fit                                               Modules/Mapping/SchwarpDatabase.cc:288-292

A point is a dict with mbBad, mpRefKF (a slot, -1: none), nObs, mnFound, mnVisible and mObservations, a map from keyframe slot to key
point index that is read in slot order (slot order stands for pointer order); a keyframe is a dict whose mvpMapPoints is a list of ids or
-1.  Also here: the counts the store reports, the scenes the CPU and GPU tests share, the replay of a map into a MapPointStore and the
conversions into the maps of the other restatements.  Nothing in defslam_amd/ imports this module."""
from __future__ import annotations

import numpy as np

f32 = np.float32
COUNT_NAMES = ("n_found", "n_ref_moved", "n_set_bad", "n_records", "n_entries")


def zero_counts():
    return dict.fromkeys(COUNT_NAMES, 0)


class EraseRefMap:
    def __init__(self):
        self.points = []         # dict(mbBad, mpRefKF, nObs, mnFound, mnVisible, mObservations)
        self.kfs = []            # dict(mvpMapPoints)
        self.log = []            # every AddObservation in call order (point, keyframe, index), for the replay

    # ---- building ----
    def add_point(self, ref=-1, bad=False, found=1, visible=1):
        self.points.append(dict(mbBad=bool(bad), mpRefKF=int(ref), nObs=0, mnFound=int(found), mnVisible=int(visible), mObservations={}))
        return len(self.points) - 1

    def add_keyframe(self, table):
        self.kfs.append(dict(mvpMapPoints=[int(p) for p in table]))
        return len(self.kfs) - 1

    def add_observation(self, p, kf, idx):                            # MapPoint.cc:109-120, monocular
        mp = self.points[p]
        if kf in mp["mObservations"]:
            return False
        assert 0 <= idx < len(self.kfs[kf]["mvpMapPoints"])
        mp["mObservations"][int(kf)] = int(idx)
        mp["nObs"] += 1
        self.log.append((int(p), int(kf), int(idx)))
        return True

    # ---- the reference's functions ----
    def erase_map_point_match(self, kf, idx):                         # KeyFrame.cc:248-252: it does not look at the entry
        self.kfs[kf]["mvpMapPoints"][idx] = -1

    def set_bad_flag(self, p, c):                                     # DefMapPoint.cc:76-94
        mp = self.points[p]
        mp["mbBad"] = True                                            # :82
        obs = dict(mp["mObservations"])                               # :83
        mp["mObservations"].clear()                                   # :84; nObs stays
        for kf in sorted(obs):                                        # :86-91
            self.erase_map_point_match(kf, obs[kf])
            c["n_records"] += 1
            c["n_entries"] += 1
        c["n_set_bad"] += 1

    def erase_observation(self, p, kf, c):                            # MapPoint.cc:122-148 -> the status of the store
        mp = self.points[p]
        bad = False
        if kf not in mp["mObservations"]:                             # :127
            return 0
        mp["nObs"] -= 1                                               # :133
        del mp["mObservations"][kf]                                   # :135
        c["n_found"] += 1
        c["n_records"] += 1
        if mp["mpRefKF"] == kf:                                       # :137
            if mp["mObservations"]:                                   # begin() == end() is undefined in the reference: mpRefKF stays
                mp["mpRefKF"] = min(mp["mObservations"])              # :138
                c["n_ref_moved"] += 1
        if mp["nObs"] <= 2:                                           # :141
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
            idx = self.points[p]["mObservations"].get(kf)
            status.append(self.erase_observation(p, kf, c))           # :290
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
                ratio = f32(mp["mnFound"]) / f32(mp["mnVisible"])     # MapPoint::GetFoundRatio, MapPoint.cc:251-255
            if mp["mbBad"]:                                           # :184
                action[i] = 1
            elif ratio < f32(0.40):                                   # :188
                self.set_bad_flag(int(p), c)                          # :191
                action[i] = 2
            elif int(current_kf) - int(first_kf[i]) >= 3:             # :194
                action[i] = 3
        return action, c

    # ---- read-backs in the shape of the store's ----
    def observations(self, p):
        """MapPoint::GetObservations of p, in slot order."""
        return dict(sorted(self.points[p]["mObservations"].items()))

    def state(self):
        P = len(self.points)
        return dict(bad=np.array([mp["mbBad"] for mp in self.points], bool).reshape(P),
                    n_obs=np.array([mp["nObs"] for mp in self.points], np.int32).reshape(P),
                    ref=np.array([mp["mpRefKF"] for mp in self.points], np.int32).reshape(P),
                    obs=[self.observations(p) for p in range(P)],
                    tables=[list(kf["mvpMapPoints"]) for kf in self.kfs])


def store_state(st):
    """The same dict read back from a MapPointStore."""
    P = st.n_points
    o = st.observations()
    return dict(bad=st.get_points().bad, n_obs=st.get_state().n_obs, ref=st.get_reference_keyframes(),
                obs=[o.of(p) for p in range(P)], tables=[st.keyframe_table(s).tolist() for s in range(st.n_keyframes)])


def assert_state(st, rm, what=""):
    g, r = store_state(st), rm.state()
    for n in ("bad", "n_obs", "ref"):
        assert np.array_equal(np.asarray(g[n]).astype(np.int64), r[n].astype(np.int64)), (what, n, g[n], r[n])
    assert g["obs"] == r["obs"], (what, "obs", [(p, a, b) for p, (a, b) in enumerate(zip(g["obs"], r["obs"])) if a != b])
    assert g["tables"] == r["tables"], (what, "tables", [(s, a, b) for s, (a, b) in enumerate(zip(g["tables"], r["tables"])) if a != b])


def assert_counts(got, want, what=""):
    assert {n: int(getattr(got, n)) for n in COUNT_NAMES} == want, (what, got, want)


def fill_store(st, rm, batches=1):
    """Replay rm into an empty MapPointStore: points with their counters, keyframes with their tables, the observations in the order
    they were added, the reference keyframes.  rm must not have erased anything yet (its log is then its state)."""
    P = len(rm.points)
    z = np.zeros((P, 3), np.float32)
    st.add_points(z, z, np.ones(P, np.float32), np.zeros((P, 32), np.uint8), np.array([mp["mbBad"] for mp in rm.points], np.uint8))
    st.set_counters(np.arange(P), [mp["mnVisible"] for mp in rm.points], [mp["mnFound"] for mp in rm.points])
    for k, kf in enumerate(rm.kfs):
        assert st.add_keyframe(np.array(kf["mvpMapPoints"], np.int32)) == k
    log = np.array(rm.log, np.int32).reshape(-1, 3)
    for part in np.array_split(log, batches):
        if len(part):
            st.add_observations(part[:, 0], part[:, 1], idx=part[:, 2])
    st.set_reference_keyframes(np.arange(P), [mp["mpRefKF"] for mp in rm.points])


# ---- conversions into the maps of the other restatements ---------------------------------------------------------------------------------

def to_local_map(rm, bad_kf=()):
    """A local_map_ref.RefMap with rm's points, observations and tables (no spanning tree; bad_kf: the slots of the bad keyframes)."""
    import local_map_ref as LM
    m = LM.RefMap()
    for mp in rm.points:
        m.add_point(bad=mp["mbBad"])
    for s, kf in enumerate(rm.kfs):
        m.add_keyframe(kf["mvpMapPoints"], bad=s in bad_kf)
    for p, mp in enumerate(rm.points):
        for kf in sorted(mp["mObservations"]):
            m.add_observation(p, kf)
    return m


def to_anchor_map(rm):
    import anchor_pairs_ref as AR
    m = AR.AnchorRefMap()
    for mp in rm.points:
        m.add_point(ref=mp["mpRefKF"], bad=mp["mbBad"])
    for kf in rm.kfs:
        m.tables.append(list(kf["mvpMapPoints"]))
    for p, mp in enumerate(rm.points):
        m.obs[p] = dict(mp["mObservations"])
    return m


def from_store_model(model):
    """An EraseRefMap with the points, live observations (in log order), tables and reference keyframes of a keyframe_insert_ref.StoreModel."""
    rm = EraseRefMap()
    for p in range(len(model.xyz)):
        rm.add_point(ref=model.ref[p], bad=model.bad[p])
    for t in model.tables:
        rm.add_keyframe(t)
    for p, s, idx, live in model.log:
        if live:
            rm.add_observation(p, s, idx)
    return rm


def into_store_model(rm, model):
    """Make a keyframe_insert_ref.StoreModel hold rm's state: bad flags, reference keyframes, nObs, tables, and exactly rm's observations."""
    for p, mp in enumerate(rm.points):
        for s, idx in model.observations(p):
            if mp["mObservations"].get(s) != idx:                     # gone, or erased and added again with another index
                model.erase_observation(p, s)
        for s, idx in mp["mObservations"].items():
            if not model.live(p, s):
                model.add_observation(p, s, idx)
        assert dict(model.observations(p)) == mp["mObservations"]
        model.bad[p], model.ref[p], model.n_obs[p] = mp["mbBad"], mp["mpRefKF"], mp["nObs"]
    for s, kf in enumerate(rm.kfs):
        model.tables[s] = list(kf["mvpMapPoints"])


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
    T = [kf["mvpMapPoints"] for kf in rm.kfs]
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
        rm.add_observation(*obs[i])
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
                rm.kfs[kf]["mvpMapPoints"][i] = p
    for i in rng.permutation(len(pairs)):
        rm.add_observation(*pairs[int(i)])
    for p, mp in enumerate(rm.points):
        seen = sorted(mp["mObservations"])
        mp["mpRefKF"] = seen[int(rng.integers(0, len(seen)))] if seen else -1
    return rm
