"""TEST INFRASTRUCTURE ONLY: sequential restatement of the creation of a keyframe on the resident stores and of its covisibility
connections (the checker of dsh_track_keyframe_candidate, dsh_keyframe_create and dsh_keyframe_update_connections) over
tests/store_model.MapModel, through tests/surface_store_ref.SurfaceModel, whose snapshot and Surface a new keyframe starts with.

Plain Python, statement by statement after the reference:
  DefTracking::CleanMatches ....................... Modules/Tracking/DefTracking.cc:667-679 (what CreateNewKeyFrame then copies, :175-178)
  DefTracking::CreateNewKeyFrame .................. Modules/Tracking/DefTracking.cc:696-707
  KeyFrame::KeyFrame(Frame&, ..) .................. Thirdparty/ORBSLAM_2/src/KeyFrame.cc:37-75
  DefKeyFrame::DefKeyFrame ........................ Modules/Common/DefKeyFrame.cc:42-77
  KeyFrame::UpdateConnections ..................... Thirdparty/ORBSLAM_2/src/KeyFrame.cc:326-419
Index order stands for pointer order: keyframes by slot.  Nothing in defslam_amd/ imports this module.
"""
from __future__ import annotations

import numpy as np

from surface_register_ref import centre_of
from surface_store_ref import SurfaceModel


class CreateModel(SurfaceModel):
    def __init__(self):
        super().__init__()
        self.first_connection = []   # per keyframe: KeyFrame::mbFirstConnection
        self.candidate = None        # mvpMapPoints of the current frame after CleanMatches, as ids or -1

    def clear(self):
        self.__init__()

    def add_keyframe(self, *a, **k):
        self.first_connection.append(True)   # KeyFrame.cc:37-75: mbFirstConnection(true)
        return super().add_keyframe(*a, **k)

    # ---- the end of a tracked frame: what stays for CreateNewKeyFrame ----
    def end_frame_candidate(self, frame_points):
        """CleanMatches: an entry whose point has nObs < 1 is emptied; outliers stay (they leave after the keyframe decision)."""
        self.candidate = [-1 if p >= 0 and self.points[p].n_obs < 1 else int(p) for p in (int(q) for q in frame_points)]
        return list(self.candidate)

    # ---- DefTracking::CreateNewKeyFrame ----
    def create(self, desc, octave, scale_factors, Tcw, points=None, kpn=None):
        table = list(self.candidate) if points is None else [int(p) for p in points]
        assert len(table) == np.asarray(desc).reshape(-1, 32).shape[0]
        Ow = centre_of(Tcw)                                                    # KeyFrame::SetPose in the constructor
        slot = self.add_keyframe(table, parent=-1, bad=False, Ow=Ow, desc=desc, octave=octave, scale_factors=scale_factors)
        n_snapshot = self.snapshot_positions(slot)                             # DefKeyFrame.cc:60-74
        if kpn is not None:
            self.surface_init(slot, kpn)                                       # new Surface(N), mpKeypointNorm
        return dict(slot=slot, n_held=sum(p >= 0 for p in table), n_snapshot=n_snapshot, Ow=Ow)

    # ---- KeyFrame::UpdateConnections ----
    def update_connections(self, slot, th=100):
        me = self.kfs[slot]
        counter = {}                                                           # map<KeyFrame*, int> KFcounter
        for p in me.table:                                                     # :335-357
            if p < 0:
                continue
            if self.points[p].bad:
                continue
            for k in sorted(self.points[p].obs):                               # GetObservations(): no isBad of the keyframe
                if k == slot:
                    continue
                counter[k] = counter.get(k, 0) + 1
        out = dict(counted_kf=[], counted_w=[], ordered_kf=[], ordered_w=[], parent=me.parent, parent_set=False, max_weight=0, max_kf=-1)
        if not counter:                                                        # :361
            return out
        nmax, kmax = 0, -1
        pairs = []                                                             # vector<pair<int, KeyFrame*>> vPairs
        for k in sorted(counter):                                              # :373-387, a std::map: by pointer
            if counter[k] > nmax:
                nmax, kmax = counter[k], k
            if counter[k] >= th:
                pairs.append((counter[k], k))
        if not pairs:                                                          # :389-393
            pairs.append((nmax, kmax))
        pairs.sort()                                                           # :395: on (weight, pointer)
        lkf, lw = [], []
        for w, k in pairs:                                                     # :396-402: push_front
            lkf.insert(0, k)
            lw.insert(0, w)
        out.update(counted_kf=sorted(counter), counted_w=[counter[k] for k in sorted(counter)], ordered_kf=lkf, ordered_w=lw, max_weight=nmax, max_kf=kmax)
        if self.first_connection[slot] and slot != 0:                          # :412-417: mbFirstConnection && mnId != 0
            me.parent = lkf[0]
            self.first_connection[slot] = False
            out["parent_set"] = True
        out["parent"] = me.parent
        return out


def connections_of(r):
    """A localmap.KeyframeConnections in the shape update_connections returns."""
    return dict(counted_kf=r.counted_kf.tolist(), counted_w=r.counted_w.tolist(), ordered_kf=r.ordered_kf.tolist(), ordered_w=r.ordered_w.tolist(),
                parent=r.parent, parent_set=r.parent_set, max_weight=r.max_weight, max_kf=r.max_kf)


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------

def topology(n_kf, n_points, tables=None, bad_points=(), bad_kf=()):
    """n_kf keyframes and n_points points without appearance; tables: {slot: table}, the others hold nothing."""
    m = CreateModel()
    for p in range(n_points):
        m.add_point(bad=p in bad_points)
    for s in range(n_kf):
        m.add_keyframe((tables or {}).get(s, []), bad=s in bad_kf)
    return m


def hand_cases():
    """name -> (model, slot, th, the calls to make before: none).  Every branch of UpdateConnections; the expectations are in
    tests/test_keyframe_create_cpu.py, from brute force."""
    cases = {}

    def case(name, n_kf, n_points, table, obs, slot, th, erase=(), **kw):
        m = topology(n_kf, n_points, {slot: table}, **kw)
        for p, k in obs:
            assert m.add_observation(p, k)
        for p, k in erase:
            assert m.erase_observation(p, k)
        cases[name] = (m, slot, th)
        return m

    # a point held twice counts twice; a bad point does not count; an erased record does not count; the own slot is skipped;
    # keyframe 1 is bad and still counts
    case("branches", 5, 6, [0, 0, 1, 2, -1, 3], [(0, 0), (0, 1), (1, 1), (2, 2), (3, 2), (3, 4), (0, 4), (3, 0)], 4, 2, erase=[(3, 0)], bad_points=(2,), bad_kf=(1,))
    case("empty", 3, 3, [0, 1, -1], [(0, 2), (2, 0)], 2, 1)                                   # only its own observation, and a point it does not hold
    case("no_table", 3, 2, [], [(0, 0)], 2, 1)
    case("alone", 1, 3, [0, 1, -1], [(0, 0)], 0, 1)                                           # the store holds the keyframe itself and nothing else
    case("th_met", 4, 4, [0, 1, 2, 3], [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1)], 3, 3)        # w = 3, 2 at th = 3: one connected
    case("th_missed", 4, 4, [0, 1, 2, 3], [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1)], 3, 4)     # nobody reaches 4: the fallback, one maximum
    case("fallback_two_maxima", 5, 4, [0, 1, 2, 3], [(0, 3), (1, 3), (0, 1), (1, 1), (2, 0)], 4, 100)   # slots 1 and 3 tie at 2: the lowest wins
    case("equal_connected", 5, 4, [0, 1, 2, 3], [(0, 3), (1, 3), (0, 1), (1, 1), (2, 0)], 4, 2)         # both connected: the highest first
    case("slot0", 3, 3, [0, 1, 2], [(0, 1), (1, 1), (2, 2)], 0, 1)                            # mnId == 0: never a parent
    return cases


def random_connections(seed, K, N, P, max_obs, p_bad=0.05, p_blank=0.1, p_hold=0.8, equal=False):
    """K old keyframes (tables of one key point: only the log matters), P points with 1 .. max_obs observations each, appended in shuffled
    order with a share blanked, and one new keyframe (slot K) of N key points that holds some of them, some twice.  equal: every point
    observes every old keyframe, so all weights are equal."""
    rng = np.random.default_rng(seed)
    m = CreateModel()
    for p in range(P):
        m.add_point(bad=rng.random() < p_bad)
    for s in range(K):
        m.add_keyframe([-1], bad=rng.random() < 0.2)
    pairs = []
    for p in range(P):
        n = K if equal else int(rng.integers(1, min(max_obs, K) + 1))
        pairs += [(p, int(s)) for s in rng.permutation(K)[:n]]
    for i in rng.permutation(len(pairs)):
        p, s = pairs[int(i)]
        assert m.add_observation(p, s)
        if not equal and rng.random() < p_blank:
            m.erase_observation(p, s)
    table = [int(rng.integers(0, P)) if rng.random() < p_hold else -1 for _ in range(N)] if P else [-1] * N
    slot = m.add_keyframe(table)
    if N and table[0] >= 0:
        assert m.add_observation(table[0], slot)                               # the own slot among the observations
    return m, slot


def create_scene(N, seed=0, K_old=2, N_old=5, P=None, levels=4, cls=None):
    """K_old old keyframes with appearance and N_old key points each, P points of every kind -- bad, without a facet, without an
    observation -- and the frame of N key points that becomes the new keyframe: frame_points (ids or -1, some twice), outlier flags (some
    on held points) and what the keyframe brings: descriptor rows, octaves, pyramid, Tcw, kpn.
    -> (model, dict)"""
    rng = np.random.default_rng(seed)
    P = max(N, 6) + 6 if P is None else P
    m = (cls or CreateModel)()
    sf = (1.2 ** np.arange(levels)).astype(np.float32)
    for p in range(P):
        m.add_point(rng.normal(0, 1, 3).astype(np.float32) + np.float32([0, 0, 5]), rng.normal(0, 1, 3).astype(np.float32), np.float32(rng.uniform(1, 9)),
                    rng.integers(0, 256, 32, dtype=np.uint8), bad=rng.random() < 0.1)
        if rng.random() < 0.8:
            m.facet[p] = (0, 1, 2)
    tables = [[int(p) for p in rng.permutation(P)[:N_old]] for _ in range(K_old)]
    for s in range(K_old):
        m.add_keyframe(tables[s], Ow=rng.normal(0, 1, 3).astype(np.float32), desc=rng.integers(0, 256, (N_old, 32), dtype=np.uint8),
                       octave=rng.integers(0, levels, N_old), scale_factors=sf, bad=False)
    observed = [p for p in range(P) if rng.random() < 0.75]                    # the others have nObs == 0: CleanMatches empties them
    for p in observed:
        s = int(rng.integers(0, K_old))
        if p in tables[s]:
            assert m.add_observation(p, s, tables[s].index(p))
        else:
            j = int(rng.integers(0, N_old))
            assert m.add_observation(p, s, j)
        m.points[p].ref = s
    fp = np.array([int(rng.integers(0, P)) if rng.random() < 0.6 else -1 for _ in range(N)], np.int32)
    if N >= 3 and fp[0] >= 0:
        fp[2] = fp[0]                                                          # a point held twice
    R = np.linalg.qr(rng.normal(0, 1, (3, 3)))[0]
    Tcw = np.eye(4, dtype=np.float32)
    Tcw[:3, :3], Tcw[:3, 3] = R.astype(np.float32), rng.normal(0, 2, 3).astype(np.float32)
    return m, dict(frame_points=fp, outlier=(rng.random(N) < 0.25).astype(np.uint8), desc=rng.integers(0, 256, (N, 32), dtype=np.uint8),
                   octave=rng.integers(0, levels, N).astype(np.int32), scale_factors=sf, Tcw=Tcw, kpn=rng.normal(0, 0.3, (N, 2)).astype(np.float32))
