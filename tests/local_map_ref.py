"""TEST INFRASTRUCTURE ONLY: sequential restatement of the tracking thread's local map (the checker of dsh_mpdb_* / dsh_local_map_*).

Plain Python with dicts and sorted containers, statement by statement after the reference:
  Tracking::UpdateLocalMap .............. Thirdparty/ORBSLAM_2/src/Tracking.cc:1472-1480
  Tracking::UpdateLocalKeyFrames ........ Tracking.cc:1510-1629
  DefTracking::UpdateLocalPoints ........ Modules/Tracking/DefTracking.cc:426-454
  Tracking::SearchLocalPoints ........... Tracking.cc:1405-1470 (the search itself: tests/track_search_ref.py)
The reference's std::map<KeyFrame*, int>, std::set<KeyFrame*> and std::set<MapPoint*> iterate in pointer order; index order stands for it
(keyframes by slot, points by id), the convention of the whole project.  Nothing in defslam_amd/ imports this module.
"""
from __future__ import annotations

import numpy as np

import track_search_ref as R
from store_model import MapModel


class RefMap(MapModel):
    """The map as the tracking thread reads it, and Tracking's own state (mvpLocalKeyFrames)."""

    def __init__(self):
        super().__init__()
        self.local_kf = []               # mvpLocalKeyFrames of the previous frame
        self.local_points = []
        self.held = set()                # points with mnLastFrameSeen == the frame of the last update

    def children(self, k):
        return [s for s, kf in enumerate(self.kfs) if kf.parent == k]        # std::set<KeyFrame*>: by slot

    # ---- Tracking::UpdateLocalMap ----
    def update_local_map(self, frame_points):
        fp = [int(p) for p in frame_points]
        frame_bad = np.zeros(len(fp), bool)
        counter = {}                                                          # map<KeyFrame*, int> keyframeCounter
        for i, p in enumerate(fp):                                            # :1514-1532
            if p < 0:
                continue
            if not self.points[p].bad:
                for k in sorted(self.points[p].obs):
                    counter[k] = counter.get(k, 0) + 1
            else:
                frame_bad[i] = True                                           # mvpMapPoints[i] = NULL
        # what SearchLocalPoints' first loop (:1408-1425) marks: held and not bad
        self.held = {p for p in fp if p >= 0 and not self.points[p].bad}
        votes, ref_kf, n_voted = [], -1, 0
        if counter:                                                           # :1534: otherwise mvpLocalKeyFrames stays
            best = 0
            local, listed = [], set()                                         # listed: mnTrackReferenceForFrame == mnId
            for k in sorted(counter):                                         # :1545-1562
                if self.kfs[k].bad:
                    continue
                if counter[k] > best:
                    best, ref_kf = counter[k], k
                local.append(k)
                votes.append(counter[k])
                listed.add(k)
            n_voted = len(local)
            for i in range(n_voted):                                          # :1566-1622, itEndKF taken before the pushes
                if len(local) > 80:
                    break
                k = local[i]
                for s in range(len(self.kfs)):                                # Map::GetAllKeyFrames (a std::set<KeyFrame*>)
                    if not self.kfs[s].bad and s not in listed:
                        local.append(s)
                        listed.add(s)
                        break
                for s in self.children(k):
                    if not self.kfs[s].bad and s not in listed:
                        local.append(s)
                        listed.add(s)
                        break
                par = self.kfs[k].parent
                if par >= 0 and par not in listed:                            # no isBad test
                    local.append(par)
                    listed.add(par)
                    break                                                     # leaves the outer for
            self.local_kf = local
        # DefTracking::UpdateLocalPoints: a std::set<MapPoint*> copied out
        pts = set()
        for k in self.local_kf:
            for p in self.kfs[k].table:
                if p >= 0 and not self.points[p].bad:
                    pts.add(p)
        self.local_points = sorted(pts)
        return dict(frame_bad=frame_bad, local_kf=np.array(self.local_kf, np.int32), votes=np.array(votes, np.int32), ref_kf=ref_kf,
                    n_voted=n_voted, local_points=np.array(self.local_points, np.int32))

    # ---- Tracking::SearchLocalPoints ----
    def queries(self):
        """The local points as the arrays of the local-map search: (ids, xyz, normal, max_distance, desc, skip)."""
        ids = self.local_points
        Q = len(ids)
        xyz = np.array([self.points[p].xyz for p in ids], np.float32).reshape(Q, 3)
        nrm = np.array([self.points[p].normal for p in ids], np.float32).reshape(Q, 3)
        md = np.array([self.points[p].max_distance for p in ids], np.float32).reshape(Q)
        desc = np.array([self.points[p].desc for p in ids], np.uint8).reshape(Q, 32)
        skip = np.array([self.points[p].bad or p in self.held for p in ids], np.uint8).reshape(Q)     # :1449-1452
        return np.array(ids, np.int32), xyz, nrm, md, desc, skip

    def search_local_points(self, track_frame, th=3):
        ids, xyz, nrm, md, desc, skip = self.queries()
        m, n, _, iv, lev, uv, vc = R.search_local(R.ref_frame(track_frame), track_frame.arrays()["state"], xyz, nrm, md, desc, skip, th)
        return dict(local_ids=ids, match=m, nmatches=n, in_view=iv, level=lev, uv=uv, view_cos=vc)


# ---- hand-built maps with known answers (CPU test: the restatement; GPU test: the device) ------------------------------------------

def _simple(n_kf, parents=None, bad_kf=(), n_points=None, tables=None):
    """n_kf keyframes; point p is observed by (and in the table of) keyframe p unless tables says otherwise."""
    rm = RefMap()
    n_points = n_kf if n_points is None else n_points
    for p in range(n_points):
        rm.add_point(xyz=(0.01 * p, 0, 1))
    for k in range(n_kf):
        t = tables[k] if tables is not None else ([k] if k < n_points else [])
        rm.add_keyframe(t, -1 if parents is None else parents[k], k in bad_kf)
        for p in t:
            if p >= 0:
                assert rm.add_observation(p, k)
    return rm


def hand_maps():
    """name -> (RefMap, frame_points, expected dict of local_kf / votes / ref_kf / local_points / frame_bad indices)."""
    cases = {}
    # the parent break: keyframes 0..5, chain parents k -> k-1; the frame holds points 3 and 4.  Voted [3, 4]; visiting 3: neighbour 0, child
    # 4 is listed already -> none, parent 2 is appended and the loop ends: 4 is never visited (its child 5 stays out).
    cases["parent_break"] = (_simple(6, parents=[-1, 0, 1, 2, 3, 4]), [3, 4],
                             dict(local_kf=[3, 4, 0, 2], votes=[1, 1], ref_kf=3, local_points=[0, 2, 3, 4], frame_bad=[]))
    # a bad parent is still appended (no isBad test on the parent): parent of 2 is 1, which is bad; neighbour 0 first
    cases["bad_parent"] = (_simple(4, parents=[-1, 0, 1, -1], bad_kf=(1,)), [2],
                           dict(local_kf=[2, 0, 1], votes=[1], ref_kf=2, local_points=[0, 1, 2], frame_bad=[]))
    # the > 80 stop: 95 voted keyframes without a tree; nothing else to add, the list is the 95 (the loop breaks at its first test)
    cases["over_80_voted"] = (_simple(95), list(range(95)),
                              dict(local_kf=list(range(95)), votes=[1] * 95, ref_kf=0, local_points=list(range(95)), frame_bad=[]))
    # the > 80 stop while expanding: 200 keyframes, 78 voted (slots 100..177), no tree: every visit appends one neighbour (0, 1, 2) until
    # the list holds 81
    cases["over_80_expanding"] = (_simple(200), list(range(100, 178)),
                                  dict(local_kf=list(range(100, 178)) + [0, 1, 2], votes=[1] * 78, ref_kf=100,
                                       local_points=[0, 1, 2] + list(range(100, 178)), frame_bad=[]))
    # a vote tie goes to the lower slot; a point held twice votes twice: frame [1, 2, 2, 3, 3] -> votes 1, 2, 2 -> pKFmax = 2
    cases["tie_and_twice"] = (_simple(4), [1, 2, 2, 3, 3],
                              dict(local_kf=[1, 2, 3, 0], votes=[1, 2, 2], ref_kf=2, local_points=[0, 1, 2, 3], frame_bad=[]))
    # all voted keyframes bad: empty list, no reference keyframe, no local points
    cases["all_voted_bad"] = (_simple(3, bad_kf=(1, 2)), [1, 2], dict(local_kf=[], votes=[], ref_kf=-1, local_points=[], frame_bad=[]))
    # an erased observation does not vote: point 1 is seen by keyframes 1 and 2, the observation in 2 is erased
    rm = _simple(3, tables=[[0], [1], [1, 2]])
    rm.erase_observation(1, 2)
    cases["erased_observation"] = (rm, [1], dict(local_kf=[1, 0], votes=[1], ref_kf=1, local_points=[0, 1], frame_bad=[]))
    # a table ahead of the observations (between CreateNewKeyFrame and ProcessNewKeyFrame): keyframe 1 lists points 0 and 2 in its table,
    # but neither observes it yet -> holding point 0 votes for keyframe 0 only (votes [1], not [1, 1]); keyframe 1 comes in as the
    # neighbour, unvoted, and its table brings point 2 into the local points although nothing observes that point
    rm = _simple(1, n_points=3, tables=[[0]])
    rm.add_keyframe([0, 2], parent=-1)
    cases["table_ahead"] = (rm, [0, -1], dict(local_kf=[0, 1], votes=[1], ref_kf=0, local_points=[0, 2], frame_bad=[]))
    # a bad point in the frame is reported and does not vote; a bad point in a table is no local point
    rm = _simple(3, tables=[[0, 2], [1], [2]])
    rm.points[2].bad = True
    cases["bad_point"] = (rm, [2, 1, -1, 2], dict(local_kf=[1, 0], votes=[1], ref_kf=1, local_points=[0, 1], frame_bad=[0, 3]))
    return cases
