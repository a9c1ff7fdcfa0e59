"""TEST INFRASTRUCTURE ONLY: sequential restatement of the end of a tracked frame (the checker of dsh_trackstate_* and
dsh_track_close_frame) on top of tests/local_map_ref.py (the map, the local lists) and tests/track_search_ref.py (isInFrustum).

Plain Python, statement by statement after the reference:
  Tracking::SearchLocalPoints, IncreaseVisible ........ Thirdparty/ORBSLAM_2/src/Tracking.cc:1408-1425, :1456
  Tracking::UpdateLocalMap, SetReferenceMapPoints ...... Tracking.cc:1472-1480 (:1475 BEFORE the list is rebuilt)
  DefPoseOptimization's write-back ..................... Modules/Tracking/DefOptimizer.cc:568-576
  DefMapPoint::RecalculatePosition / setBadFlag ......... Modules/Common/DefMapPoint.cc:129-147 / :76-94
  MapPoint::AddObservation / EraseObservation (nObs) .... Thirdparty/ORBSLAM_2/src/MapPoint.cc:88-121 / :123-147
  DefTracking::TrackLocalMap, the counting loops ........ Modules/Tracking/DefTracking.cc:253-319
  DefTracking::MonocularInitialization .................. DefTracking.cc:641,645
  DefMap::clearTemplate ................................. Modules/Common/DefMap.cc:75-81
  LocalMapping::MapPointCulling ......................... Thirdparty/ORBSLAM_2/src/LocalMapping.cc:173-199
Nothing in defslam_amd/ imports this module.
"""
from __future__ import annotations

import numpy as np

import local_map_ref as LM
import track_search_ref as R

f32 = np.float32
COUNT_NAMES = ("matches_inliers", "matches_outliers", "to_match_local", "observed", "inliers", "outliers", "local_map_points", "n_moved")


class TrackRefMap(LM.RefMap):
    """RefMap whose points also carry the facet, and which keeps Map::mvpReferenceMapPoints (mnVisible, mnFound and nObs are the model's)."""

    def __init__(self):
        super().__init__()
        self.nodes, self.bary = [], []           # per point None or (n0, n1, n2) ascending / (b1, b2, b3) float64
        self.reference_points = []               # Map::GetReferenceMapPoints()
        self.held_count = {}                     # how many key points of the frame of the last update hold a point that was not bad then

    # ---- mutations ----
    def add_point(self, *a, **k):
        p = super().add_point(*a, **k)           # MapPoint.cc:38,58: mnVisible(1), mnFound(1), nObs(0)
        self.nodes.append(None)
        self.bary.append(None)
        return p

    def set_bad(self, p):
        """DefMapPoint::setBadFlag as the store sees it: the flag; nObs stays (DefMapPoint.cc:84 clears mObservations, not nObs)."""
        self.points[p].bad = True

    def set_embedding(self, p, nodes, bary=None):
        if nodes is None or nodes[0] < 0:
            self.nodes[p], self.bary[p] = None, None
        else:
            self.nodes[p], self.bary[p] = tuple(int(n) for n in nodes), tuple(float(b) for b in bary)

    def clear_embedding(self):
        for p in range(len(self.points)):
            self.nodes[p], self.bary[p] = None, None

    def set_counters(self, p, visible, found):
        self.points[p].visible, self.points[p].found = int(visible), int(found)

    def seed_local_points(self, ids):
        self.local_points = [int(p) for p in ids]                     # DefTracking.cc:641
        self.reference_points = list(self.local_points)               # :645

    # ---- the frame ----
    def update_local_map(self, frame_points):
        self.reference_points = list(self.local_points)               # Tracking.cc:1475: the list as it was, before it is rebuilt
        self.held_count = {}
        for p in frame_points:
            p = int(p)
            if p >= 0 and not self.points[p].bad:
                self.held_count[p] = self.held_count.get(p, 0) + 1
        return super().update_local_map(frame_points)

    def search_local_points(self, track_frame, th=3):
        for p, k in self.held_count.items():                          # Tracking.cc:1408-1425: IncreaseVisible per key point
            self.points[p].visible += k
        r = super().search_local_points(track_frame, th)
        for q, p in enumerate(r["local_ids"]):
            if r["in_view"][q]:
                self.points[int(p)].visible += 1                      # :1456
        return r

    def repose(self, node_xyz):
        """DefOptimizer.cc:568-576: GetAllMapPoints() holds no bad point; RecalculatePosition of every point with a facet."""
        x = np.asarray(node_xyz, np.float64).reshape(-1, 3)
        moved = 0
        for p, pt in enumerate(self.points):
            if pt.bad or self.nodes[p] is None:
                continue
            n0, n1, n2 = self.nodes[p]
            b = [np.float64(v) for v in self.bary[p]]
            pt.xyz = ((b[0] * x[n0] + b[1] * x[n1]) + b[2] * x[n2]).astype(np.float32)     # DefMapPoint.cc:141-146
            moved += 1
        return moved

    def in_frustum(self, fr: R.RefFrame, p):
        pt = self.points[p]
        return R.is_in_frustum(fr, pt.xyz, pt.normal, pt.max_distance) is not None

    def frustum_count(self, fr: R.RefFrame, points):
        """DefTracking.cc:284-298 over `points`; also why the others were left out."""
        n, left_out = 0, dict(bad=0, no_facet=0, out_of_frustum=0)
        for p in points:
            if self.points[p].bad:                                    # :290
                left_out["bad"] += 1
            elif self.nodes[p] is None:                               # :292
                left_out["no_facet"] += 1
            elif not self.in_frustum(fr, p):                          # :293
                left_out["out_of_frustum"] += 1
            else:
                n += 1
        return n, left_out

    def close_frame(self, track_frame, frame_points, outlier, node_xyz=None, only_tracking=False):
        """The rest of DefTracking::TrackLocalMap after the optimisation; returns the counts as a dict (COUNT_NAMES)."""
        c = dict.fromkeys(COUNT_NAMES, 0)
        if node_xyz is not None:
            c["n_moved"] = self.repose(node_xyz)
        fp = [int(p) for p in frame_points]
        for i, p in enumerate(fp):                                    # :257-283
            if p < 0:
                continue
            if not outlier[i]:
                self.points[p].found += 1                             # IncreaseFound
                if not only_tracking:
                    if self.points[p].n_obs > 0:                      # Observations()
                        c["matches_inliers"] += 1
                        if self.nodes[p] is not None:
                            c["to_match_local"] += 1
                else:
                    c["matches_inliers"] += 1
            else:
                c["matches_outliers"] += 1
        fr = R.ref_frame(track_frame)
        c["local_map_points"], self.left_out = self.frustum_count(fr, self.reference_points)     # :284-298
        for i, p in enumerate(fp):                                    # :300-319
            if p < 0 or self.points[p].bad:
                continue
            c["observed"] += 1
            if not outlier[i]:
                c["inliers"] += 1
            else:
                c["outliers"] += 1
        return c

    def cull(self, ids, first_kf, current_kf):
        """LocalMapping::MapPointCulling: 1 was bad, 2 set bad (found ratio), 3 old enough, 0 stays."""
        action = np.zeros(len(ids), np.uint8)
        for i, p in enumerate(ids):
            p = int(p)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = f32(self.points[p].found) / f32(self.points[p].visible)   # MapPoint::GetFoundRatio, MapPoint.cc:254
            if self.points[p].bad:                                    # :184
                action[i] = 1
            elif ratio < f32(0.40):                                   # :188
                self.set_bad(p)
                action[i] = 2
            elif int(current_kf) - int(first_kf[i]) >= 3:             # :194
                action[i] = 3
        return action

    def track_state(self):
        """(visible, found, n_obs, xyz) of every point, as MapPointStore.get_state() returns them."""
        P = len(self.points)
        return (np.array([pt.visible for pt in self.points], np.int32), np.array([pt.found for pt in self.points], np.int32),
                np.array([pt.n_obs for pt in self.points], np.int32), np.array([pt.xyz for pt in self.points], np.float32).reshape(P, 3))

    def embedding_arrays(self):
        """(nodes, bary) of every point, as MapPointStore.get_embedding() returns them."""
        P = len(self.points)
        nodes, bary = np.full((P, 3), -1, np.int32), np.zeros((P, 3), np.float64)
        for p in range(P):
            if self.nodes[p] is not None:
                nodes[p], bary[p] = self.nodes[p], self.bary[p]
        return nodes, bary


def scene_to_ref(sc, embed=True, cls=TrackRefMap):
    """A synth.make_track_close_scene dict as a TrackRefMap (or as cls, a class over it)."""
    rm = cls()
    for p in range(sc["xyz"].shape[0]):
        rm.add_point(sc["xyz"][p], sc["normal"][p], sc["max_distance"][p], sc["desc"][p], sc["bad"][p])
    for k in range(sc["tables"].shape[0]):
        rm.add_keyframe(sc["tables"][k], sc["parents"][k], sc["kf_bad"][k])
    for p, k in zip(sc["obs_point"].tolist(), sc["obs_kf"].tolist()):
        assert rm.add_observation(p, k)
    for p in range(sc["xyz"].shape[0]):
        rm.set_counters(p, sc["visible"][p], sc["found"][p])
        if embed:
            rm.set_embedding(p, sc["nodes"][p], sc["bary"][p])
    return rm


def previous_frame_points(sc):
    """What the frame before the scene's frame held: points from a third of the map earlier (ids follow the camera path), so that it
    voted for other keyframes and its local list is another one."""
    fp = sc["frame_points"]
    return np.where(fp >= 0, np.maximum(fp - sc["xyz"].shape[0] // 3, 0), -1).astype(np.int32)


def run_generated_frame(rm: TrackRefMap, sc, N=None, only_tracking=False):
    """The frame of a generated scene on the restatement, as the GPU tests run it on the store: the previous frame's update (its list
    becomes the reference list), the points that turn bad in between, then update -> search -> close.  Returns the counts."""
    rm.update_local_map(previous_frame_points(sc))
    for p in sc["late_bad"]:
        rm.set_bad(int(p))
    rm.update_local_map(sc["frame_points"])
    rm.search_local_points(sc["frame"])
    N = sc["final_points"].shape[0] if N is None else N
    return rm.close_frame(sc["frame_after"], sc["final_points"][:N], sc["outlier"][:N], sc["node_xyz"], only_tracking)


def cull_list(sc):
    """mlpRecentAddedMapPoints of a generated scene: every third point."""
    ids = np.arange(0, sc["xyz"].shape[0], 3, dtype=np.int32)
    return ids, sc["first_kf"][ids]


# ---- the hand-built map: four nodes, two facets, six points, two keyframes ---------------------------------------------------------

HAND_NODES = np.array([[-0.125, -0.125, 1.0], [0.125, -0.125, 1.0], [-0.125, 0.125, 1.0], [0.125, 0.125, 1.0]], np.float64)
HAND_NODES_AFTER = HAND_NODES + np.array([0.0, 0.0, 0.0078125])        # every node 2^-7 further away: the reposed positions are exact
FACET_A, FACET_B = (0, 1, 2), (1, 2, 3)


def hand_map(erased=True) -> TrackRefMap:
    """p0 facet A, faces the camera          held twice, inlier at both key points
    p1 facet B, normal (1, 0, 0)           held, outlier; looks away: not in the frustum
    p2 no facet                            held, inlier
    p3 facet A                             held, inlier; becomes bad after the search: nObs stays 2
    p4 facet B, in the table of keyframe 1 only: nObs == 0; held, inlier
    p5 facet B                             not held: a query of the search, in view; observed twice, one observation erased
    Keyframe 0 holds p0..p3, keyframe 1 (child of 0) holds p3, p4, p5.  erased=False leaves the erase of (p5, keyframe 0) to the caller."""
    rm = TrackRefMap()
    rm.add_point(xyz=(-0.0625, -0.0625, 1.0), normal=(0, 0, 1), max_distance=2.0)
    rm.add_point(xyz=(0.0625, 0.0, 1.0), normal=(1, 0, 0), max_distance=2.0)
    rm.add_point(xyz=(0.0, 0.0, 1.0), normal=(0, 0, 1), max_distance=2.0)
    rm.add_point(xyz=(-0.03125, -0.03125, 1.0), normal=(0, 0, 1), max_distance=2.0)
    rm.add_point(xyz=(0.0625, 0.0625, 1.0), normal=(0, 0, 1), max_distance=2.0)
    rm.add_point(xyz=(0.03125, 0.03125, 1.0), normal=(0, 0, 1), max_distance=2.0)
    rm.add_keyframe([0, 1, 2, 3], parent=-1)
    rm.add_keyframe([3, 4, 5, -1], parent=0)
    for p, k in ((0, 0), (1, 0), (2, 0), (3, 0), (3, 1), (5, 1), (5, 0)):
        assert rm.add_observation(p, k)
    if erased:
        rm.erase_observation(5, 0)
    rm.set_embedding(0, FACET_A, (0.5, 0.25, 0.25))
    rm.set_embedding(1, FACET_B, (0.5, 0.25, 0.25))
    rm.set_embedding(3, FACET_A, (0.25, 0.5, 0.25))
    rm.set_embedding(4, FACET_B, (0.25, 0.25, 0.5))
    rm.set_embedding(5, FACET_B, (0.25, 0.5, 0.25))
    return rm


HAND_FRAME_POINTS = [0, 0, 1, 2, 3, 4, -1, -1]
HAND_OUTLIER = [0, 0, 1, 0, 0, 0, 0, 0]
# after update -> search -> set_bad(3) -> close with HAND_NODES_AFTER
HAND_COUNTS = dict(matches_inliers=4, matches_outliers=1, to_match_local=3, observed=5, inliers=4, outliers=1, local_map_points=0, n_moved=4)
HAND_COUNTS_ONLY_TRACKING = dict(HAND_COUNTS, matches_inliers=5, to_match_local=0)
HAND_VISIBLE = [3, 2, 2, 2, 2, 2]
HAND_FOUND = [3, 1, 2, 2, 2, 1]
HAND_N_OBS = [1, 1, 1, 2, 0, 1]
HAND_XYZ_AFTER = np.array([[-0.0625, -0.0625, 1.0078125], [0.0625, 0.0, 1.0078125], [0.0, 0.0, 1.0], [-0.03125, -0.03125, 1.0],
                           [0.0625, 0.0625, 1.0078125], [0.0, 0.0625, 1.0078125]], np.float32)
# the second frame holds p0 only and keyframe 1 is bad by then: the new list is [0, 1, 2], the reference list is the first frame's
HAND_FIRST_LIST = [0, 1, 2, 3, 4, 5]
HAND_SECOND_LIST = [0, 1, 2]
HAND_SECOND_LOCAL_MAP_POINTS = 3        # of [0, 1, 2, 3, 4, 5]: p0, p4, p5 (p1 looks away, p2 has no facet, p3 is bad)
HAND_SECOND_WRONG_LIST_COUNT = 1        # what the current list [0, 1, 2] would give
# culling with the counters of p1 set to visible 5, found 1
HAND_FIRST_KF = [0, 0, 2, 0, 2, 0]
HAND_CURRENT_KF = 3
HAND_ACTIONS = [3, 2, 0, 1, 0, 3]


def hand_frame():
    """Identity pose, 640 x 480, fx = fy = 500; eight key points, none near the projections of the six points."""
    from test_track_search_cpu import hand_frame as hf
    return hf([[10 + 5 * i, 10] for i in range(8)], [0] * 8, state=[1, 1, 1, 1, 1, 1, 0, 0])
