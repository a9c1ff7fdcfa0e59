// Host integration shim of the end of a tracked frame on the resident map point store (include/defslam_hip.h: dsh_trackstate_*,
// dsh_track_close_frame), over MapPointStoreHIP of local_map_hip.h:
//
//   CloseTrackedFrameHIP(store, CurrentFrame, nodes, mbOnlyTracking, counts)
//       drop-in for what DefTracking::TrackLocalMap does after SearchLocalPoints (Modules/Tracking/DefTracking.cc:241-328) once the
//       optimiser has returned the node positions and the pose: the position write-back of DefPoseOptimization
//       (Modules/Tracking/DefOptimizer.cc:568-576) and the three counting loops run on the device, from the store's own points.  `nodes`
//       are the template's nodes in index order (the positions after updateNodes), or empty when there is no template and nothing
//       moves.  Write-backs on the host objects, as the reference does them: IncreaseFound of the inliers' points (:263) and the moved
//       mWorldPos of every point that has a facet and is not bad.  counts receives mnMatchesInliers and the Matches.txt row; the
//       caller decides as :331-338 does.  Returns false when the library fails.
//   MapPointCullingHIP(store, mlpRecentAddedMapPoints, nCurrentKFid)
//       drop-in for LocalMapping::MapPointCulling (Thirdparty/ORBSLAM_2/src/LocalMapping.cc:173-199): the found ratio is read from the
//       store's counters; points below 0.40 get setBadFlag() on the host object (the store has set its own flag) and leave the list, as
//       do the bad and the old ones.  Returns the number of points set bad, -1 when the library fails.
// The store's counters follow the reference's only if the frame went through UpdateLocalMapHIP and SearchLocalPointsStoreHIP.
#pragma once
#include <cstdint>
#include <cstring>
#include <list>
#include <vector>

#include "local_map_hip.h"

namespace defslam_hip {

template <class FrameT, class KeyFrameT, class MapPointT, class NodeT>
bool CloseTrackedFrameHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, FrameT& CurrentFrame, const std::vector<NodeT*>& nodes, bool mbOnlyTracking,
                          dsh_track_close_counts& counts) {
  typedef TrackAccess<FrameT, MapPointT> A;
  const int N = CurrentFrame.N;
  std::vector<int32_t> fp(N);
  std::vector<uint8_t> outlier(N);
  for (int i = 0; i < N; i++) {
    fp[i] = CurrentFrame.mvpMapPoints[i] ? store.id(CurrentFrame.mvpMapPoints[i]) : -1;
    outlier[i] = CurrentFrame.mvbOutlier[i] ? 1 : 0;
  }
  std::vector<double> xyz(3 * nodes.size());
  for (size_t n = 0; n < nodes.size(); n++) {
    xyz[3 * n] = nodes[n]->x; xyz[3 * n + 1] = nodes[n]->y; xyz[3 * n + 2] = nodes[n]->z;
  }
  float T[16];
  dsh_track_frame f;
  std::memset(&f, 0, sizeof(f));
  A::pose(CurrentFrame, T);
  f.Tcw = T;
  A::center(CurrentFrame, f.Ow);
  f.K[0] = CurrentFrame.fx; f.K[1] = CurrentFrame.fy; f.K[2] = CurrentFrame.cx; f.K[3] = CurrentFrame.cy;
  f.bounds[0] = CurrentFrame.mnMinX; f.bounds[1] = CurrentFrame.mnMaxX; f.bounds[2] = CurrentFrame.mnMinY; f.bounds[3] = CurrentFrame.mnMaxY;
  if (dsh_track_close_frame(store.handle(), &f, N, fp.data(), outlier.data(), (int)nodes.size(), nodes.empty() ? nullptr : xyz.data(),
                            mbOnlyTracking ? 1 : 0, &counts) != DSH_OK)
    return false;
  for (int i = 0; i < N; i++)
    if (CurrentFrame.mvpMapPoints[i] && !CurrentFrame.mvbOutlier[i]) CurrentFrame.mvpMapPoints[i]->IncreaseFound();   // DefTracking.cc:263
  if (counts.n_moved > 0) {                                                                                           // DefOptimizer.cc:571-576
    std::vector<int32_t> ids;
    for (int p = 0; p < store.point_count(); p++)
      if (!store.point(p)->isBad() && store.point(p)->getFacet()) ids.push_back(p);
    std::vector<float> pos(3 * ids.size());
    if (dsh_trackstate_get(store.handle(), (int)ids.size(), ids.data(), nullptr, nullptr, nullptr, pos.data()) != DSH_OK) return false;
    for (size_t i = 0; i < ids.size(); i++) A::set_world_pos(store.point(ids[i]), &pos[3 * i]);
  }
  return true;
}

template <class KeyFrameT, class MapPointT>
int MapPointCullingHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, std::list<MapPointT*>& mlpRecentAddedMapPoints, unsigned long nCurrentKFid) {
  std::vector<int32_t> ids, first;
  for (MapPointT* p : mlpRecentAddedMapPoints) {
    ids.push_back(store.id(p));
    first.push_back((int32_t)p->mnFirstKFid);
  }
  std::vector<uint8_t> action(ids.size() ? ids.size() : 1);
  if (dsh_trackstate_cull(store.handle(), (int)ids.size(), ids.data(), first.data(), (int32_t)nCurrentKFid, action.data()) != DSH_OK) return -1;
  int n_bad = 0;
  size_t i = 0;
  for (auto lit = mlpRecentAddedMapPoints.begin(); lit != mlpRecentAddedMapPoints.end(); i++) {
    if (action[i] == 2) {                                                         // LocalMapping.cc:188-193
      (*lit)->setBadFlag();
      n_bad++;
    }
    if (action[i] != 0) lit = mlpRecentAddedMapPoints.erase(lit);                 // :186, :192, :195
    else ++lit;                                                                   // :197
  }
  return n_bad;
}

}  // namespace defslam_hip
