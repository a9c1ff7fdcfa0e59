// Host integration shim of Shape-from-Template on the resident map point store (include/defslam_hip.h: dsh_track_sft):
//
//   DefPoseOptimizationStoreHIP(ctx, binding, store, pFrame, mMap, RegLap, RegInex, RegTemp, NeighboursLayers)
//       drop-in for defSLAM::Optimizer::DefPoseOptimization (Modules/Tracking/DefOptimizer.cc:251-578) where DefTracking calls it
//       (Modules/Tracking/DefTracking.cc:115, :244), like DefPoseOptimizationHIP of defslam_hip_shim.h but without its walk over the
//       map points of the frame: the frame sends its pose, its undistorted key points with their octaves, mvInvLevelSigma2, mvbOutlier
//       and the store ids of mvpMapPoints; facets and barycentrics are the store's (SetEmbedding of local_map_hip.h, or a template
//       switch on the device).  Performs the reference's mutations: mvbOutlier at the key points that entered the graph, repError,
//       SetPose, the roles and positions of the nodes, and SetWorldPos of every map point of the map that has a facet, from one
//       dsh_point_store_get_points of their ids (the points moved on the device).  The frame is closed with CloseTrackedFrameHIP (track_close_hip.h)
//       and no nodes afterwards.  A point the store does not know is an error.  Returns nInitialCorrespondences - nBad, 0 when nothing entered the
//       graph (nothing changes then) and when the library fails (dsh_last_error of the context has the text).
// `store` is MapPointStoreHIP of local_map_hip.h or anything with its handle() and id(MapPoint*).  A template over the reference's
// classes; ShimWorldPos<MapPointT> is the one type-specific accessor next to ShimPose (cv::Mat in DefSLAM).
#pragma once
#include <cstdint>
#include <mutex>
#include <set>
#include <vector>

#include "defslam_hip_shim.h"

namespace defslam_hip {

// MapPoint::SetWorldPos from three floats; specialise for the map point type (cv::Mat(3, 1, CV_32F) in DefSLAM)
template <class MapPointT>
struct ShimWorldPos {
  static void set(MapPointT* p, const float* xyz) { p->SetWorldPos(xyz); }
};

template <class FrameT, class MapT, class TemplateT, class NodeT, class DefMapPointT, class StoreT>
int DefPoseOptimizationStoreHIP(dsh_ctx* ctx, TemplateBinding<TemplateT, NodeT>& binding, StoreT& store, FrameT* pFrame, MapT* mMap,
                                double RegLap = 5000, double RegInex = 5000, double RegTemp = 0, unsigned int NeighboursLayers = 1) {
  TemplateT* tmpl = mMap->GetTemplate();                       // DefMap.h:69
  if (!tmpl || binding.sync(ctx, tmpl) != DSH_OK) return 0;
  const std::vector<NodeT*>& nodes = binding.nodes();
  const int n = (int)nodes.size();
  for (int i = 0; i < n; i++) nodes[i]->setIndex((unsigned)(i + 1));   // setMeshNodes, DefOptimizer.cc:926-952
  std::unique_lock<decltype(DefMapPointT::mGlobalMutex)> lock(DefMapPointT::mGlobalMutex);   // :287, held to the end
  const int N = pFrame->N;
  const size_t cap = N > 0 ? (size_t)N : 1;
  std::vector<float> kp(2 * cap);
  std::vector<int32_t> oct(cap), ids(cap);
  std::vector<uint8_t> flags(cap);
  for (int i = 0; i < N; i++) {
    kp[2 * i] = pFrame->mvKeysUn[i].pt.x;
    kp[2 * i + 1] = pFrame->mvKeysUn[i].pt.y;
    oct[i] = pFrame->mvKeysUn[i].octave;
    flags[i] = pFrame->mvbOutlier[i] ? 1 : 0;
    ids[i] = -1;
    if (pFrame->mvpMapPoints[i]) {
      ids[i] = store.id(pFrame->mvpMapPoints[i]);
      if (ids[i] < 0) return 0;
    }
  }
  std::vector<double> xyz(3 * (size_t)n), xyz_out(3 * (size_t)n);
  for (int i = 0; i < n; i++) nodes[i]->getXYZ(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);   // Node.h:126
  float Tcw[16], Tcw_out[16];
  ShimPose<FrameT>::get(*pFrame, Tcw);
  dsh_track_sft_frame f = dsh_track_sft_frame();
  f.Tcw = Tcw;
  f.K[0] = pFrame->fx; f.K[1] = pFrame->fy; f.K[2] = pFrame->cx; f.K[3] = pFrame->cy;
  f.N = N;
  f.kp = kp.data();
  f.octave = oct.data();
  f.levels = (int32_t)pFrame->mvInvLevelSigma2.size();
  f.inv_level_sigma2 = pFrame->mvInvLevelSigma2.data();
  f.frame_points = ids.data();
  f.outlier = flags.data();
  f.xyz = xyz.data();
  f.reg_lap = RegLap; f.reg_inex = RegInex; f.reg_temp = RegTemp;
  f.neighbour_layers = (int32_t)NeighboursLayers;
  f.max_iters = 50;                                            // optimizer.optimize(50), :513
  std::vector<int32_t> row_nodes(3 * cap);
  dsh_track_sft_table t = dsh_track_sft_table();
  t.capacity = (int32_t)cap;
  t.nodes = row_nodes.data();
  dsh_sft_result r = dsh_sft_result();
  r.Tcw = Tcw_out;
  r.xyz = xyz_out.data();
  if (dsh_track_sft(store.handle(), &f, 1, &t, &r) != DSH_OK) return 0;
  if (t.M == 0) return 0;                                      // empty graph: nothing changes, no inliers
  // ---- the reference's mutations
  for (int i = 0; i < N; i++) pFrame->mvbOutlier[i] = flags[i] != 0;   // :307, :515-537: only the key points of the graph changed
  std::set<NodeT*> ViewedNodes;                                // :331-332, :388-432
  for (int k = 0; k < 3 * t.M; k++) {
    ViewedNodes.insert(nodes[row_nodes[k]]);
    nodes[row_nodes[k]]->setViewed();
  }
  if (NeighboursLayers >= 1)
    for (NodeT* v : ViewedNodes)
      for (NodeT* nb : v->GetNeighbours()) nb->setLocal();
  for (NodeT* v : ViewedNodes) v->setLocal();
  pFrame->repError = (float)r.rep_error;                       // :559
  ShimPose<FrameT>::set(*pFrame, Tcw_out);                     // :561-565
  for (int i = 0; i < n; i++) {                                // updateNodes, :954-968
    nodes[i]->update();
    nodes[i]->resetRole();
    nodes[i]->setXYZ(xyz_out[3 * i], xyz_out[3 * i + 1], xyz_out[3 * i + 2]);
  }
  std::vector<DefMapPointT*> moved;                            // :567-575: the device moved them, the objects follow
  std::vector<int32_t> moved_ids;
  for (auto* pMP : mMap->GetAllMapPoints()) {
    DefMapPointT* d = static_cast<DefMapPointT*>(pMP);
    if (!d->getFacet() || d->isBad()) continue;
    const int id = store.id(d);
    if (id < 0) continue;
    moved.push_back(d);
    moved_ids.push_back(id);
  }
  std::vector<float> pos(3 * (moved.size() > 0 ? moved.size() : 1));
  if (dsh_point_store_get_points(store.handle(), (int)moved_ids.size(), moved_ids.data(), pos.data(), nullptr, nullptr, nullptr, nullptr) != DSH_OK) return 0;
  for (size_t i = 0; i < moved.size(); i++) ShimWorldPos<DefMapPointT>::set(moved[i], &pos[3 * i]);
  return r.inliers;
}

}  // namespace defslam_hip
