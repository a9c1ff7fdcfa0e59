// Host integration shim of the map point upkeep on the resident stores (include/defslam_hip.h: dsh_keyframe_process_new,
// dsh_point_store_upkeep):
//
//   ProcessNewKeyFrameStoreHIP(store, kfstore, pKF, recent)
//       drop-in for the map point loop of LocalMapping::ProcessNewKeyFrame (Thirdparty/ORBSLAM_2/src/LocalMapping.cc:142-165, via
//       DefLocalMapping.cc:160-164) for a keyframe that is in both stores: one call decides IsInKeyFrame per entry, appends the
//       observation records and runs UpdateNormalAndDepth and ComputeDistinctiveDescriptors on the device; then the reference's
//       mutations are written back on the host objects: AddObservation(pKF, i) for every added point, its descriptor, normal and both
//       distances from dsh_point_store_get_points of the added points (min = max / mvScaleFactors[levels-1] of the point's reference
//       keyframe, in float, as UpdateTemplateHIP does), and the other good points go to `recent` (mlpRecentAddedMapPoints).
//   ReposeUpkeepStoreHIP(store, kfstore)
//       DefMapPoint::Repose's UpdateNormalAndDepth (Modules/Common/DefMapPoint.cc:122-126, from TriangularMesh.cc:192) after a template
//       switch: every point of the store that is not bad and has a facet, on the device, then normal and distances written back.
// Both return false when the library refuses (dsh_last_error of the stores' context says why); nothing is written to an object then.
// The two stores number the keyframes alike (local_map_hip.h, mappoint_upkeep_hip.h).  A point without a reference keyframe keeps its
// normal and distances, as in the store.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "local_map_hip.h"
#include "mappoint_upkeep_hip.h"

namespace defslam_hip {

template <class KeyFrameT, class MapPointT>
struct UpkeepAccess {
  static void set_descriptor(MapPointT* p, const uint8_t* d) { std::memcpy(p->desc, d, 32); }
  static void set_normal_and_depth(MapPointT* p, const float* n, float max_d, float min_d) {
    std::memcpy(p->normal, n, 3 * sizeof(float));
    p->mfMaxDistance = max_d;
    p->mfMinDistance = min_d;
  }
};

// normal and distances (and the descriptor) of the points ids[n] from the store onto their objects
template <class KeyFrameT, class MapPointT>
bool upkeep_write_back(MapPointStoreHIP<KeyFrameT, MapPointT>& store, const std::vector<int32_t>& ids, bool with_descriptor) {
  typedef UpkeepAccess<KeyFrameT, MapPointT> A;
  const int n = (int)ids.size();
  if (n == 0) return true;
  std::vector<float> nrm(3 * (size_t)n), maxd(n);
  std::vector<uint8_t> desc(32 * (size_t)n);
  if (dsh_point_store_get_points(store.handle(), n, ids.data(), nullptr, nrm.data(), maxd.data(), with_descriptor ? desc.data() : nullptr, nullptr) != DSH_OK)
    return false;
  for (int j = 0; j < n; j++) {
    MapPointT* pMP = store.point(ids[j]);
    if (with_descriptor) A::set_descriptor(pMP, &desc[32 * (size_t)j]);
    KeyFrameT* ref = pMP->GetReferenceKeyFrame();
    if (!ref || pMP->Observations() == 0) continue;                    // UpdateNormalAndDepth left them alone
    A::set_normal_and_depth(pMP, &nrm[3 * (size_t)j], maxd[j], maxd[j] / ref->mvScaleFactors[ref->mnScaleLevels - 1]);
  }
  return true;
}

template <class KeyFrameT, class MapPointT>
bool ProcessNewKeyFrameStoreHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, KeyFrameStoreHIP<KeyFrameT, MapPointT>& kfstore, KeyFrameT* pKF,
                                std::vector<MapPointT*>* recent = nullptr, dsh_keyframe_process_counts* counts = nullptr) {
  int rc = DSH_OK;
  const int32_t slot = store.slot(pKF);
  if (slot < 0 || kfstore.Slot(pKF, &rc) != slot) return false;        // the two stores number the keyframes alike
  const std::vector<MapPointT*> vpMapPointMatches = pKF->GetMapPointMatches();
  const size_t N = vpMapPointMatches.size();
  std::vector<uint8_t> action(N > 0 ? N : 1);
  std::vector<int32_t> added(N > 0 ? N : 1);
  dsh_keyframe_process_input in;
  in.kfdb = kfstore.db(); in.slot = slot;
  dsh_keyframe_process_counts c;
  if (dsh_keyframe_process_new(store.handle(), &in, action.data(), added.data(), &c) != DSH_OK) return false;
  if (counts) *counts = c;
  for (size_t i = 0; i < N; i++) {
    MapPointT* pMP = vpMapPointMatches[i];
    if (action[i] == 2) pMP->AddObservation(pKF, i);                   // LocalMapping.cc:151
    else if (action[i] == 3 && recent) recent->push_back(pMP);         // :155-158
  }
  added.resize((size_t)c.n_added);
  return upkeep_write_back(store, added, true);                        // :152-153
}

template <class KeyFrameT, class MapPointT>
bool ReposeUpkeepStoreHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, KeyFrameStoreHIP<KeyFrameT, MapPointT>& kfstore,
                          dsh_point_upkeep_counts* counts = nullptr) {
  dsh_point_upkeep_input in;
  in.kfdb = kfstore.db(); in.what = DSH_MP_NORMAL_DEPTH; in.select = DSH_UPKEEP_EMBEDDED; in.n = 0; in.ids = nullptr;
  dsh_point_upkeep_counts c;
  if (dsh_point_store_upkeep(store.handle(), &in, nullptr, &c) != DSH_OK) return false;
  if (counts) *counts = c;
  std::vector<int32_t> ids;
  for (int id = 0; id < store.point_count(); id++) {
    MapPointT* pMP = store.point(id);
    if (!pMP->isBad() && pMP->getFacet()) ids.push_back(id);
  }
  return (int)ids.size() == c.n_selected && upkeep_write_back(store, ids, false);
}

}  // namespace defslam_hip
