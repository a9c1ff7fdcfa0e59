// Host integration shim of the erase on the resident map point store (include/defslam_hip.h: dsh_point_store_cull,
// dsh_point_store_erase_observations), over MapPointStoreHIP of local_map_hip.h:
//
//   MapPointCullingStoreHIP(store, mlpRecentAddedMapPoints, nCurrentKFid)
//       drop-in for LocalMapping::MapPointCulling (Thirdparty/ORBSLAM_2/src/LocalMapping.cc:173-199): one call decides every entry of
//       the list from the store's mnFound / mnVisible and bad flags and erases the observation records and table entries of the points
//       it sets bad; then the reference's mutations are written back on the host objects: setBadFlag() of the culled points
//       (DefMapPoint.cc:76-94, which empties the entries of the host keyframes too) and the list loses every entry but the ones that stay.
//   DropMatchesStoreHIP(store, KF2, dropped)
//       the drops of one Schwarp fit (Modules/Mapping/SchwarpDatabase.cc:288-292) in one call: for each dropped point
//       mapPoint2->EraseObservation(KF2) -- with the move of its reference keyframe and the nObs <= 2 cascade -- and
//       KF2->EraseMapPointMatch(idx2), on the device and then on the host objects.  The points of one fit are distinct.  idx2 is the
//       point's index in KF2 (the pair lists of AnchorPairsHIP take it from the same record); a point that does not observe KF2 is left
//       alone by both sides.  With DropMatchHIP of anchor_pairs_hip.h, which edits the snapshot lists, this is the whole drop.
// Both return false when the library refuses (dsh_last_error of the store's context says why); nothing is written to an object then.
// The host objects' own EraseObservation and setBadFlag do the write-back: inside DefSLAM they are the reference's.  The stand-ins of
// the repository's CI are simpler, so its driver specialises EraseAccess with the reference's bodies.
#pragma once
#include <cstdint>
#include <list>
#include <vector>

#include "local_map_hip.h"

namespace defslam_hip {

template <class KeyFrameT, class MapPointT>
struct EraseAccess {
  static void erase_observation(MapPointT* p, KeyFrameT* kf) { p->EraseObservation(kf); }   // MapPoint.cc:122-148
  static void set_bad_flag(MapPointT* p) { p->setBadFlag(); }                               // DefMapPoint.cc:76-94
};

template <class KeyFrameT, class MapPointT>
bool MapPointCullingStoreHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, std::list<MapPointT*>& mlpRecentAddedMapPoints,
                             unsigned long nCurrentKFid, dsh_point_erase_counts* counts = nullptr) {
  typedef EraseAccess<KeyFrameT, MapPointT> A;
  std::vector<int32_t> ids, first_kf;
  for (MapPointT* pMP : mlpRecentAddedMapPoints) {
    ids.push_back(store.id(pMP));
    first_kf.push_back((int32_t)pMP->mnFirstKFid);
  }
  std::vector<uint8_t> action(ids.size() > 0 ? ids.size() : 1);
  dsh_point_erase_counts c;
  if (dsh_point_store_cull(store.handle(), (int)ids.size(), ids.data(), first_kf.data(), (int32_t)nCurrentKFid, action.data(), &c) != DSH_OK) return false;
  if (counts) *counts = c;
  size_t i = 0;
  for (typename std::list<MapPointT*>::iterator lit = mlpRecentAddedMapPoints.begin(); lit != mlpRecentAddedMapPoints.end(); i++) {
    if (action[i] == 2) A::set_bad_flag(*lit);                           // :191
    if (action[i] != 0) lit = mlpRecentAddedMapPoints.erase(lit);        // :186, :192, :195
    else lit++;                                                          // :197
  }
  return true;
}

template <class KeyFrameT, class MapPointT>
bool DropMatchesStoreHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, KeyFrameT* KF2, const std::vector<MapPointT*>& dropped,
                         dsh_point_erase_counts* counts = nullptr) {
  typedef EraseAccess<KeyFrameT, MapPointT> A;
  const size_t n = dropped.size();
  std::vector<int32_t> ids(n), slots(n, store.slot(KF2));
  for (size_t i = 0; i < n; i++) ids[i] = store.id(dropped[i]);
  std::vector<uint8_t> status(n > 0 ? n : 1);
  dsh_point_erase_counts c;
  if (dsh_point_store_erase_observations(store.handle(), (int)n, ids.data(), slots.data(), 1, status.data(), &c) != DSH_OK) return false;
  if (counts) *counts = c;
  for (size_t i = 0; i < n; i++) {
    if (status[i] == 0) continue;                                        // the point does not observe KF2
    const int idx2 = dropped[i]->GetIndexInKeyFrame(KF2);
    A::erase_observation(dropped[i], KF2);                               // SchwarpDatabase.cc:290
    KF2->EraseMapPointMatch((size_t)idx2);                               // :291
  }
  return true;
}

}  // namespace defslam_hip
