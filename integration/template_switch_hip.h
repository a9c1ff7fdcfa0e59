// Host integration shim of the template switch on the resident map point store (include/defslam_hip.h: dsh_need_new_template,
// dsh_template_switch), over MapPointStoreHIP of local_map_hip.h and KeyFrameStoreHIP of mappoint_upkeep_hip.h:
//
//   NeedNewTemplateHIP(store, mpCurrentKeyFrame)
//       drop-in for the counting of DefLocalMapping::needNewTemplate (Modules/Mapping/DefLocalMapping.cc:355-404): returns newPoints, which
//       the caller compares with pointsToTemplate_, or -1 when the library fails.
//   UpdateTemplateHIP(store, kfstore, referenceKF_, new_point, facet_of, created)
//       drop-in for the body of DefLocalMapping::updateTemplate (:145-147) once the caller has built the context's template from
//       dsh_surface_vertices and dsh_template_build: clearTemplate, CreateNewMapPoints and the embedding of createTemplate run on the
//       device.  The host write-backs, as the reference does them:
//         new points        new_point(x3w) makes the object (new DefMapPoint(x3w, referenceKF_, mpMap)); it is registered under the id the
//                           store gave it, gets AddObservation(referenceKF_, i) and referenceKF_->addMapPoint(pMP, i) (:337-338), the
//                           descriptor, normal and distances (:340-341; min distance = max / mvScaleFactors[levels - 1] in float) and is
//                           appended to `created` (the caller's mpMap->addMapPoint and mlpRecentAddedMapPoints, :342-343)
//         every good point  SetWorldPos with its position after the switch; SetFacet(facet_of(n0, n1, n2)) -- null without a facet --
//                           and SetCoordinates with the barycentrics (TriangularMesh.cc:186-190)
//       Returns false when the library fails (dsh_last_error of the store's context has the text).
//       A keyframe whose Surface is resident in the store (surface_store_hip.h) has no surface points on the host: surface_pts = NULL.
// Not done here: DefMapPoint::Repose's UpdateNormalAndDepth of the embedded points (UpdateMapPointsHIP of mappoint_upkeep_hip.h with
// DSH_MP_NORMAL_DEPTH, as before), DefKeyFrame::assignTemplate, the textures, lastincorporasion.
//
// Templates over the reference's classes; the type-specific accessors are SwitchAccess<KeyFrameT, MapPointT>: cv::Mat in DefSLAM
// (imGray.rows / cols, GetPoseInverse(), surface->get3DSurfacePoint, and writers of MapPoint's protected members), plain members in
// the stand-ins of standin_localmap_types.h.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "local_map_hip.h"
#include "mappoint_upkeep_hip.h"

namespace defslam_hip {

template <class KeyFrameT, class MapPointT>
struct SwitchAccess {
  static int rows(KeyFrameT* kf) { return kf->rows; }
  static int cols(KeyFrameT* kf) { return kf->cols; }
  static void pose_inverse(KeyFrameT* kf, float* T16) { std::memcpy(T16, kf->Twc, 16 * sizeof(float)); }
  static void surface_point(KeyFrameT* kf, int i, float* x3c) { std::memcpy(x3c, &kf->surface_points[3 * (size_t)i], 3 * sizeof(float)); }
  static void set_descriptor(MapPointT* p, const uint8_t* d) { std::memcpy(p->desc, d, 32); }
  static void set_normal_and_depth(MapPointT* p, KeyFrameT* ref, const float* n, float max_d, float min_d) {
    std::memcpy(p->normal, n, 3 * sizeof(float));
    p->mfMaxDistance = max_d;
    p->mfMinDistance = min_d;
    p->mpRefKF = ref;
  }
};

// mvKeysUn as the mask reads it
template <class KeyFrameT>
inline void switch_keypoints(KeyFrameT* kf, int rows, int cols, std::vector<float>& kp, dsh_kf_keypoints& k) {
  const size_t N = kf->mvKeysUn.size();
  kp.resize(2 * N);
  for (size_t i = 0; i < N; i++) { kp[2 * i] = kf->mvKeysUn[i].pt.x; kp[2 * i + 1] = kf->mvKeysUn[i].pt.y; }
  k.rows = rows; k.cols = cols; k.N = (int32_t)N; k.kp = kp.data();
}

template <class KeyFrameT, class MapPointT>
int NeedNewTemplateHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, KeyFrameT* mpCurrentKeyFrame) {
  typedef SwitchAccess<KeyFrameT, MapPointT> A;
  std::vector<float> kp;
  dsh_kf_keypoints k;
  switch_keypoints(mpCurrentKeyFrame, A::rows(mpCurrentKeyFrame), A::cols(mpCurrentKeyFrame), kp, k);
  int32_t newPoints = 0;
  if (dsh_need_new_template(store.handle(), store.slot(mpCurrentKeyFrame), &k, &newPoints, nullptr) != DSH_OK) return -1;
  return newPoints;
}

template <class KeyFrameT, class MapPointT, class NewPoint, class FacetOf>
bool UpdateTemplateHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, KeyFrameStoreHIP<KeyFrameT, MapPointT>& kfstore, KeyFrameT* referenceKF,
                       NewPoint new_point, FacetOf facet_of, std::vector<MapPointT*>& created, dsh_template_switch_counts* counts = nullptr) {
  typedef SwitchAccess<KeyFrameT, MapPointT> A;
  int rc = DSH_OK;
  const int32_t slot = store.slot(referenceKF);
  if (slot < 0 || kfstore.Slot(referenceKF, &rc) != slot) return false;           // the two stores number the keyframes alike
  std::vector<float> kp;
  dsh_kf_keypoints k;
  switch_keypoints(referenceKF, A::rows(referenceKF), A::cols(referenceKF), kp, k);
  const int N = k.N;
  const bool resident = dsh_keyframe_surface_state(store.handle(), slot) > 0;
  std::vector<float> surf(3 * (size_t)N);
  for (int i = 0; !resident && i < N; i++) A::surface_point(referenceKF, i, &surf[3 * (size_t)i]);
  float Twc[16];
  A::pose_inverse(referenceKF, Twc);
  dsh_template_switch_input in;
  in.kfdb = kfstore.db(); in.slot = slot; in.kf = &k; in.surface_pts = resident ? nullptr : surf.data(); in.Twc = Twc;
  std::vector<int32_t> new_idx(N > 0 ? N : 1);
  dsh_template_switch_counts c;
  if (dsh_template_switch(store.handle(), &in, new_idx.data(), &c) != DSH_OK) return false;
  if (counts) *counts = c;

  // read back every point once: position, facet; for the new ones also descriptor, normal, max distance
  const int P = c.n_points;
  std::vector<int32_t> ids(P > 0 ? P : 1), nodes(3 * (size_t)(P > 0 ? P : 1));
  for (int p = 0; p < P; p++) ids[p] = p;
  std::vector<float> xyz(3 * ids.size()), nrm(3 * ids.size()), maxd(ids.size());
  std::vector<uint8_t> desc(32 * ids.size());
  std::vector<double> bary(3 * ids.size());
  if (dsh_point_store_get_points(store.handle(), P, ids.data(), xyz.data(), nrm.data(), maxd.data(), desc.data(), nullptr) != DSH_OK) return false;
  if (dsh_point_store_get_embedding(store.handle(), P, ids.data(), nodes.data(), bary.data()) != DSH_OK) return false;
  const float sf_last = referenceKF->mvScaleFactors[referenceKF->mnScaleLevels - 1];
  for (int j = 0; j < c.n_new; j++) {
    const int id = c.first_id + j, i = new_idx[j];
    MapPointT* pMP = new_point(&xyz[3 * (size_t)id]);                             // DefLocalMapping.cc:335
    if (!pMP || !store.AdoptPoint(pMP, id)) return false;
    pMP->AddObservation(referenceKF, (size_t)i);                                  // :337
    referenceKF->addMapPoint(pMP, (size_t)i);                                     // :338
    A::set_descriptor(pMP, &desc[32 * (size_t)id]);                               // :340
    A::set_normal_and_depth(pMP, referenceKF, &nrm[3 * (size_t)id], maxd[id], maxd[id] / sf_last);   // :341
    created.push_back(pMP);
  }
  for (int p = 0; p < P; p++) {
    MapPointT* pMP = store.point(p);
    if (pMP->isBad()) continue;                                                   // not in the map: clearTemplate and the embedding pass it by
    pMP->SetWorldPos(&xyz[3 * (size_t)p]);
    const int32_t* n = &nodes[3 * (size_t)p];
    pMP->SetFacet(n[0] >= 0 ? facet_of(n[0], n[1], n[2]) : nullptr);
    if (n[0] >= 0) pMP->SetCoordinates(bary[3 * (size_t)p], bary[3 * (size_t)p + 1], bary[3 * (size_t)p + 2]);
  }
  return true;
}

}  // namespace defslam_hip
