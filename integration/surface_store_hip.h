// Host integration shim of the resident Surface of a keyframe (include/defslam_hip.h: dsh_keyframe_surface_init,
// dsh_keyframe_surface_gather, dsh_keyframe_surface_take_normals, dsh_keyframe_sfn), over MapPointStoreHIP of local_map_hip.h.  With
// RegisterSurfacesStoreHIP (surface_register_store_hip.h) and UpdateTemplateHIP (template_switch_hip.h), which keep their signatures and
// accept the resident surface points, a keyframe of the mapping thread goes through the normals, the surface, the registration and the
// template switch on the stores without a host Surface:
//
//   InitSurfaceStoreHIP(store, kf)
//       for the DefKeyFrame constructor (Modules/Common/DefKeyFrame.cc: surface = new Surface(N), mpKeypointNorm), once the keyframe is
//       in the store.
//   ObtainK1K2StoreHIP(ctx, store, diffdb, points, second_keyframe_of_tag, result)
//       drop-in for NormalEstimator::ObtainK1K2 (Modules/Mapping/NormalEstimator.cc:44-228) over the points the caller found to have a
//       new observation, not bad and with enough records (:50-64): the start values and the reference key points are gathered from
//       the resident Surfaces, dsh_normals_estimate_db solves, and the normals it left on the device are written into the Surfaces
//       in the reference's order -- per point the normal in its reference keyframe (:169), then its records' propagated normals in
//       the keyframe their tag names, at the record's second key point (:223).  A tag is whatever the fits stored with the record;
//       second_keyframe_of_tag turns it into the keyframe.  No normal visits the host.
//   ShapeFromNormalsStoreHIP(ctx, store, kf, bbs, bendingWeight, meanDepth, result)
//       drop-in for ShapeFromNormals(kf, bendingWeight).estimate() (Modules/Mapping/ShapeFromNormals.cc:38-171): returns its return
//       value; the surface points and the depth spline stay in the store.
//
// Templates over the reference's classes; the type-specific accessor is SurfaceAccess<KeyFrameT>: mpKeypointNorm[i].pt in DefSLAM
// and in the stand-ins of the CI driver.
#pragma once
#include <cstdint>
#include <vector>

#include "local_map_hip.h"

namespace defslam_hip {

template <class KeyFrameT>
struct SurfaceAccess {
  static int key_points(KeyFrameT* kf) { return (int)kf->mvpMapPoints.size(); }
  static void keypoint_norm(KeyFrameT* kf, int i, float* uv) {
    uv[0] = kf->mpKeypointNorm[i].pt.x;
    uv[1] = kf->mpKeypointNorm[i].pt.y;
  }
};

template <class KeyFrameT, class MapPointT>
bool InitSurfaceStoreHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, KeyFrameT* kf) {
  typedef SurfaceAccess<KeyFrameT> A;
  const int N = A::key_points(kf);
  std::vector<float> kpn(2 * (size_t)(N > 0 ? N : 1));
  for (int i = 0; i < N; i++) A::keypoint_norm(kf, i, &kpn[2 * (size_t)i]);
  return dsh_keyframe_surface_init(store.handle(), store.slot(kf), N, kpn.data()) == DSH_OK;
}

struct NormalsStoreResult {
  std::vector<int32_t> status;       // per point, as dsh_normals_estimate_db
  int n_solved = 0;                  // points whose normal was written in their reference keyframe
  int n_propagated = 0;              // records whose normal was written in their second keyframe
};

// points[p] has reference keyframe points[p]->GetReferenceKeyFrame() and key point GetIndexInKeyFrame(refKF) there (:70-71)
template <class KeyFrameT, class MapPointT, class KeyFrameOfTag>
bool ObtainK1K2StoreHIP(dsh_ctx* ctx, MapPointStoreHIP<KeyFrameT, MapPointT>& store, dsh_diffdb* diffdb, const std::vector<MapPointT*>& points,
                        KeyFrameOfTag second_keyframe_of_tag, NormalsStoreResult* result = nullptr) {
  const int P = (int)points.size();
  const int64_t R = dsh_diffdb_count(diffdb);
  std::vector<int32_t> ids(P > 0 ? P : 1), ref_slot(ids.size()), ref_idx(ids.size());
  for (int p = 0; p < P; p++) {
    KeyFrameT* refKF = points[p]->GetReferenceKeyFrame();
    ids[p] = store.id(points[p]);
    ref_slot[p] = store.slot(refKF);
    ref_idx[p] = (int32_t)points[p]->GetIndexInKeyFrame(refKF);
    if (ids[p] < 0 || ref_slot[p] < 0 || ref_idx[p] < 0) return false;
  }
  // x0 / has_x0 / ref_uv: the stored normal and mpKeypointNorm at the reference key point (:125-135, :162-163)
  std::vector<float> x0(2 * ids.size()), uv(2 * ids.size());
  std::vector<uint8_t> has(ids.size());
  if (dsh_keyframe_surface_gather(store.handle(), P, ref_slot.data(), ref_idx.data(), x0.data(), has.data(), uv.data()) != DSH_OK) return false;
  const size_t cap = (size_t)(R > 0 ? R : 1);
  std::vector<double> k1k2(2 * ids.size()), cov(4 * ids.size());
  std::vector<int32_t> status(ids.size()), iters(ids.size()), rec_point(cap), rec_tag(cap), rec_idx2(cap);
  std::vector<float> normal_ref(3 * ids.size());
  std::vector<uint8_t> written(cap);
  int32_t n_rec = 0;
  if (dsh_normals_estimate_db(ctx, diffdb, P, ids.data(), x0.data(), has.data(), uv.data(), k1k2.data(), cov.data(), status.data(), normal_ref.data(),
                              iters.data(), (int32_t)cap, &n_rec, rec_point.data(), rec_tag.data(), rec_idx2.data(), nullptr, written.data()) != DSH_OK)
    return false;
  // the writes in the reference's order: per point :169, then its records :223 (the records come back in point order)
  std::vector<int32_t> sel, slot, idx;
  NormalsStoreResult res;
  int32_t r = 0;
  for (int p = 0; p < P; p++) {
    if (status[p] == 0) {
      sel.push_back(p); slot.push_back(ref_slot[p]); idx.push_back(ref_idx[p]);
      res.n_solved++;
    }
    for (; r < n_rec && rec_point[r] == p; r++) {
      if (!written[r]) continue;
      const int32_t s2 = store.slot(second_keyframe_of_tag(rec_tag[r]));
      if (s2 < 0) return false;
      sel.push_back(-1 - r); slot.push_back(s2); idx.push_back(rec_idx2[r]);
      res.n_propagated++;
    }
  }
  dsh_surface_take_input in;
  in.ddb = diffdb; in.n = (int32_t)sel.size(); in.sel = sel.data(); in.slot = slot.data(); in.idx = idx.data();
  if (dsh_keyframe_surface_take_normals(store.handle(), &in, nullptr) != DSH_OK) return false;
  res.status.assign(status.begin(), status.begin() + P);
  if (result) *result = res;
  return true;
}

template <class KeyFrameT, class MapPointT>
bool ShapeFromNormalsStoreHIP(dsh_ctx* ctx, MapPointStoreHIP<KeyFrameT, MapPointT>& store, KeyFrameT* kf, const dsh_bbs& bbs, double bendingWeight,
                              double meanDepth, dsh_keyframe_sfn_result* result = nullptr, bool* ok = nullptr) {
  dsh_keyframe_sfn_input in;
  in.ctx = ctx; in.slot = store.slot(kf); in.bbs = &bbs; in.bending_weight = bendingWeight; in.mean_depth = meanDepth;
  dsh_keyframe_sfn_result r;
  const bool done = dsh_keyframe_sfn(store.handle(), &in, nullptr, nullptr, nullptr, &r) == DSH_OK;
  if (ok) *ok = done;
  if (!done) return false;
  if (result) *result = r;
  return r.ok != 0;
}

}  // namespace defslam_hip
