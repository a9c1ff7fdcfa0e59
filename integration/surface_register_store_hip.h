// Host integration shim of the surface registration of a keyframe on the resident stores (include/defslam_hip.h:
// dsh_keyframe_snapshot_positions, dsh_keyframe_register), over MapPointStoreHIP of local_map_hip.h and KeyFrameStoreHIP of
// mappoint_upkeep_hip.h:
//
//   SnapshotKeyFrameStoreHIP(store, kf)
//       for the DefKeyFrame constructor (Modules/Common/DefKeyFrame.cc:60-74), once the keyframe is in the store: the positions its
//       points have now are kept on the device as their PosesKeyframes[kf].  Returns the number of entries taken, -1 when the library
//       fails.  The loop over the host objects can go: nothing else reads PosesKeyframes.
//   RegisterSurfacesStoreHIP(store, kfstore, refKF, u, nu, chiLimit, check_chi, result)
//       drop-in for SurfaceRegistration::registerSurfaces (Modules/Mapping/SurfaceRegistration.cc:48-153); u[nu] is the rand() stream
//       of scaleMinMedian, as for dsh_surface_register.  The clouds are selected on the device from the store and the snapshot; the
//       host write-backs, as the reference does them when it registers:
//         refKF->surface->applyScale(s22)   the scaled surface points come back from the device and replace the keyframe's (:145)
//         refKF->SetPose(mScw)              with the new pose (:150); the keyframe store's camera centre has been written by the call
//       Returns the reference's return value; *ok (may be null) is false when the library failed (dsh_last_error has the text).
//       A keyframe whose Surface is resident in the store (surface_store_hip.h, InitSurfaceStoreHIP) has no surface points on the host:
//       the call then passes surface_pts = NULL, the finishing launch scales the resident points and depth spline, and applyScale's
//       host write-back is skipped; SetPose is done as before.
//
// Templates over the reference's classes; the type-specific accessors are RegisterAccess<KeyFrameT>: cv::Mat and Surface in DefSLAM
// (GetPoseInverse(), surface->get3DSurfacePoint, a setter of the Surface's points, SetPose(cv::Mat)), plain members in the stand-ins
// of standin_localmap_types.h.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "local_map_hip.h"
#include "mappoint_upkeep_hip.h"

namespace defslam_hip {

template <class KeyFrameT>
struct RegisterAccess {
  static int key_points(KeyFrameT* kf) { return (int)kf->mvpMapPoints.size(); }
  static void pose_inverse(KeyFrameT* kf, float* T16) { std::memcpy(T16, kf->Twc, 16 * sizeof(float)); }
  static void surface_point(KeyFrameT* kf, int i, float* x3c) { std::memcpy(x3c, &kf->surface_points[3 * (size_t)i], 3 * sizeof(float)); }
  static void set_surface_point(KeyFrameT* kf, int i, const float* x3c) { std::memcpy(&kf->surface_points[3 * (size_t)i], x3c, 3 * sizeof(float)); }
  static void set_pose(KeyFrameT* kf, const float* Tcw16) { kf->SetPose(Tcw16); }
};

template <class KeyFrameT, class MapPointT>
int SnapshotKeyFrameStoreHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, KeyFrameT* kf) {
  int32_t taken = 0;
  if (dsh_keyframe_snapshot_positions(store.handle(), store.slot(kf), &taken) != DSH_OK) return -1;
  return taken;
}

template <class KeyFrameT, class MapPointT>
bool RegisterSurfacesStoreHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, KeyFrameStoreHIP<KeyFrameT, MapPointT>& kfstore, KeyFrameT* refKF,
                              const double* u, int64_t nu, double chiLimit, bool check_chi, dsh_keyframe_register_result* result = nullptr,
                              bool* ok = nullptr) {
  typedef RegisterAccess<KeyFrameT> A;
  if (ok) *ok = false;
  int rc = DSH_OK;
  const int32_t slot = store.slot(refKF);
  if (slot < 0 || kfstore.Slot(refKF, &rc) != slot) return false;                 // the two stores number the keyframes alike
  const int N = A::key_points(refKF);
  const bool resident = dsh_keyframe_surface_state(store.handle(), slot) > 0;     // the Surface lives in the store: nothing of it on the host
  std::vector<float> surf(3 * (size_t)(N > 0 ? N : 1)), scaled(surf.size());
  for (int i = 0; !resident && i < N; i++) A::surface_point(refKF, i, &surf[3 * (size_t)i]);
  float Twc[16];
  A::pose_inverse(refKF, Twc);
  dsh_keyframe_register_input in;
  in.kfdb = kfstore.db(); in.slot = slot; in.N = N; in.surface_pts = resident ? nullptr : surf.data(); in.Twc = Twc;
  in.u = u; in.nu = nu; in.chi_limit = chiLimit; in.check_chi = check_chi ? 1 : 0;
  dsh_keyframe_register_result r;
  if (dsh_keyframe_register(store.handle(), &in, nullptr, resident ? nullptr : scaled.data(), &r) != DSH_OK) return false;
  if (ok) *ok = true;
  if (result) *result = r;
  if (!r.registered) return false;
  for (int i = 0; !resident && i < N; i++) A::set_surface_point(refKF, i, &scaled[3 * (size_t)i]);   // surface->applyScale(s22), :145
  A::set_pose(refKF, r.Tcw_new);                                                  // :150
  return true;
}

}  // namespace defslam_hip
