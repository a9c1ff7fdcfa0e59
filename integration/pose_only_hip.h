// Host integration shim of the rigid pose-only optimisation on the resident map point store (include/defslam_hip.h:
// dsh_track_pose_only), over MapPointStoreHIP of local_map_hip.h:
//
//   PoseOptimizationStoreHIP(Frame, store[, detail])
//       drop-in for ORB_SLAM2::Optimizer::poseOptimization(&Frame) (Thirdparty/ORBSLAM_2/src/Optimizer.cc:236-445) where
//       DefTracking::TrackLocalMap calls it (Modules/Tracking/DefTracking.cc:250), monocular frames only.  The frame sends its pose, its
//       undistorted key points with their octaves, mvInvLevelSigma2 and the store ids of mvpMapPoints; the positions are the store's, no
//       GetWorldPos() is read.  Writes mvbOutlier where the frame holds a point and, unless fewer than three points are held, the pose
//       through SetPose, as the reference does.  A point the store does not know is an error.  Returns the number of inliers, -1 when
//       the library fails; *detail (optional) receives the call's record with the counts per round.
// A template over the reference's classes; the stand-ins of the CI are standin::LmFrame / standin::TrackFrame.
#pragma once
#include <cstdint>
#include <vector>

#include "local_map_hip.h"

namespace defslam_hip {

template <class FrameT, class KeyFrameT, class MapPointT>
int PoseOptimizationStoreHIP(FrameT& Frame, MapPointStoreHIP<KeyFrameT, MapPointT>& store, dsh_pose_only_problem* detail = nullptr) {
  const int N = Frame.N;
  std::vector<float> kp(2 * (size_t)(N > 0 ? N : 1));
  std::vector<int32_t> oct(N > 0 ? N : 1), ids(N > 0 ? N : 1);
  std::vector<uint8_t> flags(N > 0 ? N : 1);
  for (int i = 0; i < N; i++) {
    kp[2 * i] = Frame.mvKeysUn[i].pt.x;
    kp[2 * i + 1] = Frame.mvKeysUn[i].pt.y;
    oct[i] = Frame.mvKeysUn[i].octave;
    flags[i] = Frame.mvbOutlier[i] ? 1 : 0;
    ids[i] = -1;
    if (Frame.mvpMapPoints[i]) {
      ids[i] = store.id(Frame.mvpMapPoints[i]);
      if (ids[i] < 0) return -1;
    }
  }
  dsh_pose_only_problem p = dsh_pose_only_problem();
  p.Tcw = Frame.mTcw;
  p.K[0] = Frame.fx; p.K[1] = Frame.fy; p.K[2] = Frame.cx; p.K[3] = Frame.cy;
  p.N = N;
  p.kp = kp.data();
  p.octave = oct.data();
  p.levels = (int32_t)Frame.mvInvLevelSigma2.size();
  p.inv_level_sigma2 = Frame.mvInvLevelSigma2.data();
  p.frame_points = ids.data();
  p.outlier = flags.data();
  if (dsh_track_pose_only(store.handle(), &p) != DSH_OK) return -1;
  for (int i = 0; i < N; i++)
    if (ids[i] >= 0) Frame.mvbOutlier[i] = flags[i] != 0;               // Optimizer.cc:285, :391-397
  if (p.rounds > 0) Frame.SetPose(p.Tcw_out);                           // :441-442; the early return at :358-359 leaves the pose
  if (detail) {
    *detail = p;
    detail->Tcw = nullptr; detail->kp = nullptr; detail->octave = nullptr; detail->inv_level_sigma2 = nullptr;   // the arrays were this call's
    detail->frame_points = nullptr; detail->outlier = nullptr;
  }
  return p.n_good;
}

}  // namespace defslam_hip
