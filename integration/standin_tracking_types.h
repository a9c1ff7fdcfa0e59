// Stand-ins of the members of ORB_SLAM2::Frame and ORB_SLAM2::MapPoint that integration/tracking_search_hip.h touches (reference
// declaration behind each), for the repository's CI: OpenCV is not in the build image.  Inside DefSLAM these are not used.
#pragma once
#include <cstdint>
#include <vector>

#include "standin_types.h"   // standin::KeyPoint (cv::KeyPoint: pt, octave)

namespace standin {

class TrackMapPoint {                          // Thirdparty/ORBSLAM_2/include/MapPoint.h
 public:
  int Observations() { return nObs; }                                   // :55
  bool isBad() { return bad; }                                          // :64
  void IncreaseVisible(int n = 1) { nVisible += n; }                    // :69
  float pos[3] = {0, 0, 0};                                             // GetWorldPos() :49 (cv::Mat 3x1 float)
  float normal[3] = {0, 0, 1};                                          // GetNormal() :51
  uint8_t desc[32] = {};                                                // GetDescriptor() :76 (1x32 CV_8U)
  float mfMaxDistance = 1.f;                                            // :152
  // tracking members written by Frame::isInFrustum (MapPoint.h:103-108)
  float mTrackProjX = 0, mTrackProjY = 0, mTrackViewCos = 0;
  int mnTrackScaleLevel = 0;
  bool mbTrackInView = false;
  unsigned long mnLastFrameSeen = 0;                                    // :110
  int nObs = 1, nVisible = 0;
  bool bad = false;
};

class TrackFrame {                             // Thirdparty/ORBSLAM_2/include/Frame.h
 public:
  float mTcw[16];                                                       // :180 cv::Mat 4x4 float
  float mOw[3];                                                         // :231 camera centre
  float fx, fy, cx, cy;                                                 // :121-124 (static in the reference)
  float mnMinX, mnMaxX, mnMinY, mnMaxY;                                 // :199-202 (static)
  int N = 0;                                                            // :140
  std::vector<KeyPoint> mvKeys, mvKeysUn;                               // :148-149
  std::vector<uint8_t> mDescriptors;                                    // :163 N rows of 32 bytes (cv::Mat CV_8U)
  std::vector<TrackMapPoint*> mvpMapPoints;                             // :166
  std::vector<bool> mvbOutlier;                                         // :172
  int mnScaleLevels = 8;                                                // :190
  float mfLogScaleFactor = 0;                                           // :192
  std::vector<float> mvScaleFactors;                                    // :193
  unsigned long mnId = 0;                                               // :184
  // what ORB_SLAM2::Optimizer::poseOptimization touches besides the above (pose_only_hip.h)
  std::vector<float> mvInvLevelSigma2;                                  // :195
  void SetPose(const float* Tcw) {                                      // :66 (Frame.cc:261-275: mTcw, then UpdatePoseMatrices)
    for (int i = 0; i < 16; i++) mTcw[i] = Tcw[i];
    for (int i = 0; i < 3; i++) mOw[i] = -(mTcw[i] * mTcw[3] + mTcw[4 + i] * mTcw[7] + mTcw[8 + i] * mTcw[11]);
  }
};

}  // namespace standin
