// Stand-ins of the members of ORB_SLAM2::KeyFrame and ORB_SLAM2::MapPoint that integration/mappoint_upkeep_hip.h touches (reference
// declaration behind each), for the repository's CI: OpenCV is not in the build image.  Inside DefSLAM these are not used.
#pragma once
#include <cstdint>
#include <map>
#include <vector>

#include "standin_types.h"   // standin::KeyPoint (cv::KeyPoint: pt, octave)

namespace standin {

class MpMapPoint;

class MpKeyFrame {                             // Thirdparty/ORBSLAM_2/include/KeyFrame.h
 public:
  bool isBad() { return mbBad; }                                        // :117
  std::vector<MpMapPoint*> GetMapPointMatches() { return mvpMapPoints; }// :94
  float Ow[3] = {0, 0, 0};                                              // GetCameraCenter() :57 (cv::Mat 3x1 float)
  int N = 0;                                                            // :178
  std::vector<KeyPoint> mvKeysUn;                                       // :182
  std::vector<uint8_t> mDescriptors;                                    // :187 N rows of 32 bytes (cv::Mat CV_8U)
  int mnScaleLevels = 8;                                                // :198
  std::vector<float> mvScaleFactors;                                    // :201
  std::vector<MpMapPoint*> mvpMapPoints;                                // :226
  bool mbBad = false;                                                   // :250
};

class MpMapPoint {                             // Thirdparty/ORBSLAM_2/include/MapPoint.h
 public:
  std::map<MpKeyFrame*, size_t> GetObservations() { return mObservations; }   // :54
  void AddObservation(MpKeyFrame* pKF, size_t idx) {                     // :57, MapPoint.cc:109-120 (monocular: mvuRight < 0)
    if (mObservations.count(pKF)) return;
    mObservations[pKF] = idx;
    nObs++;
  }
  bool IsInKeyFrame(MpKeyFrame* pKF) { return mObservations.count(pKF) != 0; }  // :61
  bool isBad() { return mbBad; }                                        // :64
  MpKeyFrame* GetReferenceKeyFrame() { return mpRefKF; }                // :52
  float pos[3] = {0, 0, 0};                                             // GetWorldPos() :49 (cv::Mat 3x1 float)
  // written by ComputeDistinctiveDescriptors / UpdateNormalAndDepth (protected members of the reference, MapPoint.h:134-152)
  uint8_t mDescriptor[32] = {};
  float mNormalVector[3] = {0, 0, 0};
  float mfMinDistance = 0, mfMaxDistance = 0;
  std::map<MpKeyFrame*, size_t> mObservations;
  MpKeyFrame* mpRefKF = nullptr;
  int nObs = 0;
  bool mbBad = false;
};

}  // namespace standin
