// Stand-ins of the members of ORB_SLAM2::KeyFrame, ORB_SLAM2::MapPoint (with defSLAM::DefMapPoint's) and ORB_SLAM2::Frame that
// integration/local_map_hip.h, integration/track_close_hip.h and integration/anchor_pairs_hip.h touch
// (reference declaration behind each), for the repository's CI: OpenCV is not in the build image.  Inside DefSLAM these are not used.
#pragma once
#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <map>
#include <memory>
#include <set>
#include <utility>
#include <vector>

#include "standin_types.h"   // standin::KeyPoint (cv::KeyPoint: pt, octave)

namespace standin {

class LmKeyFrame;

struct LmNode {                                // Modules/Template/Node.h
  double x = 0, y = 0, z = 0;                                           // :140
};

class LmFacet {                                // Modules/Template/Facet.h
 public:
  std::set<LmNode*> getNodes() { return Nodes; }                        // :65 (a copy, ordered by pointer)
  std::set<LmNode*> Nodes;                                              // :99
};

class LmMapPoint {                             // Thirdparty/ORBSLAM_2/include/MapPoint.h
 public:
  std::map<LmKeyFrame*, size_t> GetObservations() { return mObservations; }   // :54 (a copy, as in the reference)
  int Observations() { return (int)mObservations.size(); }              // :55
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
  unsigned long mnTrackReferenceForFrame = 0;                           // :109
  unsigned long mnLastFrameSeen = 0;                                    // :110
  std::map<LmKeyFrame*, size_t> mObservations;                          // :127
  int nVisible = 0;
  bool bad = false;
  // what the end of DefTracking::TrackLocalMap and LocalMapping::MapPointCulling touch
  void IncreaseFound(int n = 1) { mnFound += n; }                       // :70
  float GetFoundRatio() { return static_cast<float>(mnFound) / nVisible; }   // :71 (MapPoint.cc:251-255)
  void setBadFlag() { bad = true; mObservations.clear(); }              // :63; nObs stays (DefMapPoint.cc:76-94)
  int mnFound = 1;                                                      // :144
  int nObs = 0;                                                         // :96: what Observations() returns in the reference
  long int mnFirstKFid = 0;                                             // :94
  // defSLAM::DefMapPoint (Modules/Common/DefMapPoint.h)
  LmFacet* getFacet() { return facet; }                                 // :76
  void RecalculatePosition() {                                          // :86 (DefMapPoint.cc:129-147)
    const std::set<LmNode*> nodes = facet->getNodes();
    std::vector<LmNode*> v(nodes.begin(), nodes.end());
    pos[0] = b1 * v[0]->x + b2 * v[1]->x + b3 * v[2]->x;
    pos[1] = b1 * v[0]->y + b2 * v[1]->y + b3 * v[2]->y;
    pos[2] = b1 * v[0]->z + b2 * v[1]->z + b3 * v[2]->z;
  }
  LmFacet* facet = nullptr;                                             // :100
  double b1 = 0, b2 = 0, b3 = 0;                                        // :96
  // what DefLocalMapping::CreateNewMapPoints and TriangularMesh::calculateFeaturesCoordinates touch (template_switch_hip.h)
  void SetWorldPos(const float* x) { pos[0] = x[0]; pos[1] = x[1]; pos[2] = x[2]; }   // MapPoint.h:48
  void AddObservation(LmKeyFrame* kf, size_t idx) {                     // MapPoint.h:57 (MapPoint.cc:86-97, monocular)
    if (mObservations.count(kf)) return;
    mObservations[kf] = idx;
    nObs++;
  }
  void SetFacet(LmFacet* f) { facet = f; }                              // DefMapPoint.h:73
  void SetCoordinates(double a, double b, double c) { b1 = a; b2 = b; b3 = c; }   // DefMapPoint.h:80
  float mfMinDistance = 0.f;                                            // MapPoint.h:151
  LmKeyFrame* mpRefKF = nullptr;                                        // MapPoint.h:141
  // what SchwarpDatabase::add and DefORBmatcher::searchBySchwarp touch (anchor_pairs_hip.h)
  LmKeyFrame* GetReferenceKeyFrame() { return mpRefKF; }                // MapPoint.h:52
  bool IsInKeyFrame(LmKeyFrame* kf) { return mObservations.count(kf) != 0; }   // :59
  int GetIndexInKeyFrame(LmKeyFrame* kf) {                              // :58
    return mObservations.count(kf) ? (int)mObservations[kf] : -1;
  }
  void EraseObservation(LmKeyFrame* kf) {                               // :58 (MapPoint.cc:99-133, without the bad-flag rule)
    if (mObservations.erase(kf)) nObs--;
  }
  // what DefKeyFrame's constructor and SurfaceRegistration::registerSurfaces touch (surface_register_store_hip.h)
  std::map<LmKeyFrame*, std::array<float, 3>> PosesKeyframes;           // DefMapPoint.h:104 (unordered_map<KeyFrame*, cv::Mat>)
};

class LmKeyFrame {                             // Thirdparty/ORBSLAM_2/include/KeyFrame.h
 public:
  std::vector<LmMapPoint*> GetMapPointMatches() { return mvpMapPoints; }    // :89 (a copy)
  std::set<LmKeyFrame*> GetChilds() { return mspChildrens; }            // :80
  LmKeyFrame* GetParent() { return mpParent; }                          // :81
  bool isBad() { return bad; }                                          // :108
  unsigned long mnId = 0;                                               // :126
  unsigned long mnTrackReferenceForFrame = 0;                           // :141
  std::vector<LmMapPoint*> mvpMapPoints;                                // :199
  LmKeyFrame* mpParent = nullptr;                                       // :217
  std::set<LmKeyFrame*> mspChildrens;                                   // :218
  bool bad = false;
  // what DefLocalMapping::updateTemplate reads of the reference keyframe (template_switch_hip.h, mappoint_upkeep_hip.h)
  void addMapPoint(LmMapPoint* p, size_t idx) { mvpMapPoints[idx] = p; }    // :86 AddMapPoint
  LmMapPoint* GetMapPoint(size_t idx) { return mvpMapPoints[idx]; }         // :90
  void EraseMapPointMatch(size_t idx) { mvpMapPoints[idx] = nullptr; }      // :87
  int N = 0;                                                            // :149
  std::vector<KeyPoint> mvKeysUn;                                       // :163
  std::vector<uint8_t> mDescriptors;                                    // :171 N rows of 32 bytes (cv::Mat CV_8U)
  int mnScaleLevels = 8;                                                // :184
  std::vector<float> mvScaleFactors;                                    // :187
  float Ow[3] = {0, 0, 0};                                              // GetCameraCenter() :62
  float Twc[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};     // GetPoseInverse() :61 (cv::Mat 4x4 float)
  int rows = 0, cols = 0;                                               // imGray.rows, imGray.cols :228
  std::vector<float> surface_points;                                    // DefKeyFrame::surface->get3DSurfacePoint(i, x3c): 3 per key point
  std::vector<KeyPoint> mpKeypointNorm;                                 // DefKeyFrame.h: the normalised key points (surface_store_hip.h)
  // what KeyFrame::UpdateConnections touches (keyframe_create_hip.h)
  std::map<LmKeyFrame*, int> mConnectedKeyFrameWeights;                 // :237
  std::vector<LmKeyFrame*> mvpOrderedConnectedKeyFrames;                // :238
  std::vector<int> mvOrderedWeights;                                    // :239
  bool mbFirstConnection = true;                                        // :242
  void AddChild(LmKeyFrame* kf) { mspChildrens.insert(kf); }            // :77
  void AddConnection(LmKeyFrame* kf, int weight) {                      // :66 (KeyFrame.cc:149-185, with UpdateBestCovisibles)
    std::map<LmKeyFrame*, int>::iterator it = mConnectedKeyFrameWeights.find(kf);
    if (it != mConnectedKeyFrameWeights.end() && it->second == weight) return;
    mConnectedKeyFrameWeights[kf] = weight;
    std::vector<std::pair<int, LmKeyFrame*>> by_weight;
    for (const auto& kv : mConnectedKeyFrameWeights) by_weight.push_back(std::make_pair(kv.second, kv.first));
    std::sort(by_weight.begin(), by_weight.end());
    mvpOrderedConnectedKeyFrames.clear();
    mvOrderedWeights.clear();
    for (size_t i = by_weight.size(); i-- > 0;) {
      mvpOrderedConnectedKeyFrames.push_back(by_weight[i].second);
      mvOrderedWeights.push_back(by_weight[i].first);
    }
  }
  // what SchwarpDatabase::add, DefORBmatcher::findbyWarp and SchwarpDatabase::calculateSchwarps touch of a DefKeyFrame
  // (schwarp_database_hip.h, schwarp_store_hip.h)
  const uint8_t* descriptor(size_t i) const { return &mDescriptors[32 * i]; }   // mDescriptors.ptr(i)
  int gridCols() const { return 64; }                                   // FRAME_GRID_COLS
  int gridRows() const { return 48; }                                   // FRAME_GRID_ROWS
  int NCu = 0, NCv = 0, valdim = 2, KeyframesRelated = 0;               // DefKeyFrame.h
  double umin = 0, umax = 0, vmin = 0, vmax = 0;
  float fx = 0, fy = 0, cx = 0, cy = 0, mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;   // KeyFrame.h:152, :210-213
  std::vector<float> mvInvLevelSigma2;                                  // :190
  // what SurfaceRegistration::registerSurfaces writes (surface_register_store_hip.h)
  float Tcw[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};     // GetPose() :60
  void SetPose(const float* T) {                                        // :59 (KeyFrame.cc:97-111: Tcw, Ow = -Rwc * tcw, Twc)
    for (int i = 0; i < 16; i++) Tcw[i] = T[i];
    for (int i = 0; i < 3; i++) Ow[i] = -(Tcw[i] * Tcw[3] + Tcw[4 + i] * Tcw[7] + Tcw[8 + i] * Tcw[11]);
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) Twc[4 * r + c] = Tcw[4 * c + r];
      Twc[4 * r + 3] = Ow[r];
    }
  }
};

struct LmDiffProp {                            // Modules/Mapping/diffProp.h:52-83
  std::pair<LmKeyFrame*, LmKeyFrame*> KFToKF;
  size_t idx1 = 0, idx2 = 0;
  float I1u, I1v, I2u, I2v, J12a, J12b, J12c, J12d, J21a, J21b, J21c, J21d, H12uux, H12uuy, H12uvx, H12uvy, H12vvx, H12vvy;
};

class LmWarpDatabase {                         // Modules/Mapping/WarpDatabase.h:39-72
 public:
  typedef std::vector<std::shared_ptr<LmDiffProp>> kr2krdata;
  virtual ~LmWarpDatabase() = default;
  virtual void add(LmKeyFrame* kf) = 0;
  virtual void erase(LmKeyFrame* kf) = 0;
  virtual void clear() = 0;
  std::map<LmMapPoint*, kr2krdata>& getDiffDatabase() { return mapPointsDB_; }
  std::map<LmMapPoint*, bool>& getToProccess() { return newInformation_; }

 protected:
  std::map<LmMapPoint*, bool> newInformation_;
  std::map<LmMapPoint*, kr2krdata> mapPointsDB_;
};

class LmFrame {                                // Thirdparty/ORBSLAM_2/include/Frame.h
 public:
  float mTcw[16];                                                       // :180 cv::Mat 4x4 float
  float mOw[3];                                                         // :231 camera centre
  float fx, fy, cx, cy;                                                 // :121-124 (static in the reference)
  float mnMinX, mnMaxX, mnMinY, mnMaxY;                                 // :199-202 (static)
  int N = 0;                                                            // :140
  std::vector<KeyPoint> mvKeys, mvKeysUn;                               // :148-149
  std::vector<uint8_t> mDescriptors;                                    // :163 N rows of 32 bytes (cv::Mat CV_8U)
  std::vector<LmMapPoint*> mvpMapPoints;                                // :166
  std::vector<bool> mvbOutlier;                                         // :172
  int mnScaleLevels = 8;                                                // :190
  float mfLogScaleFactor = 0;                                           // :192
  std::vector<float> mvScaleFactors;                                    // :193
  unsigned long mnId = 0;                                               // :184
  LmKeyFrame* mpReferenceKF = nullptr;                                  // :187
  // what ORB_SLAM2::Optimizer::poseOptimization touches besides the above (pose_only_hip.h)
  std::vector<float> mvInvLevelSigma2;                                  // :195
  void SetPose(const float* Tcw) {                                      // :66 (Frame.cc:261-275: mTcw, then UpdatePoseMatrices)
    for (int i = 0; i < 16; i++) mTcw[i] = Tcw[i];
    for (int i = 0; i < 3; i++) mOw[i] = -(mTcw[i] * mTcw[3] + mTcw[4 + i] * mTcw[7] + mTcw[8 + i] * mTcw[11]);
  }
};

}  // namespace standin
