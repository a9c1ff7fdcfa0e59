// Host integration shim of the creation of a keyframe on the resident stores and of its covisibility connections
// (include/defslam_hip.h: dsh_keyframe_create, dsh_keyframe_update_connections), over MapPointStoreHIP of local_map_hip.h and
// KeyFrameStoreHIP of mappoint_upkeep_hip.h:
//
//   CreateNewKeyFrameStoreHIP(store, kfstore, CurrentFrame, pKF)
//       for DefTracking::CreateNewKeyFrame (Modules/Tracking/DefTracking.cc:696-707), inside the callback of EndTrackedFrameHIP
//       (motion_model_hip.h), where the reference creates the keyframe: pKF is the object `new DefKeyFrame(*mCurrentFrame, ..)` made.
//       Its constructor keeps NormaliseKeypoints and `new Surface`; what it copied of the frame goes into both stores in ONE call --
//       descriptor rows, octaves, pyramid, the camera centre of mTcw, the Surface with mpKeypointNorm -- and the table does not travel
//       at all: the store copies the keyframe candidate that dsh_track_end_frame left on the device.  The PosesKeyframes loop of the
//       constructor (Modules/Common/DefKeyFrame.cc:60-74) runs in the same call and can go from the host: nothing else reads it.
//       pKF is registered under the new slot in both shims.  Returns the slot, -1 when the library refuses or when the store holds a
//       keyframe the shim does not know (added behind its back); nothing is created then.
//   UpdateConnectionsStoreHIP(store, pKF, th)
//       drop-in for KeyFrame::UpdateConnections (Thirdparty/ORBSLAM_2/src/KeyFrame.cc:326-419) of a keyframe of the store: the walk over
//       GetObservations() of every point runs on the device over the observation log, and the reference's mutations are written on the
//       host objects: mConnectedKeyFrameWeights, mvpOrderedConnectedKeyFrames, mvOrderedWeights, on the first connection mpParent,
//       AddChild and mbFirstConnection, and AddConnection(pKF, w) on the listed keyframes, which the store does not keep.
//       Returns false when the library refuses; nothing is written then.
// Templates over the reference's classes; the type-specific accessors are CreateAccess<FrameT, KeyFrameT>: cv::Mat in DefSLAM (mTcw,
// mDescriptors.ptr(), the writers of KeyFrame's protected connection members, which need a friend declaration there), plain members in
// the stand-ins of standin_localmap_types.h.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "local_map_hip.h"
#include "mappoint_upkeep_hip.h"

namespace defslam_hip {

template <class FrameT, class KeyFrameT>
struct CreateAccess {
  static void pose(const FrameT& F, float* T16) { std::memcpy(T16, F.mTcw, 16 * sizeof(float)); }
  static const uint8_t* descriptors(const FrameT& F) { return F.mDescriptors.data(); }
  static void keypoint_norm(KeyFrameT* kf, int i, float* uv) {
    uv[0] = kf->mpKeypointNorm[i].pt.x;
    uv[1] = kf->mpKeypointNorm[i].pt.y;
  }
};

template <class FrameT, class KeyFrameT, class MapPointT>
int CreateNewKeyFrameStoreHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, KeyFrameStoreHIP<KeyFrameT, MapPointT>& kfstore, const FrameT& F, KeyFrameT* pKF,
                              dsh_keyframe_create_result* result = nullptr) {
  typedef CreateAccess<FrameT, KeyFrameT> A;
  const int N = F.N;
  std::vector<int32_t> oct(N > 0 ? N : 1);
  std::vector<float> kpn(2 * (size_t)(N > 0 ? N : 1));
  for (int i = 0; i < N; i++) {
    oct[i] = F.mvKeysUn[i].octave;
    A::keypoint_norm(pKF, i, &kpn[2 * (size_t)i]);
  }
  float Tcw[16];
  A::pose(F, Tcw);
  dsh_mp_keyframe k;
  std::memset(&k, 0, sizeof(k));
  k.N = N;
  k.desc = A::descriptors(F);
  k.octave = oct.data();
  k.levels = F.mnScaleLevels;
  k.scale_factors = F.mvScaleFactors.data();
  dsh_keyframe_create_input in;
  in.kfdb = kfstore.db();
  in.kf = &k;
  in.Tcw = Tcw;
  in.points = nullptr;                                                 // the candidate of the dsh_track_end_frame that just ran
  in.kpn = kpn.data();
  // the shim must know every keyframe of the store, or the new slot would have no object behind it: checked before anything is created
  if (store.keyframe_count() != dsh_mpdb_keyframe_count(store.handle())) return -1;
  dsh_keyframe_create_result r;
  if (dsh_keyframe_create(store.handle(), &in, &r) != DSH_OK) return -1;
  store.AdoptKeyFrame(pKF, r.slot);                                    // r.slot == keyframe_count(): checked above
  kfstore.Adopt(pKF, r.slot);
  if (result) *result = r;
  return r.slot;
}

template <class KeyFrameT, class MapPointT>
bool UpdateConnectionsStoreHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, KeyFrameT* pKF, int th = 100, dsh_keyframe_connections* result = nullptr) {
  const int32_t K = dsh_mpdb_keyframe_count(store.handle());
  const size_t cap = K > 0 ? K : 1;
  std::vector<int32_t> ck(cap), cw(cap), ok(cap), ow(cap);
  dsh_keyframe_connections c;
  if (dsh_keyframe_update_connections(store.handle(), store.slot(pKF), th, (int32_t)cap, ck.data(), cw.data(), ok.data(), ow.data(), &c) != DSH_OK) return false;
  if (result) *result = c;
  if (c.n_counted == 0) return true;                                   // KeyFrame.cc:361
  for (int i = 0; i < c.n_connected; i++) store.keyframe(ok[i])->AddConnection(pKF, ow[i]);   // :385, :392
  pKF->mConnectedKeyFrameWeights.clear();                              // :408-410
  for (int i = 0; i < c.n_counted; i++) pKF->mConnectedKeyFrameWeights[store.keyframe(ck[i])] = cw[i];
  pKF->mvpOrderedConnectedKeyFrames.clear();
  pKF->mvOrderedWeights.assign(ow.begin(), ow.begin() + c.n_connected);
  for (int i = 0; i < c.n_connected; i++) pKF->mvpOrderedConnectedKeyFrames.push_back(store.keyframe(ok[i]));
  if (c.parent_set) {                                                  // :412-417
    pKF->mpParent = store.keyframe(c.parent);
    pKF->mpParent->AddChild(pKF);
    pKF->mbFirstConnection = false;
  }
  return true;
}

}  // namespace defslam_hip
