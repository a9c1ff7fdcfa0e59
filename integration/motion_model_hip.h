// Host integration shim of the end of a tracked frame and of the next frame's motion-model search on the resident map point store
// (include/defslam_hip.h: dsh_track_end_frame, dsh_motion_model_search), over MapPointStoreHIP of local_map_hip.h:
//
//   EndTrackedFrameHIP(store, CurrentFrame[, between])
//       drop-in for what DefTracking::Track does with the frame after a successful TrackLocalMap (Modules/Tracking/DefTracking.cc:169-172,
//       :185-191, :211): CleanMatches, then `between(CurrentFrame)` where the reference has EraseTemporalPoints and CreateNewKeyFrame
//       (:172-178; the frame still holds its outliers there), then the outlier drop.  Both loops run on the device against the store's
//       n_obs and are applied to the host frame from the outputs; the store keeps the result as its last-frame list, which is what
//       `mLastFrame = Frame(*mCurrentFrame)` is to the next search.  DefTracking::MonocularInitialization (:637) makes the same call.
//       Returns the number of entries the list holds, -1 when the library fails.
//   TrackWithMotionModelStoreHIP(store, CurrentFrame, LastFrame, bMono)
//       drop-in for the two searches of DefTracking::TrackWithMotionModel (:352-370) after SetPose: clears CurrentFrame.mvpMapPoints,
//       searches with th = 20 and again with th = 25 when fewer than 20 matched -- both on the device, from the store's own positions,
//       descriptors, bad flags, facets and n_obs; only the frame's key points travel up -- and writes mvpMapPoints from the ids.  LastFrame
//       must be the frame EndTrackedFrameHIP saw last (its N is checked); nothing else of it is read.  Returns nmatches (the caller
//       applies < 15, :373), -1 when the library fails or bMono is false.
// Templates over the reference's classes; the type-specific accessors are TrackAccess<FrameT, MapPointT> of tracking_search_hip.h.
#pragma once
#include <cstdint>
#include <vector>

#include "local_map_hip.h"

namespace defslam_hip {

template <class FrameT, class KeyFrameT, class MapPointT, class Between>
int EndTrackedFrameHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, FrameT& CurrentFrame, Between between, dsh_track_end_counts* counts = nullptr) {
  const int N = CurrentFrame.N;
  std::vector<int32_t> fp(N), oct(N), after(N > 0 ? N : 1);
  std::vector<uint8_t> outlier(N), flag(N > 0 ? N : 1);
  for (int i = 0; i < N; i++) {
    fp[i] = CurrentFrame.mvpMapPoints[i] ? store.id(CurrentFrame.mvpMapPoints[i]) : -1;
    outlier[i] = CurrentFrame.mvbOutlier[i] ? 1 : 0;
    oct[i] = CurrentFrame.mvKeys[i].octave;
  }
  dsh_track_end_counts c;
  if (dsh_track_end_frame(store.handle(), N, fp.data(), outlier.data(), oct.data(), after.data(), flag.data(), &c) != DSH_OK) return -1;
  for (int i = 0; i < N; i++) {                                        // CleanMatches (DefTracking.cc:667-679)
    if (after[i] < 0) CurrentFrame.mvpMapPoints[i] = nullptr;
    CurrentFrame.mvbOutlier[i] = flag[i] != 0;
  }
  between(CurrentFrame);                                               // :172-178
  for (int i = 0; i < N; i++)                                          // :185-191
    if (CurrentFrame.mvpMapPoints[i] && CurrentFrame.mvbOutlier[i]) CurrentFrame.mvpMapPoints[i] = nullptr;
  if (counts) *counts = c;
  return c.kept;
}

template <class FrameT, class KeyFrameT, class MapPointT>
int EndTrackedFrameHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, FrameT& CurrentFrame, dsh_track_end_counts* counts = nullptr) {
  return EndTrackedFrameHIP(store, CurrentFrame, [](FrameT&) {}, counts);
}

template <class FrameT, class KeyFrameT, class MapPointT>
int TrackWithMotionModelStoreHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, FrameT& CurrentFrame, const FrameT& LastFrame, const bool bMono,
                                 float* th_used = nullptr, int grid_cols = 64, int grid_rows = 48) {
  if (!bMono) return -1;   // the stereo branches (bForward / bBackward, mvuRight) are not part of the device search
  int32_t n_last = 0;
  if (dsh_track_last_frame(store.handle(), LastFrame.N, nullptr, nullptr, &n_last) != DSH_OK || n_last != LastFrame.N) return -1;
  for (auto& p : CurrentFrame.mvpMapPoints) p = nullptr;              // DefTracking.cc:352-353
  TrackFrameView<FrameT, MapPointT> v(CurrentFrame, grid_cols, grid_rows);
  std::vector<int32_t> fp(CurrentFrame.N > 0 ? CurrentFrame.N : 1);
  int32_t n = 0;
  if (dsh_motion_model_search(store.handle(), &v.f, 20.0f, 25.0f, 20, fp.data(), nullptr, &n, th_used) != DSH_OK) return -1;   // :356-370
  for (int j = 0; j < CurrentFrame.N; j++)
    if (fp[j] >= 0) CurrentFrame.mvpMapPoints[j] = store.point(fp[j]);   // DefORBmatcher.cc:406
  return n;
}

}  // namespace defslam_hip
