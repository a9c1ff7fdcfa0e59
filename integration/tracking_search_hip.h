// Host integration shim of the tracking searches (include/defslam_hip.h: dsh_search_by_projection_*):
//
//   SearchByProjectionHIP(ctx, CurrentFrame, LastFrame, th, bMono)
//       drop-in for ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono) (Thirdparty/ORBSLAM_2/src/ORBmatcher.cc:1360-1510),
//       the call of DefTracking::TrackWithMotionModel (Modules/Tracking/DefTracking.cc:358,368): queries are the last frame's map
//       points that are present and not outliers, in index order; fills CurrentFrame.mvpMapPoints and returns nmatches.
//   SearchLocalPointsHIP(ctx, CurrentFrame, vpLocalMapPoints, th)
//       drop-in for Tracking::SearchLocalPoints (Tracking.cc:1405-1470, called at DefTracking.cc:240): the bookkeeping of the frame's
//       map points (:1408-1425), isInFrustum(pMP, 0.5) of every local point not seen in this frame (:1443-1456: mbTrackInView,
//       mTrackProjX / Y, mnTrackScaleLevel, mTrackViewCos, IncreaseVisible) and ORBmatcher(0.8).SearchByProjection(F, points, th)
//       (:1468), whose matches overwrite CurrentFrame.mvpMapPoints.  Returns the number of matches.
// Monocular only (DefSLAM): bMono == false is refused.  Both return -1 when the library fails (dsh_last_error(ctx) has the text):
// no match is written then (SearchLocalPointsHIP has already done the bookkeeping of :1408-1425, as the reference does first).
//
// Like defslam_hip_shim.h the functions are templates over the reference's classes; the only type-specific pieces are the accessors of
// `TrackAccess<FrameT, MapPointT>`: cv::Mat in DefSLAM (GetWorldPos() / GetNormal() / GetDescriptor() / mTcw / mOw /
// mDescriptors.ptr(j), to be specialised there), plain arrays in the stand-ins of standin_tracking_types.h.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "../include/defslam_hip.h"

namespace defslam_hip {

template <class FrameT, class MapPointT>
struct TrackAccess {
  static void pose(const FrameT& f, float* T16) { std::memcpy(T16, f.mTcw, 16 * sizeof(float)); }
  static void center(const FrameT& f, float* Ow) { std::memcpy(Ow, f.mOw, 3 * sizeof(float)); }
  static const uint8_t* descriptors(const FrameT& f) { return f.mDescriptors.data(); }   // N x 32, row j = mDescriptors.row(j)
  static void world_pos(MapPointT* p, float* x) { std::memcpy(x, p->pos, 3 * sizeof(float)); }
  static void set_world_pos(MapPointT* p, const float* x) { std::memcpy(p->pos, x, 3 * sizeof(float)); }   // mWorldPos (track_close_hip.h)
  static void normal(MapPointT* p, float* n) { std::memcpy(n, p->normal, 3 * sizeof(float)); }
  static void descriptor(MapPointT* p, uint8_t* d) { std::memcpy(d, p->desc, 32); }
};

// the current frame as the library sees it; state[j] from mvpMapPoints[j]: 0 none, 1 a map point with observations, 2 one without
template <class FrameT, class MapPointT>
struct TrackFrameView {
  float T[16];
  std::vector<float> kp;
  std::vector<int32_t> octave;
  std::vector<uint8_t> state;
  dsh_track_frame f;
  TrackFrameView(const FrameT& F, int grid_cols, int grid_rows) : kp(2 * (size_t)F.N), octave(F.N), state(F.N) {
    typedef TrackAccess<FrameT, MapPointT> A;
    A::pose(F, T);
    std::memset(&f, 0, sizeof(f));
    f.Tcw = T;
    A::center(F, f.Ow);
    f.K[0] = F.fx; f.K[1] = F.fy; f.K[2] = F.cx; f.K[3] = F.cy;
    f.bounds[0] = F.mnMinX; f.bounds[1] = F.mnMaxX; f.bounds[2] = F.mnMinY; f.bounds[3] = F.mnMaxY;
    f.grid_cols = grid_cols;
    f.grid_rows = grid_rows;
    f.levels = F.mnScaleLevels;
    f.scale_factors = F.mvScaleFactors.data();
    f.log_scale_factor = F.mfLogScaleFactor;
    f.N = F.N;
    for (int j = 0; j < F.N; j++) {
      kp[2 * j] = F.mvKeysUn[j].pt.x;
      kp[2 * j + 1] = F.mvKeysUn[j].pt.y;
      octave[j] = F.mvKeysUn[j].octave;
      MapPointT* p = F.mvpMapPoints[j];
      state[j] = !p ? 0 : (p->Observations() > 0 ? 1 : 2);   // ORBmatcher.cc:1439-1441 / :90-92
    }
    f.kp = kp.data();
    f.octave = octave.data();
    f.desc = A::descriptors(F);
    f.state = state.data();
  }
};

template <class FrameT, class MapPointT>
int SearchByProjectionHIP(dsh_ctx* ctx, FrameT& CurrentFrame, const FrameT& LastFrame, const float th, const bool bMono,
                          int grid_cols = 64, int grid_rows = 48) {
  typedef TrackAccess<FrameT, MapPointT> A;
  if (!bMono) return -1;   // the stereo branches (bForward / bBackward, mvuRight) are not part of the device search
  std::vector<MapPointT*> src;
  std::vector<float> xyz;
  std::vector<int32_t> oct;
  std::vector<uint8_t> desc;
  for (int i = 0; i < LastFrame.N; i++) {                              // ORBmatcher.cc:1384-1390
    MapPointT* p = LastFrame.mvpMapPoints[i];
    if (!p || LastFrame.mvbOutlier[i]) continue;
    float x[3];
    uint8_t d[32];
    A::world_pos(p, x);
    A::descriptor(p, d);
    xyz.insert(xyz.end(), x, x + 3);
    oct.push_back(LastFrame.mvKeys[i].octave);                         // :1410
    desc.insert(desc.end(), d, d + 32);
    src.push_back(p);
  }
  TrackFrameView<FrameT, MapPointT> v(CurrentFrame, grid_cols, grid_rows);
  std::vector<int32_t> match(src.size());
  int32_t n = 0;
  if (dsh_search_by_projection_frame(ctx, &v.f, (int)src.size(), xyz.data(), oct.data(), desc.data(), th, match.data(), &n) != DSH_OK) return -1;
  for (size_t q = 0; q < src.size(); q++)
    if (match[q] >= 0) CurrentFrame.mvpMapPoints[match[q]] = src[q];   // :1466
  return n;
}

template <class FrameT, class MapPointT>
int SearchLocalPointsHIP(dsh_ctx* ctx, FrameT& CurrentFrame, const std::vector<MapPointT*>& vpLocalMapPoints, const float th,
                         int grid_cols = 64, int grid_rows = 48) {
  typedef TrackAccess<FrameT, MapPointT> A;
  for (auto& p : CurrentFrame.mvpMapPoints) {                          // Tracking.cc:1408-1425
    if (!p) continue;
    if (p->isBad()) {
      p = nullptr;
    } else {
      p->IncreaseVisible();
      p->mnLastFrameSeen = CurrentFrame.mnId;
      p->mbTrackInView = false;
    }
  }
  std::vector<MapPointT*> pts;
  std::vector<float> xyz, nrm, maxd;
  std::vector<uint8_t> desc, skip;
  for (MapPointT* p : vpLocalMapPoints) {                              // :1443-1452
    if (!p) continue;
    float x[3], n[3];
    uint8_t d[32];
    A::world_pos(p, x);
    A::normal(p, n);
    A::descriptor(p, d);
    xyz.insert(xyz.end(), x, x + 3);
    nrm.insert(nrm.end(), n, n + 3);
    maxd.push_back(p->mfMaxDistance);
    desc.insert(desc.end(), d, d + 32);
    skip.push_back(p->mnLastFrameSeen == CurrentFrame.mnId || p->isBad() ? 1 : 0);
    pts.push_back(p);
  }
  const int Q = (int)pts.size();
  TrackFrameView<FrameT, MapPointT> v(CurrentFrame, grid_cols, grid_rows);
  std::vector<int32_t> match(Q), level(Q);
  std::vector<uint8_t> in_view(Q);
  std::vector<float> uv(2 * (size_t)Q), vcos(Q);
  dsh_track_problem pr;
  std::memset(&pr, 0, sizeof(pr));
  pr.frame = v.f;
  pr.mode = DSH_TRACK_LOCAL;
  pr.th = th;
  pr.Q = Q;
  pr.xyz = xyz.data();
  pr.normal = nrm.data();
  pr.max_distance = maxd.data();
  pr.desc = desc.data();
  pr.skip = skip.data();
  pr.match = match.data();
  pr.in_view = in_view.data();
  pr.level = level.data();
  pr.uv = uv.data();
  pr.view_cos = vcos.data();
  if (dsh_search_by_projection_batch(ctx, 1, &pr) != DSH_OK) return -1;
  for (int q = 0; q < Q; q++) {
    if (skip[q]) continue;                                             // :1448-1451: not projected, mbTrackInView untouched
    MapPointT* p = pts[q];
    p->mbTrackInView = in_view[q] != 0;                                // Frame.cc:340, :383-388
    if (!in_view[q]) continue;
    p->mTrackProjX = uv[2 * q];
    p->mTrackProjY = uv[2 * q + 1];
    p->mnTrackScaleLevel = level[q];
    p->mTrackViewCos = vcos[q];
    p->IncreaseVisible();                                              // Tracking.cc:1456
  }
  for (int q = 0; q < Q; q++)
    if (match[q] >= 0) CurrentFrame.mvpMapPoints[match[q]] = pts[q];   // ORBmatcher.cc:127 (overwrites)
  return pr.nmatches;
}

}  // namespace defslam_hip
