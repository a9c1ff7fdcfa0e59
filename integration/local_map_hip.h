// Host integration shim of the local map from the resident map point store (include/defslam_hip.h: dsh_mpdb_*, dsh_local_map_*):
//
//   MapPointStoreHIP<KeyFrameT, MapPointT>
//       owns a dsh_mpdb and the two dictionaries pointer <-> number (MapPoint* <-> id, KeyFrame* <-> slot).  The mapping thread calls
//       it where it changes the map: AddMapPoint / AddKeyFrame when one is created, AddObservation / EraseObservation next to
//       MapPoint::AddObservation / EraseObservation, SetKeyFramePoint next to KeyFrame::AddMapPoint / EraseMapPointMatch, SetParent next
//       to KeyFrame::ChangeParent, SetBad next to SetBadFlag, UpdatePositions after DefPoseOptimization moved the points (or, with SetEmbedding next to
//       DefMapPoint::SetFacet / SetCoordinates, ClearEmbedding next to DefMap::clearTemplate and SeedLocalPoints at the initialisation,
//       nothing per frame: track_close_hip.h moves the points on the device).
//   UpdateLocalMapHIP(store, CurrentFrame, mvpLocalKeyFrames, mvpLocalMapPoints, mpReferenceKF)
//       drop-in for Tracking::UpdateLocalMap (Thirdparty/ORBSLAM_2/src/Tracking.cc:1472-1480, called at DefTracking.cc:237): fills the
//       two vectors and does the reference's write-backs -- bad points leave CurrentFrame.mvpMapPoints (:1529), the listed keyframes and
//       the local points get mnTrackReferenceForFrame = CurrentFrame.mnId (:1561, :1589, :1606, :1618, DefTracking.cc:446), and
//       mpReferenceKF / CurrentFrame.mpReferenceKF become pKFmax when there is one (:1626-1627).  Returns the number of local points.
//   SearchLocalPointsStoreHIP(store, CurrentFrame, mvpLocalMapPoints, th)
//       drop-in for Tracking::SearchLocalPoints (:1405-1470) after UpdateLocalMapHIP of the same frame: the queries are the resident
//       local points, only the frame's key points travel up; the write-backs are those of SearchLocalPointsHIP
//       (tracking_search_hip.h).  Returns the number of matches.
// Both return -1 when the library fails (dsh_last_error of the store's context has the text).  Pointer order in the reference's
// containers becomes index order here (keyframes by slot, points by id): register keyframes and points in creation order.
//
// Templates over the reference's classes; the type-specific accessors are TrackAccess<FrameT, MapPointT> of tracking_search_hip.h.
#pragma once
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "../include/defslam_hip.h"
#include "tracking_search_hip.h"

namespace defslam_hip {

template <class KeyFrameT, class MapPointT>
class MapPointStoreHIP {
 public:
  explicit MapPointStoreHIP(dsh_ctx* ctx, int points = 4096, int keyframes = 64, long long observations = 1 << 16) {
    dsh_mpdb_desc d;
    d.ctx = ctx;
    d.point_capacity = points;
    d.keyframe_capacity = keyframes;
    d.observation_capacity = observations;
    if (dsh_mpdb_create(&d, &db_) != DSH_OK) db_ = nullptr;
  }
  ~MapPointStoreHIP() { if (db_) dsh_mpdb_destroy(db_); }
  MapPointStoreHIP(const MapPointStoreHIP&) = delete;
  MapPointStoreHIP& operator=(const MapPointStoreHIP&) = delete;

  dsh_mpdb* handle() const { return db_; }
  bool ok() const { return db_ != nullptr; }
  int id(MapPointT* p) const { auto it = ids_.find(p); return it == ids_.end() ? -1 : it->second; }
  int slot(KeyFrameT* k) const { auto it = slots_.find(k); return it == slots_.end() ? -1 : it->second; }
  MapPointT* point(int id) const { return points_[id]; }
  KeyFrameT* keyframe(int slot) const { return kfs_[slot]; }

  // a batch of new map points (DefLocalMapping::CreateNewMapPoints, the initialisation); false when the library refuses
  template <class FrameT>
  bool AddMapPoints(const std::vector<MapPointT*>& pts) {
    typedef TrackAccess<FrameT, MapPointT> A;
    const size_t n = pts.size();
    std::vector<float> xyz(3 * n), nrm(3 * n), maxd(n);
    std::vector<uint8_t> desc(32 * n), bad(n);
    for (size_t i = 0; i < n; i++) {
      A::world_pos(pts[i], &xyz[3 * i]);
      A::normal(pts[i], &nrm[3 * i]);
      A::descriptor(pts[i], &desc[32 * i]);
      maxd[i] = pts[i]->mfMaxDistance;
      bad[i] = pts[i]->isBad() ? 1 : 0;
    }
    int32_t first = -1;
    if (dsh_mpdb_add_points(db_, (int)n, xyz.data(), nrm.data(), maxd.data(), desc.data(), bad.data(), &first) != DSH_OK) return false;
    for (size_t i = 0; i < n; i++) {
      ids_[pts[i]] = first + (int)i;
      points_.push_back(pts[i]);
    }
    return true;
  }
  // a new keyframe with its table (Map::AddKeyFrame); its map points are registered already
  bool AddKeyFrame(KeyFrameT* kf) {
    const std::vector<MapPointT*> mps = kf->GetMapPointMatches();
    std::vector<int32_t> table(mps.size());
    for (size_t j = 0; j < mps.size(); j++) table[j] = mps[j] ? id(mps[j]) : -1;
    KeyFrameT* par = kf->GetParent();
    int32_t s = -1;
    if (dsh_mpdb_add_keyframe(db_, (int32_t)table.size(), table.data(), par ? slot(par) : -1, kf->isBad() ? 1 : 0, &s) != DSH_OK) return false;
    slots_[kf] = s;
    kfs_.push_back(kf);
    return true;
  }
  bool AddObservations(const std::vector<MapPointT*>& pts, const std::vector<KeyFrameT*>& kfs) { return observations(pts, kfs, true); }
  bool EraseObservations(const std::vector<MapPointT*>& pts, const std::vector<KeyFrameT*>& kfs) { return observations(pts, kfs, false); }
  bool SetKeyFramePoint(KeyFrameT* kf, int idx, MapPointT* p) { return dsh_mpdb_set_keyframe_point(db_, slot(kf), idx, p ? id(p) : -1) == DSH_OK; }
  bool SetParent(KeyFrameT* kf, KeyFrameT* parent) { return dsh_mpdb_set_keyframe_parent(db_, slot(kf), parent ? slot(parent) : -1) == DSH_OK; }
  bool SetBad(KeyFrameT* kf) { return dsh_mpdb_set_keyframe_bad(db_, slot(kf), 1) == DSH_OK; }
  bool SetBad(MapPointT* p) {
    const int32_t i = id(p);
    return dsh_mpdb_set_points_bad(db_, 1, &i, nullptr) == DSH_OK;
  }
  // DefMapPoint::SetFacet + SetCoordinates of these points (a point whose getFacet() is null loses its facet in the store too);
  // index_of(Node*) is the node's index in the template, and pointer order of a facet's nodes must be index order
  template <class NodeIndex>
  bool SetEmbedding(const std::vector<MapPointT*>& pts, NodeIndex index_of) {
    const size_t n = pts.size();
    std::vector<int32_t> ids(n), nodes(3 * n, -1);
    std::vector<double> bary(3 * n, 0.0);
    for (size_t i = 0; i < n; i++) {
      ids[i] = id(pts[i]);
      if (!pts[i]->getFacet()) continue;
      const auto set = pts[i]->getFacet()->getNodes();
      int k = 0;
      for (auto* nd : set) nodes[3 * i + k++] = index_of(nd);
      bary[3 * i] = pts[i]->b1; bary[3 * i + 1] = pts[i]->b2; bary[3 * i + 2] = pts[i]->b3;
    }
    return dsh_trackstate_set_embedding(db_, (int)n, ids.data(), nodes.data(), bary.data()) == DSH_OK;
  }
  bool ClearEmbedding() { return dsh_trackstate_clear_embedding(db_) == DSH_OK; }                 // DefMap::clearTemplate
  // DefTracking::MonocularInitialization (DefTracking.cc:641,645): the local and the reference list become pts (in creation order)
  bool SeedLocalPoints(const std::vector<MapPointT*>& pts) {
    std::vector<int32_t> ids(pts.size());
    for (size_t i = 0; i < pts.size(); i++) ids[i] = id(pts[i]);
    return dsh_trackstate_seed_local_points(db_, (int)ids.size(), ids.data()) == DSH_OK;
  }
  int point_count() const { return (int)points_.size(); }
  int keyframe_count() const { return (int)kfs_.size(); }
  // a point the store created itself (dsh_template_switch): the host object made for it takes the id; ids arrive in order
  bool AdoptPoint(MapPointT* p, int id) {
    if (id != (int)points_.size()) return false;
    ids_[p] = id;
    points_.push_back(p);
    return true;
  }
  // a keyframe the library put into the store itself (dsh_keyframe_create): its host object takes the slot; slots arrive in order
  bool AdoptKeyFrame(KeyFrameT* kf, int slot) {
    if (slot != (int)kfs_.size()) return false;
    slots_[kf] = slot;
    kfs_.push_back(kf);
    return true;
  }
  // DefPoseOptimization moved these points (DefMapPoint::RecalculatePosition)
  template <class FrameT>
  bool UpdatePositions(const std::vector<MapPointT*>& pts) {
    std::vector<int32_t> ids(pts.size());
    std::vector<float> xyz(3 * pts.size());
    for (size_t i = 0; i < pts.size(); i++) {
      ids[i] = id(pts[i]);
      TrackAccess<FrameT, MapPointT>::world_pos(pts[i], &xyz[3 * i]);
    }
    return dsh_mpdb_update_points(db_, (int)ids.size(), ids.data(), DSH_MPDB_POSITION, xyz.data(), nullptr, nullptr, nullptr) == DSH_OK;
  }

 private:
  bool observations(const std::vector<MapPointT*>& pts, const std::vector<KeyFrameT*>& kfs, bool add) {
    std::vector<int32_t> p(pts.size()), k(pts.size());
    for (size_t i = 0; i < pts.size(); i++) {
      p[i] = id(pts[i]);
      k[i] = slot(kfs[i]);
    }
    return (add ? dsh_mpdb_add_observations : dsh_mpdb_erase_observations)(db_, (int)p.size(), p.data(), k.data()) == DSH_OK;
  }
  dsh_mpdb* db_ = nullptr;
  std::unordered_map<MapPointT*, int> ids_;
  std::unordered_map<KeyFrameT*, int> slots_;
  std::vector<MapPointT*> points_;
  std::vector<KeyFrameT*> kfs_;
};

template <class FrameT, class KeyFrameT, class MapPointT>
int UpdateLocalMapHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, FrameT& CurrentFrame, std::vector<KeyFrameT*>& mvpLocalKeyFrames,
                      std::vector<MapPointT*>& mvpLocalMapPoints, KeyFrameT*& mpReferenceKF, std::vector<int32_t>* votes = nullptr) {
  const int N = CurrentFrame.N;
  std::vector<int32_t> fp(N);
  for (int i = 0; i < N; i++) fp[i] = CurrentFrame.mvpMapPoints[i] ? store.id(CurrentFrame.mvpMapPoints[i]) : -1;
  const int32_t K = dsh_mpdb_keyframe_count(store.handle());
  std::vector<uint8_t> fbad(N);
  std::vector<int32_t> kf(K > 0 ? K : 1), vt(K > 0 ? K : 1);
  int32_t n_voted = 0, n_kf = 0, ref = -1, n_pts = 0;
  if (dsh_local_map_update(store.handle(), N, fp.data(), fbad.data(), (int32_t)kf.size(), kf.data(), vt.data(), &n_voted, &n_kf, &ref, &n_pts) != DSH_OK)
    return -1;
  for (int i = 0; i < N; i++)
    if (fbad[i]) CurrentFrame.mvpMapPoints[i] = nullptr;                          // Tracking.cc:1529
  if (n_voted > 0 || n_kf == 0) {                                                 // :1534: without a vote the reference returns before the clear
    mvpLocalKeyFrames.clear();
    for (int i = 0; i < n_kf; i++) {
      KeyFrameT* k = store.keyframe(kf[i]);
      k->mnTrackReferenceForFrame = CurrentFrame.mnId;                            // :1561, :1589, :1606, :1618
      mvpLocalKeyFrames.push_back(k);
    }
  }
  if (votes) votes->assign(vt.begin(), vt.begin() + n_voted);
  if (ref >= 0) {                                                                 // :1624-1628
    mpReferenceKF = store.keyframe(ref);
    CurrentFrame.mpReferenceKF = mpReferenceKF;
  }
  std::vector<int32_t> ids(n_pts > 0 ? n_pts : 1);
  int32_t got = 0;
  if (dsh_local_map_points(store.handle(), (int32_t)ids.size(), ids.data(), &got) != DSH_OK) return -1;
  mvpLocalMapPoints.resize(got);
  for (int q = 0; q < got; q++) {
    MapPointT* p = store.point(ids[q]);
    p->mnTrackReferenceForFrame = CurrentFrame.mnId;                              // DefTracking.cc:446
    mvpLocalMapPoints[q] = p;
  }
  return got;
}

template <class FrameT, class KeyFrameT, class MapPointT>
int SearchLocalPointsStoreHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, FrameT& CurrentFrame, const std::vector<MapPointT*>& mvpLocalMapPoints,
                              const float th, int grid_cols = 64, int grid_rows = 48) {
  for (auto& p : CurrentFrame.mvpMapPoints) {                                     // Tracking.cc:1408-1425
    if (!p) continue;
    if (p->isBad()) {
      p = nullptr;
    } else {
      p->IncreaseVisible();
      p->mnLastFrameSeen = CurrentFrame.mnId;
      p->mbTrackInView = false;
    }
  }
  const int Q = (int)mvpLocalMapPoints.size();
  TrackFrameView<FrameT, MapPointT> v(CurrentFrame, grid_cols, grid_rows);
  const size_t cap = Q > 0 ? Q : 1;
  std::vector<int32_t> ids(cap), match(cap), level(cap);
  std::vector<uint8_t> in_view(cap);
  std::vector<float> uv(2 * cap), vcos(cap);
  int32_t n = 0;
  if (dsh_local_map_search(store.handle(), &v.f, th, Q, ids.data(), match.data(), in_view.data(), level.data(), uv.data(), vcos.data(), &n) != DSH_OK)
    return -1;
  for (int q = 0; q < Q; q++) {
    MapPointT* p = mvpLocalMapPoints[q];
    if (store.id(p) != ids[q]) return -1;                                         // the vector is not the one UpdateLocalMapHIP filled
    if (p->mnLastFrameSeen == CurrentFrame.mnId || p->isBad()) continue;          // :1449-1452: not projected, mbTrackInView untouched
    p->mbTrackInView = in_view[q] != 0;                                           // Frame.cc:340, :383-388
    if (!in_view[q]) continue;
    p->mTrackProjX = uv[2 * q];
    p->mTrackProjY = uv[2 * q + 1];
    p->mnTrackScaleLevel = level[q];
    p->mTrackViewCos = vcos[q];
    p->IncreaseVisible();                                                         // Tracking.cc:1456
  }
  for (int q = 0; q < Q; q++)
    if (match[q] >= 0) CurrentFrame.mvpMapPoints[match[q]] = mvpLocalMapPoints[q];    // ORBmatcher.cc:127 (overwrites)
  return n;
}

}  // namespace defslam_hip
