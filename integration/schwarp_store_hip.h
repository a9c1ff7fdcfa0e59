// Host integration shim of one anchor of SchwarpDatabase::add on the resident stores (include/defslam_hip.h: dsh_keyframe_set_view,
// dsh_keyframe_warp_pair), over MapPointStoreHIP of local_map_hip.h and the lists of anchor_pairs_hip.h:
//
//   SetViewStoreHIP(store, kf)        what the pair call reads of a keyframe beyond its resident Surface: mvKeysUn[i].pt, fx, fy, cx, cy,
//                                     mnMinX .. mnMaxY, FRAME_GRID_COLS / ROWS and the warp grid (umin, umax, NCu, vmin, vmax, NCv,
//                                     valdim).  Once per keyframe, after dsh_keyframe_surface_init (surface_store_hip.h).
//   WarpPairStoreHIP(store, in, KF1, KF2, lists, a, result)
//       DefORBmatcher::findbyWarp (Modules/Matching/DefORBmatcher.cc:47-71) and SchwarpDatabase::calculateSchwarps
//       (Modules/Mapping/SchwarpDatabase.cc:145-349) for anchor a of `lists` in one library call; then the reference's mutations are
//       written back on the host objects, in the reference's order: EraseMapPointMatch of the filtered matches (DefORBmatcher.cc:172),
//       AddObservation / addMapPoint of the matched queries in query order (:58-66), and over the kept list EraseObservation +
//       EraseMapPointMatch of the dropped matches (SchwarpDatabase.cc:288-292).  The later anchors' lists follow through DropQueryHIP
//       and DropMatchHIP.  result.stored lists the points whose record went into the database (newInformation_, :345).
//   SchwarpDatabaseStoreHIP<Base, ..>::add(KF2)
//       drop-in for SchwarpDatabase::add (SchwarpDatabase.cc:50-128): AnchorPairsHIP, then one WarpPairStoreHIP per anchor that fits, by
//       ascending slot (where the reference iterates an unordered_map).  The DiffProp records stay in the device database
//       (device_records()) under the STORE's point ids with the new keyframe's slot as their tag.
// Every function returns false when the library refuses (dsh_last_error of the store's context says why); nothing is written to an
// object then.  EraseObservation is the host objects' own through EraseAccess of point_erase_hip.h: inside DefSLAM it is the reference's,
// with the move of the reference keyframe and the nObs <= 2 cascade the store applies.
// Templates over the reference's classes; the repository's CI instantiates them with integration/standin_localmap_types.h.
#pragma once
#include <cstdint>
#include <set>
#include <utility>
#include <vector>

#include "anchor_pairs_hip.h"
#include "point_erase_hip.h"

namespace defslam_hip {

template <class KeyFrameT, class MapPointT>
bool SetViewStoreHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, KeyFrameT* kf) {
  std::vector<float> px(2 * (size_t)kf->N + 2);
  for (int i = 0; i < kf->N; i++) { px[2 * i] = kf->mvKeysUn[i].pt.x; px[2 * i + 1] = kf->mvKeysUn[i].pt.y; }
  dsh_keyframe_view v;
  v.N = kf->N; v.kp_px = px.data();
  v.fx = kf->fx; v.fy = kf->fy; v.cx = kf->cx; v.cy = kf->cy;
  v.mnMinX = kf->mnMinX; v.mnMaxX = kf->mnMaxX; v.mnMinY = kf->mnMinY; v.mnMaxY = kf->mnMaxY;
  v.grid_cols = kf->gridCols(); v.grid_rows = kf->gridRows();
  v.warp_grid = dsh_bbs{kf->umin, kf->umax, kf->NCu, kf->vmin, kf->vmax, kf->NCv, kf->valdim};
  return dsh_keyframe_set_view(store.handle(), store.slot(kf), &v) == DSH_OK;
}

// the stores and the constants of the calls of one keyframe
struct WarpPairSetup {
  dsh_ctx* ctx = nullptr;
  dsh_kfdb* kfdb = nullptr;
  dsh_diffdb* ddb = nullptr;
  double lambda = 0.0;
  int min_pairs = 20, max_iters = 3, th_low = 50;     // SchwarpDatabase.cc:105, :213; DefORBmatcher.cc:193
  float radius = 2.f;
};

template <class MapPointT>
struct WarpPairOutcome {
  std::vector<double> x;                     // the fitted warp (the initialisation when not fitted)
  dsh_warp_pair_result r;                    // counts, init_ok, fitted, info, costs (its arrays point into the vectors below)
  std::vector<uint8_t> pair_state, query_state, query_added;
  std::vector<int32_t> query_match, query_point;
  std::vector<MapPointT*> stored;            // in list order
};

template <class KeyFrameT, class MapPointT>
bool WarpPairStoreHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, const WarpPairSetup& s, KeyFrameT* KF2, AnchorPairs<KeyFrameT, MapPointT>& lists, size_t a,
                      WarpPairOutcome<MapPointT>& out) {
  typedef EraseAccess<KeyFrameT, MapPointT> E;
  typename AnchorPairs<KeyFrameT, MapPointT>::Anchor A = lists.anchors[a];   // a copy: the Drop helpers edit the lists
  KeyFrameT* KF1 = A.refkf;
  const size_t P = A.vMatchedIndices.size(), Q = A.listMapPoints.size();
  std::vector<int32_t> i1(P + 1), i2(P + 1), q1(A.listMapPoints.begin(), A.listMapPoints.end());
  for (size_t n = 0; n < P; n++) { i1[n] = (int32_t)A.vMatchedIndices[n].first; i2[n] = (int32_t)A.vMatchedIndices[n].second; }
  q1.resize(Q + 1);
  out.x.assign(2 * (size_t)KF1->NCu * KF1->NCv, 0.0);
  out.pair_state.assign(P + 1, 0); out.query_state.assign(Q + 1, 0); out.query_added.assign(Q + 1, 0);
  out.query_match.assign(Q + 1, -1); out.query_point.assign(Q + 1, -1);
  out.stored.clear();
  dsh_warp_pair_input in;
  in.ctx = s.ctx; in.kfdb = s.kfdb; in.ddb = s.ddb;
  in.slot = store.slot(KF2); in.anchor = store.slot(KF1); in.tag = in.slot;
  in.lambda = s.lambda; in.min_pairs = s.min_pairs; in.max_iters = s.max_iters; in.radius = s.radius; in.th_low = s.th_low;
  in.n_pairs = (int32_t)P; in.pair_idx1 = i1.data(); in.pair_idx2 = i2.data();
  in.n_queries = (int32_t)Q; in.query_idx1 = q1.data();
  dsh_warp_pair_result& r = out.r;
  r = dsh_warp_pair_result();
  r.x = out.x.data(); r.pair_state = out.pair_state.data(); r.query_state = out.query_state.data(); r.query_match = out.query_match.data();
  r.query_point = out.query_point.data(); r.query_added = out.query_added.data();
  if (dsh_keyframe_warp_pair(store.handle(), &in, &r) != DSH_OK) return false;
  // ---- the write-back, in the reference's order.  DefORBmatcher.cc:167-175: the filtered matches leave KF2's table, their observation stays
  for (size_t n = 0; n < P; n++)
    if (out.pair_state[n] == DSH_WARP_FILTERED) KF2->EraseMapPointMatch((size_t)i2[n]);
  // :58-66: the new matches, in query order (a later query of the same key point takes the entry)
  for (size_t j = 0; j < Q; j++) {
    if (out.query_match[j] < 0 || out.query_point[j] < 0) continue;
    MapPointT* pMP = store.point(out.query_point[j]);
    pMP->AddObservation(KF2, (size_t)out.query_match[j]);
    KF2->addMapPoint(pMP, (size_t)out.query_match[j]);
    DropQueryHIP(lists, a, pMP);
  }
  // SchwarpDatabase.cc:268-346 over the kept list: the kept pairs, then the matched queries
  std::vector<std::pair<std::pair<size_t, size_t>, uint8_t>> kept;
  for (size_t n = 0; n < P; n++)
    if (out.pair_state[n] != DSH_WARP_FILTERED) kept.push_back(std::make_pair(A.vMatchedIndices[n], out.pair_state[n]));
  for (size_t j = 0; j < Q; j++)
    if (out.query_match[j] >= 0) kept.push_back(std::make_pair(std::make_pair((size_t)q1[j], (size_t)out.query_match[j]), out.query_state[j]));
  for (size_t n = 0; n < kept.size(); n++) {
    const size_t idx1 = kept[n].first.first, idx2 = kept[n].first.second;
    if (kept[n].second == DSH_WARP_DROPPED) {
      MapPointT* mapPoint2 = KF2->GetMapPoint(idx2);
      E::erase_observation(mapPoint2, KF2);                              // :290
      KF2->EraseMapPointMatch(idx2);                                     // :291
      DropMatchHIP(lists, a, idx2, mapPoint2);
    } else if (kept[n].second == DSH_WARP_STORED) {
      out.stored.push_back(KF1->GetMapPoint(idx1));                      // :345 newInformation_
    }
  }
  return true;
}

// Base = defSLAM::WarpDatabase (WarpDatabase.h:39-72)
template <class Base, class KeyFrameT, class MapPointT>
class SchwarpDatabaseStoreHIP : public Base {
 public:
  SchwarpDatabaseStoreHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, const WarpPairSetup& setup) : store_(store), setup_(setup) {}

  // SchwarpDatabase::add (SchwarpDatabase.cc:50-128)
  void add(KeyFrameT* mpCurrentKeyFrame) override {
    ok_ = true;
    outcomes.clear();
    if (mpkeyframes.count(mpCurrentKeyFrame)) return;
    if (mpkeyframes.empty()) { mpkeyframes.insert(mpCurrentKeyFrame); return; }
    AnchorPairs<KeyFrameT, MapPointT> lists;
    if (!AnchorPairsHIP(store_, mpCurrentKeyFrame, lists, setup_.min_pairs)) { ok_ = false; return; }
    for (size_t a = 0; a < lists.anchors.size(); a++) {
      if (!lists.anchors[a].fits) continue;                              // :105-106
      outcomes.push_back(std::make_pair(lists.anchors[a].refkf, WarpPairOutcome<MapPointT>()));
      WarpPairOutcome<MapPointT>& o = outcomes.back().second;
      if (!WarpPairStoreHIP(store_, setup_, mpCurrentKeyFrame, lists, a, o)) { ok_ = false; return; }
      if (!o.r.fitted) continue;                                         // :113-114
      for (MapPointT* p : o.stored) this->newInformation_[p] = true;
      mpCurrentKeyFrame->KeyframesRelated++;                             // :116
    }
    mpkeyframes.insert(mpCurrentKeyFrame);
  }
  void erase(KeyFrameT* kf) override { mpkeyframes.erase(kf); }
  void clear() override {
    mpkeyframes.clear();
    if (setup_.ddb) dsh_diffdb_clear(setup_.ddb);
  }
  bool ok() const { return ok_; }                                        // false: the library refused inside the last add
  dsh_diffdb* device_records() const { return setup_.ddb; }
  std::vector<std::pair<KeyFrameT*, WarpPairOutcome<MapPointT>>> outcomes;   // of the last add, per anchor that was fitted

 private:
  MapPointStoreHIP<KeyFrameT, MapPointT>& store_;
  WarpPairSetup setup_;
  std::set<KeyFrameT*> mpkeyframes;
  bool ok_ = true;
};

}  // namespace defslam_hip
