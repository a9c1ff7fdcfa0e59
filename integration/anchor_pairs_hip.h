// Host integration shim of the mapping thread's entry into the Schwarp chain on the resident map point store (include/defslam_hip.h:
// dsh_keyframe_anchors and the two fields it reads), over MapPointStoreHIP of local_map_hip.h:
//
//   AddObservationsIndexedHIP(store, pts, kfs, idx)    MapPoint::AddObservation(pKF, idx) with the key point index (MapPoint.cc:86-97)
//   SetReferenceKeyFramesHIP(store, pts)               the points' GetReferenceKeyFrame() (a keyframe of the store, or null)
//   AnchorPairsHIP(store, KF2, out[, min_pairs])
//       what SchwarpDatabase::add (Modules/Mapping/SchwarpDatabase.cc:61-106) reads of the map for the new keyframe KF2, and the query
//       list of DefORBmatcher::searchBySchwarp (Modules/Matching/DefORBmatcher.cc:200-211), in one call on the device: per anchor
//       keyframe (by ascending slot, where the reference iterates an unordered_map) the vMatchedIndices and the listMapPoints that the
//       functions of schwarp_database_hip.h take, the flag of the pairs whose record the fit stores (:296-298), and has[] of KF2's
//       entries for dsh_search_by_schwarp.  An anchor with fewer than min_pairs pairs is listed with fits == false and empty lists
//       (:105-106).  Key point coordinates stay with the caller, who indexes mpKeypointNorm with the indices.  Returns false when the
//       library refuses (dsh_last_error of the store's context says why).
//   DropMatchHIP(out, a_from, idx2)
//       THE ONE SEQUENTIAL EFFECT between the anchors of a keyframe.  The lists are a snapshot taken before the first fit.  A fit that
//       drops a match erases (point, KF2) and empties KF2's entry idx2 (SchwarpDatabase.cc:288-292; DropMatchesStoreHIP of
//       point_erase_hip.h does both on the objects and in the store, for all drops of a fit in one call), so for the anchors behind
//       a_from the point is no longer in both keyframes: its pair leaves their
//       vMatchedIndices, and where their table holds the point it becomes a query of their search (DefORBmatcher.cc:208).  This helper
//       applies exactly that to the snapshot (an anchor that falls below min_pairs stops fitting; n_pairs of an anchor that did not fit
//       in the snapshot stays the snapshot's: its pairs were not listed).  Matches that findbyWarp ADDS land on entries of KF2 that were empty in the snapshot and
//       on points that were queries, i.e. not in KF2: they never enter a later anchor's vMatchedIndices snapshot; the caller drops the
//       matched query from the later lists with DropQueryHIP.
// Templates over the reference's classes; the repository's CI instantiates them with integration/standin_localmap_types.h.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "local_map_hip.h"

namespace defslam_hip {

template <class KeyFrameT, class MapPointT>
bool AddObservationsIndexedHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, const std::vector<MapPointT*>& pts, const std::vector<KeyFrameT*>& kfs,
                               const std::vector<int>& idx) {
  std::vector<int32_t> p(pts.size()), k(pts.size()), i(pts.size());
  for (size_t n = 0; n < pts.size(); n++) {
    p[n] = store.id(pts[n]);
    k[n] = store.slot(kfs[n]);
    i[n] = idx[n];
  }
  return dsh_point_store_add_observations_indexed(store.handle(), (int)p.size(), p.data(), k.data(), i.data()) == DSH_OK;
}

template <class KeyFrameT, class MapPointT>
bool SetReferenceKeyFramesHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, const std::vector<MapPointT*>& pts) {
  std::vector<int32_t> p(pts.size()), k(pts.size());
  for (size_t n = 0; n < pts.size(); n++) {
    p[n] = store.id(pts[n]);
    KeyFrameT* ref = pts[n]->GetReferenceKeyFrame();
    k[n] = ref ? store.slot(ref) : -1;
  }
  return dsh_point_store_set_reference_keyframes(store.handle(), (int)p.size(), p.data(), k.data()) == DSH_OK;
}

template <class KeyFrameT, class MapPointT>
struct AnchorPairs {
  struct Anchor {
    KeyFrameT* refkf = nullptr;                              // kv.first (:86)
    int count = 0;                                           // kv.second
    int n_pairs = 0;                                         // vMatchedIndices.size() at :105
    bool fits = false;                                       // n_pairs >= min_pairs
    std::vector<std::pair<size_t, size_t>> vMatchedIndices;  // (idx1 in refkf, idx2 in KF2), :100-102
    std::vector<MapPointT*> points;                          // the shared point of each pair
    std::vector<uint8_t> own;                                // 1: refkf is the point's reference keyframe, its record is stored (:296-298)
    std::vector<int> listMapPoints;                          // DefORBmatcher.cc:198-211
  };
  std::vector<Anchor> anchors;
  std::vector<uint8_t> has;                                  // per entry of KF2: it holds a point
  int n_no_ref = 0;                                          // entries whose point has no reference keyframe in the store
  int min_pairs = 20;                                        // the threshold of :105 the lists were made with
};

template <class KeyFrameT, class MapPointT>
bool AnchorPairsHIP(MapPointStoreHIP<KeyFrameT, MapPointT>& store, KeyFrameT* KF2, AnchorPairs<KeyFrameT, MapPointT>& out, int min_pairs = 20) {
  const int32_t slot = store.slot(KF2);
  const size_t N = KF2->GetMapPointMatches().size();
  out = AnchorPairs<KeyFrameT, MapPointT>();
  out.has.assign(N > 0 ? N : 1, 0);
  dsh_anchor_lists l = dsh_anchor_lists();
  std::vector<int32_t> as, ac, ap, pp, qp, i1, i2, pt, q1, qpt;
  std::vector<uint8_t> own;
  l.anchor_capacity = 64;
  l.pair_capacity = (int32_t)(4 * N + 1);
  l.query_capacity = (int32_t)(16 * N + 1);
  for (int attempt = 0; attempt < 2; attempt++) {            // the second call has the sizes the first one reported
    as.resize(l.anchor_capacity); ac.resize(l.anchor_capacity); ap.resize(l.anchor_capacity);
    pp.resize(l.anchor_capacity + 1); qp.resize(l.anchor_capacity + 1);
    i1.resize(l.pair_capacity); i2.resize(l.pair_capacity); pt.resize(l.pair_capacity); own.resize(l.pair_capacity);
    q1.resize(l.query_capacity); qpt.resize(l.query_capacity);
    l.anchor_slot = as.data(); l.anchor_count = ac.data(); l.anchor_pairs = ap.data();
    l.pair_ptr = pp.data(); l.pair_idx1 = i1.data(); l.pair_idx2 = i2.data(); l.pair_point = pt.data(); l.pair_own = own.data();
    l.query_ptr = qp.data(); l.query_idx1 = q1.data(); l.query_point = qpt.data();
    l.has = out.has.data();
    const int rc = dsh_keyframe_anchors(store.handle(), slot, min_pairs, &l);
    if (rc == DSH_OK) break;
    const bool small = l.n_anchors > l.anchor_capacity || l.n_pairs > l.pair_capacity || l.n_queries > l.query_capacity;
    if (rc != DSH_ERR_ARG || !small || attempt == 1) return false;
    l.anchor_capacity = std::max(l.anchor_capacity, l.n_anchors);
    l.pair_capacity = std::max(l.pair_capacity, l.n_pairs);
    l.query_capacity = std::max(l.query_capacity, l.n_queries);
  }
  out.has.resize(N);
  out.min_pairs = min_pairs;
  out.n_no_ref = l.n_no_ref;
  out.anchors.resize(l.n_anchors);
  for (int a = 0; a < l.n_anchors; a++) {
    typename AnchorPairs<KeyFrameT, MapPointT>::Anchor& A = out.anchors[a];
    A.refkf = store.keyframe(as[a]);
    A.count = ac[a];
    A.n_pairs = ap[a];
    A.fits = ap[a] >= min_pairs;
    for (int n = pp[a]; n < pp[a + 1]; n++) {
      A.vMatchedIndices.push_back(std::make_pair((size_t)i1[n], (size_t)i2[n]));
      A.points.push_back(store.point(pt[n]));
      A.own.push_back(own[n]);
    }
    A.listMapPoints.assign(q1.begin() + qp[a], q1.begin() + qp[a + 1]);
  }
  return true;
}

// the fit of anchor a_from dropped its match at key point idx2 of KF2, whose point was `dropped` (read before the entry was emptied)
template <class KeyFrameT, class MapPointT>
void DropMatchHIP(AnchorPairs<KeyFrameT, MapPointT>& out, size_t a_from, size_t idx2, MapPointT* dropped) {
  if (idx2 < out.has.size()) out.has[idx2] = 0;              // KF2->EraseMapPointMatch(idx2)
  for (size_t a = a_from + 1; a < out.anchors.size(); a++) {
    typename AnchorPairs<KeyFrameT, MapPointT>::Anchor& A = out.anchors[a];
    if (!A.fits) continue;
    for (size_t n = A.vMatchedIndices.size(); n-- > 0;)
      if (A.points[n] == dropped) {                          // the point is in KF2 no more (:97)
        A.vMatchedIndices.erase(A.vMatchedIndices.begin() + n);
        A.points.erase(A.points.begin() + n);
        A.own.erase(A.own.begin() + n);
        A.n_pairs--;
      }
    if (A.n_pairs < out.min_pairs) {                         // :105-106 when the anchor is reached: no fit, no search
      A.fits = false;
      A.vMatchedIndices.clear(); A.points.clear(); A.own.clear(); A.listMapPoints.clear();
      continue;
    }
    if (dropped->isBad()) continue;
    const std::vector<MapPointT*> table = A.refkf->GetMapPointMatches();   // and where the anchor holds it, it is a query now
    for (size_t j = 0; j < table.size(); j++)
      if (table[j] == dropped && !std::binary_search(A.listMapPoints.begin(), A.listMapPoints.end(), (int)j))
        A.listMapPoints.insert(std::lower_bound(A.listMapPoints.begin(), A.listMapPoints.end(), (int)j), (int)j);
  }
}

// findbyWarp matched the query at entry idx1 of anchor a_from's keyframe, whose point is `matched`, into KF2: later anchors search it no more
template <class KeyFrameT, class MapPointT>
void DropQueryHIP(AnchorPairs<KeyFrameT, MapPointT>& out, size_t a_from, MapPointT* matched) {
  for (size_t a = a_from + 1; a < out.anchors.size(); a++) {
    typename AnchorPairs<KeyFrameT, MapPointT>::Anchor& A = out.anchors[a];
    const std::vector<MapPointT*> table = A.refkf->GetMapPointMatches();
    for (size_t n = A.listMapPoints.size(); n-- > 0;)
      if (table[A.listMapPoints[n]] == matched) A.listMapPoints.erase(A.listMapPoints.begin() + n);
  }
}

}  // namespace defslam_hip
