// CI driver of integration/anchor_pairs_hip.h: one new keyframe of a map read from a text file, both ways over the same stand-in objects:
//   the store way  MapPointStoreHIP with indexed observations and reference keyframes + AnchorPairsHIP: one call, nothing per map
//                  point travels; then DropMatchHIP on the snapshot for one dropped match
//   the host way   the loops of SchwarpDatabase::add (SchwarpDatabase.cc:61-106) and DefORBmatcher::searchBySchwarp
//                  (DefORBmatcher.cc:200-211) over the pointer graph, anchors by ascending slot; then the drop as calculateSchwarps does
//                  it (:288-292) on the objects and the same loops again for the anchors behind it
// Every list is dumped per route, in lines "route lists anchor|has|no_ref .."; tests/test_anchor_pairs_shim_gpu.py compares the routes with each other and with the restatement.
//   scene file: standin_store_scene.h, then the tail "slot min_pairs drop_anchor drop_pair" (the drop_pair-th pair of the drop_anchor-th
//               anchor is dropped; -1 -1: none)
//   usage and exit codes: shim_driver.h; the driver's own argument behind the device is reps
// With reps > 0 both routes are also timed, reps calls each after one warm-up call, and a line "time <host_us> <store_us>" (the medians)
// ends the output: tools/bench_anchor_pairs.py reads it.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <fstream>
#include <map>

#include "anchor_pairs_hip.h"
#include "shim_driver.h"
#include "standin_store_scene.h"

using namespace standin;
typedef defslam_hip::MapPointStoreHIP<LmKeyFrame, LmMapPoint> Store;
typedef defslam_hip::AnchorPairs<LmKeyFrame, LmMapPoint> Lists;

namespace {

// SchwarpDatabase::add up to the fit, and the search's query list, for the anchors behind `after` (-1: all); vpMapPointMatches is the
// copy the reference takes at :62, slots stands for the order of the unordered_map
void host_anchor_pairs(LmKeyFrame* KF2, const std::vector<LmMapPoint*>& vpMapPointMatches, const std::map<LmKeyFrame*, int>& slots, int min_pairs,
                       int after, Lists& out) {
  std::map<int, std::pair<LmKeyFrame*, int>> countKFMatches;   // by slot
  out.n_no_ref = 0;
  for (size_t i = 0; i < vpMapPointMatches.size(); i++) {
    LmMapPoint* mapPoint = vpMapPointMatches[i];
    if (!mapPoint) continue;
    if (mapPoint->isBad()) continue;
    LmKeyFrame* refkf = mapPoint->GetReferenceKeyFrame();
    if (!refkf) { out.n_no_ref++; continue; }
    std::pair<LmKeyFrame*, int>& c = countKFMatches[slots.at(refkf)];
    c.first = refkf;
    c.second++;
  }
  int a = 0;
  for (const auto& kv : countKFMatches) {
    if (a++ <= after) continue;
    Lists::Anchor A;
    A.refkf = kv.second.first;
    A.count = kv.second.second;
    for (size_t i = 0; i < vpMapPointMatches.size(); i++) {
      LmMapPoint* mapPoint = vpMapPointMatches[i];
      if (!mapPoint) continue;
      if (mapPoint->isBad()) continue;
      if (mapPoint->IsInKeyFrame(KF2) && mapPoint->IsInKeyFrame(A.refkf)) {
        A.vMatchedIndices.push_back(std::make_pair((size_t)mapPoint->GetIndexInKeyFrame(A.refkf), (size_t)mapPoint->GetIndexInKeyFrame(KF2)));
        A.points.push_back(mapPoint);
        A.own.push_back(mapPoint->GetReferenceKeyFrame() == A.refkf ? 1 : 0);
      }
    }
    A.n_pairs = (int)A.vMatchedIndices.size();
    A.fits = A.n_pairs >= min_pairs;
    if (!A.fits) {
      A.vMatchedIndices.clear(); A.points.clear(); A.own.clear();
    } else {
      for (size_t i = 0; i < A.refkf->mvpMapPoints.size(); i++) {
        LmMapPoint* pMP = A.refkf->GetMapPoint(i);
        if (!pMP) continue;
        if (pMP->isBad()) continue;
        if (pMP->IsInKeyFrame(KF2)) continue;
        A.listMapPoints.push_back((int)i);
      }
    }
    out.anchors.push_back(A);
  }
  out.has.assign(KF2->mvpMapPoints.size(), 0);
  for (size_t i = 0; i < KF2->mvpMapPoints.size(); i++) out.has[i] = KF2->mvpMapPoints[i] ? 1 : 0;
}

void dump(std::FILE* f, const char* route, const Lists& l, const std::map<LmKeyFrame*, int>& slots, size_t first) {
  for (size_t a = first; a < l.anchors.size(); a++) {
    const Lists::Anchor& A = l.anchors[a];
    std::fprintf(f, "%s lists anchor %d %d %d %d |", route, slots.at(A.refkf), A.count, A.n_pairs, A.fits ? 1 : 0);
    for (size_t n = 0; n < A.vMatchedIndices.size(); n++)
      std::fprintf(f, " %zu:%zu:%d", A.vMatchedIndices[n].first, A.vMatchedIndices[n].second, (int)A.own[n]);
    std::fprintf(f, " |");
    for (int j : A.listMapPoints) std::fprintf(f, " %d", j);
    std::fprintf(f, "\n");
  }
  std::fprintf(f, "%s lists has", route);
  for (uint8_t h : l.has) std::fprintf(f, " %d", (int)h);
  std::fprintf(f, "\n%s lists no_ref %d\n", route, l.n_no_ref);
}

}  // namespace

static int drive(const DriverArgs& arg) {
  dsh_ctx* ctx = arg.ctx;
  std::FILE* f = arg.out;
  StoreScene sc;
  std::ifstream in(arg.in[0]);
  int slot = 0, min_pairs = 20, drop_anchor = -1, drop_pair = -1;
  if (!sc.read(in) || !(in >> slot >> min_pairs >> drop_anchor >> drop_pair) || slot < 0 || slot >= sc.K) return driver_bad_input(arg.in[0]);
  std::map<LmKeyFrame*, int> slots;
  for (int k = 0; k < sc.K; k++) slots[&sc.kfs[k]] = k;
  LmKeyFrame* KF2 = &sc.kfs[slot];

  // the store way: the map goes up once, as the mapping thread would have kept it current
  Store store(ctx, 16, 2, 16);
  if (!sc.fill(store)) return driver_fail(ctx, "filling the store");
  Lists st, host;
  if (!defslam_hip::AnchorPairsHIP(store, KF2, st, min_pairs)) return driver_fail(ctx, "AnchorPairsHIP");
  const std::vector<LmMapPoint*> vpMapPointMatches = KF2->GetMapPointMatches();   // the copy of :62
  host_anchor_pairs(KF2, vpMapPointMatches, slots, min_pairs, -1, host);
  dump(f, "store", st, slots, 0);
  dump(f, "host", host, slots, 0);
  const int reps = arg.n_extra > 0 ? std::atoi(arg.extra[0]) : 0;
  if (reps > 0) {
    std::vector<double> th, ts;
    for (int r = 0; r < reps; r++) {
      Lists tmp;
      const auto t0 = std::chrono::steady_clock::now();
      host_anchor_pairs(KF2, KF2->GetMapPointMatches(), slots, min_pairs, -1, tmp);
      const auto t1 = std::chrono::steady_clock::now();
      if (!defslam_hip::AnchorPairsHIP(store, KF2, tmp, min_pairs)) return driver_fail(ctx, "AnchorPairsHIP");
      const auto t2 = std::chrono::steady_clock::now();
      th.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
      ts.push_back(std::chrono::duration<double, std::micro>(t2 - t1).count());
    }
    std::sort(th.begin(), th.end());
    std::sort(ts.begin(), ts.end());
    std::fprintf(f, "time %.1f %.1f\n", th[reps / 2], ts[reps / 2]);
  }
  if (drop_anchor >= 0 && drop_anchor < (int)host.anchors.size() && drop_pair >= 0 && drop_pair < (int)host.anchors[drop_anchor].vMatchedIndices.size()) {
    const size_t idx2 = host.anchors[drop_anchor].vMatchedIndices[drop_pair].second;
    LmMapPoint* mapPoint2 = KF2->GetMapPoint(idx2);
    mapPoint2->EraseObservation(KF2);                      // SchwarpDatabase.cc:290-291
    KF2->EraseMapPointMatch(idx2);
    defslam_hip::DropMatchHIP(st, (size_t)drop_anchor, idx2, mapPoint2);
    Lists later;
    host_anchor_pairs(KF2, vpMapPointMatches, slots, min_pairs, drop_anchor, later);
    dump(f, "store_drop", st, slots, (size_t)drop_anchor + 1);
    dump(f, "host_drop", later, slots, 0);
    // and the store follows the two mutations: a fresh call sees what the host sees
    std::vector<LmMapPoint*> dp(1, mapPoint2);
    std::vector<LmKeyFrame*> dk(1, KF2);
    if (!store.EraseObservations(dp, dk) || !store.SetKeyFramePoint(KF2, (int)idx2, nullptr)) return driver_fail(ctx, "the drop on the store");
    Lists again;
    if (!defslam_hip::AnchorPairsHIP(store, KF2, again, min_pairs)) return driver_fail(ctx, "AnchorPairsHIP after the drop");
    dump(f, "store_again", again, slots, 0);
  }
  return 0;
}

int main(int argc, char** argv) { return run_driver(argc, argv, 1, drive); }
