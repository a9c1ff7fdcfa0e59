// CI driver of integration/anchor_pairs_hip.h: one new keyframe of a map read from a text file, both ways over the same stand-in objects:
//   the store way  MapPointStoreHIP with indexed observations and reference keyframes + AnchorPairsHIP: one call, nothing per map
//                  point travels; then DropMatchHIP on the snapshot for one dropped match
//   the host way   the loops of SchwarpDatabase::add (SchwarpDatabase.cc:61-106) and DefORBmatcher::searchBySchwarp
//                  (DefORBmatcher.cc:200-211) over the pointer graph, anchors by ascending slot; then the drop as calculateSchwarps does
//                  it (:288-292) on the objects and the same loops again for the anchors behind it
// Every list is dumped per route; tests/test_anchor_pairs_shim_gpu.py compares the routes with each other and with the restatement.
//   map file: P K / P lines "bad ref" / K lines "N t0 .. tN-1" / L / L lines "point kf idx" / E / E lines "point kf" (erased again) /
//             "slot min_pairs drop_anchor drop_pair" (the drop_pair-th pair of the drop_anchor-th anchor is dropped; -1 -1: none)
//   usage: anchor_pairs_shim_test <map.txt> <output.txt> [device [reps]]
// With reps > 0 both routes are also timed, reps calls each after one warm-up call, and a line "time <host_us> <store_us>" (the medians)
// ends the output: tools/bench_anchor_pairs.py reads it.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <string>

#include "anchor_pairs_hip.h"
#include "standin_localmap_types.h"

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
    std::fprintf(f, "%s anchor %d %d %d %d |", route, slots.at(A.refkf), A.count, A.n_pairs, A.fits ? 1 : 0);
    for (size_t n = 0; n < A.vMatchedIndices.size(); n++)
      std::fprintf(f, " %zu:%zu:%d", A.vMatchedIndices[n].first, A.vMatchedIndices[n].second, (int)A.own[n]);
    std::fprintf(f, " |");
    for (int j : A.listMapPoints) std::fprintf(f, " %d", j);
    std::fprintf(f, "\n");
  }
  std::fprintf(f, "%s has", route);
  for (uint8_t h : l.has) std::fprintf(f, " %d", (int)h);
  std::fprintf(f, "\n%s no_ref %d\n", route, l.n_no_ref);
}

int fail(dsh_ctx* ctx, const char* what) {
  std::fprintf(stderr, "%s: %s\n", what, ctx ? dsh_last_error(ctx) : "");
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return std::fprintf(stderr, "usage: %s <map.txt> <output.txt> [device]\n", argv[0]), 2;
  std::ifstream in(argv[1]);
  int P = 0, K = 0;
  in >> P >> K;
  if (!in || P < 0 || K < 1) return std::fprintf(stderr, "cannot read %s\n", argv[1]), 2;
  std::vector<LmMapPoint> mps(P);
  std::vector<LmKeyFrame> kfs(K);
  std::vector<int> ref(P);
  for (int p = 0; p < P; p++) {
    int bad;
    in >> bad >> ref[p];
    mps[p].bad = bad != 0;
    mps[p].mpRefKF = ref[p] >= 0 ? &kfs[ref[p]] : nullptr;
  }
  std::map<LmKeyFrame*, int> slots;
  for (int k = 0; k < K; k++) {
    in >> kfs[k].N;
    kfs[k].mvpMapPoints.assign(kfs[k].N, nullptr);
    for (int j = 0; j < kfs[k].N; j++) {
      int p;
      in >> p;
      if (p >= 0) kfs[k].mvpMapPoints[j] = &mps[p];
    }
    slots[&kfs[k]] = k;
  }
  int L = 0, E = 0;
  in >> L;
  std::vector<LmMapPoint*> op(L);
  std::vector<LmKeyFrame*> ok(L);
  std::vector<int> oi(L);
  for (int n = 0; n < L; n++) {
    int p, k;
    in >> p >> k >> oi[n];
    op[n] = &mps[p];
    ok[n] = &kfs[k];
    mps[p].AddObservation(ok[n], (size_t)oi[n]);
  }
  in >> E;
  std::vector<LmMapPoint*> ep(E);
  std::vector<LmKeyFrame*> ek(E);
  for (int n = 0; n < E; n++) {
    int p, k;
    in >> p >> k;
    ep[n] = &mps[p];
    ek[n] = &kfs[k];
    mps[p].EraseObservation(ek[n]);
  }
  int slot = 0, min_pairs = 20, drop_anchor = -1, drop_pair = -1;
  in >> slot >> min_pairs >> drop_anchor >> drop_pair;
  if (!in || slot < 0 || slot >= K) return std::fprintf(stderr, "malformed %s\n", argv[1]), 2;
  LmKeyFrame* KF2 = &kfs[slot];

  dsh_ctx* ctx = nullptr;
  if (dsh_create(&ctx, argc > 3 ? std::atoi(argv[3]) : 0) != DSH_OK) return fail(ctx, "dsh_create");
  std::FILE* f = std::fopen(argv[2], "w");
  if (!f) return std::fprintf(stderr, "cannot write %s\n", argv[2]), 2;
  int rc = 0;
  {
    // the store way: the map goes up once, as the mapping thread would have kept it current
    Store store(ctx, 16, 2, 16);
    std::vector<LmMapPoint*> all(P);
    for (int p = 0; p < P; p++) all[p] = &mps[p];
    if (!store.ok() || !store.AddMapPoints<LmFrame>(all)) return fail(ctx, "AddMapPoints");
    for (int k = 0; k < K; k++)
      if (!store.AddKeyFrame(&kfs[k])) return fail(ctx, "AddKeyFrame");
    if (!defslam_hip::AddObservationsIndexedHIP(store, op, ok, oi)) return fail(ctx, "AddObservationsIndexedHIP");
    if (E > 0 && !store.EraseObservations(ep, ek)) return fail(ctx, "EraseObservations");
    if (!defslam_hip::SetReferenceKeyFramesHIP(store, all)) return fail(ctx, "SetReferenceKeyFramesHIP");
    Lists st, host;
    if (!defslam_hip::AnchorPairsHIP(store, KF2, st, min_pairs)) return fail(ctx, "AnchorPairsHIP");
    const std::vector<LmMapPoint*> vpMapPointMatches = KF2->GetMapPointMatches();   // the copy of :62
    host_anchor_pairs(KF2, vpMapPointMatches, slots, min_pairs, -1, host);
    dump(f, "store", st, slots, 0);
    dump(f, "host", host, slots, 0);
    const int reps = argc > 4 ? std::atoi(argv[4]) : 0;
    if (reps > 0) {
      std::vector<double> th, ts;
      for (int r = 0; r < reps; r++) {
        Lists tmp;
        const auto t0 = std::chrono::steady_clock::now();
        host_anchor_pairs(KF2, KF2->GetMapPointMatches(), slots, min_pairs, -1, tmp);
        const auto t1 = std::chrono::steady_clock::now();
        if (!defslam_hip::AnchorPairsHIP(store, KF2, tmp, min_pairs)) return fail(ctx, "AnchorPairsHIP");
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
      if (!store.EraseObservations(dp, dk) || !store.SetKeyFramePoint(KF2, (int)idx2, nullptr)) return fail(ctx, "the drop on the store");
      Lists again;
      if (!defslam_hip::AnchorPairsHIP(store, KF2, again, min_pairs)) return fail(ctx, "AnchorPairsHIP after the drop");
      dump(f, "store_again", again, slots, 0);
    }
  }
  std::fclose(f);
  dsh_destroy(ctx);
  return rc;
}
