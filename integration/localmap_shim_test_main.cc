// CI driver of integration/local_map_hip.h: a map (points, keyframes with tables and a spanning tree, observations) and a current frame
// from a text file; the map goes into a MapPointStoreHIP, then DefTracking::TrackLocalMap's first two steps (DefTracking.cc:237-240) run
// through UpdateLocalMapHIP and SearchLocalPointsStoreHIP, and what the reference's calls change is dumped.
//   usage: localmap_shim_test <input.txt> <output.txt> [device] [timing.json reps]
// With a timing file the frame is then repeated `reps` times both ways and the medians are written: the device path above, and the way
// the frame was done before the store existed -- UpdateLocalKeyFrames + UpdateLocalPoints on the host over the same objects
// (std::map / std::set, below) followed by SearchLocalPointsHIP, which re-packs every local point.  The host lists are also compared
// with the device's (the stand-in objects live in arrays, so pointer order is index order).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <fstream>
#include <map>
#include <set>
#include <string>

#include "local_map_hip.h"
#include "standin_localmap_types.h"

using namespace standin;

namespace {

// Tracking::UpdateLocalKeyFrames (Tracking.cc:1510-1629) and DefTracking::UpdateLocalPoints (DefTracking.cc:426-454) as the host does
// them: ordered containers keyed by pointer, one tree insertion per observation of every point the frame holds.
void host_update_local_map(LmFrame& F, const std::vector<LmKeyFrame*>& all_kfs, std::vector<LmKeyFrame*>& local_kfs, std::vector<LmMapPoint*>& local_pts,
                           LmKeyFrame*& ref_kf) {
  std::map<LmKeyFrame*, int> counter;
  for (LmMapPoint*& mp : F.mvpMapPoints) {
    if (!mp) continue;
    if (mp->isBad()) { mp = nullptr; continue; }
    const std::map<LmKeyFrame*, size_t> obs = mp->GetObservations();
    for (const auto& o : obs) counter[o.first]++;
  }
  if (!counter.empty()) {
    local_kfs.clear();
    local_kfs.reserve(3 * counter.size());
    int top = 0;
    LmKeyFrame* winner = nullptr;
    for (const auto& c : counter) {
      if (c.first->isBad()) continue;
      if (c.second > top) { top = c.second; winner = c.first; }
      local_kfs.push_back(c.first);
      c.first->mnTrackReferenceForFrame = F.mnId;
    }
    auto take = [&](LmKeyFrame* k) { local_kfs.push_back(k); k->mnTrackReferenceForFrame = F.mnId; };
    const size_t voted = local_kfs.size();
    for (size_t i = 0; i < voted && local_kfs.size() <= 80; i++) {
      LmKeyFrame* kf = local_kfs[i];
      for (LmKeyFrame* n : all_kfs)
        if (!n->isBad() && n->mnTrackReferenceForFrame != F.mnId) { take(n); break; }
      const std::set<LmKeyFrame*> children = kf->GetChilds();
      for (LmKeyFrame* ch : children)
        if (!ch->isBad() && ch->mnTrackReferenceForFrame != F.mnId) { take(ch); break; }
      LmKeyFrame* parent = kf->GetParent();
      if (parent && parent->mnTrackReferenceForFrame != F.mnId) { take(parent); break; }
    }
    if (winner) { ref_kf = winner; F.mpReferenceKF = winner; }
  }
  std::set<LmMapPoint*> all;
  for (LmKeyFrame* kf : local_kfs) {
    const std::vector<LmMapPoint*> mps = kf->GetMapPointMatches();
    for (LmMapPoint* mp : mps) {
      if (!mp || mp->mnTrackReferenceForFrame == F.mnId || mp->isBad()) continue;
      mp->mnTrackReferenceForFrame = F.mnId;
      all.insert(mp);
    }
  }
  local_pts.assign(all.begin(), all.end());
}

double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v.empty() ? 0.0 : v[v.size() / 2];
}

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::ifstream in(argv[1]);
  int levels, P, K, R, N;
  float logsf;
  in >> levels >> logsf;
  std::vector<float> sf(levels);
  for (float& s : sf) in >> s;
  // map points: x y z nx ny nz maxd bad desc[32]
  in >> P;
  std::vector<LmMapPoint> mps(P);
  for (LmMapPoint& m : mps) {
    int bad;
    in >> m.pos[0] >> m.pos[1] >> m.pos[2] >> m.normal[0] >> m.normal[1] >> m.normal[2] >> m.mfMaxDistance >> bad;
    m.bad = bad != 0;
    for (auto& b : m.desc) { int v; in >> v; b = (uint8_t)v; }
  }
  // keyframes: parent bad n, then n table entries (point id or -1)
  in >> K;
  std::vector<LmKeyFrame> kfs(K);
  for (int k = 0; k < K; k++) {
    int parent, bad, n;
    in >> parent >> bad >> n;
    kfs[k].mnId = k;
    kfs[k].bad = bad != 0;
    kfs[k].mpParent = parent >= 0 ? &kfs[parent] : nullptr;
    if (parent >= 0) kfs[parent].mspChildrens.insert(&kfs[k]);
    kfs[k].mvpMapPoints.assign(n, nullptr);
    for (auto& p : kfs[k].mvpMapPoints) { int id; in >> id; p = id >= 0 ? &mps[id] : nullptr; }
  }
  // observations: point keyframe
  in >> R;
  std::vector<LmMapPoint*> obs_p(R);
  std::vector<LmKeyFrame*> obs_k(R);
  for (int r = 0; r < R; r++) {
    int p, k;
    in >> p >> k;
    obs_p[r] = &mps[p];
    obs_k[r] = &kfs[k];
    mps[p].mObservations[&kfs[k]] = 0;
  }
  // the current frame: camera, pose, centre, key points (x y octave point-id desc[32])
  LmFrame cur;
  in >> cur.fx >> cur.fy >> cur.cx >> cur.cy >> cur.mnMinX >> cur.mnMaxX >> cur.mnMinY >> cur.mnMaxY;
  for (float& t : cur.mTcw) in >> t;
  for (float& o : cur.mOw) in >> o;
  cur.mnScaleLevels = levels;
  cur.mfLogScaleFactor = logsf;
  cur.mvScaleFactors = sf;
  cur.mnId = 7;
  in >> N;
  cur.N = N;
  cur.mvKeysUn.resize(N);
  cur.mDescriptors.resize(32 * (size_t)N);
  cur.mvpMapPoints.assign(N, nullptr);
  cur.mvbOutlier.assign(N, false);
  for (int j = 0; j < N; j++) {
    int id;
    in >> cur.mvKeysUn[j].pt.x >> cur.mvKeysUn[j].pt.y >> cur.mvKeysUn[j].octave >> id;
    if (id >= 0) cur.mvpMapPoints[j] = &mps[id];
    for (int k = 0; k < 32; k++) { int v; in >> v; cur.mDescriptors[32 * (size_t)j + k] = (uint8_t)v; }
  }
  cur.mvKeys = cur.mvKeysUn;
  if (!in) { std::fprintf(stderr, "bad input\n"); return 2; }
  const std::vector<LmMapPoint*> frame0 = cur.mvpMapPoints;

  dsh_ctx* ctx = nullptr;
  if (dsh_create(&ctx, argc > 3 ? std::stoi(argv[3]) : 0) != DSH_OK) { std::fprintf(stderr, "dsh_create failed\n"); return 3; }
  typedef defslam_hip::MapPointStoreHIP<LmKeyFrame, LmMapPoint> Store;
  {
    Store store(ctx, 64, 2, 64);   // small on purpose: the store grows
    std::vector<LmMapPoint*> pts(P);
    for (int p = 0; p < P; p++) pts[p] = &mps[p];
    bool ok = store.ok() && store.AddMapPoints<LmFrame>(pts);
    for (int k = 0; ok && k < K; k++) ok = store.AddKeyFrame(&kfs[k]);
    ok = ok && store.AddObservations(obs_p, obs_k);
    if (!ok) { std::fprintf(stderr, "filling the store: %s\n", dsh_last_error(ctx)); return 4; }

    std::vector<LmKeyFrame*> local_kfs;
    std::vector<LmMapPoint*> local_pts;
    std::vector<int32_t> votes;
    LmKeyFrame* ref_kf = nullptr;
    const int npts = defslam_hip::UpdateLocalMapHIP(store, cur, local_kfs, local_pts, ref_kf, &votes);
    if (npts < 0) { std::fprintf(stderr, "UpdateLocalMapHIP: %s\n", dsh_last_error(ctx)); return 5; }
    std::FILE* out = std::fopen(argv[2], "w");
    auto dump_frame = [&]() {
      for (int j = 0; j < N; j++) std::fprintf(out, "%d ", cur.mvpMapPoints[j] ? (int)(cur.mvpMapPoints[j] - mps.data()) : -1);
      std::fprintf(out, "\n");
    };
    std::fprintf(out, "%zu %zu %d %d\n", local_kfs.size(), votes.size(), ref_kf ? (int)(ref_kf - kfs.data()) : -1,
                 cur.mpReferenceKF ? (int)(cur.mpReferenceKF - kfs.data()) : -1);
    for (LmKeyFrame* k : local_kfs) std::fprintf(out, "%d ", (int)(k - kfs.data()));
    std::fprintf(out, "\n");
    for (int32_t v : votes) std::fprintf(out, "%d ", v);
    std::fprintf(out, "\n");
    dump_frame();
    std::fprintf(out, "%d\n", npts);
    for (LmMapPoint* p : local_pts) std::fprintf(out, "%d ", (int)(p - mps.data()));
    std::fprintf(out, "\n");
    for (const LmKeyFrame& k : kfs) std::fprintf(out, "%lu ", k.mnTrackReferenceForFrame);
    std::fprintf(out, "\n");
    for (const LmMapPoint& p : mps) std::fprintf(out, "%lu ", p.mnTrackReferenceForFrame);
    std::fprintf(out, "\n");
    const int n2 = defslam_hip::SearchLocalPointsStoreHIP(store, cur, local_pts, 3.f);
    if (n2 < 0) { std::fprintf(stderr, "SearchLocalPointsStoreHIP: %s\n", dsh_last_error(ctx)); return 6; }
    std::fprintf(out, "%d\n", n2);
    for (LmMapPoint* p : local_pts)
      std::fprintf(out, "%d %d %.9g %.9g %.9g %d %lu\n", p->mbTrackInView ? 1 : 0, p->mnTrackScaleLevel, p->mTrackProjX, p->mTrackProjY, p->mTrackViewCos,
                   p->nVisible, p->mnLastFrameSeen);
    dump_frame();
    const std::vector<LmMapPoint*> frame_end = cur.mvpMapPoints;

    // the same frame the way it was done without the store, over the same objects: equal lists, equal final frame
    std::vector<LmKeyFrame*> all_kfs(K);
    for (int k = 0; k < K; k++) all_kfs[k] = &kfs[k];
    auto fresh_frame = [&](unsigned long id) {
      cur.mvpMapPoints = frame0;
      cur.mnId = id;
    };
    fresh_frame(8);
    std::vector<LmKeyFrame*> h_kfs;
    std::vector<LmMapPoint*> h_pts;
    LmKeyFrame* h_ref = nullptr;
    host_update_local_map(cur, all_kfs, h_kfs, h_pts, h_ref);
    const int h_n = defslam_hip::SearchLocalPointsHIP<LmFrame, LmMapPoint>(ctx, cur, h_pts, 3.f);
    const int same = h_kfs == local_kfs && h_pts == local_pts && h_ref == ref_kf && h_n == n2 && cur.mvpMapPoints == frame_end;
    std::fprintf(out, "%d\n", same);
    std::fclose(out);

    if (argc > 5) {
      const int reps = std::stoi(argv[5]);
      std::vector<double> t_host, t_shim, t_dev_up, t_dev_search;
      unsigned long id = 100;
      for (int r = 0; r < reps + 3; r++) {   // three warm-up rounds
        fresh_frame(id++);
        double t0 = now_ms();
        host_update_local_map(cur, all_kfs, h_kfs, h_pts, h_ref);
        double t1 = now_ms();
        if (defslam_hip::SearchLocalPointsHIP<LmFrame, LmMapPoint>(ctx, cur, h_pts, 3.f) < 0) return 7;
        double t2 = now_ms();
        fresh_frame(id++);
        double t3 = now_ms();
        if (defslam_hip::UpdateLocalMapHIP(store, cur, local_kfs, local_pts, ref_kf) < 0) return 7;
        double t4 = now_ms();
        if (defslam_hip::SearchLocalPointsStoreHIP(store, cur, local_pts, 3.f) < 0) return 7;
        double t5 = now_ms();
        if (r >= 3) { t_host.push_back(t1 - t0); t_shim.push_back(t2 - t1); t_dev_up.push_back(t4 - t3); t_dev_search.push_back(t5 - t4); }
      }
      std::FILE* tj = std::fopen(argv[4], "w");
      std::fprintf(tj, "{\"reps\": %d, \"keyframes\": %d, \"points\": %d, \"observations\": %d, \"frame_keypoints\": %d, \"local_points\": %zu, "
                   "\"host_update_ms\": %.4f, \"host_repack_search_ms\": %.4f, \"store_update_ms\": %.4f, \"store_search_ms\": %.4f}\n",
                   reps, K, P, R, N, local_pts.size(), median(t_host), median(t_shim), median(t_dev_up), median(t_dev_search));
      std::fclose(tj);
    }
  }
  dsh_destroy(ctx);
  return 0;
}
