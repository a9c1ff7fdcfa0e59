// What the CI drivers of the local map and of the end of a tracked frame share (localmap_shim_test_main.cc, trackclose_shim_test_main.cc):
// the map and the current frame of a synth.write_local_map_scene file as stand-in objects, and Tracking::UpdateLocalMap as the host does it.
#pragma once
#include <fstream>
#include <map>
#include <set>
#include <vector>

#include "standin_localmap_types.h"

namespace standin {

// the stand-in objects live in arrays, so pointer order is index order
struct LmScene {
  int levels = 0, P = 0, K = 0, R = 0, N = 0;
  std::vector<LmMapPoint> mps;
  std::vector<LmKeyFrame> kfs;
  std::vector<LmMapPoint*> obs_p;
  std::vector<LmKeyFrame*> obs_k;
  LmFrame cur;

  bool read(std::istream& in) {
    float logsf;
    in >> levels >> logsf;
    std::vector<float> sf(levels > 0 ? levels : 0);
    for (float& s : sf) in >> s;
    // map points: x y z nx ny nz maxd bad desc[32]
    in >> P;
    mps.assign(P > 0 ? P : 0, LmMapPoint());
    for (LmMapPoint& m : mps) {
      int bad;
      in >> m.pos[0] >> m.pos[1] >> m.pos[2] >> m.normal[0] >> m.normal[1] >> m.normal[2] >> m.mfMaxDistance >> bad;
      m.bad = bad != 0;
      for (auto& b : m.desc) { int v; in >> v; b = (uint8_t)v; }
    }
    // keyframes: parent bad n, then n table entries (point id or -1)
    in >> K;
    kfs.assign(K > 0 ? K : 0, LmKeyFrame());
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
    obs_p.resize(R > 0 ? R : 0);
    obs_k.resize(R > 0 ? R : 0);
    for (int r = 0; r < R; r++) {
      int p, k;
      in >> p >> k;
      obs_p[r] = &mps[p];
      obs_k[r] = &kfs[k];
      mps[p].mObservations[&kfs[k]] = 0;
      mps[p].nObs++;
    }
    // the current frame: camera, pose, centre, key points (x y octave point-id desc[32])
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
    return (bool)in;
  }
};

// Tracking::UpdateLocalKeyFrames (Tracking.cc:1510-1629) and DefTracking::UpdateLocalPoints (DefTracking.cc:426-454) as the host does
// them: ordered containers keyed by pointer, one tree insertion per observation of every point the frame holds.
inline void host_update_local_map(LmFrame& F, const std::vector<LmKeyFrame*>& all_kfs, std::vector<LmKeyFrame*>& local_kfs,
                                  std::vector<LmMapPoint*>& local_pts, LmKeyFrame*& ref_kf) {
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

}  // namespace standin
