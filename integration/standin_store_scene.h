// What the CI drivers of the mapping thread's store calls share (anchor_pairs_, keyframe_insert_, point_erase_shim_test_main.cc): the
// state of the two resident stores from a tests/store_model.py write_scene file as stand-in objects, its replay into the stores, and the
// dump of every field the calls mutate.
//   "store_scene P K R appearance"
//   P lines   "x y z nx ny nz max_distance min_distance bad ref n_obs found visible d0 .. d31"
//   K blocks  "N parent bad t0 .. tN-1", and with appearance "Owx Owy Owz levels sf0 .." and N lines "octave d0 .. d31"
//   R lines   "point slot idx live": the log in arrival order, an erased record blanked (live 0)
// and after these a tail that the driver reads itself.
#pragma once
#include <cstdio>
#include <cstring>
#include <istream>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "anchor_pairs_hip.h"
#include "standin_localmap_types.h"

namespace standin {

// the stand-in objects live in arrays, so pointer order is slot order
struct StoreScene {
  int P = 0, K = 0, R = 0, appearance = 0;
  std::vector<LmMapPoint> pts;
  std::vector<LmKeyFrame> kfs;
  std::vector<int> log_p, log_k, log_i, log_live;

  int id(const LmMapPoint* p) const { return p ? (int)(p - pts.data()) : -1; }
  int slot(const LmKeyFrame* k) const { return k ? (int)(k - kfs.data()) : -1; }

  // leaves the stream at the tail
  bool read(std::istream& in) {
    std::string magic;
    in >> magic >> P >> K >> R >> appearance;
    if (!in || magic != "store_scene" || P < 0 || K < 0 || R < 0) return false;
    pts.assign(P, LmMapPoint());
    kfs.assign(K, LmKeyFrame());
    std::vector<int> n_obs(P);
    for (int p = 0; p < P; p++) {
      LmMapPoint& m = pts[p];
      int bad, ref;
      in >> m.pos[0] >> m.pos[1] >> m.pos[2] >> m.normal[0] >> m.normal[1] >> m.normal[2] >> m.mfMaxDistance >> m.mfMinDistance >> bad >> ref >>
          n_obs[p] >> m.mnFound >> m.nVisible;
      if (!in || ref < -1 || ref >= K) return false;
      m.bad = bad != 0;
      m.mpRefKF = ref >= 0 ? &kfs[ref] : nullptr;
      for (auto& b : m.desc) { int v; in >> v; b = (uint8_t)v; }
    }
    for (int k = 0; k < K; k++) {
      LmKeyFrame& kf = kfs[k];
      int parent, bad;
      in >> kf.N >> parent >> bad;
      if (!in || kf.N < 0 || parent < -1 || parent >= K) return false;
      kf.mnId = (unsigned long)k;
      kf.bad = bad != 0;
      kf.mpParent = parent >= 0 ? &kfs[parent] : nullptr;
      if (parent >= 0) kfs[parent].mspChildrens.insert(&kf);
      kf.mvpMapPoints.assign(kf.N, nullptr);
      for (auto& p : kf.mvpMapPoints) {
        int t;
        in >> t;
        if (!in || t < -1 || t >= P) return false;
        p = t >= 0 ? &pts[t] : nullptr;
      }
      if (!appearance) continue;
      in >> kf.Ow[0] >> kf.Ow[1] >> kf.Ow[2] >> kf.mnScaleLevels;
      if (!in || kf.mnScaleLevels < 0) return false;
      kf.mvScaleFactors.resize(kf.mnScaleLevels);
      for (float& s : kf.mvScaleFactors) in >> s;
      kf.mvKeysUn.resize(kf.N);
      kf.mDescriptors.resize(32 * (size_t)kf.N);
      for (int j = 0; j < kf.N; j++) {
        in >> kf.mvKeysUn[j].octave;
        for (int b = 0; b < 32; b++) { int v; in >> v; kf.mDescriptors[32 * (size_t)j + b] = (uint8_t)v; }
      }
    }
    log_p.resize(R); log_k.resize(R); log_i.resize(R); log_live.resize(R);
    for (int r = 0; r < R; r++) {
      in >> log_p[r] >> log_k[r] >> log_i[r] >> log_live[r];
      if (!in || log_p[r] < 0 || log_p[r] >= P || log_k[r] < 0 || log_k[r] >= K || log_i[r] < -1 || log_i[r] >= kfs[log_k[r]].N) return false;
      if (log_live[r]) pts[log_p[r]].mObservations[&kfs[log_k[r]]] = (size_t)log_i[r];
    }
    for (int p = 0; p < P; p++) pts[p].nObs = n_obs[p];   // not the size of mObservations once setBadFlag has cleared them
    return (bool)in;
  }

  // The replay into an empty point store, and into a keyframe store when given, by the rule of MapModel.fill (tests/store_model.py).  The
  // device log ends up in the file's order, blanked records too: a pair that is in the batch already closes the batch, and a batch's
  // erased records are blanked right after it.  Unlike MapModel.fill it refuses a record without a key point index (idx -1), which the
  // file format allows: the store calls of the drivers refuse a store that holds one.
  template <class Store, class KfStore>
  bool fill(Store& store, KfStore* kfstore) {
    std::vector<LmMapPoint*> all(P);
    std::vector<int32_t> ids(P), visible(P), found(P);
    for (int p = 0; p < P; p++) {
      all[p] = &pts[p];
      ids[p] = p;
      visible[p] = pts[p].nVisible;
      found[p] = pts[p].mnFound;
    }
    bool ok = store.ok() && store.template AddMapPoints<LmFrame>(all) &&
              dsh_trackstate_set_counters(store.handle(), P, ids.data(), visible.data(), found.data()) == DSH_OK;
    for (int k = 0; ok && k < K; k++) {
      LmKeyFrame* parent = kfs[k].mpParent;                 // a parent that comes later in slot order is set once it exists
      if (slot(parent) > k) kfs[k].mpParent = nullptr;
      int rc = DSH_OK;
      ok = store.AddKeyFrame(&kfs[k]) && (!kfstore || kfstore->Slot(&kfs[k], &rc) == k);
      kfs[k].mpParent = parent;
    }
    for (int k = 0; ok && k < K; k++)
      if (slot(kfs[k].mpParent) > k) ok = store.SetParent(&kfs[k], kfs[k].mpParent);
    std::vector<LmMapPoint*> bp, ep;
    std::vector<LmKeyFrame*> bk, ek;
    std::vector<int> bi;
    std::set<std::pair<int, int>> pairs;
    for (int r = 0; ok && r <= R; r++) {
      if (r < R && log_i[r] < 0) {
        std::fprintf(stderr, "StoreScene::fill: record %d has no key point index\n", r);
        return false;
      }
      if (r == R || pairs.count(std::make_pair(log_p[r], log_k[r]))) {
        ok = bp.empty() || (defslam_hip::AddObservationsIndexedHIP(store, bp, bk, bi) && (ep.empty() || store.EraseObservations(ep, ek)));
        bp.clear(); bk.clear(); bi.clear(); ep.clear(); ek.clear(); pairs.clear();
        if (r == R) break;
      }
      pairs.insert(std::make_pair(log_p[r], log_k[r]));
      bp.push_back(&pts[log_p[r]]); bk.push_back(&kfs[log_k[r]]); bi.push_back(log_i[r]);
      if (!log_live[r]) { ep.push_back(bp.back()); ek.push_back(bk.back()); }
    }
    return ok && defslam_hip::SetReferenceKeyFramesHIP(store, all);
  }

  struct NoKeyFrameStore {
    int Slot(LmKeyFrame*, int*) { return -1; }
  };
  template <class Store>
  bool fill(Store& store) { return fill(store, (NoKeyFrameStore*)nullptr); }

  // Every field a store call mutates, floats as bit patterns, in lines "route step kind ..":
  //   recent  id ..                                                           (the list the driver passes, may be empty)
  //   pt      p bad n_obs ref found visible | xyz normal max min (bits) | d0 .. d31 | slot:idx ..
  //   kf      slot parent bad t0 .. tN-1
  template <class Recent>
  void dump(std::FILE* o, const char* route, const char* step, const Recent& recent) const {
    std::fprintf(o, "%s %s recent", route, step);
    for (const LmMapPoint* p : recent) std::fprintf(o, " %d", id(p));
    std::fprintf(o, "\n");
    for (int p = 0; p < P; p++) {
      const LmMapPoint& m = pts[p];
      std::fprintf(o, "%s %s pt %d %d %d %d %d %d |", route, step, p, m.bad ? 1 : 0, m.nObs, slot(m.mpRefKF), m.mnFound, m.nVisible);
      const float f[8] = {m.pos[0], m.pos[1], m.pos[2], m.normal[0], m.normal[1], m.normal[2], m.mfMaxDistance, m.mfMinDistance};
      for (float v : f) {
        uint32_t u;
        std::memcpy(&u, &v, 4);
        std::fprintf(o, " %u", u);
      }
      std::fprintf(o, " |");
      for (uint8_t b : m.desc) std::fprintf(o, " %d", (int)b);
      std::fprintf(o, " |");
      for (const auto& kv : m.mObservations) std::fprintf(o, " %d:%d", slot(kv.first), (int)kv.second);
      std::fprintf(o, "\n");
    }
    for (int k = 0; k < K; k++) {
      std::fprintf(o, "%s %s kf %d %d %d", route, step, k, slot(kfs[k].mpParent), kfs[k].bad ? 1 : 0);
      for (const LmMapPoint* p : kfs[k].mvpMapPoints) std::fprintf(o, " %d", id(p));
      std::fprintf(o, "\n");
    }
  }
};

}  // namespace standin
