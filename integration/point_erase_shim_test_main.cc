// CI driver of integration/point_erase_hip.h: one culling and one drop batch of a map read from a text file, both ways over two copies
// of the same stand-in objects:
//   the store way  MapPointStoreHIP with indexed observations, reference keyframes and counters + MapPointCullingStoreHIP and
//                  DropMatchesStoreHIP: one call each, the reference's mutations written back on the objects
//   the host way   the loop of LocalMapping::MapPointCulling (LocalMapping.cc:173-199) and the drop of SchwarpDatabase.cc:288-292 over the
//                  pointer graph (the keyframes lie in one array, so pointer order is slot order)
// The stand-ins' EraseObservation and setBadFlag are shortened, so both ways use the reference's bodies written out below.
// Every mutated field is dumped per route and step; tests/test_point_erase_shim_gpu.py compares the routes with each other and with the
// restatement.
//   map file: P K / P lines "bad ref found visible first_kf" / K lines "N t0 .. tN-1" / L / L lines "point kf idx" /
//             "current_kf R id .." (mlpRecentAddedMapPoints) / "KF2 D id .." (the points one fit drops)
//   usage: point_erase_shim_test <map.txt> <output.txt> [device]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <list>
#include <map>

#include "anchor_pairs_hip.h"
#include "point_erase_hip.h"
#include "standin_localmap_types.h"

using namespace standin;

namespace {

// DefMapPoint::setBadFlag, Modules/Common/DefMapPoint.cc:76-94
void set_bad_flag(LmMapPoint* p) {
  std::map<LmKeyFrame*, size_t> obs;
  p->bad = true;
  obs = p->mObservations;
  p->mObservations.clear();
  for (std::map<LmKeyFrame*, size_t>::iterator mit = obs.begin(), mend = obs.end(); mit != mend; mit++) {
    LmKeyFrame* pKF = mit->first;
    pKF->EraseMapPointMatch(mit->second);
  }
}

// MapPoint::EraseObservation, Thirdparty/ORBSLAM_2/src/MapPoint.cc:122-148 (monocular)
void erase_observation(LmMapPoint* p, LmKeyFrame* pKF) {
  bool bBad = false;
  if (p->mObservations.count(pKF)) {
    p->nObs--;
    p->mObservations.erase(pKF);
    if (p->mpRefKF == pKF && !p->mObservations.empty())   // the reference reads begin() of an empty map there
      p->mpRefKF = p->mObservations.begin()->first;
    if (p->nObs <= 2) bBad = true;
  }
  if (bBad) set_bad_flag(p);
}

}  // namespace

namespace defslam_hip {
template <>
struct EraseAccess<LmKeyFrame, LmMapPoint> {
  static void erase_observation(LmMapPoint* p, LmKeyFrame* kf) { ::erase_observation(p, kf); }
  static void set_bad_flag(LmMapPoint* p) { ::set_bad_flag(p); }
};
}  // namespace defslam_hip

typedef defslam_hip::MapPointStoreHIP<LmKeyFrame, LmMapPoint> Store;

namespace {

struct Scene {
  std::vector<LmKeyFrame> kfs;      // one array: pointer order is slot order
  std::vector<LmMapPoint> pts;
  std::vector<int> log_p, log_k, log_i;
  int current_kf = 0, KF2 = 0;
  std::list<LmMapPoint*> recent;
  std::vector<LmMapPoint*> dropped;
};

bool read_scene(const char* path, Scene& s) {
  std::ifstream f(path);
  int P, K;
  if (!(f >> P >> K)) return false;
  s.pts.resize(P);
  s.kfs.resize(K);
  for (int p = 0; p < P; p++) {
    LmMapPoint& m = s.pts[p];
    int bad, ref;
    f >> bad >> ref >> m.mnFound >> m.nVisible >> m.mnFirstKFid;
    m.bad = bad != 0;
    m.mpRefKF = ref >= 0 ? &s.kfs[ref] : nullptr;
  }
  for (int k = 0; k < K; k++) {
    LmKeyFrame& kf = s.kfs[k];
    f >> kf.N;
    kf.mnId = (unsigned long)k;
    kf.mvpMapPoints.assign(kf.N, nullptr);
    for (int j = 0; j < kf.N; j++) {
      int t;
      f >> t;
      if (t >= 0) kf.mvpMapPoints[j] = &s.pts[t];
    }
  }
  int L, n;
  f >> L;
  s.log_p.resize(L); s.log_k.resize(L); s.log_i.resize(L);
  for (int r = 0; r < L; r++) {
    f >> s.log_p[r] >> s.log_k[r] >> s.log_i[r];
    s.pts[s.log_p[r]].AddObservation(&s.kfs[s.log_k[r]], (size_t)s.log_i[r]);
  }
  f >> s.current_kf >> n;
  for (int i = 0, p; i < n; i++) { f >> p; s.recent.push_back(&s.pts[p]); }
  f >> s.KF2 >> n;
  for (int i = 0, p; i < n; i++) { f >> p; s.dropped.push_back(&s.pts[p]); }
  return (bool)f;
}

void dump(FILE* o, const char* route, const char* step, Scene& s) {
  std::fprintf(o, "%s %s recent", route, step);
  for (LmMapPoint* p : s.recent) std::fprintf(o, " %d", (int)(p - &s.pts[0]));
  std::fprintf(o, "\n");
  for (size_t p = 0; p < s.pts.size(); p++) {
    LmMapPoint& m = s.pts[p];
    std::fprintf(o, "%s %s pt %d %d %d %d |", route, step, (int)p, m.isBad() ? 1 : 0, m.nObs,
                 m.GetReferenceKeyFrame() ? (int)(m.GetReferenceKeyFrame() - &s.kfs[0]) : -1);
    const std::map<LmKeyFrame*, size_t> obs = m.GetObservations();
    for (const auto& kv : obs) std::fprintf(o, " %d:%d", (int)(kv.first - &s.kfs[0]), (int)kv.second);
    std::fprintf(o, "\n");
  }
  for (size_t k = 0; k < s.kfs.size(); k++) {
    std::fprintf(o, "%s %s kf %d", route, step, (int)k);
    for (LmMapPoint* p : s.kfs[k].mvpMapPoints) std::fprintf(o, " %d", p ? (int)(p - &s.pts[0]) : -1);
    std::fprintf(o, "\n");
  }
}

// LocalMapping::MapPointCulling, LocalMapping.cc:173-199
void host_culling(Scene& s) {
  std::list<LmMapPoint*>::iterator lit = s.recent.begin();
  const unsigned long int nCurrentKFid = (unsigned long)s.current_kf;
  while (lit != s.recent.end()) {
    LmMapPoint* pMP = *lit;
    if (pMP->isBad()) {
      lit = s.recent.erase(lit);
    } else if (pMP->GetFoundRatio() < 0.40f) {
      set_bad_flag(pMP);
      lit = s.recent.erase(lit);
    } else if (((int)nCurrentKFid - (int)pMP->mnFirstKFid) >= 3)
      lit = s.recent.erase(lit);
    else
      lit++;
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s <map.txt> <output.txt> [device]\n", argv[0]); return 2; }
  const int device = argc > 3 ? std::atoi(argv[3]) : 0;
  Scene a, b;
  if (!read_scene(argv[1], a) || !read_scene(argv[1], b)) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  dsh_ctx* ctx = nullptr;
  if (dsh_create(&ctx, device) != DSH_OK) { std::fprintf(stderr, "dsh_create failed\n"); return 1; }
  FILE* o = std::fopen(argv[2], "w");
  if (!o) return 2;
  int rc = 1;
  {
    // ---- the store way, on copy a ----
    Store store(ctx, 4, 2, 4);
    std::vector<LmMapPoint*> all, lp;
    std::vector<LmKeyFrame*> lk;
    std::vector<int32_t> ids, visible, found;
    for (size_t p = 0; p < a.pts.size(); p++) {
      all.push_back(&a.pts[p]);
      ids.push_back((int32_t)p);
      visible.push_back(a.pts[p].nVisible);
      found.push_back(a.pts[p].mnFound);
    }
    bool ok = store.ok() && store.AddMapPoints<LmFrame>(all);
    for (size_t k = 0; ok && k < a.kfs.size(); k++) ok = store.AddKeyFrame(&a.kfs[k]);
    for (size_t r = 0; r < a.log_p.size(); r++) {
      lp.push_back(&a.pts[a.log_p[r]]);
      lk.push_back(&a.kfs[a.log_k[r]]);
    }
    ok = ok && defslam_hip::AddObservationsIndexedHIP(store, lp, lk, a.log_i) && defslam_hip::SetReferenceKeyFramesHIP(store, all) &&
         dsh_trackstate_set_counters(store.handle(), (int)ids.size(), ids.data(), visible.data(), found.data()) == DSH_OK;
    ok = ok && defslam_hip::MapPointCullingStoreHIP(store, a.recent, (unsigned long)a.current_kf);
    if (ok) dump(o, "store", "cull", a);
    ok = ok && defslam_hip::DropMatchesStoreHIP(store, &a.kfs[a.KF2], a.dropped);
    if (ok) dump(o, "store", "drop", a);
    if (!ok) std::fprintf(stderr, "store way: %s\n", dsh_last_error(ctx));

    // ---- the host way, on copy b ----
    host_culling(b);
    dump(o, "host", "cull", b);
    LmKeyFrame* KF2 = &b.kfs[b.KF2];
    for (LmMapPoint* mapPoint2 : b.dropped) {
      if (!mapPoint2->IsInKeyFrame(KF2)) continue;
      const int idx2 = mapPoint2->GetIndexInKeyFrame(KF2);
      erase_observation(mapPoint2, KF2);       // SchwarpDatabase.cc:290
      KF2->EraseMapPointMatch((size_t)idx2);   // :291
    }
    dump(o, "host", "drop", b);
    rc = ok ? 0 : 1;
  }
  std::fclose(o);
  dsh_destroy(ctx);
  return rc;
}
