// CI driver of integration/point_erase_hip.h: one culling and one drop batch of a map read from a text file, both ways over two copies
// of the same stand-in objects:
//   the store way  MapPointStoreHIP with indexed observations, reference keyframes and counters + MapPointCullingStoreHIP and
//                  DropMatchesStoreHIP: one call each, the reference's mutations written back on the objects
//   the host way   the loop of LocalMapping::MapPointCulling (LocalMapping.cc:173-199) and the drop of SchwarpDatabase.cc:288-292 over the
//                  pointer graph (the keyframes lie in one array, so pointer order is slot order)
// The stand-ins' EraseObservation and setBadFlag are shortened, so both ways use the reference's bodies written out below.
// Every mutated field is dumped per route and step; tests/test_point_erase_shim_gpu.py compares the routes with each other and with the
// restatement.
//   scene file: standin_store_scene.h, then the tail "current_kf" / P values mnFirstKFid / "R id .." (mlpRecentAddedMapPoints) /
//               "KF2 D id .." (the points one fit drops)
//   usage and exit codes: shim_driver.h
#include <fstream>
#include <list>
#include <map>

#include "point_erase_hip.h"
#include "shim_driver.h"
#include "standin_store_scene.h"

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

struct EraseScene : StoreScene {
  int current_kf = 0, KF2 = 0;
  std::list<LmMapPoint*> recent;
  std::vector<LmMapPoint*> dropped;

  bool read_file(const char* path) {
    std::ifstream f(path);
    int n = 0;
    if (!read(f) || !(f >> current_kf)) return false;
    for (LmMapPoint& m : pts) f >> m.mnFirstKFid;
    f >> n;
    for (int i = 0, p; f && i < n; i++) {
      f >> p;
      if (!f || p < 0 || p >= P) return false;
      recent.push_back(&pts[p]);
    }
    f >> KF2 >> n;
    if (!f || KF2 < 0 || KF2 >= K) return false;
    for (int i = 0, p; i < n; i++) {
      f >> p;
      if (!f || p < 0 || p >= P) return false;
      dropped.push_back(&pts[p]);
    }
    return (bool)f;
  }
};

// LocalMapping::MapPointCulling, LocalMapping.cc:173-199
void host_culling(EraseScene& s) {
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

static int drive(const DriverArgs& arg) {
  dsh_ctx* ctx = arg.ctx;
  std::FILE* o = arg.out;
  EraseScene a, b;
  if (!a.read_file(arg.in[0]) || !b.read_file(arg.in[0])) return driver_bad_input(arg.in[0]);
  // ---- the store way, on copy a ----
  Store store(ctx, 4, 2, 4);
  if (!a.fill(store)) return driver_fail(ctx, "filling the store");
  if (!defslam_hip::MapPointCullingStoreHIP(store, a.recent, (unsigned long)a.current_kf)) return driver_fail(ctx, "MapPointCullingStoreHIP");
  a.dump(o, "store", "cull", a.recent);
  if (!defslam_hip::DropMatchesStoreHIP(store, &a.kfs[a.KF2], a.dropped)) return driver_fail(ctx, "DropMatchesStoreHIP");
  a.dump(o, "store", "drop", a.recent);

  // ---- the host way, on copy b ----
  host_culling(b);
  b.dump(o, "host", "cull", b.recent);
  LmKeyFrame* KF2 = &b.kfs[b.KF2];
  for (LmMapPoint* mapPoint2 : b.dropped) {
    if (!mapPoint2->IsInKeyFrame(KF2)) continue;
    const int idx2 = mapPoint2->GetIndexInKeyFrame(KF2);
    erase_observation(mapPoint2, KF2);       // SchwarpDatabase.cc:290
    KF2->EraseMapPointMatch((size_t)idx2);   // :291
  }
  b.dump(o, "host", "drop", b.recent);
  return 0;
}

int main(int argc, char** argv) { return run_driver(argc, argv, 1, drive); }
