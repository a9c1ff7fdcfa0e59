// CI driver of integration/schwarp_store_hip.h: SchwarpDatabase::add of one new keyframe with several anchors, of a map read from a
// text file, both ways over two copies of the same stand-in objects:
//   the store way  MapPointStoreHIP + a keyframe store + the resident Surface and view of every keyframe, then
//                  SchwarpDatabaseStoreHIP::add = AnchorPairsHIP + one dsh_keyframe_warp_pair per anchor, the results written back on
//                  the objects, DropMatchHIP / DropQueryHIP between the anchors
//   the host way   a subclass of SchwarpDatabaseHIP (schwarp_database_hip.h) with device records enabled that calls its protected
//                  findbyWarp / calculateSchwarps per anchor by ascending slot: host-gathered arrays, four library calls per anchor, the
//                  bookkeeping on the objects
// Dumped per route: every mutated field of the objects (standin_store_scene.h), "x <anchor slot> <bit patterns>" per fitted anchor,
// "related n", and per point with new information "normal p status k1 k2 n0 n1 n2" (bit patterns) of dsh_normals_estimate_db on the
// route's own database; for the store route also "table k .." read back from the device.  tests/test_warp_pair_shim_gpu.py compares.
// The stand-in EraseObservation has neither the move of the reference keyframe nor the nObs <= 2 cascade (standin_localmap_types.h),
// and the host way decides the stored records before its drops: the test's scene keeps every point above two observations and
// anchored in an old keyframe, and has no two entries on one key point.
//   scene file: standin_store_scene.h with appearance, then the tail "slot lambda" and per keyframe
//               "NCu NCv umin umax vmin vmax fx fy cx cy mnMinX mnMaxX mnMinY mnMaxY" and N lines "kpn.x kpn.y px.x px.y"
//   usage and exit codes: shim_driver.h
#include <cstring>
#include <fstream>
#include <map>

#include "schwarp_database_hip.h"
#include "schwarp_store_hip.h"
#include "shim_driver.h"
#include "standin_store_scene.h"

using namespace standin;
typedef defslam_hip::MapPointStoreHIP<LmKeyFrame, LmMapPoint> Store;
typedef defslam_hip::SchwarpDatabaseStoreHIP<LmWarpDatabase, LmKeyFrame, LmMapPoint> StoreDB;
typedef defslam_hip::SchwarpDatabaseHIP<LmWarpDatabase, LmKeyFrame, LmKeyFrame, LmMapPoint, LmDiffProp> HostBase;

namespace {

struct PairScene : StoreScene {
  int new_slot = 0;
  double lambda = 0.0;
  bool read_file(const char* path) {
    std::ifstream f(path);
    if (!read(f) || !appearance || !(f >> new_slot >> lambda) || new_slot < 0 || new_slot >= K) return false;
    for (LmKeyFrame& k : kfs) {
      f >> k.NCu >> k.NCv >> k.umin >> k.umax >> k.vmin >> k.vmax >> k.fx >> k.fy >> k.cx >> k.cy >> k.mnMinX >> k.mnMaxX >> k.mnMinY >> k.mnMaxY;
      k.mpKeypointNorm.resize(k.N);
      for (int i = 0; i < k.N; i++) f >> k.mpKeypointNorm[i].pt.x >> k.mpKeypointNorm[i].pt.y >> k.mvKeysUn[i].pt.x >> k.mvKeysUn[i].pt.y;
      k.mvInvLevelSigma2.resize(k.mvScaleFactors.size());
      for (size_t l = 0; l < k.mvScaleFactors.size(); l++) {              // ORBextractor.cc:422,430
        const float sigma2 = k.mvScaleFactors[l] * k.mvScaleFactors[l];
        k.mvInvLevelSigma2[l] = 1.0f / sigma2;
      }
    }
    return (bool)f;
  }
};

// the keyframe store of StoreScene::fill, by the C ABI
struct KfStore {
  dsh_kfdb* db = nullptr;
  explicit KfStore(dsh_ctx* ctx) { if (dsh_kfdb_create(ctx, 4, &db) != DSH_OK) db = nullptr; }
  ~KfStore() { if (db) dsh_kfdb_destroy(db); }
  int Slot(LmKeyFrame* kf, int* rc) {
    dsh_mp_keyframe k;
    std::memset(&k, 0, sizeof(k));
    std::memcpy(k.Ow, kf->Ow, sizeof(k.Ow));
    k.N = kf->N;
    std::vector<int32_t> oct(kf->N + 1);
    for (int j = 0; j < kf->N; j++) oct[j] = kf->mvKeysUn[j].octave;
    k.desc = kf->mDescriptors.data(); k.octave = oct.data();
    k.levels = kf->mnScaleLevels; k.scale_factors = kf->mvScaleFactors.data();
    k.bad = kf->isBad() ? 1 : 0;
    int32_t s = -1;
    *rc = dsh_kfdb_add(db, &k, &s);
    return *rc == DSH_OK ? s : -1;
  }
};

// SchwarpDatabase::add with the anchors by ascending slot (the objects lie in one array: pointer order is slot order)
struct HostDB : HostBase {
  HostDB(dsh_ctx* ctx, double lambda) : HostBase(ctx, lambda) {}
  std::vector<std::pair<LmKeyFrame*, std::vector<double>>> xs;
  void add_by_slot(LmKeyFrame* KF2) {
    const std::vector<LmMapPoint*> vpMapPointMatches = KF2->GetMapPointMatches();
    std::map<LmKeyFrame*, int> countKFMatches;
    for (LmMapPoint* mapPoint : vpMapPointMatches) {
      if (!mapPoint || mapPoint->isBad()) continue;
      countKFMatches[mapPoint->GetReferenceKeyFrame()]++;
    }
    for (const auto& kv : countKFMatches) {
      LmKeyFrame* refkf = kv.first;
      Matches vMatchedIndices;
      for (LmMapPoint* mapPoint : vpMapPointMatches) {
        if (!mapPoint || mapPoint->isBad()) continue;
        if (mapPoint->IsInKeyFrame(KF2) && mapPoint->IsInKeyFrame(refkf))
          vMatchedIndices.push_back({(size_t)mapPoint->GetIndexInKeyFrame(refkf), (size_t)mapPoint->GetIndexInKeyFrame(KF2)});
      }
      if (vMatchedIndices.size() < 20) continue;
      std::vector<double> x(2 * (size_t)refkf->NCu * refkf->NCv, 0.0);
      findbyWarp(refkf, KF2, vMatchedIndices, x, lambda_);
      if (last_status() == DSH_OK && vMatchedIndices.size() >= 20) {
        calculateSchwarps(refkf, KF2, vMatchedIndices, x, lambda_);
        KF2->KeyframesRelated++;
        xs.push_back(std::make_pair(refkf, x));
      }
      if (last_status() != DSH_OK) return;
    }
  }
};

void dump_x(std::FILE* f, const char* route, int slot, const std::vector<double>& x) {
  std::fprintf(f, "%s x %d", route, slot);
  for (double v : x) {
    unsigned long long u;
    std::memcpy(&u, &v, 8);
    std::fprintf(f, " %llu", u);
  }
  std::fprintf(f, "\n");
}

// NormalEstimator's solve over the route's database for the points with new information: ids[n] names point pts[n] in the database
int dump_normals(dsh_ctx* ctx, std::FILE* f, const char* route, dsh_diffdb* ddb, PairScene& sc, const std::vector<LmMapPoint*>& pts, const std::vector<int32_t>& ids) {
  const size_t P = pts.size();
  if (P == 0) return DSH_OK;
  std::vector<float> x0(2 * P, 0.f), uv(2 * P), nref(3 * P);
  std::vector<uint8_t> has(P, 0);
  std::vector<double> k(2 * P), cov(4 * P);
  std::vector<int32_t> st(P), it(P);
  for (size_t n = 0; n < P; n++) {
    LmKeyFrame* ref = pts[n]->GetReferenceKeyFrame();
    const int idx = pts[n]->GetIndexInKeyFrame(ref);
    uv[2 * n] = ref->mpKeypointNorm[idx].pt.x; uv[2 * n + 1] = ref->mpKeypointNorm[idx].pt.y;
  }
  int32_t n_rec = 0;
  const int rc = dsh_normals_estimate_db(ctx, ddb, (int)P, ids.data(), x0.data(), has.data(), uv.data(), k.data(), cov.data(), st.data(), nref.data(), it.data(), 0,
                                         &n_rec, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (rc != DSH_OK) return rc;
  for (size_t n = 0; n < P; n++) {
    unsigned long long u[2];
    uint32_t w[3];
    std::memcpy(u, &k[2 * n], 16);
    std::memcpy(w, &nref[3 * n], 12);
    std::fprintf(f, "%s normal %d %d %llu %llu %u %u %u\n", route, sc.id(pts[n]), st[n], u[0], u[1], w[0], w[1], w[2]);
  }
  return DSH_OK;
}

}  // namespace

static int drive(const DriverArgs& arg) {
  dsh_ctx* ctx = arg.ctx;
  std::FILE* f = arg.out;
  PairScene sa, sh;
  if (!sa.read_file(arg.in[0]) || !sh.read_file(arg.in[0])) return driver_bad_input(arg.in[0]);
  const std::vector<LmMapPoint*> none;

  {  // ---- the store way
    Store store(ctx, 16, 2, 16);
    KfStore kfstore(ctx);
    if (!kfstore.db || !sa.fill(store, &kfstore)) return driver_fail(ctx, "filling the stores");
    dsh_diffdb* ddb = nullptr;
    if (dsh_diffdb_create(ctx, 4, &ddb) != DSH_OK) return driver_fail(ctx, "dsh_diffdb_create");
    for (int k = 0; k < sa.K; k++) {
      LmKeyFrame& kf = sa.kfs[k];
      std::vector<float> kpn(2 * (size_t)kf.N + 2);
      for (int i = 0; i < kf.N; i++) { kpn[2 * i] = kf.mpKeypointNorm[i].pt.x; kpn[2 * i + 1] = kf.mpKeypointNorm[i].pt.y; }
      if (dsh_keyframe_surface_init(store.handle(), k, kf.N, kpn.data()) != DSH_OK || !defslam_hip::SetViewStoreHIP(store, &kf))
        return driver_fail(ctx, "the Surface and the view of a keyframe");
    }
    defslam_hip::WarpPairSetup setup;
    setup.ctx = ctx; setup.kfdb = kfstore.db; setup.ddb = ddb; setup.lambda = sa.lambda;
    int rc = 0;
    {
      StoreDB db(store, setup);
      db.add(&sa.kfs[0]);                                    // the first keyframe only enters the set (SchwarpDatabase.cc:54-58)
      db.add(&sa.kfs[sa.new_slot]);
      if (!db.ok()) rc = driver_fail(ctx, "SchwarpDatabaseStoreHIP::add");
      if (!rc) {
        sa.dump(f, "store", "pair", none);
        for (const auto& o : db.outcomes) {
          if (o.second.r.fitted) dump_x(f, "store", sa.slot(o.first), o.second.x);
          std::fprintf(f, "store counts %d %d %d %d %d %d %d %d\n", sa.slot(o.first), o.second.r.n_filtered, o.second.r.n_matched, o.second.r.n_list,
                       o.second.r.n_dropped, o.second.r.n_stored, o.second.r.n_skipped, o.second.r.fitted);
        }
        std::fprintf(f, "store related %d\n", sa.kfs[sa.new_slot].KeyframesRelated);
        std::vector<LmMapPoint*> pts;
        std::vector<int32_t> ids;
        for (auto& kv : db.getToProccess())
          if (kv.second) { pts.push_back(kv.first); ids.push_back(store.id(kv.first)); }
        if (dump_normals(ctx, f, "store", ddb, sa, pts, ids) != DSH_OK) rc = driver_fail(ctx, "dsh_normals_estimate_db (store)");
        for (int k = 0; !rc && k < sa.K; k++) {
          std::vector<int32_t> t(sa.kfs[k].N + 1);
          if (dsh_point_store_get_keyframe_table(store.handle(), k, sa.kfs[k].N, t.data()) != DSH_OK) rc = driver_fail(ctx, "the table read-back");
          std::fprintf(f, "store table %d", k);
          for (int i = 0; i < sa.kfs[k].N; i++) std::fprintf(f, " %d", t[i]);
          std::fprintf(f, "\n");
        }
      }
    }
    dsh_diffdb_destroy(ddb);
    if (rc) return rc;
  }

  {  // ---- the host way
    HostDB db(ctx, sh.lambda);
    if (!db.enable_device_records(4)) return driver_fail(ctx, "enable_device_records");
    db.add_by_slot(&sh.kfs[sh.new_slot]);
    if (db.last_status() != DSH_OK) return driver_fail(ctx, "SchwarpDatabaseHIP");
    sh.dump(f, "host", "pair", none);
    for (const auto& o : db.xs) dump_x(f, "host", sh.slot(o.first), o.second);
    std::fprintf(f, "host related %d\n", sh.kfs[sh.new_slot].KeyframesRelated);
    std::vector<LmMapPoint*> pts;
    std::vector<int32_t> ids;
    for (auto& kv : db.getToProccess())
      if (kv.second) { pts.push_back(kv.first); ids.push_back(db.device_point_id(kv.first)); }
    if (dump_normals(ctx, f, "host", db.device_records(), sh, pts, ids) != DSH_OK) return driver_fail(ctx, "dsh_normals_estimate_db (host)");
  }
  return 0;
}

int main(int argc, char** argv) { return run_driver(argc, argv, 1, drive); }
