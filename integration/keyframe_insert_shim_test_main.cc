// CI driver of integration/keyframe_insert_hip.h: one new keyframe and one repose upkeep of a map read from a text file, both ways over
// two copies of the same stand-in objects:
//   the store way  MapPointStoreHIP + KeyFrameStoreHIP, ProcessNewKeyFrameStoreHIP and ReposeUpkeepStoreHIP: one call each, the results
//                  written back on the objects
//   the host way   ProcessNewKeyFrameHIP and UpdateMapPointsHIP of mappoint_upkeep_hip.h: the loop over the host objects and
//                  dsh_mappoint_update with the lists of std::map<KeyFrame*, size_t> (the keyframes lie in one array, so pointer order
//                  is slot order)
// Between the two steps the driver gives some points a facet and a new position in both copies and in the store, which is what a
// template switch leaves behind for Repose; it does not run the switch itself (tmplswitch_shim_test_main.cc does).
// Every mutated field is dumped per route and step, floats as bit patterns; tests/test_keyframe_insert_shim_gpu.py compares the routes
// with each other and with the restatement.
//   scene file: standin_store_scene.h with appearance, then the tail "slot E" / E lines "point x y z" (facet and new position)
//   usage and exit codes: shim_driver.h
#include <cstring>
#include <fstream>

#include "keyframe_insert_hip.h"
#include "shim_driver.h"
#include "standin_store_scene.h"

using namespace standin;

namespace defslam_hip {
// the stand-ins of standin_localmap_types.h name these members desc / normal
template <>
struct MapPointAccess<LmKeyFrame, LmMapPoint> {
  static void center(LmKeyFrame* kf, float* Ow) { std::memcpy(Ow, kf->Ow, 3 * sizeof(float)); }
  static const uint8_t* descriptors(LmKeyFrame* kf) { return kf->mDescriptors.data(); }
  static void world_pos(LmMapPoint* p, float* x) { std::memcpy(x, p->pos, 3 * sizeof(float)); }
  static void descriptor(LmMapPoint* p, uint8_t* d) { std::memcpy(d, p->desc, 32); }
  static void set_descriptor(LmMapPoint* p, const uint8_t* d) { std::memcpy(p->desc, d, 32); }
  static void set_normal_and_depth(LmMapPoint* p, const float* n, float max_d, float min_d) {
    std::memcpy(p->normal, n, 3 * sizeof(float));
    p->mfMaxDistance = max_d;
    p->mfMinDistance = min_d;
  }
};
}  // namespace defslam_hip

typedef defslam_hip::MapPointStoreHIP<LmKeyFrame, LmMapPoint> Store;
typedef defslam_hip::KeyFrameStoreHIP<LmKeyFrame, LmMapPoint> KfStore;

namespace {

struct InsertScene : StoreScene {
  int slot = 0;
  std::vector<int> emb;
  std::vector<float> emb_xyz;
  LmFacet facet;

  bool read_file(const char* path) {
    std::ifstream f(path);
    int E = 0;
    if (!read(f) || !appearance || !(f >> slot >> E) || slot < 0 || slot >= K || E < 0) return false;
    emb.resize(E);
    emb_xyz.resize(3 * (size_t)E);
    for (int e = 0; e < E; e++) f >> emb[e] >> emb_xyz[3 * e] >> emb_xyz[3 * e + 1] >> emb_xyz[3 * e + 2];
    for (int p : emb)
      if (p < 0 || p >= P) return false;
    return (bool)f;
  }
};

// what a template switch leaves for Repose: a facet and a new position for some points
void embed(InsertScene& s) {
  for (size_t e = 0; e < s.emb.size(); e++) {
    LmMapPoint& m = s.pts[s.emb[e]];
    m.SetFacet(&s.facet);
    m.SetWorldPos(&s.emb_xyz[3 * e]);
  }
}

}  // namespace

static int drive(const DriverArgs& arg) {
  dsh_ctx* ctx = arg.ctx;
  std::FILE* o = arg.out;
  InsertScene a, b;
  if (!a.read_file(arg.in[0]) || !b.read_file(arg.in[0])) return driver_bad_input(arg.in[0]);
  const std::vector<LmMapPoint*> none;
  // ---- the store way, on copy a ----
  Store store(ctx, 4, 2, 4);
  KfStore kfstore(ctx, 2);
  if (kfstore.status() != DSH_OK || !a.fill(store, &kfstore)) return driver_fail(ctx, "filling the stores");
  std::vector<LmMapPoint*> recent;
  if (!defslam_hip::ProcessNewKeyFrameStoreHIP(store, kfstore, &a.kfs[a.slot], &recent)) return driver_fail(ctx, "ProcessNewKeyFrameStoreHIP");
  a.dump(o, "store", "new", recent);
  embed(a);
  std::vector<LmMapPoint*> moved;
  std::vector<int32_t> ids, nodes;
  std::vector<double> bary;
  for (size_t e = 0; e < a.emb.size(); e++) {
    moved.push_back(&a.pts[a.emb[e]]);
    ids.push_back(a.emb[e]);
    nodes.push_back(0); nodes.push_back(1); nodes.push_back(2);
    bary.push_back(1.0); bary.push_back(0.0); bary.push_back(0.0);
  }
  if (!store.UpdatePositions<LmFrame>(moved) ||
      dsh_trackstate_set_embedding(store.handle(), (int)ids.size(), ids.data(), nodes.data(), bary.data()) != DSH_OK)
    return driver_fail(ctx, "the embedding on the store");
  if (!defslam_hip::ReposeUpkeepStoreHIP(store, kfstore)) return driver_fail(ctx, "ReposeUpkeepStoreHIP");
  a.dump(o, "store", "repose", none);

  // ---- the host way, on copy b ----
  KfStore hk(ctx, 2);
  bool okb = hk.status() == DSH_OK;
  for (size_t k = 0; okb && k < b.kfs.size(); k++) {
    int r = DSH_OK;
    okb = hk.Slot(&b.kfs[k], &r) == (int)k;
  }
  if (!okb) return driver_fail(ctx, "filling the host way's keyframe store");
  std::vector<LmMapPoint*> recent_b;
  if (defslam_hip::ProcessNewKeyFrameHIP(ctx, hk, &b.kfs[b.slot], &recent_b) != DSH_OK) return driver_fail(ctx, "ProcessNewKeyFrameHIP");
  b.dump(o, "host", "new", recent_b);
  embed(b);
  std::vector<LmMapPoint*> rep;
  for (size_t p = 0; p < b.pts.size(); p++)
    if (!b.pts[p].isBad() && b.pts[p].getFacet() && b.pts[p].GetReferenceKeyFrame()) rep.push_back(&b.pts[p]);
  if (defslam_hip::UpdateMapPointsHIP(ctx, hk, rep, DSH_MP_NORMAL_DEPTH) != DSH_OK) return driver_fail(ctx, "UpdateMapPointsHIP");
  b.dump(o, "host", "repose", none);
  return 0;
}

int main(int argc, char** argv) { return run_driver(argc, argv, 1, drive); }
