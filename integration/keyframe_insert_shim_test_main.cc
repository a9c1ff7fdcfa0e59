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
//   map file: P K / P lines "bad ref x y z nx ny nz maxd d0 .. d31" / K blocks "N bad Owx Owy Owz levels sf0 .." then N lines
//             "octave table d0 .. d31" / L / L lines "point kf idx live" / "slot E" / E lines "point x y z" (facet and new position)
//   usage: keyframe_insert_shim_test <map.txt> <output.txt> [device]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>

#include "anchor_pairs_hip.h"
#include "keyframe_insert_hip.h"
#include "standin_localmap_types.h"

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

struct Scene {
  std::vector<LmKeyFrame> kfs;      // one array: pointer order is slot order
  std::vector<LmMapPoint> pts;
  std::vector<int> log_p, log_k, log_i, log_live;
  int slot = 0;
  std::vector<int> emb;
  std::vector<float> emb_xyz;
  LmFacet facet;
};

bool read_scene(const char* path, Scene& s) {
  std::ifstream f(path);
  int P, K;
  if (!(f >> P >> K)) return false;
  s.pts.resize(P);
  s.kfs.resize(K);
  std::vector<int> ref(P);
  for (int p = 0; p < P; p++) {
    LmMapPoint& m = s.pts[p];
    int bad, d;
    f >> bad >> ref[p] >> m.pos[0] >> m.pos[1] >> m.pos[2] >> m.normal[0] >> m.normal[1] >> m.normal[2] >> m.mfMaxDistance;
    m.bad = bad != 0;
    for (int b = 0; b < 32; b++) { f >> d; m.desc[b] = (uint8_t)d; }
    m.mpRefKF = ref[p] >= 0 ? &s.kfs[ref[p]] : nullptr;
  }
  for (int k = 0; k < K; k++) {
    LmKeyFrame& kf = s.kfs[k];
    int bad;
    f >> kf.N >> bad >> kf.Ow[0] >> kf.Ow[1] >> kf.Ow[2] >> kf.mnScaleLevels;
    kf.bad = bad != 0;
    kf.mnId = (unsigned long)k;
    kf.mvScaleFactors.resize(kf.mnScaleLevels);
    for (int l = 0; l < kf.mnScaleLevels; l++) f >> kf.mvScaleFactors[l];
    kf.mvKeysUn.resize(kf.N);
    kf.mvpMapPoints.assign(kf.N, nullptr);
    kf.mDescriptors.resize(32 * (size_t)kf.N);
    for (int j = 0; j < kf.N; j++) {
      int t, d;
      f >> kf.mvKeysUn[j].octave >> t;
      if (t >= 0) kf.mvpMapPoints[j] = &s.pts[t];
      for (int b = 0; b < 32; b++) { f >> d; kf.mDescriptors[32 * (size_t)j + b] = (uint8_t)d; }
    }
  }
  int L, E;
  f >> L;
  s.log_p.resize(L); s.log_k.resize(L); s.log_i.resize(L); s.log_live.resize(L);
  for (int r = 0; r < L; r++) {
    f >> s.log_p[r] >> s.log_k[r] >> s.log_i[r] >> s.log_live[r];
    if (s.log_live[r]) s.pts[s.log_p[r]].AddObservation(&s.kfs[s.log_k[r]], (size_t)s.log_i[r]);
  }
  f >> s.slot >> E;
  s.emb.resize(E);
  s.emb_xyz.resize(3 * (size_t)E);
  for (int e = 0; e < E; e++) f >> s.emb[e] >> s.emb_xyz[3 * e] >> s.emb_xyz[3 * e + 1] >> s.emb_xyz[3 * e + 2];
  return (bool)f;
}

uint32_t bits(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }

void dump(FILE* o, const char* route, const char* step, Scene& s, const std::vector<LmMapPoint*>& recent) {
  std::fprintf(o, "%s %s recent", route, step);
  for (size_t i = 0; i < recent.size(); i++) std::fprintf(o, " %d", (int)(recent[i] - &s.pts[0]));
  std::fprintf(o, "\n");
  for (size_t p = 0; p < s.pts.size(); p++) {
    LmMapPoint& m = s.pts[p];
    std::fprintf(o, "%s %s pt %d %d %u %u %u %u %u", route, step, (int)p, m.nObs, bits(m.mfMaxDistance), bits(m.mfMinDistance), bits(m.normal[0]),
                 bits(m.normal[1]), bits(m.normal[2]));
    for (int b = 0; b < 32; b++) std::fprintf(o, " %d", (int)m.desc[b]);
    std::fprintf(o, " |");
    for (const auto& kv : m.mObservations) std::fprintf(o, " %d:%d", (int)(kv.first - &s.kfs[0]), (int)kv.second);
    std::fprintf(o, "\n");
  }
}

// what a template switch leaves for Repose: a facet and a new position for some points
void embed(Scene& s) {
  for (size_t e = 0; e < s.emb.size(); e++) {
    LmMapPoint& m = s.pts[s.emb[e]];
    m.SetFacet(&s.facet);
    m.SetWorldPos(&s.emb_xyz[3 * e]);
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
    KfStore kfstore(ctx, 2);
    std::vector<LmMapPoint*> all;
    for (size_t p = 0; p < a.pts.size(); p++) all.push_back(&a.pts[p]);
    bool ok = store.ok() && kfstore.status() == DSH_OK && store.AddMapPoints<LmFrame>(all);
    for (size_t k = 0; ok && k < a.kfs.size(); k++) {
      int r = DSH_OK;
      ok = store.AddKeyFrame(&a.kfs[k]) && kfstore.Slot(&a.kfs[k], &r) == (int)k;
    }
    for (size_t r = 0; ok && r < a.log_p.size(); r++) {   // the log in its order, blanked records too
      std::vector<LmMapPoint*> p(1, &a.pts[a.log_p[r]]);
      std::vector<LmKeyFrame*> k(1, &a.kfs[a.log_k[r]]);
      ok = defslam_hip::AddObservationsIndexedHIP(store, p, k, std::vector<int>(1, a.log_i[r]));
      if (ok && !a.log_live[r]) ok = store.EraseObservations(p, k);
    }
    ok = ok && defslam_hip::SetReferenceKeyFramesHIP(store, all);
    std::vector<LmMapPoint*> recent;
    ok = ok && defslam_hip::ProcessNewKeyFrameStoreHIP(store, kfstore, &a.kfs[a.slot], &recent);
    if (ok) dump(o, "store", "new", a, recent);
    if (ok) {
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
      ok = store.UpdatePositions<LmFrame>(moved) &&
           dsh_trackstate_set_embedding(store.handle(), (int)ids.size(), ids.data(), nodes.data(), bary.data()) == DSH_OK;
    }
    ok = ok && defslam_hip::ReposeUpkeepStoreHIP(store, kfstore);
    if (ok) dump(o, "store", "repose", a, std::vector<LmMapPoint*>());
    if (!ok) std::fprintf(stderr, "store way: %s\n", dsh_last_error(ctx));

    // ---- the host way, on copy b ----
    KfStore hk(ctx, 2);
    bool okb = ok && hk.status() == DSH_OK;
    for (size_t k = 0; okb && k < b.kfs.size(); k++) {
      int r = DSH_OK;
      okb = hk.Slot(&b.kfs[k], &r) == (int)k;
    }
    std::vector<LmMapPoint*> recent_b;
    okb = okb && defslam_hip::ProcessNewKeyFrameHIP(ctx, hk, &b.kfs[b.slot], &recent_b) == DSH_OK;
    if (okb) dump(o, "host", "new", b, recent_b);
    if (okb) {
      embed(b);
      std::vector<LmMapPoint*> rep;
      for (size_t p = 0; p < b.pts.size(); p++)
        if (!b.pts[p].isBad() && b.pts[p].getFacet() && b.pts[p].GetReferenceKeyFrame()) rep.push_back(&b.pts[p]);
      okb = defslam_hip::UpdateMapPointsHIP(ctx, hk, rep, DSH_MP_NORMAL_DEPTH) == DSH_OK;
    }
    if (okb) dump(o, "host", "repose", b, std::vector<LmMapPoint*>());
    if (ok && !okb) std::fprintf(stderr, "host way: %s\n", dsh_last_error(ctx));
    rc = ok && okb ? 0 : 1;
  }
  std::fclose(o);
  dsh_destroy(ctx);
  return rc;
}
