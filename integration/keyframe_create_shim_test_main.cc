// CI driver of integration/keyframe_create_hip.h: the end of one tracked frame that becomes a keyframe, its map point upkeep and its
// connections, both ways over two copies of the same stand-in objects:
//   the store way  EndTrackedFrameHIP with CreateNewKeyFrameStoreHIP in its callback, ProcessNewKeyFrameStoreHIP,
//                  UpdateConnectionsStoreHIP: the table, the snapshot and the observation walk stay on the device
//   the host way   the reference's loops written out over the host objects: CleanMatches, the constructor's PosesKeyframes loop, the
//                  outlier drop, ProcessNewKeyFrameHIP of mappoint_upkeep_hip.h, and KeyFrame::UpdateConnections over GetObservations()
//                  (the keyframes lie in one array, so pointer order is slot order)
// Every mutated field is dumped per route, floats as bit patterns; tests/test_keyframe_create_shim_gpu.py compares the routes with each
// other and with the restatement.
//   scene file: standin_store_scene.h with appearance, whose LAST keyframe is an empty placeholder: the object the new keyframe is
//   constructed in.  Then the tail "th E" / E ids of the points with a facet / "N" / N lines "point outlier octave kpn_x kpn_y d0 .. d31"
//   / "levels sf0 .." / the 16 floats of Tcw.
//   usage and exit codes: shim_driver.h
#include <cstring>
#include <fstream>

#include "keyframe_create_hip.h"
#include "keyframe_insert_hip.h"
#include "motion_model_hip.h"
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

struct CreateScene : StoreScene {
  int th = 100;
  std::vector<int> emb;
  LmFacet facet;
  LmFrame F;
  std::vector<KeyPoint> kpn;

  bool read_file(const char* path) {
    std::ifstream f(path);
    int E = 0, N = 0;
    if (!read(f) || !appearance || K < 1 || kfs[K - 1].N != 0 || !(f >> th >> E) || E < 0) return false;
    emb.resize(E);
    for (int& p : emb)
      if (!(f >> p) || p < 0 || p >= P) return false;
    for (int p : emb) pts[p].SetFacet(&facet);
    if (!(f >> N) || N < 0) return false;
    F.N = N;
    F.mvpMapPoints.assign(N, nullptr);
    F.mvbOutlier.assign(N, false);
    F.mvKeys.resize(N);
    F.mDescriptors.resize(32 * (size_t)N);
    kpn.resize(N);
    for (int i = 0; i < N; i++) {
      int p, out;
      if (!(f >> p >> out >> F.mvKeys[i].octave >> kpn[i].pt.x >> kpn[i].pt.y) || p < -1 || p >= P) return false;
      F.mvpMapPoints[i] = p >= 0 ? &pts[p] : nullptr;
      F.mvbOutlier[i] = out != 0;
      for (int b = 0; b < 32; b++) { int v; f >> v; F.mDescriptors[32 * (size_t)i + b] = (uint8_t)v; }
    }
    F.mvKeysUn = F.mvKeys;
    if (!(f >> F.mnScaleLevels) || F.mnScaleLevels < 1) return false;
    F.mvScaleFactors.resize(F.mnScaleLevels);
    for (float& s : F.mvScaleFactors) f >> s;
    float T[16];
    for (float& v : T) f >> v;
    F.SetPose(T);
    return (bool)f;
  }

  LmKeyFrame* new_kf() { return &kfs[K - 1]; }

  // KeyFrame::KeyFrame(Frame&, ..) and what DefKeyFrame's constructor adds but the PosesKeyframes loop (KeyFrame.cc:37-75, DefKeyFrame.cc:42-58)
  void construct(const LmFrame& f) {
    LmKeyFrame* kf = new_kf();
    kf->mnId = (unsigned long)(K - 1);
    kf->N = f.N;
    kf->mvKeysUn = f.mvKeysUn;
    kf->mDescriptors = f.mDescriptors;
    kf->mnScaleLevels = f.mnScaleLevels;
    kf->mvScaleFactors = f.mvScaleFactors;
    kf->mvpMapPoints = f.mvpMapPoints;
    kf->SetPose(f.mTcw);
    kf->mpKeypointNorm = kpn;                     // NormaliseKeypoints stays with the constructor: the scene brings its result
  }
};

void bits(std::FILE* o, const float* v, int n) {
  for (int i = 0; i < n; i++) {
    uint32_t u;
    std::memcpy(&u, &v[i], 4);
    std::fprintf(o, "%s%u", i ? ":" : "", u);
  }
}

// the fields the two call sites mutate beyond StoreScene::dump: the frame after the outlier drop, the centre, the connection members
void dump_more(const CreateScene& s, std::FILE* o, const char* route, const float* Ow) {
  std::fprintf(o, "%s kf frame", route);
  for (const LmMapPoint* p : s.F.mvpMapPoints) std::fprintf(o, " %d", s.id(p));
  std::fprintf(o, "\n%s kf centre ", route);
  bits(o, Ow, 3);
  std::fprintf(o, "\n");
  for (int k = 0; k < s.K; k++) {
    const LmKeyFrame& kf = s.kfs[k];
    std::fprintf(o, "%s kf conn %d %d %d |", route, k, kf.mbFirstConnection ? 1 : 0, s.slot(kf.mpParent));
    for (const auto& kv : kf.mConnectedKeyFrameWeights) std::fprintf(o, " %d:%d", s.slot(kv.first), kv.second);
    std::fprintf(o, " |");
    for (size_t i = 0; i < kf.mvpOrderedConnectedKeyFrames.size(); i++) std::fprintf(o, " %d:%d", s.slot(kf.mvpOrderedConnectedKeyFrames[i]), kf.mvOrderedWeights[i]);
    std::fprintf(o, " |");
    for (const LmKeyFrame* c : kf.mspChildrens) std::fprintf(o, " %d", s.slot(c));
    std::fprintf(o, "\n");
  }
}

}  // namespace

static int drive(const DriverArgs& arg) {
  dsh_ctx* ctx = arg.ctx;
  std::FILE* o = arg.out;
  CreateScene a, b;
  if (!a.read_file(arg.in[0]) || !b.read_file(arg.in[0])) return driver_bad_input(arg.in[0]);
  const int N = a.F.N;
  // ---- the store way, on copy a ----
  {
    Store store(ctx, 4, 2, 4);
    KfStore kfstore(ctx, 2);
    a.K -= 1;                                      // the placeholder is not in the stores yet
    const bool filled = kfstore.status() == DSH_OK && a.fill(store, &kfstore);
    a.K += 1;
    if (!filled) return driver_fail(ctx, "filling the stores");
    std::vector<int32_t> ids(a.emb.begin(), a.emb.end()), nodes;
    std::vector<double> bary;
    for (size_t e = 0; e < ids.size(); e++) {
      nodes.push_back(0); nodes.push_back(1); nodes.push_back(2);
      bary.push_back(1.0); bary.push_back(0.0); bary.push_back(0.0);
    }
    if (dsh_trackstate_set_embedding(store.handle(), (int)ids.size(), ids.data(), nodes.data(), bary.data()) != DSH_OK) return driver_fail(ctx, "the embedding on the store");
    LmKeyFrame* kf = a.new_kf();
    int slot = -1;
    if (defslam_hip::EndTrackedFrameHIP(store, a.F, [&](LmFrame& f) {
          a.construct(f);                          // DefTracking.cc:175-178: CreateNewKeyFrame, the frame still holds its outliers
          slot = defslam_hip::CreateNewKeyFrameStoreHIP(store, kfstore, f, kf);
        }) < 0 || slot != a.K - 1)
      return driver_fail(ctx, "EndTrackedFrameHIP with CreateNewKeyFrameStoreHIP");
    std::vector<LmMapPoint*> recent;
    if (!defslam_hip::ProcessNewKeyFrameStoreHIP(store, kfstore, kf, &recent)) return driver_fail(ctx, "ProcessNewKeyFrameStoreHIP");
    if (!defslam_hip::UpdateConnectionsStoreHIP(store, kf, a.th)) return driver_fail(ctx, "UpdateConnectionsStoreHIP");
    a.dump(o, "store", "kf", recent);
    float Ow[3];
    dsh_keyframe_pose_input pin;
    pin.kfdb = kfstore.db(); pin.slot = slot; pin.Tcw = nullptr;
    std::vector<int32_t> sp(N > 0 ? N : 1);
    std::vector<float> sx(3 * (size_t)(N > 0 ? N : 1));
    if (dsh_keyframe_get_centre(store.handle(), &pin, Ow) != DSH_OK || dsh_keyframe_get_snapshot(store.handle(), slot, N, sp.data(), sx.data()) != DSH_OK ||
        dsh_keyframe_surface_state(store.handle(), slot) != 1)
      return driver_fail(ctx, "reading the new keyframe back");
    dump_more(a, o, "store", Ow);
    std::fprintf(o, "store kf snap");
    for (int i = 0; i < N; i++)
      if (sp[i] >= 0) {
        std::fprintf(o, " %d:%d:", i, sp[i]);
        bits(o, &sx[3 * (size_t)i], 3);
      }
    std::fprintf(o, "\n");
  }

  // ---- the host way, on copy b ----
  LmFrame& F = b.F;
  for (int i = 0; i < N; i++) {                    // CleanMatches (DefTracking.cc:667-679)
    LmMapPoint* p = F.mvpMapPoints[i];
    if (p && p->nObs < 1) {
      F.mvpMapPoints[i] = nullptr;
      F.mvbOutlier[i] = false;
    }
  }
  b.construct(F);                                  // CreateNewKeyFrame (:175-178, :696-707)
  LmKeyFrame* kf = b.new_kf();
  for (LmMapPoint* p : kf->mvpMapPoints)           // DefKeyFrame.cc:60-74
    if (p && !p->isBad() && p->getFacet()) p->PosesKeyframes[kf] = {{p->pos[0], p->pos[1], p->pos[2]}};
  for (int i = 0; i < N; i++)                      // the outlier drop (:185-191)
    if (F.mvpMapPoints[i] && F.mvbOutlier[i]) F.mvpMapPoints[i] = nullptr;
  KfStore hk(ctx, 2);
  bool okb = hk.status() == DSH_OK;
  for (size_t k = 0; okb && k < b.kfs.size(); k++) {
    int r = DSH_OK;
    okb = hk.Slot(&b.kfs[k], &r) == (int)k;
  }
  if (!okb) return driver_fail(ctx, "filling the host way's keyframe store");
  std::vector<LmMapPoint*> recent_b;
  if (defslam_hip::ProcessNewKeyFrameHIP(ctx, hk, kf, &recent_b) != DSH_OK) return driver_fail(ctx, "ProcessNewKeyFrameHIP");
  {                                                // KeyFrame::UpdateConnections (KeyFrame.cc:326-419)
    std::map<LmKeyFrame*, int> KFcounter;
    for (LmMapPoint* pMP : kf->GetMapPointMatches()) {
      if (!pMP || pMP->isBad()) continue;
      for (const auto& ob : pMP->GetObservations())
        if (ob.first->mnId != kf->mnId) KFcounter[ob.first]++;
    }
    if (!KFcounter.empty()) {
      int nmax = 0;
      LmKeyFrame* pKFmax = nullptr;
      std::vector<std::pair<int, LmKeyFrame*>> vPairs;
      for (const auto& kc : KFcounter) {
        if (kc.second > nmax) { nmax = kc.second; pKFmax = kc.first; }
        if (kc.second >= b.th) {
          vPairs.push_back(std::make_pair(kc.second, kc.first));
          kc.first->AddConnection(kf, kc.second);
        }
      }
      if (vPairs.empty()) {
        vPairs.push_back(std::make_pair(nmax, pKFmax));
        pKFmax->AddConnection(kf, nmax);
      }
      std::sort(vPairs.begin(), vPairs.end());
      kf->mConnectedKeyFrameWeights = KFcounter;
      kf->mvpOrderedConnectedKeyFrames.clear();
      kf->mvOrderedWeights.clear();
      for (size_t i = vPairs.size(); i-- > 0;) {
        kf->mvpOrderedConnectedKeyFrames.push_back(vPairs[i].second);
        kf->mvOrderedWeights.push_back(vPairs[i].first);
      }
      if (kf->mbFirstConnection && kf->mnId != 0) {
        kf->mpParent = kf->mvpOrderedConnectedKeyFrames.front();
        kf->mpParent->AddChild(kf);
        kf->mbFirstConnection = false;
      }
    }
  }
  b.dump(o, "host", "kf", recent_b);
  dump_more(b, o, "host", kf->Ow);
  std::fprintf(o, "host kf snap");
  for (int i = 0; i < N; i++) {
    LmMapPoint* p = kf->mvpMapPoints[i];
    if (!p || !p->PosesKeyframes.count(kf)) continue;
    std::fprintf(o, " %d:%d:", i, b.id(p));
    bits(o, p->PosesKeyframes[kf].data(), 3);
  }
  std::fprintf(o, "\n");
  return 0;
}

int main(int argc, char** argv) { return run_driver(argc, argv, 1, drive); }
