// CI driver of integration/mappoint_upkeep_hip.h: keyframes and map points from a text file, then LocalMapping::ProcessNewKeyFrame's
// map point loop for a sequence of keyframes (ProcessNewKeyFrameHIP) and a DefMapPoint::Repose-style update of moved points
// (UpdateMapPointsHIP with DSH_MP_NORMAL_DEPTH), with a dump of every map point after each stage.
//   usage: mappoint_shim_test <input.txt> <output.txt> [device]
// input   levels sf[levels]; K, per keyframe "Ow[3] N bad" and N lines "octave desc[32]"; P, per point "x y z ref n (kf idx) * n";
//         S, per step "kf n id[n]" (the keyframe's mvpMapPoints, -1 = none); R, per line "point x y z"
// output  the rank of each keyframe's address (the order of std::map<KeyFrame*, size_t>), then twice (after the steps, after the
//         moves) per point "n (kf idx) * n desc[32] normal[3] max min"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <string>

#include "mappoint_upkeep_hip.h"
#include "standin_mappoint_types.h"

using namespace standin;

static void dump(FILE* out, const std::vector<std::unique_ptr<MpMapPoint>>& mps, const std::map<MpKeyFrame*, int>& id) {
  for (const auto& m : mps) {
    std::fprintf(out, "%zu", m->mObservations.size());
    for (const auto& o : m->mObservations) std::fprintf(out, " %d %zu", id.at(o.first), o.second);
    for (int b = 0; b < 32; b++) std::fprintf(out, " %d", (int)m->mDescriptor[b]);
    for (int k = 0; k < 3; k++) std::fprintf(out, " %.9g", m->mNormalVector[k]);
    std::fprintf(out, " %.9g %.9g\n", m->mfMaxDistance, m->mfMinDistance);
  }
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::ifstream in(argv[1]);
  int levels, K, P, S, R;
  in >> levels;
  std::vector<float> sf(levels);
  for (float& s : sf) in >> s;
  in >> K;
  std::vector<std::unique_ptr<MpKeyFrame>> kfs;
  std::map<MpKeyFrame*, int> id;
  for (int k = 0; k < K; k++) {
    kfs.emplace_back(new MpKeyFrame());
    MpKeyFrame& f = *kfs.back();
    int bad;
    in >> f.Ow[0] >> f.Ow[1] >> f.Ow[2] >> f.N >> bad;
    f.mbBad = bad != 0;
    f.mnScaleLevels = levels;
    f.mvScaleFactors = sf;
    f.mvKeysUn.resize(f.N);
    f.mDescriptors.resize(32 * (size_t)f.N);
    f.mvpMapPoints.assign(f.N, nullptr);
    for (int j = 0; j < f.N; j++) {
      in >> f.mvKeysUn[j].octave;
      for (int b = 0; b < 32; b++) {
        int v;
        in >> v;
        f.mDescriptors[32 * (size_t)j + b] = (uint8_t)v;
      }
    }
    id[&f] = k;
  }
  in >> P;
  std::vector<std::unique_ptr<MpMapPoint>> mps;
  for (int p = 0; p < P; p++) {
    mps.emplace_back(new MpMapPoint());
    MpMapPoint& m = *mps.back();
    int ref, n;
    in >> m.pos[0] >> m.pos[1] >> m.pos[2] >> ref >> n;
    m.mpRefKF = kfs[ref].get();
    for (int i = 0; i < n; i++) {
      int k;
      size_t j;
      in >> k >> j;
      m.AddObservation(kfs[k].get(), j);
    }
  }
  if (!in) return 3;
  const int device = argc > 3 ? std::atoi(argv[3]) : 0;
  dsh_ctx* ctx = nullptr;
  if (dsh_create(&ctx, device) != DSH_OK) return 4;
  int rc = DSH_OK;
  {
    defslam_hip::KeyFrameStoreHIP<MpKeyFrame, MpMapPoint> store(ctx, 4);
    if (store.status() != DSH_OK) { std::fprintf(stderr, "store: %s\n", dsh_last_error(ctx)); return 5; }
    FILE* out = std::fopen(argv[2], "w");
    if (!out) return 6;
    std::vector<MpKeyFrame*> by_addr;
    for (auto& f : kfs) by_addr.push_back(f.get());
    std::sort(by_addr.begin(), by_addr.end());
    for (int k = 0; k < K; k++) std::fprintf(out, "%d ", (int)(std::find(by_addr.begin(), by_addr.end(), kfs[k].get()) - by_addr.begin()));
    std::fprintf(out, "\n");
    in >> S;
    for (int s = 0; s < S && rc == DSH_OK; s++) {
      int k, n;
      in >> k >> n;
      MpKeyFrame& f = *kfs[k];
      for (int i = 0; i < n; i++) {
        int p;
        in >> p;
        f.mvpMapPoints[i] = p >= 0 ? mps[p].get() : nullptr;
      }
      std::vector<MpMapPoint*> recent;
      rc = defslam_hip::ProcessNewKeyFrameHIP(ctx, store, &f, &recent);
    }
    dump(out, mps, id);
    in >> R;
    std::vector<MpMapPoint*> moved;
    for (int r = 0; r < R; r++) {
      int p;
      in >> p;
      MpMapPoint& m = *mps[p];
      in >> m.pos[0] >> m.pos[1] >> m.pos[2];   // DefMapPoint::RecalculatePosition
      moved.push_back(&m);
    }
    if (rc == DSH_OK) rc = defslam_hip::UpdateMapPointsHIP(ctx, store, moved, DSH_MP_NORMAL_DEPTH);
    dump(out, mps, id);
    std::fclose(out);
    if (rc != DSH_OK) std::fprintf(stderr, "upkeep: status %d: %s\n", rc, dsh_last_error(ctx));
  }
  dsh_destroy(ctx);
  return rc == DSH_OK ? 0 : 1;
}
