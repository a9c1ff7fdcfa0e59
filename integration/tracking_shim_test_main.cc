// CI driver of integration/tracking_search_hip.h: a current frame, a last frame and local map points from a text file, then
// DefTracking::TrackWithMotionModel's sequence (DefTracking.cc:350-369: clear, th = 20, clear and th = 25 below 20 matches) through
// SearchByProjectionHIP and DefTracking::TrackLocalMap's search (DefTracking.cc:240) through SearchLocalPointsHIP, and a dump of
// what the reference's calls change.
//   usage: tracking_shim_test <input.txt> <output.txt> [device]
#include <cstdio>
#include <fstream>
#include <memory>
#include <string>

#include "standin_tracking_types.h"
#include "tracking_search_hip.h"

using namespace standin;

static void read_frame_camera(std::ifstream& in, TrackFrame& f, int levels, float logsf, const std::vector<float>& sf) {
  in >> f.fx >> f.fy >> f.cx >> f.cy >> f.mnMinX >> f.mnMaxX >> f.mnMinY >> f.mnMaxY;
  for (float& t : f.mTcw) in >> t;
  for (float& o : f.mOw) in >> o;
  f.mnScaleLevels = levels;
  f.mfLogScaleFactor = logsf;
  f.mvScaleFactors = sf;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::ifstream in(argv[1]);
  int levels, N, P, NL, L;
  float logsf;
  in >> levels >> logsf;
  std::vector<float> sf(levels);
  for (float& s : sf) in >> s;
  // map points: x y z nx ny nz maxd nobs bad desc[32]
  in >> P;
  std::vector<std::unique_ptr<TrackMapPoint>> mps;
  for (int p = 0; p < P; p++) {
    mps.emplace_back(new TrackMapPoint());
    TrackMapPoint& m = *mps.back();
    int bad;
    in >> m.pos[0] >> m.pos[1] >> m.pos[2] >> m.normal[0] >> m.normal[1] >> m.normal[2] >> m.mfMaxDistance >> m.nObs >> bad;
    m.bad = bad != 0;
    for (auto& b : m.desc) { int v; in >> v; b = (uint8_t)v; }
  }
  TrackFrame cur, last;
  read_frame_camera(in, cur, levels, logsf, sf);
  cur.mnId = 2;
  in >> N;   // current frame key points: x y octave desc[32]
  cur.N = N;
  cur.mvKeys.resize(N);
  cur.mvKeysUn.resize(N);
  cur.mDescriptors.resize(32 * (size_t)N);
  cur.mvpMapPoints.assign(N, nullptr);
  cur.mvbOutlier.assign(N, false);
  for (int j = 0; j < N; j++) {
    in >> cur.mvKeysUn[j].pt.x >> cur.mvKeysUn[j].pt.y >> cur.mvKeysUn[j].octave;
    cur.mvKeys[j] = cur.mvKeysUn[j];
    for (int k = 0; k < 32; k++) { int v; in >> v; cur.mDescriptors[32 * (size_t)j + k] = (uint8_t)v; }
  }
  read_frame_camera(in, last, levels, logsf, sf);
  last.mnId = 1;
  in >> L;   // last frame entries: map point id (-1: none) outlier octave
  last.N = L;
  last.mvKeys.resize(L);
  last.mvpMapPoints.assign(L, nullptr);
  last.mvbOutlier.assign(L, false);
  for (int i = 0; i < L; i++) {
    int id, outl;
    in >> id >> outl >> last.mvKeys[i].octave;
    if (id >= 0) last.mvpMapPoints[i] = mps[id].get();
    last.mvbOutlier[i] = outl != 0;
  }
  in >> NL;   // local map points, in mvpLocalMapPoints order
  std::vector<TrackMapPoint*> local(NL);
  for (auto& p : local) { int id; in >> id; p = mps[id].get(); }
  if (!in) { std::fprintf(stderr, "bad input\n"); return 2; }

  dsh_ctx* ctx = nullptr;
  if (dsh_create(&ctx, argc > 3 ? std::stoi(argv[3]) : 0) != DSH_OK) { std::fprintf(stderr, "dsh_create failed\n"); return 3; }
  // DefTracking.cc:353-369
  int th = 20;
  int n1 = defslam_hip::SearchByProjectionHIP<TrackFrame, TrackMapPoint>(ctx, cur, last, (float)th, true);
  if (n1 >= 0 && n1 < 20) {
    cur.mvpMapPoints.assign(N, nullptr);
    th = 25;
    n1 = defslam_hip::SearchByProjectionHIP<TrackFrame, TrackMapPoint>(ctx, cur, last, (float)th, true);
  }
  if (n1 < 0) { std::fprintf(stderr, "SearchByProjectionHIP: %s\n", dsh_last_error(ctx)); return 4; }
  auto id_of = [&](TrackMapPoint* p) -> int {
    for (int i = 0; i < P; i++) if (mps[i].get() == p) return i;
    return -1;
  };
  std::FILE* out = std::fopen(argv[2], "w");
  std::fprintf(out, "%d %d\n", n1, th);
  for (int j = 0; j < N; j++) std::fprintf(out, "%d ", id_of(cur.mvpMapPoints[j]));
  std::fprintf(out, "\n");
  const int n2 = defslam_hip::SearchLocalPointsHIP<TrackFrame, TrackMapPoint>(ctx, cur, local, 3.f);
  if (n2 < 0) { std::fprintf(stderr, "SearchLocalPointsHIP: %s\n", dsh_last_error(ctx)); return 5; }
  std::fprintf(out, "%d\n", n2);
  for (TrackMapPoint* p : local)
    std::fprintf(out, "%d %d %.9g %.9g %.9g %d %lu\n", p->mbTrackInView ? 1 : 0, p->mnTrackScaleLevel, p->mTrackProjX, p->mTrackProjY, p->mTrackViewCos,
                 p->nVisible, p->mnLastFrameSeen);
  for (int j = 0; j < N; j++) std::fprintf(out, "%d ", id_of(cur.mvpMapPoints[j]));
  std::fprintf(out, "\n");
  std::fclose(out);
  dsh_destroy(ctx);
  return 0;
}
