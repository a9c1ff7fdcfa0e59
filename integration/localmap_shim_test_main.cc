// CI driver of integration/local_map_hip.h: a map (points, keyframes with tables and a spanning tree, observations) and a current frame
// from a text file; the map goes into a MapPointStoreHIP, then DefTracking::TrackLocalMap's first two steps (DefTracking.cc:237-240) run
// through UpdateLocalMapHIP and SearchLocalPointsStoreHIP, and what the reference's calls change is dumped.
//   usage: localmap_shim_test <input.txt> <output.txt> [device] [timing.json reps]; exit codes: shim_driver.h
// With a timing file the frame is then repeated `reps` times both ways and the medians are written: the device path above, and the way
// the frame was done before the store existed -- UpdateLocalKeyFrames + UpdateLocalPoints on the host over the same objects
// (std::map / std::set, below) followed by SearchLocalPointsHIP, which re-packs every local point.  The host lists are also compared
// with the device's (the stand-in objects live in arrays, so pointer order is index order).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <fstream>
#include <map>
#include <set>
#include <string>

#include "local_map_hip.h"
#include "shim_driver.h"
#include "standin_localmap_scene.h"
#include "standin_localmap_types.h"

using namespace standin;

namespace {

double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v.empty() ? 0.0 : v[v.size() / 2];
}

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

static int drive(const DriverArgs& arg) {
  dsh_ctx* ctx = arg.ctx;
  std::FILE* out = arg.out;
  std::ifstream in(arg.in[0]);
  LmScene scene;
  if (!scene.read(in)) return driver_bad_input(arg.in[0]);
  const int P = scene.P, K = scene.K, R = scene.R, N = scene.N;
  std::vector<LmMapPoint>& mps = scene.mps;
  std::vector<LmKeyFrame>& kfs = scene.kfs;
  std::vector<LmMapPoint*>& obs_p = scene.obs_p;
  std::vector<LmKeyFrame*>& obs_k = scene.obs_k;
  LmFrame& cur = scene.cur;
  const std::vector<LmMapPoint*> frame0 = cur.mvpMapPoints;

  typedef defslam_hip::MapPointStoreHIP<LmKeyFrame, LmMapPoint> Store;
  {
    Store store(ctx, 64, 2, 64);   // small on purpose: the store grows
    std::vector<LmMapPoint*> pts(P);
    for (int p = 0; p < P; p++) pts[p] = &mps[p];
    bool ok = store.ok() && store.AddMapPoints<LmFrame>(pts);
    for (int k = 0; ok && k < K; k++) ok = store.AddKeyFrame(&kfs[k]);
    ok = ok && store.AddObservations(obs_p, obs_k);
    if (!ok) return driver_fail(ctx, "filling the store");

    std::vector<LmKeyFrame*> local_kfs;
    std::vector<LmMapPoint*> local_pts;
    std::vector<int32_t> votes;
    LmKeyFrame* ref_kf = nullptr;
    const int npts = defslam_hip::UpdateLocalMapHIP(store, cur, local_kfs, local_pts, ref_kf, &votes);
    if (npts < 0) return driver_fail(ctx, "UpdateLocalMapHIP");
    auto dump_frame = [&]() {
      for (int j = 0; j < N; j++) std::fprintf(out, "%d ", cur.mvpMapPoints[j] ? (int)(cur.mvpMapPoints[j] - mps.data()) : -1);
      std::fprintf(out, "\n");
    };
    std::fprintf(out, "%zu %zu %d %d\n", local_kfs.size(), votes.size(), ref_kf ? (int)(ref_kf - kfs.data()) : -1,
                 cur.mpReferenceKF ? (int)(cur.mpReferenceKF - kfs.data()) : -1);
    for (LmKeyFrame* k : local_kfs) std::fprintf(out, "%d ", (int)(k - kfs.data()));
    std::fprintf(out, "\n");
    for (int32_t v : votes) std::fprintf(out, "%d ", v);
    std::fprintf(out, "\n");
    dump_frame();
    std::fprintf(out, "%d\n", npts);
    for (LmMapPoint* p : local_pts) std::fprintf(out, "%d ", (int)(p - mps.data()));
    std::fprintf(out, "\n");
    for (const LmKeyFrame& k : kfs) std::fprintf(out, "%lu ", k.mnTrackReferenceForFrame);
    std::fprintf(out, "\n");
    for (const LmMapPoint& p : mps) std::fprintf(out, "%lu ", p.mnTrackReferenceForFrame);
    std::fprintf(out, "\n");
    const int n2 = defslam_hip::SearchLocalPointsStoreHIP(store, cur, local_pts, 3.f);
    if (n2 < 0) return driver_fail(ctx, "SearchLocalPointsStoreHIP");
    std::fprintf(out, "%d\n", n2);
    for (LmMapPoint* p : local_pts)
      std::fprintf(out, "%d %d %.9g %.9g %.9g %d %lu\n", p->mbTrackInView ? 1 : 0, p->mnTrackScaleLevel, p->mTrackProjX, p->mTrackProjY, p->mTrackViewCos,
                   p->nVisible, p->mnLastFrameSeen);
    dump_frame();
    const std::vector<LmMapPoint*> frame_end = cur.mvpMapPoints;

    // the same frame the way it was done without the store, over the same objects: equal lists, equal final frame
    std::vector<LmKeyFrame*> all_kfs(K);
    for (int k = 0; k < K; k++) all_kfs[k] = &kfs[k];
    auto fresh_frame = [&](unsigned long id) {
      cur.mvpMapPoints = frame0;
      cur.mnId = id;
    };
    fresh_frame(8);
    std::vector<LmKeyFrame*> h_kfs;
    std::vector<LmMapPoint*> h_pts;
    LmKeyFrame* h_ref = nullptr;
    host_update_local_map(cur, all_kfs, h_kfs, h_pts, h_ref);
    const int h_n = defslam_hip::SearchLocalPointsHIP<LmFrame, LmMapPoint>(ctx, cur, h_pts, 3.f);
    const int same = h_kfs == local_kfs && h_pts == local_pts && h_ref == ref_kf && h_n == n2 && cur.mvpMapPoints == frame_end;
    std::fprintf(out, "%d\n", same);

    if (arg.n_extra > 1) {
      const int reps = std::stoi(arg.extra[1]);
      std::vector<double> t_host, t_shim, t_dev_up, t_dev_search;
      unsigned long id = 100;
      for (int r = 0; r < reps + 3; r++) {   // three warm-up rounds
        fresh_frame(id++);
        double t0 = now_ms();
        host_update_local_map(cur, all_kfs, h_kfs, h_pts, h_ref);
        double t1 = now_ms();
        if (defslam_hip::SearchLocalPointsHIP<LmFrame, LmMapPoint>(ctx, cur, h_pts, 3.f) < 0) return driver_fail(ctx, "SearchLocalPointsHIP");
        double t2 = now_ms();
        fresh_frame(id++);
        double t3 = now_ms();
        if (defslam_hip::UpdateLocalMapHIP(store, cur, local_kfs, local_pts, ref_kf) < 0) return driver_fail(ctx, "UpdateLocalMapHIP");
        double t4 = now_ms();
        if (defslam_hip::SearchLocalPointsStoreHIP(store, cur, local_pts, 3.f) < 0) return driver_fail(ctx, "SearchLocalPointsStoreHIP");
        double t5 = now_ms();
        if (r >= 3) { t_host.push_back(t1 - t0); t_shim.push_back(t2 - t1); t_dev_up.push_back(t4 - t3); t_dev_search.push_back(t5 - t4); }
      }
      std::FILE* tj = std::fopen(arg.extra[0], "w");
      std::fprintf(tj, "{\"reps\": %d, \"keyframes\": %d, \"points\": %d, \"observations\": %d, \"frame_keypoints\": %d, \"local_points\": %zu, "
                   "\"host_update_ms\": %.4f, \"host_repack_search_ms\": %.4f, \"store_update_ms\": %.4f, \"store_search_ms\": %.4f}\n",
                   reps, K, P, R, N, local_pts.size(), median(t_host), median(t_shim), median(t_dev_up), median(t_dev_search));
      std::fclose(tj);
    }
  }
  return 0;
}

int main(int argc, char** argv) { return run_driver(argc, argv, 1, drive); }
