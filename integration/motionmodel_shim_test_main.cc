// CI driver of integration/motion_model_hip.h: a map and a frame (synth.write_local_map_scene) plus the template embedding of the points
// and the state after the pose optimisation (synth.write_track_close_scene).  The frame after its optimisation is ended, then two
// consecutive frames are searched and ended, both ways over two copies of the same stand-in objects, and every field the end of
// DefTracking::Track and TrackWithMotionModel mutate is dumped:
//   the store way  MapPointStoreHIP + EndTrackedFrameHIP and TrackWithMotionModelStoreHIP: nothing per map point travels
//   the host way   CleanMatches and the outlier drop over the pointer graph (DefTracking.cc:667-679, :185-191), mLastFrame as a copy of
//                  the frame, and SearchByProjectionHIP (tracking_search_hip.h) at th 20 and 25 over that copy without the bad points
//                  and the points without a facet, which DefORBmatcher's search skips (DefORBmatcher.cc:329-332)
// Frame 1 is searched at the pose before the optimisation, frame 2 at the pose after it; before frame 2 the points of the scene's
// late_bad list turn bad.  Every seventh held entry of a searched frame becomes an outlier before the frame ends.
//   usage: motionmodel_shim_test <map.txt> <close.txt> <output.txt> [device]; exit codes: shim_driver.h
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <string>

#include "motion_model_hip.h"
#include "shim_driver.h"
#include "standin_localmap_scene.h"

using namespace standin;

namespace {

// what synth.write_track_close_scene adds to the map, as far as this driver reads it
struct CloseData {
  std::vector<LmNode> nodes;
  std::vector<LmFacet> facets;                 // one per point that has one
  std::vector<int> late_bad, final_pts, outlier;
  float Tcw[16], Ow[3];
};

bool read_close(std::istream& in, LmScene& sc, CloseData& d) {
  int n_nodes = 0;
  in >> n_nodes;
  d.nodes.resize(n_nodes > 0 ? n_nodes : 0);
  for (LmNode& n : d.nodes) {
    double after[3];
    in >> n.x >> n.y >> n.z >> after[0] >> after[1] >> after[2];
  }
  d.facets.resize(sc.P);
  for (int p = 0; p < sc.P; p++) {
    int n[3], vis, found, first;
    double b[3];
    in >> n[0] >> n[1] >> n[2] >> b[0] >> b[1] >> b[2] >> vis >> found >> first;
    if (n[0] < 0) continue;
    for (int k = 0; k < 3; k++) d.facets[p].Nodes.insert(&d.nodes[n[k]]);
    sc.mps[p].facet = &d.facets[p];
    sc.mps[p].b1 = b[0]; sc.mps[p].b2 = b[1]; sc.mps[p].b3 = b[2];
  }
  int current_kf, n_late;
  in >> current_kf >> n_late;
  d.late_bad.resize(n_late > 0 ? n_late : 0);
  for (int& p : d.late_bad) in >> p;
  for (float& t : d.Tcw) in >> t;
  for (float& o : d.Ow) in >> o;
  d.final_pts.resize(sc.N); d.outlier.resize(sc.N);
  for (int j = 0; j < sc.N; j++) {
    int prev;
    in >> prev >> d.final_pts[j] >> d.outlier[j];
  }
  return (bool)in;
}

// CleanMatches, the outlier drop and mLastFrame = Frame(*mCurrentFrame) as the host does them
void host_end_frame(LmFrame& F, LmFrame& last, dsh_track_end_counts& c) {
  c = dsh_track_end_counts();
  for (int i = 0; i < F.N; i++) {
    LmMapPoint* p = F.mvpMapPoints[i];
    if (p && p->nObs < 1) {                    // Observations() of the reference returns nObs
      F.mvbOutlier[i] = false;
      F.mvpMapPoints[i] = nullptr;
      c.cleaned++;
    }
  }
  for (int i = 0; i < F.N; i++)
    if (F.mvpMapPoints[i] && F.mvbOutlier[i]) { F.mvpMapPoints[i] = nullptr; c.dropped++; }
  for (int i = 0; i < F.N; i++) c.kept += F.mvpMapPoints[i] ? 1 : 0;
  last = F;
}

// the two searches of TrackWithMotionModel through the packed call
int host_motion_model(dsh_ctx* ctx, LmFrame& F, const LmFrame& last, float& th_used) {
  LmFrame queries = last;                      // DefORBmatcher.cc:329-332: bad points and points without a facet are no queries
  for (auto& p : queries.mvpMapPoints)
    if (p && (p->isBad() || !p->getFacet())) p = nullptr;
  std::fill(F.mvpMapPoints.begin(), F.mvpMapPoints.end(), nullptr);
  th_used = 20.f;
  int n = defslam_hip::SearchByProjectionHIP<LmFrame, LmMapPoint>(ctx, F, queries, th_used, true);
  if (n >= 0 && n < 20) {
    std::fill(F.mvpMapPoints.begin(), F.mvpMapPoints.end(), nullptr);
    th_used = 25.f;
    n = defslam_hip::SearchByProjectionHIP<LmFrame, LmMapPoint>(ctx, F, queries, th_used, true);
  }
  return n;
}

void mark_outliers(LmFrame& F) {
  int held = 0;
  for (int i = 0; i < F.N; i++) {
    F.mvbOutlier[i] = false;
    if (F.mvpMapPoints[i] && ++held % 7 == 0) F.mvbOutlier[i] = true;
  }
}

void dump_frame(std::FILE* out, const LmScene& sc, const LmFrame& F) {
  for (int i = 0; i < F.N; i++) std::fprintf(out, "%d ", F.mvpMapPoints[i] ? (int)(F.mvpMapPoints[i] - sc.mps.data()) : -1);
  std::fprintf(out, "\n");
  for (int i = 0; i < F.N; i++) std::fprintf(out, "%d ", F.mvbOutlier[i] ? 1 : 0);
  std::fprintf(out, "\n");
}

}  // namespace

static int drive(const DriverArgs& arg) {
  dsh_ctx* ctx = arg.ctx;
  std::FILE* out = arg.out;
  LmScene dev, host;                        // two copies of the same objects, one per way
  CloseData dd, hd;
  for (int w = 0; w < 2; w++) {
    std::ifstream in(arg.in[0]), in2(arg.in[1]);
    LmScene& sc = w ? host : dev;
    if (!sc.read(in) || !read_close(in2, sc, w ? hd : dd)) return driver_bad_input(arg.in[0]);
  }
  const int P = dev.P, K = dev.K;
  typedef defslam_hip::MapPointStoreHIP<LmKeyFrame, LmMapPoint> Store;
  {
    Store store(ctx, 64, 2, 64);   // small on purpose: the store grows
    std::vector<LmMapPoint*> pts(P);
    for (int p = 0; p < P; p++) pts[p] = &dev.mps[p];
    bool ok = store.ok() && store.AddMapPoints<LmFrame>(pts);
    for (int k = 0; ok && k < K; k++) ok = store.AddKeyFrame(&dev.kfs[k]);
    ok = ok && store.AddObservations(dev.obs_p, dev.obs_k);
    ok = ok && store.SetEmbedding(pts, [&](LmNode* n) { return (int)(n - dd.nodes.data()); });
    if (!ok) return driver_fail(ctx, "filling the store");

    for (int w = 0; w < 2; w++) {
      LmScene& sc = w ? host : dev;
      CloseData& d = w ? hd : dd;
      float pose0[16], Ow0[3];
      std::copy(sc.cur.mTcw, sc.cur.mTcw + 16, pose0);
      std::copy(sc.cur.mOw, sc.cur.mOw + 3, Ow0);
      // frame 0 after its optimisation: the final matches, the outlier flags, the new pose
      LmFrame F = sc.cur, last;
      for (int j = 0; j < sc.N; j++) {
        F.mvpMapPoints[j] = d.final_pts[j] >= 0 ? &sc.mps[d.final_pts[j]] : nullptr;
        F.mvbOutlier[j] = d.outlier[j] != 0;
      }
      std::copy(d.Tcw, d.Tcw + 16, F.mTcw);
      std::copy(d.Ow, d.Ow + 3, F.mOw);
      for (int t = 0; t < 3; t++) {
        if (t > 0) {
          // the next frame: the same key points at the pose before (frame 1) or after (frame 2) the optimisation
          std::copy(t == 1 ? pose0 : d.Tcw, (t == 1 ? pose0 : d.Tcw) + 16, F.mTcw);
          std::copy(t == 1 ? Ow0 : d.Ow, (t == 1 ? Ow0 : d.Ow) + 3, F.mOw);
          std::fill(F.mvbOutlier.begin(), F.mvbOutlier.end(), false);
          if (t == 2)
            for (int p : d.late_bad) {
              sc.mps[p].setBadFlag();
              if (!w && !store.SetBad(&sc.mps[p])) return driver_fail(ctx, "SetBad");
            }
          float th_used = 0.f;
          const int n = w ? host_motion_model(ctx, F, last, th_used)
                          : defslam_hip::TrackWithMotionModelStoreHIP(store, F, last, true, &th_used);
          if (n < 0) { std::fprintf(stderr, "frame %d, way %d: ", t, w); return driver_fail(ctx, "search"); }
          std::fprintf(out, "%d %d\n", n, (int)th_used);
          dump_frame(out, sc, F);
          mark_outliers(F);
        }
        dsh_track_end_counts c;
        if (w) {
          host_end_frame(F, last, c);
        } else {
          if (defslam_hip::EndTrackedFrameHIP(store, F, &c) < 0) { std::fprintf(stderr, "frame %d: ", t); return driver_fail(ctx, "EndTrackedFrameHIP"); }
          last = F;                                                  // mLastFrame = Frame(*mCurrentFrame)
        }
        std::fprintf(out, "%d %d %d\n", c.cleaned, c.dropped, c.kept);
        dump_frame(out, sc, F);
      }
    }
  }
  return 0;
}

int main(int argc, char** argv) { return run_driver(argc, argv, 2, drive); }
