// CI driver of integration/track_close_hip.h: a map and a frame (synth.write_local_map_scene) plus the template embedding of the points
// and the state after the pose optimisation (synth.write_track_close_scene).  Two frames are tracked both ways over two copies of the
// same stand-in objects, and every field the end of DefTracking::TrackLocalMap and LocalMapping::MapPointCulling mutate is dumped:
//   the device way  MapPointStoreHIP + UpdateLocalMapHIP + SearchLocalPointsStoreHIP, then CloseTrackedFrameHIP and MapPointCullingHIP
//   the host way    what the frame did before: UpdateLocalMap on the host, SearchLocalPointsHIP, DefMapPoint::RecalculatePosition of every
//                   point with a facet (and, for the timing, dsh_mpdb_update_points of all of them), the loops of
//                   DefTracking.cc:253-319 and LocalMapping.cc:173-199 over the pointer graph
//   usage: trackclose_shim_test <map.txt> <close.txt> <output.txt> [device] [timing.json reps]; exit codes: shim_driver.h
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <list>
#include <string>

#include "shim_driver.h"
#include "standin_localmap_scene.h"
#include "track_close_hip.h"

using namespace standin;

namespace {

// what synth.write_track_close_scene adds to the map
struct CloseData {
  int n_nodes = 0, current_kf = 0;
  std::vector<LmNode> nodes, nodes_after;
  std::vector<LmFacet> facets;                 // one per point that has one
  std::vector<int> late_bad, prev, final_pts, outlier;
  float Tcw[16], Ow[3];
};

bool read_close(std::istream& in, LmScene& sc, CloseData& d, bool fill) {
  in >> d.n_nodes;
  d.nodes.resize(d.n_nodes);
  d.nodes_after.resize(d.n_nodes);
  for (int n = 0; n < d.n_nodes; n++)
    in >> d.nodes[n].x >> d.nodes[n].y >> d.nodes[n].z >> d.nodes_after[n].x >> d.nodes_after[n].y >> d.nodes_after[n].z;
  d.facets.resize(sc.P);
  for (int p = 0; p < sc.P; p++) {
    int n[3], vis, found, first;
    double b[3];
    in >> n[0] >> n[1] >> n[2] >> b[0] >> b[1] >> b[2] >> vis >> found >> first;
    if (!fill) continue;
    LmMapPoint& m = sc.mps[p];
    m.nVisible = vis; m.mnFound = found; m.mnFirstKFid = first;
    if (n[0] >= 0) {
      for (int k = 0; k < 3; k++) d.facets[p].Nodes.insert(&d.nodes[n[k]]);
      m.facet = &d.facets[p];
      m.b1 = b[0]; m.b2 = b[1]; m.b3 = b[2];
    }
  }
  int n_late;
  in >> d.current_kf >> n_late;
  d.late_bad.resize(n_late);
  for (int& p : d.late_bad) in >> p;
  for (float& t : d.Tcw) in >> t;
  for (float& o : d.Ow) in >> o;
  d.prev.resize(sc.N); d.final_pts.resize(sc.N); d.outlier.resize(sc.N);
  for (int j = 0; j < sc.N; j++) in >> d.prev[j] >> d.final_pts[j] >> d.outlier[j];
  return (bool)in;
}

void hold(LmScene& sc, const std::vector<int>& ids, unsigned long frame_id) {
  for (int j = 0; j < sc.N; j++) sc.cur.mvpMapPoints[j] = ids[j] >= 0 ? &sc.mps[ids[j]] : nullptr;
  sc.cur.mnId = frame_id;
}

// the frame after the optimisation: the final matches, the outlier flags, the new pose, the moved nodes
void after_optimisation(LmScene& sc, CloseData& d) {
  for (int j = 0; j < sc.N; j++) {
    sc.cur.mvpMapPoints[j] = d.final_pts[j] >= 0 ? &sc.mps[d.final_pts[j]] : nullptr;
    sc.cur.mvbOutlier[j] = d.outlier[j] != 0;
  }
  std::copy(d.Tcw, d.Tcw + 16, sc.cur.mTcw);
  std::copy(d.Ow, d.Ow + 3, sc.cur.mOw);
  for (int n = 0; n < d.n_nodes; n++) d.nodes[n] = d.nodes_after[n];            // updateNodes (DefOptimizer.cc:570)
}

// Frame::isInFrustum(pMP, 0.5) (Frame.cc:338-390) with OpenCV's arithmetic as include/defslam_hip.h states it, what it reads only
bool host_in_frustum(const LmFrame& F, const LmMapPoint& m) {
  float Pc[3];
  for (int k = 0; k < 3; k++) {
    const float s = F.mTcw[4 * k] * m.pos[0] + F.mTcw[4 * k + 1] * m.pos[1] + F.mTcw[4 * k + 2] * m.pos[2];
    Pc[k] = (float)((double)s + (double)F.mTcw[4 * k + 3]);
  }
  if (Pc[2] < 0.0f) return false;
  const float invz = 1.0f / Pc[2];
  const float u = F.fx * Pc[0] * invz + F.cx, v = F.fy * Pc[1] * invz + F.cy;
  if (u != u || v != v) return false;
  if (u < F.mnMinX || u > F.mnMaxX || v < F.mnMinY || v > F.mnMaxY) return false;
  const float PO[3] = {m.pos[0] - F.mOw[0], m.pos[1] - F.mOw[1], m.pos[2] - F.mOw[2]};
  const float dist = (float)std::sqrt((double)PO[0] * (double)PO[0] + (double)PO[1] * (double)PO[1] + (double)PO[2] * (double)PO[2]);
  const double dot = (double)PO[0] * (double)m.normal[0] + (double)PO[1] * (double)m.normal[1] + (double)PO[2] * (double)m.normal[2];
  return !((float)(dot / (double)dist) < 0.5f);
}

// DefOptimizer.cc:568-576 (with repose) and DefTracking.cc:253-319 over the objects
void host_close(LmScene& sc, const std::vector<LmMapPoint*>& reference_points, bool only_tracking, dsh_track_close_counts& c, bool repose = true) {
  c = dsh_track_close_counts();
  for (LmMapPoint& m : sc.mps)                                       // Map::GetAllMapPoints holds no bad point
    if (repose && !m.isBad() && m.getFacet()) { m.RecalculatePosition(); c.n_moved++; }
  LmFrame& F = sc.cur;
  for (int i = 0; i < F.N; i++) {
    LmMapPoint* p = F.mvpMapPoints[i];
    if (!p) continue;
    if (!F.mvbOutlier[i]) {
      p->IncreaseFound();
      if (!only_tracking) {
        if (p->nObs > 0) {                                           // Observations() of the reference returns nObs
          c.matches_inliers++;
          if (p->getFacet()) c.to_match_local++;
        }
      } else {
        c.matches_inliers++;
      }
    } else {
      c.matches_outliers++;
    }
  }
  for (LmMapPoint* p : reference_points) {
    if (!p || p->isBad()) continue;
    if (p->getFacet() && host_in_frustum(F, *p)) c.local_map_points++;
  }
  for (int i = 0; i < F.N; i++) {
    LmMapPoint* p = F.mvpMapPoints[i];
    if (!p || p->isBad()) continue;
    c.observed++;
    if (!F.mvbOutlier[i]) c.inliers++;
    else c.outliers++;
  }
}

int host_culling(std::list<LmMapPoint*>& recent, unsigned long nCurrentKFid) {
  int n_bad = 0;
  auto lit = recent.begin();
  while (lit != recent.end()) {
    LmMapPoint* p = *lit;
    if (p->isBad()) lit = recent.erase(lit);
    else if (p->GetFoundRatio() < 0.40f) { n_bad++; p->setBadFlag(); lit = recent.erase(lit); }
    else if (((int)nCurrentKFid - (int)p->mnFirstKFid) >= 3) lit = recent.erase(lit);
    else lit++;
  }
  return n_bad;
}

std::list<LmMapPoint*> recent_list(LmScene& sc) {                    // every third point: mlpRecentAddedMapPoints
  std::list<LmMapPoint*> l;
  for (int p = 0; p < sc.P; p += 3) l.push_back(&sc.mps[p]);
  return l;
}

void dump(std::FILE* out, LmScene& sc, const dsh_track_close_counts& c, int n_bad, const std::list<LmMapPoint*>& recent) {
  std::fprintf(out, "%d %d %d %d %d %d %d %d %d %zu\n", c.matches_inliers, c.matches_outliers, c.to_match_local, c.observed, c.inliers, c.outliers,
               c.local_map_points, c.n_moved, n_bad, recent.size());
  for (LmMapPoint* p : recent) std::fprintf(out, "%d ", (int)(p - sc.mps.data()));
  std::fprintf(out, "\n");
  for (const LmMapPoint& m : sc.mps)
    std::fprintf(out, "%.9g %.9g %.9g %d %d %d %d\n", m.pos[0], m.pos[1], m.pos[2], m.mnFound, m.nVisible, m.nObs, m.bad ? 1 : 0);
}

double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v.empty() ? 0.0 : v[v.size() / 2];
}

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

static int drive(const DriverArgs& arg) {
  dsh_ctx* ctx = arg.ctx;
  std::FILE* out = arg.out;
  LmScene dev, host;                        // two copies of the same objects, one per way
  CloseData dd, hd;
  for (int w = 0; w < 2; w++) {
    std::ifstream in(arg.in[0]), in2(arg.in[1]);
    LmScene& sc = w ? host : dev;
    if (!sc.read(in) || !read_close(in2, sc, w ? hd : dd, true)) return driver_bad_input(arg.in[0]);
  }
  const int P = dev.P, K = dev.K, N = dev.N;
  std::vector<int> frame0(N);
  for (int j = 0; j < N; j++) frame0[j] = dev.cur.mvpMapPoints[j] ? (int)(dev.cur.mvpMapPoints[j] - dev.mps.data()) : -1;
  typedef defslam_hip::MapPointStoreHIP<LmKeyFrame, LmMapPoint> Store;
  {
    // ---- the device way ----
    Store store(ctx, 64, 2, 64);   // small on purpose: the store grows
    std::vector<LmMapPoint*> pts(P);
    std::vector<int32_t> ids(P), vis(P), fnd(P);
    for (int p = 0; p < P; p++) { pts[p] = &dev.mps[p]; ids[p] = p; vis[p] = dev.mps[p].nVisible; fnd[p] = dev.mps[p].mnFound; }
    bool ok = store.ok() && store.AddMapPoints<LmFrame>(pts);
    for (int k = 0; ok && k < K; k++) ok = store.AddKeyFrame(&dev.kfs[k]);
    ok = ok && store.AddObservations(dev.obs_p, dev.obs_k);
    ok = ok && dsh_trackstate_set_counters(store.handle(), P, ids.data(), vis.data(), fnd.data()) == DSH_OK;   // a loaded map
    ok = ok && store.SetEmbedding(pts, [&](LmNode* n) { return (int)(n - dd.nodes.data()); });
    if (!ok) return driver_fail(ctx, "filling the store");
    std::vector<LmKeyFrame*> local_kfs;
    std::vector<LmMapPoint*> local_pts;
    LmKeyFrame* ref_kf = nullptr;
    hold(dev, dd.prev, 7);                                           // the previous frame: its list becomes the reference list
    if (defslam_hip::UpdateLocalMapHIP(store, dev.cur, local_kfs, local_pts, ref_kf) < 0) return driver_fail(ctx, "UpdateLocalMapHIP");
    for (int p : dd.late_bad) { dev.mps[p].setBadFlag(); store.SetBad(&dev.mps[p]); }
    hold(dev, frame0, 8);
    if (defslam_hip::UpdateLocalMapHIP(store, dev.cur, local_kfs, local_pts, ref_kf) < 0) return driver_fail(ctx, "UpdateLocalMapHIP");
    if (defslam_hip::SearchLocalPointsStoreHIP(store, dev.cur, local_pts, 3.f) < 0) return driver_fail(ctx, "SearchLocalPointsStoreHIP");
    after_optimisation(dev, dd);
    std::vector<LmNode*> nodes(dd.n_nodes);
    for (int n = 0; n < dd.n_nodes; n++) nodes[n] = &dd.nodes[n];
    dsh_track_close_counts dc;
    if (!defslam_hip::CloseTrackedFrameHIP(store, dev.cur, nodes, false, dc)) return driver_fail(ctx, "CloseTrackedFrameHIP");
    std::list<LmMapPoint*> d_recent = recent_list(dev);
    const int d_bad = defslam_hip::MapPointCullingHIP(store, d_recent, (unsigned long)dd.current_kf);
    if (d_bad < 0) return driver_fail(ctx, "MapPointCullingHIP");
    dump(out, dev, dc, d_bad, d_recent);
    // the store's own counters and positions
    std::vector<int32_t> s_vis(P), s_fnd(P), s_obs(P);
    std::vector<float> s_xyz(3 * (size_t)P);
    if (dsh_trackstate_get(store.handle(), P, ids.data(), s_vis.data(), s_fnd.data(), s_obs.data(), s_xyz.data()) != DSH_OK) return driver_fail(ctx, "dsh_trackstate_get");
    for (int p = 0; p < P; p++) std::fprintf(out, "%.9g %.9g %.9g %d %d %d\n", s_xyz[3 * p], s_xyz[3 * p + 1], s_xyz[3 * p + 2], s_fnd[p], s_vis[p], s_obs[p]);

    // ---- the host way, over the second copy ----
    std::vector<LmKeyFrame*> all_kfs(K), h_kfs;
    for (int k = 0; k < K; k++) all_kfs[k] = &host.kfs[k];
    std::vector<LmMapPoint*> h_pts, h_ref_pts;
    LmKeyFrame* h_ref = nullptr;
    hold(host, hd.prev, 7);
    host_update_local_map(host.cur, all_kfs, h_kfs, h_pts, h_ref);
    for (int p : hd.late_bad) host.mps[p].setBadFlag();
    hold(host, frame0, 8);
    h_ref_pts = h_pts;                                               // Tracking.cc:1475: SetReferenceMapPoints before the rebuild
    host_update_local_map(host.cur, all_kfs, h_kfs, h_pts, h_ref);
    if (defslam_hip::SearchLocalPointsHIP<LmFrame, LmMapPoint>(ctx, host.cur, h_pts, 3.f) < 0) return driver_fail(ctx, "SearchLocalPointsHIP");
    after_optimisation(host, hd);
    dsh_track_close_counts hc;
    host_close(host, h_ref_pts, false, hc);
    std::list<LmMapPoint*> h_recent = recent_list(host);
    const int h_bad = host_culling(h_recent, (unsigned long)hd.current_kf);
    dump(out, host, hc, h_bad, h_recent);

    if (arg.n_extra > 1) {
      // medians of closing the frame both ways (the counters drift with the repeats; the work per call does not)
      const int reps = std::stoi(arg.extra[1]);
      std::vector<LmMapPoint*> facet_pts;
      for (LmMapPoint& m : host.mps)
        if (!m.isBad() && m.getFacet()) facet_pts.push_back(&m);
      Store parent(ctx, P, K, 64);                                   // the parent's store: positions are uploaded per frame
      std::vector<LmMapPoint*> hpts(P);
      for (int p = 0; p < P; p++) hpts[p] = &host.mps[p];
      if (!parent.ok() || !parent.AddMapPoints<LmFrame>(hpts)) return driver_fail(ctx, "the parent's store");
      std::vector<double> t_dev, t_host_repose, t_host_upload, t_host_loops;
      for (int r = 0; r < reps + 3; r++) {   // three warm-up rounds
        double t0 = now_ms();
        if (!defslam_hip::CloseTrackedFrameHIP(store, dev.cur, nodes, false, dc)) return driver_fail(ctx, "CloseTrackedFrameHIP");
        double t1 = now_ms();
        for (LmMapPoint* m : facet_pts) m->RecalculatePosition();
        double t2 = now_ms();
        if (!parent.UpdatePositions<LmFrame>(facet_pts)) return driver_fail(ctx, "UpdatePositions");
        double t3 = now_ms();
        host_close(host, h_ref_pts, false, hc, false);   // the loops alone: the repose was timed above
        double t4 = now_ms();
        if (r >= 3) { t_dev.push_back(t1 - t0); t_host_repose.push_back(t2 - t1); t_host_upload.push_back(t3 - t2); t_host_loops.push_back(t4 - t3); }
      }
      std::FILE* tj = std::fopen(arg.extra[0], "w");
      std::fprintf(tj, "{\"reps\": %d, \"points\": %d, \"facet_points\": %zu, \"frame_keypoints\": %d, \"reference_points\": %zu, "
                   "\"device_close_ms\": %.4f, \"host_repose_ms\": %.4f, \"host_upload_ms\": %.4f, \"host_loops_ms\": %.4f}\n",
                   reps, P, facet_pts.size(), N, h_ref_pts.size(), median(t_dev), median(t_host_repose), median(t_host_upload), median(t_host_loops));
      std::fclose(tj);
    }
  }
  return 0;
}

int main(int argc, char** argv) { return run_driver(argc, argv, 2, drive); }
