// CI driver of integration/template_switch_hip.h: a map (synth.write_local_map_scene) plus what DefLocalMapping::updateTemplate reads of
// the reference keyframe and the keyframe store's side of every keyframe (synth.write_template_switch_scene).  One template switch is
// run both ways over two copies of the same stand-in objects, and every field it mutates is dumped:
//   the device way  MapPointStoreHIP + KeyFrameStoreHIP, NeedNewTemplateHIP, UpdateTemplateHIP
//   the host way    DefLocalMapping::needNewTemplate and CreateNewMapPoints over the pointer graph with the occupancy mask as an image,
//                   UpdateNormalAndDepth of the new points, then the embedding with the library's host routine dsh_template_embed,
//                   SetFacet / SetCoordinates / RecalculatePosition
// Both use the template the caller builds first: dsh_surface_vertices -> the regular triangulation -> dsh_template_build.
//   usage: tmplswitch_shim_test <map.txt> <switch.txt> <output.txt> [device]; exit codes: shim_driver.h
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <deque>
#include <fstream>
#include <map>
#include <string>

#include "shim_driver.h"
#include "standin_localmap_scene.h"
#include "template_switch_hip.h"

using namespace standin;

namespace {

struct SwitchData {
  int ref = 0, xs = 0, ys = 0;
  dsh_bbs bbs;
  std::vector<double> ctrl;
};

// what synth.write_template_switch_scene adds to the map
bool read_switch(std::istream& in, LmScene& sc, SwitchData& d) {
  int rows, cols, levels;
  in >> d.ref >> rows >> cols >> d.xs >> d.ys;
  LmKeyFrame& r = sc.kfs[d.ref];
  r.rows = rows; r.cols = cols;
  for (float& t : r.Twc) in >> t;
  in >> d.bbs.umin >> d.bbs.umax >> d.bbs.nptsu >> d.bbs.vmin >> d.bbs.vmax >> d.bbs.nptsv >> d.bbs.valdim;
  d.ctrl.resize((size_t)d.bbs.nptsu * d.bbs.nptsv);
  for (double& c : d.ctrl) in >> c;
  in >> levels;
  std::vector<float> sf(levels);
  for (float& s : sf) in >> s;
  for (LmKeyFrame& k : sc.kfs) {
    k.N = (int)k.mvpMapPoints.size();
    k.mnScaleLevels = levels;
    k.mvScaleFactors = sf;
    in >> k.Ow[0] >> k.Ow[1] >> k.Ow[2];
    k.mvKeysUn.resize(k.N);
    k.mDescriptors.resize(32 * (size_t)k.N);
    for (int j = 0; j < k.N; j++) {
      in >> k.mvKeysUn[j].octave;
      k.mvKeysUn[j].pt.x = k.mvKeysUn[j].pt.y = 0.f;
      for (int b = 0; b < 32; b++) { int v; in >> v; k.mDescriptors[32 * (size_t)j + b] = (uint8_t)v; }
    }
  }
  r.surface_points.resize(3 * (size_t)r.N);
  for (int j = 0; j < r.N; j++)
    in >> r.mvKeysUn[j].pt.x >> r.mvKeysUn[j].pt.y >> r.surface_points[3 * j] >> r.surface_points[3 * j + 1] >> r.surface_points[3 * j + 2];
  return (bool)in;
}

// the template as objects: nodes in index order (pointer order is index order), the facets of the regular triangulation
struct Mesh {
  std::vector<LmNode> nodes;
  std::vector<LmFacet> facets;
  std::vector<int32_t> tri;
  std::map<std::array<int, 3>, LmFacet*> by_nodes;
  void build(const std::vector<double>& xyz, int xs, int ys) {
    nodes.resize((size_t)xs * ys);
    for (size_t n = 0; n < nodes.size(); n++) { nodes[n].x = xyz[3 * n]; nodes[n].y = xyz[3 * n + 1]; nodes[n].z = xyz[3 * n + 2]; }
    const int rows = xs, cols = ys;   // node id = col + cols * row (TriangularMesh.cc:92-107)
    for (int j = 0; j < rows - 1; j++)
      for (int i = 0; i < cols - 1; i++) {
        const int a[6] = {i + cols * j, i + cols * j + 1, cols * (j + 1) + i, i + cols * j + 1, cols * (j + 1) + i, cols * (j + 1) + i + 1};
        tri.insert(tri.end(), a, a + 6);
      }
    facets.resize(tri.size() / 3);
    for (size_t f = 0; f < facets.size(); f++) {
      std::array<int, 3> key = {{tri[3 * f], tri[3 * f + 1], tri[3 * f + 2]}};
      std::sort(key.begin(), key.end());
      for (int n : key) facets[f].Nodes.insert(&nodes[n]);
      by_nodes[key] = &facets[f];
    }
  }
  LmFacet* facet_of(int a, int b, int c) {
    std::array<int, 3> key = {{a, b, c}};
    std::sort(key.begin(), key.end());
    const auto it = by_nodes.find(key);
    return it == by_nodes.end() ? nullptr : it->second;
  }
};

int reflect101(int p, int n) { return p < 0 ? -p : (p >= n ? 2 * (n - 1) - p : p); }

// the mask of DefLocalMapping.cc:245-271 / :359-383 as an image: filter2D with a k x k box of ones, anchor k / 2, BORDER_REFLECT_101,
// then threshold > 1 -- a pixel is set when its reflected window holds a held pixel
std::vector<uint8_t> host_mask(LmKeyFrame& kf) {
  std::vector<uint8_t> src((size_t)kf.rows * kf.cols, 0), mask(src.size(), 0);
  for (int i = 0; i < kf.N; i++) {
    LmMapPoint* p = kf.mvpMapPoints[i];
    if (p && !p->isBad()) src[(size_t)(int)kf.mvKeysUn[i].pt.y * kf.cols + (int)kf.mvKeysUn[i].pt.x] = 255;
  }
  const int k = kf.cols / 20, a = k / 2;
  for (int y = 0; y < kf.rows; y++)
    for (int x = 0; x < kf.cols; x++) {
      bool any = false;
      for (int dy = -a; dy < k - a && !any; dy++)
        for (int dx = -a; dx < k - a && !any; dx++) any = src[(size_t)reflect101(y + dy, kf.rows) * kf.cols + reflect101(x + dx, kf.cols)] != 0;
      mask[(size_t)y * kf.cols + x] = any ? 255 : 0;
    }
  return mask;
}

int host_need_new_template(LmKeyFrame& kf) {
  const std::vector<uint8_t> mask = host_mask(kf);
  int newPoints = 0;
  for (int i = 0; i < kf.N; i++)
    if (!kf.mvpMapPoints[i] && !mask[(size_t)(int)kf.mvKeysUn[i].pt.y * kf.cols + (int)kf.mvKeysUn[i].pt.x]) newPoints++;
  return newPoints;
}

void to_world(const float* T, const float* s, float* w) {
  for (int r = 0; r < 3; r++) {
    volatile float acc = T[4 * r] * s[0];     // every product and sum rounded to float32, left to right
    volatile float t = T[4 * r + 1] * s[1];
    acc = acc + t;
    t = T[4 * r + 2] * s[2];
    acc = acc + t;
    t = T[4 * r + 3] * 1.0f;
    acc = acc + t;
    w[r] = acc;
  }
}

// MapPoint::UpdateNormalAndDepth with one observation, the arithmetic include/defslam_hip.h states for dsh_mappoint_update
void host_normal_and_depth(LmMapPoint& m, LmKeyFrame& kf, int idx) {
  float n[3];
  for (int k = 0; k < 3; k++) n[k] = m.pos[k] - kf.Ow[k];
  const double nrm = std::sqrt((double)n[0] * (double)n[0] + (double)n[1] * (double)n[1] + (double)n[2] * (double)n[2]);
  const float alpha = (float)(1.0 / nrm);
  for (int k = 0; k < 3; k++) {
    volatile float t = n[k] * alpha;
    volatile float s = t + 0.0f;
    m.normal[k] = s + 0.0f;
  }
  const float dist = (float)nrm;
  volatile float mx = dist * kf.mvScaleFactors[kf.mvKeysUn[idx].octave];
  m.mfMaxDistance = mx;
  m.mfMinDistance = mx / kf.mvScaleFactors[kf.mnScaleLevels - 1];
  m.mpRefKF = &kf;
}

// DefLocalMapping::updateTemplate (:145-147) over the objects; `all` are the map's points in creation order, new ones are appended
bool host_update_template(dsh_ctx* ctx, LmKeyFrame& kf, std::vector<LmMapPoint*>& all, std::deque<LmMapPoint>& fresh, Mesh& mesh, dsh_template_switch_counts& c) {
  c = dsh_template_switch_counts();
  for (LmMapPoint* p : all)
    if (!p->isBad()) p->SetFacet(nullptr);                           // DefMap::clearTemplate: the map holds no bad point
  const std::vector<uint8_t> mask = host_mask(kf);
  c.first_id = (int32_t)all.size();
  for (int i = 0; i < kf.N; i++) {                                   // :273-345
    LmMapPoint* pMP = kf.mvpMapPoints[i];
    float x3w[3];
    if (pMP) {
      if (pMP->isBad()) continue;
      to_world(kf.Twc, &kf.surface_points[3 * (size_t)i], x3w);
      pMP->SetWorldPos(x3w);
      c.n_moved++;
    } else {
      if (mask[(size_t)(int)kf.mvKeysUn[i].pt.y * kf.cols + (int)kf.mvKeysUn[i].pt.x]) { c.n_masked++; continue; }
      to_world(kf.Twc, &kf.surface_points[3 * (size_t)i], x3w);
      fresh.emplace_back();
      pMP = &fresh.back();
      pMP->SetWorldPos(x3w);
      pMP->nVisible = 1;
      pMP->AddObservation(&kf, (size_t)i);
      kf.addMapPoint(pMP, (size_t)i);
      std::copy(&kf.mDescriptors[32 * (size_t)i], &kf.mDescriptors[32 * (size_t)i] + 32, pMP->desc);   // one observation elects its row
      host_normal_and_depth(*pMP, kf, i);
      all.push_back(pMP);
      c.n_new++;
    }
  }
  c.n_points = (int32_t)all.size();
  std::vector<LmMapPoint*> good;
  for (LmMapPoint* p : all)
    if (!p->isBad()) good.push_back(p);
  const int G = (int)good.size();
  std::vector<float> pts(3 * (size_t)G), bary(3 * (size_t)G);
  std::vector<int32_t> fid(G), nodes(3 * (size_t)G);
  for (int g = 0; g < G; g++) std::copy(good[g]->pos, good[g]->pos + 3, &pts[3 * (size_t)g]);
  if (G > 0 && dsh_template_embed(ctx, G, pts.data(), fid.data(), nodes.data(), bary.data()) != DSH_OK) return false;
  for (int g = 0; g < G; g++) {
    if (fid[g] < 0) continue;
    int order[3] = {0, 1, 2};
    std::sort(order, order + 3, [&](int a, int b) { return nodes[3 * g + a] < nodes[3 * g + b]; });
    good[g]->SetFacet(mesh.facet_of(nodes[3 * g], nodes[3 * g + 1], nodes[3 * g + 2]));
    good[g]->SetCoordinates((double)bary[3 * g + order[0]], (double)bary[3 * g + order[1]], (double)bary[3 * g + order[2]]);
    good[g]->RecalculatePosition();
    c.n_embedded++;
  }
  return true;
}

void dump(std::FILE* out, int need, const dsh_template_switch_counts& c, const std::vector<LmMapPoint*>& all, LmKeyFrame& kf, Mesh& mesh) {
  std::fprintf(out, "%d %d %d %d %d %d %d\n", need, c.n_new, c.first_id, c.n_moved, c.n_masked, c.n_embedded, c.n_points);
  for (LmMapPoint* m : all) {
    std::fprintf(out, "%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g", m->pos[0], m->pos[1], m->pos[2], m->normal[0], m->normal[1], m->normal[2], m->mfMaxDistance,
                 m->mfMinDistance);
    for (uint8_t b : m->desc) std::fprintf(out, " %d", (int)b);
    int n[3] = {-1, -1, -1}, k = 0;
    if (m->getFacet())
      for (LmNode* nd : m->getFacet()->getNodes()) n[k++] = (int)(nd - mesh.nodes.data());
    const bool f = m->getFacet() != nullptr;
    std::fprintf(out, " %d %d %d %d %d %d %.17g %.17g %.17g\n", m->nObs, m->bad ? 1 : 0, m->mObservations.count(&kf) ? (int)m->mObservations[&kf] : -1, n[0], n[1], n[2],
                 f ? m->b1 : 0.0, f ? m->b2 : 0.0, f ? m->b3 : 0.0);
  }
  std::map<LmMapPoint*, int> id;
  for (size_t p = 0; p < all.size(); p++) id[all[p]] = (int)p;
  for (LmMapPoint* p : kf.mvpMapPoints) std::fprintf(out, "%d ", p ? id[p] : -1);
  std::fprintf(out, "\n");
}

}  // namespace

static int drive(const DriverArgs& arg) {
  dsh_ctx* ctx = arg.ctx;
  std::FILE* out = arg.out;
  LmScene dev, host;                        // two copies of the same objects, one per way
  SwitchData dd, hd;
  for (int w = 0; w < 2; w++) {
    std::ifstream in(arg.in[0]), in2(arg.in[1]);
    LmScene& sc = w ? host : dev;
    if (!sc.read(in) || !read_switch(in2, sc, w ? hd : dd)) return driver_bad_input(arg.in[0]);
  }
  const int P = dev.P, K = dev.K;
  {
    // the caller's side of createTemplate: the vertices, the triangulation, the template constants
    dsh_surface_grid g;
    g.ctx = ctx; g.bbs = &dd.bbs; g.depth_ctrl = dd.ctrl.data(); g.Twc = dev.kfs[dd.ref].Twc; g.xs = dd.xs; g.ys = dd.ys;
    std::vector<double> xyz(3 * (size_t)dd.xs * dd.ys);
    if (dsh_surface_vertices(&g, xyz.data()) != DSH_OK) return driver_fail(ctx, "dsh_surface_vertices");
    Mesh mesh;
    mesh.build(xyz, dd.xs, dd.ys);
    if (dsh_template_build(ctx, (int)mesh.nodes.size(), xyz.data(), (int)mesh.facets.size(), mesh.tri.data()) != DSH_OK) return driver_fail(ctx, "dsh_template_build");

    // ---- the device way ----
    typedef defslam_hip::MapPointStoreHIP<LmKeyFrame, LmMapPoint> Store;
    Store store(ctx, 64, 2, 64);   // small on purpose: the store grows
    defslam_hip::KeyFrameStoreHIP<LmKeyFrame, LmMapPoint> kfstore(ctx, 1);
    std::vector<LmMapPoint*> pts(P);
    for (int p = 0; p < P; p++) pts[p] = &dev.mps[p];
    bool ok = store.ok() && kfstore.status() == DSH_OK && store.AddMapPoints<LmFrame>(pts);
    int rc = DSH_OK;
    for (int k = 0; ok && k < K; k++) ok = store.AddKeyFrame(&dev.kfs[k]) && kfstore.Slot(&dev.kfs[k], &rc) == k;
    ok = ok && store.AddObservations(dev.obs_p, dev.obs_k);
    if (!ok) return driver_fail(ctx, "filling the stores");
    LmKeyFrame* ref = &dev.kfs[dd.ref];
    const int d_need = defslam_hip::NeedNewTemplateHIP(store, ref);
    if (d_need < 0) return driver_fail(ctx, "NeedNewTemplateHIP");
    std::deque<LmMapPoint> d_fresh;
    std::vector<LmMapPoint*> created;
    dsh_template_switch_counts dc;
    if (!defslam_hip::UpdateTemplateHIP(
            store, kfstore, ref,
            [&](const float* x3w) { d_fresh.emplace_back(); d_fresh.back().SetWorldPos(x3w); d_fresh.back().nVisible = 1; return &d_fresh.back(); },
            [&](int a, int b, int c) { return mesh.facet_of(a, b, c); }, created, &dc)) return driver_fail(ctx, "UpdateTemplateHIP");
    pts.insert(pts.end(), created.begin(), created.end());
    dump(out, d_need, dc, pts, *ref, mesh);
    const int d_again = defslam_hip::NeedNewTemplateHIP(store, ref);   // the new points are held now

    // ---- the host way, over the second copy ----
    LmKeyFrame* href = &host.kfs[hd.ref];
    const int h_need = host_need_new_template(*href);
    std::vector<LmMapPoint*> all(P);
    for (int p = 0; p < P; p++) all[p] = &host.mps[p];
    std::deque<LmMapPoint> h_fresh;
    dsh_template_switch_counts hc;
    if (!host_update_template(ctx, *href, all, h_fresh, mesh, hc)) return driver_fail(ctx, "the host way's updateTemplate");
    dump(out, h_need, hc, all, *href, mesh);
    std::fprintf(out, "%d %d\n", d_again, host_need_new_template(*href));
  }
  return 0;
}

int main(int argc, char** argv) { return run_driver(argc, argv, 2, drive); }
