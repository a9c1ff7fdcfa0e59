// CI driver of integration/surface_store_hip.h: one keyframe of a map read from a text file goes through the mapping thread's chain --
// normals, Shape from Normals, surface registration, template switch -- both ways over two copies of the same stand-in objects, each
// with stores of its own:
//   the store way  InitSurfaceStoreHIP per keyframe, then twice ObtainK1K2StoreHIP (the second solve starts from the normals of the
//                  first), ShapeFromNormalsStoreHIP, RegisterSurfacesStoreHIP, the template from dsh_keyframe_surface_vertices,
//                  UpdateTemplateHIP: no Surface on the host, kf->surface_points stays empty, the fields come from dsh_keyframe_surface_get
//   the host way   a Surface per keyframe on the host (Modules/Mapping/Surface.cc): x0 from getNormalSurfacePoint, dsh_normals_estimate_db
//                  with the normals downloaded, setNormalSurfacePoint in the reference's order (NormalEstimator.cc:169, :223), obtainM's
//                  walk over the objects (ShapeFromNormals.cc:190-210), dsh_sfn_estimate on host arrays, set3DSurfacePoint and saveArray;
//                  then the same two shim calls on a store WITHOUT a resident Surface: they upload the keyframe's host surface points,
//                  applyScale comes back to the host (the points by the shim, nodesDepth_ by the caller, Surface.cc:117-120), the
//                  template from dsh_surface_vertices on the host spline
// Every mutated Surface field of every keyframe, the registration's result, the keyframe's pose and every map point of the store after
// the switch are dumped per route, floats and doubles as bit patterns; tests/test_surface_store_shim_gpu.py compares the routes.
//   scene file: standin_store_scene.h with appearance, then the tail
//     "slot umin umax nptsu vmin vmax nptsv bending_weight mean_depth", per keyframe its N lines "x y" (mpKeypointNorm),
//     "R" and R lines "point tag idx2 f0 .. f17" (the DiffProp records; the tag is the slot of the record's second keyframe),
//     "Q" and Q point ids (the points with a new observation),
//     "rows cols xs ys chi_limit check_chi", 16 floats Twc, N lines "px py" (mvKeysUn of keyframe slot), "F" and F point ids (the points
//     with a facet when the keyframe was constructed), "nu" and nu doubles (the rand() stream)
//   usage and exit codes: shim_driver.h
#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <string>

#include "shim_driver.h"
#include <deque>

#include "standin_store_scene.h"
#include "surface_register_store_hip.h"
#include "surface_store_hip.h"
#include "template_switch_hip.h"

using namespace standin;

typedef defslam_hip::MapPointStoreHIP<LmKeyFrame, LmMapPoint> Store;
typedef defslam_hip::KeyFrameStoreHIP<LmKeyFrame, LmMapPoint> KfStore;

namespace {

struct SurfaceScene : StoreScene {
  int kf_slot = 0;
  dsh_bbs bbs;
  double bending = 0, mean_depth = 0;
  std::vector<dsh_diffprop> recs;
  std::vector<int32_t> rec_point, rec_tag, rec_idx2;
  std::vector<LmMapPoint*> todo;
  int xs = 0, ys = 0, check_chi = 0;
  double chi_limit = 0;
  std::vector<int32_t> with_facet;
  std::vector<double> u;

  bool read_file(const char* path) {
    std::ifstream f(path);
    if (!read(f) || !(f >> kf_slot >> bbs.umin >> bbs.umax >> bbs.nptsu >> bbs.vmin >> bbs.vmax >> bbs.nptsv >> bending >> mean_depth) || kf_slot < 0 || kf_slot >= K) return false;
    bbs.valdim = 1;
    for (LmKeyFrame& kf : kfs) {
      kf.mpKeypointNorm.resize(kf.N);
      for (KeyPoint& k : kf.mpKeypointNorm) f >> k.pt.x >> k.pt.y;
    }
    int nrec = 0, Q = 0;
    if (!(f >> nrec) || nrec < 0) return false;
    recs.resize(nrec); rec_point.resize(nrec); rec_tag.resize(nrec); rec_idx2.resize(nrec);
    for (int r = 0; r < nrec; r++) {
      f >> rec_point[r] >> rec_tag[r] >> rec_idx2[r];
      float v[18];
      for (float& x : v) f >> x;
      static_assert(sizeof(dsh_diffprop) == sizeof(v), "dsh_diffprop is eighteen floats");
      std::memcpy(&recs[r], v, sizeof(v));
      if (!f || rec_point[r] < 0 || rec_point[r] >= P || rec_tag[r] < 0 || rec_tag[r] >= K || rec_idx2[r] < 0 || rec_idx2[r] >= kfs[rec_tag[r]].N) return false;
    }
    if (!(f >> Q) || Q < 0) return false;
    for (int q = 0; q < Q; q++) {
      int p = -1;
      if (!(f >> p) || p < 0 || p >= P) return false;
      todo.push_back(&pts[p]);
    }
    LmKeyFrame& kf = kfs[kf_slot];
    if (!appearance || !(f >> kf.rows >> kf.cols >> xs >> ys >> chi_limit >> check_chi) || xs < 2 || ys < 2) return false;
    for (float& t : kf.Twc) f >> t;
    for (KeyPoint& k : kf.mvKeysUn) f >> k.pt.x >> k.pt.y;
    int F = 0;
    long long nu = 0;
    if (!(f >> F) || F < 0) return false;
    with_facet.resize(F);
    for (int32_t& p : with_facet)
      if (!(f >> p) || p < 0 || p >= P) return false;
    if (!(f >> nu) || nu < 0) return false;
    u.resize((size_t)nu);
    for (double& v : u) f >> v;
    return (bool)f;
  }
};

// defSLAM::Surface as the host way keeps it (Modules/Mapping/Surface.cc)
struct HostSurface {
  std::vector<float> normal, x3D;
  std::vector<uint8_t> on;
  std::vector<double> nodesDepth_;
  int numberofNormals_ = 0;
  explicit HostSurface(int n) : normal(3 * (size_t)n, 0.f), x3D(3 * (size_t)n, 0.f), on(n, 0) {}
  void setNormalSurfacePoint(size_t ind, const float* N) {   // :76-85
    if (!on[ind]) numberofNormals_++;
    on[ind] = 1;
    std::memcpy(&normal[3 * ind], N, 12);
  }
  bool getNormalSurfacePoint(size_t ind, float* N) const {   // :88-91
    if (!on[ind]) return false;
    std::memcpy(N, &normal[3 * ind], 12);
    return true;
  }
};

// NormalEstimator::ObtainK1K2 over the host Surfaces, the solve by dsh_normals_estimate_db with everything downloaded
bool host_normals(dsh_ctx* ctx, SurfaceScene& s, dsh_diffdb* ddb, std::vector<HostSurface>& surf) {
  const int P = (int)s.todo.size();
  const size_t m = (size_t)(P > 0 ? P : 1), cap = std::max<size_t>(s.recs.size(), 1);
  std::vector<int32_t> ids(m), ref_slot(m), ref_idx(m), status(m), iters(m), rec_point(cap), rec_tag(cap), rec_idx2(cap);
  std::vector<float> x0(2 * m, 0.f), uv(2 * m), normal_ref(3 * m), normal_rec(3 * cap);
  std::vector<uint8_t> has(m, 0), written(cap);
  std::vector<double> k1k2(2 * m), cov(4 * m);
  for (int p = 0; p < P; p++) {
    LmKeyFrame* refKF = s.todo[p]->GetReferenceKeyFrame();
    ids[p] = s.id(s.todo[p]); ref_slot[p] = s.slot(refKF); ref_idx[p] = s.todo[p]->GetIndexInKeyFrame(refKF);
    if (ref_slot[p] < 0 || ref_idx[p] < 0) return false;
    float Ni[3];
    if (surf[ref_slot[p]].getNormalSurfacePoint(ref_idx[p], Ni)) {   // :125-135
      x0[2 * p] = Ni[0]; x0[2 * p + 1] = Ni[1]; has[p] = 1;
    }
    uv[2 * p] = refKF->mpKeypointNorm[ref_idx[p]].pt.x;             // :162-163
    uv[2 * p + 1] = refKF->mpKeypointNorm[ref_idx[p]].pt.y;
  }
  int32_t n_rec = 0;
  if (dsh_normals_estimate_db(ctx, ddb, P, ids.data(), x0.data(), has.data(), uv.data(), k1k2.data(), cov.data(), status.data(), normal_ref.data(), iters.data(),
                              (int32_t)cap, &n_rec, rec_point.data(), rec_tag.data(), rec_idx2.data(), normal_rec.data(), written.data()) != DSH_OK)
    return false;
  int32_t r = 0;
  for (int p = 0; p < P; p++) {
    if (status[p] == 0) surf[ref_slot[p]].setNormalSurfacePoint(ref_idx[p], &normal_ref[3 * (size_t)p]);   // :169
    for (; r < n_rec && rec_point[r] == p; r++)
      if (written[r]) surf[rec_tag[r]].setNormalSurfacePoint(rec_idx2[r], &normal_rec[3 * (size_t)r]);       // :223
  }
  return true;
}

// ShapeFromNormals(kf, bendingWeight).estimate() over the objects, the solve by dsh_sfn_estimate on host arrays
bool host_sfn(dsh_ctx* ctx, SurfaceScene& s, HostSurface& sref, dsh_keyframe_sfn_result& out, bool* ok) {
  LmKeyFrame* Refkf = &s.kfs[s.kf_slot];
  std::memset(&out, 0, sizeof(out));
  std::vector<double> u_vector_, v_vector_, u_all, v_all;
  std::vector<float> Normals;
  for (size_t var = 0; var < Refkf->mvpMapPoints.size(); ++var) {                  // ShapeFromNormals.cc:190-210
    float Normal[3];
    LmMapPoint* mp = Refkf->GetMapPoint(var);
    u_all.push_back(Refkf->mpKeypointNorm[var].pt.x);
    v_all.push_back(Refkf->mpKeypointNorm[var].pt.y);
    if (!mp) { out.n_empty++; continue; }
    if (mp->isBad()) { out.n_bad++; continue; }
    if (!sref.getNormalSurfacePoint(var, Normal)) { out.n_no_normal++; continue; }
    if (!(Normal[0] == Normal[0] && Normal[1] == Normal[1] && Normal[2] == Normal[2])) { out.n_nan++; continue; }
    Normals.insert(Normals.end(), Normal, Normal + 3);
    u_vector_.push_back(Refkf->mpKeypointNorm[var].pt.x);
    v_vector_.push_back(Refkf->mpKeypointNorm[var].pt.y);
  }
  out.n_sites = (int32_t)u_vector_.size();
  const size_t Nc = (size_t)s.bbs.nptsu * s.bbs.nptsv;
  std::vector<double> Array(Nc);
  std::vector<float> pts(3 * std::max<size_t>(u_all.size(), 1));
  int32_t good = 0;
  *ok = dsh_sfn_estimate(ctx, &s.bbs, out.n_sites, u_vector_.data(), v_vector_.data(), Normals.data(), s.bending, s.mean_depth, (int)u_all.size(), u_all.data(),
                         v_all.data(), nullptr, Array.data(), pts.data(), &good) == DSH_OK;
  if (!*ok || !good) return false;
  out.ok = 1;
  std::copy(pts.begin(), pts.begin() + 3 * u_all.size(), sref.x3D.begin());        // :158-165 set3DSurfacePoint
  sref.nodesDepth_ = Array;                                                       // :167 saveArray
  return true;
}

// The stores of one route from its copy of the scene: the map, the facets the points had when the keyframe was constructed, and
// DefKeyFrame's snapshot of their positions (surface_register_store_hip.h).
bool fill_stores(SurfaceScene& s, Store& store, KfStore& kfstore) {
  if (kfstore.status() != DSH_OK || !s.fill(store, &kfstore)) return false;
  std::vector<int32_t> nodes;
  std::vector<double> bary;
  for (size_t e = 0; e < s.with_facet.size(); e++) {
    nodes.push_back(0); nodes.push_back(1); nodes.push_back(2);
    bary.push_back(1.0); bary.push_back(0.0); bary.push_back(0.0);
  }
  if (dsh_trackstate_set_embedding(store.handle(), (int)s.with_facet.size(), s.with_facet.data(), nodes.data(), bary.data()) != DSH_OK) return false;
  return defslam_hip::SnapshotKeyFrameStoreHIP(store, &s.kfs[s.kf_slot]) >= 0;
}

template <class T, class U>
void row(std::FILE* o, const char* route, const char* kind, const T* v, size_t n) {
  std::fprintf(o, "%s %s", route, kind);
  for (size_t i = 0; i < n; i++) {
    U b;
    std::memcpy(&b, &v[i], sizeof(U));
    std::fprintf(o, " %llu", (unsigned long long)b);
  }
  std::fprintf(o, "\n");
}

// SurfaceRegistration::registerSurfaces and DefLocalMapping::updateTemplate through the two shims, whichever way the keyframe keeps its
// Surface; vertices(Twc, xyz) gives the nodes of the new template.  Dumps the registration, the pose and every point of the store.
template <class Vertices>
const char* register_and_switch(dsh_ctx* ctx, std::FILE* o, const char* route, SurfaceScene& s, Store& store, KfStore& kfstore, Vertices vertices,
                                dsh_keyframe_register_result& r) {
  LmKeyFrame* kf = &s.kfs[s.kf_slot];
  bool ok = false;
  const bool ret = defslam_hip::RegisterSurfacesStoreHIP(store, kfstore, kf, s.u.data(), (int64_t)s.u.size(), s.chi_limit, s.check_chi != 0, &r, &ok);
  if (!ok) return "RegisterSurfacesStoreHIP";
  std::fprintf(o, "%s register %d %d %d %d %d %d %d\n", route, ret ? 1 : 0, r.n_pairs, r.n_empty, r.n_bad, r.n_no_facet, r.n_no_snapshot, r.registered);
  row<double, uint64_t>(o, route, "sim3", r.sim3, 8);
  row<double, uint64_t>(o, route, "s22", &r.s22, 1);
  row<float, uint32_t>(o, route, "kf_Tcw", kf->Tcw, 16);
  row<float, uint32_t>(o, route, "kf_Twc", kf->Twc, 16);
  std::vector<double> xyz(3 * (size_t)s.xs * s.ys);
  if (!vertices(kf->Twc, xyz.data())) return "the vertices of the template";
  row<double, uint64_t>(o, route, "vertices", xyz.data(), xyz.size());
  std::vector<int32_t> tri;
  for (int j = 0; j < s.xs - 1; j++)                                               // TriangularMesh.cc:92-107
    for (int i = 0; i < s.ys - 1; i++) {
      const int c = s.ys, a[6] = {i + c * j, i + c * j + 1, c * (j + 1) + i, i + c * j + 1, c * (j + 1) + i, c * (j + 1) + i + 1};
      tri.insert(tri.end(), a, a + 6);
    }
  if (dsh_template_build(ctx, s.xs * s.ys, xyz.data(), (int)tri.size() / 3, tri.data()) != DSH_OK) return "dsh_template_build";
  static LmFacet some_facet;   // the objects' facets are not compared: the store's node indices are
  std::deque<LmMapPoint> fresh;
  std::vector<LmMapPoint*> created;
  dsh_template_switch_counts c = dsh_template_switch_counts();
  if (!defslam_hip::UpdateTemplateHIP(
          store, kfstore, kf, [&](const float* x3w) { fresh.emplace_back(); fresh.back().SetWorldPos(x3w); fresh.back().nVisible = 1; return &fresh.back(); },
          [&](int, int, int) { return &some_facet; }, created, &c))
    return "UpdateTemplateHIP";
  std::fprintf(o, "%s switch %d %d %d %d %d %d\n", route, c.n_new, c.first_id, c.n_moved, c.n_masked, c.n_embedded, c.n_points);
  const int P = c.n_points;
  std::vector<int32_t> ids(P), nodes(3 * (size_t)P);
  for (int p = 0; p < P; p++) ids[p] = p;
  std::vector<float> pos(3 * (size_t)P), nrm(3 * (size_t)P), maxd(P);
  std::vector<double> bary(3 * (size_t)P);
  if (dsh_point_store_get_points(store.handle(), P, ids.data(), pos.data(), nrm.data(), maxd.data(), nullptr, nullptr) != DSH_OK ||
      dsh_point_store_get_embedding(store.handle(), P, ids.data(), nodes.data(), bary.data()) != DSH_OK)
    return "the read-back of the points";
  row<float, uint32_t>(o, route, "xyz", pos.data(), pos.size());
  row<float, uint32_t>(o, route, "point_normal", nrm.data(), nrm.size());
  row<float, uint32_t>(o, route, "max_distance", maxd.data(), maxd.size());
  row<int32_t, uint32_t>(o, route, "nodes", nodes.data(), nodes.size());
  row<double, uint64_t>(o, route, "bary", bary.data(), bary.size());
  return nullptr;
}

template <class T, class U>
void bits(std::FILE* o, const char* route, int k, const char* kind, const T* v, size_t n) {
  std::fprintf(o, "%s kf %d %s", route, k, kind);
  for (size_t i = 0; i < n; i++) {
    U b;
    std::memcpy(&b, &v[i], sizeof(U));
    std::fprintf(o, " %llu", (unsigned long long)b);
  }
  std::fprintf(o, "\n");
}

void dump(std::FILE* o, const char* route, int k, int n_normals, const std::vector<float>& normal, const std::vector<uint8_t>& on, const std::vector<float>& x3D,
          const std::vector<double>& depth) {
  std::fprintf(o, "%s kf %d counts %d %d\n", route, k, n_normals, (int)depth.size());
  bits<float, uint32_t>(o, route, k, "normal", normal.data(), normal.size());
  bits<uint8_t, uint8_t>(o, route, k, "on", on.data(), on.size());
  bits<float, uint32_t>(o, route, k, "x3D", x3D.data(), x3D.size());
  bits<double, uint64_t>(o, route, k, "depth", depth.data(), depth.size());
}

}  // namespace

static int drive(const DriverArgs& arg) {
  dsh_ctx* ctx = arg.ctx;
  std::FILE* o = arg.out;
  SurfaceScene a, b;
  if (!a.read_file(arg.in[0]) || !b.read_file(arg.in[0])) return driver_bad_input(arg.in[0]);
  dsh_diffdb* ddb = nullptr;
  if (dsh_diffdb_create(ctx, 16, &ddb) != DSH_OK) return driver_fail(ctx, "dsh_diffdb_create");
  int rc = 1;
  do {
    if (dsh_diffdb_append(ddb, (int)a.recs.size(), a.recs.data(), a.rec_point.data(), a.rec_tag.data(), a.rec_idx2.data()) != DSH_OK) {
      driver_fail(ctx, "dsh_diffdb_append");
      break;
    }
    // ---- the store way, on copy a ----
    Store store(ctx, 4, 1, 4);   // small on purpose: the store grows, the Surface arrays beside the tables too
    KfStore kfstore(ctx, 1);
    if (!fill_stores(a, store, kfstore)) { driver_fail(ctx, "filling the stores"); break; }
    bool ok = true;
    for (LmKeyFrame& kf : a.kfs) ok = ok && defslam_hip::InitSurfaceStoreHIP(store, &kf);
    if (!ok) { driver_fail(ctx, "InitSurfaceStoreHIP"); break; }
    defslam_hip::NormalsStoreResult nr;
    auto of_tag = [&](int32_t tag) { return &a.kfs[tag]; };
    for (int round = 0; ok && round < 2; round++) ok = defslam_hip::ObtainK1K2StoreHIP(ctx, store, ddb, a.todo, of_tag, &nr);
    if (!ok) { driver_fail(ctx, "ObtainK1K2StoreHIP"); break; }
    dsh_keyframe_sfn_result ra;
    bool ok_a = false;
    const bool ret_a = defslam_hip::ShapeFromNormalsStoreHIP(ctx, store, &a.kfs[a.kf_slot], a.bbs, a.bending, a.mean_depth, &ra, &ok_a);
    if (!ok_a) { driver_fail(ctx, "ShapeFromNormalsStoreHIP"); break; }
    std::fprintf(o, "store sfn %d %d %d %d %d %d %d\n", ret_a ? 1 : 0, ra.n_sites, ra.n_empty, ra.n_bad, ra.n_no_normal, ra.n_nan, ra.ok);
    std::fprintf(o, "store solved %d %d\n", nr.n_solved, nr.n_propagated);
    // the keyframe object holds no surface point: what the registration and the switch read is the store's
    std::fprintf(o, "store host_surface_points %d\n", (int)a.kfs[a.kf_slot].surface_points.size());
    dsh_keyframe_register_result ga;
    if (const char* what = register_and_switch(ctx, o, "store", a, store, kfstore, [&](const float* Twc, double* xyz) {
          return dsh_keyframe_surface_vertices(store.handle(), a.kf_slot, Twc, a.xs, a.ys, xyz) == DSH_OK;
        }, ga)) { driver_fail(ctx, what); break; }
    for (int k = 0; ok && k < a.K; k++) {
      const size_t n = (size_t)a.kfs[k].N;
      std::vector<float> normal(3 * n), x3D(3 * n), kpn(2 * n);
      std::vector<uint8_t> on(n);
      std::vector<double> depth(512);
      dsh_keyframe_surface_info info;
      ok = dsh_keyframe_surface_get(store.handle(), k, (int32_t)n, normal.data(), on.data(), x3D.data(), kpn.data(), depth.data(), &info) == DSH_OK;
      depth.resize(info.has_depth ? (size_t)info.grid.nptsu * info.grid.nptsv : 0);
      if (ok) dump(o, "store", k, info.n_normals, normal, on, x3D, depth);
    }
    if (!ok) { driver_fail(ctx, "dsh_keyframe_surface_get"); break; }

    // ---- the host way, on copy b ----
    std::vector<HostSurface> surf;
    for (LmKeyFrame& kf : b.kfs) surf.push_back(HostSurface(kf.N));
    for (int round = 0; ok && round < 2; round++) ok = host_normals(ctx, b, ddb, surf);
    if (!ok) { driver_fail(ctx, "the host way's dsh_normals_estimate_db"); break; }
    dsh_keyframe_sfn_result rb;
    bool ok_b = false;
    const bool ret_b = host_sfn(ctx, b, surf[b.kf_slot], rb, &ok_b);
    if (!ok_b) { driver_fail(ctx, "the host way's dsh_sfn_estimate"); break; }
    std::fprintf(o, "host sfn %d %d %d %d %d %d %d\n", ret_b ? 1 : 0, rb.n_sites, rb.n_empty, rb.n_bad, rb.n_no_normal, rb.n_nan, rb.ok);
    Store store_b(ctx, 4, 1, 4);   // no resident Surface here: the shims upload the keyframe's own points
    KfStore kfstore_b(ctx, 1);
    if (!fill_stores(b, store_b, kfstore_b)) { driver_fail(ctx, "filling the host way's stores"); break; }
    LmKeyFrame* kfb = &b.kfs[b.kf_slot];
    HostSurface& sb = surf[b.kf_slot];
    kfb->surface_points = sb.x3D;                                                  // surface->get3DSurfacePoint
    dsh_keyframe_register_result gb;
    bool scaled = false;
    if (const char* what = register_and_switch(ctx, o, "host", b, store_b, kfstore_b, [&](const float* Twc, double* xyz) {
          if (gb.registered && !scaled) {                                            // Surface::applyScale, :107-121: the shim wrote the points back
            sb.x3D = kfb->surface_points;
            for (double& d : sb.nodesDepth_) d = gb.s22 * d;
            scaled = true;
          }
          dsh_surface_grid g;
          g.ctx = ctx; g.bbs = &b.bbs; g.depth_ctrl = sb.nodesDepth_.data(); g.Twc = Twc; g.xs = b.xs; g.ys = b.ys;
          return dsh_surface_vertices(&g, xyz) == DSH_OK;
        }, gb)) { driver_fail(ctx, what); break; }
    for (int k = 0; k < b.K; k++) dump(o, "host", k, surf[k].numberofNormals_, surf[k].normal, surf[k].on, surf[k].x3D, surf[k].nodesDepth_);
    rc = 0;
  } while (false);
  dsh_diffdb_destroy(ddb);
  return rc;
}

int main(int argc, char** argv) { return run_driver(argc, argv, 1, drive); }
