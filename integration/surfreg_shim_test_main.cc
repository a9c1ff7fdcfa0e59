// CI driver of integration/surface_register_store_hip.h: one keyframe of a map read from a text file is snapshotted, the map changes,
// and the keyframe's surface is registered, both ways over two copies of the same stand-in objects:
//   the store way  MapPointStoreHIP + KeyFrameStoreHIP, SnapshotKeyFrameStoreHIP and RegisterSurfacesStoreHIP: one call each, applyScale and
//                  SetPose written back on the keyframe object
//   the host way   DefKeyFrame's constructor loop and SurfaceRegistration::registerSurfaces over the pointer graph: the walk over
//                  GetMapPoint, isBad, getFacet and PosesKeyframes, dsh_surface_register on the two host clouds, applyScale, SetPose
// Everything the registration yields or mutates is dumped per route, floats and doubles as bit patterns;
// tests/test_surface_register_shim_gpu.py compares the routes with each other and with the restatement.
//   scene file: standin_store_scene.h with appearance, then the tail
//     "slot chi_limit check_chi", 16 floats Twc, N lines "sx sy sz" (the surface points of keyframe slot, camera frame),
//     "F" and F point ids (the points with a facet), "A" and A lines of what happens after the snapshot -- "move p x y z", "bad p",
//     "facet_off p", "table idx p" --, "nu" and nu doubles (the rand() stream)
//   usage and exit codes: shim_driver.h
#include <cstring>
#include <fstream>
#include <string>

#include "shim_driver.h"
#include "standin_store_scene.h"
#include "surface_register_store_hip.h"

using namespace standin;

typedef defslam_hip::MapPointStoreHIP<LmKeyFrame, LmMapPoint> Store;
typedef defslam_hip::KeyFrameStoreHIP<LmKeyFrame, LmMapPoint> KfStore;

namespace {

struct Op {
  std::string what;
  int a = 0, b = 0;
  float x[3] = {0, 0, 0};
};

struct RegisterScene : StoreScene {
  int slot = 0, check_chi = 1;
  double chi_limit = 0;
  std::vector<int> with_facet;
  std::vector<Op> ops;
  std::vector<double> u;
  LmFacet facet;

  bool read_file(const char* path) {
    std::ifstream f(path);
    if (!read(f) || !appearance || !(f >> slot >> chi_limit >> check_chi) || slot < 0 || slot >= K) return false;
    LmKeyFrame& kf = kfs[slot];
    for (float& t : kf.Twc) f >> t;
    kf.surface_points.resize(3 * (size_t)kf.N);
    for (float& s : kf.surface_points) f >> s;
    int F = 0, A = 0;
    long long nu = 0;
    if (!(f >> F) || F < 0) return false;
    with_facet.resize(F);
    for (int& p : with_facet)
      if (!(f >> p) || p < 0 || p >= P) return false;
    if (!(f >> A) || A < 0) return false;
    ops.resize(A);
    for (Op& o : ops) {
      f >> o.what >> o.a;
      if (o.what == "move") f >> o.x[0] >> o.x[1] >> o.x[2];
      else if (o.what == "table") f >> o.b;
      else if (o.what != "bad" && o.what != "facet_off") return false;
      if (!f || o.a < 0 || (o.what == "table" ? o.a >= kf.N || o.b < -1 || o.b >= P : o.a >= P)) return false;
    }
    if (!(f >> nu) || nu < 0) return false;
    u.resize((size_t)nu);
    for (double& v : u) f >> v;
    for (int p : with_facet) pts[p].SetFacet(&facet);
    return (bool)f;
  }

  // what happens to the map between the keyframe's construction and its registration, on the objects
  void apply(const Op& o) {
    if (o.what == "move") pts[o.a].SetWorldPos(o.x);
    else if (o.what == "bad") pts[o.a].bad = true;
    else if (o.what == "facet_off") pts[o.a].SetFacet(nullptr);
    else kfs[slot].mvpMapPoints[o.a] = o.b >= 0 ? &pts[o.b] : nullptr;
  }
};

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

// SurfaceRegistration::registerSurfaces over the objects (SurfaceRegistration.cc:48-153), the numeric part by dsh_surface_register
bool host_register(dsh_ctx* ctx, RegisterScene& s, dsh_keyframe_register_result& r, std::vector<int>& pairs, bool* ok) {
  LmKeyFrame* refKF = &s.kfs[s.slot];
  std::memset(&r, 0, sizeof(r));
  std::vector<float> cloud1pc, cloud2pc;
  for (size_t i = 0; i < refKF->mvpMapPoints.size(); i++) {                        // :60-104
    LmMapPoint* pMP = refKF->GetMapPoint(i);
    if (!pMP) { r.n_empty++; continue; }
    if (pMP->isBad()) { r.n_bad++; continue; }
    if (!pMP->getFacet()) { r.n_no_facet++; continue; }
    const auto it = pMP->PosesKeyframes.find(refKF);
    if (it == pMP->PosesKeyframes.end()) { r.n_no_snapshot++; continue; }          // x3Dy.empty()
    cloud1pc.insert(cloud1pc.end(), it->second.begin(), it->second.end());
    float x3DKf[3];
    to_world(refKF->Twc, &refKF->surface_points[3 * i], x3DKf);
    cloud2pc.insert(cloud2pc.end(), x3DKf, x3DKf + 3);
    pairs.push_back((int)i);
  }
  r.n_pairs = (int32_t)pairs.size();
  *ok = dsh_surface_register(ctx, r.n_pairs, cloud2pc.data(), cloud1pc.data(), s.u.data(), (int64_t)s.u.size(), refKF->Twc, s.chi_limit, s.check_chi, &r.registered,
                             r.sim3, &r.s22, r.Tcw_new, r.info) == DSH_OK;
  if (!*ok || !r.registered) return false;
  for (float& v : refKF->surface_points) v = (float)((double)v * r.s22);          // Surface::applyScale, :145
  refKF->SetPose(r.Tcw_new);                                                      // :150
  return true;
}

template <class T, class U>
void bits(std::FILE* o, const char* route, const char* kind, const T* v, size_t n) {
  std::fprintf(o, "%s %s", route, kind);
  for (size_t i = 0; i < n; i++) {
    U b;
    std::memcpy(&b, &v[i], sizeof(U));
    std::fprintf(o, " %llu", (unsigned long long)b);
  }
  std::fprintf(o, "\n");
}

void dump(std::FILE* o, const char* route, bool ret, const dsh_keyframe_register_result& r, LmKeyFrame& kf) {
  std::fprintf(o, "%s counts %d %d %d %d %d %d %d\n", route, r.n_pairs, r.n_empty, r.n_bad, r.n_no_facet, r.n_no_snapshot, r.registered, ret ? 1 : 0);
  bits<double, uint64_t>(o, route, "sim3", r.sim3, 8);
  bits<double, uint64_t>(o, route, "s22", &r.s22, 1);
  bits<double, uint64_t>(o, route, "info", r.info, 8);
  bits<float, uint32_t>(o, route, "Tcw_new", r.Tcw_new, 16);
  bits<float, uint32_t>(o, route, "kf_Tcw", kf.Tcw, 16);
  bits<float, uint32_t>(o, route, "kf_Twc", kf.Twc, 16);
  bits<float, uint32_t>(o, route, "kf_Ow", kf.Ow, 3);
  bits<float, uint32_t>(o, route, "surface", kf.surface_points.data(), kf.surface_points.size());
}

}  // namespace

static int drive(const DriverArgs& arg) {
  dsh_ctx* ctx = arg.ctx;
  std::FILE* o = arg.out;
  RegisterScene a, b;
  if (!a.read_file(arg.in[0]) || !b.read_file(arg.in[0])) return driver_bad_input(arg.in[0]);

  // ---- the store way, on copy a ----
  Store store(ctx, 4, 1, 4);   // small on purpose: the store grows, the snapshot beside the tables too
  KfStore kfstore(ctx, 1);
  if (kfstore.status() != DSH_OK || !a.fill(store, &kfstore)) return driver_fail(ctx, "filling the stores");
  {
    std::vector<int32_t> ids(a.with_facet.begin(), a.with_facet.end()), nodes;
    std::vector<double> bary;
    for (size_t e = 0; e < ids.size(); e++) {
      nodes.push_back(0); nodes.push_back(1); nodes.push_back(2);
      bary.push_back(1.0); bary.push_back(0.0); bary.push_back(0.0);
    }
    if (dsh_trackstate_set_embedding(store.handle(), (int)ids.size(), ids.data(), nodes.data(), bary.data()) != DSH_OK) return driver_fail(ctx, "the facets on the store");
  }
  LmKeyFrame* kfa = &a.kfs[a.slot];
  const int taken = defslam_hip::SnapshotKeyFrameStoreHIP(store, kfa);
  if (taken < 0) return driver_fail(ctx, "SnapshotKeyFrameStoreHIP");
  for (const Op& op : a.ops) {
    a.apply(op);
    bool ok = true;
    if (op.what == "move") ok = store.UpdatePositions<LmFrame>(std::vector<LmMapPoint*>(1, &a.pts[op.a]));
    else if (op.what == "bad") ok = dsh_mpdb_set_points_bad(store.handle(), 1, &op.a, nullptr) == DSH_OK;
    else if (op.what == "facet_off") {
      const int32_t none[3] = {-1, -1, -1};
      ok = dsh_trackstate_set_embedding(store.handle(), 1, &op.a, none, nullptr) == DSH_OK;
    } else ok = store.SetKeyFramePoint(kfa, op.a, op.b >= 0 ? &a.pts[op.b] : nullptr);
    if (!ok) return driver_fail(ctx, "the changes after the snapshot on the store");
  }
  dsh_keyframe_register_result ra;
  std::memset(&ra, 0, sizeof(ra));
  bool ok_a = false;
  const bool ret_a = defslam_hip::RegisterSurfacesStoreHIP(store, kfstore, kfa, a.u.data(), (int64_t)a.u.size(), a.chi_limit, a.check_chi != 0, &ra, &ok_a);
  if (!ok_a) return driver_fail(ctx, "RegisterSurfacesStoreHIP");
  std::fprintf(o, "store taken %d\n", taken);
  dump(o, "store", ret_a, ra, *kfa);
  dsh_keyframe_pose_input pin;
  pin.kfdb = kfstore.db(); pin.slot = a.slot; pin.Tcw = nullptr;
  float centre[3];
  if (dsh_keyframe_get_centre(store.handle(), &pin, centre) != DSH_OK) return driver_fail(ctx, "dsh_keyframe_get_centre");
  bits<float, uint32_t>(o, "store", "centre", centre, 3);

  // ---- the host way, on copy b ----
  LmKeyFrame* kfb = &b.kfs[b.slot];
  int taken_b = 0;
  for (LmMapPoint* pMP : kfb->mvpMapPoints)                                       // DefKeyFrame.cc:60-74
    if (pMP && !pMP->isBad() && pMP->getFacet()) {
      pMP->PosesKeyframes[kfb] = {{pMP->pos[0], pMP->pos[1], pMP->pos[2]}};
      taken_b++;
    }
  for (const Op& op : b.ops) b.apply(op);
  dsh_keyframe_register_result rb;
  std::vector<int> pairs_b;
  bool ok_b = false;
  const bool ret_b = host_register(ctx, b, rb, pairs_b, &ok_b);
  if (!ok_b) return driver_fail(ctx, "the host way's dsh_surface_register");
  std::fprintf(o, "host taken %d\n", taken_b);
  dump(o, "host", ret_b, rb, *kfb);
  return 0;
}

int main(int argc, char** argv) { return run_driver(argc, argv, 1, drive); }
