// CI driver of the Shape-from-Template shim on the map point store (integration/def_pose_store_hip.h): builds the stand-in Template /
// Frame / DefMap / DefMapPoint objects of a text file TWICE, runs one frame the store way (DefPoseOptimizationStoreHIP: the facets and
// barycentrics are the store's, the points move on the device) on the first copy and the existing way (DefPoseOptimizationHIP of
// defslam_hip_shim.h: the observation table from a walk over the objects) on the second, and writes every mutation the reference's call
// makes of each copy to <output>.store and <output>.host in one layout, numbers as bit patterns: equal files mean equal mutations.
//   usage: tracksft_shim_test <input.txt> <output> [device]
// Input (floats round-trip):
//   n F | n rest positions | n current positions | F facets "a b c" | fx fy cx cy | Tcw (16) | N levels | mvInvLevelSigma2
//   P | P points "bad has_facet n0 n1 n2 b1 b2 b3 x y z" | N key points "x y octave id outlier" | RegLap RegInex RegTemp layers
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>

#include "def_pose_store_hip.h"
#include "standin_types.h"

using namespace standin;
CountingMutex standin::MapPoint::mGlobalMutex;

namespace {

struct World {
  std::vector<Node> nodes;
  std::vector<Facet> facets;
  Template tmpl;
  Frame frame;
  DefMap map;
  std::vector<std::unique_ptr<DefMapPoint>> points;   // every point of the store, bad ones too; map.points holds the others
  double RegLap = 0, RegInex = 0, RegTemp = 0;
  unsigned layers = 1;

  bool read(const char* path) {
    std::ifstream in(path);
    if (!in.good()) return false;
    int n, F;
    in >> n >> F;
    nodes.reserve(n);   // contiguous: std::set<Node*> iterates in index order
    for (int i = 0; i < n; i++) { double x, y, z; in >> x >> y >> z; nodes.emplace_back(x, y, z); }
    for (int i = 0; i < n; i++) { double x, y, z; in >> x >> y >> z; nodes[i].setXYZ(x, y, z); }
    facets.reserve(F);
    std::map<std::array<int, 3>, int> facet_of;
    for (int f = 0; f < F; f++) {
      int v[3];
      in >> v[0] >> v[1] >> v[2];
      facets.emplace_back(&nodes[v[0]], &nodes[v[1]], &nodes[v[2]]);
      for (int p = 0; p < 3; p++)
        for (int q = 0; q < 3; q++)
          if (p != q) nodes[v[p]].neighbours.insert(&nodes[v[q]]);
      std::array<int, 3> key = {{v[0], v[1], v[2]}};
      std::sort(key.begin(), key.end());
      facet_of[key] = f;
    }
    for (auto& nd : nodes) tmpl.nodes.insert(&nd);
    for (auto& fc : facets) tmpl.facets.insert(&fc);
    map.tmpl = &tmpl;
    in >> frame.fx >> frame.fy >> frame.cx >> frame.cy;
    for (int i = 0; i < 16; i++) in >> frame.mTcw[i];
    int levels;
    in >> frame.N >> levels;
    frame.mvInvLevelSigma2.resize(levels);
    for (auto& v : frame.mvInvLevelSigma2) in >> v;
    int P;
    in >> P;
    for (int p = 0; p < P; p++) {
      int bad, has, nd[3];
      double b[3];
      points.emplace_back(new DefMapPoint());
      DefMapPoint* mp = points.back().get();
      in >> bad >> has >> nd[0] >> nd[1] >> nd[2] >> b[0] >> b[1] >> b[2] >> mp->mWorldPos[0] >> mp->mWorldPos[1] >> mp->mWorldPos[2];
      mp->bad = bad != 0;
      if (has) {
        const auto it = facet_of.find(std::array<int, 3>{{nd[0], nd[1], nd[2]}});
        if (it == facet_of.end()) return false;
        mp->facet = &facets[it->second];
        mp->b1 = b[0]; mp->b2 = b[1]; mp->b3 = b[2];
      }
      if (!mp->bad) map.points.push_back(mp);   // DefMapPoint::setBadFlag erases the point from the map
    }
    frame.mvKeysUn.resize(frame.N);
    frame.mvpMapPoints.assign(frame.N, nullptr);
    frame.mvbOutlier.assign(frame.N, false);
    for (int i = 0; i < frame.N; i++) {
      int id, out;
      in >> frame.mvKeysUn[i].pt.x >> frame.mvKeysUn[i].pt.y >> frame.mvKeysUn[i].octave >> id >> out;
      if (id >= P) return false;
      if (id >= 0) frame.mvpMapPoints[i] = points[id].get();
      frame.mvbOutlier[i] = out != 0;
    }
    in >> RegLap >> RegInex >> RegTemp >> layers;
    return in.good();
  }

  // every field the call mutates, numbers as bit patterns
  void dump(const std::string& path, int ret) {
    std::FILE* f = std::fopen(path.c_str(), "w");
    if (!f) return;
    auto bits = [](float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; };
    int under_lock = 0, recalculated = 0;
    for (auto& p : points) { under_lock += p->recalculated_under_lock; recalculated += p->recalculated; }
    std::fprintf(f, "ret %d repError %u pose_sets %d held %d recalculated %d under_lock %d\nTcw", ret, bits(frame.repError), frame.pose_sets,
                 (int)MapPoint::mGlobalMutex.held, recalculated, under_lock);
    for (int i = 0; i < 16; i++) std::fprintf(f, " %u", bits(frame.mTcw[i]));
    std::fprintf(f, "\n");
    for (auto& nd : nodes) std::fprintf(f, "node %a %a %a %u %d %d %d\n", nd.x, nd.y, nd.z, nd.getIndex(), (int)nd.viewed, (int)nd.local, (int)nd.role);
    std::fprintf(f, "flags");
    for (int i = 0; i < frame.N; i++) std::fprintf(f, " %d", (int)frame.mvbOutlier[i]);
    std::fprintf(f, "\n");
    for (auto& p : points) std::fprintf(f, "pt %u %u %u %d\n", bits(p->mWorldPos[0]), bits(p->mWorldPos[1]), bits(p->mWorldPos[2]), p->recalculated);
    std::fclose(f);
  }
};

// what DefPoseOptimizationStoreHIP needs of a store; MapPointStoreHIP of local_map_hip.h has both
struct SftStore {
  dsh_mpdb* db = nullptr;
  std::unordered_map<MapPoint*, int> ids;
  dsh_mpdb* handle() const { return db; }
  int id(MapPoint* p) const { auto it = ids.find(p); return it == ids.end() ? -1 : it->second; }

  // the world's points with their facets, in file order: what AddMapPoints and SetEmbedding of MapPointStoreHIP send
  bool fill(dsh_ctx* ctx, World& w, const std::vector<Node>& nodes) {
    dsh_mpdb_desc d;
    d.ctx = ctx;
    d.point_capacity = 64; d.keyframe_capacity = 4; d.observation_capacity = 64;
    if (dsh_mpdb_create(&d, &db) != DSH_OK) return false;
    const size_t P = w.points.size();
    std::vector<float> xyz(3 * P), nrm(3 * P, 0.f), maxd(P, 2.f);
    std::vector<uint8_t> desc(32 * P, 0), bad(P);
    std::vector<int32_t> id(P), nd(3 * P, -1);
    std::vector<double> bary(3 * P, 0.0);
    for (size_t p = 0; p < P; p++) {
      DefMapPoint* mp = w.points[p].get();
      for (int c = 0; c < 3; c++) xyz[3 * p + c] = mp->mWorldPos[c];
      nrm[3 * p + 2] = 1.f;
      bad[p] = mp->bad ? 1 : 0;
      id[p] = (int32_t)p;
      ids[mp] = (int)p;
      if (!mp->facet) continue;
      int k = 0;
      for (Node* n : mp->facet->getNodes()) nd[3 * p + k++] = (int32_t)(n - nodes.data());
      bary[3 * p] = mp->b1; bary[3 * p + 1] = mp->b2; bary[3 * p + 2] = mp->b3;
    }
    int32_t first = -1;
    return dsh_mpdb_add_points(db, (int)P, xyz.data(), nrm.data(), maxd.data(), desc.data(), bad.data(), &first) == DSH_OK && first == 0 &&
           dsh_trackstate_set_embedding(db, (int)P, id.data(), nd.data(), bary.data()) == DSH_OK;
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s in out [device]\n", argv[0]); return 2; }
  World a, b;
  if (!a.read(argv[1]) || !b.read(argv[1])) { std::fprintf(stderr, "bad input\n"); return 2; }
  dsh_ctx* ctx = nullptr;
  if (dsh_create(&ctx, argc > 3 ? std::atoi(argv[3]) : 0) != DSH_OK) { std::fprintf(stderr, "no device\n"); return 3; }
  int rc = 0;
  {
    defslam_hip::TemplateBinding<Template, Node> binding;
    SftStore store;
    if (!store.fill(ctx, a, a.nodes)) { std::fprintf(stderr, "store: %s\n", dsh_last_error(ctx)); return 4; }
    const int ret = defslam_hip::DefPoseOptimizationStoreHIP<Frame, DefMap, Template, Node, DefMapPoint>(ctx, binding, store, &a.frame, &a.map, a.RegLap,
                                                                                                       a.RegInex, a.RegTemp, a.layers);
    if (ret == 0) { std::fprintf(stderr, "store way: %s\n", dsh_last_error(ctx)); rc = 5; }
    a.dump(std::string(argv[2]) + ".store", ret);
    dsh_mpdb_destroy(store.db);
  }
  {
    defslam_hip::TemplateBinding<Template, Node> binding;
    const int ret = defslam_hip::DefPoseOptimizationHIP<Frame, DefMap, Template, Node, DefMapPoint>(ctx, binding, &b.frame, &b.map, b.RegLap, b.RegInex,
                                                                                                  b.RegTemp, b.layers);
    if (ret == 0) { std::fprintf(stderr, "host way: %s\n", dsh_last_error(ctx)); rc = 5; }
    b.dump(std::string(argv[2]) + ".host", ret);
  }
  dsh_destroy(ctx);
  return rc;
}
