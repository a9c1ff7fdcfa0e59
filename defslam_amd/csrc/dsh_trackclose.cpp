// Host side of the per-point tracking state of the map point store and of closing a tracked frame (include/defslam_hip.h:
// dsh_trackstate_*, dsh_track_close_frame): validation against the host mirror, per call one upload, the launches of
// trackclose_kernels.hip and one download.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "mpdb_store.h"
#include "track_problem.h"
#include "trackclose_problem.h"

namespace {

TcState state_of(dsh_mpdb* db) {
  TcState s;
  s.xyz = db->d_xyz; s.bad = db->d_bad; s.visible = db->d_visible; s.found = db->d_found; s.nobs = db->d_nobs; s.nodes = db->d_nodes;
  s.bary = db->d_bary;
  return s;
}

// the upload block of a call: laid out, filled in the context's page-locked buffer, copied up in one piece
struct Upload {
  Arena a;
  char* h = nullptr;
  const char* d = nullptr;
  int stage(dsh_ctx_base* c) {
    HIPCHK(c, c->pin_in.ensure(a.size, true));
    h = c->pin_in.p;
    return DSH_OK;
  }
  int copy(dsh_ctx_base* c) {
    void* dup = nullptr;
    HIPCHK(c, c->scratch.take(a.size, &dup));
    HIPCHK(c, hipMemcpyAsync(dup, h, a.size, hipMemcpyHostToDevice, c->stream));
    d = static_cast<const char*>(dup);
    return DSH_OK;
  }
};

// what is wrong with the stored embedding against a template of n_nodes nodes
std::string nodes_error(dsh_mpdb* db, int n_nodes, const double* node_xyz) {
  if (n_nodes < 0) return "n_nodes < 0";
  if (n_nodes > 0 && !node_xyz) return "node_xyz is NULL";
  if (db->largest_node() >= n_nodes) return "a stored node index (" + std::to_string(db->largest_node()) + ") is >= n_nodes";
  return "";
}

}  // namespace

extern "C" {

int dsh_trackstate_set_embedding(dsh_mpdb* db, int n, const int32_t* ids, const int32_t* nodes, const double* bary) {
  MPDB_ENTER("dsh_trackstate_set_embedding");
  const std::string ie = mpdb_ids_error(n, ids, db->P, "point id");
  if (!ie.empty()) return bad(ie);
  if (n > 0 && !nodes) return bad("nodes is NULL");
  bool any = false;
  for (int i = 0; i < n; i++) {
    const int32_t a = nodes[3 * i], b = nodes[3 * i + 1], d = nodes[3 * i + 2];
    if (a == -1 && b == -1 && d == -1) continue;
    if (!(0 <= a && a < b && b < d)) return bad("nodes of entry " + std::to_string(i) + " are neither -1 -1 -1 nor ascending and distinct");
    any = true;
  }
  if (any && !bary) return bad("bary is NULL");
  if (const int rc = dsh_enter(c, "dsh_trackstate_set_embedding")) return rc;
  if (n == 0) return DSH_OK;
  Upload up;
  const size_t m = (size_t)n, o_ids = up.a.take(4 * m), o_nodes = up.a.take(12 * m), o_bary = up.a.take(24 * m);
  if (const int rc = up.stage(c)) return rc;
  std::memcpy(up.h + o_ids, ids, 4 * m);
  std::memcpy(up.h + o_nodes, nodes, 12 * m);
  if (bary) std::memcpy(up.h + o_bary, bary, 24 * m);
  else std::memset(up.h + o_bary, 0, 24 * m);
  if (const int rc = up.copy(c)) return rc;
  HIPCHK(c, tc_set_embedding_launch(state_of(db), reinterpret_cast<const int32_t*>(up.d + o_ids), reinterpret_cast<const int32_t*>(up.d + o_nodes),
                                    reinterpret_cast<const double*>(up.d + o_bary), n, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < n; i++) {
    int32_t& top = db->top_node[ids[i]];
    if (top == db->max_node && nodes[3 * i + 2] < top) db->max_node_stale = true;
    top = nodes[3 * i + 2];
    if (!db->max_node_stale) db->max_node = std::max(db->max_node, top);
  }
  return DSH_OK;
}

int dsh_trackstate_clear_embedding(dsh_mpdb* db) {
  MPDB_ENTER("dsh_trackstate_clear_embedding");
  (void)bad;
  if (const int rc = dsh_enter(c, "dsh_trackstate_clear_embedding")) return rc;
  HIPCHK(c, tc_set_embedding_launch(state_of(db), nullptr, nullptr, nullptr, db->P, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::fill(db->top_node.begin(), db->top_node.end(), -1);
  db->max_node = -1;
  db->max_node_stale = false;
  return DSH_OK;
}

int dsh_trackstate_set_counters(dsh_mpdb* db, int n, const int32_t* ids, const int32_t* visible, const int32_t* found) {
  MPDB_ENTER("dsh_trackstate_set_counters");
  const std::string ie = mpdb_ids_error(n, ids, db->P, "point id");
  if (!ie.empty()) return bad(ie);
  if (n > 0 && (!visible || !found)) return bad("visible or found is NULL");
  if (const int rc = dsh_enter(c, "dsh_trackstate_set_counters")) return rc;
  if (n == 0) return DSH_OK;
  Upload up;
  const size_t m = (size_t)n, o_ids = up.a.take(4 * m), o_vis = up.a.take(4 * m), o_fnd = up.a.take(4 * m);
  if (const int rc = up.stage(c)) return rc;
  std::memcpy(up.h + o_ids, ids, 4 * m);
  std::memcpy(up.h + o_vis, visible, 4 * m);
  std::memcpy(up.h + o_fnd, found, 4 * m);
  if (const int rc = up.copy(c)) return rc;
  HIPCHK(c, tc_set_counters_launch(state_of(db), reinterpret_cast<const int32_t*>(up.d + o_ids), reinterpret_cast<const int32_t*>(up.d + o_vis),
                                   reinterpret_cast<const int32_t*>(up.d + o_fnd), n, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return DSH_OK;
}

int dsh_trackstate_get(dsh_mpdb* db, int n, const int32_t* ids, int32_t* visible, int32_t* found, int32_t* n_obs, float* xyz) {
  MPDB_ENTER("dsh_trackstate_get");
  const std::string ie = mpdb_ids_error(n, ids, db->P, "point id");
  if (!ie.empty()) return bad(ie);
  if (const int rc = dsh_enter(c, "dsh_trackstate_get")) return rc;
  if (n == 0) return DSH_OK;
  Upload up;
  const size_t m = (size_t)n, o_ids = up.a.take(4 * m);
  Arena down;
  const size_t d_vis = down.take(visible ? 4 * m : 0), d_fnd = down.take(found ? 4 * m : 0), d_nobs = down.take(n_obs ? 4 * m : 0),
               d_xyz = down.take(xyz ? 12 * m : 0);
  if (const int rc = up.stage(c)) return rc;
  HIPCHK(c, c->pin_out.ensure(down.size + 256, true));
  std::memcpy(up.h + o_ids, ids, 4 * m);
  if (const int rc = up.copy(c)) return rc;
  void* ddown = nullptr;
  HIPCHK(c, c->scratch.take(down.size + 256, &ddown));
  char* dd = static_cast<char*>(ddown);
  HIPCHK(c, tc_get_launch(state_of(db), reinterpret_cast<const int32_t*>(up.d + o_ids), n, visible ? reinterpret_cast<int32_t*>(dd + d_vis) : nullptr,
                          found ? reinterpret_cast<int32_t*>(dd + d_fnd) : nullptr, n_obs ? reinterpret_cast<int32_t*>(dd + d_nobs) : nullptr,
                          xyz ? reinterpret_cast<float*>(dd + d_xyz) : nullptr, c->stream));
  if (down.size > 0) HIPCHK(c, hipMemcpyAsync(c->pin_out.p, ddown, down.size, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const char* o = c->pin_out.p;
  if (visible) std::memcpy(visible, o + d_vis, 4 * m);
  if (found) std::memcpy(found, o + d_fnd, 4 * m);
  if (n_obs) std::memcpy(n_obs, o + d_nobs, 4 * m);
  if (xyz) std::memcpy(xyz, o + d_xyz, 12 * m);
  return DSH_OK;
}

int dsh_trackstate_seed_local_points(dsh_mpdb* db, int n, const int32_t* ids) {
  MPDB_ENTER("dsh_trackstate_seed_local_points");
  const std::string ie = mpdb_ids_error(n, ids, db->P, "point id");
  if (!ie.empty()) return bad(ie);
  for (int i = 1; i < n; i++)
    if (ids[i] <= ids[i - 1]) return bad("ids are not ascending");
  if (const int rc = dsh_enter(c, "dsh_trackstate_seed_local_points")) return rc;
  if (n > 0) {
    HIPCHK(c, c->pin_in.ensure(4 * (size_t)n, true));
    std::memcpy(c->pin_in.p, ids, 4 * (size_t)n);
    HIPCHK(c, hipMemcpyAsync(db->d_local_ids, c->pin_in.p, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(db->d_ref_ids, c->pin_in.p, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  }
  const int32_t n32 = n;
  HIPCHK(c, hipMemcpyAsync(&db->d_hdr->n_local_points, &n32, 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  db->n_local_points = db->n_ref_points = n;
  return DSH_OK;
}

int dsh_trackstate_repose(dsh_mpdb* db, int n_nodes, const double* node_xyz, int32_t* n_moved) {
  MPDB_ENTER("dsh_trackstate_repose");
  const std::string ne = nodes_error(db, n_nodes, node_xyz);
  if (!ne.empty()) return bad(ne);
  if (const int rc = dsh_enter(c, "dsh_trackstate_repose")) return rc;
  if (n_moved) *n_moved = 0;
  if (n_nodes == 0 || db->P == 0) return DSH_OK;
  Upload up;
  const size_t o_cnt = up.a.take(4), o_nodes = up.a.take(24 * (size_t)n_nodes);
  if (const int rc = up.stage(c)) return rc;
  HIPCHK(c, c->pin_out.ensure(4, true));
  std::memset(up.h + o_cnt, 0, 4);
  std::memcpy(up.h + o_nodes, node_xyz, 24 * (size_t)n_nodes);
  if (const int rc = up.copy(c)) return rc;
  int32_t* dcnt = reinterpret_cast<int32_t*>(const_cast<char*>(up.d + o_cnt));
  HIPCHK(c, tc_repose_launch(state_of(db), db->P, reinterpret_cast<const double*>(up.d + o_nodes), dcnt, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->pin_out.p, dcnt, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n_moved) std::memcpy(n_moved, c->pin_out.p, 4);
  return DSH_OK;
}

int dsh_trackstate_cull(dsh_mpdb* db, int n, const int32_t* ids, const int32_t* first_kf, int32_t current_kf, uint8_t* action) {
  MPDB_ENTER("dsh_trackstate_cull");
  const std::string ie = mpdb_ids_error(n, ids, db->P, "point id");
  if (!ie.empty()) return bad(ie);
  if (n > 0 && (!first_kf || !action)) return bad("first_kf or action is NULL");
  if (const int rc = dsh_enter(c, "dsh_trackstate_cull")) return rc;
  if (n == 0) return DSH_OK;
  Upload up;
  const size_t m = (size_t)n, o_ids = up.a.take(4 * m), o_first = up.a.take(4 * m);
  if (const int rc = up.stage(c)) return rc;
  HIPCHK(c, c->pin_out.ensure(m, true));
  std::memcpy(up.h + o_ids, ids, 4 * m);
  std::memcpy(up.h + o_first, first_kf, 4 * m);
  if (const int rc = up.copy(c)) return rc;
  void* dact = nullptr;
  HIPCHK(c, c->scratch.take(m, &dact));
  HIPCHK(c, tc_cull_launch(state_of(db), reinterpret_cast<const int32_t*>(up.d + o_ids), reinterpret_cast<const int32_t*>(up.d + o_first), current_kf, n,
                           static_cast<uint8_t*>(dact), c->stream));
  HIPCHK(c, hipMemcpyAsync(c->pin_out.p, dact, m, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::memcpy(action, c->pin_out.p, m);
  return DSH_OK;
}

int dsh_track_close_frame(dsh_mpdb* db, const dsh_track_frame* frame, int N, const int32_t* frame_points, const uint8_t* outlier, int n_nodes,
                          const double* node_xyz, int32_t only_tracking, dsh_track_close_counts* out) {
  MPDB_ENTER("dsh_track_close_frame");
  if (!frame) return bad("frame is NULL");
  const std::string pe = trk_pose_error(*frame);
  if (!pe.empty()) return bad(pe);
  if (N < 0 || N > (1 << 20)) return bad("N outside 0 .. 2^20");
  if (N > 0 && (!frame_points || !outlier)) return bad("frame_points or outlier is NULL");
  for (int i = 0; i < N; i++)
    if (frame_points[i] < -1 || frame_points[i] >= db->P) return bad("frame_points[" + std::to_string(i) + "] is neither -1 nor a point of the store");
  if (node_xyz) {
    const std::string ne = nodes_error(db, n_nodes, node_xyz);
    if (!ne.empty()) return bad(ne);
  }
  if (!out) return bad("out is NULL");
  if (const int rc = dsh_enter(c, "dsh_track_close_frame")) return rc;

  // up: the counts (zero), the pose, the frame's ids and flags, the nodes
  Upload up;
  const size_t n = (size_t)N, nn = node_xyz ? (size_t)n_nodes : 0;
  const size_t o_cnt = up.a.take(sizeof(dsh_track_close_counts)), o_pose = up.a.take(sizeof(TrkProb)), o_fp = up.a.take(4 * n), o_out = up.a.take(n),
               o_nodes = up.a.take(24 * nn);
  if (const int rc = up.stage(c)) return rc;
  HIPCHK(c, c->pin_out.ensure(sizeof(dsh_track_close_counts), true));
  std::memset(up.h + o_cnt, 0, sizeof(dsh_track_close_counts));
  TrkProb pose;
  trk_fill_pose(pose, *frame);
  std::memcpy(up.h + o_pose, &pose, sizeof(pose));
  if (N > 0) {
    std::memcpy(up.h + o_fp, frame_points, 4 * n);
    std::memcpy(up.h + o_out, outlier, n);
  }
  if (nn > 0) std::memcpy(up.h + o_nodes, node_xyz, 24 * nn);
  if (const int rc = up.copy(c)) return rc;
  TcClose k;
  k.pose = reinterpret_cast<const TrkProb*>(up.d + o_pose);
  k.frame_points = reinterpret_cast<const int32_t*>(up.d + o_fp);
  k.outlier = reinterpret_cast<const uint8_t*>(up.d + o_out);
  k.node_xyz = nn > 0 ? reinterpret_cast<const double*>(up.d + o_nodes) : nullptr;
  k.ref_ids = db->d_ref_ids;
  k.normal = db->d_nrm;
  k.P = db->P; k.N = N; k.n_ref = db->n_ref_points; k.only_tracking = only_tracking;
  k.counts = reinterpret_cast<dsh_track_close_counts*>(const_cast<char*>(up.d + o_cnt));
  HIPCHK(c, tc_close_launch(state_of(db), k, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->pin_out.p, k.counts, sizeof(dsh_track_close_counts), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::memcpy(out, c->pin_out.p, sizeof(dsh_track_close_counts));
  return DSH_OK;
}

}  // extern "C"
