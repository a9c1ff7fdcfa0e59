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

namespace {

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
  DSH_STORE_ENTER("dsh_trackstate_set_embedding");
  DSH_CHECK(mpdb_ids_error(n, ids, db->P, "point id"));
  if (n > 0 && !nodes) return bad("nodes is NULL");
  bool any = false;
  for (int i = 0; i < n; i++) {
    const int32_t a = nodes[3 * i], b = nodes[3 * i + 1], d = nodes[3 * i + 2];
    if (a == -1 && b == -1 && d == -1) continue;
    if (!(0 <= a && a < b && b < d)) return bad("nodes of entry " + std::to_string(i) + " are neither -1 -1 -1 nor ascending and distinct");
    any = true;
  }
  if (any && !bary) return bad("bary is NULL");
  DSH_STORE_GATE();
  if (n == 0) return DSH_OK;
  UpBlock up;
  const size_t m = (size_t)n, o_ids = up.copy_of(ids, 4 * m), o_nodes = up.copy_of(nodes, 12 * m), o_bary = up.take(24 * m);
  up.copy_of(o_bary, bary, 24 * m);
  if (const int rc = up.stage(c)) return rc;
  if (!bary) std::memset(up.host<double>(o_bary), 0, 24 * m);   // no entry has a facet: the kernel still gets coordinates, zeros
  if (const int rc = up.send(c)) return rc;
  HIPCHK(c, tc_set_embedding_launch(mpdb_state(db), up.dev<const int32_t>(o_ids), up.dev<const int32_t>(o_nodes), up.dev<const double>(o_bary), n,
                                    c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < n; i++) {
    int32_t& top = db->top_node[ids[i]];
    if ((db->top_on_device || top == db->max_node) && nodes[3 * i + 2] < db->max_node) db->max_node_stale = true;
    top = nodes[3 * i + 2];
    if (!db->max_node_stale) db->max_node = std::max(db->max_node, top);
  }
  return DSH_OK;
}

int dsh_trackstate_clear_embedding(dsh_mpdb* db) {
  DSH_STORE_ENTER("dsh_trackstate_clear_embedding");
  DSH_STORE_GATE();
  HIPCHK(c, tc_set_embedding_launch(mpdb_state(db), nullptr, nullptr, nullptr, db->P, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::fill(db->top_node.begin(), db->top_node.end(), -1);
  db->max_node = -1;
  db->max_node_stale = false;
  db->top_on_device = false;
  return DSH_OK;
}

int dsh_trackstate_set_counters(dsh_mpdb* db, int n, const int32_t* ids, const int32_t* visible, const int32_t* found) {
  DSH_STORE_ENTER("dsh_trackstate_set_counters");
  DSH_CHECK(mpdb_ids_error(n, ids, db->P, "point id"));
  if (n > 0 && (!visible || !found)) return bad("visible or found is NULL");
  DSH_STORE_GATE();
  if (n == 0) return DSH_OK;
  UpBlock up;
  const size_t m = (size_t)n, o_ids = up.copy_of(ids, 4 * m), o_vis = up.copy_of(visible, 4 * m), o_fnd = up.copy_of(found, 4 * m);
  if (const int rc = up.copy(c)) return rc;
  HIPCHK(c, tc_set_counters_launch(mpdb_state(db), up.dev<const int32_t>(o_ids), up.dev<const int32_t>(o_vis), up.dev<const int32_t>(o_fnd), n,
                                   c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return DSH_OK;
}

int dsh_trackstate_get(dsh_mpdb* db, int n, const int32_t* ids, int32_t* visible, int32_t* found, int32_t* n_obs, float* xyz) {
  DSH_STORE_ENTER("dsh_trackstate_get");
  DSH_CHECK(mpdb_ids_error(n, ids, db->P, "point id"));
  DSH_STORE_GATE();
  if (n == 0) return DSH_OK;
  UpBlock up;
  const size_t m = (size_t)n, o_ids = up.copy_of(ids, 4 * m);
  DownBlock down;
  const size_t d_vis = down.copy_to(visible, 4 * m), d_fnd = down.copy_to(found, 4 * m), d_nobs = down.copy_to(n_obs, 4 * m),
               d_xyz = down.copy_to(xyz, 12 * m);
  if (const int rc = up.copy(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  HIPCHK(c, tc_get_launch(mpdb_state(db), up.dev<const int32_t>(o_ids), n, down.dev_if<int32_t>(visible, d_vis), down.dev_if<int32_t>(found, d_fnd),
                          down.dev_if<int32_t>(n_obs, d_nobs), down.dev_if<float>(xyz, d_xyz), c->stream));
  return down.receive(c);
}

int dsh_trackstate_seed_local_points(dsh_mpdb* db, int n, const int32_t* ids) {
  DSH_STORE_ENTER("dsh_trackstate_seed_local_points");
  DSH_CHECK(mpdb_ids_error(n, ids, db->P, "point id"));
  for (int i = 1; i < n; i++)
    if (ids[i] <= ids[i - 1]) return bad("ids are not ascending");
  DSH_STORE_GATE();
  if (n > 0) {
    UpBlock up;   // staged here, copied into both lists of the store: an exact slice, up.size is what the lists receive
    const size_t o_ids = up.take_exact(4 * (size_t)n);
    up.copy_of(o_ids, ids, up.size);
    if (const int rc = up.stage(c)) return rc;
    HIPCHK(c, hipMemcpyAsync(db->d_local_ids, up.host<int32_t>(o_ids), up.size, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(db->d_ref_ids, up.host<int32_t>(o_ids), up.size, hipMemcpyHostToDevice, c->stream));
  }
  const int32_t n32 = n;
  HIPCHK(c, hipMemcpyAsync(&db->d_hdr->n_local_points, &n32, 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  db->n_local_points = db->n_ref_points = n;
  return DSH_OK;
}

int dsh_trackstate_repose(dsh_mpdb* db, int n_nodes, const double* node_xyz, int32_t* n_moved) {
  DSH_STORE_ENTER("dsh_trackstate_repose");
  DSH_CHECK(nodes_error(db, n_nodes, node_xyz));
  DSH_STORE_GATE();
  if (n_moved) *n_moved = 0;
  if (n_nodes == 0 || db->P == 0) return DSH_OK;
  UpBlock up;
  const size_t o_cnt = up.take(4), o_nodes = up.copy_of(node_xyz, 24 * (size_t)n_nodes);
  DownBlock down;   // the counter comes down from where it went up as zero: an exact slice over the upload block
  const size_t d_cnt = down.take_exact(4);
  down.copy_to(d_cnt, n_moved, 4);
  if (const int rc = up.stage(c)) return rc;
  *up.host<int32_t>(o_cnt) = 0;
  if (const int rc = up.send(c)) return rc;
  if (const int rc = down.at(c, up.dev<int32_t>(o_cnt))) return rc;
  HIPCHK(c, tc_repose_launch(mpdb_state(db), db->P, up.dev<const double>(o_nodes), down.dev<int32_t>(d_cnt), c->stream));
  return down.receive(c);
}

int dsh_trackstate_cull(dsh_mpdb* db, int n, const int32_t* ids, const int32_t* first_kf, int32_t current_kf, uint8_t* action) {
  DSH_STORE_ENTER("dsh_trackstate_cull");
  DSH_CHECK(mpdb_ids_error(n, ids, db->P, "point id"));
  if (n > 0 && (!first_kf || !action)) return bad("first_kf or action is NULL");
  DSH_STORE_GATE();
  if (n == 0) return DSH_OK;
  UpBlock up;
  const size_t m = (size_t)n, o_ids = up.copy_of(ids, 4 * m), o_first = up.copy_of(first_kf, 4 * m);
  DownBlock down;
  const size_t d_act = down.copy_to(action, m);
  if (const int rc = up.copy(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  HIPCHK(c, tc_cull_launch(mpdb_state(db), up.dev<const int32_t>(o_ids), up.dev<const int32_t>(o_first), current_kf, n, down.dev<uint8_t>(d_act), c->stream));
  return down.receive(c);
}

int dsh_track_close_frame(dsh_mpdb* db, const dsh_track_frame* frame, int N, const int32_t* frame_points, const uint8_t* outlier, int n_nodes,
                          const double* node_xyz, int32_t only_tracking, dsh_track_close_counts* out) {
  DSH_STORE_ENTER("dsh_track_close_frame");
  if (!frame) return bad("frame is NULL");
  DSH_CHECK(trk_pose_error(*frame));
  DSH_CHECK(dsh_keypoint_count_error(N));
  if (N > 0 && (!frame_points || !outlier)) return bad("frame_points or outlier is NULL");
  DSH_CHECK(mpdb_table_error(db, N, frame_points, "frame_points[", "]"));
  if (node_xyz) DSH_CHECK(nodes_error(db, n_nodes, node_xyz));
  if (!out) return bad("out is NULL");
  DSH_STORE_GATE();

  // up: the counts (zero), the pose, the frame's ids and flags, the nodes
  UpBlock up;
  const size_t n = (size_t)N, nn = node_xyz ? (size_t)n_nodes : 0;
  const size_t o_cnt = up.take(sizeof(dsh_track_close_counts)), o_pose = up.take(sizeof(TrkProb)), o_fp = up.copy_of(frame_points, 4 * n),
               o_out = up.copy_of(outlier, n), o_nodes = up.copy_of(node_xyz, 24 * nn);
  DownBlock down;   // the counts come down from where they went up as zeros: an exact slice over the upload block
  const size_t d_cnt = down.take_exact(sizeof(dsh_track_close_counts));
  down.copy_to(d_cnt, out, sizeof(dsh_track_close_counts));
  if (const int rc = up.stage(c)) return rc;
  std::memset(up.host<dsh_track_close_counts>(o_cnt), 0, sizeof(dsh_track_close_counts));   // the counters go up as zeros
  trk_fill_pose(*up.host<TrkProb>(o_pose), *frame);                                         // the pose is packed, not copied
  if (const int rc = up.send(c)) return rc;
  if (const int rc = down.at(c, up.dev<dsh_track_close_counts>(o_cnt))) return rc;
  TcClose k;
  k.pose = up.dev<const TrkProb>(o_pose);
  k.frame_points = up.dev<const int32_t>(o_fp);
  k.outlier = up.dev<const uint8_t>(o_out);
  k.node_xyz = nn > 0 ? up.dev<const double>(o_nodes) : nullptr;
  k.ref_ids = db->d_ref_ids;
  k.normal = db->d_nrm;
  k.P = db->P; k.N = N; k.n_ref = db->n_ref_points; k.only_tracking = only_tracking;
  k.counts = down.dev<dsh_track_close_counts>(d_cnt);
  HIPCHK(c, tc_close_launch(mpdb_state(db), k, c->stream));
  return down.receive(c);
}

}  // extern "C"
