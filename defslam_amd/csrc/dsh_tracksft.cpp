// Host side of Shape-from-Template on the map point store (include/defslam_hip.h: dsh_track_sft_observations, dsh_track_sft):
// validation against the host mirror, one upload of the frame, the one launch of tracksft_kernels.hip, one download of the table; then
// the one-problem path of dsh_sft_solve on that table (pack, plan, upload, run, download: dsh_api.cpp), the scatter of the flags and the
// repose of the store's points from the result's node positions in HBM.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/defslam_hip.h"
#include "dsh_sft_ctx.h"
#include "mpdb_store.h"
#include "tracksft_host.h"
#include "tracksft_problem.h"

// the layout tests/test_track_sft_cpu.py expects of the ctypes mirrors
static_assert(sizeof(dsh_track_sft_frame) == 136 && offsetof(dsh_track_sft_frame, xyz) == 96, "dsh_track_sft_frame: layout");
static_assert(sizeof(dsh_track_sft_table) == 64 && offsetof(dsh_track_sft_table, kp_index) == 16, "dsh_track_sft_table: layout");

namespace {

// Both entries up to the downloaded table: the checks in the order of the other store calls, the selection, the synchronise.  On DSH_OK
// the table lies in the host side of `down` (valid until the next DownBlock of the context is placed).
int select_rows(dsh_mpdb* db, const dsh_track_sft_frame* fp, bool solve, const char* who, DownBlock& down, TfTable& t) {
  DSH_STORE_ENTER(who);
  if (!fp) return bad("f is NULL");
  const dsh_track_sft_frame& f = *fp;
  if (f.N < 0 || f.N > TF_MAX_KEYPOINTS) return bad("N outside 0 .. 8192");
  if (f.levels < 1 || f.levels > TF_MAX_LEVELS) return bad("levels outside 1 .. 32");
  if (!f.inv_level_sigma2) return bad("inv_level_sigma2 is NULL");
  if (f.N > 0 && (!f.kp || !f.octave || !f.frame_points || !f.outlier)) return bad("kp, octave, frame_points or outlier is NULL");
  if (solve && (!f.Tcw || !f.xyz)) return bad("Tcw or xyz is NULL");
  if (solve && (f.max_iters < 0 || f.max_iters > DSH_MAX_ITERS)) return bad("max_iters outside 0 .. 64");
  DSH_CHECK(mpdb_table_error(db, f.N, f.frame_points, "frame_points[", "]"));
  for (int i = 0; i < f.N; i++)
    if (f.frame_points[i] >= 0 && (f.octave[i] < 0 || f.octave[i] >= f.levels)) return bad("octave[" + std::to_string(i) + "] outside 0 .. levels-1");
  const dsh_ctx* x = static_cast<const dsh_ctx*>(c);
  if (!x->tmpl.valid) return refuse(DSH_ERR_STATE, "no template");
  if (db->largest_node() >= x->tmpl.n)
    return bad("a stored node index (" + std::to_string(db->largest_node()) + ") is >= the " + std::to_string(x->tmpl.n) + " nodes of the template");
  DSH_STORE_GATE();
  t = TfTable{};
  if (f.N == 0) return DSH_OK;

  // up: the frame's ids, flags, octaves, key points and the sigma table; down: M and Points_Obs, then the table with room for N rows
  UpBlock up;
  const size_t n = (size_t)f.N;
  const size_t o_ids = up.copy_of(f.frame_points, 4 * n), o_out = up.copy_of(f.outlier, n), o_oct = up.take(4 * n), o_kp = up.copy_of(f.kp, 8 * n),
               o_sig = up.copy_of(f.inv_level_sigma2, 4 * (size_t)f.levels);
  const size_t d_head = down.take(8), d_idx = down.take(4 * n), d_pid = down.take(4 * n), d_nodes = down.take(12 * n), d_bary = down.take(24 * n),
               d_uv = down.take(16 * n), d_sig = down.take_exact(8 * n);
  if (const int rc = up.stage(c)) return rc;
  int32_t* oct = up.host<int32_t>(o_oct);
  for (size_t i = 0; i < n; i++) oct[i] = f.frame_points[i] >= 0 ? f.octave[i] : 0;   // read only where a point is held
  if (const int rc = up.send(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  TfSelect s;
  s.N = f.N;
  s.frame_points = up.dev<const int32_t>(o_ids);
  s.outlier = up.dev<const uint8_t>(o_out);
  s.octave = up.dev<const int32_t>(o_oct);
  s.kp = up.dev<const float>(o_kp);
  s.sig = up.dev<const float>(o_sig);
  s.bad = db->d_bad; s.nodes = db->d_nodes; s.bary = db->d_bary;
  s.head = down.dev<int32_t>(d_head);
  s.kp_index = down.dev<int32_t>(d_idx);
  s.point_id = down.dev<int32_t>(d_pid);
  s.row_nodes = down.dev<int32_t>(d_nodes);
  s.row_bary = down.dev<double>(d_bary);
  s.uv = down.dev<double>(d_uv);
  s.invsig2 = down.dev<double>(d_sig);
  HIPCHK(c, tf_select_launch(s, c->stream));
  if (const int rc = down.fetch(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  t.M = down.host<int32_t>(d_head)[0];
  t.points_obs = down.host<int32_t>(d_head)[1];
  t.kp_index = down.host<int32_t>(d_idx);
  t.point_id = down.host<int32_t>(d_pid);
  t.nodes = down.host<int32_t>(d_nodes);
  t.bary = down.host<double>(d_bary);
  t.uv = down.host<double>(d_uv);
  t.invsig2 = down.host<double>(d_sig);
  if (t.M < 0 || t.M > f.N) return refuse(DSH_ERR_HIP, "the selection returned a row count outside 0 .. N");
  return DSH_OK;
}

// "... observation m: its nodes are not joined ..." of the packer (sft_pack.cpp): m, or -1 for any other message
int refused_observation(const std::string& e) {
  const char* key = "observation ";
  const size_t at = e.find(key);
  if (at == std::string::npos || e.find("not joined by a mesh edge") == std::string::npos) return -1;
  const char* p = e.c_str() + at + std::strlen(key);
  char* end = nullptr;
  const long m = std::strtol(p, &end, 10);
  return end != p && *end == ':' && m >= 0 ? (int)m : -1;
}

}  // namespace

extern "C" {

int dsh_track_sft_observations(dsh_mpdb* db, const dsh_track_sft_frame* f, dsh_track_sft_table* out) {
  DSH_STORE_ENTER("dsh_track_sft_observations");
  if (!out) return bad("t is NULL");
  DownBlock down;
  TfTable t;
  if (const int rc = select_rows(db, f, false, who__, down, t)) return rc;
  if (!tf_table_fits(t, *out)) return bad("capacity (" + std::to_string(out->capacity) + ") < M (" + std::to_string(t.M) + ")");
  tf_hand_out(t, out);
  return DSH_OK;
}

int dsh_track_sft(dsh_mpdb* db, const dsh_track_sft_frame* f, int32_t write_back, dsh_track_sft_table* out, dsh_sft_result* r) {
  DSH_STORE_ENTER("dsh_track_sft");
  if (!r) return bad("r is NULL");
  DownBlock down;
  TfTable t;
  if (const int rc = select_rows(db, f, true, who__, down, t)) return rc;
  if (out && !tf_table_fits(t, *out)) return bad("capacity (" + std::to_string(out->capacity) + ") < M (" + std::to_string(t.M) + ")");
  dsh_ctx* x = static_cast<dsh_ctx*>(c);
  if (t.M == 0) {   // not the reference's numbers (an optimiser without observation edges): the input comes back
    if (out) tf_hand_out(t, out);
    r->rep_error = std::nan("");
    r->inliers = r->iters = r->trials = r->dim = r->half_bandwidth = r->status = 0;
    if (r->Tcw) std::memcpy(r->Tcw, f->Tcw, 16 * sizeof(float));
    if (r->pose7) dsh::pose7_from_Tcw(f->Tcw, r->pose7);
    if (r->xyz) std::memcpy(r->xyz, f->xyz, 24 * (size_t)x->tmpl.n);
    if (r->trace) std::memset(r->trace, 0, 8 * DSH_TRACE_STRIDE * (size_t)f->max_iters);
    return DSH_OK;
  }
  const dsh_sft_frame sf = tf_sft_frame(*f, t);
  dsh_sft_result rr = *r;
  std::vector<uint8_t> flags;
  if (!rr.outlier) {   // the scatter needs the flags whether the caller asked for them or not
    flags.resize((size_t)t.M);
    rr.outlier = flags.data();
  }
  if (const int rc = dsh_sft_solve(x, &sf, &rr)) {
    const int m = rc == DSH_ERR_ARG ? refused_observation(c->err) : -1;
    c->err = std::string(who__) + ": " + c->err;
    if (m >= 0 && m < t.M) c->err += " (key point " + std::to_string(t.kp_index[m]) + ")";
    return rc;
  }
  r->rep_error = rr.rep_error;
  r->inliers = rr.inliers; r->iters = rr.iters; r->trials = rr.trials; r->dim = rr.dim; r->half_bandwidth = rr.half_bandwidth; r->status = rr.status;
  if (out) tf_hand_out(t, out);
  tf_scatter_flags(t, rr.outlier, f->outlier);
  if (write_back && db->P > 0) {   // DefOptimizer.cc:568-576 from the result region of the batch arena
    const double* node_xyz = reinterpret_cast<const double*>(x->d_batch + x->layout.res_off + x->layout.res_offs[0].xyz);
    int32_t* moved = nullptr;
    HIPCHK(c, dsh_scratch_array(c, &moved, 1));
    HIPCHK(c, hipMemsetAsync(moved, 0, 4, c->stream));
    HIPCHK(c, tc_repose_launch(mpdb_state(db), db->P, node_xyz, moved, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return DSH_OK;
}

}  // extern "C"
