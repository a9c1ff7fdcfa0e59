// Host side of the end of a tracked frame and of the motion-model search on the map point store (include/defslam_hip.h:
// dsh_track_end_frame, dsh_track_last_frame, dsh_motion_model_search): validation against the host mirror, per call one upload, the
// launches of motionmodel_kernels.hip (and, for the search, of track_kernels.hip) and one download.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "motionmodel_problem.h"
#include "mpdb_store.h"
#include "track_problem.h"

extern "C" {

int dsh_track_end_frame(dsh_mpdb* db, int N, const int32_t* frame_points, const uint8_t* outlier, const int32_t* octave, int32_t* points_out,
                        uint8_t* outlier_out, dsh_track_end_counts* out) {
  DSH_STORE_ENTER("dsh_track_end_frame");
  if (N < 0 || N > TRK_MAX_KEYPOINTS) return bad("N outside 0 .. 8192");
  if (N > 0 && (!frame_points || !outlier || !octave)) return bad("frame_points, outlier or octave is NULL");
  DSH_CHECK(mpdb_table_error(db, N, frame_points, "frame_points[", "]"));
  for (int i = 0; i < N; i++)
    if (octave[i] < 0 || octave[i] > 127) return bad("octave[" + std::to_string(i) + "] outside 0 .. 127");
  DSH_STORE_GATE();
  HIPCHK(c, mpdb_reserve_last_frame(db, std::max(N, 1)));

  // up: the frame's ids, flags and octaves; down: the state after CleanMatches and the counts
  UpBlock up;
  DownBlock down;
  const size_t n = (size_t)N, o_fp = up.copy_of(frame_points, 4 * n), o_out = up.copy_of(outlier, n), o_oct = up.copy_of(octave, 4 * n);
  const size_t d_cnt = down.take(16), d_pts = down.take(4 * n), d_flag = down.take(n);
  down.copy_to(d_pts, points_out, 4 * n);   // the kernel writes both whether the caller wants them or not
  down.copy_to(d_flag, outlier_out, n);
  if (const int rc = up.copy(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  MmEnd e;
  e.N = N;
  e.frame_points = up.dev<const int32_t>(o_fp);
  e.outlier = up.dev<const uint8_t>(o_out);
  e.octave = up.dev<const int32_t>(o_oct);
  e.nobs = db->d_nobs;
  e.last_ids = db->d_last_ids;
  e.last_oct = db->d_last_oct;
  e.cand_ids = db->d_cand_ids;
  e.points_out = down.dev<int32_t>(d_pts);
  e.outlier_out = down.dev<uint8_t>(d_flag);
  e.counts = down.dev<int32_t>(d_cnt);
  db->last_N = db->cand_N = -1;   // the list and the candidate are being overwritten: they count again once the call has succeeded
  HIPCHK(c, mm_end_frame_launch(e, c->stream));
  if (const int rc = down.receive(c)) return rc;

  const int32_t* cnt = down.host<int32_t>(d_cnt);
  db->last_N = db->cand_N = N;
  db->last_kept = cnt[2];
  db->last_max_octave = cnt[3];
  if (out) { out->cleaned = cnt[0]; out->dropped = cnt[1]; out->kept = cnt[2]; }
  return DSH_OK;
}

int dsh_track_last_frame(dsh_mpdb* db, int32_t capacity, int32_t* ids, int32_t* octave, int32_t* n) {
  DSH_STORE_ENTER("dsh_track_last_frame");
  if (capacity < 0) return bad("capacity < 0");
  DSH_STORE_GATE();
  if (db->last_N < 0) return bad("no resident last-frame list (dsh_track_end_frame has not run since the store was created or cleared)");
  if (capacity < db->last_N) return bad("capacity is smaller than the last-frame list");
  const size_t bytes = 4 * (size_t)db->last_N;
  if (bytes > 0) {
    if (ids) HIPCHK(c, hipMemcpyAsync(ids, db->d_last_ids, bytes, hipMemcpyDeviceToHost, c->stream));
    if (octave) HIPCHK(c, hipMemcpyAsync(octave, db->d_last_oct, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (n) *n = db->last_N;
  return DSH_OK;
}

int dsh_motion_model_search(dsh_mpdb* db, const dsh_track_frame* frame, float th, float th_wide, int32_t min_matches, int32_t* frame_points,
                            int32_t* match, int32_t* nmatches, float* th_used) {
  DSH_STORE_ENTER("dsh_motion_model_search");
  if (!frame) return bad("frame is NULL");
  if (frame->N < 0 || frame->N > TRK_MAX_KEYPOINTS) return bad("N outside 0 .. 8192");
  // every key point enters empty (DefTracking.cc:352-353): frame->state is not read
  const std::vector<uint8_t> empty((size_t)std::max(frame->N, 1), 0);
  dsh_track_frame f = *frame;
  f.state = empty.data();
  DSH_CHECK(trk_frame_error(f));
  if (!(th > 0.0f) || !std::isfinite(th) || !(th_wide > 0.0f) || !std::isfinite(th_wide)) return bad("th and th_wide must be positive finite numbers");
  if (min_matches < 0) return bad("min_matches < 0");
  if (f.N > 0 && !frame_points) return bad("frame_points is NULL");
  DSH_STORE_GATE();
  if (db->last_N < 0) return bad("no resident last-frame list (dsh_track_end_frame has not run since the store was created or cleared)");
  if (db->last_max_octave >= f.levels)
    return bad("the last-frame list holds octave " + std::to_string(db->last_max_octave) + ", which is outside 0 .. levels-1");

  const int NL = db->last_N, Q = db->last_kept;
  auto empty_outputs = [&]() {
    for (int j = 0; j < f.N; j++) frame_points[j] = -1;
    if (match)
      for (int i = 0; i < NL; i++) match[i] = -1;
  };
  if (Q == 0) {
    // no query: both searches find nothing, and the second one runs when nothing is too few
    empty_outputs();
    if (nmatches) *nmatches = 0;
    if (th_used) *th_used = 0 < min_matches ? th_wide : th;
    return DSH_OK;
  }

  // up: the frame at both window factors; the queries are gathered from the store on the device; down: the matches with each query's
  // point and entry, and how many queries there were
  const size_t q = (size_t)Q;
  UpBlock up;
  DownBlock down;
  TrkPlan pl;
  trk_plan_layout(pl, up, down, 2, (size_t)f.N, q, (size_t)f.grid_cols * f.grid_rows + 1);
  const size_t d_ids = down.take(4 * q), d_idx = down.take(4 * q), d_count = down.take(4);
  if (const int rc = up.stage(c)) return rc;
  TrkProb pr;
  trk_fill_prob(pr, f, DSH_TRACK_FRAME, th, Q);
  trk_plan_pack_frame(pl, up, 0, pr, f);
  pr.th = th_wide;
  up.host<TrkProb>(pl.o_prob)[1] = pr;   // the same frame, grid and key points
  hipStream_t st = c->stream;
  TrkBufs b;
  if (const int rc = trk_plan_device(c, pl, up, down, b)) return rc;
  MmGather g;
  uint8_t* qfree = nullptr;
  HIPCHK(c, dsh_scratch_array(c, &g.qpid, q));
  HIPCHK(c, dsh_scratch_array(c, &g.qxyz, 3 * q));
  HIPCHK(c, dsh_scratch_array(c, &g.qmeta, q));
  HIPCHK(c, dsh_scratch_array(c, &g.qdesc, 2 * q));
  HIPCHK(c, dsh_scratch_array(c, &qfree, q));
  g.N = NL;
  g.last_ids = db->d_last_ids; g.last_oct = db->d_last_oct;
  g.xyz = db->d_xyz; g.desc = db->d_desc; g.bad = db->d_bad; g.nodes = db->d_nodes; g.nobs = db->d_nobs;
  g.qfree = qfree;
  g.out_ids = down.dev<int32_t>(d_ids);
  g.out_idx = down.dev<int32_t>(d_idx);
  g.out_count = down.dev<int32_t>(d_count);
  HIPCHK(c, mm_gather_launch(g, st));
  b.qpid = g.qpid; b.qxyz = g.qxyz; b.qnrm = nullptr; b.qmaxd = nullptr; b.qmeta = g.qmeta; b.qdesc = g.qdesc;
  b.qcount = g.out_count;
  b.qfree = qfree;
  HIPCHK(c, trk_launch(b, 1, Q, st));
  // the fresh search at th_wide (DefTracking.cc:364-370), behind the narrow one: it leaves at once when pstat[0], the narrow count, suffices
  TrkBufs w = b;
  w.prob = b.prob + 1;
  w.gate = b.pstat;
  w.gate_min = min_matches;
  HIPCHK(c, trk_launch_search(w, 1, Q, st));
  if (const int rc = down.fetch(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(st));

  if (down.host<int32_t>(pl.d_pstat)[2]) return bad(TRK_REFUSED);
  const int32_t* pstat = down.host<int32_t>(pl.d_pstat);
  const int32_t *qm = down.host<int32_t>(pl.d_match), *ids = down.host<int32_t>(d_ids), *idx = down.host<int32_t>(d_idx);
  const int nq = *down.host<int32_t>(d_count);
  empty_outputs();
  for (int k = 0; k < nq; k++) {   // in query order: the last writer owns the key point (DefORBmatcher.cc:406)
    if (qm[k] < 0) continue;
    frame_points[qm[k]] = ids[k];
    if (match) match[idx[k]] = qm[k];
  }
  if (nmatches) *nmatches = pstat[0];
  if (th_used) *th_used = pstat[3] ? th_wide : th;
  return DSH_OK;
}

}  // extern "C"
