// Host side of the tracking searches (include/defslam_hip.h: dsh_search_by_projection_*): validation, one packed upload, the three
// launches of track_kernels.hip, one download.  The device plan of a search (trk_plan_*) is shared with dsh_local_map_search.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "track_problem.h"

std::string trk_pose_error(const dsh_track_frame& f) {
  if (!f.Tcw) return "Tcw is NULL";
  for (int k = 0; k < 4; k++)
    if (!std::isfinite(f.K[k]) || !std::isfinite(f.bounds[k])) return "K / bounds not finite";
  if (!(f.bounds[1] > f.bounds[0]) || !(f.bounds[3] > f.bounds[2])) return "empty image bounds";
  return "";
}

std::string trk_frame_error(const dsh_track_frame& f) {
  const std::string pe = trk_pose_error(f);
  if (!pe.empty()) return pe;
  if (f.grid_cols <= 0 || f.grid_rows <= 0 || (long long)f.grid_cols * f.grid_rows > TRK_MAX_CELLS) return "grid size outside 1 .. 8192 cells";
  if (f.levels <= 0 || f.levels > TRK_MAX_LEVELS || !f.scale_factors) return "levels outside 1 .. 32 or no scale factors";
  if (f.N < 0 || f.N > TRK_MAX_KEYPOINTS) return "N outside 0 .. 8192";
  if (f.N > 0 && (!f.kp || !f.octave || !f.desc || !f.state)) return "key point arrays are NULL";
  for (int j = 0; j < f.N; j++) {
    if (f.octave[j] < 0 || f.octave[j] > 127) return "key point octave outside 0 .. 127";
    if (f.state[j] > 2) return "key point state not 0, 1 or 2";
  }
  return "";
}

void trk_fill_pose(TrkProb& P, const dsh_track_frame& f) {
  std::memset(&P, 0, sizeof(P));
  for (int i = 0; i < 3; i++) {
    for (int k = 0; k < 3; k++) P.R[3 * i + k] = f.Tcw[4 * i + k];
    P.t[i] = f.Tcw[4 * i + 3];
    P.Ow[i] = f.Ow[i];
  }
  P.fx = f.K[0]; P.fy = f.K[1]; P.cx = f.K[2]; P.cy = f.K[3];
  P.minX = f.bounds[0]; P.maxX = f.bounds[1]; P.minY = f.bounds[2]; P.maxY = f.bounds[3];
}

void trk_fill_prob(TrkProb& P, const dsh_track_frame& f, int mode, float th, int Q) {
  trk_fill_pose(P, f);
  // Frame.cc:97-98: mfGridElementWidthInv = float(FRAME_GRID_COLS) / (mnMaxX - mnMinX)
  P.winv = (float)f.grid_cols / (P.maxX - P.minX);
  P.hinv = (float)f.grid_rows / (P.maxY - P.minY);
  P.logsf = f.log_scale_factor;
  P.th = th;
  for (int l = 0; l < f.levels; l++) P.sf[l] = f.scale_factors[l];
  P.cols = f.grid_cols; P.rows = f.grid_rows; P.levels = f.levels; P.mode = mode;
  P.N = f.N; P.Q = Q;
}

void trk_plan_layout(TrkPlan& pl, UpBlock& up, DownBlock& down, size_t B, size_t Nt, size_t Qt, size_t Ct) {
  pl.B = B; pl.Nt = Nt; pl.Qt = Qt; pl.Ct = Ct;
  pl.o_prob = up.take(sizeof(TrkProb) * B); pl.o_kp = up.take(8 * Nt); pl.o_km = up.take(4 * Nt); pl.o_kd = up.take(32 * Nt);
  pl.d_match = down.take(4 * Qt); pl.d_level = down.take(4 * Qt); pl.d_inview = down.take(4 * Qt); pl.d_uv = down.take(8 * Qt);
  pl.d_vcos = down.take(4 * Qt); pl.d_pstat = down.take(16 * B);
}

void trk_plan_pack_frame(const TrkPlan& pl, UpBlock& up, int p, const TrkProb& P, const dsh_track_frame& f) {
  up.host<TrkProb>(pl.o_prob)[p] = P;
  if (f.N <= 0) return;
  const size_t N = (size_t)f.N, at = (size_t)P.kp_off;
  up.copy_of(pl.o_kp + 8 * at, f.kp, 8 * N);
  int32_t* km = up.host<int32_t>(pl.o_km) + at;   // octave and state share a word
  for (size_t j = 0; j < N; j++) km[j] = f.octave[j] | ((int32_t)f.state[j] << 8);
  up.copy_of(pl.o_kd + 32 * at, f.desc, 32 * N);
}

int trk_plan_device(dsh_ctx_base* c, const TrkPlan& pl, UpBlock& up, DownBlock& down, TrkBufs& b) {
  if (const int rc = up.send(c)) return rc;
  HIPCHK(c, dsh_scratch_array(c, &b.cell_start, pl.Ct));
  HIPCHK(c, dsh_scratch_array(c, &b.skp, pl.Nt));
  HIPCHK(c, dsh_scratch_array(c, &b.smeta, pl.Nt));
  HIPCHK(c, dsh_scratch_array(c, &b.sdesc, 2 * pl.Nt));
  HIPCHK(c, dsh_scratch_array(c, &b.keys, TRK_K * pl.Qt));
  HIPCHK(c, dsh_scratch_array(c, &b.ncand, pl.Qt));
  HIPCHK(c, dsh_scratch_array(c, &b.win, pl.Qt));
  if (const int rc = down.alloc(c)) return rc;
  b.pstat = down.dev<int32_t>(pl.d_pstat);
  HIPCHK(c, hipMemsetAsync(b.pstat, 0, 16 * pl.B, c->stream));
  b.prob = up.dev<const TrkProb>(pl.o_prob);
  b.kp = up.dev<const float2>(pl.o_kp);
  b.kmeta = up.dev<const int32_t>(pl.o_km);
  b.kdesc = up.dev<const uint4>(pl.o_kd);
  b.match = down.dev<int32_t>(pl.d_match);
  b.level = down.dev<int32_t>(pl.d_level);
  b.inview = down.dev<int32_t>(pl.d_inview);
  b.uv = down.dev<float>(pl.d_uv);
  b.vcos = down.dev<float>(pl.d_vcos);
  return DSH_OK;
}

int trk_plan_refused(const TrkPlan& pl, const DownBlock& down) {
  const int32_t* pstat = down.host<int32_t>(pl.d_pstat);
  for (size_t p = 0; p < pl.B; p++)
    if (pstat[4 * p + 2]) return (int)p;
  return -1;
}

extern "C" {

int dsh_search_by_projection_batch(dsh_ctx* ctx, int B, dsh_track_problem* problems) {
  dsh_ctx_base* c = dsh_base(ctx);
  if (!c) return DSH_ERR_ARG;
  if (B < 0 || (B > 0 && !problems)) return dsh_fail(c, DSH_ERR_ARG, "dsh_search_by_projection: bad batch");
  // validation, sizes and offsets
  long long Nt = 0, Qt = 0, Ct = 0;
  for (int p = 0; p < B; p++) {
    dsh_track_problem& pr = problems[p];
    auto bad = [&](const std::string& m) { return dsh_fail(c, DSH_ERR_ARG, "dsh_search_by_projection: problem " + std::to_string(p) + ": " + m); };
    DSH_CHECK(trk_frame_error(pr.frame));
    if (pr.mode != DSH_TRACK_FRAME && pr.mode != DSH_TRACK_LOCAL) return bad("mode is neither DSH_TRACK_FRAME nor DSH_TRACK_LOCAL");
    if (!(pr.th > 0.0f) || !std::isfinite(pr.th)) return bad("th must be a positive finite number");
    if (pr.Q < 0) return bad("Q < 0");
    if (pr.Q > 0 && (!pr.xyz || !pr.desc || !pr.match)) return bad("query arrays are NULL");
    if (pr.Q > 0 && pr.mode == DSH_TRACK_FRAME) {
      if (!pr.octave) return bad("frame to frame needs the query octaves");
      for (int q = 0; q < pr.Q; q++)
        if (pr.octave[q] < 0 || pr.octave[q] >= pr.frame.levels) return bad("query octave outside 0 .. levels-1");
    }
    if (pr.Q > 0 && pr.mode == DSH_TRACK_LOCAL && (!pr.normal || !pr.max_distance)) return bad("the local map needs normals and max distances");
    Nt += pr.frame.N;
    Qt += pr.Q;
    Ct += (long long)pr.frame.grid_cols * pr.frame.grid_rows + 1;
  }
  if (Qt > (1LL << 28) || Nt > (1LL << 28)) return dsh_fail(c, DSH_ERR_ARG, "dsh_search_by_projection: batch too large");
  for (int p = 0; p < B; p++) problems[p].nmatches = problems[p].rescans = 0;
  // arguments first, so that a host-only context reports bad ones too
  if (const int rc = dsh_enter(c, "dsh_search_by_projection")) return rc;
  if (B == 0) return DSH_OK;

  // one host buffer, one copy up: problem descriptors, key points, queries; one copy down: match, level, in view, uv, view cos, counters
  UpBlock up;
  DownBlock down;
  TrkPlan pl;
  trk_plan_layout(pl, up, down, (size_t)B, (size_t)Nt, (size_t)Qt, (size_t)Ct);
  const size_t o_qpid = up.take(4 * Qt), o_qxyz = up.take(12 * Qt), o_qnrm = up.take(12 * Qt), o_qmaxd = up.take(4 * Qt), o_qmeta = up.take(4 * Qt),
               o_qdesc = up.take(32 * Qt);
  if (const int rc = up.stage(c)) return rc;
  long long kp_off = 0, q_off = 0, cell_off = 0;
  for (int p = 0; p < B; p++) {
    const dsh_track_problem& pr = problems[p];
    const dsh_track_frame& f = pr.frame;
    TrkProb P;
    trk_fill_prob(P, f, pr.mode, pr.th, pr.Q);
    P.kp_off = (int32_t)kp_off; P.q_off = (int32_t)q_off; P.cell_off = (int32_t)cell_off;
    trk_plan_pack_frame(pl, up, p, P, f);
    const size_t Q = (size_t)pr.Q, q0 = (size_t)q_off;
    const bool local = pr.mode == DSH_TRACK_LOCAL;
    int32_t* qpid = up.host<int32_t>(o_qpid) + q_off;   // the problem of each query, and its octave or its skip flag
    int32_t* qmeta = up.host<int32_t>(o_qmeta) + q_off;
    for (int q = 0; q < pr.Q; q++) {
      qpid[q] = p;
      qmeta[q] = local ? (pr.skip && pr.skip[q] ? 1 : 0) : pr.octave[q];
    }
    up.copy_of(o_qxyz + 12 * q0, pr.xyz, 12 * Q);
    up.copy_of(o_qnrm + 12 * q0, local ? pr.normal : nullptr, 12 * Q);
    up.copy_of(o_qmaxd + 4 * q0, local ? pr.max_distance : nullptr, 4 * Q);
    up.copy_of(o_qdesc + 32 * q0, pr.desc, 32 * Q);
    // down: the local map's extras only for a local search
    down.copy_to(pl.d_match + 4 * q0, pr.match, 4 * Q);
    down.copy_to(pl.d_level + 4 * q0, local ? pr.level : nullptr, 4 * Q);
    down.copy_to(pl.d_uv + 8 * q0, local ? pr.uv : nullptr, 8 * Q);
    down.copy_to(pl.d_vcos + 4 * q0, local ? pr.view_cos : nullptr, 4 * Q);
    kp_off += f.N;
    q_off += pr.Q;
    cell_off += (long long)f.grid_cols * f.grid_rows + 1;
  }

  hipStream_t st = c->stream;
  TrkBufs b;
  if (const int rc = trk_plan_device(c, pl, up, down, b)) return rc;
  b.qpid = up.dev<const int32_t>(o_qpid);
  b.qxyz = up.dev<const float>(o_qxyz);
  b.qnrm = up.dev<const float>(o_qnrm);
  b.qmaxd = up.dev<const float>(o_qmaxd);
  b.qmeta = up.dev<const int32_t>(o_qmeta);
  b.qdesc = up.dev<const uint4>(o_qdesc);
  HIPCHK(c, trk_launch(b, B, (int)Qt, st));
  if (const int rc = down.fetch(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(st));

  const int refused = trk_plan_refused(pl, down);
  if (refused >= 0)   // a refused batch leaves the callers' arrays
    return dsh_fail(c, DSH_ERR_ARG, "dsh_search_by_projection: problem " + std::to_string(refused) + ": " TRK_REFUSED);
  down.hand_out();
  const int32_t* pstat = down.host<int32_t>(pl.d_pstat);
  q_off = 0;
  for (int p = 0; p < B; p++) {
    dsh_track_problem& pr = problems[p];
    if (pr.mode == DSH_TRACK_LOCAL && pr.in_view) {   // int32 on the device, uint8 for the caller
      const int32_t* iv = down.host<int32_t>(pl.d_inview) + q_off;
      for (int q = 0; q < pr.Q; q++) pr.in_view[q] = (uint8_t)iv[q];
    }
    pr.nmatches = pstat[4 * p];
    pr.rescans = pstat[4 * p + 1];
    q_off += pr.Q;
  }
  return DSH_OK;
}

int dsh_search_by_projection_frame(dsh_ctx* ctx, const dsh_track_frame* frame, int Q, const float* xyz, const int32_t* octave,
                                   const uint8_t* desc, float th, int32_t* match, int32_t* nmatches) {
  dsh_ctx_base* c = dsh_base(ctx);
  if (!c) return DSH_ERR_ARG;
  if (!frame) return dsh_fail(c, DSH_ERR_ARG, "dsh_search_by_projection_frame: frame is NULL");
  dsh_track_problem pr;
  std::memset(&pr, 0, sizeof(pr));
  pr.frame = *frame;
  pr.mode = DSH_TRACK_FRAME;
  pr.th = th;
  pr.Q = Q;
  pr.xyz = xyz;
  pr.octave = octave;
  pr.desc = desc;
  pr.match = match;
  const int rc = dsh_search_by_projection_batch(ctx, 1, &pr);
  if (rc == DSH_OK && nmatches) *nmatches = pr.nmatches;
  return rc;
}

int dsh_search_by_projection_local(dsh_ctx* ctx, const dsh_track_frame* frame, int Q, const float* xyz, const float* normal,
                                   const float* max_distance, const uint8_t* desc, const uint8_t* skip, float th, int32_t* match,
                                   uint8_t* in_view, int32_t* level, int32_t* nmatches) {
  dsh_ctx_base* c = dsh_base(ctx);
  if (!c) return DSH_ERR_ARG;
  if (!frame) return dsh_fail(c, DSH_ERR_ARG, "dsh_search_by_projection_local: frame is NULL");
  dsh_track_problem pr;
  std::memset(&pr, 0, sizeof(pr));
  pr.frame = *frame;
  pr.mode = DSH_TRACK_LOCAL;
  pr.th = th;
  pr.Q = Q;
  pr.xyz = xyz;
  pr.normal = normal;
  pr.max_distance = max_distance;
  pr.desc = desc;
  pr.skip = skip;
  pr.match = match;
  pr.in_view = in_view;
  pr.level = level;
  const int rc = dsh_search_by_projection_batch(ctx, 1, &pr);
  if (rc == DSH_OK && nmatches) *nmatches = pr.nmatches;
  return rc;
}

}  // extern "C"
