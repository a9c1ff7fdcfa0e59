// Host side of the rigid pose-only optimisation on the map point store (include/defslam_hip.h: dsh_track_pose_only,
// dsh_track_pose_only_batch): validation against the host mirror, one upload of the whole batch, the one launch of
// poseonly_kernels.hip and one download of the flags and the result records.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <string>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "mpdb_store.h"
#include "poseonly_problem.h"

// the layout tests/test_pose_only_cpu.py expects of the ctypes mirror
static_assert(sizeof(dsh_pose_only_problem) == 296 && offsetof(dsh_pose_only_problem, Tcw_out) == 80 && offsetof(dsh_pose_only_problem, pose) == 144 &&
                  offsetof(dsh_pose_only_problem, chi2) == 264,
              "dsh_pose_only_problem: layout");

namespace {

// Both entry points: `who` names the one that was called in every message, `one` leaves the problem index out of them.
int pose_only_run(dsh_mpdb* db, int B, dsh_pose_only_problem* problems, const char* who, bool one) {
  DSH_STORE_ENTER(who);
  size_t n_kp = 0, n_sig = 0;
  for (int k = 0; k < B; k++) {
    const dsh_pose_only_problem& p = problems[k];
    const std::string at = one ? std::string() : "problem " + std::to_string(k) + ": ";
    if (!p.Tcw) return bad(at + "Tcw is NULL");
    if (p.N < 0 || p.N > PO_MAX_KEYPOINTS) return bad(at + "N outside 0 .. 8192");
    if (p.levels < 1 || p.levels > PO_MAX_LEVELS) return bad(at + "levels outside 1 .. 32");
    if (!p.inv_level_sigma2) return bad(at + "inv_level_sigma2 is NULL");
    if (p.N > 0 && (!p.kp || !p.octave || !p.frame_points || !p.outlier)) return bad(at + "kp, octave, frame_points or outlier is NULL");
    const std::string te = mpdb_table_error(db, p.N, p.frame_points, "frame_points[", "]");
    if (!te.empty()) return bad(at + te);
    for (int i = 0; i < p.N; i++)
      if (p.frame_points[i] >= 0 && (p.octave[i] < 0 || p.octave[i] >= p.levels))
        return bad(at + "octave[" + std::to_string(i) + "] outside 0 .. levels-1");
    n_kp += (size_t)p.N;
    n_sig += (size_t)p.levels;
  }
  DSH_STORE_GATE();
  if (B == 0) return DSH_OK;

  // up: the poses, key points, octaves, sigma tables and ids of the whole batch; down: the flags and the result records
  UpBlock up;
  DownBlock down;
  const size_t nb = (size_t)B;
  const size_t o_prob = up.take(sizeof(PoProb) * nb), o_kp = up.take(8 * n_kp), o_oct = up.take(4 * n_kp), o_ids = up.take(4 * n_kp),
               o_sig = up.take(4 * n_sig);
  const size_t d_res = down.take(sizeof(PoResult) * nb), d_state = down.take(n_kp);
  if (const int rc = up.stage(c)) return rc;
  size_t kp0 = 0, sig0 = 0;
  for (int k = 0; k < B; k++) {
    const dsh_pose_only_problem& p = problems[k];
    PoProb& r = up.host<PoProb>(o_prob)[k];   // the problem's record is packed from fields
    std::memcpy(r.Tcw, p.Tcw, sizeof r.Tcw);
    std::memcpy(r.K, p.K, sizeof r.K);
    r.N = p.N; r.levels = p.levels; r.kp0 = (int32_t)kp0; r.sig0 = (int32_t)sig0;
    const size_t n = (size_t)p.N;
    up.copy_of(o_kp + 8 * kp0, p.kp, 8 * n);
    up.copy_of(o_ids + 4 * kp0, p.frame_points, 4 * n);
    int32_t* oct = up.host<int32_t>(o_oct) + kp0;
    for (size_t i = 0; i < n; i++) oct[i] = p.frame_points[i] >= 0 ? p.octave[i] : 0;   // read only where a point is held
    up.copy_of(o_sig + 4 * sig0, p.inv_level_sigma2, 4 * (size_t)p.levels);
    kp0 += n;
    sig0 += (size_t)p.levels;
  }
  if (const int rc = up.send(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  PoBatch b;
  b.B = B;
  b.prob = up.dev<const PoProb>(o_prob);
  b.kp = up.dev<const float>(o_kp);
  b.octave = up.dev<const int32_t>(o_oct);
  b.ids = up.dev<const int32_t>(o_ids);
  b.sig = up.dev<const float>(o_sig);
  b.xyz = db->d_xyz;
  HIPCHK(c, dsh_scratch_array(c, &b.edge, 6 * n_kp));
  b.state = down.dev<uint8_t>(d_state);
  b.res = down.dev<PoResult>(d_res);
  HIPCHK(c, po_launch(b, c->stream));
  if (const int rc = down.fetch(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));

  kp0 = 0;
  for (int k = 0; k < B; k++) {   // the flags only where a point is held; the rest are fields of the problem's record
    dsh_pose_only_problem& p = problems[k];
    const PoResult& r = down.host<PoResult>(d_res)[k];
    const uint8_t* st = down.host<uint8_t>(d_state) + kp0;
    for (int i = 0; i < p.N; i++)
      if (p.frame_points[i] >= 0) p.outlier[i] = st[i];
    std::memcpy(p.Tcw_out, r.Tcw_out, sizeof p.Tcw_out);
    std::memcpy(p.pose, r.pose, sizeof p.pose);
    std::memcpy(p.chi2, r.chi2, sizeof p.chi2);
    p.n_initial = r.n_initial; p.n_bad = r.n_bad; p.n_good = r.n_good; p.rounds = r.rounds;
    std::memcpy(p.iters, r.iters, sizeof p.iters);
    std::memcpy(p.trials, r.trials, sizeof p.trials);
    std::memcpy(p.bad, r.bad, sizeof p.bad);
    kp0 += (size_t)p.N;
  }
  return DSH_OK;
}

}  // namespace

extern "C" {

int dsh_track_pose_only_batch(dsh_mpdb* db, int B, dsh_pose_only_problem* problems) {
  DSH_STORE_ENTER("dsh_track_pose_only_batch");
  if (B < 0 || B > PO_MAX_BATCH) return bad("B outside 0 .. 65536");
  if (B > 0 && !problems) return bad("problems is NULL");
  return pose_only_run(db, B, problems, who__, false);
}

int dsh_track_pose_only(dsh_mpdb* db, dsh_pose_only_problem* p) {
  DSH_STORE_ENTER("dsh_track_pose_only");
  if (!p) return bad("p is NULL");
  return pose_only_run(db, 1, p, who__, true);
}

}  // extern "C"
