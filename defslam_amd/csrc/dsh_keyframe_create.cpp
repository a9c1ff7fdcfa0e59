// Host side of the creation of a keyframe on the two resident stores and of its covisibility connections (include/defslam_hip.h:
// dsh_track_keyframe_candidate, dsh_keyframe_create, dsh_keyframe_update_connections): validation against the host mirrors of dsh_mpdb
// and dsh_kfdb, per call one upload block, the launches of keyframe_create_kernels.hip (and the snapshot of surfreg_kernels.hip) and
// one block down.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "keyframe_create_problem.h"
#include "kfdb_store.h"
#include "mpdb_store.h"
#include "surfreg_problem.h"

namespace {

// what is wrong with the input of dsh_keyframe_create, "" if nothing: decided on the two host mirrors, before any device work
std::string create_error(const dsh_mpdb* db, const dsh_keyframe_create_input* in, const dsh_keyframe_create_result* out) {
  if (!in) return "in is NULL";
  if (!out) return "out is NULL";
  if (!in->kfdb) return "kfdb is NULL";
  if (!in->kf) return "kf is NULL";
  if (!in->Tcw) return "Tcw is NULL";
  // the handle is looked up among the context's stores before it is read, as dsh_keyframe_set_pose does
  const dsh_ctx_base* c = db->ctx;
  if (std::find(c->stores.begin(), c->stores.end(), static_cast<const dsh_store*>(in->kfdb)) == c->stores.end())
    return "the keyframe store belongs to another context or was detached";
  if (in->kfdb->count != db->K)
    return "the keyframe store holds " + std::to_string(in->kfdb->count) + " keyframes and the point store " + std::to_string(db->K) + ": the new slot must be the same in both";
  const std::string ke = kfdb_keyframe_error(in->kfdb, in->kf);
  if (!ke.empty()) return ke;
  const int32_t N = in->kf->N;
  if (N > KC_MAX_KEYPOINTS) return "N outside 0 .. 8192";
  if (db->K >= KC_MAX_KEYFRAMES) return "the store holds 65535 keyframes already";
  if (db->T + N > INT32_MAX) return "store full";
  for (int i = 0; i < 16; i++)
    if (!std::isfinite(in->Tcw[i])) return "Tcw is not finite";
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(sr_camera_centre(in->Tcw, k))) return "camera centre not finite";
  if (in->points) {
    const std::string te = mpdb_table_error(db, N, in->points, "table entry ", "");
    if (!te.empty()) return te;
  } else {
    if (db->cand_N < 0) return "points is NULL and there is no resident keyframe candidate (dsh_track_end_frame has not run since the store was created or cleared)";
    if (db->cand_N != N) return "the resident keyframe candidate has " + std::to_string(db->cand_N) + " entries, kf->N is " + std::to_string(N);
  }
  if (in->kpn)
    for (size_t i = 0; i < 2 * (size_t)N; i++)
      if (!std::isfinite(in->kpn[i])) return "key point " + std::to_string(i / 2) + " is not finite";
  return "";
}

}  // namespace

extern "C" {

int dsh_track_keyframe_candidate(dsh_mpdb* db, int32_t capacity, int32_t* ids, int32_t* n) {
  DSH_STORE_ENTER("dsh_track_keyframe_candidate");
  if (capacity < 0) return bad("capacity < 0");
  DSH_STORE_GATE();
  if (db->cand_N < 0) return bad("no resident keyframe candidate (dsh_track_end_frame has not run since the store was created or cleared)");
  if (capacity < db->cand_N) return bad("capacity is smaller than the keyframe candidate");
  if (db->cand_N > 0 && ids) {
    HIPCHK(c, hipMemcpyAsync(ids, db->d_cand_ids, 4 * (size_t)db->cand_N, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (n) *n = db->cand_N;
  return DSH_OK;
}

int dsh_keyframe_create(dsh_mpdb* db, const dsh_keyframe_create_input* in, dsh_keyframe_create_result* out) {
  DSH_STORE_ENTER("dsh_keyframe_create");
  DSH_CHECK(create_error(db, in, out));
  DSH_STORE_GATE();
  dsh_kfdb* kfdb = in->kfdb;
  const dsh_mp_keyframe& kf = *in->kf;
  const size_t N = (size_t)kf.N;
  // growth, as in the four calls this one stands for
  HIPCHK(c, kfdb_reserve(kfdb, kf.N));
  HIPCHK(c, mpdb_reserve_keyframes(db, (long long)db->K + 1));
  HIPCHK(c, mpdb_reserve_table(db, db->T + kf.N));
  dsh_kfdb::Kf mirror = kfdb_mirror(kfdb, &kf, false);

  // one block up; its last slice goes up as zeros and comes down as the result
  UpBlock up;
  const size_t o_rows = up.copy_of(kf.desc, 32 * N), o_oct = up.copy_of(mirror.octave.data(), N), o_sf = up.copy_of(mirror.sf, sizeof(mirror.sf)),
               o_T = up.copy_of(in->Tcw, 64), o_pts = up.copy_of(in->points, 4 * N), o_kpn = up.copy_of(in->kpn, 8 * N),
               o_out = up.take_exact(sizeof(KcCreateOut));
  DownBlock down;
  const size_t d_out = down.take_exact(sizeof(KcCreateOut));
  if (const int rc = up.stage(c)) return rc;
  std::memset(up.host<KcCreateOut>(o_out), 0, sizeof(KcCreateOut));   // the result goes up as zeros
  if (const int rc = up.send(c)) return rc;
  if (const int rc = down.at(c, up.dev<KcCreateOut>(o_out))) return rc;

  const int32_t slot = db->K;
  KcCreate k;
  k.N = kf.N; k.levels = kf.levels;
  k.src_rows = up.dev<const uint4>(o_rows);
  k.src_oct = up.dev<const int8_t>(o_oct);
  k.src_sf = up.dev<const float>(o_sf);
  k.Tcw = up.dev<const float>(o_T);
  k.src_points = in->points ? up.dev<const int32_t>(o_pts) : db->d_cand_ids;   // device to device: the host mirror holds no table contents
  k.src_kpn = up.dev_if<const float>(in->kpn, o_kpn);
  k.kf_slot = kfdb->d_slots + slot;
  k.row_off = (int32_t)kfdb->rows;
  k.rows = kfdb->d_rows; k.oct = kfdb->d_oct;
  k.levels_out = kfdb->d_levels + slot;
  k.sf = kfdb->d_sf + MPU_MAX_LEVELS * (size_t)slot;
  k.kf = db->d_kf + slot;
  k.tab_off = (int32_t)db->T;
  k.table = db->d_table; k.snap_point = db->d_snap_point;
  k.surf_normal = db->d_surf_normal; k.surf_pts = db->d_surf_pts; k.surf_kpn = db->d_surf_kpn; k.surf_has = db->d_surf_has;
  k.surf_nn = db->d_surf_nn + slot;
  k.out = up.dev<KcCreateOut>(o_out);
  HIPCHK(c, kc_create_launch(k, c->stream));
  // DefKeyFrame.cc:60-74 on the table the launch above wrote
  SrKeyframe s;
  s.N = kf.N; s.tab_off = k.tab_off; s.table = db->d_table; s.snap_point = db->d_snap_point; s.snap_xyz = db->d_snap_xyz;
  HIPCHK(c, sr_snapshot_launch(mpdb_state(db), s, &k.out->n_snapshot, c->stream));
  if (const int rc = down.receive(c)) return rc;

  // the mirrors, as dsh_kfdb_add, dsh_mpdb_add_keyframe, dsh_keyframe_snapshot_positions and dsh_keyframe_surface_init leave them
  kfdb_push(kfdb, std::move(mirror));
  LmKf m;
  m.tab_off = k.tab_off; m.N = kf.N; m.parent = -1; m.bad = 0;
  db->kf.push_back(m);
  db->snapped.push_back(1);
  db->surf.emplace_back();
  db->surf.back().has_surface = in->kpn ? 1 : 0;
  db->first_conn.push_back(1);
  db->K++;
  db->T += kf.N;
  const KcCreateOut& r = *down.host<KcCreateOut>(d_out);
  out->slot = slot; out->n_held = r.n_held; out->n_snapshot = r.n_snapshot;
  std::memcpy(out->Ow, r.Ow, 12);   // a field of the result record
  return DSH_OK;
}

int dsh_keyframe_update_connections(dsh_mpdb* db, int32_t slot, int32_t th, int32_t capacity, int32_t* counted_kf, int32_t* counted_w, int32_t* ordered_kf,
                                    int32_t* ordered_w, dsh_keyframe_connections* out) {
  DSH_STORE_ENTER("dsh_keyframe_update_connections");
  if (slot < 0 || slot >= db->K) return bad("slot outside the store");
  if (th < 1) return bad("th < 1");
  if ((counted_kf || counted_w || ordered_kf || ordered_w) && capacity < db->K) return bad("capacity is smaller than the store's keyframe count");
  if (db->kf[slot].N > KC_MAX_KEYPOINTS) return bad("the keyframe has more than 8192 key points");
  if (db->K > KC_MAX_KEYFRAMES) return bad("the store holds more than 65535 keyframes");
  DSH_STORE_GATE();

  const size_t K = (size_t)db->K;
  DownBlock down;
  const size_t d_hdr = down.take(sizeof(KcConnOut)), d_ck = down.take(4 * K), d_cw = down.take(4 * K), d_ok = down.take(4 * K), d_ow = down.take_exact(4 * K);
  KcConn k;
  HIPCHK(c, dsh_scratch_array(c, &k.cnt, (size_t)db->P));
  HIPCHK(c, dsh_scratch_array(c, &k.w, K));
  if (const int rc = down.alloc(c)) return rc;
  k.P = db->P; k.K = db->K; k.slot = slot; k.th = th; k.first = db->first_conn[slot];
  k.tab_off = db->kf[slot].tab_off; k.N = db->kf[slot].N;
  k.R = db->R;
  k.bad = db->d_bad; k.log = db->d_log; k.kf = db->d_kf; k.table = db->d_table;
  k.hdr = down.dev<KcConnOut>(d_hdr);
  k.counted_kf = down.dev<int32_t>(d_ck); k.counted_w = down.dev<int32_t>(d_cw);
  k.ordered_kf = down.dev<int32_t>(d_ok); k.ordered_w = down.dev<int32_t>(d_ow);
  HIPCHK(c, kc_connections_launch(k, c->stream));
  if (const int rc = down.receive(c)) return rc;

  const KcConnOut h = *down.host<KcConnOut>(d_hdr);
  if (h.parent_set) {   // KeyFrame.cc:412-417: the mirror follows the device
    db->kf[slot].parent = h.parent;
    db->first_conn[slot] = 0;
  }
  // the lists: their lengths came down with them
  if (counted_kf) std::memcpy(counted_kf, down.host<int32_t>(d_ck), 4 * (size_t)h.n_counted);
  if (counted_w) std::memcpy(counted_w, down.host<int32_t>(d_cw), 4 * (size_t)h.n_counted);
  if (ordered_kf) std::memcpy(ordered_kf, down.host<int32_t>(d_ok), 4 * (size_t)h.n_connected);
  if (ordered_w) std::memcpy(ordered_w, down.host<int32_t>(d_ow), 4 * (size_t)h.n_connected);
  if (out) {
    out->n_counted = h.n_counted; out->n_connected = h.n_connected; out->parent = h.parent; out->parent_set = h.parent_set;
    out->max_weight = h.max_weight; out->max_kf = h.max_kf;
  }
  return DSH_OK;
}

}  // extern "C"
