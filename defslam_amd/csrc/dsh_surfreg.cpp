// Host side of the surface registration of a keyframe on the resident stores (include/defslam_hip.h: dsh_keyframe_snapshot_positions,
// dsh_keyframe_get_snapshot, dsh_keyframe_register_clouds, dsh_keyframe_register, dsh_keyframe_set_pose, dsh_keyframe_get_centre):
// validation against the host mirrors of dsh_mpdb and dsh_kfdb, the launches of surfreg_kernels.hip and, between the selection and the
// finish, the stages of dsh_register.cpp on the clouds where the selection left them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "dsh_register.h"
#include "kfdb_store.h"
#include "mpdb_store.h"
#include "surfreg_problem.h"

namespace {

SrKeyframe keyframe_slice(const dsh_mpdb* db, int32_t slot) {
  SrKeyframe k;
  k.N = db->kf[slot].N; k.tab_off = db->kf[slot].tab_off;
  k.table = db->d_table; k.snap_point = db->d_snap_point; k.snap_xyz = db->d_snap_xyz;
  return k;
}

// The keyframe store of a call that writes or reads the camera centre of keyframe `slot`: "" or what is wrong.  The handle is looked up
// among the stores attached to the context before anything of it is read, so a store of another context, a detached one and a pointer
// that is no store at all are refused without being dereferenced, wherever this check stands among the others.
std::string centre_error(const dsh_ctx_base* c, const dsh_kfdb* kfdb, int32_t slot) {
  if (std::find(c->stores.begin(), c->stores.end(), static_cast<const dsh_store*>(kfdb)) == c->stores.end())
    return "the keyframe store belongs to another context or was detached";
  if (slot < 0 || slot >= kfdb->count) return "slot outside the keyframe store";
  return "";
}

// a pose whose centre goes into the keyframe store: dsh_kfdb_add refuses a centre that is not finite, and so does every later writer
bool pose_finite(const float* T) {
  for (int i = 0; i < 16; i++)
    if (!std::isfinite(T[i])) return false;
  return true;
}

// what is wrong with the input of a registration, "" if nothing; with_stream: u and nu are read
std::string input_error(const dsh_mpdb* db, const dsh_keyframe_register_input* in, const dsh_keyframe_register_result* out, bool with_stream) {
  if (!in) return "in is NULL";
  if (!out) return "out is NULL";
  if (in->slot < 0 || in->slot >= db->K) return "slot outside the store";
  const int32_t N = db->kf[in->slot].N;
  if (in->N != N) return "N (" + std::to_string(in->N) + ") is not the N of keyframe " + std::to_string(in->slot) + " in the store (" + std::to_string(N) + ")";
  if (N > SR_MAX_KEYPOINTS) return "the keyframe has more than 8192 key points";
  // a NULL surface_pts names the keyframe's resident surface points (dsh_keyframe_surface_init); without them it is the refusal it was
  if (!in->Twc || (N > 0 && !in->surface_pts && !db->surf[in->slot].has_surface)) return "Twc or surface_pts is NULL";
  if (!pose_finite(in->Twc)) return "Twc is not finite";
  if (with_stream && (in->nu < 0 || (in->nu > 0 && !in->u))) return "nu < 0, or u is NULL";
  if (in->kfdb) {
    const std::string ke = centre_error(db->ctx, in->kfdb, in->slot);
    if (!ke.empty()) return ke;
    if (in->kfdb->kf[in->slot].N != N) return "N is not the N of keyframe " + std::to_string(in->slot) + " in the keyframe store";
  }
  return "";
}

// The selection: surface points (unless the keyframe's resident ones are read) and Twc go up, the launch leaves the clouds in scratch
// (or, when `clouds` asks for them, in the block down) and the counts and pair_idx come down; synchronised on return.  pairs receives
// pair_idx; *surface_dev: the surface points on the device, uploaded or resident.
// LIFETIME: d and *surface_dev point into slices of the context's scratch that outlive the UpBlock / DownBlock objects of this function.
// The scratch only grows within a call and is reset by dsh_enter alone, which an entry point calls once, at its start; the stages of
// dsh_register.h take further slices and never enter.  So the pointers hold until the caller returns, and no longer: nothing that calls
// dsh_enter may come between this function and their last use (finish, below).
int select_clouds(dsh_mpdb* db, const dsh_keyframe_register_input* in, bool clouds, dsh::Clouds& d, SrCounts& counts, std::vector<int32_t>& pairs,
                  float* cloud_surface, float* cloud_map, const float** surface_dev) {
  dsh_ctx_base* c = db->ctx;
  const size_t N = (size_t)in->N;
  UpBlock up;
  const bool resident = !in->surface_pts && db->surf[in->slot].has_surface;
  const size_t o_T = up.copy_of(in->Twc, 64), o_surf = up.take_exact(resident ? 0 : 12 * N);
  up.copy_of(o_surf, resident ? nullptr : in->surface_pts, 12 * N);
  DownBlock down;
  const size_t d_cnt = down.take(sizeof(SrCounts)), d_idx = down.take(4 * N), d_a = down.take(clouds ? 12 * N : 0), d_b = down.take_exact(clouds ? 12 * N : 0);
  if (const int rc = up.copy(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  SrSelect k;
  k.kf = keyframe_slice(db, in->slot);
  k.P = db->P;
  k.surface = resident ? db->d_surf_pts + 3 * (size_t)k.kf.tab_off : up.dev<const float>(o_surf);
  k.Twc = up.dev<const float>(o_T);
  k.pair_idx = down.dev<int32_t>(d_idx);
  k.counts = down.dev<SrCounts>(d_cnt);
  if (clouds) {
    k.cloud_surface = down.dev<float>(d_a);
    k.cloud_map = down.dev<float>(d_b);
  } else {
    HIPCHK(c, dsh_scratch_array(c, &k.cloud_surface, 3 * N));
    HIPCHK(c, dsh_scratch_array(c, &k.cloud_map, 3 * N));
  }
  HIPCHK(c, dsh_scratch_array(c, &k.entry_of, (size_t)db->P));
  HIPCHK(c, sr_select_launch(mpdb_state(db), k, c->stream));
  if (const int rc = down.fetch(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  counts = *down.host<SrCounts>(d_cnt);
  const size_t n = (size_t)counts.n_pairs;
  pairs.assign(down.host<int32_t>(d_idx), down.host<int32_t>(d_idx) + n);
  // the clouds: their length came down with them
  if (cloud_surface && n > 0) std::memcpy(cloud_surface, down.host<float>(d_a), 12 * n);
  if (cloud_map && n > 0) std::memcpy(cloud_map, down.host<float>(d_b), 12 * n);
  d = {k.cloud_surface, k.cloud_map};
  if (surface_dev) *surface_dev = k.surface;
  return DSH_OK;
}

void put_counts(dsh_keyframe_register_result* out, const SrCounts& s) {
  out->n_pairs = s.n_pairs; out->n_empty = s.n_empty; out->n_bad = s.n_bad; out->n_no_facet = s.n_no_facet; out->n_no_snapshot = s.n_no_snapshot;
}

// the finishing launch: surface_scaled (N > 0) and the centre come down; kfdb: the store whose centre is written, or null; db: the point
// store when keyframe `slot` of it is the one being registered (its resident Surface, where it has one, is scaled too), or null
int finish(dsh_ctx_base* c, int32_t N, const float* surface_dev, double s22, const float* Tcw, dsh_kfdb* kfdb, int32_t slot, float* surface_scaled, float* Ow,
           dsh_mpdb* db) {
  DownBlock down;
  const size_t d_Ow = down.take(12), d_s = down.take_exact(12 * (size_t)N);
  down.copy_to(d_Ow, Ow, 12);   // the kernel writes both whether the caller wants them or not
  down.copy_to(d_s, surface_scaled, 12 * (size_t)N);
  if (const int rc = down.alloc(c)) return rc;
  SrFinish k;
  k.N = N;
  k.surface = surface_dev;
  k.s22 = s22;
  std::memcpy(k.Tcw, Tcw, 64);   // a kernel argument
  k.kf_slot = kfdb ? kfdb->d_slots + slot : nullptr;
  k.surface_scaled = down.dev<float>(d_s);
  k.Ow = down.dev<float>(d_Ow);
  k.resident_pts = nullptr; k.resident_depth = nullptr; k.n_depth = 0;
  if (db && db->surf[slot].has_surface) {   // Surface::applyScale of the copy the store holds (Surface.cc:107-121)
    const dsh_mpdb::SurfKf& sk = db->surf[slot];
    k.resident_pts = db->d_surf_pts + 3 * (size_t)db->kf[slot].tab_off;
    if (sk.has_depth) {
      k.resident_depth = db->d_surf_depth + (size_t)dsh_mpdb::SURF_MAX_CTRL * slot;
      k.n_depth = sk.grid.nptsu * sk.grid.nptsv;
    }
  }
  HIPCHK(c, sr_finish_launch(k, c->stream));
  return down.receive(c);
}

}  // namespace

extern "C" {

int dsh_keyframe_snapshot_positions(dsh_mpdb* db, int32_t slot, int32_t* n_taken) {
  DSH_STORE_ENTER("dsh_keyframe_snapshot_positions");
  if (slot < 0 || slot >= db->K) return bad("slot outside the store");
  if (db->snapped[slot]) return refuse(DSH_ERR_STATE, "the snapshot of keyframe " + std::to_string(slot) + " has been taken already");
  DSH_STORE_GATE();
  DownBlock down;
  const size_t d_n = down.take_exact(4);
  down.copy_to(d_n, n_taken, 4);   // the kernel counts whether the caller wants the count or not
  if (const int rc = down.alloc(c)) return rc;
  HIPCHK(c, sr_snapshot_launch(mpdb_state(db), keyframe_slice(db, slot), down.dev<int32_t>(d_n), c->stream));
  if (const int rc = down.receive(c)) return rc;
  db->snapped[slot] = 1;
  return DSH_OK;
}

int dsh_keyframe_get_snapshot(dsh_mpdb* db, int32_t slot, int32_t capacity, int32_t* point, float* xyz) {
  DSH_STORE_ENTER("dsh_keyframe_get_snapshot");
  if (slot < 0 || slot >= db->K) return bad("slot outside the store");
  const LmKf k = db->kf[slot];
  if (capacity < k.N) return bad("capacity is smaller than the keyframe's N");
  if (k.N > 0 && (!point || !xyz)) return bad("point or xyz is NULL");
  DSH_STORE_GATE();
  if (k.N == 0) return DSH_OK;
  HIPCHK(c, hipMemcpyAsync(point, db->d_snap_point + k.tab_off, 4 * (size_t)k.N, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(xyz, db->d_snap_xyz + 3 * (size_t)k.tab_off, 12 * (size_t)k.N, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // an entry without a snapshot holds whatever the allocation held: zeros for the caller
  for (int i = 0; i < k.N; i++)
    if (point[i] < 0) xyz[3 * (size_t)i] = xyz[3 * (size_t)i + 1] = xyz[3 * (size_t)i + 2] = 0.f;
  return DSH_OK;
}

int dsh_keyframe_register_clouds(dsh_mpdb* db, const dsh_keyframe_register_input* in, int32_t* pair_idx, float* cloud_surface, float* cloud_map,
                                 dsh_keyframe_register_result* out) {
  DSH_STORE_ENTER("dsh_keyframe_register_clouds");
  DSH_CHECK(input_error(db, in, out, false));
  DSH_STORE_GATE();
  dsh::Clouds d;
  SrCounts counts;
  std::vector<int32_t> pairs;
  if (const int rc = select_clouds(db, in, cloud_surface || cloud_map, d, counts, pairs, cloud_surface, cloud_map, nullptr)) return rc;
  std::memset(out, 0, sizeof(*out));
  put_counts(out, counts);
  if (pair_idx && !pairs.empty()) std::memcpy(pair_idx, pairs.data(), 4 * pairs.size());
  return DSH_OK;
}

int dsh_keyframe_register(dsh_mpdb* db, const dsh_keyframe_register_input* in, int32_t* pair_idx, float* surface_scaled, dsh_keyframe_register_result* out) {
  DSH_STORE_ENTER("dsh_keyframe_register");
  DSH_CHECK(input_error(db, in, out, true));
  DSH_STORE_GATE();
  dsh::Clouds d;
  SrCounts counts;
  std::vector<int32_t> pairs;
  const float* surface_dev = nullptr;
  if (const int rc = select_clouds(db, in, false, d, counts, pairs, nullptr, nullptr, &surface_dev)) return rc;
  dsh_keyframe_register_result r;
  std::memset(&r, 0, sizeof(r));
  put_counts(&r, counts);
  const int n = counts.n_pairs;
  if (n > dsh::kMaxPairs) {
    *out = r;
    return bad(std::to_string(n) + " pairs: more than the 8000 of dsh_surface_register");
  }
  if (n >= 15) {   // SurfaceRegistration.cc:106-107
    // the reference's draws, walked on the host as scaleMinMedian's first stage does: too few is a refusal before anything runs
    if (dsh::smm_walk_candidates(n, in->u, in->nu, nullptr, nullptr, &r.consumed) < 0) {
      r.consumed = 0;
      r.stream_status = 1;
      *out = r;
      return bad("the uniform stream is shorter than the draws the reference makes for " + std::to_string(n) + " pairs");
    }
    // from here on as dsh_surface_register, on the clouds the selection left on the device
    float scale = 0.f;
    int32_t status = 0;
    if (const int rc = dsh::scale_min_median_dev(c, n, nullptr, nullptr, in->u, in->nu, &scale, nullptr, &status, d)) return rc;
    r.sim3[0] = r.sim3[1] = r.sim3[2] = 0.0; r.sim3[3] = 1.0;
    r.sim3[4] = r.sim3[5] = r.sim3[6] = 0.0; r.sim3[7] = (double)scale;
    int32_t acceptable = 0;
    double hi[6];
    if (const int rc = dsh::optimize_horn_dev(c, n, d, nullptr, nullptr, r.sim3, in->chi_limit * in->chi_limit, 0.01, &acceptable, hi)) return rc;
    r.info[0] = scale;
    for (int i = 0; i < 6; i++) r.info[1 + i] = hi[i];
    r.info[7] = acceptable;
    if (acceptable || !in->check_chi) {
      dsh::compose(r.sim3, in->Twc, &r.s22, r.Tcw_new);
      if (!pose_finite(r.Tcw_new) || !std::isfinite(r.s22)) {   // a degenerate alignment (scale 0): the reference would SetPose it; the stores keep finite centres
        *out = r;
        return refuse(DSH_ERR_STATE, "the registration composed a pose that is not finite; nothing was written");
      }
      // Surface::applyScale of the surface points, KeyFrame::SetPose's centre into the keyframe store
      if (const int rc = finish(c, in->N, surface_dev, r.s22, r.Tcw_new, in->kfdb, in->slot, surface_scaled, r.Ow_new, db)) return rc;
      r.registered = 1;
    }
  }
  *out = r;
  if (pair_idx && !pairs.empty()) std::memcpy(pair_idx, pairs.data(), 4 * pairs.size());
  return DSH_OK;
}

int dsh_keyframe_set_pose(dsh_mpdb* db, const dsh_keyframe_pose_input* in, float* Ow) {
  DSH_STORE_ENTER("dsh_keyframe_set_pose");
  if (!in) return bad("in is NULL");
  if (!in->kfdb) return bad("kfdb is NULL");
  if (!in->Tcw) return bad("Tcw is NULL");
  if (!pose_finite(in->Tcw)) return bad("Tcw is not finite");
  DSH_CHECK(centre_error(c, in->kfdb, in->slot));
  DSH_STORE_GATE();
  return finish(c, 0, nullptr, 1.0, in->Tcw, in->kfdb, in->slot, nullptr, Ow, nullptr);
}

int dsh_keyframe_get_centre(dsh_mpdb* db, const dsh_keyframe_pose_input* in, float* Ow) {
  DSH_STORE_ENTER("dsh_keyframe_get_centre");
  if (!in) return bad("in is NULL");
  if (!in->kfdb) return bad("kfdb is NULL");
  if (!Ow) return bad("Ow is NULL");
  DSH_CHECK(centre_error(c, in->kfdb, in->slot));
  DSH_STORE_GATE();
  HIPCHK(c, hipMemcpyAsync(Ow, in->kfdb->d_slots[in->slot].Ow, 12, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return DSH_OK;
}

}  // extern "C"
