// Host side of the map point upkeep on the resident stores (include/defslam_hip.h: dsh_keyframe_process_new, dsh_point_store_upkeep):
// validation against the host mirrors of the two stores, the launches of kfinsert_kernels.hip and one download; afterwards the mirror
// of the point store follows the records the device appended.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "kfdb_store.h"
#include "kfinsert_problem.h"
#include "mpdb_store.h"

namespace {

// the keyframe store of a call against the point store: "" or what is wrong
std::string kfdb_error(const dsh_mpdb* db, const dsh_kfdb* kfdb) {
  if (!kfdb) return "kfdb is NULL";
  if (kfdb->ctx != db->ctx) return "the keyframe store belongs to another context or was detached";
  if (kfdb->count < db->K) return "the keyframe store holds fewer keyframes than the point store";
  for (int s = 0; s < db->K; s++)
    if (kfdb->kf[s].N != db->kf[s].N) return "keyframe " + std::to_string(s) + " has another N in the keyframe store than in the point store";
  if (db->K > DSH_MP_MAX_OBS) return "more than 65535 keyframes in the store";
  if (kfdb->n_octave_over > 0)
    for (int s = 0; s < kfdb->count; s++)
      if (kfdb->kf[s].octave_over) return "keyframe " + std::to_string(s) + " has an octave >= levels in the keyframe store";
  return "";
}

// the stores' arrays and the temporaries of a call that selects at most S points with at most cap_obs observations
int fill_bufs(dsh_ctx_base* c, KiBufs& b, dsh_mpdb* db, const dsh_kfdb* kfdb, int32_t S, long long cap_obs) {
  std::memset(&b, 0, sizeof(b));
  b.P = db->P; b.S = S;
  b.xyz = db->d_xyz; b.bad = db->d_bad; b.ref_kf = db->d_ref_kf; b.nodes = db->d_nodes; b.nobs = db->d_nobs; b.table = db->d_table;
  b.desc = db->d_desc; b.normal = db->d_nrm; b.max_distance = db->d_maxd;
  b.slots = kfdb->d_slots; b.rows = kfdb->d_rows; b.oct = kfdb->d_oct; b.levels = kfdb->d_levels; b.sf = kfdb->d_sf;
  const size_t s = (size_t)S, m = (size_t)cap_obs;
  // a large point has more than MPU_SMALL observations and takes a block for its normal and one per MPU_ROWS election rows
  const size_t cap_blocks = m / MPU_ROWS + 2 * (m / (MPU_SMALL + 1)) + 2;
  HIPCHK(c, mpdb_obs_lists(db, b.ol, s, m));
  b.ol.kf = db->d_kf;
  HIPCHK(c, dsh_scratch_array(c, &b.ol.off, s + 1));
  HIPCHK(c, dsh_scratch_array(c, &b.sel_pid, s));
  HIPCHK(c, dsh_scratch_array(c, &b.obs_slot, m));
  HIPCHK(c, dsh_scratch_array(c, &b.el_row, m));
  HIPCHK(c, dsh_scratch_array(c, &b.pts, s));
  HIPCHK(c, dsh_scratch_array(c, &b.small_list, 4 * s));
  HIPCHK(c, dsh_scratch_array(c, &b.large_pts, s));
  HIPCHK(c, dsh_scratch_array(c, &b.large_blocks, cap_blocks));
  HIPCHK(c, dsh_scratch_array(c, &b.large_key, s));
  return DSH_OK;
}

}  // namespace

extern "C" {

int dsh_keyframe_process_new(dsh_mpdb* db, const dsh_keyframe_process_input* in, uint8_t* action, int32_t* added_point,
                             dsh_keyframe_process_counts* out) {
  DSH_STORE_ENTER("dsh_keyframe_process_new");
  if (!in) return bad("in is NULL");
  if (!out) return bad("out is NULL");
  if (in->slot < 0 || in->slot >= db->K) return bad("slot outside the store");
  DSH_CHECK(kfdb_error(db, in->kfdb));
  const LmKf nk = db->kf[in->slot];
  const long long cap_obs = (long long)db->obs.size() + nk.N;
  if (cap_obs > INT32_MAX || db->R + nk.N > INT32_MAX) return bad("store full");
  if (!db->unindexed.empty()) return mpdb_unindexed_error(db, who__);
  DSH_STORE_GATE();
  std::memset(out, 0, sizeof(*out));   // a refused call leaves the caller's counts as they were
  out->first_record = db->R;

  // room for a record per entry: how many points the keyframe adds is known on the device only
  const size_t N = (size_t)nk.N;
  HIPCHK(c, mpdb_reserve_log(db, db->R + nk.N));
  DownBlock down;
  const size_t d_hdr = down.take(sizeof(KiHdr)), d_added = down.take(4 * N), d_action = down.take_exact(N);
  down.copy_to(d_action, action, N);   // the kernel writes the actions whether the caller wants them or not
  if (const int rc = down.alloc(c)) return rc;
  KiBufs b;
  if (const int rc = fill_bufs(c, b, db, in->kfdb, nk.N, cap_obs)) return rc;
  b.what = DSH_MP_DESCRIPTOR | DSH_MP_NORMAL_DEPTH;
  b.slot = in->slot; b.N = nk.N; b.tab_off = nk.tab_off;
  HIPCHK(c, dsh_scratch_array(c, &b.first_i, (size_t)db->P));
  HIPCHK(c, dsh_scratch_array(c, &b.observes, (size_t)db->P));
  b.hdr = b.out_hdr = down.dev<KiHdr>(d_hdr);
  b.out_added = down.dev<int32_t>(d_added);
  b.out_action = down.dev<uint8_t>(d_action);
  HIPCHK(c, ki_process_new_launch(b, c->stream));
  if (const int rc = down.receive(c)) return rc;

  // the host mirror follows: the records the device appended, as dsh_point_store_add_observations_indexed leaves them
  const KiHdr& h = *down.host<KiHdr>(d_hdr);
  const int32_t* added = down.host<int32_t>(d_added);
  for (int j = 0; j < h.n_appended; j++) db->obs[mpdb_obs_key(added[j], in->slot)] = db->R + j;
  db->R += h.n_appended;
  out->n_empty = h.n_empty; out->n_bad = h.n_bad; out->n_added = h.n_appended; out->n_recent = h.n_recent;
  out->n_no_good_desc = h.n_no_good_desc; out->n_no_ref = h.n_no_ref;
  if (added_point && h.n_appended > 0) std::memcpy(added_point, added, 4 * (size_t)h.n_appended);   // its length came down with it
  return DSH_OK;
}

int dsh_point_store_upkeep(dsh_mpdb* db, const dsh_point_upkeep_input* in, int32_t* status, dsh_point_upkeep_counts* out) {
  DSH_STORE_ENTER("dsh_point_store_upkeep");
  if (!in) return bad("in is NULL");
  if (!out) return bad("out is NULL");
  if (in->what < 1 || in->what > (DSH_MP_DESCRIPTOR | DSH_MP_NORMAL_DEPTH))
    return bad("what is not a non-empty mask of DSH_MP_DESCRIPTOR, DSH_MP_NORMAL_DEPTH");
  if (in->select != DSH_UPKEEP_IDS && in->select != DSH_UPKEEP_EMBEDDED) return bad("select is neither DSH_UPKEEP_IDS nor DSH_UPKEEP_EMBEDDED");
  const bool embedded = in->select == DSH_UPKEEP_EMBEDDED;
  if (!embedded) {
    DSH_CHECK(mpdb_ids_error(in->n, in->ids, db->P, "point id"));
  }
  DSH_CHECK(kfdb_error(db, in->kfdb));
  if (db->obs.size() > (size_t)INT32_MAX) return bad("store full");
  if (!db->unindexed.empty()) return mpdb_unindexed_error(db, who__);
  DSH_STORE_GATE();
  std::memset(out, 0, sizeof(*out));   // a refused call leaves the caller's counts as they were
  const int32_t S = embedded ? db->P : in->n;
  if (S == 0) return DSH_OK;

  UpBlock up;
  const size_t o_ids = up.take_exact(embedded ? 0 : 4 * (size_t)S);
  up.copy_of(o_ids, embedded ? nullptr : in->ids, 4 * (size_t)S);
  DownBlock down;
  const size_t d_hdr = down.take(sizeof(KiHdr)), d_status = down.take_exact(embedded ? 0 : 4 * (size_t)S);
  down.copy_to(d_status, embedded ? nullptr : status, 4 * (size_t)S);   // the kernel writes the status whether the caller wants it or not
  if (const int rc = up.copy(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  KiBufs b;
  if (const int rc = fill_bufs(c, b, db, in->kfdb, S, (long long)db->obs.size())) return rc;
  b.what = in->what;
  b.n_ids = embedded ? 0 : S;
  b.ids = up.dev<const int32_t>(o_ids);
  b.hdr = b.out_hdr = down.dev<KiHdr>(d_hdr);
  b.out_status = embedded ? nullptr : down.dev<int32_t>(d_status);
  HIPCHK(c, ki_upkeep_launch(b, embedded ? 1 : 0, c->stream));
  if (const int rc = down.receive(c)) return rc;

  const KiHdr& h = *down.host<KiHdr>(d_hdr);
  out->n_selected = h.n_sel - h.n_skipped_bad; out->n_no_obs = h.n_no_obs; out->n_no_good_desc = h.n_no_good_desc; out->n_no_ref = h.n_no_ref;
  out->n_bad = h.n_skipped_bad;
  return DSH_OK;
}

}  // extern "C"
