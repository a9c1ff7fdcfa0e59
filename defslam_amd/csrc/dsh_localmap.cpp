// Host side of the map point store and the local map (include/defslam_hip.h: dsh_mpdb_*, dsh_local_map_*): the store's arrays in HBM and
// the host mirror that validates (mpdb_store.h), and per call one upload, the launches of localmap_kernels.hip (and, for the search, of
// track_kernels.hip) and one download.  The entries here also keep the per-point tracking state of dsh_trackstate_* current
// (trackclose_kernels.hip): new points start at mnVisible = mnFound = 1, observations count into nObs, the update keeps the previous
// local point list, the search adds SearchLocalPoints' IncreaseVisible.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "localmap_problem.h"
#include "mpdb_store.h"
#include "track_problem.h"

namespace {

// one int32 of the store, written in stream order
int put_i32(dsh_ctx_base* c, int32_t* dst, int32_t v) {
  HIPCHK(c, hipMemcpyAsync(dst, &v, 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return DSH_OK;
}

// MapPoint::AddObservation for n pairs, with the key point index of each (indexed) or without one
int add_observations(dsh_mpdb* db, const char* who, int n, const int32_t* point_ids, const int32_t* keyframe_slots, const int32_t* idx, bool indexed) {
  DSH_STORE_ENTER(who);
  if (n < 0) return bad("n < 0");
  if (n > 0 && (!point_ids || !keyframe_slots)) return bad("point_ids or keyframe_slots is NULL");
  if (n > 0 && indexed && !idx) return bad("idx is NULL");
  std::unordered_set<uint64_t> batch;
  for (int i = 0; i < n; i++) {
    const int32_t p = point_ids[i], s = keyframe_slots[i];
    const std::string at = "pair " + std::to_string(i) + ": ", pe = mpdb_pair_error(db, p, s);
    if (!pe.empty()) return bad(at + pe);
    if (indexed && (idx[i] < 0 || idx[i] >= db->kf[s].N)) return bad(at + "index outside the keyframe's key points");
    if (db->obs.count(mpdb_obs_key(p, s))) return bad(at + "the point already observes this keyframe");
    if (!batch.insert(mpdb_obs_key(p, s)).second) return bad(at + "repeated in the batch");
  }
  DSH_STORE_GATE();
  if (n == 0) return DSH_OK;
  HIPCHK(c, mpdb_reserve_log(db, db->R + n));
  UpBlock up;   // staged here, copied to the end of the log and of the indices beside it
  const size_t o_rec = up.take(8 * (size_t)n), o_idx = up.copy_of(indexed ? idx : nullptr, 4 * (size_t)n);
  if (const int rc = up.stage(c)) return rc;
  int2* h = up.host<int2>(o_rec);   // the records are interleaved from the two arrays
  for (int i = 0; i < n; i++) h[i] = make_int2(point_ids[i], keyframe_slots[i]);
  HIPCHK(c, hipMemcpyAsync(db->d_log + db->R, h, 8 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  if (indexed) {
    HIPCHK(c, hipMemcpyAsync(db->d_log_idx + db->R, up.host<int32_t>(o_idx), 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  } else {
    HIPCHK(c, hipMemsetAsync(db->d_log_idx + db->R, 0xff, 4 * (size_t)n, c->stream));   // -1: no index
  }
  HIPCHK(c, tc_add_by_index_launch(db->d_nobs, reinterpret_cast<const int32_t*>(db->d_log + db->R), 2, 1, n, c->stream));   // nObs++ (MapPoint.cc:116-119)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < n; i++) {
    const uint64_t k = mpdb_obs_key(point_ids[i], keyframe_slots[i]);
    db->obs[k] = db->R + i;
    if (!indexed) db->unindexed.insert(k);
  }
  db->R += n;
  return DSH_OK;
}

}  // namespace

extern "C" {

int dsh_mpdb_create(const dsh_mpdb_desc* desc, dsh_mpdb** out) {
  if (!desc) return DSH_ERR_ARG;
  dsh_ctx_base* c = dsh_base(desc->ctx);
  if (!c) return DSH_ERR_ARG;
  if (!out) return dsh_fail(c, DSH_ERR_ARG, "dsh_mpdb_create: out is NULL");
  *out = nullptr;
  if (desc->point_capacity <= 0 || desc->keyframe_capacity <= 0 || desc->observation_capacity <= 0 || desc->observation_capacity > (1ll << 40))
    return dsh_fail(c, DSH_ERR_ARG, "dsh_mpdb_create: capacities must be positive");
  dsh_mpdb* db = new dsh_mpdb();
  if (!c->host_only) {
    // a host-only context gets a store without arrays: its entry points check arguments and refuse (dsh_enter)
    if (const int rc = dsh_enter(c, "dsh_mpdb_create")) { delete db; return rc; }
    db->Tcap = (long long)desc->keyframe_capacity * 1024;
    db->Rcap = desc->observation_capacity;
    if (mpdb_reserve_points(db, desc->point_capacity) != hipSuccess || mpdb_reserve_keyframes(db, desc->keyframe_capacity) != hipSuccess ||
        mpdb_reserve_log(db, db->Rcap) != hipSuccess || mpdb_reserve_table(db, db->Tcap) != hipSuccess || hipMalloc((void**)&db->d_hdr, sizeof(LmHdr)) != hipSuccess ||
        hipMemset(db->d_hdr, 0, sizeof(LmHdr)) != hipSuccess) {
      db->free_all();
      delete db;
      return dsh_fail(c, DSH_ERR_HIP, "dsh_mpdb_create: out of device memory");
    }
  }
  dsh_attach_store(c, db);
  *out = db;
  return DSH_OK;
}

int dsh_mpdb_destroy(dsh_mpdb* db) {
  if (!db) return DSH_ERR_ARG;
  if (db->d_hdr) dsh_store_unregister(db);
  else if (db->ctx) db->ctx->stores.erase(std::remove(db->ctx->stores.begin(), db->ctx->stores.end(), (dsh_store*)db), db->ctx->stores.end());
  db->free_all();
  delete db;
  return DSH_OK;
}

int dsh_mpdb_clear(dsh_mpdb* db) {
  DSH_STORE_ENTER("dsh_mpdb_clear");
  if (db->d_hdr) {
    if (hipSetDevice(c->device) != hipSuccess) return refuse(DSH_ERR_HIP, "hipSetDevice failed");
    HIPCHK(c, hipMemsetAsync(db->d_hdr, 0, sizeof(LmHdr), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  db->P = db->K = 0;
  db->R = db->T = 0;
  db->n_local_points = db->n_ref_points = db->P_cnt = 0;
  db->top_node.clear();
  db->max_node = -1;
  db->max_node_stale = false;
  db->top_on_device = false;
  db->last_N = db->cand_N = -1;
  db->last_kept = 0;
  db->last_max_octave = -1;
  db->obs.clear();
  db->unindexed.clear();
  db->kf.clear();
  db->snapped.clear();
  db->surf.clear();
  db->first_conn.clear();
  return DSH_OK;
}

int32_t dsh_mpdb_point_count(const dsh_mpdb* db) { return db ? db->P : -1; }
int32_t dsh_mpdb_keyframe_count(const dsh_mpdb* db) { return db ? db->K : -1; }

int dsh_mpdb_add_points(dsh_mpdb* db, int n, const float* xyz, const float* normal, const float* max_distance, const uint8_t* desc,
                        const uint8_t* bad_flags, int32_t* first_id) {
  DSH_STORE_ENTER("dsh_mpdb_add_points");
  if (n < 0) return bad("n < 0");
  if (n > 0 && (!xyz || !normal || !max_distance || !desc)) return bad("a point array is NULL");
  if ((long long)db->P + n > INT32_MAX) return bad("store full");
  DSH_STORE_GATE();
  if (first_id) *first_id = db->P;
  if (n == 0) return DSH_OK;
  HIPCHK(c, mpdb_reserve_points(db, (long long)db->P + n));
  std::vector<int32_t> b32(n, 0);
  if (bad_flags)
    for (int i = 0; i < n; i++) b32[i] = bad_flags[i] ? 1 : 0;
  hipStream_t st = c->stream;
  const size_t P = (size_t)db->P;
  HIPCHK(c, hipMemcpyAsync(db->d_xyz + 3 * P, xyz, 12 * (size_t)n, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(db->d_nrm + 3 * P, normal, 12 * (size_t)n, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(db->d_maxd + P, max_distance, 4 * (size_t)n, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(db->d_desc + 2 * P, desc, 32 * (size_t)n, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(db->d_bad + P, b32.data(), 4 * (size_t)n, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(db->d_ref_kf + P, 0xff, 4 * (size_t)n, st));   // no reference keyframe yet (dsh_point_store_set_reference_keyframes)
  HIPCHK(c, tc_init_points_launch(mpdb_state(db), db->P, n, st));   // mnVisible = mnFound = 1, nObs = 0, no facet
  HIPCHK(c, hipStreamSynchronize(st));
  db->P += n;
  db->top_node.resize((size_t)db->P, -1);
  return DSH_OK;
}

int dsh_mpdb_update_points(dsh_mpdb* db, int n, const int32_t* ids, int32_t what, const float* xyz, const float* normal,
                           const float* max_distance, const uint8_t* desc) {
  DSH_STORE_ENTER("dsh_mpdb_update_points");
  if (what < 1 || what > (DSH_MPDB_POSITION | DSH_MPDB_NORMAL_DEPTH | DSH_MPDB_DESCRIPTOR))
    return bad("what is not a non-empty mask of DSH_MPDB_POSITION, DSH_MPDB_NORMAL_DEPTH, DSH_MPDB_DESCRIPTOR");
  DSH_CHECK(mpdb_ids_error(n, ids, db->P, "point id"));
  const bool wp = (what & DSH_MPDB_POSITION) != 0, wn = (what & DSH_MPDB_NORMAL_DEPTH) != 0, wd = (what & DSH_MPDB_DESCRIPTOR) != 0;
  if (n > 0 && ((wp && !xyz) || (wn && (!normal || !max_distance)) || (wd && !desc))) return bad("an array that `what` selects is NULL");
  DSH_STORE_GATE();
  if (n == 0) return DSH_OK;
  UpBlock up;   // an array that `what` does not select is not read: an empty slice
  const size_t m = (size_t)n, o_ids = up.copy_of(ids, 4 * m), o_xyz = up.copy_of(wp ? xyz : nullptr, 12 * m), o_nrm = up.copy_of(wn ? normal : nullptr, 12 * m),
               o_maxd = up.copy_of(wn ? max_distance : nullptr, 4 * m), o_desc = up.copy_of(wd ? desc : nullptr, 32 * m);
  if (const int rc = up.copy(c)) return rc;
  hipStream_t st = c->stream;
  LmWriteBufs w;
  w.ids = up.dev<const int32_t>(o_ids);
  w.src_xyz = up.dev<const float>(o_xyz);
  w.src_normal = up.dev<const float>(o_nrm);
  w.src_max_distance = up.dev<const float>(o_maxd);
  w.src_desc = up.dev<const uint4>(o_desc);
  w.xyz = db->d_xyz; w.normal = db->d_nrm; w.max_distance = db->d_maxd; w.desc = db->d_desc;
  HIPCHK(c, lm_write_points_launch(w, n, what, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return DSH_OK;
}

int dsh_mpdb_set_points_bad(dsh_mpdb* db, int n, const int32_t* ids, const uint8_t* bad_flags) {
  DSH_STORE_ENTER("dsh_mpdb_set_points_bad");
  DSH_CHECK(mpdb_ids_error(n, ids, db->P, "point id"));
  DSH_STORE_GATE();
  if (n == 0) return DSH_OK;
  UpBlock up;
  const size_t m = (size_t)n, o_ids = up.copy_of(ids, 4 * m), o_val = up.take(4 * m);
  if (const int rc = up.stage(c)) return rc;
  int32_t* v = up.host<int32_t>(o_val);   // the flags widen to int32, and a null array means all
  for (int i = 0; i < n; i++) v[i] = !bad_flags || bad_flags[i] ? 1 : 0;
  if (const int rc = up.send(c)) return rc;
  hipStream_t st = c->stream;
  HIPCHK(c, lm_scatter_i32_launch(db->d_bad, up.dev<const int32_t>(o_ids), up.dev<const int32_t>(o_val), 0, n, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return DSH_OK;
}

int dsh_mpdb_add_observations(dsh_mpdb* db, int n, const int32_t* point_ids, const int32_t* keyframe_slots) {
  return add_observations(db, "dsh_mpdb_add_observations", n, point_ids, keyframe_slots, nullptr, false);
}

int dsh_point_store_add_observations_indexed(dsh_mpdb* db, int n, const int32_t* point_ids, const int32_t* keyframe_slots, const int32_t* idx) {
  return add_observations(db, "dsh_point_store_add_observations_indexed", n, point_ids, keyframe_slots, idx, true);
}

int dsh_mpdb_erase_observations(dsh_mpdb* db, int n, const int32_t* point_ids, const int32_t* keyframe_slots) {
  DSH_STORE_ENTER("dsh_mpdb_erase_observations");
  if (n < 0) return bad("n < 0");
  if (n > 0 && (!point_ids || !keyframe_slots)) return bad("point_ids or keyframe_slots is NULL");
  for (int i = 0; i < n; i++) {
    const std::string pe = mpdb_pair_error(db, point_ids[i], keyframe_slots[i]);
    if (!pe.empty()) return bad("pair " + std::to_string(i) + ": " + pe);
  }
  DSH_STORE_GATE();
  // the records to blank: 2 * record is the point field of the log seen as int32 pairs
  std::vector<int32_t> idx;
  std::vector<uint64_t> keys;
  for (int i = 0; i < n; i++) {
    const uint64_t k = mpdb_obs_key(point_ids[i], keyframe_slots[i]);
    const auto it = db->obs.find(k);
    if (it == db->obs.end() || std::find(keys.begin(), keys.end(), k) != keys.end()) continue;
    if (it->second > (INT32_MAX >> 1)) return bad("log too long to erase from");
    idx.push_back((int32_t)(2 * it->second));
    keys.push_back(k);
  }
  if (idx.empty()) return DSH_OK;
  UpBlock up;
  const size_t o_idx = up.take_exact(4 * idx.size());
  up.copy_of(o_idx, idx.data(), up.size);
  if (const int rc = up.copy(c)) return rc;
  const int32_t* didx = up.dev<const int32_t>(o_idx);
  // nObs-- of every pair that was found (MapPoint.cc:114-133), read from the records before they are blanked
  HIPCHK(c, tc_add_by_record_launch(db->d_nobs, reinterpret_cast<const int32_t*>(db->d_log), didx, -1, (int)idx.size(), c->stream));
  HIPCHK(c, lm_scatter_i32_launch(reinterpret_cast<int32_t*>(db->d_log), didx, nullptr, -1, (int)idx.size(), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (const uint64_t k : keys) {
    db->obs.erase(k);
    db->unindexed.erase(k);
  }
  return DSH_OK;
}

int dsh_mpdb_add_keyframe(dsh_mpdb* db, int32_t N, const int32_t* points, int32_t parent, int32_t bad_flag, int32_t* slot) {
  DSH_STORE_ENTER("dsh_mpdb_add_keyframe");
  DSH_CHECK(dsh_keypoint_count_error(N));
  if (N > 0 && !points) return bad("the table is NULL");
  DSH_CHECK(mpdb_table_error(db, N, points, "table entry ", ""));
  if (parent < -1 || parent >= db->K) return bad("parent is neither -1 nor a slot of the store");
  if (db->K == INT32_MAX || db->T + N > INT32_MAX) return bad("store full");
  DSH_STORE_GATE();
  HIPCHK(c, mpdb_reserve_keyframes(db, (long long)db->K + 1));
  HIPCHK(c, mpdb_reserve_table(db, db->T + N));
  LmKf k;
  k.tab_off = (int32_t)db->T; k.N = N; k.parent = parent; k.bad = bad_flag ? 1 : 0;
  HIPCHK(c, hipMemcpyAsync(db->d_kf + db->K, &k, sizeof(k), hipMemcpyHostToDevice, c->stream));
  if (N > 0) {
    HIPCHK(c, hipMemcpyAsync(db->d_table + db->T, points, 4 * (size_t)N, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(db->d_snap_point + db->T, 0xff, 4 * (size_t)N, c->stream));   // -1: no snapshot yet (dsh_keyframe_snapshot_positions)
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  db->kf.push_back(k);
  db->snapped.push_back(0);
  db->surf.emplace_back();
  db->first_conn.push_back(1);
  if (slot) *slot = db->K;
  db->K++;
  db->T += N;
  return DSH_OK;
}

int dsh_mpdb_set_keyframe_point(dsh_mpdb* db, int32_t slot, int32_t idx, int32_t point_id) {
  DSH_STORE_ENTER("dsh_mpdb_set_keyframe_point");
  if (slot < 0 || slot >= db->K) return bad("slot outside the store");
  if (idx < 0 || idx >= db->kf[slot].N) return bad("index outside the keyframe's key points");
  if (point_id < -1 || point_id >= db->P) return bad("point_id is neither -1 nor a point of the store");
  DSH_STORE_GATE();
  return put_i32(c, db->d_table + db->kf[slot].tab_off + idx, point_id);
}

int dsh_mpdb_set_keyframe_parent(dsh_mpdb* db, int32_t slot, int32_t parent) {
  DSH_STORE_ENTER("dsh_mpdb_set_keyframe_parent");
  if (slot < 0 || slot >= db->K) return bad("slot outside the store");
  if (parent < -1 || parent >= db->K || parent == slot) return bad("parent is neither -1 nor another slot of the store");
  DSH_STORE_GATE();
  db->kf[slot].parent = parent;
  return put_i32(c, &db->d_kf[slot].parent, parent);
}

int dsh_mpdb_set_keyframe_bad(dsh_mpdb* db, int32_t slot, int32_t bad_flag) {
  DSH_STORE_ENTER("dsh_mpdb_set_keyframe_bad");
  if (slot < 0 || slot >= db->K) return bad("slot outside the store");
  DSH_STORE_GATE();
  db->kf[slot].bad = bad_flag ? 1 : 0;
  return put_i32(c, &db->d_kf[slot].bad, bad_flag ? 1 : 0);
}

int dsh_local_map_update(dsh_mpdb* db, int N, const int32_t* frame_points, uint8_t* frame_bad, int32_t kf_capacity, int32_t* local_kf,
                         int32_t* local_votes, int32_t* n_voted, int32_t* n_local_kf, int32_t* ref_kf, int32_t* n_local_points) {
  DSH_STORE_ENTER("dsh_local_map_update");
  DSH_CHECK(dsh_keypoint_count_error(N));
  if (N > 0 && !frame_points) return bad("frame_points is NULL");
  DSH_CHECK(mpdb_table_error(db, N, frame_points, "frame_points[", "]"));
  if ((local_kf || local_votes) && kf_capacity < db->K) return bad("kf_capacity is smaller than the store's keyframe count");
  DSH_STORE_GATE();

  const size_t P = (size_t)db->P, K = (size_t)db->K, nb = (P + LM_CHUNK - 1) / LM_CHUNK;
  UpBlock up;
  DownBlock down;
  const size_t o_fp = up.take_exact(4 * (size_t)N);
  up.copy_of(o_fp, frame_points, 4 * (size_t)N);
  const size_t d_hdr = down.take(sizeof(LmHdr)), d_kf = down.take(4 * K), d_votes = down.take(4 * K), d_fbad = down.take((size_t)N);
  down.copy_to(d_fbad, frame_bad, (size_t)N);   // the kernel writes the flags whether the caller wants them or not
  hipStream_t st = c->stream;
  LmBufs b;
  if (const int rc = up.copy(c)) return rc;
  HIPCHK(c, dsh_scratch_array(c, &b.votes, K));
  HIPCHK(c, dsh_scratch_array(c, &b.mark, K));
  HIPCHK(c, dsh_scratch_array(c, &b.flag, P));
  HIPCHK(c, dsh_scratch_array(c, &b.block_cnt, nb));
  if (const int rc = down.alloc(c)) return rc;
  // Tracking.cc:1475: SetReferenceMapPoints(mvpLocalMapPoints) before the list is rebuilt -- the list this call found stays, as the
  // reference list of dsh_track_close_frame, and the new one is written into the other buffer
  std::swap(db->d_local_ids, db->d_ref_ids);
  db->n_ref_points = db->n_local_points;
  db->P_cnt = db->P;
  b.P = db->P; b.K = db->K; b.N = N; b.R = db->R;
  b.bad = db->d_bad; b.log = db->d_log; b.kf = db->d_kf; b.table = db->d_table;
  b.frame_points = up.dev<const int32_t>(o_fp);
  b.cnt = db->d_cnt;
  b.local_kf = db->d_local_kf; b.local_ids = db->d_local_ids; b.hdr = db->d_hdr;
  b.out_hdr = down.dev<LmHdr>(d_hdr);
  b.out_kf = down.dev<int32_t>(d_kf);
  b.out_votes = down.dev<int32_t>(d_votes);
  b.out_frame_bad = down.dev<uint8_t>(d_fbad);
  HIPCHK(c, lm_update_launch(b, st));
  if (const int rc = down.receive(c)) return rc;

  const LmHdr h = *down.host<LmHdr>(d_hdr);
  db->n_local_points = h.n_local_points;
  // the lists: their lengths came down with them
  if (local_kf) std::memcpy(local_kf, down.host<int32_t>(d_kf), 4 * (size_t)h.n_local_kf);
  if (local_votes) std::memcpy(local_votes, down.host<int32_t>(d_votes), 4 * (size_t)h.n_voted);
  if (n_voted) *n_voted = h.n_voted;
  if (n_local_kf) *n_local_kf = h.n_local_kf;
  if (ref_kf) *ref_kf = h.ref_kf;
  if (n_local_points) *n_local_points = h.n_local_points;
  return DSH_OK;
}

int dsh_local_map_points(dsh_mpdb* db, int32_t capacity, int32_t* ids, int32_t* n) {
  DSH_STORE_ENTER("dsh_local_map_points");
  if (capacity < db->n_local_points) return bad("capacity is smaller than the number of local points");
  if (db->n_local_points > 0 && !ids) return bad("ids is NULL");
  DSH_STORE_GATE();
  if (db->n_local_points > 0) {
    HIPCHK(c, hipMemcpyAsync(ids, db->d_local_ids, 4 * (size_t)db->n_local_points, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (n) *n = db->n_local_points;
  return DSH_OK;
}

int dsh_local_map_search(dsh_mpdb* db, const dsh_track_frame* frame, float th, int32_t capacity, int32_t* local_ids, int32_t* match,
                         uint8_t* in_view, int32_t* level, float* uv, float* view_cos, int32_t* nmatches) {
  DSH_STORE_ENTER("dsh_local_map_search");
  if (!frame) return bad("frame is NULL");
  DSH_CHECK(trk_frame_error(*frame));
  if (!(th > 0.0f) || !std::isfinite(th)) return bad("th must be a positive finite number");
  const int Q = db->n_local_points;
  if (capacity < Q) return bad("capacity is smaller than the number of local points");
  if (Q > 0 && !match) return bad("match is NULL");
  if (Q > (1 << 28)) return bad("too many local points");
  DSH_STORE_GATE();
  if (nmatches) *nmatches = 0;
  if (Q == 0) {
    // no query, but the frame's own points are still seen (Tracking.cc:1408-1425)
    HIPCHK(c, tc_visible_launch(db->d_visible, db->d_cnt, db->P_cnt, nullptr, nullptr, 0, nullptr, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSH_OK;
  }

  // up: the frame and its key points; the queries are gathered from the store on the device, and their ids come down too
  const dsh_track_frame& f = *frame;
  const size_t q = (size_t)Q;
  UpBlock up;
  DownBlock down;
  TrkPlan pl;
  trk_plan_layout(pl, up, down, 1, (size_t)f.N, q, (size_t)f.grid_cols * f.grid_rows + 1);
  const size_t d_ids = down.take(4 * q);   // read by the visibility launch too, whether the caller wants the ids or not
  down.copy_to(d_ids, local_ids, 4 * q);
  down.copy_to(pl.d_match, match, 4 * q);
  down.copy_to(pl.d_level, level, 4 * q);
  down.copy_to(pl.d_uv, uv, 8 * q);
  down.copy_to(pl.d_vcos, view_cos, 4 * q);
  if (const int rc = up.stage(c)) return rc;
  TrkProb pr;
  trk_fill_prob(pr, f, DSH_TRACK_LOCAL, th, Q);
  trk_plan_pack_frame(pl, up, 0, pr, f);
  hipStream_t st = c->stream;
  TrkBufs b;
  if (const int rc = trk_plan_device(c, pl, up, down, b)) return rc;
  LmQueryBufs g;
  HIPCHK(c, dsh_scratch_array(c, &g.qpid, q));
  HIPCHK(c, dsh_scratch_array(c, &g.qxyz, 3 * q));
  HIPCHK(c, dsh_scratch_array(c, &g.qnrm, 3 * q));
  HIPCHK(c, dsh_scratch_array(c, &g.qmaxd, q));
  HIPCHK(c, dsh_scratch_array(c, &g.qmeta, q));
  HIPCHK(c, dsh_scratch_array(c, &g.qdesc, 2 * q));
  g.xyz = db->d_xyz; g.normal = db->d_nrm; g.max_distance = db->d_maxd; g.desc = db->d_desc; g.bad = db->d_bad; g.cnt = db->d_cnt;
  g.local_ids = db->d_local_ids;
  g.out_ids = down.dev<int32_t>(d_ids);
  HIPCHK(c, lm_gather_launch(g, Q, st));
  b.qpid = g.qpid; b.qxyz = g.qxyz; b.qnrm = g.qnrm; b.qmaxd = g.qmaxd; b.qmeta = g.qmeta; b.qdesc = g.qdesc;
  HIPCHK(c, trk_launch(b, 1, Q, st));
  // MapPoint::IncreaseVisible of the points the frame holds and of the queries in view (Tracking.cc:1408-1425, :1456); not when the search refuses
  HIPCHK(c, tc_visible_launch(db->d_visible, db->d_cnt, db->P_cnt, g.out_ids, b.inview, Q, b.pstat + 2, st));
  if (const int rc = down.fetch(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(st));

  if (trk_plan_refused(pl, down) >= 0) return bad(TRK_REFUSED);   // a refused search leaves the caller's arrays
  down.hand_out();
  if (in_view) {   // int32 on the device, uint8 for the caller
    const int32_t* iv = down.host<int32_t>(pl.d_inview);
    for (size_t i = 0; i < q; i++) in_view[i] = (uint8_t)iv[i];
  }
  if (nmatches) *nmatches = down.host<int32_t>(pl.d_pstat)[0];
  return DSH_OK;
}

}  // extern "C"
