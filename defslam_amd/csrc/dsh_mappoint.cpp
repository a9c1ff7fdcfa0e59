// Host side of the map point upkeep (include/defslam_hip.h: dsh_kfdb_*, dsh_mappoint_update): the keyframe store in HBM (descriptor rows
// and camera centres, and beside them the octaves and scale pyramids that the upkeep on the stores reads: dsh_kfinsert.cpp), validation,
// one packed upload, the launches of mappoint_kernels.hip, one download.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "kfdb_store.h"
#include "mappoint_problem.h"

namespace {

int width_class(int M) { return M <= 8 ? 0 : M <= 16 ? 1 : M <= 32 ? 2 : 3; }

void free_arrays(dsh_kfdb* db) {
  for (void* p : {(void*)db->d_slots, (void*)db->d_rows, (void*)db->d_oct, (void*)db->d_levels, (void*)db->d_sf})
    if (p) (void)hipFree(p);
}

}  // namespace

extern "C" {

int dsh_kfdb_create(dsh_ctx* ctx, int32_t capacity, dsh_kfdb** out) {
  dsh_ctx_base* c = dsh_base(ctx);
  if (!c) return DSH_ERR_ARG;
  if (!out || capacity <= 0 || capacity > (1 << 24)) return dsh_fail(c, DSH_ERR_ARG, "dsh_kfdb_create: bad argument");
  *out = nullptr;
  if (const int rc = dsh_enter(c, "dsh_kfdb_create")) return rc;
  dsh_kfdb* db = new dsh_kfdb();
  db->row_cap = (long long)capacity * 1024;
  if (hipMalloc((void**)&db->d_slots, sizeof(MpuSlot) * (size_t)capacity) != hipSuccess ||
      hipMalloc((void**)&db->d_rows, 32 * (size_t)db->row_cap) != hipSuccess || hipMalloc((void**)&db->d_oct, (size_t)db->row_cap) != hipSuccess ||
      hipMalloc((void**)&db->d_levels, 4 * (size_t)capacity) != hipSuccess ||
      hipMalloc((void**)&db->d_sf, 4 * MPU_MAX_LEVELS * (size_t)capacity) != hipSuccess) {
    free_arrays(db);
    delete db;
    return dsh_fail(c, DSH_ERR_HIP, "dsh_kfdb_create: out of device memory");
  }
  db->cap = capacity;
  dsh_attach_store(c, db);
  *out = db;
  return DSH_OK;
}

int dsh_kfdb_destroy(dsh_kfdb* db) {
  if (!db) return DSH_ERR_ARG;
  dsh_store_unregister(db);
  free_arrays(db);
  delete db;
  return DSH_OK;
}

int dsh_kfdb_clear(dsh_kfdb* db) {
  DSH_STORE_ENTER("dsh_kfdb_clear");
  db->count = 0;
  db->rows = 0;
  db->n_octave_over = 0;
  db->kf.clear();
  return DSH_OK;
}

int32_t dsh_kfdb_count(const dsh_kfdb* db) { return db ? db->count : -1; }

int dsh_kfdb_set_bad(dsh_kfdb* db, int32_t slot, int32_t bad_flag) {
  DSH_STORE_ENTER("dsh_kfdb_set_bad");
  if (slot < 0 || slot >= db->count) return bad("slot outside the store");
  db->kf[slot].bad = bad_flag ? 1 : 0;   // read by the host when it lists a call's election rows
  return DSH_OK;
}

int dsh_kfdb_add(dsh_kfdb* db, const dsh_mp_keyframe* kf, int32_t* slot) {
  DSH_STORE_ENTER("dsh_kfdb_add");
  if (!kf) return bad("keyframe is NULL");
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(kf->Ow[k])) return bad("camera centre not finite");
  DSH_CHECK(kfdb_keyframe_error(db, kf));
  if (hipSetDevice(c->device) != hipSuccess) return refuse(DSH_ERR_HIP, "hipSetDevice failed");
  HIPCHK(c, kfdb_reserve(db, kf->N));
  dsh_kfdb::Kf h = kfdb_mirror(db, kf, kf->bad != 0);
  MpuSlot s;
  s.Ow[0] = kf->Ow[0]; s.Ow[1] = kf->Ow[1]; s.Ow[2] = kf->Ow[2];
  s.row_off = (int32_t)db->rows;
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync(db->d_slots + db->count, &s, sizeof(s), hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(db->d_levels + db->count, &h.levels, 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(db->d_sf + MPU_MAX_LEVELS * (size_t)db->count, h.sf, sizeof(h.sf), hipMemcpyHostToDevice, st));
  if (kf->N > 0) {
    HIPCHK(c, hipMemcpyAsync(db->d_rows + 2 * db->rows, kf->desc, 32 * (size_t)kf->N, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(db->d_oct + db->rows, h.octave.data(), (size_t)kf->N, hipMemcpyHostToDevice, st));
  }
  HIPCHK(c, hipStreamSynchronize(st));
  const int32_t at = kfdb_push(db, std::move(h));
  if (slot) *slot = at;
  return DSH_OK;
}

int dsh_mappoint_update(dsh_ctx* ctx, dsh_kfdb* db, int P, const float* xyz, const int32_t* obs_ptr, const int32_t* obs_kf,
                        const int32_t* obs_idx, const int32_t* ref_kf, int32_t what, uint8_t* desc, int32_t* best, float* normal,
                        float* max_distance, float* min_distance, int32_t* status) {
  dsh_ctx_base* c = dsh_base(ctx);
  if (!c) return DSH_ERR_ARG;
  auto bad = [&](const std::string& m) { return dsh_fail(c, DSH_ERR_ARG, "dsh_mappoint_update: " + m); };
  // arguments that need no store
  if (P < 0) return bad("P < 0");
  if (what < 1 || what > (DSH_MP_DESCRIPTOR | DSH_MP_NORMAL_DEPTH)) return bad("what is not a non-empty mask of DSH_MP_DESCRIPTOR, DSH_MP_NORMAL_DEPTH");
  const bool want_d = (what & DSH_MP_DESCRIPTOR) != 0, want_g = (what & DSH_MP_NORMAL_DEPTH) != 0;
  if (P > 0 && (!xyz || !obs_ptr)) return bad("xyz or obs_ptr is NULL");
  if (P > 0 && want_d && !desc) return bad("DSH_MP_DESCRIPTOR needs desc");
  if (P > 0 && want_g && (!ref_kf || !normal || !max_distance || !min_distance)) return bad("DSH_MP_NORMAL_DEPTH needs ref_kf, normal, max_distance, min_distance");
  if (P > 0 && obs_ptr[0] != 0) return bad("obs_ptr[0] != 0");
  for (int p = 0; p < P; p++) {
    const long long m = (long long)obs_ptr[p + 1] - obs_ptr[p];
    if (m < 0) return bad("obs_ptr decreases at point " + std::to_string(p));
    if (m > DSH_MP_MAX_OBS) return bad("point " + std::to_string(p) + " has more than 65535 observations");
  }
  const long long Mt = P > 0 ? obs_ptr[P] : 0;
  if (Mt > 0 && (!obs_kf || !obs_idx)) return bad("obs_kf or obs_idx is NULL");
  if (db && db->ctx != c) return bad("the store belongs to another context or was detached");
  if (const int rc = dsh_enter(c, "dsh_mappoint_update")) return rc;
  if (!db) return bad("store is NULL");

  // arguments against the store; the election lists and the reference levels on the way
  std::vector<int32_t> stamp(db->count, 0), el_obs;   // el_obs: observation index of each election row
  std::vector<MpuPoint> pts(P);
  std::vector<int32_t> el_row;
  std::vector<uint8_t> no_good(P, 0);
  el_row.reserve(want_d ? Mt : 0);
  el_obs.reserve(want_d ? Mt : 0);
  for (int p = 0; p < P; p++) {
    MpuPoint& q = pts[p];
    std::memset(&q, 0, sizeof(q));
    q.x = xyz[3 * p]; q.y = xyz[3 * p + 1]; q.z = xyz[3 * p + 2];
    q.obs_off = obs_ptr[p];
    q.M = obs_ptr[p + 1] - obs_ptr[p];
    q.el_off = (int32_t)el_row.size();
    q.ref_slot = -1;
    q.what = what;
    const std::string at = "point " + std::to_string(p) + ": ";
    const int32_t ref = want_g && q.M > 0 ? ref_kf[p] : -1;
    if (want_g && q.M > 0 && (ref < 0 || ref >= db->count)) return bad(at + "reference keyframe slot outside the store");
    int32_t ref_idx = 0;   // observations[pRefKF] of a copy that lacks pRefKF inserts and yields 0
    int ngood = 0;
    for (int m = 0; m < q.M; m++) {
      const int32_t s = obs_kf[q.obs_off + m], j = obs_idx[q.obs_off + m];
      if (s < 0 || s >= db->count) return bad(at + "keyframe slot outside the store");
      if (stamp[s] == p + 1) return bad(at + "keyframe slot " + std::to_string(s) + " repeated");
      stamp[s] = p + 1;
      const dsh_kfdb::Kf& k = db->kf[s];
      if (j < 0 || j >= k.N) return bad(at + "obs_idx outside the keyframe's key points");
      if (s == ref) ref_idx = j;
      ngood += !k.bad;
      if (want_d && !k.bad) {
        el_row.push_back((int32_t)(k.row_off + j));
        el_obs.push_back(m);
      }
    }
    q.Me = (int32_t)el_row.size() - q.el_off;
    if (q.M > 0 && ngood == 0) no_good[p] = 1;
    if (want_g && q.M > 0) {
      const dsh_kfdb::Kf& k = db->kf[ref];
      if (ref_idx >= k.N) return bad(at + "the reference keyframe has no key point 0");
      const int level = k.octave[ref_idx];
      if (level >= k.levels) return bad(at + "reference octave >= levels");
      q.ref_slot = ref;
      q.sf_level = k.sf[level];
      q.sf_last = k.sf[k.levels - 1];
    }
  }
  if (P == 0) return DSH_OK;

  // work lists: small points by width class; large points biggest first, each a normal block and its election row blocks
  std::vector<int32_t> small_order, large_pts;
  std::vector<int32_t> cls_n(4, 0);
  for (int p = 0; p < P; p++) {
    const int M = pts[p].M;
    if (M == 0) continue;
    if (M <= MPU_SMALL) cls_n[width_class(M)]++;
    else large_pts.push_back(p);
  }
  int32_t small_off[5] = {0, 0, 0, 0, 0};
  for (int k = 0; k < 4; k++) small_off[k + 1] = small_off[k] + cls_n[k];
  small_order.resize(small_off[4]);
  {
    int32_t cur[4] = {small_off[0], small_off[1], small_off[2], small_off[3]};
    for (int p = 0; p < P; p++)
      if (pts[p].M > 0 && pts[p].M <= MPU_SMALL) small_order[cur[width_class(pts[p].M)]++] = p;
  }
  std::stable_sort(large_pts.begin(), large_pts.end(), [&](int a, int b) { return pts[a].M > pts[b].M; });
  std::vector<int32_t> blocks;   // pairs (point, first row or -1)
  for (int p : large_pts) {
    if (want_g) { blocks.push_back(p); blocks.push_back(-1); }
    if (want_d)
      for (int r = 0; r < pts[p].Me; r += MPU_ROWS) { blocks.push_back(p); blocks.push_back(r); }
  }
  const int NB = (int)blocks.size() / 2, NL = (int)large_pts.size();
  const size_t Met = el_row.size();

  // one host buffer, one copy up
  UpBlock up;
  DownBlock down;
  const size_t o_pts = up.copy_of(pts.data(), sizeof(MpuPoint) * P), o_oslot = up.copy_of(obs_kf, 4 * (size_t)Mt), o_el = up.copy_of(el_row.data(), 4 * Met),
               o_small = up.copy_of(small_order.data(), 4 * small_order.size()), o_blk = up.copy_of(blocks.data(), 4 * blocks.size()),
               o_lpts = up.copy_of(large_pts.data(), 4 * (size_t)NL);
  const size_t d_best = down.take(4 * (size_t)P), d_desc = down.take(32 * (size_t)P), d_nrm = down.take(12 * (size_t)P), d_dist = down.take(8 * (size_t)P);
  hipStream_t st = c->stream;
  MpuBufs b;
  if (const int rc = up.copy(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  HIPCHK(c, dsh_scratch_array(c, &b.large_key, (size_t)P));
  if (NL > 0) HIPCHK(c, hipMemsetAsync(b.large_key, 0xFF, 4 * (size_t)P, st));
  b.slots = db->d_slots;
  b.rows = db->d_rows;
  b.pts = up.dev<const MpuPoint>(o_pts);
  b.obs_slot = up.dev<const int32_t>(o_oslot);
  b.el_row = up.dev<const int32_t>(o_el);
  b.small_order = up.dev<const int32_t>(o_small);
  b.large_blocks = up.dev<const int2>(o_blk);
  b.large_pts = up.dev<const int32_t>(o_lpts);
  b.best = down.dev<int32_t>(d_best);
  b.desc = down.dev<uint4>(d_desc);
  b.normal = down.dev<float>(d_nrm);
  b.dist = down.dev<float>(d_dist);
  HIPCHK(c, mpu_launch(b, small_off, NB, NL, st));
  if (const int rc = down.fetch(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(st));

  // outputs by hand: only what was asked for, only where the reference writes, which the flags that came down decide per point
  const int32_t* obest = down.host<int32_t>(d_best);
  const float* onrm = down.host<float>(d_nrm);
  const float* odist = down.host<float>(d_dist);
  for (int p = 0; p < P; p++) {
    const MpuPoint& q = pts[p];
    int32_t flags = 0;
    if (q.M == 0) flags |= DSH_MP_NO_OBS;
    if (no_good[p]) flags |= DSH_MP_NO_GOOD_DESC;
    if (want_d) {
      const bool elected = q.Me > 0;
      if (best) best[p] = elected ? el_obs[q.el_off + obest[p]] : -1;
      if (elected) std::memcpy(desc + 32 * (size_t)p, down.host<uint4>(d_desc) + 2 * (size_t)p, 32);
    }
    if (want_g && q.M > 0) {
      std::memcpy(normal + 3 * (size_t)p, onrm + 3 * (size_t)p, 12);
      max_distance[p] = odist[2 * (size_t)p];
      min_distance[p] = odist[2 * (size_t)p + 1];
    }
    if (status) status[p] = flags;
  }
  return DSH_OK;
}

}  // extern "C"
