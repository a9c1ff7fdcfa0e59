// C ABI of the device-resident DiffProp database (include/defslam_hip.h: dsh_diffdb_*, dsh_normals_estimate_db): the records of
// SchwarpDatabase::calculateSchwarps stay in HBM between the Schwarp fits and NormalEstimator::ObtainK1K2.  dsh_normals_estimate_db groups
// and gathers them, then runs the normals stage it shares with dsh_normals_estimate (dsh::normals_stage, dsh_nrsfm.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "dsh_diffdb.h"
#include "mapping_launch.h"

extern "C" {

int dsh_diffdb_create(dsh_ctx* ctx, int64_t capacity, dsh_diffdb** out) {
  dsh_ctx_base* c = dsh_base(ctx);
  if (!c || !out || capacity <= 0 || capacity > (int64_t)1 << 30) return dsh_fail(c, DSH_ERR_ARG, "dsh_diffdb_create: bad argument");
  *out = nullptr;
  if (const int rc = dsh_enter(c, "dsh_diffdb_create")) return rc;
  dsh_diffdb* db = new dsh_diffdb();
  db->cap = capacity;
  char* base = nullptr;
  const size_t bytes = (size_t)capacity * (72 + 12);
  if (hipMalloc((void**)&base, bytes) != hipSuccess) { delete db; return dsh_fail(c, DSH_ERR_HIP, "dsh_diffdb_create: out of device memory"); }
  db->rec = reinterpret_cast<float*>(base);
  db->pid = reinterpret_cast<int32_t*>(base + (size_t)capacity * 72);
  db->tag = db->pid + capacity;
  db->idx2 = db->tag + capacity;
  dsh_attach_store(c, db);
  *out = db;
  return DSH_OK;
}

int dsh_diffdb_destroy(dsh_diffdb* db) {
  if (!db) return DSH_ERR_ARG;
  dsh_store_unregister(db);
  if (db->rec) (void)hipFree(db->rec);
  if (db->last_normals) (void)hipFree(db->last_normals);
  delete db;
  return DSH_OK;
}

}  // extern "C"

int ddb_reserve(dsh_diffdb* db, long long need) {
  if (need <= db->cap) return 0;
  if (need > (1ll << 30)) return (int)hipErrorOutOfMemory;
  const long long ncap = std::min<long long>(std::max(need, 2 * db->cap), 1ll << 30);
  (void)hipSetDevice(db->device);
  void* base = db->rec;
  int32_t *pid = nullptr, *tag = nullptr, *idx2 = nullptr;
  const hipError_t e = dsh_store_grow(&base, (size_t)ncap * (72 + 12), [&](char* q) {
    pid = reinterpret_cast<int32_t*>(q + (size_t)ncap * 72);
    tag = pid + ncap;
    idx2 = tag + ncap;
    const size_t n = (size_t)db->count;
    hipError_t r = hipSuccess;
    if (n) {
      r = hipMemcpy(q, db->rec, 72 * n, hipMemcpyDeviceToDevice);
      if (r == hipSuccess) r = hipMemcpy(pid, db->pid, 4 * n, hipMemcpyDeviceToDevice);
      if (r == hipSuccess) r = hipMemcpy(tag, db->tag, 4 * n, hipMemcpyDeviceToDevice);
      if (r == hipSuccess) r = hipMemcpy(idx2, db->idx2, 4 * n, hipMemcpyDeviceToDevice);
    }
    return r;
  });
  if (e != hipSuccess) return (int)e;
  db->rec = static_cast<float*>(base); db->pid = pid; db->tag = tag; db->idx2 = idx2; db->cap = ncap;
  return 0;
}

extern "C" {

int dsh_diffdb_clear(dsh_diffdb* db) {
  if (!db) return DSH_ERR_ARG;
  db->count = 0;
  db->max_pid = -1;
  db->last_P = db->last_R = 0;
  return DSH_OK;
}

int64_t dsh_diffdb_count(const dsh_diffdb* db) { return db ? (int64_t)db->count : -1; }

int dsh_diffdb_append(dsh_diffdb* db, int n, const dsh_diffprop* recs, const int32_t* point_id, const int32_t* tag, const int32_t* idx2) {
  DSH_STORE_ENTER("dsh_diffdb_append");
  if (n < 0 || (n > 0 && (!recs || !point_id))) return bad("bad argument");
  if (n == 0) return DSH_OK;
  (void)hipSetDevice(c->device);
  if (ddb_reserve(db, db->count + n) != 0) return refuse(DSH_ERR_HIP, "out of device memory while growing the database");
  hipStream_t st = c->stream;
  std::vector<int32_t> fill;
  const std::vector<int32_t> zeros(tag ? 0 : (size_t)n, 0);   // lives until the stream synchronisation below
  HIPCHK(c, hipMemcpyAsync(db->rec + 18 * (size_t)db->count, recs, 72 * (size_t)n, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(db->pid + db->count, point_id, 4 * (size_t)n, hipMemcpyHostToDevice, st));
  if (!tag || !idx2) { fill.assign(n, 0); if (!idx2) for (int i = 0; i < n; i++) fill[i] = i; }
  HIPCHK(c, hipMemcpyAsync(db->tag + db->count, tag ? tag : zeros.data(), 4 * (size_t)n, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(db->idx2 + db->count, idx2 ? idx2 : fill.data(), 4 * (size_t)n, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipStreamSynchronize(st));
  for (int i = 0; i < n; i++) db->max_pid = std::max(db->max_pid, point_id[i]);
  db->count += n;
  return DSH_OK;
}

int dsh_normals_estimate_db(dsh_ctx* ctx, dsh_diffdb* db, int P, const int32_t* point_ids, const float* x0, const uint8_t* has_x0, const float* ref_uv,
                            double* k1k2, double* cov, int32_t* status, float* normal_ref, int32_t* iters, int32_t max_rec, int32_t* n_rec, int32_t* rec_point,
                            int32_t* rec_tag, int32_t* rec_idx2, float* normal_rec, uint8_t* rec_written) {
  dsh_ctx_base* c = dsh_base(ctx);
  if (!c) return DSH_ERR_ARG;
  if (const int rc = dsh_enter(c, "dsh_normals_estimate_db")) return rc;
  if (!db || db->ctx != c || P < 0 || (P > 0 && (!point_ids || !x0 || !has_x0 || !ref_uv || !k1k2 || !status)) || max_rec < 0)
    return dsh_fail(c, DSH_ERR_ARG, "dsh_normals_estimate_db: bad argument");
  if (n_rec) *n_rec = 0;
  db->last_P = db->last_R = 0;
  if (P == 0) return DSH_OK;
  hipStream_t st = c->stream;
  const long long n = db->count;
  const size_t Pn = (size_t)P, nn = n > 0 ? (size_t)n : 1;
  if (db->max_pid == INT32_MAX) return dsh_fail(c, DSH_ERR_ARG, "dsh_normals_estimate_db: point id 2^31 - 1 is not supported");
  const int nlook = std::max(db->max_pid + 1, 1);
  UpBlock up;
  const size_t o_ids = up.copy_of(point_ids, 4 * Pn), o_x0 = up.copy_of(x0, 8 * Pn), o_hx0 = up.copy_of(has_x0, Pn), o_uv = up.copy_of(ref_uv, 8 * Pn);
  Arena ws;   // work space of the grouping
  const size_t o_look = ws.take(4 * (size_t)nlook), o_key = ws.take(4 * nn), o_count = ws.take(4 * (Pn + 1)), o_cursor = ws.take(4 * (Pn + 1)), o_perm = ws.take(4 * nn),
               o_owner = ws.take(4 * nn), o_tmp = ws.take(ddb_group_tmp_bytes(P)), o_ptr = ws.take(4 * (Pn + 2));
  char* w = nullptr;
  HIPCHK(c, c->scratch.take(ws.size, (void**)&w));
  auto i32 = [&](size_t off) { return reinterpret_cast<int32_t*>(w + off); };
  if (const int rc = up.copy(c)) return rc;
  // group the database by the requested points (a point's records keep their insertion order)
  HIPCHK(c, ddb_group(n, db->pid, P, up.dev<int32_t>(o_ids), nlook, i32(o_look), i32(o_key), i32(o_count), i32(o_cursor), i32(o_perm), i32(o_owner), w + o_tmp,
                      i32(o_ptr), st));
  DownBlock count;   // records that belong to a requested point: the one number the host needs before it can size the launches
  count.take_exact(4);
  if (const int rc = count.at(c, i32(o_ptr) + P)) return rc;
  if (const int rc = count.receive(c)) return rc;
  const int32_t R = *count.host<int32_t>(0);
  if (n_rec) *n_rec = R;
  if ((rec_point || rec_tag || rec_idx2 || normal_rec || rec_written) && R > max_rec)
    return dsh_fail(c, DSH_ERR_ARG, "dsh_normals_estimate_db: " + std::to_string(R) + " records, the per-record buffers hold " + std::to_string(max_rec));
  // the normals stay behind for dsh_sfn_estimate_db (nothing is in flight here: the old allocation can go)
  const long long need = 3ll * P + 3ll * R;
  if (need > db->last_cap) {
    if (db->last_normals) (void)hipFree(db->last_normals);
    db->last_normals = nullptr; db->last_cap = 0;
    if (hipMalloc((void**)&db->last_normals, 4 * (size_t)(need + need / 2)) != hipSuccess) return dsh_fail(c, DSH_ERR_HIP, "dsh_normals_estimate_db: out of device memory");
    db->last_cap = need + need / 2;
  }
  const size_t Rn = R > 0 ? (size_t)R : 1;
  Arena ws2;   // the gathered records and what the host-record route uploads with them
  const size_t o_soa = ws2.take(72 * Rn), o_tag = ws2.take(4 * Rn), o_idx2 = ws2.take(4 * Rn), o_isref = ws2.take(Rn), o_fn = ws2.take(8 * Rn), o_hfn = ws2.take(Rn);
  char* g = nullptr;
  HIPCHK(c, c->scratch.take(ws2.size, (void**)&g));
  float* d_soa = reinterpret_cast<float*>(g + o_soa);
  int32_t *d_tag = reinterpret_cast<int32_t*>(g + o_tag), *d_idx2 = reinterpret_cast<int32_t*>(g + o_idx2);
  HIPCHK(c, ddb_gather(R, i32(o_perm), db->rec, db->tag, db->idx2, d_soa, d_tag, d_idx2, st));
  // every stored record is anchored in its point's reference keyframe (SchwarpDatabase.cc:297: records of other points are not saved)
  HIPCHK(c, hipMemsetAsync(g + o_isref, 1, Rn, st));
  HIPCHK(c, hipMemsetAsync(g + o_fn, 0, 8 * Rn, st));
  HIPCHK(c, hipMemsetAsync(g + o_hfn, 0, Rn, st));
  const dsh::NormalsIn in = {i32(o_ptr), i32(o_owner), d_soa, reinterpret_cast<uint8_t*>(g + o_isref), reinterpret_cast<float*>(g + o_fn),
                             reinterpret_cast<uint8_t*>(g + o_hfn), up.dev<float>(o_x0), up.dev<uint8_t>(o_hx0), up.dev<float>(o_uv),
                             {i32(o_owner), d_tag, d_idx2}, db->last_normals};
  if (const int rc = dsh::normals_stage(c, P, R, in, {k1k2, cov, status, normal_ref, iters, normal_rec, rec_written, {rec_point, rec_tag, rec_idx2}})) return rc;
  db->last_P = P; db->last_R = R;
  return DSH_OK;
}

}  // extern "C"
