// Host side of the erase on the resident map point store (include/defslam_hip.h: dsh_point_store_erase_observations,
// dsh_point_store_set_bad, dsh_point_store_cull, dsh_point_store_get_observations, dsh_point_store_get_keyframe_table): validation
// against the host mirror, one upload, the launches of pointerase_kernels.hip and one download; afterwards the mirror drops exactly the
// keys the device reports erased.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "mpdb_store.h"
#include "pointerase_problem.h"

namespace {

// One erase call from the device gate on: mode PE_*; slots and first_kf as the mode needs them; code[n] receives the status or the action.
int run(dsh_mpdb* db, dsh_ctx_base* c, int mode, int n, const int32_t* ids, const int32_t* slots, const int32_t* first_kf, int32_t erase_match,
        int32_t current_kf, uint8_t* code, dsh_point_erase_counts* out) {
  std::memset(out, 0, sizeof(*out));   // a refused call leaves the caller's counts as they were
  if (n == 0) return DSH_OK;
  const size_t m = (size_t)n, cap = db->obs.size();   // the sweep erases live records only, and the mirror knows how many there are
  UpBlock up;
  const size_t o_ids = up.copy_of(ids, 4 * m), o_slots = up.copy_of(mode == PE_ERASE ? slots : nullptr, 4 * m),
               o_first = up.copy_of(mode == PE_CULL ? first_kf : nullptr, 4 * m), o_rec = up.take_exact(mode == PE_ERASE ? 8 * m : 0);
  DownBlock down;
  const size_t d_hdr = down.take(sizeof(PeHdr)), d_code = down.take(mode == PE_SET_BAD ? 0 : m);
  down.copy_to(d_code, mode == PE_SET_BAD ? nullptr : code, m);   // the kernel writes the codes whether the caller wants them or not
  const size_t head = down.size;                      // what every call fetches; the erased list lies behind it
  const size_t d_erased = down.take_exact(8 * cap);
  if (const int rc = up.stage(c)) return rc;
  if (mode == PE_ERASE) {
    long long* rec = up.host<long long>(o_rec);       // 64-bit positions: a log of any length
    for (int i = 0; i < n; i++) {
      const auto it = db->obs.find(mpdb_obs_key(ids[i], slots[i]));
      rec[i] = it == db->obs.end() ? -1 : it->second;
    }
  }
  if (const int rc = up.send(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;

  PeBufs b;
  std::memset(&b, 0, sizeof(b));
  b.P = db->P; b.n = n; b.mode = mode; b.erase_match = erase_match; b.current_kf = current_kf; b.R = db->R;
  b.bad = db->d_bad; b.ref_kf = db->d_ref_kf; b.nobs = db->d_nobs; b.found = db->d_found; b.visible = db->d_visible;
  b.log = db->d_log; b.log_idx = db->d_log_idx; b.kf = db->d_kf; b.table = db->d_table;
  b.ids = up.dev<const int32_t>(o_ids); b.slots = up.dev<const int32_t>(o_slots); b.first_kf = up.dev<const int32_t>(o_first);
  b.rec = up.dev<const long long>(o_rec);
  HIPCHK(c, dsh_scratch_array(c, &b.mark, (size_t)db->P));
  HIPCHK(c, dsh_scratch_array(c, &b.cand, (size_t)db->P));
  b.hdr = down.dev<PeHdr>(d_hdr);
  b.out_code = mode == PE_SET_BAD ? nullptr : down.dev<uint8_t>(d_code);
  b.out_erased = down.dev<int2>(d_erased);
  HIPCHK(c, pe_erase_launch(b, c->stream));
  // the head of the block comes down; the used part of the erased list follows when the sweep erased records
  HIPCHK(c, hipMemcpyAsync(down.h, down.d, head, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const PeHdr h = *down.host<PeHdr>(d_hdr);
  if (h.n_erased > 0) {
    HIPCHK(c, hipMemcpyAsync(down.h + d_erased, down.d + d_erased, 8 * (size_t)h.n_erased, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }

  // the host mirror follows: the pairs that were found and the records of the points that became bad
  if (mode == PE_ERASE) {
    const long long* rec = up.host<long long>(o_rec);
    for (int i = 0; i < n; i++)
      if (rec[i] >= 0) db->obs.erase(mpdb_obs_key(ids[i], slots[i]));
  }
  const int2* erased = down.host<int2>(d_erased);
  for (int j = 0; j < h.n_erased; j++) db->obs.erase(mpdb_obs_key(erased[j].x, erased[j].y));
  out->n_found = h.n_found; out->n_ref_moved = h.n_ref_moved; out->n_set_bad = h.n_set_bad;
  out->n_records = h.n_found + h.n_erased;
  out->n_entries = (erase_match ? h.n_found : 0) + h.n_erased;
  down.hand_out();
  return DSH_OK;
}

}  // namespace

extern "C" {

int dsh_point_store_erase_observations(dsh_mpdb* db, int n, const int32_t* point_ids, const int32_t* keyframe_slots, int32_t erase_match,
                                       uint8_t* status, dsh_point_erase_counts* out) {
  DSH_STORE_ENTER("dsh_point_store_erase_observations");
  if (!out) return bad("out is NULL");
  if (n > 0 && !keyframe_slots) return bad("keyframe_slots is NULL");
  DSH_CHECK(mpdb_ids_error(n, point_ids, db->P, "point id", true));
  for (int i = 0; i < n; i++)
    if (keyframe_slots[i] < 0 || keyframe_slots[i] >= db->K) return bad("pair " + std::to_string(i) + ": keyframe slot outside the store");
  if (!db->unindexed.empty()) return mpdb_unindexed_error(db, who__);
  DSH_STORE_GATE();
  return run(db, c, PE_ERASE, n, point_ids, keyframe_slots, nullptr, erase_match ? 1 : 0, 0, status, out);
}

int dsh_point_store_set_bad(dsh_mpdb* db, int n, const int32_t* ids, dsh_point_erase_counts* out) {
  DSH_STORE_ENTER("dsh_point_store_set_bad");
  if (!out) return bad("out is NULL");
  DSH_CHECK(mpdb_ids_error(n, ids, db->P, "point id", true));
  if (!db->unindexed.empty()) return mpdb_unindexed_error(db, who__);
  DSH_STORE_GATE();
  return run(db, c, PE_SET_BAD, n, ids, nullptr, nullptr, 0, 0, nullptr, out);
}

int dsh_point_store_cull(dsh_mpdb* db, int n, const int32_t* ids, const int32_t* first_kf, int32_t current_kf, uint8_t* action,
                         dsh_point_erase_counts* out) {
  DSH_STORE_ENTER("dsh_point_store_cull");
  if (!out) return bad("out is NULL");
  DSH_CHECK(mpdb_ids_error(n, ids, db->P, "point id", true));
  if (n > 0 && (!first_kf || !action)) return bad("first_kf or action is NULL");
  if (!db->unindexed.empty()) return mpdb_unindexed_error(db, who__);
  DSH_STORE_GATE();
  return run(db, c, PE_CULL, n, ids, nullptr, first_kf, 0, current_kf, action, out);
}

int dsh_point_store_get_observations(dsh_mpdb* db, int n, const int32_t* ids, int32_t* obs_ptr, int32_t capacity, int32_t* slots, int32_t* idx,
                                     int32_t* n_total) {
  DSH_STORE_ENTER("dsh_point_store_get_observations");
  DSH_CHECK(mpdb_ids_error(n, ids, db->P, "point id", true));
  if (!obs_ptr || !n_total) return bad("obs_ptr or n_total is NULL");
  if (capacity < 0) return bad("capacity < 0");
  if (capacity > 0 && (!slots || !idx)) return bad("slots or idx is NULL");
  if (db->obs.size() > (size_t)INT32_MAX) return bad("store full");
  DSH_STORE_GATE();
  *n_total = 0;
  const size_t m = (size_t)n, live = db->obs.size(), cap = std::min((size_t)capacity, live);
  UpBlock up;
  const size_t o_ids = up.take_exact(4 * m);
  up.copy_of(o_ids, ids, 4 * m);
  DownBlock down;
  const size_t d_hdr = down.take(sizeof(PeHdr)), d_ptr = down.copy_to(obs_ptr, 4 * (m + 1)), d_slot = down.take(4 * cap), d_idx = down.take_exact(4 * cap);
  if (const int rc = up.copy(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  PeObsBufs b;
  std::memset(&b, 0, sizeof(b));
  b.P = db->P; b.n = n; b.cap = (int32_t)cap; b.ids = up.dev<const int32_t>(o_ids);
  HIPCHK(c, mpdb_obs_lists(db, b.ol, m, live));
  b.hdr = down.dev<PeHdr>(d_hdr);
  b.ol.off = down.dev<int32_t>(d_ptr); b.out_slot = down.dev<int32_t>(d_slot); b.out_idx = down.dev<int32_t>(d_idx);
  HIPCHK(c, pe_observations_launch(b, c->stream));
  if (const int rc = down.fetch(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int32_t total = down.host<PeHdr>(d_hdr)->total;
  *n_total = total;
  if (total > capacity)   // a refused call leaves the caller's arrays
    return bad("capacity " + std::to_string(capacity) + " is too small for the " + std::to_string(total) + " observations of the points");
  down.hand_out();
  if (total > 0) {   // the lists: their length came down with them
    std::memcpy(slots, down.host<int32_t>(d_slot), 4 * (size_t)total);
    std::memcpy(idx, down.host<int32_t>(d_idx), 4 * (size_t)total);
  }
  return DSH_OK;
}

int dsh_point_store_get_keyframe_table(dsh_mpdb* db, int32_t slot, int32_t capacity, int32_t* points) {
  DSH_STORE_ENTER("dsh_point_store_get_keyframe_table");
  if (slot < 0 || slot >= db->K) return bad("slot outside the store");
  const LmKf k = db->kf[slot];
  if (capacity < k.N) return bad("capacity " + std::to_string(capacity) + " is too small for the keyframe's " + std::to_string(k.N) + " key points");
  if (k.N > 0 && !points) return bad("points is NULL");
  DSH_STORE_GATE();
  if (k.N == 0) return DSH_OK;
  DownBlock down;
  down.copy_to(down.take_exact(4 * (size_t)k.N), points, 4 * (size_t)k.N);   // an exact slice: the block lies over the store's table
  if (const int rc = down.at(c, db->d_table + k.tab_off)) return rc;
  return down.receive(c);
}

}  // extern "C"
