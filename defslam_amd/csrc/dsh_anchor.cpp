// Host side of the anchor keyframes of a new keyframe on the map point store (include/defslam_hip.h: dsh_point_store_set_reference_keyframes,
// dsh_point_store_get_reference_keyframes, dsh_keyframe_anchors): validation against the host mirror, the launches of anchor_kernels.hip and
// one download.  Nothing goes up: the call's inputs are a slot and a threshold, which travel as kernel arguments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/defslam_hip.h"
#include "anchor_problem.h"
#include "dsh_ctx.h"
#include "mpdb_store.h"

namespace {

const long long AN_DEFAULT_MATRIX_BYTES = 64ll << 20;

}  // namespace

extern "C" {

int dsh_point_store_set_reference_keyframes(dsh_mpdb* db, int n, const int32_t* ids, const int32_t* slots) {
  DSH_STORE_ENTER("dsh_point_store_set_reference_keyframes");
  DSH_CHECK(mpdb_ids_error(n, ids, db->P, "point id"));
  if (n > 0 && !slots) return bad("slots is NULL");
  for (int i = 0; i < n; i++)
    if (slots[i] < -1 || slots[i] >= db->K) return bad("slots[" + std::to_string(i) + "] is neither -1 nor a slot of the store");
  DSH_STORE_GATE();
  if (n == 0) return DSH_OK;
  UpBlock up;
  const size_t m = (size_t)n, o_ids = up.copy_of(ids, 4 * m), o_val = up.copy_of(slots, 4 * m);
  if (const int rc = up.copy(c)) return rc;
  HIPCHK(c, lm_scatter_i32_launch(db->d_ref_kf, up.dev<const int32_t>(o_ids), up.dev<const int32_t>(o_val), 0, n, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return DSH_OK;
}

int dsh_point_store_get_reference_keyframes(dsh_mpdb* db, int n, const int32_t* ids, int32_t* slots_out) {
  DSH_STORE_ENTER("dsh_point_store_get_reference_keyframes");
  DSH_CHECK(mpdb_ids_error(n, ids, db->P, "point id"));
  if (n > 0 && !slots_out) return bad("slots_out is NULL");
  DSH_STORE_GATE();
  if (n == 0) return DSH_OK;
  UpBlock up;
  const size_t m = (size_t)n, o_ids = up.copy_of(ids, 4 * m);
  DownBlock down;
  const size_t d_val = down.copy_to(slots_out, 4 * m);
  if (const int rc = up.copy(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  HIPCHK(c, an_gather_i32_launch(db->d_ref_kf, up.dev<const int32_t>(o_ids), n, down.dev<int32_t>(d_val), c->stream));
  return down.receive(c);
}

int dsh_keyframe_anchors(dsh_mpdb* db, int32_t slot, int32_t min_pairs, dsh_anchor_lists* out) {
  DSH_STORE_ENTER("dsh_keyframe_anchors");
  if (!out) return bad("out is NULL");
  out->n_anchors = out->n_pairs = out->n_queries = out->n_no_ref = 0;
  if (slot < 0 || slot >= db->K) return bad("slot outside the store");
  if (min_pairs < 0) return bad("min_pairs < 0");
  const LmKf nk = db->kf[slot];
  if (nk.N > AN_MAX_KEYPOINTS) return bad("the keyframe has more than 8192 key points");
  if (out->anchor_capacity < 0 || out->pair_capacity < 0 || out->query_capacity < 0) return bad("a capacity is negative");
  if (out->max_matrix_bytes < 0) return bad("max_matrix_bytes < 0");
  if (!out->pair_ptr || !out->query_ptr) return bad("pair_ptr or query_ptr is NULL");
  if (out->anchor_capacity > 0 && (!out->anchor_slot || !out->anchor_count || !out->anchor_pairs)) return bad("an anchor array is NULL");
  if (out->pair_capacity > 0 && (!out->pair_idx1 || !out->pair_idx2 || !out->pair_point || !out->pair_own)) return bad("a pair array is NULL");
  if (out->query_capacity > 0 && (!out->query_idx1 || !out->query_point)) return bad("a query array is NULL");
  if (!db->unindexed.empty()) return mpdb_unindexed_error(db, who__);
  DSH_STORE_GATE();

  // what the host knows of the sizes: an anchor takes a vote of an entry, a pair an entry per anchor, a query an entry of a table
  const long long N = nk.N, Amax = std::min<long long>(db->K, N);
  const size_t P = (size_t)db->P, K = (size_t)db->K, am = (size_t)std::max<long long>(Amax, 1);
  const size_t ca = (size_t)std::min<long long>(out->anchor_capacity, Amax), cp = (size_t)std::min<long long>(out->pair_capacity, Amax * N),
               cq = (size_t)std::min<long long>(out->query_capacity, db->T);
  const long long budget = out->max_matrix_bytes > 0 ? out->max_matrix_bytes : AN_DEFAULT_MATRIX_BYTES;
  const long long chunk = std::max<long long>(1, std::min<long long>(am, budget / (4 * std::max<long long>(N, 1))));

  DownBlock down;
  const size_t d_hdr = down.take(sizeof(AnHdr)), d_slot = down.take(4 * ca), d_count = down.take(4 * ca), d_np = down.take(4 * ca),
               d_pptr = down.take(4 * (ca + 1)), d_qptr = down.take(4 * (ca + 1)), d_i1 = down.take(4 * cp), d_i2 = down.take(4 * cp),
               d_pt = down.take(4 * cp), d_own = down.take(cp), d_q1 = down.take(4 * cq), d_qp = down.take(4 * cq), d_has = down.take((size_t)N);
  down.copy_to(d_has, out->has, (size_t)N);   // the kernel writes it whether the caller wants it or not
  if (const int rc = down.alloc(c)) return rc;
  AnBufs b;
  std::memset(&b, 0, sizeof(b));
  b.P = db->P; b.K = db->K; b.N = nk.N; b.slot = slot; b.min_pairs = min_pairs; b.tab_off = nk.tab_off;
  b.max_anchors = (int32_t)Amax;
  b.R = db->R;
  b.bad = db->d_bad; b.ref_kf = db->d_ref_kf; b.log = db->d_log; b.log_idx = db->d_log_idx; b.kf = db->d_kf; b.table = db->d_table;
  HIPCHK(c, dsh_scratch_array(c, &b.first_i, P));
  HIPCHK(c, dsh_scratch_array(c, &b.mult, P));
  HIPCHK(c, dsh_scratch_array(c, &b.idx2_of, P));
  HIPCHK(c, dsh_scratch_array(c, &b.votes, K));
  HIPCHK(c, dsh_scratch_array(c, &b.rank, K));
  HIPCHK(c, dsh_scratch_array(c, &b.a_slot, am));
  HIPCHK(c, dsh_scratch_array(c, &b.a_pairs, am));
  HIPCHK(c, dsh_scratch_array(c, &b.a_queries, am));
  HIPCHK(c, dsh_scratch_array(c, &b.pptr, am + 1));
  HIPCHK(c, dsh_scratch_array(c, &b.qptr, am + 1));
  HIPCHK(c, dsh_scratch_array(c, &b.matrix, (size_t)chunk * (size_t)std::max<long long>(N, 1)));
  HIPCHK(c, dsh_scratch_array(c, &b.hdr, 1));
  b.chunk = (int32_t)chunk;
  b.cap_anchors = (int32_t)ca; b.cap_pairs = (int32_t)cp; b.cap_queries = (int32_t)cq;
  b.out_hdr = down.dev<AnHdr>(d_hdr);
  b.out_slot = down.dev<int32_t>(d_slot); b.out_count = down.dev<int32_t>(d_count); b.out_npairs = down.dev<int32_t>(d_np);
  b.out_pptr = down.dev<int32_t>(d_pptr); b.out_qptr = down.dev<int32_t>(d_qptr);
  b.out_idx1 = down.dev<int32_t>(d_i1); b.out_idx2 = down.dev<int32_t>(d_i2); b.out_point = down.dev<int32_t>(d_pt);
  b.out_own = down.dev<uint8_t>(d_own);
  b.out_qidx1 = down.dev<int32_t>(d_q1); b.out_qpoint = down.dev<int32_t>(d_qp);
  b.out_has = down.dev<uint8_t>(d_has);
  HIPCHK(c, an_anchors_launch(b, c->stream));
  if (const int rc = down.fetch(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));

  const AnHdr h = *down.host<AnHdr>(d_hdr);
  out->n_anchors = h.n_anchors; out->n_pairs = h.n_pairs; out->n_queries = h.n_queries; out->n_no_ref = h.n_no_ref;
  if (h.n_anchors > out->anchor_capacity || h.n_pairs > out->pair_capacity || h.n_queries > out->query_capacity)   // leaves the caller's arrays
    return bad("the lists do not fit: " + std::to_string(h.n_anchors) + " anchors, " + std::to_string(h.n_pairs) + " pairs and " +
               std::to_string(h.n_queries) + " queries are needed (n_anchors, n_pairs, n_queries of out)");
  down.hand_out();
  // the lists: their lengths came down with them
  const size_t A = (size_t)h.n_anchors, np = (size_t)h.n_pairs, nq = (size_t)h.n_queries;
  if (A > 0) {
    std::memcpy(out->anchor_slot, down.host<int32_t>(d_slot), 4 * A);
    std::memcpy(out->anchor_count, down.host<int32_t>(d_count), 4 * A);
    std::memcpy(out->anchor_pairs, down.host<int32_t>(d_np), 4 * A);
  }
  std::memcpy(out->pair_ptr, down.host<int32_t>(d_pptr), 4 * (A + 1));
  std::memcpy(out->query_ptr, down.host<int32_t>(d_qptr), 4 * (A + 1));
  if (np > 0) {
    std::memcpy(out->pair_idx1, down.host<int32_t>(d_i1), 4 * np);
    std::memcpy(out->pair_idx2, down.host<int32_t>(d_i2), 4 * np);
    std::memcpy(out->pair_point, down.host<int32_t>(d_pt), 4 * np);
    std::memcpy(out->pair_own, down.host<uint8_t>(d_own), np);
  }
  if (nq > 0) {
    std::memcpy(out->query_idx1, down.host<int32_t>(d_q1), 4 * nq);
    std::memcpy(out->query_point, down.host<int32_t>(d_qp), 4 * nq);
  }
  return DSH_OK;
}

}  // extern "C"
