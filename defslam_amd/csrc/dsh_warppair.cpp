// Host side of one anchor of SchwarpDatabase::add on the resident stores (include/defslam_hip.h: dsh_keyframe_set_view,
// dsh_keyframe_get_view, dsh_keyframe_warp_pair): validation against the host mirrors of dsh_mpdb, dsh_kfdb and dsh_diffdb, one upload
// block, the launches of warppair_kernels.hip around the stages of dsh_warp_initialize (dsh_sfn.h), dsh_schwarp_eval,
// dsh_search_by_schwarp and the Schwarp fit (dsh_schwarp.h), one count read back in between and one result block; afterwards the
// mirror of the point store follows the records the device appended and blanked.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "dsh_diffdb.h"
#include "dsh_schwarp.h"
#include "dsh_sfn.h"
#include "kfdb_store.h"
#include "mapping_launch.h"
#include "mpdb_store.h"
#include "schwarp_problem.h"
#include "warppair_problem.h"

namespace {

// a store of the call against the point store's context: alive, attached, of that context
bool same_context(const dsh_ctx_base* c, const dsh_store* s) {
  return s && s->ctx == c && std::find(c->stores.begin(), c->stores.end(), s) != c->stores.end();
}

// the keyframe store as the gather reads it: "" or what is wrong
std::string kfdb_error(const dsh_mpdb* db, const dsh_kfdb* kfdb) {
  if (kfdb->count < db->K) return "the keyframe store holds fewer keyframes than the point store";
  for (int s = 0; s < db->K; s++)
    if (kfdb->kf[s].N != db->kf[s].N) return "keyframe " + std::to_string(s) + " has another N in the keyframe store than in the point store";
  return "";
}

// n indices inside [0, N), distinct when asked: "" or what is wrong with the first faulty one
std::string index_error(int n, const int32_t* idx, int32_t N, const char* what, bool distinct) {
  if (n > 0 && !idx) return std::string(what) + " is NULL";
  std::vector<uint8_t> seen(distinct ? (size_t)N : 0, 0);
  for (int i = 0; i < n; i++) {
    if (idx[i] < 0 || idx[i] >= N) return std::string(what) + "[" + std::to_string(i) + "] is outside its keyframe";
    if (distinct) {
      if (seen[idx[i]]) return std::string(what) + "[" + std::to_string(i) + "] repeats an earlier entry";
      seen[idx[i]] = 1;
    }
  }
  return "";
}

}  // namespace

extern "C" {

int dsh_keyframe_set_view(dsh_mpdb* db, int32_t slot, const dsh_keyframe_view* view) {
  DSH_STORE_ENTER("dsh_keyframe_set_view");
  if (!view) return bad("view is NULL");
  if (slot < 0 || slot >= db->K) return bad("slot outside the store");
  const LmKf k = db->kf[slot];
  if (view->N != k.N) return bad("N (" + std::to_string(view->N) + ") is not the N of keyframe " + std::to_string(slot) + " in the store (" + std::to_string(k.N) + ")");
  if (k.N > 0 && !view->kp_px) return bad("kp_px is NULL");
  for (size_t i = 0; i < 2 * (size_t)k.N; i++)
    if (!std::isfinite(view->kp_px[i])) return bad("key point " + std::to_string(i / 2) + " is not finite");
  const float cam[4] = {view->fx, view->fy, view->cx, view->cy}, bounds[4] = {view->mnMinX, view->mnMaxX, view->mnMinY, view->mnMaxY};
  for (int i = 0; i < 4; i++)
    if (!std::isfinite(cam[i]) || !std::isfinite(bounds[i])) return bad("the camera or the image bounds are not finite");
  if (!(bounds[1] > bounds[0]) || !(bounds[3] > bounds[2])) return bad("the image bounds are empty");
  if (view->grid_cols < 1 || view->grid_rows < 1 || (long long)view->grid_cols * view->grid_rows > 8192) return bad("the image grid is outside 1 .. 8192 cells");
  const dsh_bbs& g = view->warp_grid;
  if (!std::isfinite(g.umin) || !std::isfinite(g.umax) || !std::isfinite(g.vmin) || !std::isfinite(g.vmax) || !bbs_grid_ok(&g)) return bad("bad warp grid");
  dsh_mpdb::SurfKf& sk = db->surf[slot];
  if (!sk.has_surface) return refuse(DSH_ERR_STATE, "keyframe " + std::to_string(slot) + " has no resident surface (dsh_keyframe_surface_init)");
  if (sk.has_view) return refuse(DSH_ERR_STATE, "keyframe " + std::to_string(slot) + " has a view already");
  DSH_STORE_GATE();
  UpBlock up;
  const size_t o_px = up.copy_of(view->kp_px, 8 * (size_t)k.N);
  if (const int rc = up.copy(c)) return rc;
  if (k.N > 0) HIPCHK(c, hipMemcpyAsync(db->d_view_px + 2 * (size_t)k.tab_off, up.dev<float>(o_px), 8 * (size_t)k.N, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  sk.has_view = 1;
  std::memcpy(sk.cam, cam, sizeof cam);
  std::memcpy(sk.bounds, bounds, sizeof bounds);
  sk.grid_cols = view->grid_cols; sk.grid_rows = view->grid_rows;
  sk.warp = g;
  return DSH_OK;
}

int dsh_keyframe_get_view(dsh_mpdb* db, int32_t slot, dsh_keyframe_view* view, float* kp_px) {
  DSH_STORE_ENTER("dsh_keyframe_get_view");
  if (!view) return bad("view is NULL");
  if (slot < 0 || slot >= db->K) return bad("slot outside the store");
  const dsh_mpdb::SurfKf& sk = db->surf[slot];
  if (!sk.has_view) return refuse(DSH_ERR_STATE, "keyframe " + std::to_string(slot) + " has no view (dsh_keyframe_set_view)");
  DSH_STORE_GATE();
  const LmKf k = db->kf[slot];
  if (kp_px && k.N > 0) {
    DownBlock down;
    down.copy_to(kp_px, 8 * (size_t)k.N);
    if (const int rc = down.at(c, db->d_view_px + 2 * (size_t)k.tab_off)) return rc;
    if (const int rc = down.receive(c)) return rc;
  }
  std::memset(view, 0, sizeof(*view));
  view->N = k.N;
  view->fx = sk.cam[0]; view->fy = sk.cam[1]; view->cx = sk.cam[2]; view->cy = sk.cam[3];
  view->mnMinX = sk.bounds[0]; view->mnMaxX = sk.bounds[1]; view->mnMinY = sk.bounds[2]; view->mnMaxY = sk.bounds[3];
  view->grid_cols = sk.grid_cols; view->grid_rows = sk.grid_rows;
  view->warp_grid = sk.warp;
  return DSH_OK;
}

int dsh_keyframe_warp_pair(dsh_mpdb* db, const dsh_warp_pair_input* in, dsh_warp_pair_result* out) {
  DSH_STORE_ENTER("dsh_keyframe_warp_pair");
  if (!in) return bad("in is NULL");
  if (!out) return bad("out is NULL");
  if (dsh_base(in->ctx) != c) return bad("in->ctx is not the context of the store");
  if (!same_context(c, in->kfdb)) return bad("the keyframe store is NULL, belongs to another context or was detached");
  if (!same_context(c, in->ddb)) return bad("the database is NULL, belongs to another context or was detached");
  dsh_kfdb* kfdb = in->kfdb;
  dsh_diffdb* ddb = in->ddb;
  DSH_CHECK(kfdb_error(db, kfdb));
  const int32_t slot = in->slot, anchor = in->anchor;
  if (slot < 0 || slot >= db->K || anchor < 0 || anchor >= db->K) return bad("slot or anchor outside the store");
  if (slot == anchor) return bad("anchor == slot: no point is anchored in the keyframe being added");
  const LmKf k1 = db->kf[anchor], k2 = db->kf[slot];
  if (k1.N > WP_MAX_KEYPOINTS || k2.N > WP_MAX_KEYPOINTS) return bad("a keyframe has more than 8192 key points");
  if (kfdb->kf[anchor].octave_over) return bad("keyframe " + std::to_string(anchor) + " has an octave >= levels in the keyframe store");
  const int P0 = in->n_pairs, Q = in->n_queries;
  if (P0 < 1 || Q < 0) return bad("n_pairs < 1 or n_queries < 0");
  DSH_CHECK(index_error(P0, in->pair_idx1, k1.N, "pair_idx1", false));
  DSH_CHECK(index_error(P0, in->pair_idx2, k2.N, "pair_idx2", true));
  DSH_CHECK(index_error(Q, in->query_idx1, k1.N, "query_idx1", true));
  if (in->max_iters < 0 || in->max_iters > 1000 || in->min_pairs < 1 || !(in->radius > 0.f) || !std::isfinite(in->radius) || in->th_low > 256 || !std::isfinite(in->lambda))
    return bad("max_iters outside 0 .. 1000, min_pairs < 1, a radius that is not positive and finite, th_low > 256 or a lambda that is not finite");
  const dsh_mpdb::SurfKf &s1 = db->surf[anchor], &s2 = db->surf[slot];
  if (s1.has_view && s1.warp.nptsu * s1.warp.nptsv > 256)
    return bad("more than 256 control points (the one-workgroup solve handles 2N <= 512 unknowns; the reference uses 13 x 15 = 195)");
  const long long cap_erased = (long long)db->obs.size() + Q;
  if (db->R + Q > INT32_MAX || cap_erased > INT32_MAX) return bad("store full");
  if (!s1.has_view || !s2.has_view)
    return refuse(DSH_ERR_STATE, "keyframe " + std::to_string(s1.has_view ? slot : anchor) + " has no view (dsh_keyframe_set_view)");
  if (!db->unindexed.empty()) return mpdb_unindexed_error(db, who__);
  DSH_STORE_GATE();

  const dsh_bbs bbs = s1.warp;
  const int Nc = bbs.nptsu * bbs.nptsv, n2 = 2 * Nc, cap = P0 + Q;
  const size_t P0z = (size_t)P0, Qz = (size_t)Q, capz = (size_t)cap, Ncz = (size_t)Nc;
  hipStream_t st = c->stream;
  // room for every record stage 4 and stage 7 can add, before anything is launched
  HIPCHK(c, mpdb_reserve_log(db, db->R + Q));
  if (ddb_reserve(ddb, ddb->count + cap) != 0) return refuse(DSH_ERR_HIP, "out of device memory while growing the database");

  // the one block up: the index lists, and the constant operands of the initialisation
  UpBlock up;
  const size_t o_i1 = up.copy_of(in->pair_idx1, 4 * P0z), o_i2 = up.copy_of(in->pair_idx2, 4 * P0z), o_q1 = up.copy_of(in->query_idx1, 4 * Qz),
               o_bend = up.take(8 * Ncz * Ncz), o_ones = up.take_exact(8 * Ncz);
  // the one block down; the erased list lies behind what every call fetches
  DownBlock down;
  const size_t d_hdr = down.take(sizeof(WpHdr)), d_x = down.take(8 * (size_t)n2), d_info = down.take(16), d_costs = down.take(16), d_qmatch = down.take(4 * Qz),
               d_qpoint = down.take(4 * Qz), d_pstate = down.take(P0z), d_qstate = down.take(Qz), d_qadded = down.take(Qz);
  down.copy_to(d_x, out->x, 8 * (size_t)n2);   // the kernels write all of these whether the caller wants them or not
  down.copy_to(d_pstate, out->pair_state, P0z);
  down.copy_to(d_qstate, out->query_state, Qz);
  down.copy_to(d_qmatch, out->query_match, 4 * Qz);
  down.copy_to(d_qpoint, out->query_point, 4 * Qz);
  down.copy_to(d_qadded, out->query_added, Qz);
  const size_t head = down.size;
  const size_t d_erased = down.take_exact(8 * (size_t)cap_erased);
  if (const int rc = up.stage(c)) return rc;
  dsh::bbs_bending_dense(&bbs, in->lambda, up.host<double>(o_bend));
  std::fill_n(up.host<double>(o_ones), Ncz, 1.0);
  if (const int rc = up.send(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  HIPCHK(c, hipMemsetAsync(down.d + d_info, 0, d_qmatch - d_info, st));   // info and costs of a call that ends at stage 5

  WpBufs b;
  std::memset(&b, 0, sizeof(b));
  b.P = db->P; b.slot = slot; b.anchor = anchor; b.tag = in->tag;
  b.n_pairs = P0; b.n_queries = Q;
  b.N1 = k1.N; b.N2 = k2.N; b.off1 = k1.tab_off; b.off2 = k2.tab_off;
  b.n_ctrl = n2; b.nan_limit = std::min(n2, 2 * bbs.nptsu * bbs.nptsu);
  b.R = db->R;
  b.bad = db->d_bad; b.ref_kf = db->d_ref_kf; b.nobs = db->d_nobs; b.log = db->d_log; b.log_idx = db->d_log_idx; b.kf = db->d_kf; b.table = db->d_table;
  b.kpn = db->d_surf_kpn;
  b.slots = kfdb->d_slots; b.rows = kfdb->d_rows; b.oct = kfdb->d_oct; b.sf = kfdb->d_sf;
  b.pair_idx1 = up.dev<const int32_t>(o_i1); b.pair_idx2 = up.dev<const int32_t>(o_i2); b.query_idx1 = up.dev<const int32_t>(o_q1);
  // LIFETIME: slices of the context's scratch, which only grows within a call; the stages below take further slices and never enter
  HIPCHK(c, dsh_scratch_array(c, &b.g_kp1, 2 * P0z)); HIPCHK(c, dsh_scratch_array(c, &b.g_kp2, 2 * P0z)); HIPCHK(c, dsh_scratch_array(c, &b.g_isg, P0z));
  HIPCHK(c, dsh_scratch_array(c, &b.q_kp1, 2 * Qz)); HIPCHK(c, dsh_scratch_array(c, &b.q_desc, 2 * Qz));
  HIPCHK(c, dsh_scratch_array(c, &b.has, (size_t)k2.N));
  HIPCHK(c, dsh_scratch_array(c, &b.k_idx1, capz)); HIPCHK(c, dsh_scratch_array(c, &b.k_idx2, capz)); HIPCHK(c, dsh_scratch_array(c, &b.k_src, capz));
  HIPCHK(c, dsh_scratch_array(c, &b.k_tag, capz)); HIPCHK(c, dsh_scratch_array(c, &b.k_pid, capz));
  HIPCHK(c, dsh_scratch_array(c, &b.k_kp1, 2 * capz)); HIPCHK(c, dsh_scratch_array(c, &b.k_kp2, 2 * capz)); HIPCHK(c, dsh_scratch_array(c, &b.k_isg, capz));
  HIPCHK(c, dsh_scratch_array(c, &b.e_p1, capz)); HIPCHK(c, dsh_scratch_array(c, &b.e_p2, capz)); HIPCHK(c, dsh_scratch_array(c, &b.e_alive, capz));
  const size_t Pz = (size_t)std::max(db->P, 1);
  HIPCHK(c, dsh_scratch_array(c, &b.rec_slot, Pz)); HIPCHK(c, dsh_scratch_array(c, &b.anc_idx, Pz)); HIPCHK(c, dsh_scratch_array(c, &b.cand, Pz));
  HIPCHK(c, dsh_scratch_array(c, &b.first, Pz)); HIPCHK(c, dsh_scratch_array(c, &b.mark, Pz));
  HIPCHK(c, dsh_scratch_array(c, &b.win2, (size_t)k2.N)); HIPCHK(c, dsh_scratch_array(c, &b.kill1, (size_t)k1.N));
  b.hdr = down.dev<WpHdr>(d_hdr);
  b.match = down.dev<int32_t>(d_qmatch); b.query_point = down.dev<int32_t>(d_qpoint);
  b.pair_state = down.dev<uint8_t>(d_pstate); b.query_state = down.dev<uint8_t>(d_qstate); b.query_added = down.dev<uint8_t>(d_qadded);
  b.out_erased = down.dev<int2>(d_erased);

  // ---- stage 1, stage 2
  HIPCHK(c, wp_gather_launch(b, st));
  dsh::WarpInitDevice wi{};
  wi.kp1 = b.g_kp1; wi.kp2 = b.g_kp2; wi.bend = up.dev<const double>(o_bend); wi.ones = up.dev<const double>(o_ones);
  if (const int rc = dsh::warp_init_stages(c, &bbs, P0, nullptr, nullptr, in->lambda, &wi, nullptr, nullptr)) return rc;
  b.x = wi.x; b.scal = wi.scal;
  HIPCHK(c, wp_fix_start_launch(b, st));
  // ---- stage 3: the residuals at x with (fx, fy) of the anchor in the slots and lambda 0, then the filter
  double* res = nullptr;
  HIPCHK(c, dsh_scratch_array(c, &res, 2 * P0z + 4 * Ncz));
  HIPCHK(c, nrsfm_swp_eval(bbs_par(&bbs, 2), P0, (double)s1.cam[0], (double)s1.cam[1], 0.0, b.g_kp1, b.g_kp2, b.g_isg, b.x, res, nullptr, 0, st));
  b.res = res;
  HIPCHK(c, wp_filter_launch(b, st));
  // ---- stage 4: the search against the new keyframe in place, then the registration
  if (Q > 0) {
    int32_t* cell = nullptr;
    HIPCHK(c, dsh_scratch_array(c, &cell, (size_t)k2.N));
    HIPCHK(c, nrsfm_match_search(bbs_par(&bbs, 2), b.x, Q, b.q_kp1, reinterpret_cast<const uint32_t*>(b.q_desc), s2.cam, s2.bounds, s2.grid_cols, s2.grid_rows, k2.N,
                                 db->d_view_px + 2 * (size_t)k2.tab_off, reinterpret_cast<const uint32_t*>(kfdb->d_rows + 2 * (size_t)kfdb->kf[slot].row_off), b.has,
                                 in->radius, in->th_low, cell, down.dev<int32_t>(d_qmatch), st));
    HIPCHK(c, wp_register_launch(b, st));
  }
  // ---- stage 5: the count
  HIPCHK(c, hipMemcpyAsync(down.h, down.d, sizeof(WpHdr), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  const int L = down.host<WpHdr>(d_hdr)->n_list;
  const bool fit = L >= in->min_pairs;
  const double* x_dev = b.x;
  if (fit) {
    // ---- stage 6: the fit on the kept arrays where they lie
    dsh_schwarp_problem q{};
    q.bbs = bbs; q.P = L; q.fx_slot = (double)s1.cam[1]; q.fy_slot = (double)s1.cam[0]; q.lambda = in->lambda; q.fx = s1.cam[0]; q.fy = s1.cam[1];
    q.max_iters = in->max_iters;
    dsh::SwpDevice sd{};
    sd.kp1 = b.k_kp1; sd.kp2 = b.k_kp2; sd.isg = b.k_isg; sd.x0 = b.x;
    uint8_t* drop = nullptr;
    HIPCHK(c, dsh_scratch_array(c, &sd.diff, 18 * (size_t)L));
    HIPCHK(c, dsh_scratch_array(c, &drop, (size_t)L));
    sd.drop = drop;
    if (const int rc = dsh::swp_fit_stages(c, 1, &q, nullptr, nullptr, &sd)) return rc;
    x_dev = sd.x;
    HIPCHK(c, hipMemcpyAsync(down.d + d_info, sd.info, 8, hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipMemcpyAsync(down.d + d_costs, sd.costs, 16, hipMemcpyDeviceToDevice, st));
    // ---- stage 7: the states, the drops, then the records of the STORED entries in list order
    b.drop = drop;
    HIPCHK(c, wp_resolve_launch(b, L, st));
    int32_t *keep = nullptr, *pos = nullptr;
    void* tmp = nullptr;
    HIPCHK(c, dsh_scratch_array(c, &keep, (size_t)L)); HIPCHK(c, dsh_scratch_array(c, &pos, (size_t)L));
    HIPCHK(c, c->scratch.take(ddb_scan_tmp_bytes(L), &tmp));
    HIPCHK(c, ddb_append(L, drop, sd.diff, b.k_pid, b.k_tag, b.k_idx2, keep, pos, tmp, ddb_scan_tmp_bytes(L), ddb->count, ddb->cap, ddb->rec, ddb->pid, ddb->tag,
                         ddb->idx2, st));
  }
  HIPCHK(c, hipMemcpyAsync(down.d + d_x, x_dev, 8 * (size_t)n2, hipMemcpyDeviceToDevice, st));
  // the head of the block comes down; the used part of the erased list follows when records were blanked
  if (const int rc = down.at(c, down.d)) return rc;   // (the stages in between may have grown the page-locked buffer)
  HIPCHK(c, hipMemcpyAsync(down.h, down.d, head, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  const WpHdr h = *down.host<WpHdr>(d_hdr);
  if (h.n_listed > 0) {
    HIPCHK(c, hipMemcpyAsync(down.h + d_erased, down.d + d_erased, 8 * (size_t)h.n_listed, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
  }

  // the host mirrors follow: the records stage 4 appended in query order, the records stage 7 blanked, the database's count
  const int32_t* qpoint = down.host<int32_t>(d_qpoint);
  const uint8_t* qadded = down.host<uint8_t>(d_qadded);
  long long r = db->R;
  for (int j = 0; j < Q; j++)
    if (qadded[j]) db->obs[mpdb_obs_key(qpoint[j], slot)] = r++;
  db->R += h.n_appended;
  const int2* erased = down.host<int2>(d_erased);
  for (int j = 0; j < h.n_listed; j++) db->obs.erase(mpdb_obs_key(erased[j].x, erased[j].y));
  if (fit) {
    ddb->count += h.n_stored;
    ddb->max_pid = std::max(ddb->max_pid, h.max_pid);
  }

  down.hand_out();
  out->init_ok = h.init_ok; out->fitted = fit ? 1 : 0;
  std::memcpy(out->info, down.host<int32_t>(d_info), sizeof out->info);   // fields of the result record, not arrays of the caller
  std::memcpy(out->costs, down.host<double>(d_costs), sizeof out->costs);
  out->first_record = db->R - h.n_appended;
  out->n_filtered = h.n_filtered; out->n_matched = h.n_matched; out->n_appended = h.n_appended; out->n_list = h.n_list;
  out->n_skipped = h.n_skipped; out->n_dropped = h.n_dropped; out->n_kept = h.n_kept; out->n_stored = h.n_stored;
  out->rounds = h.rounds;
  out->erase.n_found = h.n_found; out->erase.n_ref_moved = h.n_ref_moved; out->erase.n_set_bad = h.n_set_bad;
  out->erase.n_records = h.n_found + h.n_erased; out->erase.n_entries = h.n_erased;
  return DSH_OK;
}

}  // extern "C"
