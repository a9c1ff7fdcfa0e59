// Host side of the template switch on the map point store (include/defslam_hip.h: dsh_surface_vertices, dsh_need_new_template,
// dsh_template_switch, dsh_point_store_get_points, dsh_point_store_get_embedding): validation against the host mirrors of dsh_mpdb and dsh_kfdb,
// per call one upload, the launches of tmplswitch_kernels.hip (and the store variant of the embedding in register_kernels.hip) and one
// download; after a switch the host mirror of the store follows what the device did.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "dsh_template.h"
#include "kfdb_store.h"
#include "mapping_launch.h"
#include "mpdb_store.h"
#include "tmplswitch_problem.h"

namespace {

// what is wrong with the keyframe's key points as the occupancy mask reads them, for keyframe `slot` of the store
std::string keypoints_error(const dsh_mpdb* db, int32_t slot, const dsh_kf_keypoints* kf) {
  if (!kf) return "kf is NULL";
  if (const char* ne = dsh_keypoint_count_error(kf->N)) return ne;
  if (kf->rows <= 0 || kf->cols <= 0) return "rows or cols <= 0";
  if (kf->cols < 40) return "cols < 40: the box kernel cols / 20 would be smaller than 2";
  const int k = kf->cols / 20;
  if (k >= kf->rows || k >= kf->cols) return "the box kernel cols / 20 does not fit into the image";
  if (kf->N > 0 && !kf->kp) return "kf->kp is NULL";
  for (int i = 0; i < kf->N; i++) {
    const float x = kf->kp[2 * (size_t)i], y = kf->kp[2 * (size_t)i + 1];
    // (int) truncates toward zero: (-1, 0) is pixel 0
    if (!(x > -1.0f && x < (float)kf->cols && y > -1.0f && y < (float)kf->rows) || (int)x >= kf->cols || (int)y >= kf->rows)
      return "key point " + std::to_string(i) + " lies outside the image";
  }
  if (slot < 0 || slot >= db->K) return "slot outside the store";
  if (kf->N != db->kf[slot].N) return "kf->N (" + std::to_string(kf->N) + ") is not the N of keyframe " + std::to_string(slot) + " in the store (" +
                                      std::to_string(db->kf[slot].N) + ")";
  return "";
}

void fill_keypoints(TsSwitch& k, const dsh_mpdb* db, int32_t slot, const dsh_kf_keypoints& kf) {
  std::memset(&k, 0, sizeof(k));
  k.rows = kf.rows; k.cols = kf.cols; k.N = kf.N; k.slot = slot;
  k.P = db->P; k.R = db->R; k.tab_off = db->kf[slot].tab_off;
  k.table = db->d_table;
}

}  // namespace

namespace dsh {
// The body of dsh_surface_vertices and dsh_keyframe_surface_vertices, after the checks and the device gate: ctrl_dev, when given, is the
// depth spline where it lies on the device and grid->depth_ctrl is not read (its slice of the block up stays empty).
int surface_vertices_run(dsh_ctx_base* c, const dsh_surface_grid* grid, const double* ctrl_dev, double* nodes_xyz) {
  const dsh_bbs* b = grid->bbs;
  const size_t n = (size_t)grid->xs * grid->ys, nctrl = (size_t)b->nptsu * b->nptsv;
  UpBlock up;
  const size_t o_T = up.copy_of(grid->Twc, 64), o_ctrl = up.copy_of(ctrl_dev ? nullptr : grid->depth_ctrl, 8 * nctrl), o_u = up.take(8 * n),
               o_v = up.take(8 * n);
  DownBlock down;
  const size_t d_xyz = down.copy_to(nodes_xyz, 24 * n);
  if (const int rc = up.stage(c)) return rc;
  double *u = up.host<double>(o_u), *v = up.host<double>(o_v);
  const unsigned int xs = (unsigned)grid->xs, ys = (unsigned)grid->ys;
  const double t = 0.03;
  size_t us = 0;
  for (unsigned int x = 0; x < xs; x++)
    for (unsigned int j = 0; j < ys; j++, us++) {   // Surface.cc:136-146
      u[us] = double((b->umax - b->umin - 2 * t) * x) / (xs - 1) + (b->umin + t);
      v[us] = double((b->vmax - b->vmin - 2 * t) * j) / (ys - 1) + (b->vmin + t);
    }
  if (const int rc = up.send(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  double* d_val = nullptr;
  HIPCHK(c, dsh_scratch_array(c, &d_val, n));
  HIPCHK(c, nrsfm_launch_bbs_eval(bbs_par(b, 1), ctrl_dev ? ctrl_dev : up.dev<const double>(o_ctrl), up.dev<const double>(o_u),
                                  up.dev<const double>(o_v), (int)n, 0, 0, d_val, nullptr, c->stream));
  HIPCHK(c, ts_vertices_launch(up.dev<const double>(o_u), up.dev<const double>(o_v), d_val, up.dev<const float>(o_T), (int)n, down.dev<double>(d_xyz),
                               c->stream));
  return down.receive(c);
}
}  // namespace dsh

extern "C" {

int dsh_surface_vertices(const dsh_surface_grid* grid, double* nodes_xyz) {
  if (!grid) return DSH_ERR_ARG;
  dsh_ctx_base* c = dsh_base(grid->ctx);
  if (!c) return DSH_ERR_ARG;
  auto bad = [&](const std::string& m) { return dsh_fail(c, DSH_ERR_ARG, "dsh_surface_vertices: " + m); };
  const dsh_bbs* b = grid->bbs;
  if (!bbs_grid_ok(b)) return bad("bad B-spline");
  if (b->valdim != 1) return bad("the depth spline has valdim 1");
  if (!grid->depth_ctrl || !grid->Twc || !nodes_xyz) return bad("depth_ctrl, Twc or nodes_xyz is NULL");
  if (grid->xs < 2 || grid->ys < 2) return bad("xs and ys must be at least 2");
  if ((long long)grid->xs * grid->ys > (1 << 24)) return bad("more than 2^24 vertices");
  if (const int rc = dsh_enter(c, "dsh_surface_vertices")) return rc;
  return dsh::surface_vertices_run(c, grid, nullptr, nodes_xyz);
}

int dsh_need_new_template(dsh_mpdb* db, int32_t slot, const dsh_kf_keypoints* kf, int32_t* n_candidates, uint8_t* candidate) {
  DSH_STORE_ENTER("dsh_need_new_template");
  DSH_CHECK(keypoints_error(db, slot, kf));
  if (!n_candidates) return bad("n_candidates is NULL");
  DSH_STORE_GATE();
  *n_candidates = 0;
  const size_t N = (size_t)kf->N;
  if (N == 0) return DSH_OK;
  UpBlock up;
  const size_t o_cnt = up.take(sizeof(TsCounts)), o_kp = up.copy_of(kf->kp, 8 * N);
  DownBlock down;
  const size_t d_cnt = down.take(sizeof(TsCounts)), d_cand = down.take_exact(N);
  down.copy_to(d_cand, candidate, N);   // the kernel writes the flags whether the caller wants them or not
  if (const int rc = up.stage(c)) return rc;
  std::memset(up.host<TsCounts>(o_cnt), 0, sizeof(TsCounts));   // the counters go up as zeros
  if (const int rc = up.send(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  TsSwitch k;
  fill_keypoints(k, db, slot, *kf);
  k.kp = up.dev<const float>(o_kp);
  k.counts = down.dev<TsCounts>(d_cnt);
  k.candidate = down.dev<uint8_t>(d_cand);
  HIPCHK(c, dsh_scratch_array(c, &k.cls, N));
  HIPCHK(c, dsh_scratch_array(c, &k.block_new, (N + TS_BLOCK - 1) / TS_BLOCK));
  HIPCHK(c, hipMemcpyAsync(k.counts, up.dev<const TsCounts>(o_cnt), sizeof(TsCounts), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, ts_classify_launch(mpdb_state(db), k, c->stream));
  if (const int rc = down.receive(c)) return rc;
  *n_candidates = down.host<TsCounts>(d_cnt)->c.n_new;
  return DSH_OK;
}

int dsh_template_switch(dsh_mpdb* db, const dsh_template_switch_input* in, int32_t* new_idx, dsh_template_switch_counts* out) {
  DSH_STORE_ENTER("dsh_template_switch");
  if (!in) return bad("in is NULL");
  DSH_CHECK(keypoints_error(db, in->slot, in->kf));
  const dsh_kf_keypoints& kf = *in->kf;
  const dsh_kfdb* kfdb = in->kfdb;
  if (!kfdb) return bad("kfdb is NULL");
  if (kfdb->ctx != c) return bad("the keyframe store belongs to another context or was detached");
  if (in->slot >= kfdb->count) return bad("slot outside the keyframe store");
  const dsh_kfdb::Kf& hk = kfdb->kf[in->slot];
  if (hk.N != kf.N) return bad("kf->N is not the N of keyframe " + std::to_string(in->slot) + " in the keyframe store");
  for (int i = 0; i < kf.N; i++)
    if (hk.octave[i] >= hk.levels) return bad("key point " + std::to_string(i) + " has an octave >= levels in the keyframe store");
  // a NULL surface_pts names the keyframe's resident surface points (dsh_keyframe_surface_init); without them it is the refusal it was
  const bool resident = !in->surface_pts && db->surf[in->slot].has_surface;
  if (!in->Twc || (kf.N > 0 && !in->surface_pts && !resident)) return bad("Twc or surface_pts is NULL");
  if (!out) return bad("out is NULL");
  if ((long long)db->P + kf.N > INT32_MAX) return bad("store full");
  const dsh::TemplateHost* t = dsh_facet_template(c);
  if (!t) return refuse(DSH_ERR_STATE, "needs a template built from facets");
  DSH_STORE_GATE();

  // room for a new point per key point: how many are empty is known on the device only
  const size_t N = (size_t)kf.N;
  HIPCHK(c, mpdb_reserve_points(db, (long long)db->P + kf.N));
  HIPCHK(c, mpdb_reserve_log(db, db->R + kf.N));

  // up: the counts (zero), Twc, the key points, the surface points, the octaves and scale factors, the template
  UpBlock up;
  const size_t o_cnt = up.take(sizeof(TsCounts)), o_T = up.copy_of(in->Twc, 64), o_kp = up.copy_of(kf.kp, 8 * N),
               o_surf = up.copy_of(resident ? nullptr : in->surface_pts, 12 * N), o_oct = up.copy_of(hk.octave.data(), N),
               o_sf = up.copy_of(hk.sf, 4 * MPU_MAX_LEVELS), o_xyz0 = up.copy_of(t->xyz0.data(), 24 * (size_t)t->n),
               o_fac = up.copy_of(t->facets.data(), 12 * (size_t)t->F), o_nfp = up.copy_of(t->nf_ptr.data(), 4 * (size_t)(t->n + 1)),
               o_nfi = up.copy_of(t->nf_idx.data(), 4 * t->nf_idx.size());
  DownBlock down;   // the counts start as a copy of the uploaded zeros
  const size_t d_cnt = down.take(sizeof(TsCounts)), d_idx = down.take_exact(4 * N);
  if (const int rc = up.stage(c)) return rc;
  TsCounts* hc = up.host<TsCounts>(o_cnt);   // the counters go up as zeros, the largest node as none
  std::memset(hc, 0, sizeof(TsCounts));
  hc->max_node = -1;
  if (const int rc = up.send(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  hipStream_t st = c->stream;
  TsSwitch k;
  fill_keypoints(k, db, in->slot, kf);
  k.kp = up.dev<const float>(o_kp);
  k.surface = resident ? db->d_surf_pts + 3 * (size_t)db->kf[in->slot].tab_off : up.dev<const float>(o_surf);
  k.Twc = up.dev<const float>(o_T);
  k.octave = up.dev<const int8_t>(o_oct);
  k.sf = up.dev<const float>(o_sf);
  k.levels = hk.levels;
  k.kf_slots = kfdb->d_slots; k.kf_rows = kfdb->d_rows;
  k.log = db->d_log; k.log_idx = db->d_log_idx; k.ref_kf = db->d_ref_kf; k.normal = db->d_nrm; k.max_distance = db->d_maxd; k.desc = db->d_desc;
  k.counts = down.dev<TsCounts>(d_cnt);
  k.new_idx = down.dev<int32_t>(d_idx);
  HIPCHK(c, dsh_scratch_array(c, &k.cls, N));
  HIPCHK(c, dsh_scratch_array(c, &k.block_new, (N + TS_BLOCK - 1) / TS_BLOCK));
  HIPCHK(c, hipMemcpyAsync(k.counts, up.dev<const TsCounts>(o_cnt), sizeof(TsCounts), hipMemcpyDeviceToDevice, st));
  TsTemplate tt;
  tt.n = t->n;
  tt.xyz0 = up.dev<const double>(o_xyz0);
  tt.facets = up.dev<const int32_t>(o_fac);
  tt.nf_ptr = up.dev<const int32_t>(o_nfp);
  tt.nf_idx = up.dev<const int32_t>(o_nfi);
  const TcState s = mpdb_state(db);
  HIPCHK(c, ts_classify_launch(s, k, st));
  HIPCHK(c, ts_create_launch(s, k, st));
  HIPCHK(c, reg_embed_store(s, db->P, kf.N, tt, k.counts, st));
  if (const int rc = down.fetch(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(st));

  // the host mirror follows: the new points, their observation records, the facets
  const TsCounts& r = *down.host<TsCounts>(d_cnt);
  const int32_t n_new = r.c.n_new, first = db->P;
  for (int j = 0; j < n_new; j++) db->obs[mpdb_obs_key(first + j, in->slot)] = db->R + j;
  db->R += n_new;
  db->P += n_new;
  db->top_node.assign((size_t)db->P, -1);
  db->top_on_device = true;
  db->max_node = r.max_node;
  db->max_node_stale = false;
  *out = r.c;
  out->first_id = first;
  out->n_points = db->P;
  if (new_idx && n_new > 0) std::memcpy(new_idx, down.host<int32_t>(d_idx), 4 * (size_t)n_new);   // its length came down with it
  return DSH_OK;
}

int dsh_point_store_get_points(dsh_mpdb* db, int n, const int32_t* ids, float* xyz, float* normal, float* max_distance, uint8_t* desc, uint8_t* bad_flags) {
  DSH_STORE_ENTER("dsh_point_store_get_points");
  DSH_CHECK(mpdb_ids_error(n, ids, db->P, "point id"));
  DSH_STORE_GATE();
  if (n == 0) return DSH_OK;
  UpBlock up;
  const size_t m = (size_t)n, o_ids = up.copy_of(ids, 4 * m);
  DownBlock down;
  const size_t d_xyz = down.copy_to(xyz, 12 * m), d_nrm = down.copy_to(normal, 12 * m), d_maxd = down.copy_to(max_distance, 4 * m),
               d_desc = down.copy_to(desc, 32 * m), d_bad = down.copy_to(bad_flags, m);
  if (const int rc = up.copy(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  HIPCHK(c, ts_get_points_launch(mpdb_state(db), db->d_nrm, db->d_maxd, db->d_desc, up.dev<const int32_t>(o_ids), n, down.dev_if<float>(xyz, d_xyz),
                                 down.dev_if<float>(normal, d_nrm), down.dev_if<float>(max_distance, d_maxd), down.dev_if<uint4>(desc, d_desc),
                                 down.dev_if<uint8_t>(bad_flags, d_bad), c->stream));
  return down.receive(c);
}

int dsh_point_store_get_embedding(dsh_mpdb* db, int n, const int32_t* ids, int32_t* nodes, double* bary) {
  DSH_STORE_ENTER("dsh_point_store_get_embedding");
  DSH_CHECK(mpdb_ids_error(n, ids, db->P, "point id"));
  DSH_STORE_GATE();
  if (n == 0) return DSH_OK;
  UpBlock up;
  const size_t m = (size_t)n, o_ids = up.copy_of(ids, 4 * m);
  DownBlock down;
  const size_t d_nodes = down.copy_to(nodes, 12 * m), d_bary = down.copy_to(bary, 24 * m);
  if (const int rc = up.copy(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  HIPCHK(c, ts_get_embedding_launch(mpdb_state(db), up.dev<const int32_t>(o_ids), n, down.dev_if<int32_t>(nodes, d_nodes), down.dev_if<double>(bary, d_bary),
                                    c->stream));
  return down.receive(c);
}

}  // extern "C"
