// Host side of the resident Surface of a keyframe (include/defslam_hip.h: dsh_keyframe_surface_init, _set_depth, _set_points,
// _set_normals, _take_normals, _gather, _get, _vertices and dsh_keyframe_sfn): validation against the host mirror of dsh_mpdb, the
// launches of surfstore_kernels.hip and, for dsh_keyframe_sfn, the stages of dsh_sfn.cpp on the sites where the selection left them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "dsh_diffdb.h"
#include "dsh_sfn.h"
#include "mapping_launch.h"
#include "mpdb_store.h"
#include "surfstore_problem.h"

namespace {

SsStore surface_arrays(const dsh_mpdb* db) {
  SsStore s;
  s.normal = db->d_surf_normal; s.has = db->d_surf_has; s.pts = db->d_surf_pts; s.kpn = db->d_surf_kpn; s.n_normals = db->d_surf_nn;
  return s;
}

double* depth_of(const dsh_mpdb* db, int32_t slot) { return db->d_surf_depth + (size_t)dsh_mpdb::SURF_MAX_CTRL * slot; }

// keyframe `slot` and its resident Surface: "" or what is wrong
std::string surface_error(const dsh_mpdb* db, int32_t slot) {
  if (slot < 0 || slot >= db->K) return "slot outside the store";
  if (!db->surf[slot].has_surface) return "keyframe " + std::to_string(slot) + " has no resident surface (dsh_keyframe_surface_init)";
  return "";
}

// n targets (slot[j], idx[j]): "" or what is wrong with the first faulty one
std::string targets_error(const dsh_mpdb* db, int n, const int32_t* slot, const int32_t* idx) {
  if (n < 0) return "n < 0";
  if (n > 0 && (!slot || !idx)) return "slot or idx is NULL";
  for (int j = 0; j < n; j++) {
    const std::string se = surface_error(db, slot[j]);
    if (!se.empty()) return "target " + std::to_string(j) + ": " + se;
    if (idx[j] < 0 || idx[j] >= db->kf[slot[j]].N) return "target " + std::to_string(j) + ": idx outside the keyframe";
  }
  return "";
}

// The targets of a call in an upload block: entry and slot per target, and the span of entries they name.
struct Targets {
  size_t o_entry = 0, o_slot = 0;
  int32_t lo = 0, hi = -1;
  void layout(UpBlock& up, int n) { o_entry = up.take(4 * (size_t)n); o_slot = up.take(4 * (size_t)n); }
  void fill(const UpBlock& up, const dsh_mpdb* db, int n, const int32_t* slot, const int32_t* idx) {
    int32_t *e = up.host<int32_t>(o_entry), *s = up.host<int32_t>(o_slot);
    for (int j = 0; j < n; j++) {
      e[j] = db->kf[slot[j]].tab_off + idx[j];
      s[j] = slot[j];
      if (j == 0 || e[j] < lo) lo = e[j];
      if (j == 0 || e[j] > hi) hi = e[j];
    }
  }
  SsTargets dev(const UpBlock& up, int n) const {
    SsTargets t;
    t.n = n; t.entry = up.dev<const int32_t>(o_entry); t.slot = up.dev<const int32_t>(o_slot); t.base = lo; t.winner = nullptr;
    return t;
  }
};

// The two normal-writing calls behind their checks: the election, the write with the count, and the counts of the keyframes named down
// into the mirror.  src.normals / src.sel are offsets' pointers into `up`, which the caller has laid out and filled but not sent.
// COST: the election array spans the table entries between the smallest and the largest one named (4 bytes each, memset and scratch),
// and the counts come down for the slots between the smallest and the largest keyframe named.  A call of the mapping thread names one
// keyframe and its neighbours, whose tables lie together; a call that names the first and the last keyframe of a large map pays for the
// tables between them (at most 4 bytes per table entry of the store), never for more.
int write_normals(dsh_mpdb* db, UpBlock& up, const Targets& tg, int n, const int32_t* slot, SsNormalSource src, int32_t* n_normals_out) {
  dsh_ctx_base* c = db->ctx;
  if (n > 0) {
    if (const int rc = up.send(c)) return rc;
    SsTargets t = tg.dev(up, n);
    const size_t span = (size_t)(tg.hi - tg.lo) + 1;
    HIPCHK(c, dsh_scratch_array(c, &t.winner, span));
    HIPCHK(c, hipMemsetAsync(t.winner, 0xff, 4 * span, c->stream));   // -1: nobody yet
    HIPCHK(c, ss_elect_launch(t, c->stream));
    HIPCHK(c, ss_write_normals_launch(surface_arrays(db), t, src, c->stream));
    const int32_t k_lo = *std::min_element(slot, slot + n), k_hi = *std::max_element(slot, slot + n);
    DownBlock down;
    const size_t d_nn = down.take_exact(4 * (size_t)(k_hi - k_lo + 1));
    if (const int rc = down.at(c, db->d_surf_nn + k_lo)) return rc;
    if (const int rc = down.receive(c)) return rc;
    for (int32_t k = k_lo; k <= k_hi; k++)
      if (db->surf[k].has_surface) db->surf[k].n_normals = down.host<int32_t>(d_nn)[k - k_lo];
  }
  if (n_normals_out)
    for (int j = 0; j < n; j++) n_normals_out[j] = db->surf[slot[j]].n_normals;
  return DSH_OK;
}

}  // namespace

extern "C" {

int dsh_keyframe_surface_init(dsh_mpdb* db, int32_t slot, int32_t N, const float* kpn) {
  DSH_STORE_ENTER("dsh_keyframe_surface_init");
  if (slot < 0 || slot >= db->K) return bad("slot outside the store");
  const LmKf k = db->kf[slot];
  if (N != k.N) return bad("N (" + std::to_string(N) + ") is not the N of keyframe " + std::to_string(slot) + " in the store (" + std::to_string(k.N) + ")");
  if (N > 0 && !kpn) return bad("kpn is NULL");
  for (size_t i = 0; i < 2 * (size_t)N; i++)
    if (!std::isfinite(kpn[i])) return bad("key point " + std::to_string(i / 2) + " is not finite");
  if (db->surf[slot].has_surface) return refuse(DSH_ERR_STATE, "keyframe " + std::to_string(slot) + " has a resident surface already");
  DSH_STORE_GATE();
  // Surface(N): default SurfacePoints -- no normal, x3D zeros -- and numberofNormals_ = 0 (Surface.cc:31-37)
  const size_t n = (size_t)N, e = (size_t)k.tab_off;
  UpBlock up;
  const size_t o_kpn = up.copy_of(kpn, 8 * n);
  if (const int rc = up.copy(c)) return rc;
  if (N > 0) {
    HIPCHK(c, hipMemsetAsync(db->d_surf_normal + 3 * e, 0, 12 * n, c->stream));
    HIPCHK(c, hipMemsetAsync(db->d_surf_pts + 3 * e, 0, 12 * n, c->stream));
    HIPCHK(c, hipMemsetAsync(db->d_surf_has + e, 0, n, c->stream));
    HIPCHK(c, hipMemcpyAsync(db->d_surf_kpn + 2 * e, up.dev<float>(o_kpn), 8 * n, hipMemcpyDeviceToDevice, c->stream));
  }
  HIPCHK(c, hipMemsetAsync(db->d_surf_nn + slot, 0, 4, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  db->surf[slot] = dsh_mpdb::SurfKf{};
  db->surf[slot].has_surface = 1;
  return DSH_OK;
}

int dsh_keyframe_surface_set_depth(dsh_mpdb* db, int32_t slot, const dsh_bbs* bbs, const double* ctrl) {
  DSH_STORE_ENTER("dsh_keyframe_surface_set_depth");
  DSH_CHECK(surface_error(db, slot));
  if (!bbs_grid_ok(bbs)) return bad("bad B-spline");
  if ((long long)bbs->nptsu * bbs->nptsv > dsh_mpdb::SURF_MAX_CTRL) return bad("more than 512 control points");
  if (!ctrl) return bad("ctrl is NULL");
  DSH_STORE_GATE();
  const size_t Nz = (size_t)bbs->nptsu * bbs->nptsv;
  UpBlock up;
  const size_t o_ctrl = up.copy_of(ctrl, 8 * Nz);
  if (const int rc = up.copy(c)) return rc;
  HIPCHK(c, hipMemcpyAsync(depth_of(db, slot), up.dev<double>(o_ctrl), 8 * Nz, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  db->surf[slot].grid = *bbs;
  db->surf[slot].grid.valdim = 1;
  db->surf[slot].has_depth = 1;
  return DSH_OK;
}

int dsh_keyframe_surface_set_points(dsh_mpdb* db, int32_t slot, int32_t n, const int32_t* idx, const float* pts) {
  DSH_STORE_ENTER("dsh_keyframe_surface_set_points");
  DSH_CHECK(surface_error(db, slot));
  DSH_CHECK(mpdb_ids_error(n, idx, db->kf[slot].N, "idx"));
  if (n > 0 && !pts) return bad("pts is NULL");
  DSH_STORE_GATE();
  if (n == 0) return DSH_OK;
  UpBlock up;
  const size_t o_idx = up.copy_of(idx, 4 * (size_t)n), o_pts = up.copy_of(pts, 12 * (size_t)n);
  if (const int rc = up.copy(c)) return rc;
  HIPCHK(c, ss_set_points_launch(surface_arrays(db), db->kf[slot].tab_off, n, up.dev<const int32_t>(o_idx), up.dev<const float>(o_pts), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return DSH_OK;
}

int dsh_keyframe_surface_set_normals(dsh_mpdb* db, int32_t n, const int32_t* slot, const int32_t* idx, const float* normals, int32_t* n_normals_out) {
  DSH_STORE_ENTER("dsh_keyframe_surface_set_normals");
  DSH_CHECK(targets_error(db, n, slot, idx));
  if (n > 0 && !normals) return bad("normals is NULL");
  DSH_STORE_GATE();
  UpBlock up;
  Targets tg;
  tg.layout(up, n);
  const size_t o_n = up.copy_of(normals, 12 * (size_t)n);
  if (const int rc = up.stage(c)) return rc;
  tg.fill(up, db, n, slot, idx);
  if (const int rc = up.place(c)) return rc;
  SsNormalSource src;
  src.normals = up.dev<const float>(o_n); src.sel = nullptr; src.nref = src.nrec = nullptr;
  return write_normals(db, up, tg, n, slot, src, n_normals_out);
}

int dsh_keyframe_surface_take_normals(dsh_mpdb* db, const dsh_surface_take_input* in, int32_t* n_normals_out) {
  DSH_STORE_ENTER("dsh_keyframe_surface_take_normals");
  if (!in) return bad("in is NULL");
  const dsh_diffdb* ddb = in->ddb;
  const int32_t n = in->n, *sel = in->sel, *slot = in->slot, *idx = in->idx;
  DSH_CHECK(targets_error(db, n, slot, idx));
  if (!ddb) return bad("ddb is NULL");
  if (std::find(c->stores.begin(), c->stores.end(), static_cast<const dsh_store*>(ddb)) == c->stores.end())
    return bad("the database belongs to another context or was detached");
  if (n > 0 && !sel) return bad("sel is NULL");
  for (int j = 0; j < n; j++)
    if (sel[j] >= ddb->last_P || -1 - (long long)sel[j] >= ddb->last_R) return bad("sel[" + std::to_string(j) + "] is outside the last normal solve of the database");
  DSH_STORE_GATE();
  UpBlock up;
  Targets tg;
  tg.layout(up, n);
  const size_t o_sel = up.copy_of(sel, 4 * (size_t)n);
  if (const int rc = up.stage(c)) return rc;
  tg.fill(up, db, n, slot, idx);
  if (const int rc = up.place(c)) return rc;
  SsNormalSource src;
  src.normals = nullptr; src.sel = up.dev<const int32_t>(o_sel);
  src.nref = ddb->last_normals; src.nrec = ddb->last_normals + 3 * (size_t)ddb->last_P;
  return write_normals(db, up, tg, n, slot, src, n_normals_out);
}

int dsh_keyframe_surface_gather(dsh_mpdb* db, int32_t n, const int32_t* slot, const int32_t* idx, float* normal_xy, uint8_t* has, float* uv) {
  DSH_STORE_ENTER("dsh_keyframe_surface_gather");
  DSH_CHECK(targets_error(db, n, slot, idx));
  if (n > 0 && (!normal_xy || !has || !uv)) return bad("normal_xy, has or uv is NULL");
  DSH_STORE_GATE();
  if (n == 0) return DSH_OK;
  UpBlock up;
  Targets tg;
  tg.layout(up, n);
  DownBlock down;
  const size_t d_nxy = down.copy_to(normal_xy, 8 * (size_t)n), d_uv = down.copy_to(uv, 8 * (size_t)n), d_has = down.copy_to(has, (size_t)n);
  if (const int rc = up.stage(c)) return rc;
  tg.fill(up, db, n, slot, idx);
  if (const int rc = up.send(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  HIPCHK(c, ss_gather_launch(surface_arrays(db), tg.dev(up, n), down.dev<float>(d_nxy), down.dev<uint8_t>(d_has), down.dev<float>(d_uv), c->stream));
  return down.receive(c);
}

int dsh_keyframe_surface_get(dsh_mpdb* db, int32_t slot, int32_t capacity, float* normals, uint8_t* has_normal, float* pts, float* kpn, double* ctrl,
                             dsh_keyframe_surface_info* info) {
  DSH_STORE_ENTER("dsh_keyframe_surface_get");
  DSH_CHECK(surface_error(db, slot));
  const LmKf k = db->kf[slot];
  if (capacity < k.N) return bad("capacity is smaller than the keyframe's N");
  DSH_STORE_GATE();
  const dsh_mpdb::SurfKf& sk = db->surf[slot];
  const size_t n = (size_t)k.N, e = (size_t)k.tab_off, Nz = sk.has_depth ? (size_t)sk.grid.nptsu * sk.grid.nptsv : 0;
  // one block down through the page-locked buffer: the arrays asked for are gathered into it device to device
  DownBlock down;
  const size_t d_nrm = down.copy_to(normals, 12 * n), d_pts = down.copy_to(pts, 12 * n), d_kpn = down.copy_to(kpn, 8 * n), d_ctrl = down.copy_to(ctrl, 8 * Nz),
               d_has = down.copy_to(has_normal, n);
  if (const int rc = down.alloc(c)) return rc;
  auto gather = [&](void* dst, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream) : hipSuccess; };
  HIPCHK(c, gather(down.dev<char>(d_nrm), db->d_surf_normal + 3 * e, normals ? 12 * n : 0));
  HIPCHK(c, gather(down.dev<char>(d_pts), db->d_surf_pts + 3 * e, pts ? 12 * n : 0));
  HIPCHK(c, gather(down.dev<char>(d_kpn), db->d_surf_kpn + 2 * e, kpn ? 8 * n : 0));
  HIPCHK(c, gather(down.dev<char>(d_ctrl), depth_of(db, slot), ctrl ? 8 * Nz : 0));
  HIPCHK(c, gather(down.dev<char>(d_has), db->d_surf_has + e, has_normal ? n : 0));
  if (const int rc = down.receive(c)) return rc;
  if (info) {
    std::memset(info, 0, sizeof(*info));
    info->N = k.N;
    info->n_normals = sk.n_normals;
    info->enough_normals = sk.n_normals >= 10;   // normalsLimit_, Surface.cc:31-37 and :62-67
    info->has_depth = sk.has_depth;
    if (sk.has_depth) info->grid = sk.grid;
  }
  return DSH_OK;
}

int32_t dsh_keyframe_surface_state(const dsh_mpdb* db, int32_t slot) {
  if (!db || !db->ctx || slot < 0 || slot >= db->K) return -1;
  return db->surf[slot].has_surface ? (db->surf[slot].has_depth ? 2 : 1) : 0;
}

int dsh_keyframe_sfn(dsh_mpdb* db, const dsh_keyframe_sfn_input* in, double* ctrl_raw, double* ctrl, float* pts, dsh_keyframe_sfn_result* out) {
  DSH_STORE_ENTER("dsh_keyframe_sfn");
  if (!in) return bad("in is NULL");
  if (!out) return bad("out is NULL");
  if (dsh_base(in->ctx) != c) return bad("in->ctx is not the context of the store");
  DSH_CHECK(surface_error(db, in->slot));
  const LmKf k = db->kf[in->slot];
  if (k.N > SS_MAX_KEYPOINTS) return bad("the keyframe has more than 8192 key points");
  if (!bbs_grid_ok(in->bbs)) return bad("bad B-spline");
  const int Nc = in->bbs->nptsu * in->bbs->nptsv;
  if (Nc > dsh_mpdb::SURF_MAX_CTRL) return bad("more than 512 control points (one-workgroup solve)");
  DSH_STORE_GATE();

  // the selection: nothing goes up, the counts come down.  LIFETIME: the sites and the widened key points are slices of the context's
  // scratch, which only grows within a call and is reset by dsh_enter alone; the stages below take further slices and never enter.
  const size_t N = (size_t)k.N;
  SsSelect s;
  s.N = k.N; s.tab_off = k.tab_off; s.table = db->d_table;
  HIPCHK(c, dsh_scratch_array(c, &s.u, N));
  HIPCHK(c, dsh_scratch_array(c, &s.v, N));
  HIPCHK(c, dsh_scratch_array(c, &s.normals, 3 * N));
  HIPCHK(c, dsh_scratch_array(c, &s.u_all, N));
  HIPCHK(c, dsh_scratch_array(c, &s.v_all, N));
  DownBlock down;
  const size_t d_cnt = down.take_exact(sizeof(SsCounts));
  if (const int rc = down.alloc(c)) return rc;
  s.counts = down.dev<SsCounts>(d_cnt);
  HIPCHK(c, ss_select_launch(mpdb_state(db), surface_arrays(db), s, c->stream));
  if (const int rc = down.receive(c)) return rc;
  const SsCounts cnt = *down.host<SsCounts>(d_cnt);
  std::memset(out, 0, sizeof(*out));
  out->n_sites = cnt.n_sites; out->n_empty = cnt.n_empty; out->n_bad = cnt.n_bad; out->n_no_normal = cnt.n_no_normal; out->n_nan = cnt.n_nan;

  // Without a site the stacked system is the bending block and the row of ones: the affine depth maps are the null space of the
  // bending energy and one row pins one of their three dimensions, so the rank is N - 2 whatever the grid.  That is not ok, and no
  // factorisation is asked (in floating point it can pass on rounding).
  if (cnt.n_sites == 0) return DSH_OK;
  // ShapeFromNormals::estimate on the sites; when it succeeds the surface points are evaluated into the store and the scaled control
  // points become the keyframe's depth spline (set3DSurfacePoint and saveArray, ShapeFromNormals.cc:158-167)
  dsh::SfnDevice dev;
  dev.u = s.u; dev.v = s.v; dev.normals = s.normals; dev.u_all = s.u_all; dev.v_all = s.v_all;
  dev.pts = db->d_surf_pts + 3 * (size_t)k.tab_off;
  dev.ctrl = depth_of(db, in->slot);
  std::vector<double> own_ctrl;
  if (!ctrl) {
    own_ctrl.resize((size_t)Nc);
    ctrl = own_ctrl.data();
  }
  int32_t ok = 0;
  if (const int rc = dsh::sfn_stages(c, in->bbs, cnt.n_sites, nullptr, nullptr, nullptr, nullptr, nullptr, in->bending_weight, in->mean_depth, k.N, nullptr, nullptr,
                                     &dev, ctrl_raw, ctrl, pts, &ok))
    return rc;
  out->ok = ok;
  if (ok) {
    db->surf[in->slot].grid = *in->bbs;
    db->surf[in->slot].grid.valdim = 1;
    db->surf[in->slot].has_depth = 1;
  }
  return DSH_OK;
}

int dsh_keyframe_surface_vertices(dsh_mpdb* db, int32_t slot, const float* Twc, int32_t xs, int32_t ys, double* nodes_xyz) {
  DSH_STORE_ENTER("dsh_keyframe_surface_vertices");
  DSH_CHECK(surface_error(db, slot));
  if (!Twc || !nodes_xyz) return bad("Twc or nodes_xyz is NULL");
  if (xs < 2 || ys < 2) return bad("xs and ys must be at least 2");
  if ((long long)xs * ys > (1 << 24)) return bad("more than 2^24 vertices");
  if (!db->surf[slot].has_depth)
    return refuse(DSH_ERR_STATE, "keyframe " + std::to_string(slot) + " has no resident depth spline");
  DSH_STORE_GATE();
  dsh_surface_grid g;
  g.ctx = nullptr; g.bbs = &db->surf[slot].grid; g.depth_ctrl = nullptr; g.Twc = Twc; g.xs = xs; g.ys = ys;
  return dsh::surface_vertices_run(c, &g, depth_of(db, slot), nodes_xyz);
}

}  // extern "C"
