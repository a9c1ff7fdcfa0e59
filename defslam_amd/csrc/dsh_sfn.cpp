// Host side of dsh_sfn_estimate / dsh_bbs_bending (include/defslam_hip.h): Shape from Normals,
// Modules/Mapping/ShapeFromNormals.cc.  The stacked least squares is solved on the device by corrected semi-normal
// equations: G = A^T A and A^T b on FP64 MFMA (swp_normal_kernel), tile Cholesky (swp_solve_kernel), two steps of
// iterative refinement with the residual formed from A itself, which restores the accuracy a QR factorisation has.
// Also dsh_warp_initialize and dsh_search_by_schwarp.  Every call moves one block up and one down (UpBlock / DownBlock, dsh_ctx.h) and
// takes its device-only work space as one Arena-laid scratch slice.
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
#include "schwarp_problem.h"

namespace {

// int_0^1 b_p^(k) b_q^(k) dt for the four cubic B-spline pieces on a knot interval, k = 0, 1, 2: the three coefficient
// tables of the reference's bending code are products of these numbers.
void spline_integrals(double I[3][4][4]) {
  const double piece[4][4] = {{1.0 / 6, -3.0 / 6, 3.0 / 6, -1.0 / 6}, {4.0 / 6, 0.0, -6.0 / 6, 3.0 / 6}, {1.0 / 6, 3.0 / 6, 3.0 / 6, -3.0 / 6}, {0.0, 0.0, 0.0, 1.0 / 6}};
  for (int k = 0; k < 3; k++)
    for (int p = 0; p < 4; p++)
      for (int q = 0; q < 4; q++) {
        double a[4], b[4];
        for (int t = 0; t < 4; t++) { a[t] = piece[p][t]; b[t] = piece[q][t]; }
        for (int s = 0; s < k; s++) {
          const double da[4] = {a[1], 2 * a[2], 3 * a[3], 0.0}, db[4] = {b[1], 2 * b[2], 3 * b[3], 0.0};
          std::memcpy(a, da, sizeof a);
          std::memcpy(b, db, sizeof b);
        }
        double s = 0.0;
        for (int i = 0; i < 4; i++)
          for (int j = 0; j < 4; j++) s += a[i] * b[j] / (double)(i + j + 1);
        I[k][p][q] = s;
      }
}

void bending_dense(const dsh_bbs* b, double lambda, double* Bm) {
  const int nx = b->nptsv, ny = b->nptsu, N = nx * ny;
  const double sy = (b->umax - b->umin) / (b->nptsu - 3), sx = (b->vmax - b->vmin) / (b->nptsv - 3);
  double I[3][4][4];
  spline_integrals(I);
  double coeff[16][16];
  for (int d = 0; d < 16; d++)
    for (int c = 0; c <= d; c++) {
      const int e1 = c / 4, f1 = c % 4, e2 = d / 4, f2 = d % 4;
      const double bxx = I[2][f1][f2] * I[0][e1][e2], byy = I[0][f1][f2] * I[2][e1][e2], bxy = 2.0 * I[1][f1][f2] * I[1][e1][e2];
      coeff[d][c] = sy * bxx / std::pow(sx, 3) + bxy / (sx * sy) + sx * byy / std::pow(sy, 3);
    }
  std::fill(Bm, Bm + (size_t)N * N, 0.0);
  for (int cb = 0; cb < ny - 3; cb++)        // knot cells, u index outer like the reference
    for (int ca = 0; ca < nx - 3; ca++)
      for (int c = 0; c < 16; c++)
        for (int d = c; d < 16; d++) {
          const int i = (cb + c / 4) * nx + ca + c % 4, j = (cb + d / 4) * nx + ca + d % 4;
          Bm[(size_t)i * N + j] += lambda * coeff[d][c];
          if (i != j) Bm[(size_t)j * N + i] = Bm[(size_t)i * N + j];
        }
}

}  // namespace

namespace dsh {
// dense N x N bending matrix of the grid (used by the batched Schwarp fit for its Warp::initialize stage, dsh_schwarp.cpp)
void bbs_bending_dense(const dsh_bbs* b, double lambda, double* Bm) { bending_dense(b, lambda, Bm); }

void sfn_fill_constant_rows(const dsh_bbs* bbs, int n, double bending_weight, double mean_depth, double* tail, double* b, double* ones) {
  const size_t N = (size_t)bbs->nptsu * bbs->nptsv, m = 2 * (size_t)n + N + 1;
  bending_dense(bbs, bending_weight, tail);
  std::fill_n(tail + N * N, N, 1.0);
  std::fill_n(b, m, 0.0);
  b[m - 1] = (double)N * mean_depth;
  std::fill_n(ones, N, 1.0);
}
}  // namespace dsh

extern "C" {

int dsh_bbs_bending(const dsh_bbs* bbs, double lambda, double* bending) {
  if (!bbs_grid_ok(bbs) || !bending) return DSH_ERR_ARG;
  bending_dense(bbs, lambda, bending);
  return DSH_OK;
}

}  // extern "C"

// The checks of dsh_sfn_estimate / dsh_sfn_estimate_db behind the device gate, then the stages.
static int sfn_estimate(dsh_ctx* ctx, const dsh_bbs* bbs, int n, const double* u, const double* v, const float* normals, const dsh_diffdb* ndb, const int32_t* sel,
                        double bending_weight, double mean_depth, int n_all, const double* u_all, const double* v_all, double* ctrl_raw, double* ctrl, float* pts,
                        int32_t* ok) {
  dsh_ctx_base* c = dsh_base(ctx);
  if (!c) return DSH_ERR_ARG;
  if (const int rc = dsh_enter(c, "dsh_sfn_estimate")) return rc;
  if (!bbs_grid_ok(bbs) || n < 0 || n_all < 0 || (n > 0 && (!u || !v || (!normals && !(ndb && sel)))) || (n_all > 0 && (!u_all || !v_all || !pts)) || !ctrl || !ok)
    return dsh_fail(c, DSH_ERR_ARG, "dsh_sfn_estimate: bad argument");
  if (ndb) {
    if (ndb->ctx != c) return dsh_fail(c, DSH_ERR_ARG, "dsh_sfn_estimate_db: the database belongs to another context");
    for (int i = 0; i < n; i++)
      if (sel[i] >= ndb->last_P || -1 - (long long)sel[i] >= ndb->last_R)
        return dsh_fail(c, DSH_ERR_ARG, "dsh_sfn_estimate_db: sel[" + std::to_string(i) + "] is outside the last normal solve of the database");
  }
  const int N = bbs->nptsu * bbs->nptsv;
  if (N > 512) return dsh_fail(c, DSH_ERR_ARG, "dsh_sfn_estimate: more than 512 control points (one-workgroup solve)");
  return dsh::sfn_stages(c, bbs, n, u, v, normals, ndb, sel, bending_weight, mean_depth, n_all, u_all, v_all, nullptr, ctrl_raw, ctrl, pts, ok);
}

// The body of dsh_sfn_estimate / dsh_sfn_estimate_db / dsh_keyframe_sfn: the normals come from the host (normals), are picked on the
// device out of the last normal solve of a database (ndb, sel), or lie on the device with the sites (dev).  Two pairs of blocks: the
// control points come down before the surface points are evaluated.
int dsh::sfn_stages(dsh_ctx_base* c, const dsh_bbs* bbs, int n, const double* u, const double* v, const float* normals, const dsh_diffdb* ndb, const int32_t* sel,
                    double bending_weight, double mean_depth, int n_all, const double* u_all, const double* v_all, const SfnDevice* dev, double* ctrl_raw,
                    double* ctrl, float* pts, int32_t* ok) {
  const int N = bbs->nptsu * bbs->nptsv;
  *ok = 0;
  hipStream_t st = c->stream;
  const int m = 2 * n + N + 1, np = nrsfm_swp_solve_np(N);
  const size_t nz = (size_t)n, Nz = (size_t)N, rows = 8 * 2 * nz * Nz;   // rows: bytes of the normal rows of A, which sfn_rows_kernel fills
  // the constant rows lead the block up and land right behind the normal rows: the device side of the block continues A
  UpBlock up;
  const size_t o_tail = up.take(8 * (Nz + 1) * Nz), o_b = up.take(8 * (size_t)m), o_ones = up.take(8 * Nz), o_u = up.copy_of(dev ? nullptr : u, 8 * nz),
               o_v = up.copy_of(dev ? nullptr : v, 8 * nz), o_n = dev ? up.take(0) : ndb ? up.copy_of(sel, 4 * nz) : up.copy_of(normals, 12 * nz);
  Arena ws;   // x and the scalars of the solve are neighbours: one memset, and the block down lies on them
  const size_t o_A = ws.take(rows + up.size), o_r = ws.take(8 * (size_t)m), o_ddx = ws.take(8 * Nz), o_G = ws.take(8 * Nz * Nz), o_g = ws.take(8 * Nz),
               o_M = ws.take(8 * (size_t)np * np), o_W = ws.take(8 * (size_t)np * 16), o_x = ws.take(8 * Nz), o_scal = ws.take(256), o_pick = ws.take(ndb ? 12 * nz : 0);
  char* w = nullptr;
  HIPCHK(c, c->scratch.take(ws.size, (void**)&w));
  auto f64 = [&](size_t off) { return reinterpret_cast<double*>(w + off); };
  up.d = w + o_A + rows;
  if (const int rc = up.stage(c)) return rc;
  dsh::sfn_fill_constant_rows(bbs, n, bending_weight, mean_depth, up.host<double>(o_tail), up.host<double>(o_b), up.host<double>(o_ones));
  if (const int rc = up.send(c)) return rc;
  HIPCHK(c, hipMemsetAsync(w + o_A, 0, rows, st));
  HIPCHK(c, hipMemsetAsync(w + o_x, 0, o_scal + 256 - o_x, st));
  const float* dn = dev ? dev->normals : up.dev<float>(o_n);
  const double *du = dev ? dev->u : up.dev<double>(o_u), *dv = dev ? dev->v : up.dev<double>(o_v);
  if (!dev && ndb && n > 0) {
    dn = reinterpret_cast<float*>(w + o_pick);
    HIPCHK(c, ddb_pick_normals(n, up.dev<int32_t>(o_n), ndb->last_normals, ndb->last_normals + 3 * (size_t)ndb->last_P, reinterpret_cast<float*>(w + o_pick), st));
  }
  double *dA = f64(o_A), *dx = f64(o_x), *db = up.dev<double>(o_b), *dones = up.dev<double>(o_ones);
  HIPCHK(c, nrsfm_sfn_rows(bbs_par(bbs, 1), n, du, dv, dn, dA, st));
  // x0: G x = A^T b  (the solve kernel returns M dx = -g, so it is fed g = A^T (-(b - A x)))
  for (int it = 0; it < 3; it++) {
    HIPCHK(c, nrsfm_sfn_residual(m, N, dA, dx, db, -1.0, f64(o_r), st));
    HIPCHK(c, nrsfm_swp_normal(m, N, dA, f64(o_r), dones, f64(o_G), f64(o_g), st));
    if (it == 0) HIPCHK(c, nrsfm_swp_solve(N, f64(o_G), f64(o_g), 1e300, f64(o_M), f64(o_W), f64(o_ddx), f64(o_scal) + 2, 0, N, st));   // dense: the mean-depth row couples every pair of control points
    else HIPCHK(c, nrsfm_swp_resolve(N, f64(o_g), f64(o_M), f64(o_W), f64(o_ddx), 0, N, st));
    HIPCHK(c, nrsfm_sfn_axpy(N, f64(o_ddx), dx, st));
  }
  DownBlock down;
  const size_t d_x = down.take(8 * Nz), d_s = down.take_exact(64);
  if (const int rc = down.at(c, dx)) return rc;
  if (const int rc = down.receive(c)) return rc;
  const double *x = down.host<double>(d_x), *s8 = down.host<double>(d_s);
  if (ctrl_raw) std::memcpy(ctrl_raw, x, 8 * Nz);
  const bool factor_ok = s8[2] != 0.0 || s8[3] != 0.0;   // out[0] also folds in "model > 0"; a positive-definite G always has it
  bool finite = true;
  for (int i = 0; i < N; i++) finite = finite && std::isfinite(x[i]);
  if (!factor_ok || !finite || n_all == 0) return DSH_OK;
  // the reference's scale: 1 / median of the float32 control points (ShapeFromNormals.cc:123-135)
  std::vector<float> dvec(Nz);
  for (int i = 0; i < N; i++) dvec[i] = (float)x[i];
  std::sort(dvec.begin(), dvec.end());
  const float corr = 1 / dvec[dvec.size() / 2];
  for (int i = 0; i < N; i++) ctrl[i] = corr * x[i];
  // second pair (x is not read past this point: the blocks reuse the page-locked buffers)
  const size_t na = (size_t)n_all;
  UpBlock up2;
  const size_t o_ctrl = up2.copy_of(ctrl, 8 * Nz), o_ua = up2.copy_of(dev ? nullptr : u_all, 8 * na), o_va = up2.copy_of(dev ? nullptr : v_all, 8 * na);
  DownBlock down2;
  const size_t d_pts = down2.copy_to(pts, 12 * na);
  if (const int rc = up2.copy(c)) return rc;
  if (dev) {
    // the surface points are evaluated into the place the caller keeps them in and come down from there; the control points follow
    if (const int rc = down2.at(c, dev->pts)) return rc;
    HIPCHK(c, nrsfm_sfn_points(bbs_par(bbs, 1), up2.dev<double>(o_ctrl), n_all, dev->u_all, dev->v_all, dev->pts, st));
    HIPCHK(c, hipMemcpyAsync(dev->ctrl, up2.dev<double>(o_ctrl), 8 * Nz, hipMemcpyDeviceToDevice, st));
  } else {
    if (const int rc = down2.alloc(c)) return rc;
    HIPCHK(c, nrsfm_sfn_points(bbs_par(bbs, 1), up2.dev<double>(o_ctrl), n_all, up2.dev<double>(o_ua), up2.dev<double>(o_va), down2.dev<float>(d_pts), st));
  }
  if (const int rc = down2.receive(c)) return rc;
  *ok = 1;
  return DSH_OK;
}

// The body of dsh_warp_initialize / the second stage of dsh_keyframe_warp_pair: the matches come from the host (kp1, kp2) or lie on the
// device with the constant operands (dev).
int dsh::warp_init_stages(dsh_ctx_base* c, const dsh_bbs* bbs, int P, const float* kp1, const float* kp2, double lambda, WarpInitDevice* dev, double* x, int32_t* ok) {
  const int N = bbs->nptsu * bbs->nptsv;
  if (!dev) *ok = 0;
  hipStream_t st = c->stream;
  const int np = nrsfm_swp_solve_np(N), kd = 3 * bbs->nptsv + 3;   // colocation and bending couple a 4 x 4 patch: banded
  const size_t Nz = (size_t)N, Pz = (size_t)P;
  UpBlock up;
  const size_t o_B = up.take(dev ? 0 : 8 * Nz * Nz), o_ones = up.take(dev ? 0 : 8 * Nz), o_k1 = up.copy_of(dev ? nullptr : kp1, 8 * Pz),
               o_k2 = up.copy_of(dev ? nullptr : kp2, 8 * Pz);
  Arena ws;   // x and the scalars of the solve are neighbours: the block down lies on them
  const size_t o_C = ws.take(8 * Pz * Nz), o_r0 = ws.take(8 * Pz), o_r1 = ws.take(8 * Pz), o_G = ws.take(8 * Nz * Nz), o_g0 = ws.take(8 * Nz), o_g1 = ws.take(8 * Nz),
               o_M = ws.take(8 * (size_t)np * np), o_W = ws.take(8 * (size_t)np * 16), o_x = ws.take(8 * 2 * Nz), o_scal = ws.take(256);
  char* w = nullptr;
  HIPCHK(c, c->scratch.take(ws.size, (void**)&w));
  auto f64 = [&](size_t off) { return reinterpret_cast<double*>(w + off); };
  if (!dev) {
    if (const int rc = up.stage(c)) return rc;
    bending_dense(bbs, lambda, up.host<double>(o_B));
    std::fill_n(up.host<double>(o_ones), Nz, 1.0);
    if (const int rc = up.send(c)) return rc;
  }
  const float *dk1 = dev ? dev->kp1 : up.dev<float>(o_k1), *dk2 = dev ? dev->kp2 : up.dev<float>(o_k2);
  const double *dB = dev ? dev->bend : up.dev<double>(o_B), *dones = dev ? dev->ones : up.dev<double>(o_ones);
  HIPCHK(c, hipMemsetAsync(w + o_C, 0, 8 * Pz * Nz, st));
  HIPCHK(c, hipMemsetAsync(w + o_scal, 0, 256, st));
  HIPCHK(c, nrsfm_warp_coloc(bbs_par(bbs, 1), P, dk1, dk2, f64(o_C), f64(o_r0), f64(o_r1), st));
  // g1 = C^T (-q2y) first (G is rebuilt by the second call), then G = C^T C, g0 = C^T (-q2x); G += Bending
  HIPCHK(c, nrsfm_swp_normal(P, N, f64(o_C), f64(o_r1), dones, f64(o_G), f64(o_g1), st));
  HIPCHK(c, nrsfm_swp_normal(P, N, f64(o_C), f64(o_r0), dones, f64(o_G), f64(o_g0), st));
  HIPCHK(c, nrsfm_mat_add(Nz * Nz, dB, f64(o_G), st));
  HIPCHK(c, nrsfm_swp_solve(N, f64(o_G), f64(o_g0), 1e300, f64(o_M), f64(o_W), f64(o_x), f64(o_scal) + 2, 0, kd, st));
  HIPCHK(c, nrsfm_swp_resolve(N, f64(o_g1), f64(o_M), f64(o_W), f64(o_x) + N, 0, kd, st));
  if (dev) {   // x and the scalars stay where they are
    dev->x = f64(o_x); dev->scal = f64(o_scal);
    return DSH_OK;
  }
  DownBlock down;
  down.copy_to(x, 8 * 2 * Nz);
  const size_t d_s = down.take_exact(64);
  if (const int rc = down.at(c, w + o_x)) return rc;
  if (const int rc = down.receive(c)) return rc;
  const double* s8 = down.host<double>(d_s);
  bool finite = true;
  for (int i = 0; i < 2 * N; i++) finite = finite && std::isfinite(x[i]);
  *ok = ((s8[2] != 0.0 || s8[3] != 0.0) && finite) ? 1 : 0;
  return DSH_OK;
}

extern "C" {

int dsh_sfn_estimate(dsh_ctx* ctx, const dsh_bbs* bbs, int n, const double* u, const double* v, const float* normals, double bending_weight,
                     double mean_depth, int n_all, const double* u_all, const double* v_all, double* ctrl_raw, double* ctrl, float* pts, int32_t* ok) {
  return sfn_estimate(ctx, bbs, n, u, v, normals, nullptr, nullptr, bending_weight, mean_depth, n_all, u_all, v_all, ctrl_raw, ctrl, pts, ok);
}

int dsh_sfn_estimate_db(dsh_ctx* ctx, const dsh_bbs* bbs, const dsh_diffdb* db, int n, const int32_t* sel, const double* u, const double* v, double bending_weight,
                        double mean_depth, int n_all, const double* u_all, const double* v_all, double* ctrl_raw, double* ctrl, float* pts, int32_t* ok) {
  dsh_ctx_base* c = dsh_base(ctx);
  if (!c) return DSH_ERR_ARG;
  if (!db || (n > 0 && !sel)) return dsh_fail(c, DSH_ERR_ARG, "dsh_sfn_estimate_db: bad argument");
  return sfn_estimate(ctx, bbs, n, u, v, nullptr, db, sel, bending_weight, mean_depth, n_all, u_all, v_all, ctrl_raw, ctrl, pts, ok);
}

int dsh_warp_initialize(dsh_ctx* ctx, const dsh_bbs* bbs, int P, const float* kp1, const float* kp2, double lambda, double* x, int32_t* ok) {
  dsh_ctx_base* c = dsh_base(ctx);
  if (!c) return DSH_ERR_ARG;
  if (const int rc = dsh_enter(c, "dsh_warp_initialize")) return rc;
  if (!bbs_grid_ok(bbs) || P <= 0 || !kp1 || !kp2 || !x || !ok) return dsh_fail(c, DSH_ERR_ARG, "dsh_warp_initialize: bad argument");
  const int N = bbs->nptsu * bbs->nptsv;
  if (N > 512) return dsh_fail(c, DSH_ERR_ARG, "dsh_warp_initialize: more than 512 control points (one-workgroup solve)");
  return dsh::warp_init_stages(c, bbs, P, kp1, kp2, lambda, nullptr, x, ok);
}

int dsh_search_by_schwarp(dsh_ctx* ctx, const dsh_bbs* bbs, const double* x, int Q, const float* kp1, const uint8_t* desc1, const float* cam2,
                          const float* bounds2, int grid_cols, int grid_rows, int N2, const float* kp2, const uint8_t* desc2, const uint8_t* has_mp2,
                          float radius, int th_low, int32_t* match, int32_t* nmatches) {
  dsh_ctx_base* c = dsh_base(ctx);
  if (!c) return DSH_ERR_ARG;
  if (const int rc = dsh_enter(c, "dsh_search_by_schwarp")) return rc;
  if (!bbs_grid_ok(bbs) || !x || Q < 0 || N2 < 0 || (Q > 0 && (!kp1 || !desc1 || !match)) || (N2 > 0 && (!kp2 || !desc2 || !has_mp2)) || !cam2 || !bounds2 ||
      grid_cols <= 0 || grid_rows <= 0 || grid_cols * grid_rows > 8192 || !(bounds2[1] > bounds2[0]) || !(bounds2[3] > bounds2[2]) || th_low > 256)
    return dsh_fail(c, DSH_ERR_ARG, "dsh_search_by_schwarp: bad argument");
  if (nmatches) *nmatches = 0;
  if (Q == 0) return DSH_OK;
  const size_t Nz = (size_t)bbs->nptsu * bbs->nptsv, Qz = (size_t)Q, N2z = (size_t)N2;
  UpBlock up;
  const size_t o_x = up.copy_of(x, 8 * 2 * Nz), o_k1 = up.copy_of(kp1, 8 * Qz), o_d1 = up.copy_of(desc1, 32 * Qz), o_k2 = up.copy_of(kp2, 8 * N2z),
               o_d2 = up.copy_of(desc2, 32 * N2z), o_mp = up.copy_of(has_mp2, N2z);
  DownBlock down;
  const size_t d_match = down.copy_to(match, 4 * Qz);
  int32_t* dcell = nullptr;
  HIPCHK(c, dsh_scratch_array(c, &dcell, N2z));
  if (const int rc = up.copy(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  HIPCHK(c, nrsfm_match_search(bbs_par(bbs, 2), up.dev<double>(o_x), Q, up.dev<float>(o_k1), up.dev<uint32_t>(o_d1), cam2, bounds2, grid_cols, grid_rows, N2,
                               up.dev<float>(o_k2), up.dev<uint32_t>(o_d2), up.dev<uint8_t>(o_mp), radius, th_low, dcell, down.dev<int32_t>(d_match), c->stream));
  if (const int rc = down.receive(c)) return rc;
  if (nmatches) {
    int n = 0;
    for (int q = 0; q < Q; q++) n += match[q] >= 0;
    *nmatches = n;
  }
  return DSH_OK;
}

}  // extern "C"
