// Host side of dsh_scale_min_median / dsh_optimize_horn / dsh_surface_register (include/defslam_hip.h):
// SurfaceRegistration::registerSurfaces (Modules/Mapping/SurfaceRegistration.cc:48-153) with its two numeric callees.
// The host only walks the caller's random stream (which points are candidates) and composes the 4x4 result; the
// residual lists, the medians, the Levenberg-Marquardt loop and its sums run in register_kernels.hip.  Each stage moves one block up and
// one down (UpBlock / DownBlock, dsh_ctx.h); a registration sends its two clouds once, with the first stage.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "dsh_register.h"
#include "mapping_launch.h"

namespace dsh {
// declared in dsh_ctx.h: one pass with null lists counts, a second one fills the slices of the block
int smm_walk_candidates(int n, const double* u, int64_t nu, int32_t* cand, int64_t* off, int64_t* consumed) {
  int64_t k = 0;
  int nc = 0;
  for (int i = 0; i < n; i++) {
    if (k >= nu) return -1;
    const double r_i = u[k++];
    if (r_i > 0.25) continue;
    if (k + (n - 1) > nu) return -1;
    if (cand) { cand[nc] = i; off[nc] = k; }
    nc++;
    k += n - 1;
  }
  *consumed = k;
  return nc;
}

// The stages, declared in dsh_register.h.
// scaleMinMedian: the clouds (unless d holds them already), the consumed part of the stream and the candidate list go up in one block,
// which stays in d for a second stage; the scale and the status (0, 1, 2) are read back
int scale_min_median_dev(dsh_ctx_base* c, int n, const float* mono, const float* stereo, const double* u, int64_t nu, float* scale, int64_t* consumed,
                         int32_t* status, Clouds& d) {
  int64_t k = 0;
  const int nc = dsh::smm_walk_candidates(n, u, nu, nullptr, nullptr, &k);
  if (nc < 0) {
    *status = 1;
    *scale = 0.f;
    return dsh_fail(c, DSH_ERR_ARG, "dsh_scale_min_median: the uniform stream is shorter than the draws the reference makes");
  }
  if (consumed) *consumed = k;
  UpBlock up;
  const size_t o_a = up.copy_of(mono, 12 * (size_t)n), o_b = up.copy_of(stereo, 12 * (size_t)n), o_u = up.copy_of(u, 8 * (size_t)k), o_c = up.take(4 * (size_t)nc),
               o_off = up.take(8 * (size_t)nc);
  DownBlock down;
  const size_t d_out = down.take_exact(64);
  float* dmed = nullptr;
  double* dsc = nullptr;
  HIPCHK(c, dsh_scratch_array(c, &dmed, (size_t)nc + 1));
  HIPCHK(c, dsh_scratch_array(c, &dsc, (size_t)nc + 1));
  if (const int rc = up.stage(c)) return rc;
  dsh::smm_walk_candidates(n, u, nu, up.host<int32_t>(o_c), up.host<int64_t>(o_off), &k);
  if (const int rc = up.send(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  if (mono) d = {up.dev<float>(o_a), up.dev<float>(o_b)};
  HIPCHK(c, reg_scale_min_median(n, nc, d.a, d.b, up.dev<double>(o_u), up.dev<int32_t>(o_c), up.dev<int64_t>(o_off), dmed, dsc, down.dev<double>(d_out), c->stream));
  if (const int rc = down.receive(c)) return rc;
  *scale = (float)down.host<double>(d_out)[0];
  *status = (int32_t)down.host<double>(d_out)[1];
  return DSH_OK;
}

// OptimizeHorn on the clouds in d, or on h1 / h2 when they are not on the device yet: then they go up with the start value
int optimize_horn_dev(dsh_ctx_base* c, int n, Clouds d, const float* h1, const float* h2, double* sim3, double chi, double huber, int32_t* acceptable, double* info) {
  UpBlock up;
  const size_t o_s = up.copy_of(sim3, 64), o_1 = up.copy_of(h1, 12 * (size_t)n), o_2 = up.copy_of(h2, 12 * (size_t)n);
  DownBlock down;
  const size_t d_out = down.take_exact(128);
  double* derr = nullptr;
  HIPCHK(c, dsh_scratch_array(c, &derr, 3 * (size_t)n));
  if (const int rc = up.copy(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  if (h1) d = {up.dev<float>(o_1), up.dev<float>(o_2)};
  const float delta_huber = (float)std::sqrt(huber);   // DefOptimizer.cc:869
  HIPCHK(c, reg_horn(n, d.a, d.b, up.dev<double>(o_s), chi, (double)delta_huber, derr, down.dev<double>(d_out), c->stream));
  if (const int rc = down.receive(c)) return rc;
  const double* out = down.host<double>(d_out);
  std::memcpy(sim3, out, 64);
  *acceptable = out[14] != 0.0 ? 1 : 0;
  if (info) std::memcpy(info, out + 8, 6 * sizeof(double));
  return DSH_OK;
}

// SurfaceRegistration.cc:132-150: mScw = [s R | t] as float32, Twc' = mScw * Twc, scale from the first row of the rotation
// block, new Tcw = inverse of the unscaled pose
void compose(const double* sim3, const float* Twc, double* s22_out, float* Tcw) {
  const double x = sim3[0], y = sim3[1], z = sim3[2], w = sim3[3], s = sim3[7];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  const double R[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
  float S[16], T[16];
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) S[4 * i + j] = (float)(s * R[3 * i + j]);
    S[4 * i + 3] = (float)sim3[4 + i];
  }
  S[12] = S[13] = S[14] = 0.f;
  S[15] = 1.f;
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      float acc = 0.f;
      for (int k = 0; k < 4; k++) acc += S[4 * i + k] * Twc[4 * k + j];
      T[4 * i + j] = acc;
    }
  float tt = 0.f;
  for (int k = 0; k < 3; k++) tt += T[k] * T[k];
  const double s22 = std::sqrt((double)tt);
  *s22_out = s22;
  float m[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) m[3 * i + j] = T[4 * i + j] / (float)s22;
  const float c00 = m[4] * m[8] - m[5] * m[7], c01 = m[3] * m[8] - m[5] * m[6], c02 = m[3] * m[7] - m[4] * m[6];
  const float det = m[0] * c00 - m[1] * c01 + m[2] * c02;
  const float inv[9] = {c00 / det, (m[2] * m[7] - m[1] * m[8]) / det, (m[1] * m[5] - m[2] * m[4]) / det,
                        (m[5] * m[6] - m[3] * m[8]) / det, (m[0] * m[8] - m[2] * m[6]) / det, (m[2] * m[3] - m[0] * m[5]) / det,
                        c02 / det, (m[1] * m[6] - m[0] * m[7]) / det, (m[0] * m[4] - m[1] * m[3]) / det};
  for (int r = 0; r < 3; r++) {
    for (int cc = 0; cc < 3; cc++) Tcw[4 * r + cc] = inv[3 * r + cc];
    Tcw[4 * r + 3] = -(inv[3 * r] * T[3] + inv[3 * r + 1] * T[7] + inv[3 * r + 2] * T[11]);
  }
  Tcw[12] = Tcw[13] = Tcw[14] = 0.f;
  Tcw[15] = 1.f;
}
}  // namespace dsh

using namespace dsh;

extern "C" {

int dsh_scale_min_median(dsh_ctx* ctx, int n, const float* pos_mono, const float* pos_stereo, const double* u, int64_t nu, float* scale,
                         int64_t* consumed, int32_t* status) {
  dsh_ctx_base* c = dsh_base(ctx);
  if (!c) return DSH_ERR_ARG;
  if (n <= 0 || n > kMaxPairs || !pos_mono || !pos_stereo || nu < 0 || (nu > 0 && !u) || !scale || !status)
    return dsh_fail(c, DSH_ERR_ARG, "dsh_scale_min_median: bad argument (1 <= n <= 8000)");
  int rc = dsh_enter(c, "dsh_scale_min_median");
  if (rc != DSH_OK) return rc;
  Clouds d;
  return scale_min_median_dev(c, n, pos_mono, pos_stereo, u, nu, scale, consumed, status, d);
}

int dsh_optimize_horn(dsh_ctx* ctx, int n, const float* pts1, const float* pts2, double* sim3, double chi, double huber, int32_t* acceptable,
                      double* info) {
  dsh_ctx_base* c = dsh_base(ctx);
  if (!c) return DSH_ERR_ARG;
  if (n <= 0 || !pts1 || !pts2 || !sim3 || !acceptable || !(huber >= 0.0)) return dsh_fail(c, DSH_ERR_ARG, "dsh_optimize_horn: bad argument");
  int rc = dsh_enter(c, "dsh_optimize_horn");
  if (rc != DSH_OK) return rc;
  return optimize_horn_dev(c, n, Clouds{}, pts1, pts2, sim3, chi, huber, acceptable, info);
}

int dsh_surface_register(dsh_ctx* ctx, int n, const float* cloud_surface, const float* cloud_map, const double* u, int64_t nu, const float* Twc,
                         double chi_limit, int check_chi, int32_t* registered, double* sim3, double* s22, float* Tcw_new, double* info) {
  dsh_ctx_base* c = dsh_base(ctx);
  if (!c) return DSH_ERR_ARG;
  if (n < 0 || n > kMaxPairs || (n > 0 && (!cloud_surface || !cloud_map)) || nu < 0 || (nu > 0 && !u) || !Twc || !registered || !sim3 || !s22 || !Tcw_new)
    return dsh_fail(c, DSH_ERR_ARG, "dsh_surface_register: bad argument (n <= 8000)");
  *registered = 0;
  if (info) std::memset(info, 0, 8 * sizeof(double));
  if (n < 15) return DSH_OK;   // SurfaceRegistration.cc:108-109
  int rc = dsh_enter(c, "dsh_surface_register");
  if (rc != DSH_OK) return rc;
  Clouds d;   // the two clouds go up once, with the first stage
  float scale = 0.f;
  int32_t status = 0;
  rc = scale_min_median_dev(c, n, cloud_surface, cloud_map, u, nu, &scale, nullptr, &status, d);
  if (rc != DSH_OK) return rc;
  // g2o::Sim3(identity rotation, zero translation, scale): Quaterniond(Matrix3d::Identity()) = (0, 0, 0, 1)
  sim3[0] = sim3[1] = sim3[2] = 0.0; sim3[3] = 1.0;
  sim3[4] = sim3[5] = sim3[6] = 0.0; sim3[7] = (double)scale;
  int32_t acceptable = 0;
  double hi[6];
  rc = optimize_horn_dev(c, n, d, nullptr, nullptr, sim3, chi_limit * chi_limit, 0.01, &acceptable, hi);
  if (rc != DSH_OK) return rc;
  if (info) {
    info[0] = scale;
    for (int i = 0; i < 6; i++) info[1 + i] = hi[i];
    info[7] = acceptable;
  }
  if (!acceptable && check_chi) return DSH_OK;
  compose(sim3, Twc, s22, Tcw_new);
  *registered = 1;
  return DSH_OK;
}

}  // extern "C"
