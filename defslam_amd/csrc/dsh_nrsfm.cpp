// C ABI of the NRSfM mapping-side entry points (include/defslam_hip.h): B-spline evaluation / colocation and
// the per-map-point normal solve.  One-shot calls: one block up, device kernels, one block down (UpBlock / DownBlock, dsh_ctx.h).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "mapping_launch.h"

namespace dsh {

void normals_fill_records(int P, const int32_t* rec_ptr, const dsh_diffprop* recs, int32_t* owner, float* soa) {
  constexpr int NF = 18;
  const int R = rec_ptr[P];
  for (int p = 0; p < P; p++)
    for (int r = rec_ptr[p]; r < rec_ptr[p + 1]; r++) owner[r] = p;
  for (int r = 0; r < R; r++) {
    const float* f = reinterpret_cast<const float*>(&recs[r]);
    for (int k = 0; k < NF; k++) soa[(size_t)k * R + r] = f[k];
  }
}

int normals_stage(dsh_ctx_base* c, int P, int R, const NormalsIn& in, const NormalsOut& out) {
  const size_t Pn = (size_t)P, Rn = R > 0 ? (size_t)R : 1, Rz = (size_t)(R > 0 ? R : 0);
  hipStream_t st = c->stream;
  // an optional output that the caller does not want, or that has no record, is written into the work space instead of the block
  DownBlock down;
  Arena ws;
  struct Slot { bool fetched; size_t off; };
  auto lay = [&](void* host, size_t bytes, size_t room) { return host && bytes ? Slot{true, down.copy_to(host, bytes)} : Slot{false, ws.take(room)}; };
  const size_t o_k = down.copy_to(out.k1k2, 16 * Pn), o_st = down.copy_to(out.status, 4 * Pn);
  const Slot s_cov = lay(out.cov, 32 * Pn, 32 * Pn), s_nref = lay(out.normal_ref, 12 * Pn, 12 * Pn), s_it = lay(out.iters, 4 * Pn, 4 * Pn),
             s_nrec = lay(out.normal_rec, 12 * Rz, 12 * Rn), s_wr = lay(out.rec_written, Rz, Rn);
  const size_t o_Q = ws.take(8 * 20 * Rn);
  size_t o_list[3];
  for (int i = 0; i < 3; i++) o_list[i] = down.copy_to(out.rec_list[i], 4 * Rz);
  char* w = nullptr;
  if (const int rc = down.alloc(c)) return rc;
  HIPCHK(c, c->scratch.take(ws.size, (void**)&w));
  auto dev = [&](Slot s) { return static_cast<void*>((s.fetched ? down.d : w) + s.off); };
  double* d_cov = static_cast<double*>(dev(s_cov));
  float *d_nref = static_cast<float*>(dev(s_nref)), *d_nrec = static_cast<float*>(dev(s_nrec));
  HIPCHK(c, hipMemsetAsync(d_cov, 0, 32 * Pn, st));
  HIPCHK(c, hipMemsetAsync(d_nref, 0, 12 * Pn, st));
  HIPCHK(c, hipMemsetAsync(d_nrec, 0, 12 * Rn, st));
  HIPCHK(c, nrsfm_launch_normals(P, R, in.rec_ptr, in.owner, in.soa, in.is_ref, in.first_n, in.has_first_n, in.x0, in.has_x0, in.ref_uv,
                                 reinterpret_cast<double*>(w + o_Q), down.dev<double>(o_k), d_cov, down.dev<int32_t>(o_st), d_nref, d_nrec,
                                 static_cast<uint8_t*>(dev(s_wr)), static_cast<int32_t*>(dev(s_it)), st));
  if (in.keep_normals) {
    HIPCHK(c, hipMemcpyAsync(in.keep_normals, d_nref, 12 * Pn, hipMemcpyDeviceToDevice, st));
    if (R > 0) HIPCHK(c, hipMemcpyAsync(in.keep_normals + 3 * Pn, d_nrec, 12 * Rz, hipMemcpyDeviceToDevice, st));
  }
  for (int i = 0; i < 3; i++)
    if (out.rec_list[i] && R > 0) HIPCHK(c, hipMemcpyAsync(down.dev<int32_t>(o_list[i]), in.rec_list[i], 4 * Rz, hipMemcpyDeviceToDevice, st));
  return down.receive(c);
}

}  // namespace dsh

extern "C" {

int dsh_bbs_eval(dsh_ctx* ctx, const dsh_bbs* bbs, const double* ctrl, const double* u, const double* v, int n, int du, int dv, double* val, uint8_t* outside) {
  dsh_ctx_base* c = dsh_base(ctx);
  int rc = dsh_enter(c, "dsh_bbs_eval");
  if (rc != DSH_OK) return rc;
  if (!bbs_grid_ok(bbs) || bbs->valdim < 1 || !ctrl || n < 0 || (n > 0 && (!u || !v || !val)) || du < 0 || du > 2 || dv < 0 || dv > 2)
    return dsh_fail(c, DSH_ERR_ARG, "dsh_bbs_eval: bad argument");
  if (n == 0) return DSH_OK;
  const size_t m = (size_t)n;
  UpBlock up;
  const size_t o_ctrl = up.copy_of(ctrl, 8 * (size_t)bbs->valdim * bbs->nptsu * bbs->nptsv), o_u = up.copy_of(u, 8 * m), o_v = up.copy_of(v, 8 * m);
  DownBlock down;
  const size_t d_val = down.copy_to(val, 8 * m * bbs->valdim), d_out = down.copy_to(outside, m);
  uint8_t* flags = nullptr;   // the kernel writes them in any case
  if (!outside) HIPCHK(c, dsh_scratch_array(c, &flags, m));
  if ((rc = up.copy(c)) != DSH_OK || (rc = down.alloc(c)) != DSH_OK) return rc;
  HIPCHK(c, nrsfm_launch_bbs_eval(bbs_par(bbs, bbs->valdim), up.dev<double>(o_ctrl), up.dev<double>(o_u), up.dev<double>(o_v), n, du, dv, down.dev<double>(d_val),
                                  outside ? down.dev<uint8_t>(d_out) : flags, c->stream));
  return down.receive(c);
}

int dsh_bbs_coloc(dsh_ctx* ctx, const dsh_bbs* bbs, const double* u, const double* v, int n, int du, int dv, int32_t* cols, double* w, int32_t* n_outside) {
  dsh_ctx_base* c = dsh_base(ctx);
  int rc = dsh_enter(c, "dsh_bbs_coloc");
  if (rc != DSH_OK) return rc;
  if (!bbs_grid_ok(bbs) || bbs->valdim < 1 || n < 0 || (n > 0 && (!u || !v || !cols || !w)) || du < 0 || du > 2 || dv < 0 || dv > 2)
    return dsh_fail(c, DSH_ERR_ARG, "dsh_bbs_coloc: bad argument");
  if (n_outside) *n_outside = 0;
  if (n == 0) return DSH_OK;
  const size_t m = (size_t)n;
  UpBlock up;
  const size_t o_u = up.copy_of(u, 8 * m), o_v = up.copy_of(v, 8 * m);
  DownBlock down;
  const size_t d_cols = down.copy_to(cols, 4 * 16 * m), d_w = down.copy_to(w, 8 * 16 * m), d_cnt = down.copy_to(n_outside, 4);
  int32_t* cnt = nullptr;   // the kernel counts in any case
  if (!n_outside) HIPCHK(c, dsh_scratch_array(c, &cnt, 1));
  if ((rc = up.copy(c)) != DSH_OK || (rc = down.alloc(c)) != DSH_OK) return rc;
  if (n_outside) cnt = down.dev<int32_t>(d_cnt);
  HIPCHK(c, hipMemsetAsync(cnt, 0, 4, c->stream));
  HIPCHK(c, nrsfm_launch_bbs_coloc(bbs_par(bbs, 1), up.dev<double>(o_u), up.dev<double>(o_v), n, du, dv, down.dev<int32_t>(d_cols), down.dev<double>(d_w), cnt, c->stream));
  return down.receive(c);
}

int dsh_normals_estimate(dsh_ctx* ctx, int P, const int32_t* rec_ptr, const dsh_diffprop* recs, const uint8_t* rec_is_ref, const float* rec_first_normal,
                         const uint8_t* rec_has_first_normal, const float* x0, const uint8_t* has_x0, const float* ref_uv, double* k1k2, double* cov,
                         int32_t* status, float* normal_ref, float* normal_rec, uint8_t* rec_written, int32_t* iters) {
  dsh_ctx_base* c = dsh_base(ctx);
  int rc = dsh_enter(c, "dsh_normals_estimate");
  if (rc != DSH_OK) return rc;
  if (P < 0 || (P > 0 && (!rec_ptr || !x0 || !has_x0 || !ref_uv || !k1k2 || !status))) return dsh_fail(c, DSH_ERR_ARG, "dsh_normals_estimate: bad argument");
  if (P == 0) return DSH_OK;
  const int R = rec_ptr[P];
  if (R < 0 || rec_ptr[0] != 0) return dsh_fail(c, DSH_ERR_ARG, "dsh_normals_estimate: bad rec_ptr");
  for (int p = 0; p < P; p++)
    if (rec_ptr[p + 1] < rec_ptr[p]) return dsh_fail(c, DSH_ERR_ARG, "dsh_normals_estimate: rec_ptr not monotone");
  if (R > 0 && (!recs || !rec_is_ref || !rec_first_normal || !rec_has_first_normal)) return dsh_fail(c, DSH_ERR_ARG, "dsh_normals_estimate: null records");
  const size_t Pn = (size_t)P, Rz = (size_t)R;
  UpBlock up;
  const size_t o_ptr = up.copy_of(rec_ptr, 4 * (Pn + 1)), o_x0 = up.copy_of(x0, 8 * Pn), o_hx0 = up.copy_of(has_x0, Pn), o_uv = up.copy_of(ref_uv, 8 * Pn),
               o_owner = up.take(4 * Rz), o_soa = up.take(72 * Rz), o_isref = up.copy_of(rec_is_ref, Rz), o_fn = up.copy_of(rec_first_normal, 8 * Rz),
               o_hfn = up.copy_of(rec_has_first_normal, Rz);
  if ((rc = up.stage(c)) != DSH_OK) return rc;
  // SoA transpose of the reference's DiffProp records + owner point of every record
  if (R > 0) dsh::normals_fill_records(P, rec_ptr, recs, up.host<int32_t>(o_owner), up.host<float>(o_soa));
  if ((rc = up.send(c)) != DSH_OK) return rc;
  const dsh::NormalsIn in = {up.dev<int32_t>(o_ptr), up.dev<int32_t>(o_owner), up.dev<float>(o_soa), up.dev<uint8_t>(o_isref), up.dev<float>(o_fn),
                             up.dev<uint8_t>(o_hfn), up.dev<float>(o_x0), up.dev<uint8_t>(o_hx0), up.dev<float>(o_uv), {nullptr, nullptr, nullptr}, nullptr};
  return dsh::normals_stage(c, P, R, in, {k1k2, cov, status, normal_ref, iters, normal_rec, rec_written, {nullptr, nullptr, nullptr}});
}

}  // extern "C"
