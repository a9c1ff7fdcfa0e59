// C ABI of the Schwarzian warp fit (include/defslam_hip.h: dsh_schwarp_eval, dsh_schwarp_fit, _fit_batch, _fit_batch_store).
// A fit -- the trust-region loop of the reference (3 iterations, SchwarpDatabase.cc:211-222) with its control on the device -- is one fixed
// sequence of launches for the whole batch (nrsfm_kernels.hip: nrsfm_swp_fit_batch); the single fit is a batch of one.
// Every call moves one block up and one block down (UpBlock / DownBlock, dsh_ctx.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "dsh_diffdb.h"
#include "dsh_schwarp.h"
#include "mapping_launch.h"
#include "schwarp_problem.h"

namespace {
bool args_ok(const dsh_bbs* b, int P, const float* kp1, const float* kp2, const float* invsig, const double* x) {
  return bbs_grid_ok(b) && P > 0 && kp1 && kp2 && invsig && x && b->nptsu * b->nptsv <= 4096;
}
}  // namespace

extern "C" {

int dsh_schwarp_eval(dsh_ctx* ctx, const dsh_bbs* bbs, int P, const float* kp1, const float* kp2, const float* invsig, double fx_slot, double fy_slot,
                     double lambda, const double* x, double* residuals, double* jacobian) {
  dsh_ctx_base* c = dsh_base(ctx);
  if (!c) return DSH_ERR_ARG;
  if (const int rc = dsh_enter(c, "dsh_schwarp_eval")) return rc;
  if (!args_ok(bbs, P, kp1, kp2, invsig, x) || !residuals) return dsh_fail(c, DSH_ERR_ARG, "dsh_schwarp_eval: bad argument");
  const SwpSizes s = swp_sizes(bbs->nptsu, bbs->nptsv, P);
  const size_t r_bytes = 8 * (size_t)s.m, j_bytes = r_bytes * s.n2;   // the dense (2P + 4N) x 2N Jacobian: only when it is asked for
  hipStream_t st = c->stream;
  UpBlock up;
  const size_t o_kp1 = up.copy_of(kp1, 8 * (size_t)P), o_kp2 = up.copy_of(kp2, 8 * (size_t)P), o_isg = up.copy_of(invsig, 4 * (size_t)P), o_x = up.copy_of(x, 8 * (size_t)s.n2);
  DownBlock down;
  const size_t d_r = down.copy_to(residuals, r_bytes), d_J = down.copy_to(jacobian, j_bytes);
  if (const int rc = up.copy(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  HIPCHK(c, nrsfm_swp_eval(bbs_par(bbs, 2), P, fx_slot, fy_slot, lambda, up.dev<float>(o_kp1), up.dev<float>(o_kp2), up.dev<float>(o_isg), up.dev<double>(o_x),
                           down.dev<double>(d_r), jacobian ? down.dev<double>(d_J) : nullptr, jacobian ? 1 : 0, st));
  return down.receive(c);
}

}  // extern "C"

// The batched fit: every problem's inputs go up in ONE copy, the fits advance together through a fixed sequence of launches
// with the trust-region control on the device (nrsfm_kernels.hip: nrsfm_swp_fit_batch), every result comes back in ONE copy.
// stores / db (both or neither): the DiffProp records of the matches that are kept go into the device-resident database instead of
// (or besides) the host -- dsh_schwarp_fit_batch_store.  fit_batch: the checks; dsh::swp_fit_stages (dsh_schwarp.h): the stages.
static int fit_batch(dsh_ctx* ctx, int B, dsh_schwarp_problem* probs, const dsh_schwarp_store* stores, dsh_diffdb* db) {
  dsh_ctx_base* c = dsh_base(ctx);
  if (!c) return DSH_ERR_ARG;
  if (const int rc = dsh_enter(c, "dsh_schwarp_fit_batch")) return rc;
  if (B <= 0 || !probs) return dsh_fail(c, DSH_ERR_ARG, "dsh_schwarp_fit_batch: bad argument");
  if (db && (db->ctx != c || !stores)) return dsh_fail(c, DSH_ERR_ARG, "dsh_schwarp_fit_batch_store: the database belongs to another context / no store descriptors");
  if (db) {   // room for every record this call can add, BEFORE anything is launched: a call stores all of its records or fails untouched
    long long worst = 0;
    for (int b = 0; b < B; b++) worst += std::max(probs[b].P, 0);
    if (ddb_reserve(db, db->count + worst) != 0) return dsh_fail(c, DSH_ERR_HIP, "dsh_schwarp_fit_batch_store: out of device memory while growing the database");
  }
  for (int b = 0; b < B; b++) {
    const dsh_schwarp_problem& q = probs[b];
    if (!args_ok(&q.bbs, q.P, q.kp1, q.kp2, q.invsig, q.x) || q.max_iters < 0 || q.max_iters > 1000) return dsh_fail(c, DSH_ERR_ARG, "dsh_schwarp_fit_batch: bad argument in problem " + std::to_string(b));
    if (q.bbs.nptsu * q.bbs.nptsv > 256)
      return dsh_fail(c, DSH_ERR_ARG, "dsh_schwarp_fit: more than 256 control points (the one-workgroup solve handles 2N <= 512 unknowns; the reference uses 13 x 15 = 195)");
    if (!db && (q.diff == nullptr) != (q.drop == nullptr)) return dsh_fail(c, DSH_ERR_ARG, "dsh_schwarp_fit_batch: diff and drop go together");
    if (db && !stores[b].point_id) return dsh_fail(c, DSH_ERR_ARG, "dsh_schwarp_fit_batch_store: point_id missing in problem " + std::to_string(b));
  }
  return dsh::swp_fit_stages(c, B, probs, stores, db, nullptr);
}

int dsh::swp_fit_stages(dsh_ctx_base* c, int B, dsh_schwarp_problem* probs, const dsh_schwarp_store* stores, dsh_diffdb* db, SwpDevice* dev) {
  int maxP = 0, maxN = 0, max_it = 0;
  for (int b = 0; b < B; b++) {
    const dsh_schwarp_problem& q = probs[b];
    maxP = std::max(maxP, q.P); maxN = std::max(maxN, q.bbs.nptsu * q.bbs.nptsv); max_it = std::max(max_it, q.max_iters);
  }
  hipStream_t st = c->stream;
  // ---- layout of the input block (host-staged) and of the output block
  UpBlock in;
  DownBlock out;
  const size_t o_fits = in.take(sizeof(SwpFit) * (size_t)B);   // the fit descriptors
  int with_init = 0;
  struct Off { size_t kp1, kp2, isg, cs, xo, diff, drop, info, costs, bend; };
  std::vector<Off> off(B);
  std::vector<SwpSizes> sizes(B);
  // x lives at the head of the output block (in/out): only that part is uploaded with the start values
  for (int b = 0; b < B; b++) {
    sizes[b] = swp_sizes(probs[b].bbs.nptsu, probs[b].bbs.nptsv, probs[b].P);
    off[b].xo = out.take(8 * (size_t)sizes[b].n2);
  }
  const size_t x_bytes = out.size;
  for (int b = 0; b < B; b++) {
    const dsh_schwarp_problem& q = probs[b];
    const size_t n2 = (size_t)sizes[b].n2;
    Off& o = off[b];
    o.kp1 = in.take(dev ? 0 : 8 * (size_t)q.P);   // dev: the matches lie on the device already
    o.kp2 = in.take(dev ? 0 : 8 * (size_t)q.P);
    o.isg = in.take(dev ? 0 : 4 * (size_t)q.P);
    o.cs = in.take(8 * n2);
    // bending matrix of the Warp::initialize stage: one per run of problems with the same grid and weight
    o.bend = 0;
    if (q.init_lambda > 0.0) {
      const bool same = b > 0 && probs[b - 1].init_lambda == q.init_lambda && std::memcmp(&probs[b - 1].bbs, &q.bbs, sizeof(dsh_bbs)) == 0 && off[b - 1].bend;
      if (same) o.bend = off[b - 1].bend;
      else { o.bend = in.take(8 * (n2 / 2) * (n2 / 2)); }
      with_init = 1;
    }
    o.diff = out.take(!db && q.diff ? 72 * (size_t)q.P : 0);     // store mode: records and flags live in one strided block (below)
    o.drop = out.take(!db && q.drop ? (size_t)q.P : 0);
    o.info = out.take(256);
    o.costs = out.take(256);
  }
  // store mode: DiffProp records / drop flags / point ids / tags / second-keyframe indices of all fits, problem b at stride maxP.  What
  // the host reads of them -- the flags, the records if a problem asks for them, the count of the records added -- ends the output block
  DevBuf sdiff_ws, skeep, spos, stmp;
  const size_t nall = (size_t)B * maxP, fits_end = out.size;   // fits_end: the part of the output block that starts at zero
  size_t o_pid = 0, o_tag = 0, o_idx2 = 0, o_sdrop = 0, o_sdiff = 0, o_added = 0;
  bool want_diff = false;
  for (int b = 0; b < B; b++) want_diff = want_diff || probs[b].diff != nullptr;
  if (db) {
    o_pid = in.take(4 * nall);
    o_tag = in.take(4 * nall);
    o_idx2 = in.take(4 * nall);
    o_sdrop = out.take(nall);
    o_sdiff = out.take(want_diff ? 72 * nall : 0);
    o_added = out.take(8);
    if (!want_diff) HIPCHK(c, sdiff_ws.alloc(c, 72 * nall));
    HIPCHK(c, skeep.alloc(c, 4 * nall)); HIPCHK(c, spos.alloc(c, 4 * nall)); HIPCHK(c, stmp.alloc(c, ddb_scan_tmp_bytes((int)nall)));
  }
  // the descriptors hold device addresses of both blocks: both are placed before anything is filled in.  The start values of x are
  // staged behind the input block, laid out like the head of the output block, and go up in a copy of their own
  if (const int rc = in.place(c)) return rc;
  if (const int rc = out.alloc(c)) return rc;
  if (const int rc = in.stage(c, x_bytes)) return rc;
  char* hx = in.host<char>(in.size);
  std::memset(hx, 0, x_bytes);
  float* sdiff = want_diff ? out.dev<float>(o_sdiff) : sdiff_ws.as<float>();
  uint8_t* sdrop = out.dev<uint8_t>(o_sdrop);
  // what has to start at zero (scalars of the controller, the step vector) lies in one block: one memset for the whole batch
  DevBuf dzero;
  size_t zero_bytes = 0;
  for (int b = 0; b < B; b++) zero_bytes += 128 + Arena::round(8 * (size_t)sizes[b].n2);
  HIPCHK(c, dzero.alloc(c, zero_bytes));
  HIPCHK(c, hipMemsetAsync(dzero.p, 0, zero_bytes, st));
  size_t zoff = 0;
  for (int b = 0; b < B; b++) {
    const dsh_schwarp_problem& q = probs[b];
    const Off& o = off[b];
    const SwpSizes& s = sizes[b];
    const bool init = q.init_lambda > 0.0;
    if (!dev) {
      std::memcpy(in.host<float>(o.kp1), q.kp1, 8 * (size_t)q.P); std::memcpy(in.host<float>(o.kp2), q.kp2, 8 * (size_t)q.P);
      std::memcpy(in.host<float>(o.isg), q.invsig, 4 * (size_t)q.P);
    }
    std::fill_n(in.host<double>(o.cs), s.n2, 1.0);
    if (init) {
      if (b == 0 || off[b - 1].bend != o.bend) dsh::bbs_bending_dense(&q.bbs, q.init_lambda, in.host<double>(o.bend));
    } else if (!dev) {
      std::memcpy(hx + o.xo, q.x, 8 * (size_t)s.n2);
    }
    SwpFit f{};
    f.p = SwpPar{q.bbs.umin, q.bbs.umax, q.bbs.vmin, q.bbs.vmax, q.fx_slot, q.fy_slot, q.lambda, q.bbs.nptsu, q.bbs.nptsv, q.bbs.nptsu * q.bbs.nptsv, q.P};
    f.fx = q.fx; f.fy = q.fy;
    f.n2 = s.n2; f.m = s.m; f.np = s.np; f.il = s.il; f.bwt = s.bwt; f.npi = s.npi; f.bwti = s.bwti;
    f.max_iters = q.max_iters;
    f.kp1 = dev ? dev->kp1 : in.dev<float>(o.kp1); f.kp2 = dev ? dev->kp2 : in.dev<float>(o.kp2); f.isg = dev ? dev->isg : in.dev<float>(o.isg);
    f.cs = in.dev<double>(o.cs);
    f.bend = init ? in.dev<double>(o.bend) : nullptr;
    f.x = out.dev<double>(o.xo);
    f.diff = dev ? dev->diff : db ? sdiff + 18 * (size_t)b * maxP : (q.diff ? out.dev<float>(o.diff) : nullptr);
    f.drop = dev ? dev->drop : db ? sdrop + (size_t)b * maxP : (q.drop ? out.dev<uint8_t>(o.drop) : nullptr);
    f.info = out.dev<int32_t>(o.info);
    f.costs = out.dev<double>(o.costs);
    f.scal = reinterpret_cast<double*>(dzero.as<char>() + zoff);
    f.dx = reinterpret_cast<double*>(dzero.as<char>() + zoff + 128);
    zoff += 128 + Arena::round(8 * (size_t)s.n2);
    // the per-fit scratch.  The dense (2P+4N) x 2N buffer only serves the Warp::initialize stage (its colocation matrix); the fit keeps
    // its Jacobian structured
    DevBuf compact;
    HIPCHK(c, dsh_scratch_array(c, &f.xn, (size_t)s.n2)); HIPCHK(c, dsh_scratch_array(c, &f.g, (size_t)s.n2)); HIPCHK(c, dsh_scratch_array(c, &f.r, (size_t)s.m));
    HIPCHK(c, dsh_scratch_array(c, &f.J, init ? (size_t)s.m * s.n2 : 32)); HIPCHK(c, compact.alloc(c, swp_compact(f, nullptr)));
    HIPCHK(c, dsh_scratch_array(c, &f.A, (size_t)s.n2 * s.n2)); HIPCHK(c, dsh_scratch_array(c, &f.M, (size_t)s.np * s.np)); HIPCHK(c, dsh_scratch_array(c, &f.W, (size_t)s.np * 16));
    swp_compact(f, compact.as<char>());
    in.host<SwpFit>(o_fits)[b] = f;
  }
  int32_t max_pid = -1;
  if (db) {
    int32_t* hp = in.host<int32_t>(o_pid);
    int32_t* ht = in.host<int32_t>(o_tag);
    int32_t* hi = in.host<int32_t>(o_idx2);
    for (int b = 0; b < B; b++)
      for (int i = 0; i < maxP; i++) {
        const bool in_fit = i < probs[b].P;
        const int32_t id = in_fit ? stores[b].point_id[i] : -1;
        hp[(size_t)b * maxP + i] = id;
        ht[(size_t)b * maxP + i] = stores[b].tag;
        hi[(size_t)b * maxP + i] = (in_fit && stores[b].idx2) ? stores[b].idx2[i] : (in_fit ? i : -1);
        max_pid = std::max(max_pid, id);
      }
  }
  if (const int rc = in.send(c)) return rc;
  if (dev) HIPCHK(c, hipMemcpyAsync(out.d + off[0].xo, dev->x0, 8 * (size_t)sizes[0].n2, hipMemcpyDeviceToDevice, st));
  else HIPCHK(c, hipMemcpyAsync(out.d, hx, x_bytes, hipMemcpyHostToDevice, st));
  if (fits_end > x_bytes) HIPCHK(c, hipMemsetAsync(out.d + x_bytes, 0, fits_end - x_bytes, st));
  HIPCHK(c, nrsfm_swp_fit_batch(in.dev<SwpFit>(o_fits), B, maxP, maxN, max_it, with_init, st));
  if (dev) {   // the results stay where they are; the caller's block brings them down
    dev->x = out.dev<double>(off[0].xo); dev->info = out.dev<int32_t>(off[0].info); dev->costs = out.dev<double>(off[0].costs);
    return DSH_OK;
  }
  if (db) {   // kept records -> the database, in (fit, match) order; records added = exclusive scan position + keep flag of the last entry
    HIPCHK(c, ddb_append((int)nall, sdrop, sdiff, in.dev<int32_t>(o_pid), in.dev<int32_t>(o_tag), in.dev<int32_t>(o_idx2), skeep.as<int32_t>(), spos.as<int32_t>(),
                         stmp.p, ddb_scan_tmp_bytes((int)nall), db->count, db->cap, db->rec, db->pid, db->tag, db->idx2, st));
    HIPCHK(c, hipMemcpyAsync(out.dev<int32_t>(o_added), spos.as<int32_t>() + nall - 1, 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipMemcpyAsync(out.dev<int32_t>(o_added) + 1, skeep.as<int32_t>() + nall - 1, 4, hipMemcpyDeviceToDevice, st));
  }
  if (const int rc = out.receive(c)) return rc;
  if (db) {
    const int32_t added = out.host<int32_t>(o_added)[0] + out.host<int32_t>(o_added)[1];
    if (db->count + added > db->cap) return dsh_fail(c, DSH_ERR_STATE, "dsh_schwarp_fit_batch_store: internal error, the reserved capacity was exceeded");
    db->count += added;
    db->max_pid = std::max(db->max_pid, max_pid);
  }
  for (int b = 0; b < B; b++) {
    dsh_schwarp_problem& q = probs[b];
    const Off& o = off[b];
    std::memcpy(q.x, out.host<double>(o.xo), 8 * (size_t)sizes[b].n2);
    if (db) {
      if (q.drop) std::memcpy(q.drop, out.host<uint8_t>(o_sdrop) + (size_t)b * maxP, (size_t)q.P);
      if (q.diff) std::memcpy(q.diff, out.host<float>(o_sdiff) + 18 * (size_t)b * maxP, 72 * (size_t)q.P);
    } else if (q.diff) { std::memcpy(q.diff, out.host<float>(o.diff), 72 * (size_t)q.P); std::memcpy(q.drop, out.host<uint8_t>(o.drop), (size_t)q.P); }
    std::memcpy(q.info, out.host<int32_t>(o.info), sizeof q.info);
    std::memcpy(&q.init_ok, out.host<int32_t>(o.info) + 2, sizeof q.init_ok);   // info[2]: the verdict on the initialisation
    std::memcpy(q.costs, out.host<double>(o.costs), sizeof q.costs);
  }
  return DSH_OK;
}

extern "C" {

int dsh_schwarp_fit_batch(dsh_ctx* ctx, int B, dsh_schwarp_problem* probs) { return fit_batch(ctx, B, probs, nullptr, nullptr); }

int dsh_schwarp_fit_batch_store(dsh_ctx* ctx, int B, dsh_schwarp_problem* probs, const dsh_schwarp_store* stores, dsh_diffdb* db) {
  if (!db || !stores) return dsh_fail(dsh_base(ctx), DSH_ERR_ARG, "dsh_schwarp_fit_batch_store: bad argument");
  return fit_batch(ctx, B, probs, stores, db);
}

int dsh_schwarp_fit(dsh_ctx* ctx, const dsh_bbs* bbs, int P, const float* kp1, const float* kp2, const float* invsig, double fx_slot, double fy_slot,
                    double lambda, float fx, float fy, int max_iters, double* x, dsh_diffprop* diff, uint8_t* drop, int32_t* info, double* costs) {
  dsh_ctx_base* c = dsh_base(ctx);
  if (!c) return DSH_ERR_ARG;
  if (c->host_only) return dsh_fail(c, DSH_ERR_NO_DEVICE, "dsh_schwarp_fit: host-only context, no GPU (there is no CPU fallback)");
  if (!args_ok(bbs, P, kp1, kp2, invsig, x) || max_iters < 0) return dsh_fail(c, DSH_ERR_ARG, "dsh_schwarp_fit: bad argument");
  dsh_schwarp_problem q{};
  q.bbs = *bbs; q.P = P; q.kp1 = kp1; q.kp2 = kp2; q.invsig = invsig; q.fx_slot = fx_slot; q.fy_slot = fy_slot; q.lambda = lambda; q.fx = fx; q.fy = fy;
  q.max_iters = max_iters; q.x = x;
  q.diff = (diff && drop) ? diff : nullptr; q.drop = (diff && drop) ? drop : nullptr;
  const int rc = dsh_schwarp_fit_batch(ctx, 1, &q);
  if (rc != DSH_OK) return rc;
  if (info) { info[0] = q.info[0]; info[1] = q.info[1]; }
  if (costs) { costs[0] = q.costs[0]; costs[1] = q.costs[1]; }
  return DSH_OK;
}

}  // extern "C"
