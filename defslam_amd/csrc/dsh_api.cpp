// C ABI of libdefslam_hip.so: context, template, SfT pack / upload / run / download.
// Declared in include/defslam_hip.h.  Compiled with hipcc (host side).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "dsh_sft_ctx.h"

#include "mapping_launch.h"

#ifdef DSH_LAB
#include "../../include/defslam_hip_debug.h"
#endif

LdsMarks g_lds_marks[64];   // (dsh_sft_ctx.h)
std::mutex g_lds_mu;

using dsh::Tcw_from_pose7;

dsh_ctx_base* dsh_base(dsh_ctx* ctx) { return static_cast<dsh_ctx_base*>(ctx); }
const dsh::TemplateHost* dsh_facet_template(dsh_ctx_base* c) {
  const dsh_ctx* x = static_cast<const dsh_ctx*>(c);
  return x && x->tmpl.valid && x->tmpl.F > 0 ? &x->tmpl : nullptr;
}

namespace {

void drop_graphs(dsh_ctx* c) {
  if (!c->host_only && c->stream) (void)hipStreamSynchronize(c->stream);   // a batch in flight may still read them
  for (auto& g : c->graphs)
    if (g->d_base) (void)hipFree(g->d_base);
  c->graphs.clear();
  c->packed.clear();
}

int upload_template(dsh_ctx* c) {
  c->B = 0;
  c->ran = false;
  drop_graphs(c);
  if (c->host_only) return DSH_OK;
  const dsh::TemplateHost& t = c->tmpl;
  Arena a;
  const size_t o_xyz0 = a.take(sizeof(double) * 3 * t.n);
  const size_t o_ptr = a.take(sizeof(int32_t) * (t.n + 1));
  const size_t o_idx = a.take(sizeof(int32_t) * t.nbr_idx.size());
  const size_t o_w = a.take(sizeof(double) * t.nbr_w.size());
  const size_t o_sw = a.take(sizeof(double) * t.n);
  const size_t o_k0 = a.take(sizeof(double) * t.n);
  if (c->d_tmpl) { (void)hipFree(c->d_tmpl); c->d_tmpl = nullptr; }
  HIPCHK(c, hipMalloc((void**)&c->d_tmpl, a.size));
  c->d_tmpl_bytes = a.size;
  std::vector<char> st(a.size, 0);
  std::memcpy(&st[o_xyz0], t.xyz0.data(), sizeof(double) * 3 * t.n);
  std::memcpy(&st[o_ptr], t.nbr_ptr.data(), sizeof(int32_t) * (t.n + 1));
  std::memcpy(&st[o_idx], t.nbr_idx.data(), sizeof(int32_t) * t.nbr_idx.size());
  std::memcpy(&st[o_w], t.nbr_w.data(), sizeof(double) * t.nbr_w.size());
  std::memcpy(&st[o_sw], t.nbr_sumw.data(), sizeof(double) * t.n);
  std::memcpy(&st[o_k0], t.k0.data(), sizeof(double) * t.n);
  HIPCHK(c, hipMemcpy(c->d_tmpl, st.data(), a.size, hipMemcpyHostToDevice));
  c->dt.xyz0 = (const double*)(c->d_tmpl + o_xyz0);
  c->dt.nbr_ptr = (const int32_t*)(c->d_tmpl + o_ptr);
  c->dt.nbr_idx = (const int32_t*)(c->d_tmpl + o_idx);
  c->dt.nbr_w = (const double*)(c->d_tmpl + o_w);
  c->dt.nbr_sumw = (const double*)(c->d_tmpl + o_sw);
  c->dt.k0 = (const double*)(c->d_tmpl + o_k0);
  return DSH_OK;
}

template <class T>
size_t reserve(Arena& a, const std::vector<T>& v) { return a.take(sizeof(T) * v.size()); }
template <class T>
void put(char* st, size_t off, const std::vector<T>& v) {
  if (!v.empty()) std::memcpy(st + off, v.data(), sizeof(T) * v.size());
}

// The graph of the frame's active set: cached per template, uploaded once, shared by every problem that has it.
int graph_for(dsh_ctx* c, const std::vector<uint8_t>& opt, dsh::SftGraph** out, std::string& err) {
  uint64_t h = 1469598103934665603ull;
  for (uint8_t b : opt) { h ^= b; h *= 1099511628211ull; }
  for (auto& g : c->graphs)
    if (g->opt_hash == h && g->opt == opt) { g->last_use = c->upload_serial; *out = g.get(); return DSH_OK; }
  if (c->graphs.size() >= 64) {
    // A long sequence with an ever-changing view: drop every graph the upload in progress does not use (rebuilding one costs a slow
    // frame).  Graphs of the problems already packed by THIS upload stay -- a batch with more than 64 active sets just grows the cache.
    if (!c->host_only && c->stream) (void)hipStreamSynchronize(c->stream);   // the previous batch may still read them
    auto& gs = c->graphs;
    for (size_t i = 0; i < gs.size();) {
      if (gs[i]->last_use != c->upload_serial) {
        if (gs[i]->d_base) (void)hipFree(gs[i]->d_base);
        gs.erase(gs.begin() + i);
      } else {
        i++;
      }
    }
  }
  std::unique_ptr<dsh::SftGraph> g(new dsh::SftGraph());
  const int rc = dsh::build_graph(c->tmpl, opt, *g, err);
  if (rc != DSH_OK) return rc;
  g->last_use = c->upload_serial;
  if (!c->host_only) {
    Arena a;
    auto& o = g->o;
    o.act = reserve(a, g->act); o.actnode = reserve(a, g->actnode); o.star_node = reserve(a, g->star_node); o.star_sL = reserve(a, g->star_sL);
    o.str_nodes = reserve(a, g->str_nodes); o.str_L0 = reserve(a, g->str_L0); o.off_ptr = reserve(a, g->off_ptr); o.off_rc = reserve(a, g->off_rc);
    o.sh_ptr = reserve(a, g->sh_ptr); o.sh_rec = reserve(a, g->sh_rec); o.sh_cf = reserve(a, g->sh_cf); o.tmask = reserve(a, g->tmask);
    o.hgather = reserve(a, g->hgather);
    o.hgatherT = reserve(a, g->hgatherT);
    std::vector<char> st(a.size, 0);
    put(st.data(), o.act, g->act); put(st.data(), o.actnode, g->actnode); put(st.data(), o.star_node, g->star_node); put(st.data(), o.star_sL, g->star_sL);
    put(st.data(), o.str_nodes, g->str_nodes); put(st.data(), o.str_L0, g->str_L0); put(st.data(), o.off_ptr, g->off_ptr); put(st.data(), o.off_rc, g->off_rc);
    put(st.data(), o.sh_ptr, g->sh_ptr); put(st.data(), o.sh_rec, g->sh_rec); put(st.data(), o.sh_cf, g->sh_cf); put(st.data(), o.tmask, g->tmask);
    put(st.data(), o.hgather, g->hgather);
    put(st.data(), o.hgatherT, g->hgatherT);
    if (hipMalloc((void**)&g->d_base, a.size) != hipSuccess) { err = "out of device memory (graph)"; return DSH_ERR_HIP; }
    g->d_bytes = a.size;
    if (hipMemcpy(g->d_base, st.data(), a.size, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(g->d_base); err = "graph upload failed"; return DSH_ERR_HIP; }
  }
  *out = g.get();
  c->graphs.push_back(std::move(g));
  return DSH_OK;
}

// Build the graph of DefOptimizer.cc:293-507 as flat arrays: shared structure from the cache, per-frame lists, scalars.
int pack_problem(dsh_ctx* c, const dsh_sft_frame& f, Packed& P, std::string& err) {
  const dsh::TemplateHost& t = c->tmpl;
  std::vector<uint8_t> viewed, opt;
  int rc = dsh::frame_active_set(t, f, viewed, opt, err);
  if (rc != DSH_OK) return rc;
  rc = graph_for(c, opt, &P.g, err);
  if (rc != DSH_OK) return rc;
  const dsh::SftGraph& g = *P.g;
  rc = dsh::pack_frame(t, g, f, viewed, P.f, err);
  if (rc != DSH_OK) return rc;
  SftDev& h = P.h;
  h = SftDev{};
  h.n = t.n; h.nA = g.nA; h.Dn = 3 * g.nA; h.kd = g.kd; h.ldh = h.kd + 1;
  // (the solver per half-bandwidth -- tile_mode, wbt, tpr -- and everything else that depends on the batch: sft_plan_batch)
  h.M = f.M; h.V = P.f.V; h.S = g.S; h.Es = g.Es; h.noff = g.noff; h.max_iters = f.max_iters; h.mode = 0;
  h.fx = f.K[0]; h.fy = f.K[1]; h.cx = f.K[2]; h.cy = f.K[3];
  h.w_ref = f.reg_temp / std::pow(t.median_L, 2);              // DefOptimizer.cc:378
  h.w_curv = f.reg_lap / (double)g.nA;                         // :458  (|OptLap|)
  h.w_str = g.Es > 0 ? f.reg_inex / (double)g.Es : 0.0;        // :497  (|medges|)
  const float deltaMono = (float)std::sqrt(5.991);             // :286
  h.hub_delta = (double)deltaMono;
  h.hub_dsqr = h.hub_delta * h.hub_delta;
  return DSH_OK;
}

// One solve of the uploaded batch.  K == 1: the persistent kernel, one launch, asynchronous.  K > 1 (latency mode): one launch
// per round of K damping trials; an iteration that accepts one of its first K trials takes one launch, so max_iters + 1 launches
// finish the typical frame; the done flags are read back behind them and further rounds are launched only while needed.
int run_rounds_enqueue(dsh_ctx* c);
// (Blocking: the rounds end with read-backs of the done counters.  On an error every sub-stream is drained before the error is returned, so that
// what the caller enqueues next on the context's stream cannot race with work left on another one.)
int run_rounds(dsh_ctx* c) {
  const int rc = run_rounds_enqueue(c);
  if (rc != DSH_OK)
    for (int s = 0; s < c->plan.n_sub; s++) if (c->sub_stream[s]) (void)hipStreamSynchronize(c->sub_stream[s]);
  return rc;
}
int run_rounds_enqueue(dsh_ctx* c) {
  // Throughput shape: every problem of the batch advances by one damping trial per round (LIN for those that start an iteration, FACTOR,
  // TRIAL).  As many rounds as the previous run needed are enqueued in one go, then the done counters are read back and rounds are added
  // in pairs while a problem still runs (a finished problem's workgroups leave at their first instruction).
  const int B = c->B, S = c->plan.n_sub;
  int b0[kSftMaxSub + 1];
  for (int s = 0; s <= S; s++) b0[s] = (int)((long long)B * s / S);
  // The last problems of a step go to the tail kernel (sft_batch.h): one workgroup runs each of them to its end.  It pays from about two
  // problems per CU downwards (a round costs one whole one-wavefront factorisation, 1 ms, however few problems it carries; a workgroup of the
  // tail kernel takes 0.5 ms per trial).  WHEN the rounds end is decided on the device: the LIN kernel of a round and the tail launch itself
  // both compare the finished count with the threshold and either can raise counters[6] (the count only grows, so the switch lands in the same
  // place) -- the results do not depend on how the launches are grouped here; a tail launch in front of the switch, like a round behind it,
  // leaves at its first instruction.
  // The threshold (A/B over batch sizes, tools/tail_ab.py): four problems per CU -- but not more than three quarters of the batch (a batch of
  // four per CU would run in the tail kernel alone: 234 against 277 k it/s), and a batch of two per CU or less does run there alone.
  int tail_below = -1;
  if (S == 1 && c->opt.tail != 0) {
    if (c->opt.tail > 0) tail_below = c->opt.tail * c->num_cus;                                                    // (lab option: exactly this many per CU)
    else tail_below = std::min(4 * c->num_cus, std::max(2 * c->num_cus, (int)((long long)3 * B / 4)));
  }
  auto launch = [&](int s, int phase) {
    const bool ev = c->phase_events && S == 1;
    if (ev) { hipEvent_t e; if (hipEventCreate(&e) == hipSuccess) { (void)hipEventRecord(e, c->stream); c->phase_events->push_back(e); c->phase_ids.push_back(phase); } }
    hipError_t r;
    {
      LDS_LOCK();
      if (phase == SFTB_PH_TAIL) r = sftb_tail_launch(c->d_probs + b0[s], c->d_runs + b0[s], c->d_counters + 16 * s, b0[s + 1] - b0[s], c->plan.max_kd, c->plan.jl_doubles, &LDS_MARKS(c).tail, c->num_cus, tail_below, c->sub_stream[s]);
      else r = sftb_launch(c->d_probs + b0[s], c->d_runs + b0[s], c->d_counters + 16 * s, c->d_linlist + b0[s], b0[s + 1] - b0[s], phase, c->plan.jl_doubles, c->plan.xyz_doubles, LDS_MARKS(c).b,
                           c->num_cus, tail_below, c->sub_stream[s]);
    }
    if (ev) { hipEvent_t e; if (hipEventCreate(&e) == hipSuccess) { (void)hipEventRecord(e, c->stream); c->phase_events->push_back(e); } }
    return r;
  };
  // the other streams start behind whatever the context's stream has enqueued (the upload)
  if (S > 1) {
    HIPCHK(c, hipEventRecord(c->sub_event[0], c->stream));
    for (int s = 1; s < S; s++) HIPCHK(c, hipStreamWaitEvent(c->sub_stream[s], c->sub_event[0], 0));
  }
  for (int s = 0; s < S; s++) HIPCHK(c, launch(s, SFTB_PH_INIT));
  const int worst = std::max(1, c->plan.max_iters_batch) * 10 + 1;
  // first group: the rounds the previous run of this context needed in front of its tail kernel (or, without one, to the end)
  int rounds = 0, group = std::max(1, std::min(worst, c->rounds_hint));
  if (tail_below >= B) group = 0;   // (a batch this small: the tail kernel from the start)
  HIPCHK(c, c->spec_done.ensure(64 * kSftMaxSub, true));
  int rc = DSH_OK;
  while (true) {
    for (int i = 0; i < group && rounds < worst; i++, rounds++)
      for (int s = 0; s < S; s++) {
        HIPCHK(c, launch(s, SFTB_PH_LIN));
        HIPCHK(c, launch(s, SFTB_PH_FACTOR));
        HIPCHK(c, launch(s, SFTB_PH_TRIAL));
      }
    if (tail_below >= 0) HIPCHK(c, launch(0, SFTB_PH_TAIL));
    // [0] finished problems, [6] tail mode, [7] the round that switched to it
    for (int s = 0; s < S; s++) HIPCHK(c, hipMemcpyAsync(c->spec_done.p + 64 * s, c->d_counters + 16 * s, 8 * sizeof(int), hipMemcpyDeviceToHost, c->sub_stream[s]));
    for (int s = 0; s < S; s++) HIPCHK(c, hipStreamSynchronize(c->sub_stream[s]));
    int done = 0;
    for (int s = 0; s < S; s++) done += *reinterpret_cast<const int*>(c->spec_done.p + 64 * s);
    const int* c0 = reinterpret_cast<const int*>(c->spec_done.p);
    if (done >= B) { c->rounds_hint = (tail_below >= 0 && c0[6]) ? std::max(1, c0[7]) : rounds; break; }
    if (rounds >= worst) { rc = dsh_fail(c, DSH_ERR_STATE, "batched rounds: a problem did not terminate within its trial budget"); break; }
    group = 2;
  }
  return rc;   // (every stream is idle here: what the caller enqueues on the context's stream is ordered behind all of them)
}

int run_once(dsh_ctx* c) {
  if (c->plan.rounds_mode) return run_rounds(c);
  if (c->plan.K <= 1) {
    LDS_LOCK();
    HIPCHK(c, sft_lm_launch(c->d_probs, c->B, c->plan.max_kd, c->plan.jl_doubles, c->plan.nw, LDS_MARKS(c).lm, c->stream));
    return DSH_OK;
  }
  const int K = c->plan.K, B = c->B;
  HIPCHK(c, hipMemsetAsync(c->d_spec, 0, sizeof(SftSpec) * (size_t)B * K, c->stream));
  const int rounds_per_iter = (10 + K - 1) / K;
  const int worst = c->plan.max_iters_batch * rounds_per_iter;
  // A round = a linearisation launch (verdict on the previous round; on a new iteration the lanes assemble H together) + a trial
  // launch.  First group: as many rounds as the previous run of this context needed (tracking is coherent from frame to frame:
  // usually exact), then the done flags are read back and rounds of two are added while a problem still runs.  Launches behind the
  // end of a problem cost a few microseconds each (it leaves at the first instruction); a read-back costs a stream synchronisation.
  auto launch = [&](int phase) { LDS_LOCK(); return sft_spec_launch(c->d_probs, c->d_spec, B, K, phase, c->plan.nh, c->opt.owner_waves, c->plan.max_kd, c->plan.jl_doubles, LDS_MARKS(c).spec, c->stream); };
  if (c->plan.nh > 0) HIPCHK(c, hipMemsetAsync(c->d_sync, 0, c->layout.sync_total, c->stream));   // progress words and column flags of the helper workgroups: epochs count from here
  HIPCHK(c, launch(SFT_SPEC_INIT));
  int rounds = 0, group = std::max(2, std::min(worst, c->spec_hint));
  HIPCHK(c, c->spec_done.ensure(sizeof(SftSpec) * (size_t)B, true));
  while (true) {
    for (int i = 0; i < group && rounds < worst; i++, rounds++) {
      HIPCHK(c, launch(SFT_SPEC_LIN));
      if (c->plan.any_split) {   // two workgroups per lane: the two parts of the two-sided factorisation, then the solve (reduced problem + own part)
        HIPCHK(c, launch(SFT_SPEC_FACTOR));
        HIPCHK(c, launch(SFT_SPEC_SOLVE));
      }
      HIPCHK(c, launch(SFT_SPEC_TRIAL));
    }
    HIPCHK(c, launch(SFT_SPEC_LIN));   // the verdict on the last round (and, unless the problem is finished, the next linearisation)
    HIPCHK(c, hipMemcpyAsync(c->spec_done.p, c->d_spec, sizeof(SftSpec) * (size_t)B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const SftSpec* sp = reinterpret_cast<const SftSpec*>(c->spec_done.p);
    bool all_done = true;
    int needed = 0;
    for (int b = 0; b < B; b++) { all_done = all_done && sp[b].done; needed = std::max(needed, sp[b].launches); }
    if (all_done) { c->spec_hint = needed; break; }
    if (rounds >= worst) return dsh_fail(c, DSH_ERR_STATE, "speculative trials: a problem did not terminate within its launch budget");
    group = 2;
  }
  return DSH_OK;
}

// ---- upload of a batch: pack, plan (sft_plan.h: sft_plan_batch), layout, binding ------------------------------------------------------

// Where everything of the batch lies in its device arena: a function of the plan and the packed sizes, nothing else.
// [SftDev table][per-frame read-only arrays of every problem] | [result region: B headers, bodies] | [workspace]
SftBatchLayout layout_batch(const SftBatchPlan& plan, const std::vector<Packed>& packed, int B) {
  const int K = plan.K, nh = plan.nh;
  SftBatchLayout L;
  Arena a;
  L.o_tab = a.take(sizeof(SftDev) * B * K);   // lane-major: lane 0 of every problem first
  L.ro.resize(B);
  for (int b = 0; b < B; b++) {
    const dsh::SftFramePack& F = packed[b].f;
    SftBatchLayout::ReadOnly& o = L.ro[b];
    o.obs_nodes = reserve(a, F.obs_nodes); o.obs_bary = reserve(a, F.obs_bary); o.obs_uv = reserve(a, F.obs_uv); o.obs_w = reserve(a, F.obs_w);
    o.ob_ptr = reserve(a, F.ob_ptr); o.ob_m = reserve(a, F.ob_m); o.ob_c = reserve(a, F.ob_c); o.viewed = reserve(a, F.viewed);
    o.xyz_init = reserve(a, F.xyz_init);
    o.pose_init = a.take(8 * 8);
  }
  L.ro_bytes = a.size;
  // result region: every header first (dsh_sft_batch_counts reads only them), then the bodies
  L.res_off = a.size;
  (void)a.take(sizeof(SftResHdr) * (size_t)B);
  L.res_offs.resize(B);
  for (int b = 0; b < B; b++) {
    const SftDev& h = packed[b].h;
    SftBatchLayout::Result& r = L.res_offs[b];
    r.xyz = a.take(8 * 3 * (size_t)h.n) - L.res_off; r.chi2 = a.take(8 * (size_t)h.M) - L.res_off;
    r.trace = a.take(8 * DSH_TRACE_STRIDE * DSH_MAX_ITERS) - L.res_off;
    r.mp = a.take(4 * 3 * (size_t)h.M) - L.res_off; r.outl = a.take((size_t)h.M) - L.res_off;
  }
  L.res_bytes = a.size - L.res_off;
  L.ws.resize((size_t)B * K);
  L.ws_off = a.size;
  L.o_spec = a.take(sizeof(SftSpec) * (size_t)B * K);
  L.o_runs = a.take(plan.rounds_mode ? sizeof(SftRun) * (size_t)B + 64 * kSftMaxSub + sizeof(int) * (size_t)B : 0);
  // (one block: a run clears it with one memset)
  if (nh > 0)
    for (int e = 0; e < B * K; e++) {
      const SftProblemPlan& p = plan.prob[e % B];
      if (p.split) for (int g = 0; g < 2; g++) L.sync_total += Arena::round((size_t)4 * (16 + p.part[g].nT));
    }
  L.o_sync = a.take(L.sync_total);
  size_t sync_used = 0;
  for (int e = 0; e < B * K; e++) {
    const int b = e % B, lane = e / B;
    const SftDev& h = packed[b].h;
    const SftProblemPlan& p = plan.prob[b];
    const size_t Dnp = (size_t)((h.Dn + kNB - 1) / kNB) * kNB;
    SftBatchLayout::Work& w = L.ws[e];
    w.sx0 = a.take(K > 1 ? 8 * 3 * (size_t)h.n : 0); w.sx1 = a.take(K > 1 ? 8 * 3 * (size_t)h.n : 0);
    // lanes > 0 keep their state, errors and pose in the workspace: only lane 0 owns a slot of the result region
    w.shadow_xyz = a.take(lane ? 8 * 3 * (size_t)h.n : 0); w.shadow_chi2 = a.take(lane ? 8 * (size_t)h.M : 0); w.shadow_hdr = a.take(lane ? sizeof(SftResHdr) : 0);
    w.bak = a.take(8 * 3 * (size_t)h.n);
    w.camrec = a.take(8 * (size_t)h.M * SFT_CAM_STRIDE);
    w.wtv = a.take(p.lds_class >= 1 ? 0 : 8 * ((size_t)h.M + 1)); w.Jstar = a.take(p.lds_class >= 1 ? 0 : 8 * 4 * (size_t)h.S);
    w.Anode = a.take(p.lds_class >= 2 ? 0 : 8 * 6 * (size_t)h.nA); w.Jstr = a.take(p.lds_class >= 2 ? 0 : 8 * 4 * (size_t)h.Es);
    // tile mode: BT+1 zero tile rows below the matrix and an 8th (zero) border row + one window of columns let the
    // factorisation load every tile of its sliding window unconditionally (SFT_H_PAD_* in sft_problem.h)
    const size_t band_elems = p.tile_mode ? (Dnp / kTS + SFT_H_PAD_TILE_ROWS) * (size_t)p.tpr * kTS * kTS : Dnp * (size_t)h.ldh;
    const size_t bord_elems = (SFT_BORDER + 1) * Dnp + SFT_H_PAD_BORDER;
    w.Hc = a.take(p.tile_mode == 1 ? 8 * packed[b].g->hc_elems() : 0);
    w.Hb = a.take(p.tile_mode == 1 ? 0 : 8 * band_elems); w.Hbord = a.take(8 * bord_elems); w.Hcn = a.take(8 * 56);
    w.Lb = a.take(8 * band_elems); w.Lbord = a.take(8 * bord_elems); w.Lc = a.take(8 * 56);
    w.Linv = a.take(8 * (Dnp / kTS) * (size_t)kTS * kTS);
    w.Lt = a.take(p.tile_mode == 2 ? 8 * band_elems : 0); w.LbT = a.take(p.tile_mode == 2 ? 8 * (Dnp / kTS) * (size_t)kTS * kTS : 0);
    w.x = a.take(8 * (Dnp + 8)); w.dbg = a.take(1024);
    if (p.split)
      for (int g = 0; g < 4; g++) {   // the band matrices of the two parts and of the reduced problem, twice (H of a part: one copy, lane 0's, shared by the lanes)
        const SftPart& q = p.part[g];
        const size_t tiles = 8 * (size_t)q.nT * q.tpr * kTS * kTS, col = 8 * (size_t)q.nT * kTS * kTS;
        SftBatchLayout::Part& po = w.part[g];
        po.Hb = a.take(g < 2 && lane == 0 ? tiles : 0);
        po.Lb = a.take(tiles); po.Lt = a.take(tiles); po.LbT = a.take(col); po.Linv = a.take(col);
        po.Lbord = a.take(8 * 8 * (size_t)kTS * q.nT); po.x = a.take(8 * ((size_t)kTS * q.nT + 8)); po.xchg = a.take(8 * (size_t)p.sp_xl);
        const bool helped = nh > 0 && g < 2;
        po.Pf = a.take(helped ? tiles : 0); po.PfB = a.take(helped ? col : 0);
        po.sync = L.o_sync + sync_used;
        if (helped) sync_used += Arena::round((size_t)4 * (16 + q.nT));
      }
  }
  L.size = a.size;
  return L;
}

// The read-only arrays of every problem into the staging buffer (lane 0's: the other lanes of a problem read the same ones).
void stage_read_only(char* st, const SftBatchLayout& L, const std::vector<Packed>& packed, int B) {
  for (int b = 0; b < B; b++) {
    const dsh::SftFramePack& F = packed[b].f;
    const SftBatchLayout::ReadOnly& o = L.ro[b];
    put(st, o.obs_nodes, F.obs_nodes); put(st, o.obs_bary, F.obs_bary); put(st, o.obs_uv, F.obs_uv); put(st, o.obs_w, F.obs_w);
    put(st, o.ob_ptr, F.ob_ptr); put(st, o.ob_m, F.ob_m); put(st, o.ob_c, F.ob_c); put(st, o.viewed, F.viewed); put(st, o.xyz_init, F.xyz_init);
    std::memcpy(st + o.pose_init, F.pose_init, 7 * sizeof(double));
  }
}

// The device record of entry e = lane * B + b: the packed scalars, what the plan decided, and every pointer -- template (dt), the graph's
// device block, and the arena at `base` through the layout.  Nothing is dereferenced: address arithmetic on device pointers.
SftDev bind_entry(const std::vector<Packed>& packed, const dsh_ctx::TemplateDev& dt, char* base, const SftBatchLayout& L, const SftBatchPlan& plan, int B, int e) {
  const int b = e % B, lane = e / B;
  const dsh::SftGraph& g = *packed[b].g;
  const SftBatchLayout::ReadOnly& o = L.ro[b];
  const SftBatchLayout::Result& r = L.res_offs[b];
  const SftBatchLayout::Work& w = L.ws[e];
  SftDev h = packed[b].h;
  plan.prob[b].apply(h);
  char* rbase = base + L.res_off;
  SftResHdr* d_hdr = (SftResHdr*)rbase;
  const char* gb = g.d_base;
  h.xyz0 = dt.xyz0; h.nbr_ptr = dt.nbr_ptr; h.nbr_idx = dt.nbr_idx; h.nbr_w = dt.nbr_w; h.nbr_sumw = dt.nbr_sumw; h.k0 = dt.k0;
  h.act = (const int32_t*)(gb + g.o.act); h.actnode = (const int32_t*)(gb + g.o.actnode); h.star_node = (const int32_t*)(gb + g.o.star_node);
  h.star_sL = (const double*)(gb + g.o.star_sL); h.str_nodes = (const int32_t*)(gb + g.o.str_nodes); h.str_L0 = (const double*)(gb + g.o.str_L0);
  h.off_ptr = (const int32_t*)(gb + g.o.off_ptr); h.off_rc = (const int32_t*)(gb + g.o.off_rc); h.sh_ptr = (const int32_t*)(gb + g.o.sh_ptr);
  h.sh_rec = (const uint32_t*)(gb + g.o.sh_rec); h.sh_cf = (const double*)(gb + g.o.sh_cf); h.tmask = (const int32_t*)(gb + g.o.tmask);
  h.hgather = (const uint32_t*)(gb + g.o.hgather);
  h.hgatherT = (const uint32_t*)(gb + g.o.hgatherT);
  h.obs_nodes = (const int32_t*)(base + o.obs_nodes); h.obs_bary = (const double*)(base + o.obs_bary);
  h.obs_uv = (const double*)(base + o.obs_uv); h.obs_w = (const double*)(base + o.obs_w);
  h.ob_ptr = (const int32_t*)(base + o.ob_ptr); h.ob_m = (const int32_t*)(base + o.ob_m); h.ob_c = (const double*)(base + o.ob_c);
  h.viewed = (const uint8_t*)(base + o.viewed);
  h.xyz_init = (const double*)(base + o.xyz_init); h.pose_init = (const double*)(base + o.pose_init);
  h.res = d_hdr + b; h.pose = d_hdr[b].pose;
  h.xyz = (double*)(rbase + r.xyz); h.chi2_obs = (double*)(rbase + r.chi2); h.trace = (double*)(rbase + r.trace);
  h.mappoint = (float*)(rbase + r.mp); h.outlier = (uint8_t*)(rbase + r.outl);
  h.xyz_bak = (double*)(base + w.bak);
  h.camrec = (double*)(base + w.camrec); h.wtv = (double*)(base + w.wtv); h.Anode = (double*)(base + w.Anode);
  h.Jstar = (double*)(base + w.Jstar); h.Jstr = (double*)(base + w.Jstr);
  h.Hc = (double*)(base + w.Hc); h.Hb = (double*)(base + w.Hb); h.Hbord = (double*)(base + w.Hbord); h.Hcorner = (double*)(base + w.Hcn);
  h.Lb = (double*)(base + w.Lb); h.Lbord = (double*)(base + w.Lbord); h.Lcorner = (double*)(base + w.Lc); h.Linv = (double*)(base + w.Linv);
  h.Lt = (double*)(base + w.Lt); h.LbT = (double*)(base + w.LbT);
  h.x = (double*)(base + w.x); h.dbg = (double*)(base + w.dbg);
  h.spec_xyz[0] = (double*)(base + w.sx0); h.spec_xyz[1] = (double*)(base + w.sx1);
  if (h.split)
    for (int g = 0; g < 4; g++) {
      const SftBatchLayout::Part& po = w.part[g];
      SftPart& q = h.part[g];
      q.Hb = g < 2 ? (double*)(base + L.ws[b].part[g].Hb) : (double*)(base + po.xchg);   // a part's H: lane 0's copy, shared by the lanes; reduced problem: H = the summed exchange buffer
      q.Lb = (double*)(base + po.Lb); q.Lt = (double*)(base + po.Lt); q.LbT = (double*)(base + po.LbT); q.Linv = (double*)(base + po.Linv);
      q.Lbord = (double*)(base + po.Lbord); q.x = (double*)(base + po.x); q.xchg = (double*)(base + po.xchg);
      const bool helped = plan.nh > 0 && g < 2;
      q.Pf = helped ? (double*)(base + po.Pf) : nullptr; q.PfB = helped ? (double*)(base + po.PfB) : nullptr;
      q.sync = helped ? (int32_t*)(base + po.sync) : nullptr;
    }
  if (lane) {   // lanes > 0 keep their state, errors and pose in the workspace: only lane 0 owns a slot of the result region
    h.xyz = (double*)(base + w.shadow_xyz); h.chi2_obs = (double*)(base + w.shadow_chi2);
    h.res = (SftResHdr*)(base + w.shadow_hdr); h.pose = ((SftResHdr*)(base + w.shadow_hdr))->pose;
    h.trace = nullptr; h.mappoint = nullptr; h.outlier = nullptr;
    if (h.tile_mode == 1 || h.split) {   // the lanes of a problem assemble one H together (each its share of the block rows) and all factor from it
      const SftBatchLayout::Work& w0 = L.ws[b];
      h.Hc = (double*)(base + w0.Hc); h.Hbord = (double*)(base + w0.Hbord); h.Hcorner = (double*)(base + w0.Hcn);
    }
  }
  return h;
}

// The streams of `want` sub-batches ([0] is the context's; the others are created on first use): how many of them can run.
int sub_streams(dsh_ctx* c, int want) {
  for (int i = 1; i < want; i++)
    if (!c->sub_stream[i] && hipStreamCreateWithFlags(&c->sub_stream[i], hipStreamNonBlocking) != hipSuccess) c->sub_stream[i] = nullptr;
  for (int i = 0; i < want; i++) if (!c->sub_stream[i] || !c->sub_event[0]) return 1;
  return want;
}

}  // namespace

int dsh_sft_upload(dsh_ctx* c, int B, const dsh_sft_frame* frames, SftUploadMode mode) {
  if (!c || B <= 0 || !frames) return dsh_fail(c, DSH_ERR_ARG, "dsh_sft_batch_upload: bad argument");
  if (!c->tmpl.valid) return dsh_fail(c, DSH_ERR_STATE, "dsh_sft_batch_upload: no template");
  if (!c->host_only) (void)hipSetDevice(c->device);
  c->B = 0;
  c->ran = false;
  c->upload_serial++;
  if ((int)c->packed.size() != B) c->packed.resize(B);   // the vectors inside keep their capacity from frame to frame
  std::vector<SftSizes> sizes(B);
  for (int b = 0; b < B; b++) {
    std::string e;
    const int rc = pack_problem(c, frames[b], c->packed[b], e);
    if (rc != DSH_OK) return dsh_fail(c, rc, "problem " + std::to_string(b) + ": " + e);
    const SftDev& h = c->packed[b].h;
    sizes[b] = SftSizes{h.n, h.nA, h.Dn, h.kd, h.M, h.S, h.Es, h.max_iters};
  }
  SftBatchPlan plan = sft_plan_batch(sizes.data(), B, c->num_cus, c->opt, c->host_only, mode);
  if (c->host_only) {  // packed on the host only; dsh_sft_batch_problem_info works, running does not
    c->h_probs.resize(B);
    for (int b = 0; b < B; b++) { c->h_probs[b] = c->packed[b].h; plan.prob[b].apply(c->h_probs[b]); }
    c->plan = std::move(plan);
    c->B = B;
    return DSH_OK;
  }
  if (sft_lm_kernel_lds_bytes(plan.max_kd, plan.jl_doubles) > 160 * 1024 || plan.max_kd + kNB + SFT_BORDER > SFT_NT)
    return dsh_fail(c, DSH_ERR_ARG, "half-bandwidth too large for the LDS panel / workgroup");
  if (plan.n_sub > 1) plan.n_sub = sub_streams(c, plan.n_sub);
  SftBatchLayout L = layout_batch(plan, c->packed, B);
  bool fresh_arena = false;
  if (L.size > c->d_batch_cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->d_batch) { (void)hipFree(c->d_batch); c->d_batch = nullptr; c->d_batch_cap = 0; }
    HIPCHK(c, hipMalloc((void**)&c->d_batch, L.size));
    c->d_batch_cap = L.size;
    fresh_arena = true;
  }
  // the staging buffer of the previous upload may still be read by its copy
  if (c->stage_busy) { HIPCHK(c, hipEventSynchronize(c->stage_free)); c->stage_busy = false; }
  HIPCHK(c, c->stage.ensure(L.ro_bytes, true));
  char* st = c->stage.p;
  char* base = c->d_batch;
  const size_t entries = (size_t)B * plan.K;
  c->h_probs.resize(entries);
  for (size_t e = 0; e < entries; e++) c->h_probs[e] = bind_entry(c->packed, c->dt, base, L, plan, B, (int)e);
  std::memcpy(st + L.o_tab, c->h_probs.data(), sizeof(SftDev) * entries);
  stage_read_only(st, L, c->packed, B);
  HIPCHK(c, hipMemcpyAsync(base, st, L.ro_bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(c->stage_free, c->stream));
  c->stage_busy = true;
  // The kernel initialises everything it reads (state, H with its zero padding, border, x, counters).  A fresh allocation
  // is cleared once; after that the workspace holds whatever the previous batch left -- including the NaN tiles of L of a
  // failed factorisation (every pivot behind a non-positive one is NaN, and the factorisation goes on storing).  So no
  // result may depend on what a tile held before this batch wrote it: tests/test_factor_waves_gpu.py runs a healthy batch on
  // the workspace of a failing one and compares it with a fresh context bit for bit.  The result region is always cleared
  // (a caller that downloads without running gets zeros, not the previous batch).
  if (fresh_arena) HIPCHK(c, hipMemsetAsync(base + L.ws_off, 0, L.size - L.ws_off, c->stream));
  HIPCHK(c, hipMemsetAsync(base + L.res_off, 0, L.res_bytes, c->stream));
  // commit: from here on the run, download and info functions see this batch
  c->d_probs = (SftDev*)(base + L.o_tab);
  c->d_spec = (SftSpec*)(base + L.o_spec);
  c->d_runs = (SftRun*)(base + L.o_runs);
  c->d_counters = (int*)(base + L.o_runs + sizeof(SftRun) * (size_t)B);
  c->d_linlist = c->d_counters + 16 * kSftMaxSub;
  c->d_sync = base + L.o_sync;
  c->plan = std::move(plan);
  c->layout = std::move(L);
  c->B = B;
  return DSH_OK;   // asynchronous: the launch of dsh_sft_batch_run is ordered behind the copy on the same stream (dsh_sft_batch_run itself BLOCKS in the
                   // latency mode and in the rounds of phase kernels: it reads done flags / counters back between groups of launches)
}

extern "C" {

int dsh_create(dsh_ctx** out, int device) {
  if (!out) return DSH_ERR_ARG;
  *out = nullptr;
  if (device == -1) {  // host-only context: template constants + packing, every GPU entry point fails loudly
    dsh_ctx* hc = new dsh_ctx();
    hc->device = -1;
    hc->host_only = true;
    *out = hc;
    return DSH_OK;
  }
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return DSH_ERR_NO_DEVICE;
  if (device < 0 || device >= count) return DSH_ERR_ARG;
  dsh_ctx* c = new dsh_ctx();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return DSH_ERR_HIP;
  }
  if (hipEventCreateWithFlags(&c->stage_free, hipEventDisableTiming) != hipSuccess) {
    (void)hipStreamDestroy(c->stream);
    delete c;
    return DSH_ERR_HIP;
  }
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->num_cus = cus;
  // streams of the sub-batches of the throughput shape: [0] is the context's stream; the others are created when a batch is first split (the
  // lab option "streams": measured and not the default).  Not before: HIP multiplexes the streams of a process onto four hardware queues, and a
  // context that holds three idle streams pushes the streams of OTHER contexts onto shared queues -- the two contexts of a connected-mesh or
  // shared-camera group then ran their phase kernels one after the other (17.5 instead of 9.5 ms per C2 frame next to a third context).
  c->sub_stream[0] = c->stream;
  if (hipEventCreateWithFlags(&c->sub_event[0], hipEventDisableTiming) != hipSuccess) c->sub_event[0] = nullptr;
  *out = c;
  return DSH_OK;
}

int dsh_destroy(dsh_ctx* c) {
  if (!c) return DSH_ERR_ARG;
  dsh_detach_stores(c);   // its stores stay valid objects (dsh_diffdb_destroy / dsh_kfdb_destroy still free them) but no longer name it
  if (c->host_only) { c->stage.release(); c->results.release(); delete c; return DSH_OK; }
  (void)hipSetDevice(c->device);
  drop_graphs(c);
  for (int i = 1; i < kSftMaxSub; i++) if (c->sub_stream[i]) { (void)hipStreamSynchronize(c->sub_stream[i]); (void)hipStreamDestroy(c->sub_stream[i]); }
  for (int i = 0; i < kSftMaxSub; i++) if (c->sub_event[i]) (void)hipEventDestroy(c->sub_event[i]);
  if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
  if (c->stage_free) (void)hipEventDestroy(c->stage_free);
  c->stage.release();
  c->results.release();
  c->spec_done.release();
  if (c->d_tmpl) (void)hipFree(c->d_tmpl);
  c->scratch.release();
  c->pin_in.release();
  c->pin_out.release();
  if (c->d_batch) (void)hipFree(c->d_batch);
  if (c->d_sc) (void)hipFree(c->d_sc);
  delete c;
  return DSH_OK;
}

const char* dsh_last_error(const dsh_ctx* c) { return c ? c->err.c_str() : "null context"; }
void* dsh_stream(dsh_ctx* c) { return c ? (void*)c->stream : nullptr; }
int dsh_synchronize(dsh_ctx* c) {
  if (const int rc = dsh_enter(c, "dsh_synchronize")) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return DSH_OK;
}

int dsh_template_build(dsh_ctx* c, int n, const double* xyz0, int F, const int32_t* facets) {
  if (!c || n <= 0 || F <= 0 || !xyz0 || !facets) return dsh_fail(c, DSH_ERR_ARG, "dsh_template_build: bad argument");
  for (int i = 0; i < 3 * F; i++)
    if (facets[i] < 0 || facets[i] >= n) return dsh_fail(c, DSH_ERR_ARG, "dsh_template_build: facet index out of range");
  if (!c->host_only) (void)hipSetDevice(c->device);
  c->tmpl.build(n, xyz0, F, facets);
  return upload_template(c);
}

int dsh_template_set(dsh_ctx* c, int n, const double* xyz0, const uint8_t* boundary, const int32_t* rp, const int32_t* col, const double* w,
                     const double* k0, int E, const int32_t* en, const double* eL, double median_L) {
  if (!c || n <= 0 || E < 0 || !xyz0 || !boundary || !rp || !col || !w || !k0 || !en || !eL) return dsh_fail(c, DSH_ERR_ARG, "dsh_template_set: bad argument");
  // The arrays become indices of the packer (inc[edge_nodes[..]], opt[nbr_col[..]]): a malformed CSR or edge list must be
  // refused here, not turn into an out-of-bounds write later.
  if (rp[0] != 0) return dsh_fail(c, DSH_ERR_ARG, "dsh_template_set: nbr_rowptr[0] != 0");
  for (int i = 0; i < n; i++)
    if (rp[i + 1] < rp[i]) return dsh_fail(c, DSH_ERR_ARG, "dsh_template_set: nbr_rowptr is not non-decreasing");
  for (int p = 0; p < rp[n]; p++)
    if (col[p] < 0 || col[p] >= n) return dsh_fail(c, DSH_ERR_ARG, "dsh_template_set: neighbour index out of range");
  for (int e = 0; e < E; e++) {
    if (en[2 * e] < 0 || en[2 * e] >= n || en[2 * e + 1] < 0 || en[2 * e + 1] >= n) return dsh_fail(c, DSH_ERR_ARG, "dsh_template_set: edge node out of range");
    if (!(eL[e] > 0.0)) return dsh_fail(c, DSH_ERR_ARG, "dsh_template_set: edge rest length must be positive");
  }
  if (!(median_L > 0.0)) return dsh_fail(c, DSH_ERR_ARG, "dsh_template_set: median edge length must be positive");
  if (!c->host_only) (void)hipSetDevice(c->device);
  c->tmpl.set(n, xyz0, boundary, rp, col, w, k0, E, en, eL, median_L);
  return upload_template(c);
}

int dsh_template_dims(const dsh_ctx* c, int32_t* n, int32_t* E, int32_t* nnz) {
  if (!c || !c->tmpl.valid) return DSH_ERR_STATE;
  if (n) *n = c->tmpl.n;
  if (E) *E = c->tmpl.E;
  if (nnz) *nnz = (int32_t)c->tmpl.nbr_idx.size();
  return DSH_OK;
}

int dsh_template_get(const dsh_ctx* c, uint8_t* boundary, int32_t* rp, int32_t* col, double* w, double* k0, int32_t* en, double* eL, double* med) {
  if (!c || !c->tmpl.valid) return DSH_ERR_STATE;
  const dsh::TemplateHost& t = c->tmpl;
  if (boundary) std::memcpy(boundary, t.boundary.data(), t.n);
  if (rp) std::memcpy(rp, t.nbr_ptr.data(), sizeof(int32_t) * (t.n + 1));
  if (col) std::memcpy(col, t.nbr_idx.data(), sizeof(int32_t) * t.nbr_idx.size());
  if (w) std::memcpy(w, t.nbr_w.data(), sizeof(double) * t.nbr_w.size());
  if (k0) std::memcpy(k0, t.k0.data(), sizeof(double) * t.n);
  if (en) std::memcpy(en, t.edge_nodes.data(), sizeof(int32_t) * 2 * t.E);
  if (eL) std::memcpy(eL, t.edge_L0.data(), sizeof(double) * t.E);
  if (med) *med = t.median_L;
  return DSH_OK;
}

int dsh_template_embed(const dsh_ctx* c, int P, const float* pts, int32_t* facet_id, int32_t* nodes, float* bary) {
  if (!c || !c->tmpl.valid || c->tmpl.F <= 0) return DSH_ERR_STATE;
  if (P < 0 || !pts || !facet_id || !nodes || !bary) return DSH_ERR_ARG;
  c->tmpl.embed(P, pts, facet_id, nodes, bary);
  return DSH_OK;
}

int dsh_template_embed_device(dsh_ctx* c, int P, const float* pts, int32_t* facet_id, int32_t* nodes, float* bary) {
  if (!c) return DSH_ERR_ARG;
  if (!c->tmpl.valid || c->tmpl.F <= 0) return dsh_fail(c, DSH_ERR_STATE, "dsh_template_embed_device: needs a template built from facets");
  if (P < 0 || (P > 0 && (!pts || !facet_id || !nodes || !bary))) return dsh_fail(c, DSH_ERR_ARG, "dsh_template_embed_device: bad argument");
  if (c->host_only) return dsh_fail(c, DSH_ERR_NO_DEVICE, "dsh_template_embed_device: host-only context, no GPU (dsh_template_embed is the host routine)");
  if (P == 0) return DSH_OK;
  if (const int rc = dsh_enter(c, "dsh_template_embed_device")) return rc;
  const dsh::TemplateHost& t = c->tmpl;
  const size_t Pz = (size_t)P;
  UpBlock up;   // the points and the template's nodes, facets and node-to-facet lists
  const size_t o_pts = up.copy_of(pts, 12 * Pz), o_xyz = up.copy_of(t.xyz0.data(), 24 * (size_t)t.n), o_fac = up.copy_of(t.facets.data(), 12 * (size_t)t.F),
               o_ptr = up.copy_of(t.nf_ptr.data(), 4 * (size_t)(t.n + 1)), o_idx = up.copy_of(t.nf_idx.data(), 4 * t.nf_idx.size());
  DownBlock down;
  const size_t d_fid = down.copy_to(facet_id, 4 * Pz), d_nodes = down.copy_to(nodes, 12 * Pz), d_bary = down.copy_to(bary, 12 * Pz);
  if (const int rc = up.copy(c)) return rc;
  if (const int rc = down.alloc(c)) return rc;
  HIPCHK(c, reg_embed(P, up.dev<float>(o_pts), t.n, up.dev<double>(o_xyz), up.dev<int32_t>(o_fac), up.dev<int32_t>(o_ptr), up.dev<int32_t>(o_idx),
                      down.dev<int32_t>(d_fid), down.dev<int32_t>(d_nodes), down.dev<float>(d_bary), c->stream));
  return down.receive(c);
}

int dsh_sft_batch_upload(dsh_ctx* c, int B, const dsh_sft_frame* frames) { return dsh_sft_upload(c, B, frames, SftUploadMode::batch); }

int dsh_sft_batch_run(dsh_ctx* c) {
  if (!c) return DSH_ERR_ARG;
  if (const int rc = dsh_enter(c, "dsh_sft_batch_run")) return rc;
  if (c->B <= 0) return dsh_fail(c, DSH_ERR_STATE, "dsh_sft_batch_run: nothing uploaded");
  const int rc = run_once(c);
  if (rc != DSH_OK) return rc;
  c->ran = true;
  return DSH_OK;
}

int dsh_sft_batch_counts(dsh_ctx* c, int64_t* iters, int64_t* trials) {
  if (!c || c->B <= 0 || !c->ran) return DSH_ERR_STATE;
  if (const int rc = dsh_enter(c, "dsh_sft_batch_counts")) return rc;
  // one copy of the B result headers (they are contiguous), ordered behind the run on the context's stream
  const size_t bytes = sizeof(SftResHdr) * (size_t)c->B;
  HIPCHK(c, c->results.ensure(std::max(bytes, c->results.cap), true));
  HIPCHK(c, hipMemcpyAsync(c->results.p, c->d_batch + c->layout.res_off, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const SftResHdr* hd = reinterpret_cast<const SftResHdr*>(c->results.p);
  int64_t it = 0, tr = 0;
  for (int b = 0; b < c->B; b++) { it += hd[b].iters; tr += hd[b].trials; }
  if (iters) *iters = it;
  if (trials) *trials = tr;
  return DSH_OK;
}

int dsh_sft_batch_problem_info(dsh_ctx* c, int b, int64_t* bytes, int32_t* counts) {
  if (!c || b < 0 || b >= c->B) return DSH_ERR_ARG;
  const Packed& P = c->packed[b];
  const SftDev& h = P.h;
  // materialised-Jacobian convention, reference edge counts (curvature unfused)
  const int64_t M = h.M, n = h.n, C = P.g->n_curv_ref, E = h.Es, V = h.V;
  const int64_t reads = 60 * M + 24 * n + 88 + 92 * C + 16 * E + 28 * V;
  const int64_t writes = 8 * (30 * M + 21 * C + 6 * E + 9 * V) + 8 * (2 * M + C + E + 3 * V) + 8 * M;
  if (bytes) *bytes = reads + writes;
  if (counts) { counts[0] = h.M; counts[1] = h.nA; counts[2] = P.g->n_curv_ref; counts[3] = h.Es; counts[4] = h.V; counts[5] = 6 + h.Dn; counts[6] = h.kd; counts[7] = c->plan.rounds_mode ? 1 : c->plan.nw; counts[8] = P.g->noff; }
  return DSH_OK;
}

int dsh_sft_batch_download(dsh_ctx* c, int B, dsh_sft_result* res) {
  if (!c || !res || B != c->B) return dsh_fail(c, DSH_ERR_ARG, "dsh_sft_batch_download: bad argument");
  if (const int rc = dsh_enter(c, "dsh_sft_batch_download")) return rc;
  if (!c->ran) return dsh_fail(c, DSH_ERR_STATE, "dsh_sft_batch_download: no run");
  // the whole result region (headers + bodies of every problem) in ONE copy into page-locked memory
  HIPCHK(c, c->results.ensure(c->layout.res_bytes, true));
  HIPCHK(c, hipMemcpyAsync(c->results.p, c->d_batch + c->layout.res_off, c->layout.res_bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const char* rb = c->results.p;
  const SftResHdr* hd = reinterpret_cast<const SftResHdr*>(rb);
  for (int b = 0; b < B; b++) {
    const SftDev& h = c->h_probs[b];
    const Packed& P = c->packed[b];
    const SftBatchLayout::Result& o = c->layout.res_offs[b];
    dsh_sft_result& r = res[b];
    r.rep_error = hd[b].rep_error;
    r.inliers = hd[b].inliers;
    r.iters = hd[b].iters;
    r.trials = hd[b].trials;
    r.status = hd[b].status;
    r.dim = 6 + h.Dn;
    r.half_bandwidth = h.kd;
    if (r.chi2_obs) std::memcpy(r.chi2_obs, rb + o.chi2, 8 * (size_t)h.M);
    if (r.outlier) std::memcpy(r.outlier, rb + o.outl, (size_t)h.M);
    if (r.xyz) std::memcpy(r.xyz, rb + o.xyz, 8 * 3 * (size_t)h.n);
    if (r.pose7) std::memcpy(r.pose7, hd[b].pose, 8 * 7);
    if (r.Tcw) Tcw_from_pose7(hd[b].pose, r.Tcw);
    if (r.mappoint_xyz) std::memcpy(r.mappoint_xyz, rb + o.mp, 4 * 3 * (size_t)h.M);
    if (r.trace) {   // rows of the executed iterations, zeros behind them
      const size_t rows = (size_t)std::max(P.f.max_iters, 0), done = std::min(rows, (size_t)std::max(hd[b].iters, 0));
      std::memcpy(r.trace, rb + o.trace, 8 * DSH_TRACE_STRIDE * done);
      std::memset(r.trace + DSH_TRACE_STRIDE * done, 0, 8 * DSH_TRACE_STRIDE * (rows - done));
    }
  }
  return DSH_OK;
}

int dsh_sft_solve(dsh_ctx* c, const dsh_sft_frame* frame, dsh_sft_result* result) {
  if (!c || !frame || !result) return dsh_fail(c, DSH_ERR_ARG, "dsh_sft_solve: bad argument");
  int rc = dsh_sft_batch_upload(c, 1, frame);
  if (rc != DSH_OK) return rc;
  rc = dsh_sft_batch_run(c);
  if (rc != DSH_OK) return rc;
  return dsh_sft_batch_download(c, 1, result);
}

#ifdef DSH_LAB
// ---- lab entry points (include/defslam_hip_debug.h): libdefslam_hip_lab.so only ----------------------------------------
namespace {
struct EventPair {   // destroyed on every path
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t create() { hipError_t e = hipEventCreate(&e0); return e != hipSuccess ? e : hipEventCreate(&e1); }
  ~EventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};
}  // namespace

int dsh_lab_set_option(dsh_ctx* c, const char* name, int value) {
  if (!c || !name) return DSH_ERR_ARG;
  const std::string k(name);
  if (k == "waves") { if (value != 0 && value != 4 && value != 8) return dsh_fail(c, DSH_ERR_ARG, "dsh_lab_set_option: waves is 0 (automatic), 4 or 8"); c->opt.waves = value; }
  else if (k == "dataflow") c->opt.dataflow = value != 0;
  else if (k == "wide_off") c->opt.wide_off = value != 0;
  else if (k == "rounds") c->opt.rounds = value != 0;
  else if (k == "streams") { if (value < 0 || value > kSftMaxSub) return dsh_fail(c, DSH_ERR_ARG, "dsh_lab_set_option: streams is 0 (automatic) or 1..4 sub-batches"); c->opt.streams = value; }
  else if (k == "split") { if (value < 0 || value > 2) return dsh_fail(c, DSH_ERR_ARG, "dsh_lab_set_option: split is 0 (off), 1 (wide bands only) or 2 (every band long enough)"); c->opt.split = value; }
  else if (k == "helpers_wbt") { if (value < 1 || value > 16) return dsh_fail(c, DSH_ERR_ARG, "dsh_lab_set_option: helpers_wbt is 1..16 (tiles of half-bandwidth from which parts get helper workgroups)"); c->opt.helpers_wbt = value; }
  else if (k == "owner_waves") { if (value != 8 && value != 16) return dsh_fail(c, DSH_ERR_ARG, "dsh_lab_set_option: owner_waves is 8 or 16 (wavefronts of a FACTOR workgroup with helpers)"); c->opt.owner_waves = value; }
  else if (k == "helpers") { if (value < -1 || value > 3) return dsh_fail(c, DSH_ERR_ARG, "dsh_lab_set_option: helpers is -1 (automatic) or 0..3 workgroups per part"); c->opt.helpers = value; }
  else if (k == "tail") { if (value < -1 || value > 8) return dsh_fail(c, DSH_ERR_ARG, "dsh_lab_set_option: tail is -1 (automatic), 0 (rounds to the end) or the number of problems per CU from which downwards the last problems go to the tail kernel"); c->opt.tail = value; }
  else if (k == "speculate") { if (value < 0 || value > SFT_SPEC_MAXK) return dsh_fail(c, DSH_ERR_ARG, "dsh_lab_set_option: speculate is 0 (automatic) or 1..4 lanes"); c->opt.speculate = value; }
  else return dsh_fail(c, DSH_ERR_ARG, "dsh_lab_set_option: unknown option " + k);
  return DSH_OK;
}

int dsh_lab_sft_solver_info(dsh_ctx* c, int b, int32_t* out8) {
  if (!c || !out8 || b < 0 || b >= c->B) return dsh_fail(c, DSH_ERR_ARG, "dsh_lab_sft_solver_info: bad argument");
  const SftDev& h = c->h_probs[b];
  out8[0] = h.split; out8[1] = h.sp_c0; out8[2] = h.sp_s; out8[3] = h.sp_n1p; out8[4] = h.sp_pad; out8[5] = c->plan.K; out8[6] = h.tile_mode; out8[7] = c->plan.nw;
  return DSH_OK;
}

int dsh_lab_sft_run_timed(dsh_ctx* c, int launches, double* total_ms) {
  if (!c || launches <= 0 || !total_ms) return dsh_fail(c, DSH_ERR_ARG, "dsh_lab_sft_run_timed: bad argument");
  if (const int rc = dsh_enter(c, "dsh_lab_sft_run_timed")) return rc;
  if (c->B <= 0) return dsh_fail(c, DSH_ERR_STATE, "dsh_lab_sft_run_timed: nothing uploaded");
  EventPair ev;
  HIPCHK(c, ev.create());
  HIPCHK(c, hipEventRecord(ev.e0, c->stream));
  for (int i = 0; i < launches; i++) { const int rc = run_once(c); if (rc != DSH_OK) return rc; }
  HIPCHK(c, hipEventRecord(ev.e1, c->stream));
  HIPCHK(c, hipEventSynchronize(ev.e1));
  float ms = 0.f;
  HIPCHK(c, hipEventElapsedTime(&ms, ev.e0, ev.e1));
  *total_ms = (double)ms;
  c->ran = true;
  return DSH_OK;
}

int dsh_lab_sft_assemble_timed(dsh_ctx* c, int launches, double* total_ms) {
  if (!c || launches <= 0 || !total_ms) return dsh_fail(c, DSH_ERR_ARG, "dsh_lab_sft_assemble_timed: bad argument");
  if (const int rc = dsh_enter(c, "dsh_lab_sft_assemble_timed")) return rc;
  if (c->B <= 0 || !c->ran) return dsh_fail(c, DSH_ERR_STATE, "dsh_lab_sft_assemble_timed: needs an uploaded batch that has run once");
  EventPair ev;
  HIPCHK(c, ev.create());
  HIPCHK(c, hipEventRecord(ev.e0, c->stream));
  for (int i = 0; i < launches; i++) HIPCHK(c, sft_assembly_launch(c->d_probs, c->B, c->plan.max_kd, c->plan.jl_doubles, c->plan.rounds_mode ? 8 : c->plan.nw, c->stream));
  HIPCHK(c, hipEventRecord(ev.e1, c->stream));
  HIPCHK(c, hipEventSynchronize(ev.e1));
  float ms = 0.f;
  HIPCHK(c, hipEventElapsedTime(&ms, ev.e0, ev.e1));
  *total_ms = ms;
  c->ran = false;   // results of the last full run are gone (state reset, H reassembled at the initial state)
  return DSH_OK;
}

int dsh_lab_sft_wave_check(dsh_ctx* c, double rel, int launches, int only, double* x_ref, double* x_new, int32_t* ok2, double* ms2) {
  if (!c || launches <= 0 || !ms2) return dsh_fail(c, DSH_ERR_ARG, "dsh_lab_sft_wave_check: bad argument");
  if (const int rc = dsh_enter(c, "dsh_lab_sft_wave_check")) return rc;
  if (c->B <= 0 || !c->ran) return dsh_fail(c, DSH_ERR_STATE, "dsh_lab_sft_wave_check: needs an uploaded batch that has run once");
  for (int b = 0; b < c->B; b++)
    if (c->h_probs[b].tile_mode != 1) return dsh_fail(c, DSH_ERR_STATE, "dsh_lab_sft_wave_check: register-window problems (half-bandwidth <= 128) only");
  HIPCHK(c, sft_assembly_launch(c->d_probs, c->B, c->plan.max_kd, c->plan.jl_doubles, c->plan.rounds_mode ? 8 : c->plan.nw, c->stream));   // H of the initial state
  EventPair ev;
  HIPCHK(c, ev.create());
  for (int which = 0; which < 2; which++) {
    if (only == 2 - which) continue;   // only = 1: the four-wavefront solver alone, 2: the one-wavefront solver alone (lambda of the last reference run)
    HIPCHK(c, sft_wave_lab_launch(c->d_probs, c->B, which, rel, c->plan.max_kd, c->plan.jl_doubles, c->stream));   // (also the warm-up)
    HIPCHK(c, hipEventRecord(ev.e0, c->stream));
    for (int i = 0; i < launches; i++) HIPCHK(c, sft_wave_lab_launch(c->d_probs, c->B, which, rel, c->plan.max_kd, c->plan.jl_doubles, c->stream));
    HIPCHK(c, hipEventRecord(ev.e1, c->stream));
    HIPCHK(c, hipEventSynchronize(ev.e1));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev.e0, ev.e1));
    ms2[which] = (double)ms / launches;
    double* dst = which == 0 ? x_ref : x_new;
    size_t off = 0;
    for (int b = 0; b < c->B; b++) {
      const SftDev& h = c->h_probs[b];
      const size_t Dnp = (size_t)((h.Dn + kNB - 1) / kNB) * kNB;
      if (dst) HIPCHK(c, hipMemcpy(dst + off, h.x, 8 * (Dnp + 6), hipMemcpyDeviceToHost));
      off += Dnp + 6;
      double flag = 0.0;
      if (ok2) { HIPCHK(c, hipMemcpy(&flag, h.dbg + 2, 8, hipMemcpyDeviceToHost)); ok2[2 * b + which] = (int32_t)flag; }
    }
  }
  return DSH_OK;   // (H stays assembled at the initial state: the check can be repeated; the results of the last full run are stale)
}

int dsh_lab_sft_factor_check(dsh_ctx* c, const double* lambda, const uint8_t* factor, int grid, double* x, int32_t* ok) {
  if (!c || !lambda || grid < 0) return dsh_fail(c, DSH_ERR_ARG, "dsh_lab_sft_factor_check: bad argument");
  if (const int rc = dsh_enter(c, "dsh_lab_sft_factor_check")) return rc;
  if (c->B <= 0 || !c->ran) return dsh_fail(c, DSH_ERR_STATE, "dsh_lab_sft_factor_check: needs an uploaded batch that has run once");
  for (int b = 0; b < c->B; b++)
    if (c->h_probs[b].tile_mode != 1) return dsh_fail(c, DSH_ERR_STATE, "dsh_lab_sft_factor_check: register-window problems (half-bandwidth <= 128) only");
  const int B = c->B;
  // run records and counters of its own: the batch need not be in the throughput shape (the records of the rounds exist only there)
  struct OwnedDevBuf { void* p = nullptr; ~OwnedDevBuf() { if (p) (void)hipFree(p); } } runs, counters;
  HIPCHK(c, hipMalloc(&runs.p, sizeof(SftRun) * (size_t)B));
  HIPCHK(c, hipMalloc(&counters.p, 16 * sizeof(int)));
  std::vector<SftRun> h_runs(B);
  for (int b = 0; b < B; b++) {
    SftRun& R = h_runs[b];
    std::memset(&R, 0, sizeof(R));
    R.lambda = lambda[b];
    R.state = (!factor || factor[b]) ? SFTB_TRIAL : SFTB_DONE;
    R.fact_ok = -1;   // stays -1 where the problem was left out
  }
  HIPCHK(c, sft_assembly_launch(c->d_probs, B, c->plan.max_kd, c->plan.jl_doubles, c->plan.rounds_mode ? 8 : c->plan.nw, c->stream));   // H of the initial state
  for (int b = 0; b < B; b++) HIPCHK(c, hipMemcpyAsync(c->h_probs[b].dbg + 1, &lambda[b], sizeof(double), hipMemcpyHostToDevice, c->stream));   // for wave_check(only = 2)
  HIPCHK(c, hipMemcpyAsync(runs.p, h_runs.data(), sizeof(SftRun) * (size_t)B, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(counters.p, 0, 16 * sizeof(int), c->stream));
  HIPCHK(c, sftb_factor_lab_launch(c->d_probs, (SftRun*)runs.p, (int*)counters.p, B, grid ? grid : std::min(B, 4 * c->num_cus), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(h_runs.data(), runs.p, sizeof(SftRun) * (size_t)B, hipMemcpyDeviceToHost));
  size_t off = 0;
  for (int b = 0; b < B; b++) {
    const SftDev& h = c->h_probs[b];
    const size_t Dnp = (size_t)((h.Dn + kNB - 1) / kNB) * kNB;
    if (x) HIPCHK(c, hipMemcpy(x + off, h.x, 8 * (Dnp + 6), hipMemcpyDeviceToHost));
    off += Dnp + 6;
    if (ok) ok[b] = h_runs[b].fact_ok;
  }
  return DSH_OK;   // (H stays assembled at the initial state, as after dsh_lab_sft_wave_check; the results of the last full run are stale)
}

int dsh_lab_sft_rounds_timed(dsh_ctx* c, double* ms4, int32_t* rounds) {
  if (!c || !ms4) return dsh_fail(c, DSH_ERR_ARG, "dsh_lab_sft_rounds_timed: bad argument");
  if (const int rc = dsh_enter(c, "dsh_lab_sft_rounds_timed")) return rc;
  if (c->B <= 0 || !c->plan.rounds_mode) return dsh_fail(c, DSH_ERR_STATE, "dsh_lab_sft_rounds_timed: needs an uploaded batch that runs as rounds of phase kernels");
  std::vector<hipEvent_t> ev;
  c->phase_events = &ev;
  c->phase_ids.clear();
  const int rc = run_rounds(c);
  c->phase_events = nullptr;
  (void)hipStreamSynchronize(c->stream);
  // launches by phase: ms[0] INIT, [1] LIN, [2] FACTOR, [3] TRIAL, [4] the tail kernel; [5] = factorisations done by the FACTOR launches, [6] = linearisations done by the LIN launches
  for (int i = 0; i < 7; i++) ms4[i] = 0.0;
  { int32_t cnt[16] = {0}; if (hipMemcpy(cnt, c->d_counters, sizeof(cnt), hipMemcpyDeviceToHost) == hipSuccess) { ms4[5] = (double)cnt[8]; ms4[6] = (double)cnt[9]; } }
  int n_trial = 0;
  for (size_t i = 0; i + 1 < ev.size(); i += 2) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
    const int ph = c->phase_ids[i / 2];
    ms4[ph == SFTB_PH_INIT ? 0 : ph == SFTB_PH_LIN ? 1 : ph == SFTB_PH_FACTOR ? 2 : ph == SFTB_PH_TRIAL ? 3 : 4] += ms;
    n_trial += ph == SFTB_PH_TRIAL;
  }
  if (rounds) *rounds = n_trial;
  for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  if (rc == DSH_OK) c->ran = true;
  return rc;
}

int dsh_lab_sft_dump(dsh_ctx* c, int b, int what, int64_t n, double* out) {
  if (!c || !out || b < 0 || b >= c->B || n <= 0) return dsh_fail(c, DSH_ERR_ARG, "dsh_lab_sft_dump: bad argument");
  if (const int rc = dsh_enter(c, "dsh_lab_sft_dump")) return rc;
  const SftDev& h = c->h_probs[b];
  const double* src = what == 0 ? h.Lb : what == 1 ? h.Linv : what == 2 ? h.Lbord : what == 3 ? h.Hc : what == 4 ? h.Hbord : what == 5 ? h.x : what == 6 ? h.Hcorner :
                      (what == 8 || what == 9) ? (const double*)h.part[what - 8].sync : h.dbg;   // 8, 9: the helper statistics of part 0 / 1 (int32 words)
  if (!src) return dsh_fail(c, DSH_ERR_STATE, "dsh_lab_sft_dump: the problem has no such buffer");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, src, 8 * (size_t)n, hipMemcpyDeviceToHost));
  return DSH_OK;
}

int dsh_lab_sft_phase_ms(dsh_ctx* c, int b, double* out8) {
  if (!c || !out8 || b < 0 || b >= c->B) return dsh_fail(c, DSH_ERR_ARG, "dsh_lab_sft_phase_ms: bad argument");
  if (const int rc = dsh_enter(c, "dsh_lab_sft_phase_ms")) return rc;
  if (!c->ran) return dsh_fail(c, DSH_ERR_STATE, "dsh_lab_sft_phase_ms: no run");
#ifndef SFT_PHASE_TIMERS
  return dsh_fail(c, DSH_ERR_STATE, "dsh_lab_sft_phase_ms: this build has no phase timers (make lab EXTRA=-DSFT_PHASE_TIMERS)");
#else
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out8, c->h_probs[b].dbg, 8 * sizeof(double), hipMemcpyDeviceToHost));
  for (int i = 0; i < 8; i++) out8[i] *= 1e-5;  // 100 MHz ticks -> ms
  {   // sections of the assembly (shader-clock cycles of wave 0), printed for tuning runs
    double as[6];
    HIPCHK(c, hipMemcpy(as, c->h_probs[b].dbg + 32, sizeof(as), hipMemcpyDeviceToHost));
    std::fprintf(stderr, "[lab] assembly sections of problem %d, kcycles of wave 0: corner %.0f, diagonal gather %.0f, butterfly+finish %.0f, off-diagonal %.0f, round overhead %.0f; rounds %.0f\n",
                 b, as[0] * 1e-3, as[1] * 1e-3, as[2] * 1e-3, as[3] * 1e-3, as[4] * 1e-3, as[5]);
  }
  return DSH_OK;
#endif
}

int dsh_lab_sft_step_trace(dsh_ctx* c, int b, double* out64) {
  if (!c || !out64 || b < 0 || b >= c->B) return dsh_fail(c, DSH_ERR_ARG, "dsh_lab_sft_step_trace: bad argument");
  if (const int rc = dsh_enter(c, "dsh_lab_sft_step_trace")) return rc;
  if (!c->ran) return dsh_fail(c, DSH_ERR_STATE, "dsh_lab_sft_step_trace: no run");
#ifndef SFT_STEP_TRACE
  return dsh_fail(c, DSH_ERR_STATE, "dsh_lab_sft_step_trace: this build has no step trace (make lab EXTRA=-DSFT_STEP_TRACE)");
#else
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out64, c->h_probs[b].dbg + 16, 64 * sizeof(double), hipMemcpyDeviceToHost));
  return DSH_OK;
#endif
}

int dsh_lab_sft_system(dsh_ctx* c, int b, int32_t D, double* H, double* bvec, double* chi2) {
  if (!c || b < 0 || b >= c->B) return dsh_fail(c, DSH_ERR_ARG, "dsh_lab_sft_system: bad argument");
  if (const int rc = dsh_enter(c, "dsh_lab_sft_system")) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));   // an asynchronous run may still be using the problem table
  SftDev h = c->h_probs[b];
  if (D != 6 + h.Dn) return dsh_fail(c, DSH_ERR_ARG, "dsh_lab_sft_system: D mismatch");
  // flip the mode of this one problem, run it alone, restore
  const int32_t mode_saved = h.mode, split_saved = h.split;
  h.mode = 1;
  h.split = 0;   // the one-workgroup kernel assembles into the undivided band matrix
  HIPCHK(c, hipMemcpy(c->d_probs + b, &h, sizeof(SftDev), hipMemcpyHostToDevice));
  { LDS_LOCK(); HIPCHK(c, sft_lm_launch(c->d_probs + b, 1, c->plan.max_kd, c->plan.jl_doubles, c->plan.nw, LDS_MARKS(c).lm, c->stream)); }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->ran = false;   // the state of problem b was reset: a download would not return the results of the last run
  h.mode = mode_saved;
  h.split = split_saved;
  HIPCHK(c, hipMemcpy(c->d_probs + b, &h, sizeof(SftDev), hipMemcpyHostToDevice));
  const size_t Dnp = (size_t)((h.Dn + kNB - 1) / kNB) * kNB;
  const size_t band_elems = h.tile_mode ? (Dnp / kTS) * (size_t)h.tpr * kTS * kTS : Dnp * (size_t)h.ldh;
  std::vector<double> Hb(h.tile_mode == 1 ? 0 : band_elems), Hbord(SFT_BORDER * Dnp), Hc(56);
  auto hidx = [&](int r, int cc) -> size_t {
    const size_t tb = ((size_t)(r >> 4) * h.tpr + ((r >> 4) - (cc >> 4))) * (kTS * kTS);
    if (h.tile_mode == 1) return tb + ((((r & 15) & 3) << 4) + (cc & 15)) * 4 + ((r & 15) >> 2);
    if (h.tile_mode == 2) return tb + ((((cc & 15) & 3) << 4) + (r & 15)) * 4 + ((cc & 15) >> 2);   // wide mode keeps the tiles transposed
    return (size_t)r * h.ldh + (cc - r + h.kd);
  };
  // tile mode 1: H is kept as compact 3x3 blocks; it is read here the way the factorisation reads it, through the gather lists
  const dsh::SftGraph& g = *c->packed[b].g;
  std::vector<double> Hcomp;
  if (h.tile_mode == 1) {
    Hcomp.resize(g.hc_elems());
    HIPCHK(c, hipMemcpy(Hcomp.data(), h.Hc, 8 * Hcomp.size(), hipMemcpyDeviceToHost));
  } else {
    HIPCHK(c, hipMemcpy(Hb.data(), h.Hb, 8 * Hb.size(), hipMemcpyDeviceToHost));
  }
  auto hval = [&](int r, int cc) -> double {
    if (h.tile_mode != 1) return Hb[hidx(r, cc)];
    const int I = r >> 4, d = I - (cc >> 4);
    if (d > kBT) return 0.0;
    const int lane = (((r & 15) & 3) << 4) + (cc & 15), q = (r & 15) >> 2;
    return Hcomp[g.hgather[(((size_t)I * (kBT + 1) + d) * 64 + lane) * 4 + q] / 8];
  };
  HIPCHK(c, hipMemcpy(Hbord.data(), h.Hbord, 8 * Hbord.size(), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(Hc.data(), h.Hcorner, 8 * 49, hipMemcpyDeviceToHost));
  if (chi2) HIPCHK(c, hipMemcpy(chi2, h.dbg, 8, hipMemcpyDeviceToHost));
  // reference index order: camera 0..5, node a -> 6+3a
  if (H) {
    std::fill(H, H + (size_t)D * D, 0.0);
    for (int r = 0; r < h.Dn; r++)
      for (int k = 0; k <= h.kd; k++) {
        const int cidx = r - h.kd + k;
        if (cidx < 0) continue;
        const double v = hval(r, cidx);
        H[(size_t)(6 + r) + (size_t)(6 + cidx) * D] = v;
        H[(size_t)(6 + cidx) + (size_t)(6 + r) * D] = v;
      }
    for (int k = 0; k < 6; k++)
      for (int r = 0; r < h.Dn; r++) {
        const double v = Hbord[(size_t)k * Dnp + r];
        H[(size_t)k + (size_t)(6 + r) * D] = v;
        H[(size_t)(6 + r) + (size_t)k * D] = v;
      }
    for (int r = 0; r < 6; r++)
      for (int k = 0; k <= r; k++) {
        H[(size_t)r + (size_t)k * D] = Hc[r * 7 + k];
        H[(size_t)k + (size_t)r * D] = Hc[r * 7 + k];
      }
  }
  if (bvec) {
    for (int r = 0; r < 6; r++) bvec[r] = Hc[42 + r];
    for (int r = 0; r < h.Dn; r++) bvec[6 + r] = Hbord[(size_t)6 * Dnp + r];
  }
  return DSH_OK;
}
#endif  // DSH_LAB

}  // extern "C"
