// The launch shape of an SfT batch (sft_plan.h).  Plain host C++: no HIP runtime call, no context.
#include "sft_plan.h"

#include <algorithm>

namespace {

// solver per half-bandwidth: register-window tiles (<= 128), left-looking wide tiles (<= 256; the lab option "wide_off"
// keeps the row-major band solver for A/B runs), row-major band otherwise
void set_tile_mode(SftProblemPlan& p, int kd, int tile_mode) {
  p.tile_mode = tile_mode;
  p.wbt = tile_mode == 1 ? kBT : (tile_mode == 2 ? (kd + kTS - 1) / kTS : 0);
  p.tpr = tile_mode ? p.wbt + 1 : 0;
}

// Two-sided factorisation (SftPart in sft_problem.h): the problem is cut at a separator of one bandwidth and its two halves are
// factored by two workgroups at the same time.
void set_cut(SftProblemPlan& p, const SftSizes& z, const SftCut& cut) {
  const int sT = cut.sT, n1p = ((cut.n1 + kTS - 1) / kTS) * kTS;
  p.split = 1; p.sp_c0 = cut.c0; p.sp_s = cut.sp; p.sp_n1p = n1p; p.sp_pad = n1p - cut.n1;
  SftPart& p0 = p.part[0]; SftPart& p1 = p.part[1]; SftPart& p2 = p.part[2];
  p0 = SftPart{}; p1 = SftPart{}; p2 = SftPart{};
  p0.nS = cut.c0 / kTS; p0.nT = p0.nS + sT; p0.tpr = p.tpr; p0.wbt = p.wbt; p0.b_base = 0; p0.b_sign = 1; p0.b_lo = 0; p0.b_hi = cut.c0 + cut.sp;
  p1.nS = n1p / kTS; p1.nT = p1.nS + sT; p1.tpr = p.tpr; p1.wbt = p.wbt; p1.b_base = z.Dn - 1 + p.sp_pad; p1.b_sign = -1; p1.b_lo = p.sp_pad; p1.b_hi = n1p;
  p2.nS = sT; p2.nT = sT; p2.wbt = sT - 1; p2.tpr = sT;
  p.sp_xl = sT * p2.tpr * kTS * kTS + 8 * kTS * sT + 64;
  p.part[3] = p2;   // second workspace of the reduced problem (SFT_SPEC_SOLVE: one per workgroup)
}

}  // namespace

SftBatchPlan sft_plan_batch(const SftSizes* sizes, int B, int num_cus, const SftOptions& opt, bool host_only, SftUploadMode mode) {
  const bool one_lane = mode != SftUploadMode::batch;         // the multi-GPU modes: always the 8-wavefront shape, no speculative lanes
  const bool force_split = mode == SftUploadMode::connected;  // the two-sided cut with one workgroup (rank) per part
  SftBatchPlan plan;
  plan.prob.resize(B);
  bool all_tiles = true;
  for (int b = 0; b < B; b++) {
    const int kd = sizes[b].kd;
    set_tile_mode(plan.prob[b], kd, (kd <= kTS * kBT) ? 1 : ((kd <= kTS * kWB && !opt.wide_off) ? 2 : 0));
    all_tiles = all_tiles && plan.prob[b].tile_mode == 1;
    plan.max_iters_batch = std::max(plan.max_iters_batch, (int)sizes[b].max_iters);
  }
  // Launch shape: 8 wavefronts per problem give the lowest latency; with at least two problems per CU, 4 wavefronts
  // per problem (two problems resident per CU, <= 80 KB of LDS each) give the higher throughput.  Band mode needs 8.
  // More problems than the latency mode takes (half a problem per CU): the throughput shape.  From two problems per CU upwards that is rounds of
  // phase kernels + the tail kernel; below, the tail threshold (run_rounds_enqueue) covers the whole batch and the step is the tail kernel
  // alone -- one persistent workgroup per CU pulling problems, with the LIN kernel's record placement: 12 against 14 ms per problem for the
  // one-workgroup-per-problem kernel that ran these sizes until r06 (tools/batch_curve.py: 256 problems 13.97 -> 11.9 ms per step)
  if (all_tiles && 2 * B > num_cus) plan.nw = 4;
  if ((opt.waves == 4 && all_tiles) || opt.waves == 8) plan.nw = opt.waves;   // lab builds only (dsh_lab_set_option)
  if (one_lane) plan.nw = 8;
  // From two problems per CU upwards the batch runs as rounds of phase kernels with one wavefront per factorisation (sft_batch.h)
  plan.rounds_mode = all_tiles && plan.nw == 4 && opt.waves == 0 && opt.rounds != 0 && !host_only;
  // sub-batches: each must still fill the device with factor waves (one per SIMD) several times over
  if (plan.rounds_mode) {
    // (measured on MI355X, tools/streams_ab.py, 16384 C2 problems: 416 / 428 / 424 / 423 ms per step for 1 / 2 / 3 / 4 sub-batches -- what the
    // overlapped tails win, the additional launches and last-problem back substitutions lose again: one sub-batch unless asked otherwise)
    const int want = opt.streams > 0 ? opt.streams : 1;
    while (plan.n_sub < want && plan.n_sub < kSftMaxSub && B / (plan.n_sub + 1) >= 16 * num_cus) plan.n_sub++;
    if (opt.streams > 0) plan.n_sub = std::min(std::min(opt.streams, kSftMaxSub), std::max(1, B / 64));
  }
  // Latency mode: while CUs would idle anyway, every problem gets K of them and tries K dampings per iteration at once.
  int K = 1;
  if (plan.nw == 8 && !one_lane && !host_only) {
    K = (4 * B <= num_cus) ? 4 : ((3 * B <= num_cus) ? 3 : ((2 * B <= num_cus) ? 2 : 1));   // as many lanes as the device holds at once
    // Wide bands (two-sided factorisation with helper workgroups, sft_wide.h): a part's helpers are worth more than the third and fourth lane when
    // the device cannot hold both -- two lanes with three helpers per part against four lanes without (C5 x 16: 47.2 against 51.0 ms per step).
    // Every problem must be one that is cut AND gets helpers below, with one difference: this rule looks at the tile mode AS PACKED -- a narrow
    // band that the promotion below moves to the wide-tile code does not count as wide here (and a wide band that stays undivided keeps its four lanes).
    bool wide = opt.split != 0 && opt.helpers != 0;
    for (int b = 0; b < B; b++) {
      const SftCut cut = sft_cut(sizes[b].Dn, sizes[b].kd);
      const int packed_tile_mode = plan.prob[b].tile_mode;   // (nothing is promoted yet)
      wide = wide && packed_tile_mode == 2 && cut.sT >= opt.helpers_wbt && cut.room;
    }
    if (wide && K == 4 && (long long)B * 4 * 2 * 3 > num_cus && (long long)B * 2 * 2 * 3 <= num_cus) K = 2;
    if (opt.speculate >= 1 && opt.speculate <= SFT_SPEC_MAXK) K = opt.speculate;   // lab builds only
    for (int b = 0; b < B; b++) if (sizes[b].max_iters < 1) K = 1;
  }
  plan.K = K;
  // LDS of the assembly (it aliases the solver workspace): the records a gather touches most often, as far as the budget goes
  // (4 wavefronts: two problems share a CU's 160 KB)
  // (rounds of phase kernels: the LIN kernel is the only one that stages records, eight wavefronts and one workgroup per CU -- sft_batch.h)
  const size_t lds_budget = ((((plan.nw == 4 && !plan.rounds_mode) || SFT_WAVES_PER_EU >= 4) ? 75 : 155) * 1024) / 8;   // doubles, next to ~4.3 KB of control block and reduction scratch
  for (int b = 0; b < B; b++) {
    const SftSizes& z = sizes[b];
    SftProblemPlan& p = plan.prob[b];
    // A narrow band (kd <= 128) that is long enough for two parts also takes the two-sided factorisation in latency mode: it runs on the
    // left-looking wide-tile code (tile mode 2 works for any half-bandwidth up to 256), two workgroups per damping trial instead of one
    // (C2: 4.1 ms per frame against 4.5 on the register-window solver -- the default since the SOLVE launch split the back substitutions).
    // Only while the launch is small: measured on C2, 4 lanes (tools/latency_batch_ab.py), the two-sided path wins up to 12 problems per launch
    // (4.09 against 4.49 ms for one, 5.97 against 6.15 for twelve) and loses from 16 on (6.31 against 6.18; 48 problems: 11.0 against 7.4) --
    // a wide band gains at every size (C5: 33 against 62 ms for one problem, 89 against 116 for 64).
    if ((force_split && p.tile_mode == 1) ||
        (K > 1 && p.tile_mode == 1 && opt.split >= 2 && 20 * B <= num_cus && z.kd > kTS && z.Dn >= 8 * kTS * ((z.kd + kTS - 1) / kTS))) {
      // (kd > kTS: a band of one tile has no separator of two tile columns -- it would run the wide-tile code on one workgroup for nothing)
      set_tile_mode(p, z.kd, 2);
    }
    p.dataflow = p.tile_mode == 1 && opt.dataflow;   // the barrier version of the factor steps exists in lab builds only
    // The cut is granted on the tile mode AFTER the promotion: in latency mode (or the connected-mesh mode) every wide-tile problem with room
    // for two parts of at least four tile columns is cut.
    if ((force_split || (K > 1 && opt.split)) && p.tile_mode == 2) {
      const SftCut cut = sft_cut(z.Dn, z.kd);
      if (cut.room) set_cut(p, z, cut);
    }
    size_t used = 0;
    // placement class of the records (sft_kernels.hip: AsmRec): 1 = node positions + observation weights + curvature records, 2 = + node matrices + stretch records
    const size_t need1 = ((3 * (size_t)z.n + 1) & ~(size_t)1) + (((size_t)z.M + 1) & ~(size_t)1) + 4 * (size_t)z.S, need2 = need1 + 6 * (size_t)z.nA + 4 * (size_t)z.Es;
    const size_t need3 = need2 + 5 * (size_t)z.M;   // + the camera records as five doubles (only the LIN kernel of the phase rounds has the code)
    p.lds_class = (plan.rounds_mode && used + need3 <= lds_budget) ? 3 : (used + need2 <= lds_budget) ? 2 : ((used + need1 <= lds_budget) ? 1 : 0);
    used += p.lds_class == 3 ? need3 : p.lds_class == 2 ? need2 : (p.lds_class == 1 ? need1 : 0);
    plan.jl_doubles = std::max(plan.jl_doubles, used);
    if (p.lds_class >= 1) plan.xyz_doubles = std::max(plan.xyz_doubles, ((3 * (size_t)z.n + 1) & ~(size_t)1));   // (sftb_trial_kernel stages the positions of exactly these)
    plan.max_kd = std::max(plan.max_kd, p.tile_mode == 2 ? std::max((int)z.kd, kTS * kBT + 1) : (int)z.kd);   // (LDS of the wide-tile solver whenever a problem runs on it)
    plan.any_split = plan.any_split || p.split != 0;
  }
  // Helper workgroups of the two-sided factorisation: while CUs idle anyway, every part gets nh more of them for the far products of its block
  // columns (sft_wide.h).  Everything has to be resident at once for that to pay, so nh is what the device holds: B * K * 2 * (1 + nh) <= CUs.
  // (only where the far products are most of a block column: bands of at least 12 tiles; a narrow band through this path gains nothing --
  // C2, 8 tiles: 4.4 against 4.0 ms per frame with helpers)
  bool any = false;
  for (int b = 0; b < B; b++) any = any || (plan.prob[b].split != 0 && plan.prob[b].wbt >= opt.helpers_wbt);
  for (int b = 0; b < B; b++)   // (the owner's progress word keeps the finished block columns in 16 bits)
    if (plan.prob[b].split && std::max(plan.prob[b].part[0].nT, plan.prob[b].part[1].nT) >= 60000) any = false;
  if (any && K > 1 && !force_split) {
    while (plan.nh < 3 && (long long)B * K * 2 * (2 + plan.nh) <= num_cus) plan.nh++;
    if (plan.nh == 1) plan.nh = 0;                       // (one helper cannot feed its owner: 8.5 against 7 us per block column -- measured slower than none)
    if (opt.helpers >= 0) plan.nh = opt.helpers;   // lab builds only
  }
  return plan;
}
