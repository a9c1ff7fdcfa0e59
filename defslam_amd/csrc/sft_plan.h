// What dsh_sft_batch_upload decides and where it puts things, as values: the launch shape of a batch (SftBatchPlan, a function of the
// problems' sizes, the batch size, the CU count and the options -- no HIP runtime call, no context) and the byte layout of its device
// arena (SftBatchLayout).  dsh_api.cpp turns the two into the pointers of the SftDev table; the run functions read the plan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "sft_problem.h"

constexpr int kNB = 32;                     // must match NB in sft_kernels.hip
constexpr int kTS = 16, kBT = 8, kWB = 16;  // must match TS / BT in sft_kernels.hip and WB in sft_wide.h
constexpr int kSftMaxSub = 4;               // sub-batches of the throughput shape, each on a stream of its own

// Solver selection.  The product library always takes the defaults; libdefslam_hip_lab.so can override them through
// dsh_lab_set_option (include/defslam_hip_debug.h) for A/B runs.  No environment variables are read.
struct SftOptions { int waves = 0; int dataflow = 1; int wide_off = 0; int speculate = 0; int split = 2; int rounds = 1; int streams = 0; int helpers = -1; int tail = -1; int owner_waves = 8; int helpers_wbt = 12; };

// Who uploads: a batch of independent problems, or one rank's problem of a multi-GPU mode.  The shared-camera and the connected-mesh
// mode run phase kernels of their own on the 8-wavefront shape with one lane; the connected-mesh mode also takes the two-sided cut
// whatever the batch and the options say (one rank per part, no helper workgroups).
enum class SftUploadMode { batch, shared_camera, connected };

// The sizes of one packed problem that the plan and the layout depend on (fields of SftDev of the same names).
struct SftSizes { int32_t n, nA, Dn, kd, M, S, Es, max_iters; };

// Geometry of the two-sided cut of a band of Dn scalars and half-bandwidth kd (SftPart in sft_problem.h): a separator of sT tile
// columns (sp scalars) behind part 0 = scalars [0, c0); part 1 = the n1 scalars behind the separator.
struct SftCut {
  int sT, sp, c0, n1;
  bool room;   // two parts of at least four tile columns next to a separator of at least two
};
inline SftCut sft_cut(int Dn, int kd) {
  SftCut c;
  c.sT = (kd + kTS - 1) / kTS;
  c.sp = kTS * c.sT;
  c.c0 = ((Dn - c.sp) / 2 / kTS) * kTS;
  c.n1 = Dn - c.sp - c.c0;
  c.room = c.sT >= 2 && c.c0 >= 4 * kTS && c.n1 >= 4 * kTS;
  return c;
}

// The fields of a problem's SftDev that the plan decides (the packer leaves them zero).
struct SftProblemPlan {
  int32_t tile_mode = 0, wbt = 0, tpr = 0;
  bool dataflow = false;   // bit 1 of SftDev::mode
  int32_t lds_class = 0;
  int32_t split = 0, sp_c0 = 0, sp_s = 0, sp_n1p = 0, sp_pad = 0, sp_xl = 0;
  SftPart part[4] = {};    // shapes only: the pointers are bound at upload
  void apply(SftDev& h) const {
    h.tile_mode = tile_mode; h.wbt = wbt; h.tpr = tpr;
    h.mode = (h.mode & ~2) | (dataflow ? 2 : 0);
    h.lds_class = lds_class;
    h.split = split; h.sp_c0 = sp_c0; h.sp_s = sp_s; h.sp_n1p = sp_n1p; h.sp_pad = sp_pad; h.sp_xl = sp_xl;
    for (int g = 0; g < 4; g++) h.part[g] = part[g];
  }
};

struct SftBatchPlan {
  int nw = 8;                 // wavefronts per problem of the persistent kernel (4: two problems share a CU)
  bool rounds_mode = false;   // throughput shape (sft_batch.h): rounds of LIN / FACTOR / TRIAL launches over the whole batch, one wavefront per factorisation
  int n_sub = 1;              // sub-batches wanted; the upload lowers it to 1 when it cannot get their streams
  int K = 1;                  // latency mode: K workgroups ("lanes") per problem run the next K damping trials of an iteration side by side (sft_spec_kernel)
  int nh = 0;                 // helper workgroups per part of a two-sided factorisation (FACTOR launches of the latency mode, sft_wide.h)
  bool any_split = false;     // some problem runs the two-sided factorisation (SftPart): a FACTOR launch precedes every trial launch
  int max_kd = 0;
  size_t jl_doubles = 0;      // LDS of the assembly records (largest problem of the batch)
  size_t xyz_doubles = 0;     // LDS copy of the node positions in the TRIAL kernel of the phase rounds (largest problem of the batch)
  int max_iters_batch = 0;
  std::vector<SftProblemPlan> prob;   // B
};

SftBatchPlan sft_plan_batch(const SftSizes* sizes, int B, int num_cus, const SftOptions& opt, bool host_only, SftUploadMode mode);

// Byte offsets inside the device arena of a batch, in the order
//   [SftDev table][per-frame read-only arrays of every problem] | [result region: B headers, bodies] | [workspace ... synchronisation block ...]
struct SftBatchLayout {
  struct ReadOnly { size_t obs_nodes, obs_bary, obs_uv, obs_w, ob_ptr, ob_m, ob_c, viewed, xyz_init, pose_init; };
  struct Result { size_t xyz, chi2, trace, mp, outl; };   // relative to res_off
  struct Part { size_t Hb, Lb, Lt, LbT, Lbord, Linv, x, xchg, Pf, PfB, sync; };
  struct Work { size_t bak, camrec, wtv, Anode, Jstar, Jstr, Hc, Hb, Hbord, Hcn, Lb, Lbord, Lc, Linv, Lt, LbT, x, dbg, sx0, sx1, shadow_xyz, shadow_chi2, shadow_hdr; Part part[4]; };
  size_t o_tab = 0;             // K * B records, lane-major: lane 0 of every problem first
  std::vector<ReadOnly> ro;     // B
  size_t ro_bytes = 0;          // the leading bytes that are uploaded
  size_t res_off = 0, res_bytes = 0;
  std::vector<Result> res_offs; // B
  size_t ws_off = 0;            // everything from here on is cleared once, when the arena is allocated
  size_t o_spec = 0;            // K * B controller states of the latency mode
  size_t o_runs = 0;            // rounds: B controller states, the counters of the sub-batches, the LIN list
  size_t o_sync = 0, sync_total = 0;   // progress words and column flags of the helper workgroups: one block, a run clears it with one memset
  std::vector<Work> ws;         // K * B, entry e = lane * B + b
  size_t size = 0;
};
