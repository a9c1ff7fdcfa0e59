// The complete dsh_ctx: what the SfT entry points (dsh_api.cpp) and the multi-GPU modes (dsh_multi.cpp) keep on a context.  Every other
// translation unit sees the context through dsh_ctx_base (dsh_ctx.h).
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "dsh_template.h"
#include "sft_pack.h"
#include "sft_plan.h"
#include "sft_problem.h"

// The dynamic LDS size a kernel has been enabled for (hipFuncSetAttribute) is a property of the (device, kernel) pair, not of a context: two
// contexts on one GPU -- tracking and mapping, say -- must not lower each other's setting.  One high-water mark per device and kernel for the
// whole process (defined in dsh_api.cpp); the launchers only ever raise it, under this lock.
struct LdsMarks { size_t lm[2] = {0, 0}, sc = 0, spec[2] = {0, 0}, cn = 0, b[2] = {0, 0}, tail = 0; };
extern LdsMarks g_lds_marks[64];
extern std::mutex g_lds_mu;
#define LDS_MARKS(c) (g_lds_marks[(c)->device & 63])
#define LDS_LOCK() std::lock_guard<std::mutex> lds_lock__(g_lds_mu)

// ---- one packed problem on the host: the shared structure (graph) + the per-frame lists + the scalars of the device record
struct Packed {
  SftDev h{};                          // sizes + scalars (what the plan decides and the pointers are filled at upload)
  dsh::SftGraph* g = nullptr;          // owned by the context's graph cache
  dsh::SftFramePack f;
};

struct dsh_ctx : dsh_ctx_base {
  dsh::TemplateHost tmpl;
  // device copy of the template
  char* d_tmpl = nullptr;
  size_t d_tmpl_bytes = 0;
  struct TemplateDev {
    const double *xyz0, *nbr_w, *nbr_sumw, *k0;
    const int32_t *nbr_ptr, *nbr_idx;
  } dt{};
  // structure of the normal equations per active set of the current template (sft_pack.h), device-resident, built on first use
  std::vector<std::unique_ptr<dsh::SftGraph>> graphs;
  uint64_t upload_serial = 0;     // graphs touched by the upload in progress carry it (eviction keeps them)
  // batch
  int B = 0;
  std::vector<Packed> packed;
  // Launch shape and arena layout of the uploaded batch (sft_plan.h): assigned once, at the end of an upload that succeeded
  // (plan.n_sub: the sub-batches that run, after the upload got their streams)
  SftBatchPlan plan;
  SftBatchLayout layout;
  char* d_batch = nullptr;
  size_t d_batch_cap = 0;
  SftDev* d_probs = nullptr;       // inside d_batch
  std::vector<SftDev> h_probs;     // host mirror with device pointers
  HostBuf stage;                   // page-locked staging of the read-only part (one hipMemcpyAsync per upload)
  hipEvent_t stage_free = nullptr; // recorded behind the upload copy: the staging buffer may be refilled once it has fired
  bool stage_busy = false;
  HostBuf results;                 // page-locked landing zone of the result region (one hipMemcpyAsync per download)
  char* d_sync = nullptr;              // progress words and column flags of the helper workgroups (inside the batch arena), cleared at the start of every run
  int spec_hint = 12;                  // launches the previous speculative run needed (first group of the next one)
  SftSpec* d_spec = nullptr;           // K*B controller states of the latency mode, inside d_batch
  HostBuf spec_done;                   // page-locked: lane 0's SftSpec of every problem (the done flag)
  SftSc* d_sc = nullptr;               // shared-camera mode: LM state between the phase kernels
  SftRun* d_runs = nullptr;            // rounds: B controller states + the done counter behind them, inside d_batch
  int* d_counters = nullptr;
  int* d_linlist = nullptr;            // B ints behind the counters: the problems the next LIN launch linearises (sft_batch.h)
  int rounds_hint = 24;                // rounds the previous run of this context needed
  // The batch runs as up to kSftMaxSub sub-batches on streams of their own: the launches of a round are enqueued sub-batch by sub-batch, so
  // the tail of one sub-batch's FACTOR launch (waves that have run out of work) overlaps with the next launches of the others.
  hipStream_t sub_stream[kSftMaxSub] = {nullptr, nullptr, nullptr, nullptr};   // [0] = stream
  hipEvent_t sub_event[kSftMaxSub] = {nullptr, nullptr, nullptr, nullptr};
  std::vector<hipEvent_t>* phase_events = nullptr;   // lab builds (dsh_lab_sft_rounds_timed): an event in front of and behind every phase launch
  std::vector<int> phase_ids;                        // ... and which phase it was (SFTB_PH_*)
  int num_cus = 256;
  bool ran = false;
  SftOptions opt;
};

// The upload behind dsh_sft_batch_upload (which passes SftUploadMode::batch); the multi-GPU modes upload their rank's problem through it.
int dsh_sft_upload(dsh_ctx* c, int B, const dsh_sft_frame* frames, SftUploadMode mode);
