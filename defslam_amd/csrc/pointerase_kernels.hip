// The erase on the resident map point store (dsh_point_store_erase_observations, dsh_point_store_set_bad, dsh_point_store_cull and the
// two read-backs; gfx950): MapPoint::EraseObservation (MapPoint.cc:122-148), DefMapPoint::setBadFlag (DefMapPoint.cc:76-94),
// KeyFrame::EraseMapPointMatch (KeyFrame.cc:248-252) and LocalMapping::MapPointCulling (LocalMapping.cc:173-199) on dsh_mpdb's log,
// tables and per-point state.  The log is an unsorted stream, so what a point's remaining observations decide -- the new reference
// keyframe, the records and table entries setBadFlag removes -- is found by one pass over it.  The launches of a call, no host read between them; every count the later launches need stays in PeHdr:
//   pe_clear_kernel      the marks and candidates over P, the counters
//   pe_select_kernel     one thread per pair or id.  An erase blanks the pair's record, decrements nObs, writes the optional table
//                        entry and marks the point PE_SEEK (its reference keyframe was the erased one) and PE_DOOMED (nObs <= 2); a
//                        set-bad marks PE_DOOMED; a cull takes tc_cull_action's decision.  Points are distinct within a batch: plain stores
//   pe_sweep_kernel      one grid-stride pass over the log that leaves at its first instruction when nothing is marked.  A live record of
//                        a PE_SEEK point lowers the point's candidate slot; a live record of a PE_DOOMED point nulls the table entry it
//                        names, is blanked and goes into the erased list (one atomic per wavefront).  Both for one record, in this
//                        order: the reference keyframe moves before the cascade, on the records the cascade removes
//   pe_finish_kernel     one thread per pair or id: commits the reference keyframe, sets the bad flag, writes the status
// Every table write is -1 and every log write a blank, so a batch does not depend on the order of its entries.
#include <hip/hip_runtime.h>

#include "mpdb_device.h"
#include "pointerase_problem.h"
#include "trackclose_problem.h"

namespace {

// KeyFrame::EraseMapPointMatch(idx) of keyframe `slot`; idx is inside the keyframe for every record the host let through
__device__ __forceinline__ void erase_match(const PeBufs& b, int slot, int idx) {
  const LmKf k = b.kf[slot];
  if ((unsigned)idx < (unsigned)k.N) b.table[(size_t)k.tab_off + idx] = -1;
}

__global__ __launch_bounds__(PE_BLOCK) void pe_clear_kernel(PeBufs b) {
  const int i = blockIdx.x * PE_BLOCK + threadIdx.x;
  if (i < b.P) { b.mark[i] = 0; b.cand[i] = PE_NO_SLOT; }
  if (i == 0) {
    PeHdr h = {};
    *b.hdr = h;
  }
}

__global__ __launch_bounds__(PE_BLOCK) void pe_select_kernel(PeBufs b) {
  const int i = blockIdx.x * PE_BLOCK + threadIdx.x;
  const bool in = i < b.n;
  bool found = false, seek = false, doomed = false;
  if (in) {
    const int p = b.ids[i];
    if (b.mode == PE_ERASE) {
      const long long r = b.rec[i];
      if (r >= 0) {                                         // MapPoint.cc:127
        const int s = b.slots[i];
        found = true;
        b.log[r].x = -1;                                    // :135
        const int left = b.nobs[p] - 1;                     // :133
        b.nobs[p] = left;
        if (b.erase_match) erase_match(b, s, b.log_idx[r]); // SchwarpDatabase.cc:291, whatever the entry holds
        seek = b.ref_kf[p] == s;                            // :137
        doomed = left <= 2;                                 // :141
      }
    } else if (b.mode == PE_SET_BAD) {
      doomed = true;
    } else {
      const uint8_t a = tc_cull_action(b.bad[p], b.found[p], b.visible[p], b.current_kf, b.first_kf[i]);
      b.out_code[i] = a;
      doomed = a == 2;                                      // LocalMapping.cc:191
    }
    if (seek || doomed) b.mark[p] = (seek ? PE_SEEK : 0) | (doomed ? PE_DOOMED : 0);
  }
  wave_count(found, &b.hdr->n_found);
  wave_count(seek, &b.hdr->n_seek);
  wave_count(doomed, &b.hdr->n_doomed);
}

__global__ __launch_bounds__(PE_BLOCK) void pe_sweep_kernel(PeBufs b) {
  if (b.hdr->n_seek == 0 && b.hdr->n_doomed == 0) return;
  const long long stride = (long long)gridDim.x * PE_BLOCK;
  for (long long r0 = (long long)blockIdx.x * PE_BLOCK; r0 < b.R; r0 += stride) {   // wave-uniform trip count: the ballot sees 64 lanes
    const long long r = r0 + threadIdx.x;
    int2 rec = make_int2(-1, -1);
    if (r < b.R) rec = b.log[r];
    const int m = rec.x >= 0 ? b.mark[rec.x] : 0;
    if (m & PE_SEEK) atomicMin(&b.cand[rec.x], rec.y);      // mObservations.begin()->first, MapPoint.cc:138
    const bool doomed = (m & PE_DOOMED) != 0;
    const int at = wave_append(doomed, &b.hdr->n_erased);
    if (doomed) {                                           // DefMapPoint.cc:83-91
      erase_match(b, rec.y, b.log_idx[r]);
      b.log[r].x = -1;
      b.out_erased[at] = rec;                               // inside the list: it has room for every live record
    }
  }
}

__global__ __launch_bounds__(PE_BLOCK) void pe_finish_kernel(PeBufs b) {
  const int i = blockIdx.x * PE_BLOCK + threadIdx.x;
  const bool in = i < b.n;
  bool moved = false, doomed = false;
  if (in) {
    const int p = b.ids[i], m = b.mark[p];
    const bool found = b.mode == PE_ERASE && b.rec[i] >= 0;
    if (m & PE_SEEK) {
      const int s = b.cand[p];
      if (s != PE_NO_SLOT) { b.ref_kf[p] = s; moved = true; }   // no record left: the reference reads end(), here mpRefKF stays
    }
    doomed = (m & PE_DOOMED) != 0;
    if (doomed) b.bad[p] = 1;                               // DefMapPoint.cc:82; nObs stays
    if (b.mode == PE_ERASE) b.out_code[i] = found ? (doomed ? 2 : 1) : 0;
  }
  wave_count(moved, &b.hdr->n_ref_moved);
  wave_count(doomed, &b.hdr->n_set_bad);
}

// ---- the read-back of observations: the lists of obslist_kernels.hip, then a rank by slot per point ----

__global__ __launch_bounds__(PE_BLOCK) void pe_obs_clear_kernel(PeObsBufs b) {
  const int i = blockIdx.x * PE_BLOCK + threadIdx.x;
  if (i < b.P) b.ol.sel_of[i] = -1;
  if (i < b.n) { b.ol.cnt[i] = 0; b.ol.fill[i] = 0; }
  if (i == 0) {
    PeHdr h = {};
    *b.hdr = h;
  }
}

__global__ __launch_bounds__(PE_BLOCK) void pe_obs_select_kernel(PeObsBufs b) {
  const int i = blockIdx.x * PE_BLOCK + threadIdx.x;
  if (i < b.n) b.ol.sel_of[b.ids[i]] = i;
}

// a wavefront per point: every observation to its rank by slot
__global__ __launch_bounds__(64) void pe_obs_rank_kernel(PeObsBufs b) {
  if (b.hdr->total > b.cap) return;   // the lists do not fit: the host reports the need, nothing is written
  const int lane = threadIdx.x;
  for (int k = blockIdx.x; k < b.n; k += gridDim.x) {
    const int o = b.ol.off[k], M = b.ol.cnt[k];
    for (int i = lane; i < M; i += 64) {
      const int s = b.ol.raw_slot[o + i];
      int unused;
      const int rank = obs_rank(b.ol.raw_slot, o, M, s, unused);
      b.out_slot[o + rank] = s;   // rank < M
      b.out_idx[o + rank] = b.ol.raw_idx[o + i];
    }
  }
}

}  // namespace

static_assert(sizeof(dsh_point_erase_counts) == 20, "dsh_point_erase_counts is five int32");

extern "C" hipError_t pe_erase_launch(const PeBufs& b, hipStream_t st) {
  hipLaunchKernelGGL(pe_clear_kernel, dim3(blocks_for(b.P > 1 ? b.P : 1, PE_BLOCK)), dim3(PE_BLOCK), 0, st, b);
  if (b.n > 0) {
    hipLaunchKernelGGL(pe_select_kernel, dim3(blocks_for(b.n, PE_BLOCK)), dim3(PE_BLOCK), 0, st, b);
    if (b.R > 0) hipLaunchKernelGGL(pe_sweep_kernel, dim3(log_blocks(b.R, PE_BLOCK)), dim3(PE_BLOCK), 0, st, b);
    hipLaunchKernelGGL(pe_finish_kernel, dim3(blocks_for(b.n, PE_BLOCK)), dim3(PE_BLOCK), 0, st, b);
  }
  return hipGetLastError();
}

extern "C" hipError_t pe_observations_launch(const PeObsBufs& b, hipStream_t st) {
  const int top = b.P > b.n ? b.P : b.n;
  hipLaunchKernelGGL(pe_obs_clear_kernel, dim3(blocks_for(top > 1 ? top : 1, PE_BLOCK)), dim3(PE_BLOCK), 0, st, b);
  if (b.n > 0) hipLaunchKernelGGL(pe_obs_select_kernel, dim3(blocks_for(b.n, PE_BLOCK)), dim3(PE_BLOCK), 0, st, b);
  ObsLists a = b.ol;
  a.total = &b.hdr->total;
  const hipError_t e = obs_lists_launch(a, a.R, st);
  if (e != hipSuccess) return e;
  if (b.n > 0 && a.R > 0) {
    hipLaunchKernelGGL(pe_obs_rank_kernel, dim3(b.n < 4096 ? b.n : 4096), dim3(64), 0, st, b);
  }
  return hipGetLastError();
}
