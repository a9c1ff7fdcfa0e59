// The erase on the resident map point store (dsh_point_store_erase_observations, dsh_point_store_set_bad, dsh_point_store_cull and the
// two read-backs; gfx950): MapPoint::EraseObservation (MapPoint.cc:122-148), DefMapPoint::setBadFlag (DefMapPoint.cc:76-94),
// KeyFrame::EraseMapPointMatch (KeyFrame.cc:248-252) and LocalMapping::MapPointCulling (LocalMapping.cc:173-199) on dsh_mpdb's log,
// tables and per-point state.  The log is an unsorted stream, so what a point's remaining observations decide -- the new reference
// keyframe, the records and table entries setBadFlag removes -- is found by one pass over it (as kfinsert_kernels.hip and
// anchor_kernels.hip do).  The launches of a call, no host read between them; every count the later launches need stays in PeHdr:
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

#include "pointerase_problem.h"
#include "trackclose_problem.h"

namespace {

__device__ __forceinline__ unsigned long long lanes_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }

// *ctr += the lanes of the wavefront with `flag`; every lane of the wavefront calls it
__device__ __forceinline__ void wave_count(bool flag, int32_t* ctr) {
  const unsigned long long m = __ballot(flag);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(ctr, __popcll(m));
}

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
    const unsigned long long dm = __ballot(doomed);
    if (!dm) continue;
    int base = 0;
    if ((threadIdx.x & 63) == 0) base = atomicAdd(&b.hdr->n_erased, __popcll(dm));
    base = __shfl(base, 0, 64);
    if (doomed) {                                           // DefMapPoint.cc:83-91
      erase_match(b, rec.y, b.log_idx[r]);
      b.log[r].x = -1;
      b.out_erased[base + __popcll(dm & lanes_below())] = rec;   // inside the list: it has room for every live record
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

// ---- the read-back of observations: count, scan, fill over the log, then a rank by slot per point (ki_sort_kernel's pattern) ----

__global__ __launch_bounds__(PE_BLOCK) void pe_obs_clear_kernel(PeObsBufs b) {
  const int i = blockIdx.x * PE_BLOCK + threadIdx.x;
  if (i < b.P) b.sel_of[i] = -1;
  if (i < b.n) { b.cnt[i] = 0; b.fill[i] = 0; }
  if (i == 0) {
    PeHdr h = {};
    *b.hdr = h;
  }
}

__global__ __launch_bounds__(PE_BLOCK) void pe_obs_select_kernel(PeObsBufs b) {
  const int i = blockIdx.x * PE_BLOCK + threadIdx.x;
  if (i < b.n) b.sel_of[b.ids[i]] = i;
}

__global__ __launch_bounds__(PE_BLOCK) void pe_obs_count_kernel(PeObsBufs b) {
  for (long long r = (long long)blockIdx.x * PE_BLOCK + threadIdx.x; r < b.R; r += (long long)gridDim.x * PE_BLOCK) {
    const int p = b.log[r].x;
    if (p < 0) continue;   // erased
    const int k = b.sel_of[p];
    if (k >= 0) atomicAdd(&b.cnt[k], 1);
  }
}

// exclusive scan of cnt[0 .. n) into out_ptr[0 .. n]; one workgroup, a contiguous chunk per thread
__global__ __launch_bounds__(PE_BLOCK) void pe_obs_scan_kernel(PeObsBufs b) {
  __shared__ int part[PE_BLOCK];
  const int n = b.n, per = (n + PE_BLOCK - 1) / PE_BLOCK, t = threadIdx.x;
  const int lo = min(t * per, n), hi = min(lo + per, n);
  int s = 0;
  for (int k = lo; k < hi; k++) s += b.cnt[k];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int w = 0; w < PE_BLOCK; w++) {
      const int v = part[w];
      part[w] = run;
      run += v;
    }
    b.out_ptr[n] = run;
    b.hdr->total = run;
  }
  __syncthreads();
  int run = part[t];
  for (int k = lo; k < hi; k++) {
    b.out_ptr[k] = run;
    run += b.cnt[k];
  }
}

__global__ __launch_bounds__(PE_BLOCK) void pe_obs_fill_kernel(PeObsBufs b) {
  for (long long r = (long long)blockIdx.x * PE_BLOCK + threadIdx.x; r < b.R; r += (long long)gridDim.x * PE_BLOCK) {
    const int2 rec = b.log[r];
    if (rec.x < 0) continue;
    const int k = b.sel_of[rec.x];
    if (k < 0) continue;
    const int pos = b.out_ptr[k] + atomicAdd(&b.fill[k], 1);   // pos < out_ptr[k + 1]: the count pass saw the same records
    b.raw_slot[pos] = rec.y;
    b.raw_idx[pos] = b.log_idx[r];
  }
}

// a wavefront per point: every observation's rank by slot (slots are unique within a point, so the result does not depend on arrival order)
__global__ __launch_bounds__(64) void pe_obs_rank_kernel(PeObsBufs b) {
  if (b.hdr->total > b.cap) return;   // the lists do not fit: the host reports the need, nothing is written
  const int lane = threadIdx.x;
  for (int k = blockIdx.x; k < b.n; k += gridDim.x) {
    const int o = b.out_ptr[k], M = b.cnt[k];
    for (int i = lane; i < M; i += 64) {
      const int s = b.raw_slot[o + i];
      int rank = 0;
      for (int q = 0; q < M; q++) rank += b.raw_slot[o + q] < s;
      b.out_slot[o + rank] = s;   // rank < M
      b.out_idx[o + rank] = b.raw_idx[o + i];
    }
  }
}

inline int blocks_for(long long n) { return (int)((n + PE_BLOCK - 1) / PE_BLOCK); }

// eight records per thread, at most 1024 workgroups, as lm_votes_kernel
inline int log_blocks(long long R) {
  const long long g = (R + 8 * PE_BLOCK - 1) / (8 * PE_BLOCK);
  return (int)(g > 1024 ? 1024 : g < 1 ? 1 : g);
}

}  // namespace

static_assert(sizeof(dsh_point_erase_counts) == 20, "dsh_point_erase_counts is five int32");

extern "C" hipError_t pe_erase_launch(const PeBufs& b, hipStream_t st) {
  hipLaunchKernelGGL(pe_clear_kernel, dim3(blocks_for(b.P > 1 ? b.P : 1)), dim3(PE_BLOCK), 0, st, b);
  if (b.n > 0) {
    hipLaunchKernelGGL(pe_select_kernel, dim3(blocks_for(b.n)), dim3(PE_BLOCK), 0, st, b);
    if (b.R > 0) hipLaunchKernelGGL(pe_sweep_kernel, dim3(log_blocks(b.R)), dim3(PE_BLOCK), 0, st, b);
    hipLaunchKernelGGL(pe_finish_kernel, dim3(blocks_for(b.n)), dim3(PE_BLOCK), 0, st, b);
  }
  return hipGetLastError();
}

extern "C" hipError_t pe_observations_launch(const PeObsBufs& b, hipStream_t st) {
  const int top = b.P > b.n ? b.P : b.n;
  hipLaunchKernelGGL(pe_obs_clear_kernel, dim3(blocks_for(top > 1 ? top : 1)), dim3(PE_BLOCK), 0, st, b);
  if (b.n > 0) hipLaunchKernelGGL(pe_obs_select_kernel, dim3(blocks_for(b.n)), dim3(PE_BLOCK), 0, st, b);
  if (b.n > 0 && b.R > 0) hipLaunchKernelGGL(pe_obs_count_kernel, dim3(log_blocks(b.R)), dim3(PE_BLOCK), 0, st, b);
  hipLaunchKernelGGL(pe_obs_scan_kernel, dim3(1), dim3(PE_BLOCK), 0, st, b);
  if (b.n > 0 && b.R > 0) {
    hipLaunchKernelGGL(pe_obs_fill_kernel, dim3(log_blocks(b.R)), dim3(PE_BLOCK), 0, st, b);
    hipLaunchKernelGGL(pe_obs_rank_kernel, dim3(b.n < 4096 ? b.n : 4096), dim3(64), 0, st, b);
  }
  return hipGetLastError();
}
