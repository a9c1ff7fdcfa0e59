// Per-point observation lists from the log of the resident map point store (gfx950).  The log is an unsorted append-only stream, so the
// lists of the points a call selected (sel_of) are built by two passes over it around a scan, no host read between them:
//   obs_count_kernel   pass over the log: live observations per list
//   obs_scan_kernel    ONE workgroup: the CSR offsets and the total
//   obs_fill_kernel    pass over the log: the observations in arrival order, optionally each with its keyframe's bad flag
// The order within a list is the callers' business: they rank by slot (obs_rank).  Integer valued.
#include <hip/hip_runtime.h>

#include "mpdb_device.h"
#include "obslist_problem.h"

namespace {

__device__ __forceinline__ long long records(const ObsLists& a) { return a.R + (a.n_extra ? *a.n_extra : 0); }

__global__ __launch_bounds__(OBS_BLOCK) void obs_count_kernel(ObsLists a) {
  const long long R = records(a);
  for (long long r = (long long)blockIdx.x * OBS_BLOCK + threadIdx.x; r < R; r += (long long)gridDim.x * OBS_BLOCK) {
    const int p = a.log[r].x;
    if (p < 0) continue;   // erased
    const int k = a.sel_of[p];
    if (k >= 0) atomicAdd(&a.cnt[k], 1);
  }
}

// exclusive scan of cnt[0 .. n) into off[0 .. n]; one workgroup, a contiguous chunk per thread
__global__ __launch_bounds__(OBS_BLOCK) void obs_scan_kernel(ObsLists a) {
  __shared__ int part[OBS_BLOCK];
  const int n = a.n_dev ? *a.n_dev : a.n, per = (n + OBS_BLOCK - 1) / OBS_BLOCK, t = threadIdx.x;
  const int lo = min(t * per, n), hi = min(lo + per, n);
  int s = 0;
  for (int k = lo; k < hi; k++) s += a.cnt[k];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int w = 0; w < OBS_BLOCK; w++) {
      const int v = part[w];
      part[w] = run;
      run += v;
    }
    a.off[n] = run;
    *a.total = run;
  }
  __syncthreads();
  int run = part[t];
  for (int k = lo; k < hi; k++) {
    a.off[k] = run;
    run += a.cnt[k];
  }
}

__global__ __launch_bounds__(OBS_BLOCK) void obs_fill_kernel(ObsLists a) {
  const long long R = records(a);
  for (long long r = (long long)blockIdx.x * OBS_BLOCK + threadIdx.x; r < R; r += (long long)gridDim.x * OBS_BLOCK) {
    const int2 rec = a.log[r];
    if (rec.x < 0) continue;
    const int k = a.sel_of[rec.x];
    if (k < 0) continue;
    const int pos = a.off[k] + atomicAdd(&a.fill[k], 1);   // pos < off[k + 1]: the count pass saw the same records
    a.raw_slot[pos] = rec.y | (a.kf && a.kf[rec.y].bad ? (int)0x80000000 : 0);   // slots fit 16 bits (DSH_MP_MAX_OBS keyframes)
    a.raw_idx[pos] = a.log_idx[r];
  }
}

}  // namespace

extern "C" hipError_t obs_lists_launch(const ObsLists& a, long long R_max, hipStream_t st) {
  const bool pass = a.n > 0 && R_max > 0;
  if (pass) hipLaunchKernelGGL(obs_count_kernel, dim3(log_blocks(R_max, OBS_BLOCK)), dim3(OBS_BLOCK), 0, st, a);
  hipLaunchKernelGGL(obs_scan_kernel, dim3(1), dim3(OBS_BLOCK), 0, st, a);
  if (pass) hipLaunchKernelGGL(obs_fill_kernel, dim3(log_blocks(R_max, OBS_BLOCK)), dim3(OBS_BLOCK), 0, st, a);
  return hipGetLastError();
}
