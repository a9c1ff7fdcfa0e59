// The end of a tracked frame and the queries of the next frame's motion-model search, on the resident map point store
// (dsh_track_end_frame, dsh_motion_model_search; gfx950).
//   DefTracking::CleanMatches, the outlier drop, mLastFrame = Frame(*mCurrentFrame)   Modules/Tracking/DefTracking.cc:667-679, :185-191, :211
//   the query filter of DefORBmatcher::SearchByProjection                               Modules/Matching/DefORBmatcher.cc:321-332
// mm_end_frame_kernel   ONE workgroup over the frame's key points (at most 8192): the two loops, the resident list and keyframe candidate, the counts
// mm_gather_kernel      the entries of the resident list that hold a point that is not bad and has a facet become the queries of
//                       track_kernels.hip, compacted IN INDEX ORDER: the queries interact in that order.  One launch, no scratch and no
//                       second pass: a workgroup counts the kept entries in front of its own MM_BLOCK entries itself (the list has at
//                       most 8192 entries, the count is a few reads per thread), then places its own by a ballot per wavefront and the
//                       wavefronts' totals in LDS.
// Integer valued; compiled without FMA contraction like track_kernels.hip, whose kernels run on what the gather writes.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "motionmodel_problem.h"
#include "mpdb_device.h"

namespace {

__global__ __launch_bounds__(MM_END_BLOCK) void mm_end_frame_kernel(MmEnd e) {
  __shared__ int tot[4];   // cleaned, dropped, kept, the largest octave kept
  if (threadIdx.x < 4) tot[threadIdx.x] = threadIdx.x == 3 ? -1 : 0;
  __syncthreads();
  int cleaned = 0, dropped = 0, kept = 0, top = -1;
  for (int i = threadIdx.x; i < e.N; i += MM_END_BLOCK) {
    int p = e.frame_points[i];
    uint8_t out = e.outlier[i] ? 1 : 0;
    if (p >= 0 && e.nobs[p] < 1) {   // CleanMatches (:673-677): Observations() is nObs, stale after a bad flag; no isBad test
      p = -1;
      out = 0;
      cleaned++;
    }
    e.points_out[i] = p;             // what CreateNewKeyFrame sees (:175-178)
    e.cand_ids[i] = p;               // and keeps resident for it
    e.outlier_out[i] = out;
    if (p >= 0 && out) {             // :185-191
      p = -1;
      dropped++;
    }
    const int oct = p >= 0 ? e.octave[i] : -1;
    e.last_ids[i] = p;               // :211
    e.last_oct[i] = oct;
    if (p >= 0) kept++;
    top = max(top, oct);
  }
  for (int off = 32; off > 0; off >>= 1) {
    cleaned += __shfl_xor(cleaned, off, 64);
    dropped += __shfl_xor(dropped, off, 64);
    kept += __shfl_xor(kept, off, 64);
    top = max(top, __shfl_xor(top, off, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&tot[0], cleaned);
    atomicAdd(&tot[1], dropped);
    atomicAdd(&tot[2], kept);
    atomicMax(&tot[3], top);
  }
  __syncthreads();
  if (threadIdx.x < 4) e.counts[threadIdx.x] = tot[threadIdx.x];
}

// DefORBmatcher.cc:325-332: the entry holds a point (its outlier flag left with the outlier drop), the point is not bad and has a facet
__device__ __forceinline__ bool is_query(const MmGather& g, int i) {
  const int p = g.last_ids[i];
  return p >= 0 && !g.bad[p] && g.nodes[3 * (size_t)p] >= 0;
}

__global__ __launch_bounds__(MM_BLOCK) void mm_gather_kernel(MmGather g) {
  __shared__ int part[MM_BLOCK / 64];
  __shared__ int own[MM_BLOCK / 64];
  const int first = blockIdx.x * MM_BLOCK;
  // the queries in front of this workgroup's entries
  int pre = 0;
  for (int j = threadIdx.x; j < first; j += MM_BLOCK) pre += is_query(g, j) ? 1 : 0;
  for (int off = 32; off > 0; off >>= 1) pre += __shfl_xor(pre, off, 64);
  const int i = first + threadIdx.x;
  const bool take = i < g.N && is_query(g, i);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = pre;
  int total;
  int pos = tile_rank<MM_BLOCK>(take, own, total);
  for (int w = 0; w < MM_BLOCK / 64; w++) pos += part[w];
  if (take) {
    const size_t p = (size_t)g.last_ids[i];
    g.out_ids[pos] = (int32_t)p;
    g.out_idx[pos] = i;
    g.qpid[pos] = 0;
    for (int k = 0; k < 3; k++) g.qxyz[3 * (size_t)pos + k] = g.xyz[3 * p + k];
    g.qmeta[pos] = g.last_oct[i];
    g.qdesc[2 * (size_t)pos] = g.desc[2 * p];
    g.qdesc[2 * (size_t)pos + 1] = g.desc[2 * p + 1];
    g.qfree[pos] = g.nobs[p] > 0 ? 0 : 1;   // DefORBmatcher.cc:381-383
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    for (int w = 0; w < MM_BLOCK / 64; w++) total += part[w];
    *g.out_count = total;
  }
}

}  // namespace

extern "C" hipError_t mm_end_frame_launch(const MmEnd& e, hipStream_t st) {
  hipLaunchKernelGGL(mm_end_frame_kernel, dim3(1), dim3(MM_END_BLOCK), 0, st, e);
  return hipGetLastError();
}

extern "C" hipError_t mm_gather_launch(const MmGather& g, hipStream_t st) {
  if (g.N > 0) hipLaunchKernelGGL(mm_gather_kernel, dim3(blocks_for(g.N, MM_BLOCK)), dim3(MM_BLOCK), 0, st, g);
  return hipGetLastError();
}
