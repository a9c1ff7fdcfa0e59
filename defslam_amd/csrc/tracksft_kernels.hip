// The observation table of Optimizer::DefPoseOptimization from the resident map point store (dsh_track_sft_observations, dsh_track_sft;
// gfx950).
//   the loop over the frame's key points   Modules/Tracking/DefOptimizer.cc:293-361
// tf_select_kernel   a key point that is no outlier and holds a point that is not bad and has a facet becomes a row: its index, the id,
//                    the facet's nodes and barycentrics as the store holds them, the key point and mvInvLevelSigma2[octave] widened to
//                    double.  The rows are compacted IN KEY POINT ORDER whatever the grid: a workgroup counts the rows in front of its
//                    own key points itself (a frame has at most 8192, the count is a few reads per thread), then places its TF_TILES
//                    tiles one after the other by a ballot per wavefront and the wavefronts' totals in LDS (ordered_slot).  The last
//                    workgroup leaves M and Points_Obs.  One launch, no atomics; conversions only, no arithmetic.
#include <hip/hip_runtime.h>

#include "mpdb_device.h"
#include "tracksft_problem.h"

namespace {

// DefOptimizer.cc:295-303.  held: no outlier and a point (Points_Obs counts it, bad or not); take: the point is not bad and has a facet
__device__ __forceinline__ void tf_flags(const TfSelect& s, int i, int& p, bool& held, bool& take) {
  p = s.frame_points[i];
  held = p >= 0 && !s.outlier[i];
  take = held && !s.bad[p] && s.nodes[3 * (size_t)p] >= 0;
}

__global__ __launch_bounds__(TF_BLOCK) void tf_select_kernel(TfSelect s) {
  __shared__ int part[TF_BLOCK / 64][2];
  __shared__ int wsum[TF_BLOCK / 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int first = blockIdx.x * (TF_BLOCK * TF_TILES);
  // the rows and the held key points in front of this workgroup's
  int rows = 0, obs = 0;
  for (int j = threadIdx.x; j < first; j += TF_BLOCK) {
    int p;
    bool held, take;
    tf_flags(s, j, p, held, take);
    rows += take ? 1 : 0;
    obs += held ? 1 : 0;
  }
  for (int off = 32; off > 0; off >>= 1) {
    rows += __shfl_xor(rows, off, 64);
    obs += __shfl_xor(obs, off, 64);
  }
  if (lane == 0) {
    part[wave][0] = rows;
    part[wave][1] = obs;
  }
  __syncthreads();
  int base = 0, obs_front = 0;
  for (int w = 0; w < TF_BLOCK / 64; w++) {
    base += part[w][0];
    obs_front += part[w][1];
  }
  int obs_own = 0;
  for (int t = 0; t < TF_TILES; t++) {
    const int i = first + t * TF_BLOCK + threadIdx.x;
    int p = -1;
    bool held = false, take = false;
    if (i < s.N) tf_flags(s, i, p, held, take);
    obs_own += held ? 1 : 0;
    const int pos = ordered_slot<TF_BLOCK>(take, base, wsum);
    if (take) {
      const size_t q = (size_t)p, r = (size_t)pos;
      s.kp_index[r] = i;
      s.point_id[r] = p;
      for (int k = 0; k < 3; k++) {
        s.row_nodes[3 * r + k] = s.nodes[3 * q + k];
        s.row_bary[3 * r + k] = s.bary[3 * q + k];
      }
      s.uv[2 * r] = (double)s.kp[2 * (size_t)i];
      s.uv[2 * r + 1] = (double)s.kp[2 * (size_t)i + 1];
      s.invsig2[r] = (double)s.sig[s.octave[i]];   // :339: a float; the division by N of :340 is the packer's
    }
  }
  if (blockIdx.x == gridDim.x - 1) {
    for (int off = 32; off > 0; off >>= 1) obs_own += __shfl_xor(obs_own, off, 64);
    __syncthreads();   // every thread has read the counts in front
    if (lane == 0) part[wave][1] = obs_own;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 0; w < TF_BLOCK / 64; w++) obs_front += part[w][1];
      s.head[0] = base;
      s.head[1] = obs_front;
    }
  }
}

}  // namespace

extern "C" hipError_t tf_select_launch(const TfSelect& s, hipStream_t st) {
  if (s.N > 0) hipLaunchKernelGGL(tf_select_kernel, dim3(blocks_for(s.N, TF_BLOCK * TF_TILES)), dim3(TF_BLOCK), 0, st, s);
  return hipGetLastError();
}
