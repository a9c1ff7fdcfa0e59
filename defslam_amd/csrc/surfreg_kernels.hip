// Surface registration of a keyframe on the resident stores (dsh_keyframe_snapshot_positions, dsh_keyframe_register_clouds,
// dsh_keyframe_register, dsh_keyframe_set_pose; gfx950).
//   DefKeyFrame::DefKeyFrame, PosesKeyframes        Modules/Common/DefKeyFrame.cc:60-74
//   SurfaceRegistration::registerSurfaces           Modules/Mapping/SurfaceRegistration.cc:60-104 (the clouds), :150 (SetPose)
//   Surface::applyScale                             Modules/Mapping/Surface.cc:107-121
//   KeyFrame::SetPose                               Thirdparty/ORBSLAM_2/src/KeyFrame.cc:97-111
// The snapshot and the selection run in ONE workgroup each: a keyframe has at most a few thousand key points, the pairs are numbered in
// entry order across the workgroup's tiles (ordered_slot, mpdb_device.h), and the selection's two passes -- the point-to-entry map of
// the snapshot, then the lookup -- are separated by a barrier instead of a second launch.  The map is a sparse set: entry_of[p] is not
// initialised and is trusted only where the snapshot names p at that entry, so nothing per point of the store is cleared.  These
// kernels are launch- and latency-bound.  Compiled without FMA contraction: the float32 expression order of the reference is kept.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "mpdb_device.h"
#include "surfreg_problem.h"

namespace {

// x3wh = Twc * x3ch of float cv::Mat, as ts_to_world (tmplswitch_kernels.hip): per row the four products summed left to right in float32
__device__ __forceinline__ void sr_to_world(const float* T, float x, float y, float z, float* w) {
#pragma unroll
  for (int r = 0; r < 3; r++) w[r] = ((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z) + T[4 * r + 3] * 1.0f;
}

// the workgroup's sum of v: every thread calls it (two barriers), every thread gets the sum
__device__ __forceinline__ int sr_block_sum(int v, int* wsum) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int w = 0; w < SR_BLOCK / 64; w++) s += wsum[w];
  return s;
}

// DefKeyFrame.cc:60-74: if (pMP && !pMP->isBad() && pMP->getFacet()) PosesKeyframes[this] = GetWorldPos()
__global__ __launch_bounds__(SR_BLOCK) void sr_snapshot_kernel(TcState s, SrKeyframe k, int32_t* n_taken) {
  __shared__ int wsum[SR_BLOCK / 64];
  int taken = 0;
  for (int i = threadIdx.x; i < k.N; i += SR_BLOCK) {
    const int p = k.table[k.tab_off + i];
    if (p < 0 || s.bad[p] || s.nodes[3 * (size_t)p] < 0) continue;
    const size_t e = (size_t)k.tab_off + i;
    k.snap_point[e] = p;
    for (int r = 0; r < 3; r++) k.snap_xyz[3 * e + r] = s.xyz[3 * (size_t)p + r];
    taken++;
  }
  const int total = sr_block_sum(taken, wsum);
  if (threadIdx.x == 0) *n_taken = total;
}

__global__ __launch_bounds__(SR_BLOCK) void sr_select_kernel(TcState s, SrSelect k) {
  __shared__ int wsum[SR_BLOCK / 64];
  const int t = threadIdx.x, N = k.kf.N;
  const int32_t* snap_point = k.kf.snap_point + k.kf.tab_off;
  const float* snap_xyz = k.kf.snap_xyz + 3 * (size_t)k.kf.tab_off;
  // pass 1: where the snapshot of a point lies.  Entries that name the same point hold the same bytes: any of them serves.
  for (int j = t; j < N; j += SR_BLOCK) {
    const int q = snap_point[j];
    if (q >= 0 && q < k.P) k.entry_of[q] = j;
  }
  __syncthreads();
  // pass 2: SurfaceRegistration.cc:60-104 per entry, the pairs in entry order
  int n_cls[4] = {0, 0, 0, 0};   // empty, bad, no facet, no snapshot
  int n_pairs = 0;
  for (int base = 0; base < N; base += SR_BLOCK) {
    const int i = base + t;
    int cls = -1, j = -1;
    if (i < N) {
      const int p = k.kf.table[k.kf.tab_off + i];
      if (p < 0) cls = 0;
      else if (s.bad[p]) cls = 1;
      else if (s.nodes[3 * (size_t)p] < 0) cls = 2;
      else {
        j = snap_point[i] == p ? i : k.entry_of[p];
        if (j < 0 || j >= N || snap_point[j] != p) cls = 3;
        else cls = 4;
      }
      if (cls < 4) n_cls[cls]++;
    }
    const int pos = ordered_slot<SR_BLOCK>(cls == 4, n_pairs, wsum);
    if (cls == 4) {   // pos < N: at most one pair per entry
      float w3[3];
      sr_to_world(k.Twc, k.surface[3 * (size_t)i], k.surface[3 * (size_t)i + 1], k.surface[3 * (size_t)i + 2], w3);
      for (int r = 0; r < 3; r++) {
        k.cloud_surface[3 * (size_t)pos + r] = w3[r];
        k.cloud_map[3 * (size_t)pos + r] = snap_xyz[3 * (size_t)j + r];
      }
      k.pair_idx[pos] = i;
    }
  }
  int sums[4];
  for (int c = 0; c < 4; c++) sums[c] = sr_block_sum(n_cls[c], wsum);
  if (t == 0) {
    SrCounts out;
    out.n_pairs = n_pairs; out.n_empty = sums[0]; out.n_bad = sums[1]; out.n_no_facet = sums[2]; out.n_no_snapshot = sums[3];
    out.pad[0] = out.pad[1] = out.pad[2] = 0;
    *k.counts = out;
  }
}

__global__ __launch_bounds__(SR_FINISH_BLOCK) void sr_finish_kernel(SrFinish k) {
  const int i = blockIdx.x * SR_FINISH_BLOCK + threadIdx.x;
  // Surface::applyScale on a cv::Vec3f: Vec * double, rounded to float32 per component
  if (i < 3 * k.N) {
    k.surface_scaled[i] = (float)((double)k.surface[i] * k.s22);
    if (k.resident_pts) k.resident_pts[i] = (float)((double)k.resident_pts[i] * k.s22);
  }
  // Surface.cc:117-120: nodesDepth_[i] = s22 * nodesDepth_[i]
  if (k.resident_depth && i < k.n_depth) k.resident_depth[i] = k.s22 * k.resident_depth[i];
  if (blockIdx.x == 0 && threadIdx.x < 3) {
    const int c = threadIdx.x;
    const float o = sr_camera_centre(k.Tcw, c);
    if (k.kf_slot) k.kf_slot->Ow[c] = o;
    k.Ow[c] = o;
  }
}

}  // namespace

static_assert(sizeof(SrCounts) == 32, "SrCounts is eight int32");

extern "C" hipError_t sr_snapshot_launch(const TcState& s, const SrKeyframe& k, int32_t* n_taken, hipStream_t st) {
  hipLaunchKernelGGL(sr_snapshot_kernel, 1, dim3(SR_BLOCK), 0, st, s, k, n_taken);
  return hipGetLastError();
}

extern "C" hipError_t sr_select_launch(const TcState& s, const SrSelect& k, hipStream_t st) {
  hipLaunchKernelGGL(sr_select_kernel, 1, dim3(SR_BLOCK), 0, st, s, k);
  return hipGetLastError();
}

extern "C" hipError_t sr_finish_launch(const SrFinish& k, hipStream_t st) {
  const long long work = 3 * (long long)k.N > (k.resident_depth ? k.n_depth : 0) ? 3 * (long long)k.N : (k.resident_depth ? k.n_depth : 0);
  hipLaunchKernelGGL(sr_finish_kernel, blocks_for(work > 0 ? work : 1, SR_FINISH_BLOCK), dim3(SR_FINISH_BLOCK), 0, st, k);
  return hipGetLastError();
}
