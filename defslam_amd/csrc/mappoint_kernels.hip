// Map point upkeep (dsh_mappoint_update): MapPoint::ComputeDistinctiveDescriptors (Thirdparty/ORBSLAM_2/src/MapPoint.cc:257-325) and
// MapPoint::UpdateNormalAndDepth (MapPoint.cc:348-391) of a batch of independent map points, on the descriptor rows dsh_kfdb keeps in
// HBM.  Observation counts are very uneven, so a call has two kinds of work, all on the context's stream:
//   small   points with M <= 64 observations: lane groups of 8, 16, 32 or 64 lanes (the host bins points by M), one lane per row.  The
//           group stages its election rows in LDS, every lane forms its row of Hamming distances (16-bit, in registers) and finds the
//           element of rank floor((Me-1)/2) by a 9-step bisection on the distance value (0 .. 256); the winner is the (median, row)
//           minimum over the group.  The same lanes form the terms of the normal, summed in observation order.
//   large   points with more: one wavefront per block of 64 election rows.  Each lane owns a row and counts its distances to every
//           election row (read with wave-uniform addresses) into its own 257-bin histogram in LDS (16-bit counts, two to a word), then
//           walks it to the median; blocks publish (median << 16 | row) with atomicMin.  One more wavefront per point forms the
//           normal's terms 64 at a time and sums them in order.  The host starts the biggest points first.
//   finish  one thread per large point: the winner's descriptor row.
// Compiled without FMA contraction: the reference's float32 expression order is kept (see include/defslam_hip.h).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "mappoint_device.h"
#include "mappoint_problem.h"

namespace {

// the lists the host built, the results into the call's arrays: a point of pts is stored under its own index
struct MpuView {
  const MpuBufs& b;
  const int32_t* list;
  int n;
  __device__ int id(int p) const { return p; }
  __device__ void store_desc(int p, int e, const uint4& d0, const uint4& d1) const {
    b.best[p] = e;
    b.desc[2 * (size_t)p] = d0;
    b.desc[2 * (size_t)p + 1] = d1;
  }
  __device__ float* normal(int p) const { return b.normal + 3 * (size_t)p; }
  __device__ void store_depth(int p, float mx, float mn) const {
    b.dist[2 * (size_t)p] = mx;
    b.dist[2 * (size_t)p + 1] = mn;
  }
};

// W lanes per point; a block of 256 threads serves 256 / W points of one width class
template <int W>
__global__ __launch_bounds__(256) void mpu_small_kernel(MpuBufs b, int off, int n) {
  __shared__ uint4 sd[2 * 256];
  mp_small_body<W>(MpuView{b, b.small_order + off, n}, sd);
}

// one wavefront per block of large_blocks
__global__ __launch_bounds__(64) void mpu_large_kernel(MpuBufs b) {
  __shared__ uint32_t hist[64 * MPU_HIST_WORDS];
  mp_large_body(MpuView{b, nullptr, (int)gridDim.x}, hist);
}

__global__ __launch_bounds__(64) void mpu_finish_kernel(MpuBufs b, int n_large) { mp_finish_body(MpuView{b, b.large_pts, n_large}); }

}  // namespace

// small_off[5]: the small points of width class c (8, 16, 32, 64 lanes) are small_order[small_off[c] .. small_off[c + 1])
extern "C" hipError_t mpu_launch(const MpuBufs& b, const int32_t* small_off, int n_large_blocks, int n_large, hipStream_t st) {
  if (n_large_blocks > 0) hipLaunchKernelGGL(mpu_large_kernel, dim3(n_large_blocks), dim3(64), 0, st, b);
  if (n_large > 0) hipLaunchKernelGGL(mpu_finish_kernel, dim3((n_large + 63) / 64), dim3(64), 0, st, b, n_large);
  const int n8 = small_off[1] - small_off[0], n16 = small_off[2] - small_off[1], n32 = small_off[3] - small_off[2], n64 = small_off[4] - small_off[3];
  if (n8 > 0) hipLaunchKernelGGL(mpu_small_kernel<8>, dim3((n8 + 31) / 32), dim3(256), 0, st, b, small_off[0], n8);
  if (n16 > 0) hipLaunchKernelGGL(mpu_small_kernel<16>, dim3((n16 + 15) / 16), dim3(256), 0, st, b, small_off[1], n16);
  if (n32 > 0) hipLaunchKernelGGL(mpu_small_kernel<32>, dim3((n32 + 7) / 8), dim3(256), 0, st, b, small_off[2], n32);
  if (n64 > 0) hipLaunchKernelGGL(mpu_small_kernel<64>, dim3((n64 + 3) / 4), dim3(256), 0, st, b, small_off[3], n64);
  return hipGetLastError();
}
