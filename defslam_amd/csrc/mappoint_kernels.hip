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

// mNormalVector = normal / n (MapPoint.cc:389) and the depth range (:379-388), written by one lane
__device__ __forceinline__ void write_geometry(const MpuBufs& b, const MpuPoint& pt, int p, float sx, float sy, float sz) {
  float mx, mn;
  mp_geometry(pt.M, sx, sy, sz, b.slots[pt.ref_slot], pt.x, pt.y, pt.z, pt.sf_level, pt.sf_last, b.normal + 3 * (size_t)p, mx, mn);
  b.dist[2 * (size_t)p] = mx;
  b.dist[2 * (size_t)p + 1] = mn;
}

// W lanes per point; a block of 256 threads serves 256 / W points of one width class
template <int W>
__global__ __launch_bounds__(256) void mpu_small_kernel(MpuBufs b, int off, int n) {
  __shared__ uint4 sd[2 * 256];
  const int t = threadIdx.x, r = t % W, g = t / W, gbase = (t & 63) - r;   // gbase: the group's first lane in the wavefront
  const int k = blockIdx.x * (256 / W) + g;
  const bool has = k < n;
  const int p = has ? b.small_order[off + k] : 0;
  MpuPoint pt;
  if (has) pt = b.pts[p];
  else { pt.M = pt.Me = 0; pt.what = 0; pt.x = pt.y = pt.z = 0.f; }
  const bool elect = (pt.what & 1) && pt.Me > 0, geom = (pt.what & 2) && pt.M > 0;
  uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
  if (elect && r < pt.Me) {
    const int row = b.el_row[pt.el_off + r];
    d0 = b.rows[2 * (size_t)row];
    d1 = b.rows[2 * (size_t)row + 1];
  }
  sd[2 * t] = d0;
  sd[2 * t + 1] = d1;
  __syncthreads();
  if (elect) {
    const uint32_t key = mp_elect_small<W>(d0, d1, sd + 2 * (t - r), pt.Me, r);
    if (r == 0) {
      const int e = (int)(key & 0xFFFF);
      b.best[p] = e;
      b.desc[2 * (size_t)p] = sd[2 * (t + e)];
      b.desc[2 * (size_t)p + 1] = sd[2 * (t + e) + 1];
    }
  }
  // the normal: lane r forms the term of observation r, every lane of the group sums the group's terms in observation order
  float tx = 0.f, ty = 0.f, tz = 0.f;
  if (geom && r < pt.M) normal_term(b.slots[b.obs_slot[pt.obs_off + r]], pt.x, pt.y, pt.z, tx, ty, tz);
  float sx, sy, sz;
  mp_normal_sum_small<W>(tx, ty, tz, gbase, pt.M, sx, sy, sz);
  if (geom && r == 0) write_geometry(b, pt, p, sx, sy, sz);
}

// one wavefront per block: (p, first election row) or (p, -1) for the point's normal and depth
__global__ __launch_bounds__(64) void mpu_large_kernel(MpuBufs b) {
  __shared__ uint32_t hist[64 * MPU_HIST_WORDS];
  const int2 blk = b.large_blocks[blockIdx.x];
  const int p = blk.x, row0 = blk.y, lane = threadIdx.x;
  const MpuPoint pt = b.pts[p];
  if (row0 < 0) {
    // UpdateNormalAndDepth: 64 terms at a time, summed in observation order by every lane (the same value in each)
    float sx, sy, sz;
    mp_normal_sum_large(b.slots, b.obs_slot, pt.obs_off, pt.M, pt.x, pt.y, pt.z, lane, sx, sy, sz);
    if (lane == 0) write_geometry(b, pt, p, sx, sy, sz);
    return;
  }
  const uint32_t key = mp_elect_block(b.rows, b.el_row, pt.el_off, pt.Me, row0, lane, hist);
  if (lane == 0) atomicMin(&b.large_key[p], key);
}

__global__ __launch_bounds__(64) void mpu_finish_kernel(MpuBufs b, int n_large) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= n_large) return;
  const int p = b.large_pts[k];
  const MpuPoint pt = b.pts[p];
  if (!(pt.what & 1) || pt.Me <= 0) return;
  const int e = (int)(b.large_key[p] & 0xFFFF);
  const int row = b.el_row[pt.el_off + e];
  b.best[p] = e;
  b.desc[2 * (size_t)p] = b.rows[2 * (size_t)row];
  b.desc[2 * (size_t)p + 1] = b.rows[2 * (size_t)row + 1];
}

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
