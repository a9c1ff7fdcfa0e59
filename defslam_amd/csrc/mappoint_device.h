// Device functions of MapPoint::UpdateNormalAndDepth (Thirdparty/ORBSLAM_2/src/MapPoint.cc:348-391) and of
// MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:257-325) that more than one kernel file uses: mappoint_kernels.hip
// (dsh_mappoint_update, lists from the host), kfinsert_kernels.hip (dsh_keyframe_process_new and dsh_point_store_upkeep, lists built on
// the device from the store's log) and tmplswitch_kernels.hip (the new points of dsh_template_switch, one observation each); at the end
// the bodies of the election and geometry kernels the first two wrap.  The arithmetic is the one include/defslam_hip.h states for
// dsh_mappoint_update; a file that includes this header is compiled without FMA contraction.
#pragma once
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "mappoint_problem.h"

// one term of UpdateNormalAndDepth's loop (MapPoint.cc:370-374): normali = mWorldPos - Owi, alpha = (float)(1.0 / cv::norm(normali));
// cv::scaleAdd adds normali * alpha to the running sum
__device__ __forceinline__ void normal_term(const MpuSlot& s, float x, float y, float z, float& tx, float& ty, float& tz) {
  const float nx = x - s.Ow[0], ny = y - s.Ow[1], nz = z - s.Ow[2];
  const double nrm = sqrt((double)nx * (double)nx + (double)ny * (double)ny + (double)nz * (double)nz);
  const float a = (float)(1.0 / nrm);
  tx = nx * a;
  ty = ny * a;
  tz = nz * a;
}

// mNormalVector = normal / n (MapPoint.cc:389) into nv[3] and the depth range (:379-388) into mx, mn, from the sum (sx, sy, sz) over the
// M observations, the reference keyframe r and its scale factors at the reference key point's level and at the last level
__device__ __forceinline__ void mp_geometry(int M, float sx, float sy, float sz, const MpuSlot& r, float x, float y, float z, float sf_level,
                                            float sf_last, float* nv, float& mx, float& mn) {
  if (M > 1) {
    const float a = (float)(1.0 / (double)M);   // Mat::convertTo(scale 1.0 / n): cvt_32f's src * a + b with b = 0
    nv[0] = sx * a + 0.0f;
    nv[1] = sy * a + 0.0f;
    nv[2] = sz * a + 0.0f;
  } else {   // n == 1: cv::add(normal, Scalar(0))
    nv[0] = sx + 0.0f;
    nv[1] = sy + 0.0f;
    nv[2] = sz + 0.0f;
  }
  const float px = x - r.Ow[0], py = y - r.Ow[1], pz = z - r.Ow[2];
  const float dist = (float)sqrt((double)px * (double)px + (double)py * (double)py + (double)pz * (double)pz);
  mx = dist * sf_level;
  mn = mx / sf_last;
}

__device__ __forceinline__ int mp_hamming(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) +
         __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// The election of a small point by a group of W lanes, one lane per election row: lane r holds row r in (d0, d1) and the group's rows lie
// in LDS at gd[2 * j], gd[2 * j + 1] (zeros past Me).  Returns the (median << 16 | row) minimum of the group, in every lane of the group.
template <int W>
__device__ __forceinline__ uint32_t mp_elect_small(const uint4 d0, const uint4 d1, const uint4* gd, int Me, int r) {
  // row r of D as 16-bit distances; columns past Me hold 511, above every value the bisection tests
  uint32_t dd[W / 2];
#pragma unroll
  for (int j = 0; j < W; j += 2) {
    const int a = j < Me ? mp_hamming(d0, d1, gd[2 * j], gd[2 * j + 1]) : 511;
    const int c = j + 1 < Me ? mp_hamming(d0, d1, gd[2 * j + 2], gd[2 * j + 3]) : 511;
    dd[j / 2] = (uint32_t)a | ((uint32_t)c << 16);
  }
  // the smallest v with #{j : D[r][j] <= v} > floor((Me-1)/2): sorted(row)[(size_t)(0.5 * (Me - 1))] (MapPoint.cc:311-313)
  const int kth = (Me - 1) / 2;
  int lo = 0, hi = 256;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < W / 2; j++) cnt += (int)((dd[j] & 0xFFFF) <= (uint32_t)mid) + (int)((dd[j] >> 16) <= (uint32_t)mid);
    if (cnt > kth) hi = mid;
    else lo = mid + 1;
  }
  uint32_t key = r < Me ? ((uint32_t)lo << 16) | (uint32_t)r : 0xFFFFFFFFu;
  // the first row with a strictly smaller median (MapPoint.cc:315-319): the (median, row) minimum of the group
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)key, o, 64);
    key = other < key ? other : key;
  }
  return key;
}

// The normal's sum of a small point: lane r of the group holds the term of observation r (zeros past M), gbase is the group's first lane
// in the wavefront; every lane of the group sums the group's terms in observation order.
template <int W>
__device__ __forceinline__ void mp_normal_sum_small(float tx, float ty, float tz, int gbase, int M, float& sx, float& sy, float& sz) {
  sx = sy = sz = 0.f;
#pragma unroll
  for (int j = 0; j < W; j++) {
    const float ux = __shfl(tx, gbase + j, 64), uy = __shfl(ty, gbase + j, 64), uz = __shfl(tz, gbase + j, 64);
    if (j < M) {
      sx = ux + sx;
      sy = uy + sy;
      sz = uz + sz;
    }
  }
}

// The normal's sum of a large point by one wavefront: 64 terms at a time over the observation slots obs_slot[obs_off .. obs_off + M),
// summed in observation order by every lane (the same value in each).
__device__ __forceinline__ void mp_normal_sum_large(const MpuSlot* slots, const int32_t* obs_slot, int obs_off, int M, float x, float y, float z,
                                                    int lane, float& sx, float& sy, float& sz) {
  sx = sy = sz = 0.f;
  for (int base = 0; base < M; base += 64) {
    float tx = 0.f, ty = 0.f, tz = 0.f;
    if (base + lane < M) normal_term(slots[obs_slot[obs_off + base + lane]], x, y, z, tx, ty, tz);
    const int cnt = min(64, M - base);
    for (int l = 0; l < cnt; l++) {
      sx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tx), l)) + sx;
      sy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ty), l)) + sy;
      sz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tz), l)) + sz;
    }
  }
}

// One block of 64 election rows of a large point by one wavefront: lane `lane` owns row row0 + lane of el_row[el_off .. el_off + Me) and counts its
// distances to every election row into its own histogram hist[lane * MPU_HIST_WORDS ..] in LDS.  Returns the (median << 16 | row) minimum
// of the block, in every lane.
__device__ __forceinline__ uint32_t mp_elect_block(const uint4* rows, const int32_t* el_row, int el_off, int Me, int row0, int lane,
                                                   uint32_t* hist) {
  const int i = row0 + lane;
  const bool valid = i < Me;
  uint32_t* h = hist + lane * MPU_HIST_WORDS;
  for (int w = 0; w < MPU_HIST_WORDS; w++) h[w] = 0;
  uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
  if (valid) {
    const int row = el_row[el_off + i];
    d0 = rows[2 * (size_t)row];
    d1 = rows[2 * (size_t)row + 1];
  }
  // each lane's histogram is its own: plain read-modify-write, no atomics.  Counts <= Me <= 65535 fit their 16 bits.
  for (int j = 0; j < Me; j++) {
    const int row = el_row[el_off + j];
    const int dist = mp_hamming(d0, d1, rows[2 * (size_t)row], rows[2 * (size_t)row + 1]);
    if (valid) h[dist >> 1] += 1u << ((dist & 1) << 4);
  }
  const int kth = (Me - 1) / 2;
  int med = 256, cum = 0;
  for (int w = 0; w < MPU_HIST_WORDS; w++) {
    const uint32_t v = h[w];
    const int lo = (int)(v & 0xFFFF), hi = (int)(v >> 16);
    if (cum + lo > kth) { med = 2 * w; break; }
    cum += lo;
    if (cum + hi > kth) { med = 2 * w + 1; break; }
    cum += hi;
  }
  uint32_t key = valid ? ((uint32_t)med << 16) | (uint32_t)i : 0xFFFFFFFFu;
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)key, o, 64);
    key = other < key ? other : key;
  }
  return key;
}

// ---- the bodies of the election and geometry kernels -------------------------------------------------------------------------------
// A kernel hands its body a view V of where its work comes from and where the results go:
//   v.b                 the buffers: pts, el_row, rows, slots, obs_slot, large_blocks, large_key
//   v.list, v.n         the list the kernel works on and its length (the large body reads v.b.large_blocks)
//   v.id(k)             the id under which point k of pts is stored
//   v.store_desc(id, e, d0, d1), v.normal(id), v.store_depth(id, mx, mn)   the elected row e with its descriptor; the normal; the depth range

// mNormalVector = normal / n (MapPoint.cc:389) and the depth range (:379-388), written by one lane
template <class V>
__device__ __forceinline__ void mp_store_geometry(const V& v, const MpuPoint& pt, int id, float sx, float sy, float sz) {
  float mx, mn;
  mp_geometry(pt.M, sx, sy, sz, v.b.slots[pt.ref_slot], pt.x, pt.y, pt.z, pt.sf_level, pt.sf_last, v.normal(id), mx, mn);
  v.store_depth(id, mx, mn);
}

// The small points of one width class: W lanes per point, a block of 256 threads serves 256 / W points of v.list; sd: 2 x 256 uint4 of LDS
template <int W, class V>
__device__ __forceinline__ void mp_small_body(const V& v, uint4* sd) {
  if (blockIdx.x * (256 / W) >= v.n) return;   // workgroup-uniform: a grid sized for the worst case
  const int t = threadIdx.x, r = t % W, g = t / W, gbase = (t & 63) - r;   // gbase: the group's first lane in the wavefront
  const int kk = blockIdx.x * (256 / W) + g;
  const bool has = kk < v.n;
  const int k = has ? v.list[kk] : 0;
  MpuPoint pt;
  if (has) pt = v.b.pts[k];
  else { pt.M = pt.Me = 0; pt.what = 0; pt.x = pt.y = pt.z = 0.f; }
  const int id = has ? v.id(k) : 0;
  const bool elect = (pt.what & 1) && pt.Me > 0, geom = (pt.what & 2) && pt.M > 0;
  uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
  if (elect && r < pt.Me) {
    const int row = v.b.el_row[pt.el_off + r];
    d0 = v.b.rows[2 * (size_t)row];
    d1 = v.b.rows[2 * (size_t)row + 1];
  }
  sd[2 * t] = d0;
  sd[2 * t + 1] = d1;
  __syncthreads();
  if (elect) {
    const uint32_t key = mp_elect_small<W>(d0, d1, sd + 2 * (t - r), pt.Me, r);
    if (r == 0) {
      const int e = (int)(key & 0xFFFF);
      v.store_desc(id, e, sd[2 * (t + e)], sd[2 * (t + e) + 1]);
    }
  }
  // the normal: lane r forms the term of observation r, every lane of the group sums the group's terms in observation order
  float tx = 0.f, ty = 0.f, tz = 0.f;
  if (geom && r < pt.M) normal_term(v.b.slots[v.b.obs_slot[pt.obs_off + r]], pt.x, pt.y, pt.z, tx, ty, tz);
  float sx, sy, sz;
  mp_normal_sum_small<W>(tx, ty, tz, gbase, pt.M, sx, sy, sz);
  if (geom && r == 0) mp_store_geometry(v, pt, id, sx, sy, sz);
}

// The large points: one wavefront strides over the v.n entries of large_blocks, (k, first election row) or (k, -1) for the point's normal
// and depth; blocks publish their (median << 16 | row) minimum in large_key[k].  hist: 64 x MPU_HIST_WORDS words of LDS
template <class V>
__device__ __forceinline__ void mp_large_body(const V& v, uint32_t* hist) {
  const int lane = threadIdx.x;
  for (int bi = blockIdx.x; bi < v.n; bi += gridDim.x) {
    const int2 blk = v.b.large_blocks[bi];
    const int k = blk.x, row0 = blk.y;
    const MpuPoint pt = v.b.pts[k];
    if (row0 < 0) {
      // UpdateNormalAndDepth: 64 terms at a time, summed in observation order by every lane (the same value in each)
      float sx, sy, sz;
      mp_normal_sum_large(v.b.slots, v.b.obs_slot, pt.obs_off, pt.M, pt.x, pt.y, pt.z, lane, sx, sy, sz);
      if (lane == 0) mp_store_geometry(v, pt, v.id(k), sx, sy, sz);
      continue;
    }
    const uint32_t key = mp_elect_block(v.b.rows, v.b.el_row, pt.el_off, pt.Me, row0, lane, hist);   // each lane clears its own histogram
    if (lane == 0) atomicMin(&v.b.large_key[k], key);
  }
}

// The winner's descriptor row of the large points v.list[0 .. v.n), a thread per point
template <class V>
__device__ __forceinline__ void mp_finish_body(const V& v) {
  for (int i = blockIdx.x * 64 + threadIdx.x; i < v.n; i += gridDim.x * 64) {
    const int k = v.list[i];
    const MpuPoint pt = v.b.pts[k];
    if (!(pt.what & 1) || pt.Me <= 0) continue;
    const int e = (int)(v.b.large_key[k] & 0xFFFF), row = v.b.el_row[pt.el_off + e];
    v.store_desc(v.id(k), e, v.b.rows[2 * (size_t)row], v.b.rows[2 * (size_t)row + 1]);
  }
}
