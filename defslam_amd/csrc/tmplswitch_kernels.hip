// The template switch on the map point store (dsh_need_new_template, dsh_template_switch, dsh_surface_vertices and the read-backs
// dsh_point_store_get_points, dsh_point_store_get_embedding; gfx950).
//   DefLocalMapping::needNewTemplate      Modules/Mapping/DefLocalMapping.cc:355-404
//   DefLocalMapping::CreateNewMapPoints   DefLocalMapping.cc:240-347
//   Surface::getVertex, the Node positions  Modules/Mapping/Surface.cc:125-161, Modules/Template/TriangularMesh.cc:71-84
// A switch is three launches: ts_classify_kernel and ts_create_kernel here, over the keyframe's key points, and embed_store_kernel
// (register_kernels.hip) over the store's points.  The occupancy mask is not rasterised: a key point is masked when a held pixel lies in
// the interval of source pixels its reflected box window reads (include/defslam_hip.h), so every key point walks the keyframe's held
// pixels, staged through LDS a workgroup's worth at a time -- N^2 integer tests, about a million at the reference's 1200 key points.
// The same walk finds the held points that a later key point holds again.  New ids are a prefix sum over the key points: the classify
// launch leaves a count per workgroup, every workgroup of the create launch sums the counts in front of it and ranks its own key points
// by ballot.  These kernels are launch- and latency-bound.  Compiled without FMA contraction: the float32 expression order of the
// reference is kept (see include/defslam_hip.h).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "mappoint_device.h"
#include "mpdb_device.h"
#include "tmplswitch_problem.h"

namespace {

// the source pixels [L, H] that the box window of pixel x reads along an axis of n pixels: kernel size k, anchor a, BORDER_REFLECT_101
__device__ __forceinline__ void ts_window(int x, int k, int a, int n, int& L, int& H) {
  const int lo = x - a, hi = x + k - 1 - a;
  L = max(lo, 0);
  H = min(hi, n - 1);
  if (lo < 0) H = max(H, -lo);
  if (hi > n - 1) L = min(L, 2 * (n - 1) - hi);
}

// x3wh = Twc * x3ch of float cv::Mat: per row the four products summed left to right in float32 (the fourth factor is 1)
__device__ __forceinline__ void ts_to_world(const float* T, float x, float y, float z, float* w) {
#pragma unroll
  for (int r = 0; r < 3; r++) w[r] = ((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z) + T[4 * r + 3] * 1.0f;
}

__global__ __launch_bounds__(TS_BLOCK) void ts_classify_kernel(TcState s, TsSwitch k) {
  __shared__ int sx[TS_BLOCK], sy[TS_BLOCK], sp[TS_BLOCK];   // a chunk of key points: pixel, and the point held if it is not bad (else -1)
  const int t = threadIdx.x, i = blockIdx.x * TS_BLOCK + t;
  const int ks = k.cols / 20, a = ks / 2;
  int qx = 0, qy = 0, p = -1;
  bool good = false;
  if (i < k.N) {
    qx = (int)k.kp[2 * (size_t)i];
    qy = (int)k.kp[2 * (size_t)i + 1];
    p = k.table[k.tab_off + i];
    good = p >= 0 && !s.bad[p];
  }
  int Lx, Hx, Ly, Hy;
  ts_window(qx, ks, a, k.cols, Lx, Hx);
  ts_window(qy, ks, a, k.rows, Ly, Hy);
  bool masked = false, again = false;
  for (int base = 0; base < k.N; base += TS_BLOCK) {
    const int j = base + t;
    __syncthreads();
    sp[t] = -1;
    if (j < k.N) {
      const int pj = k.table[k.tab_off + j];
      sx[t] = (int)k.kp[2 * (size_t)j];
      sy[t] = (int)k.kp[2 * (size_t)j + 1];
      sp[t] = pj >= 0 && !s.bad[pj] ? pj : -1;
    }
    __syncthreads();
    const int m = min(TS_BLOCK, k.N - base);
    for (int l = 0; l < m; l++) {
      const int pj = sp[l];
      if (pj < 0) continue;
      masked = masked || (Lx <= sx[l] && sx[l] <= Hx && Ly <= sy[l] && sy[l] <= Hy);
      again = again || (pj == p && base + l > i);
    }
  }
  int c = -1;
  if (i < k.N) {
    c = p >= 0 ? (good ? (again ? TS_HELD_AGAIN : TS_HELD) : TS_HELD_BAD) : (masked ? TS_MASKED : TS_NEW);
    k.cls[i] = (uint8_t)c;
    if (k.candidate) k.candidate[i] = c == TS_NEW ? 1 : 0;
  }
  // n_new, n_moved, n_masked of the workgroup
  const bool f[3] = {c == TS_NEW, c == TS_HELD || c == TS_HELD_AGAIN, c == TS_MASKED};
  const int n = block_sums<TS_BLOCK, 3>(f);
  if (t < 3) {
    if (t == 0) k.block_new[blockIdx.x] = n;
    int32_t* dst = t == 0 ? &k.counts->c.n_new : t == 1 ? &k.counts->c.n_moved : &k.counts->c.n_masked;
    if (n) atomicAdd(dst, n);
  }
}

__global__ __launch_bounds__(TS_BLOCK) void ts_create_kernel(TcState s, TsSwitch k) {
  __shared__ int wsum[TS_BLOCK / 64];
  const int t = threadIdx.x, i = blockIdx.x * TS_BLOCK + t, wave = t >> 6, lane = t & 63;
  // the new points of the workgroups in front of this one
  int front = 0;
  for (int b = t; b < (int)blockIdx.x; b += TS_BLOCK) front += k.block_new[b];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) front += __shfl_xor(front, m, 64);
  if (lane == 0) wsum[wave] = front;
  __syncthreads();
  int j = 0;
#pragma unroll
  for (int w = 0; w < TS_BLOCK / 64; w++) j += wsum[w];
  const int c = i < k.N ? k.cls[i] : -1;
  int total;
  j += tile_rank<TS_BLOCK>(c == TS_NEW, wsum, total);   // its first barrier: the sums in front have been read
  if (c != TS_HELD && c != TS_NEW) return;

  float w3[3];
  ts_to_world(k.Twc, k.surface[3 * (size_t)i], k.surface[3 * (size_t)i + 1], k.surface[3 * (size_t)i + 2], w3);   // DefLocalMapping.cc:282-298, :318-333
  if (c == TS_HELD) {
    const size_t p = (size_t)k.table[k.tab_off + i];
    for (int r = 0; r < 3; r++) s.xyz[3 * p + r] = w3[r];   // SetWorldPos (:305, :309)
    return;
  }
  // new DefMapPoint(x3w, referenceKF_, map), AddObservation, addMapPoint, ComputeDistinctiveDescriptors, UpdateNormalAndDepth (:335-342)
  const size_t p = (size_t)k.P + j;
  for (int r = 0; r < 3; r++) {
    s.xyz[3 * p + r] = w3[r];
    s.nodes[3 * p + r] = -1;
    s.bary[3 * p + r] = 0.0;
  }
  s.bad[p] = 0;
  s.visible[p] = 1;
  s.found[p] = 1;
  s.nobs[p] = 1;
  k.log[k.R + j] = make_int2((int)p, k.slot);
  k.log_idx[k.R + j] = i;   // the observation's key point, and mpRefKF = referenceKF_ (what dsh_keyframe_anchors reads)
  k.ref_kf[p] = k.slot;
  k.table[k.tab_off + i] = (int)p;
  const MpuSlot kf = k.kf_slots[k.slot];
  k.desc[2 * p] = k.kf_rows[2 * ((size_t)kf.row_off + i)];   // one observation: its descriptor is elected
  k.desc[2 * p + 1] = k.kf_rows[2 * ((size_t)kf.row_off + i) + 1];
  float tx, ty, tz, mx, mn;
  normal_term(kf, w3[0], w3[1], w3[2], tx, ty, tz);
  mp_geometry(1, tx + 0.0f, ty + 0.0f, tz + 0.0f, kf, w3[0], w3[1], w3[2], k.sf[k.octave[i]], k.sf[k.levels - 1], k.normal + 3 * p, mx, mn);
  k.max_distance[p] = mx;
  k.new_idx[j] = i;
}

__global__ __launch_bounds__(TS_BLOCK) void ts_max_node_kernel(const int32_t* nodes, int P, int32_t* out) {
  const int p = blockIdx.x * TS_BLOCK + threadIdx.x;
  int v = p < P ? nodes[3 * (size_t)p + 2] : -1;   // ascending: the third is the largest
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
  if ((threadIdx.x & 63) == 0 && v >= 0) atomicMax(out, v);
}

// Surface.cc:152-159 and the Node constructor's arguments (TriangularMesh.cc:71-84)
__global__ __launch_bounds__(TS_BLOCK) void ts_vertices_kernel(const double* u, const double* v, const double* d, const float* Twc, int n, double* nodes_xyz) {
  const int i = blockIdx.x * TS_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float x = (float)(u[i] * d[i]), y = (float)(v[i] * d[i]), z = (float)d[i];
  float w3[3];
  ts_to_world(Twc, x, y, z, w3);
  for (int r = 0; r < 3; r++) nodes_xyz[3 * (size_t)i + r] = (double)w3[r];
}

__global__ __launch_bounds__(TS_BLOCK) void ts_get_points_kernel(TcState s, const float* normal, const float* max_distance, const uint4* desc,
                                                                 const int32_t* ids, int n, float* xyz, float* onormal, float* omaxd, uint4* odesc,
                                                                 uint8_t* obad) {
  const int i = blockIdx.x * TS_BLOCK + threadIdx.x;
  if (i >= n) return;
  const size_t p = (size_t)ids[i];
  for (int r = 0; r < 3; r++) {
    if (xyz) xyz[3 * (size_t)i + r] = s.xyz[3 * p + r];
    if (onormal) onormal[3 * (size_t)i + r] = normal[3 * p + r];
  }
  if (omaxd) omaxd[i] = max_distance[p];
  if (odesc) {
    odesc[2 * (size_t)i] = desc[2 * p];
    odesc[2 * (size_t)i + 1] = desc[2 * p + 1];
  }
  if (obad) obad[i] = s.bad[p] ? 1 : 0;
}

__global__ __launch_bounds__(TS_BLOCK) void ts_get_embedding_kernel(TcState s, const int32_t* ids, int n, int32_t* nodes, double* bary) {
  const int i = blockIdx.x * TS_BLOCK + threadIdx.x;
  if (i >= n) return;
  const size_t p = (size_t)ids[i];
  for (int r = 0; r < 3; r++) {
    if (nodes) nodes[3 * (size_t)i + r] = s.nodes[3 * p + r];
    if (bary) bary[3 * (size_t)i + r] = s.bary[3 * p + r];
  }
}

}  // namespace

static_assert(sizeof(dsh_template_switch_counts) == 24 && sizeof(TsCounts) == 32, "dsh_template_switch_counts is six int32");

extern "C" hipError_t ts_classify_launch(const TcState& s, const TsSwitch& k, hipStream_t st) {
  if (k.N > 0) hipLaunchKernelGGL(ts_classify_kernel, blocks_for(k.N, TS_BLOCK), dim3(TS_BLOCK), 0, st, s, k);
  return hipGetLastError();
}

extern "C" hipError_t ts_create_launch(const TcState& s, const TsSwitch& k, hipStream_t st) {
  if (k.N > 0) hipLaunchKernelGGL(ts_create_kernel, blocks_for(k.N, TS_BLOCK), dim3(TS_BLOCK), 0, st, s, k);
  return hipGetLastError();
}

extern "C" hipError_t ts_max_node_launch(const int32_t* nodes, int P, int32_t* out, hipStream_t st) {
  if (P > 0) hipLaunchKernelGGL(ts_max_node_kernel, blocks_for(P, TS_BLOCK), dim3(TS_BLOCK), 0, st, nodes, P, out);
  return hipGetLastError();
}

extern "C" hipError_t ts_vertices_launch(const double* u, const double* v, const double* d, const float* Twc, int n, double* nodes_xyz, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(ts_vertices_kernel, blocks_for(n, TS_BLOCK), dim3(TS_BLOCK), 0, st, u, v, d, Twc, n, nodes_xyz);
  return hipGetLastError();
}

extern "C" hipError_t ts_get_points_launch(const TcState& s, const float* normal, const float* max_distance, const uint4* desc, const int32_t* ids, int n,
                                           float* xyz, float* onormal, float* omaxd, uint4* odesc, uint8_t* obad, hipStream_t st) {
  if (n > 0)
    hipLaunchKernelGGL(ts_get_points_kernel, blocks_for(n, TS_BLOCK), dim3(TS_BLOCK), 0, st, s, normal, max_distance, desc, ids, n, xyz, onormal, omaxd, odesc, obad);
  return hipGetLastError();
}

extern "C" hipError_t ts_get_embedding_launch(const TcState& s, const int32_t* ids, int n, int32_t* nodes, double* bary, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(ts_get_embedding_kernel, blocks_for(n, TS_BLOCK), dim3(TS_BLOCK), 0, st, s, ids, n, nodes, bary);
  return hipGetLastError();
}
