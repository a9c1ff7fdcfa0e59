// The per-point tracking state of the map point store and the back half of DefTracking::TrackLocalMap on it (dsh_trackstate_*,
// dsh_track_close_frame; gfx950).
//   DefPoseOptimization's write-back    Modules/Tracking/DefOptimizer.cc:568-576 -> DefMapPoint::RecalculatePosition (DefMapPoint.cc:129-147)
//   the counting loops of TrackLocalMap  Modules/Tracking/DefTracking.cc:253-319
//   LocalMapping::MapPointCulling        Thirdparty/ORBSLAM_2/src/LocalMapping.cc:173-199
// Closing a frame is at most three launches: tc_repose_kernel over the store's points, tc_frame_kernel over the frame's key points,
// tc_frustum_kernel over the reference list.  Everything but the repose is integer valued.  A count is a ballot per wavefront, summed per
// workgroup in LDS, and leaves with one atomic per workgroup and counter; mnFound / mnVisible / nObs are integer atomics on the point
// arrays (a point is held by a handful of key points, and integer adds commute: the result does not depend on the order).
// The repose keeps the reference's double expression (b1 * x1 + b2 * x2) + b3 * x3 with every product and sum rounded (_rn intrinsics),
// then one rounding to float; the frustum test is track_frustum.h, the one the local-map search applies.
#include "mpdb_device.h"
#include "track_frustum.h"
#include "trackclose_problem.h"

namespace {

// flags[c] of every thread of the workgroup counted into dst[c]; every thread of the workgroup calls it (it holds a barrier)
template <int NC>
__device__ __forceinline__ void block_count(const bool (&flags)[NC], int32_t* dst) {
  const int s = block_sums<TC_BLOCK, NC>(flags);
  if (s) atomicAdd(dst + threadIdx.x, s);   // s is 0 in the threads from NC on
}

__global__ __launch_bounds__(TC_BLOCK) void tc_init_points_kernel(TcState s, int first, int n) {
  const int i = blockIdx.x * TC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const size_t p = (size_t)first + i;
  s.visible[p] = 1;
  s.found[p] = 1;
  s.nobs[p] = 0;
  for (int k = 0; k < 3; k++) { s.nodes[3 * p + k] = -1; s.bary[3 * p + k] = 0.0; }
}

__global__ __launch_bounds__(TC_BLOCK) void tc_add_by_index_kernel(int32_t* dst, const int32_t* src, int stride, int32_t delta, int n) {
  const int i = blockIdx.x * TC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int p = src[(size_t)i * stride];
  if (p >= 0) atomicAdd(&dst[p], delta);
}

__global__ __launch_bounds__(TC_BLOCK) void tc_add_by_record_kernel(int32_t* dst, const int32_t* src, const int32_t* idx, int32_t delta, int n) {
  const int i = blockIdx.x * TC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int p = src[idx[i]];
  if (p >= 0) atomicAdd(&dst[p], delta);
}

__global__ __launch_bounds__(TC_BLOCK) void tc_visible_kernel(int32_t* visible, const int32_t* cnt, int P_cnt, const int32_t* local_ids,
                                                               const int32_t* inview, int Q, const int32_t* refused) {
  if (refused && *refused) return;
  const int i = blockIdx.x * TC_BLOCK + threadIdx.x;
  if (i < P_cnt) {
    const int k = cnt[i];                                          // Tracking.cc:1408-1425: once per key point that holds the point
    if (k > 0) atomicAdd(&visible[i], k);
  }
  if (i < Q && inview[i]) atomicAdd(&visible[local_ids[i]], 1);   // :1456
}

__global__ __launch_bounds__(TC_BLOCK) void tc_set_embedding_kernel(TcState s, const int32_t* ids, const int32_t* src_nodes, const double* src_bary,
                                                                     int n) {
  const int i = blockIdx.x * TC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const size_t p = ids ? (size_t)ids[i] : (size_t)i;
  const bool facet = ids && src_nodes[3 * i] >= 0;
  for (int k = 0; k < 3; k++) {
    s.nodes[3 * p + k] = facet ? src_nodes[3 * i + k] : -1;
    s.bary[3 * p + k] = facet ? src_bary[3 * i + k] : 0.0;
  }
}

__global__ __launch_bounds__(TC_BLOCK) void tc_set_counters_kernel(TcState s, const int32_t* ids, const int32_t* visible, const int32_t* found, int n) {
  const int i = blockIdx.x * TC_BLOCK + threadIdx.x;
  if (i >= n) return;
  s.visible[ids[i]] = visible[i];
  s.found[ids[i]] = found[i];
}

__global__ __launch_bounds__(TC_BLOCK) void tc_get_kernel(TcState s, const int32_t* ids, int n, int32_t* visible, int32_t* found, int32_t* nobs,
                                                           float* xyz) {
  const int i = blockIdx.x * TC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const size_t p = (size_t)ids[i];
  if (visible) visible[i] = s.visible[p];
  if (found) found[i] = s.found[p];
  if (nobs) nobs[i] = s.nobs[p];
  if (xyz)
    for (int k = 0; k < 3; k++) xyz[3 * (size_t)i + k] = s.xyz[3 * p + k];
}

// DefMapPoint::RecalculatePosition of every point the loop over Map::GetAllMapPoints reaches: not bad (setBadFlag erased it from the
// map) and with a facet
__global__ __launch_bounds__(TC_BLOCK) void tc_repose_kernel(TcState s, int P, const double* node_xyz, int32_t* n_moved) {
  const int p = blockIdx.x * TC_BLOCK + threadIdx.x;
  bool moved[1] = {false};
  if (p < P && !s.bad[p]) {
    const int n0 = s.nodes[3 * (size_t)p], n1 = s.nodes[3 * (size_t)p + 1], n2 = s.nodes[3 * (size_t)p + 2];
    if (n0 >= 0) {
      const double b0 = s.bary[3 * (size_t)p], b1 = s.bary[3 * (size_t)p + 1], b2 = s.bary[3 * (size_t)p + 2];
      for (int k = 0; k < 3; k++)
        s.xyz[3 * (size_t)p + k] = (float)__dadd_rn(__dadd_rn(__dmul_rn(b0, node_xyz[3 * (size_t)n0 + k]), __dmul_rn(b1, node_xyz[3 * (size_t)n1 + k])),
                                                    __dmul_rn(b2, node_xyz[3 * (size_t)n2 + k]));
      moved[0] = true;
    }
  }
  block_count<1>(moved, n_moved);
}

// DefTracking.cc:257-283 and :300-319, one thread per key point
__global__ __launch_bounds__(TC_BLOCK) void tc_frame_kernel(TcState s, TcClose k) {
  const int i = blockIdx.x * TC_BLOCK + threadIdx.x;
  // matches_inliers, matches_outliers, to_match_local, observed, inliers, outliers: the first six fields of dsh_track_close_counts
  bool f[6] = {false, false, false, false, false, false};
  const int p = i < k.N ? k.frame_points[i] : -1;
  if (p >= 0) {
    const bool out = k.outlier[i] != 0;
    if (!out) {
      atomicAdd(&s.found[p], 1);                                   // IncreaseFound (:263): per key point, no isBad test
      if (!k.only_tracking) {
        if (s.nobs[p] > 0) {                                       // Observations() (:266) is nObs, which setBadFlag leaves as it was
          f[0] = true;
          if (s.nodes[3 * (size_t)p] >= 0) f[2] = true;            // getFacet() (:269-272)
        }
      } else {
        f[0] = true;
      }
    } else {
      f[1] = true;
    }
    if (!s.bad[p]) {                                               // :307
      f[3] = true;
      f[out ? 5 : 4] = true;
    }
  }
  block_count<6>(f, &k.counts->matches_inliers);
}

// DefTracking.cc:284-298 over Map::GetReferenceMapPoints(), one thread per entry
__global__ __launch_bounds__(TC_BLOCK) void tc_frustum_kernel(TcState s, TcClose k) {
  const int i = blockIdx.x * TC_BLOCK + threadIdx.x;
  bool in[1] = {false};
  if (i < k.n_ref) {
    const size_t p = (size_t)k.ref_ids[i];
    if (!s.bad[p] && s.nodes[3 * p] >= 0) {
      TrkView w;
      in[0] = trk_in_frustum(*k.pose, s.xyz[3 * p], s.xyz[3 * p + 1], s.xyz[3 * p + 2], k.normal[3 * p], k.normal[3 * p + 1], k.normal[3 * p + 2], w);
    }
  }
  block_count<1>(in, &k.counts->local_map_points);
}

__global__ __launch_bounds__(TC_BLOCK) void tc_cull_kernel(TcState s, const int32_t* ids, const int32_t* first_kf, int32_t current_kf, int n,
                                                            uint8_t* action) {
  const int i = blockIdx.x * TC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int p = ids[i];
  const uint8_t a = tc_cull_action(s.bad[p], s.found[p], s.visible[p], current_kf, first_kf[i]);
  if (a == 2) s.bad[p] = 1;
  action[i] = a;
}

}  // namespace

static_assert(sizeof(dsh_track_close_counts) == 32, "dsh_track_close_counts is eight int32");

extern "C" hipError_t tc_init_points_launch(const TcState& s, int first, int n, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(tc_init_points_kernel, blocks_for(n, TC_BLOCK), dim3(TC_BLOCK), 0, st, s, first, n);
  return hipGetLastError();
}

extern "C" hipError_t tc_add_by_index_launch(int32_t* dst, const int32_t* src, int stride, int32_t delta, int n, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(tc_add_by_index_kernel, blocks_for(n, TC_BLOCK), dim3(TC_BLOCK), 0, st, dst, src, stride, delta, n);
  return hipGetLastError();
}

extern "C" hipError_t tc_add_by_record_launch(int32_t* dst, const int32_t* src, const int32_t* idx, int32_t delta, int n, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(tc_add_by_record_kernel, blocks_for(n, TC_BLOCK), dim3(TC_BLOCK), 0, st, dst, src, idx, delta, n);
  return hipGetLastError();
}

extern "C" hipError_t tc_visible_launch(int32_t* visible, const int32_t* cnt, int P_cnt, const int32_t* local_ids, const int32_t* inview, int Q,
                                        const int32_t* refused, hipStream_t st) {
  const int top = P_cnt > Q ? P_cnt : Q;
  if (top > 0) hipLaunchKernelGGL(tc_visible_kernel, blocks_for(top, TC_BLOCK), dim3(TC_BLOCK), 0, st, visible, cnt, P_cnt, local_ids, inview, Q, refused);
  return hipGetLastError();
}

extern "C" hipError_t tc_set_embedding_launch(const TcState& s, const int32_t* ids, const int32_t* src_nodes, const double* src_bary, int n, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(tc_set_embedding_kernel, blocks_for(n, TC_BLOCK), dim3(TC_BLOCK), 0, st, s, ids, src_nodes, src_bary, n);
  return hipGetLastError();
}

extern "C" hipError_t tc_set_counters_launch(const TcState& s, const int32_t* ids, const int32_t* visible, const int32_t* found, int n, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(tc_set_counters_kernel, blocks_for(n, TC_BLOCK), dim3(TC_BLOCK), 0, st, s, ids, visible, found, n);
  return hipGetLastError();
}

extern "C" hipError_t tc_get_launch(const TcState& s, const int32_t* ids, int n, int32_t* visible, int32_t* found, int32_t* nobs, float* xyz,
                                    hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(tc_get_kernel, blocks_for(n, TC_BLOCK), dim3(TC_BLOCK), 0, st, s, ids, n, visible, found, nobs, xyz);
  return hipGetLastError();
}

extern "C" hipError_t tc_repose_launch(const TcState& s, int P, const double* node_xyz, int32_t* n_moved, hipStream_t st) {
  if (P > 0) hipLaunchKernelGGL(tc_repose_kernel, blocks_for(P, TC_BLOCK), dim3(TC_BLOCK), 0, st, s, P, node_xyz, n_moved);
  return hipGetLastError();
}

extern "C" hipError_t tc_close_launch(const TcState& s, const TcClose& k, hipStream_t st) {
  if (k.node_xyz && k.P > 0) hipLaunchKernelGGL(tc_repose_kernel, blocks_for(k.P, TC_BLOCK), dim3(TC_BLOCK), 0, st, s, k.P, k.node_xyz, &k.counts->n_moved);
  if (k.N > 0) hipLaunchKernelGGL(tc_frame_kernel, blocks_for(k.N, TC_BLOCK), dim3(TC_BLOCK), 0, st, s, k);
  if (k.n_ref > 0) hipLaunchKernelGGL(tc_frustum_kernel, blocks_for(k.n_ref, TC_BLOCK), dim3(TC_BLOCK), 0, st, s, k);
  return hipGetLastError();
}

extern "C" hipError_t tc_cull_launch(const TcState& s, const int32_t* ids, const int32_t* first_kf, int32_t current_kf, int n, uint8_t* action,
                                     hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(tc_cull_kernel, blocks_for(n, TC_BLOCK), dim3(TC_BLOCK), 0, st, s, ids, first_kf, current_kf, n, action);
  return hipGetLastError();
}
