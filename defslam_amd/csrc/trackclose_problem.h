// Device-side layout of the per-point tracking state of the map point store and of closing a tracked frame (dsh_trackstate_*,
// dsh_track_close_frame: dsh_trackclose.cpp and dsh_localmap.cpp -> trackclose_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/defslam_hip.h"
#include "track_problem.h"

#define TC_BLOCK 256

// the tracking state of the store's points
struct TcState {
  float* xyz;              // 3 per point
  int32_t* bad;
  int32_t* visible;        // mnVisible
  int32_t* found;          // mnFound
  int32_t* nobs;           // MapPoint::nObs
  int32_t* nodes;          // 3 per point, ascending, -1 -1 -1: no facet
  double* bary;            // 3 per point, in the order of nodes
};

// one dsh_track_close_frame: the upload block's slices and the list the frustum count walks
struct TcClose {
  const TrkProb* pose;             // R, t, Ow, the camera and the image bounds
  const int32_t* frame_points;     // N: mvpMapPoints as ids or -1
  const uint8_t* outlier;          // N: mvbOutlier
  const double* node_xyz;          // n_nodes x 3, or null: no repose
  const int32_t* ref_ids;          // n_ref: the local points before the last dsh_local_map_update
  const float* normal;             // 3 per point of the store
  int32_t P, N, n_ref, only_tracking;
  dsh_track_close_counts* counts;  // zero on entry
};

// LocalMapping::MapPointCulling's decision for one entry of mlpRecentAddedMapPoints (LocalMapping.cc:184-197), the first case that applies:
// 1 already bad, 2 GetFoundRatio() < 0.40f (MapPoint.cc:251-255), 3 old enough to leave the list, 0 stays.  tc_cull_kernel and the
// select stage of dsh_point_store_cull (pointerase_kernels.hip) share it.
__device__ __forceinline__ uint8_t tc_cull_action(int bad, int found, int visible, int32_t current_kf, int32_t first_kf) {
  if (bad) return 1;                                                         // :184
  if (__fdiv_rn((float)found, (float)visible) < 0.40f) return 2;             // :188
  if (current_kf - first_kf >= 3) return 3;                                  // :194
  return 0;
}

// visible = found = 1, nobs = 0, no facet for the points first .. first + n - 1 (MapPoint.cc:38,58)
extern "C" hipError_t tc_init_points_launch(const TcState& s, int first, int n, hipStream_t st);
// dst[src[i * stride]] += delta for i < n; entries < 0 are skipped (nObs from the records of the observation log)
extern "C" hipError_t tc_add_by_index_launch(int32_t* dst, const int32_t* src, int stride, int32_t delta, int n, hipStream_t st);
// dst[src[idx[i]]] += delta for i < n (the erase: idx[i] is the point field of a record that is about to be blanked)
extern "C" hipError_t tc_add_by_record_launch(int32_t* dst, const int32_t* src, const int32_t* idx, int32_t delta, int n, hipStream_t st);
// Tracking::SearchLocalPoints' IncreaseVisible (Tracking.cc:1408-1425 and :1456): visible[p] += cnt[p] for p < P_cnt, and +1 for every query
// i < Q with inview[i]; nothing when *refused (the search's "window over TRK_MAX_CANDIDATES" flag, may be null)
extern "C" hipError_t tc_visible_launch(int32_t* visible, const int32_t* cnt, int P_cnt, const int32_t* local_ids, const int32_t* inview, int Q,
                                        const int32_t* refused, hipStream_t st);
// nodes / bary of ids[n] (src_bary is not read where src_nodes says -1); ids == null: every point i < n loses its facet
extern "C" hipError_t tc_set_embedding_launch(const TcState& s, const int32_t* ids, const int32_t* src_nodes, const double* src_bary, int n, hipStream_t st);
extern "C" hipError_t tc_set_counters_launch(const TcState& s, const int32_t* ids, const int32_t* visible, const int32_t* found, int n, hipStream_t st);
// each output may be null
extern "C" hipError_t tc_get_launch(const TcState& s, const int32_t* ids, int n, int32_t* visible, int32_t* found, int32_t* nobs, float* xyz,
                                    hipStream_t st);
// DefOptimizer.cc:568-576: every point that is not bad and has a facet; *n_moved += how many
extern "C" hipError_t tc_repose_launch(const TcState& s, int P, const double* node_xyz, int32_t* n_moved, hipStream_t st);
// the rest of TrackLocalMap (DefTracking.cc:253-319): repose when node_xyz is given, the two loops over the frame, the frustum count
extern "C" hipError_t tc_close_launch(const TcState& s, const TcClose& k, hipStream_t st);
// LocalMapping::MapPointCulling (LocalMapping.cc:173-199) of ids[n]
extern "C" hipError_t tc_cull_launch(const TcState& s, const int32_t* ids, const int32_t* first_kf, int32_t current_kf, int n, uint8_t* action,
                                     hipStream_t st);
