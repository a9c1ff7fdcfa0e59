// Device-side layout of the surface registration of a keyframe on the resident stores (dsh_keyframe_snapshot_positions,
// dsh_keyframe_register_clouds, dsh_keyframe_register, dsh_keyframe_set_pose: dsh_surfreg.cpp -> surfreg_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/defslam_hip.h"
#include "mappoint_problem.h"
#include "trackclose_problem.h"

#define SR_BLOCK 1024           // the snapshot and the selection are one workgroup each: the compaction is ordered across its tiles
#define SR_FINISH_BLOCK 256
#define SR_MAX_KEYPOINTS 8192   // of a keyframe whose clouds are selected

// what the selection counts, in the order of dsh_keyframe_register_result
struct SrCounts {
  int32_t n_pairs, n_empty, n_bad, n_no_facet, n_no_snapshot, pad[3];
};

// the keyframe's slice of the tables: table, snap_point [tab_off .. tab_off + N), snap_xyz three floats per entry
struct SrKeyframe {
  int32_t N, tab_off;
  const int32_t* table;
  int32_t* snap_point;
  float* snap_xyz;
};

// one dsh_keyframe_register_clouds / dsh_keyframe_register
struct SrSelect {
  SrKeyframe kf;
  int32_t P;                 // points of the store
  const float* surface;      // N x 3, camera frame
  const float* Twc;          // 16, row major
  int32_t* entry_of;         // P, not initialised: entry_of[p] is trusted only where snap_point names p there
  int32_t* pair_idx;         // N
  float* cloud_surface;      // N x 3
  float* cloud_map;          // N x 3
  SrCounts* counts;          // written, not added to
};

// the finishing launch of a registration, and dsh_keyframe_set_pose (N == 0)
struct SrFinish {
  int32_t N;
  const float* surface;      // N x 3
  double s22;
  float Tcw[16];             // the new pose, by value
  MpuSlot* kf_slot;          // the keyframe's record in dsh_kfdb, or null
  float* surface_scaled;     // N x 3
  float* Ow;                 // 3: the centre, always written
  // the keyframe's resident Surface (dsh_keyframe_surface_init), or nulls: Surface::applyScale of the copy the store holds, in place
  float* resident_pts;       // N x 3; may be `surface` itself
  double* resident_depth;    // n_depth control points of nodesDepth_, or null
  int32_t n_depth;
};

// KeyFrame::SetPose (KeyFrame.cc:97-111): component c of Ow = -Rcw.t() * tcw of a row-major Tcw, the three products of a row summed left
// to right in float32.  The one statement of it: the finishing launch here and dsh_keyframe_create's (keyframe_create_kernels.hip) call
// it, both compiled without FMA contraction; the host calls it only to refuse a centre that is not finite.
__host__ __device__ __forceinline__ float sr_camera_centre(const float* T, int c) { return -((T[c] * T[3] + T[4 + c] * T[7]) + T[8 + c] * T[11]); }

// one launch, one workgroup: snap_point / snap_xyz of the entries whose point is not bad and has a facet; *n_taken = their number
extern "C" hipError_t sr_snapshot_launch(const TcState& s, const SrKeyframe& k, int32_t* n_taken, hipStream_t st);
// one launch, one workgroup: the pairs of SurfaceRegistration.cc:60-104 in ascending entry order, and the counts
extern "C" hipError_t sr_select_launch(const TcState& s, const SrSelect& k, hipStream_t st);
// one launch: Surface::applyScale of the surface points (and of the resident Surface) and KeyFrame::SetPose's camera centre
extern "C" hipError_t sr_finish_launch(const SrFinish& k, hipStream_t st);
