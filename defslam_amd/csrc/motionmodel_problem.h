// Device-side layout of the end of a tracked frame and of the motion-model search on the map point store (dsh_track_end_frame,
// dsh_motion_model_search: dsh_motionmodel.cpp -> motionmodel_kernels.hip, then track_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/defslam_hip.h"

#define MM_BLOCK 256          // entries of the last-frame list one workgroup of the gather compacts
#define MM_END_BLOCK 1024     // the one workgroup of the end-of-frame kernel

// one dsh_track_end_frame
struct MmEnd {
  int32_t N;
  const int32_t* frame_points;   // N: mvpMapPoints as ids or -1
  const uint8_t* outlier;        // N: mvbOutlier
  const int32_t* octave;         // N: mvKeys[i].octave
  const int32_t* nobs;           // the store's MapPoint::nObs
  int32_t* last_ids;             // N, resident: the id after CleanMatches and the outlier drop, or -1
  int32_t* last_oct;             // N, resident: the octave of an entry that holds a point, else -1
  int32_t* cand_ids;             // N, resident: the id after CleanMatches alone -- the keyframe candidate (dsh_keyframe_create)
  // the download block
  int32_t* points_out;           // N: after CleanMatches
  uint8_t* outlier_out;          // N
  int32_t* counts;               // 4: cleaned, dropped, kept, the largest octave kept (-1: none)
};

// the gather of dsh_motion_model_search: the resident list into the query arrays of the tracking search (track_problem.h, TrkBufs)
struct MmGather {
  int32_t N;                     // length of the resident list
  const int32_t* last_ids;
  const int32_t* last_oct;
  const float* xyz;              // store: 3 per point
  const uint4* desc;             // two per point
  const int32_t* bad;
  const int32_t* nodes;          // 3 per point, -1: no facet
  const int32_t* nobs;
  int32_t* qpid;                 // the queries, at most `kept` of them, in index order
  float* qxyz;
  int32_t* qmeta;                // the last frame's octave
  uint4* qdesc;
  uint8_t* qfree;                // 1: the point has no observations
  // the download block
  int32_t* out_ids;              // the point of each query
  int32_t* out_idx;              // its entry in the list
  int32_t* out_count;            // how many there are
};

extern "C" hipError_t mm_end_frame_launch(const MmEnd& e, hipStream_t st);
extern "C" hipError_t mm_gather_launch(const MmGather& g, hipStream_t st);
