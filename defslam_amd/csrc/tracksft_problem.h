// Device-side layout of the observation selection of Shape-from-Template on the map point store (dsh_track_sft_observations,
// dsh_track_sft: dsh_tracksft.cpp -> tracksft_kernels.hip): the argument record host and kernel share, and the launcher.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/defslam_hip.h"

#define TF_BLOCK 256            // threads of a workgroup, one key point each per tile
#define TF_TILES 2              // consecutive tiles of TF_BLOCK key points a workgroup compacts
#define TF_MAX_KEYPOINTS 8192
#define TF_MAX_LEVELS 32

struct TfSelect {
  int32_t N;
  // the upload block
  const int32_t* frame_points;   // N: a point of the store or -1
  const uint8_t* outlier;        // N: mvbOutlier on entry
  const int32_t* octave;         // N: inside the levels where a point is held
  const float* kp;               // 2 per key point
  const float* sig;              // mvInvLevelSigma2
  // the store
  const int32_t* bad;            // 1 per point
  const int32_t* nodes;          // 3 per point, -1 -1 -1: no facet
  const double* bary;            // 3 per point
  // the download block: the table as a structure of arrays with room for N rows, in key point order
  int32_t* head;                 // M, points_obs
  int32_t* kp_index;             // 1 per row
  int32_t* point_id;             // 1 per row
  int32_t* row_nodes;            // 3 per row
  double* row_bary;              // 3 per row
  double* uv;                    // 2 per row
  double* invsig2;               // 1 per row
};

extern "C" hipError_t tf_select_launch(const TfSelect& s, hipStream_t st);
