// Device-side layout of the rigid pose-only optimisation on the map point store (dsh_track_pose_only, dsh_track_pose_only_batch:
// dsh_poseonly.cpp -> poseonly_kernels.hip): the records host and kernel share, and the launcher.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/defslam_hip.h"

#define PO_BLOCK 256            // threads of the one workgroup of a problem; the summation order is defined over it
#define PO_MAX_KEYPOINTS 8192
#define PO_MAX_LEVELS 32
#define PO_MAX_BATCH 65536      // problems of one call: their key points are indexed with 32 bits
#define PO_NOT_HELD 2           // state of a key point without a point (0: inlier, level 0; 1: outlier, level 1)

// Every pointer of PoBatch addresses global memory; saying so in the device pass of the kernel file keeps flat_* loads out of the
// loops.  The host pass sees plain pointers; the layout is identical.
#if defined(__HIP_DEVICE_COMPILE__) && defined(PO_KERNEL_SOURCE)
#define PO_G __attribute__((address_space(1)))
#else
#define PO_G
#endif

// one problem, in the upload block
struct PoProb {
  float Tcw[16];     // pFrame->mTcw, row-major
  float K[4];        // fx, fy, cx, cy
  int32_t N;         // key points
  int32_t levels;
  int32_t kp0;       // its first key point in the batch's per-key-point arrays
  int32_t sig0;      // its first entry in the batch's sigma tables
};

// one result, in the download block
struct PoResult {
  double pose[7];    // t, q (x y z w)
  double chi2[4];
  float Tcw_out[16];
  int32_t n_initial, n_bad, n_good, rounds;
  int32_t iters[4], trials[4], bad[4];
};

struct PoBatch {
  int32_t B;
  // the upload block
  PO_G const PoProb* prob;       // B
  PO_G const float* kp;          // 2 per key point of the batch
  PO_G const int32_t* octave;    // 1 per key point
  PO_G const int32_t* ids;       // 1 per key point: a point of the store or -1
  PO_G const float* sig;         // the problems' mvInvLevelSigma2 tables, one after the other
  // the store
  PO_G const float* xyz;         // 3 per point
  // scratch: per key point the edge as six float32 (Xw, the measurement, the information) gathered once
  PO_G float* edge;
  // the download block
  PO_G uint8_t* state;           // 1 per key point: 0 / 1 = mvbOutlier of a key point that holds a point, PO_NOT_HELD otherwise
  PO_G PoResult* res;            // B
};

extern "C" hipError_t po_launch(const PoBatch& b, hipStream_t st);
