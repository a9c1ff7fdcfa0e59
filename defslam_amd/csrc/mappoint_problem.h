// Device-side layout of the map point upkeep (dsh_kfdb_*, dsh_mappoint_update: dsh_mappoint.cpp -> mappoint_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define MPU_MAX_LEVELS 32
#define MPU_SMALL 64        // points with at most this many observations go to the packed kernel (one lane per row)
#define MPU_ROWS 64         // election rows of a large point per wavefront
#define MPU_HIST_WORDS 129  // 257 bins of 16-bit counts packed two to a 32-bit word (odd stride: fewer LDS bank conflicts)

// one keyframe of the store: what the kernels read besides its descriptor rows
struct MpuSlot {
  float Ow[3];
  int32_t row_off;   // first descriptor row in the store
};

// one map point of a call
struct MpuPoint {
  float x, y, z;
  int32_t obs_off, M;   // its observations: slots obs_slot[obs_off .. obs_off + M)
  int32_t el_off, Me;   // its election rows: el_row[el_off .. el_off + Me), the observations whose keyframe is not bad, in order
  int32_t ref_slot;     // mpRefKF (-1 without DSH_MP_NORMAL_DEPTH)
  float sf_level, sf_last;   // mvScaleFactors[level] and mvScaleFactors[nLevels - 1] of the reference keyframe
  int32_t what, pad;
};

struct MpuBufs {
  const MpuSlot* slots;
  const uint4* rows;       // the store's descriptor rows, two uint4 per row
  const MpuPoint* pts;
  const int32_t* obs_slot;
  const int32_t* el_row;
  // small kernel: points in work order, grouped by width class (lane groups of 8, 16, 32 or 64 lanes)
  const int32_t* small_order;
  // large kernel: one wavefront per (point, block of MPU_ROWS election rows)
  const int2* large_blocks;    // (point, first row)
  uint32_t* large_key;         // per point: min over rows of median << 16 | row (atomicMin), 0xFFFFFFFF initially
  const int32_t* large_pts;    // the large points (finish kernel)
  // outputs, per point
  int32_t* best;      // election row of the winner, -1
  uint4* desc;        // two uint4 per point
  float* normal;      // 3 per point
  float* dist;        // 2 per point: max, min
};

extern "C" hipError_t mpu_launch(const MpuBufs& b, const int32_t* small_off, int n_large_blocks, int n_large, hipStream_t st);
