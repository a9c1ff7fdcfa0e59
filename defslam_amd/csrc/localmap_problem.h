// Device-side layout of the map point store and the local map (dsh_mpdb_*, dsh_local_map_*: dsh_localmap.cpp -> localmap_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/defslam_hip.h"

#define LM_MAX_LOCAL 80     // the expansion stops once mvpLocalKeyFrames holds more than this (Tracking.cc:1571)
#define LM_BINS 8192        // keyframes per pass of the vote histogram in LDS (32 KB); more keyframes take more passes over the log
#define LM_BLOCK 256
#define LM_CHUNK 1024       // point flags one wavefront compacts

// one keyframe of the store
struct LmKf {
  int32_t tab_off, N;   // its table: table[tab_off .. tab_off + N), a point id or -1 per key point
  int32_t parent;       // slot or -1
  int32_t bad;
};

// the counters of the resident local map
struct LmHdr {
  int32_t n_voted, n_local_kf, ref_kf, n_local_points;
};

// the store's arrays (P points, K keyframes, R log records) and the temporaries of one dsh_local_map_update
struct LmBufs {
  int32_t P, K, N;
  long long R;
  const int32_t* bad;          // P
  const int2* log;             // R records (point, keyframe slot); point -1: erased
  const LmKf* kf;              // K
  const int32_t* table;
  const int32_t* frame_points; // N
  int32_t* cnt;                // P: how many key points of the frame hold the point (bad points: 0); kept for the search
  int32_t* votes;              // K
  int32_t* mark;               // K: listed in this call (mnTrackReferenceForFrame == mnId)
  int32_t* flag;               // P: local point
  int32_t* block_cnt;          // ceil(P / LM_CHUNK)
  int32_t* local_kf;           // K, resident
  int32_t* local_ids;          // P, resident
  LmHdr* hdr;                  // resident
  // the download block
  LmHdr* out_hdr;
  int32_t* out_kf;             // K
  int32_t* out_votes;          // K
  uint8_t* out_frame_bad;      // N
};

// what the gather kernel fills: the query arrays of the tracking search (track_problem.h, TrkBufs)
struct LmQueryBufs {
  const float* xyz;            // store: 3 per point
  const float* normal;         // 3 per point
  const float* max_distance;
  const uint4* desc;           // two per point
  const int32_t* bad;
  const int32_t* cnt;
  const int32_t* local_ids;
  int32_t* qpid;
  float* qxyz;
  float* qnrm;
  float* qmaxd;
  int32_t* qmeta;
  uint4* qdesc;
  int32_t* out_ids;
};

// a batch of point overwrites by id (dsh_mpdb_update_points): what is a mask of DSH_MPDB_*
struct LmWriteBufs {
  const int32_t* ids;
  const float* src_xyz;
  const float* src_normal;
  const float* src_max_distance;
  const uint4* src_desc;
  float* xyz;
  float* normal;
  float* max_distance;
  uint4* desc;
};

extern "C" hipError_t lm_update_launch(const LmBufs& b, hipStream_t st);
extern "C" hipError_t lm_gather_launch(const LmQueryBufs& q, int Q, hipStream_t st);
extern "C" hipError_t lm_write_points_launch(const LmWriteBufs& w, int n, int what, hipStream_t st);
// dst[idx[i]] = val ? val[i] : fill for i < n (bad flags by id; blanking log records: dst is the log seen as int32 pairs, idx = 2 * record)
extern "C" hipError_t lm_scatter_i32_launch(int32_t* dst, const int32_t* idx, const int32_t* val, int32_t fill, int n, hipStream_t st);
