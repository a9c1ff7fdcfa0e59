// Device-side layout of the creation of a keyframe on the two resident stores and of its covisibility connections
// (dsh_keyframe_create, dsh_keyframe_update_connections: dsh_keyframe_create.cpp -> keyframe_create_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/defslam_hip.h"
#include "localmap_problem.h"
#include "mappoint_problem.h"

#define KC_BLOCK 256
#define KC_MAX_KEYPOINTS 8192    // of a keyframe that is created or connected: a weight is at most this (13 bits and one)
#define KC_MAX_KEYFRAMES 65535   // of the store: a slot fits 16 bits, so (weight << 16) | slot is a unique 30-bit key

// what dsh_keyframe_create brings down; it goes up as zeros at the end of the upload block
struct KcCreateOut {
  int32_t n_held, n_snapshot;
  float Ow[3];
  int32_t pad[3];
};

// one dsh_keyframe_create: the upload block, and where its parts belong in the two stores
struct KcCreate {
  int32_t N, levels;
  const uint4* src_rows;       // 2 N: the descriptor rows
  const int8_t* src_oct;       // N
  const float* src_sf;         // MPU_MAX_LEVELS, zeros past levels
  const float* Tcw;            // 16, row major
  const int32_t* src_points;   // N: of the upload block, or the store's resident keyframe candidate
  const float* src_kpn;        // N x 2, or null: no Surface
  // the keyframe store, at the new slot and at its first row
  MpuSlot* kf_slot;
  int32_t row_off;
  uint4* rows;
  int8_t* oct;
  int32_t* levels_out;
  float* sf;
  // the point store, at the new slot and at its first table entry
  LmKf* kf;
  int32_t tab_off;
  int32_t* table;
  int32_t* snap_point;
  float* surf_normal;
  float* surf_pts;
  float* surf_kpn;
  uint8_t* surf_has;
  int32_t* surf_nn;
  KcCreateOut* out;            // n_held is added to; Ow is written
};

// what dsh_keyframe_update_connections brings down ahead of its four lists: dsh_keyframe_connections and two words of padding
struct KcConnOut {
  int32_t n_counted, n_connected, parent, parent_set, max_weight, max_kf, pad[2];
};

// one dsh_keyframe_update_connections
struct KcConn {
  int32_t P, K, slot, th, first;   // first: mbFirstConnection of the keyframe, from the host mirror
  int32_t tab_off, N;              // its table
  long long R;
  const int32_t* bad;              // P
  const int2* log;                 // R
  LmKf* kf;                        // K: the parent of `slot` is written
  const int32_t* table;
  int32_t* cnt;                    // P, scratch: the table's multiplicities
  int32_t* w;                      // K, scratch: the weights
  // the download block
  KcConnOut* hdr;
  int32_t* counted_kf;             // K each
  int32_t* counted_w;
  int32_t* ordered_kf;
  int32_t* ordered_w;
};

// one launch: the upload block into both stores, an empty snapshot, the Surface when there is one, the centre of Tcw
extern "C" hipError_t kc_create_launch(const KcCreate& k, hipStream_t st);
// at most four launches, no host read between them: clear, scatter, the sweep over the log, the ordering
extern "C" hipError_t kc_connections_launch(const KcConn& k, hipStream_t st);
