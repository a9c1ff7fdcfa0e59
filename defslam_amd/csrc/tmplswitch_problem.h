// Device-side layout of the template switch on the map point store (dsh_need_new_template, dsh_template_switch, dsh_surface_vertices,
// dsh_point_store_get_points, dsh_point_store_get_embedding: dsh_tmplswitch.cpp -> tmplswitch_kernels.hip, and the store variant of the
// embedding kernel in register_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/defslam_hip.h"
#include "localmap_problem.h"
#include "mappoint_problem.h"
#include "trackclose_problem.h"

#define TS_BLOCK 256

// what a key point of the keyframe is to CreateNewMapPoints (DefLocalMapping.cc:273-345)
#define TS_HELD 0        // holds a point that is not bad and no later key point holds the same point: the point moves
#define TS_HELD_AGAIN 1  // the same, but a later key point holds the point too: the later SetWorldPos wins
#define TS_HELD_BAD 2    // holds a bad point: nothing
#define TS_MASKED 3      // empty, inside the occupancy mask: nothing
#define TS_NEW 4         // empty, outside the mask: a new point

// the counts as the kernels see them: the ABI's struct and, behind it, the largest node index the embedding stored
struct TsCounts {
  dsh_template_switch_counts c;
  int32_t max_node, pad;
};

// one dsh_need_new_template / dsh_template_switch: the upload block's slices, the store's arrays and the temporaries
struct TsSwitch {
  int32_t rows, cols, N, slot;
  int32_t P;                     // points of the store before the call
  long long R;                   // log records before the call
  int32_t tab_off;               // the keyframe's table in the store: table[tab_off .. tab_off + N)
  const float* kp;               // N x 2
  const float* surface;          // N x 3, camera frame (null for dsh_need_new_template)
  const float* Twc;              // 16, row major
  const int8_t* octave;          // N: the key points' octaves (dsh_kfdb's host table)
  const float* sf;               // MPU_MAX_LEVELS scale factors of the keyframe
  int32_t levels;
  // dsh_kfdb
  const MpuSlot* kf_slots;
  const uint4* kf_rows;
  // dsh_mpdb besides TcState
  int32_t* table;
  int2* log;
  int32_t* log_idx;              // the key point index of each log record
  int32_t* ref_kf;               // the reference keyframe of each point
  float* normal;
  float* max_distance;
  uint4* desc;
  // temporaries and outputs
  uint8_t* cls;                  // N: TS_*
  int32_t* block_new;            // new points per workgroup of the classify launch
  uint8_t* candidate;            // N, or null (dsh_need_new_template)
  int32_t* new_idx;              // N (dsh_template_switch)
  TsCounts* counts;              // zero on entry
};

// the template of the context as the embedding reads it
struct TsTemplate {
  int32_t n;
  const double* xyz0;
  const int32_t* facets;
  const int32_t* nf_ptr;
  const int32_t* nf_idx;
};

// one launch: cls[] and block_new[] of every key point, n_moved / n_masked / n_new into counts, candidate[] when given
extern "C" hipError_t ts_classify_launch(const TcState& s, const TsSwitch& k, hipStream_t st);
// one launch: the held points move, the new points are created with ids P + j in ascending key point index
extern "C" hipError_t ts_create_launch(const TcState& s, const TsSwitch& k, hipStream_t st);
// register_kernels.hip, one launch over P + max_new points, of which the first P + counts->c.n_new exist: a bad point loses its facet;
// every other point is embedded as by reg_embed from its position in the store, the facet's nodes and the widened barycentrics are
// written into the state and the point moves to its barycentric position on the rest shape
extern "C" hipError_t reg_embed_store(const TcState& s, int P, int max_new, const TsTemplate& t, TsCounts* counts, hipStream_t st);
// *out = max(*out, the largest node index stored for the points 0 .. P - 1)
extern "C" hipError_t ts_max_node_launch(const int32_t* nodes, int P, int32_t* out, hipStream_t st);
// camera points (float)(u d), (float)(v d), (float)d, 1 through Twc, widened: nodes_xyz[n x 3]
extern "C" hipError_t ts_vertices_launch(const double* u, const double* v, const double* d, const float* Twc, int n, double* nodes_xyz, hipStream_t st);
// read-backs by id; each output may be null
extern "C" hipError_t ts_get_points_launch(const TcState& s, const float* normal, const float* max_distance, const uint4* desc, const int32_t* ids, int n,
                                           float* xyz, float* onormal, float* omaxd, uint4* odesc, uint8_t* obad, hipStream_t st);
extern "C" hipError_t ts_get_embedding_launch(const TcState& s, const int32_t* ids, int n, int32_t* nodes, double* bary, hipStream_t st);
