// Device-side layout of the anchor keyframes and match lists of a new keyframe on the map point store (dsh_keyframe_anchors,
// dsh_point_store_get_reference_keyframes: dsh_anchor.cpp -> anchor_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/defslam_hip.h"
#include "localmap_problem.h"

#define AN_BLOCK 256              // threads of a workgroup; one workgroup compacts the row of one anchor
#define AN_MAX_KEYPOINTS 8192     // key points of the new keyframe
#define AN_UNMARKED 0x7fffffff    // first_i of a point no good entry of the new keyframe holds

// the counters of one call, on the device and in the download block
struct AnHdr {
  int32_t n_anchors, n_pairs, n_queries, n_no_ref;
};

// one dsh_keyframe_anchors: the store's arrays (P points, K keyframes, R log records), the temporaries and the download block
struct AnBufs {
  int32_t P, K, N, slot, min_pairs, tab_off;   // N, tab_off: the new keyframe's table, table[tab_off .. tab_off + N)
  int32_t max_anchors;                         // min(K, N): what the host knows of the number of anchors
  long long R;
  const int32_t* bad;        // P
  const int32_t* ref_kf;     // P: slot or -1
  const int2* log;           // R records (point, keyframe slot); point -1: erased
  const int32_t* log_idx;    // R: the key point index of the record in its keyframe
  const LmKf* kf;            // K
  const int32_t* table;
  // temporaries
  int32_t* first_i;          // P: the first entry of the new keyframe that holds the point and finds it good, else AN_UNMARKED
  int32_t* mult;             // P: how many such entries there are
  int32_t* idx2_of;          // P: the index of the live record (point, slot), else -1
  int32_t* votes;            // K: countKFMatches
  int32_t* rank;             // K: position among the anchors, else -1
  int32_t* a_slot;           // max_anchors: the anchors by ascending slot
  int32_t* a_pairs;          // max_anchors: pairs of each anchor, below min_pairs or not
  int32_t* a_queries;        // max_anchors: queries of each anchor
  int32_t* pptr;             // max_anchors + 1: CSR offsets of the pairs (anchors below min_pairs contribute none)
  int32_t* qptr;             // max_anchors + 1: of the queries
  int32_t* matrix;           // chunk x N: idx1 of (anchor c0 + row, point with first_i == column), else -1
  int32_t chunk;             // anchors per pass over the matrix
  AnHdr* hdr;
  // the download block: lists are written as far as the capacities reach, the counters in full
  int32_t cap_anchors, cap_pairs, cap_queries;
  AnHdr* out_hdr;
  int32_t *out_slot, *out_count, *out_npairs;   // cap_anchors
  int32_t *out_pptr, *out_qptr;                 // cap_anchors + 1
  int32_t *out_idx1, *out_idx2, *out_point;     // cap_pairs
  uint8_t* out_own;                             // cap_pairs: ref_kf[point] == anchor
  int32_t *out_qidx1, *out_qpoint;              // cap_queries
  uint8_t* out_has;                             // N: table[j] != -1
};

// every launch of a call, in stream order and without a host read in between
extern "C" hipError_t an_anchors_launch(const AnBufs& b, hipStream_t st);
// out[i] = src[ids[i]] for i < n
extern "C" hipError_t an_gather_i32_launch(const int32_t* src, const int32_t* ids, int n, int32_t* out, hipStream_t st);
