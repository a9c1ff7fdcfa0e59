// Device-side layout of one anchor of SchwarpDatabase::add on the resident stores (dsh_keyframe_warp_pair: dsh_warppair.cpp ->
// warppair_kernels.hip).  The numeric stages between the launchers declared here are the launchers of mapping_launch.h and
// schwarp_problem.h, run by dsh_warppair.cpp through the stage headers dsh_sfn.h and dsh_schwarp.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/defslam_hip.h"
#include "localmap_problem.h"
#include "mappoint_problem.h"

#define WP_BLOCK 256
#define WP_SEQ_BLOCK 1024        // the one workgroup of the ordered stages (filter, register, resolve)
#define WP_MAX_KEYPOINTS 8192    // key points of either keyframe
#define WP_NONE 0x7fffffff       // no list position / no slot

// the counters of one call on the device; the head of the download block
struct WpHdr {
  int32_t init_ok;               // stage 2
  int32_t n_kept_pairs;          // stage 3: pairs that stay
  int32_t n_filtered;
  int32_t n_matched;             // stage 4: queries that found a key point
  int32_t n_appended;            // log records appended
  int32_t n_list;                // L = n_kept_pairs + n_matched: what the host reads at stage 5
  int32_t n_skipped, n_dropped, n_kept, n_stored;   // stage 7, per entry of the list
  int32_t max_pid;               // the largest point id stored, -1: none
  int32_t rounds;                // of the election
  int32_t n_found, n_ref_moved, n_set_bad;          // EraseObservation: live records blanked, reference keyframes moved, points set bad
  int32_t n_erased;              // records the cascade blanked
  int32_t n_listed;              // entries of the erased list: n_found + n_erased
  int32_t pad;
};

struct WpBufs {
  int32_t P, slot, anchor, tag;
  int32_t n_pairs, n_queries;
  int32_t N1, N2, off1, off2;    // key points and table offsets of the anchor (1) and the new keyframe (2)
  int32_t n_ctrl, nan_limit;     // 2 NCu NCv values of x; min(2N, 2 NCu NCu)
  long long R;                   // log records before the call
  // the point store
  int32_t* bad;
  int32_t* ref_kf;
  int32_t* nobs;
  int2* log;
  int32_t* log_idx;
  const LmKf* kf;
  int32_t* table;
  const float* kpn;              // 2 per table entry
  // the keyframe store
  const MpuSlot* slots;
  const uint4* rows;
  const int8_t* oct;
  const float* sf;               // MPU_MAX_LEVELS per slot
  // the upload block
  const int32_t* pair_idx1;
  const int32_t* pair_idx2;
  const int32_t* query_idx1;
  // stage 1: the gathered arrays
  float *g_kp1, *g_kp2, *g_isg;  // n_pairs
  float* q_kp1;                  // n_queries x 2
  uint4* q_desc;                 // n_queries x 2
  // stage 2 / 3
  double* x;                     // n_ctrl
  const double* scal;            // the scalars of the initialisation's solve
  const double* res;             // 2 n_pairs + 4 N residuals
  uint8_t* has;                  // N2: the key point holds a point after the filter's clears
  // stage 4
  const int32_t* match;          // n_queries (the download block's query_match)
  // the kept list: n_pairs + n_queries entries each
  int32_t *k_idx1, *k_idx2, *k_src, *k_tag, *k_pid;   // k_src: pair i, or n_pairs + query j
  float *k_kp1, *k_kp2, *k_isg;
  // stage 7
  const uint8_t* drop;           // the fit's drop flags, per entry of the list
  int32_t *e_p1, *e_p2;          // per entry: the points it names at the start of stage 7
  uint8_t* e_alive;
  // per point of the store
  int32_t* rec_slot;             // the live record (p, slot), -1: none
  int32_t* anc_idx;              // the key point index of the live record (p, anchor), -1: none
  int32_t* cand;                 // ref_kf[p] == slot: the lowest other slot among the live records, else WP_NONE
  int32_t* first;                // stage 4: the first query of the point; stage 7: the first alive dropped entry with p2 == p
  int32_t* mark;                 // 1: setBadFlag runs on the point
  // per key point
  int32_t* win2;                 // N2.  stage 4: the last query that found it; stage 7: the first alive dropped entry with that idx2
  int32_t* kill1;                // N1.  stage 7: the first drop whose cascade clears the anchor's entry
  // the download block
  WpHdr* hdr;
  uint8_t* pair_state;           // n_pairs
  uint8_t* query_state;          // n_queries
  int32_t* query_point;
  uint8_t* query_added;
  int2* out_erased;              // (point, slot) of every record blanked; the host sized it for every live record and every query
};

// every launch of a stage, in stream order and without a host read in between
extern "C" hipError_t wp_gather_launch(const WpBufs& b, hipStream_t st);      // the clears, the pass over the log, stage 1
extern "C" hipError_t wp_fix_start_launch(const WpBufs& b, hipStream_t st);   // the tail of stage 2: init_ok, NaN -> 0
extern "C" hipError_t wp_filter_launch(const WpBufs& b, hipStream_t st);      // stage 3 behind the evaluation, and `has`
extern "C" hipError_t wp_register_launch(const WpBufs& b, hipStream_t st);    // stage 4 behind the search
extern "C" hipError_t wp_resolve_launch(const WpBufs& b, int L, hipStream_t st);   // stage 7 behind the fit
