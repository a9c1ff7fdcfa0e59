// Device-side layout of the map point upkeep on the resident stores (dsh_keyframe_process_new, dsh_point_store_upkeep:
// dsh_kfinsert.cpp -> kfinsert_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/defslam_hip.h"
#include "localmap_problem.h"
#include "mappoint_problem.h"
#include "obslist_problem.h"

#define KI_BLOCK 256
#define KI_UNMARKED 0x7fffffff   // first_i of a point no entry of the keyframe holds
#define KI_LARGE_GRID 1024       // wavefronts that stride over the block list of the large points

// the counters of one call on the device; the head of the download block
struct KiHdr {
  int32_t n_sel;                 // selected points: entries of sel_pid
  int32_t n_appended;            // log records this call appended (dsh_keyframe_process_new)
  int32_t total;                 // observations of the selected points
  int32_t cls_n[4];              // small points per width class (8, 16, 32, 64 lanes)
  int32_t n_large, n_blocks;     // large points, entries of their block list
  int32_t n_empty, n_bad, n_recent;             // dsh_keyframe_process_new, per table entry (n_appended is n_added)
  int32_t n_no_obs, n_no_good_desc, n_no_ref;   // among the selected points
  int32_t n_skipped_bad;         // ids of dsh_point_store_upkeep that name a bad point
};

struct KiBufs {
  int32_t P, S;                  // points of the store; what the host knows of the number of selected points
  int32_t what;                  // DSH_MP_* mask
  // the store's log (R: its records before the call), the store's keyframes (the bad flag the election reads), sel_of (the position of
  // a point in sel_pid, else -1) and the observation lists of the selected points; the launchers point n_dev, n_extra and total into hdr
  ObsLists ol;
  // the point store
  const float* xyz;
  const int32_t* bad;
  const int32_t* ref_kf;
  const int32_t* nodes;          // 3 per point, -1: no facet
  int32_t* nobs;
  const int32_t* table;
  uint4* desc;                   // results: two uint4 per point
  float* normal;                 // 3 per point
  float* max_distance;
  // the keyframe store
  const MpuSlot* slots;
  const uint4* rows;
  const int8_t* oct;
  const int32_t* levels;
  const float* sf;               // MPU_MAX_LEVELS per slot
  // the new keyframe (dsh_keyframe_process_new)
  int32_t slot, N, tab_off;
  int32_t* first_i;              // P: the lowest entry of the keyframe that holds the point, else KI_UNMARKED
  int32_t* observes;             // P: the log holds a live record (point, slot)
  // the selection (dsh_point_store_upkeep)
  int32_t n_ids;
  const int32_t* ids;
  // temporaries
  int32_t* sel_pid;              // S: the selected points (-1: an id that names a bad point)
  int32_t* obs_slot;             // cap_obs: by ascending slot
  int32_t* el_row;               // cap_obs: the election rows, by ascending slot, at the same offsets
  MpuPoint* pts;                 // S
  int32_t* small_list;           // 4 x S
  int32_t* large_pts;            // S
  int2* large_blocks;            // cap_blocks: (position in sel_pid, first election row or -1)
  uint32_t* large_key;           // S
  KiHdr* hdr;
  // the download block
  KiHdr* out_hdr;
  int32_t* out_status;           // S (dsh_point_store_upkeep with ids), or null
  uint8_t* out_action;           // N (dsh_keyframe_process_new)
  int32_t* out_added;            // N
};

// every launch of a call, in stream order and without a host read in between
extern "C" hipError_t ki_process_new_launch(const KiBufs& b, hipStream_t st);
extern "C" hipError_t ki_upkeep_launch(const KiBufs& b, int embedded, hipStream_t st);
