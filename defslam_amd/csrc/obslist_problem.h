// The builder of per-point observation lists from the unsorted log of the map point store (obslist_kernels.hip), as
// dsh_keyframe_process_new, dsh_point_store_upkeep and dsh_point_store_get_observations run it, and the rank by slot that orders a list.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "localmap_problem.h"

#define OBS_BLOCK 256

struct ObsLists {
  int2* log;                     // (point, keyframe slot); point -1: erased
  int32_t* log_idx;              // parallel to the log: the observation's key point index
  long long R;                   // the passes read the records [0, R + *n_extra)
  const int32_t* n_extra;        // device: records the call appended behind R, or null
  const LmKf* kf;                // when given, bit 31 of a raw_slot entry is the bad flag of its keyframe
  int32_t n;                     // lists; *n_dev when n_dev is given (n then bounds it)
  const int32_t* n_dev;
  int32_t* sel_of;               // P: the list of a point, else -1; the caller's selection
  int32_t* cnt;                  // n: live observations per list; zero before the launch
  int32_t* fill;                 // n: zero before the launch
  int32_t* off;                  // n + 1: the CSR offsets
  int32_t* raw_slot;             // every live record fits: per list its observations in log order, the slot
  int32_t* raw_idx;              //                                                                 and the key point index
  int32_t* total;                // device: receives off[n]
};

// count, scan, fill in stream order; R_max: what the host knows of the number of records the passes read
extern "C" hipError_t obs_lists_launch(const ObsLists& a, long long R_max, hipStream_t st);

// The rank by slot of the observation with slot s among raw_slot[o .. o + M) (slots are unique within a point, so the ranks are a
// permutation and do not depend on arrival order); grank: its rank among the observations without the flag in bit 31.
__device__ __forceinline__ int obs_rank(const int32_t* raw_slot, int o, int M, int s, int& grank) {
  int rank = 0;
  grank = 0;
  for (int q = 0; q < M; q++) {   // wave-uniform address
    const uint32_t u = (uint32_t)raw_slot[o + q];
    const bool lt = (int)(u & 0x7FFFFFFFu) < s;
    rank += lt;
    grank += lt && !(u >> 31);
  }
  return rank;
}
