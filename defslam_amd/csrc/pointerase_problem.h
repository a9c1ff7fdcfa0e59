// Device-side layout of the erase on the resident map point store (dsh_point_store_erase_observations, dsh_point_store_set_bad,
// dsh_point_store_cull and the two read-backs: dsh_pointerase.cpp -> pointerase_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/defslam_hip.h"
#include "localmap_problem.h"
#include "obslist_problem.h"

#define PE_BLOCK 256
#define PE_NO_SLOT 0x7fffffff   // cand of a point no live record names
#define PE_SEEK 1               // mark: the point's reference keyframe was erased, the lowest remaining slot is sought
#define PE_DOOMED 2             // mark: setBadFlag runs on the point

#define PE_ERASE 0              // mode: MapPoint::EraseObservation per pair
#define PE_SET_BAD 1            // mode: DefMapPoint::setBadFlag per id
#define PE_CULL 2               // mode: LocalMapping::MapPointCulling per id

// the counters of one call on the device; the head of the download block
struct PeHdr {
  int32_t n_seek;       // points the select stage marked PE_SEEK    } the sweep leaves at once when both are 0
  int32_t n_doomed;     // points the select stage marked PE_DOOMED  }
  int32_t n_found;      // pairs whose record was live
  int32_t n_ref_moved;  // points whose reference keyframe changed
  int32_t n_set_bad;    // points the finish stage set bad
  int32_t n_erased;     // records the sweep blanked: entries of the erased list
  int32_t total;        // the read-back of observations: entries of its lists
  int32_t pad;
};

struct PeBufs {
  int32_t P, n, mode;
  int32_t erase_match, current_kf;
  long long R;                   // log records
  // the point store
  int32_t* bad;
  int32_t* ref_kf;
  int32_t* nobs;
  const int32_t* found;
  const int32_t* visible;
  int2* log;
  const int32_t* log_idx;
  const LmKf* kf;
  int32_t* table;
  // the upload block
  const int32_t* ids;            // n: the points
  const int32_t* slots;          // n: the keyframe of each pair (PE_ERASE)
  const long long* rec;          // n: the record of each pair in the log, -1: not stored (PE_ERASE)
  const int32_t* first_kf;       // n: mnFirstKFid (PE_CULL)
  // temporaries
  int32_t* mark;                 // P: PE_SEEK | PE_DOOMED
  int32_t* cand;                 // P: the lowest slot among the live records of a PE_SEEK point, else PE_NO_SLOT
  // the download block
  PeHdr* hdr;
  uint8_t* out_code;             // n: the status (PE_ERASE) or the action (PE_CULL); null for PE_SET_BAD
  int2* out_erased;              // (point, slot) of every record the sweep blanked, in any order; the host sized it for every live record
};

// the read-back of observations: MapPoint::GetObservations of ids[n]
struct PeObsBufs {
  int32_t P, n, cap;             // cap: entries of out_slot / out_idx
  const int32_t* ids;
  ObsLists ol;                   // the lists of ids[n]: sel_of is the position of a point in ids, off the download block's n + 1 offsets
  PeHdr* hdr;
  int32_t* out_slot;             // cap: by ascending slot; written only when total <= cap
  int32_t* out_idx;
};

// every launch of a call, in stream order and without a host read in between
extern "C" hipError_t pe_erase_launch(const PeBufs& b, hipStream_t st);
extern "C" hipError_t pe_observations_launch(const PeObsBufs& b, hipStream_t st);
