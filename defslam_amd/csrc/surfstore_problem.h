// Device-side layout of the resident Surface of a keyframe (dsh_keyframe_surface_*, dsh_keyframe_sfn: dsh_surfstore.cpp ->
// surfstore_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/defslam_hip.h"
#include "trackclose_problem.h"

#define SS_BLOCK 256
#define SS_SELECT_BLOCK 1024    // the selection is one workgroup: the compaction is ordered across its tiles
#define SS_MAX_KEYPOINTS 8192   // of a keyframe whose sites are selected

// the surface arrays of the store, whole: an entry is addressed by its place in the tables (tab_off + idx)
struct SsStore {
  float* normal;        // 3 per entry
  uint8_t* has;         // 1 per entry
  float* pts;           // 3 per entry
  float* kpn;           // 2 per entry
  int32_t* n_normals;   // per keyframe
};

// n targets of dsh_keyframe_surface_set_normals / _take_normals / _gather
struct SsTargets {
  int32_t n;
  const int32_t* entry;   // n: tab_off of the keyframe + idx
  const int32_t* slot;    // n: the keyframe
  int32_t base;           // the smallest entry named: winner is indexed by entry - base
  int32_t* winner;        // the election: -1 before ss_elect_launch, then the largest j that names the entry
};

// where normal j comes from: normals[3 j], or with sel the last normal solve of a database (sel >= 0: nref, < 0: nrec[-1 - sel])
struct SsNormalSource {
  const float* normals;
  const int32_t* sel;
  const float *nref, *nrec;
};

// what the selection of dsh_keyframe_sfn counts, in the order of dsh_keyframe_sfn_result
struct SsCounts {
  int32_t n_sites, n_empty, n_bad, n_no_normal, n_nan, pad[3];
};

// one dsh_keyframe_sfn: the selection of ShapeFromNormals::obtainM and the widened key points of the whole keyframe
struct SsSelect {
  int32_t N, tab_off;
  const int32_t* table;
  double *u, *v;          // N: the sites
  float* normals;         // N x 3
  double *u_all, *v_all;  // N: every key point
  SsCounts* counts;       // written, not added to
};

// the largest j per entry, by an integer atomic
extern "C" hipError_t ss_elect_launch(const SsTargets& t, hipStream_t st);
// the elected j of every entry writes its normal; an entry that had none raises its keyframe's n_normals
extern "C" hipError_t ss_write_normals_launch(const SsStore& s, const SsTargets& t, const SsNormalSource& src, hipStream_t st);
// normal_xy[2 n], has[n], uv[2 n] of the targets
extern "C" hipError_t ss_gather_launch(const SsStore& s, const SsTargets& t, float* normal_xy, uint8_t* has, float* uv, hipStream_t st);
// pts[3 idx[j]] of the keyframe at tab_off = pts_in[3 j]
extern "C" hipError_t ss_set_points_launch(const SsStore& s, int32_t tab_off, int32_t n, const int32_t* idx, const float* pts_in, hipStream_t st);
// one launch, one workgroup: the sites of ShapeFromNormals.cc:190-210 in ascending entry order, the counts, u_all / v_all
extern "C" hipError_t ss_select_launch(const TcState& st8, const SsStore& s, const SsSelect& k, hipStream_t st);
