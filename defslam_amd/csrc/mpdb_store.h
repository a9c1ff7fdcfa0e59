// The map point store dsh_mpdb as its translation units see it: the arrays in HBM, the host mirror that validates, and the checks and
// set-up the entry points share.
//   dsh_localmap.cpp      dsh_mpdb_*, dsh_local_map_*
//   dsh_trackclose.cpp    dsh_trackstate_*, dsh_track_close_frame
//   dsh_tmplswitch.cpp    dsh_need_new_template, dsh_template_switch and the read-backs of points and facets
//   dsh_motionmodel.cpp   dsh_track_end_frame, dsh_track_last_frame, dsh_motion_model_search
//   dsh_anchor.cpp        dsh_keyframe_anchors and the two fields it reads: the key point index of an observation, the reference
//                         keyframe of a point
//   dsh_kfinsert.cpp      dsh_keyframe_process_new, dsh_point_store_upkeep
//   dsh_pointerase.cpp    dsh_point_store_erase_observations, dsh_point_store_set_bad, dsh_point_store_cull and the read-backs of
//                         observations and keyframe tables
//   dsh_tracksft.cpp      dsh_track_sft_observations, dsh_track_sft
//   dsh_surfreg.cpp       dsh_keyframe_snapshot_positions, dsh_keyframe_register and the keyframe pose of the keyframe store
//   dsh_surfstore.cpp     dsh_keyframe_surface_*, dsh_keyframe_sfn: the resident Surface of a keyframe
//   dsh_warppair.cpp      dsh_keyframe_set_view, dsh_keyframe_get_view, dsh_keyframe_warp_pair (warppair_problem.h, warppair_kernels.hip)
//   dsh_keyframe_create.cpp  dsh_track_keyframe_candidate, dsh_keyframe_create, dsh_keyframe_update_connections (keyframe_create_problem.h,
//                         keyframe_create_kernels.hip)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "localmap_problem.h"
#include "obslist_problem.h"
#include "tmplswitch_problem.h"
#include "trackclose_problem.h"

struct dsh_mpdb : dsh_store {
  int32_t P = 0, Pcap = 0, K = 0, Kcap = 0;
  long long R = 0, Rcap = 0, T = 0, Tcap = 0;   // log records, table entries
  // points
  float *d_xyz = nullptr, *d_nrm = nullptr, *d_maxd = nullptr;
  uint4* d_desc = nullptr;
  int32_t *d_bad = nullptr, *d_cnt = nullptr, *d_local_ids = nullptr;
  int32_t* d_ref_kf = nullptr;   // per point MapPoint::GetReferenceKeyFrame as a slot, -1: not given
  // tracking state per point (dsh_trackstate_*, dsh_track_close_frame): mnVisible, mnFound, nObs, the facet as three ascending node
  // indices (-1: none) with its barycentrics, and the local point list as it was before the last dsh_local_map_update
  int32_t *d_visible = nullptr, *d_found = nullptr, *d_nobs = nullptr, *d_nodes = nullptr, *d_ref_ids = nullptr;
  double* d_bary = nullptr;
  // observations, keyframes, the resident local map
  int2* d_log = nullptr;
  int32_t* d_log_idx = nullptr;   // parallel to the log: the key point index of the observation in its keyframe, -1: not given
  LmKf* d_kf = nullptr;
  int32_t *d_table = nullptr, *d_local_kf = nullptr;
  // DefKeyFrame's PosesKeyframes, parallel to d_table (dsh_keyframe_snapshot_positions): per table entry the point whose position was
  // taken there (-1: none) and that position.  Keyed by point: later edits of the table do not touch it.
  int32_t* d_snap_point = nullptr;
  float* d_snap_xyz = nullptr;
  // defSLAM::Surface of a keyframe (dsh_keyframe_surface_*), parallel to d_table: per table entry SurfacePoint::Normal, NormalOn and
  // x3D, and mpKeypointNorm[i].pt.  Per keyframe, parallel to d_kf: numberofNormals_ and the SURF_MAX_CTRL doubles of nodesDepth_.
  // An entry's four fields mean something from dsh_keyframe_surface_init of its keyframe on (surf[slot].has_surface).
  float *d_surf_normal = nullptr, *d_surf_pts = nullptr, *d_surf_kpn = nullptr;
  uint8_t* d_surf_has = nullptr;
  int32_t* d_surf_nn = nullptr;
  double* d_surf_depth = nullptr;
  // the view of a keyframe (dsh_keyframe_set_view), parallel to d_table: per table entry the pixel key point mvKeysUn[i].pt; its
  // scalars live in surf[slot].  An entry means something from dsh_keyframe_set_view of its keyframe on (surf[slot].has_view).
  float* d_view_px = nullptr;
  LmHdr* d_hdr = nullptr;
  // the resident last-frame list (dsh_track_end_frame): per key point of the last frame the id it holds or -1, and its octave (-1 there)
  int32_t *d_last_ids = nullptr, *d_last_oct = nullptr;
  // the resident keyframe candidate beside it: the same frame's ids after CleanMatches alone, outliers still held -- the table
  // DefTracking::CreateNewKeyFrame copies (dsh_keyframe_create with points == NULL)
  int32_t* d_cand_ids = nullptr;
  int32_t last_cap = 0;
  // host mirror
  std::unordered_map<uint64_t, long long> obs;   // (point, keyframe) -> its record in the log
  std::unordered_set<uint64_t> unindexed;        // the live records without a key point index (dsh_mpdb_add_observations)
  std::vector<LmKf> kf;
  std::vector<uint8_t> snapped;          // per keyframe: its snapshot has been taken (the reference takes it once, in the constructor)
  static constexpr int SURF_MAX_CTRL = 512;   // control points of a resident depth spline: the limit of dsh_sfn_estimate
  struct SurfKf {                        // per keyframe: what the host knows of its resident Surface
    uint8_t has_surface = 0, has_depth = 0;
    int32_t n_normals = 0;               // numberofNormals_, as d_surf_nn holds it
    dsh_bbs grid{};                      // of the depth spline, valdim 1
    // dsh_keyframe_set_view: camera (fx, fy, cx, cy), image bounds (mnMinX, mnMaxX, mnMinY, mnMaxY), image grid, warp grid
    uint8_t has_view = 0;
    float cam[4] = {0, 0, 0, 0}, bounds[4] = {0, 0, 0, 0};
    int32_t grid_cols = 0, grid_rows = 0;
    dsh_bbs warp{};
  };
  std::vector<SurfKf> surf;
  int32_t n_local_points = 0;
  int32_t n_ref_points = 0;            // length of d_ref_ids
  int32_t P_cnt = 0;                   // points d_cnt covers: the store's size at the last dsh_local_map_update
  std::vector<int32_t> top_node;       // per point its largest node index, -1 without a facet
  int32_t max_node = -1;               // the largest of top_node, unless max_node_stale
  bool max_node_stale = false;
  bool top_on_device = false;          // a template switch wrote facets on the device: top_node does not know them, max_node does
  int32_t last_N = -1;                 // length of the resident last-frame list, -1: there is none
  int32_t last_kept = 0;               // its entries that hold a point
  int32_t last_max_octave = -1;        // the largest octave among them
  int32_t cand_N = -1;                 // length of the resident keyframe candidate, -1: there is none
  std::vector<uint8_t> first_conn;     // per keyframe: KeyFrame::mbFirstConnection (dsh_keyframe_update_connections)

  // INT32_MAX, which refuses every template, when the device cannot be asked
  int32_t largest_node() {
    if (max_node_stale) {
      max_node = -1;
      if (top_on_device) {
        int32_t* d = nullptr;
        if (hipSetDevice(device) != hipSuccess || ctx->scratch.take(4, (void**)&d) != hipSuccess ||
            hipMemcpyAsync(d, &max_node, 4, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
            ts_max_node_launch(d_nodes, P, d, ctx->stream) != hipSuccess ||
            hipMemcpyAsync(&max_node, d, 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
          return INT32_MAX;
      } else {
        for (const int32_t v : top_node) max_node = std::max(max_node, v);
      }
      max_node_stale = false;
    }
    return max_node;
  }
  void free_all() {
    for (void* p : {(void*)d_xyz, (void*)d_nrm, (void*)d_maxd, (void*)d_desc, (void*)d_bad, (void*)d_cnt, (void*)d_local_ids, (void*)d_visible,
                    (void*)d_found, (void*)d_nobs, (void*)d_nodes, (void*)d_ref_ids, (void*)d_bary, (void*)d_log, (void*)d_kf, (void*)d_table,
                    (void*)d_local_kf, (void*)d_hdr, (void*)d_last_ids, (void*)d_last_oct, (void*)d_ref_kf, (void*)d_log_idx, (void*)d_snap_point, (void*)d_snap_xyz,
                    (void*)d_cand_ids, (void*)d_surf_normal, (void*)d_surf_pts, (void*)d_surf_kpn, (void*)d_surf_has, (void*)d_surf_nn, (void*)d_surf_depth, (void*)d_view_px})
      if (p) (void)hipFree(p);
  }
};

inline uint64_t mpdb_obs_key(int32_t point, int32_t slot) { return ((uint64_t)(uint32_t)point << 32) | (uint32_t)slot; }

// the per-point tracking state as the kernels of trackclose_kernels.hip take it
inline TcState mpdb_state(const dsh_mpdb* db) {
  TcState s;
  s.xyz = db->d_xyz; s.bad = db->d_bad; s.visible = db->d_visible; s.found = db->d_found; s.nobs = db->d_nobs; s.nodes = db->d_nodes;
  s.bary = db->d_bary;
  return s;
}

inline hipError_t mpdb_reserve_points(dsh_mpdb* db, long long need) {
  if (need <= db->Pcap) return hipSuccess;
  const size_t cap = (size_t)std::min<long long>(std::max(need, 2ll * db->Pcap), INT32_MAX), P = (size_t)db->P;
  hipError_t e;
  if ((e = dsh_store_grow_array(&db->d_xyz, 3 * P, 3 * cap)) != hipSuccess || (e = dsh_store_grow_array(&db->d_nrm, 3 * P, 3 * cap)) != hipSuccess ||
      (e = dsh_store_grow_array(&db->d_maxd, P, cap)) != hipSuccess || (e = dsh_store_grow_array(&db->d_desc, 2 * P, 2 * cap)) != hipSuccess ||
      (e = dsh_store_grow_array(&db->d_bad, P, cap)) != hipSuccess || (e = dsh_store_grow_array(&db->d_cnt, P, cap)) != hipSuccess ||
      (e = dsh_store_grow_array(&db->d_local_ids, P, cap)) != hipSuccess || (e = dsh_store_grow_array(&db->d_ref_ids, P, cap)) != hipSuccess ||
      (e = dsh_store_grow_array(&db->d_visible, P, cap)) != hipSuccess || (e = dsh_store_grow_array(&db->d_found, P, cap)) != hipSuccess ||
      (e = dsh_store_grow_array(&db->d_nobs, P, cap)) != hipSuccess || (e = dsh_store_grow_array(&db->d_nodes, 3 * P, 3 * cap)) != hipSuccess ||
      (e = dsh_store_grow_array(&db->d_bary, 3 * P, 3 * cap)) != hipSuccess || (e = dsh_store_grow_array(&db->d_ref_kf, P, cap)) != hipSuccess)
    return e;
  db->Pcap = (int32_t)cap;
  return hipSuccess;
}

// room for `need` log records: the log and the key point indices beside it
inline hipError_t mpdb_reserve_log(dsh_mpdb* db, long long need) {
  if (need <= db->Rcap && db->d_log && db->d_log_idx) return hipSuccess;
  const size_t cap = (size_t)std::max(need, db->d_log ? 2 * db->Rcap : db->Rcap), R = (size_t)db->R;
  hipError_t e;
  if ((e = dsh_store_grow_array(&db->d_log, R, cap)) != hipSuccess || (e = dsh_store_grow_array(&db->d_log_idx, R, cap)) != hipSuccess) return e;
  db->Rcap = (long long)cap;
  return hipSuccess;
}

// room for a last-frame list and a keyframe candidate of N entries (the list it holds stays until the call that grows it writes the new one)
inline hipError_t mpdb_reserve_last_frame(dsh_mpdb* db, int32_t N) {
  if (N <= db->last_cap) return hipSuccess;
  const size_t cap = (size_t)std::max(N, 2 * db->last_cap), used = (size_t)std::max(db->last_N, 0);
  hipError_t e;
  if ((e = dsh_store_grow_array(&db->d_last_ids, used, cap)) != hipSuccess || (e = dsh_store_grow_array(&db->d_last_oct, used, cap)) != hipSuccess ||
      (e = dsh_store_grow_array(&db->d_cand_ids, (size_t)std::max(db->cand_N, 0), cap)) != hipSuccess)
    return e;
  db->last_cap = (int32_t)cap;
  return hipSuccess;
}

// room for `need` table entries: the tables, the snapshot and the surface points beside them
inline hipError_t mpdb_reserve_table(dsh_mpdb* db, long long need) {
  if (need <= db->Tcap && db->d_table && db->d_snap_point && db->d_snap_xyz && db->d_surf_normal && db->d_surf_pts && db->d_surf_kpn && db->d_surf_has &&
      db->d_view_px)
    return hipSuccess;
  const size_t cap = (size_t)std::max(need, db->d_table ? 2 * db->Tcap : db->Tcap), T = (size_t)db->T;
  hipError_t e;
  if ((e = dsh_store_grow_array(&db->d_table, T, cap)) != hipSuccess || (e = dsh_store_grow_array(&db->d_snap_point, T, cap)) != hipSuccess ||
      (e = dsh_store_grow_array(&db->d_snap_xyz, 3 * T, 3 * cap)) != hipSuccess ||
      (e = dsh_store_grow_array(&db->d_surf_normal, 3 * T, 3 * cap)) != hipSuccess || (e = dsh_store_grow_array(&db->d_surf_pts, 3 * T, 3 * cap)) != hipSuccess ||
      (e = dsh_store_grow_array(&db->d_surf_kpn, 2 * T, 2 * cap)) != hipSuccess || (e = dsh_store_grow_array(&db->d_surf_has, T, cap)) != hipSuccess ||
      (e = dsh_store_grow_array(&db->d_view_px, 2 * T, 2 * cap)) != hipSuccess)
    return e;
  db->Tcap = (long long)cap;
  return hipSuccess;
}

inline hipError_t mpdb_reserve_keyframes(dsh_mpdb* db, long long need) {
  if (need <= db->Kcap) return hipSuccess;
  const size_t cap = (size_t)std::min<long long>(std::max(need, 2ll * db->Kcap), INT32_MAX), K = (size_t)db->K;
  hipError_t e;
  if ((e = dsh_store_grow_array(&db->d_kf, K, cap)) != hipSuccess || (e = dsh_store_grow_array(&db->d_local_kf, K, cap)) != hipSuccess ||
      (e = dsh_store_grow_array(&db->d_surf_nn, K, cap)) != hipSuccess ||
      (e = dsh_store_grow_array(&db->d_surf_depth, (size_t)dsh_mpdb::SURF_MAX_CTRL * K, (size_t)dsh_mpdb::SURF_MAX_CTRL * cap)) != hipSuccess)
    return e;
  db->Kcap = (int32_t)cap;
  return hipSuccess;
}

// n distinct ids inside [0, count): the first fault in sorted order.  With repeat_first (the erase calls) a repeat is named ahead of
// an id outside the store, and that id is the first in the caller's order.
inline std::string mpdb_ids_error(int n, const int32_t* ids, int32_t count, const char* what, bool repeat_first = false) {
  if (n < 0) return "n < 0";
  if (n > 0 && !ids) return std::string(what) + " array is NULL";
  std::vector<int32_t> s(ids, ids + n);
  std::sort(s.begin(), s.end());
  if (repeat_first) {
    for (int i = 1; i < n; i++)
      if (s[i] == s[i - 1]) return std::string(what) + " " + std::to_string(s[i]) + " repeated in the batch";
    s.assign(ids, ids + n);   // distinct: the loop below finds the range alone
  }
  for (int i = 0; i < n; i++) {
    if (s[i] < 0 || s[i] >= count) return std::string(what) + " " + std::to_string(s[i]) + " outside the store";
    if (i > 0 && s[i] == s[i - 1]) return std::string(what) + " " + std::to_string(s[i]) + " repeated in the batch";
  }
  return "";
}

// a table of N entries that are -1 or a point of the store; entry i is named open + i + close in the message
inline std::string mpdb_table_error(const dsh_mpdb* db, int N, const int32_t* table, const char* open, const char* close) {
  for (int i = 0; i < N; i++)
    if (table[i] < -1 || table[i] >= db->P) return open + std::to_string(i) + close + " is neither -1 nor a point of the store";
  return "";
}

// an observation: a point and a keyframe of the store
inline std::string mpdb_pair_error(const dsh_mpdb* db, int32_t point, int32_t slot) {
  if (point < 0 || point >= db->P) return "point id outside the store";
  if (slot < 0 || slot >= db->K) return "keyframe slot outside the store";
  return "";
}

// DSH_ERR_STATE of an entry point that reads the key point index of every observation
inline int mpdb_unindexed_error(dsh_mpdb* db, const char* who) {
  return dsh_fail(db->ctx, DSH_ERR_STATE,
                  std::string(who) + ": the store holds " + std::to_string(db->unindexed.size()) +
                      " live observation records without a key point index (dsh_mpdb_add_observations); add them with dsh_point_store_add_observations_indexed");
}

// The builder of observation lists on the store's log: the temporaries of n lists with at most cap_obs observations.  off, n_dev,
// n_extra, kf and total stay with the caller.
inline hipError_t mpdb_obs_lists(dsh_mpdb* db, ObsLists& a, size_t n, size_t cap_obs) {
  a = ObsLists{};
  a.log = db->d_log; a.log_idx = db->d_log_idx; a.R = db->R; a.n = (int32_t)n;
  dsh_ctx_base* c = db->ctx;
  hipError_t e;
  if ((e = dsh_scratch_array(c, &a.sel_of, (size_t)db->P)) != hipSuccess || (e = dsh_scratch_array(c, &a.cnt, n)) != hipSuccess ||
      (e = dsh_scratch_array(c, &a.fill, n)) != hipSuccess || (e = dsh_scratch_array(c, &a.raw_slot, cap_obs)) != hipSuccess ||
      (e = dsh_scratch_array(c, &a.raw_idx, cap_obs)) != hipSuccess)
    return e;
  return hipSuccess;
}
