// Host logic of dsh_track_sft between its two device stages (dsh_tracksft.cpp): the downloaded observation table as the dsh_sft_frame the
// packer reads, the table handed to the caller, and the scatter of the result's flags into mvbOutlier.  Plain functions over host
// pointers, no HIP: tools/diag/tracksft_host_check.cpp runs them under AddressSanitizer on blocks of exactly the sizes of the call site.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/defslam_hip.h"

// the table where the download left it: M rows in arrays with room for N
struct TfTable {
  int32_t M = 0, points_obs = 0;
  const int32_t *kp_index = nullptr, *point_id = nullptr, *nodes = nullptr;
  const double *bary = nullptr, *uv = nullptr, *invsig2 = nullptr;
};

// DefOptimizer.cc:293-361 on the table: what dsh_sft_solve takes (n_frame is pFrame->N, the division of :340 is the packer's)
inline dsh_sft_frame tf_sft_frame(const dsh_track_sft_frame& f, const TfTable& t) {
  dsh_sft_frame s;
  std::memset(&s, 0, sizeof s);
  s.Tcw = f.Tcw;
  std::memcpy(s.K, f.K, sizeof s.K);
  s.n_frame = f.N;
  s.M = t.M;
  s.obs_nodes = t.nodes; s.obs_bary = t.bary; s.obs_uv = t.uv; s.obs_invsig2 = t.invsig2;
  s.xyz = f.xyz;
  s.reg_lap = f.reg_lap; s.reg_inex = f.reg_inex; s.reg_temp = f.reg_temp;
  s.neighbour_layers = f.neighbour_layers;
  s.max_iters = f.max_iters;
  return s;
}

// whether the caller's table has room for the rows (an array that is not given needs none)
inline bool tf_table_fits(const TfTable& t, const dsh_track_sft_table& out) {
  const bool any = out.kp_index || out.point_id || out.nodes || out.bary || out.uv || out.invsig2;
  return !any || out.capacity >= t.M;
}

inline void tf_hand_out(const TfTable& t, dsh_track_sft_table* out) {
  const size_t m = (size_t)t.M;
  out->M = t.M;
  out->points_obs = t.points_obs;
  if (m == 0) return;
  if (out->kp_index) std::memcpy(out->kp_index, t.kp_index, 4 * m);
  if (out->point_id) std::memcpy(out->point_id, t.point_id, 4 * m);
  if (out->nodes) std::memcpy(out->nodes, t.nodes, 12 * m);
  if (out->bary) std::memcpy(out->bary, t.bary, 24 * m);
  if (out->uv) std::memcpy(out->uv, t.uv, 16 * m);
  if (out->invsig2) std::memcpy(out->invsig2, t.invsig2, 8 * m);
}

// DefOptimizer.cc:515-537: the flag of every row goes to its key point, every other entry keeps its value
inline void tf_scatter_flags(const TfTable& t, const uint8_t* flags, uint8_t* outlier) {
  for (int32_t m = 0; m < t.M; m++) outlier[t.kp_index[m]] = flags[m];
}
