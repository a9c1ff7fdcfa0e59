// One anchor of SchwarpDatabase::add on the resident stores (dsh_keyframe_warp_pair; gfx950): the integer and gather stages around the
// numeric kernels of nrsfm_kernels.hip -- DefORBmatcher::findbyWarp (DefORBmatcher.cc:47-71, :111-187) and the bookkeeping loop of
// SchwarpDatabase::calculateSchwarps (SchwarpDatabase.cc:268-346) on dsh_mpdb's tables, log and per-point state.  The launches, in
// stream order; every count a later launch needs stays in WpHdr:
//   wp_clear_kernel      the per-call arrays over points and key points, the counters
//   wp_log_kernel        one pass over the log: the live record (p, slot), the key point index of the live record (p, anchor), and for a
//                        point whose reference keyframe is `slot` the lowest other slot among its live records
//   wp_gather_kernel     stage 1: key points, inverse sigmas, query key points and descriptor rows
//   wp_fix_start_kernel  the tail of stage 2, one workgroup: the verdict on the initialisation, NaN control points -> 0
//   wp_filter_kernel     stage 3 behind the evaluation, ONE workgroup: lane 0 adds the squares in index order, then the test per match,
//                        the table clears and the ordered compaction of the kept matches; at its end the `has` flags of the search
//   wp_register_kernel   stage 4 behind the search, ONE workgroup: the first query per point and the last query per key point by
//                        integer atomics, then the queries in order -- the appended records, n_obs, the table entries, the kept list
//   wp_resolve_kernel    stage 7, ONE workgroup: the elections of the alive dropped entries repeated until the alive flags stop
//                        changing, the state per entry, then EraseObservation of the elected entries
//   wp_cascade_kernel    one pass over the log that leaves at once when no point was set bad: setBadFlag's records and table entries
// The ordered stages run in one workgroup because their outputs are positions in lists; their work is a few integer operations per
// entry of at most 16384.  Compiled without FMA contraction (see include/defslam_hip.h).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "mpdb_device.h"
#include "warppair_problem.h"

namespace {

__global__ __launch_bounds__(WP_BLOCK) void wp_clear_kernel(WpBufs b) {
  const int i = blockIdx.x * WP_BLOCK + threadIdx.x;
  if (i < b.P) { b.rec_slot[i] = -1; b.anc_idx[i] = -1; b.cand[i] = WP_NONE; b.first[i] = WP_NONE; b.mark[i] = 0; }
  if (i < b.N2) b.win2[i] = -1;
  if (i < b.N1) b.kill1[i] = WP_NONE;
  if (i == 0) {
    WpHdr h = {};
    h.max_pid = -1;
    *b.hdr = h;
  }
}

__global__ __launch_bounds__(WP_BLOCK) void wp_log_kernel(WpBufs b) {
  for (long long r = (long long)blockIdx.x * WP_BLOCK + threadIdx.x; r < b.R; r += (long long)gridDim.x * WP_BLOCK) {
    const int2 rec = b.log[r];
    if (rec.x < 0) continue;
    if (rec.y == b.slot) b.rec_slot[rec.x] = (int32_t)r;            // at most one live record per pair
    else if (b.ref_kf[rec.x] == b.slot) atomicMin(&b.cand[rec.x], rec.y);   // mObservations.begin()->first once (p, slot) is gone
    if (rec.y == b.anchor) b.anc_idx[rec.x] = b.log_idx[r];
  }
}

// sqrt(mvInvLevelSigma2[octave]) of key point i of the anchor: float32, every operation rounded (ORBextractor.cc:422,430)
__device__ __forceinline__ float inv_sigma(const WpBufs& b, int i) {
  const int o = b.oct[(size_t)b.slots[b.anchor].row_off + i];      // < levels: the host refuses a store with an octave >= levels
  const float sf = b.sf[MPU_MAX_LEVELS * (size_t)b.anchor + o];
  const float sigma2 = sf * sf;
  const float inv = 1.0f / sigma2;
  return sqrtf(inv);
}

__global__ __launch_bounds__(WP_BLOCK) void wp_gather_kernel(WpBufs b) {
  const int i = blockIdx.x * WP_BLOCK + threadIdx.x;
  if (i < b.n_pairs) {
    const int i1 = b.pair_idx1[i], i2 = b.pair_idx2[i];
    b.g_kp1[2 * i] = b.kpn[2 * (size_t)(b.off1 + i1)]; b.g_kp1[2 * i + 1] = b.kpn[2 * (size_t)(b.off1 + i1) + 1];
    b.g_kp2[2 * i] = b.kpn[2 * (size_t)(b.off2 + i2)]; b.g_kp2[2 * i + 1] = b.kpn[2 * (size_t)(b.off2 + i2) + 1];
    b.g_isg[i] = inv_sigma(b, i1);
  }
  if (i < b.n_queries) {
    const int i1 = b.query_idx1[i];
    b.q_kp1[2 * i] = b.kpn[2 * (size_t)(b.off1 + i1)]; b.q_kp1[2 * i + 1] = b.kpn[2 * (size_t)(b.off1 + i1) + 1];
    const size_t row = (size_t)b.slots[b.anchor].row_off + i1;
    b.q_desc[2 * (size_t)i] = b.rows[2 * row];
    b.q_desc[2 * (size_t)i + 1] = b.rows[2 * row + 1];
  }
}

// dsh_warp_initialize's verdict (a factorisation that went through and finite control points), taken before the NaN entries among
// the first nan_limit values become 0 (DefORBmatcher.cc:139-152)
__global__ __launch_bounds__(WP_SEQ_BLOCK) void wp_fix_start_kernel(WpBufs b) {
  bool finite = true;
  for (int i = threadIdx.x; i < b.n_ctrl; i += WP_SEQ_BLOCK) finite = finite && isfinite(b.x[i]);
  const int all = __syncthreads_and(finite ? 1 : 0);
  if (threadIdx.x == 0) b.hdr->init_ok = ((b.scal[2] != 0.0 || b.scal[3] != 0.0) && all) ? 1 : 0;
  for (int i = threadIdx.x; i < b.nan_limit; i += WP_SEQ_BLOCK)
    if (isnan(b.x[i])) b.x[i] = 0.0;
}

__global__ __launch_bounds__(WP_SEQ_BLOCK) void wp_filter_kernel(WpBufs b) {
  __shared__ int wsum[WP_SEQ_BLOCK / 64];
  __shared__ double scale;
  __shared__ double sq[WP_SEQ_BLOCK];
  // Ceres' Corrector for HuberLoss(5.77) on the one block of 2P residuals: the sum in index order, as a host loop forms it.  The squares
  // are formed by the workgroup, a tile at a time; lane 0 adds them from LDS, so the dependent chain is the additions alone
  double s = 0.0;
  for (int t0 = 0; t0 < 2 * b.n_pairs; t0 += WP_SEQ_BLOCK) {
    const int i = t0 + threadIdx.x, n = min(WP_SEQ_BLOCK, 2 * b.n_pairs - t0);
    if (i < 2 * b.n_pairs) sq[threadIdx.x] = b.res[i] * b.res[i];
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll 8
      for (int k = 0; k < n; k++) s = s + sq[k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) scale = s > 5.77 * 5.77 ? sqrt(5.77 / sqrt(s)) : 1.0;
  __syncthreads();
  const double sc = scale;
  int base = 0;
  for (int t0 = 0; t0 < b.n_pairs; t0 += WP_SEQ_BLOCK) {
    const int i = t0 + threadIdx.x;
    bool keep = false;
    if (i < b.n_pairs) {
      const double r0 = b.res[2 * i] * sc, r1 = b.res[2 * i + 1] * sc;
      const double q0 = r0 * r0, q1 = r1 * r1;
      const double error = q0 + q1;
      keep = !(error > 20);
      if (!keep) {
        b.table[b.off2 + b.pair_idx2[i]] = -1;                      // EraseMapPointMatch; the observation stays
        b.pair_state[i] = DSH_WARP_FILTERED;
      }
    }
    const int pos = ordered_slot<WP_SEQ_BLOCK>(keep, base, wsum);
    if (keep) {   // pos <= i < n_pairs
      b.k_idx1[pos] = b.pair_idx1[i]; b.k_idx2[pos] = b.pair_idx2[i]; b.k_src[pos] = i;
      b.k_kp1[2 * pos] = b.g_kp1[2 * i]; b.k_kp1[2 * pos + 1] = b.g_kp1[2 * i + 1];
      b.k_kp2[2 * pos] = b.g_kp2[2 * i]; b.k_kp2[2 * pos + 1] = b.g_kp2[2 * i + 1];
      b.k_isg[pos] = b.g_isg[i];
      b.pair_state[i] = DSH_WARP_UNFITTED;
    }
  }
  if (threadIdx.x == 0) { b.hdr->n_kept_pairs = base; b.hdr->n_filtered = b.n_pairs - base; b.hdr->n_list = base; }
  __threadfence();
  __syncthreads();   // the clears above are this workgroup's own
  for (int j = threadIdx.x; j < b.N2; j += WP_SEQ_BLOCK) b.has[j] = b.table[b.off2 + j] != -1;
}

// DefORBmatcher.cc:57-70 over the queries in order
__global__ __launch_bounds__(WP_SEQ_BLOCK) void wp_register_kernel(WpBufs b) {
  __shared__ int wsum[WP_SEQ_BLOCK / 64];
  for (int q = threadIdx.x; q < b.n_queries; q += WP_SEQ_BLOCK) {
    const int m = b.match[q];
    const int p = b.table[b.off1 + b.query_idx1[q]];
    if (m >= 0 && p >= 0) {
      atomicMin(&b.first[p], q);
      atomicMax(&b.win2[m], q);
    }
  }
  __threadfence();
  __syncthreads();
  const int list0 = b.hdr->n_kept_pairs;
  int n_add = 0, n_match = 0;
  for (int t0 = 0; t0 < b.n_queries; t0 += WP_SEQ_BLOCK) {
    const int q = t0 + threadIdx.x;
    int m = -1, p = -1, i1 = 0;
    bool add = false;
    if (q < b.n_queries) {
      m = b.match[q];
      i1 = b.query_idx1[q];
      p = b.table[b.off1 + i1];
      // MapPoint::AddObservation returns early on a point that observes the keyframe already (MapPoint.cc:112)
      add = m >= 0 && p >= 0 && b.first[p] == q && b.rec_slot[p] < 0;
      b.query_point[q] = m >= 0 ? p : -1;
      b.query_added[q] = add ? 1 : 0;
      b.query_state[q] = m >= 0 ? DSH_WARP_UNFITTED : DSH_WARP_NO_MATCH;
    }
    const int at = ordered_slot<WP_SEQ_BLOCK>(add, n_add, wsum);
    if (add) {   // at < n_queries: the host reserved that many records behind R
      b.log[b.R + at] = make_int2(p, b.slot);
      b.log_idx[b.R + at] = m;
      b.nobs[p] += 1;                                               // one query per point gets here
      b.rec_slot[p] = (int32_t)(b.R + at);
    }
    const int pos = list0 + ordered_slot<WP_SEQ_BLOCK>(m >= 0, n_match, wsum);
    if (m >= 0) {   // pos < n_pairs + n_queries
      if (p >= 0 && b.win2[m] == q) b.table[b.off2 + m] = p;       // KeyFrame::addMapPoint: the last in query order holds the entry
      b.k_idx1[pos] = i1; b.k_idx2[pos] = m; b.k_src[pos] = b.n_pairs + q;
      b.k_kp1[2 * pos] = b.q_kp1[2 * q]; b.k_kp1[2 * pos + 1] = b.q_kp1[2 * q + 1];
      b.k_kp2[2 * pos] = b.kpn[2 * (size_t)(b.off2 + m)]; b.k_kp2[2 * pos + 1] = b.kpn[2 * (size_t)(b.off2 + m) + 1];
      b.k_isg[pos] = inv_sigma(b, i1);
    }
  }
  if (threadIdx.x == 0) { b.hdr->n_matched = n_match; b.hdr->n_appended = n_add; b.hdr->n_list = list0 + n_match; }
}

// the position at which the first alive dropped entry of point p sets it bad, WP_NONE when it does not: EraseObservation finds the
// record (p, slot) and leaves n_obs <= 2 (MapPoint.cc:127-145)
__device__ __forceinline__ int bad_at(const WpBufs& b, int p) {
  const int j = b.first[p];
  return (j != WP_NONE && b.rec_slot[p] >= 0 && b.nobs[p] - 1 <= 2) ? j : WP_NONE;
}

// SchwarpDatabase.cc:268-346 over the kept list of L entries
__global__ __launch_bounds__(WP_SEQ_BLOCK) void wp_resolve_kernel(WpBufs b, int L) {
  const int t = threadIdx.x;
  for (int j = t; j < L; j += WP_SEQ_BLOCK) {
    const int p1 = b.table[b.off1 + b.k_idx1[j]], p2 = b.table[b.off2 + b.k_idx2[j]];
    b.e_p1[j] = p1; b.e_p2[j] = p2;
    b.e_alive[j] = p1 >= 0 && p2 >= 0 && !b.bad[p1] && !b.bad[p2];
    b.k_tag[j] = b.tag;
  }
  __threadfence();
  __syncthreads();
  // Entry j is reached alive unless a dropped entry before it, itself reached alive, took its idx2, set one of its points bad or cleared
  // its entry of the anchor.  The flags of a round follow from the elections over the flags of the round before; entry j depends on
  // entries before j alone, so after round k the first k entries of every chain are final and the loop ends after at most L rounds.
  int rounds = 0;
  for (;;) {
    rounds++;
    for (int j = t; j < L; j += WP_SEQ_BLOCK) {
      const int p1 = b.e_p1[j], p2 = b.e_p2[j];
      b.win2[b.k_idx2[j]] = WP_NONE;
      if (p1 >= 0) b.first[p1] = WP_NONE;   // (stage 4 left its queries in `first`)
      if (p2 >= 0) {
        b.first[p2] = WP_NONE;
        if (b.anc_idx[p2] >= 0 && b.anc_idx[p2] < b.N1) b.kill1[b.anc_idx[p2]] = WP_NONE;
      }
    }
    __threadfence();
    __syncthreads();
    for (int j = t; j < L; j += WP_SEQ_BLOCK)
      if (b.e_alive[j] && b.drop[j]) {
        atomicMin(&b.first[b.e_p2[j]], j);
        atomicMin(&b.win2[b.k_idx2[j]], j);
      }
    __threadfence();
    __syncthreads();
    for (int j = t; j < L; j += WP_SEQ_BLOCK)
      if (b.e_alive[j] && b.drop[j]) {
        const int p2 = b.e_p2[j], a = b.anc_idx[p2];
        if (b.first[p2] == j && bad_at(b, p2) == j && a >= 0 && a < b.N1) atomicMin(&b.kill1[a], j);   // setBadFlag clears the anchor's entry
      }
    __threadfence();
    __syncthreads();
    int changed = 0;
    for (int j = t; j < L; j += WP_SEQ_BLOCK) {
      const int p1 = b.e_p1[j], p2 = b.e_p2[j];
      bool alive = p1 >= 0 && p2 >= 0 && !b.bad[p1] && !b.bad[p2];
      alive = alive && !(b.win2[b.k_idx2[j]] < j) && !(bad_at(b, p1) < j) && !(bad_at(b, p2) < j) && !(b.kill1[b.k_idx1[j]] < j);
      if ((b.e_alive[j] != 0) != alive) changed = 1;
      b.e_alive[j] = alive;
    }
    __threadfence();
    if (!__syncthreads_or(changed) || rounds > L) break;
  }
  // the state per entry; nothing of the stores is written before every entry has read what it needs
  int n_skip = 0, n_drop = 0, n_keep = 0, n_store = 0;
  for (int j = t; j < L; j += WP_SEQ_BLOCK) {
    const int p1 = b.e_p1[j];
    int state;
    if (!b.e_alive[j]) { state = DSH_WARP_SKIPPED; n_skip++; }
    else if (b.drop[j]) { state = DSH_WARP_DROPPED; n_drop++; }
    else {
      // GetReferenceKeyFrame of p1 when the loop reaches j: an earlier drop that erased the record (p1, slot) of a point anchored in
      // `slot` has moved it to the lowest remaining slot (MapPoint.cc:137-138)
      int ref = b.ref_kf[p1];
      if (b.first[p1] < j && b.rec_slot[p1] >= 0 && ref == b.slot && b.cand[p1] != WP_NONE) ref = b.cand[p1];
      if (ref != b.anchor) { state = DSH_WARP_KEPT; n_keep++; }
      else { state = DSH_WARP_STORED; n_store++; atomicMax(&b.hdr->max_pid, p1); }
    }
    b.k_pid[j] = state == DSH_WARP_STORED ? p1 : -1;
    const int src = b.k_src[j];
    if (src < b.n_pairs) b.pair_state[src] = (uint8_t)state;
    else b.query_state[src - b.n_pairs] = (uint8_t)state;
  }
  atomicAdd(&b.hdr->n_skipped, n_skip); atomicAdd(&b.hdr->n_dropped, n_drop); atomicAdd(&b.hdr->n_kept, n_keep); atomicAdd(&b.hdr->n_stored, n_store);
  if (t == 0) b.hdr->rounds = rounds;
  __threadfence();
  __syncthreads();
  // the drops: the elected entry of a point runs EraseObservation, every dropped entry clears its own table entry
  for (int j0 = 0; j0 < L; j0 += WP_SEQ_BLOCK) {   // whole wavefronts: the append below ballots
    const int j = j0 + t;
    bool found = false, moved = false, doomed = false;
    int p2 = -1;
    if (j < L && b.e_alive[j] && b.drop[j]) {
      p2 = b.e_p2[j];
      b.table[b.off2 + b.k_idx2[j]] = -1;                           // SchwarpDatabase.cc:291
      const int r = b.rec_slot[p2];
      if (b.first[p2] == j && r >= 0) {                             // MapPoint.cc:127
        found = true;
        b.log[r].x = -1;                                            // :135
        const int left = b.nobs[p2] - 1;                            // :133
        b.nobs[p2] = left;
        if (b.ref_kf[p2] == b.slot && b.cand[p2] != WP_NONE) { b.ref_kf[p2] = b.cand[p2]; moved = true; }   // :137-138
        if (left <= 2) { doomed = true; b.mark[p2] = 1; b.bad[p2] = 1; }   // :141, DefMapPoint.cc:82
      }
    }
    const int at = wave_append(found, &b.hdr->n_listed);
    if (found) b.out_erased[at] = make_int2(p2, b.slot);
    wave_count(found, &b.hdr->n_found);
    wave_count(moved, &b.hdr->n_ref_moved);
    wave_count(doomed, &b.hdr->n_set_bad);
  }
}

// DefMapPoint::setBadFlag's loop over the observations (DefMapPoint.cc:83-91) of the points stage 7 set bad
__global__ __launch_bounds__(WP_BLOCK) void wp_cascade_kernel(WpBufs b) {
  if (b.hdr->n_set_bad == 0) return;
  const long long R = b.R + b.hdr->n_appended;   // what lies behind the appended records was never written
  const long long stride = (long long)gridDim.x * WP_BLOCK;
  for (long long r0 = (long long)blockIdx.x * WP_BLOCK; r0 < R; r0 += stride) {   // wave-uniform trip count: the ballot sees 64 lanes
    const long long r = r0 + threadIdx.x;
    int2 rec = make_int2(-1, -1);
    if (r < R) rec = b.log[r];
    const bool doomed = rec.x >= 0 && b.mark[rec.x] != 0;
    const int at = wave_append(doomed, &b.hdr->n_listed);
    if (doomed) {
      const LmKf k = b.kf[rec.y];
      const int idx = b.log_idx[r];
      if ((unsigned)idx < (unsigned)k.N) b.table[(size_t)k.tab_off + idx] = -1;   // EraseMapPointMatch, whatever the entry holds
      b.log[r].x = -1;
      b.out_erased[at] = rec;                                       // inside the list: it has room for every live record
    }
    wave_count(doomed, &b.hdr->n_erased);
  }
}

}  // namespace

extern "C" hipError_t wp_gather_launch(const WpBufs& b, hipStream_t st) {
  int top = b.P > b.N1 ? b.P : b.N1;
  top = top > b.N2 ? top : b.N2;
  hipLaunchKernelGGL(wp_clear_kernel, dim3(blocks_for(top > 1 ? top : 1, WP_BLOCK)), dim3(WP_BLOCK), 0, st, b);
  if (b.R > 0) hipLaunchKernelGGL(wp_log_kernel, dim3(log_blocks(b.R, WP_BLOCK)), dim3(WP_BLOCK), 0, st, b);
  const int n = b.n_pairs > b.n_queries ? b.n_pairs : b.n_queries;
  if (n > 0) hipLaunchKernelGGL(wp_gather_kernel, dim3(blocks_for(n, WP_BLOCK)), dim3(WP_BLOCK), 0, st, b);
  return hipGetLastError();
}

extern "C" hipError_t wp_fix_start_launch(const WpBufs& b, hipStream_t st) {
  hipLaunchKernelGGL(wp_fix_start_kernel, dim3(1), dim3(WP_SEQ_BLOCK), 0, st, b);
  return hipGetLastError();
}

extern "C" hipError_t wp_filter_launch(const WpBufs& b, hipStream_t st) {
  hipLaunchKernelGGL(wp_filter_kernel, dim3(1), dim3(WP_SEQ_BLOCK), 0, st, b);
  return hipGetLastError();
}

extern "C" hipError_t wp_register_launch(const WpBufs& b, hipStream_t st) {
  hipLaunchKernelGGL(wp_register_kernel, dim3(1), dim3(WP_SEQ_BLOCK), 0, st, b);
  return hipGetLastError();
}

extern "C" hipError_t wp_resolve_launch(const WpBufs& b, int L, hipStream_t st) {
  hipLaunchKernelGGL(wp_resolve_kernel, dim3(1), dim3(WP_SEQ_BLOCK), 0, st, b, L);
  hipLaunchKernelGGL(wp_cascade_kernel, dim3(log_blocks(b.R + b.n_queries, WP_BLOCK)), dim3(WP_BLOCK), 0, st, b);   // a grid for every record stage 4 can append
  return hipGetLastError();
}
