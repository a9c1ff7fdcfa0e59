// The creation of a keyframe on the two resident stores and its covisibility connections (dsh_keyframe_create,
// dsh_keyframe_update_connections; gfx950).
//   DefTracking::CreateNewKeyFrame   Modules/Tracking/DefTracking.cc:696-707
//   KeyFrame::KeyFrame(Frame&, ..)   Thirdparty/ORBSLAM_2/src/KeyFrame.cc:37-75
//   DefKeyFrame::DefKeyFrame         Modules/Common/DefKeyFrame.cc:42-77
//   KeyFrame::UpdateConnections      Thirdparty/ORBSLAM_2/src/KeyFrame.cc:326-419
// kc_create_kernel    the one upload block of a new keyframe into the arrays of both stores: descriptor rows, octaves, pyramid and the
//                     centre of Tcw (sr_camera_centre, surfreg_problem.h) into dsh_kfdb; the record, the table (from the block or from the
//                     resident keyframe candidate), an empty snapshot and Surface(N) into dsh_mpdb.  The snapshot itself is
//                     sr_snapshot_kernel (surfreg_kernels.hip), launched behind it.
// kc_clear_kernel, kc_scatter_kernel, kc_votes_kernel
//                     the weights: the vote of mpdb_device.h (vote_scatter, vote_sweep) with the keyframe's table as the frame and its
//                     own slot left out
// kc_order_kernel     a thread per keyframe.  (weight << 16) | slot is a unique key, so the place of a keyframe in a list is a COUNT:
//                     among the counted ones the slots below it, among the connected ones the larger keys.  Every workgroup walks all K
//                     weights once, a tile of connected keys in LDS at a time (a compare and an add per key and connected thread; tens
//                     of keyframes in a running map, 65535 at most, which is 256 workgroups of 256 tiles) and, on the way, sums up what
//                     the header needs -- n_counted, n_connected, the two maxima -- and the counted keyframes in front of its own
//                     tile for itself, so there is no launch between the weights and the lists; the rank inside its own tile is a
//                     ballot (tile_rank).  Workgroup 0 writes the header, the fallback pair and the parent.
// Integer valued except the centre: compiled without FMA contraction like surfreg_kernels.hip, which states the centre.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "keyframe_create_problem.h"
#include "mpdb_device.h"
#include "surfreg_problem.h"

namespace {

__global__ __launch_bounds__(KC_BLOCK) void kc_create_kernel(KcCreate k) {
  const int i = blockIdx.x * KC_BLOCK + threadIdx.x;
  bool held = false;
  if (i < k.N) {
    const size_t r = (size_t)k.row_off + i, e = (size_t)k.tab_off + i;
    k.rows[2 * r] = k.src_rows[2 * (size_t)i];
    k.rows[2 * r + 1] = k.src_rows[2 * (size_t)i + 1];
    k.oct[r] = k.src_oct[i];
    const int p = k.src_points[i];
    held = p >= 0;
    k.table[e] = p;
    k.snap_point[e] = -1;   // no snapshot yet: sr_snapshot_kernel takes it next
    if (k.src_kpn) {        // Surface(N): no normal, x3D zeros (Surface.cc:31-37), and mpKeypointNorm
      for (int c = 0; c < 3; c++) { k.surf_normal[3 * e + c] = 0.f; k.surf_pts[3 * e + c] = 0.f; }
      k.surf_has[e] = 0;
      k.surf_kpn[2 * e] = k.src_kpn[2 * (size_t)i];
      k.surf_kpn[2 * e + 1] = k.src_kpn[2 * (size_t)i + 1];
    }
  }
  wave_count(held, &k.out->n_held);
  if (blockIdx.x == 0) {
    const int t = threadIdx.x;
    if (t < MPU_MAX_LEVELS) k.sf[t] = k.src_sf[t];
    if (t < 3) {
      const float o = sr_camera_centre(k.Tcw, t);
      k.kf_slot->Ow[t] = o;
      k.out->Ow[t] = o;
    }
    if (t == 0) {
      k.kf_slot->row_off = k.row_off;
      *k.levels_out = k.levels;
      LmKf f;
      f.tab_off = k.tab_off; f.N = k.N; f.parent = -1; f.bad = 0;
      *k.kf = f;
      if (k.src_kpn) *k.surf_nn = 0;
    }
  }
}

__global__ __launch_bounds__(KC_BLOCK) void kc_clear_kernel(KcConn k) {
  const int i = blockIdx.x * KC_BLOCK + threadIdx.x;
  if (i < k.P) k.cnt[i] = 0;
  if (i < k.K) k.w[i] = 0;
}

__global__ __launch_bounds__(KC_BLOCK) void kc_scatter_kernel(KcConn k) {
  const int i = blockIdx.x * KC_BLOCK + threadIdx.x;
  if (i < k.N) (void)vote_scatter(k.bad, k.cnt, k.table[(size_t)k.tab_off + i]);   // KeyFrame.cc:341-347: pMP, !isBad
}

__global__ __launch_bounds__(LM_BLOCK) void kc_votes_kernel(KcConn k) {
  __shared__ int hist[LM_BINS];
  vote_sweep<LM_BLOCK, LM_BINS>(k.log, k.R, k.cnt, k.w, k.K, k.slot, hist);   // :351-356: mnId == this->mnId is skipped, no isBad of the other
}

__global__ __launch_bounds__(KC_BLOCK) void kc_order_kernel(KcConn k) {
  __shared__ __attribute__((aligned(16))) int tile[KC_BLOCK];
  __shared__ int part[5][KC_BLOCK / 64];
  __shared__ int wsum[KC_BLOCK / 64];
  const int t = threadIdx.x, first_of_mine = blockIdx.x * KC_BLOCK, me = first_of_mine + t;
  const int wm = me < k.K ? k.w[me] : 0;
  const bool connected = wm >= k.th;                   // th >= 1: a connected keyframe is a counted one
  const int key = (wm << 16) | me;
  int above = 0;                                       // connected keys above mine
  int n_counted = 0, n_conn = 0, n_before = 0, top_hi = -1, top_lo = -1;
  for (int base = 0; base < k.K; base += KC_BLOCK) {
    const int j = base + t;
    const int wj = j < k.K ? k.w[j] : 0;
    tile[t] = wj >= k.th ? (wj << 16) | j : -1;        // the key of a connected keyframe; -1 is above nobody
    if (wj > 0) {
      n_counted++;
      n_before += base < first_of_mine;                // the counted keyframes of the workgroups before this one
      n_conn += wj >= k.th;
      top_hi = max(top_hi, (wj << 16) | j);                        // the largest weight, the HIGHEST slot among equals: the sort (:395-402)
      top_lo = max(top_lo, (wj << 16) | (KC_MAX_KEYFRAMES - j));   // the largest weight, the LOWEST slot among equals: pKFmax (:373-381)
    }
    __syncthreads();
    if (connected) {   // the whole tile, four keys a read: a compare and an add per key
      const int4* quad = reinterpret_cast<const int4*>(tile);
#pragma unroll 8
      for (int q = 0; q < KC_BLOCK / 4; q++) {
        const int4 v = quad[q];
        above += (v.x > key) + (v.y > key) + (v.z > key) + (v.w > key);
      }
    }
    __syncthreads();
  }
  // among the counted ones the slots below mine: those of the workgroups before, and the rank inside this one
  int in_block;
  const int below_here = tile_rank<KC_BLOCK>(wm > 0, wsum, in_block);
  for (int off = 32; off > 0; off >>= 1) {
    n_counted += __shfl_xor(n_counted, off, 64);
    n_conn += __shfl_xor(n_conn, off, 64);
    n_before += __shfl_xor(n_before, off, 64);
    top_hi = max(top_hi, __shfl_xor(top_hi, off, 64));
    top_lo = max(top_lo, __shfl_xor(top_lo, off, 64));
  }
  if ((t & 63) == 0) {
    part[0][t >> 6] = n_counted; part[1][t >> 6] = n_conn; part[2][t >> 6] = top_hi; part[3][t >> 6] = top_lo; part[4][t >> 6] = n_before;
  }
  __syncthreads();
  n_counted = n_conn = n_before = 0;
  for (int w = 0; w < KC_BLOCK / 64; w++) {
    n_counted += part[0][w];
    n_conn += part[1][w];
    top_hi = max(top_hi, part[2][w]);
    top_lo = max(top_lo, part[3][w]);
    n_before += part[4][w];
  }
  const int below = n_before + below_here;
  if (n_counted == 0) {   // vpConnectedKFs.empty() is not reached: KFcounter.empty() returns first (:361)
    if (me == 0) {
      KcConnOut h = {};
      h.parent = k.kf[k.slot].parent;
      h.max_kf = -1;
      *k.hdr = h;
    }
    return;
  }
  if (wm > 0) {
    k.counted_kf[below] = me;
    k.counted_w[below] = wm;
    if (connected) {      // n_conn > 0 here: the list is the connected keyframes by descending key
      k.ordered_kf[above] = me;
      k.ordered_w[above] = wm;
    }
  }
  if (me == 0) {
    KcConnOut h = {};
    h.n_counted = n_counted;
    h.max_weight = top_lo >> 16;
    h.max_kf = KC_MAX_KEYFRAMES - (top_lo & 0xffff);
    h.n_connected = n_conn;
    int first = top_hi & 0xffff;
    if (n_conn == 0) {    // :388-393: nobody reaches th, the best one alone
      h.n_connected = 1;
      first = h.max_kf;
      k.ordered_kf[0] = h.max_kf;
      k.ordered_w[0] = h.max_weight;
    }
    if (k.first && k.slot != 0) {   // :412-417
      k.kf[k.slot].parent = first;
      h.parent_set = 1;
      h.parent = first;
    } else {
      h.parent = k.kf[k.slot].parent;
    }
    *k.hdr = h;
  }
}

}  // namespace

static_assert(sizeof(KcCreateOut) == 32 && sizeof(KcConnOut) == 32, "the result blocks are eight words");
static_assert(KC_MAX_KEYPOINTS <= (1 << 14) && KC_MAX_KEYFRAMES < (1 << 16), "(weight << 16) | slot must stay a positive int32");

extern "C" hipError_t kc_create_launch(const KcCreate& k, hipStream_t st) {
  hipLaunchKernelGGL(kc_create_kernel, dim3(blocks_for(k.N > 0 ? k.N : 1, KC_BLOCK)), dim3(KC_BLOCK), 0, st, k);
  return hipGetLastError();
}

extern "C" hipError_t kc_connections_launch(const KcConn& k, hipStream_t st) {
  const int top = k.P > k.K ? k.P : k.K;
  hipLaunchKernelGGL(kc_clear_kernel, dim3(blocks_for(top, KC_BLOCK)), dim3(KC_BLOCK), 0, st, k);
  if (k.N > 0) hipLaunchKernelGGL(kc_scatter_kernel, dim3(blocks_for(k.N, KC_BLOCK)), dim3(KC_BLOCK), 0, st, k);
  if (k.R > 0 && k.N > 0) hipLaunchKernelGGL(kc_votes_kernel, dim3(log_blocks(k.R, LM_BLOCK)), dim3(LM_BLOCK), 0, st, k);
  hipLaunchKernelGGL(kc_order_kernel, dim3(blocks_for(k.K, KC_BLOCK)), dim3(KC_BLOCK), 0, st, k);
  return hipGetLastError();
}
