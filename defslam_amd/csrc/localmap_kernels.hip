// The local map of the tracking thread from the resident map point store (dsh_local_map_update, dsh_local_map_search; gfx950).
//   Tracking::UpdateLocalKeyFrames   Thirdparty/ORBSLAM_2/src/Tracking.cc:1510-1629
//   DefTracking::UpdateLocalPoints   Modules/Tracking/DefTracking.cc:426-454
// Seven launches, no host round trip between them, every value an integer:
//   lm_clear_kernel     zero the per-call arrays
//   lm_scatter_kernel   the frame's multiplicities into cnt[point]; bad points reported
//   lm_votes_kernel     one coalesced pass over the observation log; votes accumulate in an LDS histogram per workgroup and leave with
//                       one global atomic per workgroup and touched keyframe (the records of a map concentrate on few keyframes: an
//                       atomic per record would serialise on them)
//   lm_build_kernel     ONE wavefront: the voted list in slot order, pKFmax, the serial expansion (at most 81 visits)
//   lm_flags_kernel     a workgroup per local keyframe marks the points of its table
//   lm_count_kernel, lm_compact_kernel   ordered compaction of the marks into the local id list (64-bit ballots, then block offsets)
// Where the reference iterates pointer-ordered containers the order here is the index: keyframes by slot, points by id.
#include "localmap_problem.h"
#include "mpdb_device.h"

namespace {

__global__ __launch_bounds__(LM_BLOCK) void lm_clear_kernel(LmBufs b) {
  const int i = blockIdx.x * LM_BLOCK + threadIdx.x;
  if (i < b.P) { b.cnt[i] = 0; b.flag[i] = 0; }
  if (i < b.K) { b.votes[i] = 0; b.mark[i] = 0; }
  if (i == 0) { b.hdr->n_local_points = 0; b.out_hdr->n_local_points = 0; }
}

__global__ __launch_bounds__(LM_BLOCK) void lm_scatter_kernel(LmBufs b) {
  const int i = blockIdx.x * LM_BLOCK + threadIdx.x;
  if (i >= b.N) return;
  b.out_frame_bad[i] = vote_scatter(b.bad, b.cnt, b.frame_points[i]) ? 1 : 0;   // Tracking.cc:1527-1530
}

__global__ __launch_bounds__(LM_BLOCK) void lm_votes_kernel(LmBufs b) {
  __shared__ int hist[LM_BINS];
  vote_sweep<LM_BLOCK, LM_BINS>(b.log, b.R, b.cnt, b.votes, b.K, -1, hist);   // a frame is no keyframe: nobody is left out
}

// first slot k in [from, K) that is not bad, not marked and (parent < 0 or a child of `parent`); -1: none.  Wave-uniform.
__device__ int first_free(const LmBufs& b, int from, int parent) {
  const int lane = threadIdx.x;
  for (int base = from; base < b.K; base += 64) {
    const int k = base + lane;
    bool ok = false;
    if (k < b.K) {
      const LmKf f = b.kf[k];
      ok = !f.bad && !b.mark[k] && (parent < 0 || f.parent == parent);
    }
    const unsigned long long m = __ballot(ok);
    if (m) return base + __ffsll((long long)m) - 1;
  }
  return -1;
}

__global__ __launch_bounds__(64) void lm_build_kernel(LmBufs b) {
  const int lane = threadIdx.x;
  // keyframeCounter.empty() (:1534): the list of the previous call stays
  bool any = false;
  for (int base = 0; base < b.K && !any; base += 64) {
    const int k = base + lane;
    any = __ballot(k < b.K && b.votes[k] > 0) != 0;
  }
  int n = b.hdr->n_local_kf, n0 = 0, ref = -1;
  if (any) {
    // the voted keyframes that are not bad, by slot, and the first strictly larger vote (:1545-1562)
    int bv = 0, bk = -1;
    for (int base = 0; base < b.K; base += 64) {
      const int k = base + lane;
      const int v = k < b.K ? b.votes[k] : 0;
      const bool take = v > 0 && !b.kf[k].bad;
      const unsigned long long m = __ballot(take);
      if (take) {
        const int pos = n0 + __popcll(m & lanes_below());
        b.local_kf[pos] = k;
        b.out_votes[pos] = v;
        b.mark[k] = 1;
        if (v > bv) { bv = v; bk = k; }
      }
      n0 += __popcll(m);
    }
    for (int off = 32; off > 0; off >>= 1) {
      const int ov = __shfl_xor(bv, off), ok = __shfl_xor(bk, off);
      if (ov > bv || (ov == bv && ov > 0 && ok < bk)) { bv = ov; bk = ok; }
    }
    ref = bk;
    n = n0;
    __syncthreads();
    // the expansion (:1566-1622): every lane runs the same control flow; lane 0 writes
    int cursor = 0;
    for (int i = 0; i < n0; i++) {
      if (n > LM_MAX_LOCAL) break;
      const int pk = b.local_kf[i];
      int f = cursor < b.K ? first_free(b, cursor, -1) : -1;   // Map::GetAllKeyFrames in slot order: what precedes the hit stays bad or listed
      cursor = f < 0 ? b.K : f + 1;
      if (f >= 0) {
        if (lane == 0) { b.local_kf[n] = f; b.mark[f] = 1; }
        n++;
        __syncthreads();
      }
      f = first_free(b, 0, pk);                                 // GetChilds
      if (f >= 0) {
        if (lane == 0) { b.local_kf[n] = f; b.mark[f] = 1; }
        n++;
        __syncthreads();
      }
      const int par = b.kf[pk].parent;                          // GetParent: no isBad test, and the break leaves the outer loop
      if (par >= 0 && !b.mark[par]) {
        if (lane == 0) { b.local_kf[n] = par; b.mark[par] = 1; }
        n++;
        break;
      }
    }
    __syncthreads();
  }
  if (lane == 0) {
    b.hdr->n_voted = n0; b.hdr->n_local_kf = n; b.hdr->ref_kf = ref;
    b.out_hdr->n_voted = n0; b.out_hdr->n_local_kf = n; b.out_hdr->ref_kf = ref;
  }
  for (int i = lane; i < n; i += 64) b.out_kf[i] = b.local_kf[i];
}

__global__ __launch_bounds__(LM_BLOCK) void lm_flags_kernel(LmBufs b) {
  if ((int)blockIdx.x >= b.hdr->n_local_kf) return;
  const LmKf f = b.kf[b.local_kf[blockIdx.x]];
  for (int j = threadIdx.x; j < f.N; j += LM_BLOCK) {
    const int p = b.table[f.tab_off + j];
    if (p >= 0 && !b.bad[p]) b.flag[p] = 1;
  }
}

__global__ __launch_bounds__(64) void lm_count_kernel(LmBufs b) {
  const int first = blockIdx.x * LM_CHUNK;
  int c = 0;
  for (int j = threadIdx.x; j < LM_CHUNK; j += 64) c += first + j < b.P && b.flag[first + j];
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if (threadIdx.x == 0) b.block_cnt[blockIdx.x] = c;
}

__global__ __launch_bounds__(64) void lm_compact_kernel(LmBufs b) {
  int pre = 0;
  for (int j = threadIdx.x; j < (int)blockIdx.x; j += 64) pre += b.block_cnt[j];
  for (int off = 32; off > 0; off >>= 1) pre += __shfl_xor(pre, off);
  const int first = blockIdx.x * LM_CHUNK;
  for (int j = 0; j < LM_CHUNK; j += 64) {
    const int p = first + j + threadIdx.x;
    const bool take = p < b.P && b.flag[p];
    const unsigned long long m = __ballot(take);
    if (take) b.local_ids[pre + __popcll(m & lanes_below())] = p;
    pre += __popcll(m);
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) { b.hdr->n_local_points = pre; b.out_hdr->n_local_points = pre; }
}

__global__ __launch_bounds__(LM_BLOCK) void lm_gather_kernel(LmQueryBufs q, int Q) {
  const int i = blockIdx.x * LM_BLOCK + threadIdx.x;
  if (i >= Q) return;
  const int p = q.local_ids[i];
  q.out_ids[i] = p;
  q.qpid[i] = 0;
  for (int k = 0; k < 3; k++) {
    q.qxyz[3 * i + k] = q.xyz[3 * (size_t)p + k];
    q.qnrm[3 * i + k] = q.normal[3 * (size_t)p + k];
  }
  q.qmaxd[i] = q.max_distance[p];
  q.qdesc[2 * i] = q.desc[2 * (size_t)p];
  q.qdesc[2 * i + 1] = q.desc[2 * (size_t)p + 1];
  q.qmeta[i] = (q.bad[p] || q.cnt[p] > 0) ? 1 : 0;   // Tracking.cc:1449-1451
}

__global__ __launch_bounds__(LM_BLOCK) void lm_write_points_kernel(LmWriteBufs w, int n, int what) {
  const int i = blockIdx.x * LM_BLOCK + threadIdx.x;
  if (i >= n) return;
  const size_t p = (size_t)w.ids[i];
  if (what & DSH_MPDB_POSITION)
    for (int k = 0; k < 3; k++) w.xyz[3 * p + k] = w.src_xyz[3 * i + k];
  if (what & DSH_MPDB_NORMAL_DEPTH) {
    for (int k = 0; k < 3; k++) w.normal[3 * p + k] = w.src_normal[3 * i + k];
    w.max_distance[p] = w.src_max_distance[i];
  }
  if (what & DSH_MPDB_DESCRIPTOR) {
    w.desc[2 * p] = w.src_desc[2 * i];
    w.desc[2 * p + 1] = w.src_desc[2 * i + 1];
  }
}

__global__ __launch_bounds__(LM_BLOCK) void lm_scatter_i32_kernel(int32_t* dst, const int32_t* idx, const int32_t* val, int32_t fill, int n) {
  const int i = blockIdx.x * LM_BLOCK + threadIdx.x;
  if (i < n) dst[idx[i]] = val ? val[i] : fill;
}

}  // namespace

extern "C" hipError_t lm_update_launch(const LmBufs& b, hipStream_t st) {
  const int top = b.P > b.K ? b.P : b.K;
  hipLaunchKernelGGL(lm_clear_kernel, dim3(blocks_for(top > 0 ? top : 1, LM_BLOCK)), dim3(LM_BLOCK), 0, st, b);
  if (b.N > 0) hipLaunchKernelGGL(lm_scatter_kernel, dim3(blocks_for(b.N, LM_BLOCK)), dim3(LM_BLOCK), 0, st, b);
  // few workgroups: every workgroup flushes its touched bins once
  if (b.R > 0 && b.N > 0) hipLaunchKernelGGL(lm_votes_kernel, dim3(log_blocks(b.R, LM_BLOCK)), dim3(LM_BLOCK), 0, st, b);
  hipLaunchKernelGGL(lm_build_kernel, dim3(1), dim3(64), 0, st, b);
  if (b.K > 0 && b.P > 0) hipLaunchKernelGGL(lm_flags_kernel, dim3(b.K), dim3(LM_BLOCK), 0, st, b);
  if (b.P > 0) {
    const int nb = (b.P + LM_CHUNK - 1) / LM_CHUNK;
    hipLaunchKernelGGL(lm_count_kernel, dim3(nb), dim3(64), 0, st, b);
    hipLaunchKernelGGL(lm_compact_kernel, dim3(nb), dim3(64), 0, st, b);
  }
  return hipGetLastError();
}

extern "C" hipError_t lm_gather_launch(const LmQueryBufs& q, int Q, hipStream_t st) {
  if (Q > 0) hipLaunchKernelGGL(lm_gather_kernel, dim3(blocks_for(Q, LM_BLOCK)), dim3(LM_BLOCK), 0, st, q, Q);
  return hipGetLastError();
}

extern "C" hipError_t lm_write_points_launch(const LmWriteBufs& w, int n, int what, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(lm_write_points_kernel, dim3(blocks_for(n, LM_BLOCK)), dim3(LM_BLOCK), 0, st, w, n, what);
  return hipGetLastError();
}

extern "C" hipError_t lm_scatter_i32_launch(int32_t* dst, const int32_t* idx, const int32_t* val, int32_t fill, int n, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(lm_scatter_i32_kernel, dim3(blocks_for(n, LM_BLOCK)), dim3(LM_BLOCK), 0, st, dst, idx, val, fill, n);
  return hipGetLastError();
}
