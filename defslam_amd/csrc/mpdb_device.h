// What the kernel files of the map point store dsh_mpdb share (localmap_, trackclose_, tmplswitch_, motionmodel_, anchor_, kfinsert_,
// pointerase_, obslist_ and tracksft_kernels.hip): the wavefront and workgroup idioms of counting, appending and ordered compaction, and the grid
// sizes of the launchers.  Integer valued; wavefronts of 64 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ unsigned long long lanes_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }

// *ctr += the lanes of the wavefront with `flag`; every lane of the wavefront calls it
__device__ __forceinline__ void wave_count(bool flag, int32_t* ctr) {
  const unsigned long long m = __ballot(flag);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(ctr, __popcll(m));
}

// Append with one atomic per wavefront: the place of this lane's element behind *ctr, which moves past the wavefront's taken lanes.
// Every lane of the wavefront calls it; the places are in lane order within the wavefront, the wavefronts in any order.
__device__ __forceinline__ int wave_append(bool take, int32_t* ctr) {
  const unsigned long long m = __ballot(take);
  int base = 0;
  if ((threadIdx.x & 63) == 0 && m) base = atomicAdd(ctr, __popcll(m));
  return __shfl(base, 0, 64) + __popcll(m & lanes_below());
}

// The rank of this thread's element among the taken ones of the workgroup's tile of BLOCK elements, and the tile's total: a ballot per
// wavefront, the wavefronts' totals through wsum[BLOCK / 64] in LDS.  Every thread of the workgroup calls it (it holds two barriers; the
// first lets the previous tile's totals be read, and orders what the caller stored in LDS before the call).
template <int BLOCK>
__device__ __forceinline__ int tile_rank(bool take, int* wsum, int& total) {
  const int wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(take);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) wsum[wave] = __popcll(m);
  __syncthreads();
  int pos = __popcll(m & lanes_below());
  total = 0;
#pragma unroll
  for (int w = 0; w < BLOCK / 64; w++) {
    if (w < wave) pos += wsum[w];
    total += wsum[w];
  }
  return pos;
}

// ordered compaction over consecutive tiles: the position of this thread's element behind `base`; base moves past the tile
template <int BLOCK>
__device__ __forceinline__ int ordered_slot(bool take, int& base, int* wsum) {
  int total;
  const int pos = base + tile_rank<BLOCK>(take, wsum, total);
  base += total;
  return pos;
}

// flags[c] of every thread of the workgroup counted: thread c < NC returns the count of flags[c], the others 0.  Every thread of the
// workgroup calls it (it holds a barrier).
template <int BLOCK, int NC>
__device__ __forceinline__ int block_sums(const bool (&flags)[NC]) {
  __shared__ int part[BLOCK / 64][NC];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < NC; c++) {
    const int n = __popcll(__ballot(flags[c]));
    if (lane == 0) part[wave][c] = n;
  }
  __syncthreads();
  int s = 0;
  if (threadIdx.x < NC) {
#pragma unroll
    for (int w = 0; w < BLOCK / 64; w++) s += part[w][threadIdx.x];
  }
  return s;
}

// The vote of a list of point ids on the keyframes that observe them, as Tracking::UpdateLocalKeyFrames (Tracking.cc:1519-1532) casts it
// for a frame and KeyFrame::UpdateConnections (KeyFrame.cc:335-357) for a keyframe's own table: first the list's multiplicities, then
// one coalesced pass over the observation log.
// vote_scatter: entry p of the list into cnt[p]; a bad point does not vote and is reported.
__device__ __forceinline__ bool vote_scatter(const int32_t* bad, int32_t* cnt, int p) {
  if (p < 0) return false;
  if (bad[p]) return true;
  atomicAdd(&cnt[p], 1);
  return false;
}

// vote_sweep: votes[k] += cnt[point] for every live record (point, k) with k != skip.  The votes accumulate in hist[BINS] in LDS and
// leave with one global atomic per workgroup and touched keyframe (the records of a map concentrate on few keyframes: an atomic per
// record would serialise on them); more than BINS keyframes take more passes over the log.  Every thread of the workgroup calls it.
template <int BLOCK, int BINS>
__device__ __forceinline__ void vote_sweep(const int2* log, long long R, const int32_t* cnt, int32_t* votes, int K, int skip, int* hist) {
  for (int base = 0; base < K; base += BINS) {
    const int bins = min(BINS, K - base);
    for (int k = threadIdx.x; k < bins; k += BLOCK) hist[k] = 0;
    __syncthreads();
    for (long long r = (long long)blockIdx.x * BLOCK + threadIdx.x; r < R; r += (long long)gridDim.x * BLOCK) {
      const int2 rec = log[r];
      if (rec.x < 0 || rec.y == skip) continue;   // erased; the voter itself
      const int w = cnt[rec.x];
      const int k = rec.y - base;
      if (w > 0 && k >= 0 && k < bins) atomicAdd(&hist[k], w);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < bins; k += BLOCK) {
      const int v = hist[k];
      if (v) atomicAdd(&votes[base + k], v);
    }
    __syncthreads();
  }
}

// workgroups of `block` threads, one element per thread
inline int blocks_for(long long n, int block) { return (int)((n + block - 1) / block); }

// a grid-stride pass over a log of R records: eight records per thread, at most 1024 workgroups, at least one
inline int log_blocks(long long R, int block) {
  const long long g = (R + 8 * block - 1) / (8 * block);
  return (int)(g > 1024 ? 1024 : g < 1 ? 1 : g);
}
