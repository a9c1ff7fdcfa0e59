// What SchwarpDatabase::add reads of the map before its first fit, on the resident map point store (dsh_keyframe_anchors; gfx950).
//   the count per reference keyframe, the matched indices per anchor   Modules/Mapping/SchwarpDatabase.cc:61-80, :83-106
//   the query list of DefORBmatcher::searchBySchwarp                   Modules/Matching/DefORBmatcher.cc:200-211
// The log is an unsorted append-only stream, so "does point p observe keyframe a, and at which key point" is answered by passes over
// the log (as lm_votes_kernel does), not by per-point lists.  The launches of a call, no host read between them, every value an integer:
//   an_clear_kernel    the per-call arrays
//   an_mark_kernel     the new keyframe's table: first_i[p] and mult[p] of every held point that is not bad, the vote for its reference
//                      keyframe (or n_no_ref), has[j]
//   an_idx2_kernel     first pass over the log: idx2_of[p] of the live records of the new keyframe
//   an_rank_kernel     ONE wavefront: the voted keyframes in slot order by ballot (lm_build_kernel's pattern)
//   an_pairs_kernel    second pass over the log: a live record (p, a) of a marked point that observes the new keyframe counts mult[p]
//                      pairs for anchor a and puts its key point index into matrix[rank a][first_i[p]].  The mirror refuses a pair that
//                      is stored already, so every cell has one writer and the count is a sum of integers: no order enters
//   an_queries_kernel  a workgroup per anchor counts the queries of the anchor's table
//   an_scan_kernel     ONE wavefront: min_pairs, the CSR offsets of pairs and queries, the counters
//   an_write_kernel    a workgroup per anchor: ordered compaction of its matrix row into the pairs and of its table into the queries
// When max_anchors x N cells exceed the matrix the host allows, the anchors are taken `chunk` at a time: the matrix is cleared, filled by
// one more pass over the log and written, per chunk; counts and offsets are complete before the first write, so the result does not
// depend on the chunking.  Lists are written as far as the caller's capacities reach; the counters always come down in full.
// Where the reference iterates an unordered_map<KeyFrame*, int> the order here is the index: anchors by ascending slot.
#include <hip/hip_runtime.h>

#include "anchor_problem.h"
#include "mpdb_device.h"

namespace {

__global__ __launch_bounds__(AN_BLOCK) void an_clear_kernel(AnBufs b) {
  const int i = blockIdx.x * AN_BLOCK + threadIdx.x;
  if (i < b.P) { b.first_i[i] = AN_UNMARKED; b.mult[i] = 0; b.idx2_of[i] = -1; }
  if (i < b.K) { b.votes[i] = 0; b.rank[i] = -1; }
  if (i < b.max_anchors) { b.a_pairs[i] = 0; b.a_queries[i] = 0; }
  if (i == 0) { b.hdr->n_anchors = 0; b.hdr->n_pairs = 0; b.hdr->n_queries = 0; b.hdr->n_no_ref = 0; }
}

__global__ __launch_bounds__(AN_BLOCK) void an_mark_kernel(AnBufs b) {
  const int i = blockIdx.x * AN_BLOCK + threadIdx.x;
  if (i >= b.N) return;
  const int p = b.table[b.tab_off + i];
  b.out_has[i] = p != -1 ? 1 : 0;
  if (p < 0 || b.bad[p]) return;            // SchwarpDatabase.cc:71-74, :92-95
  atomicMin(&b.first_i[p], i);
  atomicAdd(&b.mult[p], 1);
  const int r = b.ref_kf[p];                // :76-79, once per entry that holds the point
  if (r < 0) atomicAdd(&b.hdr->n_no_ref, 1);
  else atomicAdd(&b.votes[r], 1);
}

__global__ __launch_bounds__(AN_BLOCK) void an_idx2_kernel(AnBufs b) {
  for (long long r = (long long)blockIdx.x * AN_BLOCK + threadIdx.x; r < b.R; r += (long long)gridDim.x * AN_BLOCK) {
    const int2 rec = b.log[r];
    if (rec.x >= 0 && rec.y == b.slot) b.idx2_of[rec.x] = b.log_idx[r];
  }
}

__global__ __launch_bounds__(64) void an_rank_kernel(AnBufs b) {
  const int lane = threadIdx.x;
  int n = 0;
  for (int base = 0; base < b.K; base += 64) {
    const int k = base + lane;
    const int v = k < b.K ? b.votes[k] : 0;
    const bool take = v > 0;
    const unsigned long long m = __ballot(take);
    if (take) {
      const int pos = n + __popcll(m & lanes_below());   // pos < max_anchors: every anchor has a vote of an entry, and is a keyframe
      b.rank[k] = pos;
      b.a_slot[pos] = k;
      if (pos < b.cap_anchors) { b.out_slot[pos] = k; b.out_count[pos] = v; }
    }
    n += __popcll(m);
  }
  if (lane == 0) b.hdr->n_anchors = n;
}

// count: the first pass counts the pairs of every anchor; every pass fills the matrix rows of the anchors c0 .. c0 + chunk - 1
__global__ __launch_bounds__(AN_BLOCK) void an_pairs_kernel(AnBufs b, int c0, int count) {
  for (long long r = (long long)blockIdx.x * AN_BLOCK + threadIdx.x; r < b.R; r += (long long)gridDim.x * AN_BLOCK) {
    const int2 rec = b.log[r];
    if (rec.x < 0) continue;   // erased
    const int a = b.rank[rec.y];
    if (a < 0) continue;
    const int fi = b.first_i[rec.x];
    if (fi == AN_UNMARKED || b.idx2_of[rec.x] < 0) continue;   // :97: the point is in both keyframes
    if (count) atomicAdd(&b.a_pairs[a], b.mult[rec.x]);
    if (a >= c0 && a < c0 + b.chunk) b.matrix[(size_t)(a - c0) * b.N + fi] = b.log_idx[r];
  }
}

// DefORBmatcher.cc:203-209: the entry holds a point that is not bad and is not in the new keyframe
__device__ __forceinline__ bool is_query(const AnBufs& b, int p) { return p >= 0 && !b.bad[p] && b.idx2_of[p] < 0; }

__global__ __launch_bounds__(AN_BLOCK) void an_queries_kernel(AnBufs b) {
  __shared__ int part[AN_BLOCK / 64];
  const int a = blockIdx.x;
  if (a >= b.hdr->n_anchors) return;
  const LmKf f = b.kf[b.a_slot[a]];
  int n = 0;
  for (int j = threadIdx.x; j < f.N; j += AN_BLOCK) n += is_query(b, b.table[f.tab_off + j]) ? 1 : 0;
  for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < AN_BLOCK / 64; w++) t += part[w];
    b.a_queries[a] = t;
  }
}

__global__ __launch_bounds__(64) void an_scan_kernel(AnBufs b) {
  const int lane = threadIdx.x, A = b.hdr->n_anchors;
  int np_run = 0, nq_run = 0;
  for (int base = 0; base < A; base += 64) {
    const int a = base + lane;
    const int np = a < A ? b.a_pairs[a] : 0;
    const bool fit = a < A && np >= b.min_pairs;   // :105-106
    int sp = fit ? np : 0, sq = fit ? b.a_queries[a] : 0;
    for (int off = 1; off < 64; off <<= 1) {       // inclusive scan of the wavefront
      const int tp = __shfl_up(sp, off, 64), tq = __shfl_up(sq, off, 64);
      if (lane >= off) { sp += tp; sq += tq; }
    }
    if (a < A) {
      b.pptr[a + 1] = np_run + sp;
      b.qptr[a + 1] = nq_run + sq;
      if (a < b.cap_anchors) {
        b.out_npairs[a] = np;
        b.out_pptr[a + 1] = np_run + sp;
        b.out_qptr[a + 1] = nq_run + sq;
      }
    }
    np_run += __shfl(sp, 63, 64);
    nq_run += __shfl(sq, 63, 64);
  }
  if (lane == 0) {
    b.pptr[0] = 0;
    b.qptr[0] = 0;
    b.out_pptr[0] = 0;
    b.out_qptr[0] = 0;
    AnHdr h = *b.hdr;
    h.n_pairs = np_run;
    h.n_queries = nq_run;
    *b.hdr = h;
    *b.out_hdr = h;
  }
}

__global__ __launch_bounds__(AN_BLOCK) void an_write_kernel(AnBufs b, int c0) {
  __shared__ int wsum[AN_BLOCK / 64];
  const int a = c0 + blockIdx.x;
  if (a >= b.hdr->n_anchors || b.a_pairs[a] < b.min_pairs) return;   // workgroup-uniform
  const int aslot = b.a_slot[a];
  const int32_t* row = b.matrix + (size_t)blockIdx.x * b.N;
  // :89-104: for i ascending, the entries whose point is in both keyframes
  int base = b.pptr[a];
  for (int t0 = 0; t0 < b.N; t0 += AN_BLOCK) {
    const int i = t0 + threadIdx.x;
    int p = -1, idx1 = -1, idx2 = -1;
    if (i < b.N) {
      p = b.table[b.tab_off + i];
      if (p >= 0 && !b.bad[p]) {
        idx2 = b.idx2_of[p];
        idx1 = row[b.first_i[p]];
      }
    }
    const bool take = idx1 >= 0 && idx2 >= 0;
    const int pos = ordered_slot<AN_BLOCK>(take, base, wsum);
    if (take && pos < b.cap_pairs) {
      b.out_idx1[pos] = idx1;
      b.out_idx2[pos] = idx2;
      b.out_point[pos] = p;
      b.out_own[pos] = b.ref_kf[p] == aslot ? 1 : 0;   // :296-298: only these are stored after the fit
    }
  }
  // DefORBmatcher.cc:201-212: for j ascending over the anchor's table
  const LmKf f = b.kf[aslot];
  base = b.qptr[a];
  for (int t0 = 0; t0 < f.N; t0 += AN_BLOCK) {
    const int j = t0 + threadIdx.x;
    const int p = j < f.N ? b.table[f.tab_off + j] : -1;
    const bool take = is_query(b, p);
    const int pos = ordered_slot<AN_BLOCK>(take, base, wsum);
    if (take && pos < b.cap_queries) {
      b.out_qidx1[pos] = j;
      b.out_qpoint[pos] = p;
    }
  }
}

__global__ __launch_bounds__(AN_BLOCK) void an_gather_i32_kernel(const int32_t* src, const int32_t* ids, int n, int32_t* out) {
  const int i = blockIdx.x * AN_BLOCK + threadIdx.x;
  if (i < n) out[i] = src[ids[i]];
}

}  // namespace

extern "C" hipError_t an_anchors_launch(const AnBufs& b, hipStream_t st) {
  const int top = b.P > b.K ? b.P : b.K;
  hipLaunchKernelGGL(an_clear_kernel, dim3(blocks_for(top > b.max_anchors ? top : b.max_anchors, AN_BLOCK)), dim3(AN_BLOCK), 0, st, b);
  if (b.N > 0) hipLaunchKernelGGL(an_mark_kernel, dim3(blocks_for(b.N, AN_BLOCK)), dim3(AN_BLOCK), 0, st, b);
  if (b.R > 0) hipLaunchKernelGGL(an_idx2_kernel, dim3(log_blocks(b.R, AN_BLOCK)), dim3(AN_BLOCK), 0, st, b);
  hipLaunchKernelGGL(an_rank_kernel, dim3(1), dim3(64), 0, st, b);
  for (int c0 = 0; c0 < b.max_anchors; c0 += b.chunk) {
    const int rows = b.max_anchors - c0 < b.chunk ? b.max_anchors - c0 : b.chunk;
    const hipError_t e = hipMemsetAsync(b.matrix, 0xff, 4 * (size_t)rows * b.N, st);   // -1: the point does not observe the anchor
    if (e != hipSuccess) return e;
    if (b.R > 0) hipLaunchKernelGGL(an_pairs_kernel, dim3(log_blocks(b.R, AN_BLOCK)), dim3(AN_BLOCK), 0, st, b, c0, c0 == 0 ? 1 : 0);
    if (c0 == 0) {
      hipLaunchKernelGGL(an_queries_kernel, dim3(b.max_anchors), dim3(AN_BLOCK), 0, st, b);
      hipLaunchKernelGGL(an_scan_kernel, dim3(1), dim3(64), 0, st, b);
    }
    hipLaunchKernelGGL(an_write_kernel, dim3(rows), dim3(AN_BLOCK), 0, st, b, c0);
  }
  if (b.max_anchors == 0) hipLaunchKernelGGL(an_scan_kernel, dim3(1), dim3(64), 0, st, b);   // no anchors: the counters and two zero offsets
  return hipGetLastError();
}

extern "C" hipError_t an_gather_i32_launch(const int32_t* src, const int32_t* ids, int n, int32_t* out, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(an_gather_i32_kernel, dim3(blocks_for(n, AN_BLOCK)), dim3(AN_BLOCK), 0, st, src, ids, n, out);
  return hipGetLastError();
}
