// Tracking-side search by projection (ORBmatcher::SearchByProjection, monocular):
//   frame to frame  ORBmatcher.cc:1360-1510 (DefTracking::TrackWithMotionModel, DefTracking.cc:342-375)
//   local map       Tracking.cc:1405-1470 -> Frame::isInFrustum (Frame.cc:338-390), MapPoint::PredictScale (MapPoint.cc:422-437),
//                   ORBmatcher.cc:42-143 (DefTracking::TrackLocalMap, DefTracking.cc:234-250)
// Three launches per batch, all on the context's stream:
//   cells    one workgroup per frame: Frame::PosInGrid (Frame.cc:484-496) of every key point, counting sort into a CSR grid
//   phase A  one wavefront per query: projection (and frustum / scale test), the query's window in the grid, 256-bit Hamming
//            distances, the TRK_K smallest keys (distance, visiting order) of the candidates that are not blocked at entry
//   phase B  one wavefront per frame: the queries in the reference's order against a "taken" bitmap in LDS, decided in parallel
//            rounds that commit every query no earlier pending pick can change; a query whose surviving keys no longer decide
//            best (and second best) walks its window again
// The reference visits column ix, then row iy, then a cell's index order and keeps the first strictly better candidate, so its
// best / second best are the two smallest keys (distance, cell = ix * rows + iy, index).
// dsh_motion_model_search runs phases A and B twice on one grid (trk_launch_search): its queries are compacted on the device (qcount),
// a query without observations does not block the key point it takes (qfree), and the second, wider pass is gated on the first
// pass's count (gate).  All three are null for the other callers.
// Compiled without FMA contraction: the reference's float32 expression order is kept (see include/defslam_hip.h).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "track_frustum.h"
#include "track_problem.h"

namespace {

__device__ __forceinline__ int kdist(unsigned long long k) { return (int)(k >> 40); }
__device__ __forceinline__ int kidx(unsigned long long k) { return (int)((k >> 8) & 0xFFFF); }
__device__ __forceinline__ int klevel(unsigned long long k) { return (int)(k & 0x7F); }
__device__ __forceinline__ bool kstate2(unsigned long long k) { return (k & 0x80) != 0; }

// Frame::GetFeaturesInArea (Frame.cc:421-480): the grid cells of the window, false when it is empty
__device__ __forceinline__ bool window_cells(const TrkProb& P, float u, float v, float r, int& c0, int& c1, int& r0, int& r1) {
  c0 = max(0, (int)floorf((u - P.minX - r) * P.winv));
  if (c0 >= P.cols) return false;
  c1 = min(P.cols - 1, (int)ceilf((u - P.minX + r) * P.winv));
  if (c1 < 0) return false;
  r0 = max(0, (int)floorf((v - P.minY - r) * P.hinv));
  if (r0 >= P.rows) return false;
  r1 = min(P.rows - 1, (int)ceilf((v - P.minY + r) * P.hinv));
  if (r1 < 0) return false;
  return true;
}

// the KK smallest keys of the query's window over the wavefront: candidates with octave in [lmin, lmax] strictly inside the
// window, not blocked at entry (state 1) and, in phase B, not taken.  Every lane returns the same sorted keys; *n = candidates.
template <int KK>
__device__ void scan_window(const TrkBufs& b, const TrkProb& P, float u, float v, float r, int lmin, int lmax, const uint4 qd0, const uint4 qd1,
                            const uint32_t* taken, int lane, unsigned long long* out, int* n_out) {
  unsigned long long top[KK];
#pragma unroll
  for (int k = 0; k < KK; k++) top[k] = TRK_NO_KEY;
  int n = 0;
  int c0, c1, r0, r1;
  if (window_cells(P, u, v, r, c0, c1, r0, r1)) {
    const int32_t* cs = b.cell_start + P.cell_off;
    for (int ix = c0; ix <= c1; ix++) {
      const int s = cs[ix * P.rows + r0], e = cs[ix * P.rows + r1 + 1];   // the column's cells r0..r1 are contiguous
      for (int pos = s + lane; pos < e; pos += 64) {
        const int g = P.kp_off + pos;
        const int meta = b.smeta[g];
        const int oct = (meta >> 16) & 0xFF, st = meta >> 24, j = meta & 0xFFFF;
        if (oct < lmin || oct > lmax) continue;
        const float2 kp = b.skp[g];
        const float dx = kp.x - u, dy = kp.y - v;
        if (!(fabsf(dx) < r && fabsf(dy) < r)) continue;
        if (st == 1) continue;
        if (taken && ((taken[j >> 5] >> (j & 31)) & 1u)) continue;
        n++;
        const uint4 d0 = b.sdesc[2 * (size_t)g], d1 = b.sdesc[2 * (size_t)g + 1];
        const int dist = __popc(d0.x ^ qd0.x) + __popc(d0.y ^ qd0.y) + __popc(d0.z ^ qd0.z) + __popc(d0.w ^ qd0.w) + __popc(d1.x ^ qd1.x) +
                         __popc(d1.y ^ qd1.y) + __popc(d1.z ^ qd1.z) + __popc(d1.w ^ qd1.w);
        const int cell = (int)roundf((kp.x - P.minX) * P.winv) * P.rows + (int)roundf((kp.y - P.minY) * P.hinv);
        unsigned long long key = ((unsigned long long)dist << 40) | ((unsigned long long)cell << 24) | ((unsigned long long)j << 8) |
                                 (st == 2 ? 0x80ull : 0ull) | (unsigned long long)oct;
        // sorted insert (keys are distinct: (cell, index) is unique)
#pragma unroll
        for (int k = 0; k < KK; k++) {
          const unsigned long long lo = key < top[k] ? key : top[k], hi = key < top[k] ? top[k] : key;
          top[k] = lo;
          key = hi;
        }
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  // KK rounds of a wave-wide minimum of the lanes' heads; the owner pops it
#pragma unroll
  for (int k = 0; k < KK; k++) {
    unsigned long long m = top[0];
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(m, o, 64);
      m = other < m ? other : m;
    }
    if (m != TRK_NO_KEY && top[0] == m) {
#pragma unroll
      for (int i = 0; i + 1 < KK; i++) top[i] = top[i + 1];
      top[KK - 1] = TRK_NO_KEY;
    }
    out[k] = m;
  }
  *n_out = n;
}

// Frame::PosInGrid of every key point, counting sort into the CSR grid of its frame
__global__ __launch_bounds__(1024) void trk_cells_kernel(TrkBufs b) {
  __shared__ int cnt[TRK_MAX_CELLS];
  __shared__ int part[1024];
  const TrkProb& P = b.prob[blockIdx.x];
  const int t = threadIdx.x, N = P.N, ncell = P.cols * P.rows, kp_off = P.kp_off;
  for (int c = t; c < ncell; c += 1024) cnt[c] = 0;
  __syncthreads();
  int mycell[TRK_MAX_KEYPOINTS / 1024], myslot[TRK_MAX_KEYPOINTS / 1024];
#pragma unroll
  for (int k = 0; k < TRK_MAX_KEYPOINTS / 1024; k++) {
    const int j = t + 1024 * k;
    int cell = -1, slot = 0;
    if (j < N) {
      const float2 kp = b.kp[kp_off + j];
      const int px = (int)roundf((kp.x - P.minX) * P.winv), py = (int)roundf((kp.y - P.minY) * P.hinv);
      if (!(px < 0 || px >= P.cols || py < 0 || py >= P.rows)) {
        cell = px * P.rows + py;
        slot = atomicAdd(&cnt[cell], 1);
      }
    }
    mycell[k] = cell;
    myslot[k] = slot;
  }
  __syncthreads();
  // exclusive scan of the counts: 8 cells per thread, then the 1024 partial sums
  int loc[TRK_MAX_CELLS / 1024], s = 0;
#pragma unroll
  for (int k = 0; k < TRK_MAX_CELLS / 1024; k++) {
    const int c = t * (TRK_MAX_CELLS / 1024) + k;
    loc[k] = s;
    s += c < ncell ? cnt[c] : 0;
  }
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int add = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  const int base = part[t] - s;
  int32_t* cs = b.cell_start + P.cell_off;
#pragma unroll
  for (int k = 0; k < TRK_MAX_CELLS / 1024; k++) {
    const int c = t * (TRK_MAX_CELLS / 1024) + k;
    if (c < ncell) {
      cnt[c] = base + loc[k];
      cs[c] = base + loc[k];
    }
  }
  if (t == 1023) cs[ncell] = part[1023];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < TRK_MAX_KEYPOINTS / 1024; k++) {
    if (mycell[k] < 0) continue;
    const int j = t + 1024 * k;
    const int g = kp_off + cnt[mycell[k]] + myslot[k];
    const int km = b.kmeta[kp_off + j];
    b.skp[g] = b.kp[kp_off + j];
    b.smeta[g] = j | ((km & 0xFF) << 16) | (((km >> 8) & 0xFF) << 24);
    b.sdesc[2 * (size_t)g] = b.kdesc[2 * (size_t)(kp_off + j)];
    b.sdesc[2 * (size_t)g + 1] = b.kdesc[2 * (size_t)(kp_off + j) + 1];
  }
}

// phase A: one wavefront per query
__global__ __launch_bounds__(256) void trk_search_kernel(TrkBufs b, int Qt) {
  if (b.gate && b.gate[0] >= b.gate_min) return;
  const int gq = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (gq >= Qt || (b.qcount && gq >= b.qcount[0])) return;
  const TrkProb& P = b.prob[b.qpid[gq]];
  const float x = b.qxyz[3 * (size_t)gq], y = b.qxyz[3 * (size_t)gq + 1], z = b.qxyz[3 * (size_t)gq + 2];
  const int meta = b.qmeta[gq];
  bool live = true;
  float u = 0.f, v = 0.f, r = 0.f, vc = 0.f;
  int lmin = 0, lmax = 0, level = 0;
  if (P.mode == 0) {
    // ORBmatcher.cc:1389-1411: invzc = 1.0 / z in double, stored as float; radius = th * mvScaleFactors[nLastOctave]
    const float xc = trk_cam_coord(P, 0, x, y, z), yc = trk_cam_coord(P, 1, x, y, z), zc = trk_cam_coord(P, 2, x, y, z);
    const float invzc = (float)(1.0 / (double)zc);
    if (invzc < 0) live = false;
    u = P.fx * xc * invzc + P.cx;
    v = P.fy * yc * invzc + P.cy;
    if (u < P.minX || u > P.maxX) live = false;
    if (v < P.minY || v > P.maxY) live = false;
    r = P.th * P.sf[meta];
    lmin = meta - 1;
    lmax = meta + 1;
  } else {
    // Frame::isInFrustum(pMP, 0.5) (track_frustum.h), MapPoint::PredictScale (MapPoint.cc:422-437)
    TrkView w;
    live = trk_in_frustum(P, x, y, z, b.qnrm[3 * (size_t)gq], b.qnrm[3 * (size_t)gq + 1], b.qnrm[3 * (size_t)gq + 2], w);
    if (meta) live = false;
    u = w.u; v = w.v; vc = w.vc;
    const float dist = w.dist;
    const float ratio = b.qmaxd[gq] / dist;
    level = (int)ceil(log((double)ratio) / (double)P.logsf);
    if (level < 0) level = 0;
    else if (level >= P.levels) level = P.levels - 1;
    r = vc > 0.998 ? 2.5f : 4.0f;   // ORBmatcher::RadiusByViewingCos
    if (P.th != 1.0f) r *= P.th;
    r = r * P.sf[level];
    lmin = level - 1;
    lmax = level;
  }
  if (u != u || v != v) live = false;   // a point on the camera plane: the reference's window arithmetic is undefined there
  unsigned long long keys[TRK_K];
  int n = 0;
  if (live) {
    const uint4 qd0 = b.qdesc[2 * (size_t)gq], qd1 = b.qdesc[2 * (size_t)gq + 1];
    scan_window<TRK_K>(b, P, u, v, r, lmin, lmax, qd0, qd1, nullptr, lane, keys, &n);
  } else {
#pragma unroll
    for (int k = 0; k < TRK_K; k++) keys[k] = TRK_NO_KEY;
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < TRK_K; k++) b.keys[(size_t)gq * TRK_K + k] = keys[k];
    b.ncand[gq] = n;
    TrkWin w;
    w.u = u; w.v = v; w.r = r; w.lmin = lmin; w.lmax = lmax; w.pad[0] = w.pad[1] = w.pad[2] = 0;
    b.win[gq] = w;
    if (P.mode == 1) {
      b.inview[gq] = live ? 1 : 0;
      b.level[gq] = live ? level : 0;
      b.uv[2 * (size_t)gq] = live ? u : 0.f;
      b.uv[2 * (size_t)gq + 1] = live ? v : 0.f;
      b.vcos[gq] = live ? vc : 0.f;
    }
    if (n > TRK_MAX_CANDIDATES) atomicOr(&b.pstat[4 * (b.qpid[gq]) + 2], 1);
  }
}

// ORBmatcher.cc:1460-1463 (frame to frame) and :122-133 (local map) on the two smallest surviving keys
__device__ __forceinline__ int accept(unsigned long long s1, unsigned long long s2, bool local) {
  if (s1 == TRK_NO_KEY || kdist(s1) > TRK_TH_HIGH) return -1;
  if (!local) return kstate2(s1) ? -1 : kidx(s1);   // ORBmatcher.cc:1462: the best key point already has a map point
  const int d1 = kdist(s1), lev1 = klevel(s1);
  const int d2 = s2 != TRK_NO_KEY ? kdist(s2) : 256, lev2 = s2 != TRK_NO_KEY ? klevel(s2) : -1;
  return (lev1 == lev2 && (float)d1 > 0.8f * (float)d2) ? -1 : kidx(s1);   // mfNNratio = 0.8f
}

// A query's match from its stored keys and the taken bits: *rescan when the stored keys no longer decide it; *nexam = how many
// of its stored keys the decision read (a key point taken later that is not among them cannot change it).
__device__ __forceinline__ int decide(const unsigned long long (&a)[TRK_K], int n, const uint32_t* taken, bool local, bool* rescan, int* nexam) {
  const int stored = n < TRK_K ? n : TRK_K, need = local ? 2 : 1;
  uint32_t tw[TRK_K];
#pragma unroll
  for (int k = 0; k < TRK_K; k++) tw[k] = taken[(k < stored ? kidx(a[k]) : 0) >> 5];   // independent LDS reads
  unsigned long long s1 = TRK_NO_KEY, s2 = TRK_NO_KEY;
  int found = 0, last = stored;
#pragma unroll
  for (int k = 0; k < TRK_K; k++) {
    if (k >= stored || found >= need || ((tw[k] >> (kidx(a[k]) & 31)) & 1u)) continue;
    if (found == 0) s1 = a[k];
    else s2 = a[k];
    if (++found == need) last = k + 1;
  }
  *nexam = last;
  *rescan = false;
  if (found < need && n > TRK_K) {
    // the unstored candidates all have keys above a[TRK_K - 1]: they matter only if they can still be accepted
    const int dref = found ? kdist(s1) : kdist(a[TRK_K - 1]);
    if (dref <= TRK_TH_HIGH) {
      *rescan = true;
      return -1;
    }
    return -1;
  }
  return accept(s1, s2, local);
}

// phase B: one wavefront per frame resolves its queries in the reference's order, 64 at a time (lane i: query base + i).  A round
// decides every pending query in parallel from the taken bits; the queries in front of the first one whose decision read a key
// point an earlier pending query picks (or that needs its window again) are exact and are committed; the round repeats from there.
// A query that needs a re-scan walks its window with the whole wavefront when it is the first pending one.
// The block is exactly ONE wavefront (launched with 64 threads, trk_launch): the owner / taken protocol reads LDS words other lanes of
// the same wave just wrote, which relies on the DS operations of one wave completing in program order; the wavefront-scope fences
// below keep the compiler from moving the LDS accesses across the protocol's steps.  A larger block would need __syncthreads there.
__global__ __launch_bounds__(64) void trk_resolve_kernel(TrkBufs b) {
  __shared__ uint32_t taken[TRK_MAX_KEYPOINTS / 32];
  __shared__ uint32_t owner[TRK_MAX_KEYPOINTS];   // lowest pending lane of the round that picks the key point, 64 = none
  if (b.gate && b.gate[0] >= b.gate_min) return;
  const TrkProb& P = b.prob[blockIdx.x];
  const int lane = threadIdx.x, Q = b.qcount ? min(P.Q, b.qcount[0]) : P.Q, q_off = P.q_off;
  const bool local = P.mode == 1;
  for (int i = lane; i < TRK_MAX_KEYPOINTS / 32; i += 64) taken[i] = 0;
  for (int i = lane; i < TRK_MAX_KEYPOINTS; i += 64) owner[i] = 64;
  __syncthreads();
  if (b.pstat[4 * blockIdx.x + 2]) return;   // a window over TRK_MAX_CANDIDATES: the call fails with DSH_ERR_ARG, nothing to resolve
  int nm = 0, nres = 0;
  for (int base = 0; base < Q; base += 64) {
    unsigned long long lk[TRK_K];
    int lnc = 0;
    const int mq = base + lane;
#pragma unroll
    for (int k = 0; k < TRK_K; k++) lk[k] = mq < Q ? b.keys[(size_t)(q_off + mq) * TRK_K + k] : TRK_NO_KEY;
    if (mq < Q) lnc = b.ncand[q_off + mq];
    // DefORBmatcher.cc:381-383: a pick blocks its key point only when the query's point has observations
    const bool blocks = !(b.qfree && mq < Q && b.qfree[q_off + mq]);
    const int cnt = min(64, Q - base);
    int myres = -1;
    int start = 0;
    while (start < cnt) {
      const bool pending = lane >= start && lane < cnt;
      bool rescan = false;
      int nexam = 0, res = -1;
      if (pending && lnc > 0) res = decide(lk, lnc, taken, local, &rescan, &nexam);
      if (res >= 0 && blocks) atomicMin(&owner[res], (uint32_t)lane);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      bool dirty = pending && rescan;
#pragma unroll
      for (int k = 0; k < TRK_K; k++)
        if (k < nexam && owner[kidx(lk[k])] < (uint32_t)lane) dirty = true;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (res >= 0 && blocks) owner[res] = 64;
      const unsigned long long dm = __ballot(dirty);
      const int f = dm ? (int)__ffsll((long long)dm) - 1 : cnt;
      if (f > start) {
        const bool commit = pending && lane < f;
        if (commit) myres = res;
        if (commit && res >= 0 && blocks) atomicOr(&taken[res >> 5], 1u << (res & 31));
        nm += __popcll(__ballot(commit && res >= 0));
        start = f;
      } else {
        // the first pending query needs its window again: all lanes walk it with the current taken bits
        const int gq = q_off + base + start;
        const TrkWin w = b.win[gq];
        const uint4 qd0 = b.qdesc[2 * (size_t)gq], qd1 = b.qdesc[2 * (size_t)gq + 1];
        unsigned long long t2[2];
        int n2;
        scan_window<2>(b, P, w.u, w.v, w.r, w.lmin, w.lmax, qd0, qd1, taken, lane, t2, &n2);
        const int r = accept(t2[0], t2[1], local);
        const int sblocks = __shfl((int)blocks, start, 64);
        if (lane == start) myres = r;
        if (r >= 0) {
          if (lane == 0 && sblocks) atomicOr(&taken[r >> 5], 1u << (r & 31));
          nm++;
        }
        nres++;
        start++;
      }
    }
    if (mq < Q) b.match[q_off + mq] = myres;
  }
  if (lane == 0) {
    b.pstat[4 * blockIdx.x] = nm;
    b.pstat[4 * blockIdx.x + 1] = nres;
    if (b.gate) b.pstat[4 * blockIdx.x + 3] = 1;
  }
}

}  // namespace

extern "C" hipError_t trk_launch(const TrkBufs& b, int B, int Qt, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(trk_cells_kernel, dim3(B), dim3(1024), 0, st, b);
  return trk_launch_search(b, B, Qt, st);
}

extern "C" hipError_t trk_launch_search(const TrkBufs& b, int B, int Qt, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (Qt > 0) hipLaunchKernelGGL(trk_search_kernel, dim3((Qt + 3) / 4), dim3(256), 0, st, b, Qt);
  hipLaunchKernelGGL(trk_resolve_kernel, dim3(B), dim3(64), 0, st, b);
  return hipGetLastError();
}
