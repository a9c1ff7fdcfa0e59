// The map point upkeep on the resident stores (dsh_keyframe_process_new, dsh_point_store_upkeep; gfx950): MapPoint::AddObservation,
// UpdateNormalAndDepth and ComputeDistinctiveDescriptors (LocalMapping.cc:142-165, DefMapPoint.cc:122-126) with the observation lists
// read from dsh_mpdb's log and the keyframes from dsh_kfdb, results written into the point store.  The log is an unsorted append-only
// stream, so the lists of the selected points are built by passes over it (as anchor_kernels.hip does).  The launches of a call, no host
// read between them; every count the later launches need stays in KiHdr on the device:
//   ki_clear_kernel      the per-call arrays and counters
//   selection            dsh_keyframe_process_new: ki_first_kernel (the lowest entry that holds each point), ki_observes_kernel (first pass
//                        over the log: who observes the keyframe already) and ki_classify_kernel, ONE workgroup that walks the table in
//                        order: the action per entry, and for action 2 the record appended to the log at R + position, nObs++ and the
//                        point's place in the selection (ordered compaction)
//                        dsh_point_store_upkeep: ki_select_ids_kernel, or ki_select_embedded_kernel (one atomic per wavefront)
//   obs_lists_launch     obslist_kernels.hip: the observations of every selected point in arrival order, each with its keyframe's bad flag
//   ki_sort_kernel       a wavefront per point: every observation's rank by slot (slots are unique within a point, so the result does not
//                        depend on arrival order) and its rank among the observations whose keyframe is not bad -> the observation slots
//                        and the election rows by ascending slot; the reference record; the point's MpuPoint, its status, and its place in
//                        a work list: one of the four lane-group classes, or the large points with their blocks of 64 election rows
//   ki_small_kernel<W>   worst-case grids that read their count from KiHdr and leave at once without work
//   ki_large_kernel      a fixed grid that strides over the block list
//   ki_finish_kernel     the winner's descriptor row of every large point
// Election and geometry are the kernel bodies of mappoint_device.h, the ones dsh_mappoint_update runs.  Compiled without FMA
// contraction (see include/defslam_hip.h).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "kfinsert_problem.h"
#include "mappoint_device.h"
#include "mpdb_device.h"

namespace {

__global__ __launch_bounds__(KI_BLOCK) void ki_clear_kernel(KiBufs b, int new_kf) {
  const int i = blockIdx.x * KI_BLOCK + threadIdx.x;
  if (i < b.P) {
    b.ol.sel_of[i] = -1;
    if (new_kf) { b.first_i[i] = KI_UNMARKED; b.observes[i] = 0; }
  }
  if (i < b.S) { b.sel_pid[i] = -1; b.ol.cnt[i] = 0; b.ol.fill[i] = 0; b.large_key[i] = 0xFFFFFFFFu; }
  if (i == 0) {
    KiHdr h = {};
    *b.hdr = h;
  }
}

__global__ __launch_bounds__(KI_BLOCK) void ki_first_kernel(KiBufs b) {
  const int i = blockIdx.x * KI_BLOCK + threadIdx.x;
  if (i >= b.N) return;
  const int p = b.table[b.tab_off + i];
  if (p >= 0) atomicMin(&b.first_i[p], i);
}

__global__ __launch_bounds__(KI_BLOCK) void ki_observes_kernel(KiBufs b) {
  for (long long r = (long long)blockIdx.x * KI_BLOCK + threadIdx.x; r < b.ol.R; r += (long long)gridDim.x * KI_BLOCK) {
    const int2 rec = b.ol.log[r];
    if (rec.x >= 0 && rec.y == b.slot) b.observes[rec.x] = 1;
  }
}

// LocalMapping.cc:142-161 over the table in order; one workgroup
__global__ __launch_bounds__(KI_BLOCK) void ki_classify_kernel(KiBufs b) {
  __shared__ int wsum[KI_BLOCK / 64];
  int base = 0, n_empty = 0, n_bad = 0, n_recent = 0;
  for (int t0 = 0; t0 < b.N; t0 += KI_BLOCK) {
    const int i = t0 + threadIdx.x;
    int p = -1, a = 0;
    if (i < b.N) {
      p = b.table[b.tab_off + i];
      a = p < 0 ? 0 : b.bad[p] ? 1 : (!b.observes[p] && b.first_i[p] == i) ? 2 : 3;
      b.out_action[i] = (uint8_t)a;
      n_empty += a == 0;
      n_bad += a == 1;
      n_recent += a == 3;
    }
    const bool take = a == 2;
    const int pos = ordered_slot<KI_BLOCK>(take, base, wsum);
    if (take) {   // pos < N: the host reserved N records behind R and N entries of the selection
      b.ol.log[b.ol.R + pos] = make_int2(p, b.slot);
      b.ol.log_idx[b.ol.R + pos] = i;
      b.nobs[p] += 1;   // MapPoint.cc:116-119; the lowest entry alone takes the point
      b.ol.sel_of[p] = pos;
      b.sel_pid[pos] = p;
      b.out_added[pos] = p;
    }
  }
  atomicAdd(&b.hdr->n_empty, n_empty);
  atomicAdd(&b.hdr->n_bad, n_bad);
  atomicAdd(&b.hdr->n_recent, n_recent);
  if (threadIdx.x == 0) { b.hdr->n_sel = base; b.hdr->n_appended = base; }
}

__global__ __launch_bounds__(KI_BLOCK) void ki_select_ids_kernel(KiBufs b) {
  const int i = blockIdx.x * KI_BLOCK + threadIdx.x;
  if (i == 0) b.hdr->n_sel = b.n_ids;
  if (i >= b.n_ids) return;
  const int p = b.ids[i];
  if (b.bad[p]) {
    atomicAdd(&b.hdr->n_skipped_bad, 1);
    if (b.out_status) b.out_status[i] = DSH_MP_SKIPPED_BAD;
    return;
  }
  b.ol.sel_of[p] = i;
  b.sel_pid[i] = p;
}

// DefMapPoint::Repose's points: not bad, with a facet
__global__ __launch_bounds__(KI_BLOCK) void ki_select_embedded_kernel(KiBufs b) {
  const int p = blockIdx.x * KI_BLOCK + threadIdx.x;
  const bool take = p < b.P && !b.bad[p] && b.nodes[3 * (size_t)p] >= 0;
  const int k = wave_append(take, &b.hdr->n_sel);
  if (take) {   // k < S = P
    b.ol.sel_of[p] = k;
    b.sel_pid[k] = p;
  }
}

__device__ __forceinline__ int width_class(int M) { return M <= 8 ? 0 : M <= 16 ? 1 : M <= 32 ? 2 : 3; }

__global__ __launch_bounds__(64) void ki_sort_kernel(KiBufs b) {
  const int lane = threadIdx.x, n = b.hdr->n_sel;
  for (int k = blockIdx.x; k < n; k += gridDim.x) {
    const int pid = b.sel_pid[k];
    if (pid < 0) continue;   // wave-uniform: an id that names a bad point
    const int M = b.ol.cnt[k], o = b.ol.off[k], ref = b.ref_kf[pid];
    int ngood = 0, ref_idx = 0;   // observations[pRefKF] of a copy that lacks pRefKF inserts and yields 0
    bool has_ref = false;
    for (int base = 0; base < M; base += 64) {
      const int i = base + lane;
      const bool valid = i < M;
      const uint32_t v = valid ? (uint32_t)b.ol.raw_slot[o + i] : 0u;
      const int s = (int)(v & 0x7FFFFFFFu), j = valid ? b.ol.raw_idx[o + i] : 0;
      const bool good = valid && !(v >> 31);
      int grank;
      const int rank = obs_rank(b.ol.raw_slot, o, M, s, grank);
      if (valid) b.obs_slot[o + rank] = s;                          // rank < M: slots are unique within a point
      if (good) b.el_row[o + grank] = b.slots[s].row_off + j;       // grank < the good ones <= M
      ngood += __popcll(__ballot(good));
      const unsigned long long mr = __ballot(valid && s == ref);
      if (mr) { ref_idx = __shfl(j, __ffsll((long long)mr) - 1, 64); has_ref = true; }
    }
    if (lane == 0) {   // the wavefront stays converged: the next point starts with ballots of all 64 lanes
      MpuPoint pt;
      pt.x = b.xyz[3 * (size_t)pid]; pt.y = b.xyz[3 * (size_t)pid + 1]; pt.z = b.xyz[3 * (size_t)pid + 2];
      pt.obs_off = o; pt.M = M; pt.el_off = o; pt.Me = ngood;
      pt.ref_slot = -1; pt.sf_level = 0.f; pt.sf_last = 0.f; pt.pad = 0;
      int what = b.what, status = 0;
      if (M == 0) {
        status = DSH_MP_NO_OBS;
        what = 0;
        atomicAdd(&b.hdr->n_no_obs, 1);
      } else {
        if (ngood == 0) { status |= DSH_MP_NO_GOOD_DESC; atomicAdd(&b.hdr->n_no_good_desc, 1); }
        // no reference keyframe; one that is not observed and has no key point 0 to lend its octave counts as none
        if (ref < 0 || (!has_ref && b.ol.kf[ref].N <= 0)) {
          status |= DSH_MP_NO_REF;
          what &= ~DSH_MP_NORMAL_DEPTH;
          atomicAdd(&b.hdr->n_no_ref, 1);
        } else if (what & DSH_MP_NORMAL_DEPTH) {
          const int level = b.oct[b.slots[ref].row_off + ref_idx];   // < levels: the host refuses a store with an octave >= levels
          pt.ref_slot = ref;
          pt.sf_level = b.sf[MPU_MAX_LEVELS * (size_t)ref + level];
          pt.sf_last = b.sf[MPU_MAX_LEVELS * (size_t)ref + b.levels[ref] - 1];
        }
      }
      pt.what = what;
      b.pts[k] = pt;
      if (b.out_status) b.out_status[k] = status;
      const bool elect = (what & DSH_MP_DESCRIPTOR) && ngood > 0, geom = (what & DSH_MP_NORMAL_DEPTH) != 0;
      if (!elect && !geom) {
        // nothing to compute: no work list
      } else if (M <= MPU_SMALL) {
        const int c = width_class(M);
        b.small_list[(size_t)c * b.S + atomicAdd(&b.hdr->cls_n[c], 1)] = k;   // at most S points in a class
      } else {
        b.large_pts[atomicAdd(&b.hdr->n_large, 1)] = k;
        const int nb = (geom ? 1 : 0) + (elect ? (ngood + MPU_ROWS - 1) / MPU_ROWS : 0);
        int at = atomicAdd(&b.hdr->n_blocks, nb);   // the host sized the list for every observation in a large point
        if (geom) b.large_blocks[at++] = make_int2(k, -1);
        if (elect)
          for (int r = 0; r < ngood; r += MPU_ROWS) b.large_blocks[at++] = make_int2(k, r);
      }
    }
  }
}

// the lists the device built, the results into the point store: a point k of the selection is the store's point sel_pid[k]
struct KiView {
  const KiBufs& b;
  const int32_t* list;
  int n;
  __device__ int id(int k) const { return b.sel_pid[k]; }
  __device__ void store_desc(int pid, int, const uint4& d0, const uint4& d1) const {
    b.desc[2 * (size_t)pid] = d0;
    b.desc[2 * (size_t)pid + 1] = d1;
  }
  __device__ float* normal(int pid) const { return b.normal + 3 * (size_t)pid; }
  __device__ void store_depth(int pid, float mx, float) const { b.max_distance[pid] = mx; }   // mfMaxDistance alone is kept
};

// mpu_small_kernel on the device-built list of width class c: a worst-case grid that reads its count from KiHdr
template <int W>
__global__ __launch_bounds__(256) void ki_small_kernel(KiBufs b, int c) {
  __shared__ uint4 sd[2 * 256];
  mp_small_body<W>(KiView{b, b.small_list + (size_t)c * b.S, b.hdr->cls_n[c]}, sd);
}

// mpu_large_kernel, one wavefront striding over the device-built block list
__global__ __launch_bounds__(64) void ki_large_kernel(KiBufs b) {
  __shared__ uint32_t hist[64 * MPU_HIST_WORDS];
  mp_large_body(KiView{b, nullptr, b.hdr->n_blocks}, hist);
}

__global__ __launch_bounds__(64) void ki_finish_kernel(KiBufs b) { mp_finish_body(KiView{b, b.large_pts, b.hdr->n_large}); }

// from the selection to the results: R_max bounds the log the passes read
hipError_t upkeep_launches(const KiBufs& b, long long R_max, hipStream_t st) {
  if (b.S == 0) return hipGetLastError();
  ObsLists a = b.ol;
  a.n = b.S; a.n_dev = &b.hdr->n_sel; a.n_extra = &b.hdr->n_appended; a.total = &b.hdr->total;
  const hipError_t e = obs_lists_launch(a, R_max, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ki_sort_kernel, dim3(b.S < 4096 ? b.S : 4096), dim3(64), 0, st, b);
  hipLaunchKernelGGL(ki_large_kernel, dim3(KI_LARGE_GRID), dim3(64), 0, st, b);
  hipLaunchKernelGGL(ki_finish_kernel, dim3(b.S < 64 * 256 ? (b.S + 63) / 64 : 256), dim3(64), 0, st, b);
  hipLaunchKernelGGL(ki_small_kernel<8>, dim3((b.S + 31) / 32), dim3(256), 0, st, b, 0);
  hipLaunchKernelGGL(ki_small_kernel<16>, dim3((b.S + 15) / 16), dim3(256), 0, st, b, 1);
  hipLaunchKernelGGL(ki_small_kernel<32>, dim3((b.S + 7) / 8), dim3(256), 0, st, b, 2);
  hipLaunchKernelGGL(ki_small_kernel<64>, dim3((b.S + 3) / 4), dim3(256), 0, st, b, 3);
  return hipGetLastError();
}

}  // namespace

extern "C" hipError_t ki_process_new_launch(const KiBufs& b, hipStream_t st) {
  const int top = b.P > b.S ? b.P : b.S;
  hipLaunchKernelGGL(ki_clear_kernel, dim3(blocks_for(top > 1 ? top : 1, KI_BLOCK)), dim3(KI_BLOCK), 0, st, b, 1);
  if (b.N > 0) hipLaunchKernelGGL(ki_first_kernel, dim3(blocks_for(b.N, KI_BLOCK)), dim3(KI_BLOCK), 0, st, b);
  if (b.ol.R > 0) hipLaunchKernelGGL(ki_observes_kernel, dim3(log_blocks(b.ol.R, KI_BLOCK)), dim3(KI_BLOCK), 0, st, b);
  hipLaunchKernelGGL(ki_classify_kernel, dim3(1), dim3(KI_BLOCK), 0, st, b);
  return upkeep_launches(b, b.ol.R + b.N, st);
}

extern "C" hipError_t ki_upkeep_launch(const KiBufs& b, int embedded, hipStream_t st) {
  const int top = b.P > b.S ? b.P : b.S;
  hipLaunchKernelGGL(ki_clear_kernel, dim3(blocks_for(top > 1 ? top : 1, KI_BLOCK)), dim3(KI_BLOCK), 0, st, b, 0);
  if (embedded) {
    if (b.P > 0) hipLaunchKernelGGL(ki_select_embedded_kernel, dim3(blocks_for(b.P, KI_BLOCK)), dim3(KI_BLOCK), 0, st, b);
  } else if (b.n_ids > 0) {
    hipLaunchKernelGGL(ki_select_ids_kernel, dim3(blocks_for(b.n_ids, KI_BLOCK)), dim3(KI_BLOCK), 0, st, b);
  }
  return upkeep_launches(b, b.ol.R, st);
}
