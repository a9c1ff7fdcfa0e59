// The resident Surface of a keyframe on the map point store (dsh_keyframe_surface_set_points, _set_normals, _take_normals, _gather,
// dsh_keyframe_sfn; gfx950).
//   Surface::setNormalSurfacePoint, numberofNormals_    Modules/Mapping/Surface.cc:76-85
//   Surface::getNormalSurfacePoint, mpKeypointNorm      Modules/Mapping/NormalEstimator.cc:60-110 (x0 / ref_uv of a solve)
//   Surface::set3DSurfacePoint                          Modules/Mapping/Surface.cc:94-97
//   ShapeFromNormals::obtainM, the walk                 Modules/Mapping/ShapeFromNormals.cc:190-210
// Normals are applied in call order: a target named twice keeps the later one.  That is an election -- the largest j per entry by an
// integer atomicMax, which no schedule changes -- and a second pass in which only the elected j writes and counts.  The selection runs
// in ONE workgroup, like the selection of surfreg_kernels.hip: the sites are numbered in entry order across the workgroup's tiles
// (ordered_slot, mpdb_device.h).  Nothing here computes in floating point: normals and coordinates are copied, or widened exactly.
#include <hip/hip_runtime.h>

#include "mpdb_device.h"
#include "surfstore_problem.h"

namespace {

__global__ __launch_bounds__(SS_BLOCK) void ss_elect_kernel(SsTargets t) {
  const int j = blockIdx.x * SS_BLOCK + threadIdx.x;
  if (j < t.n) atomicMax(&t.winner[t.entry[j] - t.base], j);
}

__global__ __launch_bounds__(SS_BLOCK) void ss_write_normals_kernel(SsStore s, SsTargets t, SsNormalSource src) {
  const int j = blockIdx.x * SS_BLOCK + threadIdx.x;
  if (j >= t.n) return;
  const size_t e = (size_t)t.entry[j];
  if (t.winner[e - t.base] != j) return;   // a later entry of the call names the same target
  const float* n = src.normals + 3 * (size_t)j;
  if (src.sel) {
    const int q = src.sel[j];
    n = q >= 0 ? src.nref + 3 * (size_t)q : src.nrec + 3 * (size_t)(-1 - q);
  }
  for (int r = 0; r < 3; r++) s.normal[3 * e + r] = n[r];
  if (!s.has[e]) {   // Surface.cc:79-82: counted once
    s.has[e] = 1;
    atomicAdd(&s.n_normals[t.slot[j]], 1);
  }
}

__global__ __launch_bounds__(SS_BLOCK) void ss_gather_kernel(SsStore s, SsTargets t, float* normal_xy, uint8_t* has, float* uv) {
  const int j = blockIdx.x * SS_BLOCK + threadIdx.x;
  if (j >= t.n) return;
  const size_t e = (size_t)t.entry[j];
  const bool h = s.has[e] != 0;
  normal_xy[2 * (size_t)j] = h ? s.normal[3 * e] : 0.f;
  normal_xy[2 * (size_t)j + 1] = h ? s.normal[3 * e + 1] : 0.f;
  has[j] = h ? 1 : 0;
  uv[2 * (size_t)j] = s.kpn[2 * e];
  uv[2 * (size_t)j + 1] = s.kpn[2 * e + 1];
}

__global__ __launch_bounds__(SS_BLOCK) void ss_set_points_kernel(SsStore s, int32_t tab_off, int32_t n, const int32_t* idx, const float* pts_in) {
  const int j = blockIdx.x * SS_BLOCK + threadIdx.x;
  if (j >= n) return;
  const size_t e = (size_t)tab_off + idx[j];
  for (int r = 0; r < 3; r++) s.pts[3 * e + r] = pts_in[3 * (size_t)j + r];
}

// ShapeFromNormals.cc:190-210 per entry, the sites in entry order
__global__ __launch_bounds__(SS_SELECT_BLOCK) void ss_select_kernel(TcState st, SsStore s, SsSelect k) {
  __shared__ int wsum[SS_SELECT_BLOCK / 64];
  const int t = threadIdx.x, N = k.N;
  int n_sites = 0;
  bool cls[4] = {false, false, false, false};   // this thread's entries are counted tile by tile
  int sums[4] = {0, 0, 0, 0};
  for (int base = 0; base < N; base += SS_SELECT_BLOCK) {
    const int i = base + t;
    int c = -1;
    size_t e = 0;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (i < N) {
      e = (size_t)k.tab_off + i;
      const int p = k.table[e];
      if (p < 0) c = 0;
      else if (st.bad[p]) c = 1;
      else if (!s.has[e]) c = 2;
      else {
        nx = s.normal[3 * e]; ny = s.normal[3 * e + 1]; nz = s.normal[3 * e + 2];
        c = (nx == nx && ny == ny && nz == nz) ? 4 : 3;   // Normal == Normal on a cv::Vec3f: an infinite component passes
      }
      k.u_all[i] = (double)s.kpn[2 * e];
      k.v_all[i] = (double)s.kpn[2 * e + 1];
    }
    for (int q = 0; q < 4; q++) cls[q] = c == q;
    const int pos = ordered_slot<SS_SELECT_BLOCK>(c == 4, n_sites, wsum);
    if (c == 4) {   // pos < N: at most one site per entry
      k.u[pos] = (double)s.kpn[2 * e];
      k.v[pos] = (double)s.kpn[2 * e + 1];
      k.normals[3 * (size_t)pos] = nx; k.normals[3 * (size_t)pos + 1] = ny; k.normals[3 * (size_t)pos + 2] = nz;
    }
    const int part = block_sums<SS_SELECT_BLOCK, 4>(cls);
    if (t < 4) sums[t] += part;
  }
  __shared__ int total[4];
  if (t < 4) total[t] = sums[t];
  __syncthreads();
  if (t == 0) {
    SsCounts out;
    out.n_sites = n_sites; out.n_empty = total[0]; out.n_bad = total[1]; out.n_no_normal = total[2]; out.n_nan = total[3];
    out.pad[0] = out.pad[1] = out.pad[2] = 0;
    *k.counts = out;
  }
}

}  // namespace

static_assert(sizeof(SsCounts) == 32, "SsCounts is eight int32");

extern "C" hipError_t ss_elect_launch(const SsTargets& t, hipStream_t st) {
  if (t.n > 0) hipLaunchKernelGGL(ss_elect_kernel, blocks_for(t.n, SS_BLOCK), dim3(SS_BLOCK), 0, st, t);
  return hipGetLastError();
}

extern "C" hipError_t ss_write_normals_launch(const SsStore& s, const SsTargets& t, const SsNormalSource& src, hipStream_t st) {
  if (t.n > 0) hipLaunchKernelGGL(ss_write_normals_kernel, blocks_for(t.n, SS_BLOCK), dim3(SS_BLOCK), 0, st, s, t, src);
  return hipGetLastError();
}

extern "C" hipError_t ss_gather_launch(const SsStore& s, const SsTargets& t, float* normal_xy, uint8_t* has, float* uv, hipStream_t st) {
  if (t.n > 0) hipLaunchKernelGGL(ss_gather_kernel, blocks_for(t.n, SS_BLOCK), dim3(SS_BLOCK), 0, st, s, t, normal_xy, has, uv);
  return hipGetLastError();
}

extern "C" hipError_t ss_set_points_launch(const SsStore& s, int32_t tab_off, int32_t n, const int32_t* idx, const float* pts_in, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(ss_set_points_kernel, blocks_for(n, SS_BLOCK), dim3(SS_BLOCK), 0, st, s, tab_off, n, idx, pts_in);
  return hipGetLastError();
}

extern "C" hipError_t ss_select_launch(const TcState& st8, const SsStore& s, const SsSelect& k, hipStream_t st) {
  hipLaunchKernelGGL(ss_select_kernel, 1, dim3(SS_SELECT_BLOCK), 0, st, st8, s, k);
  return hipGetLastError();
}
