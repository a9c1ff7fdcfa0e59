// Kernels of the ORB front end (orb_problem.h; the readings of the OpenCV steps are stated in include/defslam_hip.h).  Integer valued
// except the angle and the rotated sampling positions, which are float32 with one rounding per operation: this file is compiled without
// FMA contraction.  Wavefronts of 64 lanes.
#include <hip/hip_runtime.h>

#include <float.h>

#include "mpdb_device.h"
#include "orb_problem.h"

namespace {

__device__ __forceinline__ int reflect101(int p, int n) { return p < 0 ? -p : (p >= n ? 2 * n - 2 - p : p); }

// ---- pyramid ---------------------------------------------------------------------------------------------------------------------

// level 0 and its frame: one thread per pixel of the framed plane
__global__ void __launch_bounds__(ORB_BLOCK) orb_frame_image_kernel(OrbLevel l, const uint8_t* __restrict__ image, long long stride) {
  const int pw = l.w + 2 * ORB_FRAME, ph = l.h + 2 * ORB_FRAME;
  const long long i = (long long)blockIdx.x * ORB_BLOCK + threadIdx.x;
  if (i >= (long long)pw * ph) return;
  const int fy = (int)(i / pw), fx = (int)(i - (long long)fy * pw);
  const int x = reflect101(fx - ORB_FRAME, l.w), y = reflect101(fy - ORB_FRAME, l.h);
  l.plane[i] = image[(long long)y * stride + x];
}

// a level from the one below: a frame pixel is the resized pixel it reflects, so the level and its frame come out of one pass
__global__ void __launch_bounds__(ORB_BLOCK) orb_resize_kernel(OrbLevel below, OrbLevel l) {
  const int pw = l.w + 2 * ORB_FRAME, ph = l.h + 2 * ORB_FRAME;
  const long long i = (long long)blockIdx.x * ORB_BLOCK + threadIdx.x;
  if (i >= (long long)pw * ph) return;
  const int fy = (int)(i / pw), fx = (int)(i - (long long)fy * pw);
  const int x = reflect101(fx - ORB_FRAME, l.w), y = reflect101(fy - ORB_FRAME, l.h);
  const int sx = l.xtab[3 * x], a0 = l.xtab[3 * x + 1], a1 = l.xtab[3 * x + 2];
  const int sy = l.ytab[3 * y], b0 = l.ytab[3 * y + 1], b1 = l.ytab[3 * y + 2];
  const int sx1 = min(sx + 1, below.w - 1), sy1 = min(sy + 1, below.h - 1);
  const int bpw = below.w + 2 * ORB_FRAME;
  const uint8_t* r0 = below.plane + (long long)(sy + ORB_FRAME) * bpw + ORB_FRAME;
  const uint8_t* r1 = below.plane + (long long)(sy1 + ORB_FRAME) * bpw + ORB_FRAME;
  const int h0 = r0[sx] * a0 + r0[sx1] * a1, h1 = r1[sx] * a0 + r1[sx1] * a1;
  l.plane[i] = (uint8_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
}

// the blurred planes: a workgroup stages the 38 x 14 frame pixels of its 32 x 8 outputs, row pass into LDS, column pass out
__global__ void __launch_bounds__(ORB_BLOCK) orb_blur_kernel(OrbLevels L) {
  __shared__ uint8_t s_src[ORB_BLUR_TY + 6][ORB_BLUR_TX + 8];
  __shared__ int s_row[ORB_BLUR_TY + 6][ORB_BLUR_TX];
  int lv = 0;
  while (lv + 1 < L.levels && (int)blockIdx.x >= L.l[lv + 1].blur_tile0) lv++;
  const OrbLevel l = L.l[lv];
  const int t = blockIdx.x - l.blur_tile0, ty = t / l.blur_tiles_x, tx = t - ty * l.blur_tiles_x;
  const int ox = tx * ORB_BLUR_TX, oy = ty * ORB_BLUR_TY;
  const int pw = l.w + 2 * ORB_FRAME, ph = l.h + 2 * ORB_FRAME, bw = l.w + 2 * ORB_BLUR_MARGIN, bh = l.h + 2 * ORB_BLUR_MARGIN;
  // blurred pixel (bx, by) is level pixel (bx - 3, by - 3), frame pixel (bx + 16, by + 16); its taps reach 3 further
  const int fx0 = ox + ORB_FRAME - ORB_BLUR_MARGIN - 3, fy0 = oy + ORB_FRAME - ORB_BLUR_MARGIN - 3;
  for (int i = threadIdx.x; i < (ORB_BLUR_TY + 6) * (ORB_BLUR_TX + 6); i += ORB_BLOCK) {
    const int r = i / (ORB_BLUR_TX + 6), c = i - r * (ORB_BLUR_TX + 6);
    // a partial tile's outputs beyond the plane are dropped: their taps are clamped into the frame
    s_src[r][c] = l.plane[(long long)min(fy0 + r, ph - 1) * pw + min(fx0 + c, pw - 1)];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < (ORB_BLUR_TY + 6) * ORB_BLUR_TX; i += ORB_BLOCK) {
    const int r = i / ORB_BLUR_TX, c = i - r * ORB_BLUR_TX;
    const uint8_t* s = &s_src[r][c];
    s_row[r][c] = 18 * (s[0] + s[6]) + 34 * (s[1] + s[5]) + 49 * (s[2] + s[4]) + 55 * s[3];
  }
  __syncthreads();
  const int cx = threadIdx.x % ORB_BLUR_TX, cy = threadIdx.x / ORB_BLUR_TX;
  const int bx = ox + cx, by = oy + cy;
  if (bx < bw && by < bh) {
    const int sum = 18 * (s_row[cy][cx] + s_row[cy + 6][cx]) + 34 * (s_row[cy + 1][cx] + s_row[cy + 5][cx]) +
                    49 * (s_row[cy + 2][cx] + s_row[cy + 4][cx]) + 55 * s_row[cy + 3][cx];
    l.blur[(long long)by * bw + bx] = (uint8_t)min(255, (sum + 32768) >> 16);
  }
}

// ---- FAST ------------------------------------------------------------------------------------------------------------------------

// the largest, over the 16 arcs of 9 contiguous circle pixels, of the arc's smallest d: minima of 2, 4, 8 and 9 neighbours in turn
__device__ __forceinline__ int best_arc_min(const int (&d)[16]) {
  int a[16], b[16], c[16];
#pragma unroll
  for (int k = 0; k < 16; k++) a[k] = min(d[k], d[(k + 1) & 15]);
#pragma unroll
  for (int k = 0; k < 16; k++) b[k] = min(a[k], a[(k + 2) & 15]);
#pragma unroll
  for (int k = 0; k < 16; k++) c[k] = min(b[k], b[(k + 4) & 15]);
  int best = -255;
#pragma unroll
  for (int k = 0; k < 16; k++) best = max(best, min(c[k], d[(k + 8) & 15]));
  return best;
}

#define ORB_CELL_STRIDE 68

// the workgroup's sum of v; every thread calls it (two barriers)
__device__ __forceinline__ int block_sum(int v, int* wsum) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int w = 0; w < ORB_BLOCK / 64; w++) s += wsum[w];
  return s;
}

// a region pixel keeps its corner at threshold th: M > th and M above its 8 neighbours (outside the region the plane holds 0)
__device__ __forceinline__ bool fast_keeps(const uint8_t* sc, int th) {
  const int m = sc[0];
  if (m <= th) return false;
  const uint8_t *u = sc - ORB_CELL_STRIDE, *d = sc + ORB_CELL_STRIDE;
  return m > u[-1] && m > u[0] && m > u[1] && m > sc[-1] && m > sc[1] && m > d[-1] && m > d[0] && m > d[1];
}

// one workgroup per cell: the sub-image and the plane of M in LDS, suppression from LDS, the retry at min_th when ini_th leaves nothing
__global__ void __launch_bounds__(ORB_BLOCK) orb_fast_kernel(OrbLevels L, OrbDetect D) {
  __shared__ uint8_t s_img[ORB_CELL_MAX * ORB_CELL_STRIDE];
  __shared__ uint8_t s_m[ORB_CELL_MAX * ORB_CELL_STRIDE];
  __shared__ int s_wsum[ORB_BLOCK / 64];
  const OrbCell cell = D.cells[blockIdx.x];
  const OrbLevel l = L.l[cell.level];
  const int cw = cell.x1 - cell.x0, ch = cell.y1 - cell.y0;   // at most ORB_CELL_MAX each (checked by the host)
  const int pw = l.w + 2 * ORB_FRAME;
  const uint8_t* src = l.plane + (long long)(cell.y0 + ORB_FRAME) * pw + cell.x0 + ORB_FRAME;
  for (int i = threadIdx.x; i < ORB_CELL_MAX * ORB_CELL_STRIDE; i += ORB_BLOCK) {
    const int y = i / ORB_CELL_STRIDE, x = i - y * ORB_CELL_STRIDE;
    s_img[i] = (x < cw && y < ch) ? src[(long long)y * pw + x] : 0;
    s_m[i] = 0;
  }
  __syncthreads();
  const int rw = cw - 6, rh = ch - 6;                          // the detection region; either may be <= 0
  const int n = (rw > 0 && rh > 0) ? rw * rh : 0;
  for (int i = threadIdx.x; i < n; i += ORB_BLOCK) {
    const int y = i / rw + 3, x = i - (y - 3) * rw + 3;
    const uint8_t* p = &s_img[y * ORB_CELL_STRIDE + x];
    const int v = p[0];
    int d[16], e[16];
    d[0] = p[3 * ORB_CELL_STRIDE] - v;       d[1] = p[3 * ORB_CELL_STRIDE + 1] - v;   d[2] = p[2 * ORB_CELL_STRIDE + 2] - v;
    d[3] = p[ORB_CELL_STRIDE + 3] - v;       d[4] = p[3] - v;                         d[5] = p[-ORB_CELL_STRIDE + 3] - v;
    d[6] = p[-2 * ORB_CELL_STRIDE + 2] - v;  d[7] = p[-3 * ORB_CELL_STRIDE + 1] - v;  d[8] = p[-3 * ORB_CELL_STRIDE] - v;
    d[9] = p[-3 * ORB_CELL_STRIDE - 1] - v;  d[10] = p[-2 * ORB_CELL_STRIDE - 2] - v; d[11] = p[-ORB_CELL_STRIDE - 3] - v;
    d[12] = p[-3] - v;                       d[13] = p[ORB_CELL_STRIDE - 3] - v;      d[14] = p[2 * ORB_CELL_STRIDE - 2] - v;
    d[15] = p[3 * ORB_CELL_STRIDE - 1] - v;
#pragma unroll
    for (int k = 0; k < 16; k++) e[k] = -d[k];
    s_m[y * ORB_CELL_STRIDE + x] = (uint8_t)max(0, max(best_arc_min(d), best_arc_min(e)));
  }
  __syncthreads();
  int th = D.ini_th, total = 0;
  for (int round = 0; round < 2; round++) {
    int mine = 0;
    for (int i = threadIdx.x; i < n; i += ORB_BLOCK) {
      const int y = i / rw + 3, x = i - (y - 3) * rw + 3;
      mine += fast_keeps(&s_m[y * ORB_CELL_STRIDE + x], th) ? 1 : 0;
    }
    total = block_sum(mine, s_wsum);                           // the same in every thread
    if (total > 0 || D.min_th == th) break;
    th = D.min_th;
  }
  for (int i = threadIdx.x; i < n; i += ORB_BLOCK) {
    const int y = i / rw + 3, x = i - (y - 3) * rw + 3;
    const uint8_t* sc = &s_m[y * ORB_CELL_STRIDE + x];
    l.kept[(long long)(cell.y0 + y) * l.w + cell.x0 + x] = fast_keeps(sc, th) ? sc[0] : 0;
  }
  if (threadIdx.x == 0) D.cell_count[blockIdx.x] = total;
}

// one workgroup: per level the exclusive scan of the cells' counts in cell order, and the level's count
__global__ void __launch_bounds__(ORB_BLOCK) orb_scan_kernel(OrbLevels L, OrbDetect D) {
  __shared__ int s_wsum[ORB_BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int lv = 0; lv < L.levels; lv++) {
    int base = 0;
    const int c1 = D.level_cell0[lv + 1];
    for (int c0 = D.level_cell0[lv]; c0 < c1; c0 += ORB_BLOCK) {
      const int c = c0 + threadIdx.x;
      const int v = c < c1 ? D.cell_count[c] : 0;
      int inc = v;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
      }
      __syncthreads();
      if (lane == 63) s_wsum[wave] = inc;
      __syncthreads();
      int pre = 0, total = 0;
#pragma unroll
      for (int w = 0; w < ORB_BLOCK / 64; w++) {
        if (w < wave) pre += s_wsum[w];
        total += s_wsum[w];
      }
      if (c < c1) D.cell_offset[c] = base + pre + inc - v;
      base += total;
    }
    if (threadIdx.x == 0) D.counts[lv] = base;
  }
}

// one workgroup per cell: its kept corners behind the cell's offset, in raster order; what does not fit into the capacity is dropped
// (the host sees the true count)
__global__ void __launch_bounds__(ORB_BLOCK) orb_scatter_kernel(OrbLevels L, OrbDetect D) {
  __shared__ int s_wsum[ORB_BLOCK / 64];
  const OrbCell cell = D.cells[blockIdx.x];
  if (D.cell_count[blockIdx.x] == 0) return;                   // the same for the whole workgroup
  const OrbLevel l = L.l[cell.level];
  const int rw = cell.x1 - cell.x0 - 6, rh = cell.y1 - cell.y0 - 6;
  const int n = (rw > 0 && rh > 0) ? rw * rh : 0;
  int base = D.cell_offset[blockIdx.x];
  int32_t* out = D.cand + (long long)cell.level * D.capacity * 3;
  for (int i0 = 0; i0 < n; i0 += ORB_BLOCK) {
    const int i = i0 + threadIdx.x;
    int x = 0, y = 0, m = 0;
    if (i < n) {
      y = cell.y0 + 3 + i / rw;
      x = cell.x0 + 3 + i % rw;
      m = l.kept[(long long)y * l.w + x];
    }
    const int pos = ordered_slot<ORB_BLOCK>(m > 0, base, s_wsum);
    if (m > 0 && pos < D.capacity) {
      out[3 * (long long)pos] = x;
      out[3 * (long long)pos + 1] = y;
      out[3 * (long long)pos + 2] = m - 1;
    }
  }
}

// ---- angle and descriptor --------------------------------------------------------------------------------------------------------

// the end of each row of the circular patch (ORBextractor.cc:454-469)
__constant__ int8_t orb_umax[ORB_HALF_PATCH + 1] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};

// cv::fastAtan2 as include/defslam_hip.h reads it, degrees
__device__ __forceinline__ float orb_fast_atan2(float y, float x) {
  const float scale = (float)(180.0 / 3.14159265358979323846);
  const float p1 = 0.9997878412794807f * scale, p3 = -0.3258083974640975f * scale, p5 = 0.1555786518463281f * scale,
              p7 = -0.04432655554792128f * scale;
  const float ax = fabsf(x), ay = fabsf(y);
  float a, c, c2;
  if (ax >= ay) {
    c = ay / (ax + (float)DBL_EPSILON);
    c2 = c * c;
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  } else {
    c = ax / (ay + (float)DBL_EPSILON);
    c2 = c * c;
    a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  }
  if (x < 0) a = 180.f - a;
  if (y < 0) a = 360.f - a;
  return a;
}

// one wavefront per key point, the pattern in LDS.  Moments: lane 2r + s takes the left (s = 0) or right half of patch row r.  Bits: lane
// l forms bits 4l .. 4l+3 from pattern points 8l .. 8l+7; eight lanes' nibbles are or-ed into a word across lanes.
__global__ void __launch_bounds__(ORB_BLOCK) orb_describe_kernel(OrbLevels L, OrbDescribe D) {
  __shared__ int2 s_pat[ORB_PATTERN_POINTS];
  for (int i = threadIdx.x; i < ORB_PATTERN_POINTS; i += ORB_BLOCK) s_pat[i] = make_int2(D.pattern[2 * i], D.pattern[2 * i + 1]);
  __syncthreads();
  const int lane = threadIdx.x & 63, waves = ORB_BLOCK / 64;
  for (int k = blockIdx.x * waves + (threadIdx.x >> 6); k < D.n; k += gridDim.x * waves) {
    const OrbLevel l = L.l[D.level[k]];
    const int cx = (int)rintf(D.xy[2 * k]), cy = (int)rintf(D.xy[2 * k + 1]);   // inside [16, w - 17] x [16, h - 17]: checked by the host
    const int pw = l.w + 2 * ORB_FRAME, bw = l.w + 2 * ORB_BLUR_MARGIN;
    int m10 = 0, m01 = 0;
    if (lane < 2 * (2 * ORB_HALF_PATCH + 1)) {
      const int v = (lane >> 1) - ORB_HALF_PATCH, d = orb_umax[v < 0 ? -v : v];
      const int u0 = (lane & 1) ? 0 : -d, u1 = (lane & 1) ? d : -1;
      const uint8_t* row = l.plane + (long long)(cy + v + ORB_FRAME) * pw + cx + ORB_FRAME;
      int s = 0;
      for (int u = u0; u <= u1; u++) {
        const int val = row[u];
        m10 += u * val;
        s += val;
      }
      m01 = v * s;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      m10 += __shfl_xor(m10, o, 64);
      m01 += __shfl_xor(m01, o, 64);
    }
    const float angle = orb_fast_atan2((float)m01, (float)m10);
    if (lane == 0) D.angle[k] = angle;
    const float ang = angle * (float)(3.14159265358979323846 / 180.f);
    const float a = (float)cos((double)ang), b = (float)sin((double)ang);
    const uint8_t* centre = l.blur + (long long)(cy + ORB_BLUR_MARGIN) * bw + cx + ORB_BLUR_MARGIN;
    uint32_t nib = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      int t[2];
#pragma unroll
      for (int e = 0; e < 2; e++) {
        const int2 p = s_pat[8 * lane + 2 * j + e];
        const float px = (float)p.x, py = (float)p.y;
        // a pattern point lies within radius sqrt(342) < 18.5: the clamp only guards the plane against a broken pattern
        const int ry = max(-18, min(18, (int)rintf(px * b + py * a))), rx = max(-18, min(18, (int)rintf(px * a - py * b)));
        t[e] = centre[(long long)ry * bw + rx];
      }
      nib |= (t[0] < t[1] ? 1u : 0u) << j;
    }
    uint32_t word = nib << (4 * (lane & 7));
    word |= __shfl_xor(word, 1, 64);
    word |= __shfl_xor(word, 2, 64);
    word |= __shfl_xor(word, 4, 64);
    if ((lane & 7) == 0) D.desc[8 * (long long)k + (lane >> 3)] = word;
  }
}

}  // namespace

extern "C" hipError_t orb_frame_image_launch(const OrbLevel& l0, const uint8_t* image, int64_t row_stride, hipStream_t st) {
  const long long n = (long long)(l0.w + 2 * ORB_FRAME) * (l0.h + 2 * ORB_FRAME);
  hipLaunchKernelGGL(orb_frame_image_kernel, dim3(blocks_for(n, ORB_BLOCK)), dim3(ORB_BLOCK), 0, st, l0, image, (long long)row_stride);
  return hipGetLastError();
}

extern "C" hipError_t orb_resize_launch(const OrbLevel& below, const OrbLevel& l, hipStream_t st) {
  const long long n = (long long)(l.w + 2 * ORB_FRAME) * (l.h + 2 * ORB_FRAME);
  hipLaunchKernelGGL(orb_resize_kernel, dim3(blocks_for(n, ORB_BLOCK)), dim3(ORB_BLOCK), 0, st, below, l);
  return hipGetLastError();
}

extern "C" hipError_t orb_blur_launch(const OrbLevels& L, hipStream_t st) {
  hipLaunchKernelGGL(orb_blur_kernel, dim3(L.blur_tiles), dim3(ORB_BLOCK), 0, st, L);
  return hipGetLastError();
}

extern "C" hipError_t orb_fast_launch(const OrbLevels& L, const OrbDetect& d, hipStream_t st) {
  hipLaunchKernelGGL(orb_fast_kernel, dim3(d.n_cells), dim3(ORB_BLOCK), 0, st, L, d);
  return hipGetLastError();
}

extern "C" hipError_t orb_scan_launch(const OrbLevels& L, const OrbDetect& d, hipStream_t st) {
  hipLaunchKernelGGL(orb_scan_kernel, dim3(1), dim3(ORB_BLOCK), 0, st, L, d);
  return hipGetLastError();
}

extern "C" hipError_t orb_scatter_launch(const OrbLevels& L, const OrbDetect& d, hipStream_t st) {
  hipLaunchKernelGGL(orb_scatter_kernel, dim3(d.n_cells), dim3(ORB_BLOCK), 0, st, L, d);
  return hipGetLastError();
}

extern "C" hipError_t orb_describe_launch(const OrbLevels& L, const OrbDescribe& d, hipStream_t st) {
  const int waves = ORB_BLOCK / 64;
  const int blocks = min(blocks_for(d.n, waves), 2048);
  hipLaunchKernelGGL(orb_describe_kernel, dim3(blocks), dim3(ORB_BLOCK), 0, st, L, d);
  return hipGetLastError();
}
