// Stand-alone check of the host logic of dsh_track_sft between its two device stages (defslam_amd/csrc/tracksft_host.h): the downloaded
// table as the dsh_sft_frame of the packer, the table handed to the caller, the scatter of the flags into mvbOutlier.  Every buffer is a
// heap block of exactly the size the call site gives it (the table's arrays with room for N rows, the caller's with room for `capacity`,
// the flags with M entries, mvbOutlier with N), so AddressSanitizer sees a read or write past it; no GPU is touched.  From the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/diag/tracksft_host_check.cpp \
//     -o /tmp/tracksft_host_check && /tmp/tracksft_host_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../defslam_amd/csrc/tracksft_host.h"

template <class T> T* exact(size_t n) { return static_cast<T*>(std::malloc(sizeof(T) * (n ? n : 1))); }

static void fail(const char* what) { std::printf("%s\n", what); std::exit(1); }

// N key points of which every `step`-th gives a row; the caller's arrays have room for `capacity` (< 0: no arrays)
static void run(int N, int step, int capacity) {
  std::vector<int> rows;
  for (int i = step - 1; i < N; i += step) rows.push_back(i);
  const int M = (int)rows.size();
  const size_t n = (size_t)N;
  int32_t *kp_index = exact<int32_t>(n), *point_id = exact<int32_t>(n), *nodes = exact<int32_t>(3 * n);
  double *bary = exact<double>(3 * n), *uv = exact<double>(2 * n), *invsig2 = exact<double>(n);
  for (int m = 0; m < M; m++) {
    kp_index[m] = rows[m];
    point_id[m] = 7 * m;
    for (int k = 0; k < 3; k++) { nodes[3 * m + k] = m + k; bary[3 * m + k] = 0.25 * (k + 1); }
    uv[2 * m] = m; uv[2 * m + 1] = -m;
    invsig2[m] = 1.0 / (m + 1);
  }
  TfTable t;
  t.M = M; t.points_obs = M + 2;
  t.kp_index = kp_index; t.point_id = point_id; t.nodes = nodes; t.bary = bary; t.uv = uv; t.invsig2 = invsig2;

  float Tcw[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  double xyz[3] = {0, 0, 1};
  dsh_track_sft_frame f = dsh_track_sft_frame();
  f.Tcw = Tcw; f.N = N; f.xyz = xyz;
  f.K[0] = 500; f.K[1] = 501; f.K[2] = 320; f.K[3] = 240;
  f.reg_lap = 1; f.reg_inex = 2; f.reg_temp = 3; f.neighbour_layers = 1; f.max_iters = 50;
  const dsh_sft_frame s = tf_sft_frame(f, t);
  if (s.n_frame != N || s.M != M || s.obs_nodes != nodes || s.obs_bary != bary || s.obs_uv != uv || s.obs_invsig2 != invsig2 || s.xyz != xyz ||
      s.Tcw != Tcw || s.K[1] != 501 || s.reg_temp != 3 || s.max_iters != 50 || s.neighbour_layers != 1)
    fail("sft frame wrong");

  dsh_track_sft_table out = dsh_track_sft_table();
  out.M = out.points_obs = -7;
  if (capacity >= 0) {
    const size_t c = (size_t)capacity;
    out.capacity = capacity;
    out.kp_index = exact<int32_t>(c); out.point_id = exact<int32_t>(c); out.nodes = exact<int32_t>(3 * c);
    out.bary = exact<double>(3 * c); out.uv = exact<double>(2 * c); out.invsig2 = exact<double>(c);
  }
  const bool fits = tf_table_fits(t, out);
  if (fits != (capacity < 0 || capacity >= M)) fail("fits wrong");
  if (fits) {
    tf_hand_out(t, &out);
    if (out.M != M || out.points_obs != M + 2) fail("counts wrong");
    if (capacity >= 0)
      for (int m = 0; m < M; m++)
        if (out.kp_index[m] != rows[m] || out.point_id[m] != 7 * m || out.nodes[3 * m + 2] != m + 2 || out.bary[3 * m + 1] != 0.5 || out.uv[2 * m + 1] != -m ||
            out.invsig2[m] != 1.0 / (m + 1))
          fail("row wrong");
  } else if (out.M != -7) {
    fail("a refusal wrote");
  }
  // the scatter: M flags into N entries, the others keep their value
  uint8_t *flags = exact<uint8_t>((size_t)M), *outlier = exact<uint8_t>(n);
  for (int m = 0; m < M; m++) flags[m] = (uint8_t)(m & 1);
  for (int i = 0; i < N; i++) outlier[i] = 3;
  tf_scatter_flags(t, flags, outlier);
  int m = 0;
  for (int i = 0; i < N; i++) {
    const bool row = m < M && rows[m] == i;
    if (outlier[i] != (row ? (m & 1) : 3)) fail("scatter wrong");
    if (row) m++;
  }
  for (void* p : {(void*)kp_index, (void*)point_id, (void*)nodes, (void*)bary, (void*)uv, (void*)invsig2, (void*)flags, (void*)outlier, (void*)out.kp_index,
                  (void*)out.point_id, (void*)out.nodes, (void*)out.bary, (void*)out.uv, (void*)out.invsig2})
    std::free(p);
}

int main() {
  for (int N : {0, 1, 2, 63, 64, 65, 300, 8192})
    for (int step : {1, 2, 7, 10000})
      for (int cap : {-1, 0, 1, N / 2, N}) run(N, step, cap);
  std::printf("track sft host functions: ok\n");
  return 0;
}
