// Stand-alone check of the host logic of the mapping calls that writes into slices of an upload block (dsh_ctx.h, namespace dsh): the normals
// transpose and owner list, the constant rows of Shape from Normals, the candidate walk of scaleMinMedian.  Every buffer is a heap block of
// exactly the size the call site gives the slice, so AddressSanitizer sees a write past it; no GPU is touched.  From defslam_amd/csrc, after make:
//   S="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
//   for f in dsh_nrsfm dsh_sfn dsh_register; do hipcc -O1 -g -std=c++17 -fPIC $S -c $f.cpp -o /tmp/$f.o; done
//   hipcc -O1 -g -std=c++17 -I. $S -c ../../tools/diag/mapping_host_fill_check.cpp -o /tmp/check.o
//   hipcc -fsanitize=address,undefined --offload-arch=gfx950 /tmp/check.o /tmp/dsh_nrsfm.o /tmp/dsh_sfn.o /tmp/dsh_register.o \
//     $(ls ../lib/obj/*.o | grep -v -E "dsh_(nrsfm|sfn|register)\.o") -o /tmp/mapping_host_fill_check && /tmp/mapping_host_fill_check
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dsh_ctx.h"

template <class T> T* exact(size_t n) { return static_cast<T*>(std::malloc(sizeof(T) * n)); }

static void normals(std::vector<int32_t> ptr) {
  const int P = (int)ptr.size() - 1, R = ptr[P];
  dsh_diffprop* recs = exact<dsh_diffprop>(R);
  for (int r = 0; r < R; r++) { float* f = reinterpret_cast<float*>(&recs[r]); for (int k = 0; k < 18; k++) f[k] = 100.f * r + k; }
  int32_t* owner = exact<int32_t>(R);
  float* soa = exact<float>(18 * (size_t)R);
  if (R > 0) dsh::normals_fill_records(P, ptr.data(), recs, owner, soa);
  for (int r = 0; r < R; r++) {
    if (!(ptr[owner[r]] <= r && r < ptr[owner[r] + 1])) { std::printf("owner wrong\n"); std::exit(1); }
    for (int k = 0; k < 18; k++) if (soa[(size_t)k * R + r] != 100.f * r + k) { std::printf("soa wrong\n"); std::exit(1); }
  }
  std::free(recs); std::free(owner); std::free(soa);
}

static void sfn(int nu, int nv, int n) {
  dsh_bbs b{-0.6, 0.6, nu, -0.5, 0.5, nv, 1};
  const size_t N = (size_t)nu * nv, m = 2 * (size_t)n + N + 1;
  double *tail = exact<double>((N + 1) * N), *rhs = exact<double>(m), *ones = exact<double>(N);
  dsh::sfn_fill_constant_rows(&b, n, 1e-2, 1.3, tail, rhs, ones);
  bool ok = rhs[m - 1] == (double)N * 1.3 && rhs[0] == 0.0;
  for (size_t i = 0; i < N; i++) ok = ok && ones[i] == 1.0 && tail[N * N + i] == 1.0 && tail[i * N + i] > 0.0;
  if (!ok) { std::printf("sfn rows wrong\n"); std::exit(1); }
  std::free(tail); std::free(rhs); std::free(ones);
}

static void smm(int n, std::vector<double> u, int want_nc, long long want_k) {
  int64_t k = -1;
  const int nc = dsh::smm_walk_candidates(n, u.data(), (int64_t)u.size(), nullptr, nullptr, &k);
  if (nc != want_nc || (nc >= 0 && k != want_k)) { std::printf("smm count wrong: %d %lld\n", nc, (long long)k); std::exit(1); }
  if (nc < 0) return;
  int32_t* cand = exact<int32_t>(nc);
  int64_t* off = exact<int64_t>(nc);
  if (dsh::smm_walk_candidates(n, u.data(), (int64_t)u.size(), cand, off, &k) != nc) { std::printf("smm second pass differs\n"); std::exit(1); }
  for (int c = 0; c < nc; c++) if (off[c] + n - 1 > (int64_t)u.size() || cand[c] >= n) { std::printf("smm list wrong\n"); std::exit(1); }
  std::free(cand); std::free(off);
}

int main() {
  normals({0, 1, 3}); normals({0, 0, 3}); normals({0, 0, 0}); normals({0, 2, 2, 7, 7, 1000});
  sfn(4, 4, 3); sfn(4, 4, 0); sfn(13, 15, 1000); sfn(5, 9, 1);
  smm(3, std::vector<double>(12, 0.1), 3, 9); smm(3, std::vector<double>(3, 1.0), 0, 3); smm(3, std::vector<double>(8, 0.1), -1, 0);
  smm(3, {}, -1, 0); smm(15, std::vector<double>(15 + 225, 0.2), 15, 15 + 15 * 14);
  std::vector<double> u(1000 + 1000 * 1000);   // the bench size, about a quarter of the points candidates
  for (size_t i = 0; i < u.size(); i++) u[i] = (double)((i * 2654435761u) % 1000) / 1000.0;
  int64_t k = 0;
  const int nc = dsh::smm_walk_candidates(1000, u.data(), (int64_t)u.size(), nullptr, nullptr, &k);
  smm(1000, u, nc, k);
  std::printf("host fill functions: ok\n");
  return 0;
}
