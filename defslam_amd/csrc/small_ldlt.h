// Eigen::LDLT<MatrixXd, Lower> restated for a small n x n matrix (column-major, the lower triangle is read): diagonal pivoting by the
// largest |A_ii|, the in-place factor, isPositive(), and solve() with its 1 / DBL_MAX threshold on D.  P and IP are pointers to double
// and int in whichever address space holds the matrix (LDS in the kernels, so the pivot's run-time indices cost no scratch).
#pragma once
#include <float.h>
#include <hip/hip_runtime.h>

template <int n, class P, class IP>
__device__ __forceinline__ bool small_ldlt(P A, IP perm, double* tmp) {
  int sign = 0;
  for (int k = 0; k < n; k++) {
    int p = k;
    double big = fabs(A[k + k * n]);
    for (int i = k + 1; i < n; i++) {
      const double v = fabs(A[i + i * n]);
      if (v > big) { big = v; p = i; }
    }
    perm[k] = p;
    if (p != k) {
      for (int j = 0; j < k; j++) { const double t = A[k + j * n]; A[k + j * n] = A[p + j * n]; A[p + j * n] = t; }
      for (int i = p + 1; i < n; i++) { const double t = A[i + k * n]; A[i + k * n] = A[i + p * n]; A[i + p * n] = t; }
      { const double t = A[k + k * n]; A[k + k * n] = A[p + p * n]; A[p + p * n] = t; }
      for (int i = k + 1; i < p; i++) { const double t = A[i + k * n]; A[i + k * n] = A[p + i * n]; A[p + i * n] = t; }
    }
    const int rs = n - k - 1;
    if (k > 0) {
      double s = 0;
      for (int j = 0; j < k; j++) { tmp[j] = A[j + j * n] * A[k + j * n]; s += A[k + j * n] * tmp[j]; }
      A[k + k * n] -= s;
      for (int j = 0; j < k; j++)
        for (int i = 0; i < rs; i++) A[(k + 1 + i) + k * n] -= A[(k + 1 + i) + j * n] * tmp[j];
    }
    const double akk = A[k + k * n];
    const bool pivot_valid = fabs(akk) > 0.0;
    if (k == 0 && !pivot_valid) {
      for (int j = 0; j < n; j++) perm[j] = j;
      return true;
    }
    if (pivot_valid)
      for (int i = 0; i < rs; i++) A[(k + 1 + i) + k * n] /= akk;
    if (sign == 1) { if (akk < 0) sign = 2; }
    else if (sign == -1) { if (akk > 0) sign = 2; }
    else if (sign == 0) { if (akk > 0) sign = 1; else if (akk < 0) sign = -1; }
  }
  return sign == 1 || sign == 0;
}

template <int n, class P, class IP, class XP>
__device__ __forceinline__ void small_ldlt_solve(P A, IP perm, XP b, XP x) {
  for (int i = 0; i < n; i++) x[i] = b[i];
  for (int k = 0; k < n; k++) { const int p = perm[k]; if (p != k) { const double t = x[k]; x[k] = x[p]; x[p] = t; } }
  for (int j = 0; j < n; j++)
    for (int i = j + 1; i < n; i++) x[i] -= A[i + j * n] * x[j];
  const double tol = 1.0 / DBL_MAX;
  for (int i = 0; i < n; i++) { const double d = A[i + i * n]; if (fabs(d) > tol) x[i] /= d; else x[i] = 0; }
  for (int j = n - 1; j >= 0; j--) {
    double s = x[j];
    for (int i = j + 1; i < n; i++) s -= A[i + j * n] * x[i];
    x[j] = s;
  }
  for (int k = n - 1; k >= 0; k--) { const int p = perm[k]; if (p != k) { const double t = x[k]; x[k] = x[p]; x[p] = t; } }
}
