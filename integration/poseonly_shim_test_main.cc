// CI driver of integration/pose_only_hip.h: the points of a store scene (tests/store_model.py write_scene) and one frame from a second
// file of the driver's own.  The frame's rigid pose-only optimisation runs both ways over two copies of the same stand-in objects:
//   the store way  MapPointStoreHIP + PoseOptimizationStoreHIP: nothing per map point travels
//   the host way   ORB_SLAM2::Optimizer::poseOptimization (Optimizer.cc:236-445, monocular) written out below as loops over the frame's
//                  map points with their positions read from the objects, sums in edge order
// and per way one block is dumped: "way ret n_initial rounds", "iters ..", "trials ..", "bad ..", "chi2 .." (%.17g), "pose .." (%.17g,
// t then q x y z w), "Tcw .." (bit patterns, the frame's pose afterwards), "flags .." (mvbOutlier), then "time_us <wall clock of the host way, the median of host_reps runs>".
// The frame file: "N levels fx fy cx cy", 16 floats of mTcw, `levels` floats of mvInvLevelSigma2, N lines "x y octave id outlier".
//   usage: poseonly_shim_test <scene.txt> <frame.txt> <output.txt> [device [host_reps]]; exit codes: shim_driver.h
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "pose_only_hip.h"
#include "shim_driver.h"
#include "standin_store_scene.h"

using namespace standin;

namespace {

// ---- SE3Quat (Thirdparty/g2o/g2o/types/se3quat.h): a pose is t[3], q[4] (x y z w) ----
void quat_from_R(const double* R, double* q) {          // Eigen::Quaterniond(Matrix3d)
  double t = R[0] + R[4] + R[8];
  if (t > 0.0) {
    t = std::sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[i * 4]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(R[i * 4] - R[j * 4] - R[k * 4] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[k * 3 + j] - R[j * 3 + k]) * t;
    q[j] = (R[j * 3 + i] + R[i * 3 + j]) * t;
    q[k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
  }
}
void quat_unit_pos(double* q) {                         // normalizeRotation
  if (q[3] < 0) for (int i = 0; i < 4; i++) q[i] = -q[i];
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; i++) q[i] /= n;
}
void quat_to_R(const double* q, double* R) {
  const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
  const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
  const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
  const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
void rotate(const double* q, const double* v, double* r) {
  double uv0 = q[1] * v[2] - q[2] * v[1], uv1 = q[2] * v[0] - q[0] * v[2], uv2 = q[0] * v[1] - q[1] * v[0];
  uv0 += uv0; uv1 += uv1; uv2 += uv2;
  const double c0 = q[1] * uv2 - q[2] * uv1, c1 = q[2] * uv0 - q[0] * uv2, c2 = q[0] * uv1 - q[1] * uv0;
  r[0] = (v[0] + q[3] * uv0) + c0; r[1] = (v[1] + q[3] * uv1) + c1; r[2] = (v[2] + q[3] * uv2) + c2;
}
void exp_times(const double* d, const double* pose, double* out) {   // SE3Quat::exp(d) * pose
  const double theta = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  const double Om[9] = {0, -d[2], d[1], d[2], 0, -d[0], -d[1], d[0], 0};
  double Om2[9], Rd[9], V[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double s = 0;
      for (int k = 0; k < 3; k++) s += Om[i * 3 + k] * Om[k * 3 + j];
      Om2[i * 3 + j] = s;
    }
  if (theta < 0.00001) {
    for (int i = 0; i < 9; i++) { Rd[i] = ((i % 4 == 0 ? 1.0 : 0.0) + Om[i]) + Om2[i]; V[i] = Rd[i]; }
  } else {
    const double a = std::sin(theta) / theta, b = (1 - std::cos(theta)) / (theta * theta), c = (theta - std::sin(theta)) / (theta * theta * theta);
    for (int i = 0; i < 9; i++) {
      const double id = (i % 4 == 0) ? 1.0 : 0.0;
      Rd[i] = (id + a * Om[i]) + b * Om2[i];
      V[i] = (id + b * Om[i]) + c * Om2[i];
    }
  }
  double qd[4], td[3], r[3];
  quat_from_R(Rd, qd);
  quat_unit_pos(qd);
  for (int i = 0; i < 3; i++) td[i] = (V[i * 3] * d[3] + V[i * 3 + 1] * d[4]) + V[i * 3 + 2] * d[5];
  rotate(qd, pose, r);
  const double* q = pose + 3;
  double nq[4];
  nq[3] = qd[3] * q[3] - qd[0] * q[0] - qd[1] * q[1] - qd[2] * q[2];
  nq[0] = qd[3] * q[0] + qd[0] * q[3] + qd[1] * q[2] - qd[2] * q[1];
  nq[1] = qd[3] * q[1] + qd[1] * q[3] + qd[2] * q[0] - qd[0] * q[2];
  nq[2] = qd[3] * q[2] + qd[2] * q[3] + qd[0] * q[1] - qd[1] * q[0];
  quat_unit_pos(nq);
  for (int i = 0; i < 3; i++) out[i] = td[i] + r[i];
  for (int i = 0; i < 4; i++) out[3 + i] = nq[i];
}

// ---- Eigen::LDLT<MatrixXd, Lower> for the 6 x 6 system, column-major ----
bool ldlt6(double* A, int* perm) {
  const int n = 6;
  int sign = 0;
  double tmp[n];
  for (int k = 0; k < n; k++) {
    int p = k;
    double big = std::fabs(A[k + k * n]);
    for (int i = k + 1; i < n; i++) {
      const double v = std::fabs(A[i + i * n]);
      if (v > big) { big = v; p = i; }
    }
    perm[k] = p;
    if (p != k) {
      for (int j = 0; j < k; j++) std::swap(A[k + j * n], A[p + j * n]);
      for (int i = p + 1; i < n; i++) std::swap(A[i + k * n], A[i + p * n]);
      std::swap(A[k + k * n], A[p + p * n]);
      for (int i = k + 1; i < p; i++) std::swap(A[i + k * n], A[p + i * n]);
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
    const bool pivot_valid = std::fabs(akk) > 0.0;
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
void ldlt6_solve(const double* A, const int* perm, const double* b, double* x) {
  const int n = 6;
  for (int i = 0; i < n; i++) x[i] = b[i];
  for (int k = 0; k < n; k++) if (perm[k] != k) std::swap(x[k], x[perm[k]]);
  for (int j = 0; j < n; j++)
    for (int i = j + 1; i < n; i++) x[i] -= A[i + j * n] * x[j];
  const double tol = 1.0 / DBL_MAX;
  for (int i = 0; i < n; i++) { const double d = A[i + i * n]; if (std::fabs(d) > tol) x[i] /= d; else x[i] = 0; }
  for (int j = n - 1; j >= 0; j--) {
    double s = x[j];
    for (int i = j + 1; i < n; i++) s -= A[i + j * n] * x[i];
    x[j] = s;
  }
  for (int k = n - 1; k >= 0; k--) if (perm[k] != k) std::swap(x[k], x[perm[k]]);
}

struct Edge {                                           // EdgeSE3ProjectXYZOnlyPose with its level and the error it holds
  int idx;
  double X[3], u, v, w, chi2;
  bool level1;
};
struct Detail {
  int n_initial = 0, rounds = 0, iters[4] = {0, 0, 0, 0}, trials[4] = {0, 0, 0, 0}, bad[4] = {0, 0, 0, 0};
  double chi2[4] = {0, 0, 0, 0}, pose[7] = {0, 0, 0, 0, 0, 0, 1};
};

double edge_error(const Edge& e, const double* pose, const double* K, double* err, double* p) {
  double r[3];
  rotate(pose + 3, e.X, r);
  for (int i = 0; i < 3; i++) p[i] = r[i] + pose[i];
  err[0] = e.u - ((p[0] / p[2]) * K[0] + K[2]);
  err[1] = e.v - ((p[1] / p[2]) * K[1] + K[3]);
  return err[0] * (e.w * err[0]) + err[1] * (e.w * err[1]);
}
double huber(double chi2, double delta, double& rho1) {
  const double dsqr = delta * delta;
  if (chi2 <= dsqr) { rho1 = 1.0; return chi2; }
  const double sq = std::sqrt(chi2);
  rho1 = delta / sq;
  return 2 * sq * delta - dsqr;
}
// computeActiveErrors and activeRobustChi2 at pose: every level-0 edge holds its error afterwards
double active_chi2(std::vector<Edge>& edges, const double* pose, const double* K, bool robust, double delta) {
  double sum = 0, err[2], p[3], rho1;
  for (Edge& e : edges) {
    if (e.level1) continue;
    e.chi2 = edge_error(e, pose, K, err, p);
    sum += robust ? huber(e.chi2, delta, rho1) : e.chi2;
  }
  return sum;
}

// Optimizer::poseOptimization over the stand-in objects
int host_pose_optimization(LmFrame& F, Detail& D) {
  const double delta = (double)(float)std::sqrt(5.991);
  const double K[4] = {F.fx, F.fy, F.cx, F.cy};
  std::vector<Edge> edges;
  for (int i = 0; i < F.N; i++) {                       // :276-315
    LmMapPoint* mp = F.mvpMapPoints[i];
    if (!mp) continue;
    F.mvbOutlier[i] = false;
    Edge e;
    e.idx = i;
    for (int k = 0; k < 3; k++) e.X[k] = mp->pos[k];
    e.u = F.mvKeysUn[i].pt.x; e.v = F.mvKeysUn[i].pt.y;
    e.w = F.mvInvLevelSigma2[F.mvKeysUn[i].octave];
    e.chi2 = 0; e.level1 = false;
    edges.push_back(e);
  }
  double start[7], R0[9];
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) R0[3 * i + j] = F.mTcw[4 * i + j];
    start[i] = F.mTcw[4 * i + 3];
  }
  quat_from_R(R0, start + 3);
  quat_unit_pos(start + 3);
  D.n_initial = (int)edges.size();
  std::copy(start, start + 7, D.pose);
  if (D.n_initial < 3) return 0;                        // :358-359
  double est[7];
  int nBad = 0;
  for (int round = 0; round < 4; round++) {
    const bool robust = round < 3;
    std::copy(start, start + 7, est);                   // :371
    double x[6] = {0, 0, 0, 0, 0, 0}, lambda = 0, ni = 2, cur = 0;
    int n_act = 0, nbad_lm = 0;
    for (const Edge& e : edges) n_act += e.level1 ? 0 : 1;
    for (int it = 0; n_act > 0 && it < 10; it++) {      // optimize(10)
      double H[36] = {0}, b[6] = {0, 0, 0, 0, 0, 0};
      cur = active_chi2(edges, est, K, robust, delta);
      for (Edge& e : edges) {                           // buildSystem
        if (e.level1) continue;
        double err[2], p[3], rho1 = 1.0;
        const double chi2 = edge_error(e, est, K, err, p);
        if (robust) huber(chi2, delta, rho1);
        const double xx = p[0], y = p[1], invz = 1.0 / p[2], invz_2 = invz * invz;
        const double A0[6] = {xx * y * invz_2 * K[0], -(1 + (xx * xx * invz_2)) * K[0], y * invz * K[0], -invz * K[0], 0.0, xx * invz_2 * K[0]};
        const double A1[6] = {(1 + y * y * invz_2) * K[1], -xx * y * invz_2 * K[1], -xx * invz * K[1], 0.0, -invz * K[1], y * invz_2 * K[1]};
        const double W = rho1 * e.w;
        for (int r = 0; r < 6; r++) {
          const double a0 = A0[r] * W, a1 = A1[r] * W;
          for (int c = 0; c <= r; c++) H[r + 6 * c] += a0 * A0[c] + a1 * A1[c];
          b[r] -= ((rho1 * A0[r]) * e.w) * err[0] + ((rho1 * A1[r]) * e.w) * err[1];
        }
      }
      for (int r = 0; r < 6; r++)
        for (int c = 0; c < r; c++) H[c + 6 * r] = H[r + 6 * c];
      const double ini = cur;
      if (it == 0) {
        double m = 0;
        for (int r = 0; r < 6; r++) m = std::max(std::fabs(H[7 * r]), m);
        lambda = 1e-5 * m; ni = 2; nbad_lm = 0;
      }
      double rho = 0;
      int q = 0;
      do {
        double Hs[36], trial[7];
        int perm[6];
        std::copy(H, H + 36, Hs);
        for (int r = 0; r < 6; r++) Hs[7 * r] += lambda;
        const bool ok = ldlt6(Hs, perm);
        if (ok) ldlt6_solve(Hs, perm, b, x);
        exp_times(x, est, trial);
        double tmp = active_chi2(edges, trial, K, robust, delta);
        if (!ok) tmp = DBL_MAX;
        double scale = 0;
        for (int j = 0; j < 6; j++) scale += x[j] * (lambda * x[j] + b[j]);
        scale += 1e-3;
        rho = (cur - tmp) / scale;
        if (rho > 0 && std::isfinite(tmp)) {
          double alpha = 1. - std::pow((2 * rho - 1), 3);
          alpha = std::min(alpha, 2. / 3.);
          lambda *= std::max(1. / 3., alpha);
          ni = 2;
          cur = tmp;
          std::copy(trial, trial + 7, est);
        } else {
          lambda *= ni;
          ni *= 2;
        }
        q++;
      } while (rho < 0 && q < 10);
      D.iters[round]++;
      D.trials[round] += q;
      if (q == 10 || rho == 0) break;
      if ((ini - cur) * 1e3 < ini) nbad_lm++; else nbad_lm = 0;
      if (nbad_lm >= 3) break;
    }
    nBad = 0;
    for (Edge& e : edges) {                             // :376-403
      double err[2], p[3];
      if (F.mvbOutlier[e.idx]) e.chi2 = edge_error(e, est, K, err, p);
      const float chi2 = (float)e.chi2;
      if (chi2 > 5.991f) { F.mvbOutlier[e.idx] = true; e.level1 = true; nBad++; }
      else { F.mvbOutlier[e.idx] = false; e.level1 = false; }
    }
    D.bad[round] = nBad;
    D.chi2[round] = cur;
    D.rounds++;
    if (edges.size() < 10) break;                       // :434-435
  }
  std::copy(est, est + 7, D.pose);
  double R[9];
  float T[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
  quat_to_R(est + 3, R);
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) T[4 * i + j] = (float)R[3 * i + j];
    T[4 * i + 3] = (float)est[i];
  }
  F.SetPose(T);                                         // :441-442
  return D.n_initial - nBad;
}

bool read_frame(std::istream& in, StoreScene& sc, LmFrame& F) {
  int levels = 0;
  in >> F.N >> levels >> F.fx >> F.fy >> F.cx >> F.cy;
  if (!in || F.N < 0 || levels < 1) return false;
  for (float& t : F.mTcw) in >> t;
  F.SetPose(F.mTcw);
  F.mnScaleLevels = levels;
  F.mvInvLevelSigma2.resize(levels);
  for (float& s : F.mvInvLevelSigma2) in >> s;
  F.mvKeysUn.resize(F.N);
  F.mvpMapPoints.assign(F.N, nullptr);
  F.mvbOutlier.assign(F.N, false);
  for (int i = 0; i < F.N; i++) {
    int id, flag;
    in >> F.mvKeysUn[i].pt.x >> F.mvKeysUn[i].pt.y >> F.mvKeysUn[i].octave >> id >> flag;
    if (!in || id < -1 || id >= sc.P) return false;
    F.mvpMapPoints[i] = id >= 0 ? &sc.pts[id] : nullptr;
    F.mvbOutlier[i] = flag != 0;
  }
  F.mvKeys = F.mvKeysUn;
  return (bool)in;
}

void dump(std::FILE* o, const char* way, int ret, const Detail& D, const LmFrame& F) {
  std::fprintf(o, "%s %d %d %d\niters", way, ret, D.n_initial, D.rounds);
  for (int r = 0; r < 4; r++) std::fprintf(o, " %d", D.iters[r]);
  std::fprintf(o, "\ntrials");
  for (int r = 0; r < 4; r++) std::fprintf(o, " %d", D.trials[r]);
  std::fprintf(o, "\nbad");
  for (int r = 0; r < 4; r++) std::fprintf(o, " %d", D.bad[r]);
  std::fprintf(o, "\nchi2");
  for (int r = 0; r < 4; r++) std::fprintf(o, " %.17g", D.chi2[r]);
  std::fprintf(o, "\npose");
  for (int i = 0; i < 7; i++) std::fprintf(o, " %.17g", D.pose[i]);
  std::fprintf(o, "\nTcw");
  for (int i = 0; i < 16; i++) {
    uint32_t u;
    std::memcpy(&u, &F.mTcw[i], 4);
    std::fprintf(o, " %u", u);
  }
  std::fprintf(o, "\nflags");
  for (int i = 0; i < F.N; i++) std::fprintf(o, " %d", F.mvbOutlier[i] ? 1 : 0);
  std::fprintf(o, "\n");
}

}  // namespace

static int drive(const DriverArgs& arg) {
  StoreScene dev, host;                     // two copies of the same objects, one per way
  LmFrame Fd, Fh;
  for (int w = 0; w < 2; w++) {
    std::ifstream in(arg.in[0]), in2(arg.in[1]);
    StoreScene& sc = w ? host : dev;
    if (!sc.read(in)) return driver_bad_input(arg.in[0]);
    if (!read_frame(in2, sc, w ? Fh : Fd)) return driver_bad_input(arg.in[1]);
  }
  {
    defslam_hip::MapPointStoreHIP<LmKeyFrame, LmMapPoint> store(arg.ctx, 64, 2, 64);   // small on purpose: the store grows
    if (!dev.fill(store)) return driver_fail(arg.ctx, "filling the store");
    dsh_pose_only_problem p;
    const int ret = defslam_hip::PoseOptimizationStoreHIP(Fd, store, &p);
    if (ret < 0) return driver_fail(arg.ctx, "PoseOptimizationStoreHIP");
    Detail D;
    D.n_initial = p.n_initial; D.rounds = p.rounds;
    for (int r = 0; r < 4; r++) { D.iters[r] = p.iters[r]; D.trials[r] = p.trials[r]; D.bad[r] = p.bad[r]; D.chi2[r] = p.chi2[r]; }
    std::copy(p.pose, p.pose + 7, D.pose);
    dump(arg.out, "dev", ret, D, Fd);
  }
  // the host way; with a repeat count behind the device it runs that often on fresh copies of the frame and reports the median
  const int reps = arg.n_extra > 0 ? std::max(1, std::atoi(arg.extra[0])) : 1;
  std::vector<double> us(reps);
  Detail H;
  LmFrame F;
  int ret = 0;
  for (int r = 0; r < reps; r++) {
    F = Fh;
    H = Detail();
    const auto t0 = std::chrono::steady_clock::now();
    ret = host_pose_optimization(F, H);
    us[r] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  }
  std::sort(us.begin(), us.end());
  dump(arg.out, "host", ret, H, F);
  std::fprintf(arg.out, "time_us %.1f\n", us[reps / 2]);
  return 0;
}

int main(int argc, char** argv) { return run_driver(argc, argv, 2, drive); }
