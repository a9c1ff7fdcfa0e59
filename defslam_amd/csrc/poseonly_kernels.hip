// The rigid pose-only optimisation of a frame (ORB_SLAM2::Optimizer::poseOptimization, Thirdparty/ORBSLAM_2/src/Optimizer.cc:236-445,
// monocular branch) as one kernel: one workgroup of PO_BLOCK threads per problem runs the gather of the positions from the store,
// the four rounds of g2o's Levenberg-Marquardt with their classifications, and the float32 conversion of the pose.  The semantics
// are stated above dsh_track_pose_only in include/defslam_hip.h, the design in DESIGN 4.6.
//
// Summation order (the one place where the result depends on more than the inputs' values): thread t of the workgroup adds the
// contributions of the key points t, t + PO_BLOCK, t + 2 PO_BLOCK, ... in ascending order to an accumulator that starts at +0;
// within a wavefront a tree over the 64 lanes follows, lane l taking lane l + 32, then l + 16, 8, 4, 2, 1; the four wavefronts'
// sums are then added in ascending order starting from +0.  A key point that holds no point, or whose edge is at level 1, adds
// nothing.  No floating-point atomics, no FMA contraction (the Makefile compiles this file with -ffp-contract=off).
#define PO_KERNEL_SOURCE
#include <float.h>
#include <hip/hip_runtime.h>

#include "poseonly_problem.h"
#include "se3_device.h"
#include "small_ldlt.h"

namespace {

constexpr int PO_WAVES = PO_BLOCK / 64;
constexpr int PO_NSUM = 28;   // 21 entries of the lower triangle of H (row i, column j <= i at i (i + 1) / 2 + j), 6 of -b, the robust chi2

struct PoShared {
  double red[PO_WAVES * PO_NSUM], sum[PO_NSUM];
  double start[7], est[7], trial[7];   // the input pose, the round's estimate, the last trial evaluated
  double K[4];
  double H[36], Hs[36], b[6], x[6];    // column-major; the factorisation reads the lower triangle
  int perm[6];
  int count, more, stop;
};

// S is the kernel's one __shared__ object and every function below is inlined into the kernel, so each access to it is compiled as an
// LDS access (ds_*), the factorisation's run-time indices included; nothing reaches it through a second, differently typed pointer.

// Deterministic sum over the workgroup of NV values per thread, in the order stated at the top; valid in S.sum[0 .. NV) for every
// thread after the call.
template <int NV>
__device__ __forceinline__ void po_block_sum(const double* v, PoShared& S) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; i++) {
    double s = v[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) S.red[wave * NV + i] = s;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double s = 0;
    for (int w = 0; w < PO_WAVES; w++) s += S.red[w * NV + threadIdx.x];
    S.sum[threadIdx.x] = s;
  }
  __syncthreads();
}

__device__ __forceinline__ int po_block_count(int n, PoShared& S) {
  if (threadIdx.x == 0) S.count = 0;
  __syncthreads();
  if (n) atomicAdd(&S.count, n);
  __syncthreads();
  const int total = S.count;
  __syncthreads();
  return total;
}

struct PoEdge {
  double X0, X1, X2, u, v, w;
};

__device__ __forceinline__ PoEdge po_load_edge(PO_G const float* edge, int i) {
  PO_G const float2* e = (PO_G const float2*)(edge + 6 * (size_t)i);
  const float2 a = e[0], b = e[1], c = e[2];
  PoEdge E;
  E.X0 = (double)a.x; E.X1 = (double)a.y; E.X2 = (double)b.x; E.u = (double)b.y; E.v = (double)c.x; E.w = (double)c.y;
  return E;
}

// EdgeSE3ProjectXYZOnlyPose::computeError at pose (t, q) and chi2 = e' Omega e; p = the point in the camera frame
__device__ __forceinline__ double po_error(const double* pose, const double* K, const PoEdge& E, double& e0, double& e1, double& px, double& py,
                                           double& pz) {
  double r0, r1, r2;
  se3_rotate(pose + 3, E.X0, E.X1, E.X2, r0, r1, r2);
  px = r0 + pose[0]; py = r1 + pose[1]; pz = r2 + pose[2];
  e0 = E.u - ((px / pz) * K[0] + K[2]);
  e1 = E.v - ((py / pz) * K[1] + K[3]);
  return e0 * (E.w * e0) + e1 * (E.w * e1);
}

// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91): rho[0]; rho1 = rho[1]
__device__ __forceinline__ double po_huber(double chi2, double delta, double dsqr, double& rho1) {
  if (chi2 <= dsqr) { rho1 = 1.0; return chi2; }
  const double sqrte = sqrt(chi2);
  rho1 = delta / sqrte;
  return 2 * sqrte * delta - dsqr;
}

}  // namespace

__global__ __launch_bounds__(PO_BLOCK) void po_solve_kernel(PoBatch bt) {
  __shared__ PoShared S;
  const int tid = threadIdx.x;
  PO_G const PoProb& P = bt.prob[blockIdx.x];
  const int N = P.N, kp0 = P.kp0;
  PO_G float* edge = bt.edge + 6 * (size_t)kp0;
  PO_G uint8_t* state = bt.state + kp0;
  const double delta = (double)(float)sqrt(5.991), dsqr = delta * delta;

  // the edges, gathered once: the store's position by id, the key point, the information of its octave (Optimizer.cc:276-315)
  int held = 0;
  for (int i = tid; i < N; i += PO_BLOCK) {
    const int id = bt.ids[kp0 + i];
    if (id < 0) { state[i] = PO_NOT_HELD; continue; }
    held++;
    state[i] = 0;
    PO_G float2* e = (PO_G float2*)(edge + 6 * (size_t)i);
    PO_G const float* X = bt.xyz + 3 * (size_t)id;
    const float2 uv = ((PO_G const float2*)bt.kp)[kp0 + i];
    e[0] = make_float2(X[0], X[1]);
    e[1] = make_float2(X[2], uv.x);
    e[2] = make_float2(uv.y, bt.sig[P.sig0 + bt.octave[kp0 + i]]);
  }
  if (tid == 0) {
    float T[16];
    for (int i = 0; i < 16; i++) T[i] = P.Tcw[i];
    double pose[7];
    se3_from_f32_matrix(T, pose);
    for (int i = 0; i < 7; i++) { S.start[i] = pose[i]; S.est[i] = pose[i]; S.trial[i] = pose[i]; }
    for (int i = 0; i < 4; i++) S.K[i] = (double)P.K[i];
  }
  const int n_initial = po_block_count(held, S);   // its barriers also publish the pose and the edges (each thread reads its own)
  PO_G PoResult& out = bt.res[blockIdx.x];
  if (tid == 0) {
    out.n_initial = n_initial; out.n_bad = 0; out.n_good = 0; out.rounds = 0;
    for (int r = 0; r < 4; r++) { out.iters[r] = 0; out.trials[r] = 0; out.bad[r] = 0; out.chi2[r] = 0.0; }
  }
  double K[4];
  for (int i = 0; i < 4; i++) K[i] = S.K[i];

  int rounds = 0, nbad = 0;
  if (n_initial >= 3) {
    for (int round = 0; round < 4; round++) {
      const bool robust = round < 3;   // setRobustKernel(0) after round index 2 (:401-402)
      // the controller's state: lane 0's copy is the one that counts
      double lambda = 0.0, ni = 2.0, cur = 0.0, ini = 0.0, rho = 0.0;
      int nbad_lm = 0, q = 0, iters = 0, trials = 0;
      if (tid == 0) {
        for (int i = 0; i < 7; i++) S.est[i] = S.start[i];   // vSE3->setEstimate(toSE3Quat(mTcw)) (:371)
        for (int i = 0; i < 6; i++) S.x[i] = 0.0;
      }
      __syncthreads();
      const bool ran = n_initial - nbad > 0;   // a round without a level-0 edge does not optimise (sparse_optimizer.cpp:405-409)
      if (ran) {
        for (int it = 0; it < 10; it++) {
          // computeActiveErrors, activeRobustChi2 and buildSystem at the estimate
          double pose[7], acc[PO_NSUM];
          for (int i = 0; i < 7; i++) pose[i] = S.est[i];
          for (int i = 0; i < PO_NSUM; i++) acc[i] = 0.0;
          for (int i = tid; i < N; i += PO_BLOCK) {
            if (state[i] != 0) continue;
            const PoEdge E = po_load_edge(edge, i);
            double e0, e1, x, y, z;
            const double chi2 = po_error(pose, K, E, e0, e1, x, y, z);
            double rho1 = 1.0;
            const double rho0 = robust ? po_huber(chi2, delta, dsqr, rho1) : chi2;
            // EdgeSE3ProjectXYZOnlyPose::linearizeOplus (types_six_dof_expmap.cpp:266-288)
            const double invz = 1.0 / z, invz_2 = invz * invz;
            const double A0[6] = {x * y * invz_2 * K[0], -(1 + (x * x * invz_2)) * K[0], y * invz * K[0], -invz * K[0], 0.0, x * invz_2 * K[0]};
            const double A1[6] = {(1 + y * y * invz_2) * K[1], -x * y * invz_2 * K[1], -x * invz * K[1], 0.0, -invz * K[1], y * invz_2 * K[1]};
            // BaseUnaryEdge::constructQuadraticForm (base_unary_edge.hpp:43-72): A' (rho1 Omega) A and rho1 A' Omega e
            const double W = rho1 * E.w;
#pragma unroll
            for (int r = 0; r < 6; r++) {
              const double a0 = A0[r] * W, a1 = A1[r] * W;
#pragma unroll
              for (int c = 0; c <= r; c++) acc[r * (r + 1) / 2 + c] += a0 * A0[c] + a1 * A1[c];
              acc[21 + r] += ((rho1 * A0[r]) * E.w) * e0 + ((rho1 * A1[r]) * E.w) * e1;
            }
            acc[27] += rho0;
          }
          po_block_sum<PO_NSUM>(acc, S);
          if (tid == 0) {
            for (int r = 0; r < 6; r++)
              for (int c = 0; c <= r; c++) { S.H[r + 6 * c] = S.sum[r * (r + 1) / 2 + c]; S.H[c + 6 * r] = S.sum[r * (r + 1) / 2 + c]; }
            for (int r = 0; r < 6; r++) S.b[r] = -S.sum[21 + r];
            cur = S.sum[27];
            ini = cur;
            if (it == 0) {   // computeLambdaInit (optimization_algorithm_levenberg.cpp:166-180)
              double m = 0.0;
              for (int r = 0; r < 6; r++) m = fmax(fabs(S.H[7 * r]), m);
              lambda = 1e-5 * m;
              ni = 2.0;
              nbad_lm = 0;
            }
            q = 0;
          }
          for (;;) {
            bool ok = false;
            if (tid == 0) {   // setLambda, LinearSolverDense::solve, the update on top of the pushed estimate
              for (int i = 0; i < 36; i++) S.Hs[i] = S.H[i];
              for (int r = 0; r < 6; r++) S.Hs[7 * r] += lambda;
              double tmp[6];
              ok = small_ldlt<6>(S.Hs, S.perm, tmp);
              if (ok) small_ldlt_solve<6>(S.Hs, S.perm, S.b, S.x);   // a failed factor leaves x as it was
              double d[6], p[7], o[7];
              for (int i = 0; i < 6; i++) d[i] = S.x[i];
              for (int i = 0; i < 7; i++) p[i] = S.est[i];
              se3_exp_times(d, p, o);
              for (int i = 0; i < 7; i++) S.trial[i] = o[i];
            }
            __syncthreads();
            // computeActiveErrors and activeRobustChi2 at the trial
            for (int i = 0; i < 7; i++) pose[i] = S.trial[i];
            double chi[1] = {0.0};
            for (int i = tid; i < N; i += PO_BLOCK) {
              if (state[i] != 0) continue;
              const PoEdge E = po_load_edge(edge, i);
              double e0, e1, x, y, z, rho1;
              const double chi2 = po_error(pose, K, E, e0, e1, x, y, z);
              chi[0] += robust ? po_huber(chi2, delta, dsqr, rho1) : chi2;
            }
            po_block_sum<1>(chi, S);
            if (tid == 0) {   // optimization_algorithm_levenberg.cpp:124-149
              const double tmp = ok ? S.sum[0] : DBL_MAX;
              double scale = 0.0;
              rho = cur - tmp;
              for (int j = 0; j < 6; j++) scale += S.x[j] * (lambda * S.x[j] + S.b[j]);
              scale += 1e-3;
              rho /= scale;
              if (rho > 0 && isfinite(tmp)) {
                double alpha = 1. - pow((2 * rho - 1), 3);
                alpha = fmin(alpha, 2. / 3.);
                const double scaleFactor = fmax(1. / 3., alpha);
                lambda *= scaleFactor;
                ni = 2;
                cur = tmp;
                for (int i = 0; i < 7; i++) S.est[i] = S.trial[i];
              } else {
                lambda *= ni;
                ni *= 2;
              }
              q++;
              S.more = rho < 0 && q < 10;
            }
            __syncthreads();
            if (!S.more) break;
          }
          if (tid == 0) {   // :151-163
            iters++;
            trials += q;
            int stop = 0;
            if (q == 10 || rho == 0) stop = 1;
            else {
              if ((ini - cur) * 1e3 < ini) nbad_lm++;
              else nbad_lm = 0;
              if (nbad_lm >= 3) stop = 1;
            }
            S.stop = stop;
          }
          __syncthreads();
          if (S.stop) break;
        }
      }
      // classification (:376-403): an outlier's error is recomputed at the estimate, an inlier keeps that of the last trial evaluated
      double pe[7], pt[7];
      for (int i = 0; i < 7; i++) { pe[i] = S.est[i]; pt[i] = S.trial[i]; }
      int bad = 0;
      for (int i = tid; i < N; i += PO_BLOCK) {
        const int st = state[i];
        if (st == PO_NOT_HELD) continue;
        const PoEdge E = po_load_edge(edge, i);
        double e0, e1, x, y, z;
        const float chi2 = (float)po_error(st ? pe : pt, K, E, e0, e1, x, y, z);
        const int o = chi2 > 5.991f ? 1 : 0;
        state[i] = (uint8_t)o;
        bad += o;
      }
      nbad = po_block_count(bad, S);
      if (tid == 0) { out.iters[round] = iters; out.trials[round] = trials; out.bad[round] = nbad; out.chi2[round] = cur; }
      rounds++;
      if (n_initial < 10) break;   // optimizer.edges().size() < 10 counts every edge (:434-435)
    }
  }
  if (tid == 0) {
    double pose[7];
    float T[16];
    for (int i = 0; i < 7; i++) pose[i] = S.est[i];
    se3_to_f32_matrix(pose, T);
    // the early return leaves the frame's pose alone (:358-359)
    for (int i = 0; i < 16; i++) out.Tcw_out[i] = rounds ? T[i] : P.Tcw[i];
    for (int i = 0; i < 7; i++) out.pose[i] = pose[i];
    out.rounds = rounds;
    out.n_bad = nbad;
    out.n_good = rounds ? n_initial - nbad : 0;
  }
}

extern "C" hipError_t po_launch(const PoBatch& b, hipStream_t st) {
  if (b.B <= 0) return hipSuccess;
  hipLaunchKernelGGL(po_solve_kernel, dim3((unsigned)b.B), dim3(PO_BLOCK), 0, st, b);
  return hipGetLastError();
}
