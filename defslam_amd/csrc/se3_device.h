// g2o's SE3Quat as the pose-only kernel needs it (Thirdparty/g2o/g2o/types/se3quat.h): a pose is t[3], q[4] (x y z w) in seven doubles.
// The rotation-matrix conversions are Eigen's (Quaterniond(R), toRotationMatrix), the exponential is SE3Quat::exp (:223-257), the
// product operator* (:104-110).  Expression order as written there; compiled without FMA contraction.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void se3_quat_to_R(const double* q, double* R) {
  const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
  const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
  const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
  const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
  R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

// Eigen::Quaterniond(R): from the trace when it is positive, else from the largest diagonal entry
__device__ __forceinline__ void se3_quat_from_R(const double* R, double* q) {
  double t = R[0] + R[4] + R[8];
  if (t > 0.0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[7] - R[5]) * t;
    q[1] = (R[2] - R[6]) * t;
    q[2] = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[i * 4]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrt(R[i * 4] - R[j * 4] - R[k * 4] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[k * 3 + j] - R[j * 3 + k]) * t;
    q[j] = (R[j * 3 + i] + R[i * 3 + j]) * t;
    q[k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
  }
}

// SE3Quat::normalizeRotation (:280-285)
__device__ __forceinline__ void se3_quat_unit_pos(double* q) {
  if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
  const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  q[0] /= nrm; q[1] /= nrm; q[2] /= nrm; q[3] /= nrm;
}

// q (x) v, Eigen's QuaternionBase::_transformVector: v + w * uv + qv x uv with uv = 2 (qv x v)
__device__ __forceinline__ void se3_rotate(const double* q, double v0, double v1, double v2, double& r0, double& r1, double& r2) {
  double uv0 = q[1] * v2 - q[2] * v1, uv1 = q[2] * v0 - q[0] * v2, uv2 = q[0] * v1 - q[1] * v0;
  uv0 += uv0; uv1 += uv1; uv2 += uv2;
  const double c0 = q[1] * uv2 - q[2] * uv1, c1 = q[2] * uv0 - q[0] * uv2, c2 = q[0] * uv1 - q[1] * uv0;
  r0 = (v0 + q[3] * uv0) + c0;
  r1 = (v1 + q[3] * uv1) + c1;
  r2 = (v2 + q[3] * uv2) + c2;
}

// Converter::toSE3Quat of a float32 4x4 row-major matrix: SE3Quat(R, t) with the entries widened to double
__device__ __forceinline__ void se3_from_f32_matrix(const float* T, double* pose) {
  double R[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[3 * i + j] = (double)T[4 * i + j];
  se3_quat_from_R(R, pose + 3);
  se3_quat_unit_pos(pose + 3);
  for (int i = 0; i < 3; i++) pose[i] = (double)T[4 * i + 3];
}

// Converter::toCvMat(SE3Quat): to_homogeneous_matrix rounded to float32
__device__ __forceinline__ void se3_to_f32_matrix(const double* pose, float* T) {
  double R[9];
  se3_quat_to_R(pose + 3, R);
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) T[4 * i + j] = (float)R[3 * i + j];
    T[4 * i + 3] = (float)pose[i];
  }
  T[12] = 0.0f; T[13] = 0.0f; T[14] = 0.0f; T[15] = 1.0f;
}

// out = SE3Quat::exp(d) * pose, d = [omega, upsilon] (VertexSE3Expmap::oplusImpl, types_six_dof_expmap.h:73-76)
__device__ __forceinline__ void se3_exp_times(const double* d, const double* pose, double* out) {
  const double om0 = d[0], om1 = d[1], om2 = d[2];
  const double theta = sqrt(om0 * om0 + om1 * om1 + om2 * om2);
  const double Om[9] = {0, -om2, om1, om2, 0, -om0, -om1, om0, 0};
  double Om2[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double s = 0;
      for (int k = 0; k < 3; k++) s += Om[i * 3 + k] * Om[k * 3 + j];
      Om2[i * 3 + j] = s;
    }
  double Rd[9], V[9];
  if (theta < 0.00001) {
    for (int i = 0; i < 9; i++) { Rd[i] = ((i % 4 == 0 ? 1.0 : 0.0) + Om[i]) + Om2[i]; V[i] = Rd[i]; }
  } else {
    const double a = sin(theta) / theta;
    const double b = (1 - cos(theta)) / (theta * theta);
    const double c = (theta - sin(theta)) / (theta * theta * theta);
    for (int i = 0; i < 9; i++) {
      const double id = (i % 4 == 0) ? 1.0 : 0.0;
      Rd[i] = (id + a * Om[i]) + b * Om2[i];
      V[i] = (id + b * Om[i]) + c * Om2[i];
    }
  }
  double qd[4], td[3];
  se3_quat_from_R(Rd, qd);
  se3_quat_unit_pos(qd);
  for (int i = 0; i < 3; i++) td[i] = (V[i * 3] * d[3] + V[i * 3 + 1] * d[4]) + V[i * 3 + 2] * d[5];
  double r0, r1, r2;
  se3_rotate(qd, pose[0], pose[1], pose[2], r0, r1, r2);
  const double* q = pose + 3;
  double nq[4];
  nq[3] = qd[3] * q[3] - qd[0] * q[0] - qd[1] * q[1] - qd[2] * q[2];
  nq[0] = qd[3] * q[0] + qd[0] * q[3] + qd[1] * q[2] - qd[2] * q[1];
  nq[1] = qd[3] * q[1] + qd[1] * q[3] + qd[2] * q[0] - qd[0] * q[2];
  nq[2] = qd[3] * q[2] + qd[2] * q[3] + qd[0] * q[1] - qd[1] * q[0];
  se3_quat_unit_pos(nq);
  out[0] = td[0] + r0; out[1] = td[1] + r1; out[2] = td[2] + r2;
  out[3] = nq[0]; out[4] = nq[1]; out[5] = nq[2]; out[6] = nq[3];
}
