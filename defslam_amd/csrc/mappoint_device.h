// Device functions of MapPoint::UpdateNormalAndDepth (Thirdparty/ORBSLAM_2/src/MapPoint.cc:348-391) that more than one kernel file
// uses: mappoint_kernels.hip (dsh_mappoint_update) and tmplswitch_kernels.hip (the new points of dsh_template_switch, one observation
// each).  The arithmetic is the one include/defslam_hip.h states for dsh_mappoint_update; a file that includes this header is compiled
// without FMA contraction.
#pragma once
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "mappoint_problem.h"

// one term of UpdateNormalAndDepth's loop (MapPoint.cc:370-374): normali = mWorldPos - Owi, alpha = (float)(1.0 / cv::norm(normali));
// cv::scaleAdd adds normali * alpha to the running sum
__device__ __forceinline__ void normal_term(const MpuSlot& s, float x, float y, float z, float& tx, float& ty, float& tz) {
  const float nx = x - s.Ow[0], ny = y - s.Ow[1], nz = z - s.Ow[2];
  const double nrm = sqrt((double)nx * (double)nx + (double)ny * (double)ny + (double)nz * (double)nz);
  const float a = (float)(1.0 / nrm);
  tx = nx * a;
  ty = ny * a;
  tz = nz * a;
}

// mNormalVector = normal / n (MapPoint.cc:389) into nv[3] and the depth range (:379-388) into mx, mn, from the sum (sx, sy, sz) over the
// M observations, the reference keyframe r and its scale factors at the reference key point's level and at the last level
__device__ __forceinline__ void mp_geometry(int M, float sx, float sy, float sz, const MpuSlot& r, float x, float y, float z, float sf_level,
                                            float sf_last, float* nv, float& mx, float& mn) {
  if (M > 1) {
    const float a = (float)(1.0 / (double)M);   // Mat::convertTo(scale 1.0 / n): cvt_32f's src * a + b with b = 0
    nv[0] = sx * a + 0.0f;
    nv[1] = sy * a + 0.0f;
    nv[2] = sz * a + 0.0f;
  } else {   // n == 1: cv::add(normal, Scalar(0))
    nv[0] = sx + 0.0f;
    nv[1] = sy + 0.0f;
    nv[2] = sz + 0.0f;
  }
  const float px = x - r.Ow[0], py = y - r.Ow[1], pz = z - r.Ow[2];
  const float dist = (float)sqrt((double)px * (double)px + (double)py * (double)py + (double)pz * (double)pz);
  mx = dist * sf_level;
  mn = mx / sf_last;
}
