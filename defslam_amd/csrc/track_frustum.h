// Frame::isInFrustum(pMP, 0.5) (Thirdparty/ORBSLAM_2/src/Frame.cc:338-390) on the device: the ONE statement of the test, shared by the
// local-map search (track_kernels.hip, trk_search_kernel) and the frustum count of dsh_track_close_frame (trackclose_kernels.hip).
// Arithmetic as include/defslam_hip.h states it for the tracking searches.  No FMA contraction: the reference's float32 expression order
// is kept, so this header switches contraction off for the rest of the translation unit that includes it.
#pragma once
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "track_problem.h"

// x3Dc = Rcw * x3Dw + tcw of a float cv::Mat: the three products summed in float32 in row order, tcw added in double and
// rounded once (OpenCV's gemm for 3-element operands accumulates in the element type and adds C in double)
__device__ __forceinline__ float trk_cam_coord(const TrkProb& P, int k, float x, float y, float z) {
  const float s = P.R[3 * k] * x + P.R[3 * k + 1] * y + P.R[3 * k + 2] * z;
  return (float)((double)s + (double)P.t[k]);
}

// what the test leaves behind for MapPoint::PredictScale and the search window
struct TrkView {
  float u, v;      // mTrackProjX, mTrackProjY
  float vc;        // mTrackViewCos
  float dist;      // cv::norm(P - Ow)
};

// Point (x, y, z) with normal (nx, ny, nz) at the pose of P: in front of the camera, inside the image bounds, viewing cosine >= 0.5.
// No distance-range test (DefSLAM computes the range and never uses it).  A projection that is NaN (a point on the camera plane) is not
// in view.  Every lane may call it; w is filled whatever the answer.
__device__ __forceinline__ bool trk_in_frustum(const TrkProb& P, float x, float y, float z, float nx, float ny, float nz, TrkView& w) {
  bool live = true;
  const float PcX = trk_cam_coord(P, 0, x, y, z), PcY = trk_cam_coord(P, 1, x, y, z), PcZ = trk_cam_coord(P, 2, x, y, z);
  if (PcZ < 0.0f) live = false;
  const float invz = 1.0f / PcZ;
  w.u = P.fx * PcX * invz + P.cx;
  w.v = P.fy * PcY * invz + P.cy;
  if (w.u < P.minX || w.u > P.maxX) live = false;
  if (w.v < P.minY || w.v > P.maxY) live = false;
  const float POx = x - P.Ow[0], POy = y - P.Ow[1], POz = z - P.Ow[2];
  w.dist = (float)sqrt((double)POx * (double)POx + (double)POy * (double)POy + (double)POz * (double)POz);   // cv::norm
  const double dot = (double)POx * (double)nx + (double)POy * (double)ny + (double)POz * (double)nz;         // cv::Mat::dot
  w.vc = (float)(dot / (double)w.dist);
  if (w.vc < 0.5f) live = false;
  if (w.u != w.u || w.v != w.v) live = false;   // a point on the camera plane: the reference's window arithmetic is undefined there
  return live;
}
