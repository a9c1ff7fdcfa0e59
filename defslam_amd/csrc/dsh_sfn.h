// The stages of Shape from Normals (dsh_sfn.cpp) for the callers that hold their sites on the device already: dsh_keyframe_sfn
// (dsh_surfstore.cpp) runs them on the sites where its selection left them, as dsh_register.h lets dsh_keyframe_register run the
// registration on its clouds.
#pragma once
#include <cstdint>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "dsh_diffdb.h"

namespace dsh {

// Inputs that lie on the device and outputs that stay there.  LIFETIME: slices of the context's scratch, or arrays of a store; the
// stages take further scratch slices and never call dsh_enter, so the pointers hold until the caller returns.
struct SfnDevice {
  const double *u, *v;          // n sites
  const float* normals;         // n x 3
  const double *u_all, *v_all;  // n_all key points
  float* pts;                   // n_all x 3: the surface points are evaluated into it; written only when *ok becomes 1
  double* ctrl;                 // nptsu * nptsv: the scaled control points; written only when *ok becomes 1
};

// The body of dsh_sfn_estimate / dsh_sfn_estimate_db behind their checks and the device gate (the caller has called dsh_enter, and
// nptsu * nptsv <= 512).  With dev, the host arrays u, v, normals, u_all, v_all and the database are not read; ctrl is a host array of
// nptsu * nptsv doubles either way, ctrl_raw and pts may be null.  Without dev, the calls, their order and their operands are what
// they were: the same bytes come out.
int sfn_stages(dsh_ctx_base* c, const dsh_bbs* bbs, int n, const double* u, const double* v, const float* normals, const dsh_diffdb* ndb, const int32_t* sel,
               double bending_weight, double mean_depth, int n_all, const double* u_all, const double* v_all, const SfnDevice* dev, double* ctrl_raw,
               double* ctrl, float* pts, int32_t* ok);

// The same for Warps::Warp::initialize: dsh_keyframe_warp_pair (dsh_warppair.cpp) initialises on the matches its gather left on the
// device.  The constant operands travel in the caller's own upload block (a call stages one block between two synchronisations):
// bend = the N x N matrix of bbs_bending_dense(bbs, lambda), ones = N ones.
struct WarpInitDevice {
  const float *kp1, *kp2;       // P x 2 each
  const double *bend, *ones;
  // set by the stages: x (2 N control points) and the 32 scalars of the solve behind it; nothing comes down, nothing is waited for
  double *x, *scal;
};

// The body of dsh_warp_initialize behind its checks and the device gate (nptsu * nptsv <= 512, P > 0).  With dev, kp1, kp2, lambda, x
// and ok are not read or written.  Without dev, the calls, their order and their operands are what they were.
int warp_init_stages(dsh_ctx_base* c, const dsh_bbs* bbs, int P, const float* kp1, const float* kp2, double lambda, WarpInitDevice* dev, double* x, int32_t* ok);

}  // namespace dsh
