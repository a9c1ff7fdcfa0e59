// The stages of the batched Schwarp fit (dsh_schwarp.cpp) for the caller that holds the matches of its one problem on the device
// already: dsh_keyframe_warp_pair (dsh_warppair.cpp) fits on the kept list where its stages left it, as dsh_sfn.h lets dsh_keyframe_sfn
// run Shape from Normals on its sites.
#pragma once
#include <cstdint>

#include "../../include/defslam_hip.h"
#include "dsh_ctx.h"
#include "dsh_diffdb.h"

namespace dsh {

// Inputs that lie on the device and outputs that stay there.  LIFETIME: slices of the context's scratch; the stages take further scratch
// slices and never call dsh_enter, so the pointers hold until the caller returns.
struct SwpDevice {
  const float *kp1, *kp2, *isg;  // P x 2, P x 2, P
  const double* x0;              // 2 N: the start value
  float* diff;                   // P x 18: the DiffProp records
  uint8_t* drop;                 // P: the drop flags
  // set by the stages: where the results of the fit lie (nothing is copied to the host, nothing is waited for)
  double* x;                     // 2 N
  int32_t* info;                 // [0] iterations [1] accepted steps [2] the verdict on the initialisation
  double* costs;                 // [0] initial [1] final
};

// The body of dsh_schwarp_fit_batch / dsh_schwarp_fit_batch_store behind their checks (the caller has called dsh_enter, validated every
// problem and, with db, reserved its records).  With dev: B == 1, db == nullptr, init_lambda == 0; the host arrays kp1, kp2, invsig, x,
// diff and drop of the problem are not read or written, and the call returns behind its last launch.  Without dev, the calls, their
// order and their operands are what they were: the same bytes come out.
int swp_fit_stages(dsh_ctx_base* c, int B, dsh_schwarp_problem* probs, const dsh_schwarp_store* stores, dsh_diffdb* db, SwpDevice* dev);

}  // namespace dsh
