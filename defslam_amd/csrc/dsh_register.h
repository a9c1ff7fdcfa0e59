// The stages of SurfaceRegistration::registerSurfaces as dsh_register.cpp runs them, for the translation units that register clouds which
// are on the device already (dsh_surfreg.cpp: dsh_keyframe_register).  Each stage moves one block up and one down (dsh_ctx.h).
#pragma once
#include <stdint.h>

#include "dsh_ctx.h"

namespace dsh {

constexpr int kMaxPairs = 8000;   // the finishing kernel keeps two floats per pair in LDS

struct Clouds {   // device copies of the two clouds (slices of a block up, or arrays a kernel left)
  const float *a = nullptr, *b = nullptr;
};

// scaleMinMedian on n pairs.  mono / stereo: host clouds, which go up with the stream and are left in d for a second stage; both null:
// the clouds are in d already.  *status: 0, 1 (stream too short: DSH_ERR_ARG), 2.
int scale_min_median_dev(dsh_ctx_base* c, int n, const float* mono, const float* stereo, const double* u, int64_t nu, float* scale, int64_t* consumed,
                         int32_t* status, Clouds& d);
// OptimizeHorn on the clouds in d, or on h1 / h2 when they are not on the device yet: then they go up with the start value
int optimize_horn_dev(dsh_ctx_base* c, int n, Clouds d, const float* h1, const float* h2, double* sim3, double chi, double huber, int32_t* acceptable, double* info);
// SurfaceRegistration.cc:132-150 on the host: the recovered scale and the new pose of the keyframe
void compose(const double* sim3, const float* Twc, double* s22_out, float* Tcw);

}  // namespace dsh
