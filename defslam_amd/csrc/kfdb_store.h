// The keyframe store dsh_kfdb as its translation units see it: dsh_mappoint.cpp (dsh_kfdb_*, dsh_mappoint_update) and dsh_tmplswitch.cpp
// (dsh_template_switch reads the descriptor rows, camera centres, octaves and scale factors of the reference keyframe).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "dsh_ctx.h"
#include "mappoint_problem.h"

// The store: descriptor rows and camera centres on the device; what validation and the election lists need on the host.
struct dsh_kfdb : dsh_store {
  int32_t cap = 0, count = 0;    // keyframes
  long long row_cap = 0, rows = 0;
  MpuSlot* d_slots = nullptr;
  uint4* d_rows = nullptr;       // two uint4 per descriptor row
  struct Kf {
    long long row_off;
    int32_t N, levels, bad;
    float sf[MPU_MAX_LEVELS];
    std::vector<int8_t> octave;
  };
  std::vector<Kf> kf;
};
