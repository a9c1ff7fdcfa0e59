// The keyframe store dsh_kfdb as its translation units see it: dsh_mappoint.cpp (dsh_kfdb_*, dsh_mappoint_update), dsh_tmplswitch.cpp
// (dsh_template_switch reads the descriptor rows, camera centres, octaves and scale factors of the reference keyframe) and
// dsh_kfinsert.cpp (dsh_keyframe_process_new, dsh_point_store_upkeep: the upkeep of map points with every input on the device) and
// dsh_surfreg.cpp (dsh_keyframe_register, dsh_keyframe_set_pose: the one writer of a stored camera centre, MpuSlot::Ow, after insertion;
// the host keeps no copy of it).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "dsh_ctx.h"
#include "mappoint_problem.h"

// The store: descriptor rows, camera centres, octaves and scale pyramids on the device; what validation and the election lists of
// dsh_mappoint_update need on the host.  The arrays beside d_slots and d_rows are parallel to them: MpuSlot keeps its layout.
struct dsh_kfdb : dsh_store {
  int32_t cap = 0, count = 0;    // keyframes
  long long row_cap = 0, rows = 0;
  MpuSlot* d_slots = nullptr;
  uint4* d_rows = nullptr;       // two uint4 per descriptor row
  int8_t* d_oct = nullptr;       // per descriptor row: the octave of its key point
  int32_t* d_levels = nullptr;   // per slot: mnScaleLevels
  float* d_sf = nullptr;         // per slot: MPU_MAX_LEVELS scale factors, zeros past levels
  int32_t n_octave_over = 0;     // keyframes with an octave >= levels
  struct Kf {
    long long row_off;
    int32_t N, levels, bad;
    bool octave_over;            // some octave >= levels (refused where it would be read)
    float sf[MPU_MAX_LEVELS];
    std::vector<int8_t> octave;
  };
  std::vector<Kf> kf;
};
