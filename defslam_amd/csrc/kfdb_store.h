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

// What the two calls that append a keyframe share (dsh_kfdb_add; dsh_keyframe_create, which writes the device side in its own launch).
// Everything dsh_kfdb_add refuses of a keyframe but its camera centre: "" or what is wrong.
inline std::string kfdb_keyframe_error(const dsh_kfdb* db, const dsh_mp_keyframe* kf) {
  if (const char* ne = dsh_keypoint_count_error(kf->N)) return ne;
  if (kf->N > 0 && (!kf->desc || !kf->octave)) return "key point arrays are NULL";
  if (kf->levels <= 0 || kf->levels > MPU_MAX_LEVELS || !kf->scale_factors) return "levels outside 1 .. 32 or no scale factors";
  for (int j = 0; j < kf->N; j++)
    if (kf->octave[j] < 0 || kf->octave[j] > 127) return "key point octave outside 0 .. 127";
  if (db->count == INT32_MAX || db->rows + kf->N > INT32_MAX) return "store full";
  return "";
}

// room for one more keyframe with N descriptor rows
inline hipError_t kfdb_reserve(dsh_kfdb* db, int32_t N) {
  hipError_t e;
  if (db->count + 1 > db->cap) {
    const int32_t ncap = (int32_t)std::min<long long>(2ll * db->cap, INT32_MAX);
    if ((e = dsh_store_grow_array(&db->d_slots, (size_t)db->count, (size_t)ncap)) != hipSuccess ||
        (e = dsh_store_grow_array(&db->d_levels, (size_t)db->count, (size_t)ncap)) != hipSuccess ||
        (e = dsh_store_grow_array(&db->d_sf, MPU_MAX_LEVELS * (size_t)db->count, MPU_MAX_LEVELS * (size_t)ncap)) != hipSuccess)
      return e;
    db->cap = ncap;
  }
  if (db->rows + N > db->row_cap) {
    const long long ncap = std::max(db->rows + N, 2 * db->row_cap);
    if ((e = dsh_store_grow_array(&db->d_rows, 2 * (size_t)db->rows, 2 * (size_t)ncap)) != hipSuccess ||
        (e = dsh_store_grow_array(&db->d_oct, (size_t)db->rows, (size_t)ncap)) != hipSuccess)
      return e;
    db->row_cap = ncap;
  }
  return hipSuccess;
}

// the host mirror of a keyframe that goes in at the end of the store
inline dsh_kfdb::Kf kfdb_mirror(const dsh_kfdb* db, const dsh_mp_keyframe* kf, bool bad) {
  dsh_kfdb::Kf h;
  h.row_off = db->rows;
  h.N = kf->N;
  h.levels = kf->levels;
  h.bad = bad ? 1 : 0;
  h.octave_over = false;
  std::memset(h.sf, 0, sizeof(h.sf));
  for (int l = 0; l < kf->levels; l++) h.sf[l] = kf->scale_factors[l];
  h.octave.assign(kf->octave, kf->octave + kf->N);
  for (const int8_t o : h.octave) h.octave_over = h.octave_over || o >= kf->levels;
  return h;
}

// the mirror joins the store once the device side is written; returns the slot
inline int32_t kfdb_push(dsh_kfdb* db, dsh_kfdb::Kf&& h) {
  db->n_octave_over += h.octave_over ? 1 : 0;
  db->rows += h.N;
  db->kf.push_back(std::move(h));
  return db->count++;
}
