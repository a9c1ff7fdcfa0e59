// Device-side layout of the ORB front end (dsh_orb_detect, dsh_orb_describe, dsh_orb_get_plane: dsh_orb.cpp -> orb_kernels.hip).
// Every level is kept twice: the level with its 19-pixel BORDER_REFLECT_101 frame, and the blurred plane 3 pixels beyond the level.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/defslam_hip.h"

#define ORB_MAX_LEVELS 32
#define ORB_FRAME 19            // EDGE_THRESHOLD
#define ORB_HALF_PATCH 15       // HALF_PATCH_SIZE
#define ORB_BLUR_MARGIN 3       // the blurred plane reaches this far beyond the level
#define ORB_MIN_LEVEL 62        // below it a level has no cell (nCols or nRows of :784-785 would be 0)
#define ORB_EDGE 16             // a described key point keeps this distance from the level's edges
#define ORB_CELL_MAX 65         // the widest sub-image of a cell: wCell <= 59, + 6
#define ORB_PATTERN_POINTS 512
#define ORB_PATTERN_R2 342      // the largest x^2 + y^2 of a pattern point: the rotated sample stays within 18 pixels
#define ORB_BLOCK 256
#define ORB_BLUR_TX 32          // the blur's tile: ORB_BLUR_TX x ORB_BLUR_TY outputs per workgroup
#define ORB_BLUR_TY 8

// one level on the device
struct OrbLevel {
  int32_t w, h;
  uint8_t* plane;        // (h + 38) rows of (w + 38): pixel (x, y) of the level at plane[(y + 19) * (w + 38) + x + 19]
  uint8_t* blur;         // (h + 6) rows of (w + 6): pixel (x, y) at blur[(y + 3) * (w + 6) + x + 3]
  uint8_t* kept;         // h rows of w: M of a corner that survived the suppression at the threshold its cell ended with, else 0
  const int32_t* xtab;   // resize from the level below, w entries of 3: first tap's column, c0, c1 (null for level 0)
  const int32_t* ytab;   // h entries of 3: first tap's row, b0, b1
  int32_t blur_tile0;    // the level's first tile in the blur launch
  int32_t blur_tiles_x;
};

struct OrbLevels {
  int32_t levels;
  int32_t blur_tiles;    // of all levels
  OrbLevel l[ORB_MAX_LEVELS];
};

// one cell of ComputeKeyPointsOctTree: the sub-image [x0, x1) x [y0, y1) in level pixels; corners are looked for 3 pixels inside it
struct OrbCell {
  int16_t level, pad;
  int16_t x0, y0, x1, y1;
};

struct OrbDetect {
  const OrbCell* cells;      // in the candidates' order: level, cell row, cell column
  int32_t n_cells;
  int32_t level_cell0[ORB_MAX_LEVELS + 1];   // the first cell of each level
  int32_t ini_th, min_th;
  int32_t capacity;
  int32_t* cell_count;       // n_cells
  int32_t* cell_offset;      // n_cells: the exclusive scan of cell_count within the level
  int32_t* counts;           // levels: the true counts
  int32_t* cand;             // levels * capacity * 3
};

struct OrbDescribe {
  int32_t n;
  const int32_t* level;
  const float* xy;
  const int32_t* pattern;    // 512 x 2
  float* angle;
  uint32_t* desc;            // n * 8 words
};

// level 0: the image into its framed plane
extern "C" hipError_t orb_frame_image_launch(const OrbLevel& l0, const uint8_t* image, int64_t row_stride, hipStream_t st);
// level l > 0: resize of level l - 1 and its frame, one launch
extern "C" hipError_t orb_resize_launch(const OrbLevel& below, const OrbLevel& l, hipStream_t st);
// the blurred planes of all levels, one launch
extern "C" hipError_t orb_blur_launch(const OrbLevels& L, hipStream_t st);
// FAST per cell, all levels in one launch: kept[] and cell_count[]
extern "C" hipError_t orb_fast_launch(const OrbLevels& L, const OrbDetect& d, hipStream_t st);
// cell_offset[] and counts[] from cell_count[]: one workgroup
extern "C" hipError_t orb_scan_launch(const OrbLevels& L, const OrbDetect& d, hipStream_t st);
// the kept corners of every cell into cand[], raster order inside the cell
extern "C" hipError_t orb_scatter_launch(const OrbLevels& L, const OrbDetect& d, hipStream_t st);
// one wavefront per key point: angle, then the 256 bits
extern "C" hipError_t orb_describe_launch(const OrbLevels& L, const OrbDescribe& d, hipStream_t st);
