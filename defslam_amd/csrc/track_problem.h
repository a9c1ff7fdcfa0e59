// Device-side layout of the tracking searches (dsh_search_by_projection_*, dsh_track.cpp -> track_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/defslam_hip.h"

#define TRK_K 4                 // keys (distance, visiting order) phase A keeps per query
#define TRK_MAX_LEVELS 32
#define TRK_MAX_KEYPOINTS 8192  // the "taken" bitmap of phase B: 1 KB of LDS
#define TRK_MAX_CELLS 8192      // FRAME_GRID_COLS x FRAME_GRID_ROWS (64 x 48 in the reference)
#define TRK_MAX_CANDIDATES 4096 // key points in one query's window; more is DSH_ERR_ARG (bounds phase B's serial re-scan)
#define TRK_TH_HIGH 75          // ORBmatcher::TH_HIGH of this reference (ORBmatcher.cc:35)
#define TRK_NO_KEY 0xFFFFFFFFFFFFFFFFull

// one frame of the batch: its pose, camera, grid, pyramid and where its arrays start in the concatenated buffers
struct TrkProb {
  float R[9], t[3], Ow[3];
  float fx, fy, cx, cy, minX, maxX, minY, maxY, winv, hinv, logsf, th;
  float sf[TRK_MAX_LEVELS];
  int32_t cols, rows, levels, mode, N, Q, kp_off, q_off, cell_off, pad;
};

// what phase B needs to walk a query's window again
struct TrkWin {
  float u, v, r;
  int32_t lmin, lmax, pad[3];
};

struct TrkBufs {
  const TrkProb* prob;
  // key points of every frame, concatenated (TrkProb::kp_off): mvKeysUn x y, octave | state << 8, 32-byte descriptor
  const float2* kp;
  const int32_t* kmeta;
  const uint4* kdesc;
  // grid cells: CSR start per frame at cell_off (cols * rows + 1 entries), key points in cell order (index order within a
  // cell is not kept: the search orders candidates by the explicit key (cell, index))
  int32_t* cell_start;
  float2* skp;
  int32_t* smeta;   // index | octave << 16 | state << 24
  uint4* sdesc;
  // queries of every frame, concatenated (TrkProb::q_off)
  const int32_t* qpid;
  const float* qxyz;
  const float* qnrm;
  const float* qmaxd;
  const int32_t* qmeta;   // frame to frame: the last frame's octave; local map: the skip flag
  const uint4* qdesc;
  // phase A -> phase B
  unsigned long long* keys;   // TRK_K per query
  int32_t* ncand;
  TrkWin* win;
  // outputs
  int32_t* match;
  int32_t* level;
  int32_t* inview;
  float* uv;
  float* vcos;
  int32_t* pstat;   // 4 per frame: matches, queries re-scanned in phase B, window over TRK_MAX_CANDIDATES, a gated pass ran
  // dsh_motion_model_search only (motionmodel_kernels.hip fills what they point to); null for every other caller
  const int32_t* gate = nullptr;     // phases A and B leave at once when gate[0] >= gate_min (the narrow pass found enough); null: run
  int32_t gate_min = 0;
  const int32_t* qcount = nullptr;   // the queries the device kept: they bound Qt and TrkProb::Q, which are upper limits then
  const uint8_t* qfree = nullptr;    // per query 1: its point has no observations, so its pick does not block the key point
};

// cells, phase A, phase B
extern "C" hipError_t trk_launch(const TrkBufs& b, int B, int Qt, hipStream_t st);
// phases A and B alone, on the grid an earlier trk_launch of the same frames built (the wide pass of dsh_motion_model_search)
extern "C" hipError_t trk_launch_search(const TrkBufs& b, int B, int Qt, hipStream_t st);

// Host side shared by the entry points that run these kernels (dsh_track.cpp; dsh_localmap.cpp takes its queries from the store):
// what is wrong with a frame ("" when nothing is), and a frame as a TrkProb -- everything but the offsets into the concatenated buffers.
std::string trk_frame_error(const dsh_track_frame& f);
void trk_fill_prob(TrkProb& P, const dsh_track_frame& f, int mode, float th, int Q);
// The part of both that the frustum test alone reads (dsh_track_close_frame): Tcw, Ow, K and the image bounds; the rest of P is zero.
std::string trk_pose_error(const dsh_track_frame& f);
void trk_fill_pose(TrkProb& P, const dsh_track_frame& f);

// The device plan of one search over B frames with Nt key points, Qt queries and Ct grid cells in all, shared by dsh_search_by_projection_batch
// and dsh_local_map_search (which takes its queries from the store on the device and downloads their ids too); dsh_ctx.h has the blocks.
struct dsh_ctx_base;
struct UpBlock;
struct DownBlock;
struct TrkPlan {
  size_t B, Nt, Qt, Ct;
  size_t o_prob, o_kp, o_km, o_kd;                               // slices of the upload block
  size_t d_match, d_level, d_inview, d_uv, d_vcos, d_pstat;      // slices of the download block
};
// Lays out the frames' slices in `up` and the six output slices in `down`; the caller may add slices of its own to both before it stages.
void trk_plan_layout(TrkPlan& pl, UpBlock& up, DownBlock& down, size_t B, size_t Nt, size_t Qt, size_t Ct);
// Frame p into the staged upload block: its TrkProb and its key points (x y, octave | state << 8, descriptors) at P.kp_off.
void trk_plan_pack_frame(const TrkPlan& pl, UpBlock& up, int p, const TrkProb& P, const dsh_track_frame& f);
// Sends `up`, allocates `down` and the work arrays, enqueues the zeroing of pstat and wires b -- all of it but the six query arrays.
int trk_plan_device(dsh_ctx_base* c, const TrkPlan& pl, UpBlock& up, DownBlock& down, TrkBufs& b);
// After the download: the first frame with a query window over TRK_MAX_CANDIDATES (the search refuses, TRK_REFUSED says why), or -1.
int trk_plan_refused(const TrkPlan& pl, const DownBlock& down);
#define TRK_REFUSED "a query window holds more than 4096 candidates"
