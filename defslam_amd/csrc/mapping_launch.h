// Launchers of the mapping-side kernels (nrsfm_kernels.hip, diffdb_kernels.hip, register_kernels.hip), declared once: the kernel
// files include this header too, so the compiler checks every declaration against its definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/defslam_hip.h"

// The grid of a uniform bicubic B-spline as the kernels and their launchers take it, by value; valdim is what the kernel evaluates (2 for a
// warp, 1 for a depth spline or a colocation row).  In an unnamed namespace like the kernels of nrsfm_kernels.hip: a kernel's symbol
// spells the namespace of its parameter types, and the code objects are compared byte for byte across host-side refactors.  Every
// translation unit sees this one definition, so the layout is the same on both sides of a launcher.
namespace {
struct BbsPar { double umin, umax, vmin, vmax; int nptsu, nptsv, valdim, pad; };
}  // namespace
inline BbsPar bbs_par(const dsh_bbs* b, int valdim) { return BbsPar{b->umin, b->umax, b->vmin, b->vmax, b->nptsu, b->nptsv, valdim, 0}; }
// What every entry point asks of a control grid (include/defslam_hip.h, dsh_bbs); the limits on valdim, N and P are the entry point's own.
inline bool bbs_grid_ok(const dsh_bbs* b) { return b && b->nptsu >= 4 && b->nptsv >= 4 && b->umax > b->umin && b->vmax > b->vmin; }

// ---- nrsfm_kernels.hip: B-spline evaluation / colocation, normals (dsh_nrsfm.cpp, dsh_diffdb.cpp)
extern "C" hipError_t nrsfm_launch_bbs_eval(BbsPar p, const double* ctrl, const double* u, const double* v, int n, int du, int dv, double* val, uint8_t* outside, hipStream_t st);
extern "C" hipError_t nrsfm_launch_bbs_coloc(BbsPar p, const double* u, const double* v, int n, int du, int dv, int32_t* cols, double* w, int32_t* n_outside, hipStream_t st);
extern "C" hipError_t nrsfm_launch_normals(int P, int R, const int32_t* rec_ptr, const int32_t* rec_point, const float* recs, const uint8_t* is_ref,
                                           const float* first_n, const uint8_t* has_first_n, const float* x0, const uint8_t* has_x0, const float* ref_uv,
                                           double* Q, double* k1k2, double* cov, int32_t* status, float* normal_ref, float* normal_rec, uint8_t* written,
                                           int32_t* iters, hipStream_t st);

// ---- nrsfm_kernels.hip: one Schwarp evaluation (dsh_schwarp.cpp), the dense normal equations and the one-workgroup solver that Shape from
// Normals and the warp initialisation run on (dsh_sfn.cpp).  The batched fit and nrsfm_swp_solve_np: schwarp_problem.h.
extern "C" hipError_t nrsfm_swp_eval(BbsPar b, int P, double fxs, double fys, double lambda, const float* kp1, const float* kp2, const float* invsig, const double* x,
                                     double* r, double* J, int with_j, hipStream_t st);
extern "C" hipError_t nrsfm_swp_normal(int m, int n, const double* J, const double* r, const double* cs, double* A, double* g, hipStream_t st);
extern "C" hipError_t nrsfm_swp_solve(int n2, const double* A, const double* g, double radius, double* M, double* Winv, double* dx, double* out, int interleave,
                                      int kd, hipStream_t st);
extern "C" hipError_t nrsfm_swp_resolve(int n2, const double* g, const double* M, const double* Winv, double* dx, int interleave, int kd, hipStream_t st);

// ---- nrsfm_kernels.hip: Shape from Normals, warp initialisation, search by Schwarp (dsh_sfn.cpp)
extern "C" hipError_t nrsfm_sfn_rows(BbsPar p, int n, const double* u, const double* v, const float* normals, double* A, hipStream_t st);
extern "C" hipError_t nrsfm_sfn_residual(int m, int N, const double* A, const double* x, const double* b, double sign, double* out, hipStream_t st);
extern "C" hipError_t nrsfm_sfn_axpy(int n, const double* dx, double* x, hipStream_t st);
extern "C" hipError_t nrsfm_sfn_points(BbsPar p, const double* ctrl, int n, const double* u, const double* v, float* pts, hipStream_t st);
extern "C" hipError_t nrsfm_warp_coloc(BbsPar p, int P, const float* kp1, const float* kp2, double* Cm, double* rhs0, double* rhs1, hipStream_t st);
extern "C" hipError_t nrsfm_mat_add(size_t n, const double* B, double* A, hipStream_t st);
extern "C" hipError_t nrsfm_match_search(BbsPar b, const double* x, int Q, const float* kp1, const uint32_t* desc1, const float* cam2, const float* bounds2, int cols,
                                         int rows, int N2, const float* kp2, const uint32_t* desc2, const uint8_t* has_mp2, float radius, int th_low, int32_t* cell,
                                         int32_t* match, hipStream_t st);

// ---- diffdb_kernels.hip: the DiffProp database (dsh_diffdb.cpp, dsh_schwarp.cpp, dsh_sfn.cpp)
extern "C" hipError_t ddb_pick_normals(int n, const int32_t* sel, const float* nref, const float* nrec, float* out, hipStream_t st);
extern "C" hipError_t ddb_append(int n, const uint8_t* drop, const float* diff, const int32_t* pid, const int32_t* tag, const int32_t* idx2, int32_t* keep, int32_t* pos,
                                 void* tmp, size_t tmp_bytes, long long base, long long cap, float* rec, int32_t* dpid, int32_t* dtag, int32_t* didx2, hipStream_t st);
extern "C" size_t ddb_scan_tmp_bytes(int n);
extern "C" size_t ddb_group_tmp_bytes(int P);
extern "C" hipError_t ddb_group(long long n, const int32_t* dpid, int P, const int32_t* point_ids, int nlook, int32_t* lookup, int32_t* key, int32_t* count,
                                int32_t* cursor, int32_t* perm, int32_t* owner, void* tmp, int32_t* rec_ptr, hipStream_t st);
extern "C" hipError_t ddb_gather(int R, const int32_t* perm, const float* rec, const int32_t* dtag, const int32_t* didx2, float* soa, int32_t* otag, int32_t* oidx2,
                                 hipStream_t st);

// ---- register_kernels.hip: embedding (dsh_api.cpp), surface registration (dsh_register.cpp)
extern "C" hipError_t reg_embed(int P, const float* pts, int n, const double* xyz0, const int32_t* facets, const int32_t* nf_ptr, const int32_t* nf_idx,
                                int32_t* facet_id, int32_t* nodes, float* bary, hipStream_t st);
extern "C" hipError_t reg_scale_min_median(int n, int ncand, const float* mono, const float* stereo, const double* u, const int32_t* cand,
                                           const int64_t* cand_off, float* medians, double* scales, double* out, hipStream_t st);
extern "C" hipError_t reg_horn(int n, const float* p1, const float* p2, const double* sim3_in, double chi, double huber_delta, double* err, double* out,
                               hipStream_t st);
