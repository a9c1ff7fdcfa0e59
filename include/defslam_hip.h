/*
 * defslam_hip.h -- C ABI of libdefslam_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the two DefSLAM hot paths:
 *   A. defSLAM::Optimizer::DefPoseOptimization(Frame*, Map*, RegLap, RegInex, RegTemp, layers)
 *        -- Modules/Tracking/DefOptimizer.h:51-53, DefOptimizer.cc:251-578 (g2o LM + dense LDLT)
 *   B. defSLAM::NormalEstimator::ObtainK1K2()       -- Modules/Mapping/NormalEstimator.h:46-53
 *      BBS::eval / Warps::Warp estimates            -- Thirdparty/BBS/bbs.h:52-66
 *
 * Conventions: plain pointers + sizes, caller-owned host buffers, every entry point
 * returns an int status (DSH_OK == 0); nothing throws or aborts across the ABI.  A context
 * is bound to one GPU and is not thread-safe (one context per host thread / per GPU),
 * mirroring the reference where each optimiser call runs on exactly one thread
 * (DefOptimizer.cc:287 holds MapPoint::mGlobalMutex for its whole body).
 * All floating point is FP64 unless a parameter says float (the reference's float32
 * boundaries: cv::Mat pose, keypoints, DefMapPoint world positions).
 */
#ifndef DEFSLAM_HIP_H
#define DEFSLAM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)   /* the library is built with -fvisibility=hidden: only this ABI is exported */
#endif

#define DSH_OK 0
#define DSH_ERR_ARG 1        /* bad argument / size */
#define DSH_ERR_HIP 2        /* HIP runtime failure (see dsh_last_error) */
#define DSH_ERR_STATE 3      /* call sequence violated (no template, no batch ...) */
#define DSH_ERR_NO_DEVICE 4  /* no usable gfx950 device */

#define DSH_TRACE_STRIDE 8   /* doubles per outer LM iteration in the trace buffer:
                                chi2_start, lambda_start, trials, chi2_end, lambda_end, rho, accepted, factor_ok */
#define DSH_MAX_ITERS 64

typedef struct dsh_ctx dsh_ctx;

/* ---- context ----------------------------------------------------------------------------- */
/* device >= 0: bind to that GPU.  device == -1: host-only context (template constants, embedding and
 * problem packing work; every entry point that needs the GPU returns DSH_ERR_NO_DEVICE -- no CPU fallback). */
int dsh_create(dsh_ctx** out, int device);
int dsh_destroy(dsh_ctx* ctx);
const char* dsh_last_error(const dsh_ctx* ctx);
/* HIP stream handle (hipStream_t) the context launches on; lets a caller time with its own events. */
void* dsh_stream(dsh_ctx* ctx);
int dsh_synchronize(dsh_ctx* ctx);

/* ---- template (replaces the numbers produced by Modules/Template) ------- */
/* Derive every constant from vertices + facets the way the reference does:
 * edges/rest lengths (Facet.cc:32-56, Edge.cc:29-59), 1-ring (Node.cc:114-129), Laplacian
 * weights / boundary flags / initial mean curvature (LaplacianMesh.cc:53-162), median edge
 * (Template.cc:158-175).  Ordering: nodes by index, edges by creation order. */
int dsh_template_build(dsh_ctx* ctx, int n, const double* xyz0 /* n*3 */, int F, const int32_t* facets /* F*3 */);
/* Or hand the constants over directly (what a host shim holding the reference's Template would do). */
int dsh_template_set(dsh_ctx* ctx, int n, const double* xyz0, const uint8_t* boundary,
                     const int32_t* nbr_rowptr /* n+1 */, const int32_t* nbr_col, const double* nbr_w,
                     const double* k0 /* n */, int E, const int32_t* edge_nodes /* E*2 */, const double* edge_L0 /* E */,
                     double median_L);
/* Read back the constants of the current template (any pointer may be NULL; sizes via dsh_template_dims). */
int dsh_template_dims(const dsh_ctx* ctx, int32_t* n, int32_t* E, int32_t* nnz_nbr);
int dsh_template_get(const dsh_ctx* ctx, uint8_t* boundary, int32_t* nbr_rowptr, int32_t* nbr_col, double* nbr_w,
                     double* k0, int32_t* edge_nodes, double* edge_L0, double* median_L);
/* Barycentric embedding of P float32 points (TriangularMesh.cc:133-236): facet id (-1: none),
 * facet node ids ascending, barycentrics (float32 arithmetic as in the reference). */
int dsh_template_embed(const dsh_ctx* ctx, int P, const float* pts /* P*3 */, int32_t* facet_id, int32_t* nodes /* P*3 */,
                       float* bary /* P*3 */);

/* ---- Shape-from-Template solve ------------------------------------------------------------ */
typedef struct dsh_sft_frame {
  const float* Tcw;            /* 4x4 row-major float32 (cv::Mat pFrame->mTcw), initial camera pose */
  double K[4];                 /* fx, fy, cx, cy */
  int32_t n_frame;             /* pFrame->N: keypoints in the frame (DefOptimizer.cc:340 divides by it) */
  int32_t M;                   /* observations that enter the graph (DefOptimizer.cc:293-361) */
  const int32_t* obs_nodes;    /* M*3 node ids of the facet, ascending */
  const double* obs_bary;      /* M*3 */
  const double* obs_uv;        /* M*2 undistorted keypoints */
  const double* obs_invsig2;   /* M   mvInvLevelSigma2[octave] */
  const double* xyz;           /* n*3 current node positions */
  double reg_lap, reg_inex, reg_temp;
  int32_t neighbour_layers;    /* >=1: viewed nodes + 1-ring (the reference quirk, DefOptimizer.cc:388-406); 0: viewed only */
  int32_t max_iters;           /* 50 in the reference (DefOptimizer.cc:513); 0 = no iteration (the reference never does this): no edge error is
                                * ever computed, every observation counts as an inlier, repError is the mean reprojection error of the
                                * initial state -- what the oracle's restatement of g2o's freshly allocated edges gives */
} dsh_sft_frame;

typedef struct dsh_sft_result {
  float* Tcw;                  /* 4x4 float32 out (Converter::toCvMat) */
  double* pose7;               /* tx,ty,tz,qx,qy,qz,qw */
  double* xyz;                 /* n*3 */
  double* chi2_obs;            /* M: e^T Omega e of each observation at its last evaluation (DefOptimizer.cc:527) */
  uint8_t* outlier;            /* M: (float)chi2 > 5.991 */
  float* mappoint_xyz;         /* M*3 float32: DefMapPoint::RecalculatePosition of each observation's point */
  double rep_error;            /* mean reprojection error over inliers (pFrame->repError) */
  int32_t inliers;             /* return value of DefPoseOptimization */
  int32_t iters;               /* outer LM iterations executed */
  int32_t trials;              /* total damping trials (linear solves) */
  int32_t dim;                 /* 6 + 3*active nodes */
  int32_t half_bandwidth;      /* scalar half-bandwidth of the node block */
  int32_t status;              /* 0, or bit 0: a factorisation failed at least once */
  double* trace;               /* max_iters*DSH_TRACE_STRIDE doubles, may be NULL */
} dsh_sft_result;

/* One-shot: pack + upload + solve + download. */
int dsh_sft_solve(dsh_ctx* ctx, const dsh_sft_frame* frame, dsh_sft_result* result);

/* Batched / device-resident form (independent problems against the current template):
 *   dsh_sft_batch_upload  packs B frames on the host and starts ONE asynchronous copy to HBM on dsh_stream
 *                         (the frame buffers may be reused as soon as it returns),
 *   dsh_sft_batch_run     launches the solve on dsh_stream; may be called repeatedly -- every run restarts from the uploaded
 *                         initial state.  The launch shape is chosen at upload from the batch and the device:
 *                           - more than num_cus/2 problems, every half-bandwidth <= 128: the throughput shape.  From two problems
 *                             per compute unit upwards a step is rounds of three phase kernels over the whole batch (linearise /
 *                             factor + solve with ONE wavefront per problem / trial + controller) and, once no more than
 *                             T = min(4 num_cus, max(2 num_cus, 3 B / 4)) problems are still running, ONE launch of a tail kernel
 *                             in which every remaining problem gets a workgroup of eight wavefronts that runs it to its end (the
 *                             switch is decided on the device from the count of finished problems).  A batch of T problems or
 *                             fewer is run by the tail kernel alone.  The call enqueues launches and returns when every problem
 *                             has terminated;
 *                           - more than num_cus/2 problems with a wider band among them: one persistent kernel, one workgroup per
 *                             problem; the call returns at once;
 *                           - smaller batches (a tracked frame) run in latency mode: min(4, num_cus / B) workgroups per problem
 *                             try consecutive dampings of a Levenberg-Marquardt iteration side by side, one launch per round,
 *                             and the call returns when the problems have terminated; while the launch holds at most
 *                             num_cus/20 problems, a band of more than one tile that is long enough is cut in two parts
 *                             factored by two workgroups.
 *                         All shapes run the same Levenberg-Marquardt controller on the same normal equations; they differ
 *                         in the elimination order of the Cholesky factorisation, so the SAME frame solved in batches of
 *                         different size, or on devices with a different number of compute units, agrees to rounding
 *                         (vertices to ~1e-12 relative on the test templates), not bit for bit.  This holds INSIDE the
 *                         throughput shape as well: the tail kernel's eight-wavefront solver sums in another order than the
 *                         one-wavefront solver of the rounds (x of one damped system agrees to ~5e-13 relative), and which of
 *                         the two finishes a problem depends on B, on num_cus and on how many trials the OTHER problems of the
 *                         batch need -- the result bits of a problem depend on the batch it is solved in.  A fixed (batch,
 *                         device) reproduces itself bit for bit.  Problems that end in terminal stagnation (an iteration of >= 8
 *                         rejected dampings in a row: the steps are below one ulp of the state) may differ between shapes
 *                         in the number of rejected trials of that last iteration; the state returned agrees as above,
 *   dsh_sft_batch_download brings every result of the batch back with ONE copy (outlier classification, inlier count,
 *                         repError and the float32 map points are computed by the kernel) and waits for it.
 * To time the device work, record your own HIP events on dsh_stream() around dsh_sft_batch_run.
 * Measurement and debugging aids (per-phase timers, assembly-only launches, the dense normal equations of a problem,
 * solver A/B switches) are NOT part of this ABI: include/defslam_hip_debug.h, libdefslam_hip_lab.so. */
int dsh_sft_batch_upload(dsh_ctx* ctx, int B, const dsh_sft_frame* frames);
int dsh_sft_batch_run(dsh_ctx* ctx);
int dsh_sft_batch_download(dsh_ctx* ctx, int B, dsh_sft_result* results);
/* Totals of the last completed run (valid after a synchronise): outer iterations and trials over the batch. */
int dsh_sft_batch_counts(dsh_ctx* ctx, int64_t* iters, int64_t* trials);
/* Algorithmic bytes of one assembly pass of problem b (SURVEY 8d convention) and its edge counts
 * counts[9] = M, n_active, curvature edges (reference count), stretch edges, viewed nodes, dim,
 * half-bandwidth of the node block (scalars), wavefronts per problem of the launch shape chosen at upload (8, 4; 1 = rounds of
 * phase kernels with one wavefront per factorisation),
 * off-diagonal 3x3 blocks of H (lower triangle). */
int dsh_sft_batch_problem_info(dsh_ctx* ctx, int b, int64_t* assembly_bytes, int32_t* counts);

/* ---- shared-camera Shape-from-Template across GPUs ---------------------------------------------------------------------
 * BASELINE north star: "the path shards naturally over independent keyframes / mesh patches ... with RCCL all-reduce of the
 * shared camera-pose normal equations".  Every rank (one GPU, one context) holds one patch -- its own template, observations
 * and vertices -- and all patches are seen by ONE camera whose pose is estimated jointly (the reference's graph with a single
 * VertexSE3Expmap and the node vertices of every patch, DefOptimizer.cc:293-507).  The camera is the only coupling: each rank
 * factorises its node block and reduces to its 6x6 Schur complement of the camera; the ranks all-reduce that block, its
 * right-hand side and the scalars of the Levenberg-Marquardt control (32 doubles, three times per damping trial) and continue
 * with identical decisions.  The result equals the single-GPU solve of the union of the patches (tested).  The default for
 * independent problems stays dsh_sft_batch_*: no collective at all. */
typedef struct dsh_comm dsh_comm;
#define DSH_COMM_ID_BYTES 128
/* ncclGetUniqueId: call on one rank, hand the bytes to every rank (RCCL is loaded at the first call, not at library load). */
int dsh_comm_unique_id(void* id /* DSH_COMM_ID_BYTES */);
/* ncclCommInitRank on the context's GPU; collective over the nranks processes. */
int dsh_comm_create(dsh_ctx* ctx, int nranks, int rank, const void* id, dsh_comm** out);
int dsh_comm_destroy(dsh_comm* comm);
/* Collective: every rank passes its own patch (frame->Tcw, K, n_frame must agree); result as dsh_sft_solve, per patch, with
 * the joint pose.  The regulariser weights use the joint counts (all optimised nodes / stretch edges of all patches). */
int dsh_sft_shared_solve(dsh_ctx* ctx, dsh_comm* comm, const dsh_sft_frame* frame, dsh_sft_result* result);
/* The same protocol inside one process over G contexts (normally on one GPU), the all-reduce done by a summation kernel:
 * how the protocol is validated against the single-GPU solve where only one GPU is available. */
int dsh_sft_shared_solve_group(int G, dsh_ctx* const* ctxs, const dsh_sft_frame* frames, dsh_sft_result* results);

/* ---- one CONNECTED template across two GPUs --------------------------------------------------------------------------------
 * The shared-camera mode above joins patches that only share the camera.  A connected mesh also couples across any cut through its
 * curvature, stretching and observation edges (DefOptimizer.cc:408-507): the band ordering of the unknowns is therefore cut at a
 * SEPARATOR of one bandwidth (the 2-ring halo of the cut), rank 0 factors the part in front of it, rank 1 the part behind it (in
 * reversed order), both all-reduce their Schur contributions to the separator + camera system (one all-reduce of about
 * (kd^2 / 2 + 8 kd) doubles per damping trial), solve that reduced system redundantly, back-substitute their own part, and a second
 * all-reduce (6 + 3 n_active doubles) assembles the update.  Residuals, Jacobians and the Levenberg-Marquardt control are replicated
 * (every rank passes the SAME frame and holds the whole state), so the ranks take identical decisions without further collectives.
 * The result equals dsh_sft_solve of the same frame (the same Cholesky factorisation in another elimination order; tested against
 * the oracle).  Needs half-bandwidth <= 256 and a band long enough to cut; exactly two ranks -- a further cut along the same
 * ordering would make an inner part carry the fill of a whole separator through every column. */
int dsh_sft_connected_solve(dsh_ctx* ctx, dsh_comm* comm, const dsh_sft_frame* frame, dsh_sft_result* result);
/* The same protocol inside one process over two contexts (normally on one GPU), the all-reduces done by a summation kernel: how the
 * protocol is validated where only one GPU is available.  results[2]: one per context (identical). */
int dsh_sft_connected_solve_group(dsh_ctx* ctx0, dsh_ctx* ctx1, const dsh_sft_frame* frame, dsh_sft_result* results);

/* ---- NRSfM mapping side ----------------------------------------------------------------------- */
/* Uniform bicubic B-spline (BBS::bbs_t, Thirdparty/BBS/bbs.h:41-50).  The control grid is an argument of every call (in the reference it
 * is a compile-time constant, 13 x 15).  Every entry point that takes one wants nptsu >= 4, nptsv >= 4, umax > umin and vmax > vmin and
 * returns DSH_ERR_ARG otherwise; the entry points that solve for the control points also limit N = nptsu*nptsv, because one workgroup
 * factors the padded system (at most 512 unknowns).  A refused call changes nothing: the context stays usable.
 *   dsh_schwarp_eval                                                N <= 4096
 *   dsh_schwarp_fit, dsh_schwarp_fit_batch, .._fit_batch_store      N <= 256   (2 N unknowns)
 *   dsh_sfn_estimate, dsh_sfn_estimate_db, dsh_warp_initialize      N <= 512
 *   dsh_bbs_eval, dsh_bbs_coloc, dsh_search_by_schwarp              no limit on N */
typedef struct dsh_bbs {
  double umin, umax;
  int32_t nptsu;
  double vmin, vmax;
  int32_t nptsv;
  int32_t valdim;
} dsh_bbs;

/* BBS::eval (Thirdparty/BBS/bbs.h:59, bbs.cc:155-195): val[valdim*k + d] = d^du d^dv spline(u_k, v_k).
 * ctrl: valdim x (nptsu*nptsv), index valdim*(iu*nptsv + iv) + d.  outside[k] (may be NULL) = 1 for a site outside the
 * definition domain (the reference reads out of bounds there; here the value is 0). */
int dsh_bbs_eval(dsh_ctx* ctx, const dsh_bbs* bbs, const double* ctrl, const double* u, const double* v, int n, int du, int dv,
                 double* val, uint8_t* outside);
/* Row view of BBS::coloc / BBS::coloc_deriv (bbs.h:61-63, bbs.cc:214-355): for site k the 16 (column, weight) pairs in
 * (iu, iv) order, cols[16k + 4iu + iv] = (iu+Iu)*nptsv + iv+Iv.  n_outside counts sites outside the domain (the reference
 * returns error code 1 for them); their columns are -1. */
int dsh_bbs_coloc(dsh_ctx* ctx, const dsh_bbs* bbs, const double* u, const double* v, int n, int du, int dv, int32_t* cols, double* w,
                  int32_t* n_outside);

/* The float32 fields of defSLAM::DiffProp the normal solve reads (Modules/Mapping/diffProp.h:52-83), in this order. */
typedef struct dsh_diffprop {
  float I1u, I1v, I2u, I2v;
  float J12a, J12b, J12c, J12d;
  float J21a, J21b, J21c, J21d;
  float H12uux, H12uuy, H12uvx, H12uvy, H12vvx, H12vvy;
} dsh_diffprop;

/* NormalEstimator::ObtainK1K2 (Modules/Mapping/NormalEstimator.h:53, NormalEstimator.cc:38-229) over the P map points that
 * have new observations.
 *   rec_ptr[P+1]            CSR: DiffProp records of point p are rec_ptr[p] .. rec_ptr[p+1]-1
 *   rec_is_ref[R]           record.KFToKF.first is the point's reference keyframe (it contributes a residual block)
 *   rec_first_normal[R*2], rec_has_first_normal[R]   (k1,k2) stored for the record's first keyframe (used by non-ref records)
 *   x0[P*2], has_x0[P]      previous normal of the reference keyframe; without it the start is (0,-0)
 *   ref_uv[P*2]             mpKeypointNorm of the point in its reference keyframe
 * Outputs: k1k2[P*2]; cov[P*4] (may be NULL); status[P]: 0 solved and written, 1 no residual block, 2 covariance failed
 * (rank-deficient Jacobian -> the reference skips the point); normal_ref[P*3] float = (k1,k2,1-k1 u-k2 v) (may be NULL);
 * normal_rec[R*3] float + rec_written[R]: normals propagated to the second keyframe of each record (may be NULL); iters[P]
 * (may be NULL). */
int dsh_normals_estimate(dsh_ctx* ctx, int P, const int32_t* rec_ptr, const dsh_diffprop* recs, const uint8_t* rec_is_ref,
                         const float* rec_first_normal, const uint8_t* rec_has_first_normal, const float* x0, const uint8_t* has_x0,
                         const float* ref_uv, double* k1k2, double* cov, int32_t* status, float* normal_ref, float* normal_rec,
                         uint8_t* rec_written, int32_t* iters);

/* Schwarzian-regularised B-spline warp between two keyframes.
 * Parameters x[2N], N = nptsu*nptsv: x[0..N) first coordinate of the control points, x[N..2N) second (index iu*nptsv+iv).
 * kp1 / kp2: P normalised key points (float32 x,y) of the reference / current keyframe; invsig[P] = sqrt(invSigma2[octave]);
 * fx_slot / fy_slot: the values the reference passes in Warp's (fx, fy) slots (SchwarpDatabase.cc:200-201 passes (fy, fx)).
 * dsh_schwarp_eval: the two Ceres cost functions evaluated once -- Warps::Warp::Evaluate (Schwarp.cc:235-303) in rows
 *   [0, 2P) and Warps::Schwarzian::Evaluate (Schwarp.cc:368-543) in rows [2P, 2P+4N); jacobian (may be NULL) is dense
 *   row-major (2P+4N) x 2N, including the reference's overwritten y-rows of the warp block. */
int dsh_schwarp_eval(dsh_ctx* ctx, const dsh_bbs* bbs, int P, const float* kp1, const float* kp2, const float* invsig, double fx_slot,
                     double fy_slot, double lambda, const double* x, double* residuals, double* jacobian);
/* SchwarpDatabase::calculateSchwarps (SchwarpDatabase.cc:145-349): HuberLoss(5.77) on the warp block, Levenberg-Marquardt
 * (max_iters = 3 in the reference), then the DiffProp record of every match (diff[P], may be NULL together with drop) and
 * drop[p] = 1 when its reprojection error exceeds 10 px (fx, fy = KF->fx, KF->fy).  x is in/out.
 * info[0] = iterations, info[1] = accepted steps; costs[0] initial, costs[1] final cost (both may be NULL).
 * At most 256 control points (nptsu*nptsv <= 256, e.g. 16 x 16): beyond them DSH_ERR_ARG, here and in the batched calls below. */
int dsh_schwarp_fit(dsh_ctx* ctx, const dsh_bbs* bbs, int P, const float* kp1, const float* kp2, const float* invsig, double fx_slot,
                    double fy_slot, double lambda, float fx, float fy, int max_iters, double* x, dsh_diffprop* diff, uint8_t* drop,
                    int32_t* info, double* costs);

/* The same fit for B keyframe pairs at once (SchwarpDatabase::add fits one warp per anchor keyframe of the new keyframe,
 * SchwarpDatabase.cc:50-128): one copy up, a fixed sequence of launches in which all fits advance together with the
 * trust-region control on the device (no host round trip), one copy back.  A fit's result does not depend on what else is in the batch
 * (dsh_schwarp_fit is the batch of one). */
typedef struct dsh_schwarp_problem {
  dsh_bbs bbs;
  int32_t P;
  const float* kp1;            /* P x 2 */
  const float* kp2;            /* P x 2 */
  const float* invsig;         /* P */
  double fx_slot, fy_slot, lambda;
  float fx, fy;
  int32_t max_iters;
  double* x;                   /* in/out, 2 N */
  dsh_diffprop* diff;          /* P, may be NULL together with drop */
  uint8_t* drop;               /* P */
  int32_t info[2];             /* out: iterations, accepted steps */
  double costs[2];             /* out: initial, final cost */
  double init_lambda;          /* > 0: x is an output only -- the fit starts from Warps::Warp::initialize (Schwarp.cc:99-160, see
                                  dsh_warp_initialize below) with this bending weight, computed on the device as the first stage of the
                                  batch; <= 0: x holds the caller's start value */
  int32_t init_ok;             /* out: the verdict of that initialisation (1 when none was asked for) */
} dsh_schwarp_problem;
int dsh_schwarp_fit_batch(dsh_ctx* ctx, int B, dsh_schwarp_problem* problems);

/* ---- device-resident mapping chain --------------------------------------------------------------------------------------
 * defSLAM::WarpDatabase keeps the DiffProp records of every map point in a host map (WarpDatabase.h:61 mapPointsDB_): the fits write
 * them (SchwarpDatabase.cc:299-345), NormalEstimator::ObtainK1K2 reads them back (NormalEstimator.cc:50-110).  dsh_diffdb is that
 * database in HBM: dsh_schwarp_fit_batch_store appends the records of its fits on the device (in fit, match order; only the drop flags
 * travel to the host), dsh_normals_estimate_db groups the records of the requested points on the device (a point's records in their
 * insertion order, like the host vector) and solves -- key points in, normals out, no record crosses PCIe. */
typedef struct dsh_diffdb dsh_diffdb;
/* capacity_records is the initial capacity: like the reference's map the database grows on demand (appends and stores reserve their
 * worst case first, so a call stores all of its records or fails without storing any).  Lifetime: a database belongs to the context it
 * was created on; dsh_destroy of that context detaches it -- every call on it then returns DSH_ERR_ARG -- and dsh_diffdb_destroy works
 * before or after dsh_destroy. */
int dsh_diffdb_create(dsh_ctx* ctx, int64_t capacity_records, dsh_diffdb** out);
int dsh_diffdb_destroy(dsh_diffdb* db);
int dsh_diffdb_clear(dsh_diffdb* db);                 /* forget every record (WarpDatabase::clear) */
int64_t dsh_diffdb_count(const dsh_diffdb* db);       /* records stored */
/* Records a host already holds (a map loaded from elsewhere, tests): point_id[n] >= 0, tag[n] / idx2[n] may be NULL (0 / the index). */
int dsh_diffdb_append(dsh_diffdb* db, int n, const dsh_diffprop* recs, const int32_t* point_id, const int32_t* tag, const int32_t* idx2);
/* What dsh_schwarp_fit_batch_store needs per problem besides the fit itself: the map point of every match (point_id[P]; < 0: the record
 * is not stored -- the reference stores only points whose reference keyframe is the pair's first keyframe, SchwarpDatabase.cc:297), the
 * key point index of the match in the second keyframe (idx2[P], NULL = the match index) and a tag the caller chooses for the keyframe
 * pair; both come back with the propagated normals. */
typedef struct dsh_schwarp_store {
  const int32_t* point_id;
  const int32_t* idx2;
  int32_t tag;
} dsh_schwarp_store;
/* dsh_schwarp_fit_batch + storing: problems[b].diff may be NULL (no record is copied to the host), problems[b].drop receives the drop
 * flags (the host bookkeeping of SchwarpDatabase.cc:283-293 needs them).  Records of matches that are dropped or have point_id < 0 are
 * not stored.  DSH_ERR_STATE when the database is full. */
int dsh_schwarp_fit_batch_store(dsh_ctx* ctx, int B, dsh_schwarp_problem* problems, const dsh_schwarp_store* stores, dsh_diffdb* db);
/* NormalEstimator::ObtainK1K2 over the database for the P map points point_ids[P] (x0 / has_x0 / ref_uv and the per-point outputs as in
 * dsh_normals_estimate; every stored record is a residual block of its point; the ids are distinct, ids without records are
 * skipped like a point without observations).  Per-record outputs (all may be NULL), n_rec entries in
 * point order then insertion order, the buffers holding max_rec entries: rec_point (index into point_ids), rec_tag, rec_idx2, the
 * normal propagated to the second keyframe (normal_rec[3 n]) and whether the reference writes it (rec_written). */
int dsh_normals_estimate_db(dsh_ctx* ctx, dsh_diffdb* db, int P, const int32_t* point_ids, const float* x0, const uint8_t* has_x0, const float* ref_uv,
                            double* k1k2, double* cov, int32_t* status, float* normal_ref, int32_t* iters, int32_t max_rec, int32_t* n_rec,
                            int32_t* rec_point, int32_t* rec_tag, int32_t* rec_idx2, float* normal_rec, uint8_t* rec_written);

/* ---- Shape from Normals -------------------------------------------------------------------------
 * ShapeFromNormals::ShapeFromNormals + ::estimate (Modules/Mapping/ShapeFromNormals.cc:38-171, obtainM :178-260): the
 * depth B-spline (valdim 1, bbs->valdim is ignored) of a keyframe from the normals of its map points.
 *   n sites (u[n], v[n] normalised key point coordinates, normals[3n] float32 as stored by Surface::getNormalSurfacePoint;
 *   the caller filters bad map points / missing normals exactly like obtainM does); bending_weight = the constructor's
 *   bendingWeight_; mean_depth = DefKeyFrame::accMean; n_all key points (u_all, v_all) receive a surface point.
 * Least squares  min |M x|^2 + |Bend x|^2 + (sum x - N mean_depth)^2  over the N = nptsu*nptsv control points, then the
 * reference's scale: ctrl = x / float(median of float(x)) (Surface::saveArray), pts[3 n_all] = float (u d, v d, d) with
 * d = BBS eval of ctrl (Surface::set3DSurfacePoint).  ctrl_raw (may be NULL) receives x before the scaling.
 * *ok = 0 (and DSH_OK) when the reference's estimate() would return false: no key points, rank-deficient system, NaN/Inf.
 * At most 512 control points (nptsu*nptsv <= 512, e.g. 16 x 32): beyond them DSH_ERR_ARG, also in dsh_sfn_estimate_db. */
int dsh_sfn_estimate(dsh_ctx* ctx, const dsh_bbs* bbs, int n, const double* u, const double* v, const float* normals, double bending_weight,
                     double mean_depth, int n_all, const double* u_all, const double* v_all, double* ctrl_raw, double* ctrl, float* pts, int32_t* ok);
/* The same with the normals taken on the device from the last dsh_normals_estimate_db of db (they never visit the host): sel[n] >= 0 is
 * the index of a point in that call's point_ids (its normal in the reference keyframe, normal_ref), sel[n] < 0 is record -1 - sel[n] of
 * that call's per-record order (the normal propagated to the record's second keyframe, normal_rec).  The caller picks solved points /
 * written records from the status and rec_written arrays that call returned, like obtainM filters missing normals. */
int dsh_sfn_estimate_db(dsh_ctx* ctx, const dsh_bbs* bbs, const dsh_diffdb* db, int n, const int32_t* sel, const double* u, const double* v, double bending_weight,
                        double mean_depth, int n_all, const double* u_all, const double* v_all, double* ctrl_raw, double* ctrl, float* pts, int32_t* ok);
/* Warps::Warp::initialize (Modules/Mapping/Schwarp.cc:99-160): the control points of the warp kp1 -> kp2 that start the
 * Schwarzian fit, (C^T C + Bending(lambda)) X = C^T kp2 with C the colocation matrix of the P key points kp1 (float32 x,y
 * pairs, normalised coordinates).  x[2N]: first coordinate of the N control points, then the second (the layout
 * dsh_schwarp_fit takes).  *ok = 0 when the matrix is not positive definite (too few matches for this lambda).
 * At most 512 control points (nptsu*nptsv <= 512): beyond them DSH_ERR_ARG. */
int dsh_warp_initialize(dsh_ctx* ctx, const dsh_bbs* bbs, int P, const float* kp1, const float* kp2, double lambda, double* x, int32_t* ok);
/* DefORBmatcher::searchBySchwarp (Modules/Matching/DefORBmatcher.cc:189-294): for each of the Q query key points of keyframe
 * 1 (the caller keeps the reference's filter :200-211: map point present, not bad, not yet in keyframe 2; kp1 = mpKeypointNorm,
 * desc1 = the 32-byte ORB descriptor rows) predict the position in keyframe 2 through the warp x[2N] (Warp::getEstimates,
 * float32 key point), convert to pixels with cam2 = {fx, fy, cx, cy}, skip predictions outside bounds2 = {mnMinX, mnMaxX,
 * mnMinY, mnMaxY} (KeyFrame::IsInImage), and among the key points of keyframe 2 (kp2 = mvKeysUn in pixels, desc2) that lie in
 * the search window of KeyFrame::GetFeaturesInArea(x, y, radius) (grid_cols x grid_rows = FRAME_GRID_COLS x FRAME_GRID_ROWS)
 * and have no map point (has_mp2[j] == 0) take the one with the smallest Hamming distance below th_low (TH_LOW = 50); among
 * equal distances the first one in the reference's visiting order (grid column, grid row, index).
 * match[q] = index in keyframe 2 or -1; *nmatches (may be NULL) = number of matches.  Bit-exact index parity. */
int dsh_search_by_schwarp(dsh_ctx* ctx, const dsh_bbs* bbs, const double* x, int Q, const float* kp1, const uint8_t* desc1, const float* cam2,
                          const float* bounds2, int grid_cols, int grid_rows, int N2, const float* kp2, const uint8_t* desc2, const uint8_t* has_mp2,
                          float radius, int th_low, int32_t* match, int32_t* nmatches);
/* BBS bending matrix (Thirdparty/BBS/bbs.cc:556-641 bending_ur, bbs_coloc.cc:406-508 BendingEigen) as a dense symmetric
 * N x N matrix, host side (the constant part of the Shape-from-Normals system). */
int dsh_bbs_bending(const dsh_bbs* bbs, double lambda, double* bending);

/* ---- surface registration ---------------------------------------------------------------------- */
/* Barycentric embedding on the device: same contract and results as dsh_template_embed (TriangularMesh.cc:133-236), one
 * wavefront per point (closest node, then the node's facets in index order).  Needs a template built from facets. */
int dsh_template_embed_device(dsh_ctx* ctx, int P, const float* pts /* P*3 */, int32_t* facet_id, int32_t* nodes /* P*3 */,
                              float* bary /* P*3 */);
/* GroundTruthTools::scaleMinMedian(PosMono, PosStereo) (Modules/GroundTruth/GroundTruthCalculator.cc:54-160).  The reference
 * draws `(double)rand() / RAND_MAX` while it runs; here the stream of those numbers is an input (u[k] = the k-th draw,
 * consumed in the reference's order: one per point i, and n-1 more for every i that was selected), so a shim that fills it
 * from rand() reproduces the reference.  *status: 0 ok, 1 stream too short (DSH_ERR_ARG is returned as well), 2 the
 * reference's early `return 0.0` (a selected point whose own selection holds fewer than two residuals; the reference reads
 * past the end of a vector when it holds none -- defined as the same early return).  *consumed (may be NULL) = draws used
 * when status is 0. */
int dsh_scale_min_median(dsh_ctx* ctx, int n, const float* pos_mono /* n*3 */, const float* pos_stereo /* n*3 */, const double* u,
                         int64_t nu, float* scale, int64_t* consumed, int32_t* status);
/* Optimizer::OptimizeHorn(pts1, pts2, g2oS12, chi, huber) (Modules/Tracking/DefOptimizer.cc:840-922): Levenberg-Marquardt on
 * one Sim(3) vertex with edges e_i = pts2_i - S.map(pts1_i), Huber(sqrt(huber) as float), numeric Jacobians (g2o's central
 * differences, delta 1e-9), optimize(50) twice.  sim3[8] = {qx, qy, qz, qw, tx, ty, tz, s}: in the initial estimate, out the
 * estimate after the FIRST optimize (what the reference reads back, :896).  *acceptable = the function's return value.
 * info[6] (may be NULL) = {plain chi2 of all edges after the second optimize, count, iterations 1st, iterations 2nd, damping
 * trials 1st, trials 2nd}. */
int dsh_optimize_horn(dsh_ctx* ctx, int n, const float* pts1 /* n*3 */, const float* pts2 /* n*3 */, double* sim3 /* 8 */, double chi,
                      double huber, int32_t* acceptable, double* info /* 6 */);
/* SurfaceRegistration::registerSurfaces (Modules/Mapping/SurfaceRegistration.cc:48-153), numeric part: cloud_surface = the
 * keyframe's surface points in world coordinates (cloud2pc), cloud_map = the map points' positions at that keyframe
 * (cloud1pc), Twc = the keyframe's inverse pose (4x4 row-major float32).  Fewer than 15 pairs -> *registered = 0.  Otherwise
 * scaleMinMedian(cloud_surface, cloud_map) initialises the scale, OptimizeHorn (chi = chi_limit^2, huber 0.01) aligns, and
 * unless (!acceptable && check_chi) the Sim(3) is composed with Twc: *s22 = recovered scale (Surface::applyScale takes it),
 * Tcw_new = the new keyframe pose (float32).  The clouds stay on the device between the two steps.
 * info[8] (may be NULL) = {initial scale, chi2, count, iterations 1st/2nd, trials 1st/2nd, acceptable}. */
int dsh_surface_register(dsh_ctx* ctx, int n, const float* cloud_surface /* n*3 */, const float* cloud_map /* n*3 */, const double* u,
                         int64_t nu, const float* Twc /* 16 */, double chi_limit, int check_chi, int32_t* registered, double* sim3 /* 8 */,
                         double* s22, float* Tcw_new /* 16 */, double* info /* 8 */);

/* ---- tracking: search by projection (the observations of the SfT problem) ----------------------------------------------
 * DefTracking::TrackWithMotionModel (Modules/Tracking/DefTracking.cc:342-375) and DefTracking::TrackLocalMap -> SearchLocalPoints
 * (DefTracking.cc:234-250, Thirdparty/ORBSLAM_2/src/Tracking.cc:1405-1470) match map points to the key points of the current frame:
 *   frame to frame  ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono)        ORBmatcher.cc:1360-1510
 *   local map       Frame::isInFrustum(pMP, 0.5) (Frame.cc:338-390), MapPoint::PredictScale (MapPoint.cc:422-437),
 *                   ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>, th), nn-ratio 0.8 (ORBmatcher.cc:42-143)
 * Both are the monocular paths DefSLAM runs: no stereo branch (mvuRight, bForward / bBackward) and no rotation histogram
 * (compiled out by `if (false)` in the reference).  TH_HIGH is this reference's 75 (ORBmatcher.cc:35).  Candidates come from
 * Frame::GetFeaturesInArea (Frame.cc:421-480) over the grid of Frame::PosInGrid (Frame.cc:484-496): |dx| < r and |dy| < r, octave in
 * [min level, max level], visiting order column, row, index; the best is the first strictly smaller Hamming distance in that order.
 * Queries interact within a call exactly as in the reference: a key point assigned to an earlier query holds a map point with
 * observations and is no candidate for a later one.  match[] is bit-exact.
 * Key point state on input (state[j]): 0 no map point, 1 a map point with observations (never a candidate), 2 a map point without
 * observations (a candidate; frame to frame drops a best that lands on it, ORBmatcher.cc:1462; the local map overwrites it).
 * DefTracking.cc:358 calls DefORBmatcher's copy of the frame-to-frame search (Modules/Matching/DefORBmatcher.cc:296-420): it also
 * skips bad points and points without a facet (the caller leaves them out of the queries) and overwrites instead of dropping; the
 * two agree whenever no key point enters in state 2, which TrackWithMotionModel guarantees by clearing mvpMapPoints first (:353).
 * Arithmetic (OpenCV internals restated): Rcw * x + tcw is three float32 products summed in row order with tcw added in double and
 * rounded once; frame to frame forms invzc = 1.0 / z in double and rounds it to float; isInFrustum forms invz = 1.0f / z in float,
 * dist = cv::norm(P - Ow) as the double square root of the double sum of squares rounded to float, viewCos = float(double dot(PO, Pn)
 * / dist); PredictScale takes ::log(double) of the float ratio mfMaxDistance / dist.  No FMA contraction anywhere.  isInFrustum has
 * no distance-range test in DefSLAM (min / max distance are computed and never used) and none is applied here.  A projection that is
 * NaN (a point exactly on the camera plane) is not in view and matches nothing.  The reference's NaN bounds tests pass, so its
 * isInFrustum reports such a point in view (in_view / level / uv / view_cos differ there), and its window arithmetic on NaN is undefined
 * behaviour; no other input is affected.
 * Limits: N <= 8192 key points, grid_cols * grid_rows <= 8192, levels <= 32, octaves < 128, at most 4096 candidates in one query's
 * window; beyond them DSH_ERR_ARG.  A host-only context returns DSH_ERR_NO_DEVICE (no CPU fallback). */
typedef struct dsh_track_frame {
  const float* Tcw;            /* 4x4 row-major float32 (CurrentFrame.mTcw) */
  float Ow[3];                 /* camera centre (Frame::mOw, float32); read by the local-map search only */
  float K[4];                  /* Frame::fx, fy, cx, cy */
  float bounds[4];             /* mnMinX, mnMaxX, mnMinY, mnMaxY */
  int32_t grid_cols, grid_rows;/* FRAME_GRID_COLS, FRAME_GRID_ROWS (64, 48) */
  int32_t levels;              /* mnScaleLevels */
  const float* scale_factors;  /* mvScaleFactors[levels] */
  float log_scale_factor;      /* mfLogScaleFactor */
  int32_t N;                   /* key points */
  const float* kp;             /* N x 2 mvKeysUn pixel positions */
  const int32_t* octave;       /* N  mvKeysUn[j].octave */
  const uint8_t* desc;         /* N x 32 mDescriptors rows */
  const uint8_t* state;        /* N  0 / 1 / 2 as above */
} dsh_track_frame;

#define DSH_TRACK_FRAME 0      /* frame to frame (motion model) */
#define DSH_TRACK_LOCAL 1      /* local map */
/* One search of a batch.  Inputs: the frame, the mode, th and the Q queries in the reference's order.
 *   frame to frame  the last frame's map points that are present and not outliers, in last-frame index order: xyz (world position,
 *                   float32, e.g. dsh_sft_result.mappoint_xyz), octave (LastFrame.mvKeys[i].octave), desc (GetDescriptor)
 *   local map       mvpLocalMapPoints in its order (DefTracking::UpdateLocalPoints copies a std::set<MapPoint*>): xyz, normal
 *                   (GetNormal), max_distance (mfMaxDistance), desc, skip (may be NULL: points already matched in this frame or bad,
 *                   Tracking.cc:1446-1451)
 * Outputs: match[Q] = key point index or -1; local map also (each may be NULL) in_view (mbTrackInView), level (mnTrackScaleLevel),
 * uv (Q x 2 mTrackProjX, mTrackProjY) and view_cos (mTrackViewCos), zero where not in view; nmatches (the function's return value)
 * and rescans (queries whose matches phase B had to search again: a measurement, not a result). */
typedef struct dsh_track_problem {
  dsh_track_frame frame;
  int32_t mode;                /* DSH_TRACK_FRAME or DSH_TRACK_LOCAL */
  float th;                    /* frame to frame: 20, then 25 (DefTracking.cc:358,368); local map: 3 (5 after a relocalisation) */
  int32_t Q;
  const float* xyz;            /* Q x 3 */
  const int32_t* octave;       /* Q, frame to frame */
  const float* normal;         /* Q x 3, local map */
  const float* max_distance;   /* Q, local map */
  const uint8_t* desc;         /* Q x 32 */
  const uint8_t* skip;         /* Q, local map, may be NULL */
  int32_t* match;              /* out Q */
  uint8_t* in_view;            /* out Q, local map */
  int32_t* level;              /* out Q, local map */
  float* uv;                   /* out Q x 2, local map */
  float* view_cos;             /* out Q, local map */
  int32_t nmatches;            /* out */
  int32_t rescans;             /* out */
} dsh_track_problem;
/* B independent searches (different frames, sizes and modes) in one upload, three launches and one download; a search's result does
 * not depend on the rest of the batch. */
int dsh_search_by_projection_batch(dsh_ctx* ctx, int B, dsh_track_problem* problems);
/* ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, true) (ORBmatcher.cc:1360-1510): the batch of one. */
int dsh_search_by_projection_frame(dsh_ctx* ctx, const dsh_track_frame* frame, int Q, const float* xyz, const int32_t* octave,
                                   const uint8_t* desc, float th, int32_t* match, int32_t* nmatches);
/* Tracking::SearchLocalPoints after its bookkeeping (Tracking.cc:1440-1468): isInFrustum(pMP, 0.5) of every query that is not
 * skipped, then ORBmatcher(0.8).SearchByProjection(F, vpMapPoints, th) (ORBmatcher.cc:42-136).  The batch of one. */
int dsh_search_by_projection_local(dsh_ctx* ctx, const dsh_track_frame* frame, int Q, const float* xyz, const float* normal,
                                   const float* max_distance, const uint8_t* desc, const uint8_t* skip, float th, int32_t* match,
                                   uint8_t* in_view, int32_t* level, int32_t* nmatches);

/* ---- map point upkeep: distinctive descriptor, normal and depth range ----------------------------------------------------
 * Two MapPoint methods keep the inputs of the local-map search current:
 *   descriptor      MapPoint::ComputeDistinctiveDescriptors   Thirdparty/ORBSLAM_2/src/MapPoint.cc:257-325
 *   normal, depth   MapPoint::UpdateNormalAndDepth            MapPoint.cc:348-391
 * called from LocalMapping::ProcessNewKeyFrame (LocalMapping.cc:142-161, via DefLocalMapping.cc:160-164: both, for every map point of
 * the new keyframe that it does not yet observe), DefLocalMapping::CreateNewMapPoints (DefLocalMapping.cc:340-341: both),
 * DefTracking::MonocularInitialization (DefTracking.cc:610-611: both) and DefMapPoint::Repose (DefMapPoint.cc:122-126, from
 * TriangularMesh.cc:192: normal and depth only).
 * dsh_kfdb keeps what these read of every keyframe resident in HBM: the descriptor rows, the octaves of mvKeysUn, the camera centre,
 * the scale pyramid and the bad flag (descriptor rows, octaves, centre and pyramid on the device; the bad flag of this store stays on
 * the host, where dsh_mappoint_update lists the election rows).  A keyframe is copied up once, when it is added.  Keyframe poses change in exactly one place after
 * insertion in DefSLAM (there is no keyframe bundle adjustment): the surface registration calls refKF->SetPose
 * (Modules/Mapping/SurfaceRegistration.cc:150), which moves the camera centre.  dsh_keyframe_register writes the new centre into this
 * store itself, and dsh_keyframe_set_pose is the call for any other caller of SetPose.  Lifetime as dsh_diffdb: a store belongs to the
 * context it was created on; dsh_destroy of that context detaches it -- every call on it then returns DSH_ERR_ARG -- and
 * dsh_kfdb_destroy works before or after dsh_destroy. */
typedef struct dsh_kfdb dsh_kfdb;
typedef struct dsh_mp_keyframe {
  float Ow[3];                 /* GetCameraCenter(), float32 */
  int32_t N;                   /* key points */
  const uint8_t* desc;         /* N x 32 mDescriptors rows */
  const int32_t* octave;       /* N  mvKeysUn[j].octave, 0 .. 127 */
  int32_t levels;              /* mnScaleLevels, 1 .. 32 */
  const float* scale_factors;  /* mvScaleFactors[levels] */
  int32_t bad;                 /* isBad() */
} dsh_mp_keyframe;
/* capacity is the initial number of keyframes; the store grows on demand (descriptor rows too). */
int dsh_kfdb_create(dsh_ctx* ctx, int32_t capacity, dsh_kfdb** out);
int dsh_kfdb_destroy(dsh_kfdb* db);
int dsh_kfdb_clear(dsh_kfdb* db);                                       /* forget every keyframe (DefMap::clear on a reset) */
int dsh_kfdb_add(dsh_kfdb* db, const dsh_mp_keyframe* kf, int32_t* slot);/* copy one keyframe up; *slot = its index, 0, 1, 2 ... */
int dsh_kfdb_set_bad(dsh_kfdb* db, int32_t slot, int32_t bad);           /* KeyFrame::SetBadFlag */
int32_t dsh_kfdb_count(const dsh_kfdb* db);                             /* keyframes stored; -1 for NULL */

#define DSH_MP_DESCRIPTOR 1    /* what: ComputeDistinctiveDescriptors */
#define DSH_MP_NORMAL_DEPTH 2  /* what: UpdateNormalAndDepth */
#define DSH_MP_NO_OBS 1        /* status: no observations -- nothing changed, no output written but best (-1) and status */
#define DSH_MP_NO_GOOD_DESC 2  /* status: observations, none in a keyframe that is not bad -- descriptor unchanged (set whatever `what` asks) */
#define DSH_MP_MAX_OBS 65535
/* Updates P independent map points (the points of ProcessNewKeyFrame's loop do not interact, so one batch is exact).  The caller leaves
 * out bad points (both methods return at once on mbBad).
 * Inputs: xyz[P x 3] (mWorldPos, float32); the observations as CSR in the reference's iteration order (std::map<KeyFrame*, size_t>, so
 * the caller supplies that order): obs_ptr[P + 1], obs_kf[] (store slots), obs_idx[] (the key point index in that keyframe); ref_kf[P]
 * (the slot of mpRefKF; read only with DSH_MP_NORMAL_DEPTH); what = DSH_MP_DESCRIPTOR | DSH_MP_NORMAL_DEPTH.
 * Outputs (each may be NULL when `what` does not ask for it; a part not asked for is never written): desc[P x 32] in/out, left as it
 * was where the reference returns early; best[P] the index into the point's observations of the elected descriptor, or -1; normal[P x
 * 3], max_distance[P], min_distance[P]; status[P] (may be NULL) DSH_MP_* flags above.
 * Election (MapPoint.cc:257-325): only observations whose keyframe is not bad take part (:279-283); D is the full M x M Hamming matrix
 * with 0 on the diagonal (:292-304); the median of row i is sorted(row)[(size_t)(0.5 * (M - 1))], the element of rank floor((M-1)/2)
 * (:311-313); the winner is the first i with a strictly smaller median, ties go to the earliest observation (:315-319).  M = 1 elects
 * that descriptor; M = 2 has both medians 0 and elects index 0.  Integer valued: best and desc are bit-exact.
 * Normal (MapPoint.cc:366-377): the sum runs over ALL observations, bad keyframes included (UpdateNormalAndDepth does not test isBad),
 * in observation order, n counts every observation.  The sum is sequential: the order is part of the result.
 * Depth (MapPoint.cc:379-390): dist = cv::norm(Pos - Ow_ref) rounded to float; level = pRefKF->mvKeysUn[observations[pRefKF]].octave;
 * max = dist * scale_factors[level], min = max / scale_factors[levels - 1], both float.  Quirk, reproduced: operator[] on the copied map
 * yields index 0 when the reference keyframe is not among the observations, so key point 0 of the reference keyframe gives the octave.
 * Arithmetic (OpenCV 4 internals restated -- a reading of OpenCV's sources; no OpenCV build was available to check against):
 *   normali = mWorldPos - Owi                float32, per element
 *   cv::norm(normali)                        sqrt in double of the double sum ((x*x + y*y) + z*z) (normL2_32f)
 *   normal + normali / norm                  MatExpr builds AddEx(normal, normali, 1, 1.0/norm), assigned as
 *                                            cv::scaleAdd(normali, 1.0/norm, normal): alpha rounded to float, then per element
 *                                            normali * alpha + normal in float32 (scaleAdd_32f's scalar tail: 3 elements never reach
 *                                            its vector loop), product and sum rounded separately
 *   normal / n                               n > 1: Mat::convertTo with scale 1.0/n: a = (float)(1.0/n), normal * a + 0.0f in float32
 *                                            (cvt_32f's scalar path); n = 1: cv::add(normal, 0), which leaves it as it is
 *   dist, max, min                           (float)sqrt(double sum), then float products / quotient as above
 * No FMA contraction anywhere.  A point that coincides with a keyframe centre gives the reference's NaN (0 * inf), not a guard.
 * Limits: at most DSH_MP_MAX_OBS observations per point.  A point with more, a slot outside the store, a slot repeated within one point
 * (the reference's map holds a keyframe once), obs_idx >= N of its keyframe, or a reference octave >= levels (checked only where it is
 * read) makes the call return DSH_ERR_ARG without writing any output.  Arguments are checked first: a host-only context (which has no
 * store) reports bad ones with DSH_ERR_ARG and then returns DSH_ERR_NO_DEVICE (no CPU fallback). */
int dsh_mappoint_update(dsh_ctx* ctx, dsh_kfdb* db, int P, const float* xyz, const int32_t* obs_ptr, const int32_t* obs_kf,
                        const int32_t* obs_idx, const int32_t* ref_kf, int32_t what, uint8_t* desc, int32_t* best, float* normal,
                        float* max_distance, float* min_distance, int32_t* status);

/* ---- tracking: the local map from a resident map point store ---------------------------------------------------------------
 * Tracking::UpdateLocalMap (Thirdparty/ORBSLAM_2/src/Tracking.cc:1472-1480) = Tracking::UpdateLocalKeyFrames (:1510-1629) +
 * DefTracking::UpdateLocalPoints (Modules/Tracking/DefTracking.cc:426-454), and Tracking::SearchLocalPoints (:1405-1470) fed from it.
 * dsh_mpdb keeps in HBM what these read of the map:
 *   points      id 0, 1, 2 ... in creation order: mWorldPos (float32), the normal, mfMaxDistance, the 32-byte descriptor, the bad flag
 *   observations  MapPoint::mObservations, the point-side relation, as an append-only log of (point id, keyframe slot) records; an
 *               erased record is blanked in place.  A host mirror finds a pair's record and refuses a pair that is already there
 *               (MapPoint::AddObservation, MapPoint.cc:88-91).  Beside the log lies the key point index of each observation in its
 *               keyframe (dsh_point_store_add_observations_indexed; -1 for a record added without one), and per point its reference
 *               keyframe mpRefKF as a slot (dsh_point_store_set_reference_keyframes; -1: not given).  The tracking entries read neither
 *   keyframes   slot 0, 1, 2 ... in insertion order -- add keyframes to dsh_kfdb and to this store in the same order and the numbers
 *               agree: N, the keyframe-side table mvpMapPoints (a point id or -1 per key point), the parent in the spanning tree (a
 *               slot or -1, KeyFrame::GetParent; the children of a keyframe are the slots whose parent it is) and the bad flag
 * Both relations are stored because the reference reads both -- votes go through the points' observations, local points through the
 * keyframes' tables -- and between CreateNewKeyFrame and LocalMapping::ProcessNewKeyFrame they disagree.
 * ORDER.  The reference iterates std::map<KeyFrame*, int>, std::set<KeyFrame*> and std::set<MapPoint*> in pointer order.  Here, as
 * everywhere in this library, index order stands for pointer order: keyframes by ascending slot, points by ascending id.
 * Lifetime as dsh_kfdb: a store belongs to the context of its descriptor; dsh_destroy of that context detaches it -- every call on it
 * then returns DSH_ERR_ARG -- and the store's own destroy works before or after.  Every entry point takes the store alone (it remembers
 * its context, runs on that context's stream and reports through that context's dsh_last_error).  Arguments are checked on the host
 * before any device work: ids and slots outside the store, an index >= N, a NULL array with n > 0 or an id repeated within one batch
 * give DSH_ERR_ARG, and nothing is stored or written.  A store can be created on a host-only context: it checks arguments (against
 * an empty store) and then returns DSH_ERR_NO_DEVICE -- there is no CPU fallback. */
typedef struct dsh_mpdb dsh_mpdb;
typedef struct dsh_mpdb_desc {
  dsh_ctx* ctx;                /* the owning context */
  int32_t point_capacity;      /* initial capacities (> 0); the store grows on demand */
  int32_t keyframe_capacity;
  int64_t observation_capacity;
} dsh_mpdb_desc;
int dsh_mpdb_create(const dsh_mpdb_desc* desc, dsh_mpdb** out);
int dsh_mpdb_destroy(dsh_mpdb* db);
int dsh_mpdb_clear(dsh_mpdb* db);                         /* forget everything, the local map included (DefMap::clear on a reset) */
int32_t dsh_mpdb_point_count(const dsh_mpdb* db);         /* points stored; -1 for NULL */
int32_t dsh_mpdb_keyframe_count(const dsh_mpdb* db);      /* keyframes stored; -1 for NULL */
/* n new points: xyz[n x 3], normal[n x 3], max_distance[n], desc[n x 32], bad[n] (may be NULL: none is bad); *first_id (may be NULL) =
 * the id of the first one, the others follow. */
int dsh_mpdb_add_points(dsh_mpdb* db, int n, const float* xyz, const float* normal, const float* max_distance, const uint8_t* desc,
                        const uint8_t* bad, int32_t* first_id);
#define DSH_MPDB_POSITION 1      /* what: xyz */
#define DSH_MPDB_NORMAL_DEPTH 2  /* what: normal and max_distance (the outputs of dsh_mappoint_update) */
#define DSH_MPDB_DESCRIPTOR 4    /* what: desc */
/* Overwrite the parts `what` selects of the n distinct points ids[n]; arrays of parts not selected are not read.  The per-frame use is
 * the write-back of DefMapPoint::RecalculatePosition after the pose optimisation (dsh_sft_result.mappoint_xyz, DSH_MPDB_POSITION). */
int dsh_mpdb_update_points(dsh_mpdb* db, int n, const int32_t* ids, int32_t what, const float* xyz, const float* normal,
                           const float* max_distance, const uint8_t* desc);
/* MapPoint::SetBadFlag of n distinct points; bad[n] may be NULL (all become bad).  The flag alone: dsh_point_store_set_bad is setBadFlag
 * in full, with the point's observation records and table entries. */
int dsh_mpdb_set_points_bad(dsh_mpdb* db, int n, const int32_t* ids, const uint8_t* bad);
/* MapPoint::AddObservation / EraseObservation for n (point, keyframe) pairs.  Adding a pair that is stored, or twice in one batch, is
 * DSH_ERR_ARG; erasing a pair that is not stored changes nothing, like the reference.  The erase blanks the record and decrements
 * n_obs only: dsh_point_store_erase_observations also moves the reference keyframe and runs the n_obs <= 2 cascade. */
int dsh_mpdb_add_observations(dsh_mpdb* db, int n, const int32_t* point_ids, const int32_t* keyframe_slots);
int dsh_mpdb_erase_observations(dsh_mpdb* db, int n, const int32_t* point_ids, const int32_t* keyframe_slots);
/* dsh_mpdb_add_observations with the key point index of each observation, mObservations[pKF] = idx (MapPoint.cc:88-91): in addition
 * 0 <= idx[i] < N of keyframe keyframe_slots[i], else DSH_ERR_ARG and nothing is stored.  A record added by the call without indices
 * has none; the store counts its live records without an index, and erasing one takes it out of that count (dsh_keyframe_anchors). */
int dsh_point_store_add_observations_indexed(dsh_mpdb* db, int n, const int32_t* point_ids, const int32_t* keyframe_slots, const int32_t* idx);
/* MapPoint::GetReferenceKeyFrame of the n distinct points ids[n]: slots[n], each a slot of the store or -1 (not given, the state of a
 * point after dsh_mpdb_add_points).  The points dsh_template_switch creates have the switch's keyframe.  The read-back writes slots_out[n]. */
int dsh_point_store_set_reference_keyframes(dsh_mpdb* db, int n, const int32_t* ids, const int32_t* slots);
int dsh_point_store_get_reference_keyframes(dsh_mpdb* db, int n, const int32_t* ids, int32_t* slots_out);
/* A keyframe with its table points[N] (ids or -1) and its parent (an existing slot or -1); *slot (may be NULL) = its slot. */
int dsh_mpdb_add_keyframe(dsh_mpdb* db, int32_t N, const int32_t* points, int32_t parent, int32_t bad, int32_t* slot);
/* KeyFrame::AddMapPoint / EraseMapPointMatch: table entry idx of the keyframe becomes point_id (or -1). */
int dsh_mpdb_set_keyframe_point(dsh_mpdb* db, int32_t slot, int32_t idx, int32_t point_id);
int dsh_mpdb_set_keyframe_parent(dsh_mpdb* db, int32_t slot, int32_t parent);   /* KeyFrame::ChangeParent; parent != slot, or -1 */
int dsh_mpdb_set_keyframe_bad(dsh_mpdb* db, int32_t slot, int32_t bad);         /* KeyFrame::SetBadFlag */

/* Tracking::UpdateLocalMap for the frame whose mvpMapPoints are frame_points[N] (ids or -1).  Integer valued: every output is exact.
 * Outputs (each may be NULL): frame_bad[N] = 1 where the frame holds a bad point (the reference nulls that entry, Tracking.cc:1527-1530);
 * local_kf[] = mvpLocalKeyFrames as slots and local_votes[] = the votes of its first *n_voted entries, both of kf_capacity entries, which
 * must be at least the store's keyframe count when either is given (the list holds a keyframe at most once); *n_local_kf its length;
 * *ref_kf = the slot of pKFmax, or -1: leave mpReferenceKF as it is; *n_local_points = the size of mvpLocalMapPoints.  The two lists
 * stay resident in the store for the next call and for dsh_local_map_search.
 * Votes (:1513-1532): a frame entry votes once for every keyframe among its point's observations, so a point held by k key points of
 * the frame votes k times; bad points do not vote; erased observations do not count.
 * No vote at all (:1534): the previous local keyframe list stays, *n_voted = 0, *ref_kf = -1; the local points are still rebuilt from
 * that list (UpdateLocalMap calls UpdateLocalPoints regardless).
 * Local keyframes (:1545-1562): the voted keyframes that are not bad, by ascending slot; pKFmax is the first of them with a strictly
 * larger vote (a tie goes to the lower slot).  When every voted keyframe is bad the list is empty and *ref_kf = -1.
 * Expansion (:1566-1622), literally: the loop visits the voted entries only (its end iterator is taken before the pushes) and stops
 * once the list holds more than 80; per visited keyframe it appends at most three: the first keyframe of the whole map, by ascending
 * slot, that is not bad and not yet listed (the reference iterates Map::GetAllKeyFrames there; its covisibility call is commented
 * out, :1576-1577); the first child that is not bad and not yet listed; and the parent when it is not yet listed -- without a test of
 * its bad flag, and appending it ends the whole loop (the break at :1619 leaves the outer for).
 * Local points (DefTracking.cc:426-454): the points in the tables of the local keyframes that are not bad, by ascending id. */
int dsh_local_map_update(dsh_mpdb* db, int N, const int32_t* frame_points, uint8_t* frame_bad, int32_t kf_capacity, int32_t* local_kf,
                         int32_t* local_votes, int32_t* n_voted, int32_t* n_local_kf, int32_t* ref_kf, int32_t* n_local_points);
/* The resident local point list of the last update: ids[capacity] receives *n ids (DSH_ERR_ARG when capacity is smaller). */
int dsh_local_map_points(dsh_mpdb* db, int32_t capacity, int32_t* ids, int32_t* n);
/* Tracking::SearchLocalPoints (:1440-1468) with the resident local points as queries, in ascending id: position, normal, max distance
 * and descriptor are gathered from the store on the device, only the frame's key points travel up, and the kernels of
 * dsh_search_by_projection_local run on them.  A query is skipped when its point is bad or was held by a key point of the frame of the
 * preceding dsh_local_map_update (mnLastFrameSeen == mnId after the loop at :1408-1425 says exactly that, :1449-1451).
 * frame->state[] as for DSH_TRACK_LOCAL.  Outputs of Q = n_local_points entries, capacity >= Q: local_ids (may be NULL), match, and
 * (each may be NULL) in_view, level, uv[Q x 2], view_cos, *nmatches.  Limits and refusals as dsh_search_by_projection_batch. */
int dsh_local_map_search(dsh_mpdb* db, const dsh_track_frame* frame, float th, int32_t capacity, int32_t* local_ids, int32_t* match,
                         uint8_t* in_view, int32_t* level, float* uv, float* view_cos, int32_t* nmatches);

/* ---- tracking: closing a tracked frame on the resident map point store --------------------------------------------------------
 * The back half of DefTracking::TrackLocalMap (Modules/Tracking/DefTracking.cc:253-339) and what it needs of the points:
 *   position write-back   DefPoseOptimization moves EVERY map point with a facet, observed or not (Modules/Tracking/DefOptimizer.cc:568-576,
 *                         DefMapPoint::RecalculatePosition, Modules/Common/DefMapPoint.cc:129-147)
 *   counting loops        IncreaseFound, mnMatchesInliers, the Matches.txt row, numberLocalMapPoints (DefTracking.cc:253-319)
 *   culling               LocalMapping::MapPointCulling (Thirdparty/ORBSLAM_2/src/LocalMapping.cc:173-199), which reads mnFound / mnVisible
 * dsh_mpdb therefore also keeps per point, resident, growing with the point arrays and forgotten by dsh_mpdb_clear:
 *   visible, found  mnVisible / mnFound; both 1 for a new point (MapPoint.cc:38,58).  dsh_local_map_search adds to visible what
 *                   Tracking::SearchLocalPoints does: +1 per key point of the frame of the preceding dsh_local_map_update that holds the
 *                   point when it is not bad (Tracking.cc:1408-1425; a point held twice gets +2) and +1 per query reported in view (:1456)
 *   n_obs           MapPoint::nObs, monocular: +1 per pair dsh_mpdb_add_observations stores, -1 per pair dsh_mpdb_erase_observations
 *                   finds (MapPoint.cc:114-133).  STALE ON PURPOSE: setBadFlag clears mObservations and leaves nObs (DefMapPoint.cc:76-94),
 *                   so setting a point bad here leaves n_obs, and TrackLocalMap's Observations() > 0 test (:266) reads the stale number
 *   nodes, bary     DefMapPoint::facet as its three node indices in ascending order (std::set<Node*> order, index for pointer) with
 *                   b1..b3 in that order -- the convention of dsh_sft_frame.obs_nodes / obs_bary; nodes -1 -1 -1: no facet
 *   reference list  Map::GetReferenceMapPoints() as TrackLocalMap reads it at :284.  Tracking::UpdateLocalMap calls
 *                   SetReferenceMapPoints(mvpLocalMapPoints) BEFORE it rebuilds that list (Tracking.cc:1475), so this is the local point
 *                   list of the PREVIOUS frame: dsh_local_map_update keeps the list it found (two buffers that swap).  Empty before
 *                   the first dsh_local_map_update or dsh_trackstate_seed_local_points
 * Discipline of the other store calls: arguments are checked on the host first -- an id outside the store, an id repeated within one
 * batch, NULL with n > 0 give DSH_ERR_ARG with a message naming the entry, and nothing is stored; then a host-only context answers
 * DSH_ERR_NO_DEVICE; a detached store answers DSH_ERR_ARG.  Integer valued but for the positions, which are the reference's expression
 * rounded the same way: every output is exact. */
/* DefMapPoint::SetFacet + SetCoordinates (DefMapPoint.cc:97-118) of the n distinct points ids[n]: nodes[n x 3] ascending and distinct,
 * bary[n x 3] in that order; nodes -1 -1 -1 removes the facet (bary may be NULL when every entry does). */
int dsh_trackstate_set_embedding(dsh_mpdb* db, int n, const int32_t* ids, const int32_t* nodes, const double* bary);
/* DefMap::clearTemplate (Modules/Common/DefMap.cc:75-81): every point loses its facet. */
int dsh_trackstate_clear_embedding(dsh_mpdb* db);
/* Overwrite mnVisible / mnFound of n distinct points (a loaded map; MapPoint::Replace, MapPoint.cc:223-224, is get + set by the caller). */
int dsh_trackstate_set_counters(dsh_mpdb* db, int n, const int32_t* ids, const int32_t* visible, const int32_t* found);
/* Read back n distinct points; each output may be NULL: visible[n], found[n], n_obs[n], xyz[n x 3]. */
int dsh_trackstate_get(dsh_mpdb* db, int n, const int32_t* ids, int32_t* visible, int32_t* found, int32_t* n_obs, float* xyz);
/* DefTracking::MonocularInitialization (DefTracking.cc:641,645): mvpLocalMapPoints = GetAllMapPoints() and SetReferenceMapPoints of it --
 * the resident local list AND the reference list become ids[n] (ascending, distinct). */
int dsh_trackstate_seed_local_points(dsh_mpdb* db, int n, const int32_t* ids);
/* DefOptimizer.cc:568-576 on its own: every point that is not bad (setBadFlag erased those from the map the loop walks) and has a facet
 * moves to (float)((b1 * x[n1] + b2 * x[n2]) + b3 * x[n3]) per coordinate, every product and sum rounded to nearest in double, no
 * contraction -- the expression of dsh_sft_result.mappoint_xyz, so the observed points get those very bytes.  node_xyz[n_nodes x 3] is e.g.
 * dsh_sft_result.xyz.  A stored node index >= n_nodes is DSH_ERR_ARG and nothing moves.  *n_moved (may be NULL) = points moved. */
int dsh_trackstate_repose(dsh_mpdb* db, int n_nodes, const double* node_xyz, int32_t* n_moved);
/* LocalMapping::MapPointCulling (LocalMapping.cc:173-199) over mlpRecentAddedMapPoints = ids[n] (distinct), first_kf[n] = mnFirstKFid,
 * current_kf = mpCurrentKeyFrame->mnId.  Per point, the first case that applies: action[n] = 1 already bad (leaves the list); 2
 * (float)found / (float)visible < 0.40f: the store sets the point's bad flag (leaves the list); 3 (int)current_kf - first_kf >= 3 (leaves
 * the list); 0 stays.  Setting bad is what dsh_mpdb_set_points_bad does: observation records, n_obs and table entries are untouched (bad
 * points neither vote nor become local points); KeyFrame::EraseMapPointMatch stays with the caller, who knows the index.
 * dsh_point_store_cull takes the same decisions and erases the records and table entries of the action-2 points as well. */
int dsh_trackstate_cull(dsh_mpdb* db, int n, const int32_t* ids, const int32_t* first_kf, int32_t current_kf, uint8_t* action);

typedef struct dsh_track_close_counts {
  int32_t matches_inliers, matches_outliers, to_match_local;   /* mnMatchesInliers, mnMatchesOutliers, DefnToMatchLOCAL (DefTracking.cc:254-283) */
  int32_t observed, inliers, outliers;                         /* observedFrame, mI, mO: the Matches.txt row (:300-328) */
  int32_t local_map_points;                                    /* numberLocalMapPoints (:284-298) */
  int32_t n_moved;                                             /* points the repose moved; 0 without node_xyz */
} dsh_track_close_counts;
/* The rest of TrackLocalMap after the optimisation, in the reference's order.  frame: only Tcw, Ow, K and bounds are read (the pose AFTER
 * SetPose, DefOptimizer.cc:566).  frame_points[N] = mvpMapPoints as ids or -1, outlier[N] = mvbOutlier.
 *   1. repose as dsh_trackstate_repose when node_xyz[n_nodes x 3] is given (NULL: no position changes)
 *   2. :257-283 per key point i with a point p: !outlier[i] gives found[p] += 1 (per key point, NO bad test), then with only_tracking == 0
 *      matches_inliers++ when n_obs[p] > 0 and also to_match_local++ when p has a facet, with only_tracking != 0 matches_inliers++
 *      unconditionally; outlier[i] gives matches_outliers++
 *   3. :284-298 local_map_points = the entries of the reference list that are not bad, have a facet and pass Frame::isInFrustum(pMP, 0.5)
 *      at the given pose -- the test of dsh_local_map_search (no distance range; a NaN projection is not in view), on the moved positions
 *   4. :300-319 held and not bad gives observed++, then inliers++ or outliers++
 * One upload (pose, ids, flags, nodes), at most three launches, one download of the counts.  N <= 2^20. */
int dsh_track_close_frame(dsh_mpdb* db, const dsh_track_frame* frame, int N, const int32_t* frame_points, const uint8_t* outlier,
                          int n_nodes, const double* node_xyz, int32_t only_tracking, dsh_track_close_counts* out);

/* ---- tracking: the end of a frame and the next frame's motion-model search on the resident map point store ----------------------
 * What DefTracking::Track does with mvpMapPoints after a successful TrackLocalMap (Modules/Tracking/DefTracking.cc:169-172, :185-191,
 * :211) and what TrackWithMotionModel (:342-375) reads of the frame that results, mLastFrame.  The store keeps that frame's point list
 * resident -- per key point of the last frame the id it holds or -1, and the key point's octave -- so the next frame's first search
 * sends up its own key points only.  dsh_mpdb_clear forgets the list.  Discipline of the other store calls: arguments are checked on
 * the host first and DSH_ERR_ARG names the entry, nothing is stored or changed; then a host-only context answers DSH_ERR_NO_DEVICE;
 * a detached store answers DSH_ERR_ARG.  Integer valued: every output is exact. */
typedef struct dsh_track_end_counts {
  int32_t cleaned;   /* entries CleanMatches emptied */
  int32_t dropped;   /* outliers the loop at :185-191 emptied */
  int32_t kept;      /* entries of the resident last-frame list that hold a point */
} dsh_track_end_counts;
/* frame_points[N] = mvpMapPoints as ids or -1, outlier[N] = mvbOutlier, octave[N] = mvKeys[i].octave, in the reference's order:
 *   1. CleanMatches (:667-679): an entry whose point has n_obs < 1 becomes -1 and its outlier flag 0.  n_obs is the store's, stale
 *      after a bad flag exactly as Observations() is (see n_obs above); there is no bad test, as in the reference.
 *   2. points_out[N], outlier_out[N] (each may be NULL) = the state after step 1: what CreateNewKeyFrame copies into a keyframe,
 *      outliers included (:175-178).
 *   3. The outlier drop (:185-191): an entry that still holds a point and is an outlier becomes -1; its flag stays 1.
 *   4. mLastFrame = Frame(*mCurrentFrame) (:211): the store keeps the result of steps 1 and 3 and octave[] as the resident last-frame
 *      list of N entries, in place of the previous one.
 *   5. *out (may be NULL) = the counts.
 * N in [0, 8192], octaves in [0, 128).  One upload, one launch, one download.  DefTracking::MonocularInitialization (:637) makes the
 * same call with the initial frame's points. */
int dsh_track_end_frame(dsh_mpdb* db, int N, const int32_t* frame_points, const uint8_t* outlier, const int32_t* octave, int32_t* points_out,
                        uint8_t* outlier_out, dsh_track_end_counts* out);
/* The resident last-frame list read back: ids[capacity] and octave[capacity] (each may be NULL) receive its *n entries, the id or -1
 * and the octave (-1 where the entry is empty).  DSH_ERR_ARG when capacity is smaller or when there is no list. */
int dsh_track_last_frame(dsh_mpdb* db, int32_t capacity, int32_t* ids, int32_t* octave, int32_t* n);
/* THE KEYFRAME CANDIDATE.  dsh_track_end_frame also keeps the state after its step 1 resident, beside the last-frame list: the N ids
 * it writes to points_out, outliers still held, cleaned entries -1.  It is the table DefTracking::CreateNewKeyFrame copies into a new
 * keyframe (:175-178, :696-707), and dsh_keyframe_create reads it on the device when it is given no table.  It is replaced by the next
 * dsh_track_end_frame, is not consumed by a keyframe made from it, and dsh_mpdb_clear forgets it with the last-frame list.  This reads
 * it back: ids[capacity] (may be NULL) receives its *n entries; DSH_ERR_ARG when capacity is smaller or when there is no candidate. */
int dsh_track_keyframe_candidate(dsh_mpdb* db, int32_t capacity, int32_t* ids, int32_t* n);
/* DefTracking::TrackWithMotionModel (:342-375) after SetPose: DefORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, true)
 * (Modules/Matching/DefORBmatcher.cc:296-424) with the resident last-frame list as LastFrame, and again with th_wide on cleared
 * mvpMapPoints when the first search finds fewer than min_matches (:364-370).  The reference passes th = 20, th_wide = 25,
 * min_matches = 20; the caller applies nmatches < 15 (:373).  frame is the current frame at the pose the caller set (:350);
 * frame->state is not read and may be NULL: mvpMapPoints are cleared first (:352-353), every key point enters empty.
 * Queries: the entries of the list that hold a point, in index order (the last frame's outliers left it at the end of that frame).
 * A query whose point is bad (:329-332) or has no facet (:331) is skipped, on the device and at call time; position, descriptor and
 * n_obs are the store's at call time, the octave is the list's.  An octave >= frame->levels in the list is DSH_ERR_ARG.
 * Projection, window, octave band [o - 1, o + 1], visiting order, strict-less best and TH_HIGH = 75 are those of DSH_TRACK_FRAME,
 * by the same kernels; the arithmetic notes above dsh_track_frame apply unchanged.  No rotation histogram (mbCheckOrientation is false).
 * Overwrite semantics, literally: a key point is no candidate only while the point it holds has Observations() > 0 (:381-383); :406
 * assigns and :407 counts whatever the key point held.  So the pick of a query whose point has n_obs == 0 does not block its key
 * point, a later query may take it again, the last writer in query order owns the entry and *nmatches counts both.
 * Outputs: frame_points[frame->N] = mvpMapPoints as ids or -1; match[n] (may be NULL; n = the length of the list) = the key point each
 * last-frame entry took, -1 for an empty, skipped or unmatched entry; *nmatches = the return value of the search that produced them;
 * *th_used = th or th_wide, whichever search that was (each may be NULL).
 * One upload (the frame), at most six launches -- the gather of the queries with its ordered compaction, the grid, and two search
 * phases per pass; the wide pass is enqueued behind the narrow one and leaves at its first instruction when the narrow count
 * suffices, there is no host read-back in between -- and one download.  Limits and refusals as dsh_search_by_projection_batch.  After
 * the device gate: no resident list (before the first dsh_track_end_frame, after dsh_mpdb_clear) is DSH_ERR_ARG.  The call changes
 * nothing in the store, the list included. */
int dsh_motion_model_search(dsh_mpdb* db, const dsh_track_frame* frame, float th, float th_wide, int32_t min_matches, int32_t* frame_points,
                            int32_t* match, int32_t* nmatches, float* th_used);

/* ---- tracking: the rigid pose-only optimisation of a frame from the resident map point store -----------------------------------
 * The else branch of DefTracking::TrackLocalMap (Modules/Tracking/DefTracking.cc:250), which runs while the map has no template, and
 * what Tracking::Relocalization and TrackReferenceKeyFrame call: ORB_SLAM2::Optimizer::poseOptimization(Frame*)
 * (Thirdparty/ORBSLAM_2/src/Optimizer.cc:236-445), monocular branch only (mvuRight < 0 always holds here: no stereo branch).  One SE3
 * vertex, one unary reprojection edge (EdgeSE3ProjectXYZOnlyPose, types_six_dof_expmap.h:143-172, .cpp:266-296) per key point that
 * holds a point; the positions are read from the store by id on the device, nothing per map point crosses the bus.
 *   Edges (:276-315): every key point with frame_points[i] >= 0, in index order; there is no bad test, and an id may be held by several
 *     key points (one edge each).  outlier[i] is cleared first.  Xw = the store's float32 position, measurement = the float32 key
 *     point, both widened to double; information = I2 * (double)inv_level_sigma2[octave[i]] (no division by N); Huber with
 *     delta = (float)sqrt(5.991) (robust_kernel_impl.cpp:78-91).
 *   Early return (:358-359): n_initial < 3 returns n_good = 0 with rounds = 0; Tcw_out and pose are the input pose, the flags stay 0.
 *   Four rounds (:368-436).  Each restarts from the input pose (Converter::toSE3Quat of the float32 matrix, :371) with the edges at
 *     level 0, i.e. those not flagged, and runs optimize(10): g2o's Levenberg-Marquardt (optimization_algorithm_levenberg.cpp:61-164)
 *     with lambda = 1e-5 * max|diag H| at the round's first iteration, at most 10 trials per iteration, the accept / reject rule, the
 *     stops on 10 trials, rho == 0 and _nBad >= 3; the 6x6 system goes through LinearSolverDense (Eigen's pivoted LDLT on H + lambda I,
 *     block_solver.hpp:356-365: no landmark vertex, no Schur complement), a factor that is not positive makes the trial's chi2 DBL_MAX;
 *     the update is SE3Quat::exp(dx) * estimate (se3quat.h:223-257).  A round without a level-0 edge does not optimise
 *     (sparse_optimizer.cpp:405-409): its estimate is the input pose.
 *   Classification after a round (:376-403): an edge flagged outlier recomputes its error at the round's estimate; an inlier edge keeps
 *     the error of the last trial evaluated, also when that trial was rejected and popped (the quirk of DefOptimizer.cc:515-537).
 *     chi2 = e' Omega e rounded to float, outlier when > 5.991f; outliers go to level 1, inliers to level 0.  After round index 2 the
 *     robust kernel is removed from every edge: round 3 is plain least squares.
 *   The break (:434-435) counts all edges: n_initial in 3 .. 9 runs one round, n_initial >= 10 runs four.
 *   Result (:439-444): Tcw_out = Converter::toCvMat(estimate) in float32, n_good = n_initial - n_bad of the last round run.
 * Arithmetic: double throughout.  The sums over the edges of a linearisation (the 21 entries of the triangle of J' rho Omega J that
 * the factorisation reads, the 6 of the right-hand side, the robust chi2) are taken in a fixed order that depends on N alone (DESIGN
 * 4.6), not in edge order: the result is a function of the inputs, equal from run to run and from batch to single call, and differs
 * from a sequential evaluation by the reassociation of those sums.
 * Not covered: a point at or behind the camera plane, or any other non-finite residual.  The call then still returns a status and
 * does not fault, but the numbers it produces are not part of the contract.
 * Discipline of the other store calls: arguments are checked on the host first -- NULL arrays with N > 0, N outside 0 .. 8192, levels
 * outside 1 .. 32, an octave outside 0 .. levels-1, an id that is neither -1 nor a point of the store, B outside 0 .. 65536 -- and DSH_ERR_ARG names
 * the entry, nothing is written; then a host-only context answers DSH_ERR_NO_DEVICE; a detached store answers DSH_ERR_ARG.  The call
 * changes nothing in the store. */
typedef struct dsh_pose_only_problem {
  const float* Tcw;                 /* in: 4x4 row-major float32, pFrame->mTcw */
  float K[4];                       /* in: fx, fy, cx, cy */
  int32_t N;                        /* in: key points, 0 .. 8192 */
  const float* kp;                  /* in: N x 2 mvKeysUn */
  const int32_t* octave;            /* in: N, read where frame_points[i] >= 0 */
  int32_t levels;                   /* in: 1 .. 32 */
  const float* inv_level_sigma2;    /* in: levels, mvInvLevelSigma2 (ORBextractor.cc:430, float32) */
  const int32_t* frame_points;      /* in: N, mvpMapPoints as store ids, -1 = none */
  uint8_t* outlier;                 /* in/out: N, mvbOutlier; written only where frame_points[i] >= 0 (Optimizer.cc:285, :391-397) */
  float Tcw_out[16];                /* out: SetPose(Converter::toCvMat(...)); the input pose when n_initial < 3 */
  double pose[7];                   /* out: t, q (x y z w) of the recovered SE3Quat */
  int32_t n_initial, n_bad, n_good; /* out: nInitialCorrespondences, nBad of the last round run, the return value */
  int32_t rounds;                   /* out: rounds run: 0, 1 or 4 */
  int32_t iters[4], trials[4], bad[4];  /* out, per round: outer iterations, damping trials over all of them, nBad after it */
  double chi2[4];                   /* out, per round: the active robust chi2 of the last accepted state (0 for a round that did not optimise) */
} dsh_pose_only_problem;
/* One frame: dsh_track_pose_only_batch with B = 1. */
int dsh_track_pose_only(dsh_mpdb* db, dsh_pose_only_problem* p);
/* B frames against the same store (relocalisation candidates, an offline re-track): one upload of the poses, key points, octaves,
 * sigma tables and ids of the whole batch, one launch with one workgroup per problem that runs all rounds, their classifications and
 * the float32 conversion, one download of the flags and the result records.  A problem's result is that of its single call, bit for
 * bit.  B = 0 does nothing. */
int dsh_track_pose_only_batch(dsh_mpdb* db, int B, dsh_pose_only_problem* problems);

/* ---- tracking: Shape-from-Template of a tracked frame from the resident map point store ---------------------------------------
 * The if branch of DefTracking::TrackLocalMap and the call of DefTracking::Track (Modules/Tracking/DefTracking.cc:244, :115):
 * Optimizer::DefPoseOptimization (Modules/Tracking/DefOptimizer.cc:251-578) with its observation table built on the device from the
 * facet and the barycentrics the store holds per point (dsh_trackstate_set_embedding, dsh_template_switch), instead of the host-built
 * obs_nodes / obs_bary / obs_uv / obs_invsig2 of dsh_sft_frame.  Both entries take the store alone: the template is the current one of
 * the store's context.
 *   Selection (:293-361, literally): key point i gives a row when outlier[i] == 0, frame_points[i] >= 0, the point is not bad and the
 *     point has a facet.  A key point that holds a point and is no outlier counts in points_obs (Points_Obs of :300) whether the point
 *     is bad or not.  An id held by several key points gives one row each; the rows are in ascending key point index.  uv is the
 *     float32 key point widened to double, invsig2 is (double)inv_level_sigma2[octave[i]] (the division by N of :340 stays in the
 *     packer), nodes and bary are the store's bytes.
 *   dsh_track_sft_observations runs the selection and downloads the table.  The store and the context's SfT batch are unchanged.
 *   dsh_track_sft runs the selection, downloads the table once, then packs, plans, uploads and runs one problem exactly as
 *     dsh_sft_solve does on that table and on the other fields of the frame, and downloads the result once; its numbers are those of
 *     dsh_sft_solve on the same table on the same context, bit for bit.  The arrays of dsh_sft_result that dsh_sft_solve sizes by M
 *     (chi2_obs, outlier, mappoint_xyz) take N entries here, the first M of them are written.  Then outlier[kp_index[m]] =
 *     r->outlier[m] for every row; every other entry of outlier keeps its value (:515-537).  With write_back != 0 every point of the
 *     store that is not bad and has a facet moves as by dsh_trackstate_repose on r->xyz (:568-576), from the result's node positions
 *     where they lie in HBM; the frame is then closed with dsh_track_close_frame and node_xyz == NULL.  With write_back == 0 the store
 *     is unchanged.  The call replaces an uploaded SfT batch of the context, as dsh_sft_solve does.
 *   No row (M == 0) is NOT the reference's numbers (it runs an optimiser without observation edges): the call returns DSH_OK with
 *     inliers = iters = trials = dim = half_bandwidth = status = 0, rep_error NaN and Tcw, pose7 and xyz of the input; nothing is
 *     written back, the flags are untouched and the context's SfT batch stays.
 * Discipline of the other store calls: arguments are checked on the host first -- NULL arrays with N > 0, N outside 0 .. 8192, levels
 * outside 1 .. 32, an octave outside 0 .. levels-1 where frame_points[i] >= 0, an id that is neither -1 nor a point of the store, a
 * table array with capacity < M, a stored node index >= the nodes of the template -- and DSH_ERR_ARG names the entry, nothing is
 * written; no current template is DSH_ERR_STATE; then a host-only context answers DSH_ERR_NO_DEVICE; a detached store answers
 * DSH_ERR_ARG.  An observation whose nodes share no mesh edge of the template (a stale embedding) is refused by the packer with
 * DSH_ERR_ARG; the message names the observation and its key point. */
typedef struct dsh_track_sft_frame {
  const float* Tcw;                 /* 4x4 row-major float32, pFrame->mTcw */
  double K[4];                      /* fx, fy, cx, cy */
  int32_t N;                        /* pFrame->N, 0 .. 8192 */
  const float* kp;                  /* N x 2 mvKeysUn */
  const int32_t* octave;            /* N, read where frame_points[i] >= 0 */
  int32_t levels;                   /* 1 .. 32 */
  const float* inv_level_sigma2;    /* levels, mvInvLevelSigma2 */
  const int32_t* frame_points;      /* N: mvpMapPoints as store ids, -1 = none */
  uint8_t* outlier;                 /* N: mvbOutlier, in/out (dsh_track_sft_observations only reads it) */
  const double* xyz;                /* n x 3 current node positions */
  double reg_lap, reg_inex, reg_temp;
  int32_t neighbour_layers;         /* as in dsh_sft_frame */
  int32_t max_iters;                /* as in dsh_sft_frame */
} dsh_track_sft_frame;
typedef struct dsh_track_sft_table {
  int32_t capacity;                 /* in: entries each array that is given has room for; capacity >= M else DSH_ERR_ARG, N always suffices */
  int32_t M;                        /* out: rows */
  int32_t points_obs;               /* out: Points_Obs of :300 */
  int32_t* kp_index;                /* out, each array may be NULL: M, the key point of a row */
  int32_t* point_id;                /* M */
  int32_t* nodes;                   /* M x 3 */
  double* bary;                     /* M x 3 */
  double* uv;                       /* M x 2 */
  double* invsig2;                  /* M */
} dsh_track_sft_table;
int dsh_track_sft_observations(dsh_mpdb* db, const dsh_track_sft_frame* f, dsh_track_sft_table* t);
/* t may be NULL */
int dsh_track_sft(dsh_mpdb* db, const dsh_track_sft_frame* f, int32_t write_back, dsh_track_sft_table* t, dsh_sft_result* r);

/* ---- mapping meets tracking: the template switch on the resident map point store -----------------------------------------------
 * DefLocalMapping::updateTemplate (Modules/Mapping/DefLocalMapping.cc:138-153), which DefTracking::Track calls on the tracking thread
 * (Modules/Tracking/DefTracking.cc:109) in front of the frame's two pose optimisations, and the mapping thread's trigger
 * DefLocalMapping::needNewTemplate (:355-404), on dsh_mpdb and dsh_kfdb:
 *   DefMap::clearTemplate                  Modules/Common/DefMap.cc:67-82
 *   DefLocalMapping::CreateNewMapPoints    DefLocalMapping.cc:240-347
 *   DefMap::createTemplate                 TriangularMesh::TriangularMesh (Modules/Template/TriangularMesh.cc:57-89): Surface::getVertex
 *                                          (Modules/Mapping/Surface.cc:125-161), calculateFeaturesCoordinates, Repose
 * Discipline of the other store calls: arguments are checked on the host before any device work, DSH_ERR_ARG comes with a message that
 * names the entry and nothing is stored; a host-only context then answers DSH_ERR_NO_DEVICE; a detached store answers DSH_ERR_ARG.  No
 * CPU fallback.  The two entries that need more than the store take a descriptor that names the context or the keyframe store, the
 * way dsh_mpdb_create does.
 *
 * THE OCCUPANCY MASK (needNewTemplate :359-383, CreateNewMapPoints :245-271), restated in integers.  This is a reading of OpenCV's
 * documented filter2D / threshold semantics; no OpenCV build was available to check against, as for the other OpenCV restatements.
 *   held pixels   key point i of the keyframe's table marks pixel ((int)kp.y, (int)kp.x) -- the conversion truncates toward zero -- when
 *                 its table entry is a point that is not bad; several key points may share a pixel
 *   kernel        k = cols / 20 (integer division), a k x k box of ones, anchor a = k / 2: the window of pixel x is x - a .. x + k - 1 - a
 *                 in each axis (asymmetric for even k)
 *   border        BORDER_REFLECT_101: a source index p < 0 reads -p, p >= n reads 2 (n - 1) - p
 *   result        the 8-bit sum saturates and the threshold > 1 keeps every pixel whose window saw a held pixel (255 each): mask(y, x) != 0
 *                 exactly when at least one held pixel lies in the reflected window.  Nothing else of OpenCV's arithmetic survives
 * The device does not build the image: with lo = x - a, hi = x + k - 1 - a, L = max(lo, 0), H = min(hi, cols - 1), then H = max(H, -lo)
 * when lo < 0 and L = min(L, 2 (cols - 1) - hi) when hi > cols - 1, pixel x is masked by a held column px iff L <= px <= H, and alike
 * for the rows (tests/test_template_switch_cpu.py holds the two forms against each other).
 * Refused with DSH_ERR_ARG, because the reference's behaviour is undefined there: cols < 40 (k < 2); k >= rows or k >= cols; a key point
 * whose pixel lies outside [0, cols) x [0, rows) (the reference writes outside the cv::Mat; the message names the key point); kf->N
 * different from the N the keyframe has in the store. */
typedef struct dsh_kf_keypoints {   /* what the mask reads of a keyframe */
  int32_t rows, cols;               /* imGray.rows, imGray.cols */
  int32_t N;                        /* == the N the keyframe has in the store */
  const float* kp;                  /* N x 2: mvKeysUn[i].pt.x, .pt.y */
} dsh_kf_keypoints;

/* Surface::getVertex with xs, ys >= 2 (the reference divides by xs - 1) and the positions TriangularMesh.cc:71-84 hands to the Node
 * constructor: nodes_xyz[xs * ys x 3] in world coordinates, site (x, j) at index x * ys + j.  In double as written at Surface.cc:140-143:
 * u = ((umax - umin - 2 t) * x) / (xs - 1) + (umin + t) with t = 0.03, v alike from j and ys; d = the B-spline depth_ctrl (valdim 1) at
 * (u, v), by the kernel of dsh_bbs_eval; the camera point is (float)(u d), (float)(v d), (float)d, 1; the world point is Twc times it
 * in float32 (the product of dsh_template_switch, below), widened to double.  The triangulation stays with the caller.  Two launches. */
typedef struct dsh_surface_grid {
  dsh_ctx* ctx;
  const dsh_bbs* bbs;               /* valdim 1 */
  const double* depth_ctrl;         /* nptsu * nptsv */
  const float* Twc;                 /* 16, row major */
  int32_t xs, ys;
} dsh_surface_grid;
int dsh_surface_vertices(const dsh_surface_grid* grid, double* nodes_xyz);

/* DefLocalMapping::needNewTemplate on keyframe `slot` of the store: candidate[i] (N entries, may be NULL) = 1 where the table entry is
 * -1 and the mask is 0 at the key point's pixel; *n_candidates = their number, the reference's newPoints, which the caller compares with
 * pointsToTemplate_.  A held bad point is neither a source of the mask nor a candidate (pMP is not null at :389).  One launch. */
int dsh_need_new_template(dsh_mpdb* db, int32_t slot, const dsh_kf_keypoints* kf, int32_t* n_candidates, uint8_t* candidate);

typedef struct dsh_template_switch_counts {
  int32_t n_new, first_id;          /* points created; they are first_id .. first_id + n_new - 1 */
  int32_t n_moved;                  /* key points that hold a point that is not bad */
  int32_t n_masked;                 /* empty key points inside the mask */
  int32_t n_embedded;               /* points with a facet afterwards */
  int32_t n_points;                 /* the store's size afterwards */
} dsh_template_switch_counts;
typedef struct dsh_template_switch_input {
  dsh_kfdb* kfdb;                   /* of the same context; the reference keyframe has the same slot in both stores */
  int32_t slot;                     /* referenceKF_ */
  const dsh_kf_keypoints* kf;
  const float* surface_pts;         /* N x 3: Surface::get3DSurfacePoint per key point, camera frame */
  const float* Twc;                 /* 16, row major: referenceKF_->GetPoseInverse() */
} dsh_template_switch_input;
/* DefLocalMapping::updateTemplate on the store, in the reference's order.  The context's current template must be one built from facets,
 * else DSH_ERR_STATE: the caller builds it just before with dsh_template_build from the nodes of dsh_surface_vertices.
 *   1. clearTemplate: every point of the store loses its facet.
 *   2. The mask of the keyframe, as above.
 *   3. CreateNewMapPoints per key point i; the iterations do not interact, so one parallel pass is exact.  Held and not bad: the point's
 *      position becomes Twc (s_i, 1), counted in n_moved (a point held by two key points keeps the later one's, as in the sequential
 *      loop).  Held and bad: nothing.  Empty and masked: nothing, counted in n_masked.  Empty and not masked: a new point.  New points get
 *      the ids first_id + j in ascending i; new_idx[j] (N entries, may be NULL) = the key point of new point j.
 *      x3wh = Twc * x3ch is a cv::Mat product of float32 4x4 by 4x1.  Reading, as for the pose products of the tracking search (a reading
 *      of OpenCV's gemm for small operands; no OpenCV build to check against): the four products of a row are summed left to right in
 *      float32, every product and sum rounded, no contraction.
 *   4. A new point is what new DefMapPoint(x3w, referenceKF_, map) and :337-342 leave: not bad, visible = found = 1, no facet, one
 *      observation record (id, slot) in the log, n_obs = 1, table entry i of the keyframe = its id; the descriptor is row i of the keyframe
 *      in kfdb (ComputeDistinctiveDescriptors with one observation elects it); normal and max distance are UpdateNormalAndDepth with
 *      that observation and this keyframe as reference, in the arithmetic of dsh_mappoint_update (n = 1: no division; level = the octave of
 *      key point i), by the same device function.  The keyframe's bad flag is not read: referenceKF_ is a keyframe of the map (with a
 *      bad one the reference's election would find no row and leave the descriptor empty).  Ow, the octaves and the scale factors come
 *      from kfdb; an octave >= levels anywhere in the keyframe is DSH_ERR_ARG.  Every later call behaves as if the caller had made
 *      these mutations through dsh_mpdb_add_points, dsh_mpdb_add_observations and dsh_mpdb_set_keyframe_point.
 *   5. createTemplate's embedding: every point of the store that is not bad, the new ones included, is embedded in the context's template
 *      from its position after step 3, as by dsh_template_embed_device (closest node, then that node's facets in index order, float32
 *      pointInTriangle).  A point with a facet gets its three node indices in ascending order and the float32 barycentrics widened to
 *      double (SetCoordinates takes doubles), and RecalculatePosition moves it: the expression of dsh_trackstate_repose on the template's
 *      rest positions.  A point without a facet keeps its position of step 3.
 * Transfers: up go the key points, the surface points, Twc, the keyframe's octaves and scale factors and the template, in one block;
 * down come the counts and new_idx.  Nothing per map point travels.  Three launches: classification with the mask, creation with the
 * prefix sum of the ids, embedding with the repose.
 * Repose's UpdateNormalAndDepth of the embedded points (DefMapPoint.cc:122-126) is the next call on the store: dsh_point_store_upkeep
 * with DSH_UPKEEP_EMBEDDED and DSH_MP_NORMAL_DEPTH, below.
 * NOT COVERED: selectKeyframe (it iterates an unordered_map, its tie order is unspecified); DefKeyFrame::assignTemplate, the
 * textures and lastincorporasion (host bookkeeping); the template constants (dsh_template_build). */
int dsh_template_switch(dsh_mpdb* db, const dsh_template_switch_input* in, int32_t* new_idx, dsh_template_switch_counts* out);

/* Read back n distinct points; each output may be NULL: xyz[n x 3], normal[n x 3], max_distance[n], desc[n x 32], bad[n]. */
int dsh_point_store_get_points(dsh_mpdb* db, int n, const int32_t* ids, float* xyz, float* normal, float* max_distance, uint8_t* desc, uint8_t* bad);
/* Read back the facets of n distinct points; each output may be NULL: nodes[n x 3] (-1 -1 -1: none), bary[n x 3]. */
int dsh_point_store_get_embedding(dsh_mpdb* db, int n, const int32_t* ids, int32_t* nodes, double* bary);

/* ---- mapping: the anchor keyframes and match lists of a new keyframe from the resident map point store --------------------------
 * What SchwarpDatabase::add (Modules/Mapping/SchwarpDatabase.cc:50-128) reads of the map before its first fit, for the new keyframe
 * `slot` of the store, and what DefORBmatcher::searchBySchwarp (Modules/Matching/DefORBmatcher.cc:200-211) lists per anchor.  The
 * stages behind it are on the device already (dsh_warp_initialize, dsh_search_by_schwarp, dsh_schwarp_fit_batch_store,
 * dsh_normals_estimate_db).  Integer valued: every output is exact.  ORDER: the reference iterates an unordered_map<KeyFrame*, int>
 * there, whose order is unspecified; here index order stands for pointer and hash order: anchors by ascending slot.
 *   COUNTS (:61-80).  For each entry i of the keyframe's table, p = table[i]: skipped when p is -1 or bad; counted in n_no_ref and
 *     skipped when p has no reference keyframe; else count[ref[p]]++.  A point held by k entries counts k times (vpMapPointMatches is
 *     walked per entry).  The anchors are the keyframes with count > 0, by ascending slot: anchor_slot[a], anchor_count[a].
 *   PAIRS (:83-106).  For every anchor a, for i ascending, an entry emits a pair when its point p is not bad, the log holds a live
 *     record (p, slot) and the log holds a live record (p, anchor a): pair_idx1 = the key point index of (p, a), pair_idx2 = that of
 *     (p, slot) -- from the record, not from i: a table entry whose point does not observe the keyframe yet (the state between
 *     CreateNewKeyFrame and ProcessNewKeyFrame) emits nothing -- and pair_point = p.  ref[p] == a is NOT required: the reference takes
 *     every shared point for the fit and only stores the records of the anchor's own points (:294-298); pair_own = 1 where
 *     ref[p] == a, which is the point_id >= 0 test of dsh_schwarp_store.  a == slot is legal and literal: idx1 == idx2.
 *     anchor_pairs[a] = the pairs of anchor a.  An anchor with fewer than min_pairs (the reference's 20, :105) keeps its place in the
 *     anchor list and contributes nothing to the lists: pairs of anchor a are pair_ptr[a] .. pair_ptr[a + 1] - 1.
 *   QUERIES (DefORBmatcher.cc:200-211).  For every anchor that passed min_pairs, the entries j of the ANCHOR's table, ascending, whose
 *     point is not -1, not bad and has no live record with `slot`: query_idx1 = j, query_point = the point, at query_ptr[a] ..
 *     query_ptr[a + 1] - 1.  has[j] = table[j] != -1 per entry of the NEW keyframe's table is the `has` of dsh_search_by_schwarp.
 * The key point coordinates stay with the caller, who indexes its own arrays with idx1, idx2.
 * Refusals, by the store's rules: arguments are checked on the host first (DSH_ERR_ARG, nothing written); while the store holds a live
 * observation record without a key point index the call returns DSH_ERR_STATE, decided by the host mirror before any launch; a
 * host-only context then answers DSH_ERR_NO_DEVICE.  The keyframe has at most 8192 key points; the number of anchors is not capped
 * below the store's keyframe count.  CAPACITIES are passed in; when a list does not fit the call returns DSH_ERR_ARG with n_anchors,
 * n_pairs, n_queries set to what is needed, and no array of the caller is written (every other refusal leaves them 0).
 * Nothing goes up (the inputs travel as kernel arguments) and one block comes down; no host round trip between the launches; the
 * temporaries come from the context's scratch.  The matrix of key point indices, anchors x N int32, takes at most max_matrix_bytes
 * (0: 64 MiB); beyond that the anchors are processed in chunks, one more pass over the log per chunk, with the same result. */
typedef struct dsh_anchor_lists {
  /* in */
  int32_t anchor_capacity;          /* entries of anchor_slot, anchor_count, anchor_pairs; pair_ptr and query_ptr have one more */
  int32_t pair_capacity;            /* entries of pair_idx1, pair_idx2, pair_point, pair_own */
  int32_t query_capacity;           /* entries of query_idx1, query_point */
  int64_t max_matrix_bytes;         /* 0: the default */
  int32_t *anchor_slot, *anchor_count, *anchor_pairs;
  int32_t *pair_ptr, *pair_idx1, *pair_idx2, *pair_point;
  uint8_t* pair_own;
  int32_t *query_ptr, *query_idx1, *query_point;
  uint8_t* has;                     /* N of the keyframe; may be NULL */
  /* out */
  int32_t n_anchors, n_pairs, n_queries;
  int32_t n_no_ref;                 /* entries whose point is not bad and has no reference keyframe */
} dsh_anchor_lists;
int dsh_keyframe_anchors(dsh_mpdb* db, int32_t slot, int32_t min_pairs, dsh_anchor_lists* out);

/* ---- mapping: a new keyframe's map point upkeep on the resident stores --------------------------------------------------------
 * LocalMapping::ProcessNewKeyFrame's loop (Thirdparty/ORBSLAM_2/src/LocalMapping.cc:142-165, via DefLocalMapping.cc:160-164) and the
 * upkeep of DefMapPoint::Repose (Modules/Common/DefMapPoint.cc:122-126, from TriangularMesh.cc:192) with every input on the device:
 * the observation lists come from the point store's log, the key point indices from beside it, the reference keyframes from the
 * points, the descriptor rows, camera centres, octaves and scale pyramids from the keyframe store, and the results go into the
 * point store's descriptor, normal and max distance (dsh_point_store_get_points reads them; min = max / scale_factors[levels - 1] of
 * the reference keyframe stays with the caller, as for dsh_template_switch).  Election, normal and depth are the arithmetic stated
 * above dsh_mappoint_update, run by the same device functions.
 * ORDER.  The observations of a point are taken by ascending slot, which stands for the pointer order of std::map<KeyFrame*, size_t>:
 * the order of the float32 normal sum and of the election's ties.  It does not depend on the order in which the records arrived.
 * BAD FLAGS.  The election skips the observations whose keyframe is bad in the POINT store (dsh_mpdb_set_keyframe_bad): that flag is
 * resident, and it is the one the local map reads.  The flag of dsh_kfdb_set_bad is not read here; a caller keeps both current.
 * The keyframe store travels in the input struct: it belongs to the same context, holds at least the keyframes of the point store,
 * in the same order with the same N each, and at most DSH_MP_MAX_OBS of them; none of its keyframes may hold an octave >= levels.
 * A point may have up to DSH_MP_MAX_OBS observations, but that limit is legal, not fast: one wavefront ranks a point's observations
 * by slot with M wave-uniform loads per 64 observations (M^2 / 64 steps), measured up to M = 500 only; its cost near the limit is
 * unmeasured.  A refused call writes nothing, the caller's counts included.
 * Refusals, by the store's rules: arguments against the point store first, then the keyframe store, each DSH_ERR_ARG with nothing
 * changed; a live observation record without a key point index is DSH_ERR_STATE, as for dsh_keyframe_anchors; a host-only context
 * then answers DSH_ERR_NO_DEVICE.  All of it is decided on the host mirrors before any launch; no host read between the launches.
 * Limits found on the device only: a reference keyframe that is not among the observations and has no key point 0 to lend its octave
 * counts as no reference keyframe (dsh_mappoint_update refuses it). */
#define DSH_MP_NO_REF 4        /* status: the point has no reference keyframe -- normal and range unchanged */
#define DSH_MP_SKIPPED_BAD 8   /* status: the point is bad -- nothing changed */

typedef struct dsh_keyframe_process_input {
  dsh_kfdb* kfdb;                   /* of the same context; a keyframe has the same slot in both stores */
  int32_t slot;                     /* the new keyframe */
} dsh_keyframe_process_input;
typedef struct dsh_keyframe_process_counts {
  int32_t n_empty, n_bad, n_added, n_recent;        /* per table entry */
  int32_t n_no_good_desc, n_no_ref;                 /* among the added points */
  int64_t first_record;                             /* log position of the first record appended */
} dsh_keyframe_process_counts;
/* For table entry i of keyframe `slot` with point p, in the reference's order:
 *   p == -1                                             action 0
 *   p bad                                               action 1
 *   no live record (p, slot), i the lowest entry with p action 2: the record (p, slot, i) is appended to the log, n_obs[p] += 1, and
 *                                                       UpdateNormalAndDepth and ComputeDistinctiveDescriptors run over the point's
 *                                                       observations, the new one included
 *   otherwise                                           action 3, the caller's mlpRecentAddedMapPoints: the point observes the keyframe
 *                                                       already, or an earlier entry has just added it; nothing changes for it
 * Records are appended in ascending i; added_point[n_added] (N entries, may be NULL) holds their points in that order, action[N] (may
 * be NULL) the actions.  An added point whose observing keyframes are all bad keeps its descriptor (n_no_good_desc); one without a
 * reference keyframe keeps normal and range (n_no_ref).  Afterwards every call behaves as if the caller had added the pairs with
 * dsh_point_store_add_observations_indexed.  Nothing goes up (the inputs travel as kernel arguments); one block comes down.
 * DSH_ERR_HIP from this call can mean that the device appended records the host mirror does not know: the store is not usable
 * afterwards and is to be cleared or destroyed (the other calls that append on the device, dsh_template_switch, share this). */
int dsh_keyframe_process_new(dsh_mpdb* db, const dsh_keyframe_process_input* in, uint8_t* action, int32_t* added_point,
                             dsh_keyframe_process_counts* out);

#define DSH_UPKEEP_IDS 0       /* the n distinct points ids[n] */
#define DSH_UPKEEP_EMBEDDED 1  /* every point that is not bad and has a facet (Repose after a switch); ids ignored */
typedef struct dsh_point_upkeep_input {
  dsh_kfdb* kfdb;
  int32_t what;                     /* DSH_MP_DESCRIPTOR | DSH_MP_NORMAL_DEPTH */
  int32_t select;                   /* DSH_UPKEEP_* */
  int32_t n;
  const int32_t* ids;
} dsh_point_upkeep_input;
typedef struct dsh_point_upkeep_counts {
  int32_t n_selected;               /* points the selection names that are not bad */
  int32_t n_no_obs, n_no_good_desc, n_no_ref;       /* among them */
  int32_t n_bad;                    /* ids that name a bad point */
} dsh_point_upkeep_counts;
/* The `what` mask of dsh_mappoint_update applied to the selected points of the store.  status[n] (DSH_UPKEEP_IDS only, may be NULL)
 * holds DSH_MP_* flags per id: a bad point is skipped (DSH_MP_SKIPPED_BAD alone); no live observation: DSH_MP_NO_OBS alone, nothing
 * written; every observing keyframe bad: DSH_MP_NO_GOOD_DESC, descriptor unchanged, geometry still from all observations; no reference
 * keyframe: DSH_MP_NO_REF, normal and range unchanged, descriptor still elected.  The two last flags are set whatever `what` asks.
 * Up go the ids; one block comes down. */
int dsh_point_store_upkeep(dsh_mpdb* db, const dsh_point_upkeep_input* in, int32_t* status, dsh_point_upkeep_counts* out);

/* ---- mapping: erasing observations and culling map points on the resident map point store --------------------------------------
 * What takes a point out of the map, on dsh_mpdb's log, tables and per-point state:
 *   MapPoint::EraseObservation       Thirdparty/ORBSLAM_2/src/MapPoint.cc:122-148
 *   DefMapPoint::setBadFlag          Modules/Common/DefMapPoint.cc:76-94
 *   KeyFrame::EraseMapPointMatch     Thirdparty/ORBSLAM_2/src/KeyFrame.cc:248-252
 *   LocalMapping::MapPointCulling    Thirdparty/ORBSLAM_2/src/LocalMapping.cc:173-199
 *   the Schwarp fit's drop           Modules/Mapping/SchwarpDatabase.cc:288-292
 * Integer valued: every output is exact.  ORDER: slot order stands for pointer order, as everywhere in the library.
 * A PAIR (p, s) THAT HAS A LIVE RECORD r (MapPoint.cc:127-143), in the reference's order:
 *   - the record is blanked and n_obs[p] -= 1;
 *   - with erase_match, table entry log_idx[r] of keyframe s becomes -1 WHATEVER THAT ENTRY HOLDS: EraseMapPointMatch(const size_t&)
 *     does not look, and between CreateNewKeyFrame and ProcessNewKeyFrame the two relations disagree;
 *   - if ref_kf[p] == s the reference keyframe becomes the lowest slot among the records of p that are still live (:137-138).  When none
 *     is left it stays as it is: the reference dereferences end() there, the one place where it is undefined;
 *   - if the decremented n_obs[p] <= 2, setBadFlag(p) (:141-147).  The reference keyframe moves BEFORE this cascade, so the move is
 *     decided on the records the cascade then removes;
 *   - status: 0 the pair is not stored, nothing changes, as in the reference; 1 erased; 2 erased and setBadFlag ran.
 *   No bad test is made anywhere: a point that is already bad and still has records is treated like any other.
 * setBadFlag OF p (DefMapPoint.cc:76-94): the bad flag is set, every live record of p is blanked, and for each such record the table
 *   entry it names becomes -1, whatever it holds.  n_obs[p] is NOT touched -- the stale-nObs quirk stated for dsh_track_close_frame.
 *   The reference keyframe, the embedding and the counters stay.  n_set_bad counts the points setBadFlag ran on, bad before or not.
 * dsh_point_store_cull: the decision is dsh_trackstate_cull's, by the same device function -- (float)found / (float)visible < 0.40f and
 *   the same order of cases.  Action 2 runs setBadFlag as above; action 1 (already bad) changes nothing, the records of such a point
 *   stay if it still has any.
 * BATCHES are order-free by construction: every table write is -1 and every log write is a blank, and a point's n_obs and reference
 *   keyframe depend on its own records only.  The one sequential effect in the reference needs the same point twice in a batch (an
 *   erase after the cascade finds nothing), so a repeated point is refused: DSH_ERR_ARG, "point id ... repeated in the batch".  The
 *   fit's drops (one keyframe, distinct points) and the culling list (distinct points) never repeat a point.
 * REFUSALS follow the store's rules.  Arguments are checked on the host first: ids or slots outside the store, NULL with n > 0,
 *   out == NULL, a repeated point and too small a capacity give DSH_ERR_ARG with a message naming the entry, and nothing changes.  A
 *   live record without a key point index gives DSH_ERR_STATE, as for dsh_keyframe_anchors, decided on the host mirror before any
 *   launch; the two read-backs are exempt and report -1 as the index.  A host-only context then gives DSH_ERR_NO_DEVICE; a detached
 *   store gives DSH_ERR_ARG.  A refused call leaves the caller's counts as they were.  The log may have any length: records are
 *   addressed as 64-bit positions (dsh_mpdb_erase_observations refuses a log beyond 2^30 records).
 * One upload and at most four launches per call -- clear, select, one sweep over the log that leaves at its first instruction when no
 * point lost its reference keyframe or became bad, finish -- with no host read between them; one block comes down, and behind it the
 * (point, slot) of the records the sweep erased, which the host mirror then drops: cost proportional to the records erased.
 * DSH_ERR_HIP from these calls can mean that the device erased records the host mirror still knows: the store is not usable
 * afterwards and is to be cleared or destroyed (the calls that append on the device, dsh_keyframe_process_new and
 * dsh_template_switch, share this). */
typedef struct dsh_point_erase_counts {
  int32_t n_found;      /* pairs whose record was live (erase_observations); 0 for the other two calls */
  int32_t n_ref_moved;  /* points whose reference keyframe changed */
  int32_t n_set_bad;    /* points this call set bad */
  int32_t n_records;    /* log records blanked, the pairs' own included */
  int32_t n_entries;    /* table entries written to -1, counted once per record that names them */
} dsh_point_erase_counts;

/* MapPoint::EraseObservation (MapPoint.cc:122-148) for n pairs with DISTINCT points; erase_match != 0 adds
 * KeyFrame::EraseMapPointMatch(idx) of the erased record's key point (SchwarpDatabase.cc:290-291).  status[n] may be NULL. */
int dsh_point_store_erase_observations(dsh_mpdb* db, int n, const int32_t* point_ids, const int32_t* keyframe_slots, int32_t erase_match,
                                       uint8_t* status, dsh_point_erase_counts* out);
/* DefMapPoint::setBadFlag (DefMapPoint.cc:76-94) of n distinct points. */
int dsh_point_store_set_bad(dsh_mpdb* db, int n, const int32_t* ids, dsh_point_erase_counts* out);
/* LocalMapping::MapPointCulling (LocalMapping.cc:173-199): dsh_trackstate_cull's arguments and actions, with action 2 doing setBadFlag in full. */
int dsh_point_store_cull(dsh_mpdb* db, int n, const int32_t* ids, const int32_t* first_kf, int32_t current_kf, uint8_t* action,
                         dsh_point_erase_counts* out);
/* Read-backs: MapPoint::GetObservations of n distinct points as a CSR by ascending slot (obs_ptr[n + 1], slots / idx of `capacity`
 * entries; when they do not fit: DSH_ERR_ARG with *n_total set and no array written), and KeyFrame::GetMapPointMatches: points[N] of
 * keyframe `slot`, capacity >= N.  A record added without a key point index reports -1. */
int dsh_point_store_get_observations(dsh_mpdb* db, int n, const int32_t* ids, int32_t* obs_ptr, int32_t capacity, int32_t* slots,
                                     int32_t* idx, int32_t* n_total);
int dsh_point_store_get_keyframe_table(dsh_mpdb* db, int32_t slot, int32_t capacity, int32_t* points);

/* ---- mapping: surface registration of a keyframe from the resident stores ------------------------------------------------------
 * SurfaceRegistration::registerSurfaces (Modules/Mapping/SurfaceRegistration.cc:48-153) with its inputs taken from the stores: the
 * walk over GetMapPoint, isBad, getFacet and PosesKeyframes[refKF] that builds the two clouds, the registration of
 * dsh_surface_register on them, Surface::applyScale (Modules/Mapping/Surface.cc:107-121) and refKF->SetPose (:150).  Every entry takes
 * the point store alone; the keyframe store travels in the input struct, as for dsh_keyframe_process_new.
 *
 * THE SNAPSHOT.  The map cloud is not the points' current position: it is the position each point had when the keyframe was
 * constructed (Modules/Common/DefKeyFrame.cc:60-74: for every key point whose point exists, is not bad and has a facet,
 * PosesKeyframes[this] = GetWorldPos).  The store keeps it beside the keyframe tables: snap_point (int32, -1: none) and snap_xyz (three
 * float32) per table entry.  A new keyframe starts with -1 everywhere; dsh_mpdb_clear forgets it.
 *   PosesKeyframes[kf] of point p is non-empty exactly when some entry j of kf has snap_point[j] == p, and its value is that entry's
 *   snap_xyz.  Entries naming the same point hold the same bytes: they were taken in one instant.  Later edits of the table --
 *   dsh_mpdb_set_keyframe_point, the template switch, the erase calls -- do not touch the snapshot: it is keyed by point, as the
 *   reference's unordered_map is.
 * dsh_keyframe_snapshot_positions takes it for keyframe `slot`: one launch, nothing goes up, one small block comes down; *n_taken (may
 * be NULL) = the entries taken.  The reference takes the snapshot once, in the constructor: a second call on the same keyframe returns
 * DSH_ERR_STATE (the host mirror keeps a flag per keyframe).  dsh_keyframe_get_snapshot reads it back: point[N] and xyz[N x 3] of the
 * keyframe's N entries, capacity >= N; an entry without a snapshot reads -1 and zeros.
 *
 * THE CLOUDS (SurfaceRegistration.cc:60-104), for table entry i ascending with p = table[i], the first matching case:
 *   p == -1                                  n_empty
 *   p bad                                    n_bad
 *   p without a facet now                    n_no_facet
 *   p without a snapshot for this keyframe   n_no_snapshot
 *   otherwise                                pair k = the number of pairs before i: cloud_map[k] = the snapshot of p, cloud_surface[k] =
 *                                            rows 0..2 of Twc * (s_i, 1), pair_idx[k] = i
 * covNorm is an array address in the reference and always true.  The product is the float32 one stated for dsh_template_switch: four
 * products per row, summed left to right, no contraction.  One launch, pairs in entry order; a keyframe has at most 8192 key points.
 * dsh_keyframe_register_clouds is the selection alone (u, nu, chi_limit and check_chi are not read; pair_idx, cloud_surface and
 * cloud_map hold N entries each and may be NULL): a caller who wants the reference's lazy rand() learns n_pairs from it.
 *
 * THE REGISTRATION.  Fewer than 15 pairs: registered = 0 and nothing else runs (:106-107).  More than 8000 pairs: DSH_ERR_ARG with the
 * counts set (the limit of dsh_surface_register).  Otherwise the stages of dsh_surface_register run on the clouds where the selection
 * left them, with the same n in the same order, so sim3, s22, Tcw_new and info are the bytes dsh_surface_register gives for the same
 * clouds; consumed = the draws of the stream the reference makes.  The counts are read back once between the selection and the first
 * stage: the host's walk of the stream needs n.  A stream that is too short is DSH_ERR_ARG with stream_status = 1 and the counts set;
 * nothing is mutated.
 * When registered, one finishing launch
 *   - writes surface_scaled[i] = (float)((double)s_i * s22) per component for all N entries (may be NULL): Surface::applyScale on a
 *     cv::Vec3f, a reading of OpenCV's Vec * double (no OpenCV build to check against); nodesDepth_ stays with the caller unless the
 *     keyframe has a resident Surface (below), which is scaled in the same launch;
 *   - with a keyframe store given, makes the keyframe's camera centre there the centre of Tcw_new by KeyFrame::SetPose
 *     (Thirdparty/ORBSLAM_2/src/KeyFrame.cc:97-111): Ow[i] = -((R[0][i] * t[0] + R[1][i] * t[1]) + R[2][i] * t[2]) in float32.  It is
 *     returned in Ow_new either way.  dsh_template_switch and dsh_point_store_upkeep, which run next, read that centre.
 * When not registered nothing in either store changes and surface_scaled is not written.
 *
 * THE KEYFRAME POSE.  dsh_keyframe_set_pose is KeyFrame::SetPose for any other caller: the centre of Tcw goes into the keyframe store
 * (and into Ow, which may be NULL); dsh_keyframe_get_centre reads the stored centre back (Tcw is not read).
 *
 * Refusals follow the store's rules: arguments first, DSH_ERR_ARG with a message that names the entry (a keyframe store, where one is
 * given, must belong to the same context and hold the slot with the same N); a host-only context then gives DSH_ERR_NO_DEVICE; a
 * detached store gives DSH_ERR_ARG.  A refused call writes nothing but the counts named above.  Every entry here names a keyframe of
 * the store, and the store of a host-only context stays empty (dsh_mpdb_add_keyframe needs the device), so there the argument check
 * "slot outside the store" always comes first and DSH_ERR_NO_DEVICE cannot be observed through these entries.  The keyframe store's
 * handle is looked up among the stores attached to the context before it is read: a store of another context, a detached one and a
 * pointer that is no store are all DSH_ERR_ARG.  Twc and the Tcw of dsh_keyframe_set_pose must be finite (DSH_ERR_ARG), as the centre
 * of dsh_kfdb_add must; a registration whose composed pose is not finite (a degenerate alignment, which the reference would hand to
 * SetPose) returns DSH_ERR_STATE with the counts, sim3 and info set, registered = 0 and nothing written. */
int dsh_keyframe_snapshot_positions(dsh_mpdb* db, int32_t slot, int32_t* n_taken);
int dsh_keyframe_get_snapshot(dsh_mpdb* db, int32_t slot, int32_t capacity, int32_t* point, float* xyz);

typedef struct dsh_keyframe_register_input {
  dsh_kfdb* kfdb;                   /* may be NULL: then no camera centre is written */
  int32_t slot, N;                  /* N == the N the keyframe has in the store */
  const float* surface_pts;         /* N x 3: Surface::get3DSurfacePoint per key point, camera frame */
  const float* Twc;                 /* 16, row major: refKF->GetPoseInverse before the registration */
  const double* u;                  /* the rand stream, as for dsh_surface_register */
  int64_t nu;
  double chi_limit;
  int32_t check_chi;
} dsh_keyframe_register_input;
typedef struct dsh_keyframe_register_result {
  int32_t n_pairs, n_empty, n_bad, n_no_facet, n_no_snapshot;   /* per table entry */
  int32_t registered, stream_status;
  int64_t consumed;
  double sim3[8], s22, info[8];     /* as dsh_surface_register */
  float Tcw_new[16], Ow_new[3];
} dsh_keyframe_register_result;
int dsh_keyframe_register_clouds(dsh_mpdb* db, const dsh_keyframe_register_input* in, int32_t* pair_idx, float* cloud_surface, float* cloud_map,
                                 dsh_keyframe_register_result* out);
int dsh_keyframe_register(dsh_mpdb* db, const dsh_keyframe_register_input* in, int32_t* pair_idx, float* surface_scaled,
                          dsh_keyframe_register_result* out);

typedef struct dsh_keyframe_pose_input {
  dsh_kfdb* kfdb;                   /* of the same context */
  int32_t slot;
  const float* Tcw;                 /* 16, row major */
} dsh_keyframe_pose_input;
int dsh_keyframe_set_pose(dsh_mpdb* db, const dsh_keyframe_pose_input* in, float* Ow /* 3, may be NULL: the centre written */);
int dsh_keyframe_get_centre(dsh_mpdb* db, const dsh_keyframe_pose_input* in, float* Ow /* 3 */);

/* ---- the resident Surface of a keyframe ----------------------------------------------------------------------------------
 * defSLAM::Surface (Modules/Mapping/Surface.cc) holds, per key point of a keyframe, SurfacePoint::Normal with NormalOn and
 * SurfacePoint::x3D, and per keyframe numberofNormals_ and the depth spline nodesDepth_ with its grid.  The store keeps it beside the
 * keyframe tables, with DefKeyFrame::mpKeypointNorm[i].pt: per table entry a normal (three float32, zeros), a has-normal flag (0), a
 * surface point (three float32, zeros as a default cv::Vec3f) and the normalised key point (two float32); per keyframe, with a host
 * mirror, "has a surface", n_normals, "has a depth spline", its grid and at most 512 doubles of control points.  dsh_mpdb_clear forgets
 * all of it.  A keyframe has no resident Surface until dsh_keyframe_surface_init, and every other entry here refuses such a keyframe.
 *
 * dsh_keyframe_surface_init      Surface(N) in DefKeyFrame's constructor plus mpKeypointNorm (Surface.cc:31-37): N must be the N of the
 *                                keyframe, kpn[N x 2] finite; once per keyframe, a second call is DSH_ERR_STATE.  The bounding box stays
 *                                with the caller.
 * dsh_keyframe_surface_set_depth Surface::saveArray (Surface.cc:50-56): bbs with at most 512 control points, ctrl[nptsu * nptsv].  Serves the
 *                                plane of ones of MonocularInitialization (DefTracking.cc:617-633) and any host-made spline.
 * dsh_keyframe_surface_set_points Surface::set3DSurfacePoint (Surface.cc:94-97) from the host: n distinct idx of the keyframe, pts[n x 3].
 * dsh_keyframe_surface_set_normals Surface::setNormalSurfacePoint (Surface.cc:76-85) for normals the host holds: target j is key point
 *                                idx[j] of keyframe slot[j], in CALL ORDER -- a target named twice keeps the later normal -- and a
 *                                keyframe's n_normals goes up once per entry that had no normal before.  The largest j per target is
 *                                elected with an integer atomic and writes in a second pass, which also counts: the result does not
 *                                depend on the schedule.  n_normals_out[n] (may be NULL) = each target keyframe's count after the call.
 * dsh_keyframe_surface_take_normals the same with normal j picked on the device from the last dsh_normals_estimate_db of in->ddb, by sel's
 *                                convention of dsh_sfn_estimate_db (>= 0: normal_ref of that point, < 0: record -1 - sel).  The normals
 *                                never visit the host; the caller chooses the entries from the status / rec_written / rec_tag /
 *                                rec_idx2 the solve returned (NormalEstimator.cc:170, :223).
 * dsh_keyframe_surface_gather    per target Ni(0), Ni(1) and the return value of Surface::getNormalSurfacePoint (zeros where there is no
 *                                normal) and mpKeypointNorm: x0 / has_x0 / ref_uv of dsh_normals_estimate[_db], first_n / has_fn of
 *                                the host-record route (NormalEstimator.cc:60-110).  One launch, one download.
 * dsh_keyframe_surface_get       reads everything back, each output may be NULL: normals[N x 3], has_normal[N], pts[N x 3], kpn[N x 2],
 *                                ctrl (the control points of the depth spline, when there is one; room for 512), info.
 * dsh_keyframe_surface_vertices  dsh_surface_vertices with the resident depth spline; DSH_ERR_STATE without one.
 * dsh_keyframe_surface_state     0 / 1 / 2 from the host mirror: no resident Surface, a Surface, a Surface with a depth spline.
 *
 * dsh_keyframe_sfn is ShapeFromNormals::ShapeFromNormals + ::estimate (ShapeFromNormals.cc:38-171) of keyframe in->slot.  The selection
 * is obtainM's (:190-210), for table entry i ascending with p = table[i], the first matching case:
 *   p == -1                               n_empty
 *   p bad                                 n_bad
 *   no normal                             n_no_normal
 *   a normal with a NaN component         n_nan      (Normal == Normal on a cv::Vec3f: an infinite component passes)
 *   otherwise                             site k = the number of sites before i, at ((double)kpn.x, (double)kpn.y) with that normal
 * One launch over at most 8192 entries, sites in entry order; the site count is read back once and sizes the launches that follow: the
 * stages of dsh_sfn_estimate on the sites where the selection left them, with u_all / v_all the keyframe's resident key points widened.
 * For the same sites ctrl_raw, ctrl and pts are the bytes dsh_sfn_estimate gives.  When ok, the surface points are evaluated into the
 * store and the scaled control points become the keyframe's depth spline (set3DSurfacePoint, saveArray, :158-167), and ctrl_raw
 * [nptsu * nptsv], ctrl [nptsu * nptsv] and pts [N x 3] (each may be NULL) come down.  When not ok nothing in the store changes.  A
 * keyframe without a site is not ok and nothing is solved or written, ctrl_raw included: the bending rows and the mean-depth row alone
 * have rank nptsu * nptsv - 2 (the affine depth maps are the null space of the bending energy), which a factorisation in floating
 * point can miss.  At most 512 control points.
 *
 * A NULL surface_pts in dsh_keyframe_register_clouds, dsh_keyframe_register and dsh_template_switch means the resident surface points of
 * the keyframe; for a keyframe without a resident Surface it stays the DSH_ERR_ARG it was.  When dsh_keyframe_register registers a
 * keyframe that has a resident Surface, its finishing launch also applies Surface::applyScale to the resident copy, whichever way
 * surface_pts was given: the points as (float)((double)s * s22), the depth spline as nodesDepth_[i] = s22 * nodesDepth_[i] in double
 * (Surface.cc:107-121).  A keyframe without one behaves as before.
 *
 * Refusals follow the store's rules: arguments on the host mirror first (DSH_ERR_ARG, the message names the entry, nothing is written),
 * then a host-only context is DSH_ERR_NO_DEVICE; a detached store is DSH_ERR_ARG. */
typedef struct dsh_keyframe_surface_info {
  int32_t N, n_normals;             /* numberofNormals_ */
  int32_t enough_normals;           /* Surface::enoughNormals: n_normals >= 10 (Surface.cc:62-67) */
  int32_t has_depth;
  dsh_bbs grid;                     /* of the depth spline; zeros without one */
} dsh_keyframe_surface_info;
int dsh_keyframe_surface_init(dsh_mpdb* db, int32_t slot, int32_t N, const float* kpn /* N x 2 */);
int dsh_keyframe_surface_set_depth(dsh_mpdb* db, int32_t slot, const dsh_bbs* bbs, const double* ctrl);
int dsh_keyframe_surface_set_points(dsh_mpdb* db, int32_t slot, int32_t n, const int32_t* idx, const float* pts);
int dsh_keyframe_surface_set_normals(dsh_mpdb* db, int32_t n, const int32_t* slot, const int32_t* idx, const float* normals /* 3 n */, int32_t* n_normals_out);
typedef struct dsh_surface_take_input {   /* the database travels in the input struct, as the keyframe store of dsh_keyframe_register does */
  const dsh_diffdb* ddb;            /* of the same context; its last dsh_normals_estimate_db is read */
  int32_t n;
  const int32_t* sel;               /* n */
  const int32_t* slot;              /* n */
  const int32_t* idx;               /* n */
} dsh_surface_take_input;
int dsh_keyframe_surface_take_normals(dsh_mpdb* db, const dsh_surface_take_input* in, int32_t* n_normals_out);
int dsh_keyframe_surface_gather(dsh_mpdb* db, int32_t n, const int32_t* slot, const int32_t* idx, float* normal_xy /* 2 n */, uint8_t* has /* n */,
                                float* uv /* 2 n */);
int dsh_keyframe_surface_get(dsh_mpdb* db, int32_t slot, int32_t capacity, float* normals, uint8_t* has_normal, float* pts, float* kpn, double* ctrl,
                             dsh_keyframe_surface_info* info);
int dsh_keyframe_surface_vertices(dsh_mpdb* db, int32_t slot, const float* Twc, int32_t xs, int32_t ys, double* nodes_xyz);
/* What the host mirror knows of keyframe `slot`, without touching the device: 0 no resident Surface, 1 a Surface, 2 a Surface with a
 * depth spline; -1 for a slot outside the store or a detached store.  The call sites that serve keyframes with and without a resident
 * Surface (integration/surface_register_store_hip.h, template_switch_hip.h) ask it before they choose surface_pts. */
int32_t dsh_keyframe_surface_state(const dsh_mpdb* db, int32_t slot);

typedef struct dsh_keyframe_sfn_input {
  dsh_ctx* ctx;                     /* the context of the store */
  int32_t slot;
  const dsh_bbs* bbs;               /* the grid of the depth spline to estimate */
  double bending_weight, mean_depth;
} dsh_keyframe_sfn_input;
typedef struct dsh_keyframe_sfn_result {
  int32_t n_sites, n_empty, n_bad, n_no_normal, n_nan;   /* per table entry */
  int32_t ok;                       /* ShapeFromNormals::estimate's return value */
} dsh_keyframe_sfn_result;
int dsh_keyframe_sfn(dsh_mpdb* db, const dsh_keyframe_sfn_input* in, double* ctrl_raw, double* ctrl, float* pts, dsh_keyframe_sfn_result* out);

/* ---- a new keyframe on the resident stores: creation and covisibility connections -------------------------------------------------
 * The two steps of a keyframe's life cycle that come before and after the map point upkeep of dsh_keyframe_process_new.  Both take the
 * point store alone; the keyframe store travels in the input struct.
 *
 * CREATION.  DefTracking::CreateNewKeyFrame (Modules/Tracking/DefTracking.cc:696-707), that is KeyFrame::KeyFrame from a Frame
 * (Thirdparty/ORBSLAM_2/src/KeyFrame.cc:37-75) and DefKeyFrame::DefKeyFrame (Modules/Common/DefKeyFrame.cc:42-77), on the tracking
 * thread at every tenth frame (DefTracking.cc:175-178).  dsh_keyframe_create leaves both stores, host mirrors included, in the state
 * these four calls leave them in, in this order:
 *   1. dsh_kfdb_add with the camera centre of Tcw and bad = 0.  The centre is KeyFrame::SetPose's, computed by the one function that
 *      serves dsh_keyframe_set_pose; kf->Ow and kf->bad are not read.
 *   2. dsh_mpdb_add_keyframe with the table, parent -1 and bad = 0.  The table is points[N], or with points == NULL the resident
 *      keyframe candidate of the last dsh_track_end_frame, copied device to device; the candidate is not consumed.
 *   3. dsh_keyframe_snapshot_positions of the new slot (DefKeyFrame.cc:60-74: point held, not bad, has a facet).
 *   4. dsh_keyframe_surface_init with kpn, when kpn is given.  NormaliseKeypoints (DefKeyFrame.cc:94-133) and the bounding box stay
 *      with the caller, as they do for dsh_keyframe_surface_init.
 * One block goes up, two launches run (the block into the arrays of both stores, then the snapshot) and one result block comes down;
 * the tables, rows and keyframe arrays grow inside the call when they must.  No observation is added: the reference adds them later,
 * in ProcessNewKeyFrame (dsh_keyframe_process_new).  ComputeBoW, the grid and the images have no counterpart in the stores.
 * Refusals are decided on the host mirrors before any device work and leave neither store changed, DSH_ERR_ARG each: a NULL points
 * without a candidate, or with one whose length is not kf->N; a table entry that is neither -1 nor a point of the store; a keyframe
 * store that is NULL, of another context or detached, or that holds another number of keyframes than the point store (the new slot is
 * the same in both); everything dsh_kfdb_add refuses (an octave outside 0 .. 127, levels outside 1 .. 32, a centre that is not
 * finite); a Tcw or kpn that is not finite; N > 8192; a store that holds 65535 keyframes already.  Then a host-only context is
 * DSH_ERR_NO_DEVICE.
 *
 * CONNECTIONS.  dsh_keyframe_update_connections is KeyFrame::UpdateConnections (KeyFrame.cc:326-419), which
 * LocalMapping::ProcessNewKeyFrame calls right after its loop (LocalMapping.cc:167), for keyframe `slot`.  Index order stands for
 * pointer order; every value is an integer and every output exact.
 *   weights     for every table entry of the keyframe that holds a point p that is not bad, every live record (p, k) of the log with
 *               k != slot adds 1 to w[k] (:335-357).  A point held by m entries counts m times; erased records do not count; there
 *               is no bad test on keyframe k.  counted_kf / counted_w: the n_counted keyframes with w > 0, by ascending slot
 *               (mConnectedKeyFrameWeights).
 *   empty       no positive weight (:361): nothing changes, n_counted = n_connected = 0, parent_set = 0, max_kf = -1.
 *   pKFmax      max_weight / max_kf: the first keyframe in ascending slot order with a strictly larger weight (:373-381) -- the LOWEST
 *               slot among the maxima.
 *   connected   every keyframe with w >= th; if there is none, the single pair (max_weight, max_kf) (:382-393).
 *   order       ordered_kf / ordered_w, n_connected entries: descending weight and, among equal weights, DESCENDING slot -- sort on
 *               (weight, pointer) and push_front (:395-402).  The tie rule is the opposite of pKFmax's; both are the reference's.
 *   parent      the store keeps mbFirstConnection per keyframe in its host mirror: true from dsh_mpdb_add_keyframe and
 *               dsh_keyframe_create on.  When it is true and slot != 0, the keyframe's parent in the store becomes ordered_kf[0] and the
 *               flag clears (:412-417, parent_set = 1).  Slot 0 (mnId == 0) never gets a parent here and keeps its flag.  A parent given
 *               to dsh_mpdb_add_keyframe or set by dsh_mpdb_set_keyframe_parent does not clear the flag -- KeyFrame::ChangeParent does
 *               not touch mbFirstConnection either -- so the first call with a positive weight OVERWRITES such a parent, as the
 *               reference would.  `parent` is the keyframe's parent after the call, -1 for none.
 * Not kept in the store: AddConnection on the OTHER keyframes and their re-sorted lists (KeyFrame.cc:149-185), which no module of
 * DefSLAM reads but the viewer; the caller applies them to its host objects from ordered_kf / ordered_w.
 * At most four launches and no host read between them: a clear, the table's multiplicities, one coalesced sweep over the log with a
 * histogram in LDS (the vote of dsh_local_map_update with the table as the frame and the own slot left out), and the ordering, which
 * is exact for as many keyframes as the store may hold: (w << 16) | slot is a unique key, w <= 8192, slot < 65535.  One block down.
 * The call reads no key point index, so records added without one are fine.  th is 100 in the reference (KeyFrame.cc:369).
 * DSH_ERR_ARG: slot outside the store; th < 1; a list given and capacity smaller than the store's keyframe count; a keyframe with more
 * than 8192 key points; a store with more than 65535 keyframes.  Then a host-only context is DSH_ERR_NO_DEVICE. */
typedef struct dsh_keyframe_create_input {
  dsh_kfdb* kfdb;               /* of the same context; must hold exactly as many keyframes as the point store */
  const dsh_mp_keyframe* kf;    /* N, descriptor rows, octaves, levels, scale factors as for dsh_kfdb_add; Ow and bad are not read */
  const float* Tcw;             /* 16, row major: F.mTcw */
  const int32_t* points;        /* N ids or -1, or NULL: the resident keyframe candidate, whose length must equal kf->N */
  const float* kpn;             /* N x 2 mpKeypointNorm, or NULL: no Surface is initialised */
} dsh_keyframe_create_input;
typedef struct dsh_keyframe_create_result {
  int32_t slot;                 /* of the new keyframe, in both stores */
  int32_t n_held;               /* table entries that hold a point */
  int32_t n_snapshot;           /* entries whose position was taken */
  float Ow[3];                  /* the camera centre written */
} dsh_keyframe_create_result;
int dsh_keyframe_create(dsh_mpdb* db, const dsh_keyframe_create_input* in, dsh_keyframe_create_result* out);

typedef struct dsh_keyframe_connections {
  int32_t n_counted;            /* keyframes with a weight > 0 */
  int32_t n_connected;          /* length of mvpOrderedConnectedKeyFrames */
  int32_t parent;               /* the keyframe's parent after the call, -1: none */
  int32_t parent_set;           /* 1: this call set it, the first connection */
  int32_t max_weight, max_kf;   /* nmax, pKFmax */
} dsh_keyframe_connections;
/* counted_kf, counted_w, ordered_kf, ordered_w: capacity entries each, each may be NULL; out may be NULL */
int dsh_keyframe_update_connections(dsh_mpdb* db, int32_t slot, int32_t th, int32_t capacity, int32_t* counted_kf, int32_t* counted_w,
                                    int32_t* ordered_kf, int32_t* ordered_w, dsh_keyframe_connections* out);

/* ---- one anchor of SchwarpDatabase::add on the resident stores -----------------------------------------------------------------------
 * The per-anchor body of SchwarpDatabase::add (Modules/Mapping/SchwarpDatabase.cc:107-117): DefORBmatcher::findbyWarp
 * (Modules/Matching/DefORBmatcher.cc:47-71) and SchwarpDatabase::calculateSchwarps (SchwarpDatabase.cc:145-349) for a new keyframe
 * `slot` (KF2) and one anchor keyframe `anchor` (KF1), with every per-key-point array read where the stores hold it.  Both entries take
 * the point store alone; the context, the keyframe store and the DiffProp database travel in the input struct.
 *
 * dsh_keyframe_set_view keeps what the pair call needs of a keyframe beyond its Surface: the pixel key points mvKeysUn[i].pt beside
 * the keyframe tables (two float32 per table entry, parallel to the Surface arrays) and, in the store's host mirror, the camera, the
 * image bounds, the image grid and the warp grid of the keyframe.  One upload and no launch beyond the copy.  DSH_ERR_ARG: slot
 * outside the store; view->N not the keyframe's N; a NULL kp_px with N > 0; a value that is not finite; mnMaxX <= mnMinX or
 * mnMaxY <= mnMinY; grid_cols or grid_rows < 1 or grid_cols * grid_rows > 8192; a warp grid with fewer than 4 control points along an
 * axis or an empty domain.  DSH_ERR_STATE: a keyframe without a resident Surface (dsh_keyframe_surface_init); a second call for the
 * keyframe.  Then a host-only context is DSH_ERR_NO_DEVICE.  dsh_mpdb_clear forgets the views.  dsh_keyframe_get_view reads one back
 * (kp_px with room for N x 2 floats, may be NULL; view->kp_px is left NULL); DSH_ERR_STATE without a view.
 *
 * dsh_keyframe_warp_pair runs the stages below.  The index lists go up in one block; the count of stage 5 is the one value read back
 * before the result block.  With N = NCu * NCv control points of the ANCHOR's warp grid and P = n_pairs:
 *   1 GATHER    kp1[i] = kpn[anchor][pair_idx1[i]], kp2[i] = kpn[slot][pair_idx2[i]] (the resident mpKeypointNorm), invsig[i] =
 *               sqrtf(1.0f / (sf * sf)) in float32, every operation rounded, sf the anchor's scale factor at the octave of key point
 *               pair_idx1[i] (ORBextractor.cc:422,430 and DefORBmatcher.cc:133-135).  For query j the key point kpn[anchor][query_idx1[j]]
 *               and the anchor's 32-byte descriptor row.  KF2's descriptor rows and pixel key points are read in place.
 *   2 INITIALISE  Warp::initialize (DefORBmatcher.cc:138-153): the launches of dsh_warp_initialize on the gathered arrays, same kernels
 *               and operands; init_ok is that call's verdict.  Then NaN entries among the first min(2N, 2 * NCu * NCu) values of x
 *               become 0 (the reference's loop bound, :139-152).
 *   3 FILTER    (:155-186) the residuals of dsh_schwarp_eval with the anchor's (fx, fy) in the slots and lambda 0; the block of 2P
 *               residuals is corrected as Ceres' HuberLoss(5.77) corrector does: s = the sum of their squares in ascending index
 *               order in double without contraction (one lane adds them, so the bytes are those of a host loop), and when
 *               s > 5.77 * 5.77 every residual is multiplied by sqrt(5.77 / sqrt(s)).  Match i is FILTERED when r[2i]^2 + r[2i+1]^2 >
 *               20, two products and one sum without contraction: entries 2i and 2i+1 of [x_0 .. x_{P-1}, y_0 .. y_{P-1}], two
 *               neighbouring x- (or y-) residuals, as the reference pairs them.  A filtered match clears table[slot][pair_idx2[i]]
 *               (EraseMapPointMatch); its observation record stays.  The kept matches are compacted in order.
 *   4 SEARCH AND REGISTER  (:57-70, :189-294) dsh_search_by_schwarp's kernels with the gathered queries against KF2 in place; a key
 *               point of KF2 is taken when its table entry is not -1 AFTER the clears of stage 3.  For query j in ascending order that
 *               found idx2, with p = table[anchor][query_idx1[j]] != -1: the first such query of a point without a live record
 *               (p, slot) appends (p, slot, idx2) to the log and n_obs[p] += 1 (AddObservation with its early return); and
 *               table[slot][idx2] = p, where of several queries that found one key point the LAST in query order holds the entry.
 *               Records are appended in ascending query order.  No UpdateNormalAndDepth and no descriptor election: the reference
 *               makes none here.  The kept list becomes the kept pairs followed by the matched queries (p == -1 included).
 *   5 COUNT     the length L of the kept list is read back and sizes the fit.  L < min_pairs ends the call with fitted = 0: the
 *               kept entries are UNFITTED, the DiffProp database is untouched.
 *   6 FIT       (SchwarpDatabase.cc:145-264) the stages of dsh_schwarp_fit_batch for one problem on the kept arrays where they lie:
 *               slots (fy, fx) of the anchor, fx and fy of the anchor for the drop test, max_iters iterations, start value the x of
 *               stage 2.  x, info and costs are that call's bytes for the same arrays.
 *   7 RECORDS AND DROPS  (:268-346) the kept list in list order, entry j with (idx1, idx2), p1 = table[anchor][idx1] and
 *               p2 = table[slot][idx2] as they are when the loop reaches j; the first matching case:
 *                 p1 or p2 is -1 or bad                SKIPPED
 *                 the fit's drop flag (error > 10 px)  DROPPED: MapPoint::EraseObservation(p2, slot) in full -- the record (p2, slot) is
 *                                                      blanked when it is live, n_obs goes down, a reference keyframe that was `slot`
 *                                                      moves to the lowest remaining slot, and at n_obs <= 2 DefMapPoint::setBadFlag
 *                                                      blanks the point's records and clears the table entries they name -- then
 *                                                      table[slot][idx2] = -1
 *                 ref_kf[p1] != anchor                 KEPT, nothing stored
 *                 otherwise                            STORED: the DiffProp record goes into in->ddb under point id p1 with in->tag and
 *                                                      idx2, in list order; p1 is the caller's newInformation_
 *               The loop is sequential in the reference.  Its entries interact in three ways, all through DROPPED entries that are
 *               reached alive: a later entry with the same idx2 finds p2 == -1; a later entry that names a point the drop set bad
 *               (as p1 or p2) is skipped; a later entry whose idx1 is the key point index of a blanked record of the anchor finds
 *               p1 == -1.  (A point that lost its record and moved its reference keyframe to the anchor is read with the new one.)
 *               The device resolves this with integer elections -- atomicMin of the list position per idx2, per point and per anchor
 *               entry over the alive dropped entries -- repeated until the alive flags stop changing: entry j depends on entries
 *               before j alone, so the fixed point is the sequential result whatever the schedule; a list without chains settles
 *               in two rounds.  A counting second pass writes.
 * After the call both stores, their host mirrors and in->ddb are what the reference's objects are when calculateSchwarps returns.
 *
 * Results: out->x[2N] (the fit's, or stage 2's when fitted == 0), pair_state[n_pairs], query_state[n_queries] (DSH_WARP_*),
 * query_match[n_queries] (idx2 or -1), query_point[n_queries] (p of stage 4, -1: none) and query_added[n_queries] (1: this query's
 * record was appended; the records follow first_record in ascending query order); each array may be NULL.  Counts as named; `erase` as
 * dsh_point_store_erase_observations reports them (n_entries counts the entries the cascade cleared).
 *
 * DSH_ERR_ARG, decided on the host mirrors before any device work, nothing written: in or out NULL; in->ctx not the context of the
 * store; a keyframe store or database that is NULL, of another context or detached; a keyframe store that does not hold the point
 * store's keyframes or holds an octave >= levels; slot or anchor outside the store; anchor == slot (the reference cannot reach it: no
 * point is anchored in the keyframe being added); a keyframe with more than 8192 key points; n_pairs < 1 or n_queries < 0; an index
 * outside its keyframe; a repeated pair_idx2 or query_idx1; more than 256 control points in the anchor's warp grid; max_iters outside
 * 0 .. 1000, min_pairs < 1, a radius that is not positive and finite, th_low > 256.  DSH_ERR_STATE: a keyframe without a view; a live
 * record without a key point index.  Then a host-only context is DSH_ERR_NO_DEVICE.  DSH_ERR_HIP after the first append leaves the
 * store unusable, as for dsh_keyframe_process_new. */
typedef struct dsh_keyframe_view {
  int32_t N;
  const float* kp_px;               /* N x 2: mvKeysUn[i].pt */
  float fx, fy, cx, cy;
  float mnMinX, mnMaxX, mnMinY, mnMaxY;
  int32_t grid_cols, grid_rows;     /* FRAME_GRID_COLS, FRAME_GRID_ROWS */
  dsh_bbs warp_grid;                /* umin, umax, NCu, vmin, vmax, NCv, valdim of the keyframe */
} dsh_keyframe_view;
int dsh_keyframe_set_view(dsh_mpdb* db, int32_t slot, const dsh_keyframe_view* view);
int dsh_keyframe_get_view(dsh_mpdb* db, int32_t slot, dsh_keyframe_view* view, float* kp_px);

#define DSH_WARP_NO_MATCH 0         /* a query that found no key point */
#define DSH_WARP_FILTERED 1         /* a pair stage 3 removed */
#define DSH_WARP_UNFITTED 2         /* on the kept list of a call that ended at stage 5 */
#define DSH_WARP_SKIPPED 3
#define DSH_WARP_DROPPED 4
#define DSH_WARP_KEPT 5
#define DSH_WARP_STORED 6
typedef struct dsh_warp_pair_input {
  dsh_ctx* ctx;                     /* the context of the store */
  dsh_kfdb* kfdb;                   /* descriptor rows, octaves, scale factors */
  dsh_diffdb* ddb;                  /* receives the DiffProp records */
  int32_t slot, anchor, tag;        /* tag is stored with the records */
  double lambda;
  int32_t min_pairs, max_iters;     /* 20, 3 in the reference */
  float radius;                     /* 2 */
  int32_t th_low;                   /* 50 */
  int32_t n_pairs;
  const int32_t* pair_idx1;         /* key point of the anchor */
  const int32_t* pair_idx2;         /* key point of the new keyframe, distinct */
  int32_t n_queries;
  const int32_t* query_idx1;        /* key points of the anchor, ascending and distinct */
} dsh_warp_pair_input;
typedef struct dsh_warp_pair_result {
  double* x;                        /* 2 NCu NCv */
  uint8_t* pair_state;              /* n_pairs */
  uint8_t* query_state;             /* n_queries */
  int32_t* query_match;             /* n_queries */
  int32_t* query_point;             /* n_queries */
  uint8_t* query_added;             /* n_queries */
  int32_t init_ok, fitted;
  int32_t info[2];                  /* iterations, accepted steps; zeros when fitted == 0 */
  double costs[2];                  /* initial, final cost */
  int64_t first_record;             /* log position of the first record stage 4 appended */
  int32_t n_filtered, n_matched, n_appended, n_list;   /* stage 3, stage 4, records appended, L */
  int32_t n_skipped, n_dropped, n_kept, n_stored;      /* stage 7 */
  int32_t rounds;                   /* of the election of stage 7 */
  dsh_point_erase_counts erase;
} dsh_warp_pair_result;
int dsh_keyframe_warp_pair(dsh_mpdb* db, const dsh_warp_pair_input* in, dsh_warp_pair_result* out);

/* ---- ORB feature front end (ORB_SLAM2::ORBextractor::operator(), Thirdparty/ORBSLAM_2/src/ORBextractor.cc:1047-1118) ----------------
 * Two device stages with the caller's selection between them, split where the reference splits:
 *   detect    image up, pyramid (ComputePyramid, :1120-1145) built and kept resident with its blurred copy (:1098-1099), FAST corners per
 *             30-pixel cell with the two-threshold rule (ComputeKeyPointsOctTree, :765-833), candidates down;
 *   (host)    the caller's DistributeOctTree (:539-763): its sort compares pointers on ties, a few thousand points per frame;
 *   describe  the selected key points up, IC_Angle (:77-104) and computeOrbDescriptor (:108-147) on the resident planes, angles and
 *             descriptors down.
 * Not covered: masks (ComputePyramid with a mask, runByPixelsMask), ComputeKeyPointsOld, DistributeOctTree, Frame's undistortion.
 *
 * READINGS, NOT VERIFIED AGAINST AN OPENCV BUILD.  The OpenCV steps of the reference are restated here in integers or single IEEE float32
 * operations from OpenCV's documented behaviour; no OpenCV build was available to compare with.  Each reading and the behaviour it reads:
 *   level sizes   sf[0] = 1, sf[l] = sf[l-1] * scale_factor in float; inv[l] = 1.0f / sf[l]; size = cvRound((float)W0 * inv[l]) per axis,
 *                 cvRound = round half to even (:415-431, :1124-1125).
 *   resize        cv::resize INTER_LINEAR on 8-bit data, the fixed-point path with INTER_RESIZE_COEF_BITS = 11.  Per axis, sc = (double)src / dst:
 *                 f = (float)((d + 0.5) * sc - 0.5), s = floor(f), f -= s; s < 0: s = 0, f = 0; s >= src - 1: s = src - 1, f = 0; the second tap
 *                 index is clamped to src - 1; taps c0 = cvRound((1.f - f) * 2048), c1 = cvRound(f * 2048).  Horizontal h = S[s] * a0 + S[s+1] * a1,
 *                 vertical D = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2.
 *   frame         copyMakeBorder with BORDER_REFLECT_101, 19 pixels, made from the level itself (BORDER_ISOLATED) for every level.
 *   blur          cv::GaussianBlur 7 x 7, sigma 2, 8-bit: weights q = cvRound(k * 256) of the normalised double Gaussian, (18, 34, 49, 55, 49,
 *                 34, 18), sum 257, not renormalised; row pass then column pass in exact integers over the frame; min(255, (sum + 32768) >> 16).
 *                 The blurred plane is defined 3 pixels beyond the level on every side, computed from the frame: inside the level this is the
 *                 reference's blur of the cloned level, outside it replaces what the reference reads outside its cloned buffer.
 *   FAST          cv::FAST 9/16 with non-maximum suppression on each cell's sub-image.  d_k = I(circle_k) - I(p) on the radius-3 circle of 16;
 *                 M(p) = the maximum over the 16 arcs of 9 contiguous circle pixels and both signs of min_k(+-d_k); p is a corner at threshold t
 *                 iff M(p) > t and its response is M(p) - 1 (cornerScore<16>).  Corners only at least 3 pixels inside the sub-image; a corner is
 *                 kept iff its response is strictly greater than that of its 8 neighbours, where a neighbour that is no corner at the threshold
 *                 in use or lies outside the cell's detection region counts 0.  A cell runs at ini_th_fast and, only if that leaves it empty,
 *                 again at min_th_fast.  Cells as :773-806 computes them.
 *   angle         cv::fastAtan2 as the scalar polynomial: c = min(ax, ay) / (max(ax, ay) + (float)DBL_EPSILON), a = (((p7 c^2 + p5) c^2 + p3) c^2 + p1) c
 *                 with p1, p3, p5, p7 = 0.9997878412794807f, -0.3258083974640975f, 0.1555786518463281f, -0.04432655554792128f, each times
 *                 (float)(180 / pi); 90 - a if ay > ax, 180 - a if x < 0, 360 - a if y < 0.  The moments are integers over the circular patch of
 *                 the unblurred level centred at (cvRound(x), cvRound(y)).
 *   descriptor    ang = angle * (float)(pi / 180.f); a = (float)cos((double)ang), b = (float)sin((double)ang); pattern point (px, py) samples the
 *                 blurred plane at row cy + cvRound(px * b + py * a), column cx + cvRound(px * a - py * b); bit k of byte i is
 *                 sample(16 i + 2 k) < sample(16 i + 2 k + 1).  All float arithmetic is float32, one rounding per operation.
 * The sampling pattern (the reference's bit_pattern_31_) is an argument, as it is of computeOrbDescriptor.
 *
 * Candidates of a level come in the reference's order: cell row, cell column, then raster (y, then x) inside the cell; coordinates are
 * level pixels (the reference's pt after :847-848), the response is M - 1.  The placement does not depend on scheduling.
 * A context is named inside the configuration; the extractor is a device-resident object like the stores: destroying its context first
 * is safe (every later call but the destroy returns DSH_ERR_ARG).  On a host-only context the create and the level sizes work, the three
 * calls that need the device return DSH_ERR_NO_DEVICE after their argument checks. */
typedef struct dsh_orb dsh_orb;
typedef struct dsh_orb_config {
  dsh_ctx* ctx;
  int32_t width, height, levels;    /* 1 <= levels <= 32; every level at least 62 pixels in both dimensions */
  float scale_factor;               /* > 1 */
  int32_t ini_th_fast, min_th_fast; /* 1 <= min <= ini <= 255 */
  int32_t capacity;                 /* candidates per level */
  const int32_t* pattern;           /* 512 points: x, y, with x^2 + y^2 <= 342 */
} dsh_orb_config;
int dsh_orb_create(const dsh_orb_config* cfg, dsh_orb** out);
int dsh_orb_destroy(dsh_orb* orb);
int dsh_orb_level_sizes(const dsh_orb* orb, int32_t* wh /* levels*2: width, height */, float* scale /* levels: sf[l] */);
/* counts[l]: the candidates of level l; cand[(l * capacity + i) * 3]: x, y, response.  A level with more candidates than capacity is
 * DSH_ERR_ARG (the message names the level and the count), counts still holds the true counts and cand the first `capacity` of a level. */
int dsh_orb_detect(dsh_orb* orb, const uint8_t* image, int64_t row_stride, int32_t* counts /* levels */, int32_t* cand /* levels*capacity*3 */);
/* Key points of the last detected image: level and position in level pixels, the rounded position at least 16 pixels from every edge of
 * the level.  DSH_ERR_STATE before the first detect. */
int dsh_orb_describe(dsh_orb* orb, int32_t n, const int32_t* level, const float* xy /* n*2, level pixels */, float* angle /* n, degrees */,
                     uint8_t* desc /* n*32 */);
/* Tests, debugging.  blurred == 0: the level with its 19-pixel frame, (h + 38) rows of (w + 38); else the blurred plane, (h + 6) rows of (w + 6). */
int dsh_orb_get_plane(dsh_orb* orb, int32_t level, int32_t blurred, uint8_t* out);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* DEFSLAM_HIP_H */
