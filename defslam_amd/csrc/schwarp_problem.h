// Device-side records of the Schwarzian warp fit (dsh_schwarp_fit, _fit_batch, _fit_batch_store: dsh_schwarp.cpp -> nrsfm_kernels.hip):
// the descriptor of one fit, the sizes a control grid gives it, the layout of its structured-Jacobian block and the launcher of a batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

struct SwpPar { double umin, umax, vmin, vmax, fxs, fys, lambda; int nu, nv, N, P; };

// Padded size of the one-workgroup tile Cholesky solve (nrsfm_swp_solve, _resolve): M takes np * np doubles, Winv np * 16.
inline int nrsfm_swp_solve_np(int n) { return 16 * ((n + 15) / 16); }

// What (nu, nv, P) give a fit: 2N unknowns, m = 2P + 4N residuals, the padded size np of the 2N x 2N solve, il = 1 (the solver interleaves
// the two coordinates: the matrix is banded, half-bandwidth 2 (3 nv + 3) + 1) and its band bwt in 16 x 16 tiles; npi / bwti: the same for
// the N x N system of Warp::initialize (colocation and bending couple a 4 x 4 patch of control points: half-bandwidth 3 nv + 3).
struct SwpSizes { int n2, m, np, il, bwt, npi, bwti; };
inline SwpSizes swp_sizes(int nu, int nv, int P) {
  const int N = nu * nv;
  auto band = [](int np, int half) { const int dense = np / 16 - 1, t = (half + 15) / 16; return dense < t ? dense : t; };
  SwpSizes s;
  s.n2 = 2 * N; s.m = 2 * P + 4 * N; s.np = nrsfm_swp_solve_np(s.n2); s.il = 1;
  s.bwt = band(s.np, 2 * (3 * nv + 3) + 1);
  s.npi = nrsfm_swp_solve_np(N);
  s.bwti = band(s.npi, 3 * nv + 3);
  return s;
}

// One fit of a batch.  The B fits advance together, one launch per stage with the fit in blockIdx.y (blockIdx.z for the 2D grids); each
// kernel reads its arguments from the fit's descriptor.  The trust-region control of the reference's Ceres run (SchwarpDatabase.cc:211-222;
// oracle/schwarp_oracle.c restates it) runs in swpb_ctl_kernel on the device: the whole batch is a fixed sequence of launches without a
// single host synchronisation, and a finished fit skips its stages by a flag.
struct SwpFit {
  SwpPar p;                      // domain, grid, P, N, slots, lambda
  float fx, fy;                  // true focal lengths (DiffProp drop test)
  int n2, m, np, il, bwt, max_iters;   // swp_sizes
  const float *kp1, *kp2, *isg;
  double *x, *xn, *cs, *g, *dx, *r, *J, *A, *M, *W, *scal;   // scal: [0] cost [1] sqrt(rho') [2] solve ok [3] model change [4] |step| [5] |x| [6] max |g|
  float* diff;
  uint8_t* drop;
  int32_t* info;                 // [0] iterations [1] accepted steps [2] verdict on the initialisation
  double* costs;                 // [0] initial [1] final
  // trust-region state (Ceres LM as restated in oracle/schwarp_oracle.c), owned by swpb_ctl_kernel
  double radius, nu, cost, cost0, change, old;
  int it, good, invalid, done, accepted, pending;   // pending: an accepted step was re-linearised, its max |g| has not been tested yet
  // optional first stage, Warps::Warp::initialize (Schwarp.cc:99-160): x = the regularised linear fit of the warp with this bending
  // matrix (N x N, shared by the fits of one grid and weight; NULL: x holds the caller's start value).  It borrows the buffers of
  // the fit: C in J, the two right-hand sides in r, C^T C + Bending in A, C^T kp2 in g, the factor in M / W.
  const double* bend;
  int npi, bwti;                 // swp_sizes
  // Structured Jacobian of the fit (every row touches the 4 x 4 patch of control points of ONE knot cell -- SURVEY 7 K11): the warp rows
  // as 16 values per match (the x row; the reference's y row is a copy of it, Schwarp.cc:291-298), the Schwarzian rows as 32 values per
  // row (16 for each coordinate), and the rows bucketed by knot cell (matches in index order: a fixed summation order).  swp_compact.
  double *Jw, *Js;               // P x 16;  N x 4 x 32 (site, row, [x taps | y taps])
  int32_t *bw_ptr, *bw_idx;      // ncell + 1, P: matches of cell (Iu, Iv) = Iu * (nv - 3) + Iv
  int32_t *bs_ptr, *bs_idx;      // ncell + 1, N: grid sites of the cell
  int32_t* cid;                  // P + N: knot cell of every match / grid site (-1: outside the domain)
};
#define SWP_STAGE_ALWAYS 0      // setup stages: run for every fit
#define SWP_STAGE_ACTIVE 1      // stages of an iteration: skipped once the fit is done
#define SWP_STAGE_ACCEPTED 2    // re-linearisation: only after an accepted step

// The structured-Jacobian block of the fit f (f.p is set): its size in bytes, 64 spare ones included, and -- with a device block of that
// size at `base` -- the slices of it in f.  base == nullptr: the size alone.
inline size_t swp_compact(SwpFit& f, char* base) {
  const size_t P = (size_t)f.p.P, N = (size_t)f.p.N, ncell = (size_t)(f.p.nu - 3) * (f.p.nv - 3);
  size_t off = 0;
  auto take = [&](auto*& slice, size_t bytes) {
    if (base) slice = reinterpret_cast<decltype(slice + 0)>(base + off);
    off += bytes;
  };
  take(f.Jw, 8 * P * 16);
  take(f.Js, 8 * N * 128);
  take(f.bw_ptr, 4 * (ncell + 1));
  take(f.bw_idx, 4 * P);
  take(f.bs_ptr, 4 * (ncell + 1));
  take(f.bs_idx, 4 * N);
  take(f.cid, 4 * (P + N));
  return off + 64;
}

// The batched fit: a fixed sequence of launches over B fit descriptors (device array), no host synchronisation inside.
// maxP / maxN: the largest sizes in the batch (grid extents); max_iters: the largest iteration limit; with_init: a fit has f.bend.
extern "C" hipError_t nrsfm_swp_fit_batch(SwpFit* d_fits, int B, int maxP, int maxN, int max_iters, int with_init, hipStream_t st);
