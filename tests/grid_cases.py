"""Control grids other than the reference's 13 x 15 for the mapping kernels (tests/test_mapping_grids_cpu.py, test_mapping_grids_gpu.py):
the grids with what each of them reaches in defslam_amd/csrc/nrsfm_kernels.hip, the inputs of every case, and references in plain numpy
that share no code with the C oracle (SVD least squares, normal equations refined with long-double residuals, central differences, a
brute-force match search)."""
import numpy as np

from defslam_amd import synth

# (nptsu, nptsv), the ones nearest to 13 x 15 first.  Fit: N <= 256 control points.
#   13 x 15  control: the grid every other test runs on
#   15 x 13  the usual size transposed; band of 6 tiles
#   16 x 16  the limit: N 256, 2N = np = 512, no padding, band of 7 tiles (the widest one of the register-window factorisation)
#   14 x 18  first grid of the memory factorisation with interleaved unknowns (band of 8 tiles); np 512 with 8 padded rows
#   8 x 8    2N = 128: no padding, NT = 8 = the number of row-owning waves
#   4 x 18   2N = 144, NT 9, band 8 = NT - 1: a band that is dense
#   6 x 40   band of 16 tiles; Warp::initialize's own band reaches 8 tiles (its memory factorisation)
#   4 x 5, 5 x 4   2N = 40 (8 rows of padding); the two index strides told apart
#   4 x 4    N 16: np 32, NT 2, band 1; one knot cell, every 7 x 7 neighbourhood clipped on all sides
FIT_GRIDS = [(13, 15), (15, 13), (16, 16), (14, 18), (8, 8), (4, 18), (6, 40), (4, 5), (5, 4), (4, 4)]
# Shape from Normals and Warp::initialize: N <= 512.  22 x 23: N 506, 6 rows of padding; 16 x 32: N 512, NT 32, the limit
SOLVE_GRIDS = FIT_GRIDS + [(22, 23), (16, 32)]
FIT_ITERS = 6


def gid(g):
    return f"{g[0]}x{g[1]}"


def fit_tiles(nu, nv):
    """(np, NT, bwt) of the fit's 2N x 2N solve: padded size, 16 x 16 tiles per side, sub-diagonal tiles of the band of the interleaved
    unknowns (half-bandwidth 2 (3 nptsv + 3) + 1)."""
    n2 = 2 * nu * nv
    npad = 16 * ((n2 + 15) // 16)
    return npad, npad // 16, min(npad // 16 - 1, (2 * (3 * nv + 3) + 1 + 15) // 16)


def init_tiles(nu, nv):
    """(np, NT, bwt) of Warp::initialize's N x N solve (half-bandwidth 3 nptsv + 3); Shape from Normals solves the same size densely."""
    N = nu * nv
    npad = 16 * ((N + 15) // 16)
    return npad, npad // 16, min(npad // 16 - 1, (3 * nv + 3 + 15) // 16)


# Fit cases per grid: (P, lambda, sigma).  The start is make_warp_problem's own start plus N(0, sigma) on every control point: from the
# unperturbed start most grids reject every step (the start already is a regularised fit), and a fit that accepts nothing compares
# nothing.  sigma is NOT proportional to the knot spacing: a control point moves the warp by about its own displacement whatever the
# grid, and a match is dropped beyond 10 px, i.e. 0.02 in normalised coordinates -- so 0.005 .. 0.02 everywhere, found with the oracle
# alone (test_mapping_grids_cpu.py asserts for every case: an accepted step, a rejected step, at most half of the matches dropped).
# 6 x 40 has many control points per match along v; it only keeps its matches with lambda 0.1 and five matches per control point.
FIT_CASES = {
    (13, 15): [(585, 0.3, 0.01), (975, 0.1, 0.02)],
    (15, 13): [(585, 0.3, 0.005), (585, 0.3, 0.02)],
    (16, 16): [(768, 0.3, 0.01), (1280, 0.1, 0.01)],
    (14, 18): [(756, 0.3, 0.005), (1260, 0.1, 0.02)],
    (8, 8): [(192, 0.3, 0.01), (320, 0.1, 0.02)],
    (4, 18): [(216, 0.3, 0.01), (360, 0.1, 0.02)],
    (6, 40): [(1200, 0.1, 0.01), (1200, 0.1, 0.02)],
    (4, 5): [(60, 0.3, 0.01), (100, 0.1, 0.005)],
    (5, 4): [(100, 0.1, 0.01)],
    (4, 4): [(60, 0.3, 0.01), (80, 0.1, 0.02)],
}
FIT_PARAMS = [(g, k) for g in FIT_GRIDS for k in range(len(FIT_CASES[g]))]
FIT_IDS = [f"{gid(g)}-{k}" for g, k in FIT_PARAMS]


def fit_problem(grid, k):
    """(problem of synth.make_warp_problem with the perturbed start in x0, lambda)."""
    P, lam, sigma = FIT_CASES[grid][k]
    pr = synth.make_warp_problem(P, 5, grid[0], grid[1])
    pr["x0"] = pr["x0"] + np.random.default_rng(5).normal(scale=sigma, size=pr["x0"].size)
    return pr, lam


def oracle_fit(oracle, pr, lam, iters=FIT_ITERS):
    return oracle.schwarp_fit(pr["bbs"], pr["kp1"], pr["kp2"], pr["invsig"], pr["fy"], pr["fx"], lam, pr["fx"], pr["fy"], pr["x0"], iters)


def eval_problem(grid):
    """Inputs of one residual / Jacobian evaluation: three matches per control point, a point away from the start."""
    N = grid[0] * grid[1]
    pr = synth.make_warp_problem(max(3 * N, 57), 8, grid[0], grid[1])
    x = pr["x0"] + np.random.default_rng(8).normal(scale=5e-3, size=pr["x0"].shape)
    return pr, x, 0.7


# ---- Shape from Normals ---------------------------------------------------------------------------------------------------------------
SFN_BENDING = 1e-3


def sfn_scene(grid):
    N = grid[0] * grid[1]
    return synth.make_sfn_scene(max(400, 3 * N), seed=4, nu=grid[0], nv=grid[1])


def sfn_lstsq(oracle, sc, lam=SFN_BENDING):
    """SVD least squares of the stacked system [M; Bending; 1^T] x = [0; 0; N mean depth] (ShapeFromNormals.cc:95 solves it by QR):
    (x, rank, condition number)."""
    bbs = sc["bbs"]
    N = bbs[2] * bbs[5]
    A = np.vstack([oracle.sfn_rows(bbs, sc["u"], sc["v"], sc["normals"]), oracle.sfn_bending(bbs, lam), np.ones((1, N))])
    b = np.zeros(A.shape[0])
    b[-1] = N * sc["mean_depth"]
    ref, _, rank, sv = np.linalg.lstsq(A, b, rcond=None)
    return ref, int(rank), float(sv[0] / sv[-1])


# ---- Warp::initialize -----------------------------------------------------------------------------------------------------------------
INIT_LAMBDA = 1e-2


def init_problem(grid):
    N = grid[0] * grid[1]
    return synth.make_warp_problem(max(3 * N, 60), 5, grid[0], grid[1])


def init_system(oracle, pr, lam=INIT_LAMBDA):
    """Normal equations of Warps::Warp::initialize, (C^T C + Bending) X = C^T kp2 with X = [x | y] (N x 2), built in numpy from the
    colocation matrix (oracle.bbs_coloc, pinned to the reference's bbs.cc) and the bending matrix."""
    bbs = pr["bbs"][:6] + (1,)
    N = bbs[2] * bbs[5]
    kp1 = pr["kp1"].astype(np.float64)
    cols, w, n_out = oracle.bbs_coloc(bbs, kp1[:, 0], kp1[:, 1])
    assert n_out == 0
    Cm = np.zeros((kp1.shape[0], N))
    np.add.at(Cm, (np.repeat(np.arange(kp1.shape[0]), 16), cols.ravel()), w.ravel())
    return Cm.T @ Cm + oracle.sfn_bending(bbs, lam), Cm.T @ pr["kp2"].astype(np.float64)


def refine(A, rhs):
    """float64 solve refined with long-double residuals (three steps)."""
    x = np.linalg.solve(A, rhs).astype(np.longdouble)
    Al, bl = A.astype(np.longdouble), rhs.astype(np.longdouble)
    for _ in range(3):
        r = bl - Al @ x
        x = x + np.linalg.solve(A, r.astype(np.float64)).astype(np.longdouble)
    return x


def backward_error(A, x, rhs):
    """Normwise backward error of A x = rhs, the residual accumulated in long double."""
    r = A.astype(np.longdouble) @ x.astype(np.longdouble) - rhs.astype(np.longdouble)
    return float(np.abs(r).max() / (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(rhs).max()))


def init_check(A, rhs, x2n):
    """x2n = [x | y] as the entry points return it.  (backward error, forward error against the refined solve, condition number)."""
    N = A.shape[0]
    X = np.stack([x2n[:N], x2n[N:]], 1)
    eta = max(backward_error(A, X[:, c], rhs[:, c]) for c in range(2))
    xt = refine(A, rhs)
    fe = float(np.abs(X.astype(np.longdouble) - xt).max() / np.abs(xt).max())
    return eta, fe, float(np.linalg.cond(A, np.inf))


# ---- Schwarzian Jacobian of the oracle against central differences --------------------------------------------------------------------
def check_schwarp_oracle_jacobian(oracle, P, nu, nv, seed=4):
    pr = synth.make_warp_problem(P, seed, nu, nv)
    N = nu * nv
    x = pr["x0"] + np.random.default_rng(seed).normal(scale=5e-3, size=2 * N)
    r, J = oracle.schwarp_eval(pr["bbs"], pr["kp1"], pr["kp2"], pr["invsig"], pr["fy"], pr["fx"], 0.7, x)
    for k in [0, N // 2, N - 1, N, N + (7 * N) // 13, 2 * N - 1]:
        d = np.zeros(2 * N)
        d[k] = 1e-6
        fd = (oracle.schwarp_eval(pr["bbs"], pr["kp1"], pr["kp2"], pr["invsig"], pr["fy"], pr["fx"], 0.7, x + d, False)[0] -
              oracle.schwarp_eval(pr["bbs"], pr["kp1"], pr["kp2"], pr["invsig"], pr["fy"], pr["fx"], 0.7, x - d, False)[0]) / 2e-6
        np.testing.assert_allclose(fd[2 * P:], J[2 * P:, k], rtol=1e-5, atol=1e-7)     # Schwarzian: true derivative
        if k < N:   # warp x rows: -coloc*fx_slot, i.e. the true derivative divided by invSigma (the constant Jacobian has no invSigma)
            np.testing.assert_allclose(fd[:P], J[:P, k] * pr["invsig"], rtol=1e-5, atol=1e-6)
    np.testing.assert_array_equal(J[:P], J[P:2 * P])            # Schwarp.cc:291-298 copies the x rows over the y rows
    assert (J[:2 * P, N:] == 0).all()
    # an affine warp has zero Schwarzian derivative
    iu, iv = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    aff = np.concatenate([(0.3 + 1.1 * iu - 0.2 * iv).ravel(), (-0.1 + 0.4 * iu + 0.9 * iv).ravel()])
    ra, _ = oracle.schwarp_eval(pr["bbs"], pr["kp1"], pr["kp2"], pr["invsig"], pr["fy"], pr["fx"], 0.7, aff, False)
    assert np.abs(ra[2 * P:]).max() < 1e-9


# ---- warp-guided match search: the grid-walking oracle against a brute force ----------------------------------------------------------
def check_match_search_brute_force(oracle, sc):
    """The oracle against mapping_views.brute_force -- an independent numpy statement with the explicit tie-break key (distance, grid column,
    grid row, index) -- at the view every scene had before tests/mapping_views.py."""
    import mapping_views as mv
    m = oracle.search_by_schwarp(sc["bbs"], sc["x"], sc["kp1"], sc["desc1"], sc["cam2"], sc["bounds2"], sc["kp2"], sc["desc2"], sc["has_mp2"])
    assert (m >= 0).sum() > 50
    exp = mv.brute_force(sc, mv.VIEWS["base"])
    for q in range(sc["kp1"].shape[0]):
        assert m[q] == exp[q], q
    return m


# ---- one batch of fits on different grids ---------------------------------------------------------------------------------------------
# (grid, P, lambda, start): start = ("x0", k): the perturbed start of FIT_CASES[grid][k] (P and lambda from there);
# ("init", weight): the fit starts from Warp::initialize with that bending weight, computed inside the call; ("init", weight, "same
# domain"): as before, with the domain of the previous fit as well -- dsh_schwarp.cpp shares one bending matrix between consecutive problems
# whose dsh_bbs and init_lambda are equal, and only a batch of different grids takes both branches of that test.  Every grid of
# FIT_GRIDS appears, every P differs, the largest grid (16 x 16) is neither first nor last; an initialisation with bending weight 0.01 is
# so close to the fitted warp that the small grids accept no step from it, 1.0 and 30.0 leave every fit steps to accept and to reject.
BATCH = [
    ((13, 15), 585, 0.3, ("init", 1.0)),
    ((15, 13), 500, 0.1, ("init", 1.0)),                   # same weight as the fit before it, another grid: a bending matrix of its own
    ((15, 13), 430, 0.3, ("init", 1.0, "same domain")),    # same grid, domain and weight: the bending matrix of the fit before it
    ((4, 5), None, None, ("x0", 0)),                       # a fit without initialisation in between
    ((5, 4), 100, 0.1, ("init", 1.0)),
    ((16, 16), None, None, ("x0", 0)),                     # the largest grid sizes every launch: the fits around it are all smaller
    ((14, 18), 756, 0.3, ("init", 30.0)),
    ((4, 4), None, None, ("x0", 1)),
    ((6, 40), 1200, 0.3, ("init", 30.0)),
    ((4, 18), 216, 0.3, ("init", 1.0)),
    ((8, 8), None, None, ("x0", 1)),
]


def batch_problems():
    """The fits of BATCH as dicts: bbs (tuple), kp1, kp2, invsig, fx, fy, lam, and x0 or init_lam."""
    out = []
    for grid, P, lam, start in BATCH:
        if start[0] == "x0":
            pr, lam = fit_problem(grid, start[1])
            q = dict(x0=pr["x0"])
        else:
            pr = synth.make_warp_problem(P, 6, grid[0], grid[1])
            q = dict(init_lam=start[1])
            if len(start) > 2:
                prev = out[-1]["bbs"]
                assert prev[2] == grid[0] and prev[5] == grid[1]
                k1 = pr["kp1"].astype(np.float64)
                assert prev[0] < k1[:, 0].min() and k1[:, 0].max() < prev[1] and prev[3] < k1[:, 1].min() and k1[:, 1].max() < prev[4]
                pr["bbs"] = prev
        q.update(grid=grid, bbs=pr["bbs"], kp1=pr["kp1"], kp2=pr["kp2"], invsig=pr["invsig"], fx=pr["fx"], fy=pr["fy"], lam=lam)
        out.append(q)
    return out
