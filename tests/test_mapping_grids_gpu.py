"""GPU: the mapping entry points that take the B-spline control grid as a run-time argument, on grids other than the reference's 13 x 15
(tests/grid_cases.py says what each grid reaches in nrsfm_kernels.hip: both factorisations with interleaved unknowns, no padding, one
tile, a dense band, the limits of 256 / 512 control points, clipped neighbourhoods, batches whose fits are smaller than the launch).
Product context, through the C ABI; same assertions and tolerances as tests/test_nrsfm_gpu.py has at 13 x 15.  The CPU side -- the oracle
pinned at these grids, the conditions on the inputs -- is tests/test_mapping_grids_cpu.py."""
import numpy as np
import pytest

import grid_cases as gc

pytestmark = pytest.mark.gpu


def _bbs(t):
    from defslam_amd import nrsfm
    return nrsfm.Bbs(*t)


def _assert_fit_follows_oracle(dev, ora):
    """The assertions of test_schwarp_fit_matches_oracle."""
    xg, dg, drg, ig, cg = dev[:5]
    xo, do, dro, io, co = ora
    np.testing.assert_array_equal(ig, io)                                   # iterations and accepted steps
    np.testing.assert_allclose(cg, co, rtol=1e-10)
    np.testing.assert_allclose(xg, xo, rtol=0, atol=1e-9 * max(1.0, np.abs(xo).max()))
    np.testing.assert_array_equal(drg, dro)                                 # which matches are dropped (> 10 px)
    np.testing.assert_allclose(dg, do, rtol=2e-6, atol=1e-6)                # float32 DiffProp fields
    # J21 fields exactly as SchwarpDatabase.cc:322-329 assigns them (note: b and c trade places w.r.t. the matrix inverse)
    a, b, c, d = dg[:, 4], dg[:, 5], dg[:, 6], dg[:, 7]
    det = a * d - c * b
    good = np.abs(det) > 0.2
    assert good.any()
    np.testing.assert_allclose(dg[good, 8], (d / det)[good], rtol=1e-5)
    np.testing.assert_allclose(dg[good, 9], (-c / det)[good], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(dg[good, 10], (-b / det)[good], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(dg[good, 11], (a / det)[good], rtol=1e-5)


def _assert_same_bits(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[3], b[3])
    np.testing.assert_array_equal(a[4], b[4])


def _assert_eval_follows_oracle(ctx, oracle, pr, x, lam):
    """The assertions of test_schwarp_residuals_and_jacobian_match_oracle, for any problem of synth.make_warp_problem."""
    from defslam_amd import nrsfm
    P, N = pr["kp1"].shape[0], pr["bbs"][2] * pr["bbs"][5]
    b = _bbs(pr["bbs"])
    ro, Jo = oracle.schwarp_eval(pr["bbs"], pr["kp1"], pr["kp2"], pr["invsig"], pr["fy"], pr["fx"], lam, x)
    rg, Jg = nrsfm.schwarp_eval(ctx, b, pr["kp1"], pr["kp2"], pr["invsig"], pr["fy"], pr["fx"], lam, x)
    np.testing.assert_array_equal(Jg != 0, Jo != 0)                       # sparsity: bit-exact tap indexing
    np.testing.assert_allclose(rg, ro, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(Jg, Jo, rtol=1e-13, atol=1e-15)
    np.testing.assert_array_equal(Jg[:P], Jg[P:2 * P])                     # quirk: y rows are copies of the x rows
    assert (Jg[:2 * P, N:] == 0).all()
    # the Schwarzian block is the true derivative (central differences); columns taken from N: a first coordinate, a second one, the last
    for k in [N // 5, N + N // 2, 2 * N - 1]:
        d = np.zeros_like(x)
        d[k] = 1e-6
        fd = (nrsfm.schwarp_eval(ctx, b, pr["kp1"], pr["kp2"], pr["invsig"], pr["fy"], pr["fx"], lam, x + d, False)[0] -
              nrsfm.schwarp_eval(ctx, b, pr["kp1"], pr["kp2"], pr["invsig"], pr["fy"], pr["fx"], lam, x - d, False)[0]) / 2e-6
        np.testing.assert_allclose(fd[2 * P:], Jg[2 * P:, k], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("grid", gc.FIT_GRIDS, ids=gc.gid)
def test_schwarp_eval_matches_oracle_on_every_grid(gpu_ctx, oracle_mod, grid):
    """Warps::Warp::Evaluate + Warps::Schwarzian::Evaluate: residuals and the dense Jacobian, as test_schwarp_residuals_and_jacobian_match_oracle."""
    pr, x, lam = gc.eval_problem(grid)
    _assert_eval_follows_oracle(gpu_ctx, oracle_mod, pr, x, lam)


@pytest.mark.parametrize("grid,k", gc.FIT_PARAMS, ids=gc.FIT_IDS)
def test_schwarp_fit_matches_oracle_on_every_grid(gpu_ctx, oracle_mod, grid, k):
    """SchwarpDatabase::calculateSchwarps: same accept / reject sequence, control points and DiffProp records as the oracle, six iterations
    from a perturbed start (every case accepts and rejects steps: test_mapping_grids_cpu.py)."""
    from defslam_amd import nrsfm
    pr, lam = gc.fit_problem(grid, k)
    ora = gc.oracle_fit(oracle_mod, pr, lam)
    dev = nrsfm.calculateSchwarps(gpu_ctx, _bbs(pr["bbs"]), pr["kp1"], pr["kp2"], pr["invsig"], pr["fy"], pr["fx"], lam, pr["fx"], pr["fy"], pr["x0"], gc.FIT_ITERS)
    print(f"\n[fit {gc.gid(grid)}-{k}] device {dev[3].tolist()} oracle {ora[3].tolist()}, costs {dev[4].tolist()} / {ora[4].tolist()}, "
          f"max |x - oracle| {np.abs(dev[0] - ora[0]).max():.2e}")
    assert 1 <= ora[3][1] < ora[3][0]
    _assert_fit_follows_oracle(dev, ora)


def _batch(probs, with_store=False):
    out = []
    for i, q in enumerate(probs):
        d = dict(bbs=_bbs(q["bbs"]), kp1=q["kp1"], kp2=q["kp2"], invsig=q["invsig"], fx_slot=q["fy"], fy_slot=q["fx"], lam=q["lam"], fx=q["fx"], fy=q["fy"],
                 max_iters=gc.FIT_ITERS)
        if "x0" in q:
            d["x0"] = q["x0"]
        else:
            d["init_lam"] = q["init_lam"]
        if with_store:
            P = q["kp1"].shape[0]
            d["point_id"] = (10000 * i + np.arange(P)).astype(np.int32)
            d["point_id"][::7] = -1                                       # matches of no stored point
            d["tag"] = 500 + i
        out.append(d)
    return out


def test_schwarp_fit_batch_of_different_grids(gpu_ctx, oracle_mod):
    """dsh_schwarp_fit_batch with one batch over all ten grids (grid_cases.BATCH): every launch is sized by the largest fit (16 x 16, in the
    middle), so every other fit is smaller than the launch in N, 2N, np and P; fits with Warp::initialize inside share the bending matrix
    with their predecessor (same dsh_bbs and weight) or build their own (same weight on another grid; after a fit without initialisation).
    Every result is bit-identical to the single calls and follows the oracle; the same batch through dsh_schwarp_fit_batch_store returns the
    same bits and stores the kept records."""
    from defslam_amd import nrsfm
    probs = gc.batch_problems()
    res = nrsfm.calculateSchwarpsBatch(gpu_ctx, _batch(probs))
    kept = 0
    for i, (q, r) in enumerate(zip(probs, res)):
        b = _bbs(q["bbs"])
        if "x0" in q:
            x0 = q["x0"]
        else:
            ok, x0 = nrsfm.WarpInitialize(gpu_ctx, b, q["kp1"], q["kp2"], q["init_lam"])
            assert ok and r[5] == ok, i
        single = nrsfm.calculateSchwarps(gpu_ctx, b, q["kp1"], q["kp2"], q["invsig"], q["fy"], q["fx"], q["lam"], q["fx"], q["fy"], x0, gc.FIT_ITERS)
        _assert_same_bits(r, single)
        # the oracle from the same start (the device's own initialisation: test_warp_initialize_... holds it to the oracle's)
        ora = oracle_mod.schwarp_fit(q["bbs"], q["kp1"], q["kp2"], q["invsig"], q["fy"], q["fx"], q["lam"], q["fx"], q["fy"], x0, gc.FIT_ITERS)
        print(f"\n[batch {i} {gc.gid(q['grid'])}] device {r[3].tolist()} oracle {ora[3].tolist()}, max |x - oracle| {np.abs(r[0] - ora[0]).max():.2e}")
        assert ora[3][1] >= 1
        _assert_fit_follows_oracle(r, ora)
    sprobs = _batch(probs, with_store=True)
    db = nrsfm.DiffDatabase(gpu_ctx, 64)                                   # grows on demand
    try:
        stored = nrsfm.calculateSchwarpsBatch(gpu_ctx, sprobs, db=db)
        for r, s, q in zip(res, stored, sprobs):
            _assert_same_bits(r[:5], s[:5])
            kept += int(((q["point_id"] >= 0) & ~s[2]).sum())
        assert len(db) == kept > 0
    finally:
        db.close()


@pytest.fixture(scope="module")
def oracle_init_backward_error(oracle_mod):
    """The worst backward error of the oracle's own Cholesky solve over the systems of the test below (CPU)."""
    worst = 0.0
    for grid in gc.SOLVE_GRIDS:
        pr = gc.init_problem(grid)
        A, rhs = gc.init_system(oracle_mod, pr)
        ok, x = oracle_mod.warp_initialize(pr["bbs"], pr["kp1"], pr["kp2"], gc.INIT_LAMBDA)
        assert ok
        worst = max(worst, gc.init_check(A, rhs, x)[0])
    return worst


@pytest.mark.parametrize("grid", gc.SOLVE_GRIDS, ids=gc.gid)
def test_warp_initialize_on_every_grid(gpu_ctx, oracle_mod, oracle_init_backward_error, grid):
    """Warps::Warp::initialize against the oracle (1e-9 max |x|, as at 13 x 15) and against (C^T C + Bending) X = C^T kp2 built in numpy:
    normwise backward error, the residual in long double, at most ten times the worst backward error the oracle's own Cholesky solve has on
    the same twelve systems (one order of magnitude for the device's tile-order sums); forward error against the refined solve within the
    first-order bound kappa x backward error.  Measured on an MI355X: oracle 2.7e-17 .. 3.4e-16 over the twelve systems (so the bound is 3.4e-15), device 4.3e-17 (5 x 4) .. 3.1e-16
    (16 x 16); forward error of the device 6.2e-15 .. 6.5e-12 at condition numbers 6.4e3 .. 8.7e6 (the worst of both is 4 x 4)."""
    from defslam_amd import nrsfm
    pr = gc.init_problem(grid)
    oko, xo = oracle_mod.warp_initialize(pr["bbs"], pr["kp1"], pr["kp2"], gc.INIT_LAMBDA)
    okg, xg = nrsfm.WarpInitialize(gpu_ctx, _bbs(pr["bbs"]), pr["kp1"], pr["kp2"], gc.INIT_LAMBDA)
    assert oko and okg and np.isfinite(xg).all()
    A, rhs = gc.init_system(oracle_mod, pr)
    eta, fe, kappa = gc.init_check(A, rhs, xg)
    print(f"\n[warp initialize {gc.gid(grid)}] device backward error {eta:.2e} (oracle's worst {oracle_init_backward_error:.2e}), forward error {fe:.2e}, "
          f"condition number {kappa:.2e}, max |x - oracle| / max |x| {np.abs(xg - xo).max() / np.abs(xo).max():.2e}")
    np.testing.assert_allclose(xg, xo, rtol=0, atol=1e-9 * np.abs(xo).max())
    assert eta <= 10.0 * oracle_init_backward_error, (eta, oracle_init_backward_error)
    assert kappa * eta < 0.5 and fe <= 2.0 * kappa * eta / (1.0 - kappa * eta) + 4.0 * 2.0 ** -53, (fe, kappa, eta)


@pytest.mark.parametrize("grid", gc.SOLVE_GRIDS, ids=gc.gid)
def test_shape_from_normals_on_every_grid(gpu_ctx, oracle_mod, grid):
    """ShapeFromNormals::estimate against numpy.linalg.lstsq of the stacked system at 1e-6 max |ref| (the tolerance the suite uses for this
    comparison): the device solves semi-normal equations with two refinement steps, each contracting the error by about cond(A)^2 2^-53,
    which is safe while cond(A) stays below about 1e6 -- asserted from the singular values (3.4e5 at worst, 4 x 18).  And against the
    oracle as test_shape_from_normals_matches_oracle does."""
    from defslam_amd import nrsfm
    sc = gc.sfn_scene(grid)
    N = grid[0] * grid[1]
    ref, rank, cond = gc.sfn_lstsq(oracle_mod, sc)
    assert rank == N and cond < 1e6, (rank, cond)
    okg, rawg, ctrlg, ptsg = nrsfm.ShapeFromNormals(gpu_ctx, _bbs(sc["bbs"]), sc["u"], sc["v"], sc["normals"], gc.SFN_BENDING, sc["mean_depth"], sc["u_all"], sc["v_all"])
    oko, rawo, ctrlo, ptso = oracle_mod.sfn_estimate(sc["bbs"], sc["u"], sc["v"], sc["normals"], gc.SFN_BENDING, sc["mean_depth"], sc["u_all"], sc["v_all"])
    assert okg and oko
    print(f"\n[shape from normals {gc.gid(grid)}] cond {cond:.2e}, device - lstsq {np.abs(rawg - ref).max() / np.abs(ref).max():.2e}, "
          f"device - oracle {np.abs(rawg - rawo).max() / np.abs(rawo).max():.2e} relative")
    np.testing.assert_allclose(rawg, ref, rtol=0, atol=1e-6 * np.abs(ref).max())
    np.testing.assert_allclose(rawg, rawo, rtol=0, atol=1e-8 * np.abs(rawo).max())
    np.testing.assert_allclose(ctrlg, ctrlo, rtol=0, atol=1e-6 * np.abs(ctrlo).max())   # float32 median in the scale factor
    np.testing.assert_allclose(ptsg, ptso, rtol=2e-6, atol=1e-6)
    assert ptsg.dtype == np.float32


@pytest.mark.parametrize("grid", [(6, 40), (4, 4)], ids=gc.gid)
def test_search_by_schwarp_bit_exact_on_other_grids(gpu_ctx, oracle_mod, grid):
    from defslam_amd import nrsfm, synth
    sc = synth.make_match_scene(600, 900, seed=2, nu=grid[0], nv=grid[1])
    assert sc["x"].size == 2 * grid[0] * grid[1]
    mo = oracle_mod.search_by_schwarp(sc["bbs"], sc["x"], sc["kp1"], sc["desc1"], sc["cam2"], sc["bounds2"], sc["kp2"], sc["desc2"], sc["has_mp2"])
    mg = nrsfm.searchBySchwarp(gpu_ctx, _bbs(sc["bbs"]), sc["x"], sc["kp1"], sc["desc1"], sc["cam2"], sc["bounds2"], sc["kp2"], sc["desc2"], sc["has_mp2"])
    np.testing.assert_array_equal(mg, mo)
    assert (mo >= 0).sum() >= 60


def test_grids_beyond_the_limits_are_refused_and_leave_the_context_usable(gpu_ctx):
    """258 control points in the fit and the batch, 513 in Shape from Normals and Warp::initialize, nptsu = 3 and umax = umin everywhere:
    DSH_ERR_ARG (include/defslam_hip.h states the limits), and a 13 x 15 fit on the same context gives the bits it gave before."""
    from defslam_amd import nrsfm, synth
    from defslam_amd.sft import DshError
    status = "status 1:"                                                     # DSH_ERR_ARG (include/defslam_hip.h)
    pr = synth.make_warp_problem(300, 3)
    b = _bbs(pr["bbs"])

    def fit(bb, x0=pr["x0"]):
        return nrsfm.calculateSchwarps(gpu_ctx, bb, pr["kp1"], pr["kp2"], pr["invsig"], pr["fy"], pr["fx"], 0.1, pr["fx"], pr["fy"], x0, 3)

    before = fit(b)
    sc = synth.make_sfn_scene(200, seed=1)

    def grid(t, nu, nv, valdim):
        return nrsfm.Bbs(t[0], t[1], nu, t[3], t[4], nv, valdim)

    def problem(bb):
        N = bb.nptsu * bb.nptsv
        return dict(bbs=bb, kp1=pr["kp1"], kp2=pr["kp2"], invsig=pr["invsig"], fx_slot=pr["fy"], fy_slot=pr["fx"], lam=0.1, fx=pr["fx"], fy=pr["fy"], x0=np.zeros(2 * N),
                    max_iters=3)

    good = problem(b)
    good["x0"] = pr["x0"]
    flat = nrsfm.Bbs(b.umin, b.umin, 13, b.vmin, b.vmax, 15, 2)              # umax = umin
    refused = 0
    for bb in (grid(pr["bbs"], 6, 43, 2), grid(pr["bbs"], 3, 15, 2), flat):
        N = bb.nptsu * bb.nptsv
        with pytest.raises(DshError, match=status):
            fit(bb, np.zeros(2 * N))
        with pytest.raises(DshError, match=status):
            nrsfm.calculateSchwarpsBatch(gpu_ctx, [good, problem(bb), good])   # one bad fit refuses the batch
        with pytest.raises(DshError, match=status):
            nrsfm.calculateSchwarpsBatch(gpu_ctx, [dict(problem(bb), init_lam=1e-2)])
        refused += 3
    for bb in (grid(pr["bbs"], 3, 15, 2), flat):
        N = bb.nptsu * bb.nptsv
        with pytest.raises(DshError, match=status):
            nrsfm.schwarp_eval(gpu_ctx, bb, pr["kp1"], pr["kp2"], pr["invsig"], pr["fy"], pr["fx"], 0.1, np.zeros(2 * N))
        with pytest.raises(DshError, match=status):
            nrsfm.searchBySchwarp(gpu_ctx, bb, np.zeros(2 * N), pr["kp1"], np.zeros((300, 32), np.uint8), np.array([520.0, 515.0, 322.5, 241.25], np.float32),
                                  np.array([0.0, 640.0, 0.0, 480.0], np.float32), np.zeros((5, 2), np.float32), np.zeros((5, 32), np.uint8), np.zeros(5, np.uint8))
        refused += 2
    for bb in (grid(pr["bbs"], 19, 27, 2), grid(pr["bbs"], 3, 15, 2), flat):
        with pytest.raises(DshError, match=status):
            nrsfm.WarpInitialize(gpu_ctx, bb, pr["kp1"], pr["kp2"], 1e-2)
        b1 = nrsfm.Bbs(sc["bbs"][0], sc["bbs"][0] if bb is flat else sc["bbs"][1], bb.nptsu, sc["bbs"][3], sc["bbs"][4], bb.nptsv, 1)
        with pytest.raises(DshError, match=status):
            nrsfm.ShapeFromNormals(gpu_ctx, b1, sc["u"], sc["v"], sc["normals"], 1e-3, sc["mean_depth"], sc["u_all"], sc["v_all"])
        refused += 2
    assert refused == 19
    # the limits themselves are accepted (16 x 16 and 16 x 32 run in the tests above); the context is as it was
    _assert_same_bits(fit(b), before)
    after = nrsfm.calculateSchwarpsBatch(gpu_ctx, [good])[0]
    _assert_same_bits(after, before)
