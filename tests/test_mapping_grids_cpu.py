"""CPU: the mapping-side oracles on control grids other than 13 x 15 (tests/grid_cases.py).  The oracle is the reference of the GPU tests
of test_mapping_grids_gpu.py and had itself only run at 13 x 15: here it is pinned at the other grids against references that share no
code with it (numpy.linalg.lstsq, normal equations built in numpy and refined with long-double residuals, central differences, a brute
force), and the conditions the GPU tests put on their inputs are asserted on the oracle alone, where there is no GPU."""
import numpy as np
import pytest

import grid_cases as gc


def test_every_grid_reaches_what_it_was_chosen_for():
    """The sizes nrsfm_kernels.hip derives from the grid (nrsfm_swp_fit_fill, nrsfm_swp_solve): padded size, tiles, band."""
    assert gc.fit_tiles(13, 15) == (400, 25, 7) and gc.init_tiles(13, 15) == (208, 13, 3)       # what every other test sees
    assert gc.fit_tiles(4, 4) == (32, 2, 1) and gc.init_tiles(4, 4) == (16, 1, 0)               # NT 2 / NT 1, one knot cell
    assert gc.fit_tiles(4, 5)[0] - 2 * 20 == 8 and gc.fit_tiles(5, 4)[0] - 2 * 20 == 8          # 8 rows of padding
    assert gc.fit_tiles(8, 8) == (128, 8, 4) and 2 * 64 == 128                                  # no padding, NT = the 8 row-owning waves
    assert gc.fit_tiles(15, 13)[2] == 6
    assert gc.fit_tiles(16, 16) == (512, 32, 7) and 2 * 256 == 512                              # the limit, no padding, register window
    assert gc.fit_tiles(14, 18) == (512, 32, 8) and 512 - 2 * 252 == 8                          # memory factorisation, interleaved
    assert gc.fit_tiles(4, 18) == (144, 9, 8) and 2 * 72 == 144                                 # band = NT - 1: dense
    assert gc.fit_tiles(6, 40)[2] == 16 and gc.init_tiles(6, 40)[2] == 8                        # Warp::initialize's memory factorisation
    assert gc.init_tiles(16, 32) == (512, 32, 7) and gc.init_tiles(22, 23)[0] - 506 == 6
    assert all(nu * nv <= 256 for nu, nv in gc.FIT_GRIDS) and all(nu * nv <= 512 for nu, nv in gc.SOLVE_GRIDS)
    assert set(gc.FIT_CASES) == set(gc.FIT_GRIDS)
    # bands the 13 x 15 grid cannot reach, on both sides of the switch between the two factorisations (bwt <= 7 / bwt > 7)
    bands = {gc.fit_tiles(*g)[2] for g in gc.FIT_GRIDS}
    assert {1, 6, 7, 8, 16} <= bands
    assert {gc.init_tiles(*g)[1] for g in gc.SOLVE_GRIDS} >= {1, 2, 4, 32}


@pytest.mark.parametrize("grid", gc.SOLVE_GRIDS, ids=gc.gid)
def test_sfn_oracle_against_numpy_lstsq(oracle_mod, grid):
    """oracle.sfn_estimate (Householder QR) against an SVD least-squares solve of the same stacked system.  The system has full rank and a
    condition number below 1e6 on every grid (measured: 1.1e3 .. 3.4e5, the worst is 4 x 18) -- the condition under which the device's
    refined semi-normal equations are held to 1e-6 in test_mapping_grids_gpu.py.  Bound of the comparison: the 1e-9 the suite already uses
    for QR against SVD at 13 x 15 (tests/test_oracle_sfn.py); two backward-stable solvers differ by a small multiple of cond x 2^-53, which
    is 4e-11 at the worst grid (measured: at most 6.3e-13)."""
    sc = gc.sfn_scene(grid)
    N = grid[0] * grid[1]
    ref, rank, cond = gc.sfn_lstsq(oracle_mod, sc)
    assert rank == N and cond < 1e6, (rank, cond)
    ok, raw, ctrl, pts = oracle_mod.sfn_estimate(sc["bbs"], sc["u"], sc["v"], sc["normals"], gc.SFN_BENDING, sc["mean_depth"], sc["u_all"], sc["v_all"])
    assert ok
    err = float(np.abs(raw - ref).max() / np.abs(ref).max())
    print(f"\n[sfn oracle {gc.gid(grid)}] cond {cond:.2e}, oracle - lstsq {err:.2e} relative")
    assert err <= 1e-9
    med = np.sort(raw.astype(np.float32))[N // 2]
    np.testing.assert_allclose(ctrl, raw * (np.float32(1) / med), rtol=1e-15)


@pytest.mark.parametrize("grid", gc.FIT_GRIDS, ids=gc.gid)
def test_schwarp_oracle_jacobian_on_other_grids(oracle_mod, grid):
    """The Schwarzian block of oracle.schwarp_eval against central differences, y rows = x rows, zero second-coordinate block of the warp
    rows, zero Schwarzian residual of an affine warp: test_schwarp_oracle_schwarzian_jacobian_... with the grid as a parameter."""
    gc.check_schwarp_oracle_jacobian(oracle_mod, 120, grid[0], grid[1])


@pytest.mark.parametrize("grid", gc.SOLVE_GRIDS, ids=gc.gid)
def test_warp_initialize_oracle_against_refined_normal_equations(oracle_mod, grid):
    """oracle.warp_initialize against (C^T C + Bending) X = C^T kp2 built in numpy and solved with long-double refinement.  The oracle
    is a plain Cholesky solve: its normwise backward error is bounded by about (3 N + 1) 2^-53 (Higham, Accuracy and Stability, thm
    10.4), the forward error by the first-order bound kappa x backward error.  Measured: backward error 2.7e-17 .. 3.4e-16, forward error 6.7e-15 .. 5.7e-12,
    condition numbers 6.4e3 (16 x 16) .. 8.7e6 (4 x 4)."""
    pr = gc.init_problem(grid)
    N = grid[0] * grid[1]
    A, rhs = gc.init_system(oracle_mod, pr)
    ok, x = oracle_mod.warp_initialize(pr["bbs"], pr["kp1"], pr["kp2"], gc.INIT_LAMBDA)
    assert ok and np.isfinite(x).all()
    eta, fe, kappa = gc.init_check(A, rhs, x)
    print(f"\n[warp initialize oracle {gc.gid(grid)}] backward error {eta:.2e}, forward error {fe:.2e}, condition number {kappa:.2e}")
    assert eta <= (3 * N + 1) * 2.0 ** -53, eta
    assert kappa * eta < 0.5 and fe <= 2.0 * kappa * eta / (1.0 - kappa * eta) + 4.0 * 2.0 ** -53, (fe, kappa, eta)
    # the device is held to 1e-9 max |x| against the oracle: meaningful only while the oracle itself is that close to the solution
    assert fe < 1e-10, fe


def test_match_search_oracle_equals_brute_force_on_another_grid(oracle_mod):
    from defslam_amd import synth
    sc = synth.make_match_scene(300, 500, seed=4, nu=6, nv=40)
    assert sc["bbs"][2] == 6 and sc["bbs"][5] == 40 and sc["x"].size == 480
    gc.check_match_search_brute_force(oracle_mod, sc)


# ---- conditions on the inputs of the GPU tests, on the oracle alone -------------------------------------------------------------------
@pytest.mark.parametrize("grid,k", gc.FIT_PARAMS, ids=gc.FIT_IDS)
def test_fit_cases_accept_and_reject_steps_and_keep_their_matches(oracle_mod, grid, k):
    """A fit whose every step is rejected, or that drops nearly all matches, compares almost nothing: every case has an accepted step, a
    rejected one, and keeps at least half of its matches."""
    pr, lam = gc.fit_problem(grid, k)
    x, diff, drop, info, costs = gc.oracle_fit(oracle_mod, pr, lam)
    P = pr["kp1"].shape[0]
    print(f"\n[fit {gc.gid(grid)}-{k}] {info[0]} iterations, {info[1]} accepted, {int(drop.sum())} of {P} dropped, cost {costs[0]:.6g} -> {costs[1]:.6g}")
    assert info[1] >= 1 and info[1] < info[0] <= gc.FIT_ITERS
    assert costs[1] < costs[0] * (1 - 1e-3)           # a decrease far from the acceptance threshold's rounding edge
    assert drop.sum() <= P // 2
    assert not np.array_equal(x, pr["x0"])


def test_mixed_batch_is_what_the_gpu_test_needs(oracle_mod):
    probs = gc.batch_problems()
    grids = [q["grid"] for q in probs]
    Ps = [q["kp1"].shape[0] for q in probs]
    assert len(probs) >= 6 and set(grids) == set(gc.FIT_GRIDS) and len(set(Ps)) == len(Ps)
    N = [g[0] * g[1] for g in grids]
    assert 0 < int(np.argmax(N)) < len(N) - 1                                       # the largest grid neither first nor last
    init = [q.get("init_lam", 0.0) for q in probs]
    pairs = list(zip(range(len(probs) - 1), range(1, len(probs))))
    assert any(init[a] > 0 and init[a] == init[b] and probs[a]["bbs"] == probs[b]["bbs"] for a, b in pairs)      # shared bending matrix
    assert any(init[a] > 0 and init[a] == init[b] and grids[a] != grids[b] for a, b in pairs)                      # same weight, other grid
    assert any(init[a] > 0 and init[b] == 0 and any(i > 0 for i in init[b + 1:]) for a, b in pairs)                # no initialisation in between
    assert len({i for i in init if i > 0}) >= 2
    both = False
    for q in probs:
        x0 = q["x0"] if "x0" in q else oracle_mod.warp_initialize(q["bbs"], q["kp1"], q["kp2"], q["init_lam"])[1]
        x, diff, drop, info, costs = oracle_mod.schwarp_fit(q["bbs"], q["kp1"], q["kp2"], q["invsig"], q["fy"], q["fx"], q["lam"], q["fx"], q["fy"], x0, gc.FIT_ITERS)
        assert info[1] >= 1 and drop.sum() <= drop.size // 2, (q["grid"], info)
        assert costs[1] < costs[0] * (1 - 1e-3)
        both = both or (gc.fit_tiles(*q["grid"])[2] >= 8 and 1 <= info[1] < info[0])
    assert both       # accepted and rejected steps at a grid of the memory factorisation
