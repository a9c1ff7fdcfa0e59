"""GPU: the warp-guided match search, the Schwarp fit, the Huber filter and dsh_keyframe_warp_pair away from the one view every other
mapping test uses (tests/mapping_views.py says what each view reaches in match_cells_kernel / match_search_kernel and which cameras the
fit runs at).  Product context, through the C ABI.  The CPU side -- the oracle against an independent brute force at every view, the
edge cases every scene holds, the errors the scenes can tell apart, the conditions on the fit cases -- is test_mapping_views_cpu.py."""
import numpy as np
import pytest

import mapping_views as mv
import warp_pair_ref as WP
from test_mapping_grids_gpu import _assert_eval_follows_oracle, _assert_fit_follows_oracle, _bbs
from test_warp_pair_gpu import _compare, _run_pair

pytestmark = pytest.mark.gpu


# ---- (a) the search -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mv.NAMES)
def test_search_equals_the_oracle_at_every_view(gpu_ctx, oracle_mod, name):
    from defslam_amd import nrsfm
    sc, view = mv.match_scene(name), mv.VIEWS[name]
    args, kw = mv.search_args(sc, view)
    b = _bbs(sc["bbs"])
    radii = [view[3]] + ([40.0] if name == "fine" else [])                  # fine once more with a window of nine cells
    for radius in radii:
        kw["radius"] = radius
        mo = oracle_mod.search_by_schwarp(sc["bbs"], *args, **kw)
        mg = nrsfm.searchBySchwarp(gpu_ctx, b, *args, **kw)
        print(f"\n[{name} radius {radius}] {int((mo >= 0).sum())} of {mo.size} matched, {int((mg != mo).sum())} differ")
        np.testing.assert_array_equal(mg, mo)
        assert (mo >= 0).sum() >= (5 if name == "pow2" else 13)
    kw["radius"] = view[3]
    # every candidate taken / no key point at all
    taken = nrsfm.searchBySchwarp(gpu_ctx, b, *args[:7], np.ones_like(sc["has_mp2"]), **kw)
    assert (taken == -1).all()
    empty = nrsfm.searchBySchwarp(gpu_ctx, b, *args[:5], np.zeros((0, 2), np.float32), np.zeros((0, 32), np.uint8), np.zeros(0, np.uint8), **kw)
    assert empty.shape == (130,) and (empty == -1).all()


# ---- (b) the fit at other cameras -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("point,grid,P", mv.FIT_PARAMS, ids=mv.FIT_IDS)
def test_schwarp_eval_and_fit_follow_the_oracle_at_other_cameras(gpu_ctx, oracle_mod, point, grid, P):
    """Residuals and Jacobian at the perturbed start, then SchwarpDatabase::calculateSchwarps from it: the assertions and tolerances of
    test_mapping_grids_gpu.py.  aniso has matches that the drop rule keeps or drops only because fx and fy sit where they do, narrow has
    knots 0.048 apart, wide a domain of 2.4 x 1.9 (test_mapping_views_cpu.py asserts what every case needs on the oracle alone)."""
    from defslam_amd import nrsfm
    pr = mv.fit_problem(point, grid, P)
    _assert_eval_follows_oracle(gpu_ctx, oracle_mod, pr, pr["x0"], mv.FIT_LAMBDA)
    ora = mv.oracle_fit(oracle_mod, pr)
    dev = nrsfm.calculateSchwarps(gpu_ctx, _bbs(pr["bbs"]), pr["kp1"], pr["kp2"], pr["invsig"], pr["fy"], pr["fx"], mv.FIT_LAMBDA, pr["fx"], pr["fy"], pr["x0"],
                                  mv.FIT_ITERS)
    print(f"\n[fit {point} {grid[0]}x{grid[1]}] device {dev[3].tolist()} oracle {ora[3].tolist()}, costs {dev[4].tolist()} / {ora[4].tolist()}, "
          f"dropped {int(dev[2].sum())} / {int(ora[2].sum())}, max |x - oracle| {np.abs(dev[0] - ora[0]).max():.2e} at max |x| {np.abs(ora[0]).max():.2e}, "
          f"max |diff - oracle| {np.abs(dev[1] - ora[1]).max():.2e}")
    assert 1 <= ora[3][1] < ora[3][0]
    _assert_fit_follows_oracle(dev, ora)


# ---- (c) the filter -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("point,P", mv.FILTER_PARAMS)
def test_initial_schwarp_filter_follows_the_oracle_at_other_cameras(gpu_ctx, oracle_mod, point, P):
    """DefORBmatcher::CalculateInitialSchwarp against the oracle's route (dense Cholesky initialisation, CPU B-spline evaluation, Ceres'
    corrector of the Huber block) as tests/test_integration_shim.py compares them: the control points, the loss-corrected residuals, and
    the same matches removed."""
    from defslam_amd import nrsfm
    pr = mv.filter_problem(point, P)
    x, out_g, res_g = nrsfm.CalculateInitialSchwarp(gpu_ctx, _bbs(pr["bbs"]), pr["kp1"], pr["kp2"], pr["invsig"], pr["fx"], pr["fy"], mv.FILTER_LAMBDA)
    ok_o, x_o = oracle_mod.warp_initialize(pr["bbs"], pr["kp1"], pr["kp2"], mv.FILTER_LAMBDA)
    assert ok_o
    res_o, _ = oracle_mod.schwarp_eval_initial(pr["bbs"], pr["kp1"], pr["kp2"], pr["invsig"], pr["fx"], pr["fy"], x_o)
    print(f"\n[filter {point} P {P}] max |x - oracle| {np.abs(x - x_o).max():.2e}, max |res - oracle| {np.abs(res_g - res_o).max():.2e}, {int(out_g.sum())} removed")
    np.testing.assert_allclose(x, x_o, rtol=0, atol=1e-8)
    np.testing.assert_allclose(res_g, res_o, rtol=1e-7, atol=1e-7)
    raw, _ = oracle_mod.schwarp_eval(pr["bbs"], pr["kp1"], pr["kp2"], pr["invsig"], pr["fx"], pr["fy"], 0.0, x_o, want_jacobian=False)
    assert np.sum(raw[:2 * P] ** 2) > 5.77 ** 2 and np.abs(res_o).max() < np.abs(raw[:2 * P]).max()      # the loss correction is active
    err_o = res_o[2 * np.arange(P)] ** 2 + res_o[2 * np.arange(P) + 1] ** 2
    np.testing.assert_array_equal(out_g, err_o > 20)
    assert 1 <= out_g.sum() < P


# ---- (d) dsh_keyframe_warp_pair with a view per keyframe --------------------------------------------------------------------------------
def _pair_scene():
    """Two anchors at aniso and cropped, the new keyframe at tall; scale factors 1.2 (8 levels) for the first anchor and the new keyframe,
    1.5 (4 levels) for the second anchor, every keyframe's octaves inside its own table.  A tenth of the pairs are outliers: the filter
    removes three and four of them, and other ones at the second anchor with the new keyframe's camera and scale factors."""
    from defslam_amd import synth
    sf8, sf4 = (1.2 ** np.arange(8)).astype(np.float32), (1.5 ** np.arange(4)).astype(np.float32)
    views = [mv.VIEWS["aniso"][:3] + (sf8,), mv.VIEWS["cropped"][:3] + (sf4,), mv.VIEWS["tall"][:3] + (sf8,)]
    sc = synth.make_warp_pair_scene(200, 40, 30, n_anchors=2, seed=23, nu=5, nv=6, outliers=0.1, views=views)
    assert all(a["octave"].max() < len(v[3]) for a, v in zip(sc["anchors"], views)) and sc["anchors"][1]["octave"].max() == 3
    return sc


def test_warp_pair_reads_the_anchors_view_for_the_fit_and_the_new_keyframes_for_the_search(gpu_ctx, oracle_mod):
    """Every keyframe has a view of its own: the call equals the explicit sequence bit for bit (which takes the camera and the scale
    factors of the filter and the fit from the anchor, and camera, bounds, grid and pixel key points of the search from the new
    keyframe: warp_pair_ref.view_of), its matches are the oracle's search at the new keyframe's view, and the explicit sequence with the
    two views exchanged gives another result -- so a call that read s2 for s1 anywhere would not pass."""
    from defslam_amd import nrsfm
    sc = _pair_scene()
    kw = dict(radius=3.0, th_low=80, max_iters=6)       # three iterations accept no step from this start, and x would say nothing about the fit
    m = WP.build_model(sc)
    new = len(m.kfs) - 1
    # the start and the matches alone: a call that never fits returns the initialisation
    A0 = sc["anchors"][0]
    m0 = WP.clone(m)
    st0, ks0 = WP.stores(gpu_ctx, sc, m0)
    ddb0 = nrsfm.DiffDatabase(gpu_ctx, 4)
    g0 = st0.warp_pair(ks0, ddb0, new, 0, A0["pair_idx1"], A0["pair_idx2"], A0["query_idx1"], sc["lam"], min_pairs=10 ** 6, **kw)
    assert not g0.fitted
    has = np.array(m.kfs[new].table) != -1
    has[A0["pair_idx2"][g0.pair_state == WP.FILTERED]] = False
    K2, bounds2, grid2, _ = WP.view_of(sc)
    mo = oracle_mod.search_by_schwarp(A0["bbs"], g0.x, A0["kpn"][A0["query_idx1"]], A0["desc"][A0["query_idx1"]], K2, bounds2, sc["px2"], sc["desc2"], has,
                                      radius=3.0, th_low=80, grid=grid2)
    np.testing.assert_array_equal(g0.query_match, mo)
    assert (mo >= 0).sum() >= 1
    # both anchors in sequence against the explicit sequence, and against the explicit sequence with the views exchanged
    st, ks = WP.stores(gpu_ctx, sc, m)
    ddb_a, ddb_b, ddb_x = nrsfm.DiffDatabase(gpu_ctx, 4), nrsfm.DiffDatabase(gpu_ctx, 4), nrsfm.DiffDatabase(gpu_ctx, 4)
    stored = []
    for a, A in enumerate(sc["anchors"]):
        mx = WP.clone(m)
        g, r = _run_pair(gpu_ctx, sc, m, st, ks, ddb_a, ddb_b, a, A["pair_idx1"], A["pair_idx2"], A["query_idx1"], tag=7 + a, **kw)
        stored += r["stored"]
        _compare(gpu_ctx, st, g, r, m, sc, ddb_a, ddb_b, f"anchor {a}", all_stored=stored)
        print(f"\n[anchor {a}] {g.counts}, {g.erase}, iterations and accepted steps {g.info.tolist()}")
        assert g.fitted and g.info[1] >= 1 and g.counts["n_matched"] >= 1 and g.counts["n_stored"] >= 1
        if a == 0:
            np.testing.assert_array_equal(g.query_match, g0.query_match)
        rx = WP.host_route(gpu_ctx, mx, WP.exchanged(sc), a, A["pair_idx1"], A["pair_idx2"], A["query_idx1"], ddb_x, 7 + a, **kw)
        differs = dict(x=g.x.tobytes() != rx["x"].tobytes(), match=not np.array_equal(g.query_match, rx["match"]),
                       pair_state=not np.array_equal(g.pair_state, rx["pair_state"]))
        print(f"[anchor {a}] against the exchanged views: {differs}")
        assert differs["x"] and differs["match"], differs
