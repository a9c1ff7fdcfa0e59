"""The three normals kernels (normals_coeff_kernel, normals_solve_kernel, normals_propagate_kernel) and the DiffProp fields of the batched
Schwarp fit against plane geometry in closed form (tests/normals_geometry.py), next to the usual parity with the oracle.  The cases, the
counted sets and every tolerance are fixed on the CPU by tests/test_normals_geometry_cpu.py; nothing here is derived from a device result."""
import numpy as np
import pytest

import normals_geometry as ng

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ng.CASE_IDS)
def test_normals_match_the_oracle_and_the_plane_geometry(gpu_ctx, oracle_mod, name):
    """ObtainK1K2 on quirk-neutral records of rigid planar scenes: parity with the oracle on every point (as test_normals_match_oracle asserts
    it), and on the oracle's counted set k1k2, normal_ref and normal_rec within TOL_FACTOR x the oracle's own measured error of the closed
    form.  The shape edges run here too: P = 1, P = block size -+ 1, R no multiple of the block, a point without reference records between
    solved points, a point with reference records only, 2 .. 6 records per point."""
    from defslam_amd import nrsfm
    sc = ng.make_scene(name)
    o = oracle_mod.normals(*ng.args(sc))
    g = nrsfm.ObtainK1K2(gpu_ctx, *ng.args(sc))
    # parity, points left out by the cap included
    np.testing.assert_array_equal(g.status, o["status"])
    np.testing.assert_array_equal(g.rec_written, o["rec_written"])
    np.testing.assert_array_equal(g.iters, o["iters"])
    solved = o["status"] == 0
    np.testing.assert_allclose(g.k1k2[solved], o["k1k2"][solved], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(g.cov[solved], o["cov"][solved], rtol=1e-7)
    np.testing.assert_allclose(g.normal_ref[solved], o["normal_ref"][solved], rtol=0, atol=1e-6)
    wr = o["rec_written"].astype(bool)
    np.testing.assert_allclose(g.normal_rec[wr], o["normal_rec"][wr], rtol=0, atol=1e-6)
    # the closed form, on the ORACLE's counted set
    cand, counted = ng.classify(sc, o["k1k2"], o["status"])
    assert (int(cand.sum()), int(counted.sum())) == ng.MEASURED[name]["counted"]
    e = ng.truth_errors(sc, counted, g.k1k2, g.normal_ref, g.normal_rec)
    eo = ng.truth_errors(sc, counted, o["k1k2"], o["normal_ref"], o["normal_rec"])
    print(f"\n[{name}] P {sc['k_true'].shape[0]} R {sc['recs'].shape[0]} counted {counted.sum()} of {cand.sum()}; to the closed form, device (oracle, recorded): " +
          ", ".join(f"{k} {e[k]:.2e} ({eo[k]:.2e}, {ng.MEASURED[name][k]:.2e})" for k in e))
    for k in e:
        assert e[k] <= ng.TOL_FACTOR * ng.MEASURED[name][k], k


def _device_fits(ctx, plane, grid):
    """The four pairs of one plane on one grid: WarpInitialize per pair, then the four Schwarzian fits as one batch."""
    from defslam_amd import nrsfm
    prs = [ng.warp_pair(plane, m, grid) for m in range(len(ng.WARP_MOTIONS))]
    probs = []
    for pr in prs:
        b = nrsfm.Bbs(*pr["bbs"])
        ok, x0 = nrsfm.WarpInitialize(ctx, b, pr["kp1"], pr["kp2"], ng.WARP_INIT_LAMBDA)
        assert ok
        probs.append(dict(bbs=b, kp1=pr["kp1"], kp2=pr["kp2"], invsig=pr["invsig"], fx_slot=pr["fy"], fy_slot=pr["fx"], lam=ng.WARP_FIT_LAMBDA, fx=pr["fx"], fy=pr["fy"],
                          x0=x0, max_iters=ng.WARP_FIT_ITERS))
    return prs, nrsfm.calculateSchwarpsBatch(ctx, probs)


@pytest.mark.parametrize("plane,grid", ng.WARP_PARAMS, ids=ng.WARP_IDS)
def test_fitted_warp_fields_are_the_derivatives_of_the_homography(gpu_ctx, plane, grid):
    """WarpInitialize + calculateSchwarpsBatch on exact homography matches: fields 4-7 and 12-17 against the homography's analytic
    derivatives, 8-11 against the analytic inverse Jacobian, within TOL_FACTOR x the oracle's measured error (b and c differ by more than
    100 such tolerances, so the slot order is pinned).  Then the chain: the device's own records of the four pairs, quirk_neutral on the
    host, ObtainK1K2, the plane's normal on the inner set -- median and 90th percentile, never the maximum of a fit error."""
    from defslam_amd import nrsfm
    rec = ng.WARP_MEASURED[(plane, grid)]
    prs, res = _device_fits(gpu_ctx, plane, grid)
    worst = dict(first=0.0, inverse=0.0, second=0.0)
    for pr, r in zip(prs, res):
        assert not r[2].any() and r[3][1] >= 1                                 # no match dropped; the fit moved the warp
        assert np.abs(pr["truth"][:, ng.F_b] - pr["truth"][:, ng.F_c]).min() > 100 * ng.TOL_FACTOR * rec["first"]
        np.testing.assert_array_equal(r[1][:, :4], np.c_[pr["kp1"], pr["kp2"]])
        for k, v in ng.warp_field_errors(r[1], pr).items():
            worst[k] = max(worst[k], v)
    g = nrsfm.ObtainK1K2(gpu_ctx, *ng.chain_inputs([r[1] for r in res]))
    assert (g.status == 0).all()
    med, p90, mx = ng.chain_errors(g.k1k2, prs[0])
    graw = nrsfm.ObtainK1K2(gpu_ctx, *ng.chain_inputs([r[1] for r in res], neutral=False))
    print(f"\n[{plane} {grid}] device fit to analytic fields (recorded oracle): " + ", ".join(f"{k} {v:.2e} ({rec[k]:.2e})" for k, v in worst.items()) +
          f"; fits (iterations, accepted) {[tuple(int(i) for i in r[3]) for r in res]}; chain median {med:.2e} ({rec['chain_median']:.2e}), 90th percentile {p90:.2e} "
          f"({rec['chain_p90']:.2e}), max {mx:.2e}; without the transform: median {ng.chain_errors(graw.k1k2, prs[0])[0]:.2e}")
    for k, v in dict(worst, chain_median=med, chain_p90=p90).items():
        assert v <= ng.TOL_FACTOR * rec[k], k
