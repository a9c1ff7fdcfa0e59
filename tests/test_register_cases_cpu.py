"""CPU: the surface registration cases of tests/register_cases.py are sound before a GPU sees them.  Every OptimizeHorn case reaches the
path it is named for (oracle.horn_counts(), in the device's summation order), the oracle's two summation orders agree on it, and the
oracle's estimate is the closed-form similarity; the scaleMinMedian inputs give the same bits from the oracle and from numpy sorting; the
oracle chain says what the end-to-end cases expect of the device.

Measured with the committed oracle (profiles/register_cases/README.md has the table): order to order at most 8.2e-10 where every pair is
an inlier and 9.0e-9 on heavy_outliers; oracle to closed form between 1.9e-11 and 1.19e-5 (size_255, where the first optimize(50) stops
on its relative-gain rule before the last digits settle)."""
import numpy as np
import pytest

import register_cases as rc


def test_scene_draws_in_the_generators_order():
    from defslam_amd import synth
    for kw in (dict(), dict(noise=0.0, outliers=0.0, scale=1.3), dict(noise=5e-3, outliers=0.3)):
        g = synth.make_register_scene(37, seed=9, **kw)
        full = dict(noise=2e-3, outliers=0.05, scale=1.35)
        full.update(kw)
        s = rc.scene(37, 9, rc.GEN_ROTVEC, rc.GEN_T, **full)
        for k in ("surface", "map"):
            np.testing.assert_array_equal(s[k].view(np.uint32), g[k].view(np.uint32))
        np.testing.assert_array_equal(s["outlier"], g["outlier"])
    p = rc.scene(37, 9, (0.3, 0.1, -0.2), (0, 0, 0), 1.2, planar=True)
    assert (p["surface"][:, 2] == 1.0).all()
    np.testing.assert_array_equal(p["surface"][:, :2], s["surface"][:, :2])


def test_stream_has_exactly_the_listed_candidates(oracle_mod):
    from defslam_amd import synth
    sc = synth.make_register_scene(50, seed=1)
    for cands in ([0, 49], [7], [], list(range(50))):
        u = rc.stream(50, cands, np.random.default_rng(2))
        assert u.shape[0] == 50 + 49 * len(cands) and (u >= 0).all() and (u <= 1).all()
        med = np.asarray(oracle_mod.scale_min_median(sc["surface"], sc["map"], u)["medians"])
        np.testing.assert_array_equal(np.nonzero(med >= 0)[0], sorted(cands))


def test_umeyama_recovers_an_exact_similarity_and_refuses_a_reflection():
    rng = np.random.default_rng(0)
    a = rng.standard_normal((40, 3))
    from scipy.spatial.transform import Rotation as Rot
    R0 = Rot.from_rotvec([2.0, -1.0, 0.5]).as_matrix()
    R, t, s = rc.umeyama(a, 0.37 * a @ R0.T + [1, 2, 3])
    np.testing.assert_allclose(R, R0, atol=1e-13)
    np.testing.assert_allclose(t, [1, 2, 3], atol=1e-13)
    assert abs(s - 0.37) < 1e-13
    np.testing.assert_allclose(rc.quat_R(Rot.from_matrix(R0).as_quat()), R0, atol=1e-14)
    R, t, s = rc.umeyama(a, a * [1, 1, -1])      # a mirror image: the best PROPER rotation, never a reflection
    assert abs(np.linalg.det(R) - 1) < 1e-12


@pytest.mark.parametrize("name", rc.NAMES)
def test_case_reaches_its_path(oracle_mod, name):
    r = rc.oracle_run(oracle_mod, name, True)
    c = r["counts"]
    for k, least in rc.CASES[name][1].items():
        assert c[k] >= least, (k, c)
    assert c["ldlt_not_ok"] == 0
    assert c["exp_both_small"] + c["exp_sigma_small"] + c["exp_theta_small"] + c["exp_general"] == c["quat_trace"] + c["quat_i0"] + c["quat_i1"] + c["quat_i2"]
    n = rc.case_scene(name)["surface"].shape[0]
    if name == "heavy_outliers":
        for order in (True, False):
            o = rc.oracle_run(oracle_mod, name, order)
            assert (o["ok"], o["count"], list(o["iters"])) == (False, 40, [5, 3])
    elif name == "nan_point":
        for order in (True, False):
            o = rc.oracle_run(oracle_mod, name, order)
            assert (o["ok"], o["count"], list(o["iters"]), list(o["trials"])) == (False, n, [50, 50], [50, 50])
            assert np.isnan(o["chi2"])
            np.testing.assert_array_equal(o["sim3"], np.array(rc.START, float))
    else:
        assert r["ok"] and r["count"] == n                # converges: every pair an inlier, verdict acceptable
    if name.startswith("half_turn"):
        assert r["iters"][0] >= 12


@pytest.mark.parametrize("name", rc.NAMES)
def test_case_is_stable_under_the_summation_order(oracle_mod, name):
    d, e = rc.oracle_run(oracle_mod, name, True), rc.oracle_run(oracle_mod, name, False)
    assert d["ok"] == e["ok"] and d["count"] == e["count"]
    dist = np.abs(d["sim3"] - e["sim3"]).max()
    print(f"{name}: order to order {dist:.3g}")
    assert dist < 1e-8
    for r in (d, e):
        c2 = rc.edge_chi2(r["sim3"], rc.case_scene(name))
        c2 = c2[np.isfinite(c2)]
        assert (np.abs(c2 / rc.CHI - 1) > 1e-6).all()      # no edge whose inlier verdict the last bits decide


@pytest.mark.parametrize("name", rc.CLOSED_FORM)
def test_oracle_estimate_is_the_closed_form_similarity(oracle_mod, name):
    sc = rc.case_scene(name)
    for order in (True, False):
        dist = rc.closed_form_distance(rc.oracle_run(oracle_mod, name, order)["sim3"], sc)
        print(f"{name}: oracle to closed form {dist:.3g}")
        assert dist < 2.5e-5
    kw = rc.CASES[name][0]
    # ... which is the alignment the scene was made with, to its noise: n pairs with noise sigma on a surface whose smallest rms extent
    # is 0.15 (and which lies at distance 1, so the translation carries the rotation's error) leave sigma / (0.15 sqrt(n)); five of those
    R, t, s = rc.umeyama(sc["surface"], sc["map"])
    bound = 5 * kw["noise"] / (0.15 * np.sqrt(kw["n"]))
    assert np.abs(R - sc["R"]).max() < bound and np.abs(t - sc["t"]).max() < bound and abs(s - kw["scale"]) < bound


def test_closed_form_cases_are_all_but_the_two_without_one():
    assert sorted(set(rc.NAMES) - set(rc.CLOSED_FORM)) == ["heavy_outliers", "nan_point"]
    assert len(rc.NAMES) == 15 + len(rc.SIZES)


@pytest.mark.parametrize("name", list(rc.SMM_CASES))
def test_scale_inputs_agree_between_oracle_and_numpy(oracle_mod, name):
    mono, stereo, u = rc.smm_inputs(name)
    o = oracle_mod.scale_min_median(mono, stereo, u)
    with np.errstate(invalid="ignore", divide="ignore"):
        s, k, st = rc.smm_numpy(mono, stereo, u)
    assert (o["status"], o["consumed"]) == (st, k)
    assert rc.same_scale(o["scale"], s)
    n = mono.shape[0]
    if name in ("n1", "n2"):
        assert (st, s) == (2, 0.0)
    elif name == "exact_fit":
        assert st == 0 and np.isnan(s) and (o["medians"][o["medians"] >= 0] == 0).all()
    elif name == "tie_below_300":      # k zeros, then pair 0's residual, which is the median of every candidate
        res = np.sqrt(((2.0 * mono.astype(np.float64) - stereo) ** 2).sum(1)).astype(np.float32)
        k = 1 + (n - 2) // 2
        assert int((res == 0).sum()) - 1 == k and res[0] == np.sort(res[res > 0])[0] and res[256] == 0
        np.testing.assert_array_equal(np.nonzero(o["medians"] >= 0)[0], rc.TIE_CANDS)
        assert (o["medians"][rc.TIE_CANDS] == res[0]).all() and res[0] > 0.01
        assert st == 0 and abs(s - 2.0) < 0.05
    else:
        assert st == 0 and abs(s - 1.35) < 0.06
    if name in ("n8000_12", "n4097_9"):
        assert (n, int((o["medians"] >= 0).sum())) == {"n8000_12": (8000, 12), "n4097_9": (4097, 9)}[name]
        assert u.shape[0] == k < 2 * 10 ** 5
    if name == "ends_300":
        assert o["medians"][0] >= 0 and o["medians"][n - 1] >= 0
    if name == "equal_240":      # the four copies of a pair share one residual: the counted median sits inside a run of equal values
        i = int(np.nonzero(o["medians"] >= 0)[0][0])
        scale = np.float32(stereo[i, 2]) / np.float32(mono[i, 2])
        res = np.linalg.norm(float(scale) * mono.astype(np.float64) - stereo, axis=1).astype(np.float32)
        assert np.unique(res).shape[0] <= 60


@pytest.mark.parametrize("name", rc.REGISTER_CASES)
def test_oracle_chain_of_the_end_to_end_cases(oracle_mod, name):
    a, b, u, Twc = rc.register_inputs(name)
    s0, o, (s22, Tcw) = rc.oracle_chain(oracle_mod, a, b, u, Twc)
    assert s0["status"] == 0
    if name == "exact_fit":      # the NaN scale: 50 + 50 iterations that change nothing, then the non-finite total: not acceptable
        assert np.isnan(s0["scale"]) and not o["ok"] and list(o["iters"]) == [50, 50] and np.isnan(o["chi2"])
        return
    assert o["ok"] and o["count"] == a.shape[0]
    want = 1.3 if name == "rotated" else 1.35
    assert abs(s22 - want) < 0.02
    R = Twc[:3, :3].astype(np.float64)
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-6)
    Tn = np.eye(4); Tn[:3, :3] = o["sim3"][7] * rc.quat_R(o["sim3"][:4]); Tn[:3, 3] = o["sim3"][4:7]
    Tn = Tn @ Twc.astype(np.float64)
    Tn[:3, :3] /= s22
    np.testing.assert_allclose(Tcw.astype(np.float64) @ Tn, np.eye(4), atol=2e-5)
