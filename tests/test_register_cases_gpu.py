"""GPU: surface registration away from synth.make_register_scene's one alignment (tests/register_cases.py names every case and what it
reaches; tests/test_register_cases_cpu.py shows the cases sound on the oracle alone).  OptimizeHorn against a closed-form similarity
that shares no code with it, against the oracle in the reference's summation order and, decision for decision, against the oracle in the
device's; scaleMinMedian bit for bit at the host's limit of 8000 pairs, with candidates at both ends of the index range, equal residuals,
the early return and an exact fit; registerSurfaces end to end under other keyframe poses."""
import numpy as np
import pytest

import register_cases as rc

pytestmark = pytest.mark.gpu

# The trajectory comparison holds where the device's sin, cos, exp and pow return the host's bits for the arguments on the trajectory.  A
# case that meets the two other comparisons on the MI355X and misses only this one belongs in ORDER_ONLY, with both sides' counts beside
# it (profiles/register_cases/README.md); nan_point may not be moved.
#
# Moved after the first run on the MI355X: each met the closed form and the edge-order oracle and differed from the device-order oracle by
# at most 8.9e-10 in the estimate.  On the arguments of these trajectories the device's exp, sin or cos is one ulp from glibc's (evaluated
# on the device one by one: size_15 at its first exp(-0.5938...), turn_x at sin(0.2106...)); (exp(sigma) - 1) / sigma and the last bits
# of the sums then decide other trials.  The fifteen cases that stay in EXACT met no such argument on an accepted step.
#                  device iters, trials      device-order oracle iters, trials
ORDER_ONLY = [
    "turn_x",      # [9 3]  [17 11]          [9 3]  [14 12]
    "turn_z",      # [10 1] [17 10]          [10 1] [15 10]
    "half_turn_y", # [12 3] [19 13]          [12 3] [19 16]
    "half_turn_z", # [14 1] [24 10]          [14 3] [22 14]
    "far_turn_z",  # [14 2] [30 14]          [14 3] [22 12]
    "size_15",     # [7 2]  [7 10]           [7 2]  [8 11]
    "size_63",     # [7 3]  [7 9]            [7 1]  [16 9]
    "size_65",     # [7 1]  [16 10]          [7 3]  [10 10]
]
EXACT = [k for k in rc.NAMES if k not in ORDER_ONLY]
assert "nan_point" in EXACT and set(ORDER_ONLY) <= set(rc.NAMES)

_DEVICE = {}


def _device_run(gpu_ctx, name):
    from defslam_amd import register
    if name not in _DEVICE:
        sc = rc.case_scene(name)
        _DEVICE[name] = register.OptimizeHorn(gpu_ctx, sc["surface"], sc["map"], rc.START, chi=rc.CHI, huber=rc.HUBER)
    return _DEVICE[name]


@pytest.mark.parametrize("name", rc.CLOSED_FORM)
def test_optimize_horn_is_the_closed_form_similarity(gpu_ctx, name):
    g = _device_run(gpu_ctx, name)
    dist = rc.closed_form_distance(g["sim3"], rc.case_scene(name))
    print(f"{name}: device to closed form {dist:.3g}")
    assert dist < 1e-4      # the north-star tolerance of this path; the oracle itself is held to 2.5e-5 on the same cases


@pytest.mark.parametrize("name", rc.NAMES)
def test_optimize_horn_matches_oracle_in_edge_order(gpu_ctx, oracle_mod, name):
    g = _device_run(gpu_ctx, name)
    o = rc.oracle_run(oracle_mod, name, False)
    print(f"{name}: device iters {g['iters']} trials {g['trials']} count {g['count']} ok {g['ok']}; edge order iters {o['iters']} trials {o['trials']}; "
          f"estimate {np.nanmax(np.abs(g['sim3'] - o['sim3'])):.3g}")
    assert g["count"] == o["count"] and g["ok"] == o["ok"]
    np.testing.assert_allclose(g["sim3"], o["sim3"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(g["chi2"], o["chi2"], rtol=1e-6, atol=1e-12)
    assert abs(int(g["iters"][0]) - int(o["iters"][0])) <= 3


@pytest.mark.parametrize("name", EXACT)
def test_optimize_horn_follows_the_oracle_in_device_order(gpu_ctx, oracle_mod, name):
    g = _device_run(gpu_ctx, name)
    t = rc.oracle_run(oracle_mod, name, True)
    print(f"{name}: device iters {g['iters']} trials {g['trials']}; device order iters {t['iters']} trials {t['trials']}; "
          f"estimate {np.nanmax(np.abs(g['sim3'] - t['sim3'])):.3g}")
    np.testing.assert_array_equal(g["iters"], t["iters"])
    np.testing.assert_array_equal(g["trials"], t["trials"])
    assert g["count"] == t["count"] and g["ok"] == t["ok"]
    np.testing.assert_allclose(g["sim3"], t["sim3"], rtol=0, atol=1e-13)
    np.testing.assert_allclose(g["chi2"], t["chi2"], rtol=1e-12)
    if name == "nan_point":      # every trial rejected, the start handed back untouched, the non-finite total not acceptable
        assert list(g["iters"]) == list(g["trials"]) == [50, 50] and not g["ok"] and np.isnan(g["chi2"])
        np.testing.assert_array_equal(g["sim3"].view(np.uint64), np.array(rc.START, np.float64).view(np.uint64))


@pytest.mark.parametrize("name", list(rc.SMM_CASES))
def test_scale_min_median_matches_oracle_bit_exact(gpu_ctx, oracle_mod, name):
    from defslam_amd import register
    mono, stereo, u = rc.smm_inputs(name)
    o = oracle_mod.scale_min_median(mono, stereo, u)
    g = register.scaleMinMedian(gpu_ctx, mono, stereo, u)
    print(f"{name}: device {g}; oracle scale {o['scale']} status {o['status']} consumed {o['consumed']}")
    assert g["status"] == o["status"] == (2 if name in ("n1", "n2") else 0)
    assert rc.same_scale(g["scale"], o["scale"])
    # the host walks the stream before the kernels run: where the reference returns early (status 2) it has walked further
    if o["status"] == 0:
        assert g["consumed"] == o["consumed"]
    if name == "exact_fit":
        assert np.isnan(g["scale"])


@pytest.mark.parametrize("name", rc.REGISTER_CASES)
def test_register_surfaces_end_to_end(gpu_ctx, oracle_mod, name):
    from defslam_amd import register
    a, b, u, Twc = rc.register_inputs(name)
    s0, o, (s22, Tcw) = rc.oracle_chain(oracle_mod, a, b, u, Twc)
    g = register.registerSurfaces(gpu_ctx, a, b, u, Twc, chi_limit=0.05, check_chi=True)
    print(f"{name}: device registered {g['registered']} acceptable {g['acceptable']} scale0 {g['scale0']} iters {g['iters']} s22 {g['s22']}; oracle s22 {s22}")
    if name == "exact_fit":      # the NaN scale of scaleMinMedian: 100 iterations that change nothing, not acceptable, not registered
        assert np.isnan(s0["scale"]) and not o["ok"]
        assert not g["registered"] and not g["acceptable"] and np.isnan(g["scale0"])
        assert list(g["iters"]) == list(o["iters"]) == [50, 50] and g["count"] == o["count"]
        return
    assert g["registered"] and g["acceptable"] == o["ok"]
    assert np.float32(g["scale0"]) == np.float32(s0["scale"])
    np.testing.assert_allclose(g["sim3"], o["sim3"], rtol=0, atol=1e-7)
    assert abs(g["s22"] - s22) < 1e-6 * s22
    np.testing.assert_allclose(g["Tcw"], Tcw, rtol=0, atol=1e-5)
