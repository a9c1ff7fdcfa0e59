"""The packed block column of L of the one-wavefront solver (sft_wave.h: "the packed block column of L").

The factorisation stores, and both back substitutions read, only the 16-byte granules of a block column that hold a structurally non-zero
element: the lower triangle of W, the corner of the d = 8 tile that lies inside the band (rows - columns <= kd), and no tile of a tile row
behind the matrix.  What is skipped is never written, so the memory there may hold anything; the readers supply the zeros -- the deferred back
substitution from a landing buffer in LDS that the previous problem of the wave has used, the immediate one in registers.

Which granules are skipped depends on the half-bandwidth alone, in seven classes: no d = 8 tile at all (kd <= 112), its smallest corner
(q8 = 3: kd 113, 116), q8 = 2 (119), q8 = 1 (122), q8 = 0 (125) and the full lower triangle (128).  Views of ONE 3 x 23 template give all of
them at 10 - 12 tile rows, with a dimension that is no multiple of 16 (the last block column is partial, tile rows lie behind the matrix), so
a wave meets them mixed in one launch.

- on the CPU, with the oracle alone: every case has the size and band it is here for, converges, and its two elimination orders stay inside
  the bounds of tests/test_sft_gpu.py::_compare (no accept / reject decision at rounding level);
- the FACTOR kernel alone (dsh_lab_sft_factor_check): every class with one problem per wave (immediate back substitution) and as the middle
  one of three problems on one wave (deferred; the landing buffer comes from another class and goes to a third), bit for bit against each other
  and against the kernel of one problem per launch, x against the dense system; failed factorisations in front of healthy ones;
- the batch (product library and lab rounds to the end), three problems per wave: every copy the same bits, every case against the oracle.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from test_factor_waves_gpu import _refine, _regs, _same, _snapshot, _view
from test_sft_gpu import _compare

ROWS, COLS, M = 3, 23, 200
# (columns kept, extra nodes on the next column, frame seed, Dn, kd) of the views of the 3 x 23 template
CASES = [
    (17, 0, 5100, 162, 110),   # no d = 8 tile
    (17, 1, 5101, 165, 113),   # q8 3, the smallest corner
    (17, 2, 5102, 168, 116),   # q8 3
    (18, 1, 5103, 174, 119),   # q8 2
    (19, 0, 5104, 180, 122),   # q8 1 (the band of the benched configuration)
    (19, 1, 5105, 183, 125),   # q8 0
    (19, 2, 5106, 186, 128),   # the whole lower triangle
]
# the order of the problems of the factor batch: every class behind a different one (128 -> 110: the granules of the widest corner are stale
# in the landing buffer when the band without a d = 8 tile is solved)
SEQ = [6, 0, 4, 1, 5, 2, 3, 6, 0]
MIDDLE = {SEQ[p]: p for p in range(1, len(SEQ) - 1)}   # class -> a position with a predecessor and a successor


def _frames():
    from defslam_amd import synth
    tmpl = synth.make_grid_template(ROWS, COLS)
    return tmpl, [_view(synth.make_frame(tmpl, M, seed), COLS, ck, ROWS, extra) for ck, extra, seed, _, _ in CASES]


@pytest.fixture(scope="module")
def packed_cases(oracle_mod):
    """The seven views and the oracle's solutions of them (computed once, never modified)."""
    tmpl, syn = _frames()
    tc = oracle_mod.template_build(tmpl.xyz0, tmpl.facets)
    ref = [oracle_mod.sft_solve(tc, fr.Tcw, fr.K, fr.n_frame, fr.obs_nodes, fr.obs_bary, fr.obs_uv, fr.obs_invsig2, fr.xyz, *_regs(), ldlt_mode=1)
           for fr in syn]
    return dict(tmpl=tmpl, syn=syn, tc=tc, ref=ref)


def test_cases_cover_the_band_classes_and_are_well_posed_for_the_oracle(host_ctx, oracle_mod, packed_cases):
    """No GPU: sizes and half-bandwidths as packed by the host side of the library; the oracle converges on every case without an iteration of
    eight or more dampings, and its other elimination order gives the same trajectory and a state inside _compare's bounds."""
    from defslam_amd import sft
    tmpl, syn, tc, ref = packed_cases["tmpl"], packed_cases["syn"], packed_cases["tc"], packed_cases["ref"]
    assert MIDDLE.keys() == set(range(len(CASES)))
    host_ctx.template_build(tmpl.xyz0, tmpl.facets)
    host_ctx.batch_upload([sft.frame_from_synth(fr) for fr in syn], *_regs(), 1, 50)
    q8 = set()
    for b, (_, _, _, Dn, kd) in enumerate(CASES):
        counts = host_ctx.problem_info(b)[1]
        assert (int(counts[5]) - 6, int(counts[6])) == (Dn, kd), (b, counts)
        assert Dn % 16 != 0 and 10 <= 2 * ((Dn + 31) // 32) <= 12
        if kd > 112:
            q8.add(min(3, (128 - kd) // 4))
    kds = [kd for *_, kd in CASES]
    assert min(kds) <= 112 and max(kds) == 128 and q8 == {0, 1, 2, 3}
    for fr, r in zip(syn, ref):
        assert 2 <= r.iters < 50 and (r.trace[:, 2] < 8).all(), r.trace
        o = oracle_mod.sft_solve(tc, fr.Tcw, fr.K, fr.n_frame, fr.obs_nodes, fr.obs_bary, fr.obs_uv, fr.obs_invsig2, fr.xyz, *_regs(), ldlt_mode=0)
        like = SimpleNamespace(status=0, iters=o.iters, trace=o.trace, nodes_xyz=o.xyz, pose7=o.pose7, mvbOutlier=np.asarray(o.outlier, bool),
                               rep_error_f64=o.rep_error)
        _compare(like, o.ret, r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret)
        assert o.trials == r.trials


# ---- the FACTOR kernel alone ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def packed_batch(lab_ctx, packed_cases):
    """The batch of SEQ on the lab context, its dense systems and max |diag H| (as the factor_batch of test_factor_waves_gpu.py)."""
    from defslam_amd import sft
    tmpl, syn = packed_cases["tmpl"], packed_cases["syn"]
    lab_ctx.template_build(tmpl.xyz0, tmpl.facets)
    lab_ctx.batch_upload([sft.frame_from_synth(syn[i]) for i in SEQ], *_regs(), 1, 50)
    for b, i in enumerate(SEQ):
        counts = lab_ctx.problem_info(b)[1]
        assert (int(counts[5]) - 6, int(counts[6])) == CASES[i][3:], (b, counts)
    systems = []
    for i in SEQ:
        H, rhs, _ = lab_ctx.debug_system(len(systems), 6 + CASES[i][3])
        systems.append((np.array(H), np.array(rhs)))
    lab_ctx.batch_run()   # (what the factor hook needs)
    maxdiag = np.array([np.abs(np.diag(H)).max() for H, _ in systems])
    return dict(ctx=lab_ctx, systems=systems, maxdiag=maxdiag)


def _check_x(xb, Dn, H, rhs, lam):
    """x of one problem against the dense system: the bounds of test_factor_waves_gpu.py (normwise backward error of (H + lambda I) x = b with a
    long-double residual <= 1e-13, forward error within the first-order bound of it)."""
    Dnp = ((Dn + 31) // 32) * 32
    x = np.concatenate([xb[Dnp:Dnp + 6], xb[:Dn]])
    A = H + lam * np.eye(6 + Dn)
    assert np.isfinite(x).all()
    r = A.astype(np.longdouble) @ x.astype(np.longdouble) - rhs.astype(np.longdouble)
    eta = float(np.abs(r).max() / (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(rhs).max()))
    xt = _refine(A, rhs)
    fe = float(np.abs(x.astype(np.longdouble) - xt).max() / np.abs(xt).max())
    kappa = float(np.linalg.cond(A, np.inf))
    print(f"  Dn {Dn}: backward error {eta:.2e}, forward error {fe:.2e}, condition {kappa:.1e}")
    assert eta <= 1e-13, eta
    assert kappa * eta < 0.5 and fe <= 2.0 * kappa * eta / (1.0 - kappa * eta) + 4.0 * 2.0 ** -53, (fe, kappa, eta)


@pytest.mark.gpu
@pytest.mark.parametrize("tau", [1e-5, 1e12])
@pytest.mark.parametrize("cls", range(len(CASES)), ids=[f"kd{c[4]}" for c in CASES])
def test_every_band_class_alone_on_a_wave_and_between_two_other_classes(packed_batch, cls, tau):
    """Class `cls` with its neighbours of SEQ: three problems on ONE wave (the deferred back substitution of each rides in the next one's factor
    steps, the last one is solved right away) against one problem per wave and one problem per launch -- the same bits; x of all three against
    the dense system."""
    ctx, systems, maxdiag = packed_batch["ctx"], packed_batch["systems"], packed_batch["maxdiag"]
    p = MIDDLE[cls]
    fac = np.zeros(len(SEQ), bool)
    fac[p - 1:p + 2] = True
    lam = tau * maxdiag
    x1, ok1 = ctx.factor_check(lam, fac, grid=1)
    x0, ok0 = ctx.factor_check(lam, fac, grid=0)
    _, xw, okw, _ = ctx.wave_check(1.0, 1, only=2)
    want = np.where(fac, 1, -1).astype(np.int32)
    np.testing.assert_array_equal(ok1, want)
    np.testing.assert_array_equal(ok0, want)
    np.testing.assert_array_equal(okw[fac, 1], want[fac])
    print()
    for b in range(p - 1, p + 2):
        np.testing.assert_array_equal(x1[b], x0[b], err_msg=f"problem {b}: deferred against immediate back substitution")
        np.testing.assert_array_equal(x1[b], xw[b], err_msg=f"problem {b}: persistent FACTOR kernel against one problem per launch")
        _check_x(x1[b], CASES[SEQ[b]][3], *systems[b], lam[b])


@pytest.mark.gpu
def test_failed_factorisations_in_front_of_healthy_ones_of_every_class(packed_batch):
    """All of SEQ on one wave; four problems are indefinite (damping -2 max |diag H|: every pivot behind the first is NaN, and so is what the wave
    stores of their L).  The healthy ones behind them give the bits of the launch without failures and of one problem per wave."""
    ctx, systems, maxdiag = packed_batch["ctx"], packed_batch["systems"], packed_batch["maxdiag"]
    fail = np.array([1, 0, 0, 1, 0, 1, 1, 0, 0], bool)
    lam_ok = 1e-5 * maxdiag
    x_all, ok_all = ctx.factor_check(lam_ok, None, grid=1)
    np.testing.assert_array_equal(ok_all, np.ones(len(SEQ), np.int32))
    lam = np.where(fail, -2.0 * maxdiag, lam_ok)
    x1, ok1 = ctx.factor_check(lam, None, grid=1)
    x0, ok0 = ctx.factor_check(lam, None, grid=0)
    np.testing.assert_array_equal(ok1, np.where(fail, 0, 1))
    np.testing.assert_array_equal(ok0, np.where(fail, 0, 1))
    print()
    for b in np.flatnonzero(~fail):
        np.testing.assert_array_equal(x1[b], x_all[b], err_msg=f"problem {b}: behind failed factorisations against a launch without them")
        np.testing.assert_array_equal(x1[b], x0[b], err_msg=f"problem {b}: deferred against immediate back substitution")
        _check_x(x1[b], CASES[SEQ[b]][3], *systems[b], lam[b])


# ---- the batch: rounds of phase kernels with three problems per wave ------------------------------------------------------------------------------

@pytest.fixture(params=["product_default_tail", "lab_rounds_to_the_end"])
def batch_ctx(request, gpu_ctx, lab_ctx):
    if request.param == "product_default_tail":
        yield gpu_ctx
    else:
        lab_ctx.set_option("tail", 0)
        try:
            yield lab_ctx
        finally:
            lab_ctx.set_option("tail", -1)


@pytest.mark.gpu
def test_batch_of_mixed_band_classes_follows_the_oracle_with_three_problems_per_wave(batch_ctx, packed_cases):
    """3 x (4 x CUs) problems: the seven classes and an indefinite copy of the kd = 122 case, interleaved, so that a wave factors problems of
    different classes one behind the other (and behind failed ones) in every round.  Every copy of a case gives the same bits; every healthy
    case follows the oracle (LM trajectory, vertices, pose, outliers, inliers: _compare)."""
    from defslam_amd import _lib, sft, synth
    tmpl, syn, ref = packed_cases["tmpl"], packed_cases["syn"], packed_cases["ref"]
    bad = synth.make_frame(tmpl, M, CASES[4][2])
    bad = _view(bad, COLS, CASES[4][0], ROWS, CASES[4][1])
    bad.obs_invsig2 = -50.0 * np.abs(bad.obs_invsig2)
    pool = list(syn) + [bad]
    B = 3 * 4 * _lib.device_cus(0)
    order = np.random.default_rng(20261020).permutation(B) % len(pool)
    frames = [sft.frame_from_synth(pool[int(q)]) for q in order]
    ctx = batch_ctx
    ctx.template_build(tmpl.xyz0, tmpl.facets)
    ctx.batch_upload(frames, *_regs(), 1, 50)
    assert int(ctx.problem_info(0)[1][7]) == 1, "the batch must run as rounds of phase kernels with the one-wavefront solver"
    ctx.batch_run()
    snap = _snapshot(frames, ctx.batch_download())
    canon = {}
    for b, q in enumerate(order):
        q = int(q)
        if q not in canon:
            canon[q] = b
        else:
            _same(snap[canon[q]], snap[b], (b, q))
    assert len(canon) == len(pool)
    for q, b in canon.items():
        f = frames[b]
        if q == len(syn):
            assert f.status & 1, "a failed factorisation must be reported"
            assert np.isfinite(f.nodes_xyz).all() and np.isfinite(f.pose7).all()
        else:
            r = ref[q]
            _compare(f, snap[b][0], r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret)
            assert f.trials == r.trials
