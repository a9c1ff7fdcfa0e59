"""The one-wavefront factor loop of the throughput shape (sftb_factor_kernel, sft_batch.h) with MANY problems per wavefront.

Each FACTOR wave is persistent: it pulls problems from a counter, defers the back substitution of its previous problem into the factor steps of
the next one (sft_wave.h: wv_bs_begin / wv_bs_step, the remainder loop behind the factor loop), hands its WvPrev record from problem to problem
and zeroes its LDS once per launch.  A batch of the sizes the other tests use gives nearly every wave ONE problem per launch; here:

- the product library (and the lab library with rounds to the end) on 16 problems per wave, every frame repeated at scattered positions: every
  copy of a frame must give the same bits, whatever problems its wave factored before it, and every distinct healthy frame follows the oracle;
- the FACTOR kernel alone (dsh_lab_sft_factor_check): its x against a long-double residual of the dense system, bit for bit against the
  kernel with one problem per wave, and on the sequences of predecessors that take the rarer paths (remainder loop, failed and skipped problems,
  the wave's last problem), at every band of the TRSM variants (q8) and at node counts where the padding of the last tile differs;
- a workspace that held failed factorisations, reused by the next batch without being cleared.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_sft_gpu import _compare

pytestmark = pytest.mark.gpu


def _regs():
    from defslam_amd import synth
    return (synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)


def _num_cus():
    from defslam_amd import _lib
    return _lib.device_cus(0)


def _view(fr, cols, cols_kept, rows_kept, extra=0):
    """Keep the observations whose facet lies on columns < cols_kept of rows < rows_kept (+ column cols_kept on its first `extra` rows)."""
    keep = [c + cols * r for r in range(rows_kept) for c in range(cols_kept)] + [cols_kept + cols * r for r in range(extra)]
    sel = np.all(np.isin(fr.obs_nodes, keep), axis=1)
    for k in ["obs_nodes", "obs_bary", "obs_uv", "obs_invsig2"]:
        setattr(fr, k, getattr(fr, k)[sel])
    return fr


def _oracle_all(oracle_mod, tc, syn, ids):
    regs = _regs()

    def one(p):
        fr = syn[p]
        return oracle_mod.sft_solve(tc, fr.Tcw, fr.K, fr.n_frame, fr.obs_nodes, fr.obs_bary, fr.obs_uv, fr.obs_invsig2, fr.xyz, *regs, ldlt_mode=1)

    with ThreadPoolExecutor(8) as ex:   # (the C oracle keeps no mutable global state; the calls release the GIL)
        return dict(zip(ids, ex.map(one, ids)))


def _snapshot(frames, inl):
    return [(int(i), f.iters, f.trials, f.status, f.trace.copy(), f.nodes_xyz.copy(), f.pose7.copy(), f.chi2_obs.copy(), f.mvbOutlier.copy())
            for i, f in zip(inl, frames)]


def _same(a, b, what):
    assert a[:4] == b[:4], what
    for u, v in zip(a[4:], b[4:]):
        np.testing.assert_array_equal(u, v, err_msg=str(what))


# ---- 1. the product's rounds with many problems per wave ------------------------------------------------------------------------------------

ROWS, COLS = 9, 14


@pytest.fixture(scope="module")
def wave_pool(oracle_mod):
    """B = 16 x (4 x CUs) problems (16 per FACTOR wave) of the 9 x 14 mesh from a pool of B / 32 distinct frames: partial views (14 .. 11
    columns, 9 or 8 rows) so that dimension and half-bandwidth vary, every 8th frame indefinite (negative information); each frame at 32
    scattered positions.  The oracle's solutions of the healthy frames are computed once."""
    from defslam_amd import synth
    cus = _num_cus()
    B = 16 * 4 * cus
    n_pool = B // 32
    tmpl = synth.make_grid_template(ROWS, COLS)
    syn = []
    for p in range(n_pool):
        fr = synth.make_frame(tmpl, 380 + 10 * (p % 5), 7000 + p)
        fr = _view(fr, COLS, COLS - (p % 4), ROWS - ((p // 4) % 2))
        if p % 8 == 5:
            fr.obs_invsig2 = -50.0 * np.abs(fr.obs_invsig2)
        syn.append(fr)
    bad = {p for p in range(n_pool) if p % 8 == 5}
    rng = np.random.default_rng(20261016)
    order = rng.permutation(B) % n_pool          # position -> pool frame: every frame 32 times, scattered
    shuffled = order[rng.permutation(B)]          # the same multiset in another (fixed) order
    tc = oracle_mod.template_build(tmpl.xyz0, tmpl.facets)
    ref = _oracle_all(oracle_mod, tc, syn, list(range(n_pool)))
    return dict(B=B, tmpl=tmpl, syn=syn, bad=bad, order=order, shuffled=shuffled, ref=ref)


@pytest.fixture(params=["product_default_tail", "lab_rounds_to_the_end"])
def wave_ctx(request, gpu_ctx, lab_ctx):
    if request.param == "product_default_tail":
        yield gpu_ctx
    else:
        lab_ctx.set_option("tail", 0)
        try:
            yield lab_ctx
        finally:
            lab_ctx.set_option("tail", -1)


def test_every_copy_of_a_frame_gives_the_same_bits_with_sixteen_problems_per_wave(wave_ctx, wave_pool):
    """What a wave carries from one problem to the next (the deferred back substitution, WvPrev, its LDS) must not reach the next problem's
    result: with 16 problems per wave every frame is solved 32 times per run behind other predecessors, in two runs of one order and one run of
    a shuffled order -- all 96 copies bit-identical (iterations, trials, status, trace, vertices, pose, chi2 per observation, outliers, inliers).
    Every distinct healthy frame against the oracle; the indefinite ones as in test_rounds_of_phase_kernels_with_failing_factorisations."""
    from defslam_amd import sft
    P = wave_pool
    tmpl, syn, bad, ref = P["tmpl"], P["syn"], P["bad"], P["ref"]
    ctx = wave_ctx
    ctx.template_build(tmpl.xyz0, tmpl.facets)
    runs = []
    for order in (P["order"], P["order"], P["shuffled"]):
        frames = [sft.frame_from_synth(syn[int(q)]) for q in order]
        ctx.batch_upload(frames, *_regs(), 1, 50)
        if not runs:
            first = {int(q): b for b, q in reversed(list(enumerate(order)))}
            for q, b in first.items():
                _, counts = ctx.problem_info(b)
                assert int(counts[7]) == 1 and int(counts[6]) <= 128, (q, b, counts)   # rounds of phase kernels, one-wavefront solver
        ctx.batch_run()
        inl = ctx.batch_download()
        runs.append((order, frames, _snapshot(frames, inl)))
    canon = {}
    for r, (order, frames, snap) in enumerate(runs):
        for b, q in enumerate(order):
            q = int(q)
            if q not in canon:
                canon[q] = (snap[b], frames[b])
            else:
                _same(canon[q][0], snap[b], (r, b, q))
    assert len(canon) == len(syn)
    for q, (s, f) in canon.items():
        r = ref[q]
        if q in bad:
            assert f.status & 1, "a failed factorisation must be reported"
            assert 1 <= f.iters <= 50 and f.trials >= f.iters
            np.testing.assert_allclose(f.trace[0, [0, 1]], r.trace[0, [0, 1]], rtol=1e-8)
            assert f.trace[0, 7] == 0 and r.trace[0, 7] == 0
            assert np.isfinite(f.nodes_xyz).all() and np.isfinite(f.pose7).all()
        else:
            _compare(f, s[0], r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret)
            assert f.trials == r.trials


# ---- 2. the FACTOR kernel alone (lab hook dsh_lab_sft_factor_check) -------------------------------------------------------------------------

# Views of the 8 x 30 mesh (700 matches): (columns kept, extra nodes on the next column, rows kept, frame seed) -> (Dn, kd).  The TRSM of a
# factor step has four variants by q8 = min(3, (128 - kd) / 4) (sft_wave.h: wv_factor); padding of the last tile row depends on Dn mod 32.
W_ROWS, W_COLS, W_M = 8, 30, 700
SEQ = [
    (19, 1, 7, 2917),   # Dn 480 kd 125  q8 0  Dn = 0 mod 32
    (18, 8, 8, 2888),   # Dn 480 kd 122  q8 1  (equal size behind the first)
    (3, 0, 8, 1308),    # Dn  96 kd  26  q8 3  (big -> small: the remainder loop; fewer tile rows than the window)
    (19, 2, 7, 2927),   # Dn 483 kd 128  q8 0  Dn = 3 mod 32  (small -> big)
    (18, 1, 8, 2818),   # Dn 459 kd 119  q8 2
    (4, 3, 7, 1437),    # Dn 126 kd  38  q8 3  Dn = 30 mod 32
    (18, 3, 4, 2834),   # Dn 291 kd 122  q8 1  Dn = 3 mod 32
    (18, 1, 4, 2814),   # Dn 285 kd 119  q8 2
    (3, 2, 7, 1327),    # Dn  99 kd  32  q8 3  Dn = 3 mod 32
    (17, 2, 8, 2728),   # kd 116 (the largest half-bandwidth of q8 3)
    (7, 1, 8, 1718),    # Dn 195 kd  53
    (19, 1, 7, 2917),   # the first frame again
]
# damping patterns over SEQ: None = left out (skipped), "fail" = -2 x max |diag H| (the first pivot is negative), else a multiple of max |diag H|
PATTERNS = {
    "tau_1e-5": [1e-5] * 12,
    "tau_1e-12": [1e-12] * 12,
    "tau_1e+12": [1e12] * 12,
    # failed -> healthy (2 -> 3), failed -> failed (5 -> 6), healthy -> skipped -> healthy (7, 8, 9), failed as the wave's last problem (11)
    "failures": [1e-5, 1e-5, "fail", 1e-5, 1e-5, "fail", "fail", 1e-5, None, 1e-5, 1e-5, "fail"],
    # big -> small behind a skip, small -> big behind a failure, mixed dampings from problem to problem
    "mixed": [1e12, None, 1e-5, "fail", 1e-12, 1e-5, 1e12, None, "fail", 1e-12, 1e-5, 1e-5],
}


@pytest.fixture(scope="module")
def factor_batch(lab_ctx):
    """The batch of SEQ uploaded on the lab context, its dense systems (dsh_lab_sft_system: camera first, then the node unknowns in band
    order) and max |diag H|; the batch has run once afterwards (what the factor hook needs)."""
    from defslam_amd import sft, synth
    tmpl = synth.make_grid_template(W_ROWS, W_COLS)
    lab_ctx.template_build(tmpl.xyz0, tmpl.facets)
    frames = [sft.frame_from_synth(_view(synth.make_frame(tmpl, W_M, pid), W_COLS, ck, rk, extra)) for ck, extra, rk, pid in SEQ]
    lab_ctx.batch_upload(frames, *_regs(), 1, 50)
    dims = []
    for b in range(len(SEQ)):
        _, counts = lab_ctx.problem_info(b)
        dims.append((int(counts[5]) - 6, int(counts[6])))
    lab_ctx.batch_run()
    systems = []
    for b, (Dn, kd) in enumerate(dims):
        H, rhs, _ = lab_ctx.debug_system(b, 6 + Dn)
        systems.append((np.array(H), np.array(rhs)))
    lab_ctx.batch_run()
    maxdiag = np.array([np.abs(np.diag(H)).max() for H, _ in systems])
    return dict(ctx=lab_ctx, dims=dims, systems=systems, maxdiag=maxdiag)


def _refine(A, rhs):
    """float64 solve refined with long-double residuals (three steps)."""
    x = np.linalg.solve(A, rhs).astype(np.longdouble)
    Al, bl = A.astype(np.longdouble), rhs.astype(np.longdouble)
    for _ in range(3):
        r = bl - Al @ x
        x = x + np.linalg.solve(A, r.astype(np.float64)).astype(np.longdouble)
    return x


def test_factor_check_covers_every_trsm_band_and_padding(factor_batch):
    dims = factor_batch["dims"]
    q8 = {min(3, max(0, (128 - kd) // 4)) for _, kd in dims}
    assert all(kd <= 128 for _, kd in dims) and q8 == {0, 1, 2, 3}, dims
    assert 128 in {kd for _, kd in dims}
    assert {0, 3, 30} <= {Dn % 32 for Dn, _ in dims}, dims
    nT = [((Dn + 31) // 32) * 2 for Dn, _ in dims]
    assert any(a > b for a, b in zip(nT, nT[1:])) and any(a < b for a, b in zip(nT, nT[1:])) and any(a == b for a, b in zip(nT, nT[1:]))


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_factor_kernel_solves_every_sequence_of_predecessors_accurately_and_bit_identically(factor_batch, pattern):
    """sftb_factor_kernel on the systems of SEQ: with ONE wave (grid 1: every problem follows the previous one of the list -- deferred back
    substitution, remainder loop, a failed or skipped predecessor), with the product's grid (one problem per wave: the back substitution
    right away) and the lab kernel of one problem per launch (dsh_lab_sft_wave_check, only = 2): the same flags and x bit for bit.  Each
    healthy x against the dense system: normwise backward error of (H + lambda I) x = b, residual accumulated in long double, <= 1e-13;
    forward error against a refined solve within the first-order bound kappa x backward error."""
    ctx, dims, systems, maxdiag = factor_batch["ctx"], factor_batch["dims"], factor_batch["systems"], factor_batch["maxdiag"]
    pat = PATTERNS[pattern]
    B = len(SEQ)
    lam = np.array([(-2.0 if t == "fail" else (1.0 if t is None else t)) * m for t, m in zip(pat, maxdiag)])
    fac = np.array([t is not None for t in pat])
    x1, ok1 = ctx.factor_check(lam, fac, grid=1)
    x0, ok0 = ctx.factor_check(lam, fac, grid=0)
    _, xw, okw, _ = ctx.wave_check(1.0, 1, only=2)
    want = np.array([-1 if t is None else (0 if t == "fail" else 1) for t in pat], np.int32)
    np.testing.assert_array_equal(ok1, want)
    np.testing.assert_array_equal(ok0, want)
    np.testing.assert_array_equal(okw[fac, 1], want[fac])
    worst = []
    for b in range(B):
        if want[b] != 1:
            continue
        np.testing.assert_array_equal(x1[b], x0[b], err_msg=f"problem {b}: deferred against immediate back substitution")
        np.testing.assert_array_equal(x1[b], xw[b], err_msg=f"problem {b}: persistent FACTOR kernel against one problem per launch")
        Dn, _ = dims[b]
        Dnp = ((Dn + 31) // 32) * 32
        x = np.concatenate([x1[b][Dnp:Dnp + 6], x1[b][:Dn]])
        H, rhs = systems[b]
        A = H + lam[b] * np.eye(6 + Dn)
        assert np.isfinite(x).all()
        r = A.astype(np.longdouble) @ x.astype(np.longdouble) - rhs.astype(np.longdouble)
        eta = float(np.abs(r).max() / (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(rhs).max()))
        xt = _refine(A, rhs)
        fe = float(np.abs(x.astype(np.longdouble) - xt).max() / np.abs(xt).max())
        kappa = float(np.linalg.cond(A, np.inf))
        worst.append((b, eta, fe, kappa))
        assert eta <= 1e-13, (b, eta)
        assert kappa * eta < 0.5 and fe <= 2.0 * kappa * eta / (1.0 - kappa * eta) + 4.0 * 2.0 ** -53, (b, fe, kappa, eta)
    print(f"\n[factor_check {pattern}] max backward error {max(w[1] for w in worst):.2e}, max forward error {max(w[2] for w in worst):.2e}, "
          f"condition numbers {min(w[3] for w in worst):.1e} .. {max(w[3] for w in worst):.1e}")


# ---- 3. a workspace that held failed factorisations ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["throughput", "latency"])
def test_workspace_reused_after_failed_factorisations_gives_the_bits_of_a_fresh_one(shape):
    """A failed Cholesky leaves non-finite numbers in its tiles of L (every pivot behind a non-positive one is NaN).  The workspace is
    cleared only when it is allocated; the next batch that fits it starts on what the failed one left (in the throughput shape this is
    checked through the lab dump of L before the healthy batch runs).  A healthy batch of smaller partial views after a batch in which
    every second problem is indefinite must give the bits of the same batch in a fresh context -- in the throughput shape (rounds of phase
    kernels) and in the latency mode."""
    from defslam_amd import sft, synth
    cus = _num_cus()
    B = 4 * cus if shape == "throughput" else 8
    tmpl = synth.make_grid_template(ROWS, COLS)
    poisoned, healthy = [], []
    for p in range(B):
        fr = synth.make_frame(tmpl, 420, 9000 + p)
        if p % 2 == 0:
            fr.obs_invsig2 = -50.0 * np.abs(fr.obs_invsig2)
        poisoned.append(fr)
        h = synth.make_frame(tmpl, 420, 9000 + p)
        healthy.append(_view(h, COLS, COLS - 1 - (p % 3), ROWS - (p % 2)))

    def run(ctx, batch):
        frames = [sft.frame_from_synth(fr) for fr in batch]
        ctx.batch_upload(frames, *_regs(), 1, 50)
        assert (int(ctx.problem_info(0)[1][7]) == 1) == (shape == "throughput")
        ctx.batch_run()
        return frames, _snapshot(frames, ctx.batch_download())

    def nonfinite_L(ctx, ids):   # problems among `ids` whose tiles of L (lab dump 0: nT block columns of 9 tiles) hold a non-finite number
        out = []
        for b in ids:
            nT = 2 * ((int(ctx.problem_info(b)[1][5]) - 6 + 31) // 32)
            if not np.isfinite(ctx.dump(b, 0, nT * 9 * 256)).all():
                out.append(b)
        return out

    used = sft.Context(0, lab=True)
    try:
        used.template_build(tmpl.xyz0, tmpl.facets)
        frames_p, _ = run(used, poisoned)
        assert all(f.status & 1 for f in frames_p[0::2]), "the indefinite problems must fail"
        left = nonfinite_L(used, range(0, min(B, 64), 2))
        frames = [sft.frame_from_synth(fr) for fr in healthy]
        used.batch_upload(frames, *_regs(), 1, 50)
        inherited = nonfinite_L(used, range(min(B, 64)))
        if shape == "throughput":   # the premise, where the one-wavefront solver stores L (measured on an MI355X: 13 of 32 and 13 of 64)
            assert left and inherited, "the healthy batch must start on the non-finite tiles a failed factorisation left behind"
        print(f"\n[{shape}] problems whose L held non-finite numbers after the failing batch: {len(left)} of {len(range(0, min(B, 64), 2))} sampled; "
              f"after the upload of the healthy batch into the same workspace: {len(inherited)} of {min(B, 64)}")
        _, after = run(used, healthy)
    finally:
        used.close()
    fresh = sft.Context(0, lab=True)
    try:
        fresh.template_build(tmpl.xyz0, tmpl.facets)
        frames_h, clean = run(fresh, healthy)
    finally:
        fresh.close()
    assert all(f.status == 0 for f in frames_h)
    for b in range(B):
        _same(clean[b], after[b], b)
