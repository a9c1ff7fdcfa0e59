"""CPU tests of the rigid pose-only optimisation on the map point store: the restatement (tests/pose_only_ref.py) against central
differences, a known pose and hand cases that pin its control flow; the validity of the cases the GPU tests use and the reassociation
noise that sets their tolerance; and the ABI of dsh_track_pose_only / dsh_track_pose_only_batch without a GPU (symbols, struct size,
every host-only refusal and its order, a detached store)."""
import ctypes as C

import numpy as np
import pytest

import pose_only_ref as R

OK, ARG, NODEV = 0, 1, 4
NEW_ENTRIES = ["dsh_track_pose_only", "dsh_track_pose_only_batch"]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------

def test_se3_helpers_agree_with_the_sft_oracle():
    from oracle import sft_oracle_np as O
    rng = np.random.default_rng(0)
    for _ in range(20):
        d = np.concatenate([rng.uniform(-1, 1, 3) * rng.choice([1e-7, 0.3, 2.5]), rng.uniform(-1, 1, 3)])
        Rm, t = O.se3_exp(d)
        p = R.exp_times([float(v) for v in d], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
        assert np.abs(np.array(R.quat_to_R(p[3:])).reshape(3, 3) - Rm).max() < 1e-14
        assert np.abs(np.array(p[:3]) - t).max() < 1e-14
        T = R.pose_to_f32_matrix(p)
        start = R.pose_from_f32_matrix(T)
        assert np.abs(np.array(R.quat_to_R(start[3:])).reshape(3, 3) - O.rotation_from_f32_pose(T[:3, :3])).max() < 1e-14


def test_pivoted_ldlt_solves_and_reports_the_sign():
    rng = np.random.default_rng(1)
    for n in (6, 7):
        A = rng.normal(size=(n, n))
        A = A @ A.T + np.diag(rng.uniform(0, 50, n))
        b = rng.normal(size=n)
        F = [float(v) for v in A.T.reshape(-1)]
        perm, ok = R.ldlt(F, n)
        assert ok and perm != list(range(n))                       # the pivoting moved something
        assert np.abs(np.array(R.ldlt_solve(F, perm, [float(v) for v in b], n)) - np.linalg.solve(A, b)).max() < 1e-12
        F = [float(v) for v in (A - 200 * np.eye(n)).T.reshape(-1)]
        assert not R.ldlt(F, n)[1]


def test_jacobian_against_central_differences():
    rng = np.random.default_rng(2)
    pose = R.true_pose(rng)
    K = [R.FX, R.FY, R.CX, R.CY]
    X = np.stack([rng.uniform(-2, 2, 6), rng.uniform(-1.5, 1.5, 6), rng.uniform(3, 8, 6)], 1)
    uv, w = rng.uniform(0, 600, (6, 2)), np.ones(6)
    _, _, _, px, py, pz = R.edge_error(pose, K, X, uv, w)
    A0, A1 = R.edge_jacobian(K, px, py, pz)
    h = 1e-6
    for d in range(6):
        dp, dm = [0.0] * 6, [0.0] * 6
        dp[d], dm[d] = h, -h
        ep, em = R.edge_error(R.exp_times(dp, pose), K, X, uv, w), R.edge_error(R.exp_times(dm, pose), K, X, uv, w)
        assert np.abs((ep[0] - em[0]) / (2 * h) - A0[d]).max() < 1e-5 * max(1.0, np.abs(A0[d]).max())
        assert np.abs((ep[1] - em[1]) / (2 * h) - A1[d]).max() < 1e-5 * max(1.0, np.abs(A1[d]).max())


def test_recovers_a_known_pose_from_noise_free_matches():
    """To 10 x the float32 spacing of the pose entries: the result passes through float32 (Tcw_out), and so did the key points."""
    model, fr, pose = R.make_case(seed=21, N=120, held=80, noise=0.0, perturb=0.05)
    # noise-free key points in double would be exact; in float32 they carry 3e-5 px, which moves the pose by far less than a float32 ulp
    res = R.solve(model, fr)
    want = R.pose_to_f32_matrix(pose)
    assert res.rounds[-1].bad == 0 and res.n_good == 80
    assert (np.abs(res.Tcw - want) <= 10 * np.spacing(np.abs(want).astype(np.float32))).all(), np.abs(res.Tcw - want).max()


@pytest.mark.parametrize("held,rounds", [(0, 0), (2, 0), (3, 1), (9, 1), (10, 4)])
def test_number_of_rounds_follows_the_number_of_edges(held, rounds):
    model, fr, _ = R.make_case(**R.GPU_CASES[f"held{held}"])
    entry = np.ones(len(fr.frame_points), bool)
    res = R.solve(model, fr, outlier=entry)
    assert res.n_initial == held and len(res.rounds) == rounds
    holes = fr.frame_points < 0
    assert res.outlier[holes].all()                                   # entries without a point are not written
    if rounds == 0:
        assert res.n_good == 0 and not res.outlier[~holes].any()      # cleared, then the early return
        assert np.array_equal(res.Tcw, fr.Tcw)
    else:
        assert res.n_good == held - res.rounds[-1].bad


def test_a_gross_outlier_of_round_0_is_an_inlier_again_later():
    model, fr, _ = R.make_case(**R.GPU_CASES["outlier_returns"])
    res = R.solve(model, fr)
    back = res.rounds[0].flags & ~res.rounds[-1].flags
    assert back.sum() >= 1 and len(res.rounds) == 4
    assert res.rounds[0].stop == "iters" and res.rounds[0].iters == 10      # round 0 runs out of iterations: its estimate is still poor
    assert res.rounds[-1].bad == 15 == int(round(0.3 * 50))                  # exactly the displaced key points stay out


def test_a_start_at_the_optimum_rejects_trials_and_stops_on_nbad():
    model, fr, _ = R.make_case(**R.GPU_CASES["start_at_optimum"])
    res = R.solve(model, fr)
    for r in res.rounds:
        assert r.stop in ("rho", "qmax", "nbad"), r.stop
        assert any(not a for it in r.accepted for a in it)                   # a rejected trial
        assert r.iters < 10 and r.bad == 0
    assert np.abs(res.Tcw - fr.Tcw).max() <= 2 * np.spacing(np.float32(8.0))


def test_a_round_without_a_level_0_edge_keeps_the_input_pose():
    """Every edge flagged after round 0: initializeOptimization(0) leaves no active vertex, optimize returns, classification proceeds."""
    model, fr, _ = R.make_case(**R.GPU_CASES["all_flagged"])                 # key points 60 px off in every direction: no pose fits
    res = R.solve(model, fr)
    assert len(res.rounds) == 4 and res.rounds[0].bad == 12
    assert [r.stop for r in res.rounds[1:]] == ["empty"] * 3 and res.rounds[1].iters == 0 and res.rounds[1].chi2 == 0.0
    assert np.array_equal(res.Tcw, R.pose_to_f32_matrix(R.pose_from_f32_matrix(fr.Tcw)))


STALE_CASE = dict(seed=20026, N=80, held=50, outlier_share=0.1, perturb=0.05, noise=1.3)


def test_an_inlier_is_classified_by_the_error_of_a_rejected_last_trial():
    """The stale-error rule of Optimizer.cc:376-403 (the quirk of DefOptimizer.cc:515-537): STALE_CASE has rounds whose last trial is
    rejected and popped, and the inlier edges then hold errors that differ, bit for bit, from their errors at the estimate; the
    classification compares the held ones.

    Over 300 seeds of this shape, 80 rounds ended that way; in 51 of them the held and the fresh chi2 of every edge were equal bit
    for bit, and the largest difference was 5.0e-7 (STALE_CASE, printed below).  The case in which the difference changes a flag is
    the next test; here the rule is also pinned on classify() with the held and the fresh chi2 on either side of the boundary."""
    model, fr, _ = R.make_case(**STALE_CASE)
    res = R.solve(model, fr)
    seen, worst = 0, 0.0
    for r in res.rounds:
        if r.accepted and not r.accepted[-1][-1]:
            differ = r.chi_held != r.chi_fresh                         # equal by construction where the edge was at level 1
            worst = max(worst, float(np.abs(r.chi_held - r.chi_fresh).max()))
            seen += int(differ.any())
            assert r.stop in ("qmax", "rho")
    print(f"largest |chi2 held - chi2 fresh| after a rejected last trial: {worst:.3e}")
    assert seen >= 1 and 0.0 < worst < 1e-5
    # the rule itself: an inlier is judged by what it holds, an outlier by the fresh error
    lo, hi = float(np.float32(5.991)), float(np.nextafter(np.float32(5.991), np.float32(6))) + 1e-9
    held, fresh = np.array([hi, lo, hi, lo]), np.array([lo, hi, lo, hi])
    assert R.classify(np.array([False, False, True, True]), held, fresh).tolist() == [True, False, False, True]


def stale_flip_case():
    """A frame in which the stale error of a rejected last trial decides a flag, built rather than found: a rejected last trial ends a
    round only at the rounding floor of the chi2, where it moves an edge's chi2 by 1e-9 or so, so a flag changes only when a chi2 lies
    that close to the float32 rounding boundary above 5.991f, and no seed search meets that.  One held key point of a generated frame
    gets a pyramid level of its own with the information 1e-4 (so that moving it does not move the pose) and sits 245 px from its
    projection, on the circle chi2 = 5.991; among the float32 positions within 1500 ulp the one was taken whose chi2 at the round's
    last trial and at its estimate lie on either side of the boundary.  Its coordinates are the bit patterns below."""
    model, fr, _ = R.make_case(seed=270387, N=80, held=50, outlier_share=0.1, perturb=0.05, noise=1.3)
    j = 5                                                             # the edge: the sixth held key point
    k = int(np.nonzero(fr.frame_points >= 0)[0][j])
    fr.inv_level_sigma2 = np.append(fr.inv_level_sigma2, np.float32(1e-4)).astype(np.float32)
    fr.octave = fr.octave.copy()
    fr.octave[k] = R.LEVELS
    fr.kp = fr.kp.copy()
    fr.kp[k] = np.array([1142478998, 1137283610], np.uint32).view(np.float32)
    return model, fr, j, k


def test_the_stale_error_of_a_rejected_last_trial_changes_a_flag():
    """Rounds 1 and 2 of stale_flip_case() end on rho == 0 with their only trial rejected and popped.  The edge holds the error of that
    trial, chi2 = 5.99100041180, which rounds to 5.991f: inlier.  Its error at the estimate, 5.99100041569, rounds to the next
    float32: a classification by the fresh error would flag it.  The restatement follows the held error, as Optimizer.cc:382-389 does.
    Sequential order only: with the device's summation order the rounds take another, equally valid, path at the rounding floor and
    the coincidence is gone, so the GPU tests cannot use this case."""
    model, fr, j, k = stale_flip_case()
    res = R.solve(model, fr, "sequential")
    hit = [i for i, r in enumerate(res.rounds) if r.stale[k]]
    assert hit == [1, 2]
    for i in hit:
        r = res.rounds[i]
        assert r.stop == "rho" and r.accepted[-1] == [False] and r.trial != r.est          # the last trial: evaluated, rejected, popped
        assert not res.rounds[i - 1].flags[k]                                              # an inlier on entry: it keeps what it holds
        held, fresh = np.float32(r.chi_held[j]), np.float32(r.chi_fresh[j])
        print(f"round {i}: held chi2 {r.chi_held[j]!r} -> {held!r}, fresh chi2 {r.chi_fresh[j]!r} -> {fresh!r}")
        assert held == R.CHI2_TH and fresh > R.CHI2_TH and r.chi_held[j] != r.chi_fresh[j]
        assert not r.flags[k]                                                              # the flag is the stale error's
        assert r.stale.sum() == 1
    # and the flag is live: the edge takes part in the next round because of it
    assert not res.rounds[2].flags[k] and res.rounds[3].iters >= 1


# ---- the cases of the GPU tests ------------------------------------------------------------------------------------------------------------

def test_gpu_cases_are_valid_and_their_reassociation_noise():
    """For every case the GPU tests use, the "sequential" and the "device" restatement agree on every decision -- flags per round,
    accept / reject per trial, iteration counts -- so none is left out; the largest pose difference between the two is the
    reassociation noise of the reference itself, and 16 x that number is the GPU tests' pose tolerance."""
    worst, worst_chi = 0.0, 0.0
    for name, kw in R.GPU_CASES.items():
        model, fr, _ = R.make_case(**kw)
        a, b = R.solve(model, fr, "sequential"), R.solve(model, fr, "device")
        assert R.decisions(a) == R.decisions(b), name
        assert np.array_equal(a.outlier, b.outlier) and (a.n_initial, a.n_bad, a.n_good) == (b.n_initial, b.n_bad, b.n_good), name
        assert np.abs(a.Tcw.view(np.int32) - b.Tcw.view(np.int32)).max() <= 1, name
        worst = max(worst, float(np.abs(a.pose - b.pose).max()))
        for ra, rb in zip(a.rounds, b.rounds):
            worst_chi = max(worst_chi, abs(ra.chi2 - rb.chi2) / max(ra.chi2, 1.0))
        # what every case carries: holes, at least three octaves, bad points that take part, one id at two key points
        held = fr.frame_points[fr.frame_points >= 0]
        if len(held) >= 4:
            assert (fr.frame_points < 0).any() and len(set(fr.octave[fr.frame_points >= 0].tolist())) >= 3, name
            assert len(held) - len(set(held.tolist())) == 1, name
        if len(held) >= 60:
            assert any(model.points[int(p)].bad for p in held), name
    print(f"largest |pose_sequential - pose_device| = {worst:.3e}, relative chi2 difference {worst_chi:.3e}")
    assert worst <= R.MEASURED_ORDER_NOISE and R.MEASURED_ORDER_NOISE <= 2 * worst, (worst, R.MEASURED_ORDER_NOISE)
    assert R.POSE_TOL == 16 * R.MEASURED_ORDER_NOISE
    assert worst_chi <= R.MEASURED_CHI2_NOISE and R.CHI2_RTOL == 16 * R.MEASURED_CHI2_NOISE


def test_the_20_percent_case_reclassifies_in_every_round():
    model, fr, _ = R.make_case(**R.GPU_CASES["outliers20"])
    res = R.solve(model, fr, "device")
    assert len(res.rounds) == 4 and all(r.bad >= 60 and r.iters >= 1 for r in res.rounds)


# ---- the ABI without a GPU ---------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_bound_declared_and_wrapped():
    import os
    from defslam_amd import _lib, localmap
    L = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "defslam_hip.h")).read()
    for n in NEW_ENTRIES:
        assert n in _lib.EXPORTED_SYMBOLS and getattr(L, n).argtypes is not None, n
        assert f"int {n}(dsh_mpdb* db" in header, n
    # the C layout on an LP64 target: pointers and doubles at multiples of 8
    assert "} dsh_pose_only_problem;" in header and C.sizeof(_lib.PoseOnlyProblemC) == 296
    assert _lib.PoseOnlyProblemC.pose.offset == 144 and _lib.PoseOnlyProblemC.chi2.offset == 264 and _lib.PoseOnlyProblemC.Tcw_out.offset == 80
    for m in ("pose_only", "pose_only_batch"):
        assert callable(getattr(localmap.MapPointStore, m))
    assert list(localmap.PoseOnly.__dataclass_fields__) == ["outlier", "Tcw", "pose", "n_initial", "n_bad", "n_good", "rounds", "iters", "trials",
                                                            "bad", "chi2"]


def _problem(keep, **kw):
    from defslam_amd import _lib
    a = dict(T=np.eye(4, dtype=np.float32), kp=np.zeros((4, 2), np.float32), oct=np.zeros(4, np.int32), sig=np.ones(8, np.float32),
             fp=np.full(4, -1, np.int32), out=np.ones(4, np.uint8))
    keep.append(a)
    p = _lib.PoseOnlyProblemC()
    ptr = lambda x, t: x.ctypes.data_as(C.POINTER(t))
    p.Tcw, p.kp, p.octave, p.inv_level_sigma2 = ptr(a["T"], C.c_float), ptr(a["kp"], C.c_float), ptr(a["oct"], C.c_int32), ptr(a["sig"], C.c_float)
    p.frame_points, p.outlier = ptr(a["fp"], C.c_int32), ptr(a["out"], C.c_uint8)
    p.K = (C.c_float * 4)(500, 500, 320, 240)
    p.N, p.levels = 4, 8
    p.n_initial = -7                                                  # a refusal writes nothing
    for k, v in kw.items():
        if k == "fp":
            a["fp"][:] = v
        elif k == "oct":
            a["oct"][:] = v
        else:
            setattr(p, k, v)
    keep.append(p)
    return p


def _rows(keep):
    """(name, arguments after the store handle, expected status, a word of the message, the problem) for an EMPTY store on a host-only
    context."""
    from defslam_amd import _lib
    one, batch = NEW_ENTRIES
    rows = []

    def both(want, word, **kw):
        p = _problem(keep, **kw)
        rows.append((one, (C.byref(p),), want, word, p))
        arr = (_lib.PoseOnlyProblemC * 2)()
        keep.append(arr)
        q0, q1 = _problem(keep), _problem(keep, **kw)
        C.memmove(C.byref(arr, 0), C.byref(q0), C.sizeof(q0))
        C.memmove(C.byref(arr, C.sizeof(q0)), C.byref(q1), C.sizeof(q1))
        rows.append((batch, (2, arr), want, word if want == NODEV else "problem 1: ", arr[1]))

    both(NODEV, "host-only")
    both(NODEV, "host-only", N=0, kp=None, octave=None, frame_points=None, outlier=None)
    both(NODEV, "host-only", oct=99)                                  # an octave is read only where a point is held
    both(ARG, "Tcw is NULL", Tcw=None)
    both(ARG, "N outside", N=-1)
    both(ARG, "N outside", N=8193)
    both(ARG, "levels outside", levels=0)
    both(ARG, "levels outside", levels=33)
    both(ARG, "inv_level_sigma2 is NULL", inv_level_sigma2=None)
    both(ARG, "NULL", kp=None)
    both(ARG, "NULL", octave=None)
    both(ARG, "NULL", frame_points=None)
    both(ARG, "NULL", outlier=None)
    both(ARG, "frame_points[0]", fp=0)                                # id 0 outside the empty store
    both(ARG, "frame_points[0]", fp=-2)
    rows.append((one, (None,), ARG, "p is NULL", None))
    rows.append((batch, (-1, None), ARG, "B outside", None))
    rows.append((batch, (65537, None), ARG, "B outside", None))
    rows.append((batch, (1, None), ARG, "problems is NULL", None))
    rows.append((batch, (0, None), NODEV, "host-only", None))
    return rows


def test_host_only_status_of_every_refusal(host_ctx):
    """On a host-only context a malformed call is DSH_ERR_ARG with a message naming the entry point and the argument and writes
    nothing, a well-formed one DSH_ERR_NO_DEVICE saying "host-only" -- arguments first, then the device; a NULL store is DSH_ERR_ARG."""
    from test_local_map_cpu import _raw_store
    L = host_ctx._L
    msg = lambda: L.dsh_last_error(host_ctx._h).decode()
    rc, h = _raw_store(L, host_ctx._h)
    assert rc == OK and h
    keep = []
    rows = _rows(keep)
    assert {r[0] for r in rows} == set(NEW_ENTRIES)
    for name, args, want, word, p in rows:
        fn = getattr(L, name)
        assert fn(h, *args) == want, (name, word, msg())
        assert msg().startswith(name + ": ") and word in msg(), (name, word, msg())
        assert fn(None, *args) == ARG, (name, "NULL store")
        if p is not None:                                             # a refusal writes nothing
            assert p.n_initial == -7, (name, word)
            if p.outlier:
                assert bytes(p.outlier[0:4]) == b"\x01" * 4, (name, word)
    assert L.dsh_mpdb_point_count(h) == 0
    assert L.dsh_mpdb_destroy(h) == OK


def test_a_detached_store_refuses_every_new_entry():
    from defslam_amd import sft
    from test_local_map_cpu import _raw_store
    ctx = sft.Context(-1)
    L = ctx._L
    rc, h = _raw_store(L, ctx._h)
    assert rc == OK
    ctx.close()                                    # dsh_destroy detaches the store
    keep = []
    for name, args, _, _, _ in _rows(keep):
        assert getattr(L, name)(h, *args) == ARG, name
    assert L.dsh_mpdb_destroy(h) == OK
