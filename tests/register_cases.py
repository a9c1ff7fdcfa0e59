"""Surface registration away from synth.make_register_scene's one alignment (tests/test_register_cases_cpu.py, test_register_cases_gpu.py):
the inputs of every case, what each of them reaches in oracle/horn_oracle.c -- and so in sim3_exp, quat_from_R and horn_lm_kernel of
defslam_amd/csrc/register_kernels.hip, which restate it -- and references that share no code with the C oracle or the kernels (a closed-form
similarity by SVD, scaleMinMedian with numpy sorting).

Every OptimizeHorn case starts from the identity, START, with chi = 0.05^2 and Huber 0.01.  CASES names, per case, the path counters of
oracle.horn_counts() that a run in the device's summation order has to reach.  Two paths are not reached by any case: an LDLT that is not
positive and a zero pivot.  H + lambda I is positive definite by construction, and none of about thirty finite inputs tried (degenerate
clouds, huge scales, points on a line) produced either; they are not required.  Points on one line are left out altogether: the rotation
about the line is unobservable and the oracle's two summation orders differ by 2e-5 there, so there is no reference to test against."""
import numpy as np

from defslam_amd import synth

START = [0, 0, 0, 1, 0, 0, 0, 1.0]
CHI = 0.05 ** 2
HUBER = 0.01
GEN_ROTVEC = (0.02, -0.035, 0.015)      # the alignment of synth.make_register_scene
GEN_T = (0.03, -0.02, 0.05)


def scene(n, seed, rotvec, t, scale, noise=0.0, outliers=0.0, planar=False):
    """synth.make_register_scene with the alignment as an argument: the same draws in the same order (with the generator's rotation and
    translation the clouds are its clouds bit for bit).  planar: the surface lies in the plane z = 1."""
    rng = np.random.default_rng(seed)
    x, y, z = rng.uniform(-0.4, 0.4, n), rng.uniform(-0.3, 0.3, n), 1.0 + 0.15 * rng.standard_normal(n)
    if planar:
        z = np.ones(n)
    surf = np.stack([x, y, z], 1)
    R = synth._rodrigues(np.array(rotvec, float))
    t = np.array(t, float)
    mp = scale * (surf @ R.T) + t + noise * rng.standard_normal((n, 3))
    bad = rng.random(n) < outliers
    mp[bad] += 0.2 * rng.standard_normal((int(bad.sum()), 3))
    return dict(surface=surf.astype(np.float32), map=mp.astype(np.float32), R=R, t=t, scale=scale, outlier=bad)


def stream(n, candidates, rng, select_all=False):
    """A uniform stream for scaleMinMedian over n pairs in which exactly the listed indices are candidates: a candidate contributes one
    draw <= 0.25 and the n - 1 random draws of its selection (all of them <= 0.25 with select_all: every other pair selected), every
    other index one draw > 0.25.  (n + n^2 numbers are never needed: about 10^5 for n = 8000 with 12 candidates.)"""
    cand = set(int(c) for c in candidates)
    assert all(0 <= c < n for c in cand)
    parts = []
    for i in range(n):
        if i in cand:
            parts.append(np.array([0.25 * rng.random()]))
            parts.append(rng.random(n - 1) * (0.25 if select_all else 1.0))
        else:
            parts.append(np.array([0.25 + 0.75 * (1.0 - rng.random())]))      # (0.25, 1]
    return np.concatenate(parts)


def umeyama(a, b):
    """The least-squares similarity b ~ s R a + t in closed form (Umeyama 1991), float64: (R, t, s).  For clouds without outliers whose
    residuals stay far below the Huber width of 0.1 it minimises the cost OptimizeHorn minimises."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    ma, mb = a.mean(0), b.mean(0)
    A, B = a - ma, b - mb
    U, D, Vt = np.linalg.svd(B.T @ A / a.shape[0])
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:      # the reflection guard
        S[2, 2] = -1.0
    R = U @ S @ Vt
    s = float((D * np.diag(S)).sum() / (A * A).sum() * a.shape[0])
    return R, mb - s * R @ ma, s


def quat_R(q):
    """Rotation matrix of [qx qy qz qw] (normalised first: the oracle and the kernel multiply quaternions without renormalising)."""
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def closed_form_distance(sim3, sc):
    """Largest difference between an estimate [q t s] and umeyama() of the scene, over the entries of R, t and s."""
    R, t, s = umeyama(sc["surface"], sc["map"])
    return max(np.abs(quat_R(sim3[:4]) - R).max(), np.abs(np.asarray(sim3[4:7]) - t).max(), abs(sim3[7] - s))


def smm_numpy(mono, stereo, u):
    """Independent restatement with numpy sorting (float32 where the reference has float)."""
    n = mono.shape[0]
    k = 0
    min_med = np.float32(10000.0)
    best = 0.0
    final_points = 0
    for i in range(n):
        r = u[k]; k += 1
        if r > 0.25:
            continue
        scale = float(np.float32(stereo[i, 2]) / np.float32(mono[i, 2]))
        draws = u[k:k + n - 1]; k += n - 1
        sel = np.ones(n, bool); sel[i] = False
        sel[np.arange(n) != i] = ~(draws > 0.25)
        d = scale * mono[sel].astype(np.float64) - stereo[sel].astype(np.float64)
        r2 = np.zeros(d.shape[0], np.float32)
        for c in range(3):
            r2 = (r2.astype(np.float64) + d[:, c] * d[:, c]).astype(np.float32)
        res = np.sort(np.sqrt(r2))
        final_points += 1
        if res.shape[0] <= 1:
            return 0.0, k, 2
        tail = res[1:]
        med = tail[tail.shape[0] // 2]
        if med < min_med:
            min_med = med; best = scale
    desv = np.float32(1.4826 * (1.0 - (5.0 / (final_points - 1.0))) * float(np.sqrt(min_med)))
    num = np.float32(0); den = np.float32(0)
    for i in range(n):
        d = best * mono[i].astype(np.float64) - stereo[i].astype(np.float64)
        r = np.float32(0)
        for c in range(3):
            r = np.float32(float(r) + d[c] * d[c])
        r = np.sqrt(r)
        if float(np.float32(r / desv)) < 2.5:
            num = np.float32(num + np.float32(stereo[i, 2] * mono[i, 2]))
            den = np.float32(den + np.float32(mono[i, 2] * mono[i, 2]))
    return float(np.float32(num / den)), k, 0


# ---- OptimizeHorn ------------------------------------------------------------------------------------------------------------------------
_TURN_T = (0.05, 0.02, -0.03)


def _axis(k, angle):
    w = [0.0, 0.0, 0.0]
    w[k] = angle
    return tuple(w)


# name -> (scene arguments, {counter: least count in the device's summation order}, compared with the closed form)
CASES = {}
for _s in range(3):
    CASES[f"scale_only_{_s}"] = (dict(n=300, seed=_s, rotvec=(0, 0, 0), t=(0, 0, 0), scale=1.6, noise=1e-3), dict(exp_theta_small=1), True)
CASES["scale_only_1"][1]["trials_exhausted"] = 2      # two iterations end on ten rejected trials
CASES["rot_only"] = (dict(n=300, seed=0, rotvec=(0.5, -0.3, 0.2), t=(0.1, 0, 0), scale=1.0, noise=1e-3), dict(exp_sigma_small=1), True)
for _k, _a in enumerate("xyz"):
    CASES[f"turn_{_a}"] = (dict(n=300, seed=5, rotvec=_axis(_k, 2.2), t=_TURN_T, scale=1.2, noise=1e-3), {f"quat_i{_k}": 4, "exp_general": 11}, True)
CASES["turn_z"][1]["trials_exhausted"] = 1
CASES["half_turn_y"] = (dict(n=300, seed=5, rotvec=_axis(1, 3.0), t=_TURN_T, scale=1.2, noise=1e-3), dict(quat_i1=1), True)
CASES["half_turn_z"] = (dict(n=300, seed=5, rotvec=_axis(2, 3.0), t=_TURN_T, scale=1.2, noise=1e-3), dict(quat_i2=5), True)
# In the turn cases above the rotation of an ACCEPTED step stays below 120 degrees: the arms are taken by overshooting trials, whose only
# use is that they are rejected, and a wrong quaternion there changes at most the number of trials.  With a scale far from the start's the
# first accepted steps turn further: here the estimate itself goes through the arm (with the sign of w flipped in the arm, an oracle built
# that way ends at -q or at other iteration counts in all three).
CASES["far_turn_x"] = (dict(n=300, seed=5, rotvec=_axis(0, 2.6), t=_TURN_T, scale=5.0, noise=1e-3), dict(quat_i0=2, quat_i1=4), True)
CASES["far_turn_y"] = (dict(n=300, seed=5, rotvec=_axis(1, 2.2), t=_TURN_T, scale=2.72, noise=1e-3), dict(quat_i1=1), True)
CASES["far_turn_z"] = (dict(n=300, seed=5, rotvec=_axis(2, 2.2), t=_TURN_T, scale=3.5, noise=1e-3), dict(quat_i2=4), True)
CASES["planar"] =(dict(n=300, seed=5, rotvec=(0.3, 0.1, -0.2), t=_TURN_T, scale=1.2, noise=1e-3, planar=True), dict(exp_general=1), True)
CASES["heavy_outliers"] = (dict(n=300, seed=5, rotvec=GEN_ROTVEC, t=GEN_T, scale=1.3, noise=0.05, outliers=0.5), dict(stop_nbad=1), False)
CASES["nan_point"] = (dict(n=300, seed=5, rotvec=GEN_ROTVEC, t=GEN_T, scale=1.3, noise=1e-3), dict(total_not_finite=1, trial_rejected=100), False)
SIZES = (15, 63, 64, 65, 255, 256, 257, 513)      # lanes, wavefronts and the 256-thread block of block_sum256 and the i += 256 loops
for _n in SIZES:
    CASES[f"size_{_n}"] = (dict(n=_n, seed=40 + _n, rotvec=(0.4, -0.9, 0.5), t=(0.3, -0.2, 0.1), scale=0.7, noise=1e-3), dict(exp_general=1), True)
NAMES = list(CASES)
CLOSED_FORM = [k for k in NAMES if CASES[k][2]]

_SCENES = {}


def case_scene(name):
    """The clouds of a case, built once (read-only for the callers)."""
    if name not in _SCENES:
        sc = scene(**CASES[name][0])
        if name == "nan_point":
            sc["map"][7, 1] = np.nan
        for k in ("surface", "map"):
            sc[k].setflags(write=False)
        _SCENES[name] = sc
    return _SCENES[name]


_ORACLE = {}


def oracle_run(oracle_mod, name, device_sum_order):
    """optimize_horn of the oracle on a case from START, run once per summation order, with the path counters of that run under "counts"."""
    key = (name, bool(device_sum_order))
    if key not in _ORACLE:
        sc = case_scene(name)
        oracle_mod.horn_counts(reset=True)
        r = oracle_mod.optimize_horn(sc["surface"], sc["map"], START, chi=CHI, huber=HUBER, device_sum_order=device_sum_order)
        r["counts"] = oracle_mod.horn_counts(reset=True)
        _ORACLE[key] = r
    return _ORACLE[key]


def edge_chi2(sim3, sc):
    """chi2 of every edge at an estimate, float64."""
    y = sim3[7] * (sc["surface"].astype(np.float64) @ quat_R(sim3[:4]).T) + np.asarray(sim3[4:7])
    e = sc["map"].astype(np.float64) - y
    return (e * e).sum(1)


# ---- scaleMinMedian ----------------------------------------------------------------------------------------------------------------------
def _spread(n, k):
    """k candidate indices spread over 0 .. n-1, none at either end."""
    return [int(v) for v in np.linspace(1, n - 2, k).round()]


def _smm_gen(n, cands, seed=3):
    """The clouds of synth.make_register_scene(n, seed) without its n + n^2 uniform numbers, and a stream with the listed candidates."""
    sc = scene(n, seed, GEN_ROTVEC, GEN_T, 1.35, noise=2e-3, outliers=0.05)
    return sc["surface"], sc["map"], stream(n, cands, np.random.default_rng(1000 + n))


def _smm_equal():
    sc = synth.make_register_scene(60, seed=4)
    return np.tile(sc["surface"], (4, 1)), np.tile(sc["map"], (4, 1)), np.random.default_rng(44).random(240 + 240 * 240)


TIE_N, TIE_CANDS = 300, [1, 10, 20, 30, 40, 50, 60, 70]


def _smm_tie_below_median():
    """The median right above a run of equal residuals.  151 pairs (indices 1 .. 75 and 200 .. 275) are scaled by exactly 2, the other 149
    by 2 + delta with |delta| in 0.05 .. 0.5, pair 0 by 2.02: for a candidate among the 151, with every other pair selected, the sorted
    residuals are 150 zeros and then the others, pair 0's first -- and the reference's median is element k = 150, pair 0's residual.  The
    count of values <= 0 equals k, so a selection by counting that lets `k <= leq` pass takes a zero as well (desv 0, no inlier, a NaN
    scale); thread 0 of the kernel holds pair 0 and then pair 256, one of the zeros."""
    sc = scene(TIE_N, 8, GEN_ROTVEC, GEN_T, 1.0)
    mono = sc["surface"]
    rng = np.random.default_rng(88)
    s = 2.0 + rng.uniform(0.05, 0.5, TIE_N) * rng.choice([-1.0, 1.0], TIE_N)
    s[1:76] = 2.0
    s[200:276] = 2.0
    s[0] = 2.02
    stereo = (s[:, None] * mono.astype(np.float64)).astype(np.float32)
    return mono, stereo, stream(TIE_N, TIE_CANDS, rng, select_all=True)


def exact_fit(n=60):
    """map = float32(2 * surface): every residual 0, desv 0, no inlier, scale 0/0."""
    sc = synth.make_register_scene(n, seed=6)
    return sc["surface"], (2 * sc["surface"]).astype(np.float32), sc["u"]


# name -> () -> (mono, stereo, u); with a dozen candidates smm_numpy walks even the 8000-pair case in a tenth of a second
SMM_CASES = {
    "n8000_12": lambda: _smm_gen(8000, _spread(8000, 12)),          # the host's limit: 64000 bytes of dynamic LDS in smm_finish_kernel
    "n4097_9": lambda: _smm_gen(4097, _spread(4097, 9)),
    "ends_300": lambda: _smm_gen(300, [0, 150, 299]),               # j < i ? j : j - 1 at i = 0 and i = n - 1
    "equal_240": _smm_equal,                                        # every residual four times: the median found by counting
    "tie_below_300": _smm_tie_below_median,                         # less == k: the first element after a run of equal values
    "n1": lambda: _smm_gen(1, [0]),                                 # the early return: status 2, scale 0
    "n2": lambda: _smm_gen(2, [1]),
    "exact_fit": exact_fit,                                         # NaN scale, status 0
}
_SMM = {}


def smm_inputs(name):
    if name not in _SMM:
        _SMM[name] = SMM_CASES[name]()
    return _SMM[name]


def same_scale(a, b):
    """float32 scales equal bit for bit; two NaNs are equal whatever their sign (0/0 is -NaN on x86 and +NaN on the device)."""
    a, b = np.float32(a), np.float32(b)
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    return a.view(np.uint32) == b.view(np.uint32)


# ---- registerSurfaces --------------------------------------------------------------------------------------------------------------------
def _twc(rotvec, t):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = synth._rodrigues(np.array(rotvec, float)).astype(np.float32)
    T[:3, 3] = np.array(t, np.float32)
    return T


def register_inputs(name):
    """(surface, map, u, Twc) of an end-to-end case."""
    if name == "exact_fit":
        a, b, u = exact_fit()
        return a, b, u, np.eye(4, dtype=np.float32)
    if name == "rotated":
        sc = scene(400, 23, (0.3, 0.1, -0.2), GEN_T, 1.3, noise=2e-3)
        return sc["surface"], sc["map"], np.random.default_rng(23).random(400 + 400 * 400), _twc((0.1, 0.05, -0.07), (0.2, -0.1, 0.3))
    sc = synth.make_register_scene(400, seed=22, outliers=0.0)
    Twc = {"twc_identity": np.eye(4, dtype=np.float32), "twc_turned": _twc((1.5, -1.6, 1.2), (1, -2, 0.5)), "twc_generator": sc["Twc"]}[name]
    return sc["surface"], sc["map"], sc["u"], Twc


REGISTER_CASES = ["twc_identity", "twc_turned", "twc_generator", "rotated", "exact_fit"]


def oracle_chain(oracle_mod, a, b, u, Twc, chi_limit=0.05):
    """SurfaceRegistration::registerSurfaces from the oracle's parts: (scale_min_median, optimize_horn from that scale, horn_compose)."""
    s0 = oracle_mod.scale_min_median(a, b, u)
    o = oracle_mod.optimize_horn(a, b, [0, 0, 0, 1, 0, 0, 0, s0["scale"]], chi=chi_limit ** 2)
    return s0, o, oracle_mod.horn_compose(o["sim3"], Twc)
