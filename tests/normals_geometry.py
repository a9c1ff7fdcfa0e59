"""Plane geometry for the NRSfM normals stage (tests/test_normals_geometry_cpu.py, test_normals_geometry_gpu.py): cases whose answer is
known in closed form, independent of oracle/nrsfm_oracle.c and of the reference file both it and the kernels were transcribed from.

A rigid plane N.X = 1 in camera 1, seen from a camera (R, t), X2 = R X1 + t, induces the homography R + t N^T between the normalised
images.  Its first and second derivatives at (u, v) are the DiffProp fields.  In camera 1 the normal of the plane at (u, v) is
    k = N[:2] / (N.(u, v, 1)),   normal = (k1, k2, 1 - k1 u - k2 v);
in camera 2 the same plane is N2 = R N / (1 + t.R N), and its normal at eta(u, v) is k2 = N2[:2] / (N2.(eta_u, eta_v, 1)).

The reference forms the polynomial's t2 from the H12vv slots (NormalEstimator.cc:96-97) and the propagation's t2 from the H12uu slots
(:210); product and oracle keep both.  With t1 = -b Hvvx / 2 + a Hvvy / 2 and t2 = d Huux / 2 - c Huuy / 2 the two polynomials vanish at
the k above; with the reference's t2 they do not.  quirk_neutral() rewrites the two H12vv slots of a record so that the reference's
expressions yield exactly those t1 and t2 -- in the polynomial and in the propagation alike -- and touches nothing else: on such
records the reference's answer IS the geometric one, and every kernel of the stage can be held to the closed form.

Every number marked "measured" below was produced by the CPU oracle with the command in profiles/normals_geometry/README.md; the
tolerances are those numbers times TOL_FACTOR and never come from a device result."""
import numpy as np

from defslam_amd import synth

BLOCK = 128          # threads per block of the three launches of nrsfm_launch_normals (defslam_amd/csrc/nrsfm_kernels.hip)
KEYS = ["rec_ptr", "recs", "rec_is_ref", "rec_first_normal", "rec_has_first_normal", "x0", "has_x0", "ref_uv"]
(F_I1u, F_I1v, F_I2u, F_I2v, F_a, F_b, F_c, F_d, F_J21a, F_J21b, F_J21c, F_J21d, F_Huux, F_Huuy, F_Huvx, F_Huvy, F_Hvvx, F_Hvvy) = range(18)
# coefficient order x^3, x^2 y, x y^2, y^3, x^2, x y, y^2, x, y, 1; the structural zeros of the two polynomials
ZERO_COEFFS = ((2, 3, 6), (0, 1, 4))
BASIN = 1e-4         # classifies an oracle answer as "at the truth": measured errors are <= 6e-5 or >= 1e-2 in every case, none between
GAP = (1e-4, 1e-2)
TOL_FACTOR = 4.0


def monomials(k):
    x, y = float(k[0]), float(k[1])
    return np.array([x ** 3, x * x * y, x * y * y, y ** 3, x * x, x * y, y * y, x, y, 1.0])


def normal_at(N, u, v):
    """(k1, k2) of the plane N.X = 1 at the normalised image point (u, v)."""
    N = np.asarray(N, np.float64)
    return N[:2] / (N @ np.array([u, v, 1.0]))


def plane_in_second_camera(N, R, t):
    RN = R @ np.asarray(N, np.float64)
    return RN / (1.0 + t @ RN)


def homography_record(N, u, v, R, t):
    """The 18 DiffProp fields (float64) of the warp R + t N^T at (u, v), in the order of DIFFPROP_FIELDS; J21 as SchwarpDatabase.cc:322-329
    assigns it (J21a = d / det, J21b = -c / det, J21c = -b / det, J21d = a / det)."""
    Hm = R + np.outer(t, N)
    eta, d1, d2 = synth._homography_derivs(Hm, u, v)
    a, b = d1["u"]
    c, d = d1["v"]
    det = a * d - c * b
    return np.array([u, v, eta[0], eta[1], a, b, c, d, d / det, -c / det, -b / det, a / det,
                     d2["uu"][0], d2["uu"][1], d2["uv"][0], d2["uv"][1], d2["vv"][0], d2["vv"][1]])


def quirk_neutral(recs):
    """(R, 18) float32 records -> a float32 copy whose H12vvx, H12vvy slots hold the solution (X, Y) of
        -b X / 2 + a Y / 2 = t1 = -b Hvvx / 2 + a Hvvy / 2
        -d X / 2 + c Y / 2 = t2 =  d Huux / 2 - c Huuy / 2
    (solved in float64 from the float32 fields).  Every other field is untouched."""
    out = np.array(recs, np.float32, copy=True).reshape(-1, 18)
    f = out.astype(np.float64)
    a, b, c, d = f[:, F_a], f[:, F_b], f[:, F_c], f[:, F_d]
    t1 = -b * f[:, F_Hvvx] / 2 + a * f[:, F_Hvvy] / 2
    t2 = d * f[:, F_Huux] / 2 - c * f[:, F_Huuy] / 2
    det = (a * d - b * c) / 4
    out[:, F_Hvvx] = ((c / 2) * t1 - (a / 2) * t2) / det
    out[:, F_Hvvy] = ((d / 2) * t1 - (b / 2) * t2) / det
    return out


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
# views: records per point, uniform in [lo, hi]; rot: rotation angle range (rad); trans: each translation component in +-trans;
# tilt: N ~ (U(-tilt, tilt), U(-tilt, tilt), 1) / U(0.8, 1.5); start: "none" = the reference's (0, -0), "near" = truth + N(0, 0.05);
# cap: the share of points with >= 2 reference records that a truth comparison may leave out (5 % small motion, 15 % large motion).
# Shape cases (block size 128, one thread per record / per point): P = 1; P = 127 and 129, R no multiple of 128; in every case with
# P >= 3 point P // 2 has no reference record (its neighbours are solved) and point P // 2 + 1 has only reference records.
CASES = {
    "small_none": dict(P=300, seed=11, views=(2, 6), rot=(0.03, 0.15), trans=0.15, tilt=0.4, start="none", nonref_frac=0.3, cap=0.05),
    "small_near": dict(P=300, seed=12, views=(2, 6), rot=(0.03, 0.15), trans=0.15, tilt=0.4, start="near", nonref_frac=0.3, cap=0.05),
    "large_none": dict(P=300, seed=13, views=(2, 6), rot=(0.2, 0.5), trans=0.15, tilt=0.4, start="none", nonref_frac=0.3, cap=0.15),
    "tilted_near": dict(P=200, seed=14, views=(2, 6), rot=(0.03, 0.15), trans=0.25, tilt=0.8, start="near", nonref_frac=0.5, cap=0.05),
    "one_point": dict(P=1, seed=15, views=(5, 5), rot=(0.03, 0.15), trans=0.15, tilt=0.4, start="near", nonref_frac=0.3, cap=0.05),
    "block_minus_1": dict(P=BLOCK - 1, seed=16, views=(2, 6), rot=(0.03, 0.15), trans=0.15, tilt=0.4, start="none", nonref_frac=0.3, cap=0.05),
    "block_plus_1": dict(P=BLOCK + 1, seed=17, views=(2, 6), rot=(0.03, 0.15), trans=0.15, tilt=0.4, start="near", nonref_frac=0.3, cap=0.05),
}
CASE_IDS = list(CASES)

# Measured with the CPU oracle (profiles/normals_geometry/README.md): the largest error to the closed form over the counted points
# (k: |k1k2 - truth|; nref: normal_ref; rec_ref: normal_rec of reference records against the camera-2 truth; rec_first: normal_rec of
# non-reference records with a first normal), the share of candidates left out, and the largest |e(truth)| / |e(0)| of the polynomial.
# It is float32 rounding of the record fields amplified by each point's conditioning.  The tests allow TOL_FACTOR times these.
# counted = (candidates, counted): points with >= 2 reference records, and those of them whose oracle answer is within BASIN of the truth.
MEASURED = {
    "small_none": dict(k=1.13e-05, nref=1.13e-05, rec_ref=1.22e-05, rec_first=6.01e-08, counted=(252, 242)),     # R 1203; 3.97 % left out, the nearest of them 1.32e-01 away
    "small_near": dict(k=4.85e-06, nref=4.84e-06, rec_ref=5.41e-06, rec_first=6.76e-08, counted=(253, 253)),     # R 1168
    "large_none": dict(k=4.11e-06, nref=4.11e-06, rec_ref=4.43e-06, rec_first=1.02e-07, counted=(244, 229)),     # R 1216; 6.15 % left out, the nearest 1.47e-01 away
    "tilted_near": dict(k=1.19e-06, nref=1.18e-06, rec_ref=1.43e-06, rec_first=1.03e-07, counted=(125, 125)),    # R 807
    "one_point": dict(k=1.24e-07, nref=1.19e-07, rec_ref=1.31e-07, rec_first=2.25e-08, counted=(1, 1)),          # R 5: three reference records, one with a first normal
    "block_minus_1": dict(k=4.26e-06, nref=4.25e-06, rec_ref=3.89e-06, rec_first=7.16e-08, counted=(109, 106)),  # R 508; 2.75 % left out, the nearest 2.54e-01 away
    "block_plus_1": dict(k=5.34e-06, nref=5.34e-06, rec_ref=5.93e-06, rec_first=6.08e-08, counted=(112, 112)),   # R 520
}
# Largest |e(truth)| / |e(0)| over the 3698 reference records of all cases (neutral records); the median is 3.05e-07.  The maximum belongs
# to records whose |e(0)| is small, so the same residual is also held relative to the sum of the absolute terms of both polynomials at
# the truth, which has no such outliers (ROOT_TERMS_MEASURED, largest over the same records).  Bounds: measured x ROOT_RATIO_FACTOR.
ROOT_RATIO_MEASURED = 4.07e-03
ROOT_TERMS_MEASURED = 4.36e-06
ROOT_RATIO_FACTOR = 10.0


def _draw_plane(rng, tilt):
    n = np.array([rng.uniform(-tilt, tilt), rng.uniform(-tilt, tilt), 1.0])
    return n / rng.uniform(0.8, 1.5)


def _draw_motion(rng, rot, trans):
    w = rng.normal(size=3)
    w *= rng.uniform(*rot) / np.linalg.norm(w)
    return synth._rodrigues(w), rng.uniform(-trans, trans, size=3)


def _draw_point(rng):
    return (float(np.float32(rng.uniform(-0.4, 0.4))), float(np.float32(rng.uniform(-0.4, 0.4))))     # exactly representable in float32


def make_scene(name, neutral=True):
    """The flat arrays of dsh_normals_estimate (KEYS) for CASES[name] plus the closed-form truth:
    k_true (P, 2), normal_ref_true (P, 3), normal_rec_true (R, 3) (camera 2 of every record: of the point's plane for reference records,
    of the record's own plane for the others), n_ref (P,) reference records per point, rec_point (R,).
    A non-reference record is a pair of two other keyframes: it carries its own plane and its own point in its own first camera, and
    where rec_has_first_normal is set, rec_first_normal is that camera's true (k1, k2).  neutral=False leaves the records as the
    homography gives them (the reference's t2 then does not have its root at the truth)."""
    cs = CASES[name]
    rng = np.random.default_rng(cs["seed"])
    P = cs["P"]
    no_ref, all_ref = (P // 2, P // 2 + 1) if P >= 3 else (-1, -1)
    recs, is_ref, first_n, has_first_n, rec_ptr, rec_true, rec_point = [], [], [], [], [0], [], []
    x0, ref_uv, k_true, nref_true = [], [], [], []
    for p in range(P):
        N = _draw_plane(rng, cs["tilt"])
        u, v = _draw_point(rng)
        k = normal_at(N, u, v)
        for _ in range(int(rng.integers(cs["views"][0], cs["views"][1] + 1))):
            ref = rng.uniform() >= cs["nonref_frac"]
            ref = False if p == no_ref else True if p == all_ref else ref
            R, t = _draw_motion(rng, cs["rot"], cs["trans"])
            if ref:
                Nr, ur, vr = N, u, v
            else:
                Nr = _draw_plane(rng, cs["tilt"])
                ur, vr = _draw_point(rng)
            rec = homography_record(Nr, ur, vr, R, t)
            k2 = normal_at(plane_in_second_camera(Nr, R, t), rec[F_I2u], rec[F_I2v])
            hf = (not ref) and rng.uniform() < 0.7
            recs.append(rec)
            is_ref.append(ref)
            has_first_n.append(hf)
            first_n.append(normal_at(Nr, ur, vr) if hf else np.zeros(2))
            rec_true.append([k2[0], k2[1], 1 - k2[0] * rec[F_I2u] - k2[1] * rec[F_I2v]])
            rec_point.append(p)
        rec_ptr.append(len(recs))
        x0.append(k + rng.normal(scale=0.05, size=2) if cs["start"] == "near" else np.zeros(2))
        ref_uv.append([u, v])
        k_true.append(k)
        nref_true.append([k[0], k[1], 1 - k[0] * u - k[1] * v])
    recs = np.asarray(recs, np.float32).reshape(-1, 18)
    rec_ptr = np.asarray(rec_ptr, np.int32)
    is_ref = np.asarray(is_ref, np.uint8)
    return dict(rec_ptr=rec_ptr, recs=quirk_neutral(recs) if neutral else recs, rec_is_ref=is_ref,
                rec_first_normal=np.asarray(first_n, np.float32).reshape(-1, 2), rec_has_first_normal=np.asarray(has_first_n, np.uint8),
                x0=np.asarray(x0, np.float32).reshape(-1, 2), has_x0=np.full(P, 1 if cs["start"] == "near" else 0, np.uint8),
                ref_uv=np.asarray(ref_uv, np.float32).reshape(-1, 2),
                k_true=np.asarray(k_true), normal_ref_true=np.asarray(nref_true), normal_rec_true=np.asarray(rec_true).reshape(-1, 3),
                n_ref=np.bincount(rec_point, weights=is_ref, minlength=P).astype(np.int64), rec_point=np.asarray(rec_point, np.int64),
                no_ref_point=no_ref, all_ref_point=all_ref)


def args(sc):
    return [sc[k] for k in KEYS]


def classify(sc, oracle_k1k2, oracle_status):
    """(candidates, counted): points with >= 2 reference records that the oracle solved; those of them whose ORACLE answer is within BASIN of
    the truth.  The counted set is the oracle's: a device result is compared on it and never redefines it."""
    cand = (sc["n_ref"] >= 2) & (np.asarray(oracle_status) == 0)
    err = np.abs(np.asarray(oracle_k1k2) - sc["k_true"]).max(axis=1)
    return cand, cand & (err <= BASIN)


def truth_errors(sc, counted, k1k2, normal_ref, normal_rec):
    """Largest errors to the closed form over the counted points: dict(k, nref, rec_ref, rec_first); 0.0 where a set is empty."""
    rc = counted[sc["rec_point"]]
    ref = rc & (sc["rec_is_ref"] == 1)
    # a non-reference record's normal depends on its own first normal alone: every point's counts, as long as the point was not rejected
    first = (sc["rec_is_ref"] == 0) & (sc["rec_has_first_normal"] == 1)

    def mx(x):
        return float(np.abs(x).max()) if x.size else 0.0
    return dict(k=mx(np.asarray(k1k2)[counted] - sc["k_true"][counted]), nref=mx(np.asarray(normal_ref, np.float64)[counted] - sc["normal_ref_true"][counted]),
                rec_ref=mx(np.asarray(normal_rec, np.float64)[ref] - sc["normal_rec_true"][ref]),
                rec_first=mx(np.asarray(normal_rec, np.float64)[first] - sc["normal_rec_true"][first]))


# ---- a fitted warp against the warp's analytic derivatives ---------------------------------------------------------------------------------
# Exact homography matches of one plane: 400 key points in [-0.55, 0.55] x [-0.42, 0.42], no ripple, no noise, float32.  Four keyframe
# motions, each with a rotation about z of 0.18 .. 0.3 rad, so that b = d eta_v / du and c = d eta_u / dv differ by about 2 sin(angle).
WARP_POINTS = 400
WARP_PLANES = {"plane": np.array([0.15, -0.1, 1.0]) / 1.1, "tilted": np.array([0.45, -0.35, 1.0]) / 1.2}
WARP_MOTIONS = [(np.array([0.02, -0.05, 0.30]), np.array([0.06, -0.04, 0.02])),
                (np.array([-0.04, 0.03, -0.35]), np.array([-0.05, 0.07, -0.03])),
                (np.array([0.05, 0.04, 0.40]), np.array([0.03, 0.08, 0.04])),
                (np.array([-0.03, -0.06, -0.28]), np.array([-0.08, -0.02, 0.03]))]
WARP_GRIDS = [(13, 15), (8, 8)]          # the reference's grid and one further grid of tests/grid_cases.py (2N = 128, no padding)
# Warp::initialize with a bending weight of 1e-7 (at the mapping default of 1e-2 the bending term alone puts the first derivatives 1e-2
# from the homography's, and b - c could not be told from the fit error), then ten iterations of the Schwarzian fit, which accept steps.
WARP_INIT_LAMBDA, WARP_FIT_LAMBDA, WARP_FIT_ITERS = 1e-7, 0.1, 10
WARP_FX, WARP_FY = 520.0, 515.0
INNER = (0.45, 0.32)                      # second derivatives are compared for |u| < 0.45, |v| < 0.32 (the spline's border is less well tied down)
FIRST_FIELDS = [F_a, F_b, F_c, F_d]
INVERSE_FIELDS = [F_J21a, F_J21b, F_J21c, F_J21d]
SECOND_FIELDS = [F_Huux, F_Huuy, F_Huvx, F_Huvy, F_Hvvx, F_Hvvy]
WARP_PARAMS = [(pl, g) for pl in WARP_PLANES for g in WARP_GRIDS]
WARP_IDS = [f"{pl}-{g[0]}x{g[1]}" for pl, g in WARP_PARAMS]

# Measured with the CPU oracle (warp_initialize + schwarp_fit), largest error over the four motions against the analytic fields:
# first (fields 4-7, all points), inverse (fields 8-11, all points), second (fields 12-17, inner set); chain: median and 90th percentile
# of |k1k2 - truth| over the inner set after quirk_neutral + the normals oracle on the four fitted records of every point.
WARP_MEASURED = {
    ("plane", (13, 15)): dict(first=9.03e-04, inverse=8.27e-04, second=1.67e-03, chain_median=3.71e-04, chain_p90=1.24e-03),    # chain max 3.52e-03
    ("plane", (8, 8)): dict(first=2.28e-04, inverse=1.70e-04, second=1.88e-04, chain_median=3.17e-05, chain_p90=1.21e-04),      # chain max 5.55e-04
    ("tilted", (13, 15)): dict(first=8.09e-04, inverse=7.82e-04, second=1.85e-03, chain_median=5.39e-04, chain_p90=1.63e-03),   # chain max 9.21e-03
    ("tilted", (8, 8)): dict(first=2.20e-04, inverse=1.78e-04, second=2.20e-04, chain_median=4.93e-05, chain_p90=1.64e-04),     # chain max 1.35e-03
}


def warp_key_points():
    rng = np.random.default_rng(21)
    return np.stack([rng.uniform(-0.55, 0.55, WARP_POINTS), rng.uniform(-0.42, 0.42, WARP_POINTS)], 1).astype(np.float32)


def warp_inner(kp1):
    return (np.abs(kp1[:, 0]) < INNER[0]) & (np.abs(kp1[:, 1]) < INNER[1])


def warp_pair(plane, m, grid):
    """Matches of motion m on the plane, the fit's inputs on the grid, and the analytic DiffProp fields (P, 18) float64."""
    kp1 = warp_key_points()
    N = WARP_PLANES[plane]
    R, t = synth._rodrigues(WARP_MOTIONS[m][0]), WARP_MOTIONS[m][1]
    truth = np.stack([homography_record(N, float(u), float(v), R, t) for u, v in kp1])
    kp2 = truth[:, [F_I2u, F_I2v]].astype(np.float32)
    bbs = (float(kp1[:, 0].min() - 0.10), float(kp1[:, 0].max() + 0.10), grid[0], float(kp1[:, 1].min() - 0.10), float(kp1[:, 1].max() + 0.10), grid[1], 2)
    octave = np.random.default_rng(22 + m).integers(0, 6, WARP_POINTS)
    invsig = np.sqrt((1.2 ** (-2.0 * octave)).astype(np.float32)).astype(np.float32)
    return dict(bbs=bbs, kp1=kp1, kp2=kp2, invsig=invsig, fx=WARP_FX, fy=WARP_FY, truth=truth, k_true=np.stack([normal_at(N, float(u), float(v)) for u, v in kp1]))


def warp_field_errors(diff, pr):
    """Largest error of fitted records against the analytic fields: dict(first, inverse, second)."""
    e = np.abs(np.asarray(diff, np.float64) - pr["truth"])
    inner = warp_inner(pr["kp1"])
    return dict(first=float(e[:, FIRST_FIELDS].max()), inverse=float(e[:, INVERSE_FIELDS].max()), second=float(e[inner][:, SECOND_FIELDS].max()))


def chain_inputs(diffs, neutral=True):
    """The four pairs' records of every key point as one ObtainK1K2 call: point p owns records 4 p .. 4 p + 3, all of the reference
    keyframe, start (0, -0).  Returns the argument list in KEYS order."""
    P = diffs[0].shape[0]
    recs = np.stack(diffs, 1).reshape(-1, 18).astype(np.float32)
    if neutral:
        recs = quirk_neutral(recs)
    M = len(diffs)
    return [np.arange(0, M * P + 1, M, dtype=np.int32), recs, np.ones(M * P, np.uint8), np.zeros((M * P, 2), np.float32), np.zeros(M * P, np.uint8),
            np.zeros((P, 2), np.float32), np.zeros(P, np.uint8), diffs[0][:, :2].astype(np.float32)]


def chain_errors(k1k2, pr):
    """(median, 90th percentile, max) of |k1k2 - truth| over the inner set."""
    e = np.abs(np.asarray(k1k2) - pr["k_true"]).max(axis=1)[warp_inner(pr["kp1"])]
    return float(np.median(e)), float(np.percentile(e, 90)), float(e.max())
