"""Seeded synthetic SfT inputs.

The reference has no dataset that can be loaded here (OpenCV + Mandala/Hamlyn
sequences absent), so tests and bench use this generator: a regular-grid template
at z~1 in front of a 640x480 pinhole camera, a smooth ground-truth deformation,
a small ground-truth camera motion and barycentric-embedded "ORB matches" with
pixel noise and outliers.  Values that are float32 in the reference (keypoints,
invSigma2, barycentrics, the 4x4 pose) are rounded through float32 here so both
the oracle and the HIP path see exactly what DefPoseOptimization would see
(Modules/Tracking/DefOptimizer.cc:293-361).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

# Regularisers of the Mandala sequences (reference yaml: Regularizer.laplacian/Inextensibility/temporal).
REG_LAP = 700.0
REG_INEX = 12000.0
REG_TEMP = 0.05
N_FRAME_KEYPOINTS = 1200
CAMERA_K = (500.0, 500.0, 320.0, 240.0)  # fx, fy, cx, cy for a 640x480 frame
IMAGE_SIZE = (640, 480)                  # width, height

CONFIGS = {
    # name: (rows, cols, matches)
    "smoke": (10, 10, 300),
    "REF": (10, 10, 450),   # the reference's own default size: 10 x 10 template (TriangularMesh.cc:63-64), 1200 features per frame of which a few hundred match
    "C2": (25, 20, 1000),   # 500-node template, 1000 matches (BASELINE.json configs[1])
    "C5": (50, 40, 4000),   # 2000-node template, 4000 matches (configs[4], per problem)
    "W12": (8, 30, 500),    # small wide-band cases for oracle-sized parity runs: half-bandwidth 182 (12 sub-diagonal tiles) ...
    "W16": (6, 41, 500),    # ... and 248 (16 tiles, the C5 band) with 246 nodes
    "B272": (5, 45, 400),   # half-bandwidth 272 > 256: the row-major band solver (general fallback)
}


@dataclass
class GridTemplate:
    rows: int
    cols: int
    xyz0: np.ndarray            # (n,3) float64 rest shape
    facets: np.ndarray          # (F,3) int32, as emitted by the regular triangulation (unsorted)

    @property
    def n(self) -> int:
        return self.rows * self.cols


@dataclass
class SftFrame:
    Tcw: np.ndarray             # (4,4) float32 initial pose (previous frame's pose)
    K: np.ndarray               # (4,) float64 fx,fy,cx,cy
    n_frame: int                # number of keypoints in the frame (scales the information)
    obs_facet: np.ndarray       # (M,) int32
    obs_nodes: np.ndarray       # (M,3) int32 ascending node ids of the facet
    obs_bary: np.ndarray        # (M,3) float64 (float32-valued)
    obs_uv: np.ndarray          # (M,2) float64 (float32-valued)
    obs_invsig2: np.ndarray     # (M,) float64 (float32-valued)
    xyz: np.ndarray             # (n,3) float64 current node estimates
    gt_xyz: np.ndarray = field(default=None)
    gt_Tcw: np.ndarray = field(default=None)
    is_outlier_gt: np.ndarray = field(default=None)


def regular_triangulation(rows: int, cols: int) -> np.ndarray:
    """Facet list of the reference's regular mesh (Modules/Template/TriangularMesh.cc:92-107),
    generalised to rows x cols with node id = col + cols*row."""
    f = []
    for j in range(rows - 1):
        for i in range(cols - 1):
            f.append((i + cols * j, i + cols * j + 1, cols * (j + 1) + i))
            f.append((i + cols * j + 1, cols * (j + 1) + i, cols * (j + 1) + i + 1))
    return np.asarray(f, dtype=np.int32)


def make_grid_template(rows: int, cols: int, seed: int = 1234, z0: float = 1.0, *, camera=CAMERA_K, image_size=IMAGE_SIZE) -> GridTemplate:
    """camera = (fx, fy, cx, cy) and image_size = (width, height) place the grid in the frustum; z0 is the scene scale (depth of the
    template, and its bump scales with it)."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = camera
    width, height = image_size
    # cover 80% of the frustum at depth z0
    xs = np.linspace(-0.8 * cx / fx, 0.8 * (width - cx) / fx, cols) * z0
    ys = np.linspace(-0.8 * cy / fy, 0.8 * (height - cy) / fy, rows) * z0
    X, Y = np.meshgrid(xs, ys)  # row-major: node id = col + cols*row
    ph = rng.uniform(0, 2 * np.pi, size=2)
    # low-frequency bump, amplitude 0.02 z0, so the rest mean curvature is non-zero
    Z = z0 + (0.02 * z0) * np.sin(2 * np.pi * X / (xs[-1] - xs[0]) + ph[0]) * np.cos(2 * np.pi * Y / (ys[-1] - ys[0]) + ph[1])
    xyz0 = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    # the reference builds nodes from float32 vertices (TriangularMesh.cc:109-123)
    xyz0 = xyz0.astype(np.float32).astype(np.float64)
    return GridTemplate(rows, cols, xyz0, regular_triangulation(rows, cols))


def _rodrigues(w: np.ndarray) -> np.ndarray:
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def make_frame(tmpl: GridTemplate, n_matches: int, problem_id: int = 0, *,
               bend: float = 0.05, rot_deg: float = 3.0, trans: float = 0.02,
               noise_px: float = 0.5, outlier_frac: float = 0.05,
               n_frame: int = N_FRAME_KEYPOINTS, init_xyz: np.ndarray | None = None,
               init_Tcw: np.ndarray | None = None, phase: float = 0.0, gt_pose: tuple | None = None,
               camera=CAMERA_K, image_size=IMAGE_SIZE, scale: float = 1.0) -> SftFrame:
    """gt_pose = (rotation vector, translation) fixes the ground-truth camera (sequences: a smooth trajectory) instead of
    drawing it from the problem's random stream; the stream is consumed identically either way.  camera = (fx, fy, cx, cy) and
    image_size = (width, height) are the frame's pinhole and the area the outliers fall in; scale is the scene scale (the z0 of the
    template): bend and ground-truth translation are multiplied by it."""
    rng = np.random.default_rng(42 + problem_id)
    fx, fy, cx, cy = camera
    xyz0 = tmpl.xyz0
    width = xyz0[:, 0].max() - xyz0[:, 0].min()
    # smooth, roughly isometric bend: sinusoid with wavelength = mesh width
    gt = xyz0.copy()
    gt[:, 2] += (bend * scale) * np.sin(2 * np.pi * (xyz0[:, 0] - xyz0[:, 0].min()) / width + phase + 0.3 * problem_id)
    # ground-truth camera: small SE3 offset
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = np.deg2rad(rot_deg) * rng.uniform(0.3, 1.0)
    R = _rodrigues(axis * ang)
    t = rng.uniform(-trans, trans, size=3) * scale
    if gt_pose is not None:
        R = _rodrigues(np.asarray(gt_pose[0], dtype=np.float64))
        t = np.asarray(gt_pose[1], dtype=np.float64)
    gtT = np.eye(4)
    gtT[:3, :3] = R
    gtT[:3, 3] = t

    F = tmpl.facets.shape[0]
    fac = rng.integers(0, F, size=n_matches).astype(np.int32)
    bary = rng.dirichlet((1.0, 1.0, 1.0), size=n_matches).astype(np.float32).astype(np.float64)
    nodes = np.sort(tmpl.facets[fac], axis=1).astype(np.int32)  # std::set<Node*> order
    pw = (bary[:, :, None] * gt[nodes]).sum(axis=1)
    pc = pw @ R.T + t
    uv = np.stack([fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy], axis=1)
    uv += rng.normal(scale=noise_px, size=uv.shape)
    is_out = rng.uniform(size=n_matches) < outlier_frac
    uv_out = np.stack([rng.uniform(0, image_size[0], size=n_matches), rng.uniform(0, image_size[1], size=n_matches)], axis=1)
    uv = np.where(is_out[:, None], uv_out, uv)
    uv = uv.astype(np.float32).astype(np.float64)
    octave = rng.integers(0, 6, size=n_matches)
    invsig2 = (1.2 ** (-2.0 * octave)).astype(np.float32).astype(np.float64)

    Tcw = np.eye(4, dtype=np.float32) if init_Tcw is None else np.asarray(init_Tcw, dtype=np.float32)
    xyz = xyz0.copy() if init_xyz is None else np.asarray(init_xyz, dtype=np.float64).copy()
    return SftFrame(Tcw=Tcw, K=np.asarray(camera, dtype=np.float64), n_frame=n_frame,
                    obs_facet=fac, obs_nodes=nodes, obs_bary=bary, obs_uv=uv, obs_invsig2=invsig2,
                    xyz=xyz, gt_xyz=gt, gt_Tcw=gtT, is_outlier_gt=is_out)


# ---------------------------------------------------------------------------------------------------------
# SEQ100 (the runnable substitute of BASELINE.json configs[0] / configs[2], the Mandala sequences that
# need OpenCV + datasets): a sequence of frames with temporally smooth deformation and camera motion.  Frame k is
# tracked from the result of frame k-1 (DefTracking.cc:350: each frame starts at the previous pose / mesh; the pose
# takes the reference's float32 round trip through cv::Mat).
# ---------------------------------------------------------------------------------------------------------
SEQ100 = dict(config="C2", n_frames=100, seq_id=0)


def sequence_gt_pose(k: int, n_frames: int, rot_deg: float = 3.0, trans: float = 0.02):
    """Ground-truth camera of frame k: a closed smooth loop (rotation <= rot_deg about a fixed axis, translation on a
    small ellipse), so consecutive frames differ by ~2*pi/n_frames of it."""
    a = 2.0 * np.pi * k / n_frames
    axis = np.array([0.4, 0.8, 0.2]) / np.linalg.norm([0.4, 0.8, 0.2])
    rotvec = axis * np.deg2rad(rot_deg) * np.sin(a)
    t = trans * np.array([np.sin(a), 0.5 * (1.0 - np.cos(a)), 0.3 * np.sin(2.0 * a)])
    return rotvec, t


def make_sequence_frame(tmpl: GridTemplate, n_matches: int, k: int, n_frames: int = 100, seq_id: int = 0,
                        init_xyz: np.ndarray | None = None, init_Tcw: np.ndarray | None = None) -> SftFrame:
    """Frame k of a smooth sequence: the bend travels one period over the sequence (phase 2 pi k / n), the camera follows
    sequence_gt_pose, matches are redrawn per frame (problem id = 100000 (seq_id + 1) + k).  init_* = the previous
    frame's result (warm start); None starts from the rest shape / identity like frame 0 of the reference."""
    return make_frame(tmpl, n_matches, 100000 * (seq_id + 1) + k, phase=2.0 * np.pi * k / n_frames - 0.3 * (100000 * (seq_id + 1) + k),
                      init_xyz=init_xyz, init_Tcw=init_Tcw, gt_pose=sequence_gt_pose(k, n_frames))


def make_problem(config: str = "C2", problem_id: int = 0):
    rows, cols, m = CONFIGS[config]
    tmpl = make_grid_template(rows, cols)
    return tmpl, make_frame(tmpl, m, problem_id)


# ---------------------------------------------------------------------------------------------------------
# NRSfM normals: a rigid planar scene seen from several keyframes.  For a plane N.X = 1 (camera-1 frame) the
# inter-image warp in normalised coordinates is the homography (R + t N^T); its first and second derivatives
# are the DiffProp fields (Modules/Mapping/diffProp.h, SchwarpDatabase.cc:299-345).  The geometric normal of
# the plane at (u, v) is k = (N1, N2) / (N.[u,v,1])  (normal ~ [k1, k2, 1 - k1 u - k2 v]).  It is NOT the
# common root of the reference's two bicubic polynomials on these records: the reference forms their t2 from
# the H12vv fields (NormalEstimator.cc:96-97), and the polynomials vanish at k only with t2 from H12uu as in
# its propagation (:210).  tests/normals_geometry.py builds records on which both coincide.
# ---------------------------------------------------------------------------------------------------------
def _homography_derivs(Hm, u, v):
    p = np.array([u, v, 1.0])
    h = Hm @ p
    ha, hb = Hm[:, 0], Hm[:, 1]
    eta = h[:2] / h[2]
    d1 = {}
    for name, hd in (("u", ha), ("v", hb)):
        d1[name] = (hd[:2] * h[2] - h[:2] * hd[2]) / h[2] ** 2
    d2 = {}
    for (na, hd_a), (nb, hd_b) in ((("u", ha), ("u", ha)), (("u", ha), ("v", hb)), (("v", hb), ("v", hb))):
        d2[na + nb] = -(hd_a[:2] * hd_b[2] + hd_b[:2] * hd_a[2]) / h[2] ** 2 + 2 * h[:2] * hd_a[2] * hd_b[2] / h[2] ** 3
    return eta, d1, d2


def make_normals_scene(n_points: int = 200, n_views: int = 4, seed: int = 7, nonref_frac: float = 0.3, min_views: int = 1):
    """Returns a dict with the flat arrays of dsh_normals_estimate plus k_true, the geometric normal (k1,k2) of every point's plane
    (not the root of the reference's polynomials on these records, see above: nothing the reference computes here equals it).
    Every point gets between min_views and n_views records (the reference puts no limit on them, NormalEstimator.cc:77-118)."""
    rng = np.random.default_rng(seed)
    recs, is_ref, first_n, has_first_n, rec_ptr = [], [], [], [], [0]
    x0, has_x0, ref_uv, truth = [], [], [], []
    for p in range(n_points):
        # plane in the reference camera frame: N.X = 1, roughly fronto-parallel at depth ~1
        n = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), 1.0])
        N = n / rng.uniform(0.8, 1.5)
        u, v = rng.uniform(-0.4, 0.4, size=2)
        k_true = N[:2] / (N @ np.array([u, v, 1.0]))
        nv = int(rng.integers(min_views, n_views + 1))
        for _ in range(nv):
            w = rng.normal(size=3)
            w *= rng.uniform(0.03, 0.15) / np.linalg.norm(w)
            R = _rodrigues(w)
            t = rng.uniform(-0.15, 0.15, size=3)
            Hm = R + np.outer(t, N)
            eta, d1, d2 = _homography_derivs(Hm, u, v)
            a, b = d1["u"]      # d eta_u/du, d eta_v/du
            c, d = d1["v"]
            det = a * d - c * b
            rec = [u, v, eta[0], eta[1], a, b, c, d, d / det, -c / det, -b / det, a / det,
                   d2["uu"][0], d2["uu"][1], d2["uv"][0], d2["uv"][1], d2["vv"][0], d2["vv"][1]]
            # J21 fields follow SchwarpDatabase.cc:322-329: J21a = J12d/det, J21b = -J12c/det, J21c = -J12b/det, J21d = J12a/det
            recs.append(rec)
            ref = rng.uniform() >= nonref_frac
            is_ref.append(1 if ref else 0)
            hf = (not ref) and rng.uniform() < 0.7
            has_first_n.append(1 if hf else 0)
            first_n.append(list(k_true + rng.normal(scale=1e-3, size=2)) if hf else [0.0, 0.0])
        rec_ptr.append(len(recs))
        hx = rng.uniform() < 0.5
        has_x0.append(1 if hx else 0)
        x0.append(list(k_true + rng.normal(scale=0.05, size=2)) if hx else [0.0, 0.0])
        ref_uv.append([u, v])
        truth.append(k_true)
    return dict(rec_ptr=np.asarray(rec_ptr, np.int32), recs=np.asarray(recs, np.float32).reshape(-1, 18), rec_is_ref=np.asarray(is_ref, np.uint8),
                rec_first_normal=np.asarray(first_n, np.float32).reshape(-1, 2), rec_has_first_normal=np.asarray(has_first_n, np.uint8),
                x0=np.asarray(x0, np.float32), has_x0=np.asarray(has_x0, np.uint8), ref_uv=np.asarray(ref_uv, np.float32),
                k_true=np.asarray(truth))


# ---------------------------------------------------------------------------------------------------------
# Schwarp fit: matches between two keyframes related by a smooth warp (a homography of a plane plus a gentle
# non-rigid ripple), normalised image coordinates, 13 x 15 control grid as in Thirdparty/BBS/bbs_MAC.h.
# ---------------------------------------------------------------------------------------------------------
def _coloc_dense(umin, umax, nu, vmin, vmax, nv, u, v):
    """Dense colocation matrix of the uniform bicubic B-spline (numpy, for building test inputs only)."""
    def parts(x, xmin, xmax, npts):
        t = (x - xmin) * (npts - 3) / (xmax - xmin)
        i = np.minimum(np.floor(t).astype(int), npts - 4)
        t = t - i
        B = np.stack([(1 - t) ** 3, 3 * t**3 - 6 * t**2 + 4, -3 * t**3 + 3 * t**2 + 3 * t + 1, t**3], 1) / 6.0
        return i, B
    Iu, Bu = parts(np.asarray(u, float), umin, umax, nu)
    Iv, Bv = parts(np.asarray(v, float), vmin, vmax, nv)
    A = np.zeros((len(Iu), nu * nv))
    for a in range(4):
        for b in range(4):
            np.add.at(A, (np.arange(len(Iu)), (Iu + a) * nv + Iv + b), Bu[:, a] * Bv[:, b])
    return A


def make_warp_problem(n_matches: int = 400, seed: int = 3, nu: int = 13, nv: int = 15, noise: float = 5e-4, outliers: float = 0.0, kp1=None, motion=None,
                      fx: float = 520.0, fy: float = 515.0, box=(0.55, 0.42), margin: float = 0.10):
    """One keyframe pair: matches kp1 -> kp2 under a plane-induced homography plus a ripple.  kp1 (given key points of the first keyframe,
    e.g. a subset of one pool shared by several pairs) and motion (rotation vector, translation of the second camera) are optional.
    fx, fy: the focal lengths handed on; box: half extent of the key points drawn here; margin: the domain beyond the key points."""
    rng = np.random.default_rng(seed)
    if kp1 is None:
        kp1 = np.stack([rng.uniform(-box[0], box[0], n_matches), rng.uniform(-box[1], box[1], n_matches)], 1)
    else:
        kp1 = np.asarray(kp1, np.float64).reshape(-1, 2)
        n_matches = kp1.shape[0]
    N = np.array([0.15, -0.1, 1.0]) / 1.1
    rv, tv = motion if motion is not None else (np.array([0.02, -0.05, 0.03]), np.array([0.06, -0.04, 0.02]))
    Hm = _rodrigues(np.asarray(rv, np.float64)) + np.outer(np.asarray(tv, np.float64), N)
    p = np.c_[kp1, np.ones(n_matches)] @ Hm.T
    kp2 = p[:, :2] / p[:, 2:3]
    kp2[:, 0] += 0.01 * np.sin(3.0 * kp1[:, 1])
    kp2 += rng.normal(scale=noise, size=kp2.shape)
    if outliers > 0:
        bad = rng.uniform(size=n_matches) < outliers
        kp2[bad] += rng.uniform(-0.2, 0.2, size=(int(bad.sum()), 2))
    # domain: bounding box of the key points +- 0.10 (DefKeyFrame.cc:116-131)
    umin, umax = float(kp1[:, 0].min() - margin), float(kp1[:, 0].max() + margin)
    vmin, vmax = float(kp1[:, 1].min() - margin), float(kp1[:, 1].max() + margin)
    octave = rng.integers(0, 6, n_matches)
    invsig = np.sqrt((1.2 ** (-2.0 * octave)).astype(np.float32)).astype(np.float32)
    # start: what Warp::initialize hands over (Schwarp.cc:99-160) -- a regularised linear least-squares fit of the control
    # points to the matches; here the regulariser pulls towards the identity map (Greville abscissae).
    C = _coloc_dense(umin, umax, nu, vmin, vmax, nv, kp1[:, 0], kp1[:, 1])
    iu, iv = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    su, sv = (umax - umin) / (nu - 3), (vmax - vmin) / (nv - 3)
    ident = np.stack([(umin + su * (iu - 1)).ravel(), (vmin + sv * (iv - 1)).ravel()], 1)
    mu = 1e-2
    cp = np.linalg.solve(C.T @ C + mu * np.eye(nu * nv), C.T @ kp2 + mu * ident)
    x0 = np.concatenate([cp[:, 0], cp[:, 1]])
    return dict(bbs=(umin, umax, nu, vmin, vmax, nv, 2), kp1=kp1.astype(np.float32), kp2=kp2.astype(np.float32), invsig=invsig, x0=x0,
                fx=float(fx), fy=float(fy))


# ---------------------------------------------------------------------------------------------------------
# Shape from Normals: a smooth depth surface z(u, v) over the normalised image plane; key points with the true
# surface normals (plus noise) as NRSfM would hand them over.  X(u, v) = z (u, v, 1): normal ~ X_u x X_v.
def make_sfn_scene(n_points: int = 600, seed: int = 4, noise: float = 0.01, with_normal_frac: float = 0.8, nu: int = 13, nv: int = 15):
    """nu x nv: the control grid of the depth spline (the reference's 13 x 15 unless a test asks for another one)."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-0.55, 0.55, n_points)
    v = rng.uniform(-0.42, 0.42, n_points)

    def z(u, v):
        return 1.0 + 0.15 * u - 0.1 * v + 0.08 * np.sin(2.5 * u) * np.cos(2.0 * v)

    def zu(u, v):
        return 0.15 + 0.08 * 2.5 * np.cos(2.5 * u) * np.cos(2.0 * v)

    def zv(u, v):
        return -0.1 - 0.08 * 2.0 * np.sin(2.5 * u) * np.sin(2.0 * v)

    d = z(u, v)
    Xu = np.stack([zu(u, v) * u + d, zu(u, v) * v, zu(u, v)], 1)
    Xv = np.stack([zv(u, v) * u, zv(u, v) * v + d, zv(u, v)], 1)
    nrm = np.cross(Xu, Xv)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm += rng.normal(scale=noise, size=nrm.shape)
    has = rng.uniform(size=n_points) < with_normal_frac
    umin, umax = float(u.min() - 0.10), float(u.max() + 0.10)
    vmin, vmax = float(v.min() - 0.10), float(v.max() + 0.10)
    return dict(bbs=(umin, umax, nu, vmin, vmax, nv, 1), u_all=u, v_all=v, depth_true=d, u=u[has], v=v[has], normals=nrm[has].astype(np.float32),
                mean_depth=float(d.mean()))


# ---------------------------------------------------------------------------------------------------------
# Warp-guided match search: keyframe 1 key points (normalised) with ORB-like 256-bit descriptors, a warp, and keyframe 2
# key points scattered around the predictions (pixels) with noisy copies of the descriptors, distractors, exact duplicates
# (distance ties), points that already carry a map point and points outside the image / the grid.
def make_match_scene(n_query: int = 600, n_extra: int = 900, seed: int = 2, nu: int = 13, nv: int = 15, cam2=(520.0, 515.0, 322.5, 241.25),
                     bounds2=(0.0, 640.0, 0.0, 480.0), radius: float = 2.0, box=(0.55, 0.42), near: float = 1.3, twin: float = 0.2, around: float = 20.0):
    """nu x nv: the control grid of the warp that predicts the matches.  cam2, bounds2: the view of keyframe 2; radius: the search radius the
    scene is made for -- candidates lie within near * radius of their prediction, a duplicate within twin * radius of its original;
    box: half extent of the warp's key points (its domain is that + 0.10); around: how far beyond the image the distractors reach."""
    rng = np.random.default_rng(seed)
    pr = make_warp_problem(400, seed + 1, nu, nv, box=box)
    bbs = pr["bbs"][:6] + (2,)
    x = pr["x0"]
    cam2 = np.array(cam2, np.float32)
    bounds2 = np.array(bounds2, np.float32)
    near, twin = near * radius, twin * radius
    lo, hi = bounds2[[0, 2]].astype(np.float64) - around, bounds2[[1, 3]].astype(np.float64) + around
    kp1 = np.stack([rng.uniform(bbs[0] + 0.02, bbs[1] - 0.02, n_query), rng.uniform(bbs[3] + 0.02, bbs[4] - 0.02, n_query)], 1).astype(np.float32)
    # predictions with numpy (double) only to PLACE key points of keyframe 2; the tests compare device and oracle, not this
    C = _coloc_dense(bbs[0], bbs[1], bbs[2], bbs[3], bbs[4], bbs[5], kp1[:, 0].astype(float), kp1[:, 1].astype(float))
    N = bbs[2] * bbs[5]
    pred = np.stack([C @ x[:N], C @ x[N:]], 1)
    pix = pred * cam2[:2] + cam2[2:]
    desc1 = rng.integers(0, 256, (n_query, 32), dtype=np.uint8)
    kp2, desc2 = [], []
    for q in range(n_query):
        k = int(rng.integers(0, 4))                       # 0..3 candidates near the prediction
        for _ in range(k):
            kp2.append(pix[q] + rng.uniform(-near, near, 2))
            d = desc1[q].copy()
            flips = rng.integers(0, 256, int(rng.integers(0, 70)))
            for f in flips:
                d[f // 8] ^= np.uint8(1 << (f % 8))
            desc2.append(d)
        if k and rng.uniform() < 0.25:                    # exact duplicate of the last candidate close by: a distance tie
            kp2.append(kp2[-1] + rng.uniform(-twin, twin, 2))
            desc2.append(desc2[-1].copy())
    kp2 += list(np.stack([rng.uniform(lo[0], hi[0], n_extra), rng.uniform(lo[1], hi[1], n_extra)], 1))
    desc2 += list(rng.integers(0, 256, (n_extra, 32), dtype=np.uint8))
    kp2 = np.asarray(kp2, np.float32)
    desc2 = np.asarray(desc2, np.uint8)
    perm = rng.permutation(kp2.shape[0])
    kp2, desc2 = kp2[perm], desc2[perm]
    has_mp2 = (rng.uniform(size=kp2.shape[0]) < 0.2).astype(np.uint8)
    return dict(bbs=bbs, x=x, kp1=kp1, desc1=desc1, cam2=cam2, bounds2=bounds2, kp2=kp2, desc2=desc2, has_mp2=has_mp2)


# ---------------------------------------------------------------------------------------------------------
# One anchor of SchwarpDatabase::add with every array keyed by key point index: a new keyframe (normalised and pixel key points,
# descriptor rows, octaves) and anchor keyframes whose matched key points (pairs) and searched key points (queries) have a counterpart
# among the new keyframe's key points, placed by make_warp_problem's motion.
def make_warp_pair_scene(n_kp: int = 200, n_pairs: int = 64, n_queries: int = 65, n_anchors: int = 1, seed: int = 0, nu: int = 13, nv: int = 15,
                         outliers: float = 0.0, lost_queries: float = 0.2, views=None):
    """Per anchor: kpn (n_kp,2) float32, desc, octave, the warp grid bbs (nu x nv over the bounding box of its key points +- 0.10),
    pair_idx1 / pair_idx2 and query_idx1 (ascending).  The new keyframe: kpn2, px2 = kpn2 * (fx, fy) + (cx, cy) in float32, desc2,
    octave2; the key points nobody names are distractors.  outliers: share of the pairs whose second key point is moved away;
    lost_queries: share of the queries whose counterpart carries a foreign descriptor.  views: one (K, bounds, grid, scale_factors) per
    anchor and a last one for the new keyframe, instead of one view for all; they come back under "views", the new keyframe's also under
    K, bounds, grid and scale_factors, and every keyframe's octaves lie inside its own table."""
    rng = np.random.default_rng(seed)
    assert n_pairs + n_queries <= n_kp and n_anchors * (n_pairs + n_queries) <= n_kp
    one = ((520.0, 515.0, 322.5, 241.25), (0.0, 640.0, 0.0, 480.0), (64, 48), (1.2 ** np.arange(8)).astype(np.float32))
    assert views is None or len(views) == n_anchors + 1
    K, bounds, grid, sf2 = one if views is None else views[-1]
    f, c0 = np.array(K[:2], np.float32), np.array(K[2:], np.float32)
    px2 = np.stack([rng.uniform(bounds[0] + 5, bounds[1] - 5, n_kp), rng.uniform(bounds[2] + 5, bounds[3] - 5, n_kp)], 1).astype(np.float32)
    # the anchors' key points: the usual box, or with views what the new keyframe sees of it (a little more: some predictions leave its image)
    box = (0.55, 0.42) if views is None else tuple(float(0.5 * (bounds[2 * i + 1] - bounds[2 * i]) / K[i]) for i in range(2))
    kpn2 = ((px2 - c0) / f).astype(np.float32)
    desc2 = rng.integers(0, 256, (n_kp, 32), dtype=np.uint8)
    free = list(rng.permutation(n_kp))
    anchors = []
    for a in range(n_anchors):
        kpn = np.stack([rng.uniform(-box[0], box[0], n_kp), rng.uniform(-box[1], box[1], n_kp)], 1).astype(np.float32)
        pr = make_warp_problem(seed=seed + 10 * a + 1, nu=nu, nv=nv, kp1=kpn.astype(np.float64),
                               motion=(np.array([0.02, -0.05, 0.03]) * (1 + a), np.array([0.06, -0.04, 0.02]) * (1 - 0.5 * a)))
        desc = rng.integers(0, 256, (n_kp, 32), dtype=np.uint8)
        sel = rng.permutation(n_kp)[:n_pairs + n_queries]
        idx2 = np.array([free.pop() for _ in sel], np.int32)
        tgt = pr["kp2"][sel].astype(np.float32)
        moved = rng.uniform(size=len(sel)) < outliers
        moved[n_pairs:] = False
        tgt[moved] += rng.uniform(-0.2, 0.2, size=(int(moved.sum()), 2)).astype(np.float32)
        kpn2[idx2] = tgt
        px2[idx2] = (tgt * f + c0).astype(np.float32)
        for k, (i1, i2) in enumerate(zip(sel, idx2)):
            lost = k >= n_pairs and rng.uniform() < lost_queries
            desc2[i2] = rng.integers(0, 256, 32, dtype=np.uint8) if lost else _flip_bits(rng, desc[i1], rng.integers(0, 40))
        order = np.argsort(sel[n_pairs:])
        levels = 8 if views is None else len(views[a][3])
        anchors.append(dict(kpn=kpn, desc=desc, octave=rng.integers(0, levels, n_kp).astype(np.int32), bbs=pr["bbs"][:6] + (2,),
                            pair_idx1=sel[:n_pairs].astype(np.int32), pair_idx2=idx2[:n_pairs].copy(),
                            query_idx1=sel[n_pairs:][order].astype(np.int32), query_idx2=idx2[n_pairs:][order].copy()))
    sc = dict(seed=seed, K=K, bounds=bounds, grid=grid, scale_factors=np.asarray(sf2, np.float32), anchors=anchors,
              kpn2=kpn2, px2=px2, desc2=desc2, octave2=rng.integers(0, len(sf2), n_kp).astype(np.int32), lam=1e-2)
    if views is not None:
        sc["views"] = [(tuple(float(v) for v in k), tuple(float(v) for v in b), tuple(g), np.asarray(t, np.float32)) for k, b, g, t in views]
    return sc


def make_register_scene(n: int = 600, seed: int = 5, noise: float = 2e-3, outliers: float = 0.05, scale: float = 1.35):
    """Surface registration (SurfaceRegistration::registerSurfaces): a keyframe surface (up to scale, in world coordinates) and
    the map points it has to be aligned with, the keyframe's inverse pose and a stream of uniform numbers for scaleMinMedian."""
    rng = np.random.default_rng(seed)
    surf = np.stack([rng.uniform(-0.4, 0.4, n), rng.uniform(-0.3, 0.3, n), 1.0 + 0.15 * rng.standard_normal(n)], 1)
    R = _rodrigues(np.array([0.02, -0.035, 0.015]))
    t = np.array([0.03, -0.02, 0.05])
    mp = scale * (surf @ R.T) + t + noise * rng.standard_normal((n, 3))
    bad = rng.random(n) < outliers
    mp[bad] += 0.2 * rng.standard_normal((int(bad.sum()), 3))
    Rwc = _rodrigues(np.array([0.1, 0.05, -0.07]))
    Twc = np.eye(4, dtype=np.float32)
    Twc[:3, :3] = Rwc.astype(np.float32)
    Twc[:3, 3] = np.array([0.2, -0.1, 0.3], np.float32)
    u = rng.random(n + n * n)
    return dict(surface=surf.astype(np.float32), map=mp.astype(np.float32), Twc=Twc, u=u, scale=scale, R=R, t=t, outlier=bad)


# ---------------------------------------------------------------------------------------------------------
# One coherent mapping scene for the chained NRSfM loop (DefLocalMapping::NRSfM, DefLocalMapping.cc:160-234 and
# SchwarpDatabase::add): a smooth surface seen from a reference keyframe and `n_kf - 1` later keyframes.  Key points of
# the reference keyframe carry ORB-like descriptors; the first `n_tracked` of them are already matched in the later
# keyframes (tracked map points), the others are what the warp-guided search has to find.
# ---------------------------------------------------------------------------------------------------------
def make_mapping_scene(n_points: int = 520, n_tracked: int = 380, n_kf: int = 3, seed: int = 11, scale_true: float = 1.3):
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = 520.0, 515.0, 322.5, 241.25
    u = rng.uniform(-0.5, 0.5, n_points)
    v = rng.uniform(-0.38, 0.38, n_points)
    depth = 1.0 + 0.12 * u - 0.08 * v + 0.05 * np.sin(2.0 * u) * np.cos(1.5 * v)
    X = np.stack([u * depth, v * depth, depth], 1)                      # reference camera frame
    desc0 = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    octave = rng.integers(0, 6, n_points)
    invsig = np.sqrt((1.2 ** (-2.0 * octave)).astype(np.float32)).astype(np.float32)
    kfs = []
    for j in range(1, n_kf):
        R = _rodrigues(np.array([0.03 * j, -0.05 * j, 0.02]) * (1.0 + 0.1 * rng.standard_normal()))
        t = np.array([0.05 * j, -0.03 * j, 0.02 * j])
        Xc = X @ R.T + t
        kp = Xc[:, :2] / Xc[:, 2:3] + rng.normal(scale=3e-4, size=(n_points, 2))
        pix = kp * np.array([fx, fy]) + np.array([cx, cy])
        desc = desc0.copy()
        for i in range(n_points):                                      # noisy copies: a few flipped bits
            for f in rng.integers(0, 256, int(rng.integers(0, 24))):
                desc[i, f // 8] ^= np.uint8(1 << (f % 8))
        n_extra = 300                                                   # distractors without a counterpart
        pix_all = np.vstack([pix, np.stack([rng.uniform(0, 640, n_extra), rng.uniform(0, 480, n_extra)], 1)])
        desc_all = np.vstack([desc, rng.integers(0, 256, (n_extra, 32), dtype=np.uint8)])
        perm = rng.permutation(pix_all.shape[0])
        inv = np.empty_like(perm)
        inv[perm] = np.arange(perm.shape[0])
        has_mp = np.zeros(pix_all.shape[0], np.uint8)
        has_mp[inv[:n_tracked]] = 1                                     # tracked map points already own their key point
        kfs.append(dict(R=R, t=t, kp_norm=kp.astype(np.float32), pix=pix_all[perm].astype(np.float32), desc=desc_all[perm], index_of_point=inv[:n_points],
                        has_mp=has_mp))
    umin, umax = float(u.min() - 0.10), float(u.max() + 0.10)
    vmin, vmax = float(v.min() - 0.10), float(v.max() + 0.10)
    # the keyframe's pose in the map and the map points the surface is registered against (another scale, small noise)
    Rwc = _rodrigues(np.array([0.06, 0.03, -0.04]))
    Twc = np.eye(4, dtype=np.float32)
    Twc[:3, :3] = Rwc.astype(np.float32)
    Twc[:3, 3] = np.array([0.1, -0.05, 0.2], np.float32)
    Xw = scale_true * (X @ Rwc.T) + Twc[:3, 3].astype(np.float64)
    map_pts = (Xw + 1e-3 * rng.standard_normal(Xw.shape)).astype(np.float32)
    return dict(bbs2=(umin, umax, 13, vmin, vmax, 15, 2), bbs1=(umin, umax, 13, vmin, vmax, 15, 1), kp0=np.stack([u, v], 1).astype(np.float32), desc0=desc0,
                invsig=invsig, depth=depth, X=X, kfs=kfs, n_tracked=n_tracked, cam=np.array([fx, fy, cx, cy], np.float32),
                bounds=np.array([0.0, 640.0, 0.0, 480.0], np.float32), Twc=Twc, map_pts=map_pts, scale_true=scale_true,
                u_stream=rng.random(n_points + n_points * n_points))


# ---------------------------------------------------------------------------------------------------------
# SEQMAP (BASELINE.json configs[2] substitute, whole: deformable tracking AND NRSfM mapping in one sequence).
# The reference interleaves the two (DefTracking.cc:109-115,175; DefLocalMapping.cc:138-153,172-234): every
# 10th frame becomes a keyframe, the mapping side fits a Schwarzian warp from the anchor keyframe to it,
# re-estimates the normals of the anchor's map points, integrates them to a surface, registers the surface to
# the map and hands tracking a NEW template; the next frame is solved against it with RegTemp = 0.
# Scene: the anchor keyframe sees a smooth surface; it deforms slowly (a travelling bump along the normal
# direction) while the camera moves; all keyframes observe the same physical points.
# ---------------------------------------------------------------------------------------------------------
SEQMAP = dict(n_frames=41, kf_every=10, n_points=520, n_tracked=380, seed=17, scale_true=1.3, mesh=(12, 14))


def make_interleaved_sequence(n_frames: int = 41, kf_every: int = 10, n_points: int = 520, n_tracked: int = 380, seed: int = 17, scale_true: float = 1.3,
                              mesh=(12, 14)):
    """Everything the tracking + mapping loop consumes, frame by frame (ground truth included for plausibility checks only)."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = 520.0, 515.0, 322.5, 241.25
    u = rng.uniform(-0.5, 0.5, n_points)
    v = rng.uniform(-0.38, 0.38, n_points)

    def depth_of(uu, vv):
        return 1.0 + 0.12 * uu - 0.08 * vv + 0.05 * np.sin(2.0 * uu) * np.cos(1.5 * vv)

    depth = depth_of(u, v)
    X0 = np.stack([u * depth, v * depth, depth], 1)                     # anchor keyframe's camera frame, unit scale
    desc0 = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    octave = rng.integers(0, 6, n_points)
    invsig = np.sqrt((1.2 ** (-2.0 * octave)).astype(np.float32)).astype(np.float32)
    Rwc = _rodrigues(np.array([0.06, 0.03, -0.04]))
    Twc = np.eye(4, dtype=np.float32)
    Twc[:3, :3] = Rwc.astype(np.float32)
    Twc[:3, 3] = np.array([0.1, -0.05, 0.2], np.float32)
    twc = Twc[:3, 3].astype(np.float64)

    def to_world(Xa):                                                   # anchor frame (unit scale) -> world (map scale)
        return scale_true * (Xa @ Rwc.T) + twc

    def deformed(Xa, uu, vv, k):                                        # the surface at frame k: a slow travelling bump along the optical axis
        a = 0.012 * k / max(n_frames - 1, 1)
        out = Xa.copy()
        out[:, 2] += a * np.sin(3.0 * uu + 0.08 * k) * np.cos(2.0 * vv)
        return out

    Rcw0 = Rwc.T
    tcw0 = -Rcw0 @ twc
    frames = []
    for k in range(n_frames):
        dR = _rodrigues(np.array([0.004 * k, -0.006 * k, 0.002 * k]))
        Rk = dR @ Rcw0
        tk = dR @ tcw0 + scale_true * np.array([0.006 * k, -0.004 * k, 0.003 * k])
        T = np.eye(4)
        T[:3, :3] = Rk
        T[:3, 3] = tk
        Xw = to_world(deformed(X0, u, v, k))
        Xc = Xw @ Rk.T + tk
        frames.append(dict(Tcw_gt=T, Xw=Xw, Xc=Xc))
    kfs = {}
    # key -1: the keyframe the map was bootstrapped with before the sequence starts (a second view of the undeformed surface with a
    # decent baseline: one warp alone leaves the normals of the anchor poorly constrained); keys k = kf_every, 2 kf_every, ...: the sequence's own
    Rb = _rodrigues(np.array([0.06, -0.10, 0.02]))
    Xc_boot = X0 @ Rb.T + np.array([0.10, -0.06, 0.04])
    for k in [-1] + list(range(kf_every, n_frames, kf_every)):          # the keyframes' own measurements of the anchor's points
        Xc = Xc_boot if k < 0 else frames[k]["Xc"]
        kp = Xc[:, :2] / Xc[:, 2:3] + rng.normal(scale=3e-4, size=(n_points, 2))
        pix = kp * np.array([fx, fy]) + np.array([cx, cy])
        desc = desc0.copy()
        for i in range(n_points):
            for f in rng.integers(0, 256, int(rng.integers(0, 24))):
                desc[i, f // 8] ^= np.uint8(1 << (f % 8))
        n_extra = 300
        pix_all = np.vstack([pix, np.stack([rng.uniform(0, 640, n_extra), rng.uniform(0, 480, n_extra)], 1)])
        desc_all = np.vstack([desc, rng.integers(0, 256, (n_extra, 32), dtype=np.uint8)])
        perm = rng.permutation(pix_all.shape[0])
        inv = np.empty_like(perm)
        inv[perm] = np.arange(perm.shape[0])
        has_mp = np.zeros(pix_all.shape[0], np.uint8)
        has_mp[inv[:n_tracked]] = 1
        kfs[k] = dict(kp_norm=kp.astype(np.float32), pix=pix_all[perm].astype(np.float32), desc=desc_all[perm], index_of_point=inv[:n_points], has_mp=has_mp,
                      u_stream=rng.random(n_points + n_points * n_points))
    umin, umax = float(u.min() - 0.10), float(u.max() + 0.10)
    vmin, vmax = float(v.min() - 0.10), float(v.max() + 0.10)
    # the first template (what MonocularInitialization + the first mapping pass leave behind): the anchor's true surface on a regular grid
    rows, cols = mesh
    gu, gv = np.meshgrid(np.linspace(u.min(), u.max(), cols), np.linspace(v.min(), v.max(), rows))
    gd = depth_of(gu.ravel(), gv.ravel())
    nodes0 = to_world(np.stack([gu.ravel() * gd, gv.ravel() * gd, gd], 1))
    noise = rng.normal(scale=0.4, size=(n_frames, n_points, 2))        # pixel noise of the tracked observations
    return dict(bbs2=(umin, umax, 13, vmin, vmax, 15, 2), bbs1=(umin, umax, 13, vmin, vmax, 15, 1), kp0=np.stack([u, v], 1).astype(np.float32), desc0=desc0,
                invsig=invsig, depth=depth, X0=X0, frames=frames, kfs=kfs, n_tracked=n_tracked, cam=np.array([fx, fy, cx, cy], np.float32),
                bounds=np.array([0.0, 640.0, 0.0, 480.0], np.float32), Twc=Twc, scale_true=scale_true, nodes0=nodes0, mesh=mesh, grid_uv=(gu, gv),
                facets=regular_triangulation(rows, cols), noise=noise, n_frames=n_frames, kf_every=kf_every)


# ---------------------------------------------------------------------------------------------------------
# Tracking searches (defslam_amd/track.py): a current frame with ORB-like key points around the projections of map points
# embedded in a deformed template, the last frame's map points (frame-to-frame queries) and local map points with normals.
# ---------------------------------------------------------------------------------------------------------
def _flip_bits(rng, d, n):
    d = d.copy()
    for f in rng.choice(256, size=int(n), replace=False):
        d[f // 8] ^= np.uint8(1 << (f % 8))
    return d


def make_track_scene(seed: int = 0, n_kp: int = 1200, n_frame_q: int = 400, n_local_q: int = 300, mappoint_xyz=None, Tcw=None,
                     levels: int = 8, adversarial: bool = True, state_mix: bool = False, n_clusters: int = 6,
                     camera=CAMERA_K, bounds=(0.0, IMAGE_SIZE[0], 0.0, IMAGE_SIZE[1]), scale: float = 1.0):
    """One current frame and the queries of both searches (returns dict(frame=track.TrackFrame, fq=FrameQueries, lq=LocalQueries,
    point_xyz, kp_of_point)).  Map points: float32 positions on a bent 10 x 10 template (or mappoint_xyz, e.g. a
    dsh_sft_result.mappoint_xyz, so that SfT(t) -> search(t+1) -> SfT(t+1) can be chained); the current pose moves slightly away
    from Tcw (identity when None), which is the pose the searches project with.  Key points: one per map point near its projection
    (descriptor = the point's with a few flipped bits, octave drawn around the point's), distractors, exact duplicates (distance
    ties) and, with adversarial, clusters of near-identical key points that several queries want (in-call conflicts that exhaust a
    query's stored keys).  Local points get normals with viewCos spread over [0.3, 1] and max distances that put the predicted level
    0.1 .. 0.9 of a level away from a boundary; viewCos is kept 1e-3 away from 0.5 and 0.998.  state_mix draws key point states
    0 / 1 / 2 (otherwise all 0).  camera = (fx, fy, cx, cy); bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY), the undistorted image area (its
    minima may be negative); scale is the scene scale: depth and bend of the template and the camera's translation."""
    from . import track
    rng = np.random.default_rng(1000 + seed)
    fx, fy, cx, cy = camera
    K = np.array(camera, np.float32)
    x_lo, x_hi, y_lo, y_hi = (float(b) for b in bounds)
    bounds = np.array([x_lo, x_hi, y_lo, y_hi], np.float32)
    sf, logsf = track.orb_pyramid(levels)
    T0 = np.eye(4, dtype=np.float32) if Tcw is None else np.asarray(Tcw, np.float32)
    if mappoint_xyz is None:
        tmpl = make_grid_template(10, 10, seed=1234 + seed, z0=scale, camera=(fx, fy, cx - x_lo, cy - y_lo), image_size=(x_hi - x_lo, y_hi - y_lo))
        n_pts = max(n_frame_q, n_local_q) + 50
        fac = rng.integers(0, tmpl.facets.shape[0], n_pts)
        bary = rng.dirichlet((1.0, 1.0, 1.0), n_pts)
        gt = tmpl.xyz0.copy()
        gt[:, 2] += (0.05 * scale) * np.sin(2 * np.pi * (gt[:, 0] - gt[:, 0].min()) / np.ptp(gt[:, 0]) + 0.3 * seed)
        pts = (bary[:, :, None] * gt[tmpl.facets[fac]]).sum(1).astype(np.float32)
    else:
        pts = np.asarray(mappoint_xyz, np.float32).reshape(-1, 3)
    P = pts.shape[0]
    # the current frame's pose: a small motion away from T0 (float32, as cv::Mat mTcw)
    dT = np.eye(4)
    dT[:3, :3] = _rodrigues(rng.normal(size=3) * 0.004)
    dT[:3, 3] = rng.uniform(-0.004, 0.004, 3) * scale
    Tc = (dT @ T0.astype(np.float64)).astype(np.float32)
    Ow = track.camera_center(Tc)
    Xc = pts.astype(np.float64) @ Tc[:3, :3].astype(np.float64).T + Tc[:3, 3].astype(np.float64)
    uv = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)
    pdesc = rng.integers(0, 256, (P, 32), dtype=np.uint8)
    poct = rng.integers(0, levels - 2, P)
    kp, koct, kdesc, kp_of_point = [], [], [], np.full(P, -1, np.int64)
    for i in range(P):
        if rng.uniform() < 0.1:                                   # not detected in this frame
            continue
        kp_of_point[i] = len(kp)
        kp.append(uv[i] + rng.uniform(-1.5, 1.5, 2))
        koct.append(int(np.clip(poct[i] + rng.integers(-1, 2), 0, levels - 1)))
        kdesc.append(_flip_bits(rng, pdesc[i], rng.integers(0, 40)))
        if rng.uniform() < 0.15:                                  # a near-identical second detection: distance tie
            kp.append(kp[-1] + rng.uniform(-0.5, 0.5, 2))
            koct.append(koct[-1])
            kdesc.append(kdesc[-1].copy())
        if rng.uniform() < 0.3:                                   # a close distractor
            kp.append(uv[i] + rng.uniform(-6, 6, 2))
            koct.append(int(rng.integers(0, levels)))
            kdesc.append(_flip_bits(rng, pdesc[i], rng.integers(10, 90)))
    clusters = []
    if adversarial:
        for c in range(n_clusters):                               # several queries want the same few key points
            i = int(rng.integers(0, P))
            clusters.append(i)
            for _ in range(8):
                kp.append(uv[i] + rng.uniform(-1.0, 1.0, 2))
                koct.append(int(np.clip(poct[i], 0, levels - 1)))
                kdesc.append(_flip_bits(rng, pdesc[i], rng.integers(0, 12)))
    n_extra = max(0, n_kp - len(kp))
    kp += list(np.stack([rng.uniform(x_lo - 5, x_hi + 5, n_extra), rng.uniform(y_lo - 5, y_hi + 5, n_extra)], 1))
    koct += list(rng.integers(0, levels, n_extra))
    kdesc += list(rng.integers(0, 256, (n_extra, 32), dtype=np.uint8))
    kp = np.asarray(kp, np.float32)
    koct = np.asarray(koct, np.int32)
    kdesc = np.asarray(kdesc, np.uint8)
    perm = rng.permutation(kp.shape[0])
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.shape[0])
    kp, koct, kdesc = kp[perm], koct[perm], kdesc[perm]
    kp_of_point = np.where(kp_of_point >= 0, inv[np.maximum(kp_of_point, 0)], -1)
    N = kp.shape[0]
    state = np.zeros(N, np.uint8)
    if state_mix:
        state = rng.choice(np.array([0, 1, 2], np.uint8), N, p=[0.7, 0.15, 0.15])
    frame = track.TrackFrame(Tcw=Tc, K=K, bounds=bounds, kp=kp, octave=koct, desc=kdesc, scale_factors=sf, log_scale_factor=float(logsf),
                             state=state, Ow=Ow)
    # frame-to-frame queries: map points in the last frame's index order, conflicts included (the cluster points repeat)
    order = rng.permutation(P)
    qi = np.concatenate([order[:n_frame_q], np.repeat(np.asarray(clusters, np.int64), 3)]) if n_frame_q else np.zeros(0, np.int64)
    rng.shuffle(qi)
    fq = track.FrameQueries(xyz=pts[qi], octave=np.clip(poct[qi], 0, levels - 1).astype(np.int32), desc=pdesc[qi])
    # local points: normals and max distances around the thresholds' safe sides
    li = np.concatenate([order[::-1][:n_local_q], np.repeat(np.asarray(clusters, np.int64), 3)]) if n_local_q else np.zeros(0, np.int64)
    rng.shuffle(li)
    L = li.shape[0]
    PO = pts[li].astype(np.float64) - Ow.astype(np.float64)
    dist = np.linalg.norm(PO, axis=1) if L else np.zeros(0)
    dirn = PO / np.maximum(dist[:, None], 1e-12)
    normals = np.zeros((L, 3), np.float32)
    maxd = np.zeros(L, np.float32)
    for k in range(L):
        while True:
            target = rng.choice([rng.uniform(0.3, 0.997), rng.uniform(0.9985, 1.0)])
            w = rng.normal(size=3)
            w -= w.dot(dirn[k]) * dirn[k]
            w /= np.linalg.norm(w)
            n = target * dirn[k] + np.sqrt(max(0.0, 1 - target * target)) * w
            n = n.astype(np.float32)
            vc = float(PO[k].dot(n.astype(np.float64)) / dist[k])
            if abs(vc - 0.5) > 1e-3 and abs(vc - 0.998) > 1e-3:
                break
        normals[k] = n
        lev = rng.integers(-1, levels + 1) + rng.uniform(0.1, 0.9)
        maxd[k] = np.float32(dist[k] * 1.2 ** lev)
    skip = (rng.uniform(size=L) < 0.05).astype(np.uint8)
    lq = track.LocalQueries(xyz=pts[li], normal=normals, max_distance=maxd, desc=pdesc[li], skip=skip)
    return dict(frame=frame, fq=fq, lq=lq, point_xyz=pts, kp_of_point=kp_of_point, frame_points=qi, local_points=li)


# ---------------------------------------------------------------------------------------------------------
# Local map (defslam_amd/localmap.py): a map of keyframes along a camera path over a surface -- point tables, observations, a
# spanning tree, bad flags -- and a current frame that already holds the matches of the frame-to-frame search.
# ---------------------------------------------------------------------------------------------------------
def make_local_map_scene(seed: int = 0, n_kf: int = 30, n_kp: int = 1200, obs_per_point: int = 8, n_frame_kp: int = 1200, fill: float = 0.7,
                         bad_kf_frac: float = 0.07, bad_point_frac: float = 0.02):
    """A map and a current frame (returns a dict).  Map: P = n_kf * n_kp * fill / obs_per_point points on a bent template (xyz, normal,
    max_distance, desc, bad); point p is seen by a run of about obs_per_point consecutive keyframes of the path, in each at a random
    key point: tables[k] (n_kp ids or -1) and the observation pairs (obs_point, obs_kf), shuffled.  parents: a chain with branches
    (parents[0] = -1); kf_bad / bad: a few bad keyframes and points.  The LAST keyframe is in the window between CreateNewKeyFrame and
    ProcessNewKeyFrame: its table is filled, its observations are not there yet.  Frame: a track.TrackFrame near the end of the path whose
    key points were generated around the projections of the most recently seen points; frame_points (N ids or -1) holds what the
    frame-to-frame search would have matched -- most of those points at their own key point, a few of them at a second key point as
    well (they vote twice), some bad points among them -- and frame.state is 1 where a point is held.  Also what the points were drawn
    from: template (the GridTemplate), template_xyz (its bent nodes), facet and facet_bary per point."""
    from . import track
    rng = np.random.default_rng(7000 + seed)
    P = max(8, int(n_kf * n_kp * fill / obs_per_point))
    tmpl = make_grid_template(10, 10, seed=1234 + seed)
    gt = tmpl.xyz0.copy()
    gt[:, 2] += 0.05 * np.sin(2 * np.pi * (gt[:, 0] - gt[:, 0].min()) / np.ptp(gt[:, 0]) + 0.3 * seed)
    fac = rng.integers(0, tmpl.facets.shape[0], P)
    bary = rng.dirichlet((1.0, 1.0, 1.0), P)
    xyz = (bary[:, :, None] * gt[tmpl.facets[fac]]).sum(1).astype(np.float32)
    # who sees whom: point p by keyframes first[p] .. first[p] + run[p] - 1; points sorted by first so that ids follow the path
    run = np.clip(rng.integers(max(1, obs_per_point // 2), obs_per_point + obs_per_point // 2 + 1, P), 1, n_kf)
    first = np.sort(rng.integers(0, np.maximum(n_kf - run // 2, 1), P))
    first = np.minimum(first, n_kf - 1)
    tables = np.full((n_kf, n_kp), -1, np.int32)
    obs_point, obs_kf = [], []
    for k in range(n_kf):
        seen = np.nonzero((first <= k) & (k < first + run))[0]
        if seen.shape[0] > int(0.9 * n_kp):
            seen = np.sort(rng.choice(seen, int(0.9 * n_kp), replace=False))
        tables[k, rng.choice(n_kp, seen.shape[0], replace=False)] = seen
        if k < n_kf - 1:                                           # the last keyframe's observations are still to come
            obs_point.append(seen)
            obs_kf.append(np.full(seen.shape[0], k))
    obs_point = np.concatenate(obs_point).astype(np.int32) if obs_point else np.zeros(0, np.int32)
    obs_kf = np.concatenate(obs_kf).astype(np.int32) if obs_kf else np.zeros(0, np.int32)
    perm = rng.permutation(obs_point.shape[0])
    obs_point, obs_kf = obs_point[perm], obs_kf[perm]
    parents = np.arange(-1, n_kf - 1, dtype=np.int32)
    for k in range(2, n_kf):
        if rng.uniform() < 0.15:
            parents[k] = rng.integers(0, k - 1)
    kf_bad = np.zeros(n_kf, bool)                                  # a few of each, at least one (never the root keyframe)
    if n_kf > 1:
        kf_bad[rng.choice(np.arange(1, n_kf), min(n_kf - 1, max(1, int(round(bad_kf_frac * n_kf)))), replace=False)] = True
    bad = np.zeros(P, bool)
    bad[rng.choice(P, max(1, int(round(bad_point_frac * P))), replace=False)] = True
    # the current frame: key points around the most recently seen points
    recent = np.nonzero(first + run >= n_kf - 2)[0]
    n_vis = max(4, min(recent.shape[0], int(0.45 * n_frame_kp)))
    vis = np.sort(rng.choice(recent, n_vis, replace=False)) if recent.shape[0] > n_vis else (recent if recent.shape[0] >= 4 else np.arange(P - 4, P))
    ts = make_track_scene(seed, n_kp=n_frame_kp, n_frame_q=0, n_local_q=vis.shape[0], mappoint_xyz=xyz[vis], adversarial=False)
    frame = ts["frame"]
    Ow = np.asarray(frame.Ow, np.float64)
    PO = xyz.astype(np.float64) - Ow
    dist = np.linalg.norm(PO, axis=1)
    nrm = PO / dist[:, None] + 0.3 * rng.normal(size=(P, 3))
    normal = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(np.float32)
    max_distance = (dist * 1.2 ** rng.uniform(0.1, 6.9, P)).astype(np.float32)
    desc = rng.integers(0, 256, (P, 32), dtype=np.uint8)
    lq, li = ts["lq"], ts["local_points"]
    for q in range(li.shape[0]):                                   # the visible points take the scene's normals, depths and descriptors
        p = vis[li[q]]
        normal[p], max_distance[p], desc[p] = lq.normal[q], lq.max_distance[q], lq.desc[q]
    N = np.asarray(frame.kp).reshape(-1, 2).shape[0]
    frame_points = np.full(N, -1, np.int32)
    kp_of = ts["kp_of_point"]
    for i in range(vis.shape[0]):
        if kp_of[i] >= 0 and rng.uniform() < 0.6:                  # matched by the frame-to-frame search
            frame_points[kp_of[i]] = vis[i]
    free = np.nonzero(frame_points < 0)[0]
    held = frame_points[frame_points >= 0]
    if held.shape[0] and free.shape[0]:
        twice = rng.choice(held, min(5, held.shape[0]), replace=False)
        frame_points[rng.choice(free, twice.shape[0], replace=False)] = twice
        bad[rng.choice(held, min(3, held.shape[0]), replace=False)] = True
    state = (frame_points >= 0).astype(np.uint8)
    frame = track.TrackFrame(**{**frame.__dict__, "state": state})
    return dict(xyz=xyz, normal=normal, max_distance=max_distance, desc=desc, bad=bad, tables=tables, parents=parents, kf_bad=kf_bad,
                obs_point=obs_point, obs_kf=obs_kf, frame=frame, frame_points=frame_points,
                template=tmpl, template_xyz=gt, facet=fac, facet_bary=bary)


def write_local_map_scene(sc, path):
    """A make_local_map_scene dict as the text file integration/localmap_shim_test_main.cc reads (floats by repr: they round-trip)."""
    tf = sc["frame"]
    a = tf.arrays()
    fl = lambda vs: " ".join(repr(float(v)) for v in vs)
    by = lambda row: " ".join(str(int(b)) for b in row)
    P, K, N = sc["xyz"].shape[0], sc["tables"].shape[0], a["kp"].shape[0]
    with open(path, "w") as f:
        f.write(f"{a['sf'].shape[0]} {float(np.float32(tf.log_scale_factor))!r}\n{fl(a['sf'])}\n{P}\n")
        for p in range(P):
            f.write(f"{fl(sc['xyz'][p])} {fl(sc['normal'][p])} {float(sc['max_distance'][p])!r} {int(sc['bad'][p])} {by(sc['desc'][p])}\n")
        f.write(f"{K}\n")
        for k in range(K):
            f.write(f"{int(sc['parents'][k])} {int(sc['kf_bad'][k])} {sc['tables'].shape[1]} {by(sc['tables'][k])}\n")
        f.write(f"{sc['obs_point'].shape[0]}\n" + "".join(f"{int(p)} {int(k)}\n" for p, k in zip(sc["obs_point"], sc["obs_kf"])))
        f.write(f"{fl(a['K'])} {fl(a['bounds'])}\n{fl(a['Tcw'].ravel())}\n{fl(a['Ow'])}\n{N}\n")
        for j in range(N):
            f.write(f"{float(a['kp'][j, 0])!r} {float(a['kp'][j, 1])!r} {int(a['octave'][j])} {int(sc['frame_points'][j])} {by(a['desc'][j])}\n")


# ---------------------------------------------------------------------------------------------------------
# Closing a tracked frame (MapPointStore.close_frame / repose / cull): a local-map scene with the template embedding of its points
# and the state of the frame after the pose optimisation.
# ---------------------------------------------------------------------------------------------------------
def make_track_close_scene(seed: int = 0, no_facet_frac: float = 0.15, away_frac: float = 0.1, outlier_frac: float = 0.15, **local_map):
    """make_local_map_scene(seed, **local_map) (its keys are kept; normal and the observations differ, see below) plus
      nodes (P,3) int32 / bary (P,3) float64   the facet of every point as ascending node indices with the barycentrics in that order;
                                               a share no_facet_frac has none (-1 -1 -1, zeros)
      normal                                   a share away_frac of the points looks away from the camera (normal negated): not in the frustum
      obs_point, obs_kf                        without the pairs of up to three points, which the final frame holds: n_obs == 0
      late_bad                                 ids that become bad after the previous frame built its local list (they sit in the reference list)
      visible (P,), found (P,)                 mnVisible / mnFound of a loaded map (found <= visible; some ratios below 0.40)
      first_kf (P,), current_kf                mnFirstKFid per point and the id of the keyframe LocalMapping::MapPointCulling runs for
      node_xyz (n,3) float64, frame_after      the template nodes and the frame "after the optimisation": the nodes moved by a few millimetres,
                                               a slightly different pose (only Tcw and Ow differ from frame)
      final_points (N,), outlier (N,)          mvpMapPoints / mvbOutlier after the local-map search and the optimisation.  Among the held points:
                                               one held twice and inlier at both key points, bad ones, points without an observation
                                               (n_obs == 0), one without a facet."""
    from . import track
    sc = dict(make_local_map_scene(seed, **local_map))
    rng = np.random.default_rng(9000 + seed)
    P = sc["xyz"].shape[0]
    tmpl = sc["template"]
    raw = tmpl.facets[sc["facet"]].astype(np.int32)
    order = np.argsort(raw, axis=1, kind="stable")                 # std::set<Node*> order
    nodes = np.take_along_axis(raw, order, 1)
    bary = np.take_along_axis(np.asarray(sc["facet_bary"], np.float64), order, 1)
    fp0 = sc["frame_points"]
    N = fp0.shape[0]
    held0 = np.unique(fp0[fp0 >= 0])
    n_obs = np.bincount(sc["obs_point"], minlength=P)
    bad = sc["bad"]
    free_pts = np.setdiff1d(np.nonzero(~bad)[0], held0)
    # the final frame: the bad entries are nulled (Tracking.cc:1527-1530) but for one; the local-map search adds matches; some points
    # without an observation come in (they sit in the newest keyframe's table only)
    final = fp0.copy()
    bad_at = np.nonzero((fp0 >= 0) & bad[np.maximum(fp0, 0)])[0]
    final[bad_at[1:]] = -1
    free_kp = np.nonzero(final < 0)[0]
    rng.shuffle(free_kp)
    zero_obs = rng.choice(free_pts, min(3, free_pts.shape[0]), replace=False)      # created by the tracking, not yet seen by a keyframe
    keep_obs = ~np.isin(sc["obs_point"], zero_obs)
    sc["obs_point"], sc["obs_kf"] = sc["obs_point"][keep_obs], sc["obs_kf"][keep_obs]
    n_obs[zero_obs] = 0
    more = rng.choice(np.setdiff1d(free_pts, zero_obs), min(max(1, free_kp.shape[0] // 4), max(free_pts.shape[0] - 3, 1)), replace=False) \
        if free_pts.shape[0] > 3 else np.zeros(0, np.int64)
    new = np.concatenate([zero_obs, more])[:free_kp.shape[0]]
    final[free_kp[:new.shape[0]]] = new
    outlier = ((final >= 0) & (rng.uniform(size=N) < outlier_frac)).astype(np.uint8)
    vals, counts = np.unique(final[final >= 0], return_counts=True)
    twice = [int(p) for p in vals[counts >= 2] if not bad[p] and n_obs[p] > 0]
    if twice:
        outlier[final == twice[0]] = 0
    outlier[np.isin(final, zero_obs)] = 0
    if bad_at.shape[0]:
        outlier[bad_at[0]] = 0
    no_facet = rng.uniform(size=P) < no_facet_frac
    inl = [int(p) for p in final[(final >= 0) & (outlier == 0)] if not bad[p] and n_obs[p] > 0 and p not in twice[:1]]
    if inl:
        no_facet[inl[0]] = True
    nodes[no_facet] = -1
    bary[no_facet] = 0.0
    normal = sc["normal"].copy()
    away = free_pts[rng.uniform(size=free_pts.shape[0]) < away_frac]
    normal[away] = -normal[away]
    late_bad = rng.choice(free_pts, min(max(2, P // 50), free_pts.shape[0]), replace=False).astype(np.int32) if free_pts.shape[0] else np.zeros(0, np.int32)
    n_kf = sc["tables"].shape[0]
    first_kf = rng.integers(max(0, n_kf - 5), n_kf + 1, P).astype(np.int32)
    visible = rng.integers(1, 20, P).astype(np.int32)
    found = np.minimum(rng.integers(1, 20, P), visible).astype(np.int32)
    node_xyz = sc["template_xyz"] + rng.normal(0.0, 2e-3, sc["template_xyz"].shape)
    f = sc["frame"]
    dT = np.eye(4)
    dT[:3, :3] = _rodrigues(rng.normal(size=3) * 0.002)
    dT[:3, 3] = rng.uniform(-0.002, 0.002, 3)
    Tc = (dT @ np.asarray(f.Tcw, np.float64)).astype(np.float32)
    frame_after = track.TrackFrame(**{**f.__dict__, "Tcw": Tc, "Ow": track.camera_center(Tc)})
    sc.update(nodes=nodes, bary=bary, normal=normal, late_bad=np.sort(late_bad), visible=visible, found=found, first_kf=first_kf, current_kf=int(n_kf), node_xyz=node_xyz,
              frame_after=frame_after, final_points=final.astype(np.int32), outlier=outlier)
    return sc


def write_track_close_scene(sc, prev_points, path):
    """What integration/trackclose_shim_test_main.cc reads beside the write_local_map_scene file of the same scene: the template nodes before
    and after the optimisation, per point its facet, barycentrics, counters and first keyframe, the culling keyframe, the points that turn
    bad after the previous frame, the pose after the optimisation, and per key point what the previous frame held (prev_points), the final
    map point and the outlier flag."""
    fl = lambda vs: " ".join(repr(float(v)) for v in vs)
    a = sc["frame_after"].arrays()
    with open(path, "w") as f:
        f.write(f"{sc['node_xyz'].shape[0]}\n")
        for x0, x1 in zip(sc["template_xyz"], sc["node_xyz"]):
            f.write(f"{fl(x0)} {fl(x1)}\n")
        for p in range(sc["xyz"].shape[0]):
            f.write(f"{' '.join(str(int(n)) for n in sc['nodes'][p])} {fl(sc['bary'][p])} {int(sc['visible'][p])} {int(sc['found'][p])} {int(sc['first_kf'][p])}\n")
        f.write(f"{int(sc['current_kf'])} {sc['late_bad'].shape[0]} {' '.join(str(int(p)) for p in sc['late_bad'])}\n")
        f.write(f"{fl(a['Tcw'].ravel())}\n{fl(a['Ow'])}\n")
        for j in range(sc["final_points"].shape[0]):
            f.write(f"{int(prev_points[j])} {int(sc['final_points'][j])} {int(sc['outlier'][j])}\n")


# ---------------------------------------------------------------------------------------------------------
# The template switch (MapPointStore.switch_template / need_new_template): a track-close scene whose map gets a reference keyframe
# with key points on a small image, a depth spline, surface points and the keyframe store's side of every keyframe.
# ---------------------------------------------------------------------------------------------------------
def switch_depth(u, v, seed: int = 0):
    """The smooth depth the template switch scenes put under their reference keyframe, over normalised image coordinates."""
    return 1.0 + 0.08 * np.sin(2.5 * np.asarray(u, np.float64) + 0.3 * seed) * np.cos(2.0 * np.asarray(v, np.float64))


def make_template_switch_scene(seed: int = 0, rows: int = 120, cols: int = 160, n_kp: int = 300, held_frac: float = 0.4, n_kf: int = 3,
                               ref_slot: int = -2, ctrl=(13, 15), levels: int = 8, half: bool = False, **local_map):
    """make_track_close_scene(seed, n_kf, n_kp, ...) (its keys are kept; the table of the reference keyframe, the observations and one bad
    flag differ, see below) plus what DefLocalMapping::updateTemplate reads of the reference keyframe ref_slot (negative: from the end):
      rows, cols, kp (n_kp,2) float32          its image size and undistorted key points.  About held_frac of the key points keep their point
                                               (the others are emptied and lose their observation); one held point is bad.  Half of the empty
                                               key points sit inside the box window of a held one (random key points mask very little at
                                               this size), the others are spread over the image; a few key points lie on the image border.
                                               half=True keeps the held key points in the left half of the image (an exploring camera)
      camera                                   fx, fy, cx, cy of that image; the B-spline domain is narrower than the image, so key points
                                               near the left and right border lie beside the mesh and embed in no facet
      bbs (umin, umax, nptsu, vmin, vmax, nptsv, 1), depth_ctrl (nptsu * nptsv,)   the keyframe's depth spline (switch_depth at the control sites)
      surface_pts (n_kp,3) float32             Surface::get3DSurfacePoint per key point: (u d, v d, d) with d = switch_depth
      Twc (4,4) float32                        GetPoseInverse() of the reference keyframe
      kf_Ow (K,3), kf_desc (K,n_kp,32), kf_octave (K,n_kp), scale_factors (levels,)   the keyframe store's side of every keyframe"""
    from . import track
    sc = dict(make_track_close_scene(seed, n_kf=n_kf, n_kp=n_kp, **local_map))
    rng = np.random.default_rng(11000 + seed)
    K = sc["tables"].shape[0]
    r = ref_slot % K
    tables = sc["tables"].copy()
    bad = sc["bad"].copy()
    sc["kf_bad"] = sc["kf_bad"].copy()
    sc["kf_bad"][r] = False                                        # referenceKF_ is a keyframe of the map: never a bad one
    held = np.nonzero(tables[r] >= 0)[0]
    want = max(4, int(held_frac * n_kp))
    if held.shape[0] > want:                                       # empty the others; their points no longer observe the keyframe
        drop = rng.choice(held, held.shape[0] - want, replace=False)
        gone = np.isin(sc["obs_point"], tables[r, drop]) & (sc["obs_kf"] == r)
        sc["obs_point"], sc["obs_kf"] = sc["obs_point"][~gone], sc["obs_kf"][~gone]
        tables[r, drop] = -1
    held = np.nonzero(tables[r] >= 0)[0]
    empty = np.nonzero(tables[r] < 0)[0]
    bad[tables[r, held[:-1]]] = False                              # exactly one held bad point
    bad[tables[r, held[-1]]] = True
    good = held[:-1]
    k = cols // 20
    a = k // 2
    kp = np.stack([rng.uniform(0, cols - 1e-3, n_kp), rng.uniform(0, rows - 1e-3, n_kp)], 1)
    if half:
        kp[held, 0] = rng.uniform(0, cols / 2, held.shape[0])
    near = empty[: empty.shape[0] // 2]                             # inside the window of a held key point: px - (k-1-a) .. px + a
    src = rng.choice(good, near.shape[0])
    kp[near, 0] = np.clip(np.floor(kp[src, 0]) + rng.integers(-(k - 1 - a), a + 1, near.shape[0]) + rng.uniform(0, 0.99, near.shape[0]), 0, cols - 1e-3)
    kp[near, 1] = np.clip(np.floor(kp[src, 1]) + rng.integers(-(k - 1 - a), a + 1, near.shape[0]) + rng.uniform(0, 0.99, near.shape[0]), 0, rows - 1e-3)
    border = np.concatenate([good[:4], empty[-4:]])                # held and empty key points in the first and last column and row
    kp[border[0::4], 0] = 0.25
    kp[border[1::4], 0] = cols - 0.5
    kp[border[2::4], 1] = 0.75
    kp[border[3::4], 1] = rows - 0.25
    kp = kp.astype(np.float32)
    fx = fy = 0.625 * cols
    cx, cy = cols / 2.0, rows / 2.0
    u, v = (kp[:, 0].astype(np.float64) - cx) / fx, (kp[:, 1].astype(np.float64) - cy) / fy
    d = switch_depth(u, v, seed)
    surface_pts = np.stack([u * d, v * d, d], 1).astype(np.float32)
    umax, vmax = 0.875 * (cols - cx) / fx, 1.05 * (rows - cy) / fy
    nu, nv = ctrl
    su = -umax + (np.arange(nu) - 1) * (2 * umax / (nu - 3))       # the sites of a uniform cubic B-spline's control points
    sv = -vmax + (np.arange(nv) - 1) * (2 * vmax / (nv - 3))
    depth_ctrl = switch_depth(su[:, None], sv[None, :], seed).reshape(-1)
    Twc = np.eye(4)
    Twc[:3, :3] = _rodrigues(rng.normal(size=3) * 0.02)
    Twc[:3, 3] = rng.uniform(-0.03, 0.03, 3)
    Twc = Twc.astype(np.float32)
    sf, _ = track.orb_pyramid(levels)
    kf_Ow = rng.uniform(-0.05, 0.05, (K, 3)).astype(np.float32)
    kf_Ow[r] = Twc[:3, 3]
    sc.update(tables=tables, bad=bad, ref_slot=int(r), rows=int(rows), cols=int(cols), kp=kp, camera=(fx, fy, cx, cy),
              bbs=(-umax, umax, int(nu), -vmax, vmax, int(nv), 1), depth_ctrl=depth_ctrl, surface_pts=surface_pts, Twc=Twc, kf_Ow=kf_Ow,
              kf_desc=rng.integers(0, 256, (K, n_kp, 32), dtype=np.uint8), kf_octave=rng.integers(0, levels, (K, n_kp)).astype(np.int32),
              scale_factors=sf)
    return sc


def write_template_switch_scene(sc, grid, path):
    """What integration/tmplswitch_shim_test_main.cc reads beside the write_local_map_scene file of the same scene: the reference keyframe,
    its image size and the template grid, Twc, the depth spline, the pyramid, per keyframe the camera centre and per key point the octave
    and the descriptor row, and per key point of the reference keyframe the position and the surface point."""
    fl = lambda vs: " ".join(repr(float(v)) for v in vs)
    K, n_kp = sc["tables"].shape
    r = sc["ref_slot"]
    with open(path, "w") as f:
        f.write(f"{r} {sc['rows']} {sc['cols']} {grid[0]} {grid[1]}\n{fl(sc['Twc'].ravel())}\n")
        b = sc["bbs"]
        f.write(f"{b[0]!r} {b[1]!r} {b[2]} {b[3]!r} {b[4]!r} {b[5]} {b[6]}\n{fl(sc['depth_ctrl'])}\n")
        f.write(f"{sc['scale_factors'].shape[0]}\n{fl(sc['scale_factors'])}\n")
        for k in range(K):
            f.write(f"{fl(sc['kf_Ow'][k])}\n")
            for j in range(n_kp):
                f.write(f"{int(sc['kf_octave'][k, j])} {' '.join(str(int(v)) for v in sc['kf_desc'][k, j])}\n")
        for j in range(n_kp):
            f.write(f"{fl(sc['kp'][j])} {fl(sc['surface_pts'][j])}\n")
