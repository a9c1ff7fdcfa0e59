"""TEST INFRASTRUCTURE ONLY: operating points of the tracking hot path away from the one synthetic camera, pose and weight triple.

Tables of cameras, regulariser weights, worlds (rigid motions of the whole scene), scene scales, noise levels and key point counts, and
about a dozen named CASES that each move several of these axes at once (not their cross product).  make_problem() turns a case into
an SfT problem with defslam_amd.synth and moves it into the case's world; uses() lists every (case, mesh, matches, problem id) the GPU
tests solve, which tests/test_operating_points_cpu.py checks for eligibility (an exact comparison of Levenberg-Marquardt trajectories
needs a problem whose accept / reject decisions are not rounding noise).  No fixtures here; nothing in defslam_amd/ imports this.
"""
from __future__ import annotations

import copy
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
from scipy.spatial.transform import Rotation

# name: (fx, fy, cx, cy, width, height) -- the pinholes of the reference's settings files; `tall` is `hamlyn` transposed (fy > fx)
CAMERAS = {
    "hamlyn": (755.312744, 420.477722, 327.875, 165.484406, 720, 288),
    "mandala": (435.2046959714599, 435.2046959714599, 367.4517211914062, 252.2008514404297, 752, 480),
    "webcam": (312.7647974, 312.0041674, 155.66387, 117.4352139, 320, 240),
    "tall": (420.477722, 755.312744, 165.484406, 327.875, 288, 720),
    "synth": (500.0, 500.0, 320.0, 240.0, 640, 480),
}

# name: (reg_lap, reg_inex, reg_temp); `switch` is the solve after a keyframe switch (RegTemp = 0)
WEIGHTS = {
    "default": (700.0, 12000.0, 0.05),
    "webcam": (25.0, 240.0, 0.21),
    "switch": (700.0, 12000.0, 0.0),
    "weak": (1.0, 10.0, 0.0),
}

# name: (rotation vector, translation) of the rigid motion G applied to the whole scene.  The turn_* worlds bring the pose's quaternion
# in through the three non-trace branches of the matrix -> quaternion conversion; their angles stay off pi so that w stays off 0.
WORLDS = {
    "identity": ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
    "oblique": ((0.9, -1.1, 0.7), (0.4, -0.3, 1.5)),
    "turn_x": ((0.98 * np.pi, 0.1, 0.0), (0.3, -0.2, 2.0)),
    "turn_y": ((0.0, 0.97 * np.pi, 0.2), (1.0, 2.0, -3.0)),
    "turn_z": ((0.1, -0.15, 0.98 * np.pi), (-0.5, 0.1, 0.4)),
}
# the branch of the matrix -> quaternion conversion each world's float32 pose must take: "trace", or the largest diagonal entry
WORLD_BRANCH = {"identity": "trace", "oblique": "trace", "turn_x": 0, "turn_y": 1, "turn_z": 2}

NOISE = {"clean": (0.0, 0.0), "usual": (0.5, 0.05), "heavy": (2.0, 0.30)}   # (pixel noise, outlier fraction)


@dataclass(frozen=True)
class Case:
    camera: str
    world: str
    weights: str
    z0: float = 1.0
    noise: str = "usual"
    n_frame: int = 1200
    # problem ids (the seed of the frame's random stream) the tests use for this case: the first one on the 9 x 14 mesh of the GPU tests, the
    # last one on the 7 x 9 mesh of the oracle comparison.  An id that fails the eligibility conditions is replaced here, never excused in a
    # GPU test.
    pids: Tuple[int, ...] = (0,)

    @property
    def name(self) -> str:
        s = f"{self.camera}/{self.world}/{self.weights}"
        if self.z0 != 1.0:
            s += f"/z0={self.z0:g}"
        if self.noise != "usual":
            s += f"/{self.noise}"
        if self.n_frame != 1200:
            s += f"/n={self.n_frame}"
        return s

    @property
    def regs(self):
        return WEIGHTS[self.weights]

    @property
    def K(self):
        return CAMERAS[self.camera][:4]

    @property
    def image_size(self):
        return CAMERAS[self.camera][4:]


_CASE_LIST = [
    Case("synth", "identity", "default"),                       # the control: today's operating point
    Case("hamlyn", "oblique", "default"),
    Case("hamlyn", "oblique", "webcam"),
    Case("hamlyn", "turn_x", "webcam"),
    Case("tall", "turn_y", "switch"),
    # id 0 replaced for eligibility: with these weak regularisers it needs ten dampings in a row on the 7 x 9 mesh (and id 1 on the 9 x 14
    # mesh, where it ends at |q_w| = 0.002)
    Case("webcam", "turn_z", "weak", pids=(3,)),
    Case("mandala", "identity", "default", z0=8.0),
    Case("hamlyn", "oblique", "default", z0=0.15),
    Case("hamlyn", "oblique", "default", noise="clean"),
    Case("hamlyn", "oblique", "default", noise="heavy"),
    Case("hamlyn", "oblique", "default", n_frame=300),
    Case("hamlyn", "oblique", "default", n_frame=5000),
]
CASES = {c.name: c for c in _CASE_LIST}
CASE_NAMES = list(CASES)


def world_matrix(world: str) -> np.ndarray:
    """G (4 x 4, float64) of a named world."""
    rv, t = WORLDS[world]
    G = np.eye(4)
    G[:3, :3] = Rotation.from_rotvec(np.asarray(rv, np.float64)).as_matrix()
    G[:3, 3] = t
    return G


def move_points(G: np.ndarray, x: np.ndarray) -> np.ndarray:
    """G x, rounded to float32 as the reference's nodes are (returned as float64)."""
    return (np.asarray(x, np.float64) @ G[:3, :3].T + G[:3, 3]).astype(np.float32).astype(np.float64)


def move_pose(G: np.ndarray, Tcw: np.ndarray) -> np.ndarray:
    """Tcw G^-1 as float32: the camera sees the moved scene as it saw the scene."""
    return (np.asarray(Tcw, np.float32).astype(np.float64) @ np.linalg.inv(G)).astype(np.float32)


def quaternion_branch(T: np.ndarray):
    """Which branch a matrix -> quaternion conversion takes on the rotation of a pose: "trace" when the trace is positive, otherwise the index
    of the largest diagonal entry."""
    R = np.asarray(T, np.float64)[:3, :3]
    if np.trace(R) > 0:
        return "trace"
    return int(np.argmax(np.diag(R)))


def make_problem(case, rows: int, cols: int, m: int, pid: Optional[int] = None, keep_cols: Optional[int] = None, template_camera: Optional[str] = None):
    """(template, frame, weights) of a case (a Case or its name) on a rows x cols grid with m matches: generated by defslam_amd.synth in
    the case's camera at the case's scale, then moved into the case's world (template and current nodes G x as float32, initial pose Tcw G^-1
    as float32, observations unchanged).  keep_cols: a partial view -- only observations whose facet lies in the first keep_cols columns.
    template_camera: the grid fills the frustum of this camera instead of the case's (problems of several cameras on ONE template)."""
    from defslam_amd import synth
    c = CASES[case] if isinstance(case, str) else case
    pid = c.pids[0] if pid is None else pid
    noise_px, outlier_frac = NOISE[c.noise]
    tcam = CAMERAS[c.camera if template_camera is None else template_camera]
    tmpl = synth.make_grid_template(rows, cols, z0=c.z0, camera=tcam[:4], image_size=tcam[4:])
    fr = synth.make_frame(tmpl, m, pid, noise_px=noise_px, outlier_frac=outlier_frac, n_frame=c.n_frame, camera=c.K, image_size=c.image_size, scale=c.z0)
    if keep_cols is not None:
        keep = [col + cols * r for r in range(rows) for col in range(keep_cols)]
        sel = np.all(np.isin(fr.obs_nodes, keep), axis=1)
        for k in ["obs_facet", "obs_nodes", "obs_bary", "obs_uv", "obs_invsig2", "is_outlier_gt"]:
            setattr(fr, k, getattr(fr, k)[sel])
    return move_problem(c.world, tmpl, fr) + (c.regs,)


def move_problem(world: str, tmpl, fr):
    """A synth template and frame moved into a world (copies; the arguments are left alone)."""
    G = world_matrix(world)
    tmpl, fr = copy.copy(tmpl), copy.copy(fr)
    tmpl.xyz0 = move_points(G, tmpl.xyz0)
    fr.xyz = move_points(G, fr.xyz)
    fr.Tcw = move_pose(G, fr.Tcw)
    fr.gt_xyz = np.asarray(fr.gt_xyz, np.float64) @ G[:3, :3].T + G[:3, 3]
    fr.gt_Tcw = np.asarray(fr.gt_Tcw, np.float64) @ np.linalg.inv(G)
    return tmpl, fr


# ---- what the GPU tests solve: (case name, rows, cols, matches, problem id, neighbour layers, columns kept or None) -----------------
SMALL = (7, 9, 200)            # C oracle against the NumPy restatement, every case
MESH = (9, 14, 420)            # latency mode and the mixed batch of the throughput shape
WIDE_CASE = "hamlyn/turn_x/webcam"
WIDE = [(6, 41, 500, 0), (5, 45, 400, 0)]                     # W16-like (two-sided / wide solver) and B272-like (row-major fallback)
LAYERS_CASE = "hamlyn/oblique/webcam"
LAYERS_VIEW = (9, 14, 420, 0, 7)                              # rows, cols, matches, pid, columns kept
NORMAL_EQ_CASES = ["hamlyn/oblique/webcam", "tall/turn_y/switch"]
GOLDEN_CASE = ("hamlyn/oblique/webcam", 8, 12, 250, 0)        # tests/golden/make_golden.py
SHARED_CASE = ("tall/turn_y/switch", 10, 20, [10], 800, 1)    # case, rows, cols, cuts, matches, pid
CONNECTED_CASE = ("hamlyn/turn_x/webcam", 10, 10, 300, 2)     # case, rows, cols, matches, pid


def uses():
    """Every solve of the GPU tests as (case, rows, cols, m, pid, layers, keep_cols)."""
    out = []
    for name, c in CASES.items():
        out.append((name, *MESH, c.pids[0], 1, None))
    for rows, cols, m, pid in WIDE:
        out.append((WIDE_CASE, rows, cols, m, pid, 1, None))
    rows, cols, m, pid, kc = LAYERS_VIEW
    for layers in (0, 1):
        out.append((LAYERS_CASE, rows, cols, m, pid, layers, kc))
    name, rows, cols, m, pid = GOLDEN_CASE
    out.append((name, rows, cols, m, pid, 1, None))
    name, rows, cols, m, pid = CONNECTED_CASE
    out.append((name, rows, cols, m, pid, 1, None))
    return out


# ---- the mixed batch of the throughput shape -----------------------------------------------------------------------------------------------
# A batch is solved on ONE template (dsh_template_build belongs to the context, not to a frame), so the rigid placement of the scene and its
# scale belong to the batch: three placements that reach the two non-trace branches the latency tests reach with other cases, and both scale
# extremes.  Inside a batch every problem takes camera, weights, noise and key point count from its own case; the grid fills the frustum of one
# camera (the narrowest) for all of them.
BATCH_TEMPLATE_CAMERA = "webcam"
BATCH_PLACEMENTS = [("oblique", 1.0), ("turn_x", 0.15), ("turn_y", 8.0)]
# (world, z0, case name) -> problem id where id 0 is not eligible: these two (the same problem) end at |q_w| = 0.010
BATCH_PID = {("turn_x", 0.15, "hamlyn/oblique/webcam"): 1, ("turn_x", 0.15, "hamlyn/turn_x/webcam"): 1}


def batch_case(world: str, z0: float, name: str) -> Case:
    """The case `name` as a member of the batch placed by (world, z0): its own camera, weights, noise and key point count."""
    c = CASES[name]
    return Case(c.camera, world, c.weights, z0=z0, noise=c.noise, n_frame=c.n_frame, pids=(BATCH_PID.get((world, z0, name), 0),))


def batch_problem(world: str, z0: float, name: str):
    rows, cols, m = MESH
    return make_problem(batch_case(world, z0, name), rows, cols, m, template_camera=BATCH_TEMPLATE_CAMERA)


def batch_plan(B: int):
    """Which case problem b of the mixed batch belongs to: the cases interleaved with a stride of 5, an order that is not sorted by case."""
    n = len(CASE_NAMES)
    assert n % 5 != 0
    return [CASE_NAMES[(5 * b + 3) % n] for b in range(B)]
