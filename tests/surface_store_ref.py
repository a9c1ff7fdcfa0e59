"""TEST INFRASTRUCTURE ONLY: sequential restatement of the resident Surface of a keyframe (the checker of dsh_keyframe_surface_init,
_set_depth, _set_points, _set_normals, _take_normals, _gather, _get, _vertices, of the selection and the write-backs of dsh_keyframe_sfn
and of Surface::applyScale inside dsh_keyframe_register) over tests/surface_register_ref.RegisterModel.

Plain Python, statement by statement after the reference:
  Surface::Surface, SurfacePoint .................. Modules/Mapping/Surface.cc:31-37
  Surface::saveArray .............................. Modules/Mapping/Surface.cc:50-56
  Surface::enoughNormals .......................... Modules/Mapping/Surface.cc:62-67
  Surface::setNormalSurfacePoint .................. Modules/Mapping/Surface.cc:76-85
  Surface::set3DSurfacePoint ...................... Modules/Mapping/Surface.cc:94-97
  Surface::applyScale ............................. Modules/Mapping/Surface.cc:107-121
  ShapeFromNormals::obtainM, the walk ............. Modules/Mapping/ShapeFromNormals.cc:190-210
  ShapeFromNormals::estimate, the write-backs ..... Modules/Mapping/ShapeFromNormals.cc:158-167
The solve of Shape from Normals is not restated here: the tests run defslam_amd.nrsfm.ShapeFromNormals and oracle.sfn_estimate on the
sites this module selects.  Nothing in defslam_amd/ imports this module.
"""
from __future__ import annotations

import numpy as np

from surface_register_ref import RegisterModel, apply_scale

SFN_COUNT_NAMES = ("n_sites", "n_empty", "n_bad", "n_no_normal", "n_nan")
NORMALS_LIMIT = 10


class SurfaceExists(Exception):
    """A second Surface for the same keyframe (DSH_ERR_STATE)."""


class Surface:
    """defSLAM::Surface of a keyframe with N key points, plus DefKeyFrame::mpKeypointNorm."""

    def __init__(self, kpn):
        self.kpn = np.asarray(kpn, np.float32).reshape(-1, 2).copy()
        N = self.kpn.shape[0]
        self.normal = np.zeros((N, 3), np.float32)
        self.has = np.zeros(N, bool)
        self.pts = np.zeros((N, 3), np.float32)
        self.n_normals = 0
        self.bbs = None          # the tuple (umin, umax, nptsu, vmin, vmax, nptsv, 1)
        self.ctrl = None         # nodesDepth_, float64

    @property
    def enough_normals(self):
        return self.n_normals >= NORMALS_LIMIT


class SurfaceModel(RegisterModel):
    def __init__(self):
        super().__init__()
        self.surface = {}        # slot -> Surface

    def clear(self):
        self.__init__()

    def surface_init(self, slot, kpn):
        if slot in self.surface:
            raise SurfaceExists(slot)
        s = Surface(kpn)
        assert s.kpn.shape[0] == len(self.kfs[slot].table) and np.isfinite(s.kpn).all()
        self.surface[slot] = s

    def set_depth(self, slot, bbs, ctrl):
        s = self.surface[slot]
        s.bbs = tuple(bbs[:6]) + (1,)
        s.ctrl = np.asarray(ctrl, np.float64).reshape(-1)[:bbs[2] * bbs[5]].copy()

    def set_points(self, slot, idx, pts):
        for i, x in zip(idx, np.asarray(pts, np.float32).reshape(-1, 3)):
            self.surface[slot].pts[int(i)] = x

    def set_normals(self, slots, idx, normals):
        """setNormalSurfacePoint per entry of the call, in call order; returns each target keyframe's numberofNormals_ after the call."""
        for k, i, n in zip(slots, idx, np.asarray(normals, np.float32).reshape(-1, 3)):
            s = self.surface[int(k)]
            if not s.has[int(i)]:
                s.n_normals += 1
            s.has[int(i)] = True
            s.normal[int(i)] = n
        return np.array([self.surface[int(k)].n_normals for k in slots], np.int32)

    def gather(self, slots, idx):
        """(Ni(0), Ni(1)) or zeros, getNormalSurfacePoint's return value, mpKeypointNorm: x0 / has_x0 / ref_uv of a normal solve."""
        n = len(slots)
        nxy, has, uv = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros((n, 2), np.float32)
        for j, (k, i) in enumerate(zip(slots, idx)):
            s = self.surface[int(k)]
            if s.has[int(i)]:
                nxy[j], has[j] = s.normal[int(i), :2], 1
            uv[j] = s.kpn[int(i)]
        return nxy, has, uv

    def sfn_select(self, slot):
        """ShapeFromNormals.cc:190-210: (counts, the entry of each site, u, v in float64, normals in float32)."""
        s = self.surface[slot]
        c = dict.fromkeys(SFN_COUNT_NAMES, 0)
        which = []
        for i, p in enumerate(self.kfs[slot].table):
            if p < 0:
                c["n_empty"] += 1
            elif self.points[p].bad:
                c["n_bad"] += 1
            elif not s.has[i]:
                c["n_no_normal"] += 1
            elif np.isnan(s.normal[i]).any():
                c["n_nan"] += 1
            else:
                which.append(i)
        c["n_sites"] = len(which)
        w = np.array(which, np.int64)
        return c, w, s.kpn[w, 0].astype(np.float64), s.kpn[w, 1].astype(np.float64), s.normal[w].copy()

    def sfn_write(self, slot, bbs, ctrl, pts):
        """What estimate() leaves when it succeeds: set3DSurfacePoint of every key point and saveArray."""
        self.surface[slot].pts = np.asarray(pts, np.float32).reshape(-1, 3).copy()
        self.set_depth(slot, bbs, ctrl)

    def apply_scale(self, slot, s22):
        s = self.surface[slot]
        s.pts = apply_scale(s.pts, s22)
        if s.ctrl is not None:
            s.ctrl = np.float64(s22) * s.ctrl


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------

HELD = ("site", "bad", "no_normal", "nan0", "nan1", "nan2", "inf", "emptied")


def make_surface_scene(N, seed=0, hold=0.5, n_sites=None, nu=13, nv=15, with_inf=True):
    """A model with two keyframes -- slot 0 a small one in front, slot 1 the keyframe of N key points whose Surface is under test -- on
    the smooth surface of synth.make_sfn_scene.  Per entry i of slot 1 a role:
      site        a point that is not bad, with a normal        empty       no point
      bad         a bad point (it has a normal)                 no_normal   a point, no normal
      nan0..2     a normal whose component 0..2 is NaN          inf         a normal with an infinite component: a site for the selection
      dup         the point of an earlier site again, with a normal of its own: a second site
      emptied     a point with a normal and an observation record that names the entry: setBadFlag empties the entry (scene["emptied"])
    n_sites given: exactly that many sites, no inf, and one entry of every other role where N leaves room for them; else
    round(hold * N) entries hold a point, and every role is there when N >= 32 and 0 < hold < 1 (inf unless with_inf is False).
    Returns a dict: model, slot, N, kpn, bbs, mean_depth, roles, normals (entry -> normal, of every entry that gets one), emptied."""
    from defslam_amd import synth
    g = synth.make_sfn_scene(max(N, 1), seed=seed + 31, with_normal_frac=1.0, nu=nu, nv=nv)
    rng = np.random.default_rng(7000 * seed + N)
    kpn = np.stack([g["u_all"], g["v_all"]], 1).astype(np.float32)[:N]
    order = rng.permutation(N).tolist()
    roles = ["empty"] * N
    others = ["bad", "no_normal", "nan0", "nan1", "nan2", "emptied", "dup"]
    if n_sites is not None:
        assert n_sites <= N
        for _ in range(n_sites - (1 if N >= n_sites + len(others) else 0)):
            roles[order.pop()] = "site"
        if N >= n_sites + len(others):
            for r in others:
                roles[order.pop()] = r
    else:
        for _ in range(int(round(hold * N))):
            x = rng.random()
            roles[order.pop()] = "bad" if x < 0.1 else "no_normal" if x < 0.25 else "site"
        if N >= 32 and 0 < hold < 1:
            sites = [i for i in range(N) if roles[i] == "site"]
            assert len(sites) >= 9 and len(order) >= 1
            for r, i in zip(["nan0", "nan1", "nan2", "emptied", "bad", "no_normal"] + (["inf"] if with_inf else []), sites[-7:]):
                roles[i] = r
            roles[order.pop()] = "dup"
    m = SurfaceModel()
    table = [-1] * N
    d = g["depth_true"]
    for i in range(N):
        if roles[i] in HELD:
            table[i] = m.add_point(xyz=(kpn[i, 0] * d[i], kpn[i, 1] * d[i], d[i]), bad=roles[i] == "bad", desc=rng.integers(0, 256, 32, dtype=np.uint8))
    first_site = next((i for i in range(N) if roles[i] == "site"), None)
    for i in range(N):
        if roles[i] == "dup":
            table[i] = table[first_site]
    loose = m.add_point(xyz=(0.0, 0.1, 0.9))
    front = [p for p in table if p >= 0][:3] + [-1, loose]
    m.add_keyframe(front)
    slot = m.add_keyframe(table)
    emptied = []
    for i in range(N):
        if roles[i] == "emptied":
            assert m.add_observation(table[i], slot, i)
            emptied.append(table[i])
    normals = {}
    for i in range(N):
        if roles[i] in ("empty", "no_normal"):
            continue
        n = g["normals"][i].astype(np.float32).copy()
        if roles[i].startswith("nan"):
            n[int(roles[i][3])] = np.nan
        elif roles[i] == "inf":
            n[1] = np.inf
        normals[i] = n
    return dict(model=m, slot=slot, N=N, kpn=kpn, bbs=g["bbs"], mean_depth=g["mean_depth"], roles=roles, normals=normals, emptied=emptied)


def normal_calls(sc, seed=0):
    """The scene's normals as two calls of set_normals on the keyframe under test, (slots, idx, normals) each: the first holds a decoy
    ahead of the true normal for every third target (a target named twice in one call keeps the later one), the second repeats a
    quarter of the targets with the normal they hold already (numberofNormals_ must not move)."""
    rng = np.random.default_rng(seed)
    ents = sorted(sc["normals"])
    idx, nr = [], []
    for j, i in enumerate(ents):
        if j % 3 == 0:
            idx.append(i)
            nr.append(rng.standard_normal(3).astype(np.float32))
    for i in rng.permutation(ents).tolist():
        idx.append(i)
        nr.append(sc["normals"][i])
    again = ents[::4]
    mk = lambda ii, nn: (np.full(len(ii), sc["slot"], np.int32), np.array(ii, np.int32), np.array(nn, np.float32).reshape(-1, 3))
    return mk(idx, nr), mk(again, [sc["normals"][i] for i in again])
