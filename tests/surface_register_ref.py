"""TEST INFRASTRUCTURE ONLY: sequential restatement of the surface registration of a keyframe from the resident stores (the checker of
dsh_keyframe_snapshot_positions, dsh_keyframe_register_clouds, dsh_keyframe_register and dsh_keyframe_set_pose) over
tests/store_model.MapModel (through tests/point_erase_ref.EraseRefMap, whose setBadFlag, EraseObservation and MapPointCulling the
snapshot has to survive).

Plain Python, statement by statement after the reference:
  DefKeyFrame::DefKeyFrame, PosesKeyframes ........ Modules/Common/DefKeyFrame.cc:60-74
  SurfaceRegistration::registerSurfaces ........... Modules/Mapping/SurfaceRegistration.cc:60-104 (the clouds), :106-107, :145, :150
  Surface::applyScale ............................. Modules/Mapping/Surface.cc:107-121
  KeyFrame::SetPose ............................... Thirdparty/ORBSLAM_2/src/KeyFrame.cc:97-111
RegisterModel keeps the literal PosesKeyframes as a dictionary (point, slot) -> xyz and the facets as a dictionary point -> nodes.  The
numeric part of the registration (scaleMinMedian, OptimizeHorn, the composition) is not restated here: the tests run
defslam_amd.register.registerSurfaces on the clouds this module selects.  Nothing in defslam_amd/ imports this module.
"""
from __future__ import annotations

import numpy as np

from point_erase_ref import EraseRefMap
from template_switch_ref import to_world

f32 = np.float32
COUNT_NAMES = ("n_pairs", "n_empty", "n_bad", "n_no_facet", "n_no_snapshot")


class SnapshotTaken(Exception):
    """A second snapshot of the same keyframe (DSH_ERR_STATE)."""


def apply_scale(surface_pts, s22):
    """Surface::applyScale on a cv::Vec3f: Vec * double, rounded to float32 per component."""
    return (np.asarray(surface_pts, np.float32).astype(np.float64) * np.float64(s22)).astype(np.float32)


def centre_of(Tcw):
    """KeyFrame::SetPose: Ow = -Rcw.t() * tcw, the three products of a row summed left to right in float32."""
    T = np.asarray(Tcw, np.float32).reshape(4, 4)
    return np.array([-f32(f32(f32(T[0, i] * T[0, 3]) + f32(T[1, i] * T[1, 3])) + f32(T[2, i] * T[2, 3])) for i in range(3)], np.float32)


def consumed(n, u):
    """GroundTruthCalculator.cc:64-84: one draw per point, and n - 1 more for each point whose draw is <= 0.25; None: u is too short."""
    k = 0
    for _ in range(n):
        if k >= len(u):
            return None
        r = u[k]
        k += 1
        if r > 0.25:
            continue
        if k + (n - 1) > len(u):
            return None
        k += n - 1
    return k


class RegisterModel(EraseRefMap):
    """The map with what takes a point out of it (tests/point_erase_ref.py) and the snapshot; none of the erasing functions touches
    self.snap: PosesKeyframes is a member of the point, keyed by keyframe, and no function of the reference erases from it."""

    def __init__(self):
        super().__init__()
        self.facet = {}          # point -> its three node indices (DefMapPoint::getFacet is non-null)
        self.snap = {}           # (point, slot) -> xyz: DefMapPoint::PosesKeyframes[kf]
        self.snap_entries = {}   # slot -> (point per entry or -1, xyz per entry): the shape dsh_keyframe_get_snapshot reads back

    def snapshot_positions(self, slot):
        """DefKeyFrame.cc:60-74 for keyframe `slot`; returns the number of entries taken."""
        if slot in self.snap_entries:
            raise SnapshotTaken(slot)
        table = self.kfs[slot].table
        pt, xyz = np.full(len(table), -1, np.int32), np.zeros((len(table), 3), np.float32)
        for i, p in enumerate(table):
            if p >= 0 and not self.points[p].bad and p in self.facet:
                self.snap[(p, slot)] = self.points[p].xyz.copy()
                pt[i], xyz[i] = p, self.points[p].xyz
        self.snap_entries[slot] = (pt, xyz)
        return int((pt >= 0).sum())

    def get_snapshot(self, slot):
        table = self.kfs[slot].table
        return self.snap_entries.get(slot, (np.full(len(table), -1, np.int32), np.zeros((len(table), 3), np.float32)))

    def clear(self):
        self.__init__()

    def select(self, slot, surface_pts, Twc):
        """SurfaceRegistration.cc:60-104: (counts, pair_idx, cloud_surface = cloud2pc, cloud_map = cloud1pc)."""
        c = dict.fromkeys(COUNT_NAMES, 0)
        idx, surf, mp = [], [], []
        for i, p in enumerate(self.kfs[slot].table):
            if p < 0:
                c["n_empty"] += 1
            elif self.points[p].bad:
                c["n_bad"] += 1
            elif p not in self.facet:
                c["n_no_facet"] += 1
            elif (p, slot) not in self.snap:
                c["n_no_snapshot"] += 1
            else:
                idx.append(i)
                mp.append(self.snap[(p, slot)])
                surf.append(to_world(Twc, surface_pts[i]))
        c["n_pairs"] = len(idx)
        return c, np.array(idx, np.int32), np.array(surf, np.float32).reshape(-1, 3), np.array(mp, np.float32).reshape(-1, 3)

    # the mutations the scenes make after the snapshot
    def move_points(self, ids, xyz):
        for p, x in zip(ids, np.asarray(xyz, np.float32).reshape(-1, 3)):
            self.points[int(p)].xyz = x.copy()

    def set_table(self, slot, idx, p):
        self.kfs[slot].table[int(idx)] = int(p)


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------

def _rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make_scene(N, seed=0, hold=0.5, n_pairs=None, p_bad=0.1, p_nofacet=0.1, specials=True, noise=1e-3, scale=1.35):
    """A store with two keyframes -- slot 0 a small one in front, slot 1 the keyframe of N key points that is registered -- and what a
    test does to it after the snapshot.  Per entry i of slot 1 a role:
      good         a point that is not bad and has a facet: a pair
      bad          a bad point                                          nofacet   a point without a facet
      empty        no point
      dup          the point of an earlier good entry again (before the snapshot: both entries are taken, both are pairs)
      spoil_bad    good at the snapshot, set bad after it               spoil_facet   good at the snapshot, its facet removed after it
      move_from    good at the snapshot; afterwards its point moves to the entry move_to (set_keyframe_point twice): a pair at move_to,
                   found through the snapshot of another entry
      add_to       empty at the snapshot; afterwards a point with a facet is put there: no snapshot
    n_pairs given: exactly that many pairs (hold is ignored); else round(hold * N) entries hold a point, with bad and facet-less points
    among them at the rates given.  The specials need N >= 32 and, in hold mode, 0 < hold < 1.
    Geometry as synth.make_register_scene: surface points in the camera frame whose world positions are a similarity of the points'
    positions AT THE SNAPSHOT with small noise; afterwards every point moves away, so a cloud read from the current positions differs.
    Returns a dict: model (the state before the snapshot), slot, surface_pts, Twc, u, after (the mutations, in order), roles."""
    rng = np.random.default_rng(1000 * seed + N)
    roles = ["empty"] * N
    order = rng.permutation(N).tolist()
    take = lambda: order.pop()
    special = specials and N >= 32 and (n_pairs is not None or 0 < hold < 1)
    if n_pairs is not None:
        n_special_pairs = 2 if special else 0                                     # dup and move_to are pairs themselves
        assert N >= n_pairs + 8
        for _ in range(n_pairs - n_special_pairs):
            roles[take()] = "good"
        for r in ("bad", "nofacet"):
            roles[take()] = r
    else:
        for _ in range(int(round(hold * N))):
            x = rng.random()
            roles[take()] = "bad" if x < p_bad else "nofacet" if x < p_bad + p_nofacet else "good"
    src = {}                                                                      # entry -> the entry whose point it shares or receives
    if special:
        free = [i for i in order]                                                 # still empty
        good = [i for i in range(N) if roles[i] == "good"]
        if n_pairs is None:                                                       # hold mode: the roles come out of what is there
            assert len(good) >= 4 and len(free) >= 4
            for r, i in zip(("spoil_bad", "spoil_facet"), good[-2:]):
                roles[i] = r
            good = good[:-2]
        else:
            for r in ("spoil_bad", "spoil_facet", "move_from"):
                roles[free.pop()] = r
        dup, move_to, add_to = free.pop(), free.pop(), free.pop()
        roles[dup], roles[move_to], roles[add_to] = "dup", "move_to", "add_to"
        src[dup] = good[0]
        if n_pairs is None:
            roles[good[1]] = "move_from"
        src[move_to] = roles.index("move_from")

    # geometry per entry
    w = np.stack([rng.uniform(-0.4, 0.4, N), rng.uniform(-0.3, 0.3, N), 1.0 + 0.15 * rng.standard_normal(N)], 1).reshape(N, 3)
    for e, s in src.items():
        w[e] = w[s] + 1e-3 * rng.standard_normal(3)
    R, t = _rodrigues(np.array([0.02, -0.035, 0.015])), np.array([0.03, -0.02, 0.05])
    m = (scale * (w @ R.T) + t + noise * rng.standard_normal((N, 3))).astype(np.float32)
    Twc = np.eye(4)
    Twc[:3, :3], Twc[:3, 3] = _rodrigues(np.array([0.1, 0.05, -0.07])), [0.2, -0.1, 0.3]
    Tcw = np.linalg.inv(Twc)
    surface_pts = (w @ Tcw[:3, :3].T + Tcw[:3, 3]).astype(np.float32)
    Twc = Twc.astype(np.float32)

    model = RegisterModel()
    table = [-1] * N
    held = ("good", "bad", "nofacet", "spoil_bad", "spoil_facet", "move_from")
    for i in range(N):
        if roles[i] in held:
            table[i] = p = model.add_point(xyz=m[i], bad=roles[i] == "bad", desc=rng.integers(0, 256, 32, dtype=np.uint8))
            if roles[i] != "nofacet":
                model.facet[p] = (3 * i % 7, 3 * i % 7 + 1 + i % 3, 3 * i % 7 + 5)
    for e in (e for e in range(N) if roles[e] == "dup"):
        table[e] = table[src[e]]
    extra = model.add_point(xyz=(0.1, 0.2, 1.3))                                  # the point that is put into the table later
    model.facet[extra] = (1, 2, 3)
    loose = model.add_point(xyz=(0.0, 0.1, 0.9))                                  # a point no keyframe holds
    levels, sf = 4, (1.2 ** np.arange(4)).astype(np.float32)
    kf = lambda n, Ow: dict(Ow=Ow, desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), octave=rng.integers(0, levels, n), scale_factors=sf)
    front = [p for p in table if p >= 0][:3] + [-1, loose]
    model.add_keyframe(front, **kf(len(front), (0.0, 0.0, 0.0)))
    slot = model.add_keyframe(table, **kf(N, Twc[:3, 3]))

    P = len(model.points)
    after = [("move", list(range(P)), (np.array([pt.xyz for pt in model.points]).reshape(P, 3) + rng.normal(0, 0.05, (P, 3))).astype(np.float32))]
    for i in range(N):
        if roles[i] == "spoil_bad":
            after.append(("bad", table[i]))
        elif roles[i] == "spoil_facet":
            after.append(("facet_off", table[i]))
        elif roles[i] == "move_to":
            after += [("table", src[i], -1), ("table", i, table[src[i]])]
        elif roles[i] == "add_to":
            after.append(("table", i, extra))
    n_u = max([n_pairs or 0, sum(r in ("good", "dup", "move_to") for r in roles)])
    u = rng.random(n_u + n_u * n_u) if n_u <= 700 else rng.random(16)
    return dict(model=model, slot=slot, surface_pts=surface_pts, Twc=Twc, u=u, after=after, roles=roles, N=N)


ERASE_PICKS = ("set_bad", "erase_cascade", "erase_match", "erase_keep", "cull", "twice")


def add_erase_fixture(sc):
    """Observations for what takes a point out of the map after the snapshot (tests/point_erase_ref.py), on a scene of make_scene with
    n_pairs given: three more keyframes of 8 key points, and six points of the registered keyframe that observe it and them.  Returns
    {name: entry of the registered keyframe}:
      set_bad        3 observations; setBadFlag blanks its records and the entries they name: the entry is EMPTY afterwards, not bad
      erase_cascade  2 observations; erasing the one in the registered keyframe (no erase_match) leaves nObs 1 and cascades into
                     setBadFlag over the other record: the entry still holds the point, which is bad now
      erase_match    4 observations; erased with erase_match: no cascade, the entry is emptied, the point stays good
      erase_keep     4 observations; erased without erase_match: the entry keeps the point, still a pair
      cull           3 observations, found / visible = 0.1: MapPointCulling sets it bad in full, the entry is emptied
      twice          the point that a second entry (dup) holds too, 3 observations, its record names this entry: setBadFlag empties this
                     one, the dup entry keeps the bad point
    The snapshot of all six stays: PosesKeyframes is keyed by point."""
    m, slot, roles = sc["model"], sc["slot"], sc["roles"]
    table = m.kfs[slot].table
    good = [i for i in range(sc["N"]) if roles[i] == "good"]
    dup = roles.index("dup")
    twice = next(i for i in good if table[i] == table[dup])
    rest = [i for i in good if i != twice]
    pick = dict(zip(ERASE_PICKS, rest[:5] + [twice]))
    n_obs = dict(set_bad=3, erase_cascade=2, erase_match=4, erase_keep=4, cull=3, twice=3)
    extra = [m.add_keyframe([table[pick[n]] for n in ERASE_PICKS] + [-1, -1]) for _ in range(3)]
    for j, n in enumerate(ERASE_PICKS):
        p = table[pick[n]]
        assert m.add_observation(p, slot, pick[n])
        for k in extra[:n_obs[n] - 1]:
            assert m.add_observation(p, k, j)
    m.points[table[pick["cull"]]].found, m.points[table[pick["cull"]]].visible = 1, 10
    return pick


def apply_after(model, sc, store=None):
    """The scene's mutations after the snapshot, on the model and, when given, the same ones on a MapPointStore."""
    for op in sc["after"]:
        if op[0] == "move":
            model.move_points(op[1], op[2])
            if store is not None and len(op[1]):
                store.update_points(op[1], xyz=op[2])
        elif op[0] == "bad":
            model.points[op[1]].bad = True
            if store is not None:
                store.set_points_bad([op[1]])
        elif op[0] == "facet_off":
            del model.facet[op[1]]
            if store is not None:
                store.set_embedding([op[1]], [[-1, -1, -1]])
        else:
            model.set_table(sc["slot"], op[1], op[2])
            if store is not None:
                store.set_keyframe_point(sc["slot"], op[1], op[2])


def fill_store(model, store, kf_store=None):
    """The model into an empty MapPointStore (and KeyFrameStore), facets included."""
    model.fill(store, kf_store)
    ids = sorted(model.facet)
    if ids:
        store.set_embedding(ids, [model.facet[p] for p in ids], np.full((len(ids), 3), 1 / 3))
