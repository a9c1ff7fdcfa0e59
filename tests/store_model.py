"""TEST INFRASTRUCTURE ONLY: the state of the two resident stores (the map point store and the keyframe store), once.

MapModel holds what the stores hold and nothing else: the points, the keyframes, and the log of observation records in arrival order with
blanked erasures.  It contains no reference logic; the restatements (local_map_ref, track_close_ref, motion_model_ref,
template_switch_ref, anchor_pairs_ref, keyframe_insert_ref, point_erase_ref) are classes over it that add their own.  Also here: the one
replay of a model into a MapPointStore (and a KeyFrameStore), the read-back of a store in the same shape, and the text file of a model
that the compiled drivers read (integration/standin_store_scene.h) with the parser of what they dump.
Nothing in defslam_amd/ imports this module.
"""
from __future__ import annotations

import numpy as np


class Point:
    def __init__(self, xyz, normal, max_distance, desc, bad, ref, found, visible):
        self.xyz = np.asarray(xyz, np.float32).reshape(3).copy()
        self.normal = np.asarray(normal, np.float32).reshape(3).copy()
        self.max_distance = np.float32(max_distance)
        self.min_distance = np.float32(0)
        self.desc = np.asarray(desc, np.uint8).reshape(32).copy()
        self.bad = bool(bad)                 # MapPoint::isBad
        self.ref = int(ref)                  # MapPoint::GetReferenceKeyFrame as a slot, -1: none
        self.n_obs = 0                       # MapPoint::nObs: it is not len(obs) once setBadFlag has cleared the observations
        self.found = int(found)              # mnFound
        self.visible = int(visible)          # mnVisible
        self.obs = {}                        # mObservations: keyframe slot -> key point index, -1: added without one


class KeyFrame:
    def __init__(self, table, parent, bad, Ow, desc, octave, scale_factors):
        self.table = [int(p) for p in table]     # mvpMapPoints: a point id or -1 per key point
        self.parent = int(parent)
        self.bad = bool(bad)                     # the flag of both stores
        self.has_appearance = desc is not None   # what mappoint_ref reads of a keyframe; absent in a topology-only scene
        if self.has_appearance:
            self.Ow = np.asarray(Ow, np.float32).reshape(3).copy()
            self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32).copy()
            self.octave = np.asarray(octave, np.int32).reshape(-1).copy()
            self.scale_factors = np.asarray(scale_factors, np.float32).reshape(-1).copy()
            assert len(self.table) == self.desc.shape[0] == self.octave.shape[0]


class MapModel:
    def __init__(self):
        self.points = []
        self.kfs = []
        self.log = []            # [point, slot, idx, live] in arrival order: an erased record keeps its place, blanked
        self._live = {}          # (point, slot) -> its live record

    # ---- the mutations of the stores ----
    def add_point(self, xyz=(0, 0, 1), normal=(0, 0, 1), max_distance=1.0, desc=None, bad=False, ref=-1, found=1, visible=1):
        self.points.append(Point(xyz, normal, max_distance, np.zeros(32, np.uint8) if desc is None else desc, bad, ref, found, visible))
        return len(self.points) - 1

    def add_keyframe(self, table, parent=-1, bad=False, Ow=None, desc=None, octave=None, scale_factors=None):
        self.kfs.append(KeyFrame(table, parent, bad, Ow, desc, octave, scale_factors))
        return len(self.kfs) - 1

    def live(self, p, s):
        return (p, s) in self._live

    def add_observation(self, p, s, idx=-1):
        """MapPoint::AddObservation (MapPoint.cc:109-120, monocular): False on a pair that is live already."""
        p, s, idx = int(p), int(s), int(idx)
        if self.live(p, s):
            return False
        assert -1 <= idx < len(self.kfs[s].table)
        self.log.append([p, s, idx, True])
        self._live[(p, s)] = self.log[-1]
        self.points[p].obs[s] = idx
        self.points[p].n_obs += 1
        return True

    def erase_observation(self, p, s):
        """The record of a live pair is blanked and nObs goes down; False when the pair is not live."""
        p, s = int(p), int(s)
        r = self._live.pop((p, s), None)
        if r is None:
            return False
        r[3] = False
        del self.points[p].obs[s]
        self.points[p].n_obs -= 1
        return True

    def observations(self, p):
        """The live observations of p as (slot, idx), by ascending slot."""
        return sorted(self.points[p].obs.items())

    # ---- the replay ----
    def fill(self, st, kf_store=None, batches=1):
        """The model's state into an empty localmap.MapPointStore, and into a mappoint.KeyFrameStore when given.  The device log ends up
        in the model's log order, blanked records too, in as few calls as the records allow: a pair that is in the batch already (erased
        and added again) closes the batch, so does a change between records with and without a key point index, and a batch's erased
        records are blanked right after it.  batches > 1 splits every batch further.  The replay cannot make nObs differ from the
        number of live records, so the model must not have run setBadFlag yet."""
        P = len(self.points)
        assert all(pt.n_obs == len(pt.obs) for pt in self.points), "fill: a point's n_obs is not the number of its live observations"
        if P:
            st.add_points(np.stack([pt.xyz for pt in self.points]), np.stack([pt.normal for pt in self.points]),
                          np.array([pt.max_distance for pt in self.points], np.float32), np.stack([pt.desc for pt in self.points]),
                          np.array([pt.bad for pt in self.points], np.uint8))
            st.set_counters(np.arange(P), [pt.visible for pt in self.points], [pt.found for pt in self.points])
        for s, k in enumerate(self.kfs):
            if kf_store is not None:
                from defslam_amd import mappoint
                assert kf_store.add(mappoint.MpKeyFrame(k.Ow, k.desc, k.octave, k.scale_factors, bad=k.bad)) == s
            # a parent that comes later in slot order is set once it exists
            assert st.add_keyframe(np.array(k.table, np.int32), k.parent if k.parent < s else -1, k.bad) == s
        for s, k in enumerate(self.kfs):
            if k.parent > s:
                st.set_keyframe_parent(s, k.parent)
        runs, pairs = [], set()
        for r in self.log:
            if not runs or (r[0], r[1]) in pairs or (r[2] < 0) != (runs[-1][0][2] < 0):
                runs.append([])
                pairs.clear()
            pairs.add((r[0], r[1]))
            runs[-1].append(r)
        for run in runs:
            for part in np.array_split(np.array(run, np.int32), batches):
                if len(part):
                    st.add_observations(part[:, 0], part[:, 1], idx=None if part[0, 2] < 0 else part[:, 2])
                    gone = part[part[:, 3] == 0]
                    if len(gone):
                        st.erase_observations(gone[:, 0], gone[:, 1])
        if P:
            st.set_reference_keyframes(np.arange(P), [pt.ref for pt in self.points])

    # ---- read-backs in the shape of the store's ----
    def state(self):
        P = len(self.points)
        return dict(bad=np.array([pt.bad for pt in self.points], bool).reshape(P),
                    n_obs=np.array([pt.n_obs for pt in self.points], np.int32).reshape(P),
                    ref=np.array([pt.ref for pt in self.points], np.int32).reshape(P),
                    obs=[dict(self.observations(p)) for p in range(P)],
                    tables=[list(kf.table) for kf in self.kfs])

    def point_arrays(self):
        """xyz, normal, max_distance, desc and bad of every point, as MapPointStore.get_points() returns them."""
        P = len(self.points)
        return dict(xyz=np.array([pt.xyz for pt in self.points], np.float32).reshape(P, 3),
                    normal=np.array([pt.normal for pt in self.points], np.float32).reshape(P, 3),
                    max_distance=np.array([pt.max_distance for pt in self.points], np.float32).reshape(P),
                    desc=np.array([pt.desc for pt in self.points], np.uint8).reshape(P, 32), bad=np.array([pt.bad for pt in self.points], bool))


def store_state(st):
    """The dict of MapModel.state() read back from a MapPointStore."""
    P = st.n_points
    o = st.observations()
    return dict(bad=st.get_points().bad, n_obs=st.get_state().n_obs, ref=st.get_reference_keyframes(),
                obs=[o.of(p) for p in range(P)], tables=[st.keyframe_table(s).tolist() for s in range(st.n_keyframes)])


def assert_state(st, model, what=""):
    g, r = store_state(st), model.state()
    for n in ("bad", "n_obs", "ref"):
        assert np.array_equal(np.asarray(g[n]).astype(np.int64), r[n].astype(np.int64)), (what, n, g[n], r[n])
    assert g["obs"] == r["obs"], (what, "obs", [(p, a, b) for p, (a, b) in enumerate(zip(g["obs"], r["obs"])) if a != b])
    assert g["tables"] == r["tables"], (what, "tables", [(s, a, b) for s, (a, b) in enumerate(zip(g["tables"], r["tables"])) if a != b])


# ---- the scene file of the compiled drivers ------------------------------------------------------------------------------------------------

def _floats(v):
    return " ".join(repr(float(x)) for x in np.asarray(v, np.float32).reshape(-1))


def _ints(v):
    return " ".join(str(int(x)) for x in np.asarray(v).reshape(-1))


def write_scene(model, path, tail=""):
    """The text file StoreScene::read reads (integration/standin_store_scene.h), floats by repr:
      "store_scene P K R appearance"
      P lines   "x y z nx ny nz max_distance min_distance bad ref n_obs found visible d0 .. d31"
      K blocks  "N parent bad t0 .. tN-1", and with appearance "Owx Owy Owz levels sf0 .." and N lines "octave d0 .. d31"
      R lines   "point slot idx live"
    and after these the tail, which the driver reads itself."""
    appearance = bool(model.kfs) and all(k.has_appearance for k in model.kfs)
    with open(path, "w") as f:
        f.write(f"store_scene {len(model.points)} {len(model.kfs)} {len(model.log)} {int(appearance)}\n")
        for pt in model.points:
            f.write(f"{_floats(pt.xyz)} {_floats(pt.normal)} {_floats(pt.max_distance)} {_floats(pt.min_distance)} {int(pt.bad)} {pt.ref} {pt.n_obs} "
                    f"{pt.found} {pt.visible} {_ints(pt.desc)}\n")
        for k in model.kfs:
            f.write(f"{len(k.table)} {k.parent} {int(k.bad)} {_ints(k.table)}\n")
            if appearance:
                f.write(f"{_floats(k.Ow)} {len(k.scale_factors)} {_floats(k.scale_factors)}\n")
                for j in range(len(k.table)):
                    f.write(f"{int(k.octave[j])} {_ints(k.desc[j])}\n")
        for p, s, idx, live in model.log:
            f.write(f"{p} {s} {idx} {int(live)}\n")
        f.write(tail if tail.endswith("\n") or not tail else tail + "\n")


def parse_dump(path):
    """The lines "route step kind ..." of a driver's dump -> {(route, step): dict}, the dict with one entry per kind it met:
      recent  id ..                                       -> recent
      pt      p bad n_obs ref found visible | xyz normal max_distance min_distance (eight bit patterns) | d0 .. d31 | slot:idx ..
                                                          -> bad, n_obs, ref, found, visible, bits, desc, obs: a list each, by point
      kf      slot parent bad t0 .. tN-1                  -> parents, kf_bad, tables
      anchor  slot count n_pairs fits | idx1:idx2:own .. | j ..   -> anchors: [(slot, count, n_pairs, fits, [(idx1, idx2, own)], [j])]
      has     h ..                                        -> has
      no_ref  n                                           -> no_ref
    bad, n_obs, ref, obs and tables have the shape of MapModel.state().  Lines of another kind (a timing) are left out."""
    out = {}
    for ln in open(path).read().splitlines():
        w = ln.split()
        if len(w) < 3 or w[2] not in ("recent", "pt", "kf", "anchor", "has", "no_ref"):
            continue
        d = out.setdefault((w[0], w[1]), {})
        if w[2] == "recent":
            d["recent"] = [int(x) for x in w[3:]]
        elif w[2] == "has":
            d["has"] = [int(x) for x in w[3:]]
        elif w[2] == "no_ref":
            d["no_ref"] = int(w[3])
        elif w[2] == "anchor":
            head, pairs, queries = " ".join(w[3:]).split("|")
            d.setdefault("anchors", []).append(tuple(int(x) for x in head.split()) + ([tuple(map(int, p.split(":"))) for p in pairs.split()],
                                                                                      [int(j) for j in queries.split()]))
        elif w[2] == "kf":
            assert int(w[3]) == len(d.setdefault("tables", []))
            for n, v in (("parents", int(w[4])), ("kf_bad", bool(int(w[5]))), ("tables", [int(x) for x in w[6:]])):
                d.setdefault(n, []).append(v)
        else:
            head, bits, desc, obs = " ".join(w[3:]).split("|")
            p, bad, n_obs, ref, found, visible = (int(x) for x in head.split())
            assert p == len(d.setdefault("bad", []))
            for n, v in (("bad", bool(bad)), ("n_obs", n_obs), ("ref", ref), ("found", found), ("visible", visible), ("bits", [int(x) for x in bits.split()]),
                         ("desc", [int(x) for x in desc.split()]), ("obs", {int(a): int(b) for a, b in (x.split(":") for x in obs.split())})):
                d.setdefault(n, []).append(v)
    return out


def dump_of(model, recent=()):
    """What parse_dump returns for a dump of the model's state with the list `recent`."""
    s = model.state()
    return dict(recent=[int(p) for p in recent], bad=s["bad"].tolist(), n_obs=s["n_obs"].tolist(), ref=s["ref"].tolist(), found=[pt.found for pt in model.points],
                visible=[pt.visible for pt in model.points], desc=[pt.desc.tolist() for pt in model.points], obs=s["obs"], tables=s["tables"],
                parents=[k.parent for k in model.kfs], kf_bad=[k.bad for k in model.kfs],
                bits=[np.concatenate([pt.xyz, pt.normal, [pt.max_distance, pt.min_distance]]).astype(np.float32).view(np.uint32).tolist() for pt in model.points])
