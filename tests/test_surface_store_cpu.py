"""CPU tests of the resident Surface of a keyframe (dsh_keyframe_surface_init, _set_depth, _set_points, _set_normals, _take_normals,
_gather, _get, _vertices, dsh_keyframe_sfn): the binding, the header's constraint on the new prototypes, the order of checks on a
host-only context, the restatement tests/surface_store_ref.py against a second transcription of obtainM's loop, setNormalSurfacePoint's
count and applyScale on SurfacePoint-like objects, and the oracle's verdict on every scene whose numbers the GPU test compares.
Integers and bytes are compared exactly."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import surface_store_ref as SS
from conftest import ROOT

OK, ARG, STATE, NODEV = 0, 1, 3, 4
NEW_ENTRIES = ("dsh_keyframe_surface_init", "dsh_keyframe_surface_set_depth", "dsh_keyframe_surface_set_points", "dsh_keyframe_surface_set_normals",
               "dsh_keyframe_surface_take_normals", "dsh_keyframe_surface_gather", "dsh_keyframe_surface_get", "dsh_keyframe_surface_vertices",
               "dsh_keyframe_sfn")
# the scenes whose numbers test_surface_store_gpu compares: (N, sites, nptsu, nptsv)
SFN_CASES = ((1200, 10, 13, 15), (1200, 64, 13, 15), (1200, 65, 13, 15), (1200, 600, 13, 15), (8192, 8192, 13, 15), (1200, 600, 6, 7), (300, 64, 6, 7))
BENDING_WEIGHT = 1e-3


def sfn_scene(N, n_sites, nu, nv):
    sc = SS.make_surface_scene(N, seed=5, n_sites=n_sites, nu=nu, nv=nv)
    m, slot = sc["model"], sc["slot"]
    m.surface_init(slot, sc["kpn"])
    ents = sorted(sc["normals"])
    m.set_normals([slot] * len(ents), ents, [sc["normals"][i] for i in ents])
    m.set_bad(sc["emptied"])
    return sc


def test_new_symbols_are_bound():
    from defslam_amd import _lib, localmap
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "defslam_hip.h")).read()
    declared = set(re.findall(r"\b(dsh_[a-z0-9_]+)\s*\(", header))
    for n in NEW_ENTRIES:
        assert n in declared and n in _lib.EXPORTED_SYMBOLS and getattr(L, n).argtypes is not None, n
    assert C.sizeof(_lib.KeyframeSurfaceInfoC) == 16 + C.sizeof(_lib.BbsC) and C.sizeof(_lib.KeyframeSfnResultC) == 24
    assert C.sizeof(_lib.KeyframeSfnInputC) == 40 and _lib.KeyframeSfnInputC.bending_weight.offset == 24
    assert C.sizeof(_lib.SurfaceTakeInputC) == 40 and _lib.SurfaceTakeInputC.sel.offset == 16
    for m in ("surface_init", "surface_set_depth", "surface_set_points", "surface_set_normals", "surface_take_normals", "surface_gather", "surface_get",
              "sfn", "surface_vertices"):
        assert callable(getattr(localmap.MapPointStore, m))


def _lib_symbols():
    from defslam_amd import _lib
    return _lib.EXPORTED_SYMBOLS


def test_new_prototypes_stay_out_of_the_host_only_table():
    """As for the registration's entries (tests/test_surface_register_store_cpu.py): every new entry takes the point store alone -- the
    database of dsh_keyframe_surface_take_normals and the context of dsh_keyframe_sfn travel in their input structs -- so none of them
    may be matched by the pattern of tests/test_abi_and_host.py, by a prototype or by a comment."""
    header = open(os.path.join(ROOT, "include", "defslam_hip.h")).read()
    takes = set(re.findall(r"\b(dsh_[a-z0-9_]+)\s*\((?:[^)]*\b(?:dsh_ctx|dsh_diffdb|dsh_kfdb|dsh_comm)\b)", header))
    assert not takes & set(NEW_ENTRIES), takes & set(NEW_ENTRIES)
    assert "nodesDepth_ stays with the caller;" not in header


def _rows(keep, ctx_h):
    """(entry, arguments after the store handle, part of the message) for an EMPTY store, in the order of the checks."""
    from defslam_amd import _lib
    f = np.zeros(16, np.float32)
    d = np.zeros(512, np.float64)
    ip = np.zeros(4, np.int32)
    u8 = np.zeros(4, np.uint8)
    keep += [f, d, ip, u8]
    fp, dp, ipp, up = (a.ctypes.data_as(C.POINTER(t)) for a, t in ((f, C.c_float), (d, C.c_double), (ip, C.c_int32), (u8, C.c_uint8)))
    bbs = _lib.BbsC(-1.0, 1.0, 13, -1.0, 1.0, 15, 1)
    res = _lib.KeyframeSfnResultC()
    fake = C.c_void_p(1)                                # never dereferenced: the checks that come first refuse
    take = lambda n, ddb=None, arr=ipp: _lib.SurfaceTakeInputC(ddb, n, arr, arr, arr)
    sfn = lambda ctx=ctx_h, slot=0: _lib.KeyframeSfnInputC(ctx, slot, C.pointer(bbs), 1e-3, 1.0)
    rows = [
        ("dsh_keyframe_surface_init", (0, 0, None), "slot outside the store"),
        ("dsh_keyframe_surface_set_depth", (0, C.byref(bbs), dp), "slot outside the store"),
        ("dsh_keyframe_surface_set_points", (-1, 0, None, None), "slot outside the store"),
        ("dsh_keyframe_surface_set_normals", (-1, None, None, None, None), "n < 0"),
        ("dsh_keyframe_surface_set_normals", (1, None, ipp, fp, None), "slot or idx is NULL"),
        ("dsh_keyframe_surface_set_normals", (1, ipp, ipp, fp, None), "target 0: slot outside the store"),
        ("dsh_keyframe_surface_take_normals", (None, None), "in is NULL"),
        ("dsh_keyframe_surface_take_normals", (take(-1), None), "n < 0"),
        ("dsh_keyframe_surface_take_normals", (take(1, fake), None), "target 0: slot outside the store"),
        ("dsh_keyframe_surface_take_normals", (take(0), None), "ddb is NULL"),
        ("dsh_keyframe_surface_take_normals", (take(0, fake), None), "belongs to another context or was detached"),
        ("dsh_keyframe_surface_gather", (-1, None, None, None, None, None), "n < 0"),
        ("dsh_keyframe_surface_gather", (1, ipp, ipp, fp, up, fp), "target 0: slot outside the store"),
        ("dsh_keyframe_surface_get", (0, 0, None, None, None, None, None, None), "slot outside the store"),
        ("dsh_keyframe_surface_vertices", (0, fp, 4, 4, dp), "slot outside the store"),
        ("dsh_keyframe_sfn", (None, None, None, None, C.byref(res)), "in is NULL"),
        ("dsh_keyframe_sfn", (sfn(), None, None, None, None), "out is NULL"),
        ("dsh_keyframe_sfn", (sfn(ctx=None), None, None, None, C.byref(res)), "in->ctx is not the context of the store"),
        ("dsh_keyframe_sfn", (sfn(), None, None, None, C.byref(res)), "slot outside the store"),
    ]
    keep += [bbs, res, rows]
    return rows


def test_order_of_checks_on_a_host_only_context(host_ctx):
    """Arguments first, each DSH_ERR_ARG with a message that names the entry.  A host-only store stays empty, so every entry that names
    a keyframe is refused by its arguments; the two that can be well-formed without one (no targets) reach the device gate, which says
    "host-only"."""
    from test_local_map_cpu import _raw_store
    L = host_ctx._L
    msg = lambda: L.dsh_last_error(host_ctx._h).decode()
    rc, h = _raw_store(L, host_ctx._h)
    assert rc == OK and h
    keep = []
    rows = _rows(keep, host_ctx._h)
    assert {r[0] for r in rows} == set(NEW_ENTRIES)
    for name, args, part in rows:
        a = [C.byref(x) if isinstance(x, C.Structure) else x for x in args]
        assert getattr(L, name)(h, *a) == ARG, (name, part)
        assert name in msg() and part in msg(), (name, part, msg())
        assert getattr(L, name)(None, *a) == ARG, (name, "NULL store")
    # the state is a read of the host mirror, not a status: -1 for a slot outside the store and for no store
    assert "dsh_keyframe_surface_state" in _lib_symbols() and L.dsh_keyframe_surface_state(h, 0) == -1 and L.dsh_keyframe_surface_state(None, 0) == -1
    assert L.dsh_keyframe_surface_set_normals(h, 0, None, None, None, None) == NODEV and "host-only" in msg()
    assert L.dsh_keyframe_surface_gather(h, 0, None, None, None, None, None) == NODEV and "host-only" in msg()
    assert L.dsh_mpdb_destroy(h) == OK


def test_a_detached_store_refuses_every_entry():
    from defslam_amd import sft
    from test_local_map_cpu import _raw_store
    ctx = sft.Context(-1)
    L = ctx._L
    rc, h = _raw_store(L, ctx._h)
    assert rc == OK
    keep = []
    rows = _rows(keep, ctx._h)
    ctx.close()                                        # dsh_destroy detaches the store
    for name, args, _ in rows:
        a = [C.byref(x) if isinstance(x, C.Structure) else x for x in args]
        assert getattr(L, name)(h, *a) == ARG, name
    assert L.dsh_mpdb_destroy(h) == OK


# ---- the restatement against a second transcription --------------------------------------------------------------------------------------

class _SurfacePoint:
    """defSLAM::SurfacePoint (Modules/Mapping/SurfacePoint.cc)."""

    def __init__(self):
        self.NormalOn, self.Normal, self.x3D = False, None, np.zeros(3, np.float32)

    def setNormal(self, N):
        self.Normal, self.NormalOn = N.copy(), True

    def getNormal(self, out):
        if not self.NormalOn:
            return False
        out[:] = self.Normal
        return True

    def thereisNormal(self):
        return self.NormalOn


class _Surface:
    """Surface.cc, line by line, on objects."""

    def __init__(self, n):
        self.surfacePoints_, self.numberofNormals_, self.normalsLimit_, self.nodesDepth_ = [_SurfacePoint() for _ in range(n)], 0, 10, None

    def setNormalSurfacePoint(self, ind, N):           # :76-85
        if not self.surfacePoints_[ind].thereisNormal():
            self.numberofNormals_ += 1
        self.surfacePoints_[ind].setNormal(N)

    def getNormalSurfacePoint(self, ind, N):           # :88-91
        return self.surfacePoints_[ind].getNormal(N)

    def enoughNormals(self):                           # :62-67
        return self.numberofNormals_ >= self.normalsLimit_

    def applyScale(self, s22):                         # :107-121
        for sp in self.surfacePoints_:
            x3D = sp.x3D.copy()
            sp.x3D = (np.float64(s22) * x3D.astype(np.float64)).astype(np.float32)
        for i in range(len(self.nodesDepth_)):
            self.nodesDepth_[i] = s22 * self.nodesDepth_[i]


class _MP:
    def __init__(self, bad):
        self.bad = bad

    def isBad(self):
        return self.bad


def _obtain_m_walk(mvpMapPoints, sref, mpKeypointNorm):
    """ShapeFromNormals.cc:190-210, line by line: (Normals, u_vector_, v_vector_, the key points that made a site)."""
    Normals, u_vector_, v_vector_, which = [], [], [], []
    for var in range(len(mvpMapPoints)):
        Normal = np.zeros(3, np.float32)
        mp = mvpMapPoints[var]
        if not mp:
            continue
        if mp.isBad():
            continue
        if sref.getNormalSurfacePoint(var, Normal):
            if (Normal == Normal).all():               # cv::Vec3f operator==: every component equal to itself
                Normals.append(Normal)
                u_vector_.append(float(mpKeypointNorm[var][0]))
                v_vector_.append(float(mpKeypointNorm[var][1]))
                which.append(var)
    return np.array(Normals, np.float32).reshape(-1, 3), np.array(u_vector_), np.array(v_vector_), which


@pytest.mark.parametrize("N,seed,hold", [(40, 0, 0.5), (64, 1, 0.7), (257, 2, 0.5), (48, 3, 0.4), (20, 4, 0.5), (64, 5, 1.0), (64, 6, 0.0), (0, 7, 0.5), (1, 8, 1.0)])
def test_restatement_equals_the_transcription_on_random_scenes(N, seed, hold):
    sc = SS.make_surface_scene(N, seed, hold=hold)
    m, slot = sc["model"], sc["slot"]
    m.surface_init(slot, sc["kpn"])
    with pytest.raises(SS.SurfaceExists):
        m.surface_init(slot, sc["kpn"])
    sref = _Surface(N)
    first, second = SS.normal_calls(sc, seed)
    for slots, idx, nr in (first, second):
        before = sref.numberofNormals_
        for i, n in zip(idx, nr):
            sref.setNormalSurfacePoint(int(i), n)
        got = m.set_normals(slots, idx, nr)
        assert (got == sref.numberofNormals_).all() and m.surface[slot].n_normals == sref.numberofNormals_
        if slots is second[0]:
            assert before == sref.numberofNormals_       # entries that hold a normal already are not counted again
    assert sref.numberofNormals_ == len(sc["normals"]) and m.surface[slot].enough_normals == sref.enoughNormals()
    for i, sp in enumerate(sref.surfacePoints_):         # a target named twice kept the later normal
        assert sp.NormalOn == (i in sc["normals"]) == bool(m.surface[slot].has[i])
        if sp.NormalOn:
            assert sp.Normal.tobytes() == sc["normals"][i].tobytes() == m.surface[slot].normal[i].tobytes()
    m.set_bad(sc["emptied"])
    objs = [_MP(m.points[p].bad) if p >= 0 else None for p in m.kfs[slot].table]
    Normals, u, v, which = _obtain_m_walk(objs, sref, sc["kpn"])
    c, w, mu, mv, mn = m.sfn_select(slot)
    assert w.tolist() == which and mn.tobytes() == Normals.tobytes() and mu.tobytes() == u.tobytes() and mv.tobytes() == v.tobytes()
    assert sum(c.values()) == N and c["n_sites"] == len(which)
    if N >= 32 and 0 < hold < 1:                         # the specials are there and do what they promise
        r = sc["roles"]
        assert c["n_nan"] == 3 and c["n_bad"] >= 1 and c["n_no_normal"] >= 1 and r.index("inf") in which and r.index("dup") in which
        assert r.index("emptied") not in which and m.kfs[slot].table[r.index("emptied")] == -1 and c["n_empty"] == r.count("empty") + 1
    # the gather: x0 / has_x0 / ref_uv
    nxy, has, uv = m.gather([slot] * N, list(range(N)))
    for i in range(N):
        Ni = np.zeros(3, np.float32)
        h = sref.getNormalSurfacePoint(i, Ni)
        assert bool(has[i]) == h and nxy[i].tobytes() == (Ni[:2] if h else np.zeros(2, np.float32)).tobytes() and uv[i].tobytes() == sc["kpn"][i].tobytes()
    # applyScale of points and depth
    rng = np.random.default_rng(seed)
    pts, ctrl = rng.standard_normal((N, 3)).astype(np.float32), rng.standard_normal(13 * 15)
    m.sfn_write(slot, sc["bbs"], ctrl, pts)
    for sp, x in zip(sref.surfacePoints_, pts):
        sp.x3D = x.copy()
    sref.nodesDepth_ = ctrl.tolist()
    m.apply_scale(slot, 1.37)
    sref.applyScale(1.37)
    assert m.surface[slot].pts.tobytes() == np.array([sp.x3D for sp in sref.surfacePoints_], np.float32).reshape(N, 3).tobytes()
    assert m.surface[slot].ctrl.tobytes() == np.array(sref.nodesDepth_).tobytes()


@pytest.mark.parametrize("N,n_sites,nu,nv", SFN_CASES)
def test_every_scene_the_gpu_test_solves_is_solvable(oracle_mod, N, n_sites, nu, nv):
    """The scenes whose numbers test_surface_store_gpu compares have exactly the sites they promise, and the oracle's estimate() on the
    restatement's sites returns ok: they are known to be solvable before any GPU sees them."""
    sc = sfn_scene(N, n_sites, nu, nv)
    m, slot = sc["model"], sc["slot"]
    c, w, u, v, nr = m.sfn_select(slot)
    assert c["n_sites"] == n_sites and sum(c.values()) == N
    if N > n_sites:
        assert (c["n_bad"], c["n_no_normal"], c["n_nan"]) == (1, 1, 3) and c["n_empty"] >= 1
    assert sc["bbs"][2] == nu and sc["bbs"][5] == nv
    kpn = sc["kpn"].astype(np.float64)
    ok, raw, ctrl, pts = oracle_mod.sfn_estimate(sc["bbs"], u, v, nr, BENDING_WEIGHT, sc["mean_depth"], kpn[:, 0].copy(), kpn[:, 1].copy())
    assert ok and np.isfinite(raw).all() and np.isfinite(pts).all() and pts.shape == (N, 3)
