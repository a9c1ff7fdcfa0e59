"""GPU tests of the resident Surface of a keyframe: its bookkeeping (dsh_keyframe_surface_init, _set_depth, _set_points, _set_normals,
_take_normals, _gather, _get) against the restatement tests/surface_store_ref.py, the selection and the numbers of dsh_keyframe_sfn against
the restatement's sites handed to dsh_sfn_estimate and to the oracle, and the chain: the registration and the template switch with the
resident surface points instead of an uploaded array, Surface::applyScale of the resident copy, dsh_keyframe_surface_vertices.  Bytes and
integers, no tolerance, except where the oracle (another algorithm) is the reference."""
import numpy as np
import pytest

import surface_register_ref as SR
import surface_store_ref as SS
from test_surface_register_store_gpu import everything
from test_surface_store_cpu import BENDING_WEIGHT, SFN_CASES

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 8192)


@pytest.fixture(scope="module")
def ctx():
    """A context of its own: the chain replaces the context's template."""
    from defslam_amd import sft
    c = sft.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def solved(ctx):
    """A DiffProp database on the context and its last normal solve, downloaded: the source of dsh_keyframe_surface_take_normals."""
    from defslam_amd import nrsfm, synth
    sc = synth.make_normals_scene(n_points=120, n_views=3, seed=9, nonref_frac=0.0)
    db = nrsfm.DiffDatabase(ctx, 16)
    R = sc["recs"].shape[0]
    db.append(sc["recs"], np.repeat(np.arange(120, dtype=np.int32), np.diff(sc["rec_ptr"])), np.arange(R, dtype=np.int32) % 5, np.arange(R, dtype=np.int32))
    d = nrsfm.ObtainK1K2Database(ctx, db, np.arange(120, dtype=np.int32), sc["x0"], sc["has_x0"], sc["ref_uv"])
    assert (d.status == 0).sum() >= 10 and d.rec_written.sum() >= 10
    yield db, d
    db.close()


def stores(ctx, model, with_kf=False):
    from defslam_amd import localmap, mappoint
    st = localmap.MapPointStore(ctx, points=64, keyframes=2, observations=64)
    ks = mappoint.KeyFrameStore(ctx, 1) if with_kf else None
    SR.fill_store(model, st, ks)
    return st, ks


def check_surface(st, m, slot):
    """surface_get against the restatement: every field, bytes."""
    g, w = st.surface_get(slot), m.surface[slot]
    assert g.normals.tobytes() == w.normal.tobytes() and g.has_normal.tolist() == w.has.tolist()
    assert g.pts.tobytes() == w.pts.tobytes() and g.kpn.tobytes() == w.kpn.tobytes()
    assert g.n_normals == w.n_normals and g.enough_normals == w.enough_normals
    assert (g.ctrl is None) == (w.ctrl is None)
    if w.ctrl is not None:
        assert g.ctrl.tobytes() == w.ctrl.tobytes()
        assert (g.bbs.umin, g.bbs.umax, g.bbs.nptsu, g.bbs.vmin, g.bbs.vmax, g.bbs.nptsv, g.bbs.valdim) == tuple(w.bbs)
    return g


def prepare(ctx, sc, with_kf=False):
    """The scene in a store and in its model: Surface of both keyframes, the scene's normals in two calls, the emptied entry."""
    m, slot = sc["model"], sc["slot"]
    st, ks = stores(ctx, m, with_kf)
    st.surface_init(slot, sc["kpn"])
    m.surface_init(slot, sc["kpn"])
    for slots, idx, nr in SS.normal_calls(sc):
        assert st.surface_set_normals(slots, idx, nr).tolist() == m.set_normals(slots, idx, nr).tolist()
    if sc["emptied"]:
        st.set_bad_full(sc["emptied"])
        m.set_bad(sc["emptied"])
    return st, ks, m, slot


@pytest.mark.parametrize("N", SIZES)
def test_bookkeeping_equals_the_restatement(ctx, solved, N):
    """init, normals from the host and from the last normal solve (repeated targets inside a call, targets in two keyframes, a second
    call on entries that hold a normal already), points, depth, gather and get; take_normals equals set_normals fed with the normals the
    solve downloaded; a second init is refused; dsh_mpdb_clear forgets everything."""
    from defslam_amd import nrsfm, sft
    db, d = solved
    sc = SS.make_surface_scene(N, seed=1, hold=0.5)
    m, slot = sc["model"], sc["slot"]
    st, _ = stores(ctx, m)
    tw, _ = stores(ctx, m)
    rng = np.random.default_rng(N)
    n0 = len(m.kfs[0].table)                                                        # the keyframe in front: two to five entries
    kpn0 = rng.uniform(-0.5, 0.5, (n0, 2)).astype(np.float32)
    with pytest.raises(sft.DshError, match="status 1: dsh_keyframe_surface_get: keyframe 1 has no resident surface"):
        st.surface_get(slot)
    with pytest.raises(sft.DshError, match=r"status 1: dsh_keyframe_surface_init: N \(1\) is not the N of keyframe 0"):
        st.surface_init(0, kpn0[:1])
    for s in (st, tw, m):
        s.surface_init(slot, sc["kpn"])
        s.surface_init(0, kpn0)
    with pytest.raises(sft.DshError, match="status 3: dsh_keyframe_surface_init: keyframe 1 has a resident surface already"):
        st.surface_init(slot, sc["kpn"])
    for k in (0, slot):
        check_surface(st, m, k)                                                     # no normal, zeros, the key points
    # the targets of the scene's two calls, with the front keyframe's entries mixed into the first (one of them twice)
    (s1, i1, _), (s2, i2, _) = SS.normal_calls(sc, seed=N)
    s1, i1 = np.r_[[0, 0], s1, [0, 0]].astype(np.int32), np.r_[[n0 - 1, 0], i1, [n0 - 1, 0]].astype(np.int32)
    okp, okr = np.flatnonzero(d.status == 0), np.flatnonzero(d.rec_written)
    for slots, idx in ((s1, i1), (s2, i2)):
        sel = np.where(rng.random(len(idx)) < 0.5, rng.choice(okp, len(idx)), -1 - rng.choice(okr, len(idx))).astype(np.int32)
        nr = np.where((sel >= 0)[:, None], d.normal_ref[np.maximum(sel, 0)], d.normal_rec[np.maximum(-1 - sel, 0)]).astype(np.float32)
        before = [m.surface[0].n_normals, m.surface[slot].n_normals]
        want = m.set_normals(slots, idx, nr)
        assert st.surface_take_normals(db, sel, slots, idx).tolist() == want.tolist()
        assert tw.surface_set_normals(slots, idx, nr).tolist() == want.tolist()
        if slots is s2:
            assert before == [m.surface[0].n_normals, m.surface[slot].n_normals]   # the second call sets no new entry: the count does not move
        for k in (0, slot):
            a, b = check_surface(st, m, k), check_surface(tw, m, k)
            assert a.normals.tobytes() == b.normals.tobytes()
    assert m.surface[0].n_normals == 2 and m.surface[slot].n_normals == len(sc["normals"])
    # points and depth
    pick = rng.permutation(N)[:N // 2 + 1 if N else 0].astype(np.int32)
    pts = rng.standard_normal((len(pick), 3)).astype(np.float32)
    ctrl = rng.uniform(0.5, 2.0, 6 * 7)
    bbs = (-0.7, 0.7, 6, -0.6, 0.6, 7, 1)
    st.surface_set_points(slot, pick, pts)
    m.set_points(slot, pick, pts)
    st.surface_set_depth(slot, nrsfm.Bbs(*bbs), ctrl)
    m.set_depth(slot, bbs, ctrl)
    check_surface(st, m, slot)
    check_surface(st, m, 0)
    # the gather over every entry of both keyframes, in a shuffled order
    order = rng.permutation(N + n0)
    gs, gi = np.where(order < N, slot, 0).astype(np.int32), np.where(order < N, order, order - N).astype(np.int32)
    g = st.surface_gather(gs, gi)
    nxy, has, uv = m.gather(gs, gi)
    assert g.normal_xy.tobytes() == nxy.tobytes() and g.has.tolist() == has.tolist() and g.uv.tobytes() == uv.tobytes()
    # refusals write nothing
    for call, msg in ((lambda: st.surface_set_normals([slot], [N], np.zeros((1, 3))), "target 0: idx outside the keyframe"),
                      (lambda: st.surface_set_normals([0, 2], [0, 0], np.zeros((2, 3))), "target 1: slot outside the store"),
                      (lambda: st.surface_take_normals(db, [len(d.status)], [0], [0]), r"sel\[0\] is outside the last normal solve"),
                      (lambda: st.surface_take_normals(db, [-1 - len(d.rec_written)], [0], [0]), r"sel\[0\] is outside the last normal solve"),
                      (lambda: st.surface_set_points(0, [1, 1], np.zeros((2, 3))), "idx 1 repeated in the batch"),
                      (lambda: st.surface_set_depth(0, nrsfm.Bbs(-1, 1, 23, -1, 1, 23, 1), np.zeros(529)), "more than 512 control points")):
        with pytest.raises(sft.DshError, match="status 1: dsh_keyframe_surface_[a-z_]+: " + msg):
            call()
    check_surface(st, m, slot)
    check_surface(st, m, 0)
    # dsh_mpdb_clear forgets everything
    st.clear()
    sc2 = SS.make_surface_scene(N, seed=1, hold=0.5)
    SR.fill_store(sc2["model"], st)
    with pytest.raises(sft.DshError, match="status 1: dsh_keyframe_surface_get: keyframe 1 has no resident surface"):
        st.surface_get(slot)
    st.surface_init(slot, sc2["kpn"])
    sc2["model"].surface_init(slot, sc2["kpn"])
    check_surface(st, sc2["model"], slot)
    st.close(), tw.close()


def run_sfn(ctx, st, m, sc, slot):
    """dsh_keyframe_sfn against the restatement's selection and dsh_sfn_estimate on its sites; the model follows the write-backs."""
    from defslam_amd import nrsfm
    b = nrsfm.Bbs(*sc["bbs"])
    c, w, u, v, nr = m.sfn_select(slot)
    r = st.sfn(slot, b, BENDING_WEIGHT, sc["mean_depth"])
    assert {k: getattr(r, k) for k in SS.SFN_COUNT_NAMES} == c
    if c["n_sites"] == 0:                                                           # rank N - 2 whatever the grid: not ok, nothing solved
        assert not r.ok and not r.ctrl_raw.any()
        check_surface(st, m, slot)
        return r, (c, w, u, v, nr), None
    kpn = sc["kpn"].astype(np.float64)
    ok, raw, ctrl, pts = nrsfm.ShapeFromNormals(ctx, b, u, v, nr, BENDING_WEIGHT, sc["mean_depth"], kpn[:, 0].copy(), kpn[:, 1].copy())
    assert r.ok == bool(ok)
    if ok:
        assert r.ctrl_raw.tobytes() == raw.tobytes() and r.ctrl.tobytes() == ctrl.tobytes() and r.pts.tobytes() == pts.tobytes()
        m.sfn_write(slot, sc["bbs"], r.ctrl, r.pts)
    check_surface(st, m, slot)                                                      # ok: the new points and depth; not ok: nothing changed
    return r, (c, w, u, v, nr), (raw, ctrl, pts)


@pytest.mark.parametrize("hold", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("N", SIZES)
def test_sfn_selection_and_counts_equal_the_restatement(ctx, N, hold):
    """obtainM's walk: bad points, an entry emptied by dsh_point_store_set_bad (it counts as empty), NaN in each component, an infinite
    component (a site), a point held by two entries (two sites); the verdict is dsh_sfn_estimate's on the restatement's sites, and
    so are the bytes where it says ok."""
    sc = SS.make_surface_scene(N, seed=2, hold=hold)
    st, _, m, slot = prepare(ctx, sc)
    r, (c, w, _, _, _), _ = run_sfn(ctx, st, m, sc, slot)
    assert sum(c.values()) == N
    if N >= 32 and 0 < hold < 1:
        roles = sc["roles"]
        assert c["n_nan"] == 3 and c["n_bad"] >= 1 and c["n_no_normal"] >= 1 and c["n_empty"] == roles.count("empty") + 1
        assert roles.index("inf") in w and roles.index("dup") in w and st.keyframe_table(slot)[roles.index("emptied")] == -1
        assert not r.ok                                                             # the infinite normal makes the system not finite
    if hold == 0.0:
        assert c["n_empty"] == N and not r.ok
    st.close()


@pytest.mark.parametrize("N,n_sites,nu,nv", SFN_CASES)
def test_sfn_numbers_equal_sfn_estimate_on_the_restatements_sites(ctx, oracle_mod, N, n_sites, nu, nv):
    sc = SS.make_surface_scene(N, seed=5, n_sites=n_sites, nu=nu, nv=nv)
    st, _, m, slot = prepare(ctx, sc)
    r, (c, w, u, v, nr), (raw, ctrl, pts) = run_sfn(ctx, st, m, sc, slot)
    assert r.ok and c["n_sites"] == n_sites
    g = st.surface_get(slot)
    assert g.pts.tobytes() == r.pts.tobytes() and g.ctrl.tobytes() == r.ctrl.tobytes() and (g.bbs.nptsu, g.bbs.nptsv) == (nu, nv)
    # the oracle (Householder QR, as the reference), at the tolerances of test_shape_from_normals_matches_oracle
    kpn = sc["kpn"].astype(np.float64)
    oko, rawo, ctrlo, ptso = oracle_mod.sfn_estimate(sc["bbs"], u, v, nr, BENDING_WEIGHT, sc["mean_depth"], kpn[:, 0].copy(), kpn[:, 1].copy())
    assert oko
    np.testing.assert_allclose(r.ctrl_raw, rawo, rtol=0, atol=1e-8 * np.abs(rawo).max())
    np.testing.assert_allclose(r.ctrl, ctrlo, rtol=0, atol=1e-6 * np.abs(ctrlo).max())
    np.testing.assert_allclose(r.pts, ptso, rtol=2e-6, atol=1e-6)
    assert r.pts.dtype == np.float32
    st.close()


def test_sfn_of_a_keyframe_without_normals_is_not_ok_and_changes_nothing(ctx):
    from defslam_amd import nrsfm
    sc = SS.make_surface_scene(64, seed=3, hold=0.5)
    m, slot = sc["model"], sc["slot"]
    st, _ = stores(ctx, m)
    rng = np.random.default_rng(0)
    pts, ctrl, bbs = rng.standard_normal((64, 3)).astype(np.float32), rng.uniform(0.5, 2.0, 42), (-0.7, 0.7, 6, -0.6, 0.6, 7, 1)
    st.surface_init(slot, sc["kpn"])
    m.surface_init(slot, sc["kpn"])
    st.surface_set_points(slot, np.arange(64), pts)
    m.set_points(slot, np.arange(64), pts)
    st.surface_set_depth(slot, nrsfm.Bbs(*bbs), ctrl)
    m.set_depth(slot, bbs, ctrl)
    r, (c, *_), _ = run_sfn(ctx, st, m, sc, slot)                                   # checks the store against the unchanged model
    assert not r.ok and r.n_sites == 0 and r.n_no_normal + r.n_bad + r.n_empty == 64 and r.n_no_normal >= 10
    assert r.ctrl is None and r.pts is None
    assert st.surface_get(slot).bbs.nptsu == 6                                      # the 13 x 15 grid of the failed estimate was not kept
    st.close()


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------

def registration_fields(g):
    return [np.asarray(a).tobytes() for a in (g.pair_idx, g.sim3, g.s22, g.info, g.Tcw_new, g.Ow_new, g.surface_scaled, g.consumed, g.registered,
                                              g.n_pairs, g.n_empty, g.n_bad, g.n_no_facet, g.n_no_snapshot)]


def test_registration_reads_and_scales_the_resident_surface(ctx):
    """surface_pts=None in register_clouds and register_surface gives the bytes of the same call with the array surface_get returns;
    afterwards the resident points are Surface::applyScale of them and the resident depth is s22 * ctrl in double, whichever way
    surface_pts was given, and surface_vertices is dsh_surface_vertices on that depth.  A keyframe without a resident Surface refuses
    NULL with the message it always had, and an explicit array leaves both stores as they were left before there was a resident Surface."""
    from defslam_amd import nrsfm, sft
    from test_surface_register_store_cpu import register_scene
    sc = register_scene(40)
    m, slot, N = sc["model"], sc["slot"], sc["N"]
    rng = np.random.default_rng(4)
    kpn = rng.uniform(-0.5, 0.5, (N, 2)).astype(np.float32)
    bbs, ctrl = (-0.62, 0.62, 13, -0.52, 0.52, 15, 1), rng.uniform(0.8, 1.6, 195)
    trio = [stores(ctx, m, with_kf=True) for _ in range(3)]                         # resident + NULL, resident + explicit array, no resident Surface
    for st, _ in trio:
        assert st.snapshot_positions(slot) > 40
    import copy
    for st, _ in trio:
        SR.apply_after(copy.deepcopy(m), sc, st)
    for st, _ in trio[:2]:
        st.surface_init(slot, kpn)
        st.surface_set_points(slot, np.arange(N), sc["surface_pts"])
        st.surface_set_depth(slot, nrsfm.Bbs(*bbs), ctrl)
    (a, ka), (b, kb), (p, kp) = trio
    held = a.surface_get(slot).pts
    assert held.tobytes() == sc["surface_pts"].tobytes()
    # the clouds
    c0, c1, c2 = a.register_clouds(slot, None, sc["Twc"]), a.register_clouds(slot, held, sc["Twc"]), p.register_clouds(slot, held, sc["Twc"])
    for x in (c1, c2):
        assert c0.pair_idx.tolist() == x.pair_idx.tolist() and c0.cloud_surface.tobytes() == x.cloud_surface.tobytes() and c0.cloud_map.tobytes() == x.cloud_map.tobytes()
        assert {k: getattr(c0, k) for k in SR.COUNT_NAMES} == {k: getattr(x, k) for k in SR.COUNT_NAMES}
    assert c0.n_pairs == 40
    # a keyframe without a resident Surface: NULL is the refusal it was
    for call in (lambda: p.register_clouds(slot, None, sc["Twc"]), lambda: p.register_surface(kp, slot, None, sc["Twc"], sc["u"], 0.05)):
        with pytest.raises(sft.DshError, match="status 1: dsh_keyframe_register[a-z_]*: Twc or surface_pts is NULL"):
            call()
    # the registration
    ga = a.register_surface(ka, slot, None, sc["Twc"], sc["u"], 0.05)
    gb = b.register_surface(kb, slot, held, sc["Twc"], sc["u"], 0.05)
    gp = p.register_surface(kp, slot, held, sc["Twc"], sc["u"], 0.05)
    assert ga.registered and registration_fields(ga) == registration_fields(gb) == registration_fields(gp)
    assert ga.surface_scaled.tobytes() == SR.apply_scale(held, ga.s22).tobytes()
    assert everything(a, ka, 2) == everything(b, kb, 2) == everything(p, kp, 2)   # points, facets, tables, snapshots, centres: as without a Surface
    for st in (a, b):
        g = st.surface_get(slot)
        assert g.pts.tobytes() == SR.apply_scale(held, ga.s22).tobytes()
        assert g.ctrl.tobytes() == (np.float64(ga.s22) * ctrl).tobytes()
        assert g.kpn.tobytes() == kpn.tobytes() and not g.has_normal.any()
        v = st.surface_vertices(slot, sc["Twc"], 7, 9)
        assert v.tobytes() == nrsfm.surface_vertices(ctx, nrsfm.Bbs(*bbs), g.ctrl, sc["Twc"], 7, 9).tobytes()
    with pytest.raises(sft.DshError, match="status 1: dsh_keyframe_surface_vertices: keyframe 1 has no resident surface"):
        p.surface_vertices(slot, sc["Twc"], 7, 9)
    a.surface_init(0, np.zeros((len(m.kfs[0].table), 2), np.float32))
    with pytest.raises(sft.DshError, match="status 3: dsh_keyframe_surface_vertices: keyframe 0 has no resident depth spline"):
        a.surface_vertices(0, sc["Twc"], 7, 9)
    for s in (a, ka, b, kb, p, kp):
        s.close()


def test_template_switch_reads_the_resident_surface(ctx):
    """surface_pts=None in switch_template: the counts, the new points and every point of the store afterwards are those of the same
    switch with the array surface_get returns; the template is built from dsh_keyframe_surface_vertices, which equals
    dsh_surface_vertices on the same depth spline."""
    import template_switch_ref as S
    from defslam_amd import localmap, nrsfm, sft, synth
    from test_template_switch_cpu import make_scene
    from test_template_switch_gpu import kf_store_from_scene
    from test_track_close_gpu import both_from_scene
    sc, (xs, ys) = make_scene("last")
    r, N = sc["ref_slot"], sc["kp"].shape[0]
    a, b = both_from_scene(ctx, sc, S.scene_to_ref).st, both_from_scene(ctx, sc, S.scene_to_ref).st
    ka, kb = kf_store_from_scene(ctx, sc, 8), kf_store_from_scene(ctx, sc, 8)
    kf = localmap.KeyFramePoints(sc["rows"], sc["cols"], sc["kp"])
    with pytest.raises(sft.DshError, match="status 1: dsh_template_switch: Twc or surface_pts is NULL"):
        b.switch_template(kb, r, kf, None, sc["Twc"])
    a.surface_init(r, np.zeros((N, 2), np.float32))
    a.surface_set_points(r, np.arange(N), sc["surface_pts"])
    a.surface_set_depth(r, nrsfm.Bbs(*sc["bbs"]), sc["depth_ctrl"])
    nodes = a.surface_vertices(r, sc["Twc"], xs, ys)
    assert nodes.tobytes() == nrsfm.surface_vertices(ctx, nrsfm.Bbs(*sc["bbs"]), sc["depth_ctrl"], sc["Twc"], xs, ys).tobytes()
    ctx.template_build(nodes, synth.regular_triangulation(xs, ys))
    held = a.surface_get(r).pts
    ga = a.switch_template(ka, r, kf, None, sc["Twc"])
    gb = b.switch_template(kb, r, kf, held, sc["Twc"])
    assert ga.n_new >= 10 and ga.new_idx.tolist() == gb.new_idx.tolist()
    assert all(getattr(ga, k) == getattr(gb, k) for k in S.COUNT_NAMES)
    assert everything(a, ka, sc["tables"].shape[0]) == everything(b, kb, sc["tables"].shape[0])
    assert a.surface_get(r).pts.tobytes() == held.tobytes()                         # the switch reads the Surface, it does not write it
    for s in (a, ka, b, kb):
        s.close()
