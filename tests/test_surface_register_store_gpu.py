"""GPU tests of the surface registration of a keyframe from the resident stores: the snapshot (dsh_keyframe_snapshot_positions,
dsh_keyframe_get_snapshot), the clouds (dsh_keyframe_register_clouds), the registration with its write-backs (dsh_keyframe_register) and the
keyframe pose of the keyframe store (dsh_keyframe_set_pose, dsh_keyframe_get_centre) against the restatement
tests/surface_register_ref.py, and the registration's numbers against dsh_surface_register on the restatement's clouds.  Bytes and
integers: no tolerance anywhere."""
import copy

import numpy as np
import pytest

import surface_register_ref as SR
from test_surface_register_store_cpu import REGISTER_PAIRS, register_scene

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 8192)


@pytest.fixture(scope="module")
def ctx():
    """A context of its own: the last test replaces the context's template."""
    from defslam_amd import sft
    c = sft.Context(0)
    yield c
    c.close()


def stores(ctx, sc, with_kf=False, **caps):
    from defslam_amd import localmap, mappoint
    st = localmap.MapPointStore(ctx, **(caps or dict(points=64, keyframes=4, observations=64)))
    ks = mappoint.KeyFrameStore(ctx, 1) if with_kf else None
    SR.fill_store(sc["model"], st, ks)
    return st, ks


def check_snapshot(st, m, slot):
    pt, xyz = st.get_snapshot(slot)
    wp, wx = m.get_snapshot(slot)
    assert pt.tolist() == wp.tolist() and xyz.tobytes() == wx.tobytes()
    return pt, xyz


def check_clouds(st, m, sc):
    g = st.register_clouds(sc["slot"], sc["surface_pts"], sc["Twc"])
    c, idx, surf, mp = m.select(sc["slot"], sc["surface_pts"], sc["Twc"])
    assert {k: getattr(g, k) for k in SR.COUNT_NAMES} == c
    assert g.pair_idx.tolist() == idx.tolist() and g.cloud_surface.tobytes() == surf.tobytes() and g.cloud_map.tobytes() == mp.tobytes()
    return g


def everything(st, ks, n_kf):
    """Every byte the two stores hand back: the points, the facets, the tracking state, the tables, the snapshots and the centres."""
    g = st.get_points()
    nodes, bary = st.get_embedding()
    s = st.get_state()
    out = [g.xyz, g.normal, g.max_distance, g.desc, g.bad, nodes, bary, s.visible, s.found, s.n_obs]
    for k in range(n_kf):
        out += [st.keyframe_table(k), *st.get_snapshot(k)]
        if ks is not None:
            out.append(st.keyframe_centre(ks, k))
    return [np.asarray(a).tobytes() for a in out]


@pytest.mark.parametrize("hold", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("N", SIZES)
def test_snapshot_and_clouds_equal_the_restatement(ctx, N, hold):
    """The snapshot is what DefKeyFrame's constructor takes, once; it survives update_points, set_keyframe_point, a removed facet and
    the plain bad flag of dsh_mpdb_set_points_bad (setBadFlag in full, the erase and the cull: the test after the next); the clouds read
    it and not the current positions, in entry order, with the five counts."""
    from defslam_amd import sft
    sc = SR.make_scene(N, seed=1, hold=hold)
    m, slot = sc["model"], sc["slot"]
    st, _ = stores(ctx, sc)
    check_snapshot(st, m, slot)                                                     # nothing yet: -1 everywhere
    empty = check_clouds(st, m, sc)
    assert empty.n_pairs == 0 and empty.n_no_snapshot == sum(r in ("good", "spoil_bad", "spoil_facet", "move_from", "dup") for r in sc["roles"])
    assert st.snapshot_positions(slot) == m.snapshot_positions(slot)
    with pytest.raises(sft.DshError, match="status 3: dsh_keyframe_snapshot_positions: the snapshot of keyframe 1 has been taken already"):
        st.snapshot_positions(slot)
    before = check_snapshot(st, m, slot)
    check_snapshot(st, m, 0)                                                        # the keyframe in front has none
    check_clouds(st, m, sc)                                                         # the positions have not moved yet
    SR.apply_after(m, sc, st)
    after = check_snapshot(st, m, slot)
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    g = check_clouds(st, m, sc)
    if N >= 32 and 0 < hold < 1:
        assert g.n_no_snapshot >= 1 and g.n_bad >= 1 and g.n_no_facet >= 1 and g.n_pairs >= 4
        assert sc["roles"].index("move_to") in g.pair_idx and sc["roles"].index("dup") in g.pair_idx
        now = st.get_points().xyz[st.keyframe_table(slot)[g.pair_idx]]
        assert (np.abs(now - g.cloud_map).max(axis=1) > 0).all()                    # the current positions are elsewhere
    if hold == 1.0:
        assert g.n_empty == 0
    st.close()


def test_clear_forgets_the_snapshot_and_growth_keeps_it(ctx):
    sc = SR.make_scene(257, seed=2)
    m, slot = sc["model"], sc["slot"]
    st, _ = stores(ctx, sc, points=2, keyframes=1, observations=2)                  # tiny: the tables and the snapshot beside them grow
    assert st.snapshot_positions(slot) == m.snapshot_positions(slot) > 50
    kept = check_snapshot(st, m, slot)
    big = np.full(3000, -1, np.int32)
    big[::3] = np.arange(1000) % st.n_points
    s2 = st.add_keyframe(big)                                                       # grows the tables past the first keyframe's snapshot
    again = check_snapshot(st, m, slot)
    assert kept[1].tobytes() == again[1].tobytes()
    pt, xyz = st.get_snapshot(s2)
    assert (pt == -1).all() and not xyz.any()
    st.clear()
    sc2 = SR.make_scene(257, seed=2)                                                # the same scene into the cleared store
    SR.fill_store(sc2["model"], st)
    check_snapshot(st, sc2["model"], slot)                                          # forgotten: -1 everywhere
    assert st.register_clouds(slot, sc2["surface_pts"], sc2["Twc"]).n_pairs == 0
    assert st.snapshot_positions(slot) == sc2["model"].snapshot_positions(slot)     # and it may be taken again
    check_snapshot(st, sc2["model"], slot)
    st.close()


def test_snapshot_survives_set_bad_erase_and_cull_which_empty_table_entries(ctx):
    """dsh_point_store_set_bad, dsh_point_store_erase_observations (with and without erase_match, with and without the cascade into
    setBadFlag) and dsh_point_store_cull blank observation records and write -1 into the table entries those name.  The snapshot is
    keyed by point and stays byte for byte; the selection then reads the tables as they are: an emptied entry counts in n_empty, an
    entry that still holds the bad point in n_bad, and an erase that leaves the entry alone leaves the pair."""
    import point_erase_ref as PE
    import store_model
    sc = register_scene(40)
    m, slot = sc["model"], sc["slot"]
    pick = SR.add_erase_fixture(sc)
    table = m.kfs[slot].table
    pt = {n: table[i] for n, i in pick.items()}
    st, _ = stores(ctx, sc)
    assert st.snapshot_positions(slot) == m.snapshot_positions(slot)
    SR.apply_after(m, sc, st)
    before = check_snapshot(st, m, slot)
    g0 = check_clouds(st, m, sc)
    assert g0.n_pairs == 40 and all(i in g0.pair_idx for i in pick.values())
    PE.assert_counts(st.set_bad_full([pt["set_bad"], pt["twice"]]), m.set_bad([pt["set_bad"], pt["twice"]]), "set_bad")
    e = st.erase_observations_full([pt["erase_cascade"], pt["erase_keep"]], [slot, slot])
    status, c = m.erase_observations([pt["erase_cascade"], pt["erase_keep"]], [slot, slot])
    assert e.status.tolist() == status.tolist() == [2, 1]
    PE.assert_counts(e.counts, c, "erase")
    e = st.erase_observations_full([pt["erase_match"]], [slot], erase_match=True)
    status, c = m.erase_observations([pt["erase_match"]], [slot], erase_match=True)
    assert e.status.tolist() == status.tolist() == [1]
    PE.assert_counts(e.counts, c, "erase_match")
    k = st.cull_full([pt["cull"], pt["erase_keep"]], [0, 0], 1)
    action, c = m.cull([pt["cull"], pt["erase_keep"]], [0, 0], 1)
    assert k.action.tolist() == action.tolist() == [2, 0]
    PE.assert_counts(k.counts, c, "cull")
    store_model.assert_state(st, m, "after the erasures")                           # tables, records, bad flags, nObs
    t = st.keyframe_table(slot)
    assert [int(t[pick[n]]) for n in SR.ERASE_PICKS] == [-1, pt["erase_cascade"], -1, pt["erase_keep"], -1, -1]
    assert int(t[sc["roles"].index("dup")]) == pt["twice"]
    after = check_snapshot(st, m, slot)                                             # the restatement's dictionary was never touched
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    assert all(after[0][pick[n]] == pt[n] for n in SR.ERASE_PICKS)
    g = check_clouds(st, m, sc)                                                     # counts, pair_idx and both clouds, bytes
    assert (g.n_pairs, g.n_empty, g.n_bad) == (g0.n_pairs - 6, g0.n_empty + 4, g0.n_bad + 2)
    assert pick["erase_keep"] in g.pair_idx and not any(pick[n] in g.pair_idx for n in SR.ERASE_PICKS if n != "erase_keep")
    st.close()


def prepared(ctx, n_pairs):
    """The scene of n_pairs pairs in a store and its twin, snapshot taken and the scene's later mutations made on all three."""
    sc = register_scene(n_pairs)
    m, slot = sc["model"], sc["slot"]
    st, ks = stores(ctx, sc, with_kf=True)
    tw, kt = stores(ctx, sc, with_kf=True)
    assert st.snapshot_positions(slot) == tw.snapshot_positions(slot) == m.snapshot_positions(slot)
    SR.apply_after(copy.deepcopy(m), sc, tw)
    SR.apply_after(m, sc, st)
    return sc, m, slot, st, ks, tw, kt


def reference_registration(ctx, m, sc, chi_limit, check_chi):
    """register.registerSurfaces on the restatement's clouds, with the condition that it reproduces itself."""
    from defslam_amd import register
    c, idx, surf, mp = m.select(sc["slot"], sc["surface_pts"], sc["Twc"])
    a = register.registerSurfaces(ctx, surf, mp, sc["u"], sc["Twc"], chi_limit, check_chi)
    b = register.registerSurfaces(ctx, surf, mp, sc["u"], sc["Twc"], chi_limit, check_chi)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k          # a condition of the comparison below
    return c, idx, a


def check_registration(g, c, idx, ref, sc):
    assert {k: getattr(g, k) for k in SR.COUNT_NAMES} == c and g.pair_idx.tolist() == idx.tolist()
    n = c["n_pairs"]
    assert g.registered == ref["registered"] and g.stream_status == 0
    assert g.consumed == (SR.consumed(n, sc["u"]) if n >= 15 else 0)
    assert g.sim3.tobytes() == ref["sim3"].tobytes() and np.float64(g.s22).tobytes() == np.float64(ref["s22"]).tobytes()
    assert g.Tcw_new.tobytes() == ref["Tcw"].tobytes()
    want_info = np.concatenate([[ref["scale0"], ref["chi2"], ref["count"]], ref["iters"], ref["trials"], [ref["acceptable"]]]).astype(np.float64)
    assert g.info.tobytes() == want_info.tobytes()
    if g.registered:
        assert g.surface_scaled.tobytes() == SR.apply_scale(sc["surface_pts"], ref["s22"]).tobytes()
        assert g.Ow_new.tobytes() == SR.centre_of(ref["Tcw"]).tobytes()
    else:
        assert g.surface_scaled is None and not g.Ow_new.any() and not g.Tcw_new.any()


@pytest.mark.parametrize("n_pairs", REGISTER_PAIRS)
def test_registration_equals_surface_register_on_the_restatements_clouds(ctx, n_pairs):
    sc, m, slot, st, ks, tw, kt = prepared(ctx, n_pairs)
    c, idx, ref = reference_registration(ctx, m, sc, 0.05, True)
    assert c["n_pairs"] == n_pairs and (n_pairs == 15 or ref["registered"] == (n_pairs >= 40))   # 14: too few; 15: the reference's own verdict, whatever it is
    centre0 = st.keyframe_centre(ks, slot)
    assert centre0.tobytes() == np.asarray(sc["model"].kfs[slot].Ow, np.float32).tobytes()
    g = st.register_surface(ks, slot, sc["surface_pts"], sc["Twc"], sc["u"], 0.05)
    check_registration(g, c, idx, ref, sc)
    got, twin = everything(st, ks, 2), everything(tw, kt, 2)
    if g.registered:
        assert st.keyframe_centre(ks, slot).tobytes() == g.Ow_new.tobytes() != centre0.tobytes()
        assert got[:-1] == twin[:-1] and got[-1] != twin[-1]                        # nothing else of either store changed
    else:
        assert got == twin
    for s in (st, ks, tw, kt):
        s.close()


def test_chi_verdicts_short_stream_and_refusals_change_nothing(ctx):
    from defslam_amd import sft
    sc, m, slot, st, ks, tw, kt = prepared(ctx, 40)
    twin = everything(tw, kt, 2)
    # chi_limit 1e-6 with check_chi: the reference refuses (the CPU test holds the oracle to the same verdicts); nothing is written
    c, idx, ref = reference_registration(ctx, m, sc, 1e-6, True)
    assert not ref["registered"] and not ref["acceptable"]
    g = st.register_surface(ks, slot, sc["surface_pts"], sc["Twc"], sc["u"], 1e-6, True)
    assert g.registered == ref["registered"] and g.sim3.tobytes() == ref["sim3"].tobytes() and g.info[7] == 0 and g.surface_scaled is None
    assert everything(st, ks, 2) == twin
    # a stream that is too short: an error with the counts set
    with pytest.raises(sft.DshError, match="status 1: dsh_keyframe_register: the uniform stream is shorter") as e:
        st.register_surface(ks, slot, sc["surface_pts"], sc["Twc"], sc["u"][:40], 0.05)
    assert e.value.result.n_pairs == 40 and e.value.result.stream_status == 1 and not e.value.result.registered
    # refusals by argument
    for call, msg in ((lambda: st.register_surface(ks, slot, sc["surface_pts"][:-1], sc["Twc"], sc["u"], 0.05), "is not the N of keyframe 1"),
                      (lambda: st.register_surface(ks, 2, sc["surface_pts"], sc["Twc"], sc["u"], 0.05), "slot outside the store"),
                      (lambda: st.register_clouds(-1, sc["surface_pts"], sc["Twc"]), "slot outside the store"),
                      (lambda: st.register_surface(kt, 0, sc["surface_pts"], sc["Twc"], sc["u"], 0.05), "is not the N of keyframe 0"),
                      (lambda: st.set_keyframe_pose(ks, 2, np.eye(4)), "slot outside the keyframe store"),
                      (lambda: st.keyframe_centre(None, 0), "kfdb is NULL"),
                      (lambda: st.get_snapshot(5), "slot outside the store")):
        with pytest.raises(sft.DshError, match="status 1: dsh_keyframe_[a-z_]+: .*" + msg):
            call()
    ctx2 = sft.Context(0)
    st2, ks2 = stores(ctx2, register_scene(14), with_kf=True)
    with pytest.raises(sft.DshError, match="status 1: dsh_keyframe_register: the keyframe store belongs to another context"):
        st.register_surface(ks2, slot, sc["surface_pts"], sc["Twc"], sc["u"], 0.05)
    st2.close(), ks2.close(), ctx2.close()
    assert everything(st, ks, 2) == twin
    # the same limit without check_chi registers: the write-backs happen
    c, idx, ref = reference_registration(ctx, m, sc, 1e-6, False)
    assert ref["registered"] and not ref["acceptable"]
    g = st.register_surface(ks, slot, sc["surface_pts"], sc["Twc"], sc["u"], 1e-6, False)
    check_registration(g, c, idx, ref, sc)
    assert st.keyframe_centre(ks, slot).tobytes() == g.Ow_new.tobytes()
    # KeyFrame::SetPose for any other caller, and its read-back
    T = np.linalg.inv(sc["Twc"].astype(np.float64)).astype(np.float32)
    Ow = st.set_keyframe_pose(ks, 0, T)
    assert Ow.tobytes() == SR.centre_of(T).tobytes() == st.keyframe_centre(ks, 0).tobytes()
    assert st.keyframe_centre(ks, slot).tobytes() == g.Ow_new.tobytes()             # the other keyframe's centre stays
    for s in (st, ks, tw, kt):
        s.close()


def test_8192_pairs_select_but_do_not_register(ctx):
    from defslam_amd import sft
    sc = SR.make_scene(8192, seed=4, hold=1.0, p_bad=0.0, p_nofacet=0.0)
    m, slot = sc["model"], sc["slot"]
    st, ks = stores(ctx, sc, with_kf=True)
    assert st.snapshot_positions(slot) == m.snapshot_positions(slot) == 8192
    g = check_clouds(st, m, sc)
    assert g.n_pairs == 8192 and g.pair_idx.tolist() == list(range(8192))
    before = everything(st, ks, 2)
    with pytest.raises(sft.DshError, match="status 1: dsh_keyframe_register: 8192 pairs: more than the 8000") as e:
        st.register_surface(ks, slot, sc["surface_pts"], sc["Twc"], sc["u"], 0.05)
    assert e.value.result.n_pairs == 8192 and not e.value.result.registered
    assert everything(st, ks, 2) == before
    st.close(), ks.close()


def test_the_template_switch_after_a_registration_reads_the_new_centre(ctx):
    """The hole, closed: after a registration with the keyframe store named, the normals and max distances dsh_template_switch gives its
    new points are UpdateNormalAndDepth from the NEW camera centre, as in the reference, where updateTemplate runs after SetPose."""
    import template_switch_ref as S
    from test_template_switch_cpu import make_scene
    from test_template_switch_gpu import build_template, check_points, kf_store_from_scene, switch_both
    from test_track_close_gpu import both_from_scene
    sc, (xs, ys) = make_scene("last")
    both = both_from_scene(ctx, sc, S.scene_to_ref)
    ks = kf_store_from_scene(ctx, sc, 8)
    r = sc["ref_slot"]
    n = both.st.snapshot_positions(r)
    assert n >= 15
    u = np.random.default_rng(9).random(n + n * n)
    g = both.st.register_surface(ks, r, sc["surface_pts"], sc["Twc"], u, 0.05, check_chi=False)
    assert g.registered and g.n_pairs == n and np.isfinite(g.Ow_new).all()
    assert both.st.keyframe_centre(ks, r).tobytes() == g.Ow_new.tobytes() == SR.centre_of(g.Tcw_new).tobytes() != sc["kf_Ow"][r].tobytes()
    check_points(both.st, both.rm)                                                  # the registration moved no point
    old = copy.deepcopy(both.rm)
    nodes = build_template(ctx, sc, xs, ys)
    moved = dict(sc, kf_Ow=sc["kf_Ow"].copy())
    moved["kf_Ow"][r] = g.Ow_new
    sw, _ = switch_both(ctx, both, ks, moved, nodes)                                # the restatement with the new centre: counts, new_idx
    pts, _, _ = check_points(both.st, both.rm)                                      # and every point, normals and max distances included
    assert sw.n_new >= 10
    old.switch_template(S.scene_kf_data(sc), r, sc["rows"], sc["cols"], sc["kp"], sc["surface_pts"], sc["Twc"], ctx.template_embed, nodes)
    new = np.arange(sw.first_id, sw.n_points)
    stale = old.point_arrays()
    assert (pts.normal[new] != stale["normal"][new]).any(axis=1).all() and (pts.max_distance[new] != stale["max_distance"][new]).any()
    both.st.close()
    ks.close()
