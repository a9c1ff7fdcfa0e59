"""GPU tests of the template switch on the map point store (dsh_surface_vertices, dsh_need_new_template, dsh_template_switch and the
read-backs dsh_point_store_get_points / dsh_point_store_get_embedding): after a switch the counts, new_idx, ALL points (position, normal, max
distance and descriptor as bytes), ALL facets and the tracking state equal the sequential restatement tests/template_switch_ref.py run
on a host mirror, and the store then answers the calls of a tracked frame as the mirror does.  Integers and bytes: no tolerance anywhere
but for the vertices, whose bound is worked out from Twc in the test."""
import numpy as np
import pytest

import template_switch_ref as S
from test_template_switch_cpu import GPU_SCENES, make_scene
from test_track_close_gpu import both_from_scene, check_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    """A context of its own: these tests replace the context's template."""
    from defslam_amd import sft
    c = sft.Context(0)
    yield c
    c.close()


def kf_store_from_scene(ctx, sc, capacity=1):
    from defslam_amd import mappoint
    ks = mappoint.KeyFrameStore(ctx, capacity)                                      # capacity 1: it grows
    for k in range(sc["tables"].shape[0]):
        assert ks.add(mappoint.MpKeyFrame(sc["kf_Ow"][k], sc["kf_desc"][k], sc["kf_octave"][k], sc["scale_factors"], bool(sc["kf_bad"][k]))) == k
    return ks


def build_template(ctx, sc, xs, ys):
    """The caller's side of createTemplate: the device's own vertices go into dsh_template_build, which keeps the embedding comparison exact."""
    from defslam_amd import nrsfm, synth
    nodes = nrsfm.surface_vertices(ctx, nrsfm.Bbs(*sc["bbs"]), sc["depth_ctrl"], sc["Twc"], xs, ys)
    ctx.template_build(nodes, synth.regular_triangulation(xs, ys))
    return nodes


def check_points(store, rm):
    """get_points and get_embedding of ALL points against the mirror, bytes."""
    g = store.get_points()
    w = rm.point_arrays()
    assert g.xyz.tobytes() == w["xyz"].tobytes() and g.normal.tobytes() == w["normal"].tobytes() and g.max_distance.tobytes() == w["max_distance"].tobytes()
    assert g.desc.tobytes() == w["desc"].tobytes() and g.bad.tolist() == w["bad"].tolist()
    nodes, bary = store.get_embedding()
    rn, rb = rm.embedding_arrays()
    np.testing.assert_array_equal(nodes, rn)
    assert bary.tobytes() == rb.tobytes()
    return g, nodes, bary


def switch_both(ctx, both, ks, sc, nodes):
    from defslam_amd import localmap
    kf = localmap.KeyFramePoints(sc["rows"], sc["cols"], sc["kp"])
    g = both.st.switch_template(ks, sc["ref_slot"], kf, sc["surface_pts"], sc["Twc"])
    c, new_idx, pre = both.rm.switch_template(S.scene_kf_data(sc), sc["ref_slot"], sc["rows"], sc["cols"], sc["kp"], sc["surface_pts"], sc["Twc"],
                                        ctx.template_embed, nodes)
    assert {k: getattr(g, k) for k in S.COUNT_NAMES} == c
    np.testing.assert_array_equal(g.new_idx, new_idx)
    return g, pre


@pytest.mark.parametrize("name", sorted(GPU_SCENES))
def test_switch_equals_the_restatement_and_the_store_tracks_on(ctx, name):
    from defslam_amd import localmap, mappoint
    sc, (xs, ys) = make_scene(name)
    caps = dict(points=2, keyframes=1, observations=2) if name == "grow" else dict(points=64, keyframes=4, observations=256)
    both = both_from_scene(ctx, sc, S.scene_to_ref, **caps)                                         # "grow": every array grows inside the switch
    ks = kf_store_from_scene(ctx, sc)
    kf = localmap.KeyFramePoints(sc["rows"], sc["cols"], sc["kp"])
    r = sc["ref_slot"]
    n_cand, cand = both.st.need_new_template(r, kf)
    rn, rc = both.rm.need_new_template(r, sc["rows"], sc["cols"], sc["kp"])
    assert n_cand == rn and cand.tolist() == rc.tolist()
    check_points(both.st, both.rm)                                                  # the read-backs before: the scene's own facets
    nodes = build_template(ctx, sc, xs, ys)
    P0 = both.st.n_points
    g, pre = switch_both(ctx, both, ks, sc, nodes)
    assert g.n_new == n_cand >= 10 and g.n_masked >= 10 and g.first_id == P0 and g.n_points == P0 + g.n_new == both.st.n_points
    assert g.new_idx.tolist() == np.nonzero(cand)[0].tolist()
    pts, enodes, ebary = check_points(both.st, both.rm)
    check_state(both.st, both.rm)
    # the facets against the host routine fed the pre-embedding positions, and against the device routine of the one-shot call
    fid, hn, hb = ctx.template_embed(pre)
    fid2, dn, db = ctx.template_embed_device(pre)
    assert fid.tolist() == fid2.tolist() and hb.tobytes() == db.tobytes()
    live = ~pts.bad
    assert ((enodes[:, 0] >= 0) == ((fid >= 0) & live)).all() and 0 < g.n_embedded == int(((fid >= 0) & live).sum()) < int(live.sum())
    hit = (fid >= 0) & live
    np.testing.assert_array_equal(enodes[hit], np.sort(hn[hit], axis=1))
    assert ebary[hit].tobytes() == np.take_along_axis(hb[hit], np.argsort(hn[hit], axis=1, kind="stable"), 1).astype(np.float64).tobytes()
    assert pts.xyz[~hit].tobytes() == pre[~hit].tobytes()                           # no facet: the position of step 3 stays
    # the new points' normal and depth against dsh_mappoint_update on the same single observations
    new = np.arange(g.first_id, g.n_points)
    u = mappoint.update(ctx, ks, pre[new], [[(r, int(i))] for i in g.new_idx], [r] * g.n_new)
    assert u.normal.tobytes() == pts.normal[new].tobytes() and u.max_distance.tobytes() == pts.max_distance[new].tobytes()
    assert u.desc.tobytes() == pts.desc[new].tobytes() == sc["kf_desc"][r][g.new_idx].tobytes()
    # the new points are held now
    n2, cand2 = both.st.need_new_template(r, kf)
    assert n2 == 0 and not cand2.any() and both.rm.need_new_template(r, sc["rows"], sc["cols"], sc["kp"])[0] == 0
    # a tracked frame on the switched store: update, search, close with the new template's nodes slightly moved
    fp = sc["frame_points"].copy()
    fp[np.nonzero(fp < 0)[0][:5]] = new[:5]                                         # the frame holds five of the new points
    u1, _ = both.update(fp)
    assert u1.n_local_points > 0
    both.search(sc["frame"], u1.n_local_points)
    moved = nodes + np.random.default_rng(3).normal(0, 1e-3, nodes.shape)
    out = (np.arange(fp.shape[0]) % 7 == 0).astype(np.uint8)
    c = both.close(sc["frame_after"], fp, out, moved)
    assert c["n_moved"] == g.n_embedded and c["to_match_local"] > 0
    check_points(both.st, both.rm)
    check_state(both.st, both.rm)
    # the mirror of the store follows: the new observations are known (adding one again is refused, erasing it works) ...
    from defslam_amd import sft
    with pytest.raises(sft.DshError, match="already observes"):
        both.st.add_observations([int(new[0])], [r])
    both.forget([(int(new[0]), r)])
    both.set_table(r, int(g.new_idx[0]), -1)
    # ... a template too small for the stored facets is refused, and removing a facet is followed
    with pytest.raises(sft.DshError, match="stored node index"):
        both.st.repose(moved[:int(enodes.max())])
    top = np.nonzero(enodes[:, 2] == enodes.max())[0]
    both.embed(top, np.full((top.shape[0], 3), -1, np.int32), np.zeros((top.shape[0], 3)))
    second = int(np.where(np.isin(np.arange(enodes.shape[0]), top), -1, enodes[:, 2]).max())
    assert second < enodes.max()
    assert both.st.repose(moved[:second + 1]) == both.rm.repose(moved[:second + 1]) == g.n_embedded - top.shape[0]
    with pytest.raises(sft.DshError, match="stored node index"):
        both.st.repose(moved[:second])
    # a second switch on the same keyframe: the key point whose entry was cleared is empty again (new, unless a point of the first
    # switch masks it now), every array consistent
    n3, _ = both.st.need_new_template(r, kf)
    assert n3 == both.rm.need_new_template(r, sc["rows"], sc["cols"], sc["kp"])[0] <= 1
    g2, _ = switch_both(ctx, both, ks, sc, nodes)
    assert g2.n_new == n3 and g2.first_id == g.n_points and g2.new_idx.tolist() == [int(g.new_idx[0])][:n3]
    check_points(both.st, both.rm)
    check_state(both.st, both.rm)
    u2, _ = both.update(fp)
    both.search(sc["frame"], u2.n_local_points)
    both.close(sc["frame_after"], fp, out, moved)
    check_state(both.st, both.rm)
    both.st.close()
    ks.close()


def test_a_point_held_by_two_key_points_keeps_the_later_position(ctx):
    sc, (xs, ys) = make_scene("grow")
    r = sc["ref_slot"]
    t = sc["tables"][r]
    held = np.nonzero((t >= 0) & ~sc["bad"][np.maximum(t, 0)])[0]
    empty = np.nonzero(t < 0)[0]
    sc["tables"][r, empty[-1]] = t[held[0]]                                         # the last empty key point holds the first held point again
    both = both_from_scene(ctx, sc, S.scene_to_ref)
    ks = kf_store_from_scene(ctx, sc, 8)
    nodes = build_template(ctx, sc, xs, ys)
    g, pre = switch_both(ctx, both, ks, sc, nodes)
    assert pre[t[held[0]]].tobytes() == S.to_world(sc["Twc"], sc["surface_pts"][empty[-1]]).tobytes()
    check_points(both.st, both.rm)
    both.st.close()
    ks.close()


def test_refused_switch_leaves_the_store_as_it_was(ctx):
    """DSH_ERR_ARG (a key point outside the image, a wrong N, a keyframe store of another size, no out) and DSH_ERR_STATE (no template
    built from facets) store nothing: get_points / get_embedding / the state are byte-identical to before."""
    from defslam_amd import localmap, sft
    sc, (xs, ys) = make_scene("last")
    both = both_from_scene(ctx, sc, S.scene_to_ref)
    ks = kf_store_from_scene(ctx, sc, 8)
    build_template(ctx, sc, xs, ys)
    r = sc["ref_slot"]
    before = check_points(both.st, both.rm)
    state = check_state(both.st, both.rm)
    kp_out = sc["kp"].copy()
    kp_out[17, 0] = sc["cols"]
    KP = localmap.KeyFramePoints
    good = KP(sc["rows"], sc["cols"], sc["kp"])
    for call, msg in ((lambda: both.st.switch_template(ks, r, KP(sc["rows"], sc["cols"], kp_out), sc["surface_pts"], sc["Twc"]), "key point 17 lies outside"),
                      (lambda: both.st.need_new_template(r, KP(sc["rows"], sc["cols"], kp_out)), "key point 17 lies outside"),
                      (lambda: both.st.switch_template(ks, r, KP(sc["rows"], sc["cols"], sc["kp"][:-1]), sc["surface_pts"][:-1], sc["Twc"]), "is not the N of keyframe"),
                      (lambda: both.st.need_new_template(r, KP(sc["rows"], sc["cols"], sc["kp"][:-1])), "is not the N of keyframe"),
                      (lambda: both.st.switch_template(ks, 7, good, sc["surface_pts"], sc["Twc"]), "slot outside the store"),
                      (lambda: both.st.switch_template(None, r, good, sc["surface_pts"], sc["Twc"]), "kfdb is NULL"),
                      (lambda: both.st.switch_template(ks, r, KP(sc["rows"], 39, np.minimum(sc["kp"], 38)), sc["surface_pts"], sc["Twc"]), "cols < 40")):
        with pytest.raises(sft.DshError, match="status 1: dsh_(template_switch|need_new_template): .*" + msg):
            call()
    ctx2 = sft.Context(0)                                                           # no template at all, and one set without facets
    both2 = both_from_scene(ctx2, sc)
    ks2 = kf_store_from_scene(ctx2, sc, 8)
    with pytest.raises(sft.DshError, match="status 3: dsh_template_switch: needs a template built from facets"):
        both2.st.switch_template(ks2, r, good, sc["surface_pts"], sc["Twc"])
    with pytest.raises(sft.DshError, match="status 1: dsh_template_switch: the keyframe store belongs to another context"):
        both.st.switch_template(ks2, r, good, sc["surface_pts"], sc["Twc"])
    check_points(both2.st, both2.rm)
    both2.st.close()
    ks2.close()
    ctx2.close()
    after = check_points(both.st, both.rm)
    for a, b in zip(before[1:], after[1:]):
        assert a.tobytes() == b.tobytes()
    assert before[0].xyz.tobytes() == after[0].xyz.tobytes() and before[0].desc.tobytes() == after[0].desc.tobytes()
    state2 = check_state(both.st, both.rm)
    assert state.n_obs.tolist() == state2.n_obs.tolist() and both.st.n_points == sc["xyz"].shape[0]
    g, _ = switch_both(ctx, both, ks, sc, build_template(ctx, sc, xs, ys))          # and it still works
    assert g.n_new > 0
    check_points(both.st, both.rm)
    both.st.close()
    ks.close()


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


@pytest.mark.parametrize("name", sorted(GPU_SCENES))
def test_surface_vertices_within_one_ulp_of_the_restatement(ctx, oracle_mod, name):
    """The device's B-spline evaluation agrees with the oracle to rtol 1e-15; a double that far off rounds to a float32 at most one ulp
    away, so each float32 camera coordinate may differ from the restatement by one ulp and a world coordinate by what those three ulps
    move it through its row of Twc, plus the roundings of the float32 row sum on either side (three products and three sums, each half an
    ulp of a partial result that is bounded by the sum of the absolute products; with inputs one ulp apart the two sides may round apart)."""
    from defslam_amd import nrsfm
    sc, (xs, ys) = make_scene(name)
    bbs = nrsfm.Bbs(*sc["bbs"])
    depth = lambda u, v: oracle_mod.bbs_eval(sc["bbs"], sc["depth_ctrl"].reshape(-1, 1), u, v)[0][:, 0]
    want, cam = S.surface_vertices(sc["bbs"], depth, sc["Twc"], xs, ys)
    got = nrsfm.surface_vertices(ctx, bbs, sc["depth_ctrl"], sc["Twc"], xs, ys)
    assert got.shape == (xs * ys, 3) and (got == got.astype(np.float32)).all()      # float32 values, widened
    T = np.abs(sc["Twc"][:3, :3].astype(np.float64))
    move = ulp32(cam) @ T.T                                                         # one ulp of every camera coordinate through |Twc|
    mag = np.abs(cam.astype(np.float64)) @ T.T + np.abs(sc["Twc"][:3, 3].astype(np.float64))
    bound = move + 2 * 6 * 0.5 * ulp32(mag + move)
    err = np.abs(got - want)
    print(f"{name}: max vertex error {err.max():.3e}, bound {bound.min():.3e} .. {bound.max():.3e}, exact in {(err == 0).mean():.0%}")
    assert (err <= bound).all()
    assert np.abs(got[:, 2] - 1.0).max() < 0.2                                      # the surface the scene describes, about one unit away
    # index x * ys + j: u moves with x
    world_u = (got - sc["Twc"][:3, 3]) @ sc["Twc"][:3, :3].astype(np.float64)
    assert (np.diff(world_u.reshape(xs, ys, 3)[:, 0, 0]) > 0).all() and (np.diff(world_u.reshape(xs, ys, 3)[0, :, 1]) > 0).all()
