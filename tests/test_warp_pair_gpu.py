"""GPU tests of dsh_keyframe_set_view / dsh_keyframe_warp_pair: one anchor of SchwarpDatabase::add on the resident stores against the
library's own one-shot calls on host-gathered arrays (dsh_warp_initialize, dsh_schwarp_eval, dsh_search_by_schwarp, dsh_schwarp_fit,
dsh_schwarp_fit_batch_store on a second database) with the bookkeeping of tests/warp_pair_ref.py between them.  Every number comes from
the same kernels on the same bytes, so everything is compared exactly."""
import numpy as np
import pytest

import warp_pair_ref as WP
from store_model import assert_state

pytestmark = pytest.mark.gpu


_bbs, _stores, _initial, _host_route = WP.bbs_of, WP.stores, WP.initial, WP.host_route


def _normals(ctx, ddb, m, sc, ids):
    from defslam_amd import nrsfm
    ids = np.asarray(sorted(ids), np.int32)
    uv = np.array([sc["anchors"][m.points[p].ref]["kpn"][m.points[p].obs[m.points[p].ref]] if m.points[p].ref < len(sc["anchors"]) else (0, 0) for p in ids], np.float32)
    return nrsfm.ObtainK1K2Database(ctx, ddb, ids, np.zeros((len(ids), 2), np.float32), np.zeros(len(ids), np.uint8), uv.reshape(-1, 2))


def _compare(ctx, st, g, r, m, sc, ddb_a, ddb_b, what="", all_stored=None):
    """all_stored: the records of the earlier calls on the same databases and this one's, when there were earlier calls."""
    assert g.x.tobytes() == r["x"].tobytes(), what
    assert (g.init_ok, g.fitted) == (r["init_ok"], r["fitted"]), what
    assert g.info.tolist() == list(r["info"]) and g.costs.tobytes() == np.asarray(r["costs"], np.float64).tobytes(), what
    for n in ("pair_state", "query_state", "query_point", "query_added"):
        assert np.array_equal(getattr(g, n), r[n]), (what, n, getattr(g, n), r[n])
    assert np.array_equal(g.query_match, r["match"]), what
    assert g.counts["n_list"] == r["n_list"] and g.counts["n_stored"] == len(r["stored"]), what
    assert g.erase == r["counts"], (what, g.erase, r["counts"])
    assert_state(st, m, what)
    assert len(ddb_a) == len(ddb_b), what
    ids = sorted({p for p, _ in (r["stored"] if all_stored is None else all_stored)})
    if ids:
        na, nb = _normals(ctx, ddb_a, m, sc, ids), _normals(ctx, ddb_b, m, sc, ids)
        for n in ("status", "k1k2", "normal_ref", "rec_point", "rec_tag", "rec_idx2", "normal_rec", "rec_written"):
            assert np.asarray(getattr(na, n)).tobytes() == np.asarray(getattr(nb, n)).tobytes(), (what, n)


def _run_pair(ctx, sc, m, st, ks, ddb_a, ddb_b, a, i1, i2, q1, tag=None, **kw):
    new = len(m.kfs) - 1
    g = st.warp_pair(ks, ddb_a, new, a, i1, i2, q1, sc["lam"], tag=tag, **kw)
    r = _host_route(ctx, m, sc, a, i1, i2, q1, ddb_b, new if tag is None else tag, **kw)
    return g, r


@pytest.mark.parametrize("grid", [(5, 6), (13, 15)])
def test_set_view_reads_back_survives_growth_and_is_forgotten_by_clear(gpu_ctx, grid):
    from defslam_amd import localmap, sft, synth
    sc = synth.make_warp_pair_scene(96, 20, 10, seed=3, nu=grid[0], nv=grid[1])
    m = WP.build_model(sc)
    st, ks = _stores(gpu_ctx, sc, m, views=False)
    new = len(m.kfs) - 1
    view = localmap.KeyframeView(sc["px2"], sc["K"], sc["bounds"], *sc["grid"], _bbs(sc["anchors"][0]["bbs"]))
    with pytest.raises(sft.DshError, match="no view"):
        st.get_view(new)
    st.set_view(new, view)
    with pytest.raises(sft.DshError, match="has a view already"):
        st.set_view(new, view)
    with pytest.raises(sft.DshError, match="no resident surface"):
        st.set_view(new - 1, localmap.KeyframeView(np.zeros((len(m.kfs[new - 1].table), 2), np.float32), sc["K"], sc["bounds"], *sc["grid"], view.warp_grid))
    for _ in range(3):                                            # the tables grow past their capacity: the view moves with them
        st.add_keyframe(np.full(4096, -1, np.int32))
    g = st.get_view(new)
    assert g.kp_px.tobytes() == sc["px2"].tobytes() and tuple(g.K) == tuple(np.float32(sc["K"])) and tuple(g.bounds) == sc["bounds"]
    assert (g.grid_cols, g.grid_rows) == sc["grid"] and g.warp_grid == view.warp_grid
    st.clear()
    with pytest.raises(sft.DshError, match="outside the store"):
        st.get_view(0)


@pytest.mark.parametrize("outliers", [0.0, 0.3])
@pytest.mark.parametrize("n_queries", [0, 1, 64, 65])
@pytest.mark.parametrize("n_pairs", [20, 21, 63, 64, 65, 130])
def test_the_call_equals_the_explicit_array_sequence(gpu_ctx, n_pairs, n_queries, outliers):
    """(a) of the issue: x, init_ok, info, costs, every state and match, both stores and the normals on either database.  Keyframes of
    96 key points where the lists fit, else 200; the grids 5 x 6 and 13 x 15 alternate."""
    from defslam_amd import nrsfm, synth
    n_kp = 96 if n_pairs + n_queries <= 96 else 200
    grid = (5, 6) if (n_pairs + n_queries // 64) % 2 else (13, 15)
    sc = synth.make_warp_pair_scene(n_kp, n_pairs, n_queries, seed=n_pairs + n_queries, nu=grid[0], nv=grid[1], outliers=outliers)
    m = WP.build_model(sc, other_ref=range(0, n_pairs, 7))
    st, ks = _stores(gpu_ctx, sc, m)
    ddb_a, ddb_b = nrsfm.DiffDatabase(gpu_ctx, 4), nrsfm.DiffDatabase(gpu_ctx, 4)
    A = sc["anchors"][0]
    g, r = _run_pair(gpu_ctx, sc, m, st, ks, ddb_a, ddb_b, 0, A["pair_idx1"], A["pair_idx2"], A["query_idx1"])
    print(n_pairs, n_queries, n_kp, grid, outliers, g.counts, g.erase)
    _compare(gpu_ctx, st, g, r, m, sc, ddb_a, ddb_b)
    if not outliers:                                              # with outliers the filter may leave fewer than min_pairs: compared all the same
        assert g.fitted and g.counts["n_stored"] > 0 and g.counts["n_filtered"] == 0
        if n_queries >= 64:                                       # (a warp initialised on outliers predicts few matches)
            assert g.counts["n_matched"] > n_queries // 4


def test_a_filter_that_leaves_fewer_than_min_pairs_ends_unfitted(gpu_ctx):
    """(b): the stores change by the clears and the matches only, the database not at all."""
    from defslam_amd import nrsfm, synth
    sc = synth.make_warp_pair_scene(96, 24, 6, seed=5, nu=5, nv=6, outliers=0.5)
    m = WP.build_model(sc)
    st, ks = _stores(gpu_ctx, sc, m)
    ddb_a, ddb_b = nrsfm.DiffDatabase(gpu_ctx, 4), nrsfm.DiffDatabase(gpu_ctx, 4)
    A = sc["anchors"][0]
    g, r = _run_pair(gpu_ctx, sc, m, st, ks, ddb_a, ddb_b, 0, A["pair_idx1"], A["pair_idx2"], A["query_idx1"], min_pairs=40)
    assert not g.fitted and g.counts["n_list"] < 40 and len(ddb_a) == 0
    assert set(g.pair_state.tolist()) <= {WP.FILTERED, WP.UNFITTED} and set(g.query_state.tolist()) <= {WP.NO_MATCH, WP.UNFITTED}
    _compare(gpu_ctx, st, g, r, m, sc, ddb_a, ddb_b)


def test_collisions_a_twice_held_point_and_an_entry_the_filter_cleared(gpu_ctx):
    """(c): two queries on one free key point, a point under two entries of the anchor, a query landing on a cleared entry."""
    from defslam_amd import nrsfm, synth
    sc = synth.make_warp_pair_scene(200, 64, 40, seed=11, nu=13, nv=15, outliers=0.0, lost_queries=0.0)
    m = WP.build_model(sc)
    A, new = sc["anchors"][0], len(m.kfs) - 1
    i1, i2, q = A["pair_idx1"], A["pair_idx2"], A["query_idx1"]
    sc["kpn2"][i2[[10, 11]]] += np.float32(0.15)                              # two neighbouring matches 78 px off: the filter's entries 10 and 11
    _, x, filt = _initial(gpu_ctx, sc, 0, i1, i2)
    assert filt.any() and not filt.all()
    has = np.array(m.kfs[new].table) != -1
    has[i2[filt]] = False
    dry = nrsfm.searchBySchwarp(gpu_ctx, _bbs(A["bbs"]), x, A["kpn"][q], A["desc"][q], sc["K"], sc["bounds"], sc["px2"], sc["desc2"], has, 2.0, 50, sc["grid"])
    ja, jb, jc = [int(j) for j in np.flatnonzero(dry >= 0) if j > 0][:3]       # three queries that find their counterparts
    # a point held by two entries of the anchor's table: query 0's key point holds pair 0's point, which observes the new keyframe already
    m.kfs[0].table[int(q[0])] = m.kfs[0].table[int(i1[0])]
    # queries ja and jb look alike: both land on ja's counterpart
    A["kpn"][q[jb]], A["desc"][q[jb]] = A["kpn"][q[ja]], A["desc"][q[ja]]
    m.kfs[0].desc[q[jb]] = A["desc"][q[ja]]
    # the counterpart of query jc moves onto the key point of a pair the filter removes: the filter's clear frees it for the search
    freed, own = int(i2[np.flatnonzero(filt)[0]]), int(dry[jc])
    sc["px2"][freed], sc["desc2"][freed] = sc["px2"][own], sc["desc2"][own]
    m.kfs[new].desc[freed] = sc["desc2"][own]
    sc["px2"][own] = (-50.0, -50.0)
    st, ks = _stores(gpu_ctx, sc, m)
    ddb_a, ddb_b = nrsfm.DiffDatabase(gpu_ctx, 4), nrsfm.DiffDatabase(gpu_ctx, 4)
    g, r = _run_pair(gpu_ctx, sc, m, st, ks, ddb_a, ddb_b, 0, i1, i2, q)
    print(g.counts, g.query_match[[0, ja, jb, jc]], freed)
    _compare(gpu_ctx, st, g, r, m, sc, ddb_a, ddb_b)
    assert g.query_match[ja] >= 0 and g.query_match[ja] == g.query_match[jb]
    assert g.query_added[ja] and g.query_added[jb] and m.kfs[new].table[g.query_match[jb]] == g.query_point[jb] != g.query_point[ja]
    assert g.query_match[jc] == freed and g.pair_state[np.flatnonzero(filt)[0]] == WP.FILTERED
    assert g.query_match[0] < 0 or not g.query_added[0]                       # the twice-held point observes the new keyframe already


def test_a_dropped_match_whose_point_falls_to_two_observations_becomes_bad(gpu_ctx):
    """(d): with every pair's point observed by the anchor and the new keyframe alone, a drop cascades to setBadFlag."""
    from defslam_amd import nrsfm, synth
    sc = synth.make_warp_pair_scene(200, 64, 10, seed=13, nu=13, nv=15, outliers=0.0)
    A = sc["anchors"][0]
    far = np.arange(0, 64, 9)                                                 # matches 15 px off: what the filter lets pass, the fit drops
    sc["kpn2"][A["pair_idx2"][far]] += np.float32(0.03)
    m = WP.build_model(sc, few_obs=range(64))
    st, ks = _stores(gpu_ctx, sc, m)
    ddb_a, ddb_b = nrsfm.DiffDatabase(gpu_ctx, 4), nrsfm.DiffDatabase(gpu_ctx, 4)
    g, r = _run_pair(gpu_ctx, sc, m, st, ks, ddb_a, ddb_b, 0, A["pair_idx1"], A["pair_idx2"], A["query_idx1"])
    print("dropped", g.counts["n_dropped"], "set bad", g.erase["n_set_bad"], "filtered", g.counts["n_filtered"])
    _compare(gpu_ctx, st, g, r, m, sc, ddb_a, ddb_b)
    assert g.counts["n_dropped"] > 0 and g.erase["n_set_bad"] == g.counts["n_dropped"] and g.erase["n_entries"] > 0
    bad = [p for p, pt in enumerate(m.points) if pt.bad]
    assert bad and all(not m.points[p].obs for p in bad)


def test_a_drop_that_sets_a_point_bad_skips_a_later_entry_of_that_point(gpu_ctx):
    """The election of the records loop needs a second round: pair 21 is 15 px off, so the fit drops it; its point is observed by the
    anchor and the new keyframe alone, so the drop sets it bad; and a query's key point of the anchor holds the same point, so the
    matched query behind it in the list is skipped, which the first round cannot know."""
    from defslam_amd import nrsfm, synth
    sc = synth.make_warp_pair_scene(200, 64, 40, seed=29, nu=13, nv=15, outliers=0.0, lost_queries=0.0)
    A = sc["anchors"][0]
    i1, i2, q = A["pair_idx1"], A["pair_idx2"], A["query_idx1"]
    sc["kpn2"][i2[21]] += np.float32(0.03)                                    # (the filter charges it to matches 10 and 42, not to 21)
    m = WP.build_model(sc, few_obs=[21])
    new = len(m.kfs) - 1
    _, x, filt = _initial(gpu_ctx, sc, 0, i1, i2)
    assert not filt[21]
    has = np.array(m.kfs[new].table) != -1
    has[i2[filt]] = False
    dry = nrsfm.searchBySchwarp(gpu_ctx, _bbs(A["bbs"]), x, A["kpn"][q], A["desc"][q], sc["K"], sc["bounds"], sc["px2"], sc["desc2"], has, 2.0, 50, sc["grid"])
    j0 = int(np.flatnonzero(dry >= 0)[0])
    m.kfs[0].table[int(q[j0])] = 21                                           # the anchor holds pair 21's point under a second key point
    st, ks = _stores(gpu_ctx, sc, m)
    ddb_a, ddb_b = nrsfm.DiffDatabase(gpu_ctx, 4), nrsfm.DiffDatabase(gpu_ctx, 4)
    g, r = _run_pair(gpu_ctx, sc, m, st, ks, ddb_a, ddb_b, 0, i1, i2, q)
    print(g.counts, g.erase, g.pair_state[21], g.query_state[j0])
    _compare(gpu_ctx, st, g, r, m, sc, ddb_a, ddb_b)
    assert g.pair_state[21] == WP.DROPPED and g.query_match[j0] >= 0 and not g.query_added[j0] and g.query_state[j0] == WP.SKIPPED
    assert g.counts["rounds"] >= 2 and g.erase["n_set_bad"] == 1 and m.points[21].bad


def test_two_anchors_in_sequence_and_a_log_that_grows_from_capacity_one(gpu_ctx):
    """(e) and (f): the second anchor's call sees what the first left; the store was created with room for one record."""
    from defslam_amd import nrsfm, synth
    sc = synth.make_warp_pair_scene(200, 40, 30, n_anchors=2, seed=17, nu=5, nv=6, outliers=0.2)
    m = WP.build_model(sc)
    st, ks = _stores(gpu_ctx, sc, m, observations=1)
    ddb_a, ddb_b = nrsfm.DiffDatabase(gpu_ctx, 1), nrsfm.DiffDatabase(gpu_ctx, 1)
    stored = []
    for a, A in enumerate(sc["anchors"]):
        g, r = _run_pair(gpu_ctx, sc, m, st, ks, ddb_a, ddb_b, a, A["pair_idx1"], A["pair_idx2"], A["query_idx1"], tag=7 + a)
        stored += r["stored"]
        _compare(gpu_ctx, st, g, r, m, sc, ddb_a, ddb_b, f"anchor {a}", all_stored=stored)
        assert g.fitted and g.counts["n_appended"] > 0


def test_refusals_leave_the_stores_unchanged(gpu_ctx):
    """(g): every refusal of the header, then the state of both stores and of the database."""
    from defslam_amd import localmap, mappoint, nrsfm, sft, synth
    sc = synth.make_warp_pair_scene(96, 24, 8, seed=19, nu=5, nv=6)
    m = WP.build_model(sc)
    st, ks = _stores(gpu_ctx, sc, m)
    ddb = nrsfm.DiffDatabase(gpu_ctx, 4)
    A, new = sc["anchors"][0], len(m.kfs) - 1
    i1, i2, q1 = A["pair_idx1"], A["pair_idx2"], A["query_idx1"]
    call = lambda **k: st.warp_pair(k.pop("ks", ks), k.pop("ddb", ddb), k.pop("slot", new), k.pop("anchor", 0), k.pop("i1", i1), k.pop("i2", i2), k.pop("q1", q1),
                                    sc["lam"], **k)
    ctx2 = sft.Context(0)
    gone_ctx = sft.Context(0)
    gone = nrsfm.DiffDatabase(gone_ctx, 4)
    gone_ctx.close()
    bad = lambda v, at, val: np.concatenate([v[:at], [val], v[at + 1:]]).astype(np.int32)
    rows = [(dict(i1=bad(i1, 3, 96)), "pair_idx1\\[3\\] is outside"), (dict(i2=bad(i2, 0, -1)), "pair_idx2\\[0\\] is outside"),
            (dict(q1=bad(q1, 2, 200)), "query_idx1\\[2\\] is outside"), (dict(i2=bad(i2, 5, i2[1])), "pair_idx2\\[5\\] repeats"),
            (dict(q1=bad(q1, 4, q1[0])), "query_idx1\\[4\\] repeats"), (dict(anchor=new), "anchor == slot"), (dict(slot=len(m.kfs)), "outside the store"),
            (dict(ks=mappoint.KeyFrameStore(ctx2, 2)), "keyframe store is NULL, belongs to another context"), (dict(ks=None), "keyframe store is NULL"),
            (dict(ddb=nrsfm.DiffDatabase(ctx2, 4)), "database is NULL, belongs to another context"), (dict(ddb=gone), "database is NULL"),
            (dict(max_iters=1001), "max_iters"), (dict(radius=float("nan")), "radius"), (dict(i1=i1[:0], i2=i2[:0]), "n_pairs < 1"),
            (dict(anchor=1, i1=np.zeros_like(i1), q1=q1[:0]), "no view")]
    for kw, msg in rows:
        with pytest.raises(sft.DshError, match=msg):
            call(**kw)
    # more than 256 control points in the anchor's warp grid: a store of its own, whose anchor's view says 17 x 16
    sc2 = synth.make_warp_pair_scene(96, 24, 0, seed=19, nu=5, nv=6)
    sc2["anchors"][0]["bbs"] = sc2["anchors"][0]["bbs"][:2] + (17,) + sc2["anchors"][0]["bbs"][3:5] + (16, 2)
    m2 = WP.build_model(sc2)
    st2, ks2 = _stores(gpu_ctx, sc2, m2)
    with pytest.raises(sft.DshError, match="more than 256 control points"):
        st2.warp_pair(ks2, ddb, len(m2.kfs) - 1, 0, i1, i2, [], sc["lam"])
    # a live record without a key point index
    p = m.kfs[0].table[int(q1[0])]
    st.add_observations([p], [new])
    with pytest.raises(sft.DshError, match="without a key point index"):
        call()
    st.erase_observations([p], [new])
    assert_state(st, m, "after the refusals")
    assert len(ddb) == 0
    ctx2.close()
    # the call still runs afterwards
    assert call().fitted
