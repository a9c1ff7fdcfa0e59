"""CPU tests of the template switch: the restatement tests/template_switch_ref.py on hand-built cases with known answers, the interval
form of the occupancy mask (what the device computes) against the image form on random scenes, the scene generators of the GPU tests, and
the refusals of the new entry points on a host-only context (arguments first, then DSH_ERR_NO_DEVICE: there is no CPU fallback)."""
import ctypes as C

import numpy as np
import pytest

import template_switch_ref as S

OK, ARG, STATE, NODEV = 0, 1, 3, 4

# the generated scenes the GPU tests run (tests/test_template_switch_gpu.py): name -> (seed, scene arguments, template grid (xs, ys))
GPU_SCENES = {"grow": (0, dict(n_kf=3, n_kp=300, obs_per_point=2, n_frame_kp=300, ctrl=(13, 15)), (4, 4)),        # more than one workgroup of key points
              "last": (1, dict(n_kf=2, n_kp=300, obs_per_point=2, n_frame_kp=300, ctrl=(6, 7), ref_slot=-1), (3, 5)),   # the newest keyframe: no observation yet
              "blocks": (2, dict(n_kf=3, n_kp=700, obs_per_point=2, n_frame_kp=300, ctrl=(13, 15), rows=75, cols=100), (10, 10))}   # odd kernel, three workgroups


def make_scene(name):
    from defslam_amd import synth
    seed, kw, grid = GPU_SCENES[name]
    return synth.make_template_switch_scene(seed, **kw), grid


def literal_masked(rows, cols, held, y, x):
    """The definition, pixel by pixel: does the reflected k x k window of (y, x) read a held pixel?"""
    k, a = cols // 20, (cols // 20) // 2
    held = set(held)
    return any((S.reflect101(y + dy, rows), S.reflect101(x + dx, cols)) in held for dy in range(-a, k - a) for dx in range(-a, k - a))


# ---- the mask ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols,k", [(24, 40, 2), (33, 61, 3), (120, 160, 8)])
def test_a_held_pixel_masks_exactly_its_window(rows, cols, k):
    a = k // 2
    assert S.kernel_of(cols) == (k, a)
    py, px = rows // 2, cols // 2
    mask = S.box_mask(rows, cols, [(py, px)])
    want = np.zeros((rows, cols), bool)
    want[py - (k - 1 - a):py + a + 1, px - (k - 1 - a):px + a + 1] = True          # queries px - (k-1-a) .. px + a away, and no further
    np.testing.assert_array_equal(mask, want)
    assert mask.sum() == k * k
    for y in range(rows):
        for x in (px - k, px - (k - 1 - a) - 1, px - (k - 1 - a), px, px + a, px + a + 1):
            assert S.masked_by_interval(rows, cols, [(py, px)], y, x) == want[y, x] == literal_masked(rows, cols, [(py, px)], y, x)


# (cols, held column, masked query columns near that border): worked out by hand from window x - a .. x + k - 1 - a and p < 0 -> -p,
# p >= n -> 2 (n - 1) - p
BORDER_COLUMNS = [(40, 0, [0, 1]), (40, 1, [0, 1, 2]),                   # k = 2, a = 1: query 0 reads columns {1, 0}
                  (40, 39, [39]), (40, 38, [38, 39]),
                  (61, 0, [0, 1]), (61, 1, [0, 1, 2]),                   # k = 3, a = 1: query 0 reads {1, 0, 1}
                  (61, 60, [59, 60]), (61, 59, [58, 59, 60]),
                  (160, 0, [0, 1, 2, 3, 4]), (160, 1, [0, 1, 2, 3, 4, 5]),      # k = 8, a = 4: query 0 reads {4, 3, 2, 1, 0, 1, 2, 3}
                  (160, 4, [0, 1, 2, 3, 4, 5, 6, 7, 8]),                 # query 0 sees column 4 through the reflection only
                  (160, 5, [2, 3, 4, 5, 6, 7, 8, 9]),                    # query 1 reads {3, 2, 1, 0, 1, 2, 3, 4}: not 5
                  (160, 159, [156, 157, 158, 159]), (160, 158, [155, 156, 157, 158, 159])]


@pytest.mark.parametrize("cols,held,masked", BORDER_COLUMNS)
def test_the_reflected_border_in_columns_and_rows(cols, held, masked):
    rows = cols - 7                                                                 # the rows follow the same rule with their own length
    k, a = S.kernel_of(cols)
    mid = rows // 2
    m = S.box_mask(rows, cols, [(mid, held)])
    assert np.nonzero(m[mid])[0].tolist() == masked
    for x in range(cols):
        assert S.masked_by_interval(rows, cols, [(mid, held)], mid, x) == (x in masked) == literal_masked(rows, cols, [(mid, held)], mid, x)
    # the same pattern along a column, counted from the same end: cols and rows differ, so the far border is restated
    hy = held if held < cols // 2 else rows - (cols - held)
    my = masked if held < cols // 2 else [y - (cols - rows) for y in masked]
    mcol = cols // 2
    m = S.box_mask(rows, cols, [(hy, mcol)])
    assert np.nonzero(m[:, mcol])[0].tolist() == my
    for y in range(rows):
        assert S.masked_by_interval(rows, cols, [(hy, mcol)], y, mcol) == (y in my)


@pytest.mark.parametrize("seed", range(12))
def test_interval_form_equals_image_form_on_random_scenes(seed):
    """What the device computes against the image: every key point of 12 random scenes, k = 2, 3, 4, 5, key points on the border."""
    rng = np.random.default_rng(500 + seed)
    cols = (40, 60, 80, 100)[seed % 4] + int(rng.integers(0, 20))
    rows = int(rng.integers(cols // 20 + 1, cols))
    n = 120
    kp = np.stack([rng.uniform(0, cols - 1e-3, n), rng.uniform(0, rows - 1e-3, n)], 1).astype(np.float32)
    kp[:6, 0] = [0, 0.5, 1.2, cols - 2, cols - 1, cols - 0.01]
    kp[6:12, 1] = [0, 0.5, 1.2, rows - 2, rows - 1, rows - 0.01]
    kp[12:16] = [[0, 0], [cols - 1, 0], [0, rows - 1], [cols - 1, rows - 1]]
    held = [S.pixel(kp[i]) for i in range(n) if rng.uniform() < 0.25 or 12 <= i < 14]
    mask = S.box_mask(rows, cols, held)
    assert S.kernel_of(cols)[0] == (2, 3, 4, 5)[seed % 4]
    n_masked = 0
    for i in range(n):
        y, x = S.pixel(kp[i])
        assert mask[y, x] == S.masked_by_interval(rows, cols, held, y, x) == literal_masked(rows, cols, held, y, x), (i, y, x)
        n_masked += int(mask[y, x])
    assert 0 < n_masked < n
    for y in (0, 1, rows - 2, rows - 1):                                             # and every pixel of the border rows and columns
        for x in range(cols):
            assert mask[y, x] == S.masked_by_interval(rows, cols, held, y, x)
    for x in (0, 1, cols - 2, cols - 1):
        for y in range(rows):
            assert mask[y, x] == S.masked_by_interval(rows, cols, held, y, x)


# ---- the restatement on hand-built keyframes -----------------------------------------------------------------------------------------------

HAND_ROWS, HAND_COLS = 24, 40                                                       # k = 2, a = 1: key point x masks queries x .. x + 1 (and 0 from 1)
SF = np.array([1.0, 1.2, 1.44], np.float32)


def hand_case(table, kp, bad=()):
    """One keyframe with the given table over len(set(table) - {-1}) points at (0, 0, 1); the keyframe store's side: descriptor row i is
    all i, octave i % 3, camera centre at the origin."""
    rm = S.TemplateRefMap()
    for p in range(max(table) + 1 if table else 0):
        rm.add_point(xyz=(0.0, 0.0, 1.0), desc=np.full(32, 200 + p, np.uint8), bad=p in bad)
    rm.add_keyframe(table)
    for p in sorted(set(table) - {-1}):
        assert rm.add_observation(p, 0)
    n = len(table)
    kfs = [S.RefKfData([0, 0, 0], np.repeat(np.arange(n, dtype=np.uint8)[:, None], 32, 1), np.arange(n) % 3, SF)]
    return rm, kfs, np.asarray(kp, np.float32).reshape(n, 2)


def no_facet(pts):
    n = len(pts)
    return np.full(n, -1, np.int32), np.full((n, 3), -1, np.int32), np.zeros((n, 3), np.float32)


def run_hand(rm, kfs, kp, Twc=np.eye(4, dtype=np.float32), embed=no_facet, rest=np.zeros((0, 3))):
    n = kp.shape[0]
    surf = np.stack([0.01 * np.arange(n), np.zeros(n), np.ones(n)], 1).astype(np.float32)
    return rm.switch_template(kfs, 0, HAND_ROWS, HAND_COLS, kp, surf, Twc, embed, rest), surf


def test_hand_built_keyframe_with_every_case():
    """Key points 0 and 1 share a pixel and hold points 0 and 1; key point 2 holds the bad point 2 next to the empty key point 3, which it
    does not mask; key point 4 is empty beside key point 0 (masked); key point 5 is empty and far away (new); key point 6 holds point 0
    again: the later SetWorldPos wins."""
    table = [0, 1, 2, -1, -1, -1, 0]
    kp = [[10.2, 5.7], [10.9, 5.1], [30.0, 12.0], [30.5, 12.5], [11.0, 6.0], [20.0, 20.0], [5.0, 5.0]]
    rm, kfs, kp = hand_case(table, kp, bad=(2,))
    n_cand, cand = rm.need_new_template(0, HAND_ROWS, HAND_COLS, kp)
    assert n_cand == 2 and cand.tolist() == [False, False, False, True, False, True, False]
    (c, new_idx, _), surf = run_hand(rm, kfs, kp)
    assert c == dict(n_new=2, first_id=3, n_moved=3, n_masked=1, n_embedded=0, n_points=5)
    assert new_idx.tolist() == [3, 5] and rm.kfs[0].table == [0, 1, 2, 3, -1, 4, 0]
    assert rm.points[0].xyz.tobytes() == surf[6].tobytes() and rm.points[1].xyz.tobytes() == surf[1].tobytes()
    assert rm.points[2].xyz.tolist() == [0.0, 0.0, 1.0]                             # the bad point stays
    for q, i in ((3, 3), (4, 5)):
        pt = rm.points[q]
        assert pt.xyz.tobytes() == surf[i].tobytes() and pt.desc.tolist() == [i] * 32 and not pt.bad and sorted(pt.obs) == [0]
        d = np.float32(np.sqrt(np.float64(surf[i][0]) ** 2 + 1.0))                  # one observation from the origin: normal = xyz / |xyz|
        assert pt.max_distance == np.float32(d * SF[i % 3])
        assert np.allclose(pt.normal, surf[i] / d, rtol=0, atol=1e-7)
    v, f, o, _ = rm.track_state()
    assert v[3:].tolist() == [1, 1] and f[3:].tolist() == [1, 1] and o.tolist() == [1, 1, 1, 1, 1]
    assert rm.need_new_template(0, HAND_ROWS, HAND_COLS, kp)[0] == 0             # the new points are held now


def test_no_held_point_every_empty_key_point_is_new_and_no_empty_key_point_creates_none():
    rm, kfs, kp = hand_case([-1, -1, -1], [[3, 3], [3.5, 3.5], [30, 20]])
    assert rm.need_new_template(0, HAND_ROWS, HAND_COLS, kp)[0] == 3
    (c, new_idx, _), _ = run_hand(rm, kfs, kp)
    assert c == dict(n_new=3, first_id=0, n_moved=0, n_masked=0, n_embedded=0, n_points=3) and new_idx.tolist() == [0, 1, 2]
    rm, kfs, kp = hand_case([0, 1, 2], [[3, 3], [3.5, 3.5], [30, 20]])
    (c, new_idx, _), _ = run_hand(rm, kfs, kp)
    assert c == dict(n_new=0, first_id=3, n_moved=3, n_masked=0, n_embedded=0, n_points=3) and new_idx.shape == (0,)
    rm, kfs, kp = hand_case([0, 0], [[3, 3], [8, 8]], bad=(0,))                     # only a held bad point: no mask at all, nothing moves
    assert rm.need_new_template(0, HAND_ROWS, HAND_COLS, kp)[0] == 0
    (c, _, _), _ = run_hand(rm, kfs, kp)
    assert c["n_moved"] == 0 and c["n_new"] == 0


def test_world_position_is_the_float32_row_sum_and_the_embedding_reposes(host_ctx):
    """Twc with a translation: the position is ((T0 x + T1 y) + T2 z) + T3 in float32; with a real template the embedded points move onto
    the mesh by the repose expression and the others keep their position."""
    from defslam_amd import synth
    Twc = np.eye(4, dtype=np.float32)
    Twc[:3, :3] = synth._rodrigues(np.array([0.01, -0.02, 0.015])).astype(np.float32)
    Twc[:3, 3] = [0.011, -0.007, 0.003]
    s = np.array([0.1234567, -0.0456789, 1.0123456], np.float32)
    w = S.to_world(Twc, s)
    assert np.allclose(w, Twc[:3, :3].astype(np.float64) @ s.astype(np.float64) + Twc[:3, 3], rtol=0, atol=3e-7)
    nodes = np.array([[-0.2, -0.2, 1.0], [0.3, -0.2, 1.0], [-0.2, 0.3, 1.0], [0.3, 0.3, 1.0]])
    host_ctx.template_build(nodes, np.array([[0, 1, 2], [1, 2, 3]], np.int32))
    rm, kfs, kp = hand_case([-1, 0, -1], [[3, 3], [20, 10], [35, 20]])
    (c, new_idx, pre), surf = run_hand(rm, kfs, kp, Twc, host_ctx.template_embed, nodes)
    assert c["n_new"] == 2 and c["n_moved"] == 1 and c["n_embedded"] == 3
    for p in range(3):
        n0, n1, n2 = rm.nodes[p]
        b = rm.bary[p]
        assert n0 < n1 < n2 and all(np.float64(np.float32(v)) == v for v in b)       # float32 barycentrics, widened
        want = ((b[0] * nodes[n0] + b[1] * nodes[n1]) + b[2] * nodes[n2]).astype(np.float32)
        assert rm.points[p].xyz.tobytes() == want.tobytes() and abs(rm.points[p].xyz[2] - 1.0) < 1e-6
    assert pre[0].tobytes() == S.to_world(Twc, surf[1]).tobytes()                   # what the embedding was fed: the moved point


# ---- the scene generators of the GPU tests -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(GPU_SCENES))
def test_generated_scenes_hold_every_case(host_ctx, name):
    from defslam_amd import synth
    sc, (xs, ys) = make_scene(name)
    seed = GPU_SCENES[name][0]
    rm = S.scene_to_ref(sc)
    r = sc["ref_slot"]
    table = sc["tables"][r]
    assert sum(1 for p in table if p >= 0 and sc["bad"][p]) == 1                    # one held bad point
    n_cand, cand = rm.need_new_template(r, sc["rows"], sc["cols"], sc["kp"])
    nodes, _ = S.surface_vertices(sc["bbs"], lambda u, v: synth.switch_depth(u, v, seed), sc["Twc"], xs, ys)
    host_ctx.template_build(nodes, synth.regular_triangulation(xs, ys))
    P0 = len(rm.points)
    c, new_idx, _ = rm.switch_template(S.scene_kf_data(sc), r, sc["rows"], sc["cols"], sc["kp"], sc["surface_pts"], sc["Twc"],
                                      host_ctx.template_embed, nodes)
    assert c["n_new"] == n_cand >= 10 and c["n_masked"] >= 10 and c["n_moved"] >= 10 and new_idx.tolist() == np.nonzero(cand)[0].tolist()
    good = [p for p, pt in enumerate(rm.points) if not pt.bad]
    assert 0 < c["n_embedded"] < len(good)                                           # points that embed in no facet
    assert any(rm.nodes[p] is None for p in range(P0, len(rm.points))) and any(rm.nodes[p] is not None for p in range(P0, len(rm.points)))
    assert any(rm.nodes[int(p)] is not None for p in table if p >= 0)
    pix = [S.pixel(k) for k in sc["kp"]]
    assert {0, sc["cols"] - 1} <= {x for _, x in pix} and {0, sc["rows"] - 1} <= {y for y, _ in pix}


# ---- refusals on a host-only context -----------------------------------------------------------------------------------------------------

def test_refusals_name_the_entry_and_come_before_the_device_gate():
    from defslam_amd import localmap, nrsfm, sft
    ctx = sft.Context(-1)
    st = localmap.MapPointStore(ctx)
    KP = localmap.KeyFramePoints
    ok = np.array([[5, 5], [20, 10]], np.float32)
    cases = [(KP(24, 39, ok), "cols < 40"), (KP(2, 40, ok), "does not fit"), (KP(24, 40, [[5, 5], [40.0, 3]]), "key point 1 lies outside"),
             (KP(24, 40, [[5, 24.0], [1, 3]]), "key point 0 lies outside"), (KP(24, 40, [[5, 5], [-1.0, 3]]), "key point 1 lies outside"),
             (KP(24, 40, [[np.nan, 5], [1, 3]]), "key point 0 lies outside"), (KP(0, 40, ok), "rows or cols"),
             (KP(24, 40, ok), "slot outside the store")]                             # a host-only store holds no keyframe
    for kf, msg in cases:
        with pytest.raises(sft.DshError, match="status 1: dsh_need_new_template: .*" + msg):
            st.need_new_template(0, kf)
        with pytest.raises(sft.DshError, match="status 1: dsh_template_switch: .*" + msg):
            st.switch_template(None, 0, kf, np.zeros((2, 3)), np.eye(4))
    # -0.5 truncates to pixel 0 and 39.9 to pixel 39: both inside
    with pytest.raises(sft.DshError, match="slot outside the store"):
        st.need_new_template(0, KP(24, 40, [[-0.5, 0.0], [39.9, 23.9]]))
    with pytest.raises(sft.DshError, match="status 1: dsh_point_store_get_points: point id 0 outside"):
        st.get_points([0])
    with pytest.raises(sft.DshError, match="status 1: dsh_point_store_get_embedding: point id 3 outside"):
        st.get_embedding([3])
    with pytest.raises(sft.DshError, match="status 1: dsh_point_store_get_embedding: n < 0"):
        st._call("dsh_point_store_get_embedding", -1, None, None, None)
    for call, name in ((lambda: st.get_points([]), "dsh_point_store_get_points"), (lambda: st.get_embedding([]), "dsh_point_store_get_embedding")):
        with pytest.raises(sft.DshError, match=f"status 4: {name}: host-only"):
            call()
    L = ctx._L
    assert L.dsh_template_switch(st._h, None, None, None) == ARG and "in is NULL" in L.dsh_last_error(ctx._h).decode()
    assert L.dsh_need_new_template(st._h, 0, None, None, None) == ARG and "kf is NULL" in L.dsh_last_error(ctx._h).decode()
    assert L.dsh_need_new_template(None, 0, None, None, None) == ARG and L.dsh_point_store_get_points(None, 0, None, None, None, None, None, None) == ARG
    # the vertices: arguments, then the device
    b = nrsfm.Bbs(-1.0, 1.0, 6, -1.0, 1.0, 7, 1)
    for args, msg in (((b, np.zeros(42), np.eye(4), 1, 4), "xs and ys"), ((b, np.zeros(42), np.eye(4), 4, 1), "xs and ys"),
                      ((nrsfm.Bbs(-1.0, 1.0, 6, -1.0, 1.0, 7, 2), np.zeros(84), np.eye(4), 4, 4), "valdim 1"),
                      ((nrsfm.Bbs(1.0, 1.0, 6, -1.0, 1.0, 7, 1), np.zeros(42), np.eye(4), 4, 4), "bad B-spline")):
        with pytest.raises(sft.DshError, match="status 1: dsh_surface_vertices: .*" + msg):
            nrsfm.surface_vertices(ctx, *args)
    with pytest.raises(sft.DshError, match="status 4: dsh_surface_vertices: host-only"):
        nrsfm.surface_vertices(ctx, b, np.zeros(42), np.eye(4), 4, 4)
    assert L.dsh_surface_vertices(None, None) == ARG
    # a detached store answers DSH_ERR_ARG
    ctx2 = sft.Context(-1)
    st2 = localmap.MapPointStore(ctx2)
    ctx2.close()
    keep = []
    k = KP(24, 40, ok).c(keep)
    n = C.c_int32(0)
    assert L.dsh_need_new_template(st2._h, 0, C.byref(k), C.byref(n), None) == ARG
    assert L.dsh_point_store_get_embedding(st2._h, 0, None, None, None) == ARG and L.dsh_point_store_get_points(st2._h, 0, None, None, None, None, None, None) == ARG
    st2.close()
    st.close()
    ctx.close()
