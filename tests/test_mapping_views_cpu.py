"""CPU: the warp-guided match search and the Schwarp fit away from the one view every other mapping test uses (tests/mapping_views.py).
The C oracle is the reference of test_mapping_views_gpu.py and had itself been held against an independent statement at one view only:
here it equals the numpy brute force at every view; every scene holds the edge cases it was made for (counted and printed); and the
brute force with one error each (MUTANTS) gives other answers, so the scenes can tell these errors apart.  The conditions the GPU tests
put on the fit cases are asserted on the oracle alone."""
import numpy as np
import pytest

import mapping_views as mv


@pytest.fixture(scope="module")
def scenes():
    return {name: mv.match_scene(name) for name in mv.NAMES}


@pytest.fixture(scope="module")
def truth(scenes):
    """The brute force with its details, once per view."""
    return {name: mv.brute_force(scenes[name], mv.VIEWS[name], detail=True) for name in mv.NAMES}


def test_the_scenes_have_the_sizes_the_issue_asks_for(scenes):
    for name, sc in scenes.items():
        Q, N2 = sc["kp1"].shape[0], sc["kp2"].shape[0]
        print(f"[{name}] {Q} queries, {N2} key points in keyframe 2")
        assert Q == 130 and Q % 4 and 300 <= N2 <= 500 and N2 % 64
        assert np.array_equal(sc["cam2"], np.array(mv.VIEWS[name][0], np.float32)) and np.array_equal(sc["bounds2"], np.array(mv.VIEWS[name][1], np.float32))
    assert mv.VIEWS["fine"][2][0] * mv.VIEWS["fine"][2][1] == 8192
    w, h = mv.inv_cell(mv.VIEWS["pow2"])
    assert w == h == np.float32(1 / 16)


@pytest.mark.parametrize("name", mv.NAMES)
def test_oracle_equals_the_brute_force_at_every_view(oracle_mod, scenes, truth, name):
    sc, view = scenes[name], mv.VIEWS[name]
    args, kw = mv.search_args(sc, view)
    m = oracle_mod.search_by_schwarp(sc["bbs"], *args, **kw)
    exp = truth[name][0]
    bad = np.flatnonzero(m != exp)
    assert bad.size == 0, (name, bad, m[bad], exp[bad])
    if name == "fine":                                      # the second radius of the GPU test
        kw["radius"] = 40.0
        m = oracle_mod.search_by_schwarp(sc["bbs"], *args, **kw)
        np.testing.assert_array_equal(m, mv.brute_force(sc, view[:3] + (40.0, view[4])))
        assert (m >= 0).sum() >= 13


def _hamming(a, b):
    return int(np.unpackbits(a ^ b).sum())


@pytest.mark.parametrize("name", mv.NAMES)
def test_every_scene_holds_what_it_was_made_for(scenes, truth, name):
    sc, view = scenes[name], mv.VIEWS[name]
    K, bounds, (cols, rows), radius, th_low = view
    minX, maxX, minY, maxY = (np.float32(v) for v in bounds)
    exp, d = truth[name]
    px, py, cx, cy = d["px"], d["py"], d["cx"], d["cy"]
    Q = exp.size
    k2 = sc["kp2"]
    n = {}
    n["matched"] = int((exp >= 0).sum())
    n["out_left"], n["out_right"] = int((px < minX).sum()), int((px >= maxX).sum())
    n["out_top"], n["out_bottom"] = int((py < minY).sum()), int((py >= maxY).sum())
    win = [w for w in d["windows"] if w is not None]
    n["clamp_left"], n["clamp_right"] = sum(w[0] < 0 for w in win), sum(w[1] > cols - 1 for w in win)
    n["clamp_top"], n["clamp_bottom"] = sum(w[2] < 0 for w in win), sum(w[3] > rows - 1 for w in win)
    r = np.float32(radius)
    n["near_but_in_no_cell"] = 0
    for q in range(Q):
        if d["windows"][q] is not None:
            near = (np.abs(k2[:, 0] - px[q]) < r) & (np.abs(k2[:, 1] - py[q]) < r)
            n["near_but_in_no_cell"] += int((near & ((cx == cols) | (cy == rows))).sum())
    below = (k2[:, 0] < minX) & (cx == 0) & d["ingrid"]
    n["below_minX_in_column_0"] = int(below.sum())
    n["below_minX_and_matched"] = int(np.isin(exp[exp >= 0], np.flatnonzero(below)).sum())
    # a tie in distance decided by the cell: the winner has the smallest key, and a candidate with the same distance and a LOWER index
    # lies in a later cell
    n["tie_decided_by_cell"] = 0
    for q in range(Q):
        if exp[q] >= 0:
            best = min(d["keys"][q])
            n["tie_decided_by_cell"] += any(k[0] == best[0] and k[3] < best[3] and k[1:3] > best[1:3] for k in d["keys"][q])
    # a candidate with a map point would have won: the answer without the flags is such a candidate
    free = mv.brute_force(sc, view, has_mp2=np.zeros_like(sc["has_mp2"]))
    n["taken_would_have_won"] = int(((free != exp) & (free >= 0) & (sc["has_mp2"][np.maximum(free, 0)] != 0)).sum())
    half = ((d["vx"] - np.floor(d["vx"])) == 0.5) & ((d["vy"] - np.floor(d["vy"])) == 0.5)
    n["on_half_cell"] = int(half.sum())
    n["at_radius"] = sum(int(((np.abs(k2[:, 0] - px[q]) == r) & (np.abs(k2[:, 1] - py[q]) < r)).sum()) for q in range(Q) if d["windows"][q] is not None)
    print(f"\n[{name}] " + ", ".join(f"{k} {v}" for k, v in n.items()))
    assert n["matched"] >= (Q + 9) // 10
    if name == "pow2":
        assert n["matched"] >= 5 and all(_hamming(sc["desc1"][q], sc["desc2"][exp[q]]) == 0 for q in range(Q) if exp[q] >= 0)
        assert n["on_half_cell"] >= 10
    for side in ("left", "right", "top", "bottom"):
        assert n["out_" + side] >= 1 and n["clamp_" + side] >= 1, side
    assert n["near_but_in_no_cell"] >= 1
    assert n["below_minX_in_column_0"] >= 1 and n["below_minX_and_matched"] >= 1
    if cols * rows > 1:                                     # one cell cannot order anything
        assert n["tie_decided_by_cell"] >= 1
    assert n["taken_would_have_won"] >= 1
    assert n["at_radius"] >= 1
    # the placed items are where the scene says, after the shuffle
    for j in sc["placed_kp2"]["taken"]:
        assert sc["has_mp2"][j] == 1


def test_every_mutant_is_caught_where_it_applies_and_by_two_views(scenes, truth):
    names = list(mv.MUTANTS) + list(mv.EXTRA_MUTANTS)
    caught = {}
    for mut in names:
        for name in mv.NAMES:
            caught[mut, name] = int((mv.brute_force(scenes[name], mv.VIEWS[name], mutant=mut) != truth[name][0]).sum())
    print("\nqueries whose answer a mutant changes ('-': does not apply at that view)")
    print(f"{'':24s}" + "".join(f"{n:>10s}" for n in mv.NAMES))
    for mut in names:
        print(f"{mut:24s}" + "".join(f"{str(caught[mut, n]) + ('' if mv.applies(mut, n) else '-'):>10s}" for n in mv.NAMES))
    for mut in names:
        for name in mv.NAMES:
            if mv.applies(mut, name):
                assert caught[mut, name] >= 1, (mut, name)
        if mut in mv.EQUIVALENT:                            # mapping_views.py says why no scene can catch it
            assert not any(caught[mut, n] for n in mv.NAMES), mut
        elif mut in mv.MUTANTS:
            assert sum(caught[mut, n] > 0 for n in mv.NAMES) >= 2, mut
    assert caught["half_to_even", "pow2"] >= 1


# ---- the fit at other cameras: conditions on the cases of the GPU test, with the oracle alone -------------------------------------------
@pytest.mark.parametrize("point,grid,P", mv.FIT_PARAMS, ids=mv.FIT_IDS)
def test_fit_cases_accept_and_reject_steps_and_keep_their_matches(oracle_mod, point, grid, P):
    pr = mv.fit_problem(point, grid, P)
    assert (pr["fx"], pr["fy"]) == mv.FIT_POINTS[point][:2]
    x, diff, drop, info, costs = mv.oracle_fit(oracle_mod, pr)
    print(f"\n[fit {point} {grid[0]}x{grid[1]}] {info[0]} iterations, {info[1]} accepted, {int(drop.sum())} of {P} dropped, cost {costs[0]:.6g} -> {costs[1]:.6g}")
    assert 1 <= info[1] < info[0] <= mv.FIT_ITERS
    assert costs[1] < costs[0] * (1 - 1e-3)
    assert drop.sum() <= P // 2
    np.testing.assert_array_equal(drop, mv.drop_rule(oracle_mod, pr, x))       # the rule restated, at the final control points
    if point == "aniso":
        other = mv.drop_rule(oracle_mod, pr, x, exchanged=True)
        only, only_exchanged = int((drop & ~other).sum()), int((~drop & other).sum())
        print(f"    dropped, but kept with fx and fy exchanged: {only}; kept, but dropped with them exchanged: {only_exchanged}")
        assert only >= 2 and only_exchanged >= 2


@pytest.mark.parametrize("point,P", mv.FILTER_PARAMS)
def test_filter_cases_remove_some_matches_and_keep_some(oracle_mod, point, P):
    pr = mv.filter_problem(point, P)
    ok, x = oracle_mod.warp_initialize(pr["bbs"], pr["kp1"], pr["kp2"], mv.FILTER_LAMBDA)
    assert ok
    res, _ = oracle_mod.schwarp_eval_initial(pr["bbs"], pr["kp1"], pr["kp2"], pr["invsig"], pr["fx"], pr["fy"], x)
    out = res[2 * np.arange(P)] ** 2 + res[2 * np.arange(P) + 1] ** 2 > 20
    print(f"\n[filter {point} P {P}] {int(out.sum())} of {P} removed")
    assert 1 <= out.sum() < P
    # the decisions are far from the threshold's rounding edge: the GPU test asks for the same matches exactly
    e = res[2 * np.arange(P)] ** 2 + res[2 * np.arange(P) + 1] ** 2
    assert np.abs(e - 20).min() > 1e-4
