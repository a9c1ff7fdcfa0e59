"""TEST INFRASTRUCTURE ONLY: restatement of the per-anchor body of SchwarpDatabase::add, written from the reference's lines and not
from the kernels:

  DefORBmatcher::findbyWarp                      Modules/Matching/DefORBmatcher.cc:47-71
  DefORBmatcher::CalculateInitialSchwarp         Modules/Matching/DefORBmatcher.cc:111-187   (the filter, :155-186)
  SchwarpDatabase::calculateSchwarps             Modules/Mapping/SchwarpDatabase.cc:268-346  (the loop over the matches)
  mvInvLevelSigma2                               Thirdparty/ORBSLAM_2/src/ORBextractor.cc:422,430

WarpPairRef holds the integer bookkeeping twice: *_seq is a literal transcription of the reference's loops over the map of
tests/store_model.py with the erase of tests/point_erase_ref.py; *_par is the formulation include/defslam_hip.h states for the device
(elections by list position, repeated until the alive flags stop changing).  The numeric stages are not restated: the GPU test runs
them through the library's own one-shot calls.  Also here: the float32 inverse sigma, Ceres' corrector with its sequential sum, and the
map of a synth.make_warp_pair_scene.  Nothing in defslam_amd/ imports this module."""
from __future__ import annotations

import copy

import numpy as np

from point_erase_ref import EraseRefMap, zero_counts

f32 = np.float32
NO_MATCH, FILTERED, UNFITTED, SKIPPED, DROPPED, KEPT, STORED = range(7)
NONE = 0x7FFFFFFF


def inv_sigma(scale_factors, octave):
    """sqrt(mvInvLevelSigma2[octave]) in float32, every operation rounded (ORBextractor.cc:422,430; DefORBmatcher.cc:133-135)."""
    sf = np.asarray(scale_factors, f32)[np.asarray(octave, np.int64)]
    sigma2 = (sf * sf).astype(f32)
    return np.sqrt((f32(1.0) / sigma2).astype(f32)).astype(f32)


def corrected(res, P):
    """The block of 2P residuals as ceres::Problem::Evaluate returns it under HuberLoss(5.77): the sum in index order."""
    r = np.array(res[:2 * P], np.float64)
    s = 0.0
    for v in r:
        s = s + v * v
    if s > 5.77 * 5.77:
        r = r * np.sqrt(5.77 / np.sqrt(s))
    return r


def filter_flags(res, P):
    """DefORBmatcher.cc:167-175: match i goes when residuals[2i]^2 + residuals[2i+1]^2 > 20 -- entries 2i and 2i+1 of the array
    [x_0 .. x_{P-1}, y_0 .. y_{P-1}], two neighbouring x- (or y-) residuals."""
    r = corrected(res, P)
    return np.array([r[2 * i] * r[2 * i] + r[2 * i + 1] * r[2 * i + 1] > 20 for i in range(P)], bool)


class WarpPairRef(EraseRefMap):
    # ---- stages 3 and 4, sequential (DefORBmatcher.cc:167-186 and :57-70) ----
    def filter_register_seq(self, anchor, slot, pair_idx1, pair_idx2, filtered, query_idx1, match):
        """-> (kept list [(idx1, idx2, src)], pair_state, query_state, query_point, query_added); src: pair i, or n_pairs + query j."""
        P, Q = len(pair_idx1), len(query_idx1)
        pair_state, query_state = np.full(P, UNFITTED, np.uint8), np.full(Q, NO_MATCH, np.uint8)
        query_point, query_added = np.full(Q, -1, np.int32), np.zeros(Q, bool)
        kept = []
        for i in range(P):
            if filtered[i]:
                self.erase_map_point_match(slot, int(pair_idx2[i]))            # :172 KF2->EraseMapPointMatch
                pair_state[i] = FILTERED
            else:
                kept.append((int(pair_idx1[i]), int(pair_idx2[i]), i))
        found = [(j, int(query_idx1[j]), int(match[j])) for j in range(Q) if match[j] >= 0]   # vMatchedIndices2, in query order
        for j, i1, i2 in found:                                                 # :58-66
            p = self.kfs[anchor].table[i1]
            query_state[j] = UNFITTED
            if p != -1:
                query_point[j] = p
                query_added[j] = self.add_observation(p, slot, i2)              # AddObservation, with its early return
                self.kfs[slot].table[i2] = p                                    # addMapPoint
        kept += [(i1, i2, P + j) for j, i1, i2 in found]                        # :67-69
        return kept, pair_state, query_state, query_point, query_added

    # ---- the same as the header states it ----
    def filter_register_par(self, anchor, slot, pair_idx1, pair_idx2, filtered, query_idx1, match):
        P, Q = len(pair_idx1), len(query_idx1)
        T1, T2 = self.kfs[anchor].table, self.kfs[slot].table
        pair_state = np.where(np.asarray(filtered, bool), FILTERED, UNFITTED).astype(np.uint8)
        for i in range(P):
            if filtered[i]:
                T2[int(pair_idx2[i])] = -1
        kept = [(int(pair_idx1[i]), int(pair_idx2[i]), i) for i in range(P) if not filtered[i]]
        pt = [T1[int(query_idx1[j])] if match[j] >= 0 else -1 for j in range(Q)]
        first, last = {}, {}
        for j in range(Q):
            if match[j] >= 0 and pt[j] >= 0:
                first[pt[j]] = min(first.get(pt[j], NONE), j)
                last[int(match[j])] = max(last.get(int(match[j]), -1), j)
        query_added = np.array([match[j] >= 0 and pt[j] >= 0 and first[pt[j]] == j and not self.live(pt[j], slot) for j in range(Q)], bool)
        for j in range(Q):                                                      # the records in ascending query order
            if query_added[j]:
                assert self.add_observation(pt[j], slot, int(match[j]))
        for j in range(Q):
            if match[j] >= 0 and pt[j] >= 0 and last[int(match[j])] == j:
                T2[int(match[j])] = pt[j]
        kept += [(int(query_idx1[j]), int(match[j]), P + j) for j in range(Q) if match[j] >= 0]
        query_state = np.where(np.asarray(match) >= 0, UNFITTED, NO_MATCH).astype(np.uint8)
        return kept, pair_state, query_state, np.array(pt, np.int32).reshape(Q), query_added

    # ---- stage 7, sequential (SchwarpDatabase.cc:268-346) ----
    def records_drops_seq(self, anchor, slot, kept, drop):
        """-> (state per entry, stored [(p1, idx2)] in list order, counts of the erase)."""
        c, state, stored = zero_counts(), np.zeros(len(kept), np.uint8), []
        for j, (i1, i2, _) in enumerate(kept):
            p1, p2 = self.kfs[anchor].table[i1], self.kfs[slot].table[i2]       # :270-271 GetMapPoint
            if p1 == -1 or p2 == -1 or self.points[p1].bad or self.points[p2].bad:   # :273-278
                state[j] = SKIPPED
            elif drop[j]:                                                       # :283-293
                self.map_point_erase_observation(p2, slot, c)                   # :290
                self.erase_map_point_match(slot, i2)                            # :291
                state[j] = DROPPED
            elif self.points[p1].ref != anchor:                                 # :295 only points anchored in the estimated keyframe
                state[j] = KEPT
            else:
                stored.append((p1, i2))                                         # :299-345
                state[j] = STORED
        return state, stored, c

    # ---- the same as the header states it: elections repeated until the alive flags stop changing ----
    def records_drops_par(self, anchor, slot, kept, drop):
        L = len(kept)
        T1, T2, pts = self.kfs[anchor].table, self.kfs[slot].table, self.points
        p1 = [T1[i1] for i1, _, _ in kept]
        p2 = [T2[i2] for _, i2, _ in kept]
        valid = [p1[j] >= 0 and p2[j] >= 0 and not pts[p1[j]].bad and not pts[p2[j]].bad for j in range(L)]
        anc_idx = lambda p: pts[p].obs.get(anchor, -1)

        def bad_at(first, p):   # the position at which the first alive dropped entry of p sets it bad
            j = first.get(p, NONE)
            return j if j != NONE and self.live(p, slot) and pts[p].n_obs - 1 <= 2 else NONE

        alive, rounds = list(valid), 0
        while True:
            rounds += 1
            first, win2, kill1 = {}, {}, {}
            for j in range(L):
                if alive[j] and drop[j]:
                    first[p2[j]] = min(first.get(p2[j], NONE), j)
                    win2[kept[j][1]] = min(win2.get(kept[j][1], NONE), j)
            for j in range(L):
                if alive[j] and drop[j] and first[p2[j]] == j and bad_at(first, p2[j]) == j and anc_idx(p2[j]) >= 0:
                    a = anc_idx(p2[j])
                    kill1[a] = min(kill1.get(a, NONE), j)
            new = [valid[j] and not win2.get(kept[j][1], NONE) < j and not bad_at(first, p1[j]) < j and not bad_at(first, p2[j]) < j
                   and not kill1.get(kept[j][0], NONE) < j for j in range(L)]
            if new == alive or rounds > L:
                break
            alive = new
        state, stored = np.zeros(L, np.uint8), []
        for j in range(L):
            if not alive[j]:
                state[j] = SKIPPED
            elif drop[j]:
                state[j] = DROPPED
            else:
                ref = pts[p1[j]].ref
                if first.get(p1[j], NONE) < j and self.live(p1[j], slot) and ref == slot and [k for k in pts[p1[j]].obs if k != slot]:
                    ref = min(k for k in pts[p1[j]].obs if k != slot)
                state[j] = KEPT if ref != anchor else STORED
                if state[j] == STORED:
                    stored.append((p1[j], kept[j][1]))
        c = zero_counts()
        for j in range(L):                                                      # the second pass writes
            if alive[j] and drop[j]:
                if first[p2[j]] == j:
                    self.map_point_erase_observation(p2[j], slot, c)
                T2[kept[j][1]] = -1
        return state, stored, c, rounds


def states_of(state, kept, P, pair_state, query_state):
    """The state of every kept entry written where its source lies."""
    ps, qs = pair_state.copy(), query_state.copy()
    for s, (_, _, src) in zip(state, kept):
        if src < P:
            ps[src] = s
        else:
            qs[src - P] = s
    return ps, qs


# ---- the map of a synth.make_warp_pair_scene ------------------------------------------------------------------------------------------

def view_of(sc, a=None):
    """(K, bounds, grid, scale factors) of anchor a, or of the new keyframe (a is None).  A scene made without `views` has one for all.
    The reference takes KF->fx, KF->fy and KF->mvInvLevelSigma2 from the anchor (DefORBmatcher.cc:133-135, SchwarpDatabase.cc:200-201,
    :284-285) and dKF2->fx, cx, IsInImage and GetFeaturesInArea from the new keyframe (DefORBmatcher.cc:229-247)."""
    if "views" not in sc:
        return sc["K"], sc["bounds"], sc["grid"], sc["scale_factors"]
    return sc["views"][-1 if a is None else a]


def exchanged(sc):
    """The scene with every anchor's view and the new keyframe's trading places: what a call computes that reads the wrong keyframe's
    camera, bounds, grid or scale factors.  The key points stay where they are."""
    out = dict(sc)
    out["exchange"] = True
    return out


def _views(sc, a):
    """(the view the gather, filter and fit read, the view the search reads)."""
    v1, v2 = view_of(sc, a), view_of(sc)
    return (v2, v1) if sc.get("exchange") else (v1, v2)


def build_model(sc, few_obs=(), other_ref=()):
    """The anchors at slots 0 .. A-1, two keyframes that only lend observations at A and A+1, the new keyframe at A+2.  Every pair and
    every query of every anchor is a point anchored in its anchor and observed there, in both lending keyframes (not for the points in
    few_obs: they fall to n_obs <= 2 with one erase) and -- the pairs -- in the new keyframe.  other_ref: points anchored in a lending
    keyframe instead.  -> (model, pairs per anchor as the point ids)."""
    rng = np.random.default_rng(sc["seed"] + 1000)
    m = WarpPairRef()
    A = len(sc["anchors"])
    n_pts = sum(len(a["pair_idx1"]) + len(a["query_idx1"]) for a in sc["anchors"])
    tables = [[-1] * a["kpn"].shape[0] for a in sc["anchors"]] + [[-1] * n_pts, [-1] * n_pts, [-1] * sc["kpn2"].shape[0]]
    obs, p = [], 0
    for s, a in enumerate(sc["anchors"]):
        for i1, i2 in list(zip(a["pair_idx1"], a["pair_idx2"])) + [(i1, -1) for i1 in a["query_idx1"]]:
            m.add_point(xyz=rng.normal(size=3), ref=A if p in other_ref else s)
            tables[s][int(i1)] = p
            obs.append((p, s, int(i1)))
            if p not in few_obs:
                for k in (A, A + 1):
                    tables[k][p] = p
                    obs.append((p, k, p))
            if i2 >= 0:
                tables[A + 2][int(i2)] = p
                obs.append((p, A + 2, int(i2)))
            p += 1
    for s, a in enumerate(sc["anchors"]):
        m.add_keyframe(tables[s], Ow=np.zeros(3), desc=a["desc"], octave=a["octave"], scale_factors=view_of(sc, s)[3])
    sf = view_of(sc)[3]
    for k in (A, A + 1):
        m.add_keyframe(tables[k], Ow=np.zeros(3), desc=rng.integers(0, 256, (n_pts, 32), dtype=np.uint8), octave=np.zeros(n_pts, np.int32), scale_factors=sf)
    m.add_keyframe(tables[A + 2], Ow=np.zeros(3), desc=sc["desc2"], octave=sc["octave2"], scale_factors=sf)
    for i in rng.permutation(len(obs)):
        assert m.add_observation(*obs[i])
    return m


# ---- the explicit-array route the GPU test and tools/bench_warp_pair.py compare with ---------------------------------------------------

def bbs_of(t):
    from defslam_amd.nrsfm import Bbs
    return Bbs(*t)


def stores(ctx, sc, m, observations=None, views=True):
    from defslam_amd import localmap, mappoint
    st = localmap.MapPointStore(ctx, points=max(len(m.points), 1), keyframes=len(m.kfs), observations=observations or max(4 * len(m.log), 16))
    ks = mappoint.KeyFrameStore(ctx, 2)
    m.fill(st, ks)
    new = len(m.kfs) - 1
    for s, a in enumerate(sc["anchors"]):
        st.surface_init(s, a["kpn"])
        if views:
            K, bounds, grid, _ = view_of(sc, s)
            f, c0 = np.array(K[:2], np.float32), np.array(K[2:], np.float32)
            st.set_view(s, localmap.KeyframeView((a["kpn"] * f + c0).astype(np.float32), K, bounds, *grid, bbs_of(a["bbs"])))
    st.surface_init(new, sc["kpn2"])
    if views:
        K, bounds, grid, _ = view_of(sc)
        st.set_view(new, localmap.KeyframeView(sc["px2"], K, bounds, *grid, bbs_of(sc["anchors"][0]["bbs"])))
    return st, ks


def initial(ctx, sc, a, i1, i2):
    """Stages 2 and 3 by the one-shot calls: (init_ok, x with the NaN rule applied, the filter's flags)."""
    from defslam_amd import nrsfm
    A = sc["anchors"][a]
    (K1, _, _, sf), _ = _views(sc, a)
    bbs, (fx, fy) = bbs_of(A["bbs"]), K1[:2]
    kp1, kp2, isg = A["kpn"][i1], sc["kpn2"][i2], inv_sigma(sf, A["octave"][i1])
    init_ok, x = nrsfm.WarpInitialize(ctx, bbs, kp1, kp2, sc["lam"])
    nz = min(x.size, 2 * bbs.nptsu * bbs.nptsu)
    x[:nz][np.isnan(x[:nz])] = 0.0
    res, _ = nrsfm.schwarp_eval(ctx, bbs, kp1, kp2, isg, fx, fy, 0.0, x, want_jacobian=False)
    return init_ok, x, filter_flags(res, len(i1))


def host_route(ctx, m, sc, a, i1, i2, q1, ddb, tag, min_pairs=20, max_iters=3, radius=2.0, th_low=50):
    """The explicit-array sequence for one anchor (integration/schwarp_database_hip.h: the four one-shot calls on host-gathered arrays) on
    the model m, which is mutated; the records into ddb.  The gather, the filter and the fit read the anchor's camera and scale factors,
    the search the new keyframe's camera, bounds, grid and pixel key points (view_of)."""
    from defslam_amd import nrsfm
    A, new = sc["anchors"][a], len(m.kfs) - 1
    (K1, _, _, sf), (K2, bounds2, grid2, _) = _views(sc, a)
    bbs, lam, (fx, fy) = bbs_of(A["bbs"]), sc["lam"], K1[:2]
    i1, i2, q1 = (np.asarray(v, np.int64) for v in (i1, i2, q1))
    P, Q = len(i1), len(q1)
    init_ok, x, filt = initial(ctx, sc, a, i1, i2)
    has = np.array(m.kfs[new].table) != -1
    has[i2[filt]] = False
    match = (nrsfm.searchBySchwarp(ctx, bbs, x, A["kpn"][q1], A["desc"][q1], K2, bounds2, sc["px2"], sc["desc2"], has, radius, th_low, grid2)
             if Q else np.zeros(0, np.int32))
    kept, ps, qs, qp, qa = m.filter_register_seq(a, new, i1, i2, filt, q1, match)
    out = dict(x=x, x_start=x, has=has, init_ok=init_ok, fitted=False, info=np.zeros(2, np.int32), costs=np.zeros(2), match=match, query_point=qp, query_added=qa,
               n_list=len(kept), stored=[], counts=zero_counts())
    if len(kept) >= min_pairs:
        k1 = A["kpn"][[e[0] for e in kept]]
        k2 = sc["kpn2"][[e[1] for e in kept]]
        ik = inv_sigma(sf, A["octave"][[e[0] for e in kept]])
        x2, _, drop, info, costs = nrsfm.calculateSchwarps(ctx, bbs, k1, k2, ik, fy, fx, lam, fx, fy, x, max_iters)
        state, stored, c = m.records_drops_seq(a, new, kept, drop)
        pid = np.full(len(kept), -1, np.int32)
        pid[state == STORED] = [p for p, _ in stored]
        r = nrsfm.calculateSchwarpsBatch(ctx, [dict(bbs=bbs, kp1=k1, kp2=k2, invsig=ik, fx_slot=fy, fy_slot=fx, lam=lam, fx=fx, fy=fy, x0=x, point_id=pid,
                                                    idx2=[e[1] for e in kept], tag=tag)], max_iters, db=ddb, want_records=False)[0]
        assert r[0].tobytes() == x2.tobytes() and np.array_equal(r[2], drop)
        ps, qs = states_of(state, kept, P, ps, qs)
        out.update(x=x2, fitted=True, info=info, costs=costs, stored=stored, counts=c, drop=drop)
    out.update(pair_state=ps, query_state=qs)
    return out


def clone(m):
    return copy.deepcopy(m)
