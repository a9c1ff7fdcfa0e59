"""The warp-pair shim (integration/schwarp_store_hip.h) compiled against stand-in KeyFrame / MapPoint types and run on the device:
SchwarpDatabase::add of one new keyframe with three anchors, the store route (SetViewStoreHIP, SchwarpDatabaseStoreHIP::add =
AnchorPairsHIP + one WarpPairStoreHIP per anchor with DropMatchHIP / DropQueryHIP between them) against the host route (a subclass of
SchwarpDatabaseHIP that calls findbyWarp / calculateSchwarps per anchor on host-gathered arrays, device records enabled).  Both leave
the objects identical -- tables, observations, nObs, bad flags, reference keyframes -- with the same x per anchor, KeyframesRelated and
the same normals from dsh_normals_estimate_db on either database, bit for bit; and the tables of the device store are the objects'."""
import os

import numpy as np
import pytest

import shim_run
import store_model
import warp_pair_ref as WP

INTEG = shim_run.INTEG


def test_shim_compiles_against_the_c_abi():
    shim_run.build()
    assert os.path.exists(shim_run.exe("warp_pair_shim_test"))
    src = open(os.path.join(INTEG, "schwarp_store_hip.h")).read()
    assert "dsh_keyframe_warp_pair" in src and "dsh_keyframe_set_view" in src and "defslam_hip_debug.h" not in src and "dsh_lab" not in src


def _tail(sc, m):
    fl = lambda v: " ".join(repr(float(x)) for x in np.asarray(v, np.float32).reshape(-1))
    A = len(sc["anchors"])
    f, c0 = np.array(sc["K"][:2], np.float32), np.array(sc["K"][2:], np.float32)
    out = f"{len(m.kfs) - 1} {sc['lam']!r}\n"
    for k, kf in enumerate(m.kfs):
        a = sc["anchors"][k] if k < A else None
        b = (a or sc["anchors"][0])["bbs"]
        out += f"{b[2]} {b[5]} {b[0]!r} {b[1]!r} {b[3]!r} {b[4]!r} {fl(sc['K'])} {fl(sc['bounds'])}\n"
        N = len(kf.table)
        kpn = a["kpn"] if a else sc["kpn2"] if k == len(m.kfs) - 1 else np.zeros((N, 2), np.float32)
        px = (a["kpn"] * f + c0).astype(np.float32) if a else sc["px2"] if k == len(m.kfs) - 1 else np.zeros((N, 2), np.float32)
        for i in range(N):
            out += f"{fl(kpn[i])} {fl(px[i])}\n"
    return out


def _more(path):
    out = {}
    for ln in open(path).read().splitlines():
        w = ln.split()
        if len(w) >= 3 and w[1] in ("x", "normal", "counts", "related", "table"):
            out.setdefault(w[0], {}).setdefault(w[1], []).append([int(v) for v in w[2:]])
    return out


@pytest.mark.gpu
def test_store_route_and_host_route_agree_over_three_anchors(tmp_path):
    from defslam_amd import synth
    shim_run.build()
    sc = synth.make_warp_pair_scene(200, 40, 25, n_anchors=3, seed=23, nu=5, nv=6, outliers=0.15)
    m = WP.build_model(sc)
    src, dst = str(tmp_path / "map.txt"), str(tmp_path / "out.txt")
    store_model.write_scene(m, src, _tail(sc, m))
    shim_run.run("warp_pair_shim_test", src, dst)
    got, more = store_model.parse_dump(dst), _more(dst)
    assert set(got) == {("store", "pair"), ("host", "pair")} and set(more) == {"store", "host"}
    s, h = got[("store", "pair")], got[("host", "pair")]
    for n in ("bad", "n_obs", "ref", "obs", "tables", "parents", "kf_bad"):
        assert s[n] == h[n], n
    counts = more["store"]["counts"]                             # slot, filtered, matched, list, dropped, stored, skipped, fitted
    print(counts)
    assert [c[0] for c in counts] == [0, 1, 2] and all(c[7] for c in counts)
    assert sum(c[1] for c in counts) > 0 and sum(c[2] for c in counts) > 0 and sum(c[4] for c in counts) > 0 and all(c[6] == 0 for c in counts)
    assert more["store"]["x"] == more["host"]["x"] and len(more["store"]["x"]) == 3
    assert more["store"]["related"] == more["host"]["related"] == [[3]]
    assert more["store"]["normal"] == more["host"]["normal"] and len(more["store"]["normal"]) == sum(c[5] for c in counts)
    assert [t[1:] for t in more["store"]["table"]] == s["tables"]  # the device store holds what the objects hold
    # and the objects moved: the new keyframe lost its filtered and dropped matches and gained the searched ones
    new = len(m.kfs) - 1
    before = m.kfs[new].table
    assert s["tables"][new] != before and sum(t >= 0 for t in s["tables"][new]) == sum(t >= 0 for t in before) + sum(c[2] - c[1] - c[4] for c in counts)
