"""The template switch shim (integration/template_switch_hip.h) compiled against stand-in types and run on the device: NeedNewTemplateHIP
and UpdateTemplateHIP leave the stand-in objects exactly as DefLocalMapping::needNewTemplate / updateTemplate over a second copy of them
do, and both equal the sequential restatement (tests/template_switch_ref.py)."""
import os

import numpy as np
import pytest

import template_switch_ref as S
import shim_run
from test_template_switch_cpu import make_scene

INTEG = shim_run.INTEG


def test_template_switch_shim_compiles_against_the_c_abi():
    shim_run.build()
    assert os.path.exists(shim_run.exe("tmplswitch_shim_test"))
    src = open(os.path.join(INTEG, "template_switch_hip.h")).read()
    assert "defslam_hip_debug.h" not in src and "dsh_lab" not in src
    assert "UpdateTemplateHIP" in src and "NeedNewTemplateHIP" in src


@pytest.mark.gpu
def test_template_switch_shim_device_way_host_way_and_restatement_agree(tmp_path):
    from defslam_amd import nrsfm, sft, synth
    shim_run.build()
    sc, (xs, ys) = make_scene("grow")
    synth.write_local_map_scene(sc, tmp_path / "map.txt")
    synth.write_template_switch_scene(sc, (xs, ys), tmp_path / "switch.txt")
    r = shim_run.run("tmplswitch_shim_test", tmp_path / "map.txt", tmp_path / "switch.txt", tmp_path / "out.txt", "0")
    tok = iter(open(tmp_path / "out.txt").read().split())
    N = sc["kp"].shape[0]

    def way():
        head = [int(next(tok)) for _ in range(7)]
        rows = []
        for _ in range(head[6]):
            f8 = [np.float32(next(tok)) for _ in range(8)]
            desc = [int(next(tok)) for _ in range(32)]
            ints = [int(next(tok)) for _ in range(6)]
            bary = [float(next(tok)) for _ in range(3)]
            rows.append((f8, desc, ints, bary))
        table = [int(next(tok)) for _ in range(N)]
        return head, rows, table

    dev = way()
    host = way()
    again = [int(next(tok)), int(next(tok))]
    assert dev == host and again == [0, 0]                           # the objects of the two ways: counts, every mutated field, the table

    # the restatement on the same template: the device's own vertices
    ctx = sft.Context(0)
    nodes = nrsfm.surface_vertices(ctx, nrsfm.Bbs(*sc["bbs"]), sc["depth_ctrl"], sc["Twc"], xs, ys)
    ctx.template_build(nodes, synth.regular_triangulation(xs, ys))
    rm = S.scene_to_ref(sc, embed=False)
    slot = sc["ref_slot"]
    need, _ = rm.need_new_template(slot, sc["rows"], sc["cols"], sc["kp"])
    kfs = S.scene_kf_data(sc)
    c, new_idx, _ = rm.switch_template(kfs, slot, sc["rows"], sc["cols"], sc["kp"], sc["surface_pts"], sc["Twc"], ctx.template_embed, nodes)
    ctx.close()
    head, rows, table = dev
    assert head == [need] + [c[k] for k in S.COUNT_NAMES] and head[1] >= 10 and head[4] >= 10 and head[5] > 0
    assert table == rm.kfs[slot].table
    x, nrm, md, desc, bad = (rm.point_arrays()[k] for k in ("xyz", "normal", "max_distance", "desc", "bad"))
    rn, rb = rm.embedding_arrays()
    assert np.array([r[0][:3] for r in rows], np.float32).tobytes() == x.tobytes()
    assert [r[1] for r in rows] == desc.tolist() and [bool(r[2][1]) for r in rows] == bad.tolist()
    assert [r[2][0] for r in rows] == rm.state()["n_obs"].tolist()
    live = ~bad                                                      # a bad point keeps what it had: neither way touches it
    assert np.array([r[2][3:6] for r in rows], np.int32)[live].tolist() == rn[live].tolist()
    assert np.array([r[3] for r in rows], np.float64)[live].tobytes() == rb[live].tobytes()
    P0 = sc["xyz"].shape[0]
    sf_last = sc["scale_factors"][-1]
    for j, q in enumerate(range(P0, len(rows))):                     # the new points: normal, both distances, the observation's key point
        f8, _, ints, _ = rows[q]
        assert np.array(f8[3:6], np.float32).tobytes() == nrm[q].tobytes() and f8[6] == md[q] and f8[7] == np.float32(md[q] / sf_last)
        assert ints[2] == int(new_idx[j])
