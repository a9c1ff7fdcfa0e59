"""The scene file of a MapModel (store_model.write_scene) through the shared C++ reader and dump (integration/standin_store_scene.h):
integration/store_scene_roundtrip_main.cc reads a file and dumps what it built, without a call into the library, and parse_dump of that
dump is the model's state again -- the flags, the counters, the reference keyframes, the live observations with their key point indices,
the tables with parent and bad flag, the descriptors, the keyframes' appearance, and every float as its bit pattern."""
import numpy as np
import pytest

import keyframe_insert_ref as KI
import point_erase_ref as PE
import shim_run
import store_model


def with_appearance():
    """keyframe_insert_ref.random_model(1): appearance, a blanked record, a pair erased and added again with another index, an
    observation without a key point index, a later-slot parent, counters and a minimum distance that are not the defaults."""
    m, slot = KI.random_model(1)
    p, s, idx, _ = m.log[0]
    assert m.erase_observation(p, s) and m.add_observation(p, s, (idx + 1) % len(m.kfs[s].table))
    q, t = next((r[0], r[1]) for r in m.log if (r[0], r[1]) != (p, s))
    assert m.erase_observation(q, t)
    free = next(k for k in range(len(m.kfs)) if k not in m.points[0].obs)
    assert m.add_observation(0, free)
    m.kfs[0].parent = 2
    m.points[1].found, m.points[1].visible, m.points[1].min_distance = 7, 9, m.points[1].max_distance / 3
    return m, f"{slot} 2\n0 0.5 -0.25 5.0\n"


def topology_only():
    return PE.small_scene()[0], "7\n"


@pytest.mark.parametrize("scene", [with_appearance, topology_only])
def test_reader_and_dump_give_the_model_back(tmp_path, scene):
    shim_run.build()
    m, tail = scene()
    assert all(k.has_appearance for k in m.kfs) == (scene is with_appearance)
    src, dst = tmp_path / "scene.txt", tmp_path / "dump.txt"
    store_model.write_scene(m, src, tail)
    shim_run.run("store_scene_roundtrip", src, dst)
    got = store_model.parse_dump(dst)
    assert set(got) == {("file", "read")}
    d, s = got[("file", "read")], m.state()
    assert d["bad"] == s["bad"].tolist() and d["n_obs"] == s["n_obs"].tolist() and d["ref"] == s["ref"].tolist()
    assert d["obs"] == s["obs"] and d["tables"] == s["tables"]
    assert d == store_model.dump_of(m)                                # and the counters, the descriptors and the float bits
    lines = open(dst).read().splitlines()
    assert [ln for ln in lines if ln.startswith("tail ")] == ["tail " + ln for ln in tail.splitlines()]
    app = [[part.split() for part in ln.split("|")[1:]] for ln in lines if ln.startswith("file read app ")]      # the keyframes' appearance
    bits = lambda v: [str(u) for u in np.asarray(v, np.float32).view(np.uint32)]
    assert app == [[bits(k.Ow) + bits(k.scale_factors), [str(o) for o in k.octave], [str(b) for b in k.desc.ravel()]] for k in m.kfs if k.has_appearance]
    assert len(app) == (len(m.kfs) if scene is with_appearance else 0)
    if scene is with_appearance:
        assert any(not r[3] for r in m.log) and any(-1 in o.values() for o in s["obs"]) and len(m.log) > sum(len(o) for o in s["obs"]) + 1


def test_reader_refuses_values_outside_the_scene(tmp_path):
    """A reference keyframe or a table entry below -1 and a key point index that is not in its keyframe: exit status 2, not a null pointer
    or an index read as it stands."""
    import subprocess
    shim_run.build()
    m, _ = topology_only()
    store_model.write_scene(m, tmp_path / "good.txt")
    good = [ln.split() for ln in open(tmp_path / "good.txt").read().splitlines()]
    P, K = len(m.points), len(m.kfs)
    for name, row, col, value in (("ref", 1, 9, "-5"), ("table", 1 + P, 3, "-7"), ("idx", 1 + P + K, 2, str(len(m.kfs[m.log[0][1]].table))), ("ok", 1, 9, "-1")):
        rows = [list(r) for r in good]
        rows[row][col] = value
        (tmp_path / "bad.txt").write_text("\n".join(" ".join(r) for r in rows) + "\n")
        r = subprocess.run(["timeout", "-k", "10", "120", shim_run.exe("store_scene_roundtrip"), tmp_path / "bad.txt", tmp_path / "out.txt"], capture_output=True, text=True)
        assert r.returncode == (0 if name == "ok" else 2), (name, r.returncode, r.stderr)
