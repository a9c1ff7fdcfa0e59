"""The ORB front end's shim (integration/orb_extractor_hip.h) compiled against stand-in types: one frame through ORBextractorHIP::operator()
gives the key points and descriptors of the Python path, byte for byte, and both equal the restatement (tests/orb_ref.py)."""
import os

import numpy as np
import pytest

import orb_ref as R
import orb_scenes as S
import shim_run


def test_orb_shim_compiles_against_the_c_abi():
    shim_run.build()
    assert os.path.exists(shim_run.exe("orb_shim_test"))
    src = open(os.path.join(shim_run.INTEG, "orb_extractor_hip.h")).read()
    assert "defslam_hip_debug.h" not in src and "dsh_lab" not in src and "ORBextractorHIP" in src
    assert "not verified against an OpenCV build" in src


@pytest.mark.gpu
def test_orb_shim_equals_the_python_path_and_the_restatement(tmp_path, gpu_ctx):
    from defslam_amd import orb
    shim_run.build()
    case, n_features, capacity = "three_levels", 60, 4096
    w, h, levels = S.CASES[case]
    ref = S.reference(case, "noise")
    pat = S.pattern(corners=True)
    with open(tmp_path / "frame.txt", "w") as f:
        f.write(f"{w} {h} {levels} {S.SCALE} {S.INI_TH} {S.MIN_TH} {n_features} {capacity}\n")
        f.write(" ".join(str(int(v)) for v in pat.ravel()) + "\n")
        f.write(" ".join(str(int(v)) for v in ref["image"].ravel()) + "\n")
    shim_run.run("orb_shim_test", tmp_path / "frame.txt", tmp_path / "out.txt", "0")
    tok = open(tmp_path / "out.txt").read().split()
    n = int(tok[0])
    rows = np.array(tok[1:], dtype=object).reshape(n, 38)
    ex = orb.OrbExtractor(gpu_ctx, w, h, pat, levels=levels, scale_factor=S.SCALE, ini_th=S.INI_TH, min_th=S.MIN_TH, capacity=capacity, n_features=n_features)
    try:
        got = ex.extract(ref["image"], S.top_n)
    finally:
        ex.close()
    assert n == len(got["octave"]) == n_features                       # noise: every level has more candidates than wanted
    f5 = np.array(rows[:, :5], np.float32)
    assert f5[:, 0:2].tobytes() == got["pt"].tobytes() and f5[:, 2].tobytes() == got["size"].tobytes()
    assert f5[:, 3].tobytes() == got["angle"].tobytes() and f5[:, 4].tobytes() == got["response"].tobytes()
    assert rows[:, 5].astype(np.int32).tolist() == got["octave"].tolist()
    assert rows[:, 6:].astype(np.uint8).tobytes() == got["desc"].tobytes()
    want = R.extract(ref["image"], pat, S.top_n, levels, S.SCALE, S.INI_TH, S.MIN_TH, n_features=n_features, pyr=ref["pyr"], cand=ref["cand"])
    for k in ("pt", "octave", "size", "angle", "response"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert not ((got["desc"] ^ want["desc"]) & ~want["fragile"]).any()
