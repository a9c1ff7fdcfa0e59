"""The ORB front end on the device against its restatement (tests/orb_ref.py), exactly: planes byte for byte, candidates in count, order,
coordinates and response, angles bit for bit, descriptors on every bit that is not fragile (a sample whose rotated coordinate lies within
1e-4 of a rounding boundary: at most 1 % of a case's bits, tests/test_orb_cpu.py; measured 0.04 .. 0.12 %)."""
import numpy as np
import pytest

import orb_ref as R
import orb_scenes as S

pytestmark = pytest.mark.gpu
CASE_NAMES = list(S.CASES)


def extractor(ctx, case, capacity=None, corners=True):
    from defslam_amd import orb
    w, h, levels = S.CASES[case]
    if capacity is None:
        capacity = 32768 if case == "default" else 8192
    return orb.OrbExtractor(ctx, w, h, S.pattern(corners=corners), levels=levels, scale_factor=S.SCALE, ini_th=S.INI_TH, min_th=S.MIN_TH,
                            capacity=capacity)


def same_candidates(got, want):
    assert [len(g) for g in got] == [len(w) for w in want]
    for l, (g, w) in enumerate(zip(got, want)):
        assert g.tobytes() == w.tobytes(), (l, int(np.argmax((g != w).any(1))))


@pytest.mark.parametrize("case", CASE_NAMES)
def test_planes_and_candidates_equal_the_restatement(gpu_ctx, case):
    ex = extractor(gpu_ctx, case)
    try:
        wh, sf = ex.level_sizes()
        w, h, levels = S.CASES[case]
        assert [tuple(r) for r in wh.tolist()] == R.level_sizes(w, h, levels, S.SCALE) and sf.tobytes() == R.scale_table(levels, S.SCALE)[0].tobytes()
        for kind in S.KINDS:
            ref = S.reference(case, kind)
            got = ex.detect(ref["image"])
            if kind in ("shapes", "noise"):
                for l, (_, framed, blurred) in enumerate(ref["pyr"]):
                    assert ex.plane(l, 0).tobytes() == framed.tobytes(), (kind, l, "level and frame")
                    assert ex.plane(l, 1).tobytes() == blurred.tobytes(), (kind, l, "blurred")
            same_candidates(got, ref["cand"])
            if kind == "flat":
                assert all(len(g) == 0 for g in got)
            if kind in ("noise", "faint"):
                assert sum(len(g) for g in got) > 0
    finally:
        ex.close()


@pytest.mark.parametrize("case", CASE_NAMES)
@pytest.mark.parametrize("kind", ["shapes", "noise"])
def test_angles_and_descriptors_equal_the_restatement(gpu_ctx, case, kind):
    lv, xy, angle, desc, frag = S.described(case, kind)
    assert len(lv) >= 100
    ex = extractor(gpu_ctx, case)
    try:
        ex.detect(S.reference(case, kind)["image"])
        got_angle, got_desc = ex.describe(lv, xy)
        assert got_angle.tobytes() == angle.tobytes(), int(np.argmax(got_angle != angle))
        wrong = (got_desc ^ desc) & ~frag
        assert not wrong.any(), (int(np.count_nonzero(wrong)), int(np.argmax(wrong.any(1))))
        # the same calls again: identical bytes
        again = ex.detect(S.reference(case, kind)["image"])
        same_candidates(again, S.reference(case, kind)["cand"])
        a2, d2 = ex.describe(lv, xy)
        assert a2.tobytes() == got_angle.tobytes() and d2.tobytes() == got_desc.tobytes()
    finally:
        ex.close()


def test_capacity_overflow_reports_the_true_counts(gpu_ctx):
    from defslam_amd import _lib
    from defslam_amd.sft import DshError
    ref = S.reference("three_levels", "noise")
    want = [len(c) for c in ref["cand"]]
    cap = want[1] + 5                                      # level 0 overflows, levels 1 and 2 fit
    assert want[0] > cap >= want[1] > want[2]
    ex = extractor(gpu_ctx, "three_levels", capacity=cap)
    try:
        with pytest.raises(DshError) as e:
            ex.detect(ref["image"])
        assert e.value.status == _lib.DSH_ERR_ARG and "level 0" in str(e.value) and str(want[0]) in str(e.value)
        assert e.value.counts.tolist() == want
    finally:
        ex.close()


def test_describe_needs_an_image_and_a_padded_image_is_the_same(gpu_ctx):
    from defslam_amd.sft import DshError
    ref = S.reference("four_cells", "shapes")
    ex = extractor(gpu_ctx, "four_cells")
    try:
        with pytest.raises(DshError, match="status 3"):
            ex.describe(np.zeros(1, np.int32), np.full((1, 2), 30, np.float32))
        with pytest.raises(DshError, match="status 3"):
            ex.plane(0, 0)
        h, w = ref["image"].shape
        padded = np.full((h, w + 13), 255, np.uint8)
        padded[:, :w] = ref["image"]
        same_candidates(ex.detect(padded[:, :w]), ref["cand"])
        assert ex.plane(0, 0).tobytes() == ref["pyr"][0][1].tobytes()
    finally:
        ex.close()


@pytest.mark.parametrize("case", ["three_levels", "default"])
def test_extract_with_a_stand_in_distribution_equals_the_restatement(gpu_ctx, case):
    ref = S.reference(case, "shapes")
    w, h, levels = S.CASES[case]
    pat = S.pattern(corners=False)
    want = R.extract(ref["image"], pat, S.top_n, levels, S.SCALE, S.INI_TH, S.MIN_TH, n_features=300, pyr=ref["pyr"], cand=ref["cand"])
    from defslam_amd import orb
    ex = orb.OrbExtractor(gpu_ctx, w, h, pat, levels=levels, scale_factor=S.SCALE, ini_th=S.INI_TH, min_th=S.MIN_TH, capacity=8192, n_features=300)
    try:
        got = ex.extract(ref["image"], S.top_n)
    finally:
        ex.close()
    assert len(got["octave"]) == len(want["octave"]) > 30 and (np.diff(got["octave"]) >= 0).all()
    for k in ("pt", "octave", "size", "angle", "response"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    assert not ((got["desc"] ^ want["desc"]) & ~want["fragile"]).any()
    assert float(np.unpackbits(want["fragile"]).mean()) <= 0.01


def test_an_extractor_survives_its_context():
    from defslam_amd import _lib, orb, sft
    ctx = sft.Context(0)
    ref = S.reference("one_cell", "noise")
    ex = orb.OrbExtractor(ctx, 62, 62, S.pattern(), levels=1)
    same_candidates(ex.detect(ref["image"]), ref["cand"])
    ctx.close()
    out = np.zeros((100, 100), np.uint8)
    assert ex._L.dsh_orb_get_plane(ex._h, 0, 0, out.ctypes.data_as(_lib.c_u8_p)) == _lib.DSH_ERR_ARG      # detached: refused, not run
    ex.close()
