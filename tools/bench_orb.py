"""Timing of the ORB front end on the device at the default frame: 640 x 480, 8 levels, scale 1.2, thresholds 20 / 7, the `shapes` image of
the tests (tests/orb_scenes.py) drawn with more shapes so that about 2000 candidates come down.
  detect     dsh_orb_detect: image up, pyramid, blur, FAST, scan, scatter, counts and candidates down
  describe   dsh_orb_describe of 1200 key points (the candidates of largest response, spread over the levels as mnFeaturesPerLevel does)
  frame      detect, the stand-in selection on the host (numpy), describe: one frame end to end
Host wall time around calls that end in a stream synchronise, medians after warm-up.  Kernel times come from a run of their own under
rocprofv3 --kernel-trace --stats (the kernels are orb_*_kernel).  With `readings` as the second argument it also prints the measured
deviations of the restatement's readings from their independent formulations (CPU, tests/orb_ref.py).  The CPU restatement's time is no
baseline and is not measured.  Prints one JSON line.
    python tools/bench_orb.py [reps] [readings]                    (profiles/orb_extract/README.md has the numbers)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import orb_ref as R   # noqa: E402
import orb_scenes as S   # noqa: E402
from defslam_amd import orb, sft   # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
W, H, LEVELS, N_KP, CAPACITY = 640, 480, 8, 1200, 8192


def timed(fn, n):
    t = []
    for r in range(max(5, n // 10) + n):
        a = time.perf_counter()
        fn()
        if r >= max(5, n // 10):
            t.append(time.perf_counter() - a)
    return dict(median_us=float(np.median(t) * 1e6), p10_us=float(np.percentile(t, 10) * 1e6), p90_us=float(np.percentile(t, 90) * 1e6))


rng = np.random.default_rng(7)
image = np.clip(S._draw_shapes(rng, W, H, 128, np.arange(10, 246), 800) + rng.integers(-2, 3, (H, W)), 0, 255).astype(np.uint8)
ctx = sft.Context(0)
ex = orb.OrbExtractor(ctx, W, H, S.pattern(), levels=LEVELS, scale_factor=S.SCALE, ini_th=S.INI_TH, min_th=S.MIN_TH, capacity=CAPACITY, n_features=N_KP)
cand = ex.detect(image)
wanted = orb.features_per_level(N_KP, LEVELS, S.SCALE)
sel = [c[S.top_n(l, c, wanted[l])] for l, c in enumerate(cand)]
lv = np.concatenate([np.full(len(s), l, np.int32) for l, s in enumerate(sel)])
xy = np.concatenate(sel)[:, :2].astype(np.float32)
out = dict(reps=reps, width=W, height=H, levels=LEVELS, candidates=[len(c) for c in cand], described=int(len(lv)),
           upload_bytes=W * H, download_bytes=4 * LEVELS + 12 * LEVELS * CAPACITY,
           detect=timed(lambda: ex.detect(image), reps), describe=timed(lambda: ex.describe(lv, xy), reps),
           frame=timed(lambda: ex.extract(image, S.top_n), reps))
out["frames_per_s"] = 1e6 / out["frame"]["median_us"]

if len(sys.argv) > 2 and sys.argv[2] == "readings":
    noise = S.image("noise", 97, 71)
    resize = max(float(np.abs(R.resize(noise, dw, dh).astype(np.float64) - R.resize_float(noise, dw, dh)).max()) for dw, dh in ((81, 59), (80, 60), (62, 62), (49, 36)))
    fr = R.frame(S.image("noise", 70, 64)).astype(np.float64)
    k = np.exp(-(np.arange(-3, 4) ** 2) / 8.0)
    k /= k.sum()
    rows = sum(k[i] * fr[:, 13 + i:13 + i + 76] for i in range(7))
    flt = sum(k[j] * rows[13 + j:13 + j + 70] for j in range(7))
    blur = float(np.abs(R.blur_plane(fr.astype(np.uint8)) - flt).max())
    m = np.random.default_rng(11).integers(-200000, 200001, (200000, 2))
    err = np.abs(R.fast_atan2(m[:, 1].astype(np.float32), m[:, 0].astype(np.float32)).astype(np.float64) - np.degrees(np.arctan2(m[:, 1], m[:, 0])) % 360.0)
    fragile = {f"{case}/{kind}": float(np.unpackbits(S.described(case, kind)[4]).mean()) for case in S.CASES for kind in ("shapes", "noise")}
    out["readings"] = dict(resize_vs_float_bilinear=resize, blur_vs_float_gaussian=blur, angle_vs_arctan2_deg=float(np.minimum(err, 360.0 - err).max()),
                           fragile_bit_share=fragile)
print(json.dumps(out))
ex.close()
ctx.close()
