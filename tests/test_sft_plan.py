"""The launch shape of an SfT batch is a value: sft_plan_batch (defslam_amd/csrc/sft_plan.h) is a function of the problems' sizes, the
batch size, the CU count and the options.  A stand-alone program (own main, host compiler, no GPU, no HIP library linked) calls it at
every hand-over point for devices of 32, 64, 256 and 304 CUs; the expected shapes restate the rules of DESIGN.md 4.0 in Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAIN = r"""
#include <cstdio>
#include <vector>
#include "defslam_amd/csrc/sft_plan.h"
// stdin: the size records "R n nA Dn kd M S Es max_iters", then the cases "C cus B record"; a case is a batch of B copies of the record
int main() {
  std::vector<SftSizes> recs;
  char kind;
  while (std::scanf(" %c", &kind) == 1) {
    if (kind == 'R') {
      SftSizes z;
      if (std::scanf("%d %d %d %d %d %d %d %d", &z.n, &z.nA, &z.Dn, &z.kd, &z.M, &z.S, &z.Es, &z.max_iters) != 8) return 2;
      recs.push_back(z);
    } else {
      int cus, B, r;
      if (std::scanf("%d %d %d", &cus, &B, &r) != 3 || r < 0 || r >= (int)recs.size() || B < 1) return 2;
      const std::vector<SftSizes> batch(B, recs[r]);
      const SftBatchPlan p = sft_plan_batch(batch.data(), B, cus, SftOptions{}, false, SftUploadMode::batch);
      if ((int)p.prob.size() != B) return 3;
      for (int b = 1; b < B; b++)   // equal problems get equal decisions
        if (p.prob[b].tile_mode != p.prob[0].tile_mode || p.prob[b].split != p.prob[0].split) return 4;
      std::printf("%d %d %d %d %d %d %d %d %d\n", cus, B, r, p.nw, (int)p.rounds_mode, p.K, p.nh, p.prob[0].tile_mode, p.prob[0].split);
    }
  }
  return 0;
}
"""


def _sizes(host_ctx, cfg):
    """The sizes dsh_sft_batch_problem_info reports for one problem of a synth configuration, packed on a host-only context, as the record
    the plan reads (S: the reference's curvature edge count -- it only places records in LDS, which no value printed here depends on)."""
    from defslam_amd import sft, synth
    tmpl, fr = synth.make_problem(cfg)
    host_ctx.template_build(tmpl.xyz0, tmpl.facets)
    host_ctx.batch_upload([sft.frame_from_synth(fr)], synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    M, nA, n_curv, Es, _V, D, kd = (int(v) for v in host_ctx.problem_info(0)[1][:7])
    return dict(n=int(tmpl.xyz0.shape[0]), nA=nA, Dn=D - 6, kd=kd, M=M, S=n_curv, Es=Es, max_iters=50)


def _expected(z, cus, B):
    """DESIGN.md 4.0 and tests/test_sft_gpu.py::test_launch_shapes_between_latency_mode_and_rounds, product defaults."""
    kd, Dn = z["kd"], z["Dn"]
    tile = 1 if kd <= 128 else (2 if kd <= 256 else 0)
    rounds = tile == 1 and 2 * B > cus                 # rounds iff every problem is register-window and more than half a problem per CU
    nw = 4 if rounds else 8
    lanes = 1 if rounds else (4 if 4 * B <= cus else (3 if 3 * B <= cus else (2 if 2 * B <= cus else 1)))
    sT = -(-kd // 16)                                   # the cut: a separator of one bandwidth between two parts of >= 4 tile columns
    sp = 16 * sT
    c0 = ((Dn - sp) // 2 // 16) * 16
    room = sT >= 2 and c0 >= 64 and Dn - sp - c0 >= 64
    if tile == 2 and sT >= 12 and room and lanes == 4 and 24 * B > cus >= 12 * B:
        lanes = 2                                       # a cut wide band: two lanes with helpers rather than four without
    if lanes > 1 and tile == 1 and 20 * B <= cus and kd > 16 and Dn >= 8 * 16 * sT:
        tile = 2                                        # promotion of a narrow band to the two-sided factorisation
    split = int(lanes > 1 and tile == 2 and room)
    nh = 0
    if split and sT >= 12:
        nh = max(h for h in range(4) if h == 0 or 2 * B * lanes * (1 + h) <= cus)
        nh = 0 if nh == 1 else nh                       # one helper counts as none
    return nw, int(rounds), lanes, nh, tile, split


def test_plan_at_the_hand_over_points_of_four_device_sizes(host_ctx, tmp_path):
    recs = [_sizes(host_ctx, "C2"), _sizes(host_ctx, "W16")]
    assert recs[0]["kd"] <= 128 < recs[1]["kd"] <= 256
    cases = []
    for cus in (32, 64, 256, 304):
        for B in sorted({1, cus // 20, cus // 20 + 1, cus // 4, cus // 4 + 1, cus // 3 + 1, cus // 2, cus // 2 + 1, 2 * cus}):
            cases += [(cus, B, r) for r in range(len(recs))]
    src = tmp_path / "plan_main.cpp"
    src.write_text(MAIN)
    exe = tmp_path / "plan_main"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")   # sft_problem.h declares the launchers next to the records: HIP's types, none of its code
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", ROOT, "-I", os.path.join(rocm, "include"), str(src),
                    os.path.join(ROOT, "defslam_amd", "csrc", "sft_plan.cpp"), "-o", str(exe)], check=True)
    keys = ["n", "nA", "Dn", "kd", "M", "S", "Es", "max_iters"]
    text = "".join("R " + " ".join(str(z[k]) for k in keys) + "\n" for z in recs) + "".join("C %d %d %d\n" % c for c in cases)
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert [row[:3] for row in rows] == cases
    seen = set()
    for row in rows:
        cus, B, rec = row[:3]
        assert row[3:] == _expected(recs[rec], cus, B), (cus, B, "C2" if rec == 0 else "W16", "nw, rounds, K, nh, tile_mode, split")
        seen.add(row[3:])
    # the cases reach every shape: rounds, 4 / 3 / 2 / 1 lanes, promoted and not, cut with and without helpers, the persistent kernel on a wide band
    assert {s[2] for s in seen} == {1, 2, 3, 4} and {s[3] for s in seen} == {0, 3}
    assert (4, 1, 1, 0, 1, 0) in seen and (8, 0, 4, 0, 2, 1) in seen and (8, 0, 4, 0, 1, 0) in seen and (8, 0, 1, 0, 2, 0) in seen
