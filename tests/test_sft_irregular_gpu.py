"""The SfT path on IRREGULAR template meshes (tests/irregular_meshes.py), CPU part and GPU part (-m gpu).

Every other SfT test builds its template with synth.make_grid_template: interior degree 6, at most 13 curvature + stretch contributions
on a diagonal block of the normal equations and 5 on an off-diagonal one, a periodic block pattern.  The C ABI takes any triangle mesh,
and these device / packer paths are taken only by meshes a grid never is (line numbers: defslam_amd/csrc/sft_kernels.hip):

  row 1  the second pass of the NCH = 8 neighbour chunk of the curvature residual (:485)         a non-boundary node of degree > 8
  row 2  the tail loop behind the 8 x HCH = 24 prefetched contributions of a diagonal block (:769)  a diagonal block with > 24
  row 3  the tail loop behind the SCH = 6 prefetched contributions of an off-diagonal block (:875)  an off-diagonal block with > 6
  row 4  SFT_REC slots 7 .. 14, `int a[kMaxDegree + 2]` (sft_pack.cpp), sh_cf through nbr_c[base + s - 1]   degree > 6
  row 5  tmask / hgather / hgatherT with a non-periodic pattern, max_slots varying by tile row     an irregular block pattern
  row 6  the edges of the degree limit: 14 accepted, 15 refused ("node degree > 14 unsupported")

MESHES names the cases; `_assert_reaches` asserts, from the library's own template constants, the property each mesh exists for (so a
change of a chunk size or of a generator names the mesh to enlarge), and the tests' docstrings say which rows they prove.
All comparisons against the oracle are test_sft_gpu.py's `_compare`, unchanged.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import irregular_meshes as im
from conftest import oracle_args
from test_sft_gpu import _compare

gpu = pytest.mark.gpu

# name -> (constructor, matches, problem id of synth.make_frame, expectations asserted by _assert_reaches)
#   deg: largest degree of a node with a curvature residual; diag / off: longest contribution list of a diagonal / off-diagonal block;
#   kd: packed half-bandwidth (full view) -> solver class: <= 128 register-window tiles, <= 256 wide tiles, above: row-major band solver
MESHES = {
    "disc14x4": (lambda: im.disc(14, 4), 300, 1, dict(n=57, deg=14, diag=29, off=5, kd=125)),          # rows 1, 2, 4, 6 (hub: degree 14, 29 contributions)
    "disc12x6": (lambda: im.disc(12, 6), 400, 2, dict(n=73, deg=12, diag=25, off=5, kd=107)),          # rows 1, 2, 4 (one element in the diagonal tail loop)
    "disc9x5": (lambda: im.disc(9, 5), 300, 3, dict(n=46, deg=9, diag=19, off=5, kd=80)),              # rows 1, 4 (second neighbour chunk with ONE element)
    "flip10x10": (lambda: im.flipped_grid(10, 10, 1), 300, 4, dict(n=100, deg=8, diag=17, off=5, kd=68)),             # rows 4, 5
    "flip12x14_holes": (lambda: im.flipped_grid(12, 14, 2, holes=6), 500, 5, dict(n=168, deg=8, diag=17, off=5, kd=92)),   # rows 4, 5 (boundary nodes inside)
    "flip8x30": (lambda: im.flipped_grid(8, 30, 7), 500, 9, dict(n=240, deg=8, diag=17, off=5, kd=188)),             # rows 4, 5, wide tiles (irregular W12)
    "flip6x41": (lambda: im.flipped_grid(6, 41, 3), 500, 6, dict(n=246, deg=8, diag=17, off=5, kd=254)),             # rows 4, 5, wide tiles (irregular W16)
    "split10x10": (lambda: im.split_grid(10, 10, (4, 4)), 300, 3, dict(n=102, deg=8, diag=17, off=7, kd=68)),        # rows 3, 4, 5
    "delaunay200": (lambda: im.delaunay_sweep(200, 4), 500, 7, dict(n=200, deg=10, diag=21, off=6, kd=458)),         # rows 1, 4, 5, band fallback
    # the widest band the library takes: kd + kNB + SFT_BORDER = 473 + 32 + 7 = 512 <= SFT_NT = 512 (the next possible kd, 476, is refused)
    "band473": (lambda: im.band_limit_grid(1), 600, 12, dict(n=309, deg=8, diag=15, off=6, kd=473)),                 # rows 4, 5, band fallback AT its limit
}
ACCEPTED = list(MESHES)
# the smallest refused neighbours of the accepted extremes
REFUSED_DEGREE = (lambda: im.disc(15, 3), 200, 9)            # hub degree 15
REFUSED_BAND = (lambda: im.delaunay_sweep(500, 5), 1000, 8)  # half-bandwidth 1043
REFUSED_BAND_EDGE = (lambda: im.band_limit_grid(2), 600, 12)  # half-bandwidth 476: the smallest that is refused (473 is taken, kd = 3 w + 2)
NARROW = ["disc14x4", "flip10x10", "split10x10"]             # kd <= 128: the one-wavefront factor kernel's range


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return MESHES[name][0]()


def _regs():
    from defslam_amd import synth
    return (synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)


def _frame(name, pid=None, m=None):
    from defslam_amd import synth
    _, m0, pid0, _ = MESHES[name]
    return synth.make_frame(_mesh(name), m0 if m is None else m, pid0 if pid is None else pid)


def _kd_class(kd):
    return "register-window" if kd <= 128 else ("wide" if kd <= 256 else "band")


def _assert_reaches(name, tg, counts):
    """The property the mesh exists for, from Context.template_get() and problem_info() of a full view."""
    exp = MESHES[name][3]
    pr = im.properties(tg)
    diag, off = max(pr["diag"].values()), max(pr["off"].values())
    got = dict(n=len(tg["boundary"]), deg=pr["max_star_degree"], diag=diag, off=off, kd=int(counts[6]))
    assert got == exp, (name, got, exp)
    assert pr["kd"] == int(counts[6])                                   # the packer's half-bandwidth is the block pattern's
    assert pr["max_degree"] <= im.MAX_DEGREE
    # which rows of the module docstring's table the mesh reaches; the lists name the mesh to enlarge if NCH, HCH or SCH change
    if name in ("disc14x4", "disc12x6", "disc9x5", "delaunay200"):
        assert got["deg"] > im.NCH, f"{name} must have a non-boundary node of degree > NCH = {im.NCH} (row 1)"
    if name == "disc9x5":
        assert got["deg"] == im.NCH + 1                                  # one element in the second chunk
    if name in ("disc14x4", "disc12x6"):
        assert got["diag"] > im.DIAG_PREFETCH, f"{name} must have a diagonal block with > {im.DIAG_PREFETCH} contributions (row 2)"
    if name == "disc12x6":
        assert got["diag"] == im.DIAG_PREFETCH + 1
    if name == "disc14x4":
        assert got["deg"] == im.MAX_DEGREE                               # row 6: the largest accepted degree
    if name == "split10x10":
        assert got["off"] > im.SCH, f"{name} must have an off-diagonal block with > SCH = {im.SCH} contributions (row 3)"
        m = _mesh(name)
        assert pr["off"][(max(m.split_edge), min(m.split_edge))] == got["off"]
    assert got["deg"] > 6                                                # row 4: record slots beyond a grid's
    assert _kd_class(got["kd"]) == {"flip8x30": "wide", "flip6x41": "wide", "delaunay200": "band", "band473": "band"}.get(name, "register-window")
    if name.startswith("flip") or name in ("split10x10", "delaunay200", "band473"):
        # row 5: no periodic block pattern -- a regular triangulation of any size has im.GRID_PATTERNS distinct block rows (column offsets with their
        # contribution counts: what tmask, the gather lists and max_slots are made from); the split grid has the defect's on top, the others several times as many
        assert pr["patterns"] > (im.GRID_PATTERNS + 16 if name == "split10x10" else 4 * im.GRID_PATTERNS), pr["patterns"]


def _partial_views():
    """(mesh, view name, nodes whose facets stay viewed): the hub / the split nodes in the 1-ring but not viewed, and not active at all;
    a corner of a flipped grid (ragged active set)."""
    k14 = 14

    def ring(k, j, idx):
        return [1 + (j - 1) * k + (i % k) for i in idx]

    half = [v for j in range(1, 5) for v in ring(k14, j, range(0, 8))]            # no hub: it stays in the 1-ring of ring 1
    rim = [v for j in (3, 4) for v in ring(k14, j, range(k14))]                   # rings 3 and 4: ring 2 is the 1-ring, ring 1 and the hub are fixed
    sp = _mesh("split10x10")
    old = [v for v in range(sp.n) if v not in sp.new_nodes]                       # old[k]: new id of grid node k (the new nodes sit behind node 45)
    upper = [old[c + 10 * r] for r in range(5) for c in range(10)]                # rows 0 .. 4: nodes 44 / 45 viewed, the two split nodes in their 1-ring
    top = [old[c + 10 * r] for r in range(3) for c in range(10)]                  # rows 0 .. 2: the split nodes are not active
    return [("disc14x4", "half_without_hub", half), ("disc14x4", "rim", rim), ("split10x10", "upper_half", upper), ("split10x10", "top_rows", top),
            ("flip10x10", "corner", [c + 10 * r for r in range(6) for c in range(6)]),
            ("flip12x14_holes", "corner", [c + 14 * r for r in range(8) for c in range(9)])]


def _viewed_frame(name, nodes, m=700, pid=21):
    return im.keep_facets_of_nodes(_frame(name, pid, m), nodes)


def _as_dict(fr):
    return dict(Tcw=fr.Tcw, K=fr.K, n_frame=fr.n_frame, obs_nodes=fr.obs_nodes, obs_bary=fr.obs_bary, obs_uv=fr.obs_uv, obs_invsig2=fr.obs_invsig2, xyz=fr.xyz)


def _oracle(oracle_mod, tc, fr, **kw):
    return oracle_mod.sft_solve(tc, fr.Tcw, fr.K, fr.n_frame, fr.obs_nodes, fr.obs_bary, fr.obs_uv, fr.obs_invsig2, fr.xyz, *_regs(), ldlt_mode=1, **kw)


# ================================================================ CPU part ================================================================

@pytest.mark.parametrize("name", ACCEPTED)
def test_host_packer_on_irregular_meshes(host_ctx, oracle_mod, name):
    """Host side of every accepted mesh: template constants bit-equal to the oracle's, the property the mesh exists for (rows 1 - 5 of the
    module's table: _assert_reaches), the packed counts equal to the oracle's dims at max_iters = 0 (as test_packer_counts_and_algorithmic_bytes
    does for C2), and -- seen on every flipped grid: corner nodes all of whose neighbour weights are zero, for which TemplateHost::finish_derived
    forms -(nbr_w / sw) with sw == 0 -- that a node with zero weight sum is always flagged boundary (it then has no curvature residual)."""
    from defslam_amd import sft
    m = _mesh(name)
    fr = _frame(name)
    tc = oracle_mod.template_build(m.xyz0, m.facets)
    host_ctx.template_build(m.xyz0, m.facets)
    tg = host_ctx.template_get()
    for k in ["boundary", "nbr_ptr", "nbr_idx", "edge_nodes", "edge_L0", "nbr_w", "k0"]:
        np.testing.assert_array_equal(tg[k], getattr(tc, k), err_msg=k)
    assert tg["median_L"] == tc.median_L
    host_ctx.batch_upload([sft.frame_from_synth(fr)], *_regs())
    _, counts = host_ctx.problem_info(0)
    _assert_reaches(name, tg, counts)
    r = oracle_mod.sft_solve(tc, fr.Tcw, fr.K, fr.n_frame, fr.obs_nodes, fr.obs_bary, fr.obs_uv, fr.obs_invsig2, fr.xyz, *_regs(), max_iters=0)
    D, nopt, nview, ncurv, nstr, _ = r.dims
    assert list(counts[:6]) == [fr.obs_nodes.shape[0], nopt, ncurv, nstr, nview, D]
    assert counts[7] == 8                                                # one problem: the latency launch shape
    deg = np.diff(tg["nbr_ptr"])
    sumw = np.array([tg["nbr_w"][a:b].sum() for a, b in zip(tg["nbr_ptr"][:-1], tg["nbr_ptr"][1:])])
    zero = (deg > 0) & (sumw == 0.0)
    assert tg["boundary"][zero].all(), np.flatnonzero(zero & ~tg["boundary"].astype(bool))
    if name.startswith("flip"):
        assert zero.any()                                                # the case exists on these meshes
    if name == "flip12x14_holes":
        inner = [v for q in m.hole_quads for v in (q % 13 + 14 * (q // 13), q % 13 + 1 + 14 * (q // 13), q % 13 + 14 * (q // 13 + 1), q % 13 + 1 + 14 * (q // 13 + 1))]
        assert tg["boundary"][inner].all()                               # the corners of a hole are boundary nodes inside the mesh


def test_degree_limit_and_band_limit_on_the_host(host_ctx):
    """Row 6: a hub of degree 14 packs (slot fields 1 .. 14 of SFT_REC all in use), one of degree 15 is refused with its message and the context
    packs the next problem as before.  The host-only packer has no band limit (that check sits behind it, on the device path): the sweep-ordered
    Delaunay mesh of 500 points packs with its half-bandwidth of 1043."""
    from defslam_amd import sft, synth
    m14 = im.disc(14, 3)
    host_ctx.template_build(m14.xyz0, m14.facets)
    host_ctx.batch_upload([sft.frame_from_synth(synth.make_frame(m14, 200, 9))], *_regs())
    ref = host_ctx.problem_info(0)
    assert im.properties(host_ctx.template_get())["max_star_degree"] == 14
    ctor, nm, pid = REFUSED_DEGREE
    m15 = ctor()
    host_ctx.template_build(m15.xyz0, m15.facets)                         # the template itself is accepted: the limit is the packer's
    assert im.properties(host_ctx.template_get())["max_star_degree"] == 15
    with pytest.raises(sft.DshError, match=r"dsh_sft_batch_upload: status 1: problem 0: node degree > 14 unsupported"):
        host_ctx.batch_upload([sft.frame_from_synth(synth.make_frame(m15, nm, pid))], *_regs())
    host_ctx.template_build(m14.xyz0, m14.facets)
    host_ctx.batch_upload([sft.frame_from_synth(synth.make_frame(m14, 200, 9))], *_regs())
    again = host_ctx.problem_info(0)
    assert again[0] == ref[0]
    np.testing.assert_array_equal(again[1], ref[1])
    ctor, nm, pid = REFUSED_BAND
    big = ctor()
    host_ctx.template_build(big.xyz0, big.facets)
    host_ctx.batch_upload([sft.frame_from_synth(synth.make_frame(big, nm, pid))], *_regs())
    assert int(host_ctx.problem_info(0)[1][6]) == 1043
    ctor, nm, pid = REFUSED_BAND_EDGE
    edge = ctor()
    host_ctx.template_build(edge.xyz0, edge.facets)
    host_ctx.batch_upload([sft.frame_from_synth(synth.make_frame(edge, nm, pid))], *_regs())
    assert int(host_ctx.problem_info(0)[1][6]) == 476                     # 476 + 32 + 7 = 515 > 512: refused on a device (GPU part), 473 is taken


def test_observation_whose_nodes_are_not_a_facet_is_refused(host_ctx):
    """The packer refuses an observation when a pair of its nodes has no block in the pattern of the normal equations (pairs that share
    a curvature star, like two ring-1 nodes of the disc, do have one)."""
    from defslam_amd import sft
    m = _mesh("disc14x4")
    host_ctx.template_build(m.xyz0, m.facets)
    f = sft.frame_from_synth(_frame("disc14x4"))
    f.obs_nodes = f.obs_nodes.copy()
    f.obs_nodes[5] = (0, 1, 36)                                           # hub, a node of ring 1 and one of ring 3
    with pytest.raises(sft.DshError, match="observation 5: its nodes are not joined by a mesh edge of the template"):
        host_ctx.batch_upload([f], *_regs())


@pytest.mark.parametrize("name", ACCEPTED + ["delaunay500"])
def test_c_oracle_matches_numpy_restatement_on_irregular_meshes(oracle_mod, name):
    """The two CPU oracles (C, and the independent NumPy restatement) on every construction, the refused band included: same trajectory,
    inliers and outlier set, vertices and pose to test_c_oracle_matches_numpy_restatement_live's 1e-11 -- the GPU comparisons below are
    exact in the trajectory, so the inputs must be ones on which the oracle itself is not in doubt."""
    from defslam_amd import synth
    from oracle import sft_oracle_np as onp
    if name == "delaunay500":
        m = REFUSED_BAND[0]()
        fr = synth.make_frame(m, REFUSED_BAND[1], REFUSED_BAND[2])
    else:
        m, fr = _mesh(name), _frame(name)
    tc, args = oracle_args(oracle_mod, m, fr)
    r = oracle_mod.sft_solve(*args)
    rn = onp.solve(*args)
    assert r.iters == rn["iters"] and r.ret == rn["ret"]
    np.testing.assert_array_equal(r.trace[:, [2, 6]], rn["trace"][:, [2, 6]])
    np.testing.assert_array_equal(r.outlier.astype(bool), rn["outlier"])
    np.testing.assert_allclose(r.xyz, rn["xyz"], atol=1e-11)
    np.testing.assert_allclose(r.pose7, rn["pose7"], atol=1e-11)


# ================================================================ GPU part ================================================================

@gpu
@pytest.mark.parametrize("name", ACCEPTED)
def test_normal_equations_match_oracle_on_irregular_meshes(lab_ctx, oracle_mod, name):
    """Residuals, Jacobians and the assembly of H and b in isolation (dsh_lab_sft_system), vertices perturbed by 2 mm so that curvature
    and stretch residuals are non-zero; sparsity pattern exact.  This is the test that localises a failure to the assembly: rows 1 - 5 of
    the module's table, each proven reached by _assert_reaches on the GPU context's own template constants (disc14x4 / disc12x6: the
    diagonal tail loop :769 and the second neighbour chunk :485; disc9x5: that chunk with one element; split10x10: the off-diagonal
    tail loop :875; every mesh: record slots > 6 and a non-periodic tmask / gather pattern).  Diagonal lists come first in sh_ptr, the
    off-diagonal ones behind them in row order: a mismatch in block (i, j) names the list."""
    from defslam_amd import sft
    m = _mesh(name)
    fr = _frame(name)
    rng = np.random.default_rng(MESHES[name][2])
    fr.xyz = fr.xyz + rng.normal(scale=0.002, size=fr.xyz.shape)
    tc, args = oracle_args(oracle_mod, m, fr)
    Ho, bo, chio = oracle_mod.sft_system(*args)
    lab_ctx.template_build(m.xyz0, m.facets)
    lab_ctx.batch_upload([sft.frame_from_synth(fr)], *_regs())
    _assert_reaches(name, lab_ctx.template_get(), lab_ctx.problem_info(0)[1])
    Hg, bg, chig = lab_ctx.debug_system(0, Ho.shape[0])
    assert chig == pytest.approx(chio, rel=1e-12)
    np.testing.assert_allclose(Hg, Ho, rtol=1e-9, atol=1e-11 * np.abs(Ho).max())
    np.testing.assert_allclose(bg, bo, rtol=1e-9, atol=1e-11 * np.abs(bo).max())
    np.testing.assert_array_equal(np.abs(Hg) > 0, np.abs(Ho) > 0)


@gpu
def test_normal_equations_with_observations_across_the_hub_star(lab_ctx, oracle_mod):
    """What test_observation_whose_nodes_are_not_a_facet_is_refused leaves open: an observation on three nodes that are no facet but share
    a curvature star (the hub and two ring-1 nodes that are not neighbours; three ring-1 nodes) is TAKEN -- its blocks exist in the pattern
    through the hub's star -- and then has to be assembled like any other: H, b and chi2 against the oracle, which takes any node triple."""
    from defslam_amd import sft
    m = _mesh("disc14x4")
    fr = _frame("disc14x4")
    fr.obs_nodes = fr.obs_nodes.copy()
    fr.obs_nodes[:6] = [(0, 1, 8), (0, 3, 12), (2, 7, 11), (1, 5, 9), (0, 2, 14), (4, 6, 13)]
    fr.xyz = fr.xyz + np.random.default_rng(8).normal(scale=0.002, size=fr.xyz.shape)
    tc, args = oracle_args(oracle_mod, m, fr)
    Ho, bo, chio = oracle_mod.sft_system(*args)
    lab_ctx.template_build(m.xyz0, m.facets)
    lab_ctx.batch_upload([sft.frame_from_synth(fr)], *_regs())
    Hg, bg, chig = lab_ctx.debug_system(0, Ho.shape[0])
    assert chig == pytest.approx(chio, rel=1e-12)
    np.testing.assert_allclose(Hg, Ho, rtol=1e-9, atol=1e-11 * np.abs(Ho).max())
    np.testing.assert_allclose(bg, bo, rtol=1e-9, atol=1e-11 * np.abs(bo).max())
    np.testing.assert_array_equal(np.abs(Hg) > 0, np.abs(Ho) > 0)


@gpu
@pytest.mark.parametrize("name", ["disc14x4", "flip12x14_holes"])
def test_template_set_gives_the_bits_of_template_build_on_irregular_meshes(gpu_ctx, name):
    """The other way a caller's mesh comes in: dsh_template_set with the constants dsh_template_get returns (variable-length neighbour rows,
    boundary nodes inside the mesh) solves to the same bits as dsh_template_build."""
    from test_sft_gpu import _solve_gpu
    from defslam_amd import sft
    m, fr = _mesh(name), _frame(name)
    f0, i0 = _solve_gpu(gpu_ctx, m.xyz0, m.facets, _as_dict(fr), _regs())
    t = gpu_ctx.template_get()
    gpu_ctx.template_set(m.xyz0, t["boundary"], t["nbr_ptr"], t["nbr_idx"], t["nbr_w"], t["k0"], t["edge_nodes"], t["edge_L0"], t["median_L"])
    f1 = sft.frame_from_synth(fr)
    i1 = sft.DefPoseOptimization(gpu_ctx, f1, *_regs())
    assert (i1, f1.iters, f1.trials, f1.status) == (i0, f0.iters, f0.trials, f0.status)
    for k in ("trace", "nodes_xyz", "pose7", "chi2_obs", "mvbOutlier", "mappoints"):
        np.testing.assert_array_equal(getattr(f1, k), getattr(f0, k), err_msg=k)


@gpu
@pytest.mark.parametrize("name", ACCEPTED)
def test_latency_solve_matches_oracle_on_irregular_meshes(gpu_ctx, oracle_mod, name):
    """One problem through DefPoseOptimization (the product library's latency mode: speculative lanes; the two-sided split with helpers for
    the two wide bands; the row-major band solver for delaunay200 (kd = 458) and for band473, whose kd = 473 is the widest band the library takes:
    473 + kNB + SFT_BORDER = 473 + 32 + 7 = 512 <= SFT_NT = 512; 476 is refused, test_refused_meshes_leave_the_gpu_context_usable)."""
    from test_sft_gpu import _solve_gpu
    m, fr = _mesh(name), _frame(name)
    r = _oracle(oracle_mod, oracle_mod.template_build(m.xyz0, m.facets), fr)
    f, inl = _solve_gpu(gpu_ctx, m.xyz0, m.facets, _as_dict(fr), _regs())
    assert f.half_bandwidth == MESHES[name][3]["kd"] and f.dim == r.dims[0] == 6 + 3 * m.n
    _compare(f, inl, r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret)
    assert f.trials == r.trials
    np.testing.assert_allclose(f.Tcw, r.Tcw, atol=2e-7)


@gpu
@pytest.mark.parametrize("name,view,nodes", _partial_views(), ids=[f"{a}-{b}" for a, b, _ in _partial_views()])
def test_partial_views_of_irregular_meshes(gpu_ctx, oracle_mod, name, view, nodes):
    """Part of the mesh viewed: the degree-14 hub (the split nodes) active through the 1-ring but not viewed -- its long lists are there, its
    observation list is empty -- and not active at all (the lists of its neighbours lose the entries of the fixed nodes); corners of the
    flipped grids.  Fixed vertices come back bit-identical."""
    from test_sft_gpu import _solve_gpu
    m = _mesh(name)
    fr = _viewed_frame(name, nodes)
    assert fr.obs_nodes.shape[0] >= 100
    tc = oracle_mod.template_build(m.xyz0, m.facets)
    r = _oracle(oracle_mod, tc, fr)
    f, inl = _solve_gpu(gpu_ctx, m.xyz0, m.facets, _as_dict(fr), _regs())
    viewed = np.zeros(m.n, bool)
    viewed[np.unique(fr.obs_nodes)] = True
    active = viewed.copy()
    for i in np.flatnonzero(viewed):
        active[tc.nbr_idx[tc.nbr_ptr[i]:tc.nbr_ptr[i + 1]]] = True
    special = {"disc14x4": [0], "split10x10": list(getattr(m, "new_nodes", ()))}.get(name, [])
    if view in ("half_without_hub", "upper_half"):
        assert all(active[s] and not viewed[s] for s in special)
    if view in ("rim", "top_rows"):
        assert not any(active[s] for s in special)
    pr = im.properties(tc, active)
    if view == "half_without_hub":
        assert pr["diag"][0] == im.DIAG_PREFETCH + 1                     # the hub's list without the stars of the four fixed ring-1 nodes: 25, one in the tail loop
    assert f.dim == r.dims[0] == 6 + 3 * int(active.sum()) < 6 + 3 * m.n and f.half_bandwidth == pr["kd"]
    _compare(f, inl, r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret)
    np.testing.assert_array_equal(f.nodes_xyz[~active], fr.xyz[~active])


POOL = 16


@pytest.fixture(scope="module")
def irregular_pool(oracle_mod):
    """Per narrow mesh: POOL distinct frames (match counts vary, every fourth a partial view) and the oracle's solution of each, computed once
    for both ways the throughput shape ends a step."""
    from concurrent.futures import ThreadPoolExecutor
    views = {n: v for n, w, v in _partial_views() if w in ("half_without_hub", "upper_half", "corner")}
    out = {}
    for name in NARROW:
        m = _mesh(name)
        syn = []
        for p in range(POOL):
            fr = _frame(name, 300 + p, 300 + 20 * (p % 4))
            if p % 4 == 3:
                fr = im.keep_facets_of_nodes(_frame(name, 300 + p, 700), views[name])
            syn.append(fr)
        tc = oracle_mod.template_build(m.xyz0, m.facets)
        with ThreadPoolExecutor(8) as ex:   # (the C oracle keeps no mutable global state; the calls release the GIL)
            ref = list(ex.map(lambda fr: _oracle(oracle_mod, tc, fr), syn))
        out[name] = (m, syn, ref)
    return out


@pytest.fixture(params=[0, -1], ids=["rounds_to_the_end", "product_default_tail"])
def rounds_ctx(request, lab_ctx):
    """As test_sft_gpu.py's: tail = 0, the rounds of phase kernels run to the end of every problem; tail = -1, the product default (the tail kernel)."""
    lab_ctx.set_option("tail", request.param)
    yield lab_ctx
    lab_ctx.set_option("tail", -1)


@gpu
@pytest.mark.parametrize("name", NARROW)
def test_throughput_shape_on_irregular_meshes(rounds_ctx, irregular_pool, name):
    """A batch of 2 x CUs problems (four times the CUs / 2 + 1 from which the library takes the throughput shape: LIN / FACTOR / TRIAL rounds with
    one wavefront per factorisation, then the tail kernel or rounds to the end) on one irregular template: the persistent linearisation, the
    one-wavefront factor kernel (kd <= 128) and the tail kernel all see the hub's 29-entry list (disc14x4), the 7-entry off-diagonal list
    (split10x10) and the ragged tile mask (flip10x10).  POOL distinct frames, each at B / POOL scattered positions: every distinct frame
    against the oracle, every copy bit-identical to the first, two runs bit-identical."""
    from defslam_amd import _lib, sft
    m, syn, ref = irregular_pool[name]
    B = 2 * _lib.device_cus(0)
    order = np.random.default_rng(5).permutation(B) % POOL
    rounds_ctx.template_build(m.xyz0, m.facets)
    frames = [sft.frame_from_synth(syn[int(q)]) for q in order]
    rounds_ctx.batch_upload(frames, *_regs(), 1, 50)
    for b in range(POOL):
        counts = rounds_ctx.problem_info(b)[1]
        assert int(counts[7]) == 1 and int(counts[6]) <= 128, (b, counts)   # rounds of phase kernels, one-wavefront solver
    snaps = []
    for _ in range(2):
        rounds_ctx.batch_run()
        inl = rounds_ctx.batch_download()
        snaps.append([(int(i), f.iters, f.trials, f.status, f.trace.copy(), f.nodes_xyz.copy(), f.pose7.copy(), f.chi2_obs.copy(), f.mvbOutlier.copy())
                      for i, f in zip(inl, frames)])
    first = {}
    for b, q in enumerate(order):
        a0, a1 = snaps[0][b], snaps[1][b]
        c = snaps[0][first.setdefault(int(q), b)]
        for other in (a1, c):
            assert a0[:4] == other[:4], (b, int(q))
            for u, v in zip(a0[4:], other[4:]):
                np.testing.assert_array_equal(u, v, err_msg=f"position {b}, pool frame {int(q)}")
    assert len(first) == POOL
    for q, b in first.items():
        r = ref[q]
        _compare(frames[b], snaps[1][b][0], r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret)
        assert frames[b].trials == r.trials and frames[b].dim == r.dims[0]


@gpu
@pytest.mark.parametrize("name", NARROW + ["flip6x41"])
def test_batch_equals_single_on_irregular_meshes(gpu_ctx, name):
    """test_batch_equals_single_and_is_reproducible on irregular templates: nine problems in one launch give the bits of one-at-a-time solves,
    run after run."""
    from defslam_amd import sft
    m = _mesh(name)
    gpu_ctx.template_build(m.xyz0, m.facets)
    frames = [sft.frame_from_synth(_frame(name, 40 + p, 200 + 10 * p)) for p in range(9)]
    inl = sft.DefPoseOptimizationBatch(gpu_ctx, frames, *_regs())
    xyz_a = [f.nodes_xyz.copy() for f in frames]
    gpu_ctx.batch_run()
    assert inl == gpu_ctx.batch_download()
    for f, xa in zip(frames, xyz_a):
        np.testing.assert_array_equal(f.nodes_xyz, xa)
    for p in [0, 4, 8]:
        f1 = sft.frame_from_synth(_frame(name, 40 + p, 200 + 10 * p))
        i1 = sft.DefPoseOptimization(gpu_ctx, f1, *_regs())
        assert i1 == inl[p]
        np.testing.assert_array_equal(f1.nodes_xyz, xyz_a[p])
        np.testing.assert_array_equal(f1.pose7, frames[p].pose7)


@gpu
@pytest.mark.parametrize("name", ["flip8x30", "flip6x41"])
def test_wide_band_solvers_on_irregular_meshes(lab_ctx, oracle_mod, name):
    """The irregular counterparts of W12 / W16 (half-bandwidths 188 and 254) in latency mode with the lab options of the wide-band tests: the
    two-sided split with 0 and 3 helper workgroups per part (four lanes) and with 2 (two lanes) -- the same bits, as
    test_helper_workgroups_of_the_two_sided_factorisation_do_not_change_a_bit asserts; the undivided wide-tile solver -- another elimination
    order, so as test_two_sided_factorisation_follows_the_undivided_one_and_the_oracle: the same trajectory, numbers to 1e-9; both against the
    oracle through _compare."""
    from defslam_amd import sft
    m, fr = _mesh(name), _frame(name)
    lab_ctx.template_build(m.xyz0, m.facets)
    res = {}
    try:
        for key, split, K, nh in (("s0", 1, 4, 0), ("s3", 1, 4, 3), ("s2", 1, 2, 2), ("u", 0, 4, 0)):
            lab_ctx.set_option("split", split)
            lab_ctx.set_option("speculate", K)
            lab_ctx.set_option("helpers", nh)
            f = sft.frame_from_synth(fr)
            lab_ctx.batch_upload([f], *_regs(), 1, 50)
            info = lab_ctx.solver_info(0)
            assert info["split"] == split and info["lanes"] == K and info["tile_mode"] == 2, (key, info)
            lab_ctx.batch_run()
            res[key] = (f, lab_ctx.batch_download()[0])
    finally:
        lab_ctx.set_option("split", 2)
        lab_ctx.set_option("speculate", 0)
        lab_ctx.set_option("helpers", -1)
    a, ia = res["s0"]
    assert 128 < a.half_bandwidth <= 256
    for key in ("s3", "s2"):
        b, ib = res[key]
        assert (ia, a.iters, a.trials, a.status) == (ib, b.iters, b.trials, b.status), key
        for k in ("trace", "nodes_xyz", "pose7", "chi2_obs", "mvbOutlier"):
            np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=f"{key}: {k}")
    u, iu = res["u"]
    assert (ia, a.iters, a.trials) == (iu, u.iters, u.trials)
    np.testing.assert_allclose(a.trace[:, :6], u.trace[:, :6], rtol=1e-7)
    np.testing.assert_array_equal(a.trace[:, 6:], u.trace[:, 6:])
    np.testing.assert_allclose(a.nodes_xyz, u.nodes_xyz, rtol=0, atol=1e-9 * np.abs(u.nodes_xyz).max())
    np.testing.assert_allclose(a.pose7, u.pose7, rtol=0, atol=1e-9)
    r = _oracle(oracle_mod, oracle_mod.template_build(m.xyz0, m.facets), fr)
    for f, i in (res["s0"], res["u"]):
        _compare(f, i, r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret)


@gpu
@pytest.mark.parametrize("name", ["disc14x4", "split10x10"])
def test_speculative_damping_trials_are_bit_identical_on_irregular_meshes(lab_ctx, name):
    """test_speculative_damping_trials_are_bit_identical's comparison (1 .. 4 lanes, several problems per launch, every result array) where the
    lanes' linearisations walk the long lists of the hub and of the split edge."""
    from defslam_amd import sft
    m = _mesh(name)
    runs = {}
    lab_ctx.set_option("split", 0)
    try:
        lab_ctx.template_build(m.xyz0, m.facets)
        for K in (1, 2, 3, 4):
            lab_ctx.set_option("speculate", K)
            frames = [sft.frame_from_synth(_frame(name, 60 + p)) for p in range(4)]
            inl = sft.DefPoseOptimizationBatch(lab_ctx, frames, *_regs(), max_iters=10)
            runs[K] = (frames, inl)
    finally:
        lab_ctx.set_option("speculate", 0)
        lab_ctx.set_option("split", 2)
    f1, i1 = runs[1]
    assert sum(f.trials for f in f1) > sum(f.iters for f in f1)           # the cases do reject trials
    for K in (2, 3, 4):
        fk, ik = runs[K]
        assert ik == i1
        for a, b in zip(fk, f1):
            assert (a.iters, a.trials, a.status) == (b.iters, b.trials, b.status)
            for k in ("trace", "nodes_xyz", "pose7", "chi2_obs", "mvbOutlier", "mappoints"):
                np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=f"{K} lanes: {k}")
            assert a.rep_error_f64 == b.rep_error_f64


@gpu
def test_warm_started_sequence_on_the_disc(gpu_ctx, oracle_mod):
    """Ten frames of a smooth sequence on disc12x6, each tracked from the previous result through the one-shot call (float32 pose round trip):
    the graph of the irregular template is built once and reused from the cache; every frame against the oracle from the same previous state."""
    from defslam_amd import sft, synth
    m = _mesh("disc12x6")
    tc = oracle_mod.template_build(m.xyz0, m.facets)
    gpu_ctx.template_build(m.xyz0, m.facets)
    T, x = np.eye(4, dtype=np.float32), m.xyz0.copy()
    for k in range(10):
        fr = synth.make_sequence_frame(m, 400, k, 100, 3, init_xyz=x, init_Tcw=T)
        f = sft.frame_from_synth(fr)
        inl = gpu_ctx.prepare_solve(f, *_regs(), 1, 50)()
        r = _oracle(oracle_mod, tc, fr)
        _compare(f, inl, r.xyz, r.pose7, r.trace, r.outlier, r.rep_error, r.ret)
        np.testing.assert_allclose(f.Tcw, r.Tcw, atol=2e-7)
        assert f.dim == 6 + 3 * m.n and inl > 0.85 * 400
        T, x = f.Tcw.copy(), f.nodes_xyz.copy()


def _embedding_points(m, rng, extra):
    F = m.facets.shape[0]
    fac = rng.integers(0, F, size=300)
    bary = rng.dirichlet((1, 1, 1), size=300)
    pts = (bary[:, :, None] * m.xyz0[m.facets[fac]]).sum(1)
    pts[::7] += rng.normal(scale=0.01, size=pts[::7].shape)
    pts[::50] += 5.0
    return np.vstack([pts, extra]).astype(np.float32)


@gpu
@pytest.mark.parametrize("name", ["disc14x4", "flip12x14_holes"])
def test_device_embedding_on_irregular_meshes(gpu_ctx, oracle_mod, name):
    """dsh_template_embed_device against the host embedding and tmpl_oracle_embed, bit for bit: the hub itself and points near it (fourteen
    candidate facets around the closest node), every node of the disc, points over the holes of the holed grid (closest node found, no facet
    contains the point: not embedded) and far away."""
    m = _mesh(name)
    rng = np.random.default_rng(11)
    if name == "disc14x4":
        near = m.xyz0[0] + np.c_[rng.normal(scale=0.01, size=(40, 2)), np.zeros(40)]
        extra = np.vstack([m.xyz0, near])
    else:
        quads = [(q % 13, q // 13) for q in m.hole_quads]
        extra = np.array([m.xyz0[[c + 14 * r, c + 1 + 14 * r, c + 14 * (r + 1), c + 1 + 14 * (r + 1)]].mean(0) for c, r in quads])
    pts = _embedding_points(m, rng, extra)
    P = pts.shape[0]
    tc = oracle_mod.template_build(m.xyz0, m.facets)
    gpu_ctx.template_build(m.xyz0, m.facets)
    fid_h, nodes_h, b_h = gpu_ctx.template_embed(pts)
    fid_d, nodes_d, b_d = gpu_ctx.template_embed_device(pts)
    ofid, ob = np.zeros(P, np.int32), np.zeros((P, 3), np.float32)
    xyz0 = np.ascontiguousarray(m.xyz0)
    oracle_mod.lib().tmpl_oracle_embed(tc.n, xyz0.ctypes.data_as(C.POINTER(C.c_double)), m.facets.shape[0], tc.facets.ctypes.data_as(C.POINTER(C.c_int32)), P,
                                       pts.ctypes.data_as(C.POINTER(C.c_float)), ofid.ctypes.data_as(C.POINTER(C.c_int32)), ob.ctypes.data_as(C.POINTER(C.c_float)))
    for fid, nodes, b in ((fid_h, nodes_h, b_h), (fid_d, nodes_d, b_d)):
        np.testing.assert_array_equal(fid, ofid)
        np.testing.assert_array_equal(b, ob)
        ok = fid >= 0
        np.testing.assert_array_equal(nodes[ok], tc.facets[fid[ok]])
        assert (nodes[~ok] == -1).all()
    assert (ofid[:300:50] == -1).all() and (ofid >= 0).sum() > 250
    if name == "disc14x4":
        assert ofid[300] >= 0 and 0 in tc.facets[ofid[300]]                # the hub is embedded in one of its fourteen facets
        assert (ofid[300 + m.n:] >= 0).all()
    else:
        assert (ofid[300:] == -1).all()                                   # over a hole


def _bits_of_a_solve(ctx, m, fr):
    from defslam_amd import sft
    ctx.template_build(m.xyz0, m.facets)
    f = sft.frame_from_synth(fr)
    inl = sft.DefPoseOptimization(ctx, f, *_regs())
    return inl, f


@gpu
def test_refused_meshes_leave_the_gpu_context_usable(gpu_ctx):
    """Row 6 and the band limit on the GPU context.  Both refusals are dsh_sft_batch_upload's (read from the code: the degree check is
    build_graph's, the check `max_kd + kNB + SFT_BORDER <= SFT_NT` follows the packing and precedes every allocation, copy and launch), both are
    DSH_ERR_ARG with their messages; band_limit_grid(1) (kd 473, accepted and solved: test_latency_solve_matches_oracle_on_irregular_meshes)
    and band_limit_grid(2) (kd 476) are the two half-bandwidths on either side of that limit, delaunay500 (kd 1043) lies far beyond it.  After each refusal a grid problem solved on the same context has the bits
    of a fresh context's solve."""
    from defslam_amd import sft, synth
    tmpl, fr = synth.make_problem("smoke", 4)
    fresh = sft.Context(0)
    try:
        i0, f0 = _bits_of_a_solve(fresh, tmpl, fr)
    finally:
        fresh.close()
    band = "half-bandwidth too large for the LDS panel / workgroup"
    for (ctor, nm, pid), msg in ((REFUSED_DEGREE, "problem 0: node degree > 14 unsupported"), (REFUSED_BAND_EDGE, band), (REFUSED_BAND, band)):
        bad = ctor()
        gpu_ctx.template_build(bad.xyz0, bad.facets)
        with pytest.raises(sft.DshError, match=rf"dsh_sft_batch_upload: status 1: {msg}"):
            gpu_ctx.batch_upload([sft.frame_from_synth(synth.make_frame(bad, nm, pid))], *_regs())
        i1, f1 = _bits_of_a_solve(gpu_ctx, tmpl, fr)
        assert (i1, f1.iters, f1.trials, f1.status) == (i0, f0.iters, f0.trials, f0.status)
        for k in ("trace", "nodes_xyz", "pose7", "chi2_obs", "mvbOutlier", "mappoints"):
            np.testing.assert_array_equal(getattr(f1, k), getattr(f0, k), err_msg=k)
