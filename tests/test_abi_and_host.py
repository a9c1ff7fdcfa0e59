"""CPU tests: the C-ABI library loads, exports every symbol the header declares, and the host-side
logic (template constants, embedding, problem packing) matches the oracle.  No GPU compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def test_library_exports_every_declared_symbol():
    from defslam_amd import _lib
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "defslam_hip.h")).read()
    declared = sorted(set(re.findall(r"\b(dsh_[a-z0-9_]+)\s*\(", header)))
    assert declared, "no prototypes found in the header"
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/defslam_hip.h but not exported"
    assert sorted(_lib.EXPORTED_SYMBOLS) == declared


def _dynamic_symbols(path):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if " T " in line)


def test_product_library_exports_exactly_the_public_header_and_the_lab_library_adds_the_debug_header():
    """The product ABI carries no lab equipment: libdefslam_hip.so exports the prototypes of include/defslam_hip.h and nothing
    else (no timers, no test hooks, no internal launchers), and does not read the environment; the measurement / debugging
    entry points of include/defslam_hip_debug.h exist only in libdefslam_hip_lab.so (the same sources with -DDSH_LAB)."""
    import subprocess
    from defslam_amd import _lib
    header = open(os.path.join(ROOT, "include", "defslam_hip.h")).read()
    debug_header = open(os.path.join(ROOT, "include", "defslam_hip_debug.h")).read()
    declared = sorted(set(re.findall(r"\b(dsh_[a-z0-9_]+)\s*\(", header)))
    lab_declared = sorted(set(re.findall(r"\b(dsh_lab_[a-z0-9_]+)\s*\(", debug_header)))
    assert lab_declared and sorted(_lib.LAB_SYMBOLS) == lab_declared
    assert not re.search(r"timed|phase_ms|debug_system|dsh_lab", header)
    assert _dynamic_symbols(_lib.LIB_PATH) == declared
    assert _dynamic_symbols(_lib.LAB_LIB_PATH) == sorted(declared + lab_declared)
    undefined = subprocess.run(["nm", "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in undefined, "the product library must not read environment switches"
    L = _lib.load_lab()
    for name in lab_declared:
        assert hasattr(L, name)


def test_template_set_refuses_malformed_index_arrays(host_ctx):
    """dsh_template_set turns the caller's CSR / edge arrays into indices of the packer: out-of-range or non-monotone
    input is DSH_ERR_ARG, not a heap overrun (nothing aborts across the ABI)."""
    from defslam_amd import sft, synth
    tmpl = synth.make_grid_template(6, 7)
    host_ctx.template_build(tmpl.xyz0, tmpl.facets)
    t = host_ctx.template_get()

    def attempt(**over):
        a = dict(t)
        a.update(over)
        host_ctx.template_set(tmpl.xyz0, a["boundary"], a["nbr_ptr"], a["nbr_idx"], a["nbr_w"], a["k0"], a["edge_nodes"], a["edge_L0"], a["median_L"])

    attempt()   # the constants the library derived itself are accepted
    bad_ptr = t["nbr_ptr"].copy(); bad_ptr[3] = bad_ptr[2] - 1
    bad_ptr0 = t["nbr_ptr"].copy(); bad_ptr0[0] = 1
    bad_col = t["nbr_idx"].copy(); bad_col[5] = tmpl.n
    neg_col = t["nbr_idx"].copy(); neg_col[0] = -1
    bad_edge = t["edge_nodes"].copy(); bad_edge[4, 1] = 10_000
    bad_len = t["edge_L0"].copy(); bad_len[2] = 0.0
    for over in (dict(nbr_ptr=bad_ptr), dict(nbr_ptr=bad_ptr0), dict(nbr_idx=bad_col), dict(nbr_idx=neg_col), dict(edge_nodes=bad_edge),
                 dict(edge_L0=bad_len), dict(median_L=0.0), dict(median_L=float("nan"))):
        with pytest.raises(sft.DshError, match="dsh_template_set"):
            attempt(**over)
    attempt()


def test_header_is_plain_c_and_a_c_client_links(tmp_path):
    """The boundary is a C ABI: include/defslam_hip.h compiles as C99 and as C++11, and a C program linked against the
    shared library creates and destroys a host-only context (what a cgo / JNI / N-API stub would do first)."""
    import subprocess
    from defslam_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "client.c"
    src.write_text('#include "include/defslam_hip.h"\n#include <stdio.h>\n'
                   'int main(void) { dsh_ctx* c = 0; if (dsh_create(&c, -1) != DSH_OK) return 1;\n'
                   '  if (dsh_synchronize(c) == DSH_OK) return 2;   /* host-only context: GPU entry points refuse */\n'
                   '  printf("%s\\n", dsh_last_error(c)); return dsh_destroy(c); }\n')
    lib = _lib.LIB_PATH
    exe = tmp_path / "client"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", root, str(src), "-o", str(exe), lib,
                    f"-Wl,-rpath,{os.path.dirname(lib)}"], check=True)
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I", root, str(src)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_gpu_entry_points_fail_loudly_without_a_device(host_ctx):
    from defslam_amd import sft, synth
    tmpl, fr = synth.make_problem("smoke")
    host_ctx.template_build(tmpl.xyz0, tmpl.facets)
    f = sft.frame_from_synth(fr)
    host_ctx.batch_upload([f], synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    with pytest.raises(sft.DshError, match="no GPU|host-only"):
        host_ctx.batch_run()


def test_mapping_and_registration_entry_points_fail_loudly_without_a_device(host_ctx):
    """No CPU fallback anywhere: the one-shot calls refuse a host-only context too (and bad arguments are a status, not a crash)."""
    from defslam_amd import nrsfm, register, sft, synth
    sc = synth.make_register_scene(40, seed=1)
    for call in (lambda: register.scaleMinMedian(host_ctx, sc["surface"], sc["map"], sc["u"]),
                 lambda: register.OptimizeHorn(host_ctx, sc["surface"], sc["map"], [0, 0, 0, 1, 0, 0, 0, 1.0], 0.01),
                 lambda: register.registerSurfaces(host_ctx, sc["surface"], sc["map"], sc["u"], sc["Twc"], 0.05),
                 lambda: nrsfm.bbs_eval(host_ctx, nrsfm.Bbs(0, 1, 5, 0, 1, 5, 1), np.zeros((25, 1)), np.array([0.5]), np.array([0.5]))):
        with pytest.raises(sft.DshError, match="no GPU|host-only|NO_DEVICE|status"):
            call()
    tmpl = synth.make_grid_template(5, 5)
    host_ctx.template_build(tmpl.xyz0, tmpl.facets)
    with pytest.raises(sft.DshError, match="host-only"):
        host_ctx.template_embed_device(np.zeros((3, 3), np.float32))
    # fewer than 15 pairs is the reference's early `return false`, answered without touching a device
    few = register.registerSurfaces(host_ctx, sc["surface"][:10], sc["map"][:10], sc["u"], sc["Twc"], 0.05)
    assert not few["registered"]
    with pytest.raises(sft.DshError):
        register.scaleMinMedian(host_ctx, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), sc["u"])


def test_bad_arguments_return_status_not_abort(host_ctx):
    from defslam_amd import sft, synth
    tmpl, fr = synth.make_problem("smoke")
    host_ctx.template_build(tmpl.xyz0, tmpl.facets)
    f = sft.frame_from_synth(fr)
    f.obs_nodes = f.obs_nodes.copy()
    f.obs_nodes[0, 0] = 10_000
    with pytest.raises(sft.DshError, match="out of range"):
        host_ctx.batch_upload([f])
    bad_facets = tmpl.facets.copy()
    bad_facets[0, 0] = -1
    with pytest.raises(sft.DshError):
        host_ctx.template_build(tmpl.xyz0, bad_facets)


@pytest.mark.parametrize("shape", [(10, 10), (25, 20), (7, 13)])
def test_template_constants_match_oracle(host_ctx, oracle_mod, shape):
    from defslam_amd import synth
    tmpl = synth.make_grid_template(*shape)
    tc = oracle_mod.template_build(tmpl.xyz0, tmpl.facets)
    host_ctx.template_build(tmpl.xyz0, tmpl.facets)
    tg = host_ctx.template_get()
    # integer / index work: bit exact
    for k in ["boundary", "nbr_ptr", "nbr_idx", "edge_nodes"]:
        np.testing.assert_array_equal(tg[k], getattr(tc, k))
    # floating point: same formulas in the same order -> identical doubles
    np.testing.assert_array_equal(tg["edge_L0"], tc.edge_L0)
    np.testing.assert_array_equal(tg["nbr_w"], tc.nbr_w)
    np.testing.assert_array_equal(tg["k0"], tc.k0)
    assert tg["median_L"] == tc.median_L
    rows, cols = shape
    assert tc.E == (rows - 1) * cols + (cols - 1) * rows + (rows - 1) * (cols - 1)
    assert int(tc.boundary.sum()) == 2 * (rows + cols) - 4


def test_irregular_mesh_constants(host_ctx, oracle_mod):
    """A fan + strip mesh: varying degrees, shuffled facet orientation."""
    rng = np.random.default_rng(5)
    xy = rng.uniform(-1, 1, size=(40, 2))
    from scipy.spatial import Delaunay
    tri = Delaunay(xy)
    xyz = np.c_[xy, 1 + 0.1 * rng.normal(size=40)]
    fac = tri.simplices.astype(np.int32)
    tc = oracle_mod.template_build(xyz, fac)
    host_ctx.template_build(xyz, fac)
    tg = host_ctx.template_get()
    for k in ["boundary", "nbr_ptr", "nbr_idx", "edge_nodes"]:
        np.testing.assert_array_equal(tg[k], getattr(tc, k))
    np.testing.assert_array_equal(tg["nbr_w"], tc.nbr_w)
    np.testing.assert_array_equal(tg["k0"], tc.k0)


def test_embedding_matches_oracle_bit_exact(host_ctx, oracle_mod):
    from defslam_amd import synth
    tmpl = synth.make_grid_template(10, 10)
    tc = oracle_mod.template_build(tmpl.xyz0, tmpl.facets)
    host_ctx.template_build(tmpl.xyz0, tmpl.facets)
    rng = np.random.default_rng(7)
    F = tmpl.facets.shape[0]
    fac = rng.integers(0, F, size=500)
    bary = rng.dirichlet((1, 1, 1), size=500)
    pts = (bary[:, :, None] * tmpl.xyz0[tmpl.facets[fac]]).sum(1)
    pts[::7] += rng.normal(scale=0.01, size=pts[::7].shape)       # off-surface points
    pts[::50] += 5.0                                               # far away: not embedded
    pts = pts.astype(np.float32)
    fid, nodes, b = host_ctx.template_embed(pts)
    L = oracle_mod.lib()
    ofid = np.zeros(500, np.int32)
    ob = np.zeros((500, 3), np.float32)
    xyz0 = np.ascontiguousarray(tmpl.xyz0)
    L.tmpl_oracle_embed(tc.n, xyz0.ctypes.data_as(C.POINTER(C.c_double)), F, tc.facets.ctypes.data_as(C.POINTER(C.c_int32)), 500,
                        pts.ctypes.data_as(C.POINTER(C.c_float)), ofid.ctypes.data_as(C.POINTER(C.c_int32)), ob.ctypes.data_as(C.POINTER(C.c_float)))
    np.testing.assert_array_equal(fid, ofid)            # bit-exact triangle indexing
    np.testing.assert_array_equal(b, ob)                # float32 barycentrics, same operation order
    ok = fid >= 0
    np.testing.assert_array_equal(nodes[ok], tc.facets[fid[ok]])
    assert (fid[::50] == -1).all() and ok.sum() > 400
    # reconstruct: sum b_k v_k is within the reference's 0.1 squared-distance gate
    rec = (b[ok][:, :, None] * tmpl.xyz0[nodes[ok]]).sum(1)
    assert ((rec - pts[ok]) ** 2).sum(1).max() <= 0.1


def test_packer_counts_and_algorithmic_bytes(host_ctx, oracle_mod):
    from defslam_amd import sft, synth
    tmpl, fr = synth.make_problem("C2")
    host_ctx.template_build(tmpl.xyz0, tmpl.facets)
    host_ctx.batch_upload([sft.frame_from_synth(fr)], synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP)
    nbytes, counts = host_ctx.problem_info(0)
    tc = oracle_mod.template_build(tmpl.xyz0, tmpl.facets)
    r = oracle_mod.sft_solve(tc, fr.Tcw, fr.K, fr.n_frame, fr.obs_nodes, fr.obs_bary, fr.obs_uv, fr.obs_invsig2, fr.xyz,
                             synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP, max_iters=0)
    D, nopt, nview, ncurv, nstr, _ = r.dims
    assert list(counts[:6]) == [1000, nopt, ncurv, nstr, nview, D]
    assert 0 < counts[6] <= 128 and counts[7] == 8     # half-bandwidth of the node block (tile mode), latency launch shape for one problem
    M, n, Cc, E, V = 1000, 500, int(ncurv), int(nstr), int(nview)
    expect = (60 * M + 24 * n + 88 + 92 * Cc + 16 * E + 28 * V) + 8 * (30 * M + 21 * Cc + 6 * E + 9 * V) + 8 * (2 * M + Cc + E + 3 * V) + 8 * M
    assert nbytes == expect
    assert 1.1e6 < nbytes < 1.25e6    # ~1.17 MB per assembly pass at C2


def test_graph_cache_survives_more_active_sets_than_it_holds(host_ctx):
    """The structure of the normal equations is cached per active set (64 entries).  A sequence whose view changes every frame, and a
    batch with more distinct active sets than the cache holds, must keep packing correctly: the eviction may only drop graphs the
    upload in progress does not use (regression: it used to clear the problems already packed by the same upload)."""
    from defslam_amd import sft, synth
    tmpl = synth.make_grid_template(14, 14)
    host_ctx.template_build(tmpl.xyz0, tmpl.facets)
    base = synth.make_frame(tmpl, 900, 3)

    def windowed(r0, c0):
        keep = [c + 14 * r for r in range(r0, r0 + 6) for c in range(c0, c0 + 6)]
        sel = np.all(np.isin(base.obs_nodes, keep), axis=1)
        f = sft.frame_from_synth(base)
        f.obs_nodes, f.obs_bary, f.obs_uv, f.obs_invsig2 = base.obs_nodes[sel], base.obs_bary[sel], base.obs_uv[sel], base.obs_invsig2[sel]
        return f

    views = [(r, c) for r in range(9) for c in range(9)]          # 81 different 6x6 windows = 81 active sets
    ref = {}
    for v in views:                                                # one frame at a time: the 65th evicts
        host_ctx.batch_upload([windowed(*v)], synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP, 1, 10)
        ref[v] = host_ctx.problem_info(0)
        assert ref[v][1][0] > 0 and 0 < ref[v][1][1] <= 64         # some observations, at most the 8x8 nodes of window + ring
    # all of them in ONE upload (more active sets than the cache holds), in a different order
    order = views[::-1]
    host_ctx.batch_upload([windowed(*v) for v in order], synth.REG_LAP, synth.REG_INEX, synth.REG_TEMP, 1, 10)
    for b, v in enumerate(order):
        nb, counts = host_ctx.problem_info(b)
        assert nb == ref[v][0]
        np.testing.assert_array_equal(counts[:7], ref[v][1][:7])
        assert counts[8] == ref[v][1][8]


DSH_OK, ARG, STATE, NODEV = 0, 1, 3, 4   # DSH_ERR_ARG, DSH_ERR_STATE, DSH_ERR_NO_DEVICE
_HOST_ONLY_MESSAGE_EMPTY = ("dsh_synchronize",)   # returns DSH_ERR_NO_DEVICE without a message


def _host_only_rows(keep):
    """One row per product entry point that takes a context, store or communicator: (name, well-formed call, its status, call with one
    malformed argument, its status).  Arguments are raw ctypes values; `None` is a null pointer, the context goes in as "ctx"."""
    from defslam_amd import _lib

    def buf(nbytes=4096, fill=None):
        b = (C.c_uint8 * nbytes)()
        if fill is not None:
            C.memmove(b, fill.ctypes.data, fill.nbytes)
        keep.append(b)
        return C.cast(b, C.c_void_p)

    def ref(s):
        keep.append(s)
        return C.cast(C.byref(s), C.c_void_p)

    I, L64, D, F = C.c_int, C.c_int64, C.c_double, C.c_float
    eye = buf(fill=np.eye(4, dtype=np.float32))
    one = buf(fill=np.ones(1, np.float32))
    bbs = ref(_lib.BbsC(0.0, 1.0, 5, 0.0, 1.0, 5, 1))
    bad_bbs = ref(_lib.BbsC(0.0, 1.0, 3, 0.0, 1.0, 5, 1))   # fewer than 4 control points

    def frame(**over):
        f = _lib.SftFrameC(Tcw=C.cast(eye, _lib.c_float_p), n_frame=1, M=1, reg_lap=1.0, reg_inex=1.0, reg_temp=1.0, neighbour_layers=1, max_iters=50,
                           obs_nodes=C.cast(buf(fill=np.array([0, 1, 2], np.int32)), _lib.c_i32_p), obs_bary=C.cast(buf(fill=np.full(3, 1 / 3)), _lib.c_double_p),
                           obs_uv=C.cast(buf(fill=np.array([320.0, 240.0])), _lib.c_double_p), obs_invsig2=C.cast(buf(fill=np.ones(1)), _lib.c_double_p),
                           xyz=C.cast(buf(fill=np.array([0, 0, 1, 1, 0, 1, 0, 1, 1], np.float64)), _lib.c_double_p))
        f.K[:] = (500.0, 500.0, 320.0, 240.0)
        for k, v in over.items():
            setattr(f, k, v)
        return ref(f)

    def track_frame(**over):
        f = _lib.TrackFrameC(Tcw=C.cast(eye, _lib.c_float_p), grid_cols=64, grid_rows=48, levels=1, scale_factors=C.cast(one, _lib.c_float_p),
                             log_scale_factor=0.18, N=0)
        f.K[:] = (500.0, 500.0, 320.0, 240.0)
        f.bounds[:] = (0.0, 640.0, 0.0, 480.0)
        for k, v in over.items():
            setattr(f, k, v)
        keep.append(f)
        return f

    def track_problem(**over):
        p = _lib.TrackProblemC(frame=track_frame(), mode=_lib.DSH_TRACK_FRAME, th=20.0, Q=0)
        for k, v in over.items():
            setattr(p, k, v)
        return ref(p)

    def schwarp_problem(**over):
        p = _lib.SchwarpProblemC(bbs=_lib.BbsC(0.0, 1.0, 5, 0.0, 1.0, 5, 2), P=0, fx_slot=1.0, fy_slot=1.0, lam=1.0, fx=500.0, fy=500.0, max_iters=10,
                                 x=buf().value)
        for k, v in over.items():
            setattr(p, k, v)
        return ref(p)

    def kf(**over):
        k = _lib.MpKeyFrameC(N=0, levels=1, scale_factors=C.cast(one, _lib.c_float_p))
        for n, v in over.items():
            setattr(k, n, v)
        return ref(k)

    out = C.c_void_p()
    o = ref(out)
    i64 = buf()
    P = buf   # an output / input array large enough for every minimal call below
    ctx = "ctx"
    return [
        ("dsh_synchronize", (ctx,), NODEV, (None,), ARG),
        ("dsh_template_build", (ctx, I(3), P(), I(1), buf(fill=np.array([0, 1, 2], np.int32))), DSH_OK,
         (ctx, I(3), P(), I(1), buf(fill=np.array([0, 1, 3], np.int32))), ARG),
        ("dsh_template_dims", (ctx, P(), P(), P()), DSH_OK, (None, P(), P(), P()), STATE),
        ("dsh_template_get", (ctx,) + tuple(P() for _ in range(8)), DSH_OK, (None,) + tuple(P() for _ in range(8)), STATE),
        ("dsh_template_embed", (ctx, I(1), P(), P(), P(), P()), DSH_OK, (ctx, I(1), None, P(), P(), P()), ARG),
        ("dsh_template_embed_device", (ctx, I(1), P(), P(), P(), P()), NODEV, (ctx, I(1), None, P(), P(), P()), ARG),
        ("dsh_sft_solve", (ctx, frame(), P()), NODEV, (ctx, None, P()), ARG),
        ("dsh_sft_batch_upload", (ctx, I(1), frame()), DSH_OK, (ctx, I(0), frame()), ARG),
        ("dsh_sft_batch_run", (ctx,), NODEV, (None,), ARG),
        ("dsh_sft_batch_download", (ctx, I(0), P()), NODEV, (ctx, I(0), None), ARG),
        ("dsh_sft_batch_counts", (ctx, i64, i64), STATE, (None, i64, i64), STATE),
        ("dsh_sft_batch_problem_info", (ctx, I(0), P(), P()), ARG, (ctx, I(-1), P(), P()), ARG),
        ("dsh_comm_create", (ctx, I(1), I(0), P(), o), NODEV, (ctx, I(1), I(1), P(), o), ARG),
        ("dsh_comm_destroy", (None,), ARG, (None,), ARG),
        ("dsh_sft_shared_solve", (ctx, None, frame(), P()), ARG, (ctx, None, None, P()), ARG),
        ("dsh_sft_shared_solve_group", (I(1), "ctxs", frame(), P()), NODEV, (I(0), None, frame(), P()), ARG),
        ("dsh_sft_connected_solve", (ctx, None, frame(), P()), ARG, (ctx, None, None, P()), ARG),
        ("dsh_sft_connected_solve_group", (ctx, ctx, frame(), P()), ARG, (ctx, None, frame(), P()), ARG),
        ("dsh_bbs_eval", (ctx, bbs, P(), None, None, I(0), I(0), I(0), None, None), NODEV, (ctx, bad_bbs, P(), None, None, I(0), I(0), I(0), None, None), NODEV),
        ("dsh_bbs_coloc", (ctx, bbs, None, None, I(0), I(0), I(0), None, None, None), NODEV, (ctx, bbs, None, None, I(0), I(3), I(0), None, None, None), NODEV),
        ("dsh_normals_estimate", (ctx, I(0), buf(fill=np.zeros(1, np.int32))) + (None,) * 7 + (P(),) + (None,) * 6, NODEV,
         (ctx, I(-1), buf(fill=np.zeros(1, np.int32))) + (None,) * 7 + (P(),) + (None,) * 6, NODEV),
        ("dsh_schwarp_eval", (ctx, bbs, I(0), None, None, None, D(1), D(1), D(1), P(), None, None), NODEV,
         (ctx, bad_bbs, I(0), None, None, None, D(1), D(1), D(1), P(), None, None), NODEV),
        ("dsh_schwarp_fit", (ctx, bbs, I(0), None, None, None, D(1), D(1), D(1), F(500), F(500), I(10), P(), None, None, P(), P()), NODEV,
         (ctx, bbs, I(0), None, None, None, D(1), D(1), D(1), F(500), F(500), I(10), None, None, None, P(), P()), NODEV),
        ("dsh_schwarp_fit_batch", (ctx, I(1), schwarp_problem()), NODEV, (ctx, I(-1), schwarp_problem()), NODEV),
        ("dsh_diffdb_create", (ctx, L64(16), o), NODEV, (ctx, L64(-1), o), ARG),
        ("dsh_diffdb_destroy", (None,), ARG, (None,), ARG),
        ("dsh_diffdb_clear", (None,), ARG, (None,), ARG),
        ("dsh_diffdb_append", (None, I(0), None, None, None, None), ARG, (None, I(-1), None, None, None, None), ARG),
        ("dsh_schwarp_fit_batch_store", (ctx, I(1), schwarp_problem(), P(), None), ARG, (ctx, I(-1), schwarp_problem(), P(), None), ARG),
        ("dsh_normals_estimate_db", (ctx, None, I(0)) + (None,) * 9 + (I(0), P()) + (None,) * 5, NODEV,
         (ctx, None, I(-1)) + (None,) * 9 + (I(0), P()) + (None,) * 5, NODEV),
        ("dsh_sfn_estimate", (ctx, bbs, I(0), None, None, None, D(1e-3), D(1), I(0), None, None, P(), P(), None, P()), NODEV,
         (ctx, bad_bbs, I(0), None, None, None, D(1e-3), D(1), I(0), None, None, P(), P(), None, P()), NODEV),
        ("dsh_sfn_estimate_db", (ctx, bbs, None, I(0), None, None, None, D(1e-3), D(1), I(0), None, None, P(), P(), None, P()), ARG,
         (ctx, bad_bbs, None, I(0), None, None, None, D(1e-3), D(1), I(0), None, None, P(), P(), None, P()), ARG),
        ("dsh_warp_initialize", (ctx, bbs, I(0), None, None, D(1), P(), P()), NODEV, (ctx, bbs, I(-1), None, None, D(1), P(), P()), NODEV),
        ("dsh_search_by_schwarp", (ctx, bbs, P(), I(0), None, None, P(), P(), I(64), I(48), I(0), None, None, None, F(10), I(50), None, P()), NODEV,
         (ctx, bbs, P(), I(-1), None, None, P(), P(), I(64), I(48), I(0), None, None, None, F(10), I(50), None, P()), NODEV),
        ("dsh_scale_min_median", (ctx, I(1), P(), P(), None, L64(0), P(), P(), P()), NODEV, (ctx, I(0), P(), P(), None, L64(0), P(), P(), P()), ARG),
        ("dsh_optimize_horn", (ctx, I(1), P(), P(), P(), D(1), D(0.01), P(), P()), NODEV, (ctx, I(1), P(), P(), P(), D(1), D(-1), P(), P()), ARG),
        ("dsh_surface_register", (ctx, I(15), P(), P(), None, L64(0), eye, D(0.05), I(1), P(), P(), P(), P(), P()), NODEV,
         (ctx, I(15), P(), P(), None, L64(0), None, D(0.05), I(1), P(), P(), P(), P(), P()), ARG),
        ("dsh_search_by_projection_batch", (ctx, I(1), track_problem()), NODEV, (ctx, I(1), track_problem(mode=2)), ARG),
        ("dsh_search_by_projection_frame", (ctx, ref(track_frame()), I(0), None, None, None, F(20), None, P()), NODEV,
         (ctx, ref(track_frame(levels=0)), I(0), None, None, None, F(20), None, P()), ARG),
        ("dsh_search_by_projection_local", (ctx, ref(track_frame()), I(0), None, None, None, None, None, F(3), None, None, None, P()), NODEV,
         (ctx, ref(track_frame()), I(-1), None, None, None, None, None, F(3), None, None, None, P()), ARG),
        ("dsh_kfdb_create", (ctx, I(16), o), NODEV, (ctx, I(0), o), ARG),
        ("dsh_kfdb_destroy", (None,), ARG, (None,), ARG),
        ("dsh_kfdb_clear", (None,), ARG, (None,), ARG),
        ("dsh_kfdb_add", (None, kf(), P()), ARG, (None, None, P()), ARG),
        ("dsh_kfdb_set_bad", (None, I(0), I(1)), ARG, (None, I(-1), I(1)), ARG),
        ("dsh_mappoint_update", (ctx, None, I(0), None, buf(fill=np.zeros(1, np.int32)), None, None, None, I(1), P(), P(), None, None, None, P()), NODEV,
         (ctx, None, I(0), None, buf(fill=np.zeros(1, np.int32)), None, None, None, I(0), P(), P(), None, None, None, P()), ARG),
    ]


def _host_only_call(name, args):
    """Status and dsh_last_error of one call on a fresh host-only context (a fresh one: the message is the call's own)."""
    from defslam_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)   # its own function objects: untyped, the rows pass ctypes values
    L.dsh_last_error.restype = C.c_char_p
    ctx = C.c_void_p()
    assert L.dsh_create(C.byref(ctx), -1) == 0
    try:   # a template built from one facet: the calls that need one get past that check
        xyz = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1]], np.float64)
        assert L.dsh_template_build(ctx, 3, C.c_void_p(xyz.ctypes.data), 1, C.c_void_p(np.array([0, 1, 2], np.int32).ctypes.data)) == 0
        ctxs = (C.c_void_p * 1)(ctx)
        rc = getattr(L, name)(*[ctx if a == "ctx" else ctxs if a == "ctxs" else a for a in args])
        return rc, (L.dsh_last_error(ctx) or b"").decode()
    finally:
        assert L.dsh_destroy(ctx) == 0


def test_host_only_status_of_every_entry_point():
    """Order of checks on a host-only context: every product entry point that takes a context, store or communicator, once with
    minimal well-formed arguments and once with one malformed argument.  Which of argument checks and the device gate comes first is
    part of the contract (e.g. dsh_mappoint_update: arguments first); a refusal for want of a device says "host-only"."""
    keep = []
    rows = _host_only_rows(keep)
    header = open(os.path.join(ROOT, "include", "defslam_hip.h")).read()
    takes = set(re.findall(r"\b(dsh_[a-z0-9_]+)\s*\((?:[^)]*\b(?:dsh_ctx|dsh_diffdb|dsh_kfdb|dsh_comm)\b)", header))
    # not in the table: the context's life cycle, the calls that return no status, dsh_template_set (its malformed arrays: above)
    assert {r[0] for r in rows} == takes - {"dsh_create", "dsh_destroy", "dsh_last_error", "dsh_stream", "dsh_diffdb_count", "dsh_kfdb_count",
                                            "dsh_template_set"}
    for name, good, good_rc, bad, bad_rc in rows:
        for args, want in ((good, good_rc), (bad, bad_rc)):
            rc, msg = _host_only_call(name, args)
            assert rc == want, (name, args is bad, rc, msg)
            if rc == NODEV and name not in _HOST_ONLY_MESSAGE_EMPTY:
                assert "host-only" in msg, (name, msg)


def test_host_files_declare_no_launcher_prototypes():
    """A kernel launcher is declared once, in a header that its .hip file includes too, so the compiler checks the declaration
    against the definition (an extern "C" name carries no parameter types: a drifted prototype would still link).  No host file
    declares an extern "C" function it does not define; `extern "C" {` blocks and definitions are fine."""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "defslam_amd", "csrc", "*.cpp"))):
        src = re.sub(r"//[^\n]*", "", open(path).read())
        for m in re.finditer(r'extern\s+"C"\s*([^{;]*)([{;])', src):
            assert not (m.group(2) == ";" and m.group(1).strip()), f"{os.path.basename(path)}: extern \"C\" {' '.join(m.group(1).split())[:80]}"
