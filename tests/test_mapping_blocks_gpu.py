"""GPU tests of the paths of the mapping-side one-shot calls that depend on how a call lays out its copy blocks (UpBlock / DownBlock of
defslam_amd/csrc/dsh_ctx.h) and that no other test reaches: optional outputs that are absent, slices without an element, page-locked
buffers that grow between two calls.  Through ctypes, because the Python wrappers always pass every array.  Every output array is two
elements longer than the call may write and pre-filled with a marker that must survive; every input array must come back unchanged.  An
output that is present must equal, byte for byte, the same output of the call with all outputs present -- which the parity tests compare
with the oracle (tests/test_nrsfm_gpu.py, test_register_gpu.py, test_diffdb_gpu.py).  Shapes are the smallest the calls accept: a 4 x 4
control grid, 1 and 3 sites, 2 map points with 3 records, 3 matches, 3 pairs (15 for dsh_surface_register), a 3 x 3-node template."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, ARG = 0, 1


def ptr(a):
    return a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))


def mark(dtype):
    return np.dtype(dtype).type(0xA5 if np.dtype(dtype) == np.uint8 else -7)


def run(L, name, args, absent=()):
    """Calls L.<name>.  args: ctypes values, numpy arrays (inputs: they must come back unchanged), None, and outputs as (name, count, dtype) or
    (name, count, dtype, start values); an output named in `absent` is passed as NULL.  Returns (status, {output name: bytes written})."""
    call, outs, ins = [], {}, []
    for a in args:
        if isinstance(a, tuple):
            if a[0] in absent:
                call.append(None)
                continue
            buf = np.full(a[1] + 2, mark(a[2]), a[2])
            if len(a) > 3:
                buf[:a[1]] = a[3]
            outs[a[0]] = (buf, a[1])
            call.append(ptr(buf))
        elif isinstance(a, np.ndarray):
            ins.append((a, a.tobytes()))
            call.append(ptr(a))
        else:
            call.append(a)
    rc = getattr(L, name)(*call)
    for a, was in ins:
        assert a.tobytes() == was, name + ": an input array was written"
    res = {}
    for nm, (buf, n) in outs.items():
        assert (buf[n:] == mark(buf.dtype)).all(), f"{name}: {nm} was written past its {n} elements"
        res[nm] = buf[:n].tobytes()
    return rc, res


def check_absent(L, name, args, subsets):
    """The call with all outputs, then without each of `subsets`: what is still present is the same bytes."""
    rc, full = run(L, name, args)
    assert rc == OK
    for s in subsets:
        rc, part = run(L, name, args, absent=s)
        assert rc == OK and set(part) == set(full) - set(s)
        for nm, b in part.items():
            assert b == full[nm], f"{name} without {sorted(s)}: {nm} differs"
    return full


def untouched(res, names):
    return all(res[nm] == np.full(len(res[nm]) // np.dtype(dt).itemsize, mark(dt), dt).tobytes() for nm, dt in names)


def grid(valdim):
    from defslam_amd import _lib
    return _lib.BbsC(-0.6, 0.6, 4, -0.5, 0.5, 4, valdim)


def sites(n, seed=1):
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-0.55, 0.55, n), rng.uniform(-0.45, 0.45, n)
    u[0] = 0.7   # outside the domain
    return u, v


@pytest.mark.parametrize("valdim,n", [(1, 1), (2, 3)])
def test_bbs_eval_and_coloc_without_their_optional_outputs(gpu_ctx, valdim, n):
    L, b = gpu_ctx._L, grid(valdim)
    u, v = sites(n)
    ctrl = np.random.default_rng(2).normal(size=16 * valdim)
    full = check_absent(L, "dsh_bbs_eval", [gpu_ctx._h, C.byref(b), ctrl, u, v, n, 1, 0, ("val", n * valdim, np.float64), ("outside", n, np.uint8)], [{"outside"}])
    assert full["outside"][0] == 1
    full = check_absent(L, "dsh_bbs_coloc", [gpu_ctx._h, C.byref(b), u, v, n, 0, 1, ("cols", 16 * n, np.int32), ("w", 16 * n, np.float64), ("n_outside", 1, np.int32)],
                        [{"n_outside"}])
    assert np.frombuffer(full["n_outside"], np.int32)[0] == 1


def normals_inputs(rec_ptr):
    """2 map points over the first rec_ptr[2] of 4 records."""
    from defslam_amd import synth
    sc = synth.make_normals_scene(2, 2, seed=5, min_views=2)
    assert sc["recs"].shape[0] == 4
    R = rec_ptr[2]
    cut = lambda k: np.ascontiguousarray(sc[k][:R]) if R else None
    return np.array(rec_ptr, np.int32), cut("recs"), cut("rec_is_ref"), cut("rec_first_normal"), cut("rec_has_first_normal"), sc["x0"], sc["has_x0"], sc["ref_uv"]


def normals_args(ctx, rec_ptr):
    ptr_, recs, is_ref, fn, hfn, x0, hx0, uv = normals_inputs(rec_ptr)
    R = rec_ptr[2]
    return [ctx._h, 2, ptr_, recs, is_ref, fn, hfn, x0, hx0, uv, ("k1k2", 4, np.float64), ("cov", 8, np.float64), ("status", 2, np.int32), ("normal_ref", 6, np.float32),
            ("normal_rec", 3 * R, np.float32), ("rec_written", R, np.uint8), ("iters", 2, np.int32)]


NORMALS_OPTIONAL = ["cov", "normal_ref", "iters", "normal_rec", "rec_written"]


@pytest.mark.parametrize("rec_ptr", [[0, 1, 3], [0, 0, 3], [0, 0, 0]], ids=["records_on_both", "records_on_the_second", "no_record"])
def test_normals_without_optional_outputs_and_with_each_one_alone(gpu_ctx, rec_ptr):
    alone = [set(NORMALS_OPTIONAL) - {nm} for nm in NORMALS_OPTIONAL]
    full = check_absent(gpu_ctx._L, "dsh_normals_estimate", normals_args(gpu_ctx, rec_ptr), [set(NORMALS_OPTIONAL)] + alone)
    if not rec_ptr[1]:
        assert np.frombuffer(full["status"], np.int32)[0] == 1   # a point without a record is skipped, not solved


def normals_db_args(ctx, db, max_rec):
    _, _, _, _, _, x0, hx0, uv = normals_inputs([0, 1, 3])
    return [ctx._h, db._h, 2, np.array([5, 9], np.int32), x0, hx0, uv, ("k1k2", 4, np.float64), ("cov", 8, np.float64), ("status", 2, np.int32),
            ("normal_ref", 6, np.float32), ("iters", 2, np.int32), max_rec, ("n_rec", 1, np.int32), ("rec_point", 3, np.int32), ("rec_tag", 3, np.int32),
            ("rec_idx2", 3, np.int32), ("normal_rec", 9, np.float32), ("rec_written", 3, np.uint8)]


def test_normals_db_without_per_record_buffers_and_with_too_small_ones(gpu_ctx):
    from defslam_amd import nrsfm
    recs = normals_inputs([0, 1, 3])[1]
    db = nrsfm.DiffDatabase(gpu_ctx, 8)
    db.append(recs, [5, 9, 9], tag=[3, 4, 4], idx2=[7, 8, 6])
    per_record = {"rec_point", "rec_tag", "rec_idx2", "normal_rec", "rec_written"}
    full = check_absent(gpu_ctx._L, "dsh_normals_estimate_db", normals_db_args(gpu_ctx, db, 3), [per_record, per_record | {"cov", "normal_ref", "iters", "n_rec"}])
    assert np.frombuffer(full["n_rec"], np.int32)[0] == 3
    assert np.frombuffer(full["rec_point"], np.int32).tolist() == [0, 1, 1] and np.frombuffer(full["rec_idx2"], np.int32).tolist() == [7, 8, 6]
    rc, res = run(gpu_ctx._L, "dsh_normals_estimate_db", normals_db_args(gpu_ctx, db, 2))   # one below R: refused, the count reported
    assert rc == ARG and np.frombuffer(res["n_rec"], np.int32)[0] == 3
    assert untouched(res, [("rec_point", np.int32), ("rec_tag", np.int32), ("rec_idx2", np.int32), ("normal_rec", np.float32), ("rec_written", np.uint8)])
    rc, again = run(gpu_ctx._L, "dsh_normals_estimate_db", normals_db_args(gpu_ctx, db, 3))   # the context and the database stay usable
    assert rc == OK and again == full
    db.close()


def test_schwarp_eval_without_the_jacobian(gpu_ctx):
    b = grid(2)
    rng = np.random.default_rng(3)
    kp1 = rng.uniform(-0.4, 0.4, (3, 2)).astype(np.float32)
    kp2 = (kp1 + rng.normal(scale=0.01, size=(3, 2))).astype(np.float32)
    x = rng.uniform(-0.5, 0.5, 32)
    m = 2 * 3 + 4 * 16
    check_absent(gpu_ctx._L, "dsh_schwarp_eval", [gpu_ctx._h, C.byref(b), 3, kp1, kp2, np.ones(3, np.float32), 1.0, 1.0, 0.1, x,
                                                   ("residuals", m, np.float64), ("jacobian", m * 32, np.float64)], [{"jacobian"}])


def sfn_args(ctx, n, n_all):
    from defslam_amd import synth
    sc = synth.make_sfn_scene(3, seed=6, with_normal_frac=1.0, nu=4, nv=4)
    b = C.byref(_bbs(sc["bbs"]))
    take = lambda a, k: np.ascontiguousarray(a[:k]) if k else None
    return [ctx._h, b, n, take(sc["u"], n), take(sc["v"], n), take(sc["normals"], n), 1e-2, sc["mean_depth"], n_all, take(sc["u_all"], n_all),
            take(sc["v_all"], n_all), ("ctrl_raw", 16, np.float64), ("ctrl", 16, np.float64), ("pts", 3 * n_all, np.float32), ("ok", 1, np.int32)]


def _bbs(t):
    from defslam_amd import _lib
    return _lib.BbsC(*t)


@pytest.mark.parametrize("n,n_all", [(3, 3), (0, 3), (3, 0)])
def test_sfn_estimate_without_ctrl_raw_and_with_empty_inputs(gpu_ctx, n, n_all):
    full = check_absent(gpu_ctx._L, "dsh_sfn_estimate", sfn_args(gpu_ctx, n, n_all), [{"ctrl_raw"}])
    ok = np.frombuffer(full["ok"], np.int32)[0]
    if n and n_all:
        assert ok == 1
    if not n_all:   # the control points are solved for and handed out raw; nothing is scaled or evaluated
        assert ok == 0 and untouched(full, [("ctrl", np.float64)]) and not untouched(full, [("ctrl_raw", np.float64)])


@pytest.mark.parametrize("n2", [None, 0])
def test_search_by_schwarp_without_nmatches_and_without_candidates(gpu_ctx, n2):
    from defslam_amd import synth
    sc = synth.make_match_scene(2 if n2 == 0 else 3, 2, seed=4, nu=4, nv=4)
    b = _bbs(sc["bbs"])
    N2 = sc["kp2"].shape[0] if n2 is None else 0
    kp2, d2, mp2 = (sc["kp2"], sc["desc2"], sc["has_mp2"]) if N2 else (None, None, None)
    Q = sc["kp1"].shape[0]
    full = check_absent(gpu_ctx._L, "dsh_search_by_schwarp", [gpu_ctx._h, C.byref(b), sc["x"], Q, sc["kp1"], sc["desc1"], sc["cam2"], sc["bounds2"], 64, 48, N2, kp2, d2, mp2,
                                                             2.0, 50, ("match", Q, np.int32), ("nmatches", 1, np.int32)], [{"nmatches"}])
    match = np.frombuffer(full["match"], np.int32)
    assert np.frombuffer(full["nmatches"], np.int32)[0] == (match >= 0).sum() and (N2 or (match == -1).all())


def test_registration_calls_without_info_and_consumed(gpu_ctx):
    from defslam_amd import synth
    L, h = gpu_ctx._L, gpu_ctx._h
    sc = synth.make_register_scene(3, seed=8, outliers=0.0)
    init = np.array([0, 0, 0, 1, 0, 0, 0, 1.3])
    check_absent(L, "dsh_optimize_horn", [h, 3, sc["surface"], sc["map"], ("sim3", 8, np.float64, init), 0.05 ** 2, 0.01, ("acceptable", 1, np.int32),
                                          ("info", 6, np.float64)], [{"info"}])
    smm = lambda u: [h, 3, sc["surface"], sc["map"], u, u.shape[0], ("scale", 1, np.float32), ("consumed", 1, np.int64), ("status", 1, np.int32)]
    full = check_absent(L, "dsh_scale_min_median", smm(np.full(12, 0.1)), [{"consumed"}])
    assert np.frombuffer(full["consumed"], np.int64)[0] == 9
    full = check_absent(L, "dsh_scale_min_median", smm(np.ones(3)), [{"consumed"}])      # no point is a candidate: an empty candidate list
    assert np.frombuffer(full["consumed"], np.int64)[0] == 3
    sc = synth.make_register_scene(15, seed=9, outliers=0.0)
    full = check_absent(L, "dsh_surface_register", [h, 15, sc["surface"], sc["map"], sc["u"], sc["u"].shape[0], sc["Twc"].reshape(16), 0.05, 0,
                                                    ("registered", 1, np.int32), ("sim3", 8, np.float64), ("s22", 1, np.float64), ("Tcw", 16, np.float32),
                                                    ("info", 8, np.float64)], [{"info"}])
    assert np.frombuffer(full["registered"], np.int32)[0] == 1


def test_template_embed_device_writes_one_point_and_no_more():
    from defslam_amd import sft, synth
    ctx = sft.Context(0)   # its own context: the template is part of a context
    tmpl = synth.make_grid_template(3, 3)
    ctx.template_build(tmpl.xyz0, tmpl.facets)
    pts = tmpl.xyz0[tmpl.facets[1]].mean(0, keepdims=True).astype(np.float32)
    rc, res = run(ctx._L, "dsh_template_embed_device", [ctx._h, 1, pts, ("facet_id", 1, np.int32), ("nodes", 3, np.int32), ("bary", 3, np.float32)])
    fid, nodes, bary = ctx.template_embed(pts)   # the host routine: the same bits (tests/test_register_gpu.py)
    assert rc == OK and fid[0] >= 0 and (res["facet_id"], res["nodes"], res["bary"]) == (fid.tobytes(), nodes.tobytes(), bary.tobytes())
    ctx.close()


def grown_calls(ctx, size):
    """One call of each family at `size` sites / pairs."""
    from defslam_amd import synth
    b = grid(2)
    u, v = sites(size, seed=size)
    ctrl = np.random.default_rng(7).normal(size=32)
    rc, ev = run(ctx._L, "dsh_bbs_eval", [ctx._h, C.byref(b), ctrl, u, v, size, 0, 0, ("val", 2 * size, np.float64), ("outside", size, np.uint8)])
    assert rc == OK
    sc = synth.make_register_scene(size, seed=9, outliers=0.0)
    rc, reg = run(ctx._L, "dsh_surface_register", [ctx._h, size, sc["surface"], sc["map"], sc["u"], sc["u"].shape[0], sc["Twc"].reshape(16), 0.05, 0,
                                                   ("registered", 1, np.int32), ("sim3", 8, np.float64), ("s22", 1, np.float64), ("Tcw", 16, np.float32),
                                                   ("info", 8, np.float64)])
    assert rc == OK
    return ev, reg


def test_a_larger_second_call_grows_the_page_locked_buffers():
    """15 sites / pairs, then 600 (more than the buffers of the first call hold): the second call equals the same call on a fresh context."""
    from defslam_amd import sft
    a, fresh = sft.Context(0), sft.Context(0)
    grown_calls(a, 15)
    assert grown_calls(a, 600) == grown_calls(fresh, 600)
    a.close()
    fresh.close()
