"""The Shape-from-Template shim on the map point store (integration/def_pose_store_hip.h) compiled against the stand-in Template / Frame /
DefMap / DefMapPoint types and run on the device: one frame the store way (DefPoseOptimizationStoreHIP: dsh_track_sft with write-back,
the objects follow) and the existing way (DefPoseOptimizationHIP: the table from a walk over the objects, dsh_sft_solve,
RecalculatePosition on the host) over two copies of the same objects.  Every mutated field of the two copies is equal: the return
value, mvbOutlier, repError, the pose, the nodes' positions, indices and roles, and every map point's position -- as bit patterns."""
import os

import numpy as np
import pytest

import shim_run
import track_sft_ref as R

INTEG = shim_run.INTEG
CASES = dict(full=dict(seed=0, regs=(700.0, 12000.0, 0.05)), partial_reg_temp0=dict(seed=3, partial=True, regs=(700.0, 12000.0, 0.0)))


def test_shim_compiles_against_the_c_abi():
    shim_run.build()
    assert os.path.exists(shim_run.exe("tracksft_shim_test"))
    src = open(os.path.join(INTEG, "def_pose_store_hip.h")).read()
    assert "dsh_track_sft(" in src and "DefPoseOptimizationStoreHIP" in src and "defslam_hip_debug.h" not in src and "dsh_lab" not in src
    assert "dsh_point_store_get_embedding" not in src and "dsh_sft_solve" not in src


def write_input(sc, regs, path):
    r = lambda v: " ".join(repr(float(x)) for x in np.asarray(v).reshape(-1))
    nodes, bary = sc.model.embedding_arrays()
    with open(path, "w") as f:
        f.write(f"{sc.tmpl.n} {len(sc.tmpl.facets)}\n")
        for row in sc.tmpl.xyz0:
            f.write(r(row) + "\n")
        for row in sc.xyz:
            f.write(r(row) + "\n")
        for a, b, c in sc.tmpl.facets:
            f.write(f"{a} {b} {c}\n")
        f.write(r(np.asarray(sc.K, np.float32)) + "\n" + r(np.asarray(sc.Tcw, np.float32)) + "\n")
        f.write(f"{len(sc.frame_points)} {R.LEVELS}\n{r(R.INV_LEVEL_SIGMA2)}\n{len(sc.model.points)}\n")
        for p, pt in enumerate(sc.model.points):
            f.write(f"{int(pt.bad)} {int(nodes[p, 0] >= 0)} {nodes[p, 0]} {nodes[p, 1]} {nodes[p, 2]} {r(bary[p])} {r(pt.xyz)}\n")
        for i in range(len(sc.frame_points)):
            f.write(f"{r(sc.kp[i])} {int(sc.octave[i])} {int(sc.frame_points[i])} {int(sc.outlier[i])}\n")
        f.write(f"{r(regs)} 1\n")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_store_way_and_existing_way_mutate_alike(tmp_path, name):
    shim_run.build()
    kw = dict(CASES[name])
    regs = kw.pop("regs")
    sc = R.make_scene(N=300, n_rows=150, **kw)
    src, dst = str(tmp_path / "in.txt"), str(tmp_path / "out")
    write_input(sc, regs, src)
    shim_run.run("tracksft_shim_test", src, dst)
    store, host = open(dst + ".store").read(), open(dst + ".host").read()
    head = dict(zip(store.split()[0:12:2], store.split()[1:12:2]))
    print(f"{name}: {store.splitlines()[0]}")
    moved = sum(1 for p, pt in enumerate(sc.model.points) if not pt.bad and sc.model.nodes[p] is not None)
    assert int(head["ret"]) > 0 and int(head["pose_sets"]) == 1 and int(head["held"]) == 0
    assert int(head["recalculated"]) == int(head["under_lock"]) == moved
    assert store == host
    flags = [int(x) for x in store.splitlines()[2 + sc.tmpl.n].split()[1:]]
    assert len(flags) == len(sc.frame_points) and all(flags[i] for i in np.nonzero(sc.outlier)[0])
    start = [f"pt {' '.join(str(int(b)) for b in pt.xyz.view(np.uint32))} 0" for pt in sc.model.points]
    pts = store.splitlines()[3 + sc.tmpl.n:]
    assert len(pts) == len(start) and sum(a != b for a, b in zip(pts, start)) == moved
