"""~point_order of the node shells and mot_adapters::Config::point_order REACH mot_set_point_order (emulator build of the kernels): the permuted
blob cloud of tests/point_order_cases.py — more (tile, cluster) groups than MOT_ORDER_SCAN takes at 8192 points — gives the oracle's boxes with
"any", the "cloud too fragmented" refusal with "scan" (and by default), and an error with anything else."""
import os
import subprocess
import sys

import numpy as np
import pytest

import capacity_cases as CC
import nodes_build as NB
import nodes_util as U
import point_order_cases as PC
import roslog as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
pytestmark = pytest.mark.skipif(not NB.have_reference(), reason="the ROS / PCL shim needs the reference's vendored Eigen")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def emu_lib():
    import build_emu
    return build_emu.build()


@pytest.fixture(scope="module")
def case(_oracle_module):
    """the cloud, the oracle's boxes [n][8][3], and the proof that the default mode cannot take it"""
    oracle = _oracle_module
    p = oracle.params(0)
    elev = PC.permuted(CC.box_blob_cloud(200, 32), 7)
    o = CC.oracle_stage(oracle, p, elev)
    assert CC.group_count(o["cl"]["point_label"]) > 8192 // 2 and 1 <= len(o["bx"]["boxes"]) <= 255
    return elev, o["bx"]["boxes"]


def node_boxes(out):
    msgs = [R.decode(ty, x) for t, ty, x in out if t == "track_box"]
    assert len(msgs) == 1
    m = msgs[0]
    corners = [np.asarray(m[k], np.float32).reshape(-1, 3) for k in ("x1", "x2", "x3", "x4", "y1", "y2", "y3", "y4")]
    return m["box_num"], np.stack(corners, axis=1)


def test_cluster_node_point_order_parameter(emu_lib, case, tmp_path):
    elev, want = case
    node = NB.own_nodes(emu_lib)["cluster"]
    recs = [("__now__", U.T0 + 0.01), ("none_ground_topic", "sensor_msgs/PointCloud2", R.pointcloud2(elev, U.T0))]
    n, got = node_boxes(U.run(node, recs, tmp_path, "any", {"_max_points": 8192, "_point_order": "any"}))
    assert n == len(want) and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for name, prm in (("scan", {"_max_points": 8192, "_point_order": "scan"}), ("default", {"_max_points": 8192})):
        with pytest.raises(RuntimeError, match="cloud too fragmented"):
            U.run(node, recs, tmp_path, name, prm)
    with pytest.raises(RuntimeError, match="point_order must be"):
        U.run(node, recs, tmp_path, "bad", {"_max_points": 8192, "_point_order": "sideways"})


def point_order_driver(lib):
    src = os.path.join(HERE, "drivers", "adapter_point_order_driver.cpp")
    exe = os.path.join(NB.OWN_BIN, "adapter_point_order_driver")
    os.makedirs(NB.OWN_BIN, exist_ok=True)
    deps = [src, lib, os.path.join(ROOT, "include", "mot_adapters.hpp"), os.path.join(ROOT, "include", "mot.h")] + NB._shim_files()
    if not NB._newer(exe, deps, lib):
        NB._cxx(["-I", NB.SHIM, "-I", os.path.join(NB.REF, "tracking"), "-I", os.path.join(ROOT, "include"), src, "-o", exe] + NB._link_args(lib), exe)
        NB._stamp(exe, lib)
    return exe


def test_adapter_config_point_order(emu_lib, case, tmp_path):
    elev, want = case
    exe = point_order_driver(emu_lib)
    i, o = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(i, "wb") as f:
        f.write(np.int32(len(elev)).tobytes()); f.write(np.ascontiguousarray(elev, np.float32).tobytes())
    run = lambda order: subprocess.run([exe, i, o, str(order)], capture_output=True, text=True, timeout=600)
    r = run(1)
    assert r.returncode == 0, r.stderr[-1000:]
    raw = open(o, "rb").read()
    nb = int(np.frombuffer(raw[:4], np.int32)[0])
    got = np.frombuffer(raw[4:], np.float32).reshape(nb, 8, 3)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    r = run(0)
    assert r.returncode == 3 and "cloud too fragmented" in r.stderr, (r.returncode, r.stderr[-500:])
    r = run(5)
    assert r.returncode != 0 and "mot_set_point_order" in r.stderr, (r.returncode, r.stderr[-500:])
