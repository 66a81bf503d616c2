"""The layers above mot_tracking_node_frame, on the emulator build of the kernels (CPU):
  * the `tracking` node shell (ros/src/tracking_node.cpp: one library call per track_box message, no tf listener) against the reference's own `tracking`
    node on three of tests/test_emu_tracker_random.py's sequences — same topics, same marker ids, positions and poses within the suite's 1e-4;
  * mot_adapters::trackingNodeFrame (include/mot_adapters.hpp) through tests/drivers/adapter_tracking_frame_driver.cpp against the stage-wise sequence
    mot_ego_update -> boxes through global_from_sensor -> mot_track_step -> records through sensor_from_global, value for value.
tests/test_nodes.py runs the same shell through the whole node chain; tests/test_sensor_tracks_gpu.py runs the library call on the MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nodes_build as NB
import nodes_util as U
import sensor_track_cases as ST

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
pytestmark = pytest.mark.skipif(not NB.have_reference(), reason="the reference sources (the shim needs their vendored Eigen) are not on this box")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu_lib():
    import build_emu
    return build_emu.build()


def _trackbox(R, boxes, t, seq):
    m = dict(header=dict(seq=seq, stamp=R.stamp(t), frame_id="velodyne"), box_num=len(boxes) & 255)
    for k, name in enumerate(("x1", "x2", "x3", "x4", "y1", "y2", "y3", "y4")):
        m[name] = boxes[:, k, :].reshape(-1).astype(np.float32)
    return m


@pytest.mark.parametrize("seed", [91001, 91002, 91003])
def test_tracking_shell_publishes_what_the_reference_node_publishes(seed, emu_lib, tmp_path):
    import roslog as R
    import test_emu_tracker_random as TR
    ref = NB.reference_nodes()["tracking"]
    own = NB.own_nodes(emu_lib)["tracking"]
    recs = []
    for f, (boxes, ts, v, yaw) in enumerate(TR.sequence(seed)):
        t = U.T0 + 0.1 * f
        odom = dict(header=dict(seq=f, stamp=R.stamp(t), frame_id="gps"), child_frame_id="base_link",
                    pose=dict(pose=dict(orientation=dict(x=0.0, y=0.0, z=float(yaw) + 0.3, w=1.0))),
                    twist=dict(twist=dict(linear=dict(x=float(v), y=0.2, z=0.0))))
        recs += [("__now__", t + 0.01), ("/gps/odom", "nav_msgs/Odometry", odom), ("track_box", "object_tracking/trackbox", _trackbox(R, boxes[:255], t, f))]
    a = U.run(ref, recs, tmp_path, "ref"); b = U.run(own, recs, tmp_path, "own")
    assert len(a) >= 4 * 14   # the four POINTS markers of every frame, plus the arrows
    U.markers_close(a, b)
    dots = [R.decode(ty, x) for _, ty, x in b if R.decode(ty, x)["ns"] == "points"]
    assert sum(len(m["points"]) for m in dots) > 0   # tracks were drawn


def _driver(lib):
    src = os.path.join(HERE, "drivers", "adapter_tracking_frame_driver.cpp")
    exe = os.path.join(NB.OWN_BIN, "adapter_tracking_frame_driver")
    os.makedirs(NB.OWN_BIN, exist_ok=True)
    deps = [src, lib, os.path.join(NB.ROOT, "include", "mot_adapters.hpp"), os.path.join(NB.ROOT, "include", "mot.h")]
    if not (os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in deps)):
        d, f = os.path.split(lib)
        r = subprocess.run(["g++"] + NB.FLAGS + ["-I", NB.SHIM, "-I", os.path.join(NB.REF, "tracking"), "-I", os.path.join(NB.ROOT, "include"), src, "-o", exe,
                            "-L", d, "-l:" + f, "-Wl,-rpath," + d], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_adapter_helper_equals_the_stage_wise_sequence(emu_lib, mot, tmp_path):
    import tracker_cases as TC
    frames = [(b, ts) + ST._ego(f) for f, (b, ts, _v, _yaw) in enumerate(TC.fast_lanes(11, 16))]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.txt")
    with open(fin, "wb") as f:
        f.write(np.int32(len(frames)).tobytes())
        for b, ts, v, yaw in frames:
            f.write(np.int32(len(b)).tobytes()); f.write(np.array([ts, v, yaw], np.float64).tobytes()); f.write(np.ascontiguousarray(b, np.float32).tobytes())
    r = subprocess.run([_driver(emu_lib), fin, fout, "32"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(fout).read().splitlines()
    assert len(lines) == len(frames)
    shown = 0
    with mot.Context(mot.params(0, lib=mot.load_library(emu_lib)), max_points=4096, max_batch=1, max_tracks_total=32, lib_path=emu_lib) as c:
        for f, ((b, ts, v, yaw), line) in enumerate(zip(frames, lines)):
            rc, origin, rec, n_ever = ST._stage_wise(c, 0, b, ts, v, yaw)
            assert rc == 0
            w = line.split()
            assert [int(w[0]), int(w[1]), int(w[2]), int(w[3])] == [f, len(rec), n_ever, int((rec["is_vis"] != 0).sum())], (f, w[:4])
            assert np.array_equal(np.array([float(x) for x in w[4:10]]), origin), f
            assert len(w) == 10 + len(rec)
            for t, word in zip(rec, w[10:]):
                p = word.split(":")
                assert [int(x) for x in p[:4]] == [t["id"], t["track_manage"], t["is_static"], t["is_vis"]], (f, word)
                assert np.array_equal(np.array([float(x) for x in p[4:7]], np.float32).view(np.uint32), t["p"].view(np.uint32)), (f, word)
                assert np.array_equal(np.array([float(x) for x in p[7:9]]), t["v_yaw"]), (f, word)
                if t["is_vis"]:
                    shown += 1
                    assert np.array_equal(np.array([float(x) for x in p[9:]], np.float32).view(np.uint32), t["vis_box"].view(np.uint32)), (f, word)
                else:
                    assert len(p) == 9
    assert shown >= 4
