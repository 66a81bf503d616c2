"""Live tracks in the sensor frame (tests/sensor_track_cases.py) on the emulator: the export kernels of csrc/track.hip (MOT_FRAME_SENSOR), the host chain of
the global -> sensor matrix and mot_tracking_node_frame, every case bit for bit. The same bodies run on the MI355X in tests/test_sensor_tracks_gpu.py; the
node shell and the adapter helper in tests/test_nodes_tracking_frame.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import capacity_cases as CC
import sensor_track_cases as ST

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))


@pytest.fixture(scope="module")
def env(mot):
    import build_emu
    return CC.Env(mot, build_emu.build())


@pytest.fixture(scope="module")
def state(env):
    st = ST.State(env)
    yield st
    st.close()


def test_emu_matrix_against_the_reference_call_sequence(env):
    """3000 poses through the node's own lines (OT/tracking/main.cpp:76-83 broadcast, :183-184 pcl_ros::transformPointCloud("/velodyne", ...)) executed by
    tests/drivers/tf_to_sensor_driver.cpp on oracle/ref_shim, against the library's restated matrix applied in fp32: bit for bit"""
    import make_tf_sensor_golden as MG
    if not MG.have_reference():
        pytest.skip("the reference tree (its vendored Eigen) is not on this machine")
    lib = env.mot.load_library(env.lib_path)
    poses, points = MG.cases(3000)
    want = MG.run_driver(poses, points)
    for k, (pose, pts) in enumerate(zip(poses, points)):
        got = ST._apply(ST.matrix_inv(lib, *pose), pts)
        assert np.array_equal(got.view(np.uint32), want[k].view(np.uint32)), (k, pose)


def test_emu_fixture_is_what_the_generator_records():
    """tests/golden/tf_to_sensor.npz = the first 64 of those cases, as the driver answers them today"""
    import golden_util as G
    import make_tf_sensor_golden as MG
    if not MG.have_reference():
        pytest.skip("the reference tree (its vendored Eigen) is not on this machine")
    fx = G.load("tf_to_sensor.npz")
    poses, points = MG.cases(64)
    assert np.array_equal(fx["pose"], poses) and np.array_equal(fx["points"].view(np.uint32), points.view(np.uint32))
    assert np.array_equal(fx["sensor"].view(np.uint32), MG.run_driver(poses, points).view(np.uint32))


def test_emu_matrix_against_golden_fixture(env):
    ST.matrix_against_fixture(env)


def test_emu_export_sensor(state):
    ST.export_sensor(state)


def test_emu_export_global_is_the_existing_call(state):
    ST.export_global(state)


def test_emu_round_trip(state):
    ST.round_trip(state)


def test_emu_node_frame_equals_the_stage_wise_sequence(env):
    ST.node_frame_equals_the_stage_wise_sequence(env)


def test_emu_node_frame_dropped_births(env):
    ST.node_frame_equals_the_stage_wise_sequence(env, max_tracks_total=3, expect_capacity=True)


def test_emu_node_frame_leaves_the_box_stage_alone(env):
    ST.node_frame_leaves_the_box_stage_alone(env)


def test_emu_python_layer(env):
    ST.python_layer(env)


def test_emu_sensor_kernels_are_launched_by_the_sensor_frame_only(state, env):
    """MOT_FRAME_GLOBAL goes to the existing kernels, MOT_FRAME_SENSOR to the new ones (the emulator counts launches per kernel name)"""
    lib = env.mot.load_library(env.lib_path)
    names = (b"export_tracks_kernel", b"export_tracks_packed_kernel", b"export_tracks_sensor_kernel", b"export_tracks_packed_sensor_kernel")
    count = lambda: [lib.hipemu_launch_count(n) for n in names]
    c0 = count()
    state.fixed(ST.GLOBAL, 8); state.packed(ST.GLOBAL, 8); state.fetched(ST.GLOBAL, 8)
    c1 = count()
    assert [b - a for a, b in zip(c0, c1)] == [2, 1, 0, 0]
    state.fixed(ST.SENSOR, 8); state.packed(ST.SENSOR, 8); state.fetched(ST.SENSOR, 8)
    assert [b - a for a, b in zip(c1, count())] == [0, 0, 2, 1]
