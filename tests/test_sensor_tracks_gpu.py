"""Live tracks in the sensor frame (tests/sensor_track_cases.py) on the MI355X: export_tracks_sensor_kernel / export_tracks_packed_sensor_kernel of
csrc/track.hip and mot_tracking_node_frame, bit for bit; the global -> sensor matrix of the real library against the fixture recorded from the reference
node's own call sequence (tests/golden/tf_to_sensor.npz). tests/test_emu_sensor_tracks.py runs the same bodies on the emulator."""
import pytest

import capacity_cases as CC
import sensor_track_cases as ST

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(mot, hip_lib):
    import hiprt

    def upload(host):
        d = hiprt.DeviceBuffer(host)
        return d.ptr, d
    return CC.Env(mot, None, upload)


@pytest.fixture(scope="module")
def state(env):
    st = ST.State(env)
    yield st
    st.close()


def test_matrix_against_golden_fixture(env):
    ST.matrix_against_fixture(env)


def test_export_sensor(state):
    ST.export_sensor(state)


def test_export_global_is_the_existing_call(state):
    ST.export_global(state)


def test_round_trip(state):
    ST.round_trip(state)


def test_node_frame_equals_the_stage_wise_sequence(env):
    ST.node_frame_equals_the_stage_wise_sequence(env)


def test_node_frame_dropped_births(env):
    ST.node_frame_equals_the_stage_wise_sequence(env, max_tracks_total=3, expect_capacity=True)


def test_node_frame_leaves_the_box_stage_alone(env):
    ST.node_frame_leaves_the_box_stage_alone(env)


def test_python_layer(env):
    ST.python_layer(env)
