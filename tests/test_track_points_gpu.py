"""Per-track point clouds (tests/track_point_cases.py) on the MI355X: the four kernels of csrc/track_points.hip against the numpy composition of the getters that
exist without them, bit for bit. tests/test_emu_track_points.py runs the same bodies on the emulator."""
import pytest

import capacity_cases as CC
import track_point_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(mot, hip_lib):
    import hiprt

    def upload(host):
        d = hiprt.DeviceBuffer(host)
        return d.ptr, d
    return CC.Env(mot, None, upload)


def test_shapes_and_many_segments(env, oracle):
    PC.shapes(env, oracle)


def test_one_track_two_boxes(env, oracle):
    PC.one_track_two_boxes(env, oracle)


def test_order_any(env, oracle):
    PC.order_any(env, oracle)


def test_global_frame(env, oracle):
    PC.global_frame(env, oracle)


def test_global_frame_sequence(env, oracle):
    PC.global_frame_sequence(env, oracle)


def test_truncation(env, oracle):
    PC.truncation(env, oracle)


def test_contract_state_and_arguments(env, oracle):
    PC.contract_state(env, oracle)


def test_contract_refused_frame(env, oracle):
    PC.contract_refused(env, oracle)


@pytest.mark.parametrize("order_any", [False, True])
def test_non_interference(env, oracle, order_any):
    PC.non_interference(env, oracle, order_any=order_any)


def test_non_interference_with_launch_graphs(env, oracle):
    PC.non_interference(env, oracle, graphs=True)
