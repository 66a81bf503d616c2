"""Object-centred track models (tests/track_model_cases.py) on the MI355X: the kernels of csrc/track_models.hip against a numpy model built from the accumulator
getters that exist without them. tests/test_emu_track_models.py runs the same bodies on the emulator."""
import pytest

import capacity_cases as CC
import track_model_cases as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(mot, hip_lib):
    import hiprt

    def upload(host):
        d = hiprt.DeviceBuffer(host)
        return d.ptr, d
    return CC.Env(mot, None, upload)


@pytest.mark.parametrize("axes,current", MC.FLAGS)
@pytest.mark.parametrize("K,O", [(1024, 4), (256, 4), (64, 4), (256, 16), (1024, 1)])
def test_moving_objects(env, oracle, K, O, axes, current):
    MC.moving_objects(env, oracle, K, O, axes, current)


@pytest.mark.parametrize("order_any", [False, True])
@pytest.mark.parametrize("K", [64, 4096])
def test_many_rows_and_tile_edges(env, oracle, K, order_any):
    MC.many_rows(env, oracle, K, order_any=order_any)


def test_log_longer_than_the_lds_tile(env, oracle):
    MC.long_log(env, oracle)


def test_slot_reuse(env, oracle):
    MC.slot_reuse(env, oracle)


def test_truncation(env, oracle):
    MC.truncation(env, oracle)


def test_contract(env, oracle):
    MC.contract(env, oracle)


def test_non_finite_pose(env, oracle):
    MC.non_finite_pose(env, oracle)


def test_non_interference(env, oracle):
    MC.non_interference(env, oracle)


def test_non_interference_with_launch_graphs(env, oracle):
    MC.non_interference(env, oracle, graphs=True)
