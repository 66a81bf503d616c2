"""Per-track accumulators (tests/track_accum_cases.py) on the MI355X: the kernels of csrc/track_accum.hip against a Python model folded from the getters that
exist without them, bit for bit. tests/test_emu_track_accum.py runs the same bodies on the emulator."""
import pytest

import capacity_cases as CC
import track_accum_cases as AC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(mot, hip_lib):
    import hiprt

    def upload(host):
        d = hiprt.DeviceBuffer(host)
        return d.ptr, d
    return CC.Env(mot, None, upload)


@pytest.mark.parametrize("K,O", [(1024, 4), (256, 4), (64, 4), (256, 0)])
def test_moving_objects(env, oracle, K, O):
    AC.moving_objects(env, oracle, K, O)


@pytest.mark.parametrize("order_any", [False, True])
@pytest.mark.parametrize("K", [64, 4096])
def test_chunk_and_tile_edges_many_segments(env, oracle, K, order_any):
    AC.shapes(env, oracle, K, order_any=order_any)


def test_one_track_two_boxes(env, oracle):
    AC.one_track_two_boxes(env, oracle)


def test_slot_reuse(env, oracle):
    AC.slot_reuse(env, oracle)


def test_contract_modes_and_arguments(env, oracle):
    AC.contract_modes(env, oracle)


def test_contract_refused_frame(env, oracle):
    AC.contract_refused_frame(env, oracle)


def test_contract_resets(env, oracle):
    AC.contract_resets(env, oracle)


@pytest.mark.parametrize("order_any", [False, True])
def test_non_interference(env, oracle, order_any):
    AC.non_interference(env, oracle, order_any=order_any)


def test_non_interference_with_launch_graphs(env, oracle):
    AC.non_interference(env, oracle, graphs=True)
