"""Rolling static-scene grid (tests/scene_grid_cases.py) on the MI355X: the kernels of csrc/scene_grid.hip against a numpy model folded from the getters that exist
without them, byte for byte. tests/test_emu_scene_grid.py runs the same bodies on the emulator."""
import pytest

import capacity_cases as CC
import scene_grid_cases as SG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(mot, hip_lib):
    import hiprt

    def upload(host):
        d = hiprt.DeviceBuffer(host)
        return d.ptr, d
    return CC.Env(mot, None, upload)


@pytest.mark.parametrize("cell,W", [(0.5, 64), (0.25, 64)])
def test_standing_and_moving_objects(env, oracle, cell, W):
    SG.standing_and_moving(env, oracle, cell, W)


def test_scroll(env, oracle):
    SG.scroll(env, oracle)


@pytest.mark.parametrize("order_any", [False, True])
def test_chunk_and_wave_edges(env, oracle, order_any):
    SG.shapes(env, oracle, order_any=order_any)


def test_contention(env, oracle):
    SG.contention(env, oracle)


def test_contract_modes_and_arguments(env, oracle):
    SG.contract_modes(env, oracle)


def test_contract_resets(env, oracle):
    SG.contract_resets(env, oracle)


@pytest.mark.parametrize("order_any", [False, True])
def test_non_interference(env, oracle, order_any):
    SG.non_interference(env, oracle, order_any=order_any)


def test_non_interference_with_launch_graphs(env, oracle):
    SG.non_interference(env, oracle, graphs=True)


def test_determinism(env, oracle):
    SG.determinism(env, oracle)
