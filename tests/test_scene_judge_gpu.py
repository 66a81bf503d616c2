"""A frame's points judged against the scene grid (tests/scene_judge_cases.py) on the MI355X: the kernels of csrc/scene_judge.hip against a numpy model built from
the getters that exist without them, byte for byte. tests/test_emu_scene_judge.py runs the same bodies on the emulator."""
import pytest

import capacity_cases as CC
import scene_judge_cases as SJ

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
    SJ.standing_and_moving(env, oracle, cell, W)


@pytest.mark.parametrize("order_any", [False, True])
def test_chunk_tile_and_wave_edges(env, oracle, order_any):
    SJ.shapes(env, oracle, order_any=order_any)


def test_threshold_edges(env, oracle):
    SJ.thresholds(env, oracle)


def test_scroll(env, oracle):
    SJ.scroll(env, oracle)


def test_contract(env, oracle):
    SJ.contract(env, oracle)


@pytest.mark.parametrize("order_any", [False, True])
def test_non_interference(env, oracle, order_any):
    SJ.non_interference(env, oracle, order_any=order_any)


def test_non_interference_with_launch_graphs(env, oracle):
    SJ.non_interference(env, oracle, graphs=True)


def test_determinism(env, oracle):
    SJ.determinism(env, oracle)
