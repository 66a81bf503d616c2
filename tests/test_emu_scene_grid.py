"""Rolling static-scene grid (tests/scene_grid_cases.py) on the emulator: the kernels of csrc/scene_grid.hip and the host layer around them (csrc/mot_api_scene.hip).
The same bodies run on the MI355X in tests/test_scene_grid_gpu.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import capacity_cases as CC
import scene_grid_cases as SG


@pytest.fixture(scope="module")
def env(mot):
    import build_emu
    return CC.Env(mot, build_emu.build())


@pytest.mark.parametrize("cell,W", [(0.5, 64), (0.25, 64)])
def test_emu_standing_and_moving_objects(env, oracle, cell, W):
    SG.standing_and_moving(env, oracle, cell, W)


def test_emu_scroll(env, oracle):
    SG.scroll(env, oracle)


@pytest.mark.parametrize("order_any", [False, True])
def test_emu_chunk_and_wave_edges(env, oracle, order_any):
    SG.shapes(env, oracle, order_any=order_any)


def test_emu_contention(env, oracle):
    SG.contention(env, oracle)


def test_emu_contract_modes_and_arguments(env, oracle):
    SG.contract_modes(env, oracle)


def test_emu_contract_resets(env, oracle):
    SG.contract_resets(env, oracle)


@pytest.mark.parametrize("order_any", [False, True])
def test_emu_non_interference(env, oracle, order_any):
    SG.non_interference(env, oracle, order_any=order_any)


def test_emu_non_interference_with_launch_graphs(env, oracle):
    SG.non_interference(env, oracle, graphs=True)


def test_emu_determinism(env, oracle):
    SG.determinism(env, oracle)


def test_emu_plain_splat_gives_the_same_bytes(env, oracle):
    """the splat kernel without run merging (-DMOT_SCENE_MERGE=0, what tools/time_scene_grid.py times it against) against the product form"""
    import build_emu
    SG.determinism(env, oracle, other_lib_path=build_emu.build(defines=("-DMOT_SCENE_MERGE=0",)))


def test_emu_kernels_launched_only_by_the_new_calls(env, oracle):
    SG.launches_only_in_the_new_calls(env, oracle)


def test_emu_setter_under_allocation_failure(env, oracle):
    SG.setter_under_allocation_failure(env, oracle)
