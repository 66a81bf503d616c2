"""A frame's points judged against the scene grid (tests/scene_judge_cases.py) on the emulator: the kernels of csrc/scene_judge.hip and the host layer around them
(csrc/mot_api_scene.hip). The same bodies run on the MI355X in tests/test_scene_judge_gpu.py. The emulator's other thread orders (MOT_EMU_SCHED=rev, rand:<seed>,
tests/README.md) apply to this file as to every test_emu_*.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import capacity_cases as CC
import scene_judge_cases as SJ


@pytest.fixture(scope="module")
def env(mot):
    import build_emu
    return CC.Env(mot, build_emu.build())


@pytest.mark.parametrize("cell,W", [(0.5, 64), (0.25, 64)])
def test_emu_standing_and_moving_objects(env, oracle, cell, W):
    SJ.standing_and_moving(env, oracle, cell, W)


@pytest.mark.parametrize("order_any", [False, True])
def test_emu_chunk_tile_and_wave_edges(env, oracle, order_any):
    SJ.shapes(env, oracle, order_any=order_any)


def test_emu_threshold_edges(env, oracle):
    SJ.thresholds(env, oracle)


def test_emu_scroll(env, oracle):
    SJ.scroll(env, oracle)


def test_emu_contract(env, oracle):
    SJ.contract(env, oracle)


@pytest.mark.parametrize("order_any", [False, True])
def test_emu_non_interference(env, oracle, order_any):
    SJ.non_interference(env, oracle, order_any=order_any)


def test_emu_non_interference_with_launch_graphs(env, oracle):
    SJ.non_interference(env, oracle, graphs=True)


def test_emu_determinism(env, oracle):
    SJ.determinism(env, oracle)


def test_emu_kernels_launched_only_by_the_new_calls(env, oracle):
    SJ.launches_only_in_the_new_calls(env, oracle)


def test_emu_scratch_under_allocation_failure(env, oracle):
    SJ.scratch_under_allocation_failure(env, oracle)
