"""Object-centred track models (tests/track_model_cases.py) on the emulator: the kernels of csrc/track_models.hip and the host layer around them. The same bodies
run on the MI355X in tests/test_track_models_gpu.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import capacity_cases as CC
import track_model_cases as MC


@pytest.fixture(scope="module")
def env(mot):
    import build_emu
    return CC.Env(mot, build_emu.build())


@pytest.mark.parametrize("axes,current", MC.FLAGS)
@pytest.mark.parametrize("K,O", [(1024, 4), (256, 4), (64, 4), (256, 16), (1024, 1)])
def test_emu_moving_objects(env, oracle, K, O, axes, current):
    MC.moving_objects(env, oracle, K, O, axes, current)


@pytest.mark.parametrize("order_any", [False, True])
@pytest.mark.parametrize("K", [64, 4096])
def test_emu_many_rows_and_tile_edges(env, oracle, K, order_any):
    MC.many_rows(env, oracle, K, order_any=order_any)


def test_emu_log_longer_than_the_lds_tile(env, oracle):
    MC.long_log(env, oracle)


def test_emu_slot_reuse(env, oracle):
    MC.slot_reuse(env, oracle)


def test_emu_truncation(env, oracle):
    MC.truncation(env, oracle)


def test_emu_contract(env, oracle):
    MC.contract(env, oracle)


def test_emu_non_finite_pose(env, oracle):
    MC.non_finite_pose(env, oracle)


def test_emu_non_interference(env, oracle):
    MC.non_interference(env, oracle)


def test_emu_non_interference_with_launch_graphs(env, oracle):
    MC.non_interference(env, oracle, graphs=True)


def test_emu_launches_and_allocations(env, oracle):
    MC.launches_and_allocations(env, oracle)


def test_emu_first_call_under_allocation_failure(env, oracle):
    MC.first_call_under_allocation_failure(env, oracle)
