"""Per-track accumulators (tests/track_accum_cases.py) on the emulator: the kernels of csrc/track_accum.hip and the host layer around them. The same bodies run on
the MI355X in tests/test_track_accum_gpu.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import capacity_cases as CC
import track_accum_cases as AC


@pytest.fixture(scope="module")
def env(mot):
    import build_emu
    return CC.Env(mot, build_emu.build())


@pytest.mark.parametrize("K,O", [(1024, 4), (256, 4), (64, 4), (256, 0)])
def test_emu_moving_objects(env, oracle, K, O):
    AC.moving_objects(env, oracle, K, O)


@pytest.mark.parametrize("order_any", [False, True])
@pytest.mark.parametrize("K", [64, 4096])
def test_emu_chunk_and_tile_edges_many_segments(env, oracle, K, order_any):
    AC.shapes(env, oracle, K, order_any=order_any)


def test_emu_one_track_two_boxes(env, oracle):
    AC.one_track_two_boxes(env, oracle)


def test_emu_slot_reuse(env, oracle):
    AC.slot_reuse(env, oracle)


def test_emu_contract_modes_and_arguments(env, oracle):
    AC.contract_modes(env, oracle)


def test_emu_contract_refused_frame(env, oracle):
    AC.contract_refused_frame(env, oracle)


def test_emu_contract_resets(env, oracle):
    AC.contract_resets(env, oracle)


@pytest.mark.parametrize("order_any", [False, True])
def test_emu_non_interference(env, oracle, order_any):
    AC.non_interference(env, oracle, order_any=order_any)


def test_emu_non_interference_with_launch_graphs(env, oracle):
    AC.non_interference(env, oracle, graphs=True)


def test_emu_kernels_launched_only_by_the_accumulate(env, oracle):
    AC.launches_only_in_the_accumulate(env, oracle)


def test_emu_setter_under_allocation_failure(env, oracle):
    AC.setter_under_allocation_failure(env, oracle)
