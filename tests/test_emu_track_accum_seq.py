"""A recorded drive into the per-track accumulators (tests/track_accum_seq_cases.py) on the emulator: the kernels of csrc/track_accum_seq.hip and the host layer
around them, against the frame-by-frame path. The same bodies run on the MI355X in tests/test_track_accum_seq_gpu.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import capacity_cases as CC
import track_accum_seq_cases as SC


@pytest.fixture(scope="module")
def env(mot):
    import build_emu
    return CC.Env(mot, build_emu.build())


@pytest.mark.parametrize("K,O", [(1024, 4), (256, 4), (64, 4), (256, 0)])
def test_emu_moving_objects_in_one_call(env, oracle, K, O):
    SC.moving_objects(env, oracle, K, O)


def test_emu_slot_reuse_inside_the_call(env, oracle):
    SC.slot_reuse(env, oracle)


def test_emu_chained_calls(env, oracle):
    SC.chained_calls(env, oracle)


@pytest.mark.parametrize("order_any", [False, True])
@pytest.mark.parametrize("K", [64, 4096])
def test_emu_chunk_and_tile_edges_many_segments(env, oracle, K, order_any):
    SC.shapes(env, oracle, K, order_any=order_any)


def test_emu_one_track_two_boxes(env, oracle):
    SC.one_track_two_boxes(env, oracle)


def test_emu_contract_state_and_arguments(env, oracle):
    SC.contract_state_and_arguments(env, oracle)


def test_emu_contract_refused_frame(env, oracle):
    SC.contract_refused_frame(env, oracle)


@pytest.mark.parametrize("order_any", [False, True])
def test_emu_non_interference(env, oracle, order_any):
    SC.non_interference(env, oracle, order_any=order_any)


def test_emu_launches_and_allocations(env, oracle):
    SC.launches_and_allocations(env, oracle)
