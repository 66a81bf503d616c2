"""Per-track point clouds (tests/track_point_cases.py) on the emulator: the four kernels of csrc/track_points.hip and the host layer around them. The same bodies
run on the MI355X in tests/test_track_points_gpu.py; the life cycle of the feature's allocations is in tests/test_emu_track_points_lifecycle.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import capacity_cases as CC
import track_point_cases as PC


@pytest.fixture(scope="module")
def env(mot):
    import build_emu
    return CC.Env(mot, build_emu.build())


def test_emu_shapes_and_many_segments(env, oracle):
    PC.shapes(env, oracle)


def test_emu_one_track_two_boxes(env, oracle):
    PC.one_track_two_boxes(env, oracle)


def test_emu_order_any(env, oracle):
    PC.order_any(env, oracle)


def test_emu_global_frame(env, oracle):
    PC.global_frame(env, oracle)


def test_emu_global_frame_sequence(env, oracle):
    PC.global_frame_sequence(env, oracle)


def test_emu_truncation(env, oracle):
    PC.truncation(env, oracle)


def test_emu_kernels_launched_only_by_the_export(env, oracle):
    PC.launches_only_in_the_export(env, oracle)


def test_emu_contract_state_and_arguments(env, oracle):
    PC.contract_state(env, oracle)


def test_emu_contract_refused_frame(env, oracle):
    PC.contract_refused(env, oracle)


@pytest.mark.parametrize("order_any", [False, True])
def test_emu_non_interference(env, oracle, order_any):
    PC.non_interference(env, oracle, order_any=order_any)


def test_emu_non_interference_with_launch_graphs(env, oracle):
    PC.non_interference(env, oracle, graphs=True)
