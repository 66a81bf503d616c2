"""Voxel-thinned object models (tests/track_voxel_cases.py) on the emulator: the kernels of csrc/track_voxels.hip and the host layer around them. The same bodies
run on the MI355X in tests/test_track_voxels_gpu.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import capacity_cases as CC
import track_model_cases as MC
import track_voxel_cases as VC


@pytest.fixture(scope="module")
def env(mot):
    import build_emu
    return CC.Env(mot, build_emu.build())


@pytest.mark.parametrize("axes,current", MC.FLAGS)
@pytest.mark.parametrize("K,O", [(64, 4), (64, 16), (256, 4), (256, 16), (1024, 4), (1024, 16)])
def test_emu_moving_objects(env, oracle, K, O, axes, current):
    VC.moving_objects(env, oracle, K, O, axes, current)


def test_emu_one_voxel_per_model(env, oracle):
    VC.one_voxel_per_model(env, oracle)


def test_emu_every_record_alone_and_off_the_lattice(env, oracle):
    VC.every_record_alone(env, oracle)


@pytest.mark.parametrize("K", [64, 4096])
def test_emu_sort_sizes(env, oracle, K):
    VC.sort_sizes(env, oracle, K)


def test_emu_min_points(env, oracle):
    VC.min_points(env, oracle)


def test_emu_truncation(env, oracle):
    VC.truncation(env, oracle)


def test_emu_non_finite_pose(env, oracle):
    VC.non_finite_pose(env, oracle)


def test_emu_slot_reuse(env, oracle):
    VC.slot_reuse(env, oracle)


def test_emu_after_a_sequence_call(env, oracle):
    VC.after_sequence(env, oracle)


def test_emu_contract(env, oracle):
    VC.contract(env, oracle)


def test_emu_non_interference(env, oracle):
    VC.non_interference(env, oracle)


def test_emu_non_interference_with_launch_graphs(env, oracle):
    VC.non_interference(env, oracle, graphs=True)


def test_emu_lifecycle(env, oracle):
    VC.lifecycle(env, oracle)


def test_emu_first_call_under_allocation_failure(env, oracle):
    VC.first_call_under_allocation_failure(env, oracle)
