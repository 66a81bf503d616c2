"""Voxel maps merged into one (tests/voxel_merge_cases.py) on the emulator: the kernels of csrc/voxel_merge.hip, the sort of csrc/mot_sort.h and the host layer
around them (csrc/mot_api_scene.hip). The same bodies run on the MI355X in tests/test_voxel_merge_gpu.py. The emulator's other thread orders (MOT_EMU_SCHED=rev,
rand:<seed>, tests/README.md) apply to this file as to every test_emu_*.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import capacity_cases as CC
import voxel_merge_cases as VM


@pytest.fixture(scope="module")
def env(mot):
    import build_emu
    return CC.Env(mot, build_emu.build())


def test_emu_sizes(env, oracle):
    VM.sizes(env, oracle)


def test_emu_runs(env, oracle):
    VM.runs(env, oracle)


def test_emu_key_digits(env, oracle):
    VM.key_digits(env, oracle)


def test_emu_lattice_edges(env, oracle):
    VM.lattice_edges(env, oracle)


def test_emu_weights(env, oracle):
    VM.weights(env, oracle)


def test_emu_identity(env, oracle):
    VM.identity(env, oracle)


def test_emu_capacities(env, oracle):
    VM.capacities(env, oracle)


def test_emu_contract(env, oracle):
    VM.contract(env, oracle)


def test_emu_order_of_maps(env, oracle):
    VM.order_of_maps(env, oracle)


def test_emu_chain_on_device(env, oracle):
    VM.chain_on_device(env, oracle)


def test_emu_kernels_launched_only_by_the_new_calls(env, oracle):
    VM.launches_only_in_the_new_calls(env, oracle)


def test_emu_scratch_under_allocation_failure(env, oracle):
    VM.scratch_under_allocation_failure(env, oracle)
