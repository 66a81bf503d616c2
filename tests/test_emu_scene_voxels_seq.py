"""The voxel-thinned static map of a recorded drive (tests/scene_voxel_seq_cases.py) on the emulator: the kernels of csrc/scene_voxels_seq.hip, the sort of
csrc/mot_sort.h and the host layer around them (csrc/mot_api_scene.hip). The same bodies run on the MI355X in tests/test_scene_voxels_seq_gpu.py. The emulator's other
thread orders (MOT_EMU_SCHED=rev, rand:<seed>, tests/README.md) apply to this file as to every test_emu_*.py: they are what pins the sort's stability."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import capacity_cases as CC
import scene_voxel_seq_cases as SV


@pytest.fixture(scope="module")
def env(mot):
    import build_emu
    return CC.Env(mot, build_emu.build())


def test_emu_sizes(env, oracle):
    SV.sizes(env, oracle)


def test_emu_runs(env, oracle):
    SV.runs(env, oracle)


def test_emu_key_digits(env, oracle):
    SV.key_digits(env, oracle)


def test_emu_lattice_edges(env, oracle):
    SV.lattice_edges(env, oracle)


def test_emu_capacities(env, oracle):
    SV.capacities(env, oracle)


def test_emu_contract(env, oracle):
    SV.contract(env, oracle)


def test_emu_non_interference(env, oracle):
    SV.non_interference(env, oracle)


def test_emu_determinism(env, oracle):
    SV.determinism(env, oracle)


def test_emu_helper_thins_every_piece(env, oracle):
    SV.helper_pieces(env, oracle)


def test_emu_kernels_launched_only_by_the_new_calls(env, oracle):
    SV.launches_only_in_the_new_calls(env, oracle)


def test_emu_scratch_under_allocation_failure(env, oracle):
    SV.scratch_under_allocation_failure(env, oracle)
