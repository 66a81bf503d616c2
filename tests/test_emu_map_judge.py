"""Voxel maps indexed and a frame's points judged against the index (tests/map_judge_cases.py) on the emulator: the kernels of csrc/map_judge.hip, the index
kernel of csrc/voxel_merge.hip and the host layer around them (csrc/mot_api_scene.hip). The same bodies run on the MI355X in tests/test_map_judge_gpu.py. The
emulator's other thread orders (MOT_EMU_SCHED=rev, rand:<seed>, tests/README.md) apply to this file as to every test_emu_*.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import capacity_cases as CC
import map_judge_cases as MJ


@pytest.fixture(scope="module")
def env(mot):
    import build_emu
    return CC.Env(mot, build_emu.build())


def test_emu_index_sizes(env, oracle):
    MJ.index_sizes(env, oracle)


def test_emu_index_cells(env, oracle):
    MJ.index_cells(env, oracle)


def test_emu_index_capacities(env, oracle):
    MJ.index_capacities(env, oracle)


def test_emu_index_contract(env, oracle):
    MJ.index_contract(env, oracle)


def test_emu_shapes(env, oracle):
    MJ.shapes(env, oracle)


def test_emu_shapes_any_order(env, oracle):
    MJ.shapes(env, oracle, order_any=True)


def test_emu_index_lengths(env, oracle):
    MJ.index_lengths(env, oracle)


def test_emu_neighbours(env, oracle):
    MJ.neighbours(env, oracle)


def test_emu_lattice_edges(env, oracle):
    MJ.lattice_edges(env, oracle)


def test_emu_kinds_and_outside(env, oracle):
    MJ.kinds_and_outside(env, oracle)


def test_emu_closed_loop(env, oracle):
    MJ.closed_loop(env, oracle)


def test_emu_chain_on_device(env, oracle):
    MJ.chain_on_device(env, oracle)


def test_emu_play_against_map(env, oracle):
    MJ.play_against_map(env, oracle)


def test_emu_contract(env, oracle):
    MJ.contract(env, oracle)


def test_emu_determinism(env, oracle):
    MJ.determinism(env, oracle)


def test_emu_launches_only_in_the_new_calls(env, oracle):
    MJ.launches_only_in_the_new_calls(env, oracle)


def test_emu_scratch_under_allocation_failure(env, oracle):
    MJ.scratch_under_allocation_failure(env, oracle)
