"""A recorded drive's points judged against the grid the drive left (tests/scene_judge_seq_cases.py) on the emulator: the kernels of csrc/scene_judge_seq.hip and the host
layer around them (csrc/mot_api_scene.hip). The same bodies run on the MI355X in tests/test_scene_judge_seq_gpu.py. The emulator's other thread orders
(MOT_EMU_SCHED=rev, rand:<seed>, tests/README.md) apply to this file as to every test_emu_*.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import capacity_cases as CC
import scene_judge_seq_cases as SJQ


@pytest.fixture(scope="module")
def env(mot):
    import build_emu
    return CC.Env(mot, build_emu.build())


@pytest.mark.parametrize("cell", [0.26, 0.27])
def test_emu_a_drive_and_its_last_frame_against_the_existing_path(env, oracle, cell):
    SJQ.a_drive(env, oracle, cell)


@pytest.mark.parametrize("order_any", [False, True])
def test_emu_chunk_tile_and_wave_edges(env, oracle, order_any):
    SJQ.shapes(env, oracle, order_any=order_any)


@pytest.mark.parametrize("frames", [1, 2, 256, 257])
def test_emu_frame_counts(env, oracle, frames):
    SJQ.frame_counts(env, oracle, frames)


def test_emu_refused_frame(env, oracle):
    SJQ.refused_frame(env, oracle)


@pytest.mark.parametrize("kind", ["jump", "invalid_middle", "invalid_last"])
def test_emu_windows(env, oracle, kind):
    SJQ.windows(env, oracle, kind)


def test_emu_chained_calls(env, oracle):
    SJQ.chained(env, oracle)


def test_emu_helper_cuts_a_drive_into_pieces(env, oracle):
    SJQ.helper_pieces(env, oracle)


def test_emu_contract(env, oracle):
    SJQ.contract(env, oracle)


@pytest.mark.parametrize("order_any", [False, True])
def test_emu_non_interference(env, oracle, order_any):
    SJQ.non_interference(env, oracle, order_any=order_any)


def test_emu_determinism(env, oracle):
    SJQ.determinism(env, oracle)


def test_emu_kernels_launched_only_by_the_new_calls(env, oracle):
    SJQ.launches_only_in_the_new_calls(env, oracle)


def test_emu_scratch_under_allocation_failure(env, oracle):
    SJQ.scratch_under_allocation_failure(env, oracle)
