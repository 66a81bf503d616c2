"""A recorded drive into the static-scene grid (tests/scene_grid_seq_cases.py) on the emulator: the kernels of csrc/scene_grid_seq.hip and the host layer around them
(csrc/mot_api_scene.hip, mot_sequence_products_dev in csrc/mot_api.hip). The same bodies run on the MI355X in tests/test_scene_grid_seq_gpu.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import capacity_cases as CC
import scene_grid_seq_cases as SS


@pytest.fixture(scope="module")
def env(mot):
    import build_emu
    return CC.Env(mot, build_emu.build())


@pytest.mark.parametrize("cell,W", [(0.5, 64), (0.25, 64)])
def test_emu_a_drive_in_one_call(env, oracle, cell, W):
    SS.a_drive(env, oracle, cell, W)


def test_emu_slot_reuse_inside_the_call(env, oracle):
    SS.slot_reuse(env, oracle)


@pytest.mark.parametrize("invalid_last", [False, True])
def test_emu_scroll_inside_one_call(env, oracle, invalid_last):
    SS.scroll(env, oracle, invalid_last=invalid_last)


def test_emu_chained_calls(env, oracle):
    SS.chained(env, oracle)


@pytest.mark.parametrize("order_any", [False, True])
def test_emu_chunk_and_wave_edges(env, oracle, order_any):
    SS.shapes(env, oracle, order_any=order_any)


@pytest.mark.parametrize("cells_n", [1, 2])
def test_emu_contention_across_frames(env, oracle, cells_n):
    SS.contention(env, oracle, cells_n)


def test_emu_refused_frame_in_the_middle(env, oracle):
    SS.refused_frame(env, oracle)


def test_emu_products(env, oracle):
    SS.products(env, oracle)


def test_emu_contract(env, oracle):
    SS.contract(env, oracle)


@pytest.mark.parametrize("order_any", [False, True])
def test_emu_non_interference(env, oracle, order_any):
    SS.non_interference(env, oracle, order_any=order_any)


def test_emu_determinism(env, oracle):
    SS.determinism(env, oracle)


def test_emu_plain_splat_gives_the_same_bytes(env, oracle):
    """the splat kernels without run merging (-DMOT_SCENE_MERGE=0) against the product form"""
    import build_emu
    SS.determinism(env, oracle, other_lib_path=build_emu.build(defines=("-DMOT_SCENE_MERGE=0",)))


def test_emu_launches_and_allocations(env, oracle):
    SS.launches_and_allocations(env, oracle)
