"""A recorded drive into the static-scene grid (tests/scene_grid_seq_cases.py) on the MI355X: mot_sequence_products_dev with MOT_SEQ_SCENE against the frame-by-frame
route (frames_dev batch 1 + accumulate_scene), byte for byte. tests/test_emu_scene_grid_seq.py runs the same bodies on the emulator."""
import pytest

import capacity_cases as CC
import scene_grid_seq_cases as SS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(mot, hip_lib):
    import hiprt

    def upload(host):
        d = hiprt.DeviceBuffer(host)
        return d.ptr, d
    return CC.Env(mot, None, upload)


@pytest.mark.parametrize("cell,W", [(0.5, 64), (0.25, 64)])
def test_a_drive_in_one_call(env, oracle, cell, W):
    SS.a_drive(env, oracle, cell, W)


def test_slot_reuse_inside_the_call(env, oracle):
    SS.slot_reuse(env, oracle)


@pytest.mark.parametrize("invalid_last", [False, True])
def test_scroll_inside_one_call(env, oracle, invalid_last):
    SS.scroll(env, oracle, invalid_last=invalid_last)


def test_chained_calls(env, oracle):
    SS.chained(env, oracle)


@pytest.mark.parametrize("order_any", [False, True])
def test_chunk_and_wave_edges(env, oracle, order_any):
    SS.shapes(env, oracle, order_any=order_any)


@pytest.mark.parametrize("cells_n", [1, 2])
def test_contention_across_frames(env, oracle, cells_n):
    SS.contention(env, oracle, cells_n)


def test_refused_frame_in_the_middle(env, oracle):
    SS.refused_frame(env, oracle)


def test_products(env, oracle):
    SS.products(env, oracle)


def test_contract(env, oracle):
    SS.contract(env, oracle)


@pytest.mark.parametrize("order_any", [False, True])
def test_non_interference(env, oracle, order_any):
    SS.non_interference(env, oracle, order_any=order_any)


def test_determinism(env, oracle):
    SS.determinism(env, oracle)
