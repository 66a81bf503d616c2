"""A recorded drive's points judged against the grid the drive left (tests/scene_judge_seq_cases.py) on the MI355X, through the C-ABI: the kernels of
csrc/scene_judge_seq.hip against a numpy model built from a frame-by-frame context's older getters, byte for byte. tests/test_emu_scene_judge_seq.py runs the same
bodies on the emulator."""
import pytest

import capacity_cases as CC
import scene_judge_seq_cases as SJQ

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(mot, hip_lib):
    import hiprt

    def upload(host):
        d = hiprt.DeviceBuffer(host)
        return d.ptr, d
    return CC.Env(mot, None, upload)


@pytest.mark.parametrize("cell", [0.26, 0.27])
def test_a_drive_and_its_last_frame_against_the_existing_path(env, oracle, cell):
    SJQ.a_drive(env, oracle, cell)


@pytest.mark.parametrize("order_any", [False, True])
def test_chunk_tile_and_wave_edges(env, oracle, order_any):
    SJQ.shapes(env, oracle, order_any=order_any)


@pytest.mark.parametrize("frames", [1, 2, 256, 257])
def test_frame_counts(env, oracle, frames):
    SJQ.frame_counts(env, oracle, frames)


def test_refused_frame(env, oracle):
    SJQ.refused_frame(env, oracle)


@pytest.mark.parametrize("kind", ["jump", "invalid_middle", "invalid_last"])
def test_windows(env, oracle, kind):
    SJQ.windows(env, oracle, kind)


def test_chained_calls(env, oracle):
    SJQ.chained(env, oracle)


def test_helper_cuts_a_drive_into_pieces(env, oracle):
    SJQ.helper_pieces(env, oracle)


def test_contract(env, oracle):
    SJQ.contract(env, oracle)


@pytest.mark.parametrize("order_any", [False, True])
def test_non_interference(env, oracle, order_any):
    SJQ.non_interference(env, oracle, order_any=order_any)


def test_determinism(env, oracle):
    SJQ.determinism(env, oracle)
