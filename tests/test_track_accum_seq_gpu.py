"""A recorded drive into the per-track accumulators (tests/track_accum_seq_cases.py) on the MI355X: mot_sequence_accumulate_dev against a second context driven
frame by frame (frames_dev batch 1 + accumulate_track_points), bit for bit. tests/test_emu_track_accum_seq.py runs the same bodies on the emulator."""
import pytest

import capacity_cases as CC
import track_accum_seq_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(mot, hip_lib):
    import hiprt

    def upload(host):
        d = hiprt.DeviceBuffer(host)
        return d.ptr, d
    return CC.Env(mot, None, upload)


@pytest.mark.parametrize("K,O", [(1024, 4), (256, 4), (64, 4), (256, 0)])
def test_moving_objects_in_one_call(env, oracle, K, O):
    SC.moving_objects(env, oracle, K, O)


def test_slot_reuse_inside_the_call(env, oracle):
    SC.slot_reuse(env, oracle)


def test_chained_calls(env, oracle):
    SC.chained_calls(env, oracle)


@pytest.mark.parametrize("order_any", [False, True])
@pytest.mark.parametrize("K", [64, 4096])
def test_chunk_and_tile_edges_many_segments(env, oracle, K, order_any):
    SC.shapes(env, oracle, K, order_any=order_any)


def test_one_track_two_boxes(env, oracle):
    SC.one_track_two_boxes(env, oracle)


def test_contract_state_and_arguments(env, oracle):
    SC.contract_state_and_arguments(env, oracle)


def test_contract_refused_frame(env, oracle):
    SC.contract_refused_frame(env, oracle)


@pytest.mark.parametrize("order_any", [False, True])
def test_non_interference(env, oracle, order_any):
    SC.non_interference(env, oracle, order_any=order_any)
