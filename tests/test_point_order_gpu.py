"""MOT_ORDER_ANY (tests/point_order_cases.py) on the MI355X: the box stage on the cluster-ordered copy that csrc/regroup.hip makes, bit for bit against
the oracle (the reference build answers first). tests/test_emu_point_order.py runs the same bodies on the emulator."""
import pytest

import capacity_cases as CC
import point_order_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(mot, hip_lib):
    import hiprt

    def upload(host):
        d = hiprt.DeviceBuffer(host)
        return d.ptr, d
    return CC.Env(mot, None, upload)


def test_refused_today_exact_with_the_mode(env, oracle):
    PC.refused_today_exact_with_the_mode(env, oracle)


def test_small_context_tiny_clusters(env, oracle):
    PC.small_context_tiny_clusters(env, oracle)


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("outputs", [0, PC.OUT_LABELS])
def test_fused_path(env, oracle, outputs, graphs):
    PC.fused_path(env, oracle, outputs, graphs)


def test_sequence_mode(env, oracle):
    PC.sequence_mode(env, oracle)


def test_stability(env, oracle):
    PC.stability(env, oracle)


def test_same_answer_where_both_modes_answer(env, oracle, synth):
    PC.same_answer_where_both_answer(env, oracle, synth)


def test_sort_edges(env, oracle):
    PC.sort_edges(env, oracle)


def test_switching(env, oracle):
    PC.switching(env, oracle)


def test_time_stage_in_the_mode(env, oracle):
    PC.time_stage_in_the_mode(env, oracle)
