"""MOT_ORDER_ANY (tests/point_order_cases.py) on the emulator: the regrouping kernels of csrc/regroup.hip and the host paths around them, every case
bit for bit against the oracle. The same bodies run on the MI355X in tests/test_point_order_gpu.py; the ROS and adapter settings are run in
tests/test_nodes_point_order.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import capacity_cases as CC
import point_order_cases as PC



@pytest.fixture(scope="module")
def env(mot):
    import build_emu
    return CC.Env(mot, build_emu.build())


def test_emu_refused_today_exact_with_the_mode(env, oracle):
    PC.refused_today_exact_with_the_mode(env, oracle)


def test_emu_small_context_tiny_clusters(env, oracle):
    PC.small_context_tiny_clusters(env, oracle)


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("outputs", [0, PC.OUT_LABELS])
def test_emu_fused_path(env, oracle, outputs, graphs):
    PC.fused_path(env, oracle, outputs, graphs)


def test_emu_sequence_mode(env, oracle):
    PC.sequence_mode(env, oracle)


def test_emu_stability(env, oracle):
    PC.stability(env, oracle)


def test_emu_same_answer_where_both_modes_answer(env, oracle, synth):
    PC.same_answer_where_both_answer(env, oracle, synth)


def test_emu_sort_edges(env, oracle):
    PC.sort_edges(env, oracle)


def test_emu_switching(env, oracle):
    PC.switching(env, oracle)


def test_emu_interface(env):
    PC.interface(env)


def test_emu_kernels_launched_only_in_the_mode(env, oracle):
    """the regrouping kernels run in MOT_ORDER_ANY and only there (the emulator counts launches per kernel name)"""
    lib = env.mot.load_library(env.lib_path)
    count = lambda: lib.hipemu_launch_count(b"regroup_gather_kernel")
    p = oracle.params(0)
    elev = CC.small_scene(0, 12)
    with env.context(0, max_points=4096) as c:
        before = count()
        c.cluster(elev); c.box_fit_resident()
        assert count() == before
        c.set_point_order(env.mot.MOT_ORDER_ANY)
        c.box_fit_resident()
        assert count() == before + 1


def test_emu_time_stage_in_the_mode(env, oracle):
    PC.time_stage_in_the_mode(env, oracle)
