"""Voxel maps indexed and a frame's points judged against the index (tests/map_judge_cases.py) on the MI355X, through the C-ABI: the kernels of
csrc/map_judge.hip and the index kernel of csrc/voxel_merge.hip against a numpy model of include/mot.h, byte for byte. tests/test_emu_map_judge.py runs the same
bodies on the emulator."""
import pytest

import capacity_cases as CC
import map_judge_cases as MJ

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(mot, hip_lib):
    import hiprt

    def upload(host):
        d = hiprt.DeviceBuffer(host)
        return d.ptr, d
    return CC.Env(mot, None, upload)


def test_index_sizes(env, oracle):
    MJ.index_sizes(env, oracle)


def test_index_cells(env, oracle):
    MJ.index_cells(env, oracle)


def test_index_capacities(env, oracle):
    MJ.index_capacities(env, oracle)


def test_index_contract(env, oracle):
    MJ.index_contract(env, oracle)


def test_shapes(env, oracle):
    MJ.shapes(env, oracle)


def test_shapes_any_order(env, oracle):
    MJ.shapes(env, oracle, order_any=True)


def test_index_lengths(env, oracle):
    MJ.index_lengths(env, oracle)


def test_neighbours(env, oracle):
    MJ.neighbours(env, oracle)


def test_lattice_edges(env, oracle):
    MJ.lattice_edges(env, oracle)


def test_kinds_and_outside(env, oracle):
    MJ.kinds_and_outside(env, oracle)


def test_closed_loop(env, oracle):
    MJ.closed_loop(env, oracle)


def test_chain_on_device(env, oracle):
    MJ.chain_on_device(env, oracle)


def test_play_against_map(env, oracle):
    MJ.play_against_map(env, oracle)


def test_contract(env, oracle):
    MJ.contract(env, oracle)


def test_determinism(env, oracle):
    MJ.determinism(env, oracle)
