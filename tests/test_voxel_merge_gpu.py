"""Voxel maps merged into one (tests/voxel_merge_cases.py) on the MI355X, through the C-ABI: the kernels of csrc/voxel_merge.hip and the sort of csrc/mot_sort.h
against a numpy model of include/mot.h, byte for byte. tests/test_emu_voxel_merge.py runs the same bodies on the emulator."""
import pytest

import capacity_cases as CC
import voxel_merge_cases as VM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(mot, hip_lib):
    import hiprt

    def upload(host):
        d = hiprt.DeviceBuffer(host)
        return d.ptr, d
    return CC.Env(mot, None, upload)


def test_sizes(env, oracle):
    VM.sizes(env, oracle)


def test_runs(env, oracle):
    VM.runs(env, oracle)


def test_key_digits(env, oracle):
    VM.key_digits(env, oracle)


def test_lattice_edges(env, oracle):
    VM.lattice_edges(env, oracle)


def test_weights(env, oracle):
    VM.weights(env, oracle)


def test_identity(env, oracle):
    VM.identity(env, oracle)


def test_capacities(env, oracle):
    VM.capacities(env, oracle)


def test_contract(env, oracle):
    VM.contract(env, oracle)


def test_order_of_maps(env, oracle):
    VM.order_of_maps(env, oracle)


def test_chain_on_device(env, oracle):
    VM.chain_on_device(env, oracle)
