"""The voxel-thinned static map of a recorded drive (tests/scene_voxel_seq_cases.py) on the MI355X, through the C-ABI: the kernels of csrc/scene_voxels_seq.hip and
the sort of csrc/mot_sort.h against a numpy model built from the older getter's records, byte for byte. tests/test_emu_scene_voxels_seq.py runs the same bodies on
the emulator."""
import pytest

import capacity_cases as CC
import scene_voxel_seq_cases as SV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(mot, hip_lib):
    import hiprt

    def upload(host):
        d = hiprt.DeviceBuffer(host)
        return d.ptr, d
    return CC.Env(mot, None, upload)


def test_sizes(env, oracle):
    SV.sizes(env, oracle)


def test_runs(env, oracle):
    SV.runs(env, oracle)


def test_key_digits(env, oracle):
    SV.key_digits(env, oracle)


def test_lattice_edges(env, oracle):
    SV.lattice_edges(env, oracle)


def test_capacities(env, oracle):
    SV.capacities(env, oracle)


def test_contract(env, oracle):
    SV.contract(env, oracle)


def test_non_interference(env, oracle):
    SV.non_interference(env, oracle)


def test_determinism(env, oracle):
    SV.determinism(env, oracle)


def test_helper_thins_every_piece(env, oracle):
    SV.helper_pieces(env, oracle)
