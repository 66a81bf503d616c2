"""Voxel-thinned object models (tests/track_voxel_cases.py) on the MI355X: the kernels of csrc/track_voxels.hip against numpy applied to the raw models the
library gives without them. tests/test_emu_track_voxels.py runs the same bodies on the emulator."""
import pytest

import capacity_cases as CC
import track_model_cases as MC
import track_voxel_cases as VC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(mot, hip_lib):
    import hiprt

    def upload(host):
        d = hiprt.DeviceBuffer(host)
        return d.ptr, d
    return CC.Env(mot, None, upload)


@pytest.mark.parametrize("axes,current", MC.FLAGS)
@pytest.mark.parametrize("K,O", [(64, 4), (64, 16), (256, 4), (256, 16), (1024, 4), (1024, 16)])
def test_moving_objects(env, oracle, K, O, axes, current):
    VC.moving_objects(env, oracle, K, O, axes, current)


def test_one_voxel_per_model(env, oracle):
    VC.one_voxel_per_model(env, oracle)


def test_every_record_alone_and_off_the_lattice(env, oracle):
    VC.every_record_alone(env, oracle)


@pytest.mark.parametrize("K", [64, 4096])
def test_sort_sizes(env, oracle, K):
    VC.sort_sizes(env, oracle, K)


def test_min_points(env, oracle):
    VC.min_points(env, oracle)


def test_truncation(env, oracle):
    VC.truncation(env, oracle)


def test_non_finite_pose(env, oracle):
    VC.non_finite_pose(env, oracle)


def test_slot_reuse(env, oracle):
    VC.slot_reuse(env, oracle)


def test_after_a_sequence_call(env, oracle):
    VC.after_sequence(env, oracle)


def test_contract(env, oracle):
    VC.contract(env, oracle)


def test_non_interference(env, oracle):
    VC.non_interference(env, oracle)


def test_non_interference_with_launch_graphs(env, oracle):
    VC.non_interference(env, oracle, graphs=True)
