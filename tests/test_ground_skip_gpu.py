"""The compaction kernel's group skip (tests/ground_skip_cases.py) on the MI355X: frame lengths around both kernels' chunk edges, an elevated point at every
group position, dropped groups, special z values, other point orders, the ground cloud and mask on demand — bit for bit against the C restatement
(oracle_lib.ground_remove). tests/test_emu_ground_skip.py runs the same bodies on the emulator."""
import os

import pytest

import capacity_cases as CC
import ground_skip_cases as GS
import oracle_lib

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def env(mot, hip_lib):
    import hiprt
    oracle_lib.build_oracle()

    def upload(host):
        d = hiprt.DeviceBuffer(host)
        return d.ptr, d
    return CC.Env(mot, None, upload)


def test_frame_lengths(env):
    GS.frame_lengths(env, oracle_lib)


@pytest.mark.parametrize("crop", [False, True])
def test_special_groups(env, crop):
    GS.special_groups(env, oracle_lib, crop)


def test_golden_frame_boxes(env):
    GS.golden_frame(env, oracle_lib, GOLDEN)
