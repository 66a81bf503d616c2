"""The compaction kernel's group skip (tests/ground_skip_cases.py) under the emulator: both kernels' LOGIC — the min-z kernel's max z per group of 8 points, the
ballot and the predicated loads of the elevated-only compaction — bit for bit against the C restatement. The same bodies run on the MI355X in
tests/test_ground_skip_gpu.py."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import capacity_cases as CC
import ground_skip_cases as GS
import oracle_lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def env(mot):
    import build_emu
    oracle_lib.build_oracle()
    return CC.Env(mot, build_emu.build())


def test_emu_frame_lengths(env):
    GS.frame_lengths(env, oracle_lib)


@pytest.mark.parametrize("crop", [False, True])
def test_emu_special_groups(env, crop):
    GS.special_groups(env, oracle_lib, crop)


def test_emu_golden_frame_boxes(env):
    GS.golden_frame(env, oracle_lib, GOLDEN)
