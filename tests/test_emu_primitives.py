"""tests/primitive_cases.py on the HOST build of tests/devcheck/primitives.hip (tests/emu/hipemu.h: the __shfl bodies of csrc/mot_wave.h, the exact math
and the tracker's scalar helpers as the host compiler builds them): the cases of tests/test_primitives_gpu.py, so that both bodies of every primitive are
held to ONE specification. Where a case compares two builds, the host build stands on both sides here and the case's checks against numpy and the C
library are what it asserts."""
import os
import sys

import primitive_cases as P

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


def test_primitives_wave_and_row_on_the_host_build():
    assert P.wave_case(P.host_lib()) > 500


def test_primitives_block_scan_on_the_host_build():
    """... and under the emulator's other thread orders and its dirty LDS: the barrier inside the primitive and the caller's one are what make it right"""
    assert P.block_scan_case(P.host_lib()) > 300


def test_primitives_exact_math_on_the_host_build(mot):
    import build_emu
    assert P.math_case(mot, P.host_lib(), P.host_lib(), ctx_lib_path=build_emu.build()) >= 1 << 22


def test_primitives_det5_on_the_host_build(oracle):
    assert P.det5_case(P.host_lib()) > 6000


def test_primitives_det5_exact_on_the_host_build():
    P.det5_exact_case(P.host_lib())


def test_primitives_wrap_pi_on_the_host_build(oracle):
    P.wrap_pi_case(P.host_lib())


def test_primitives_inv2_on_the_host_build(oracle):
    P.inv2_case(P.host_lib())


def test_primitives_box_fp64_on_the_host_build():
    P.box_fp64_case(P.host_lib())
