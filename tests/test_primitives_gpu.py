"""The device-only code of the product, driven directly on the MI355X (tests/primitive_cases.py; the gfx950 build of tests/devcheck/primitives.hip):
the DPP bodies of csrc/mot_wave.h, the exact fp32 math and the tracker's scalar fp64 helpers as hipcc compiles them for gfx950, and the box stage's
fp64 library calls. tests/test_emu_primitives.py runs the same cases on the host build."""
import pytest

import primitive_cases as P

pytestmark = pytest.mark.gpu


def test_primitives_wave_and_row_on_device():
    """every primitive of mot_wave.h, DPP body, lane by lane against the header's prose restated in numpy"""
    assert P.wave_case(P.device_lib()) > 500


def test_primitives_block_scan_on_device():
    """block_scan_excl_i32 at 128, 256, 512 and 1024 threads, one and two components, one and three chained rounds, thread by thread against numpy"""
    assert P.block_scan_case(P.device_lib()) > 300


def test_primitives_exact_math_device_equals_host(mot, hip_lib):
    """mot_atanf / mot_atan2f / exact polar cell and bin / Cartesian cell: gfx950 == host build (== glibc, tests/test_math_exact.py), bit for bit,
    on the MotDevParams of the two presets and of the polar range at ratio 4"""
    assert P.math_case(mot, P.device_lib(), P.host_lib()) >= 1 << 22


def test_primitives_det5_on_device(oracle):
    """det5 == the oracle's PartialPivLU determinant bit for bit: every swap pattern, ties, zero pivots, NaN / inf, the divergence guard's neighbourhood"""
    assert P.det5_case(P.device_lib()) > 6000


def test_primitives_det5_exact_on_device():
    P.det5_exact_case(P.device_lib())


def test_primitives_wrap_pi_on_device(oracle):
    P.wrap_pi_case(P.device_lib())


def test_primitives_inv2_on_device(oracle):
    P.inv2_case(P.device_lib())


def test_primitives_box_fp64_device_equals_glibc():
    """(float)sqrt / atan2 / cos / sin of the box stage on gfx950 == glibc: every integer (dx, dy) of the two-point hull branch and 2^22
    direction-times-width pairs of the rotating-calipers branch (profiles/box_fp64_rounding.md)"""
    P.box_fp64_case(P.device_lib())
