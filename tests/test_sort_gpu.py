"""The device-wide radix sort of csrc/mot_sort.h, driven directly on the MI355X (tests/sort_cases.py; the gfx950 build of tests/devcheck/sort.hip) against
np.argsort(kind="stable"). tests/test_emu_sort.py runs the same cases on the host build."""
import pytest

import sort_cases as SC

pytestmark = pytest.mark.gpu


def test_sort_sizes_and_ties_on_device():
    SC.sizes_and_ties(SC.device_lib())


def test_sort_digits_on_device():
    SC.digits(SC.device_lib())


def test_sort_counts_and_capacities_on_device():
    SC.counts_and_capacities(SC.device_lib())
