"""tests/sort_cases.py on the HOST build of tests/devcheck/sort.hip (tests/emu/hipemu.h): the device-wide radix sort of csrc/mot_sort.h against
np.argsort(kind="stable"). The emulator's other thread orders (MOT_EMU_SCHED=rev, rand:<seed>) apply; tests/test_sort_gpu.py runs the same cases on the MI355X."""
import sort_cases as SC


def test_sort_sizes_and_ties_on_the_host_build():
    SC.sizes_and_ties(SC.host_lib())


def test_sort_digits_on_the_host_build():
    SC.digits(SC.host_lib())


def test_sort_counts_and_capacities_on_the_host_build():
    SC.counts_and_capacities(SC.host_lib())
