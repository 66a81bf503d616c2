"""The device-wide stable radix sort of csrc/mot_sort.h on its own, driven through the test-only library tests/devcheck/sort.hip: shared by tests/test_sort_gpu.py (the
gfx950 build on the MI355X) and tests/test_emu_sort.py (the host build, CPU suite; the emulator's other thread orders apply). Random keys with many ties, the payload
is the input position: the output must equal np.argsort(kind="stable") — a tie swapped is a wrong payload."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "devcheck"))
T = 2048   # elements per workgroup: kSortTile of csrc/mot_sort.h (asserted against the library below)
SIZES = (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 5 * T + 333)


def _load(path):
    lib = C.CDLL(path)
    lib.mot_sort_check.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    assert lib.mot_sort_tile() == T
    return lib


def device_lib():
    import build_sort
    return _load(build_sort.build())


def host_lib():
    import build_sort
    return _load(build_sort.build_emu())


def run(lib, keys, n=None, cap=None, key_bits=56):
    keys = np.ascontiguousarray(keys, np.uint64)
    n = len(keys) if n is None else n
    cap = max(len(keys), 1) if cap is None else cap
    vals = np.arange(len(keys), dtype=np.uint32)
    ko = np.full(max(len(keys), 1) + 1, 0x7777777777777777, np.uint64); vo = np.full(max(len(keys), 1) + 1, 0x77777777, np.uint32)
    assert lib.mot_sort_check(keys.ctypes.data, vals.ctypes.data, n, cap, key_bits, ko.ctypes.data, vo.ctypes.data) == 0
    live = min(n, cap)
    assert (ko[live:] == 0x7777777777777777).all() and (vo[live:] == 0x77777777).all(), "written beyond the elements in play"
    return ko[:live], vo[:live]


def expect(keys, live, key_bits):
    part = np.asarray(keys[:live], np.uint64)
    order = np.argsort(part & np.uint64((1 << key_bits) - 1 if key_bits < 64 else 0xFFFFFFFFFFFFFFFF), kind="stable")
    return part[order], order.astype(np.uint32)


def check(lib, keys, what, **kw):
    ko, vo = run(lib, keys, **kw)
    ek, ev = expect(np.asarray(keys, np.uint64), len(ko), kw.get("key_bits", 56))
    assert vo.tobytes() == ev.tobytes(), (what, "payloads", np.argwhere(vo != ev)[:4].ravel())
    assert ko.tobytes() == ek.tobytes(), (what, "keys")


def sizes_and_ties(lib):
    """every size of the voxel cases; keys from a handful of values (long runs of ties), from a few thousand, and all distinct; the all-ones key among them"""
    rng = np.random.default_rng(41)
    for n in SIZES:
        for kinds in (5, 3000, None):
            keys = rng.integers(0, 2 ** 54, n, dtype=np.uint64) if kinds is None else rng.integers(0, 2 ** 54, kinds, dtype=np.uint64)[rng.integers(0, kinds, n)]
            if n:
                keys[rng.integers(0, n, max(n // 50, 1))] = np.uint64(0xFFFFFFFFFFFFFFFF)
            check(lib, keys, ("sizes", n, kinds))


def digits(lib):
    """keys that use only the bottom digit, only the top digit of the 56 bits, one digit in the middle; bits above key_bits are carried along and do not decide"""
    rng = np.random.default_rng(43)
    n = 3 * T + 17
    for shift in (0, 48, 24):
        check(lib, rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(shift), ("one digit", shift))
    keys = rng.integers(0, 2 ** 16, n, dtype=np.uint64) | (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(56))
    check(lib, keys, "bits above the key width", key_bits=16)
    check(lib, rng.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64), "64 bits", key_bits=64)
    check(lib, np.full(n, 7, np.uint64), "one value")
    check(lib, np.arange(n, dtype=np.uint64)[::-1].copy(), "descending")


def counts_and_capacities(lib):
    """the count on the device below, at and above the capacity of the buffers; a capacity of several tiles for one element"""
    rng = np.random.default_rng(47)
    keys = rng.integers(0, 2 ** 20, 2 * T + 100, dtype=np.uint64)
    for n, cap in ((len(keys), len(keys)), (len(keys) - 1, len(keys)), (T, len(keys)), (1, len(keys)), (0, len(keys)), (len(keys), T + 5), (len(keys) + 1000, len(keys)), (-3, len(keys))):
        if n < 0:
            assert lib.mot_sort_check(keys.ctypes.data, keys.ctypes.data, n, cap, 56, keys.ctypes.data, keys.ctypes.data) == 1
            continue
        check(lib, keys, ("count", n, cap), n=n, cap=cap)
