"""The allocations of the per-track point clouds (csrc/mot_api_tracks.hip ensure_track_points) on the emulator's ledger (tests/emu/hipemu.h, as
tests/test_emu_lifecycle.py uses it): a context that exported gives everything back at mot_destroy, and each of the two entry points walked through a failure
at each of its allocations answers MOT_E_HIP, leaves the context usable, and succeeds when called again — with the result of a context that never saw a failure."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import capacity_cases as CC
import lifecycle_cases as LC
import track_point_cases as PC


@pytest.fixture(scope="module")
def env(mot):
    import build_emu
    return CC.Env(mot, build_emu.build())


@pytest.fixture(scope="module")
def lib(env):
    lib = env.mot.load_library(env.lib_path)
    lib.hipemu_live_allocs.restype = lib.hipemu_live_events.restype = C.c_long
    lib.hipemu_fail_alloc_at.argtypes = [C.c_long]; lib.hipemu_fail_alloc_at.restype = None
    yield lib
    lib.hipemu_fail_alloc_at(0)


def live(lib):
    return lib.hipemu_live_allocs(), lib.hipemu_live_events()


def prelude(env):
    c = LC.context(env)
    c.set_track_links(True)
    frames = LC.clouds()
    keep = [PC.launch(env, c, [frames[f], frames[f + 1]], LC.MAX_POINTS, f, yaw=0.03 * f) for f in range(3)]
    c.synchronize()
    return c, keep


def export(env, c):
    """-> (code, what the call delivered)"""
    blk = PC.DevBlocks(env, LC.BATCH, LC.MAX_POINTS, PC.MAX_SEG)
    rc = PC.raw_export(env, c, blk, LC.BATCH, env.mot.MOT_TRACK_POINTS_REST, env.mot.MOT_FRAME_GLOBAL)
    c.synchronize()
    return rc, [np.array(x) for x in blk.read()]


def getter(env, c):
    try:
        r = c.get_track_points(1, rest=True, frame="global")
    except env.mot.MotError as e:
        return e.code, None
    return 0, [r[k] for k in ("xyz", "index", "track_id", "first", "count", "n_boxes")]


def test_emu_nothing_is_left_after_destroy(env, lib):
    base = live(lib)
    c, keep = prelude(env)
    before = live(lib)
    assert export(env, c)[0] == 0 and getter(env, c)[0] == 0
    assert live(lib)[0] > before[0] and live(lib)[1] > before[1]   # (the feature did allocate, memory and the ring's events)
    c.close()
    assert live(lib) == base


@pytest.mark.parametrize("call", [export, getter])
def test_emu_call_under_allocation_failure(env, lib, call):
    base = live(lib)
    c, keep = prelude(env)
    before = sum(live(lib))
    rc, want = call(env, c)
    n = sum(live(lib)) - before   # every allocation and event of the entry point's first call (it frees none)
    c.close()
    assert rc == 0 and n >= 6 and live(lib) == base
    assert want[1].size > 0
    for k in range(1, n + 1):
        c, keep = prelude(env)
        ids = c.get_point_tracks(1)
        lib.hipemu_fail_alloc_at(k)
        rc, got = call(env, c)
        lib.hipemu_fail_alloc_at(0)
        assert rc == LC.MOT_E_HIP, (k, rc)
        assert b"hipMalloc(&c->d_tp_" in c.lib.mot_last_error(c._h) or b"hipHostMalloc(&" in c.lib.mot_last_error(c._h) or b"hipEventCreateWithFlags(&" in c.lib.mot_last_error(c._h), k
        if got is not None:
            assert all((x == -7).all() for x in got), (k, "a refused call wrote into the caller's blocks")
        assert np.array_equal(c.get_point_tracks(1), ids) and len(c.get_boxes(1)["boxes"]) > 0, (k, "the context is no longer usable")
        rc, got = call(env, c)
        assert rc == 0, (k, rc)
        LC.same_run(got, want, (call.__name__, k))
        c.close()
        assert live(lib) == base, k
