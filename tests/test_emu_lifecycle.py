"""A context's life cycle on the emulator (tests/lifecycle_cases.py): the ownership helpers of csrc/mot_host.h give back everything a context took, whichever lazy
path took it, and every allocating call walked through a failure at each of its allocations keeps the promise its comments make — MOT_E_HIP, the mode not
entered, what exists kept for mot_destroy and for the next request, which succeeds and computes what a context that never saw the failure computes. The
ledger and the injected failure are tests/emu/hipemu.h's (hipemu_live_allocs, hipemu_live_events, hipemu_fail_alloc_at). tests/test_lifecycle_gpu.py runs
create -> touch_everything -> destroy on the MI355X."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import capacity_cases as CC
import lifecycle_cases as LC


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


@pytest.fixture(scope="module")
def frames():
    return LC.clouds()


def live(lib):
    return lib.hipemu_live_allocs(), lib.hipemu_live_events()


def test_emu_nothing_is_left_after_destroy(env, lib, frames):
    """create -> every lazily allocating path once -> destroy: live allocations and live events are back where they were"""
    base = live(lib)
    c = LC.context(env)
    created = live(lib)
    LC.touch_everything(env, c, frames)
    assert live(lib)[0] > created[0] and live(lib)[1] > created[1]   # (the lazy paths did allocate)
    c.close()
    assert live(lib) == base


def raw_create(env, lib):
    p = env.params(0); h = C.c_void_p(0x1)
    rc = lib.mot_create(C.byref(p), 0, LC.MAX_POINTS, LC.BATCH, LC.T_TOTAL, C.byref(h))
    return rc, h


def test_emu_create_under_allocation_failure(env, lib, capfd):
    """mot_create refused at each of its allocations in turn: MOT_E_HIP, *out null, a reason, nothing left behind"""
    base = live(lib)
    rc, h = raw_create(env, lib)
    assert rc == 0
    n = sum(live(lib)) - sum(base)   # every allocation and event a successful mot_create makes (it frees none)
    lib.mot_destroy(h)
    assert n > 60 and live(lib) == base
    for k in range(1, n + 1):
        lib.hipemu_fail_alloc_at(k)
        rc, h = raw_create(env, lib)
        assert rc == LC.MOT_E_HIP and not h.value, k
        why = lib.mot_last_error(None)
        assert any(t in why for t in (b"hipMalloc(&c->", b"hipHostMalloc(&", b"hipEventCreateWithFlags(&")), (k, why)   # (the reason names what could not be had)
        assert live(lib) == base, k
    lib.hipemu_fail_alloc_at(n + 1)   # (one beyond: the walk above covered them all)
    rc, h = raw_create(env, lib)
    lib.hipemu_fail_alloc_at(0)
    assert rc == 0
    lib.mot_destroy(h)
    capfd.readouterr()   # ("mot_create failed: ..." on stderr, once per refusal)


# ------------------------------------------------------------------------------------------------------------------ lazy modes
class Lazy:
    """one lazily allocating call: what precedes it on a fresh context, the call itself (returns the ABI's code), how to see that a refused call left
    the mode alone, and what follows — whose results are compared with a context that never saw a failure"""

    def __init__(self, env, frames):
        self.env, self.frames = env, frames

    def prelude(self, c):
        fd = LC.Feed(c, self.frames)
        host = np.zeros((LC.BATCH, LC.MAX_POINTS, 4), np.float32)
        pair = fd.pair()
        for b, x in enumerate(pair):
            host[b, : len(x)] = x
        ts = [2.0e8] * LC.BATCH
        c.frames_dev(host.ctypes.data, LC.MAX_POINTS * 4, [len(x) for x in pair], run_tracker=True, timestamps=ts, ego_v=[1.0] * LC.BATCH, ego_yaw=[0.0] * LC.BATCH)
        fd.keep.append(host); fd._done(pair, ts[0])
        return fd

    def results(self, c, fd, extra):
        return LC.flatten(fd.boxes, dict(tracks=[c.get_tracks(b) for b in range(LC.BATCH)], node=extra, fetched=[]))


class PointOrder(Lazy):
    def call(self, c, fd):
        return c.lib.mot_set_point_order(c._h, LC.ORDER_ANY)

    def not_entered(self, c):
        ms = C.c_float(0)   # (the regrouping kernels can be timed in MOT_ORDER_ANY only)
        assert c.lib.mot_time_stage(c._h, 35, LC.BATCH, 1, C.byref(ms)) == LC.MOT_E_STATE and b"MOT_ORDER_ANY only" in c.lib.mot_last_error(c._h)

    def after(self, c, fd):
        fd.host(4)
        return None


class TrackLinks(Lazy):
    def call(self, c, fd):
        return c.lib.mot_set_track_links(c._h, 1)

    def not_entered(self, c):
        nb = C.c_int(0)
        assert c.lib.mot_get_box_tracks(c._h, 0, None, 0, C.byref(nb)) == LC.MOT_E_STATE and b"track links are off" in c.lib.mot_last_error(c._h)

    def after(self, c, fd):
        fd.host(4)
        return dict(tracks=np.concatenate([c.get_box_tracks(b) for b in range(LC.BATCH)] + [c.get_point_tracks(b) for b in range(LC.BATCH)]), n_live=0, n_ever=0, origin=np.zeros(6))


class FramesHost(Lazy):
    def call(self, c, fd):
        try:
            fd.host(4)
        except self.env.mot.MotError as e:
            return e.code
        return 0

    def not_entered(self, c):
        pass   # (no mode: the repeated call must allocate what is missing, and the slots still hold the prelude's frame — compared below)

    def after(self, c, fd):
        fd.host(3)
        return None


class NodeFrame(Lazy):
    def call(self, c, fd):
        try:
            self.out = fd.node_frame(0)
        except self.env.mot.MotError as e:
            return e.code
        return 0

    def not_entered(self, c):
        pass   # (the stream has not stepped: its tracks after the repeated call are those of a stream that stepped once — compared below)

    def after(self, c, fd):
        fd.host(4)
        return self.out


@pytest.mark.parametrize("kind", [PointOrder, TrackLinks, FramesHost, NodeFrame])
def test_emu_lazy_call_under_allocation_failure(env, lib, frames, kind):
    """for every allocation k of the call: refused with MOT_E_HIP and the mode not entered; the same call again succeeds; what follows is bit-identical to
    a context that never saw the failure; destroy gives everything back"""
    base = live(lib)
    case = kind(env, frames)
    c = LC.context(env)
    fd = case.prelude(c)
    before = sum(live(lib))
    assert case.call(c, fd) == 0
    n = sum(live(lib)) - before   # (none of these calls frees anything on a fresh context)
    want = case.results(c, fd, case.after(c, fd))
    c.close()
    assert n >= 3 and live(lib) == base
    for k in range(1, n + 1):
        c = LC.context(env)
        fd = case.prelude(c)
        lib.hipemu_fail_alloc_at(k)
        rc = case.call(c, fd)
        lib.hipemu_fail_alloc_at(0)
        assert rc == LC.MOT_E_HIP, (k, rc)
        case.not_entered(c)
        assert case.call(c, fd) == 0, k
        LC.same_run(case.results(c, fd, case.after(c, fd)), want, (kind.__name__, k))
        c.close()
        assert live(lib) == base, k
