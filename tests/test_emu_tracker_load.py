"""tests/tracker_cases.py on the emulator build (CPU): 64 simultaneously live tracks per stream through mot_track_steps_dev
against the oracle — isolated gates and crowded (shared) gates — and angles far beyond the 32 turns up to which wrap_pi runs the
reference's loop. A check of the kernels' LOGIC; the -m gpu twin (tests/test_tracker_gpu.py) runs the same on the MI355X."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))


def _host(a):
    a = np.ascontiguousarray(a)
    return a.ctypes.data, lambda keep=a: None


@pytest.mark.parametrize("spacing,min_live", [(9.0, 64), (2.0, 20)])
def test_64_live_tracks_vs_oracle_emulated(mot, oracle, spacing, min_live):
    import build_emu
    import tracker_cases as TC
    st = TC.many_live_tracks(mot, oracle, _host, lib_path=build_emu.build(), streams=2, T=64, frames=18, spacing=spacing, min_live=min_live)
    assert st["live_max"] >= min_live


def test_angles_beyond_32_turns_emulated(mot, oracle):
    import build_emu
    import tracker_cases as TC
    TC.angle_far_beyond_32_turns(mot, oracle, lib_path=build_emu.build())


def test_long_run_on_bounded_track_slots_emulated(mot, oracle):
    """far more tracks created than there are slots: every frame equal to the oracle with unbounded memory (eviction one step after death,
    positions of dead tracks kept for the merge step)"""
    import build_emu
    import tracker_cases as TC
    st = TC.long_run_bounded_slots(mot, oracle, lib_path=build_emu.build(), frames=700, slots=16, spots=9)
    assert st["tracks_ever"] >= 64
    if "reference_builds_stepped" in st:   # the head of the run also met the reference's own builds (narrow criterion + their noise floor)
        print(st["reference_builds_stepped"], st.get("reference_frames"), st.get("reference_builds_retired_at"), st.get("head_vs_reference_builds"))
        assert st.get("reference_frames", 0) >= 40 and st["head_vs_reference_builds"]["state_compares"] > 50


def test_wide_batch_four_launch_path_emulated(mot, oracle):
    """tracker_cases.wide_batch at a small size: 40 streams (> 32: AUTO takes the four launches) of <= 16 tracks — empty, one-box, ~8-box, crowded (2 m), late and
    full streams side by side, a partial reset, a repeated timestamp, a call that leaves streams out — so the body's logic is checked before it meets a GPU"""
    import build_emu
    import tracker_cases as TC
    before = _launches(mot, build_emu.build())
    st = TC.wide_batch(mot, oracle, _host, lib_path=build_emu.build(), size="emu")
    after = _launches(mot, build_emu.build())
    print({k: v for k, v in st.items() if k != "live_by_kind"}, st["live_by_kind"])
    assert after["track_predict_kernel"] - before["track_predict_kernel"] == st["frames"]           # the product's switch picked the four launches on every step
    assert after["track_step_stream_kernel"] == before["track_step_stream_kernel"]


def _launches(mot, lib):
    import ctypes as C
    L = mot.load_library(lib)
    L.hipemu_launch_count.restype = C.c_long; L.hipemu_launch_count.argtypes = [C.c_char_p]
    return {k: L.hipemu_launch_count(k.encode()) for k in ("track_prep_kernel", "track_predict_kernel", "track_update_kernel", "track_update_dense_kernel", "track_finish_kernel", "track_step_stream_kernel")}


@pytest.mark.parametrize("streams,dense", [(512, True), (384, True), (383, False), (128, False)])
def test_dense_update_launch_is_issued_iff_the_context_can_hold_the_threshold(mot, streams, dense):
    """DEFAULT threshold (MOT_UPDATE_DENSE_TRACKS = 24576): a call over streams x 64 track slots issues track_update_dense_kernel iff streams x 64 >= 24576 — the launch
    that round 6's predicate (`item_groups * 8 > MOT_UPDATE_DENSE_TRACKS / 2`, always false) never issued. One step of empty streams launches everything."""
    import build_emu
    lib = build_emu.build()
    with mot.Context(lib_path=lib, max_points=1024, max_batch=streams, max_tracks_total=64) as c:
        before = _launches(mot, lib)
        for s in range(streams):
            c.ego_update(1.0e9, 0.0, 0.0, s)
        c.track_steps_dev(np.zeros(24, np.float32).ctypes.data, 24, [0] * streams, [1.0e9] * streams)
        c.synchronize()
        d = {k: v - before[k] for k, v in _launches(mot, lib).items()}
    assert d["track_prep_kernel"] == d["track_predict_kernel"] == d["track_update_kernel"] == d["track_finish_kernel"] == 1 and d["track_step_stream_kernel"] == 0, d
    assert d["track_update_dense_kernel"] == (1 if dense else 0), d
