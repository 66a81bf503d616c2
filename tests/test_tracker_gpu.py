"""Parity of the HIP IMM-UKF-PDA tracker (through the C-ABI) against the golden vectors produced by the reference's own
sources and against the oracle. Bar (BASELINE.json): track sets / track-management states exact, continuous state
<= 1e-4 relative."""
import numpy as np
import pytest

import golden_util as G

pytestmark = pytest.mark.gpu
RTOL = 1e-4


@pytest.fixture(scope="module")
def ctx(mot, hip_lib):
    c = mot.Context(max_points=131072, max_batch=4, max_tracks_total=2048)
    yield c
    c.close()


@pytest.mark.parametrize("name", G.TRACKERS)
def test_golden_tracker_sequences(ctx, name):
    fx = G.load(name)
    ctx.reset()
    for f in range(len(fx["n_boxes"])):
        ts = 1.0e9 + f * float(fx["unit"])
        ego = ctx.ego_update(ts, *G.ego_of(fx, f))
        assert np.allclose(ego, fx["ego"][f], rtol=1e-12, atol=1e-12)
        out = ctx.track_step(fx["boxes"][f][: fx["n_boxes"][f]], ts)
        G.check_tracker_frame(fx, f, out, lambda i: ctx.track_state(i), rtol=RTOL)


@pytest.mark.parametrize("name", G.TRACKERS_OT0)
def test_golden_tracker_sequences_ot0(mot, hip_lib, name):
    """object_tracking0's tracker (its own ukf.cpp / imm_ukf_jpda.cpp built into oracle/_ref/libmot_ref0.so): preset 1"""
    fx = G.load(name)
    with mot.Context(mot.params(1), max_points=4096, max_tracks_total=512) as c:
        for f in range(len(fx["n_boxes"])):
            ts = 1.0e9 + f * float(fx["unit"])
            ego = c.ego_update(ts, *G.ego_of(fx, f))
            assert np.allclose(ego, fx["ego"][f], rtol=1e-12, atol=1e-12)
            out = c.track_step(fx["boxes"][f][: fx["n_boxes"][f]], ts)
            G.check_tracker_frame(fx, f, out, lambda i: c.track_state(i), rtol=RTOL)


def _boxes_sequence(oracle, synth, p, stream, nframes, npts):
    seq = []
    for f in range(nframes):
        c = synth.make_cloud(npts, stream, f)
        g = oracle.ground_remove(p, c); cl = oracle.cluster(p, g["elevated"])
        seq.append(oracle.box_fit(p, g["elevated"], cl["grid"], cl["num_cluster"])["boxes"])
    return seq


def _compare_step(a, o, state_dev, state_orc, f):
    assert a["n"] == o["n"], f
    assert np.array_equal(a["track_manage"], o["track_manage"]), f
    assert np.array_equal(a["is_static"], o["is_static"]) and np.array_equal(a["is_vis"], o["is_vis"]), f
    assert np.array_equal(a["lifetime"], o["lifetime"]), f
    live = o["track_manage"] > 0
    assert np.allclose(a["p"][live], o["p"][live], rtol=RTOL, atol=1e-6)
    assert np.allclose(a["v_yaw"][live], o["v_yaw"][live], rtol=RTOL, atol=1e-7)
    assert np.allclose(a["vis_box"], o["vis_box"], rtol=RTOL, atol=1e-5)
    for i in np.nonzero(live)[0]:
        sd, so = state_dev(int(i)), state_orc(int(i))
        for k in ("x_merge", "x_cv", "x_ctrv", "x_rm", "p_merge", "p_cv", "p_ctrv", "p_rm", "mode_prob", "z_pred", "s", "k"):
            scale = max(np.abs(so[k]).max(), 1e-300)
            assert np.abs(sd[k] - so[k]).max() <= RTOL * scale + 1e-9, (f, i, k)


@pytest.mark.parametrize("unit,stream", [(1e5, 3), (0.1, 3), (1e5, 6)])
def test_tracker_vs_oracle_long_sequence(ctx, oracle, synth, unit, stream):
    p = oracle.params(0)
    seq = _boxes_sequence(oracle, synth, p, stream, 60, 40000)
    ctx.reset()
    T = oracle.Tracker(p)
    for f, b in enumerate(seq):
        ts = 2.0e8 + f * unit
        v, yaw = 5.0, 0.01 * f
        assert np.allclose(ctx.ego_update(ts, v, yaw), T.ego_update(ts, v, yaw), rtol=1e-12, atol=1e-12)
        a = ctx.track_step(b, ts); o = T.step(b, ts)
        _compare_step(a, o, ctx.track_state, T.state, f)
    assert (o["track_manage"] >= 5).sum() >= 3  # the sequence really exercises confirmed tracks
    T.close()


def test_tracker_slots_are_independent_and_reset_works(ctx, oracle, synth):
    p = oracle.params(0)
    seqs = [_boxes_sequence(oracle, synth, p, s, 15, 30000) for s in (1, 2)]
    ctx.reset()
    Ts = [oracle.Tracker(p), oracle.Tracker(p)]
    for f in range(15):
        for slot in (1, 0):  # interleaved, different slots
            ts = 1.0e8 + f * 1e5 + slot
            ctx.ego_update(ts, 1.0 + slot, 0.0, slot=slot); Ts[slot].ego_update(ts, 1.0 + slot, 0.0)
            a = ctx.track_step(seqs[slot][f], ts, slot=slot); o = Ts[slot].step(seqs[slot][f], ts)
            _compare_step(a, o, lambda i: ctx.track_state(i, slot=slot), Ts[slot].state, (f, slot))
    ctx.reset()
    T = oracle.Tracker(p)
    for f in range(5):
        ts = 1.0e8 + f * 1e5
        ctx.ego_update(ts, 0.0, 0.0); T.ego_update(ts, 0.0, 0.0)
        _compare_step(ctx.track_step(seqs[0][f], ts), T.step(seqs[0][f], ts), ctx.track_state, T.state, f)


def test_tracker_edge_cases(mot, hip_lib, oracle):
    p = oracle.params(0)
    with mot.Context(max_points=1024, max_tracks_total=3) as c:
        with pytest.raises(mot.MotError) as e:   # ego update must come first (getOriginPoints precedes immUkfJpdaf)
            c.track_step(np.zeros((0, 8, 3), np.float32), 0.0)
        assert e.value.code == mot.MOT_E_STATE
        T = oracle.Tracker(p)
        # first frame with fewer boxes than the seed index: no track is seeded, init_ still flips
        c.ego_update(1e6, 0, 0); T.ego_update(1e6, 0, 0)
        box = np.zeros((1, 8, 3), np.float32); box[0, :, :2] = [[0, 0], [1, 0], [1, 1], [0, 1]] * 2
        a = c.track_step(box, 1e6); o = T.step(box, 1e6)
        assert a["n"] == o["n"] == 0
        rng = np.random.default_rng(0)
        full = False   # more births in a frame than free slots: reported (MOT_E_CAPACITY in C, `capacity_exceeded` here), the records still delivered
        for f in range(1, 6):
            ts = 1e6 + f * 1e5
            c.ego_update(ts, 0, 0)
            b = np.zeros((4, 8, 3), np.float32)
            for k in range(4):
                cx, cy = rng.uniform(-20, 20, 2)
                b[k, :, :2] = (np.array([[0, 0], [2, 0], [2, 1], [0, 1]] * 2) + [cx, cy])
            out = c.track_step(b, ts)
            full |= out["capacity_exceeded"]
            assert int((out["track_manage"] > 0).sum()) <= 3   # 3 slots, 4 births per frame
        assert full


def test_fused_frames_with_tracker(mot, hip_lib, oracle, synth):
    """ground -> cluster -> box -> tracker per frame with everything on the device, 2 streams, 12 frames. The oracle tracker is fed
    through the tracking node's own tf sequence (oracle/ref_tf_capi.cpp via seq_parity.boxes_to_global), the same arithmetic the
    fused path applies: boxes in the global frame bit-exact, every state key at the 1e-4 bar."""
    import ctypes as C
    import hiprt
    import seq_parity as SP
    p = oracle.params(0)
    B, N, stride = 2, 40000, 40960
    stats = {}
    with mot.Context(max_points=stride, max_batch=B, max_tracks_total=1024) as c:
        Ts = [oracle.Tracker(p) for _ in range(B)]
        for f in range(12):
            host = np.zeros((B, stride, 4), np.float32)
            clouds = [synth.make_cloud(N, 30 + b, f) for b in range(B)]
            for b in range(B):
                host[b, :N] = clouds[b]
            dev = hiprt.DeviceBuffer(host)
            ts = [3.0e8 + f * 1e5] * B; ev = [2.0, 0.0]; ey = [0.002 * f, 0.0]
            c.frames_dev(dev.ptr, stride * 4, [N] * B, run_tracker=True, timestamps=ts, ego_v=ev, ego_yaw=ey)
            for b in range(B):
                g = oracle.ground_remove(p, clouds[b]); cl = oracle.cluster(p, g["elevated"])
                bx = oracle.box_fit(p, g["elevated"], cl["grid"], cl["num_cluster"])["boxes"]
                assert SP.bits_equal(c.get_boxes(b)["boxes"], bx)
                ego = Ts[b].ego_update(ts[b], ev[b], ey[b])
                gb = SP.boxes_to_global(oracle, c.lib, bx, ego[:3])
                if len(gb):
                    gdev = np.zeros((1024, 8, 3), np.float32)
                    assert c.lib.mot_debug_copy(c._h, 11, b, gdev.ctypes.data_as(C.c_void_p), C.c_size_t(gdev.nbytes)) == 0
                    assert SP.bits_equal(gdev[: len(gb)], gb), (f, b)
                o = Ts[b].step(gb, ts[b])
                SP.compare_tracks(c.get_tracks(b), o, lambda i: c.track_state(i, slot=b), Ts[b].state, (f, b), rtol=RTOL, stats=stats)
            dev.free()
    assert stats["tracks_ever"] >= 3


def _to_dev(a):
    import hiprt
    d = hiprt.DeviceBuffer(np.ascontiguousarray(a))
    return d.ptr, d.free


@pytest.mark.parametrize("spacing,min_live", [(9.0, 64), (2.0, 20)])
def test_64_live_tracks_vs_oracle(mot, hip_lib, oracle, spacing, min_live):
    """BASELINE.json configs[3]'s tracker load (<= 64 tracks) against the ORACLE, not another HIP entry point: 64 simultaneously
    live tracks per stream through mot_track_steps_dev (the 16-lane-per-track kernels, the (stream, track) work list), every frame
    and stream; at 2 m spacing neighbouring tracks share gated boxes (the matchingVec bookkeeping of imm_ukf_jpda.cpp:232, H12)"""
    import tracker_cases as TC
    st = TC.many_live_tracks(mot, oracle, _to_dev, streams=4, T=64, frames=30, spacing=spacing, min_live=min_live)
    assert st["live_max"] >= min_live and st["max_rel_state_err"] <= RTOL


def test_angles_beyond_32_turns(mot, hip_lib, oracle):
    """csrc/mot_track_prep.h wrap_pi's bounded path (the one documented deviation): discrete outputs equal the looping oracle's"""
    import tracker_cases as TC
    TC.angle_far_beyond_32_turns(mot, oracle)


@pytest.mark.parametrize("preset", [0, 1])
def test_tracker_random_and_degenerate_sequences(mot, hip_lib, oracle, preset):
    """the generators of tests/test_emu_tracker_random.py on the real kernel: objects that move, stop, vanish, split into two
    boxes, crowd each other, clutter, duplicate / zero-area / far-away measurements, a wandering ego pose. Discrete outputs
    exact; continuous state to the 1e-4 bar while the filter is well conditioned (a diverging track amplifies last-bit
    differences by decades per frame — see well_conditioned). On the CPU the same sequences pass with the kernels' sin / cos /
    exp / atan2 / pow results moved by an ulp (MOT_EMU_PERTURB), i.e. they do not hang on the device math library's last bit."""
    import tempfile
    import oracle_lib as OL
    import test_emu_tracker_random as TR
    p = oracle.params(preset)
    # preset 1 = object_tracking0's tracker, which reads its ego motion from two text files: the proxy routes it to the restatement, so here the
    # reference's own build (oracle/_ref/libmot_ref0.so) is driven directly — the sequence's whole ego motion is known up front (round-4 review:
    # this case never met the reference's code on the GPU box)
    use_ref0 = preset == 1 and OL.ref0() is not None
    with mot.Context(mot.params(preset), max_points=4096, max_tracks_total=512) as c:
        for seed in range(1000 * preset, 1000 * preset + 14):
            seq = list(TR.sequence(seed) if seed % 4 else TR.hostile_sequence(seed))
            c.reset()
            if use_ref0:
                T = OL.Ref0Tracker(); T.reset(tempfile.mkdtemp(prefix="mot_ref0_"), [s[2] for s in seq], [s[3] for s in seq])
                if hasattr(oracle, "_note"):
                    oracle._note("Tracker", "reference build")
            else:
                T = oracle.Tracker(p)
            for f, (boxes, ts, v, yaw) in enumerate(seq):
                c.ego_update(ts, v, yaw)
                if use_ref0:
                    T.ego_update(ts)
                else:
                    T.ego_update(ts, v, yaw)
                a = c.track_step(boxes, ts); o = T.step(boxes, ts)
                assert a["n"] == o["n"], (seed, f)
                for k in ("track_manage", "is_static", "is_vis", "lifetime"):
                    assert np.array_equal(a[k], o[k]), (seed, f, k)
                for i in np.nonzero(o["track_manage"] > 0)[0]:
                    so = T.state(int(i))
                    if not TR.well_conditioned(so):
                        continue
                    sa = c.track_state(int(i))
                    assert np.allclose(a["p"][i], o["p"][i], rtol=RTOL, atol=1e-5), (seed, f, int(i))
                    for k in ("x_merge", "p_merge", "mode_prob"):
                        scale = max(np.abs(so[k]).max(), 1e-300)
                        assert np.abs(np.asarray(sa[k]) - so[k]).max() <= RTOL * scale + 1e-9, (seed, f, int(i), k)
            T.close()


def test_long_run_on_256_track_slots(mot, hip_lib, oracle):
    """10 000 frames on max_tracks_total = 256 slots, thousands of tracks created: every frame the discrete outputs of every track ever
    created equal the oracle's with unbounded memory (the reference never frees a track, imm_ukf_jpda.cpp:972-989); filter states of the
    live tracks every 50 frames. The world replays the situation in which a dead track's last position decides a live track's fate."""
    import tracker_cases as TC
    st = TC.long_run_bounded_slots(mot, oracle, frames=10000, slots=256, spots=40, state_every=50, min_ever_factor=8, max_chaos_restarts=40)
    assert st["tracks_ever"] >= 2048 and st["max_rel_state_err"] <= 1e-2 and st["frames_compared"] >= 9900
    _report_head(st)


def test_long_run_on_few_slots(mot, hip_lib, oracle):
    """the same with 24 slots for up to ~20 live tracks: slots are recycled constantly"""
    import tracker_cases as TC
    st = TC.long_run_bounded_slots(mot, oracle, frames=2500, slots=24, spots=14, state_every=25, min_ever_factor=8, max_chaos_restarts=6)
    assert st["tracks_ever"] >= 192 and st["frames_compared"] >= 2450
    _report_head(st)


def _report_head(st):
    """the head of a long run against the reference's OWN builds (tracker_cases.long_run_bounded_slots: ref_frames): stepped as long as their
    discrete outputs equal the restatement's; the device's states on those frames under the narrow criterion + the builds' noise floor"""
    if "reference_builds_stepped" not in st:
        return
    print("long run, head vs the reference builds:", st["reference_builds_stepped"], "frames", st.get("reference_frames"), "retired at",
          st.get("reference_builds_retired_at"), st.get("head_vs_reference_builds"))
    assert st.get("reference_frames", 0) >= 40 and st["head_vs_reference_builds"]["state_compares"] > 50


# ---- the many-stream path: four launches, one work list over all streams (what 512-stream contexts run); tests/tracker_cases.py has the bodies

def _timed(fn, *a, **kw):
    import time
    t0 = time.time()
    st = fn(*a, **kw)
    st["wall_s"] = round(time.time() - t0, 1)
    return st


def test_wide_batch_four_launch_path_vs_oracle(mot, hip_lib, oracle):
    """256 streams in one context under AUTO (batch * 8 reaches the 1536-workgroup clamp, the plain update its 1024: every workgroup takes several rounds of the
    work list): empty, 1-box, ~8-box, crowded (2 m), late and 64-box streams side by side, every stream its own sequence, a partial reset, a repeated timestamp,
    a call that leaves streams out; > 14 000 live tracks at the peak. Every stream on every frame against its own reference tracker."""
    import tracker_cases as TC
    st = _timed(TC.wide_batch, mot, oracle, _to_dev, size="gpu")
    print("wide_batch:", {k: v for k, v in st.items() if k != "live_by_kind"}, st["live_by_kind"])
    assert st["streams"] >= 224 and max(st["live_total"]) >= 12000


def test_dense_threshold_crossings(mot, hip_lib, oracle):
    """512 streams x 64 track slots, default library, AUTO: the live-track count of the step crosses MOT_UPDATE_DENSE_TRACKS = 24576 back and forth, with one
    step at exactly 24576 and one at 24575 — track_update_dense_kernel (3 waves per SIMD, spills) and track_update_kernel take turns on the device. Every stream
    on every frame against its own reference tracker; the planned sequence of n_items is asserted from the oracles' live counts."""
    import tracker_cases as TC
    st = _timed(TC.dense_threshold, mot, oracle, _to_dev)
    print("dense_threshold:", {k: v for k, v in st.items() if k != "live_by_kind"}, st["live_by_kind"])


def test_tracker_launch_modes_give_identical_results_on_the_device(mot, hip_lib, oracle):
    """MOT_TRACKER_SPLIT against MOT_TRACKER_STREAM on the MI355X: outputs and every state key bit for bit, NaNs included (random, hostile and 40-live-track sequences)"""
    import tracker_cases as TC
    st = _timed(TC.launch_modes_identical, mot, oracle, _to_dev)
    print("launch modes:", st)


@pytest.fixture(scope="session")
def dense4_lib(hip_lib):
    """test-variant library with the dense threshold pulled down to 4 live tracks (variants/ is not in git; built once when missing)"""
    import os
    import conftest
    build = conftest.load_sub("build")
    out = os.path.join(conftest.ROOT, "variants", "libmot_dense4.so")
    deps = [os.path.join(build.CSRC, s) for s in build.SOURCES + build.HEADERS]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        build.build(extra_flags=("-DMOT_UPDATE_DENSE_TRACKS=4",), out=out)
    return out


def test_dense_variant_library_equals_the_default_bit_for_bit(mot, hip_lib, dense4_lib, oracle):
    """-DMOT_UPDATE_DENSE_TRACKS=4 against the default library, both in SPLIT mode: the golden sequences cross the threshold back and forth, the 64-live-track
    case sits above it — the spilled instantiation held against the unspilled one directly: bit-identical; and both within the bar of the reference."""
    import conftest
    import tracker_cases as TC
    build = conftest.load_sub("build")
    st = _timed(TC.dense_variant_identical, mot, oracle, _to_dev, build.LIB, dense4_lib, G.TRACKERS)
    print("dense variant:", st)
    assert st["threshold_crossings"] >= 2, st
