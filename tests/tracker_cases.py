"""Tracker load cases shared by the emulator test (tests/test_emu_tracker_load.py, CPU) and the MI355X test
(tests/test_tracker_gpu.py): bodies only; the callers supply the library and how a numpy array becomes a device buffer.
TEST INFRASTRUCTURE (compares with the oracle)."""
import numpy as np

import seq_parity as SP


def grid_boxes(streams, T, f, vel, rng, spacing):
    """`T` boxes per stream on a sqrt(T) x sqrt(T) lattice `spacing` metres apart, drifting with `vel` (bench.py tracker_stress's
    generator): spacing 9 m keeps every gate to itself; 2 m makes neighbouring tracks share gated boxes — the cross-track
    matchingVec bookkeeping of imm_ukf_jpda.cpp:232 at the size BASELINE.json configs[3] names (<= 64 tracks)"""
    side = int(np.ceil(np.sqrt(T)))
    centres = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)[:T] * spacing - side * spacing / 2
    ctr = centres[None] + vel * (0.1 * f) + rng.normal(0, 0.02, size=(streams, T, 2))
    bx = np.zeros((streams, T, 8, 3), np.float32)
    w, l = (3.8, 1.7) if spacing >= 6 else (1.2, 0.8)
    bx[..., :2] = ctr[:, :, None, :] + np.array([[0, 0], [w, 0], [w, l], [0, l]] * 2)[None, None]
    bx[:, :, :4, 2] = -2.0; bx[:, :, 4:, 2] = -0.4
    return bx


def many_live_tracks(mot, oracle, to_dev, lib_path=None, streams=3, T=64, frames=30, spacing=9.0, seed=11, min_live=64):
    """mot_track_steps_dev (every stream at once, boxes on the device) against the oracle with `T` simultaneously live tracks
    per stream: every frame, every stream, discrete outputs exact and every state key <= 1e-4"""
    rng = np.random.default_rng(seed)
    vel = rng.uniform(-1.0, 1.0, size=(streams, T, 2))
    p = oracle.params(0)
    kw = dict(lib_path=lib_path) if lib_path else {}
    stats = {}
    with mot.Context(max_points=1024, max_batch=streams, max_tracks_total=1024, **kw) as c:
        Ts = [oracle.Tracker(p) for _ in range(streams)]
        stride = T * 24
        live = [0] * streams
        for f in range(frames):
            ts = 1.0e9 + f * 1e5
            bx = grid_boxes(streams, T, f, vel, rng, spacing)
            ptr, free = to_dev(bx.reshape(streams, stride))
            for s in range(streams):
                a_ego = c.ego_update(ts, 0.0, 0.0, s); o_ego = Ts[s].ego_update(ts, 0.0, 0.0)
                assert np.array_equal(a_ego, o_ego)
            c.track_steps_dev(ptr, stride, [T] * streams, [ts] * streams)
            for s in range(streams):
                a = c.get_tracks(s); o = Ts[s].step(bx[s], ts, max_tracks=1024)
                SP.compare_tracks(a, o, lambda i: c.track_state(i, slot=s), Ts[s].state, (f, s), stats=stats, skip_ill_conditioned=spacing < 6)
                live[s] = int((o["track_manage"] > 0).sum())
            free()
        for T_ in Ts:
            T_.close()
    assert min(live) >= min_live, live
    stats["live_last"] = live
    return stats


def angle_far_beyond_32_turns(mot, oracle, lib_path=None):
    """The one documented deviation from the reference (csrc/mot_track_prep.h wrap_pi): up to 32 turns the normalisation loop runs as
    written, beyond it whole turns come off in one step. Two ways past 32 turns: (a) an ego yaw of hundreds of radians — the
    output yaw is wrap(x_merge(3) + egoYaw), OT/tracking/imm_ukf_jpda.cpp:1010 — and (b) a time step of thousands of seconds,
    which carries every CTRV sigma point yaw + yawd * dt round and round (ukf.cpp:539-571). The oracle keeps the reference's
    loops (oracle/mot_oracle_track.c). Discrete outputs must stay equal on every frame; the yaw outputs agree to 1e-9."""
    import test_emu_tracker_random as TR
    p = oracle.params(0)
    kw = dict(lib_path=lib_path) if lib_path else {}
    rng = np.random.default_rng(5)
    n_obj = 6
    pos = rng.uniform(-20, 20, (n_obj, 2)); vel = rng.uniform(-1.5, 1.5, (n_obj, 2)); yaw = rng.uniform(-3, 3, n_obj)
    hit_ego = hit_dt = False
    with mot.Context(max_points=1024, max_tracks_total=512, **kw) as c:
        T = oracle.Tracker(p)
        ts = 1.0e9
        for f in range(34):
            jump = f in (16, 25)
            ts += 6.0e9 if jump else 1.0e5                      # (b): dt = 6000 s on two frames
            ego_yaw = 0.01 * f + (900.0 if f >= 8 else 0.0)     # (a): 143 turns from frame 8 on
            boxes = np.array([TR.box(*(pos[o] + vel[o] * 0.1 * f), 1.8, 4.2, yaw[o] + 0.02 * f, -0.3) for o in range(n_obj)], np.float32)
            a_ego = c.ego_update(ts, 3.0, ego_yaw); o_ego = T.ego_update(ts, 3.0, ego_yaw)
            assert np.allclose(a_ego, o_ego, rtol=1e-12, atol=1e-9)
            pre = [T.state(i) for i in range(c.get_tracks(0)["n"])] if jump else []   # states the 6000 s prediction starts from
            a = c.track_step(boxes, ts); o = T.step(boxes, ts)
            assert a["n"] == o["n"], f
            for k in ("track_manage", "is_static", "is_vis", "lifetime"):
                assert np.array_equal(a[k], o[k]), (f, k)
            livei = np.nonzero(o["track_manage"] > 0)[0]
            fin = np.isfinite(o["v_yaw"][livei, 1])
            assert np.allclose(a["v_yaw"][livei, 1][fin], o["v_yaw"][livei, 1][fin], rtol=0, atol=1e-9), f
            if f >= 8 and len(livei):
                hit_ego = True
            if jump:
                hit_dt |= any(s["track_manage"] > 0 and abs(s["x_ctrv"][4]) * 6000.0 > 64 * np.pi for s in pre)
        T.close()
    assert hit_ego and hit_dt


def blinking_world(seed, spots, frames):
    """objects that appear at fixed spots of a lattice, drift a little, vanish, and come back: the tracks of a spot die and new ones
    are born where dead ones lie — over a long run far more tracks are created than are ever alive, and a new track's visible box
    regularly contains the last position of a dead one (the reference's merge step looks at those too, imm_ukf_jpda.cpp:666-700)"""
    import test_emu_tracker_random as TR
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(spots)))
    centre = (np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)[:spots] - side / 2) * 7.0 + rng.uniform(-1, 1, (spots, 2))
    state = np.zeros(spots, np.int64)           # > 0: frames the object stays; < 0: frames until it is back
    state[:] = rng.integers(1, 40, spots) * np.where(rng.random(spots) < 0.7, 1, -1)
    drift = rng.uniform(-0.6, 0.6, (spots, 2)); size = rng.uniform(0.8, 4.5, (spots, 2)); yaw = rng.uniform(-3, 3, spots)
    age = np.zeros(spots)
    for f in range(frames):
        boxes = []
        for k in range(spots):
            if k % 3 == 0:
                # Every third spot replays, with a period of 200 frames, the one situation in which a DEAD track changes a live one's fate in
                # the reference (mergeOverSegmentation runs over every track ever created, imm_ukf_jpda.cpp:666-700): a small object D lives
                # and dies at (2, 0.9); later a large static object A stands over the spot and a long object B drives into A's box from the
                # right. B's centre inside A's visible box would merge B away (A is older) — unless B's own box holds some track's position:
                # D's last position does that job for a while. An implementation that forgets dead tracks kills B the moment it enters.
                t = (f + 37 * k) % 200
                c0 = centre[k] + rng.normal(0, 0.01, 2)
                if t < 25:
                    boxes.append(TR.box(c0[0] + 2.0, c0[1] + 0.9, 1.0, 1.0, 0.0, -0.3))
                if 40 <= t < 190:
                    boxes.append(TR.box(c0[0], c0[1], 3.0, 6.0, 0.0, -0.3))                                # A: x in [-3, 3], y in [-1.5, 1.5]
                if 42 <= t < 190:
                    boxes.append(TR.box(c0[0] + 8.0 - 0.06 * (t - 42), c0[1] + 0.9, 1.0, 3.0, 0.0, -0.3))   # B: 3 m long, 1 m wide, moving left
                continue
            if state[k] > 0:
                p = centre[k] + drift[k] * 0.1 * age[k] + rng.normal(0, 0.03, 2)
                boxes.append(TR.box(p[0], p[1], size[k, 0], size[k, 1], yaw[k] + rng.normal(0, 0.02), -0.3))
                age[k] += 1; state[k] -= 1
                if state[k] == 0:
                    state[k] = -int(rng.integers(4, 30)); age[k] = 0; drift[k] = rng.uniform(-0.6, 0.6, 2)
            else:
                state[k] += 1
                if state[k] == 0:
                    state[k] = int(rng.integers(12, 70))
        if rng.random() < 0.2:
            boxes.append(TR.box(*rng.uniform(-30, 30, 2), *rng.uniform(0.5, 2.5, 2), rng.uniform(-3, 3), -0.2))   # clutter
        yield np.array(boxes, np.float32).reshape(-1, 8, 3), 1.0e9 + f * 1.0e5, 1.0 + 0.5 * np.sin(0.01 * f), 0.0005 * f


def fast_lanes(seed, frames, lanes=5, speeds=(10.3, 11.5), turns=(0.3, 1.2), start=(5.0, 7.0)):
    """objects on lanes 15 m apart that drive along x through the origin at 10.3 .. 11.5 m/s (more than a metre a frame; meant for a dozen frames: near the
    origin an fp32 ulp of x is small against the step, so a last bit of a coordinate moves the estimated speed by less than 1e-6 of it), their boxes turned against the direction of
    travel by up to 1.2 rad: once such a track is confirmed, the box inside its gate lies MORE than 1 m from the track's last position — the
    situation in which distance_thres decides whether the track takes the box over (getNearestEuclidBBox, imm_ukf_jpda.cpp:396-463) — and
    the box's yaw differs from the track's by more than the preset's bb_yaw_change_thres"""
    import test_emu_tracker_random as TR
    rng = np.random.default_rng(seed)
    sign = np.where(rng.random(lanes) < 0.5, -1.0, 1.0)
    speed = rng.uniform(speeds[0], speeds[1], lanes) * sign
    x0 = -sign * rng.uniform(start[0], start[1], lanes); y0 = (np.arange(lanes) - lanes / 2) * 15.0 + rng.uniform(-2, 2, lanes)
    turn = rng.uniform(turns[0], turns[1], lanes) * np.where(rng.random(lanes) < 0.5, -1.0, 1.0)
    size = rng.uniform(1.5, 4.5, (lanes, 2))
    for f in range(frames):
        # every fourth frame a lane's box arrives smaller and turned by half a radian (a partial view): the frame-to-frame yaw change that
        # bb_yaw_change_thres judges (updateBB, imm_ukf_jpda.cpp:565-653) lies between the preset's 0.2 rad and pi / 2
        part = [f >= 6 and f % 4 == k % 4 for k in range(lanes)]
        boxes = [TR.box(x0[k] + speed[k] * 0.1 * f + rng.normal(0, 0.02), y0[k] + rng.normal(0, 0.02), size[k, 0] * (0.9 if part[k] else 1.0), size[k, 1] * (0.9 if part[k] else 1.0),
                        (0.0 if sign[k] > 0 else np.pi) + turn[k] + (0.5 if part[k] else 0.0) + rng.normal(0, 0.01), -0.3) for k in range(lanes)]
        yield np.array(boxes, np.float32).reshape(-1, 8, 3), 1.0e9 + f * 1.0e5, 0.0, 0.0


def long_run_bounded_slots(mot, oracle, lib_path=None, frames=1500, slots=16, spots=10, seed=3, state_every=25, min_ever_factor=4, max_chaos_restarts=0,
                           ref_frames=500):
    """SURVEY.md H14 / the reference never frees a track: a long run on `slots` track slots must give what the oracle gives with
    unbounded memory — every frame the discrete outputs of EVERY track ever created (reference index order), every `state_every`
    frames the filter states of the live ones — while far more tracks are created than there are slots.

    max_chaos_restarts (the MI355X run; 0 on the emulator, whose arithmetic is the oracle's up to operation order): the reference's
    filter diverges now and then (a covariance that stops being positive definite; its own guards kill the track a few frames
    later). While it lasts, the track's state is numerical noise — last-bit differences of the device's sin / cos / exp grow to
    O(1) within three frames (the same run on the emulator with those functions perturbed by one ulp, MOT_EMU_PERTURB, parts
    from the oracle at exactly the same frame) — and when such a track's gate decides about a box, the noise becomes a discrete
    difference (a birth more or less). That is the reference's chaos, not a property of the implementation: a discrete mismatch
    is accepted ONLY while the oracle has a live track that is or was ill-conditioned within the last 30 frames, both sides are
    then started over, and the number of such restarts is bounded."""
    if hasattr(oracle, "restatement"):
        # The GPU suite's oracle is the reference build first (oracle_lib.RefFirst) — not here: the reference's tracker never frees a track and
        # walks all of them every frame, so thousands of frames with thousands of tracks ever created cost minutes of host time (5 min for the
        # two long runs on the GPU box, measured in round 4) where the restatement takes seconds; and this world is chaos by construction —
        # two builds of the REFERENCE part discretely within a few hundred frames of it (tests/test_tracker_noise_floor.py: the floor's
        # replicas are retired at frame 45-399 of a blinking world), so "equal to libmot_ref.so for 10 000 frames" is not a property any
        # second implementation, or any second compilation of the first, has. The restatement is pinned to libmot_ref.so on CPU
        # (tests/test_oracle_vs_ref.py), and every other tracker test of the GPU suite runs against libmot_ref.so itself.
        oracle = oracle.restatement("Tracker", "long chaotic run: the reference's tracker is O(tracks ever) per frame, and its own rebuilds part discretely in this world")
    p = oracle.params(0)
    kw = dict(lib_path=lib_path) if lib_path else {}
    stats = {"chaos_restarts": 0, "frames_compared": 0}
    taint = {}
    ever_total = 0
    # THE REFERENCE'S OWN BUILD for the head of the run (round-4 review: these runs never met the reference's code on the GPU box): for the
    # first `ref_frames` frames — while the tracks ever created are few and its O(tracks ever) step is cheap — oracle/_ref/libmot_ref.so
    # (and its -DEIGEN_DONT_VECTORIZE rebuild) are stepped beside the restatement. Their DISCRETE outputs must equal the restatement's (a
    # replica that parts from it is chaos reaching a gate decision: it is retired and the frame recorded), and their state differences are
    # the noise floor the device's states are held against under the NARROW criterion on those frames (assert: every live track-frame
    # within 1e-4, or within 10 x the reference's own noise there). Beyond ref_frames: the wide criterion at 1e-2, see below.
    floor = None
    if ref_frames and getattr(oracle, "ref", lambda: None)() is not None:
        floor = SP.NoiseFloor(oracle, p, primary_is_ref=False, instance=3, kinds=("ref", "novec"))
        stats["reference_builds_stepped"] = floor.names()
    with mot.Context(max_points=1024, max_tracks_total=slots, **kw) as c:
        T = oracle.Tracker(p)
        o = None
        for f, (boxes, ts, v, yaw) in enumerate(blinking_world(seed, spots, frames)):
            assert np.allclose(c.ego_update(ts, v, yaw), T.ego_update(ts, v, yaw), rtol=1e-12, atol=1e-12)
            a = c.track_step(boxes, ts); o_prev = o; o = T.step(boxes, ts, max_tracks=1 << 16)
            assert not a["capacity_exceeded"], f
            if floor is not None:
                if f < ref_frames and floor.reps:
                    floor.step(boxes, ts, v, yaw, o, f)
                    stats["reference_frames"] = f + 1
                else:
                    stats["reference_builds_retired_at"] = dict(floor.retired); floor.close(); floor = None
            equal = a["n"] == o["n"] and all(np.array_equal(a[k], o[k]) for k in ("track_manage", "is_static", "is_vis", "lifetime"))
            if not equal:
                chaotic = any(until >= f - 1 for until in taint.values())
                assert chaotic and stats["chaos_restarts"] < max_chaos_restarts, (f, a["n"], o["n"], "discrete outputs differ", "oracle has a diverging track" if chaotic else "NO diverging track")
                stats["chaos_restarts"] += 1; ever_total += o["n"]
                c.reset(); T.reset(); taint.clear(); o = None
                continue
            stats["frames_compared"] += 1
            live = o["track_manage"] > 0
            dead = ~live
            assert np.array_equal(a["vis_box"][dead & (o["is_vis"] == 0)], o["vis_box"][dead & (o["is_vis"] == 0)])
            SP.note_conditioning(o, T.state, f, taint, criterion="wide")
            if f % state_every == 0 or f == frames - 1:
                # continuous values: filter states of the live tracks (a track that is or recently was diverging is compared in its discrete
                # outputs only: seq_parity.well_conditioned / note_conditioning), and the last positions the dead tracks left behind (the
                # merge step keeps reading them)
                # (rtol 1e-2 here, not the 1e-4 of the sequence tests: this world is built to stress the track BOOKKEEPING — overlapping
                # boxes, tracks driven into each other for thousands of frames — and keeps long-lived filters loose (yaw-rate variances
                # of 5-6 (rad/s)^2) or lets them pass through short indefinite phases; such a filter carries the device's last-bit
                # differences at the 1e-3 level long after its covariance looks sane again. The discrete outputs of every track ever
                # created, compared exactly on every frame, are what this test is about.)
                # criterion "wide" + the 30-frame conditioning memory: THIS world needs them, the rendered streams do not. With the narrow
                # criterion the MI355X run of round 4 (gpurun session r4s1) failed here at frame 2900 on a track with yaw / yaw-rate variances
                # of 11.3 / 10.4 (rad)^2 — a filter that is alive by every test of the reference and a random walk in yaw — by 1.7e-2 in
                # p_merge. The counts per criterion are in stats["set_aside_by"].
                SP.compare_tracks(a, o, c.track_state, T.state, f, rtol=1e-2, stats=stats, skip_ill_conditioned=True, taint=taint, frame=f, criterion="wide")
            if floor is not None and floor.reps and (f % 5 == 0):   # the head of the run, against the reference's own builds: narrow criterion + noise floor
                head = stats.setdefault("head", {})
                # (assert_floor: a track-frame above 1e-4 — set aside or not — fails unless the reference's own builds differ about as much there.
                # On the MI355X this world does produce a few well-conditioned track-frames at 2-3e-4: loose filters, where libmot_ref.so and
                # its -DEIGEN_DONT_VECTORIZE rebuild are 1.7-1.9e-4 apart themselves — counted in head["above_bar_well_conditioned"], reported.)
                SP.compare_tracks(a, o, c.track_state, T.state, f, rtol=float("inf"), stats=head, criterion="narrow", floor=floor.floor, assert_floor=True)
                for i in np.nonzero(dead)[0][-64:]:
                    if SP.well_conditioned(T.state(int(i)), "wide") and taint.get(int(i), -1) < 0:
                        assert np.allclose(a["p"][i][:2], o["p"][i][:2], rtol=1e-2, atol=1e-4), (f, int(i), "position of a dead track")
                        # ... and its frozen speed / (frozen yaw + the current ego yaw), which the reference keeps reporting (imm_ukf_jpda.cpp:1012-1016)
                        dv = np.abs(a["v_yaw"][i] - o["v_yaw"][i]); dv[1] = min(dv[1], abs(2 * np.pi - dv[1]))   # (a yaw at +-pi may wrap either way)
                        assert np.all(dv <= 1e-2 * np.maximum(np.abs(o["v_yaw"][i]), 1.0)), (f, int(i), "v / yaw of a dead track", a["v_yaw"][i], o["v_yaw"][i])
            stats["live_peak"] = max(stats.get("live_peak", 0), int(live.sum()))
        ever_total += o["n"] if o is not None else 0
        T.close()
        if floor is not None:
            stats["reference_builds_retired_at"] = dict(floor.retired); floor.close()
    if "head" in stats:
        h = stats.pop("head")
        stats["head_vs_reference_builds"] = {k: h.get(k) for k in ("state_compares", "max_rel_state_err", "above_bar", "above_bar_well_conditioned", "ill_conditioned", "unexplained") if k in h}
        stats["head_vs_reference_builds"]["noise_floor_max"] = max([x for x in h.get("floors", []) if np.isfinite(x)] + [0.0])
    assert ever_total >= min_ever_factor * slots and stats["live_peak"] <= slots, (ever_total, stats)
    stats["tracks_ever"] = ever_total
    return stats


# ---------------------------------------------------------------------------------------------------------------------------------
# Many streams in ONE context: the step as four launches (track_prep -> track_predict -> track_update [+ track_update_dense] -> track_finish,
# csrc/track.hip mot_launch_track), the live tracks of all streams dealt over the chip through one work list. Contexts of more than
# MOT_STREAM_KERNEL_MAX_BATCH = 32 streams take that path under AUTO; the bodies below never set a mode.

DENSE_TRACKS = 24576   # MOT_UPDATE_DENSE_TRACKS of the default build (csrc/track.hip): n_items >= this -> the dense update instantiation works


class StreamPlan:
    """what ONE stream of a many-stream run is fed: `nbox` boxes of grid_boxes(spacing) from frame `start` on (none before), drawn from
    default_rng(seed) the way many_live_tracks draws them; `resets`: frames before whose step the stream's tracks are forgotten
    (mot_reset_tracks_slot / the oracle's reset); `dup`: the frame that repeats its predecessor's timestamp (dt = 0); `skips`: frames on
    which the stream is not part of the call at all (neither side is stepped, its clock stands still)"""

    def __init__(self, kind, nbox, spacing=9.0, seed=0, start=0, resets=(), dup=None, skips=()):
        self.kind, self.nbox, self.spacing, self.seed, self.start = kind, int(nbox), float(spacing), int(seed), int(start)
        self.resets, self.dup, self.skips = frozenset(resets), dup, frozenset(skips)

    def key(self):
        """the schedule without the seed: what a seed is selected FOR (tools: tests/golden/make_stream_seeds.py)"""
        return (self.nbox, self.spacing, self.start, tuple(sorted(self.resets)), self.dup, tuple(sorted(self.skips)))

    def boxes(self, frames):
        rng = np.random.default_rng(self.seed)
        n = max(self.nbox, 1)
        vel = rng.uniform(-1.0, 1.0, size=(1, n, 2))
        out = [grid_boxes(1, n, f, vel, rng, self.spacing)[0] for f in range(frames)]   # (drawn for every frame: a late start does not shift the sequence)
        return [b[: self.nbox if f >= self.start else 0] for f, b in enumerate(out)]

    def timestamps(self, frames):
        ts = [1.0e9 + f * 1.0e5 for f in range(frames)]
        if self.dup is not None:
            ts[self.dup] = ts[self.dup - 1]
        return ts


def replay_on_oracle(plan, frames, tracker, on_frame=None):
    """the stream's exact schedule on one oracle tracker; -> live count after every frame (None where the stream did not run)"""
    bx, ts = plan.boxes(frames), plan.timestamps(frames)
    live = []
    for f in range(frames):
        if f in plan.skips:
            live.append(None); continue
        if f in plan.resets:
            tracker.reset()
        tracker.ego_update(ts[f], 0.0, 0.0)
        o = tracker.step(bx[f], ts[f], max_tracks=1024)
        live.append(int((o["track_manage"] != 0).sum()))
        if on_frame is not None:
            on_frame(f, o)
    return live


def _compare_records(a, o, where, rtol=SP.RTOL):
    """discrete outputs exact, NaN patterns equal, the records of the live tracks (position, speed / yaw, visible box) within rtol of the
    vector they belong to — seq_parity.compare_tracks's output checks for a whole stream at once, without the per-track state fetch"""
    assert a["n"] == o["n"], (where, a["n"], o["n"])
    for k in ("track_manage", "is_static", "is_vis"):
        assert np.array_equal(a[k], o[k]), (where, k, np.nonzero(a[k] != o[k])[0][:8])
    if "lifetime" in o:
        assert np.array_equal(a["lifetime"], o["lifetime"]), (where, "lifetime")
    live = o["track_manage"] > 0
    for key, atol in (("p", 1e-6), ("v_yaw", 1e-7), ("vis_box", 1e-5)):
        av, ov = np.asarray(a[key], np.float64)[live], np.asarray(o[key], np.float64)[live]
        nan = np.isnan(ov)
        assert np.array_equal(nan, np.isnan(av)), (where, key, "NaN pattern")
        if av.size:
            scale = np.nanmax(np.where(nan, 0.0, np.abs(ov)), axis=1, keepdims=True)
            bad = np.where(nan, 0.0, np.abs(av - ov)) > rtol * scale + atol
            assert not bad.any(), (where, key, np.nonzero(bad.any(axis=1))[0][:8])
    return int(live.sum())


def run_stream_plans(mot, oracle, to_dev, plans, frames, lib_path=None, slots=64, full_every=5, always=(), mode=None, short_call=None):
    """`plans[s]` on slot s of ONE context through mot_track_steps_dev, one oracle tracker per stream, stepped ONE AFTER ANOTHER while the device works: the
    reference build is not re-entrant even across its private library copies (oracle/ref_capi.cpp's Quiet swaps the process-wide std::cout buffer for a
    stack-local sink; stepping copies from a thread pool crashed the host in exactly that, on the first run of this body) — 4 ms a step, 37 s for the largest case. Every stream on every frame: discrete outputs exact and the track records within the bar
    (_compare_records); the full filter state of every live track (seq_parity.compare_tracks, every STATE_KEY) on every `full_every`-th
    frame and the last, and on every frame for the streams in `always`. Streams of spacing < 6 m (shared gates) are compared with
    skip_ill_conditioned exactly as many_live_tracks does, and always in full; no other stream has anything set aside — asserted by the callers
    through stats["ill_conditioned_9m"]. short_call = (frame, k): on that frame the call covers all but the last k streams (their plans
    must list the frame in `skips`).
    -> stats: n_items[f] (the work-list length of step f, from the oracles' live counts: a stream contributes what it held after its
    previous step, nothing on a first frame or when it does not run), live_total[f], live_by_kind, resets, state_compares, ..."""
    B = len(plans)
    p = oracle.params(0)
    kw = dict(lib_path=lib_path) if lib_path else {}
    boxes = [pl.boxes(frames) for pl in plans]
    tss = [pl.timestamps(frames) for pl in plans]
    maxbox = max(max(pl.nbox for pl in plans), 1)
    stride = maxbox * 24
    always = set(always) | {s for s, pl in enumerate(plans) if pl.spacing < 6}
    stats, stats2m = {}, {}
    n_items, live_total, resets = [], [], 0
    held = [0] * B            # live-list length each stream holds (what its next step contributes to the work list)
    fresh = [True] * B        # the next step of the stream is a first frame
    live_by_kind, peak_by_stream = {}, [0] * B
    records_compared = 0
    with mot.Context(max_points=1024, max_batch=B, max_tracks_total=slots, **kw) as c:
        if mode is not None:
            c.set_tracker_mode(mode)
        Ts = [oracle.Tracker(p) for _ in range(B)]
        try:
            for f in range(frames):
                nb = B - short_call[1] if short_call and short_call[0] == f else B
                run = [s < nb for s in range(B)]
                for s, pl in enumerate(plans):
                    assert (f in pl.skips) == (not run[s]), (f, s, "plan and call disagree about who runs")
                    if f in pl.resets:
                        c.reset_tracks_slot(s); Ts[s].reset(); fresh[s] = True; held[s] = 0; resets += 1
                n_items.append(sum(held[s] for s in range(B) if run[s] and not fresh[s]))
                host = np.zeros((B, stride), np.float32)
                m = [len(boxes[s][f]) for s in range(B)]
                for s in range(B):
                    host[s, : m[s] * 24] = boxes[s][f].reshape(-1)
                ptr, free = to_dev(host)
                egos = [c.ego_update(tss[s][f], 0.0, 0.0, s) for s in range(nb)]
                c.track_steps_dev(ptr, stride, m[:nb], [tss[s][f] for s in range(nb)])

                def orc_step(s):
                    e = Ts[s].ego_update(tss[s][f], 0.0, 0.0)
                    return e, Ts[s].step(boxes[s][f], tss[s][f], max_tracks=1024)
                outs = [orc_step(s) for s in range(nb)]
                full_frame = f % full_every == 0 or f == frames - 1
                tot = 0
                for s in range(nb):
                    e, o = outs[s]
                    # (the oracle has no tracks-only reset: its reset() also starts the ego dead reckoning over, and getOriginPoints' first call reports the
                    # first-frame yaw offset. The ego stands still here (v = 0, yaw = 0), so the origin of the global frame is the same on both sides, and
                    # the one record a first frame writes — the seed track's — does not depend on the ego yaw. From the next frame on the poses must be equal again.)
                    assert np.array_equal(e, egos[s]) or f in plans[s].resets, (f, s, "ego pose", e, egos[s])
                    a = c.get_tracks(s)
                    assert not a["capacity_exceeded"], (f, s)
                    if full_frame or s in always:
                        two_m = plans[s].spacing < 6
                        SP.compare_tracks(a, o, lambda i: c.track_state(i, slot=s), Ts[s].state, (f, s, plans[s].kind), stats=stats2m if two_m else stats, skip_ill_conditioned=two_m)
                    else:
                        _compare_records(a, o, (f, s, plans[s].kind))
                    records_compared += int((o["track_manage"] > 0).sum())
                    held[s] = int((o["track_manage"] != 0).sum()); fresh[s] = False
                    peak_by_stream[s] = max(peak_by_stream[s], held[s])
                    tot += held[s]
                tot += sum(held[s] for s in range(nb, B))
                live_total.append(tot)
                free()
        finally:
            for T_ in Ts:
                T_.close()
    for s, pl in enumerate(plans):
        k = live_by_kind.setdefault(pl.kind, dict(streams=0, peak_min=1 << 30, peak_max=0))
        k["streams"] += 1; k["peak_min"] = min(k["peak_min"], peak_by_stream[s]); k["peak_max"] = max(k["peak_max"], peak_by_stream[s])
    return dict(n_items=n_items, live_total=live_total, resets=resets, live_by_kind=live_by_kind, records_compared=records_compared,
                state_compares=stats.get("state_compares", 0) + stats2m.get("state_compares", 0), ill_conditioned_9m=stats.get("ill_conditioned", 0),
                ill_conditioned_2m=stats2m.get("ill_conditioned", 0), max_rel_state_err=stats.get("max_rel_state_err", 0.0),
                max_rel_state_err_2m=stats2m.get("max_rel_state_err", 0.0), streams=B, frames=frames)


STREAM_SEEDS = "stream_seeds.json"   # tests/golden: the selected seeds of the 9 m streams, per case and schedule (tests/golden/make_stream_seeds.py)


def fixture_seeds(case):
    """-> next_seed(plan_key): the committed seeds for the streams of `case`, in order; running out of them is an error (a plan that
    changed needs its seeds selected again: the seed list changes, never the bar)"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", STREAM_SEEDS)) as fh:
        table = json.load(fh)[case]
    taken = {}

    def next_seed(key):
        k = repr(key)
        i = taken.get(k, 0); taken[k] = i + 1
        assert k in table and i < len(table[k]), ("no selected seed left for schedule", k, "of", case, ": run tests/golden/make_stream_seeds.py")
        return table[k][i]
    return next_seed


def _seeded(plans, next_seed):
    """the 9 m streams get selected seeds (per schedule); the 2 m and the empty streams keep the fixed ones they were planned with"""
    for pl in plans:
        if pl.spacing >= 6 and pl.nbox > 0:
            pl.seed = next_seed(pl.key())
    return plans


WIDE_SIZES = {
    # streams of each kind; boxes of a "full" stream; frames; the frame of the partial reset, of the repeated timestamp, of the short call
    "gpu": dict(empty=6, one=6, eight=10, crowded=6, late=40, full=188, nbox=64, frames=16, reset_at=9, dup_at=6, short_at=12, short_k=5, late_start=3, slots=128),
    "emu": dict(empty=2, one=2, eight=4, crowded=2, late=6, full=24, nbox=16, frames=12, reset_at=7, dup_at=5, short_at=9, short_k=3, late_start=3, slots=32),
}


def wide_batch_plans(size, next_seed):
    """streams of very different sizes side by side, interleaved over the slots (kinds alternate, so one wave's four work items regularly
    belong to different streams and kinds), ragged in time: `late` streams get their first boxes `late_start` frames after the others; at
    `reset_at` every 6th full stream, one one-box, one eight-box and one crowded stream are reset while the rest carry on; one full stream
    repeats a timestamp at `dup_at`; at `short_at` the call leaves the last `short_k` streams (full ones) out."""
    z = WIDE_SIZES[size]
    kinds = ["empty"] * z["empty"] + ["one"] * z["one"] + ["eight"] * z["eight"] + ["crowded"] * z["crowded"] + ["late"] * z["late"] + ["full"] * (z["full"] - z["short_k"])
    order = np.random.default_rng(2024).permutation(len(kinds))
    kinds = [kinds[i] for i in order] + ["full"] * z["short_k"]
    plans, seen = [], {}
    for s, kind in enumerate(kinds):
        j = seen.get(kind, 0); seen[kind] = j + 1
        last = s >= len(kinds) - z["short_k"]
        resets = (z["reset_at"],) if (kind == "full" and j % 6 == 1 and not last) or (kind in ("one", "eight", "crowded") and j == 1) else ()
        nbox = dict(empty=0, one=1, eight=(7, 9, 8)[j % 3], crowded=z["nbox"], late=z["nbox"], full=z["nbox"])[kind]
        plans.append(StreamPlan(kind, nbox, spacing=2.0 if kind == "crowded" else 9.0, seed=500 + s, start=z["late_start"] if kind == "late" else 0, resets=resets,
                                dup=z["dup_at"] if kind == "full" and j == 0 else None, skips=(z["short_at"],) if last else ()))
    return _seeded(plans, next_seed)


def wide_batch(mot, oracle, to_dev, lib_path=None, size="gpu", next_seed=None):
    """The four-launch tracker step against one oracle tracker per stream, AUTO mode (more than 32 streams: the product's own switch picks the
    launches). See wide_batch_plans for what runs side by side and run_stream_plans for what is compared. Asserts what the run exercised."""
    z = WIDE_SIZES[size]
    plans = wide_batch_plans(size, next_seed or fixture_seeds("wide_" + size))
    B, nbox, frames = len(plans), z["nbox"], z["frames"]
    assert B > 32
    always = [next(s for s, pl in enumerate(plans) if pl.kind == k) for k in ("empty", "one", "eight", "crowded", "late", "full")]
    always += [s for s, pl in enumerate(plans) if pl.resets or pl.dup is not None or pl.skips][:8]
    always += [s for s in range(B) if s not in always][: max(0, 16 - len(set(always)))]
    st = run_stream_plans(mot, oracle, to_dev, plans, frames, lib_path=lib_path, slots=z["slots"], full_every=5, always=always, short_call=(z["short_at"], z["short_k"]))
    st["always"] = len(set(always))
    k = st["live_by_kind"]
    # what the run exercised — a comparison that silently went empty fails here
    assert k["empty"]["streams"] == z["empty"] and k["empty"]["peak_max"] == 0, k            # the empty streams stayed empty
    assert k["one"]["peak_min"] == 1 and k["one"]["peak_max"] == 1, k
    assert 7 <= k["eight"]["peak_min"] and k["eight"]["peak_max"] <= 9, k
    assert k["full"]["peak_min"] == nbox and k["late"]["peak_min"] == nbox, k
    assert k["crowded"]["peak_min"] >= nbox // 4, k
    n_full = z["full"] + z["late"]
    assert max(st["live_total"]) >= n_full * nbox and max(st["n_items"]) >= n_full * nbox, st["live_total"]
    n_reset = sum(1 for pl in plans if pl.resets)
    assert st["resets"] == n_reset and n_reset >= 4, st["resets"]
    odd = sum(1 for n in st["n_items"] if n % 8 and n % 64)
    assert odd > frames // 2, st["n_items"]                                                    # a ragged tail in the last wave on most frames
    assert st["ill_conditioned_9m"] == 0, st                                                     # selected seeds: nothing of a 9 m stream is set aside
    assert st["max_rel_state_err"] <= SP.RTOL
    always_min = sum(1 for f in range(frames) for s in set(always) if f not in plans[s].skips and plans[s].nbox and f > plans[s].start + 1) * 1
    assert st["state_compares"] >= 4 * (n_full - z["short_k"]) * nbox + always_min, st["state_compares"]   # >= 4 full frames of every full stream + the always-streams
    assert st["records_compared"] >= (frames - 6) * (n_full - z["short_k"]) * nbox, st["records_compared"]
    return st


DENSE_PLAN = dict(streams=512, nbox=64, frames=18, odd_stream=350, odd_nbox=63,
                  # frame -> the streams whose tracks are forgotten before it
                  resets={4: range(0, 200), 8: range(200, 350), 11: range(350, 478), 14: range(0, 128)})
# n_items of every step with the canonical live counts (a stream holds 1 track after a first frame, its box count after that — the seeds are
# selected for exactly that, make_stream_seeds.py): 511 x 64 + 63 = 32767 when everything runs at full size
DENSE_N_ITEMS = [0, 512, 32767, 32767,
                 312 * 64 - 1, 312 * 64 - 1 + 200, 32767, 32767,        # 200 streams reset: below, below, above again
                 362 * 64 - 1, 362 * 64 - 1 + 150, 32767,                # another 150: below (23167, 23317), above
                 384 * 64, 384 * 64 + 128, 32767,                        # 128 reset, the 63-box stream among them: EXACTLY 24576 -> the dense kernel's first count
                 383 * 64 + 63, 383 * 64 + 63 + 128, 32767, 32767]       # 128 others: 24575 -> the plain kernel's last count


def dense_threshold_plans(next_seed):
    d = DENSE_PLAN
    plans = []
    for s in range(d["streams"]):
        resets = [f for f, who in d["resets"].items() if s in who]
        plans.append(StreamPlan("odd" if s == d["odd_stream"] else "full", d["odd_nbox"] if s == d["odd_stream"] else d["nbox"], seed=s, resets=resets))
    return _seeded(plans, next_seed)


def dense_threshold(mot, oracle, to_dev, lib_path=None, next_seed=None):
    """The default build's switch between track_update_kernel and track_update_dense_kernel (n_items < / >= MOT_UPDATE_DENSE_TRACKS = 24576, decided
    on the device), crossed back and forth in one run of 512 streams x 64 track slots under AUTO: above, below, above, below, above, EXACTLY
    24576 (the dense kernel's first count), above, 24575 (the plain kernel's last). An off-by-one in `n < lo || n >= hi` leaves every track of
    such a frame without its update, or updates it twice. The planned n_items sequence is asserted from the oracles' own live counts."""
    plans = dense_threshold_plans(next_seed or fixture_seeds("dense"))
    d = DENSE_PLAN
    always = [0, 127, 128, 199, 200, 349, 350, 351, 477, 478, 500, 511, 64, 300, 400, 490]
    st = run_stream_plans(mot, oracle, to_dev, plans, d["frames"], lib_path=lib_path, slots=64, full_every=5, always=always)
    assert st["n_items"] == DENSE_N_ITEMS, st["n_items"]
    sides = [n >= DENSE_TRACKS for n in st["n_items"]]
    assert sides == [False, False, True, True, False, False, True, True, False, False, True, True, True, True, False, True, True, True]
    assert DENSE_TRACKS in st["n_items"] and DENSE_TRACKS - 1 in st["n_items"]
    assert st["resets"] == 200 + 150 + 128 + 128
    assert st["ill_conditioned_9m"] == 0 and st["ill_conditioned_2m"] == 0, st
    assert st["max_rel_state_err"] <= SP.RTOL
    assert st["state_compares"] >= 4 * 300 * 64 + 16 * 14 * 60, st["state_compares"]
    assert st["records_compared"] >= 12 * 32767, st["records_compared"]
    return st


# ---------------------------------------------------------------------------------------------------------------------------------
# The same bits from the three instantiations of the step: the stream kernel (one launch), the four launches with the plain update, and the four
# launches with the dense update. The source promises it ("Same arithmetic, same results (-ffp-contract=off: a spill changes no rounding)").

class RecordingPkg:
    """the package with every new Context put into one tracker launch mode (and, optionally, one library), every track_step / get_tracks / track_state
    result appended to `log`: for bodies that create their own contexts"""

    def __init__(self, mot, mode, log=None, lib_path=None):
        self._mot, self._mode, self._log, self._lib = mot, mode, log, lib_path

    def __getattr__(self, k):
        return getattr(self._mot, k)

    def Context(self, *a, **kw):
        if self._lib:
            kw["lib_path"] = self._lib
        c = self._mot.Context(*a, **kw); c.set_tracker_mode(self._mode)
        if self._log is not None:
            for name in ("track_step", "get_tracks", "track_state"):
                def wrap(fn):
                    def call(*aa, **kk):
                        r = fn(*aa, **kk); self._log.append(r); return r
                    return call
                setattr(c, name, wrap(getattr(c, name)))
        return c


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)   # (NaN outputs of a diverged track must be the same NaNs)


def assert_logs_bit_identical(la, lb, what):
    """two RecordingPkg logs of the same calls: every output and every state key bit for bit, NaNs included"""
    assert len(la) == len(lb) and len(la) > 0, (what, len(la), len(lb))
    n_state = 0
    for i, (ra, rb) in enumerate(zip(la, lb)):
        assert ra.keys() == rb.keys(), (what, i)
        for k in ra:
            if k in ("capacity_exceeded",):
                assert ra[k] == rb[k], (what, i, k)
            else:
                assert np.array_equal(_bits(np.asarray(ra[k])), _bits(np.asarray(rb[k]))), (what, i, k)
        n_state += "x_merge" in ra
    return n_state


def launch_modes_identical(mot, oracle, to_dev, lib_path=None):
    """mot_set_tracker_mode: the step as four launches (MOT_TRACKER_SPLIT: tracks of all streams dealt over the chip — what the 512-stream contexts run) and as
    ONE launch with a workgroup per stream (MOT_TRACKER_STREAM: what contexts of few streams run) must give the same bits: same phases, same order per track,
    kernel boundaries replaced by workgroup barriers. Random and degenerate sequences on three streams at once, then 40 live tracks per stream through the
    batched device entry point (more than one round of 32 groups in the stream kernel) — that part also against the oracle, in both modes."""
    import test_emu_tracker_random as TR
    logs, many = {}, {}
    for mode in (mot.MOT_TRACKER_SPLIT, mot.MOT_TRACKER_STREAM):
        log = logs[mode] = []
        pkg = RecordingPkg(mot, mode, log, lib_path)
        with pkg.Context(max_points=1024, max_batch=3, max_tracks_total=256) as c:
            seqs = [TR.sequence(70 + k, frames=20) if k < 2 else TR.hostile_sequence(5, frames=20) for k in range(3)]
            for f in range(20):
                for s in range(3):
                    boxes, ts, v, yaw = seqs[s][f]
                    c.ego_update(ts, v, yaw, s)
                    tr = c.track_step(boxes, ts, s)
                    for i in np.nonzero(tr["track_manage"] > 0)[0]:
                        c.track_state(int(i), slot=s)
        many[mode] = many_live_tracks(pkg, oracle, to_dev, streams=2, T=40, frames=14, spacing=9.0, min_live=40)
    n_state = assert_logs_bit_identical(logs[mot.MOT_TRACKER_SPLIT], logs[mot.MOT_TRACKER_STREAM], "split vs stream")
    assert n_state >= 2 * 12 * 40 + 100, n_state
    assert many[mot.MOT_TRACKER_SPLIT]["max_rel_state_err"] == many[mot.MOT_TRACKER_STREAM]["max_rel_state_err"]
    return dict(states_compared=n_state, calls=len(logs[mot.MOT_TRACKER_SPLIT]))


def dense_variant_identical(mot, oracle, to_dev, lib_default, lib_dense4, golden, frames=30):
    """A library built with -DMOT_UPDATE_DENSE_TRACKS=4 against the default one, both in MOT_TRACKER_SPLIT mode on the same inputs: in the variant every step with
    >= 4 live tracks goes through track_update_dense_kernel (on the MI355X: the instantiation held to 3 waves per SIMD, which spills), in the default library
    the plain kernel does all the work. The golden tracker sequences cross the threshold back and forth (checked against the fixtures' reference values at the bar),
    the 64-live-track case sits far above it (checked against the oracle at the bar); all outputs and all states of the two libraries bit for bit."""
    import golden_util as G
    logs = {}
    crossings = 0
    for tag, lib in (("default", lib_default), ("dense4", lib_dense4)):
        log = logs[tag] = []
        pkg = RecordingPkg(mot, mot.MOT_TRACKER_SPLIT, log, lib)
        for name in golden:
            fx = G.load(name)
            side = []
            with pkg.Context(max_points=4096, max_tracks_total=256) as c:
                for f in range(len(fx["n_boxes"])):
                    ts = 1.0e9 + f * float(fx["unit"])
                    c.ego_update(ts, *G.ego_of(fx, f))
                    side.append(int((c.get_tracks(0)["track_manage"] != 0).sum()) >= 4 if f else False)   # the live list this step starts from
                    out = c.track_step(fx["boxes"][f][: fx["n_boxes"][f]], ts)
                    G.check_tracker_frame(fx, f, out, lambda i: c.track_state(i), rtol=SP.RTOL)
            crossings += sum(1 for x, y in zip(side, side[1:]) if x != y) if tag == "dense4" else 0
            assert tag != "dense4" or (True in side and False in side), (name, side)
        many_live_tracks(pkg, oracle, to_dev, streams=4, T=64, frames=frames, spacing=9.0, min_live=64)   # (test_64_live_tracks_vs_oracle[9.0-64]'s case: streams and seed as there)
    n_state = assert_logs_bit_identical(logs["default"], logs["dense4"], "default vs -DMOT_UPDATE_DENSE_TRACKS=4")
    assert n_state >= 4 * 64 * (frames - 2), n_state
    return dict(states_compared=n_state, calls=len(logs["default"]), threshold_crossings=crossings)
