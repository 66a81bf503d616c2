"""A recorded drive into the per-track accumulators (mot_sequence_accumulate_dev, csrc/track_accum_seq.hip): bodies shared by tests/test_emu_track_accum_seq.py
(emulator) and tests/test_track_accum_seq_gpu.py (MI355X). The callers supply a capacity_cases.Env.

The reference in every case is a SECOND context with max_batch = 1 and otherwise the same parameters, driven frame by frame with frames_dev(batch 1) +
accumulate_track_points(1): the path tests/track_accum_cases.py holds against its Python model, never the code under test. Compared as bytes, slot 0 of both:
the rows, for every row with an id the getter's row / points / steps / observations and the device view's rings unrolled by the ring rule, and the track models
under all four flag combinations. Raw ring bytes outside a row's kept range are undefined in both and are not compared. There is no tolerance anywhere."""
import ctypes as C

import numpy as np

import capacity_cases as CC
import track_accum_cases as AC
import track_link_cases as LC
import track_point_cases as PC

SEQ_KERNELS = (b"track_accum_capture_kernel", b"track_accum_seq_segments_kernel", b"track_accum_seq_plan_kernel", b"track_accum_seq_finish_kernel",
               b"track_accum_seq_scatter_kernel")


def stamp(f):
    return 2.0e8 + f * 1e5   # (track_accum_cases.launch's clock)


# ------------------------------------------------------------------------------------------------------------------ the two drivers
def ref_step(env, c, cloud, stride, f, ego_v=1.0, yaw=0.0):
    """the existing path: one frame through frames_dev(batch 1), then appended"""
    keep = AC.launch(env, c, [cloud], stride, f, ego_v=[ego_v], yaw=[yaw])
    c.accumulate_track_points(1)
    c.synchronize()


def seq_call(env, c, clouds, stride, f0, ego_v, yaw, accumulate=True, tracks=(0, 0, 0)):
    """frames f0 .. f0 + len(clouds) - 1 of one stream in one call; ego_v / yaw: one value per frame -> the input block"""
    host = np.zeros((len(clouds), stride, 4), np.float32)
    for k, x in enumerate(clouds):
        host[k, : len(x)] = x
    ptr, keep = env.upload(host)
    fn = c.sequence_accumulate_dev if accumulate else c.sequence_dev
    fn(ptr, stride * 4, [len(x) for x in clouds], [stamp(f0 + k) for k in range(len(clouds))], list(ego_v), list(yaw), *tracks)
    c.synchronize()
    return keep   # (get_ground re-runs the compaction from the batch's input: a caller that reads the slots out holds on to it)


def snapshot(env, c):
    """everything of slot 0's accumulators that is defined, as (name, bytes) items"""
    E = env.mot
    rows = c.get_accum_rows(0)
    v = c.track_accumulators_dev()
    T, K, O = v["tracks_per_slot"], v["points_per_track"], v["obs_per_track"]
    items = [("rows", rows.tobytes())]
    for r in np.nonzero(rows["track_id"] >= 0)[0]:
        tid = int(rows["track_id"][r]); w = "track %d row %d: " % (tid, r)
        g = c.get_track_accumulated(0, tid)
        items += [(w + "getter row", g["row"].tobytes()), (w + "getter xyz", np.ascontiguousarray(g["xyz"], np.float32).tobytes()),
                  (w + "getter step", np.ascontiguousarray(g["step"]).tobytes()), (w + "getter obs", g["obs"].tobytes())]
        raw = AC.peek(env, c, v["d_points"] + int(r) * K * 16, E.ACCUM_POINT_DTYPE, K)
        items.append((w + "device view: ring", np.ascontiguousarray(AC.unroll(raw, rows["total"][r], K)).tobytes()))
        if O:
            rawo = AC.peek(env, c, v["d_obs"] + int(r) * O * 48, E.ACCUM_OBS_DTYPE, O)
            items.append((w + "device view: log", np.ascontiguousarray(AC.unroll(rawo, rows["obs_total"][r], O)).tobytes()))
    if O:
        for axes in (False, True):
            for current in (False, True):
                m = c.get_track_models(0, axes=axes, current=current)
                items += [("models axes=%d current=%d: %s" % (axes, current, k), np.ascontiguousarray(x).tobytes()) for k, x in sorted(m.items())]
    return items


def same_snapshots(got, want, what):
    assert [n for n, _ in got] == [n for n, _ in want], (what, "other rows hold ids", [n for n, _ in got][:8], [n for n, _ in want][:8])
    for (n, x), (_, y) in zip(got, want):
        assert x == y, (what, n)


def other_slots_empty(c, what):
    for b in range(1, c.max_batch):
        rows = c.get_accum_rows(b)
        assert (rows["track_id"] == -1).all() and not rows.tobytes().replace(b"\xff", b"\x00").strip(b"\x00"), (what, "a row of slot", b, "was touched")


def contexts(env, frames, K, O, max_points, T, order_any=False):
    """(the sequence context, the frame-by-frame reference): the same parameters, max_batch = frames against 1"""
    out = []
    for B in (frames, 1):
        c = env.context(0, max_points=max_points, max_batch=B, max_tracks_total=T)
        c.set_track_links(True); c.set_track_accumulation(K, O)
        if order_any:
            c.set_point_order(env.mot.MOT_ORDER_ANY)
        out.append(c)
    return out


def one_call_against_reference(env, clouds, K, O, max_points, T, ego_v, yaw, what, order_any=False):
    """all frames in ONE sequence call against the reference -> (the reference's rows after every frame, its context's final snapshot rows)"""
    F = len(clouds)
    seq, ref = contexts(env, F, K, O, max_points, T, order_any)
    with seq, ref:
        history = []
        for f, x in enumerate(clouds):
            ref_step(env, ref, x, max_points, f, ego_v[f], yaw[f])
            history.append(ref.get_accum_rows(0))
        seq_call(env, seq, clouds, max_points, 0, ego_v, yaw)
        same_snapshots(snapshot(env, seq), snapshot(env, ref), what)
        other_slots_empty(seq, what)
        LC.state_error(env, lambda: seq.accumulate_track_points(1), (what, "the sequence slots cannot be appended again"))
        obs = {int(r["track_id"]): ref.get_track_accumulated(0, int(r["track_id"]))["obs"] for r in history[-1] if r["track_id"] >= 0}
    return history, obs


# ------------------------------------------------------------------------------------------------------------------ 1: moving objects in one call
def moving_stream(seed=5, frames_n=10):
    """stream 2 of track_accum_cases.moving_objects (its generator, its seed): two 200-point blobs that move; the vehicle drives and turns"""
    rng = np.random.default_rng(seed)
    def blob(cx, cy):
        q = np.zeros((200, 4), np.float32); q[:, 0] = cx + rng.uniform(-0.4, 0.4, 200); q[:, 1] = cy + rng.uniform(-0.4, 0.4, 200); q[:, 2] = rng.uniform(-1.0, 0.3, 200); return q
    clouds = [np.concatenate([blob(8.0 + 0.3 * f, 5.0), blob(-9.0, -6.0 - 0.3 * f)]) for f in range(frames_n)]
    return clouds, [1.0] * frames_n, [0.05 * f for f in range(frames_n)]


def moving_objects(env, oracle, K, O):
    """K = 1024 never meets itself, 256 wraps ACROSS frames inside the call (the hazard one frame at a time does not have), 64 is less than one frame brings and
    wraps too; O = 4 wraps the log inside the call"""
    clouds, ego_v, yaw = moving_stream()
    history, obs = one_call_against_reference(env, clouds, K, O, 2048, 256, ego_v, yaw, ("moving", K, O))
    rows = history[-1]
    assert (rows["track_id"] >= 0).any()
    if K <= 256:
        assert (rows["total"] > K).any(), ("no ring met the wrap this K is here for", rows[rows["track_id"] >= 0])
    if O:
        assert (rows["obs_total"] > O).any(), ("no log wrapped", rows[rows["track_id"] >= 0])


# ------------------------------------------------------------------------------------------------------------------ 2: slot reuse inside the call
def slot_reuse(env, oracle):
    clouds = AC.reuse_stream()
    history, obs = one_call_against_reference(env, clouds, 64, 4, 1024, 8, [0.0] * len(clouds), [0.0] * len(clouds), "reuse")
    first, last = history[0], history[-1]
    changed = np.nonzero((first["track_id"] >= 0) & (last["track_id"] >= 0) & (first["track_id"] != last["track_id"]))[0]
    assert len(changed) >= 1, ("no row went from one id to another inside the call", first["track_id"], last["track_id"])
    assert (last["total"][changed] > 0).any(), ("the new ids brought no points", last[changed])


# ------------------------------------------------------------------------------------------------------------------ 3: chained calls
def chained_calls(env, oracle, K=256, O=4):
    """frames 0-2 frame by frame, 3-7 one sequence call, 8-9 a second one, then frame 9's cloud once more frame by frame with a later stamp = eleven steps"""
    clouds, ego_v, yaw = moving_stream()
    clouds, ego_v, yaw = clouds + [clouds[9]], ego_v + [1.0], yaw + [0.5]
    seq, ref = contexts(env, 5, K, O, 2048, 256)
    with seq, ref:
        for f, x in enumerate(clouds):
            ref_step(env, ref, x, 2048, f, ego_v[f], yaw[f])
        for f in range(3):
            ref_step(env, seq, clouds[f], 2048, f, ego_v[f], yaw[f])
        seq_call(env, seq, clouds[3:8], 2048, 3, ego_v[3:8], yaw[3:8])
        seq_call(env, seq, clouds[8:10], 2048, 8, ego_v[8:10], yaw[8:10])
        ref_step(env, seq, clouds[10], 2048, 10, ego_v[10], yaw[10])
        same_snapshots(snapshot(env, seq), snapshot(env, ref), "chained")
        other_slots_empty(seq, "chained")
        rows = ref.get_accum_rows(0)
        assert rows["last_step"].max() == 10 and (rows["total"] > K).any() and (rows["obs_total"] > O).any(), rows[rows["track_id"] >= 0]


# ------------------------------------------------------------------------------------------------------------------ 4: chunk and tile edges, many segments
def shapes(env, oracle, K, order_any=False):
    """the longest stream of track_point_cases.shape_frames (7 719 points, 160 blobs: eight 1024-point chunks, the last one partial) as a 3-frame sequence"""
    clouds = [fr[-1] for fr in PC.shape_frames(oracle)]
    if order_any:
        clouds = [np.ascontiguousarray(x[np.random.default_rng(7 + f).permutation(len(x))]) for f, x in enumerate(clouds)]
    history, obs = one_call_against_reference(env, clouds, K, 2, 8192, 512, [1.0] * 3, [0.0] * 3, ("shapes", K, order_any), order_any=order_any)
    rows = history[-1]
    assert ((rows["track_id"] >= 0) & (rows["total"] > 0)).sum() >= 65, ("too few accumulated tracks", ((rows["track_id"] >= 0) & (rows["total"] > 0)).sum())


# ------------------------------------------------------------------------------------------------------------------ 5: one track, two boxes
def one_track_two_boxes(env, oracle):
    clouds, _ = PC.split_stream()
    history, obs = one_call_against_reference(env, clouds, 256, 8, 2048, 256, [0.0] * len(clouds), [0.0] * len(clouds), "split")
    assert any((o["n_boxes"] >= 2).any() for o in obs.values()), "no logged observation of a track that owned two boxes"


# ------------------------------------------------------------------------------------------------------------------ 6: contract
def sequence_readout(env, c, n_points):
    F = len(n_points)
    exports = [(fr + str(rest) + str(b) + k, np.ascontiguousarray(v).tobytes()) for fr in ("sensor", "global") for rest in (False, True) for b in range(F)
               for k, v in sorted(c.get_track_points(b, rest=rest, frame=fr).items())]
    return AC.defined_items(PC.readout(c, F, n_points)) + exports


class TrackBlocks:
    """d_tracks / d_counts of a sequence call: caller-owned device blocks, filled with the sentinel -7"""

    def __init__(self, env, F, per_frame):
        self.per_frame = per_frame
        self.h_tr = np.full(F * per_frame * env.mot.TRACK_DTYPE.itemsize // 4, -7, np.int32); self.h_cnt = np.full(F, -7, np.int32)
        (self.p_tr, self.k_tr), (self.p_cnt, self.k_cnt) = env.upload(self.h_tr), env.upload(self.h_cnt)

    def args(self):
        return (self.p_tr, self.per_frame, self.p_cnt)

    def read(self):
        return [("d_tracks", LC.download(self.k_tr, self.h_tr).tobytes()), ("d_counts", LC.download(self.k_cnt, self.h_cnt).tobytes())]


def contract_state_and_arguments(env, oracle):
    """off / links off: MOT_E_STATE and the tracker has not stepped; frames > max_batch; the accumulate afterwards; reset_slot"""
    E = env.mot
    clouds = [CC.small_scene(f, 20) for f in range(5)]
    n_points = [len(x) for x in clouds[:3]]
    zeros = [0.0] * 3
    res = {}
    for tag in ("refused first", "fresh"):
        with env.context(0, max_points=4096, max_batch=3, max_tracks_total=64) as c:
            if tag == "refused first":
                assert AC.code_of(env, lambda: seq_call(env, c, clouds[:3], 4096, 0, [1.0] * 3, zeros)) == E.MOT_E_STATE, "links off"
                c.set_track_links(True)
                assert AC.code_of(env, lambda: seq_call(env, c, clouds[:3], 4096, 0, [1.0] * 3, zeros)) == E.MOT_E_STATE, "accumulation off"
                assert b"mot_sequence_accumulate_dev" in c.lib.mot_last_error(c._h)
            c.set_track_links(True)
            keep = seq_call(env, c, clouds[:3], 4096, 0, [1.0] * 3, zeros, accumulate=False)
            res[tag] = sequence_readout(env, c, n_points)
    PC.equal_readouts(res["refused first"], res["fresh"], "sequence_dev after two refused calls against a fresh context: the tracker had not stepped")
    seq, ref = contexts(env, 3, 64, 4, 4096, 64)
    with seq, ref:
        assert AC.code_of(env, lambda: seq_call(env, seq, clouds[:4], 4096, 0, [1.0] * 4, [0.0] * 4)) == E.MOT_E_ARG, "frames > max_batch"
        assert AC.code_of(env, lambda: seq.sequence_accumulate_dev(0, 4096 * 4, n_points, [stamp(0)] * 3, zeros, zeros)) == E.MOT_E_ARG, "null cloud"
        assert (seq.get_accum_rows(0)["track_id"] == -1).all()
        for f in range(3):
            ref_step(env, ref, clouds[f], 4096, f)
        seq_call(env, seq, clouds[:3], 4096, 0, [1.0] * 3, zeros)
        same_snapshots(snapshot(env, seq), snapshot(env, ref), "after the refused calls")
        before = AC.rows_bytes(seq, 3)
        assert (seq.get_accum_rows(0)["track_id"] >= 0).any()
        for batch in (1, 3):
            assert AC.code_of(env, lambda: seq.accumulate_track_points(batch)) == E.MOT_E_STATE, batch
        assert AC.rows_bytes(seq, 3) == before, "a refused accumulate changed rows"
        # reset_slot(0): rows empty, the counter restarted (both contexts: the next frames are first frames again)
        seq.reset_slot(0); ref.reset_slot(0)
        assert (seq.get_accum_rows(0)["track_id"] == -1).all()
        for f in (3, 4):
            ref_step(env, ref, clouds[f], 4096, f)
        seq_call(env, seq, clouds[3:5], 4096, 3, [1.0] * 2, [0.0] * 2)
        same_snapshots(snapshot(env, seq), snapshot(env, ref), "after reset_slot")
        rows = seq.get_accum_rows(0); used = rows[rows["track_id"] >= 0]
        assert len(used) > 0 and used["first_step"].min() == 0 and used["last_step"].max() == 1, used


def contract_refused_frame(env, oracle):
    """track_accum_cases.contract_refused_frame's frame in the MIDDLE of a sequence: it appends nothing and counts its step"""
    max_points = 8192
    at, beyond = CC.fused_edges(oracle, oracle.params(0), "groups", max_points)
    clouds = [CC.small_scene(0, 20), beyond, CC.small_scene(2, 20)]
    seq, ref = contexts(env, 3, 64, 2, max_points, 2048)
    with seq, ref:
        for f, x in enumerate(clouds):
            ref_step(env, ref, x, max_points, f)
        keep = seq_call(env, seq, clouds, max_points, 0, [1.0] * 3, [0.0] * 3)
        CC.refused(env, lambda: seq.get_track_points(1), CC.MSG_GROUPS, "track points of the refused frame")
        same_snapshots(snapshot(env, seq), snapshot(env, ref), "a refused frame in mid-sequence")
        rows = seq.get_accum_rows(0); used = rows[rows["track_id"] >= 0]
        assert len(used) > 0 and used["last_step"].max() == 2 and not ((used["first_step"] == 1) | (used["last_step"] == 1)).any(), used
        m = seq.get_track_models(0, current=True)["models"]
        assert (m["track_id"] >= 0).any() and (m["last_step"][m["track_id"] >= 0] == 2).all(), "MOT_MODEL_CURRENT is the step of the last frame"


# ------------------------------------------------------------------------------------------------------------------ 7: non-interference
def non_interference(env, oracle, order_any=False):
    """everything readable after the new call — every slot's track_point_cases.readout, the track-points exports in both frames, d_tracks / d_counts — is what
    sequence_dev leaves in a context that never turned accumulation on; two calls in a row, so the second one starts from the state the first one left"""
    clouds = [CC.small_scene(f, 20) for f in range(4)]
    if order_any:
        clouds = [np.ascontiguousarray(x[np.random.default_rng(11 + f).permutation(len(x))]) for f, x in enumerate(clouds)]
    res = {}
    for tag in ("never", "accumulates"):
        with env.context(0, max_points=4096, max_batch=2, max_tracks_total=256) as c:
            c.set_track_links(True)
            if order_any:
                c.set_point_order(env.mot.MOT_ORDER_ANY)
            if tag == "accumulates":
                c.set_track_accumulation(256, 4)
            out = []
            for f0 in (0, 2):
                blk = TrackBlocks(env, 2, 64)
                keep = seq_call(env, c, clouds[f0:f0 + 2], 4096, f0, [1.0] * 2, [0.02 * f0, 0.02 * (f0 + 1)], accumulate=tag == "accumulates", tracks=blk.args())
                out.append(sequence_readout(env, c, [len(x) for x in clouds[f0:f0 + 2]]) + blk.read())
            if tag == "accumulates":
                assert (c.get_accum_rows(0)["total"] > 0).any()
            res[tag] = out
    for k in range(2):
        PC.equal_readouts(res["accumulates"][k], res["never"][k], (k, "against sequence_dev in a context that never accumulated"))
    cnt = np.frombuffer(res["never"][1][-1][1], np.int32)
    assert (cnt > 0).all(), ("no live tracks were exported", cnt)


# ------------------------------------------------------------------------------------------------------------------ 8: emulator only
def launches_and_allocations(env, oracle):
    """the new kernels' launch counters move in the new call and nowhere else (one capture per step, the others once per call); the existing accumulate kernels keep
    theirs; the call's two allocations fail one by one; turning accumulation off gives everything back"""
    lib = env.mot.load_library(env.lib_path)
    lib.hipemu_live_allocs.restype = C.c_long
    lib.hipemu_fail_alloc_at.argtypes = [C.c_long]; lib.hipemu_fail_alloc_at.restype = None
    E = env.mot
    count = lambda names: [lib.hipemu_launch_count(k) for k in names]
    clouds = [CC.small_scene(f, 20) for f in range(6)]
    try:
        seq, ref = contexts(env, 3, 64, 4, 4096, 64)
        with ref:   # (closed before anything is counted: every allocation below is the sequence context's)
            for f in range(3):
                ref_step(env, ref, clouds[f], 4096, f)
            want = snapshot(env, ref)
        with seq:
            seq.set_track_accumulation(0, 0)
            mine, old = count(SEQ_KERNELS), count(AC.KERNELS)
            # the scratch the per-track point clouds keep until mot_destroy, first: what is counted below is the accumulators' and the new call's own
            seq_call(env, seq, clouds[:3], 4096, 0, [1.0] * 3, [0.0] * 3, accumulate=False)
            seq.get_track_points(1, frame="global")
            seq.reset_slot(0)
            base = lib.hipemu_live_allocs()
            seq.set_track_accumulation(64, 4)
            assert lib.hipemu_live_allocs() == base + 4
            for k in (1, 2):
                lib.hipemu_fail_alloc_at(k)
                assert AC.code_of(env, lambda: seq_call(env, seq, clouds[:3], 4096, 0, [1.0] * 3, [0.0] * 3)) == E.MOT_E_HIP, k
                lib.hipemu_fail_alloc_at(0)
                assert b"hipMalloc(&c->d_tas_" in seq.lib.mot_last_error(seq._h), seq.lib.mot_last_error(seq._h)
                assert lib.hipemu_live_allocs() == base + 4, (k, "a failed call kept memory")
                assert count(SEQ_KERNELS) == mine, (k, "a refused call launched")
            seq_call(env, seq, clouds[:3], 4096, 0, [1.0] * 3, [0.0] * 3)   # the next call succeeds, from the state the refused ones did not touch
            assert lib.hipemu_live_allocs() == base + 4 + 2
            assert count(SEQ_KERNELS) == [mine[0] + 3] + [n + 1 for n in mine[1:]] and count(AC.KERNELS) == old
            same_snapshots(snapshot(env, seq), want, "after two calls refused for memory")
            mine = count(SEQ_KERNELS)
            # sequence_dev with accumulation on, the getters, the resets: none of the new kernels
            seq_call(env, seq, clouds[3:6], 4096, 3, [1.0] * 3, [0.0] * 3, accumulate=False)
            assert AC.code_of(env, lambda: seq.accumulate_track_points(1)) == E.MOT_E_STATE
            for b in range(3):
                seq.get_point_tracks(b); seq.get_box_tracks(b); seq.get_track_points(b, frame="global"); seq.get_accum_rows(b)
            seq.get_track_models(0); seq.reset_slot(0); seq.reset()
            assert count(SEQ_KERNELS) == mine and count(AC.KERNELS) == old
            assert lib.hipemu_live_allocs() >= base + 4 + 2   # (and the track models' own blocks: they go with the accumulators too)
            seq.set_track_accumulation(0, 0)
            assert lib.hipemu_live_allocs() == base, "turning accumulation off did not free the call's scratch"
            # on again: the scratch comes back with the first call; a frame-by-frame step launches the existing kernels and none of the new ones
            seq.set_track_accumulation(128, 0)
            seq_call(env, seq, clouds[:3], 4096, 0, [1.0] * 3, [0.0] * 3)
            assert lib.hipemu_live_allocs() == base + 3 + 2 and (seq.get_accum_rows(0)["total"] > 0).any()
            mine = count(SEQ_KERNELS)
            ref_step(env, seq, clouds[3], 4096, 3)
            assert count(SEQ_KERNELS) == mine and count(AC.KERNELS) == [n + 1 for n in old]
    finally:
        lib.hipemu_fail_alloc_at(0)
