"""Per-track accumulators (mot_set_track_accumulation / mot_accumulate_track_points, csrc/track_accum.hip): bodies shared by tests/test_emu_track_accum.py
(emulator) and tests/test_track_accum_gpu.py (MI355X). The callers supply a capacity_cases.Env.

The expectation is a Python model that shares no code with the kernels: after every fused call it reads, per slot, get_track_points(rest=False, frame="global")
and get_tracks — both exist without the feature — and folds them per track id into a list of {x, y, z, step} records, a list of observations, total, first_step
and last_step; the ring rule keeps the last K points and the last O observations. The model keeps every id for ever and knows nothing about track slots. All
comparisons are exact (bytes, float bits through view(np.uint32)); there is no tolerance anywhere."""
import ctypes as C

import numpy as np

import capacity_cases as CC
import track_link_cases as LC
import track_point_cases as PC


# ------------------------------------------------------------------------------------------------------------------ the model
class Model:
    def __init__(self, B, K, O):
        self.B, self.K, self.O = B, K, O
        self.tracks = [dict() for _ in range(B)]   # per slot: id -> entry
        self.step = [0] * B
        self.latest = [np.zeros(0, np.int32) for _ in range(B)]

    def restart(self, b):
        self.tracks[b] = {}; self.step[b] = 0; self.latest[b] = np.zeros(0, np.int32)

    def fold(self, env, c, b, refused=False):
        """one accepted accumulate call covered slot b: what the slot's fused step contributes"""
        step = self.step[b]; self.step[b] += 1
        self.latest[b] = np.zeros(0, np.int32)
        if refused:   # a frame refused for capacity has no owners; its step still counts
            return
        r = c.get_track_points(b, rest=False, frame="global")
        t = c.get_tracks(b)
        assert (r["track_id"] >= 0).all()
        self.latest[b] = r["track_id"]
        for k, tid in enumerate(r["track_id"]):
            tid = int(tid); f, n = int(r["first"][k]), int(r["count"][k])
            e = self.tracks[b].setdefault(tid, dict(xyz=[], step=[], obs=[], first_step=step, total=0))
            e["xyz"].append(r["xyz"][f:f + n]); e["step"].append(np.full(n, step, np.int32)); e["total"] += n; e["last_step"] = step
            o = np.zeros(1, env.mot.ACCUM_OBS_DTYPE)
            o["step"], o["count"], o["n_boxes"], o["track_manage"] = step, n, r["n_boxes"][k], t["track_manage"][tid]
            o["px"], o["py"], o["is_static"], o["lifetime"] = t["p"][tid][0], t["p"][tid][1], t["is_static"][tid], t["lifetime"][tid]
            o["v"], o["yaw"] = t["v_yaw"][tid][0], t["v_yaw"][tid][1]
            e["obs"].append(o)

    def kept(self, b, tid):
        e = self.tracks[b][tid]
        xyz = np.concatenate(e["xyz"]).reshape(-1, 3)[-self.K:]; step = np.concatenate(e["step"])[-self.K:]
        obs = np.concatenate(e["obs"])[-self.O:] if self.O else np.zeros(0, e["obs"][0].dtype)
        return np.ascontiguousarray(xyz, np.float32), step, obs


def peek(env, c, ptr, dtype, n):
    """n records at a device address of the zero-copy view (the emulator's "device" memory is host memory)"""
    out = np.zeros(n, dtype)
    if n == 0:
        return out
    c.synchronize()
    if env.lib_path is not None:
        C.memmove(out.ctypes.data, ptr, out.nbytes)
    else:
        import hiprt
        assert hiprt.hip().hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
    return out


def unroll(raw, total, cap):
    """the ring rule, restated: record t lies at t & (cap - 1); oldest first"""
    total = int(total)
    return raw[:total] if total <= cap else np.roll(raw, -(total & (cap - 1)), axis=0)


def same_points(xyz, step, want_xyz, want_step, what):
    assert len(xyz) == len(want_xyz), (what, "kept points", len(xyz), len(want_xyz))
    assert np.array_equal(np.ascontiguousarray(xyz, np.float32).view(np.uint32), want_xyz.view(np.uint32)), (what, "xyz bits")
    assert np.array_equal(step, want_step), (what, "step stamps")


def check(env, c, m, b, what):
    """slot b's rows, rings (raw through the device view, and through the getter) against the model -> the non-empty rows"""
    rows = c.get_accum_rows(b)
    v = c.track_accumulators_dev()
    T, K, O = v["tracks_per_slot"], v["points_per_track"], v["obs_per_track"]
    assert (T, K, O, v["max_batch"]) == (c.max_tracks_total, m.K, m.O, c.max_batch) and len(rows) == T and (v["d_obs"] == 0) == (O == 0), (what, v)
    used = np.nonzero(rows["track_id"] >= 0)[0]
    ids = rows["track_id"][used]
    assert len(set(ids.tolist())) == len(ids), (what, "two rows hold one id", ids)
    assert set(m.latest[b].tolist()) <= set(ids.tolist()), (what, "an id that owned a segment in the latest step has no row", m.latest[b], ids)
    empty = rows[rows["track_id"] < 0]
    assert not empty.tobytes().replace(b"\xff", b"\x00").strip(b"\x00"), (what, "an empty row is not {-1, 0, ...}")
    for r in used:
        row = rows[r]; tid = int(row["track_id"]); w = (what, "track", tid, "row", int(r))
        assert tid in m.tracks[b], (w, "the model never saw this id")
        e = m.tracks[b][tid]
        got = (int(row["first_step"]), int(row["last_step"]), int(row["obs_total"]), int(row["total"]), int(row["reserved"]))
        want = (e["first_step"], e["last_step"], len(e["obs"]) if O else 0, e["total"], 0)
        assert got == want, (w, "first_step, last_step, obs_total, total, reserved", got, want)
        wx, ws, wo = m.kept(b, tid)
        at = b * T + int(r)
        raw = peek(env, c, v["d_points"] + at * K * 16, env.mot.ACCUM_POINT_DTYPE, K)
        ring = unroll(raw, row["total"], K)
        same_points(ring["xyz"], ring["step"], wx, ws, (w, "device view"))
        g = c.get_track_accumulated(b, tid)
        assert g["row"].tobytes() == row.tobytes(), (w, "the getter's row")
        same_points(g["xyz"], g["step"], wx, ws, (w, "getter"))
        assert g["obs"].tobytes() == wo.tobytes(), (w, "getter: observations", g["obs"], wo)
        if O:
            rawo = peek(env, c, v["d_obs"] + at * O * 48, env.mot.ACCUM_OBS_DTYPE, O)
            assert unroll(rawo, row["obs_total"], O).tobytes() == wo.tobytes(), (w, "device view: observations")
    return rows[used]


def launch(env, c, clouds, stride, f, ego_v=None, yaw=None):
    B = len(clouds)
    host = np.zeros((B, stride, 4), np.float32)
    for b, x in enumerate(clouds):
        host[b, : len(x)] = x
    ptr, keep = env.upload(host)
    c.frames_dev(ptr, stride * 4, [len(x) for x in clouds], run_tracker=True, timestamps=[2.0e8 + f * 1e5] * B, ego_v=ego_v or [1.0] * B, ego_yaw=yaw or [0.0] * B)
    return keep


def step_and_check(env, c, m, clouds, stride, f, what, **kw):
    keep = launch(env, c, clouds, stride, f, **kw)
    B = len(clouds)
    for b in range(B):
        m.fold(env, c, b)
    c.accumulate_track_points(B)
    return [check(env, c, m, b, (what, "frame", f, "slot", b)) for b in range(B)]


# ------------------------------------------------------------------------------------------------------------------ 1: moving objects
def moving_objects(env, oracle, K, O):
    """the two-blob scene of track_link_cases.persistence, ten frames on three streams (own seeds; stream 2 drives and turns): K = 1024 never wraps, 256 wraps from
    the second frame, 64 is less than one frame brings (the skip rule); O = 4 wraps the log, O = 0 has none. At the end both blobs' rows have grown over at least
    five steps under one confirmed id, so the case cannot pass on empty rows."""
    frames_n, B = 10, 3
    def stream(seed):
        rng = np.random.default_rng(seed)
        def blob(cx, cy):
            q = np.zeros((200, 4), np.float32); q[:, 0] = cx + rng.uniform(-0.4, 0.4, 200); q[:, 1] = cy + rng.uniform(-0.4, 0.4, 200); q[:, 2] = rng.uniform(-1.0, 0.3, 200); return q
        return [np.concatenate([blob(8.0 + 0.3 * f, 5.0), blob(-9.0, -6.0 - 0.3 * f)]) for f in range(frames_n)]
    streams = [stream(3 + b) for b in range(B)]
    with env.context(0, max_points=2048, max_batch=B, max_tracks_total=256) as c:
        c.set_track_links(True); c.set_track_accumulation(K, O)
        m = Model(B, K, O)
        for f in range(frames_n):
            rows = step_and_check(env, c, m, [s[f] for s in streams], 2048, f, ("moving", K, O), ego_v=[0.0, 0.0, 1.0], yaw=[0.0, 0.0, 0.05 * f])
        for b in range(2):   # (the streams that stand still: persistence's own assertion; the driving stream is held to the model like the others)
            ids = c.get_point_tracks(b); elev = c.get_ground(b, n_hint=len(streams[b][-1]))["elevated"]
            east = elev[:, 0] > 0
            tm = c.get_tracks(b)["track_manage"]
            for side in (east, ~east):
                own = ids[side]; own = own[own >= 0]
                major = int(np.bincount(own).argmax())
                row = rows[b][rows[b]["track_id"] == major]
                assert len(row) == 1, (b, major, rows[b]["track_id"])
                row = row[0]
                assert row["last_step"] == frames_n - 1 and row["last_step"] - row["first_step"] >= 4 and row["total"] >= 5 * 100, (b, major, row)
                assert tm[major] == 5, (b, major, tm)
                if O:
                    assert row["obs_total"] >= 5 and c.get_track_accumulated(b, major)["obs"][-1]["track_manage"] == 5, (b, major, row)
                assert K >= 1024 or row["total"] > K, (b, major, row, "the ring did not meet the wrap this K is here for")
        if K == 64:
            assert max(int(x["count"][0]) for e in m.tracks[0].values() for x in e["obs"]) > K, "no frame brought more than K points of a track: the skip rule was not met"


# ------------------------------------------------------------------------------------------------------------------ 2: chunk and tile edges, many segments
def shapes(env, oracle, K, order_any=False):
    frames = PC.shape_frames(oracle)
    targets = [len(x) for x in frames[0]]
    B = len(targets)
    with env.context(0, max_points=8192, max_batch=B, max_tracks_total=512) as c:
        c.set_track_links(True); c.set_track_accumulation(K, 2)
        if order_any:
            c.set_point_order(env.mot.MOT_ORDER_ANY)
        m = Model(B, K, 2)
        for f in range(3):
            sent = [np.ascontiguousarray(x[np.random.default_rng(7 + b).permutation(len(x))]) for b, x in enumerate(frames[f])] if order_any else frames[f]
            rows = step_and_check(env, c, m, sent, 8192, f, ("shapes", K, order_any))
        assert [len(c.get_point_tracks(b)) for b in range(B)] == targets
        assert len(rows[B - 1]) >= 65 and (rows[B - 1]["total"] > 0).sum() >= 65, ("the longest frame has too few accumulated tracks", len(rows[B - 1]))
        assert len(rows[0]) == 0 and sum(len(r) for r in rows[3:]) > 0


# ------------------------------------------------------------------------------------------------------------------ 3: one track, two boxes
def one_track_two_boxes(env, oracle):
    frames, _ = PC.split_stream()
    seen = 0
    with env.context(0, max_points=2048, max_batch=1, max_tracks_total=256) as c:
        c.set_track_links(True); c.set_track_accumulation(256, 8)
        m = Model(1, 256, 8)
        for f, x in enumerate(frames):
            rows = step_and_check(env, c, m, [x], 2048, f, "split", ego_v=[0.0])[0]
            lab = c.get_clusters(0, n_elevated=max(len(c.get_point_tracks(0)), 1))["point_label"]
            r = c.get_track_points(0, rest=False)
            for k in np.nonzero(r["n_boxes"] >= 2)[0]:
                tid, n = int(r["track_id"][k]), int(r["count"][k])
                idx = r["index"][r["first"][k]: r["first"][k] + n]
                assert len(np.unique(lab[idx])) >= 2 and (np.diff(lab[idx]) != 0).sum() > 4, (f, "the two clusters' points are not interleaved in the segment")
                g = c.get_track_accumulated(0, tid)
                assert g["obs"][-1]["n_boxes"] >= 2 and g["obs"][-1]["count"] == n and (g["step"][-n:] == f).all(), (f, tid, g["obs"][-1])   # ONE row, in input order (check())
                seen += 1
    assert seen >= 1, "no track ever owned two boxes: the stream's geometry no longer splits a blob inside its track's gate"


# ------------------------------------------------------------------------------------------------------------------ 4: slot reuse
def reuse_stream(frames=12, per_group=3, hold=3):
    """blobs appear and vanish on a lattice: group g (per_group blobs, places of its own) is there in frames hold * g .. hold * g + hold - 1"""
    rng = np.random.default_rng(9)
    ctr = CC.cell_centres(CC.lattice_cells(250, 6, 3), 250, 50.0)
    def blob(k):
        q = np.zeros((48, 4), np.float32); q[:, 0] = ctr[k][0] + rng.uniform(-0.25, 0.25, 48); q[:, 1] = ctr[k][1] + rng.uniform(-0.25, 0.25, 48); q[:, 2] = rng.uniform(-1.0, 0.3, 48); return q
    return [np.concatenate([blob(40 * (per_group * (f // hold) + j)) for j in range(per_group)]) for f in range(frames)]


def slot_reuse(env, oracle, T_slots=8):
    frames = reuse_stream()
    reused = []
    with env.context(0, max_points=1024, max_batch=1, max_tracks_total=T_slots) as c:
        c.set_track_links(True); c.set_track_accumulation(64, 4)
        m = Model(1, 64, 4)
        before = c.get_accum_rows(0)
        for f, x in enumerate(frames):
            step_and_check(env, c, m, [x], 1024, f, "reuse", ego_v=[0.0])
            assert not c.get_tracks(0)["capacity_exceeded"], (f, "a birth was dropped: the script needs more track slots")
            rows = c.get_accum_rows(0)
            for r in np.nonzero((before["track_id"] >= 0) & (rows["track_id"] >= 0) & (before["track_id"] != rows["track_id"]))[0]:
                old, new = int(before["track_id"][r]), int(rows["track_id"][r])
                count = int(m.tracks[0][new]["obs"][0]["count"][0])
                assert rows["first_step"][r] == f and rows["last_step"][r] == f and rows["total"][r] == count and rows["obs_total"][r] == 1, (f, r, rows[r], count)
                LC.state_error(env, lambda: c.get_track_accumulated(0, old), "the evicted id")
                assert c.get_track_accumulated(0, new)["row"]["track_id"] == new
                reused.append((f, int(r), old, new))
            before = rows
    assert reused, "the script never reused a track slot: no row changed from one id to another"
    assert any(count > 0 for f, r, old, new in reused for count in [int(m.tracks[0][new]["obs"][0]["count"][0])]), reused


# ------------------------------------------------------------------------------------------------------------------ 5: contract
def code_of(env, fn):
    try:
        fn()
    except env.mot.MotError as e:
        return e.code
    return 0


def rows_bytes(c, B):
    return [c.get_accum_rows(b).tobytes() for b in range(B)]


def contract_modes(env, oracle):
    """off, the setter's arguments and states, links, sequence mode, a taken slot, the second call for a step, getters with buffers too small, off-then-on"""
    E = env.mot
    clouds = [[CC.small_scene(f, 20), CC.small_scene(f + 5, 12)] for f in range(8)]
    with env.context(0, max_points=4096, max_batch=2, max_tracks_total=64) as c:
        # links off: the setter refuses; feature off: the other four refuse
        assert code_of(env, lambda: c.set_track_accumulation(64, 4)) == E.MOT_E_STATE
        c.set_track_links(True)
        keep = launch(env, c, clouds[0], 4096, 0)
        row = np.zeros(1, E.ACCUM_ROW_DTYPE); n1, n2 = C.c_int(-7), C.c_int(-7)
        for what, fn in (("accumulate", lambda: c.accumulate_track_points(2)), ("view", c.track_accumulators_dev), ("rows", lambda: c.get_accum_rows(0)),
                         ("track", lambda: c.get_track_accumulated(0, 0))):
            assert code_of(env, fn) == E.MOT_E_STATE, what
        c.set_track_accumulation(0, 0)   # off while off
        for K, O in ((63, 0), (96, 0), (1 << 21, 0), (32, 0), (-64, 0), (64, 3), (64, 8192), (64, -1)):
            assert code_of(env, lambda: c.set_track_accumulation(K, O)) == E.MOT_E_ARG, (K, O)
        assert code_of(env, c.track_accumulators_dev) == E.MOT_E_STATE, "a refused setter turned the feature on"
        c.set_track_accumulation(64, 4)
        assert code_of(env, lambda: c.set_track_links(False)) == E.MOT_E_STATE, "links off while accumulation is on"
        assert all((c.get_accum_rows(b)["track_id"] == -1).all() for b in (0, 1))
        # the step the slots hold was taken before the feature was on
        assert code_of(env, lambda: c.accumulate_track_points(2)) == E.MOT_E_STATE
        m = Model(2, 64, 4)
        good = lambda f: step_and_check(env, c, m, clouds[f], 4096, f, "contract")
        def refused_unchanged(fn, code, what):
            before = rows_bytes(c, 2)
            assert code_of(env, fn) == code, what
            assert rows_bytes(c, 2) == before, (what, "a refused call changed rows")
        good(1)
        rows = good(2)
        assert len(rows[0]) > 0 and len(rows[1]) > 0
        refused_unchanged(lambda: c.accumulate_track_points(2), E.MOT_E_STATE, "a second accumulate for the same step")
        refused_unchanged(lambda: c.accumulate_track_points(1), E.MOT_E_STATE, "a second accumulate for the same step, slot 0 alone")
        refused_unchanged(lambda: c.accumulate_track_points(0), E.MOT_E_ARG, "batch 0")
        refused_unchanged(lambda: c.accumulate_track_points(3), E.MOT_E_ARG, "batch 3")
        # arguments of the getters; buffers too small
        assert c.lib.mot_get_accum_rows(c._h, 2, None, 0, C.byref(n1)) == E.MOT_E_ARG and c.lib.mot_get_accum_rows(c._h, 0, None, 0, None) == E.MOT_E_ARG
        small = np.full(63 * 8, -7, np.int32)
        assert c.lib.mot_get_accum_rows(c._h, 0, small.ctypes.data_as(C.c_void_p), 63, C.byref(n1)) == E.MOT_E_CAPACITY and n1.value == 64 and (small == -7).all()
        tid = int(rows[1]["track_id"][np.argmax(rows[1]["total"])])
        full = c.get_track_accumulated(1, tid); npts, nobs = len(full["xyz"]), len(full["obs"])
        assert npts > 1 and nobs > 1
        getter = lambda pts, cp, obs, co: c.lib.mot_get_track_accumulated(c._h, 1, tid, row.ctypes.data_as(C.c_void_p), pts.ctypes.data_as(C.c_void_p) if pts is not None else None, cp,
                                                                            C.byref(n1), obs.ctypes.data_as(C.c_void_p) if obs is not None else None, co, C.byref(n2))
        for cp, co in ((npts - 1, nobs), (npts, nobs - 1)):
            pts = np.full(64 * 4, -7, np.int32); obs = np.full(4 * 12, -7, np.int32); row[:] = 0; row["track_id"] = -7; n1.value = n2.value = -7
            assert getter(pts, cp, obs, co) == E.MOT_E_CAPACITY and (n1.value, n2.value) == (npts, nobs), (cp, co)
            assert (pts == -7).all() and (obs == -7).all() and row["track_id"][0] == -7, (cp, co, "a refused getter wrote")
        pts = np.full(64 * 4, -7, np.int32); obs = np.full(4 * 12, -7, np.int32)
        assert getter(pts, npts, obs, nobs) == 0 and (pts[npts * 4:] == -7).all() and (obs[nobs * 12:] == -7).all() and row["track_id"][0] == tid
        assert getter(None, 0, None, 0) == 0 and (n1.value, n2.value) == (npts, nobs), "null buffers: the counts alone"
        assert c.lib.mot_get_track_accumulated(c._h, 1, -1, None, None, 0, C.byref(n1), None, 0, C.byref(n2)) == E.MOT_E_ARG
        assert c.lib.mot_get_track_accumulated(c._h, 1, tid, None, None, 0, None, None, 0, C.byref(n2)) == E.MOT_E_ARG
        LC.state_error(env, lambda: c.get_track_accumulated(1, 60000), "an id no row holds")
        # a stage-wise call takes slot 0; a tracker step fed from outside takes slot 1's chain
        keep = launch(env, c, clouds[3], 4096, 3)
        elev = c.get_ground(0, n_hint=len(clouds[3][0]))["elevated"]
        c.cluster(elev)
        refused_unchanged(lambda: c.accumulate_track_points(2), E.MOT_E_STATE, "a batch that includes a taken slot")
        refused_unchanged(lambda: c.accumulate_track_points(1), E.MOT_E_STATE, "the taken slot alone")
        rows = good(4)   # step 2 of both slots: the refused calls counted nothing (check() holds last_step against the model's count)
        assert all((r["last_step"].max() == 2) for r in rows)
        # off then on: empty, steps from 0
        c.set_track_accumulation(0, 0)
        assert code_of(env, lambda: c.get_accum_rows(0)) == E.MOT_E_STATE
        c.set_track_links(False); c.set_track_links(True)   # (allowed again while the feature is off)
        c.set_track_accumulation(128, 0)
        assert all((c.get_accum_rows(b)["track_id"] == -1).all() for b in (0, 1))
        m = Model(2, 128, 0)
        rows = good(5)
        assert all(len(r) > 0 and (r["first_step"] == 0).all() and (r["last_step"] == 0).all() for r in rows)
    # sequence mode
    with env.context(0, max_points=4096, max_batch=2, max_tracks_total=64) as c:
        c.set_track_links(True); c.set_track_accumulation(64, 4)
        host = np.zeros((2, 4096, 4), np.float32)
        for f in range(2):
            host[f, : len(clouds[f][0])] = clouds[f][0]
        ptr, keep = env.upload(host)
        c.sequence_dev(ptr, 4096 * 4, [len(clouds[f][0]) for f in range(2)], [2.0e8, 2.001e8], [1.0] * 2, [0.0] * 2)
        c.get_track_points(1)   # (the export serves sequence mode)
        before = rows_bytes(c, 2)
        assert code_of(env, lambda: c.accumulate_track_points(2)) == E.MOT_E_STATE and code_of(env, lambda: c.accumulate_track_points(1)) == E.MOT_E_STATE
        assert rows_bytes(c, 2) == before


def contract_refused_frame(env, oracle):
    """a frame refused for capacity in slot 1 (track_point_cases.contract_refused): nothing is appended there, its step still advances, the neighbour appends"""
    p = oracle.params(0)
    max_points = 8192
    at, beyond = CC.fused_edges(oracle, p, "groups", max_points)
    with env.context(0, max_points=max_points, max_batch=2, max_tracks_total=2048) as c:
        c.set_track_links(True); c.set_track_accumulation(64, 2)
        m = Model(2, 64, 2)
        for f in range(2):
            keep = launch(env, c, [CC.small_scene(f, 20), beyond], max_points, f)
            CC.refused(env, lambda: c.get_track_points(1), CC.MSG_GROUPS, "track points of a refused frame")
            m.fold(env, c, 0); m.fold(env, c, 1, refused=True)
            c.accumulate_track_points(2)
            assert len(check(env, c, m, 0, ("refused: the neighbour", f))) > 0
            assert (c.get_accum_rows(1)["track_id"] == -1).all(), "a refused frame appended"
        keep = launch(env, c, [CC.small_scene(2, 20), CC.small_scene(7, 12)], max_points, 2)
        m.fold(env, c, 0); m.fold(env, c, 1)   # (the stream's capacity flag is sticky; get_tracks delivers the records all the same)
        c.accumulate_track_points(2)
        assert check(env, c, m, 0, "after the refused frames")["last_step"].max() == 2
        rows = check(env, c, m, 1, "the good frame after two refused ones")
        assert len(rows) > 0 and (rows["first_step"] == 2).all() and (rows["last_step"] == 2).all(), ("the refused frames' steps did not count", rows)


def contract_resets(env, oracle):
    """reset_slot, reset_tracks_slot, stream_load and reset empty the rows of the slots they touch and restart their steps; the other slots keep theirs"""
    E = env.mot
    B = 3
    clouds = [[CC.small_scene(f + 3 * b, 12) for b in range(B)] for f in range(12)]
    with env.context(0, max_points=4096, max_batch=B, max_tracks_total=64) as c:
        c.set_track_links(True); c.set_track_accumulation(128, 4)
        m = Model(B, 128, 4)
        f = 0
        def good():
            nonlocal f
            rows = step_and_check(env, c, m, clouds[f], 4096, f, "resets")
            f += 1
            return rows
        good(); good()
        blob = c.stream_save(2)
        for what, fn in (("reset_slot", lambda: c.reset_slot(1)), ("reset_tracks_slot", lambda: c.reset_tracks_slot(1)), ("stream_load", lambda: c.stream_load(1, blob))):
            keep = launch(env, c, clouds[f], 4096, f); f += 1   # a step that is not yet accumulated when the slot is reset
            others = [c.get_accum_rows(b).tobytes() for b in (0, 2)]
            fn()
            assert (c.get_accum_rows(1)["track_id"] == -1).all(), (what, "rows not emptied")
            assert [c.get_accum_rows(b).tobytes() for b in (0, 2)] == others, (what, "another slot's rows changed")
            assert code_of(env, lambda: c.accumulate_track_points(B)) == E.MOT_E_STATE, (what, "the step the reset slot holds belongs to ids that are gone")
            assert [c.get_accum_rows(b).tobytes() for b in (0, 2)] == others
            c.accumulate_track_points(1); m.fold(env, c, 0)   # (slot 0 alone is still whole — and now one step ahead of slot 2)
            m.restart(1)   # (stream_load: the loaded stream goes on with ITS ids; the model of slot 1 starts empty all the same, with whatever ids come)
            rows = good()
            assert len(rows[1]) > 0 and (rows[1]["first_step"] == 0).all() and (rows[1]["last_step"] == 0).all(), (what, rows[1])
            assert rows[0]["last_step"].max() == m.step[0] - 1 > rows[2]["last_step"].max() == m.step[2] - 1 > 0, what
        good()
        c.reset()
        assert all((c.get_accum_rows(b)["track_id"] == -1).all() for b in range(B))
        assert code_of(env, lambda: c.accumulate_track_points(B)) == E.MOT_E_STATE
        for b in range(B):
            m.restart(b)
        rows = good()
        assert all(len(r) > 0 and (r["last_step"] == 0).all() for r in rows)


# ------------------------------------------------------------------------------------------------------------------ 6: non-interference
KERNELS = (b"track_accum_plan_kernel", b"track_accum_scatter_kernel")


def defined_items(readout):
    """track_point_cases.readout with the snapshot's per-ever-track arrays cut down to what a snapshot DEFINES: positions and the slot map of every track, the
    tombstone (24 bytes: lifetime, static flag, frozen speed and yaw) of the EVICTED ones only — the tracker writes a tombstone when it evicts a track (track.hip,
    "eviction"); until then the entry is whatever the context's memory held, and two contexts differ there whatever they were asked to do"""
    out = []
    for name, x in readout:
        if name != "snapshot: per-ever-track arrays":
            out.append((name, x)); continue
        nt = len(x) // 44
        assert len(x) == nt * 44
        slot_of = np.frombuffer(x[16 * nt: 20 * nt], np.int32)
        tomb = np.frombuffer(x[20 * nt:], np.uint8).reshape(nt, 24)
        out += [(name + " (positions, slot map)", x[: 20 * nt]), (name + " (tombstones of the evicted)", tomb[slot_of < 0].tobytes())]
    return out


def non_interference(env, oracle, order_any=False, graphs=False):
    """everything a caller could read before the feature existed — ground, clusters, boxes, tracks, box and point links, snapshots (track_point_cases.readout) and the
    track-points export in both frames — is byte-identical in a context that accumulates after every call and one that never turns accumulation on"""
    clouds = [[CC.small_scene(f, 20), CC.small_scene(f + 5, 12)] for f in range(4)]
    if order_any:
        clouds = [[np.ascontiguousarray(x[np.random.default_rng(11 + b).permutation(len(x))]) for b, x in enumerate(fr)] for fr in clouds]
    res = {}
    for tag in ("never", "accumulates"):
        with env.context(0, max_points=4096, max_batch=2, max_tracks_total=256) as c:
            c.set_launch_graphs(graphs); c.set_track_links(True)
            if order_any:
                c.set_point_order(env.mot.MOT_ORDER_ANY)
            if tag == "accumulates":
                c.set_track_accumulation(256, 4)
            out = []
            for f in range(4):
                keep = PC.launch(env, c, clouds[f], 4096, f, yaw=0.02 * f)
                n_points = [len(x) for x in clouds[f]]
                before = PC.readout(c, 2, n_points)
                if tag == "accumulates":
                    c.accumulate_track_points(2)
                    PC.equal_readouts(PC.readout(c, 2, n_points), before, (f, "after the accumulate"))   # (one context: every byte, the undefined ones included)
                    assert (c.get_accum_rows(1)["track_id"] >= 0).any() or f == 0
                exports = [(fr + str(rest) + k, np.ascontiguousarray(v).tobytes()) for fr in ("sensor", "global") for rest in (False, True) for b in (0, 1)
                           for k, v in sorted(c.get_track_points(b, rest=rest, frame=fr).items())]
                out.append(defined_items(before) + exports)
            res[tag] = out
    for f in range(4):
        PC.equal_readouts(res["accumulates"][f], res["never"][f], (f, "against a context that never accumulated"))


def launches_only_in_the_accumulate(env, oracle):
    """emulator: the launch counters of the two new kernels move in mot_accumulate_track_points and nowhere else; off, nothing is allocated"""
    lib = env.mot.load_library(env.lib_path)
    lib.hipemu_live_allocs.restype = C.c_long
    count = lambda: [lib.hipemu_launch_count(k) for k in KERNELS]
    with env.context(0, max_points=4096, max_batch=2, max_tracks_total=64) as c:
        before = count()
        c.set_track_links(True)
        keep = PC.launch(env, c, [CC.small_scene(0, 20), CC.small_scene(5, 12)], 4096, 0)
        c.get_track_points(1, frame="global")
        allocs = lib.hipemu_live_allocs()
        for fn in (lambda: c.accumulate_track_points(2), c.track_accumulators_dev, lambda: c.get_accum_rows(0), lambda: c.set_track_accumulation(63, 0)):
            assert code_of(env, fn) != 0
        c.set_track_accumulation(0, 0)
        assert lib.hipemu_live_allocs() == allocs, "the feature allocated while it was off"
        c.set_track_accumulation(64, 4)
        assert lib.hipemu_live_allocs() == allocs + 4
        for f in range(1, 4):
            keep = PC.launch(env, c, [CC.small_scene(f, 20), CC.small_scene(f + 5, 12)], 4096, f)
            for b in (0, 1):
                c.get_point_tracks(b); c.get_box_tracks(b); c.get_boxes(b); c.get_tracks(b); c.get_track_points(b, frame="global"); c.get_accum_rows(b)
            assert count() == before, f
        c.accumulate_track_points(2)
        assert count() == [n + 1 for n in before]
        c.get_accum_rows(0); c.track_accumulators_dev(); c.get_track_accumulated(1, int(c.get_accum_rows(1)["track_id"].max()))
        c.reset_slot(0); c.reset(); c.get_track_points(1)
        assert code_of(env, lambda: c.accumulate_track_points(2)) == env.mot.MOT_E_STATE
        assert count() == [n + 1 for n in before]
        c.set_track_accumulation(0, 0)
        assert lib.hipemu_live_allocs() == allocs, "turning the feature off did not free its memory"


def setter_under_allocation_failure(env, oracle):
    """emulator: each of the setter's allocations failing in turn -> MOT_E_HIP, the mode stays as it was (off, or the earlier geometry with its rows), nothing is leaked"""
    lib = env.mot.load_library(env.lib_path)
    lib.hipemu_live_allocs.restype = C.c_long
    lib.hipemu_fail_alloc_at.argtypes = [C.c_long]; lib.hipemu_fail_alloc_at.restype = None
    E = env.mot
    try:
        with env.context(0, max_points=4096, max_batch=2, max_tracks_total=64) as c:
            c.set_track_links(True)
            allocs = lib.hipemu_live_allocs()
            for k in (1, 2, 3, 4):
                lib.hipemu_fail_alloc_at(k)
                assert code_of(env, lambda: c.set_track_accumulation(64, 4)) == E.MOT_E_HIP, k
                lib.hipemu_fail_alloc_at(0)
                assert b"hipMalloc(&d_accum_" in c.lib.mot_last_error(c._h), c.lib.mot_last_error(c._h)
                assert lib.hipemu_live_allocs() == allocs and code_of(env, c.track_accumulators_dev) == E.MOT_E_STATE, k
            c.set_track_accumulation(64, 4)
            m = Model(2, 64, 4)
            rows = step_and_check(env, c, m, [CC.small_scene(0, 20), CC.small_scene(5, 12)], 4096, 0, "before the failed change of geometry")
            allocs = lib.hipemu_live_allocs()
            for k in (1, 2, 3):   # (O = 0: three allocations)
                lib.hipemu_fail_alloc_at(k)
                assert code_of(env, lambda: c.set_track_accumulation(128, 0)) == E.MOT_E_HIP, k
                lib.hipemu_fail_alloc_at(0)
                assert lib.hipemu_live_allocs() == allocs and c.track_accumulators_dev()["points_per_track"] == 64, k
                check(env, c, m, 1, ("the earlier geometry is whole", k))
            step_and_check(env, c, m, [CC.small_scene(1, 20), CC.small_scene(6, 12)], 4096, 1, "after the failed change of geometry")
    finally:
        lib.hipemu_fail_alloc_at(0)
