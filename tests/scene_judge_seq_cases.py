"""A recorded drive's points judged against the grid the drive left (mot_export_sequence_scene_points_dev / mot_get_sequence_scene_points, csrc/scene_judge_seq.hip):
bodies shared by tests/test_emu_scene_judge_seq.py (emulator) and tests/test_scene_judge_seq_gpu.py (MI355X). The callers supply a capacity_cases.Env.

The expectation shares no code with the kernels. A SECOND context with max_batch = 1 and otherwise the same parameters is driven frame by frame with frames_dev(batch 1) +
accumulate_scene(1) (scene_grid_seq_cases.contexts). Per frame it gives the points, the owners and the kinds of that step — get_track_points(rest=True) in both frames
and get_tracks()["is_static"]: the glob / sensor / ids / moving parts of scene_judge_cases.observe —, after the last frame get_scene_grid(0) and whether the last
window could be placed. A numpy lookup of every frame's cells in that FINAL grid, scene_judge_cases.classify, and a class-major packing written here follow. Class
bytes, both tables and the records are compared AS BYTES, with sentinel margins round every block, through the export and through the getter. No tolerance anywhere."""
import ctypes as C

import numpy as np

import capacity_cases as CC
import scene_grid_cases as SG
import scene_grid_seq_cases as SGQ
import scene_judge_cases as SJ
import track_accum_cases as AC
import track_link_cases as LC
import track_point_cases as PC

UNKNOWN, MOVING, TRAIL, NEW, KNOWN = range(5)
ALL, MASKS, LIMIT, CLS_SENT = SJ.ALL, SJ.MASKS, SJ.LIMIT, SJ.CLS_SENT
KERNELS = (b"scene_judge_seq_classify_kernel", b"scene_judge_seq_scan_kernel", b"scene_judge_seq_bases_kernel", b"scene_judge_seq_scatter_kernel")


# ------------------------------------------------------------------------------------------------------------------ the model
def to_global(m, sensor):
    """mot_track_place.h's expression in np.float32, left to right (checked against the getter's bits on every frame that has one)"""
    m = np.asarray(m, np.float32); x, y, z = sensor[:, 0], sensor[:, 1], sensor[:, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)], axis=1).astype(np.float32)


def ref_frame(env, ref, cloud, stride, f, ego_v, yaw, inv, accumulate=False, oracle=None):
    """one frame through the frame-by-frame reference -> the parts of the verdicts that belong to this step (read BEFORE the next step moves them)"""
    keep = AC.launch(env, ref, [cloud], stride, f, ego_v=[ego_v], yaw=[yaw])
    ok = SJ.placeable(ref, 0, inv)
    ref.accumulate_scene(1)
    if accumulate:
        ref.accumulate_track_points(1)
    m = ref.sensor_pose(0)[1]
    try:
        o = SJ.observe(ref, 0, ok)
        part = {k: o[k] for k in ("n", "glob", "sensor", "ids", "owned", "flagged", "moving")}
        assert part["glob"].tobytes() == to_global(m, part["sensor"]).tobytes(), "the model's transform is not the getter's"
        part["refused"] = False
    except env.mot.MotError as e:   # the box stage refused the frame for capacity: its elevated points, none of them owned
        assert e.code == env.mot.MOT_E_CAPACITY and oracle is not None, e   # (every getter of the slot refuses: the elevated cloud is the oracle's ground stage's)
        sensor = np.ascontiguousarray(oracle.ground_remove(oracle.params(0), cloud)["elevated"][:, :3], np.float32); n = len(sensor)
        part = dict(n=n, glob=to_global(m, sensor), sensor=sensor, ids=np.full(n, -1, np.int64), owned=np.zeros(n, bool), flagged=np.zeros(n, bool), moving=np.zeros(n, bool), refused=True)
    part["placed"] = ok
    return part


def against_grid(o, g, ok):
    """the cells of one frame's points in the FINAL grid: take / in_window / s / d, as scene_judge_cases.observe computes them against the grid of its own step"""
    h = g["header"]
    W = int(h["size"]); inv = np.float32(1.0) / np.float32(h["cell"])
    ok = bool(ok) and int(h["step"]) >= 0
    glob = o["glob"]; n = o["n"]
    with np.errstate(over="ignore", invalid="ignore"):
        tx, ty = glob[:, 0] * inv, glob[:, 1] * inv
        take = np.isfinite(glob).all(axis=1) & (np.abs(tx) < LIMIT) & (np.abs(ty) < LIMIT) & ok
        gi = np.where(take, np.floor(tx), 0).astype(np.int64); gj = np.where(take, np.floor(ty), 0).astype(np.int64)
    u, v = gi - int(h["origin_i"]), gj - int(h["origin_j"])
    in_window = (u >= 0) & (u < W) & (v >= 0) & (v < W)
    take = take & in_window
    s = np.zeros(n, np.uint64); d = np.zeros(n, np.uint64)
    s[take] = g["cells"]["static_hits"][v[take], u[take]]; d[take] = g["cells"]["dynamic_hits"][v[take], u[take]]
    return dict(o, take=take, in_window=in_window, s=s, d=d, u=u, v=v, ok=ok)


def pack(obs, cls, mask, frame):
    """class-major over the drive -> segments [F, 5, 2], totals [5, 2], records [m, 4], all int32"""
    F = len(obs)
    seg = np.zeros((F, 5, 2), np.int32); tot = np.zeros((5, 2), np.int32); recs = []; run = 0
    for c in range(5):
        picked = bool((mask >> c) & 1); start = run; count = 0
        for k in range(F):
            at = np.nonzero(cls[k] == c)[0]
            seg[k, c] = (run if picked else -1, len(at)); count += len(at)
            if picked:
                xyz = (obs[k]["glob"] if frame == "global" else obs[k]["sensor"]).view(np.int32)
                r = np.zeros((len(at), 4), np.int32); r[:, :3] = xyz[at]; r[:, 3] = at
                recs.append(r); run += len(at)
        tot[c] = (start if picked else -1, count)
    return seg, tot, (np.concatenate(recs) if recs else np.zeros((0, 4), np.int32))


class Expect:
    """a reference context driven frame by frame; after each piece (a sequence call's frames) the pieces' frames against the grid as it then stands"""

    def __init__(self, env, ref, cell, stride, accumulate=False, oracle=None):
        self.env, self.ref, self.stride, self.inv, self.accumulate, self.oracle = env, ref, stride, np.float32(1.0) / np.float32(cell), accumulate, oracle
        self.f = 0; self.placed = False

    def piece(self, clouds, ego_v, yaw):
        parts = []
        for k, x in enumerate(clouds):
            parts.append(ref_frame(self.env, self.ref, x, self.stride, self.f, ego_v[k], yaw[k], self.inv, self.accumulate, self.oracle)); self.f += 1
        self.placed = parts[-1]["placed"]
        g = self.ref.get_scene_grid(0)
        return [against_grid(o, g, self.placed) for o in parts]

    def one_step(self, cloud, ego_v=1.0, yaw=0.0):
        return self.piece([cloud], [ego_v], [yaw])


class Blocks:
    """sentinel-filled device blocks for mot_export_sequence_scene_points_dev: ONE block of `capacity` records, [F][5] segments, [5] totals, [F][class_stride] class bytes,
    a margin on both sides of each; misalign: records, segments and totals start 4 bytes off a 16-byte (8-byte) boundary"""

    def __init__(self, env, F, capacity, class_stride, misalign=False):
        self.F, self.cap, self.cs, self.off = F, capacity, class_stride, (1 if misalign else 0)
        self.h_pts = np.full(4 + 1 + capacity * 4 + 4, -7, np.int32); self.h_seg = np.full(2 + 1 + F * 10 + 2, -7, np.int32); self.h_tot = np.full(2 + 1 + 10 + 2, -7, np.int32)
        self.h_cls = np.full(16 + F * class_stride + 16, CLS_SENT, np.uint8)
        (self.p_pts, self.k_pts), (self.p_seg, self.k_seg), (self.p_tot, self.k_tot), (self.p_cls, self.k_cls) = (env.upload(h) for h in (self.h_pts, self.h_seg, self.h_tot, self.h_cls))
        assert self.p_pts % 16 == 0
        self.a_pts, self.a_seg, self.a_tot, self.a_cls = self.p_pts + 16 + 4 * self.off, self.p_seg + 8 + 4 * self.off, self.p_tot + 8 + 4 * self.off, self.p_cls + 16

    def run(self, c, frames, mask, frame, params=(1, 1, 2), points=True, classes=True):
        c.export_sequence_scene_points_dev(frames, self.a_pts if points else 0, self.cap if points else 0, self.a_seg, self.a_tot, self.a_cls if classes else 0, self.cs,
                                           min_static_hits=params[0], trail=params[1:], classes=mask, frame=frame)
        c.synchronize()
        return self.read(frames)

    def raw(self):
        return tuple(LC.download(k, h).copy() for k, h in ((self.k_pts, self.h_pts), (self.k_seg, self.h_seg), (self.k_tot, self.h_tot), (self.k_cls, self.h_cls)))

    def read(self, frames):
        pts, seg, tot, cls = self.raw()
        o = self.off
        assert (pts[: 4 + o] == -7).all() and (pts[4 + o + self.cap * 4:] == -7).all(), "records outside the drive's block"
        assert (seg[: 2 + o] == -7).all() and (seg[2 + o + frames * 10:] == -7).all(), "segments outside the frames' rows"
        assert (tot[: 2 + o] == -7).all() and (tot[2 + o + 10:] == -7).all(), "totals outside their block"
        assert (cls[:16] == CLS_SENT).all() and (cls[16 + frames * self.cs:] == CLS_SENT).all(), "class bytes outside the frames' rows"
        return (pts[4 + o: 4 + o + self.cap * 4].reshape(self.cap, 4), seg[2 + o: 2 + o + frames * 10].reshape(frames, 5, 2), tot[2 + o: 2 + o + 10].reshape(5, 2),
                cls[16: 16 + frames * self.cs].reshape(frames, self.cs))

    def free(self):
        for k in (self.k_pts, self.k_seg, self.k_tot, self.k_cls):
            if hasattr(k, "free"):
                k.free()


def check_export(blk, out, obs, cls, mask, frame, what, points=True, classes=True):
    """an export's blocks against the model: both tables, the records below the capacity, the class bytes below the stride, the sentinel behind them"""
    p, s, t, k = out
    F = len(s)
    seg, tot, rec = pack(obs[:F], cls[:F], mask, frame)
    assert s.tobytes() == seg.tobytes(), (what, "segments", np.argwhere(s != seg)[:4])
    assert t.tobytes() == tot.tobytes(), (what, "totals", t.tolist(), tot.tolist())
    w = min(len(rec), blk.cap) if points else 0
    if p[:w].tobytes() != rec[:w].tobytes():
        bad = np.argwhere(p[:w] != rec[:w])
        raise AssertionError((what, "records", len(bad), "words differ; first", bad[0], p[bad[0][0]], rec[bad[0][0]]))
    assert (p[w:] == -7).all(), (what, "written beyond the drive's records")
    for f in range(F):
        wc = min(obs[f]["n"], blk.cs) if classes else 0
        assert k[f, :wc].tobytes() == cls[f][:wc].tobytes(), (what, "frame", f, "class bytes", np.argwhere(k[f, :wc] != cls[f][:wc])[:4])
        assert (k[f, wc:] == CLS_SENT).all(), (what, "frame", f, "class bytes beyond the frame's points")


def check_getter(c, obs, cls, mask, frame, params, what, frames=None):
    F = frames or len(obs)
    r = c.get_sequence_scene_points(F, min_static_hits=params[0], trail=params[1:], classes=mask, frame=frame)
    seg, tot, rec = pack(obs[:F], cls[:F], mask, frame)
    got = np.zeros((len(r["index"]), 4), np.int32); got[:, :3] = np.ascontiguousarray(r["xyz"], np.float32).view(np.int32).reshape(-1, 3); got[:, 3] = r["index"]
    assert r["segments"].tobytes() == seg.tobytes() and r["totals"].tobytes() == tot.tobytes() and got.tobytes() == rec.tobytes(), (what, "getter")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(r["classes"], cls[:F])), (what, "getter, class bytes")
    for f in range(F):
        for first, n in seg[f]:
            if first >= 0:
                assert (np.diff(r["index"][first: first + n]) > 0).all(), (what, "index not ascending inside a frame's part")


def judge_and_check(env, c, obs, params_list, what, masks=(ALL,), frames_of=("global",), facts=None, getter=True):
    need = sum(o["n"] for o in obs)
    stride = max(max(o["n"] for o in obs), 1) + 3
    for params in params_list:
        cls = [SJ.classify(o, *params) for o in obs]
        for mask in masks:
            for frame in frames_of:
                blk = Blocks(env, len(obs), need + 3, stride)
                check_export(blk, blk.run(c, len(obs), mask, frame, params), obs, cls, mask, frame, (what, params, mask, frame))
                blk.free()
        if getter:
            check_getter(c, obs, cls, masks[-1], frames_of[-1], params, (what, params))
        if facts is not None:
            for o, k in zip(obs, cls):
                SJ.tally(facts, o, k)
    return [SJ.classify(o, *params_list[0]) for o in obs]


def contexts(env, F, cell, W, max_points, T, order_any=False, accum=None):
    return SGQ.contexts(env, F, cell, W, max_points, T, order_any, accum)


def call_and_expect(env, seq, ex, clouds, stride, ego_v, yaw, f0=0, accumulate=False):
    obs = ex.piece(clouds, ego_v, yaw)
    keep = SGQ.seq_call(env, seq, clouds, stride, f0, ego_v, yaw, accumulate=accumulate)
    return obs, keep


# ------------------------------------------------------------------------------------------------------------------ 1, 2: a drive; its last frame against the existing path
def a_drive(env, oracle, cell, W=64):
    """scene_grid_seq_cases.drive (16 frames, two blobs that stand in the world, one that moves, the vehicle drives and turns): several parameter sets, every mask, both
    frames. From the model alone: all five classes, a flagged-static point in a trail cell, an id that is dynamic in one frame and static in another, early points
    outside the final window. Then frame F - 1 against export_scene_points_dev(1) of the frame-by-frame context behind its last accumulate_scene"""
    clouds, ego_v, yaw = SGQ.drive(env)
    F = len(clouds)
    seq, ref = contexts(env, F, cell, W, 2048, 256)
    facts = {}
    with seq, ref:
        ex = Expect(env, ref, cell, 2048)
        obs, keep = call_and_expect(env, seq, ex, clouds, 2048, ego_v, yaw)
        judge_and_check(env, seq, obs, SJ.PARAMS, ("drive", cell), masks=MASKS, frames_of=("sensor", "global"), facts=facts)
        for k in ("unknown", "moving", "trail", "new", "known", "parked_trail", "unknown_outside"):
            assert facts.get(k, 0) > 0, (k, facts)
        kinds = {}   # id -> the kinds it had over the frames of the call: what the per-frame bit rows exist for
        for o in obs:
            for tid in np.unique(o["ids"][o["owned"]]):
                kinds.setdefault(int(tid), set()).add(bool(o["flagged"][o["ids"] == tid][0]))
        assert any(len(v) == 2 for v in kinds.values()), ("no id is dynamic in one frame of the call and static in another", kinds)
        early = sum(int((~o["in_window"] & np.isfinite(o["glob"]).all(axis=1)).sum()) for o in obs[: F // 2])
        assert early > 0 and obs[-1]["in_window"].any(), "no point of an early frame lies outside the final window"
        # 2: the last frame is judged against the same grid by both routes
        params = SJ.PARAMS[0]
        cls = [SJ.classify(o, *params) for o in obs]
        n = obs[-1]["n"]
        old = SJ.Blocks(env, 1, n + 3, n + 3)
        po, so, ko = old.run(ref, 1, ALL, "global", params)
        blk = Blocks(env, F, sum(o["n"] for o in obs) + 3, n + 3)
        p, s, t, k = blk.run(seq, F, ALL, "global", params)
        assert ko[0, :n].tobytes() == k[F - 1, :n].tobytes() == cls[-1].tobytes(), "the last frame's class bytes"
        assert so[0, :, 1].tobytes() == s[F - 1, :, 1].tobytes(), "the last frame's counts"
        for c in range(5):
            a, m = int(s[F - 1, c, 0]), int(s[F - 1, c, 1])
            assert po[0, so[0, c, 0]: so[0, c, 0] + m].tobytes() == p[a: a + m].tobytes(), ("the last frame's records of class", c)
        old.free(); blk.free()
    return facts


# ------------------------------------------------------------------------------------------------------------------ 3: chunk, tile and wave edges
def shapes(env, oracle, order_any=False):
    """successive frames of ONE call with 0, 1, 63, 64, 65, 2047, 2048, 2049, 5000 elevated points and a full frame (track_point_cases.shape_frames; max_points 8192): every
    mask in both frames; the capacity one below the need and at it; blocks 4 bytes off; counts alone; no class block; a class_stride below a frame's count; fewer frames"""
    frames = PC.shape_frames(oracle)
    clouds = list(frames[0])
    targets = [len(x) for x in clouds]
    assert {0, 1, 63, 64, 65, 2047, 2048, 2049, 5000} <= set(targets)
    if order_any:
        clouds = [np.ascontiguousarray(x[np.random.default_rng(7 + f).permutation(len(x))]) for f, x in enumerate(clouds)]
    F = len(clouds)
    params = (2, 1, 3)
    facts = {}
    seq, ref = contexts(env, F, 1.0, 64, 8192, 512, order_any)
    with seq, ref:
        ex = Expect(env, ref, 1.0, 8192)
        obs, keep = call_and_expect(env, seq, ex, clouds, 8192, [1.0] * F, [0.0] * F)
        assert [o["n"] for o in obs] == targets
        cls = [SJ.classify(o, *params) for o in obs]
        for o, k in zip(obs, cls):
            SJ.tally(facts, o, k)
        total, widest = sum(targets), max(targets)
        for mask in MASKS:
            for frame in ("global", "sensor"):
                blk = Blocks(env, F, total + 3, widest + 3)
                check_export(blk, blk.run(seq, F, mask, frame, params), obs, cls, mask, frame, ("shapes", order_any, mask, frame))
                blk.free()
        for mask, frame in ((ALL, "global"), (0b10100, "sensor"), (0, "global")):
            check_getter(seq, obs, cls, mask, frame, params, ("shapes", order_any, mask, frame))
        for mask in (ALL, 0b10100):
            need = int(sum((k == c).sum() for k in cls for c in range(5) if (mask >> c) & 1))
            for cap, cs, mis in ((need - 1, widest, False), (need, widest, True), (need, 5000 - 1, True), (1, 1, False)):
                blk = Blocks(env, F, cap, cs, misalign=mis)
                check_export(blk, blk.run(seq, F, mask, "global", params), obs, cls, mask, "global", ("shapes, capacity", order_any, mask, cap, cs, mis))
                blk.free()
        blk = Blocks(env, F, 0, widest)
        check_export(blk, blk.run(seq, F, 0, "global", params, points=False), obs, cls, 0, "global", ("shapes, counts and classes alone", order_any), points=False)
        blk.free()
        blk = Blocks(env, F, 0, 0)
        check_export(blk, blk.run(seq, F, 0, "sensor", params, points=False, classes=False), obs, cls, 0, "sensor", ("shapes, counts alone", order_any), points=False, classes=False)
        blk.free()
        blk = Blocks(env, F, total, widest)
        check_export(blk, blk.run(seq, F, ALL, "sensor", params, classes=False), obs, cls, ALL, "sensor", ("shapes, no class block", order_any), classes=False)
        blk.free()
        for fewer in (F - 1, 7, 1):   # `frames` below the call's: the first frames alone, still against the final grid
            blk = Blocks(env, F, total, widest)
            check_export(blk, blk.run(seq, fewer, ALL, "global", params), obs[:fewer], cls[:fewer], ALL, "global", ("shapes, fewer frames", order_any, fewer))
            blk.free()
            check_getter(seq, obs, cls, 0b10100, "global", params, ("shapes, fewer frames", fewer), frames=fewer)
    for k in ("unknown", "moving", "new", "known"):
        assert facts.get(k, 0) > 0, (k, facts)
    return facts


# ------------------------------------------------------------------------------------------------------------------ 4: frame counts
def frame_counts(env, oracle, F):
    """F frames of small scenes (max_points 1024): 256 / 257 cross the round of the scan over frames. With 5 frames or more the middle one has no elevated point"""
    clouds = [CC.small_scene(f % 7, 3) for f in range(F)]
    if F >= 5:
        clouds[F // 2] = clouds[F // 2][:0]
    seq, ref = contexts(env, F, 1.0, 64, 1024, 64)
    with seq, ref:
        ex = Expect(env, ref, 1.0, 1024)
        obs, keep = call_and_expect(env, seq, ex, clouds, 1024, [1.0] * F, [0.0] * F)
        assert all(o["n"] > 0 for k, o in enumerate(obs) if not (F >= 5 and k == F // 2)) and (F < 5 or obs[F // 2]["n"] == 0)
        cls = judge_and_check(env, seq, obs, ((1, 1, 2),), ("frame counts", F), masks=(0b10100, ALL), frames_of=("global",))
        assert sum(int((k == KNOWN).sum()) for k in cls) > 0 and len({int(c) for k in cls for c in np.unique(k)}) >= 2


def refused_frame(env, oracle):
    """scene_grid_seq_cases.refused_frame's drive: the box stage refuses the middle frame for capacity — its elevated points are judged, none of them owned"""
    max_points = 8192
    at, beyond = CC.fused_edges(oracle, oracle.params(0), "groups", max_points)
    clouds = [CC.small_scene(0, 20), beyond, CC.small_scene(2, 20)]
    seq, ref = contexts(env, 3, 1.0, 64, max_points, 2048)
    with seq, ref:
        ex = Expect(env, ref, 1.0, max_points, oracle=oracle)
        obs, keep = call_and_expect(env, seq, ex, clouds, max_points, [1.0] * 3, [0.0] * 3)
        assert obs[1]["refused"] and obs[1]["n"] > 0 and not obs[0]["refused"] and not obs[2]["refused"]
        cls = judge_and_check(env, seq, obs, ((1, 1, 2),), "a refused frame", masks=(ALL,), frames_of=("global", "sensor"))
        assert not (cls[1] == MOVING).any() and (cls[1] == KNOWN).any()


# ------------------------------------------------------------------------------------------------------------------ 5: windows
def windows(env, oracle, kind, cell=0.25, W=64):
    """scene_grid_seq_cases.scroll's per-frame speeds and headings. jump: a shift of at least W in the middle — the frames before it are UNKNOWN unless MOVING;
    invalid_middle: a window that cannot be placed in mid-drive; invalid_last: the LAST window cannot be placed — nothing takes part"""
    spec = {"jump": [(0.0, 0.0), (0.0, 0.0), (0.0, 0.0), (200.0, 0.0)] + [(0.0, 0.0)] * 14,
            "invalid_middle": [(0.0, 0.0), (2.5, 0.0), (2.5, 0.0), (3.0e9, 0.0), (3.0e9, np.pi), (0.0, 0.0), (2.5, 0.0), (0.0, 0.0)],
            "invalid_last": [(0.0, 0.0), (2.5, 0.0), (2.5, 0.0), (0.0, 0.0), (0.0, 0.0), (3.0e9, 0.0)]}[kind]
    F = len(spec)
    rng = np.random.default_rng(17)
    clouds = [np.concatenate([SG.world_blob(rng, cx, cy) for cx, cy in ((5.0, 3.0), (-4.0, 5.0), (2.0, -6.0), (-5.0, -4.0))]) for f in range(F)]
    ego_v, yaw = [s[0] for s in spec], [s[1] for s in spec]
    seq, ref = contexts(env, F, cell, W, 1024, 64)
    with seq, ref:
        ex = Expect(env, ref, cell, 1024)
        obs, keep = call_and_expect(env, seq, ex, clouds, 1024, ego_v, yaw)
        cls = judge_and_check(env, seq, obs, SJ.PARAMS[:2], ("windows", kind), masks=(ALL, 0b10000), frames_of=("global",))
        placed = [o["placed"] for o in obs]
        if kind == "jump":
            assert all(placed) and all(np.isin(cls[f], (UNKNOWN, MOVING)).all() and obs[f]["n"] > 0 for f in range(3)), "something of the frames before the jump takes part"
            assert any(obs[f]["take"].any() and not np.isin(cls[f], (UNKNOWN, MOVING)).all() for f in range(4, F)), "nothing behind the jump takes part"
        elif kind == "invalid_middle":
            assert not placed[3] and placed[-1] and obs[3]["n"] > 0 and any(o["take"].any() for o in obs[:3]) and any(o["take"].any() for o in obs[5:])
        else:
            assert not placed[-1] and placed[0] and all(np.isin(k, (UNKNOWN, MOVING)).all() for k in cls) and sum(int((k == UNKNOWN).sum()) for k in cls) > 0


def chained(env, oracle, cell=0.5, W=64):
    """a prior grid from frame-by-frame steps and an earlier call, then a second call that continues it: each call's frames against the grid so far"""
    clouds, ego_v, yaw = SGQ.drive(env, 14, 10.0, 0.04)
    seq, ref = contexts(env, 5, cell, W, 2048, 256)
    with seq, ref:
        ex = Expect(env, ref, cell, 2048)
        for f in range(3):
            ex.one_step(clouds[f], ego_v[f], yaw[f])
            SGQ.ref_step(env, seq, clouds[f], 2048, f, ego_v[f], yaw[f])
        assert AC.code_of(env, lambda: seq.get_sequence_scene_points(1)) == env.mot.MOT_E_STATE, "frame-by-frame slots"
        obs, keep = call_and_expect(env, seq, ex, clouds[3:8], 2048, ego_v[3:8], yaw[3:8], f0=3)
        first = judge_and_check(env, seq, obs, SJ.PARAMS[:2], "chained, first call")
        obs2, keep2 = call_and_expect(env, seq, ex, clouds[8:10], 2048, ego_v[8:10], yaw[8:10], f0=8)
        judge_and_check(env, seq, obs2, SJ.PARAMS[:2], "chained, second call")
        assert AC.code_of(env, lambda: seq.get_sequence_scene_points(3)) == env.mot.MOT_E_ARG, "frames beyond the latest call's"
        assert int(SGQ.header(ref)["step"][0]) == 9 and any(o["take"].any() for o in obs) and any(o["take"].any() for o in obs2)
        g = ref.get_scene_grid(0)["cells"]
        assert ((g["last_seen"] > 0) & (g["last_seen"] <= 8)).any(), "nothing from before the second call is left in the grid it is judged against"


def helper_pieces(env, oracle, cell=0.27, W=64):
    """sequence.play_static_map cuts the 16-frame drive into calls of max_batch = 5 frames: every piece against the grid so far, as its docstring says"""
    import importlib
    seq_mod = importlib.import_module(env.mot.__name__ + ".sequence")
    clouds, ego_v, yaw = SGQ.drive(env)
    seq, ref = contexts(env, 5, cell, W, 2048, 256)
    with seq, ref:
        ex = Expect(env, ref, cell, 2048)
        got = seq_mod.play_static_map(seq, list(zip(clouds, ego_v, yaw)), dt_us=1e5, t0=2.0e8, classes=(KNOWN, TRAIL), upload=env.upload)
        assert [r["first_frame"] for r in got] == [0, 5, 10, 15]
        known = 0
        for r in got:
            k0 = r["first_frame"]
            obs = ex.piece(clouds[k0: k0 + 5], ego_v[k0: k0 + 5], yaw[k0: k0 + 5])
            cls = [SJ.classify(o, 1, 1, 2) for o in obs]
            seg, tot, rec = pack(obs, cls, 0b10100, "global")
            have = np.zeros((len(r["index"]), 4), np.int32); have[:, :3] = np.ascontiguousarray(r["xyz"], np.float32).view(np.int32).reshape(-1, 3); have[:, 3] = r["index"]
            assert r["segments"].tobytes() == seg.tobytes() and r["totals"].tobytes() == tot.tobytes() and have.tobytes() == rec.tobytes(), ("piece", k0)
            known += int(tot[KNOWN, 1])
        assert known > 0


# ------------------------------------------------------------------------------------------------------------------ 6: contract
def raw_export(c, E, blk, frames=3, params=(1, 1, 2), mask=ALL, frame=0, points="a", cap=None, segments="a", totals="a", classes="a", cstride=None):
    P = E.MotSceneJudgeParams(*params) if params is not None else None
    ptr = lambda v, a: None if v is None else (a if v == "a" else v)
    return c.lib.mot_export_sequence_scene_points_dev(c._h, frames, C.byref(P) if P is not None else None, mask, frame, C.c_void_p(ptr(points, blk.a_pts)),
                                                      C.c_long(blk.cap if cap is None else cap), C.c_void_p(ptr(segments, blk.a_seg)), C.c_void_p(ptr(totals, blk.a_tot)),
                                                      C.c_void_p(ptr(classes, blk.a_cls)), C.c_long(blk.cs if cstride is None else cstride))


def contract(env, oracle):
    """every refusal with the caller's blocks unchanged; the states that answer MOT_E_STATE; served behind MOT_SEQ_SCENE | MOT_SEQ_ACCUMULATE; the getter's MOT_E_CAPACITY
    delivers the counts"""
    E = env.mot
    W, F, stride = 64, 3, 4096
    clouds = [CC.small_scene(f, 20) for f in range(8)]
    ones, zeros = [1.0] * F, [0.0] * F
    seq, ref = contexts(env, F, 1.0, W, stride, 64, accum=(64, 4))
    with seq, ref:
        c = seq
        blk = Blocks(env, F, F * stride, stride)
        export = lambda frames=F: c.export_sequence_scene_points_dev(frames, blk.a_pts, blk.cap, blk.a_seg, blk.a_tot, blk.a_cls, blk.cs)
        getter = lambda frames=F: c.get_sequence_scene_points(frames)
        def untouched(what, before):
            c.synchronize()
            assert all((a == b).all() for a, b in zip(blk.raw(), before)), (what, "a refused call wrote into the caller's blocks")
        def state_error(what, frames=F):
            before = blk.raw()
            assert AC.code_of(env, lambda: export(frames)) == E.MOT_E_STATE and AC.code_of(env, lambda: getter(frames)) == E.MOT_E_STATE, what
            untouched(what, before)
        state_error("no sequence call yet")
        keep = AC.launch(env, c, clouds[:F], stride, 0)
        state_error("a fused batch")
        f0 = F
        def drive(scene=True, accumulate=False):
            nonlocal f0
            keep = SGQ.seq_call(env, c, clouds[:F], stride, f0, ones, zeros, scene=scene, accumulate=accumulate); f0 += F
            return keep
        keep = drive(scene=False)
        state_error("a sequence call without MOT_SEQ_SCENE")
        keep = drive(); export(); getter()
        keep = drive(scene=False)
        state_error("a later sequence call without MOT_SEQ_SCENE")
        keep = drive()
        before = blk.raw()
        for what, kw in (("null params", dict(params=None)), ("null segments", dict(segments=None)), ("null totals", dict(totals=None)), ("min_static_hits 0", dict(params=(0, 1, 2))),
                         ("min_static_hits 2^31 + 1", dict(params=(2 ** 31 + 1, 1, 2))), ("den 0", dict(params=(1, 0, 0))), ("den 65536", dict(params=(1, 1, 65536))),
                         ("num > den", dict(params=(1, 3, 2))), ("mask bit 5", dict(mask=32)), ("negative mask", dict(mask=-1)), ("frame 2", dict(frame=2)), ("frame -1", dict(frame=-1)),
                         ("frames 0", dict(frames=0)), ("frames beyond the call's", dict(frames=F + 1)), ("negative capacity", dict(cap=-1)), ("negative class stride", dict(cstride=-1)),
                         ("null points with a capacity", dict(points=None, mask=0)), ("null points with a mask", dict(points=None, cap=0)),
                         ("points off 4 bytes", dict(points=blk.a_pts + 2)), ("segments off 4 bytes", dict(segments=blk.a_seg + 2)), ("totals off 4 bytes", dict(totals=blk.a_tot + 2))):
            assert raw_export(c, E, blk, **kw) == E.MOT_E_ARG, what
            untouched(what, before)
        assert raw_export(c, E, blk, params=(2 ** 31, 65535, 65535)) == 0 and raw_export(c, E, blk, params=(1, 0, 1)) == 0, "the limits themselves are served"
        # the per-frame call keeps refusing the sequence slots
        old = SJ.Blocks(env, F, stride, stride)
        assert AC.code_of(env, lambda: c.export_scene_points_dev(F, old.a_pts, old.ps, old.a_seg, old.a_cls, old.cs)) == E.MOT_E_STATE and AC.code_of(env, lambda: c.get_scene_points(0)) == E.MOT_E_STATE
        export(F - 1); getter(1)   # fewer frames are served, again and again
        # the states that end it, each after a fresh drive
        c.ego_update(3.0e8, 0.0, 0.0, 1); c.track_step(LC.lattice(3), 3.0e8, slot=1)
        state_error("a tracker step fed from outside")
        keep = drive(); export()
        elev = c.get_ground(0, n_hint=len(clouds[0]))["elevated"]
        getter()   # (a getter that re-runs the compaction takes nothing)
        c.cluster(elev)
        state_error("a stage-wise call took slot 0")
        keep = drive(); export()
        c.reset_slot(0)
        state_error("mot_reset_slot")
        keep = drive(); export()
        blob = c.stream_save(0); c.stream_load(0, blob)
        state_error("mot_stream_load")
        keep = drive(); export()
        c.reset()
        state_error("mot_reset")
        keep = drive(); export()
        c.set_scene_grid(0.5, 128)
        state_error("mot_set_scene_grid: another geometry")
        keep = drive(); export()
        keep = AC.launch(env, c, clouds[:F], stride, f0); f0 += 1
        state_error("a fused call")
        keep = drive(); export()
        c.set_scene_grid(None)
        state_error("the grid off")
        blk.free(); old.free()
    # served behind MOT_SEQ_SCENE | MOT_SEQ_ACCUMULATE, against the model; the getter's MOT_E_CAPACITY
    seq, ref = contexts(env, F, 1.0, W, stride, 64, accum=(64, 4))
    with seq, ref:
        ex = Expect(env, ref, 1.0, stride, accumulate=True)
        obs, keep = call_and_expect(env, seq, ex, clouds[:F], stride, ones, zeros, accumulate=True)
        cls = judge_and_check(env, seq, obs, ((1, 1, 2),), "behind both products")
        seg, tot, rec = pack(obs, cls, ALL, "global")
        total, widest = len(rec), max(o["n"] for o in obs)
        assert total > 1
        n = C.c_long(-7); hs = np.full(F * 10, -7, np.int32); ht = np.full(10, -7, np.int32); P = E.MotSceneJudgeParams(1, 1, 2)
        pts = np.full((total + 1) * 4, -7, np.int32); kb = np.full(F * widest + 1, CLS_SENT, np.uint8)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        raw_get = lambda frames=F, P=P, mask=ALL, frame=0, pts=None, pcap=0, n=n, seg=hs, tot=ht, cls=None, cs=0: seq.lib.mot_get_sequence_scene_points(
            seq._h, frames, C.byref(P) if P is not None else None, mask, frame, vp(pts) if pts is not None else None, C.c_long(pcap), C.byref(n) if n is not None else None,
            vp(seg) if seg is not None else None, vp(tot) if tot is not None else None, vp(cls) if cls is not None else None, C.c_long(cs))
        for what, kw in (("frames 0", dict(frames=0)), ("frames 4", dict(frames=F + 1)), ("null params", dict(P=None)), ("mask", dict(mask=32)), ("frame", dict(frame=2)), ("null n_points", dict(n=None)),
                         ("null segments", dict(seg=None)), ("null totals", dict(tot=None)), ("negative capacity", dict(pcap=-1)), ("negative class stride", dict(cs=-1))):
            assert raw_get(**kw) == E.MOT_E_ARG, what
        assert n.value == -7 and (hs == -7).all() and (ht == -7).all()
        for pcap, cs in ((total - 1, widest), (total, widest - 1)):
            hs[:] = -7; ht[:] = -7; n.value = -7
            assert raw_get(pts=pts, pcap=pcap, cls=kb, cs=cs) == E.MOT_E_CAPACITY
            assert n.value == total and hs.tobytes() == seg.tobytes() and ht.tobytes() == tot.tobytes() and (pts == -7).all() and (kb == CLS_SENT).all()
        assert raw_get(pts=pts, pcap=total, cls=kb, cs=widest) == 0 and pts[: total * 4].tobytes() == rec.tobytes() and (pts[total * 4:] == -7).all() and kb[-1] == CLS_SENT
        for f in range(F):
            assert kb[f * widest: f * widest + obs[f]["n"]].tobytes() == cls[f].tobytes() and (kb[f * widest + obs[f]["n"]: (f + 1) * widest] == CLS_SENT).all(), f
        assert raw_get(mask=0b10000) == 0 and n.value == sum(int((k == KNOWN).sum()) for k in cls), "null buffers: the counts alone"


# ------------------------------------------------------------------------------------------------------------------ 7: non-interference
def judge_calls(env, c, F, total, stride):
    blk = Blocks(env, F, total, stride)
    for mask, frame in ((ALL, "global"), (0b10100, "sensor")):
        out = blk.run(c, F, mask, frame)
        assert int(out[2][:, 1].sum()) > 0
    c.get_sequence_scene_points(F, classes=(KNOWN, NEW)); c.get_sequence_scene_points(1)
    blk.free()


def non_interference(env, oracle, order_any=False):
    """two sequence calls in a row with both products: the grid, the accumulators' rows and the call's own outputs (every slot's readout, d_tracks / d_counts) are
    byte-identical with and without judge calls between them; the second call continues the same grid"""
    import track_accum_seq_cases as SQ
    clouds = [CC.small_scene(f, 20) for f in range(4)]
    if order_any:
        clouds = [np.ascontiguousarray(x[np.random.default_rng(11 + f).permutation(len(x))]) for f, x in enumerate(clouds)]
    res = {}
    for tag in ("never", "judged"):
        with env.context(0, max_points=4096, max_batch=2, max_tracks_total=256) as c:
            c.set_track_links(True); c.set_track_accumulation(256, 4); c.set_scene_grid(1.0, 64)
            if order_any:
                c.set_point_order(env.mot.MOT_ORDER_ANY)
            out = []
            for f0 in (0, 2):
                tb = SQ.TrackBlocks(env, 2, 64)
                keep = SGQ.seq_call(env, c, clouds[f0:f0 + 2], 4096, f0, [1.0] * 2, [0.02 * f0, 0.02 * (f0 + 1)], accumulate=True, tracks=tb.args())
                if tag == "judged":
                    judge_calls(env, c, 2, 2 * 4096, 4096)
                items = SQ.sequence_readout(env, c, [len(x) for x in clouds[f0:f0 + 2]]) + tb.read()
                items += [("rows", c.get_accum_rows(0).tobytes())] + [("grid " + n, x) for n, x in SGQ.grid_state(env, c, 64)]
                if tag == "judged":
                    judge_calls(env, c, 2, 2 * 4096, 4096)   # (the readers took no slot and changed no grid)
                out.append(items)
            assert int(SGQ.header(c)["step"][0]) == 3
            res[tag] = out
    for k in range(2):
        PC.equal_readouts(res["judged"][k], res["never"][k], (k, "against a context that never judged"))


# ------------------------------------------------------------------------------------------------------------------ 8: determinism
def run_script(env, c):
    clouds, ego_v, yaw = SGQ.drive(env)
    c.set_track_links(True); c.set_scene_grid(0.27, 64)
    out = []
    for f0 in (0, 8):
        SGQ.seq_call(env, c, clouds[f0:f0 + 8], 2048, f0, ego_v[f0:f0 + 8], yaw[f0:f0 + 8])
        blk = Blocks(env, 8, 8 * 2048, 2048)
        blk.run(c, 8, ALL, "global"); first = [x.tobytes() for x in blk.raw()]
        blk.run(c, 8, ALL, "global")
        assert [x.tobytes() for x in blk.raw()] == first, (f0, "two calls on one state differ")
        blk.free()
        out.append(first)
    return out


def determinism(env, oracle):
    """two calls on one state give identical bytes; the same steps in two contexts give identical bytes"""
    runs = []
    for k in range(2):
        with env.context(0, max_points=2048, max_batch=8, max_tracks_total=256) as c:
            runs.append(run_script(env, c))
    assert runs[0] == runs[1]
    tot = np.frombuffer(runs[0][-1][2], np.int32)[2: 12].reshape(5, 2)
    assert (tot[:, 1] > 0).sum() >= 3, tot


# ------------------------------------------------------------------------------------------------------------------ 10: emulator only
def launches_only_in_the_new_calls(env, oracle):
    """emulator: the four kernels' launch counters move in the new calls and nowhere else (the scatter only with a mask and room for records); the same number of launches
    for 2 and for 257 frames; the scratch goes with the grid and with mot_destroy"""
    lib = env.mot.load_library(env.lib_path)
    lib.hipemu_live_allocs.restype = C.c_long
    count = lambda: [lib.hipemu_launch_count(k) for k in KERNELS]
    base = lib.hipemu_live_allocs()
    per_call = {}
    for F in (2, 257):
        clouds = [CC.small_scene(f % 5, 2) for f in range(F)]
        with env.context(0, max_points=1024, max_batch=F, max_tracks_total=64) as c:
            c.set_track_links(True); c.set_scene_grid(1.0, 64)
            before = count()
            old = [lib.hipemu_launch_count(k) for k in SJ.KERNELS]
            keep = AC.launch(env, c, clouds[:2], 1024, 0); c.accumulate_scene(2)
            SGQ.seq_call(env, c, clouds[:2], 1024, 1, [1.0] * 2, [0.0] * 2, scene=False)
            SGQ.seq_call(env, c, clouds, 1024, 3, [1.0] * F, [0.0] * F)
            c.get_scene_grid(0); c.get_track_points(0, frame="global"); c.get_point_tracks(1)
            allocs = lib.hipemu_live_allocs()
            assert count() == before, "a kernel of the drive's judge ran outside the new calls"
            blk = Blocks(env, F, F * 1024, 1024)
            assert raw_export(c, env.mot, blk, frames=F, mask=32) == env.mot.MOT_E_ARG
            assert lib.hipemu_live_allocs() == allocs and count() == before, "a refused call allocated or launched"
            blk.run(c, F, ALL, "global")
            assert count() == [n + 1 for n in before] and lib.hipemu_live_allocs() == allocs + 4   # class bytes, rows, arguments, bases
            blk.run(c, F, 0, "global")
            blk.run(c, F, 0, "global", points=False)
            assert count() == [before[0] + 3, before[1] + 3, before[2] + 3, before[3] + 1], "mask 0: the scatter is not launched"
            c.get_sequence_scene_points(F)   # (two calls: the counts alone, then the records)
            assert count() == [before[0] + 5, before[1] + 5, before[2] + 5, before[3] + 2] and lib.hipemu_live_allocs() == allocs + 5   # (the getter's table block)
            assert [lib.hipemu_launch_count(k) for k in SJ.KERNELS] == old, "a kernel of the per-frame judge ran"
            per_call[F] = [a - b for a, b in zip(count(), before)]
            c.set_scene_grid(None)
            assert lib.hipemu_live_allocs() < allocs, "turning the grid off did not free the scratch"
            c.set_scene_grid(1.0, 64)
            SGQ.seq_call(env, c, clouds[:2], 1024, 0, [1.0] * 2, [0.0] * 2)
            c.get_sequence_scene_points(2, classes=(KNOWN,))
        assert lib.hipemu_live_allocs() == base, "mot_destroy left allocations of the feature behind"
    assert per_call[2] == per_call[257], per_call


def scratch_under_allocation_failure(env, oracle):
    """emulator: each of the four scratch allocations failing in turn at the first call -> MOT_E_HIP, nothing kept, the caller's blocks untouched; the next call succeeds
    and gives the bytes of the model"""
    lib = env.mot.load_library(env.lib_path)
    lib.hipemu_live_allocs.restype = C.c_long
    lib.hipemu_fail_alloc_at.argtypes = [C.c_long]; lib.hipemu_fail_alloc_at.restype = None
    E = env.mot
    F = 3
    clouds = [CC.small_scene(f, 20) for f in range(F)]
    try:
        seq, ref = contexts(env, F, 1.0, 64, 4096, 64)
        with seq, ref:
            ex = Expect(env, ref, 1.0, 4096)
            obs, keep = call_and_expect(env, seq, ex, clouds, 4096, [1.0] * F, [0.0] * F)
            seq.get_scene_grid(0)
            blk = Blocks(env, F, F * 4096, 4096); sentinel = blk.raw()
            allocs = lib.hipemu_live_allocs()
            for k in (1, 2, 3, 4):
                lib.hipemu_fail_alloc_at(k)
                rc = AC.code_of(env, lambda: seq.export_sequence_scene_points_dev(F, blk.a_pts, blk.cap, blk.a_seg, blk.a_tot, blk.a_cls, blk.cs))
                lib.hipemu_fail_alloc_at(0)
                assert rc == E.MOT_E_HIP and lib.hipemu_live_allocs() == allocs, k
                assert all((a == b).all() for a, b in zip(blk.raw(), sentinel)), k
            lib.hipemu_fail_alloc_at(5)   # the getter's table block, behind the four
            rc = AC.code_of(env, lambda: seq.get_sequence_scene_points(F))
            lib.hipemu_fail_alloc_at(0)
            assert rc == E.MOT_E_HIP and lib.hipemu_live_allocs() == allocs
            judge_and_check(env, seq, obs, SJ.PARAMS[:1], "after the failed attempts")
            assert lib.hipemu_live_allocs() == allocs + 5
    finally:
        lib.hipemu_fail_alloc_at(0)
