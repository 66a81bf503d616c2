"""A frame's points judged against the scene grid (mot_export_scene_points_dev / mot_get_scene_points, csrc/scene_judge.hip): bodies shared by
tests/test_emu_scene_judge.py (emulator) and tests/test_scene_judge_gpu.py (MI355X). The callers supply a capacity_cases.Env.

The expectation is a numpy model that shares no code with the kernels and uses only getters that exist without the feature, read BEFORE the call: get_scene_grid
(cells and header), get_track_points(rest=True) in the global frame (coordinates, owners, indices) and in the sensor frame (the elevated cloud's bits),
get_tracks()["is_static"], and sensor_pose at every accepted mot_accumulate_scene (whether that step's window could be placed, by the rule of
scene_grid_cases.Model.fold). The rules of include/mot.h are applied in np.float32 and np.uint64; class bytes, segment tables and records are compared AS BYTES,
through the export (sentinel margins on both sides of every block) and through the getter. There is no tolerance anywhere."""
import ctypes as C
from math import gcd

import numpy as np

import capacity_cases as CC
import scene_grid_cases as SG
import track_accum_cases as AC
import track_link_cases as LC
import track_point_cases as PC

UNKNOWN, MOVING, TRAIL, NEW, KNOWN = range(5)
ALL = 0b11111
MASKS = (0, 1, 2, 4, 8, 16, 0b10100, ALL)
LIMIT = SG.LIMIT
CLS_SENT = 0xF9


# ------------------------------------------------------------------------------------------------------------------ the model
def placeable(c, b, inv):
    """could the window of the step slot b holds be placed (scene_grid_cases.Model.fold's rule)"""
    m = c.sensor_pose(b)[1]
    with np.errstate(over="ignore", invalid="ignore"):
        a, e = np.float32(m[0, 3]) * inv, np.float32(m[1, 3]) * inv
        return bool(np.isfinite(a) and np.isfinite(e) and abs(a) < LIMIT and abs(e) < LIMIT)


class Windows:
    """per slot: did the latest ACCEPTED mot_accumulate_scene place its window — bookkeeping of the test, read from sensor_pose when the call is made"""

    def __init__(self, B, cell):
        self.ok = [False] * B
        self.inv = np.float32(1.0) / np.float32(cell)

    def accumulate(self, c, batch):
        for b in range(batch):
            self.ok[b] = placeable(c, b, self.inv)
        c.accumulate_scene(batch)

    def restart(self, b):
        self.ok[b] = False


def observe(c, b, ok):
    """everything the verdicts of slot b depend on, from the getters that exist without the feature"""
    g = c.get_scene_grid(b)
    h = g["header"]
    W = int(h["size"]); inv = np.float32(1.0) / np.float32(h["cell"])
    ok = bool(ok) and int(h["step"]) >= 0   # (no step yet: nothing takes part)
    rg = c.get_track_points(b, rest=True, frame="global"); rs = c.get_track_points(b, rest=True, frame="sensor")
    idx = rg["index"]; n = len(idx)
    assert np.array_equal(idx, rs["index"]) and np.array_equal(np.sort(idx), np.arange(n))
    glob = np.zeros((n, 3), np.float32); sensor = np.zeros((n, 3), np.float32); ids = np.full(n, -1, np.int64)
    glob[idx] = rg["xyz"]; sensor[idx] = rs["xyz"]; ids[idx] = SG.owners(rg)
    static_flag = c.get_tracks(b)["is_static"]
    owned = ids >= 0
    flagged = np.zeros(n, bool); flagged[owned] = static_flag[ids[owned]] != 0
    moving = owned & ~flagged
    with np.errstate(over="ignore", invalid="ignore"):
        tx, ty = glob[:, 0] * inv, glob[:, 1] * inv
        take = np.isfinite(glob).all(axis=1) & (np.abs(tx) < LIMIT) & (np.abs(ty) < LIMIT) & ok
        gi = np.where(take, np.floor(tx), 0).astype(np.int64); gj = np.where(take, np.floor(ty), 0).astype(np.int64)
    u, v = gi - int(h["origin_i"]), gj - int(h["origin_j"])
    in_window = (u >= 0) & (u < W) & (v >= 0) & (v < W)
    take &= in_window
    s = np.zeros(n, np.uint64); d = np.zeros(n, np.uint64)
    s[take] = g["cells"]["static_hits"][v[take], u[take]]; d[take] = g["cells"]["dynamic_hits"][v[take], u[take]]
    return dict(n=n, glob=glob, sensor=sensor, ids=ids, owned=owned, flagged=flagged, moving=moving, take=take, in_window=in_window, s=s, d=d, u=u, v=v, ok=ok)


def classify(o, min_static_hits, num, den):
    """the rules of include/mot.h, lowest priority first"""
    s, d = o["s"], o["d"]
    cls = np.full(o["n"], KNOWN, np.uint8)
    cls[s < np.uint64(min_static_hits)] = NEW
    cls[(d > 0) & (d * np.uint64(den) > (s + d) * np.uint64(num))] = TRAIL
    cls[~o["take"]] = UNKNOWN
    cls[o["moving"]] = MOVING
    return cls


def records(o, cls, mask, frame):
    """-> the segment table [5, 2] and the records [m, 4] as int32"""
    xyz = (o["glob"] if frame == "global" else o["sensor"]).view(np.int32)
    seg = np.zeros((5, 2), np.int32); recs = []; run = 0
    for k in range(5):
        at = np.nonzero(cls == k)[0]
        seg[k] = (run if (mask >> k) & 1 else -1, len(at))
        if (mask >> k) & 1:
            r = np.zeros((len(at), 4), np.int32); r[:, :3] = xyz[at]; r[:, 3] = at
            recs.append(r); run += len(at)
    return seg, (np.concatenate(recs) if recs else np.zeros((0, 4), np.int32))


class Blocks:
    """sentinel-filled device blocks for mot_export_scene_points_dev: [B][point_stride] records, [B][5] segments, [B][class_stride] class bytes, a margin on both sides
    of each; misalign: the records and the segments start 4 bytes off a 16-byte (8-byte) boundary"""

    def __init__(self, env, B, point_stride, class_stride, misalign=False):
        self.B, self.ps, self.cs, self.off = B, point_stride, class_stride, (1 if misalign else 0)
        self.h_pts = np.full(4 + 1 + B * point_stride * 4 + 4, -7, np.int32); self.h_seg = np.full(2 + 1 + B * 10 + 2, -7, np.int32)
        self.h_cls = np.full(16 + B * class_stride + 16, CLS_SENT, np.uint8)
        (self.p_pts, self.k_pts), (self.p_seg, self.k_seg), (self.p_cls, self.k_cls) = env.upload(self.h_pts), env.upload(self.h_seg), env.upload(self.h_cls)
        assert self.p_pts % 16 == 0
        self.a_pts, self.a_seg, self.a_cls = self.p_pts + 16 + 4 * self.off, self.p_seg + 8 + 4 * self.off, self.p_cls + 16

    def run(self, c, batch, mask, frame, params=(1, 1, 2), points=True, classes=True):
        c.export_scene_points_dev(batch, self.a_pts if points else 0, self.ps if points else 0, self.a_seg, self.a_cls if classes else 0, self.cs,
                                  min_static_hits=params[0], trail=params[1:], classes=mask, frame=frame)
        c.synchronize()
        return self.read(batch)

    def raw(self):
        return tuple(LC.download(k, h).copy() for k, h in ((self.k_pts, self.h_pts), (self.k_seg, self.h_seg), (self.k_cls, self.h_cls)))

    def read(self, batch):
        pts, seg, cls = self.raw()
        B, o = self.B, self.off
        assert (pts[: 4 + o] == -7).all() and (pts[4 + o + batch * self.ps * 4:] == -7).all(), "records outside the slots' blocks"
        assert (seg[: 2 + o] == -7).all() and (seg[2 + o + batch * 10:] == -7).all(), "segments outside the slots' blocks"
        assert (cls[:16] == CLS_SENT).all() and (cls[16 + batch * self.cs:] == CLS_SENT).all(), "class bytes outside the slots' blocks"
        return (pts[4 + o: 4 + o + B * self.ps * 4].reshape(B, self.ps, 4), seg[2 + o: 2 + o + B * 10].reshape(B, 5, 2), cls[16: 16 + B * self.cs].reshape(B, self.cs))

    def free(self):
        for k in (self.k_pts, self.k_seg, self.k_cls):
            if hasattr(k, "free"):
                k.free()


def check_slot(blk, out, b, o, cls, mask, frame, what, points=True, classes=True):
    """slot b of an export's blocks against the model: the table, the records that fit, the class bytes that fit, the sentinel behind them"""
    p, s, k = out
    seg, rec = records(o, cls, mask, frame)
    assert s[b].tobytes() == seg.tobytes(), (what, "slot", b, "segments", s[b].tolist(), seg.tolist())
    w = min(len(rec), blk.ps) if points else 0
    if p[b, :w].tobytes() != rec[:w].tobytes():
        bad = np.argwhere(p[b, :w] != rec[:w])
        raise AssertionError((what, "slot", b, "records", len(bad), "words differ; first", bad[0], p[b, bad[0][0]], rec[bad[0][0]]))
    assert (p[b, w:] == -7).all(), (what, "slot", b, "written beyond the slot's records")
    wc = min(o["n"], blk.cs) if classes else 0
    assert k[b, :wc].tobytes() == cls[:wc].tobytes(), (what, "slot", b, "class bytes", np.argwhere(k[b, :wc] != cls[:wc])[:4])
    assert (k[b, wc:] == CLS_SENT).all(), (what, "slot", b, "class bytes beyond the slot's points")


def check_getter(c, b, o, cls, mask, frame, params, what):
    r = c.get_scene_points(b, min_static_hits=params[0], trail=params[1:], classes=mask, frame=frame)
    seg, rec = records(o, cls, mask, frame)
    got = np.zeros((len(r["index"]), 4), np.int32); got[:, :3] = np.ascontiguousarray(r["xyz"], np.float32).view(np.int32).reshape(-1, 3); got[:, 3] = r["index"]
    assert r["segments"].tobytes() == seg.tobytes() and got.tobytes() == rec.tobytes() and r["classes"].tobytes() == cls.tobytes(), (what, "slot", b, "getter")
    for first, n in seg:
        if first >= 0:
            assert (np.diff(r["index"][first: first + n]) > 0).all(), (what, "index not ascending inside a segment")


def judge_and_check(env, c, win, B, params_list, what, facts=None, mask=ALL, frame="global", stride=None):
    """the model from the getters first, then the export and the getter for every parameter set"""
    obs = [observe(c, b, win.ok[b]) for b in range(B)]
    stride = stride or max(max(o["n"] for o in obs), 1) + 3
    for params in params_list:
        cls = [classify(o, *params) for o in obs]
        blk = Blocks(env, B, stride, stride)
        out = blk.run(c, B, mask, frame, params)
        for b in range(B):
            check_slot(blk, out, b, obs[b], cls[b], mask, frame, (what, params))
            check_getter(c, b, obs[b], cls[b], mask, frame, params, (what, params))
            if facts is not None:
                tally(facts, obs[b], cls[b])
        blk.free()
    return obs


def tally(f, o, cls):
    for k, name in enumerate(("unknown", "moving", "trail", "new", "known")):
        f[name] = f.get(name, 0) + int((cls == k).sum())
    f["parked_trail"] = f.get("parked_trail", 0) + int(((cls == TRAIL) & o["flagged"]).sum())      # a track that turned static over its earlier dynamic hits
    f["moving_outside"] = f.get("moving_outside", 0) + int(((cls == MOVING) & ~o["in_window"]).sum())
    f["unknown_unowned"] = f.get("unknown_unowned", 0) + int(((cls == UNKNOWN) & ~o["owned"]).sum())
    f["unknown_outside"] = f.get("unknown_outside", 0) + int(((cls == UNKNOWN) & o["ok"] & ~o["in_window"]).sum())


# ------------------------------------------------------------------------------------------------------------------ 1: standing and moving objects
PARAMS = ((1, 1, 2), (50, 1, 2), (1, 0, 1), (1, 1, 1))


def standing_and_moving(env, oracle, cell, W):
    """scene_grid_cases.standing_and_moving's scene (two blobs that stand in the world, one that moves; three streams, the sensor driving and turning), a copy with a
    fourth blob: a second mover far out, outside every window of the run. Judged before every mot_accumulate_scene and again after it, four parameter sets. That the
    run shows every class — and the parked-car trail among them — is asserted from the model's own bookkeeping."""
    frames_n, B = 16, 3
    ego_v = [0.0, 1.0, 1.0]; yaws = [[0.0, 0.0, 0.04 * f] for f in range(frames_n)]
    S = SG.sensor_from_world(env, ego_v, yaws, frames_n)
    rngs = [np.random.default_rng(3 + b) for b in range(B)]
    facts = {}
    with env.context(0, max_points=2048, max_batch=B, max_tracks_total=256) as c:
        c.set_track_links(True); c.set_scene_grid(cell, W)
        win = Windows(B, cell)
        for f in range(frames_n):
            world = lambda b: np.concatenate([SG.world_blob(rngs[b], 8.0, 5.0), SG.world_blob(rngs[b], 3.0, -7.0), SG.world_blob(rngs[b], -9.0, -6.0 - 0.3 * f),
                                              SG.world_blob(rngs[b], 21.0 - 0.3 * f, 20.0, n=100)])
            keep = AC.launch(env, c, [SG.to_sensor(S[f, b], world(b)) for b in range(B)], 2048, f, ego_v=ego_v, yaw=yaws[f])
            judge_and_check(env, c, win, B, PARAMS, ("standing and moving", cell, W, f, "before"), facts)
            win.accumulate(c, B)
            judge_and_check(env, c, win, B, PARAMS, ("standing and moving", cell, W, f, "after"), facts)
    for k in ("unknown", "moving", "trail", "new", "known", "parked_trail", "moving_outside", "unknown_unowned"):
        assert facts.get(k, 0) > 0, (k, facts)
    return facts


# ------------------------------------------------------------------------------------------------------------------ 2: chunk, tile and wave edges
def shapes(env, oracle, order_any=False):
    """elevated counts 0, 1, 63, 64, 65, the chunk (2048) - 1 / exact / + 1, 5000 and a full frame (track_point_cases.shape_frames), three steps: every mask in both
    frames; strides one below and at a slot's need; a block 4 bytes off; counts alone; no class block"""
    frames = PC.shape_frames(oracle)
    targets = [len(x) for x in frames[0]]
    assert {0, 1, 63, 64, 65, 2047, 2048, 2049, 5000} <= set(targets)
    B, W = len(targets), 64
    facts = {}
    with env.context(0, max_points=8192, max_batch=B, max_tracks_total=512) as c:
        c.set_track_links(True); c.set_scene_grid(1.0, W)
        if order_any:
            c.set_point_order(env.mot.MOT_ORDER_ANY)
        win = Windows(B, 1.0)
        params = (2, 1, 3)
        for f in range(3):
            sent = [np.ascontiguousarray(x[np.random.default_rng(7 + b).permutation(len(x))]) for b, x in enumerate(frames[f])] if order_any else frames[f]
            keep = AC.launch(env, c, sent, 8192, f)
            if f == 0:
                win.accumulate(c, B)   # (frame 0 is judged against its own hits, the later frames against history)
            obs = [observe(c, b, win.ok[b]) for b in range(B)]
            assert [o["n"] for o in obs] == targets
            cls = [classify(o, *params) for o in obs]
            for b in range(B):
                tally(facts, obs[b], cls[b])
            full = max(targets) + 3
            for mask in MASKS:
                for frame in ("global", "sensor"):
                    blk = Blocks(env, B, full, full)
                    out = blk.run(c, B, mask, frame, params)
                    for b in range(B):
                        check_slot(blk, out, b, obs[b], cls[b], mask, frame, ("shapes", order_any, f, mask, frame))
                    blk.free()
            for b in (1, 4, 7, 9):   # 1, 65, 2049 points and the full frame through the getter
                for mask, frame in ((ALL, "global"), (0b10100, "sensor"), (0, "global")):
                    check_getter(c, b, obs[b], cls[b], mask, frame, params, ("shapes", order_any, f, mask, frame))
            # strides one below and at a slot's need (the other slots then fit or are cut: all are checked); a block 4 bytes off; counts alone; no class block
            for b in (7, 9):
                for mask in (ALL, 0b10100):
                    need = int(sum((cls[b] == k).sum() for k in range(5) if (mask >> k) & 1))
                    for ps, cs, mis in ((max(need - 1, 0), targets[b] - 1, False), (need, targets[b], True)):
                        blk = Blocks(env, B, ps, cs, misalign=mis)
                        out = blk.run(c, B, mask, "global", params)
                        for k in range(B):
                            check_slot(blk, out, k, obs[k], cls[k], mask, "global", ("shapes, strides", order_any, f, b, mask, ps, cs))
                        blk.free()
            blk = Blocks(env, B, 0, full)
            out = blk.run(c, B, 0, "global", params, points=False)
            for b in range(B):
                check_slot(blk, out, b, obs[b], cls[b], 0, "global", ("shapes, counts and classes alone", order_any, f), points=False)
            blk.free()
            blk = Blocks(env, B, 0, 0)
            out = blk.run(c, B, 0, "sensor", params, points=False, classes=False)
            for b in range(B):
                check_slot(blk, out, b, obs[b], cls[b], 0, "sensor", ("shapes, counts alone", order_any, f), points=False, classes=False)
            blk.free()
            blk = Blocks(env, B, full, full)
            out = blk.run(c, B, ALL, "sensor", params, classes=False)
            for b in range(B):
                check_slot(blk, out, b, obs[b], cls[b], ALL, "sensor", ("shapes, no class block", order_any, f), classes=False)
            blk.free()
            if f > 0:
                win.accumulate(c, B)
    for k in ("unknown", "moving", "new", "known"):
        assert facts.get(k, 0) > 0, (k, facts)
    return facts


# ------------------------------------------------------------------------------------------------------------------ 3: threshold edges
def thresholds(env, oracle):
    """scene_grid_cases.contention's scene (cell 10: one or two cells take every point), four frames. The counters are read back; for each hit cell min_static_hits
    = s and s + 1, and num / den with d * den == (s + d) * num exactly and one either side of it: the class flips exactly where the contract says"""
    W = 64
    rng = np.random.default_rng(21)
    S = SG.sensor_from_world(env, [0.0, 0.0], [[0.0, 0.0]] * 4, 4)
    seen = dict(exact=0, below=0, above=0, new=0, known=0, both=0)
    with env.context(0, max_points=2048, max_batch=2, max_tracks_total=64) as c:
        c.set_track_links(True); c.set_scene_grid(10.0, W)
        win = Windows(2, 10.0)
        for f in range(4):
            one = np.concatenate([SG.world_blob(rng, 3.0, 4.0, 400), SG.world_blob(rng, 7.0, 6.0, 400), SG.world_blob(rng, 5.0, 2.0, 300)])
            two = np.concatenate([SG.world_blob(rng, 3.0, 4.0, 500), SG.world_blob(rng, 13.0, 6.0, 500)])
            keep = AC.launch(env, c, [SG.to_sensor(S[f, 0], one), SG.to_sensor(S[f, 1], two)], 2048, f, ego_v=[0.0, 0.0])
            for when in ("before", "after"):
                if when == "after":
                    win.accumulate(c, 2)
                obs = [observe(c, b, win.ok[b]) for b in range(2)]
                cells = sorted({(int(s), int(d)) for o in obs for s, d, t in zip(o["s"], o["d"], o["take"] & ~o["moving"]) if t})
                for s, d in cells:
                    here = [o["take"] & ~o["moving"] & (o["s"] == s) & (o["d"] == d) for o in obs]
                    g = gcd(d, s + d) or 1
                    num, den = d // g, (s + d) // g
                    assert den <= 65535 and d * den == (s + d) * num
                    sets = [("exact", (max(s, 1), num, den))]
                    if num >= 1 and 2 * den <= 65535:
                        sets.append(("below", (max(s, 1), 2 * num - 1, 2 * den)))
                    if 2 * num + 1 <= 2 * den <= 65535:
                        sets.append(("above", (max(s, 1), 2 * num + 1, 2 * den)))
                    if s >= 1:
                        sets += [("known", (s, num, den)), ("new", (s + 1, num, den))]
                    for name, params in sets:
                        cls = [classify(o, *params) for o in obs]
                        mine = np.concatenate([k[h] for k, h in zip(cls, here)])
                        want = dict(exact=(NEW, KNOWN), below=(TRAIL,), above=(NEW, KNOWN), known=(KNOWN,), new=(NEW,))[name]
                        if name == "below" and d == 0:
                            want = (NEW, KNOWN)
                        assert len(mine) and np.isin(mine, want).all(), (f, when, s, d, name, params, np.unique(mine))
                        seen[name] += 1; seen["both"] += int(s > 0 and d > 0)
                        blk = Blocks(env, 2, 2048, 2048)
                        out = blk.run(c, 2, ALL, "global", params)
                        for b in range(2):
                            check_slot(blk, out, b, obs[b], cls[b], ALL, "global", ("thresholds", f, when, s, d, name, params))
                        blk.free()
    assert all(v > 0 for v in seen.values()), seen
    return seen


# ------------------------------------------------------------------------------------------------------------------ 4: scroll
def scroll(env, oracle, cell=0.25, W=64):
    """the ten streams of scene_grid_cases.scroll (a copy with one more blob, near the sensor: inside the 16 m windows), judged before and after every accumulate: windows that stay, shift by one cell, by several, by more than W, and a
    last stream that drives out of the range a window can be placed in"""
    frames_n = 10
    spec = [(0.0, lambda f: 0.0), (2.5, lambda f: 0.0), (10.0, lambda f: 0.0), (1.0, lambda f: 0.0), (200.0, lambda f: 0.0), (10.0, lambda f: np.pi),
            (10.0, lambda f: np.pi / 2), (10.0, lambda f: np.pi / 4), (10.0, lambda f: 0.5 * f), (3.0e9, lambda f: 0.0)]
    B = len(spec)
    ego_v = [s[0] for s in spec]
    facts = {}
    last = dict(good_then_bad_before=0, after_bad=0, shifts=[set() for _ in range(B)])
    rngs = [np.random.default_rng(31 + b) for b in range(B)]
    with env.context(0, max_points=1024, max_batch=B, max_tracks_total=64) as c:
        c.set_track_links(True); c.set_scene_grid(cell, W)
        win = Windows(B, cell)
        for f in range(frames_n):
            clouds = [np.concatenate([CC.small_scene(f + b, 8), SG.world_blob(rngs[b], 3.0, 2.0, 120)]) for b in range(B)]   # (the scene's blobs lie 30 m out: one more, near the sensor)
            keep = AC.launch(env, c, clouds, 1024, f, ego_v=ego_v, yaw=[s[1](f) for s in spec])
            origin = [tuple(int(c.get_scene_grid(b, cells=False)["header"][k]) for k in ("origin_i", "origin_j")) for b in range(B)]
            was_ok = list(win.ok)
            before = judge_and_check(env, c, win, B, PARAMS[:2], ("scroll", f, "before"), facts)
            win.accumulate(c, B)
            after = judge_and_check(env, c, win, B, PARAMS[:2], ("scroll", f, "after"), facts)
            for b in range(B):
                now = tuple(int(c.get_scene_grid(b, cells=False)["header"][k]) for k in ("origin_i", "origin_j"))
                if f > 0:
                    last["shifts"][b].add(max(abs(now[0] - origin[b][0]), abs(now[1] - origin[b][1])))
                if not win.ok[b]:   # the step's window could not be placed: before its accumulate the points met the last good window, after it nothing takes part
                    assert not after[b]["take"].any() and after[b]["n"] > 0, (f, b)
                    last["after_bad"] += 1
                    last["good_then_bad_before"] += int(was_ok[b] and before[b]["ok"])
    sh = last["shifts"]
    assert sh[0] == {0} and 1 in sh[1] and any(1 < x < W for x in sh[2]) and any(x >= W for x in sh[4]), sh
    assert last["after_bad"] > 0 and last["good_then_bad_before"] > 0, last
    for k in ("unknown", "new", "known", "unknown_outside"):
        assert facts.get(k, 0) > 0, (k, facts)
    return facts


# ------------------------------------------------------------------------------------------------------------------ 5: contract
def code_of(env, fn):
    return AC.code_of(env, fn)


def raw_export(c, E, blk, batch=2, params=(1, 1, 2), mask=ALL, frame=0, points="a", pstride=None, segments="a", classes="a", cstride=None):
    P = E.MotSceneJudgeParams(*params) if params is not None else None
    ptr = lambda v, a: None if v is None else (a if v == "a" else v)
    return c.lib.mot_export_scene_points_dev(c._h, batch, C.byref(P) if P is not None else None, mask, frame, C.c_void_p(ptr(points, blk.a_pts)),
                                             C.c_long(blk.ps if pstride is None else pstride), C.c_void_p(ptr(segments, blk.a_seg)), C.c_void_p(ptr(classes, blk.a_cls)),
                                             C.c_long(blk.cs if cstride is None else cstride))


def contract(env, oracle):
    """every refusal with sentinel blocks unchanged; the states that answer MOT_E_STATE; MOT_E_CAPACITY of the getter with the counts delivered; a smaller batch;
    another geometry"""
    E = env.mot
    W = 64
    clouds = [[CC.small_scene(f, 20), CC.small_scene(f + 5, 12)] for f in range(10)]
    with env.context(0, max_points=4096, max_batch=2, max_tracks_total=64) as c:
        blk = Blocks(env, 2, 4096, 4096)
        sentinel = blk.raw()
        def untouched(what, before=None):
            c.synchronize()
            assert all((a == b).all() for a, b in zip(blk.raw(), before or sentinel)), (what, "a refused call wrote into the caller's blocks")
        export = lambda batch=2: c.export_scene_points_dev(batch, blk.a_pts, blk.ps, blk.a_seg, blk.a_cls, blk.cs)
        getter = lambda b=0: c.get_scene_points(b)
        def state_error(what, batch=2, slot=0):
            before = blk.raw()   # (served calls have written into the blocks since they were made)
            assert code_of(env, lambda: export(batch)) == E.MOT_E_STATE and code_of(env, lambda: getter(slot)) == E.MOT_E_STATE, what
            untouched(what, before)
        c.set_track_links(True)
        keep = AC.launch(env, c, clouds[0], 4096, 0)
        state_error("the feature off")
        c.set_scene_grid(1.0, W)
        win = Windows(2, 1.0)
        state_error("the step the slots hold was taken before the grid was on")
        keep = AC.launch(env, c, clouds[1], 4096, 1)
        judge_and_check(env, c, win, 2, PARAMS[:1], "contract, no step yet")
        win.accumulate(c, 2)
        keep = AC.launch(env, c, clouds[2], 4096, 2)
        # argument errors, on a context whose state would serve the call
        for what, kw in (("null params", dict(params=None)), ("null segments", dict(segments=None)), ("min_static_hits 0", dict(params=(0, 1, 2))),
                         ("min_static_hits 2^31 + 1", dict(params=(2 ** 31 + 1, 1, 2))), ("den 0", dict(params=(1, 0, 0))), ("den 65536", dict(params=(1, 1, 65536))),
                         ("num > den", dict(params=(1, 3, 2))), ("mask bit 5", dict(mask=32)), ("negative mask", dict(mask=-1)), ("frame 2", dict(frame=2)), ("frame -1", dict(frame=-1)),
                         ("batch 0", dict(batch=0)), ("batch 3", dict(batch=3)), ("negative point stride", dict(pstride=-1)), ("negative class stride", dict(cstride=-1)),
                         ("null points with a stride", dict(points=None, mask=0)), ("null points with a mask", dict(points=None, pstride=0)),
                         ("points off 4 bytes", dict(points=blk.a_pts + 2)), ("segments off 4 bytes", dict(segments=blk.a_seg + 2))):
            assert raw_export(c, E, blk, **kw) == E.MOT_E_ARG, what
            untouched(what)
        n, ne = C.c_int(-7), C.c_int(-7); seg = np.full(10, -7, np.int32); P = E.MotSceneJudgeParams(1, 1, 2)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        raw_get = lambda slot=0, P=P, mask=ALL, frame=0, pts=None, pcap=0, n=n, seg=seg, cls=None, ccap=0, ne=ne: c.lib.mot_get_scene_points(
            c._h, slot, C.byref(P) if P is not None else None, mask, frame, vp(pts) if pts is not None else None, pcap, C.byref(n) if n is not None else None,
            vp(seg) if seg is not None else None, vp(cls) if cls is not None else None, ccap, C.byref(ne) if ne is not None else None)
        for what, kw in (("slot 2", dict(slot=2)), ("slot -1", dict(slot=-1)), ("null params", dict(P=None)), ("mask", dict(mask=32)), ("frame", dict(frame=2)), ("null n_points", dict(n=None)),
                         ("null segments", dict(seg=None)), ("null n_elevated", dict(ne=None)), ("negative capacity", dict(pcap=-1)), ("negative class capacity", dict(ccap=-1)),
                         ("den 0", dict(P=E.MotSceneJudgeParams(1, 0, 0)))):
            assert raw_get(**kw) == E.MOT_E_ARG, what
        assert n.value == -7 and ne.value == -7 and (seg == -7).all()
        # the limits themselves are served
        served = Blocks(env, 2, 4096, 4096)
        assert raw_export(c, E, served, params=(2 ** 31, 65535, 65535)) == 0 and raw_export(c, E, served, params=(1, 0, 1)) == 0
        obs = [observe(c, b, win.ok[b]) for b in range(2)]
        cls = [classify(o, 1, 1, 2) for o in obs]
        # MOT_E_CAPACITY of the getter: the counts and the table are delivered, the buffers stay as they were
        want_seg, rec = records(obs[0], cls[0], ALL, "global")
        total = obs[0]["n"]
        assert total > 1
        pts = np.full((total + 1) * 4, -7, np.int32); kb = np.full(total + 1, CLS_SENT, np.uint8)
        for pcap, ccap in ((total - 1, total), (total, total - 1)):
            seg[:] = -7
            assert raw_get(pts=pts, pcap=pcap, cls=kb, ccap=ccap) == E.MOT_E_CAPACITY
            assert (n.value, ne.value) == (total, total) and seg.tobytes() == want_seg.tobytes() and (pts == -7).all() and (kb == CLS_SENT).all()
        assert raw_get(pts=pts, pcap=total, cls=kb, ccap=total) == 0 and pts[: total * 4].tobytes() == rec.tobytes() and (pts[total * 4:] == -7).all()
        assert kb[:total].tobytes() == cls[0].tobytes() and kb[total] == CLS_SENT
        assert raw_get(mask=0b10000) == 0 and n.value == int((cls[0] == KNOWN).sum()) and ne.value == total, "null buffers: the counts alone"
        # a batch smaller than max_batch leaves the other slot's blocks alone
        blk1 = Blocks(env, 2, 4096, 4096)
        out = blk1.run(c, 1, ALL, "global")
        check_slot(blk1, out, 0, obs[0], cls[0], ALL, "global", "batch 1 of 2")
        assert (out[0][1] == -7).all() and (out[1][1] == -7).all() and (out[2][1] == CLS_SENT).all()
        # legal again and again on one step, before and after the accumulate; the accumulate itself is still accepted once
        win.accumulate(c, 2)
        judge_and_check(env, c, win, 2, PARAMS[:2], "contract, after the accumulate")
        assert code_of(env, lambda: c.accumulate_scene(2)) == E.MOT_E_STATE
        # a stage-wise call takes slot 0
        keep = AC.launch(env, c, clouds[3], 4096, 3)
        elev = c.get_ground(0, n_hint=len(clouds[3][0]))["elevated"]
        c.cluster(elev)
        state_error("a stage-wise call took slot 0")
        getter(1)   # slot 1 alone is still whole
        keep = AC.launch(env, c, clouds[4], 4096, 4)
        export(); win.accumulate(c, 2)
        # a tracker step fed from outside
        c.ego_update(3.0e8, 0.0, 0.0, 1); c.track_step(LC.lattice(3), 3.0e8, slot=1)
        state_error("a tracker step fed from outside", slot=1)
        export(1); getter(0)
        # mot_reset_slot and mot_stream_load
        keep = AC.launch(env, c, clouds[5], 4096, 5)
        blob = c.stream_save(1)
        c.reset_slot(0); win.restart(0)
        state_error("mot_reset_slot")
        getter(1)
        keep = AC.launch(env, c, clouds[6], 4096, 6)
        judge_and_check(env, c, win, 2, PARAMS[:1], "contract, the step after a reset")
        c.stream_load(1, blob); win.restart(1)
        state_error("mot_stream_load", slot=1)
        export(1)
        # another geometry frees the scratch and makes it again
        keep = AC.launch(env, c, clouds[7], 4096, 7)
        export()
        c.set_scene_grid(0.5, 128)
        win = Windows(2, 0.5)
        state_error("the step the slots hold was taken with the old geometry")
        keep = AC.launch(env, c, clouds[8], 4096, 8)
        win.accumulate(c, 2)
        judge_and_check(env, c, win, 2, PARAMS[:2], "contract, another geometry")
        c.set_scene_grid(None)
        state_error("off again")
    # sequence mode
    with env.context(0, max_points=4096, max_batch=2, max_tracks_total=64) as c:
        c.set_track_links(True); c.set_scene_grid(1.0, W)
        host = np.zeros((2, 4096, 4), np.float32)
        for f in range(2):
            host[f, : len(clouds[f][0])] = clouds[f][0]
        ptr, keep = env.upload(host)
        c.sequence_dev(ptr, 4096 * 4, [len(clouds[f][0]) for f in range(2)], [2.0e8, 2.001e8], [1.0] * 2, [0.0] * 2)
        blk = Blocks(env, 2, 4096, 4096); sentinel = blk.raw()
        for fn in (lambda: c.export_scene_points_dev(2, blk.a_pts, blk.ps, blk.a_seg, blk.a_cls, blk.cs), lambda: c.export_scene_points_dev(1, blk.a_pts, blk.ps, blk.a_seg, blk.a_cls, blk.cs),
                   lambda: c.get_scene_points(0), lambda: c.get_scene_points(1)):
            assert code_of(env, fn) == E.MOT_E_STATE, "sequence slots"
        c.synchronize()
        assert all((a == b).all() for a, b in zip(blk.raw(), sentinel))


# ------------------------------------------------------------------------------------------------------------------ 6: non-interference
KERNELS = (b"scene_judge_classify_kernel", b"scene_judge_scan_kernel", b"scene_judge_scatter_kernel")


def judge_calls(env, c, B, stride):
    blk = Blocks(env, B, stride, stride)
    for mask, frame in ((ALL, "global"), (0b10100, "sensor")):
        out = blk.run(c, B, mask, frame)
        assert int(out[1][:, :, 1].sum()) > 0
    for b in range(B):
        c.get_scene_points(b, classes=(KNOWN, NEW))
    blk.free()


def non_interference(env, oracle, order_any=False, graphs=False):
    """a judge call changes not a byte of the grid and mot_accumulate_scene is still accepted after it; a run with judge calls interleaved leaves grids, boxes,
    tracks, point tracks, track points, the accumulators' rows and the raw track models byte-identical to a run without"""
    clouds = [[CC.small_scene(f, 20), CC.small_scene(f + 5, 12)] for f in range(4)]
    if order_any:
        clouds = [[np.ascontiguousarray(x[np.random.default_rng(11 + b).permutation(len(x))]) for b, x in enumerate(fr)] for fr in clouds]
    res = {}
    for tag in ("never", "judged"):
        with env.context(0, max_points=4096, max_batch=2, max_tracks_total=256) as c:
            c.set_launch_graphs(graphs); c.set_track_links(True); c.set_track_accumulation(256, 4); c.set_scene_grid(1.0, 64)
            if order_any:
                c.set_point_order(env.mot.MOT_ORDER_ANY)
            out = []
            for f in range(4):
                keep = PC.launch(env, c, clouds[f], 4096, f, yaw=0.02 * f)
                n_points = [len(x) for x in clouds[f]]
                before = PC.readout(c, 2, n_points)
                if tag == "judged":
                    grids = SG.grids(c, 2)
                    judge_calls(env, c, 2, 4096)
                    assert SG.grids(c, 2) == grids, (f, "a judge call changed a grid")
                    PC.equal_readouts(PC.readout(c, 2, n_points), before, (f, "after the judge calls"))
                c.accumulate_scene(2)   # (still accepted)
                c.accumulate_track_points(2)
                grids = SG.grids(c, 2)
                if tag == "judged":
                    judge_calls(env, c, 2, 4096)
                    assert SG.grids(c, 2) == grids, (f, "a judge call after the accumulate changed a grid")
                    PC.equal_readouts(PC.readout(c, 2, n_points), before, (f, "after the judge calls behind the accumulate"))
                tp = [(k + str(b), np.ascontiguousarray(v).tobytes()) for b in (0, 1) for k, v in sorted(c.get_track_points(b, rest=True, frame="global").items())]
                models = [(k + str(b), np.ascontiguousarray(v).tobytes()) for b in (0, 1) for k, v in sorted(c.get_track_models(b).items())]
                rows = [("rows" + str(b), c.get_accum_rows(b).tobytes()) for b in (0, 1)]
                gr = [("grid" + str(b) + part, x) for b, g in enumerate(grids) for part, x in zip(("header", "cells"), g)]
                out.append(AC.defined_items(before) + rows + models + tp + gr)
            res[tag] = out
    for f in range(4):
        PC.equal_readouts(res["judged"][f], res["never"][f], (f, "against a context that never judged"))


# ------------------------------------------------------------------------------------------------------------------ 7: determinism
def run_script(env, c, frames_n=4):
    B = 3
    c.set_track_links(True); c.set_scene_grid(1.0, 64)
    out = []
    for f in range(frames_n):
        keep = AC.launch(env, c, [CC.small_scene(f + 2 * b, 16) for b in range(B)], 2048, f, ego_v=[0.0, 3.0, 8.0], yaw=[0.0, 0.1 * f, -0.2 * f])
        for when in ("before", "after"):
            if when == "after":
                c.accumulate_scene(B)
            blk = Blocks(env, B, 2048, 2048)
            blk.run(c, B, ALL, "global"); first = [x.tobytes() for x in blk.raw()]
            blk.run(c, B, ALL, "global")
            assert [x.tobytes() for x in blk.raw()] == first, (f, when, "two calls on one state differ")
            blk.free()
            out.append(first)
    return out


def determinism(env, oracle):
    """two calls on one state give identical bytes; the same steps in two contexts give identical bytes"""
    runs = []
    for k in range(2):
        with env.context(0, max_points=2048, max_batch=3, max_tracks_total=64) as c:
            runs.append(run_script(env, c))
    assert runs[0] == runs[1]
    seg = np.stack([np.frombuffer(r[1], np.int32)[2: 2 + 30].reshape(3, 5, 2) for r in runs[0]])
    assert (seg[:, :, :, 1].sum(axis=(0, 1)) > 0).sum() >= 3, seg[:, :, :, 1].sum(axis=(0, 1))


# ------------------------------------------------------------------------------------------------------------------ 8: emulator only
def launches_only_in_the_new_calls(env, oracle):
    """emulator: the launch counters of the three kernels move in the new calls and nowhere else (the scatter only with a mask and room for records); the scratch is
    taken at the first call, the getter's staging block at its first call, and all of it goes with the grid and with mot_destroy"""
    lib = env.mot.load_library(env.lib_path)
    lib.hipemu_live_allocs.restype = C.c_long
    count = lambda: [lib.hipemu_launch_count(k) for k in KERNELS]
    base = lib.hipemu_live_allocs()
    with env.context(0, max_points=4096, max_batch=2, max_tracks_total=64) as c:
        before = count()
        c.set_track_links(True); c.set_scene_grid(1.0, 64)
        blk = Blocks(env, 2, 4096, 4096)
        for f in range(3):
            keep = PC.launch(env, c, [CC.small_scene(f, 20), CC.small_scene(f + 5, 12)], 4096, f)
            c.accumulate_scene(2)
            for b in (0, 1):
                c.get_point_tracks(b); c.get_tracks(b); c.get_track_points(b, frame="global"); c.get_scene_grid(b)
        allocs = lib.hipemu_live_allocs()
        assert count() == before, "a judge kernel ran outside the new calls"
        assert raw_export(c, env.mot, blk, mask=32) == env.mot.MOT_E_ARG
        assert lib.hipemu_live_allocs() == allocs and count() == before, "a refused call allocated or launched"
        blk.run(c, 2, ALL, "global")
        assert count() == [before[0] + 1, before[1] + 1, before[2] + 1] and lib.hipemu_live_allocs() == allocs + 3   # class bytes, rows, arguments
        blk.run(c, 2, 0, "global")
        assert count() == [before[0] + 2, before[1] + 2, before[2] + 1], "mask 0: the scatter is not launched"
        blk.run(c, 2, 0, "global", points=False)
        assert count() == [before[0] + 3, before[1] + 3, before[2] + 1] and lib.hipemu_live_allocs() == allocs + 3
        c.get_scene_points(1)
        assert count() == [before[0] + 4, before[1] + 4, before[2] + 2] and lib.hipemu_live_allocs() == allocs + 4   # (the getter's staging block)
        keep = PC.launch(env, c, [CC.small_scene(3, 20), CC.small_scene(8, 12)], 4096, 3)
        c.accumulate_scene(2); c.reset_slot(0)
        assert count() == [before[0] + 4, before[1] + 4, before[2] + 2]
        c.set_scene_grid(0.5, 128)
        assert lib.hipemu_live_allocs() == allocs - 1, "another geometry did not free the scratch"   # (mot_get_scene_grid's staging block goes too)
        keep = PC.launch(env, c, [CC.small_scene(4, 20), CC.small_scene(9, 12)], 4096, 4)
        blk.run(c, 2, ALL, "sensor")
        assert lib.hipemu_live_allocs() == allocs + 2
        c.set_scene_grid(None)
        c.set_scene_grid(1.0, 64)
        assert lib.hipemu_live_allocs() == allocs - 1, "turning the feature off did not free the scratch"
        keep = PC.launch(env, c, [CC.small_scene(5, 20), CC.small_scene(10, 12)], 4096, 5)
        c.get_scene_points(0)
    assert lib.hipemu_live_allocs() == base, "mot_destroy left allocations of the feature behind"


def scratch_under_allocation_failure(env, oracle):
    """emulator: each of the three scratch allocations failing in turn at the first call -> MOT_E_HIP, nothing kept, the caller's blocks untouched; the next call
    resumes and gives the bytes of the model"""
    lib = env.mot.load_library(env.lib_path)
    lib.hipemu_live_allocs.restype = C.c_long
    lib.hipemu_fail_alloc_at.argtypes = [C.c_long]; lib.hipemu_fail_alloc_at.restype = None
    E = env.mot
    try:
        with env.context(0, max_points=4096, max_batch=2, max_tracks_total=64) as c:
            c.set_track_links(True); c.set_scene_grid(1.0, 64)
            win = Windows(2, 1.0)
            keep = AC.launch(env, c, [CC.small_scene(0, 20), CC.small_scene(5, 12)], 4096, 0)
            win.accumulate(c, 2)
            obs = [observe(c, b, win.ok[b]) for b in range(2)]   # (the getters' own staging blocks exist from here on)
            blk = Blocks(env, 2, 4096, 4096); sentinel = blk.raw()
            allocs = lib.hipemu_live_allocs()
            for k in (1, 2, 3):
                lib.hipemu_fail_alloc_at(k)
                rc = code_of(env, lambda: c.export_scene_points_dev(2, blk.a_pts, blk.ps, blk.a_seg, blk.a_cls, blk.cs))
                lib.hipemu_fail_alloc_at(0)
                assert rc == E.MOT_E_HIP and lib.hipemu_live_allocs() == allocs, k
                assert all((a == b).all() for a, b in zip(blk.raw(), sentinel)), k
            judge_and_check(env, c, win, 2, PARAMS[:1], "after the failed attempts")
            assert lib.hipemu_live_allocs() == allocs + 4   # (the scratch and the getter's staging block)
    finally:
        lib.hipemu_fail_alloc_at(0)
