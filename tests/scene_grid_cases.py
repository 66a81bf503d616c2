"""Rolling static-scene grid (mot_set_scene_grid / mot_accumulate_scene, csrc/scene_grid.hip): bodies shared by tests/test_emu_scene_grid.py (emulator) and
tests/test_scene_grid_gpu.py (MI355X). The callers supply a capacity_cases.Env.

The expectation is a numpy model that shares no code with the kernels and is built only from getters that exist without the feature: per slot and step
get_track_points(rest=True, frame="global") (the global coordinates and, through the segments, every point's owner), get_tracks()["is_static"] and
sensor_pose()[1] (tx, ty). The rules of include/mot.h are applied in np.float32; the state is a dense [W, W] window plus an origin, shifted every step, the strips
that entered emptied, then np.add.at / np.maximum.at. After every step the header and all W^2 cells are compared AS BYTES, through the export and through the
getter; there is no tolerance anywhere."""
import ctypes as C

import numpy as np

import capacity_cases as CC
import track_accum_cases as AC
import track_link_cases as LC
import track_point_cases as PC

LIMIT = np.float32(2.0 ** 30)


# ------------------------------------------------------------------------------------------------------------------ the model
def zkey(z):
    """the total order of finite floats in which -0.0 lies below +0.0, as integers"""
    k = np.ascontiguousarray(z, np.float32).view(np.int32).astype(np.int64)
    return np.where(k >= 0, k, k ^ 0x7FFFFFFF)


def key_z(k):
    k = np.asarray(k, np.int64)
    return np.where(k >= 0, k, k ^ 0x7FFFFFFF).astype(np.int32).view(np.float32)


def owners(r):
    ids = np.full(len(r["xyz"]), -2, np.int64)
    for k, tid in enumerate(r["track_id"]):
        f, n = int(r["first"][k]), int(r["count"][k])
        ids[f: f + n] = tid
    assert (ids >= -1).all(), "a point of the export belongs to no segment"
    return ids


class Model:
    NONE = -(1 << 40)   # "no static hit yet" in key space

    def __init__(self, mot, B, cell, W):
        self.mot, self.B, self.W = mot, B, W
        self.cell = np.float32(cell); self.inv = np.float32(1.0) / self.cell
        self.facts = dict(unowned_static=0, flagged_static=0, dynamic=0, outside=0, both_kinds=0, negative_cells=0, shifts=[[] for _ in range(B)], invalid=0)
        for b in range(B):
            self.restart(b)

    def restart(self, b):
        W = self.W
        if b == 0 and not hasattr(self, "hits"):
            self.hits = [None] * self.B; self.zk = [None] * self.B; self.seen = [None] * self.B; self.origin = [None] * self.B; self.step = [0] * self.B; self.hdr = [None] * self.B
        self.hits[b] = np.zeros((2, W, W), np.uint32); self.zk[b] = np.full((W, W), self.NONE, np.int64); self.seen[b] = np.zeros((W, W), np.int32)
        self.origin[b] = (0, 0); self.step[b] = 0
        self.hdr[b] = self.header(b, -1, 0, 0, 0)

    def header(self, b, step, ns, nd, no):
        h = np.zeros(1, self.mot.SCENE_HEADER_DTYPE)
        h["origin_i"], h["origin_j"], h["step"], h["size"], h["n_static"], h["n_dynamic"], h["n_outside"], h["cell"] = self.origin[b][0], self.origin[b][1], step, self.W, ns, nd, no, self.cell
        return h

    def fold(self, c, b):
        """one accepted mot_accumulate_scene call covered slot b: what the slot's fused step contributes"""
        W, inv = self.W, self.inv
        step = self.step[b]; self.step[b] += 1
        r = c.get_track_points(b, rest=True, frame="global")
        static_flag = c.get_tracks(b)["is_static"]
        m = c.sensor_pose(b)[1]
        with np.errstate(over="ignore", invalid="ignore"):
            a, e = np.float32(m[0, 3]) * inv, np.float32(m[1, 3]) * inv
            ok = bool(np.isfinite(a) and np.isfinite(e) and abs(a) < LIMIT and abs(e) < LIMIT)
            old = self.origin[b]
            new = (int(np.floor(a)) - W // 2, int(np.floor(e)) - W // 2) if ok else old
            self.facts["invalid"] += not ok
            # scroll: the cell at new offset (u, v) was at old offset (u + di, v + dj)
            di, dj = new[0] - old[0], new[1] - old[1]
            self.facts["shifts"][b].append((di, dj))
            hits = np.zeros_like(self.hits[b]); zk = np.full_like(self.zk[b], self.NONE); seen = np.zeros_like(self.seen[b])
            u0, u1, v0, v1 = max(0, -di), min(W, W - di), max(0, -dj), min(W, W - dj)
            if u0 < u1 and v0 < v1:
                hits[:, v0:v1, u0:u1] = self.hits[b][:, v0 + dj: v1 + dj, u0 + di: u1 + di]
                zk[v0:v1, u0:u1] = self.zk[b][v0 + dj: v1 + dj, u0 + di: u1 + di]
                seen[v0:v1, u0:u1] = self.seen[b][v0 + dj: v1 + dj, u0 + di: u1 + di]
            self.origin[b] = new
            # points
            xyz = np.ascontiguousarray(r["xyz"], np.float32).reshape(-1, 3)
            ids = owners(r)
            tx, ty = xyz[:, 0] * inv, xyz[:, 1] * inv
            take = np.isfinite(xyz).all(axis=1) & (np.abs(tx) < LIMIT) & (np.abs(ty) < LIMIT) & ok
            gi = np.where(take, np.floor(tx), 0).astype(np.int64); gj = np.where(take, np.floor(ty), 0).astype(np.int64)
            u, v = gi - new[0], gj - new[1]
            take &= (u >= 0) & (u < W) & (v >= 0) & (v < W)
        owned = ids >= 0
        flagged = np.zeros(len(ids), bool); flagged[owned] = static_flag[ids[owned]] != 0
        dyn = take & owned & ~flagged
        sta = take & ~dyn
        np.add.at(hits[0], (v[sta], u[sta]), np.uint32(1)); np.add.at(hits[1], (v[dyn], u[dyn]), np.uint32(1))
        np.maximum.at(zk, (v[sta], u[sta]), zkey(xyz[sta, 2]))
        seen[v[take], u[take]] = step + 1
        self.hits[b], self.zk[b], self.seen[b] = hits, zk, seen
        self.hdr[b] = self.header(b, step, int(sta.sum()), int(dyn.sum()), int(len(ids) - take.sum()))
        f = self.facts
        f["unowned_static"] += int((sta & ~owned).sum()); f["flagged_static"] += int((sta & flagged).sum()); f["dynamic"] += int(dyn.sum()); f["outside"] += int(len(ids) - take.sum())
        f["both_kinds"] += int(((hits[0] > 0) & (hits[1] > 0)).sum()); f["negative_cells"] += int(((gi < 0) & take).sum() + ((gj < 0) & take).sum())
        return dict(xyz=xyz, ids=ids, take=take, sta=sta, dyn=dyn, u=u, v=v)

    def cells(self, b):
        out = np.zeros((self.W, self.W), self.mot.SCENE_CELL_DTYPE)
        out["static_hits"], out["dynamic_hits"], out["last_seen"] = self.hits[b][0], self.hits[b][1], self.seen[b]
        out["max_z"] = np.where(self.hits[b][0] > 0, key_z(np.maximum(self.zk[b], -(1 << 31) + 1)), np.float32(0))
        return out


class Export:
    """sentinel-filled device blocks for mot_export_scene_grid_dev: [B][stride] cells and [B] headers, with a margin on either side"""

    def __init__(self, env, B, W, stride=None):
        self.B, self.W, self.stride = B, W, stride or W * W + 8
        self.h_cells = np.full(4 + B * self.stride * 4 + 4, -7, np.int32); self.h_hdr = np.full(B * 8 + 8, -7, np.int32)
        (self.p_cells, self.k_cells), (self.p_hdr, self.k_hdr) = env.upload(self.h_cells), env.upload(self.h_hdr)
        assert self.p_cells % 16 == 0

    def run(self, c, batch):
        c.export_scene_grid_dev(batch, self.p_cells + 16, self.stride, self.p_hdr)
        c.synchronize()
        return self.read(batch)

    def raw(self):
        return LC.download(self.k_cells, self.h_cells).copy(), LC.download(self.k_hdr, self.h_hdr).copy()

    def read(self, batch):
        cells, hdr = self.raw()
        assert (cells[:4] == -7).all() and (cells[4 + batch * self.stride * 4:] == -7).all() and (hdr[batch * 8:] == -7).all(), "the export wrote outside its blocks"
        blk = cells[4: 4 + batch * self.stride * 4].reshape(batch, self.stride, 4)
        assert (blk[:, self.W * self.W:] == -7).all(), "the export wrote between the slots' blocks"
        return [blk[b, : self.W * self.W].tobytes() for b in range(batch)], [hdr[8 * b: 8 * b + 8].tobytes() for b in range(batch)]


def check(c, m, ex, batch, what):
    cells, hdrs = ex.run(c, batch)
    for b in range(batch):
        want_c, want_h = m.cells(b), m.hdr[b]
        got_h = np.frombuffer(hdrs[b], m.mot.SCENE_HEADER_DTYPE)
        assert hdrs[b] == want_h.tobytes(), (what, "slot", b, "header (export)", got_h, want_h)
        if cells[b] != want_c.tobytes():
            got = np.frombuffer(cells[b], m.mot.SCENE_CELL_DTYPE).reshape(m.W, m.W)
            bad = np.argwhere(got != want_c)
            raise AssertionError((what, "slot", b, "cells (export)", len(bad), "differ; first (v, u)", bad[0], got[tuple(bad[0])], want_c[tuple(bad[0])]))
        g = c.get_scene_grid(b)
        assert g["header"].tobytes() == want_h.tobytes() and g["cells"].tobytes() == want_c.tobytes(), (what, "slot", b, "getter")
        assert c.get_scene_grid(b, cells=False)["header"].tobytes() == want_h.tobytes(), (what, "slot", b, "getter, header alone")


def step_and_check(env, c, m, ex, clouds, stride, f, what, ego_v=None, yaw=None, batch=None):
    keep = AC.launch(env, c, clouds, stride, f, ego_v=ego_v, yaw=yaw)
    B = batch or len(clouds)
    folds = [m.fold(c, b) for b in range(B)]
    c.accumulate_scene(B)
    check(c, m, ex, len(clouds), (what, "frame", f))
    return folds


# ------------------------------------------------------------------------------------------------------------------ scenes in the world
def sensor_from_world(env, ego_v, yaws, frames_n):
    """every stream's global -> sensor matrix at every frame, from a scout context driven with the same timestamps, speeds and yaws (the dead reckoning does not
    look at the clouds; it advances with the tracker steps of the fused calls)"""
    B = len(ego_v)
    out = np.zeros((frames_n, B, 3, 4), np.float64)
    with env.context(0, max_points=1024, max_batch=B, max_tracks_total=64) as c:
        for f in range(frames_n):
            keep = AC.launch(env, c, [CC.small_scene(0, 2)] * B, 1024, f, ego_v=ego_v, yaw=yaws[f])
            for b in range(B):
                out[f, b] = c.sensor_pose(b)[0]
    return out


def to_sensor(S, world):
    q = world.copy()
    q[:, :3] = (world[:, :3].astype(np.float64) @ S[:, :3].T + S[:, 3]).astype(np.float32)
    return q


def world_blob(rng, cx, cy, n=200, half=0.4):
    q = np.zeros((n, 4), np.float32); q[:, 0] = cx + rng.uniform(-half, half, n); q[:, 1] = cy + rng.uniform(-half, half, n); q[:, 2] = rng.uniform(-1.0, 0.3, n); return q


# ------------------------------------------------------------------------------------------------------------------ 1: standing and moving objects
def standing_and_moving(env, oracle, cell, W):
    """three blobs of 200 points (track_model_cases.moving_stream's) at (8, 5), (3, -7) and (-9, -6 - 0.3 f) IN THE WORLD; the sensor drives at ego_v x 0.1 m a frame,
    stream 2 also turns, so the first two blobs stand in the global frame whatever the sensor does: 16 frames, three streams. The coverage the case is here for is
    asserted from the model's own bookkeeping."""
    frames_n, B = 16, 3
    ego_v = [0.0, 1.0, 1.0]; yaws = [[0.0, 0.0, 0.04 * f] for f in range(frames_n)]
    S = sensor_from_world(env, ego_v, yaws, frames_n)
    rngs = [np.random.default_rng(3 + b) for b in range(B)]
    with env.context(0, max_points=2048, max_batch=B, max_tracks_total=256) as c:
        c.set_track_links(True); c.set_scene_grid(cell, W)
        m = Model(env.mot, B, cell, W); ex = Export(env, B, W)
        check(c, m, ex, B, "before the first step")
        edge = 0
        for f in range(frames_n):
            clouds = [to_sensor(S[f, b], np.concatenate([world_blob(rngs[b], 8.0, 5.0), world_blob(rngs[b], 3.0, -7.0), world_blob(rngs[b], -9.0, -6.0 - 0.3 * f)])) for b in range(B)]
            folds = step_and_check(env, c, m, ex, clouds, 2048, f, ("standing and moving", cell, W), ego_v=ego_v, yaw=yaws[f])
            for b, fo in enumerate(folds):   # a blob straddling the window's edge: one owner (or the unowned rest of frame 0) with points inside and outside
                for tid in np.unique(fo["ids"]):
                    mine = fo["ids"] == tid
                    edge += bool((mine & fo["take"]).any() and (mine & ~fo["take"]).any())
        fa = m.facts
        assert fa["unowned_static"] > 0 and fa["flagged_static"] > 0 and fa["dynamic"] > 0 and fa["both_kinds"] > 0 and fa["negative_cells"] > 0, fa
        if W * cell < 20:   # (0.25, 64): a 16 m window, the blobs 9 to 11 m out
            assert fa["outside"] > 0 and edge > 0, (fa, edge)
        static_tracks = [int(c.get_tracks(b)["is_static"].sum()) for b in range(B)]
        assert min(static_tracks) >= 1, ("no stream flagged a standing blob static", static_tracks)


# ------------------------------------------------------------------------------------------------------------------ 2: scroll
def scroll(env, oracle, cell=0.25, W=64):
    """one blob scene, per-stream speed and yaw: windows that stay, move by one cell, by several, by a fraction that sometimes rounds to a shift, by more than W
    (a full clear), backwards, sideways, diagonally and round a circle; the last stream drives out of the range a window can be placed in. Which kinds of shift
    occurred is asserted from the headers the model predicted (and the library matched byte for byte)."""
    frames_n = 10
    spec = [(0.0, lambda f: 0.0), (2.5, lambda f: 0.0), (10.0, lambda f: 0.0), (1.0, lambda f: 0.0), (200.0, lambda f: 0.0), (10.0, lambda f: np.pi),
            (10.0, lambda f: np.pi / 2), (10.0, lambda f: np.pi / 4), (10.0, lambda f: 0.5 * f), (3.0e9, lambda f: 0.0)]
    B = len(spec)
    ego_v = [s[0] for s in spec]
    with env.context(0, max_points=1024, max_batch=B, max_tracks_total=64) as c:
        c.set_track_links(True); c.set_scene_grid(cell, W)
        m = Model(env.mot, B, cell, W); ex = Export(env, B, W)
        for f in range(frames_n):
            step_and_check(env, c, m, ex, [CC.small_scene(f + b, 8) for b in range(B)], 1024, f, "scroll", ego_v=ego_v, yaw=[s[1](f) for s in spec])
        sh = m.facts["shifts"]
        later = lambda b: sh[b][1:]   # (the first step moves the window from the origin of an empty grid)
        assert all(s == (0, 0) for s in later(0)), sh[0]
        assert any(max(abs(i), abs(j)) == 1 for i, j in later(1)), sh[1]
        assert any(1 < max(abs(i), abs(j)) < W for i, j in later(2)), sh[2]
        assert any(s == (0, 0) for s in later(3)) and any(s != (0, 0) for s in later(3)), sh[3]
        assert any(max(abs(i), abs(j)) >= W for i, j in later(4)), sh[4]
        flat = [s for b in range(B - 1) for s in later(b)]
        assert any(i < 0 for i, j in flat) and any(i > 0 for i, j in flat) and any(j < 0 for i, j in flat) and any(j > 0 for i, j in flat), flat
        assert any(i != 0 and j != 0 for i, j in flat), flat
        assert m.facts["invalid"] > 0 and m.hdr[B - 1]["n_outside"][0] > 0 and m.hdr[B - 1]["n_static"][0] == 0, (m.facts["invalid"], m.hdr[B - 1])


# ------------------------------------------------------------------------------------------------------------------ 3: chunk and wave edges
def shapes(env, oracle, order_any=False):
    """elevated counts 0, 1, 63, 64, 65, the splat kernel's chunk (2048) - 1 / exact / + 1, 5000 and a full frame of 160 blobs (track_point_cases.shape_frames), three steps"""
    frames = PC.shape_frames(oracle)
    targets = [len(x) for x in frames[0]]
    assert {0, 1, 63, 64, 65, 2047, 2048, 2049} <= set(targets)
    B, W = len(targets), 64
    with env.context(0, max_points=8192, max_batch=B, max_tracks_total=512) as c:
        c.set_track_links(True); c.set_scene_grid(1.0, W)
        if order_any:
            c.set_point_order(env.mot.MOT_ORDER_ANY)
        m = Model(env.mot, B, 1.0, W); ex = Export(env, B, W)
        for f in range(3):
            sent = [np.ascontiguousarray(x[np.random.default_rng(7 + b).permutation(len(x))]) for b, x in enumerate(frames[f])] if order_any else frames[f]
            step_and_check(env, c, m, ex, sent, 8192, f, ("shapes", order_any))
        assert [len(c.get_point_tracks(b)) for b in range(B)] == targets
        assert [int(m.hdr[b]["n_static"][0]) + int(m.hdr[b]["n_dynamic"][0]) + int(m.hdr[b]["n_outside"][0]) for b in range(B)] == targets
        assert m.facts["dynamic"] > 0 and m.facts["unowned_static"] > 0 and m.facts["outside"] > 0, m.facts


# ------------------------------------------------------------------------------------------------------------------ 4: contention
def contention(env, oracle):
    """cell 10: every point of a frame lands in one cell (stream 0) or two (stream 1); counts exact, max_z the maximum"""
    W = 64
    rng = np.random.default_rng(21)
    S = sensor_from_world(env, [0.0, 0.0], [[0.0, 0.0]] * 4, 4)   # (the blobs are placed in the global frame: its axes are not the sensor's)
    with env.context(0, max_points=2048, max_batch=2, max_tracks_total=64) as c:
        c.set_track_links(True); c.set_scene_grid(10.0, W)
        m = Model(env.mot, 2, 10.0, W); ex = Export(env, 2, W)
        total = [0, 0]
        for f in range(4):
            one = np.concatenate([world_blob(rng, 3.0, 4.0, 400), world_blob(rng, 7.0, 6.0, 400), world_blob(rng, 5.0, 2.0, 300)])
            two = np.concatenate([world_blob(rng, 3.0, 4.0, 500), world_blob(rng, 13.0, 6.0, 500)])
            folds = step_and_check(env, c, m, ex, [to_sensor(S[f, 0], one), to_sensor(S[f, 1], two)], 2048, f, "contention", ego_v=[0.0, 0.0])
            for b, cells_n in ((0, 1), (1, 2)):
                g = c.get_scene_grid(b)["cells"]
                hit = np.argwhere((g["static_hits"] > 0) | (g["dynamic_hits"] > 0))
                assert len(hit) == cells_n, (f, b, hit)
                fo = folds[b]
                total[b] += len(fo["ids"])   # (the sensor stands: nothing scrolls out)
                assert len(fo["ids"]) > 0 and fo["take"].all() and int(g["static_hits"].sum()) + int(g["dynamic_hits"].sum()) == total[b], (f, b)
                for v, u in hit:
                    here = fo["sta"] & (fo["u"] == u) & (fo["v"] == v)
                    if f == 0 and here.any():
                        assert g["max_z"][v, u] == fo["xyz"][here, 2].max() and g["static_hits"][v, u] == here.sum(), (f, b, v, u)
        assert m.facts["dynamic"] > 0 and m.facts["unowned_static"] > 0, m.facts


# ------------------------------------------------------------------------------------------------------------------ 5: contract
def code_of(env, fn):
    return AC.code_of(env, fn)


def grids(c, B):
    return [(g["header"].tobytes(), g["cells"].tobytes()) for g in (c.get_scene_grid(b) for b in range(B))]


def contract_modes(env, oracle):
    """the setter's arguments and states, links, readers' arguments with sentinel blocks, twice per step, a taken slot, a smaller batch, geometry change, off-then-on, sequence slots"""
    E = env.mot
    W = 64
    clouds = [[CC.small_scene(f, 20), CC.small_scene(f + 5, 12)] for f in range(8)]
    with env.context(0, max_points=4096, max_batch=2, max_tracks_total=64) as c:
        ex = Export(env, 2, W)
        sentinel = ex.raw()
        def untouched(what):
            now = ex.raw()
            assert (now[0] == sentinel[0]).all() and (now[1] == sentinel[1]).all(), (what, "a refused call wrote into the caller's blocks")
        # links off: the setter refuses; feature off: the other three refuse
        assert code_of(env, lambda: c.set_scene_grid(1.0, W)) == E.MOT_E_STATE
        c.set_track_links(True)
        keep = AC.launch(env, c, clouds[0], 4096, 0)
        n = C.c_int(-7); hdr = np.full(8, -7, np.int32); small = np.full(W * W * 4, -7, np.int32)
        for what, fn in (("accumulate", lambda: c.accumulate_scene(2)), ("export", lambda: c.export_scene_grid_dev(2, ex.p_cells + 16, ex.stride, ex.p_hdr)),
                         ("getter", lambda: c.get_scene_grid(0))):
            assert code_of(env, fn) == E.MOT_E_STATE, what
        untouched("feature off")
        c.set_scene_grid(None)   # off while off
        for cell, size in ((0.049, 64), (10.5, 64), (float("nan"), 64), (float("inf"), 64), (-1.0, 64), (0.0, 64), (0.5, 63), (0.5, 96), (0.5, 32), (0.5, 4096), (0.5, 0), (0.5, -64)):
            assert code_of(env, lambda: c.set_scene_grid(cell, size)) == E.MOT_E_ARG, (cell, size)
        assert code_of(env, lambda: c.get_scene_grid(0)) == E.MOT_E_STATE, "a refused setter turned the feature on"
        c.set_scene_grid(1.0, W)
        assert code_of(env, lambda: c.set_track_links(False)) == E.MOT_E_STATE, "links off while the grid is on"
        m = Model(E, 2, 1.0, W)
        check(c, m, ex, 2, "empty, step -1")
        # the step the slots hold was taken before the feature was on
        assert code_of(env, lambda: c.accumulate_scene(2)) == E.MOT_E_STATE
        good = lambda f, **kw: step_and_check(env, c, m, ex, clouds[f], 4096, f, "contract", **kw)
        def refused_unchanged(fn, code, what):
            before = grids(c, 2)
            assert code_of(env, fn) == code, what
            assert grids(c, 2) == before, (what, "a refused call changed a grid")
        good(1); good(2)
        c.set_scene_grid(1.0, W)   # the same geometry again changes nothing
        check(c, m, ex, 2, "the same geometry again")
        refused_unchanged(lambda: c.accumulate_scene(2), E.MOT_E_STATE, "a second call for the same step")
        refused_unchanged(lambda: c.accumulate_scene(1), E.MOT_E_STATE, "a second call for the same step, slot 0 alone")
        refused_unchanged(lambda: c.accumulate_scene(0), E.MOT_E_ARG, "batch 0")
        refused_unchanged(lambda: c.accumulate_scene(3), E.MOT_E_ARG, "batch 3")
        # the readers' arguments: sentinel blocks stay as they are
        ex = Export(env, 2, W); sentinel = ex.raw()
        for what, fn in (("stride below W^2", lambda: c.export_scene_grid_dev(2, ex.p_cells + 16, W * W - 1, ex.p_hdr)), ("null cells", lambda: c.export_scene_grid_dev(2, 0, ex.stride, ex.p_hdr)),
                         ("null headers", lambda: c.export_scene_grid_dev(2, ex.p_cells + 16, ex.stride, 0)), ("cells off 16 bytes", lambda: c.export_scene_grid_dev(2, ex.p_cells + 8, ex.stride, ex.p_hdr)),
                         ("batch 0", lambda: c.export_scene_grid_dev(0, ex.p_cells + 16, ex.stride, ex.p_hdr)), ("batch 3", lambda: c.export_scene_grid_dev(3, ex.p_cells + 16, ex.stride, ex.p_hdr))):
            assert code_of(env, fn) == E.MOT_E_ARG, what
            c.synchronize(); untouched(what)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        assert c.lib.mot_get_scene_grid(c._h, 2, None, 0, C.byref(n), vp(hdr)) == E.MOT_E_ARG and c.lib.mot_get_scene_grid(c._h, -1, None, 0, C.byref(n), vp(hdr)) == E.MOT_E_ARG
        assert c.lib.mot_get_scene_grid(c._h, 0, None, 0, None, vp(hdr)) == E.MOT_E_ARG and c.lib.mot_get_scene_grid(c._h, 0, vp(small), -1, C.byref(n), vp(hdr)) == E.MOT_E_ARG
        assert n.value == -7 and (hdr == -7).all()
        assert c.lib.mot_get_scene_grid(c._h, 0, vp(small), W * W - 1, C.byref(n), vp(hdr)) == E.MOT_E_CAPACITY and n.value == W * W and (small == -7).all() and (hdr == -7).all()
        assert c.lib.mot_get_scene_grid(c._h, 0, None, 0, C.byref(n), vp(hdr)) == 0 and hdr.tobytes() == m.hdr[0].tobytes(), "null cells: the header alone"
        # a batch smaller than max_batch leaves the other slot's grid as it is
        keep = AC.launch(env, c, clouds[3], 4096, 3)
        other = grids(c, 2)[1]
        m.fold(c, 0); c.accumulate_scene(1)
        assert grids(c, 2)[1] == other
        check(c, m, ex, 2, "slot 0 alone")
        refused_unchanged(lambda: c.accumulate_scene(2), E.MOT_E_STATE, "a batch that holds a slot already taken")
        # a stage-wise call takes slot 0
        keep = AC.launch(env, c, clouds[4], 4096, 4)
        elev = c.get_ground(0, n_hint=len(clouds[4][0]))["elevated"]
        c.cluster(elev)
        refused_unchanged(lambda: c.accumulate_scene(2), E.MOT_E_STATE, "a batch that includes a taken slot")
        refused_unchanged(lambda: c.accumulate_scene(1), E.MOT_E_STATE, "the taken slot alone")
        good(5)
        assert [int(m.hdr[b]["step"][0]) for b in (0, 1)] == [3, 2], "the refused calls counted a step"
        # another geometry: empty grids, steps from 0; off then on likewise
        c.set_scene_grid(0.5, 128)
        m = Model(E, 2, 0.5, 128); ex = Export(env, 2, 128)
        check(c, m, ex, 2, "another geometry")
        assert code_of(env, lambda: c.accumulate_scene(2)) == E.MOT_E_STATE, "the step the slots hold was taken with the old geometry"
        step_and_check(env, c, m, ex, clouds[6], 4096, 6, "another geometry")
        c.set_scene_grid(None)
        assert code_of(env, lambda: c.get_scene_grid(0)) == E.MOT_E_STATE
        c.set_track_links(False); c.set_track_links(True)   # (allowed again while the feature is off)
        c.set_scene_grid(0.5, 128)
        m = Model(E, 2, 0.5, 128)
        check(c, m, ex, 2, "off then on")
        folds = step_and_check(env, c, m, ex, clouds[7], 4096, 7, "off then on")
        assert all(int(m.hdr[b]["step"][0]) == 0 for b in (0, 1)) and all(fo["take"].any() for fo in folds) and m.facts["dynamic"] > 0
    # sequence mode
    with env.context(0, max_points=4096, max_batch=2, max_tracks_total=64) as c:
        c.set_track_links(True); c.set_scene_grid(1.0, W)
        host = np.zeros((2, 4096, 4), np.float32)
        for f in range(2):
            host[f, : len(clouds[f][0])] = clouds[f][0]
        ptr, keep = env.upload(host)
        c.sequence_dev(ptr, 4096 * 4, [len(clouds[f][0]) for f in range(2)], [2.0e8, 2.001e8], [1.0] * 2, [0.0] * 2)
        before = grids(c, 2)
        assert code_of(env, lambda: c.accumulate_scene(2)) == E.MOT_E_STATE and code_of(env, lambda: c.accumulate_scene(1)) == E.MOT_E_STATE
        assert grids(c, 2) == before


def contract_resets(env, oracle):
    """reset_slot, reset_tracks_slot, stream_load and reset empty the grids of the slots they touch and restart their steps; the other slots keep theirs"""
    E = env.mot
    B, W = 3, 64
    clouds = [[CC.small_scene(f + 3 * b, 12) for b in range(B)] for f in range(12)]
    with env.context(0, max_points=4096, max_batch=B, max_tracks_total=64) as c:
        c.set_track_links(True); c.set_scene_grid(1.0, W)
        m = Model(E, B, 1.0, W); ex = Export(env, B, W)
        f = 0
        def good():
            nonlocal f
            step_and_check(env, c, m, ex, clouds[f], 4096, f, "resets")
            f += 1
        good(); good()
        blob = c.stream_save(2)
        for what, fn in (("reset_slot", lambda: c.reset_slot(1)), ("reset_tracks_slot", lambda: c.reset_tracks_slot(1)), ("stream_load", lambda: c.stream_load(1, blob))):
            keep = AC.launch(env, c, clouds[f], 4096, f); f += 1   # a step that is not yet taken when the slot is reset
            others = [grids(c, B)[b] for b in (0, 2)]
            fn()
            m.restart(1)
            check(c, m, ex, B, (what, "the touched slot is empty, the others as they were"))
            assert [grids(c, B)[b] for b in (0, 2)] == others, what
            assert code_of(env, lambda: c.accumulate_scene(B)) == E.MOT_E_STATE, (what, "the step the reset slot holds is out of reach")
            m.fold(c, 0); c.accumulate_scene(1)   # (slot 0 alone is still whole — and now one step ahead of slot 2)
            check(c, m, ex, B, (what, "slot 0 alone"))
            good()
            assert int(m.hdr[1]["step"][0]) == 0 and int(m.hdr[0]["step"][0]) > int(m.hdr[2]["step"][0]) > 0, what
        c.reset()
        for b in range(B):
            m.restart(b)
        check(c, m, ex, B, "reset")
        assert code_of(env, lambda: c.accumulate_scene(B)) == E.MOT_E_STATE
        good()
        assert all(int(m.hdr[b]["step"][0]) == 0 for b in range(B)) and m.facts["dynamic"] > 0 and m.facts["unowned_static"] > 0, m.facts


# ------------------------------------------------------------------------------------------------------------------ 6: non-interference
KERNELS = (b"scene_scroll_kernel", b"scene_splat_kernel", b"scene_export_kernel", b"scene_reset_kernel")


def non_interference(env, oracle, order_any=False, graphs=False):
    """everything a caller could read before the feature existed — the fused outputs and snapshots (track_point_cases.readout), the accumulators' rows and the raw
    track models — is byte-identical in a context that keeps a scene grid (before or after the accumulators' call, by turns) and one that never turns it on"""
    clouds = [[CC.small_scene(f, 20), CC.small_scene(f + 5, 12)] for f in range(4)]
    if order_any:
        clouds = [[np.ascontiguousarray(x[np.random.default_rng(11 + b).permutation(len(x))]) for b, x in enumerate(fr)] for fr in clouds]
    res = {}
    for tag in ("never", "grid"):
        with env.context(0, max_points=4096, max_batch=2, max_tracks_total=256) as c:
            c.set_launch_graphs(graphs); c.set_track_links(True); c.set_track_accumulation(256, 4)
            if order_any:
                c.set_point_order(env.mot.MOT_ORDER_ANY)
            if tag == "grid":
                c.set_scene_grid(1.0, 64)
            out = []
            for f in range(4):
                keep = PC.launch(env, c, clouds[f], 4096, f, yaw=0.02 * f)
                n_points = [len(x) for x in clouds[f]]
                before = PC.readout(c, 2, n_points)
                if tag == "grid" and f % 2 == 0:
                    c.accumulate_scene(2)
                c.accumulate_track_points(2)
                if tag == "grid" and f % 2 == 1:
                    c.accumulate_scene(2)
                if tag == "grid":
                    PC.equal_readouts(PC.readout(c, 2, n_points), before, (f, "after the scene call"))   # (one context: every byte, the undefined ones included)
                    assert int(c.get_scene_grid(1, cells=False)["header"]["step"]) == f
                models = [(k + str(b), np.ascontiguousarray(v).tobytes()) for b in (0, 1) for k, v in sorted(c.get_track_models(b).items())]
                rows = [("rows" + str(b), c.get_accum_rows(b).tobytes()) for b in (0, 1)]
                out.append(AC.defined_items(before) + rows + models)
            res[tag] = out
    for f in range(4):
        PC.equal_readouts(res["grid"][f], res["never"][f], (f, "against a context that never kept a grid"))


# ------------------------------------------------------------------------------------------------------------------ 7: determinism
def run_script(env, c, frames_n=5):
    B, W = 3, 64
    c.set_track_links(True); c.set_scene_grid(1.0, W)
    ex = Export(env, B, W)
    out = []
    for f in range(frames_n):
        keep = AC.launch(env, c, [CC.small_scene(f + 2 * b, 16) for b in range(B)], 2048, f, ego_v=[0.0, 3.0, 8.0], yaw=[0.0, 0.1 * f, -0.2 * f])
        c.accumulate_scene(B)
        first = ex.run(c, B)
        assert ex.run(c, B) == first, (f, "two exports of one state differ")
        out.append(first)
    return out


def determinism(env, oracle, other_lib_path=None):
    """the same steps in two contexts give byte-identical exports; exporting twice gives identical bytes. other_lib_path (emulator): the second context runs a variant
    build of the kernels (the plain form of the splat kernel, without run merging)"""
    runs = []
    for k in range(2):
        e = env if (k == 0 or other_lib_path is None) else CC.Env(env.mot, other_lib_path, env.upload)
        with e.context(0, max_points=2048, max_batch=3, max_tracks_total=64) as c:
            runs.append(run_script(e, c))
    assert runs[0] == runs[1]
    assert any(np.frombuffer(h, env.mot.SCENE_HEADER_DTYPE)["n_dynamic"][0] > 0 for h in runs[0][-1][1])


# ------------------------------------------------------------------------------------------------------------------ 8: emulator only
def launches_only_in_the_new_calls(env, oracle):
    """emulator: the launch counters of the new kernels move in the new calls and nowhere else; nothing is allocated before the setter; the live allocations return
    to their base after off and after mot_destroy"""
    lib = env.mot.load_library(env.lib_path)
    lib.hipemu_live_allocs.restype = C.c_long
    count = lambda: [lib.hipemu_launch_count(k) for k in KERNELS]
    base = lib.hipemu_live_allocs()
    with env.context(0, max_points=4096, max_batch=2, max_tracks_total=64) as c:
        before = count()
        c.set_track_links(True)
        keep = PC.launch(env, c, [CC.small_scene(0, 20), CC.small_scene(5, 12)], 4096, 0)
        c.get_track_points(1, frame="global"); c.sensor_pose(0)
        allocs = lib.hipemu_live_allocs()
        for fn in (lambda: c.accumulate_scene(2), lambda: c.get_scene_grid(0), lambda: c.set_scene_grid(1.0, 63)):
            assert code_of(env, fn) != 0
        c.set_scene_grid(None)
        assert lib.hipemu_live_allocs() == allocs and count() == before, "the feature allocated or launched while it was off"
        c.set_scene_grid(1.0, 64)
        assert lib.hipemu_live_allocs() == allocs + 5   # cells, headers, origins, arguments, the ring of page-locked blocks
        assert count() == [before[0], before[1], before[2], before[3] + 1]   # (the setter empties the grids)
        ex = Export(env, 2, 64)
        for f in range(1, 4):
            keep = PC.launch(env, c, [CC.small_scene(f, 20), CC.small_scene(f + 5, 12)], 4096, f)
            for b in (0, 1):
                c.get_point_tracks(b); c.get_box_tracks(b); c.get_boxes(b); c.get_tracks(b); c.get_track_points(b, frame="global")
            assert count() == [before[0], before[1], before[2], before[3] + 1], f
        c.accumulate_scene(2)
        assert count() == [before[0] + 1, before[1] + 1, before[2], before[3] + 1]
        ex.run(c, 2)
        assert count() == [before[0] + 1, before[1] + 1, before[2] + 1, before[3] + 1]
        c.get_scene_grid(1, cells=False)
        assert count()[2] == before[2] + 1, "the header alone needs no kernel"
        c.get_scene_grid(1)
        assert count()[2] == before[2] + 2 and lib.hipemu_live_allocs() == allocs + 6   # (the getter's staging block)
        c.reset_slot(0); c.reset()
        assert count() == [before[0] + 1, before[1] + 1, before[2] + 2, before[3] + 3]
        assert code_of(env, lambda: c.accumulate_scene(2)) == env.mot.MOT_E_STATE
        c.set_scene_grid(None)
        assert lib.hipemu_live_allocs() == allocs, "turning the feature off did not free its memory"
        c.set_scene_grid(1.0, 64)
    assert lib.hipemu_live_allocs() == base, "mot_destroy left allocations of the feature behind"


def setter_under_allocation_failure(env, oracle):
    """emulator: each of the setter's allocations (four device blocks, the ring's page-locked block, its 16 events) failing in turn -> MOT_E_HIP, the mode stays as
    it was (off, or the earlier geometry with its grids), no memory is leaked"""
    lib = env.mot.load_library(env.lib_path)
    lib.hipemu_live_allocs.restype = C.c_long
    lib.hipemu_fail_alloc_at.argtypes = [C.c_long]; lib.hipemu_fail_alloc_at.restype = None
    E = env.mot
    try:
        with env.context(0, max_points=4096, max_batch=2, max_tracks_total=64) as c:
            c.set_track_links(True)
            allocs = lib.hipemu_live_allocs()
            for k in range(1, 23):   # 5 allocations; then the ring's 16 events, which stay in the context's registry once created: a later attempt skips them
                lib.hipemu_fail_alloc_at(k)
                rc = code_of(env, lambda: c.set_scene_grid(1.0, 64))
                lib.hipemu_fail_alloc_at(0)
                if rc == 0:
                    break
                assert rc == E.MOT_E_HIP and lib.hipemu_live_allocs() == allocs and code_of(env, lambda: c.get_scene_grid(0)) == E.MOT_E_STATE, k
            assert 6 < k < 22, k   # (every memory allocation was met, and the attempts came to an end)
            c.set_scene_grid(None)
            assert lib.hipemu_live_allocs() == allocs
            c.set_scene_grid(1.0, 64)
            m = Model(E, 2, 1.0, 64); ex = Export(env, 2, 64)
            step_and_check(env, c, m, ex, [CC.small_scene(0, 20), CC.small_scene(5, 12)], 4096, 0, "before the failed change of geometry")
            allocs = lib.hipemu_live_allocs()
            for k in (1, 2, 3, 4):   # (the ring exists: four allocations)
                lib.hipemu_fail_alloc_at(k)
                assert code_of(env, lambda: c.set_scene_grid(0.5, 128)) == E.MOT_E_HIP, k
                lib.hipemu_fail_alloc_at(0)
                assert lib.hipemu_live_allocs() == allocs, k
                check(c, m, ex, 2, ("the earlier geometry is whole", k))
            step_and_check(env, c, m, ex, [CC.small_scene(1, 20), CC.small_scene(6, 12)], 4096, 1, "after the failed change of geometry")
    finally:
        lib.hipemu_fail_alloc_at(0)
