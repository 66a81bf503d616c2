"""Per-track point clouds (mot_export_track_points_dev / mot_get_track_points, csrc/track_points.hip): bodies shared by tests/test_emu_track_points.py
(emulator) and tests/test_track_points_gpu.py (MI355X). The callers supply a capacity_cases.Env.

Every expectation is a numpy composition of getters that existed before the feature — get_point_tracks, get_box_tracks, get_ground, sensor_pose — so the
oracle shares no code with the kernels under test: the distinct owners of the row, a stable argsort of the points by the rank of their id, the segment table
from the counts. All comparisons are exact (bytes); there is no tolerance anywhere."""
import ctypes as C

import numpy as np

import capacity_cases as CC
import track_link_cases as LC

MAX_SEG = 1025   # a frame's distinct owners and the rest segment


# ------------------------------------------------------------------------------------------------------------------ the composition
def want_partition(c, b, rest, matrix=None):
    """what the feature must deliver for slot b, from the getters that exist without it"""
    ids = c.get_point_tracks(b); bt = c.get_box_tracks(b)
    elev = c.get_ground(b)["elevated"][:, :3]
    assert len(elev) == len(ids)
    return compose(ids, bt, elev, rest, matrix)


def compose(ids, bt, elev, rest, matrix=None):
    owners = np.unique(bt[bt >= 0])
    R = len(owners)
    key = np.full(len(ids), R, np.int64)
    has = ids >= 0
    key[has] = np.searchsorted(owners, ids[has])
    assert (key[has] < R).all() and np.array_equal(owners[key[has]], ids[has]), "a point carries an id the owner row does not hold"
    order = np.argsort(key, kind="stable")
    if not rest:
        order = order[key[order] < R]
    counts = np.bincount(key, minlength=R + 1)
    nseg = R + (1 if rest else 0)
    xyz = np.ascontiguousarray(elev[order], np.float32)
    if matrix is not None:   # fp32, left to right (include/mot.h, mot_sensor_pose)
        m = np.asarray(matrix, np.float32).reshape(3, 4)
        x, y, z = xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy()
        xyz = np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)], -1).astype(np.float32)
    return dict(index=order.astype(np.int32), xyz=xyz,
                track_id=np.concatenate([owners, [-1]]).astype(np.int32)[:nseg],
                first=np.concatenate([[0], np.cumsum(counts)])[:nseg].astype(np.int32),
                count=counts[:nseg].astype(np.int32),
                n_boxes=np.array([(bt == o).sum() for o in owners] + [0], np.int32)[:nseg])


def same(got, want, what, points=None, segments=None):
    """bytes; points / segments: only that many leading records are compared (truncated exports)"""
    np_, ns = (len(want["index"]) if points is None else points), (len(want["track_id"]) if segments is None else segments)
    for k in ("track_id", "first", "count", "n_boxes"):
        assert np.array_equal(np.asarray(got[k])[:ns], want[k][:ns]), (what, k, np.asarray(got[k])[:8], want[k][:8])
    assert np.array_equal(np.asarray(got["index"])[:np_], want["index"][:np_]), (what, "index")
    assert np.array_equal(np.ascontiguousarray(got["xyz"], np.float32)[:np_].view(np.uint32), want["xyz"][:np_].view(np.uint32)), (what, "xyz bits")


def segments_well_formed(r, what):
    """back to back from 0, ids ascending (the rest last), index ascending inside every segment"""
    ids = r["track_id"]
    own = ids[ids >= 0]
    assert (np.diff(own) > 0).all() and (ids[: len(own)] >= 0).all(), (what, ids)
    assert np.array_equal(r["first"], np.concatenate([[0], np.cumsum(r["count"])])[: len(ids)]), (what, "not back to back")
    assert int(r["count"].sum()) == len(r["index"]), what
    for f, n in zip(r["first"], r["count"]):
        assert (np.diff(r["index"][f:f + n]) > 0).all(), (what, "index not ascending inside a segment")


class DevBlocks:
    """caller-owned device blocks for one export, filled with the sentinel -7; misalign: both record blocks start 4 bytes off a 16-byte boundary"""

    def __init__(self, env, B, stride, max_seg, misalign=False):
        self.B, self.stride, self.max_seg, self.off = B, stride, max_seg, (1 if misalign else 0)
        self.h_pts = np.full(B * stride * 4 + 4, -7, np.int32); self.h_seg = np.full(B * max_seg * 4 + 4, -7, np.int32); self.h_cnt = np.full(2 * B + 2, -7, np.int32)
        (self.p_pts, self.k_pts), (self.p_seg, self.k_seg), (self.p_cnt, self.k_cnt) = env.upload(self.h_pts), env.upload(self.h_seg), env.upload(self.h_cnt)

    def run(self, c, batch, rest, frame):
        c.export_track_points_dev(batch, self.p_pts + 4 * self.off, self.stride, self.p_seg + 4 * self.off, self.max_seg, self.p_cnt, rest=rest, frame=frame)
        c.synchronize()
        return self.read()

    def read(self):
        pts = LC.download(self.k_pts, self.h_pts); seg = LC.download(self.k_seg, self.h_seg); cnt = LC.download(self.k_cnt, self.h_cnt)
        self.raw = (pts, seg, cnt)
        assert (pts[: self.off] == -7).all() and (seg[: self.off] == -7).all() and (cnt[2 * self.B:] == -7).all()
        assert (pts[self.off + self.B * self.stride * 4:] == -7).all() and (seg[self.off + self.B * self.max_seg * 4:] == -7).all()
        p = pts[self.off: self.off + self.B * self.stride * 4].reshape(self.B, self.stride, 4)
        s = seg[self.off: self.off + self.B * self.max_seg * 4].reshape(self.B, self.max_seg, 4)
        return p, s, cnt[: 2 * self.B].reshape(self.B, 2)


def check_block(p, s, cnt, b, want, what):
    """slot b of an export's blocks against the composition: the true counts, the records that fit, the sentinel behind them"""
    n, ns = len(want["index"]), len(want["track_id"])
    assert tuple(cnt[b]) == (ns, n), (what, "counts", tuple(cnt[b]), (ns, n))
    wn, wns = min(n, p.shape[1]), min(ns, s.shape[1])
    got = dict(xyz=np.ascontiguousarray(p[b, :wn, :3]).view(np.float32), index=p[b, :wn, 3],
               track_id=s[b, :wns, 0], first=s[b, :wns, 1], count=s[b, :wns, 2], n_boxes=s[b, :wns, 3])
    same(got, want, what, points=wn, segments=wns)
    assert (p[b, wn:] == -7).all() and (s[b, wns:] == -7).all(), (what, "written beyond the slot's records")


# ------------------------------------------------------------------------------------------------------------------ inputs
_FRAMES = {}


def shape_frames(oracle):
    """three frames of ten streams: exactly NE_SHAPES elevated points each, and the whole of link_frame_source (7 719 points, 160 box-sized blobs) in the last"""
    if "shapes" not in _FRAMES:
        p = oracle.params(0)
        full = len(LC.link_frame_source(0))
        _FRAMES["shapes"] = [[LC.frame_with_elevated(oracle, p, t, seed=s) for t in LC.NE_SHAPES + (full,)] for s in range(3)]
    return _FRAMES["shapes"]


def launch(env, c, clouds, stride, f, ego_v=1.0, yaw=0.0):
    host = np.zeros((len(clouds), stride, 4), np.float32)
    for b, x in enumerate(clouds):
        host[b, : len(x)] = x
    ptr, keep = env.upload(host)
    c.frames_dev(ptr, stride * 4, [len(x) for x in clouds], run_tracker=True, timestamps=[2.0e8 + f * 1e5] * len(clouds), ego_v=[ego_v] * len(clouds), ego_yaw=[yaw] * len(clouds))
    return keep


# ------------------------------------------------------------------------------------------------------------------ 1, 2: shapes, many segments
def shapes(env, oracle, order_any=False, max_points=8192):
    """-> per frame and slot the getter's result with the flag. Host getter and device export (a 16-byte-aligned block and one 4 bytes off), with and without the rest
    segment, against the composition; sentinels and true counts"""
    frames = shape_frames(oracle)
    targets = [len(x) for x in frames[0]]
    B = len(targets)
    out = []
    with env.context(0, max_points=max_points, max_batch=B, max_tracks_total=512) as c:
        c.set_track_links(True)
        if order_any:
            c.set_point_order(env.mot.MOT_ORDER_ANY)
        for f in range(3):
            perms = [np.random.default_rng(7 + b).permutation(len(x)) for b, x in enumerate(frames[f])]
            sent = [np.ascontiguousarray(x[q]) for x, q in zip(frames[f], perms)] if order_any else frames[f]
            keep = launch(env, c, sent, max_points, f)
            want = {rest: [want_partition(c, b, rest) for b in range(B)] for rest in (False, True)}
            got = []
            for b in range(B):
                for rest in (False, True):
                    r = c.get_track_points(b, rest=rest)
                    same(r, want[rest][b], (f, targets[b], rest, "getter"))
                    segments_well_formed(r, (f, targets[b], rest))
                assert len(r["index"]) == targets[b] and np.array_equal(np.sort(r["index"]), np.arange(targets[b])), (f, targets[b], "with the rest every point occurs once")
                r["perm"] = perms[b]; got.append(r)
            stride = max(targets) + 3
            for rest in (False, True):
                for misalign in (False, True):
                    p, s, cnt = DevBlocks(env, B, stride, MAX_SEG, misalign).run(c, B, rest, "sensor")
                    for b in range(B):
                        check_block(p, s, cnt, b, want[rest][b], (f, targets[b], rest, misalign, "export"))
            out.append(got)
            if f == 2:   # the last slot: more owners than a wave has lanes, and than one 6-bit digit holds
                owners = got[B - 1]["track_id"]
                assert (owners >= 0).sum() >= 65, ("frame 2 of the longest prefix has too few distinct owners", (owners >= 0).sum())
                assert (got[B - 1]["count"][:-1] > 0).sum() >= 65
    return out


def order_any(env, oracle):
    """MOT_ORDER_ANY on shuffled copies of the same frames: the composition in that mode (inside shapes), and against SCAN under the permutation — the same
    segment table and the same set of points per segment"""
    scan = shapes(env, oracle)
    anyo = shapes(env, oracle, order_any=True)
    for f in range(3):
        for b in range(len(scan[f])):
            a, s = anyo[f][b], scan[f][b]
            for k in ("track_id", "first", "count", "n_boxes"):
                assert np.array_equal(a[k], s[k]), (f, b, k)
            q = a["perm"]   # sent[i] = cloud[q[i]]: point `index` of the shuffled frame is point q[index] of the SCAN frame
            for first, n in zip(a["first"], a["count"]):
                mine = q[a["index"][first:first + n]]; by_scan = np.argsort(mine)
                assert np.array_equal(mine[by_scan], s["index"][first:first + n]), (f, b, "another set of points in a segment")
                assert np.array_equal(a["xyz"][first:first + n][by_scan].view(np.uint32), s["xyz"][first:first + n].view(np.uint32)), (f, b, "xyz")


# ------------------------------------------------------------------------------------------------------------------ 3: one track, several boxes
def split_stream(frames=9):
    """a blob of 96 points stands still until its track is established, then splits into two blobs of 48 points 1.2 m apart (two clusters: two free cells between
    them), both inside the track's gate; the two blobs' points are INTERLEAVED in the input. A second blob far away keeps the seed box (the first frame's box 0) busy."""
    rng = np.random.default_rng(5)
    def blob(cx, cy, n):
        q = np.zeros((n, 4), np.float32); q[:, 0] = cx + rng.uniform(-0.25, 0.25, n); q[:, 1] = cy + rng.uniform(-0.25, 0.25, n); q[:, 2] = rng.uniform(-1.0, 0.3, n); return q
    ctr = CC.cell_centres(CC.lattice_cells(250, 6, 3), 250, 50.0)
    far, a, b = ctr[0], ctr[900], ctr[901]   # a, b: neighbours on the blob lattice (1.2 m apart)
    assert abs(np.hypot(*(a - b)) - 1.2) < 1e-9
    mid = (a + b) / 2
    out = []
    for f in range(frames):
        if f < 6:
            out.append(np.concatenate([blob(far[0], far[1], 48), blob(a[0], a[1], 96)]))
        else:
            two = np.empty((96, 4), np.float32); two[0::2] = blob(a[0], a[1], 48); two[1::2] = blob(b[0], b[1], 48)
            out.append(np.concatenate([blob(far[0], far[1], 48), two]))
    return out, mid


def one_track_two_boxes(env, oracle):
    frames, _ = split_stream()
    seen = 0
    with env.context(0, max_points=2048, max_batch=1, max_tracks_total=256) as c:
        c.set_track_links(True)
        for f, x in enumerate(frames):
            keep = launch(env, c, [x], 2048, f, ego_v=0.0)
            r = c.get_track_points(0, rest=True)
            same(r, want_partition(c, 0, True), (f, "getter"))
            segments_well_formed(r, f)
            lab = c.get_clusters(0, n_elevated=max(len(c.get_point_tracks(0)), 1))["point_label"]
            for k in np.nonzero(r["n_boxes"] >= 2)[0]:
                idx = r["index"][r["first"][k]: r["first"][k] + r["count"][k]]
                clusters = np.unique(lab[idx])
                assert len(clusters) >= 2 and (np.diff(idx) > 0).all(), (f, k, clusters)
                assert (np.diff(lab[idx]) != 0).sum() > 4, (f, "the two clusters' points are not interleaved in the segment")
                seen += 1
    assert seen >= 1, "no track ever owned two boxes: the stream's geometry no longer splits a blob inside its track's gate"


# ------------------------------------------------------------------------------------------------------------------ 5: global frame
def global_frame(env, oracle):
    """ego_v = 1, a yaw that changes per frame: MOT_FRAME_GLOBAL = the elevated points under global_from_sensor of sensor_pose read right after the fused call, in
    numpy fp32 left to right, bit for bit; index and segments as in the sensor frame"""
    frames = shape_frames(oracle)
    pick = [4, 7, 9]   # 65, 2049 and 7 719 points
    B = len(pick)
    with env.context(0, max_points=8192, max_batch=B, max_tracks_total=512) as c:
        c.set_track_links(True)
        for f in range(3):
            keep = launch(env, c, [frames[f][k] for k in pick], 8192, f, ego_v=1.0, yaw=0.05 * f)
            mats = [c.sensor_pose(b)[1] for b in range(B)]
            if f > 0:
                assert abs(mats[0][0, 1]) > 1e-3 and abs(mats[0][0, 3]) + abs(mats[0][1, 3]) > 1e-3, "the matrix is no real rotation plus translation"
            for rest in (False, True):
                wg = [want_partition(c, b, rest, mats[b]) for b in range(B)]
                ws = [want_partition(c, b, rest) for b in range(B)]
                for b in range(B):
                    g, s = c.get_track_points(b, rest=rest, frame="global"), c.get_track_points(b, rest=rest, frame="sensor")
                    same(g, wg[b], (f, b, rest, "global getter")); same(s, ws[b], (f, b, rest, "sensor getter"))
                    for k in ("index", "track_id", "first", "count", "n_boxes"):
                        assert np.array_equal(g[k], s[k]), (f, b, k)
                    if f > 0 and len(g["xyz"]):
                        assert not np.array_equal(g["xyz"], s["xyz"])
                for misalign in (False, True):
                    p, s, cnt = DevBlocks(env, B, 8192, MAX_SEG, misalign).run(c, B, rest, "global")
                    for b in range(B):
                        check_block(p, s, cnt, b, wg[b], (f, b, rest, misalign, "global export"))


def global_frame_sequence(env, oracle):
    """five frames through sequence_dev (slot k = frame k, frame k's matrix) equal the same five fed one by one into a second context, slot k against call k, in both frames"""
    rng = np.random.default_rng(3)
    def blob(cx, cy):
        q = np.zeros((200, 4), np.float32); q[:, 0] = cx + rng.uniform(-0.4, 0.4, 200); q[:, 1] = cy + rng.uniform(-0.4, 0.4, 200); q[:, 2] = rng.uniform(-1.0, 0.3, 200); return q
    frames = [np.concatenate([blob(8.0 + 0.3 * f, 5.0), blob(-9.0, -6.0 - 0.3 * f), CC.small_scene(f, 12)]) for f in range(5)]
    ts = [2.0e8 + f * 1e5 for f in range(5)]; yaw = [0.05 * f for f in range(5)]
    one = []
    with env.context(0, max_points=2048, max_batch=1, max_tracks_total=256) as c:
        c.set_track_links(True)
        for f in range(5):
            keep = launch(env, c, [frames[f]], 2048, f, ego_v=1.0, yaw=yaw[f])
            m = c.sensor_pose(0)[1]
            r = {(rest, fr): c.get_track_points(0, rest=rest, frame=fr) for rest in (False, True) for fr in ("sensor", "global")}
            same(r[True, "global"], want_partition(c, 0, True, m), (f, "one by one, global"))
            one.append(r)
    assert any((r[True, "sensor"]["track_id"] >= 0).sum() >= 2 and (r[False, "sensor"]["count"] > 0).any() for r in one)
    with env.context(0, max_points=2048, max_batch=5, max_tracks_total=256) as c:
        c.set_track_links(True)
        host = np.zeros((5, 2048, 4), np.float32)
        for f, x in enumerate(frames):
            host[f, : len(x)] = x
        ptr, keep = env.upload(host)
        c.sequence_dev(ptr, 2048 * 4, [len(x) for x in frames], ts, [1.0] * 5, yaw)
        for rest in (False, True):
            for fr in ("sensor", "global"):
                p, s, cnt = DevBlocks(env, 5, 2048, MAX_SEG).run(c, 5, rest, fr)
                for k in range(5):
                    same(c.get_track_points(k, rest=rest, frame=fr), one[k][rest, fr], (k, rest, fr, "sequence getter"))
                    check_block(p, s, cnt, k, one[k][rest, fr], (k, rest, fr, "sequence export"))


# ------------------------------------------------------------------------------------------------------------------ 6: truncation
def truncation(env, oracle):
    frames = shape_frames(oracle)
    pick = [5, 9]   # 2047 and 7 719 points
    with env.context(0, max_points=8192, max_batch=2, max_tracks_total=512) as c:
        c.set_track_links(True)
        for f in range(3):
            keep = launch(env, c, [frames[f][k] for k in pick], 8192, f)
        for rest in (False, True):
            want = [want_partition(c, b, rest) for b in range(2)]
            for b in range(2):
                n, ns = len(want[b]["index"]), len(want[b]["track_id"])
                assert n > 1 and ns > 1
                for misalign in (False, True):   # one record / one segment less than slot b has (the other slot may then fit or not: both are checked)
                    p, s, cnt = DevBlocks(env, 2, n - 1, ns - 1, misalign).run(c, 2, rest, "sensor")
                    for k in range(2):
                        check_block(p, s, cnt, k, want[k], (rest, b, k, misalign, "truncated export"))
                # the host getter: MOT_E_CAPACITY, counts delivered, buffers untouched
                for cap_p, cap_s in ((n - 1, ns), (n, ns - 1)):
                    pts = np.full((n + 1) * 4, -7, np.int32); seg = np.full((ns + 1) * 4, -7, np.int32); npts, nseg = C.c_int(-7), C.c_int(-7)
                    rc = c.lib.mot_get_track_points(c._h, b, int(rest), env.mot.MOT_FRAME_SENSOR, pts.ctypes.data_as(C.c_void_p), cap_p, seg.ctypes.data_as(C.c_void_p), cap_s, C.byref(npts), C.byref(nseg))
                    assert rc == env.mot.MOT_E_CAPACITY and (npts.value, nseg.value) == (n, ns) and (pts == -7).all() and (seg == -7).all(), (rest, b, cap_p, cap_s, rc)
                rc = c.lib.mot_get_track_points(c._h, b, int(rest), env.mot.MOT_FRAME_SENSOR, pts.ctypes.data_as(C.c_void_p), n, seg.ctypes.data_as(C.c_void_p), ns, C.byref(npts), C.byref(nseg))
                assert rc == 0 and (pts[n * 4:] == -7).all() and (seg[ns * 4:] == -7).all() and np.array_equal(pts[: n * 4].reshape(n, 4)[:, 3], want[b]["index"])


# ------------------------------------------------------------------------------------------------------------------ 7: contract
KERNELS = (b"track_points_table_kernel", b"track_points_count_kernel", b"track_points_scan_kernel", b"track_points_scatter_kernel")


def launches_only_in_the_export(env, oracle):
    """emulator: the launch counter of every new kernel moves in the export calls and nowhere else"""
    lib = env.mot.load_library(env.lib_path)
    count = lambda: [lib.hipemu_launch_count(k) for k in KERNELS]
    with env.context(0, max_points=4096, max_batch=2, max_tracks_total=256) as c:
        before = count()
        c.set_track_links(True)
        for f in range(3):
            keep = launch(env, c, [CC.small_scene(f, 20), CC.small_scene(f + 5, 12)], 4096, f)
            for b in (0, 1):
                c.get_point_tracks(b); c.get_box_tracks(b); c.get_boxes(b); c.get_tracks(b)
        assert count() == before
        c.get_track_points(1)
        assert count() == [n + 1 for n in before]
        DevBlocks(env, 2, 4096, MAX_SEG).run(c, 2, True, "global")
        assert count() == [n + 2 for n in before]
        keep = launch(env, c, [CC.small_scene(3, 20), CC.small_scene(8, 12)], 4096, 3)
        assert count() == [n + 2 for n in before]


def raw_export(env, c, blk, batch, flags, frame, points=True, segments=True, counts=True):
    return c.lib.mot_export_track_points_dev(c._h, batch, flags, frame, C.c_void_p(blk.p_pts if points else None), C.c_long(blk.stride), C.c_void_p(blk.p_seg if segments else None),
                                             blk.max_seg, C.c_void_p(blk.p_cnt if counts else None))


def contract_state(env, oracle):
    E = env.mot
    with env.context(0, max_points=4096, max_batch=2, max_tracks_total=256) as c:
        blk = DevBlocks(env, 2, 4096, MAX_SEG)
        export = lambda batch=2: c.export_track_points_dev(batch, blk.p_pts, blk.stride, blk.p_seg, blk.max_seg, blk.p_cnt)
        clouds = [CC.small_scene(0, 20), CC.small_scene(1, 12)]
        keep = launch(env, c, clouds, 4096, 0)
        LC.state_error(env, lambda: c.get_track_points(0), "links off, getter"); LC.state_error(env, export, "links off, export")
        c.set_track_links(True)
        LC.state_error(env, lambda: c.get_track_points(0), "no step since the links were turned on"); LC.state_error(env, export, "no step, export")
        keep = launch(env, c, clouds, 4096, 1)
        before = [c.get_track_points(b, rest=True) for b in (0, 1)]
        assert len(before[1]["index"]) > 0
        # argument errors, on a context whose state would serve the call
        npts, nseg = C.c_int(0), C.c_int(0)
        getter = lambda slot, flags, frame, np_=npts, ns_=nseg: c.lib.mot_get_track_points(c._h, slot, flags, frame, None, 0, None, 0, C.byref(np_) if np_ is not None else None,
                                                                                               C.byref(ns_) if ns_ is not None else None)
        assert getter(0, 0, 2) == E.MOT_E_ARG and getter(0, 2, 0) == E.MOT_E_ARG and getter(2, 0, 0) == E.MOT_E_ARG and getter(-1, 0, 0) == E.MOT_E_ARG
        assert getter(0, 0, 0, None, nseg) == E.MOT_E_ARG and getter(0, 0, 0, npts, None) == E.MOT_E_ARG
        assert raw_export(env, c, blk, 2, 0, 2) == E.MOT_E_ARG and raw_export(env, c, blk, 2, 2, 0) == E.MOT_E_ARG
        assert raw_export(env, c, blk, 0, 0, 0) == E.MOT_E_ARG and raw_export(env, c, blk, 3, 0, 0) == E.MOT_E_ARG
        for kw in (dict(points=False), dict(segments=False), dict(counts=False)):
            assert raw_export(env, c, blk, 2, 0, 0, **kw) == E.MOT_E_ARG, kw
        p, s, cnt = blk.read()
        assert (p == -7).all() and (s == -7).all() and (cnt == -7).all(), "a refused call wrote into the caller's blocks"
        # a stage-wise call takes slot 0
        elev = c.get_ground(0, n_hint=len(clouds[0]))["elevated"]
        c.cluster(elev)
        LC.state_error(env, lambda: c.get_track_points(0), "slot 0 after mot_cluster")
        same(c.get_track_points(1, rest=True), before[1], "slot 1 is still served")
        LC.state_error(env, export, "export over a taken slot")
        keep = launch(env, c, clouds, 4096, 2)   # a fused call gives the slot back
        export(); c.get_track_points(0)
        c.ego_update(3.0e8, 0.0, 0.0, 1); c.track_step(LC.lattice(3), 3.0e8, slot=1)   # a tracker step fed from outside
        LC.state_error(env, lambda: c.get_track_points(1), "slot 1 after mot_track_step"); LC.state_error(env, export, "export after mot_track_step")
        export(1)   # slot 0 alone is still whole


def contract_refused(env, oracle):
    """a frame refused for capacity in slot 1: the getter answers MOT_E_CAPACITY with the limit's message; the export gives one rest segment of all its points
    with the flag and nothing without; the neighbour is served"""
    p = oracle.params(0)
    max_points = 8192
    at, beyond = CC.fused_edges(oracle, p, "groups", max_points)
    with env.context(0, max_points=max_points, max_batch=2, max_tracks_total=2048) as c:
        c.set_track_links(True)
        keep = launch(env, c, [CC.small_scene(0, 20), beyond], max_points, 0)
        keep2 = launch(env, c, [CC.small_scene(1, 20), beyond], max_points, 1)
        for rest in (False, True):
            CC.refused(env, lambda: c.get_track_points(1, rest=rest), CC.MSG_GROUPS, "track points of a refused frame")
            w0 = want_partition(c, 0, rest)
            same(c.get_track_points(0, rest=rest), w0, ("the neighbour", rest))
            pts, seg, cnt = DevBlocks(env, 2, max_points, MAX_SEG).run(c, 2, rest, "sensor")
            check_block(pts, seg, cnt, 0, w0, ("the neighbour, export", rest))
            if rest:
                n = int(cnt[1, 1])
                assert n > max_points // 2 and tuple(cnt[1]) == (1, n) and tuple(seg[1, 0]) == (-1, 0, n, 0), (cnt[1], seg[1, 0])
                assert np.array_equal(pts[1, :n, 3], np.arange(n)) and (pts[1, n:] == -7).all() and (seg[1, 1:] == -7).all()
            else:
                assert tuple(cnt[1]) == (0, 0) and (pts[1] == -7).all() and (seg[1] == -7).all(), cnt[1]


# ------------------------------------------------------------------------------------------------------------------ 8: non-interference
def readout(c, B, n_points):
    out = []
    for b in range(B):
        bx = c.get_boxes(b); t = c.get_tracks(b); g = c.get_ground(b, n_hint=n_points[b])
        ids = c.get_point_tracks(b)
        out += [("boxes", bx["boxes"].tobytes()), ("box_cluster", bx["box_cluster"].tobytes()), ("box_tracks", c.get_box_tracks(b).tobytes()), ("point_tracks", ids.tobytes()),
                ("point_label", c.get_clusters(b, n_elevated=max(len(ids), 1))["point_label"][: len(ids)].tobytes()),
                ("elevated", g["elevated"].tobytes()), ("ground", g["ground"].tobytes()), ("mask", g["mask"].tobytes()), ("markers", c.box_markers(b).tobytes())]
        out += [("tracks." + k, np.ascontiguousarray(t[k]).tobytes()) for k in ("track_manage", "lifetime", "p", "v_yaw", "vis_box", "is_vis", "is_static")]
        out += [("snapshot: " + n, x) for n, x in LC.snapshot_items(c.stream_save(b))]
    return out


def equal_readouts(a, b, what):
    assert [n for n, _ in a] == [n for n, _ in b], what
    for (n, x), (_, y) in zip(a, b):
        assert x == y, (what, n)


def non_interference(env, oracle, order_any=False, graphs=False):
    """everything a caller could read before the feature existed: the same before an export, after it, and in a context that never exported; the fused call after an
    export computes what it computes without one"""
    clouds = [[CC.small_scene(f, 20), CC.small_scene(f + 5, 12)] for f in range(4)]
    if order_any:
        clouds = [[np.ascontiguousarray(x[np.random.default_rng(11 + b).permutation(len(x))]) for b, x in enumerate(fr)] for fr in clouds]
    res = {}
    for tag in ("never", "exports"):
        with env.context(0, max_points=4096, max_batch=2, max_tracks_total=256) as c:
            c.set_launch_graphs(graphs); c.set_track_links(True)
            if order_any:
                c.set_point_order(env.mot.MOT_ORDER_ANY)
            for f in range(3):
                keep = launch(env, c, clouds[f], 4096, f, yaw=0.02 * f)
            n_points = [len(x) for x in clouds[2]]
            before = readout(c, 2, n_points)
            if tag == "exports":
                blk = DevBlocks(env, 2, 4096, MAX_SEG)
                for rest in (False, True):
                    for fr in ("sensor", "global"):
                        p, s, cnt = blk.run(c, 2, rest, fr)
                        r = c.get_track_points(1, rest=rest, frame=fr)
                        assert len(r["index"]) == cnt[1, 1] > 0
                equal_readouts(readout(c, 2, n_points), before, (tag, "after the export"))
            keep = launch(env, c, clouds[3], 4096, 3, yaw=0.06)
            res[tag] = (before, readout(c, 2, [len(x) for x in clouds[3]]))
    equal_readouts(res["exports"][0], res["never"][0], "against a context that never exported")
    equal_readouts(res["exports"][1], res["never"][1], "the fused call after an export")
