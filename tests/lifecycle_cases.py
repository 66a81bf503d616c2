"""A context's life cycle (csrc/mot_host.h "ownership": every allocation, event and captured graph of a mot_ctx has one owner), shared by
tests/test_emu_lifecycle.py (emulator: live-allocation ledger and injected allocation failures of tests/emu/hipemu.h) and tests/test_lifecycle_gpu.py
(MI355X: create -> touch_everything -> destroy, repeated). Bodies only, the callers supply where they run (capacity_cases.Env). TEST INFRASTRUCTURE.

touch_everything calls once every path of the C-ABI that allocates lazily; every call in it is a valid one."""
import ctypes as C

import numpy as np

import capacity_cases as CC

MAX_POINTS, BATCH, T_TOTAL = 4096, 2, 16
ORDER_SCAN, ORDER_ANY, SENSOR = 0, 1, 1
MOT_E_HIP, MOT_E_STATE = 3, 4
K1 = 10   # kernel id of mot_profile_kernel: the first ground kernel
TRACK_REC = 144


def clouds():
    """four frames of 8 box-sized blobs (384 points each), on the same cells whatever the seed: a stream of them keeps its tracks"""
    return [CC.small_scene(s, 8) for s in range(4)]


def context(env):
    return env.context(0, max_points=MAX_POINTS, max_batch=BATCH, max_tracks_total=T_TOTAL)


def ok(c, rc):
    assert rc == 0, (rc, c.lib.mot_last_error(c._h))


class Feed:
    """frames for both slots, one pair after another, through whichever ingest call; remembers what it fed (`steps`: the tracker steps, for an oracle to replay)
    and what it read back (`boxes`)"""

    def __init__(self, c, frames):
        self.c, self.frames, self.f = c, frames, 0
        self.steps, self.boxes = [], []
        self.keep = []

    def pair(self):
        k = self.f % (len(self.frames) - 1)
        return [self.frames[k], self.frames[k + 1]]

    def _args(self):
        ts = 2.0e8 + self.f * 1e5
        return dict(run_tracker=True, timestamps=[ts] * BATCH, ego_v=[1.0] * BATCH, ego_yaw=[0.0] * BATCH), ts

    def _done(self, pair, ts):
        c = self.c
        c.synchronize(); c.wait_uploads()
        for b, x in enumerate(pair):
            self.steps.append(("fused", b, x, ts))
            self.boxes.append((x, c.get_boxes(b)))
        self.f += 1

    def host(self, w):
        """mot_frames_host (w = 4) / mot_frames_host_xyz (w = 3)"""
        pair = self.pair(); kw, ts = self._args()
        host = np.zeros((BATCH, MAX_POINTS, w), np.float32)
        for b, x in enumerate(pair):
            host[b, : len(x)] = x[:, :w]
        self.keep.append(host)
        (self.c.frames_host if w == 4 else self.c.frames_host_xyz)(host.ctypes.data, MAX_POINTS * w, [len(x) for x in pair], **kw)
        self._done(pair, ts)

    def pointcloud2(self, point_step):
        """x, y, z at 4, 8, 12 of a record of point_step bytes, no 4th field"""
        pair = self.pair(); kw, ts = self._args()
        payloads = []
        for x in pair:
            raw = np.zeros((len(x), point_step), np.uint8)
            raw[:, 4:16] = np.ascontiguousarray(x[:, :3]).view(np.uint8).reshape(len(x), 12)
            payloads.append(raw)
        self.keep.append(payloads)
        self.c.frames_host_pointcloud2(payloads, [len(x) for x in pair], point_step, 4, 8, 12, -1, **kw)
        self._done(pair, ts)

    def node_frame(self, slot):
        """mot_tracking_node_frame on the boxes the slot's last fused frame left"""
        x, bx = self.boxes[-BATCH + slot]
        ts = 2.0e8 + self.f * 1e5
        out = self.c.tracking_node_frame(bx["boxes"], ts, 1.0, 0.0, slot=slot)
        self.steps.append(("node", slot, x, ts))
        self.f += 1
        return out


def touch_everything(env, c, frames):
    """every lazily allocating path of the ABI once, on a fresh context; returns (boxes read, tracks read, tracker steps taken)"""
    lib, h = c.lib, c._h
    fd = Feed(c, frames)
    fd.host(4)                         # copy stream, d_stage, ev_copied / ev_consumed
    fd.host(3)                         # d_stage12, ev_expanded
    fd.pointcloud2(16)                 # d_stage_raw
    fd.pointcloud2(32)                 # ... replaced by larger ones
    c.set_point_order(ORDER_ANY)       # the regrouping buffers
    fd.host(4)
    c.set_track_links(True)            # owner rows, per-point ids
    fd.host(4)
    links = [c.get_box_tracks(b) for b in range(BATCH)]
    for per_slot in (4, T_TOTAL):      # d_fetch, grown
        rec = np.zeros((BATCH, per_slot, TRACK_REC), np.uint8); cnt = np.zeros(BATCH, np.int32)
        ok(c, lib.mot_fetch_tracks_async(h, BATCH, C.c_void_p(rec.ctypes.data), per_slot, C.c_void_p(cnt.ctypes.data)))
        c.synchronize()
    rec_s = np.zeros((BATCH, T_TOTAL, TRACK_REC), np.uint8); cnt_s = np.zeros(BATCH, np.int32)
    ok(c, lib.mot_fetch_tracks_frame_async(h, BATCH, SENSOR, C.c_void_p(rec_s.ctypes.data), T_TOTAL, C.c_void_p(cnt_s.ctypes.data)))   # d_sensor_tf and its ring
    c.synchronize()
    node = fd.node_frame(0)            # d_node_boxes, d_node_out
    products = c.cluster_products(1)   # the side-product buffers
    markers = c.box_markers(1)         # d_markers
    for point_step in (16, 32):        # d_raw, grown
        x = frames[0]
        raw = np.zeros((len(x), point_step), np.uint8)
        raw[:, 4:16] = np.ascontiguousarray(x[:, :3]).view(np.uint8).reshape(len(x), 12)
        ground = c.ground_remove_pointcloud2(raw, len(x), point_step, 4, 8, 12)
    c.profile_kernel(K1)               # the timing events
    fd.host(4)
    prof = c.profile_read()
    c.profile_kernel(0)
    c.set_launch_graphs(True)          # a captured launch sequence (GPU; the emulator launches plainly)
    fd.host(4)
    c.set_tracker_mode(1)              # ... dropped, and captured again
    fd.host(4)
    tracks = [c.get_tracks(b) for b in range(BATCH)]   # the page-locked read-back block
    assert prof["samples"] >= 1 and len(markers) == len(fd.boxes[-1][1]["boxes"]) and len(ground["elevated"]) and products["cost_map"].size
    assert all(len(links[b]) for b in range(BATCH)) and cnt_s[0] == cnt[0]
    return fd.boxes, dict(tracks=tracks, node=node, fetched=(rec, cnt, rec_s, cnt_s)), fd.steps


def flatten(boxes, tracks):
    """everything touch_everything read, as one list of arrays: two runs are the same run when these are the same bytes"""
    out = []
    for _, bx in boxes:
        out += [bx["boxes"], bx["box_cluster"], np.array([bx["n_undefined"]])]
    for t in tracks["tracks"]:
        out += [np.array([t["n"], int(t["capacity_exceeded"])]), t["track_manage"], t["lifetime"], t["is_static"], t["is_vis"], t["p"], t["v_yaw"], t["vis_box"]]
    node = tracks["node"]
    if node is not None:
        out += [node["tracks"].view(np.uint8), np.array([node["n_live"], node["n_ever"]]), node["origin"]]
    out += list(tracks["fetched"])
    return out


def same_run(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        x = np.ascontiguousarray(x); y = np.ascontiguousarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, k)


def against_oracle(oracle, boxes, tracks, steps):
    """the boxes of every frame against the oracle's for that frame (bit for bit), the final tracks of both streams against oracle trackers that took the same steps"""
    p = oracle.params(0)
    fit = {}
    for x, got in boxes:
        if id(x) not in fit:
            fit[id(x)] = CC.oracle_frame(oracle, p, x)[1]["bx"]
        CC.same_boxes(got, fit[id(x)], "boxes of a frame")
    T = [oracle.Tracker(p) for _ in range(BATCH)]
    last = [None] * BATCH
    for _, b, x, ts in steps:   # (a fused step and the node call feed the tracker the same boxes: the frame's, sensor -> global by the stream's pose)
        ego = T[b].ego_update(ts, 1.0, 0.0)
        co, si = np.cos(-ego[2]), np.sin(-ego[2])
        gb = fit[id(x)]["boxes"].astype(np.float64).copy()
        dx, dy = gb[..., 0] - ego[0], gb[..., 1] - ego[1]
        gb[..., 0] = co * dx - si * dy; gb[..., 1] = si * dx + co * dy
        last[b] = T[b].step(gb.astype(np.float32), ts)
    for b in range(BATCH):
        CC.same_tracks(tracks["tracks"][b], last[b], ("tracks of stream", b))
        T[b].close()
