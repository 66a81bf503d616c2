"""Live tracks in the SENSOR frame (include/mot.h: mot_sensor_pose, mot_export_tracks_frame_dev, mot_export_tracks_packed_frame_dev,
mot_fetch_tracks_frame_async, mot_tracking_node_frame), shared by tests/test_emu_sensor_tracks.py (emulator) and tests/test_sensor_tracks_gpu.py
(MI355X): bodies only, the callers supply where they run (capacity_cases.Env). TEST INFRASTRUCTURE.

What is pinned bit for bit, and against what:
  the matrix     tests/golden/tf_to_sensor.npz: the reference node's own call sequence (tf broadcast, pcl_ros::transformPointCloud("/velodyne", ...)) on the
                 tf / pcl_ros restatement of oracle/ref_shim, recorded by tests/golden/make_tf_sensor_golden.py
  the exports    numpy's fp32 evaluation of pcl::transformPointCloud's per-point arithmetic (_apply) on the MOT_FRAME_GLOBAL records
  the node call  the stage-wise sequence mot_ego_update -> boxes through global_from_sensor -> mot_track_step -> records through sensor_from_global"""
import ctypes as C

import numpy as np

import golden_util as G
import tracker_cases as TC

REC = np.dtype([("id", "i4"), ("track_manage", "i4"), ("is_static", "i4"), ("is_vis", "i4"), ("p", "f4", 3), ("lifetime", "i4"),
                ("v_yaw", "f8", 2), ("vis_box", "f4", 24)])   # struct mot_track
assert REC.itemsize == 144
GLOBAL, SENSOR = 0, 1
POISON = 0xAB


def _apply(m, pts):
    """pcl::transformPointCloud's arithmetic: fp32, left to right (tests/test_tf_exact.py)"""
    m = np.asarray(m, np.float32).reshape(3, 4); b = np.asarray(pts, np.float32)
    x, y, z = b[..., 0], b[..., 1], b[..., 2]
    return np.stack([((m[r, 0] * x + m[r, 1] * y).astype(np.float32) + m[r, 2] * z).astype(np.float32) + m[r, 3] for r in range(3)], -1).astype(np.float32)


def matrix_inv(lib, x, y, yaw):
    m = np.zeros(12, np.float32)
    assert lib.mot_debug_tf_matrix_inv(C.c_double(x), C.c_double(y), C.c_double(yaw), m.ctypes.data_as(C.c_void_p)) == 0
    return m


def matrix_fwd(lib, x, y, yaw):
    m = np.zeros(12, np.float32)
    assert lib.mot_debug_tf_matrix(C.c_double(x), C.c_double(y), C.c_double(yaw), m.ctypes.data_as(C.c_void_p)) == 0
    return m


def to_sensor(rec, m):
    """what MOT_FRAME_SENSOR makes of global-frame records: px, py, pz and, where is_vis, the 8 corners of vis_box through m; nothing else"""
    out = rec.copy()
    if len(rec):
        out["p"] = _apply(m, rec["p"])
        vis = rec["is_vis"] != 0
        out["vis_box"][vis] = _apply(m, rec["vis_box"][vis].reshape(-1, 8, 3)).reshape(-1, 24)
    return out


def same_bytes(a, b, what):
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1); b = np.ascontiguousarray(b).view(np.uint8).reshape(-1)
    assert a.shape == b.shape, what
    bad = np.nonzero(a != b)[0]
    assert not len(bad), (what, "first differing byte", int(bad[0]), "of", len(a))


# ------------------------------------------------------------------------------------------------------------------ 1. the matrix
def matrix_against_fixture(env):
    lib = env.mot.load_library(env.lib_path)
    fx = G.load("tf_to_sensor.npz")
    assert len(fx["pose"]) == 64
    for pose, pts, want in zip(fx["pose"], fx["points"], fx["sensor"]):
        got = _apply(matrix_inv(lib, *pose), pts)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), pose


# ------------------------------------------------------------------------------------------------------------------ 2. - 4. the exports
STREAMS, T_TOTAL, BIG = 3, 70, 66


class State:
    """3 streams on 70 track slots, stepped with mot_track_steps_dev: stream 0 holds >= 65 live tracks (more than a wavefront, not a multiple of 64, and more than
    a 64-record tile of the export kernel), stream 1 none, stream 2 a handful of which the late-born are still hidden. Poses: stream 0 beyond pi and 300 m out,
    stream 1 beyond pi, stream 2 at exactly pi / 2 (first_ego_yaw_offset = 0 makes the dead-reckoned yaw -pi/2 + pi in doubles)."""

    def __init__(self, env):
        self.env = env
        self.c = c = env.context(0, pkw=dict(first_ego_yaw_offset=0.0), max_points=1024, max_batch=STREAMS, max_tracks_total=T_TOTAL)
        rng = np.random.default_rng(21)
        vel = rng.uniform(-1.0, 1.0, size=(1, BIG, 2))
        few_vel = rng.uniform(-1.0, 1.0, size=(1, 6, 2))
        stride = BIG * 24
        frames = 12
        for f in range(frames):
            ts = 1.0e9 + f * 1e5
            bx = np.zeros((STREAMS, BIG, 8, 3), np.float32)
            bx[0] = TC.grid_boxes(1, BIG, f, vel, rng, 9.0)[0]
            m2 = 4 if f < frames - 2 else 6   # two objects appear at the end: their tracks are tentative, not shown
            bx[2, :6] = TC.grid_boxes(1, 6, f, few_vel, rng, 9.0)[0]
            last = f == frames - 1
            c.ego_update(ts, 3000.0 if last else 4.0, 0.5 * f, 0)          # yaw -pi/2 - 0.5 f: -7.07 at the end; 300 m in the last step
            c.ego_update(ts, 2.0, -0.45 * f, 1)                          # yaw -pi/2 + 0.45 f: 3.38 at the end
            c.ego_update(ts, 0.0, 0.0 if f == 0 else -np.pi, 2)          # yaw -pi/2 + pi = pi/2 exactly from frame 1 on
            ptr, keep = env.upload(bx.reshape(STREAMS, stride))
            c.track_steps_dev(ptr, stride, [BIG, 0, m2], [ts] * STREAMS)
            c.synchronize()
            del keep
        self.sfg = [c.sensor_pose(s)[0] for s in range(STREAMS)]
        self.gfs = [c.sensor_pose(s)[1] for s in range(STREAMS)]
        self.all = [c.get_tracks(s) for s in range(STREAMS)]

    def close(self):
        self.c.close()

    # the three calls, each into a poisoned destination; returns host copies
    def fixed(self, frame, max_per_slot):
        env, c = self.env, self.c
        rec = np.full((STREAMS, max_per_slot, REC.itemsize), POISON, np.uint8); cnt = np.full(STREAMS, -7, np.int32)
        pr, kr = env.upload(rec); pc, kc = env.upload(cnt)
        rc = c.lib.mot_export_tracks_frame_dev(c._h, STREAMS, frame, C.c_void_p(pr), max_per_slot, C.c_void_p(pc)) if frame is not None else \
            c.lib.mot_export_tracks_dev(c._h, STREAMS, C.c_void_p(pr), max_per_slot, C.c_void_p(pc))
        assert rc == 0, c.lib.mot_last_error(c._h)
        c.synchronize()
        return _download(kr, rec).view(REC).reshape(STREAMS, max_per_slot), _download(kc, cnt)

    def packed(self, frame, capacity):
        env, c = self.env, self.c
        nbytes = 16 + capacity * REC.itemsize
        blk = np.full(nbytes, POISON, np.uint8)
        pb, kb = env.upload(blk)
        rc = c.lib.mot_export_tracks_packed_frame_dev(c._h, STREAMS, frame, C.c_void_p(pb), C.c_long(nbytes)) if frame is not None else \
            c.lib.mot_export_tracks_packed_dev(c._h, STREAMS, C.c_void_p(pb), C.c_long(nbytes))
        assert rc == 0, c.lib.mot_last_error(c._h)
        c.synchronize()
        return _download(kb, blk)

    def fetched(self, frame, max_per_slot):
        c = self.c
        rec = np.full((STREAMS, max_per_slot, REC.itemsize), POISON, np.uint8); cnt = np.full(STREAMS, -7, np.int32)
        rc = c.lib.mot_fetch_tracks_frame_async(c._h, STREAMS, frame, C.c_void_p(rec.ctypes.data), max_per_slot, C.c_void_p(cnt.ctypes.data)) if frame is not None else \
            c.lib.mot_fetch_tracks_async(c._h, STREAMS, C.c_void_p(rec.ctypes.data), max_per_slot, C.c_void_p(cnt.ctypes.data))
        assert rc == 0, c.lib.mot_last_error(c._h)
        c.synchronize()
        return rec.view(REC).reshape(STREAMS, max_per_slot), cnt


def _download(keep, like):
    """the destination's content: the emulator's "device" memory IS the host array; a tests/hiprt.py DeviceBuffer is copied back"""
    return keep if isinstance(keep, np.ndarray) else keep.to_host(like.dtype, like.shape)


def state_is_what_the_cases_need(st):
    """the shape of the state, asserted before anything is compared on it"""
    live = [int((a["track_manage"] != 0).sum()) for a in st.all]
    assert live[0] >= 65 and live[0] % 64 != 0 and live[0] <= T_TOTAL, live
    assert live[1] == 0 and 4 <= live[2] <= 8, live
    vis2 = st.all[2]["is_vis"][st.all[2]["track_manage"] != 0]
    assert (vis2 != 0).any() and (vis2 == 0).any(), vis2
    assert (st.all[0]["is_vis"] != 0).sum() >= 60
    lib = st.c.lib
    # the poses, read back through the matrices: rebuilt from the dead reckoning the case drove
    yaw0 = -np.pi / 2 - 0.5 * 11
    assert abs(yaw0) > np.pi
    same_bytes(st.sfg[2].reshape(-1), matrix_inv(lib, 0.0, 0.0, np.pi / 2), "stream 2 sits at exactly pi / 2")
    same_bytes(st.gfs[2].reshape(-1), matrix_fwd(lib, 0.0, 0.0, np.pi / 2), "stream 2 sits at exactly pi / 2")
    assert abs(np.arctan2(st.sfg[1][1, 0], st.sfg[1][0, 0]) - (-np.pi / 2 + 0.45 * 11 - 2 * np.pi)) < 1e-5   # stream 1: 3.38 rad, beyond pi
    assert np.hypot(st.sfg[0][0, 3], st.sfg[0][1, 3]) > 295.0, st.sfg[0]
    assert not np.array_equal(st.sfg[0], st.sfg[1]) and not np.array_equal(st.sfg[1], st.sfg[2])
    return live


def _expect_fixed(st, g_rec, g_cnt):
    want = g_rec.copy()
    for s in range(STREAMS):
        want[s, : g_cnt[s]] = to_sensor(g_rec[s, : g_cnt[s]], st.sfg[s])
    return want


def export_sensor(st):
    live = state_is_what_the_cases_need(st)
    for max_per_slot in (T_TOTAL, 40):   # whole, and cut inside stream 0 (40 < 64 < live[0])
        g_rec, g_cnt = st.fixed(GLOBAL, max_per_slot)
        assert list(g_cnt) == [min(n, max_per_slot) for n in live]
        for s in range(STREAMS):   # the live tracks in id order: what mot_get_tracks reports as alive
            a = st.all[s]; ids = np.nonzero(a["track_manage"] != 0)[0][: g_cnt[s]]
            assert np.array_equal(g_rec[s, : g_cnt[s]]["id"], ids), s
            same_bytes(g_rec[s, : g_cnt[s]]["p"], a["p"][ids], ("global records are mot_get_tracks'", s))
        want = _expect_fixed(st, g_rec, g_cnt)
        for name, call in (("fixed block", st.fixed), ("async fetch", st.fetched)):
            rec, cnt = call(SENSOR, max_per_slot)
            assert np.array_equal(cnt, g_cnt), (name, cnt, g_cnt)
            # every dword: transformed coordinates, everything else as in the global record; the fixed block's poisoned tail untouched (the fetch copies its
            # whole device block, whose tail is nobody's)
            if name == "fixed block":
                same_bytes(rec, want, (name, max_per_slot))
            for s in range(STREAMS):
                same_bytes(rec[s, : cnt[s]], want[s, : cnt[s]], (name, max_per_slot, s))
            for s in range(STREAMS):
                hidden = rec[s, : cnt[s]]; hidden = hidden[hidden["is_vis"] == 0]
                assert not hidden["vis_box"].view(np.uint32).any(), (name, s)
        moved = want[0, : g_cnt[0]]["p"].view(np.uint32) != g_rec[0, : g_cnt[0]]["p"].view(np.uint32)
        assert moved.any(), "the sensor-frame records differ from the global ones"
    total = sum(live)
    for capacity in (total, live[0] + live[1] + 2, 40):   # whole; cut inside stream 2; cut inside stream 0
        g = st.packed(GLOBAL, capacity)
        head = g[:16].view(np.int32)
        assert list(head[:STREAMS]) == live
        want = g.copy()
        wrec = want[16:].view(REC)
        off = 0
        for s in range(STREAMS):
            n = max(0, min(live[s], capacity - off))
            wrec[off: off + n] = to_sensor(wrec[off: off + n], st.sfg[s])
            off += live[s]
        same_bytes(st.packed(SENSOR, capacity), want, ("packed block", capacity))


def export_global(st):
    """MOT_FRAME_GLOBAL is the existing call, byte for byte (poisoned tails included)"""
    live = state_is_what_the_cases_need(st)
    for max_per_slot in (T_TOTAL, 40):
        for name, call in (("fixed block", st.fixed), ("async fetch", st.fetched)):
            a, ac = call(None, max_per_slot); b, bc = call(GLOBAL, max_per_slot)
            assert np.array_equal(ac, bc), name
            if name == "fixed block":
                same_bytes(a, b, (name, max_per_slot))
            for s in range(STREAMS):
                same_bytes(a[s, : ac[s]], b[s, : bc[s]], (name, max_per_slot, s))
    for capacity in (sum(live), live[0] + 2, 40):
        same_bytes(st.packed(None, capacity), st.packed(GLOBAL, capacity), ("packed block", capacity))
    c = st.c
    assert c.lib.mot_export_tracks_packed_frame_dev(c._h, STREAMS, 2, C.c_void_p(16), C.c_long(1024)) == 1   # MOT_E_ARG: no such frame


def round_trip(st):
    """A sanity bound, not a pin: sensor -> global -> sensor returns to within 1e-3 m with the vehicle 300 m from its origin. fp32 spacing at 300 m is 3e-5 m;
    each direction is a handful of fp32 operations on values of that size. Catches a swapped or transposed matrix, nothing finer."""
    lib = st.c.lib
    rng = np.random.default_rng(4)
    boxes = rng.uniform(-60, 60, size=(50, 8, 3)).astype(np.float32)
    poses = [(300.0, 0.0, 0.3), (-212.0, 212.0, -2.9), (0.0, -300.0, np.pi / 2), (250.0, 160.0, 5.5)]
    for x, y, yaw in poses:
        back = _apply(matrix_inv(lib, x, y, yaw), _apply(matrix_fwd(lib, x, y, yaw), boxes))
        assert np.abs(back - boxes).max() < 1e-3, (x, y, yaw, np.abs(back - boxes).max())
    back = _apply(st.sfg[0], _apply(st.gfs[0], boxes))   # and the 300 m pose the state's stream 0 holds, through the public call
    assert np.abs(back - boxes).max() < 1e-3


# ------------------------------------------------------------------------------------------------------------------ 5. the one-call node
class _Frame(C.Structure):
    _fields_ = [("origin6", C.c_double * 6), ("n_live", C.c_int32), ("n_ever", C.c_int32), ("tracks", C.c_void_p)]


def _node_call(c, slot, boxes, ts, v, yaw):
    b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 8, 3); fr = _Frame()
    rc = c.lib.mot_tracking_node_frame(c._h, slot, b.ctypes.data_as(C.c_void_p), len(b), C.c_double(ts), C.c_double(v), C.c_double(yaw), C.byref(fr))
    rec = np.ctypeslib.as_array(C.cast(fr.tracks, C.POINTER(C.c_uint8)), shape=(fr.n_live * REC.itemsize,)).view(REC).copy() if fr.n_live > 0 else np.zeros(0, REC)
    return rc, np.array(fr.origin6[:]), rec, fr.n_ever


def _stage_wise(c, slot, boxes, ts, v, yaw, cap=512):
    """the four calls the node call stands for"""
    origin = c.ego_update(ts, v, yaw, slot)
    sfg, gfs = c.sensor_pose(slot)
    b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 8, 3)
    bg = np.ascontiguousarray(_apply(gfs, b)) if len(b) else b
    arr = np.zeros(cap, REC); nt = C.c_int(0)
    rc = c.lib.mot_track_step(c._h, slot, bg.ctypes.data_as(C.c_void_p), len(bg), C.c_double(ts), arr.ctypes.data_as(C.c_void_p), cap, C.byref(nt))
    assert 0 <= nt.value <= cap
    rec = arr[: nt.value]
    return rc, origin, to_sensor(rec[rec["track_manage"] != 0], sfg), nt.value


def _ego(f):
    return 1.0 + 0.5 * np.sin(0.4 * f), 0.02 * f * np.cos(0.3 * f) - 0.2   # a wandering vehicle


def node_frame_equals_the_stage_wise_sequence(env, max_tracks_total=64, frames=20, expect_capacity=False):
    """slot 1 of a 2-slot context (a hard-wired slot 0 would show), 20 frames of fast_lanes, one of them empty and one refused call with 1025 boxes"""
    seen_capacity = None; shown = most = 0
    with env.context(0, max_points=1024, max_batch=2, max_tracks_total=max_tracks_total) as a, env.context(0, max_points=1024, max_batch=2, max_tracks_total=max_tracks_total) as b:
        for f, (boxes, ts, _v, _yaw) in enumerate(TC.fast_lanes(7, frames)):
            v, yaw = _ego(f)
            if f == 6:
                boxes = boxes[:0]   # m = 0
            if f == 9:   # m = 1025: refused before anything runs; the frames after it equal the other route's, which never saw the call
                rc, _, rec, _ = _node_call(a, 1, np.zeros((1025, 8, 3), np.float32), ts, v, yaw)
                assert rc == 1 and len(rec) == 0
            ra, oa, reca, na = _node_call(a, 1, boxes, ts, v, yaw)
            rb, ob, recb, nb = _stage_wise(b, 1, boxes, ts, v, yaw)
            assert ra == rb and ra in (0, 2), (f, ra, rb)
            same_bytes(oa, ob, ("origin6", f))
            assert na == nb, (f, na, nb)
            same_bytes(reca, recb, ("records", f))
            shown += int((reca["is_vis"] != 0).sum()); most = max(most, len(reca))
            if ra == 2 and seen_capacity is None:
                seen_capacity = f
            if seen_capacity is not None:
                assert ra == 2, ("sticky", f)
        assert (seen_capacity is not None) == expect_capacity, seen_capacity
        assert len(reca) >= 1 and (expect_capacity or (most >= 4 and shown >= 4)), (most, shown, reca)   # records with a visible box went through both routes
        ga, gb = a.get_tracks(1), b.get_tracks(1)   # the state behind the records
        assert ga["n"] == gb["n"]
        for k in ("track_manage", "is_vis", "lifetime", "p", "v_yaw", "vis_box"):
            same_bytes(ga[k], gb[k], k)
        alive = [int(i) for i in reca["id"][:3]]
        assert len(alive) == 3 or expect_capacity
        for i in alive:
            sa, sb = a.track_state(i, slot=1), b.track_state(i, slot=1)
            for k in sa:
                same_bytes(np.asarray(sa[k]), np.asarray(sb[k]), ("state", i, k))
        assert a.get_tracks(0)["n"] == 0   # slot 0 was never stepped


def node_frame_leaves_the_box_stage_alone(env):
    """mot_get_boxes / mot_box_markers of a slot that holds a fused frame answer the same before and after mot_tracking_node_frame on it"""
    import capacity_cases as CC
    N, stride = 4096, 4096
    clouds = np.zeros((2, stride, 4), np.float32)
    n = []
    for s in range(2):
        cl = CC.small_scene(s, 12)[:N]
        clouds[s, : len(cl)] = cl; n.append(len(cl))
    with env.context(0, max_points=stride, max_batch=2, max_tracks_total=64) as c:
        ptr, keep = env.upload(clouds)
        c.frames_dev(ptr, stride * 4, n)
        before = [(c.get_boxes(s), c.box_markers(s)) for s in range(2)]
        assert len(before[1][0]["boxes"]) >= 4
        for f in range(3):
            rc, _, rec, _ = _node_call(c, 1, before[1][0]["boxes"], 1.0e9 + f * 1e5, 2.0, 0.01 * f)
            assert rc == 0
        assert len(rec) >= 1
        for s in range(2):
            bx, mk = c.get_boxes(s), c.box_markers(s)
            same_bytes(bx["boxes"], before[s][0]["boxes"], ("boxes", s)); assert np.array_equal(bx["box_cluster"], before[s][0]["box_cluster"])
            same_bytes(mk, before[s][1], ("markers", s))
        del keep


def python_layer(env):
    """Context.tracking_node_frame / sensor_pose / export_tracks_dev(frame=) / fetch_tracks_async(frame=) say what the C calls say"""
    with env.context(0, max_points=1024, max_batch=2, max_tracks_total=32) as a, env.context(0, max_points=1024, max_batch=2, max_tracks_total=32) as b:
        sfg, gfs = a.sensor_pose(1)
        lib = a.lib
        same_bytes(sfg.reshape(-1), matrix_inv(lib, 0.0, 0.0, 0.0), "pose (0, 0, 0) before the first update"); same_bytes(gfs.reshape(-1), matrix_fwd(lib, 0.0, 0.0, 0.0), "forward")
        for f, (boxes, ts, _v, _yaw) in enumerate(TC.fast_lanes(3, 8)):
            v, yaw = _ego(f)
            r = a.tracking_node_frame(boxes, ts, v, yaw, slot=1)
            rb, ob, recb, nb = _stage_wise(b, 1, boxes, ts, v, yaw)
            assert not r["capacity_exceeded"] and r["n_ever"] == nb and r["n_live"] == len(recb)
            same_bytes(r["origin"], ob, f); same_bytes(r["tracks"], recb, f)
        for ctx in (a, b):   # both routes left the same records for the frame-aware exports
            rec = np.full((2, 32), 0, REC); cnt = np.zeros(2, np.int32)
            ctx.fetch_tracks_async(2, rec.ctypes.data, 32, cnt.ctypes.data, frame="sensor"); ctx.synchronize()
            assert cnt[0] == 0 and cnt[1] == len(recb)
            same_bytes(rec[1, : cnt[1]], recb, "fetch_tracks_async(frame='sensor')")
        try:
            a.fetch_tracks_async(2, rec.ctypes.data, 32, cnt.ctypes.data, frame="vehicle")
            raise AssertionError("an unknown frame must be refused")
        except ValueError:
            pass
