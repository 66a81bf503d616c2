"""Object-centred track models (mot_export_track_models_dev / mot_get_track_models, csrc/track_models.hip): bodies shared by tests/test_emu_track_models.py
(emulator) and tests/test_track_models_gpu.py (MI355X). The callers supply a capacity_cases.Env.

The expectation is a Python model that shares no code with the kernels: per slot, get_accum_rows and get_track_accumulated — both exist without the feature —
give the unrolled ring and log of every row, and numpy applies the definition of include/mot.h: the kept points whose step is at least the oldest logged
observation's, each minus the position of the observation of its step, optionally rotated by minus that observation's yaw; packed in ascending row.

Comparisons: headers, counts, packing, z bits and step stamps exactly under every flag; without MOT_MODEL_AXES x', y' bit for bit (one fp32 subtraction); with it
|x' - x'_64| <= 5 * 2^-24 * (|dx| + |dy|) against the float64 model (one rounding each of dx, c, the two products and the sum is 4.5 units of 2^-24 relative to
|dx| + |dy|, the rest is second-order slack; dx, dy are the float64 differences), likewise y'. Extents equal, by value, min / max over the finite records the
call itself wrote; without AXES they also equal the model's."""
import ctypes as C

import numpy as np

import capacity_cases as CC
import track_accum_cases as AC
import track_link_cases as LC
import track_point_cases as PC

TILE = 128   # records a workgroup of the transform kernel takes per round (csrc/mot_internal.h kTrackModelTile)
OBS_TILE = 64   # observations the transform kernel holds in LDS at a time (csrc/track_models.hip kTmObsTile)
FLAGS = [(False, False), (True, False), (False, True), (True, True)]   # (axes, current)
KERNELS = (b"track_models_plan_kernel", b"track_models_transform_kernel")
INT_FIELDS = ("track_id", "first", "count", "n_obs", "first_step", "last_step")


def flag_bits(env, axes, current):
    return (env.mot.MOT_MODEL_AXES if axes else 0) | (env.mot.MOT_MODEL_CURRENT if current else 0)


# ------------------------------------------------------------------------------------------------------------------ the model
def want_slot(env, c, b, axes, current, latest):
    """slot b's models by the definition, from the accumulator getters. latest: the slot's latest accumulated step (accepted accumulate calls - 1)"""
    E = env.mot
    rows = c.get_accum_rows(b)
    v = c.track_accumulators_dev()
    T, K, O = v["tracks_per_slot"], v["points_per_track"], v["obs_per_track"]
    models = np.zeros(T, E.TRACK_MODEL_DTYPE); models["track_id"] = -1
    z, step, x32, y32, x64, y64, bound = [], [], [], [], [], [], []
    facts = dict(strict_suffix=0, whole_ring=0, sin_max=0.0, dropped_by_current=0, n_obs=[], counts=[])
    first = 0
    for r in range(T):
        row = rows[r]
        if row["track_id"] < 0 or row["obs_total"] <= 0:
            continue
        if current and row["last_step"] != latest:
            facts["dropped_by_current"] += 1
            continue
        g = c.get_track_accumulated(b, int(row["track_id"]))
        assert g["row"].tobytes() == row.tobytes(), "two rows hold one id"
        obs = g["obs"]
        assert len(obs) == min(int(row["obs_total"]), O) and (np.diff(obs["step"]) > 0).all() and (np.diff(g["step"]) >= 0).all()
        keep = g["step"] >= obs["step"][0]
        n = int(keep.sum())
        assert keep[len(keep) - n:].all(), "the kept records are not a suffix of the unrolled ring"
        facts["strict_suffix" if n < len(keep) else "whole_ring"] += 1
        facts["sin_max"] = max(facts["sin_max"], float(np.abs(np.sin(obs["yaw"])).max()))
        facts["n_obs"].append(len(obs)); facts["counts"].append(n)
        p = np.ascontiguousarray(g["xyz"][keep], np.float32); s = g["step"][keep]
        j = np.searchsorted(obs["step"], s)
        assert (obs["step"][j] == s).all(), "a kept point's step has no observation"
        px, py, yaw = obs["px"][j], obs["py"][j], obs["yaw"][j]
        with np.errstate(invalid="ignore"):
            dx32, dy32 = p[:, 0] - px, p[:, 1] - py   # fp32
            dx, dy = p[:, 0].astype(np.float64) - px.astype(np.float64), p[:, 1].astype(np.float64) - py.astype(np.float64)
            if axes:
                cs, sn = np.cos(yaw), np.sin(yaw)
                x64.append(cs * dx + sn * dy); y64.append(cs * dy - sn * dx)
            else:
                x64.append(dx); y64.append(dy)
            bound.append(5 * 2.0 ** -24 * (np.abs(dx) + np.abs(dy)))
        x32.append(dx32); y32.append(dy32); z.append(p[:, 2]); step.append(s)
        m = models[r]
        m["track_id"], m["first"], m["count"], m["n_obs"], m["first_step"], m["last_step"] = row["track_id"], first, n, len(obs), obs["step"][0], row["last_step"]
        if not axes:
            m["min"], m["max"] = extent(np.stack([dx32, dy32, p[:, 2]], 1))
        first += n
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return dict(models=models, counts=(int((models["track_id"] >= 0).sum()), first), z=cat(z, np.float32), step=cat(step, np.int32), x32=cat(x32, np.float32),
                y32=cat(y32, np.float32), x64=cat(x64, np.float64), y64=cat(y64, np.float64), bound=cat(bound, np.float64), facts=facts)


def extent(xyz):
    """min / max over the rows whose three coordinates are finite; zeros when there are none"""
    ok = np.isfinite(xyz).all(1)
    if not ok.any():
        return np.zeros(3, np.float32), np.zeros(3, np.float32)
    return xyz[ok].min(0), xyz[ok].max(0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_or_both_nan(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN records")
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan]), (what, "bits")


def compare(models, recs, counts, want, axes, what, full_models=None):
    """one slot of a call against the model. recs: the int32 [n_written, 4] records the call wrote (all of them, or the first point_stride); full_models: the
    headers of an untruncated call under the same flags, whose extents a truncated call must repeat"""
    wm = want["models"]
    for f in INT_FIELDS:
        assert np.array_equal(models[f], wm[f]), (what, f, models[f][models[f] != wm[f]][:8], wm[f][models[f] != wm[f]][:8])
    assert tuple(int(x) for x in counts) == want["counts"], (what, "counts", tuple(counts), want["counts"])
    used = models[models["track_id"] >= 0]
    assert np.array_equal(used["first"], np.concatenate([[0], np.cumsum(used["count"])[:-1]])[: len(used)]), (what, "packing")
    empty = models[models["track_id"] < 0]
    assert not empty.tobytes().replace(b"\xff", b"\x00").strip(b"\x00"), (what, "an empty model is not {-1, 0, ...}")
    n = want["counts"][1]; wn = len(recs)
    assert wn <= n
    xyz = np.ascontiguousarray(recs[:, :3]).view(np.float32)
    assert np.array_equal(recs[:, 3], want["step"][:wn]), (what, "step stamps")
    assert np.array_equal(bits(xyz[:, 2]), bits(want["z"][:wn])), (what, "z bits")
    if not axes:
        same_or_both_nan(xyz[:, 0], want["x32"][:wn], (what, "x'")); same_or_both_nan(xyz[:, 1], want["y32"][:wn], (what, "y'"))
    else:
        for k, w64 in ((0, want["x64"][:wn]), (1, want["y64"][:wn])):
            nan = np.isnan(w64)
            assert np.array_equal(np.isnan(xyz[:, k]), nan), (what, "NaN records", k)
            err = np.abs(xyz[:, k].astype(np.float64) - w64)[~nan]; lim = want["bound"][:wn][~nan]
            assert (err <= lim).all(), (what, "xy"[k] + "' against the float64 model", float((err - lim).max()), float(err.max()))
    for m in used:
        f, k = int(m["first"]), int(m["count"])
        if f + k <= wn:   # (every record of the model was written)
            lo, hi = extent(xyz[f:f + k])
            assert (m["min"] == lo).all() and (m["max"] == hi).all(), (what, "extent of track", int(m["track_id"]), m["min"], lo, m["max"], hi)
    if not axes:
        assert (models["min"] == wm["min"]).all() and (models["max"] == wm["max"]).all(), (what, "extents against the model")
    if full_models is not None:
        assert models.tobytes() == full_models.tobytes(), (what, "a truncated call's headers differ from the untruncated call's")


# ------------------------------------------------------------------------------------------------------------------ the two calls
class ModelBlocks:
    """caller-owned device blocks for one export, filled with the sentinel -7"""

    def __init__(self, env, B, T, stride):
        self.env, self.B, self.T, self.stride = env, B, T, stride
        self.h_pts = np.full(B * stride * 4 + 4, -7, np.int32); self.h_mod = np.full(B * T * 12 + 4, -7, np.int32); self.h_cnt = np.full(2 * B + 2, -7, np.int32)
        (self.p_pts, self.k_pts), (self.p_mod, self.k_mod), (self.p_cnt, self.k_cnt) = env.upload(self.h_pts), env.upload(self.h_mod), env.upload(self.h_cnt)

    def raw(self, c, batch, flags, points=True, models=True, counts=True, stride=None):
        return c.lib.mot_export_track_models_dev(c._h, batch, flags, C.c_void_p(self.p_pts if points else None), C.c_long(self.stride if stride is None else stride),
                                                 C.c_void_p(self.p_mod if models else None), C.c_void_p(self.p_cnt if counts else None))

    def run(self, c, batch, axes, current):
        c.export_track_models_dev(batch, self.p_pts, self.stride, self.p_mod, self.p_cnt, axes=axes, current=current)
        c.synchronize()
        return self.read(batch)

    def read(self, batch=None):
        batch = self.B if batch is None else batch
        pts = LC.download(self.k_pts, self.h_pts); mod = LC.download(self.k_mod, self.h_mod); cnt = LC.download(self.k_cnt, self.h_cnt)
        self.bytes = (pts.tobytes(), mod.tobytes(), cnt.tobytes())
        assert (pts[batch * self.stride * 4:] == -7).all() and (mod[batch * self.T * 12:] == -7).all() and (cnt[2 * batch:] == -7).all(), "written beyond the batch's blocks"
        models = np.ascontiguousarray(mod[: batch * self.T * 12]).view(self.env.mot.TRACK_MODEL_DTYPE).reshape(batch, self.T)
        return pts[: batch * self.stride * 4].reshape(batch, self.stride, 4), models, cnt[: 2 * batch].reshape(batch, 2)


def check_all(env, c, B, latest, what, flags=FLAGS, stride=None):
    """export and getter of slots 0..B-1 under every flag combination against the model -> {(axes, current): [want of every slot]}"""
    T = c.max_tracks_total
    K = c.track_accumulators_dev()["points_per_track"]
    out = {}
    for axes, current in flags:
        want = [want_slot(env, c, b, axes, current, latest[b]) for b in range(B)]
        blk = ModelBlocks(env, B, T, stride or max(max(w["counts"][1] for w in want), 1))
        p, models, cnt = blk.run(c, B, axes, current)
        for b in range(B):
            w = (what, "axes" if axes else "centred", "current" if current else "all", "slot", b)
            n = want[b]["counts"][1]
            compare(models[b], p[b, :n], cnt[b], want[b], axes, (w, "export"))
            assert (p[b, n:] == -7).all(), (w, "written beyond the slot's records")
            g = c.get_track_models(b, axes=axes, current=current)
            assert g["models"].tobytes() == models[b].tobytes(), (w, "the getter's headers differ from the export's")
            assert len(g["step"]) == n and bits(g["xyz"]).tobytes() == np.ascontiguousarray(p[b, :n, :3]).tobytes() and np.array_equal(g["step"], p[b, :n, 3]), (w, "getter records")
        first = blk.bytes
        blk.run(c, B, axes, current)
        assert blk.bytes == first, (what, axes, current, "two consecutive calls differ")
        out[(axes, current)] = want
    return out


def accumulate(c, B, latest):
    c.accumulate_track_points(B)
    for b in range(B):
        latest[b] += 1


# ------------------------------------------------------------------------------------------------------------------ 1: moving objects
def moving_stream(seed, frames_n=10, speed=0.3):
    """the two-blob stream of track_accum_cases.moving_objects"""
    rng = np.random.default_rng(seed)
    def blob(cx, cy):
        q = np.zeros((200, 4), np.float32); q[:, 0] = cx + rng.uniform(-0.4, 0.4, 200); q[:, 1] = cy + rng.uniform(-0.4, 0.4, 200); q[:, 2] = rng.uniform(-1.0, 0.3, 200); return q
    return [np.concatenate([blob(8.0 + speed * f, 5.0), blob(-9.0, -6.0 - speed * f)]) for f in range(frames_n)]


def run_moving(env, c, K, O, B=3, frames_n=10, between=None):
    streams = [moving_stream(3 + b, frames_n) for b in range(B)]
    c.set_track_links(True); c.set_track_accumulation(K, O)
    latest = [-1] * B
    for f in range(frames_n):
        keep = AC.launch(env, c, [s[f] for s in streams], 2048, f, ego_v=[0.0, 0.0, 1.0][:B], yaw=[0.0, 0.0, 0.05 * f][:B])
        accumulate(c, B, latest)
        if between:
            between(f)
    return latest


def moving_objects(env, oracle, K, O, axes, current):
    """two confirmed tracks per stream over ten frames: (1024, 4) keeps a strict suffix of the ring, (256, 4) and (64, 4) the whole ring, (256, 16) logs nine steps,
    (1024, 1) the latest step alone; the logged yaws turn far enough for the rotation to matter, and track 0's dead row is what MOT_MODEL_CURRENT drops"""
    B = 3
    with env.context(0, max_points=2048, max_batch=B, max_tracks_total=256) as c:
        latest = run_moving(env, c, K, O, B)
        want = check_all(env, c, B, latest, ("moving", K, O), flags=[(axes, current)])[(axes, current)]
        facts = [w["facts"] for w in want]
        assert all(w["counts"][0] >= 2 for w in want), [w["counts"] for w in want]
        assert max(f["sin_max"] for f in facts) > 0.5, "no logged yaw turns far enough for the rotation to be told from the identity"
        if (K, O) == (1024, 4):
            assert all(f["strict_suffix"] >= 2 for f in facts), (facts, "the models do not leave ring points out")
            assert all(0 < n < 1024 for f in facts for n in f["counts"][-2:])
        if (K, O) in ((256, 4), (64, 4)):
            assert all(f["whole_ring"] >= 2 for f in facts), facts
        if (K, O) == (256, 16):
            assert max(max(f["n_obs"]) for f in facts) >= 9, facts
        if current:
            assert all(f["dropped_by_current"] >= 1 for f in facts), (facts, "MOT_MODEL_CURRENT dropped no non-empty row")


def long_log(env, oracle, frames_n=70, K=4096, O=128):
    """a log longer than the transform kernel's tile of OBS_TILE observations in LDS: the kernel walks the log in tiles, each covering a contiguous range of records"""
    with env.context(0, max_points=2048, max_batch=1, max_tracks_total=64) as c:
        c.set_track_links(True); c.set_track_accumulation(K, O)
        latest = [-1]
        for f, x in enumerate(moving_stream(5, frames_n, speed=0.08)):
            keep = AC.launch(env, c, [x], 2048, f, ego_v=[0.0])
            accumulate(c, 1, latest)
        want = check_all(env, c, 1, latest, ("long log", K, O), flags=[(False, False), (True, True)])[(False, False)][0]
        m = want["models"][want["models"]["track_id"] >= 0]
        big = m[m["n_obs"] > OBS_TILE]
        assert len(big) >= 1, (m, "no log longer than one tile")
        for x in big:   # records on both sides of the boundary between the first tile and the second
            steps = want["step"][x["first"]: x["first"] + x["count"]]
            assert x["count"] > TILE and steps.min() < x["first_step"] + OBS_TILE <= steps.max(), (x, steps.min(), steps.max())


# ------------------------------------------------------------------------------------------------------------------ 2: many rows, edges
def many_rows(env, oracle, K, order_any=False):
    """track_point_cases.shape_frames, three frames, 512 track slots, O = 2: packing over many rows with empty rows between non-empty ones, and model sizes on both
    sides of the transform kernel's tile of TILE records"""
    frames = PC.shape_frames(oracle)
    B = len(frames[0])
    with env.context(0, max_points=8192, max_batch=B, max_tracks_total=512) as c:
        c.set_track_links(True); c.set_track_accumulation(K, 2)
        if order_any:
            c.set_point_order(env.mot.MOT_ORDER_ANY)
        latest = [-1] * B
        for f in range(3):
            sent = [np.ascontiguousarray(x[np.random.default_rng(7 + b).permutation(len(x))]) for b, x in enumerate(frames[f])] if order_any else frames[f]
            keep = AC.launch(env, c, sent, 8192, f)
            accumulate(c, B, latest)
        want = check_all(env, c, B, latest, ("many rows", K, order_any))
        w = want[(False, False)]
        assert w[B - 1]["counts"][0] >= 65, ("the longest frame has too few models", w[B - 1]["counts"])
        ids = w[B - 1]["models"]["track_id"]
        used = np.nonzero(ids >= 0)[0]
        assert any((x["models"]["track_id"][: np.nonzero(x["models"]["track_id"] >= 0)[0].max(initial=0)] < 0).any() for x in want[(False, True)]), "no empty model between non-empty ones"
        counts = np.concatenate([x["models"]["count"][x["models"]["track_id"] >= 0] for x in w])
        assert (counts < TILE).any() and (counts > 0).any()
        if K > TILE:
            assert (counts > TILE).any(), ("no model larger than the transform kernel's tile", int(counts.max()))
        else:
            assert counts.max() <= K


# ------------------------------------------------------------------------------------------------------------------ 3: slot reuse
def slot_reuse(env, oracle, T_slots=8):
    """track_accum_cases.reuse_stream: a row that restarted under a new id gives a model of the new track only"""
    frames = AC.reuse_stream()
    reused = 0
    with env.context(0, max_points=1024, max_batch=1, max_tracks_total=T_slots) as c:
        c.set_track_links(True); c.set_track_accumulation(64, 4)
        latest = [-1]
        before = c.get_accum_rows(0)
        for f, x in enumerate(frames):
            keep = AC.launch(env, c, [x], 1024, f, ego_v=[0.0])
            accumulate(c, 1, latest)
            assert not c.get_tracks(0)["capacity_exceeded"], f
            check_all(env, c, 1, latest, ("reuse", f), flags=[(False, False), (True, True)])
            rows = c.get_accum_rows(0)
            g = c.get_track_models(0)
            for r in np.nonzero((before["track_id"] >= 0) & (rows["track_id"] >= 0) & (before["track_id"] != rows["track_id"]))[0]:
                m = g["models"][r]
                assert m["track_id"] == rows["track_id"][r] and m["first_step"] == f and m["last_step"] == f and m["n_obs"] == 1 and m["count"] == rows["total"][r], (f, r, m, rows[r])
                assert (g["step"][m["first"]: m["first"] + m["count"]] == f).all()
                reused += 1
            before = rows
    assert reused, "the script never reused a track slot"


# ------------------------------------------------------------------------------------------------------------------ 4: truncation
def truncation(env, oracle):
    """point_stride cuts in the middle of a model: the first point_stride records, nothing beyond them, true headers and counts, extents over all records"""
    B = 3
    with env.context(0, max_points=2048, max_batch=B, max_tracks_total=256) as c:
        latest = run_moving(env, c, 256, 4, B, frames_n=6)
        for axes, current in ((False, False), (True, True)):
            want = [want_slot(env, c, b, axes, current, latest[b]) for b in range(B)]
            n = [w["counts"][1] for w in want]
            full = ModelBlocks(env, B, 256, max(n)).run(c, B, axes, current)[1]
            used = want[1]["models"][want[1]["models"]["track_id"] >= 0]
            last = used[-1]
            assert len(used) >= 2 and last["count"] > 2
            for stride in (int(last["first"]) + int(last["count"]) // 2, int(used[0]["count"]) // 2, 1, 0):   # inside the last model, inside the first, one record, none
                p, models, cnt = ModelBlocks(env, B, 256, stride).run(c, B, axes, current)
                for b in range(B):
                    wn = min(n[b], stride)
                    compare(models[b], p[b, :wn], cnt[b], want[b], axes, ("truncated", axes, current, stride, b), full_models=full[b])
                    assert (p[b, wn:] == -7).all(), ("truncated", stride, b, "written beyond the slot's records")
            blk = ModelBlocks(env, B, 256, 4)
            assert blk.raw(c, B, flag_bits(env, axes, current), points=False, stride=0) == 0   # no point block at all: headers and extents
            c.synchronize()
            p, models, cnt = blk.read()
            assert (p == -7).all() and models.tobytes() == full.tobytes()


# ------------------------------------------------------------------------------------------------------------------ 5: contract
def code_of(env, fn):
    return AC.code_of(env, fn)


def all_empty(env, c, B, what):
    T = c.max_tracks_total
    for axes, current in FLAGS:
        p, models, cnt = ModelBlocks(env, B, T, 8).run(c, B, axes, current)
        assert (models["track_id"] == -1).all() and not models.tobytes().replace(b"\xff", b"\x00").strip(b"\x00") and (cnt == 0).all() and (p == -7).all(), (what, axes, current)
        for b in range(B):
            g = c.get_track_models(b, axes=axes, current=current)
            assert (g["models"]["track_id"] == -1).all() and len(g["models"]) == T and len(g["step"]) == 0, (what, b)


def contract(env, oracle):
    E = env.mot
    B, T = 2, 64
    clouds = [[CC.small_scene(f, 20), CC.small_scene(f + 5, 12)] for f in range(8)]
    with env.context(0, max_points=4096, max_batch=B, max_tracks_total=T) as c:
        blk = ModelBlocks(env, B, T, 4096)
        nm, npts = C.c_int(-7), C.c_int(-7)
        getter = lambda slot=0, flags=0, models=None, max_models=0, points=None, cap=0, nm_=nm, np_=npts: c.lib.mot_get_track_models(
            c._h, slot, flags, models.ctypes.data_as(C.c_void_p) if models is not None else None, max_models, C.byref(nm_) if nm_ is not None else None,
            points.ctypes.data_as(C.c_void_p) if points is not None else None, cap, C.byref(np_) if np_ is not None else None)
        # the feature off; on without a log
        c.set_track_links(True)
        assert blk.raw(c, B, 0) == E.MOT_E_STATE and getter() == E.MOT_E_STATE, "accumulation off"
        c.set_track_accumulation(64, 0)
        assert blk.raw(c, B, 0) == E.MOT_E_STATE and getter() == E.MOT_E_STATE, "obs_per_track 0"
        c.set_track_accumulation(64, 4)
        all_empty(env, c, B, "before the first accumulate")
        # arguments, on a context whose state would serve the call
        for flags in (4, 8, 1 << 30, -1):
            assert blk.raw(c, B, flags) == E.MOT_E_ARG and getter(flags=flags) == E.MOT_E_ARG, flags
        assert blk.raw(c, 0, 0) == E.MOT_E_ARG and blk.raw(c, B + 1, 0) == E.MOT_E_ARG and blk.raw(c, -1, 0) == E.MOT_E_ARG
        assert blk.raw(c, B, 0, models=False) == E.MOT_E_ARG and blk.raw(c, B, 0, counts=False) == E.MOT_E_ARG and blk.raw(c, B, 0, points=False) == E.MOT_E_ARG
        assert blk.raw(c, B, 0, stride=-1) == E.MOT_E_ARG
        assert getter(slot=B) == E.MOT_E_ARG and getter(slot=-1) == E.MOT_E_ARG and getter(max_models=-1) == E.MOT_E_ARG and getter(cap=-1) == E.MOT_E_ARG
        assert getter(np_=None) == E.MOT_E_ARG and getter(nm_=None) == E.MOT_E_ARG
        p, models, cnt = blk.read()
        assert (p == -7).all() and (blk.h_mod == -7).all() and (cnt == -7).all(), "a refused call wrote into the caller's blocks"
        latest = [-1] * B
        for f in range(3):
            keep = AC.launch(env, c, clouds[f], 4096, f)
            accumulate(c, B, latest)
        want = check_all(env, c, B, latest, "contract")[(False, False)]
        n = want[1]["counts"][1]
        assert n > 1
        # buffers too small: the counts, nothing copied
        for max_models, cap in ((T - 1, n), (T, n - 1)):
            mod = np.full(T * 12, -7, np.int32); pts = np.full(n * 4, -7, np.int32); nm.value = npts.value = -7
            assert getter(1, 0, mod, max_models, pts, cap) == E.MOT_E_CAPACITY and (nm.value, npts.value) == (T, n), (max_models, cap)
            assert (mod == -7).all() and (pts == -7).all(), "a refused getter wrote"
        mod = np.full(T * 12 + 4, -7, np.int32); pts = np.full(n * 4 + 4, -7, np.int32)
        assert getter(1, 0, mod, T, pts, n) == 0 and (mod[T * 12:] == -7).all() and (pts[n * 4:] == -7).all() and mod[: T * 12].tobytes() == c.get_track_models(1)["models"].tobytes()
        nm.value = npts.value = -7
        assert getter(1) == 0 and (nm.value, npts.value) == (T, n), "null buffers: the counts alone"
        # a stage-wise call takes slot 0: the accumulators, and so the models, are what they were
        first = ModelBlocks(env, B, T, 4096); first.run(c, B, True, False)
        keep = AC.launch(env, c, clouds[3], 4096, 3)
        c.cluster(c.get_ground(0, n_hint=len(clouds[3][0]))["elevated"])
        assert code_of(env, lambda: c.accumulate_track_points(B)) == E.MOT_E_STATE
        again = ModelBlocks(env, B, T, 4096); again.run(c, B, True, False)
        assert again.bytes == first.bytes, "the models changed although nothing was accumulated"
        check_all(env, c, B, latest, "after a stage-wise call took slot 0")
        # the resets
        c.reset_slot(1)
        g0, g1 = c.get_track_models(0), c.get_track_models(1)
        assert (g1["models"]["track_id"] == -1).all() and len(g1["step"]) == 0 and (g0["models"]["track_id"] >= 0).any(), "reset_slot"
        c.reset_tracks_slot(0)
        all_empty(env, c, B, "reset_slot and reset_tracks_slot")
        latest = [-1] * B
        for f in range(4, 6):
            keep = AC.launch(env, c, clouds[f], 4096, f)
            accumulate(c, B, latest)
        want = check_all(env, c, B, latest, "after the resets")[(False, False)]
        assert all(w["counts"][0] > 0 for w in want)
        c.reset()
        all_empty(env, c, B, "reset")
        c.set_track_accumulation(0, 0)
        assert blk.raw(c, B, 0) == E.MOT_E_STATE and getter() == E.MOT_E_STATE, "off again"


# ------------------------------------------------------------------------------------------------------------------ 6: non-finite pose
def poke(env, ptr, data):
    """bytes to a device address of the zero-copy view"""
    if env.lib_path is not None:
        C.memmove(ptr, data.ctypes.data, data.nbytes)
    else:
        import hiprt
        assert hiprt.hip().hipMemcpy(C.c_void_p(ptr), data.ctypes.data_as(C.c_void_p), C.c_size_t(data.nbytes), 1) == 0


def non_finite_pose(env, oracle):
    """one logged observation's px overwritten with NaN: that step's records are NaN in x' (with AXES in y' too) and still written, the extent is that of the other
    records, every other model keeps its bytes"""
    B, T, K, O = 3, 256, 256, 4
    with env.context(0, max_points=2048, max_batch=B, max_tracks_total=T) as c:
        latest = run_moving(env, c, K, O, B, frames_n=6)
        c.synchronize()
        v = c.track_accumulators_dev()
        rows = c.get_accum_rows(1)
        r = int(np.argmax(rows["total"]))
        assert rows["obs_total"][r] >= O
        pos = (int(rows["obs_total"][r]) - 2) & (O - 1)   # the observation before the latest
        at = 1 * T + r
        obs = AC.peek(env, c, v["d_obs"] + (at * O + pos) * 48, env.mot.ACCUM_OBS_DTYPE, 1)
        step = int(obs["step"][0])
        for axes in (False, True):
            blk = ModelBlocks(env, B, T, 2048)
            p0, m0, cnt0 = blk.run(c, B, axes, False)
            poke(env, v["d_obs"] + (at * O + pos) * 48 + 16, np.array([np.nan], np.float32))
            want = check_all(env, c, B, latest, ("NaN px", axes), flags=[(axes, False)])[(axes, False)]
            p1, m1, cnt1 = blk.run(c, B, axes, False)
            m = m1[1, r]
            seg = slice(int(m["first"]), int(m["first"]) + int(m["count"]))
            xyz = np.ascontiguousarray(p1[1, seg, :3]).view(np.float32); hit = p1[1, seg, 3] == step
            assert 0 < hit.sum() < len(hit) and np.isnan(xyz[hit, 0]).all() and not np.isnan(xyz[~hit]).any() and (np.isnan(xyz[hit, 1]).all() if axes else not np.isnan(xyz[hit, 1]).any())
            lo, hi = extent(xyz[~hit])
            assert (m["min"] == lo).all() and (m["max"] == hi).all(), (m, lo, hi)
            keep = np.ones((B, T), bool); keep[1, r] = False
            assert m1[keep].tobytes() == m0[keep].tobytes() and np.array_equal(cnt0, cnt1), "another model's header changed"
            other = np.ones(p1.shape[1], bool); other[seg] = False
            assert np.array_equal(p1[1, other], p0[1, other]) and np.array_equal(p1[0], p0[0]) and np.array_equal(p1[2], p0[2]), "another model's records changed"
            assert np.array_equal(p1[1, seg][~hit], p0[1, seg][~hit])
            poke(env, v["d_obs"] + (at * O + pos) * 48 + 16, obs["px"].astype(np.float32))   # (back: the next flag starts from the same log)
        # every pose of the row NaN: no finite record, the extent is all 0
        for k in range(O):
            poke(env, v["d_obs"] + (at * O + k) * 48 + 16, np.array([np.nan], np.float32))
        g = c.get_track_models(1)
        m = g["models"][r]
        assert m["count"] > 0 and (m["min"] == 0).all() and (m["max"] == 0).all() and np.isnan(g["xyz"][m["first"]: m["first"] + m["count"], 0]).all()


# ------------------------------------------------------------------------------------------------------------------ 7: non-interference
def accumulators(env, c, B):
    """rows, rings and logs of slots 0..B-1 as the device view holds them: what the model calls must not touch. Of the rings only what the rows define is
    compared across contexts (the rest is whatever the context's memory held)"""
    v = c.track_accumulators_dev()
    T, K, O = v["tracks_per_slot"], v["points_per_track"], v["obs_per_track"]
    out = []
    for b in range(B):
        rows = c.get_accum_rows(b)
        out.append(("rows", rows.tobytes()))
        for r in np.nonzero(rows["track_id"] >= 0)[0]:
            g = c.get_track_accumulated(b, int(rows["track_id"][r]))
            out += [("ring", g["xyz"].tobytes() + g["step"].tobytes()), ("log", g["obs"].tobytes())]
    raw = [AC.peek(env, c, v["d_rows"], np.uint8, B * T * 32).tobytes(), AC.peek(env, c, v["d_points"], np.uint8, B * T * K * 16).tobytes(),
           AC.peek(env, c, v["d_obs"], np.uint8, B * T * O * 48).tobytes()]
    return out, raw


def non_interference(env, oracle, graphs=False):
    """model calls interleaved with the steps: rows, rings and logs, and every getter of the fused step, are byte-identical to a run without them"""
    B, T = 2, 256
    clouds = [[CC.small_scene(f, 20), CC.small_scene(f + 5, 12)] for f in range(4)]
    res = {}
    for tag in ("never", "models"):
        with env.context(0, max_points=4096, max_batch=B, max_tracks_total=T) as c:
            c.set_launch_graphs(graphs); c.set_track_links(True); c.set_track_accumulation(256, 4)
            blk = ModelBlocks(env, B, T, 4096)
            out = []
            for f in range(4):
                keep = PC.launch(env, c, clouds[f], 4096, f, yaw=0.02 * f)
                n_points = [len(x) for x in clouds[f]]
                if tag == "models":   # between the fused step and its accumulate
                    blk.run(c, B, True, True); c.get_track_models(1, axes=True)
                c.accumulate_track_points(B)
                before = PC.readout(c, B, n_points)
                acc, raw = accumulators(env, c, B)
                if tag == "models":
                    for axes, current in FLAGS:
                        p, models, cnt = blk.run(c, B, axes, current)
                        assert cnt[1, 1] > 0 or f == 0
                        c.get_track_models(0, axes=axes, current=current)
                    PC.equal_readouts(PC.readout(c, B, n_points), before, (f, "after the model calls"))   # (one context: every byte)
                    acc2, raw2 = accumulators(env, c, B)
                    assert acc2 == acc and raw2 == raw, (f, "the model calls wrote into the accumulators")
                exports = [(fr + k, np.ascontiguousarray(x).tobytes()) for fr in ("sensor", "global") for b in range(B) for k, x in sorted(c.get_track_points(b, rest=True, frame=fr).items())]
                out.append((AC.defined_items(before) + exports, acc))
            res[tag] = out
    for f in range(4):
        PC.equal_readouts(res["models"][f][0], res["never"][f][0], (f, "against a context that never asked for models"))
        assert res["models"][f][1] == res["never"][f][1], (f, "accumulators against a context that never asked for models")


# ------------------------------------------------------------------------------------------------------------------ 8: emulator only
def launches_and_allocations(env, oracle):
    """the launch counters of the two new kernels move in the two new calls and nowhere else; the setter allocates its four tables and nothing for the models, the
    first model call allocates, turning accumulation off gives everything back"""
    lib = env.mot.load_library(env.lib_path)
    lib.hipemu_live_allocs.restype = C.c_long
    count = lambda: [lib.hipemu_launch_count(k) for k in KERNELS]
    B, T = 2, 64
    with env.context(0, max_points=4096, max_batch=B, max_tracks_total=T) as c:
        before = count()
        c.set_track_links(True)
        keep = PC.launch(env, c, [CC.small_scene(0, 20), CC.small_scene(5, 12)], 4096, 0)
        c.get_track_points(1, frame="global")   # (the scratch the accumulate call shares with the per-track point clouds exists from here on)
        allocs = lib.hipemu_live_allocs()
        blk = ModelBlocks(env, B, T, 4096)
        assert blk.raw(c, B, 0) == env.mot.MOT_E_STATE and lib.hipemu_live_allocs() == allocs
        c.set_track_accumulation(64, 4)
        assert lib.hipemu_live_allocs() == allocs + 4, "the setter allocates its four tables, nothing for the models"
        for f in range(1, 4):
            keep = PC.launch(env, c, [CC.small_scene(f, 20), CC.small_scene(f + 5, 12)], 4096, f)
            c.accumulate_track_points(B)
            for b in range(B):
                c.get_point_tracks(b); c.get_box_tracks(b); c.get_boxes(b); c.get_tracks(b); c.get_track_points(b, frame="global"); c.get_accum_rows(b)
            c.track_accumulators_dev(); c.get_track_accumulated(1, int(c.get_accum_rows(1)["track_id"].max()))
        assert count() == before, "a new kernel ran outside the two new calls"
        assert lib.hipemu_live_allocs() == allocs + 4, "something was allocated for the models before the first model call"
        for flags in (4, -1):
            assert blk.raw(c, B, flags) == env.mot.MOT_E_ARG
        assert count() == before and lib.hipemu_live_allocs() == allocs + 4
        blk.run(c, B, False, False)
        assert count() == [n + 1 for n in before]
        with_export = lib.hipemu_live_allocs()
        assert with_export > allocs + 4
        blk.run(c, B, True, True)
        assert count() == [n + 2 for n in before] and lib.hipemu_live_allocs() == with_export
        n, npts = C.c_int(0), C.c_int(0)
        assert c.lib.mot_get_track_models(c._h, 1, 0, None, 0, C.byref(n), None, 0, C.byref(npts)) == 0 and npts.value > 0
        assert count() == [n + 3 for n in before]
        c.get_track_models(1)   # (two calls of the C getter: the counts, then the records)
        assert count() == [n + 5 for n in before]
        with_getter = lib.hipemu_live_allocs()
        assert with_getter > with_export
        c.get_track_models(0, axes=True); blk.run(c, B, False, True)
        assert lib.hipemu_live_allocs() == with_getter
        now = count()
        c.reset_slot(0); c.reset()
        keep = PC.launch(env, c, [CC.small_scene(4, 20), CC.small_scene(9, 12)], 4096, 4)
        c.accumulate_track_points(B)
        assert count() == now
        c.set_track_accumulation(128, 4)   # another geometry: the models' blocks go with the old tables
        assert lib.hipemu_live_allocs() == allocs + 4
        blk.run(c, B, False, False); c.get_track_models(0)
        c.set_track_accumulation(0, 0)
        assert lib.hipemu_live_allocs() == allocs, "turning accumulation off did not free the models' memory"


def first_call_under_allocation_failure(env, oracle):
    """each allocation of the first model calls failing in turn: MOT_E_HIP, the accumulators as they were, and the next call resumes"""
    lib = env.mot.load_library(env.lib_path)
    lib.hipemu_live_allocs.restype = C.c_long
    lib.hipemu_fail_alloc_at.argtypes = [C.c_long]; lib.hipemu_fail_alloc_at.restype = None
    E = env.mot
    B, T = 2, 64
    try:
        with env.context(0, max_points=4096, max_batch=B, max_tracks_total=T) as c:
            c.set_track_links(True); c.set_track_accumulation(64, 4)
            latest = [-1] * B
            keep = AC.launch(env, c, [CC.small_scene(0, 20), CC.small_scene(5, 12)], 4096, 0)
            accumulate(c, B, latest)
            acc = accumulators(env, c, B)
            blk = ModelBlocks(env, B, T, 4096)
            for who, call, least in (("export", lambda: blk.raw(c, B, 0), 3), ("getter", lambda: code_of(env, lambda: c.get_track_models(1)), 2)):
                failed = 0   # (export: device block, page-locked ring, the ring's events; getter: its two staging blocks)
                for k in range(1, 40):
                    lib.hipemu_fail_alloc_at(k)
                    rc = call()
                    lib.hipemu_fail_alloc_at(0)
                    if rc == 0:
                        break
                    assert rc == E.MOT_E_HIP, (who, k, rc)
                    failed += 1
                    assert accumulators(env, c, B) == acc, (who, k, "a failed model call changed the accumulators")
                assert failed >= least, (who, failed)
            check_all(env, c, B, latest, "after the failed allocations")
    finally:
        lib.hipemu_fail_alloc_at(0)
