"""Voxel-thinned object models (mot_export_track_model_voxels_dev / mot_get_track_model_voxels, csrc/track_voxels.hip): bodies shared by
tests/test_emu_track_voxels.py (emulator) and tests/test_track_voxels_gpu.py (MI355X). The callers supply a capacity_cases.Env.

The expectation is numpy and shares no code with the kernels: per slot, Context.get_track_models under the same flags — it exists without the feature and is pinned by
its own tests — gives the raw records and headers, and the definition of include/mot.h is applied to those bits: inv = 1 / leaf in fp32, one fp32 product, the range
test on the floats, np.floor, np.unique over the (i_z, i_y, i_x) keys, the counts, and every voxel's exact mean in integer fractions, rounded correctly to fp32.

Compared exactly: every integer header field, n_records == the raw count, n_outside, n_sparse, the raw extents, first / count packing, the two counts per slot, the
voxel order (strictly ascending key when the cells are recomputed from the returned centroids), every voxel's count, sum(count) + dropped records == n_records -
n_outside. Centroids: within 1 fp32 ulp of the correctly rounded exact mean — all members of a cell share a sign per axis (no cancellation), an fp64 sum of at most
4096 terms in any order is relatively wrong by less than 2^-40, so the rounded result is the correctly rounded mean or, at a near-tie, its neighbour — and within
[min, max] of the members per axis, hence in the voxel's own cell."""
import ctypes as C
from fractions import Fraction

import numpy as np

import capacity_cases as CC
import track_accum_cases as AC
import track_accum_seq_cases as SC
import track_link_cases as LC
import track_model_cases as MC
import track_point_cases as PC

KERNELS = (b"track_voxels_count_kernel", b"track_voxels_pack_kernel", b"track_voxels_write_kernel")
FLAGS = MC.FLAGS
LEAVES = (0.1, 0.25, (0.3, 0.2, 0.05))
MAX_K = 4096
RAW_FIELDS = ("track_id", "n_obs", "first_step", "last_step")


def leaf3(leaf):
    return np.array([leaf] * 3 if np.isscalar(leaf) else leaf, np.float32)


def cells_of(xyz, leaf):
    """(takes part [n], key [n] of those that do) by the definition: fp32 inverse, fp32 product, the range test on the floats, floor"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    inv = np.float32(1.0) / leaf3(leaf)
    assert inv.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        t = xyz * inv[None, :]
        assert t.dtype == np.float32
        lim = np.array([1024, 1024, 512], np.float32)
        part = np.isfinite(xyz).all(1) & (t >= -lim).all(1) & (t < lim).all(1)
    i = np.floor(t[part]).astype(np.int64)
    return part, ((i[:, 2] + 512) << 22) | ((i[:, 1] + 1024) << 11) | (i[:, 0] + 1024), i


def round_f32(q):
    """the fp32 value nearest to the fraction q (ties cannot be told from near-ties by the caller's bound: either neighbour passes it)"""
    c = np.float32(float(q))
    best = c
    for other in (np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))):
        if abs(Fraction(float(other)) - q) < abs(Fraction(float(best)) - q):
            best = other
    return best


def want_slot(env, c, b, leaf, min_points, axes, current):
    """slot b's voxel models by the definition, from the raw models the library gives under the same flags"""
    g = c.get_track_models(b, axes=axes, current=current)
    raw, xyz = g["models"], np.ascontiguousarray(g["xyz"], np.float32)
    T = len(raw)
    models = np.zeros(T, env.mot.VOXEL_MODEL_DTYPE); models["track_id"] = -1
    vox_xyz, vox_lo, vox_hi, vox_cnt, vox_key = [], [], [], [], []
    facts = dict(neg_xy=False, occupied=[], idx=[])
    first = 0
    for r in np.nonzero(raw["track_id"] >= 0)[0]:
        m = raw[r]
        p = xyz[int(m["first"]): int(m["first"]) + int(m["count"])]
        part, key, idx = cells_of(p, leaf)
        facts["neg_xy"] |= bool(((idx[:, 0] < 0) & (idx[:, 1] < 0)).any()) if len(idx) else False
        q = p[part]
        uniq, inverse, cnt = np.unique(key, return_inverse=True, return_counts=True)
        keep = cnt >= min_points
        order = np.argsort(inverse, kind="stable"); starts = np.concatenate([[0], np.cumsum(cnt)])
        for k in np.nonzero(keep)[0]:
            mem = q[order[starts[k]: starts[k + 1]]]
            n = len(mem)
            vox_xyz.append([round_f32(sum(map(Fraction, mem[:, a].tolist())) / n) for a in range(3)])
            vox_lo.append(mem.min(0)); vox_hi.append(mem.max(0)); vox_cnt.append(n); vox_key.append(int(uniq[k]))
        w = models[r]
        for f in RAW_FIELDS:
            w[f] = m[f]
        w["first"], w["count"], w["min"], w["max"] = first, int(keep.sum()), m["min"], m["max"]
        w["n_records"], w["n_outside"], w["n_sparse"] = m["count"], int((~part).sum()), int((~keep).sum())
        facts["occupied"].append(len(uniq))
        first += int(keep.sum())
    arr = lambda x, dt, shape: np.array(x, dt).reshape(shape)
    return dict(models=models, raw=raw, counts=(int((models["track_id"] >= 0).sum()), first), xyz=arr(vox_xyz, np.float32, (-1, 3)), lo=arr(vox_lo, np.float32, (-1, 3)),
                hi=arr(vox_hi, np.float32, (-1, 3)), count=arr(vox_cnt, np.int32, (-1,)), key=arr(vox_key, np.int64, (-1,)), facts=facts)


def compare(models, vox, counts, want, leaf, what, full_models=None):
    """one slot of a call against the expectation. vox: the int32 [n_written, 4] voxels the call wrote (all of them, or the first voxel_stride)"""
    wm = want["models"]
    for f in wm.dtype.names:
        if f not in ("min", "max"):
            assert np.array_equal(models[f], wm[f]), (what, f, models[f][models[f] != wm[f]][:8], wm[f][models[f] != wm[f]][:8])
    assert models["min"].tobytes() == want["raw"]["min"].tobytes() and models["max"].tobytes() == want["raw"]["max"].tobytes(), (what, "the raw extents")
    assert np.array_equal(models["n_records"], np.where(want["raw"]["track_id"] >= 0, want["raw"]["count"], 0)), (what, "n_records against the raw count")
    assert tuple(int(x) for x in counts) == want["counts"], (what, "counts", tuple(counts), want["counts"])
    used = models[models["track_id"] >= 0]
    assert np.array_equal(used["first"], np.concatenate([[0], np.cumsum(used["count"])[:-1]])[: len(used)]), (what, "packing")
    empty = models[models["track_id"] < 0]
    assert not empty.tobytes().replace(b"\xff", b"\x00").strip(b"\x00"), (what, "an empty model is not {-1, 0, ...}")
    assert (models["reserved"] == 0).all()
    wn = len(vox)
    assert wn <= want["counts"][1]
    xyz = np.ascontiguousarray(vox[:, :3]).view(np.float32).reshape(-1, 3)
    assert np.array_equal(vox[:, 3], want["count"][:wn]), (what, "voxel counts")
    part, key, _ = cells_of(xyz, leaf)
    assert part.all() and np.array_equal(key, want["key"][:wn]), (what, "the cells of the returned centroids are not the voxels' own")
    for m in used:
        f, k = int(m["first"]), int(m["count"])
        if f + k <= wn:   # (every voxel of the model was written)
            assert (np.diff(key[f: f + k]) > 0).all(), (what, "voxel order", int(m["track_id"]))
            dropped = int(m["n_records"]) - int(m["n_outside"]) - int(vox[f: f + k, 3].sum())
            assert dropped >= 0 and (dropped == 0) == (m["n_sparse"] == 0), (what, "sum(count) + dropped == n_records - n_outside", m)
    assert (xyz >= want["lo"][:wn]).all() and (xyz <= want["hi"][:wn]).all(), (what, "a centroid outside [min, max] of its members")
    ulps = np.abs(xyz.astype(np.float64) - want["xyz"][:wn].astype(np.float64)) / np.spacing(np.abs(want["xyz"][:wn])).astype(np.float64)
    assert (ulps <= 1).all(), (what, "centroid beyond 1 ulp of the correctly rounded mean", float(ulps.max()))
    if full_models is not None:
        assert models.tobytes() == full_models.tobytes(), (what, "a truncated call's headers differ from the untruncated call's")


# ------------------------------------------------------------------------------------------------------------------ the two calls
class VoxelBlocks:
    """caller-owned device blocks for one export, filled with the sentinel -7"""

    def __init__(self, env, B, T, stride):
        self.env, self.B, self.T, self.stride = env, B, T, stride
        self.h_vox = np.full(B * stride * 4 + 4, -7, np.int32); self.h_mod = np.full(B * T * 16 + 4, -7, np.int32); self.h_cnt = np.full(2 * B + 2, -7, np.int32)
        (self.p_vox, self.k_vox), (self.p_mod, self.k_mod), (self.p_cnt, self.k_cnt) = env.upload(self.h_vox), env.upload(self.h_mod), env.upload(self.h_cnt)

    def raw(self, c, batch, flags, leaf=0.1, min_points=1, voxels=True, models=True, counts=True, stride=None, params=True):
        p = self.env.mot.voxel_params(leaf, 1); p.min_points = min_points
        return c.lib.mot_export_track_model_voxels_dev(c._h, batch, flags, C.byref(p) if params else None, C.c_void_p(self.p_vox if voxels else None),
                                                       C.c_long(self.stride if stride is None else stride), C.c_void_p(self.p_mod if models else None),
                                                       C.c_void_p(self.p_cnt if counts else None))

    def run(self, c, batch, leaf, min_points, axes, current):
        c.export_track_model_voxels_dev(batch, self.p_vox if self.stride else 0, self.stride, self.p_mod, self.p_cnt, leaf, min_points, axes=axes, current=current)
        c.synchronize()
        return self.read(batch)

    def read(self, batch=None):
        batch = self.B if batch is None else batch
        vox, mod, cnt = (LC.download(k, h).copy() for k, h in ((self.k_vox, self.h_vox), (self.k_mod, self.h_mod), (self.k_cnt, self.h_cnt)))   # (the emulator's blocks ARE the host arrays)
        self.bytes = (vox.tobytes(), mod.tobytes(), cnt.tobytes())
        assert (vox[batch * self.stride * 4:] == -7).all() and (mod[batch * self.T * 16:] == -7).all() and (cnt[2 * batch:] == -7).all(), "written beyond the batch's blocks"
        models = np.ascontiguousarray(mod[: batch * self.T * 16]).view(self.env.mot.VOXEL_MODEL_DTYPE).reshape(batch, self.T)
        return vox[: batch * self.stride * 4].reshape(batch, self.stride, 4), models, cnt[: 2 * batch].reshape(batch, 2)


def check_all(env, c, B, leaf, what, min_points=1, flags=FLAGS):
    """export and getter of slots 0..B-1 under the flag combinations against the expectation, twice -> {(axes, current): [want of every slot]}"""
    T = c.max_tracks_total
    out = {}
    for axes, current in flags:
        want = [want_slot(env, c, b, leaf, min_points, axes, current) for b in range(B)]
        blk = VoxelBlocks(env, B, T, max(max(w["counts"][1] for w in want), 1))
        v, models, cnt = blk.run(c, B, leaf, min_points, axes, current)
        for b in range(B):
            w = (what, leaf, min_points, "axes" if axes else "centred", "current" if current else "all", "slot", b)
            n = want[b]["counts"][1]
            compare(models[b], v[b, :n], cnt[b], want[b], leaf, (w, "export"))
            assert (v[b, n:] == -7).all(), (w, "written beyond the slot's voxels")
            g = c.get_track_model_voxels(b, leaf, min_points, axes=axes, current=current)
            assert g["models"].tobytes() == models[b].tobytes(), (w, "the getter's headers differ from the export's")
            assert len(g["count"]) == n and MC.bits(g["xyz"]).tobytes() == np.ascontiguousarray(v[b, :n, :3]).tobytes() and np.array_equal(g["count"], v[b, :n, 3]), (w, "getter voxels")
        first = blk.bytes
        blk.run(c, B, leaf, min_points, axes, current)
        assert blk.bytes == first, (what, axes, current, "two consecutive calls differ")
        out[(axes, current)] = want
    return out


def used_models(want):
    return [m for w in want for m in w["models"][w["models"]["track_id"] >= 0]]


# ------------------------------------------------------------------------------------------------------------------ 1: moving objects
def moving_objects(env, oracle, K, O, axes, current):
    """track_model_cases' two moving blobs per stream, ten frames, under the three leaves: voxels that hold several records, models thinner than their records, cells
    with negative indices on both axes (the lattice is centred on the object)"""
    B = 3
    with env.context(0, max_points=2048, max_batch=B, max_tracks_total=256) as c:
        MC.run_moving(env, c, K, O, B)
        for leaf in LEAVES:
            want = check_all(env, c, B, leaf, ("moving", K, O), flags=[(axes, current)])[(axes, current)]
            used = used_models(want)
            assert len(used) >= 2 * B, len(used)
            assert max(int(w["count"].max(initial=0)) for w in want) >= 2, (leaf, "no voxel holds two records")
            assert any(m["count"] < m["n_records"] for m in used), (leaf, "no model has fewer voxels than records")
            assert any(w["facts"]["neg_xy"] for w in want), (leaf, "no cell with negative indices on both axes")


# ------------------------------------------------------------------------------------------------------------------ 2, 3: the two ends of the leaf range
def low_stream(seed, frames_n=6, speed=0.3):
    """track_model_cases.moving_stream with every point below the sensor: one sign in z"""
    rng = np.random.default_rng(seed)
    def blob(cx, cy):
        q = np.zeros((200, 4), np.float32); q[:, 0] = cx + rng.uniform(-0.4, 0.4, 200); q[:, 1] = cy + rng.uniform(-0.4, 0.4, 200); q[:, 2] = rng.uniform(-1.0, -0.1, 200); return q
    return [np.concatenate([blob(8.0 + speed * f, 5.0), blob(-9.0, -6.0 - speed * f)]) for f in range(frames_n)]


def shift_logged_positions(env, c, B, by):
    """every logged px, py of slots 0..B-1 moved by `by`, in the zero-copy view: the models' records then lie in one quadrant of the object's frame"""
    v = c.track_accumulators_dev()
    n = B * v["tracks_per_slot"] * v["obs_per_track"]
    obs = AC.peek(env, c, v["d_obs"], env.mot.ACCUM_OBS_DTYPE, n)
    obs["px"] += np.float32(by); obs["py"] += np.float32(by)
    MC.poke(env, v["d_obs"], obs)


def one_voxel_per_model(env, oracle, K=256, O=4):
    """leaf 1000 and records of one sign per axis: a model is ONE run as long as the model — the long-run path of the sums"""
    B = 2
    streams = [low_stream(3 + b) for b in range(B)]
    with env.context(0, max_points=2048, max_batch=B, max_tracks_total=64) as c:
        c.set_track_links(True); c.set_track_accumulation(K, O)
        latest = [-1] * B
        for f in range(len(streams[0])):
            keep = AC.launch(env, c, [s[f] for s in streams], 2048, f, ego_v=[0.0] * B)
            MC.accumulate(c, B, latest)
        shift_logged_positions(env, c, B, -10.0)
        want = check_all(env, c, B, 1000.0, "one voxel", flags=[(False, False), (True, True)])[(False, False)]
        hit = [m for m in used_models(want) if m["count"] == 1 and m["n_sparse"] == 0 and m["n_outside"] == 0 and m["n_records"] >= 64]
        assert hit, ([m for m in used_models(want)], "no model of one voxel that holds all its records")
        assert any(int(w["count"].max(initial=0)) >= 64 for w in want)
        assert max(m["n_records"] for m in hit) == K, "no full ring in one voxel"


def every_record_alone(env, oracle, K=256, O=4):
    """leaf 1e-3: the lattice ends 1.024 / 0.512 from the object, records beyond it take no part, and the others sit alone in their voxels"""
    B = 2
    with env.context(0, max_points=2048, max_batch=B, max_tracks_total=64) as c:
        MC.run_moving(env, c, K, O, B, frames_n=6)
        want = check_all(env, c, B, 1e-3, "alone", flags=[(False, False), (True, False)])[(False, False)]
        used = used_models(want)
        assert any(m["n_outside"] > 0 for m in used), "no record off the lattice"
        assert any(m["count"] > 0 and m["count"] == m["n_records"] - m["n_outside"] for m in used), "no model whose voxels all hold one record"
        check_all(env, c, B, 1e-3, "alone, two per voxel", min_points=2, flags=[(False, False)])


# ------------------------------------------------------------------------------------------------------------------ 4: sort sizes
def set_model_count(env, c, b, r, n):
    """row r of slot b keeps its ring and log, but only its last n kept records still have a logged step: the others are stamped one step before the oldest logged
    observation (steps stay non-decreasing along the unrolled ring), written in the zero-copy view"""
    E = env.mot
    v = c.track_accumulators_dev()
    T, K, O = v["tracks_per_slot"], v["points_per_track"], v["obs_per_track"]
    row = c.get_accum_rows(b)[r]
    at = b * T + r
    kept = min(int(row["total"]), K); ring0 = int(row["total"]) & (K - 1) if int(row["total"]) > K else 0
    n_obs = min(int(row["obs_total"]), O); obs0 = int(row["obs_total"]) & (O - 1) if int(row["obs_total"]) > O else 0
    assert 0 <= n <= kept and n_obs >= 1
    obs = AC.peek(env, c, v["d_obs"] + at * O * 48, E.ACCUM_OBS_DTYPE, O)
    oldest = int(obs["step"][obs0])
    ring = AC.peek(env, c, v["d_points"] + at * K * 16, E.ACCUM_POINT_DTYPE, K)
    pos = (ring0 + np.arange(kept)) & (K - 1)
    assert (ring["step"][pos] >= oldest).all(), "the scene's rows keep every ring point in their model"
    ring["step"][pos[: kept - n]] = oldest - 1
    MC.poke(env, v["d_points"] + at * K * 16, ring)


def sort_sizes(env, oracle, K):
    """models of 0, 1, 63, 64, 65, K - 1 and K records (65 only where K holds it): the sizes on both sides of the sort network's smallest size, one wave, and the
    whole of LDS. The scene fills eight rings (two tracks in each of four streams, points per object and steps chosen to fill K); the exact counts are then set by
    restamping the oldest records of a row in the zero-copy view, which is how a log that has moved on leaves a ring"""
    B, O = 4, 16
    per = 200 if K == 64 else 900
    rng = np.random.default_rng(11)
    def blob(cx, cy):
        q = np.zeros((per, 4), np.float32); q[:, 0] = cx + rng.uniform(-0.4, 0.4, per); q[:, 1] = cy + rng.uniform(-0.4, 0.4, per); q[:, 2] = rng.uniform(-1.0, 0.3, per); return q
    frames_n = 9
    streams = [[np.concatenate([blob(8.0 + 0.3 * f, 5.0 + b), blob(-9.0, -6.0 - 0.3 * f - b)]) for f in range(frames_n)] for b in range(B)]
    targets = sorted({0, 1, 63, 64, 65, K - 1, K} - ({65} if K < 65 else set()), reverse=True)
    with env.context(0, max_points=2048, max_batch=B, max_tracks_total=64) as c:
        c.set_track_links(True); c.set_track_accumulation(K, O)
        latest = [-1] * B
        for f in range(frames_n):
            keep = AC.launch(env, c, [s[f] for s in streams], 2048, f, ego_v=[0.0] * B)
            MC.accumulate(c, B, latest)
        full = [(b, int(r)) for b in range(B) for r in np.nonzero((c.get_accum_rows(b)["track_id"] >= 0) & (c.get_accum_rows(b)["total"] >= K))[0]]
        assert len(full) >= len(targets), (len(full), "too few full rings")
        for (b, r), n in zip(full, targets):
            set_model_count(env, c, b, r, n)
        for leaf in (0.1, 1000.0):
            want = check_all(env, c, B, leaf, ("sort sizes", K), flags=[(False, False), (True, False)])[(False, False)]
            got = sorted({int(m["n_records"]) for m in used_models(want)}, reverse=True)
            assert set(targets) <= set(got), (targets, got)
            zero = [m for m in used_models(want) if m["n_records"] == 0]
            assert zero and all(m["count"] == 0 and m["n_obs"] >= 1 for m in zero), "no model with a logged observation and no record"


# ------------------------------------------------------------------------------------------------------------------ 5: min_points
def min_points(env, oracle):
    """1, 2 and 4096: at 4096 every voxel is dropped, the models stay, and n_sparse is what was occupied"""
    B = 2
    with env.context(0, max_points=2048, max_batch=B, max_tracks_total=64) as c:
        MC.run_moving(env, c, 256, 4, B, frames_n=6)
        for flags in ((False, False), (True, True)):
            one = check_all(env, c, B, 0.1, "min_points 1", min_points=1, flags=[flags])[flags]
            two = check_all(env, c, B, 0.1, "min_points 2", min_points=2, flags=[flags])[flags]
            none = check_all(env, c, B, 0.1, "min_points 4096", min_points=MAX_K, flags=[flags])[flags]
            assert sum(w["counts"][1] for w in two) < sum(w["counts"][1] for w in one) and any(m["n_sparse"] > 0 and m["count"] > 0 for m in used_models(two))
            for a, z in zip(one, none):
                assert z["counts"] == (a["counts"][0], 0) and a["counts"][0] >= 2
                assert (z["models"]["count"] == 0).all() and np.array_equal(z["models"]["n_sparse"], a["models"]["count"]) and (a["models"]["n_sparse"] == 0).all()
                assert np.array_equal(z["models"]["track_id"], a["models"]["track_id"])


# ------------------------------------------------------------------------------------------------------------------ 6: truncation
def truncation(env, oracle):
    """voxel_stride none (null block), 1, in the middle of a model, exactly the total: the first voxel_stride voxels, nothing beyond them, true headers and counts"""
    B, T = 3, 256
    with env.context(0, max_points=2048, max_batch=B, max_tracks_total=T) as c:
        MC.run_moving(env, c, 256, 4, B, frames_n=6)
        for axes, current in ((False, False), (True, True)):
            want = [want_slot(env, c, b, 0.1, 1, axes, current) for b in range(B)]
            n = [w["counts"][1] for w in want]
            full = VoxelBlocks(env, B, T, max(n) + 3).run(c, B, 0.1, 1, axes, current)[1]
            used = want[1]["models"][want[1]["models"]["track_id"] >= 0]
            last = used[-1]
            assert len(used) >= 2 and last["count"] > 2
            for stride in (n[1], int(last["first"]) + int(last["count"]) // 2, int(used[0]["count"]) // 2, 1):
                v, models, cnt = VoxelBlocks(env, B, T, stride).run(c, B, 0.1, 1, axes, current)
                for b in range(B):
                    wn = min(n[b], stride)
                    compare(models[b], v[b, :wn], cnt[b], want[b], 0.1, ("truncated", axes, current, stride, b), full_models=full[b])
                    assert (v[b, wn:] == -7).all(), ("truncated", stride, b, "written beyond the slot's voxels")
            blk = VoxelBlocks(env, B, T, 4)
            assert blk.raw(c, B, MC.flag_bits(env, axes, current), voxels=False, stride=0) == 0   # no voxel block at all: headers and counts
            c.synchronize()
            v, models, cnt = blk.read()
            assert (v == -7).all() and models.tobytes() == full.tobytes() and [tuple(x) for x in cnt] == [w["counts"] for w in want]


# ------------------------------------------------------------------------------------------------------------------ 7: non-finite pose
def non_finite_pose(env, oracle):
    """every logged px of one row NaN: all its records are outside, the model stays without voxels, every other model keeps its bytes"""
    B, T, K, O = 3, 256, 256, 4
    with env.context(0, max_points=2048, max_batch=B, max_tracks_total=T) as c:
        MC.run_moving(env, c, K, O, B, frames_n=6)
        c.synchronize()
        v = c.track_accumulators_dev()
        r = int(np.argmax(c.get_accum_rows(1)["total"]))
        at = 1 * T + r
        for axes in (False, True):
            blk = VoxelBlocks(env, B, T, 2048)
            v0, m0, cnt0 = blk.run(c, B, 0.1, 1, axes, False)
            obs = AC.peek(env, c, v["d_obs"] + at * O * 48, env.mot.ACCUM_OBS_DTYPE, O)
            for k in range(O):
                MC.poke(env, v["d_obs"] + (at * O + k) * 48 + 16, np.array([np.nan], np.float32))
            check_all(env, c, B, 0.1, ("NaN px", axes), flags=[(axes, False)])
            v1, m1, cnt1 = blk.run(c, B, 0.1, 1, axes, False)
            m = m1[1, r]
            assert m["track_id"] >= 0 and m["n_records"] > 0 and m["n_outside"] == m["n_records"] and m["count"] == 0 and m["n_sparse"] == 0 and (m["min"] == 0).all() and (m["max"] == 0).all(), m
            keep = np.ones((B, T), bool); keep[1, r] = False
            same = ("track_id", "count", "n_obs", "first_step", "last_step", "min", "max", "n_records", "n_outside", "n_sparse")
            assert all(np.array_equal(m1[keep][f], m0[keep][f]) for f in same), "another model's header changed"
            assert np.array_equal(v1[0], v0[0]) and np.array_equal(v1[2], v0[2]), "another slot's voxels changed"
            f0, k0 = int(m0[1, r]["first"]), int(m0[1, r]["count"])
            assert k0 > 0 and np.array_equal(v1[1, :f0], v0[1, :f0]) and np.array_equal(v1[1, f0: cnt1[1, 1]], v0[1, f0 + k0: cnt0[1, 1]]), "another model's voxels changed"
            MC.poke(env, v["d_obs"] + at * O * 48, obs)   # (back: the next flag starts from the same log)


# ------------------------------------------------------------------------------------------------------------------ 8: the voxels follow the raw models
def slot_reuse(env, oracle, T_slots=8):
    """track_accum_cases.reuse_stream: a row that restarted under a new id gives the voxels of the new track only (those of its raw model)"""
    frames = AC.reuse_stream()
    with env.context(0, max_points=1024, max_batch=1, max_tracks_total=T_slots) as c:
        c.set_track_links(True); c.set_track_accumulation(64, 4)
        latest = [-1]
        seen = set()
        for f, x in enumerate(frames):
            keep = AC.launch(env, c, [x], 1024, f, ego_v=[0.0])
            MC.accumulate(c, 1, latest)
            want = check_all(env, c, 1, 0.25, ("reuse", f), flags=[(False, False), (True, True)])[(False, False)][0]
            seen |= {(int(r), int(m["track_id"])) for r, m in enumerate(want["models"]) if m["track_id"] >= 0}
    assert len({r for r, _ in seen}) < len(seen), "the script never reused a track slot"


def after_sequence(env, oracle, K=256, O=4):
    """a recorded drive appended by mot_sequence_accumulate_dev: slot 0's voxel models follow its raw models"""
    clouds, ego_v, yaw = SC.moving_stream()
    with env.context(0, max_points=2048, max_batch=len(clouds), max_tracks_total=64) as c:
        c.set_track_links(True); c.set_track_accumulation(K, O)
        keep = SC.seq_call(env, c, clouds, 2048, 0, ego_v, yaw)
        want = check_all(env, c, 1, 0.1, "after a sequence call")[(False, False)][0]
        assert want["counts"][0] >= 2 and want["counts"][1] > 0


# ------------------------------------------------------------------------------------------------------------------ 9: contract
def contract(env, oracle):
    E = env.mot
    B, T = 2, 64
    clouds = [[CC.small_scene(f, 20), CC.small_scene(f + 5, 12)] for f in range(4)]
    with env.context(0, max_points=4096, max_batch=B, max_tracks_total=T) as c:
        blk = VoxelBlocks(env, B, T, 4096)
        nm, nv = C.c_int(-7), C.c_int(-7)
        def getter(slot=0, flags=0, leaf=0.1, mp=1, models=None, max_models=0, voxels=None, cap=0, nm_=nm, nv_=nv, params=True):
            p = E.voxel_params(leaf, 1); p.min_points = mp
            return c.lib.mot_get_track_model_voxels(c._h, slot, flags, C.byref(p) if params else None, models.ctypes.data_as(C.c_void_p) if models is not None else None, max_models,
                                                    C.byref(nm_) if nm_ is not None else None, voxels.ctypes.data_as(C.c_void_p) if voxels is not None else None, cap,
                                                    C.byref(nv_) if nv_ is not None else None)
        # the feature off; on without a log
        c.set_track_links(True)
        assert blk.raw(c, B, 0) == E.MOT_E_STATE and getter() == E.MOT_E_STATE, "accumulation off"
        c.set_track_accumulation(64, 0)
        assert blk.raw(c, B, 0) == E.MOT_E_STATE and getter() == E.MOT_E_STATE, "obs_per_track 0"
        c.set_track_accumulation(64, 4)
        for b in range(B):
            g = c.get_track_model_voxels(b, 0.1)
            assert (g["models"]["track_id"] == -1).all() and len(g["models"]) == T and len(g["count"]) == 0, "before the first accumulate"
        # arguments, on a context whose state would serve the call
        for leaf in (np.nan, np.inf, -0.1, 0.0, 0.99e-3, 1001.0, (0.1, np.nan, 0.1), (0.1, 0.1, 2e3)):
            assert blk.raw(c, B, 0, leaf=leaf) == E.MOT_E_ARG and getter(leaf=leaf) == E.MOT_E_ARG, leaf
        for leaf in (1e-3, 1e3):
            assert blk.raw(c, B, 0, leaf=leaf) == 0 and getter(leaf=leaf) == 0, leaf
        for mp in (0, -1, MAX_K + 1):
            assert blk.raw(c, B, 0, min_points=mp) == E.MOT_E_ARG and getter(mp=mp) == E.MOT_E_ARG, mp
        assert blk.raw(c, B, 0, min_points=MAX_K) == 0 and getter(mp=MAX_K) == 0
        blk = VoxelBlocks(env, B, T, 4096)
        assert blk.raw(c, B, 0, params=False) == E.MOT_E_ARG and getter(params=False) == E.MOT_E_ARG
        for flags in (4, 8, 1 << 30, -1):
            assert blk.raw(c, B, flags) == E.MOT_E_ARG and getter(flags=flags) == E.MOT_E_ARG, flags
        assert blk.raw(c, 0, 0) == E.MOT_E_ARG and blk.raw(c, B + 1, 0) == E.MOT_E_ARG and blk.raw(c, -1, 0) == E.MOT_E_ARG
        assert blk.raw(c, B, 0, models=False) == E.MOT_E_ARG and blk.raw(c, B, 0, counts=False) == E.MOT_E_ARG and blk.raw(c, B, 0, voxels=False) == E.MOT_E_ARG
        assert blk.raw(c, B, 0, stride=-1) == E.MOT_E_ARG
        assert c.lib.mot_export_track_model_voxels_dev(c._h, B, 0, C.byref(E.voxel_params(0.1)), C.c_void_p(blk.p_vox + 4), C.c_long(8), C.c_void_p(blk.p_mod), C.c_void_p(blk.p_cnt)) == E.MOT_E_ARG
        assert getter(slot=B) == E.MOT_E_ARG and getter(slot=-1) == E.MOT_E_ARG and getter(max_models=-1) == E.MOT_E_ARG and getter(cap=-1) == E.MOT_E_ARG
        assert getter(nv_=None) == E.MOT_E_ARG and getter(nm_=None) == E.MOT_E_ARG
        v, models, cnt = blk.read()
        assert (v == -7).all() and (blk.h_mod == -7).all() and (cnt == -7).all(), "a refused call wrote into the caller's blocks"
        latest = [-1] * B
        for f in range(3):
            keep = AC.launch(env, c, clouds[f], 4096, f)
            MC.accumulate(c, B, latest)
        want = check_all(env, c, B, 0.1, "contract")[(False, False)]
        n = want[1]["counts"][1]
        assert n > 1
        # buffers too small: the counts, nothing copied
        for max_models, cap in ((T - 1, n), (T, n - 1)):
            mod = np.full(T * 16, -7, np.int32); vox = np.full(n * 4, -7, np.int32); nm.value = nv.value = -7
            assert getter(1, models=mod, max_models=max_models, voxels=vox, cap=cap) == E.MOT_E_CAPACITY and (nm.value, nv.value) == (T, n), (max_models, cap)
            assert (mod == -7).all() and (vox == -7).all(), "a refused getter wrote"
        mod = np.full(T * 16 + 4, -7, np.int32); vox = np.full(n * 4 + 4, -7, np.int32)
        assert getter(1, models=mod, max_models=T, voxels=vox, cap=n) == 0 and (mod[T * 16:] == -7).all() and (vox[n * 4:] == -7).all()
        assert mod[: T * 16].tobytes() == c.get_track_model_voxels(1, 0.1)["models"].tobytes()
        nm.value = nv.value = -7
        assert getter(1) == 0 and (nm.value, nv.value) == (T, n), "null buffers: the counts alone"
        c.reset()
        assert all((c.get_track_model_voxels(b, 0.1)["models"]["track_id"] == -1).all() for b in range(B)), "reset"
        c.set_track_accumulation(0, 0)
        assert blk.raw(c, B, 0) == E.MOT_E_STATE and getter() == E.MOT_E_STATE, "off again"
    # a ring longer than a model the voxel calls sort: refused by name, and the raw export serves it
    with env.context(0, max_points=4096, max_batch=1, max_tracks_total=4) as c:
        c.set_track_links(True); c.set_track_accumulation(2 * MAX_K, 4)
        keep = AC.launch(env, c, [CC.small_scene(0, 20)], 4096, 0)
        c.accumulate_track_points(1)
        blk = VoxelBlocks(env, 1, 4, 64)
        assert blk.raw(c, 1, 0) == E.MOT_E_STATE and b"4096" in c.lib.mot_last_error(c._h) and b"MOT_MODEL_VOXEL_MAX_K" in c.lib.mot_last_error(c._h)
        assert AC.code_of(env, lambda: c.get_track_model_voxels(0, 0.1)) == E.MOT_E_STATE and b"4096" in c.lib.mot_last_error(c._h)
        v, models, cnt = blk.read()
        assert (v == -7).all() and (blk.h_mod == -7).all() and (cnt == -7).all()
        raw = MC.ModelBlocks(env, 1, 4, 64)
        assert raw.raw(c, 1, 0) == 0
        c.synchronize()
        assert len(c.get_track_models(0)["models"]) == 4


# ------------------------------------------------------------------------------------------------------------------ 10: non-interference
def non_interference(env, oracle, graphs=False):
    """voxel calls interleaved with the steps: the fused outputs, the accumulators and the raw models are byte-identical to a run without them; on the emulator no
    voxel kernel is launched unless a voxel call is made"""
    B, T = 2, 256
    clouds = [[CC.small_scene(f, 20), CC.small_scene(f + 5, 12)] for f in range(4)]
    count = None
    if env.lib_path is not None:
        lib = env.mot.load_library(env.lib_path)
        count = lambda: [lib.hipemu_launch_count(k) for k in KERNELS]
    res = {}
    for tag in ("never", "voxels"):
        with env.context(0, max_points=4096, max_batch=B, max_tracks_total=T) as c:
            c.set_launch_graphs(graphs); c.set_track_links(True); c.set_track_accumulation(256, 4)
            blk = VoxelBlocks(env, B, T, 4096)
            raw = MC.ModelBlocks(env, B, T, 4096)
            before_launches = count() if count else None
            out = []
            for f in range(4):
                keep = PC.launch(env, c, clouds[f], 4096, f, yaw=0.02 * f)
                n_points = [len(x) for x in clouds[f]]
                if tag == "voxels":   # between the fused step and its accumulate
                    blk.run(c, B, 0.1, 1, True, True); c.get_track_model_voxels(1, 0.25, axes=True)
                c.accumulate_track_points(B)
                before = PC.readout(c, B, n_points)
                acc, mem = MC.accumulators(env, c, B)
                raw.run(c, B, True, False)
                models = raw.bytes
                if tag == "voxels":
                    for axes, current in FLAGS:
                        v, m, cnt = blk.run(c, B, (0.3, 0.2, 0.05), 2, axes, current)
                        assert cnt[1, 1] > 0 or f == 0
                        c.get_track_model_voxels(0, 0.1, axes=axes, current=current)
                    PC.equal_readouts(PC.readout(c, B, n_points), before, (f, "after the voxel calls"))   # (one context: every byte)
                    acc2, mem2 = MC.accumulators(env, c, B)
                    assert acc2 == acc and mem2 == mem, (f, "the voxel calls wrote into the accumulators")
                    raw.run(c, B, True, False)
                    assert raw.bytes == models, (f, "the raw models changed behind the voxel calls")
                out.append((AC.defined_items(before), acc, models))
            if count:
                moved = [a - b for a, b in zip(count(), before_launches)]
                assert all(x > 0 for x in moved) if tag == "voxels" else moved == [0, 0, 0], (tag, moved)
            res[tag] = out
    for f in range(4):
        PC.equal_readouts(res["voxels"][f][0], res["never"][f][0], (f, "against a context that never asked for voxels"))
        assert res["voxels"][f][1] == res["never"][f][1], (f, "accumulators against a context that never asked for voxels")
        assert res["voxels"][f][2] == res["never"][f][2], (f, "raw models against a context that never asked for voxels")


# ------------------------------------------------------------------------------------------------------------------ 11: emulator only
def lifecycle(env, oracle):
    """nothing is allocated or launched before the first voxel call; the scratch goes with the accumulators (off, another geometry) and with the context"""
    lib = env.mot.load_library(env.lib_path)
    lib.hipemu_live_allocs.restype = C.c_long
    count = lambda: [lib.hipemu_launch_count(k) for k in KERNELS]
    B, T = 2, 64
    outside = lib.hipemu_live_allocs()
    with env.context(0, max_points=4096, max_batch=B, max_tracks_total=T) as c:
        before = count()
        c.set_track_links(True)
        keep = PC.launch(env, c, [CC.small_scene(0, 20), CC.small_scene(5, 12)], 4096, 0)
        c.get_track_points(1, frame="global")   # (the scratch the accumulate call shares with the per-track point clouds exists from here on)
        allocs = lib.hipemu_live_allocs()
        c.set_track_accumulation(64, 4)
        for f in range(1, 4):
            keep = PC.launch(env, c, [CC.small_scene(f, 20), CC.small_scene(f + 5, 12)], 4096, f)
            c.accumulate_track_points(B)
        raw = MC.ModelBlocks(env, B, T, 4096); raw.run(c, B, True, True); c.get_track_models(1)
        with_raw = lib.hipemu_live_allocs()
        blk = VoxelBlocks(env, B, T, 4096)
        for bad in (dict(flags=4), dict(flags=0, leaf=0.0), dict(flags=0, min_points=0)):
            assert blk.raw(c, B, **bad) == env.mot.MOT_E_ARG
        assert count() == before and lib.hipemu_live_allocs() == with_raw, "a refused voxel call launched or allocated"
        assert blk.raw(c, B, 0, voxels=False, stride=0) == 0
        assert count() == [before[0] + 1, before[1] + 1, before[2]], "a call for the headers runs the count and pack kernels alone"
        with_export = lib.hipemu_live_allocs()
        assert with_export == with_raw + 1, "the export's scratch is one block"
        blk.run(c, B, 0.1, 1, True, True)
        assert count() == [n + 2 for n in before[:2]] + [before[2] + 1] and lib.hipemu_live_allocs() == with_export
        c.get_track_model_voxels(1, 0.1)   # (two calls of the C getter: the counts, then the voxels)
        assert count() == [n + 4 for n in before[:2]] + [before[2] + 2]
        with_getter = lib.hipemu_live_allocs()
        assert with_getter == with_export + 2, "the getter adds its two staging blocks"
        c.get_track_model_voxels(0, 0.25, axes=True); blk.run(c, B, 0.1, 2, False, True)
        assert lib.hipemu_live_allocs() == with_getter
        c.set_track_accumulation(128, 4)   # another geometry: the voxel blocks go with the old tables
        assert lib.hipemu_live_allocs() == allocs + 4
        blk.run(c, B, 0.1, 1, False, False); c.get_track_model_voxels(0, 0.1)
        assert lib.hipemu_live_allocs() > allocs + 4
        c.set_track_accumulation(0, 0)
        assert lib.hipemu_live_allocs() == allocs, "turning accumulation off did not free the voxel calls' memory"
        c.set_track_accumulation(64, 4)
        blk.run(c, B, 0.1, 1, False, False); c.get_track_model_voxels(0, 0.1)   # (mot_destroy releases what these took)
    assert lib.hipemu_live_allocs() == outside, "mot_destroy left memory of the voxel calls behind"


def first_call_under_allocation_failure(env, oracle):
    """each allocation of the first voxel calls failing in turn: MOT_E_HIP, the accumulators as they were, and the next call resumes"""
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
            MC.accumulate(c, B, latest)
            acc = MC.accumulators(env, c, B)
            blk = VoxelBlocks(env, B, T, 4096)
            for who, call, least in (("export", lambda: blk.raw(c, B, 0), 4), ("getter", lambda: AC.code_of(env, lambda: c.get_track_model_voxels(1, 0.1)), 2)):
                failed = 0   # (export: the latest-step block, its page-locked ring, the ring's events, the scratch; getter: its two staging blocks)
                for k in range(1, 40):
                    live = lib.hipemu_live_allocs()
                    lib.hipemu_fail_alloc_at(k)
                    rc = call()
                    lib.hipemu_fail_alloc_at(0)
                    if rc == 0:
                        break
                    assert rc == E.MOT_E_HIP, (who, k, rc)
                    failed += 1
                    assert lib.hipemu_live_allocs() >= live
                    assert MC.accumulators(env, c, B) == acc, (who, k, "a failed voxel call changed the accumulators")
                assert failed >= least, (who, failed)
            check_all(env, c, B, 0.1, "after the failed allocations")
    finally:
        lib.hipemu_fail_alloc_at(0)
