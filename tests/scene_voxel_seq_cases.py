"""The voxel-thinned static map of a recorded drive (mot_export_sequence_scene_voxels_dev / mot_get_sequence_scene_voxels, csrc/scene_voxels_seq.hip, csrc/mot_sort.h):
bodies shared by tests/test_emu_scene_voxels_seq.py (emulator) and tests/test_scene_voxels_seq_gpu.py (MI355X). The callers supply a capacity_cases.Env.

The expectation shares no code with the new kernels. The records come from the existing get_sequence_scene_points(frame="global") on the SAME context behind the SAME
sequence call (that getter is pinned against the frame-by-frame model by tests/scene_judge_seq_cases.py). From them numpy reproduces include/mot.h word for word: the
fp32 cells, a stable np.lexsort on (i_x, i_y, i_z), the 64 fp64 accumulators per axis (vectorised over the voxels: a loop over the rounds, then over l). Voxels, header
and totals are compared AS BYTES, with sentinel margins round every block, through the export and through the getter. No tolerance anywhere."""
import ctypes as C

import numpy as np

import capacity_cases as CC
import scene_grid_seq_cases as SGQ
import scene_judge_cases as SJ
import track_accum_cases as AC
import track_link_cases as LC
import track_point_cases as PC

UNKNOWN, MOVING, TRAIL, NEW, KNOWN = range(5)
ALL = SJ.ALL
MASKS = (1 << KNOWN, (1 << KNOWN) | (1 << NEW), ALL)
T = 2048   # records per workgroup of the sort: kSortTile of csrc/mot_sort.h
KERNELS = (b"scene_voxels_seq_key_kernel", b"radix_sort_hist_kernel", b"radix_sort_scan_kernel", b"radix_sort_scatter_kernel", b"scene_voxels_seq_heads_kernel",
           b"scene_voxels_seq_scan_kernel", b"scene_voxels_seq_runs_kernel", b"scene_voxels_seq_kept_kernel", b"scene_voxels_seq_write_kernel")
PER_CALL = [1, 7, 7, 7, 1, 2, 1, 2, 1]   # launches of an export with a voxel block: 7 passes of the sort, the scan and the kept kernel twice


# ------------------------------------------------------------------------------------------------------------------ the model
def leaf3(leaf):
    return tuple(np.float32(v) for v in ((leaf,) * 3 if np.isscalar(leaf) else leaf))


def cells_of(xyz, leaf):
    """include/mot.h, CELL OF A RECORD -> (takes part [n], i [n, 3] int64 (0 where it does not))"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    inv = np.array([np.float32(1.0) / l for l in leaf3(leaf)], np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        t = (xyz * inv[None, :]).astype(np.float32)
        ok = np.isfinite(xyz).all(axis=1)
        for a, lim in ((0, 2.0 ** 20), (1, 2.0 ** 20), (2, 2.0 ** 11)):
            ok &= (t[:, a] >= np.float32(-lim)) & (t[:, a] < np.float32(lim))
        i = np.where(ok[:, None], np.floor(t), 0).astype(np.int64)
    return ok, i


def keys_of(i):
    return ((i[:, 2] + 2 ** 11) << 42) | ((i[:, 1] + 2 ** 20) << 21) | (i[:, 0] + 2 ** 20)


def centroids(p64, starts, counts):
    """include/mot.h, CENTROID: p64 [n, 3] float64 in sorted order, voxel v owns [starts[v], starts[v] + counts[v])"""
    V = len(starts)
    out = np.zeros((V, 3), np.float32)
    if V == 0:
        return out
    lanes = np.arange(64)[None, :]
    rounds = (int(counts.max()) + 63) // 64
    for a in range(3):
        col = p64[:, a]
        acc = np.zeros((V, 64), np.float64)
        for j in range(rounds):
            has = lanes + 64 * j < counts[:, None]
            val = col[np.where(has, starts[:, None] + lanes + 64 * j, 0)]
            acc = np.where(has, val if j == 0 else acc + val, acc)   # (each accumulator starts FROM its first record)
        S = acc[:, 0].copy()
        for l in range(1, 64):
            S = np.where(l < counts, S + acc[:, l], S)
        out[:, a] = (S / counts.astype(np.float64)).astype(np.float32)
    return out


def model(xyz, n_records, leaf, min_points, record_capacity, voxel_capacity):
    """-> (voxels [n_voxels, 4] int32 (the centroid's bits, count), header [8] int32, facts)"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    assert len(xyz) == n_records
    play = xyz[: min(n_records, record_capacity)]
    ok, i = cells_of(play, leaf)
    pts, cell = play[ok], i[ok]
    order = np.lexsort((cell[:, 0], cell[:, 1], cell[:, 2]))   # stable: a cell's records stay in record order
    pts, cell = pts[order], cell[order]
    n = len(pts)
    head = np.ones(n, bool)
    head[1:] = (cell[1:] != cell[:-1]).any(axis=1)
    starts = np.nonzero(head)[0]
    counts = np.diff(np.append(starts, n))
    kept = counts >= min_points
    cen = centroids(pts.astype(np.float64), starts[kept], counts[kept])
    vox = np.zeros((int(kept.sum()), 4), np.int32)
    vox[:, :3] = cen.view(np.int32); vox[:, 3] = counts[kept]
    nv = len(vox)
    hdr = np.array([n_records, n_records - len(play), int((~ok).sum()), nv, int((~kept).sum()), min(nv, voxel_capacity), 0, 0], np.int32)
    assert hdr[0] == hdr[1] + hdr[2] + int(counts.sum()), "the header invariant (the model's own)"
    facts = dict(m=len(play), runs=len(starts), longest=int(counts.max(initial=0)), cells=cell[starts] if n else np.zeros((0, 3), np.int64), keys=keys_of(cell[starts]) if n else np.zeros(0, np.int64))
    return vox, hdr, facts


def records(c, frames, mask, params=(1, 1, 2)):
    r = c.get_sequence_scene_points(frames, min_static_hits=params[0], trail=params[1:], classes=mask, frame="global", with_classes=False)
    return np.ascontiguousarray(r["xyz"], np.float32), r["totals"].copy()


# ------------------------------------------------------------------------------------------------------------------ the caller's blocks
class Blocks:
    """sentinel-filled device blocks: `capacity` voxels (16-byte aligned), the 32-byte header, [5] totals, a margin on both sides of each; misalign: header and totals
    start 4 bytes off an 8-byte boundary"""

    def __init__(self, env, capacity, misalign=False):
        self.cap, self.off = capacity, (1 if misalign else 0)
        self.h_vox = np.full(4 + capacity * 4 + 4, -7, np.int32); self.h_hdr = np.full(2 + 1 + 8 + 2, -7, np.int32); self.h_tot = np.full(2 + 1 + 10 + 2, -7, np.int32)
        (self.p_vox, self.k_vox), (self.p_hdr, self.k_hdr), (self.p_tot, self.k_tot) = (env.upload(h) for h in (self.h_vox, self.h_hdr, self.h_tot))
        assert self.p_vox % 16 == 0
        self.a_vox, self.a_hdr, self.a_tot = self.p_vox + 16, self.p_hdr + 8 + 4 * self.off, self.p_tot + 8 + 4 * self.off

    def run(self, c, frames, mask, leaf, min_points=1, record_capacity=None, params=(1, 1, 2), voxels=True, totals=True):
        c.export_sequence_scene_voxels_dev(frames, leaf, self.a_vox if voxels else 0, self.cap if voxels else 0, self.a_hdr, self.a_tot if totals else 0, min_points=min_points,
                                           min_static_hits=params[0], trail=params[1:], classes=mask, record_capacity=record_capacity)
        c.synchronize()
        return self.read()

    def raw(self):
        return tuple(LC.download(k, h).copy() for k, h in ((self.k_vox, self.h_vox), (self.k_hdr, self.h_hdr), (self.k_tot, self.h_tot)))

    def read(self):
        vox, hdr, tot = self.raw()
        o = self.off
        assert (vox[:4] == -7).all() and (vox[4 + self.cap * 4:] == -7).all(), "voxels outside the caller's block"
        assert (hdr[: 2 + o] == -7).all() and (hdr[2 + o + 8:] == -7).all(), "the header outside its block"
        assert (tot[: 2 + o] == -7).all() and (tot[2 + o + 10:] == -7).all(), "totals outside their block"
        return vox[4: 4 + self.cap * 4].reshape(self.cap, 4), hdr[2 + o: 2 + o + 8], tot[2 + o: 2 + o + 10].reshape(5, 2)

    def free(self):
        for k in (self.k_vox, self.k_hdr, self.k_tot):
            if hasattr(k, "free"):
                k.free()


def check(env, c, frames, mask, leaf, what, min_points=1, record_capacity=None, voxel_capacity=None, params=(1, 1, 2), misalign=False, getter=True, totals=True):
    """one export (and the getter) against the model -> the model's facts and header"""
    xyz, tot = records(c, frames, mask, params)
    m = int(sum(int(tot["count"][k]) for k in range(5) if (mask >> k) & 1))
    rc = frames * c.max_points if record_capacity is None else record_capacity
    vox, _, _ = model(xyz, m, leaf, min_points, rc, 0)
    vc = len(vox) + 3 if voxel_capacity is None else voxel_capacity
    vox, hdr, facts = model(xyz, m, leaf, min_points, rc, vc)
    blk = Blocks(env, vc, misalign)
    v, h, t = blk.run(c, frames, mask, leaf, min_points, record_capacity, params, totals=totals)
    blk.free()
    assert h.tobytes() == hdr.tobytes(), (what, "header", h.tolist(), hdr.tolist())
    if totals:
        assert t.tobytes() == tot.tobytes(), (what, "totals", t.tolist(), tot.tolist())
    else:
        assert (t == -7).all(), (what, "totals written without a block")
    w = min(len(vox), vc)
    if v[:w].tobytes() != vox[:w].tobytes():
        bad = np.argwhere(v[:w] != vox[:w])
        raise AssertionError((what, "voxels", len(bad), "words differ; first", bad[0], v[bad[0][0]], vox[bad[0][0]]))
    assert (v[w:] == -7).all(), (what, "written beyond the kept voxels")
    if getter:
        r = c.get_sequence_scene_voxels(frames, leaf, min_points=min_points, min_static_hits=params[0], trail=params[1:], classes=mask, record_capacity=record_capacity)
        got = np.zeros((len(r["count"]), 4), np.int32); got[:, :3] = np.ascontiguousarray(r["xyz"], np.float32).view(np.int32).reshape(-1, 3); got[:, 3] = r["count"]
        gh = np.frombuffer(r["header"].tobytes(), np.int32).copy(); want = hdr.copy(); want[5] = len(vox)   # (the getter's second call has room for all)
        assert got.tobytes() == vox.tobytes() and gh.tobytes() == want.tobytes() and r["totals"].tobytes() == tot.tobytes(), (what, "getter", gh.tolist(), want.tolist())
    return facts, hdr


def context(env, F, cell, W, max_points, tracks, order_any=False, accum=None, pkw=None):
    c = env.context(0, pkw=pkw, max_points=max_points, max_batch=F, max_tracks_total=tracks)
    c.set_track_links(True); c.set_scene_grid(cell, W)
    if accum:
        c.set_track_accumulation(*accum)
    if order_any:
        c.set_point_order(env.mot.MOT_ORDER_ANY)
    return c


# ------------------------------------------------------------------------------------------------------------------ 1: sizes
SIZES = (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 2 * T + 1 + 5000)


def sizes(env, oracle):
    """successive frames of ONE call whose elevated counts add up to 0, 1, 63, 64, 65, T - 1, T, T + 1, 2 T + 1 and 4.4 tiles (prefixes of track_link_cases'
    source: a frame of n points has n elevated points): with mask ALL m is the sum over the first `frames` frames. Every mask at every size"""
    p = oracle.params(0)
    per = np.diff((0,) + SIZES)
    clouds = [LC.frame_with_elevated(oracle, p, int(n), seed=k % 3) for k, n in enumerate(per)]
    F = len(clouds)
    with context(env, F, 1.0, 64, 8192, 512) as c:
        keep = SGQ.seq_call(env, c, clouds, 8192, 0, [1.0] * F, [0.0] * F)
        seen = set()
        for frames in range(1, F + 1):
            for mask in MASKS:
                facts, hdr = check(env, c, frames, mask, 0.5, ("sizes", frames, mask), getter=(frames == F))
                if mask == ALL:
                    assert facts["m"] == hdr[0] == SIZES[frames - 1], (frames, facts["m"])
                    seen.add(facts["m"])
        assert set(SIZES) <= seen
        facts, hdr = check(env, c, F, 1 << KNOWN, 0.5, "sizes, KNOWN")
        assert hdr[3] > 0, "no KNOWN voxel in the drive"


# ------------------------------------------------------------------------------------------------------------------ 2: runs
def standing(env, oracle, n_blobs=12, F=17):
    return [CC.small_scene(3, n_blobs)] * F, [0.0] * F, [0.0] * F


def runs(env, oracle):
    """a standing vehicle that sees the same cloud in 17 frames: frames 1 .. 16 share one pose (the tracker's first step places frame 0 a quarter turn away, by the
    reference's rule), so every voxel a later frame touches holds 16 records or more, frame 0's own cells its one frame's; runs cross tile boundaries; a leaf of 1000 m: one voxel holds
    every record of a quadrant (n > 64: the wave path, a run over many tiles); a leaf of 0.01 m: nearly every point is a voxel of its own"""
    clouds, ego_v, yaw = standing(env, oracle)
    F = len(clouds)
    with context(env, F, 1.0, 64, 1024, 64) as c:
        keep = SGQ.seq_call(env, c, clouds, 1024, 0, ego_v, yaw)
        facts, hdr = check(env, c, F, ALL, 0.5, "runs, the same cloud 17 times")
        assert facts["m"] > 2 * T and hdr[3] > 0 and hdr[2] == 0
        xyz, _ = records(c, F, ALL)
        seg = c.get_sequence_scene_points(F, frame="global", with_classes=False)["segments"]
        later = np.ones(len(xyz), bool)   # the records of frames 1 .. 16 (the layout is class-major: frame 0's part of every class)
        for k in range(5):
            later[int(seg["first"][0, k]): int(seg["first"][0, k]) + int(seg["count"][0, k])] = False
        ok, i = cells_of(xyz[later], 0.5)
        _, n_per = np.unique(i[ok], axis=0, return_counts=True)
        assert n_per.min() >= F - 1, "a voxel with fewer records than the frames that share a pose"
        facts, hdr = check(env, c, F, ALL, 1000.0, "runs, a leaf of 1000 m")
        assert hdr[3] <= 8 and facts["longest"] > T, (hdr.tolist(), facts["longest"])
        facts, hdr = check(env, c, F, ALL, (1000.0, 1000.0, 0.01), "runs, flat slabs")
        facts, hdr = check(env, c, 1, ALL, 0.01, "runs, a leaf of 0.01 m")
        assert hdr[3] > 0.9 * facts["m"], (hdr.tolist(), facts["m"])
        facts, hdr = check(env, c, F, ALL, 0.01, "runs, a leaf of 0.01 m, 17 frames", min_points=F)
        assert hdr[3] > 0


# ------------------------------------------------------------------------------------------------------------------ 3: key digits
def quadrant_cloud(seed, zs):
    """blobs in one quadrant of the sensor frame, z values from `zs` (the transform is a rotation about z and a shift in x, y: z passes through bit for bit)"""
    rng = np.random.default_rng(seed)
    xy = np.concatenate([np.array([cx, cy]) + rng.uniform(-0.3, 0.3, (48, 2)) for cx in (6.0, 9.0, 12.0) for cy in (6.0, 9.0, 12.0)])
    q = np.zeros((len(xy), 4), np.float32); q[:, :2] = xy; q[:, 2] = rng.choice(np.asarray(zs, np.float32), len(xy))
    return q


def key_digits(env, oracle):
    """cells that straddle 0 on every axis (the bias); keys that differ only in the lowest digit, and only in the highest digit used; non-finite z lands in n_outside
    (planted here: no shared cloud has one). The lattice's edges: lattice_edges"""
    F = 3
    with context(env, F, 1.0, 64, 4096, 64) as c:
        rng = np.random.default_rng(23)
        ring = np.concatenate([np.array([cx, cy]) + rng.uniform(-0.3, 0.3, (48, 2)) for cx in (-9.0, -5.0, 5.0, 9.0) for cy in (-9.0, -5.0, 5.0, 9.0)])
        cloud = np.zeros((len(ring), 4), np.float32); cloud[:, :2] = ring; cloud[:, 2] = rng.uniform(-0.3, 0.3, len(ring))
        clouds = [cloud] * F   # blobs in all four quadrants of the sensor frame, z on both sides of 0
        keep = SGQ.seq_call(env, c, clouds, 4096, 0, [1.0] * F, [0.0] * F)
        facts, hdr = check(env, c, F, ALL, (8.0, 8.0, 0.25), "key digits, straddling 0")
        for a in range(3):
            assert {-1, 0} <= set(facts["cells"][:, a].tolist()), ("no cell at -1 and at 0 on axis", a)
    with context(env, F, 1.0, 64, 4096, 64) as c:
        # one quadrant, z on chosen heights: i_x and i_y constant under a leaf of 1000 m
        zs_top = [0.005 + 0.64 * k for k in range(4)]   # i_z = 0, 64, 128, 192 at a leaf of 0.01: bits 48 and above of the key alone
        clouds = [quadrant_cloud(5, zs_top)[:0]] + [quadrant_cloud(5, zs_top)] * (F - 1)   # (frame 0 empty: the tracker's first step places it a quarter turn away)
        keep = SGQ.seq_call(env, c, clouds, 4096, 0, [0.0] * F, [0.0] * F)
        facts, hdr = check(env, c, F, ALL, (1000.0, 1000.0, 0.01), "key digits, the highest digit alone")
        k = facts["keys"]
        assert len(k) >= 3 and len(set((k & ((1 << 48) - 1)).tolist())) == 1, "the keys differ below bit 48"
        xyz, _ = records(c, F, ALL)
        assert len(set(np.sign(xyz[:, 0]).tolist())) == 1 and len(set(np.sign(xyz[:, 1]).tolist())) == 1, "the quadrant straddles an axis of the global frame"
        leaf_x = float(np.abs(xyz[:, 0]).max()) / 255.5   # i_x in [0, 255] or [-256, -1]: the low 8 bits of i_x + 2^20 alone
        facts, hdr = check(env, c, F, ALL, (leaf_x, 1000.0, 1000.0), "key digits, the lowest digit alone")
        k = facts["keys"]
        assert len(k) >= 3 and len(set((k >> 8).tolist())) == 1, "the keys differ above bit 7"
    with context(env, F, 1.0, 64, 4096, 64) as c:
        clouds = [CC.small_scene(f, 20).copy() for f in range(F)]
        for f, x in enumerate(clouds):
            x[5 + f::97, 2] = (np.nan, np.inf, -np.inf)[f]
        keep = SGQ.seq_call(env, c, clouds, 4096, 0, [1.0] * F, [0.0] * F)
        facts, hdr = check(env, c, F, ALL, 0.25, "key digits, non-finite z")
        assert hdr[2] > 0, "no record with a non-finite coordinate reached the voxel call"
        check(env, c, F, 1 << UNKNOWN, 0.25, "key digits, non-finite z, UNKNOWN alone")


def edge_leaf(far, target):
    """a float32 leaf whose inv = 1.0f / leaf puts the fp32 product far * inv exactly on `target` (searched among the neighbours of target / far)"""
    f32 = np.float32
    inv = f32(f32(target) / f32(far))
    invs = [inv]
    for _ in range(400):
        invs = [np.nextafter(invs[0], f32(0))] + invs + [np.nextafter(invs[-1], f32(np.inf))]
    for cand in sorted((v for v in invs if f32(f32(far) * v) == f32(target)), key=lambda v: abs(float(v) - float(inv))):
        leaf = f32(f32(1.0) / cand)
        leaves = [leaf]
        for _ in range(16):
            leaves = [np.nextafter(leaves[0], f32(0))] + leaves + [np.nextafter(leaves[-1], f32(np.inf))]
        for l in leaves:
            if f32(1.0) / l == cand and 1e-2 <= float(l) <= 1e3:
                return float(l)
    raise AssertionError(("no legal leaf puts the record on the limit", float(far), float(target)))


def lattice_edges(env, oracle):
    """finite records ON the lattice's limits at a legal leaf. The ground stage keeps no point further out than its region of interest, so the far coordinates come
    from the drive: 20 km a frame along +y, -y, -x, +x of the global frame (speed and heading of the sequence call), and a planted point 31.5 m up for +z. For -z a
    standing drive in a context whose ground stage clamps a cell's ground height at t_hmin = -100 m instead of the preset's: a planted point at -40 m is the ground
    of its cell and one at -25 m above it stays elevated. Per edge
    the record with the largest |coordinate| is put EXACTLY on a float the contract names by the choice of the leaf (edge_leaf; the other axes at 1000 m): on the
    inner side — t = -2^20, the largest float below 2^20, t_z = -2^11, the largest float below 2^11 — n_outside is 0 and the edge cell (-2^20, 2^20 - 1, -2^11,
    2^11 - 1) holds a voxel; on the outer side — the float below -2^20, t = 2^20, the float below -2^11, t_z = 2^11 — n_outside is the number of records at that
    coordinate. Every one of the twelve checks must run."""
    f32 = np.float32
    base = CC.small_scene(1, 8)
    high = np.zeros((1, 4), np.float32); high[0, :3] = (6.0, 6.0, 31.5)
    cloud = np.concatenate([base, high])
    q = np.pi / 2
    low = np.zeros((2, 4), np.float32); low[:, :3] = ((6.0, 6.0, -40.0), (6.0, 6.0, -25.0))
    deep = np.concatenate([base, low])
    drives = ((((1, +1), (2, +1)), [2.0e5] * 3, [0.0] * 3, cloud, None), (((1, -1),), [-2.0e5] * 3, [0.0] * 3, cloud, None), (((0, -1),), [2.0e5] * 3, [0.0, q, q], cloud, None),
              (((0, +1),), [2.0e5] * 3, [0.0, -q, -q], cloud, None), (((2, -1),), [0.0] * 3, [0.0] * 3, deep, dict(t_hmin=-100.0)))
    ran = 0
    for edges, ego_v, yaw, cloud, pkw in drives:
        with context(env, 3, 1.0, 64, 1024, 64, pkw=pkw) as c:
            keep = SGQ.seq_call(env, c, [cloud[:0], cloud, cloud], 1024, 0, ego_v, yaw)
            xyz, _ = records(c, 3, ALL)
            for a, sign in edges:
                L = f32(2.0 ** 11 if a == 2 else 2.0 ** 20)
                col = xyz[:, a]
                far = col[np.argmax(np.abs(col))]
                assert np.sign(far) == sign and abs(float(far)) >= 0.0101 * float(L), ("the drive does not reach the limit at a legal leaf", a, sign, float(far))
                at_far = int((col == far).sum())
                inner, outer = (np.nextafter(L, f32(0)), L) if sign > 0 else (-L, np.nextafter(-L, f32(-np.inf)))
                for target, inside in ((inner, True), (outer, False)):
                    leaf = [1000.0, 1000.0, 1000.0]; leaf[a] = edge_leaf(far, target)
                    assert f32(far * (f32(1.0) / f32(leaf[a]))) == target
                    facts, hdr = check(env, c, 3, ALL, tuple(leaf), ("edges", a, sign, float(target)), getter=inside); ran += 1
                    if inside:
                        assert hdr[2] == 0, ("a record on the inner side of a limit was left out", a, sign, hdr.tolist())
                        assert (facts["cells"][:, a] == int(np.floor(target))).any(), ("no voxel in the edge cell", a, sign)
                    else:
                        assert hdr[2] == at_far > 0, ("n_outside for the records on the outer side of a limit", a, sign, hdr.tolist(), at_far)
    assert ran == 12, ran


# ------------------------------------------------------------------------------------------------------------------ 4: capacities
def capacities(env, oracle):
    """record_capacity at m, m - 1, 1 and 0 (n_beyond and the invariant); voxel_capacity at n_voxels, one below and 0, nothing written beyond; min_points at 1, 2 and
    above every count; header and totals 4 bytes off; no totals block; no voxel block"""
    clouds, ego_v, yaw = standing(env, oracle, n_blobs=20, F=5)
    F = len(clouds)
    with context(env, F, 1.0, 64, 1024, 64) as c:
        keep = SGQ.seq_call(env, c, clouds, 1024, 0, ego_v, yaw)
        facts, hdr = check(env, c, F, ALL, 0.3, "capacities, plain")
        m, nv = int(hdr[0]), int(hdr[3])
        assert m > T and nv > 3
        for rc in (m, m - 1, T, 1, 0, m + 1):
            f2, h2 = check(env, c, F, ALL, 0.3, ("capacities, record_capacity", rc), record_capacity=rc, misalign=(rc % 2 == 1))
            assert h2[1] == max(m - rc, 0) and h2[0] == m
        for vc in (nv, nv - 1, 1, 0):
            f2, h2 = check(env, c, F, ALL, 0.3, ("capacities, voxel_capacity", vc), voxel_capacity=vc, misalign=True)
            assert h2[3] == nv and h2[5] == min(nv, vc)
        for mp in (1, 2, F, F + 1, facts["longest"], facts["longest"] + 1, 2 ** 30):
            f2, h2 = check(env, c, F, ALL, 0.3, ("capacities, min_points", mp), min_points=mp)
            assert h2[3] + h2[4] == facts["runs"]
            if mp > facts["longest"]:
                assert h2[3] == 0 and h2[4] == facts["runs"]
        check(env, c, F, (1 << KNOWN) | (1 << NEW), 0.3, "capacities, no totals block", totals=False, getter=False)
        blk = Blocks(env, 4)
        v, h, t = blk.run(c, F, ALL, 0.3, voxels=False)
        assert (v == -7).all() and h[3] == nv and h[5] == 0
        blk.free()


# ------------------------------------------------------------------------------------------------------------------ 5: contract
def raw_export(c, E, blk, frames=3, params=(1, 1, 2), mask=ALL, leaf=(0.5, 0.5, 0.5), min_points=1, rcap=3 * 4096, voxels="a", vcap=None, header="a", totals="a", voxel=True):
    P = E.MotSceneJudgeParams(*params) if params is not None else None
    V = E.MotVoxelParams(leaf[0], leaf[1], leaf[2], min_points) if voxel else None
    ptr = lambda v, a: None if v is None else (a if v == "a" else v)
    return c.lib.mot_export_sequence_scene_voxels_dev(c._h, frames, C.byref(P) if P is not None else None, mask, C.byref(V) if V is not None else None, C.c_long(rcap),
                                                      C.c_void_p(ptr(voxels, blk.a_vox)), C.c_long(blk.cap if vcap is None else vcap), C.c_void_p(ptr(header, blk.a_hdr)),
                                                      C.c_void_p(ptr(totals, blk.a_tot)))


def contract(env, oracle):
    """every refusal with the caller's blocks unchanged; the states that answer MOT_E_STATE (the judge cases' list; links cannot go off while the grid is on: "the grid off" covers both); served behind MOT_SEQ_SCENE | MOT_SEQ_ACCUMULATE;
    the getter's MOT_E_CAPACITY delivers the counts"""
    E = env.mot
    W, F, stride = 64, 3, 4096
    clouds = [CC.small_scene(f, 20) for f in range(8)]
    ones, zeros = [1.0] * F, [0.0] * F
    with context(env, F, 1.0, W, stride, 64, accum=(64, 4)) as c:
        blk = Blocks(env, F * stride)
        export = lambda frames=F: c.export_sequence_scene_voxels_dev(frames, 0.5, blk.a_vox, blk.cap, blk.a_hdr, blk.a_tot, classes=ALL)
        getter = lambda frames=F: c.get_sequence_scene_voxels(frames, 0.5)
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
        blk2 = Blocks(env, F * stride); export(); before = blk.raw()
        nan = float("nan")
        for what, kw in (("null params", dict(params=None)), ("min_static_hits 0", dict(params=(0, 1, 2))), ("den 0", dict(params=(1, 0, 0))), ("num > den", dict(params=(1, 3, 2))),
                         ("mask bit 5", dict(mask=32)), ("negative mask", dict(mask=-1)), ("frames 0", dict(frames=0)), ("frames beyond the call's", dict(frames=F + 1)),
                         ("null voxel params", dict(voxel=False)), ("null header", dict(header=None)), ("leaf NaN", dict(leaf=(nan, 0.5, 0.5))), ("leaf inf", dict(leaf=(0.5, float("inf"), 0.5))),
                         ("leaf below 1e-2", dict(leaf=(0.5, 0.5, 0.009))), ("leaf above 1e3", dict(leaf=(1000.5, 0.5, 0.5))), ("leaf 0", dict(leaf=(0.0, 0.5, 0.5))),
                         ("negative leaf", dict(leaf=(0.5, -0.5, 0.5))), ("min_points 0", dict(min_points=0)), ("min_points 2^30 + 1", dict(min_points=2 ** 30 + 1)),
                         ("negative min_points", dict(min_points=-1)), ("negative record_capacity", dict(rcap=-1)), ("record_capacity 2^31", dict(rcap=2 ** 31)),
                         ("negative voxel_capacity", dict(vcap=-1)), ("null voxels with a capacity", dict(voxels=None)), ("voxels off 16 bytes", dict(voxels=blk.a_vox + 4)),
                         ("voxels off 16 bytes by 8", dict(voxels=blk.a_vox + 8)), ("header off 4 bytes", dict(header=blk.a_hdr + 2)), ("totals off 4 bytes", dict(totals=blk.a_tot + 2))):
            assert raw_export(c, E, blk, **kw) == E.MOT_E_ARG, what
            untouched(what, before)
        assert raw_export(c, E, blk, leaf=(1e-2, 1e3, 0.5), min_points=2 ** 30) == 0 and raw_export(c, E, blk, voxels=None, vcap=0, totals=None) == 0, "the limits themselves are served"
        export(F - 1); getter(1)   # fewer frames are served, again and again
        c.ego_update(3.0e8, 0.0, 0.0, 1); c.track_step(LC.lattice(3), 3.0e8, slot=1)
        state_error("a tracker step fed from outside")
        keep = drive(); export()
        elev = c.get_ground(0, n_hint=len(clouds[0]))["elevated"]
        getter()
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
        blk.free(); blk2.free()
    with context(env, F, 1.0, W, stride, 64, accum=(64, 4)) as c:
        keep = SGQ.seq_call(env, c, clouds[:F], stride, 0, ones, zeros, accumulate=True)
        facts, hdr = check(env, c, F, ALL, 0.5, "behind both products")
        xyz, tot = records(c, F, ALL)
        vox, hdr, facts = model(xyz, int(hdr[0]), 0.5, 1, F * stride, 0)
        nv = len(vox)
        assert nv > 1
        n = C.c_long(-7); hh = np.full(8, -7, np.int32); ht = np.full(10, -7, np.int32); P = E.MotSceneJudgeParams(1, 1, 2); V = E.MotVoxelParams(0.5, 0.5, 0.5, 1)
        out = np.full((nv + 1) * 4, -7, np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        raw_get = lambda frames=F, P=P, mask=ALL, V=V, rcap=F * stride, out=None, vcap=0, n=n, hdr=hh, tot=ht: c.lib.mot_get_sequence_scene_voxels(
            c._h, frames, C.byref(P) if P is not None else None, mask, C.byref(V) if V is not None else None, C.c_long(rcap), vp(out) if out is not None else None, C.c_long(vcap),
            C.byref(n) if n is not None else None, vp(hdr) if hdr is not None else None, vp(tot) if tot is not None else None)
        for what, kw in (("frames 0", dict(frames=0)), ("frames 4", dict(frames=F + 1)), ("null params", dict(P=None)), ("mask", dict(mask=32)), ("null voxel params", dict(V=None)),
                         ("null n_voxels", dict(n=None)), ("null header", dict(hdr=None)), ("negative capacity", dict(vcap=-1)), ("negative record_capacity", dict(rcap=-1)),
                         ("a bad leaf", dict(V=E.MotVoxelParams(0.5, 0.001, 0.5, 1)))):
            assert raw_get(**kw) == E.MOT_E_ARG, what
        assert n.value == -7 and (hh == -7).all() and (ht == -7).all()
        assert raw_get(out=out, vcap=nv - 1) == E.MOT_E_CAPACITY
        want = hdr.copy(); want[5] = 0   # (the getter's n_stored: what it copied)
        assert n.value == nv and hh.tobytes() == want.tobytes() and ht.tobytes() == tot.tobytes() and (out == -7).all()
        assert raw_get(out=out, vcap=nv) == 0 and out[: nv * 4].tobytes() == vox.tobytes() and (out[nv * 4:] == -7).all()
        assert hh[5] == nv, "the getter's n_stored after a full copy"
        n.value = -7
        assert raw_get(tot=None) == 0 and n.value == nv and hh[5] == 0 and hh[3] == nv, "null buffers: the counts alone, nothing stored"


# ------------------------------------------------------------------------------------------------------------------ 6: non-interference, determinism
def voxel_calls(env, c, F):
    blk = Blocks(env, F * c.max_points)
    for mask, leaf in ((ALL, 0.5), (1 << KNOWN, (0.2, 0.3, 0.1))):
        v, h, t = blk.run(c, F, mask, leaf)
        assert h[0] > 0 or mask != ALL
    c.get_sequence_scene_voxels(F, 0.25, classes=(KNOWN, NEW)); c.get_sequence_scene_voxels(1, 1.0, min_points=2)
    blk.free()


def non_interference(env, oracle):
    """two sequence calls in a row with both products: the grid, the accumulators' rows, every slot's readout and a following judge call are byte-identical with and
    without voxel calls in between"""
    import scene_judge_seq_cases as SJQ
    import track_accum_seq_cases as SQ
    clouds = [CC.small_scene(f, 20) for f in range(4)]
    res = {}
    for tag in ("never", "thinned"):
        with env.context(0, max_points=4096, max_batch=2, max_tracks_total=256) as c:
            c.set_track_links(True); c.set_track_accumulation(256, 4); c.set_scene_grid(1.0, 64)
            out = []
            for f0 in (0, 2):
                tb = SQ.TrackBlocks(env, 2, 64)
                keep = SGQ.seq_call(env, c, clouds[f0:f0 + 2], 4096, f0, [1.0] * 2, [0.02 * f0, 0.02 * (f0 + 1)], accumulate=True, tracks=tb.args())
                if tag == "thinned":
                    voxel_calls(env, c, 2)
                items = SQ.sequence_readout(env, c, [len(x) for x in clouds[f0:f0 + 2]]) + tb.read()
                items += [("rows", c.get_accum_rows(0).tobytes())] + [("grid " + n, x) for n, x in SGQ.grid_state(env, c, 64)]
                if tag == "thinned":
                    voxel_calls(env, c, 2)
                jb = SJQ.Blocks(env, 2, 2 * 4096, 4096)
                jb.run(c, 2, ALL, "global")
                items += [("judge %d" % k, x.tobytes()) for k, x in enumerate(jb.raw())]
                jb.free()
                out.append(items)
            res[tag] = out
    for k in range(2):
        PC.equal_readouts(res["thinned"][k], res["never"][k], (k, "against a context that never thinned"))


def run_script(env, c):
    clouds, ego_v, yaw = SGQ.drive(env)
    c.set_track_links(True); c.set_scene_grid(0.27, 64)
    out = []
    for f0 in (0, 8):
        SGQ.seq_call(env, c, clouds[f0:f0 + 8], 2048, f0, ego_v[f0:f0 + 8], yaw[f0:f0 + 8])
        blk = Blocks(env, 8 * 2048)
        blk.run(c, 8, ALL, 0.2); first = [x.tobytes() for x in blk.raw()]
        blk.run(c, 8, ALL, 0.2)
        assert [x.tobytes() for x in blk.raw()] == first, (f0, "two calls on one state differ")
        blk.free()
        out.append(first)
    return out


def determinism(env, oracle):
    """two calls on one state give identical bytes; the same script in two contexts gives identical bytes"""
    runs_ = []
    for k in range(2):
        with env.context(0, max_points=2048, max_batch=8, max_tracks_total=256) as c:
            runs_.append(run_script(env, c))
    assert runs_[0] == runs_[1]
    hdr = np.frombuffer(runs_[0][-1][1], np.int32)[2: 10]
    assert hdr[3] > 0 and hdr[0] > T, hdr


def helper_pieces(env, oracle):
    """sequence.play_static_voxel_map cuts the 16-frame drive into calls of max_batch = 5 frames: every piece thinned on its own, against the model"""
    import importlib
    seq_mod = importlib.import_module(env.mot.__name__ + ".sequence")
    clouds, ego_v, yaw = SGQ.drive(env)
    res = {}
    for tag in ("voxels", "points"):
        with context(env, 5, 0.27, 64, 2048, 256) as c:
            fn = seq_mod.play_static_voxel_map if tag == "voxels" else seq_mod.play_static_map
            kw = dict(leaf=0.3, min_points=2) if tag == "voxels" else dict(frame="global")
            res[tag] = fn(c, list(zip(clouds, ego_v, yaw)), dt_us=1e5, t0=2.0e8, classes=(KNOWN, TRAIL), upload=env.upload, **kw)
    assert [r["first_frame"] for r in res["voxels"]] == [0, 5, 10, 15]
    kept = 0
    for rv, rp in zip(res["voxels"], res["points"]):
        m = int(rp["totals"]["count"][[TRAIL, KNOWN]].sum())
        vox, hdr, facts = model(rp["xyz"], m, 0.3, 2, 5 * 2048, 0)
        got = np.zeros((len(rv["count"]), 4), np.int32); got[:, :3] = np.ascontiguousarray(rv["xyz"], np.float32).view(np.int32).reshape(-1, 3); got[:, 3] = rv["count"]
        assert got.tobytes() == vox.tobytes() and rv["totals"].tobytes() == rp["totals"].tobytes(), ("piece", rv["first_frame"])
        kept += len(vox)
    assert kept > 0


# ------------------------------------------------------------------------------------------------------------------ 7: emulator only
def launches_only_in_the_new_calls(env, oracle):
    """emulator: the new kernels' launch counters move in the new calls and nowhere else; the same number of launches for 2 and for 17 frames, and for m = 1 and
    several tiles; the scratch goes with the grid and with mot_destroy"""
    import scene_judge_seq_cases as SJQ
    lib = env.mot.load_library(env.lib_path)
    lib.hipemu_live_allocs.restype = C.c_long
    count = lambda: [lib.hipemu_launch_count(k) for k in KERNELS]
    base = lib.hipemu_live_allocs()
    per_call = {}
    for F, n_blobs in ((2, 0), (17, 12)):
        clouds = [CC.small_scene(f % 5, n_blobs) if n_blobs else LC.link_frame_source(0)[:f] for f in range(F)]   # (F = 2: frames of 0 and 1 points, m = 1)
        with context(env, F, 1.0, 64, 1024, 64) as c:
            before = count()
            keep = AC.launch(env, c, clouds[:2], 1024, 0); c.accumulate_scene(2)
            SGQ.seq_call(env, c, clouds[:2], 1024, 1, [1.0] * 2, [0.0] * 2, scene=False)
            SGQ.seq_call(env, c, clouds, 1024, 3, [1.0] * F, [0.0] * F)
            c.get_scene_grid(0); c.get_sequence_scene_points(F)
            jb = SJQ.Blocks(env, F, F * 1024, 1024); jb.run(c, F, ALL, "global"); jb.free()
            allocs = lib.hipemu_live_allocs()
            assert count() == before, "a kernel of the voxel calls ran outside them"
            blk = Blocks(env, F * 1024)
            assert raw_export(c, env.mot, blk, frames=F, mask=32) == env.mot.MOT_E_ARG
            assert lib.hipemu_live_allocs() == allocs and count() == before, "a refused call allocated or launched"
            v, h, t = blk.run(c, F, ALL, 0.5)
            assert h[0] == (1 if F == 2 else h[0]) and (F == 2 or h[0] > 2 * T)
            assert count() == [a + b for a, b in zip(before, PER_CALL)] and lib.hipemu_live_allocs() == allocs + 1, "one block of the feature's own (the judge's were there)"
            blk.run(c, F, ALL, 0.5, voxels=False)
            assert count() == [a + 2 * b for a, b in zip(before[:-1], PER_CALL[:-1])] + [before[-1] + 1], "no voxel block: the write kernel is not launched"
            per_call[F] = PER_CALL
            blk.run(c, F, ALL, 0.5, record_capacity=F * 1024 + 5000)   # the block grows: still one
            assert lib.hipemu_live_allocs() == allocs + 1
            c.get_sequence_scene_voxels(F, 0.5)
            assert lib.hipemu_live_allocs() == allocs + 2   # (the getter's table block)
            c.set_scene_grid(None)
            assert lib.hipemu_live_allocs() < allocs, "turning the grid off did not free the scratch"
            c.set_scene_grid(1.0, 64)
            SGQ.seq_call(env, c, clouds[:2], 1024, 0, [1.0] * 2, [0.0] * 2)
            c.get_sequence_scene_voxels(2, 0.5)
            blk.free()
        assert lib.hipemu_live_allocs() == base, "mot_destroy left allocations of the feature behind"
    assert per_call[2] == per_call[17]


def scratch_under_allocation_failure(env, oracle):
    """emulator: each of the five scratch allocations failing in turn at the first call -> MOT_E_HIP, nothing kept, the caller's blocks untouched; the next call gives
    the model's bytes"""
    lib = env.mot.load_library(env.lib_path)
    lib.hipemu_live_allocs.restype = C.c_long
    lib.hipemu_fail_alloc_at.argtypes = [C.c_long]; lib.hipemu_fail_alloc_at.restype = None
    E = env.mot
    F = 3
    clouds = [CC.small_scene(f, 20) for f in range(F)]
    try:
        with context(env, F, 1.0, 64, 4096, 64) as c:
            keep = SGQ.seq_call(env, c, clouds, 4096, 0, [1.0] * F, [0.0] * F)
            c.get_scene_grid(0)
            blk = Blocks(env, F * 4096); sentinel = blk.raw()
            allocs = lib.hipemu_live_allocs()
            for k in (1, 2, 3, 4, 5):   # class bytes, rows, arguments, bases, the voxel block
                lib.hipemu_fail_alloc_at(k)
                rc = AC.code_of(env, lambda: c.export_sequence_scene_voxels_dev(F, 0.5, blk.a_vox, blk.cap, blk.a_hdr, blk.a_tot, classes=ALL))
                lib.hipemu_fail_alloc_at(0)
                assert rc == E.MOT_E_HIP and lib.hipemu_live_allocs() == allocs, k
                assert all((a == b).all() for a, b in zip(blk.raw(), sentinel)), k
            lib.hipemu_fail_alloc_at(6)   # the getter's table block, behind the five
            n = C.c_long(0); hh = np.zeros(8, np.int32); P = E.MotSceneJudgeParams(1, 1, 2); V = E.MotVoxelParams(0.5, 0.5, 0.5, 1)   # (the C getter itself: the Python one asks the judge first)
            rc = c.lib.mot_get_sequence_scene_voxels(c._h, F, C.byref(P), ALL, C.byref(V), C.c_long(F * 4096), None, C.c_long(0), C.byref(n), hh.ctypes.data_as(C.c_void_p), None)
            lib.hipemu_fail_alloc_at(0)
            assert rc == E.MOT_E_HIP and lib.hipemu_live_allocs() == allocs
            v, h, t = blk.run(c, F, ALL, 0.5)   # (before the model's own getter: that one takes the judge's blocks)
            assert lib.hipemu_live_allocs() == allocs + 5 and h[3] > 0
            blk.free()
            check(env, c, F, ALL, 0.5, "after the failed attempts")
    finally:
        lib.hipemu_fail_alloc_at(0)
