"""Voxel maps merged into one (mot_merge_voxel_maps_dev / mot_merge_voxel_maps, csrc/voxel_merge.hip, csrc/mot_sort.h): bodies shared by
tests/test_emu_voxel_merge.py (emulator) and tests/test_voxel_merge_gpu.py (MI355X). The callers supply a capacity_cases.Env.

The merge is a function of its input arrays alone, so almost every case plants numpy arrays. The yardstick is a numpy model of include/mot.h, "voxel maps merged
into one", that shares no code with the kernels: the fp32 cells (scene_voxel_seq_cases.cells_of: the CELL OF A RECORD rule), a stable np.lexsort, int64 sums, the 64
fp64 accumulators per axis over the terms (double)c * (double)count, one division by the true W. Voxels and header are compared AS BYTES, with sentinel margins round
every block, through the _dev call and through the host call. No tolerance anywhere but the one derived bound of chain_on_device."""
import ctypes as C

import numpy as np

import scene_voxel_seq_cases as SV
import track_accum_cases as AC
import track_link_cases as LC

T = SV.T
VOX = np.dtype([("xyz", "f4", 3), ("count", "i4")])
I32_MAX = 2 ** 31 - 1
KERNELS = (b"voxel_merge_key_kernel", b"voxel_merge_heads_kernel", b"voxel_merge_scan_kernel", b"voxel_merge_runs_kernel", b"voxel_merge_reduce_kernel", b"voxel_merge_kept_kernel")
PER_CALL = [1, 1, 2, 1, 2, 2]   # launches of a merge with an output block (beside the sort's 7 + 7 + 7)
SORT_KERNELS = (b"radix_sort_hist_kernel", b"radix_sort_scan_kernel", b"radix_sort_scatter_kernel")


# ------------------------------------------------------------------------------------------------------------------ the model
def vmap(xyz, count):
    b = np.zeros(len(count), VOX)
    b["xyz"] = np.asarray(xyz, np.float32).reshape(-1, 3); b["count"] = count
    return b


def clamp_count(count, cap):
    return cap if count is None else min(max(int(count), 0), cap)


def model(blocks, counts, leaf, min_points, out_capacity):
    """-> (voxels [n_voxels, 4] int32 (the centroid's bits, the stored count), header [8] int32, facts)"""
    parts = [b[: clamp_count(n, len(b))] for b, n in zip(blocks, counts) if b is not None]
    I = np.concatenate(parts) if parts else np.zeros(0, VOX)
    ok, i = SV.cells_of(I["xyz"], leaf)
    ok &= I["count"] > 0
    pts, cnt, cell = I["xyz"][ok].astype(np.float64), I["count"][ok].astype(np.int64), i[ok]
    order = np.lexsort((cell[:, 0], cell[:, 1], cell[:, 2]))   # stable: a cell's inputs stay in concatenation order
    pts, cnt, cell = pts[order], cnt[order], cell[order]
    n = len(pts)
    head = np.ones(n, bool)
    head[1:] = (cell[1:] != cell[:-1]).any(axis=1)
    starts = np.nonzero(head)[0]
    lens = np.diff(np.append(starts, n))
    W = np.add.reduceat(cnt, starts) if n else np.zeros(0, np.int64)
    kept = W >= min_points
    terms = pts * cnt.astype(np.float64)[:, None]   # one fp64 multiply per coordinate
    cen = centroids(terms, starts[kept], lens[kept], W[kept])
    vox = np.zeros((int(kept.sum()), 4), np.int32)
    vox[:, :3] = cen.view(np.int32); vox[:, 3] = np.minimum(W[kept], I32_MAX)
    nv = len(vox)
    hdr = np.array([len(I), int((~ok).sum()), nv, int((~kept).sum()), min(nv, out_capacity), int((W[kept] > I32_MAX).sum()), 0, 0], np.int32)
    facts = dict(n=len(I), starts=starts, lens=lens, W=W, kept=kept, cells=cell[starts] if n else np.zeros((0, 3), np.int64), keys=SV.keys_of(cell[starts]) if n else np.zeros(0, np.int64))
    return vox, hdr, facts


def centroids(t64, starts, lens, W):
    """include/mot.h, CENTROID: t64 [n, 3] the terms in sorted order, voxel v owns [starts[v], starts[v] + lens[v]) and divides by W[v]"""
    V = len(starts)
    out = np.zeros((V, 3), np.float32)
    if V == 0:
        return out
    lanes = np.arange(64)[None, :]
    rounds = (int(lens.max()) + 63) // 64
    for a in range(3):
        col = t64[:, a]
        acc = np.zeros((V, 64), np.float64)
        for j in range(rounds):
            has = lanes + 64 * j < lens[:, None]
            val = col[np.where(has, starts[:, None] + lanes + 64 * j, 0)]
            acc = np.where(has, val if j == 0 else acc + val, acc)   # (each accumulator starts FROM its first term)
        S = acc[:, 0].copy()
        for l in range(1, 64):
            S = np.where(l < lens, S + acc[:, l], S)
        out[:, a] = (S / W.astype(np.float64)).astype(np.float32)
    return out


def as_words(b):
    return np.ascontiguousarray(b).view(np.int32).reshape(-1, 4)


# ------------------------------------------------------------------------------------------------------------------ the caller's blocks
class Dev:
    """the maps on the device, each in a block of its own between sentinel margins (16 bytes each side), the counts in one int32 array, the output block of
    `out_capacity` voxels and the 32-byte header between margins"""

    def __init__(self, env, blocks, counts, out_capacity):
        self.env, self.cap = env, out_capacity
        self.keep, self.maps = [], []
        self.h_cnt = np.array([-7] + [(-7 if n is None else int(n)) for n in counts] + [-7], np.int32)
        self.p_cnt, self.k_cnt = env.upload(self.h_cnt)
        for k, (b, n) in enumerate(zip(blocks, counts)):
            if b is None:
                self.maps.append((0, 0 if n is None else self.p_cnt + 4 * (k + 1), 0)); self.keep.append(None)
                continue
            h = np.full(4 + len(b) * 4 + 4, -7, np.int32); h[4: 4 + len(b) * 4] = as_words(b).ravel()
            p, keep = env.upload(h)
            assert p % 16 == 0
            self.keep.append((keep, h))
            self.maps.append((p + 16, 0 if n is None else self.p_cnt + 4 * (k + 1), len(b)))
        self.h_out = np.full(4 + out_capacity * 4 + 4, -7, np.int32); self.h_hdr = np.full(2 + 8 + 2, -7, np.int32)
        (self.p_out, self.k_out), (self.p_hdr, self.k_hdr) = env.upload(self.h_out), env.upload(self.h_hdr)
        self.a_out, self.a_hdr = self.p_out + 16, self.p_hdr + 8

    def run(self, c, leaf, min_points=1, out=True):
        c.merge_voxel_maps_dev(self.maps, leaf, self.a_out if out else 0, self.cap if out else 0, self.a_hdr, min_points=min_points)
        c.synchronize()
        return self.read()

    def raw(self):
        return [LC.download(k, h).copy() for k, h in ((self.k_out, self.h_out), (self.k_hdr, self.h_hdr), (self.k_cnt, self.h_cnt))] + [LC.download(*kh).copy() for kh in self.keep if kh]

    def read(self):
        out, hdr = LC.download(self.k_out, self.h_out).copy(), LC.download(self.k_hdr, self.h_hdr).copy()
        assert (out[:4] == -7).all() and (out[4 + self.cap * 4:] == -7).all(), "voxels outside the caller's block"
        assert (hdr[:2] == -7).all() and (hdr[10:] == -7).all(), "the header outside its block"
        return out[4: 4 + self.cap * 4].reshape(self.cap, 4), hdr[2: 10]

    def free(self):
        for k in [self.k_out, self.k_hdr, self.k_cnt] + [kh[0] for kh in self.keep if kh]:
            if hasattr(k, "free"):
                k.free()


def host_call(c, E, blocks, counts, leaf, min_points, out_capacity, with_out=True):
    """the C host call itself -> (rc, n_voxels, header [8], out [out_capacity + 1, 4] with a guard record)"""
    arr = (E.MotVoxelMapSrc * len(blocks))()
    keep = []
    for k, (b, n) in enumerate(zip(blocks, counts)):
        cnt = None if n is None else C.c_int32(int(n))
        b = None if b is None else np.ascontiguousarray(b)
        keep += [cnt, b]
        arr[k] = E.MotVoxelMapSrc(b.ctypes.data if b is not None and len(b) else None, C.addressof(cnt) if cnt is not None else None, 0 if b is None else len(b))
    V = E.voxel_params(leaf, min_points)
    out = np.full((out_capacity + 1, 4), -7, np.int32); hdr = np.full(8, -7, np.int32); n = C.c_long(-7)
    rc = c.lib.mot_merge_voxel_maps(c._h, arr, len(blocks), C.byref(V), out.ctypes.data_as(C.c_void_p) if with_out else None, C.c_long(out_capacity if with_out else 0), C.byref(n),
                                    hdr.ctypes.data_as(C.c_void_p))
    return rc, n.value, hdr, out


def check(env, c, blocks, counts, leaf, what, min_points=1, out_capacity=None, host=True):
    """one _dev merge (and the host call) against the model -> the model's voxels, header and facts"""
    vox, _, _ = model(blocks, counts, leaf, min_points, 0)
    oc = len(vox) + 3 if out_capacity is None else out_capacity
    vox, hdr, facts = model(blocks, counts, leaf, min_points, oc)
    d = Dev(env, blocks, counts, oc)
    before = d.raw()[2:]
    v, h = d.run(c, leaf, min_points)
    assert all((a == b).all() for a, b in zip(d.raw()[2:], before)), (what, "the merge wrote into its inputs")
    d.free()
    assert h.tobytes() == hdr.tobytes(), (what, "header", h.tolist(), hdr.tolist())
    w = min(len(vox), oc)
    if v[:w].tobytes() != vox[:w].tobytes():
        bad = np.argwhere(v[:w] != vox[:w])
        raise AssertionError((what, "voxels", len(bad), "words differ; first", bad[0], v[bad[0][0]], vox[bad[0][0]], "run length", facts["lens"][facts["kept"]][bad[0][0]]))
    assert (v[w:] == -7).all(), (what, "written beyond the kept voxels")
    if host:
        rc, n, gh, out = host_call(c, env.mot, blocks, counts, leaf, min_points, len(vox))
        want = hdr.copy(); want[4] = len(vox)   # (the host call's n_stored: what it copied)
        assert rc == 0 and n == len(vox) and gh.tobytes() == want.tobytes(), (what, "host call", rc, n, gh.tolist(), want.tolist())
        assert out[: len(vox)].tobytes() == vox.tobytes() and (out[len(vox):] == -7).all(), (what, "host call: voxels")
    return vox, hdr, facts


def context(env):
    """the merge needs neither the grid nor the links: the smallest context there is"""
    return env.context(0, max_points=1024, max_batch=1, max_tracks_total=16)


def random_map(rng, n, span=20.0, max_count=20):
    xyz = np.concatenate([rng.uniform(-span, span, (n, 2)), rng.uniform(-2.0, 2.0, (n, 1))], axis=1)
    return vmap(xyz, rng.integers(1, max_count + 1, n))


def poison(n):
    """what must never be read: NaN centroids and finite ones with huge counts, in turn"""
    b = vmap(np.full((n, 3), 0.1, np.float32), np.full(n, 2 ** 30, np.int32))
    b["xyz"][::2] = np.nan; b["count"][::2] = I32_MAX
    return b


# ------------------------------------------------------------------------------------------------------------------ 1: sizes
SIZES = (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 2 * T + 1 + 5000)


def split(rng, total, n_maps):
    """(blocks, counts) of n_maps maps whose clamped counts add up to `total`: tails of poison beyond the count, a count above its capacity, one below 0, a map of
    count 0, a map with NULL voxels and capacity 0"""
    src = random_map(rng, total)
    if n_maps == 1:
        return [np.concatenate([src, poison(5)])], [total]
    if n_maps == 2:
        a = total // 3
        return [np.concatenate([src[:a], poison(3)]), src[a:].copy()], [a, (total - a) + 7]   # (the second count is above its capacity: clamped)
    blocks, counts = [None, poison(9), poison(4)], [None, -3, 0]
    cuts = np.sort(rng.integers(0, total + 1, n_maps - 4))
    parts = np.split(src, cuts)
    for k, p in enumerate(parts):
        mode = k % 3
        if mode == 0:
            blocks.append(p.copy()); counts.append(None)
        elif mode == 1:
            blocks.append(p.copy()); counts.append(len(p) + 1 + k)
        else:
            blocks.append(np.concatenate([p, poison(2 + k)])); counts.append(len(p))
    assert len(blocks) == n_maps
    return blocks, counts


def sizes(env, oracle):
    """total inputs 0, 1, 63, 64, 65, T - 1, T, T + 1, 2 T + 1 and 4.4 tiles over 1, 2 and 16 maps; bytes beyond the clamped counts are never read"""
    rng = np.random.default_rng(11)
    with context(env) as c:
        for total in SIZES:
            for n_maps in (1, 2, 16):
                blocks, counts = split(rng, total, n_maps)
                vox, hdr, facts = check(env, c, blocks, counts, 0.5, ("sizes", total, n_maps), host=(n_maps != 2 or total < T))
                assert hdr[0] == total and hdr[1] == 0, (total, n_maps, hdr.tolist())
                if total >= T - 1:
                    assert 0 < hdr[2] < total, "no two inputs share a cell"


# ------------------------------------------------------------------------------------------------------------------ 2: runs
RUN_LENGTHS = [65, 1, 2, 63, 64, 65, 128, 129, 500] + [1] * 887 + [500] + [1] * 1600 + [129, 65, 64, 1, 2, 128]


def runs(env, oracle):
    """inputs made at a leaf of 0.1 merged at 2x, 4x and 8x of it: cells of 1, 2, 63, 64, 65, 128, 129 and 500 inputs along x (negative and positive indices), a
    64- and a 65-input cell next to each other (the thread path against the wave path), cells that straddle a 2048 boundary of the sorted order, a long first and
    a long last cell; the inputs shuffled over three maps"""
    rng = np.random.default_rng(5)
    with context(env) as c:
        for mult in (2, 4, 8):
            L = np.float32(0.1 * mult)
            ix = np.repeat(np.arange(len(RUN_LENGTHS)) - 1000, RUN_LENGTHS)
            n = len(ix)
            xyz = np.stack([(ix + rng.uniform(0.1, 0.9, n)) * L, rng.uniform(0.1, 0.9, n) * L, -rng.uniform(0.1, 0.9, n) * L], axis=1)
            src = vmap(xyz, rng.integers(1, 6, n))[rng.permutation(n)]
            blocks = [src[: n // 2].copy(), src[n // 2: n // 2 + 700].copy(), src[n // 2 + 700:].copy()]
            vox, hdr, facts = check(env, c, blocks, [None] * 3, float(L), ("runs", mult))
            assert facts["lens"].tolist() == RUN_LENGTHS, "the planted cells are not the model's runs"
            s, e = facts["starts"], facts["starts"] + facts["lens"]
            for edge in (T, 2 * T):
                assert ((s < edge) & (e > edge) & (facts["lens"] > 64)).any(), ("no long run straddles sorted position", edge)
            pairs = list(zip(facts["lens"][:-1].tolist(), facts["lens"][1:].tolist()))
            assert (64, 65) in pairs and (65, 64) in pairs
        vox, hdr, facts = check(env, c, blocks, [None] * 3, 1000.0, "runs, a leaf of 1000 m")   # a few cells along x: a run over more than a tile
        assert hdr[2] <= 3 and facts["lens"].max() > T, (hdr.tolist(), facts["lens"].tolist())


# ------------------------------------------------------------------------------------------------------------------ 3: key digits
def key_digits(env, oracle):
    """inputs whose cells differ in exactly one of the seven key bytes, each byte in turn, from two base cells that have negative and positive indices on every
    axis between them. Leaf 0.5: inv = 2 and the centroids (i + 0.5) * 0.5 are exact, so the planned cells are the model's"""
    X0, Y0, Z0 = 0x0F3C5A, 0x12A4B7, 0x5A3   # biased indices: i_x < 0, i_y > 0, i_z < 0; the second base flips the three signs
    with context(env) as c:
        for base in ((Z0 << 42) | (Y0 << 21) | X0, ((Z0 ^ 0x800) << 42) | ((Y0 ^ 0x100000) << 21) | (X0 ^ 0x100000)):
            for byte in range(7):
                vals = sorted({v & (0x3F if byte == 6 else 0xFF) for v in (0, 1, 0x7F, 0x80, 0xFF)})
                keys = np.array([(base & ~(0xFF << (8 * byte))) | (v << (8 * byte)) for v in vals], np.int64)
                i = np.stack([(keys & 0x1FFFFF) - 2 ** 20, ((keys >> 21) & 0x1FFFFF) - 2 ** 20, (keys >> 42) - 2 ** 11], axis=1)
                xyz = ((i + 0.5) * 0.5).astype(np.float32)
                assert (xyz.astype(np.float64) == (i + 0.5) * 0.5).all()
                order = np.random.default_rng(byte).permutation(len(keys))
                blocks = [vmap(xyz[order], np.arange(1, len(keys) + 1)), vmap(xyz[order[::-1]], np.full(len(keys), 3))]
                vox, hdr, facts = check(env, c, blocks, [None, None], 0.5, ("key digits", hex(base), byte))
                assert facts["keys"].tolist() == sorted(keys.tolist()) and hdr[2] == len(keys) and hdr[1] == 0
                assert len(set((facts["keys"] & ~(0xFF << (8 * byte))).tolist())) == 1


# ------------------------------------------------------------------------------------------------------------------ 4: lattice edges
def lattice_edges(env, oracle):
    """centroids exactly on +-2^20 * leaf (x, y) and +-2^11 * leaf (z), one float below and above; NaN and +-inf in each coordinate; count 0, -1 and INT32_MIN:
    n_outside accounts for each of them. Leaf 0.5: inv = 2, the products are exact"""
    f32 = np.float32
    rows, outside = [], 0
    for a, lim in ((0, 2.0 ** 20), (1, 2.0 ** 20), (2, 2.0 ** 11)):
        edge = f32(lim * 0.5)
        for val, inside in ((-edge, True), (np.nextafter(-edge, f32(0)), True), (np.nextafter(-edge, f32(-np.inf)), False),
                            (edge, False), (np.nextafter(edge, f32(0)), True), (np.nextafter(edge, f32(np.inf)), False)):
            p = [0.25, 0.25, 0.25]; p[a] = val
            rows.append((p, 1)); outside += not inside
        for bad in (np.nan, np.inf, -np.inf):
            p = [0.25, 0.25, 0.25]; p[a] = bad
            rows.append((p, 5)); outside += 1
    for cnt in (0, -1, -2 ** 31):
        rows.append(([0.25, 0.25, 0.25], cnt)); outside += 1
    rows.append(([0.25, 0.25, 0.25], 7))
    src = vmap([r[0] for r in rows], [r[1] for r in rows])
    with context(env) as c:
        for blocks in ([src], [src[::2].copy(), src[1::2].copy()]):
            vox, hdr, facts = check(env, c, blocks, [None] * len(blocks), 0.5, ("lattice edges", len(blocks)))
            assert hdr[0] == len(rows) and hdr[1] == outside, (hdr.tolist(), outside)
            for a, lim in ((0, 2 ** 20), (1, 2 ** 20), (2, 2 ** 11)):
                assert {-lim, lim - 1} <= set(facts["cells"][:, a].tolist()), ("no voxel in the edge cells of axis", a)
        one = vmap([[0.25, 0.25, 0.25]] * 3, [0, -1, -2 ** 31])
        vox, hdr, facts = check(env, c, [one], [None], 0.5, "lattice edges, nothing takes part")
        assert hdr.tolist()[:6] == [3, 3, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------------------ 5: weights
def weights(env, oracle):
    """counts 1 against 2^24 in one cell; three inputs of 2^30 in one cell and two of 2^31 - 1 in another (n_saturated, the stored count 2^31 - 1, the centroid
    still divided by the true W); min_points 1, 2 and 2^30 compared with the summed count, not with the number of inputs"""
    cell = lambda k, u: [k + u, 0.5 + 0.1 * u, 0.25]   # cell k along x at a leaf of 1
    rows = [(cell(0, 0.125), 1), (cell(0, 0.875), 2 ** 24),
            (cell(1, 0.2), 2 ** 30), (cell(1, 0.5), 2 ** 30), (cell(1, 0.9), 2 ** 30),
            (cell(2, 0.3), I32_MAX), (cell(2, 0.7), I32_MAX),
            (cell(3, 0.5), 1),                       # W = 1, one input
            (cell(4, 0.4), 1), (cell(4, 0.6), 1),    # W = 2, two inputs
            (cell(5, 0.5), 2 ** 30),                 # W = 2^30, one input
            (cell(6, 0.1), 2 ** 29), (cell(6, 0.9), 2 ** 29 - 1)]   # W = 2^30 - 1, two inputs
    src = vmap([r[0] for r in rows], [r[1] for r in rows])
    with context(env) as c:
        for mp, kept_cells in ((1, [0, 1, 2, 3, 4, 5, 6]), (2, [0, 1, 2, 4, 5, 6]), (2 ** 30, [1, 2, 5])):
            for blocks in ([src], [src[::2].copy(), src[1::2].copy()]):
                vox, hdr, facts = check(env, c, blocks, [None] * len(blocks), 1.0, ("weights", mp, len(blocks)), min_points=mp)
                got = vox.copy().view(np.float32)[:, 0]
                assert np.floor(got).astype(int).tolist() == kept_cells, (mp, got.tolist())
                assert hdr[5] == 2 and hdr[3] == 7 - len(kept_cells)
                k1, k2 = kept_cells.index(1), kept_cells.index(2)
                assert vox[k1, 3] == I32_MAX and vox[k2, 3] == I32_MAX
                assert 1.2 < got[k1] < 1.9 and 2.3 < got[k2] < 2.7, "a saturated voxel's centroid is not divided by the true W"
                if mp == 1:
                    assert vox[0, 3] == 2 ** 24 + 1 and 0.8749 < got[0] <= 0.875, got[0]


# ------------------------------------------------------------------------------------------------------------------ 6: identity
def lattice_map(rng, n, leaf):
    """one voxel per cell, ascending in (i_z, i_y, i_x), every centroid well inside its cell, counts small enough for centroid * count to be exact in fp64"""
    i = np.unique(np.stack([rng.integers(-60, 60, n), rng.integers(-60, 60, n), rng.integers(-4, 4, n)], axis=1), axis=0)
    i = i[np.lexsort((i[:, 0], i[:, 1], i[:, 2]))]
    return vmap((i + rng.uniform(0.2, 0.8, i.shape)) * leaf, rng.integers(1, 1000, len(i)))


def identity(env, oracle):
    """a map that has one voxel per cell, merged at its own leaf with min_points 1, comes back byte for byte; merged with itself (two inputs on ONE block: inputs
    may overlap each other) every count doubles and every centroid keeps its bytes"""
    rng = np.random.default_rng(17)
    src = lattice_map(rng, 3000, 0.3)
    assert len(src) > T
    with context(env) as c:
        vox, hdr, facts = check(env, c, [src], [None], 0.3, "identity")
        assert vox.tobytes() == as_words(src).tobytes() and hdr.tolist()[:6] == [len(src), 0, len(src), 0, len(src), 0]
        d = Dev(env, [src], [None], len(src))
        d.maps = [d.maps[0], d.maps[0]]
        v, h = d.run(c, 0.3)
        d.free()
        twice, hdr2, _ = model([src, src], [None, None], 0.3, 1, len(src))
        assert v.tobytes() == twice.tobytes() and h.tobytes() == hdr2.tobytes()
        assert (v[:, :3] == vox[:, :3]).all() and (v[:, 3] == 2 * vox[:, 3]).all()


# ------------------------------------------------------------------------------------------------------------------ 7: capacities
def capacities(env, oracle):
    """out_capacity 0, 1, n_voxels - 1, n_voxels and n_voxels + 1: nothing beyond, the header TRUE; no output block; the host call's MOT_E_CAPACITY"""
    rng = np.random.default_rng(23)
    blocks, counts = [random_map(rng, 2500), random_map(rng, 1700)], [None, 1500]
    E = env.mot
    with context(env) as c:
        vox, hdr, facts = check(env, c, blocks, counts, 0.5, "capacities, plain")
        nv = len(vox)
        assert nv > T
        for oc in (0, 1, nv - 1, nv, nv + 1):
            v2, h2, _ = check(env, c, blocks, counts, 0.5, ("capacities", oc), out_capacity=oc, host=False)
            assert h2[2] == nv and h2[4] == min(nv, oc)
        d = Dev(env, blocks, counts, 4)
        v, h = d.run(c, 0.5, out=False)
        d.free()
        assert (v == -7).all() and h[2] == nv and h[4] == 0
        rc, n, gh, out = host_call(c, E, blocks, counts, 0.5, 1, nv - 1)
        want = hdr.copy(); want[4] = 0
        assert rc == E.MOT_E_CAPACITY and n == nv and gh.tobytes() == want.tobytes() and (out == -7).all()
        rc, n, gh, out = host_call(c, E, blocks, counts, 0.5, 1, 0, with_out=False)
        assert rc == 0 and n == nv and gh.tobytes() == want.tobytes(), "no output block: the counts alone"


# ------------------------------------------------------------------------------------------------------------------ 8: contract
def contract(env, oracle):
    """every refusal leaves the caller's blocks unchanged, overlap of the output or the header with an input or a count and misalignment included; the limits
    themselves are served"""
    E = env.mot
    rng = np.random.default_rng(29)
    blocks, counts = [random_map(rng, 300), random_map(rng, 200)], [None, 150]
    nan = float("nan")
    with context(env) as c:
        d = Dev(env, blocks, counts, 600)
        d.run(c, 0.5)
        before = d.raw()
        (v0, c0, cap0), (v1, c1, cap1) = d.maps

        def raw(maps=None, n_maps=None, leaf=(0.5, 0.5, 0.5), min_points=1, out="a", ocap=None, header="a", voxel=True, ctx=True):
            null, maps = maps == "null", (d.maps if maps is None or maps == "null" else maps)
            arr = (E.MotVoxelMapSrc * max(len(maps), 1))(*[E.MotVoxelMapSrc(p or None, n or None, cap) for p, n, cap in maps])
            V = E.MotVoxelParams(leaf[0], leaf[1], leaf[2], min_points)
            ptr = lambda v, a: None if v is None else (a if v == "a" else v)
            return c.lib.mot_merge_voxel_maps_dev(c._h if ctx else None, None if null else arr, len(maps) if n_maps is None else n_maps, C.byref(V) if voxel else None,
                                                  C.c_void_p(ptr(out, d.a_out)), C.c_long(d.cap if ocap is None else ocap), C.c_void_p(ptr(header, d.a_hdr)))
        sixteen = [d.maps[0]] * 16
        for what, kw in (("null context", dict(ctx=False)), ("null maps", dict(maps="null", n_maps=2)), ("null voxel params", dict(voxel=False)), ("null header", dict(header=None)),
                         ("n_maps 0", dict(n_maps=0)), ("n_maps 17", dict(maps=sixteen + [d.maps[1]])), ("negative n_maps", dict(n_maps=-1)),
                         ("leaf NaN", dict(leaf=(nan, 0.5, 0.5))), ("leaf inf", dict(leaf=(0.5, float("inf"), 0.5))), ("leaf below 1e-2", dict(leaf=(0.5, 0.5, 0.009))),
                         ("leaf above 1e3", dict(leaf=(1000.5, 0.5, 0.5))), ("leaf 0", dict(leaf=(0.0, 0.5, 0.5))), ("negative leaf", dict(leaf=(0.5, -0.5, 0.5))),
                         ("min_points 0", dict(min_points=0)), ("min_points 2^30 + 1", dict(min_points=2 ** 30 + 1)), ("negative min_points", dict(min_points=-1)),
                         ("a negative capacity", dict(maps=[(v0, c0, -1), d.maps[1]])), ("the capacities beyond 2^31 - 1", dict(maps=[(v0, c0, 2 ** 30), (v1, c1, 2 ** 30)])),
                         ("a capacity of 2^31", dict(maps=[(v0, c0, 2 ** 31)])), ("null voxels with a capacity", dict(maps=[(0, c0, 5), d.maps[1]])),
                         ("negative out_capacity", dict(ocap=-1)), ("null output with a capacity", dict(out=None)), ("output off 16 bytes", dict(out=d.a_out + 4)),
                         ("output off 16 bytes by 8", dict(out=d.a_out + 8)), ("an input off 16 bytes", dict(maps=[(v0 + 8, c0, cap0 - 1), d.maps[1]])),
                         ("a count off 4 bytes", dict(maps=[d.maps[0], (v1, c1 + 2, cap1)])), ("header off 4 bytes", dict(header=d.a_hdr + 2)),
                         ("the output is an input", dict(out=v0, ocap=cap0)), ("the output ends inside an input", dict(out=v0 - 16, ocap=2)),
                         ("the output starts inside an input", dict(out=v1 + 16 * (cap1 - 1), ocap=4)), ("the output covers a count", dict(out=(c1 & ~15), ocap=1)),
                         ("the header inside an input", dict(header=v1 + 32)), ("the header covers a count", dict(header=c1 - 28)), ("the header is the count's", dict(header=c1))):
            assert raw(**kw) == E.MOT_E_ARG, what
            c.synchronize()
            assert all((a == b).all() for a, b in zip(d.raw(), before)), (what, "a refused call wrote into the caller's blocks")
        assert raw(leaf=(1e-2, 1e3, 0.5), min_points=2 ** 30) == 0 and raw(out=None, ocap=0) == 0 and raw(maps=[(0, 0, 0)]) == 0 and raw(maps=sixteen) == 0, "the limits themselves are served"
        assert raw(out=v0 - 16, ocap=1) == 0, "an output block that ends where an input starts is served (it is that input's margin here)"
        c.synchronize()
        d.free()
        # the host call
        src = blocks[0]
        n = C.c_long(-7); hh = np.full(8, -7, np.int32); out = np.full((8, 4), -7, np.int32)
        one = (E.MotVoxelMapSrc * 1)(E.MotVoxelMapSrc(src.ctypes.data, None, len(src)))
        V = E.voxel_params(0.5, 1)
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        get = lambda h=c._h, maps=one, n_maps=1, V=V, out=None, ocap=0, n=n, hdr=hh: c.lib.mot_merge_voxel_maps(h, maps, n_maps, C.byref(V) if V is not None else None, vp(out), C.c_long(ocap),
                                                                                                             C.byref(n) if n is not None else None, vp(hdr))
        for what, kw in (("null context", dict(h=None)), ("null maps", dict(maps=None)), ("n_maps 0", dict(n_maps=0)), ("n_maps 17", dict(n_maps=17)), ("null voxel params", dict(V=None)),
                         ("a bad leaf", dict(V=E.voxel_params((0.5, 0.001, 0.5), 1))), ("null n_voxels", dict(n=None)), ("null header", dict(hdr=None)), ("negative capacity", dict(ocap=-1)),
                         ("null out with a capacity", dict(ocap=4)), ("a negative capacity", dict(maps=(E.MotVoxelMapSrc * 1)(E.MotVoxelMapSrc(src.ctypes.data, None, -1)))),
                         ("null voxels with a capacity", dict(maps=(E.MotVoxelMapSrc * 1)(E.MotVoxelMapSrc(None, None, 3))))):
            assert get(**kw) == E.MOT_E_ARG, what
        assert n.value == -7 and (hh == -7).all() and (out == -7).all()
        assert get() == 0 and n.value == hh[2] > 0 and hh[4] == 0


# ------------------------------------------------------------------------------------------------------------------ 9: order of maps, determinism
def order_of_maps(env, oracle):
    """swapping two maps changes only what the rule says — the centroids' bytes may differ, the cells and counts may not; the same call twice gives identical bytes"""
    rng = np.random.default_rng(31)
    a, b, c3 = random_map(rng, 2600, span=6.0), random_map(rng, 1900, span=6.0), random_map(rng, 700, span=6.0)
    with context(env) as c:
        v1, h1, f1 = check(env, c, [a, b, c3], [None] * 3, 0.4, "order, a b c")
        v2, h2, f2 = check(env, c, [b, a, c3], [None] * 3, 0.4, "order, b a c", host=False)
        assert h1.tobytes() == h2.tobytes() and (v1[:, 3] == v2[:, 3]).all() and (f1["keys"] == f2["keys"]).all()
        assert f1["lens"].max() > 3, "no cell with inputs of several maps"
        d = Dev(env, [a, b, c3], [None] * 3, len(v1))
        first = [x.tobytes() for x in d.run(c, 0.4)]
        assert [x.tobytes() for x in d.run(c, 0.4)] == first == [v1.tobytes(), h1.tobytes()]
        d.free()


# ------------------------------------------------------------------------------------------------------------------ 10: the chain on the device
def chain_on_device(env, oracle):
    """the one case with a drive: two pieces of three frames. Each piece goes through mot_sequence_products_dev(MOT_SEQ_SCENE) -> mot_export_sequence_scene_voxels_dev
    -> mot_merge_voxel_maps_dev, every count read on the device from the header in front of it, two accumulation blocks used in turn, no host synchronisation until
    the end. Cells and counts equal a numpy thinning of both pieces' records (taken from get_sequence_scene_points in a context that plays the same drive);
    the centroids lie within 2^-22 * max(|coordinate|, leaf) of the one-pass centroid (one float rounding per input centroid, one at the output, doubled); the bytes
    equal the model's. Afterwards the sequence export repeats its bytes, and sequence.play_merged_voxel_map on the same frames gives the chain's result"""
    import importlib
    import scene_grid_seq_cases as SGQ
    E = env.mot
    F, P, stride, leaf, mask = 3, 2, 2048, 0.3, SV.ALL
    clouds, ego_v, yaw = SGQ.drive(env)
    sl = lambda p: slice(p * F, (p + 1) * F)
    recs = []
    with SV.context(env, F, 0.27, 64, stride, 256) as c:   # the records of both pieces
        for p in range(P):
            keep = SGQ.seq_call(env, c, clouds[sl(p)], stride, p * F, ego_v[sl(p)], yaw[sl(p)])
            recs.append(SV.records(c, F, mask)[0])
    cap = F * stride
    with SV.context(env, F, 0.27, 64, stride, 256) as c:
        exp = [SV.Blocks(env, cap) for p in range(P)]
        acc = [Dev(env, [], [], P * cap) for k in range(2)]
        keeps = []
        for p in range(P):
            host = np.zeros((F, stride, 4), np.float32)
            for k, x in enumerate(clouds[sl(p)]):
                host[k, : len(x)] = x
            ptr, keep = env.upload(host); keeps.append(keep)
            c.sequence_products_dev(ptr, stride * 4, [len(x) for x in clouds[sl(p)]], [SGQ.SQ.stamp(p * F + k) for k in range(F)], list(ego_v[sl(p)]), list(yaw[sl(p)]), 0, 0, 0, scene=True)
            c.export_sequence_scene_voxels_dev(F, leaf, exp[p].a_vox, cap, exp[p].a_hdr, 0, classes=mask)
            maps = [(exp[p].a_vox, exp[p].a_hdr + 20, cap)]   # (n_stored of the export's header)
            if p:
                maps = [(acc[(p - 1) % 2].a_out, acc[(p - 1) % 2].a_hdr + 16, P * cap)] + maps   # (n_stored of the earlier merge's header)
            c.merge_voxel_maps_dev(maps, leaf, acc[p % 2].a_out, P * cap, acc[p % 2].a_hdr)
        c.synchronize()
        maps_in = []
        for p in range(P):
            v, h, t = exp[p].read()
            assert h[0] == len(recs[p]) > 0 and h[5] == h[3] > 0, ("the piece's export", p, h.tolist())
            maps_in.append(np.ascontiguousarray(v[: h[5]]).view(VOX).reshape(-1))
        got, gh = acc[(P - 1) % 2].read()
        first, h0, _ = model([maps_in[0]], [None], leaf, 1, P * cap)
        vox, hdr, facts = model([first.view(VOX).reshape(-1), maps_in[1]], [None, None], leaf, 1, P * cap)
        assert gh.tobytes() == hdr.tobytes() and got[: len(vox)].tobytes() == vox.tobytes() and (got[len(vox):] == -7).all(), ("the chain against the model", gh.tolist(), hdr.tolist())
        # ... against one pass over the records of both pieces
        xyz = np.concatenate(recs)
        one, oh, of = SV.model(xyz, len(xyz), leaf, 1, len(xyz), len(xyz))
        assert oh[2] == 0 and gh[1] == 0
        mine = SV.keys_of(SV.cells_of(vox[:, :3].copy().view(np.float32), leaf)[1])
        if len(mine) != len(of["keys"]) or (mine != of["keys"]).any():
            odd = sorted(set(mine.tolist()) ^ set(of["keys"].tolist()))
            raise AssertionError(("a voxel's centroid left its cell: the cells of the chain are not those of one pass; first key", odd[:1], len(mine), len(of["keys"])))
        assert (vox[:, 3] == one[:, 3]).all(), "the counts of the chain are not those of one pass"
        a, b = vox[:, :3].copy().view(np.float32).astype(np.float64), one[:, :3].copy().view(np.float32).astype(np.float64)
        bound = 2.0 ** -22 * np.maximum(np.abs(b), leaf)
        assert (np.abs(a - b) <= bound).all(), ("centroids beyond the derived bound", float((np.abs(a - b) / bound).max()))
        assert len(vox) < len(maps_in[0]) + len(maps_in[1]), "no voxel that both pieces see"
        # non-interference: the sequence export is still valid and repeats its bytes
        again = SV.Blocks(env, cap)
        v, h, t = again.run(c, F, mask, leaf, totals=False)
        v1, h1, t1 = exp[P - 1].read()
        assert v.tobytes() == v1.tobytes() and h.tobytes() == h1.tobytes(), "the sequence export after the merges"
        for b_ in exp + [again] + acc:
            b_.free()
    seq_mod = importlib.import_module(E.__name__ + ".sequence")
    with SV.context(env, F, 0.27, 64, stride, 256) as c:
        merged, heads = seq_mod.play_merged_voxel_map(c, list(zip(clouds[: P * F], ego_v, yaw)), leaf, dt_us=1e5, t0=SGQ.SQ.stamp(0), classes=mask, upload=env.upload)
    assert [h["first_frame"] for h in heads] == [0, F]
    pm = np.zeros((len(merged["count"]), 4), np.int32); pm[:, :3] = np.ascontiguousarray(merged["xyz"], np.float32).view(np.int32).reshape(-1, 3); pm[:, 3] = merged["count"]
    want = hdr.copy(); want[4] = len(vox)
    assert pm.tobytes() == vox.tobytes() and np.frombuffer(merged["header"].tobytes(), np.int32).tobytes() == want.tobytes(), "play_merged_voxel_map against the chain"


# ------------------------------------------------------------------------------------------------------------------ 11: emulator only
def launches_only_in_the_new_calls(env, oracle):
    """emulator: the new kernels' launch counters move in the new calls and nowhere else, by a constant whatever the data and n_maps are; a refused call launches
    and allocates nothing; one block of scratch, grown in place, released by mot_destroy"""
    import scene_grid_seq_cases as SGQ
    lib = env.mot.load_library(env.lib_path)
    lib.hipemu_live_allocs.restype = C.c_long
    count = lambda names=KERNELS: [lib.hipemu_launch_count(k) for k in names]
    rng = np.random.default_rng(37)
    base = lib.hipemu_live_allocs()
    clouds, ego_v, yaw = SGQ.drive(env)
    with SV.context(env, 3, 0.27, 64, 2048, 256) as c:
        before = count()
        keep = SGQ.seq_call(env, c, clouds[:3], 2048, 0, ego_v[:3], yaw[:3])
        c.get_sequence_scene_voxels(3, 0.3, classes=SV.ALL); c.get_sequence_scene_points(3); c.get_scene_grid(0)
        assert count() == before, "a kernel of the merge ran outside it"
        allocs = lib.hipemu_live_allocs()
        for k, (total, n_maps) in enumerate(((1, 1), (2 * T + 9, 16), (300, 2))):
            blocks, counts = split(rng, total, n_maps)
            d = Dev(env, blocks, counts, total)
            arr = (env.mot.MotVoxelMapSrc * 1)(env.mot.MotVoxelMapSrc(d.maps[0][0] or None, None, -1))
            V = env.mot.voxel_params(0.5, 1)
            before, sort_before = count(), count(SORT_KERNELS)
            assert c.lib.mot_merge_voxel_maps_dev(c._h, arr, 1, C.byref(V), C.c_void_p(d.a_out), C.c_long(d.cap), C.c_void_p(d.a_hdr)) == env.mot.MOT_E_ARG
            assert count() == before and lib.hipemu_live_allocs() == allocs + (k > 0), "a refused call allocated or launched"
            d.run(c, 0.5)
            assert count() == [a + b for a, b in zip(before, PER_CALL)] and count(SORT_KERNELS) == [a + 7 for a in sort_before], (total, n_maps)
            assert lib.hipemu_live_allocs() == allocs + 1, "one block of the merge's own"
            d.run(c, 0.5, out=False)
            assert count() == [a + 2 * b - (name == b"voxel_merge_reduce_kernel") for a, b, name in zip(before, PER_CALL, KERNELS)], "no output block: the write launch is left out"
            d.free()
        blocks, counts = split(rng, 700, 2)
        check(env, c, blocks, counts, 0.5, "behind the launches")
        assert lib.hipemu_live_allocs() == allocs + 1, "the host call kept a block"
        c.set_scene_grid(None)
        check(env, c, blocks, counts, 0.5, "with the grid off")
    assert lib.hipemu_live_allocs() == base, "mot_destroy left allocations of the merge behind"


def scratch_under_allocation_failure(env, oracle):
    """emulator: the scratch allocation failing -> MOT_E_HIP, nothing kept, the caller's blocks untouched, the next call gives the model's bytes; the host call's
    blocks (inputs, scratch, output) failing in turn: all or none"""
    lib = env.mot.load_library(env.lib_path)
    lib.hipemu_live_allocs.restype = C.c_long
    lib.hipemu_fail_alloc_at.argtypes = [C.c_long]; lib.hipemu_fail_alloc_at.restype = None
    E = env.mot
    rng = np.random.default_rng(41)
    blocks, counts = split(rng, 900, 2)
    try:
        for grown in (False, True):
            with context(env) as c:
                if grown:
                    check(env, c, [blocks[0][:10].copy()], [None], 0.5, "a small merge first")
                d = Dev(env, blocks, counts, 900)
                sentinel = d.raw()
                allocs = lib.hipemu_live_allocs()
                lib.hipemu_fail_alloc_at(1)
                rc = AC.code_of(env, lambda: c.merge_voxel_maps_dev(d.maps, 0.5, d.a_out, d.cap, d.a_hdr))
                lib.hipemu_fail_alloc_at(0)
                assert rc == E.MOT_E_HIP and lib.hipemu_live_allocs() == allocs - grown, ("the scratch", grown)
                assert all((a == b).all() for a, b in zip(d.raw(), sentinel))
                d.free()
                check(env, c, blocks, counts, 0.5, "after the failed attempt", host=False)
        with context(env) as c:
            check(env, c, [blocks[0][:10].copy()], [None], 0.5, "a small merge first")   # (its scratch is too small for what follows)
            allocs = lib.hipemu_live_allocs()
            for k in (1, 2, 3):   # the staged inputs, the scratch grown, the staged output: all of the call's blocks or none
                lib.hipemu_fail_alloc_at(k)
                rc, n, gh, out = host_call(c, E, blocks, counts, 0.5, 1, 900)
                lib.hipemu_fail_alloc_at(0)
                assert rc == E.MOT_E_HIP and lib.hipemu_live_allocs() == allocs - (k > 1) and (out == -7).all(), k
            check(env, c, blocks, counts, 0.5, "after the host call's failed attempts")
    finally:
        lib.hipemu_fail_alloc_at(0)
