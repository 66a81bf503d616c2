"""Voxel maps indexed and a frame's points judged against the index (mot_index_voxel_maps_dev, mot_export_map_points_dev / mot_get_map_points; csrc/voxel_merge.hip,
csrc/map_judge.hip): bodies shared by tests/test_emu_map_judge.py (emulator) and tests/test_map_judge_gpu.py (MI355X). The callers supply a capacity_cases.Env.

The yardstick is a numpy model written from the prose of include/mot.h that shares no code with the kernels. The index: voxel_merge_cases.model (the merge's cells,
int64 sums and header) without the centroid — keys, saturated counts, header. The judge: the getters that exist without the feature, read BEFORE the call
(get_track_points(rest=True) in both frames: coordinates, owners, indices; get_tracks()["is_static"]), the CELL OF A RECORD rule in np.float32
(scene_voxel_seq_cases.cells_of), and a plain Python set of the index's cells — no search, no keys: a neighbour is the integer triple (i_x + d_x, i_y + d_y, i_z + d_z)
inside the lattice. Index keys, counts and header, segment tables, records and class bytes are compared AS BYTES, between sentinel margins. No tolerance anywhere;
the closed loop's condition is a count that must be zero."""
import ctypes as C
import itertools
from types import SimpleNamespace

import numpy as np

import capacity_cases as CC
import scene_judge_cases as SJ
import scene_voxel_seq_cases as SV
import track_accum_cases as AC
import track_link_cases as LC
import track_point_cases as PC
import voxel_merge_cases as VM

OUTSIDE, MOVING, SPARSE, ABSENT, PRESENT = range(5)
ALL = 0b11111
MASKS = (0, 1, 2, 4, 8, 16, 0b01100, ALL)
I32_MAX = VM.I32_MAX
T = VM.T
VOX = VM.VOX
KERNELS = (b"map_judge_classify_kernel", b"map_judge_scan_kernel", b"map_judge_scatter_kernel")
INDEX_KERNEL = b"voxel_merge_index_kernel"
XY, Z = 2 ** 20, 2 ** 11


# ------------------------------------------------------------------------------------------------------------------ the index: model and blocks
def index_model(blocks, counts, leaf, min_points, capacity):
    """-> (keys [n_voxels] uint64, counts [n_voxels] int32, header [8] int32): the merge's kept cells without the centroid"""
    vox, hdr, facts = VM.model(blocks, counts, leaf, min_points, capacity)
    kept = facts["kept"]
    keys = np.asarray(facts["keys"], np.int64)[kept].astype(np.uint64)
    return keys, vox[:, 3].astype(np.int32), hdr


class Index:
    """the caller's index blocks on the device between sentinel margins: [capacity] uint64 keys (8-byte aligned), [capacity] int32 counts, the 32-byte header; and
    the descriptor"""

    def __init__(self, env, capacity):
        self.env, self.cap = env, capacity
        self.h_keys = np.full(2 + 2 * capacity + 2, -7, np.int32); self.h_cnt = np.full(2 + capacity + 2, -7, np.int32); self.h_hdr = np.full(2 + 8 + 2, -7, np.int32)
        (self.p_keys, self.k_keys), (self.p_cnt, self.k_cnt), (self.p_hdr, self.k_hdr) = env.upload(self.h_keys), env.upload(self.h_cnt), env.upload(self.h_hdr)
        assert self.p_keys % 8 == 0
        self.a_keys, self.a_cnt, self.a_hdr = self.p_keys + 8, self.p_cnt + 8, self.p_hdr + 8
        self.desc = env.mot.voxel_index(self.a_keys, self.a_cnt, self.a_hdr, capacity)

    def run(self, c, maps, leaf, min_points=1):
        c.index_voxel_maps_dev(maps, leaf, self.desc, min_points=min_points)
        c.synchronize()
        return self.read()

    def raw(self):
        return [LC.download(k, h).copy() for k, h in ((self.k_keys, self.h_keys), (self.k_cnt, self.h_cnt), (self.k_hdr, self.h_hdr))]

    def read(self):
        keys, cnt, hdr = self.raw()
        assert (keys[:2] == -7).all() and (keys[2 + 2 * self.cap:] == -7).all(), "keys outside the caller's block"
        assert (cnt[:2] == -7).all() and (cnt[2 + self.cap:] == -7).all(), "counts outside the caller's block"
        assert (hdr[:2] == -7).all() and (hdr[10:] == -7).all(), "the header outside its block"
        return keys[2: 2 + 2 * self.cap].copy().view(np.uint64), cnt[2: 2 + self.cap], hdr[2: 10]

    def free(self):
        for k in (self.k_keys, self.k_cnt, self.k_hdr):
            if hasattr(k, "free"):
                k.free()


SENT64 = np.full(2, -7, np.int32).view(np.uint64)[0]


def check_index(env, c, blocks, counts, leaf, what, min_points=1, capacity=None):
    """one index call against the model -> (keys, counts, header) of the model, and the Index with the call's result (the caller frees it)"""
    keys, cnt, _ = index_model(blocks, counts, leaf, min_points, 0)
    cap = len(keys) + 3 if capacity is None else capacity
    keys, cnt, hdr = index_model(blocks, counts, leaf, min_points, cap)
    d = VM.Dev(env, blocks, counts, 0)
    before = d.raw()[2:]
    x = Index(env, cap)
    k, n, h = x.run(c, d.maps, leaf, min_points)
    assert all((a == b).all() for a, b in zip(d.raw()[2:], before)), (what, "the index call wrote into its inputs")
    assert h.tobytes() == hdr.tobytes(), (what, "header", h.tolist(), hdr.tolist())
    w = min(len(keys), cap)
    assert k[:w].tobytes() == keys[:w].tobytes(), (what, "keys", np.argwhere(k[:w] != keys[:w])[:3].tolist())
    assert n[:w].tobytes() == cnt[:w].tobytes(), (what, "counts", np.argwhere(n[:w] != cnt[:w])[:3].tolist())
    assert (k[w:] == SENT64).all() and (n[w:] == -7).all(), (what, "written beyond the kept cells")
    assert (np.diff(keys.astype(np.int64)) > 0).all(), "the model's keys are strictly ascending"
    lf = SV.leaf3(leaf)
    assert (np.float32(x.desc.leaf_x), np.float32(x.desc.leaf_y), np.float32(x.desc.leaf_z)) == lf and x.desc.reserved == 0, (what, "the descriptor's leaf")
    d.free()
    return (keys, cnt, hdr), x


# ------------------------------------------------------------------------------------------------------------------ 1: index sizes
INDEX_SIZES = (0, 1, T - 1, T, T + 1, 2 * T + 1)


def index_sizes(env, oracle):
    """0, 1, 2047, 2048, 2049 and 4097 inputs over one and over sixteen maps (voxel_merge_cases.split: poison beyond the counts, a device count above its
    capacity and a negative one, a map of count 0, a map with NULL voxels): the sort tile and the run tile are crossed"""
    rng = np.random.default_rng(111)
    with VM.context(env) as c:
        for total in INDEX_SIZES:
            for n_maps in (1, 16):
                blocks, counts = VM.split(rng, total, n_maps)
                (keys, cnt, hdr), x = check_index(env, c, blocks, counts, 0.5, ("index sizes", total, n_maps))
                x.free()
                assert hdr[0] == total and hdr[1] == 0 and hdr[4] == hdr[2] == len(keys)
                if total >= T - 1:
                    assert 0 < len(keys) < total, "no two inputs share a cell"


# ------------------------------------------------------------------------------------------------------------------ 2: cells, orders, weights, digits, edges
def index_cells(env, oracle):
    """cells repeated across maps (counts summed), a sum past 2^31 - 1 stored saturated and counted; inputs in descending and in random cell order; inputs that take
    no part (count <= 0, NaN / inf centroids, cells on and just beyond each lattice edge); keys that differ in exactly one of the seven sort digits; min_points at W
    and W + 1; a cell made of one long run (more than 64 inputs: the wave's path) next to short ones"""
    rng = np.random.default_rng(113)
    with VM.context(env) as c:
        # repeated cells, ascending / descending / random, three maps
        src = VM.lattice_map(rng, 1500, 0.3)
        for name, order in (("ascending", np.arange(len(src))), ("descending", np.arange(len(src))[::-1]), ("random", rng.permutation(len(src)))):
            a = src[order].copy()
            blocks = [a, a[::2].copy(), a[::-3].copy()]
            (keys, cnt, hdr), x = check_index(env, c, blocks, [None] * 3, 0.3, ("index cells", name))
            x.free()
            assert len(keys) == len(src) and int(cnt.astype(np.int64).sum()) == sum(int(b["count"].astype(np.int64).sum()) for b in blocks)
        # weights: voxel_merge_cases.weights' rows; W = 1, 2, 2^30, 2^30 - 1, three times 2^30 and twice 2^31 - 1
        cell = lambda k, u: [k + u, 0.5 + 0.1 * u, 0.25]
        rows = [(cell(0, 0.125), 1), (cell(0, 0.875), 2 ** 24), (cell(1, 0.2), 2 ** 30), (cell(1, 0.5), 2 ** 30), (cell(1, 0.9), 2 ** 30), (cell(2, 0.3), I32_MAX), (cell(2, 0.7), I32_MAX),
                (cell(3, 0.5), 1), (cell(4, 0.4), 1), (cell(4, 0.6), 1), (cell(5, 0.5), 2 ** 30), (cell(6, 0.1), 2 ** 29), (cell(6, 0.9), 2 ** 29 - 1)]
        src = VM.vmap([r[0] for r in rows], [r[1] for r in rows])
        for mp, kept_cells in ((1, 7), (2, 6), (2 ** 30 - 1, 4), (2 ** 30, 3)):   # (W = 2^30 - 1 of cell 6: min_points at W keeps it, at W + 1 drops it)
            for blocks in ([src], [src[::2].copy(), src[1::2].copy()]):
                (keys, cnt, hdr), x = check_index(env, c, blocks, [None] * len(blocks), 1.0, ("index weights", mp, len(blocks)), min_points=mp)
                x.free()
                assert len(keys) == kept_cells and hdr[5] == 2 and int((cnt == I32_MAX).sum()) == 2 and hdr[3] == 7 - kept_cells, (mp, hdr.tolist())
        # one digit at a time (voxel_merge_cases.key_digits' cells)
        X0, Y0, Z0 = 0x0F3C5A, 0x12A4B7, 0x5A3
        for base in ((Z0 << 42) | (Y0 << 21) | X0, ((Z0 ^ 0x800) << 42) | ((Y0 ^ 0x100000) << 21) | (X0 ^ 0x100000)):
            for byte in range(7):
                vals = sorted({v & (0x3F if byte == 6 else 0xFF) for v in (0, 1, 0x7F, 0x80, 0xFF)})
                want = np.array([(base & ~(0xFF << (8 * byte))) | (v << (8 * byte)) for v in vals], np.int64)
                i = np.stack([(want & 0x1FFFFF) - XY, ((want >> 21) & 0x1FFFFF) - XY, (want >> 42) - Z], axis=1)
                xyz = ((i + 0.5) * 0.5).astype(np.float32)
                order = np.random.default_rng(byte).permutation(len(want))
                blocks = [VM.vmap(xyz[order], np.arange(1, len(want) + 1)), VM.vmap(xyz[order[::-1]], np.full(len(want), 3))]
                (keys, cnt, hdr), x = check_index(env, c, blocks, [None, None], 0.5, ("index key digits", hex(base), byte))
                x.free()
                assert keys.astype(np.int64).tolist() == sorted(want.tolist()) and (cnt == np.arange(1, len(want) + 1)[np.argsort(want[order])] + 3).all()
        # the lattice's edges and what takes no part (voxel_merge_cases.lattice_edges' rows)
        f32 = np.float32
        rows, outside = [], 0
        for a, lim in ((0, 2.0 ** 20), (1, 2.0 ** 20), (2, 2.0 ** 11)):
            edge = f32(lim * 0.5)
            for val, inside in ((-edge, True), (np.nextafter(-edge, f32(0)), True), (np.nextafter(-edge, f32(-np.inf)), False), (edge, False), (np.nextafter(edge, f32(0)), True),
                                (np.nextafter(edge, f32(np.inf)), False)):
                p = [0.25, 0.25, 0.25]; p[a] = val
                rows.append((p, 1)); outside += not inside
            for bad in (np.nan, np.inf, -np.inf):
                p = [0.25, 0.25, 0.25]; p[a] = bad
                rows.append((p, 5)); outside += 1
        for n in (0, -1, -2 ** 31):
            rows.append(([0.25, 0.25, 0.25], n)); outside += 1
        rows.append(([0.25, 0.25, 0.25], 7))
        src = VM.vmap([r[0] for r in rows], [r[1] for r in rows])
        (keys, cnt, hdr), x = check_index(env, c, [src[::2].copy(), src[1::2].copy()], [None, None], 0.5, "index lattice edges")
        x.free()
        assert hdr[0] == len(rows) and hdr[1] == outside
        edge_keys = {int(k) & 0x1FFFFF for k in keys} | {(int(k) >> 21) & 0x1FFFFF for k in keys}
        assert {0, 2 * XY - 1} <= edge_keys and {0, 2 * Z - 1} <= {int(k) >> 42 for k in keys}, "no cell on a lattice edge"
        # runs of 1, 64, 65 and 500 inputs side by side: the thread's path against the wave's
        lens = [1, 64, 65, 500, 2, 129, 1, 63]
        ix = np.repeat(np.arange(len(lens)) - 3, lens)
        n = len(ix)
        xyz = np.stack([(ix + rng.uniform(0.1, 0.9, n)) * 0.2, rng.uniform(0.1, 0.9, n) * 0.2, -rng.uniform(0.1, 0.9, n) * 0.2], axis=1)
        src = VM.vmap(xyz, rng.integers(1, 6, n))[rng.permutation(n)]
        (keys, cnt, hdr), x = check_index(env, c, [src[: n // 2].copy(), src[n // 2:].copy()], [None, None], 0.2, "index long runs")
        x.free()
        assert len(keys) == len(lens)


# ------------------------------------------------------------------------------------------------------------------ 3: capacities
def index_capacities(env, oracle):
    """capacity 0, n_voxels - 1 and n_voxels: nothing beyond n_stored is written, the header is true; the same call twice gives the same bytes"""
    rng = np.random.default_rng(127)
    blocks, counts = [VM.random_map(rng, 2500), VM.random_map(rng, 1700)], [None, 1500]
    with VM.context(env) as c:
        (keys, cnt, hdr), x = check_index(env, c, blocks, counts, 0.5, "index capacities, plain")
        first = [a.tobytes() for a in x.raw()]
        d = VM.Dev(env, blocks, counts, 0)
        x.run(c, d.maps, 0.5)
        assert [a.tobytes() for a in x.raw()] == first, "two calls on the same inputs differ"
        d.free(); x.free()
        nv = len(keys)
        assert nv > T
        for cap in (0, nv - 1, nv):
            (k2, n2, h2), x = check_index(env, c, blocks, counts, 0.5, ("index capacities", cap), capacity=cap)
            x.free()
            assert h2[2] == nv and h2[4] == min(nv, cap)


# ------------------------------------------------------------------------------------------------------------------ 4: the index call's refusals
def index_contract(env, oracle):
    """every refusal of the index call leaves the caller's blocks and the descriptor unchanged; the limits themselves are served"""
    E = env.mot
    rng = np.random.default_rng(129)
    blocks, counts = [VM.random_map(rng, 300), VM.random_map(rng, 200)], [None, 150]
    nan = float("nan")
    with VM.context(env) as c:
        d = VM.Dev(env, blocks, counts, 0)
        x = Index(env, 600)
        x.run(c, d.maps, 0.5)
        before = x.raw() + d.raw()
        (v0, c0, cap0), (v1, c1, cap1) = d.maps

        def raw(maps=None, n_maps=None, leaf=(0.5, 0.5, 0.5), min_points=1, keys="a", cnts="a", header="a", cap=None, voxel=True, ctx=True, index=True):
            null, maps = maps == "null", (d.maps if maps is None or maps == "null" else maps)
            arr = (E.MotVoxelMapSrc * max(len(maps), 1))(*[E.MotVoxelMapSrc(p or None, n or None, k) for p, n, k in maps])
            V = E.MotVoxelParams(leaf[0], leaf[1], leaf[2], min_points)
            ptr = lambda v, a: None if v is None else (a if v == "a" else v)
            D = E.MotVoxelIndex(ptr(keys, x.a_keys), ptr(cnts, x.a_cnt), ptr(header, x.a_hdr), x.cap if cap is None else cap, -1.0, -2.0, -3.0, 77)
            rc = c.lib.mot_index_voxel_maps_dev(c._h if ctx else None, None if null else arr, len(maps) if n_maps is None else n_maps, C.byref(V) if voxel else None,
                                                C.byref(D) if index else None)
            return rc, (D.leaf_x, D.leaf_y, D.leaf_z, D.reserved)
        sixteen = [d.maps[0]] * 16
        for what, kw in (("null context", dict(ctx=False)), ("null index", dict(index=False)), ("null header", dict(header=None)), ("null voxel params", dict(voxel=False)),
                         ("null maps", dict(maps="null", n_maps=2)), ("n_maps 0", dict(n_maps=0)), ("n_maps 17", dict(maps=sixteen + [d.maps[1]])), ("leaf NaN", dict(leaf=(nan, 0.5, 0.5))),
                         ("leaf below 1e-2", dict(leaf=(0.5, 0.5, 0.009))), ("leaf above 1e3", dict(leaf=(1000.5, 0.5, 0.5))), ("min_points 0", dict(min_points=0)),
                         ("min_points 2^30 + 1", dict(min_points=2 ** 30 + 1)), ("a negative capacity of a map", dict(maps=[(v0, c0, -1), d.maps[1]])),
                         ("the capacities beyond 2^31 - 1", dict(maps=[(v0, c0, 2 ** 30), (v1, c1, 2 ** 30)])), ("null voxels with a capacity", dict(maps=[(0, c0, 5), d.maps[1]])),
                         ("an input off 16 bytes", dict(maps=[(v0 + 8, c0, cap0 - 1), d.maps[1]])), ("a count off 4 bytes", dict(maps=[d.maps[0], (v1, c1 + 2, cap1)])),
                         ("null keys with a capacity", dict(keys=None)), ("null counts with a capacity", dict(cnts=None)), ("negative capacity", dict(cap=-1)),
                         ("capacity 2^31", dict(cap=2 ** 31)), ("keys off 8 bytes", dict(keys=x.a_keys + 4)), ("counts off 4 bytes", dict(cnts=x.a_cnt + 2)),
                         ("header off 4 bytes", dict(header=x.a_hdr + 2)), ("the keys are an input", dict(keys=v0, cap=cap0)), ("the keys end inside an input", dict(keys=v0 - 16, cap=3)),
                         ("the counts start inside an input", dict(cnts=v1 + 16 * (cap1 - 1), cap=8)), ("the keys cover a count", dict(keys=(c1 & ~7), cap=1)),
                         ("the counts are the count words", dict(cnts=c1, cap=1)), ("the header inside an input", dict(header=v1 + 32)), ("the header is the count's", dict(header=c1)),
                         ("keys and counts overlap", dict(cnts=x.a_keys + 8, cap=4)), ("the header inside the keys", dict(header=x.a_keys + 16)),
                         ("the header inside the counts", dict(header=x.a_cnt + 4))):
            rc, left = raw(**kw)
            assert rc == E.MOT_E_ARG, what
            assert left == (-1.0, -2.0, -3.0, 77), (what, "a refused call wrote into the descriptor")
            c.synchronize()
            assert all((a == b).all() for a, b in zip(x.raw() + d.raw(), before)), (what, "a refused call wrote into the caller's blocks")
        for what, kw in (("the limits", dict(leaf=(1e-2, 1e3, 0.5), min_points=2 ** 30)), ("capacity 0 without blocks", dict(keys=None, cnts=None, cap=0)), ("an empty map", dict(maps=[(0, 0, 0)])),
                         ("sixteen maps", dict(maps=sixteen)), ("keys that end where an input starts", dict(keys=v0 - 16, cap=2))):
            rc, left = raw(**kw)
            assert rc == 0 and left[3] == 0, (what, "is served")
        c.synchronize()
        d.free(); x.free()


# ------------------------------------------------------------------------------------------------------------------ the judge: model and blocks
def observe(c, b):
    """everything the verdicts of slot b depend on beside the index, from the getters that exist without the feature"""
    rg = c.get_track_points(b, rest=True, frame="global"); rs = c.get_track_points(b, rest=True, frame="sensor")
    idx = rg["index"]; n = len(idx)
    assert np.array_equal(idx, rs["index"]) and np.array_equal(np.sort(idx), np.arange(n))
    glob = np.zeros((n, 3), np.float32); sensor = np.zeros((n, 3), np.float32); ids = np.full(n, -1, np.int64)
    glob[idx] = rg["xyz"]; sensor[idx] = rs["xyz"]; ids[idx] = SJ.SG.owners(rg)
    static_flag = c.get_tracks(b)["is_static"]
    owned = ids >= 0
    flagged = np.zeros(n, bool); flagged[owned] = static_flag[ids[owned]] != 0
    return dict(n=n, glob=glob, sensor=sensor, ids=ids, owned=owned, flagged=flagged, moving=owned & ~flagged)


def cell_set(keys, counts, n):
    """the index as the prose has it: the cells among keys[0..n) and their counts"""
    k = keys[:n].astype(np.int64)
    cells = zip(((k & 0x1FFFFF) - XY).tolist(), (((k >> 21) & 0x1FFFFF) - XY).tolist(), ((k >> 42) - Z).tolist())
    return dict(zip(cells, counts[:n].tolist()))


def classify(o, cells, leaf, min_count, reach):
    """the rules of include/mot.h in their order; cells: {(i_x, i_y, i_z): count}"""
    ok, i = SV.cells_of(o["glob"], leaf)
    cls = np.full(o["n"], ABSENT, np.uint8)
    offs = list(itertools.product(range(-reach, reach + 1), repeat=3))
    memo = {}
    for p in np.nonzero(ok & ~o["moving"])[0]:
        me = (int(i[p, 0]), int(i[p, 1]), int(i[p, 2]))
        if me not in memo:
            seen = full = False
            for dx, dy, dz in offs:
                nb = (me[0] + dx, me[1] + dy, me[2] + dz)
                if not (-XY <= nb[0] < XY and -XY <= nb[1] < XY and -Z <= nb[2] < Z):
                    continue   # (a neighbour outside the lattice is in no map)
                if nb in cells:
                    seen = True; full |= cells[nb] >= min_count
            memo[me] = PRESENT if full else (SPARSE if seen else ABSENT)
        cls[p] = memo[me]
    cls[~ok] = OUTSIDE
    cls[o["moving"]] = MOVING
    return cls


class Blocks(SJ.Blocks):
    """scene_judge_cases.Blocks (sentinel-filled records, segments and class bytes) filled by mot_export_map_points_dev"""

    def run(self, c, batch, index, mask, frame, params=(1, 0), points=True, classes=True):
        c.export_map_points_dev(batch, index, self.a_pts if points else 0, self.ps if points else 0, self.a_seg, self.a_cls if classes else 0, self.cs, min_count=params[0],
                                reach=params[1], classes=mask, frame=frame)
        c.synchronize()
        return self.read(batch)


def check_getter(c, b, index, o, cls, mask, frame, params, what):
    r = c.get_map_points(b, index, min_count=params[0], reach=params[1], classes=mask, frame=frame)
    seg, rec = SJ.records(o, cls, mask, frame)
    got = np.zeros((len(r["index"]), 4), np.int32); got[:, :3] = np.ascontiguousarray(r["xyz"], np.float32).view(np.int32).reshape(-1, 3); got[:, 3] = r["index"]
    assert r["segments"].tobytes() == seg.tobytes() and got.tobytes() == rec.tobytes() and r["classes"].tobytes() == cls.tobytes(), (what, "slot", b, "getter")


def judge_and_check(env, c, B, x, model_index, leaf, params_list, what, facts=None, mask=ALL, frame="global", obs=None, getter=True):
    """the model from the getters first, then the export and the getter for every parameter set. x: the Index; model_index: (keys, counts, n)"""
    obs = obs or [observe(c, b) for b in range(B)]
    cells = cell_set(*model_index)
    stride = max(max(o["n"] for o in obs), 1) + 3
    out_cls = []
    for params in params_list:
        cls = [classify(o, cells, leaf, *params) for o in obs]
        blk = Blocks(env, B, stride, stride)
        out = blk.run(c, B, x.desc, mask, frame, params)
        for b in range(B):
            SJ.check_slot(blk, out, b, obs[b], cls[b], mask, frame, (what, params))
            if getter:
                check_getter(c, b, x.desc, obs[b], cls[b], mask, frame, params, (what, params))
            if facts is not None:
                for k, name in enumerate(("outside", "moving", "sparse", "absent", "present")):
                    facts[name] = facts.get(name, 0) + int((cls[b] == k).sum())
        blk.free()
        out_cls.append(cls)
    return obs, out_cls


def centroid_in(i, leaf):
    """a float32 point whose cell, by the model's rule, is the integer triple i (near a lattice edge (i + 0.5) * leaf may round out of the cell)"""
    lf = np.array(SV.leaf3(leaf), np.float64)
    for u in (0.5, 0.375, 0.625, 0.25, 0.75, 0.125, 0.875):
        p = ((np.asarray(i, np.float64) + u) * lf).astype(np.float32)
        ok, got = SV.cells_of(p[None, :], leaf)
        if ok[0] and got[0].tolist() == [int(v) for v in i]:
            return p
    raise AssertionError(("no float32 point in cell", i, leaf))


def plant(cells_counts, leaf):
    """a voxel map (one input per cell) whose model cells are exactly the given ones: [((i_x, i_y, i_z), count)]"""
    if not cells_counts:
        return VM.vmap(np.zeros((0, 3), np.float32), np.zeros(0, np.int32))
    return VM.vmap(np.stack([centroid_in(i, leaf) for i, _ in cells_counts]), [n for _, n in cells_counts])


def make_index(env, c, cells_counts, leaf, what, extra_capacity=3):
    """plant, index on the device (checked against the index model) -> (Index, (keys, counts, n))"""
    src = plant(cells_counts, leaf)
    (keys, cnt, hdr), x = check_index(env, c, [src], [None], leaf, what, capacity=len(src) + extra_capacity)
    assert len(keys) == len({i for i, _ in cells_counts}), (what, "the planted cells are not the model's")
    return x, (keys, cnt, int(hdr[4]))


def frame_cells(obs, leaf):
    """the distinct cells of the frames' points that are judged by cell (not moving, inside the lattice), ascending in key order"""
    got = set()
    for o in obs:
        ok, i = SV.cells_of(o["glob"], leaf)
        got |= {tuple(r) for r in i[ok & ~o["moving"]].tolist()}
    return sorted(got, key=lambda t: (t[2], t[1], t[0]))


def filler(n, leaf, below):
    """n cells far from every frame: a row at the lattice's lowest (highest) z"""
    z = -Z + 1 if below else Z - 2
    return [((k - n // 2, 7, z), 4) for k in range(n)]


# ------------------------------------------------------------------------------------------------------------------ 5: shapes
def shapes(env, oracle, order_any=False):
    """elevated counts 0, 1, 63, 64, 65, the chunk (2048) - 1 / exact / + 1, 5000 and a full frame (track_point_cases.shape_frames), ten slots with different ego
    poses, two steps; an index of about 5000 cells that holds a third of the frames' cells at min_count, a third below it and leaves a third out, at leaves 0.25
    and 0.1; min_count at a cell's count and one above it; reach 0 and 1; every mask in both frames; strides one below and at a slot's need, a block 4 bytes off,
    counts alone, no class block; the getter"""
    frames = PC.shape_frames(oracle)
    targets = [len(x) for x in frames[0]]
    assert {0, 1, 63, 64, 65, 2047, 2048, 2049, 5000} <= set(targets)
    B = len(targets)
    facts = {}
    rng = np.random.default_rng(131)
    with env.context(0, max_points=8192, max_batch=B, max_tracks_total=512) as c:
        c.set_track_links(True)
        if order_any:
            c.set_point_order(env.mot.MOT_ORDER_ANY)
        for f in range(2):
            sent = [np.ascontiguousarray(x[np.random.default_rng(7 + b).permutation(len(x))]) for b, x in enumerate(frames[f])] if order_any else frames[f]
            keep = AC.launch(env, c, sent, 8192, f, ego_v=[0.5 * b for b in range(B)], yaw=[0.03 * b * f for b in range(B)])
            obs = [observe(c, b) for b in range(B)]
            assert [o["n"] for o in obs] == targets
            leaf = (0.25, 0.1)[f]
            cells = frame_cells(obs, leaf)
            role = rng.integers(0, 3, len(cells))
            planted = [(i, 5) for i, r in zip(cells, role) if r == 0] + [(i, 2) for i, r in zip(cells, role) if r == 1]
            planted += filler(max(5000 - len(planted), 10) // 2, leaf, True) + filler(max(5000 - len(planted), 10) // 2, leaf, False)
            x, mi = make_index(env, c, planted, leaf, ("shapes index", order_any, f))
            obs, cls = judge_and_check(env, c, B, x, mi, leaf, ((5, 0), (6, 0), (5, 1), (1, 1)), ("shapes", order_any, f), facts, obs=obs, getter=False)
            params = (5, 0)
            cls = cls[0]
            full = max(targets) + 3
            for mask in MASKS:
                for frame in ("global", "sensor"):
                    blk = Blocks(env, B, full, full)
                    out = blk.run(c, B, x.desc, mask, frame, params)
                    for b in range(B):
                        SJ.check_slot(blk, out, b, obs[b], cls[b], mask, frame, ("shapes", order_any, f, mask, frame))
                    blk.free()
            for b in (1, 4, 7, 9):   # 1, 65, 2049 points and the full frame through the getter
                for mask, frame in ((ALL, "global"), (0b01100, "sensor"), (0, "global")):
                    check_getter(c, b, x.desc, obs[b], cls[b], mask, frame, params, ("shapes", order_any, f, mask, frame))
            for b in (7, 9):
                for mask in (ALL, 0b11000):
                    need = int(sum((cls[b] == k).sum() for k in range(5) if (mask >> k) & 1))
                    for ps, cs, mis in ((max(need - 1, 0), targets[b] - 1, False), (need, targets[b], True)):
                        blk = Blocks(env, B, ps, cs, misalign=mis)
                        out = blk.run(c, B, x.desc, mask, "global", params)
                        for k in range(B):
                            SJ.check_slot(blk, out, k, obs[k], cls[k], mask, "global", ("shapes, strides", order_any, f, b, mask, ps, cs))
                        blk.free()
            blk = Blocks(env, B, 0, full)
            out = blk.run(c, B, x.desc, 0, "global", params, points=False)
            for b in range(B):
                SJ.check_slot(blk, out, b, obs[b], cls[b], 0, "global", ("shapes, counts and classes alone", order_any, f), points=False)
            blk.free()
            blk = Blocks(env, B, 0, 0)
            out = blk.run(c, B, x.desc, 0, "sensor", params, points=False, classes=False)
            for b in range(B):
                SJ.check_slot(blk, out, b, obs[b], cls[b], 0, "sensor", ("shapes, counts alone", order_any, f), points=False, classes=False)
            blk.free()
            blk = Blocks(env, B, full, full)
            out = blk.run(c, B, x.desc, ALL, "sensor", params, classes=False)
            for b in range(B):
                SJ.check_slot(blk, out, b, obs[b], cls[b], ALL, "sensor", ("shapes, no class block", order_any, f), classes=False)
            blk.free()
            x.free()
    for k in ("moving", "sparse", "absent", "present"):
        assert facts.get(k, 0) > 0, (k, facts)
    return facts


# ------------------------------------------------------------------------------------------------------------------ 6: index lengths
def wall(rng, x0, y0, x1, y1, z0, z1, n):
    """n points along a strip: a cluster too long for a box, so its points belong to no track — they are judged by cell"""
    t = rng.uniform(0, 1, n); q = np.zeros((n, 4), np.float32)
    q[:, 0] = x0 + t * (x1 - x0) + rng.uniform(-.1, .1, n); q[:, 1] = y0 + t * (y1 - y0) + rng.uniform(-.1, .1, n); q[:, 2] = rng.uniform(z0, z1, n)
    return q


def scene(seed, n_blobs=16):
    """capacity_cases.small_scene (box-sized blobs: owned points, MOVING while their tracks are young) and two 40 m walls (unowned points, negative and positive
    coordinates)"""
    rng = np.random.default_rng(1000 + seed)
    return np.concatenate([CC.small_scene(seed, n_blobs), wall(rng, -20, 12, 20, 12, -0.9, 0.3, 450), wall(rng, -12, -20, -12, 20, -0.9, 0.3, 450)])


def small_frames(env, c, f=0, B=3, stride=2048):
    clouds = [scene(f + 2 * b) for b in range(B)]
    keep = AC.launch(env, c, clouds, stride, f, ego_v=[0.0, 3.0, 8.0][:B], yaw=[0.0, 0.1 * f, -0.2 * f][:B])
    return keep


def index_lengths(env, oracle):
    """index lengths 0, 1, 2, 1023, 1024, 1025 and about 5000 (whatever sampling the search uses is straddled), the frames' cells in the middle of the index, at its
    start and at its end; points whose key is below the first and above the last key of the index; the device length clamped: an n_stored above the capacity and a
    negative one, planted in the header"""
    leaf = 0.25
    seen = dict(below=0, above=0)
    with env.context(0, max_points=2048, max_batch=3, max_tracks_total=64) as c:
        c.set_track_links(True)
        for f in range(2):
            keep = small_frames(env, c, f)
        obs = [observe(c, b) for b in range(3)]
        cells = frame_cells(obs, leaf)
        assert len(cells) > 40
        mid = cells[len(cells) // 2]
        for length in (0, 1, 2, 1023, 1024, 1025, 5000):
            for where in ("middle", "start", "end"):
                if length <= 2:
                    planted = [(i, 3) for i in cells[len(cells) // 2: len(cells) // 2 + length]]
                    if where != "middle":
                        continue
                else:
                    mine = [(i, 3) for i in cells[:: 2]][: length // 2]
                    rest = length - len(mine)
                    lo = rest // 2 if where == "middle" else (0 if where == "start" else rest)
                    planted = mine + filler(lo, leaf, True) + filler(rest - lo, leaf, False)
                x, mi = make_index(env, c, planted, leaf, ("index lengths", length, where))
                assert mi[2] == length
                judge_and_check(env, c, 3, x, mi, leaf, ((3, 0), (4, 1)), ("index lengths", length, where), obs=obs, getter=(length in (0, 1025)))
                if length:
                    k = np.concatenate([SV.keys_of(SV.cells_of(o["glob"], leaf)[1][SV.cells_of(o["glob"], leaf)[0]]) for o in obs])
                    seen["below"] += int((k < int(mi[0][0])).sum()); seen["above"] += int((k > int(mi[0][length - 1])).sum())
                if length == 1025 and where == "middle":   # the length is the DEVICE's word, clamped there
                    for planted_n, n in ((x.cap + 1000, x.cap), (-5, 0), (17, 17)):   # a header of the test's own in front of the same keys and counts
                        hdr = LC.download(x.k_hdr, x.h_hdr).copy()
                        hdr[2 + 4] = planted_n
                        p_hdr, k_hdr = env.upload(hdr)
                        other = SimpleNamespace(desc=env.mot.voxel_index(x.a_keys, x.a_cnt, p_hdr + 8, x.cap, leaf))
                        # (n = capacity reads the three sentinel keys beyond the stored cells, all above every cell's key: they match no point)
                        judge_and_check(env, c, 3, other, (mi[0], mi[1], min(n, length)), leaf, ((3, 0), (3, 1)), ("index lengths, n_stored planted", planted_n), obs=obs, getter=False)
                        if hasattr(k_hdr, "free"):
                            k_hdr.free()
                x.free()
    assert seen["below"] > 0 and seen["above"] > 0, seen


# ------------------------------------------------------------------------------------------------------------------ 7: neighbours
DIRECTIONS = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 1), (-1, 1, -1))


def neighbours(env, oracle):
    """reach 1 with the own cell absent and the ONLY cell of the map at +x, -x, +y, -y, +z, -z and at two diagonals of a chosen point's cell (PRESENT; reach 0 on the
    same data: ABSENT); the own cell sparse and a neighbour full (reach 0 SPARSE, reach 1 PRESENT); the own cell and a neighbour both sparse (SPARSE at both);
    min_count equal to a cell's count (PRESENT) and one above it (SPARSE); negative coordinates (floorf)"""
    leaf = 0.25
    with env.context(0, max_points=2048, max_batch=3, max_tracks_total=64) as c:
        c.set_track_links(True)
        for f in range(2):
            keep = small_frames(env, c, f)
        obs = [observe(c, b) for b in range(3)]
        ok, i = SV.cells_of(obs[1]["glob"], leaf)
        cand = np.nonzero(ok & ~obs[1]["moving"] & (i < 0).any(axis=1))[0]
        assert len(cand), "no point with a negative cell index"
        p = int(cand[len(cand) // 2])
        me = tuple(int(v) for v in i[p])
        for d in DIRECTIONS:
            nb = (me[0] + d[0], me[1] + d[1], me[2] + d[2])
            x, mi = make_index(env, c, [(nb, 4)], leaf, ("neighbours", d))
            o, cls = judge_and_check(env, c, 3, x, mi, leaf, ((4, 0), (4, 1), (5, 1)), ("neighbours", d), obs=obs, getter=False)
            assert cls[0][1][p] == ABSENT and cls[1][1][p] == PRESENT and cls[2][1][p] == SPARSE, (d, [k[1][p] for k in cls])
            x.free()
        nb = (me[0] - 1, me[1] + 1, me[2])
        x, mi = make_index(env, c, [(me, 2), (nb, 9)], leaf, "neighbours, own sparse and a neighbour full")
        o, cls = judge_and_check(env, c, 3, x, mi, leaf, ((5, 0), (5, 1), (2, 0), (3, 0), (9, 1), (10, 1)), "neighbours, own sparse and a neighbour full", obs=obs)
        assert [k[1][p] for k in cls] == [SPARSE, PRESENT, PRESENT, SPARSE, PRESENT, SPARSE]
        x.free()


# ------------------------------------------------------------------------------------------------------------------ 8: lattice edges
EDGE_PARAMS = dict(t_hmin=-40.0, t_hmax=-30.0)   # (no ground within reach: points 20 m below the sensor stay elevated)


def lattice_edges(env, oracle):
    """points in the lattice's last cells: i_x = -2^20 and i_x = 2^20 - 1 (two streams that drive 10485.76 m along -x and +x, a leaf of 0.01), i_z = 2^11 - 1 and
    i_z = -2^11 (strips 20.48 m above and below the sensor), points beyond each edge (OUTSIDE). For a point of an edge cell the map holds NOTHING but the cell a
    carrying key addition or subtraction (a wrapping index) would hit — the first cell of the next row, the last cell of the row below, the other end of the z axis:
    reach 1 must say ABSENT. Then the true neighbour inside the lattice is planted as well: PRESENT"""
    leaf = 0.01
    rng = np.random.default_rng(137)
    hits = {}
    with env.context(0, pkw=EDGE_PARAMS, max_points=4096, max_batch=2, max_tracks_total=64) as c:
        c.set_track_links(True)
        turn = [np.pi / 2, -np.pi / 2]
        for f, (v, yaw) in enumerate(((0.0, [0.0, 0.0]), (0.0, turn), (104857.6, turn))):
            extra = np.concatenate([wall(rng, -18, 5, 18, 8, 20.38, 20.58, 600), wall(rng, -18, -8, 18, -5, -20.58, -20.38, 600)])
            clouds = [np.concatenate([scene(f + 2 * b), extra]) for b in range(2)]
            keep = AC.launch(env, c, clouds, 4096, f, ego_v=[v, v], yaw=yaw)
        obs = [observe(c, b) for b in range(2)]
        edge_of = {"x-": (0, -XY), "x+": (0, XY - 1), "z-": (2, -Z), "z+": (2, Z - 1)}
        for name, (axis, at) in edge_of.items():
            for b in range(2):
                ok, i = SV.cells_of(obs[b]["glob"], leaf)
                on_edge = np.nonzero(ok & ~obs[b]["moving"] & (i[:, axis] == at))[0]
                if not len(on_edge):
                    continue
                assert (~ok).any(), "no point beyond the lattice"
                p = int(on_edge[0])
                me = [int(v) for v in i[p]]
                # the cells a carry / a wrap would wrongly hit for the neighbour beyond the edge, (d_y, d_z) all nine where they exist
                wrong = []
                for dy, dz in itertools.product((-1, 0, 1), repeat=2):
                    if axis == 0:
                        w = (-at - 1, me[1] + dy + (1 if at > 0 else -1), me[2] + dz)   # the other end of the row above / below
                        w2 = (-at - 1, me[1] + dy, me[2] + dz)                             # ... and of the same row (a wrap inside the field)
                    else:
                        w = (me[0] + dy, me[1] + dz, -at - 1)                              # the other end of the z axis
                        w2 = w
                    for cell in (w, w2):
                        if -XY <= cell[0] < XY and -XY <= cell[1] < XY and -Z <= cell[2] < Z:
                            wrong.append(cell)
                wrong = sorted(set(wrong))
                x, mi = make_index(env, c, [(w, 9) for w in wrong], leaf, ("lattice edges, the wrong cells", name, b))
                o, cls = judge_and_check(env, c, 2, x, mi, leaf, ((1, 1), (1, 0)), ("lattice edges, the wrong cells", name, b), obs=obs, getter=False)
                assert cls[0][b][p] == ABSENT, (name, b, "a neighbour beyond the lattice edge was found in the map: the key arithmetic carried or wrapped")
                x.free()
                inward = list(me); inward[axis] += 1 if at < 0 else -1
                x, mi = make_index(env, c, [(w, 9) for w in wrong] + [(tuple(inward), 9)], leaf, ("lattice edges, the true neighbour", name, b))
                o, cls = judge_and_check(env, c, 2, x, mi, leaf, ((1, 1), (1, 0)), ("lattice edges, the true neighbour", name, b), obs=obs)
                assert cls[0][b][p] == PRESENT and cls[1][b][p] == ABSENT
                x.free()
                hits[name] = hits.get(name, 0) + 1
    assert set(hits) == set(edge_of), ("the frames do not reach every lattice edge", hits)


# ------------------------------------------------------------------------------------------------------------------ 9: kinds, non-finite coordinates
def kinds_and_outside(env, oracle):
    """owned points of static and of dynamic tracks (scene_judge_cases.standing_and_moving's scene: two blobs stand in the world, one moves), MOVING inside and outside
    the map alike; a point whose global z is not finite (OUTSIDE); the scene grid off and on with identical bytes, and its validity left alone"""
    frames_n, B = 12, 3
    SG = SJ.SG
    ego_v = [0.0, 1.0, 1.0]; yaws = [[0.0, 0.0, 0.04 * f] for f in range(frames_n)]
    S = SG.sensor_from_world(env, ego_v, yaws, frames_n)
    facts = {}
    leaf = 0.5
    runs = {}
    for grid in (False, True):
        rngs = [np.random.default_rng(3 + b) for b in range(B)]
        out = []
        with env.context(0, max_points=2048, max_batch=B, max_tracks_total=256) as c:
            c.set_track_links(True)
            if grid:
                c.set_scene_grid(1.0, 64)
            for f in range(frames_n):
                world = lambda b: np.concatenate([SG.world_blob(rngs[b], 8.0, 5.0), SG.world_blob(rngs[b], 3.0, -7.0), SG.world_blob(rngs[b], -9.0, -6.0 - 0.3 * f)])
                clouds = [SG.to_sensor(S[f, b], world(b)) for b in range(B)]
                clouds[0] = np.concatenate([clouds[0], np.array([[5.0, 5.0, np.inf, 0.0], [5.1, 5.0, np.nan, 0.0]], np.float32)])
                keep = AC.launch(env, c, clouds, 2048, f, ego_v=ego_v, yaw=yaws[f])
                if f < frames_n - 3:
                    continue
                obs = [observe(c, b) for b in range(B)]
                cells = frame_cells(obs, leaf)
                x, mi = make_index(env, c, [(i, 3 + (k % 2)) for k, i in enumerate(cells[::2])], leaf, ("kinds index", grid, f))
                if grid:
                    hdr = [c.get_scene_grid(b, cells=False)["header"].tobytes() for b in range(B)]
                o, cls = judge_and_check(env, c, B, x, mi, leaf, ((4, 0), (3, 1)), ("kinds", grid, f), facts, obs=obs)
                blk = Blocks(env, B, 2048, 2048)
                blk.run(c, B, x.desc, ALL, "global", (4, 1))
                out.append([a.tobytes() for a in blk.raw()])
                blk.free(); x.free()
                if grid:
                    assert [c.get_scene_grid(b, cells=False)["header"].tobytes() for b in range(B)] == hdr
                    c.accumulate_scene(B)   # (still accepted: the judge consumed no step)
                facts["nonfinite"] = facts.get("nonfinite", 0) + int((~np.isfinite(obs[0]["glob"])).any(axis=1).sum())
                facts["static_owned"] = facts.get("static_owned", 0) + sum(int((o_["owned"] & o_["flagged"]).sum()) for o_ in obs)
        runs[grid] = out
    assert runs[False] == runs[True], "the scene grid changes the judge's bytes"
    for k in ("outside", "moving", "sparse", "absent", "present", "nonfinite", "static_owned"):
        assert facts.get(k, 0) > 0, (k, facts)
    return facts


# ------------------------------------------------------------------------------------------------------------------ 10: the closed loop
def closed_loop(env, oracle):
    """a map and a frame made by the same device functions agree on cells. A fused frame's MOT_FRAME_GLOBAL records, each a voxel of count 1, merged
    (mot_merge_voxel_maps, min_points 1) at leaf L; that map indexed at L; the same frame judged at reach 0, min_count 1: among the points that are neither MOVING nor
    OUTSIDE the number of ABSENT and of SPARSE is ZERO — a condition, not a tolerance (a centroid is an fp64 mean of floats rounded to float, hence within [min, max]
    of them, and fl(x * inv) is monotone in x). First with the numpy model alone, then on the device; at leaves 0.25 (an exact reciprocal) and 0.1 (none)"""
    with env.context(0, max_points=2048, max_batch=3, max_tracks_total=64) as c:
        c.set_track_links(True)
        for f in range(3):
            keep = small_frames(env, c, f)
        obs = [observe(c, b) for b in range(3)]
        for leaf in (0.25, 0.1):
            for b in range(3):
                o = obs[b]
                recs = VM.vmap(o["glob"], np.ones(o["n"], np.int32))
                # the numpy model alone
                vox, hdr, facts = VM.model([recs], [None], leaf, 1, o["n"])
                merged = np.ascontiguousarray(vox).view(VOX).reshape(-1)
                keys, cnt, ih = index_model([merged], [None], leaf, 1, len(merged))
                cls = classify(o, cell_set(keys, cnt, len(keys)), leaf, 1, 0)
                assert int(((cls == ABSENT) | (cls == SPARSE)).sum()) == 0, ("the model: a centroid left its records' cell", leaf, b)
                assert len(keys) == len(merged), "two voxels of the map share a cell"
                # the library: the host merge, the map uploaded and indexed, the frame judged
                m = c.merge_voxel_maps([dict(xyz=o["glob"], count=np.ones(o["n"], np.int32))], leaf, min_points=1)
                got = np.zeros(len(m["count"]), VOX); got["xyz"] = m["xyz"]; got["count"] = m["count"]
                assert got.tobytes() == merged.tobytes(), "the host merge against the model"
                (k2, n2, h2), x = check_index(env, c, [got], [None], leaf, ("closed loop index", leaf, b), capacity=len(got))
                blk = Blocks(env, 3, 2048, 2048)
                pts, seg, kls = blk.run(c, 3, x.desc, ALL, "global", (1, 0))
                assert seg[b, ABSENT, 1] == 0 and seg[b, SPARSE, 1] == 0, ("the device: points of the frame miss the map made of them", leaf, b, seg[b].tolist())
                assert seg[b, PRESENT, 1] == int((cls == PRESENT).sum()) > 0 and kls[b, : o["n"]].tobytes() == cls.tobytes()
                blk.free(); x.free()


# ------------------------------------------------------------------------------------------------------------------ 11: the chain on the device
def chain_on_device(env, oracle):
    """a sequence voxel export indexed with its count taken from &d_header->n_stored, then a fused step, then the judge — no synchronisation in between. The result
    equals the synchronised route (the export read back, indexed again with the count known, the same step judged again) and the model"""
    import scene_grid_seq_cases as SGQ
    F, stride, leaf = 3, 4096, 0.3
    clouds, ego_v, yaw = SGQ.drive(env)
    walls = scene(0, 1)[48:]   # (unowned points in every frame of the drive and in the live frames: judged by cell)
    clouds = [np.concatenate([q, walls]) for q in clouds]
    cap = F * stride
    with SV.context(env, F, 0.27, 64, stride, 256) as c:
        host = np.zeros((F, stride, 4), np.float32)
        for k, x_ in enumerate(clouds[:F]):
            host[k, : len(x_)] = x_
        ptr, keep = env.upload(host)
        exp = SV.Blocks(env, cap)
        x = Index(env, cap)
        blk = Blocks(env, 2, stride, stride)
        c.sequence_products_dev(ptr, stride * 4, [len(q) for q in clouds[:F]], [SGQ.SQ.stamp(k) for k in range(F)], list(ego_v[:F]), list(yaw[:F]), 0, 0, 0, scene=True)
        c.export_sequence_scene_voxels_dev(F, leaf, exp.a_vox, cap, exp.a_hdr, 0, classes=SV.ALL)
        c.index_voxel_maps_dev([(exp.a_vox, exp.a_hdr + 20, cap)], leaf, x.desc)   # (n_stored of the export's header, read on the device)
        live = [clouds[F], clouds[F + 1]]
        h2 = np.zeros((2, stride, 4), np.float32)
        for b, q in enumerate(live):
            h2[b, : len(q)] = q
        p2, keep2 = env.upload(h2)
        c.frames_dev(p2, stride * 4, [len(q) for q in live], run_tracker=True, timestamps=[SGQ.SQ.stamp(F)] * 2, ego_v=[float(ego_v[F])] * 2, ego_yaw=[float(yaw[F])] * 2)
        c.export_map_points_dev(2, x.desc, blk.a_pts, blk.ps, blk.a_seg, blk.a_cls, blk.cs, min_count=1, reach=1)
        c.synchronize()
        chain = [a.tobytes() for a in blk.raw()]
        keys, cnt, hdr = x.read()
        v, h, t = exp.read()
        nv = int(h[5])
        assert nv > 0 and hdr[0] == nv
        # the synchronised route: the export's voxels as a host-known map
        vox = np.ascontiguousarray(v[:nv]).view(VOX).reshape(-1)
        mk, mc, mh = index_model([vox], [None], leaf, 1, cap)
        assert hdr.tobytes() == mh.tobytes() and keys[: len(mk)].tobytes() == mk.tobytes() and cnt[: len(mk)].tobytes() == mc.tobytes()
        x2 = Index(env, cap)
        x2.run(c, [(exp.a_vox, 0, nv)], leaf)
        blk2 = Blocks(env, 2, stride, stride)
        blk2.run(c, 2, x2.desc, ALL, "global", (1, 1))
        assert [a.tobytes() for a in blk2.raw()] == chain, "the chain on the device against the synchronised route"
        obs, cls = judge_and_check(env, c, 2, x, (mk, mc, len(mk)), leaf, ((1, 1), (2, 0)), "the chain against the model")
        assert int((cls[0][0] == PRESENT).sum()) + int((cls[0][1] == PRESENT).sum()) > 0, "no point of the live frames meets the drive's map"
        for q in (exp, x, x2, blk, blk2):
            q.free()


def play_against_map(env, oracle):
    """sequence.play_against_map: a drive played frame by frame on one slot against an index -> per-frame class counts, equal to the model's of a context that
    plays the same frames"""
    import importlib
    leaf, frames_n = 0.25, 3
    clouds = [scene(f) for f in range(frames_n)]
    want = []
    with env.context(0, max_points=2048, max_batch=1, max_tracks_total=64) as c:
        c.set_track_links(True)
        obs = []
        for f in range(frames_n):
            keep = AC.launch(env, c, [clouds[f]], 2048, f)
            obs.append(observe(c, 0))
        x, mi = make_index(env, c, [(i, 2 + k % 3) for k, i in enumerate(frame_cells(obs[:1], leaf))], leaf, "helper index")
        for o in obs:
            cls = classify(o, cell_set(*mi), leaf, 3, 1)
            want.append([int((cls == k).sum()) for k in range(5)])
    seq_mod = importlib.import_module(env.mot.__name__ + ".sequence")
    with env.context(0, max_points=2048, max_batch=1, max_tracks_total=64) as c:
        c.set_track_links(True)
        got = seq_mod.play_against_map(c, [(q, 1.0, 0.0) for q in clouds], x.desc, min_count=3, reach=1, dt_us=1e5, t0=2.0e8, upload=env.upload)
    assert got.tolist() == want and sum(w[PRESENT] for w in want) > 0 and sum(w[ABSENT] for w in want) > 0, (got.tolist(), want)
    x.free()


# ------------------------------------------------------------------------------------------------------------------ 12: the judge's refusals
def raw_export(c, E, blk, x, batch=2, params=(1, 0), mask=ALL, frame=0, points="a", pstride=None, segments="a", classes="a", cstride=None, index=True, desc=None):
    P = E.MotMapJudgeParams(*params) if params is not None else None
    ptr = lambda v, a: None if v is None else (a if v == "a" else v)
    D = desc if desc is not None else x.desc
    return c.lib.mot_export_map_points_dev(c._h, batch, C.byref(D) if index else None, C.byref(P) if P is not None else None, mask, frame, C.c_void_p(ptr(points, blk.a_pts)),
                                           C.c_long(blk.ps if pstride is None else pstride), C.c_void_p(ptr(segments, blk.a_seg)), C.c_void_p(ptr(classes, blk.a_cls)),
                                           C.c_long(blk.cs if cstride is None else cstride))


def contract(env, oracle):
    """every refusal with sentinel blocks unchanged; the states that answer MOT_E_STATE (links off, no fused step, a stage-wise call, a tracker step from outside,
    sequence slots) — the scene grid is never needed; MOT_E_CAPACITY of the getter with the counts delivered; a smaller batch"""
    E = env.mot
    leaf = 0.25
    clouds = [[scene(f, 20), scene(f + 5, 12)] for f in range(6)]
    with env.context(0, max_points=4096, max_batch=2, max_tracks_total=64) as c:
        blk = Blocks(env, 2, 4096, 4096)
        sentinel = blk.raw()
        x, mi = make_index(env, c, [((k, 3, -2), 4) for k in range(40)], leaf, "contract index")
        def untouched(what, before=None):
            c.synchronize()
            assert all((a == b).all() for a, b in zip(blk.raw(), before or sentinel)), (what, "a refused call wrote into the caller's blocks")
        export = lambda batch=2: c.export_map_points_dev(batch, x.desc, blk.a_pts, blk.ps, blk.a_seg, blk.a_cls, blk.cs)
        getter = lambda b=0: c.get_map_points(b, x.desc)
        def state_error(what, batch=2, slot=0):
            before = blk.raw()
            assert SJ.code_of(env, lambda: export(batch)) == E.MOT_E_STATE and SJ.code_of(env, lambda: getter(slot)) == E.MOT_E_STATE, what
            untouched(what, before)
        state_error("links off")
        c.set_track_links(True)
        state_error("no fused step since the links were turned on")
        keep = AC.launch(env, c, clouds[0], 4096, 0)
        keep = AC.launch(env, c, clouds[1], 4096, 1)
        D = lambda **kw: E.MotVoxelIndex(**{**dict(keys=x.a_keys, counts=x.a_cnt, header=x.a_hdr, capacity=x.cap, leaf_x=leaf, leaf_y=leaf, leaf_z=leaf, reserved=0), **kw})
        nan = float("nan")
        for what, kw in (("null index", dict(index=False)), ("null params", dict(params=None)), ("null segments", dict(segments=None)), ("leaf NaN", dict(desc=D(leaf_y=nan))),
                         ("leaf inf", dict(desc=D(leaf_x=float("inf")))), ("leaf 0 (a descriptor the index call never filled)", dict(desc=D(leaf_x=0.0, leaf_y=0.0, leaf_z=0.0))),
                         ("leaf below 1e-2", dict(desc=D(leaf_z=0.009))), ("leaf above 1e3", dict(desc=D(leaf_x=1000.5))), ("min_count 0", dict(params=(0, 0))),
                         ("negative min_count", dict(params=(-1, 0))), ("reach 2", dict(params=(1, 2))), ("reach -1", dict(params=(1, -1))), ("mask bit 5", dict(mask=32)),
                         ("negative mask", dict(mask=-1)), ("frame 2", dict(frame=2)), ("frame -1", dict(frame=-1)), ("batch 0", dict(batch=0)), ("batch 3", dict(batch=3)),
                         ("negative point stride", dict(pstride=-1)), ("negative class stride", dict(cstride=-1)), ("null points with a stride", dict(points=None, mask=0)),
                         ("null points with a mask", dict(points=None, pstride=0)), ("points off 4 bytes", dict(points=blk.a_pts + 2)), ("segments off 4 bytes", dict(segments=blk.a_seg + 2)),
                         ("keys off 8 bytes", dict(desc=D(keys=x.a_keys + 4))), ("counts off 4 bytes", dict(desc=D(counts=x.a_cnt + 2))), ("header off 4 bytes", dict(desc=D(header=x.a_hdr + 2))),
                         ("null header", dict(desc=D(header=None))), ("negative index capacity", dict(desc=D(capacity=-1))), ("index capacity 2^31", dict(desc=D(capacity=2 ** 31))),
                         ("null keys with a capacity", dict(desc=D(keys=None))), ("null counts with a capacity", dict(desc=D(counts=None))),
                         ("the records are the keys", dict(points=x.a_keys)), ("the records end inside the counts", dict(points=x.a_cnt - 16 * 2 * 4096 + 16)),
                         ("the segments are the header", dict(segments=x.a_hdr)), ("the class bytes inside the keys", dict(classes=x.a_keys + 9)),
                         ("the class bytes cover the header", dict(classes=x.a_hdr - 2 * 4096 + 1))):
            assert raw_export(c, E, blk, x, **kw) == E.MOT_E_ARG, what
            untouched(what)
        n, ne = C.c_int(-7), C.c_int(-7); seg = np.full(10, -7, np.int32); P = E.MotMapJudgeParams(1, 0)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        raw_get = lambda slot=0, P=P, mask=ALL, frame=0, pts=None, pcap=0, n=n, seg=seg, cls=None, ccap=0, ne=ne, desc=x.desc: c.lib.mot_get_map_points(
            c._h, slot, C.byref(desc) if desc is not None else None, C.byref(P) if P is not None else None, mask, frame, vp(pts) if pts is not None else None, pcap,
            C.byref(n) if n is not None else None, vp(seg) if seg is not None else None, vp(cls) if cls is not None else None, ccap, C.byref(ne) if ne is not None else None)
        for what, kw in (("slot 2", dict(slot=2)), ("slot -1", dict(slot=-1)), ("null index", dict(desc=None)), ("null params", dict(P=None)), ("mask", dict(mask=32)), ("frame", dict(frame=2)),
                         ("null n_points", dict(n=None)), ("null segments", dict(seg=None)), ("null n_elevated", dict(ne=None)), ("negative capacity", dict(pcap=-1)),
                         ("negative class capacity", dict(ccap=-1)), ("reach 2", dict(P=E.MotMapJudgeParams(1, 2))), ("a bad leaf", dict(desc=D(leaf_x=0.0)))):
            assert raw_get(**kw) == E.MOT_E_ARG, what
        assert n.value == -7 and ne.value == -7 and (seg == -7).all()
        # the limits themselves are served
        served = Blocks(env, 2, 4096, 4096)
        assert raw_export(c, E, served, x, params=(2 ** 31 - 1, 1)) == 0 and raw_export(c, E, served, x, desc=D(leaf_x=1e-2, leaf_y=1e3)) == 0
        assert raw_export(c, E, served, x, desc=D(keys=None, counts=None, capacity=0)) == 0, "an index of capacity 0 needs no blocks"
        c.synchronize()
        obs = [observe(c, b) for b in range(2)]
        cells = frame_cells(obs, leaf)
        x.free()
        x, mi = make_index(env, c, [(i, 4) for i in cells[::2]], leaf, "contract index of the frame")
        cls = [classify(o, cell_set(*mi), leaf, 1, 0) for o in obs]
        # MOT_E_CAPACITY of the getter: the counts and the table are delivered, the buffers stay as they were
        want_seg, rec = SJ.records(obs[0], cls[0], ALL, "global")
        total = obs[0]["n"]
        assert total > 1 and int((cls[0] == PRESENT).sum()) > 0 and int((cls[0] == ABSENT).sum()) > 0
        pts = np.full((total + 1) * 4, -7, np.int32); kb = np.full(total + 1, SJ.CLS_SENT, np.uint8)
        for pcap, ccap in ((total - 1, total), (total, total - 1)):
            seg[:] = -7
            assert raw_get(pts=pts, pcap=pcap, cls=kb, ccap=ccap, desc=x.desc) == E.MOT_E_CAPACITY
            assert (n.value, ne.value) == (total, total) and seg.tobytes() == want_seg.tobytes() and (pts == -7).all() and (kb == SJ.CLS_SENT).all()
        assert raw_get(pts=pts, pcap=total, cls=kb, ccap=total, desc=x.desc) == 0 and pts[: total * 4].tobytes() == rec.tobytes() and (pts[total * 4:] == -7).all()
        assert kb[:total].tobytes() == cls[0].tobytes() and kb[total] == SJ.CLS_SENT
        assert raw_get(mask=1 << PRESENT, desc=x.desc) == 0 and n.value == int((cls[0] == PRESENT).sum()) and ne.value == total, "null buffers: the counts alone"
        # a batch smaller than max_batch leaves the other slot's blocks alone
        blk1 = Blocks(env, 2, 4096, 4096)
        out = blk1.run(c, 1, x.desc, ALL, "global")
        SJ.check_slot(blk1, out, 0, obs[0], cls[0], ALL, "global", "batch 1 of 2")
        assert (out[0][1] == -7).all() and (out[1][1] == -7).all() and (out[2][1] == SJ.CLS_SENT).all()
        # a stage-wise call takes slot 0; a tracker step fed from outside takes slot 1's links
        keep = AC.launch(env, c, clouds[2], 4096, 2)
        elev = c.get_ground(0, n_hint=len(clouds[2][0]))["elevated"]
        c.cluster(elev)
        state_error("a stage-wise call took slot 0")
        getter(1)
        keep = AC.launch(env, c, clouds[3], 4096, 3)
        export()
        c.ego_update(3.0e8, 0.0, 0.0, 1); c.track_step(LC.lattice(3), 3.0e8, slot=1)
        state_error("a tracker step fed from outside", slot=1)
        export(1); getter(0)
        # a reset leaves the slot without a step; the next fused call serves again (no grid: nothing else to restart)
        keep = AC.launch(env, c, clouds[4], 4096, 4)
        export(); getter(1)
        c.set_track_links(False)
        state_error("links off again")
        x.free()
    # sequence slots
    with env.context(0, max_points=4096, max_batch=2, max_tracks_total=64) as c:
        c.set_track_links(True)
        host = np.zeros((2, 4096, 4), np.float32)
        for f in range(2):
            host[f, : len(clouds[f][0])] = clouds[f][0]
        ptr, keep = env.upload(host)
        c.sequence_dev(ptr, 4096 * 4, [len(clouds[f][0]) for f in range(2)], [2.0e8, 2.001e8], [1.0] * 2, [0.0] * 2)
        x, mi = make_index(env, c, [((k, 3, -2), 4) for k in range(4)], leaf, "contract index, sequence slots")
        blk = Blocks(env, 2, 4096, 4096); sentinel = blk.raw()
        for fn in (lambda: c.export_map_points_dev(2, x.desc, blk.a_pts, blk.ps, blk.a_seg, blk.a_cls, blk.cs), lambda: c.export_map_points_dev(1, x.desc, blk.a_pts, blk.ps, blk.a_seg, blk.a_cls, blk.cs),
                   lambda: c.get_map_points(0, x.desc), lambda: c.get_map_points(1, x.desc)):
            assert SJ.code_of(env, fn) == E.MOT_E_STATE, "sequence slots"
        c.synchronize()
        assert all((a == b).all() for a, b in zip(blk.raw(), sentinel))
        x.free()


# ------------------------------------------------------------------------------------------------------------------ 13: determinism, non-interference
def determinism(env, oracle):
    """two calls on one state give identical bytes; the same steps in two contexts give identical bytes; a run with index and judge calls interleaved leaves boxes,
    tracks, point tracks and track points byte-identical to a run without"""
    leaf = 0.25
    res = {}
    for tag in ("never", "judged", "judged again"):
        out, judged = [], []
        with env.context(0, max_points=4096, max_batch=2, max_tracks_total=64) as c:
            c.set_track_links(True)
            for f in range(3):
                clouds = [scene(f, 20), scene(f + 5, 12)]
                keep = PC.launch(env, c, clouds, 4096, f, yaw=0.02 * f)
                n_points = [len(q) for q in clouds]
                before = PC.readout(c, 2, n_points)
                if tag != "never":
                    obs = [observe(c, b) for b in range(2)]
                    x, mi = make_index(env, c, [(i, 2 + k % 3) for k, i in enumerate(frame_cells(obs, leaf)[::2])], leaf, ("determinism index", f))
                    blk = Blocks(env, 2, 4096, 4096)
                    blk.run(c, 2, x.desc, ALL, "global", (3, 1)); first = [a.tobytes() for a in blk.raw()]
                    blk.run(c, 2, x.desc, ALL, "global", (3, 1))
                    assert [a.tobytes() for a in blk.raw()] == first, (f, "two calls on one state differ")
                    c.get_map_points(1, x.desc, reach=1)
                    judged.append(first)
                    blk.free(); x.free()
                    PC.equal_readouts(PC.readout(c, 2, n_points), before, (f, "after the judge calls"))
                out.append(AC.defined_items(before))
        res[tag] = (out, judged)
    assert res["judged"][1] == res["judged again"][1], "the same steps in two contexts differ"
    for f in range(3):
        PC.equal_readouts(res["judged"][0][f], res["never"][0][f], (f, "against a context that never judged"))


# ------------------------------------------------------------------------------------------------------------------ 14: emulator only
def launches_only_in_the_new_calls(env, oracle):
    """emulator: the launch counters of the new kernels move in the new calls and nowhere else, by a constant whatever the data (the scatter only with a mask and
    room for records; the index's write launch only with a capacity); a refused call launches and allocates nothing; the judge's scratch — class bytes, rows,
    arguments and the page-locked ring — is taken at the first call, the getter's staging block at its first call, none of it goes with the grid, all of it with
    mot_destroy; the index call shares the merge's ONE block"""
    lib = env.mot.load_library(env.lib_path)
    lib.hipemu_live_allocs.restype = C.c_long
    count = lambda names=KERNELS: [lib.hipemu_launch_count(k) for k in names]
    E = env.mot
    leaf = 0.25
    rng = np.random.default_rng(139)
    base = lib.hipemu_live_allocs()
    with env.context(0, max_points=4096, max_batch=2, max_tracks_total=64) as c:
        before, ibefore, mbefore, sbefore = count(), count((INDEX_KERNEL,)), count(VM.KERNELS), count(VM.SORT_KERNELS)
        c.set_track_links(True); c.set_scene_grid(1.0, 64)
        blk = Blocks(env, 2, 4096, 4096)
        for f in range(3):
            keep = PC.launch(env, c, [scene(f, 20), scene(f + 5, 12)], 4096, f)
            c.accumulate_scene(2)
            for b in (0, 1):
                c.get_point_tracks(b); c.get_tracks(b); c.get_track_points(b, frame="global"); c.get_scene_grid(b); c.get_scene_points(b)
        SJ.Blocks(env, 2, 4096, 4096).run(c, 2, SJ.ALL, "global")
        blocks, counts = VM.split(rng, 700, 2)
        VM.check(env, c, blocks, counts, 0.5, "a merge before the index calls")
        assert count() == before and count((INDEX_KERNEL,)) == ibefore, "a kernel of the feature ran outside the new calls"
        allocs = lib.hipemu_live_allocs()
        mbefore, sbefore = count(VM.KERNELS), count(VM.SORT_KERNELS)
        # the index call: the merge's block, its count launches, one write launch
        for k, (total, n_maps) in enumerate(((1, 1), (300, 2), (2 * T + 9, 16))):
            blocks, counts = VM.split(rng, total, n_maps)
            d = VM.Dev(env, blocks, counts, 0)
            x = Index(env, total + 1)
            bad = E.MotVoxelIndex(x.a_keys + 4, x.a_cnt, x.a_hdr, x.cap, 0, 0, 0, 0)
            arr = (E.MotVoxelMapSrc * 1)(E.MotVoxelMapSrc(d.maps[0][0] or None, None, d.maps[0][2]))
            V = E.voxel_params(0.5, 1)
            assert c.lib.mot_index_voxel_maps_dev(c._h, arr, 1, C.byref(V), C.byref(bad)) == E.MOT_E_ARG
            assert count(VM.KERNELS) == mbefore and count((INDEX_KERNEL,)) == [ibefore[0] + k] and lib.hipemu_live_allocs() == allocs, "a refused index call allocated or launched"
            x.run(c, d.maps, 0.5)
            per = [n - (name == b"voxel_merge_reduce_kernel") for n, name in zip(VM.PER_CALL, VM.KERNELS)]   # (the count launches: M5 once)
            assert count(VM.KERNELS) == [a + b for a, b in zip(mbefore, per)] and count(VM.SORT_KERNELS) == [a + 7 for a in sbefore] and count((INDEX_KERNEL,)) == [ibefore[0] + k + 1], (total, n_maps)
            mbefore, sbefore = count(VM.KERNELS), count(VM.SORT_KERNELS)
            allocs = lib.hipemu_live_allocs()   # (the merge's one block may have grown in place)
            d.free(); x.free()
        x0 = Index(env, 0)
        d = VM.Dev(env, blocks, counts, 0)
        x0.run(c, d.maps, 0.5)
        assert count((INDEX_KERNEL,)) == [ibefore[0] + 3], "capacity 0: the write launch is left out"
        d.free(); x0.free()
        allocs = lib.hipemu_live_allocs()
        # the judge
        obs = [observe(c, b) for b in range(2)]
        x, mi = make_index(env, c, [(i, 4) for i in frame_cells(obs, leaf)[::2]], leaf, "launches index")
        allocs = lib.hipemu_live_allocs()
        assert count() == before
        assert raw_export(c, E, blk, x, mask=32) == E.MOT_E_ARG
        assert lib.hipemu_live_allocs() == allocs and count() == before, "a refused call allocated or launched"
        blk.run(c, 2, x.desc, ALL, "global")
        assert count() == [before[0] + 1, before[1] + 1, before[2] + 1] and lib.hipemu_live_allocs() == allocs + 4   # class bytes, rows, arguments, the ring
        blk.run(c, 2, x.desc, 0, "global")
        assert count() == [before[0] + 2, before[1] + 2, before[2] + 1], "mask 0: the scatter is not launched"
        blk.run(c, 2, x.desc, 0, "global", points=False)
        assert count() == [before[0] + 3, before[1] + 3, before[2] + 1] and lib.hipemu_live_allocs() == allocs + 4
        c.get_map_points(1, x.desc, reach=1)
        assert count() == [before[0] + 4, before[1] + 4, before[2] + 2] and lib.hipemu_live_allocs() == allocs + 5   # (the getter's staging block)
        sj = [lib.hipemu_launch_count(k) for k in SJ.KERNELS]
        for f in range(3, 20):   # more calls than the ring has blocks
            keep = PC.launch(env, c, [scene(f, 20), scene(f + 5, 12)], 4096, f)
            blk.run(c, 2, x.desc, ALL, "sensor", (1, 1))
        assert [lib.hipemu_launch_count(k) for k in SJ.KERNELS] == sj, "a kernel of the scene judge ran in the map judge"
        live = lib.hipemu_live_allocs()
        c.set_scene_grid(None)
        gone = live - lib.hipemu_live_allocs()
        obs = [observe(c, b) for b in range(2)]
        judge_and_check(env, c, 2, x, mi, leaf, ((4, 0), (4, 1)), "with the grid off", obs=obs)
        assert lib.hipemu_live_allocs() == live - gone, "the judge's scratch went with the grid, or was taken again"
        x.free()
    assert lib.hipemu_live_allocs() == base, "mot_destroy left allocations of the feature behind"


def scratch_under_allocation_failure(env, oracle):
    """emulator: each of the judge's allocations failing in turn at the first call (class bytes, rows, arguments, the ring's block, the ring's first event) ->
    MOT_E_HIP, no block kept, the caller's blocks untouched; the next call resumes and gives the bytes of the model. The index call's scratch failing -> MOT_E_HIP,
    nothing kept, the descriptor and the blocks untouched"""
    lib = env.mot.load_library(env.lib_path)
    lib.hipemu_live_allocs.restype = C.c_long
    lib.hipemu_fail_alloc_at.argtypes = [C.c_long]; lib.hipemu_fail_alloc_at.restype = None
    E = env.mot
    leaf = 0.25
    rng = np.random.default_rng(149)
    try:
        with env.context(0, max_points=4096, max_batch=2, max_tracks_total=64) as c:
            c.set_track_links(True)
            keep = AC.launch(env, c, [scene(0, 20), scene(5, 12)], 4096, 0)
            obs = [observe(c, b) for b in range(2)]   # (the getters' own staging blocks exist from here on)
            # the index call first: its scratch is the merge's one block
            blocks, counts = VM.split(rng, 900, 2)
            d = VM.Dev(env, blocks, counts, 0)
            x = Index(env, 900)
            sentinel = x.raw()
            allocs = lib.hipemu_live_allocs()
            lib.hipemu_fail_alloc_at(1)
            rc = SJ.code_of(env, lambda: c.index_voxel_maps_dev(d.maps, 0.5, x.desc))
            lib.hipemu_fail_alloc_at(0)
            assert rc == E.MOT_E_HIP and lib.hipemu_live_allocs() == allocs and x.desc.leaf_x == 0.0, "the index call's scratch"
            c.synchronize()
            assert all((a == b).all() for a, b in zip(x.raw(), sentinel))
            d.free(); x.free()
            (k0, n0, h0), x = check_index(env, c, blocks, counts, 0.5, "after the failed attempt")
            x.free()
            x, mi = make_index(env, c, [(i, 4) for i in frame_cells(obs, leaf)[::2]], leaf, "failure index")
            blk = Blocks(env, 2, 4096, 4096); sentinel = blk.raw()
            allocs = lib.hipemu_live_allocs()
            for k in (1, 2, 3, 4, 5):
                lib.hipemu_fail_alloc_at(k)
                rc = SJ.code_of(env, lambda: c.export_map_points_dev(2, x.desc, blk.a_pts, blk.ps, blk.a_seg, blk.a_cls, blk.cs))
                lib.hipemu_fail_alloc_at(0)
                assert rc == E.MOT_E_HIP and lib.hipemu_live_allocs() == allocs, k
                assert all((a == b).all() for a, b in zip(blk.raw(), sentinel)), k
            judge_and_check(env, c, 2, x, mi, leaf, ((4, 0),), "after the failed attempts", obs=obs)
            assert lib.hipemu_live_allocs() == allocs + 5   # (the scratch, the ring and the getter's staging block)
            x.free()
    finally:
        lib.hipemu_fail_alloc_at(0)
