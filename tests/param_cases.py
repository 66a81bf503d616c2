"""Parity AWAY from the two presets, inside the declared parameter domain (include/mot.h, "parameter domain"): shared by
tests/test_emu_params.py (emulator) and tests/test_params_gpu.py (MI355X); tests/test_math_exact.py sweeps the guarded fast cells over the
same settings. The oracle is the C restatement with the same constants (oracle.params(preset, **overrides): the reference build has its
constants compiled in). Every input is generated here from a fixed seed, and every case asserts with numpy and the oracle, BEFORE it calls the
library, that the input exercises what the case names.

Every case goes through both routes, everything bit-exact (mask, ground and elevated clouds, label grid, per-point labels, cluster count,
boxes and their order, cube markers, side products):
  stage-wise   mot_ground_remove -> mot_cluster -> mot_box_fit_resident
  fused        a three-slot mot_frames_dev batch with the case in the MIDDLE slot and ragged neighbours, mot_set_fused_outputs 0 and everything
"""
import ctypes as C

import numpy as np

import patterns
from capacity_cases import Env, same_boxes, same_clusters, same_markers   # noqa: F401  (Env: re-exported for the callers)

# ---- the settings (also swept by tests/test_math_exact.py and, on the device, tests/test_api_v2_gpu.py)
POLAR_RANGES = ((2.0, 80.0), (0.5, 200.0), (20.0, 60.0), (45.0, 60.0))   # the last one sits ON the domain's edge: r_max / (r_max - r_min) = 4
POLAR_OUTSIDE = (58.0, 65.0)                                              # refused by mot_create; the sweeps' negative control
GRID_SIZES = (8, 31, 32, 33, 64, 97, 224, 255, 256)
GRID_SETTINGS = tuple((g, roi) for g in GRID_SIZES for roi in (30.0, 50.0)) + ((97, 37.5),)
MAX_POINTS = 24576
NUM_CHANNEL, NUM_BIN = 80, 120   # MOT_NUM_CHANNEL, MOT_NUM_BIN of include/mot.h
OUT_LABELS = 4
OUT_ALL = 7   # MOT_OUT_GROUND | MOT_OUT_MASK | MOT_OUT_LABELS
f32 = np.float32


def ident(over):
    return ",".join("%s=%g" % kv for kv in sorted(over.items()))


# ------------------------------------------------------------------------------------------------------------------ numpy models
def cart_cells(pts, G, roi):
    """mapCartesianGrid's cell of every point in fp32 as the reference evaluates it (component_clustering.cpp:42-48); -1 outside the ROI"""
    roi = f32(roi); half = roi / f32(2)
    xc, yc = pts[:, 0].astype(f32) + half, pts[:, 1].astype(f32) + half
    inside = (xc >= 0) & (xc < roi) & (yc >= 0) & (yc < roi)
    fx, fy = np.floor(f32(G) * xc / roi), np.floor(f32(G) * yc / roi)
    inside &= (fx >= 0) & (fx < G) & (fy >= 0) & (fy < G)
    return np.where(inside, fx, -1).astype(np.int64), np.where(inside, fy, -1).astype(np.int64)


def cell_counts(pts, G, roi):
    x, y = cart_cells(pts, G, roi)
    cnt = np.zeros((G, G), np.int64)
    np.add.at(cnt, (x[x >= 0], y[x >= 0]), 1)
    return cnt


def distance32(pts):
    """sqrtf(x * x + y * y) in fp32, products rounded one by one (ground_removal.cpp:52)"""
    x, y = pts[:, 0].astype(f32), pts[:, 1].astype(f32)
    return np.sqrt(x * x + y * y, dtype=f32)


def ulps(v, k):
    v = f32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, f32(np.inf) if k > 0 else f32(-np.inf), dtype=f32)
    return v


def points_in_cells(cells, reps, G, roi, rng, z=(0.0, 1.0)):
    """reps[i] points inside cell i (within 0.3 of a cell of its centre), heights above every ground threshold: the ground stage keeps them all"""
    cells = np.asarray(cells, np.int64).reshape(-1, 2)
    idx = np.repeat(np.arange(len(cells)), reps)
    xy = (cells[idx] + 0.5 + rng.uniform(-0.3, 0.3, (len(idx), 2))) * (roi / G) - roi / 2
    out = np.zeros((len(idx), 4), f32)
    out[:, :2] = xy; out[:, 2] = rng.uniform(z[0], z[1], len(idx)); out[:, 3] = rng.uniform(0, 1, len(idx))
    cx, cy = cart_cells(out, G, roi)
    assert np.array_equal(cx, cells[idx, 0]) and np.array_equal(cy, cells[idx, 1]), "a point left its cell"
    return out


# ------------------------------------------------------------------------------------------------------------------ the two routes
def oracle_all(oracle, p, cloud):
    import oracle_lib as O
    g = oracle.ground_remove(p, cloud, want_dump=True)
    cl = oracle.cluster(p, g["elevated"])
    bx = oracle.box_fit(p, g["elevated"], cl["grid"], cl["num_cluster"], debug=True)
    return dict(g=g, cl=cl, bx=bx, markers=O.box_markers_numpy(g["elevated"], cl["point_label"], bx["box_cluster"]),
                side=oracle.cluster_products(p, g["elevated"], cl["grid"]))


def same_ground(got, g, what):
    for k in ("elevated", "ground"):
        assert got[k].shape == g[k].shape and np.array_equal(got[k].view(np.uint32), g[k].view(np.uint32)), (what, k)
    assert np.array_equal(got["mask"], g["mask"]), (what, "mask")


def same_side(got, want, what):
    for k in ("clustered", "obstacles", "cost_map"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)


def hground(ctx, slot=0):
    """the per-cell ground thresholds the filter kernel left (mot_debug_copy, which = 10): hGround on ground cells, -inf elsewhere"""
    hg = np.zeros(NUM_CHANNEL * NUM_BIN, f32)
    assert ctx.lib.mot_debug_copy(ctx._h, 10, slot, hg.ctypes.data_as(C.c_void_p), C.c_size_t(hg.nbytes)) == 0
    return hg


def same_polar_grid(ctx, g, what, slot=0):
    hg = hground(ctx, slot)
    isg = g["is_ground"].reshape(-1).astype(bool)
    assert np.array_equal(np.isfinite(hg), isg), what
    assert np.array_equal(hg[isg].view(np.uint32), g["hground"].astype(f32).reshape(-1)[isg].view(np.uint32)), what


def check_stagewise(ctx, o, cloud, what, polar=False):
    g = ctx.ground_remove(cloud); same_ground(g, o["g"], (what, "stage-wise"))
    if polar:
        same_polar_grid(ctx, o["g"], (what, "stage-wise hGround"))
    same_clusters(ctx.cluster(g["elevated"]), o["cl"], (what, "stage-wise"))
    same_boxes(ctx.box_fit_resident(), o["bx"], (what, "stage-wise"))
    same_markers(ctx.box_markers(0), o["markers"], (what, "stage-wise"))
    same_side(ctx.cluster_products(0), o["side"], (what, "stage-wise"))


def check_slot(ctx, b, o, n, what, polar=False):
    same_ground(ctx.get_ground(b, n_hint=n), o["g"], what)
    if polar:
        same_polar_grid(ctx, o["g"], (what, "hGround"), b)
    same_clusters(ctx.get_clusters(b, n_elevated=len(o["g"]["elevated"])), o["cl"], what)
    same_boxes(ctx.get_boxes(b), o["bx"], what)
    same_markers(ctx.box_markers(b), o["markers"], what)
    same_side(ctx.cluster_products(b), o["side"], what)


def neighbours(synth, seed):
    """two ordinary frames of different sizes for slots 0 and 2"""
    return synth.make_cloud(9000, 3 + seed % 5, seed)[: 8801 - 97 * (seed % 7)], synth.make_cloud(3000, 11 + seed % 3, seed + 1)[: 2500 + 13 * (seed % 11)]


def run_case(env, oracle, synth, preset, over, cloud, what, edge=None, polar=False, flags=(0, OUT_ALL), seed=0, want=None):
    """`cloud` under oracle.params(preset, **over): the edge assertion on the oracle's products, then both routes. Returns the oracle's products."""
    p = oracle.params(preset, **over)
    o = want or oracle_all(oracle, p, cloud)
    if edge is not None:
        edge(p, o)
    assert len(cloud) <= 24000
    left, right = neighbours(synth, seed)
    ol, orr = oracle_all(oracle, p, left), oracle_all(oracle, p, right)
    host = np.zeros((3, MAX_POINTS, 4), f32)
    n = [len(left), len(cloud), len(right)]
    for b, x in enumerate((left, cloud, right)):
        host[b, : len(x)] = x
    with env.context(preset, pkw=over, max_points=MAX_POINTS, max_batch=3, max_tracks_total=16) as c:
        check_stagewise(c, o, cloud, what, polar)
        ptr, keep = env.upload(host)
        for fl in flags:
            c.set_fused_outputs(fl)
            c.frames_dev(ptr, MAX_POINTS * 4, n)
            for b, ob in ((1, o), (0, ol), (2, orr)):
                check_slot(c, b, ob, n[b], (what, "fused, outputs %d" % fl, "slot %d" % b), polar)
        del keep
    return o


# ------------------------------------------------------------------------------------------------------------------ 1 grid sizes
def grid_cells(G, which, rng):
    """cell patterns scaled to G. "frame": the border (row 0 full, row G-1 / column 0 / column G-1 in part, so that a bit that leaks past
    column G-1 or row G-1 lands on a FREE cell), the four corners, columns 31/32 and 223/224 (a run across a word boundary of the 256-bit
    row) and a sparse checkerboard inside; "shapes": spiral, comb and diagonals of tests/patterns.py"""
    shapes = dict((name, cells) for name, cells in patterns.occupancy_cases(G, rng, dense=True))
    if which == "frame":
        cells = [(0, y) for y in range(G)] + [(G - 1, y) for y in range(0, G, 7)] + [(x, 0) for x in range(0, G, 9)] + [(x, G - 1) for x in range(2, G, 5)]
        cells += shapes["corners"]
        for ca in (31, 223):
            if G > ca + 1:
                cells += [(x, y) for x in range(3, G - 1, 4) for y in (ca, ca + 1)]
        cells += [(x, y) for x, y in shapes["checker5"] if 2 <= x < G - 2 and 2 <= y < G - 2 and (x + y) % 3 == 0]
    else:
        cells = shapes["spiral"] + shapes["comb"] + shapes["diag"]
    return sorted(set((int(x), int(y)) for x, y in cells))


def grid_case(env, oracle, synth, G, roi, dilate, which, flags=(0, OUT_ALL)):
    seed = G * 1000 + int(roi * 2) * 4 + dilate * 2 + (which == "frame")
    rng = np.random.default_rng(seed)
    occ = 1 + (G + dilate) % 2                               # both occupancy rules over the lattice
    over = dict(num_grid=G, roi_m=roi, dilate=dilate, occ_min_count=occ, pic_scale=900.0 / roi, min_points=1)
    cells = grid_cells(G, which, rng)
    if len(cells) > 4500:   # at most ~12 000 points: in random order nearly every point is a (tile, cluster) group of its own, and a frame takes max_points / 2 of them
        border = [c for c in cells if min(c) == 0 or max(c) == G - 1]
        inner = [c for c in cells if not (min(c) == 0 or max(c) == G - 1)]
        cells = sorted(border + [inner[i] for i in rng.permutation(len(inner))[: 4500 - len(border)]])
    # the patterns' cells hold occ .. 3 points (so that they count whatever the rule); beside them, cells with fewer points than the rule asks for
    reps = rng.integers(occ, 3 if len(cells) > 3000 else 4, len(cells))
    taken = set(cells)
    lone = [c for c in ((int(a), int(b)) for a, b in rng.integers(1, G - 1, (min(60, G * G // 16), 2))) if c not in taken]   # (interior cells: the border stays as designed)
    cloud = np.concatenate([points_in_cells(cells, reps, G, roi, rng), points_in_cells(lone, 1, G, roi, rng)]) if lone else points_in_cells(cells, reps, G, roi, rng)
    cloud = cloud[rng.permutation(len(cloud))]
    assert len(cloud) <= MAX_POINTS // 2

    def edge(p, o):
        cnt = cell_counts(o["g"]["elevated"], G, roi)
        occd = cnt >= occ
        assert occd[0, :].any() and occd[G - 1, :].any() and occd[:, 0].any() and occd[:, G - 1].any(), "border rows / columns"
        if which == "frame":
            assert occd[0, 0] and occd[0, G - 1] and occd[G - 1, 0] and occd[G - 1, G - 1], "corners"
            for ca in (31, 223):
                if G > ca + 1:
                    assert (occd[:, ca] & occd[:, ca + 1]).any(), "a run across columns %d/%d" % (ca, ca + 1)
            # a cell at column G-1 whose successor in memory, (x + 1, 0), and the one after it stay free even after the dilation: where a label written
            # past column G-1 would land (the dilation's column mask alone cannot be seen this way: csrc/cluster.hip says why)
            free = ~(occd | np.roll(occd, 1, 0) | np.roll(occd, -1, 0))[:, 0]
            assert any(occd[x, G - 1] and free[x + 1] for x in range(G - 2)), "nothing would show a bit leaking past column G-1"
            assert (cnt == 1).any() and (cnt >= 2).any()
        else:
            assert o["cl"]["num_cluster"] >= 1 and (o["cl"]["grid"] > 0).sum() > G
        assert (o["cl"]["grid"][0, :] > 0).any() and (o["cl"]["grid"][G - 1, :] > 0).any()
        assert len(o["bx"]["debug"]) >= 1   # (the box stage sees every cluster; few are box-shaped: min_points = 1 lets the rule filter decide on shape alone)
    run_case(env, oracle, synth, 0 if roi == 50.0 else 1, over, cloud, ("grid", G, roi, dilate, which), edge, flags=flags, seed=seed)


# ------------------------------------------------------------------------------------------------------------------ 2 occupancy rule
def occupancy_cloud(seed=5):
    """preset 0's grid (250 cells of 0.2 m). Isolated cells on a pitch-3 lattice, three 4096-point chunks of the compaction kernel:
    A one point;  B two points next to each other in ONE chunk;  C two points in DIFFERENT chunks (0 and 2): the fused fold's "promoted by
    whichever entry arrives second";  D three points, one per chunk;  E two in chunk 1 and one in chunk 2. Returns cloud and the cell lists."""
    rng = np.random.default_rng(seed)
    G, roi = 250, 50.0
    lat = [(x, y) for x in range(1, G - 1, 3) for y in range(1, G - 1, 3) if (x - 125) ** 2 + (y - 125) ** 2 > 30 ** 2]   # clear of r_min
    lat = [lat[i] for i in rng.permutation(len(lat))]
    A, B, Cc, D, E = (lat[a:b] for a, b in ((0, 1800), (1800, 2500), (2500, 3000), (3000, 3120), (3120, 3240)))
    pt = lambda cells: points_in_cells(cells, 1, G, roi, rng)
    pairs = lambda cells: points_in_cells(cells, 2, G, roi, rng)          # the two points of a cell are consecutive
    chunk0 = [pt(Cc), pt(D), pairs(B[:350])]
    chunk1 = [pt(D), pairs(E), pairs(B[350:])]
    chunk2 = [pt(Cc), pt(D), pt(E)]
    a = [0, 600, 1200, 1800]
    parts = []
    for k, ch in enumerate((chunk0, chunk1, chunk2)):
        body = np.concatenate(ch)
        fill = pt(A[a[k]: a[k + 1]])
        body = np.concatenate([body, fill])
        assert len(body) <= 4096
        if k < 2:   # fill the chunk up to exactly 4096 points with points outside the ROI (inside the polar range: elevated like all the others)
            pad = np.zeros((4096 - len(body), 4), f32); pad[:, 0] = 60.0 + rng.uniform(0, 5, len(pad)); pad[:, 1] = rng.uniform(-5, 5, len(pad)); pad[:, 2] = 0.5
            body = np.concatenate([body, pad])
        parts.append(body)
    return np.concatenate(parts), dict(A=A, B=B, C=Cc, D=D, E=E)


def occupancy_case(env, oracle, synth, occ, dilate):
    G, roi = 250, 50.0
    cloud, cells = occupancy_cloud()
    other = oracle.cluster(oracle.params(0, occ_min_count=3 - occ, dilate=dilate), oracle.ground_remove(oracle.params(0), cloud)["elevated"])

    def edge(p, o):
        assert (o["g"]["mask"] == 2).all(), "every point elevated: a point's index in the frame is its index in the elevated cloud"
        cx, cy = cart_cells(cloud, G, roi)
        key = cx * G + cy
        chunk = np.arange(len(cloud)) // 4096
        cnt = cell_counts(cloud, G, roi)
        chunks_of = lambda c: sorted(chunk[key == c[0] * G + c[1]].tolist())
        assert all(cnt[c] == 1 for c in cells["A"]) and all(cnt[c] == 2 for c in cells["B"] + cells["C"]) and all(cnt[c] == 3 for c in cells["D"] + cells["E"])
        assert all(chunks_of(c) in ([0, 0], [1, 1]) for c in cells["B"]), "two points in one chunk"
        assert all(chunks_of(c) == [0, 2] for c in cells["C"]), "two points in different chunks"
        assert all(chunks_of(c) == [0, 1, 2] for c in cells["D"]) and all(chunks_of(c) == [1, 1, 2] for c in cells["E"])
        assert set(np.unique(cnt)) == {0, 1, 2, 3}
        # the rule matters on this cloud
        assert o["cl"]["num_cluster"] != other["num_cluster"] and not np.array_equal(o["cl"]["grid"] > 0, other["grid"] > 0)
        occupied = (o["cl"]["grid"] > 0)
        assert all(occupied[c] == (occ == 1) for c in cells["A"]) if not dilate else True
        assert all(occupied[c] for c in cells["B"] + cells["C"] + cells["D"] + cells["E"])
    run_case(env, oracle, synth, 0, dict(occ_min_count=occ, dilate=dilate), cloud, ("occupancy", occ, dilate), edge, seed=occ * 2 + dilate)


# ------------------------------------------------------------------------------------------------------------------ 3 polar range
def ring_points(d_target, count, rng, z):
    """points whose fp32 distance sqrtf(x*x + y*y) is EXACTLY d_target, at random angles"""
    out = []
    for _ in range(400 * count):
        a = rng.uniform(-np.pi, np.pi)
        q = np.array([[f32(np.cos(a) * float(d_target)), f32(np.sin(a) * float(d_target)), f32(z()), 0]], f32)
        if distance32(q)[0] == d_target:
            out.append(q[0])
            if len(out) == count:
                break
    assert len(out) == count, "no point at distance %r" % d_target
    return np.array(out, f32)


def polar_cloud(synth, r_min, r_max, seed):
    rng = np.random.default_rng(seed)
    base = synth.make_cloud(16000, 4, seed)
    base[:, :2] *= f32(r_max / 100.0)                       # the scene fills the range: returns on both sides of either limit
    z = lambda: rng.choice([-1.95, -1.7, -1.2, -0.3, 0.6]) + rng.uniform(-0.05, 0.05)
    span = f32(r_max) - f32(r_min)
    extra = []
    for lim in (f32(r_min), f32(r_max)):
        for k in range(-3, 4):
            extra.append(ring_points(ulps(lim, k), 6, rng, z))
    for k in rng.choice(np.arange(1, 120), 40, replace=False):   # bin rings, as the reference's expression places them, +-2 ulp
        ring = f32(r_min) + f32(k) * (span / f32(120))
        for s in (-2, -1, 0, 1, 2):
            extra.append(ring_points(ulps(ring, s), 2, rng, z))
    spokes = []
    for k in range(81):   # channel spokes at random radii inside the range
        a = -np.pi + k * (2 * np.pi / 80)
        r = rng.uniform(r_min * 1.01 + 0.01, r_max * 0.99, 12)
        q = np.zeros((12, 4), f32); q[:, 0] = np.cos(a) * r; q[:, 1] = np.sin(a) * r; q[:, 2] = [z() for _ in range(12)]
        for s in (-1, 0, 1):
            t = q.copy(); t[:, 1] = [ulps(v, s) for v in t[:, 1]]; spokes.append(t)
    cloud = np.concatenate([base] + extra + spokes)
    return cloud[rng.permutation(len(cloud))]


def polar_case(env, oracle, synth, r_min, r_max):
    seed = int(r_min * 10 + r_max)
    cloud = polar_cloud(synth, r_min, r_max, seed)

    def edge(p, o):
        assert f32(r_max) <= f32(4) * (f32(r_max) - f32(r_min)), "inside the declared domain"
        d = distance32(cloud)
        for lim in (f32(r_min), f32(r_max)):
            for k in range(-3, 4):
                assert (d == ulps(lim, k)).sum() >= 6, (lim, k)
        # the range filter cuts exactly at the limits: a point AT a limit is dropped, its neighbour inside is kept
        m = o["g"]["mask"]
        assert (m[d == f32(r_min)] == 0).all() and (m[d == f32(r_max)] == 0).all()
        assert (m[d == ulps(r_min, 1)] != 0).all() and (m[d == ulps(r_max, -1)] != 0).all()
        assert min((m == k).sum() for k in (0, 1, 2)) > 100, ("dropped, ground and elevated points", [(m == k).sum() for k in (0, 1, 2)])
        assert o["g"]["is_ground"].sum() > 200
    run_case(env, oracle, synth, 0, dict(r_min=r_min, r_max=r_max), cloud, ("polar", r_min, r_max), edge, polar=True, seed=seed)


# ------------------------------------------------------------------------------------------------------------------ 4 ground thresholds
# (setting, the setting it must ALSO differ from — None: the preset alone). 0.1 is no fp32 / fp64 number: the margin is compared in double (ground_removal.cpp:239)
GROUND_SETTINGS = (dict(t_hmin=-1.7), dict(t_hmax=-1.2), dict(t_hdiff=0.1), dict(t_hmin=-2.4, t_hmax=-0.1), dict(h_sensor=-0.35), dict(h_sensor=2.3, t_hdiff=0.8),
                   dict(ground_margin=0.0), dict(ground_margin=0.1), dict(ground_margin=0.6, t_hdiff=0.2), dict(gauss_sigma=0.5, h_sensor=-0.35),
                   dict(gauss_sigma=2.0, t_hdiff=5.0))
GROUND_ALSO = {"gauss_sigma=0.5,h_sensor=-0.35": dict(h_sensor=-0.35), "gauss_sigma=2,t_hdiff=5": dict(t_hdiff=5.0)}


def polar_cells64(pts, r_min=3.4, r_max=120.0):
    """(channel, bin) of every point, in double: good enough to CLEAR cells and to place points at cell centres"""
    d = np.hypot(pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64))
    ch = np.floor((np.arctan2(pts[:, 1].astype(np.float64), pts[:, 0].astype(np.float64)) + np.pi) / (2 * np.pi) * 80).astype(int)
    return ch, np.floor((d - r_min) / (r_max - r_min) * 120).astype(int)


def ground_cloud(base):
    """a synthetic scan plus three kinds of five-cell structures along a channel, where the Gaussian smoothing decides (an empty or obstacle-only
    cell takes the height h_sensor; it is ground iff its SMOOTHED height is below t_hmax = -0.4 and its step to the neighbours below t_hdiff = 0.4):
      platform  min z -0.55 | -0.55 | obstacle only | -0.55 | -0.55    h_sensor = -0.35: step 0.20; smoothed -0.459 (sigma 1: ground) / -0.392 (sigma 0.5: not)
      terrace   min z -0.74 | -0.74 | obstacle only | -0.74 | -0.74    h_sensor = -0.35: step 0.39; smoothed -0.432 at sigma 0.5: ground (preset: h_sensor 2, not ground)
      valley    min z -1.95 | -1.95 | obstacle only | -1.95 | -1.95    h_sensor = 2: smoothed -0.17 (sigma 1: not ground) / -0.52 (sigma 2: ground, once t_hdiff admits the step)
    The obstacle-only cell holds points at z = -0.25, 0.2 and 1.0 (-0.25 < h_sensor + ground_margin: ground when the cell is)."""
    rng = np.random.default_rng(12)
    ch, bn = polar_cells64(base)
    sites = [(c, b, kind) for kind, cs in (("platform", (5, 25, 45)), ("terrace", (10, 30, 50)), ("valley", (15, 35, 65))) for c in cs for b in (12, 40, 80)]
    clear = np.zeros(len(base), bool)
    extra = []
    for c, b, kind in sites:
        clear |= (ch == c) & (bn >= b - 2) & (bn <= b + 2)
        for k in range(-2, 3):
            a = -np.pi + (c + 0.5 + rng.uniform(-0.2, 0.2, 6)) * (2 * np.pi / 80)
            r = 3.4 + (b + k + 0.5 + rng.uniform(-0.2, 0.2, 6)) * (116.6 / 120)
            q = np.zeros((6, 4), f32); q[:, 0] = r * np.cos(a); q[:, 1] = r * np.sin(a)
            q[:, 2] = [-0.25, -0.25, 0.2, 0.2, 1.0, 1.0] if k == 0 else dict(platform=-0.55, terrace=-0.74, valley=-1.95)[kind] + np.array([0, 0.3, 0.6, 0.02, 0.9, 0.05])
            extra.append(q)
    cloud = np.concatenate([base[~clear]] + extra)
    return cloud[rng.permutation(len(cloud))]


def ground_case(env, oracle, synth, over):
    cloud = ground_cloud(synth.make_cloud(20000, 6, 2))
    base = oracle.ground_remove(oracle.params(0), cloud)["mask"]
    also = GROUND_ALSO.get(ident(over))

    def edge(p, o):
        assert int((o["g"]["mask"] != base).sum()) > 0, "the setting changes nothing on this cloud"
        if also is not None:   # ... and the Gaussian's part in it is real
            assert int((o["g"]["mask"] != oracle.ground_remove(oracle.params(0, **also), cloud)["mask"]).sum()) > 0, "the sigma changes nothing on this cloud"
        assert min((o["g"]["mask"] == k).sum() for k in (1, 2)) > 500
    run_case(env, oracle, synth, 0, over, cloud, ("ground", sorted(over.items())), edge, polar=True, seed=len(str(over)))


# ------------------------------------------------------------------------------------------------------------------ 5 box stage
BOX_SETTINGS = (dict(pic_scale=6.0), dict(pic_scale=18.0, rng_mapping=0), dict(pic_scale=20.0), dict(l_slope_dist=0), dict(l_slope_dist=3, lshape_side_cond=0),
                dict(l_num_points=1), dict(l_num_points=300, lshape_side_cond=0), dict(lshape_side_cond=0), dict(min_points=1), dict(min_points=100),
                dict(ram_points=1), dict(ram_points=128, rng_mapping=0), dict(ram_points=80, rng_mapping=0), dict(min_points=30, l_num_points=1, lshape_side_cond=0, pic_scale=20.0))


def box_cloud(seed=7):
    """car-, pole- and wall-sized blobs of 20 .. 420 points in random order, on both sides of the sensor's lane (the L-shape side condition
    looks at y > 8 m / y < -5 m), heights that pass and heights that fail ruleBasedFilter"""
    rng = np.random.default_rng(seed)
    ctr = np.array([(-21 + 6.0 * (k % 8), -21 + 6.0 * (k // 8)) for k in range(64)])
    parts = []
    for k, c in enumerate(ctr):
        n = int(rng.choice([20, 60, 150, 320, 420]))
        half = [(0.9, 0.5), (0.3, 0.3), (2.2, 0.25), (1.6, 1.2)][k % 4]
        q = np.zeros((n, 4), f32)
        q[:, :2] = c + rng.uniform(-1, 1, (n, 2)) * half
        q[:, 2] = rng.uniform(-1.2, [0.3, 1.4, -0.6][k % 3], n)
        parts.append(q)
    cloud = np.concatenate(parts)
    return cloud[rng.permutation(len(cloud))]


def box_case(env, oracle, synth, over):
    cloud = box_cloud()

    def edge(p, o):
        dbg = o["bx"]["debug"]
        lshape = [d for d in dbg if d["branch"] == 0]; rect = [d for d in dbg if d["branch"] == 1]
        assert len(lshape) >= 3 and len(rect) >= 3, "both the L-shape and the rectangle branch"
        assert any(d["accepted"] for d in dbg) and any(not d["accepted"] for d in dbg), "the rule filter keeps some boxes and drops some"
        assert f32(p.pic_scale) * f32(p.roi_m) in (f32(300), f32(900), f32(1000))
    run_case(env, oracle, synth, 0, over, cloud, ("box", sorted(over.items())), edge, seed=len(str(over)))


def box_wide_case(env, oracle, synth, along_y, pic_scale=20.0):
    """ONE cluster across the whole picture at pic_scale * roi_m = 1000: two rails 46.6 m apart and three cross ties, 926 pixel columns with two
    extreme pixels each (the rails along x, or along y: whichever axis the picture's columns follow) — more candidate hull points than a 901-column picture can have (box.hip: kMaxHullIn); l_num_points = 100000 sends it to the minimum-area rectangle"""
    rng = np.random.default_rng(21)
    G, roi = 250, 50.0
    cols = np.arange(40, 966)                                       # 926 pixel columns of 0.05 m: one point per column in each of two rails
    x = -roi / 2 + (cols + 0.5) / pic_scale
    rails = [np.stack([x, np.full(len(x), y) + rng.uniform(-0.05, 0.05, len(x))], 1) for y in (-23.3, 23.3)]
    ties = [(gx, gy) for gx in (10, 125, 240) for gy in range(8, G - 8)]   # three cross ties make the two rails ONE component
    q = np.zeros((2 * len(x), 4), f32); q[:, :2] = np.concatenate(rails); q[:, 2] = rng.uniform(-0.3, 0.4, len(q))
    cloud = np.concatenate([q, points_in_cells(ties, 2, G, roi, rng, z=(-0.3, 0.4))])
    cloud = cloud[rng.permutation(len(cloud))]
    if along_y:
        cloud[:, [0, 1]] = cloud[:, [1, 0]]

    def edge(p, o):
        lab = o["cl"]["point_label"]; big = np.bincount(lab).argmax()
        assert big > 0 and o["bx"]["debug"][big - 1]["branch"] == 1, "the rectangle branch"
        e = o["g"]["elevated"][lab == big]
        px = np.floor(e[:, int(along_y)] * f32(pic_scale) + f32(roi * pic_scale / 2)).astype(int)
        cols = np.unique(px)
        both = sum(1 for c in cols[:: 7] if np.ptp(e[px == c, 1 - int(along_y)]) * pic_scale > 2)
        assert len(cols) > 901 and both > 0.9 * len(cols[:: 7]), (len(cols), both)
    run_case(env, oracle, synth, 0, dict(pic_scale=pic_scale, l_num_points=100000), cloud, ("one cluster over the whole picture", pic_scale, along_y), edge, seed=3)


# ------------------------------------------------------------------------------------------------------------------ 6 tracker thresholds
# (preset, overrides): 0.25 is preset 1's own distance_thres and 99 preset 0's, so each is set on the OTHER preset
TRACK_SETTINGS = ((0, dict(life_time_thres=1)), (0, dict(life_time_thres=8)), (0, dict(seed_box_index=0)), (0, dict(seed_box_index=3)), (0, dict(distance_thres=0.25)),
                  (1, dict(distance_thres=99.0)), (1, dict(distance_thres=99.0, life_time_thres=1)), (0, dict(bb_yaw_change_thres=0.02)), (0, dict(bb_yaw_change_thres=1.5)),
                  (0, dict(gamma_g=2.0)), (0, dict(gamma_g=30.0)), (0, dict(p_d=0.5)), (0, dict(p_g=0.7)), (1, dict(p_d=0.99, p_g=0.9)), (1, dict(gamma_g=2.0, seed_box_index=3)))
# tracker_cases generators: gates to themselves / shared gates / objects that vanish and come back under a moving ego pose / objects that move more than
# a metre a frame with partial views (where distance_thres and a large bb_yaw_change_thres decide)
TRACK_KINDS = ("lattice9", "lattice2", "blinking", "fast")
TRACK_PAIRS = 36   # pairs with a seed in tests/golden/param_seeds.json: pinned, so that a re-run chooser cannot shrink the lattice unnoticed
TRACK_FRAMES = 20
TRACK_SEEDS = "param_seeds.json"                      # tests/golden/, written by tests/golden/make_param_seeds.py
PERTURB_TOL = 1e-6


def track_ident(preset, over):
    return "preset%d:%s" % (preset, ident(over))


def track_sequence(kind, seed, over, frames=TRACK_FRAMES):
    """[(boxes, timestamp, ego speed, ego yaw)] of at most 25 frames from the generators of tests/tracker_cases.py. seed_box_index decides on the
    FIRST frame only (a track is seeded iff the frame has more boxes than the index): those settings get lattices of as many boxes as the index
    (0 -> 1 box: seeded where the preset's index 1 is not; 3 -> 3 boxes: not seeded where the preset is)"""
    import tracker_cases as TC
    if kind == "blinking":
        return [(b, ts, v, yaw) for b, ts, v, yaw in TC.blinking_world(seed, 7, frames)]
    if kind == "fast":   # 12 frames: the lanes stay within 8 m of the origin (tracker_cases.fast_lanes says why)
        return list(TC.fast_lanes(seed, min(frames, 12)))
    nbox = max(over["seed_box_index"], 1) if "seed_box_index" in over else 12
    pl = TC.StreamPlan(kind, nbox, 9.0 if kind == "lattice9" else 2.0, seed)
    return [(b, ts, 0.0, 0.0) for b, ts in zip(pl.boxes(frames), pl.timestamps(frames))]


def one_ulp_off(seq):
    """the same boxes with ONE coordinate per frame moved by one fp32 ulp (x of corner f % 4 of box f % m, top and bottom face alike)"""
    out = []
    for f, (b, ts, v, yaw) in enumerate(seq):
        b = b.copy()
        if len(b):
            k, c = f % len(b), f % 4
            b[k, c, 0] = np.nextafter(b[k, c, 0], f32(np.inf), dtype=f32); b[k, c + 4, 0] = b[k, c, 0]
        out.append((b, ts, v, yaw))
    return out


def oracle_track_run(oracle, p, seq):
    """the restatement stepped on a sequence: per frame the records and the states of the live tracks"""
    T = oracle.Tracker(p)
    out = []
    try:
        for b, ts, v, yaw in seq:
            T.ego_update(ts, v, yaw)
            o = T.step(b, ts, max_tracks=1024)
            out.append((o, {int(i): T.state(int(i)) for i in np.nonzero(o["track_manage"] > 0)[0]}))
    finally:
        T.close()
    return out


def runs_differ(ra, rb, tol):
    """None when two oracle runs agree in every discrete output and to `tol` relative in every state of every live track-frame, else where they part"""
    import seq_parity as SP
    for f, ((a, sa), (b, sb)) in enumerate(zip(ra, rb)):
        if a["n"] != b["n"] or any(not np.array_equal(a[k], b[k]) for k in ("track_manage", "is_static", "is_vis", "lifetime")):
            return (f, "discrete")
        for i in sa:
            e, same = SP.state_rel_err(sb[i], sa[i])
            if not same or not e <= tol:
                return (f, i, e)
            for k in ("p", "v_yaw", "vis_box"):   # the records: the visible box is where box association (distance_thres, bb_yaw_change_thres) shows
                x, y = np.asarray(a[k][i], np.float64), np.asarray(b[k][i], np.float64)
                if not np.array_equal(np.isnan(x), np.isnan(y)) or not np.all(np.nan_to_num(np.abs(x - y)) <= tol * max(float(np.nanmax(np.abs(x), initial=0.0)), 1e-6) + tol * 1e-3):
                    return (f, i, k)
    return None


def track_seed_qualifies(oracle, preset, over, kind, seed):
    """the chooser's rule, from the restatement alone: (1) the run on the boxes and the run on the boxes one ulp off agree in every discrete
    output and to 1e-6 relative in every state on every live track-frame — a sequence on which a last-bit difference decides nothing;
    (2) each field of the setting, put back to the preset's value alone, changes what the tracker answers on these boxes; (3) tracks are alive most of the time"""
    seq = track_sequence(kind, seed, over)
    p = oracle.params(preset, **over)
    run = oracle_track_run(oracle, p, seq)
    if runs_differ(run, oracle_track_run(oracle, p, one_ulp_off(seq)), PERTURB_TOL) is not None:
        return False
    for k in over:   # every field the setting names matters here: put back to the preset's value alone, it changes the answer
        if runs_differ(run, oracle_track_run(oracle, oracle.params(preset, **{q: v for q, v in over.items() if q != k}), seq), 1e-9) is None:
            return False
    return sum(len(s) for _, s in run) >= len(seq) // 2


def track_seeds():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", TRACK_SEEDS)) as fh:
        return json.load(fh)


def tracker_case(env, oracle, preset, over, kind):
    """mot_track_step against oracle.Tracker(p) on the chosen sequence: track set, track_manage, lifetime and flags exact, every state of EVERY live
    track-frame within 1e-4 relative (seq_parity.compare_tracks with nothing set aside)"""
    import seq_parity as SP
    seed = track_seeds()[track_ident(preset, over)][kind]
    base = getattr(oracle, "_b", oracle)              # the chooser's rule is about the restatement
    assert track_seed_qualifies(base, preset, over, kind, seed), "tests/golden/param_seeds.json no longer fits the generators: run tests/golden/make_param_seeds.py"
    seq = track_sequence(kind, seed, over)
    assert len(seq) <= 25
    p = oracle.params(preset, **over)
    stats = {}
    T = oracle.Tracker(p)
    try:
        with env.context(preset, pkw=over, max_points=1024, max_batch=1, max_tracks_total=256) as c:
            for f, (b, ts, v, yaw) in enumerate(seq):
                assert np.allclose(c.ego_update(ts, v, yaw), T.ego_update(ts, v, yaw), rtol=1e-12, atol=1e-12)
                a = c.track_step(b, ts); o = T.step(b, ts, max_tracks=1024)
                assert not a["capacity_exceeded"]
                SP.compare_tracks(a, o, c.track_state, T.state, (track_ident(preset, over), kind, f), rtol=SP.RTOL, stats=stats)
    finally:
        T.close()
    return stats


def track_pairs():
    """(preset, overrides, generator) of every pair the chooser found a seed for. Not every generator can show every setting (a lattice of slow
    boxes never puts a box a metre from its track); check_track_pairs holds the list to what the issue names."""
    seeds = track_seeds()
    return [(preset, over, kind) for preset, over in TRACK_SETTINGS for kind in TRACK_KINDS if kind in seeds.get(track_ident(preset, over), {})]


def check_track_pairs():
    """every setting of TRACK_SETTINGS runs on at least one generator, every value the lattice is about is among them, and the count is the pinned one"""
    pairs = track_pairs()
    for preset, over in TRACK_SETTINGS:
        assert any(p == preset and o == over for p, o, _ in pairs), ("no sequence for", track_ident(preset, over))
    run = [tuple(sorted(o.items())) for _, o, _ in pairs]
    for field, values in (("life_time_thres", (1, 8)), ("seed_box_index", (0, 3)), ("distance_thres", (0.25, 99.0)), ("bb_yaw_change_thres", (0.02, 1.5)),
                          ("gamma_g", (2.0, 30.0)), ("p_d", (0.5, 0.99)), ("p_g", (0.7, 0.9))):
        for v in values:
            assert any((field, v) in r for r in run), (field, v)
    assert len(pairs) == TRACK_PAIRS, len(pairs)
