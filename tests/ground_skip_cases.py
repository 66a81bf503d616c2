"""The compaction kernel's group skip (csrc/ground.hip: the min-z kernel hands one conservative max z per aligned group of 8 input points, the elevated-only
compaction does not load a group none of whose lanes can be elevated), shared by tests/test_emu_ground_skip.py (emulator) and tests/test_ground_skip_gpu.py
(MI355X). Every cloud is built here in numpy — a flat ground under a 16-beam scanner plus a few boxes, beam-major — and every result is compared bit for bit
with the C restatement (oracle_lib.ground_remove): the elevated cloud, the mask and the three counts.

What the elevated-only instantiation ITSELF wrote is read without a re-run through mot_debug_copy (14: the elevated cloud as it lies, 12-byte points; 15: the
mask bytes; 16: the group max z); mot_get_ground re-runs the instantiation that loads every point, and set_fused_outputs(7) runs that one in the fused call: all
three must agree with the oracle, hence with each other."""
import ctypes as C

import numpy as np

DROPPED, GROUND, ELEVATED = 0, 1, 2
OUT_GROUND, OUT_MASK, OUT_LABELS = 1, 2, 4
LENGTHS = (0, 1, 7, 8, 9, 2047, 2049, 4095, 4096, 4097, 4104, 9001)   # partial last groups, the 2048-point (min-z) and 4096-point (compaction) chunk edges
MAX_POINTS = 9216
BEAMS = 16


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ inputs
def base_cloud(n, seed=0):
    """n points, beam-major: beam k sweeps the azimuth once at the range where it meets the ground (z about -1.7); three boxes at 8 m replace the returns of
    the beams that pass over them (z in -1.2 .. 0.3: elevated, in contiguous runs)"""
    rng = np.random.default_rng(seed)
    per = max((n + BEAMS - 1) // BEAMS, 1)
    az = -np.pi + (np.arange(per) + 0.5) * (2 * np.pi / per)
    pts = np.zeros((BEAMS * per, 4), np.float32)
    for k in range(BEAMS):
        r = np.full(per, 5.0 + 2.3 * k); z = -1.7 + rng.uniform(-0.01, 0.01, per)
        if r[0] > 8.5:
            for a0, a1 in ((-2.6, -2.2), (0.3, 0.75), (1.9, 2.1)):
                hit = (az > a0) & (az < a1)
                r[hit] = 8.0 + rng.uniform(0.0, 0.3, hit.sum()); z[hit] = rng.uniform(-1.2, 0.3, hit.sum())
        s = slice(k * per, (k + 1) * per)
        pts[s, 0] = r * np.cos(az); pts[s, 1] = r * np.sin(az); pts[s, 2] = z; pts[s, 3] = rng.uniform(0.0, 1.0, per)
    return np.ascontiguousarray(pts[:n])


def cell_fractions(p, x, y):
    d = np.hypot(float(x), float(y))
    return (np.arctan2(float(y), float(x)) + np.pi) / (2 * np.pi) * 80, (d - p.r_min) / (p.r_max - p.r_min) * 120


def polar_cell(p, x, y):
    """ch * 120 + bin of a point well inside its cell (the callers place their points; fp64 here, the fractions are asserted to be far from a boundary)"""
    fc, fb = cell_fractions(p, x, y)
    assert 0.05 < fc % 1 < 0.95 and 0.05 < fb % 1 < 0.95 and 0 <= fc < 80 and 0 <= fb < 120, (fc, fb)
    return int(fc) * 120 + int(fb)


def crop_keep(p, a):
    """the node's pre-filter (mot_crop_keep): finite, z closed, x and y strict"""
    fin = np.isfinite(a[:, :3]).all(1)
    with np.errstate(invalid="ignore"):
        return fin & (a[:, 2] >= p.crop_z_min) & (a[:, 2] <= p.crop_z_max) & (a[:, 0] > p.crop_x_min) & (a[:, 0] < p.crop_x_max) & (a[:, 1] > p.crop_y_min) & (a[:, 1] < p.crop_y_max)


def reference(O, p, cloud):
    """oracle_lib.ground_remove with the mask over the INPUT points (the pre-filter's drops included)"""
    if not p.crop_enable:
        return O.ground_remove(p, cloud)
    keep = crop_keep(p, cloud)
    assert np.array_equal(bits(cloud[keep]), bits(O.crop(p, cloud)))
    g = O.ground_remove(p, np.ascontiguousarray(cloud[keep]))
    mask = np.zeros(len(cloud), np.uint8); mask[keep] = g["mask"]
    return dict(elevated=g["elevated"], ground=g["ground"], mask=mask)


def special_cloud(O, p0):
    """one frame with every special group of the issue, each in a 64-point tile of its own that the oracle classifies all GROUND before the change. Returns the
    cloud and {name: point indices}; the properties each case is there for are asserted on the oracle's answer for the FINAL cloud (expectations())."""
    cloud = base_cloud(9001, seed=3)
    m = O.ground_remove(p0, cloud)["mask"]
    tiles = [t for t in range(len(cloud) // 64) if (m[t * 64:(t + 1) * 64] == GROUND).all()][1::2]   # every second one: no two changes in neighbouring tiles
    assert len(tiles) >= 24, len(tiles)
    it = iter(tiles)
    idx = {}
    for j in range(8):   # an elevated point at each position of an otherwise all-ground group (the group in the middle of its tile)
        i = next(it) * 64 + 24 + j; cloud[i, 2] = 1.0; idx["elevated_at_%d" % j] = [i]
    i = next(it) * 64; cloud[i, 2] = 1.0; idx["elevated_first_lane"] = [i]
    i = next(it) * 64 + 63; cloud[i, 2] = 1.0; idx["elevated_last_lane"] = [i]
    g = next(it) * 64 + 16; cloud[g:g + 8, :3] = (1.0, 0.5, -1.7); idx["dropped_group_inside_rmin"] = list(range(g, g + 8))
    g = next(it) * 64 + 16; cloud[g:g + 8, :3] = (130.0, 5.0, -1.7); idx["dropped_group_beyond_rmax"] = list(range(g, g + 8))
    g = next(it) * 64 + 16; idx["group_cropped"] = list(range(g, g + 8))   # x = 10 m is outside crop_x_max = 5 m: dropped with crop_enable, a ground group without
    cloud[g:g + 8, 0] = 10.0 + 0.01 * np.arange(8); cloud[g:g + 8, 1] = 0.3; cloud[g:g + 8, 2] = -1.7
    i = next(it) * 64 + 27; cloud[i, :3] = (1.0, 0.0, 50.0); idx["dropped_high_z_inside_rmin"] = [i]
    i = next(it) * 64 + 28; cloud[i, :3] = (125.0, 0.0, 1.0e6); idx["dropped_high_z_beyond_rmax"] = [i]
    for name, z in (("nan", np.nan), ("plus_inf", np.inf), ("minus_inf", -np.inf), ("minus_zero", -0.0)):
        i = next(it) * 64 + 29; cloud[i, 2] = z; idx["z_" + name] = [i]
    # a point alone in a cell between two beams, too high to be a ground height: its cell is not ground (hg = -inf); z is BELOW nothing else in the group
    i = next(it) * 64 + 30; a = np.arctan2(cloud[i, 1], cloud[i, 0]); cloud[i, :3] = (29.15 * np.cos(a), 29.15 * np.sin(a), -0.3); idx["non_ground_cell"] = [i]
    # z exactly at h + margin and one float below it: h is the cell's threshold on the final cloud (raising a point never lowers its cell's minimum)
    where = {}
    for name in ("z_at_threshold", "z_below_threshold"):
        t0 = next(it) * 64
        i = next(k for k in range(t0 + 24, t0 + 40) if 0.1 < cell_fractions(p0, cloud[k, 0], cloud[k, 1])[0] % 1 < 0.9)   # well inside its channel
        where[name] = i; cloud[i, 2] = -1.0   # not its cell's minimum from here on
    h = O.ground_remove(p0, cloud, want_dump=True)
    for name, i in where.items():
        cell = polar_cell(p0, cloud[i, 0], cloud[i, 1])
        assert h["is_ground"].reshape(-1)[cell]
        t = np.float32(np.float64(h["hground"].reshape(-1)[cell]) + p0.ground_margin)
        if np.float64(t) < np.float64(h["hground"].reshape(-1)[cell]) + p0.ground_margin:   # h + margin is no float: the smallest float not below it
            t = np.nextafter(t, np.float32(np.inf))
        cloud[i, 2] = t if name == "z_at_threshold" else np.nextafter(t, np.float32(-np.inf))
        idx[name] = [i]
    return cloud, idx


def expectations(O, p, cloud, idx, ref):
    """what the special groups are there for, on the oracle's answer for this cloud"""
    m = ref["mask"]
    rest = lambda i: [k for k in range(i // 8 * 8, i // 8 * 8 + 8) if k != i]
    crop = bool(p.crop_enable)
    for name, ii in idx.items():
        i = ii[0]
        if crop:   # the pre-filter takes most of the cases' points away (x beyond 5 m, non-finite z): those are dropped; what the others become is the oracle's business
            gone = ~crop_keep(p, cloud[ii])
            assert (m[np.array(ii)[gone]] == DROPPED).all() and (name != "group_cropped" or gone.all()), name
            if not name.startswith("dropped_"):
                continue
        if name.startswith("elevated_") or name in ("z_nan", "z_plus_inf", "non_ground_cell", "z_at_threshold"):
            assert m[i] == ELEVATED, (name, m[i])
            if name.startswith("elevated_at") and not crop:
                assert (m[rest(i)] == GROUND).all(), name
        elif name.startswith("dropped_group"):
            assert (m[ii] == DROPPED).all(), name
        elif name == "group_cropped":
            assert (m[ii] == (DROPPED if crop else GROUND)).all(), (name, m[ii])
        elif name.startswith("dropped_high_z"):
            assert m[i] == DROPPED and (crop or (m[rest(i)] == GROUND).all()), name
        elif name in ("z_minus_zero",):
            assert m[i] == ELEVATED, name   # 0 m is far above the road
        elif name in ("z_minus_inf", "z_below_threshold"):
            assert m[i] == GROUND, (name, m[i])
    if not crop:
        h = O.ground_remove(p, cloud, want_dump=True)
        i = idx["non_ground_cell"][0]; cell = polar_cell(p, cloud[i, 0], cloud[i, 1])
        assert not h["is_ground"].reshape(-1)[cell]   # (the library's threshold of such a cell is -inf)
        for name in ("z_at_threshold", "z_below_threshold"):
            i = idx[name][0]; thr = np.float64(h["hground"].reshape(-1)[polar_cell(p, cloud[i, 0], cloud[i, 1])]) + p.ground_margin
            z, up = np.float64(cloud[i, 2]), np.float64(np.nextafter(cloud[i, 2], np.float32(np.inf)))
            assert (z >= thr > np.float64(np.nextafter(cloud[i, 2], np.float32(-np.inf)))) if name == "z_at_threshold" else (z < thr <= up), (name, z, thr)


def firing_order(cloud):
    return np.ascontiguousarray(cloud[np.argsort(np.arctan2(cloud[:, 1], cloud[:, 0]), kind="stable")])


def permuted(cloud, seed):
    return np.ascontiguousarray(cloud[np.random.default_rng(seed).permutation(len(cloud))])


def expected_group_max(cloud, mask):
    """the min-z kernel's word per aligned group of 8: max z over the points with a cell (mask != DROPPED), +-0 as +0, NaN if one of them is NaN, -inf if none"""
    n = len(cloud); ng = (n + 7) // 8
    z = np.full(ng * 8, -np.inf, np.float32)
    z[:n] = np.where(mask != DROPPED, cloud[:, 2] + np.float32(0.0), np.float32(-np.inf))
    z = z.reshape(ng, 8)
    with np.errstate(invalid="ignore"):
        out = np.where(np.isnan(z).any(1), np.float32(np.nan), np.nanmax(np.where(np.isnan(z), -np.inf, z), axis=1)).astype(np.float32)
    return out


def same_floats(a, b):
    """bit for bit, any NaN for a NaN"""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a[~na]), bits(b[~nb]))


def elevated_free_share(mask, width):
    m = len(mask) // width * width
    return float(1.0 - (mask[:m].reshape(-1, width) == ELEVATED).any(1).mean()) if m else 0.0


# ------------------------------------------------------------------------------------------------------------------ checks
def debug_copy(c, which, slot, dtype, count):
    out = np.zeros(max(count, 1), dtype)
    assert c.lib.mot_debug_copy(c._h, which, slot, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes)) == 0
    return out[:count]


def launch(env, c, clouds):
    host = np.zeros((len(clouds), MAX_POINTS, 4), np.float32)
    for b, x in enumerate(clouds):
        host[b, : len(x)] = x
    ptr, keep = env.upload(host)
    c.frames_dev(ptr, MAX_POINTS * 4, [len(x) for x in clouds])
    c.synchronize()
    return keep


def check_batch(env, c, clouds, refs, what):
    """the same batch three ways: default outputs (the skipping instantiation; its own cloud and counts, then mot_get_ground's re-run), the mask asked for (the skipping
    instantiation writes it), every output asked for (the instantiation that loads every point, in the fused call)"""
    for outputs in (0, OUT_MASK, OUT_GROUND | OUT_MASK | OUT_LABELS):
        c.set_fused_outputs(outputs)
        keep = launch(env, c, clouds)
        for b, (x, r) in enumerate(zip(clouds, refs)):
            tag = (what, outputs, b, len(x))
            ne, ng = len(r["elevated"]), len(r["ground"])
            cnt = c.get_ground(b, want_clouds=False)
            got = (cnt["n_elevated"], cnt["n_ground"], len(x) - cnt["n_elevated"] - cnt["n_ground"])
            print(tag, "counts (elevated, ground, dropped):", got, "oracle:", (ne, ng, int((r["mask"] == DROPPED).sum())))
            assert got == (ne, ng, int((r["mask"] == DROPPED).sum())), tag
            if not (outputs & OUT_GROUND):   # what the skipping instantiation left: 12-byte points
                raw = debug_copy(c, 14, b, np.uint32, 3 * ne).reshape(ne, 3)
                assert np.array_equal(raw, bits(r["elevated"][:, :3]).reshape(ne, 3)), tag
                gz = debug_copy(c, 16, b, np.float32, (len(x) + 7) // 8)
                assert same_floats(gz, expected_group_max(x, r["mask"])), tag
            if outputs == OUT_MASK:
                assert np.array_equal(debug_copy(c, 15, b, np.uint8, len(x)), r["mask"]), tag
        for b, (x, r) in enumerate(zip(clouds, refs)):   # (behind the raw reads: outputs 0 / mask only materialise on demand, by re-running the instantiation that loads every point)
            tag = (what, outputs, b, len(x), "get_ground")
            g = c.get_ground(b, n_hint=len(x))
            assert np.array_equal(g["mask"], r["mask"]), tag
            assert np.array_equal(bits(g["elevated"]), bits(r["elevated"])) and np.array_equal(bits(g["ground"]), bits(r["ground"])), tag
        del keep
    c.set_fused_outputs(0)


def frame_lengths(env, O):
    p = O.params(0)
    clouds = [base_cloud(n, seed=10 + k) for k, n in enumerate(LENGTHS)]
    refs = [reference(O, p, x) for x in clouds]
    assert sum(len(r["elevated"]) for r in refs) > 1000 and elevated_free_share(refs[-1]["mask"], 8) > 0.3   # both kinds of group occur
    with env.context(0, max_points=MAX_POINTS, max_batch=len(clouds)) as c:
        check_batch(env, c, clouds, refs, "lengths")


def special_groups(env, O, crop):
    p0, p = O.params(0), O.params(0, crop_enable=int(crop))
    cloud, idx = special_cloud(O, p0)
    clouds = [cloud, firing_order(cloud), permuted(cloud, 7)]
    refs = [reference(O, p, x) for x in clouds]
    expectations(O, p, cloud, idx, refs[0])
    print("elevated-free share of the special cloud: 8-groups %.2f, 64-tiles %.2f" % (elevated_free_share(refs[0]["mask"], 8), elevated_free_share(refs[0]["mask"], 64)))
    with env.context(0, pkw=dict(crop_enable=int(crop)), max_points=MAX_POINTS, max_batch=len(clouds)) as c:
        check_batch(env, c, clouds, refs, "special, crop %d" % crop)


def golden_frame(env, O, golden_dir):
    """one fused frame (tracker off) on the recorded 9k frame: the stage behind the compaction sees an unchanged cloud"""
    import os
    d = np.load(os.path.join(golden_dir, "frame_ot_9k.npz"))
    cloud = np.ascontiguousarray(d["cloud"], np.float32)
    p = O.params(0)
    r = O.ground_remove(p, cloud)
    cl = O.cluster(p, r["elevated"])
    bx = O.box_fit(p, r["elevated"], cl["grid"], cl["num_cluster"])
    assert len(r["elevated"]) == int(d["n_elevated"]) and np.array_equal(bits(bx["boxes"]), bits(d["boxes"]))   # (the recorded frame's own figures)
    with env.context(0, max_points=MAX_POINTS, max_batch=1) as c:
        keep = launch(env, c, [cloud])
        got = c.get_boxes(0)
        assert np.array_equal(bits(got["boxes"]), bits(bx["boxes"])) and len(got["boxes"]) > 0
        raw = debug_copy(c, 14, 0, np.uint32, 3 * len(r["elevated"])).reshape(-1, 3)
        assert np.array_equal(raw, bits(r["elevated"][:, :3]).reshape(-1, 3))
        assert np.array_equal(c.get_ground(0, n_hint=len(cloud))["mask"], r["mask"])
        del keep
