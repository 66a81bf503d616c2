"""The product's small pure device functions, driven directly through the test-only library tests/devcheck/primitives.hip: shared by
tests/test_primitives_gpu.py (the gfx950 build on the MI355X) and tests/test_emu_primitives.py (the host build, CPU suite). Every case takes the
library to run as an argument; the cases that compare two builds take the host build as `ref`.

  wave_case      every primitive of csrc/mot_wave.h, lane by lane, against a numpy restatement of the header's PROSE (not of either body): integer ops
                 exact, sums in float64 along the documented tree (partner at lane distance 1, 2, 4, 8: IEEE-exact, so bit for bit), NaN equal to NaN
  block_scan_case  the workgroup collective of the same header, block_scan_excl_i32, thread by thread against numpy's cumsum in wrapping int32: 128 to 1024 threads, one
                 and two components, one round and three rounds chained through the caller's carry and barrier (one body for both builds, over wave_scan_incl_i32)
  math_case      mot_atanf / mot_atan2f / the exact polar cell and bin / the Cartesian cell as compiled for the device, against the host build of the
                 same file (which tests/test_math_exact.py ties to glibc), bit for bit
  det5_case, wrap_pi_case, inv2_case   the tracker's scalar fp64 helpers (csrc/mot_track_prep.h) against the oracle's own (oracle/mot_oracle_track.c)
  box_fp64_case  the box stage's fp64 library calls rounded to float (box.hip's rectangle epilogue) against the host build (glibc)
"""
import ctypes as C
import functools
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "devcheck"))
sys.path.insert(0, os.path.join(HERE, "emu"))

f32, f64, i32, u32, u64 = np.float32, np.float64, np.int32, np.uint32, np.uint64
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
NUM_CHANNEL, NUM_BIN, MAX_GRID = 80, 120, 256    # MOT_NUM_CHANNEL, MOT_NUM_BIN, MOT_MAX_GRID of include/mot.h
vp = lambda a: a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------------------------------ the libraries
def _load(path):
    L = C.CDLL(path)
    L.mot_prim_wave.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.mot_prim_block_scan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.mot_prim_math.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
    for fn in (L.mot_prim_det5, L.mot_prim_inv2, L.mot_prim_wrap_pi):
        fn.argtypes = [C.c_void_p, C.c_long, C.c_void_p]
    L.mot_prim_box_fp64.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p]
    return L


@functools.lru_cache(None)
def device_lib():
    """the gfx950 build (hipcc, the product's flags)"""
    import build_primitives
    return _load(build_primitives.build())


@functools.lru_cache(None)
def host_lib():
    """the host build of the same file (tests/emu/hipemu.h, -ffp-contract=off -fno-fast-math)"""
    import build_primitives
    return _load(build_primitives.build_emu())


def same_bits(a, b):
    """elementwise: the same bit pattern, or both NaN (floats only)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.kind != "f":
        return a == b
    bits = {4: u32, 8: u64}[a.dtype.itemsize]
    return (a.view(bits) == b.view(bits)) | (np.isnan(a) & np.isnan(b))


def first_bad(ok, *show):
    """(index, values there) of the first mismatch, for the assertion message"""
    bad = np.argwhere(~ok)
    if not len(bad):
        return None
    k = tuple(bad[0])
    return (int(len(bad)), k) + tuple(repr(s[k]) for s in show)


# ------------------------------------------------------------------------------------------------------------------ 1 wave and row primitives
WAVE_IN = np.dtype([("id_min", i32), ("id_max", i32), ("bcast_lane", i32), ("fill", i32), ("vi", i32, 256), ("vu", u64, 256), ("vd", f64, (256, 8))])
WAVE_OUT = np.dtype([(k, i32, 256) for k in ("rmin", "rmax", "rmin_id", "rmax_id", "scan", "sum", "bcast", "prev", "next", "idx8")] +
                    [(k, u64, 256) for k in ("umin", "umax", "uor", "row_or")] + [("row_sum", f64, 256), ("row_sum8", f64, 256)])
BCAST_LANES = (0, 15, 16, 31, 32, 63)
LANE = np.arange(256) % 64
WAVE = np.arange(256) // 64


def wave_cases():
    """the records (WAVE_IN) and, per record, what it is about. Every record carries different data in every wave and row; a record aimed at one
    primitive still goes through all of them."""
    rng = np.random.default_rng(20240611)
    recs, names = [], []

    def new(name, vi=None, vu=None, vd0=None, fill=None, lane=None):
        r = np.zeros((), WAVE_IN)
        k = len(recs)
        r["id_min"], r["id_max"] = INT_MAX, INT_MIN
        r["bcast_lane"] = (list(BCAST_LANES) + list(range(64)))[k % 70] if lane is None else lane
        r["fill"] = (-7 - k, INT_MIN, INT_MAX, 0)[k % 4] if fill is None else fill
        r["vi"] = rng.integers(-10 ** 6, 10 ** 6, 256) if vi is None else vi
        r["vu"] = rng.integers(0, 2 ** 64, 256, dtype=u64) if vu is None else vu
        r["vd"] = rng.standard_normal((256, 8)) * 10.0 ** rng.integers(-8, 9, (256, 8))
        if vd0 is not None:
            r["vd"][:, 0] = vd0
            for j in range(1, 8):   # the other seven columns of row_sum8_f64: the same terms, rotated differently in every row
                r["vd"][:, j] = np.concatenate([np.roll(vd0[q * 16:(q + 1) * 16], j + q) for q in range(16)])
        recs.append(r); names.append(name)

    own = lambda L: (L + 21 * WAVE) % 64    # the lane that holds the special value in each of the four waves: over L = 0..63 every lane of every wave
    # -- wave_reduce_i32 / _id: the extremum at each lane in turn, all others equal
    for L in range(64):
        base = 1000 + 17 * WAVE
        new("min at lane %d" % L, vi=np.where(LANE == own(L), base - 5 - WAVE, base))
        new("max at lane %d" % L, vi=np.where(LANE == own(L), base + 5 + WAVE, base))
    for L in range(0, 64, 5):   # the callers' pattern: every lane but one hands in the identity (box.hip: `mine ? key : kNoMin`)
        new("only lane %d has a key (min)" % L, vi=np.where(LANE == own(L), -123456 + WAVE, INT_MAX))
        new("only lane %d has a key (max)" % L, vi=np.where(LANE == own(L), -123456 + WAVE, INT_MIN))
    new("all equal", vi=np.repeat([7, -7, 0, INT_MIN], 64))
    new("all INT_MAX / all INT_MIN", vi=np.repeat([INT_MAX, INT_MIN, INT_MAX, INT_MIN], 64))
    for s in range(4):
        v = rng.integers(INT_MIN, INT_MAX, 256, endpoint=True)
        v[rng.integers(0, 64, 4) + 64 * np.arange(4)] = INT_MIN
        v[(rng.integers(0, 64, 4) + 64 * np.arange(4)) ^ 1] = INT_MAX      # (^ 1: never the lane that got INT_MIN)
        new("INT_MIN and INT_MAX together %d" % s, vi=v)
    for s in range(8):
        new("random %d" % s, vi=rng.integers(INT_MIN, INT_MAX, 256, endpoint=True))
    # -- wave_reduce_u64: the halves travel in separate DPP moves
    H = (np.array([5, 0xffffffff, 0x80000000, 0])[WAVE]).astype(u64) << u64(32)
    for s in range(4):
        new("tie in the high word %d" % s, vu=H | rng.integers(0, 2 ** 32, 256, dtype=u64))
        new("tie in the low word %d" % s, vu=(rng.integers(0, 2 ** 32, 256, dtype=u64) << u64(32)) | u64(0x80000000 + s))
        new("halves crossed %d" % s, vu=np.where(rng.integers(0, 2, 256) == 1, u64(1) << u64(32), u64(0xffffffff)))   # min 0x0_ffffffff, max 0x1_00000000: a mixed pair is neither
    for L in range(64):
        o = LANE == own(L)
        new("u64 min in the low word at lane %d" % L, vu=np.where(o, H | u64(0x7fffffff), H | u64(0x80000000)))
        new("u64 max in the low word at lane %d" % L, vu=np.where(o, H | u64(0x80000001), H | u64(0x80000000)))
        bit = u64(1) << ((5 * L + WAVE) % 64).astype(u64)
        new("one bit, owned by lane %d" % L, vu=np.where(o, bit, u64(0)))
        new("all but one bit, lane %d" % L, vu=np.where(o, ~bit, ~u64(0)))
        new("every lane its own bit, rotated by %d" % L, vu=u64(1) << ((LANE + L + 3 * WAVE) % 64).astype(u64))
    # -- wave_scan_incl_i32 / wave_sum_i32 / wave_bcast_i32
    new("ones", vi=np.ones(256, i32))
    for L in range(64):
        new("a single 1 at lane %d" % L, vi=(LANE == own(L)).astype(i32), lane=L)
    for s in range(4):
        new("mixed signs %d" % s, vi=rng.integers(-1000, 1000, 256))
        new("running sum wraps 2^32 %d" % s, vi=rng.integers(2 ** 29, INT_MAX, 256) * rng.choice([1, 1, 1, -1], 256))
    new("running sum wraps 2^32: all INT_MAX", vi=np.full(256, INT_MAX))
    # -- row_sum_f64 / row_sum8_f64
    canc = np.array([1e16, 1.0, -1e16, 3.0, 1e-3, -1.0, 2.0 ** 53, -2.0 ** 53, 1.0, 1e16, -1e16, 0.5, 2.0 ** -1074, 1e300, -1e300, 7.0])
    for s in range(6):
        new("cancelling terms %d" % s, vd0=np.concatenate([rng.permutation(canc) * (1 + q) for q in range(16)]))
    den = np.array([2.0 ** -1074, -2.0 ** -1074, 2.0 ** -1060, 2.0 ** -1022, -2.0 ** -1023, 3 * 2.0 ** -1074, 0.0, -0.0] * 2)
    for s in range(3):
        new("denormals %d" % s, vd0=np.concatenate([rng.permutation(den) * (1 + (q % 3)) for q in range(16)]))
    z = np.zeros(256); z[16:32] = -0.0; z[32:48] = np.where(np.arange(16) % 2, -0.0, 0.0); z[48:64] = np.where(np.arange(16) == 9, 0.0, -0.0)
    z[64:] = np.where(rng.integers(0, 2, 192) == 1, -0.0, 0.0)
    new("+-0.0: a row of -0.0 sums to -0.0", vd0=z)
    for s, (row, lane) in enumerate(((0, 0), (5, 15), (10, 7), (15, 8))):
        v = rng.standard_normal(256)
        v[row * 16 + lane] = np.nan
        inf_row = (row + 3) % 16
        v[inf_row * 16 + (lane + 1) % 16] = np.inf
        both = (row + 7) % 16
        v[both * 16 + 2] = np.inf; v[both * 16 + 13] = -np.inf       # inf - inf: NaN in that row only
        new("NaN in row %d, inf in row %d, +-inf in row %d" % (row, inf_row, both), vd0=v)
    for s in range(6):
        new("random doubles %d" % s)
    assert set(BCAST_LANES) <= set(int(r["bcast_lane"]) for r in recs)
    return np.stack(recs), names


def row_tree(v):
    """the documented addition tree over each row of 16 lanes (last axis): partial = own partial + partner's partial at lane distances 1, 2, 4, 8"""
    v = np.array(v, f64)
    lane = np.arange(16)
    with np.errstate(all="ignore"):
        for d in (1, 2, 4, 8):
            v = v + v[..., lane ^ d]
    return v


def wave_reference(c):
    """what mot_wave.h's prose promises for the records `c`, in plain numpy"""
    n = len(c)
    o = np.zeros(n, WAVE_OUT)
    vi = c["vi"].reshape(n, 4, 64); vu = c["vu"].reshape(n, 4, 64)
    spread = lambda w: np.repeat(w[..., None], 64, -1).reshape(n, 256)     # every lane of a wave receives the wave's result
    o["rmin"] = o["rmin_id"] = spread(vi.min(-1)); o["rmax"] = o["rmax_id"] = spread(vi.max(-1))
    scan = np.cumsum(vi.astype(np.int64).astype(u32), -1, dtype=u32).view(i32)       # two's complement: the running sum wraps modulo 2^32
    o["scan"] = scan.reshape(n, 256); o["sum"] = spread(scan[..., 63])
    o["bcast"] = spread(np.take_along_axis(vi, np.broadcast_to(c["bcast_lane"][:, None, None], (n, 4, 1)), -1)[..., 0])
    rows = c["vi"].reshape(n, 16, 16)
    fill = np.broadcast_to(c["fill"][:, None, None], (n, 16, 1))
    o["prev"] = np.concatenate([fill, rows[..., :-1]], -1).reshape(n, 256); o["next"] = np.concatenate([rows[..., 1:], fill], -1).reshape(n, 256)
    o["umin"] = spread(vu.min(-1)); o["umax"] = spread(vu.max(-1)); o["uor"] = spread(np.bitwise_or.reduce(vu, -1))
    o["row_or"] = np.repeat(np.bitwise_or.reduce(c["vu"].reshape(n, 16, 16), -1)[..., None], 16, -1).reshape(n, 256)
    o["row_sum"] = row_tree(c["vd"][:, :, 0].reshape(n, 16, 16)).reshape(n, 256)
    return o


def wave_case(lib):
    cases, names = wave_cases()
    sizes = (C.c_int(), C.c_int())
    lib.mot_prim_wave_sizes(C.byref(sizes[0]), C.byref(sizes[1]))
    assert (sizes[0].value, sizes[1].value) == (WAVE_IN.itemsize, WAVE_OUT.itemsize)
    # the identities are identities for these records (what every caller guarantees)
    assert (cases["vi"] <= cases["id_min"][:, None]).all() and (cases["vi"] >= cases["id_max"][:, None]).all()
    got = np.zeros(len(cases), WAVE_OUT)
    assert lib.mot_prim_wave(vp(cases), len(cases), vp(got)) == 0
    want = wave_reference(cases)
    for k in WAVE_OUT.names:
        if k in ("idx8", "row_sum8"):
            continue
        ok = same_bits(got[k], want[k])
        assert ok.all(), (k, [names[i] for i in np.unique(np.argwhere(~ok)[:, 0])[:5]], first_bad(ok, got[k], want[k]))
    # row_sum8_index: onto 0..7 within each half-row, the same in every row; lane L receives exactly row_sum_f64(v[row_sum8_index(L)])
    idx = got["idx8"].reshape(len(cases), 16, 16)
    assert (idx == idx[0, 0]).all()
    assert sorted(idx[0, 0, :8]) == list(range(8)) and sorted(idx[0, 0, 8:]) == list(range(8)), idx[0, 0]
    sums = row_tree(np.moveaxis(cases["vd"].reshape(len(cases), 16, 16, 8), -1, -2))          # [case, row, column j, lane]: the complete sum of v[j]
    want8 = np.take_along_axis(sums, np.broadcast_to(idx[0, 0][None, None, None, :], (len(cases), 16, 1, 16)), 2)[:, :, 0, :].reshape(len(cases), 256)
    ok = same_bits(got["row_sum8"], want8)
    assert ok.all(), ("row_sum8", [names[i] for i in np.unique(np.argwhere(~ok)[:, 0])[:5]], first_bad(ok, got["row_sum8"], want8))
    # ... which for the lanes whose index is 0 is row_sum_f64's own result on the same inputs, bit for bit (the header's promise)
    sel = np.broadcast_to(np.tile(idx[0, 0] == 0, 16)[None, :], got["row_sum"].shape)
    assert sel.any() and same_bits(got["row_sum8"][sel], got["row_sum"][sel]).all()
    return len(cases)


# ------------------------------------------------------------------------------------------------------------------ 1b the workgroup scan
BLOCK_SCAN_WAVES = (2, 4, 8, 16)     # 128, 256, 512, 1024 threads: the block sizes of the call sites in csrc/
BLOCK_SCAN_ROUNDS = (1, 3)


def block_scan_values(waves, rounds):
    """[(what, values (rounds, waves * 64))] for one component; the rounds of a case are chained through the caller's carry"""
    rng = np.random.default_rng(20241020 + 100 * waves + rounds)
    T = waves * 64
    shape = (rounds, T)
    out = [("all zeros", np.zeros(shape, np.int64)), ("all ones", np.ones(shape, np.int64))]
    edges = sorted({0, 63, 64, T - 1} | {64 * w for w in range(waves)} | {64 * w + 63 for w in range(waves)})
    for k, t in enumerate(edges):    # (the round moves with the position, so that with three rounds the value also travels through the carry)
        v = np.zeros(shape, np.int64)
        v[k % rounds, t] = 5 + k
        out.append(("a single value at thread %d of round %d" % (t, k % rounds), v))
    w, r = np.arange(T) // 64, np.arange(rounds)[:, None]
    out.append(("a constant per wave", 1 + 3 * w[None, :] * (w[None, :] + 2) + 1000 * r))    # strictly convex in the wave: no two orders of the waves give the same prefixes
    for s in range(3):
        out.append(("random in [0, 2^20] %d" % s, rng.integers(0, 2 ** 20, shape, endpoint=True)))
        out.append(("random of both signs %d" % s, rng.integers(-2 ** 20, 2 ** 20, shape, endpoint=True)))
    out.append(("sparse: most threads hand in 0", rng.integers(1, 9, shape) * (rng.integers(0, 8, shape) == 0)))
    out.append(("the running sum passes 2^31", rng.integers(2 ** 29, 2 ** 30, shape)))
    out.append(("the running sum passes 2^31 both ways", rng.integers(2 ** 29, INT_MAX, shape) * rng.choice([1, 1, -1], shape)))
    out.append(("all INT_MAX", np.full(shape, INT_MAX, np.int64)))
    return out


def block_scan_reference(v):
    """v (cases, rounds, threads, n) int32 -> what csrc/mot_wave.h promises, the rounds chained by `carry += total`: the exclusive running sum over rounds x threads and
    each round's total, per component, in 32-bit two's complement (the sums wrap)"""
    n_cases, rounds, T, n = v.shape
    u = v.astype(np.int64).astype(u32)
    flat = np.moveaxis(u, -1, 1).reshape(n_cases, n, rounds * T)
    excl = (np.cumsum(flat, -1, dtype=u32) - flat).reshape(n_cases, n, rounds, T)
    return np.ascontiguousarray(np.moveaxis(excl, 1, -1)).view(i32), np.ascontiguousarray(u.sum(2, dtype=u32)).view(i32)


def block_scan_case(lib):
    """block_scan_excl_i32 thread by thread at every block size of the product, one and two components, one round and three chained rounds"""
    total = 0
    for waves, rounds, n in itertools.product(BLOCK_SCAN_WAVES, BLOCK_SCAN_ROUNDS, (1, 2)):
        vals = block_scan_values(waves, rounds)
        names = [what for what, _ in vals]
        cols = [np.stack([a for _, a in vals])]
        if n == 2:   # the second component: the NEXT case's values, so that the two columns of a case always differ (and come from different generators)
            cols.append(np.roll(cols[0], -1, 0))
            assert (cols[0] != cols[1]).reshape(len(vals), -1).any(1).all()
        v = np.ascontiguousarray(np.stack(cols, -1).astype(np.int64).astype(u32).view(i32))      # (cases, rounds, threads, n)
        assert v.shape == (len(vals), rounds, waves * 64, n)
        excl, tot = np.full(v.shape, -77, i32), np.full((len(vals), rounds, n), -77, i32)
        assert lib.mot_prim_block_scan(vp(v), len(vals), waves, n, rounds, vp(excl), vp(tot)) == 0
        want_excl, want_tot = block_scan_reference(v)
        what = "%d waves, %d component(s), %d round(s)" % (waves, n, rounds)
        ok = excl == want_excl
        assert ok.all(), (what, [names[i] for i in np.unique(np.argwhere(~ok)[:, 0])[:5]], first_bad(ok, excl, want_excl))
        ok = tot == want_tot
        assert ok.all(), (what, "totals", [names[i] for i in np.unique(np.argwhere(~ok)[:, 0])[:5]], first_bad(ok, tot, want_tot))
        total += len(vals)
    return total


# ------------------------------------------------------------------------------------------------------------------ 2 the exact fp32 math
DEV_PARAMS_HEAD = np.dtype([("r_min", f32), ("r_max", f32), ("r_span", f32), ("k_bin", f32), ("t", f32, 4), ("ground_margin", f64), ("gk", f64, 3), ("crop_enable", i32),
                            ("crop", f32, 6), ("num_grid", i32), ("occ_min_count", i32), ("dilate", i32), ("roi_m", f32), ("roi_half", f32)])   # struct MotDevParams (csrc/mot_internal.h), its head
SPECIALS = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 3.4e38, -3.4e38, 2.0 ** 26, 2.0 ** 25, float.fromhex("0x1.fffffep24"), 2.0 ** -29,
                     float.fromhex("0x1.fffffep-30"), 0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** 61, 2.0 ** -61, float.fromhex("0x1.b42faep+25")], f32)   # tests/test_math_exact.py's sp[] table
MATH_RANDOM = 1 << 20    # pairs of random bit patterns
ATAN_BREAKS = np.array([2.0 ** -29, 0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** 25], f32)


def dev_params(ctx, lib):
    dp = (C.c_char * 512)()
    assert lib.mot_debug_dev_params(ctx._h, dp, C.c_size_t(512)) == 0
    return dp


def ulp_steps(v, k):
    """v moved by k representable steps (sign-magnitude walk, as tests/devcheck/sweep.hip's ulp_step: fine away from 0)"""
    i = np.ascontiguousarray(v, f32).view(i32).astype(np.int64)
    return (i + np.where(i >= 0, k, -k)).astype(i32).view(f32)


@functools.lru_cache(None)
def math_inputs_common():
    """(x, y) that do not depend on the parameters, 1.4 M pairs"""
    rng = np.random.default_rng(31337)
    bits = lambda n: rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(u32).view(f32)
    X, Y = [], []
    n = MATH_RANDOM
    X.append(bits(n)); Y.append(bits(n))                                                     # any bit pattern in both operands
    sx, sy = np.meshgrid(SPECIALS, SPECIALS)
    X.append(sx.ravel()); Y.append(sy.ravel())                                               # the specials, each against each
    br = np.concatenate([ulp_steps(ATAN_BREAKS, k) for k in range(-8, 9)])                  # every atanf breakpoint +-8 ulp, both signs
    br = np.concatenate([br, -br])
    m = 64
    X.append(np.tile(br, m)); Y.append(np.concatenate([bits(len(br) * (m - 2)), np.ones(len(br), f32), -np.ones(len(br), f32)]))   # (as x of atanf; with y = +-1 ...)
    X.append(np.concatenate([np.ones(len(br), f32), -np.ones(len(br), f32)])); Y.append(np.tile(br, 2))                             # ... and as the quotient y / x of atan2f
    t = (rng.uniform(1, 2, len(br) * 32)).astype(f32) * f32(2.0) ** rng.integers(-20, 21, len(br) * 32).astype(f32)
    X.append(t * rng.choice(f32([1, -1]), len(t))); Y.append(np.tile(br, 32) * t)                                                   # quotients that round to the neighbourhood of a breakpoint
    k = 1 << 16
    mant = lambda n: rng.uniform(1, 2, n).astype(f32)
    sign = lambda n: rng.choice(f32([1, -1]), n)
    ey = rng.integers(-126, -60, k); ex = ey + rng.integers(127, 150, k)                     # y / x below 2^-126: denormal quotients (and some that underflow to 0)
    X.append(sign(k) * mant(k) * f32(2.0) ** np.minimum(ex, 127).astype(f32)); Y.append(sign(k) * mant(k) * f32(2.0) ** ey.astype(f32))
    gap = rng.integers(55, 67, k) * rng.choice([1, -1], k)                                   # exponent gaps around the k > 60 / k < -60 branches
    e0 = rng.integers(-30, 31, k)
    X.append(sign(k) * mant(k) * f32(2.0) ** e0.astype(f32)); Y.append(sign(k) * mant(k) * f32(2.0) ** (e0 + gap).astype(f32))
    den = lambda n: (rng.integers(1, 2 ** 23, n).astype(u32) | (rng.integers(0, 2, n).astype(u32) << u32(31))).view(f32)
    X.append(den(k)); Y.append(den(k))                                                       # denormal x and y
    X.append(den(k)); Y.append(bits(k))
    X.append(bits(k)); Y.append(den(k))
    return np.concatenate(X).astype(f32), np.concatenate(Y).astype(f32)


def math_inputs_boundaries(h, seed):
    """(x, y) on the cell boundaries of the parameters `h` (DEV_PARAMS_HEAD), moved by -3..+3 steps of 1..64 ulp in x and in y — the sweep's mode 2, built on the
    host: every channel spoke at random radii, every bin ring at random angles, every grid line of the Cartesian grid; and radii within 3 ulp of r_min and r_max"""
    rng = np.random.default_rng(seed)
    r_min, r_max, span, G, roi, half = h["r_min"], h["r_max"], h["r_span"], int(h["num_grid"]), h["roi_m"], h["roi_half"]
    per = 1 << 17
    X, Y = [], []
    # spokes
    k = np.tile(np.arange(NUM_CHANNEL + 1), per // (NUM_CHANNEL + 1) + 1)[:per]
    a = -np.pi + k * (2 * np.pi / NUM_CHANNEL)
    r = (r_min * f32(0.5) + rng.uniform(0, 1, per).astype(f32) * (r_max * f32(1.05) - r_min * f32(0.5))).astype(f64)
    X.append((np.cos(a) * r).astype(f32)); Y.append((np.sin(a) * r).astype(f32))
    # rings (the range limits are rings 0 and 120), as the reference's expression places them
    k = np.tile(np.arange(NUM_BIN + 1), per // (NUM_BIN + 1) + 1)[:per]
    r = (r_min + k.astype(f32) * (span / f32(NUM_BIN))).astype(f64)
    a = rng.uniform(-np.pi, np.pi, per)
    X.append((np.cos(a) * r).astype(f32)); Y.append((np.sin(a) * r).astype(f32))
    # grid lines
    k = np.tile(np.arange(G + 1), per // (G + 1) + 1)[:per]
    line = (-half + k.astype(f32) * (roi / f32(G))).astype(f32)
    other = (rng.uniform(-1, 1, per).astype(f32) * f32(1.2) * half).astype(f32)
    xy = rng.integers(0, 2, per) == 1
    X.append(np.where(xy, line, other)); Y.append(np.where(xy, other, line))
    x, y = np.concatenate(X), np.concatenate(Y)
    step = lambda n: (rng.integers(0, 7, n) - 3) * (1 << rng.integers(0, 7, n))
    x, y = ulp_steps(x, step(len(x))), ulp_steps(y, step(len(y)))
    # distances within 3 ulp of either range limit: a random direction scaled onto the wanted fp32 distance
    n = 1 << 15
    a = rng.uniform(-np.pi, np.pi, n)
    want = ulp_steps(np.where(rng.integers(0, 2, n) == 1, r_max, r_min).astype(f32), rng.integers(-3, 4, n)).astype(f64)
    qx, qy = (np.cos(a) * want).astype(f32), (np.sin(a) * want).astype(f32)
    d = np.sqrt(qx * qx + qy * qy, dtype=f32)
    lim = np.minimum(np.abs(d.view(i32).astype(np.int64) - r_min.view(i32)), np.abs(d.view(i32).astype(np.int64) - r_max.view(i32)))
    assert (lim <= 3).mean() > 0.5 and all(((d.view(i32).astype(np.int64) - L.view(i32)) == s).any() for L in (r_min, r_max) for s in range(-3, 4))
    return np.concatenate([x, qx]).astype(f32), np.concatenate([y, qy]).astype(f32)


def run_math(lib, dp, x, y):
    x, y = np.ascontiguousarray(x, f32), np.ascontiguousarray(y, f32)
    out = np.zeros((5, len(x)), i32)
    assert lib.mot_prim_math(dp, vp(x), vp(y), len(x), vp(out)) == 0
    return dict(atanf=out[0].view(f32), atan2f=out[1].view(f32), polar_cell=out[2], polar_bin=out[3], cart=out[4])


def math_models(h, x, y, at):
    """the polar cell (given the angle `at` = atan2f(y, x)), the bin and the Cartesian cell in numpy fp32, operation by operation (every one of them IEEE-exact: +, *, /,
    sqrt, floor, fp32 <-> fp64) — independent of both builds"""
    with np.errstate(all="ignore"):
        d = np.sqrt(x * x + y * y, dtype=f32)
        fb = np.floor((d - h["r_min"]) / h["r_span"] * f32(NUM_BIN))
        bin_ = np.where(~((d <= h["r_min"]) | (d >= h["r_max"])) & (fb >= 0) & (fb < NUM_BIN), fb, -1).astype(i32)
        fc = np.floor(((at.astype(f64) + 3.14159265358979323846) / (2 * 3.14159265358979323846)).astype(f32) * f32(NUM_CHANNEL))
        cell = np.where((bin_ >= 0) & (fc >= 0) & (fc < NUM_CHANNEL), np.nan_to_num(fc) * NUM_BIN + bin_, -1).astype(i32)
        G, roi = f32(h["num_grid"]), h["roi_m"]
        xc, yc = x + h["roi_half"], y + h["roi_half"]
        fx, fy = np.floor(G * xc / roi), np.floor(G * yc / roi)
        inside = ~((xc < 0) | (xc >= roi) | (yc < 0) | (yc >= roi)) & (fx >= 0) & (fx < G) & (fy >= 0) & (fy < G)
        cart = np.where(inside, np.nan_to_num(fx) * MAX_GRID + np.nan_to_num(fy), -1).astype(i32)
    return cell, bin_, cart


def math_settings(mot, lib_path=None):
    """the two presets and the polar range on the edge of the declared domain (tests/param_cases.py: r_max / (r_max - r_min) = 4)"""
    import param_cases as PC
    r_min, r_max = PC.POLAR_RANGES[3]
    assert r_max / (r_max - r_min) == 4.0
    L = mot.load_library(lib_path)
    return [("preset 0", mot.params(0, lib=L)), ("preset 1", mot.params(1, lib=L)), ("polar range %g..%g" % (r_min, r_max), mot.params(0, lib=L, r_min=r_min, r_max=r_max))]


def math_case(mot, lib, ref, ctx_lib_path=None):
    """`lib` against `ref` (the host build) on the same MotDevParams bytes, which come from a context of the library at ctx_lib_path"""
    L = mot.load_library(ctx_lib_path)
    total = 0
    libm = C.CDLL("libm.so.6")
    libm.atan2f.restype = C.c_float; libm.atan2f.argtypes = [C.c_float, C.c_float]
    for s, (name, p) in enumerate(math_settings(mot, ctx_lib_path)):
        with mot.Context(p, lib_path=ctx_lib_path, max_points=1024) as c:
            dp = dev_params(c, L)
        h = np.frombuffer(dp, DEV_PARAMS_HEAD, 1)[0]
        assert h["r_min"] == f32(p.r_min) and h["r_max"] == f32(p.r_max) and h["r_span"] == f32(p.r_max) - f32(p.r_min) and h["num_grid"] == p.num_grid \
            and h["roi_m"] == f32(p.roi_m) and h["roi_half"] == f32(p.roi_m) / f32(2), "DEV_PARAMS_HEAD no longer mirrors MotDevParams"
        bx, by = math_inputs_boundaries(h, 1000 + s)
        cx, cy = math_inputs_common()
        x, y = np.concatenate([bx, cx]), np.concatenate([by, cy])
        want = run_math(ref, dp, x, y)
        # the host build itself, against what does not share its code: the bin and the Cartesian cell in numpy, atan2f of the C library on the specials
        cell, bin_, cart = math_models(h, x, y, want["atan2f"])
        assert np.array_equal(want["polar_bin"], bin_) and np.array_equal(want["cart"], cart) and np.array_equal(want["polar_cell"], cell), name
        assert (cell >= 0).sum() > 1 << 17 and (cart >= 0).sum() > 1 << 17, name
        if s == 0:
            k = len(bx) + MATH_RANDOM
            sp = slice(k, k + len(SPECIALS) ** 2)
            glibc = np.array([libm.atan2f(float(b), float(a)) for a, b in zip(x[sp], y[sp])], f32)
            assert same_bits(want["atan2f"][sp], glibc).all()
        got = run_math(lib, dp, x, y)
        for k in want:
            ok = same_bits(got[k], want[k])
            assert ok.all(), (name, k, first_bad(ok, x, y, got[k], want[k]))
        total += len(x)
    assert total >= 1 << 22, total
    return total


# ------------------------------------------------------------------------------------------------------------------ 3 the tracker's scalar helpers
def _orc():
    import oracle_lib
    o = oracle_lib.orc()
    o.orc_det5.restype = C.c_double; o.orc_det5.argtypes = [C.c_void_p]
    o.orc_inv2.restype = None; o.orc_inv2.argtypes = [C.c_void_p, C.c_void_p]
    o.orc_wrap_pi.restype = C.c_double; o.orc_wrap_pi.argtypes = [C.c_double]
    return o


def run_det5(lib, m):
    m = np.ascontiguousarray(m, f64).reshape(-1, 25)
    out = np.zeros(len(m))
    assert lib.mot_prim_det5(vp(m), len(m), vp(out)) == 0
    return out


def oracle_det5(m):
    o = _orc()
    m = np.ascontiguousarray(m, f64).reshape(-1, 25)
    return np.array([o.orc_det5(vp(r)) for r in m])


def det5_matrices():
    """[(what, matrices (n, 5, 5))]"""
    rng = np.random.default_rng(555)
    sets = []
    perms = np.array([np.eye(5)[list(p)] for p in itertools.permutations(range(5))])
    sets.append(("the 120 permutation matrices", perms))
    sets.append(("permutation matrices, rows scaled", perms * rng.uniform(0.5, 20, (120, 5, 1)) * rng.choice([1.0, -1.0], (120, 5, 1))))
    sets.append(("permutation matrices, scaled, with off-diagonal noise", perms * rng.uniform(0.5, 20, (120, 5, 1)) + rng.uniform(-1e-3, 1e-3, (120, 5, 5))))
    sets.append(("permutation matrices + noise of the entries' own size", perms * 3.0 + rng.uniform(-1, 1, (120, 5, 5))))
    # equal-magnitude pivot candidates: the earlier row must win
    t = rng.choice([1.0, -1.0], (400, 5, 5))
    sets.append(("entries +-1: every pivot search ties", t))
    t = rng.uniform(-1, 1, (200, 5, 5)); t[:, :, 0] = rng.choice([2.0, -2.0], (200, 5)); t[:, 2:, 1] = t[:, 1:2, 1] * rng.choice([1.0, -1.0], (200, 3))
    sets.append(("ties in the first two columns", t))
    t = perms.copy(); t[np.arange(120), rng.integers(0, 5, 120), :] += perms[np.arange(120), rng.integers(0, 5, 120), :]
    sets.append(("permutation matrices with one row added to another", t))
    # a zero column at elimination step k (the `done` latch): [[D, B], [0, C]] with C's first column zero, rows shuffled
    z = []
    for k in range(5):
        for rep in range(40):
            m = rng.uniform(-2, 2, (5, 5))
            m[:, :k] = 0
            m[np.arange(k), np.arange(k)] = rng.uniform(3, 9, k) * rng.choice([1.0, -1.0], k) * (1e200 if rep % 8 == 7 and k >= 2 else 1.0)   # (1e200 twice: inf * 0 = NaN)
            m[:k, k:] = rng.uniform(-2, 2, (k, 5 - k))
            m[k:, k] = rng.choice([0.0, -0.0], 5 - k)
            if rep % 2:
                m = m[rng.permutation(5)]
            z.append(m)
    sets.append(("a zero column at each elimination step", np.array(z)))
    t = []
    for base in (np.eye(5), rng.uniform(-3, 3, (5, 5)), (lambda a: a @ a.T)(rng.uniform(-1, 1, (5, 5)))):
        for pos in range(25):
            for v in (np.nan, np.inf, -np.inf):
                m = base.copy(); m.flat[pos] = v; t.append(m)
    sets.append(("NaN or inf at each position", np.array(t)))
    sets.append(("4096 random general matrices", rng.standard_normal((4096, 5, 5)) * 10.0 ** rng.integers(-3, 4, (4096, 1, 1))))
    sets.append(("random matrices with entries over many decades", rng.standard_normal((1024, 5, 5)) * 10.0 ** rng.integers(-6, 7, (1024, 5, 5))))
    return sets


def det5_guard_matrices():
    """symmetric positive definite A A^T scaled so that the determinant lies within a few ulp of 10 (the divergence guard, det5(Pm) > 10), on both sides"""
    rng = np.random.default_rng(556)
    out = []
    for _ in range(64):
        a = rng.uniform(-0.3, 0.3, (5, 5)) + np.diag(rng.uniform(1, 2, 5))     # well conditioned: the elimination's own rounding stays at a few ulp
        m = a @ a.T
        for _ in range(3):   # Newton on the scale: det(s m) = s^5 det(m)
            m = m * (10.0 / float(oracle_det5(m)[0])) ** 0.2
        for j in range(-6, 7):
            out.append(m * (1.0 + j * 2.0 ** -52))
    return np.array(out)


def det5_case(lib):
    n = 0
    for what, m in det5_matrices():
        got, want = run_det5(lib, m), oracle_det5(m)
        ok = same_bits(got, want)
        assert ok.all(), (what, first_bad(ok, got, want), m[np.argwhere(~ok)[0, 0]].tolist())
        n += len(m)
        if what.startswith("a zero column"):
            assert (want[~np.isnan(want)] == 0).all() and np.isnan(want).any() and (np.signbit(want)).any() and (~np.signbit(want)).any(), what
        if what.startswith("the 120"):
            assert sorted(want) == [-1.0] * 60 + [1.0] * 60
    g = det5_guard_matrices()
    got, want = run_det5(lib, g), oracle_det5(g)
    assert (np.abs(want - 10) < 1e-13).all() and (want > 10).sum() > 50 and (want <= 10).sum() > 50, "the guard matrices straddle 10"
    ok = same_bits(got, want)
    assert ok.all(), ("guard", first_bad(ok, got, want))
    return n + len(g)


def det5_exact_case(lib):
    """a check that does not share the algorithm: 1000 integer matrices with |entry| <= 4 against the exact determinant (Leibniz sum in Python integers — exact, as
    fractions.Fraction elimination would be), to 1e-12 x the Hadamard bound of the matrix: n^3 u growth <= 125 x 1.1e-16 x 16 = 2.2e-13 of that bound, factor 5 over it"""
    rng = np.random.default_rng(557)
    m = rng.integers(-4, 5, (1000, 5, 5))
    m[:20, 2] = m[:20, 0]; m[20:40, 3] = 0     # singular ones among them: a repeated row, a zero row
    perms = list(itertools.permutations(range(5)))
    sgn = [round(float(np.linalg.det(np.eye(5)[list(p)]))) for p in perms]
    got = run_det5(lib, m.astype(f64))
    for a, g in zip(m.tolist(), got):
        exact = sum(s * a[0][p[0]] * a[1][p[1]] * a[2][p[2]] * a[3][p[3]] * a[4][p[4]] for s, p in zip(sgn, perms))
        hadamard = float(np.prod(np.sqrt((np.array(a, f64) ** 2).sum(1))))
        assert abs(g - exact) <= 1e-12 * hadamard, (a, g, exact, hadamard)
    return len(m)


def run_wrap_pi(lib, a):
    a = np.ascontiguousarray(a, f64)
    out = np.full(len(a), 123.0)
    assert lib.mot_prim_wrap_pi(vp(a), len(a), vp(out)) == 0     # the kernel returns for every one of them: the reason the branch exists
    return out


def wrap_pi_case(lib):
    rng = np.random.default_rng(558)
    o = _orc()
    loop = lambda a: np.array([o.orc_wrap_pi(float(v)) for v in a])
    pi, lim = np.pi, 64.0 * np.pi
    nx = lambda v, k: np.nextafter(v, np.inf if k > 0 else -np.inf)
    # |a| <= 64 pi: the loop runs as written
    odd = np.array([k * pi for k in range(1, 64, 2)])
    a = np.concatenate([[0.0, -0.0, pi, nx(pi, 1), nx(pi, -1), lim, nx(lim, -1), 1e-300, 2.0 ** -1074], odd, nx(odd, 1), nx(odd, -1), rng.uniform(-lim, lim, 4000),
                        rng.uniform(-4, 4, 1000)])
    a = np.concatenate([a, -a])
    assert (np.abs(a) <= lim).all()
    got, want = run_wrap_pi(lib, a), loop(a)
    ok = same_bits(got, want)
    assert ok.all(), ("|a| <= 64 pi", first_bad(ok, a, got, want))
    # 64 pi < |a| < 1e4: whole turns come off in one step; within 1e-9 of the loop (the bound csrc/mot_track_prep.h states)
    a = np.concatenate([[nx(lim, 1), 9999.999], rng.uniform(lim, 1e4, 3000)])
    a = np.concatenate([a, -a])
    assert (np.abs(a) > lim).all() and (np.abs(a) < 1e4).all()
    got, want = run_wrap_pi(lib, a), loop(a)
    assert (np.abs(got - want) <= 1e-9).all(), ("64 pi < |a| < 1e4", a[np.argmax(np.abs(got - want))], np.abs(got - want).max())
    # up to 1e16: a result in [-pi, pi]
    a = np.concatenate([[1e4, 1e15, 1e16, 2.0 ** 53, 2.0 ** 53 + 2], 10.0 ** rng.uniform(4, 16, 4000)])
    a = np.concatenate([a, -a])
    got = run_wrap_pi(lib, a)
    assert (np.abs(got) <= pi).all(), ("|a| <= 1e16", a[~(np.abs(got) <= pi)][:4], got[~(np.abs(got) <= pi)][:4])
    # no digit of the angle means anything: NaN
    a = np.array([np.inf, -np.inf, np.nan, 1e18, -1e18, 1e300, -1e300])
    got = run_wrap_pi(lib, a)
    assert np.isnan(got).all(), (a.tolist(), got.tolist())


def inv2_case(lib):
    rng = np.random.default_rng(559)
    o = _orc()
    m = np.concatenate([rng.standard_normal((2000, 4)) * 10.0 ** rng.integers(-6, 7, (2000, 1)), rng.standard_normal((500, 4)) * 10.0 ** rng.integers(-150, 151, (500, 4)),
                        [[1, 2, 2, 4], [0, 0, 0, 0], [-0.0, 0, 0, -0.0], [1, 0, 0, 0], [0, 1, 0, 0], [3, 3, 3, 3], [1e200, 1e200, 1e200, 1e200], [2, -1, -4, 2], [1e-200, 0, 0, 1e-200]],
                        [[v if k == pos else 1.5 + k for k in range(4)] for pos in range(4) for v in (np.nan, np.inf, -np.inf, 0.0)]]).astype(f64)
    out = np.zeros((len(m), 5))
    assert lib.mot_prim_inv2(vp(m), len(m), vp(out)) == 0
    want = np.zeros((len(m), 4))
    for r, w in zip(m, want):
        o.orc_inv2(vp(r), vp(w))
    with np.errstate(all="ignore"):
        det = m[:, 0] * m[:, 3] - m[:, 1] * m[:, 2]
    assert (det == 0).sum() >= 6, "zero determinants among the inputs"
    ok = same_bits(out[:, :4], want)
    assert ok.all(), ("inv2", first_bad(ok, out[:, :4], want))
    ok = same_bits(out[:, 4], det)
    assert ok.all(), ("det2", first_bad(ok, out[:, 4], det))


# ------------------------------------------------------------------------------------------------------------------ 4 the box stage's fp64 calls
BOX_FP64_NAMES = ("sqrt", "atan2", "cos", "sin")


@functools.lru_cache(None)
def box_fp64_inputs():
    """mode 0: every integer (dx, dy) in [-899, 899]^2 — the whole domain of the two-point hull branch (pixel indices); mode 1: 2^22 pairs (o2, o3) = a unit
    direction times a width in (0, 900], what the rotating-calipers branch feeds the same calls"""
    g = np.arange(-899, 900, dtype=f32)
    dx, dy = np.meshgrid(g, g)
    rng = np.random.default_rng(560)
    n = 1 << 22
    a = rng.uniform(-np.pi, np.pi, n)
    w = (1.0 - rng.uniform(0, 1, n)) * 900.0            # (0, 900]
    return (np.ascontiguousarray(dx.ravel()), np.ascontiguousarray(dy.ravel())), ((np.cos(a) * w).astype(f32), (np.sin(a) * w).astype(f32))


def run_box_fp64(lib, a, b, mode):
    out = np.zeros((4, len(a)), f32)
    assert lib.mot_prim_box_fp64(vp(a), vp(b), len(a), mode, vp(out)) == 0
    return out


@functools.lru_cache(None)
def box_fp64_reference():
    """the host build (glibc) on both input sets, computed once; its width is also held against numpy's correctly rounded square root"""
    ref = host_lib()
    out = []
    for mode, (a, b) in enumerate(box_fp64_inputs()):
        r = run_box_fp64(ref, a, b, mode)
        assert np.array_equal(r[0], np.sqrt(a.astype(f64) ** 2 + b.astype(f64) ** 2).astype(f32))
        out.append(r)
    return out


def box_fp64_measure(lib):
    """per input set and function: how many of the floats differ from the host build's, the largest difference in fp32 ulp, and the inputs"""
    res = []
    for mode, (a, b) in enumerate(box_fp64_inputs()):
        got, want = run_box_fp64(lib, a, b, mode), box_fp64_reference()[mode]
        for k, name in enumerate(BOX_FP64_NAMES):
            bad = np.nonzero(~same_bits(got[k], want[k]))[0]
            ulp = np.abs(got[k][bad].view(i32).astype(np.int64) - want[k][bad].view(i32).astype(np.int64))
            res.append(dict(mode=mode, name=name, n=len(a), bad=len(bad), max_ulp=int(ulp.max()) if len(bad) else 0,
                            inputs=[(float(a[i]), float(b[i]), float(got[k][i]), float(want[k][i])) for i in bad[:32]]))
    return res


def box_fp64_case(lib):
    res = box_fp64_measure(lib)
    for r in res:
        print("box fp64: %s, %s of %d inputs: %d differ from glibc (max %d ulp) %s" % (("integer (dx, dy)", "direction x width")[r["mode"]], r["name"], r["n"], r["bad"], r["max_ulp"], r["inputs"][:4]))
    assert sum(r["n"] for r in res) // 4 == 1799 * 1799 + (1 << 22)
    for r in res:
        assert r["bad"] == 0, r
    return res
