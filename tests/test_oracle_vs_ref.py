"""Pins the C restatement (oracle/mot_oracle_*.c): (a) against the golden vectors generated from the reference's own
sources (tests/golden/, always), (b) live against oracle/_ref when that library is present (the build container and
any box the prebuilt .so travelled to)."""
import os

import numpy as np
import pytest

import golden_util as G


@pytest.mark.parametrize("name", G.FRAMES)
def test_restatement_matches_golden_frames(oracle, name):
    fx = G.load(name)
    p = oracle.params(0)
    g = oracle.ground_remove(p, fx["cloud"], want_dump=True)
    cl = oracle.cluster(p, g["elevated"])
    bx = oracle.box_fit(p, g["elevated"], cl["grid"], cl["num_cluster"])
    G.check_frame(fx, g, cl, bx["boxes"], polar=g)


@pytest.mark.parametrize("name", G.FRAMES_OT0)
def test_restatement_matches_golden_frames_ot0(oracle, name):
    """preset 1 against the fixture generated from object_tracking0's own sources"""
    fx = G.load(name)
    p = oracle.params(1)
    g = oracle.ground_remove(p, fx["cloud"])
    cl = oracle.cluster(p, g["elevated"])
    bx = oracle.box_fit(p, g["elevated"], cl["grid"], cl["num_cluster"])
    G.check_frame(fx, g, cl, bx["boxes"])


@pytest.mark.parametrize("name", G.TRACKERS + G.TRACKERS_OT0)
def test_restatement_matches_golden_tracker(oracle, name):
    fx = G.load(name)
    T = oracle.Tracker(oracle.params(int(name in G.TRACKERS_OT0)))
    for f in range(len(fx["n_boxes"])):
        ts = 1.0e9 + f * float(fx["unit"])
        ego = T.ego_update(ts, *G.ego_of(fx, f))
        assert np.allclose(ego, fx["ego"][f], rtol=1e-12, atol=1e-12)
        out = T.step(fx["boxes"][f][: fx["n_boxes"][f]], ts)
        G.check_tracker_frame(fx, f, out, T.state, rtol=1e-7)
    T.close()


def _need_ref(oracle):
    if oracle.ref() is None:
        pytest.skip("oracle/_ref not built on this box")


@pytest.mark.parametrize("stream,frame,n", [(0, 0, 120000), (1, 3, 60000), (2, 1, 30000), (4, 0, 200000)])
def test_restatement_vs_ref_stateless_stages(oracle, synth, stream, frame, n):
    _need_ref(oracle)
    p = oracle.params(0)
    c = np.concatenate([synth.make_cloud(n, stream, frame), synth.edge_case_points()])
    g = oracle.ground_remove(p, c, want_dump=True)
    r = oracle.ref_ground_remove(c)
    assert np.array_equal(g["elevated"][:, :3], r["elevated"][:, :3]) and np.array_equal(g["ground"][:, :3], r["ground"][:, :3])
    rp = oracle.ref_ground_polar(c)
    for k in ("min_z", "height", "smoothed", "hdiff", "is_ground"):
        assert np.array_equal(g[k], rp[k]), k
    cl = oracle.cluster(p, g["elevated"]); rc = oracle.ref_cluster(g["elevated"])
    assert cl["num_cluster"] == rc["num_cluster"] and np.array_equal(cl["grid"], rc["grid"])
    bx = oracle.box_fit(p, g["elevated"], cl["grid"], cl["num_cluster"]); rb = oracle.ref_box_fit(g["elevated"], cl["grid"], cl["num_cluster"])
    assert bx["n_undefined"] == 0
    assert bx["boxes"].shape == rb["boxes"].shape and np.array_equal(bx["boxes"], rb["boxes"])


@pytest.mark.parametrize("stream,frame,n", [(0, 0, 120000), (3, 2, 40000), (6, 1, 9000)])
def test_side_products_vs_ref(oracle, synth, stream, frame, n):
    """makeClusteredCloud / setObsMsg / createCostMap: the restatement against the reference's own functions"""
    _need_ref(oracle)
    p = oracle.params(0)
    elev = oracle.ref_ground_remove(synth.make_cloud(n, stream, frame))["elevated"]
    elev = np.concatenate([elev, synth.edge_case_points()])   # ROI edges, the car footprint, huge coordinates
    cl = oracle.ref_cluster(elev)
    r = oracle.ref_cluster_products(elev, cl["grid"])
    o = oracle.cluster_products(p, elev, cl["grid"])
    assert len(r["clustered"]) > 100 and len(r["obstacles"]) > 10 and r["cost_map"].max() == 100
    for k in ("clustered", "obstacles", "cost_map"):
        assert r[k].shape == o[k].shape and np.array_equal(r[k], o[k]), k


@pytest.mark.parametrize("stream,frame,n", [(0, 0, 120000), (3, 1, 36000), (4, 1, 200000)])
def test_box_markers_restatement_vs_ref(oracle, synth, stream, frame, n):
    """the rviz cubes (mark_cluster, box_fitting.cpp:161-209): the float32 restatement the device is held against (sequential sums in
    input order, max - min) equals the MarkerArray the reference's own boxFitting fills, after the 0 -> 0.1 substitution of :192-199"""
    _need_ref(oracle)
    p = oracle.params(0)
    elev = oracle.ref_ground_remove(synth.make_cloud(n, stream, frame))["elevated"]
    cl = oracle.cluster(p, elev); bx = oracle.box_fit(p, elev, cl["grid"], cl["num_cluster"])
    rm = oracle.ref_box_markers(elev, cl["grid"], cl["num_cluster"])
    mine = oracle.box_markers_numpy(elev, cl["point_label"], bx["box_cluster"]).astype(np.float64)
    mine[:, 3:][mine[:, 3:] == 0] = 0.1
    assert len(rm) == len(bx["boxes"]) > 3 and np.array_equal(mine, rm)


@pytest.mark.parametrize("stream,frame,n", [(0, 0, 120000), (1, 3, 60000), (5, 2, 24000), (4, 0, 200000)])
def test_preset_ot0_vs_ref0(oracle, synth, stream, frame, n):
    """preset 1 (the KITTI-tuned constants and rules of object_tracking0) against that package's own sources"""
    if oracle.ref0() is None:
        pytest.skip("oracle/_ref/libmot_ref0.so not built on this box")
    p = oracle.params(1)
    cloud = np.concatenate([synth.make_cloud(n, stream, frame), synth.edge_case_points()])
    r = oracle.ref0_frame(cloud)
    g = oracle.ground_remove(p, cloud)
    assert np.array_equal(g["elevated"][:, :3], r["elevated"][:, :3]) and np.array_equal(g["ground"][:, :3], r["ground"][:, :3])
    cl = oracle.cluster(p, g["elevated"])
    assert cl["num_cluster"] == r["num_cluster"] and np.array_equal(cl["grid"], r["grid"])
    bx = oracle.box_fit(p, g["elevated"], cl["grid"], cl["num_cluster"])
    assert bx["boxes"].shape == r["boxes"].shape and np.array_equal(bx["boxes"], r["boxes"])
    assert r["num_cluster"] > 3


def test_side_products_golden(oracle):
    """the same, against the fixture generated from the reference (runs where oracle/_ref is absent)"""
    fx = G.load("side_ot_9k.npz")
    o = oracle.cluster_products(oracle.params(0), fx["elevated"], fx["grid"].astype(np.int32))
    for k in ("clustered", "obstacles", "cost_map"):
        assert np.array_equal(o[k], fx[k]), k


def test_restatement_vs_ref_cell_index(oracle):
    _need_ref(oracle)
    import ctypes as C
    p = oracle.params(0)
    rng = np.random.default_rng(0)
    xy = rng.uniform(-130, 130, size=(20000, 2)).astype(np.float32)
    k = np.arange(0, 81); ang = (k / 80.0) * 2 * np.pi - np.pi   # channel boundaries
    xy = np.concatenate([xy, np.stack([10 * np.cos(ang), 10 * np.sin(ang)], 1).astype(np.float32)])
    for x, y in xy:
        ch = C.c_int(0); b = C.c_int(0)
        oracle.orc().orc_cell_index(C.byref(p), C.c_float(x), C.c_float(y), C.byref(ch), C.byref(b))
        assert (ch.value, b.value) == oracle.ref_cell_index(float(x), float(y))


def test_lshape_rng_matches_libstdcxx(oracle):
    """mt19937_64(0) + uniform_int_distribution<>(0, n-1): restated generator vs libstdc++ (compiled here)"""
    import os, subprocess, tempfile
    src = r'''
#include <random>
#include <cstdio>
int main(){ int ns[]={1,2,6,7,30,31,100,1000,4097,65536,1000003};
 for(int n: ns){ std::mt19937_64 mt(0); std::uniform_int_distribution<> d(0,n-1); for(int i=0;i<80;i++) printf("%d ", d(mt)); printf("\n"); } }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "r.cpp"), "w").write(src)
        subprocess.run(["g++", "-O1", os.path.join(d, "r.cpp"), "-o", os.path.join(d, "r")], check=True)
        lines = subprocess.run([os.path.join(d, "r")], capture_output=True, text=True).stdout.strip().split("\n")
    for n, line in zip([1, 2, 6, 7, 30, 31, 100, 1000, 4097, 65536, 1000003], lines):
        assert np.array_equal(oracle.lshape_indices(n, 80), np.array(line.split(), np.int32)), n


def test_lshape_sampling_of_older_libstdcxx(oracle):
    """mot_params.rng_mapping = MOT_RNG_LIBSTDCXX10: uniform_int_distribution as GCC 5..10 ship it (every ROS1 toolchain), restated
    from bits/uniform_int_dist.h of libstdc++ 9 (no such library in this image: parity unpinned upstream). The test carries that
    operator()'s downscaling branch as a C++ program of its own over the real std::mt19937_64."""
    import os, subprocess, tempfile
    src = r'''
#include <random>
#include <cstdio>
#include <cstdint>
// libstdc++ <= 10, uniform_int_distribution<int>::operator()(urng, param), branch __urngrange > __urange
static int old_dist(std::mt19937_64& urng, int a, int b) {
  typedef uint64_t uctype;
  const uctype urngmin = urng.min(), urngmax = urng.max(), urngrange = urngmax - urngmin, urange = uctype(b) - uctype(a);
  uctype ret;
  const uctype uerange = urange + 1, scaling = urngrange / uerange, past = uerange * scaling;
  do ret = uctype(urng()) - urngmin; while (ret >= past);
  ret /= scaling;
  return int(ret + a);
}
int main(){ int ns[]={1,2,6,7,30,31,100,1000,4097,65536,1000003};
 for(int n: ns){ std::mt19937_64 mt(0); for(int i=0;i<80;i++) printf("%d ", old_dist(mt, 0, n-1)); printf("\n"); } }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "r.cpp"), "w").write(src)
        subprocess.run(["g++", "-O1", os.path.join(d, "r.cpp"), "-o", os.path.join(d, "r")], check=True)
        lines = subprocess.run([os.path.join(d, "r")], capture_output=True, text=True).stdout.strip().split("\n")
    differ = 0
    for n, line in zip([1, 2, 6, 7, 30, 31, 100, 1000, 4097, 65536, 1000003], lines):
        want = np.array(line.split(), np.int32)
        assert np.array_equal(oracle.lshape_indices_mapping(n, 80, 0), want), n
        differ += int(not np.array_equal(oracle.lshape_indices_mapping(n, 80, 1), want))
    # Both generations scale the draw proportionally — floor(g * n / 2^64) vs floor(g / floor((2^64 - 1) / n)) — and disagree only when
    # g * n / 2^64 lies within ~n^2 / 2^64 of an integer (5e-8 per draw at n = 1e6, 5e-14 at n = 1e3): on these sequences they coincide,
    # i.e. the L-shape boxes of a GCC <= 10 build of the reference equal those of this image's GCC 11 build except with that probability
    assert differ == 0


@pytest.mark.parametrize("unit", [1e5, 0.1])
def test_restatement_vs_ref_tracker(oracle, synth, unit):
    _need_ref(oracle)
    p = oracle.params(0)
    T = oracle.Tracker(p); R = oracle.RefTracker(); R.reset()
    for f in range(25):
        c = synth.make_cloud(40000, 2, f)
        g = oracle.ground_remove(p, c); cl = oracle.cluster(p, g["elevated"]); b = oracle.box_fit(p, g["elevated"], cl["grid"], cl["num_cluster"])["boxes"]
        ts = 5.0e8 + f * unit
        assert np.allclose(T.ego_update(ts, 4.0, -0.01 * f), R.ego_update(ts, 4.0, -0.01 * f), rtol=1e-12, atol=1e-12)
        a = T.step(b, ts); r = R.step(b, ts)
        assert a["n"] == r["n"] and np.array_equal(a["track_manage"], r["track_manage"])
        assert np.array_equal(a["is_static"], r["is_static"]) and np.array_equal(a["is_vis"], r["is_vis"])
        assert np.array_equal(a["vis_box"], r["vis_box"])
        for i in range(a["n"]):
            if r["track_manage"][i] == 0:
                continue
            sa, sr = T.state(i), R.state(i)
            assert sa["lifetime"] == sr["lifetime"]
            for k in ("x_merge", "x_cv", "x_ctrv", "x_rm", "p_merge", "p_cv", "p_ctrv", "p_rm", "mode_prob", "z_pred", "s", "k"):
                scale = max(np.abs(sr[k]).max(), 1e-300)
                assert np.abs(sa[k] - sr[k]).max() <= 1e-7 * scale + 1e-12, (f, i, k)
    T.close()


def test_tracker_ot0_vs_ref0(oracle, synth, tmp_path):
    """preset 1 of the restated tracker (distanceThres_ 0.25, lifeTimeThres_ 8, first-yaw offset 1.22191 - pi/2) against
    object_tracking0's own ukf.cpp / imm_ukf_jpda.cpp, which read the ego motion from text files"""
    _need_ref(oracle)
    p0, p1 = oracle.params(0), oracle.params(1)
    nf = 40
    # the package's own fixtures (ego motion of KITTI drive_0005, one value per frame: ego_velo.txt / ego_yaw.txt, kept in golden/)
    ego = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ego_drive0005.npz"))
    velo = ego["ego_v"][:nf]; yaw = ego["ego_yaw"][:nf]
    T = oracle.Tracker(p1); R = oracle.Ref0Tracker(); R.reset(tmp_path, velo, yaw)
    try:
        seen = 0
        for f in range(nf):
            c = synth.make_cloud(40000, 2, f)
            g = oracle.ground_remove(p0, c); cl = oracle.cluster(p0, g["elevated"]); b = oracle.box_fit(p0, g["elevated"], cl["grid"], cl["num_cluster"])["boxes"]
            ts = 5.0e8 + f * 1e5
            assert np.allclose(T.ego_update(ts, velo[f], yaw[f]), R.ego_update(ts), rtol=1e-12, atol=1e-12)
            a = T.step(b, ts); r = R.step(b, ts)
            assert a["n"] == r["n"] and np.array_equal(a["track_manage"], r["track_manage"])
            assert np.array_equal(a["is_static"], r["is_static"]) and np.array_equal(a["is_vis"], r["is_vis"])
            assert np.array_equal(a["vis_box"], r["vis_box"])
            seen = max(seen, int(a["is_vis"].sum()))
            for i in range(a["n"]):
                if r["track_manage"][i] == 0:
                    continue
                sa, sr = T.state(i), R.state(i)
                assert sa["lifetime"] == sr["lifetime"]
                for k in ("x_merge", "x_cv", "x_ctrv", "x_rm", "p_merge", "p_cv", "p_ctrv", "p_rm", "mode_prob", "z_pred", "s", "k"):
                    scale = max(np.abs(sr[k]).max(), 1e-300)
                    assert np.abs(sa[k] - sr[k]).max() <= 1e-7 * scale + 1e-12, (f, i, k)
        assert seen > 0   # the lifetime-8 / 0.25 m association path was exercised
    finally:
        R.close(); T.close()


@pytest.mark.parametrize("preset", [0, 1])
def test_restatement_vs_ref_tracker_random_sequences(oracle, preset, tmp_path):
    """the restated tracker against the reference's own tracker sources (object_tracking for preset 0, object_tracking0 for
    preset 1) on randomised box sequences: moving / stopping / vanishing objects, over-segmentation, crowded gates, clutter —
    the branches the synthetic scenes rarely reach"""
    _need_ref(oracle)
    import test_emu_tracker_random as RS
    p = oracle.params(preset)
    for seed in range(5000 * preset, 5000 * preset + 30 * RS.SCALE):
        seq = RS.sequence(seed) if seed % 6 else RS.hostile_sequence(seed)   # every sixth: degenerate measurements
        T = oracle.Tracker(p)
        if preset == 0:
            R = oracle.RefTracker(); R.reset()
        else:
            R = oracle.Ref0Tracker(); R.reset(tmp_path, [s[2] for s in seq], [s[3] for s in seq])
        try:
            for f, (boxes, ts, v, yaw) in enumerate(seq):
                ea = T.ego_update(ts, v, yaw); er = R.ego_update(ts, v, yaw) if preset == 0 else R.ego_update(ts)
                assert np.allclose(ea, er, rtol=1e-12, atol=1e-12)
                a = T.step(boxes, ts); r = R.step(boxes, ts)
                assert a["n"] == r["n"] and np.array_equal(a["track_manage"], r["track_manage"]), (seed, f)
                assert np.array_equal(a["is_static"], r["is_static"]) and np.array_equal(a["is_vis"], r["is_vis"]), (seed, f)
                assert np.array_equal(a["vis_box"], r["vis_box"]), (seed, f)
                for i in range(a["n"]):
                    if r["track_manage"][i] == 0:
                        continue
                    sa, sr = T.state(i), R.state(i)
                    assert sa["lifetime"] == sr["lifetime"]
                    if not RS.well_conditioned(sr):
                        continue
                    for k in ("x_merge", "p_merge", "mode_prob"):
                        scale = max(np.abs(sr[k]).max(), 1e-300)
                        assert np.abs(sa[k] - sr[k]).max() <= 1e-6 * scale + 1e-12, (seed, f, i, k)
        finally:
            T.close()
            if preset == 1:
                R.close()


def test_restatement_vs_ref_on_adversarial_clouds(oracle):
    """the stateless stages of the restatement against the reference's own sources on small hostile clouds (NaN / Inf /
    denormal / huge coordinates, ring and cell boundaries, duplicates, signed zeros). The cluster and box stages get finite
    points only — what a ground stage can emit; box fits in which the reference reads uninitialised memory (SURVEY.md H7,
    counted by the restatement) are skipped."""
    _need_ref(oracle)
    import test_emu_tracker_random as RS
    rng = np.random.default_rng(99)
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-40, -1e-40, 3.4, -3.4, 120.0, -120.0, 25.0, -25.0, 24.999998, -24.999998, 1e9,
                        3.4028235e38, 0.2, 0.1, 8.0, -5.0, 4.5, 2.0], np.float32)
    zs = np.array([np.nan, np.inf, -np.inf, -2.0, -0.4, -1.75, 0.1, 1000.0, -99.0, 0.0, -0.0], np.float32)
    p = oracle.params(0)

    def cloud():
        n = int(rng.integers(0, 150)); a = np.zeros((n, 4), np.float32)
        for col in (0, 1):
            pick = rng.random(n)
            a[:, col] = np.where(pick < 0.3, rng.choice(special, n), np.where(pick < 0.65, rng.uniform(-130, 130, n), rng.uniform(-30, 30, n))).astype(np.float32)
        a[:, 2] = np.where(rng.random(n) < 0.3, rng.choice(zs, n), rng.uniform(-4, 3, n)).astype(np.float32)
        return a

    boxes_checked = 0
    for it in range(300 * RS.SCALE):
        c = np.repeat(cloud(), int(rng.integers(1, 4)), axis=0)
        g = oracle.ground_remove(p, c); r = oracle.ref_ground_remove(c)
        assert np.array_equal(g["elevated"][:, :3].view(np.uint32), r["elevated"][:, :3].view(np.uint32)), it
        assert np.array_equal(g["ground"][:, :3].view(np.uint32), r["ground"][:, :3].view(np.uint32)), it
        e = np.repeat(cloud(), int(rng.integers(1, 40)), axis=0)
        e = e[np.isfinite(e[:, :3]).all(1)]
        o = oracle.cluster(p, e); rc = oracle.ref_cluster(e)
        assert o["num_cluster"] == rc["num_cluster"] and np.array_equal(o["grid"], rc["grid"]), it
        ob = oracle.box_fit(p, e, o["grid"], o["num_cluster"])
        if ob["n_undefined"] == 0:
            rb = oracle.ref_box_fit(e, o["grid"], o["num_cluster"])
            assert np.array_equal(ob["boxes"].view(np.uint32), rb["boxes"].view(np.uint32)), it
            boxes_checked += 1   # frames whose box stage was compared (most of these small clouds yield candidates that the size rules reject: also compared)
    assert boxes_checked > 50


def test_min_area_rect_properties(oracle):
    """the restated cv::minAreaRect is 'parity unpinned' (no OpenCV here): at least check what a minimum-area
    rectangle must satisfy — contains every point, area <= axis-aligned bounding box, duplicate invariance."""
    rng = np.random.default_rng(5)
    for trial in range(200):
        n = int(rng.integers(3, 60))
        pts = rng.integers(-200, 200, size=(n, 2)).astype(np.int32)
        if trial % 3 == 0:
            pts[:, 1] = pts[:, 0] // 2 + rng.integers(-3, 3, size=n)   # thin, slanted
        r = oracle.min_area_rect_points(pts).astype(np.float64)
        e0, e1 = r[1] - r[0], r[2] - r[1]
        area = abs(e0[0] * e1[1] - e0[1] * e1[0])
        aabb = float(np.ptp(pts[:, 0])) * float(np.ptp(pts[:, 1]))
        assert area <= aabb * (1 + 1e-4) + 1e-3
        # containment: project on the two edge directions
        for e, a, b in ((e0, r[0], r[1]), (e1, r[1], r[2])):
            L = np.linalg.norm(e)
            if L < 1e-9:
                continue
            t = (pts - a) @ (e / L)
            assert t.min() >= -1e-2 * max(L, 1) - 0.05 and t.max() <= L + 1e-2 * max(L, 1) + 0.05
        r2 = oracle.min_area_rect_points(np.concatenate([pts, pts[::2]]))
        assert np.array_equal(r2.astype(np.float32), oracle.min_area_rect_points(pts))


def test_min_area_rect_is_the_exact_minimum(oracle):
    """the restated cv::minAreaRect against the DEFINITION: for integer points the minimum-area enclosing rectangle has a
    side on a hull edge, and its area over every hull edge is computable exactly in rationals. The restatement's rectangle
    must have that area (to float32 rounding). This pins the function mathematically; OpenCV's own rounding and corner
    order stay unpinned (no OpenCV here)."""
    from fractions import Fraction

    def hull(pts):
        pts = sorted(set((int(x), int(y)) for x, y in pts))
        if len(pts) <= 2:
            return pts
        cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
        lo, up = [], []
        for q in pts:
            while len(lo) >= 2 and cross(lo[-2], lo[-1], q) <= 0: lo.pop()
            lo.append(q)
        for q in reversed(pts):
            while len(up) >= 2 and cross(up[-2], up[-1], q) <= 0: up.pop()
            up.append(q)
        return lo[:-1] + up[:-1]

    def exact_min_area(pts):
        h = hull(pts)
        if len(h) < 3:
            return Fraction(0)
        best = None
        for i in range(len(h)):
            a, b = h[i], h[(i + 1) % len(h)]
            ex, ey = b[0] - a[0], b[1] - a[1]
            us = [(q[0] - a[0]) * ex + (q[1] - a[1]) * ey for q in h]; vs = [-(q[0] - a[0]) * ey + (q[1] - a[1]) * ex for q in h]
            area = Fraction((max(us) - min(us)) * (max(vs) - min(vs)), ex * ex + ey * ey)
            best = area if best is None or area < best else best
        return best

    rng = np.random.default_rng(5)
    for trial in range(600):
        n = int(rng.integers(3, 60))
        pts = rng.integers(-200, 200, size=(n, 2)).astype(np.int32)
        if trial % 3 == 0:
            pts[:, 1] = pts[:, 0] // 2 + rng.integers(-3, 3, size=n)   # thin, slanted
        r = oracle.min_area_rect_points(pts).astype(np.float64)
        e0, e1 = r[1] - r[0], r[2] - r[1]
        area = abs(e0[0] * e1[1] - e0[1] * e1[0])
        exact = float(exact_min_area(pts))
        assert abs(area - exact) <= 1e-4 * max(exact, 1.0), (trial, area, exact)


def test_hull_column_reduction(oracle):
    """the device path feeds cv::convexHull only the lowest / highest pixel of every pixel column (already sorted);
    the restated OpenCV hull and min-area rectangle must be unchanged by that reduction"""
    rng = np.random.default_rng(1)

    def reduce_cols(pts):
        d = {}
        for x, y in pts:
            d[x] = (min(d[x][0], y), max(d[x][1], y)) if x in d else (y, y)
        out = []
        for x in sorted(d):
            lo, hi = d[x]
            out.append((x, lo))
            if hi != lo:
                out.append((x, hi))
        return np.array(out, np.int32)

    for trial in range(6000):
        n = int(rng.integers(1, 80)); mode = trial % 6
        if mode == 0: pts = rng.integers(-30, 30, size=(n, 2))
        elif mode == 1: pts = rng.integers(-5, 5, size=(n, 2))
        elif mode == 2:
            x = rng.integers(-40, 40, size=n); pts = np.stack([x, x // 2 + rng.integers(-2, 2, size=n)], 1)
        elif mode == 3:
            x = rng.integers(-40, 40, size=n); pts = np.stack([x, 3 * x + 7], 1)
        elif mode == 4: pts = np.stack([np.full(n, 5), rng.integers(-20, 20, size=n)], 1)
        else: pts = np.stack([rng.integers(-20, 20, size=n), np.full(n, -3)], 1)
        pts = pts.astype(np.int32)
        if trial % 2:
            pts = np.concatenate([pts, pts[rng.integers(0, n, size=n // 2 + 1)]])
        red = reduce_cols(pts)
        assert np.array_equal(oracle.convex_hull(pts), oracle.convex_hull(red))
        assert np.array_equal(oracle.min_area_rect_points(pts), oracle.min_area_rect_points(red))


def test_parallel_hull_construction(oracle):
    """cluster_rect_kernel builds cv::convexHull's output without the sequential Sklansky scans: the (x,y)-sorted point
    list is PEELED — every interior point that does not make a strict turn with its current neighbours is dropped, all
    at once, until nothing changes — once for the larger-y side and once for the smaller-y side, and the hull is emitted
    as [first point, larger-y side by increasing (x,y), last point, smaller-y side by decreasing (x,y)].
    The same construction in numpy must reproduce the restated OpenCV scan, degenerate inputs included."""
    rng = np.random.default_rng(5)

    def peel(pts, sign):
        idx = list(range(len(pts)))
        while True:
            rem = set()
            for k in range(1, len(idx) - 1):
                a, b, c = pts[idx[k - 1]], pts[idx[k]], pts[idx[k + 1]]
                cr = (b[0] - a[0]) * (c[1] - b[1]) - (b[1] - a[1]) * (c[0] - b[0])
                if sign * cr >= 0:
                    rem.add(k)
            if not rem:
                return idx
            idx = [v for k, v in enumerate(idx) if k not in rem]

    def peel_hull(pts):
        s = len(pts)
        if s <= 1:
            return pts[:s]
        up, lo = peel(pts, +1), peel(pts, -1)
        return pts[[0] + up[1:-1] + [s - 1] + lo[1:-1][::-1]]

    for trial in range(3200):
        n = int(rng.integers(1, 120)); mode = trial % 8
        if mode == 0: pts = rng.integers(-30, 30, size=(n, 2))
        elif mode == 1: pts = rng.integers(-4, 4, size=(n, 2))
        elif mode == 2:
            x = rng.integers(-100, 100, size=n); pts = np.stack([x, x // 2 + rng.integers(-2, 2, size=n)], 1)
        elif mode == 3:
            x = rng.integers(-40, 40, size=n); pts = np.stack([x, 3 * x + 7], 1)
        elif mode == 4: pts = np.stack([np.full(n, 5), rng.integers(-20, 20, size=n)], 1)
        elif mode == 5: pts = np.stack([rng.integers(-20, 20, size=n), np.full(n, -3)], 1)
        elif mode == 6:
            x = np.arange(n) - n // 2; pts = np.stack([x, (x * x) // 8], 1)
        else:
            x = np.arange(n) - n // 2; pts = np.stack([x, -(x * x) // 8 + rng.integers(0, 2, size=n)], 1)
        pts = np.unique(pts.astype(np.int64), axis=0)
        assert np.array_equal(oracle.convex_hull(pts.astype(np.int32)), peel_hull(pts))


@pytest.mark.parametrize("preset", [0, 1])
def test_ref_first_proxy(oracle, synth, preset):
    """the oracle the GPU suite uses (oracle_lib.RefFirst: the reference build first) against the restatement, on CPU: the mask it
    reconstructs from the reference's two clouds, the clouds with their 4th float, label grid, boxes, tracker outputs — and that a
    parameter set which is not a preset is answered by the restatement"""
    _need_ref(oracle)
    R = oracle.RefFirst(oracle)
    p = oracle.params(preset)
    for f in range(3):
        cloud = np.concatenate([synth.make_cloud(30000, 5 + preset, f)] + ([synth.edge_case_points()] if preset == 0 else [])).astype(np.float32)   # (under preset 1 the edge points make a cluster on which the reference reads uninitialised memory: that frame would go to the restatement)
        cloud[::7, 3] = 0.25                                  # the 4th float must come back as it went in
        a = R.ground_remove(p, cloud, want_dump=True); o = oracle.ground_remove(p, cloud, want_dump=True)
        assert np.array_equal(a["mask"], o["mask"])
        for k in ("elevated", "ground"):
            assert np.array_equal(a[k].view(np.uint32), o[k].view(np.uint32)), k
        for k in ("min_z", "height", "hground", "is_ground"):
            m = o["is_ground"].astype(bool) if k == "hground" else slice(None)
            assert np.array_equal(np.asarray(a[k])[m], np.asarray(o[k])[m]), k
        ca = R.cluster(p, a["elevated"]); co = oracle.cluster(p, o["elevated"])
        assert ca["num_cluster"] == co["num_cluster"] and np.array_equal(ca["grid"], co["grid"]) and np.array_equal(ca["point_label"], co["point_label"])
        ba = R.box_fit(p, a["elevated"], ca["grid"], ca["num_cluster"]); bo = oracle.box_fit(p, o["elevated"], co["grid"], co["num_cluster"])
        assert np.array_equal(ba["boxes"].view(np.uint32), bo["boxes"].view(np.uint32)) and np.array_equal(ba["box_cluster"], bo["box_cluster"])
    assert R.used.get(("ground_remove", "reference build" + (" (object_tracking0)" if preset else ""))) == 3
    assert any(k[0] == "box_fit" and k[1].startswith("reference build") for k in R.used) and any(k[0] == "cluster" and k[1].startswith("reference build") for k in R.used)
    q = oracle.params(preset, t_hdiff=0.07)
    R.ground_remove(q, cloud)
    assert ("ground_remove", "restatement (parameters are not a preset)") in R.used
    if preset == 0:   # two trackers at once: private copies of the reference library
        import test_emu_tracker_random as RS
        T1, T2, T0 = R.Tracker(p), R.Tracker(p), oracle.Tracker(p)
        assert isinstance(T1, oracle.RefTracker) and isinstance(T2, oracle.RefTracker) and T1._lib() is not T2._lib()
        for (b1, ts, v, yaw), (b2, _, _, _) in zip(RS.sequence(11), RS.sequence(12)):
            for T in (T1, T2, T0):
                T.ego_update(ts, v, yaw)
            o1, o2, o0 = T1.step(b1, ts), T2.step(b2, ts), T0.step(b1, ts)
            assert o1["n"] == o0["n"] and np.array_equal(o1["track_manage"], o0["track_manage"])
        assert o2["n"] != o1["n"] or not np.array_equal(o2["p"], o1["p"])     # the second instance really followed its own sequence
        T0.close()
