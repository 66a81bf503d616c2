"""MOT_ORDER_ANY (mot_set_point_order): the box stage on a cluster-ordered copy of the elevated points. Shared by tests/test_emu_point_order.py
(emulator) and tests/test_point_order_gpu.py (MI355X); generators and comparison helpers are those of tests/capacity_cases.py. Every case
first asserts with numpy and the oracle that its input is what it claims, then compares bit for bit against the oracle: boxes as uint32,
box_cluster, n_undefined, grid, point_label (input order), the cube markers, the side products (input order)."""
import numpy as np
import pytest

import capacity_cases as CC
from capacity_cases import MSG_CLUSTERS, MSG_GROUPS, oracle_frame, oracle_stage, refused, same_boxes, same_clusters, same_markers, same_tracks

OUT_LABELS = 4


def permuted(cloud, seed):
    return np.ascontiguousarray(cloud[np.random.default_rng(seed).permutation(len(cloud))])


def any_context(env, preset=0, **kw):
    c = env.context(preset, **kw)
    c.set_point_order(env.mot.MOT_ORDER_ANY)
    return c


def same_products(got, want, what):
    for k in ("clustered", "obstacles"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (what, k)
    assert np.array_equal(got["cost_map"], want["cost_map"]), what


def stagewise_exact(ctx, oracle, p, elev, o, what):
    """every stage-wise route that runs the box stage, and the getters behind it: everything equal to the oracle, per-point outputs in input order"""
    n = len(elev)
    cl = ctx.cluster(elev); same_clusters(cl, o["cl"], what)
    same_boxes(ctx.box_fit_resident(), o["bx"], (what, "resident")); same_markers(ctx.box_markers(0), o["markers"], (what, "resident"))
    if n:
        same_clusters(ctx.get_clusters(0, n_elevated=n), o["cl"], (what, "labels after the box stage"))
    same_boxes(ctx.get_boxes(0), o["bx"], (what, "get_boxes"))
    same_boxes(ctx.box_fit(elev, o["cl"]["grid"], o["cl"]["num_cluster"]), o["bx"], (what, "box_fit")); same_markers(ctx.box_markers(0), o["markers"], (what, "box_fit"))
    fr = ctx.cluster_node_frame(elev)
    assert fr["num_cluster"] == o["cl"]["num_cluster"], what
    same_boxes(fr, o["bx"], (what, "node frame")); same_markers(fr["cubes"], o["markers"], (what, "node frame"))
    same_products(fr, oracle.cluster_products(p, elev, o["cl"]["grid"]), (what, "node frame"))
    same_products(ctx.cluster_products(0), oracle.cluster_products(p, elev, o["cl"]["grid"]), (what, "products of the resident cloud"))
    if n:
        same_clusters(ctx.get_clusters(0, n_elevated=n), o["cl"], (what, "labels after the node frame"))


# ------------------------------------------------------------------------------------------------------------------ 1
def refused_today_exact_with_the_mode(env, oracle, max_points=8192):
    p = oracle.params(0)
    elev = permuted(CC.box_blob_cloud(200, 32), 7)
    o = oracle_stage(oracle, p, elev)
    groups = CC.group_count(o["cl"]["point_label"])
    print("groups of the permuted cloud:", groups, "boxes:", len(o["bx"]["boxes"]))
    assert groups > max_points // 2 and len(elev) <= max_points and len(o["bx"]["boxes"]) >= 1
    with env.context(0, max_points=max_points) as c:   # the default stays pinned
        c.cluster(elev)
        refused(env, c.box_fit_resident, MSG_GROUPS, "MOT_ORDER_SCAN")
        refused(env, lambda: c.cluster_node_frame(elev), MSG_GROUPS, "MOT_ORDER_SCAN, node frame")
    with any_context(env, 0, max_points=max_points) as c:
        stagewise_exact(c, oracle, p, elev, o, "MOT_ORDER_ANY")
        stagewise_exact(c, oracle, p, elev, o, "MOT_ORDER_ANY, again")


# ------------------------------------------------------------------------------------------------------------------ 2
def small_context_tiny_clusters(env, oracle):
    p = oracle.params(1)
    elev = CC.single_cell_cloud(4000)
    o = oracle_stage(oracle, p, elev)
    assert o["cl"]["num_cluster"] == 4000 and CC.group_count(o["cl"]["point_label"]) == 4000 > 4096 // 2 and len(o["bx"]["boxes"]) == 0
    with env.context(1, max_points=4096) as c:
        c.cluster(elev)
        refused(env, c.box_fit_resident, MSG_GROUPS, "MOT_ORDER_SCAN")
    with any_context(env, 1, max_points=4096) as c:
        stagewise_exact(c, oracle, p, elev, o, "4000 single-cell clusters, 4096-point context")
    beyond = CC.single_cell_cloud(CC.MAX_CLUSTERS + 1)
    ob = oracle_stage(oracle, p, beyond)
    assert ob["cl"]["num_cluster"] == CC.MAX_CLUSTERS + 1
    for order in (env.mot.MOT_ORDER_SCAN, env.mot.MOT_ORDER_ANY):   # the cluster limit is the same limit in both modes
        with env.context(1, max_points=8192) as c:
            c.set_point_order(order)
            same_clusters(c.cluster(beyond), ob["cl"], order)
            refused(env, c.box_fit_resident, MSG_CLUSTERS, (order, "resident"))
            refused(env, lambda: c.get_boxes(0), MSG_CLUSTERS, (order, "get_boxes"))
            refused(env, lambda: c.cluster_node_frame(beyond), MSG_CLUSTERS, (order, "node frame"))


# ------------------------------------------------------------------------------------------------------------------ 3
def fused_frames(oracle, p, max_points, step):
    """slot 0 a scene in order, slot 1 box-sized blobs in no order (more groups than MOT_ORDER_SCAN takes), slot 2 the tiled fragment construction"""
    frames = [CC.small_scene(step), permuted(CC.box_blob_cloud(160, 48, seed=20 + step), 30 + step), CC.tiled_fragment_cloud(max_points // 2 + 1, seed=step)]
    assert all(len(x) <= max_points for x in frames)
    return frames


def fused_path(env, oracle, outputs, graphs, max_points=8192):
    p = oracle.params(0)
    with any_context(env, 0, max_points=max_points, max_batch=3, max_tracks_total=2048) as c:
        c.set_fused_outputs(outputs)
        c.set_launch_graphs(graphs)
        run = CC.FusedRun(env, c, oracle, p, max_points)
        for step in range(3):
            frames = fused_frames(oracle, p, max_points, step)
            groups = [CC.group_count(oracle_frame(oracle, p, x)[1]["cl"]["point_label"]) for x in frames]
            print("step", step, "groups per slot:", groups, "boxes:", [len(oracle_frame(oracle, p, x)[1]["bx"]["boxes"]) for x in frames])
            assert groups[1] > max_points // 2, groups   # (on the oracle's ELEVATED cloud)
            run.launch(frames)
            for b in range(3):
                run.check_good(b, ("fused", outputs, graphs, step, b))   # ground / elevated clouds and labels in input order, boxes, cubes, tracks (no sticky refusal)
        for t in run.T:
            t.close()


def sequence_mode(env, oracle, max_points=8192):
    p = oracle.params(0)
    frames = fused_frames(oracle, p, max_points, 0)
    assert CC.group_count(oracle_frame(oracle, p, frames[1])[1]["cl"]["point_label"]) > max_points // 2
    with any_context(env, 0, max_points=max_points, max_batch=3, max_tracks_total=512) as c:
        host = np.zeros((3, max_points, 4), np.float32)
        for b, x in enumerate(frames):
            host[b, : len(x)] = x
        ptr, keep = env.upload(host)
        ts = [2.0e8 + k * 1e5 for k in range(3)]
        c.sequence_dev(ptr, max_points * 4, [len(x) for x in frames], ts, [1.0] * 3, [0.0] * 3)
        T = oracle.Tracker(p)
        for k in range(3):
            ego = T.ego_update(ts[k], 1.0, 0.0)
            g, o = oracle_frame(oracle, p, frames[k])
            same_boxes(c.get_boxes(k), o["bx"], ("sequence", k)); same_markers(c.box_markers(k), o["markers"], ("sequence", k))
            gb = o["bx"]["boxes"].astype(np.float64).copy(); co, si = np.cos(-ego[2]), np.sin(-ego[2])
            dx, dy = gb[..., 0] - ego[0], gb[..., 1] - ego[1]
            gb[..., 0] = co * dx - si * dy; gb[..., 1] = si * dx + co * dy
            ot = T.step(gb.astype(np.float32), ts[k])
        same_tracks(c.get_tracks(0), ot, "sequence")
        T.close()


# ------------------------------------------------------------------------------------------------------------------ 4
def stability_cloud(seed=5):
    """clusters of about 5000, 3000 and 40 points and 100 blobs, exact duplicates inside the two large ones, the whole cloud permuted: the large clusters
    cross several 2048-point sort chunks, equal slopes occur (the duplicates), and the float centroid sums, the L-shape draws and the slope tie-breaks
    all depend on the order inside a cluster"""
    rng = np.random.default_rng(seed)

    def slab(n, cx, cy, hx, hy):
        q = np.zeros((n, 4), np.float32)
        q[:, 0] = cx + rng.uniform(-hx, hx, n); q[:, 1] = cy + rng.uniform(-hy, hy, n); q[:, 2] = rng.uniform(-1.2, 0.3, n)
        return q
    big, mid, tiny = slab(5000, 10.0, 12.0, 2.0, 0.9), slab(3000, -10.0, -12.0, 1.8, 0.8), slab(40, 15.0, -15.0, 0.15, 0.15)
    for q, k in ((big, 300), (mid, 200)):   # exact duplicates: point j takes the coordinates of point i
        i, j = rng.integers(0, len(q), k), rng.integers(0, len(q), k)
        q[j] = q[i]
    blobs = CC.box_blob_cloud(100, 32, seed=9)
    return permuted(np.concatenate([big, mid, tiny, blobs]), seed + 1)


def stability(env, oracle):
    p = oracle.params(0)
    elev = stability_cloud()
    o = oracle_stage(oracle, p, elev)
    sizes = np.sort(np.bincount(o["cl"]["point_label"])[1:])[::-1]
    print("cluster sizes:", sizes[:4], "clusters:", o["cl"]["num_cluster"], "boxes:", len(o["bx"]["boxes"]))
    assert sizes[0] >= 4500 and 2500 <= sizes[1] <= 3500 and o["cl"]["num_cluster"] >= 100 and len(elev) <= 16384
    xy = elev[:, :2]
    assert len(np.unique(xy, axis=0)) <= len(xy) - 300, "no exact duplicates"
    big = np.nonzero(o["cl"]["point_label"] == np.argmax(np.bincount(o["cl"]["point_label"])[1:]) + 1)[0]
    assert big.max() - big.min() > 4 * 2048   # spread over the input, and > 2 chunks of its own once sorted
    assert len(o["bx"]["boxes"]) >= 50
    with any_context(env, 0, max_points=16384) as c:
        stagewise_exact(c, oracle, p, elev, o, "stability")


# ------------------------------------------------------------------------------------------------------------------ 5
def firing_order(cloud):
    """azimuth-major: the lasers of one firing together (a stable sort of a beam-major frame by azimuth)"""
    return np.ascontiguousarray(cloud[np.argsort(np.arctan2(cloud[:, 1], cloud[:, 0]), kind="stable")])


def fused_getters(env, c, cloud, max_points):
    host = np.zeros((1, max_points, 4), np.float32); host[0, : len(cloud)] = cloud
    ptr, keep = env.upload(host)
    c.frames_dev(ptr, max_points * 4, [len(cloud)])
    g = c.get_ground(0, n_hint=len(cloud))
    return dict(g=g, cl=c.get_clusters(0, n_elevated=g["n_elevated"]), bx=c.get_boxes(0), mk=c.box_markers(0), sd=c.cluster_products(0))


def same_answer_where_both_answer(env, oracle, synth, max_points=16384):
    p = oracle.params(0)
    beam = synth.make_cloud(16000, 1, 0)
    clouds = {"small_scene": CC.small_scene(0), "hdl64 beam-major": beam, "hdl64 firing order": firing_order(beam)}
    for name, cloud in clouds.items():
        g, o = oracle_frame(oracle, p, cloud)
        assert CC.group_count(o["cl"]["point_label"]) <= max_points // 2 and o["cl"]["num_cluster"] > 0, name
        res = {}
        for order, outputs in ((env.mot.MOT_ORDER_SCAN, 0), (env.mot.MOT_ORDER_ANY, 0), (env.mot.MOT_ORDER_ANY, OUT_LABELS)):
            with env.context(0, max_points=max_points) as c:
                c.set_point_order(order); c.set_fused_outputs(outputs)
                res[order, outputs] = fused_getters(env, c, cloud, max_points)
        for key, r in res.items():
            what = (name, key)
            assert np.array_equal(r["g"]["elevated"], g["elevated"]) and np.array_equal(r["g"]["ground"], g["ground"]), what
            same_clusters(r["cl"], o["cl"], what); same_boxes(r["bx"], o["bx"], what); same_markers(r["mk"], o["markers"], what)
            same_products(r["sd"], res[env.mot.MOT_ORDER_SCAN, 0]["sd"], what)
        same_products(res[env.mot.MOT_ORDER_SCAN, 0]["sd"], oracle.cluster_products(p, g["elevated"], o["cl"]["grid"]), name)


# ------------------------------------------------------------------------------------------------------------------ 6
EDGE_COUNTS = (0, 1, 63, 64, 65, 2047, 2048, 2049)


def sort_edges(env, oracle):
    p = oracle.params(0)
    full = permuted(CC.box_blob_cloud(80, 32, seed=3), 11)
    assert len(full) >= max(EDGE_COUNTS)
    rng = np.random.default_rng(2)
    outside = np.zeros((500, 4), np.float32); outside[:, 0] = rng.uniform(60, 90, 500); outside[:, 1] = rng.uniform(-90, 90, 500)
    one = np.zeros((3000, 4), np.float32); one[:, :2] = (5.0, 9.0) + rng.uniform(-1.0, 1.0, (3000, 2)); one[:, 2] = rng.uniform(-1.2, 0.2, 3000)
    with any_context(env, 0, max_points=8192) as c:
        for n in EDGE_COUNTS:
            elev = np.ascontiguousarray(full[:n])
            o = oracle_stage(oracle, p, elev)
            assert len(elev) == n
            stagewise_exact(c, oracle, p, elev, o, ("elevated points", n))
        o = oracle_stage(oracle, p, outside)
        assert o["cl"]["num_cluster"] == 0 and not o["cl"]["point_label"].any()
        stagewise_exact(c, oracle, p, outside, o, "all points outside the ROI")
        o = oracle_stage(oracle, p, one)
        assert o["cl"]["num_cluster"] == 1 and o["cl"]["point_label"].all()
        stagewise_exact(c, oracle, p, one, o, "all points in one cluster")
    p1 = oracle.params(1)
    at = CC.single_cell_cloud(CC.MAX_CLUSTERS)
    o = oracle_stage(oracle, p1, at)
    assert o["cl"]["num_cluster"] == CC.MAX_CLUSTERS
    with any_context(env, 1, max_points=4096) as c:
        stagewise_exact(c, oracle, p1, at, o, "exactly 4096 clusters")


# ------------------------------------------------------------------------------------------------------------------ 7
def switching(env, oracle, max_points=8192):
    p = oracle.params(0)
    frag = permuted(CC.box_blob_cloud(160, 48, seed=21), 31)
    good = CC.small_scene(2)
    (gf, of), (gg, og) = oracle_frame(oracle, p, frag), oracle_frame(oracle, p, good)
    assert CC.group_count(of["cl"]["point_label"]) > max_points // 2 >= CC.group_count(og["cl"]["point_label"])
    ANY, SCAN = env.mot.MOT_ORDER_ANY, env.mot.MOT_ORDER_SCAN

    def launch(c, cloud):
        host = np.zeros((1, max_points, 4), np.float32); host[0, : len(cloud)] = cloud
        ptr, keep = env.upload(host)
        c.frames_dev(ptr, max_points * 4, [len(cloud)])
        c.synchronize()
        return keep

    def good_frame(c, o, g, what):
        same_boxes(c.get_boxes(0), o["bx"], what); same_markers(c.box_markers(0), o["markers"], what)
        same_clusters(c.get_clusters(0, n_elevated=len(g["elevated"])), o["cl"], what)
    with env.context(0, max_points=max_points) as c:
        c.set_launch_graphs(True)
        c.set_point_order(ANY)
        k = launch(c, frag); good_frame(c, of, gf, "ANY, first")
        c.set_point_order(SCAN)
        good_frame(c, of, gf, "the resident ANY frame read after the switch")   # (its cubes come from the copy)
        k = launch(c, frag)
        refused(env, lambda: c.get_boxes(0), MSG_GROUPS, "SCAN refuses the same frame, message unchanged")
        k = launch(c, good); good_frame(c, og, gg, "SCAN, a frame it accepts")
        c.set_point_order(ANY)
        good_frame(c, og, gg, "the resident SCAN frame read after the switch")
        k = launch(c, frag); good_frame(c, of, gf, "ANY again")
        k = launch(c, good); good_frame(c, og, gg, "ANY, the ordinary frame")
        c.set_point_order(ANY)   # (no change: nothing happens)
        good_frame(c, og, gg, "ANY set twice")


# ------------------------------------------------------------------------------------------------------------------ 8
def interface(env):
    mot = env.mot
    lib = mot.load_library(env.lib_path)
    assert hasattr(lib, "mot_set_point_order") and "mot_set_point_order" in mot.EXPORTS
    assert (mot.MOT_ORDER_SCAN, mot.MOT_ORDER_ANY) == (0, 1)
    with env.context(0, max_points=4096) as c:
        for bad in (-1, 2, 7):
            with pytest.raises(mot.MotError) as e:
                c.set_point_order(bad)
            assert e.value.code == mot.MOT_E_ARG, bad
        c.set_point_order(mot.MOT_ORDER_ANY); c.set_point_order(mot.MOT_ORDER_SCAN)


# ------------------------------------------------------------------------------------------------------------------ mot_time_stage in the mode
def time_stage_in_the_mode(env, oracle, max_points=8192):
    """mot_time_stage of the regrouping kernels (35-37), of the box stage and its kernels and of the whole chain, several iterations each, in
    MOT_ORDER_ANY: every sequence leaves the slots as the batch left them (boxes, cubes and labels still the oracle's), and the ids are refused
    with MOT_E_STATE where the resident batch was not made in the current mode"""
    mot = env.mot
    p = oracle.params(0)
    frames = [permuted(CC.box_blob_cloud(160, 48, seed=21), 31), CC.small_scene(2)]
    ora = [oracle_frame(oracle, p, x) for x in frames]
    assert CC.group_count(ora[0][1]["cl"]["point_label"]) > max_points // 2

    def launch(c):
        host = np.zeros((2, max_points, 4), np.float32)
        for b, x in enumerate(frames):
            host[b, : len(x)] = x
        ptr, keep = env.upload(host)
        c.frames_dev(ptr, max_points * 4, [len(x) for x in frames])
        c.synchronize()
        return keep

    def intact(c, what):
        for b, (g, o) in enumerate(ora):
            same_boxes(c.get_boxes(b), o["bx"], (what, b)); same_markers(c.box_markers(b), o["markers"], (what, b))
            same_clusters(c.get_clusters(b, n_elevated=len(g["elevated"])), o["cl"], (what, b))

    def state_error(c, stage):
        with pytest.raises(mot.MotError) as e:
            c.time_stage(stage, 2, 1)
        assert e.value.code == mot.MOT_E_STATE, (stage, str(e.value))
    with any_context(env, 0, max_points=max_points, max_batch=2) as c:
        keep = launch(c)
        intact(c, "after the batch")
        # any order: none depends on what the one before left. (30, 34 and 31 time a kernel from the front of the box stage and, in either mode, close the
        # sequence with the finalize kernel alone: the slot's boxes are then not the batch's until a whole box stage has run again — 2 follows them)
        for stage in (36, 37, 35, 36, 2, 30, 2, 34, 2, 37, 31, 2, 36, 33, 32, 37, 100, 35):
            assert c.time_stage(stage, 2, 3) >= 0.0
            if stage not in (30, 34, 31):
                intact(c, ("after mot_time_stage", stage))
        c.set_point_order(mot.MOT_ORDER_SCAN)
        for stage in (35, 36, 37, 2, 100, 30, 31):   # the resident batch is the other mode's
            state_error(c, stage)
        intact(c, "after the refusals")
    with env.context(0, max_points=max_points, max_batch=2) as c:
        frames[0] = CC.small_scene(1); ora[0] = oracle_frame(oracle, p, frames[0])   # (a batch MOT_ORDER_SCAN accepts)
        keep = launch(c)
        assert c.time_stage(2, 2, 2) >= 0.0
        for stage in (35, 36, 37):   # exist in MOT_ORDER_ANY only
            state_error(c, stage)
        c.set_point_order(mot.MOT_ORDER_ANY)
        for stage in (2, 36, 30):
            state_error(c, stage)
        intact(c, "MOT_ORDER_SCAN batch")
