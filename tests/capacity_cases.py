"""Per-frame capacity edges of the cluster and box stage (the device flags kFlag* of csrc/mot_internal.h -> MOT_E_CAPACITY), shared by
tests/test_emu_capacity.py (emulator) and tests/test_capacity_gpu.py (MI355X). Every input is generated here from a fixed seed, and every
case asserts with numpy and the oracle, BEFORE it calls the library, that its input sits exactly on the edge it names:

  groups    E == max_points / 2 (bit-exact) and E == max_points / 2 + 1 (refused), E = distinct (i // 64, point_label[i]) over the labelled points
  clusters  4096 (bit-exact) and 4097 (refused) single-cell clusters, preset 1 (no dilation); preset 0 cannot get there: preset0_cluster_ceiling
  boxes     1024 (bit-exact) and 1025 (refused) accepted boxes, preset 0
  hull      not reachable: lattice_polygon_vertex_bound;  RNG draws: not reachable, ram_points 128 / 129 is the edge that exists: ram_points_edge

"At the limit" = boxes as uint32, box_cluster, n_undefined, grid, point_label and the cube markers against the oracle; "one beyond" = the flag's
own message. A frame beyond a limit must be REFUSED BY A KERNEL THAT STAYED IN BOUNDS: the CPU file runs these under the emulator's
AddressSanitizer build before anything here goes to a GPU (tests/README.md)."""
import ctypes as C

import numpy as np
import pytest

MSG_GROUPS = "cloud too fragmented: more than max_points/2 (tile, cluster) groups in a frame"
MSG_CLUSTERS = "more clusters in a frame than the library supports (4096)"
MSG_BOXES = "more boxes in a frame than the library supports (1024)"
MAX_CLUSTERS, MAX_BOXES = 4096, 1024


class Env:
    """where a case runs: the library (emulator or HIP), and how a host block becomes the pointer mot_frames_dev takes"""

    def __init__(self, mot, lib_path=None, upload=None):
        self.mot, self.lib_path = mot, lib_path
        self.upload = upload or (lambda host: (host.ctypes.data, host))   # emulator: "device" memory is host memory

    def params(self, preset, **kw):
        return self.mot.params(preset, lib=self.mot.load_library(self.lib_path), **kw)

    def context(self, preset=0, pkw=None, **kw):
        return self.mot.Context(self.params(preset, **(pkw or {})), lib_path=self.lib_path, **kw)


# ------------------------------------------------------------------------------------------------------------------ inputs
def lattice_cells(G, pitch, first):
    return [(x, y) for x in range(first, G - first, pitch) for y in range(first, G - first, pitch)]


def cell_centres(cells, G, roi):
    return (np.array(cells, np.float64).reshape(-1, 2) + 0.5) * (roi / G) - roi / 2


def group_count(point_label):
    """the (tile, cluster) groups of a frame as the label kernel forms them: a tile is 64 consecutive elevated points"""
    lab = np.asarray(point_label)
    i = np.nonzero(lab > 0)[0]
    return len(np.unique((i // 64).astype(np.int64) * 65536 + lab[i].astype(np.int64)))


def tiled_fragment_cloud(n_groups, seed=0):
    """preset 0. Isolated blobs on the pitch-5 lattice of the 250 x 250 grid (x, y within +-0.05 m of a cell centre, z in U(-1, 0.5)), ordered so
    that every 64-point tile holds 64 DIFFERENT blobs: point k belongs to blob (k // 64 % 8) * 64 + k % 64, so each point is a group of its own
    and E == n == n_groups. 512 blobs; a blob receives a point every eighth tile."""
    rng = np.random.default_rng(seed)
    cells = lattice_cells(250, 5, 2)[:512]
    ctr = cell_centres(cells, 250, 50.0)
    k = np.arange(n_groups)
    blob = (k // 64 % 8) * 64 + k % 64
    pts = np.zeros((n_groups, 4), np.float32)
    pts[:, :2] = ctr[blob] + rng.uniform(-0.05, 0.05, (n_groups, 2))
    pts[:, 2] = rng.uniform(-1.0, 0.5, n_groups)
    return pts


def permuted_blob_cloud(seed=0):
    """the cloud of the report that found the overflow crash: 1000 blobs of 8 points on the same lattice, the whole cloud permuted at random —
    nearly every point a group of its own (n = 8000)"""
    rng = np.random.default_rng(seed)
    ctr = cell_centres(lattice_cells(250, 5, 2)[:1000], 250, 50.0)
    pts = np.zeros((8000, 4), np.float32)
    pts[:, :2] = np.repeat(ctr, 8, 0) + rng.uniform(-0.05, 0.05, (8000, 2))
    pts[:, 2] = rng.uniform(-1.0, 0.5, 8000)
    return pts[rng.permutation(8000)]


def prefix_with(cloud, measure, target, lo=1):
    """the shortest prefix of `cloud` on which measure(prefix) == target (measure grows with the prefix, by one at a time near the target;
    the callers assert the result again on what they send)"""
    hi = len(cloud)
    assert measure(cloud[:hi]) >= target, "the cloud never reaches the target"
    while lo < hi:   # smallest n with measure >= target
        mid = (lo + hi) // 2
        if measure(cloud[:mid]) >= target:
            hi = mid
        else:
            lo = mid + 1
    for n in range(lo, min(lo + 64, len(cloud)) + 1):   # (a non-monotone step right at the target: look a little further)
        if measure(cloud[:n]) == target:
            return cloud[:n]
    raise AssertionError("no prefix sits on %d" % target)


def single_cell_cloud(n_cells, seed=0):
    """preset 1 (200 x 200 cells of 0.15 m, a cell with one point is occupied, no dilation): one point in every second cell of every second
    row = isolated single-cell clusters, in random order"""
    rng = np.random.default_rng(seed)
    cells = lattice_cells(200, 2, 0)
    assert len(cells) == 10000 >= n_cells
    ctr = cell_centres([cells[i] for i in rng.permutation(len(cells))[:n_cells]], 200, 30.0)
    pts = np.zeros((n_cells, 4), np.float32)
    pts[:, :2] = ctr + rng.uniform(-0.03, 0.03, (n_cells, 2))
    pts[:, 2] = rng.uniform(-0.9, 0.2, n_cells)
    return pts


def box_blob_cloud(n_blobs, per=32, seed=1):
    """preset 0: blobs of `per` points within +-0.25 m of every sixth cell (3 x 3 cells, 5 x 5 after the dilation, two free cells between
    neighbours), heights up to 0.3 m above the sensor plane: each passes ruleBasedFilter (the recipe was found with the oracle; the
    callers assert the count of accepted boxes). Blob after blob: few groups."""
    rng = np.random.default_rng(seed)
    cells = lattice_cells(250, 6, 3)
    assert len(cells) >= n_blobs
    ctr = cell_centres(cells[:n_blobs], 250, 50.0)
    pts = np.zeros((n_blobs * per, 4), np.float32)
    pts[:, :2] = np.repeat(ctr, per, 0) + rng.uniform(-0.25, 0.25, (n_blobs * per, 2))
    pts[:, 2] = rng.uniform(-1.0, 0.3, len(pts))
    return pts


def small_scene(seed, n_blobs=40):
    """a good frame for the neighbouring slots: a few dozen box-sized blobs, on the same cells whatever the seed — 48 points a blob, so that every blob
    is still a box after the ground stage has taken its quarter of the points, and a stream of these frames keeps its tracks alive"""
    return box_blob_cloud(n_blobs, 48, seed=100 + seed)


# ------------------------------------------------------------------------------------------------------------------ oracle side
def oracle_frame(oracle, p, cloud):
    """the whole stateless chain of the oracle on a raw frame"""
    g = oracle.ground_remove(p, cloud)
    return g, oracle_stage(oracle, p, g["elevated"])


def oracle_stage(oracle, p, elev):
    import oracle_lib as O
    cl = oracle.cluster(p, elev)
    if cl["num_cluster"] > MAX_CLUSTERS:   # (the oracle's box stage is not asked beyond the reference's own use; nothing compares with it there)
        return dict(cl=cl, bx=None, markers=None)
    bx = oracle.box_fit(p, elev, cl["grid"], cl["num_cluster"])
    return dict(cl=cl, bx=bx, markers=O.box_markers_numpy(elev, cl["point_label"], bx["box_cluster"]))


def same_boxes(got, want, what):
    assert got["n_undefined"] == want["n_undefined"], what
    assert np.array_equal(got["box_cluster"], want["box_cluster"]), what
    assert got["boxes"].shape == want["boxes"].shape and np.array_equal(got["boxes"].view(np.uint32), want["boxes"].view(np.uint32)), what


def same_clusters(got, want, what):
    assert got["num_cluster"] == want["num_cluster"], what
    assert np.array_equal(got["grid"], want["grid"]) and np.array_equal(got["point_label"], want["point_label"]), what


def same_markers(got, want, what):
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), what


def same_tracks(got, want, what):
    """a stream's tracks against the oracle tracker's: management states, lifetimes, positions (the suite's bar for tracker states)"""
    assert not got["capacity_exceeded"], what
    assert got["n"] == want["n"] and np.array_equal(got["track_manage"], want["track_manage"]), what
    live = np.asarray(want["track_manage"]) > 0
    assert np.array_equal(got["lifetime"][live], want["lifetime"][live]) and np.allclose(got["p"][live], want["p"][live], rtol=0, atol=1e-4), what


def refused(env, fn, msg, what):
    with pytest.raises(env.mot.MotError) as e:
        fn()
    assert e.value.code == env.mot.MOT_E_CAPACITY and msg in str(e.value), (what, str(e.value))


def kernel_group_count(ctx, slot, num_cluster):
    """the frame's groups as the label kernel counted them (per cluster, into the statistics) and the index kernel summed them: the start of
    the one-past-the-last cluster in the cluster-ordered group list (mot_debug_copy, which = 13)"""
    buf = np.zeros(MAX_CLUSTERS + 1, np.int32)
    rc = ctx.lib.mot_debug_copy(ctx._h, 13, slot, buf.ctypes.data_as(C.c_void_p), C.c_size_t(buf.nbytes))
    assert rc == 0
    return int(buf[num_cluster])


# ------------------------------------------------------------------------------------------------------------------ stage-wise routes
def stagewise_at_limit(ctx, oracle, p, elev, o, what):
    """mot_cluster + mot_box_fit_resident, mot_box_fit with a caller grid, mot_cluster_node_frame: everything bit-exact"""
    cl = ctx.cluster(elev); same_clusters(cl, o["cl"], what)
    same_boxes(ctx.box_fit_resident(), o["bx"], what); same_markers(ctx.box_markers(0), o["markers"], what)
    same_boxes(ctx.box_fit(elev, o["cl"]["grid"], o["cl"]["num_cluster"]), o["bx"], what); same_markers(ctx.box_markers(0), o["markers"], what)
    fr = ctx.cluster_node_frame(elev)
    assert fr["num_cluster"] == o["cl"]["num_cluster"], what
    same_boxes(fr, o["bx"], what); same_markers(fr["cubes"], o["markers"], what)


def stagewise_beyond(env, ctx, oracle, p, elev, o, msg, what):
    """every stage-wise route refuses with the flag's message — on the first call, the second and the fifth; a new cloud is judged on its own.
    (More than 4096 clusters: mot_box_fit_resident turns the frame down on the host, before a kernel runs, and leaves the refusal on slot 0 —
    the getters answer it exactly as they answer one a kernel raised.)"""
    cl = ctx.cluster(elev); same_clusters(cl, o["cl"], what)   # the cluster stage itself has no such limit
    for k in range(5):
        refused(env, ctx.box_fit_resident, msg, (what, "resident", k))
    for k in range(5):
        refused(env, lambda: ctx.get_boxes(0), msg, (what, "get_boxes", k))
        refused(env, lambda: ctx.box_markers(0), msg, (what, "markers", k))
        refused(env, lambda: ctx.get_clusters(0), msg, (what, "get_clusters", k))
        refused(env, lambda: ctx.cluster_products(0), msg, (what, "products", k))
    refused(env, lambda: ctx.box_fit(elev, o["cl"]["grid"], o["cl"]["num_cluster"]), msg, (what, "box_fit"))
    refused(env, lambda: ctx.cluster_node_frame(elev), msg, (what, "node frame"))
    refused(env, lambda: ctx.cluster_node_frame(elev), msg, (what, "node frame again"))


def groups_refused_first(env, oracle, max_points=8192):
    """The refused frame where nothing of an earlier frame stands in for what its kernels did not write: the FIRST frame of a fresh context
    in slot 0 (cluster starts, processing order and candidate records are as the allocation left them), and the frame after one with fewer
    clusters (the order and the records beyond that frame's clusters likewise) — through each stage-wise route and through the fused one.
    A per-cluster kernel that followed such a value would leave the slot's buffers: this is the case the AddressSanitizer run is for."""
    p = oracle.params(0)
    cap = max_points // 2
    beyond = tiled_fragment_cloud(cap + 1); o_beyond = oracle_stage(oracle, p, beyond)
    few = small_scene(3, 12); o_few = oracle_stage(oracle, p, few)
    good = small_scene(0); o_good = oracle_stage(oracle, p, good)
    assert group_count(o_beyond["cl"]["point_label"]) == cap + 1 and len(beyond) <= max_points
    assert 0 < o_few["cl"]["num_cluster"] < o_good["cl"]["num_cluster"] < o_beyond["cl"]["num_cluster"] and len(o_good["bx"]["boxes"]) > 10
    routes = {"resident": lambda c: (c.cluster(beyond), c.box_fit_resident()),
              "box_fit": lambda c: c.box_fit(beyond, o_beyond["cl"]["grid"], o_beyond["cl"]["num_cluster"]),
              "node frame": lambda c: c.cluster_node_frame(beyond)}
    for name, route in routes.items():
        for before in (None, few):
            what = ("refused first" if before is None else "refused after fewer clusters", name)
            with env.context(0, max_points=max_points) as c:
                if before is not None:
                    stagewise_at_limit(c, oracle, p, few, o_few, what)
                refused(env, lambda: route(c), MSG_GROUPS, what)
                for k in range(2):
                    refused(env, lambda: c.get_boxes(0), MSG_GROUPS, (what, "get_boxes", k))
                    refused(env, lambda: c.box_markers(0), MSG_GROUPS, (what, "markers", k))
                    refused(env, lambda: c.get_clusters(0), MSG_GROUPS, (what, "get_clusters", k))
                stagewise_at_limit(c, oracle, p, good, o_good, (what, "the next frame"))
    # fused: the refused frame in slot 0 of the context's first batch; then, on another context, behind a batch of small frames
    f_at, f_beyond = fused_edges(oracle, p, "groups", max_points)
    nc = lambda x: oracle_frame(oracle, p, x)[1]["cl"]["num_cluster"]
    assert 0 < nc(few) < nc(f_beyond)
    for before in (None, few):
        what = "fused, refused first" if before is None else "fused, refused after fewer clusters"
        with env.context(0, max_points=max_points, max_batch=3, max_tracks_total=2048) as c:
            run = FusedRun(env, c, oracle, p, max_points)
            if before is not None:
                run.launch([few, few, few])
                for b in range(3):
                    run.check_good(b, (what, "before", b))
            run.launch([f_beyond, good, f_beyond])
            run.check_refused(0, MSG_GROUPS, (what, 0)); run.check_refused(2, MSG_GROUPS, (what, 2))
            run.check_good(1, (what, "beside the refused frames"))
            run.launch([good, small_scene(1), small_scene(2)])
            for b in range(3):
                run.check_good(b, (what, "the next batch", b))
            for t in run.T:
                t.close()


def groups_stagewise(env, oracle, max_points, permuted):
    """E == group_cap exactly, then E == group_cap + 1, through the stage-wise calls (the index kernel's many-groups path: thousands of groups,
    hundreds of clusters per chunk). permuted: the reproduction cloud cut to the edge; otherwise the tiled construction."""
    p = oracle.params(0)
    cap = max_points // 2
    if permuted:
        full = permuted_blob_cloud()
        measure = lambda c: group_count(oracle.cluster(p, c)["point_label"])
        at, beyond = prefix_with(full, measure, cap, lo=cap), prefix_with(full, measure, cap + 1, lo=cap)
    else:
        at, beyond = tiled_fragment_cloud(cap), tiled_fragment_cloud(cap + 1)
    o_at, o_beyond = oracle_stage(oracle, p, at), oracle_stage(oracle, p, beyond)
    assert group_count(o_at["cl"]["point_label"]) == cap and group_count(o_beyond["cl"]["point_label"]) == cap + 1
    assert max(len(at), len(beyond)) <= max_points and o_at["cl"]["num_cluster"] > 256
    good = small_scene(0); o_good = oracle_stage(oracle, p, good)
    assert len(o_good["bx"]["boxes"]) > 10
    with env.context(0, max_points=max_points) as c:
        stagewise_at_limit(c, oracle, p, at, o_at, "E == cap")
        # the model of E against the label kernel's own count, on the frame at the limit and on an ordinary one
        c.cluster(at); c.box_fit_resident()
        assert kernel_group_count(c, 0, o_at["cl"]["num_cluster"]) == cap
        c.cluster(good); c.box_fit_resident()
        assert kernel_group_count(c, 0, o_good["cl"]["num_cluster"]) == group_count(o_good["cl"]["point_label"])
        stagewise_beyond(env, c, oracle, p, beyond, o_beyond, MSG_GROUPS, "E == cap + 1")
        # a refused frame that nobody read, then a good frame on the same slot
        c.cluster(beyond)
        refused(env, c.box_fit_resident, MSG_GROUPS, "unread")
        stagewise_at_limit(c, oracle, p, good, o_good, "after a refusal")
        stagewise_at_limit(c, oracle, p, at, o_at, "E == cap again")


def clusters_stagewise(env, oracle):
    p = oracle.params(1)
    at, beyond = single_cell_cloud(MAX_CLUSTERS), single_cell_cloud(MAX_CLUSTERS + 1)
    o_at, o_beyond = oracle_stage(oracle, p, at), oracle_stage(oracle, p, beyond)
    assert o_at["cl"]["num_cluster"] == MAX_CLUSTERS and o_beyond["cl"]["num_cluster"] == MAX_CLUSTERS + 1
    with env.context(1, max_points=16384) as c:
        stagewise_at_limit(c, oracle, p, at, o_at, "4096 clusters")
        stagewise_beyond(env, c, oracle, p, beyond, o_beyond, MSG_CLUSTERS, "4097 clusters")
        stagewise_at_limit(c, oracle, p, at, o_at, "4096 clusters after a refusal")


def boxes_stagewise(env, oracle):
    p = oracle.params(0)
    at, beyond = box_blob_cloud(MAX_BOXES), box_blob_cloud(MAX_BOXES + 1)
    o_at, o_beyond = oracle_stage(oracle, p, at), oracle_stage(oracle, p, beyond)
    assert len(o_at["bx"]["boxes"]) == MAX_BOXES and len(o_beyond["bx"]["boxes"]) == MAX_BOXES + 1
    with env.context(0, max_points=65536) as c:
        stagewise_at_limit(c, oracle, p, at, o_at, "1024 boxes")
        stagewise_beyond(env, c, oracle, p, beyond, o_beyond, MSG_BOXES, "1025 boxes")
        stagewise_at_limit(c, oracle, p, at, o_at, "1024 boxes after a refusal")


# ------------------------------------------------------------------------------------------------------------------ the fused route
def fused_edges(oracle, p, kind, max_points):
    """raw frames whose ELEVATED cloud (what the ground stage keeps: the oracle's ground_remove) sits on the edge / one beyond it"""
    if kind == "groups":
        full, target = permuted_blob_cloud(), max_points // 2
        measure = lambda c: group_count(oracle_frame(oracle, p, c)[1]["cl"]["point_label"])
        lo = target
    elif kind == "clusters":
        full, target = single_cell_cloud(4400), MAX_CLUSTERS
        measure = lambda c: oracle.cluster(p, oracle.ground_remove(p, c)["elevated"])["num_cluster"]
        lo = target
    else:
        full, target = box_blob_cloud(1300, 48), MAX_BOXES   # (the ground stage takes a quarter of the points: 48 a blob keep most blobs above min_points)
        measure = lambda c: len(oracle_frame(oracle, p, c)[1]["bx"]["boxes"])
        lo = 1
    at, beyond = prefix_with(full, measure, target, lo), prefix_with(full, measure, target + 1, lo)
    assert measure(at) == target and measure(beyond) == target + 1 and max(len(at), len(beyond)) <= max_points
    return at, beyond


class FusedRun:
    """three streams on one context, frame after frame through mot_frames_dev with the tracker on, next to oracle trackers of their own"""

    def __init__(self, env, ctx, oracle, p, stride):
        self.env, self.c, self.oracle, self.p, self.stride = env, ctx, oracle, p, stride
        self.T = [oracle.Tracker(p) for _ in range(3)]
        self.trusted = [True, True, True]   # the oracle tracker of a stream has seen every frame the library's has
        self.f = 0

    def launch(self, clouds):
        host = np.zeros((3, self.stride, 4), np.float32)
        for b, x in enumerate(clouds):
            host[b, : len(x)] = x
        self.ts = [2.0e8 + self.f * 1e5] * 3
        ptr, self.keep = self.env.upload(host)
        self.c.frames_dev(ptr, self.stride * 4, [len(x) for x in clouds], run_tracker=True, timestamps=self.ts, ego_v=[1.0] * 3, ego_yaw=[0.0] * 3)
        self.clouds = clouds
        self.f += 1

    def step_oracle_tracker(self, b, boxes):
        ego = self.T[b].ego_update(self.ts[b], 1.0, 0.0)
        co, si = np.cos(-ego[2]), np.sin(-ego[2])
        gb = boxes.astype(np.float64).copy()
        dx, dy = gb[..., 0] - ego[0], gb[..., 1] - ego[1]
        gb[..., 0] = co * dx - si * dy; gb[..., 1] = si * dx + co * dy
        return self.T[b].step(gb.astype(np.float32), self.ts[b])

    def check_good(self, b, what):
        """every output of slot b against the oracle run on that frame alone"""
        c, x = self.c, self.clouds[b]
        g, o = oracle_frame(self.oracle, self.p, x)
        r = c.get_ground(b, n_hint=len(x))
        assert np.array_equal(r["elevated"], g["elevated"]) and np.array_equal(r["ground"], g["ground"]) and np.array_equal(r["mask"][: len(x)], g["mask"]), what
        same_clusters(c.get_clusters(b, n_elevated=len(g["elevated"])), o["cl"], what)
        same_boxes(c.get_boxes(b), o["bx"], what)
        same_markers(c.box_markers(b), o["markers"], what)
        ot = self.step_oracle_tracker(b, o["bx"]["boxes"])
        a = c.get_tracks(b)
        if self.trusted[b]:
            same_tracks(a, ot, what)
        else:
            assert a["capacity_exceeded"], what   # sticky: the stream stepped on a refused frame earlier

    def check_refused(self, b, msg, what):
        c = self.c
        for k in (1, 2, 3, 4, 5):
            for name, fn in (("get_boxes", lambda: c.get_boxes(b)), ("get_clusters", lambda: c.get_clusters(b)), ("box_markers", lambda: c.box_markers(b)),
                             ("cluster_products", lambda: c.cluster_products(b)), ("get_ground", lambda: c.get_ground(b, want_clouds=False))):
                refused(self.env, fn, msg, (what, name, k))
        self.trusted[b] = False
        assert c.get_tracks(b)["capacity_exceeded"], what


def fused_contract(env, oracle, kind, graphs):
    """The overflowing frame in the MIDDLE slot of a three-slot fused batch with the tracker on.
    1 the frame at the limit: all three slots bit-exact, all three streams' tracks equal the oracle's;
    2 one beyond, read by nobody;  3 good frames on the same slots: every getter MOT_OK and bit-exact (no stale flag), the middle stream's
    tracks report the refusal (sticky), the other two equal the oracle's;  4 one beyond again: every getter of the middle slot refuses with the
    flag's message on calls 1 to 5, slots 0 and 2 are untouched."""
    preset, max_points, msg = {"groups": (0, 8192, MSG_GROUPS), "clusters": (1, 16384, MSG_CLUSTERS), "boxes": (0, 65536, MSG_BOXES)}[kind]
    p = oracle.params(preset)
    at, beyond = fused_edges(oracle, p, kind, max_points)
    good = [small_scene(s, 40) if preset == 0 else single_cell_cloud(300, seed=10 + s) for s in range(6)]
    if preset == 0:   # the neighbours' tracker comparison is about something: dozens of boxes a frame, through the ground stage
        assert all(len(oracle_frame(oracle, p, x)[1]["bx"]["boxes"]) > 30 for x in good)
    with env.context(preset, max_points=max_points, max_batch=3, max_tracks_total=2048) as c:
        c.set_launch_graphs(graphs)
        run = FusedRun(env, c, oracle, p, max_points)
        run.launch([good[0], at, good[1]])
        for b in range(3):
            run.check_good(b, (kind, "at the limit", b))
        run.launch([good[2], beyond, good[3]])   # nobody reads this batch
        for b in (0, 2):
            run.step_oracle_tracker(b, oracle_frame(oracle, p, run.clouds[b])[1]["bx"]["boxes"])
        run.trusted[1] = False
        run.launch([good[4], good[5], good[0]])
        for b in range(3):
            run.check_good(b, (kind, "after an unread refusal", b))
        run.launch([good[1], beyond, good[2]])
        run.check_refused(1, msg, (kind, "one beyond"))
        for b in (0, 2):
            run.check_good(b, (kind, "beside the refused frame", b))
        run.check_refused(1, msg, (kind, "one beyond, after the neighbours were read"))
        for t in run.T:
            t.close()


def sequence_refusal(env, oracle):
    """mot_sequence_dev (frames of ONE stream in slots 0 .. K-1): a refused frame in the middle makes the stream's mot_get_tracks report it;
    the frames beside it are delivered"""
    p = oracle.params(0)
    at, beyond = fused_edges(oracle, p, "groups", 8192)
    frames = [small_scene(0), beyond, small_scene(1)]
    with env.context(0, max_points=8192, max_batch=3, max_tracks_total=512) as c:
        host = np.zeros((3, 8192, 4), np.float32)
        for b, x in enumerate(frames):
            host[b, : len(x)] = x
        ptr, keep = env.upload(host)
        ts = [2.0e8 + k * 1e5 for k in range(3)]
        c.sequence_dev(ptr, 8192 * 4, [len(x) for x in frames], ts, [1.0] * 3, [0.0] * 3)
        assert c.get_tracks(0)["capacity_exceeded"]
        for b in (0, 2):
            same_boxes(c.get_boxes(b), oracle_frame(oracle, p, frames[b])[1]["bx"], ("sequence", b))
        refused(env, lambda: c.get_boxes(1), MSG_GROUPS, "sequence, refused frame")
        # without the refused frame the same stream reports nothing
        c.reset()
        frames[1] = at
        host[1] = 0; host[1, : len(at)] = at
        ptr, keep = env.upload(host)
        c.sequence_dev(ptr, 8192 * 4, [len(x) for x in frames], ts, [1.0] * 3, [0.0] * 3)
        T = oracle.Tracker(p)
        for k in range(3):
            ego = T.ego_update(ts[k], 1.0, 0.0)
            bx = oracle_frame(oracle, p, frames[k])[1]["bx"]
            same_boxes(c.get_boxes(k), bx, ("sequence at the limit", k))
            gb = bx["boxes"].astype(np.float64).copy(); co, si = np.cos(-ego[2]), np.sin(-ego[2])
            dx, dy = gb[..., 0] - ego[0], gb[..., 1] - ego[1]
            gb[..., 0] = co * dx - si * dy; gb[..., 1] = si * dx + co * dy
            ot = T.step(gb.astype(np.float32), ts[k])
        assert ot["n"] > 10   # (the comparison is about something)
        same_tracks(c.get_tracks(0), ot, "sequence at the limit")
        T.close()


# ------------------------------------------------------------------------------------------------------------------ limits no input reaches
def preset0_cluster_ceiling(oracle):
    """preset 0 dilates the occupancy 3 x 3: two occupied cells are separate components only from pitch 4 on, and a pitch-4 lattice of the
    250 x 250 grid has 63 x 63 = 3969 < 4097 cells — the cluster limit cannot be reached through mot_cluster with this preset"""
    p = oracle.params(0)
    rng = np.random.default_rng(0)

    def count(pitch):
        cells = lattice_cells(250, pitch, 0)
        ctr = cell_centres(cells, 250, 50.0)
        pts = np.zeros((2 * len(cells), 4), np.float32)
        pts[:, :2] = np.repeat(ctr, 2, 0) + rng.uniform(-0.05, 0.05, (2 * len(cells), 2)); pts[:, 2] = -0.5
        return len(cells), oracle.cluster(p, pts)["num_cluster"]
    assert count(4) == (63 * 63, 63 * 63) and 63 * 63 <= MAX_CLUSTERS
    assert count(3)[1] == 1   # one step denser and the dilated cells touch: everything is one component


def ram_points_edge(env, oracle):
    """the L-shape sampling draws ram_points indices out of 128 pre-generated raw draws: mot_create takes 1 .. 128"""
    with pytest.raises(env.mot.MotError):
        env.context(0, pkw=dict(ram_points=129), max_points=16384)
    with pytest.raises(env.mot.MotError):
        env.context(0, pkw=dict(ram_points=0), max_points=16384)
    p = oracle.params(0, ram_points=128)
    rng = np.random.default_rng(7)   # 64 car-sized blobs of 300 points in random order; those beside the sensor's lane (y > 8 m, y < -5 m) take the L-shape branch
    ctr = np.array([(-22 + 5.5 * (k % 8), -22 + 5.5 * (k // 8)) for k in range(64)])
    cloud = np.zeros((64 * 300, 4), np.float32)
    cloud[:, :2] = np.repeat(ctr, 300, 0) + rng.uniform(-1, 1, (len(cloud), 2)) * (0.9, 0.5)
    cloud[:, 2] = rng.uniform(-1.2, 0.3, len(cloud))
    cloud = cloud[rng.permutation(len(cloud))]
    o = oracle_stage(oracle, p, cloud)
    dbg = oracle.box_fit(p, cloud, o["cl"]["grid"], o["cl"]["num_cluster"], debug=True)["debug"]
    assert sum(1 for d in dbg if d["branch"] == 0 and d["accepted"]) >= 16, [(d["branch"], d["accepted"]) for d in dbg]   # L-shape clusters: the branch that samples
    with env.context(0, pkw=dict(ram_points=128), max_points=32768) as c:
        stagewise_at_limit(c, oracle, p, cloud, o, "ram_points 128")


def lattice_polygon_vertex_bound(span):
    """An upper bound on the vertices of a STRICTLY convex lattice polygon (no three consecutive vertices on a line) inside a box of
    span x span pixel steps: its edge vectors have pairwise different directions, so each is a positive multiple of a different primitive
    vector (gcd(|dx|, |dy|) == 1), and going round once sum|dx| <= 2 span, sum|dy| <= 2 span. Relaxed to sum(|dx| + |dy|) <= 4 span and
    every edge at its cheapest (the primitive vector itself), the most edges are had by taking primitive vectors cheapest first."""
    from math import gcd
    budget, edges, cost = 4 * span, 0, 1
    while True:
        k = sum(1 for dx in range(0, cost + 1) if gcd(dx, cost - dx) == 1 for sx in ((1, -1) if dx else (1,)) for sy in ((1, -1) if cost - dx else (1,)))
        if k * cost > budget:
            return edges + budget // cost
        edges += k; budget -= k * cost; cost += 1
