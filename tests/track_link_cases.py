"""Boxes and points linked to their tracks (mot_set_track_links): bodies shared by tests/test_emu_track_links.py (emulator) and
tests/test_track_links_gpu.py (MI355X). The callers supply a capacity_cases.Env (library + how a host block becomes a device pointer).

The expected owner row is a Python fp64 RESTATEMENT of the reference's matchingVec bookkeeping (imm_ukf_jpda.cpp:205-257, 806, 974-989) from the
oracle tracker's own state after the step — z_pred and s of every track, findMaxZandS, S x 4, the NIS of every box against gamma_g — walked in
track index order; only tracks whose lifetime grew in the step may own. A (track, box) pair with |nis - gamma| <= 1e-3 gamma is UNDECIDED (the
margin covers the 1e-4 state bar): a frame holding one is checked on births and claim counts only, and at most 2 % of a fixture's frames may be
set aside that way. The restatement validates itself: its claim count per track must equal the reference's lifetime increase."""
import os

import numpy as np

import capacity_cases as CC
import tracker_cases as TC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "track_boxes.npz")
STREAM_CLAIM_CAP = 256   # kStreamClaimCap of csrc/track.hip


# ------------------------------------------------------------------------------------------------------------------ the restatement
def box_centres(boxes):
    """getCpFromBbox (imm_ukf_jpda.cpp:465-479): fp32 products, then fp64"""
    b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 8, 3)
    f = np.float32
    p1x, p1y, p2x, p2y, p3x, p3y, p4x, p4y = (b[:, 0, 0], b[:, 0, 1], b[:, 1, 0], b[:, 1, 1], b[:, 2, 0], b[:, 2, 1], b[:, 3, 0], b[:, 3, 1])
    S1 = (((p4x - p2x) * (p1y - p2y) - (p4y - p2y) * (p1x - p2x)) / f(2)).astype(np.float64)
    S2 = (((p4x - p2x) * (p2y - p3y) - (p4y - p2y) * (p2x - p3x)) / f(2)).astype(np.float64)
    with np.errstate(all="ignore"):
        cx = p1x.astype(np.float64) + (p3x - p1x).astype(np.float64) * S1 / (S1 + S2)
        cy = p1y.astype(np.float64) + (p3y - p1y).astype(np.float64) * S1 / (S1 + S2)
    return np.stack([cx, cy], -1)


def restate_owners(state, pre, post, boxes, gamma, first_frame, seed_box_index):
    """-> (owner row, undecided, stats). pre / post: the oracle's outputs before / after the step (None before the first); state(i): its state after."""
    M = len(boxes)
    own = np.full(M, -1, np.int32)
    stats = dict(contested=0, second_init_lost=0, claims={})
    if first_frame:
        if M > seed_box_index:
            own[seed_box_index] = 0
        return own, False, stats
    n_before = pre["n"] if pre is not None else 0
    cp = box_centres(boxes)
    claimed = np.zeros(M, bool)
    undecided = False
    for i in range(n_before):
        grew = int(post["lifetime"][i]) - int(pre["lifetime"][i])
        if int(pre["track_manage"][i]) == 0 or M == 0:
            continue   # dead before the step (:826)
        s = state(i)
        S = np.asarray(s["s"], np.float64).reshape(3, 2, 2); z = np.asarray(s["z_pred"], np.float64).reshape(3, 2)
        det = [S[m, 0, 0] * S[m, 1, 1] - S[m, 0, 1] * S[m, 1, 0] for m in range(3)]
        mx = (0 if det[0] > det[2] else 2) if det[0] > det[1] else (1 if det[1] > det[2] else 2)   # findMaxZandS :176-203
        with np.errstate(all="ignore"):
            Si = np.linalg.inv(S[mx] * 4) if np.isfinite(S[mx]).all() and abs(det[mx]) > 0 else np.full((2, 2), np.nan)
            d = cp - z[mx]
            nis = np.einsum("ki,ij,kj->k", d, Si, d)
            gated = nis < gamma
        second = int(pre["track_manage"][i]) == 1
        marks = gated
        if second:   # second initialisation: only the progressive minima are marked (:238-245)
            marks = np.zeros(M, bool); smallest = 999.0
            for k in np.nonzero(gated)[0]:
                if nis[k] < smallest:
                    smallest = nis[k]; marks[k] = True
        if grew <= 0:
            # the track owns nothing: a guard skipped it (:828-851; z_pred and s are then the previous step's) or somebody claimed every box of its gate
            # before. The reference's state cannot tell the two apart, so such a track only COUNTS (the hand-made cases ask for these situations): a track
            # whose gate, on the state it has, holds boxes that were all claimed already
            if gated.any() and claimed[gated].all():
                stats["contested"] += int(gated.sum())
                stats["second_init_lost"] += int(second)
            continue
        if np.any(np.abs(nis - gamma) <= 1e-3 * gamma):
            undecided = True
        if second:
            g = nis[gated]
            if len(g) > 1 and np.min(np.abs(g[:, None] - g[None, :]) + np.eye(len(g))) <= 1e-3 * max(np.max(g), 1e-12):
                undecided = True   # two gated boxes at the same distance: which one is a minimum is not decided
            if marks.any() and claimed[np.nonzero(marks)[0][0]]:
                stats["second_init_lost"] += 1
        stats["contested"] += int((gated & claimed).sum())
        stats["claims"][i] = (int((gated & ~claimed).sum()), grew, int(pre["track_manage"][i]))
        mine = marks & ~claimed
        own[mine] = i
        claimed |= marks
    born = post["n"] - n_before   # births that found a slot (a dropped birth leaves its box without owner), in box order
    free = np.nonzero(~claimed)[0]
    own[free[:born]] = n_before + np.arange(min(born, len(free)))
    stats["unclaimed"] = len(free); stats["born"] = born
    return own, undecided, stats


def check_row(row, boxes, pre, post, state, dev_state, gamma, first_frame, seed_box_index, what):
    """(a) births, (b) claim counts, (c) identity unless the frame is undecided; -> (undecided, stats)"""
    want, undecided, st = restate_owners(state, pre, post, boxes, gamma, first_frame, seed_box_index)
    assert len(row) == len(boxes), (what, len(row), len(boxes))
    if first_frame:
        assert np.array_equal(row, want), (what, "first frame", row, want)
        return False, st
    n_before = pre["n"] if pre is not None else 0
    # the restatement against the reference itself: what it counts per track is the lifetime increase
    for i, (count, grew, tm) in st["claims"].items():
        if not undecided:
            assert count == grew, (what, "restatement != lifetime increase", i, count, grew)
    # (a) births: exactly the reference's, in box order, each newborn at its box
    births = np.nonzero(row >= n_before)[0]
    assert len(births) == st["born"] == post["n"] - n_before, (what, "births", len(births), st["born"])
    assert np.array_equal(row[births], n_before + np.arange(len(births))), (what, "births not in box order")
    cp = box_centres(boxes)
    for k in births:
        assert np.array_equal(np.asarray(dev_state(int(row[k]))["x_merge"][:2]), cp[k]), (what, "newborn not at its box", k)
    # (b) claim counts
    for i in range(n_before):
        tm, grew = int(pre["track_manage"][i]), int(post["lifetime"][i]) - int(pre["lifetime"][i])
        owned = int((row == i).sum())
        if tm >= 2:
            assert owned == grew, (what, "claims of track", i, owned, grew)
        else:
            assert owned <= max(grew, 0), (what, "claims of a second-init / dead track", i, owned, grew)
    # (c) identity
    if not undecided:
        assert np.array_equal(row, want), (what, "owners", np.nonzero(row != want)[0][:8], row[row != want][:8], want[row != want][:8])
    return undecided, st


# ------------------------------------------------------------------------------------------------------------------ 1: against the reference
def golden_streams(frames=40, names=("scene1_120k_unit100000_preset0", "scene7_200k_unit100000_preset0")):
    """the first 40 frames of two rendered streams. Chosen with the reference alone (reference_alone_within_margin, run again by every test): these two have
    no undecided frame; scene0 and scene1001 have one in 40 (2.5 %, beyond the 2 % the check allows) and are left out."""
    d = np.load(GOLDEN)
    for name in names:
        scene, points, unit, preset, F = d[name + "/meta"]
        off = np.concatenate([[0], np.cumsum(d[name + "/n_boxes"])])
        bx = d[name + "/boxes_global"]
        yield name, [(bx[off[f]:off[f + 1]], 1.0e9 + f * float(unit), float(d[name + "/ego_v"][f]), float(d[name + "/ego_yaw"][f])) for f in range(frames)]


def crossing_stream(frames=12, T=12, seed=11):
    """tracker_cases.grid_boxes at 2 m: neighbouring tracks share gated boxes (the cross-track matchingVec bookkeeping). Size and seed chosen
    with the reference alone: a dozen tracks over a dozen boxes put some pair within 1e-3 of the gate on most draws (16 tracks: every seed 1..8 has an
    undecided frame); this draw has none, 92 contested (track, box) pairs and 11 second-init tracks whose first minimum was already claimed."""
    rng = np.random.default_rng(seed)
    vel = rng.uniform(-1.0, 1.0, size=(1, T, 2))
    return "crossing lattice 2 m", [(TC.grid_boxes(1, T, f, vel, rng, 2.0)[0], 1.0e9 + f * 1.0e5, 0.0, 0.0) for f in range(frames)]


def reference_alone_within_margin(oracle, stream):
    """before anything else, with the reference alone: the fixture's undecided frames stay within 2 %"""
    name, frames = stream
    p = oracle.params(0)
    T = oracle.Tracker(p); pre = None; aside = 0
    for f, (boxes, ts, v, yaw) in enumerate(frames):
        T.ego_update(ts, v, yaw)
        post = T.step(boxes, ts)
        _, und, _ = restate_owners(T.state, pre, post, boxes, p.gamma_g, f == 0, p.seed_box_index)
        aside += und; pre = post
    T.close()
    assert aside <= 0.02 * len(frames), (name, aside, len(frames))
    return aside


def owners_against_reference(env, oracle, stream, mode):
    name, frames = stream
    p = oracle.params(0)
    reference_alone_within_margin(oracle, stream)
    T = oracle.Tracker(p)
    tot = dict(contested=0, second_init_lost=0, aside=0)
    with env.context(0, max_points=1024, max_tracks_total=1024) as c:
        c.set_tracker_mode(mode); c.set_track_links(True)
        pre = None
        for f, (boxes, ts, v, yaw) in enumerate(frames):
            c.ego_update(ts, v, yaw); T.ego_update(ts, v, yaw)
            a = c.track_step(boxes, ts); post = T.step(boxes, ts)
            assert a["n"] == post["n"] and np.array_equal(a["track_manage"], post["track_manage"]), (name, f)
            und, st = check_row(c.get_box_tracks(0), boxes, pre, post, T.state, c.track_state, p.gamma_g, f == 0, p.seed_box_index, (name, mode, f))
            tot["aside"] += und; tot["contested"] += st["contested"]; tot["second_init_lost"] += st["second_init_lost"]
            pre = post
    T.close()
    assert tot["aside"] <= 0.02 * len(frames), (name, tot)
    print(name, "mode", mode, tot)
    return tot


# ------------------------------------------------------------------------------------------------------------------ 2: edges of the owner row
def lattice(n, spacing=9.0, shift=(0.0, 0.0), first=0):
    """n small boxes on a lattice far from the seed position, numbered from `first` on (the same number = the same place)"""
    import test_emu_tracker_random as TR
    k = np.arange(first, first + n)
    return np.array([TR.box(40.0 + (i % 20) * spacing + shift[0], 40.0 + (i // 20) * spacing + shift[1], 0.8, 1.2, 0.0, -0.4) for i in k], np.float32).reshape(-1, 8, 3)


def edge_scripts():
    """name -> (track slots, [box list per frame]). M = 0, 1, 64, 65, 130 on the first and on later frames; live tracks at and just above
    kStreamClaimCap when a frame of <= 64 boxes arrives; births dropped for want of slots."""
    s = {}
    s["sizes"] = (1024, [lattice(130), lattice(130), lattice(65), lattice(64), lattice(1), lattice(0), lattice(130, shift=(0.2, 0.1)), lattice(64)])
    for m in (0, 1, 64, 65):
        s["first frame of %d" % m] = (256, [lattice(m), lattice(m), lattice(m)])
    s["live tracks at the claim cap"] = (1024, [lattice(2), lattice(STREAM_CLAIM_CAP), lattice(64), lattice(40)])
    s["live tracks above the claim cap"] = (1024, [lattice(2), lattice(STREAM_CLAIM_CAP + 1), lattice(64), lattice(40)])
    s["dropped births"] = (4, [lattice(3), lattice(10), lattice(10), lattice(12)])
    return s


def contested_script(frames=10):
    """two gates over the same boxes (the lower id wins), and a second-init track whose first gated box is already claimed: an established track A at the
    origin of the scene; a box appears 3 m beside it for one frame (track B is born); from then on two boxes, both inside A's gate, the first of them
    nearer to A — A (lower id) claims both, B's progressive minima are claimed already"""
    import test_emu_tracker_random as TR
    out = []
    for f in range(frames):
        bx = [TR.box(30.0, 30.0, 0.8, 1.2, 0.0, -0.4), TR.box(60.0, 60.0, 0.8, 1.2, 0.0, -0.4)]
        if f == 5:
            bx.append(TR.box(33.0, 30.0, 0.8, 1.2, 0.0, -0.4))
        if f >= 6:
            bx = [TR.box(30.2, 30.0, 0.8, 1.2, 0.0, -0.4), TR.box(31.0, 30.0, 0.8, 1.2, 0.0, -0.4), bx[1]]
        out.append(np.array(bx, np.float32).reshape(-1, 8, 3))
    return out


def run_script(env, oracle, T_slots, script, mode):
    """-> the owner row of every frame; every row is checked against the restatement on the oracle tracker (unless births are dropped: then the oracle,
    which never runs out of slots, is left out and the row's own invariants are checked)"""
    p = oracle.params(0)
    rows, tot = [], dict(contested=0, second_init_lost=0)
    dropping = T_slots < 16
    T = None if dropping else oracle.Tracker(p)
    with env.context(0, max_points=1024, max_tracks_total=T_slots) as c:
        c.set_tracker_mode(mode); c.set_track_links(True)
        pre = None; n_before = 0
        for f, boxes in enumerate(script):
            ts = 1.0e9 + f * 1.0e5
            c.ego_update(ts, 0.0, 0.0)
            a = c.track_step(boxes, ts)
            row = c.get_box_tracks(0)
            assert len(row) == len(boxes), (f, len(row))
            if T is not None:
                T.ego_update(ts, 0.0, 0.0); post = T.step(boxes, ts)
                und, st = check_row(row, boxes, pre, post, T.state, c.track_state, p.gamma_g, f == 0, p.seed_box_index, (mode, f))
                assert not und, (mode, f, "a hand-made frame must be decided")
                tot["contested"] += st["contested"]; tot["second_init_lost"] += st["second_init_lost"]
                pre = post
            else:
                births = row[row >= n_before]
                assert np.array_equal(births, n_before + np.arange(len(births))) and len(births) == a["n"] - n_before, (f, row)
            n_before = a["n"]
            rows.append(row)
        last = a
    if T is not None:
        T.close()
    return rows, tot, last


def owner_edges(env, oracle, name):
    T_slots, script = edge_scripts()[name]
    res = {mode: run_script(env, oracle, T_slots, script, mode) for mode in (env.mot.MOT_TRACKER_SPLIT, env.mot.MOT_TRACKER_STREAM)}
    (ra, _, la), (rb, _, _) = res[env.mot.MOT_TRACKER_SPLIT], res[env.mot.MOT_TRACKER_STREAM]
    assert len(ra) == len(rb) and all(np.array_equal(x, y) for x, y in zip(ra, rb)), (name, "SPLIT and STREAM rows differ")
    if name == "dropped births":
        assert la["capacity_exceeded"] and any((r == -1).any() for r in ra[1:]), (name, "no birth was dropped")
    if name.startswith("live tracks"):
        want = STREAM_CLAIM_CAP + (1 if "above" in name else 0)
        assert (ra[1] >= 0).sum() == want and len(np.unique(ra[2])) == 64, (name, "the frame of 64 boxes did not meet %d live tracks" % want)
    return ra


def contested(env, oracle):
    script = contested_script()
    res = {mode: run_script(env, oracle, 256, script, mode) for mode in (env.mot.MOT_TRACKER_SPLIT, env.mot.MOT_TRACKER_STREAM)}
    (ra, ta, _), (rb, _, _) = res[env.mot.MOT_TRACKER_SPLIT], res[env.mot.MOT_TRACKER_STREAM]
    assert all(np.array_equal(x, y) for x, y in zip(ra, rb))
    assert ta["contested"] >= 1 and ta["second_init_lost"] >= 1, ta
    # frame 6: both boxes near A belong to A (the lower id), although track B (born in frame 5 from the box beside A) gates them too
    a_id = ra[5][0]
    assert a_id >= 0 and ra[6][0] == a_id and ra[6][1] == a_id and ra[5][2] > a_id, (ra[5], ra[6])


def batch_of_three(env, oracle):
    """mot_track_steps_dev over three slots with different box counts, one of them empty; SPLIT == STREAM, every row against the restatement"""
    p = oracle.params(0)
    scripts = [[lattice(5), lattice(5), lattice(6)], [lattice(0), lattice(0), lattice(0)], [lattice(70), lattice(70), lattice(66)]]
    rows = {}
    for mode in (env.mot.MOT_TRACKER_SPLIT, env.mot.MOT_TRACKER_STREAM):
        Ts = [oracle.Tracker(p) for _ in range(3)]; pre = [None] * 3
        with env.context(0, max_points=1024, max_batch=3, max_tracks_total=256) as c:
            c.set_tracker_mode(mode); c.set_track_links(True)
            for f in range(3):
                ts = 1.0e9 + f * 1.0e5
                host = np.zeros((3, 70 * 24), np.float32)
                for b in range(3):
                    host[b, : scripts[b][f].size] = scripts[b][f].ravel()
                    c.ego_update(ts, 0.0, 0.0, b); Ts[b].ego_update(ts, 0.0, 0.0)
                ptr, keep = env.upload(host)
                c.track_steps_dev(ptr, 70 * 24, [len(scripts[b][f]) for b in range(3)], [ts] * 3)
                for b in range(3):
                    row = c.get_box_tracks(b); post = Ts[b].step(scripts[b][f], ts)
                    und, _ = check_row(row, scripts[b][f], pre[b], post, Ts[b].state, lambda i, b=b: c.track_state(i, slot=b), p.gamma_g, f == 0, p.seed_box_index, (mode, f, b))
                    assert not und
                    pre[b] = post; rows[mode, f, b] = row
                with np.testing.assert_raises(env.mot.MotError):   # the tracker was fed from outside: no point chain
                    c.get_point_tracks(0)
        for t in Ts:
            t.close()
    for f in range(3):
        for b in range(3):
            assert np.array_equal(rows[env.mot.MOT_TRACKER_SPLIT, f, b], rows[env.mot.MOT_TRACKER_STREAM, f, b]), (f, b)
    assert len(rows[env.mot.MOT_TRACKER_SPLIT, 2, 1]) == 0 and len(rows[env.mot.MOT_TRACKER_SPLIT, 2, 2]) == 66


# ------------------------------------------------------------------------------------------------------------------ 3: point ids
NE_SHAPES = (0, 1, 63, 64, 65, 2047, 2048, 2049, 5000)


def link_frame_source(seed=0):
    """preset 0, in this order: a cluster of 4 points (under min_points), a blob of 32 points whose top lies 3.2 m above the ground (a cluster the rule-based
    filter rejects: t_height_max 2.6), three points outside the region of interest (no cluster), then box-sized blobs of 48 points. Every z lies above
    -0.3: groundRemove keeps every point, so a prefix of n points is a frame of exactly n elevated points (asserted by frame_with_elevated)."""
    rng = np.random.default_rng(50 + seed)
    def pts(xy, z):
        q = np.zeros((len(xy), 4), np.float32); q[:, :2] = xy; q[:, 2] = z; return q
    small = pts(np.array([-20.0, -20.0]) + rng.uniform(-0.05, 0.05, (4, 2)), rng.uniform(-0.3, 0.2, 4))
    tall = pts(np.array([-15.0, 15.0]) + rng.uniform(-0.25, 0.25, (32, 2)), rng.uniform(0.7, 1.2, 32))
    outside = pts(np.array([[40.0, 3.0], [-33.0, 8.0], [3.0, 41.0]]), np.array([0.0, 0.1, -0.2]))
    blobs = CC.box_blob_cloud(160, 48, seed=60 + seed)
    blobs[:, 2] = rng.uniform(-0.3, 0.3, len(blobs))
    return np.concatenate([small, tall, outside, blobs])


def frame_with_elevated(oracle, p, target, seed=0):
    x = np.ascontiguousarray(link_frame_source(seed)[:target])
    assert len(x) == target and len(oracle.ground_remove(p, x)["elevated"]) == target
    return x


def download(keep, like):
    """what Env.upload handed back, read again: the emulator's "device" block is the host array itself"""
    return keep.to_host(like.dtype, like.shape) if hasattr(keep, "to_host") else np.asarray(keep).reshape(like.shape)


def compose(point_label, box_cluster, box_track):
    tab = np.full(max(int(point_label.max(initial=0)), int(box_cluster.max(initial=0))) + 1, -1, np.int32)
    tab[box_cluster] = box_track
    tab[0] = -1
    return tab[point_label]


def read_links(c, b, n_points):
    bt = c.get_box_tracks(b); bx = c.get_boxes(b)
    ids = c.get_point_tracks(b)
    cl = c.get_clusters(b, n_elevated=max(len(ids), 1))
    lab = cl["point_label"][: len(ids)]
    assert len(bt) == len(bx["box_cluster"])
    return dict(ids=ids, label=lab, box_cluster=bx["box_cluster"], box_track=bt, want=compose(lab, bx["box_cluster"], bt) if len(ids) else np.zeros(0, np.int32))


def launch(env, c, clouds, stride, f, ego_v=1.0):
    host = np.zeros((len(clouds), stride, 4), np.float32)
    for b, x in enumerate(clouds):
        host[b, : len(x)] = x
    ptr, keep = env.upload(host)
    c.frames_dev(ptr, stride * 4, [len(x) for x in clouds], run_tracker=True, timestamps=[2.0e8 + f * 1e5] * len(clouds), ego_v=[ego_v] * len(clouds), ego_yaw=[0.0] * len(clouds))
    return keep


def point_ids(env, oracle, targets, graphs=False, order_any=False, max_points=8192):
    """frames whose elevated count is exactly each of `targets`, three frames of the same stream each (so that owners are claims, not only births): the ids
    equal the numpy composition of the three getters bit for bit; the device export equals the getter"""
    p = oracle.params(0)
    B = len(targets)
    frames = [[frame_with_elevated(oracle, p, t, seed=s) for t in targets] for s in range(3)]
    out = []
    with env.context(0, max_points=max_points, max_batch=B, max_tracks_total=512) as c:
        c.set_launch_graphs(graphs); c.set_track_links(True)
        if order_any:
            c.set_point_order(env.mot.MOT_ORDER_ANY)
        for f in range(3):
            clouds = frames[f]
            perms = [np.random.default_rng(7 + b).permutation(len(x)) for b, x in enumerate(clouds)]
            sent = [np.ascontiguousarray(x[q]) for x, q in zip(clouds, perms)] if order_any else clouds
            keep = launch(env, c, sent, max_points, f)
            got = []
            for b in range(B):
                r = read_links(c, b, len(sent[b]))
                assert len(r["ids"]) == targets[b], (targets[b], len(r["ids"]))
                assert np.array_equal(r["ids"], r["want"]), (f, targets[b], "ids != composition of the getters")
                if f == 2 and targets[b] >= 63 and not order_any:
                    counts = np.bincount(r["label"], minlength=2)
                    small = [l for l in range(1, len(counts)) if 0 < counts[l] < p.min_points]
                    rejected = [l for l in range(1, len(counts)) if counts[l] >= p.min_points and l not in set(r["box_cluster"].tolist())]
                    assert small and rejected and (r["label"] == 0).any(), (targets[b], "the frame lacks a small / a rejected cluster / unclustered points", small, rejected)
                    for l in small + rejected:
                        assert (r["ids"][r["label"] == l] == -1).all()
                    assert (r["ids"][r["label"] == 0] == -1).all()
                    if targets[b] >= 2047:
                        assert (r["ids"] >= 0).sum() > targets[b] // 2
                r["perm"] = perms[b]; got.append(r)
            # the device export against the host getter
            stride = max(max(targets), 1) + 3   # (an odd stride: slots that do not start on 16 bytes take the scalar stores)
            for st in (stride, (stride + 3) & ~3):
                dev = np.full((B, st), -7, np.int32); cnt = np.full(B, -7, np.int32)
                pd, kd = env.upload(dev); pc, kc = env.upload(cnt)
                c.export_point_tracks_dev(B, pd, st, pc); c.synchronize()
                dev, cnt = download(kd, dev), download(kc, cnt)
                for b in range(B):
                    assert cnt[b] == targets[b] and np.array_equal(dev[b, : targets[b]], got[b]["ids"]) and (dev[b, targets[b]:] == -7).all(), (f, b, st)
            out.append(got)
    return out


def order_any_equals_scan(env, oracle, targets=(65, 2049)):
    scan = point_ids(env, oracle, targets)
    anyo = point_ids(env, oracle, targets, order_any=True)
    for f in range(3):
        for b in range(len(targets)):
            q = anyo[f][b]["perm"]
            assert np.array_equal(anyo[f][b]["ids"], scan[f][b]["ids"][q]), (f, targets[b], "MOT_ORDER_ANY on a shuffled copy != SCAN's ids under the permutation")


def graphs_equal_plain(env, oracle, targets=(64, 2048)):
    a = point_ids(env, oracle, targets, graphs=False); b = point_ids(env, oracle, targets, graphs=True)
    for f in range(3):
        for k in range(len(targets)):
            assert np.array_equal(a[f][k]["ids"], b[f][k]["ids"]) and np.array_equal(a[f][k]["box_track"], b[f][k]["box_track"])


def persistence(env, oracle, sequence=False):
    """two blobs moving 0.3 m a frame for five frames: in frames 3 and 4 the id that owns most of each blob's points is the same, and confirmed"""
    rng = np.random.default_rng(3)
    def blob(cx, cy):
        q = np.zeros((200, 4), np.float32); q[:, 0] = cx + rng.uniform(-0.4, 0.4, 200); q[:, 1] = cy + rng.uniform(-0.4, 0.4, 200); q[:, 2] = rng.uniform(-1.0, 0.3, 200); return q
    frames = [np.concatenate([blob(8.0 + 0.3 * f, 5.0), blob(-9.0, -6.0 - 0.3 * f)]) for f in range(5)]
    major = []
    with env.context(0, max_points=2048, max_batch=5 if sequence else 1, max_tracks_total=256) as c:
        c.set_track_links(True)
        if sequence:
            host = np.zeros((5, 2048, 4), np.float32)
            for f, x in enumerate(frames):
                host[f, : len(x)] = x
            ptr, keep = env.upload(host)
            c.sequence_dev(ptr, 2048 * 4, [len(x) for x in frames], [2.0e8 + f * 1e5 for f in range(5)], [0.0] * 5, [0.0] * 5)
        for f in range(5):
            if not sequence:
                keep = launch(env, c, [frames[f]], 2048, f, ego_v=0.0)
            b = f if sequence else 0
            r = read_links(c, b, len(frames[f]))
            assert np.array_equal(r["ids"], r["want"]), f
            elev = c.get_ground(b, n_hint=len(frames[f]))["elevated"]
            east = elev[:, 0] > 0
            m = []
            for side in (east, ~east):
                ids = r["ids"][side]; ids = ids[ids >= 0]
                m.append(int(np.bincount(ids).argmax()) if len(ids) else -1)
            major.append(m)
            if not sequence and f == 4:   # (born in frame 1, second initialisation in frame 2, trackManage 3 after frame 3: confirmed with frame 4)
                tm = c.get_tracks(0)["track_manage"]
                assert all(i >= 0 and tm[i] == 5 for i in m), (f, m, tm)
        if sequence:
            tm = c.get_tracks(0)["track_manage"]
            assert all(i >= 0 and tm[i] == 5 for i in major[4]), (major, tm)
    assert major[3] == major[4] and major[3][0] != major[3][1] and min(major[3]) >= 0, major


# ------------------------------------------------------------------------------------------------------------------ 4: contract
def state_error(env, fn, what):
    try:
        fn()
    except env.mot.MotError as e:
        assert e.code == env.mot.MOT_E_STATE, (what, str(e))
        return
    raise AssertionError((what, "no MOT_E_STATE"))


def snapshot_items(blob):
    """what a snapshot DEFINES, by name (csrc/mot_api_tracks.hip mot_stream_save: header, T track records, the live and just-died lists, the slot bitmap, T output records, then
    the per-ever-track arrays): the records of slots not in use and the tails of the two lists are whatever the context's memory held — two contexts differ there"""
    u = np.frombuffer(blob[:40], np.uint32)
    hb, tb, rb, T, nt, nlive, nzomb = int(u[2]), int(u[3]), int(u[4]), int(u[5]), int(u[6]), int(u[7]), int(u[8])
    o_live = hb + T * tb; o_zomb = o_live + 4 * T; o_used = o_zomb + 4 * T; o_out = o_used + 8 * ((T + 63) // 64); o_ever = o_out + T * rb
    used = np.frombuffer(blob[o_used:o_out], np.uint64)
    slots = [i for i in range(T) if (int(used[i // 64]) >> (i % 64)) & 1]
    items = [("header", blob[:hb]), ("live list", blob[o_live:o_live + 4 * nlive]), ("just-died list", blob[o_zomb:o_zomb + 4 * nzomb]), ("slot bitmap", blob[o_used:o_out]),
             ("per-ever-track arrays", blob[o_ever:])]
    assert len(blob) == o_ever + nt * (16 + 4 + 24), (len(blob), o_ever, nt)
    for i in slots:
        items += [("track record of slot %d" % i, blob[hb + i * tb: hb + (i + 1) * tb]), ("output record of slot %d" % i, blob[o_out + i * rb: o_out + (i + 1) * rb])]
    return items


def contract_off(env, oracle):
    """links off: the getters answer MOT_E_STATE; a context that turned the links on and off again, one that has them on, and one that never heard of them
    deliver byte-identical boxes, tracks and snapshots"""
    blobs = {}
    for tag in ("never", "off again", "on"):
        with env.context(0, max_points=4096, max_batch=2, max_tracks_total=256) as c:
            if tag != "never":
                c.set_track_links(True)
            if tag == "off again":
                c.set_track_links(False)
            for f in range(3):
                keep = launch(env, c, [CC.small_scene(f, 20), CC.small_scene(f + 5, 12)], 4096, f)
            if tag != "on":
                for b in (0, 1):
                    state_error(env, lambda: c.get_box_tracks(b), (tag, "box tracks")); state_error(env, lambda: c.get_point_tracks(b), (tag, "point tracks"))
                dev = np.zeros((2, 64), np.int32); cnt = np.zeros(2, np.int32); pd, kd = env.upload(dev); pc, kc = env.upload(cnt)
                state_error(env, lambda: c.export_point_tracks_dev(2, pd, 64, pc), (tag, "export"))
            out = []
            for b in (0, 1):
                bx = c.get_boxes(b); t = c.get_tracks(b)
                out += [("boxes", bx["boxes"].tobytes()), ("box_cluster", bx["box_cluster"].tobytes())]
                out += [("tracks." + k, np.ascontiguousarray(t[k]).tobytes()) for k in ("track_manage", "lifetime", "p", "v_yaw", "vis_box", "is_vis", "is_static")]
                out += [("snapshot: " + n, x) for n, x in snapshot_items(c.stream_save(b))]
            blobs[tag] = out
    for tag in ("off again", "on"):
        assert [n for n, _ in blobs[tag]] == [n for n, _ in blobs["never"]], tag
        for (n, x), (_, y) in zip(blobs[tag], blobs["never"]):
            assert x == y, (tag, n, "differs from a context that never heard of the links")


def contract_slot_taken(env, oracle):
    p = oracle.params(0)
    with env.context(0, max_points=4096, max_batch=2, max_tracks_total=256) as c:
        c.set_track_links(True)
        state_error(env, lambda: c.get_box_tracks(0), "no step since the links were turned on")
        clouds = [CC.small_scene(0, 20), CC.small_scene(1, 12)]
        keep = launch(env, c, clouds, 4096, 0)
        before = [c.get_point_tracks(b) for b in (0, 1)]
        elev = c.get_ground(0, n_hint=len(clouds[0]))["elevated"]
        c.cluster(elev)   # a stage-wise call takes slot 0
        state_error(env, lambda: c.get_point_tracks(0), "slot 0 after mot_cluster")
        assert np.array_equal(c.get_point_tracks(1), before[1]) and len(before[1]) > 0
        assert len(c.get_box_tracks(0)) == len(c.get_box_tracks(0)) > 0   # the owner row still is the last tracker step's
        dev = np.zeros((2, 4096), np.int32); cnt = np.zeros(2, np.int32); pd, kd = env.upload(dev); pc, kc = env.upload(cnt)
        state_error(env, lambda: c.export_point_tracks_dev(2, pd, 4096, pc), "export over a taken slot")
        keep = launch(env, c, clouds, 4096, 1)   # a fused call gives the slot back
        assert len(c.get_point_tracks(0)) == len(before[0])
        c.ego_update(3.0e8, 0.0, 0.0, 1); c.track_step(lattice(3), 3.0e8, slot=1)   # a tracker step fed from outside
        state_error(env, lambda: c.get_point_tracks(1), "slot 1 after mot_track_step")
        assert len(c.get_box_tracks(1)) == 3
        c.set_track_links(False); c.set_track_links(True)
        state_error(env, lambda: c.get_box_tracks(1), "after switching")


def contract_refused(env, oracle):
    """a frame refused for capacity (capacity_cases: one group beyond max_points / 2) in slot 1 of a fused batch: its link getters answer MOT_E_CAPACITY
    with the limit's message, the neighbour is served, and the device export reads -1 throughout"""
    p = oracle.params(0)
    max_points = 8192
    at, beyond = CC.fused_edges(oracle, p, "groups", max_points)
    with env.context(0, max_points=max_points, max_batch=2, max_tracks_total=2048) as c:
        c.set_track_links(True)
        keep = launch(env, c, [CC.small_scene(0, 20), beyond], max_points, 0)
        CC.refused(env, lambda: c.get_point_tracks(1), CC.MSG_GROUPS, "point tracks of a refused frame")
        CC.refused(env, lambda: c.get_box_tracks(1), CC.MSG_GROUPS, "box tracks of a refused frame")
        r = read_links(c, 0, 0)
        assert np.array_equal(r["ids"], r["want"]) and len(r["ids"]) > 0
        dev = np.full((2, max_points), -7, np.int32); cnt = np.zeros(2, np.int32); pd, kd = env.upload(dev); pc, kc = env.upload(cnt)
        c.export_point_tracks_dev(2, pd, max_points, pc); c.synchronize()
        dev, cnt = download(kd, dev), download(kc, cnt)
        assert cnt[1] > 0 and (dev[1, : cnt[1]] == -1).all() and np.array_equal(dev[0, : cnt[0]], r["ids"])
