"""A recorded drive into the static-scene grid (mot_sequence_products_dev with MOT_SEQ_SCENE, csrc/scene_grid_seq.hip): bodies shared by
tests/test_emu_scene_grid_seq.py (emulator) and tests/test_scene_grid_seq_gpu.py (MI355X). The callers supply a capacity_cases.Env.

The reference in every case is a SECOND context with max_batch = 1 and otherwise the same parameters, driven frame by frame with frames_dev(batch 1) +
accumulate_scene(1): the path tests/scene_grid_cases.py holds against its numpy model, never the code under test. Compared AS BYTES, slot 0 of both: the export's
cells and header and the getter's. There is no tolerance anywhere. What a case is there to cover (kinds of hits, shifts, invalid windows) is asserted from the
reference alone: its headers after every frame, and scene_grid_cases.Model folded from the reference context's getters."""
import ctypes as C

import numpy as np

import capacity_cases as CC
import scene_grid_cases as SG
import track_accum_cases as AC
import track_accum_seq_cases as SQ
import track_point_cases as PC

SEQ_KERNELS = (b"scene_seq_capture_kernel", b"scene_seq_windows_kernel", b"scene_seq_clear_kernel", b"scene_seq_splat_kernel")


# ------------------------------------------------------------------------------------------------------------------ the two drivers
def ref_step(env, c, cloud, stride, f, ego_v=1.0, yaw=0.0, model=None, accumulate=False):
    """the existing path: one frame through frames_dev(batch 1), then taken into slot 0's grid; model: folded from the getters before the call, as scene_grid_cases does"""
    keep = AC.launch(env, c, [cloud], stride, f, ego_v=[ego_v], yaw=[yaw])
    fold = model.fold(c, 0) if model is not None else None
    c.accumulate_scene(1)
    if accumulate:
        c.accumulate_track_points(1)
    c.synchronize()
    return fold


def seq_call(env, c, clouds, stride, f0, ego_v, yaw, scene=True, accumulate=False, tracks=(0, 0, 0), products=None):
    """frames f0 .. f0 + len(clouds) - 1 of one stream in one call; ego_v / yaw: one value per frame"""
    host = np.zeros((len(clouds), stride, 4), np.float32)
    for k, x in enumerate(clouds):
        host[k, : len(x)] = x
    ptr, keep = env.upload(host)
    c.sequence_products_dev(ptr, stride * 4, [len(x) for x in clouds], [SQ.stamp(f0 + k) for k in range(len(clouds))], list(ego_v), list(yaw), *tracks,
                            accumulate=accumulate, scene=scene, products=products)
    c.synchronize()
    return keep


def grid_state(env, c, W):
    """slot 0's grid as (name, bytes) items: through the export (sentinel margins checked) and through the getter"""
    cells, hdrs = SG.Export(env, 1, W).run(c, 1)
    g = c.get_scene_grid(0)
    return [("export: header", hdrs[0]), ("export: cells", cells[0]), ("getter: header", g["header"].tobytes()), ("getter: cells", g["cells"].tobytes()),
            ("getter: header alone", c.get_scene_grid(0, cells=False)["header"].tobytes())]


def same_grids(env, got, want, W, what):
    for (n, x), (_, y) in zip(got, want):
        if x != y and n.endswith("cells"):
            a, b = (np.frombuffer(v, env.mot.SCENE_CELL_DTYPE).reshape(W, W) for v in (x, y))
            bad = np.argwhere(a != b)
            raise AssertionError((what, n, len(bad), "cells differ; first (v, u)", bad[0], a[tuple(bad[0])], b[tuple(bad[0])]))
        assert x == y, (what, n, np.frombuffer(x, env.mot.SCENE_HEADER_DTYPE), np.frombuffer(y, env.mot.SCENE_HEADER_DTYPE))


def header(c):
    return np.atleast_1d(c.get_scene_grid(0, cells=False)["header"])


def contexts(env, frames, cell, W, max_points, T, order_any=False, accum=None):
    """(the sequence context, the frame-by-frame reference): the same parameters, max_batch = frames against 1"""
    out = []
    for B in (frames, 1):
        c = env.context(0, max_points=max_points, max_batch=B, max_tracks_total=T)
        c.set_track_links(True); c.set_scene_grid(cell, W)
        if accum:
            c.set_track_accumulation(*accum)
        if order_any:
            c.set_point_order(env.mot.MOT_ORDER_ANY)
        out.append(c)
    return out


def other_grids(c):
    return SG.grids(c, c.max_batch)[1:]


def one_call_against_reference(env, clouds, cell, W, max_points, T, ego_v, yaw, what, order_any=False, model=True):
    """all frames in ONE call against the reference -> (the model folded from the reference, its folds, the reference's header after every frame)"""
    F = len(clouds)
    seq, ref = contexts(env, F, cell, W, max_points, T, order_any)
    with seq, ref:
        m = SG.Model(env.mot, 1, cell, W) if model else None
        folds, headers = [], []
        for f, x in enumerate(clouds):
            folds.append(ref_step(env, ref, x, max_points, f, ego_v[f], yaw[f], model=m))
            if m is not None:
                folds[-1]["invalid_so_far"] = m.facts["invalid"]
            headers.append(header(ref).copy())
        others = other_grids(seq)
        seq_call(env, seq, clouds, max_points, 0, ego_v, yaw)
        same_grids(env, grid_state(env, seq, W), grid_state(env, ref, W), W, what)
        assert other_grids(seq) == others, (what, "the grid of a slot >= 1 was touched")
        assert AC.code_of(env, lambda: seq.accumulate_scene(1)) == env.mot.MOT_E_STATE, (what, "the sequence slots cannot be taken again")
    return m, folds, headers


def shifts_of(headers):
    o = [(0, 0)] + [(int(h["origin_i"][0]), int(h["origin_j"][0])) for h in headers]
    return [(b[0] - a[0], b[1] - a[1]) for a, b in zip(o, o[1:])]


# ------------------------------------------------------------------------------------------------------------------ 1: a drive in one call
_DRIVES = {}


def drive(env, frames_n=16, ego_v=1.0, yaw_rate=0.04):
    """stream 2 of scene_grid_cases.standing_and_moving (its generator, its seed): blobs at (8, 5) and (3, -7) stand IN THE WORLD, one at (-9, -6 - 0.3 f) moves;
    the vehicle drives and turns"""
    key = (frames_n, ego_v, yaw_rate)
    if key not in _DRIVES:
        yaw = [yaw_rate * f for f in range(frames_n)]
        S = SG.sensor_from_world(env, [ego_v], [[y] for y in yaw], frames_n)
        rng = np.random.default_rng(3 + 2)
        clouds = [SG.to_sensor(S[f, 0], np.concatenate([SG.world_blob(rng, 8.0, 5.0), SG.world_blob(rng, 3.0, -7.0), SG.world_blob(rng, -9.0, -6.0 - 0.3 * f)]))
                  for f in range(frames_n)]
        _DRIVES[key] = (clouds, [ego_v] * frames_n, yaw)
    return _DRIVES[key]


def a_drive(env, oracle, cell, W):
    clouds, ego_v, yaw = drive(env)
    m, folds, headers = one_call_against_reference(env, clouds, cell, W, 2048, 256, ego_v, yaw, ("drive", cell, W))
    fa = m.facts
    # a track turns static in mid-call: the same blob's cells hold dynamic hits of its young steps and static hits of its later ones
    assert fa["unowned_static"] > 0 and fa["flagged_static"] > 0 and fa["dynamic"] > 0 and fa["both_kinds"] > 0, fa
    ref_cells = m.cells(0)
    assert ((ref_cells["static_hits"] > 0) & (ref_cells["dynamic_hits"] > 0)).any(), "no cell of the reference's final grid holds both kinds"
    if W * cell < 20:   # (0.25, 64): a 16 m window, the blobs 9 to 11 m out
        edge = sum(bool((fo["ids"] == tid)[fo["take"]].any() and (fo["ids"] == tid)[~fo["take"]].any()) for fo in folds for tid in np.unique(fo["ids"]))
        assert fa["outside"] > 0 and edge > 0, (fa, edge)


# ------------------------------------------------------------------------------------------------------------------ 2: slot reuse inside the call
def slot_reuse(env, oracle):
    """track_accum_cases.reuse_stream with 8 track slots: the id -> slot map changes in mid-call. Both products at once, so the accumulators' rows show the reuse"""
    clouds = AC.reuse_stream()
    F, W = len(clouds), 64
    seq, ref = contexts(env, F, 0.5, W, 1024, 8, accum=(64, 4))
    with seq, ref:
        m = SG.Model(env.mot, 1, 0.5, W)
        history = []
        for f, x in enumerate(clouds):
            ref_step(env, ref, x, 1024, f, 0.0, 0.0, model=m, accumulate=True)
            history.append(ref.get_accum_rows(0))
        seq_call(env, seq, clouds, 1024, 0, [0.0] * F, [0.0] * F, accumulate=True)
        same_grids(env, grid_state(env, seq, W), grid_state(env, ref, W), W, "reuse")
        SQ.same_snapshots(SQ.snapshot(env, seq), SQ.snapshot(env, ref), "reuse: the accumulators of the same call")
    first, last = history[0], history[-1]
    changed = np.nonzero((first["track_id"] >= 0) & (last["track_id"] >= 0) & (first["track_id"] != last["track_id"]))[0]
    assert len(changed) >= 1, ("no row went from one id to another inside the call", first["track_id"], last["track_id"])
    assert m.facts["dynamic"] > 0, m.facts


# ------------------------------------------------------------------------------------------------------------------ 3: scroll inside one call
def scroll(env, oracle, invalid_last=False, cell=0.25, W=64):
    """per-frame speed and heading (0.1 s a frame, 0.25 m cells: ego_v 2.5 is one cell a frame). A jump of more than W cells first — nothing of the frames before it
    may be left —, then the window stays, moves by one cell, by several, drives back over its own track and out again (cells leave and re-enter: empty of their
    old hits), jumps out of the range a window can be placed in (invalid) and comes back, and stays. invalid_last: the invalid window is the LAST frame's"""
    spec = [(0.0, 0.0), (0.0, 0.0), (200.0, 0.0), (0.0, 0.0), (0.0, 0.0), (2.5, 0.0), (2.5, 0.0), (10.0, 0.0), (10.0, 0.0), (10.0, np.pi), (10.0, np.pi), (10.0, np.pi),
            (10.0, 0.0), (10.0, 0.0), (3.0e9, 0.0), (3.0e9, np.pi), (1.0, np.pi / 2), (0.0, 0.0)]
    if invalid_last:
        spec = spec[:14] + [(0.0, 0.0), (3.0e9, 0.0)]
    F = len(spec)
    rng = np.random.default_rng(17)   # four blobs within 7 m of the sensor, whatever it does: the window is 16 m wide
    clouds = [np.concatenate([SG.world_blob(rng, cx, cy) for cx, cy in ((5.0, 3.0), (-4.0, 5.0), (2.0, -6.0), (-5.0, -4.0))]) for f in range(F)]
    ego_v, yaw = [s[0] for s in spec], [s[1] for s in spec]
    m, folds, headers = one_call_against_reference(env, clouds, cell, W, 1024, 64, ego_v, yaw, ("scroll", invalid_last))
    sh = shifts_of(headers)[1:]   # (the first step moves the window from the origin of an empty grid)
    big = lambda s: max(abs(s[0]), abs(s[1]))
    assert any(s == (0, 0) for s in sh) and any(big(s) == 1 for s in sh) and any(1 < big(s) < W for s in sh) and any(big(s) >= W for s in sh), sh
    assert any(s[0] < 0 or s[1] < 0 for s in sh) and any(s[0] > 0 or s[1] > 0 for s in sh), ("the window never came back", sh)
    invalid = [f for f in range(F) if folds[f]["invalid_so_far"] > (folds[f - 1]["invalid_so_far"] if f else 0)]
    assert invalid and all(int(headers[f]["n_static"][0]) + int(headers[f]["n_dynamic"][0]) == 0 and headers[f]["n_outside"][0] > 0 and sh[f - 1] == (0, 0) for f in invalid), invalid
    if invalid_last:
        assert invalid[-1] == F - 1 and m.facts["invalid"] == 1, invalid
    else:
        first = invalid[0]
        assert len(invalid) == 1 and 2 < first < F - 2 and big(sh[first]) < W, ("the window did not come back next to where it was", invalid, sh)
        assert sum(int(h["n_static"][0] + h["n_dynamic"][0]) for h in headers[first + 1:]) > 0
    # something of the frames before the invalid one is in the final grid, and nothing of the frames before the jump
    last_seen = m.cells(0)["last_seen"]
    jump = next(f for f, s in enumerate(sh) if big(s) >= W) + 1
    assert (last_seen > 0).any() and last_seen[last_seen > 0].min() > jump, (jump, np.unique(last_seen))
    assert len(np.unique(last_seen[last_seen > 0])) >= 3, np.unique(last_seen)


# ------------------------------------------------------------------------------------------------------------------ 4: chained
def chained(env, oracle, cell=0.5, W=64):
    """frames 0-2 frame by frame, 3-7 one call, 8-9 a second call, frame 10 frame by frame; the vehicle drives two cells a frame, so the rectangle of the old
    contents cuts them. Then reset_slot(0) and a call into the emptied grid"""
    clouds, ego_v, yaw = drive(env, 14, 10.0, 0.04)
    seq, ref = contexts(env, 5, cell, W, 2048, 256)
    with seq, ref:
        headers = []
        for f in range(11):
            ref_step(env, ref, clouds[f], 2048, f, ego_v[f], yaw[f])
            headers.append(header(ref).copy())
        for f in range(3):
            ref_step(env, seq, clouds[f], 2048, f, ego_v[f], yaw[f])
        seq_call(env, seq, clouds[3:8], 2048, 3, ego_v[3:8], yaw[3:8])
        assert header(seq).tobytes() == headers[7].tobytes(), ("after the first call", header(seq), headers[7])
        seq_call(env, seq, clouds[8:10], 2048, 8, ego_v[8:10], yaw[8:10])
        ref_step(env, seq, clouds[10], 2048, 10, ego_v[10], yaw[10])
        same_grids(env, grid_state(env, seq, W), grid_state(env, ref, W), W, "chained")
        sh = shifts_of(headers)
        assert all(s != (0, 0) for s in sh[1:]) and int(headers[-1]["step"][0]) == 10, sh
        g = ref.get_scene_grid(0)["cells"]
        assert (g["last_seen"] > 0).any() and g["last_seen"][g["last_seen"] > 0].min() <= 3, "nothing of the frames before the first call is left: the old contents are not tested"
        seq.reset_slot(0); ref.reset_slot(0)
        for f in (11, 12, 13):
            ref_step(env, ref, clouds[f], 2048, f, ego_v[f], yaw[f])
        seq_call(env, seq, clouds[11:14], 2048, 11, ego_v[11:14], yaw[11:14])
        same_grids(env, grid_state(env, seq, W), grid_state(env, ref, W), W, "after reset_slot")
        assert int(header(ref)["step"][0]) == 2 and int(header(ref)["n_static"][0]) + int(header(ref)["n_dynamic"][0]) > 0, header(ref)


# ------------------------------------------------------------------------------------------------------------------ 5: chunk and wave edges
def shapes(env, oracle, order_any=False):
    """one frame per slot with 0, 1, 63, 64, 65, 2047, 2048, 2049 and 5 000 elevated points and the 160-blob frame (7 719) three times: the splat kernel's chunk is 2048"""
    frames = PC.shape_frames(oracle)
    clouds = list(frames[0]) + [frames[1][-1], frames[2][-1]]
    targets = [len(x) for x in frames[0]]
    assert {0, 1, 63, 64, 65, 2047, 2048, 2049} <= set(targets)
    if order_any:
        clouds = [np.ascontiguousarray(x[np.random.default_rng(7 + f).permutation(len(x))]) for f, x in enumerate(clouds)]
    F = len(clouds)
    seq, ref = contexts(env, F, 1.0, 64, 8192, 512, order_any)
    with seq, ref:
        m = SG.Model(env.mot, 1, 1.0, 64)
        elevated = []
        for f, x in enumerate(clouds):
            ref_step(env, ref, x, 8192, f, 1.0, 0.0, model=m)
            elevated.append(len(ref.get_point_tracks(0)))
        seq_call(env, seq, clouds, 8192, 0, [1.0] * F, [0.0] * F)
        same_grids(env, grid_state(env, seq, 64), grid_state(env, ref, 64), 64, ("shapes", order_any))
        h = header(ref)
        assert elevated[: len(targets)] == targets and elevated[-1] == elevated[-3] == max(targets)
        assert int(h["n_static"][0]) + int(h["n_dynamic"][0]) + int(h["n_outside"][0]) == elevated[-1], (h, elevated[-1])
        assert m.facts["dynamic"] > 0 and m.facts["unowned_static"] > 0 and m.facts["outside"] > 0, m.facts


# ------------------------------------------------------------------------------------------------------------------ 6: contention across frames
def contention(env, oracle, cells_n):
    """cell 10, a standing vehicle: every point of EVERY frame of the call lands in one cell (two with cells_n = 2); counts exact, max_z the maximum"""
    F, W = 6, 64
    rng = np.random.default_rng(21 + cells_n)
    S = SG.sensor_from_world(env, [0.0], [[0.0]] * F, F)
    if cells_n == 1:
        world = [np.concatenate([SG.world_blob(rng, 3.0, 4.0, 400), SG.world_blob(rng, 7.0, 6.0, 400), SG.world_blob(rng, 5.0, 2.0, 300)]) for f in range(F)]
    else:
        world = [np.concatenate([SG.world_blob(rng, 3.0, 4.0, 500), SG.world_blob(rng, 13.0, 6.0, 500)]) for f in range(F)]
    clouds = [SG.to_sensor(S[f, 0], x) for f, x in enumerate(world)]
    m, folds, headers = one_call_against_reference(env, clouds, 10.0, W, 2048, 64, [0.0] * F, [0.0] * F, ("contention", cells_n))
    g = m.cells(0)
    hit = np.argwhere((g["static_hits"] > 0) | (g["dynamic_hits"] > 0))
    total = sum(len(fo["ids"]) for fo in folds)
    assert len(hit) == cells_n and all(fo["take"].all() for fo in folds), (hit, cells_n)
    assert total > 0.7 * sum(len(x) for x in clouds) and int(g["static_hits"].sum()) + int(g["dynamic_hits"].sum()) == total, (total, g[tuple(hit[0])])
    for v, u in hit:
        z = np.concatenate([fo["xyz"][fo["sta"] & (fo["u"] == u) & (fo["v"] == v), 2] for fo in folds])
        assert len(z) == g["static_hits"][v, u] and g["max_z"][v, u] == (z.max() if len(z) else 0.0) and g["last_seen"][v, u] == F, (v, u, g[v, u], len(z))
    assert g["static_hits"].sum() > 0 and g["dynamic_hits"].sum() > 0, g[tuple(hit[0])]
    assert m.facts["dynamic"] > 0 and m.facts["unowned_static"] > 0, m.facts


# ------------------------------------------------------------------------------------------------------------------ 7: a refused frame in the middle
def refused_frame(env, oracle):
    """track_accum_seq_cases.contract_refused_frame's recipe: the frame is taken as the frame-by-frame route takes it, and its step counts"""
    max_points, W = 8192, 64
    at, beyond = CC.fused_edges(oracle, oracle.params(0), "groups", max_points)
    clouds = [CC.small_scene(0, 20), beyond, CC.small_scene(2, 20)]
    seq, ref = contexts(env, 3, 1.0, W, max_points, 2048)
    with seq, ref:
        headers = []
        for f, x in enumerate(clouds):
            ref_step(env, ref, x, max_points, f)
            headers.append(header(ref).copy())
        keep = seq_call(env, seq, clouds, max_points, 0, [1.0] * 3, [0.0] * 3)
        CC.refused(env, lambda: seq.get_track_points(1), CC.MSG_GROUPS, "track points of the refused frame")
        same_grids(env, grid_state(env, seq, W), grid_state(env, ref, W), W, "a refused frame in mid-sequence")
        assert [int(h["step"][0]) for h in headers] == [0, 1, 2] and int(headers[1]["n_dynamic"][0]) == 0, headers
        assert int(headers[2]["n_static"][0]) + int(headers[2]["n_dynamic"][0]) > 0, headers[2]


# ------------------------------------------------------------------------------------------------------------------ 8: products
def products(env, oracle, cell=0.5, W=64):
    """3: the accumulators of sequence_accumulate_dev and the grid of the frame-by-frame reference; 1: sequence_accumulate_dev's snapshot; 0: sequence_dev's readout"""
    clouds, ego_v, yaw = drive(env)
    F = len(clouds)
    def accum_context(grid):
        c = env.context(0, max_points=2048, max_batch=F, max_tracks_total=256)
        c.set_track_links(True); c.set_track_accumulation(256, 4)
        if grid:
            c.set_scene_grid(cell, W)
        return c
    with accum_context(False) as c:
        SQ.seq_call(env, c, clouds, 2048, 0, ego_v, yaw)
        want = SQ.snapshot(env, c)
    assert len(want) > 1, "sequence_accumulate_dev accumulated no track"
    with accum_context(False) as c:
        seq_call(env, c, clouds, 2048, 0, ego_v, yaw, products=env.mot.SEQ_ACCUMULATE)
        SQ.same_snapshots(SQ.snapshot(env, c), want, "products = 1 against sequence_accumulate_dev")
    with env.context(0, max_points=2048, max_batch=1, max_tracks_total=256) as ref:
        ref.set_track_links(True); ref.set_scene_grid(cell, W)
        for f, x in enumerate(clouds):
            ref_step(env, ref, x, 2048, f, ego_v[f], yaw[f])
        want_grid = grid_state(env, ref, W)
    with accum_context(True) as c:
        seq_call(env, c, clouds, 2048, 0, ego_v, yaw, products=env.mot.SEQ_ACCUMULATE | env.mot.SEQ_SCENE)
        SQ.same_snapshots(SQ.snapshot(env, c), want, "products = 3: the accumulators")
        same_grids(env, grid_state(env, c, W), want_grid, W, "products = 3: the grid")
    small = [CC.small_scene(f, 20) for f in range(3)]
    res = []
    for plain in (True, False):
        with env.context(0, max_points=4096, max_batch=3, max_tracks_total=64) as c:
            c.set_track_links(True)
            blk = SQ.TrackBlocks(env, 3, 64)
            if plain:
                keep = SQ.seq_call(env, c, small, 4096, 0, [1.0] * 3, [0.0] * 3, accumulate=False, tracks=blk.args())
            else:
                keep = seq_call(env, c, small, 4096, 0, [1.0] * 3, [0.0] * 3, products=0, tracks=blk.args())
            res.append(SQ.sequence_readout(env, c, [len(x) for x in small]) + blk.read())
    PC.equal_readouts(res[1], res[0], "products = 0 against sequence_dev")


# ------------------------------------------------------------------------------------------------------------------ 9: contract
def contract(env, oracle):
    """every refusal before the tracker has stepped; frames > max_batch; accumulate_scene on the slots afterwards; the other slots' grids"""
    E = env.mot
    W = 64
    clouds = [CC.small_scene(f, 20) for f in range(5)]
    n_points = [len(x) for x in clouds[:3]]
    ones, zeros = [1.0] * 3, [0.0] * 3
    call = lambda c, **kw: AC.code_of(env, lambda: seq_call(env, c, clouds[:3], 4096, 0, ones, zeros, **kw))
    res = {}
    for tag in ("refused first", "fresh"):
        with env.context(0, max_points=4096, max_batch=3, max_tracks_total=64) as c:
            if tag == "refused first":
                assert call(c, scene=True) == E.MOT_E_STATE and call(c, accumulate=True) == E.MOT_E_STATE and call(c, products=3) == E.MOT_E_STATE, "links off"
                c.set_track_links(True)
                assert call(c, scene=True) == E.MOT_E_STATE, "the grid is off"
                assert b"mot_sequence_products_dev" in c.lib.mot_last_error(c._h) and b"scene grid is off" in c.lib.mot_last_error(c._h), c.lib.mot_last_error(c._h)
                assert call(c, accumulate=True) == E.MOT_E_STATE, "accumulation is off"
                c.set_scene_grid(1.0, W)
                assert call(c, products=3) == E.MOT_E_STATE, "the grid on, accumulation off"
                for bits in (4, 6, 8 | 1, -1, 1 << 30):
                    assert call(c, products=bits) == E.MOT_E_ARG, bits
                assert AC.code_of(env, lambda: seq_call(env, c, clouds[:4], 4096, 0, [1.0] * 4, [0.0] * 4)) == E.MOT_E_ARG, "frames > max_batch"
                assert AC.code_of(env, lambda: c.sequence_products_dev(0, 4096 * 4, n_points, [SQ.stamp(0)] * 3, zeros, zeros, scene=True)) == E.MOT_E_ARG, "null cloud"
                assert AC.code_of(env, lambda: c.sequence_products_dev(8, 4096 * 4, n_points, [SQ.stamp(0)] * 3, zeros, zeros, scene=True)) == E.MOT_E_ARG, "misaligned cloud"
                assert int(header(c)["step"][0]) == -1, "a refused call stamped the grid"
                c.set_scene_grid(None)
            c.set_track_links(True)
            keep = SQ.seq_call(env, c, clouds[:3], 4096, 0, ones, zeros, accumulate=False)
            res[tag] = SQ.sequence_readout(env, c, n_points)
    PC.equal_readouts(res["refused first"], res["fresh"], "sequence_dev after the refused calls against a fresh context: the tracker had not stepped")
    seq, ref = contexts(env, 3, 1.0, W, 4096, 64)
    with seq, ref:
        # the other slots' grids hold something: a batch of three streams first (slot 0's grid is the one the call continues, in both contexts)
        keep = AC.launch(env, seq, clouds[2:5], 4096, 0, ego_v=[0.0] * 3)
        seq.accumulate_scene(3)
        ref_step(env, ref, clouds[2], 4096, 0, 0.0)
        others = other_grids(seq)
        assert all(np.frombuffer(h, E.SCENE_HEADER_DTYPE)["n_static"][0] > 0 for h, _ in others)
        for f in range(3):
            ref_step(env, ref, clouds[f], 4096, 1 + f)
        seq_call(env, seq, clouds[:3], 4096, 1, ones, zeros)
        same_grids(env, grid_state(env, seq, W), grid_state(env, ref, W), W, "contract")
        assert other_grids(seq) == others, "the grid of a slot >= 1 was touched"
        before = SG.grids(seq, 3)
        for batch in (1, 3):
            assert AC.code_of(env, lambda: seq.accumulate_scene(batch)) == E.MOT_E_STATE, batch
        assert b"mot_sequence_products_dev" in seq.lib.mot_last_error(seq._h)
        assert SG.grids(seq, 3) == before, "a refused accumulate_scene changed a grid"
        assert int(header(ref)["step"][0]) == 3


# ------------------------------------------------------------------------------------------------------------------ 10: non-interference
def non_interference(env, oracle, order_any=False):
    """everything readable after the call but the grid — every slot's track_point_cases.readout, the track-points exports in both frames, d_tracks / d_counts — is what
    sequence_dev leaves in a context that never turned the grid on; two calls in a row, so the second one starts from the state the first one left"""
    clouds = [CC.small_scene(f, 20) for f in range(4)]
    if order_any:
        clouds = [np.ascontiguousarray(x[np.random.default_rng(11 + f).permutation(len(x))]) for f, x in enumerate(clouds)]
    res = {}
    for tag in ("never", "grid"):
        with env.context(0, max_points=4096, max_batch=2, max_tracks_total=256) as c:
            c.set_track_links(True)
            if order_any:
                c.set_point_order(env.mot.MOT_ORDER_ANY)
            if tag == "grid":
                c.set_scene_grid(1.0, 64)
            out = []
            for f0 in (0, 2):
                blk = SQ.TrackBlocks(env, 2, 64)
                args = (env, c, clouds[f0:f0 + 2], 4096, f0, [1.0] * 2, [0.02 * f0, 0.02 * (f0 + 1)])
                keep = seq_call(*args, tracks=blk.args()) if tag == "grid" else SQ.seq_call(*args, accumulate=False, tracks=blk.args())
                out.append(SQ.sequence_readout(env, c, [len(x) for x in clouds[f0:f0 + 2]]) + blk.read())
            if tag == "grid":
                h = header(c)
                assert int(h["step"][0]) == 3 and int(h["n_static"][0]) + int(h["n_dynamic"][0]) > 0, h
            res[tag] = out
    for k in range(2):
        PC.equal_readouts(res["grid"][k], res["never"][k], (k, "against sequence_dev in a context that never kept a grid"))
    cnt = np.frombuffer(res["never"][1][-1][1], np.int32)
    assert (cnt > 0).all(), ("no live tracks were exported", cnt)


# ------------------------------------------------------------------------------------------------------------------ 11: determinism
def run_script(env, c, W=64):
    clouds, ego_v, yaw = drive(env, 8, 10.0, 0.04)
    c.set_track_links(True); c.set_scene_grid(0.5, W)
    out = []
    for f0 in (0, 4):
        seq_call(env, c, clouds[f0:f0 + 4], 2048, f0, ego_v[f0:f0 + 4], yaw[f0:f0 + 4])
        first = grid_state(env, c, W)
        assert grid_state(env, c, W) == first, (f0, "two readouts of one state differ")
        out.append(first)
    return out


def determinism(env, oracle, other_lib_path=None):
    """the same calls in two contexts give byte-identical grids. other_lib_path (emulator): the second context runs a variant build of the kernels (the plain form of
    the splat kernels, without run merging)"""
    runs = []
    for k in range(2):
        e = env if (k == 0 or other_lib_path is None) else CC.Env(env.mot, other_lib_path, env.upload)
        with e.context(0, max_points=2048, max_batch=4, max_tracks_total=64) as c:
            runs.append(run_script(e, c))
    assert runs[0] == runs[1]
    h = np.frombuffer(runs[0][-1][0][1], env.mot.SCENE_HEADER_DTYPE)
    assert h["step"][0] == 7 and h["n_static"][0] + h["n_dynamic"][0] > 0, h


# ------------------------------------------------------------------------------------------------------------------ 12: emulator only
def launches_and_allocations(env, oracle):
    """the new kernels' launch counters move in the new call and nowhere else (one capture per step, the others once per call); the four existing scene kernels are not
    launched by it; the call's two allocations fail one by one; turning the grid off gives everything back"""
    lib = env.mot.load_library(env.lib_path)
    lib.hipemu_live_allocs.restype = C.c_long
    lib.hipemu_fail_alloc_at.argtypes = [C.c_long]; lib.hipemu_fail_alloc_at.restype = None
    E = env.mot
    W = 64
    count = lambda names: [lib.hipemu_launch_count(k) for k in names]
    clouds = [CC.small_scene(f, 20) for f in range(6)]
    ones, zeros = [1.0] * 3, [0.0] * 3
    try:
        seq, ref = contexts(env, 3, 1.0, W, 4096, 64)
        with ref:   # (closed before anything is counted: every allocation below is the sequence context's)
            for f in range(3):
                ref_step(env, ref, clouds[f], 4096, f)
            want = grid_state(env, ref, W)
        with seq:
            # what sequence mode and the readers keep until mot_destroy, first: what is counted below is the grid's and the new call's own
            SQ.seq_call(env, seq, clouds[:3], 4096, 0, ones, zeros, accumulate=False)
            seq.get_track_points(1, frame="global"); seq.get_scene_grid(0)
            seq.reset_slot(0)
            seq.set_scene_grid(None)
            base = lib.hipemu_live_allocs()
            seq.set_scene_grid(1.0, W); seq.get_scene_grid(0)
            on = lib.hipemu_live_allocs()
            mine, old = count(SEQ_KERNELS), count(SG.KERNELS)
            for k in (1, 2):
                lib.hipemu_fail_alloc_at(k)
                assert AC.code_of(env, lambda: seq_call(env, seq, clouds[:3], 4096, 0, ones, zeros)) == E.MOT_E_HIP, k
                lib.hipemu_fail_alloc_at(0)
                assert b"hipMalloc(&c->d_sgs_" in seq.lib.mot_last_error(seq._h), seq.lib.mot_last_error(seq._h)
                assert lib.hipemu_live_allocs() == on, (k, "a failed call kept memory")
                assert count(SEQ_KERNELS) == mine and count(SG.KERNELS) == old, (k, "a refused call launched")
            seq_call(env, seq, clouds[:3], 4096, 0, ones, zeros)   # the next call succeeds, from the state the refused ones did not touch
            assert lib.hipemu_live_allocs() == on + 2
            assert count(SEQ_KERNELS) == [mine[0] + 3] + [n + 1 for n in mine[1:]] and count(SG.KERNELS) == old
            got = grid_state(env, seq, W)   # (the export kernel: twice)
            same_grids(env, got, want, W, "after two calls refused for memory")
            old = count(SG.KERNELS)
            mine = count(SEQ_KERNELS)
            # sequence_dev and products = 0 with the grid on, the getters, the resets: none of the new kernels
            SQ.seq_call(env, seq, clouds[3:6], 4096, 3, ones, zeros, accumulate=False)
            seq_call(env, seq, clouds[3:6], 4096, 6, ones, zeros, products=0)
            assert AC.code_of(env, lambda: seq.accumulate_scene(1)) == E.MOT_E_STATE
            for b in range(3):
                seq.get_point_tracks(b); seq.get_box_tracks(b); seq.get_track_points(b, frame="global")
            assert count(SEQ_KERNELS) == mine and count(SG.KERNELS) == old
            seq.reset_slot(0); seq.reset()
            assert count(SEQ_KERNELS) == mine
            # a frame-by-frame step launches the existing kernels and none of the new ones
            old = count(SG.KERNELS)
            ref_step(env, seq, clouds[0], 4096, 0)
            assert count(SEQ_KERNELS) == mine and count(SG.KERNELS) == [old[0] + 1, old[1] + 1, old[2], old[3]]
            seq.set_scene_grid(None)
            assert lib.hipemu_live_allocs() == base, "turning the grid off did not free the call's scratch"
            # on again: the scratch comes back with the first call
            seq.set_scene_grid(1.0, W)
            seq_call(env, seq, clouds[:3], 4096, 0, ones, zeros)
            assert lib.hipemu_live_allocs() == on - 1 + 2 and int(header(seq)["step"][0]) == 2
    finally:
        lib.hipemu_fail_alloc_at(0)
