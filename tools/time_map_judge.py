"""What indexing a drive's voxel map and judging live frames against the index costs (one context at a time, nothing else on the GPU).
    python tools/time_map_judge.py [--batch 512] [--frames 4] [--drive 154] [--reps 8] [--rounds 3] [--leaves 0.1 0.2] [--out profiles/map_judge.md]
THE MAP: the drive of tools/time_voxel_merge.py — ONE 64-beam stream of the bench's synthetic street scene, `drive` frames x 120 k points with the drive's ego
motion, links on, mot_set_scene_grid({0.2, 512}), 256 track slots, cut into 16 pieces; every piece goes through mot_sequence_products_dev(MOT_SEQ_SCENE) and
mot_export_sequence_scene_voxels_dev (mask KNOWN, min_points 1) at every leaf. Per leaf, interleaved, each call between two events on the context stream:
    merge                 mot_merge_voxel_maps_dev of the 16 maps (counts read from the exports' headers on the device), room for every voxel
    index                 mot_index_voxel_maps_dev on the same inputs
THE FRAMES: ONE context of the headline's shape, 512 streams x 120 k points per launch through mot_frames_dev with links on and mot_set_scene_grid({0.2, 512}) (the
grid only for the comparison: the map judge does not read it); `frames` fused frames per stream taken into the grids, then ONE more fused step that is judged —
the workload of tools/time_scene_judge.py. Per round and interleaved in this one process:
    scene judge           mot_export_scene_points_dev, mask 0b11111, MOT_FRAME_GLOBAL, no class block: the grid judge on the same frames
    map judge             mot_export_map_points_dev, mask 0b11111, MOT_FRAME_GLOBAL, no class block, min_count 1, per leaf at reach 0 and at reach 1
    map judge, counts     the same with null d_points, stride 0, mask 0: classify and scan — what the search itself costs
    the record copy       a device-to-device copy of 16 N_e bytes: 16 N_e read + 16 N_e written, what a full call must move
Reports medians (min - max) over the rounds and writes the markdown of profiles/map_judge.md. No threshold is fixed in advance."""
import argparse
import importlib.util
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_POINTS = 120000
KNOWN = 16
PIECES = 16


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path, submodule_search_locations=[os.path.dirname(path)])
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--drive", type=int, default=154)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leaves", type=float, nargs="+", default=[0.1, 0.2])
    ap.add_argument("--out", default=None, help="write the markdown here as well")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    mot = _load("mot_amd", os.path.join(ROOT, "3d-lidar-multi-object-tracking_amd", "__init__.py"))
    sdev = _load("mot_amd.synth_dev", os.path.join(ROOT, "tools", "synth", "synth_dev.py"))
    stride = ((N_POINTS + 2047) // 2048) * 2048
    res, lines = {}, []

    def timer(c, stream):
        def timed(fn):
            """microseconds per call: `reps` calls, each between two events on the context stream"""
            pairs = []
            for _ in range(args.reps + 1):   # (the first is the warm-up)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream); fn(); b.record(stream)
                pairs.append((a, b))
            c.synchronize()
            return statistics.mean(a.elapsed_time(b) for a, b in pairs[1:]) * 1e3
        return timed
    row = lambda k: f"{statistics.median(res[k]):.0f} ({min(res[k]):.0f} - {max(res[k]):.0f})"
    med = lambda k: statistics.median(res[k])

    # ---- the map: the drive's 16 pieces, merged and indexed
    F = args.drive
    v, yaw = sdev.load_ego(F)
    seq, n_seq, _, _ = sdev.SequenceRenderer("cuda").render([0], F, N_POINTS, stride, v, yaw)
    torch.cuda.synchronize()
    fstride = int(seq.stride(0))
    n0 = np.ascontiguousarray(n_seq[:F, 0])
    ego_v, ego_yaw = [float(x) for x in v[:F]], [float(x) for x in yaw[:F]]
    per = (F + PIECES - 1) // PIECES
    index = {}
    with mot.Context(max_points=stride, max_batch=per, max_tracks_total=256) as c:
        c.set_track_links(True)
        c.set_scene_grid(0.2, 512)
        timed = timer(c, torch.cuda.ExternalStream(c.lib.mot_stream(c._h)))
        maps = {leaf: [] for leaf in args.leaves}
        for k0 in range(0, F, per):
            k1 = min(k0 + per, F)
            c.sequence_products_dev(seq[k0, 0].data_ptr(), fstride, n0[k0:k1], 1.0e9 + 1e5 * np.arange(k0, k1), ego_v[k0:k1], ego_yaw[k0:k1], scene=True)
            for leaf in args.leaves:
                big = torch.empty(((k1 - k0) * stride, 4), dtype=torch.int32, device="cuda"); hdr = torch.zeros(8, dtype=torch.int32, device="cuda")
                c.export_sequence_scene_voxels_dev(k1 - k0, leaf, big.data_ptr(), (k1 - k0) * stride, hdr.data_ptr(), 0, classes=KNOWN)
                c.synchronize()
                n = int(hdr.cpu().numpy()[5])
                maps[leaf].append((big[:n].clone(), hdr, n))
                del big
        for leaf in args.leaves:
            total = sum(n for _, _, n in maps[leaf])
            out = torch.empty((total + 1, 4), dtype=torch.int32, device="cuda"); mh = torch.zeros(8, dtype=torch.int32, device="cuda")
            keys = torch.zeros(total + 1, dtype=torch.int64, device="cuda"); cnt = torch.zeros(total + 1, dtype=torch.int32, device="cuda"); ih = torch.zeros(8, dtype=torch.int32, device="cuda")
            arg = [(b.data_ptr(), h.data_ptr() + 20, n) for b, h, n in maps[leaf]]
            desc = mot.voxel_index(keys.data_ptr(), cnt.data_ptr(), ih.data_ptr(), total)
            calls = {"merge": lambda: c.merge_voxel_maps_dev(arg, leaf, out.data_ptr(), total, mh.data_ptr()), "index": lambda: c.index_voxel_maps_dev(arg, leaf, desc)}
            for _ in range(args.rounds):
                for name, fn in calls.items():
                    res.setdefault((leaf, name), []).append(timed(fn))
                print(leaf, {name: round(res[(leaf, name)][-1], 1) for name in calls}, flush=True)
            h = ih.cpu().numpy()
            assert h.tobytes() == mh.cpu().numpy().tobytes(), "the index call's header is not the merge's"
            k = keys.cpu().numpy()[: h[4]]
            assert (np.diff(k) > 0).all(), "the index's keys are not strictly ascending"
            index[leaf] = dict(desc=desc, keep=(keys, cnt, ih), inputs=total, cells=int(h[4]))
            del out
    del seq, maps

    # ---- the frames: one context of the headline's shape
    B = args.batch
    v, yaw = sdev.load_ego(args.frames)
    seq, n_seq, _, _ = sdev.SequenceRenderer("cuda").render(list(range(B)), args.frames, N_POINTS, stride, v, yaw)
    classes = {}
    with mot.Context(max_points=stride, max_batch=B, max_tracks_total=64) as c:
        c.set_track_links(True)
        c.set_scene_grid(0.2, 512)
        stream = torch.cuda.ExternalStream(c.lib.mot_stream(c._h))
        timed = timer(c, stream)
        ts = [1.0e9]
        def fused(f, ev):
            c.frames_dev(seq[f].data_ptr(), stride * 4, n_seq[f], run_tracker=True, timestamps=[ts[0]] * B, ego_v=[ev] * B, ego_yaw=[float(yaw[f])] * B)
            ts[0] += 1.0e5
        for f in range(args.frames):
            fused(f, float(v[f]))
            c.accumulate_scene(B)
        fused(args.frames - 1, 0.0)   # the judged step
        c.synchronize()
        pts = torch.empty((B, stride, 4), dtype=torch.int32, device="cuda"); seg = torch.zeros((B, 5, 2), dtype=torch.int32, device="cuda")
        scene = lambda: c.export_scene_points_dev(B, pts.data_ptr(), stride, seg.data_ptr(), 0, 0, classes=31, frame="global")
        def judge(leaf, reach, points=True):
            return lambda: c.export_map_points_dev(B, index[leaf]["desc"], pts.data_ptr() if points else 0, stride if points else 0, seg.data_ptr(), 0, 0, min_count=1, reach=reach,
                                                   classes=31 if points else 0, frame="global")
        scene(); c.synchronize()
        ne = int(seg.cpu().numpy()[:, :, 1].astype(np.int64).sum())
        src = torch.empty(4 * ne, dtype=torch.int32, device="cuda").fill_(1); dst = torch.empty_like(src)
        def record_copy():
            with torch.cuda.stream(stream):
                dst.copy_(src)
        calls = {"record copy": record_copy, "scene judge": scene}
        for leaf in args.leaves:
            for reach in (0, 1):
                calls[(leaf, reach, "full")] = judge(leaf, reach); calls[(leaf, reach, "counts")] = judge(leaf, reach, points=False)
                judge(leaf, reach)(); c.synchronize()
                classes[(leaf, reach)] = seg.cpu().numpy()[:, :, 1].astype(np.int64).sum(axis=0)
        for _ in range(args.rounds):
            for name, fn in calls.items():
                res.setdefault(name, []).append(timed(fn))
            print({str(k): round(x[-1], 1) for k, x in res.items() if k in calls}, flush=True)

    lines.append(f"one stream x {F} frames x {N_POINTS} points in {PIECES} pieces, W = 512, cell 0.2 m, mask KNOWN; {args.reps} calls per figure, medians (min - max) of {args.rounds} rounds, us per call\n")
    lines.append("| leaf | input voxels | cells of the index | mot_merge_voxel_maps_dev | mot_index_voxel_maps_dev | index / merge |")
    lines.append("|---|---|---|---|---|---|")
    for leaf in args.leaves:
        lines.append(f"| {leaf} | {index[leaf]['inputs']} | {index[leaf]['cells']} | {row((leaf, 'merge'))} | {row((leaf, 'index'))} | {med((leaf, 'index')) / med((leaf, 'merge')):.2f} |")
    lines.append(f"\n{B} streams x {N_POINTS} points per call, {ne} elevated points, min_count 1, mask 0b11111, MOT_FRAME_GLOBAL; us per call\n")
    lines.append(f"device-to-device copy of 16 N_e bytes: {row('record copy')}; mot_export_scene_points_dev on the same frames: {row('scene judge')}\n")
    lines.append("| leaf | reach | outside / moving / sparse / absent / present | mot_export_map_points_dev | x the record copy | x the scene judge | counts only (classify and scan) |")
    lines.append("|---|---|---|---|---|---|---|")
    for leaf in args.leaves:
        for reach in (0, 1):
            k = (leaf, reach, "full")
            lines.append(f"| {leaf} | {reach} | {' / '.join(str(int(n)) for n in classes[(leaf, reach)])} | {row(k)} | {med(k) / med('record copy'):.2f} | {med(k) / med('scene judge'):.2f} | "
                         f"{row((leaf, reach, 'counts'))} |")
    text = "\n".join(lines)
    print("\n" + text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
