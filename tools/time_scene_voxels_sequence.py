"""What thinning a recorded drive's static map to a voxel grid costs (one context at a time, nothing else on the GPU): ONE 64-beam stream of the bench's synthetic
street scene, 154 frames x 120 k points with the drive's ego motion (BASELINE.json configs[3]), inputs resident in HBM, mot_set_track_links on,
mot_set_scene_grid({0.2, 512}), 256 track slots — the drive of tools/time_scene_judge_sequence.py.
    python tools/time_scene_voxels_sequence.py [--frames 154] [--reps 8] [--rounds 3] [--size 512] [--cell 0.2] [--leaves 0.1 0.2]
Per round and interleaved in this one process, each call between two events on the context stream:
    sequence call         mot_sequence_products_dev(MOT_SEQ_SCENE) over the drive (each call takes the drive into the grid once more; `--seq-reps` calls)
    records               mot_export_sequence_scene_points_dev, mask KNOWN, MOT_FRAME_GLOBAL, no class block: the run the voxel call thins
    record copy           a device-to-device copy of the KNOWN records' 16 m bytes
    voxels, leaf L        mot_export_sequence_scene_voxels_dev, mask KNOWN, min_points 1, record_capacity = m, room for every voxel — per leaf
A voxel call consumes no step, so the timed calls follow each other behind the last sequence call. Reports medians (min - max) over the rounds and prints markdown
rows for profiles/scene_voxels_sequence.md. No ratio is fixed in advance."""
import argparse
import importlib.util
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_POINTS = 120000
KNOWN = 16


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path, submodule_search_locations=[os.path.dirname(path)])
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=154)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--seq-reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cell", type=float, default=0.2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--leaves", type=float, nargs="+", default=[0.1, 0.2])
    ap.add_argument("--tracks", type=int, default=256, help="max_tracks_total")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    mot = _load("mot_amd", os.path.join(ROOT, "3d-lidar-multi-object-tracking_amd", "__init__.py"))
    sdev = _load("mot_amd.synth_dev", os.path.join(ROOT, "tools", "synth", "synth_dev.py"))
    F = args.frames
    stride = ((N_POINTS + 2047) // 2048) * 2048
    v, yaw = sdev.load_ego(F)
    seq, n_seq, _, _ = sdev.SequenceRenderer("cuda").render([0], F, N_POINTS, stride, v, yaw)
    torch.cuda.synchronize()
    fstride = int(seq.stride(0))   # floats between consecutive frames of the stream
    n0 = np.ascontiguousarray(n_seq[:F, 0])
    ego_v, ego_yaw = [float(x) for x in v[:F]], [float(x) for x in yaw[:F]]
    res = {}
    with mot.Context(max_points=stride, max_batch=F, max_tracks_total=args.tracks) as c:
        c.set_track_links(True)
        c.set_scene_grid(args.cell, args.size)
        stream = torch.cuda.ExternalStream(c.lib.mot_stream(c._h))
        calls_made = [0]

        def drive(_s=None):
            ts = 1.0e9 + 1e5 * (np.arange(F) + F * calls_made[0]); calls_made[0] += 1
            c.sequence_products_dev(seq[0, 0].data_ptr(), fstride, n0, ts, ego_v, ego_yaw, scene=True)

        def timed(fn, reps):
            """microseconds per call: `reps` calls, each between two events on the context stream"""
            pairs = []
            for _ in range(reps + 1):   # (the first is the warm-up)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream); fn(stream); b.record(stream)
                pairs.append((a, b))
            c.synchronize()
            return statistics.mean(a.elapsed_time(b) for a, b in pairs[1:]) * 1e3

        drive(); c.synchronize()
        seg = torch.zeros((F, 5, 2), dtype=torch.int32, device="cuda"); tot = torch.zeros((5, 2), dtype=torch.int32, device="cuda")
        hdr = torch.zeros(8, dtype=torch.int32, device="cuda")
        c.export_sequence_scene_points_dev(F, 0, 0, seg.data_ptr(), tot.data_ptr(), classes=0)
        c.synchronize()
        m = int(tot.cpu().numpy()[4, 1])
        pts = torch.empty((m + 1, 4), dtype=torch.int32, device="cuda"); vox = torch.empty((m + 1, 4), dtype=torch.int32, device="cuda")
        src = torch.empty(4 * m, dtype=torch.int32, device="cuda").fill_(1); dst = torch.empty_like(src)

        def record_copy(s):
            with torch.cuda.stream(s):
                dst.copy_(src)
        calls = {"sequence call": (drive, args.seq_reps),
                 "records": (lambda s: c.export_sequence_scene_points_dev(F, pts.data_ptr(), m, seg.data_ptr(), tot.data_ptr(), classes=KNOWN, frame="global"), args.reps),
                 "record copy": (record_copy, args.reps)}
        for leaf in args.leaves:
            calls[f"voxels, leaf {leaf}"] = (lambda s, leaf=leaf: c.export_sequence_scene_voxels_dev(F, leaf, vox.data_ptr(), m, hdr.data_ptr(), 0, classes=KNOWN, record_capacity=m), args.reps)
        for _ in range(args.rounds):
            for name, (fn, reps) in calls.items():
                res.setdefault(name, []).append(timed(fn, reps))
            print({k: round(x[-1], 1) for k, x in res.items()}, flush=True)
        headers = {}
        for leaf in args.leaves:
            calls[f"voxels, leaf {leaf}"][0](stream); c.synchronize()
            headers[leaf] = hdr.cpu().numpy().copy()
    med = {k: statistics.median(x) for k, x in res.items()}
    row = lambda k: f"{med[k]:.0f} ({min(res[k]):.0f} - {max(res[k]):.0f})"
    print(f"\none stream x {F} frames x {N_POINTS} points, W = {args.size}, cell {args.cell} m: {m} KNOWN records; {args.reps} calls per figure ({args.seq_reps} for the "
          f"sequence call), medians (min - max) of {args.rounds} rounds")
    print("| call | us per call | x the record copy | x the records call | x the sequence call | voxels | n_outside |")
    print("|---|---|---|---|---|---|---|")
    print(f"| device-to-device copy of 16 m bytes | {row('record copy')} | 1 | | | | |")
    print(f"| mot_export_sequence_scene_points_dev, KNOWN, global | {row('records')} | {med['records'] / med['record copy']:.2f} | 1 | {med['records'] / med['sequence call']:.3f} | | |")
    print(f"| mot_sequence_products_dev(MOT_SEQ_SCENE), {F} frames | {row('sequence call')} | {med['sequence call'] / med['record copy']:.1f} | | 1 | | |")
    for leaf in args.leaves:
        k = f"voxels, leaf {leaf}"; h = headers[leaf]
        print(f"| mot_export_sequence_scene_voxels_dev, KNOWN, leaf {leaf} m | {row(k)} | {med[k] / med['record copy']:.1f} | {med[k] / med['records']:.1f} | {med[k] / med['sequence call']:.3f} | "
              f"{int(h[3])} | {int(h[2])} |")


if __name__ == "__main__":
    main()
