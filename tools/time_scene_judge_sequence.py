"""What judging a recorded drive against its scene grid costs (one context at a time, nothing else on the GPU): ONE 64-beam stream of the bench's synthetic street
scene, 154 frames x 120 k points with the drive's ego motion (BASELINE.json configs[3]), inputs resident in HBM, mot_set_track_links on,
mot_set_scene_grid({0.2, 512}), 256 track slots — the drive of tools/time_scene_grid_sequence.py.
    python tools/time_scene_judge_sequence.py [--frames 154] [--reps 8] [--rounds 3] [--size 512] [--cell 0.2]
The drive is taken once with mot_sequence_products_dev(MOT_SEQ_SCENE); a judge call consumes no step, so the timed calls follow each other. Per round and interleaved
in this one process, each call between two events on the context stream:
    full                  mot_export_sequence_scene_points_dev, mask 0b11111, MOT_FRAME_GLOBAL, no class block: classify, two scans, scatter
    known only            the same with mask 0b10000: the static map
    counts only           null d_points, capacity 0, mask 0, no class block: classify and the two scans
    the record copy       a device-to-device copy of 16 N_e bytes: what the full call must write, and read once
    the read copy         a device-to-device copy of 8 N_e bytes: 16 N_e bytes moved, what the counts-only call must read
Then, in the same session, the SAME frames as `frames` streams of a batch (mot_frames_dev + mot_accumulate_scene twice, a third step not taken in) and
    per-frame call        mot_export_scene_points_dev over the batch, mask 0b11111, MOT_FRAME_GLOBAL, no class block: the same number of points in batch mode
Reports medians (min - max) over the rounds and prints markdown rows for profiles/scene_judge_sequence.md. No ratio is fixed in advance."""
import argparse
import importlib.util
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_POINTS = 120000


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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cell", type=float, default=0.2)
    ap.add_argument("--size", type=int, default=512)
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
    n0 = np.ascontiguousarray(n_seq[:F, 0]); ts = 1.0e9 + 1e5 * np.arange(F)
    ego_v, ego_yaw = [float(x) for x in v[:F]], [float(x) for x in yaw[:F]]
    res = {}

    def context():
        c = mot.Context(max_points=stride, max_batch=F, max_tracks_total=args.tracks)
        c.set_track_links(True)
        c.set_scene_grid(args.cell, args.size)
        return c

    def measure(c, calls):
        stream = torch.cuda.ExternalStream(c.lib.mot_stream(c._h))

        def timed(fn):
            """microseconds per call: `reps` calls, each between two events on the context stream"""
            pairs = []
            for _ in range(args.reps + 1):   # (the first is the warm-up)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream); fn(stream); b.record(stream)
                pairs.append((a, b))
            c.synchronize()
            return statistics.mean(a.elapsed_time(b) for a, b in pairs[1:]) * 1e3

        for k in calls:
            res.setdefault(k, [])
        for _ in range(args.rounds):
            for name, fn in calls.items():
                res[name].append(timed(fn))
            print({k: round(res[k][-1], 1) for k in calls}, flush=True)

    with context() as c:
        c.sequence_products_dev(seq[0, 0].data_ptr(), fstride, n0, ts, ego_v, ego_yaw, scene=True)
        c.synchronize()
        seg = torch.zeros((F, 5, 2), dtype=torch.int32, device="cuda"); tot = torch.zeros((5, 2), dtype=torch.int32, device="cuda")
        c.export_sequence_scene_points_dev(F, 0, 0, seg.data_ptr(), tot.data_ptr(), classes=0)
        c.synchronize()
        counts = tot.cpu().numpy()[:, 1].astype(np.int64)
        ne = int(counts.sum())
        pts = torch.empty((ne + 1, 4), dtype=torch.int32, device="cuda")
        src = torch.empty(4 * ne, dtype=torch.int32, device="cuda").fill_(1); dst = torch.empty_like(src)
        judge = lambda mask, points=True: c.export_sequence_scene_points_dev(F, pts.data_ptr() if points else 0, ne if points else 0, seg.data_ptr(), tot.data_ptr(), classes=mask, frame="global")

        def record_copy(stream):
            with torch.cuda.stream(stream):
                dst.copy_(src)

        def read_copy(stream):
            with torch.cuda.stream(stream):
                dst[: 2 * ne].copy_(src[: 2 * ne])
        measure(c, {"full": lambda s: judge(31), "known only": lambda s: judge(16), "counts only": lambda s: judge(0, points=False), "record copy": record_copy, "read copy": read_copy})
        del pts, src, dst
    with context() as c:   # the same frames as F streams of a batch: two steps taken in, a third judged against history alone
        blk = torch.empty((F, stride, 4), dtype=torch.int32, device="cuda"); bseg = torch.zeros((F, 5, 2), dtype=torch.int32, device="cuda")
        for k in range(3):
            c.frames_dev(seq[0, 0].data_ptr(), fstride, n0, run_tracker=True, timestamps=[1.0e9 + 1e5 * k] * F, ego_v=[0.0] * F, ego_yaw=ego_yaw)
            if k < 2:
                c.accumulate_scene(F)
        c.synchronize()
        per_frame = lambda s: c.export_scene_points_dev(F, blk.data_ptr(), stride, bseg.data_ptr(), 0, 0, classes=31, frame="global")
        per_frame(None); c.synchronize()
        ne_batch = int(bseg.cpu().numpy()[:, :, 1].astype(np.int64).sum())
        measure(c, {"per-frame call": per_frame})
    med = {k: statistics.median(x) for k, x in res.items()}
    row = lambda k: f"{med[k]:.0f} ({min(res[k]):.0f} - {max(res[k]):.0f})"
    names = ("unknown", "moving", "trail", "new", "known")
    print(f"\none stream x {F} frames x {N_POINTS} points, W = {args.size}, cell {args.cell} m: {ne} elevated points ({ne_batch} in the batch); " +
          ", ".join(f"{int(k)} {n}" for k, n in zip(counts, names)) + f"; {args.reps} calls per figure, medians (min - max) of {args.rounds} rounds")
    print("| call | us per call | x the record copy | x the read copy | x the per-frame call |")
    print("|---|---|---|---|---|")
    print(f"| device-to-device copy of 16 N_e bytes (32 N_e moved) | {row('record copy')} | 1 | | |")
    print(f"| device-to-device copy of 8 N_e bytes (16 N_e moved) | {row('read copy')} | | 1 | |")
    print(f"| mot_export_scene_points_dev, {F} streams of a batch, mask 0b11111, global | {row('per-frame call')} | {med['per-frame call'] / med['record copy']:.2f} | | 1 |")
    for k, what in (("full", "mot_export_sequence_scene_points_dev, mask 0b11111, global"), ("known only", "... KNOWN only (mask 0b10000): the static map"),
                    ("counts only", "... counts only (null d_points, mask 0)")):
        print(f"| {what} | {row(k)} | {med[k] / med['record copy']:.2f} | {med[k] / med['read copy']:.2f} | {med[k] / med['per-frame call']:.2f} |")


if __name__ == "__main__":
    main()
