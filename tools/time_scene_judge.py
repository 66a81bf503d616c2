"""What judging a frame's points against the scene grid costs (one context, nothing else on the GPU), on the bench's synthetic street frames in the shape of ONE
context of the headline: 512 streams x 120 k points per launch, ground -> cluster -> box -> tracker through mot_frames_dev with mot_set_track_links on, inputs
resident in HBM, mot_set_scene_grid({0.2, 512}) — the shape of tools/time_scene_grid.py.
    python tools/time_scene_judge.py [--batch 512] [--frames 4] [--reps 8] [--rounds 3] [--size 512] [--cell 0.2]
`frames` fused frames per stream are taken into the grids first, then ONE more fused step (the last frame again, the ego standing) that is NOT taken in: the
judged state is the intended one, a frame against history alone. A judge call consumes no step, so the timed calls follow each other; per round and interleaved
in this one process, each call between two events on the context stream:
    full                  mot_export_scene_points_dev, mask 0b11111, MOT_FRAME_GLOBAL, no class block: classify, scan, scatter
    known only            the same with mask 0b10000
    counts only           null d_points, stride 0, mask 0, no class block: classify and scan
    the record copy       a device-to-device copy of 16 N_e bytes: 16 N_e read + 16 N_e written, what the full call must move
    the read copy         a device-to-device copy of 8 N_e bytes: 16 N_e bytes moved, what the counts-only call must read
    track points          mot_export_track_points_dev(rest, MOT_FRAME_GLOBAL) on the same frames: the nearest relative
Reports medians (min - max) over the rounds and prints markdown rows for profiles/scene_judge.md. No ratio is fixed in advance."""
import argparse
import importlib.util
import os
import statistics
import sys

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
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--cell", type=float, default=0.2)
    ap.add_argument("--tracks", type=int, default=64, help="max_tracks_total")
    ap.add_argument("--points", type=int, default=N_POINTS, help="points per frame")
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    mot = _load("mot_amd", os.path.join(ROOT, "3d-lidar-multi-object-tracking_amd", "__init__.py"))
    sdev = _load("mot_amd.synth_dev", os.path.join(ROOT, "tools", "synth", "synth_dev.py"))
    B, W, n_points = args.batch, args.size, args.points
    stride = ((n_points + 2047) // 2048) * 2048
    v, yaw = sdev.load_ego(args.frames)
    seq, n_seq, _, _ = sdev.SequenceRenderer("cuda").render(list(range(B)), args.frames, n_points, stride, v, yaw)
    with mot.Context(max_points=stride, max_batch=B, max_tracks_total=args.tracks) as c:
        c.set_track_links(True)
        c.set_scene_grid(args.cell, W)
        stream = torch.cuda.ExternalStream(c.lib.mot_stream(c._h))
        ts = [1.0e9]
        def fused(f, ego_v):
            c.frames_dev(seq[f].data_ptr(), stride * 4, n_seq[f], run_tracker=True, timestamps=[ts[0]] * B, ego_v=[ego_v] * B, ego_yaw=[float(yaw[f])] * B)
            ts[0] += 1.0e5
        for f in range(args.frames):
            fused(f, float(v[f]))
            c.accumulate_scene(B)
        fused(args.frames - 1, 0.0)   # the judged step: not taken in
        c.synchronize()
        pts = torch.empty((B, stride, 4), dtype=torch.int32, device="cuda"); seg = torch.zeros((B, 5, 2), dtype=torch.int32, device="cuda")
        tseg = torch.empty((B, 1025, 4), dtype=torch.int32, device="cuda"); tcnt = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
        judge = lambda mask, points=True: c.export_scene_points_dev(B, pts.data_ptr() if points else 0, stride if points else 0, seg.data_ptr(), 0, 0, classes=mask, frame="global")
        judge(31); c.synchronize()
        counts = seg.cpu().numpy()[:, :, 1].astype(np.int64).sum(axis=0)
        ne = int(counts.sum())
        src = torch.empty(4 * ne, dtype=torch.int32, device="cuda").fill_(1); dst = torch.empty_like(src)
        def record_copy():
            with torch.cuda.stream(stream):
                dst.copy_(src)
        def read_copy():
            with torch.cuda.stream(stream):
                dst[: 2 * ne].copy_(src[: 2 * ne])
        calls = {"full": lambda: judge(31), "known only": lambda: judge(16), "counts only": lambda: judge(0, points=False), "record copy": record_copy, "read copy": read_copy,
                 "track points": lambda: c.export_track_points_dev(B, pts.data_ptr(), stride, tseg.data_ptr(), 1025, tcnt.data_ptr(), rest=True, frame="global")}
        res = {k: [] for k in calls}

        def timed(fn):
            """microseconds per call: `reps` calls, each between two events on the context stream"""
            pairs = []
            for _ in range(args.reps + 1):   # (the first is the warm-up)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream); fn(); b.record(stream)
                pairs.append((a, b))
            c.synchronize()
            return statistics.mean(a.elapsed_time(b) for a, b in pairs[1:]) * 1e3

        for _ in range(args.rounds):
            for name, fn in calls.items():
                res[name].append(timed(fn))
            print({k: round(x[-1], 1) for k, x in res.items()}, flush=True)
    med = {k: statistics.median(x) for k, x in res.items()}
    row = lambda k: f"{med[k]:.0f} ({min(res[k]):.0f} - {max(res[k]):.0f})"
    names = ("unknown", "moving", "trail", "new", "known")
    print(f"\n{B} streams x {n_points} points per call, W = {W}, cell {args.cell} m: {ne} elevated points; " + ", ".join(f"{int(k)} {n}" for k, n in zip(counts, names)) +
          f"; {args.reps} calls per figure, medians (min - max) of {args.rounds} rounds")
    print("| call | us per call | x the record copy | x the read copy | x track points |")
    print("|---|---|---|---|---|")
    print(f"| device-to-device copy of 16 N_e bytes (32 N_e moved) | {row('record copy')} | 1 | | |")
    print(f"| device-to-device copy of 8 N_e bytes (16 N_e moved) | {row('read copy')} | | 1 | |")
    print(f"| mot_export_track_points_dev (rest, global) | {row('track points')} | {med['track points'] / med['record copy']:.2f} | | 1 |")
    for k, what in (("full", "mot_export_scene_points_dev, mask 0b11111, global"), ("known only", "... KNOWN only (mask 0b10000)"), ("counts only", "... counts only (null d_points, mask 0)")):
        print(f"| {what} | {row(k)} | {med[k] / med['record copy']:.2f} | {med[k] / med['read copy']:.2f} | {med[k] / med['track points']:.2f} |")


if __name__ == "__main__":
    main()
