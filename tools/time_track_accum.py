"""What mot_accumulate_track_points costs (one context, nothing else on the GPU), on the bench's synthetic street frames in the shape of ONE context of the
headline: 512 streams x 120 k points per launch, ground -> cluster -> box -> tracker through mot_frames_dev with mot_set_track_links on, inputs resident in HBM.
    python tools/time_track_accum.py [--batch 512] [--frames 4] [--reps 8] [--rounds 3] [--points-per-track 4096] [--obs-per-track 16]
After the streams' first frames, per round and interleaved in this one process, each figure between two events on the context stream (a step is appended at most
once, so ONE fused step — the last frame again, the ego standing — runs untimed before every timed call, of all three kinds alike):
    accumulate                    mot_accumulate_track_points(batch): the table and count kernels of the per-track point clouds, the plan kernel, the scatter into
                                  the rings, and one copy of 52 bytes per slot ahead of them
    the export                    mot_export_track_points_dev, global frame, without the rest segment: the call a user would make before an append of their own
    the copy                      a device-to-device copy of 16 N_e bytes, as in tools/time_track_points.py
Reports the medians over the rounds, the accumulate call as a multiple of both yardsticks and the bytes it moves on the accounting of csrc/track_accum.hip.
Prints markdown rows for profiles/track_accum.md. No ratio is fixed in advance."""
import argparse
import importlib.util
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_POINTS = 120000
MAX_SEG = 1025


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
    ap.add_argument("--points-per-track", type=int, default=4096)
    ap.add_argument("--obs-per-track", type=int, default=16)
    ap.add_argument("--tracks", type=int, default=64, help="max_tracks_total")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    mot = _load("mot_amd", os.path.join(ROOT, "3d-lidar-multi-object-tracking_amd", "__init__.py"))
    sdev = _load("mot_amd.synth_dev", os.path.join(ROOT, "tools", "synth", "synth_dev.py"))
    B, K, O = args.batch, args.points_per_track, args.obs_per_track
    stride = ((N_POINTS + 2047) // 2048) * 2048
    v, yaw = sdev.load_ego(args.frames)
    seq, n_seq, _, _ = sdev.SequenceRenderer("cuda").render(list(range(B)), args.frames, N_POINTS, stride, v, yaw)
    res = {"accumulate": [], "export": [], "copy": []}
    with mot.Context(max_points=stride, max_batch=B, max_tracks_total=args.tracks) as c:
        c.set_track_links(True)
        c.set_track_accumulation(K, O)
        stream = torch.cuda.ExternalStream(c.lib.mot_stream(c._h))
        ts = [1.0e9]
        def fused(f, ego_v):
            c.frames_dev(seq[f].data_ptr(), stride * 4, n_seq[f], run_tracker=True, timestamps=[ts[0]] * B, ego_v=[ego_v] * B, ego_yaw=[float(yaw[f])] * B)
            ts[0] += 1.0e5
        for f in range(args.frames):
            fused(f, float(v[f]))
            c.accumulate_track_points(B)
        c.synchronize()
        last = args.frames - 1
        pts = torch.empty((B, stride, 4), dtype=torch.int32, device="cuda"); seg = torch.empty((B, MAX_SEG, 4), dtype=torch.int32, device="cuda")
        cnt = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
        export = lambda rest=False: c.export_track_points_dev(B, pts.data_ptr(), stride, seg.data_ptr(), MAX_SEG, cnt.data_ptr(), rest=rest, frame="global")
        export(True); c.synchronize()
        ne = int(cnt[:, 1].sum().item())
        src = torch.empty(4 * ne, dtype=torch.int32, device="cuda").fill_(1); dst = torch.empty_like(src)
        def copy():
            with torch.cuda.stream(stream):
                dst.copy_(src)
        calls = {"accumulate": lambda: c.accumulate_track_points(B), "export": export, "copy": copy}

        def timed(fn):
            """microseconds per call: `reps` calls, each behind an untimed fused step, each between two events on the context stream"""
            pairs = []
            for _ in range(args.reps + 1):   # (the first is the warm-up)
                fused(last, 0.0)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream); fn(); b.record(stream)
                pairs.append((a, b))
            c.synchronize()
            return statistics.mean(a.elapsed_time(b) for a, b in pairs[1:]) * 1e3

        for _ in range(args.rounds):
            for name, fn in calls.items():
                res[name].append(timed(fn))
            print({k: round(x[-1], 1) for k, x in res.items()}, flush=True)
        export(False); c.synchronize()
        owned = int(cnt[:, 1].sum().item()); nseg = float(cnt[:, 0].float().mean().item())
        rows = [c.get_accum_rows(b) for b in range(0, B, max(B // 8, 1))]
        wrapped = sum(int((r["total"] > K).sum()) for r in rows); used = sum(int((r["track_id"] >= 0).sum()) for r in rows)
    med = {k: statistics.median(x) for k, x in res.items()}
    spread = {k: (min(x), max(x)) for k, x in res.items()}
    moved = 20.0 * ne + 16.0 * owned + nseg * B * (2 * 32 + 48 + 8 + 144)
    print(f"\n{B} streams x {N_POINTS} points per call, K = {K}, O = {O}, {args.tracks} track slots: {ne} elevated points, {owned} of them ({100.0 * owned / max(ne, 1):.0f} %) owned by a "
          f"track, {nseg:.1f} tracks per frame; {used} rows in use in the sampled slots, {wrapped} of them wrapped; {args.reps} calls per figure, medians (min - max) of {args.rounds} rounds")
    print("| call | us per call | x the copy | x the export | TB/s on its own bytes |")
    print("|---|---|---|---|---|")
    print(f"| device-to-device copy of 16 N_e bytes | {med['copy']:.0f} ({spread['copy'][0]:.0f} - {spread['copy'][1]:.0f}) | 1 | {med['copy'] / med['export']:.2f} | {32.0 * ne / med['copy'] / 1e6:.2f} |")
    print(f"| export, global frame, without the rest segment | {med['export']:.0f} ({spread['export'][0]:.0f} - {spread['export'][1]:.0f}) | {med['export'] / med['copy']:.2f} | 1 | "
          f"{(20.0 * ne + 16.0 * owned) / med['export'] / 1e6:.2f} |")
    print(f"| mot_accumulate_track_points | {med['accumulate']:.0f} ({spread['accumulate'][0]:.0f} - {spread['accumulate'][1]:.0f}) | {med['accumulate'] / med['copy']:.2f} | "
          f"{med['accumulate'] / med['export']:.2f} | {moved / med['accumulate'] / 1e6:.2f} |")
    print(f"bytes moved per accumulate call: {moved / 1e6:.1f} MB (20 N_e read + 16 per owned point written + 296 per segment)")


if __name__ == "__main__":
    main()
