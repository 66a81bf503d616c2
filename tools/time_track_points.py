"""What mot_export_track_points_dev costs (one context, nothing else on the GPU), on the bench's synthetic street frames in the shape of ONE context of the
headline: 512 streams x 120 k points per launch, ground -> cluster -> box -> tracker through mot_frames_dev with mot_set_track_links on, inputs resident in HBM.
    python tools/time_track_points.py [--batch 512] [--frames 4] [--reps 20] [--rounds 3]
After the streams' first frames, per round and interleaved in this one process:
    export, sensor / global frame, without / with MOT_TRACK_POINTS_REST    microseconds per call of `batch` frames: wall clock over `reps` back-to-back calls that
                                                                           end in a synchronise (four kernels per call; global: and one 48-byte-per-slot copy)
    the yardstick                                                          a device-to-device copy of 16 N_e bytes: it reads what the export must read (4 N_e of ids
                                                                           + 12 N_e of points) and writes what it must write with the flag (16 N_e of records)
Reports the medians over the rounds, each export as a multiple of the copy, and the achieved bytes/s on the export's own accounting (csrc/track_points.hip:
36 bytes per elevated point with the flag; without it the records of the rest are not written). Prints markdown rows for profiles/track_points.md. No ratio is
fixed in advance: the copy is the yardstick."""
import argparse
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_POINTS = 120000
MAX_SEG = 1025


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path, submodule_search_locations=[os.path.dirname(path)])
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def timed(fn, sync, reps):
    fn(); sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / reps * 1e6


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    mot = _load("mot_amd", os.path.join(ROOT, "3d-lidar-multi-object-tracking_amd", "__init__.py"))
    sdev = _load("mot_amd.synth_dev", os.path.join(ROOT, "tools", "synth", "synth_dev.py"))
    B = args.batch
    stride = ((N_POINTS + 2047) // 2048) * 2048
    v, yaw = sdev.load_ego(args.frames)
    seq, n_seq, _, _ = sdev.SequenceRenderer("cuda").render(list(range(B)), args.frames, N_POINTS, stride, v, yaw)
    legs = [(fr, rest) for fr in ("sensor", "global") for rest in (False, True)]
    res = {leg: [] for leg in legs}; res["copy"] = []
    with mot.Context(max_points=stride, max_batch=B, max_tracks_total=64) as c:
        c.set_track_links(True)
        for f in range(args.frames):
            c.frames_dev(seq[f].data_ptr(), stride * 4, n_seq[f], run_tracker=True, timestamps=[1.0e9 + f * 1.0e5] * B, ego_v=[float(v[f])] * B, ego_yaw=[float(yaw[f])] * B)
        c.synchronize()
        pts = torch.empty((B, stride, 4), dtype=torch.int32, device="cuda"); seg = torch.empty((B, MAX_SEG, 4), dtype=torch.int32, device="cuda")
        cnt = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
        export = lambda fr, rest: c.export_track_points_dev(B, pts.data_ptr(), stride, seg.data_ptr(), MAX_SEG, cnt.data_ptr(), rest=rest, frame=fr)
        export("sensor", True); c.synchronize()
        ne = int(cnt[:, 1].sum().item()); nseg = float(cnt[:, 0].float().mean().item()) - 1
        export("sensor", False); c.synchronize()
        owned = int(cnt[:, 1].sum().item())
        src = torch.empty(4 * ne, dtype=torch.int32, device="cuda").fill_(1); dst = torch.empty_like(src)
        for _ in range(args.rounds):
            for leg in legs:
                res[leg].append(timed(lambda: export(*leg), c.synchronize, args.reps))
            res["copy"].append(timed(lambda: dst.copy_(src), torch.cuda.synchronize, args.reps))
            print({str(k): round(x[-1], 1) for k, x in res.items()}, flush=True)
    med = {k: statistics.median(x) for k, x in res.items()}
    print(f"\n{B} streams x {N_POINTS} points per call: {ne} elevated points, {owned} of them ({100.0 * owned / max(ne, 1):.0f} %) owned by a track, {nseg:.1f} tracks per frame; "
          f"{args.reps} back-to-back calls per figure, medians of {args.rounds} rounds")
    print("| call | us per call | x the copy | TB/s on its own bytes |")
    print("|---|---|---|---|")
    print(f"| device-to-device copy of 16 N_e bytes (16 N_e read, 16 N_e written) | {med['copy']:.0f} | 1 | {32.0 * ne / med['copy'] / 1e6:.2f} |")
    for fr, rest in legs:
        own = 20.0 * ne + 16.0 * (ne if rest else owned)
        print(f"| export, {fr} frame, {'with' if rest else 'without'} the rest segment | {med[fr, rest]:.0f} | {med[fr, rest] / med['copy']:.2f} | {own / med[fr, rest] / 1e6:.2f} |")


if __name__ == "__main__":
    main()
