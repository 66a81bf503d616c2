"""What the rolling static-scene grid costs (one context, nothing else on the GPU), on the bench's synthetic street frames in the shape of ONE context of the
headline: 512 streams x 120 k points per launch, ground -> cluster -> box -> tracker through mot_frames_dev with mot_set_track_links on, inputs resident in HBM.
    python tools/time_scene_grid.py [--batch 512] [--frames 4] [--reps 8] [--rounds 3] [--size 512] [--cell 0.2] [--lib PATH]
After the streams' first frames, per round and interleaved in this one process, each figure between two events on the context stream (a step is taken at most
once, so ONE fused step — the last frame again, the ego standing — runs untimed before every timed call, of all kinds alike):
    accumulate                    mot_accumulate_scene(batch): the scroll kernel, the splat kernel, and one copy of 52 bytes per slot ahead of them
    the point copy                a device-to-device copy of the bytes the splat kernel reads, 16 N_e (12 of the point, 4 of the id)
    export                        mot_export_scene_grid_dev(batch) into a block of the caller's
    the cell copy                 a device-to-device copy of the export's batch x W^2 x 16 bytes
--lib: another build of the library, e.g. the splat kernel without run merging:
    python -c "import build; build.build(extra_flags=['-DMOT_SCENE_MERGE=0'], out='variants/libmot_hip_nomerge.so')"   (in the package directory)
Reports the medians over the rounds and both calls as multiples of their copies; prints markdown rows for profiles/scene_grid.md. No ratio is fixed in advance."""
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
    ap.add_argument("--lib", default=None, help="a variant build of the library (default: the product)")
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.init()
    mot = _load("mot_amd", os.path.join(ROOT, "3d-lidar-multi-object-tracking_amd", "__init__.py"))
    sdev = _load("mot_amd.synth_dev", os.path.join(ROOT, "tools", "synth", "synth_dev.py"))
    B, W = args.batch, args.size
    stride = ((N_POINTS + 2047) // 2048) * 2048
    v, yaw = sdev.load_ego(args.frames)
    seq, n_seq, _, _ = sdev.SequenceRenderer("cuda").render(list(range(B)), args.frames, N_POINTS, stride, v, yaw)
    res = {"accumulate": [], "point copy": [], "export": [], "cell copy": []}
    with mot.Context(max_points=stride, max_batch=B, max_tracks_total=args.tracks, lib_path=args.lib) as c:
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
        c.synchronize()
        last = args.frames - 1
        ids = torch.empty((B, stride), dtype=torch.int32, device="cuda"); cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
        c.export_point_tracks_dev(B, ids.data_ptr(), stride, cnt.data_ptr()); c.synchronize()
        ne = int(cnt.sum().item())
        src = torch.empty(4 * ne, dtype=torch.int32, device="cuda").fill_(1); dst = torch.empty_like(src)
        cells = torch.empty((B, W * W, 4), dtype=torch.int32, device="cuda"); hdr = torch.empty((B, 8), dtype=torch.int32, device="cuda")
        cells2 = torch.empty_like(cells)
        def point_copy():
            with torch.cuda.stream(stream):
                dst.copy_(src)
        def cell_copy():
            with torch.cuda.stream(stream):
                cells2.copy_(cells)
        export = lambda: c.export_scene_grid_dev(B, cells.data_ptr(), W * W, hdr.data_ptr())
        calls = {"accumulate": lambda: c.accumulate_scene(B), "point copy": point_copy, "export": export, "cell copy": cell_copy}

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
        export(); c.synchronize()
        h = hdr.cpu().numpy().view(mot.SCENE_HEADER_DTYPE).reshape(B)
        ns, nd, no = int(h["n_static"].sum()), int(h["n_dynamic"].sum()), int(h["n_outside"].sum())
        g = cells.cpu().numpy().view(np.uint32)
        occupied = int(((g[:, :, 0] > 0) | (g[:, :, 1] > 0)).sum())
    med = {k: statistics.median(x) for k, x in res.items()}
    spread = {k: (min(x), max(x)) for k, x in res.items()}
    print(f"\n{B} streams x {N_POINTS} points per call, W = {W}, cell {args.cell} m, library {args.lib or 'product'}: {ne} elevated points; the latest step: {ns} static, {nd} dynamic, "
          f"{no} outside the window; {occupied} occupied cells ({100.0 * occupied / (B * W * W):.1f} %); {args.reps} calls per figure, medians (min - max) of {args.rounds} rounds")
    print("| call | us per call | x its copy | TB/s on its own bytes |")
    print("|---|---|---|---|")
    print(f"| device-to-device copy of 16 N_e bytes | {med['point copy']:.0f} ({spread['point copy'][0]:.0f} - {spread['point copy'][1]:.0f}) | 1 | {32.0 * ne / med['point copy'] / 1e6:.2f} |")
    print(f"| mot_accumulate_scene | {med['accumulate']:.0f} ({spread['accumulate'][0]:.0f} - {spread['accumulate'][1]:.0f}) | {med['accumulate'] / med['point copy']:.2f} | "
          f"{16.0 * ne / med['accumulate'] / 1e6:.2f} (16 N_e read) |")
    print(f"| device-to-device copy of batch x W^2 x 16 bytes | {med['cell copy']:.0f} ({spread['cell copy'][0]:.0f} - {spread['cell copy'][1]:.0f}) | 1 | {32.0 * B * W * W / med['cell copy'] / 1e6:.2f} |")
    print(f"| mot_export_scene_grid_dev | {med['export']:.0f} ({spread['export'][0]:.0f} - {spread['export'][1]:.0f}) | {med['export'] / med['cell copy']:.2f} | "
          f"{32.0 * B * W * W / med['export'] / 1e6:.2f} |")


if __name__ == "__main__":
    main()
