"""What merging the voxel maps of a drive's pieces costs (one context at a time, nothing else on the GPU): the drive of tools/time_scene_voxels_sequence.py — ONE
64-beam stream of the bench's synthetic street scene, 154 frames x 120 k points with the drive's ego motion, mot_set_track_links on, mot_set_scene_grid({0.2, 512}),
256 track slots — cut into 2 and into 16 pieces; every piece goes through mot_sequence_products_dev(MOT_SEQ_SCENE) and mot_export_sequence_scene_voxels_dev (mask
KNOWN, min_points 1) at every leaf, its voxels and header staying on the device.
    python tools/time_voxel_merge.py [--frames 154] [--reps 8] [--rounds 3] [--size 512] [--cell 0.2] [--leaves 0.1 0.2] [--pieces 2 16]
Per round and interleaved in this one process, each call between two events on the context stream, per (pieces, leaf):
    input copy            a device-to-device copy of the pieces' voxels, 16 bytes each: the project's yardstick
    merge                 mot_merge_voxel_maps_dev of the pieces' maps (capacity = the piece's voxels, the count read from the export's header on the device),
                          min_points 1, room for every voxel; reduce kernel: cells of at most 64 inputs by one thread, longer ones by a wave (the default)
    merge, waves only     the same with every cell taken by a wave (mot_debug_voxel_merge_cut(0)): the other cut of the reduce kernel
    voxel call            mot_export_sequence_scene_voxels_dev of the LAST piece (still valid behind its sequence call): the call that produced one of the maps
Reports medians (min - max) over the rounds and prints markdown rows for profiles/voxel_merge.md. No ratio is fixed in advance."""
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cell", type=float, default=0.2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--leaves", type=float, nargs="+", default=[0.1, 0.2])
    ap.add_argument("--pieces", type=int, nargs="+", default=[2, 16])
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
    res, facts = {}, {}
    for P in args.pieces:
        per = (F + P - 1) // P
        with mot.Context(max_points=stride, max_batch=per, max_tracks_total=args.tracks) as c:
            c.set_track_links(True)
            c.set_scene_grid(args.cell, args.size)
            stream = torch.cuda.ExternalStream(c.lib.mot_stream(c._h))

            def timed(fn, reps):
                """microseconds per call: `reps` calls, each between two events on the context stream"""
                pairs = []
                for _ in range(reps + 1):   # (the first is the warm-up)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream); fn(stream); b.record(stream)
                    pairs.append((a, b))
                c.synchronize()
                return statistics.mean(a.elapsed_time(b) for a, b in pairs[1:]) * 1e3

            # the pieces' maps: one block of frames * stride voxels per (piece, leaf) while the drive plays, cut down to the stored voxels afterwards
            maps = {leaf: [] for leaf in args.leaves}
            last = 0
            for k0 in range(0, F, per):
                k1 = min(k0 + per, F); last = k1 - k0
                c.sequence_products_dev(seq[k0, 0].data_ptr(), fstride, n0[k0:k1], 1.0e9 + 1e5 * np.arange(k0, k1), ego_v[k0:k1], ego_yaw[k0:k1], scene=True)
                for leaf in args.leaves:
                    big = torch.empty((last * stride, 4), dtype=torch.int32, device="cuda"); hdr = torch.zeros(8, dtype=torch.int32, device="cuda")
                    c.export_sequence_scene_voxels_dev(last, leaf, big.data_ptr(), last * stride, hdr.data_ptr(), 0, classes=KNOWN)
                    c.synchronize()
                    n = int(hdr.cpu().numpy()[5])
                    maps[leaf].append((big[:n].clone(), hdr, n))
                    del big
            for leaf in args.leaves:
                total = sum(n for _, _, n in maps[leaf])
                out = torch.empty((total + 1, 4), dtype=torch.int32, device="cuda"); mh = torch.zeros(8, dtype=torch.int32, device="cuda")
                src = torch.empty(4 * max(total, 1), dtype=torch.int32, device="cuda").fill_(1); dst = torch.empty_like(src)
                vox = torch.empty((last * stride, 4), dtype=torch.int32, device="cuda"); vh = torch.zeros(8, dtype=torch.int32, device="cuda")
                arg = [(b.data_ptr(), h.data_ptr() + 20, n) for b, h, n in maps[leaf]]

                def input_copy(s):
                    with torch.cuda.stream(s):
                        dst.copy_(src)

                def merge(s, cut=64):
                    assert c.lib.mot_debug_voxel_merge_cut(c._h, cut) == 0
                    c.merge_voxel_maps_dev(arg, leaf, out.data_ptr(), total, mh.data_ptr())
                calls = {"input copy": input_copy, "merge": merge, "merge, waves only": lambda s: merge(s, 0),
                         "voxel call": lambda s: c.export_sequence_scene_voxels_dev(last, leaf, vox.data_ptr(), last * stride, vh.data_ptr(), 0, classes=KNOWN)}
                for _ in range(args.rounds):
                    for name, fn in calls.items():
                        res.setdefault((P, leaf, name), []).append(timed(fn, args.reps))
                    print({name: round(res[(P, leaf, name)][-1], 1) for name in calls}, flush=True)
                both = []
                for cut in (64, 0):
                    merge(stream, cut); c.synchronize()
                    both.append((out.cpu().numpy().copy()[:total], mh.cpu().numpy().copy()))
                assert both[0][1].tobytes() == both[1][1].tobytes() and both[0][0][: both[0][1][4]].tobytes() == both[1][0][: both[1][1][4]].tobytes(), "the two cuts differ"
                c.lib.mot_debug_voxel_merge_cut(c._h, 64)
                facts[(P, leaf)] = dict(total=total, header=both[0][1], last_piece=int(vh.cpu().numpy()[3]), frames=last)
                del out, src, dst, vox
    med = {k: statistics.median(x) for k, x in res.items()}
    row = lambda k: f"{med[k]:.0f} ({min(res[k]):.0f} - {max(res[k]):.0f})"
    print(f"\none stream x {F} frames x {N_POINTS} points, W = {args.size}, cell {args.cell} m, mask KNOWN; {args.reps} calls per figure, medians (min - max) of {args.rounds} rounds, us per call")
    print("| pieces | leaf | input voxels | merged voxels | copy of the inputs | merge | x the copy | merge, every cell by a wave | voxel call of the last piece (frames, voxels) | merge / voxel call |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for (P, leaf), f in facts.items():
        k = lambda name: (P, leaf, name)
        print(f"| {P} | {leaf} | {f['total']} | {int(f['header'][2])} | {row(k('input copy'))} | {row(k('merge'))} | {med[k('merge')] / med[k('input copy')]:.1f} | {row(k('merge, waves only'))} | "
              f"{row(k('voxel call'))} ({f['frames']}, {f['last_piece']}) | {med[k('merge')] / med[k('voxel call')]:.2f} |")


if __name__ == "__main__":
    main()
