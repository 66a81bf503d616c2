"""What mot_export_track_model_voxels_dev costs (one context, nothing else on the GPU), on the scene and accumulators of tools/time_track_models.py: the bench's
synthetic street frames in the shape of ONE context of the headline, 512 streams x 120 k points per launch, 64 track slots, K = 4096, O = 16, 16 accumulated steps.
    python tools/time_track_voxels.py [--batch 512] [--frames 16] [--reps 8] [--rounds 3] [--points-per-track 4096] [--obs-per-track 16] [--leaves 0.1 0.25]
After the streams' frames (each followed by mot_accumulate_track_points), per round and interleaved in this one process, each figure between two events on the
context stream:
    raw                           mot_export_track_models_dev(batch) with MOT_MODEL_AXES: the raw export, as it stands
    voxels, leaf L                mot_export_track_model_voxels_dev(batch) with MOT_MODEL_AXES at every leaf: the plan, count, pack and write kernels
    headers, leaf L               the same without a voxel block (d_voxels null): the plan, count and pack kernels
    the copy                      a device-to-device copy of the raw records: 16 bytes each
Reports the medians over the rounds and every voxel call as a multiple of the raw export of the same session. Prints markdown rows for profiles/track_voxels.md.
No ratio is fixed in advance."""
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
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--points-per-track", type=int, default=4096)
    ap.add_argument("--obs-per-track", type=int, default=16)
    ap.add_argument("--tracks", type=int, default=64, help="max_tracks_total")
    ap.add_argument("--leaves", type=float, nargs="+", default=[0.1, 0.25])
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    mot = _load("mot_amd", os.path.join(ROOT, "3d-lidar-multi-object-tracking_amd", "__init__.py"))
    sdev = _load("mot_amd.synth_dev", os.path.join(ROOT, "tools", "synth", "synth_dev.py"))
    B, K, O, T = args.batch, args.points_per_track, args.obs_per_track, args.tracks
    stride = ((N_POINTS + 2047) // 2048) * 2048
    v, yaw = sdev.load_ego(args.frames)
    seq, n_seq, _, _ = sdev.SequenceRenderer("cuda").render(list(range(B)), args.frames, N_POINTS, stride, v, yaw)
    names = ["raw"] + [f"voxels {l:g}" for l in args.leaves] + [f"headers {l:g}" for l in args.leaves] + ["copy"]
    res = {k: [] for k in names}
    with mot.Context(max_points=stride, max_batch=B, max_tracks_total=T) as c:
        c.set_track_links(True)
        c.set_track_accumulation(K, O)
        stream = torch.cuda.ExternalStream(c.lib.mot_stream(c._h))
        for f in range(args.frames):
            c.frames_dev(seq[f].data_ptr(), stride * 4, n_seq[f], run_tracker=True, timestamps=[1.0e9 + f * 1.0e5] * B, ego_v=[float(v[f])] * B, ego_yaw=[float(yaw[f])] * B)
            c.accumulate_track_points(B)
        c.synchronize()
        del seq
        models = torch.empty((B, T, 12), dtype=torch.int32, device="cuda"); cnt = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
        probe = torch.empty((4,), dtype=torch.int32, device="cuda")
        c.export_track_models_dev(B, probe.data_ptr(), 0, models.data_ptr(), cnt.data_ptr()); c.synchronize()   # the true numbers first
        per_slot = int(cnt[:, 1].max().item()); records = int(cnt[:, 1].sum().item()); n_models = int(cnt[:, 0].sum().item())
        n_obs = int(models[:, :, 3].sum().item())
        pts = torch.empty((B, max(per_slot, 1), 4), dtype=torch.int32, device="cuda")
        export = lambda **kw: c.export_track_models_dev(B, pts.data_ptr(), max(per_slot, 1), models.data_ptr(), cnt.data_ptr(), **kw)
        vmodels = torch.empty((B, T, 16), dtype=torch.int32, device="cuda"); vcnt = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
        voxels, vox = {}, {}
        for leaf in args.leaves:   # the true numbers first: a block that holds every slot's voxels
            c.export_track_model_voxels_dev(B, 0, 0, vmodels.data_ptr(), vcnt.data_ptr(), leaf, axes=True); c.synchronize()
            voxels[leaf] = (int(vcnt[:, 1].sum().item()), int(vcnt[:, 1].max().item()), int(vmodels[:, :, 13].sum().item()))
            vox[leaf] = torch.empty((B, max(voxels[leaf][1], 1), 4), dtype=torch.int32, device="cuda")
        src = torch.empty(4 * max(records, 1), dtype=torch.int32, device="cuda").fill_(1); dst = torch.empty_like(src)
        def copy():
            with torch.cuda.stream(stream):
                dst.copy_(src)
        calls = {"raw": lambda: export(axes=True), "copy": copy}
        for leaf in args.leaves:
            calls[f"voxels {leaf:g}"] = lambda leaf=leaf: c.export_track_model_voxels_dev(B, vox[leaf].data_ptr(), vox[leaf].shape[1], vmodels.data_ptr(), vcnt.data_ptr(), leaf, axes=True)
            calls[f"headers {leaf:g}"] = lambda leaf=leaf: c.export_track_model_voxels_dev(B, 0, 0, vmodels.data_ptr(), vcnt.data_ptr(), leaf, axes=True)

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
            for name in names:
                res[name].append(timed(calls[name]))
            print({k: round(x[-1], 1) for k, x in res.items()}, flush=True)
    med = {k: statistics.median(x) for k, x in res.items()}
    spread = {k: (min(x), max(x)) for k, x in res.items()}
    print(f"\n{B} streams, {T} track slots, K = {K}, O = {O}, {args.frames} accumulated steps of {N_POINTS} points: {n_models} models of {records} records "
          f"({records / max(n_models, 1):.0f} per model, at most {per_slot} per stream), {n_obs} logged observations; {args.reps} calls per figure, medians (min - max) of "
          f"{args.rounds} rounds")
    print("| call | voxels (records outside the lattice) | us per call | x the raw export |")
    print("|---|---|---|---|")
    row = lambda what, k, n: print(f"| {what} | {n} | {med[k]:.0f} ({spread[k][0]:.0f} - {spread[k][1]:.0f}) | {med[k] / med['raw']:.2f} |")
    row("device-to-device copy of the raw records (16 bytes each)", "copy", "")
    row("mot_export_track_models_dev, MOT_MODEL_AXES", "raw", "")
    for leaf in args.leaves:
        n = f"{voxels[leaf][0]} ({voxels[leaf][2]})"
        row(f"mot_export_track_model_voxels_dev, MOT_MODEL_AXES, leaf {leaf:g}", f"voxels {leaf:g}", n)
        row(f"... headers only (no voxel block)", f"headers {leaf:g}", n)


if __name__ == "__main__":
    main()
