"""What mot_set_track_links costs (one context, nothing else on the GPU), on the bench's synthetic street frames in the shape of ONE context of the headline:
512 streams x 120 k points per launch, ground -> cluster -> box -> tracker through mot_frames_dev, inputs resident in HBM.
    python tools/time_track_links.py [--parent-lib PATH] [--batch 512] [--frames 4] [--passes 3] [--rounds 3]
Legs, interleaved round by round in this one process (same rendered frames, a fresh context per leg and round):
    parent commit        --parent-lib: a libmot_hip.so built from the parent commit (it has no links)
    links off            this build as it comes
    links on             mot_set_track_links(1): owner rows in the tracker + the per-point kernel at the end of every call
Reports frames/s per leg (median over the rounds), the off / parent and on / off ratios, and — links on — the per-point kernel alone: microseconds per launch
of `batch` frames (mot_export_point_tracks_dev runs the same kernel into a caller's block; wall clock over back-to-back launches) and the fraction of a
6.29 TB/s copy it reaches on its algorithmic bytes (2 read + 4 written per elevated point). Prints markdown rows for profiles/track_links.md."""
import argparse
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_POINTS = 120000
COPY_BYTES_PER_S = 6.29e12


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path, submodule_search_locations=[os.path.dirname(path)])
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def run_leg(mot, torch, lib, links, seq, n_seq, v, yaw, stride, batch, passes):
    kw = {"lib_path": lib} if lib else {}
    F = len(seq)
    out = {}
    with mot.Context(max_points=stride, max_batch=batch, max_tracks_total=64, **kw) as c:
        if links:
            c.set_track_links(True)
        k = 0

        def one_pass():
            nonlocal k
            for f in range(F):
                ts = 1.0e9 + k * 1.0e5
                c.frames_dev(seq[f].data_ptr(), stride * 4, n_seq[f], run_tracker=True, timestamps=[ts] * batch, ego_v=[float(v[k % len(v)])] * batch, ego_yaw=[float(yaw[k % len(yaw)])] * batch)
                k += 1
        one_pass(); c.synchronize()   # warm-up (and the streams' first frames)
        t0 = time.perf_counter()
        for _ in range(passes):
            one_pass()
        c.synchronize()
        out["fps"] = batch * F * passes / (time.perf_counter() - t0)
        if links:
            ids = torch.empty((batch, stride), dtype=torch.int32, device="cuda"); cnt = torch.zeros(batch, dtype=torch.int32, device="cuda")
            c.export_point_tracks_dev(batch, ids.data_ptr(), stride, cnt.data_ptr()); c.synchronize()
            reps = 20
            t0 = time.perf_counter()
            for _ in range(reps):
                c.export_point_tracks_dev(batch, ids.data_ptr(), stride, cnt.data_ptr())
            c.synchronize()
            out["kernel_us"] = (time.perf_counter() - t0) / reps * 1e6
            out["n_elevated"] = int(cnt.sum().item())
            out["linked"] = float((ids[0, : int(cnt[0].item())] >= 0).float().mean().item())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    mot = _load("mot_amd", os.path.join(ROOT, "3d-lidar-multi-object-tracking_amd", "__init__.py"))
    sdev = _load("mot_amd.synth_dev", os.path.join(ROOT, "tools", "synth", "synth_dev.py"))
    stride = ((N_POINTS + 2047) // 2048) * 2048
    v, yaw = sdev.load_ego(args.frames)
    seq, n_seq, _, _ = sdev.SequenceRenderer("cuda").render(list(range(args.batch)), args.frames, N_POINTS, stride, v, yaw)
    legs = ([("parent commit", args.parent_lib, False)] if args.parent_lib else []) + [("links off", None, False), ("links on", None, True)]
    res = {name: [] for name, _, _ in legs}
    for _ in range(args.rounds):
        for name, lib, links in legs:
            res[name].append(run_leg(mot, torch, lib, links, seq, n_seq, v, yaw, stride, args.batch, args.passes))
            print(name, res[name][-1], flush=True)
    med = {name: statistics.median(r["fps"] for r in rs) for name, rs in res.items()}
    print(f"\n{args.batch} streams x {N_POINTS} points per launch, {args.frames} frames x {args.passes} passes per leg, {args.rounds} rounds (medians)")
    print("| leg | frames/s | ratio |")
    print("|---|---|---|")
    for name, _, _ in legs:
        base = {"parent commit": None, "links off": med.get("parent commit"), "links on": med["links off"]}[name]
        print(f"| {name} | {med[name]:.0f} | " + (f"{med[name] / base:.4f} vs " + ("parent commit" if name == "links off" else "links off") if base else "-") + " |")
    on = res["links on"]
    us = statistics.median(r["kernel_us"] for r in on); ne = on[0]["n_elevated"]
    print(f"\npoint_tracks_kernel alone: {us:.1f} us per launch of {args.batch} frames ({ne} elevated points, {100 * on[0]['linked']:.0f} % of slot 0's linked to a track): "
          f"{6 * ne / (us * 1e-6) / 1e12:.2f} TB/s on its algorithmic bytes = {6 * ne / (us * 1e-6) / COPY_BYTES_PER_S:.3f} of a {COPY_BYTES_PER_S / 1e12:.2f} TB/s copy")


if __name__ == "__main__":
    main()
