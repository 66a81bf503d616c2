"""What MOT_ORDER_ANY costs and buys (mot_time_stage: HIP events, one context, nothing else on the GPU), on the bench's synthetic 120 k-point frames,
B frames per launch, with the points of every frame in one of the bench's three orders:
    python tools/point_order_timing.py --order beam|firing|random [--batch 64] [--rounds 3] [--parent-lib PATH]
Reports the box stage (stage 2), label_stats (30), cluster_gather (31) and the regrouping kernels (35 labels, 36 sort, 37 gather) in microseconds per
launch of B frames: MOT_ORDER_ANY and MOT_ORDER_SCAN of this build and, with --parent-lib (a libmot_hip.so built from the parent commit), that
library's only mode — interleaved round by round in this one process. Prints one markdown table row per library / mode (the median over the rounds).
tools/point_order_timing.sh runs the three orders, each under its own time limit."""
import argparse
import importlib.util
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_POINTS, N_FRAMES = 120000, 2
# mot_time_stage ids. Each id is a self-contained sequence (the library runs what the timed kernel needs before it and what restores the slots
# after it), so the order of this tuple does not matter; stage 2 runs once more at the end of a leg so that the boxes read back are a whole stage's.
SCAN_IDS = (2, 30, 31)
ANY_IDS = (2, 30, 31, 35, 36, 37)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path, submodule_search_locations=[os.path.dirname(path)])
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def parse_args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--order", choices=("beam", "firing", "random"), default="random")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    return ap.parse_args()


def time_leg(mot, lib, order, ids, cloud_ptr, n_points, stride, batch, iters):
    """one context of one library in one mode: {id: microseconds per launch}, and the boxes of the first slots after a whole box stage"""
    kw = {"lib_path": lib} if lib else {}
    with mot.Context(max_points=stride, max_batch=batch, **kw) as c:
        if order is not None:
            c.set_point_order(order)
        c.frames_dev(cloud_ptr, stride * 4, n_points)
        c.synchronize()
        c.time_stage(2, batch, 2)   # warm-up
        times = {k: c.time_stage(k, batch, iters) * 1e3 for k in ids}
        c.time_stage(2, batch, 1)
        try:
            boxes = [c.get_boxes(s)["boxes"].tobytes() for s in range(min(batch, 4))]
        except mot.MotError as e:
            boxes = str(e)
    return times, boxes


def main():
    args = parse_args()
    import torch
    torch.cuda.init()
    pkg = os.path.join(ROOT, "3d-lidar-multi-object-tracking_amd")
    mot = _load("mot_amd", os.path.join(pkg, "__init__.py"))
    sdev = _load("mot_amd.synth_dev", os.path.join(ROOT, "tools", "synth", "synth_dev.py"))
    batch = args.batch
    stride = ((N_POINTS + 2047) // 2048) * 2048
    v, yaw = sdev.load_ego(N_FRAMES)
    seq, n_seq, _, _ = sdev.SequenceRenderer("cuda").render(list(range(batch)), N_FRAMES, N_POINTS, stride, v, yaw, order=args.order)
    legs = [("this build, ANY", None, mot.MOT_ORDER_ANY, ANY_IDS), ("this build, SCAN", None, mot.MOT_ORDER_SCAN, SCAN_IDS)]
    if args.parent_lib:
        legs.append(("parent commit (SCAN)", args.parent_lib, None, SCAN_IDS))
    times = {name: {k: [] for k in ids} for name, _, _, ids in legs}
    boxes = {}
    for _ in range(args.rounds):
        for name, lib, order, ids in legs:
            t, boxes[name] = time_leg(mot, lib, order, ids, seq[1].data_ptr(), n_seq[1], stride, batch, args.iters)
            for k in ids:
                times[name][k].append(t[k])
    same = all(b == boxes[legs[0][0]] for b in boxes.values())
    print(f"order {args.order}, {batch} frames of {N_POINTS} points per launch, {args.rounds} rounds x {args.iters} launches; "
          f"boxes of the first slots equal across the legs: {same}")
    print("| order | library, mode | box stage (2) | label_stats (30) | cluster_gather (31) | regroup labels (35) | sort (36) | gather (37) |")
    print("|---|---|---|---|---|---|---|---|")
    for name, _, _, ids in legs:
        med = {k: statistics.median(x) for k, x in times[name].items()}
        cells = [f"{med[k]:.1f}" if k in med else "-" for k in ANY_IDS]
        print(f"| {args.order} | {name} | " + " | ".join(cells) + " |  (us)", flush=True)


if __name__ == "__main__":
    main()
