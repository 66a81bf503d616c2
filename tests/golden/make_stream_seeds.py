"""Selects the seeds of the 9 m streams of tests/tracker_cases.py's many-stream cases (wide_batch, dense_threshold) and writes them to
tests/golden/stream_seeds.json (integers only). CPU, a few minutes; needs the reference build (oracle/_ref) — run it where `make -C oracle ref`
works, after ANY change of a plan:   python tests/golden/make_stream_seeds.py

Why seeds are selected: the 9 m lattice is not well conditioned for every seed (a coasting or freshly born track whose covariance leaves the
rails for a few frames amplifies last-bit differences by decades), and a test built on unselected seeds sits at the edge of the 1e-4 bar with no
device in the picture. A candidate seed is kept for a schedule (box count, late start, resets, repeated timestamp, skipped frames — StreamPlan.key())
iff, replaying EXACTLY that schedule on the C restatement and on the reference's own build side by side,
  * their discrete outputs are equal on every frame,
  * no live track-frame is set aside by the narrow criterion (seq_parity.conditioning), and
  * the two stay within seq_parity.MEASURED_FLOOR = 1e-5 of each other on every state key of every live track-frame,
  * and the live counts are the canonical ones (0 or 1 track after a first frame, the box count after every later one), which
    dense_threshold's planned n_items sequence is computed from,
  * and the stream never needs more track slots than its case gives it (live tracks + the ones that died in the step: a dead track keeps its slot
    until the next step; a seed track that dies beside 64 births needs a 65th slot — the first MI355X run of dense_threshold met MOT_E_CAPACITY there).
Candidates are 1000, 1001, ... in order, each used at most once over all cases. The tests assert ill_conditioned == 0 on these streams at run time,
so a list that drifted from the plans fails loudly. Worst spread between the two builds over all kept seeds of the last run: printed, and
recorded in the JSON under "_worst_spread": 7.5e-9 over the 792 kept seeds (1786 candidates tried; 1e-5 is the limit by construction)."""
import json
import os
import sys
from multiprocessing import Pool

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

FRAMES = {}


def _plan(args):
    import tracker_cases as TC
    nbox, spacing, start, resets, dup, skips = args[0]
    return TC.StreamPlan("candidate", nbox, spacing, args[1], start, resets, dup, skips)


def qualifies(args):
    """(key, seed, frames, track slots) -> (seed, ok, worst spread)"""
    import oracle_lib as OL
    import seq_parity as SP
    pl = _plan(args); frames = args[2]
    p = OL.params(0)
    A = OL.Tracker(p); R = OL.RefTracker(OL.ref()); R.reset()
    bx, ts = pl.boxes(frames), pl.timestamps(frames)
    stats = {}
    fresh, dead_before = True, 0
    try:
        for f in range(frames):
            if f in pl.skips:
                continue
            if f in pl.resets:
                A.reset(); R.reset(); fresh = True
            A.ego_update(ts[f], 0.0, 0.0); R.ego_update(ts[f], 0.0, 0.0)
            a = A.step(bx[f], ts[f], max_tracks=1024); o = R.step(bx[f], ts[f], max_tracks=1024)
            SP.compare_tracks(a, o, A.state, R.state, f, rtol=float("inf"), stats=stats)
            live = int((o["track_manage"] != 0).sum())
            want = (1 if len(bx[f]) > 1 else 0) if fresh else len(bx[f])
            dead = int((o["track_manage"] == 0).sum())
            resident = live + max(0, dead - (0 if fresh else dead_before))   # a track that dies keeps its slot until the next step evicts it
            dead_before = dead
            if live != want or resident > args[3]:
                return args[1], False, 0.0
            fresh = False
    except AssertionError:
        return args[1], False, 0.0
    finally:
        A.close()
    w = stats.get("max_rel_state_err", 0.0)
    return args[1], stats.get("ill_conditioned", 0) == 0 and w <= SP.MEASURED_FLOOR, w


def main():
    import oracle_lib as OL
    import tracker_cases as TC
    OL.build_oracle()
    assert OL.ref() is not None, "the reference build (oracle/_ref) is needed to select seeds"
    cases = {"wide_gpu": (lambda ns: TC.wide_batch_plans("gpu", ns), TC.WIDE_SIZES["gpu"]["frames"], TC.WIDE_SIZES["gpu"]["slots"]),
             "wide_emu": (lambda ns: TC.wide_batch_plans("emu", ns), TC.WIDE_SIZES["emu"]["frames"], TC.WIDE_SIZES["emu"]["slots"]),
             "dense": (TC.dense_threshold_plans, TC.DENSE_PLAN["frames"], 64)}
    out, worst, nxt, tried = {}, 0.0, 1000, 0
    with Pool(min(16, len(os.sched_getaffinity(0)))) as pool:
        for case, (make, frames, slots) in cases.items():
            need = {}
            for pl in make(lambda key: 0):
                if pl.spacing >= 6 and pl.nbox > 0:
                    need[pl.key()] = need.get(pl.key(), 0) + 1
            out[case] = {}
            for key, n in sorted(need.items(), key=repr):
                got = []
                while len(got) < n:
                    batch = list(range(nxt, nxt + max(16, 2 * (n - len(got))))); nxt = batch[-1] + 1; tried += len(batch)
                    for seed, ok, w in pool.map(qualifies, [(key, s, frames, slots) for s in batch]):
                        if ok and len(got) < n:
                            got.append(seed); worst = max(worst, w)
                out[case][repr(key)] = got
                print(case, key, n, "seeds; candidates tried so far", tried, "worst spread", worst, flush=True)
    out["_worst_spread"] = worst
    out["_candidates_tried"] = tried
    with open(os.path.join(HERE, TC.STREAM_SEEDS), "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")


if __name__ == "__main__":
    main()
