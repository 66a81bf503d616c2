"""Selects the seeds of the tracker-threshold cases of tests/param_cases.py (case 6) and writes them to tests/golden/param_seeds.json
(integers only). CPU, the C restatement alone; run it after ANY change of TRACK_SETTINGS, TRACK_KINDS or a generator:
    python tests/golden/make_param_seeds.py

A candidate seed is kept for a (setting, generator) pair iff param_cases.track_seed_qualifies says so: the restatement stepped on the
boxes and on the same boxes with one coordinate per frame moved by one fp32 ulp agrees in every discrete output and to 1e-6 relative in
every state on every live track-frame; the setting changes the restatement's answer against the preset's constants on these boxes; tracks
are alive most of the time. Candidates are 3000 .. 3149 in order for every pair; a pair for which none qualifies is left out of the list. The tests assert the rule again on the seed they load,
so a list that drifted from the generators fails loudly."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


CANDIDATES = range(3000, 3150)


def choose(job):
    import oracle_lib as OL
    import param_cases as PC
    preset, over, kind = job
    for seed in CANDIDATES:
        if PC.track_seed_qualifies(OL, preset, over, kind, seed):
            return seed
    return None


def main():
    from multiprocessing import Pool
    import oracle_lib as OL
    import param_cases as PC
    OL.build_oracle()
    jobs = [(preset, over, kind) for preset, over in PC.TRACK_SETTINGS for kind in PC.TRACK_KINDS]
    with Pool(min(16, len(os.sched_getaffinity(0)))) as pool:
        seeds = pool.map(choose, jobs)
    out = {}
    for (preset, over, kind), seed in zip(jobs, seeds):
        print(PC.track_ident(preset, over), kind, seed, flush=True)
        if seed is not None:   # (no candidate qualifies: the pair is not a case — tests/param_cases.py track_pairs)
            out.setdefault(PC.track_ident(preset, over), {})[kind] = seed
    with open(os.path.join(HERE, PC.TRACK_SEEDS), "w") as fh:
        json.dump(out, fh, separators=(",", ":"), sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
