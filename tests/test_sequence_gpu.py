"""BASELINE.json configs[3] as written, on the MI355X: 154-frame sequences (ego motion of KITTI drive_0005) of the generator the
bench times (csrc/synth.hip through synth_dev.py), 120 k-point frames — and one stream of configs[4]'s 200 k-point frames —
through the fused device path, EVERY frame against the oracle (tests/seq_parity.py). Both timestamp units.
Reference loop matched: OT/tracking/imm_ukf_jpda.cpp:812-961 (births :972-989), ego fixture OT0/src/imm_ukf_jpda.cpp:65-72."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _run(*argv, timeout=900):
    r = subprocess.run([sys.executable, os.path.join(HERE, "seq_parity_gpu_run.py"), *map(str, argv)], capture_output=True, text=True, timeout=timeout)
    ok = [l for l in r.stdout.splitlines() if l.startswith("sequence parity ok ")]
    assert r.returncode == 0 and ok, (r.stdout[-1500:], r.stderr[-3000:])
    return json.loads(ok[-1][len("sequence parity ok "):])


def test_154_frame_sequences_120k_points_every_frame_vs_oracle(hip_lib):
    st = _run("--points", 120000, "--frames", 154, "--scenes", 0, 1001, "--units", 1e5, 0.1)
    assert st["frames"] == 154 and st["streams"] == 2 and st["points_per_frame"] > 100000
    assert st["max_rel_state_err"] <= 1e-4 and st["above_1e-4_unexplained"] == 0 and st.get("above_bar_well_conditioned", 0) == 0
    assert st["mar_clusters_cross_checked"] > 1000 and st["mar_worst_area_err_units"] <= 6.0 and not st.get("mar_failures")   # every rectangle-branch cluster of both streams
    print("sequence parity:", st)


def test_154_frame_sequence_200k_points_every_frame_vs_oracle(hip_lib):
    st = _run("--points", 200000, "--frames", 154, "--scenes", 7, "--units", 1e5)
    assert st["frames"] == 154 and st["points_per_frame"] > 150000 and st["max_rel_state_err"] <= 1e-4
    assert st["above_1e-4_unexplained"] == 0 and st.get("above_bar_well_conditioned", 0) == 0 and not st.get("mar_failures")


def test_154_frame_dense_scene_measured_conditioning(hip_lib):
    """configs[3]'s "<= 64 tracks": the plaza scene of the bench's dense_scene leg (50-65 live tracks throughout), all 154 frames, 120 k points — under the MEASURED
    conditioning (round-5 review, item 1): a live track-frame is ill-conditioned iff the reference's own builds (the restatement, the -DEIGEN_DONT_VECTORIZE rebuild: fp64
    addition order only) part from libmot_ref.so by more than 1e-5 on it; EVERY other live track-frame within 1e-4, asserted; discrete outputs exact on every frame.
    Reference loop: OT/tracking/imm_ukf_jpda.cpp:812-961, ukf.cpp:630-772."""
    st = _run("--points", 120000, "--frames", 154, "--scenes", 7000, "--units", 1e5, "--scene", "plaza", "--measured", timeout=1500)
    m = st["measured"]
    assert st["frames"] == 154 and st["live_max"] >= 50 and st["tracker_oracle"].startswith("reference build"), st
    assert m["above_bar_well_conditioned"] == 0 and m["max_err_well_conditioned"] <= 1e-4 and m["ill_without_replica"] == 0, m
    assert m["well_conditioned"] >= 0.97 * (m["well_conditioned"] + m["ill_conditioned"]), m   # what is set aside stays a small minority
    print("dense scene, measured conditioning:", m, {k: st.get(k) for k in ("live_max", "tracks_ever", "state_compares", "noise_floor_replicas")})


@pytest.mark.parametrize("order,points,frames,preset", [("firing", 120000, 40, 0), ("random", 120000, 40, 0), ("firing", 200000, 16, 0), ("random", 60000, 24, 1)])
def test_sequence_point_orders(hip_lib, order, points, frames, preset):
    """the same pipeline on azimuth-major (the velodyne driver's `velodyne_points`: OT/src/groundremove/main.cpp:146) and randomly permuted clouds: every
    output against the oracle on the same clouds (box fitting depends on the point order, SURVEY.md H9: the oracle sees the same order) — also at
    configs[4]'s 200 k points and with object_tracking0's constants (preset 1)"""
    st = _run("--points", points, "--frames", frames, "--scenes", 5, "--units", 1e5, "--order", order, "--preset", preset)
    assert st["frames"] == frames and st["point_order"] == order and st["boxes"] > frames // 2


def test_sequence_kitti_preset(hip_lib):
    """preset 1 (object_tracking0's KITTI constants: 200-cell grid, no dilation, L-shape rule without the side test), 40 frames"""
    st = _run("--points", 120000, "--frames", 40, "--scenes", 3, "--units", 1e5, "--preset", 1)
    assert st["frames"] == 40


def test_bench_on_a_kitti_shaped_drive(hip_lib, tmp_path):
    """`bench.py --kitti-dir DIR` (the real-data leg: `data: "kitti"`). With $MOT_KITTI_DIR set it runs on that drive; without (no KITTI data
    in this image) on a KITTI-raw-shaped directory of rendered scans, which exercises the loader, the ragged frame sizes and the line."""
    import numpy as np
    root = os.path.dirname(HERE)
    d = os.environ.get("MOT_KITTI_DIR")
    if not d:
        sys.path.insert(0, HERE)
        from conftest import load_sub
        synth = load_sub("synth")
        d = str(tmp_path / "2011_09_26_drive_0005_sync")
        os.makedirs(os.path.join(d, "velodyne_points", "data")); os.makedirs(os.path.join(d, "oxts", "data"))
        for f in range(6):
            synth.make_cloud(60000 - 501 * f, 3, f).tofile(os.path.join(d, "velodyne_points", "data", f"{f:010d}.bin"))
            ox = np.zeros(30); ox[8] = 3.0 + 0.1 * f; ox[5] = 0.004 * f
            np.savetxt(os.path.join(d, "oxts", "data", f"{f:010d}.txt"), ox[None])
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--kitti-dir", d, "--batch", "8", "--contexts", "2", "--steps", "2", "--warmup", "1", "--full", "--no-aux",
                        "--no-cpu-baseline", "--phase", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["data"] == "kitti" and line["value"] > 0 and line["config"]["kitti"]["frames"] >= 6 and line["all_outputs"]["value"] > 0


def test_bench_plain_line_and_dumped_outputs(hip_lib, tmp_path):
    """a plain `bench.py` run prints the headline alone, timed over --steps steps; `--dump-outputs DIR` writes what the last timed step
    computed, the same for two runs of the same workload (seeded inputs; one and two timed steps)"""
    import numpy as np
    root = os.path.dirname(HERE)
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d, steps in zip(dirs, (1, 2)):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--batch", "8", "--contexts", "2", "--frames", "6", "--steps", str(steps), "--warmup", "1",
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == steps and line["value"] > 0 and line["ms_per_step"] > 0 and line["unit"] == "frames/s" and line["higher_is_better"]
        assert "roofline" not in line and "cpu_baseline" not in line and "all_outputs" not in line
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1])) and "boxes.npy" in names
    for name in names:
        a, b = (np.load(d / name) for d in dirs)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all() and np.array_equal(a, b), name
    assert np.load(dirs[0] / "n_boxes.npy").sum() > 0


def test_sequence_mode_on_the_device(hip_lib):
    """mot_sequence_dev on the MI355X: a rendered 154-frame stream in ONE call against 154 calls of mot_frames_dev — boxes of every frame,
    the per-frame live-track records and the final filter states bit for bit (tests/test_emu_sequence.py is the same check on the emulator)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "seq_mode_gpu_run.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "sequence mode ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
