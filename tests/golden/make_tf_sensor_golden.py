"""Records tests/golden/tf_to_sensor.npz: 64 (pose, points, images) of the tracking node's change of frame global -> sensor, as the node's own call
sequence answers it (tests/drivers/tf_to_sensor_driver.cpp on oracle/ref_shim: tf broadcast + pcl_ros::transformPointCloud("/velodyne", ...)). The fixture
is how that pin reaches machines without the reference tree (the GPU suite). Also the home of the case generator and of the driver's build, which
tests/test_emu_sensor_tracks.py uses for the 3000-pose comparison.

    python tests/golden/make_tf_sensor_golden.py"""
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
REF = "/root/reference/object_tracking"
SHIM = os.path.join(ROOT, "oracle", "ref_shim")
SRC = os.path.join(TESTS, "drivers", "tf_to_sensor_driver.cpp")
EXE = os.path.join(TESTS, "emu", "bin", "tf_to_sensor_driver")
FLAGS = ["-std=c++14", "-O2", "-ffp-contract=off", "-fno-fast-math", "-w"]   # tests/nodes_build.py's
POINTS = 32


def have_reference() -> bool:
    return os.path.isdir(os.path.join(REF, "tracking", "Eigen"))


def cases(count):
    """poses as tests/test_tf_exact.py draws them: yaw in +-7 plus the special angles, translations within +-300 m; 32 points within +-60 m each"""
    rng = np.random.default_rng(3)
    poses = np.zeros((count, 3)); points = np.zeros((count, POINTS, 3), np.float32)
    for k in range(count):
        yaw = rng.uniform(-7, 7) if k % 5 else rng.choice([0.0, np.pi, -np.pi, np.pi / 2, -np.pi / 2, 3.0, -3.1415926])
        poses[k] = (rng.uniform(-300, 300), rng.uniform(-300, 300), yaw)
        points[k] = rng.uniform(-60, 60, size=(POINTS, 3)).astype(np.float32)
    return poses, points


def build_driver() -> str:
    deps = [SRC, os.path.abspath(__file__)] + [os.path.join(d, f) for d, _, fs in os.walk(SHIM) for f in fs]
    if os.path.exists(EXE) and all(os.path.getmtime(d) <= os.path.getmtime(EXE) for d in deps):
        return EXE
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    r = subprocess.run(["g++"] + FLAGS + ["-I", SHIM, "-I", os.path.join(REF, "tracking"), SRC, "-o", EXE], capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError("building tf_to_sensor_driver failed:\n" + r.stderr[-4000:])
    return EXE


def run_driver(poses, points):
    exe = build_driver()
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([len(poses), points.shape[1]], np.int32).tobytes())
            for pose, pts in zip(poses, points):
                f.write(np.asarray(pose, np.float64).tobytes()); f.write(np.ascontiguousarray(pts, np.float32).tobytes())
        subprocess.run([exe, fin, fout], check=True, timeout=120)
        return np.fromfile(fout, np.float32).reshape(points.shape)


if __name__ == "__main__":
    poses, points = cases(64)
    np.savez(os.path.join(HERE, "tf_to_sensor.npz"), pose=poses, points=points, sensor=run_driver(poses, points))
    print("wrote", os.path.join(HERE, "tf_to_sensor.npz"))
