"""Times the live-track export kernels on the MI355X with HIP events on the context stream: mot_export_tracks_packed_dev (the existing kernel) against
mot_export_tracks_packed_frame_dev(MOT_FRAME_SENSOR), and the host time of a sensor-frame call (the matrices of every stream + their stream-ordered copy +
the launch). State: `streams` streams with `tracks` live tracks each, built with mot_track_steps_dev. Writes the figures of profiles/sensor_frame_export.md.

    python tools/time_sensor_export.py [streams=512] [tracks=64] [out.json]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest   # noqa: E402  (the package loader of the test suite)
import hiprt      # noqa: E402
import tracker_cases as TC   # noqa: E402


def main():
    streams = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    tracks = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    mot = conftest.load_pkg()
    hip = hiprt.hip()
    rng = np.random.default_rng(1)
    vel = rng.uniform(-1.0, 1.0, size=(streams, tracks, 2))
    with mot.Context(max_points=1024, max_batch=streams, max_tracks_total=tracks + 8) as c:
        stride = tracks * 24
        for f in range(10):
            ts = 1.0e9 + f * 1e5
            d = hiprt.DeviceBuffer(TC.grid_boxes(streams, tracks, f, vel, rng, 9.0).reshape(streams, stride))
            for s in range(streams):
                c.ego_update(ts, 3.0, 0.01 * f + 0.001 * s, s)
            c.track_steps_dev(d.ptr, stride, [tracks] * streams, [ts] * streams)
            c.synchronize(); d.free()
        live = [int((c.get_tracks(s)["track_manage"] != 0).sum()) for s in (0, streams // 2, streams - 1)]
        cap = streams * (tracks + 8)
        nbytes = ((streams * 4 + 15) & ~15) + cap * 144
        blk = hiprt.DeviceBuffer(np.zeros(nbytes, np.uint8))
        stream = C.c_void_p(c.lib.mot_stream(c._h))
        e0, e1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
        calls = {"global": lambda: c.lib.mot_export_tracks_packed_dev(c._h, streams, C.c_void_p(blk.ptr), C.c_long(nbytes)),
                 "sensor": lambda: c.lib.mot_export_tracks_packed_frame_dev(c._h, streams, 1, C.c_void_p(blk.ptr), C.c_long(nbytes))}
        iters, rounds = 200, 7
        res = {k: [] for k in calls}; host = {k: [] for k in calls}
        for k in calls:   # warm-up: code objects, the matrix ring
            for _ in range(20):
                assert calls[k]() == 0
        c.synchronize()
        for r in range(rounds):   # the two alternate inside one process
            for k in calls:
                assert hip.hipEventRecord(e0, stream) == 0
                t0 = time.perf_counter()
                for _ in range(iters):
                    calls[k]()
                t1 = time.perf_counter()
                assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
                ms = C.c_float(0)
                assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
                res[k].append(ms.value * 1000.0 / iters); host[k].append((t1 - t0) * 1e6 / iters)
        head = blk.to_host(np.int32, (streams,))
        out = dict(streams=streams, tracks_per_stream=tracks, live_sampled=live, records=int(head.sum()), bytes_per_call=int(head.sum()) * 144 * 2,
                   iters_per_window=iters, rounds=rounds,
                   us_per_call_device={k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in res.items()},
                   us_per_call_host_enqueue={k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in host.items()},
                   what="device: HIP event pair around 200 back-to-back calls on the context stream (kernel + launch gap; sensor: + the 48 B x streams H2D copy); "
                        "host: wall clock of the same 200 calls' enqueue (sensor - global = the matrices and their copy)")
        blk.free()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 3:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[3])), exist_ok=True)
        open(sys.argv[3], "w").write(line + "\n")


if __name__ == "__main__":
    main()
