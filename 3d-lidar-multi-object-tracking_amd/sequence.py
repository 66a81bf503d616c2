"""A rosbag-free sequence player: KITTI raw `velodyne_points/data/*.bin` frames and `oxts/data/*.txt`
ego motion through the same per-frame sequence the three reference nodes run (OT/src/groundremove/main.cpp:120,
OT/src/cluster/main.cpp:74,119, OT/tracking/main.cpp:74-166) on a `Context` of this package.

`play` uses the host-buffer stage calls on purpose — it mirrors the nodes one to one; `play_fused` runs the same sequence on the
throughput path (`Context.frames_host`: pipelined uploads, one launch sequence per frame, several streams per call)."""
from __future__ import annotations

import glob
import os

import numpy as np


def load_kitti_bin(path: str) -> np.ndarray:
    """one velodyne scan: float32 x, y, z, reflectance — already the (n, 4) layout of this library"""
    a = np.fromfile(path, dtype=np.float32)
    if a.size % 4:
        raise ValueError(f"{path}: size is not a multiple of 16 bytes")
    return a.reshape(-1, 4)


def load_oxts(path: str) -> tuple[float, float]:
    """(forward velocity vf [m/s], yaw [rad]) of one KITTI oxts record (fields 8 and 5 of dataformat.txt)"""
    f = np.loadtxt(path).reshape(-1)
    return float(f[8]), float(f[5])


def kitti_frames(drive_dir: str):
    """yields (cloud, v, yaw) for every scan of a KITTI raw drive directory (…/2011_09_26_drive_0005_sync)"""
    scans = sorted(glob.glob(os.path.join(drive_dir, "velodyne_points", "data", "*.bin")))
    for s in scans:
        o = os.path.join(drive_dir, "oxts", "data", os.path.splitext(os.path.basename(s))[0] + ".txt")
        v, yaw = load_oxts(o) if os.path.exists(o) else (0.0, 0.0)
        yield load_kitti_bin(s), v, yaw


def boxes_to_global(boxes: np.ndarray, ego: np.ndarray) -> np.ndarray:
    """sensor frame -> the tracker's global frame: rotate by -egoYaw about the ego position (a plain rigid transform; the
    reference asks tf for it, OT/tracking/main.cpp:143-158)"""
    g = np.asarray(boxes, np.float64).copy()
    co, si = np.cos(-ego[2]), np.sin(-ego[2])
    dx, dy = g[..., 0] - ego[0], g[..., 1] - ego[1]
    g[..., 0] = co * dx - si * dy
    g[..., 1] = si * dx + co * dy
    return g.astype(np.float32)


def play_frame(ctx, cloud: np.ndarray, timestamp: float, v: float, yaw: float, slot: int = 0) -> dict:
    """one frame through ground removal -> clustering -> box fitting -> ego pose -> tracker, as the three nodes do"""
    g = ctx.ground_remove(cloud, want_mask=False)
    cl = ctx.cluster(g["elevated"])
    bx = ctx.box_fit(g["elevated"], cl["grid"], cl["num_cluster"])
    ego = ctx.ego_update(timestamp, v, yaw, slot)
    tr = ctx.track_step(boxes_to_global(bx["boxes"], ego), timestamp, slot)
    return dict(n_elevated=len(g["elevated"]), n_ground=len(g["ground"]), num_cluster=cl["num_cluster"], boxes=bx["boxes"], ego=ego, tracks=tr)


def play(ctx, frames, dt_us: float = 1.0e5, t0: float = 1.0e9):
    """frames: iterable of (cloud, v, yaw); timestamps advance by dt_us microseconds (the tracking node's unit)"""
    for k, (cloud, v, yaw) in enumerate(frames):
        yield play_frame(ctx, cloud, t0 + k * dt_us, v, yaw)


def play_fused(ctx, frames, dt_us: float = 1.0e5, t0: float = 1.0e9, slot_count: int = 1, frame: str = "global"):
    """The same sequence on the THROUGHPUT path: one `frames_host` call per frame (pipelined upload from a page-locked staging
    block, ground -> cluster -> box -> tf -> tracker in one launch sequence, nothing but the results comes back). The change of
    frame is the tracking node's own tf chain (mot_api_tracks.hip: tf_velodyne_to_global), not the numpy transform of `play`.

    frames: iterable of (cloud, v, yaw) — or of lists of `slot_count` such triples, one per stream. Yields per frame a list of
    per-stream dicts (boxes in the sensor frame, tracks).

    frame="sensor": each dict also carries `live`, the stream's live tracks relative to its vehicle at this frame (records of
    the package's TRACK_DTYPE in id order, `Context.fetch_tracks_async(frame="sensor")`: what the tracking node draws,
    OT/tracking/main.cpp:180-196). `tracks` stays what it is with the default: every track ever created, global frame."""
    import ctypes as C
    if frame not in ("global", "sensor"):
        raise ValueError(f'frame must be "global" or "sensor", not {frame!r}')
    track_dtype = np.dtype([("id", "i4"), ("track_manage", "i4"), ("is_static", "i4"), ("is_vis", "i4"), ("p", "f4", 3), ("lifetime", "i4"),
                            ("v_yaw", "f8", 2), ("vis_box", "f4", 24)])   # struct mot_track
    stride = ctx.max_points                       # points between the streams of a batch
    hp = C.c_void_p()
    ctx._ck(ctx.lib.mot_host_alloc(C.c_size_t(slot_count * stride * 16), C.byref(hp)))
    try:
        pinned = np.ctypeslib.as_array(C.cast(hp, C.POINTER(C.c_float)), shape=(slot_count, stride, 4))
        for k, fr in enumerate(frames):
            per = fr if isinstance(fr, list) else [fr]
            if len(per) != slot_count:
                raise ValueError(f"frame {k}: {len(per)} streams, expected {slot_count}")
            ctx.wait_uploads()                    # the previous upload has left the staging block
            n = []
            for s, (cloud, _v, _yaw) in enumerate(per):
                a = np.asarray(cloud, np.float32).reshape(-1, 4)
                if len(a) > stride:
                    raise ValueError(f"frame {k}, stream {s}: {len(a)} points, the context holds {stride}")
                pinned[s, : len(a)] = a
                n.append(len(a))
            ts = [t0 + k * dt_us] * slot_count
            ctx.frames_host(hp.value, stride * 4, n, run_tracker=True, timestamps=ts, ego_v=[p[1] for p in per], ego_yaw=[p[2] for p in per])
            out = [dict(boxes=ctx.get_boxes(s)["boxes"], tracks=ctx.get_tracks(s)) for s in range(slot_count)]
            if frame == "sensor":
                T = ctx.max_tracks_total
                rec = np.zeros((slot_count, T), track_dtype); cnt = np.zeros(slot_count, np.int32)
                ctx.fetch_tracks_async(slot_count, rec.ctypes.data, T, cnt.ctypes.data, frame="sensor")
                ctx.synchronize()
                for s in range(slot_count):
                    out[s]["live"] = rec[s, : cnt[s]].copy()
            yield out
    finally:
        ctx.synchronize()
        ctx.lib.mot_host_free(hp)


def _torch_upload(host: np.ndarray):
    import torch
    d = torch.from_numpy(host).cuda()
    return d.data_ptr(), d


def _play_pieces(ctx, frames, dt_us, t0, upload, behind) -> list:
    """the loop play_static_map and play_static_voxel_map share: the drive in pieces of at most `ctx.max_batch` frames, each through sequence_products_dev(scene=True);
    behind(n_frames) reads the piece right behind its call (it synchronises: the upload may go) and returns the piece's dict, which gets `first_frame`"""
    upload = upload or _torch_upload
    frames = list(frames)
    stride = ctx.max_points
    out = []
    for k0 in range(0, len(frames), ctx.max_batch):
        piece = frames[k0: k0 + ctx.max_batch]
        host = np.zeros((len(piece), stride, 4), np.float32)
        n = []
        for k, (cloud, _v, _yaw) in enumerate(piece):
            a = np.asarray(cloud, np.float32).reshape(-1, 4)
            if len(a) > stride:
                raise ValueError(f"frame {k0 + k}: {len(a)} points, the context holds {stride}")
            host[k, : len(a)] = a
            n.append(len(a))
        ptr, keep = upload(host)
        ctx.sequence_products_dev(ptr, stride * 4, n, [t0 + (k0 + k) * dt_us for k in range(len(piece))], [p[1] for p in piece], [p[2] for p in piece], scene=True)
        r = behind(len(piece))
        r["first_frame"] = k0
        out.append(r)
        del keep
    return out


def play_static_map(ctx, frames, dt_us: float = 1.0e5, t0: float = 1.0e9, classes=("known",), frame: str = "global", min_static_hits: int = 1, trail=(1, 2),
                    upload=None) -> list:
    """A recorded drive into its static map on the SEQUENCE path: the drive is cut into pieces of at most `ctx.max_batch` frames, each piece goes through
    `Context.sequence_products_dev(scene=True)` (one asynchronous call: stateless stages batched, tracker steps chained, every frame into stream 0's scene grid) and is
    judged right behind its call with `Context.get_sequence_scene_points`. Needs `set_track_links(True)` and `set_scene_grid(...)` on the context.

    EACH PIECE IS JUDGED AGAINST THE GRID SO FAR: the frames of piece p see every frame of pieces 0..p (their own piece with hindsight), not the pieces behind them.
    A drive that fits one call (`max_batch >= len(frames)`) is judged against the whole drive.

    frames: a sequence of (cloud, v, yaw), clouds (n, 4) float32. upload: host array -> (device pointer, an object that keeps the block alive); default: through torch.
    Returns one `get_sequence_scene_points` dict per piece (totals, segments, xyz, index, classes) with `first_frame` added; with the defaults `xyz` of the pieces,
    concatenated, is the drive's static map in the global frame — movers and their trails cut out."""
    return _play_pieces(ctx, frames, dt_us, t0, upload,
                        lambda n: ctx.get_sequence_scene_points(n, min_static_hits=min_static_hits, trail=trail, classes=classes, frame=frame))


def play_static_voxel_map(ctx, frames, leaf, min_points: int = 1, dt_us: float = 1.0e5, t0: float = 1.0e9, classes=("known",), min_static_hits: int = 1, trail=(1, 2),
                          upload=None) -> list:
    """`play_static_map`'s loop with `Context.get_sequence_scene_voxels` behind each piece: the piece's selected records (global frame) thinned on the device to one
    centroid and one count per occupied voxel of edge `leaf` (a float, or three) of a lattice anchored at the global origin; voxels with fewer than `min_points`
    records are dropped. Needs `set_track_links(True)` and `set_scene_grid(...)` on the context.

    EACH PIECE IS JUDGED AGAINST THE GRID SO FAR, as in `play_static_map`, AND THINNED ON ITS OWN: a voxel that two pieces see appears in both results (the lattice
    is the same from piece to piece, so the cells can be matched). `play_merged_voxel_map` merges the pieces' maps into one on the device; a drive that fits one
    call (`max_batch >= len(frames)`) gives one map.

    Returns one `get_sequence_scene_voxels` dict per piece (xyz, count, header, totals) with `first_frame` added."""
    return _play_pieces(ctx, frames, dt_us, t0, upload,
                        lambda n: ctx.get_sequence_scene_voxels(n, leaf, min_points=min_points, min_static_hits=min_static_hits, trail=trail, classes=classes))


def play_merged_voxel_map(ctx, frames, leaf, min_points: int = 1, dt_us: float = 1.0e5, t0: float = 1.0e9, classes=("known",), min_static_hits: int = 1, trail=(1, 2),
                          upload=None):
    """`play_static_voxel_map`'s loop with every piece thinned at `min_points=1` and the pieces' voxel maps merged into ONE map (`Context.merge_voxel_maps`, on the
    device): a voxel that several pieces see appears once, its count the sum of theirs, its centroid theirs weighted by count; `min_points` is applied by the merge,
    to the summed count. Needs `set_track_links(True)` and `set_scene_grid(...)` on the context. Up to 16 maps go into one merge; a drive of more pieces is merged in
    rounds (the map so far and the next 15 pieces).

    EACH PIECE IS JUDGED AGAINST THE GRID SO FAR, as in `play_static_map`: a drive longer than the grid's window keeps its start this way.

    Returns (one dict: xyz, count, header of the last merge; the list of the pieces' headers with `first_frame`)."""
    pieces = play_static_voxel_map(ctx, frames, leaf, 1, dt_us, t0, classes, min_static_hits, trail, upload)
    heads = [dict(header=p["header"], totals=p["totals"], first_frame=p["first_frame"]) for p in pieces]
    if not pieces:
        return ctx.merge_voxel_maps([dict(xyz=np.zeros((0, 3), np.float32), count=np.zeros(0, np.int32))], leaf, min_points), heads
    # rounds of up to 16 maps; min_points only in the last one (a cell sparse so far may still fill up)
    acc, rest = None, list(pieces)
    while True:
        take = rest[: 16 - (acc is not None)]
        rest = rest[len(take):]
        acc = ctx.merge_voxel_maps(([acc] if acc is not None else []) + take, leaf, 1 if rest else min_points)
        if not rest:
            return acc, heads


def play_against_map(ctx, frames, index, min_count: int = 1, reach: int = 0, dt_us: float = 1.0e5, t0: float = 1.0e9, slot_count: int = 1, upload=None) -> np.ndarray:
    """Yesterday's map, today's drive: the drive played frame by frame with `Context.frames_dev` on slot 0 and every frame judged against a voxel index
    (`Context.index_voxel_maps_dev` -> `Context.export_map_points_dev`, counts alone: no records travel). Needs `set_track_links(True)`; the scene grid is not needed.

    frames: a sequence of (cloud, v, yaw), clouds (n, 4) float32. index: the `MotVoxelIndex` an index call filled, its blocks on the device. upload: host array ->
    (device pointer, an object that keeps the block alive); default: through torch. slot_count: the slots of a call (the context's others get the same frame).
    Returns counts [len(frames), 5] int64: per frame the elevated points per class MAP_OUTSIDE .. MAP_PRESENT — MAP_ABSENT counts what stands where the map
    has nothing. One synchronisation, at the end: the segment tables of all frames stay on the device until then."""
    MAP_CLASSES = 5   # (MOT_MAP_CLASSES of include/mot.h)
    upload = upload or _torch_upload
    frames = list(frames)
    stride = ctx.max_points
    seg_host = np.zeros((max(len(frames), 1), slot_count, MAP_CLASSES, 2), np.int32)
    seg_ptr, seg_keep = upload(seg_host)
    keeps = []
    for k, (cloud, v, yaw) in enumerate(frames):
        a = np.asarray(cloud, np.float32).reshape(-1, 4)
        if len(a) > stride:
            raise ValueError(f"frame {k}: {len(a)} points, the context holds {stride}")
        host = np.zeros((slot_count, stride, 4), np.float32)
        host[:, : len(a)] = a
        ptr, keep = upload(host)
        keeps.append(keep)
        ctx.frames_dev(ptr, stride * 4, [len(a)] * slot_count, run_tracker=True, timestamps=[t0 + k * dt_us] * slot_count, ego_v=[v] * slot_count, ego_yaw=[yaw] * slot_count)
        ctx.export_map_points_dev(slot_count, index, 0, 0, seg_ptr + k * seg_host[0].nbytes, min_count=min_count, reach=reach, classes=0)
    ctx.synchronize()
    if hasattr(seg_keep, "to_host"):
        seg = seg_keep.to_host(seg_host.dtype, seg_host.shape)
    elif hasattr(seg_keep, "cpu"):
        seg = seg_keep.cpu().numpy()
    else:
        seg = np.asarray(seg_keep).reshape(seg_host.shape)
    return seg[: len(frames), 0, :, 1].astype(np.int64)
