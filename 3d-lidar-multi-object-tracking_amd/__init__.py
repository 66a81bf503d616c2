"""MI355X-native LiDAR perception hot path — Python host binding over the C-ABI (include/mot.h).

The product is ``libmot_hip.so`` (hand-written HIP for gfx950, built in-tree by ``build.py``); this module is
ctypes plumbing plus thin wrappers named after the reference functions they stand in for
(``groundRemove`` / ``componentClustering`` / ``boxFitting`` / ``getOriginPoints`` / ``immUkfJpdaf`` of
/root/reference/object_tracking). There is no CPU fallback: loading fails loudly when the extension is
missing, and ``Context()`` fails when no GPU is present.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmot_hip.so")

MOT_OK, MOT_E_ARG, MOT_E_CAPACITY, MOT_E_HIP, MOT_E_STATE = 0, 1, 2, 3, 4
MOT_MAX_BOXES_PER_FRAME = 1024   # include/mot.h
MOT_TRACKER_AUTO, MOT_TRACKER_SPLIT, MOT_TRACKER_STREAM = 0, 1, 2   # mot_set_tracker_mode (include/mot.h)
MOT_ORDER_SCAN, MOT_ORDER_ANY = 0, 1   # mot_set_point_order (include/mot.h)
MOT_FRAME_GLOBAL, MOT_FRAME_SENSOR = 0, 1   # mot_export_tracks*_frame_dev, mot_fetch_tracks_frame_async, mot_*_track_points* (include/mot.h)
MOT_TRACK_POINTS_REST = 1   # mot_export_track_points_dev / mot_get_track_points flags (include/mot.h)
PRESET_OBJECT_TRACKING, PRESET_OBJECT_TRACKING0 = 0, 1
MASK_DROPPED, MASK_GROUND, MASK_ELEVATED = 0, 1, 2
NUM_CHANNEL, NUM_BIN = 80, 120


class MotParams(C.Structure):
    """struct mot_params (include/mot.h)"""
    _fields_ = [
        ("r_min", C.c_float), ("r_max", C.c_float), ("t_hmin", C.c_float), ("t_hmax", C.c_float),
        ("t_hdiff", C.c_float), ("h_sensor", C.c_float), ("ground_margin", C.c_double), ("gauss_sigma", C.c_double),
        ("gauss_samples", C.c_int32), ("crop_enable", C.c_int32),
        ("crop_z_min", C.c_float), ("crop_z_max", C.c_float), ("crop_x_min", C.c_float), ("crop_x_max", C.c_float),
        ("crop_y_min", C.c_float), ("crop_y_max", C.c_float),
        ("num_grid", C.c_int32), ("roi_m", C.c_float), ("occ_min_count", C.c_int32), ("dilate", C.c_int32),
        ("pic_scale", C.c_float), ("ram_points", C.c_int32), ("l_slope_dist", C.c_int32), ("l_num_points", C.c_int32),
        ("lshape_side_cond", C.c_int32), ("sensor_height", C.c_float),
        ("t_height_min", C.c_float), ("t_height_max", C.c_float), ("t_width_min", C.c_float), ("t_width_max", C.c_float),
        ("t_len_min", C.c_float), ("t_len_max", C.c_float), ("t_area_max", C.c_float),
        ("t_ratio_min", C.c_float), ("t_ratio_max", C.c_float), ("min_len_ratio", C.c_float), ("t_pt_per_m3", C.c_float),
        ("min_points", C.c_int32),
        ("gamma_g", C.c_double), ("p_g", C.c_double), ("p_d", C.c_double), ("distance_thres", C.c_double),
        ("life_time_thres", C.c_int32), ("seed_box_index", C.c_int32), ("bb_yaw_change_thres", C.c_double),
        ("first_ego_yaw_offset", C.c_double), ("seed_px", C.c_double), ("seed_py", C.c_double),
        ("rng_mapping", C.c_int32), ("max_tracks_ever", C.c_int32),
    ]


class MotTrack(C.Structure):
    """struct mot_track"""
    _fields_ = [("id", C.c_int32), ("track_manage", C.c_int32), ("is_static", C.c_int32), ("is_vis", C.c_int32),
                ("px", C.c_float), ("py", C.c_float), ("pz", C.c_float), ("lifetime", C.c_int32),
                ("v", C.c_double), ("yaw", C.c_double), ("vis_box", C.c_float * 24)]


class MotTrackState(C.Structure):
    """struct mot_track_state"""
    _fields_ = [("x_merge", C.c_double * 5), ("x_cv", C.c_double * 5), ("x_ctrv", C.c_double * 5), ("x_rm", C.c_double * 5),
                ("p_merge", C.c_double * 25), ("p_cv", C.c_double * 25), ("p_ctrv", C.c_double * 25), ("p_rm", C.c_double * 25),
                ("mode_prob", C.c_double * 3), ("z_pred", C.c_double * 6), ("s", C.c_double * 12), ("k", C.c_double * 30),
                ("init_meas", C.c_double * 2), ("dist_from_init", C.c_double), ("best_yaw", C.c_double),
                ("lifetime", C.c_int32), ("track_manage", C.c_int32), ("is_static", C.c_int32), ("is_vis", C.c_int32),
                ("has_best_box", C.c_int32), ("_pad", C.c_int32), ("bbox", C.c_float * 24), ("best_bbox", C.c_float * 24)]


class MotTrackSegment(C.Structure):
    """struct mot_track_segment"""
    _fields_ = [("track_id", C.c_int32), ("first", C.c_int32), ("count", C.c_int32), ("n_boxes", C.c_int32)]


class MotTrackPoint(C.Structure):
    """struct mot_track_point"""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("index", C.c_int32)]


assert C.sizeof(MotTrackSegment) == 16 and C.sizeof(MotTrackPoint) == 16
# the same two records as numpy dtypes
TRACK_SEGMENT_DTYPE = np.dtype([("track_id", "i4"), ("first", "i4"), ("count", "i4"), ("n_boxes", "i4")])
TRACK_POINT_DTYPE = np.dtype([("xyz", "f4", 3), ("index", "i4")])
# struct mot_accum_row / mot_accum_point / mot_accum_obs (per-track accumulators, include/mot.h)
ACCUM_ROW_DTYPE = np.dtype([("track_id", "i4"), ("first_step", "i4"), ("last_step", "i4"), ("obs_total", "i4"), ("total", "u8"), ("reserved", "u8")])
ACCUM_POINT_DTYPE = np.dtype([("xyz", "f4", 3), ("step", "i4")])
ACCUM_OBS_DTYPE = np.dtype([("step", "i4"), ("count", "i4"), ("n_boxes", "i4"), ("track_manage", "i4"), ("px", "f4"), ("py", "f4"), ("is_static", "i4"), ("lifetime", "i4"),
                            ("v", "f8"), ("yaw", "f8")])
# struct mot_track_model and the flags of mot_export_track_models_dev / mot_get_track_models (object-centred track models, include/mot.h)
MOT_MODEL_AXES, MOT_MODEL_CURRENT = 1, 2
TRACK_MODEL_DTYPE = np.dtype([("track_id", "i4"), ("first", "i4"), ("count", "i4"), ("n_obs", "i4"), ("first_step", "i4"), ("last_step", "i4"),
                              ("min", "f4", 3), ("max", "f4", 3)])
# struct mot_track_voxel_model / mot_model_voxel / mot_voxel_params of mot_export_track_model_voxels_dev / mot_get_track_model_voxels (voxel-thinned models, include/mot.h)
MODEL_VOXEL_MAX_K = 4096
VOXEL_MODEL_DTYPE = np.dtype([("track_id", "i4"), ("first", "i4"), ("count", "i4"), ("n_obs", "i4"), ("first_step", "i4"), ("last_step", "i4"),
                              ("min", "f4", 3), ("max", "f4", 3), ("n_records", "i4"), ("n_outside", "i4"), ("n_sparse", "i4"), ("reserved", "i4")])
MODEL_VOXEL_DTYPE = np.dtype([("xyz", "f4", 3), ("count", "i4")])
assert VOXEL_MODEL_DTYPE.itemsize == 64 and MODEL_VOXEL_DTYPE.itemsize == 16
# struct mot_scene_cell / mot_scene_header of mot_export_scene_grid_dev / mot_get_scene_grid (rolling static-scene grid, include/mot.h)
SCENE_CELL_DTYPE = np.dtype([("static_hits", "u4"), ("dynamic_hits", "u4"), ("max_z", "f4"), ("last_seen", "i4")])
SCENE_HEADER_DTYPE = np.dtype([("origin_i", "i4"), ("origin_j", "i4"), ("step", "i4"), ("size", "i4"), ("n_static", "u4"), ("n_dynamic", "u4"), ("n_outside", "u4"), ("cell", "f4")])
assert SCENE_CELL_DTYPE.itemsize == 16 and SCENE_HEADER_DTYPE.itemsize == 32
# the classes of mot_export_scene_points_dev / mot_get_scene_points, struct mot_scene_segment and struct mot_scene_judge_params (a frame's points judged against the grid)
SCENE_UNKNOWN, SCENE_MOVING, SCENE_TRAIL, SCENE_NEW, SCENE_KNOWN, SCENE_CLASSES = 0, 1, 2, 3, 4, 5
SCENE_CLASS_NAMES = ("unknown", "moving", "trail", "new", "known")
SCENE_SEGMENT_DTYPE = np.dtype([("first", "i4"), ("count", "i4")])
assert SCENE_SEGMENT_DTYPE.itemsize == 8
# struct mot_scene_voxel_header of mot_export_sequence_scene_voxels_dev / mot_get_sequence_scene_voxels (voxel-thinned static map of a recorded drive)
SCENE_VOXEL_HEADER_DTYPE = np.dtype([("n_records", "i4"), ("n_beyond", "i4"), ("n_outside", "i4"), ("n_voxels", "i4"), ("n_sparse", "i4"), ("n_stored", "i4"), ("reserved", "i4", 2)])
assert SCENE_VOXEL_HEADER_DTYPE.itemsize == 32
# struct mot_voxel_merge_header / mot_voxel_map_src of mot_merge_voxel_maps_dev / mot_merge_voxel_maps (voxel maps merged into one)
VOXEL_MERGE_MAX_MAPS = 16
VOXEL_MERGE_HEADER_DTYPE = np.dtype([("n_inputs", "i4"), ("n_outside", "i4"), ("n_voxels", "i4"), ("n_sparse", "i4"), ("n_stored", "i4"), ("n_saturated", "i4"), ("reserved", "i4", 2)])
assert VOXEL_MERGE_HEADER_DTYPE.itemsize == 32


class MotSceneJudgeParams(C.Structure):
    """struct mot_scene_judge_params"""
    _fields_ = [("min_static_hits", C.c_uint32), ("trail_num", C.c_uint32), ("trail_den", C.c_uint32)]


def _scene_mask(classes) -> int:
    """None: all five; an int: the bit mask itself; else an iterable of class numbers or names"""
    if classes is None:
        return (1 << SCENE_CLASSES) - 1
    if isinstance(classes, (int, np.integer)):
        return int(classes)
    return sum({1 << (SCENE_CLASS_NAMES.index(k) if isinstance(k, str) else int(k)) for k in classes})


class MotSceneParams(C.Structure):
    """struct mot_scene_params"""
    _fields_ = [("cell", C.c_float), ("size", C.c_int32)]


class MotVoxelParams(C.Structure):
    """struct mot_voxel_params"""
    _fields_ = [("leaf_x", C.c_float), ("leaf_y", C.c_float), ("leaf_z", C.c_float), ("min_points", C.c_int32)]


def voxel_params(leaf, min_points: int = 1) -> MotVoxelParams:
    """leaf: one edge length for the three axes, or three"""
    lx, ly, lz = (leaf, leaf, leaf) if np.isscalar(leaf) else leaf
    return MotVoxelParams(float(lx), float(ly), float(lz), int(min_points))


class MotVoxelMapSrc(C.Structure):
    """struct mot_voxel_map_src"""
    _fields_ = [("voxels", C.c_void_p), ("count", C.c_void_p), ("capacity", C.c_long)]


assert C.sizeof(MotVoxelMapSrc) == 24
# the classes of mot_export_map_points_dev / mot_get_map_points (a frame's points judged against a voxel index); the segments are SCENE_SEGMENT_DTYPE
MAP_OUTSIDE, MAP_MOVING, MAP_SPARSE, MAP_ABSENT, MAP_PRESENT, MAP_CLASSES = 0, 1, 2, 3, 4, 5
MAP_CLASS_NAMES = ("outside", "moving", "sparse", "absent", "present")


class MotVoxelIndex(C.Structure):
    """struct mot_voxel_index: a HOST struct of device pointers (mot_index_voxel_maps_dev fills the leaf in)"""
    _fields_ = [("keys", C.c_void_p), ("counts", C.c_void_p), ("header", C.c_void_p), ("capacity", C.c_long), ("leaf_x", C.c_float), ("leaf_y", C.c_float), ("leaf_z", C.c_float),
                ("reserved", C.c_int32)]


class MotMapJudgeParams(C.Structure):
    """struct mot_map_judge_params"""
    _fields_ = [("min_count", C.c_int32), ("reach", C.c_int32)]


assert C.sizeof(MotVoxelIndex) == 48 and C.sizeof(MotMapJudgeParams) == 8


def voxel_index(d_keys_ptr: int, d_counts_ptr: int, d_header_ptr: int, capacity: int, leaf=None) -> MotVoxelIndex:
    """the descriptor of an index in the caller's device blocks: [capacity] uint64 keys (8-byte aligned), [capacity] int32 counts, a 32-byte header
    (VOXEL_MERGE_HEADER_DTYPE). leaf: only for an index that index_voxel_maps_dev wrote earlier through another descriptor"""
    lx, ly, lz = (0.0, 0.0, 0.0) if leaf is None else ((leaf, leaf, leaf) if np.isscalar(leaf) else leaf)
    return MotVoxelIndex(int(d_keys_ptr) or None, int(d_counts_ptr) or None, int(d_header_ptr) or None, int(capacity), float(lx), float(ly), float(lz), 0)


def _map_mask(classes) -> int:
    """None: all five; an int: the bit mask itself; else an iterable of class numbers or names"""
    if classes is None:
        return (1 << MAP_CLASSES) - 1
    if isinstance(classes, (int, np.integer)):
        return int(classes)
    return sum({1 << (MAP_CLASS_NAMES.index(k) if isinstance(k, str) else int(k)) for k in classes})


class MotAccumView(C.Structure):
    """mirror of struct mot_accum_view (include/mot.h)"""
    _fields_ = [("d_rows", C.c_void_p), ("d_points", C.c_void_p), ("d_obs", C.c_void_p), ("tracks_per_slot", C.c_int32), ("points_per_track", C.c_int32),
                ("obs_per_track", C.c_int32), ("max_batch", C.c_int32)]


class MotError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mot error {code}: {msg}")
        self.code = code


EXPORTS = (
    "mot_abi_version", "mot_params_preset", "mot_create", "mot_destroy", "mot_reset", "mot_last_error",
    "mot_synchronize", "mot_stream", "mot_ground_remove", "mot_cluster", "mot_box_fit", "mot_ego_update",
    "mot_track_step", "mot_track_get_state", "mot_frames_dev", "mot_sequence_dev", "mot_get_ground", "mot_get_clusters",
    "mot_get_boxes", "mot_get_tracks", "mot_export_tracks_dev", "mot_side_params_default", "mot_cluster_products", "mot_cluster_products_host", "mot_box_markers", "mot_decode_pointcloud2_dev", "mot_time_stage",
    "mot_ground_remove_pointcloud2", "mot_box_fit_resident", "mot_frame_pointcloud2",
    "mot_reset_slot", "mot_stream_snapshot_size", "mot_stream_save", "mot_stream_load", "mot_frames_host", "mot_frames_host_xyz", "mot_frames_host_pointcloud2", "mot_wait_uploads", "mot_host_alloc", "mot_host_free", "mot_fetch_tracks_async",
    "mot_track_steps_dev", "mot_profile_kernel", "mot_profile_read", "mot_get_params", "mot_set_fused_outputs", "mot_set_point_order", "mot_set_tracker_mode", "mot_set_trace_ranges", "mot_reset_tracks_slot", "mot_export_tracks_packed_dev", "mot_set_launch_graphs",
    "mot_cluster_node_frame", "mot_ground_node_frame",
    "mot_sensor_pose", "mot_export_tracks_frame_dev", "mot_export_tracks_packed_frame_dev", "mot_fetch_tracks_frame_async", "mot_tracking_node_frame",
    "mot_set_track_links", "mot_get_box_tracks", "mot_get_point_tracks", "mot_export_point_tracks_dev",
    "mot_export_track_points_dev", "mot_get_track_points",
    "mot_set_track_accumulation", "mot_accumulate_track_points", "mot_sequence_accumulate_dev", "mot_track_accumulators_dev", "mot_get_accum_rows", "mot_get_track_accumulated",
    "mot_export_track_models_dev", "mot_get_track_models", "mot_export_track_model_voxels_dev", "mot_get_track_model_voxels",
    "mot_set_scene_grid", "mot_accumulate_scene", "mot_export_scene_grid_dev", "mot_get_scene_grid", "mot_sequence_products_dev",
    "mot_export_scene_points_dev", "mot_get_scene_points", "mot_export_sequence_scene_points_dev", "mot_get_sequence_scene_points",
    "mot_export_sequence_scene_voxels_dev", "mot_get_sequence_scene_voxels", "mot_merge_voxel_maps_dev", "mot_merge_voxel_maps",
    "mot_index_voxel_maps_dev", "mot_export_map_points_dev", "mot_get_map_points",
    "mot_gather_unique_id", "mot_gather_create", "mot_gather_contribute", "mot_gather_result", "mot_gather_synchronize", "mot_gather_destroy", "mot_gather_last_error",
)
ABI_VERSION = 6
OUT_GROUND, OUT_MASK, OUT_LABELS = 1, 2, 4
SEQ_ACCUMULATE, SEQ_SCENE = 1, 2   # mot_sequence_products_dev's product bits

_libs: dict[str, C.CDLL] = {}


def load_library(path: str | None = None) -> C.CDLL:
    """dlopen the HIP extension (no fallback: a missing library is an error)."""
    path = path or LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing — run `python __graft_entry__.py build` (hipcc, gfx950). "
                          "There is no CPU fallback for this library.")
    lib = C.CDLL(path)
    lib.mot_last_error.restype = C.c_char_p
    lib.mot_last_error.argtypes = [C.c_void_p]
    lib.mot_stream.restype = C.c_void_p
    lib.mot_destroy.restype = None
    lib.mot_gather_last_error.restype = C.c_char_p
    lib.mot_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    lib.mot_host_free.argtypes = [C.c_void_p]
    if lib.mot_abi_version() != ABI_VERSION:
        raise ImportError(f"{path}: ABI version {lib.mot_abi_version()}, this binding is for {ABI_VERSION} — rebuild the library")
    _libs[path] = lib
    return lib


def params(preset: int = PRESET_OBJECT_TRACKING, lib: C.CDLL | None = None, **overrides) -> MotParams:
    lib = lib or load_library()
    p = MotParams()
    rc = lib.mot_params_preset(preset, C.byref(p))
    if rc:
        raise MotError(rc, "mot_params_preset")
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


class MotSideParams(C.Structure):
    """mirror of struct mot_side_params (include/mot.h)"""
    _fields_ = [("cell_size", C.c_float), ("cost_width", C.c_int32), ("cost_height", C.c_int32), ("cost_resolution", C.c_double),
                ("cost_offset_x", C.c_double), ("cost_offset_y", C.c_double), ("height_limit", C.c_double),
                ("car_length", C.c_double), ("car_width", C.c_double), ("cost_offset_z", C.c_double)]


class MotClusterFrame(C.Structure):
    """mirror of struct mot_cluster_frame (include/mot.h): counts + views into the context's page-locked block"""
    _fields_ = [("num_cluster", C.c_int32), ("n_clustered", C.c_int32), ("n_obstacles", C.c_int32), ("n_boxes", C.c_int32), ("n_undefined", C.c_int32),
                ("cost_cells", C.c_int32), ("clustered_xyzw", C.POINTER(C.c_float)), ("obstacles_xyzc", C.POINTER(C.c_float)), ("cost_map", C.POINTER(C.c_int32)),
                ("boxes", C.POINTER(C.c_float)), ("box_cluster", C.POINTER(C.c_int32)), ("centroid_extent", C.POINTER(C.c_float))]


class MotTrackingFrame(C.Structure):
    """mirror of struct mot_tracking_frame (include/mot.h): the ego origin, counts and a view of the live records in the sensor frame"""
    _fields_ = [("origin6", C.c_double * 6), ("n_live", C.c_int32), ("n_ever", C.c_int32), ("tracks", C.POINTER(MotTrack))]


# struct mot_track as a numpy record (144 bytes)
TRACK_DTYPE = np.dtype([("id", "i4"), ("track_manage", "i4"), ("is_static", "i4"), ("is_vis", "i4"), ("p", "f4", 3), ("lifetime", "i4"),
                        ("v_yaw", "f8", 2), ("vis_box", "f4", 24)])


def _frame(frame) -> int:
    """"global" / "sensor" (or MOT_FRAME_GLOBAL / MOT_FRAME_SENSOR) -> the enum of include/mot.h"""
    if frame in ("global", MOT_FRAME_GLOBAL):
        return MOT_FRAME_GLOBAL
    if frame in ("sensor", MOT_FRAME_SENSOR):
        return MOT_FRAME_SENSOR
    raise ValueError(f'frame must be "global" or "sensor", not {frame!r}')


def _pts(a) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError("points must be (n, 4) float32: x, y, z, w")
    return a


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Context:
    """One mot_ctx: ``max_batch`` independent sensor-stream slots on one GPU, one HIP stream."""

    def __init__(self, p: MotParams | None = None, device: int = 0, max_points: int = 131072, max_batch: int = 1,
                 max_tracks_total: int = 4096, lib_path: str | None = None):
        self.lib = load_library(lib_path)
        self.params = p if p is not None else params(lib=self.lib)
        self.max_points, self.max_batch, self.max_tracks_total = max_points, max_batch, max_tracks_total
        h = C.c_void_p()
        rc = self.lib.mot_create(C.byref(self.params), device, max_points, max_batch, max_tracks_total, C.byref(h))
        if rc:
            why = self.lib.mot_last_error(None)
            raise MotError(rc, "mot_create failed (no GPU / bad arguments); this library has no CPU fallback: " + (why.decode(errors="replace") if why else ""))
        self._h = h

    # ------------------------------------------------------------------ plumbing
    def close(self):
        if getattr(self, "_h", None):
            self.lib.mot_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, rc):
        if rc:
            raise MotError(rc, (self.lib.mot_last_error(self._h) or b"").decode())

    def synchronize(self):
        self._ck(self.lib.mot_synchronize(self._h))

    def reset(self):
        self._ck(self.lib.mot_reset(self._h))

    def reset_slot(self, slot: int):
        self._ck(self.lib.mot_reset_slot(self._h, slot))

    def reset_tracks_slot(self, slot: int):
        """forget the tracks of one stream, keep its ego pose (the origin of its global frame)"""
        self._ck(self.lib.mot_reset_tracks_slot(self._h, slot))

    def stream_save(self, slot: int = 0) -> bytes:
        """the tracker state of one stream as a relocatable block (mot_stream_save): load it into any slot of a context with the
        same max_tracks_total and the stream continues bit for bit"""
        cap = C.c_size_t(0)
        self._ck(self.lib.mot_stream_snapshot_size(self._h, C.byref(cap)))
        buf = (C.c_char * cap.value)(); n = C.c_size_t(0)
        self._ck(self.lib.mot_stream_save(self._h, slot, buf, cap, C.byref(n)))
        return bytes(buf[: n.value])

    def stream_load(self, slot: int, blob: bytes):
        self._ck(self.lib.mot_stream_load(self._h, slot, blob, C.c_size_t(len(blob))))

    def set_launch_graphs(self, on: bool = True):
        """send the fused entry points' launch sequence as one hipGraph launch (per-frame latency path; default off)"""
        self._ck(self.lib.mot_set_launch_graphs(self._h, int(on)))

    def set_trace_ranges(self, on: bool = True):
        """roctx ranges "mot:ground / cluster / box / tracker" around the stages of the fused entry points (rocprofv3 --marker-trace)"""
        self._ck(self.lib.mot_set_trace_ranges(self._h, int(on)))

    def set_tracker_mode(self, mode: int):
        """0 auto (by the number of streams per call), 1 split (four launches, tracks of all streams over the whole chip), 2 stream (one launch, a workgroup per stream)"""
        self._ck(self.lib.mot_set_tracker_mode(self._h, mode))

    def set_fused_outputs(self, flags: int):
        """which by-products of the ground stage the fused entry points write (OUT_GROUND | OUT_MASK | OUT_LABELS; default 0: on demand)"""
        self._ck(self.lib.mot_set_fused_outputs(self._h, flags))

    def set_point_order(self, order: int):
        """MOT_ORDER_SCAN (default) or MOT_ORDER_ANY: clouds in no point order — the box stage regroups the elevated points by cluster on the device
        first; same results, every output in input order, no frame refused for its (tile, cluster) groups"""
        self._ck(self.lib.mot_set_point_order(self._h, int(order)))

    def set_track_links(self, on: bool = True):
        """keep the tracker's box -> track association per step and compose the per-point track ids at the end of every fused call with the tracker
        (mot_set_track_links; default off): get_box_tracks, get_point_tracks, export_point_tracks_dev"""
        self._ck(self.lib.mot_set_track_links(self._h, int(on)))

    def get_box_tracks(self, slot: int = 0, max_boxes: int = 1024) -> np.ndarray:
        """id of the track that owns every box of the slot's last tracker step, in that step's box order (-1: none)"""
        out = np.full(max_boxes, -1, np.int32); nb = C.c_int(0)
        self._ck(self.lib.mot_get_box_tracks(self._h, slot, _vp(out), max_boxes, C.byref(nb)))
        return out[: nb.value].copy()

    def get_point_tracks(self, slot: int = 0, capacity: int | None = None) -> np.ndarray:
        """track id of every elevated point of the slot's last fused frame, in the elevated cloud's input order (-1: none)"""
        cap = self.max_points if capacity is None else capacity
        out = np.full(cap, -1, np.int32); ne = C.c_int(0)
        self._ck(self.lib.mot_get_point_tracks(self._h, slot, _vp(out), cap, C.byref(ne)))
        return out[: ne.value].copy()

    def export_point_tracks_dev(self, batch: int, d_ids_ptr: int, stride: int, d_counts_ptr: int):
        """the per-point track ids of slots 0..batch-1 -> caller's device block d_ids[b * stride + i] and d_counts[b] (asynchronous)"""
        self._ck(self.lib.mot_export_point_tracks_dev(self._h, batch, C.c_void_p(d_ids_ptr), C.c_long(stride), C.c_void_p(d_counts_ptr)))

    def get_track_points(self, slot: int = 0, rest: bool = False, frame=MOT_FRAME_SENSOR, point_capacity: int | None = None, max_segments: int = MOT_MAX_BOXES_PER_FRAME + 1):
        """the slot's elevated points stably partitioned by owning track (mot_get_track_points): xyz [n, 3] (sensor frame: the elevated points' bits; "global":
        under the matrix the slot's boxes took), index [n] (position in the elevated cloud's input order), and per segment track_id (ascending; -1: the rest
        segment, with rest=True), first, count, n_boxes"""
        cap = self.max_points if point_capacity is None else point_capacity
        pts = np.zeros(max(cap, 1), TRACK_POINT_DTYPE); seg = np.zeros(max(max_segments, 1), TRACK_SEGMENT_DTYPE); npts, nseg = C.c_int(0), C.c_int(0)
        self._ck(self.lib.mot_get_track_points(self._h, slot, MOT_TRACK_POINTS_REST if rest else 0, _frame(frame), _vp(pts), cap, _vp(seg), max_segments, C.byref(npts), C.byref(nseg)))
        pts, seg = pts[: npts.value], seg[: nseg.value]
        return dict(xyz=pts["xyz"].copy(), index=pts["index"].copy(), track_id=seg["track_id"].copy(), first=seg["first"].copy(), count=seg["count"].copy(), n_boxes=seg["n_boxes"].copy())

    def export_track_points_dev(self, batch: int, d_points_ptr: int, point_stride: int, d_segments_ptr: int, max_segments: int, d_counts_ptr: int, rest: bool = False,
                                frame=MOT_FRAME_SENSOR):
        """the same for slots 0..batch-1 -> caller's device blocks: 16-byte records d_points[b * point_stride + i] and d_segments[b * max_segments + k], the true
        numbers of segments and records in d_counts[2 b], d_counts[2 b + 1] (asynchronous)"""
        self._ck(self.lib.mot_export_track_points_dev(self._h, batch, MOT_TRACK_POINTS_REST if rest else 0, _frame(frame), C.c_void_p(d_points_ptr), C.c_long(point_stride),
                                                      C.c_void_p(d_segments_ptr), int(max_segments), C.c_void_p(d_counts_ptr)))

    def set_track_accumulation(self, points_per_track: int, obs_per_track: int = 0):
        """per-track accumulators (mot_set_track_accumulation): a ring of points_per_track points (a power of two in [64, 2^20]; 0: off) and of obs_per_track
        observations (0 or a power of two up to 4096) per track slot of every stream; needs set_track_links"""
        self._ck(self.lib.mot_set_track_accumulation(self._h, int(points_per_track), int(obs_per_track)))

    def accumulate_track_points(self, batch: int):
        """append the latest fused step of slots 0..batch-1 to the tracks' accumulators (asynchronous; once per step)"""
        self._ck(self.lib.mot_accumulate_track_points(self._h, int(batch)))

    def track_accumulators_dev(self) -> dict:
        """the accumulators' device pointers and geometry (mot_track_accumulators_dev): d_rows, d_points, d_obs (0 when obs_per_track is 0), tracks_per_slot,
        points_per_track, obs_per_track, max_batch"""
        v = MotAccumView()
        self._ck(self.lib.mot_track_accumulators_dev(self._h, C.byref(v)))
        return dict(d_rows=v.d_rows or 0, d_points=v.d_points or 0, d_obs=v.d_obs or 0, tracks_per_slot=v.tracks_per_slot, points_per_track=v.points_per_track,
                    obs_per_track=v.obs_per_track, max_batch=v.max_batch)

    def get_accum_rows(self, slot: int = 0) -> np.ndarray:
        """the slot's accumulator rows, one per track slot (ACCUM_ROW_DTYPE; track_id -1: empty)"""
        rows = np.zeros(self.max_tracks_total, ACCUM_ROW_DTYPE); n = C.c_int(0)
        self._ck(self.lib.mot_get_accum_rows(self._h, slot, _vp(rows), len(rows), C.byref(n)))
        return rows[: n.value]

    def get_track_accumulated(self, slot: int, track_id: int) -> dict:
        """what the slot's accumulator holds of one track, oldest first (mot_get_track_accumulated): row (an ACCUM_ROW_DTYPE record), xyz [n, 3] (global frame),
        step [n], obs (ACCUM_OBS_DTYPE records)"""
        v = self.track_accumulators_dev()
        row = np.zeros(1, ACCUM_ROW_DTYPE); pts = np.zeros(v["points_per_track"], ACCUM_POINT_DTYPE); obs = np.zeros(max(v["obs_per_track"], 1), ACCUM_OBS_DTYPE)
        npts, nobs = C.c_int(0), C.c_int(0)
        self._ck(self.lib.mot_get_track_accumulated(self._h, slot, int(track_id), _vp(row), _vp(pts), len(pts), C.byref(npts), _vp(obs), len(obs), C.byref(nobs)))
        pts = pts[: npts.value]
        return dict(row=row[0].copy(), xyz=pts["xyz"].copy(), step=pts["step"].copy(), obs=obs[: nobs.value].copy())

    def export_track_models_dev(self, batch: int, d_points_ptr: int, point_stride: int, d_models_ptr: int, d_counts_ptr: int, axes: bool = False, current: bool = False):
        """object-centred track models of slots 0..batch-1 from the accumulators -> caller's device blocks (mot_export_track_models_dev): 16-byte records
        d_points[b * point_stride + i] (x', y' relative to the track's position of the point's step — axes: in the object's axes of that step — z and step as
        accumulated), 48-byte headers d_models[b * max_tracks_total + r] (TRACK_MODEL_DTYPE) and the true numbers d_counts[b] = (non-empty models, records).
        current: only the tracks the latest accumulate call appended to. Asynchronous on the context stream"""
        flags = (MOT_MODEL_AXES if axes else 0) | (MOT_MODEL_CURRENT if current else 0)
        self._ck(self.lib.mot_export_track_models_dev(self._h, int(batch), flags, C.c_void_p(d_points_ptr), C.c_long(point_stride), C.c_void_p(d_models_ptr), C.c_void_p(d_counts_ptr)))

    def get_track_models(self, slot: int, axes: bool = False, current: bool = False) -> dict:
        """the same for one slot, on the host (mot_get_track_models): models (TRACK_MODEL_DTYPE, one per track slot; track_id -1: none), xyz [n, 3] and step [n]
        (the models' records back to back: model m owns [m.first, m.first + m.count))"""
        flags = (MOT_MODEL_AXES if axes else 0) | (MOT_MODEL_CURRENT if current else 0)
        models = np.zeros(self.max_tracks_total, TRACK_MODEL_DTYPE); nm, npts = C.c_int(0), C.c_int(0)
        self._ck(self.lib.mot_get_track_models(self._h, int(slot), flags, None, 0, C.byref(nm), None, 0, C.byref(npts)))   # the counts alone
        pts = np.zeros(max(npts.value, 1), ACCUM_POINT_DTYPE)
        self._ck(self.lib.mot_get_track_models(self._h, int(slot), flags, _vp(models), len(models), C.byref(nm), _vp(pts), len(pts), C.byref(npts)))
        pts = pts[: npts.value]
        return dict(models=models[: nm.value].copy(), xyz=pts["xyz"].copy(), step=pts["step"].copy())

    def export_track_model_voxels_dev(self, batch: int, d_voxels_ptr: int, voxel_stride: int, d_models_ptr: int, d_counts_ptr: int, leaf, min_points: int = 1,
                                      axes: bool = False, current: bool = False):
        """the same models, one record per occupied voxel of edge `leaf` (a float, or three) -> caller's device blocks (mot_export_track_model_voxels_dev): 16-byte
        voxels d_voxels[b * voxel_stride + i] (MODEL_VOXEL_DTYPE: the centroid of the cell's records and their number, in ascending (i_z, i_y, i_x)), 64-byte
        headers d_models[b * max_tracks_total + r] (VOXEL_MODEL_DTYPE) and the true numbers d_counts[b] = (models, voxels). min_points: voxels with fewer records
        are dropped. d_voxels_ptr 0 with voxel_stride 0: headers only. Asynchronous on the context stream"""
        flags = (MOT_MODEL_AXES if axes else 0) | (MOT_MODEL_CURRENT if current else 0)
        p = voxel_params(leaf, min_points)
        self._ck(self.lib.mot_export_track_model_voxels_dev(self._h, int(batch), flags, C.byref(p), C.c_void_p(d_voxels_ptr or None), C.c_long(voxel_stride),
                                                            C.c_void_p(d_models_ptr), C.c_void_p(d_counts_ptr)))

    def get_track_model_voxels(self, slot: int, leaf, min_points: int = 1, axes: bool = False, current: bool = False) -> dict:
        """the same for one slot, on the host (mot_get_track_model_voxels): models (VOXEL_MODEL_DTYPE, one per track slot; track_id -1: none), xyz [n, 3] and
        count [n] (the models' voxels back to back: model m owns [m.first, m.first + m.count))"""
        flags = (MOT_MODEL_AXES if axes else 0) | (MOT_MODEL_CURRENT if current else 0)
        p = voxel_params(leaf, min_points)
        models = np.zeros(self.max_tracks_total, VOXEL_MODEL_DTYPE); nm, nv = C.c_int(0), C.c_int(0)
        self._ck(self.lib.mot_get_track_model_voxels(self._h, int(slot), flags, C.byref(p), None, 0, C.byref(nm), None, 0, C.byref(nv)))   # the counts alone
        vox = np.zeros(max(nv.value, 1), MODEL_VOXEL_DTYPE)
        self._ck(self.lib.mot_get_track_model_voxels(self._h, int(slot), flags, C.byref(p), _vp(models), len(models), C.byref(nm), _vp(vox), len(vox), C.byref(nv)))
        vox = vox[: nv.value]
        return dict(models=models[: nm.value].copy(), xyz=vox["xyz"].copy(), count=vox["count"].copy())

    def set_scene_grid(self, cell, size: int | None = None):
        """rolling static-scene grid per stream (mot_set_scene_grid): `cell` metres per cell in [0.05, 10], `size` cells per side, a power of two in [64, 2048];
        set_scene_grid(None): off, memory freed. Needs set_track_links"""
        if cell is None:
            self._ck(self.lib.mot_set_scene_grid(self._h, None))
            self._scene_size = 0
            return
        p = MotSceneParams(float(cell), int(size))
        self._ck(self.lib.mot_set_scene_grid(self._h, C.byref(p)))
        self._scene_size = int(size)

    def accumulate_scene(self, batch: int):
        """take the latest fused step of slots 0..batch-1 into their scene grids (asynchronous; once per step): points without owner and points of static-flagged
        tracks as static hits, every other owned point as a dynamic hit"""
        self._ck(self.lib.mot_accumulate_scene(self._h, int(batch)))

    def export_scene_grid_dev(self, batch: int, d_cells_ptr: int, cell_stride: int, d_headers_ptr: int):
        """the grids of slots 0..batch-1, unrolled -> caller's device blocks (mot_export_scene_grid_dev): 16-byte cells d_cells[b * cell_stride + v * size + u]
        (SCENE_CELL_DTYPE; window offset (u, v) = global cell (origin_i + u, origin_j + v)) and 32-byte headers d_headers[b] (SCENE_HEADER_DTYPE). Asynchronous"""
        self._ck(self.lib.mot_export_scene_grid_dev(self._h, int(batch), C.c_void_p(d_cells_ptr or None), C.c_long(cell_stride), C.c_void_p(d_headers_ptr or None)))

    def export_scene_points_dev(self, batch: int, d_points_ptr: int, point_stride: int, d_segments_ptr: int, d_classes_ptr: int = 0, class_stride: int = 0,
                                min_static_hits: int = 1, trail=(1, 2), classes=None, frame=MOT_FRAME_GLOBAL):
        """the elevated points of slots 0..batch-1 judged against their scene grids and partitioned by class (mot_export_scene_points_dev) -> caller's device blocks:
        16-byte records d_points[b * point_stride + i] (the classes of `classes`, ascending, each in input order), 8-byte segments d_segments[b * 5 + k] = {first,
        count} (SCENE_SEGMENT_DTYPE; the true count of every class, first = -1 outside the mask) and, if given, one class byte per elevated point
        d_classes[b * class_stride + i]. trail = (num, den). Reads the grid; asynchronous"""
        p = MotSceneJudgeParams(int(min_static_hits), int(trail[0]), int(trail[1]))
        self._ck(self.lib.mot_export_scene_points_dev(self._h, int(batch), C.byref(p), _scene_mask(classes), _frame(frame), C.c_void_p(d_points_ptr or None), C.c_long(point_stride),
                                                      C.c_void_p(d_segments_ptr or None), C.c_void_p(d_classes_ptr or None), C.c_long(class_stride)))

    def get_scene_points(self, slot: int = 0, min_static_hits: int = 1, trail=(1, 2), classes=None, frame=MOT_FRAME_GLOBAL) -> dict:
        """one slot's elevated points judged against its scene grid (mot_get_scene_points): segments [5] (SCENE_SEGMENT_DTYPE: first, count per class SCENE_UNKNOWN ..
        SCENE_KNOWN; first = -1 for a class outside `classes`), xyz [n, 3] and index [n] of the selected classes back to back, classes [n_elevated] (uint8, input order)"""
        p = MotSceneJudgeParams(int(min_static_hits), int(trail[0]), int(trail[1]))
        cap = self.max_points
        pts = np.zeros(max(cap, 1), TRACK_POINT_DTYPE); seg = np.zeros(SCENE_CLASSES, SCENE_SEGMENT_DTYPE); cls = np.zeros(max(cap, 1), np.uint8); npts, ne = C.c_int(0), C.c_int(0)
        self._ck(self.lib.mot_get_scene_points(self._h, int(slot), C.byref(p), _scene_mask(classes), _frame(frame), _vp(pts), cap, C.byref(npts), _vp(seg), _vp(cls), cap, C.byref(ne)))
        pts = pts[: npts.value]
        return dict(segments=seg, xyz=pts["xyz"].copy(), index=pts["index"].copy(), classes=cls[: ne.value].copy())

    def export_sequence_scene_points_dev(self, frames: int, d_points_ptr: int, point_capacity: int, d_segments_ptr: int, d_totals_ptr: int, d_classes_ptr: int = 0,
                                         class_stride: int = 0, min_static_hits: int = 1, trail=(1, 2), classes=None, frame=MOT_FRAME_GLOBAL):
        """frames 0..frames-1 of the latest sequence_products_dev(scene=True) call judged against slot 0's grid as the whole drive left it
        (mot_export_sequence_scene_points_dev) -> caller's device blocks: ONE block of 16-byte records for the drive, class-major (the classes of `classes` ascending,
        inside a class the frames ascending, inside a frame input order), 8-byte d_totals[c] = {first, count} (the drive's run of class c) and d_segments[k * 5 + c]
        (frame k's part of it, first absolute; SCENE_SEGMENT_DTYPE, first = -1 outside the mask, true counts) and, if given, class bytes d_classes[k * class_stride + i].
        With classes=("known",) and frame="global" the records are the drive's static map. Reads the grid; asynchronous"""
        p = MotSceneJudgeParams(int(min_static_hits), int(trail[0]), int(trail[1]))
        self._ck(self.lib.mot_export_sequence_scene_points_dev(self._h, int(frames), C.byref(p), _scene_mask(classes), _frame(frame), C.c_void_p(d_points_ptr or None),
                                                               C.c_long(point_capacity), C.c_void_p(d_segments_ptr or None), C.c_void_p(d_totals_ptr or None),
                                                               C.c_void_p(d_classes_ptr or None), C.c_long(class_stride)))

    def get_sequence_scene_points(self, frames: int, min_static_hits: int = 1, trail=(1, 2), classes=None, frame=MOT_FRAME_GLOBAL, with_classes: bool = True) -> dict:
        """the same on the host (mot_get_sequence_scene_points; two calls: the counts, then the records): totals [5] and segments [frames, 5] (SCENE_SEGMENT_DTYPE),
        xyz [n, 3] and index [n] of the selected classes, class-major over the drive, classes: a list of `frames` uint8 arrays (input order; None without with_classes)"""
        p = MotSceneJudgeParams(int(min_static_hits), int(trail[0]), int(trail[1]))
        mask, fr, F = _scene_mask(classes), _frame(frame), int(frames)
        seg = np.zeros((max(F, 1), SCENE_CLASSES), SCENE_SEGMENT_DTYPE); tot = np.zeros(SCENE_CLASSES, SCENE_SEGMENT_DTYPE); n = C.c_long(0)
        self._ck(self.lib.mot_get_sequence_scene_points(self._h, F, C.byref(p), mask, fr, None, C.c_long(0), C.byref(n), _vp(seg), _vp(tot), None, C.c_long(0)))
        elevated = seg["count"].sum(axis=1)
        stride = max(int(elevated.max()), 1)
        pts = np.zeros(max(n.value, 1), TRACK_POINT_DTYPE); cls = np.zeros((F, stride), np.uint8) if with_classes else None
        self._ck(self.lib.mot_get_sequence_scene_points(self._h, F, C.byref(p), mask, fr, _vp(pts), C.c_long(n.value), C.byref(n), _vp(seg), _vp(tot), _vp(cls), C.c_long(stride)))
        pts = pts[: n.value]
        return dict(totals=tot, segments=seg[:F], xyz=pts["xyz"].copy(), index=pts["index"].copy(),
                    classes=[cls[k, : int(elevated[k])].copy() for k in range(F)] if with_classes else None)

    def export_sequence_scene_voxels_dev(self, frames: int, leaf, d_voxels_ptr: int, voxel_capacity: int, d_header_ptr: int, d_totals_ptr: int = 0, min_points: int = 1,
                                         min_static_hits: int = 1, trail=(1, 2), classes=("known",), record_capacity=None):
        """the records export_sequence_scene_points_dev(frame="global") would give for `classes`, thinned on the device to one record per occupied voxel of edge `leaf`
        (a float, or three) of a lattice anchored at the global origin (mot_export_sequence_scene_voxels_dev) -> caller's device blocks: 16-byte voxels
        (MODEL_VOXEL_DTYPE: the centroid of the cell's records and their number, in ascending (i_z, i_y, i_x); voxels with fewer than min_points records are dropped),
        the 32-byte header (SCENE_VOXEL_HEADER_DTYPE) and, if given, d_totals[c] = {first, count} of the judge call. record_capacity: the records that take part at
        the most (None: frames * max_points); the library's scratch grows to 40 bytes a record of it. Reads the grid; asynchronous"""
        p = MotSceneJudgeParams(int(min_static_hits), int(trail[0]), int(trail[1])); v = voxel_params(leaf, min_points)
        cap = int(frames) * self.max_points if record_capacity is None else int(record_capacity)
        self._ck(self.lib.mot_export_sequence_scene_voxels_dev(self._h, int(frames), C.byref(p), _scene_mask(classes), C.byref(v), C.c_long(cap), C.c_void_p(d_voxels_ptr or None),
                                                               C.c_long(voxel_capacity), C.c_void_p(d_header_ptr or None), C.c_void_p(d_totals_ptr or None)))

    def get_sequence_scene_voxels(self, frames: int, leaf, min_points: int = 1, min_static_hits: int = 1, trail=(1, 2), classes=("known",), record_capacity=None) -> dict:
        """the same on the host (mot_get_sequence_scene_voxels): xyz [n, 3] and count [n] of the kept voxels in ascending (i_z, i_y, i_x), header (a
        SCENE_VOXEL_HEADER_DTYPE record), totals [5] (SCENE_SEGMENT_DTYPE). With the defaults: the drive's static map, one point a voxel. The records are sorted
        ONCE: the judge's counts alone (mot_get_sequence_scene_points without buffers: classify and two scans) bound the voxels by the selected records, then one
        voxel call fills a buffer of that size"""
        p = MotSceneJudgeParams(int(min_static_hits), int(trail[0]), int(trail[1])); v = voxel_params(leaf, min_points)
        mask, F = _scene_mask(classes), int(frames)
        cap = C.c_long(F * self.max_points if record_capacity is None else int(record_capacity))
        hdr = np.zeros(1, SCENE_VOXEL_HEADER_DTYPE); tot = np.zeros(SCENE_CLASSES, SCENE_SEGMENT_DTYPE); n = C.c_long(0)
        seg = np.zeros((max(F, 1), SCENE_CLASSES), SCENE_SEGMENT_DTYPE)
        self._ck(self.lib.mot_get_sequence_scene_points(self._h, F, C.byref(p), mask, MOT_FRAME_GLOBAL, None, C.c_long(0), C.byref(n), _vp(seg), _vp(tot), None, C.c_long(0)))
        bound = max(min(n.value, cap.value), 0)   # a voxel holds a record or more
        vox = np.zeros(max(bound, 1), MODEL_VOXEL_DTYPE)
        self._ck(self.lib.mot_get_sequence_scene_voxels(self._h, F, C.byref(p), mask, C.byref(v), cap, _vp(vox), C.c_long(bound), C.byref(n), _vp(hdr), _vp(tot)))
        vox = vox[: n.value]
        return dict(xyz=vox["xyz"].copy(), count=vox["count"].copy(), header=hdr[0].copy(), totals=tot)

    def merge_voxel_maps_dev(self, maps, leaf, d_out_ptr: int, out_capacity: int, d_header_ptr: int, min_points: int = 1):
        """up to 16 voxel maps of the global lattice merged into one on the device (mot_merge_voxel_maps_dev). maps: (d_voxels_ptr, d_count_ptr or 0, capacity)
        each — device blocks of MODEL_VOXEL_DTYPE as every voxel export writes them, the count an int32 ON THE DEVICE (e.g. the address of n_stored in the header
        an earlier export (header pointer + 20) or an earlier merge (+ 16) wrote; 0: the capacity is the count). -> caller's device blocks: the voxels of the distinct cells of edge
        `leaf` in ascending (i_z, i_y, i_x), counts added, centroids weighted by count, cells whose summed count is below min_points dropped; the 32-byte header
        (VOXEL_MERGE_HEADER_DTYPE). Reads nothing but its arguments; asynchronous"""
        arr = (MotVoxelMapSrc * max(len(maps), 1))(*[MotVoxelMapSrc(int(p) or None, int(n) or None, int(cap)) for p, n, cap in maps])
        v = voxel_params(leaf, min_points)
        self._ck(self.lib.mot_merge_voxel_maps_dev(self._h, arr, len(maps), C.byref(v), C.c_void_p(d_out_ptr or None), C.c_long(out_capacity), C.c_void_p(d_header_ptr or None)))

    def merge_voxel_maps(self, maps, leaf, min_points: int = 1) -> dict:
        """the same from host arrays (mot_merge_voxel_maps; synchronises). maps: dicts with xyz [n, 3] and count [n] (what the voxel getters return), or
        MODEL_VOXEL_DTYPE arrays. -> xyz [n, 3], count [n], header (a VOXEL_MERGE_HEADER_DTYPE record)"""
        blocks = []
        for mp in maps:
            if isinstance(mp, dict):
                b = np.zeros(len(mp["count"]), MODEL_VOXEL_DTYPE); b["xyz"] = np.asarray(mp["xyz"], np.float32).reshape(-1, 3); b["count"] = mp["count"]
            else:
                b = np.ascontiguousarray(mp, MODEL_VOXEL_DTYPE)
            blocks.append(b)
        arr = (MotVoxelMapSrc * max(len(blocks), 1))(*[MotVoxelMapSrc(b.ctypes.data if len(b) else None, None, len(b)) for b in blocks])
        v = voxel_params(leaf, min_points)
        bound = sum(len(b) for b in blocks)   # a voxel holds an input or more
        out = np.zeros(max(bound, 1), MODEL_VOXEL_DTYPE); hdr = np.zeros(1, VOXEL_MERGE_HEADER_DTYPE); n = C.c_long(0)
        self._ck(self.lib.mot_merge_voxel_maps(self._h, arr, len(blocks), C.byref(v), _vp(out), C.c_long(bound), C.byref(n), _vp(hdr)))
        out = out[: n.value]
        return dict(xyz=out["xyz"].copy(), count=out["count"].copy(), header=hdr[0].copy())

    def index_voxel_maps_dev(self, maps, leaf, index: MotVoxelIndex, min_points: int = 1) -> MotVoxelIndex:
        """up to 16 voxel maps of the global lattice indexed on the device (mot_index_voxel_maps_dev): the merge without the centroid. maps: as for
        merge_voxel_maps_dev, the counts read on the device. -> the caller's device blocks named by `index` (voxel_index()): the kept cells' 64-bit keys, strictly
        ascending, their summed counts (saturated at 2^31 - 1) and the merge's header, whose n_stored is the index's length; the descriptor's leaf is filled in and
        the descriptor returned: what export_map_points_dev / get_map_points take. Asynchronous"""
        arr = (MotVoxelMapSrc * max(len(maps), 1))(*[MotVoxelMapSrc(int(p) or None, int(n) or None, int(cap)) for p, n, cap in maps])
        v = voxel_params(leaf, min_points)
        self._ck(self.lib.mot_index_voxel_maps_dev(self._h, arr, len(maps), C.byref(v), C.byref(index)))
        return index

    def export_map_points_dev(self, batch: int, index: MotVoxelIndex, d_points_ptr: int, point_stride: int, d_segments_ptr: int, d_classes_ptr: int = 0, class_stride: int = 0,
                              min_count: int = 1, reach: int = 0, classes=None, frame=MOT_FRAME_GLOBAL):
        """the elevated points of slots 0..batch-1 judged against a voxel index and partitioned by class (mot_export_map_points_dev) -> caller's device blocks, in
        the shape of export_scene_points_dev: 16-byte records d_points[b * point_stride + i] (the classes of `classes`, ascending, each in input order), 8-byte
        segments d_segments[b * 5 + k] = {first, count} (SCENE_SEGMENT_DTYPE; classes MAP_OUTSIDE .. MAP_PRESENT) and, if given, one class byte per elevated point.
        MAP_ABSENT: the map of the earlier pass has nothing there. reach 1: the 27 cells round the point's. Needs links, not the scene grid; asynchronous"""
        p = MotMapJudgeParams(int(min_count), int(reach))
        self._ck(self.lib.mot_export_map_points_dev(self._h, int(batch), C.byref(index), C.byref(p), _map_mask(classes), _frame(frame), C.c_void_p(d_points_ptr or None),
                                                    C.c_long(point_stride), C.c_void_p(d_segments_ptr or None), C.c_void_p(d_classes_ptr or None), C.c_long(class_stride)))

    def get_map_points(self, slot: int, index: MotVoxelIndex, min_count: int = 1, reach: int = 0, classes=None, frame=MOT_FRAME_GLOBAL) -> dict:
        """one slot's elevated points judged against a voxel index in DEVICE blocks (mot_get_map_points; synchronises): segments [5] (SCENE_SEGMENT_DTYPE: first,
        count per class MAP_OUTSIDE .. MAP_PRESENT; first = -1 for a class outside `classes`), xyz [n, 3] and index [n] of the selected classes back to back,
        classes [n_elevated] (uint8, input order)"""
        p = MotMapJudgeParams(int(min_count), int(reach))
        cap = self.max_points
        pts = np.zeros(max(cap, 1), TRACK_POINT_DTYPE); seg = np.zeros(MAP_CLASSES, SCENE_SEGMENT_DTYPE); cls = np.zeros(max(cap, 1), np.uint8); npts, ne = C.c_int(0), C.c_int(0)
        self._ck(self.lib.mot_get_map_points(self._h, int(slot), C.byref(index), C.byref(p), _map_mask(classes), _frame(frame), _vp(pts), cap, C.byref(npts), _vp(seg), _vp(cls), cap,
                                             C.byref(ne)))
        pts = pts[: npts.value]
        return dict(segments=seg, xyz=pts["xyz"].copy(), index=pts["index"].copy(), classes=cls[: ne.value].copy())

    def get_scene_grid(self, slot: int = 0, cells: bool = True) -> dict:
        """one slot's grid on the host (mot_get_scene_grid): header (a SCENE_HEADER_DTYPE record) and cells [size, size] indexed (v, u) (SCENE_CELL_DTYPE;
        cells=False: the header alone, cells None)"""
        hdr = np.zeros(1, SCENE_HEADER_DTYPE); n = C.c_int(0)
        if not cells:
            self._ck(self.lib.mot_get_scene_grid(self._h, int(slot), None, 0, C.byref(n), _vp(hdr)))
            return dict(header=hdr[0].copy(), cells=None)
        self._ck(self.lib.mot_get_scene_grid(self._h, int(slot), None, 0, C.byref(n), None))   # the count alone
        W = int(round(n.value ** 0.5))
        out = np.zeros(max(n.value, 1), SCENE_CELL_DTYPE)
        self._ck(self.lib.mot_get_scene_grid(self._h, int(slot), _vp(out), n.value, C.byref(n), _vp(hdr)))
        return dict(header=hdr[0].copy(), cells=out[: n.value].reshape(W, W))

    def _track_buffer(self, slot, max_tracks):
        """records a call can deliver: one per track EVER created on the stream, which outgrows the number of slots on a long run"""
        if max_tracks:
            return max_tracks
        hint = getattr(self, "_nt_hint", None)
        if hint is None:
            hint = self._nt_hint = {}
        return max(self.max_tracks_total, hint.get(slot, 0) + 256)

    def _ck_tracks(self, rc, n, cap):
        """mot_get_tracks / mot_track_step deliver the records AND report MOT_E_CAPACITY once a stream has used up max_tracks_total
        (sticky until reset): a soft condition here — the records are returned, `capacity_exceeded` says so"""
        if rc == MOT_E_CAPACITY and 0 <= n <= cap:   # (n = -1: mot_track_step refused the frame — more than 1024 boxes — and did not run: an error like any other)
            return True
        self._ck(rc)
        return False

    # ------------------------------------------------------------------ stage calls, host buffers
    def ground_remove(self, xyzw, want_mask: bool = True):
        """groundRemove(cloud, elevatedCloud, groundCloud) — OT/include/ground_removal.h:62-64"""
        a = _pts(xyzw); n = len(a)
        elev = np.empty((max(n, 1), 4), np.float32); ground = np.empty((max(n, 1), 4), np.float32)
        mask = np.zeros(max(n, 1), np.uint8) if want_mask else None
        ne, ng = C.c_int(0), C.c_int(0)
        self._ck(self.lib.mot_ground_remove(self._h, _vp(a), n, _vp(elev), C.byref(ne), _vp(ground), C.byref(ng), _vp(mask)))
        out = dict(elevated=elev[: ne.value].copy(), ground=ground[: ng.value].copy())
        if want_mask:
            out["mask"] = mask[:n].copy()
        return out

    def ground_remove_pointcloud2(self, payload, n: int, point_step: int, off_x: int, off_y: int, off_z: int, want_mask: bool = True):
        """fromROSMsg + groundRemove on a sensor_msgs/PointCloud2 payload in host memory (one H2D of the raw records)"""
        raw = np.ascontiguousarray(payload, np.uint8).reshape(-1)
        assert raw.size >= n * point_step
        elev = np.empty((max(n, 1), 4), np.float32); ground = np.empty((max(n, 1), 4), np.float32)
        mask = np.zeros(max(n, 1), np.uint8) if want_mask else None
        ne, ng = C.c_int(0), C.c_int(0)
        self._ck(self.lib.mot_ground_remove_pointcloud2(self._h, _vp(raw), n, point_step, off_x, off_y, off_z, _vp(elev), C.byref(ne),
                                                        _vp(ground), C.byref(ng), _vp(mask)))
        out = dict(elevated=elev[: ne.value].copy(), ground=ground[: ng.value].copy())
        if want_mask:
            out["mask"] = mask[:n].copy()
        return out

    def frame_pointcloud2(self, payload, n: int, point_step: int, off_x: int, off_y: int, off_z: int):
        """ground -> cluster -> box on a PointCloud2 payload in host memory, everything resident in slot 0 (asynchronous)"""
        raw = np.ascontiguousarray(payload, np.uint8).reshape(-1)
        assert raw.size >= n * point_step
        self._ck(self.lib.mot_frame_pointcloud2(self._h, _vp(raw), n, point_step, off_x, off_y, off_z))

    def box_fit_resident(self, max_boxes: int = 4096):
        """boxFitting on the cloud and label grid that cluster() left resident in slot 0"""
        boxes = np.zeros((max_boxes, 8, 3), np.float32); nb = C.c_int(0); bc = np.zeros(max_boxes, np.int32); nu = C.c_int(0)
        self._ck(self.lib.mot_box_fit_resident(self._h, _vp(boxes), max_boxes, C.byref(nb), _vp(bc), C.byref(nu)))
        return dict(boxes=boxes[: nb.value].copy(), box_cluster=bc[: nb.value].copy(), n_undefined=nu.value)

    def cluster(self, elevated_xyzw):
        """componentClustering(elevatedCloud, cartesianData, numCluster) — OT/include/component_clustering.h:20-22"""
        a = _pts(elevated_xyzw); n = len(a); G = self.params.num_grid
        grid = np.zeros((G, G), np.int32); nc = C.c_int(0); lab = np.zeros(max(n, 1), np.int32)
        self._ck(self.lib.mot_cluster(self._h, _vp(a), n, _vp(grid), C.byref(nc), _vp(lab)))
        return dict(grid=grid, num_cluster=nc.value, point_label=lab[:n].copy())

    def box_fit(self, elevated_xyzw, grid, num_cluster: int, max_boxes: int = 4096):
        """boxFitting(elevatedCloud, cartesianData, numCluster, ma) — OT/include/box_fitting.h:34-36"""
        a = _pts(elevated_xyzw); n = len(a)
        grid = np.ascontiguousarray(grid, np.int32)
        boxes = np.zeros((max_boxes, 8, 3), np.float32); nb = C.c_int(0); bc = np.zeros(max_boxes, np.int32); nu = C.c_int(0)
        self._ck(self.lib.mot_box_fit(self._h, _vp(a), n, _vp(grid), num_cluster, _vp(boxes), max_boxes, C.byref(nb), _vp(bc), C.byref(nu)))
        return dict(boxes=boxes[: nb.value].copy(), box_cluster=bc[: nb.value].copy(), n_undefined=nu.value)

    def ego_update(self, timestamp: float, v_gps: float, yaw_gps: float, slot: int = 0):
        """getOriginPoints(timestamp, originPoints, v_gps, yaw_gps) — OT/include/imm_ukf_jpda.h:15"""
        out = np.zeros(6)
        self._ck(self.lib.mot_ego_update(self._h, slot, C.c_double(timestamp), C.c_double(v_gps), C.c_double(yaw_gps), _vp(out)))
        return out

    def track_step(self, boxes_global, timestamp: float, slot: int = 0, max_tracks: int | None = None):
        """immUkfJpdaf(bBoxes, timestamp, ...) — OT/include/imm_ukf_jpda.h:19-22"""
        b = np.ascontiguousarray(boxes_global, np.float32).reshape(-1, 8, 3)
        cap = self._track_buffer(slot, max_tracks)
        arr = (MotTrack * cap)(); nt = C.c_int(0)
        rc = self.lib.mot_track_step(self._h, slot, _vp(b), len(b), C.c_double(timestamp), arr, cap, C.byref(nt))
        self._nt_hint[slot] = max(nt.value, 0)
        if rc == MOT_E_CAPACITY and nt.value > cap and not max_tracks:   # the step has run; only the buffer was too small: fetch again
            return self.get_tracks(slot)
        full = self._ck_tracks(rc, nt.value, cap)
        out = tracks_to_dict(arr, nt.value); out["capacity_exceeded"] = full
        return out

    def track_state(self, track_id: int, slot: int = 0):
        s = MotTrackState()
        self._ck(self.lib.mot_track_get_state(self._h, slot, track_id, C.byref(s)))
        return state_to_dict(s)

    # ------------------------------------------------------------------ fused frames, device buffers
    def frames_dev(self, d_ptr: int, frame_stride_floats: int, n_points, run_tracker: bool = False,
                   timestamps=None, ego_v=None, ego_yaw=None):
        """ground -> cluster -> box (-> tracker) for one frame per slot; everything stays in HBM. Asynchronous."""
        n = np.ascontiguousarray(n_points, np.int32); B = len(n)
        ts = np.ascontiguousarray(timestamps if timestamps is not None else np.zeros(B), np.float64)
        ev = np.ascontiguousarray(ego_v if ego_v is not None else np.zeros(B), np.float64)
        ey = np.ascontiguousarray(ego_yaw if ego_yaw is not None else np.zeros(B), np.float64)
        self._ck(self.lib.mot_frames_dev(self._h, C.c_void_p(d_ptr), C.c_long(frame_stride_floats), _vp(n), B,
                                         int(run_tracker), _vp(ts), _vp(ev), _vp(ey)))

    def sequence_dev(self, d_ptr: int, frame_stride_floats: int, n_points, timestamps, ego_v, ego_yaw, d_tracks_ptr: int = 0,
                     max_per_frame: int = 0, d_counts_ptr: int = 0):
        """SEQUENCE MODE (mot_sequence_dev): len(n_points) consecutive frames of ONE stream — stateless stages as one batch (slot k = frame
        k), the tracker chained on the device on stream 0's tracks. Optional device buffers receive the live tracks after every frame."""
        n = np.ascontiguousarray(n_points, np.int32); K = len(n)
        ts = np.ascontiguousarray(timestamps, np.float64); ev = np.ascontiguousarray(ego_v, np.float64); ey = np.ascontiguousarray(ego_yaw, np.float64)
        assert len(ts) == len(ev) == len(ey) == K
        self._ck(self.lib.mot_sequence_dev(self._h, C.c_void_p(d_ptr), C.c_long(frame_stride_floats), _vp(n), K, _vp(ts), _vp(ev), _vp(ey),
                                           C.c_void_p(d_tracks_ptr or None), int(max_per_frame), C.c_void_p(d_counts_ptr or None)))

    def sequence_accumulate_dev(self, d_ptr: int, frame_stride_floats: int, n_points, timestamps, ego_v, ego_yaw, d_tracks_ptr: int = 0,
                                max_per_frame: int = 0, d_counts_ptr: int = 0):
        """sequence_dev, and every frame appended to stream 0's per-track accumulators in the same asynchronous call (mot_sequence_accumulate_dev): what
        len(n_points) rounds of frames_dev(batch 1) + accumulate_track_points(1) leave in slot 0, bit for bit. Needs links and accumulation on."""
        n = np.ascontiguousarray(n_points, np.int32); K = len(n)
        ts = np.ascontiguousarray(timestamps, np.float64); ev = np.ascontiguousarray(ego_v, np.float64); ey = np.ascontiguousarray(ego_yaw, np.float64)
        assert len(ts) == len(ev) == len(ey) == K
        self._ck(self.lib.mot_sequence_accumulate_dev(self._h, C.c_void_p(d_ptr), C.c_long(frame_stride_floats), _vp(n), K, _vp(ts), _vp(ev), _vp(ey),
                                                      C.c_void_p(d_tracks_ptr or None), int(max_per_frame), C.c_void_p(d_counts_ptr or None)))

    def sequence_products_dev(self, d_ptr: int, frame_stride_floats: int, n_points, timestamps, ego_v, ego_yaw, d_tracks_ptr: int = 0,
                              max_per_frame: int = 0, d_counts_ptr: int = 0, accumulate: bool = False, scene: bool = False, products: int | None = None):
        """sequence_dev with products taken from every frame in the same asynchronous call (mot_sequence_products_dev): accumulate = stream 0's per-track
        accumulators (as sequence_accumulate_dev), scene = stream 0's scene grid — what len(n_points) rounds of frames_dev(batch 1) + accumulate_scene(1) leave
        in slot 0, byte for byte. products: the raw bit set instead of the two flags."""
        n = np.ascontiguousarray(n_points, np.int32); K = len(n)
        ts = np.ascontiguousarray(timestamps, np.float64); ev = np.ascontiguousarray(ego_v, np.float64); ey = np.ascontiguousarray(ego_yaw, np.float64)
        assert len(ts) == len(ev) == len(ey) == K
        bits = int(products) if products is not None else (SEQ_ACCUMULATE if accumulate else 0) | (SEQ_SCENE if scene else 0)
        self._ck(self.lib.mot_sequence_products_dev(self._h, C.c_void_p(d_ptr), C.c_long(frame_stride_floats), _vp(n), K, _vp(ts), _vp(ev), _vp(ey),
                                                    C.c_void_p(d_tracks_ptr or None), int(max_per_frame), C.c_void_p(d_counts_ptr or None), bits))

    def get_ground(self, slot: int = 0, n_hint: int | None = None, want_clouds: bool = True):
        """n_hint: number of input points of the frame (length of the returned mask); the buffers are sized by max_points"""
        cap = self.max_points
        n = min(n_hint, cap) if n_hint is not None else cap
        elev = np.empty((cap, 4), np.float32) if want_clouds else None
        ground = np.empty((cap, 4), np.float32) if want_clouds else None
        mask = np.zeros(cap, np.uint8) if want_clouds else None
        ne, ng = C.c_int(0), C.c_int(0)
        self._ck(self.lib.mot_get_ground(self._h, slot, _vp(elev), C.byref(ne), _vp(ground), C.byref(ng), _vp(mask), cap))
        out = dict(n_elevated=ne.value, n_ground=ng.value)
        if want_clouds:
            out.update(elevated=elev[: ne.value].copy(), ground=ground[: ng.value].copy(), mask=mask[:n].copy())
        return out

    def get_clusters(self, slot: int = 0, n_elevated: int = 0):
        """n_elevated > 0: also return the per-point labels (the resident count is what is delivered; the hint only switches them on)"""
        G = self.params.num_grid
        grid = np.zeros((G, G), np.int32); nc = C.c_int(0)
        lab = np.zeros(self.max_points, np.int32) if n_elevated else None
        self._ck(self.lib.mot_get_clusters(self._h, slot, _vp(grid), C.byref(nc), _vp(lab), self.max_points if n_elevated else 0))
        return dict(grid=grid, num_cluster=nc.value, point_label=lab[:n_elevated].copy() if n_elevated else np.zeros(0, np.int32))

    def decode_pointcloud2_dev(self, d_data_ptr: int, n: int, point_step: int, off_x: int, off_y: int, off_z: int, off_w: int, d_xyzw_ptr: int):
        """PointCloud2 payload (device) -> float4 points (device), asynchronous on the context stream"""
        self._ck(self.lib.mot_decode_pointcloud2_dev(self._h, C.c_void_p(d_data_ptr), n, point_step, off_x, off_y, off_z, off_w, C.c_void_p(d_xyzw_ptr)))

    def cluster_products(self, slot: int = 0, sp: "MotSideParams | None" = None):
        """makeClusteredCloud / setObsMsg / createCostMap of the cluster node (component_clustering.cpp:311-379, 425-457) on the
        elevated cloud and label grid resident in ``slot``"""
        if sp is None:
            sp = MotSideParams(); self._ck(self.lib.mot_side_params_default(C.byref(sp)))
        n = self.max_points; G = self.params.num_grid
        cc = np.zeros((n, 4), np.float32); ob = np.zeros((G * G, 4), np.float32)
        cm = np.zeros(sp.cost_width * sp.cost_height, np.int32); ncc = C.c_int(0); nob = C.c_int(0)
        self._ck(self.lib.mot_cluster_products(self._h, slot, C.byref(sp), _vp(cc), n, C.byref(ncc), _vp(ob), G * G, C.byref(nob), _vp(cm)))
        return dict(clustered=cc[: ncc.value].copy(), obstacles=ob[: nob.value].copy(), cost_map=cm.reshape(sp.cost_height, sp.cost_width))

    def cluster_products_host(self, elev, grid, sp: "MotSideParams | None" = None):
        """the same on a caller-supplied cloud and label grid (the reference functions' argument lists)"""
        if sp is None:
            sp = MotSideParams(); self._ck(self.lib.mot_side_params_default(C.byref(sp)))
        a = _pts(elev); n = len(a); G = self.params.num_grid
        grid = np.ascontiguousarray(grid, np.int32)
        cc = np.zeros((max(n, 1), 4), np.float32); ob = np.zeros((G * G, 4), np.float32)
        cm = np.zeros(sp.cost_width * sp.cost_height, np.int32); ncc = C.c_int(0); nob = C.c_int(0)
        self._ck(self.lib.mot_cluster_products_host(self._h, _vp(a), n, _vp(grid), C.byref(sp), _vp(cc), max(n, 1), C.byref(ncc), _vp(ob), G * G,
                                                    C.byref(nob), _vp(cm)))
        return dict(clustered=cc[: ncc.value].copy(), obstacles=ob[: nob.value].copy(), cost_map=cm.reshape(sp.cost_height, sp.cost_width))

    def cluster_node_frame(self, elev, sp: "MotSideParams | None" = None, copy: bool = True):
        """the cluster node's whole callback in one call (mot_cluster_node_frame): labelling, side products, box fit, cubes"""
        if sp is None:
            sp = MotSideParams(); self._ck(self.lib.mot_side_params_default(C.byref(sp)))
        a = _pts(elev); fr = MotClusterFrame()
        self._ck(self.lib.mot_cluster_node_frame(self._h, _vp(a), len(a), C.byref(sp), C.byref(fr)))
        view = lambda ptr, shape, dt: (np.ctypeslib.as_array(ptr, shape=shape).view(dt) if shape[0] else np.zeros(shape, dt))
        out = dict(num_cluster=fr.num_cluster, n_undefined=fr.n_undefined,
                   clustered=view(fr.clustered_xyzw, (fr.n_clustered, 4), np.float32), obstacles=view(fr.obstacles_xyzc, (fr.n_obstacles, 4), np.float32),
                   cost_map=view(fr.cost_map, (fr.cost_cells,), np.int32).reshape(sp.cost_height, sp.cost_width),
                   boxes=view(fr.boxes, (fr.n_boxes, 24), np.float32).reshape(-1, 8, 3), box_cluster=view(fr.box_cluster, (fr.n_boxes,), np.int32),
                   cubes=view(fr.centroid_extent, (fr.n_boxes, 6), np.float32))
        return {k: (v.copy() if copy and isinstance(v, np.ndarray) else v) for k, v in out.items()}

    def ground_node_frame(self, cloud, copy: bool = True):
        """mot_ground_node_frame: groundRemove with the two clouds as views into the context's page-locked block"""
        a = _pts(cloud); pe, pg = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(); ne, ng = C.c_int(0), C.c_int(0)
        self._ck(self.lib.mot_ground_node_frame(self._h, _vp(a), len(a), C.byref(pe), C.byref(ne), C.byref(pg), C.byref(ng)))
        e = np.ctypeslib.as_array(pe, shape=(ne.value, 4)) if ne.value else np.zeros((0, 4), np.float32)
        g = np.ctypeslib.as_array(pg, shape=(ng.value, 4)) if ng.value else np.zeros((0, 4), np.float32)
        return dict(elevated=e.copy() if copy else e, ground=g.copy() if copy else g)

    def box_markers(self, slot: int = 0, max_boxes: int = 1024):
        """mark_cluster (box_fitting.cpp:161-209) of every box of ``slot``'s last box stage -> [n_boxes, 6]: centroid xyz, extent xyz"""
        out = np.zeros((max_boxes, 6), np.float32); nb = C.c_int(0)
        self._ck(self.lib.mot_box_markers(self._h, slot, _vp(out), max_boxes, C.byref(nb)))
        return out[: nb.value].copy()

    def get_boxes(self, slot: int = 0, max_boxes: int = 4096):
        boxes = np.zeros((max_boxes, 8, 3), np.float32); nb = C.c_int(0); bc = np.zeros(max_boxes, np.int32); nu = C.c_int(0)
        self._ck(self.lib.mot_get_boxes(self._h, slot, _vp(boxes), max_boxes, C.byref(nb), _vp(bc), C.byref(nu)))
        return dict(boxes=boxes[: nb.value].copy(), box_cluster=bc[: nb.value].copy(), n_undefined=nu.value)

    def get_tracks(self, slot: int = 0, max_tracks: int | None = None):
        cap = self._track_buffer(slot, max_tracks)
        arr = (MotTrack * cap)(); nt = C.c_int(0)
        rc = self.lib.mot_get_tracks(self._h, slot, arr, cap, C.byref(nt))
        self._nt_hint[slot] = max(nt.value, 0)
        if rc == MOT_E_CAPACITY and nt.value > cap and not max_tracks:
            cap = nt.value + 256
            arr = (MotTrack * cap)()
            rc = self.lib.mot_get_tracks(self._h, slot, arr, cap, C.byref(nt))
        full = self._ck_tracks(rc, nt.value, cap)
        out = tracks_to_dict(arr, nt.value); out["capacity_exceeded"] = full
        return out

    def frames_host(self, h_ptr: int, frame_stride_floats: int, n_points, run_tracker: bool = False,
                    timestamps=None, ego_v=None, ego_yaw=None):
        """frames_dev for frames in (page-locked) HOST memory: the upload of this batch overlaps the previous batch's kernels"""
        n = np.ascontiguousarray(n_points, np.int32); B = len(n)
        ts = np.ascontiguousarray(timestamps if timestamps is not None else np.zeros(B), np.float64)
        ev = np.ascontiguousarray(ego_v if ego_v is not None else np.zeros(B), np.float64)
        ey = np.ascontiguousarray(ego_yaw if ego_yaw is not None else np.zeros(B), np.float64)
        self._ck(self.lib.mot_frames_host(self._h, C.c_void_p(h_ptr), C.c_long(frame_stride_floats), _vp(n), B,
                                          int(run_tracker), _vp(ts), _vp(ev), _vp(ey)))

    def frames_host_xyz(self, h_ptr: int, frame_stride_floats: int, n_points, run_tracker: bool = False,
                        timestamps=None, ego_v=None, ego_yaw=None):
        """frames_host for packed {x, y, z} records (12 bytes a point; frame_stride_floats >= 3 n): pcl::PointXYZ has no 4th value, the host link carries 25 % less"""
        n = np.ascontiguousarray(n_points, np.int32); B = len(n)
        ts = np.ascontiguousarray(timestamps if timestamps is not None else np.zeros(B), np.float64)
        ev = np.ascontiguousarray(ego_v if ego_v is not None else np.zeros(B), np.float64)
        ey = np.ascontiguousarray(ego_yaw if ego_yaw is not None else np.zeros(B), np.float64)
        self._ck(self.lib.mot_frames_host_xyz(self._h, C.c_void_p(h_ptr), C.c_long(frame_stride_floats), _vp(n), B,
                                              int(run_tracker), _vp(ts), _vp(ev), _vp(ey)))

    def frames_host_pointcloud2(self, payloads, n_points, point_step: int, off_x: int, off_y: int, off_z: int, off_w: int = -1, run_tracker: bool = False,
                                timestamps=None, ego_v=None, ego_yaw=None):
        """frames_host for one sensor_msgs/PointCloud2 payload per stream (payloads: host addresses, or numpy uint8 arrays kept alive by the caller until wait_uploads)"""
        n = np.ascontiguousarray(n_points, np.int32); B = len(n)
        ptrs = (C.c_void_p * B)(*[(p.ctypes.data if hasattr(p, "ctypes") else int(p)) if p is not None else None for p in payloads])
        ts = np.ascontiguousarray(timestamps if timestamps is not None else np.zeros(B), np.float64)
        ev = np.ascontiguousarray(ego_v if ego_v is not None else np.zeros(B), np.float64)
        ey = np.ascontiguousarray(ego_yaw if ego_yaw is not None else np.zeros(B), np.float64)
        self._ck(self.lib.mot_frames_host_pointcloud2(self._h, ptrs, _vp(n), B, point_step, off_x, off_y, off_z, off_w, int(run_tracker), _vp(ts), _vp(ev), _vp(ey)))

    def wait_uploads(self):
        self._ck(self.lib.mot_wait_uploads(self._h))

    def fetch_tracks_async(self, batch: int, h_tracks_ptr: int, max_per_slot: int, h_counts_ptr: int, frame="global"):
        """frame="sensor": the records relative to each stream's vehicle (mot_fetch_tracks_frame_async)"""
        if _frame(frame) == MOT_FRAME_GLOBAL:
            self._ck(self.lib.mot_fetch_tracks_async(self._h, batch, C.c_void_p(h_tracks_ptr), max_per_slot, C.c_void_p(h_counts_ptr)))
        else:
            self._ck(self.lib.mot_fetch_tracks_frame_async(self._h, batch, _frame(frame), C.c_void_p(h_tracks_ptr), max_per_slot, C.c_void_p(h_counts_ptr)))

    def sensor_pose(self, slot: int = 0):
        """(sensor_from_global, global_from_sensor): the float 3 x 4 matrices of the pose the slot's dead reckoning holds (mot_sensor_pose)"""
        a, b = np.zeros(12, np.float32), np.zeros(12, np.float32)
        self._ck(self.lib.mot_sensor_pose(self._h, slot, _vp(a), _vp(b)))
        return a.reshape(3, 4), b.reshape(3, 4)

    def tracking_node_frame(self, boxes_sensor, timestamp: float, v_gps: float, yaw_gps: float, slot: int = 0, copy: bool = True):
        """the tracking node's whole callback in one call (mot_tracking_node_frame): getOriginPoints, the boxes sensor -> global on the device, immUkfJpdaf,
        the live tracks back in the sensor frame. `tracks`: a TRACK_DTYPE record array, in id order. Dropped births: capacity_exceeded, records delivered."""
        b = np.ascontiguousarray(boxes_sensor, np.float32).reshape(-1, 8, 3); fr = MotTrackingFrame()
        rc = self.lib.mot_tracking_node_frame(self._h, slot, _vp(b), len(b), C.c_double(timestamp), C.c_double(v_gps), C.c_double(yaw_gps), C.byref(fr))
        full = rc == MOT_E_CAPACITY
        if not full:
            self._ck(rc)
        rec = np.ctypeslib.as_array(C.cast(fr.tracks, C.POINTER(C.c_uint8)), shape=(fr.n_live * C.sizeof(MotTrack),)).view(TRACK_DTYPE) if fr.n_live else np.zeros(0, TRACK_DTYPE)
        return dict(origin=np.array(fr.origin6[:]), n_live=fr.n_live, n_ever=fr.n_ever, tracks=rec.copy() if copy else rec, capacity_exceeded=full)

    def track_steps_dev(self, d_boxes_ptr: int, box_stride_floats: int, m, timestamps):
        """immUkfJpdaf for one frame of every slot, boxes (global frame) already on the device"""
        mm = np.ascontiguousarray(m, np.int32); ts = np.ascontiguousarray(timestamps, np.float64)
        self._ck(self.lib.mot_track_steps_dev(self._h, C.c_void_p(d_boxes_ptr), C.c_long(box_stride_floats), _vp(mm), len(mm), _vp(ts)))

    def profile_kernel(self, kernel_id: int, every: int = 1):
        """time every `every`-th launch of kernel `kernel_id` inside frames_dev / frames_host (0 = off); see profile_read"""
        self._ck(self.lib.mot_profile_kernel(self._h, kernel_id, every))

    def profile_read(self):
        mean, mn, mx, k = C.c_float(0), C.c_float(0), C.c_float(0), C.c_int(0)
        self._ck(self.lib.mot_profile_read(self._h, C.byref(mean), C.byref(mn), C.byref(mx), C.byref(k)))
        return dict(mean_ms=mean.value, min_ms=mn.value, max_ms=mx.value, samples=k.value)

    def export_tracks_dev(self, batch: int, d_tracks_ptr: int, max_per_slot: int, d_counts_ptr: int, frame="global"):
        """live tracks of every slot -> caller's device buffer (the block that is all-gathered across GPUs); frame="sensor": relative to each stream's vehicle"""
        if _frame(frame) == MOT_FRAME_GLOBAL:
            self._ck(self.lib.mot_export_tracks_dev(self._h, batch, C.c_void_p(d_tracks_ptr), max_per_slot, C.c_void_p(d_counts_ptr)))
        else:
            self._ck(self.lib.mot_export_tracks_frame_dev(self._h, batch, _frame(frame), C.c_void_p(d_tracks_ptr), max_per_slot, C.c_void_p(d_counts_ptr)))

    def export_tracks_packed_dev(self, batch: int, d_block_ptr: int, block_bytes: int, frame="global"):
        """live tracks of every slot, packed (counts header + records back to back) -> caller's device block; frame="sensor" as above"""
        if _frame(frame) == MOT_FRAME_GLOBAL:
            self._ck(self.lib.mot_export_tracks_packed_dev(self._h, batch, C.c_void_p(d_block_ptr), C.c_long(block_bytes)))
        else:
            self._ck(self.lib.mot_export_tracks_packed_frame_dev(self._h, batch, _frame(frame), C.c_void_p(d_block_ptr), C.c_long(block_bytes)))

    def export_tracks(self, batch: int, d_ptr: int, max_per_slot: int | None = None, d_counts_ptr: int | None = None, block_bytes: int | None = None, frame="global"):
        """either export by its arguments: (d_tracks, max_per_slot, d_counts) the fixed block, (d_block, block_bytes=) the packed one"""
        if block_bytes is not None:
            return self.export_tracks_packed_dev(batch, d_ptr, block_bytes, frame=frame)
        return self.export_tracks_dev(batch, d_ptr, max_per_slot, d_counts_ptr, frame=frame)

    def time_stage(self, stage: int, batch: int, iters: int) -> float:
        """average ms per iteration of one stage re-run on resident data, HIP events on the context stream"""
        ms = C.c_float(0)
        self._ck(self.lib.mot_time_stage(self._h, stage, batch, iters, C.byref(ms)))
        return ms.value


def tracks_to_dict(arr, n):
    buf = np.frombuffer(arr, dtype=np.dtype([("id", "i4"), ("track_manage", "i4"), ("is_static", "i4"), ("is_vis", "i4"),
                                             ("p", "f4", 3), ("lifetime", "i4"), ("v_yaw", "f8", 2), ("vis_box", "f4", 24)]),
                        count=n) if n else None
    if n == 0:
        return dict(n=0, track_manage=np.zeros(0, np.int32), is_static=np.zeros(0, np.int32), is_vis=np.zeros(0, np.int32),
                    lifetime=np.zeros(0, np.int32), p=np.zeros((0, 3), np.float32), v_yaw=np.zeros((0, 2)), vis_box=np.zeros((0, 24), np.float32))
    return dict(n=n, track_manage=buf["track_manage"].copy(), is_static=buf["is_static"].copy(), is_vis=buf["is_vis"].copy(),
                lifetime=buf["lifetime"].copy(), p=buf["p"].copy(), v_yaw=buf["v_yaw"].copy(), vis_box=buf["vis_box"].copy())


def state_to_dict(s: MotTrackState):
    d = {}
    for name, _ in MotTrackState._fields_:
        v = getattr(s, name)
        d[name] = np.array(v[:]) if hasattr(v, "__len__") else v
    return d


# ---------------------------------------------------------------------- reference-named convenience layer
_default_ctx: Context | None = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context()
    return _default_ctx


def groundRemove(cloud):
    """drop-in for groundRemove(); returns (elevatedCloud, groundCloud)"""
    r = default_context().ground_remove(cloud, want_mask=False)
    return r["elevated"], r["ground"]


def componentClustering(elevatedCloud):
    """drop-in for componentClustering(); returns (cartesianData, numCluster)"""
    r = default_context().cluster(elevatedCloud)
    return r["grid"], r["num_cluster"]


def boxFitting(elevatedCloud, cartesianData, numCluster):
    """drop-in for boxFitting(); returns the list of 8-corner boxes"""
    return default_context().box_fit(elevatedCloud, cartesianData, numCluster)["boxes"]


def getOriginPoints(timestamp, v_gps, yaw_gps):
    return default_context().ego_update(timestamp, v_gps, yaw_gps).reshape(2, 3)


def immUkfJpdaf(bBoxes, timestamp):
    return default_context().track_step(bBoxes, timestamp)


class NativeGather:
    """include/mot.h mot_gather_*: the per-tick all-gather of the live-track blocks of a rank's contexts, issued from C (RCCL over xGMI on GPUs; a device copy
    with one rank and no communicator). contribute(ci) is what context ci's issuing thread calls after its frame tick."""

    def __init__(self, ctxs, batch: int, capacity_records: int, world: int = 1, rank: int = 0, unique_id: bytes | None = None):
        self.ctxs, self.batch, self.cap, self.world, self.rank = list(ctxs), batch, capacity_records, world, rank
        self.lib = self.ctxs[0].lib
        arr = (C.c_void_p * len(self.ctxs))(*[cx._h for cx in self.ctxs])
        self._g = C.c_void_p()
        idb = (C.c_char * 128).from_buffer_copy(unique_id) if unique_id is not None else None
        rc = self.lib.mot_gather_create(arr, len(self.ctxs), batch, capacity_records, world, rank, idb, C.byref(self._g))
        if rc != MOT_OK:
            raise MotError(rc, "mot_gather_create failed" + (" (no RCCL in this process)" if rc == MOT_E_STATE else ""))
        self.block = ((batch * 4 + 15) & ~15) + capacity_records * C.sizeof(MotTrack)

    @staticmethod
    def unique_id(lib) -> bytes:
        buf = (C.c_char * 128)()
        rc = lib.mot_gather_unique_id(buf)
        if rc != MOT_OK:
            raise MotError(rc, "mot_gather_unique_id failed (no RCCL in this process)")
        return bytes(buf.raw)

    def _ck(self, rc):
        if rc != MOT_OK:
            raise MotError(rc, (self.lib.mot_gather_last_error(self._g) or b"").decode())

    def contribute(self, ci: int):
        self._ck(self.lib.mot_gather_contribute(self._g, ci))

    def result(self):
        """(device pointer of [world][n_ctx] packed blocks, block bytes, tick, hipEvent_t handle) of the last completed tick"""
        d, nb, tick, ev = C.c_void_p(), C.c_long(), C.c_long(), C.c_void_p()
        self._ck(self.lib.mot_gather_result(self._g, C.byref(d), C.byref(nb), C.byref(tick), C.byref(ev)))
        return d.value, nb.value, tick.value, ev.value

    def synchronize(self):
        self._ck(self.lib.mot_gather_synchronize(self._g))

    def close(self):
        if self._g:
            self.lib.mot_gather_destroy(self._g); self._g = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
