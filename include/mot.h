/*
 * mot.h — C-ABI of the MI355X-native LiDAR perception hot path.
 *
 * Drop-in boundary: the plain C++ free functions the three reference ROS nodes call
 * (reference = /root/reference/object_tracking, abbreviated OT/ below):
 *
 *   groundRemove()          OT/include/ground_removal.h:62-64   (called OT/src/groundremove/main.cpp:120)
 *   componentClustering()   OT/include/component_clustering.h:20-22 (called OT/src/cluster/main.cpp:74)
 *   boxFitting()            OT/include/box_fitting.h:34-36       (called OT/src/cluster/main.cpp:119)
 *   getOriginPoints()       OT/include/imm_ukf_jpda.h:15         (called OT/tracking/main.cpp:74)
 *   immUkfJpdaf()           OT/include/imm_ukf_jpda.h:19-22      (called OT/tracking/main.cpp:166)
 *
 * The reference has no FFI; these entry points are what a maintainer binds instead of those
 * functions (see INTEGRATION.md for the C++ adapters with the exact reference signatures).
 * Plain pointers and sizes only — no torch / PCL / Eigen types cross this boundary.
 *
 * Conventions
 *   - points are 16-byte records (x, y, z, w) fp32 — PCL PointXYZ and KITTI .bin share it;
 *     w is carried through untouched.
 *   - every function returns MOT_OK or an error code; mot_last_error() has the text.
 *     Nothing aborts (the reference asserts / prints instead: OT/tracking/imm_ukf_jpda.cpp:130,159,…).
 *   - "_dev" variants take DEVICE pointers and leave results on the device, so stages chain
 *     with no D2H/H2D; they run on the context's HIP stream and do not synchronise.
 *   - a context owns B = max_batch independent sensor streams ("slots"); batch entry points
 *     process slot b = 0..B-1 in one launch sequence. The single-frame entry points use slot 0.
 *   - all device code is HIP for gfx950; there is NO CPU fallback: without a GPU (or on a
 *     device that is not gfx950) mot_create() fails with MOT_E_HIP.
 *   - every entry point makes the context's device current for its own duration and restores the
 *     caller's: contexts on different GPUs may be used from one thread, and from any thread.
 */
#ifndef MOT_H_
#define MOT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOT_ABI_VERSION 6
/* format of mot_stream_save's blobs: its own version since ABI v6 (5 = what ABI v5 wrote; blobs of ABI v4 and older are refused by mot_stream_load) */
#define MOT_SNAPSHOT_FORMAT 5

/* polar grid of the ground stage: compile-time in the reference too
 * (OT/include/ground_removal.h:16-17) */
#define MOT_NUM_CHANNEL 80
#define MOT_NUM_BIN 120
#define MOT_POLAR_CELLS (MOT_NUM_CHANNEL * MOT_NUM_BIN)
/* Cartesian grid edge: 250 in OT/ (component_clustering.h:13), 200 in OT0/; runtime, <= 256 */
#define MOT_MAX_GRID 256
/* trackbox.box_num is uint8 on the wire (OT/msg/trackbox.msg:2) */
#define MOT_MAX_BOXES 255

enum {
  MOT_OK = 0,
  MOT_E_ARG = 1,      /* bad argument (null pointer, n out of range, …) */
  MOT_E_CAPACITY = 2, /* more points / clusters / boxes / tracks than the context was created for */
  MOT_E_HIP = 3,      /* HIP runtime error or no gfx950 device */
  MOT_E_STATE = 4     /* call sequence error */
};

enum { MOT_RNG_LIBSTDCXX10 = 0, MOT_RNG_LIBSTDCXX11 = 1 };

enum {
  MOT_PRESET_OBJECT_TRACKING = 0, /* OT/  constants (the package north_star names) */
  MOT_PRESET_OBJECT_TRACKING0 = 1 /* OT0/ constants (KITTI-tuned), SURVEY.md §2.1 */
};

/* per-point classification written by the ground stage */
enum { MOT_MASK_DROPPED = 0, MOT_MASK_GROUND = 1, MOT_MASK_ELEVATED = 2 };

/* order of the points of an input cloud (mot_set_point_order) */
enum { MOT_ORDER_SCAN = 0, /* default: a scan's own order (beam-major or firing order): the box stage works on the cloud as it lies */
       MOT_ORDER_ANY = 1   /* no order assumed: the box stage first regroups the elevated points by cluster on the device */ };
/* by-products of groundRemove that nothing downstream of it reads (mot_set_fused_outputs) */
enum { MOT_OUT_GROUND = 1, /* groundCloud */ MOT_OUT_MASK = 2, /* the per-point classification */ MOT_OUT_LABELS = 4 /* the cluster label of every elevated point */ };

/* ---- parameter domain ------------------------------------------------------------------------------------------------
 * The rule: a parameter set is either answered exactly as the reference answers it, or mot_create() refuses it with
 * MOT_E_ARG and a message that names the field. What mot_create() admits:
 *   every float / double field   finite (no NaN, no Inf)
 *   gauss_samples                3;    gauss_sigma > 0
 *   r_min, r_max                 0 <= r_min < r_max, MOT_R_MAX_MIN <= r_max <= MOT_R_MAX_MAX, and
 *                                r_max / (r_max - r_min) <= MOT_POLAR_RATIO_MAX (the same as r_min <= 0.75 r_max; the difference
 *                                is the fp32 one). The streaming kernels estimate a point's polar bin with the hardware's 1-ulp
 *                                square root, and that estimate's error, in bins, grows with this ratio: up to the bound it is
 *                                proven to stay inside the guard band that sends a point to the exact evaluation
 *                                (csrc/mot_internal.h, kCellGuard: the derivation). A narrower range is REFUSED, not run on a
 *                                slower path.
 *   num_grid                     8 .. MOT_MAX_GRID
 *   roi_m                        MOT_ROI_M_MIN .. MOT_ROI_M_MAX (the guarded Cartesian cell, kCartGuard, holds for every such
 *                                roi_m: its bound depends on num_grid <= 256 only)
 *   occ_min_count                1 or 2 (the device keeps the two bit planes "cell seen >= 1" and ">= 2" and nothing else)
 *   dilate                       0 or 1
 *   pic_scale                    > 0, pic_scale * roi_m <= 1000 pixels
 *   ram_points                   1 .. 128;   rng_mapping  MOT_RNG_LIBSTDCXX10 or MOT_RNG_LIBSTDCXX11
 * Every other field is taken as it is. The two presets are pinned to the reference's own build; away from them "as the
 * reference answers" means its restatement with the same constants (oracle/), since the reference compiles its constants in.
 * What the suite establishes away from the presets: the ground, cluster and box stages over the lattice of tests/param_cases.py,
 * bit for bit; the tracker's thresholds (life_time_thres, seed_box_index, distance_thres, bb_yaw_change_thres, gamma_g, p_d, p_g)
 * on short sequences chosen so that each of them changes the answer. */
#define MOT_POLAR_RATIO_MAX 4.0f
#define MOT_R_MAX_MIN 1.0e-3f
#define MOT_R_MAX_MAX 1.0e6f
#define MOT_ROI_M_MIN 1.0e-3f
#define MOT_ROI_M_MAX 1.0e6f

/* All tunables of the path. The reference keeps them as file-scope globals; file:line in the
 * comments. mot_params_preset() fills either preset. Their admitted values: "parameter domain" above. */
typedef struct mot_params {
  /* ---- ground stage: OT/src/groundremove/ground_removal.cpp:24-33 ---- */
  float r_min;          /* rMin 3.4 */
  float r_max;          /* rMax 120 */
  float t_hmin;         /* tHmin -2.0 (OT0 -1.9) */
  float t_hmax;         /* tHmax -0.4 (OT0 -1.0) */
  float t_hdiff;        /* tHDiff 0.4 */
  float h_sensor;       /* hSeonsor 2 (OT0 1.73) */
  double ground_margin; /* 0.25, ground_removal.cpp:239 (a double literal) */
  double gauss_sigma;   /* 1, ground_removal.cpp:200 */
  int32_t gauss_samples; /* 3, ground_removal.cpp:200 (only 3 is supported) */
  /* node pre-filter of the `ground` node: OT/src/groundremove/main.cpp:56-81,104-112.
   * crop_enable=0 feeds the full cloud to groundRemove (what OT0/src/main.cpp:57-63 does). */
  int32_t crop_enable;
  float crop_z_min, crop_z_max; /* PassThrough: keep z_min <= z <= z_max  (-3, 1) */
  float crop_x_min, crop_x_max; /* ConditionalRemoval: keep x_min < x < x_max (-15, 5) */
  float crop_y_min, crop_y_max; /* keep y_min < y < y_max (-50, 50) */
  /* ---- cluster stage: OT/src/cluster/component_clustering.cpp:11-12,134-214 ---- */
  int32_t num_grid;      /* numGrid 250 (OT0 200) */
  float roi_m;           /* roiM 50 (OT0 30) */
  int32_t occ_min_count; /* OT: cell occupied iff count > 1  => 2 ; OT0: any point => 1 */
  int32_t dilate;        /* OT: 3x3 dilation of occupied cells => 1 ; OT0 => 0 */
  /* ---- box stage: OT/src/cluster/box_fitting.cpp:18-44 ---- */
  float pic_scale;      /* picScale = 900/roiM */
  int32_t ram_points;   /* ramPoints 80 */
  int32_t l_slope_dist; /* lSlopeDist (int!) 1 (OT0 3) */
  int32_t l_num_points; /* lnumPoints 5 (OT0 300) */
  int32_t lshape_side_cond; /* OT: && (maxMy > 8 || maxMy < -5)  box_fitting.cpp:308 ; OT0: absent */
  float sensor_height;  /* sensorHeight 2 (OT0 1.73) */
  float t_height_min, t_height_max; /* 0.8 (OT0 1.0), 2.6 */
  float t_width_min, t_width_max;   /* 0.2 (OT0 .25), 3.5 */
  float t_len_min, t_len_max;       /* 0.2 (OT0 .5), 14 */
  float t_area_max;                 /* 20 */
  float t_ratio_min, t_ratio_max;   /* 1 (OT0 1.3), 8 (OT0 5) */
  float min_len_ratio;              /* 3 */
  float t_pt_per_m3;                /* 8 */
  int32_t min_points;               /* 30 (OT0 100), box_fitting.cpp:100 */
  /* ---- tracker: OT/tracking/imm_ukf_jpda.cpp:26-51,70,749-760 ---- */
  double gamma_g;        /* gammaG_ 9.22 */
  double p_g, p_d;       /* 0.99, 0.9 */
  double distance_thres; /* distanceThres_ 99 (OT0 0.25) */
  int32_t life_time_thres; /* lifeTimeThres_ 3 (OT0 8) */
  int32_t seed_box_index;  /* first frame seeds a track from box #1 (OT0 #10), :749 */
  double bb_yaw_change_thres; /* 0.2 */
  double first_ego_yaw_offset; /* -0.63035 - pi/2 (OT0 1.22191 - pi/2) */
  double seed_px, seed_py;     /* hard-coded seed position (-1.5125, -8.975), :755-756 */
  /* ---- toolchain dependence of the reference ----
   * box_fitting.cpp:303-315 draws its 80 sample indices with std::uniform_int_distribution<> over std::mt19937_64(0); how a
   * 64-bit draw becomes an index is libstdc++'s choice and changed in GCC 11:
   *   MOT_RNG_LIBSTDCXX11 (1, default)  libstdc++ >= 11: Lemire's multiply-shift with rejection (bits/uniform_int_dist.h, _S_nd)
   *   MOT_RNG_LIBSTDCXX10 (0)           libstdc++ <= 10 (GCC 5 .. 10, i.e. every ROS1 distribution's compiler): scale = (2^64-1) / n,
   *                                     reject draws >= n * scale, index = draw / scale
   * Both scale the draw proportionally and disagree only when draw * n / 2^64 lies within ~n^2 / 2^64 of an integer (5e-14 per
   * draw for a 1000-point cluster): pick the one the reference build you replace was compiled with and the boxes are
   * identical; pick the other and they still are, except with that probability (tests/test_oracle_vs_ref.py). */
  int32_t rng_mapping;
  /* ---- track storage: how many tracks a stream may CREATE over its lifetime (the per-ever-track arrays: 44 bytes each);
   * 0 (preset) = 64 x max_tracks_total. See mot_create. */
  int32_t max_tracks_ever;
} mot_params;

/* one record per track EVER created on a stream (the reference's output vectors are sized that
 * way: targetPoints / targetVandYaw / trackManage / isStaticVec / isVisVec,
 * OT/tracking/imm_ukf_jpda.cpp:995-1041). 144 bytes. A track that died more than one step ago is reported with
 * track_manage 0, is_vis 0, its last position, lifetime and static flag, v = yaw = 0. */
typedef struct mot_track {
  int32_t id;           /* index into targets_ */
  int32_t track_manage; /* trackNumVec_[id] : 0 dead, 1..3 tentative, 5 confirmed, 6..9 coasting */
  int32_t is_static;    /* isStaticVec[id] */
  int32_t is_vis;       /* isVisVec[id] */
  float px, py, pz;     /* targetPoints[id] (pz = -0.865) */
  int32_t lifetime;     /* UKF::lifetime_ */
  double v, yaw;        /* targetVandYaw[id] = {x_merge(2), x_merge(3)+egoYaw wrapped} */
  float vis_box[24];    /* BBox_ (8 corners x,y,z) when is_vis, else zeros */
} mot_track;

/* full filter state of one track, for parity checks against the reference's targets_[id] */
typedef struct mot_track_state {
  double x_merge[5], x_cv[5], x_ctrv[5], x_rm[5];
  double p_merge[25], p_cv[25], p_ctrv[25], p_rm[25]; /* row-major 5x5 */
  double mode_prob[3];                                 /* CV, CTRV, RM */
  double z_pred[3][2], s[3][4], k[3][10];              /* zPred*l_, lS_*_, K_*_ (5x2 row-major) */
  double init_meas[2], dist_from_init, best_yaw;
  int32_t lifetime, track_manage, is_static, is_vis, has_best_box, _pad;
  float bbox[24], best_bbox[24];
} mot_track_state;

typedef struct mot_ctx mot_ctx;

/* ---------------------------------------------------------------- lifecycle */
int mot_abi_version(void);
int mot_params_preset(int preset, mot_params* out);
/* device: HIP device ordinal. max_points: capacity per frame. max_batch: number of stream slots (>=1).
 * max_tracks_total: track SLOTS per stream = how many tracks may be alive (or dead since the last step) at the same time.
 * The reference never frees a track (targets_ only grows, OT/tracking/imm_ukf_jpda.cpp:972-989) and addresses tracks by their
 * index in that vector; here the filter state (~2 KB) of a track is evicted one step after the track died, while the index
 * keeps counting: ids, output order and every result stay those of the reference with unbounded memory. Per track EVER
 * created 44 bytes remain (its last position, frozen speed and yaw — the reference's merge step tests dead tracks' positions too — lifetime and
 * static flag): mot_params.max_tracks_ever of them, 64 x max_tracks_total by default. A birth that finds no slot or exceeds
 * that budget is dropped and reported (MOT_E_CAPACITY, sticky). */
int mot_create(const mot_params* params, int device, int max_points, int max_batch,
               int max_tracks_total, mot_ctx** out);
void mot_destroy(mot_ctx* ctx);
/* forget all tracker state of every slot (the reference cannot: file-scope globals,
 * OT/tracking/imm_ukf_jpda.cpp:19-24,56-70) */
int mot_reset(mot_ctx* ctx);
/* the same for one stream */
int mot_reset_slot(mot_ctx* ctx, int slot);
/* forget the TRACKS of one stream but keep its dead-reckoned ego pose, i.e. the origin of its global frame: what a long-running
 * node wants when a stream has used up max_tracks_total (mot_reset_slot would re-origin /global at the current pose and make
 * every published position jump). The next tracker step of the slot behaves like the reference's first frame (one seeded
 * track, OT/tracking/imm_ukf_jpda.cpp:741-795). */
int mot_reset_tracks_slot(mot_ctx* ctx, int slot);
/* Checkpoint / resume of ONE stream's tracker (the reference keeps this state in file-scope globals,
 * OT/tracking/imm_ukf_jpda.cpp:19-24,56-70, and can neither save nor reset it). mot_stream_save writes everything the next
 * frame of the stream depends on — the filter state of every track slot, the per-track-ever arrays, the live / just-died lists,
 * the last step's outputs, the dead-reckoned ego pose and timestamps — into a block of HOST memory that holds no pointers;
 * mot_stream_load puts it into any slot of any context of the same library version with the same max_tracks_total (another GPU,
 * another process, after a restart; max_tracks_ever at least the stream's track count), and the stream continues bit for bit:
 * the next mot_get_tracks returns what it returned before the save, the next step what it would have computed. Both calls
 * synchronise the context's stream. mot_stream_snapshot_size: the upper bound for this context (a snapshot is shorter when
 * the stream has created fewer than max_tracks_ever tracks; *written says how long). Errors: MOT_E_CAPACITY (blob too small;
 * more tracks than the loading context's max_tracks_ever), MOT_E_ARG (not a snapshot, another version, another slot count,
 * truncated) — a failed load leaves the slot as it was. */
int mot_stream_snapshot_size(mot_ctx* ctx, size_t* bytes);
int mot_stream_save(mot_ctx* ctx, int slot, void* blob, size_t capacity, size_t* written);
int mot_stream_load(mot_ctx* ctx, int slot, const void* blob, size_t bytes);
/* the parameters the context was created with */
int mot_get_params(const mot_ctx* ctx, mot_params* out);
/* ctx == NULL: why the calling thread's last mot_create() failed (which field of mot_params it refused). That string belongs
 * to the calling thread and is valid until its next mot_create(); a context's string until the next call on the context. */
const char* mot_last_error(const mot_ctx* ctx);
int mot_synchronize(mot_ctx* ctx);
/* the HIP stream (hipStream_t) the context launches on, for callers that enqueue their own work */
void* mot_stream(mot_ctx* ctx);

/* ---------------------------------------------------------------- stage entry points, HOST buffers
 * (copy in, run, copy out, synchronise — the literal drop-in for the reference call sites) */

/* replaces groundRemove(cloud, elevatedCloud, groundCloud), OT/include/ground_removal.h:62-64.
 * xyzw: n x 4 floats. elevated/ground: caller buffers of capacity n x 4 floats, filled in input
 * order (the reference push_backs in input order, ground_removal.cpp:221-247). mask (optional, n bytes). */
int mot_ground_remove(mot_ctx* ctx, const float* xyzw, int n, float* elevated_xyzw, int* n_elevated,
                      float* ground_xyzw, int* n_ground, uint8_t* mask);

/* replaces componentClustering(elevatedCloud, cartesianData, numCluster),
 * OT/include/component_clustering.h:20-22. grid: num_grid x num_grid int32, x-major
 * (grid[x*num_grid+y] == cartesianData[x][y]); labels 1..num_cluster in raster order of first cell.
 * point_label (optional, n int32): label of the cell each point falls in, 0 if none / outside ROI.
 * grid may be NULL when only the resident result is needed (mot_box_fit_resident, mot_cluster_products). */
int mot_cluster(mot_ctx* ctx, const float* elevated_xyzw, int n, int32_t* grid, int* num_cluster,
                int32_t* point_label);

/* replaces boxFitting(elevatedCloud, cartesianData, numCluster, ma), OT/include/box_fitting.h:34-36.
 * boxes: capacity max_boxes x 8 x 3 floats (4 bottom corners z=-sensor_height, 4 top corners z=maxZ,
 * box_fitting.cpp:379-389). box_cluster (optional): 1-based cluster id of each emitted box.
 * n_undefined (optional): clusters whose result is undefined behaviour in the reference
 * (uninitialised reads); they are rejected here.
 * LABEL RANGE: the device's label grid is 16 bits wide (a frame has at most 4096 clusters). A grid value outside 0..num_cluster
 * names no cluster — getClusteredPoints would index past its per-cluster vectors with it (box_fitting.cpp:59-66) — and is read as 0. */
int mot_box_fit(mot_ctx* ctx, const float* elevated_xyzw, int n, const int32_t* grid, int num_cluster,
                float* boxes, int max_boxes, int* n_boxes, int32_t* box_cluster, int* n_undefined);

/* mot_box_fit on the elevated cloud and label grid that mot_cluster left resident (slot 0): the cluster node calls
 * componentClustering and boxFitting back to back on the same cloud (OT/src/cluster/main.cpp:74,119) — one upload serves both. */
int mot_box_fit_resident(mot_ctx* ctx, float* boxes, int max_boxes, int* n_boxes, int32_t* box_cluster, int* n_undefined);

/* fromROSMsg(*input, *cloud) + groundRemove (OT/src/groundremove/main.cpp:100,120) for a sensor_msgs/PointCloud2 payload in
 * HOST memory: data = n_points records of point_step bytes, the FLOAT32 fields x, y, z at the given byte offsets. One H2D
 * copy of the raw records, unpacked on the device (mot_decode_pointcloud2_dev), then exactly mot_ground_remove; with
 * params.crop_enable the node's PassThrough / ConditionalRemoval pre-filter runs fused in the first kernel. The 4th float
 * of every output point is 1.0f — what pcl::PointXYZ's padding holds — so the outputs are toROSMsg payloads as they are. */
int mot_ground_remove_pointcloud2(mot_ctx* ctx, const void* data, int n_points, int point_step, int off_x, int off_y, int off_z,
                                  float* elevated_xyzw, int* n_elevated, float* ground_xyzw, int* n_ground, uint8_t* mask);

/* The stateless chain of one frame — fromROSMsg, groundRemove, componentClustering, boxFitting, as OT0/src/main.cpp:57-88 runs
 * them in a single process — on a PointCloud2 payload in HOST memory: one upload, every intermediate stays in HBM (slot 0).
 * Asynchronous; read the results back with mot_get_ground / mot_get_clusters / mot_get_boxes / mot_cluster_products(slot 0). */
int mot_frame_pointcloud2(mot_ctx* ctx, const void* data, int n_points, int point_step, int off_x, int off_y, int off_z);

/* replaces getOriginPoints(timestamp, originPoints, v_gps, yaw_gps), OT/include/imm_ukf_jpda.h:15.
 * origin6 = {x, y, yaw, x, y, yaw + pi/2}. Must be called before mot_track_step of the same frame,
 * like OT/tracking/main.cpp:74. */
int mot_ego_update(mot_ctx* ctx, int slot, double timestamp, double v_gps, double yaw_gps, double* origin6);

/* replaces immUkfJpdaf(bBoxes, timestamp, ...), OT/include/imm_ukf_jpda.h:19-22.
 * boxes_global: m x 8 x 3 floats in the global frame. tracks: capacity max_tracks records — one per track EVER created on the
 * stream (see mot_get_tracks for sizing and the two meanings of MOT_E_CAPACITY). A THIRD one here: m > MOT_MAX_BOXES_PER_FRAME is
 * refused before anything runs — the step has NOT been taken, *n_tracks = -1 says so (the other two deliver n_tracks >= 0). */
#define MOT_MAX_BOXES_PER_FRAME 1024
int mot_track_step(mot_ctx* ctx, int slot, const float* boxes_global, int m, double timestamp,
                   mot_track* tracks, int max_tracks, int* n_tracks);
/* ---- the per-tick gather of the live tracks across GPUs, native (ABI v6) ------------------------------------------------------------
 * BASELINE.json's partitioning: sensor streams shard across the GPUs of a node, one process per GPU; the only exchange is ONE all-gather
 * per frame tick of every rank's packed live-track blocks (mot_export_tracks_packed_dev's layout, one block per context) — RCCL over
 * xGMI, enqueued from C on a side stream behind the contexts' export kernels: no host synchronisation, no Python / torch in the loop.
 * RCCL is looked up at run time (the library already in the process, else librccl.so): MOT_E_STATE when there is none.
 *   mot_gather_unique_id(id128)            rank 0: 128 bytes (ncclGetUniqueId) the launcher hands to every rank
 *   mot_gather_create(ctxs, n_ctx, batch, capacity_records, world, rank, id128, &g)
 *                                          this rank's contexts (one device); capacity_records = records ONE context's block holds for all its
 *                                          `batch` streams together; id128 NULL with world 1: no communicator, the tick's collective is a copy
 *   mot_gather_contribute(g, ci)           after context ci's frame tick, from ITS issuing thread (thread-safe: a thread per context, or one for
 *                                          all): exports the block on the context's stream; the call that completes a tick enqueues the collective.
 *                                          Every rank contributes every context once per tick; a context runs at most one tick ahead of the slowest
 *   mot_gather_result(g, &d_blocks, &block_bytes, &tick, &done_event)
 *                                          the last completed tick's receive buffer on the device, [world][n_ctx] blocks of block_bytes; complete
 *                                          when done_event (a hipEvent_t) has fired / after mot_gather_synchronize; rewritten by the tick after next
 *   mot_gather_synchronize / mot_gather_destroy / mot_gather_last_error */
typedef struct mot_gather mot_gather;
int mot_gather_unique_id(void* id128);
int mot_gather_create(mot_ctx* const* ctxs, int n_ctx, int batch, int capacity_records, int world, int rank, const void* id128, mot_gather** out);
int mot_gather_contribute(mot_gather* g, int ctx_index);
int mot_gather_result(mot_gather* g, const void** d_blocks, long* block_bytes, long* tick, void** done_event);
int mot_gather_synchronize(mot_gather* g);
int mot_gather_destroy(mot_gather* g);
const char* mot_gather_last_error(const mot_gather* g);

/* filter state of track `id` (reference index) on `slot` (parity/debug); MOT_E_STATE once the track has been dead for more than a step */
int mot_track_get_state(mot_ctx* ctx, int slot, int id, mot_track_state* out);

/* ---------------------------------------------------------------- fused frame, DEVICE buffers
 * One sensor frame per slot through ground -> cluster -> box -> (optional) tracker with every
 * intermediate left in HBM. d_xyzw: max_batch frames, frame b at d_xyzw + b*frame_stride floats.
 * n_points[b] host array. timestamps/ego (host arrays of length batch) feed the tracker when
 * run_tracker != 0; boxes are then taken in the sensor frame transformed to the global frame with
 * the dead-reckoned ego pose (what OT/tracking/main.cpp:143-158 does through tf).
 * Asynchronous: results are read back with the mot_get_* calls below (which synchronise). */
int mot_frames_dev(mot_ctx* ctx, const float* d_xyzw, long frame_stride, const int* n_points, int batch,
                   int run_tracker, const double* timestamps, const double* ego_v, const double* ego_yaw);

/* SEQUENCE MODE: `frames` CONSECUTIVE frames of ONE sensor stream in one call (BASELINE.json configs[3] as written — a recorded drive
 * replayed; the reference's single-process precedent runs one callback per frame, OT0/src/main.cpp:51-375). Frame k of the sequence is
 * at d_xyzw + k*frame_stride floats; n_points / timestamps / ego_v / ego_yaw are host arrays of length `frames` (frames <= max_batch).
 * The stateless stages (groundRemove, componentClustering, boxFitting) of all frames run as ONE batch — slot k of the context holds
 * frame k afterwards: mot_get_ground / mot_get_clusters / mot_get_boxes(slot k) read its results — and the tracker
 * (immUkfJpdaf, OT/tracking/imm_ukf_jpda.cpp:704-1112: sequential by nature) runs `frames` steps chained on the device on the track state
 * of stream (slot) 0, step k taking frame k's boxes through the ego pose of frame k. Results are those of `frames` calls of
 * mot_frames_dev(batch 1) in a row, bit for bit. Optional per-frame track records: the LIVE tracks after step k (mot_export_tracks_dev's
 * records) go to d_tracks[k][max_per_frame] / d_counts[k] (device pointers; both NULL: none). After the call mot_get_tracks(slot 0) /
 * mot_track_get_state(slot 0) see the state after the last frame. Asynchronous. */
int mot_sequence_dev(mot_ctx* ctx, const float* d_xyzw, long frame_stride, const int* n_points, int frames,
                     const double* timestamps, const double* ego_v, const double* ego_yaw,
                     void* d_tracks, int max_per_frame, int32_t* d_counts);

/* Which by-products of the ground stage the FUSED entry points (mot_frames_dev, mot_frames_host, mot_frame_pointcloud2) write
 * besides what the next stage needs: flags = OR of MOT_OUT_GROUND / MOT_OUT_MASK / MOT_OUT_LABELS, default 0. The reference's own fused
 * precedent never touches groundCloud after groundRemove (OT0/src/main.cpp:63-79), and the ground cloud is a quarter of the
 * compaction kernel's HBM traffic. Nothing is lost with the default: mot_get_ground materialises the ground cloud / mask of
 * the LAST batch on demand — and, since ABI v5, the ELEVATED cloud as float4 records too (between its stages the fused path keeps the
 * elevated points as 12-byte {x, y, z}: nothing after groundRemove reads the 4th float). A mot_get_ground that asks for a cloud or the
 * mask after a fused call re-runs the compaction from the batch's input, polar cells and thresholds, all still resident —
 * so with mot_frames_dev the caller's input buffer must be unchanged until then; a stage-wise mot_cluster / mot_box_fit /
 * mot_cluster_products_host / mot_cluster_node_frame in between takes slot 0 for itself and ends that possibility: MOT_E_STATE (the batch's
 * OTHER slots keep everything else readable after such a call — labels, side products, boxes, cubes: the library knows per slot which layout
 * the elevated cloud has). Likewise the per-point cluster labels
 * (getClusteredPoints, OT/src/cluster/box_fitting.cpp:46-72: the box stage itself works on a cluster-sorted index and never reads
 * them back): mot_get_clusters(point_label) computes them for the slot it is asked about, from the cells and the label grid still
 * resident. Sticky per context. The stage-wise mot_ground_remove / mot_cluster always deliver all their outputs
 * (OT/src/groundremove/ground_removal.cpp:226-247). */
int mot_set_fused_outputs(mot_ctx* ctx, int flags);

/* The order the library may assume of an input cloud's points. MOT_ORDER_SCAN (default): the box stage describes a cluster by its groups in the
 * cloud as it lies, which is compact for scans in beam-major or firing order; a cloud in no order is slow there and can be refused (the group limit
 * under mot_get_ground). MOT_ORDER_ANY: for merged, voxel- or KD-tree-filtered clouds and non-repetitive scanners. Every entry point that runs the box
 * stage — mot_frames_dev, mot_frames_host*, mot_frame_pointcloud2, mot_sequence_dev, mot_box_fit, mot_box_fit_resident, mot_cluster_node_frame — first
 * puts the frame's elevated points into cluster order on the device (a stable sort by cluster label; unlabelled points are kept, in front) and fits
 * the boxes on that internal copy, as the reference's getClusteredPoints copies the cloud into one vector per cluster (box_fitting.cpp:46-72). Every
 * result equals MOT_ORDER_SCAN's bit for bit on any frame that mode accepts — boxes, box_cluster, n_undefined, mot_box_markers, tracks — and
 * everything the caller reads keeps the INPUT order: per-point labels, the elevated / ground clouds, the side products. No frame is refused for its
 * groups; the cluster and box limits hold in both modes with their own messages. Cost: the extra pass (48 bytes per elevated point).
 * Sticky per context. The mode's buffers (24 bytes per point and slot) are allocated by the first MOT_ORDER_ANY request: MOT_E_HIP if that fails, and
 * the mode stays as it was. Switching leaves every resident result readable, and drops the captured launch graphs. Unknown order: MOT_E_ARG. */
int mot_set_point_order(mot_ctx* ctx, int order);

/* ---------------------------------------------------------------- boxes and points linked to their tracks (additions within ABI v6)
 * Which track does a box — and every elevated point of its cluster — belong to? The tracker decides that itself: the reference's matchingVec
 * (OT/tracking/imm_ukf_jpda.cpp:205-257, 806, 974-989). on != 0: every tracker step keeps that association as a row of BOX OWNERS per slot, and every
 * fused call that runs the tracker (mot_frames_*, mot_frame_pointcloud2 with the tracker, mot_sequence_dev) ends with one more streaming kernel that
 * composes elevated point -> cell -> cluster label -> box -> owner on the device. Default off: nothing is launched, written or allocated, and every other
 * output is byte-identical either way. Sticky per context. The buffers (4 bytes x max_points + 4 KB per slot) are allocated by the first request:
 * MOT_E_HIP if that fails, and the mode stays as it was. Switching drops the captured launch graphs (the kernel is part of the captured sequence) and
 * forgets the rows: the getters below answer MOT_E_STATE until the next step. Not stream state: mot_stream_save / _load do not carry it.
 * Cost (profiles/track_links.md; 512 streams x 120 k points per launch): on, 0.93 x the frames/s of off; the kernel alone 59 us per 512 frames. Off: 0.999 x a library without it.
 *
 * OWNER of box i of a step's box list = the id (mot_track.id, the reference's index into targets_) of
 *   - the track that turned matchingVec[i] from 0 to 1: tracks are walked in id order; a track skipped by a guard (dead, diverged: :826-851) claims
 *     nothing; a track in its second initialisation (trackManage 1) marks only its progressive NIS minima (:238-245) and owns those nobody claimed
 *     before; every other track claims every box inside its gate that nobody claimed before. A box inside two gates belongs to the lower id.
 *   - or, for a box nobody claimed, the track born from it (:974-989): ids n_ever_before, n_ever_before + 1, ... in box order; -1 if the birth was
 *     dropped (no free track slot, or max_tracks_ever reached).
 *   - first frame of a stream (:741-795): the box at seed_box_index owns track 0 (the reference looks at no other box, and seeds nothing when the
 *     frame has no such box); every other box -1.
 * The owner is the track that CLAIMED the box, also when that track ends the same step dead (the state machine, or mergeOverSegmentation): consumers
 * check track_manage of the id, as for every other use of a track. Identical in every tracker mode (mot_set_tracker_mode). */
int mot_set_track_links(mot_ctx* ctx, int on);
/* owners of the slot's LAST tracker step, in the order of that step's box list (fused calls: mot_get_boxes' order): box_track[0 .. *n_boxes - 1]. Valid
 * after mot_frames_*, mot_sequence_dev (slot k = frame k), mot_track_step, mot_track_steps_dev and mot_tracking_node_frame. MOT_E_STATE when links are
 * off or no step was taken on the slot since they were turned on; MOT_E_CAPACITY (n_boxes delivered, nothing copied) when max_boxes is too small,
 * and with the limit's message when the step's boxes came from a fused frame that was refused (the per-frame limits under mot_get_ground). */
int mot_get_box_tracks(mot_ctx* ctx, int slot, int32_t* box_track, int max_boxes, int* n_boxes);
/* track id of every elevated point of the slot, in the elevated cloud's INPUT order (mot_get_ground's, mot_get_clusters' point_label order; the same in
 * MOT_ORDER_ANY): ids[i] = owner of the box of point i's cluster; -1 when the point lies in no cluster, the cluster was not kept as a box (min_points, the
 * rule-based filter, an undefined fit) or the box has no owner. Equals the composition of mot_get_clusters(point_label), mot_get_boxes(box_cluster) and
 * mot_get_box_tracks. Valid only while the slot's cloud, boxes and tracker step come from ONE fused call: MOT_E_STATE after a stage-wise call took the slot
 * (mot_cluster, mot_box_fit, mot_ground_remove, ...: slot 0; the other slots stay readable), after a fused call without the tracker, or after a tracker step
 * fed from outside (mot_track_step, mot_track_steps_dev, mot_tracking_node_frame). MOT_E_CAPACITY with the limit's message on a refused frame, and
 * (n_elevated delivered, nothing copied) when `capacity` is too small. */
int mot_get_point_tracks(mot_ctx* ctx, int slot, int32_t* ids, int capacity, int* n_elevated);
/* the same ids of slots 0..batch-1 into a caller-owned DEVICE block: d_ids[b * stride + i] (int32, 4-byte aligned; 16-byte aligned slots are written
 * 16 bytes at a time), and every slot's elevated count into d_counts[b]. A slot with more elevated points than `stride` gets the first `stride` ids
 * (d_counts carries the true count). Asynchronous on the context stream, nothing is read back: a refused frame reads -1 throughout here (mot_get_point_tracks
 * tells). Same validity rule, for every slot of the batch. */
int mot_export_point_tracks_dev(mot_ctx* ctx, int batch, int32_t* d_ids, long stride, int32_t* d_counts);

/* ---------------------------------------------------------------- per-track point clouds (additions within ABI v6)
 * "Which track" turned into "that track's points": the slot's elevated points STABLY PARTITIONED by owning track, on the device — what accumulating an
 * object's points over frames and cutting dynamic objects out of a map start from (INTEGRATION.md has a recipe for each). For a slot whose point chain is
 * valid (the rule of mot_get_point_tracks: cloud, boxes and tracker step from ONE fused call, links on).
 *
 * SEGMENTS: one per distinct id >= 0 in the step's owner row (mot_get_box_tracks), in ascending id, whether or not a point carries the id; a track that
 * claimed several boxes gets ONE segment with the points of all its clusters and n_boxes > 1. With MOT_TRACK_POINTS_REST a last segment, track_id -1,
 * n_boxes 0, holds every point whose id is -1 (no cluster, a cluster not kept as a box, a box nobody owns); the segment is there even when it is empty.
 * Without the flag those points are left out. Segments lie back to back: first of segment k + 1 = first + count of segment k, the first one starts at 0.
 * POINTS of a segment keep the elevated cloud's INPUT order (index strictly ascending), also in MOT_ORDER_ANY. index = the point's position in that order:
 * mot_get_ground's elevated cloud, mot_get_clusters' point_label, mot_get_point_tracks — what a caller fetches intensity, or anything it keeps per point, by.
 * frame = MOT_FRAME_SENSOR: x, y, z are the elevated point's bits, untouched. MOT_FRAME_GLOBAL: its image under the float 3 x 4 matrix the slot's boxes took
 * in that fused call — global_from_sensor of mot_sensor_pose read right after the call, applied as that comment states (fp32, left to right, no contraction);
 * in mot_sequence_dev slot k has frame k's matrix. The library keeps the 48 bytes per slot on the host while links are on and sends them ahead of the
 * kernels in one stream-ordered copy (page-locked ring: no host synchronisation). Any other frame, or unknown flag bits: MOT_E_ARG.
 *
 * mot_export_track_points_dev: slots 0..batch-1 into caller-owned DEVICE blocks, d_points[b * point_stride + i] and d_segments[b * max_segments + k] (4-byte
 * aligned; a slot that starts on 16 bytes is written one 16-byte store per record), d_counts[2 b] = the slot's segments, d_counts[2 b + 1] = its records — the
 * TRUE numbers: a slot with more records than point_stride gets the first point_stride, one with more segments than max_segments the first max_segments,
 * nothing beyond a slot's own records is written. Asynchronous on the context stream, nothing is read back: a frame refused for capacity has no owners here
 * (as in mot_export_point_tracks_dev) — one rest segment with all its points under MOT_TRACK_POINTS_REST, nothing otherwise. MOT_E_STATE under exactly the
 * conditions of mot_export_point_tracks_dev, tested for every slot of the batch before anything is launched.
 * mot_get_track_points: one slot to the host (synchronises). *n_points / *n_segments are always delivered; MOT_E_CAPACITY with nothing copied when either
 * buffer is too small, and with the limit's message on a refused frame. MOT_E_STATE as mot_get_point_tracks.
 *
 * Four kernels per call (csrc/track_points.hip), none in any other call: 36 bytes moved per elevated point plus 12 bytes per (1024-point chunk, segment)
 * against the 32 of a plain copy into such records. Scratch, allocated at the first call and kept until mot_destroy (MOT_E_HIP if that fails; the next call
 * resumes): per slot 4100 bytes per 1024 points of max_points (rounded up) + 8 KB + 56 bytes, and 832 bytes x max_batch page-locked; mot_get_track_points adds one
 * block of 16 bytes x max_points + 17 KB per context at ITS first call. Cost (profiles/track_points.md; 512 streams x 120 k points per call): 202 - 266 us, 1.6 - 2.1 x a device-to-device copy of the same bytes. */
enum { MOT_TRACK_POINTS_REST = 1 };            /* flags */
typedef struct mot_track_segment {             /* 16 bytes */
  int32_t track_id;   /* mot_track.id; -1: the rest segment */
  int32_t first;      /* index of the segment's first record in the slot's point block */
  int32_t count;      /* its records */
  int32_t n_boxes;    /* boxes of the step's owner row that carry this id (0 for the rest segment) */
} mot_track_segment;
typedef struct mot_track_point { float x, y, z; int32_t index; } mot_track_point;   /* 16 bytes */
int mot_export_track_points_dev(mot_ctx* ctx, int batch, int flags, int frame,
        mot_track_point* d_points, long point_stride,          /* records per slot */
        mot_track_segment* d_segments, int max_segments,       /* records per slot */
        int32_t* d_counts /* [batch][2]: segments, points - the TRUE numbers */);
int mot_get_track_points(mot_ctx* ctx, int slot, int flags, int frame,
        mot_track_point* points, int point_capacity, mot_track_segment* segments, int max_segments,
        int* n_points, int* n_segments);

/* ---------------------------------------------------------------- per-track accumulators (additions within ABI v6)
 * The last step of the chain above, on the device: every track's points ACCUMULATED OVER FRAMES, in the tracker's global frame, with a log of the track's pose
 * at each contributing step beside them (so a consumer can re-centre the points on the object: INTEGRATION.md, "object-centred cloud"). One call after a fused
 * step appends that step; nothing is launched, written or allocated unless the feature is turned on and called.
 *
 * LAYOUT. One accumulator per TRACK SLOT of a stream — max_tracks_total of them, the tracker's own bounded set of objects alive (or dead since the last step) at
 * once; a slot freed by a dead track goes to a later birth, and the accumulator goes with it. Per slot: a ROW (below), a ring of points_per_track = K points and
 * a ring of obs_per_track = O observations. The row of the track that holds slot r of stream b is d_rows[b * T + r]; its rings start at d_points[(b * T + r) * K]
 * and d_obs[(b * T + r) * O]. RING RULE: the record appended as number t (0-based, row.total / row.obs_total count them) lies at position t & (K - 1) resp.
 * t & (O - 1); kept = min(total, K) points, the oldest of them at position total & (K - 1) once the ring has wrapped, at 0 before.
 *
 * mot_set_track_accumulation(K, O): K a power of two in [64, 2^20], O 0 (no log, d_obs null) or a power of two in [1, 4096], else MOT_E_ARG. K = 0 turns the
 * feature off and frees its memory (draining the context stream). Needs mot_set_track_links on (MOT_E_STATE otherwise), and while accumulation is on
 * mot_set_track_links(0) answers MOT_E_STATE. Allocates max_batch x max_tracks_total x (16 K + 48 O + 32) bytes plus 8 KB of scratch per slot; MOT_E_HIP when
 * that fails, and the mode (an earlier geometry included) stays as it was. All rows start empty (track_id -1, everything else 0) and every slot's step counter
 * at 0, also when the geometry changes; the same geometry again changes nothing. The accumulators are NOT stream state: mot_stream_save / mot_stream_load do not
 * carry them. mot_reset, mot_reset_slot, mot_reset_tracks_slot and mot_stream_load empty the rows of the slots they touch and restart those slots' step counters
 * (ids restart there, so the rows must), stream-ordered and without a host synchronisation; the step those slots hold can then no longer be appended.
 *
 * mot_accumulate_track_points(batch): appends the latest fused step of slots 0..batch-1. Asynchronous on the context stream, nothing is read back. Validity is
 * tested for every slot before anything is launched, and a refused call appends nothing and counts no step: MOT_E_STATE under the conditions of
 * mot_export_point_tracks_dev (cloud, boxes and tracker step from ONE fused call, links on), and also
 *   - after mot_sequence_dev: there slot k is frame k of ONE stream, and the id -> slot map of the intermediate frames is gone when the call returns.
 *     This call does not serve sequence mode; mot_sequence_accumulate_dev (below) appends a sequence's frames inside the sequence call.
 *   - when a slot of the batch was already accumulated for its current step (a step is appended at most once), or was reset / loaded since that step.
 * STEP STAMP of a slot = the number of accepted accumulate calls that covered the slot before this one (0, 1, ...; counted on the host, it travels with the
 * slots' matrices in one stream-ordered copy). A frame refused for capacity has no owners: it appends nothing, its step still counts.
 * APPENDING: every segment of the step as mot_export_track_points_dev defines it without MOT_TRACK_POINTS_REST (the distinct ids >= 0 of the owner row, points
 * in input order; points without owner are not accumulated). Segment of id with n points: the row is that of the track's slot; when the row holds another id
 * it restarts (total 0, obs_total 0, first_step = this step, track_id = id) — this is how a slot taken by a new track drops the old track's points; a dead
 * track's row stays readable until then. Point j of the segment goes to ring position (total + j) & (K - 1), for j >= n - K only (one frame with more than K
 * points of a track keeps the last K), as {x, y, z, step}: x, y, z the very bits the MOT_FRAME_GLOBAL export writes. Then total += n, last_step = this step,
 * and when O > 0 one observation goes to position obs_total & (O - 1) and obs_total counts it (with O = 0 obs_total stays 0). A segment of 0 points still
 * leaves its observation. OBSERVATION: copied, not recomputed, from the mot_track record the same step wrote for the id — what mot_get_tracks returns for it
 * right after the fused call; count = n, n_boxes = the segment's.
 *
 * READERS (MOT_E_STATE while the feature is off). mot_track_accumulators_dev: the device pointers, no copy — for consumers on the context stream (or behind
 * an event on it). mot_get_accum_rows: the slot's max_tracks_total rows to the host (synchronises); *n_rows is delivered, MOT_E_CAPACITY with nothing copied
 * when max_rows is smaller. mot_get_track_accumulated: the row that holds track_id — MOT_E_STATE with a message when none does (never accumulated, or its slot
 * went to another track) — its kept points and observations in CHRONOLOGICAL order, the ring unrolled, oldest first (synchronises). *n_points / *n_obs are
 * always delivered; a null buffer is not filled and not tested; MOT_E_CAPACITY with nothing copied when a buffer that was given is too small.
 *
 * Kernels (csrc/track_accum.hip): the table and count kernels of the per-track point clouds, a plan kernel (one workgroup per frame) and a scatter kernel —
 * 36 bytes moved per owned point, as mot_export_track_points_dev, nothing staged in between. Cost: unmeasured (profiles/track_accum.md; tools/time_track_accum.py
 * measures it against that export and a device-to-device copy). */
typedef struct mot_accum_row {      /* 32 bytes; one per TRACK SLOT of a stream */
  int32_t  track_id;                /* mot_track.id of the track the row holds; -1: empty */
  int32_t  first_step, last_step;   /* the slot's accumulation steps of the first / latest append */
  int32_t  obs_total;               /* observations ever logged for this track */
  uint64_t total;                   /* points ever appended for this track; kept = min(total, points_per_track) */
  uint64_t reserved;                /* 0 */
} mot_accum_row;
typedef struct mot_accum_point { float x, y, z; int32_t step; } mot_accum_point;   /* 16 bytes, MOT_FRAME_GLOBAL */
typedef struct mot_accum_obs {      /* 48 bytes: the track as the step that contributed left it */
  int32_t step, count, n_boxes, track_manage;   /* the step stamp, the segment's points and boxes, mot_track.track_manage */
  float   px, py;  int32_t is_static, lifetime; /* mot_track.px, .py (global frame), .is_static, .lifetime */
  double  v, yaw;                               /* mot_track.v, .yaw */
} mot_accum_obs;
typedef struct mot_accum_view {     /* device pointers of the context's accumulators, valid until they are turned off (or their geometry changes) or the context is destroyed */
  const mot_accum_row* d_rows;      /* [max_batch][tracks_per_slot] */
  const mot_accum_point* d_points;  /* [max_batch][tracks_per_slot][points_per_track], a ring per row */
  const mot_accum_obs* d_obs;       /* [max_batch][tracks_per_slot][obs_per_track], a ring per row; null when obs_per_track == 0 */
  int32_t tracks_per_slot, points_per_track, obs_per_track, max_batch;
} mot_accum_view;
int mot_set_track_accumulation(mot_ctx* ctx, int points_per_track, int obs_per_track);
int mot_accumulate_track_points(mot_ctx* ctx, int batch);
int mot_track_accumulators_dev(mot_ctx* ctx, mot_accum_view* out);
int mot_get_accum_rows(mot_ctx* ctx, int slot, mot_accum_row* rows, int max_rows, int* n_rows);
int mot_get_track_accumulated(mot_ctx* ctx, int slot, int track_id, mot_accum_row* row,
        mot_accum_point* points, int point_capacity, int* n_points,
        mot_accum_obs* obs, int obs_capacity, int* n_obs);

/* ---------------------------------------------------------------- a recorded drive into the accumulators (addition within ABI v6)
 * mot_sequence_accumulate_dev IS mot_sequence_dev — the same arguments, the same launch sequence — and appends all `frames` steps to the accumulators of stream
 * (slot) 0 in the same asynchronous call: nothing is read back, no host synchronisation. What mot_accumulate_track_points cannot do after mot_sequence_dev
 * (the id -> slot map of the intermediate frames is gone when that call returns) is done inside the call: a small kernel behind every tracker step keeps what
 * the next step moves, and behind the last step all frames are appended at once.
 *
 * RESULT. The accumulators hold, bit for bit, what `frames` rounds of { mot_frames_dev(batch 1) on frame k; mot_accumulate_track_points(ctx, 1) } would have
 * left in slot 0 — its rows, the kept part of their rings (RING RULE above) and the logs — from the same tracker and accumulator state. Ring and log positions
 * outside a row's kept range are undefined, as they are after a restart. Every other result is byte-identical to mot_sequence_dev's: slot k = frame k for
 * mot_get_ground / _clusters / _boxes / _box_tracks / _point_tracks / _track_points, the tracker state, d_tracks / d_counts.
 * ROWS: those of slot 0, d_rows[0 * T + r], with the rings beside them; the rows of slots >= 1 are not touched. The accumulators stay sized max_batch x
 * max_tracks_total (mot_set_track_accumulation): a context used for sequences only fills slot 0's.
 * STEP STAMPS: frame k gets (slot 0's step counter) + k and the counter advances by `frames`; a frame refused for capacity appends nothing and still counts.
 * Calls chain: frame-by-frame steps on slot 0 (mot_frames_dev batch 1 + mot_accumulate_track_points) before and after, several sequence calls in a row (a
 * drive replayed in chunks) — all continue the same rows and the same counter.
 * AFTER THE CALL the slots are sequence slots, as after mot_sequence_dev: mot_accumulate_track_points answers MOT_E_STATE on them (nothing is appended twice).
 * mot_reset* and mot_stream_load empty slot 0's rows and restart its counter as they always do. mot_export_track_models_dev / mot_get_track_models on slot 0
 * work unchanged on the result; MOT_MODEL_CURRENT refers to the step of the last frame.
 * REFUSALS, each before anything has run (the tracker has not stepped): MOT_E_STATE unless mot_set_track_links and mot_set_track_accumulation are on; the
 * argument errors of mot_sequence_dev; MOT_E_HIP when the scratch of the call's own (72 KB per slot of max_batch: what every step leaves behind and the plan of
 * every frame's segments) cannot be had at the first call — both blocks or neither, the next call tries again. That scratch — and, at a first use, the scratch of
 * the per-track point clouds — is all the call allocates; it is released with the accumulators (mot_set_track_accumulation(0, ...) or another geometry) and by
 * mot_destroy. mot_sequence_dev itself launches, writes and allocates what it always did, with accumulation on or off.
 * WITHIN ONE CALL frames meet in a ring (many frames bring more than K points of a track between them; a track slot goes to a new track in mid-call): every
 * ring and log position is written by at most one record of the call — only the segments of a row's FINAL id contribute, only its last K points and last O
 * observations are written — so the result does not depend on the order in which workgroups run.
 * Kernels (csrc/track_accum_seq.hip): one capture launch per step; behind the chain the table and count kernels of the per-track point clouds over all frames,
 * a per-frame segment kernel, ONE serial plan workgroup that walks the frames in order, a finish kernel (logs, kept ranges) and the scatter — six launches
 * whatever `frames` is. Cost (profiles/track_accum_sequence.md, tools/time_track_accum_sequence.py; one 154-frame drive of 120 k-point frames, K = 4096, O = 16):
 * 8.17 ms per call against 7.71 ms of mot_sequence_dev alone (+ 0.46 ms, 3.2 us per frame) and 31.1 ms of the frame-by-frame route: 0.26 x. */
int mot_sequence_accumulate_dev(mot_ctx* ctx, const float* d_xyzw, long frame_stride, const int* n_points, int frames,
                                const double* timestamps, const double* ego_v, const double* ego_yaw,
                                void* d_tracks, int max_per_frame, int32_t* d_counts);

/* ---------------------------------------------------------------- object-centred track models (additions within ABI v6)
 * What the accumulators exist for, computed where they live: every track's accumulated points RE-CENTRED ON THE OBJECT — each point minus the track's position
 * at the step that brought it, optionally turned into the object's axes of that step — dense over frames, packed per stream, with the cloud's extent. The calls
 * only READ the accumulators; nothing is launched or allocated outside them. Valid whenever accumulation is on with obs_per_track > 0 (MOT_E_STATE otherwise),
 * whatever the slots' frame chain holds: after a stage-wise call, after a reset or mot_stream_load (the touched slots' models are then empty), before the first
 * accumulate call (all empty).
 *
 * mot_export_track_models_dev(batch, flags, ...): rows r = 0 .. T-1 (T = max_tracks_total, indexed as mot_accum_row is) of slots 0 .. batch-1, into block b of the
 * caller's DEVICE buffers: d_models[b * T + r], d_points[b * point_stride + ...], d_counts[2 * b] = the slot's non-empty models, d_counts[2 * b + 1] = its records.
 * Asynchronous on the context stream, nothing is read back; two calls on the same accumulators give identical bytes. flags: MOT_MODEL_AXES | MOT_MODEL_CURRENT,
 * any other bit MOT_E_ARG. MOT_E_ARG also for batch outside [1, max_batch], point_stride < 0, null d_models / d_counts, d_points null with point_stride > 0
 * (null with point_stride 0: headers and extents only), d_points not 16-byte or the others not 4-byte aligned.
 *   WHICH ROWS GIVE NO MODEL ({-1, 0, ...}): a row with track_id < 0 or without a logged observation; with MOT_MODEL_CURRENT every row whose last_step is not the
 *     slot's latest accumulated step (the tracks the latest accumulate call did not append to; the step travels in one stream-ordered copy ahead of the kernels).
 *     A dead track's row that is still readable gives a model unless MOT_MODEL_CURRENT is set.
 *   KEPT RECORDS: the ring's kept points in chronological order whose step is at least the OLDEST LOGGED observation's step — a contiguous suffix of the unrolled
 *     ring (step stamps never decrease along it, the log holds one observation per contributing step). Older points, whose pose has left the log, are left out:
 *     choose obs_per_track for the history the models should span.
 *   RECORD {x', y', z, step}: z and step are the ring's bits; o = the logged observation whose step is the point's; dx = x - o.px, dy = y - o.py (one fp32
 *     subtraction each). Without MOT_MODEL_AXES x' = dx, y' = dy. With it c = (float)cos(o.yaw), s = (float)sin(o.yaw) (evaluated in double, once per
 *     observation), x' = c*dx + s*dy, y' = c*dy - s*dx in fp32, left to right, no contraction: the rotation by -yaw.
 *   PACKING: the models of a slot lie back to back in ascending r: `first` of a model = first + count of the previous non-empty one, 0 for the first. A slot with
 *     more records than point_stride gets the first point_stride of them and nothing beyond is written; first, count and d_counts carry the TRUE numbers.
 *   EXTENT: min / max over the model's records whose three coordinates are all finite (all 0 when none is), over all `count` records also when the block
 *     truncates them. A record with a non-finite coordinate (a diverged track's pose can be NaN) is still written.
 * mot_get_track_models(slot, flags, ...): the same for ONE slot, to the host (synchronises). *n_models = T and *n_points are always delivered; a null buffer is
 * not filled and not tested; MOT_E_CAPACITY with nothing copied when a buffer that was given is too small; MOT_E_ARG for a slot or capacity out of range,
 * unknown flag bits or a null count.
 * Memory: the latest-step block of the export (4 bytes per slot, device and page-locked) and the getter's staging block (48 T bytes, and the slot's records,
 * grown on demand) are allocated at the first call and released when accumulation is turned off or its geometry changes, and by mot_destroy; MOT_E_HIP when
 * that fails, with everything else as it was.
 * Kernels (csrc/track_models.hip): a plan kernel (one workgroup per stream) and a transform kernel (one workgroup per model): 16 bytes read and 16 written per
 * record. Cost (profiles/track_models.md, tools/time_track_models.py): 512 streams x 64 track slots, K = 4096, O = 16, 28 M records in 12 k models: 261 us per call,
 * 265 with MOT_MODEL_AXES = 1.5 x a device-to-device copy of the same records. */
enum { MOT_MODEL_AXES = 1, MOT_MODEL_CURRENT = 2 };
typedef struct mot_track_model {    /* 48 bytes; one per TRACK SLOT of a stream, indexed as mot_accum_row is */
  int32_t track_id;                 /* the row's id; -1: empty row, every other field 0 */
  int32_t first, count;             /* the model's records in the slot's point block (TRUE numbers) */
  int32_t n_obs;                    /* logged observations the model draws on = min(row.obs_total, obs_per_track) */
  int32_t first_step, last_step;    /* step of the oldest logged observation; row.last_step */
  float   min_x, min_y, min_z, max_x, max_y, max_z;   /* extent of the records in the model's frame; all 0 when no finite record */
} mot_track_model;
int mot_export_track_models_dev(mot_ctx* ctx, int batch, int flags,
        mot_accum_point* d_points, long point_stride,      /* records per slot */
        mot_track_model* d_models,                          /* [batch][max_tracks_total] */
        int32_t* d_counts /* [batch][2]: non-empty models, records — the TRUE numbers */);
int mot_get_track_models(mot_ctx* ctx, int slot, int flags, mot_track_model* models, int max_models, int* n_models,
        mot_accum_point* points, int point_capacity, int* n_points);

/* ---------------------------------------------------------------- voxel-thinned object models (additions within ABI v6)
 * The same models, ONE RECORD PER OCCUPIED VOXEL: a LiDAR scans the same surface at every step, so a raw model is the same few hundred surface points many times
 * over; here every model is reduced, where it lives, to the centroids and point counts of the cells of a lattice anchored at the track's position (a voxel is the
 * same piece of the object from call to call). Nothing is launched, written or allocated unless these calls are made; every other entry point gives the bytes it
 * gives without them.
 *
 * mot_export_track_model_voxels_dev(batch, flags, params, ...): rows r = 0 .. T-1 of slots 0 .. batch-1 into block b of the caller's DEVICE buffers:
 * d_models[b * T + r], d_voxels[b * voxel_stride + ...], d_counts[2 * b] = the slot's models, d_counts[2 * b + 1] = its voxels. Asynchronous on the context stream,
 * nothing is read back; two calls on the same accumulators give identical bytes (no floating-point atomics, nothing depends on scheduling).
 *   ROWS, RECORDS: the rows that give a model, the records {x', y', z} that belong to it and their coordinates are those of mot_export_track_models_dev under the
 *     same flags (MOT_MODEL_AXES, MOT_MODEL_CURRENT), bit for bit: one device function computes the record for both calls.
 *   CELL of a record, per axis a = x, y, z: inv_a = 1.0f / leaf_a (fp32, once, on the host); t_a = coord_a * inv_a (one fp32 multiplication). The record TAKES PART
 *     iff its three coordinates are finite and -1024 <= t_x, t_y < 1024 and -512 <= t_z < 512, compared as floats; then i_a = (int)floorf(t_a). Every other record
 *     is counted in n_outside.
 *   VOXELS of a model: the distinct cells in ascending (i_z, i_y, i_x); count = the cell's records; a voxel with count < min_points is dropped and counted in
 *     n_sparse.
 *   CENTROID: x, y, z = the mean of the cell's records, accumulated in fp64 and rounded once to fp32, (float)(sum / count); the order of the additions is fixed by
 *     the model's records alone. It lies within [min, max] of the cell's records on every axis, so floorf(c * inv) is the voxel's own cell.
 *   PACKING: the models of a slot lie back to back in ascending r: `first` of a model = first + count of the previous model, 0 for the first. A slot with more
 *     voxels than voxel_stride gets the first voxel_stride of them and nothing beyond is written; the headers and d_counts carry the TRUE numbers. d_voxels null
 *     with voxel_stride 0: headers only.
 *   HEADER: n_obs, first_step, last_step and the extent are mot_track_model's (the extent is that of the RAW records); n_records = mot_track_model.count;
 *     sum of the voxels' counts + the records of the dropped voxels = n_records - n_outside.
 * MOT_E_ARG: a leaf that is not finite or outside [1e-3, 1e3], min_points outside [1, MOT_MODEL_VOXEL_MAX_K], null params, unknown flag bits, batch outside
 * [1, max_batch], voxel_stride < 0, null d_models / d_counts, d_voxels null with voxel_stride > 0, d_voxels not 16-byte or the others not 4-byte aligned.
 * MOT_E_STATE: accumulation off or obs_per_track == 0; points_per_track > MOT_MODEL_VOXEL_MAX_K (the message names the limit: a model is sorted in the LDS of one
 * workgroup; longer rings would need a sort in global memory). Every refusal comes before anything is launched.
 * mot_get_track_model_voxels(slot, flags, params, ...): the same for ONE slot, to the host (synchronises). *n_models = T and *n_voxels are always delivered; a null
 * buffer is not filled and not tested; MOT_E_CAPACITY with nothing copied when a buffer that was given is too small; MOT_E_ARG for a slot or capacity out of
 * range or a null count.
 * Memory: no voxel is staged — the models are sorted twice, once to count and once to write — so the library's scratch is 96 bytes per row (96 * max_batch *
 * max_tracks_total + 8 * max_batch bytes: the plan's headers and the per-model counts), beside the latest-step block of the raw export; the getter adds a staging
 * block of 64 T bytes and one for the slot's voxels, grown on demand. Allocated at the first call, released when accumulation is turned off or its geometry
 * changes, and by mot_destroy; MOT_E_HIP when that fails, with everything else as it was (the next call resumes).
 * Kernels (csrc/track_voxels.hip): the raw export's plan kernel, a count kernel and a write kernel (one workgroup per model, a bitonic sort of the model's cells in
 * LDS) and a pack kernel (one workgroup per stream). Cost: profiles/track_voxels.md (tools/time_track_voxels.py). */
#define MOT_MODEL_VOXEL_MAX_K 4096          /* largest points_per_track the voxel calls serve */
typedef struct mot_voxel_params { float leaf_x, leaf_y, leaf_z; int32_t min_points; } mot_voxel_params;   /* 16 bytes */
typedef struct mot_model_voxel  { float x, y, z; int32_t count; } mot_model_voxel;                        /* 16 bytes */
typedef struct mot_track_voxel_model {      /* 64 bytes; one per TRACK SLOT, indexed as mot_accum_row / mot_track_model are */
  int32_t track_id;                          /* -1: no model, every other field 0 */
  int32_t first, count;                      /* the model's VOXELS in the slot's block (TRUE numbers) */
  int32_t n_obs, first_step, last_step;      /* as mot_track_model */
  float   min_x, min_y, min_z, max_x, max_y, max_z;   /* as mot_track_model: extent of the RAW records */
  int32_t n_records;                         /* raw records of the model = mot_track_model.count */
  int32_t n_outside;                         /* records that took no part: a non-finite coordinate or a cell outside the lattice */
  int32_t n_sparse;                          /* occupied voxels dropped for holding fewer than min_points records */
  int32_t reserved;                          /* 0 */
} mot_track_voxel_model;
int mot_export_track_model_voxels_dev(mot_ctx* ctx, int batch, int flags, const mot_voxel_params* params,
        mot_model_voxel* d_voxels, long voxel_stride,      /* voxels per slot */
        mot_track_voxel_model* d_models,                    /* [batch][max_tracks_total] */
        int32_t* d_counts /* [batch][2]: models, voxels — the TRUE numbers */);
int mot_get_track_model_voxels(mot_ctx* ctx, int slot, int flags, const mot_voxel_params* params,
        mot_track_voxel_model* models, int max_models, int* n_models, mot_model_voxel* voxels, int voxel_capacity, int* n_voxels);

/* ---------------------------------------------------------------- rolling static-scene grid (additions within ABI v6)
 * The third use of mot_set_track_links, on the device: a MAP WITHOUT THE MOVING OBJECTS. Per stream a rolling W x W occupancy grid in the tracker's global frame,
 * centred on the vehicle, updated by one asynchronous call after a fused step; every elevated point of the step is counted in its cell as STATIC or DYNAMIC. The
 * scene-side twin of the per-track accumulators; independent of them (either, both, in either order after one step). Integer atomics only: the grid is
 * byte-identical from run to run. Off by default; nothing is launched, written or allocated unless the feature is turned on and called. The reference has no such
 * output (its createCostMap is a 50 x 50 per-frame cost map without memory and without tracks). Every rule below is fp32 exactly as written.
 *
 * mot_set_scene_grid(p): cell finite and in [0.05, 10] metres, size = W a power of two in [64, 2048], else MOT_E_ARG; inv = 1.0f / cell. p = NULL turns the feature
 * off and frees its memory (draining the context stream). Needs mot_set_track_links on (MOT_E_STATE otherwise), and while the grid is on mot_set_track_links(0)
 * answers MOT_E_STATE. Allocates max_batch x W^2 x 16 bytes, 48 bytes of headers and 52 of arguments per slot and a ring of page-locked argument blocks; MOT_E_HIP
 * when that fails, and the mode (an earlier geometry included) stays as it was. The same geometry again changes nothing; another geometry frees the memory and
 * starts from empty grids. The grid is NOT stream state: mot_stream_save / mot_stream_load do not carry it. mot_reset, mot_reset_slot, mot_reset_tracks_slot and
 * mot_stream_load empty the grids of the slots they touch and restart those slots' step counters, stream-ordered and without a host synchronisation; the step those
 * slots hold can then no longer be taken. mot_get_scene_grid's staging block (W^2 x 16 bytes, at its first call) goes with the rest.
 *
 * mot_accumulate_scene(batch): takes every elevated point of the latest fused step of slots 0..batch-1. Asynchronous on the context stream, nothing is read back.
 * Validity is that of mot_accumulate_track_points, tested for every slot before anything is launched; a refused call changes nothing and counts no step:
 * MOT_E_STATE unless the slot's cloud, boxes and tracker step come from ONE fused call with links on (a stage-wise call since, a tracker step fed from outside),
 * on the slots of mot_sequence_dev / mot_sequence_accumulate_dev / mot_sequence_products_dev (the last takes a sequence's frames inside the call, below), for a second call on the same step, and after a reset or a load since that step.
 * STEP STAMP of a slot = the number of accepted mot_accumulate_scene calls that covered the slot before this one (0, 1, ...; a counter of its own, apart from the
 * accumulators'; counted on the host, it travels with the slots' matrices in one stream-ordered copy).
 * POINTS: the slot's elevated cloud in input order (MOT_ORDER_ANY included), each under the matrix mot_export_track_points_dev(MOT_FRAME_GLOBAL) applies —
 * global_from_sensor of mot_sensor_pose read right after the fused call; fp32, left to right, no contraction: g = ((m0 x + m1 y) + m2 z) + m3 per row.
 * WINDOW: (tx, ty) = entries 3 and 7 of that matrix; ci = floorf(tx * inv), cj = floorf(ty * inv); origin = (ci - W/2, cj - W/2); the window is [origin, origin + W)
 * on both axes. When tx * inv or ty * inv is not finite or is >= 2^30 in magnitude the step keeps the slot's old origin and clears nothing, every point of the
 * step counts in n_outside, and the step is still stamped. After the setter, a reset or a load the origin is (0, 0) until the first step with a valid window.
 * SCROLL: before the adds of a step every cell whose global index lay outside the previous window is empty (16 zero bytes); cells in the intersection of the old
 * and the new window keep their contents. The first step after the setter, a reset or a load starts from an empty grid. Storage is toroidal — global cell
 * (gi, gj) lives at (gi & (W - 1), gj & (W - 1)) — so a scroll clears only the columns and rows that entered, or everything when the shift is >= W on an axis.
 * CELL OF A POINT: t = g * inv per axis, one fp32 product. The point takes part when its global x, y and z are finite, both |t| < 2^30 and (floorf(tx), floorf(ty))
 * lies in the window; every other point counts in n_outside.
 * KIND: a point is DYNAMIC when its owner id (mot_get_point_tracks) is >= 0 and that track's mot_track.is_static, as this step left it, is 0; every other point
 * is STATIC: points without owner and points of static-flagged tracks. A track is flagged static only once it is confirmed and older than 8 steps, so TENTATIVE
 * AND YOUNG TRACKS COUNT AS DYNAMIC — a parked car shows up as dynamic hits for its first steps and as static hits from then on.
 * PER CELL: static_hits / dynamic_hits count the points (uint32, wrapping); max_z = the largest global z over the cell's static hits since the cell was last
 * emptied, 0.0f while static_hits == 0; last_seen = 1 + the stamp of the latest step that hit the cell (0: never).
 * HEADER: the window's origin; step = the latest stamp, -1 when there was none; n_static, n_dynamic, n_outside of the latest step; size and cell.
 *
 * READERS (MOT_E_STATE while the feature is off; valid whenever it is on, whatever the slots hold: before the first step every grid is empty with step = -1).
 * mot_export_scene_grid_dev writes slot b's grid UNROLLED: the cell at window offset (u, v) — global cell (origin_i + u, origin_j + v) — goes to
 * d_cells[b * cell_stride + v * W + u], the header to d_headers[b]; asynchronous on the context stream, nothing is read back. MOT_E_ARG for cell_stride < W^2, null
 * pointers, a d_cells that is not 16-byte aligned (d_headers: 4-byte), or a batch outside [1, max_batch]. mot_get_scene_grid does the same for ONE slot, to
 * the host (synchronises): *n_cells = W^2 is always delivered; MOT_E_CAPACITY with nothing copied when cells is given and capacity is smaller; a null cells gives
 * the header alone. A refused call writes nothing into the caller's blocks.
 *
 * Kernels (csrc/scene_grid.hip): a scroll kernel (clears what entered, writes the header), the splat kernel (16 bytes read per point and two small gathers per
 * owned point; one lane per run of neighbouring points of one cell and kind issues the atomics) and the export kernel (32 bytes per cell). Cost:
 * profiles/scene_grid.md (tools/time_scene_grid.py measures both calls against device-to-device copies of the bytes they read). */
typedef struct mot_scene_params { float cell; int32_t size; } mot_scene_params;   /* metres per cell; W cells per side */
typedef struct mot_scene_cell {     /* 16 bytes */
  uint32_t static_hits, dynamic_hits;
  float    max_z;                   /* global frame; 0.0f while static_hits == 0 */
  int32_t  last_seen;               /* 1 + step stamp of the latest hit; 0: never */
} mot_scene_cell;
typedef struct mot_scene_header {   /* 32 bytes */
  int32_t  origin_i, origin_j;      /* global cell index of window offset (0, 0) */
  int32_t  step;                    /* latest step stamp; -1: none yet */
  int32_t  size;                    /* W */
  uint32_t n_static, n_dynamic, n_outside;   /* of the latest step */
  float    cell;
} mot_scene_header;
int mot_set_scene_grid(mot_ctx* ctx, const mot_scene_params* p /* NULL: off, memory freed */);
int mot_accumulate_scene(mot_ctx* ctx, int batch);
int mot_export_scene_grid_dev(mot_ctx* ctx, int batch, mot_scene_cell* d_cells, long cell_stride /* cells per slot */, mot_scene_header* d_headers);
int mot_get_scene_grid(mot_ctx* ctx, int slot, mot_scene_cell* cells, int capacity, int* n_cells, mot_scene_header* header);

/* ---------------------------------------------------------------- a frame's points judged against the scene grid (additions within ABI v6)
 * The grid asked a question, on the device: which of the points of the latest fused step belong to the standing scene, which to something that has just appeared,
 * which lie where a mover passed. One verdict per elevated point, the points partitioned by verdict into the caller's block. The call READS the grid: it changes
 * not a byte of it and consumes no step. Nothing is launched, written or allocated unless these calls are used. All integer work is exact.
 *
 * CLASS of an elevated point of the slot's latest fused step, the rules in this order:
 *   1 MOVING   the grid's KIND rule says DYNAMIC: owner id >= 0 and that track's is_static, as this step left it, is 0 (an id or a track slot out of range counts as
 *              dynamic, as in the splat kernel). No cell is needed: inside and outside the window alike.
 *   2 UNKNOWN  the point does not take part by the grid's rule CELL OF A POINT, tested against the window in the slot's grid header AS IT STANDS: a global x, y or z
 *              that is not finite, |t| >= 2^30, a cell outside [origin, origin + W)^2, a grid whose latest accepted step had a window that could not be placed, a
 *              grid with no step yet. The matrix is the one mot_accumulate_scene would use for this step and the arithmetic is the grid's own: the cell is bit for
 *              bit the one the point would be counted in.
 *   3 otherwise, with s = static_hits and d = dynamic_hits of that cell as stored:
 *     TRAIL    d > 0 and (uint64)d * trail_den > ((uint64)s + d) * trail_num: dynamic_hits / (static_hits + dynamic_hits) > num / den. Equality is not a trail;
 *              num == den turns the class off; num == 0 makes every cell with a dynamic hit a trail.
 *     NEW      not TRAIL and s < min_static_hits. An empty cell is NEW.
 *     KNOWN    every other point.
 * BEFORE OR AFTER mot_accumulate_scene of the same step, both are legal. Before: the point is judged against history alone — the intended use; cells the vehicle's
 * motion is about to bring into the window are UNKNOWN. After: the cell already holds the frame's own hits.
 * VALIDITY is that of mot_accumulate_scene without its once-per-step clause, tested for every slot before anything is launched: MOT_E_STATE while the grid is off,
 * unless the slot's cloud, boxes and tracker step come from ONE fused call with links on, on sequence slots, and after the setter, a reset or a load since that step.
 *
 * mot_export_scene_points_dev, slots 0..batch-1, asynchronous on the context stream, nothing is read back:
 *   d_segments[b * 5 + k] = {first, count}: count is the TRUE number of class-k points of slot b, for every class whether or not it is in class_mask (bits 0..4);
 *   the classes in the mask are packed back to back into d_points[b * point_stride ..] in ascending class order, first = the segment's start; a class that is not in
 *   the mask gets first = -1. Inside a segment the 16-byte records {x, y, z, index} keep the elevated cloud's INPUT order, index strictly ascending (MOT_ORDER_ANY
 *   included). frame: MOT_FRAME_SENSOR (the point's bits) or MOT_FRAME_GLOBAL (the bits mot_export_track_points_dev writes). A slot with more selected records than
 *   point_stride gets the first point_stride of them and nothing beyond. d_points == NULL with point_stride == 0 and mask 0 gives the counts alone.
 *   d_classes (may be NULL): d_classes[b * class_stride + i] = the class of elevated point i in input order, truncated at class_stride.
 * REFUSALS, each before anything runs, the caller's blocks untouched: MOT_E_STATE as above; MOT_E_ARG for null params or segments, min_static_hits of 0 or > 2^31,
 * trail_den of 0 or > 65535, trail_num > trail_den, mask bits >= 5, an unknown frame, a batch outside [1, max_batch], a negative stride, null d_points with
 * point_stride > 0 or a non-zero mask, d_points or d_segments not 4-byte aligned; MOT_E_HIP when the scratch cannot be had at the first call — all of its blocks or
 * none, the next call tries again.
 * mot_get_scene_points does the same for ONE slot, to the host (synchronises): *n_points (the selected records), *n_elevated and the five segments are always
 * delivered; MOT_E_CAPACITY with nothing copied when a buffer that was given (points, classes) is too small; either may be NULL.
 *
 * Scratch, at the first call: 1 byte per point of max_points and 40 bytes per 2048 points per slot, and an argument block as the grid's (52 bytes per slot, sent
 * through the grid's page-locked ring in one stream-ordered copy); the getter's staging block at ITS first call. Released with the grid (mot_set_scene_grid(NULL) or
 * another geometry) and by mot_destroy.
 * Kernels (csrc/scene_judge.hip): classify (per point 16 bytes read, two small gathers for an owned point, ONE 8-byte gather of the cell's two counters; the class
 * byte and the chunk's five counts out), a scan (one workgroup per slot) and the scatter (class byte and point in, one 16-byte store per selected record). No global
 * atomics, no workgroup waits on another, the output does not depend on scheduling. Cost: profiles/scene_judge.md (tools/time_scene_judge.py). */
enum { MOT_SCENE_UNKNOWN = 0, MOT_SCENE_MOVING = 1, MOT_SCENE_TRAIL = 2, MOT_SCENE_NEW = 3, MOT_SCENE_KNOWN = 4, MOT_SCENE_CLASSES = 5 };
typedef struct mot_scene_judge_params {
  uint32_t min_static_hits;      /* [1, 2^31]: a cell with fewer static hits has not been seen standing */
  uint32_t trail_num, trail_den; /* 0 <= num <= den, den in [1, 65535]: a cell is a mover's trail when dynamic_hits / (static + dynamic) > num / den */
} mot_scene_judge_params;
typedef struct mot_scene_segment { int32_t first, count; } mot_scene_segment;   /* 8 bytes */
int mot_export_scene_points_dev(mot_ctx* ctx, int batch, const mot_scene_judge_params* params, int class_mask, int frame,
        mot_track_point* d_points, long point_stride, mot_scene_segment* d_segments /* [batch][5] */,
        uint8_t* d_classes /* may be NULL */, long class_stride);
int mot_get_scene_points(mot_ctx* ctx, int slot, const mot_scene_judge_params* params, int class_mask, int frame,
        mot_track_point* points, int point_capacity, int* n_points, mot_scene_segment segments[5],
        uint8_t* classes /* may be NULL */, int class_capacity, int* n_elevated);

/* ---------------------------------------------------------------- a recorded drive into a map: sequence mode with products (addition within ABI v6)
 * mot_sequence_products_dev IS mot_sequence_dev — the same arguments, the same launch sequence — plus a bit set of products taken from every frame of the call in
 * the same asynchronous call (nothing is read back, no host synchronisation). products == 0 is mot_sequence_dev; products == MOT_SEQ_ACCUMULATE is
 * mot_sequence_accumulate_dev (above); MOT_SEQ_SCENE takes every frame into STREAM 0's scene grid; both bits: a drive into the accumulators and the grid at once.
 * The two older entry points stay as they are.
 *
 * RESULT of MOT_SEQ_SCENE. Slot 0's grid and header (mot_export_scene_grid_dev / mot_get_scene_grid) are, byte for byte, what `frames` rounds of
 * { mot_frames_dev(batch 1) on frame k; mot_accumulate_scene(ctx, 1) } leave there from the same tracker and grid state: the toroidal cells, last_seen, the header of
 * the LAST frame (origin, stamp, that frame's three counters), the stored previous origin and window validity — frame-by-frame steps and further sequence calls
 * continue the same grid. The grids of slots >= 1 are not touched. Every other result of the call is byte-identical to mot_sequence_dev's (with
 * MOT_SEQ_ACCUMULATE: to mot_sequence_accumulate_dev's).
 * STEP STAMPS: frame k gets (slot 0's scene step counter) + k and the counter advances by `frames`; a frame the box stage refused for capacity is taken as the
 * frame-by-frame route takes it (its elevated points, none of them owned), and it counts.
 * AFTER THE CALL the slots are sequence slots: mot_accumulate_scene keeps answering MOT_E_STATE on them. mot_reset* and mot_stream_load empty slot 0's grid and
 * restart its counter as they always do.
 * REFUSALS, each before anything has run (the tracker has not stepped): MOT_E_ARG for unknown bits and for mot_sequence_dev's argument errors; MOT_E_STATE when
 * MOT_SEQ_SCENE is set and the grid is off, when MOT_SEQ_ACCUMULATE is set and accumulation is off, when either is set with links off; MOT_E_HIP when a product's
 * own scratch cannot be had at its first use — all of its blocks or none, the next call tries again. The scene's scratch is 32 bytes per slot of max_batch (+ 32)
 * for the windows and max_batch x ceil(max_tracks_ever / 32) x 4 bytes (one bit per track id and frame: the tracks a frame's step left flagged static; 16 KB a
 * frame at the default max_tracks_ever of 64 x 2048); it is released with the grid (mot_set_scene_grid(NULL) or another geometry) and by mot_destroy.
 * HOW (csrc/scene_grid_seq.hip). The kind of a point ("is_static as this step left it") is gone one tracker step later: a small kernel behind every step keeps it,
 * one bit per id. The rolling window needs no serial pass: all windows are squares of one size, so "this cell was never scrolled out between frame k and the last
 * frame" is membership in ONE rectangle per frame, R[k] = [max_{j >= k} o[j], min_{j >= k} o[j] + W) per axis over the origins o[j] of the windows k .. frames - 1
 * (an invalid window keeps the origin before it; R[-1] starts at the origin the grid was laid out for before the call). Cells of the final window outside R[-1]
 * are emptied, a point of frame k takes part iff its frame's window is valid and its cell lies in R[k] — with the arithmetic of mot_accumulate_scene bit for bit;
 * last_seen is an integer maximum, only the last frame feeds the header's counters. One windows workgroup (two scans), a clear and ONE splat launch over all
 * frames, whatever `frames` is. Cost: profiles/scene_grid_sequence.md (tools/time_scene_grid_sequence.py). */
enum { MOT_SEQ_ACCUMULATE = 1, MOT_SEQ_SCENE = 2 };
int mot_sequence_products_dev(mot_ctx* ctx, const float* d_xyzw, long frame_stride, const int* n_points, int frames,
                              const double* timestamps, const double* ego_v, const double* ego_yaw,
                              void* d_tracks, int max_per_frame, int32_t* d_counts, int products);

/* ---------------------------------------------------------------- a drive's points judged against its grid: the static map in one call (additions within ABI v6)
 * The sequence-mode twin of mot_export_scene_points_dev. Behind a mot_sequence_products_dev call with MOT_SEQ_SCENE, EVERY frame of that call is judged against
 * slot 0's grid AS THE WHOLE DRIVE LEFT IT — with hindsight, on purpose: sequence mode is offline, and the first frames of a drive are not all NEW. The records come
 * packed across frames, class-major, so all KNOWN points of the drive are ONE contiguous run in the global frame: the static map, movers and their trails cut out.
 * Asynchronous, behind the sequence call on the context stream. The call READS the grid and consumes no step. Nothing is launched, written or allocated unless
 * these calls are used. (The causal variant — every frame against the grid as it stood before that frame — is what interleaved frame-by-frame calls give.)
 *
 * VERDICTS. The five classes, the parameter domain and the class rules are exactly those of mot_export_scene_points_dev, applied to frame k (slot k) with frame k's
 * own matrix. KIND of an owned point: the track's is_static AS STEP k LEFT IT (the bit rows the sequence call captured; id < 0: no owner, static; id >= max_tracks_ever
 * or no bit: dynamic). CELL: tested against slot 0's header and grid as they stand — the final window and its validity (a drive whose last frame could not place its
 * window: nothing takes part, every point is UNKNOWN or MOVING) — with the grid's own arithmetic: bit for bit the cell the point was counted in.
 * LAYOUT, ONE block for the drive: the classes of class_mask in ascending order; inside a class the frames ascending; inside a frame the elevated cloud's input order
 * (index strictly ascending, MOT_ORDER_ANY included). d_totals[c] = {first, count} is the drive's run of class c, d_segments[k * 5 + c] = {first, count} frame k's part
 * of it, `first` an ABSOLUTE position in d_points; a class outside the mask gets first = -1 in both tables; counts are the TRUE counts for all five classes. A record
 * whose position is at or beyond point_capacity is not stored, nothing is written beyond the capacity. frame: MOT_FRAME_SENSOR (the point's bits) or MOT_FRAME_GLOBAL
 * (the bits mot_export_track_points_dev writes, with frame k's matrix). d_classes (may be NULL): d_classes[k * class_stride + i] = the class of point i of frame k,
 * truncated at class_stride. d_points == NULL with point_capacity == 0 and mask 0 gives the counts alone.
 * VALIDITY: served only while slots 0..frames-1 are the sequence slots of the LATEST mot_sequence_products_dev call that had MOT_SEQ_SCENE (MOT_SEQ_ACCUMULATE may have
 * been set with it), frames in [1, frames of that call], links and grid on, and nothing has emptied or changed a grid or taken a slot since: a fused or stage-wise
 * call, a tracker step from outside, mot_reset*, mot_stream_load, mot_set_scene_grid, mot_set_track_links, a later sequence call without MOT_SEQ_SCENE — MOT_E_STATE.
 * mot_export_scene_points_dev keeps refusing sequence slots.
 * REFUSALS, each before anything is launched, the caller's blocks untouched: MOT_E_STATE as above; MOT_E_ARG as for mot_export_scene_points_dev (params, mask,
 * frame, null d_segments, a negative stride, null d_points with a capacity or a mask, a block off 4 bytes), for null d_totals, a negative capacity, frames outside
 * [1, frames of the sequence call] and frames * max_points beyond 2^31 - 1 (positions are int32); MOT_E_HIP when the scratch cannot be had — all of its blocks or
 * none, the next call tries again.
 * mot_get_sequence_scene_points does the same to the host (synchronises): *n_points (the selected records), segments [frames][5] and totals [5] are always delivered;
 * MOT_E_CAPACITY with nothing copied when points is given and point_capacity < *n_points, or classes is given and class_stride is below a frame's elevated count;
 * either may be NULL. Frame k's class bytes go to classes[k * class_stride ..], as many as the frame has points.
 *
 * Scratch: that of mot_export_scene_points_dev (sized for max_batch slots, shared with it) and 20 bytes per slot for the (frame, class) places; the getter adds a
 * table block at its first call and takes a block of the records' size for the duration of a call. Released with the grid and by mot_destroy.
 * Kernels (csrc/scene_judge_seq.hip): classify over (chunks, frames) — per point one 4-byte gather of the kind bit row and one 8-byte gather of the cell's two
 * counters —, a scan per frame, ONE workgroup that scans the frames per class, and the scatter; four launches whatever `frames` is. No global atomics, no workgroup
 * waits on another, the output does not depend on scheduling. Cost: profiles/scene_judge_sequence.md (tools/time_scene_judge_sequence.py). */
int mot_export_sequence_scene_points_dev(mot_ctx* ctx, int frames, const mot_scene_judge_params* params, int class_mask, int frame,
        mot_track_point* d_points, long point_capacity /* ONE block for the drive */,
        mot_scene_segment* d_segments /* [frames][5] */, mot_scene_segment* d_totals /* [5] */,
        uint8_t* d_classes /* may be NULL */, long class_stride);
int mot_get_sequence_scene_points(mot_ctx* ctx, int frames, const mot_scene_judge_params* params, int class_mask, int frame,
        mot_track_point* points /* may be NULL */, long point_capacity, long* n_points,
        mot_scene_segment* segments /* [frames][5] */, mot_scene_segment totals[5],
        uint8_t* classes /* may be NULL */, long class_stride);

/* ---------------------------------------------------------------- voxel-thinned static map of a recorded drive (additions within ABI v6)
 * The run mot_export_sequence_scene_points_dev gives holds a standing wall once per frame that saw it. These calls reduce the same records, on the device, to ONE
 * RECORD PER OCCUPIED VOXEL: the centroid of the cell's records and their number. Asynchronous, behind the sequence call on the context stream; the call READS the
 * grid and consumes no step. Nothing is launched, written or allocated unless these calls are used. Every rule below is fp32 exactly as written, no contraction.
 *
 * RECORDS. R[0..m) are the records mot_export_sequence_scene_points_dev(frames, params, class_mask, MOT_FRAME_GLOBAL, ...) would write with unlimited capacity, in
 * that call's order (class ascending, then frame ascending, then input order): its verdicts, its global coordinates and its order, bit for bit (the same device
 * functions). Records at positions >= record_capacity take no part and are counted in n_beyond.
 * CELL OF A RECORD. inv_a = 1.0f / leaf_a, computed once on the host; t_a = coord_a * inv_a. The record takes part iff all three coordinates are finite and
 * -2^20 <= t_x, t_y < 2^20 and -2^11 <= t_z < 2^11, compared as floats; then i_a = (int)floorf(t_a). Every other record below the capacity counts in n_outside. The
 * lattice is anchored at the global origin: a voxel is the same piece of the world from call to call and from drive to drive.
 * VOXELS. The distinct cells in ascending (i_z, i_y, i_x); count = the cell's records. A voxel with count < min_points is dropped and counted in n_sparse; the kept
 * voxels are packed back to back, the first voxel_capacity of them are stored and nothing is written beyond.
 * CENTROID. A voxel's records in record order r_0 .. r_{n-1}; per axis 64 fp64 accumulators acc[l] = ((r_l + r_{l+64}) + r_{l+128}) + ..., each starting from its
 * first record; S = ((acc[0] + acc[1]) + acc[2]) + ... + acc[min(n, 64) - 1], added in ascending l; the centroid is (float)(S / (double)n). For n <= 64 this is the
 * plain left-to-right sum. (The order is fixed so that a wave can sum a long run and the bytes do not depend on how the work was cut.)
 * HEADER. n_records = n_beyond + n_outside + sum of count over the kept voxels + sum of count over the sparse ones. d_totals (may be NULL): the five {first, count}
 * of the judge call for this mask (first = -1 outside the mask).
 * VALIDITY: exactly that of mot_export_sequence_scene_points_dev — only behind the latest MOT_SEQ_SCENE sequence call, frames within that call's, links and grid on,
 * nothing having taken a slot or changed a grid since.
 * REFUSALS, each before anything is launched, the caller's blocks untouched: MOT_E_STATE as above; MOT_E_ARG for the judge call's argument errors, null voxel or
 * d_header, a leaf that is not finite or outside [1e-2, 1e3], min_points outside [1, 2^30], record_capacity outside [0, 2^31 - 1], a negative voxel_capacity, null
 * d_voxels with voxel_capacity > 0, d_voxels not 16-byte aligned or another block not 4-byte aligned; MOT_E_HIP when the scratch cannot be had — all of its blocks
 * or none, the next call tries again.
 * mot_get_sequence_scene_voxels does the same to the host (synchronises): the header, *n_voxels (the true count) and the totals are always delivered;
 * MOT_E_CAPACITY with nothing copied when voxels is given and voxel_capacity < *n_voxels. The getter's n_stored is what it copied to the caller: n_voxels, or 0
 * when voxels is NULL or the call answers MOT_E_CAPACITY.
 *
 * Scratch: that of mot_export_sequence_scene_points_dev and ONE block grown on demand to record_capacity — 40 bytes per record of capacity (two 8-byte keys and two
 * 4-byte payloads, which ping-pong in the sort, and the 16-byte record staged at its place) and 1036 bytes per 2048 records for the sort's tables. The launches are
 * sized by record_capacity as well; the kernels read the true m on the device and leave early. Released with the grid (mot_set_scene_grid(NULL) or another
 * geometry) and by mot_destroy. The host getter adds, as mot_get_sequence_scene_points does, a 96-byte table block at ITS first call (released with the rest) and
 * takes a device block of n_voxels x 16 bytes for the duration of a call that copies voxels (allocated and freed inside the call).
 * Kernels (csrc/scene_voxels_seq.hip, csrc/mot_sort.h): the judge's three count launches; a key kernel on the scatter kernel's geometry; a device-wide stable LSD
 * radix sort of the 64-bit keys, key = (i_z + 2^11) << 42 | (i_y + 2^20) << 21 | (i_x + 2^20), all ones outside the lattice (7 passes of 8 bits, three launches a
 * pass); run heads, a scan, the run table; kept runs, a scan, the header; one wave per run writes the voxels. 32 launches whatever `frames` and the data are. No
 * global atomics, no workgroup waits on another, the output does not depend on scheduling. Cost: profiles/scene_voxels_sequence.md
 * (tools/time_scene_voxels_sequence.py). */
typedef struct mot_scene_voxel_header {   /* 32 bytes */
  int32_t n_records;   /* selected records of the drive: the sum of the mask's class totals (TRUE) */
  int32_t n_beyond;    /* records at positions >= record_capacity: took no part */
  int32_t n_outside;   /* records below the capacity with a non-finite coordinate or a cell outside the lattice */
  int32_t n_voxels;    /* kept voxels (TRUE, whatever voxel_capacity is) */
  int32_t n_sparse;    /* occupied voxels dropped for fewer than min_points records */
  int32_t n_stored;    /* min(n_voxels, voxel_capacity) */
  int32_t reserved[2]; /* 0 */
} mot_scene_voxel_header;
int mot_export_sequence_scene_voxels_dev(mot_ctx* ctx, int frames, const mot_scene_judge_params* params, int class_mask,
        const mot_voxel_params* voxel, long record_capacity,
        mot_model_voxel* d_voxels, long voxel_capacity,
        mot_scene_voxel_header* d_header, mot_scene_segment* d_totals /* [5], may be NULL */);
int mot_get_sequence_scene_voxels(mot_ctx* ctx, int frames, const mot_scene_judge_params* params, int class_mask,
        const mot_voxel_params* voxel, long record_capacity,
        mot_model_voxel* voxels /* may be NULL */, long voxel_capacity, long* n_voxels,
        mot_scene_voxel_header* header, mot_scene_segment totals[5] /* may be NULL */);

/* ---------------------------------------------------------------- voxel maps merged into one (additions within ABI v6)
 * The voxel lattice is anchored at the global origin: the maps of a drive's pieces, of a drive longer than the scene grid's window, or of two passes over one
 * street speak of the same cells. These calls merge up to 16 such maps — blocks of mot_model_voxel, as every voxel export of the library writes them — into ONE map
 * of the same record format and the same order, counts added and centroids weighted by count, on the device. Asynchronous on the context stream; the host never
 * reads the data; deterministic byte for byte. Nothing is launched or allocated unless these calls are used. Every rule below is fp32 or fp64 exactly as written,
 * no contraction.
 *
 * INPUTS. I[0..n) is the concatenation of the maps in argument order; map k contributes its first min(max(*count_k, 0), capacity_k) voxels, in position order.
 * count_k is an int32 ON THE DEVICE, read there (NULL: capacity_k is the count): it may point at &d_header->n_stored of an earlier
 * mot_export_sequence_scene_voxels_dev or of an earlier merge, so that an export -> merge -> export -> merge chain needs no synchronisation. Voxels beyond the
 * clamped count are never read.
 * CELL OF AN INPUT. The CELL OF A RECORD rule of the drive voxel call (above), applied to the input's centroid with THIS call's leaf — the same device function.
 * An input with count <= 0, a non-finite centroid or a cell outside the lattice takes no part and counts in n_outside.
 * LEAF. It need not be the one the inputs were made with: merging at a coarser leaf is re-thinning. The merge is defined by the centroids' cells, whatever they are.
 * VOXELS. The distinct cells in ascending (i_z, i_y, i_x). A cell's inputs are taken in concatenation order (map ascending, then position). W = the int64 sum of
 * the cell's counts; a cell with W < min_points is dropped and counted in n_sparse; a kept voxel's count is min(W, 2^31 - 1), and it counts in n_saturated when W
 * is larger. The kept voxels are packed back to back, the first out_capacity of them are stored and nothing is written beyond.
 * CENTROID. The order of the drive voxel call's CENTROID rule: a cell's inputs r_0 .. r_{m-1}, per axis 64 fp64 accumulators acc[l] = ((t_l + t_{l+64}) + ...), each
 * starting from its own first term, S = ((acc[0] + acc[1]) + ...) + acc[min(m, 64) - 1] in ascending l; the term of input r is t_r = (double)c_r * (double)count_r,
 * one fp64 multiply; the centroid is (float)(S / (double)W), W the TRUE sum. For m <= 64 this is the plain left-to-right sum.
 * HEADER. n_inputs = n_outside + sum of the inputs of the kept cells + those of the sparse cells.
 * STATE. The calls read nothing but their arguments: they work with the grid and the links on or off and on any slot state, touch no slot, no step counter and no
 * grid, and leave the validity of the sequence exports alone.
 * REFUSALS, each before anything is launched, the caller's blocks untouched: MOT_E_ARG for a null context, maps, voxel or header; n_maps outside [1, 16]; a leaf or
 * min_points outside the domain of the drive voxel call; a negative capacity; a sum of capacities above 2^31 - 1; null voxels with capacity > 0; null d_out with
 * out_capacity > 0; d_out or an input not 16-byte aligned; a count or header pointer off 4 bytes; d_out or d_header overlapping any input block or count word
 * (inputs may overlap each other). MOT_E_HIP when the scratch cannot be had — all of its blocks or none, the next call tries again.
 * mot_merge_voxel_maps takes host blocks (and host counts, clamped on the host), synchronises and stages inputs and output through device blocks that live for the
 * duration of the call: *n_voxels and the header are always delivered; MOT_E_CAPACITY with nothing copied when out is given and out_capacity < *n_voxels; its
 * n_stored is what it copied (n_voxels, or 0). Host blocks need 4-byte alignment only, and may overlap.
 *
 * Scratch: ONE block of the merge's own on the context, grown on demand to the sum of the capacities — 24 bytes per input of capacity (two 8-byte keys and two
 * 4-byte payloads, which ping-pong in the sort; the buffers the sort leaves free hold the run table) and 1040 bytes per 2048 inputs for the sort's tables and the
 * per-tile counts. The inputs are read in place, not staged. Released by mot_destroy.
 * Kernels (csrc/voxel_merge.hip, csrc/mot_sort.h, csrc/mot_voxel_runs.h): a key kernel over the concatenation (every workgroup repeats the prefix over the <= 16
 * counts); the radix sort of the drive voxel call over the same 56 key bits; run heads, a scan, the run table; the runs' summed counts; kept runs, a scan, the
 * header; the voxels — a run of at most 64 inputs by one thread, a longer one by a wave. 30 launches whatever the data and n_maps are (29 without an output block).
 * No global atomics, no workgroup waits on another, the output does not depend on scheduling. Cost: profiles/voxel_merge.md (tools/time_voxel_merge.py). */
enum { MOT_VOXEL_MERGE_MAX_MAPS = 16 };
typedef struct mot_voxel_map_src {      /* 24 bytes */
  const mot_model_voxel* voxels;        /* _dev call: device block, 16-byte aligned; host call: host block */
  const int32_t* count;                 /* _dev call: an int32 ON THE DEVICE, read there and clamped to [0, capacity]; NULL: capacity is the count.
                                           Host call: a host int32 or NULL */
  long capacity;                        /* [0, 2^31 - 1]; voxels may be NULL when 0 */
} mot_voxel_map_src;
typedef struct mot_voxel_merge_header { /* 32 bytes */
  int32_t n_inputs;     /* sum of the clamped counts */
  int32_t n_outside;    /* inputs that took no part: count <= 0, a non-finite centroid, or a cell outside the lattice */
  int32_t n_voxels;     /* kept voxels (TRUE, whatever out_capacity is) */
  int32_t n_sparse;     /* occupied cells dropped: summed count < min_points */
  int32_t n_stored;     /* min(n_voxels, out_capacity) */
  int32_t n_saturated;  /* kept voxels whose summed count exceeds 2^31 - 1 (stored as 2^31 - 1) */
  int32_t reserved[2];  /* 0 */
} mot_voxel_merge_header;
int mot_merge_voxel_maps_dev(mot_ctx* ctx, const mot_voxel_map_src* maps /* HOST array */, int n_maps, const mot_voxel_params* voxel,
        mot_model_voxel* d_out, long out_capacity, mot_voxel_merge_header* d_header);
int mot_merge_voxel_maps(mot_ctx* ctx, const mot_voxel_map_src* maps /* host array, host blocks */, int n_maps, const mot_voxel_params* voxel,
        mot_model_voxel* out /* may be NULL */, long out_capacity, long* n_voxels, mot_voxel_merge_header* header);

/* ---------------------------------------------------------------- voxel maps indexed, and a frame's points judged against the index (additions within ABI v6)
 * The reader of the maps above: given the static map of an earlier pass, which points of the live frame lie where the map has something standing, and which lie
 * where it has nothing — a parked car that was not there yesterday, a barrier. Two calls: a device-resident INDEX of one or several voxel maps, and a JUDGE that
 * gives every elevated point of a fused step one verdict against it, the points partitioned by verdict in the shape of mot_export_scene_points_dev. Asynchronous on
 * the context stream, no host round trip from drive to map to the next drive. Nothing is launched or allocated unless these calls are used.
 *
 * mot_index_voxel_maps_dev. EXACTLY the merge's meaning (above) without the centroid: INPUTS, CELL OF AN INPUT, LEAF and the cells, W and n_saturated of VOXELS are
 * those rules word for word, the counts of the maps read on the device and clamped — a count may point at an earlier export's or merge's n_stored, so export ->
 * merge -> index -> judge never synchronises. The kept cells are the distinct cells in ascending key order whose W >= min_points;
 *   keys[r]   = the cell's key itself: (i_z + 2^11) << 42 | (i_y + 2^20) << 21 | (i_x + 2^20) — the sorted key of its inputs, not re-derived from a centroid;
 *   counts[r] = min(W, 2^31 - 1);
 * the first `capacity` kept cells are stored and nothing is written beyond. *header is a mot_voxel_merge_header with the merge's meaning, field for field (n_stored =
 * min(n_voxels, capacity): the index's length). The call writes leaf_x/y/z of the descriptor from `voxel` (the judge takes its leaf from there) and reserved = 0.
 * REFUSALS, each before anything is launched, the caller's blocks and the descriptor untouched: those of mot_merge_voxel_maps_dev with keys / counts / header read
 * in place of d_out / d_header — MOT_E_ARG for a null index, index->header or voxel; null keys or counts with capacity > 0; a capacity outside [0, 2^31 - 1]; keys
 * off 8 bytes, counts or header off 4; keys, counts or header overlapping any input block or count word, or each other. MOT_E_HIP when the scratch cannot be had.
 * Scratch and kernels: the merge's own block and its count launches as they are (csrc/voxel_merge.hip), then ONE write launch — per kept cell below the capacity
 * the key and the saturated W, a run of at most 64 inputs by one thread, a longer one by a wave. 30 launches whatever the data (29 with a capacity of 0).
 *
 * mot_export_map_points_dev. CLASS of an elevated point of the slot's latest fused step, the rules in this order:
 *   1 MOVING   the grid's KIND rule says DYNAMIC: owner id >= 0 and that track's is_static, as this step left it, is 0 (an id or a track slot out of range counts as
 *              dynamic). No cell is needed.
 *   2 OUTSIDE  the point's global record takes no part by the rule CELL OF A RECORD (above): the coordinates are the bits mot_export_track_points_dev writes with
 *              MOT_FRAME_GLOBAL — the bits a drive's map is made from — and the cell test is the map's own device function with inv_a = 1.0f / index->leaf_a, computed
 *              once on the host. A non-finite global coordinate is OUTSIDE.
 *   3 otherwise, with (i_x, i_y, i_z) the point's cell and n = clamp(header->n_stored, 0, capacity), read ON THE DEVICE: the neighbourhood is the cells
 *     (i_x + d_x, i_y + d_y, i_z + d_z), |d| <= reach, that lie inside the lattice (i_x, i_y in [-2^20, 2^20), i_z in [-2^11, 2^11)); a neighbour outside the
 *     lattice is in no map — the cell before i_x = -2^20 is NOT the last cell of the row below.
 *     PRESENT  some neighbourhood cell is among keys[0..n) with counts >= min_count.
 *     SPARSE   some neighbourhood cell is among keys[0..n), none of them reaches min_count.
 *     ABSENT   none is. n == 0 makes every such point ABSENT.
 * An index whose blocks were not written by mot_index_voxel_maps_dev gives unspecified classes, never an access outside the blocks.
 * OUTPUT: word for word that of mot_export_scene_points_dev with these five classes — d_segments[b * 5 + k] = {first, count} with the TRUE count of every class and
 * first = -1 outside the mask; the selected classes packed in ascending class order into d_points[b * point_stride ..], records {x, y, z, index} in input order
 * (MOT_ORDER_ANY included), MOT_FRAME_SENSOR or MOT_FRAME_GLOBAL, truncated at point_stride; d_points == NULL with stride 0 and mask 0: the counts alone; d_classes
 * optional, truncated at class_stride. mot_get_map_points is mot_get_scene_points' twin: one slot to the host (synchronises), the counts and the table always
 * delivered, MOT_E_CAPACITY with nothing copied when a buffer that was given is too small. Its index blocks are DEVICE blocks all the same.
 * VALIDITY: the slot's cloud, boxes and tracker step come from ONE fused call with links on (MOT_E_STATE otherwise, and on sequence slots). The scene grid is NOT
 * required: the calls work with the grid off, read nothing of it and leave its validity alone. They change no slot, no step counter, no accumulator.
 * REFUSALS, each before anything is launched, the caller's blocks untouched: MOT_E_STATE as above; MOT_E_ARG for a null index or params; a leaf in the descriptor
 * that is not finite or outside [1e-2, 1e3]; min_count < 1; reach outside {0, 1}; mask bits >= 5; an unknown frame; a batch outside [1, max_batch]; a negative
 * stride; null d_points with a stride or a mask; null d_segments; d_points or d_segments off 4 bytes, keys off 8, counts or header off 4; an index capacity outside
 * [0, 2^31 - 1]; a null header; null keys or counts with capacity > 0; an output block overlapping an index block. MOT_E_HIP when the scratch cannot be had.
 * Scratch of the calls' own, at the first call, all of it or none (the next call tries again): 1 byte per point of max_points and 40 bytes per 2048 points per slot,
 * a 48-byte-per-slot argument block and a page-locked ring in front of it; the getter's staging block at ITS first call. Released by mot_destroy alone.
 * Kernels (csrc/map_judge.hip): classify — per point 16 bytes read, the kind rule's two gathers for an owned point, the transform and the cell, then a binary
 * search of the keys (reach 0: one lower bound of at most 32 steps and a compare; reach 1: nine, one per (i_z + d_z, i_y + d_y) row, each followed by at most three
 * consecutive entries: a row's three x-neighbours are adjacent in key order); only the first lane of a run of equal cells inside a wave searches. Then the scene
 * judge's scan and scatter, the same text. Three launches whatever the data; no global atomics, no workgroup waits on another, the output does not depend on
 * scheduling. Cost: profiles/map_judge.md (tools/time_map_judge.py).
 * OUT OF SCOPE: a recorded-drive (sequence-slot) variant; host-block variants of the index call; reach > 1; updating an index in place. */
typedef struct mot_voxel_index {       /* HOST struct of device pointers; 48 bytes */
  uint64_t* keys;                      /* [capacity], 8-byte aligned: the occupied cells' keys, strictly ascending */
  int32_t*  counts;                    /* [capacity], 4-byte aligned: the cell's summed count, saturated at 2^31 - 1 */
  mot_voxel_merge_header* header;      /* device, 4-byte aligned; header->n_stored is the index's length, read ON THE DEVICE by the judge */
  long capacity;                       /* [0, 2^31 - 1] */
  float leaf_x, leaf_y, leaf_z;        /* written by the index call from `voxel`: the judge takes its leaf from here */
  int32_t reserved;                    /* 0 */
} mot_voxel_index;
int mot_index_voxel_maps_dev(mot_ctx* ctx, const mot_voxel_map_src* maps /* HOST array */, int n_maps, const mot_voxel_params* voxel,
        mot_voxel_index* index /* in: keys, counts, header, capacity; out: leaf */);
enum { MOT_MAP_OUTSIDE = 0, MOT_MAP_MOVING = 1, MOT_MAP_SPARSE = 2, MOT_MAP_ABSENT = 3, MOT_MAP_PRESENT = 4, MOT_MAP_CLASSES = 5 };
typedef struct mot_map_judge_params {
  int32_t min_count;                   /* [1, 2^31 - 1]: a cell counts as standing from this summed count on */
  int32_t reach;                       /* 0: the point's own cell; 1: its 27 neighbours */
} mot_map_judge_params;
int mot_export_map_points_dev(mot_ctx* ctx, int batch, const mot_voxel_index* index, const mot_map_judge_params* params, int class_mask, int frame,
        mot_track_point* d_points, long point_stride, mot_scene_segment* d_segments /* [batch][5] */,
        uint8_t* d_classes /* may be NULL */, long class_stride);
int mot_get_map_points(mot_ctx* ctx, int slot, const mot_voxel_index* index /* device blocks */, const mot_map_judge_params* params, int class_mask, int frame,
        mot_track_point* points, int point_capacity, int* n_points, mot_scene_segment segments[5],
        uint8_t* classes /* may be NULL */, int class_capacity, int* n_elevated);

/* on != 0: the fused entry points send their launch sequence (13 kernels with the tracker) as ONE hipGraph launch, captured once per launch geometry
 * (batch, chunks of the largest frame, tracker on / off, outputs); what changes per call without changing the geometry travels in the
 * device-resident argument block. For contexts somebody waits on frame by frame (one or a few streams): the host's part of a frame
 * drops to one copy and one launch. Default off; a runtime that cannot capture the sequence falls back to plain launches silently.
 * Kernel timing (mot_profile_kernel) uses plain launches while it is armed. */
int mot_set_launch_graphs(mot_ctx* ctx, int on);

/* on != 0: the fused entry points wrap their stages in roctx ranges — "mot:ground", "mot:cluster", "mot:box", "mot:tracker" on the issuing thread
 * (rocprofv3 --marker-trace shows them next to the kernels). libroctx64 is loaded at run time on first use; MOT_E_STATE when it is not installed
 * (the ranges then stay off, nothing else changes). A tracing aid of this library: the reference has none. */
int mot_set_trace_ranges(mot_ctx* ctx, int on);

/* How a tracker step (immUkfJpdaf for one frame of every stream of the call) is launched. Results are identical in every mode.
 *   MOT_TRACKER_AUTO (default)  by the number of streams in the call: STREAM up to 32, SPLIT beyond
 *   MOT_TRACKER_SPLIT           four launches (prologue, prediction + gating, association + update, merge / birth / outputs), the tracks of
 *                               ALL streams dealt over the whole chip: the throughput form (hundreds of streams per call)
 *   MOT_TRACKER_STREAM          ONE launch, one workgroup per stream doing the four phases behind workgroup barriers: the latency form (one
 *                               sensor per process, mot_sequence_dev's chained steps) — three launch boundaries fewer per frame */
enum { MOT_TRACKER_AUTO = 0, MOT_TRACKER_SPLIT = 1, MOT_TRACKER_STREAM = 2 };
int mot_set_tracker_mode(mot_ctx* ctx, int mode);

/* The same for frames in HOST memory — what the reference's nodes receive, one message per frame
 * (OT/src/groundremove/main.cpp:91-136, OT0/src/main.cpp:51-95) — pipelined: the H2D copy of this batch runs on the
 * context's copy stream into one of two staging buffers while the kernels of the previous batch run. Returns when
 * everything is queued. h_xyzw should be page-locked (mot_host_alloc): copies from pageable memory are staged by the
 * runtime and do not overlap. The host buffer may be reused after mot_wait_uploads (or mot_synchronize). */
int mot_frames_host(mot_ctx* ctx, const float* h_xyzw, long frame_stride, const int* n_points, int batch,
                    int run_tracker, const double* timestamps, const double* ego_v, const double* ego_yaw);
/* mot_frames_host for clouds WITHOUT a 4th value (ABI v6): h_xyz holds packed {x, y, z} records, 12 bytes a point, frame_stride FLOATS between the
 * frames of the batch (>= 3 * n_points[b]; 3 * the context's point capacity = one copy for the whole batch). pcl::PointXYZ — what groundRemove is
 * handed, OT/include/ground_removal.h:62-64 — has no 4th value, and the host link bounds a host-fed deployment: 25 % fewer bytes cross PCIe. The
 * records are expanded on the device (w = 1.0f, PCL's padding value: mot_get_ground's float4 records carry it); every result equals mot_frames_host's
 * on the same x, y, z. Same pipelining, same mot_wait_uploads. */
int mot_frames_host_xyz(mot_ctx* ctx, const float* h_xyz, long frame_stride, const int* n_points, int batch,
                        int run_tracker, const double* timestamps, const double* ego_v, const double* ego_yaw);
/* mot_frames_host for sensor_msgs/PointCloud2 payloads as they arrive (ABI v6): h_payloads[b] = the `data` of stream b's message (n_points[b] records of
 * point_step bytes, little-endian float32 fields at off_x / off_y / off_z; off_w = the float32 field that becomes the 4th value of the output records —
 * intensity — or -1: 1.0f, what fromROSMsg into PointXYZ leaves, OT/src/groundremove/main.cpp:100). One message per sensor stream, each in its own host
 * buffer: the raw records cross PCIe (copy stream, double-buffered) and are unpacked on the device; no host-side repacking, any point_step 12 .. 4096
 * (16: kitti2bag's x, y, z, intensity; 22-32: a velodyne driver's records with ring / time). Same pipelining as mot_frames_host, same mot_wait_uploads. */
int mot_frames_host_pointcloud2(mot_ctx* ctx, const void* const* h_payloads, const int* n_points, int batch, int point_step, int off_x, int off_y,
                                int off_z, int off_w, int run_tracker, const double* timestamps, const double* ego_v, const double* ego_yaw);
int mot_wait_uploads(mot_ctx* ctx);
int mot_host_alloc(size_t bytes, void** out);
int mot_host_free(void* p);
/* live tracks of slots 0..batch-1 (mot_export_tracks_dev's block) into HOST memory h_tracks[batch][max_per_slot] /
 * h_counts[batch], asynchronously on the context stream: valid after mot_synchronize */
int mot_fetch_tracks_async(mot_ctx* ctx, int batch, void* h_tracks, int max_per_slot, int32_t* h_counts);

/* read back results of the last mot_frames_dev / stage call for `slot` (host buffers; any may be NULL).
 * capacity_points: points each of elevated_xyzw / ground_xyzw / mask can hold; label_capacity: ints point_label can hold.
 * The counts are always delivered; MOT_E_CAPACITY (nothing copied) when a requested buffer is too small.
 *
 * PER-FRAME LIMITS OF THE CLUSTER AND BOX STAGE. A frame beyond one of them is REFUSED: the kernels stay inside their buffers, nothing outside
 * the frame's slot is touched, and mot_get_ground / mot_get_clusters / mot_get_boxes / mot_box_markers / mot_cluster_products (and the stage calls
 * that end in one of them: mot_box_fit, mot_box_fit_resident, mot_cluster_node_frame) answer MOT_E_CAPACITY with the limit's message for that
 * slot — on every call, not only the first — until a new stage call or fused batch writes the slot; the next frame is judged on its own.
 * With the tracker on (mot_frames_*, mot_sequence_dev) the tracker steps on the cut (possibly empty) box list of a refused frame and the
 * stream's mot_get_tracks reports MOT_E_CAPACITY like a dropped birth: sticky until mot_reset / mot_reset_slot / mot_reset_tracks_slot.
 *   - (tile, cluster) groups: at most max_points / 2 per frame, a group = the points of one cluster among 64 consecutive elevated points.
 *     REACHABLE: a cloud in no order at all whose clusters are tiny (n elevated points in random order over >> 64 clusters give ~n groups:
 *     more than max_points / 2 points of that kind). Scans in firing order stay far below (a few groups per tile). Raise max_points — or
 *     call mot_set_point_order(MOT_ORDER_ANY): the box stage then works on a copy of the elevated points in cluster order, where a cluster is
 *     ONE run of consecutive points. A run of r points starting at position s meets floor((s + r - 1) / 64) - floor(s / 64) + 1 tiles: one
 *     group, plus one per tile boundary inside the run; the N_e elevated points have ceil(N_e / 64) - 1 tile boundaries, each inside at most
 *     one run. A frame of C clusters therefore has at most C + ceil(N_e / 64) - 1 <= 4096 + max_points / 64 groups in that mode, whatever the
 *     input order; the mode sizes its group buffers to that bound (it exceeds max_points / 2 only below about 8500 points), so NOT reachable
 *     there: no frame is refused for its groups.
 *   - clusters: 4096 per frame. REACHABLE with mot_params.dilate == 0 (preset OBJECT_TRACKING0: single occupied cells two cells apart, up to
 *     10 000 on its 200 x 200 grid) and through mot_box_fit's num_cluster argument. NOT reachable through mot_cluster with the 3 x 3 dilation
 *     of preset OBJECT_TRACKING: separate components are at least 4 cells apart, 63 x 63 = 3969 on the 250 x 250 grid.
 *     mot_cluster itself delivers such a frame (the cluster stage has no limit of this kind). mot_box_fit_resident turns it down before a
 *     kernel runs and leaves the refusal on slot 0: mot_get_boxes / mot_box_markers / mot_get_clusters / mot_cluster_products of slot 0 answer
 *     it like a refusal raised on the device, until a stage call puts a new cloud there. mot_box_fit with num_cluster > 4096 is turned down
 *     before anything of slot 0 is overwritten: the slot keeps the frame it held, and its getters what they answered before.
 *   - accepted boxes: MOT_MAX_BOXES_PER_FRAME (1024) per frame. REACHABLE: 1025 clusters that pass the rule-based filter (about 33 000 points).
 *   - convex hull: 384 vertices per cluster. NOT reachable: a cluster's picture lies in 901 x 901 pixels, and a convex lattice polygon there
 *     (collinear points are not vertices) has at most 328 vertices — tests/test_emu_capacity.py computes the bound.
 *   - L-shape sampling: 128 pre-generated raw draws per cluster for ram_points (1 .. 128, checked by mot_create) indices. NOT reachable: a draw
 *     is rejected with probability below numPoints / 2^64 (the rejection sampling of std::uniform_int_distribution), so a cluster needs a
 *     129th raw draw with probability below 128 x numPoints / 2^64 (2^-33 for a cluster of 16 million points): a guard, not a limit an
 *     input can hit. */
int mot_get_ground(mot_ctx* ctx, int slot, float* elevated_xyzw, int* n_elevated, float* ground_xyzw,
                   int* n_ground, uint8_t* mask, int capacity_points);
int mot_get_clusters(mot_ctx* ctx, int slot, int32_t* grid, int* num_cluster, int32_t* point_label, int label_capacity);
int mot_get_boxes(mot_ctx* ctx, int slot, float* boxes, int max_boxes, int* n_boxes, int32_t* box_cluster,
                  int* n_undefined);
/* One record per track EVER created on the stream, in the reference's index order (its output vectors are sized that way,
 * OT/tracking/imm_ukf_jpda.cpp:995-1041): n_tracks grows with the stream's age, up to mot_params.max_tracks_ever (default
 * 64 x max_tracks_total). SIZE THE BUFFER FOR THAT: max_tracks >= max_tracks_ever never overflows; a long-running consumer either
 * creates the context with max_tracks_ever = its buffer size (ros/src/mot_ros_common.hpp does) or re-fetches with a larger buffer when
 * n_tracks > max_tracks (MOT_E_CAPACITY, nothing copied, n_tracks delivered — the step itself has run). The call costs a D2H copy
 * of 44 B x n_tracks + the live slots: consumers that only need the LIVE tracks every frame read mot_fetch_tracks_async /
 * mot_export_tracks[_packed]_dev instead, whose cost does not grow with the stream's age.
 * MOT_E_CAPACITY WITH the records delivered (n_tracks <= max_tracks) when births were dropped on this stream (no free track slot, or
 * max_tracks_ever tracks created), or when the box stage refused a frame of this stream in a fused call with the tracker on (the per-frame
 * limits above: the tracker stepped on an incomplete box list): STICKY until mot_reset / mot_reset_slot / mot_reset_tracks_slot. */
int mot_get_tracks(mot_ctx* ctx, int slot, mot_track* tracks, int max_tracks, int* n_tracks);

/* immUkfJpdaf for one frame of every slot 0..batch-1 with the boxes already on the DEVICE (global frame):
 * d_boxes_global holds box_stride_floats floats per slot (24 per box), m[b] (host) boxes per slot. mot_ego_update(slot)
 * precedes it as for mot_track_step. Asynchronous; read with mot_get_tracks / mot_export_tracks_dev. */
int mot_track_steps_dev(mot_ctx* ctx, const float* d_boxes_global, long box_stride_floats, const int* m, int batch,
                        const double* timestamps);

/* packs the LIVE tracks (track_manage != 0) of every slot, in track-id order, into a caller-owned DEVICE buffer
 * d_tracks[batch][max_per_slot] (mot_track records) and their number into d_counts[batch] (int32) — the fixed-size
 * per-stream record block that the multi-GPU harness all-gathers over RCCL. Asynchronous on the context stream. */
int mot_export_tracks_dev(mot_ctx* ctx, int batch, void* d_tracks, int max_per_slot, int32_t* d_counts);

/* The same records PACKED into one caller-owned DEVICE block of block_bytes bytes (16-byte aligned):
 *   int32 counts[batch]                       live tracks per slot (always the true number)
 *   (padding to a multiple of 16 bytes)
 *   mot_track records[]                       slot 0's live tracks in id order, then slot 1's, ... back to back
 * as many records as fit; sum(counts) > (block_bytes - header) / sizeof(mot_track) means the tail was dropped. This is the block
 * the multi-GPU harness all-gathers: at ~17 live tracks per stream it is a quarter of the fixed 64-slot block. Asynchronous. */
int mot_export_tracks_packed_dev(mot_ctx* ctx, int batch, void* d_block, long block_bytes);

/* ---------------------------------------------------------------- live tracks in the SENSOR frame
 * The tracker works in its own global frame (origin: the stream's first pose); the reference never publishes a position in it: OT/tracking/main.cpp:180-196
 * takes targetPoints and every visBBs[i] back into /velodyne through tf and pcl_ros::transformPointCloud and draws from those. The calls below do that on
 * the device, per stream, with the pose the stream's dead reckoning holds when the call is made.
 *
 * mot_sensor_pose: the two float 3 x 4 matrices (row major) of `slot`'s current pose — after the last mot_ego_update or fused tracker step; the pose
 * (0, 0, 0) before the first. global_from_sensor is what the fused path applies to the boxes (pcl_ros::transformPointCloud("/global", ...), main.cpp:143-158),
 * sensor_from_global what the calls below apply (transformPointCloud("/velodyne", ...), :183-184, :195). Each is restated step by step from the tf chain the
 * node runs (tf LinearMath, tf2 BufferCore, pcl_ros, Eigen in float): they are NOT each other's inverse bit for bit. A point p becomes
 * m[4r] * p.x + m[4r + 1] * p.y + m[4r + 2] * p.z + m[4r + 3], r = 0..2, in fp32, left to right. Host only, does not synchronise; either pointer may be NULL. */
int mot_sensor_pose(mot_ctx* ctx, int slot, float sensor_from_global[12], float global_from_sensor[12]);

/* mot_export_tracks_dev / mot_export_tracks_packed_dev / mot_fetch_tracks_async with the frame of the records chosen: same layouts, counts, order,
 * truncation rules and asynchrony.
 *   MOT_FRAME_GLOBAL  the existing call (byte-identical output)
 *   MOT_FRAME_SENSOR  px, py, pz of every record, and the 8 corners of vis_box when is_vis != 0, are replaced by their image under the slot's
 *                     sensor_from_global matrix; every other field is copied untouched — id, track_manage, is_static, is_vis, lifetime, v, yaw (the
 *                     reference draws its arrows with targetVandYaw as it is, main.cpp:230-246) and the zeros of a hidden track's vis_box.
 * The matrices are computed on the host from each slot's dead reckoning at call time and go out in one stream-ordered copy of batch x 48 bytes ahead of
 * the kernel (page-locked ring: no host synchronisation): the records are those of the pose of the LAST tracker step as long as no mot_ego_update of a
 * later frame has been made. Cost: unmeasured so far (profiles/sensor_frame_export.md: the method, and the figures once taken). Any other `frame`: MOT_E_ARG. */
enum { MOT_FRAME_GLOBAL = 0, MOT_FRAME_SENSOR = 1 };
int mot_export_tracks_frame_dev(mot_ctx* ctx, int batch, int frame, void* d_tracks, int max_per_slot, int32_t* d_counts);
int mot_export_tracks_packed_frame_dev(mot_ctx* ctx, int batch, int frame, void* d_block, long block_bytes);
int mot_fetch_tracks_frame_async(mot_ctx* ctx, int batch, int frame, void* h_tracks, int max_per_slot, int32_t* h_counts);

/* The `tracking` node's callback (OT/tracking/main.cpp:65-196, one track_box message) as ONE call: getOriginPoints (mot_ego_update), the frame's boxes
 * sensor -> global on the device (the tracker prologue of the fused path), immUkfJpdaf, and the live tracks back in the sensor frame. One upload of
 * m x 24 floats, ONE synchronisation, one device-to-host batch (max_tracks_total records + three counters) into the context's page-locked block; `tracks`
 * is a VIEW into that block, valid until the next call on this context (like mot_cluster_frame). Results equal, bit for bit, the stage-wise sequence
 * mot_ego_update -> boxes through global_from_sensor -> mot_track_step -> live records through sensor_from_global; mot_get_tracks / mot_track_get_state
 * afterwards see the same state.
 *   m > MOT_MAX_BOXES_PER_FRAME: MOT_E_ARG before anything runs (the ego pose is not advanced either).
 *   Dropped births: MOT_E_CAPACITY with the records delivered, sticky, as mot_track_step / mot_get_tracks report them: the step has run.
 *   The boxes go into a staging buffer of their own: the slot's box-stage residency is not touched — mot_get_boxes / mot_box_markers of the slot answer
 *   what they answered before. */
typedef struct mot_tracking_frame {
  double origin6[6];          /* getOriginPoints' egoPoints: what the node broadcasts as tf */
  int32_t n_live;             /* records below */
  int32_t n_ever;             /* tracks ever created on the stream: the size of the reference's output vectors */
  const mot_track* tracks;    /* n_live live tracks in id order, SENSOR frame; view into the context's page-locked block */
} mot_tracking_frame;
int mot_tracking_node_frame(mot_ctx* ctx, int slot, const float* boxes_sensor, int m, double timestamp,
                            double v_gps, double yaw_gps, mot_tracking_frame* out);

/* ---------------------------------------------------------------- cluster-node side products
 * What OT/src/cluster/main.cpp publishes besides the boxes, computed from the elevated cloud and the label grid resident in
 * `slot` (after mot_cluster / mot_box_fit on slot 0, or mot_frames_dev on any slot). SURVEY.md 8(f) rank 3.
 *   clustered cloud  makeClusteredCloud(), component_clustering.cpp:311-339 — for every elevated point whose cell carries a
 *                    cluster: the CELL CENTRE (cell_size*xI - roiM/2 + cell_size/2, same for y, z = -1), in input order
 *   obstacle list    setObsMsg(), :341-379 — the same point for the FIRST elevated point of every labelled cell (the
 *                    function zeroes the cell in its by-value copy of the grid), in input order, with the cluster id
 *   cost map         createCostMap(), :425-457 — cost_width x cost_height ints, 15 per elevated point (z <= height_limit,
 *                    outside the car footprint) saturating at 100
 * The constants are file-scope globals of the reference (component_clustering.h:15, component_clustering.cpp:15-24). */
typedef struct mot_side_params {
  float cell_size;                 /* grid_size 0.2 */
  int32_t cost_width, cost_height; /* g_cell_width, g_cell_height 50, 50 */
  double cost_resolution;          /* g_resolution 1.0 */
  double cost_offset_x, cost_offset_y; /* g_offset_x, g_offset_y 0, 25 */
  double height_limit;             /* HEIGHT_LIMIT 0.1 */
  double car_length, car_width;    /* CAR_LENGTH 4.5, CAR_WIDTH 2 */
  double cost_offset_z;            /* g_offset_z -2: only the OccupancyGrid origin (setOccupancyGrid, :410-422) uses it */
} mot_side_params;
int mot_side_params_default(mot_side_params* out);
/* every output may be NULL; clustered_xyzw: max_clustered x 4 floats (x, y, z, 0); obstacles_xyzc: max_obstacles x 4 floats
 * (x, y, z, cluster id); cost_map: cost_width*cost_height int32 (<= 65536 cells). MOT_E_CAPACITY when a list does not fit. */
int mot_cluster_products(mot_ctx* ctx, int slot, const mot_side_params* sp, float* clustered_xyzw, int max_clustered,
                         int* n_clustered, float* obstacles_xyzc, int max_obstacles, int* n_obstacles, int32_t* cost_map);
/* the same on a caller-supplied cloud and label grid (the argument lists of the three reference functions): uploads them
 * into slot 0 first. elevated_xyzw: n x 4 floats; grid: num_grid x num_grid int32, x-major.
 * LABEL RANGE: 0 .. 65535 (the device's grid is 16 bits wide; componentClustering's labels never exceed numGrid^2 / 2 = 31 250); any other
 * value is MOT_E_ARG, checked before slot 0 is touched. The reference's int grid would take any int as an obstacle's cluster id. */
int mot_cluster_products_host(mot_ctx* ctx, const float* elevated_xyzw, int n, const int32_t* grid, const mot_side_params* sp,
                              float* clustered_xyzw, int max_clustered, int* n_clustered, float* obstacles_xyzc,
                              int max_obstacles, int* n_obstacles, int32_t* cost_map);
/* The rviz CUBE of every box: mark_cluster(), OT/src/cluster/box_fitting.cpp:161-209, which getBoundingBox calls (:410) for each
 * cluster whose box it keeps. For box i of `slot`'s last box stage (mot_box_fit / mot_box_fit_resident on slot 0, mot_frames_dev /
 * mot_sequence_dev on any slot), in the order mot_get_boxes returns them:
 *   centroid_extent[6*i + 0..2] = pcl::compute3DCentroid of the cluster's points: float sums in input order, divided by the count
 *   centroid_extent[6*i + 3..5] = pcl::getMinMax3D's max - min, as floats (marker.scale; the caller substitutes 0.1 for a 0, :192-199)
 * centroid_extent may be NULL (only *n_boxes is written). MOT_E_CAPACITY when max_boxes < *n_boxes. MOT_E_STATE when the slot's cloud has
 * been replaced since its last box stage (mot_ground_remove*, mot_cluster, mot_cluster_products_host write into slot 0): the cluster
 * order the cubes are folded from would belong to another cloud. */
int mot_box_markers(mot_ctx* ctx, int slot, float* centroid_extent, int max_boxes, int* n_boxes);

/* ---------------------------------------------------------------- one call per node callback (round 5)
 * What the reference's `cluster` node does per scan (OT/src/cluster/main.cpp:63-234: componentClustering, makeClusteredCloud, createCostMap,
 * setObsMsg, boxFitting with its cube markers) as ONE call on the elevated cloud in host memory: one upload, every kernel on the resident
 * copy, TWO synchronisations (the counts, then every result in one batch of copies) instead of the nine of the call-by-call sequence
 * mot_cluster + mot_cluster_products + mot_box_fit_resident + mot_box_markers — same kernels, same results. The results are VIEWS into a
 * page-locked block owned by the context, valid until the next call on this context (a node copies them into its messages anyway). */
typedef struct mot_cluster_frame {
  int32_t num_cluster;             /* componentClustering's numCluster */
  int32_t n_clustered;             /* makeClusteredCloud */
  int32_t n_obstacles;             /* setObsMsg */
  int32_t n_boxes, n_undefined;    /* boxFitting (n_undefined: see mot_box_fit) */
  int32_t cost_cells;              /* cost_width * cost_height */
  const float* clustered_xyzw;     /* n_clustered x 4 (x, y, z, 0) */
  const float* obstacles_xyzc;     /* n_obstacles x 4 (x, y, z, cluster id) */
  const int32_t* cost_map;         /* cost_cells */
  const float* boxes;              /* n_boxes x 8 x 3 */
  const int32_t* box_cluster;      /* n_boxes: 1-based cluster id of every box */
  const float* centroid_extent;    /* n_boxes x 6: mot_box_markers */
} mot_cluster_frame;
int mot_cluster_node_frame(mot_ctx* ctx, const float* elevated_xyzw, int n, const mot_side_params* sp, mot_cluster_frame* out);

/* The `ground` node's call (OT/src/groundremove/main.cpp:120: groundRemove) with the two clouds returned as VIEWS into the context's page-locked
 * block (valid until the next call on this context) instead of copies into caller buffers: mot_ground_remove's results, one device-to-host
 * transfer less staging. *elevated_xyzw / *ground_xyzw: n_elevated / n_ground x 4 floats. */
int mot_ground_node_frame(mot_ctx* ctx, const float* xyzw, int n, const float** elevated_xyzw, int* n_elevated, const float** ground_xyzw,
                          int* n_ground);

/* ---------------------------------------------------------------- input decode
 * sensor_msgs/PointCloud2 payload -> the float4 (x, y, z, w) layout of this library, on the device: what
 * `fromROSMsg(*input, *cloud)` (OT/src/groundremove/main.cpp:100; pcl_conversions + pcl::fromPCLPointCloud2, not part of
 * the reference tree) does for PointXYZ — copy the FLOAT32 fields named x, y, z of every point (NaN points included), at
 * their byte offsets inside a record of `point_step` bytes, little endian. w = the FLOAT32 at `off_w`, or 1.0f (what
 * PointXYZ's padding holds) when off_w < 0. A KITTI velodyne .bin file is the case point_step = 16, offsets 0/4/8/12.
 * d_data and d_xyzw are DEVICE pointers (d_data only byte aligned is fine); asynchronous on the context stream, so the
 * result can be handed straight to mot_frames_dev. Parity: restated from the PCL documentation, pinned against a numpy
 * structured-array view in tests/ (PCL itself is not available here). */
int mot_decode_pointcloud2_dev(mot_ctx* ctx, const void* d_data, int n_points, int point_step, int off_x, int off_y, int off_z,
                               int off_w, float* d_xyzw);

/* ---------------------------------------------------------------- measurement helpers (bench.py) */
/* Re-runs only the named stage `iters` times on the data resident from the last mot_frames_dev call,
 * bracketed by hipEvents ON THE CONTEXT STREAM; returns average milliseconds per iteration.
 * stage: 0 ground, 1 cluster, 2 box, 100 the three stateless stages; single kernels: 10-12 ground, 21 cluster,
 * 30-34 box; 35-37 the regrouping pass of MOT_ORDER_ANY (35 labels + first histogram, 36 the sort by cluster label, 37 the gather of points and
 * cells into the cluster-ordered copy: MOT_E_STATE in MOT_ORDER_SCAN; stages 2 and 100 include them when the mode is on, and need the last
 * mot_frames_dev to have run in the current mode); 40 re-runs the tracker kernel with the last frame's arguments (that ADVANCES tracker state: bench only). */
int mot_time_stage(mot_ctx* ctx, int stage, int batch, int iters, float* ms_per_iter);
/* In-run timing: from now on every `every`-th mot_frames_dev / mot_frames_host call brackets its launch of kernel `kernel_id`
 * (ids as for mot_time_stage; 0 = off) with a HIP event pair on the context stream, up to 64 launches; mot_profile_read synchronises,
 * returns mean / min / max of the recorded durations in milliseconds and re-arms. This is the kernel's duration INSIDE the
 * running pipeline (other contexts' kernels overlapping it), the number a rocprofv3 kernel trace of the same run reports. */
int mot_profile_kernel(mot_ctx* ctx, int kernel_id, int every);
int mot_profile_read(mot_ctx* ctx, float* mean_ms, float* min_ms, float* max_ms, int* samples);

#ifdef __cplusplus
}
#endif
#endif /* MOT_H_ */
