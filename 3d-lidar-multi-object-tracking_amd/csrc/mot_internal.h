// mot_internal.h — shared between the HIP kernels (*.hip) and the host side of the C-ABI (mot_api.hip).
// Product code. No oracle code is included or linked here.
#ifndef MOT_INTERNAL_H_
#define MOT_INTERNAL_H_

#ifndef MOT_HIPEMU
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#include "../../include/mot.h"
#include "mot_math.h"

// ---- geometry of the launches --------------------------------------------------------------
#ifndef MOT_GROUND_BLOCK
#define MOT_GROUND_BLOCK 256
#endif
constexpr int kGroundBlock = MOT_GROUND_BLOCK;    // threads per workgroup of the min-z kernel
#ifndef MOT_GROUND_ITEMS
#define MOT_GROUND_ITEMS 8
#endif
constexpr int kGroundItems = MOT_GROUND_ITEMS;    // points per thread
constexpr int kGroundChunk = kGroundBlock * kGroundItems;  // 2048 points = 32 KB per workgroup
#ifndef MOT_COMPACT_BLOCK
#define MOT_COMPACT_BLOCK 512
#endif
constexpr int kCompactBlock = MOT_COMPACT_BLOCK;  // threads per workgroup of the compaction kernel
#ifndef MOT_COMPACT_CHUNK
#define MOT_COMPACT_CHUNK 4096
#endif
constexpr int kCompactChunk = MOT_COMPACT_CHUNK;  // points per workgroup (4096 = 64 KB in flight); a multiple of 4096
constexpr int kCompactItems = kCompactChunk / kCompactBlock;  // points per thread
constexpr int kSubTiles = kCompactChunk / 64;     // 64-point wave tiles per chunk, kSubTiles / 64 per lane in the tile scan
constexpr int kMinzInit = 0x447A0000;             // ordered key of 1000.0f (Cell::Cell, ground_removal.cpp:35-38)

// descriptor word of the decoupled look-back in the compaction kernel (one 8-byte granule, written
// by ONE store and read by ONE load, so it can never be seen torn):
//   [63:62] status 1 = chunk aggregate, 2 = inclusive prefix
//   [61:42] launch epoch (a descriptor whose epoch is not the current one is "not ready": no reset pass)
//   [41:21] elevated count, [20:0] ground count   (frames of up to 2^21-1 points)
constexpr int kDescCountBits = 21;
constexpr unsigned long long kDescCountMask = (1ull << kDescCountBits) - 1;
constexpr int kDescEpochShift = 42;
constexpr unsigned kDescEpochMask = (1u << 20) - 1;
constexpr unsigned long long kDescAggregate = 1ull << 62;
constexpr unsigned long long kDescPrefix = 2ull << 62;
constexpr int kMaxPointsPerFrame = (1 << kDescCountBits) - 1;

// parameters as the kernels want them (floats pre-combined exactly as the reference combines them)
struct MotDevParams {
  float r_min, r_max, r_span;                  // r_span = rMax - rMin (fp32, ground_removal.cpp:72)
  float k_bin;                                 // 120 / r_span, for the guarded fast path only
  float t_hmin, t_hmax, t_hdiff, h_sensor;
  double ground_margin;
  double gk[3];                                // normalised 3-tap Gaussian (gaus_blur.cpp:26-49), host libm
  int crop_enable;
  float crop_z_min, crop_z_max, crop_x_min, crop_x_max, crop_y_min, crop_y_max;
  int num_grid, occ_min_count, dilate;
  float roi_m, roi_half;                       // roi_half = roiM/2 (fp32)
  float k_grid;                                // numGrid / roiM, for the guarded fast path of the Cartesian cell only
  float pic_scale, pic_full, pic_half;         // picScale*roiM and roiM*picScale/2 (fp32 products)
  int ram_points, l_slope_dist, l_num_points, lshape_side_cond, min_points;
  int rng_mapping;                             // MOT_RNG_LIBSTDCXX10 / 11: how a 64-bit draw becomes a sample index
  float sensor_height;
  float t_height_min, t_height_max, t_width_min, t_width_max, t_len_min, t_len_max, t_area_max, t_ratio_min,
      t_ratio_max, min_len_ratio, t_pt_per_m3;
};

// The elevated cloud between the ground stage and the stages after it. Stage-wise entry points hold it as the ABI's float4 records; the FUSED
// path's default (ground cloud / mask on demand) writes it PACKED, 12 bytes a point (x, y, z: nothing after groundRemove reads the 4th float —
// the reference's elevatedCloud is PointCloud<PointXYZ>): 4 bytes less written by the compaction kernel and 4 less read by the label kernel per
// elevated point, 0.19 of the 3.8 GB a 512-frame launch sequence moves (round 5). A slot's cloud starts at the same address either way
// (elevated + slot * cap float4); `packed` travels with the buffer descriptors, every reader goes through mot_load_xyz.
#ifndef MOT_PACKED_ELEVATED
#define MOT_PACKED_ELEVATED 1
#endif
struct PackedXyz { float x, y, z; };
static_assert(sizeof(PackedXyz) == 12, "12-byte points");
MOT_HD float4 mot_load_xyz(const float4* slot_base, long i, int packed) {
  if (packed) { const PackedXyz q = reinterpret_cast<const PackedXyz*>(slot_base)[i]; float4 r; r.x = q.x; r.y = q.y; r.z = q.z; r.w = 0.f; return r; }
  return slot_base[i];
}

struct OccWord { unsigned word, a, b, pad; };   // word index in the bit-plane, its "seen >= 1" and "seen >= 2" bits

// What changes from one launch sequence to the next without changing the launch geometry — the input cloud's address and the
// look-back epoch — as a DEVICE-resident record (part of the argument block): a launch sequence captured once in a hipGraph
// (mot_api.hip, small batches: the per-frame latency path) reads them from here instead of from its baked-in kernel arguments.
struct FrameLaunch {
  const float4* in;
  long in_stride;
  unsigned epoch;
  int pad;
};

// device buffers of the ground stage for a batch of frames (frame b = slot b)
struct GroundBuffers {
  const FrameLaunch* launch;  // non-null (graph-captured sequences): in / in_stride / epoch are read from this record, not from the fields below
  const float4* in;        // [B][in_stride] points
  long in_stride;          // in points
  const int* n;            // [B] points per frame (device)
  uint2* pairs;            // [B][max_chunks][kGroundChunk] {polar cell, ordered-int key of a partial min z}
  int* pair_count;         // [B][max_chunks] entries each workgroup of the min-z kernel produced
  unsigned short* cell;    // [B][cap] polar cell of every point (0xffff: takes no part), written by the min-z kernel, read by the compaction kernel
  float* gzmax;            // [B][cap / 8] per aligned group of 8 points (a 128-byte line of the cloud): the largest z among its points that have a cell (+-0 as +0; NaN
                           // if one of them has a NaN z; -inf if none has a cell), written by the min-z kernel; the elevated-only compaction skips lines by it
  float* hg;               // [B][9600] hGround of ground cells, -inf for non-ground cells
  unsigned long long* desc;  // [B][max_chunks]
  int* ticket;             // [B], zero between launches (the workgroup drawing the last ticket re-arms it)
  unsigned epoch;          // launch epoch, 1..kDescEpochMask
  float4* elevated;        // [B][cap]
  int elevated_packed;     // the elevated-only compaction writes 12-byte points (see PackedXyz)
  float4* ground;          // [B][cap]
  uint8_t* mask;           // [B][cap] or null
  int* counts;             // [B][kCountsStride]: n_elevated, n_ground, n_dropped, ...
  long cap;                // capacity (points) per frame of the outputs
  int max_chunks;
  // Occupancy of the cluster stage's grid, or null: when set, the compaction kernel also files every elevated point under its
  // Cartesian cell (mapCartesianGrid's histogram, component_clustering.cpp:36-50) while the point is still in registers, and
  // the fused path skips cart_occupancy_kernel. Every workgroup (chunk) leaves the non-zero words of its two bit-planes
  // ("cell seen >= 1" / ">= 2" within the chunk) as a list; the labelling kernel folds the lists of a frame.
  OccWord* occ_list;       // [B][occ_chunks][kPlaneWords]
  int* occ_count;          // [B][occ_chunks] entries of each list
  int occ_chunks;
  // Cartesian cell (xI * 256 + yI; 0xffff = outside the ROI) of every ELEVATED point, at its position in the elevated cloud, or null:
  // written next to the occupancy (same value, still in registers) so that the box stage's label kernel reads 2 bytes per point
  // instead of recomputing the cell (only with occ_list, and only for grids of fewer than 256 cells per side: 0xffff must be free)
  unsigned short* ecell;   // [B][cap]
};

// ---- cluster + box stages ------------------------------------------------------------------
constexpr int kRowWords = 8;                       // a grid row (<= 256 cells) as 8 x 32 bits
constexpr int kPlaneWords = MOT_MAX_GRID * kRowWords;  // 2048 words: bit (x*256 + y)
constexpr int kMaxRuns = 32768;                    // 128 runs per row x 256 rows
constexpr int kMaxClusters = 4096;                 // per frame (MOT_E_CAPACITY beyond)
constexpr int kMaxBoxesPerFrame = 1024;
constexpr int kRngTable = 128;                     // raw mt19937_64(0) outputs kept on the device
constexpr int kCountsStride = 12;                  // ints per frame in `counts`
enum { kCntElev = 0, kCntGround = 1, kCntDropped = 2, kCntClusters = 3, kCntBoxes = 4, kCntUndef = 5, kCntFlags = 6, kCntPoly = 7, kCntGroups = 8,
       kCntIrregular = 9 };   // kCntGroups, kCntIrregular: label kernel -> index kernel, zero between launches
enum { kFlagClusterOverflow = 1, kFlagBoxOverflow = 2, kFlagRngExhausted = 4, kFlagHullOverflow = 8, kFlagGroupOverflow = 16 };
// boxes of frame b's owner row, as every kernel that walks the row counts them: a frame the box stage refused has no owners (link.hip: its points read -1 throughout)
MOT_HD int mot_owner_boxes(const int* counts, int b) {
  const int* cnt = counts + (long)b * kCountsStride;
  const int M = cnt[kCntFlags] != 0 ? 0 : cnt[kCntBoxes];
  return M < 0 ? 0 : (M > kMaxBoxesPerFrame ? kMaxBoxesPerFrame : M);
}
// workgroups per frame of a launch that takes `chunk` points a workgroup, over frames of at most max_n points: at least one, at most what the scratch has rows for
inline int mot_launch_chunks(int max_n, int chunk, int max_chunks = 0x7fffffff) {
  const int chunks = (max_n + chunk - 1) / chunk;
  return chunks < 1 ? 1 : (chunks > max_chunks ? max_chunks : chunks);
}

struct alignas(64) ClusterStats {   // per cluster, accumulated by the label kernel, reset by the finalize kernel. A cache line each: the five
                               // atomics of a commit go to ONE line and no two clusters share one (40-byte records: the label kernel alone
                               // 4 us faster, the four-context line 2 % slower, profiles/r03_box_stage_experiments.txt)
  unsigned long long count_groups;   // low word: numPoints; high word: (tile, cluster) groups of the cluster = 64-point tiles that hold a point
                               // of it (ONE 64-bit atomic for both: a wall's statistics are hit by every chunk it spans)
  unsigned long long argmin;   // (key(m) << 32) | idx        -> minimum = smallest slope, first occurrence
  unsigned long long argmax;   // (key(m) << 32) | ~idx       -> maximum = largest slope, first occurrence
  int first;                   // smallest point index (clusteredPoints[i][0])
  int maxz_key;                // ordered key of max z (init key(-99)); -0 and +0 share the key of +0
  int first_zero;              // smallest index of a point with z == +-0 (0x7fffffff if none): the sign of a zero maximum
  int pad;
};
static_assert(sizeof(ClusterStats) == 64, "ClusterStats layout");
struct PointGroup {            // the points of one 64-point tile that belong to one cluster (label kernel)
  unsigned long long mask;     // lanes of the tile
  int label;                   // bits 0-15: 1-based cluster id; bits 16-31: GROUPS of the cluster in earlier tiles of the same chunk
  int tile;                    // bits 0-19: points 64*tile .. 64*tile + 63; bits 20-31: POINTS of the cluster in EARLIER tiles of the
                               // same label-kernel workgroup (2048-point chunk)
};
constexpr int kGroupTileBits = 20;
constexpr int kGroupTileMask = (1 << kGroupTileBits) - 1;
constexpr int kGroupLabelMask = 0xffff;
struct SortedGroup {           // the same groups in cluster order (index kernel): what the per-cluster kernels walk
  unsigned long long mask;     // lanes of the tile
  int tile;                    // points 64*tile .. 64*tile + 63
  int before;                  // points of the cluster in its earlier groups (= rank of the group's first point within the cluster)
};
constexpr int kIndexPointBits = 19;   // the index kernel's fast path packs (groups << 19 | points) per cluster: frames of up to 2^19 points
constexpr int kWgClusters = 64;     // distinct clusters a label-kernel workgroup merges in LDS (its open-addressed table)
struct BoxCandidate {          // per cluster, written by the box kernels
  float pc[8];                 // 4 corners (x,y)
  float max_z;
  int accepted, undefined, branch;   // branch: 0 L-shape (complete), 1 min-area rectangle (polygon pending / done)
  int poly_off, poly_n;        // candidate hull points of the cluster in the frame's polygon pool
  int off_x, off_y;            // offsetInitX / offsetInitY (box_fitting.cpp:224-225)
  int num_points, pad;
};

// A cell's cluster label on the device: 16 bits. A grid of at most 256 x 256 cells has at most 32 768 runs, hence clusters; the ABI's int32
// cartesianData (component_clustering.h:20-22) is widened / narrowed on the host by the entry points that cross it. Half the bytes of the labelling
// kernel's grid write and half the footprint of the label kernel's per-point gathers (each XCD's L2 fetches a frame's occupied lines for itself).
typedef unsigned short GridLabel;
struct ClusterBuffers {
  const float4* elevated;      // [B][cap]
  int elevated_packed;         // 12-byte points (the fused path's default: see PackedXyz)
  long cap;
  int* counts;                 // [B][kCountsStride]
  unsigned* plane_a;           // [B][2048] cell seen >= 1   (filled by cart_occupancy_kernel: the stage-wise mot_cluster)
  unsigned* plane_b;           // [B][2048] cell seen >= 2
  const OccWord* occ_list;     // fused path: the compaction kernel's per-chunk lists instead (see GroundBuffers), else null
  const int* occ_count;
  const int* n_in;             //   ... points of the frame's input cloud (chunks in use)
  int occ_chunks;
  const unsigned short* ecell; // fused path: Cartesian cell of every elevated point from the compaction kernel (see GroundBuffers), else null
  unsigned* ccl_parent;        // [B][kMaxRuns] union-find array of the labelling kernel for frames with more runs than its LDS holds
  GridLabel* grid;             // [B][65536] labels (16 bits each), x-major with stride num_grid
  int* label;                  // [B][cap] label of each elevated point
  ClusterStats* stats;         // [B][kMaxClusters]
  BoxCandidate* cand;          // [B][kMaxClusters]
  float* boxes;                // [B][kMaxBoxesPerFrame][24]
  int* box_cluster;            // [B][kMaxBoxesPerFrame]
  const unsigned long long* rng;  // [kRngTable]
  int* poly;                   // [B][cap] candidate hull points (x | y << 16) of the min-area-rectangle clusters
  PointGroup* groups;          // [B][cap / 2] (tile, cluster) groups of the frame, any order
  int group_cap;               // cap / 2 (MOT_ORDER_ANY: max(cap / 2, kMaxClusters + cap / 64), see mot_regroup_group_cap)
  uint2* group_scratch;        // [B][group_cap] or null: where the index kernel buckets the groups of a many-group frame. Null: in the polygon pool
                               // (cap ints = cap / 2 entries per slot: only large enough while group_cap <= cap / 2)
  int* order;                  // [B][kMaxClusters] clusters by falling size: the per-cluster kernels start on the largest ones
  int* cluster_start;          // [B][kMaxClusters + 1] points of all earlier clusters (a cluster's own slots of the polygon pool start here)
  int* cluster_gstart;         // [B][kMaxClusters + 1] first entry of every cluster in `gsorted`
  SortedGroup* gsorted;        // [B][cap / 2] the frame's groups by cluster, in input (tile) order inside a cluster
  int* pix;                    // [B][cap] picture pixel of every elevated point (x | y << 16, x = 0xffff outside), box_fitting.cpp:244-254
  int2* wgtab;                 // [B][max_wg][kWgClusters] {cluster, points | groups << 16} per label-kernel workgroup (its LDS table, empty = {0,0})
  int max_wg;                  // cap / 2048 rounded up
};

// occupancy_done: the compaction kernel of the ground stage already filled the bit-planes (fused path)
void mot_launch_cluster(const MotDevParams& p, const ClusterBuffers& c, int batch, int max_n, hipStream_t stream, bool occupancy_done = false);
void mot_launch_box(const MotDevParams& p, const ClusterBuffers& c, int batch, int max_n, hipStream_t stream);
// pieces, for the stage-wise host entry points and per-kernel timing
void mot_launch_cluster_kernel(int which, const MotDevParams& p, const ClusterBuffers& c, int batch, int max_n, hipStream_t stream);
void mot_launch_stats_init(const ClusterBuffers& c, int batch, hipStream_t stream);
void mot_launch_point_labels(const MotDevParams& p, const ClusterBuffers& c, int slot, int max_n, hipStream_t stream);
void mot_launch_box_kernel(int which, const MotDevParams& p, const ClusterBuffers& c, int batch, int max_n, hipStream_t stream);

// ---- MOT_ORDER_ANY: the elevated points regrouped by cluster before the box stage (regroup.hip) -------------------------------
// A stable sort of every frame's elevated points by cluster label (0 = no cluster, first; labels 1 .. 4096 after it), two LSD radix passes
// of 7 + 6 bits over 2048-point chunks, and a copy of the points (12 bytes each) and their cells in that order. The box stage then runs on
// the copy: a cluster's points are neighbours there, in the order they had in the input.
constexpr int kRegroupDigits = 128;               // histogram row of a chunk (pass 0: 128 digits, pass 1: 64)
// Groups of a frame AFTER regrouping: a cluster's points form one run of the copy, and a run of r points that starts at position s meets
// floor((s + r - 1) / 64) - floor(s / 64) + 1 tiles: one group, plus one for every tile boundary inside the run. The N_e points of a frame have
// ceil(N_e / 64) - 1 tile boundaries between them and each lies inside at most one run, so a frame of C clusters has at most
// C + ceil(N_e / 64) - 1 <= kMaxClusters + cap / 64 - 1 groups, whatever the input order. (The unlabelled points in front form no group.)
// That exceeds the default cap / 2 only for cap < 2 * kMaxClusters * 64 / 62 ~ 8456 points.
constexpr long mot_regroup_group_cap(long cap) { return cap / 2 > kMaxClusters + cap / 64 ? cap / 2 : kMaxClusters + cap / 64; }
struct RegroupBuffers {
  unsigned short* key;         // [B][cap] cluster label of every elevated point (0 .. kMaxClusters), input order
  unsigned* tmp;               // [B][cap] after pass 0: input index (bits 0-20) | high digit of the key (bits 21-26), by low digit
  int* hist;                   // [B][max_wg][kRegroupDigits] per-chunk digit counts, turned into the chunks' scatter offsets by the scan kernel
  float4* xyz;                 // [B][cap] the cluster-ordered copy: 12-byte points, a slot every cap * 16 bytes like `elevated`
  unsigned short* cell;        // [B][cap] their Cartesian cells (fused path; unused when the source has none)
  int* label;                  // [B][cap] per-point labels IN INPUT ORDER are written here by the label pass, or null
};
// which = 0 label pass (+ histogram of the low digit), 1 the sort (scan, scatter by low digit, histogram of the high digit, scan),
// 2 scatter by high digit = gather of points and cells into the copy, -1 all three. `src` is the frame as the cluster stage left it.
void mot_launch_regroup(int which, const MotDevParams& p, const ClusterBuffers& src, const RegroupBuffers& r, int batch, int max_n, hipStream_t stream);

// ---- cluster-node side products (side.hip) ------------------------------------------------------
struct SideDevParams {
  float cell_size;
  int cost_width, cost_height;
  double cost_resolution, center_x, center_y;   // map_center_x/y, component_clustering.cpp:428-429
  double height_limit, car_length, car_width;
};
struct SideBuffers {
  const float4* elevated;   // the slot's elevated cloud
  int elevated_packed;      // 12-byte points (see PackedXyz)
  const GridLabel* grid;    // the slot's label grid, x-major with stride num_grid
  const int* counts;        // the slot's counters (kCntElev)
  int* cell_first;          // [MOT_MAX_GRID^2] scratch: first point of every labelled cell
  int2* chunk_counts;       // [ceil(cap / 1024)] scratch: clustered points / obstacles of every 1024-point chunk
  float4* clustered;        // [max_clustered]
  float4* obstacles;        // [max_obstacles] (x, y, z, cluster)
  int* cost;                // [cost_width * cost_height]
  int* out_counts;          // [2] clustered points, obstacles
  int max_clustered, max_obstacles;
};
void mot_launch_side_products(const MotDevParams& p, const SideDevParams& sp, const SideBuffers& s, int max_points, hipStream_t stream);
void mot_launch_box_markers(const ClusterBuffers& c, int slot, int n_boxes, float* out /*[n_boxes][6]*/, hipStream_t stream);

// ---- tracker stage ---------------------------------------------------------------------------
#ifndef MOT_TRACK_BLOCK
#define MOT_TRACK_BLOCK 512
#endif
constexpr int kTrackBlock = MOT_TRACK_BLOCK;      // one workgroup (a wave per live track at a time) steps one sensor stream
constexpr int kTrackWaves = kTrackBlock / 64;
constexpr int kGateWords = kMaxBoxesPerFrame / 64;  // gate bit-mask of one track over the frame's boxes

// Track storage. The reference keeps every track it ever created (targets_ only grows, OT/tracking/imm_ukf_jpda.cpp:972-989) and
// addresses a track by its index in that vector. Here a track's filter state lives in one of T = max_tracks_total SLOTS; a track
// keeps its slot while it is alive and for one more step after it died (that step's outputs still show the dead track as the
// reference would), then the slot is free again. What outlives the slot, per track EVER created, addressed by the reference's
// index: the merged position (the over-segmentation merge tests EVERY track's last position against the visible boxes, dead
// tracks included, :666-700), lifetime_, the static flag and the frozen speed / yaw (outputs), and the slot map — 44 bytes instead of ~2 KB.
constexpr int kEverFactor = 64;   // default capacity of the per-ever-track arrays, as a multiple of max_tracks_total
struct TrackTomb { int lifetime, is_static; double v, yaw; };   // v, yaw: x_merge_(2..3) as the filter left them — the reference keeps reporting them (yaw + the current ego yaw, imm_ukf_jpda.cpp:1012-1016)
struct DevTrack {               // filter state of one track (the reference's class UKF, OT/include/ukf.h:15-263)
  double x[4][5];               // x_merge_, x_cv_, x_ctrv_, x_rm_
  double P[4][25];              // P_merge_, P_cv_, P_ctrv_, P_rm_ (row-major)
  double mode[3];               // modeProbCV_, modeProbCTRV_, modeProbRM_
  double zpred[3][2], S[3][4], K[3][10];
  double init_meas[2], dist_from_init, best_yaw;
  int lifetime, track_num, is_static, is_vis, has_bbox, has_best, ref_id, pad1;   // ref_id: index the reference gives this track (its position in targets_)
  float bbox[24], best_bbox[24];
};

struct TrackFrameArgs {         // per slot and step, written by the host
  int m;                        // boxes this frame
  int first_frame;              // !init_  (imm_ukf_jpda.cpp:741)
  int run;                      // 0: leave this slot untouched
  int pad;
  double dt;                    // (timestamp - timestamp_) / 1e6   (:807)
  double ego_yaw;               // egoPoints_[0][2]                 (:1010)
};

struct MotTrackParams {
  double gamma_g, p_g, p_d, distance_thres, bb_yaw_change_thres, seed_px, seed_py;
  int life_time_thres, seed_box_index;
};

struct Vec2d { double x, y; };
struct TrackItem { int b, li; };  // one unit of per-track work: live track `li` (index into the stream's live list) of stream `b`
// sensor -> global change of frame of the fused path: the float 3 x 4 matrix the tracking node's tf chain ends in
// (mot_api.hip: tf_velodyne_to_global), row major; the MOT_FRAME_SENSOR exports carry the way back (tf_global_to_velodyne) in the same record
struct EgoTf { float m[12]; };

struct TrackBuffers {
  DevTrack* tracks;             // [B][T] by SLOT
  int* nt;                      // [B] tracks ever created = the next reference index
  const float* boxes;           // [B][box_stride] floats, 24 per box, global frame: what the tracker reads
  long box_stride;              // floats per slot (kMaxBoxesPerFrame * 24 for the library's own buffer)
  const float* boxes_sensor;    // fused path: [B][kMaxBoxesPerFrame][24] boxes of the box stage in the sensor frame, or null
  const EgoTf* ego;             //   ... the sensor -> global transform per slot: the prep kernel writes their global-frame image
  float* boxes_out;             //   ... into this buffer (= boxes)
  const TrackFrameArgs* args;   // [B]
  unsigned long long* gate;     // [B][T][kGateWords]
  unsigned long long* prog;     // [B][T][kGateWords]
  int* live;                    // [B][2*T]: compact list of the SLOTS of the tracks alive at the start of the step, in the order of their reference
                                // indices; then their flags (0 killed by a guard, 1 reached gating, 2 reached gating in second initialisation)
  int* nlive;                   // [B] length of that list (written by the previous step's finish kernel)
  Vec2d* pos;                   // [B][E] merged position (x_merge_(0..1)) of every track EVER created, by reference index, for the merge phase
  int* slot_of;                 // [B][E] slot of the track with reference index i; -1 once it has been evicted
  TrackTomb* tomb;              // [B][E] lifetime_ / static flag of evicted tracks
  unsigned long long* used;     // [B][(T + 63) / 64] slots in use
  int* zomb;                    // [B][T] slots of the tracks that died in the last step (evicted at the start of the next one)
  int* nzomb;                   // [B]
  int E;                        // capacity of the per-ever-track arrays
  Vec2d* cp;                    // [B][kMaxBoxesPerFrame] box centres of the frame (trackPoints)
  TrackItem* items;             // [B*T] work list of the two per-track kernels, any order
  int* n_items;                 // its length; zero between steps
  mot_track* out;               // [B][T] by slot
  int* flags;                   // [B] capacity flags
  const int* m_dev;             // optional: boxes per frame read from counts[b*kCountsStride + kCntBoxes] (fused path)
  int* owner;                   // [B][kMaxBoxesPerFrame] or null (mot_set_track_links off: nothing is written): reference index of the track that owns box i of
                                // this step's box list — the track that claimed it (the first live one, in index order, whose claim mask holds it), the
                                // track born from it, or -1 (the birth was dropped; first frame: every box but the seeded one). A per-frame output, not state.
  int* owner_n;                 // [B] boxes of the step that wrote the row
  int T;
  int step_mode;                // host only: MOT_TRACKER_AUTO / _SPLIT / _STREAM (mot_set_tracker_mode) — how mot_launch_track launches the step
  MotTrackParams tp;
};
enum { kTrackFlagCapacity = 1 };   // a birth was dropped: no free slot (more than T tracks alive or just dead) or E tracks ever created; or (fused path) the box stage refused a frame of the stream (kFlag*): track_prep_body

void mot_launch_track(const TrackBuffers& t, int batch, hipStream_t stream, bool prep_done = false);
void mot_launch_box_finalize_prep(const MotDevParams& p, const ClusterBuffers& c, const TrackBuffers& tb, int batch, hipStream_t stream);
void mot_launch_export_tracks(const TrackBuffers& t, int batch, mot_track* dst, int max_per_slot, int* dst_counts, hipStream_t stream);
void mot_launch_export_tracks_packed(const TrackBuffers& t, int batch, int* header, mot_track* dst, int capacity, hipStream_t stream);
// the same blocks in the SENSOR frame: tf[k] = the global -> sensor matrix of the k-th stream of the launch (streams first .. first + batch - 1; the packed block always starts at stream 0)
void mot_launch_export_tracks_sensor(const TrackBuffers& t, int first, int batch, const EgoTf* tf, mot_track* dst, int max_per_slot, int* dst_counts, hipStream_t stream);
void mot_launch_export_tracks_packed_sensor(const TrackBuffers& t, int batch, const EgoTf* tf, int* header, mot_track* dst, int capacity, hipStream_t stream);

// ---- per-point track ids (link.hip) ------------------------------------------------------------
// elevated point -> cell -> cluster label -> box -> owning track, for frames 0..batch-1 of a fused call: ids[b * id_stride + i] = the reference index of the track
// that owns the box of point i's cluster, -1 where the point has no cluster, the cluster no box, the box no owner, or the frame was refused for capacity. Points
// at and beyond id_stride are not written; n_out[b] (or null) receives the frame's elevated count. `c` is the frame as the cluster stage left it (input order:
// never the regrouped view), `owner` the tracker's rows ([batch][kMaxBoxesPerFrame]).
constexpr int kLinkChunk = 2048;                  // points per workgroup
void mot_launch_point_tracks(const MotDevParams& p, const ClusterBuffers& c, const int* owner, int batch, int max_n, int* ids, long id_stride, int* n_out, hipStream_t stream);

// ---- per-track point clouds (track_points.hip) ---------------------------------------------------
// The elevated points of frames first .. first + batch - 1, stably partitioned by owning track: the per-point ids above, the input-order cloud and the owner
// rows in; records and segments (include/mot.h: mot_track_point, mot_track_segment) out, into block k = 0 .. batch - 1 of the caller's buffers. Scratch of the
// feature's own: the frame's distinct owners and their boxes, and one row of kTrackPointKeys ints per 1024-point chunk (points per key, then where they go).
constexpr int kTrackPointChunk = 1024;                      // points per workgroup: 16 tiles of 64, four per step
constexpr int kTrackPointKeys = kMaxBoxesPerFrame + 1;      // a frame's distinct owners, and the rest
struct TrackPointBuffers {
  const int* ids;              // [B][cap] track id of every elevated point (link.hip)
  const float4* elevated;      // [B][cap] the elevated cloud in INPUT order (never the regrouped copy)
  int elevated_packed;
  long cap;
  const int* counts;           // [B][kCountsStride]
  const int* owner;            // [B][kMaxBoxesPerFrame] the tracker's owner rows
  int* seg_id;                 // [B][kMaxBoxesPerFrame] the row's distinct ids >= 0, ascending
  int* seg_boxes;              // [B][kMaxBoxesPerFrame] boxes of the row that carry each
  int* seg_n;                  // [B] how many
  int* rows;                   // [B][max_chunks][kTrackPointKeys]
  int max_chunks;              // cap / kTrackPointChunk rounded up
};
// rest != 0: the points without owner form a last segment; tf: null (sensor frame) or the sensor -> global matrix of every frame of the launch ([batch]).
// points / segs / counts_out: block 0 of the launch (point_stride / max_segments records and 2 ints per frame)
void mot_launch_track_points(const TrackPointBuffers& t, int first, int batch, int max_n, int rest, const EgoTf* tf, mot_track_point* points, long point_stride,
                             mot_track_segment* segs, int max_segments, int* counts_out, hipStream_t stream);

// Per-track accumulators (track_accum.hip, mot_set_track_accumulation): one row, one ring of K points and one ring of O observations per TRACK SLOT of a stream —
// the tracker's own bounded set of objects alive at once (TrackBuffers::slot_of, ::out), eviction included. K and O are powers of two (O may be 0).
struct TrackAccumPlan { int row, at; };   // per segment of a step: the row it appends to (-1: none) and the ring position of its first KEPT point
struct TrackAccumBuffers {
  mot_accum_row* rows;         // [B][T]
  mot_accum_point* points;     // [B][T][K]
  mot_accum_obs* obs;          // [B][T][O], null when O == 0
  TrackAccumPlan* plan;        // [B][kMaxBoxesPerFrame] scratch between the two kernels
  const int* slot_of;          // [B][E] TrackBuffers::slot_of
  const mot_track* out;        // [B][T] TrackBuffers::out
  const int* steps;            // [batch] of the launch: every frame's step stamp
  int T, E, K, O;
};
// appends the step of slots first .. first + batch - 1 (t.seg_* and t.rows hold what mot_launch_track_point_counts left); tf: every frame's sensor -> global matrix
void mot_launch_track_accum(const TrackPointBuffers& t, const TrackAccumBuffers& a, int first, int batch, int max_n, const EgoTf* tf, hipStream_t stream);
// rows [first, first + n) of the context's row table back to empty
void mot_launch_track_accum_clear(mot_accum_row* rows, long first, long n, hipStream_t stream);

// The accumulators fed by sequence mode (track_accum_seq.hip, mot_sequence_accumulate_dev): slot k = frame k of ONE stream, every frame appended to stream 0's rows.
struct TrackAccumCapture {     // 40 bytes, per (frame, box of its owner row): what is gone a tracker step later
  int slot;                    // slot_of[owner] right after the frame's step; -1: no owner, or an id / slot out of range
  int track_manage, is_static, lifetime;   // the slot's mot_track record as that step left it: the fields of mot_accum_obs
  float px, py;
  double v, yaw;
};
struct TrackAccumSeqSeg {      // 32 bytes, per (frame, segment)
  int id, row, count, box;     // the segment's id, its row of stream 0 (-1: dropped), its points, a box of the frame that carries the id
  unsigned long long t0;       // sequence number of its first point within the track's incarnation (the row's total before the frame)
  int u, lo;                   // ... of its observation (obs_total before the frame); first point of the segment that the call writes (0x7fffffff: none)
};
struct TrackAccumSeqBuffers {
  TrackAccumCapture* cap;      // [frames][kMaxBoxesPerFrame]
  TrackAccumSeqSeg* seg;       // [frames][kMaxBoxesPerFrame]
  int step0;                   // step stamp of frame 0; frame k gets step0 + k
};
// right behind tracker step `frame` of a sequence: a's slot_of / out are stream 0's, counts / owner the context's tables ([slot]...)
void mot_launch_track_accum_capture(const int* counts, const int* owner, const TrackAccumBuffers& a, TrackAccumCapture* cap, int frame, hipStream_t stream);
// behind the last step and the point-link launch: slots 0 .. frames - 1 appended, in order, to the rows / rings a points at (stream 0's); tf: every frame's matrix
void mot_launch_track_accum_sequence(const TrackPointBuffers& t, const TrackAccumBuffers& a, const TrackAccumSeqBuffers& s, int frames, int max_n, const EgoTf* tf,
                                     hipStream_t stream);

// Object-centred track models (track_models.hip, mot_export_track_models_dev): the accumulators' rings joined with their pose logs. Read-only views of the tables above.
constexpr int kTrackModelTile = 128;   // records a workgroup (one wave) of the transform kernel takes per round
struct TrackModelBuffers {
  const mot_accum_row* rows;       // [B][T]
  const mot_accum_point* points;   // [B][T][K]
  const mot_accum_obs* obs;        // [B][T][O], O > 0
  const int* latest;               // [B] every slot's latest accumulated step (-1: none yet); read with MOT_MODEL_CURRENT only
  int T, K, O;
};
// slots first .. first + batch - 1 into block k = 0 .. batch - 1 of the caller's buffers: the headers (extent 0) and the two counts per slot, then the records and the extents
// (points may be null with point_stride 0: extents only). The second launch reads the headers the first one wrote.
void mot_launch_track_models_plan(const TrackModelBuffers& a, int first, int batch, int flags, mot_track_model* models, int* counts, hipStream_t stream);
void mot_launch_track_models_transform(const TrackModelBuffers& a, int first, int batch, int flags, mot_accum_point* points, long point_stride, mot_track_model* models,
                                       hipStream_t stream);

// Voxel-thinned object models (track_voxels.hip, mot_export_track_model_voxels_dev): the same rows and records, one record per occupied voxel.
struct TrackVoxelArgs { float inv_x, inv_y, inv_z; int min_points; };   // 1.0f / leaf, computed once on the host in fp32
struct TrackVoxelResult {      // 48 bytes, per (stream of the call, row): what the count kernel leaves for the pack kernel
  int n_voxels, n_outside, n_sparse, n_records;
  float min_x, min_y, min_z, max_x, max_y, max_z;   // extent of the raw records, as mot_track_model's
  int reserved[2];
};
// plan: [batch][T] headers mot_launch_track_models_plan wrote for the same slots and flags; res: [batch][T] scratch. The count launches (two kernels) give the
// 64-byte headers and the two counts per slot; the write launch reads those headers back and stores every slot's voxels below voxel_stride.
void mot_launch_track_voxels_count(const TrackModelBuffers& a, int first, int batch, int flags, const TrackVoxelArgs& v, const mot_track_model* plan, TrackVoxelResult* res,
                                   mot_track_voxel_model* models, int* counts, hipStream_t stream);
void mot_launch_track_voxels_write(const TrackModelBuffers& a, int first, int batch, int flags, const TrackVoxelArgs& v, const mot_track_model* plan, mot_model_voxel* voxels,
                                   long voxel_stride, const mot_track_voxel_model* models, hipStream_t stream);

// Rolling static-scene grid (scene_grid.hip, mot_set_scene_grid): per stream a W x W torus of 16-byte cells in the tracker's global frame, W a power of two.
constexpr int kSceneChunk = 2048;          // points per workgroup of the splat kernel
constexpr int kSceneScrollBlocks = 32;     // workgroups per slot of the scroll kernel (a grid-stride loop over the cells that entered)
struct SceneCell { unsigned static_hits, dynamic_hits, zkey; int last_seen; };   // as mot_scene_cell, max_z as (unsigned)mot_float_key(z) ^ 0x80000000 (0: none); empty = 16 zero bytes
struct SceneWindow { int oi, oj, ok, pad; };   // per slot: the origin the cells are laid out for, and whether the latest step's window was valid
struct SceneGridBuffers {
  SceneCell* cells;            // [B][W * W], global cell (gi, gj) at (gj & (W - 1)) * W + (gi & (W - 1))
  mot_scene_header* hdr;       // [B] the latest step's header
  SceneWindow* prev;           // [B]
  int W, log2_W;
  float cell, inv;             // inv = 1.0f / cell, computed once on the host in fp32
};
struct SceneSplatInput {
  const int* ids;              // [B][cap] track id of every elevated point (link.hip)
  const float4* elevated;      // [B][cap] the elevated cloud in INPUT order
  int elevated_packed;
  long cap;
  const int* counts;           // [B][kCountsStride]
  const int* slot_of;          // [B][E] TrackBuffers::slot_of
  const mot_track* out;        // [B][T] TrackBuffers::out
  int T, E;
};
// the step of slots first .. first + batch - 1 (scroll, then splat); tf / steps: [batch] of the launch, every frame's sensor -> global matrix and step stamp
void mot_launch_scene_accumulate(const SceneGridBuffers& g, const SceneSplatInput& in, int first, int batch, int max_n, const EgoTf* tf, const int* steps, hipStream_t stream);
// slots first .. first + batch - 1 unrolled into block k = 0 .. batch - 1 of the caller's buffers (out may be null: headers only; headers may be null)
void mot_launch_scene_export(const SceneGridBuffers& g, int first, int batch, mot_scene_cell* out, long cell_stride, mot_scene_header* headers, hipStream_t stream);
// headers and origins of slots [first, first + n) back to "no step yet" (the cells are the caller's memset)
void mot_launch_scene_reset(const SceneGridBuffers& g, int first, int n, hipStream_t stream);

// The scene grid fed by sequence mode (scene_grid_seq.hip, mot_sequence_products_dev with MOT_SEQ_SCENE): slot k = FRAME k of stream 0, all frames into slot 0's grid.
constexpr int kSceneSeqClearBlocks = 256;  // workgroups of the clear kernel (a grid-stride loop over the cells the drive scrolled out)
struct SceneSeqFrame {         // 32 bytes; entry k + 1 is frame k, entry 0 the window the grid was laid out for before the call (ok unused)
  int oi, oj, ok, pad;         // the frame's window (the window before it when its own is invalid) and whether its own is valid
  int lo_i, hi_i, lo_j, hi_j;  // the intersection of this window and every later one of the call: global cells [lo, hi) per axis, may be empty
};
struct SceneSeqBuffers {
  SceneSeqFrame* win;          // [frames + 1]
  unsigned* is_static;         // [frames][words]: bit id of frame k = track id was flagged static as step k left it (ids of the frame's owner row only)
  int words;                   // (E + 31) / 32
  int step0;                   // step stamp of frame 0; frame k gets step0 + k
};
// right behind tracker step `frame` of a sequence (the frame's words are zero: one memset per call); slot_of / out are stream 0's
void mot_launch_scene_seq_capture(const int* counts, const int* owner, const int* slot_of, const mot_track* out, int T, int E, const SceneSeqBuffers& s, int frame, hipStream_t stream);
// behind the last step and the point-link launch: windows, clear, splat — slots 0 .. frames - 1 into slot 0's grid; in.slot_of / in.out are not read
void mot_launch_scene_sequence(const SceneGridBuffers& g, const SceneSplatInput& in, const SceneSeqBuffers& s, int frames, int max_n, const EgoTf* tf, hipStream_t stream);

// A frame's points judged against the scene grid (scene_judge.hip, mot_export_scene_points_dev): READS the grid. Chunks of kSceneChunk points, as the splat kernel's.
constexpr int kSceneJudgeRow = 2 * MOT_SCENE_CLASSES;   // ints per (slot, chunk): the chunk's points per class, then where its first record of every class goes
struct SceneJudgeBuffers {
  uint8_t* cls;                // [B][cap] class of every elevated point (classify -> scatter: the cell of a point is gathered once per call)
  int* rows;                   // [B][max_chunks][kSceneJudgeRow]
  int max_chunks;              // max_points / kSceneChunk rounded up
  unsigned min_static_hits, trail_num, trail_den;
  int class_mask;
};
// slots first .. first + batch - 1 into block k = 0 .. batch - 1 of the caller's buffers: classify, scan and — with a mask and room for records — scatter. tf: [batch]
// sensor -> global matrices of the launch; global != 0: the records carry global coordinates. points / classes may be null
void mot_launch_scene_judge(const SceneGridBuffers& g, const SceneSplatInput& in, const SceneJudgeBuffers& j, int first, int batch, int max_n, const EgoTf* tf, int global,
                            mot_track_point* points, long point_stride, mot_scene_segment* segments, uint8_t* classes, long class_stride, hipStream_t stream);
// A recorded drive's points judged against the grid it left (scene_judge_seq.hip, mot_export_sequence_scene_points_dev): slots 0 .. frames - 1 = the frames of the
// latest MOT_SEQ_SCENE call against SLOT 0's grid, the records class-major over the drive. bases: [frames][5] ints of scratch (a frame's totals, then its drive-wide
// places); s.is_static: that call's bit rows (s.win / s.step0 are not read); tf: [frames] matrices. count: classify, the scan per frame and the scan over frames — the
// class bytes, j.rows, bases and both tables; scatter (behind count, same j and bases): the records — nothing is launched without a mask or room for records
void mot_launch_scene_judge_seq_count(const SceneGridBuffers& g, const SceneSplatInput& in, const SceneJudgeBuffers& j, const SceneSeqBuffers& s, int* bases, int frames, int max_n,
                                      const EgoTf* tf, mot_scene_segment* segments, mot_scene_segment* totals, uint8_t* classes, long class_stride, hipStream_t stream);
void mot_launch_scene_judge_seq_scatter(const SceneSplatInput& in, const SceneJudgeBuffers& j, const int* bases, int frames, int max_n, const EgoTf* tf, int global,
                                        mot_track_point* points, long capacity, hipStream_t stream);

// Voxel-thinned static map of a recorded drive (scene_voxels_seq.hip, mot_export_sequence_scene_voxels_dev): behind mot_launch_scene_judge_seq_count with the same j and
// bases and `tab` as its two tables. The selected records of the drive, in the order of mot_launch_scene_judge_seq_scatter (global frame), are keyed by cell, sorted
// (mot_sort.h), cut into runs and reduced to one centroid and one count per kept voxel. All of it is library scratch, sized by `cap` records (the call's
// record_capacity, at least 1 of room): see mot_scene_voxel_scratch_bytes.
constexpr int kSceneVoxelKeyBits = 56;     // bits of a key that decide the order: 54 of the cell, and two of the all-ones key of a record outside the lattice
constexpr int kSceneVoxelPlan = 8;         // ints: n_records, records in play, runs, n_outside, n_voxels
struct SceneVoxelArgs { float inv_x, inv_y, inv_z; int min_points; };   // 1.0f / leaf, computed once on the host in fp32
struct SceneVoxelBuffers {
  unsigned long long* key[2];  // [cap] each: the keys at their record position / ping-pong of the sort; the buffer the sort leaves free holds the run table
  unsigned* val[2];            // [cap] each: the record position a key came from
  float4* staged;              // [cap] the records at their record position
  int* table;                  // [256][tiles] the sort's digit table
  int* totals;                 // [256]
  int* part;                   // [3][tiles] per tile: run heads, records outside the lattice, kept runs (the voxel merge adds a fourth row: saturated runs)
  int* plan;                   // [kSceneVoxelPlan]
  const mot_scene_segment* tab;// [frames][5] segments, then [5] totals: what the count launches wrote
  int cap, tiles;              // tiles = ceil(cap / 2048), at least 1
};
inline size_t mot_scene_voxel_scratch_bytes(long cap, int batch, SceneVoxelBuffers* at = nullptr, char* base = nullptr) {
  const size_t n = (size_t)((cap < 1 ? 1 : cap) + 3) & ~(size_t)3;   // (every block starts 16-byte aligned)
  const size_t tiles = (n + 2047) / 2048;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 15) & ~(size_t)15; return at; };
  const size_t k0 = take(8 * n), k1 = take(8 * n), st = take(16 * n), v0 = take(4 * n), v1 = take(4 * n);
  const size_t tb = take(4 * 256 * tiles), tt = take(4 * 256), pt = take(4 * 3 * tiles), pl = take(4 * kSceneVoxelPlan);
  const size_t sg = take(sizeof(mot_scene_segment) * MOT_SCENE_CLASSES * ((size_t)batch + 1));
  if (at && base) {
    at->key[0] = reinterpret_cast<unsigned long long*>(base + k0); at->key[1] = reinterpret_cast<unsigned long long*>(base + k1); at->staged = reinterpret_cast<float4*>(base + st);
    at->val[0] = reinterpret_cast<unsigned*>(base + v0); at->val[1] = reinterpret_cast<unsigned*>(base + v1); at->table = reinterpret_cast<int*>(base + tb);
    at->totals = reinterpret_cast<int*>(base + tt); at->part = reinterpret_cast<int*>(base + pt); at->plan = reinterpret_cast<int*>(base + pl);
    at->tab = reinterpret_cast<const mot_scene_segment*>(base + sg);
  }
  return o;
}
// keys, the sort, runs, kept voxels and the header (d_totals may be null); then — with room for voxels — one wave per run writes the centroids. The write launch
// reads what the count launches left in the scratch: it may follow them later on the same stream (the getter sizes its block in between)
void mot_launch_scene_voxels_seq_count(const SceneSplatInput& in, const SceneJudgeBuffers& j, const int* bases, int frames, int max_n, const EgoTf* tf, const SceneVoxelBuffers& v,
                                       const SceneVoxelArgs& a, long voxel_capacity, mot_scene_voxel_header* header, mot_scene_segment* totals, hipStream_t stream);
void mot_launch_scene_voxels_seq_write(const SceneVoxelBuffers& v, mot_model_voxel* voxels, long voxel_capacity, hipStream_t stream);

// Voxel maps merged into one (voxel_merge.hip, mot_merge_voxel_maps_dev): the maps' voxels, read in place, are keyed by the cell of their centroid (sv_key,
// mot_voxel_runs.h), sorted (mot_sort.h), cut into runs and reduced to one record per kept cell. The scratch is a SceneVoxelBuffers without staged records and
// without the judge's tables, sized by `cap` = the sum of the maps' capacities (at least 1 of room): see mot_voxel_merge_scratch_bytes.
constexpr int kVoxelMergeMaps = 16;
constexpr int kVmPrefix = 8;               // plan[kVmPrefix + k]: the inputs of the maps before k (k = 0 .. 16); the ints below are those of the drive voxel call
constexpr int kVoxelMergePlan = 32;        // ints
struct VoxelMergeMaps {
  const mot_model_voxel* vox[kVoxelMergeMaps];   // device blocks, 16-byte aligned
  const int* count[kVoxelMergeMaps];             // on the device; null: the capacity is the count
  int cap[kVoxelMergeMaps];
  int n_maps;
  int short_max;                                 // runs of at most so many inputs are summed by one thread, the longer ones by a wave; [0, 64]: the bytes do not depend on it
};
inline size_t mot_voxel_merge_scratch_bytes(long cap, SceneVoxelBuffers* at = nullptr, char* base = nullptr) {
  const size_t n = (size_t)((cap < 1 ? 1 : cap) + 3) & ~(size_t)3;   // (every block starts 16-byte aligned)
  const size_t tiles = (n + 2047) / 2048;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 15) & ~(size_t)15; return at; };
  const size_t k0 = take(8 * n), k1 = take(8 * n), v0 = take(4 * n), v1 = take(4 * n);
  const size_t tb = take(4 * 256 * tiles), tt = take(4 * 256), pt = take(4 * 4 * tiles), pl = take(4 * kVoxelMergePlan);
  if (at && base) {
    at->key[0] = reinterpret_cast<unsigned long long*>(base + k0); at->key[1] = reinterpret_cast<unsigned long long*>(base + k1); at->staged = nullptr;
    at->val[0] = reinterpret_cast<unsigned*>(base + v0); at->val[1] = reinterpret_cast<unsigned*>(base + v1); at->table = reinterpret_cast<int*>(base + tb);
    at->totals = reinterpret_cast<int*>(base + tt); at->part = reinterpret_cast<int*>(base + pt); at->plan = reinterpret_cast<int*>(base + pl);
    at->tab = nullptr;
  }
  return o;
}
// count: keys, the sort, runs, the runs' summed counts, kept voxels and the header; write (behind count on the same stream, the same maps and buffers; nothing without
// room for voxels): the kept voxels. part is [4][tiles] here: run heads, inputs outside the lattice, kept runs, saturated runs
void mot_launch_voxel_merge_count(const VoxelMergeMaps& m, const SceneVoxelBuffers& v, const SceneVoxelArgs& a, long out_capacity, mot_voxel_merge_header* header, hipStream_t stream);
void mot_launch_voxel_merge_write(const VoxelMergeMaps& m, const SceneVoxelBuffers& v, int min_points, mot_model_voxel* out, long out_capacity, hipStream_t stream);

// the same count pipeline, then — with room in the index — ONE write launch: per kept run below the capacity the run's key itself (the sorted key at the run's
// start) and its saturated summed count (mot_index_voxel_maps_dev). Behind mot_launch_voxel_merge_count on the same stream, the same maps and buffers
void mot_launch_voxel_merge_index(const VoxelMergeMaps& m, const SceneVoxelBuffers& v, unsigned long long* keys, int* counts, long capacity, hipStream_t stream);

// A frame's points judged against a voxel index (map_judge.hip, mot_export_map_points_dev): READS the index mot_index_voxel_maps_dev wrote — `capacity` ascending
// keys and their counts, the length in play an int32 ON THE DEVICE, clamped there. The chunk rows and the class bytes are a SceneJudgeBuffers of the feature's own
// (its three grid thresholds unused): the scan and the scatter are the scene judge's bodies (mot_scene_judge.h).
struct MapJudgeIndex {
  const unsigned long long* keys;   // [capacity], strictly ascending below n
  const int* counts;                // [capacity]
  const int* n_stored;              // on the device: the index's length, clamped to [0, capacity] by every reader
  int capacity;
  SceneVoxelArgs a;                 // 1.0f / leaf of the index, computed once on the host (min_points unused)
  int min_count, reach;             // a cell counts from min_count on; reach 0: the point's own cell, 1: its 27 neighbours
};
// slots first .. first + batch - 1 into block k = 0 .. batch - 1 of the caller's buffers: classify, scan and — with a mask and room for records — scatter
void mot_launch_map_judge(const SceneSplatInput& in, const SceneJudgeBuffers& j, const MapJudgeIndex& x, int first, int batch, int max_n, const EgoTf* tf, int global,
                          mot_track_point* points, long point_stride, mot_scene_segment* segments, uint8_t* classes, long class_stride, hipStream_t stream);

#include "mot_wave_sync.h"   // MOT_WAVE_SYNC (shared with mot_wave.h)

void mot_launch_ground(const MotDevParams& p, const GroundBuffers& g, int batch, int max_n, hipStream_t stream);
void mot_launch_noop(int batch, hipStream_t stream);   // measurement only: an empty one-workgroup-per-frame launch (mot_debug_skip_kernels)
void mot_launch_expand_xyz12(const float* in, long in_stride_floats, float4* out, long out_stride, int batch, int max_n, hipStream_t stream);
void mot_launch_decode_pointcloud2_batch(const void* data, long raw_stride, int batch, int max_n, int step, int ox, int oy, int oz, int ow, float4* out, long out_stride, hipStream_t stream);
void mot_launch_decode_pointcloud2(const void* data, int n, int step, int ox, int oy, int oz, int ow, float4* out, hipStream_t stream);
// single kernels, for per-kernel timing (mot_time_stage): which = 0 min-z, 1 polar filter, 2 classify+compact
void mot_launch_ground_kernel(int which, const MotDevParams& p, const GroundBuffers& g, int batch, int max_n,
                              hipStream_t stream);

// ordered-int key of a float: signed integer compare == float compare
// slot of a cluster in a label-kernel workgroup's 64-entry table (linear probing from here)
MOT_HD int mot_stats_count(const ClusterStats& s) { return (int)(unsigned)s.count_groups; }
MOT_HD int mot_stats_groups(const ClusterStats& s) { return (int)(s.count_groups >> 32); }
MOT_HD unsigned mot_label_hash(int label) { return ((unsigned)label * 0x9E3779B1u) >> 26; }
MOT_HD int mot_float_key(float f) { int k = mot_f2i(f); return k >= 0 ? k : k ^ 0x7fffffff; }
MOT_HD float mot_key_float(int k) { return mot_i2f(k >= 0 ? k : k ^ 0x7fffffff); }

// Cartesian cell of a point: component_clustering.cpp:42-48 (same expression at :318-324 and
// box_fitting.cpp:52-58). fp32: int*float, then /float, floor. Returns false outside the ROI.
MOT_HD bool mot_cart_cell(const MotDevParams& p, float x, float y, int* xI, int* yI) {
  float xC = x + p.roi_half;
  float yC = y + p.roi_half;
  if (xC < 0 || xC >= p.roi_m || yC < 0 || yC >= p.roi_m) return false;
  float fx = floorf(p.num_grid * xC / p.roi_m), fy = floorf(p.num_grid * yC / p.roi_m);
  // NaN slips through the ROI test in the reference and indexes out of bounds (UB); dropped here
  if (!(fx >= 0.f && fx < (float)p.num_grid && fy >= 0.f && fy < (float)p.num_grid)) return false;
  *xI = (int)fx; *yI = (int)fy;
  return true;
}

// Guarded fast path of mot_cart_cell for the streaming kernels: bit index xI * 256 + yI of the cell, -1 outside the ROI,
// -2 undecided (call mot_cart_cell). The exact index is floor(fl(fl(G * xC) / roiM)); the estimate xC * fl(G / roiM)
// differs from that quotient by at most 4 roundings of a value below 256 (< 6.2e-5), so whenever the estimate is farther
// than kCartGuard from an integer both floors agree. NaN fails every guard compare and lands in the exact path, which
// drops it. tests/test_math_exact.py::test_fast_cart_cell_agrees checks the claim.
// The admitted parameters keep this true: with V = G * xC / roiM < G <= 256 (mot_create: num_grid <= MOT_MAX_GRID), u = 2^-24,
// the exact quotient carries the roundings of G * xC and of the divide, the estimate those of k_grid and of its multiply, each
// at most u * V relative to the real V: |estimate - quotient| <= 4 u V (1 + 2u) < 6.2e-5 = kCartGuard / 4, whatever roiM is. roiM
// enters only through over- and underflow: for MOT_ROI_M_MIN <= roiM <= MOT_ROI_M_MAX (1e-3 .. 1e6, mot_create) k_grid lies in
// 8e-6 .. 2.6e5 and G * xC below 2.6e8, all normal numbers; a denormal xC gives V < 1e-30, far below the guard.
constexpr float kCartGuard = 2.5e-4f;
MOT_HD int mot_cart_bit_try(const MotDevParams& p, float x, float y) {
  const float xC = x + p.roi_half, yC = y + p.roi_half;
  const bool outside = xC < 0 || xC >= p.roi_m || yC < 0 || yC >= p.roi_m;
  const float tx = xC * p.k_grid, ty = yC * p.k_grid;
  const float fx = floorf(tx), fy = floorf(ty);
  const float rx = tx - fx, ry = ty - fy;
  const bool safe = rx > kCartGuard && rx < 1.f - kCartGuard && ry > kCartGuard && ry < 1.f - kCartGuard;   // false on NaN
  const int bit = (int)((unsigned)(int)fx * (unsigned)MOT_MAX_GRID + (unsigned)(int)fy);   // (unsigned: a point far outside wraps, and is discarded)
  return outside ? -1 : (safe ? bit : -2);
}
MOT_HD int mot_cart_bit(const MotDevParams& p, float x, float y) {
  int bit = mot_cart_bit_try(p, x, y);
  if (bit == -2) { int xI, yI; bit = mot_cart_cell(p, x, y, &xI, &yI) ? xI * MOT_MAX_GRID + yI : -1; }
  return bit;
}

// getClusteredPoints' label of elevated point i of slot b (box_fitting.cpp:46-72): its cell — the 2 bytes the compaction kernel left (fused path) or
// the guarded cell computation — then the label grid; a value that names no cluster of the frame reads as 0
MOT_HD int mot_point_label(const MotDevParams& p, const ClusterBuffers& c, int b, long i, int num_cluster) {
  int cell;
  if (c.ecell) {
    const unsigned e = c.ecell[(long)b * c.cap + i];
    cell = e != 0xffffu ? (int)((e >> 8) * (unsigned)p.num_grid + (e & 255u)) : -1;
  } else {
    const float4 q = mot_load_xyz(c.elevated + (long)b * c.cap, i, c.elevated_packed);
    const int bit = mot_cart_bit(p, q.x, q.y);
    cell = bit >= 0 ? (bit >> 8) * p.num_grid + (bit & 255) : -1;
  }
  int lab = cell >= 0 ? (int)c.grid[(long)b * (MOT_MAX_GRID * MOT_MAX_GRID) + cell] : 0;
  if (lab < 0 || lab > num_cluster) lab = 0;
  return lab;
}

// getCellIndexFromPoints (ground_removal.cpp:67-76) + filterCloud's range test (:53) + the callers'
// bounds test (:89,:233), evaluated exactly as the reference does (correctly rounded sqrtf, bit-exact atan2f, fp64
// intermediate, IEEE divide). Returns the polar cell (ch*120+bin) or -1 when the point takes no part.
MOT_HD int mot_polar_cell_exact(const MotDevParams& p, float x, float y) {
  float distance = sqrtf(x * x + y * y);
  if (distance <= p.r_min || distance >= p.r_max) return -1;       // filterCloud (NaN passes, as in the reference)
  float at = mot_atan2f(y, x);
  float chP = (float)(((double)at + 3.14159265358979323846) / (2 * 3.14159265358979323846));
  float binP = (distance - p.r_min) / p.r_span;
  float fc = floorf(chP * MOT_NUM_CHANNEL);
  float fb = floorf(binP * MOT_NUM_BIN);
  // (int) of NaN / out-of-range is INT_MIN on the reference's x86 build and is then dropped
  if (!(fc >= 0.f && fc < (float)MOT_NUM_CHANNEL && fb >= 0.f && fb < (float)MOT_NUM_BIN)) return -1;
  return (int)fc * MOT_NUM_BIN + (int)fb;
}

// Guarded fast path. The cell is floor() of two quantities; floor only depends on them to within the distance to the
// nearest integer. Both are first estimated cheaply: the hardware's 1-ulp square root and one multiply instead of the
// correctly rounded sqrtf and the IEEE divide for the bin (error < 5.8e-5 bins at the presets, derived below); a degree-13 odd polynomial for atan on
// [0,1] with a hardware reciprocal for the channel (absolute error < 1e-6 rad => < 2e-5 channels). If either estimate is
// within kCellGuard of an integer — or anything is NaN/Inf — the answer is -2 and the exact evaluation decides;
// otherwise the estimate's floor IS the exact floor, and the range filter rMin < d < rMax is the test 0 <= bin < 120
// (a distance within an ulp of either limit lands inside the guard). ~4e-4 of the points need the exact path.
// tests/test_math_exact.py::test_fast_cell_agrees checks the claim on 2e8 points (square root and reciprocal perturbed by
// +-1 ulp to cover v_sqrt_f32 / v_rcp_f32), the -m gpu parity tests check it end to end.
//
// The bin's error, and the polar ranges for which the guard is enough (mot_create refuses every other one: make_dev_params,
// MOT_POLAR_RATIO_MAX in mot.h). Notation: u = 2^-24, K = MOT_NUM_BIN = 120, s = r_span = fl(rMax - rMin), d = sqrtf(x*x + y*y)
// correctly rounded, d' the hardware's root of the same argument (within 1 ulp of the real root, so d' is d or a neighbour of d:
// |d' - d| <= ulp(d) <= 2 u d), T = (d - rMin) K / s in real arithmetic, rho = rMax / s.
//   exact     E  = fl(fl(fl(d - rMin) / s) * K)           = T (1 + e1)(1 + e2)(1 + e3),                    |e_i| <= u
//   estimate  tb = fl(fl(d' - rMin) * k_bin), k_bin = fl(K / s)  = ((d' - rMin) K / s)(1 + e4)(1 + e5)(1 + e6)
//   |tb - E| <= |d' - d| K / s + 6 u T (1 + 3u)  <=  2 u K d / s + 6 u T (1 + 3u)
// Only T in [0, K + 1] matters (beyond it both sides are far from 0 .. K and answer "outside"), where d / s <= rho + 1 / K and
// T <= K + 1. For rho >= 2 the range starts at rMin >= rMax / 2, so both subtractions are exact (Sterbenz) and two of the six
// rounding terms vanish:
//   rho <  2:  |tb - E| < u K (2 rho + 6) (1 + 1/K)  <  10 u K (1 + 1/K) = 7.2e-5
//   rho <= 4:  |tb - E| < u K (2 rho + 4) (1 + 1/K) <=  12 u K (1 + 1/K) = 8.7e-5        (u K = 7.153e-6)
// i.e. below kCellGuard = 1e-4 with a margin of 1.15 for rMax / (rMax - rMin) <= 4 — the declared domain — and the presets
// (rho = 1.03) have 5.8e-5. When the estimate's fraction lies in (kCellGuard, 1 - kCellGuard), E therefore has the same floor.
// The range filter follows from the same bound: tb > kCellGuard means (d' - rMin) K / s > 2 u K d / s (1 + 3u), so d' - rMin >
// ulp(d) and d > rMin; tb < K - kCellGuard means d' < rMax - s (kCellGuard / K - 4u) < rMax - ulp(d), so d < rMax; tb beyond
// either end by more than the guard puts E beyond it as well, and the exact evaluation answers -1 there too.
// The sqrt term is attained (a neighbour of d IS what the hardware may return), the rounding terms seldom all at once: ranges with
// 4 < rho < ~7 are refused because they are unproven, not because a wrong answer is known; from 2^-23 * 2^floor(log2 rMax) * K / s >
// kCellGuard + 4 u K on (rho = 9.3 at rMax = 65) a wrong answer exists whatever the roundings do — the negative control of
// tests/test_math_exact.py. rMax itself: MOT_R_MAX_MIN .. MOT_R_MAX_MAX (1e-3 .. 1e6 m) keeps x*x + y*y, s and k_bin normal
// numbers for every d near the range, which the relative-error model above assumes.
constexpr float kCellGuard = 1.0e-4f;
MOT_HD int mot_polar_cell_fast(const MotDevParams& p, float x, float y, float distance_approx, float rcp_mx) {
  // bin
  const float tb = (distance_approx - p.r_min) * p.k_bin;
  const float fb = floorf(tb), rb = tb - fb;
  const bool bin_safe = rb > kCellGuard && rb < 1.f - kCellGuard;  // false on NaN
  const bool bin_in = fb >= 0.f && fb < (float)MOT_NUM_BIN;
  // channel: atan2 by octant reduction
  const float ax = fabsf(x), ay = fabsf(y);
  const float mn = ax < ay ? ax : ay;
  const float q = mn * rcp_mx;
  const float s = q * q;
  // an estimate: fused multiply-adds are welcome here (the build has -ffp-contract=off for everything that must round
  // as the reference does)
  float a = 0.006658289581537247f;
  a = __builtin_fmaf(a, s, -0.03310525044798851f);
  a = __builtin_fmaf(a, s, 0.0789998322725296f);
  a = __builtin_fmaf(a, s, -0.13195902109146118f);
  a = __builtin_fmaf(a, s, 0.19796891510486603f);
  a = __builtin_fmaf(a, s, -0.33316001296043396f);
  a = __builtin_fmaf(a, s, 0.9999956488609314f);
  a = a * q;
  a = ay > ax ? 1.57079632679489662f - a : a;
  a = x < 0.f ? 3.14159265358979324f - a : a;
  a = y < 0.f ? -a : a;
  const float tc = __builtin_fmaf(a, MOT_NUM_CHANNEL / 6.28318530717958648f, MOT_NUM_CHANNEL / 2.0f);
  const float fc = floorf(tc), rc = tc - fc;
  const bool ch_safe = rc > kCellGuard && rc < 1.f - kCellGuard;  // false on NaN
  const bool ch_in = fc >= 0.f && fc < (float)MOT_NUM_CHANNEL;
  // straight-line selects, no branches: clearly outside rMin..rMax needs no channel; otherwise both estimates must be safe
  const int idx = (int)fc * MOT_NUM_BIN + (int)fb;
  int cell = (bin_safe && ch_safe) ? (ch_in ? idx : -1) : -2;
  cell = (bin_safe && !bin_in) ? -1 : cell;
  return cell;
}

// ---- the BIN alone. Round 5's compaction kernel read one byte per point (the polar channel) and recomputed the bin from x, y with these; since
// it decides from the cell and the group's max z whether to load a point AT ALL (ground.hip), the whole 2-byte cell travels again and no kernel
// calls them. Kept for the device sweeps of the guard with the channel switched off (tests/devcheck/sweep.hip what = 2, primitives.hip).
MOT_HD int mot_polar_bin_exact(const MotDevParams& p, float x, float y) {   // the bin of mot_polar_cell_exact (same expressions), -1: outside rMin..rMax
  float distance = sqrtf(x * x + y * y);
  if (distance <= p.r_min || distance >= p.r_max) return -1;
  float binP = (distance - p.r_min) / p.r_span;
  float fb = floorf(binP * MOT_NUM_BIN);
  if (!(fb >= 0.f && fb < (float)MOT_NUM_BIN)) return -1;
  return (int)fb;
}
MOT_HD int mot_polar_bin_fast(const MotDevParams& p, float distance_approx) {   // the bin part of mot_polar_cell_fast: bin, -1 (outside), -2 (undecided)
  const float tb = (distance_approx - p.r_min) * p.k_bin;
  const float fb = floorf(tb), rb = tb - fb;
  const bool bin_safe = rb > kCellGuard && rb < 1.f - kCellGuard;  // false on NaN
  const bool bin_in = fb >= 0.f && fb < (float)MOT_NUM_BIN;
  return bin_safe ? (bin_in ? (int)fb : -1) : -2;
}
MOT_HD int mot_polar_bin_try(const MotDevParams& p, float x, float y) {
  const float d2 = x * x + y * y;
#if defined(__HIP_DEVICE_COMPILE__) && !defined(MOT_HIPEMU)
  return mot_polar_bin_fast(p, __builtin_amdgcn_sqrtf(d2));
#else
  return mot_polar_bin_fast(p, sqrtf(d2));
#endif
}

// the fast path with the hardware estimates; -2 = undecided (call mot_polar_cell_exact)
MOT_HD int mot_polar_cell_try(const MotDevParams& p, float x, float y) {
  const float ax = fabsf(x), ay = fabsf(y);
  const float d2 = x * x + y * y, mx = ax > ay ? ax : ay;
#if defined(__HIP_DEVICE_COMPILE__) && !defined(MOT_HIPEMU)
  return mot_polar_cell_fast(p, x, y, __builtin_amdgcn_sqrtf(d2), __builtin_amdgcn_rcpf(mx));
#else
  return mot_polar_cell_fast(p, x, y, sqrtf(d2), 1.0f / mx);
#endif
}

MOT_HD int mot_polar_cell(const MotDevParams& p, float x, float y) {
  int cell = mot_polar_cell_try(p, x, y);
  if (cell == -2) cell = mot_polar_cell_exact(p, x, y);
  return cell;
}

// node pre-filter, OT/src/groundremove/main.cpp:56-81,104-112: PassThrough z (closed, finite) then
// ConditionalRemoval x,y (strict)
MOT_HD bool mot_crop_keep(const MotDevParams& p, float x, float y, float z) {
  if (!p.crop_enable) return true;
  if (!(x - x == 0.f) || !(y - y == 0.f) || !(z - z == 0.f)) return false;  // non-finite
  if (z < p.crop_z_min || z > p.crop_z_max) return false;
  return x > p.crop_x_min && x < p.crop_x_max && y > p.crop_y_min && y < p.crop_y_max;
}

#endif  // MOT_INTERNAL_H_
