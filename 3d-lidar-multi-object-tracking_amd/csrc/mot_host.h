// mot_host.h — what the host-only translation units of the C-ABI share (mot_api.hip: life cycle, setters, launch sequence, ingest; mot_api_stages.hip: stage-wise calls and
// getters; mot_api_tracks.hip: tracker, exports, snapshots; mot_api_scene.hip: the scene grid; mot_gather.hip: the RCCL gather): the context, the record of slot residency, the ONE owner of every device /
// page-locked allocation, event and captured graph of a context ("ownership", below), and the ONE owner of each view of the elevated cloud and of each step around a
// launch that the track and scene calls share (at the end). No kernel includes this.
#ifndef MOT_HOST_H_
#define MOT_HOST_H_
#include "mot_internal.h"
#include "mot_debug_api.h"

#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

// ---------------------------------------------------------------------------------------- what each slot holds
// The one record of slot residency, and the only code that writes it: per slot the four facts of SlotState, per context the input description of the last batch
// ("its compaction can be re-run"). What include/mot.h promises of mot_get_ground, mot_box_markers and mot_get_clusters is this table; tests/test_emu_slot_residency.py walks it.
//   transition (callers)                                                          slots       packed       labels                        boxes  ground                        last_fused
//   fused_batch (mot_frames_*, mot_sequence_dev)                                   0..batch-1  !OUT_GROUND  OUT_LABELS ? Ready : FromCells  yes    GROUND & MASK ? Resident : None  yes
//   ground_stage (mot_ground_remove*, mot_ground_node_frame)                       0           no           FromPoints                    no     mask ? Resident : None        no
//   slot0_taken (mot_cluster, _box_fit, _cluster_products_host, _cluster_node_frame)  0        no           FromPoints                    no     Foreign                       no
//   labels_written (mot_get_clusters on demand, mot_cluster with labels)           one         -            Ready                         -      -                             -
//   box_stage (mot_box_fit, _box_fit_resident, _cluster_node_frame once it fit)    one         -            Ready                         yes    -                             -
//   every transition above also moves `links` (mot_set_track_links): fused_batch with the tracker and links on -> Points (box stage and tracker step of ONE fused call: the owner
//   row and the per-point ids belong to the slot's cloud); every other transition that gives the slot a new cloud or new boxes (fused_batch without the tracker, ground_stage,
//   slot0_taken) takes Points back to Boxes: the owner row still is the last tracker step's, the point chain is broken
//   tracker_fed (mot_track_step, _track_steps_dev, _tracking_node_frame: boxes from outside)  the slots stepped   links on ? Boxes : as before
//   links_switched (mot_set_track_links)                                           all         links -> None (no step since)
//   (fused_batch and box_stage also record `regrouped`: whether the box stage ran on the cluster-ordered copy, MOT_ORDER_ANY; every transition that clears `boxes` clears it)
//   sequence_accumulated (mot_sequence_accumulate_dev, behind its fused_batch)      0..frames-1 `accumulated`: the frames are in stream 0's accumulators; they stay `sequence` slots
//   sequence_scene_taken (mot_sequence_products_dev(MOT_SEQ_SCENE), behind its fused_batch)  0..frames-1 `scene`, and scene_drive = frames: the drive can be judged until ANY
//                                                                                 transition above but labels_written / compaction_rerun, a scene restart or mot_accumulate_scene
//   compaction_rerun (mot_get_ground on demand, mot_time_stage)                    0..batch-1  as run       -                             -      as run, unless Foreign        -
//   describe_batch (set_batch): the last_* input description. Nothing is vouched for in a slot at or beyond last_batch that needs the batch's input.
// per-point labels: not computed, the cloud was uploaded by a stage-wise call (no cell codes: mot_get_clusters computes them from the points) / not computed, cloud and cell
// codes come from the fused compaction kernel (... from the cells) / in d_label
enum LabelState : char { kLabelsFromPoints, kLabelsFromCells, kLabelsReady };
// d_ground / d_mask of the slot: not (both) resident, a fused batch's can be rebuilt (can_rebuild_ground) / hold the ground cloud and the mask that go with the slot's elevated cloud /
// belong to ANOTHER cloud: a stage-wise cluster / box call has put its own elevated cloud into the slot since the ground stage ran
enum GroundState : char { kGroundNone, kGroundResident, kGroundForeign };
// mot_set_track_links: no tracker step wrote the slot's owner row since the links were turned on / the row is the slot's last tracker step's (mot_get_box_tracks) / and that step
// was fed by the box stage of the same fused call, whose cloud, cells, label grid and boxes are the slot's: the per-point ids are valid too (mot_get_point_tracks)
enum LinkState : char { kLinksNone, kLinksBoxes, kLinksPoints };
struct SlotState {
  bool packed = false;                    // the elevated cloud is 12-byte points (the elevated-only compaction: mot_internal.h PackedXyz), not float4 records
  LabelState labels = kLabelsFromPoints;
  bool boxes = false;                     // the box stage's products (boxes, cluster order, groups) belong to the cloud now resident in the slot
  GroundState ground = kGroundNone;
  bool regrouped = false;                 // the box stage ran in MOT_ORDER_ANY: its products (groups, cluster order, first / extreme point indices) index the slot's
                                          // cluster-ordered COPY of the cloud, not the cloud itself. Meaningful while `boxes`; every reader that walks clusters asks.
  LinkState links = kLinksNone;
  bool sequence = false;                  // the slot holds FRAME k of one stream (mot_sequence_dev, mot_sequence_accumulate_dev, mot_sequence_products_dev), not
                                          // stream k's frame: mot_accumulate_track_points and mot_accumulate_scene refuse it
  bool accumulated = false;               // mot_accumulate_track_points has appended the step the slot holds (or a reset / load has put it out of reach): not again
  bool scene = false;                     // the same for mot_accumulate_scene and the slot's scene grid (every transition that gives the slot a new step starts it over)
  bool scene_restarted = false;           // the slot's grid was emptied (the setter, a reset, a load) since the step the slot holds: mot_export_scene_points_dev refuses it too
};
struct Residency {
  std::vector<SlotState> slots;
  bool last_fused = false;                // the last ground launch was a fused one (input, cells and thresholds of the batch still resident)
  int last_batch = 0, last_max_n = 0;     // the last ground launch's geometry and input: what a re-run of its compaction needs
  const float4* last_in = nullptr; long last_in_stride = 0;
  // frames of the latest mot_sequence_products_dev(MOT_SEQ_SCENE) call while slots 0 .. scene_drive - 1 still hold them and slot 0's grid is as that call left it
  // (mot_export_sequence_scene_points_dev judges exactly that); 0: no such call, or a slot was taken / stream 0's grid was emptied or changed since
  int scene_drive = 0;
  void reset(int batch) { slots.assign(batch, SlotState()); scene_drive = 0; }
  void describe_batch(int batch, int max_n, const float4* in, long stride) { last_batch = batch; last_max_n = max_n; last_in = in; last_in_stride = stride; }
  static bool fused_packs(int outputs) { return MOT_PACKED_ELEVATED && !(outputs & MOT_OUT_GROUND); }   // the elevated-only compaction leaves 12-byte points
  static bool fused_keeps_ground(int outputs) { return (outputs & (MOT_OUT_GROUND | MOT_OUT_MASK)) == (MOT_OUT_GROUND | MOT_OUT_MASK); }
  // a fused call over slots 0..batch-1 was issued: what those slots hold from now on (the slots beyond keep what an earlier, larger batch left). Host
  // state, so it also holds when a captured graph is replayed: every reader built from cluster_buffers afterwards is told the layout
  // linked: the call runs the tracker with mot_set_track_links on
  // one_stream: mot_sequence_dev. Every fused call gives the slot a new step: `accumulated` starts over
  void fused_batch(int batch, int outputs, bool regrouped, bool linked, bool one_stream = false) {
    last_fused = true; scene_drive = 0;
    for (int b = 0; b < batch; b++)
      slots[b] = {fused_packs(outputs), (outputs & MOT_OUT_LABELS) ? kLabelsReady : kLabelsFromCells, true, fused_keeps_ground(outputs) ? kGroundResident : kGroundNone, regrouped,
                  linked ? kLinksPoints : unlinked(slots[b].links), one_stream, false};
  }
  static LinkState unlinked(LinkState l) { return l == kLinksPoints ? kLinksBoxes : l; }   // the slot's cloud or boxes are being replaced: its owner row stays the last tracker step's
  // a stage-wise ground stage ran on slot 0 (float4 records); without a mask a later mot_get_ground that asks for one answers MOT_E_STATE
  void ground_stage(bool with_mask) { last_fused = false; scene_drive = 0; slots[0] = {false, kLabelsFromPoints, false, with_mask ? kGroundResident : kGroundNone, false, unlinked(slots[0].links)}; }
  // slot 0 now holds a stage-wise cluster / box call's cloud, as float4 records: mot_get_ground must not re-run a fused batch's compaction over it, slot 0's ground cloud / mask (if any) are another
  // cloud's (mot_get_ground(0) answers MOT_E_STATE, as include/mot.h promises), what an earlier label kernel or box stage left is stale (mot_box_markers: MOT_E_STATE). The caller then states what it produced.
  void slot0_taken() { last_fused = false; scene_drive = 0; slots[0] = {false, kLabelsFromPoints, false, kGroundForeign, false, unlinked(slots[0].links)}; }
  // the label kernel ran on the slot's cloud; written = false: in the fused geometry without per-point labels (mot_time_stage)
  void labels_written(int slot, bool written = true) { slots[slot].labels = written ? kLabelsReady : kLabelsFromCells; }
  // the box stage (label kernel included) ran on the slot's cloud: mot_box_markers / mot_get_boxes / mot_get_clusters may read its products
  void box_stage(int slot, bool regrouped) { scene_drive = 0; slots[slot].labels = kLabelsReady; slots[slot].boxes = true; slots[slot].regrouped = regrouped; }
  // the compaction of the last batch was run again: same points in the same order (what the later stages hold stays valid), in the layout and with the outputs
  // of this run. (A slot a stage-wise call has taken since stays refused: only mot_time_stage gets here in that state.)
  void compaction_rerun(int batch, bool packed, bool ground_and_mask) {
    for (int b = 0; b < batch; b++) { slots[b].packed = packed; if (slots[b].ground != kGroundForeign) slots[b].ground = ground_and_mask ? kGroundResident : kGroundNone; }
  }
  // a tracker step fed from outside the fused path ran on the slot (links on): its owner row is that step's, over the caller's box list
  void tracker_fed(int slot) { slots[slot].links = kLinksBoxes; scene_drive = 0; }
  void links_switched() { for (auto& s : slots) s.links = kLinksNone; scene_drive = 0; }
  bool box_tracks_valid(int slot) const { return slots[slot].links != kLinksNone; }
  bool point_tracks_valid(int slot) const { return slots[slot].links == kLinksPoints; }
  bool sequence_frame(int slot) const { return slots[slot].sequence; }
  bool accumulated(int slot) const { return slots[slot].accumulated; }
  void step_accumulated(int slot) { slots[slot].accumulated = true; }   // (also: the slot's stream was reset or loaded — the step it holds belongs to ids that are gone)
  // mot_sequence_accumulate_dev has appended the frames the slots hold to stream 0's accumulators (they stay sequence slots: no call appends them again)
  void sequence_accumulated(int frames) { for (int b = 0; b < frames; b++) slots[b].accumulated = true; }
  bool scene_done(int slot) const { return slots[slot].scene; }
  void scene_taken(int slot) { slots[slot].scene = true; scene_drive = 0; }
  void scene_restarted(int slot) { slots[slot].scene = true; slots[slot].scene_restarted = true; scene_drive = 0; }   // the slot's stream was reset or loaded, or the setter emptied the grids
  bool scene_judgeable(int slot) const { return !slots[slot].scene_restarted; }   // (taken or not: judging a step is legal before and after mot_accumulate_scene)
  // mot_sequence_products_dev(MOT_SEQ_SCENE) has taken the frames the slots hold into stream 0's grid (they stay sequence slots: no call takes them again)
  void sequence_scene_taken(int frames) { for (int b = 0; b < frames; b++) slots[b].scene = true; scene_drive = frames; }
  // the frames a drive's judge may cover: every transition that takes a slot (a fused or stage-wise call, a tracker step from outside, the links switched) or that empties
  // or changes a grid (the setter, a reset, a load, mot_accumulate_scene) ends it — any slot's, which is more than needed and costs nothing
  int sequence_scene_frames() const { return scene_drive; }
  bool elev_packed_at(int slot) const { return slots[slot].packed; }
  bool labels_ready(int slot) const { return slots[slot].labels == kLabelsReady; }
  bool cells_usable(int slot) const { return slots[slot].labels == kLabelsFromCells; }
  bool boxes_valid(int slot) const { return slots[slot].boxes; }
  bool regrouped(int slot) const { return slots[slot].boxes && slots[slot].regrouped; }
  bool ground_foreign(int slot) const { return slots[slot].ground == kGroundForeign; }
  // (a slot beyond the last batch: whatever an earlier batch left is not vouched for)
  bool ground_readable(int slot) const { return slots[slot].ground == kGroundResident && slot < last_batch; }
  bool can_rebuild_ground(int slot) const { return last_fused && last_in && last_batch >= 1 && slot < last_batch; }
};

struct mot_ctx;
// A ring of page-locked staging blocks in front of ONE device block: small per-call arguments travel in one stream-ordered H2D copy, no pageable copy (the runtime stages those
// through its own buffer and may hold the calling thread). acquire() hands out the next block and makes the host wait only when the copy queued from it kBlocks calls ago has not
// executed yet, i.e. when the host is that far ahead of the GPU; commit() queues the copy of bytes [src_off, src_off + bytes) of that block to dst, records the block's event and
// moves on. Serves the argument block and the sensor-frame matrices. Memory and events belong to the context's registry.
struct PinnedRing {
  static constexpr int kBlocks = 16;
  char* base = nullptr;                // pinned, kBlocks blocks of block_bytes
  size_t block_bytes = 0;
  hipEvent_t ev[kBlocks] = {};
  bool used[kBlocks] = {};
  int next = 0;
  int create(mot_ctx* c, size_t bytes_per_block);   // skips what exists: resumes after a failed attempt
  int acquire(mot_ctx* c, char** blk);
  int commit(mot_ctx* c, void* dst, size_t src_off, size_t bytes, hipStream_t stream);
};

struct mot_ctx {
  // ownership: every hipMalloc / hipHostMalloc / event of the context is recorded here by the helper that made it (dev_alloc, pinned_alloc, new_event, below) and released by
  // release() or, at the end, by mot_destroy's walk over the records. No member is freed by name anywhere.
  std::vector<void*> own_dev, own_pinned;
  std::vector<hipEvent_t> own_events;
  mot_params params;
  MotDevParams dp;
  int device = 0;
  int cap = 0;        // per-slot stride of the per-point buffers (max_points rounded up to 64)
  int max_points = 0; // points per frame the caller asked for: the limit every entry point enforces
  int batch = 0;      // slots
  int max_tracks_total = 0;
  hipStream_t stream = nullptr;
  std::string err;
  // ground stage
  float4* d_in = nullptr;
  int* d_n = nullptr;
  uint2* d_pairs = nullptr;
  int* d_pair_count = nullptr;
  float* d_hg = nullptr;
  unsigned short* d_cell = nullptr;
  float* d_gzmax = nullptr;
  unsigned long long* d_desc = nullptr;
  int* d_ticket = nullptr;
  float4* d_elev = nullptr;
  float4* d_ground = nullptr;
  uint8_t* d_mask = nullptr;
  int* d_counts = nullptr;
  int max_chunks = 0;
  unsigned epoch = 0;
  // cluster + box stages
  unsigned* d_plane_a = nullptr;
  unsigned* d_plane_b = nullptr;
  unsigned* d_ccl_parent = nullptr;
  OccWord* d_occ_list = nullptr;
  int* d_occ_count = nullptr;
  int occ_chunks = 0;
  GridLabel* d_grid = nullptr;
  std::vector<GridLabel> h_grid16;     // host side of the int32 <-> 16-bit conversion of the ABI's label grid
  int* d_label = nullptr;
  ClusterStats* d_stats = nullptr;
  BoxCandidate* d_cand = nullptr;
  float* d_boxes = nullptr;
  int* d_box_cluster = nullptr;
  unsigned long long* d_rng = nullptr;
  int* d_poly = nullptr;
  PointGroup* d_groups = nullptr;
  int* d_cluster_start = nullptr;
  int* d_order = nullptr;
  SortedGroup* d_gsorted = nullptr;
  int* d_cluster_gstart = nullptr;
  int* d_pix = nullptr;
  // MOT_ORDER_ANY (mot_set_point_order): allocated at the first request, kept until mot_destroy
  int point_order = MOT_ORDER_SCAN;
  unsigned short* d_rg_key = nullptr;
  unsigned* d_rg_tmp = nullptr;
  int* d_rg_hist = nullptr;
  float4* d_rg_xyz = nullptr;          // the cluster-ordered copy of every slot's elevated cloud (12-byte points) ...
  unsigned short* d_rg_cell = nullptr; // ... and of its cells
  PointGroup* d_rg_groups = nullptr;   // group buffers of the mode's own, only in contexts whose cap / 2 is below the mode's group bound
  SortedGroup* d_rg_gsorted = nullptr;
  uint2* d_rg_gscratch = nullptr;
  int rg_group_cap = 0;
  // cluster-node side products (allocated on first use)
  int* d_side_cell = nullptr;
  float4* d_side_cloud = nullptr;
  float4* d_side_obs = nullptr;
  int* d_side_cost = nullptr;
  int* d_side_counts = nullptr;
  int2* d_side_chunks = nullptr;
  float* d_markers = nullptr;          // [kMaxBoxesPerFrame][6], mot_box_markers (allocated at its first call)
  int2* d_wgtab = nullptr;
  int max_wg = 0;
  // staging buffer of mot_ground_remove_pointcloud2 (grow-only, allocated on first use)
  void* d_raw = nullptr;
  size_t raw_bytes = 0;
  // tracker stage
  DevTrack* d_tracks = nullptr;
  int* d_nt = nullptr;
  float* d_tboxes = nullptr;
  TrackFrameArgs* d_targs = nullptr;
  unsigned long long* d_gate = nullptr;
  unsigned long long* d_prog = nullptr;
  int* d_live = nullptr;
  mot_track* d_tout = nullptr;
  int* d_tflags = nullptr;
  EgoTf* d_ego = nullptr;
  int* d_nlive = nullptr;
  Vec2d* d_pos = nullptr;
  int* d_slot_of = nullptr;
  TrackTomb* d_tomb = nullptr;
  unsigned long long* d_used = nullptr;
  int* d_zomb = nullptr;
  int* d_nzomb = nullptr;
  int max_tracks_ever = 0;             // E: capacity of the per-ever-track arrays (positions, slot map, tombstones)
  char* h_pin = nullptr;               // page-locked scratch of the getters' small read-backs (mot_get_tracks: counters, slot bitmap, slot records, per-ever-track
  size_t h_pin_bytes = 0;              // arrays): a copy into pageable memory is staged by the runtime and costs ~10 us apiece whatever its size
  // mot_set_track_links: allocated at the first request, kept until mot_destroy
  int track_links = 0;
  int* d_owner = nullptr;              // [batch][kMaxBoxesPerFrame] box owners of every slot's last tracker step (TrackBuffers::owner)
  int* d_owner_n = nullptr;            // [batch] boxes of that step
  int* d_point_track = nullptr;        // [batch][cap] track id of every elevated point (link.hip)
  // mot_export_track_points_dev / mot_get_track_points (track_points.hip): allocated at the first call, kept until mot_destroy. Only mot_accumulate_track_points shares it
  // (same kernels, same meaning); no other entry point reads it, and the kernels write nothing else of the context's
  int* d_tp_seg_id = nullptr;          // [batch][kMaxBoxesPerFrame] distinct owners of every slot's row
  int* d_tp_seg_boxes = nullptr;       // [batch][kMaxBoxesPerFrame]
  int* d_tp_seg_n = nullptr;           // [batch]
  int* d_tp_rows = nullptr;            // [batch][tp_chunks][kTrackPointKeys]
  int tp_chunks = 0;                   // max_points / kTrackPointChunk rounded up
  EgoTf* d_tp_tf = nullptr;            // [batch] sensor -> global matrices of the slots of an export (MOT_FRAME_GLOBAL), then [batch] ints: the step stamps of an accumulate call
  PinnedRing tp_tf_ring;               // blocks of `batch` matrices and `batch` ints
  char* d_tp_stage = nullptr;          // mot_get_track_points: one slot's records, segments and counts before they go to the host (allocated at ITS first call)
  // mot_set_track_accumulation (track_accum.hip): allocated by the setter, released when it turns the feature off or changes its geometry. The scratch of the
  // per-track point clouds above is shared (distinct owners, per-chunk rows, matrices); the plan is the feature's own
  int accum_K = 0, accum_O = 0;        // points / observations per track; K == 0: off
  mot_accum_row* d_ta_rows = nullptr;      // [batch][max_tracks_total]
  mot_accum_point* d_ta_points = nullptr;  // [batch][max_tracks_total][K]
  mot_accum_obs* d_ta_obs = nullptr;       // [batch][max_tracks_total][O], null when O == 0
  TrackAccumPlan* d_ta_plan = nullptr;     // [batch][kMaxBoxesPerFrame]
  std::vector<int> accum_step;             // [batch] accepted accumulate calls that covered the slot (the next step stamp); a sequence call counts its frames on slot 0
  // mot_sequence_accumulate_dev (track_accum_seq.hip): allocated together at its first call, released WITH the accumulators (the setter: off, or another geometry)
  TrackAccumCapture* d_tas_cap = nullptr;  // [batch][kMaxBoxesPerFrame] what every step of the chain leaves for the append behind it
  TrackAccumSeqSeg* d_tas_seg = nullptr;   // [batch][kMaxBoxesPerFrame] the plan of every (frame, segment)
  // mot_export_track_models_dev / mot_get_track_models (track_models.hip): allocated at the first call, released WITH the accumulators (the setter: off, or another
  // geometry); the ring's events stay in the registry until mot_destroy. The kernels read the accumulators and write only the caller's blocks or the staging blocks
  int* d_tm_latest = nullptr;              // [batch] every slot's latest accumulated step (accum_step - 1), sent ahead of a MOT_MODEL_CURRENT call
  PinnedRing tm_ring;                      // blocks of `batch` ints
  char* d_tm_stage = nullptr;              // mot_get_track_models: one slot's [T headers][2 counts] before they go to the host (allocated at ITS first call)
  mot_accum_point* d_tm_points = nullptr;  // ... and its records: tm_points_cap of them, grown to what a call needs
  size_t tm_points_cap = 0;
  // mot_export_track_model_voxels_dev / mot_get_track_model_voxels (track_voxels.hip): allocated at the first call, released with the blocks above
  char* d_tv_scratch = nullptr;            // [batch][T] plan headers (48 bytes), [batch][T] per-model results (48 bytes), [batch][2] the plan's counts
  char* d_tv_stage = nullptr;              // the getter: one slot's [T headers][2 counts] before they go to the host (allocated at ITS first call)
  mot_model_voxel* d_tv_voxels = nullptr;  // ... and its voxels: tv_voxels_cap of them, grown to what a call needs
  size_t tv_voxels_cap = 0;
  // mot_set_scene_grid (scene_grid.hip, mot_api_scene.hip): allocated by the setter, released when it turns the feature off or changes its geometry
  int scene_W = 0;                         // cells per side; 0: off
  float scene_cell = 0.f, scene_inv = 0.f; // metres per cell, and 1.0f / cell
  SceneCell* d_sg_cells = nullptr;         // [batch][W * W], toroidal
  mot_scene_header* d_sg_hdr = nullptr;    // [batch] the latest step's header
  SceneWindow* d_sg_prev = nullptr;        // [batch] the origin the cells are laid out for
  char* d_sg_args = nullptr;               // [batch] sensor -> global matrices, then [batch] ints: the step stamps of an accumulate call
  PinnedRing sg_ring;                      // blocks of `batch` matrices and `batch` ints
  mot_scene_cell* d_sg_stage = nullptr;    // mot_get_scene_grid: one slot's unrolled cells before they go to the host (allocated at ITS first call)
  std::vector<int> scene_step;             // [batch] accepted mot_accumulate_scene calls that covered the slot (the next step stamp)
  // mot_export_scene_points_dev / mot_get_scene_points (scene_judge.hip): allocated at the first call, all three or none; released with the blocks above
  uint8_t* d_sj_cls = nullptr;             // [batch][cap] class of every elevated point
  int* d_sj_rows = nullptr;                // [batch][sj_chunks][10] per chunk the points per class and where its records go
  int sj_chunks = 0;                       // max_points / kSceneChunk rounded up
  char* d_sj_args = nullptr;               // [batch] sensor -> global matrices (a block as d_sg_args, sent through sg_ring)
  char* d_sj_stage = nullptr;              // mot_get_scene_points: one slot's records, segments and classes before they go to the host (allocated at ITS first call)
  // mot_sequence_products_dev(MOT_SEQ_SCENE) (scene_grid_seq.hip): allocated at its first call, both or neither; released with the blocks above
  SceneSeqFrame* d_sgs_win = nullptr;      // [batch + 1] every frame's window and what is left of it at the end of the call; entry 0: the window before the call
  unsigned* d_sgs_static = nullptr;        // [batch][(E + 31) / 32] per frame one bit per track id: flagged static as that frame's step left it
  // mot_export_sequence_scene_points_dev / mot_get_sequence_scene_points (scene_judge_seq.hip): the judge's scratch above, and at the first call of these
  int* d_sjs_base = nullptr;               // [batch][5] a frame's points per class, then where its first record of the class goes in the drive's block
  char* d_sjs_stage = nullptr;             // the getter: [batch][5] + [5] segments before they go to the host (allocated at ITS first call)
  // mot_export_sequence_scene_voxels_dev / mot_get_sequence_scene_voxels (scene_voxels_seq.hip): the drive judge's scratch above, and ONE block of their own
  char* d_sv_scratch = nullptr;            // mot_scene_voxel_scratch_bytes(sv_cap, batch): keys, payloads, staged records, the sort's table, the plan, the judge's two tables
  long sv_cap = -1;                        // the record capacity the block was laid out for (grown on demand; -1: none)
  char* d_sv_stage = nullptr;              // the getter: the header and [5] totals before they go to the host (allocated at ITS first call)
  // mot_merge_voxel_maps_dev / mot_merge_voxel_maps (voxel_merge.hip): ONE block of their own, allocated at the first call, kept until mot_destroy (no grid needed)
  char* d_vm_scratch = nullptr;            // mot_voxel_merge_scratch_bytes(vm_cap): keys, payloads, the sort's table, the per-tile counts, the plan
  long vm_cap = -1;                        // the sum of capacities the block was laid out for (grown on demand; -1: none)
  int vm_short_max = 64;                   // runs of at most so many inputs are summed by one thread (mot_debug_voxel_merge_cut: measurement; the bytes do not depend on it)
  // mot_export_map_points_dev / mot_get_map_points (map_judge.hip): blocks of their own — the calls work with the grid off, so nothing here is the grid's.
  // Allocated at the first call, the three blocks and the ring or none; kept until mot_destroy
  uint8_t* d_mj_cls = nullptr;             // [batch][cap] class of every elevated point
  int* d_mj_rows = nullptr;                // [batch][mj_chunks][10] per chunk the points per class and where its records go
  int mj_chunks = 0;                       // max_points / kSceneChunk rounded up
  char* d_mj_args = nullptr;               // [batch] sensor -> global matrices
  PinnedRing mj_ring;                      // blocks of `batch` matrices
  char* d_mj_stage = nullptr;              // mot_get_map_points: one slot's records, segments and classes before they go to the host (allocated at ITS first call)
  std::vector<EgoTf> link_tf;          // [batch] the matrix every slot's boxes took in its last fused call with the tracker, kept while links are on (host side)
  Vec2d* d_cp = nullptr;
  TrackItem* d_items = nullptr;
  int* d_nitems = nullptr;
  struct SlotEgo {  // file-scope globals of OT/tracking/imm_ukf_jpda.cpp:19-24,56-70, one set per stream
    bool init = false, ego_called = false;
    bool tracks_restart = false;   // mot_reset_tracks_slot: the next tracker step seeds anew, the ego history stays
    double timestamp = 0, egoVelo = 0, egoYaw = 0, egoPreYaw = 0;
    double rx = 0, ry = 0, ryaw = -M_PI / 2;   // running result of the ego-history replay (:137-151)
    double egoPoint[3] = {0, 0, 0};
    double step_ego_yaw = 0;   // egoPoints_[0][2] of the last tracker step (the outputs of evicted tracks add it to their frozen yaw)
    int nt = 0;
  };
  std::vector<SlotEgo> ego;
  // Per-batch launch arguments — points per frame, tracker arguments, sensor -> global matrices — live in ONE device block
  // (d_n, d_targs and d_ego point into it) and travel in ONE stream-ordered H2D copy at the head of a launch sequence, from a ring
  // of page-locked staging blocks: no pageable copy (the runtime stages those through its own buffer and may hold the calling
  // thread), and nothing between the box stage's last kernel and the tracker's first.
  char* d_argblk = nullptr;
  PinnedRing arg_ring;                 // blocks of arg_bytes
  size_t arg_bytes = 0, arg_off_targs = 0, arg_off_ego = 0, arg_off_launch = 0;
  // launch sequences captured as hipGraphs (contexts of few streams: the per-frame latency path), keyed by launch geometry
  struct GraphKey { int batch, chunks, tracker, outputs, order; };
  struct GraphEntry { GraphKey key; void* exec; };
  std::vector<GraphEntry> graphs;
  int graph_mode = 0;                  // 0 off, 1 on; turned off for good when a capture fails
  int tracker_mode = MOT_TRACKER_AUTO; // mot_set_tracker_mode
  int trace_ranges = 0;                // mot_set_trace_ranges
  // host mirrors
  std::vector<int> h_n;
  unsigned short* d_ecell = nullptr;   // Cartesian cell of every elevated point (fused path: compaction kernel -> label kernel)
  int fused_outputs = 0;               // MOT_OUT_* the fused entry points materialise besides what the next stage needs
  Residency res;                       // what each slot holds (above)
  int dbg_skip = 0;                    // mot_debug_skip_kernels: MEASUREMENT ONLY (upper bounds of launch-fusion experiments); the results of a frame are then stale
  int* h_counts = nullptr;  // pinned [batch][4]
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // pipelined host ingest (mot_frames_host): a copy stream and two staging copies of the input batch
  hipStream_t copy_stream = nullptr;
  bool copy_ready = false;             // copy stream, staging buffers and events all exist
  float4* d_stage[2] = {nullptr, nullptr};
  unsigned char* d_stage_raw[2] = {nullptr, nullptr};   // mot_frames_host_pointcloud2: where the raw message payloads land (grow-only, batch x cap x point_step bytes)
  size_t stage_raw_bytes = 0;
  float* d_stage12[2] = {nullptr, nullptr};        // mot_frames_host_xyz: where the packed {x, y, z} records land (12 bytes a point); expanded into d_stage[i] on the compute stream
  hipEvent_t ev_expanded[2] = {nullptr, nullptr};  // the expansion kernel that read d_stage12[i] has run (compute stream)
  bool stage12_used[2] = {false, false};
  hipEvent_t ev_copied[2] = {nullptr, nullptr};    // H2D of stage[i] complete (copy stream)
  hipEvent_t ev_consumed[2] = {nullptr, nullptr};  // last kernel reading stage[i] launched and done (compute stream)
  bool stage_used[2] = {false, false};
  int stage_next = 0;
  // device block of mot_fetch_tracks_async
  mot_track* d_fetch = nullptr;
  int* d_fetch_counts = nullptr;
  int fetch_cap = 0;
  // MOT_FRAME_SENSOR exports (mot_export_tracks*_frame_dev, mot_fetch_tracks_frame_async, mot_tracking_node_frame): every slot's global -> sensor matrix, computed
  // from the slot's dead reckoning at call time, goes to d_sensor_tf in ONE stream-ordered copy ahead of the export kernel, from a ring of page-locked blocks
  // like the argument block's (no host synchronisation; nothing here reads d_ego, which the fused sequence rewrites every call). Allocated at the first such call.
  EgoTf* d_sensor_tf = nullptr;
  PinnedRing sensor_tf_ring;           // blocks of `batch` matrices
  // mot_tracking_node_frame (allocated at its first call): the frame's boxes in the sensor frame — a staging buffer of their own, d_boxes belongs to the box
  // stage — and the device block its results leave in: [T records][n_live, n_ever, flags, 0]
  float* d_node_boxes = nullptr;
  char* d_node_out = nullptr;
  // in-run kernel timing (mot_profile_kernel): event pairs around one kernel inside mot_frames_dev / mot_frames_host
  int prof_kernel = 0;
  int prof_every = 1, prof_seen = 0;   // every prof_every-th launch of the kernel is recorded
  static constexpr int kProfRing = 64;
  hipEvent_t prof_ev[kProfRing][2] = {};
  int prof_n = 0;
};

// every entry point runs with the context's device current and puts the caller's device back afterwards: contexts on
// different GPUs in one process, callback threads, torch.cuda.set_device after mot_create all work
struct DevGuard {
  int prev = -1;
  bool changed = false;
  explicit DevGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = hipSetDevice(dev) == hipSuccess;
  }
  ~DevGuard() { if (changed) (void)hipSetDevice(prev); }
};
#define MOT_GUARD(c) DevGuard guard_((c)->device)

#define MOT_HIP_AS(ctx, what, call)                                                            \
  do {                                                                                         \
    hipError_t e_ = (call);                                                                    \
    if (e_ != hipSuccess) {                                                                    \
      (ctx)->err = std::string(what) + ": " + hipGetErrorString(e_);                           \
      return MOT_E_HIP;                                                                        \
    }                                                                                          \
  } while (0)
#define MOT_HIP(ctx, call) MOT_HIP_AS(ctx, #call, call)
#define MOT_TRY(call) do { const int rc_ = (call); if (rc_ != MOT_OK) return rc_; } while (0)

inline int fail(mot_ctx* c, int code, const char* msg) { if (c) c->err = msg; return code; }
inline int fail(mot_ctx* c, int code, const char* who, const char* msg) { c->err = std::string(who) + msg; return code; }   // "<entry point>: ..."

// ---------------------------------------------------------------------------------------- ownership (defined in mot_api.hip)
// The only code of the host layer that allocates or releases for a context. Each helper skips what already exists — a lazy allocator that failed half-way leaves what it got in
// the registry (for mot_destroy, and for the next request, which resumes) — and records what it hands out. (macros: a refusal names the member that could not be had,
// "hipMalloc(&c->d_rg_key): ..."; dev_zeroed: dev_alloc + a memset to 0 queued on the context stream)
enum OwnKind { kOwnDev, kOwnDevZeroed, kOwnPinned };
int own_alloc(mot_ctx* c, void** p, size_t bytes, OwnKind kind, const char* what);
int own_event(mot_ctx* c, hipEvent_t* ev, unsigned flags, const char* what);
#define dev_alloc(c, p, bytes) own_alloc((c), reinterpret_cast<void**>(p), (bytes), kOwnDev, "hipMalloc(" #p ")")
#define dev_zeroed(c, p, bytes) own_alloc((c), reinterpret_cast<void**>(p), (bytes), kOwnDevZeroed, "hipMalloc(" #p ")")
#define pinned_alloc(c, p, bytes) own_alloc((c), reinterpret_cast<void**>(p), (bytes), kOwnPinned, "hipHostMalloc(" #p ")")
#define new_event(c, ev, flags) own_event((c), (ev), (flags), "hipEventCreateWithFlags(" #ev ")")
int own_release(mot_ctx* c, void** p);   // the grow-only buffers that are replaced; *p = nullptr. The caller has made sure that nothing reads it any more
template <typename T> inline int release(mot_ctx* c, T** p) { return own_release(c, reinterpret_cast<void**>(p)); }
int drop_graphs(mot_ctx* c);             // drains the context stream if a captured launch sequence exists, then destroys them all

// kernel ids used by mot_time_stage and mot_profile_kernel
enum { kK1 = 10, kK2 = 11, kK3 = 12, kC1 = 20, kC2 = 21, kB1 = 30, kB2 = 31, kB3 = 32, kB2b = 33, kB1b = 34, kR1 = 35, kR2 = 36, kR3 = 37, kT1 = 40 };
struct ProfScope {
  mot_ctx* c; bool on;
  ProfScope(mot_ctx* ctx, int id) : c(ctx), on(false) {
    if (ctx->prof_kernel != id || ctx->prof_n >= mot_ctx::kProfRing) return;
    on = (ctx->prof_seen++ % ctx->prof_every) == 0;
    if (on) (void)hipEventRecord(c->prof_ev[c->prof_n][0], c->stream);
  }
  ~ProfScope() { if (on) { (void)hipEventRecord(c->prof_ev[c->prof_n][1], c->stream); c->prof_n++; } }
};

// ---------------------------------------------------------------------------------------- helpers that cross the host files
// mot_api.hip
int arg_block_acquire(mot_ctx* c, char** blk);
int arg_block_commit(mot_ctx* c, size_t off, size_t bytes);
ClusterBuffers cluster_buffers(mot_ctx* c, int slot = -1);
ClusterBuffers regrouped_view(const mot_ctx* c, ClusterBuffers cb);
ClusterBuffers box_products(mot_ctx* c, int slot);
ClusterBuffers launch_box_stage(mot_ctx* c, const ClusterBuffers& cb, int n);
int next_epoch(mot_ctx* c);
GroundBuffers ground_buffers(mot_ctx* c, const float4* in, long stride, bool want_mask, bool planes = false);
int check_field_offsets(mot_ctx* c, int point_step, int off_x, int off_y, int off_z, int off_w);
int set_batch(mot_ctx* c, const int* n_points, int batch, const float4* in, long stride, bool upload = true);
void fused_buffers(mot_ctx* c, GroundBuffers* g, ClusterBuffers* cb);
RegroupBuffers fused_regroup_buffers(const mot_ctx* c);
// mot_api_stages.hip
int fetch_counts(mot_ctx* c, int slot);
// mot_api_tracks.hip
void tf_velodyne_to_global(double x, double y, double yaw, float m[12]);
TrackBuffers track_buffers(mot_ctx* c, bool fused);
void prepare_track_args(mot_ctx* c, TrackFrameArgs* targs, int slot, int m, double timestamp, bool run);
int pinned_scratch(mot_ctx* c, size_t bytes, char** out);
int accum_restart_slots(mot_ctx* c, int first, int n);   // the accumulators of those streams back to empty, stream-ordered (nothing while the feature is off)
// mot_api_scene.hip
int scene_restart_slots(mot_ctx* c, int first, int n);   // the scene grids of those streams back to empty, stream-ordered (nothing while the feature is off)
// mot_sequence_accumulate_dev's share of the accumulators (the entry point itself is mot_sequence_dev's body, mot_api.hip): links and accumulation on and the scratch
// there, before anything runs / the capture behind tracker step `frame` / the append of slots 0 .. frames - 1 behind the chain, with the host's bookkeeping
int seq_accum_ready(mot_ctx* c, const char* who);
void seq_accum_capture(mot_ctx* c, int frame);
int seq_accum_append(mot_ctx* c, int frames, int max_n);
// ... and into stream 0's scene grid (mot_api_scene.hip, scene_grid_seq.hip): ready refuses (grid or links off, no scratch) before anything has run and zeroes the
// capture table of `frames` frames; capture right behind tracker step `frame`; append behind the last step and the point links
int seq_scene_ready(mot_ctx* c, const char* who, int frames);
void seq_scene_capture(mot_ctx* c, int frame);
int seq_scene_append(mot_ctx* c, int frames, int max_n);

// ---------------------------------------------------------------------------------------- the elevated cloud and its links as the track and scene kernels see them
// ONE owner for each view and for each step around a launch that mot_api_tracks.hip and mot_api_scene.hip share. The views carry slot 0's cloud layout (what a
// recorded drive has throughout: one fused call filled its slots); a launch over live slots sets elevated_packed per run of for_layout_runs.
inline int check_links_on(mot_ctx* c, const char* who) { return c->track_links ? MOT_OK : fail(c, MOT_E_STATE, who, ": track links are off (mot_set_track_links)"); }
// the slot's per-point ids belong to the cloud it holds. THE test of every call that reads them (accumulators and scene grid cannot be on with the links off, so
// their callers never see the first message)
inline int check_point_tracks(mot_ctx* c, int slot, const char* who) {
  MOT_TRY(check_links_on(c, who));
  if (!c->res.point_tracks_valid(slot))
    return fail(c, MOT_E_STATE, who, ": the slot's cloud, boxes and tracker step do not come from one fused call (a stage-wise call took the slot, the tracker was fed from outside, "
                                     "or no fused call ran the tracker since the links were turned on)");
  return MOT_OK;
}
inline TrackPointBuffers track_point_buffers(const mot_ctx* c) {
  TrackPointBuffers t;
  t.ids = c->d_point_track; t.elevated = c->d_elev; t.elevated_packed = c->res.elev_packed_at(0) ? 1 : 0; t.cap = c->cap; t.counts = c->d_counts; t.owner = c->d_owner;
  t.seg_id = c->d_tp_seg_id; t.seg_boxes = c->d_tp_seg_boxes; t.seg_n = c->d_tp_seg_n; t.rows = c->d_tp_rows; t.max_chunks = c->tp_chunks;
  return t;
}
// live: the kind of an owned point comes from the slot's map and records; recorded (a drive's frames): from the captured bits, slot_of / out are not read
inline SceneSplatInput scene_input(const mot_ctx* c, bool live) {
  SceneSplatInput in;
  in.ids = c->d_point_track; in.elevated = c->d_elev; in.elevated_packed = c->res.elev_packed_at(0) ? 1 : 0; in.cap = c->cap; in.counts = c->d_counts;
  in.slot_of = live ? c->d_slot_of : nullptr; in.out = live ? c->d_tout : nullptr;
  in.T = c->max_tracks_total; in.E = c->max_tracks_ever;
  return in;
}
inline SceneJudgeBuffers judge_buffers(const mot_ctx* c, const mot_scene_judge_params* p, int class_mask) {
  SceneJudgeBuffers j;
  j.cls = c->d_sj_cls; j.rows = c->d_sj_rows; j.max_chunks = c->sj_chunks;
  j.min_static_hits = p->min_static_hits; j.trail_num = p->trail_num; j.trail_den = p->trail_den; j.class_mask = class_mask;
  return j;
}
// fn(k0, k1, packed) once per run [first + k0, first + k1) of slots whose clouds share a layout (12- or 16-byte points: slots filled by fused calls under different
// mot_set_fused_outputs may differ), k0 / k1 counted from `first`: a batch goes out as one launch per run — one, as a rule
template <class Fn> inline void for_layout_runs(const mot_ctx* c, int first, int n, Fn fn) {
  for (int k0 = 0; k0 < n;) {
    const bool packed = c->res.elev_packed_at(first + k0);
    int k1 = k0 + 1;
    while (k1 < n && c->res.elev_packed_at(first + k1) == packed) k1++;
    fn(k0, k1, packed ? 1 : 0);
    k0 = k1;
  }
}
// The matrices the boxes of slots first .. first + n - 1 took (link_tf) and, with `stamps`, those slots' step stamps behind them: through `ring` into `d_block` in ONE
// stream-ordered copy ahead of the kernels that read them. *d_tf / *d_stamps: where they lie on the device
inline int send_link_tf(mot_ctx* c, PinnedRing* ring, void* d_block, int first, int n, const std::vector<int>* stamps, const EgoTf** d_tf, const int** d_stamps = nullptr) {
  char* raw;
  MOT_TRY(ring->acquire(c, &raw));
  size_t bytes = (size_t)n * sizeof(EgoTf);
  memcpy(raw, c->link_tf.data() + first, bytes);
  if (stamps) { memcpy(raw + bytes, stamps->data() + first, (size_t)n * sizeof(int)); bytes += (size_t)n * sizeof(int); }
  MOT_TRY(ring->commit(c, d_block, 0, bytes, c->stream));
  *d_tf = static_cast<const EgoTf*>(d_block);
  if (stamps) *d_stamps = reinterpret_cast<const int*>(*d_tf + n);
  return MOT_OK;
}
// a getter's grow-only staging block: at least n elements, in steps of 64 Ki; the old block goes first (the caller has drained the stream: nothing reads it)
inline int grow_stage_as(mot_ctx* c, void** p, size_t* cap, size_t n, size_t elem_bytes, const char* what) {
  if (*cap >= n) return MOT_OK;
  MOT_TRY(own_release(c, p));
  *cap = 0;
  const size_t want = (n + 65535) & ~(size_t)65535;
  MOT_TRY(own_alloc(c, p, want * elem_bytes, kOwnDev, what));
  *cap = want;
  return MOT_OK;
}
#define grow_stage(c, p, cap, n, elem_bytes) grow_stage_as((c), reinterpret_cast<void**>(p), (cap), (n), (elem_bytes), "hipMalloc(" #p ")")
// a getter's counts (at most four ints) back through the page-locked scratch, the stream drained; the range checks are the caller's
inline int read_counts(mot_ctx* c, const int* d_cnt, int n_ints, int* host_out) {
  char* pin;
  MOT_TRY(pinned_scratch(c, 16, &pin));
  MOT_HIP(c, hipMemcpyAsync(pin, d_cnt, (size_t)n_ints * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  memcpy(host_out, pin, (size_t)n_ints * sizeof(int));
  return MOT_OK;
}
// head of a packed live-track block: one count per slot, padded to 16 bytes; the records follow (mot_export_tracks_packed_dev, mot_gather)
inline long mot_packed_head_bytes(int batch) { return ((long)batch * 4 + 15) & ~15l; }
#endif  // MOT_HOST_H_
