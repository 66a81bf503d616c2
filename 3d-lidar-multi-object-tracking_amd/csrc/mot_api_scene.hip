// mot_api_scene.hip — host side of the C-ABI (include/mot.h), the rolling static-scene grid: the setter and what it owns, the per-slot step counters, the state
// checks of mot_accumulate_scene, the two readers, the frame's points and a recorded drive's points judged against the grid, the drive's static map thinned to voxels, voxel maps merged into one, voxel maps indexed and the frame's points judged against the index (its own scratch: no grid needed). Kernels: scene_grid.hip, scene_grid_seq.hip, scene_judge.hip, scene_judge_seq.hip, scene_voxels_seq.hip, voxel_merge.hip, map_judge.hip. Context and helpers: mot_host.h.
#include "mot_host.h"

// The setter owns the feature's memory: cells, headers, previous origins, the argument block and its ring of page-locked staging blocks are allocated together and
// released together (off, or another geometry); the getter's staging block, taken at ITS first call, goes with them. (The ring's events stay in the registry until
// mot_destroy, as those of every ring do.)
struct SceneBlocks {
  SceneCell* cells = nullptr; mot_scene_header* hdr = nullptr; SceneWindow* prev = nullptr; char* args = nullptr;
};
static int scene_release(mot_ctx* c, SceneBlocks* s) {
  MOT_TRY(release(c, &s->cells)); MOT_TRY(release(c, &s->hdr)); MOT_TRY(release(c, &s->prev));
  return release(c, &s->args);
}
// what mot_sequence_products_dev(MOT_SEQ_SCENE) took at its first call: both blocks or neither (the caller has drained the stream)
static int seq_scene_release(mot_ctx* c) {
  MOT_TRY(release(c, &c->d_sgs_win));
  return release(c, &c->d_sgs_static);
}
// what mot_export_scene_points_dev took at its first call (all three or none) and the getter's staging block (the caller has drained the stream)
static int judge_release(mot_ctx* c) {
  MOT_TRY(release(c, &c->d_sj_cls)); MOT_TRY(release(c, &c->d_sj_rows)); MOT_TRY(release(c, &c->d_sj_args));
  MOT_TRY(release(c, &c->d_sjs_base)); MOT_TRY(release(c, &c->d_sjs_stage));   // (the drive's judge: its bases and its getter's staging block)
  MOT_TRY(release(c, &c->d_sv_scratch)); c->sv_cap = -1; MOT_TRY(release(c, &c->d_sv_stage));   // (the drive's voxels: scene_voxels_seq.hip)
  return release(c, &c->d_sj_stage);
}
static size_t scene_arg_bytes(const mot_ctx* c) { return (size_t)c->batch * (sizeof(EgoTf) + sizeof(int)); }   // [batch] matrices, then [batch] step stamps
static SceneGridBuffers scene_buffers(const mot_ctx* c) {
  SceneGridBuffers g;
  g.cells = c->d_sg_cells; g.hdr = c->d_sg_hdr; g.prev = c->d_sg_prev; g.W = c->scene_W; g.log2_W = __builtin_ctz((unsigned)c->scene_W); g.cell = c->scene_cell; g.inv = c->scene_inv;
  return g;
}
static int check_scene_on(mot_ctx* c, const char* who) { return c->scene_W ? MOT_OK : fail(c, MOT_E_STATE, who, ": the scene grid is off (mot_set_scene_grid)"); }

int scene_restart_slots(mot_ctx* c, int first, int n) {
  if (!c->scene_W) return MOT_OK;
  const size_t slot_cells = (size_t)c->scene_W * c->scene_W;
  MOT_HIP(c, hipMemsetAsync(c->d_sg_cells + (size_t)first * slot_cells, 0, (size_t)n * slot_cells * sizeof(SceneCell), c->stream));
  mot_launch_scene_reset(scene_buffers(c), first, n, c->stream);
  MOT_HIP(c, hipGetLastError());
  for (int b = first; b < first + n; b++) { c->scene_step[b] = 0; c->res.scene_restarted(b); }
  return MOT_OK;
}

// off: nothing may still read the blocks
static int scene_off(mot_ctx* c) {
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  c->scene_W = 0; c->scene_cell = 0.f; c->scene_inv = 0.f;
  SceneBlocks s = {c->d_sg_cells, c->d_sg_hdr, c->d_sg_prev, c->d_sg_args};
  c->d_sg_cells = nullptr; c->d_sg_hdr = nullptr; c->d_sg_prev = nullptr; c->d_sg_args = nullptr;
  MOT_TRY(scene_release(c, &s));
  MOT_TRY(release(c, &c->sg_ring.base));
  for (bool& u : c->sg_ring.used) u = false;
  MOT_TRY(seq_scene_release(c));
  MOT_TRY(judge_release(c));
  return release(c, &c->d_sg_stage);
}

extern "C" int mot_set_scene_grid(mot_ctx* c, const mot_scene_params* p) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_set_scene_grid";
  if (!p) return c->scene_W ? scene_off(c) : MOT_OK;
  if (!(p->cell >= 0.05f && p->cell <= 10.f)) return fail(c, MOT_E_ARG, who, ": cell must be finite and in [0.05, 10] metres");   // (NaN fails both compares)
  const int W = p->size;
  if (W < 64 || W > 2048 || (W & (W - 1))) return fail(c, MOT_E_ARG, who, ": size must be a power of two in [64, 2048]");
  MOT_TRY(check_links_on(c, who));
  if (W == c->scene_W && p->cell == c->scene_cell) return MOT_OK;
  // the new blocks first: a failure leaves the mode, an earlier geometry included, as it was
  const bool had_ring = c->sg_ring.base != nullptr;
  SceneBlocks s;
  int rc = dev_alloc(c, &s.cells, (size_t)c->batch * W * W * sizeof(SceneCell));
  if (!rc) rc = dev_alloc(c, &s.hdr, (size_t)c->batch * sizeof(mot_scene_header));
  if (!rc) rc = dev_alloc(c, &s.prev, (size_t)c->batch * sizeof(SceneWindow));
  if (!rc) rc = dev_alloc(c, &s.args, scene_arg_bytes(c));
  if (!rc) rc = c->sg_ring.create(c, scene_arg_bytes(c));   // (skips what exists: the blocks do not depend on the geometry)
  if (rc) {
    const std::string why = c->err;
    (void)scene_release(c, &s);
    if (!had_ring) (void)release(c, &c->sg_ring.base);
    c->err = why;
    return rc;
  }
  if (c->scene_W) {   // another geometry: nothing may still read the old blocks
    MOT_HIP(c, hipStreamSynchronize(c->stream));
    SceneBlocks old = {c->d_sg_cells, c->d_sg_hdr, c->d_sg_prev, c->d_sg_args};
    MOT_TRY(scene_release(c, &old));
    MOT_TRY(seq_scene_release(c));
    MOT_TRY(judge_release(c));
    MOT_TRY(release(c, &c->d_sg_stage));
  }
  c->d_sg_cells = s.cells; c->d_sg_hdr = s.hdr; c->d_sg_prev = s.prev; c->d_sg_args = s.args;
  c->scene_W = W; c->scene_cell = p->cell; c->scene_inv = 1.0f / p->cell;
  c->scene_step.assign(c->batch, 0);
  return scene_restart_slots(c, 0, c->batch);   // every grid empty; the steps the slots hold were taken without the feature: the next fused call is the first to be taken
}

extern "C" int mot_accumulate_scene(mot_ctx* c, int batch) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_accumulate_scene";
  MOT_TRY(check_scene_on(c, who));
  if (batch < 1 || batch > c->batch) return fail(c, MOT_E_ARG, who, ": batch out of range");
  for (int b = 0; b < batch; b++) {   // every slot before anything is launched or counted
    MOT_TRY(check_point_tracks(c, b, who));
    if (c->res.sequence_frame(b)) return fail(c, MOT_E_STATE, who, ": the slots hold the frames of ONE stream (mot_sequence_dev); mot_sequence_products_dev(MOT_SEQ_SCENE) takes a drive's frames into "
                                                                              "the grid inside the sequence call");
    if (c->res.scene_done(b)) return fail(c, MOT_E_STATE, who, ": a slot of the batch was already taken into its grid for its current step, or was reset / loaded since that step");
  }
  const EgoTf* d_tf; const int* d_steps;   // the matrices the slots' boxes took and the slots' step stamps
  MOT_TRY(send_link_tf(c, &c->sg_ring, c->d_sg_args, 0, batch, &c->scene_step, &d_tf, &d_steps));
  SceneSplatInput in = scene_input(c, true);
  const SceneGridBuffers g = scene_buffers(c);
  for_layout_runs(c, 0, batch, [&](int k0, int k1, int packed) {
    in.elevated_packed = packed;
    mot_launch_scene_accumulate(g, in, k0, k1 - k0, c->max_points, d_tf + k0, d_steps + k0, c->stream);
  });
  MOT_HIP(c, hipGetLastError());
  for (int b = 0; b < batch; b++) { c->scene_step[b]++; c->res.scene_taken(b); }
  return MOT_OK;
}

// ---------------------------------------------------------------------------------------- the grid fed by sequence mode (scene_grid_seq.hip)
// mot_sequence_products_dev with MOT_SEQ_SCENE is mot_sequence_dev's body (mot_api.hip) with these three hooks. The scratch of the feature's own — 32 bytes per
// frame for the windows and one bit per track id and frame for the kinds — is taken at the first call, both blocks or neither (a failure leaves the live allocations
// as they were), and goes with the grid.
static SceneSeqBuffers seq_scene_buffers(const mot_ctx* c) {
  SceneSeqBuffers s;
  s.win = c->d_sgs_win; s.is_static = c->d_sgs_static; s.words = (c->max_tracks_ever + 31) / 32; s.step0 = c->scene_step[0];
  return s;
}
int seq_scene_ready(mot_ctx* c, const char* who, int frames) {
  MOT_TRY(check_scene_on(c, who));
  MOT_TRY(check_links_on(c, who));
  const size_t row_bytes = (size_t)((c->max_tracks_ever + 31) / 32) * sizeof(unsigned);
  if (!c->d_sgs_win || !c->d_sgs_static) {
    int rc = dev_alloc(c, &c->d_sgs_win, ((size_t)c->batch + 1) * sizeof(SceneSeqFrame));
    if (!rc) rc = dev_alloc(c, &c->d_sgs_static, (size_t)c->batch * row_bytes);
    if (rc) {
      const std::string why = c->err;
      (void)seq_scene_release(c);
      c->err = why;
      return rc;
    }
  }
  // the captures set bits with an OR: every frame's row starts from zero (scratch of the call's own: nothing anybody reads if the call is refused after this)
  MOT_HIP(c, hipMemsetAsync(c->d_sgs_static, 0, (size_t)frames * row_bytes, c->stream));
  return MOT_OK;
}
void seq_scene_capture(mot_ctx* c, int frame) {
  mot_launch_scene_seq_capture(c->d_counts, c->d_owner, c->d_slot_of, c->d_tout, c->max_tracks_total, c->max_tracks_ever, seq_scene_buffers(c), frame, c->stream);
}
int seq_scene_append(mot_ctx* c, int frames, int max_n) {
  // frame k's matrix is entry k of the call's own argument block (what link_tf[k] keeps on the host): later calls rewrite it behind these kernels, stream-ordered
  mot_launch_scene_sequence(scene_buffers(c), scene_input(c, false), seq_scene_buffers(c), frames, max_n, c->d_ego, c->stream);   // (slot 0's layout: one fused call filled the slots)
  MOT_HIP(c, hipGetLastError());
  c->scene_step[0] += frames;   // (a frame refused for capacity has no points to add and counts)
  c->res.sequence_scene_taken(frames);
  return MOT_OK;
}

extern "C" int mot_export_scene_grid_dev(mot_ctx* c, int batch, mot_scene_cell* d_cells, long cell_stride, mot_scene_header* d_headers) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_export_scene_grid_dev";
  MOT_TRY(check_scene_on(c, who));
  if (!d_cells || !d_headers || batch < 1 || batch > c->batch || cell_stride < (long)c->scene_W * c->scene_W || ((size_t)d_cells & 15) || ((size_t)d_headers & 3))
    return fail(c, MOT_E_ARG, who, ": bad argument (null or misaligned block, cell_stride below size^2, batch out of range)");
  mot_launch_scene_export(scene_buffers(c), 0, batch, d_cells, cell_stride, d_headers, c->stream);
  MOT_HIP(c, hipGetLastError());
  return MOT_OK;
}

extern "C" int mot_get_scene_grid(mot_ctx* c, int slot, mot_scene_cell* cells, int capacity, int* n_cells, mot_scene_header* header) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_get_scene_grid";
  if (slot < 0 || slot >= c->batch || capacity < 0 || !n_cells) return fail(c, MOT_E_ARG, who, ": slot or capacity out of range, or null n_cells");
  MOT_TRY(check_scene_on(c, who));
  const size_t n = (size_t)c->scene_W * c->scene_W;
  *n_cells = (int)n;
  if (cells && (size_t)capacity < n) return fail(c, MOT_E_CAPACITY, "more cells (size^2) than the caller's buffer holds");
  char* pin;
  MOT_TRY(pinned_scratch(c, sizeof(mot_scene_header), &pin));
  if (cells) {   // the slot alone, unrolled into the staging block; the header comes from the device block either way
    MOT_TRY(dev_alloc(c, &c->d_sg_stage, n * sizeof(mot_scene_cell)));
    mot_launch_scene_export(scene_buffers(c), slot, 1, c->d_sg_stage, (long)n, nullptr, c->stream);
    MOT_HIP(c, hipGetLastError());
    MOT_HIP(c, hipMemcpyAsync(cells, c->d_sg_stage, n * sizeof(mot_scene_cell), hipMemcpyDeviceToHost, c->stream));
  }
  if (header) MOT_HIP(c, hipMemcpyAsync(pin, c->d_sg_hdr + slot, sizeof(mot_scene_header), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  if (header) memcpy(header, pin, sizeof(mot_scene_header));
  return MOT_OK;
}

// ---------------------------------------------------------------------------------------- a frame's points judged against the grid (scene_judge.hip)
// The validity of mot_accumulate_scene without its once-per-step clause: the step may have been taken or not, but a grid emptied since (the setter, a reset, a load)
// no longer belongs to the step the slot holds.
static int check_judge_slot(mot_ctx* c, int b, const char* who) {
  MOT_TRY(check_point_tracks(c, b, who));
  if (c->res.sequence_frame(b)) return fail(c, MOT_E_STATE, who, ": the slots hold the frames of ONE stream (mot_sequence_dev)");
  if (!c->res.scene_judgeable(b)) return fail(c, MOT_E_STATE, who, ": the slot's grid was emptied (mot_set_scene_grid, a reset or a load) since the step the slot holds");
  return MOT_OK;
}
static int check_judge_args(mot_ctx* c, const char* who, const mot_scene_judge_params* p, int class_mask, int frame) {
  if (!p) return fail(c, MOT_E_ARG, who, ": null params");
  if (p->min_static_hits < 1u || p->min_static_hits > 0x80000000u) return fail(c, MOT_E_ARG, who, ": min_static_hits must lie in [1, 2^31]");
  if (p->trail_den < 1u || p->trail_den > 65535u || p->trail_num > p->trail_den) return fail(c, MOT_E_ARG, who, ": trail_den must lie in [1, 65535] and trail_num in [0, trail_den]");
  if (class_mask & ~((1 << MOT_SCENE_CLASSES) - 1)) return fail(c, MOT_E_ARG, who, ": unknown class bits");
  if (frame != MOT_FRAME_GLOBAL && frame != MOT_FRAME_SENSOR) return fail(c, MOT_E_ARG, who, ": frame must be MOT_FRAME_GLOBAL or MOT_FRAME_SENSOR");
  return MOT_OK;
}
// the scratch, at the first call: all of its blocks or none (a failure leaves the live allocations as they were; the next call tries again)
static int ensure_judge(mot_ctx* c, bool host_stage) {
  c->sj_chunks = (c->cap + kSceneChunk - 1) / kSceneChunk;
  if (!c->d_sj_cls || !c->d_sj_rows || !c->d_sj_args) {
    int rc = dev_alloc(c, &c->d_sj_cls, (size_t)c->batch * c->cap);
    if (!rc) rc = dev_alloc(c, &c->d_sj_rows, (size_t)c->batch * c->sj_chunks * kSceneJudgeRow * sizeof(int));
    if (!rc) rc = dev_alloc(c, &c->d_sj_args, scene_arg_bytes(c));
    if (rc) {
      const std::string why = c->err;
      (void)release(c, &c->d_sj_cls); (void)release(c, &c->d_sj_rows); (void)release(c, &c->d_sj_args);
      c->err = why;
      return rc;
    }
  }
  // [cap records][5 segments, padded to 48 bytes][cap class bytes]
  if (host_stage) MOT_TRY(dev_alloc(c, &c->d_sj_stage, (size_t)c->cap * sizeof(mot_track_point) + 48 + (size_t)c->cap));
  return MOT_OK;
}
// the kernels over slots first .. first + n - 1, block k of the caller's buffers for slot first + k; one launch per run of slots of one cloud layout (for_layout_runs)
static int launch_judge(mot_ctx* c, int first, int n, const mot_scene_judge_params* p, int class_mask, int frame, mot_track_point* d_points, long point_stride,
                        mot_scene_segment* d_segments, uint8_t* d_classes, long class_stride) {
  const EgoTf* d_tf;   // the matrices the slots' boxes took (the cell test needs them in either frame)
  MOT_TRY(send_link_tf(c, &c->sg_ring, c->d_sj_args, first, n, nullptr, &d_tf));
  SceneSplatInput in = scene_input(c, true);
  const SceneJudgeBuffers j = judge_buffers(c, p, class_mask);
  const SceneGridBuffers g = scene_buffers(c);
  for_layout_runs(c, first, n, [&](int k0, int k1, int packed) {
    in.elevated_packed = packed;
    mot_launch_scene_judge(g, in, j, first + k0, k1 - k0, c->max_points, d_tf + k0, frame == MOT_FRAME_GLOBAL, d_points ? d_points + (long)k0 * point_stride : nullptr, point_stride,
                           d_segments + (long)k0 * MOT_SCENE_CLASSES, d_classes ? d_classes + (long)k0 * class_stride : nullptr, class_stride, c->stream);
  });
  MOT_HIP(c, hipGetLastError());
  return MOT_OK;
}

extern "C" int mot_export_scene_points_dev(mot_ctx* c, int batch, const mot_scene_judge_params* p, int class_mask, int frame, mot_track_point* d_points, long point_stride,
                                           mot_scene_segment* d_segments, uint8_t* d_classes, long class_stride) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_export_scene_points_dev";
  MOT_TRY(check_scene_on(c, who));
  MOT_TRY(check_judge_args(c, who, p, class_mask, frame));
  if (!d_segments || batch < 1 || batch > c->batch || point_stride < 0 || class_stride < 0 || (!d_points && (point_stride > 0 || class_mask)) ||
      (((size_t)d_points | (size_t)d_segments) & 3))
    return fail(c, MOT_E_ARG, who, ": bad argument (null segments, batch out of range, a negative stride, null points with a stride or a mask, a block off 4 bytes)");
  for (int b = 0; b < batch; b++) MOT_TRY(check_judge_slot(c, b, who));   // every slot before anything is launched
  MOT_TRY(ensure_judge(c, false));
  return launch_judge(c, 0, batch, p, class_mask, frame, d_points, point_stride, d_segments, d_classes, class_stride);
}

extern "C" int mot_get_scene_points(mot_ctx* c, int slot, const mot_scene_judge_params* p, int class_mask, int frame, mot_track_point* points, int point_capacity, int* n_points,
                                    mot_scene_segment segments[5], uint8_t* classes, int class_capacity, int* n_elevated) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_get_scene_points";
  MOT_TRY(check_scene_on(c, who));
  MOT_TRY(check_judge_args(c, who, p, class_mask, frame));
  if (slot < 0 || slot >= c->batch || point_capacity < 0 || class_capacity < 0 || !n_points || !n_elevated || !segments)
    return fail(c, MOT_E_ARG, who, ": slot or a capacity out of range, or a null count or segment table");
  MOT_TRY(check_judge_slot(c, slot, who));
  MOT_TRY(ensure_judge(c, true));
  // the slot alone into the staging block, with the block's own capacities; what fits the caller's buffers is decided here
  mot_track_point* d_pts = reinterpret_cast<mot_track_point*>(c->d_sj_stage);
  mot_scene_segment* d_seg = reinterpret_cast<mot_scene_segment*>(c->d_sj_stage + (size_t)c->cap * sizeof(mot_track_point));
  uint8_t* d_cls = reinterpret_cast<uint8_t*>(c->d_sj_stage + (size_t)c->cap * sizeof(mot_track_point) + 48);
  MOT_TRY(launch_judge(c, slot, 1, p, class_mask, frame, d_pts, c->cap, d_seg, classes ? d_cls : nullptr, c->cap));
  char* pin;
  MOT_TRY(pinned_scratch(c, 48, &pin));
  MOT_HIP(c, hipMemcpyAsync(pin, d_seg, MOT_SCENE_CLASSES * sizeof(mot_scene_segment), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  const mot_scene_segment* h = reinterpret_cast<const mot_scene_segment*>(pin);
  long ne = 0, np = 0;
  for (int k = 0; k < MOT_SCENE_CLASSES; k++) {
    if (h[k].count < 0 || h[k].count > c->cap) return fail(c, MOT_E_STATE, who, ": inconsistent counts");
    ne += h[k].count;
    if ((class_mask >> k) & 1) np += h[k].count;
  }
  if (ne > c->cap) return fail(c, MOT_E_STATE, who, ": inconsistent counts");
  memcpy(segments, h, MOT_SCENE_CLASSES * sizeof(mot_scene_segment));
  *n_points = (int)np; *n_elevated = (int)ne;
  if (points && np > point_capacity) return fail(c, MOT_E_CAPACITY, "more selected points than the caller's point buffer holds");
  if (classes && ne > class_capacity) return fail(c, MOT_E_CAPACITY, "more elevated points than the caller's class buffer holds");
  if (points && np > 0) MOT_HIP(c, hipMemcpyAsync(points, d_pts, (size_t)np * sizeof(mot_track_point), hipMemcpyDeviceToHost, c->stream));
  if (classes && ne > 0) MOT_HIP(c, hipMemcpyAsync(classes, d_cls, (size_t)ne, hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  return MOT_OK;
}

// ---------------------------------------------------------------------------------------- a recorded drive's points judged against the grid it left (scene_judge_seq.hip)
// Served while Residency::sequence_scene_frames() vouches for the slots and for slot 0's grid: the frames of the latest MOT_SEQ_SCENE call, nothing taken, emptied or
// changed since. The judge's scratch (ensure_judge: sized for max_batch slots) and [max_batch][5] bases of the call's own; all of it or none.
static int check_seq_judge(mot_ctx* c, const char* who, int frames) {
  MOT_TRY(check_links_on(c, who));
  const int held = c->res.sequence_scene_frames();
  if (!held || !c->d_sgs_static)
    return fail(c, MOT_E_STATE, who, ": slots 0 .. frames - 1 are not the frames of the latest mot_sequence_products_dev(MOT_SEQ_SCENE) call with stream 0's grid as that call left it "
                                     "(no such call, or a fused or stage-wise call, a tracker step from outside, a reset, a load or the setter since)");
  if (frames < 1 || frames > held) return fail(c, MOT_E_ARG, who, ": frames must lie in [1, frames of the sequence call]");
  for (int b = 0; b < frames; b++)
    if (!c->res.point_tracks_valid(b) || !c->res.sequence_frame(b) || c->res.elev_packed_at(b) != c->res.elev_packed_at(0))
      return fail(c, MOT_E_STATE, who, ": a slot of the drive no longer holds its frame as the sequence call left it");
  if ((long)frames * c->max_points > 2147483647L) return fail(c, MOT_E_ARG, who, ": frames * max_points exceeds 2^31 - 1 (places are int32)");
  return MOT_OK;
}
static int ensure_seq_judge(mot_ctx* c, bool host_stage) {
  const bool had = c->d_sj_cls && c->d_sj_rows && c->d_sj_args;
  MOT_TRY(ensure_judge(c, false));
  int rc = dev_alloc(c, &c->d_sjs_base, (size_t)c->batch * MOT_SCENE_CLASSES * sizeof(int));
  if (!rc && host_stage) rc = dev_alloc(c, &c->d_sjs_stage, ((size_t)c->batch + 1) * MOT_SCENE_CLASSES * sizeof(mot_scene_segment));
  if (rc) {   // all blocks or none: what this call took goes back (the per-frame judge's blocks stay if they were there before)
    const std::string why = c->err;
    (void)release(c, &c->d_sjs_base); (void)release(c, &c->d_sjs_stage);
    if (!had) { (void)release(c, &c->d_sj_cls); (void)release(c, &c->d_sj_rows); (void)release(c, &c->d_sj_args); }
    c->err = why;
    return rc;
  }
  return MOT_OK;
}
struct SeqJudgeLaunch { SceneSplatInput in; SceneJudgeBuffers j; const EgoTf* d_tf; };
// classify, the two scans and both tables; the matrices the frames' boxes took go ahead of the kernels (the cell test needs them in either frame)
static int launch_seq_judge_count(mot_ctx* c, int frames, const mot_scene_judge_params* p, int class_mask, mot_scene_segment* d_segments, mot_scene_segment* d_totals,
                                  uint8_t* d_classes, long class_stride, SeqJudgeLaunch* L) {
  MOT_TRY(send_link_tf(c, &c->sg_ring, c->d_sj_args, 0, frames, nullptr, &L->d_tf));
  L->in = scene_input(c, false);   // (slot 0's layout is every frame's: check_seq_judge)
  L->j = judge_buffers(c, p, class_mask);
  mot_launch_scene_judge_seq_count(scene_buffers(c), L->in, L->j, seq_scene_buffers(c), c->d_sjs_base, frames, c->max_points, L->d_tf, d_segments, d_totals, d_classes, class_stride, c->stream);
  MOT_HIP(c, hipGetLastError());
  return MOT_OK;
}

extern "C" int mot_export_sequence_scene_points_dev(mot_ctx* c, int frames, const mot_scene_judge_params* p, int class_mask, int frame, mot_track_point* d_points, long point_capacity,
                                                    mot_scene_segment* d_segments, mot_scene_segment* d_totals, uint8_t* d_classes, long class_stride) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_export_sequence_scene_points_dev";
  MOT_TRY(check_scene_on(c, who));
  MOT_TRY(check_judge_args(c, who, p, class_mask, frame));
  if (!d_segments || !d_totals || point_capacity < 0 || class_stride < 0 || (!d_points && (point_capacity > 0 || class_mask)) ||
      (((size_t)d_points | (size_t)d_segments | (size_t)d_totals) & 3))
    return fail(c, MOT_E_ARG, who, ": bad argument (null segments or totals, a negative capacity or stride, null points with a capacity or a mask, a block off 4 bytes)");
  MOT_TRY(check_seq_judge(c, who, frames));
  MOT_TRY(ensure_seq_judge(c, false));
  SeqJudgeLaunch L;
  MOT_TRY(launch_seq_judge_count(c, frames, p, class_mask, d_segments, d_totals, d_classes, class_stride, &L));
  mot_launch_scene_judge_seq_scatter(L.in, L.j, c->d_sjs_base, frames, c->max_points, L.d_tf, frame == MOT_FRAME_GLOBAL, d_points, point_capacity, c->stream);
  MOT_HIP(c, hipGetLastError());
  return MOT_OK;
}

extern "C" int mot_get_sequence_scene_points(mot_ctx* c, int frames, const mot_scene_judge_params* p, int class_mask, int frame, mot_track_point* points, long point_capacity,
                                             long* n_points, mot_scene_segment* segments, mot_scene_segment totals[5], uint8_t* classes, long class_stride) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_get_sequence_scene_points";
  MOT_TRY(check_scene_on(c, who));
  MOT_TRY(check_judge_args(c, who, p, class_mask, frame));
  if (!n_points || !segments || !totals || point_capacity < 0 || class_stride < 0)
    return fail(c, MOT_E_ARG, who, ": a negative capacity or stride, or a null count, segment table or totals");
  MOT_TRY(check_seq_judge(c, who, frames));
  MOT_TRY(ensure_seq_judge(c, true));
  // the counts first (they are always delivered); what fits the caller's buffers is decided here, and the records are scattered into a block of their own size
  const size_t table = ((size_t)frames + 1) * MOT_SCENE_CLASSES * sizeof(mot_scene_segment);
  mot_scene_segment* d_seg = reinterpret_cast<mot_scene_segment*>(c->d_sjs_stage);
  mot_scene_segment* d_tot = d_seg + (size_t)frames * MOT_SCENE_CLASSES;
  SeqJudgeLaunch L;
  MOT_TRY(launch_seq_judge_count(c, frames, p, class_mask, d_seg, d_tot, nullptr, 0, &L));
  char* pin;
  MOT_TRY(pinned_scratch(c, table, &pin));
  MOT_HIP(c, hipMemcpyAsync(pin, d_seg, table, hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  const mot_scene_segment* h = reinterpret_cast<const mot_scene_segment*>(pin);
  const mot_scene_segment* ht = h + (size_t)frames * MOT_SCENE_CLASSES;
  std::vector<long> elevated(frames, 0);
  long np = 0, widest = 0;
  for (int k = 0; k < frames; k++) {
    for (int cc = 0; cc < MOT_SCENE_CLASSES; cc++) {
      const int n = h[k * MOT_SCENE_CLASSES + cc].count;
      if (n < 0 || n > c->cap) return fail(c, MOT_E_STATE, who, ": inconsistent counts");
      elevated[k] += n;
    }
    if (elevated[k] > c->cap) return fail(c, MOT_E_STATE, who, ": inconsistent counts");
    widest = elevated[k] > widest ? elevated[k] : widest;
  }
  for (int cc = 0; cc < MOT_SCENE_CLASSES; cc++)
    if ((class_mask >> cc) & 1) np += ht[cc].count;
  if (np < 0 || np > (long)frames * c->cap) return fail(c, MOT_E_STATE, who, ": inconsistent counts");
  memcpy(segments, h, (size_t)frames * MOT_SCENE_CLASSES * sizeof(mot_scene_segment));
  memcpy(totals, ht, MOT_SCENE_CLASSES * sizeof(mot_scene_segment));
  *n_points = np;
  if (points && np > point_capacity) return fail(c, MOT_E_CAPACITY, "more selected points than the caller's point buffer holds");
  if (classes && widest > class_stride) return fail(c, MOT_E_CAPACITY, "a frame has more elevated points than the caller's class_stride");
  if (points && np > 0) {   // a block of this call's own, as large as the records (a getter's convenience: the export is the hot path)
    mot_track_point* d_pts = nullptr;
    MOT_TRY(dev_alloc(c, &d_pts, (size_t)np * sizeof(mot_track_point)));
    mot_launch_scene_judge_seq_scatter(L.in, L.j, c->d_sjs_base, frames, c->max_points, L.d_tf, frame == MOT_FRAME_GLOBAL, d_pts, np, c->stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(points, d_pts, (size_t)np * sizeof(mot_track_point), hipMemcpyDeviceToHost, c->stream);
    const hipError_t e2 = hipStreamSynchronize(c->stream);
    MOT_TRY(release(c, &d_pts));
    MOT_HIP_AS(c, "mot_get_sequence_scene_points: the records", e != hipSuccess ? e : e2);
  }
  if (classes)   // frame k's class bytes from where the classify kernel left them, as many as the frame has points
    for (int k = 0; k < frames; k++)
      if (elevated[k] > 0) MOT_HIP(c, hipMemcpyAsync(classes + (size_t)k * class_stride, c->d_sj_cls + (size_t)k * c->cap, (size_t)elevated[k], hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  return MOT_OK;
}

// ---------------------------------------------------------------------------------------- the drive's static map thinned to a voxel grid (scene_voxels_seq.hip)
// The validity, the scratch and the count launches are the drive judge's (above); ONE block of this feature's own, laid out by mot_scene_voxel_scratch_bytes for the
// largest record_capacity asked so far. Growing it drains the stream first (nothing may still read the old block). All of the scratch or none.
static int check_voxel_args(mot_ctx* c, const char* who, const mot_voxel_params* v, long record_capacity, long voxel_capacity) {
  if (!v) return fail(c, MOT_E_ARG, who, ": null voxel params");
  const float leaf[3] = {v->leaf_x, v->leaf_y, v->leaf_z};
  for (float l : leaf)
    if (!(l >= 1e-2f && l <= 1e3f)) return fail(c, MOT_E_ARG, who, ": every leaf must be finite and in [1e-2, 1e3] metres");   // (NaN fails both compares)
  if (v->min_points < 1 || v->min_points > (1 << 30)) return fail(c, MOT_E_ARG, who, ": min_points must lie in [1, 2^30]");
  if (record_capacity < 0 || record_capacity > 2147483647L) return fail(c, MOT_E_ARG, who, ": record_capacity must lie in [0, 2^31 - 1] (positions are int32)");
  if (voxel_capacity < 0) return fail(c, MOT_E_ARG, who, ": negative voxel_capacity");
  return MOT_OK;
}
static int ensure_seq_voxels(mot_ctx* c, long record_capacity, bool host_stage) {
  const bool had_judge = c->d_sj_cls && c->d_sj_rows && c->d_sj_args, had_base = c->d_sjs_base != nullptr, had_stage = c->d_sv_stage != nullptr;
  MOT_TRY(ensure_seq_judge(c, false));
  int rc = MOT_OK;
  bool had_scratch = c->d_sv_scratch != nullptr;   // (a block large enough for this call stays whatever fails behind it)
  if (c->sv_cap < record_capacity) {
    had_scratch = false;
    if (c->d_sv_scratch) {
      MOT_HIP(c, hipStreamSynchronize(c->stream));
      MOT_TRY(release(c, &c->d_sv_scratch));
      c->sv_cap = -1;
    }
    rc = dev_alloc(c, &c->d_sv_scratch, mot_scene_voxel_scratch_bytes(record_capacity, c->batch));
    if (!rc) c->sv_cap = record_capacity;
  }
  if (!rc && host_stage) rc = dev_alloc(c, &c->d_sv_stage, 96);
  if (rc) {   // all blocks or none: what this call took goes back
    const std::string why = c->err;
    if (!had_scratch) { (void)release(c, &c->d_sv_scratch); c->sv_cap = -1; }
    if (!had_stage) (void)release(c, &c->d_sv_stage);
    if (!had_base) (void)release(c, &c->d_sjs_base);
    if (!had_judge) { (void)release(c, &c->d_sj_cls); (void)release(c, &c->d_sj_rows); (void)release(c, &c->d_sj_args); }
    c->err = why;
    return rc;
  }
  return MOT_OK;
}
static SceneVoxelBuffers voxel_buffers(const mot_ctx* c, long record_capacity) {
  SceneVoxelBuffers v;
  (void)mot_scene_voxel_scratch_bytes(c->sv_cap, c->batch, &v, c->d_sv_scratch);
  v.cap = (int)record_capacity;
  v.tiles = (int)((record_capacity + 2047) / 2048); if (v.tiles < 1) v.tiles = 1;
  return v;
}
// the judge's count launches into the scratch's two tables, then the keys, the sort, the runs and the header
static int launch_seq_voxels_count(mot_ctx* c, int frames, const mot_scene_judge_params* p, int class_mask, const mot_voxel_params* vp, const SceneVoxelBuffers& v,
                                   long voxel_capacity, mot_scene_voxel_header* d_header, mot_scene_segment* d_totals) {
  SeqJudgeLaunch L;
  mot_scene_segment* tab = const_cast<mot_scene_segment*>(v.tab);
  MOT_TRY(launch_seq_judge_count(c, frames, p, class_mask, tab, tab + (size_t)frames * MOT_SCENE_CLASSES, nullptr, 0, &L));
  const SceneVoxelArgs a = {1.0f / vp->leaf_x, 1.0f / vp->leaf_y, 1.0f / vp->leaf_z, vp->min_points};
  mot_launch_scene_voxels_seq_count(L.in, L.j, c->d_sjs_base, frames, c->max_points, L.d_tf, v, a, voxel_capacity, d_header, d_totals, c->stream);
  MOT_HIP(c, hipGetLastError());
  return MOT_OK;
}

extern "C" int mot_export_sequence_scene_voxels_dev(mot_ctx* c, int frames, const mot_scene_judge_params* p, int class_mask, const mot_voxel_params* voxel, long record_capacity,
                                                    mot_model_voxel* d_voxels, long voxel_capacity, mot_scene_voxel_header* d_header, mot_scene_segment* d_totals) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_export_sequence_scene_voxels_dev";
  MOT_TRY(check_scene_on(c, who));
  MOT_TRY(check_judge_args(c, who, p, class_mask, MOT_FRAME_GLOBAL));
  MOT_TRY(check_voxel_args(c, who, voxel, record_capacity, voxel_capacity));
  if (!d_header || (!d_voxels && voxel_capacity > 0) || ((size_t)d_voxels & 15) || (((size_t)d_header | (size_t)d_totals) & 3))
    return fail(c, MOT_E_ARG, who, ": bad argument (null header, null voxels with a capacity, voxels off 16 bytes, header or totals off 4 bytes)");
  MOT_TRY(check_seq_judge(c, who, frames));
  MOT_TRY(ensure_seq_voxels(c, record_capacity, false));
  const SceneVoxelBuffers v = voxel_buffers(c, record_capacity);
  MOT_TRY(launch_seq_voxels_count(c, frames, p, class_mask, voxel, v, voxel_capacity, d_header, d_totals));
  mot_launch_scene_voxels_seq_write(v, d_voxels, voxel_capacity, c->stream);
  MOT_HIP(c, hipGetLastError());
  return MOT_OK;
}

extern "C" int mot_get_sequence_scene_voxels(mot_ctx* c, int frames, const mot_scene_judge_params* p, int class_mask, const mot_voxel_params* voxel, long record_capacity,
                                             mot_model_voxel* voxels, long voxel_capacity, long* n_voxels, mot_scene_voxel_header* header, mot_scene_segment totals[5]) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_get_sequence_scene_voxels";
  MOT_TRY(check_scene_on(c, who));
  MOT_TRY(check_judge_args(c, who, p, class_mask, MOT_FRAME_GLOBAL));
  MOT_TRY(check_voxel_args(c, who, voxel, record_capacity, voxel_capacity));
  if (!n_voxels || !header) return fail(c, MOT_E_ARG, who, ": null count or header");
  MOT_TRY(check_seq_judge(c, who, frames));
  MOT_TRY(ensure_seq_voxels(c, record_capacity, true));
  const SceneVoxelBuffers v = voxel_buffers(c, record_capacity);
  // the counts first (they are always delivered); what fits the caller's buffer is decided here, and the voxels are written into a block of their own size
  mot_scene_voxel_header* d_hdr = reinterpret_cast<mot_scene_voxel_header*>(c->d_sv_stage);
  mot_scene_segment* d_tot = reinterpret_cast<mot_scene_segment*>(c->d_sv_stage + sizeof(mot_scene_voxel_header));
  const size_t table = sizeof(mot_scene_voxel_header) + MOT_SCENE_CLASSES * sizeof(mot_scene_segment);
  MOT_TRY(launch_seq_voxels_count(c, frames, p, class_mask, voxel, v, voxel_capacity, d_hdr, d_tot));
  char* pin;
  MOT_TRY(pinned_scratch(c, table, &pin));
  MOT_HIP(c, hipMemcpyAsync(pin, d_hdr, table, hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  const mot_scene_voxel_header* h = reinterpret_cast<const mot_scene_voxel_header*>(pin);
  const long nv = h->n_voxels;
  if (nv < 0 || nv > record_capacity || h->n_records < 0) return fail(c, MOT_E_STATE, who, ": inconsistent counts");
  memcpy(header, h, sizeof(mot_scene_voxel_header));
  header->n_stored = (voxels && nv <= voxel_capacity) ? (int32_t)nv : 0;   // what this call copies to the caller: all of the voxels or none
  if (totals) memcpy(totals, pin + sizeof(mot_scene_voxel_header), MOT_SCENE_CLASSES * sizeof(mot_scene_segment));
  *n_voxels = nv;
  if (voxels && nv > voxel_capacity) return fail(c, MOT_E_CAPACITY, "more voxels than the caller's buffer holds");
  if (voxels && nv > 0) {   // a block of this call's own, as large as the voxels (a getter's convenience: the export is the hot path)
    mot_model_voxel* d_vox = nullptr;
    MOT_TRY(dev_alloc(c, &d_vox, (size_t)nv * sizeof(mot_model_voxel)));
    mot_launch_scene_voxels_seq_write(v, d_vox, nv, c->stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(voxels, d_vox, (size_t)nv * sizeof(mot_model_voxel), hipMemcpyDeviceToHost, c->stream);
    const hipError_t e2 = hipStreamSynchronize(c->stream);
    MOT_TRY(release(c, &d_vox));
    MOT_HIP_AS(c, "mot_get_sequence_scene_voxels: the voxels", e != hipSuccess ? e : e2);
  }
  return MOT_OK;
}

// ---------------------------------------------------------------------------------------- voxel maps merged into one (voxel_merge.hip)
// The calls read nothing but their arguments: no state check, no slot, no step counter, no grid. ONE block of the feature's own, laid out by
// mot_voxel_merge_scratch_bytes for the largest sum of capacities asked so far and released by mot_destroy alone (it does not go with the grid: the calls work
// without one). Growing it drains the stream first (nothing may still read the old block).
static bool blocks_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return a && b && a_bytes && b_bytes && pa < pb + b_bytes && pb < pa + a_bytes;
}
// what the device call and the host call refuse alike; *total: the sum of the capacities
static int check_merge_args(mot_ctx* c, const char* who, const mot_voxel_map_src* maps, int n_maps, const mot_voxel_params* voxel, const void* out, long out_capacity, long* total) {
  if (!maps) return fail(c, MOT_E_ARG, who, ": null maps");
  if (n_maps < 1 || n_maps > MOT_VOXEL_MERGE_MAX_MAPS) return fail(c, MOT_E_ARG, who, ": n_maps must lie in [1, 16]");
  MOT_TRY(check_voxel_args(c, who, voxel, 0, out_capacity));
  long sum = 0;
  for (int k = 0; k < n_maps; k++) {
    const long cap = maps[k].capacity;
    if (cap < 0 || cap > 2147483647L) return fail(c, MOT_E_ARG, who, ": a map's capacity must lie in [0, 2^31 - 1]");
    sum += cap;
    if (sum > 2147483647L) return fail(c, MOT_E_ARG, who, ": the capacities add up to more than 2^31 - 1 (positions are int32)");
    if (!maps[k].voxels && cap > 0) return fail(c, MOT_E_ARG, who, ": null voxels with a capacity");
  }
  if (!out && out_capacity > 0) return fail(c, MOT_E_ARG, who, ": null output block with a capacity");
  *total = sum;
  return MOT_OK;
}
static int ensure_merge_scratch(mot_ctx* c, long total) {
  if (c->d_vm_scratch && c->vm_cap >= total) return MOT_OK;
  if (c->d_vm_scratch) {
    MOT_HIP(c, hipStreamSynchronize(c->stream));
    MOT_TRY(release(c, &c->d_vm_scratch));
  }
  c->vm_cap = -1;
  MOT_TRY(dev_alloc(c, &c->d_vm_scratch, mot_voxel_merge_scratch_bytes(total)));
  c->vm_cap = total;
  return MOT_OK;
}
static SceneVoxelBuffers merge_buffers(const mot_ctx* c, long total) {
  SceneVoxelBuffers v;
  (void)mot_voxel_merge_scratch_bytes(c->vm_cap, &v, c->d_vm_scratch);
  v.cap = (int)total;
  v.tiles = (int)((total + 2047) / 2048); if (v.tiles < 1) v.tiles = 1;
  return v;
}
static SceneVoxelArgs merge_args(const mot_voxel_params* vp) { return {1.0f / vp->leaf_x, 1.0f / vp->leaf_y, 1.0f / vp->leaf_z, vp->min_points}; }

extern "C" int mot_merge_voxel_maps_dev(mot_ctx* c, const mot_voxel_map_src* maps, int n_maps, const mot_voxel_params* voxel, mot_model_voxel* d_out, long out_capacity,
                                        mot_voxel_merge_header* d_header) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_merge_voxel_maps_dev";
  long total = 0;
  MOT_TRY(check_merge_args(c, who, maps, n_maps, voxel, d_out, out_capacity, &total));
  if (!d_header) return fail(c, MOT_E_ARG, who, ": null header");
  if (((size_t)d_out & 15) || ((size_t)d_header & 3)) return fail(c, MOT_E_ARG, who, ": the output block off 16 bytes or the header off 4 bytes");
  const size_t out_bytes = (size_t)(out_capacity > 2147483647L ? 2147483647L : out_capacity) * sizeof(mot_model_voxel);
  VoxelMergeMaps m = {};
  for (int k = 0; k < n_maps; k++) {
    const size_t in_bytes = (size_t)maps[k].capacity * sizeof(mot_model_voxel);
    if (((size_t)maps[k].voxels & 15) || ((size_t)maps[k].count & 3)) return fail(c, MOT_E_ARG, who, ": an input block off 16 bytes or a count off 4 bytes");
    if (blocks_overlap(d_out, out_bytes, maps[k].voxels, in_bytes) || blocks_overlap(d_out, out_bytes, maps[k].count, 4) ||
        blocks_overlap(d_header, sizeof(mot_voxel_merge_header), maps[k].voxels, in_bytes) || blocks_overlap(d_header, sizeof(mot_voxel_merge_header), maps[k].count, 4))
      return fail(c, MOT_E_ARG, who, ": the output block or the header overlaps an input block or a count");
    m.vox[k] = maps[k].voxels; m.count[k] = maps[k].count; m.cap[k] = (int)maps[k].capacity;
  }
  m.n_maps = n_maps; m.short_max = c->vm_short_max;
  MOT_TRY(ensure_merge_scratch(c, total));
  const SceneVoxelBuffers v = merge_buffers(c, total);
  mot_launch_voxel_merge_count(m, v, merge_args(voxel), out_capacity, d_header, c->stream);
  mot_launch_voxel_merge_write(m, v, voxel->min_points, d_out, out_capacity, c->stream);
  MOT_HIP(c, hipGetLastError());
  return MOT_OK;
}

// the host call's device blocks live for the duration of the call: whatever way it ends, the stream is drained and they go back
struct MergeCallBlocks {
  mot_ctx* c; char* stage = nullptr; mot_model_voxel* vox = nullptr;
  explicit MergeCallBlocks(mot_ctx* ctx) : c(ctx) {}
  ~MergeCallBlocks() {
    if (!stage && !vox) return;
    const std::string why = c->err;
    (void)hipStreamSynchronize(c->stream); (void)release(c, &stage); (void)release(c, &vox);
    c->err = why;
  }
};
extern "C" int mot_merge_voxel_maps(mot_ctx* c, const mot_voxel_map_src* maps, int n_maps, const mot_voxel_params* voxel, mot_model_voxel* out, long out_capacity, long* n_voxels,
                                    mot_voxel_merge_header* header) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_merge_voxel_maps";
  long total = 0;
  MOT_TRY(check_merge_args(c, who, maps, n_maps, voxel, out, out_capacity, &total));
  if (!n_voxels || !header) return fail(c, MOT_E_ARG, who, ": null count or header");
  long cnt[MOT_VOXEL_MERGE_MAX_MAPS];
  total = 0;
  for (int k = 0; k < n_maps; k++) {   // the counts are the host's: clamped here, and only those voxels travel
    const long v = maps[k].count ? (long)*maps[k].count : maps[k].capacity;
    cnt[k] = v < 0 ? 0 : (v > maps[k].capacity ? maps[k].capacity : v);
    total += cnt[k];
  }
  // the inputs back to back, then the header: one block; the scratch behind it — all of the call's blocks or none
  const bool had_scratch = c->d_vm_scratch && c->vm_cap >= total;
  MergeCallBlocks blk(c);
  const size_t in_bytes = (size_t)(total < 1 ? 1 : total) * sizeof(mot_model_voxel);
  MOT_TRY(dev_alloc(c, &blk.stage, in_bytes + sizeof(mot_voxel_merge_header)));
  int rc = ensure_merge_scratch(c, total);
  if (rc) return rc;
  mot_voxel_merge_header* d_hdr = reinterpret_cast<mot_voxel_merge_header*>(blk.stage + in_bytes);
  VoxelMergeMaps m = {};
  long at = 0;
  for (int k = 0; k < n_maps; k++) {
    m.vox[k] = reinterpret_cast<const mot_model_voxel*>(blk.stage) + at; m.count[k] = nullptr; m.cap[k] = (int)cnt[k];
    if (cnt[k] > 0) MOT_HIP(c, hipMemcpyAsync(blk.stage + (size_t)at * sizeof(mot_model_voxel), maps[k].voxels, (size_t)cnt[k] * sizeof(mot_model_voxel), hipMemcpyHostToDevice, c->stream));
    at += cnt[k];
  }
  m.n_maps = n_maps; m.short_max = c->vm_short_max;
  const SceneVoxelBuffers v = merge_buffers(c, total);
  // the counts first (they are always delivered); what fits the caller's buffer is decided here, and the voxels are written into a block of their own size
  mot_launch_voxel_merge_count(m, v, merge_args(voxel), out_capacity, d_hdr, c->stream);
  MOT_HIP(c, hipGetLastError());
  char* pin;
  MOT_TRY(pinned_scratch(c, sizeof(mot_voxel_merge_header), &pin));
  MOT_HIP(c, hipMemcpyAsync(pin, d_hdr, sizeof(mot_voxel_merge_header), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  const mot_voxel_merge_header* h = reinterpret_cast<const mot_voxel_merge_header*>(pin);
  const long nv = h->n_voxels;
  if (nv < 0 || nv > total || h->n_inputs != total) return fail(c, MOT_E_STATE, who, ": inconsistent counts");
  memcpy(header, h, sizeof(mot_voxel_merge_header));
  header->n_stored = (out && nv <= out_capacity) ? (int32_t)nv : 0;   // what this call copies to the caller: all of the voxels or none
  *n_voxels = nv;
  if (out && nv > out_capacity) return fail(c, MOT_E_CAPACITY, "more voxels than the caller's buffer holds");
  if (out && nv > 0) {
    rc = dev_alloc(c, &blk.vox, (size_t)nv * sizeof(mot_model_voxel));
    if (rc) {
      if (!had_scratch) { const std::string why = c->err; (void)release(c, &c->d_vm_scratch); c->vm_cap = -1; c->err = why; }
      return rc;
    }
    mot_launch_voxel_merge_write(m, v, voxel->min_points, blk.vox, nv, c->stream);
    MOT_HIP(c, hipGetLastError());
    MOT_HIP(c, hipMemcpyAsync(out, blk.vox, (size_t)nv * sizeof(mot_model_voxel), hipMemcpyDeviceToHost, c->stream));
    MOT_HIP(c, hipStreamSynchronize(c->stream));
  }
  return MOT_OK;
}

// ---------------------------------------------------------------------------------------- voxel maps indexed (voxel_merge.hip: the merge's count launches, one write launch)
// The merge's argument checks, scratch block and launches; the descriptor's three blocks are read in place of d_out and d_header.
struct IndexBlock { const void* p; size_t bytes; };
static void index_blocks(const mot_voxel_index* x, IndexBlock (&blk)[3]) {
  const size_t cap = (size_t)(x->capacity < 0 ? 0 : x->capacity);
  blk[0] = {x->keys, cap * sizeof(uint64_t)}; blk[1] = {x->counts, cap * sizeof(int32_t)}; blk[2] = {x->header, sizeof(mot_voxel_merge_header)};
}
// what the index call and the judge refuse alike of a descriptor's blocks
static int check_index_blocks(mot_ctx* c, const char* who, const mot_voxel_index* x) {
  if (!x) return fail(c, MOT_E_ARG, who, ": null index");
  if (!x->header) return fail(c, MOT_E_ARG, who, ": null index header");
  if (x->capacity < 0 || x->capacity > 2147483647L) return fail(c, MOT_E_ARG, who, ": the index capacity must lie in [0, 2^31 - 1]");
  if ((!x->keys || !x->counts) && x->capacity > 0) return fail(c, MOT_E_ARG, who, ": null index keys or counts with a capacity");
  if (((size_t)x->keys & 7) || (((size_t)x->counts | (size_t)x->header) & 3)) return fail(c, MOT_E_ARG, who, ": index keys off 8 bytes, or counts or header off 4 bytes");
  return MOT_OK;
}

extern "C" int mot_index_voxel_maps_dev(mot_ctx* c, const mot_voxel_map_src* maps, int n_maps, const mot_voxel_params* voxel, mot_voxel_index* index) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_index_voxel_maps_dev";
  MOT_TRY(check_index_blocks(c, who, index));
  long total = 0;
  MOT_TRY(check_merge_args(c, who, maps, n_maps, voxel, index->keys, index->capacity, &total));
  IndexBlock blk[3];
  index_blocks(index, blk);
  for (int a = 0; a < 3; a++)
    for (int b = a + 1; b < 3; b++)
      if (blocks_overlap(blk[a].p, blk[a].bytes, blk[b].p, blk[b].bytes)) return fail(c, MOT_E_ARG, who, ": the index's keys, counts and header overlap each other");
  VoxelMergeMaps m = {};
  for (int k = 0; k < n_maps; k++) {
    const size_t in_bytes = (size_t)maps[k].capacity * sizeof(mot_model_voxel);
    if (((size_t)maps[k].voxels & 15) || ((size_t)maps[k].count & 3)) return fail(c, MOT_E_ARG, who, ": an input block off 16 bytes or a count off 4 bytes");
    for (const IndexBlock& o : blk)
      if (blocks_overlap(o.p, o.bytes, maps[k].voxels, in_bytes) || blocks_overlap(o.p, o.bytes, maps[k].count, 4))
        return fail(c, MOT_E_ARG, who, ": an index block overlaps an input block or a count");
    m.vox[k] = maps[k].voxels; m.count[k] = maps[k].count; m.cap[k] = (int)maps[k].capacity;
  }
  m.n_maps = n_maps; m.short_max = c->vm_short_max;
  MOT_TRY(ensure_merge_scratch(c, total));
  const SceneVoxelBuffers v = merge_buffers(c, total);
  mot_launch_voxel_merge_count(m, v, merge_args(voxel), index->capacity, index->header, c->stream);
  mot_launch_voxel_merge_index(m, v, reinterpret_cast<unsigned long long*>(index->keys), index->counts, index->capacity, c->stream);
  MOT_HIP(c, hipGetLastError());
  index->leaf_x = voxel->leaf_x; index->leaf_y = voxel->leaf_y; index->leaf_z = voxel->leaf_z; index->reserved = 0;
  return MOT_OK;
}

// ---------------------------------------------------------------------------------------- a frame's points judged against a voxel index (map_judge.hip)
// The validity of check_point_tracks, sequence slots refused; the grid is neither required nor read. The scratch and the ring are the calls' own (the scene judge's
// go with the grid): taken at the first call, all or none, released by mot_destroy alone.
static int check_map_judge_args(mot_ctx* c, const char* who, const mot_voxel_index* x, const mot_map_judge_params* p, int class_mask, int frame) {
  MOT_TRY(check_index_blocks(c, who, x));
  if (!p) return fail(c, MOT_E_ARG, who, ": null params");
  const float leaf[3] = {x->leaf_x, x->leaf_y, x->leaf_z};
  for (float l : leaf)
    if (!(l >= 1e-2f && l <= 1e3f)) return fail(c, MOT_E_ARG, who, ": every leaf of the index must be finite and in [1e-2, 1e3] metres (mot_index_voxel_maps_dev writes it)");
  if (p->min_count < 1) return fail(c, MOT_E_ARG, who, ": min_count must lie in [1, 2^31 - 1]");
  if (p->reach != 0 && p->reach != 1) return fail(c, MOT_E_ARG, who, ": reach must be 0 or 1");
  if (class_mask & ~((1 << MOT_MAP_CLASSES) - 1)) return fail(c, MOT_E_ARG, who, ": unknown class bits");
  if (frame != MOT_FRAME_GLOBAL && frame != MOT_FRAME_SENSOR) return fail(c, MOT_E_ARG, who, ": frame must be MOT_FRAME_GLOBAL or MOT_FRAME_SENSOR");
  return MOT_OK;
}
static int check_map_judge_slot(mot_ctx* c, int b, const char* who) {
  MOT_TRY(check_point_tracks(c, b, who));
  if (c->res.sequence_frame(b)) return fail(c, MOT_E_STATE, who, ": the slots hold the frames of ONE stream (mot_sequence_dev)");
  return MOT_OK;
}
static int ensure_map_judge(mot_ctx* c, bool host_stage) {
  c->mj_chunks = (c->cap + kSceneChunk - 1) / kSceneChunk;
  if (!c->d_mj_cls || !c->d_mj_rows || !c->d_mj_args || !c->mj_ring.base) {
    int rc = dev_alloc(c, &c->d_mj_cls, (size_t)c->batch * c->cap);
    if (!rc) rc = dev_alloc(c, &c->d_mj_rows, (size_t)c->batch * c->mj_chunks * kSceneJudgeRow * sizeof(int));
    if (!rc) rc = dev_alloc(c, &c->d_mj_args, (size_t)c->batch * sizeof(EgoTf));
    if (!rc) rc = c->mj_ring.create(c, (size_t)c->batch * sizeof(EgoTf));   // (skips what exists; the ring's events stay in the registry, as those of every ring do)
    if (rc) {
      const std::string why = c->err;
      (void)release(c, &c->d_mj_cls); (void)release(c, &c->d_mj_rows); (void)release(c, &c->d_mj_args); (void)release(c, &c->mj_ring.base);
      c->err = why;
      return rc;
    }
  }
  // [cap records][5 segments, padded to 48 bytes][cap class bytes]
  if (host_stage) MOT_TRY(dev_alloc(c, &c->d_mj_stage, (size_t)c->cap * sizeof(mot_track_point) + 48 + (size_t)c->cap));
  return MOT_OK;
}
static int launch_map_judge(mot_ctx* c, int first, int n, const mot_voxel_index* x, const mot_map_judge_params* p, int class_mask, int frame, mot_track_point* d_points,
                            long point_stride, mot_scene_segment* d_segments, uint8_t* d_classes, long class_stride) {
  const EgoTf* d_tf;   // the matrices the slots' boxes took (the cell test needs them in either frame)
  MOT_TRY(send_link_tf(c, &c->mj_ring, c->d_mj_args, first, n, nullptr, &d_tf));
  SceneSplatInput in = scene_input(c, true);
  SceneJudgeBuffers j = {};
  j.cls = c->d_mj_cls; j.rows = c->d_mj_rows; j.max_chunks = c->mj_chunks; j.class_mask = class_mask;
  MapJudgeIndex ix;
  ix.keys = reinterpret_cast<const unsigned long long*>(x->keys); ix.counts = x->counts; ix.n_stored = &x->header->n_stored; ix.capacity = (int)x->capacity;
  ix.a = {1.0f / x->leaf_x, 1.0f / x->leaf_y, 1.0f / x->leaf_z, 1};
  ix.min_count = p->min_count; ix.reach = p->reach;
  for_layout_runs(c, first, n, [&](int k0, int k1, int packed) {
    in.elevated_packed = packed;
    mot_launch_map_judge(in, j, ix, first + k0, k1 - k0, c->max_points, d_tf + k0, frame == MOT_FRAME_GLOBAL, d_points ? d_points + (long)k0 * point_stride : nullptr, point_stride,
                         d_segments + (long)k0 * MOT_MAP_CLASSES, d_classes ? d_classes + (long)k0 * class_stride : nullptr, class_stride, c->stream);
  });
  MOT_HIP(c, hipGetLastError());
  return MOT_OK;
}

extern "C" int mot_export_map_points_dev(mot_ctx* c, int batch, const mot_voxel_index* index, const mot_map_judge_params* p, int class_mask, int frame, mot_track_point* d_points,
                                         long point_stride, mot_scene_segment* d_segments, uint8_t* d_classes, long class_stride) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_export_map_points_dev";
  MOT_TRY(check_map_judge_args(c, who, index, p, class_mask, frame));
  if (!d_segments || batch < 1 || batch > c->batch || point_stride < 0 || class_stride < 0 || (!d_points && (point_stride > 0 || class_mask)) ||
      (((size_t)d_points | (size_t)d_segments) & 3))
    return fail(c, MOT_E_ARG, who, ": bad argument (null segments, batch out of range, a negative stride, null points with a stride or a mask, a block off 4 bytes)");
  IndexBlock blk[3];
  index_blocks(index, blk);
  const IndexBlock out[3] = {{d_points, (size_t)batch * (size_t)point_stride * sizeof(mot_track_point)}, {d_segments, (size_t)batch * MOT_MAP_CLASSES * sizeof(mot_scene_segment)},
                             {d_classes, (size_t)batch * (size_t)class_stride}};
  for (const IndexBlock& o : out)
    for (const IndexBlock& i : blk)
      if (blocks_overlap(o.p, o.bytes, i.p, i.bytes)) return fail(c, MOT_E_ARG, who, ": an output block overlaps a block of the index");
  for (int b = 0; b < batch; b++) MOT_TRY(check_map_judge_slot(c, b, who));   // every slot before anything is launched
  MOT_TRY(ensure_map_judge(c, false));
  return launch_map_judge(c, 0, batch, index, p, class_mask, frame, d_points, point_stride, d_segments, d_classes, class_stride);
}

extern "C" int mot_get_map_points(mot_ctx* c, int slot, const mot_voxel_index* index, const mot_map_judge_params* p, int class_mask, int frame, mot_track_point* points,
                                  int point_capacity, int* n_points, mot_scene_segment segments[5], uint8_t* classes, int class_capacity, int* n_elevated) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_get_map_points";
  MOT_TRY(check_map_judge_args(c, who, index, p, class_mask, frame));
  if (slot < 0 || slot >= c->batch || point_capacity < 0 || class_capacity < 0 || !n_points || !n_elevated || !segments)
    return fail(c, MOT_E_ARG, who, ": slot or a capacity out of range, or a null count or segment table");
  MOT_TRY(check_map_judge_slot(c, slot, who));
  MOT_TRY(ensure_map_judge(c, true));
  // the slot alone into the staging block, with the block's own capacities; what fits the caller's buffers is decided here
  mot_track_point* d_pts = reinterpret_cast<mot_track_point*>(c->d_mj_stage);
  mot_scene_segment* d_seg = reinterpret_cast<mot_scene_segment*>(c->d_mj_stage + (size_t)c->cap * sizeof(mot_track_point));
  uint8_t* d_cls = reinterpret_cast<uint8_t*>(c->d_mj_stage + (size_t)c->cap * sizeof(mot_track_point) + 48);
  MOT_TRY(launch_map_judge(c, slot, 1, index, p, class_mask, frame, d_pts, c->cap, d_seg, classes ? d_cls : nullptr, c->cap));
  char* pin;
  MOT_TRY(pinned_scratch(c, 48, &pin));
  MOT_HIP(c, hipMemcpyAsync(pin, d_seg, MOT_MAP_CLASSES * sizeof(mot_scene_segment), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  const mot_scene_segment* h = reinterpret_cast<const mot_scene_segment*>(pin);
  long ne = 0, np = 0;
  for (int k = 0; k < MOT_MAP_CLASSES; k++) {
    if (h[k].count < 0 || h[k].count > c->cap) return fail(c, MOT_E_STATE, who, ": inconsistent counts");
    ne += h[k].count;
    if ((class_mask >> k) & 1) np += h[k].count;
  }
  if (ne > c->cap) return fail(c, MOT_E_STATE, who, ": inconsistent counts");
  memcpy(segments, h, MOT_MAP_CLASSES * sizeof(mot_scene_segment));
  *n_points = (int)np; *n_elevated = (int)ne;
  if (points && np > point_capacity) return fail(c, MOT_E_CAPACITY, "more selected points than the caller's point buffer holds");
  if (classes && ne > class_capacity) return fail(c, MOT_E_CAPACITY, "more elevated points than the caller's class buffer holds");
  if (points && np > 0) MOT_HIP(c, hipMemcpyAsync(points, d_pts, (size_t)np * sizeof(mot_track_point), hipMemcpyDeviceToHost, c->stream));
  if (classes && ne > 0) MOT_HIP(c, hipMemcpyAsync(classes, d_cls, (size_t)ne, hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  return MOT_OK;
}

extern "C" int mot_debug_voxel_merge_cut(mot_ctx* c, int short_max) {
  if (!c || short_max < 0 || short_max > 64) return MOT_E_ARG;
  c->vm_short_max = short_max;
  return MOT_OK;
}
