// mot_api.hip — host side of the C-ABI declared in include/mot.h. Product code: the context's life cycle and the owner of everything it allocates, the setters, the fused launch
// sequence and the ingest paths. (The stage-wise calls and getters: mot_api_stages.hip; tracker, exports, snapshots: mot_api_tracks.hip; the RCCL gather: mot_gather.hip; what
// they share: mot_host.h.) There is no CPU fallback: mot_create() fails with MOT_E_HIP when no HIP device is present.
#include "mot_host.h"
#ifndef MOT_HIPEMU
#include <dlfcn.h>
#endif

#include <algorithm>
#include <cmath>
#include <mutex>
#include <random>

extern "C" int mot_abi_version(void) { return MOT_ABI_VERSION; }

// constants of the two reference packages; file:line in include/mot.h
extern "C" int mot_params_preset(int preset, mot_params* o) {
  if (!o) return MOT_E_ARG;
  if (preset != MOT_PRESET_OBJECT_TRACKING && preset != MOT_PRESET_OBJECT_TRACKING0) return MOT_E_ARG;
  const bool kitti = preset == MOT_PRESET_OBJECT_TRACKING0;
  memset(o, 0, sizeof *o);
  o->r_min = 3.4f; o->r_max = 120.f;
  o->t_hmin = kitti ? -1.9f : -2.0f;
  o->t_hmax = kitti ? -1.0f : -0.4f;
  o->t_hdiff = 0.4f;
  o->h_sensor = kitti ? 1.73f : 2.0f;
  o->ground_margin = 0.25; o->gauss_sigma = 1.0; o->gauss_samples = 3;
  o->crop_enable = 0;
  o->crop_z_min = -3.0f; o->crop_z_max = 1.0f; o->crop_x_min = -15.f; o->crop_x_max = 5.f;
  o->crop_y_min = -50.f; o->crop_y_max = 50.f;
  o->num_grid = kitti ? 200 : 250;
  o->roi_m = kitti ? 30.f : 50.f;
  o->occ_min_count = kitti ? 1 : 2;
  o->dilate = kitti ? 0 : 1;
  o->pic_scale = 900 / o->roi_m;
  o->ram_points = 80;
  o->l_slope_dist = kitti ? 3 : 1;
  o->l_num_points = kitti ? 300 : 5;
  o->lshape_side_cond = kitti ? 0 : 1;
  o->sensor_height = kitti ? 1.73f : 2.0f;
  o->t_height_min = kitti ? 1.0f : 0.8f; o->t_height_max = 2.6f;
  o->t_width_min = kitti ? 0.25f : 0.2f; o->t_width_max = 3.5f;
  o->t_len_min = kitti ? 0.5f : 0.2f; o->t_len_max = 14.0f;
  o->t_area_max = 20.0f;
  o->t_ratio_min = kitti ? 1.3f : 1.0f; o->t_ratio_max = kitti ? 5.0f : 8.0f;
  o->min_len_ratio = 3.0f; o->t_pt_per_m3 = 8.0f;
  o->min_points = kitti ? 100 : 30;
  o->gamma_g = 9.22; o->p_g = 0.99; o->p_d = 0.9;
  o->distance_thres = kitti ? 0.25 : 99.0;
  o->life_time_thres = kitti ? 8 : 3;
  o->seed_box_index = kitti ? 10 : 1;
  o->bb_yaw_change_thres = 0.2;
  o->first_ego_yaw_offset = (kitti ? 1.22191 : -0.63035) - M_PI / 2;
  o->seed_px = -1.5125; o->seed_py = -8.975;
  o->rng_mapping = MOT_RNG_LIBSTDCXX11;
  return MOT_OK;
}

static std::string range_message(const char* field, float lo, float hi) {
  char buf[96];
  snprintf(buf, sizeof buf, "%s must be in %g .. %g m", field, (double)lo, (double)hi);
  return buf;
}

static int make_dev_params(const mot_params& p, MotDevParams* d, std::string* err) {
  if (p.gauss_samples != 3) { *err = "gauss_samples must be 3"; return MOT_E_ARG; }
  if (p.num_grid < 8 || p.num_grid > MOT_MAX_GRID) { *err = "num_grid out of range"; return MOT_E_ARG; }
  if (p.ram_points < 1 || p.ram_points > 128) { *err = "ram_points must be in 1..128"; return MOT_E_ARG; }
  if (p.rng_mapping != MOT_RNG_LIBSTDCXX10 && p.rng_mapping != MOT_RNG_LIBSTDCXX11) { *err = "rng_mapping must be MOT_RNG_LIBSTDCXX10 or MOT_RNG_LIBSTDCXX11"; return MOT_E_ARG; }
  // The declared domain (include/mot.h, "parameter domain"): inside it every stage answers as the reference does, outside it mot_create refuses.
  {
    const struct { const char* name; double v; } reals[] = {
        {"r_min", p.r_min}, {"r_max", p.r_max}, {"t_hmin", p.t_hmin}, {"t_hmax", p.t_hmax}, {"t_hdiff", p.t_hdiff}, {"h_sensor", p.h_sensor},
        {"ground_margin", p.ground_margin}, {"gauss_sigma", p.gauss_sigma}, {"crop_z_min", p.crop_z_min}, {"crop_z_max", p.crop_z_max},
        {"crop_x_min", p.crop_x_min}, {"crop_x_max", p.crop_x_max}, {"crop_y_min", p.crop_y_min}, {"crop_y_max", p.crop_y_max}, {"roi_m", p.roi_m},
        {"pic_scale", p.pic_scale}, {"sensor_height", p.sensor_height}, {"t_height_min", p.t_height_min}, {"t_height_max", p.t_height_max},
        {"t_width_min", p.t_width_min}, {"t_width_max", p.t_width_max}, {"t_len_min", p.t_len_min}, {"t_len_max", p.t_len_max},
        {"t_area_max", p.t_area_max}, {"t_ratio_min", p.t_ratio_min}, {"t_ratio_max", p.t_ratio_max}, {"min_len_ratio", p.min_len_ratio},
        {"t_pt_per_m3", p.t_pt_per_m3}, {"gamma_g", p.gamma_g}, {"p_g", p.p_g}, {"p_d", p.p_d}, {"distance_thres", p.distance_thres},
        {"bb_yaw_change_thres", p.bb_yaw_change_thres}, {"first_ego_yaw_offset", p.first_ego_yaw_offset}, {"seed_px", p.seed_px}, {"seed_py", p.seed_py}};
    for (const auto& f : reals)
      if (!std::isfinite(f.v)) { *err = std::string(f.name) + " must be finite"; return MOT_E_ARG; }
  }
  if (p.occ_min_count != 1 && p.occ_min_count != 2) { *err = "occ_min_count must be 1 or 2"; return MOT_E_ARG; }
  if (p.dilate != 0 && p.dilate != 1) { *err = "dilate must be 0 or 1"; return MOT_E_ARG; }
  if (!(p.gauss_sigma > 0)) { *err = "gauss_sigma must be > 0"; return MOT_E_ARG; }
  if (!(p.roi_m >= MOT_ROI_M_MIN && p.roi_m <= MOT_ROI_M_MAX)) { *err = range_message("roi_m", MOT_ROI_M_MIN, MOT_ROI_M_MAX); return MOT_E_ARG; }
  if (!(p.pic_scale > 0.f)) { *err = "pic_scale must be > 0"; return MOT_E_ARG; }
  if (!(p.pic_scale * p.roi_m <= 1000.f)) { *err = "pic_scale * roi_m must be <= 1000 pixels"; return MOT_E_ARG; }
  if (!(p.r_min >= 0.f)) { *err = "r_min must be >= 0"; return MOT_E_ARG; }
  if (!(p.r_max > p.r_min)) { *err = "r_max must be > r_min"; return MOT_E_ARG; }
  if (!(p.r_max >= MOT_R_MAX_MIN && p.r_max <= MOT_R_MAX_MAX)) { *err = range_message("r_max", MOT_R_MAX_MIN, MOT_R_MAX_MAX); return MOT_E_ARG; }
  // the guarded fast polar bin (kCellGuard, mot_internal.h) is proven for r_max / (r_max - r_min) <= MOT_POLAR_RATIO_MAX only;
  // the test uses the fp32 span the kernels divide by
  if (!(p.r_max <= MOT_POLAR_RATIO_MAX * (p.r_max - p.r_min))) {
    char buf[160];
    snprintf(buf, sizeof buf, "r_max / (r_max - r_min) must be <= %g: polar range too narrow for the guarded cell estimate", (double)MOT_POLAR_RATIO_MAX);
    *err = buf; return MOT_E_ARG;
  }
  memset(d, 0, sizeof *d);
  d->r_min = p.r_min; d->r_max = p.r_max; d->r_span = p.r_max - p.r_min;
  d->k_bin = (float)MOT_NUM_BIN / d->r_span;
  d->t_hmin = p.t_hmin; d->t_hmax = p.t_hmax; d->t_hdiff = p.t_hdiff; d->h_sensor = p.h_sensor;
  d->ground_margin = p.ground_margin;
  {  // gaussKernel(samples=3, sigma), gaus_blur.cpp:26-49 — host libm, exactly as the reference evaluates it
    int samples = p.gauss_samples;
    double sigma = p.gauss_sigma;
    double mean = samples / 2;  // integer division
    double sum = 0.0, k[3];
    for (int x = 0; x < samples; ++x) {
      k[x] = exp(-0.5 * (pow((x - mean) / sigma, 2.0))) / (2 * M_PI * sigma * sigma);
      sum += k[x];
    }
    for (int x = 0; x < samples; ++x) d->gk[x] = k[x] / sum;
  }
  d->crop_enable = p.crop_enable;
  d->crop_z_min = p.crop_z_min; d->crop_z_max = p.crop_z_max; d->crop_x_min = p.crop_x_min;
  d->crop_x_max = p.crop_x_max; d->crop_y_min = p.crop_y_min; d->crop_y_max = p.crop_y_max;
  d->num_grid = p.num_grid; d->occ_min_count = p.occ_min_count; d->dilate = p.dilate;
  d->roi_m = p.roi_m; d->roi_half = p.roi_m / 2;
  d->k_grid = (float)p.num_grid / p.roi_m;
  d->pic_scale = p.pic_scale; d->pic_full = p.pic_scale * p.roi_m; d->pic_half = p.roi_m * p.pic_scale / 2;
  d->rng_mapping = p.rng_mapping;
  d->ram_points = p.ram_points; d->l_slope_dist = p.l_slope_dist; d->l_num_points = p.l_num_points;
  d->lshape_side_cond = p.lshape_side_cond; d->min_points = p.min_points; d->sensor_height = p.sensor_height;
  d->t_height_min = p.t_height_min; d->t_height_max = p.t_height_max; d->t_width_min = p.t_width_min;
  d->t_width_max = p.t_width_max; d->t_len_min = p.t_len_min; d->t_len_max = p.t_len_max;
  d->t_area_max = p.t_area_max; d->t_ratio_min = p.t_ratio_min; d->t_ratio_max = p.t_ratio_max;
  d->min_len_ratio = p.min_len_ratio; d->t_pt_per_m3 = p.t_pt_per_m3;
  return MOT_OK;
}
// ---------------------------------------------------------------------------------------- ownership (mot_host.h)
int own_alloc(mot_ctx* c, void** p, size_t bytes, OwnKind kind, const char* what) {
  if (*p) return MOT_OK;
  std::vector<void*>& list = kind == kOwnPinned ? c->own_pinned : c->own_dev;
  list.reserve(list.size() + 1);   // (so that recording cannot fail once the memory exists)
  void* q = nullptr;
  MOT_HIP_AS(c, what, kind == kOwnPinned ? hipHostMalloc(&q, bytes, hipHostMallocDefault) : hipMalloc(&q, bytes));
  list.push_back(*p = q);
  if (kind == kOwnDevZeroed) MOT_HIP(c, hipMemsetAsync(q, 0, bytes, c->stream));
  return MOT_OK;
}
int own_event(mot_ctx* c, hipEvent_t* ev, unsigned flags, const char* what) {
  if (*ev) return MOT_OK;
  c->own_events.reserve(c->own_events.size() + 1);
  hipEvent_t e = nullptr;
  MOT_HIP_AS(c, what, hipEventCreateWithFlags(&e, flags));
  c->own_events.push_back(*ev = e);
  return MOT_OK;
}
int own_release(mot_ctx* c, void** p) {
  if (!*p) return MOT_OK;
  for (std::vector<void*>* list : {&c->own_dev, &c->own_pinned}) {
    const auto it = std::find(list->begin(), list->end(), *p);
    if (it == list->end()) continue;
    MOT_HIP(c, list == &c->own_dev ? hipFree(*p) : hipHostFree(*p));
    list->erase(it);
  }
  *p = nullptr;
  return MOT_OK;
}
static void destroy_graph(void* exec) {
#ifndef MOT_HIPEMU
  if (exec) (void)hipGraphExecDestroy((hipGraphExec_t)exec);
#endif
}
// captured launch sequences hold the modes they were captured in (tracker mode, point order, track links): a setter that changes one of them drops them all. None is running once
// the stream has drained.
int drop_graphs(mot_ctx* c) {
  if (c->graphs.empty()) return MOT_OK;
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  for (auto& ge : c->graphs) destroy_graph(ge.exec);
  c->graphs.clear();
  return MOT_OK;
}

extern "C" void mot_destroy(mot_ctx* c) {
  if (!c) return;
  MOT_GUARD(c);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
  (void)drop_graphs(c);
  for (hipEvent_t e : c->own_events) (void)hipEventDestroy(e);
  for (void* p : c->own_dev) (void)hipFree(p);
  for (void* p : c->own_pinned) (void)hipHostFree(p);
  if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int PinnedRing::create(mot_ctx* c, size_t bytes_per_block) {
  block_bytes = bytes_per_block;
  MOT_TRY(pinned_alloc(c, &base, block_bytes * kBlocks));
  for (int i = 0; i < kBlocks; i++) MOT_TRY(new_event(c, &ev[i], hipEventDisableTiming));
  return MOT_OK;
}
int PinnedRing::acquire(mot_ctx* c, char** blk) {
  if (used[next]) MOT_HIP(c, hipEventSynchronize(ev[next]));
  *blk = base + (size_t)next * block_bytes;
  return MOT_OK;
}
int PinnedRing::commit(mot_ctx* c, void* dst, size_t src_off, size_t bytes, hipStream_t stream) {
  MOT_HIP(c, hipMemcpyAsync(dst, base + (size_t)next * block_bytes + src_off, bytes, hipMemcpyHostToDevice, stream));
  MOT_HIP(c, hipEventRecord(ev[next], stream));
  used[next] = true;
  next = (next + 1) % kBlocks;
  return MOT_OK;
}

// the next staging block of the argument ring; bytes [off, off + bytes) of it into the device block (stream-ordered: behind every kernel of the previous launch sequence that
// still reads the old values), and the ring moves on
int arg_block_acquire(mot_ctx* c, char** blk) { return c->arg_ring.acquire(c, blk); }
int arg_block_commit(mot_ctx* c, size_t off, size_t bytes) { return c->arg_ring.commit(c, c->d_argblk + off, off, bytes, c->stream); }

// slot < 0: a launch over the whole fused batch just issued (every slot of it has slot 0's layout); otherwise the slot a single-frame launch works on
ClusterBuffers cluster_buffers(mot_ctx* c, int slot) {
  ClusterBuffers b;
  b.elevated = c->d_elev; b.elevated_packed = c->res.elev_packed_at(slot < 0 ? 0 : slot) ? 1 : 0; b.cap = c->cap; b.counts = c->d_counts; b.plane_a = c->d_plane_a; b.plane_b = c->d_plane_b; b.ccl_parent = c->d_ccl_parent;
  b.occ_list = nullptr; b.occ_count = nullptr; b.n_in = c->d_n; b.occ_chunks = c->occ_chunks;   // the fused path points these at the compaction kernel's lists
  b.grid = c->d_grid; b.label = c->d_label; b.stats = c->d_stats; b.cand = c->d_cand; b.boxes = c->d_boxes;
  b.box_cluster = c->d_box_cluster; b.rng = c->d_rng; b.poly = c->d_poly; b.groups = c->d_groups; b.group_cap = c->cap / 2; b.cluster_start = c->d_cluster_start; b.cluster_gstart = c->d_cluster_gstart; b.order = c->d_order; b.gsorted = c->d_gsorted;
  b.pix = c->d_pix; b.wgtab = c->d_wgtab; b.max_wg = c->max_wg;
  b.ecell = nullptr;   // stage-wise: the label kernel computes the cells itself
  b.group_scratch = nullptr;
  return b;
}

// ---------------------------------------------------------------------------------------- MOT_ORDER_ANY
// What the box stage — and every later reader that walks clusters (mot_box_markers) — is handed for a slot whose points were regrouped: the same buffers
// with `elevated`, `ecell` pointing at the cluster-ordered copy, so that pix, first, the groups and cluster_gstart index the copy consistently. The label
// kernel writes no per-point labels there (they would come out in copy order): regroup_label_kernel has written them in input order.
ClusterBuffers regrouped_view(const mot_ctx* c, ClusterBuffers cb) {
  cb.elevated = c->d_rg_xyz; cb.elevated_packed = 1;
  cb.ecell = cb.ecell ? c->d_rg_cell : nullptr;
  cb.label = nullptr;
  if (c->d_rg_groups) { cb.groups = c->d_rg_groups; cb.gsorted = c->d_rg_gsorted; cb.group_scratch = c->d_rg_gscratch; cb.group_cap = c->rg_group_cap; }
  return cb;
}
static RegroupBuffers regroup_buffers(const mot_ctx* c, int* label) {
  RegroupBuffers r;
  r.key = c->d_rg_key; r.tmp = c->d_rg_tmp; r.hist = c->d_rg_hist; r.xyz = c->d_rg_xyz; r.cell = c->d_rg_cell; r.label = label;
  return r;
}
// a reader's view of a slot's box-stage products, whichever mode produced them (the mode may have been switched since)
ClusterBuffers box_products(mot_ctx* c, int slot) {
  ClusterBuffers cb = cluster_buffers(c, slot);
  return c->res.regrouped(slot) ? regrouped_view(c, cb) : cb;
}
// the box stage of a stage-wise call on slot 0's resident cloud; returns the view its products are read through
ClusterBuffers launch_box_stage(mot_ctx* c, const ClusterBuffers& cb, int n) {
  if (c->point_order != MOT_ORDER_ANY) { mot_launch_box(c->dp, cb, 1, n, c->stream); return cb; }
  mot_launch_regroup(-1, c->dp, cb, regroup_buffers(c, c->d_label), 1, n, c->stream);
  const ClusterBuffers view = regrouped_view(c, cb);
  mot_launch_box(c->dp, view, 1, n, c->stream);
  return view;
}
// The mode's buffers, at the first request (a context that never asks pays nothing). A failure half-way leaves what exists for mot_destroy and the
// next request; the mode is not entered.
static int ensure_regroup(mot_ctx* c) {
  const size_t B = c->batch, N = c->cap;
  MOT_TRY(dev_alloc(c, &c->d_rg_key, B * N * sizeof(unsigned short)));
  MOT_TRY(dev_alloc(c, &c->d_rg_tmp, B * N * sizeof(unsigned)));
  MOT_TRY(dev_alloc(c, &c->d_rg_hist, B * c->max_wg * kRegroupDigits * sizeof(int)));
  MOT_TRY(dev_alloc(c, &c->d_rg_xyz, B * N * sizeof(float4)));   // (a slot every cap * 16 bytes, as the box kernels address `elevated`; the points are 12 bytes)
  MOT_TRY(dev_alloc(c, &c->d_rg_cell, B * N * sizeof(unsigned short)));
  // Group slots. After regrouping a frame has at most kMaxClusters + cap / 64 - 1 groups (derivation: mot_internal.h, mot_regroup_group_cap; include/mot.h,
  // "limits"), so with that many slots no frame is refused for its groups. The context's own cap / 2 slots are fewer only below ~8456 points per frame:
  // such a context gets group buffers of the mode's own, and buckets for the index kernel (the polygon pool it otherwise borrows holds cap / 2 entries).
  const long gc = mot_regroup_group_cap((long)N);
  if (gc > (long)(N / 2)) {
    MOT_TRY(dev_alloc(c, &c->d_rg_groups, B * gc * sizeof(PointGroup)));
    MOT_TRY(dev_alloc(c, &c->d_rg_gsorted, B * gc * sizeof(SortedGroup)));
    MOT_TRY(dev_alloc(c, &c->d_rg_gscratch, B * gc * sizeof(uint2)));
    c->rg_group_cap = (int)gc;
  }
  return MOT_OK;
}

static int create_impl(mot_ctx* c) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(c, MOT_E_HIP, "no HIP device: this library has no CPU fallback");
  if (c->device < 0 || c->device >= ndev) return fail(c, MOT_E_ARG, "device ordinal out of range");
  MOT_HIP(c, hipSetDevice(c->device));   // mot_create restores the caller's device (DevGuard)
  c->res.reset(c->batch);
  {
    hipDeviceProp_t prop;
    MOT_HIP(c, hipGetDeviceProperties(&prop, c->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
      c->err = std::string("device is ") + prop.gcnArchName + ": this library contains gfx950 (MI355X) code only";
      return MOT_E_HIP;
    }
  }
  MOT_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  MOT_TRY(new_event(c, &c->ev0, 0));
  MOT_TRY(new_event(c, &c->ev1, 0));
  const size_t B = c->batch, N = c->cap;
  c->max_chunks = (int)((N + kGroundChunk - 1) / kGroundChunk) + 1;
  MOT_TRY(dev_alloc(c, &c->d_in, B * N * sizeof(float4)));
  {  // the argument block and its staging ring
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    c->arg_off_targs = up(B * sizeof(int));
    c->arg_off_ego = up(c->arg_off_targs + B * sizeof(TrackFrameArgs));
    c->arg_off_launch = up(c->arg_off_ego + B * sizeof(EgoTf));
    c->arg_bytes = up(c->arg_off_launch + sizeof(FrameLaunch));
    MOT_TRY(dev_zeroed(c, &c->d_argblk, c->arg_bytes));
    MOT_TRY(c->arg_ring.create(c, c->arg_bytes));
    memset(c->arg_ring.base, 0, c->arg_bytes * PinnedRing::kBlocks);
    c->d_n = reinterpret_cast<int*>(c->d_argblk);
    c->d_targs = reinterpret_cast<TrackFrameArgs*>(c->d_argblk + c->arg_off_targs);
    c->d_ego = reinterpret_cast<EgoTf*>(c->d_argblk + c->arg_off_ego);
  }
  MOT_TRY(dev_alloc(c, &c->d_ecell, B * N * sizeof(unsigned short)));
  MOT_TRY(dev_alloc(c, &c->d_pairs, B * c->max_chunks * kGroundChunk * sizeof(uint2)));
  MOT_TRY(dev_zeroed(c, &c->d_pair_count, B * c->max_chunks * sizeof(int)));
  MOT_TRY(dev_alloc(c, &c->d_hg, B * MOT_POLAR_CELLS * sizeof(float)));
  MOT_TRY(dev_alloc(c, &c->d_cell, B * N * sizeof(unsigned short)));
  MOT_TRY(dev_alloc(c, &c->d_gzmax, B * (N / 8) * sizeof(float)));   // (cap is a multiple of 64)
  MOT_TRY(dev_zeroed(c, &c->d_desc, B * c->max_chunks * sizeof(unsigned long long)));
  MOT_TRY(dev_zeroed(c, &c->d_ticket, B * sizeof(int)));
  MOT_TRY(dev_alloc(c, &c->d_elev, B * N * sizeof(float4)));
  MOT_TRY(dev_alloc(c, &c->d_ground, B * N * sizeof(float4)));
  MOT_TRY(dev_alloc(c, &c->d_mask, B * N));
  MOT_TRY(dev_zeroed(c, &c->d_counts, B * kCountsStride * sizeof(int)));
  MOT_TRY(pinned_alloc(c, &c->h_counts, B * kCountsStride * sizeof(int)));
  MOT_TRY(dev_zeroed(c, &c->d_plane_a, B * kPlaneWords * sizeof(unsigned)));
  MOT_TRY(dev_zeroed(c, &c->d_plane_b, B * kPlaneWords * sizeof(unsigned)));
  MOT_TRY(dev_alloc(c, &c->d_ccl_parent, B * kMaxRuns * sizeof(unsigned)));
  c->occ_chunks = (int)((N + kCompactChunk - 1) / kCompactChunk);
  MOT_TRY(dev_alloc(c, &c->d_occ_list, B * c->occ_chunks * kPlaneWords * sizeof(OccWord)));
  MOT_TRY(dev_zeroed(c, &c->d_occ_count, B * c->occ_chunks * sizeof(int)));
  MOT_TRY(dev_zeroed(c, &c->d_grid, B * MOT_MAX_GRID * MOT_MAX_GRID * sizeof(GridLabel)));
  MOT_TRY(dev_alloc(c, &c->d_label, B * N * sizeof(int)));
  MOT_TRY(dev_alloc(c, &c->d_stats, B * kMaxClusters * sizeof(ClusterStats)));
  MOT_TRY(dev_alloc(c, &c->d_cand, B * kMaxClusters * sizeof(BoxCandidate)));
  MOT_TRY(dev_alloc(c, &c->d_boxes, B * kMaxBoxesPerFrame * 24 * sizeof(float)));
  MOT_TRY(dev_alloc(c, &c->d_box_cluster, B * kMaxBoxesPerFrame * sizeof(int)));
  MOT_TRY(dev_alloc(c, &c->d_rng, kRngTable * sizeof(unsigned long long)));
  MOT_TRY(dev_alloc(c, &c->d_poly, B * N * sizeof(int)));
  MOT_TRY(dev_alloc(c, &c->d_groups, B * (N / 2) * sizeof(PointGroup)));
  MOT_TRY(dev_alloc(c, &c->d_cluster_start, B * (kMaxClusters + 1) * sizeof(int)));
  MOT_TRY(dev_alloc(c, &c->d_order, B * kMaxClusters * sizeof(int)));
  MOT_TRY(dev_alloc(c, &c->d_gsorted, B * (N / 2) * sizeof(SortedGroup)));
  MOT_TRY(dev_alloc(c, &c->d_cluster_gstart, B * (kMaxClusters + 1) * sizeof(int)));
  MOT_TRY(dev_alloc(c, &c->d_pix, B * N * sizeof(int)));
  c->max_wg = (int)((N + 2047) / 2048);
  MOT_TRY(dev_alloc(c, &c->d_wgtab, B * c->max_wg * kWgClusters * sizeof(int2)));
  {  // mt19937_64 mt(0), box_fitting.cpp:303 — raw draws; the libstdc++ range mapping is applied on the device
    std::mt19937_64 mt(0);
    unsigned long long raw[kRngTable];
    for (int i = 0; i < kRngTable; i++) raw[i] = mt();
    MOT_HIP(c, hipMemcpyAsync(c->d_rng, raw, sizeof raw, hipMemcpyHostToDevice, c->stream));
    MOT_HIP(c, hipStreamSynchronize(c->stream));
  }
  {
    ClusterBuffers cb = cluster_buffers(c);
    mot_launch_stats_init(cb, (int)B, c->stream);
    MOT_HIP(c, hipGetLastError());
  }
  const size_t T = c->max_tracks_total;
  MOT_TRY(dev_alloc(c, &c->d_tracks, B * T * sizeof(DevTrack)));
  MOT_TRY(dev_zeroed(c, &c->d_nt, B * sizeof(int)));
  MOT_TRY(dev_alloc(c, &c->d_tboxes, B * kMaxBoxesPerFrame * 24 * sizeof(float)));
  MOT_TRY(dev_alloc(c, &c->d_gate, B * T * kGateWords * sizeof(unsigned long long)));
  MOT_TRY(dev_alloc(c, &c->d_prog, B * T * kGateWords * sizeof(unsigned long long)));
  MOT_TRY(dev_alloc(c, &c->d_live, B * 2 * T * sizeof(int)));
  MOT_TRY(dev_alloc(c, &c->d_tout, B * T * sizeof(mot_track)));
  MOT_TRY(dev_zeroed(c, &c->d_tflags, B * sizeof(int)));
  MOT_TRY(dev_zeroed(c, &c->d_nlive, B * sizeof(int)));
  const size_t E = c->max_tracks_ever;
  MOT_TRY(dev_alloc(c, &c->d_pos, B * E * sizeof(Vec2d)));
  MOT_TRY(dev_alloc(c, &c->d_slot_of, B * E * sizeof(int)));
  // zeroed: the tracker writes a tombstone when it EVICTS a track, and mot_stream_save copies the tombstones of every id so far — those of the live ones must not be
  // whatever the allocator handed out (two contexts with one history then give the same snapshot bytes)
  MOT_TRY(dev_zeroed(c, &c->d_tomb, B * E * sizeof(TrackTomb)));
  MOT_TRY(dev_zeroed(c, &c->d_used, B * ((T + 63) / 64) * sizeof(unsigned long long)));
  MOT_TRY(dev_alloc(c, &c->d_zomb, B * T * sizeof(int)));
  MOT_TRY(dev_zeroed(c, &c->d_nzomb, B * sizeof(int)));
  MOT_TRY(dev_alloc(c, &c->d_cp, B * kMaxBoxesPerFrame * sizeof(Vec2d)));
  MOT_TRY(dev_alloc(c, &c->d_items, B * T * sizeof(TrackItem)));
  MOT_TRY(dev_zeroed(c, &c->d_nitems, sizeof(int)));
  c->ego.assign(B, mot_ctx::SlotEgo());
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  c->h_n.assign(B, 0);
  return MOT_OK;
}

// why the calling thread's last mot_create failed: there is no context to ask then (mot_last_error(NULL))
static thread_local std::string g_create_err;

extern "C" int mot_create(const mot_params* params, int device, int max_points, int max_batch, int max_tracks_total,
                          mot_ctx** out) {
  g_create_err = "mot_create: null pointer, or max_points / max_batch / max_tracks_total out of range";
  if (!params || !out || max_points < 1 || max_points > kMaxPointsPerFrame || max_batch < 1 || max_tracks_total < 1) return MOT_E_ARG;
  *out = nullptr;
  mot_ctx* c = new mot_ctx();
  int prev_device = -1;
  (void)hipGetDevice(&prev_device);
  struct Restore { int d; ~Restore() { if (d >= 0) (void)hipSetDevice(d); } } restore{prev_device};
  c->params = *params; c->device = device; c->batch = max_batch;
  c->max_points = max_points;
  c->cap = (max_points + 63) / 64 * 64;  // per-slot stride of every per-point buffer: keeps 16-byte vector loads aligned
  c->max_tracks_total = max_tracks_total;
  {  // tracks EVER created per stream that the light arrays hold (44 bytes each); mot_params.max_tracks_ever, 0 = kEverFactor x the slots
    long e = params->max_tracks_ever > 0 ? (long)params->max_tracks_ever : (long)max_tracks_total * kEverFactor;
    if (e < max_tracks_total) e = max_tracks_total;
    if (e > (1l << 26)) e = 1l << 26;
    c->max_tracks_ever = (int)e;
  }
  int rc = make_dev_params(c->params, &c->dp, &c->err);
  if (rc == MOT_OK) rc = create_impl(c);
  if (rc != MOT_OK) {
    fprintf(stderr, "mot_create failed: %s\n", c->err.c_str());
    g_create_err = c->err;
    mot_destroy(c);
    return rc;
  }
  *out = c;
  g_create_err.clear();
  return MOT_OK;
}

extern "C" int mot_get_params(const mot_ctx* c, mot_params* out) {
  if (!c || !out) return MOT_E_ARG;
  *out = c->params;
  return MOT_OK;
}
extern "C" const char* mot_last_error(const mot_ctx* c) { return c ? c->err.c_str() : (g_create_err.empty() ? "null context" : g_create_err.c_str()); }
extern "C" void* mot_stream(mot_ctx* c) { return c ? (void*)c->stream : nullptr; }
extern "C" int mot_synchronize(mot_ctx* c) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (c->copy_stream) MOT_HIP(c, hipStreamSynchronize(c->copy_stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  return MOT_OK;
}
extern "C" int mot_reset(mot_ctx* c) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  // stream-ordered: takes effect after the steps already queued, before the next one (no host synchronisation)
  MOT_HIP(c, hipMemsetAsync(c->d_nt, 0, c->batch * sizeof(int), c->stream));
  MOT_HIP(c, hipMemsetAsync(c->d_nlive, 0, c->batch * sizeof(int), c->stream));
  MOT_HIP(c, hipMemsetAsync(c->d_tflags, 0, c->batch * sizeof(int), c->stream));
  MOT_TRY(accum_restart_slots(c, 0, c->batch));
  MOT_TRY(scene_restart_slots(c, 0, c->batch));
  c->ego.assign(c->batch, mot_ctx::SlotEgo());
  return MOT_OK;
}

// every launch of the compaction kernel gets a fresh epoch; on wrap-around the descriptors are cleared so a
// 2^20-launches-old descriptor can never be mistaken for a current one
int next_epoch(mot_ctx* c) {
  c->epoch++;
  if (c->epoch > kDescEpochMask) {
    MOT_HIP(c, hipMemsetAsync(c->d_desc, 0, (size_t)c->batch * c->max_chunks * sizeof(unsigned long long), c->stream));
    c->epoch = 1;
  }
  return MOT_OK;
}

GroundBuffers ground_buffers(mot_ctx* c, const float4* in, long stride, bool want_mask, bool planes) {
  GroundBuffers g;
  g.launch = nullptr;
  g.epoch = c->epoch;
  g.in = in; g.in_stride = stride; g.n = c->d_n; g.pairs = c->d_pairs; g.pair_count = c->d_pair_count; g.hg = c->d_hg; g.cell = c->d_cell; g.gzmax = c->d_gzmax; g.desc = c->d_desc;
  g.ticket = c->d_ticket; g.elevated = c->d_elev; g.elevated_packed = 0; g.ground = c->d_ground; g.mask = want_mask ? c->d_mask : nullptr;
  g.counts = c->d_counts; g.cap = c->cap; g.max_chunks = c->max_chunks;
  g.occ_list = planes ? c->d_occ_list : nullptr; g.occ_count = planes ? c->d_occ_count : nullptr; g.occ_chunks = c->occ_chunks;
  g.ecell = (planes && c->params.num_grid < MOT_MAX_GRID) ? c->d_ecell : nullptr;   // (a 256-cell grid uses all 65536 codes: no "outside" left)
  return g;
}

// validates n[], remembers the launch geometry and (stage-wise entry points: upload = true) sends n[] to the device; the fused
// path sends it with the rest of its arguments (launch_frames)
// The one walk over a batch's point counts: the batch in range, every count in 0 .. max_points, *max_n the largest frame. stride_points >= 0: frames of a batch of several must
// fit their stride, tested frame by frame where the walk gets to them (per_frame: the host-ingest calls) or once on the largest frame behind the walk (the device calls) — which
// refusal a batch with two faults gets is part of the ABI's behaviour. payloads: one host buffer per frame, none of them null.
static int check_batch(mot_ctx* c, const int* n_points, int batch, long stride_points, bool per_frame, const void* const* payloads, int* max_n) {
  if (batch < 1 || batch > c->batch) return fail(c, MOT_E_ARG, "batch out of range");
  const bool strided = stride_points >= 0 && batch > 1;
  *max_n = 0;
  for (int b = 0; b < batch; b++) {
    const int n = n_points[b];
    if (n < 0 || (payloads && n > 0 && !payloads[b])) return fail(c, MOT_E_ARG, payloads ? "negative point count or null payload" : "negative point count");
    if (n > c->max_points) return fail(c, MOT_E_CAPACITY, "frame has more points than max_points");
    if (strided && per_frame && stride_points < n) return fail(c, MOT_E_ARG, "frame_stride is smaller than a frame");
    if (n > *max_n) *max_n = n;
  }
  if (strided && !per_frame && stride_points < *max_n) return fail(c, MOT_E_ARG, "frame_stride is smaller than a frame");
  return MOT_OK;
}
static int check_tracker_inputs(mot_ctx* c, int run_tracker, const double* timestamps, const double* ego_v, const double* ego_yaw) {
  return (run_tracker && (!timestamps || !ego_v || !ego_yaw)) ? fail(c, MOT_E_ARG, "run_tracker needs timestamps, ego_v and ego_yaw") : MOT_OK;
}
// x, y, z and — where there is one (off_w >= 0) — the 4th field lie inside the point record
int check_field_offsets(mot_ctx* c, int point_step, int off_x, int off_y, int off_z, int off_w) {
  const int offs[4] = {off_x, off_y, off_z, off_w};
  for (int k = 0; k < 4; k++)
    if ((k < 3 || offs[k] >= 0) && (offs[k] < 0 || offs[k] + 4 > point_step)) return fail(c, MOT_E_ARG, "field offset outside the point record");
  return MOT_OK;
}

int set_batch(mot_ctx* c, const int* n_points, int batch, const float4* in, long stride, bool upload) {
  int max_n;
  MOT_TRY(check_batch(c, n_points, batch, stride, false, nullptr, &max_n));
  for (int b = 0; b < batch; b++) c->h_n[b] = n_points[b];
  if (upload) {
    char* blk;
    MOT_TRY(arg_block_acquire(c, &blk));
    memcpy(blk, c->h_n.data(), batch * sizeof(int));
    MOT_TRY(arg_block_commit(c, 0, batch * sizeof(int)));
  }
  c->res.describe_batch(batch, max_n, in, stride);
  return MOT_OK;
}

// in-run timing of one kernel: an event pair around its launch, on the context stream, while the ring has room
// roctx ranges around the stages of a launch sequence (the reference has none; a tracing aid of this library):
// "mot:ground", "mot:cluster", "mot:box", "mot:tracker" on the issuing thread, visible in rocprofv3 --marker-trace / rocprof-sys
// timelines next to the kernels they launched. libroctx64 is looked up at run time on first use (no link-time dependency; silently
// off when it is not there). mot_set_trace_ranges(ctx, 1) turns them on.
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  std::once_flag once;
  void load() { std::call_once(once, [this] { find(); }); }   // (contexts of several threads may switch their ranges on at the same time)
  void find() {
#ifndef MOT_HIPEMU
    for (const char* name : {"libroctx64.so", "libroctx64.so.4", "librocprofiler-sdk-roctx.so"}) {
      if (void* h = dlopen(name, RTLD_LAZY | RTLD_LOCAL)) {
        push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (push && pop) return;
        push = nullptr; pop = nullptr;
      }
    }
#endif
  }
};
static Roctx g_roctx;
struct RangeScope {
  bool on;
  RangeScope(const mot_ctx* c, const char* name);
  ~RangeScope() { if (on) (void)g_roctx.pop(); }
};

// the kernels of one fused launch sequence, in order, on the context stream (plain launches, or under stream capture)
RangeScope::RangeScope(const mot_ctx* c, const char* name) : on(false) {
  if (!c->trace_ranges) return;
  g_roctx.load();
  if (g_roctx.push) { (void)g_roctx.push(name); on = true; }
}

// the buffer sets of a launch in the fused geometry: the compaction kernel leaves the occupancy as per-chunk lists and every elevated point's cell for the label kernel; the ground cloud, the mask and the
// per-point labels only where mot_set_fused_outputs asks for them (on demand otherwise: mot_get_ground, mot_get_clusters). The readers' layout (cluster_buffers) comes from the residency record, which the
// CALLERS of issue_frame_kernels set: they also run when a captured graph is replayed and issue_frame_kernels is not.
void fused_buffers(mot_ctx* c, GroundBuffers* g, ClusterBuffers* cb) {
  *g = ground_buffers(c, c->res.last_in, c->res.last_in_stride, (c->fused_outputs & MOT_OUT_MASK) != 0, true);
  if (!(c->fused_outputs & MOT_OUT_GROUND)) g->ground = nullptr;
  g->elevated_packed = Residency::fused_packs(c->fused_outputs) ? 1 : 0;
  *cb = cluster_buffers(c);
  cb->occ_list = c->d_occ_list; cb->occ_count = c->d_occ_count; cb->ecell = g->ecell;
  if (!(c->fused_outputs & MOT_OUT_LABELS)) cb->label = nullptr;
}

// the regrouping pass of a fused launch writes the per-point labels (input order) where the label kernel would have
RegroupBuffers fused_regroup_buffers(const mot_ctx* c) { return regroup_buffers(c, (c->fused_outputs & MOT_OUT_LABELS) ? c->d_label : nullptr); }

static void issue_frame_kernels(mot_ctx* c, int batch, int max_n, int run_tracker, bool from_block) {
  GroundBuffers g; ClusterBuffers cb;
  fused_buffers(c, &g, &cb);
  if (from_block) g.launch = reinterpret_cast<const FrameLaunch*>(c->d_argblk + c->arg_off_launch);
  {
    RangeScope rs(c, "mot:ground");
    { ProfScope ps(c, kK1); mot_launch_ground_kernel(0, c->dp, g, batch, max_n, c->stream); }
    if (!(c->dbg_skip & 1)) { ProfScope ps(c, kK2); mot_launch_ground_kernel(1, c->dp, g, batch, max_n, c->stream); }
    { ProfScope ps(c, kK3); mot_launch_ground_kernel(2, c->dp, g, batch, max_n, c->stream); }
  }
  // MEASUREMENT ONLY (mot_debug_skip_kernels bits 8-11: a count): that many EXTRA launch boundaries — empty one-workgroup-per-frame kernels — in the middle of the
  // sequence. What k more boundaries cost is what fusing k of the sequence's one-workgroup-per-frame launches away could at most win (profiles/r06_launch_boundaries.md).
  for (int k = 0; k < ((c->dbg_skip >> 8) & 15); k++) mot_launch_noop(batch, c->stream);
  if (!(c->dbg_skip & 2)) { RangeScope rs(c, "mot:cluster"); ProfScope ps(c, kC2); mot_launch_cluster(c->dp, cb, batch, max_n, c->stream, true); }
  RangeScope rb(c, "mot:box");
  const ClusterBuffers cb_input = cb;   // the frame in input order: what the per-point track ids follow in either point order
  if (c->point_order == MOT_ORDER_ANY) {   // the points into cluster order first; the box stage runs on the copy
    const RegroupBuffers rg = fused_regroup_buffers(c);
    { ProfScope ps(c, kR1); mot_launch_regroup(0, c->dp, cb, rg, batch, max_n, c->stream); }
    { ProfScope ps(c, kR2); mot_launch_regroup(1, c->dp, cb, rg, batch, max_n, c->stream); }
    { ProfScope ps(c, kR3); mot_launch_regroup(2, c->dp, cb, rg, batch, max_n, c->stream); }
    cb = regrouped_view(c, cb);
  }
  { ProfScope ps(c, kB1); mot_launch_box_kernel(0, c->dp, cb, batch, max_n, c->stream); }
  if (!(c->dbg_skip & 4)) { ProfScope ps(c, kB1b); mot_launch_box_kernel(4, c->dp, cb, batch, max_n, c->stream); }
  { ProfScope ps(c, kB2); mot_launch_box_kernel(1, c->dp, cb, batch, max_n, c->stream); }
  { ProfScope ps(c, kB2b); mot_launch_box_kernel(3, c->dp, cb, batch, max_n, c->stream); }
  if (run_tracker) {   // the tracker's per-frame prologue rides at the tail of the box stage's last kernel (same geometry)
    const TrackBuffers tb = track_buffers(c, true);
    if (!(c->dbg_skip & 8)) { ProfScope ps(c, kB3); mot_launch_box_finalize_prep(c->dp, cb, tb, batch, c->stream); }
    if (rb.on) { (void)g_roctx.pop(); rb.on = false; }
    if (!(c->dbg_skip & 32)) { RangeScope rt(c, "mot:tracker"); ProfScope ps(c, kT1); mot_launch_track(tb, batch, c->stream, true); }
    if (c->track_links) { RangeScope rl(c, "mot:links"); mot_launch_point_tracks(c->dp, cb_input, c->d_owner, batch, max_n, c->d_point_track, c->cap, nullptr, c->stream); }
  } else {
    ProfScope ps(c, kB3); mot_launch_box_kernel(2, c->dp, cb, batch, max_n, c->stream);
  }
}

// Every per-batch argument in ONE copy at the head of a fused sequence: n[], and for the tracker the tracking node's per-frame host work
// (OT/tracking/main.cpp:72-166): ego pose, the tf chain's matrix, dt / first-frame flags. one_stream (mot_sequence_dev): entry k is FRAME k of
// stream 0 — its ego pose advanced frame by frame on the host (slot 0's dead reckoning) — instead of stream k's frame.
static int send_frame_args(mot_ctx* c, int batch, int run_tracker, bool one_stream, const double* timestamps, const double* ego_v, const double* ego_yaw) {
  char* blk;
  MOT_TRY(arg_block_acquire(c, &blk));
  memcpy(blk, c->h_n.data(), batch * sizeof(int));
  TrackFrameArgs* targs = reinterpret_cast<TrackFrameArgs*>(blk + c->arg_off_targs);
  EgoTf* ego = reinterpret_cast<EgoTf*>(blk + c->arg_off_ego);
  for (int b = 0; b < c->batch; b++) targs[b].run = 0;
  if (run_tracker)
    for (int b = 0; b < batch; b++) {
      const int s = one_stream ? 0 : b;   // the stream whose ego / tracker state entry b advances
      MOT_TRY(mot_ego_update(c, s, timestamps[b], ego_v[b], ego_yaw[b], nullptr));
      tf_velodyne_to_global(c->ego[s].egoPoint[0], c->ego[s].egoPoint[1], c->ego[s].egoPoint[2], ego[b].m);
      if (c->track_links) c->link_tf[b] = ego[b];   // what mot_export_track_points_dev applies to slot b's points (the argument block is rewritten by every later call)
      TrackFrameArgs one[1];
      prepare_track_args(c, one_stream ? one : targs, s, 0, timestamps[b], true);   // (fills entry s of the array it is given)
      if (one_stream) targs[b] = one[0];
    }
  FrameLaunch* fl = reinterpret_cast<FrameLaunch*>(blk + c->arg_off_launch);
  fl->in = c->res.last_in; fl->in_stride = c->res.last_in_stride; fl->epoch = c->epoch; fl->pad = 0;
  return arg_block_commit(c, 0, (run_tracker || c->graph_mode) ? c->arg_bytes : batch * sizeof(int));
}

// the fused launch sequence of one batch on the context stream; every argument has been validated
static int launch_frames(mot_ctx* c, int batch, int run_tracker, const double* timestamps, const double* ego_v, const double* ego_yaw) {
  MOT_TRY(next_epoch(c));
  const int max_n = c->res.last_max_n;
  MOT_TRY(send_frame_args(c, batch, run_tracker, false, timestamps, ego_v, ego_yaw));
  c->res.fused_batch(batch, c->fused_outputs, c->point_order == MOT_ORDER_ANY, run_tracker && c->track_links);
#ifndef MOT_HIPEMU
  // Few streams per launch = somebody waits for every frame: the sequence's 10-13 launches go out as ONE hipGraph launch, captured
  // once per launch geometry. What differs from call to call without changing the geometry (the cloud's address, the look-back
  // epoch) travels in the argument block (FrameLaunch). Not while a kernel is being timed (the event pairs are host calls).
  if (c->graph_mode && c->prof_kernel == 0) {
    const mot_ctx::GraphKey key = {batch, (max_n + kGroundChunk - 1) / kGroundChunk, run_tracker ? 1 : 0, c->fused_outputs, c->point_order};
    void* exec = nullptr;
    for (const auto& ge : c->graphs)
      if (ge.key.batch == key.batch && ge.key.chunks == key.chunks && ge.key.tracker == key.tracker && ge.key.outputs == key.outputs && ge.key.order == key.order) { exec = ge.exec; break; }
    if (!exec) {
      hipGraph_t graph = nullptr;
      hipGraphExec_t ge = nullptr;
      bool ok = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
      if (ok) {
        issue_frame_kernels(c, batch, key.chunks * kGroundChunk, run_tracker, true);   // (grids from the chunk count: any frame of this geometry)
        ok = hipStreamEndCapture(c->stream, &graph) == hipSuccess && graph != nullptr;
      }
      if (ok) ok = hipGraphInstantiate(&ge, graph, nullptr, nullptr, 0) == hipSuccess;
      if (graph) (void)hipGraphDestroy(graph);
      if (!ok) { (void)hipGetLastError(); c->graph_mode = 0; }   // this runtime cannot capture the sequence: plain launches from now on
      else { if (c->graphs.size() >= 16) { destroy_graph(c->graphs.front().exec); c->graphs.erase(c->graphs.begin()); }
             c->graphs.push_back({key, (void*)ge}); exec = (void*)ge; }
    }
    if (exec) {
      MOT_HIP(c, hipGraphLaunch((hipGraphExec_t)exec, c->stream));
      return MOT_OK;
    }
  }
#endif
  issue_frame_kernels(c, batch, max_n, run_tracker, false);
  MOT_HIP(c, hipGetLastError());
  return MOT_OK;
}

static int check_frames_args(mot_ctx* c, const void* xyzw, long frame_stride, const int* n_points, int batch, int run_tracker,
                             const double* timestamps, const double* ego_v, const double* ego_yaw) {
  if (!xyzw || !n_points) return fail(c, MOT_E_ARG, "null cloud or point-count pointer");
  if (frame_stride < 0 || frame_stride % 4) return fail(c, MOT_E_ARG, "frame_stride must be a non-negative multiple of 4 floats");
  if (((size_t)xyzw & 15) != 0 || (batch > 1 && (frame_stride * 4) % 16 != 0)) return fail(c, MOT_E_ARG, "clouds must be 16-byte aligned");
  return check_tracker_inputs(c, run_tracker, timestamps, ego_v, ego_yaw);
}

extern "C" int mot_frames_dev(mot_ctx* c, const float* d_xyzw, long frame_stride, const int* n_points, int batch,
                              int run_tracker, const double* timestamps, const double* ego_v, const double* ego_yaw) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  // every argument is checked before the first launch or state change
  MOT_TRY(check_frames_args(c, d_xyzw, frame_stride, n_points, batch, run_tracker, timestamps, ego_v, ego_yaw));
  MOT_TRY(set_batch(c, n_points, batch, (const float4*)d_xyzw, frame_stride / 4, false));
  return launch_frames(c, batch, run_tracker, timestamps, ego_v, ego_yaw);
}

// ---------------------------------------------------------------------------------------- pipelined host ingest
// K consecutive frames of ONE stream (BASELINE.json configs[3] as written: one 154-frame drive; the single-process precedent is
// OT0/src/main.cpp:51-375 — one callback per frame): the stateless stages are independent per frame, so all K frames go through
// ground -> cluster -> box as ONE batch (slot k = frame k: the launches a batch of K streams would get), and only the tracker — sequential
// by nature, imm_ukf_jpda.cpp:704-1112 carries targets_ from frame to frame — runs K steps, chained on the device, each reading frame
// k's boxes where the box stage left them (slot k) and stream 0's track state. No host synchronisation anywhere.
static int sequence_frames(mot_ctx* c, const char* who, int products, const float* d_xyzw, long frame_stride, const int* n_points, int frames,
                           const double* timestamps, const double* ego_v, const double* ego_yaw, void* d_tracks, int max_per_frame, int32_t* d_counts) {
  MOT_TRY(check_frames_args(c, d_xyzw, frame_stride, n_points, frames, 1, timestamps, ego_v, ego_yaw));
  if ((d_tracks != nullptr) != (d_counts != nullptr) || (d_tracks && max_per_frame < 1)) return fail(c, MOT_E_ARG, who, ": d_tracks and d_counts go together, max_per_frame >= 1");
  const bool accumulate = (products & MOT_SEQ_ACCUMULATE) != 0, scene = (products & MOT_SEQ_SCENE) != 0;
  if (products) {   // every refusal before the first state change: the tracker has not stepped, nothing has run
    int max_n;
    MOT_TRY(check_batch(c, n_points, frames, frame_stride / 4, false, nullptr, &max_n));
    if (accumulate) MOT_TRY(seq_accum_ready(c, who));
    if (scene) MOT_TRY(seq_scene_ready(c, who, frames));
  }
  MOT_TRY(set_batch(c, n_points, frames, (const float4*)d_xyzw, frame_stride / 4, false));
  MOT_TRY(next_epoch(c));
  const int K = frames, max_n = c->res.last_max_n;
  MOT_TRY(send_frame_args(c, K, 1, true, timestamps, ego_v, ego_yaw));   // one argument block for the whole sequence
  c->res.fused_batch(K, c->fused_outputs, c->point_order == MOT_ORDER_ANY, c->track_links != 0, true);   // (links: row k / the ids of slot k = frame k)
  issue_frame_kernels(c, K, max_n, 0, false);   // slots = frames; ends with the plain box_finalize_kernel
  const TrackBuffers base = track_buffers(c, true);
  RangeScope rt(c, "mot:tracker (sequence)");
  for (int k = 0; k < K; k++) {   // the per-frame inputs of step k live in slot k, the track state in slot 0
    TrackBuffers tb = base;
    tb.args += k; tb.ego += k; tb.m_dev += (long)k * kCountsStride; tb.cp += (long)k * kMaxBoxesPerFrame;
    tb.boxes_sensor += (long)k * kMaxBoxesPerFrame * 24; tb.boxes += (long)k * tb.box_stride; tb.boxes_out += (long)k * tb.box_stride;
    if (tb.owner) { tb.owner += (long)k * kMaxBoxesPerFrame; tb.owner_n += k; }
    mot_launch_track(tb, 1, c->stream, false);
    if (accumulate) seq_accum_capture(c, k);   // the id -> slot map and the records of step k, before step k + 1 moves them
    if (scene) seq_scene_capture(c, k);        // ... and which ids of the frame step k left flagged static
    if (d_tracks) mot_launch_export_tracks(tb, 1, reinterpret_cast<mot_track*>(d_tracks) + (long)k * max_per_frame, max_per_frame, reinterpret_cast<int*>(d_counts) + k, c->stream);
  }
  if (c->track_links) {   // every frame's points against its own owner row, in one launch behind the last step
    GroundBuffers g; ClusterBuffers cb;
    fused_buffers(c, &g, &cb);
    mot_launch_point_tracks(c->dp, cb, c->d_owner, K, max_n, c->d_point_track, c->cap, nullptr, c->stream);
  }
  MOT_HIP(c, hipGetLastError());
  if (accumulate) MOT_TRY(seq_accum_append(c, K, max_n));
  return scene ? seq_scene_append(c, K, max_n) : MOT_OK;
}
extern "C" int mot_sequence_dev(mot_ctx* c, const float* d_xyzw, long frame_stride, const int* n_points, int frames,
                                const double* timestamps, const double* ego_v, const double* ego_yaw,
                                void* d_tracks, int max_per_frame, int32_t* d_counts) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  return sequence_frames(c, "mot_sequence_dev", 0, d_xyzw, frame_stride, n_points, frames, timestamps, ego_v, ego_yaw, d_tracks, max_per_frame, d_counts);
}
// the same call, and every frame appended to stream 0's per-track accumulators behind the chain (mot_api_tracks.hip: seq_accum_*; kernels: track_accum_seq.hip)
extern "C" int mot_sequence_accumulate_dev(mot_ctx* c, const float* d_xyzw, long frame_stride, const int* n_points, int frames,
                                           const double* timestamps, const double* ego_v, const double* ego_yaw,
                                           void* d_tracks, int max_per_frame, int32_t* d_counts) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  return sequence_frames(c, "mot_sequence_accumulate_dev", MOT_SEQ_ACCUMULATE, d_xyzw, frame_stride, n_points, frames, timestamps, ego_v, ego_yaw, d_tracks, max_per_frame, d_counts);
}
// the same call with a set of products: MOT_SEQ_ACCUMULATE as above, MOT_SEQ_SCENE every frame into stream 0's scene grid (mot_api_scene.hip: seq_scene_*; kernels:
// scene_grid_seq.hip), both, or none
extern "C" int mot_sequence_products_dev(mot_ctx* c, const float* d_xyzw, long frame_stride, const int* n_points, int frames,
                                         const double* timestamps, const double* ego_v, const double* ego_yaw,
                                         void* d_tracks, int max_per_frame, int32_t* d_counts, int products) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (products & ~(MOT_SEQ_ACCUMULATE | MOT_SEQ_SCENE)) return fail(c, MOT_E_ARG, "mot_sequence_products_dev: unknown product bit");
  return sequence_frames(c, "mot_sequence_products_dev", products, d_xyzw, frame_stride, n_points, frames, timestamps, ego_v, ego_yaw, d_tracks, max_per_frame, d_counts);
}

static int ensure_copy_path(mot_ctx* c) {
  if (c->copy_ready) return MOT_OK;
  // a failure half-way (two batch x cap x 16-byte staging buffers: out of memory is plausible) leaves what exists for mot_destroy
  // and the path not ready: the next call tries again from where this one stopped
  if (!c->copy_stream) MOT_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  for (int i = 0; i < 2; i++) {
    MOT_TRY(dev_alloc(c, &c->d_stage[i], (size_t)c->batch * c->cap * sizeof(float4)));
    MOT_TRY(new_event(c, &c->ev_copied[i], hipEventDisableTiming));
    MOT_TRY(new_event(c, &c->ev_consumed[i], hipEventDisableTiming));
  }
  c->copy_ready = true;
  return MOT_OK;
}

// the next staging parity; the copy stream waits for the last reader of where the copies go: d_stage[s]'s last compaction kernel, or a landing buffer's (12-byte / raw records) last unpacking kernel
static int next_stage(mot_ctx* c, bool landing, int* s_out) {
  const int s = *s_out = c->stage_next;
  c->stage_next ^= 1;
  if (landing ? c->stage12_used[s] : c->stage_used[s]) MOT_HIP(c, hipStreamWaitEvent(c->copy_stream, landing ? c->ev_expanded[s] : c->ev_consumed[s], 0));
  return MOT_OK;
}
// the copies of parity s are queued: the compute stream waits for them
static int stage_copied(mot_ctx* c, int s) {
  MOT_HIP(c, hipEventRecord(c->ev_copied[s], c->copy_stream));
  MOT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_copied[s], 0));
  return MOT_OK;
}
// host frames of w floats a point -> a staging buffer at its stride of cap points (frames already at that stride: one copy for the whole batch)
static int copy_frames(mot_ctx* c, int s, float* dst, const float* src, long frame_stride, int w, const int* n_points, int batch) {
  const size_t cap_w = (size_t)c->cap * w;
  if ((size_t)frame_stride == cap_w) {
    const size_t bytes = ((size_t)(batch - 1) * cap_w + (size_t)n_points[batch - 1] * w) * sizeof(float);
    if (bytes) MOT_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->copy_stream));
  } else {
    for (int b = 0; b < batch; b++)
      if (n_points[b] > 0)
        MOT_HIP(c, hipMemcpyAsync(dst + (size_t)b * cap_w, src + (size_t)b * frame_stride, (size_t)n_points[b] * w * sizeof(float), hipMemcpyHostToDevice, c->copy_stream));
  }
  return stage_copied(c, s);
}
// the fused sequence on the batch staged in d_stage[s]
// an unpacking kernel has just filled d_stage[s] from the landing buffer of parity s (d_stage[s] was last read two batches ago, on this same stream: ordered)
static int mark_unpacked(mot_ctx* c, int s) {
  MOT_HIP(c, hipGetLastError());
  MOT_HIP(c, hipEventRecord(c->ev_expanded[s], c->stream));
  c->stage12_used[s] = true;
  return MOT_OK;
}
static int launch_staged(mot_ctx* c, int s, const int* n_points, int batch, int run_tracker, const double* timestamps, const double* ego_v, const double* ego_yaw) {
  MOT_TRY(set_batch(c, n_points, batch, c->d_stage[s], c->cap, false));
  const int rc = launch_frames(c, batch, run_tracker, timestamps, ego_v, ego_yaw);
  // (recorded after the whole sequence: the input is last read by the compaction kernel, but mot_time_stage may re-read it)
  MOT_HIP(c, hipEventRecord(c->ev_consumed[s], c->stream));
  c->stage_used[s] = true;
  return rc;
}

// One sensor frame per slot from HOST memory (what the reference's nodes receive per message: OT/src/groundremove/main.cpp:91-136,
// OT0/src/main.cpp:51-95), pipelined: the H2D copy of this batch runs on the context's copy stream into one of two staging
// buffers while the kernels of the previous batch run on the compute stream. Returns as soon as everything is queued.
extern "C" int mot_frames_host(mot_ctx* c, const float* h_xyzw, long frame_stride, const int* n_points, int batch,
                               int run_tracker, const double* timestamps, const double* ego_v, const double* ego_yaw) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  MOT_TRY(check_frames_args(c, h_xyzw, frame_stride, n_points, batch, run_tracker, timestamps, ego_v, ego_yaw));
  int max_n, s;
  MOT_TRY(check_batch(c, n_points, batch, frame_stride / 4, true, nullptr, &max_n));
  MOT_TRY(ensure_copy_path(c));
  MOT_TRY(next_stage(c, false, &s));
  MOT_TRY(copy_frames(c, s, reinterpret_cast<float*>(c->d_stage[s]), h_xyzw, frame_stride, 4, n_points, batch));
  return launch_staged(c, s, n_points, batch, run_tracker, timestamps, ego_v, ego_yaw);
}

// mot_frames_host for clouds WITHOUT a 4th value: packed {x, y, z} records, 12 bytes a point (include/mot.h). pcl::PointXYZ has no 4th value (its
// padding float is 1.0f), the node shells repack the PointCloud2 payload anyway (ros/src/ground_node.cpp) — and the host link, not the GPU, bounds a
// host-fed deployment: 25 % fewer bytes over PCIe. The records land in a 12-byte staging buffer (copy stream) and a small kernel on the compute
// stream expands them to the float4 layout every kernel of the path reads (w = 1.0f: what fromROSMsg leaves in PointXYZ's padding and what the
// PointCloud2 decoder writes for a cloud without a 4th field); 28 bytes of HBM traffic per point against 12 over a link ~100 x slower.
extern "C" int mot_frames_host_xyz(mot_ctx* c, const float* h_xyz, long frame_stride, const int* n_points, int batch,
                                   int run_tracker, const double* timestamps, const double* ego_v, const double* ego_yaw) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (!h_xyz || !n_points) return fail(c, MOT_E_ARG, "null cloud or point-count pointer");
  if (frame_stride < 0 || ((size_t)h_xyz & 3) != 0) return fail(c, MOT_E_ARG, "mot_frames_host_xyz: frame_stride (floats) must be non-negative, the cloud 4-byte aligned");
  int max_n, s;
  MOT_TRY(check_tracker_inputs(c, run_tracker, timestamps, ego_v, ego_yaw));
  MOT_TRY(check_batch(c, n_points, batch, frame_stride / 3, true, nullptr, &max_n));
  MOT_TRY(ensure_copy_path(c));
  for (int i = 0; i < 2; i++) {
    MOT_TRY(dev_alloc(c, &c->d_stage12[i], (size_t)c->batch * c->cap * 3 * sizeof(float)));
    MOT_TRY(new_event(c, &c->ev_expanded[i], hipEventDisableTiming));
  }
  MOT_TRY(next_stage(c, true, &s));
  MOT_TRY(copy_frames(c, s, c->d_stage12[s], h_xyz, frame_stride, 3, n_points, batch));
  mot_launch_expand_xyz12(c->d_stage12[s], (long)c->cap * 3, c->d_stage[s], c->cap, batch, max_n, c->stream);
  MOT_TRY(mark_unpacked(c, s));
  return launch_staged(c, s, n_points, batch, run_tracker, timestamps, ego_v, ego_yaw);
}

// mot_frames_host for sensor_msgs/PointCloud2 payloads as they arrive — one message per sensor stream, each in its own host buffer (include/mot.h): what a
// node that fuses several lidars holds in its callbacks (fromROSMsg, OT/src/groundremove/main.cpp:100, for every one of them). The raw records cross PCIe
// on the copy stream (point_step bytes a point: 16 for kitti2bag's x, y, z, intensity; 22-32 for a velodyne driver's records with ring / time) and are
// unpacked on the device under the next batch's copy — no host-side repacking. off_w >= 0: the float32 field that becomes the 4th value of the ground /
// elevated records (intensity); -1: 1.0f, as fromROSMsg into PointXYZ leaves it.
extern "C" int mot_frames_host_pointcloud2(mot_ctx* c, const void* const* h_payloads, const int* n_points, int batch, int point_step, int off_x, int off_y,
                                           int off_z, int off_w, int run_tracker, const double* timestamps, const double* ego_v, const double* ego_yaw) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (!h_payloads || !n_points) return fail(c, MOT_E_ARG, "null payload list or point-count pointer");
  if (batch < 1 || batch > c->batch) return fail(c, MOT_E_ARG, "batch out of range");
  if (point_step < 12 || point_step > 4096) return fail(c, MOT_E_ARG, "PointCloud2 payload: point_step must be 12 .. 4096");
  int max_n;
  MOT_TRY(check_field_offsets(c, point_step, off_x, off_y, off_z, off_w));
  if (off_w < -1) return fail(c, MOT_E_ARG, "off_w must be -1 (no 4th field) or a field offset");
  MOT_TRY(check_tracker_inputs(c, run_tracker, timestamps, ego_v, ego_yaw));
  MOT_TRY(check_batch(c, n_points, batch, -1, false, h_payloads, &max_n));
  MOT_TRY(ensure_copy_path(c));
  const size_t slot_bytes = ((size_t)c->cap * (size_t)point_step + 15) & ~(size_t)15, need = (size_t)c->batch * slot_bytes;
  if (need > c->stage_raw_bytes) {   // (grow-only; a larger point_step than any before: both buffers are replaced once nothing reads them)
    MOT_HIP(c, hipStreamSynchronize(c->copy_stream)); MOT_HIP(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 2; i++) MOT_TRY(release(c, &c->d_stage_raw[i]));
    c->stage_raw_bytes = 0;
    for (int i = 0; i < 2; i++) MOT_TRY(dev_alloc(c, &c->d_stage_raw[i], need));
    c->stage_raw_bytes = need;
  }
  for (int i = 0; i < 2; i++) MOT_TRY(new_event(c, &c->ev_expanded[i], hipEventDisableTiming));
  int s;
  MOT_TRY(next_stage(c, true, &s));   // (shared with the 12-byte path: "the landing buffer of parity s has been unpacked")
  for (int b = 0; b < batch; b++)
    if (n_points[b] > 0)
      MOT_HIP(c, hipMemcpyAsync(c->d_stage_raw[s] + (size_t)b * slot_bytes, h_payloads[b], (size_t)n_points[b] * (size_t)point_step, hipMemcpyHostToDevice, c->copy_stream));
  MOT_TRY(stage_copied(c, s));
  mot_launch_decode_pointcloud2_batch(c->d_stage_raw[s], (long)slot_bytes, batch, max_n, point_step, off_x, off_y, off_z, off_w, c->d_stage[s], c->cap, c->stream);
  MOT_TRY(mark_unpacked(c, s));
  return launch_staged(c, s, n_points, batch, run_tracker, timestamps, ego_v, ego_yaw);
}

// blocks until every H2D copy queued by mot_frames_host has completed: the caller's host buffers may be reused
extern "C" int mot_wait_uploads(mot_ctx* c) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (c->copy_stream) MOT_HIP(c, hipStreamSynchronize(c->copy_stream));
  return MOT_OK;
}

// page-locked host memory for mot_frames_host / mot_fetch_tracks_async (pageable memory works too, but its copies are
// staged by the runtime and do not overlap)
extern "C" int mot_host_alloc(size_t bytes, void** out) {
  if (!out || bytes == 0) return MOT_E_ARG;
  *out = nullptr;
  return hipHostMalloc(out, bytes, hipHostMallocDefault) == hipSuccess ? MOT_OK : MOT_E_HIP;
}
extern "C" int mot_host_free(void* p) { return (!p || hipHostFree(p) == hipSuccess) ? MOT_OK : MOT_E_HIP; }

extern "C" int mot_set_launch_graphs(mot_ctx* c, int on) {
  if (!c) return MOT_E_ARG;
  c->graph_mode = on ? 1 : 0;
  return MOT_OK;
}

extern "C" int mot_set_trace_ranges(mot_ctx* c, int on) {
  if (!c) return MOT_E_ARG;
  c->trace_ranges = on ? 1 : 0;
  if (on) { g_roctx.load(); if (!g_roctx.push) return fail(c, MOT_E_STATE, "mot_set_trace_ranges: libroctx64 was not found (ranges stay off)"); }
  return MOT_OK;
}

extern "C" int mot_set_tracker_mode(mot_ctx* c, int mode) {
  if (!c) return MOT_E_ARG;
  if (mode != MOT_TRACKER_AUTO && mode != MOT_TRACKER_SPLIT && mode != MOT_TRACKER_STREAM) return fail(c, MOT_E_ARG, "mot_set_tracker_mode: unknown mode");
  MOT_GUARD(c);
  MOT_TRY(drop_graphs(c));   // captured launch sequences hold the old choice
  c->tracker_mode = mode;
  return MOT_OK;
}

// MOT_ORDER_ANY: every box stage from now on first regroups the frame's elevated points by cluster (regroup.hip). Sticky; what is resident stays readable
// (each slot remembers which view its box stage ran on).
extern "C" int mot_set_point_order(mot_ctx* c, int order) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (order != MOT_ORDER_SCAN && order != MOT_ORDER_ANY) return fail(c, MOT_E_ARG, "mot_set_point_order: order must be MOT_ORDER_SCAN or MOT_ORDER_ANY");
  if (order == c->point_order) return MOT_OK;
  if (order == MOT_ORDER_ANY) MOT_TRY(ensure_regroup(c));   // MOT_E_HIP: the mode stays as it was
  MOT_TRY(drop_graphs(c));   // the mode is part of the launch sequence: graphs captured in the other mode go
  c->point_order = order;
  return MOT_OK;
}

// ---------------------------------------------------------------------------------------- boxes and points linked to their tracks
// mot_set_track_links: every tracker step from now on keeps the association it computes anyway (track.hip "box owners") as a row of box owners per slot, and every
// fused call that runs the tracker ends with the per-point composition (link.hip). Sticky; off by default, and then nothing of this is launched, written or allocated.
static int ensure_links(mot_ctx* c) {   // a failure half-way leaves what exists for mot_destroy and the next request; the mode is not entered
  const size_t B = c->batch;
  MOT_TRY(dev_alloc(c, &c->d_owner, B * kMaxBoxesPerFrame * sizeof(int)));
  MOT_TRY(dev_alloc(c, &c->d_owner_n, B * sizeof(int)));
  MOT_TRY(dev_alloc(c, &c->d_point_track, B * (size_t)c->cap * sizeof(int)));
  c->link_tf.resize(B);
  return MOT_OK;
}
extern "C" int mot_set_track_links(mot_ctx* c, int on) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  on = on ? 1 : 0;
  if (on == c->track_links) return MOT_OK;
  if (!on && c->accum_K) return fail(c, MOT_E_STATE, "mot_set_track_links: the per-track accumulators are on (mot_set_track_accumulation(ctx, 0, 0) first)");
  if (!on && c->scene_W) return fail(c, MOT_E_STATE, "mot_set_track_links: the scene grid is on (mot_set_scene_grid(ctx, NULL) first)");
  if (on) MOT_TRY(ensure_links(c));   // MOT_E_HIP: the mode stays as it was
  MOT_TRY(drop_graphs(c));   // the link kernel and the owner pointers are part of the launch sequence: graphs captured in the other mode go
  c->track_links = on;
  c->res.links_switched();
  return MOT_OK;
}
extern "C" int mot_set_fused_outputs(mot_ctx* c, int flags) {
  if (!c) return MOT_E_ARG;
  if (flags & ~(MOT_OUT_GROUND | MOT_OUT_MASK | MOT_OUT_LABELS)) return fail(c, MOT_E_ARG, "mot_set_fused_outputs: unknown flag");
  c->fused_outputs = flags;
  return MOT_OK;
}
