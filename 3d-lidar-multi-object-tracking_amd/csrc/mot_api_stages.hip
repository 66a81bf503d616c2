// mot_api_stages.hip — host side of the C-ABI (include/mot.h), the calls that work on ONE stage or read what a stage left: in-run kernel timing, the getters, the stage-wise
// cluster / box / ground calls and node callbacks, the cluster node's side products, mot_time_stage, the debug hooks. Context and helpers: mot_host.h.
#include "mot_host.h"

// ---------------------------------------------------------------------------------------- in-run kernel timing
extern "C" int mot_profile_kernel(mot_ctx* c, int kernel_id, int every) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (every < 1) return fail(c, MOT_E_ARG, "mot_profile_kernel: every must be >= 1");
  for (int i = 0; i < mot_ctx::kProfRing; i++) { MOT_TRY(new_event(c, &c->prof_ev[i][0], 0)); MOT_TRY(new_event(c, &c->prof_ev[i][1], 0)); }   // (at the first call)
  c->prof_kernel = kernel_id; c->prof_n = 0; c->prof_every = every; c->prof_seen = 0;
  return MOT_OK;
}
extern "C" int mot_profile_read(mot_ctx* c, float* mean_ms, float* min_ms, float* max_ms, int* samples) {
  if (!c || !mean_ms || !samples) return MOT_E_ARG;
  MOT_GUARD(c);
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  double tot = 0; float mn = 1e30f, mx = 0;
  for (int i = 0; i < c->prof_n; i++) {
    float ms = 0;
    MOT_HIP(c, hipEventElapsedTime(&ms, c->prof_ev[i][0], c->prof_ev[i][1]));
    tot += ms; mn = ms < mn ? ms : mn; mx = ms > mx ? ms : mx;
  }
  *samples = c->prof_n;
  *mean_ms = c->prof_n ? (float)(tot / c->prof_n) : 0.f;
  if (min_ms) *min_ms = c->prof_n ? mn : 0.f;
  if (max_ms) *max_ms = mx;
  c->prof_n = 0;   // the ring fills again
  return MOT_OK;
}

// a slot's device-side capacity flags (read back with its counters) become MOT_E_CAPACITY. Reading does NOT clear them: the refusal belongs to the
// frame, and every getter answers it, however often, until a new stage call writes the slot — the flags are re-armed where a stage starts on
// it (the label kernel at the head of the box stage, inside the launch sequence and any graph captured from it; take_slot0 and
// ground_stage_slot0 for the stage-wise calls that put a new cloud into slot 0 without running the box stage).
static const char kMsgClusterOverflow[] = "more clusters in a frame than the library supports (4096)";
static int capacity_error(mot_ctx* c, int f) {
  if (f) {
    if (f & kFlagClusterOverflow) return fail(c, MOT_E_CAPACITY, kMsgClusterOverflow);
    if (f & kFlagBoxOverflow) return fail(c, MOT_E_CAPACITY, "more boxes in a frame than the library supports (1024)");
    if (f & kFlagHullOverflow) return fail(c, MOT_E_CAPACITY, "convex hull larger than 384 vertices");
    if (f & kFlagGroupOverflow) return fail(c, MOT_E_CAPACITY, "cloud too fragmented: more than max_points/2 (tile, cluster) groups in a frame");
    if (f & kFlagRngExhausted) return fail(c, MOT_E_CAPACITY, "L-shape sampling ran out of pre-generated random draws");
  }
  return MOT_OK;
}
// D2H of the per-frame counters (synchronises)
int fetch_counts(mot_ctx* c, int slot) {
  int* h = c->h_counts + slot * kCountsStride;
  MOT_HIP(c, hipMemcpyAsync(h, c->d_counts + slot * kCountsStride, kCountsStride * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  return capacity_error(c, h[kCntFlags]);
}

static int set_count(mot_ctx* c, int slot, int which, int value) {
  c->h_counts[slot * kCountsStride + which] = value;
  MOT_HIP(c, hipMemcpyAsync(c->d_counts + slot * kCountsStride + which, c->h_counts + slot * kCountsStride + which, sizeof(int),
                            hipMemcpyHostToDevice, c->stream));
  return MOT_OK;
}

// the argument checks the stage-wise cluster / box calls share (each with its own message)
static int check_cloud(mot_ctx* c, const float* elev, int n, bool others_ok, const char* msg) {
  if ((!elev && n > 0) || n < 0 || !others_ok) return fail(c, MOT_E_ARG, msg);
  if (n > c->max_points) return fail(c, MOT_E_CAPACITY, "cloud has more points than max_points");
  return MOT_OK;
}
// a stage-wise cluster / box call's own float4 cloud into slot 0, with_grid: and its label grid (already converted into h_grid16, each caller by its own rule)
static int take_slot0(mot_ctx* c, const float* elev, int n, bool with_grid) {
  if (n > 0) MOT_HIP(c, hipMemcpyAsync(c->d_elev, elev, (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
  if (with_grid) {
    MOT_HIP(c, hipMemcpyAsync(c->d_grid, c->h_grid16.data(), c->h_grid16.size() * sizeof(GridLabel), hipMemcpyHostToDevice, c->stream));
    MOT_HIP(c, hipStreamSynchronize(c->stream));   // (h_grid16 is reused by the next call)
  }
  c->res.slot0_taken();
  MOT_TRY(set_count(c, 0, kCntFlags, 0));   // a new cloud: the flags of the frame it replaces go with that frame
  return set_count(c, 0, kCntElev, n);
}

extern "C" int mot_get_clusters(mot_ctx* c, int slot, int32_t* grid, int* num_cluster, int32_t* point_label, int label_capacity) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (slot < 0 || slot >= c->batch) return fail(c, MOT_E_ARG, "slot out of range");
  MOT_TRY(fetch_counts(c, slot));
  const int G = c->params.num_grid;
  if (num_cluster) *num_cluster = c->h_counts[slot * kCountsStride + kCntClusters];
  int ne = c->h_counts[slot * kCountsStride + kCntElev];
  if (point_label && ne > label_capacity) return fail(c, MOT_E_CAPACITY, "more elevated points than the caller's label buffer holds");   // before any copy is queued: "nothing copied"
  if (grid) { c->h_grid16.resize((size_t)G * G); MOT_HIP(c, hipMemcpyAsync(c->h_grid16.data(), c->d_grid + (size_t)slot * MOT_MAX_GRID * MOT_MAX_GRID, (size_t)G * G * sizeof(GridLabel), hipMemcpyDeviceToHost, c->stream)); }
  if (point_label && ne > 0 && !c->res.labels_ready(slot)) {
    // the fused path left the per-point labels out (mot_set_fused_outputs): this slot's, from its cells and label grid
    ClusterBuffers cb = cluster_buffers(c, slot);
    cb.ecell = (c->res.cells_usable(slot) && c->params.num_grid < MOT_MAX_GRID) ? c->d_ecell : nullptr;
    mot_launch_point_labels(c->dp, cb, slot, ne, c->stream);
    MOT_HIP(c, hipGetLastError());
    c->res.labels_written(slot);
  }
  if (point_label && ne > 0) MOT_HIP(c, hipMemcpyAsync(point_label, c->d_label + (size_t)slot * c->cap, (size_t)ne * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  if (grid) for (size_t i = 0, n = (size_t)G * G; i < n; i++) grid[i] = (int32_t)c->h_grid16[i];   // the ABI's cartesianData is int32 (component_clustering.h:20-22)
  return MOT_OK;
}

extern "C" int mot_get_boxes(mot_ctx* c, int slot, float* boxes, int max_boxes, int* n_boxes, int32_t* box_cluster, int* n_undefined) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (slot < 0 || slot >= c->batch || max_boxes < 0) return fail(c, MOT_E_ARG, "mot_get_boxes: slot or max_boxes out of range");
  MOT_TRY(fetch_counts(c, slot));
  int nb = c->h_counts[slot * kCountsStride + kCntBoxes];
  if (n_boxes) *n_boxes = nb;
  if (n_undefined) *n_undefined = c->h_counts[slot * kCountsStride + kCntUndef];
  if (nb > max_boxes) return fail(c, MOT_E_CAPACITY, "more boxes than the caller's buffer holds");
  if (boxes && nb > 0) MOT_HIP(c, hipMemcpyAsync(boxes, c->d_boxes + (size_t)slot * kMaxBoxesPerFrame * 24, (size_t)nb * 24 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (box_cluster && nb > 0) MOT_HIP(c, hipMemcpyAsync(box_cluster, c->d_box_cluster + (size_t)slot * kMaxBoxesPerFrame, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  return MOT_OK;
}

extern "C" int mot_cluster(mot_ctx* c, const float* elev, int n, int32_t* grid, int* num_cluster, int32_t* point_label) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  MOT_TRY(check_cloud(c, elev, n, num_cluster != nullptr, "mot_cluster: null cloud / negative n / null num_cluster"));   // grid may be NULL: nothing but the count is read back
  MOT_TRY(take_slot0(c, elev, n, false));
  ClusterBuffers cb = cluster_buffers(c, 0);
  mot_launch_cluster(c->dp, cb, 1, n, c->stream);
  if (point_label) {  // getClusteredPoints' per-point lookup; the statistics it also gathers are discarded
    mot_launch_box_kernel(0, c->dp, cb, 1, n, c->stream);
    mot_launch_stats_init(cb, 1, c->stream);
    MOT_HIP(c, hipMemsetAsync(c->d_counts + kCntGroups, 0, 2 * sizeof(int), c->stream));   // kCntGroups, kCntIrregular
  }
  if (point_label) c->res.labels_written(0);
  MOT_HIP(c, hipGetLastError());
  return mot_get_clusters(c, 0, grid, num_cluster, point_label, n);
}

extern "C" int mot_box_fit(mot_ctx* c, const float* elev, int n, const int32_t* grid, int num_cluster, float* boxes, int max_boxes,
                           int* n_boxes, int32_t* box_cluster, int* n_undefined) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  MOT_TRY(check_cloud(c, elev, n, grid && num_cluster >= 0 && n_boxes, "mot_box_fit: null cloud / grid / n_boxes or a negative count"));
  if (num_cluster > kMaxClusters) return fail(c, MOT_E_CAPACITY, kMsgClusterOverflow);
  const int G = c->params.num_grid;
  // the caller's int32 grid onto the device's 16-bit one: a value outside 0 .. num_cluster names no cluster (getClusteredPoints indexes
  // its per-cluster vectors with it, box_fitting.cpp:59-66; the kernels treat it as "no label") and becomes 0
  c->h_grid16.resize((size_t)G * G);
  for (size_t i = 0, ng = (size_t)G * G; i < ng; i++) { const int32_t v = grid[i]; c->h_grid16[i] = (v < 0 || v > num_cluster) ? (GridLabel)0 : (GridLabel)v; }
  MOT_TRY(take_slot0(c, elev, n, true));
  MOT_TRY(set_count(c, 0, kCntClusters, num_cluster));
  launch_box_stage(c, cluster_buffers(c, 0), n);
  c->res.box_stage(0, c->point_order == MOT_ORDER_ANY);
  MOT_HIP(c, hipGetLastError());
  return mot_get_boxes(c, 0, boxes, max_boxes, n_boxes, box_cluster, n_undefined);
}

// boxFitting on the elevated cloud and label grid resident in slot 0 after mot_cluster (the host-buffer stage calls work on
// slot 0): no second upload of the cloud and the grid between the two stages of the cluster node
extern "C" int mot_box_fit_resident(mot_ctx* c, float* boxes, int max_boxes, int* n_boxes, int32_t* box_cluster, int* n_undefined) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (!n_boxes || max_boxes < 0) return fail(c, MOT_E_ARG, "mot_box_fit_resident: null n_boxes or negative max_boxes");
  MOT_TRY(fetch_counts(c, 0));
  const int n = c->h_counts[kCntElev];
  if (n < 0 || n > c->cap) return fail(c, MOT_E_STATE, "mot_box_fit_resident: no cloud resident in slot 0");
  if (c->h_counts[kCntClusters] > kMaxClusters) {
    // turned down before a kernel runs — and the refusal is left on the resident frame, as the kernels would have left it: every getter of slot 0
    // answers it from now on (fetch_counts), until a stage call puts a new cloud there
    MOT_TRY(set_count(c, 0, kCntFlags, kFlagClusterOverflow));
    return fail(c, MOT_E_CAPACITY, kMsgClusterOverflow);
  }
  launch_box_stage(c, cluster_buffers(c, 0), n);
  c->res.box_stage(0, c->point_order == MOT_ORDER_ANY);
  MOT_HIP(c, hipGetLastError());
  return mot_get_boxes(c, 0, boxes, max_boxes, n_boxes, box_cluster, n_undefined);
}

// fromROSMsg for PointXYZ (OT/src/groundremove/main.cpp:100), device to device
extern "C" int mot_decode_pointcloud2_dev(mot_ctx* c, const void* d_data, int n, int point_step, int off_x, int off_y, int off_z,
                                          int off_w, float* d_xyzw) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (n < 0 || (n > 0 && (!d_data || !d_xyzw)) || point_step < 12) return fail(c, MOT_E_ARG, "mot_decode_pointcloud2_dev: null buffer, negative n or point_step < 12");
  MOT_TRY(check_field_offsets(c, point_step, off_x, off_y, off_z, off_w));
  if (((size_t)d_xyzw & 15) != 0) return fail(c, MOT_E_ARG, "d_xyzw must be 16-byte aligned");
  mot_launch_decode_pointcloud2(d_data, n, point_step, off_x, off_y, off_z, off_w, (float4*)d_xyzw, c->stream);
  MOT_HIP(c, hipGetLastError());
  return MOT_OK;
}

// ------------------------------------------------------------------------------------------ side products
extern "C" int mot_side_params_default(mot_side_params* o) {
  if (!o) return MOT_E_ARG;
  memset(o, 0, sizeof *o);
  o->cell_size = 0.2f;                                                 // component_clustering.h:15
  o->cost_resolution = 1.0; o->cost_width = 50; o->cost_height = 50;   // component_clustering.cpp:15-17
  o->cost_offset_x = 0; o->cost_offset_y = 25;                         // :18-19
  o->height_limit = 0.1; o->car_length = 4.5; o->car_width = 2;        // :22-24
  o->cost_offset_z = -2;                                               // :20
  return MOT_OK;
}

constexpr int kMaxCostCells = 65536;
static int check_cost_map(mot_ctx* c, const mot_side_params* sp) {
  const bool ok = sp->cost_width >= 1 && sp->cost_height >= 1 && (long)sp->cost_width * sp->cost_height <= kMaxCostCells && sp->cost_resolution > 0;
  return ok ? MOT_OK : fail(c, MOT_E_ARG, "cost map must have 1..65536 cells and a positive resolution");
}
static int ensure_markers(mot_ctx* c) { MOT_TRY(dev_alloc(c, &c->d_markers, (size_t)kMaxBoxesPerFrame * 6 * sizeof(float))); return MOT_OK; }

static int side_setup(mot_ctx* c, int slot, const mot_side_params* sp, SideDevParams* dout, SideBuffers* sout) {
  // (a failure half-way — out of memory is plausible — leaves what exists for mot_destroy; the next call tries again from there)
  MOT_TRY(dev_alloc(c, &c->d_side_cell, (size_t)MOT_MAX_GRID * MOT_MAX_GRID * sizeof(int)));
  MOT_TRY(dev_alloc(c, &c->d_side_cloud, (size_t)c->cap * sizeof(float4)));
  MOT_TRY(dev_alloc(c, &c->d_side_obs, (size_t)MOT_MAX_GRID * MOT_MAX_GRID * sizeof(float4)));
  MOT_TRY(dev_alloc(c, &c->d_side_cost, (size_t)kMaxCostCells * sizeof(int)));
  MOT_TRY(dev_alloc(c, &c->d_side_counts, 2 * sizeof(int)));
  MOT_TRY(dev_alloc(c, &c->d_side_chunks, ((size_t)c->cap / 1024 + 1) * sizeof(int2)));
  SideDevParams d;
  d.cell_size = sp->cell_size; d.cost_width = sp->cost_width; d.cost_height = sp->cost_height; d.cost_resolution = sp->cost_resolution;
  d.center_x = (sp->cost_width / 2.0) * sp->cost_resolution - sp->cost_offset_x;    // map_center_x, :428
  d.center_y = (sp->cost_height / 2.0) * sp->cost_resolution - sp->cost_offset_y;   // map_center_y, :429
  d.height_limit = sp->height_limit; d.car_length = sp->car_length; d.car_width = sp->car_width;
  SideBuffers s;
  s.elevated = c->d_elev + (size_t)slot * c->cap; s.elevated_packed = c->res.elev_packed_at(slot) ? 1 : 0; s.grid = c->d_grid + (size_t)slot * MOT_MAX_GRID * MOT_MAX_GRID;
  s.counts = c->d_counts + (size_t)slot * kCountsStride; s.cell_first = c->d_side_cell; s.clustered = c->d_side_cloud;
  s.obstacles = c->d_side_obs; s.cost = c->d_side_cost; s.out_counts = c->d_side_counts; s.chunk_counts = c->d_side_chunks;
  s.max_clustered = c->cap; s.max_obstacles = MOT_MAX_GRID * MOT_MAX_GRID;
  *dout = d; *sout = s;
  return MOT_OK;
}

// makeClusteredCloud / setObsMsg / createCostMap, OT/src/cluster/component_clustering.cpp:311-379, 425-457
extern "C" int mot_cluster_products(mot_ctx* c, int slot, const mot_side_params* sp, float* clustered_xyzw, int max_clustered,
                                    int* n_clustered, float* obstacles_xyzc, int max_obstacles, int* n_obstacles, int32_t* cost_map) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (!sp || slot < 0 || slot >= c->batch || max_clustered < 0 || max_obstacles < 0) return fail(c, MOT_E_ARG, "mot_cluster_products: null parameters, slot or a capacity out of range");
  if ((clustered_xyzw && !n_clustered) || (obstacles_xyzc && !n_obstacles)) return fail(c, MOT_E_ARG, "mot_cluster_products: an output list needs its count pointer");
  MOT_TRY(check_cost_map(c, sp));
  MOT_TRY(fetch_counts(c, slot));   // a frame the box stage refused is refused here as well: nothing of it is delivered
  SideDevParams d; SideBuffers s;
  MOT_TRY(side_setup(c, slot, sp, &d, &s));
  mot_launch_side_products(c->dp, d, s, c->cap, c->stream);
  MOT_HIP(c, hipGetLastError());
  char* pin;
  MOT_TRY(pinned_scratch(c, 64, &pin));
  int* h = reinterpret_cast<int*>(pin);
  MOT_HIP(c, hipMemcpyAsync(h, c->d_side_counts, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  if (n_clustered) *n_clustered = h[0];
  if (n_obstacles) *n_obstacles = h[1];
  if ((clustered_xyzw && h[0] > max_clustered) || (obstacles_xyzc && h[1] > max_obstacles))
    return fail(c, MOT_E_CAPACITY, "more clustered points / obstacles than the caller's buffer holds");
  if (clustered_xyzw && h[0] > 0) MOT_HIP(c, hipMemcpyAsync(clustered_xyzw, c->d_side_cloud, (size_t)h[0] * 16, hipMemcpyDeviceToHost, c->stream));
  if (obstacles_xyzc && h[1] > 0) MOT_HIP(c, hipMemcpyAsync(obstacles_xyzc, c->d_side_obs, (size_t)h[1] * 16, hipMemcpyDeviceToHost, c->stream));
  if (cost_map) MOT_HIP(c, hipMemcpyAsync(cost_map, c->d_side_cost, (size_t)sp->cost_width * sp->cost_height * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  return MOT_OK;
}

extern "C" int mot_cluster_products_host(mot_ctx* c, const float* elev, int n, const int32_t* grid, const mot_side_params* sp,
                                         float* clustered_xyzw, int max_clustered, int* n_clustered, float* obstacles_xyzc,
                                         int max_obstacles, int* n_obstacles, int32_t* cost_map) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  MOT_TRY(check_cloud(c, elev, n, grid != nullptr, "mot_cluster_products_host: null cloud / grid or negative n"));
  const int G = c->params.num_grid;
  // the caller's int32 grid onto the device's 16-bit one. componentClustering's labels are 0 .. numCluster <= 32 768; the three functions replaced
  // here use a label only as "!= 0" and as the obstacle's cluster id, so anything outside 0 .. 65 535 is not a label grid (checked before anything
  // of slot 0 is overwritten)
  c->h_grid16.resize((size_t)G * G);
  for (size_t i = 0, ng = (size_t)G * G; i < ng; i++) {
    if (grid[i] < 0 || grid[i] > 65535) return fail(c, MOT_E_ARG, "mot_cluster_products_host: grid labels must lie in 0 .. 65535");
    c->h_grid16[i] = (GridLabel)grid[i];
  }
  MOT_TRY(take_slot0(c, elev, n, true));   // (the labels of the slot's previous cloud go with it: mot_get_clusters recomputes them from this cloud and this grid)
  return mot_cluster_products(c, 0, sp, clustered_xyzw, max_clustered, n_clustered, obstacles_xyzc, max_obstacles, n_obstacles, cost_map);
}

// mark_cluster() for every box of the slot's last box stage (OT/src/cluster/box_fitting.cpp:161-209, :410): what the cluster node's rviz CUBE
// markers are made of, from the cloud and the cluster-ordered groups still resident in HBM
extern "C" int mot_box_markers(mot_ctx* c, int slot, float* centroid_extent, int max_boxes, int* n_boxes) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (slot < 0 || slot >= c->batch || max_boxes < 0 || !n_boxes) return fail(c, MOT_E_ARG, "mot_box_markers: slot or max_boxes out of range, or null n_boxes");
  MOT_TRY(fetch_counts(c, slot));   // (a refused frame first, with the limit's message like every other getter: its cluster order is incomplete or absent)
  if (!c->res.boxes_valid(slot)) return fail(c, MOT_E_STATE, "mot_box_markers: no box stage has run on the cloud now resident in this slot (a stage-wise call replaced it since)");
  const int nb = c->h_counts[slot * kCountsStride + kCntBoxes];
  *n_boxes = nb;
  if (nb > max_boxes) return fail(c, MOT_E_CAPACITY, "more boxes than the caller's buffer holds");
  if (nb == 0 || !centroid_extent) return MOT_OK;
  MOT_TRY(ensure_markers(c));
  mot_launch_box_markers(box_products(c, slot), slot, nb < kMaxBoxesPerFrame ? nb : kMaxBoxesPerFrame, c->d_markers, c->stream);
  MOT_HIP(c, hipGetLastError());
  MOT_HIP(c, hipMemcpyAsync(centroid_extent, c->d_markers, (size_t)nb * 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  return MOT_OK;
}

// The cluster node's whole callback in one call (include/mot.h): upload, labelling, side products, box fit and cubes queued back to back on
// the resident cloud; the counts come back first (one small copy + synchronisation), then every result in one batch of copies into the
// context's page-locked block (second synchronisation). Same kernels as the call-by-call entry points.
extern "C" int mot_cluster_node_frame(mot_ctx* c, const float* elev, int n, const mot_side_params* sp, mot_cluster_frame* out) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  MOT_TRY(check_cloud(c, elev, n, sp && out, "mot_cluster_node_frame: null cloud / parameters / result, or negative n"));
  MOT_TRY(check_cost_map(c, sp));
  memset(out, 0, sizeof *out);
  SideDevParams d; SideBuffers s;
  MOT_TRY(side_setup(c, 0, sp, &d, &s));
  MOT_TRY(ensure_markers(c));
  const size_t cost_cells = (size_t)sp->cost_width * sp->cost_height;
  // the page-locked block: [counts 64 B][clustered n x 16][obstacles min(n, G^2) x 16][cost map][boxes][box clusters][cubes]
  const size_t G2 = (size_t)c->params.num_grid * c->params.num_grid, max_obs = (size_t)n < G2 ? (size_t)n : G2;
  const size_t o_cc = 64, o_ob = o_cc + (size_t)n * 16, o_cm = o_ob + max_obs * 16, o_bx = o_cm + cost_cells * sizeof(int),
               o_bc = o_bx + (size_t)kMaxBoxesPerFrame * 24 * sizeof(float), o_mk = o_bc + (size_t)kMaxBoxesPerFrame * sizeof(int),
               total = o_mk + (size_t)kMaxBoxesPerFrame * 6 * sizeof(float);
  char* pin;
  MOT_TRY(pinned_scratch(c, total, &pin));
  MOT_TRY(take_slot0(c, elev, n, false));   // (nothing of this frame is vouched for until the device's flags say that it fit: below)
  s.elevated_packed = 0;   // (side_setup looked at slot 0 BEFORE the upload: after a fused batch on this context it saw 12-byte points there)
  ClusterBuffers cb = cluster_buffers(c, 0);
  mot_launch_cluster(c->dp, cb, 1, n, c->stream);
  mot_launch_side_products(c->dp, d, s, n > 0 ? n : 1, c->stream);
  const ClusterBuffers products = launch_box_stage(c, cb, n);
  mot_launch_box_markers(products, 0, kMaxBoxesPerFrame, c->d_markers, c->stream);   // (the box count is still on the device: workgroups beyond it leave at once)
  MOT_HIP(c, hipGetLastError());
  int* h = reinterpret_cast<int*>(pin);
  MOT_HIP(c, hipMemcpyAsync(h, c->d_counts, kCountsStride * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipMemcpyAsync(h + kCountsStride, c->d_side_counts, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  memcpy(c->h_counts, h, kCountsStride * sizeof(int));
  MOT_TRY(capacity_error(c, h[kCntFlags]));
  const int ncc = h[kCountsStride], nob = h[kCountsStride + 1], nb = h[kCntBoxes];
  if (ncc < 0 || ncc > n || nob < 0 || (size_t)nob > max_obs || nb < 0 || nb > kMaxBoxesPerFrame) return fail(c, MOT_E_STATE, "mot_cluster_node_frame: inconsistent counts");
  c->res.box_stage(0, c->point_order == MOT_ORDER_ANY);   // no overflow: slot 0 holds this cloud's labels and boxes
  if (ncc > 0) MOT_HIP(c, hipMemcpyAsync(pin + o_cc, c->d_side_cloud, (size_t)ncc * 16, hipMemcpyDeviceToHost, c->stream));
  if (nob > 0) MOT_HIP(c, hipMemcpyAsync(pin + o_ob, c->d_side_obs, (size_t)nob * 16, hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipMemcpyAsync(pin + o_cm, c->d_side_cost, cost_cells * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (nb > 0) {
    MOT_HIP(c, hipMemcpyAsync(pin + o_bx, c->d_boxes, (size_t)nb * 24 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    MOT_HIP(c, hipMemcpyAsync(pin + o_bc, c->d_box_cluster, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    MOT_HIP(c, hipMemcpyAsync(pin + o_mk, c->d_markers, (size_t)nb * 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  out->num_cluster = h[kCntClusters]; out->n_clustered = ncc; out->n_obstacles = nob; out->n_boxes = nb; out->n_undefined = h[kCntUndef];
  out->cost_cells = (int32_t)cost_cells;
  out->clustered_xyzw = reinterpret_cast<const float*>(pin + o_cc); out->obstacles_xyzc = reinterpret_cast<const float*>(pin + o_ob);
  out->cost_map = reinterpret_cast<const int32_t*>(pin + o_cm); out->boxes = reinterpret_cast<const float*>(pin + o_bx);
  out->box_cluster = reinterpret_cast<const int32_t*>(pin + o_bc); out->centroid_extent = reinterpret_cast<const float*>(pin + o_mk);
  return MOT_OK;
}

extern "C" int mot_get_ground(mot_ctx* c, int slot, float* elev, int* n_elev, float* ground, int* n_ground,
                              uint8_t* mask, int capacity_points) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (slot < 0 || slot >= c->batch) return fail(c, MOT_E_ARG, "slot out of range");
  MOT_TRY(fetch_counts(c, slot));
  int ne = c->h_counts[slot * kCountsStride + kCntElev], ng = c->h_counts[slot * kCountsStride + kCntGround];
  if (n_elev) *n_elev = ne;
  if (n_ground) *n_ground = ng;
  if ((elev && ne > capacity_points) || (ground && ng > capacity_points) || (mask && c->h_n[slot] > capacity_points))
    return fail(c, MOT_E_CAPACITY, "more points resident than the caller's buffers hold (capacity_points)");
  // (known, kept as it is: the counts above are written and the capacity tested before this refusal)
  if (c->res.ground_foreign(slot) && (elev || ground || mask))
    return fail(c, MOT_E_STATE, "mot_get_ground: a stage-wise cluster / box call has put its own cloud into slot 0 since the ground stage ran: no ground result of that cloud is resident");
  if (((ground || mask) && !c->res.ground_readable(slot)) || (elev && c->res.elev_packed_at(slot))) {   // (packed: the fused path left 12-byte points; the ABI's records are float4 with the input's 4th value)
    // The fused path left the ground cloud / mask out (mot_set_fused_outputs): materialise them for the whole last batch by
    // re-running the compaction with every output, from the batch's input, polar cells and thresholds — all still resident.
    // (No occupancy this time: the cluster stage has consumed it. The elevated cloud and the counts are rewritten with the
    // same values.)
    if (!c->res.can_rebuild_ground(slot)) return fail(c, MOT_E_STATE, "mot_get_ground: no ground result resident");
    MOT_TRY(next_epoch(c));
    GroundBuffers g = ground_buffers(c, c->res.last_in, c->res.last_in_stride, true, false);
    mot_launch_ground_kernel(2, c->dp, g, c->res.last_batch, c->res.last_max_n, c->stream);
    MOT_HIP(c, hipGetLastError());
    c->res.compaction_rerun(c->res.last_batch, false, true);   // every slot's elevated cloud is float4 again
  }
  if (elev && ne > 0) MOT_HIP(c, hipMemcpyAsync(elev, c->d_elev + (size_t)slot * c->cap, (size_t)ne * 16, hipMemcpyDeviceToHost, c->stream));
  if (ground && ng > 0) MOT_HIP(c, hipMemcpyAsync(ground, c->d_ground + (size_t)slot * c->cap, (size_t)ng * 16, hipMemcpyDeviceToHost, c->stream));
  if (mask && c->h_n[slot] > 0) MOT_HIP(c, hipMemcpyAsync(mask, c->d_mask + (size_t)slot * c->cap, (size_t)c->h_n[slot], hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  return MOT_OK;
}

// the stage-wise ground stage on the cloud a caller has put into d_in (slot 0)
static int ground_stage_slot0(mot_ctx* c, int n, bool want_mask) {
  MOT_TRY(set_batch(c, &n, 1, c->d_in, c->cap));
  MOT_TRY(next_epoch(c));
  MOT_TRY(set_count(c, 0, kCntFlags, 0));   // a new cloud in slot 0: the flags of the frame it replaces go with that frame
  GroundBuffers g = ground_buffers(c, c->d_in, c->cap, want_mask);
  mot_launch_ground(c->dp, g, 1, n, c->stream);
  MOT_HIP(c, hipGetLastError());
  c->res.ground_stage(want_mask);
  return MOT_OK;
}

extern "C" int mot_ground_remove(mot_ctx* c, const float* xyzw, int n, float* elev, int* n_elev, float* ground,
                                 int* n_ground, uint8_t* mask) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if ((!xyzw && n > 0) || n < 0) return fail(c, MOT_E_ARG, "mot_ground_remove: null cloud or negative n");
  if (n > c->max_points) return fail(c, MOT_E_CAPACITY, "frame has more points than max_points");
  if (n > 0) MOT_HIP(c, hipMemcpyAsync(c->d_in, xyzw, (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
  MOT_TRY(ground_stage_slot0(c, n, true));
  return mot_get_ground(c, 0, elev, n_elev, ground, n_ground, mask, n);
}

// mot_ground_remove with the two clouds left in the context's page-locked block (include/mot.h)
extern "C" int mot_ground_node_frame(mot_ctx* c, const float* xyzw, int n, const float** elev, int* n_elev, const float** ground, int* n_ground) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if ((!xyzw && n > 0) || n < 0 || !elev || !n_elev || !ground || !n_ground) return fail(c, MOT_E_ARG, "mot_ground_node_frame: null cloud / result pointers or negative n");
  if (n > c->max_points) return fail(c, MOT_E_CAPACITY, "frame has more points than max_points");
  char* pin;
  MOT_TRY(pinned_scratch(c, 64 + 2 * (size_t)n * 16, &pin));
  if (n > 0) MOT_HIP(c, hipMemcpyAsync(c->d_in, xyzw, (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
  MOT_TRY(ground_stage_slot0(c, n, false));
  MOT_TRY(fetch_counts(c, 0));
  const int ne = c->h_counts[kCntElev], ng = c->h_counts[kCntGround];
  if (ne < 0 || ng < 0 || ne + ng > n) return fail(c, MOT_E_STATE, "mot_ground_node_frame: inconsistent counts");
  if (ne > 0) MOT_HIP(c, hipMemcpyAsync(pin + 64, c->d_elev, (size_t)ne * 16, hipMemcpyDeviceToHost, c->stream));
  if (ng > 0) MOT_HIP(c, hipMemcpyAsync(pin + 64 + (size_t)ne * 16, c->d_ground, (size_t)ng * 16, hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  *elev = reinterpret_cast<const float*>(pin + 64); *n_elev = ne;
  *ground = reinterpret_cast<const float*>(pin + 64 + (size_t)ne * 16); *n_ground = ng;
  return MOT_OK;
}

// one H2D of the raw PointCloud2 records of a frame into the staging buffer, unpacked on the device into the context's own
// input buffer (slot 0), 4th float = 1.0f
static int upload_pointcloud2(mot_ctx* c, const void* data, int n, int point_step, int off_x, int off_y, int off_z) {
  if (n < 0 || (n > 0 && !data) || point_step < 12) return fail(c, MOT_E_ARG, "PointCloud2 payload: null data, negative n or point_step < 12");
  if (n > c->max_points) return fail(c, MOT_E_CAPACITY, "frame has more points than max_points");
  MOT_TRY(check_field_offsets(c, point_step, off_x, off_y, off_z, -1));
  const size_t bytes = (size_t)n * (size_t)point_step;
  if (bytes > c->raw_bytes) {
    if (c->d_raw) { MOT_HIP(c, hipStreamSynchronize(c->stream)); MOT_TRY(release(c, &c->d_raw)); c->raw_bytes = 0; }
    MOT_TRY(dev_alloc(c, &c->d_raw, bytes));
    c->raw_bytes = bytes;
  }
  if (n > 0) {
    MOT_HIP(c, hipMemcpyAsync(c->d_raw, data, bytes, hipMemcpyHostToDevice, c->stream));
    mot_launch_decode_pointcloud2(c->d_raw, n, point_step, off_x, off_y, off_z, -1, (float4*)c->d_in, c->stream);
  }
  return MOT_OK;
}

// fromROSMsg + groundRemove for a message payload in host memory
extern "C" int mot_ground_remove_pointcloud2(mot_ctx* c, const void* data, int n, int point_step, int off_x, int off_y, int off_z,
                                             float* elev, int* n_elev, float* ground, int* n_ground, uint8_t* mask) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  MOT_TRY(upload_pointcloud2(c, data, n, point_step, off_x, off_y, off_z));
  MOT_TRY(ground_stage_slot0(c, n, true));
  return mot_get_ground(c, 0, elev, n_elev, ground, n_ground, mask, n);
}

// the whole stateless chain of a frame (what OT0/src/main.cpp:57-88 runs in one process) on a message payload in host memory:
// the cloud is uploaded once and never leaves HBM between the stages
extern "C" int mot_frame_pointcloud2(mot_ctx* c, const void* data, int n, int point_step, int off_x, int off_y, int off_z) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  MOT_TRY(upload_pointcloud2(c, data, n, point_step, off_x, off_y, off_z));
  return mot_frames_dev(c, (const float*)c->d_in, (long)c->cap * 4, &n, 1, 0, nullptr, nullptr, nullptr);
}

static int launch_one(mot_ctx* c, int id, int batch) {
  const int max_n = c->res.last_max_n;
  if (id == kK3) MOT_TRY(next_epoch(c));
  if (id == kK3) c->res.compaction_rerun(batch, Residency::fused_packs(c->fused_outputs), Residency::fused_keeps_ground(c->fused_outputs));
  GroundBuffers g; ClusterBuffers cb;
  fused_buffers(c, &g, &cb);   // as in the fused path
  const bool any = c->point_order == MOT_ORDER_ANY;
  const ClusterBuffers src = cb;           // the frame as the cluster stage left it: what the regrouping pass reads
  if (any && id >= kB1 && id <= kB1b) cb = regrouped_view(c, cb);
  switch (id) {
    case kK1: mot_launch_ground_kernel(0, c->dp, g, batch, max_n, c->stream); break;
    case kK2: mot_launch_ground_kernel(1, c->dp, g, batch, max_n, c->stream); break;
    case kK3: mot_launch_ground_kernel(2, c->dp, g, batch, max_n, c->stream); break;
    case kC2: mot_launch_cluster_kernel(1, c->dp, cb, batch, max_n, c->stream); break;
    case kB1: mot_launch_box_kernel(0, c->dp, cb, batch, max_n, c->stream); if (!any) for (int b = 0; b < batch; b++) c->res.labels_written(b, cb.label != nullptr); break;   // (MOT_ORDER_ANY: the labels are the regrouping pass's)
    case kB2: mot_launch_box_kernel(1, c->dp, cb, batch, max_n, c->stream); break;
    case kB3: mot_launch_box_kernel(2, c->dp, cb, batch, max_n, c->stream); break;
    case kB2b: mot_launch_box_kernel(3, c->dp, cb, batch, max_n, c->stream); break;
    case kB1b: mot_launch_box_kernel(4, c->dp, cb, batch, max_n, c->stream); break;
    case kR1: case kR2: case kR3: mot_launch_regroup(id - kR1, c->dp, src, fused_regroup_buffers(c), batch, max_n, c->stream); break;
    case kT1: mot_launch_track(track_buffers(c, true), batch, c->stream); break;  // last frame's arguments again
    default: return fail(c, MOT_E_ARG, "unknown kernel id");
  }
  return MOT_OK;
}

// Re-runs a stage (0 ground, 1 cluster, 2 box, 100 all three) or one kernel (10-12, 20-21, 30-32) on the data
// resident from the last mot_frames_dev call. Each iteration launches the untimed kernels the timed ones need
// (e.g. the occupancy kernel before the labelling kernel, which consumes and clears the bit-planes), records a
// HIP event on the context stream, launches the timed kernels, records a second event, and synchronises;
// the result is the mean of the event-to-event times. Every sequence leaves the context in its between-calls state.
extern "C" int mot_time_stage(mot_ctx* c, int stage, int batch, int iters, float* ms_per_iter) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (!ms_per_iter || iters < 1) return fail(c, MOT_E_ARG, "mot_time_stage: null result pointer or iters < 1");
  if (!c->res.last_in || batch != c->res.last_batch) return fail(c, MOT_E_STATE, "call mot_frames_dev with the same batch first");
  // MOT_ORDER_ANY: the box stage includes the regrouping pass (35-37), and its kernels run on the copy that pass left — which must be the last batch's
  const bool any = c->point_order == MOT_ORDER_ANY;
  if ((stage == 2 || stage == 100 || (stage >= kB1 && stage <= kR3)) && any != c->res.regrouped(0)) return fail(c, MOT_E_STATE, "mot_time_stage: call mot_frames_dev in the current point order first");
  if (stage >= kR1 && stage <= kR3 && !any) return fail(c, MOT_E_STATE, "mot_time_stage: kernels 35-37 exist in MOT_ORDER_ANY only");
  struct Seq { int pre[4], timed[12], post[3]; };
  Seq s = {{0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0}};
  switch (stage) {
    // (the compaction kernel K3 leaves the occupancy lists the labelling kernel C2 folds; the stand-alone occupancy kernel
    // of the stage-wise mot_cluster is not timed here)
    case 0: s = {{0}, {kK1, kK2, kK3}, {kC2}}; break;
    case 1: s = {{kK3}, {kC2}, {0}}; break;
    case 2: if (any) s = {{0}, {kR1, kR2, kR3, kB1, kB1b, kB2, kB2b, kB3}, {0}}; else s = {{0}, {kB1, kB1b, kB2, kB2b, kB3}, {0}}; break;
    case 100: if (any) s = {{0}, {kK1, kK2, kK3, kC2, kR1, kR2, kR3, kB1, kB1b, kB2, kB2b, kB3}, {0}}; else s = {{0}, {kK1, kK2, kK3, kC2, kB1, kB1b, kB2, kB2b, kB3}, {0}}; break;
    case kK1: s = {{0}, {kK1}, {0}}; break;
    case kK2: s = {{0}, {kK2}, {0}}; break;
    case kK3: s = {{0}, {kK3}, {kC2}}; break;
    case kC2: s = {{kK3}, {kC2}, {0}}; break;
    case kB1: s = {{0}, {kB1}, {kB1b, kB3}}; break;
    case kB1b: s = {{kB1}, {kB1b}, {kB3}}; break;
    case kB2: s = {{kB1, kB1b}, {kB2}, {kB3}}; break;
    case kB2b: s = {{kB1, kB1b, kB2}, {kB2b}, {kB3}}; break;
    case kB3: s = {{kB1, kB1b, kB2, kB2b}, {kB3}, {0}}; break;
    // (the regrouping kernels hand the chunk histograms on: 35 leaves the low digit's counts, 36 scans them IN PLACE into offsets and leaves the high digit's
    // offsets, which 37 scatters by. Each is therefore timed behind the ones before it and followed by the ones after it: the cluster-ordered copy the slots vouch for is whole again)
    case kR1: s = {{0}, {kR1}, {kR2, kR3}}; break;
    case kR2: s = {{kR1}, {kR2}, {kR3}}; break;
    case kR3: s = {{kR1, kR2}, {kR3}, {0}}; break;
    case kT1: s = {{0}, {kT1}, {0}}; break;
    default: return fail(c, MOT_E_ARG, "unknown stage");
  }
  double total = 0;
  for (int it = 0; it < iters; it++) {
    for (int k = 0; k < 4 && s.pre[k]; k++) MOT_TRY(launch_one(c, s.pre[k], batch));
    MOT_HIP(c, hipEventRecord(c->ev0, c->stream));
    for (int k = 0; k < 12 && s.timed[k]; k++) MOT_TRY(launch_one(c, s.timed[k], batch));
    MOT_HIP(c, hipEventRecord(c->ev1, c->stream));
    for (int k = 0; k < 3 && s.post[k]; k++) MOT_TRY(launch_one(c, s.post[k], batch));
    MOT_HIP(c, hipEventSynchronize(c->ev1));
    float ms = 0;
    MOT_HIP(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    total += ms;
  }
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  MOT_HIP(c, hipGetLastError());
  *ms_per_iter = (float)(total / iters);
  return MOT_OK;
}

// internal debugging aid (not part of include/mot.h): raw copy of a per-slot device array to the host
extern "C" int mot_debug_copy(mot_ctx* c, int which, int slot, void* dst, size_t bytes) {
  if (!c || !dst || slot < 0 || slot >= c->batch) return MOT_E_ARG;
  MOT_GUARD(c);
  const void* src = nullptr;
  if (which == 0) src = c->d_cand + (size_t)slot * kMaxClusters;
  else if (which == 1) src = c->d_stats + (size_t)slot * kMaxClusters;
  else if (which == 3) src = c->d_poly + (size_t)slot * c->cap;
  else if (which == 5) { const ClusterBuffers v = box_products(c, slot); src = v.gsorted + (size_t)slot * v.group_cap; }   // (the buffers and stride of the mode the slot's box stage ran in)
  else if (which == 7) src = c->d_cluster_start + (size_t)slot * (kMaxClusters + 1);
  else if (which == 8) src = c->d_pix + (size_t)slot * c->cap;
  else if (which == 9) { const ClusterBuffers v = box_products(c, slot); src = v.groups + (size_t)slot * v.group_cap; }
  else if (which == 10) src = c->d_hg + (size_t)slot * MOT_POLAR_CELLS;
  else if (which == 11) src = c->d_tboxes + (size_t)slot * kMaxBoxesPerFrame * 24;
  else if (which == 12) src = reinterpret_cast<const long long*>(c->d_items) + (size_t)slot * 32;   // -DMOT_DBG_STREAM_TIMING builds: phase clocks of track_step_stream_kernel
  else if (which == 13) src = c->d_cluster_gstart + (size_t)slot * (kMaxClusters + 1);
  else if (which == 14) src = c->d_elev + (size_t)slot * c->cap;    // as the last compaction left it: 12-byte points behind the fused path's default, float4 records otherwise
  else if (which == 15) src = c->d_mask + (size_t)slot * c->cap;
  else if (which == 16) src = c->d_gzmax + (size_t)slot * (c->cap / 8);
  else if (which == 17) src = c->d_cell + (size_t)slot * c->cap;
  else return MOT_E_ARG;
  MOT_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  return MOT_OK;
}

// test hook (mot_debug_api.h): the context's device parameters, for the fast-path sweeps of tests/devcheck (a library of their own)
// MEASUREMENT ONLY (tools/, bench.py MOT_BENCH_SKIP): leaves launches of the fused sequence out — 1 polar_filter, 2 ccl, 4 cluster_index, 8 box_finalize_prep,
// 32 the tracker (the frame's results are stale / wrong while one of these bits is set: on a moving scene stale thresholds change the WORKLOAD, so these bound
// nothing — profiles/r06_launch_boundaries.md); bits 8-11: a count of extra EMPTY launches per sequence (results unaffected): the cost of a launch boundary.
extern "C" int mot_debug_skip_kernels(mot_ctx* c, int mask) {
  if (!c) return MOT_E_ARG;
  c->dbg_skip = mask;
  return MOT_OK;
}

extern "C" int mot_debug_dev_params(mot_ctx* c, void* dst, size_t bytes) {
  if (!c || !dst || bytes < sizeof(MotDevParams)) return MOT_E_ARG;
  memcpy(dst, &c->dp, sizeof(MotDevParams));
  return MOT_OK;
}
