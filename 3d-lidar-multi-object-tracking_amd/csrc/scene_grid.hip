// scene_grid.hip — a rolling static-scene grid per stream, movers kept apart, on gfx950. Product code (HIP, wave64).
//
// The scene-side twin of the per-track accumulators (track_accum.hip): per stream a W x W occupancy grid in the tracker's global frame, centred on the vehicle,
// that takes every elevated point of a fused step and counts it as STATIC (no owner, or an owner the tracker has flagged static) or DYNAMIC (every other owner).
// The reference's createCostMap (cluster node) is a 50 x 50 per-frame cost map without memory and without tracks; it has no such output.
//
//   G0  scene_scroll_kernel   grid (kSceneScrollBlocks, B): every workgroup computes the slot's new window from the matrix and reads the previous origin; together they
//                             clear the columns and rows of the torus that ENTERED the window (everything when the shift is >= W on an axis); workgroup 0 writes the
//                             header (origin, stamp, the three counters at 0) and the window's validity. Nobody writes what another workgroup of the launch reads:
//                             the previous origin is moved on by G1
//   G1  scene_splat_kernel    grid (ceil(N_e / 2048), B), 256 threads, 8 points a thread: per point one 12-byte load (16 in the float4 layout), one 4-byte id load, the
//                             transform, the cell test, and for an owned point the two dependent gathers id -> track slot -> is_static (track_accum_plan's reads).
//                             Then, wave by wave, ONE lane per run of neighbouring lanes with the same (cell, kind) adds the run's length and its largest z
//                             (MOT_SCENE_MERGE, below); the three counters of the step are summed per wave first. Workgroup (0, b) moves the previous origin on.
//                             The kernel decides the slot's window, validity, stamp and cells and moves the origin on; everything per point is scene_splat_body of
//                             mot_scene_splat.h (kind: SceneKindLive), the ONE body it shares with scene_seq_splat_kernel of scene_grid_seq.hip
//   G2  scene_export_kernel   the torus unrolled into the caller's block, one 16-byte load and one 16-byte store a cell; the z image converted; the header copied
//   --  scene_reset_kernel    headers and previous origins of a run of slots back to "no step yet" (the setter, the resets, mot_stream_load; the cells by a memset)
//
// INTEGER ATOMICS ONLY: atomicAdd on the two hit counters, atomicMax on the order-preserving unsigned image of z (mot_float_key with the sign bit flipped: every finite z maps
// above 0, so 0 is "none yet" and an empty cell is 16 zero bytes), a plain store for last_seen (every writer of a step stores the same value), integer adds for
// the header's counters. Sums and maxima of integers do not depend on the order of arrival: the grid is byte-identical from run to run, whatever the order of workgroups.
// RUN MERGING. Atomics execute at the memory side; 64 lanes into 64 different lines run an order of magnitude below the streaming rate, so the atomics, not the 16
// bytes read per point, set this kernel's time. In scan order neighbouring lanes mostly hit the same cell with the same kind: heads of runs are found with one
// shuffle and one ballot per 64 points, the run's maximum with six masked shuffles (a run may span the wave; -DMOT_SCENE_RUN=16 ends runs at multiples of 16 lanes and
// needs four). -DMOT_SCENE_MERGE=0 builds the plain form (one lane, one set of atomics) for tools/time_scene_grid.py; all forms give the same bytes. Measured
// (profiles/scene_grid.md, 512 streams x 120 k points): plain 2.0 ms, runs of 16 0.55 ms, runs of 64 0.52 ms a call.
// INDEX SAFETY. A point takes part only with |t| < 2^30 per axis, so floorf(t) converts exactly and cell - origin cannot overflow (origins lie within 2^30 + W / 2); the
// storage index is (gi & (W - 1)) + (gj & (W - 1)) * W < W^2 by construction, the slot offset b * W^2 with b below the launch's batch <= max_batch. Point and id loads stay
// below min(count, cap) of the slot; an id outside [0, E) or a track slot outside [0, T) is not followed (the point then counts as dynamic: an owner that is not static).
// Resources (tools/kernel_resources.py): no LDS, no scratch.
#include "mot_scene_splat.h"   // the window rule, the kind rules, the per-point step, the merged adds and the splat body, shared with scene_grid_seq.hip

static_assert(sizeof(mot_scene_cell) == 16 && sizeof(SceneCell) == 16 && sizeof(mot_scene_header) == 32 && sizeof(SceneWindow) == 16, "include/mot.h documents the sizes");

// ------------------------------------------------------------------------------------------ G0
__global__ void MOT_SG_BOUNDS(kSceneBlock)
scene_scroll_kernel(SceneGridBuffers g, int b0, const EgoTf* __restrict__ tf, const int* __restrict__ steps) {
  const int kb = blockIdx.y, b = b0 + kb, tid = threadIdx.x;
  const int W = g.W;
  const int old_oi = g.prev[b].oi, old_oj = g.prev[b].oj;   // (not .ok: workgroup 0 writes it)
  int oi = old_oi, oj = old_oj;
  const bool ok = scene_window(tf[kb], g.inv, W, &oi, &oj);
  if (blockIdx.x == 0 && tid == 0) {
    mot_scene_header h;
    h.origin_i = oi; h.origin_j = oj; h.step = steps[kb]; h.size = W; h.n_static = 0; h.n_dynamic = 0; h.n_outside = 0; h.cell = g.cell;
    g.hdr[b] = h;
    g.prev[b].ok = ok ? 1 : 0;   // (a word no workgroup of this launch reads; G1 moves oi / oj on)
  }
  // columns / rows of the new window that the old one did not hold; a window kept as it was (ok == false) gives 0 and 0
  const long long di = (long long)oi - old_oi, dj = (long long)oj - old_oj;
  const int ni = (int)(di < 0 ? (-di > W ? W : -di) : (di > W ? W : di)), nj = (int)(dj < 0 ? (-dj > W ? W : -dj) : (dj > W ? W : dj));
  const int ci0 = di > 0 ? oi + W - ni : oi, cj0 = dj > 0 ? oj + W - nj : oj;   // first entering global column / row
  const long total = ((long)ni + nj) * W;
  const int lw = g.log2_W;
  uint4* __restrict__ cells = reinterpret_cast<uint4*>(g.cells + (long)b * W * W);
  uint4 zero;
  zero.x = 0u; zero.y = 0u; zero.z = 0u; zero.w = 0u;
  for (long k = (long)blockIdx.x * kSceneBlock + tid; k < total; k += (long)gridDim.x * kSceneBlock) {
    const int q = (int)(k >> lw), r = (int)(k & (W - 1));
    int si, sj;
    if (q < ni) { si = (ci0 + q) & (W - 1); sj = r; }        // an entering column, every row of it
    else { si = r; sj = (cj0 + (q - ni)) & (W - 1); }        // an entering row, every column of it
    cells[(long)sj * W + si] = zero;
  }
}

// ------------------------------------------------------------------------------------------ G1
__global__ void MOT_SG_BOUNDS(kSceneBlock)
scene_splat_kernel(SceneGridBuffers g, SceneSplatInput in, int b0, const EgoTf* __restrict__ tf, const int* __restrict__ steps) {
  const int kb = blockIdx.y, b = b0 + kb;
  const int W = g.W;
  mot_scene_header* __restrict__ hdr = g.hdr + b;
  const int oi = hdr->origin_i, oj = hdr->origin_j;
  if (blockIdx.x == 0 && threadIdx.x == 0) { g.prev[b].oi = oi; g.prev[b].oj = oj; }   // (G0 of the next step reads them; nobody in this launch does)
  const SceneRect window = {oi, oi + W, oj, oj + W};
  scene_splat_body<false>(in, b, tf + kb, g.inv, g.prev[b].ok != 0, window, W, SceneKindLive(in, b), g.cells + (long)b * W * W, steps[kb] + 1, hdr, true);
}

// ------------------------------------------------------------------------------------------ G2
__global__ void MOT_SG_BOUNDS(kSceneBlock)
scene_export_kernel(SceneGridBuffers g, int b0, mot_scene_cell* __restrict__ out, long cell_stride, mot_scene_header* __restrict__ headers) {
  const int kb = blockIdx.y, b = b0 + kb;
  const int W = g.W;
  const mot_scene_header h = g.hdr[b];
  if (blockIdx.x == 0 && threadIdx.x == 0 && headers) headers[kb] = h;
  if (!out) return;
  const long k = (long)blockIdx.x * kSceneBlock + threadIdx.x;
  if (k >= (long)W * W) return;
  const int u = (int)(k & (W - 1)), v = (int)(k >> g.log2_W);
  const long at = (long)((h.origin_j + v) & (W - 1)) * W + ((h.origin_i + u) & (W - 1));
  uint4 c = reinterpret_cast<const uint4*>(g.cells + (long)b * W * W)[at];   // {static_hits, dynamic_hits, z image, last_seen}
  c.z = c.x ? (unsigned)mot_f2i(mot_key_float((int)(c.z ^ 0x80000000u))) : 0u;
  reinterpret_cast<uint4*>(out + (long)kb * cell_stride)[k] = c;
}

// ------------------------------------------------------------------------------------------ headers and origins back to "no step yet"
__global__ void MOT_SG_BOUNDS(kSceneBlock)
scene_reset_kernel(SceneGridBuffers g, int first, int n) {
  const int k = blockIdx.x * kSceneBlock + threadIdx.x;
  if (k >= n) return;
  mot_scene_header h;
  h.origin_i = 0; h.origin_j = 0; h.step = -1; h.size = g.W; h.n_static = 0; h.n_dynamic = 0; h.n_outside = 0; h.cell = g.cell;
  g.hdr[first + k] = h;
  SceneWindow w;
  w.oi = 0; w.oj = 0; w.ok = 0; w.pad = 0;
  g.prev[first + k] = w;
}

// ------------------------------------------------------------------------------------------ host
void mot_launch_scene_accumulate(const SceneGridBuffers& g, const SceneSplatInput& in, int first, int batch, int max_n, const EgoTf* tf, const int* steps, hipStream_t stream) {
  const int chunks = mot_launch_chunks(max_n, kSceneChunk);   // (at least one: workgroup 0 of a frame also moves the previous origin on)
  hipLaunchKernelGGL(scene_scroll_kernel, dim3(kSceneScrollBlocks, batch), dim3(kSceneBlock), 0, stream, g, first, tf, steps);
  hipLaunchKernelGGL(scene_splat_kernel, dim3(chunks, batch), dim3(kSceneBlock), 0, stream, g, in, first, tf, steps);
}
void mot_launch_scene_export(const SceneGridBuffers& g, int first, int batch, mot_scene_cell* out, long cell_stride, mot_scene_header* headers, hipStream_t stream) {
  const long cells = out ? (long)g.W * g.W : 1;
  hipLaunchKernelGGL(scene_export_kernel, dim3((unsigned)((cells + kSceneBlock - 1) / kSceneBlock), batch), dim3(kSceneBlock), 0, stream, g, first, out, cell_stride, headers);
}
void mot_launch_scene_reset(const SceneGridBuffers& g, int first, int n, hipStream_t stream) {
  if (n <= 0) return;
  hipLaunchKernelGGL(scene_reset_kernel, dim3((n + kSceneBlock - 1) / kSceneBlock), dim3(kSceneBlock), 0, stream, g, first, n);
}
