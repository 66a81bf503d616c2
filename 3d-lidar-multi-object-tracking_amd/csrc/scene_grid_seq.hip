// scene_grid_seq.hip — the rolling static-scene grid (scene_grid.hip) fed by SEQUENCE MODE, on gfx950. Product code (HIP, wave64).
//
// mot_sequence_products_dev(MOT_SEQ_SCENE): the frames of one recorded drive go through the tracker chained on the device (slot k = frame k, the track state in
// stream 0), and all of them are taken into stream 0's grid in the same call. Two things the one-step code reads are gone when the chain has run: the kind of a
// point (slot_of[id] -> is_static "as this step left it" is overwritten by the next step) and the window (it rolls from frame to frame, and a scroll clears what
// entered). The first is captured inside the chain; the second needs no serial pass:
//
// THE RECTANGLE RULE. All windows are axis-aligned squares of one size W, window k = [o[k], o[k] + W) per axis (o[k] = o[k - 1] when frame k's window is invalid;
// o[-1] = the origin the grid is laid out for before the call). A cell's contents of frame k survive to the end of the call iff no scroll k + 1 .. F - 1 cleared the
// cell, i.e. iff the cell lies in EVERY window k .. F - 1: once it is outside window j it is either outside all later ones or is cleared when it enters again. An
// intersection of such squares is the rectangle R[k] = [max_{j >= k} o[j], min_{j >= k} o[j] + W) per axis — a suffix maximum and minimum of the origins. So:
// the cells of the final window outside R[-1] are emptied (they held other global cells, or were scrolled out on the way), the rest keep what they hold, and a point
// of frame k takes part iff its cell lies in R[k]. Every cell operation is an integer add or maximum, so the frames are splatted in ONE launch, in any order.
//
//   Q0  scene_seq_capture_kernel   one launch per step, right behind it: for every box of the step's owner row whose track is flagged static as the step left it
//                                  (slot_of[id] in [0, T), is_static != 0) bit `id` of the frame's row of the table, with an integer OR. The rows are zeroed once a call
//   Q1  scene_seq_windows_kernel   ONE workgroup: ok[k] and o[k] of every frame from the matrices (the carry through invalid windows is a last-valid scan), the suffix
//                                  maxima / minima -> R[-1 .. F - 1]; the final header (the last frame's origin and stamp, counters 0) and the final previous origin
//   Q2  scene_seq_clear_kernel     the columns and rows of the torus outside R[-1] (one run each: the window minus a rectangle inside it), or everything
//   Q3  scene_seq_splat_kernel     grid (chunks, frames), chunk index fastest: scene_splat_body (mot_scene_splat.h), the ONE body it shares with scene_splat_kernel.
//                                  The kernel decides what differs: frame k's matrix, stamp, validity and rectangle; the kind from the captured bits
//                                  (SceneKindRecorded); last_seen by atomicMax of stamp + 1, since several frames hit a cell in one launch; only frame F - 1 feeds the
//                                  header's counters (against its own window = R[F - 1]). A frame with an invalid window or an empty rectangle leaves at once,
//                                  frame F - 1 never does
//
// INTEGER ATOMICS ONLY (adds, maxima, one OR); nobody waits for another workgroup; Q1's two scans hand values over inside one workgroup across __syncthreads().
// INDEX SAFETY as in scene_grid.hip: the storage index is masked, point and id loads stay below min(count, cap) of the frame's slot, an id outside [0, E) is not looked up
// (dynamic), Q0 follows an id / a slot only inside [0, E) / [0, T); frames <= max_batch bounds every per-frame table.
// Bytes: Q0 per box 4 (owner) + 4 (slot_of) + 4 (is_static) read; Q3 per point 16 as the one-step kernel, and one 4-byte gather into a table of E / 8 bytes a frame.
// Resources (tools/kernel_resources.py, gfx950): Q0 10 VGPRs; Q1 44 VGPRs, 4 096 bytes of LDS; Q2 10 VGPRs; Q3 47 VGPRs (scene_splat_kernel: 58, as before the
// shared helpers). 8 waves per SIMD each, no LDS but Q1's, no scratch memory.
#include "mot_scene_splat.h"

static_assert(sizeof(SceneSeqFrame) == 32, "mot_internal.h documents the size");
constexpr int kSeqIntMax = 2147483647, kSeqIntMin = -2147483647 - 1;

// ------------------------------------------------------------------------------------------ Q0
__global__ void MOT_SG_BOUNDS(kSceneBlock)
scene_seq_capture_kernel(const int* __restrict__ counts, const int* __restrict__ owner, const int* __restrict__ slot_of, const mot_track* __restrict__ out, int T, int E,
                         SceneSeqBuffers s, int k) {
  const int M = mot_owner_boxes(counts, k);
  unsigned* __restrict__ row = s.is_static + (long)k * s.words;
  for (int i = threadIdx.x; i < M; i += kSceneBlock) {
    const int id = owner[(long)k * kMaxBoxesPerFrame + i];
    if (id < 0 || id >= E) continue;
    const int r = slot_of[id];   // (stream 0's map and records)
    if (r >= 0 && r < T && out[r].is_static != 0) atomicOr(row + (id >> 5), 1u << (id & 31));
  }
}

// ------------------------------------------------------------------------------------------ Q1
__global__ void MOT_SG_BOUNDS(kSceneBlock)
scene_seq_windows_kernel(SceneGridBuffers g, SceneSeqBuffers s, const EgoTf* __restrict__ tf, int frames) {
  __shared__ int s_a[kSceneBlock], s_b[kSceneBlock], s_c[kSceneBlock], s_d[kSceneBlock];
  const int tid = threadIdx.x, W = g.W;
  SceneSeqFrame* win = s.win;   // (written by one thread, read by another behind a barrier)
  int carry_i = g.prev[0].oi, carry_j = g.prev[0].oj;   // o[-1]; every thread reads it before the first barrier, the new one is written behind it
  if (tid == 0) { win[0].oi = carry_i; win[0].oj = carry_j; win[0].ok = 1; win[0].pad = 0; }
  // forward, 256 frames a round: o[k] = the window of the last frame <= k that has a valid one
  for (int k0 = 0; k0 < frames; k0 += kSceneBlock) {
    const int k = k0 + tid;
    int oi = 0, oj = 0;
    const bool ok = k < frames && scene_window(tf[k], g.inv, W, &oi, &oj);
    s_a[tid] = ok ? 1 : 0; s_b[tid] = oi; s_c[tid] = oj;
    __syncthreads();
    for (int d = 1; d < kSceneBlock; d <<= 1) {
      int have = s_a[tid], vi = s_b[tid], vj = s_c[tid];
      if (tid >= d && !have) { have = s_a[tid - d]; vi = s_b[tid - d]; vj = s_c[tid - d]; }
      __syncthreads();
      s_a[tid] = have; s_b[tid] = vi; s_c[tid] = vj;
      __syncthreads();
    }
    const int ri = s_a[tid] ? s_b[tid] : carry_i, rj = s_a[tid] ? s_c[tid] : carry_j;
    if (k < frames) { win[k + 1].oi = ri; win[k + 1].oj = rj; win[k + 1].ok = ok ? 1 : 0; win[k + 1].pad = 0; }
    if (k == frames - 1) {   // what the last step of the frame-by-frame route leaves: its header, counters at 0 (Q3 adds), and the origin the cells are laid out for
      mot_scene_header h;
      h.origin_i = ri; h.origin_j = rj; h.step = s.step0 + k; h.size = W; h.n_static = 0; h.n_dynamic = 0; h.n_outside = 0; h.cell = g.cell;
      g.hdr[0] = h;
      g.prev[0].oi = ri; g.prev[0].oj = rj; g.prev[0].ok = ok ? 1 : 0;
    }
    const int li = s_a[kSceneBlock - 1] ? s_b[kSceneBlock - 1] : carry_i, lj = s_a[kSceneBlock - 1] ? s_c[kSceneBlock - 1] : carry_j;
    __syncthreads();   // (the next round rewrites the arrays)
    carry_i = li; carry_j = lj;
  }
  // backward over the entries e = k + 1 = frames .. 0: suffix maxima and minima of the origins (the barriers above order the origins written there before these reads)
  int max_i = kSeqIntMin, min_i = kSeqIntMax, max_j = kSeqIntMin, min_j = kSeqIntMax;   // over the rounds behind this one
  for (int e0 = frames / kSceneBlock * kSceneBlock; e0 >= 0; e0 -= kSceneBlock) {
    const int e = e0 + tid;
    const bool valid = e <= frames;
    const int oi = valid ? win[e].oi : 0, oj = valid ? win[e].oj : 0;
    s_a[tid] = valid ? oi : kSeqIntMin; s_b[tid] = valid ? oi : kSeqIntMax; s_c[tid] = valid ? oj : kSeqIntMin; s_d[tid] = valid ? oj : kSeqIntMax;
    __syncthreads();
    for (int d = 1; d < kSceneBlock; d <<= 1) {
      int a = s_a[tid], b = s_b[tid], c = s_c[tid], dd = s_d[tid];
      if (tid + d < kSceneBlock) {
        a = max(a, s_a[tid + d]); b = min(b, s_b[tid + d]); c = max(c, s_c[tid + d]); dd = min(dd, s_d[tid + d]);
      }
      __syncthreads();
      s_a[tid] = a; s_b[tid] = b; s_c[tid] = c; s_d[tid] = dd;
      __syncthreads();
    }
    if (valid) {   // (a valid entry's minimum is a real origin, within 2^30 + W / 2: + W does not overflow)
      win[e].lo_i = max(s_a[tid], max_i); win[e].hi_i = min(s_b[tid], min_i) + W;
      win[e].lo_j = max(s_c[tid], max_j); win[e].hi_j = min(s_d[tid], min_j) + W;
    }
    const int a0 = max(s_a[0], max_i), b0 = min(s_b[0], min_i), c0 = max(s_c[0], max_j), d0 = min(s_d[0], min_j);
    __syncthreads();
    max_i = a0; min_i = b0; max_j = c0; min_j = d0;
  }
}

// ------------------------------------------------------------------------------------------ Q2
__global__ void MOT_SG_BOUNDS(kSceneBlock)
scene_seq_clear_kernel(SceneGridBuffers g, SceneSeqBuffers s) {
  const int W = g.W, lw = g.log2_W;
  const SceneSeqFrame r = s.win[0];   // R[-1], inside the final window [o, o + W): lo >= o, hi <= o + W
  long wi = (long)r.hi_i - r.lo_i, wj = (long)r.hi_j - r.lo_j;
  wi = wi > W ? W : wi; wj = wj > W ? W : wj;
  // the window's columns outside [lo_i, hi_i) are one run of the torus, from hi_i on (column o + W is column o); the rows likewise. An empty rectangle: every column
  const bool none = wi <= 0 || wj <= 0;
  const int ni = none ? W : W - (int)wi, nj = none ? 0 : W - (int)wj;
  const int ci0 = none ? 0 : r.hi_i, cj0 = none ? 0 : r.hi_j;
  const long total = ((long)ni + nj) * W;
  uint4* __restrict__ cells = reinterpret_cast<uint4*>(g.cells);   // (slot 0's)
  uint4 zero;
  zero.x = 0u; zero.y = 0u; zero.z = 0u; zero.w = 0u;
  for (long k = (long)blockIdx.x * kSceneBlock + threadIdx.x; k < total; k += (long)gridDim.x * kSceneBlock) {
    const int q = (int)(k >> lw), t = (int)(k & (W - 1));
    int si, sj;
    if (q < ni) { si = (ci0 + q) & (W - 1); sj = t; }
    else { si = t; sj = (cj0 + (q - ni)) & (W - 1); }
    cells[(long)sj * W + si] = zero;
  }
}

// ------------------------------------------------------------------------------------------ Q3
__global__ void MOT_SG_BOUNDS(kSceneBlock)
scene_seq_splat_kernel(SceneGridBuffers g, SceneSplatInput in, SceneSeqBuffers s, const EgoTf* __restrict__ tf, int frames) {
  const int k = blockIdx.y;   // frame k lives in slot k; the grid is slot 0's
  const SceneSeqFrame f = s.win[k + 1];
  const bool last = k == frames - 1;
  const bool window_ok = f.ok != 0;
  if (!last && (!window_ok || f.hi_i <= f.lo_i || f.hi_j <= f.lo_j)) return;   // nothing of the frame survives the drive; the last frame's counters are due either way
  const SceneRect rect = {f.lo_i, f.hi_i, f.lo_j, f.hi_j};
  scene_splat_body<true>(in, k, tf + k, g.inv, window_ok, rect, g.W, SceneKindRecorded(in, s, k), g.cells, s.step0 + k + 1, g.hdr, last);
}

// ------------------------------------------------------------------------------------------ host
void mot_launch_scene_seq_capture(const int* counts, const int* owner, const int* slot_of, const mot_track* out, int T, int E, const SceneSeqBuffers& s, int frame,
                                  hipStream_t stream) {
  hipLaunchKernelGGL(scene_seq_capture_kernel, dim3(1), dim3(kSceneBlock), 0, stream, counts, owner, slot_of, out, T, E, s, frame);
}
void mot_launch_scene_sequence(const SceneGridBuffers& g, const SceneSplatInput& in, const SceneSeqBuffers& s, int frames, int max_n, const EgoTf* tf, hipStream_t stream) {
  const int chunks = mot_launch_chunks(max_n, kSceneChunk);
  hipLaunchKernelGGL(scene_seq_windows_kernel, dim3(1), dim3(kSceneBlock), 0, stream, g, s, tf, frames);
  hipLaunchKernelGGL(scene_seq_clear_kernel, dim3(kSceneSeqClearBlocks), dim3(kSceneBlock), 0, stream, g, s);
  hipLaunchKernelGGL(scene_seq_splat_kernel, dim3(chunks, frames), dim3(kSceneBlock), 0, stream, g, in, s, tf, frames);
}
