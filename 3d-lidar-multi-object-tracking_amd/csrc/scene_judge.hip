// scene_judge.hip — a frame's points judged against the rolling static-scene grid, on gfx950. Product code (HIP, wave64).
//
// scene_grid.hip fills the grid; the kernels here ask it a question about the live frame (include/mot.h, "a frame's points judged against the scene grid"): every
// elevated point of a fused step gets one of five classes — UNKNOWN, MOVING, TRAIL, NEW, KNOWN — and the points are partitioned by class, in input order, into the
// caller's block. The grid is only READ. The reference has no such output (scene_grid.hip's header).
//
//   J1  scene_judge_classify_kernel  grid (ceil(N_e / 2048), B), 256 threads, 8 points a thread — the geometry of scene_splat_kernel. Per point the 12-byte point (16 in
//                                    the float4 layout), the 4-byte id, for an owned point the two dependent gathers id -> track slot -> is_static, the transform
//                                    and cell test of scene_point_cell (mot_scene_splat.h: the cell is bit for bit the one the point would be counted in) and ONE
//                                    8-byte load of the cell's {static_hits, dynamic_hits}; neighbouring lanes mostly share a cell, so the loads coalesce by
//                                    themselves. The 64-bit trail test, then the class as one byte to the library's scratch (and to the caller's class block), and
//                                    the chunk's five counts — wave ballots on the three class bits, merged through LDS — as plain stores to the chunk's row
//   J2  scene_judge_scan_kernel      one workgroup per slot: per class an exclusive scan of the chunks' counts (the DPP wave scans of mot_wave.h), the mask applied,
//                                    the segment table, and where every chunk's first record of every class goes
//   J3  scene_judge_scatter_kernel   the grid of J1: class byte in, rank inside the 64-point tile by ballots on the class bits, the 32 tiles of a chunk chained
//                                    through a small LDS table (five serial scans of 32 entries), the point and the global transform on request, one 16-byte store
//                                    per selected record below the caller's stride. Only the points of selected classes are loaded
//
// The cell of a point is gathered ONCE per call (J3 reads J1's byte). No global atomics, no workgroup waits on another, every count and every place is a sum of
// integers over a fixed set: the output does not depend on the order in which workgroups or waves run.
// INDEX SAFETY. Point, id and class loads stay below min(count, cap) of the slot; the storage index is masked (scene_point_cell); an id outside [0, E) or a
// track slot outside [0, T) is not followed (the point then counts as dynamic, as in the splat kernel); chunk rows are indexed below the slot's chunk capacity; a
// record is stored only below min(point_stride, selected records), a class byte only below class_stride.
// Resources (tools/kernel_resources.py): no scratch; LDS 80 bytes (J1), 48 (J2), 1280 (J3); 68 / 13 / 101 VGPRs. Cost: profiles/scene_judge.md.
#include "mot_scene_splat.h"   // the per-point step shared with the splat kernels

static_assert(sizeof(mot_scene_segment) == 8 && sizeof(mot_track_point) == 16, "include/mot.h documents the sizes");
static_assert(MOT_SCENE_CLASSES == 5 && MOT_SCENE_KNOWN < 8, "a class is three bits");

constexpr int kSjWaves = kSceneBlock / 64;
constexpr int kSjTiles = kSceneChunk / 64;   // tile k * kSjWaves + wave of a chunk: item k of that wave
constexpr int kSjNone = 7;                   // the class bits of a lane without a point

__device__ __forceinline__ int sj_count(const SceneSplatInput& in, int b) {
  const int n = in.counts[b * kCountsStride + kCntElev];
  return n < 0 ? 0 : (n < (int)in.cap ? n : (int)in.cap);
}
// the lanes of the wave that hold class c, from the ballots of the three class bits (a lane without a point holds kSjNone)
__device__ __forceinline__ unsigned long long sj_lanes_of(int c, unsigned long long b0, unsigned long long b1, unsigned long long b2) {
  return ((c & 1) ? b0 : ~b0) & ((c & 2) ? b1 : ~b1) & ((c & 4) ? b2 : ~b2);
}

// ------------------------------------------------------------------------------------------ J1
__global__ void MOT_SG_BOUNDS(kSceneBlock)
scene_judge_classify_kernel(SceneGridBuffers g, SceneSplatInput in, SceneJudgeBuffers j, int b0, const EgoTf* __restrict__ tf, uint8_t* __restrict__ classes, long class_stride) {
  __shared__ int s_cnt[kSjWaves][MOT_SCENE_CLASSES];
  const int kb = blockIdx.y, b = b0 + kb, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int W = g.W;
  const int n = sj_count(in, b);
  const long base = (long)blockIdx.x * kSceneChunk;
  if (base >= n || (int)blockIdx.x >= j.max_chunks) return;   // (uniform over the workgroup)
  const int oi = g.hdr[b].origin_i, oj = g.hdr[b].origin_j;
  const bool window_ok = g.prev[b].ok != 0;   // the latest accepted step placed its window (0 after the setter, a reset or a load: no step yet)
  const EgoTf m = tf[kb];
  const float inv = g.inv;
  const int* __restrict__ ids = in.ids + (long)b * in.cap;
  const float4* __restrict__ cloud = in.elevated + (long)b * in.cap;
  const SceneCell* __restrict__ cells = g.cells + (long)b * W * W;
  uint8_t* __restrict__ cls_out = j.cls + (long)b * in.cap;
  uint8_t* __restrict__ user = classes ? classes + (long)kb * class_stride : nullptr;
  int id[kSceneItems];
  float4 q[kSceneItems];
#pragma unroll
  for (int k = 0; k < kSceneItems; k++) {
    const long i = base + k * kSceneBlock + tid;
    id[k] = -1;
    q[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n) { id[k] = ids[i]; q[k] = mot_load_xyz(cloud, i, in.elevated_packed); }
  }
  const SceneRect window = {oi, oi + W, oj, oj + W};
  int count[MOT_SCENE_CLASSES] = {0, 0, 0, 0, 0};   // of this wave (uniform)
#pragma unroll
  for (int k = 0; k < kSceneItems; k++) {
    const long i = base + k * kSceneBlock + tid;
    const bool valid = i < n;
    int dynamic = 0;
    if (valid && id[k] >= 0) {   // the grid's KIND rule
      dynamic = 1;
      if (id[k] < in.E) {
        const int r = in.slot_of[(long)b * in.E + id[k]];
        if (r >= 0 && r < in.T) dynamic = in.out[(long)b * in.T + r].is_static == 0;
      }
    }
    float gz;
    const int at = scene_point_cell(m, q[k], inv, valid && window_ok, window, W, &gz);   // (mot_scene_splat.h)
    int c = MOT_SCENE_UNKNOWN;
    if (dynamic) c = MOT_SCENE_MOVING;
    else if (at >= 0) {
      const uint2 h = *reinterpret_cast<const uint2*>(cells + at);   // {static_hits, dynamic_hits}
      const unsigned long long s = h.x, d = h.y;
      const bool trail = d > 0 && d * j.trail_den > (s + d) * j.trail_num;   // < 2^33 * 2^16: exact
      c = trail ? MOT_SCENE_TRAIL : (h.x < j.min_static_hits ? MOT_SCENE_NEW : MOT_SCENE_KNOWN);
    }
    if (valid) {
      cls_out[i] = (uint8_t)c;
      if (user && i < class_stride) user[i] = (uint8_t)c;
    }
    const int bits = valid ? c : kSjNone;
    const unsigned long long a0 = __ballot(bits & 1), a1 = __ballot(bits & 2), a2 = __ballot(bits & 4);
#pragma unroll
    for (int cc = 0; cc < MOT_SCENE_CLASSES; cc++) count[cc] += __popcll(sj_lanes_of(cc, a0, a1, a2));
  }
  if (lane == 0) {
#pragma unroll
    for (int cc = 0; cc < MOT_SCENE_CLASSES; cc++) s_cnt[wave][cc] = count[cc];
  }
  __syncthreads();
  if (tid < MOT_SCENE_CLASSES) {
    int sum = 0;
#pragma unroll
    for (int w = 0; w < kSjWaves; w++) sum += s_cnt[w][tid];
    j.rows[((long)b * j.max_chunks + blockIdx.x) * kSceneJudgeRow + tid] = sum;
  }
}

// ------------------------------------------------------------------------------------------ J2
// rows[chunk][c] (counts) -> rows[chunk][5 + c]: the place of the chunk's first record of class c — the records of the selected classes below c, then the class's
// points of earlier chunks (whatever for a class outside the mask: nobody reads it). Chunks tid, tid + 256, ... per thread; every lane takes part in every scan.
__global__ void MOT_SG_BOUNDS(kSceneBlock)
scene_judge_scan_kernel(SceneSplatInput in, SceneJudgeBuffers j, int b0, mot_scene_segment* __restrict__ segments) {
  __shared__ int s_part[kSjWaves];
  __shared__ int s_total[MOT_SCENE_CLASSES];
  const int kb = blockIdx.x, b = b0 + kb, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = sj_count(in, b);
  int chunks = (n + kSceneChunk - 1) / kSceneChunk;
  if (chunks > j.max_chunks) chunks = j.max_chunks;
  int* __restrict__ rows = j.rows + (long)b * j.max_chunks * kSceneJudgeRow;
  for (int c = 0; c < MOT_SCENE_CLASSES; c++) {
    int carry = 0;   // the class's points in the chunks of earlier rounds
    for (int r0 = 0; r0 < chunks; r0 += kSceneBlock) {   // (uniform)
      const int ch = r0 + tid;
      const int v = ch < chunks ? rows[(long)ch * kSceneJudgeRow + c] : 0;
      const int incl = wave_scan_incl_i32(v);
      if (lane == 63) s_part[wave] = incl;
      __syncthreads();
      int first = carry + incl - v, total = 0;
      for (int w = 0; w < kSjWaves; w++) { if (w < wave) first += s_part[w]; total += s_part[w]; }
      carry += total;
      __syncthreads();   // (s_part is written again in the next round)
      if (ch < chunks) rows[(long)ch * kSceneJudgeRow + MOT_SCENE_CLASSES + c] = first;
    }
    if (tid == 0) s_total[c] = carry;
  }
  __syncthreads();
  int first_of[MOT_SCENE_CLASSES];
  int run = 0;
#pragma unroll
  for (int c = 0; c < MOT_SCENE_CLASSES; c++) {
    const bool picked = (j.class_mask >> c) & 1;
    first_of[c] = picked ? run : -1;
    if (picked) run += s_total[c];
  }
  if (tid < MOT_SCENE_CLASSES) {
    int* o = reinterpret_cast<int*>(segments + (long)kb * MOT_SCENE_CLASSES + tid);
    int first = -1;
#pragma unroll
    for (int c = 0; c < MOT_SCENE_CLASSES; c++) first = tid == c ? first_of[c] : first;
    o[0] = first; o[1] = s_total[tid];
  }
  // every thread adds the segment starts to the places it wrote itself (chunk ch is thread ch % 256's)
  for (int ch = tid; ch < chunks; ch += kSceneBlock) {
#pragma unroll
    for (int c = 0; c < MOT_SCENE_CLASSES; c++)
      if (first_of[c] > 0) rows[(long)ch * kSceneJudgeRow + MOT_SCENE_CLASSES + c] += first_of[c];
  }
}

// ------------------------------------------------------------------------------------------ J3
__global__ void MOT_SG_BOUNDS(kSceneBlock)
scene_judge_scatter_kernel(SceneSplatInput in, SceneJudgeBuffers j, int b0, const EgoTf* __restrict__ tf, mot_track_point* __restrict__ points, long point_stride) {
  __shared__ int s_cnt[kSjTiles][MOT_SCENE_CLASSES];   // points of (tile, class)
  __shared__ int s_at[kSjTiles][MOT_SCENE_CLASSES];    // where the tile's first record of the class goes
  const int kb = blockIdx.y, b = b0 + kb, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = sj_count(in, b);
  const long base = (long)blockIdx.x * kSceneChunk;
  if (base >= n || (int)blockIdx.x >= j.max_chunks) return;   // (uniform over the workgroup)
  const uint8_t* __restrict__ cls_in = j.cls + (long)b * in.cap;
  const float4* __restrict__ cloud = in.elevated + (long)b * in.cap;
  const int* __restrict__ row = j.rows + ((long)b * j.max_chunks + blockIdx.x) * kSceneJudgeRow;
  mot_track_point* out = points + (long)kb * point_stride;
  const bool vec_out = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  int cls[kSceneItems];
  float4 q[kSceneItems];
#pragma unroll
  for (int k = 0; k < kSceneItems; k++) {
    const long i = base + k * kSceneBlock + tid;
    cls[k] = i < n ? (int)cls_in[i] : kSjNone;
  }
#pragma unroll
  for (int k = 0; k < kSceneItems; k++) {   // the points of the selected classes alone
    const long i = base + k * kSceneBlock + tid;
    q[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cls[k] < MOT_SCENE_CLASSES && ((j.class_mask >> cls[k]) & 1)) q[k] = mot_load_xyz(cloud, i, in.elevated_packed);
  }
  const unsigned long long below = (1ull << lane) - 1ull;
  int rank[kSceneItems];
#pragma unroll
  for (int k = 0; k < kSceneItems; k++) {   // tile k * 4 + wave of the chunk: points 64 * tile .. 64 * tile + 63
    const unsigned long long a0 = __ballot(cls[k] & 1), a1 = __ballot(cls[k] & 2), a2 = __ballot(cls[k] & 4);
    rank[k] = __popcll(sj_lanes_of(cls[k], a0, a1, a2) & below);
    if (lane < MOT_SCENE_CLASSES) s_cnt[k * kSjWaves + wave][lane] = __popcll(sj_lanes_of(lane, a0, a1, a2));
  }
  __syncthreads();
  if (tid < MOT_SCENE_CLASSES) {   // the chunk's tiles in index order
    int run = row[MOT_SCENE_CLASSES + tid];
    for (int t = 0; t < kSjTiles; t++) { s_at[t][tid] = run; run += s_cnt[t][tid]; }
  }
  __syncthreads();
  const EgoTf m = tf ? tf[kb] : EgoTf();
#pragma unroll
  for (int k = 0; k < kSceneItems; k++) {
    const long i = base + k * kSceneBlock + tid;
    if (cls[k] >= MOT_SCENE_CLASSES || !((j.class_mask >> cls[k]) & 1)) continue;
    const long dst = (long)s_at[k * kSjWaves + wave][cls[k]] + rank[k];
    if (dst >= point_stride) continue;   // (dst < n while the rows are this call's; never a store outside the slot's records)
    float4 o;
    if (tf) {   // fp32, left to right; the build has -ffp-contract=off (mot_track_place.h's sensor -> global step: the bits mot_export_track_points_dev writes)
      o.x = m.m[0] * q[k].x + m.m[1] * q[k].y + m.m[2] * q[k].z + m.m[3];
      o.y = m.m[4] * q[k].x + m.m[5] * q[k].y + m.m[6] * q[k].z + m.m[7];
      o.z = m.m[8] * q[k].x + m.m[9] * q[k].y + m.m[10] * q[k].z + m.m[11];
    } else { o.x = q[k].x; o.y = q[k].y; o.z = q[k].z; }
    o.w = __int_as_float((int)i);
    if (vec_out) *reinterpret_cast<float4*>(out + dst) = o;
    else { float* p = reinterpret_cast<float*>(out + dst); p[0] = o.x; p[1] = o.y; p[2] = o.z; p[3] = o.w; }
  }
}

// ------------------------------------------------------------------------------------------ host
void mot_launch_scene_judge(const SceneGridBuffers& g, const SceneSplatInput& in, const SceneJudgeBuffers& j, int first, int batch, int max_n, const EgoTf* tf, int global,
                            mot_track_point* points, long point_stride, mot_scene_segment* segments, uint8_t* classes, long class_stride, hipStream_t stream) {
  int chunks = (max_n + kSceneChunk - 1) / kSceneChunk;
  if (chunks < 1) chunks = 1;
  if (chunks > j.max_chunks) chunks = j.max_chunks;
  const dim3 grid(chunks, batch);
  hipLaunchKernelGGL(scene_judge_classify_kernel, grid, dim3(kSceneBlock), 0, stream, g, in, j, first, tf, classes, class_stride);
  hipLaunchKernelGGL(scene_judge_scan_kernel, dim3(batch), dim3(kSceneBlock), 0, stream, in, j, first, segments);
  if (j.class_mask && points && point_stride > 0)
    hipLaunchKernelGGL(scene_judge_scatter_kernel, grid, dim3(kSceneBlock), 0, stream, in, j, first, global ? tf : nullptr, points, point_stride);
}
