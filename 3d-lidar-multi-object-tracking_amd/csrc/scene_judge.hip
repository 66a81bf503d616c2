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
//   J2  scene_judge_scan_kernel      one workgroup per slot: per class an exclusive scan of the chunks' counts (block_scan_excl_i32 of mot_wave.h), the mask applied,
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
// The class rule, the ballots, the scan over chunks, the tile chain and the record store live in mot_scene_judge.h: scene_judge_seq.hip (a recorded drive judged against
// slot 0's grid) runs the same inline functions, so that the last frame of a drive gets these kernels' bytes.
#include "mot_scene_judge.h"   // the class rule, the ballots, the scans and the record store shared with scene_judge_seq.hip (and, through it, mot_scene_splat.h)

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
    const int c = sj_class(dynamic, at, cells, j);
    if (valid) {
      cls_out[i] = (uint8_t)c;
      if (user && i < class_stride) user[i] = (uint8_t)c;
    }
    sj_tally(valid ? c : kSjNone, count);
  }
  sj_store_counts(s_cnt, count, j.rows + ((long)b * j.max_chunks + blockIdx.x) * kSceneJudgeRow, tid, lane, wave);
}

// ------------------------------------------------------------------------------------------ J2
// rows[chunk][c] (counts) -> rows[chunk][5 + c]: the place of the chunk's first record of class c — the records of the selected classes below c, then the class's
// points of earlier chunks (whatever for a class outside the mask: nobody reads it). Chunks tid, tid + 256, ... per thread; every lane takes part in every scan.
__global__ void MOT_SG_BOUNDS(kSceneBlock)
scene_judge_scan_kernel(SceneSplatInput in, SceneJudgeBuffers j, int b0, mot_scene_segment* __restrict__ segments) {
  __shared__ int s_part[kSjWaves];
  __shared__ int s_total[MOT_SCENE_CLASSES];
  const int kb = blockIdx.x, b = b0 + kb, tid = threadIdx.x;
  const int n = sj_count(in, b);
  int chunks = (n + kSceneChunk - 1) / kSceneChunk;
  if (chunks > j.max_chunks) chunks = j.max_chunks;
  int* __restrict__ rows = j.rows + (long)b * j.max_chunks * kSceneJudgeRow;
  sj_scan_chunks(rows, chunks, s_part, s_total, tid);
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
    rank[k] = sj_rank(cls[k], k * kSjWaves + wave, lane, below, s_cnt);
  }
  __syncthreads();
  if (tid < MOT_SCENE_CLASSES) sj_chain(s_cnt, s_at, tid, row[MOT_SCENE_CLASSES + tid]);   // the chunk's tiles in index order
  __syncthreads();
  const EgoTf m = tf ? tf[kb] : EgoTf();
#pragma unroll
  for (int k = 0; k < kSceneItems; k++) {
    const long i = base + k * kSceneBlock + tid;
    if (cls[k] >= MOT_SCENE_CLASSES || !((j.class_mask >> cls[k]) & 1)) continue;
    const long dst = (long)s_at[k * kSjWaves + wave][cls[k]] + rank[k];
    if (dst >= point_stride) continue;   // (dst < n while the rows are this call's; never a store outside the slot's records)
    sj_store_record(out + dst, vec_out, tf != nullptr, m, q[k], (int)i);
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
