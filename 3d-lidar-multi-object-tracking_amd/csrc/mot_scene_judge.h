// mot_scene_judge.h — device helpers the judge kernels of scene_judge.hip (every slot against its own grid) and scene_judge_seq.hip (a recorded drive against slot 0's
// grid) share: THE class rule of a cell, the ballots that count and rank a wave's points by class, the scan over a frame's chunks, the chain over a chunk's tiles, the
// record store, and the two bodies built from them — sj_classify_body and sj_scatter_body, each the ONE text of a live and a recorded kernel. One definition, so that
// the last frame of a drive gets the very bytes the frame-by-frame route gives it (include/mot.h). Product code.
#ifndef MOT_SCENE_JUDGE_H_
#define MOT_SCENE_JUDGE_H_
#include "mot_scene_splat.h"   // the per-point step shared with the splat kernels

static_assert(sizeof(mot_scene_segment) == 8 && sizeof(mot_track_point) == 16, "include/mot.h documents the sizes");
static_assert(MOT_SCENE_CLASSES == 5 && MOT_SCENE_KNOWN < 8, "a class is three bits");

constexpr int kSjWaves = kSceneBlock / 64;
constexpr int kSjTiles = kSceneChunk / 64;   // tile k * kSjWaves + wave of a chunk: item k of that wave
constexpr int kSjNone = 7;                   // the class bits of a lane without a point

// the chunks of frame `slot` that the judge has rows for (the frame's points: scene_count, mot_scene_splat.h)
__device__ __forceinline__ int sj_chunks(const SceneSplatInput& in, const SceneJudgeBuffers& j, int slot) {
  const int chunks = (scene_count(in, slot) + kSceneChunk - 1) / kSceneChunk;
  return chunks > j.max_chunks ? j.max_chunks : chunks;
}
// the lanes of the wave that hold class c, from the ballots of the three class bits (a lane without a point holds kSjNone)
__device__ __forceinline__ unsigned long long sj_lanes_of(int c, unsigned long long b0, unsigned long long b1, unsigned long long b2) {
  return ((c & 1) ? b0 : ~b0) & ((c & 2) ? b1 : ~b1) & ((c & 4) ? b2 : ~b2);
}

// THE class rule: dynamic by the grid's kind rule -> MOVING; no cell (at < 0) -> UNKNOWN; else ONE 8-byte load of the cell's two counters and the 64-bit trail test
__device__ __forceinline__ int sj_class(int dynamic, int at, const SceneCell* __restrict__ cells, const SceneJudgeBuffers& j) {
  int c = MOT_SCENE_UNKNOWN;
  if (dynamic) c = MOT_SCENE_MOVING;
  else if (at >= 0) {
    const uint2 h = *reinterpret_cast<const uint2*>(cells + at);   // {static_hits, dynamic_hits}
    const unsigned long long s = h.x, d = h.y;
    const bool trail = d > 0 && d * j.trail_den > (s + d) * j.trail_num;   // < 2^33 * 2^16: exact
    c = trail ? MOT_SCENE_TRAIL : (h.x < j.min_static_hits ? MOT_SCENE_NEW : MOT_SCENE_KNOWN);
  }
  return c;
}
// the wave's points per class, added to count[] (uniform over the wave). EVERY lane of the wave calls this
__device__ __forceinline__ void sj_tally(int bits, int (&count)[MOT_SCENE_CLASSES]) {
  const unsigned long long a0 = __ballot(bits & 1), a1 = __ballot(bits & 2), a2 = __ballot(bits & 4);
#pragma unroll
  for (int cc = 0; cc < MOT_SCENE_CLASSES; cc++) count[cc] += __popcll(sj_lanes_of(cc, a0, a1, a2));
}
// the waves' counts merged through LDS into the chunk's row (plain stores). EVERY thread of the workgroup calls this
__device__ __forceinline__ void sj_store_counts(int (*s_cnt)[MOT_SCENE_CLASSES], const int (&count)[MOT_SCENE_CLASSES], int* __restrict__ row, int tid, int lane, int wave) {
  if (lane == 0) {
#pragma unroll
    for (int cc = 0; cc < MOT_SCENE_CLASSES; cc++) s_cnt[wave][cc] = count[cc];
  }
  __syncthreads();
  if (tid < MOT_SCENE_CLASSES) {
    int sum = 0;
#pragma unroll
    for (int w = 0; w < kSjWaves; w++) sum += s_cnt[w][tid];
    row[tid] = sum;
  }
}

// rows[chunk][c] (counts) -> rows[chunk][5 + c]: per class the exclusive scan over the frame's chunks (block_scan_excl_i32 of mot_wave.h), s_total[c] = the class's points
// (readable behind the caller's barrier). Chunks tid, tid + 256, ... per thread; every thread takes part in every scan.
__device__ __forceinline__ void sj_scan_chunks(int* __restrict__ rows, int chunks, int* s_part, int* s_total, int tid) {
  for (int c = 0; c < MOT_SCENE_CLASSES; c++) {
    int carry = 0;   // the class's points in the chunks of earlier rounds
    for (int r0 = 0; r0 < chunks; r0 += kSceneBlock) {   // (uniform)
      const int ch = r0 + tid;
      const int v = ch < chunks ? rows[(long)ch * kSceneJudgeRow + c] : 0;
      int total;
      const int first = carry + block_scan_excl_i32<kSjWaves>(v, s_part, total);
      carry += total;
      __syncthreads();   // (s_part is written again in the next round)
      if (ch < chunks) rows[(long)ch * kSceneJudgeRow + MOT_SCENE_CLASSES + c] = first;
    }
    if (tid == 0) s_total[c] = carry;
  }
}

// THE per-slot scan body (scene_judge_scan_kernel, map_judge_scan_kernel; ONE workgroup per slot): the chunks of slot b scanned per class, the mask applied, the
// slot's segment table `seg` ([5] of the caller's), and the segment starts added to every chunk's places
__device__ __forceinline__ void sj_scan_body(const SceneSplatInput& in, const SceneJudgeBuffers& j, int b, mot_scene_segment* __restrict__ seg, int* s_part, int* s_total) {
  const int tid = threadIdx.x;
  const int chunks = sj_chunks(in, j, b);
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
    int* o = reinterpret_cast<int*>(seg + tid);
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

// the in-chunk ranking, a wave's share: the lane's rank among the points of its class inside the 64-point tile, and the tile's five counts into the LDS table
__device__ __forceinline__ int sj_rank(int cls, int tile, int lane, unsigned long long below, int (*s_cnt)[MOT_SCENE_CLASSES]) {
  const unsigned long long a0 = __ballot(cls & 1), a1 = __ballot(cls & 2), a2 = __ballot(cls & 4);
  if (lane < MOT_SCENE_CLASSES) s_cnt[tile][lane] = __popcll(sj_lanes_of(lane, a0, a1, a2));
  return __popcll(sj_lanes_of(cls, a0, a1, a2) & below);
}
// ... and thread c < 5 chains the chunk's tiles of class c, in index order, from where the chunk's first record of the class goes
__device__ __forceinline__ void sj_chain(const int (*s_cnt)[MOT_SCENE_CLASSES], int (*s_at)[MOT_SCENE_CLASSES], int c, int run) {
  for (int t = 0; t < kSjTiles; t++) { s_at[t][c] = run; run += s_cnt[t][c]; }
}
// one 16-byte record {x, y, z, index}: the point's bits, or (global) mot_track_place.h's sensor -> global step — fp32, left to right; the build has -ffp-contract=off:
// the bits mot_export_track_points_dev writes. THE record expression: the voxel kernels (scene_voxels_seq.hip) take their coordinates from it as well
__device__ __forceinline__ float4 sj_record(bool global, const EgoTf& m, const float4& q, int index) {
  float4 o;
  if (global) {
    o.x = m.m[0] * q.x + m.m[1] * q.y + m.m[2] * q.z + m.m[3];
    o.y = m.m[4] * q.x + m.m[5] * q.y + m.m[6] * q.z + m.m[7];
    o.z = m.m[8] * q.x + m.m[9] * q.y + m.m[10] * q.z + m.m[11];
  } else { o.x = q.x; o.y = q.y; o.z = q.z; }
  o.w = __int_as_float(index);
  return o;
}
// where the scatter body's records go: the caller's block, one 16-byte store where it is aligned
struct SjRecordStore {
  mot_track_point* __restrict__ out; bool vec_out;
  __device__ __forceinline__ void operator()(long dst, const float4& o) const {
    if (vec_out) *reinterpret_cast<float4*>(out + dst) = o;
    else { float* p = reinterpret_cast<float*>(out + dst); p[0] = o.x; p[1] = o.y; p[2] = o.z; p[3] = o.w; }
  }
};

// THE classify body: chunk blockIdx.x of frame `slot` judged against the grid of slot `of`. What the two kernels decide for themselves and hand in:
//   live (scene_judge_classify_kernel)          of = slot = b: the slot's own header, validity and cells; kind = SceneKindLive; the caller's class block at kb
//   recorded (scene_judge_seq_classify_kernel)  of = 0, slot = k: slot 0's header, validity and cells; kind = SceneKindRecorded of frame k; the class block at k
// The kind is asked of EVERY valid owned point — MOVING needs no cell (the splat body asks only points inside the window). `user`: the frame's share of the
// caller's class block, or null. Every thread of a workgroup that passes the exit reaches every ballot and the barrier of sj_store_counts.
template <class Kind>
__device__ __forceinline__ void sj_classify_body(const SceneGridBuffers& g, const SceneSplatInput& in, const SceneJudgeBuffers& j, int of, int slot, const EgoTf* __restrict__ tf,
                                                 const Kind& kind, uint8_t* __restrict__ user, long class_stride, int (*s_cnt)[MOT_SCENE_CLASSES]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int W = g.W;
  const int n = scene_count(in, slot);
  const long base = (long)blockIdx.x * kSceneChunk;
  if (base >= n || (int)blockIdx.x >= j.max_chunks) return;   // (uniform over the workgroup)
  const int oi = g.hdr[of].origin_i, oj = g.hdr[of].origin_j;
  const bool window_ok = g.prev[of].ok != 0;   // the latest accepted step (the drive's last frame) placed its window; 0 after the setter, a reset or a load
  const EgoTf m = *tf;
  const float inv = g.inv;
  const SceneCell* __restrict__ cells = g.cells + (long)of * W * W;
  uint8_t* __restrict__ cls_out = j.cls + (long)slot * in.cap;
  int id[kSceneItems];
  float4 q[kSceneItems];
  scene_load_points(in, slot, base, n, tid, id, q);
  const SceneRect window = {oi, oi + W, oj, oj + W};
  int count[MOT_SCENE_CLASSES] = {0, 0, 0, 0, 0};   // of this wave (uniform)
#pragma unroll
  for (int k = 0; k < kSceneItems; k++) {
    const long i = base + k * kSceneBlock + tid;
    const bool valid = i < n;
    const int dynamic = (valid && id[k] >= 0) ? kind.dynamic(id[k]) : 0;
    float gz;
    const int at = scene_point_cell(m, q[k], inv, valid && window_ok, window, W, &gz);   // (mot_scene_splat.h: the cell the point would be counted in)
    const int c = sj_class(dynamic, at, cells, j);
    if (valid) {
      cls_out[i] = (uint8_t)c;
      if (user && i < class_stride) user[i] = (uint8_t)c;
    }
    sj_tally(valid ? c : kSjNone, count);
  }
  sj_store_counts(s_cnt, count, j.rows + ((long)slot * j.max_chunks + blockIdx.x) * kSceneJudgeRow, tid, lane, wave);
}

// THE scatter body (no kind: it reads the classify body's bytes): the selected records of chunk blockIdx.x of frame `slot` into `out`, below `lim`.
//   live (scene_judge_scatter_kernel)          kDrive = false: the chain starts at row[5 + c]; out = the caller's block kb, lim = point_stride, dst >= lim is skipped
//   recorded (scene_judge_seq_scatter_kernel)  kDrive = true: the chain starts at bases[c] + row[5 + c] (bases: frame k's five drive-wide places); out = the drive's ONE
//                                              block, lim = its capacity, dst < 0 || dst >= lim is skipped
// tf: the frame's matrix (entry kb / k of what the launch was given) when the records are global, else null. Only the points of selected classes are loaded.
// sink(dst, record): what is done with the record of place dst < lim — the two scatter kernels store it (SjRecordStore), the voxel key kernel keeps its cell as well.
template <bool kDrive, class Sink>
__device__ __forceinline__ void sj_scatter_body(const SceneSplatInput& in, const SceneJudgeBuffers& j, int slot, const int* __restrict__ bases, const EgoTf* __restrict__ tf,
                                                long lim, int (*s_cnt)[MOT_SCENE_CLASSES], int (*s_at)[MOT_SCENE_CLASSES], const Sink& sink) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = scene_count(in, slot);
  const long base = (long)blockIdx.x * kSceneChunk;
  if (base >= n || (int)blockIdx.x >= j.max_chunks) return;   // (uniform over the workgroup)
  const uint8_t* __restrict__ cls_in = j.cls + (long)slot * in.cap;
  const float4* __restrict__ cloud = in.elevated + (long)slot * in.cap;
  const int* __restrict__ row = j.rows + ((long)slot * j.max_chunks + blockIdx.x) * kSceneJudgeRow;
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
  for (int k = 0; k < kSceneItems; k++) rank[k] = sj_rank(cls[k], k * kSjWaves + wave, lane, below, s_cnt);   // tile k * 4 + wave of the chunk: points 64 * tile .. 64 * tile + 63
  __syncthreads();
  if (tid < MOT_SCENE_CLASSES) sj_chain(s_cnt, s_at, tid, kDrive ? bases[tid] + row[MOT_SCENE_CLASSES + tid] : row[MOT_SCENE_CLASSES + tid]);   // the chunk's tiles in index order
  __syncthreads();
  const EgoTf m = tf ? *tf : EgoTf();
#pragma unroll
  for (int k = 0; k < kSceneItems; k++) {
    const long i = base + k * kSceneBlock + tid;
    if (cls[k] >= MOT_SCENE_CLASSES || !((j.class_mask >> cls[k]) & 1)) continue;
    const long dst = (long)s_at[k * kSjWaves + wave][cls[k]] + rank[k];
    if ((kDrive && dst < 0) || dst >= lim) continue;   // never a store outside the slot's records / the caller's block (live: dst < n while the rows are this call's)
    sink(dst, sj_record(tf != nullptr, m, q[k], (int)i));
  }
}
template <bool kDrive>
__device__ __forceinline__ void sj_scatter_body(const SceneSplatInput& in, const SceneJudgeBuffers& j, int slot, const int* __restrict__ bases, const EgoTf* __restrict__ tf,
                                                mot_track_point* __restrict__ out, long lim, int (*s_cnt)[MOT_SCENE_CLASSES], int (*s_at)[MOT_SCENE_CLASSES]) {
  sj_scatter_body<kDrive>(in, j, slot, bases, tf, lim, s_cnt, s_at, SjRecordStore{out, (reinterpret_cast<uintptr_t>(out) & 15) == 0});
}
#endif
