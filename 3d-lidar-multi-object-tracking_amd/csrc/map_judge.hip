// map_judge.hip — a frame's points judged against a voxel index of earlier maps, on gfx950: change detection. Product code (HIP, wave64).
//
// voxel_merge.hip writes the index (mot_index_voxel_maps_dev: the occupied cells' keys, strictly ascending, and their summed counts); the kernels here ask it a
// question about the live frame (include/mot.h, "a frame's points judged against a voxel map"): every elevated point of a fused step gets one of five classes —
// OUTSIDE, MOVING, SPARSE, ABSENT, PRESENT — and the points are partitioned by class, in input order, into the caller's block, in the shape scene_judge.hip gives.
// The index is only READ; the scene grid is not read at all (the calls work with the grid off). The reference has no such output.
//
//   K1  map_judge_classify_kernel  grid (ceil(N_e / 2048), B), 256 threads, 8 points a thread — the geometry of J1. Per point the 12-byte point (16 in the float4
//                                  layout), the 4-byte id, for an owned point the two dependent gathers of the live kind rule (SceneKindLive), the global record
//                                  (sj_record: the bits the MOT_FRAME_GLOBAL export writes, the bits the drive's map was made from) and its cell (sv_key: THE
//                                  cell rule, the map's own device function). Then the search of keys[0 .. n), n = clamp(*n_stored, 0, capacity) read here:
//                                  reach 0 — ONE lower bound and one compare; reach 1 — nine lower bounds, one per row (i_z + d_z, i_y + d_y) inside the lattice,
//                                  each for the row's key at max(i_x - 1, -2^20), followed by at most three consecutive entries while the key stays <= the row's
//                                  key at min(i_x + 1, 2^20 - 1): the three x-neighbours are adjacent in key order. The fields of a neighbour's key are composed
//                                  from its three clamped indices, never by arithmetic on the key: nothing carries from one field into the next, and a neighbour
//                                  outside the lattice is not looked up. Of a run of neighbouring lanes with the same cell (beam-major clouds: most of a wave)
//                                  only the first lane searches; the others take its verdict by one shuffle — the class is a function of the cell alone.
//                                  The class byte to the feature's scratch (and to the caller's class block), the chunk's five counts as plain stores
//   K2  map_judge_scan_kernel      one workgroup per slot: sj_scan_body, the text of J2
//   K3  map_judge_scatter_kernel   the grid of K1: sj_scatter_body<false>, the text of J3
//
// Three launches whatever the data (two without a mask or room for records). No global atomics, no workgroup waits on another, every count and every place is a sum
// of integers over a fixed set, a verdict depends on the point's cell and the index alone: the output does not depend on the order in which workgroups or waves run.
// INDEX SAFETY. Point, id and class loads stay below min(count, cap) of the slot; an id outside [0, E) or a track slot outside [0, T) is not followed;
// every key or count load is at a position below n <= capacity; a lower bound halves its range in at most 32 steps (kMjSteps: a fixed bound, n < 2^31), the walk
// behind it takes at most three; chunk rows are indexed below the slot's chunk capacity; a record is stored only below min(point_stride, selected records), a class
// byte only below class_stride. An index whose content the index call did not write (keys out of order, say) gives unspecified classes — never a load outside the
// blocks, never a loop without end.
// Resources (tools/kernel_resources.py): no scratch. Cost: profiles/map_judge.md (tools/time_map_judge.py).
// Out of scope here: a recorded drive's (sequence slots') variant, host-block variants of the index call, reach > 1, updating an index in place.
#include "mot_scene_judge.h"
#include "mot_voxel_cell.h"   // sv_key, kSvOutside

static_assert(MOT_MAP_CLASSES == MOT_SCENE_CLASSES, "sj_tally, sj_store_counts, sj_scan_chunks, sj_rank, sj_chain and sj_scatter_body serve both judges");
static_assert(MOT_MAP_PRESENT < 8, "a class is three bits");
constexpr int kMjSteps = 32;                       // steps of a lower bound at the most
constexpr int kMjXY = 1 << 21, kMjZ = 1 << 12;     // biased indices: x, y in [0, 2^21), z in [0, 2^12)

// the first position in [0, n) whose key is not below `key` (n when there is none); every load below n
__device__ __forceinline__ int mj_lower_bound(const unsigned long long* __restrict__ keys, int n, unsigned long long key) {
  int lo = 0, len = n;
  for (int step = 0; step < kMjSteps && len > 0; step++) {
    const int half = len >> 1;
    if (keys[lo + half] < key) { lo += half + 1; len -= half + 1; }
    else len = half;
  }
  return lo;
}
// bit 0: a cell of the neighbourhood is in the index; bit 1: one of them holds min_count or more
__device__ __forceinline__ int mj_lookup(const MapJudgeIndex& x, int n, unsigned long long key) {
  if (x.reach == 0) {
    const int p = mj_lower_bound(x.keys, n, key);
    if (p >= n || x.keys[p] != key) return 0;
    return x.counts[p] >= x.min_count ? 3 : 1;
  }
  const int bx = (int)(key & (kMjXY - 1)), by = (int)((key >> 21) & (kMjXY - 1)), bz = (int)(key >> 42) & (kMjZ - 1);
  const unsigned long long x0 = (unsigned long long)(bx > 0 ? bx - 1 : 0), x1 = (unsigned long long)(bx < kMjXY - 1 ? bx + 1 : kMjXY - 1);
  int seen = 0;
  for (int dz = -1; dz <= 1; dz++) {
    const int z = bz + dz;
    if (z < 0 || z >= kMjZ) continue;   // (a neighbour outside the lattice is in no map)
    for (int dy = -1; dy <= 1; dy++) {
      const int y = by + dy;
      if (y < 0 || y >= kMjXY) continue;
      const unsigned long long row = ((unsigned long long)z << 42) | ((unsigned long long)y << 21);
      const unsigned long long hi = row | x1;
      int p = mj_lower_bound(x.keys, n, row | x0);
      for (int t = 0; t < 3 && p < n; t++, p++) {
        if (x.keys[p] > hi) break;
        seen |= 1;
        if (x.counts[p] >= x.min_count) return 3;
      }
    }
  }
  return seen;
}

// ------------------------------------------------------------------------------------------ K1
__global__ void MOT_SG_BOUNDS(kSceneBlock)
map_judge_classify_kernel(SceneSplatInput in, SceneJudgeBuffers j, MapJudgeIndex x, int b0, const EgoTf* __restrict__ tf, uint8_t* __restrict__ classes, long class_stride) {
  __shared__ int s_cnt[kSjWaves][MOT_SCENE_CLASSES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kb = blockIdx.y, b = b0 + kb;   // slot b; block kb of the caller's
  const int n = scene_count(in, b);
  const long base = (long)blockIdx.x * kSceneChunk;
  if (base >= n || (int)blockIdx.x >= j.max_chunks) return;   // (uniform over the workgroup)
  int len = *x.n_stored; len = len < 0 ? 0 : (len > x.capacity ? x.capacity : len);   // the index's length, read HERE
  const EgoTf m = tf[kb];
  const SceneKindLive kind(in, b);
  uint8_t* __restrict__ cls_out = j.cls + (long)b * in.cap;
  uint8_t* __restrict__ user = classes ? classes + (long)kb * class_stride : nullptr;
  int id[kSceneItems];
  float4 q[kSceneItems];
  scene_load_points(in, b, base, n, tid, id, q);
  const unsigned long long upto = (2ull << lane) - 1ull;   // lanes 0 .. lane
  int count[MOT_SCENE_CLASSES] = {0, 0, 0, 0, 0};   // of this wave (uniform)
#pragma unroll
  for (int k = 0; k < kSceneItems; k++) {
    const long i = base + k * kSceneBlock + tid;
    const bool valid = i < n;
    const int dynamic = (valid && id[k] >= 0) ? kind.dynamic(id[k]) : 0;
    const unsigned long long key = valid ? sv_key(sj_record(true, m, q[k], 0), x.a) : kSvOutside;
    // the first lane of a run of equal keys searches for the run (EVERY lane of the wave reaches the shuffles and the ballot)
    const unsigned long long before = __shfl_up(key, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || before != key);
    int found = 0;
    if (((heads >> lane) & 1) && key != kSvOutside) found = mj_lookup(x, len, key);
    found = __shfl(found, 63 - __clzll((long long)(heads & upto)), 64);
    int c = MOT_MAP_ABSENT;
    if (dynamic) c = MOT_MAP_MOVING;
    else if (key == kSvOutside) c = MOT_MAP_OUTSIDE;
    else if (found & 2) c = MOT_MAP_PRESENT;
    else if (found & 1) c = MOT_MAP_SPARSE;
    if (valid) {
      cls_out[i] = (uint8_t)c;
      if (user && i < class_stride) user[i] = (uint8_t)c;
    }
    sj_tally(valid ? c : kSjNone, count);
  }
  sj_store_counts(s_cnt, count, j.rows + ((long)b * j.max_chunks + blockIdx.x) * kSceneJudgeRow, tid, lane, wave);
}

// ------------------------------------------------------------------------------------------ K2
__global__ void MOT_SG_BOUNDS(kSceneBlock)
map_judge_scan_kernel(SceneSplatInput in, SceneJudgeBuffers j, int b0, mot_scene_segment* __restrict__ segments) {
  __shared__ int s_part[kSjWaves];
  __shared__ int s_total[MOT_SCENE_CLASSES];
  sj_scan_body(in, j, b0 + blockIdx.x, segments + (long)blockIdx.x * MOT_SCENE_CLASSES, s_part, s_total);
}

// ------------------------------------------------------------------------------------------ K3
__global__ void MOT_SG_BOUNDS(kSceneBlock)
map_judge_scatter_kernel(SceneSplatInput in, SceneJudgeBuffers j, int b0, const EgoTf* __restrict__ tf, mot_track_point* __restrict__ points, long point_stride) {
  __shared__ int s_cnt[kSjTiles][MOT_SCENE_CLASSES];   // points of (tile, class)
  __shared__ int s_at[kSjTiles][MOT_SCENE_CLASSES];    // where the tile's first record of the class goes
  const int kb = blockIdx.y;
  sj_scatter_body<false>(in, j, b0 + kb, nullptr, tf ? tf + kb : nullptr, points + (long)kb * point_stride, point_stride, s_cnt, s_at);
}

// ------------------------------------------------------------------------------------------ host
void mot_launch_map_judge(const SceneSplatInput& in, const SceneJudgeBuffers& j, const MapJudgeIndex& x, int first, int batch, int max_n, const EgoTf* tf, int global,
                          mot_track_point* points, long point_stride, mot_scene_segment* segments, uint8_t* classes, long class_stride, hipStream_t stream) {
  const dim3 grid(mot_launch_chunks(max_n, kSceneChunk, j.max_chunks), batch);
  hipLaunchKernelGGL(map_judge_classify_kernel, grid, dim3(kSceneBlock), 0, stream, in, j, x, first, tf, classes, class_stride);
  hipLaunchKernelGGL(map_judge_scan_kernel, dim3(batch), dim3(kSceneBlock), 0, stream, in, j, first, segments);
  if (j.class_mask && points && point_stride > 0)
    hipLaunchKernelGGL(map_judge_scatter_kernel, grid, dim3(kSceneBlock), 0, stream, in, j, first, global ? tf : nullptr, points, point_stride);
}
