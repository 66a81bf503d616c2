// scene_voxels_seq.hip — the voxel-thinned static map of a recorded drive, on gfx950. Product code (HIP, wave64).
//
// scene_judge_seq.hip gives the drive's selected records as one run in the global frame: the same wall once per frame that saw it. Here the same records — the same
// verdicts (sj_classify_body, behind mot_launch_scene_judge_seq_count), the same places and the same record expression (sj_scatter_body, sj_record) — are reduced to
// ONE RECORD PER OCCUPIED VOXEL of a lattice anchored at the global origin: the centroid of the cell's records and their number, in ascending (i_z, i_y, i_x)
// (include/mot.h, "voxel-thinned static map of a recorded drive"). A drive has millions of records: the sort that groups them by cell runs in global memory (mot_sort.h).
//
//   X1  scene_voxels_seq_key_kernel    the scatter kernel's geometry and body: a record of place p below the capacity leaves its 64-bit cell key at key[p], p itself as
//                                      the payload and its 16 bytes at staged[p]; a record outside the lattice gets the all-ones key. Workgroup (0, 0) writes the plan:
//                                      the drive's selected records and how many of them are in play
//       the sort                       mot_sort_launch over 56 bits: 7 passes of three launches; stable, so a cell's records stay in record order
//   X2  scene_voxels_seq_heads_kernel  per tile of 2048 sorted positions: the run heads (a cell that differs from its predecessor's) and the all-ones keys, counted
//   X3  scene_voxels_seq_scan_kernel   ONE workgroup: the exclusive scan of the tiles' counts (block_scan_excl_i32), the totals into the plan — used twice: for the
//                                      heads (runs, n_outside) and for the kept runs (n_voxels, and the header and the caller's totals)
//   X4  scene_voxels_seq_runs_kernel   the heads again, ranked inside the tile: run r starts at start[r] (the run table, in the key buffer the sort left free)
//   X5  scene_voxels_seq_kept_kernel   per tile of 2048 runs: those with min_points records or more, counted; and behind X3 a second launch of the SAME kernel ranks
//                                      them: voxel[r] = the run's place among the kept voxels, -1 for a sparse run
//   X6  scene_voxels_seq_write_kernel  one wave per run, a grid-stride loop: lane l adds records l, l + 64, ... of the run in fp64, the 64 sums are added in lane order
//                                      (include/mot.h, CENTROID: a fixed order whatever runs where), (float)(S / n), one 16-byte store per kept voxel below the capacity
//
// 3 (the judge's counts) + 1 + 21 + 6 + 1 launches whatever `frames` and the data are (the last one only with a voxel block). No global atomics, no workgroup waits on another: the order between the
// launches is the only synchronisation; every count and place is a sum of integers over a fixed set.
// INDEX SAFETY. The launches are sized by the call's record_capacity; every kernel reads the records in play, m' = min(selected records, capacity),
// from the plan and clamps it to the capacity; every load of a key, a payload, a staged record, a run start or a voxel place is below m'; a payload is used only
// below m'; a run's bounds are clamped to the valid positions; a voxel is stored only below the caller's voxel_capacity. Positions are int32 (the host refuses a
// capacity beyond 2^31 - 1).
// Resources (tools/kernel_resources.py): profiles/scene_voxels_sequence.md.
#include "mot_scene_judge.h"
#include "mot_voxel_runs.h"   // sv_key (THE cell rule), the plan's ints, sv_heads_body: shared with voxel_merge.hip

static_assert(sizeof(mot_scene_voxel_header) == 32 && sizeof(mot_model_voxel) == 16, "include/mot.h documents the sizes");
static_assert(kSortTile == 2048, "SceneVoxelBuffers::tiles and mot_scene_voxel_scratch_bytes count tiles of 2048");
constexpr int kSvWriteBlocks = 16384;   // workgroups of X6 at the most (four runs a round each)

// ------------------------------------------------------------------------------------------ X1
struct SvKeySink {
  unsigned long long* __restrict__ key; unsigned* __restrict__ val; float4* __restrict__ staged; SceneVoxelArgs a;
  __device__ __forceinline__ void operator()(long dst, const float4& o) const { key[dst] = sv_key(o, a); val[dst] = (unsigned)dst; staged[dst] = o; }
};
__global__ void MOT_SG_BOUNDS(kSceneBlock)
scene_voxels_seq_key_kernel(SceneSplatInput in, SceneJudgeBuffers j, const int* __restrict__ bases, const EgoTf* __restrict__ tf, SceneVoxelBuffers v, SceneVoxelArgs a, int frames) {
  __shared__ int s_cnt[kSjTiles][MOT_SCENE_CLASSES];
  __shared__ int s_at[kSjTiles][MOT_SCENE_CLASSES];
  const int k = blockIdx.y;
  if (blockIdx.x == 0 && k == 0 && threadIdx.x == 0) {   // the plan (read by the launches behind this one)
    const mot_scene_segment* tot = v.tab + (long)frames * MOT_SCENE_CLASSES;
    long m = 0;
    for (int c = 0; c < MOT_SCENE_CLASSES; c++)
      if ((j.class_mask >> c) & 1) m += tot[c].count;
    if (m < 0) m = 0;
    if (m > 2147483647L) m = 2147483647L;
    v.plan[kSvRecords] = (int)m; v.plan[kSvPlay] = m > v.cap ? v.cap : (int)m;
  }
  sj_scatter_body<true>(in, j, k, bases + k * MOT_SCENE_CLASSES, tf + k, (long)v.cap, s_cnt, s_at, SvKeySink{v.key[0], v.val[0], v.staged, a});
}

// ------------------------------------------------------------------------------------------ X2, X4
// sv_heads_body (mot_voxel_runs.h): the tile's run heads and all-ones keys, counted (X2) or ranked into the run table (X4)
__global__ void MOT_SORT_BOUNDS(kSortBlock) scene_voxels_seq_heads_kernel(SceneVoxelBuffers v) {
  __shared__ int s_part[kSortWaves * 2];
  sv_heads_body<false>(v, s_part);
}
__global__ void MOT_SORT_BOUNDS(kSortBlock) scene_voxels_seq_runs_kernel(SceneVoxelBuffers v) {
  __shared__ int s_part[kSortWaves * 2];
  sv_heads_body<true>(v, s_part);
}

// ------------------------------------------------------------------------------------------ X3
// stage 0: part[0][t] (heads) scanned over the tiles of the records in play, part[1][t] summed -> runs, n_outside. stage 1: part[2][t] (kept runs) scanned over the
// tiles of the runs -> n_voxels, the header, the caller's totals
__global__ void MOT_SORT_BOUNDS(kSortBlock)
scene_voxels_seq_scan_kernel(SceneVoxelBuffers v, int stage, int frames, long voxel_capacity, mot_scene_voxel_header* __restrict__ header, mot_scene_segment* __restrict__ totals) {
  __shared__ int s_part[kSortWaves * 2];
  const int tid = threadIdx.x;
  const int n = sv_play(v);
  int of = n;
  if (stage) { of = v.plan[kSvRuns]; of = of < 0 ? 0 : (of > n ? n : of); }
  int live = (int)(((long)of + kSortTile - 1) / kSortTile);
  if (live > v.tiles) live = v.tiles;
  int* __restrict__ a = v.part + (stage ? 2 * v.tiles : 0);
  const int* __restrict__ b = v.part + v.tiles;
  int sum_a = 0, sum_b = 0;
  for (int t0 = 0; t0 < live; t0 += kSortBlock) {   // (uniform)
    const int t = t0 + tid;
    const int in[2] = {t < live ? a[t] : 0, (!stage && t < live) ? b[t] : 0};
    int before[2], all[2];
    block_scan_excl_i32<kSortWaves, 2>(in, s_part, before, all);
    __syncthreads();   // (s_part is written again in the next round)
    if (t < live) a[t] = sum_a + before[0];
    sum_a += all[0]; sum_b += all[1];
  }
  if (!stage) {
    if (tid == 0) { v.plan[kSvRuns] = sum_a; v.plan[kSvOutsideN] = sum_b; }
    return;
  }
  if (tid == 0) {
    v.plan[kSvVoxels] = sum_a;
    int* h = reinterpret_cast<int*>(header);   // (4-byte aligned: the host checked)
    const int m = v.plan[kSvRecords];
    h[0] = m; h[1] = m - n; h[2] = v.plan[kSvOutsideN]; h[3] = sum_a; h[4] = of - sum_a; h[5] = sum_a > voxel_capacity ? (int)voxel_capacity : sum_a; h[6] = 0; h[7] = 0;
  }
  if (totals && tid < 2 * MOT_SCENE_CLASSES) reinterpret_cast<int*>(totals)[tid] = reinterpret_cast<const int*>(v.tab + (long)frames * MOT_SCENE_CLASSES)[tid];
}

// ------------------------------------------------------------------------------------------ X5
// thread t owns runs base + 8 t .. base + 8 t + 7 of the tile. kWrite = false: the tile's kept runs; true: every run's place among the kept voxels (-1: sparse)
template <bool kWrite>
__device__ __forceinline__ void sv_kept_body(const SceneVoxelBuffers& v, const SceneVoxelArgs& a, int* s_part) {
  const int tid = threadIdx.x, tile = blockIdx.x;
  const int n = sv_play(v);
  int R = v.plan[kSvRuns]; R = R < 0 ? 0 : (R > n ? n : R);
  int valid = n - v.plan[kSvOutsideN]; valid = valid < 0 ? 0 : (valid > n ? n : valid);   // the sorted positions that hold a cell
  const long base = (long)tile * kSortTile;
  if (base >= R || tile >= v.tiles) return;   // (uniform over the workgroup)
  int* __restrict__ start = reinterpret_cast<int*>(v.key[kSvSorted ^ 1]);
  int* __restrict__ voxel = start + v.cap;
  unsigned kept = 0;
  const long r0 = base + (long)tid * kSortItems;
#pragma unroll
  for (int q = 0; q < kSortItems; q++) {
    const long r = r0 + q;
    if (r >= R) break;
    const int end = r + 1 < R ? start[r + 1] : valid;
    if (end - start[r] >= a.min_points) kept |= 1u << q;
  }
  int all;
  const int before = block_scan_excl_i32<kSortWaves>((int)__popc(kept), s_part, all);
  if (!kWrite) {
    if (tid == 0) v.part[2 * v.tiles + tile] = all;
    return;
  }
  int at = v.part[2 * v.tiles + tile] + before;   // (X3 turned the tile's count into the kept runs of earlier tiles)
#pragma unroll
  for (int q = 0; q < kSortItems; q++) {
    const long r = r0 + q;
    if (r >= R) break;
    voxel[r] = ((kept >> q) & 1) ? at++ : -1;
  }
}
__global__ void MOT_SORT_BOUNDS(kSortBlock) scene_voxels_seq_kept_kernel(SceneVoxelBuffers v, SceneVoxelArgs a, int rank) {
  __shared__ int s_part[kSortWaves];
  if (rank) sv_kept_body<true>(v, a, s_part); else sv_kept_body<false>(v, a, s_part);
}

// ------------------------------------------------------------------------------------------ X6
__global__ void MOT_SORT_BOUNDS(kSortBlock)
scene_voxels_seq_write_kernel(SceneVoxelBuffers v, mot_model_voxel* __restrict__ out, long voxel_capacity) {
  __shared__ double s_acc[kSortWaves][3][64];
  __shared__ float s_out[kSortWaves][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = sv_play(v);
  int R = v.plan[kSvRuns]; R = R < 0 ? 0 : (R > n ? n : R);
  int valid = n - v.plan[kSvOutsideN]; valid = valid < 0 ? 0 : (valid > n ? n : valid);
  const int* __restrict__ start = reinterpret_cast<const int*>(v.key[kSvSorted ^ 1]);
  const int* __restrict__ voxel = start + v.cap;
  const unsigned* __restrict__ src = v.val[kSvSorted];
  for (long r = (long)blockIdx.x * kSortWaves + wave; r < R; r += (long)gridDim.x * kSortWaves) {   // (r is the wave's: every branch on it is uniform over the wave)
    const int at = voxel[r];
    if (at < 0 || at >= voxel_capacity) continue;
    int s = start[r], e = r + 1 < R ? start[r + 1] : valid;
    s = s < 0 ? 0 : s; e = e > valid ? valid : e;
    const int len = e - s;
    if (len <= 0) continue;
    double ax = 0.0, ay = 0.0, az = 0.0;
    bool first = true;
    for (long p = (long)s + lane; p < e; p += 64) {   // lane l: records l, l + 64, ... of the run, each sum starting from its first record
      const unsigned i = src[p];
      if (i >= (unsigned)n) continue;   // (never: the payloads are this call's record positions)
      const float4 q = v.staged[i];
      if (first) { ax = (double)q.x; ay = (double)q.y; az = (double)q.z; first = false; }
      else { ax = ax + (double)q.x; ay = ay + (double)q.y; az = az + (double)q.z; }
    }
    s_acc[wave][0][lane] = ax; s_acc[wave][1][lane] = ay; s_acc[wave][2][lane] = az;
    MOT_WAVE_SYNC();
    if (lane < 3) {   // lane a adds axis a's sums in lane order
      const int m = len < 64 ? len : 64;
      double S = s_acc[wave][lane][0];
      for (int l = 1; l < m; l++) S = S + s_acc[wave][lane][l];
      s_out[wave][lane] = (float)(S / (double)len);
    }
    MOT_WAVE_SYNC();
    if (lane == 0) *reinterpret_cast<float4*>(out + at) = make_float4(s_out[wave][0], s_out[wave][1], s_out[wave][2], __int_as_float(len));
    MOT_WAVE_SYNC();   // (s_out is read: the next round may write it)
  }
}

// ------------------------------------------------------------------------------------------ host
void mot_launch_scene_voxels_seq_count(const SceneSplatInput& in, const SceneJudgeBuffers& j, const int* bases, int frames, int max_n, const EgoTf* tf, const SceneVoxelBuffers& v,
                                       const SceneVoxelArgs& a, long voxel_capacity, mot_scene_voxel_header* header, mot_scene_segment* totals, hipStream_t stream) {
  hipLaunchKernelGGL(scene_voxels_seq_key_kernel, dim3(mot_launch_chunks(max_n, kSceneChunk, j.max_chunks), frames), dim3(kSceneBlock), 0, stream, in, j, bases, tf, v, a, frames);
  SortBuffers s;
  s.key[0] = v.key[0]; s.key[1] = v.key[1]; s.val[0] = v.val[0]; s.val[1] = v.val[1]; s.table = v.table; s.totals = v.totals; s.n = v.plan + kSvPlay; s.cap = v.cap;
  (void)mot_sort_launch(s, kSceneVoxelKeyBits, stream);
  hipLaunchKernelGGL(scene_voxels_seq_heads_kernel, dim3(v.tiles), dim3(kSortBlock), 0, stream, v);
  hipLaunchKernelGGL(scene_voxels_seq_scan_kernel, dim3(1), dim3(kSortBlock), 0, stream, v, 0, frames, voxel_capacity, header, totals);
  hipLaunchKernelGGL(scene_voxels_seq_runs_kernel, dim3(v.tiles), dim3(kSortBlock), 0, stream, v);
  hipLaunchKernelGGL(scene_voxels_seq_kept_kernel, dim3(v.tiles), dim3(kSortBlock), 0, stream, v, a, 0);
  hipLaunchKernelGGL(scene_voxels_seq_scan_kernel, dim3(1), dim3(kSortBlock), 0, stream, v, 1, frames, voxel_capacity, header, totals);
  hipLaunchKernelGGL(scene_voxels_seq_kept_kernel, dim3(v.tiles), dim3(kSortBlock), 0, stream, v, a, 1);
}
void mot_launch_scene_voxels_seq_write(const SceneVoxelBuffers& v, mot_model_voxel* voxels, long voxel_capacity, hipStream_t stream) {
  if (!voxels || voxel_capacity <= 0) return;
  const long blocks = ((long)v.cap + kSortWaves - 1) / kSortWaves;
  hipLaunchKernelGGL(scene_voxels_seq_write_kernel, dim3((unsigned)(blocks < 1 ? 1 : (blocks > kSvWriteBlocks ? kSvWriteBlocks : blocks))), dim3(kSortBlock), 0, stream, v, voxels, voxel_capacity);
}
