// voxel_merge.hip — up to 16 voxel maps of the global lattice merged into one, on gfx950. Product code (HIP, wave64).
//
// Every voxel export of the library writes 16-byte records {centroid, count}; the lattice is anchored at the global origin, so the maps of a drive's pieces, or of two
// drives, speak of the same cells. Here the maps' voxels — read IN PLACE, the counts of the maps read on the device — are keyed by the cell of their centroid at this
// call's leaf (sv_key, mot_voxel_runs.h: THE cell rule), sorted, cut into runs and reduced to one record per cell: the counts added, the centroids weighted by count
// (include/mot.h, "voxel maps merged into one").
//
//   M1  voxel_merge_key_kernel     over the concatenation of the maps: every workgroup repeats the prefix over the <= 16 clamped counts (LDS); input i leaves its
//                                  64-bit cell key at key[i] and i itself as the payload; count <= 0, a non-finite centroid or a cell outside the lattice: the
//                                  all-ones key. Workgroup 0 writes the plan: the inputs in play and the prefix (read by the launches behind this one)
//       the sort                   mot_sort_launch over 56 bits: 7 passes of three launches; stable, so a cell's inputs stay in concatenation order
//   M2  voxel_merge_heads_kernel   per tile of 2048 sorted positions: run heads and all-ones keys, counted           (sv_heads_body, shared with scene_voxels_seq.hip)
//   M3  voxel_merge_scan_kernel    ONE workgroup, twice: the tiles' run heads scanned, the all-ones keys summed (runs, n_outside); the tiles' kept runs scanned, the
//                                  saturated ones summed (n_voxels, n_saturated, the header)
//   M4  voxel_merge_runs_kernel    the heads again, ranked inside the tile: the run table                           (sv_heads_body)
//   M5  voxel_merge_reduce_kernel  twice. First the summed count W of every run (int64): voxel[r] = 1 kept (W >= min_points), 3 kept and beyond 2^31 - 1, 0 sparse.
//                                  Then, behind M6, the voxels: W again and the fp64 sums of centroid * count, (float)(S / W), one 16-byte store per kept voxel below
//                                  the capacity. Thread t of a workgroup owns run base + t: a run of at most short_max (64) inputs is summed by its thread, left to
//                                  right; the longer ones of a wave's 64 runs are then taken one after another by the whole wave in the order of include/mot.h
//                                  (CENTROID: lane l adds inputs l, l + 64, ..., the 64 sums are added in lane order) — for a run of at most 64 inputs the two orders
//                                  are the same additions, so the cut does not show in the bytes
//   M6  voxel_merge_kept_kernel    per tile of 2048 runs: the kept and the saturated ones, counted; and behind M3 a second launch of the SAME kernel ranks them:
//                                  voxel[r] = the run's place among the kept voxels, -1 for a sparse run
//   M7  voxel_merge_index_kernel   mot_index_voxel_maps_dev alone, in M5's second place: per kept run below the capacity the run's KEY and its saturated W — the
//                                  index of the maps' occupied cells that map_judge.hip searches (29 + 1 launches; 29 with a capacity of 0)
//
// 1 + 21 + 1 + 2 + 1 + 2 + 2 = 30 launches whatever the data and n_maps are (29 without an output block). No global atomics, no workgroup waits on another (no
// look-back): the order between the launches is the only synchronisation; every count and place is a sum of integers over a fixed set, every fp64 sum has a fixed
// order — the output does not depend on how workgroups or waves are scheduled.
// INDEX SAFETY (as mot_sort.h states it for itself). The launches are sized by the sum of the maps' capacities, never by data; every kernel reads the inputs in play,
// n = min(sum of the clamped counts, capacity), from the plan and clamps it; every load of a key, a payload, a run start or a voxel place is below n; a payload is
// used only after a range check (below n, and its position below its map's capacity); a run's bounds are clamped to the valid positions; a voxel is stored only
// below the caller's out_capacity. Positions are int32 (the host refuses a sum of capacities beyond 2^31 - 1).
// Resources (tools/kernel_resources.py) and cost: profiles/voxel_merge.md.
#include "mot_voxel_runs.h"

static_assert(sizeof(mot_voxel_merge_header) == 32 && sizeof(mot_voxel_map_src) == 24 && sizeof(mot_model_voxel) == 16, "include/mot.h documents the sizes");
static_assert(kVoxelMergeMaps == MOT_VOXEL_MERGE_MAX_MAPS && kVoxelMergeMaps == 16, "vm_map's four steps search 16 maps");
static_assert(kVoxelMergePlan >= kVmPrefix + kVoxelMergeMaps + 1, "the plan holds the prefix");
constexpr int kVmBlocks = 16384;   // workgroups of M1 and M5 at the most (grid-stride loops)

// the prefix over the maps' clamped counts in LDS: pre[k] = inputs of the maps before k, pre[k] = n for every k >= n_maps (so that no search ends there)
__device__ __forceinline__ int vm_map(const int* pre, int i) {
  int k = 0;
  if (i >= pre[8]) k = 8;
  if (i >= pre[k + 4]) k += 4;
  if (i >= pre[k + 2]) k += 2;
  if (i >= pre[k + 1]) k += 1;
  return k;
}
// input i of the concatenation, read in place; false (never, while the plan is this call's own): i is no input in play
__device__ __forceinline__ bool vm_input(const VoxelMergeMaps& m, const int* pre, unsigned i, int n, float4* q) {
  if (i >= (unsigned)n) return false;
  const int k = vm_map(pre, (int)i);
  const int pos = (int)i - pre[k];
  if (k >= m.n_maps || pos < 0 || pos >= m.cap[k]) return false;
  *q = reinterpret_cast<const float4*>(m.vox[k])[pos];
  return true;
}
// the plan's prefix into LDS, clamped (every thread of the workgroup; ends with a barrier)
__device__ __forceinline__ void vm_prefix_from_plan(const SceneVoxelBuffers& v, int n, int* s_pre) {
  const int tid = threadIdx.x;
  if (tid <= kVoxelMergeMaps) { const int p = v.plan[kVmPrefix + tid]; s_pre[tid] = p < 0 ? 0 : (p > n ? n : p); }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------ M1
__global__ void MOT_SORT_BOUNDS(kSortBlock) voxel_merge_key_kernel(VoxelMergeMaps m, SceneVoxelBuffers v, SceneVoxelArgs a) {
  __shared__ int s_cnt[kVoxelMergeMaps];
  __shared__ int s_pre[kVoxelMergeMaps + 1];
  const int tid = threadIdx.x;
  if (tid < kVoxelMergeMaps) {   // map tid's inputs: its count, read here, clamped to [0, capacity]
    int c = 0;
    if (tid < m.n_maps) {
      const int cap = m.cap[tid];
      c = m.count[tid] ? *m.count[tid] : cap;
      c = c < 0 ? 0 : (c > cap ? cap : c);
    }
    s_cnt[tid] = c;
  }
  __syncthreads();
  if (tid == 0) {
    long at = 0;
    for (int k = 0; k < kVoxelMergeMaps; k++) { s_pre[k] = (int)at; at += s_cnt[k]; if (at > v.cap) at = v.cap; }   // (the sum of the capacities is v.cap: never clamped)
    s_pre[kVoxelMergeMaps] = (int)at;
  }
  __syncthreads();
  const int n = s_pre[kVoxelMergeMaps];
  if (blockIdx.x == 0 && tid <= kVoxelMergeMaps) {   // the plan
    v.plan[kVmPrefix + tid] = s_pre[tid];
    if (tid == 0) { v.plan[kSvRecords] = n; v.plan[kSvPlay] = n; }
  }
  for (long i = (long)blockIdx.x * kSortBlock + tid; i < n; i += (long)gridDim.x * kSortBlock) {
    float4 q;
    unsigned long long key = kSvOutside;
    if (vm_input(m, s_pre, (unsigned)i, n, &q) && __float_as_int(q.w) > 0) key = sv_key(q, a);
    v.key[0][i] = key; v.val[0][i] = (unsigned)i;
  }
}

// ------------------------------------------------------------------------------------------ M2, M4
__global__ void MOT_SORT_BOUNDS(kSortBlock) voxel_merge_heads_kernel(SceneVoxelBuffers v) {
  __shared__ int s_part[kSortWaves * 2];
  sv_heads_body<false>(v, s_part);
}
__global__ void MOT_SORT_BOUNDS(kSortBlock) voxel_merge_runs_kernel(SceneVoxelBuffers v) {
  __shared__ int s_part[kSortWaves * 2];
  sv_heads_body<true>(v, s_part);
}

// ------------------------------------------------------------------------------------------ M3
// stage 0: part[0][t] (heads) scanned over the tiles of the inputs in play, part[1][t] (all-ones keys) summed -> runs, n_outside. stage 1: part[2][t] (kept runs)
// scanned over the tiles of the runs, part[3][t] (saturated ones) summed -> n_voxels, n_saturated, the header
__global__ void MOT_SORT_BOUNDS(kSortBlock) voxel_merge_scan_kernel(SceneVoxelBuffers v, int stage, long out_capacity, mot_voxel_merge_header* __restrict__ header) {
  __shared__ int s_part[kSortWaves * 2];
  const int tid = threadIdx.x;
  const int n = sv_play(v);
  int of = n;
  if (stage) { of = v.plan[kSvRuns]; of = of < 0 ? 0 : (of > n ? n : of); }
  int live = (int)(((long)of + kSortTile - 1) / kSortTile);
  if (live > v.tiles) live = v.tiles;
  int* __restrict__ a = v.part + (stage ? 2 * v.tiles : 0);
  const int* __restrict__ b = v.part + (stage ? 3 * v.tiles : v.tiles);
  int sum_a = 0, sum_b = 0;
  for (int t0 = 0; t0 < live; t0 += kSortBlock) {   // (uniform)
    const int t = t0 + tid;
    const int in[2] = {t < live ? a[t] : 0, t < live ? b[t] : 0};
    int before[2], all[2];
    block_scan_excl_i32<kSortWaves, 2>(in, s_part, before, all);
    __syncthreads();   // (s_part is written again in the next round)
    if (t < live) a[t] = sum_a + before[0];
    sum_a += all[0]; sum_b += all[1];
  }
  if (tid != 0) return;
  if (!stage) { v.plan[kSvRuns] = sum_a; v.plan[kSvOutsideN] = sum_b; return; }
  v.plan[kSvVoxels] = sum_a;
  int* h = reinterpret_cast<int*>(header);   // (4-byte aligned: the host checked)
  h[0] = n; h[1] = v.plan[kSvOutsideN]; h[2] = sum_a; h[3] = of - sum_a; h[4] = sum_a > out_capacity ? (int)out_capacity : sum_a; h[5] = sum_b; h[6] = 0; h[7] = 0;
}

// ------------------------------------------------------------------------------------------ M5
struct VmSum {
  double x, y, z; long long w; bool first;
  // the term of an input is centroid * count, one fp64 multiply; a sum starts FROM its first term
  template <bool kWrite> __device__ __forceinline__ void add(const float4& q) {
    const int c = __float_as_int(q.w);
    w += c;
    if (!kWrite) return;
    const double tx = (double)q.x * (double)c, ty = (double)q.y * (double)c, tz = (double)q.z * (double)c;
    if (first) { x = tx; y = ty; z = tz; first = false; }
    else { x = x + tx; y = y + ty; z = z + tz; }
  }
};
__device__ __forceinline__ int vm_flag(long long W, int min_points) { return W >= min_points ? (W > 2147483647LL ? 3 : 1) : 0; }
__device__ __forceinline__ int vm_stored(long long W) { return W > 2147483647LL ? 2147483647 : (int)W; }

template <bool kWrite>
__device__ __forceinline__ void vm_reduce_body(const VoxelMergeMaps& m, const SceneVoxelBuffers& v, int min_points, mot_model_voxel* __restrict__ out, long out_capacity, int* s_pre,
                                               double (*s_acc)[3][64], long long (*s_w)[64], float (*s_out)[4]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = sv_play(v);
  int R = v.plan[kSvRuns]; R = R < 0 ? 0 : (R > n ? n : R);
  int valid = n - v.plan[kSvOutsideN]; valid = valid < 0 ? 0 : (valid > n ? n : valid);   // the sorted positions that hold a cell
  vm_prefix_from_plan(v, n, s_pre);
  int* __restrict__ start = reinterpret_cast<int*>(v.key[kSvSorted ^ 1]);
  int* __restrict__ voxel = start + v.cap;
  const unsigned* __restrict__ src = v.val[kSvSorted];
  const int short_max = m.short_max < 0 ? 0 : (m.short_max > 64 ? 64 : m.short_max);
  for (long base = (long)blockIdx.x * kSortBlock; base < R; base += (long)gridDim.x * kSortBlock) {   // (uniform over the workgroup)
    const long r = base + tid;
    int s = 0, e = 0, at = 0;
    if (r < R) {
      s = start[r]; e = r + 1 < R ? start[r + 1] : valid;
      s = s < 0 ? 0 : s; e = e > valid ? valid : e;
      if (kWrite) { at = voxel[r]; if (at < 0 || at >= out_capacity) e = s; }   // (a sparse run, or no room: nothing to do)
    }
    const int len = e - s;
    if (len > 0 && len <= short_max) {   // the thread's own run, left to right
      VmSum t = {0.0, 0.0, 0.0, 0, true};
      for (int p = s; p < e; p++) {
        float4 q;
        if (vm_input(m, s_pre, src[p], n, &q)) t.add<kWrite>(q);
      }
      if (!kWrite) voxel[r] = vm_flag(t.w, min_points);
      else if (t.w > 0) {
        const double W = (double)t.w;
        *reinterpret_cast<float4*>(out + at) = make_float4((float)(t.x / W), (float)(t.y / W), (float)(t.z / W), __int_as_float(vm_stored(t.w)));
      }
    } else if (!kWrite && r < R && len <= 0) voxel[r] = 0;   // (never: a run holds its head)
    unsigned long long longs = __ballot(len > short_max);
    while (longs) {   // the wave's long runs, one after another (uniform over the wave)
      const int l = __ffsll(longs) - 1;
      longs &= longs - 1;
      const int sl = __shfl(s, l), el = __shfl(e, l), atl = __shfl(at, l);
      VmSum t = {0.0, 0.0, 0.0, 0, true};
      for (long p = (long)sl + lane; p < el; p += 64) {   // lane l: inputs l, l + 64, ... of the run
        float4 q;
        if (vm_input(m, s_pre, src[p], n, &q)) t.add<kWrite>(q);
      }
      s_w[wave][lane] = t.w;
      if (kWrite) { s_acc[wave][0][lane] = t.x; s_acc[wave][1][lane] = t.y; s_acc[wave][2][lane] = t.z; }
      MOT_WAVE_SYNC();
      if (lane < (kWrite ? 3 : 1)) {   // lane a adds axis a's sums in lane order (and the counts: integers)
        long long W = 0;
        for (int k = 0; k < 64; k++) W += s_w[wave][k];
        if (!kWrite) voxel[base + wave * 64 + l] = vm_flag(W, min_points);
        else {
          const int terms = el - sl < 64 ? el - sl : 64;
          double S = s_acc[wave][lane][0];
          for (int k = 1; k < terms; k++) S = S + s_acc[wave][lane][k];
          s_out[wave][lane] = W > 0 ? (float)(S / (double)W) : 0.f;
          if (lane == 0) s_out[wave][3] = __int_as_float(vm_stored(W));
        }
      }
      MOT_WAVE_SYNC();
      if (kWrite && lane == 0) *reinterpret_cast<float4*>(out + atl) = make_float4(s_out[wave][0], s_out[wave][1], s_out[wave][2], s_out[wave][3]);
      MOT_WAVE_SYNC();   // (s_w, s_acc and s_out are read: the next round may write them)
    }
  }
}
__global__ void MOT_SORT_BOUNDS(kSortBlock)
voxel_merge_reduce_kernel(VoxelMergeMaps m, SceneVoxelBuffers v, int min_points, int write, mot_model_voxel* __restrict__ out, long out_capacity) {
  __shared__ int s_pre[kVoxelMergeMaps + 1];
  __shared__ double s_acc[kSortWaves][3][64];
  __shared__ long long s_w[kSortWaves][64];
  __shared__ float s_out[kSortWaves][4];
  if (write) vm_reduce_body<true>(m, v, min_points, out, out_capacity, s_pre, s_acc, s_w, s_out);
  else vm_reduce_body<false>(m, v, min_points, out, out_capacity, s_pre, s_acc, s_w, s_out);
}

// ------------------------------------------------------------------------------------------ M6
// thread t owns runs base + 8 t .. base + 8 t + 7 of the tile. kWrite = false: the tile's kept and saturated runs (M5's flags); true: every run's place among the kept
// voxels (-1: sparse)
template <bool kWrite>
__device__ __forceinline__ void vm_kept_body(const SceneVoxelBuffers& v, int* s_part) {
  const int tid = threadIdx.x, tile = blockIdx.x;
  const int n = sv_play(v);
  int R = v.plan[kSvRuns]; R = R < 0 ? 0 : (R > n ? n : R);
  const long base = (long)tile * kSortTile;
  if (base >= R || tile >= v.tiles) return;   // (uniform over the workgroup)
  int* __restrict__ voxel = reinterpret_cast<int*>(v.key[kSvSorted ^ 1]) + v.cap;
  unsigned kept = 0, sat = 0;
  const long r0 = base + (long)tid * kSortItems;
#pragma unroll
  for (int q = 0; q < kSortItems; q++) {
    const long r = r0 + q;
    if (r >= R) break;
    const int f = voxel[r];
    kept |= (unsigned)(f & 1) << q; sat |= (unsigned)((f >> 1) & 1) << q;
  }
  const int cnt[2] = {(int)__popc(kept), (int)__popc(sat)};
  int before[2], all[2];
  block_scan_excl_i32<kSortWaves, 2>(cnt, s_part, before, all);
  if (!kWrite) {
    if (tid == 0) { v.part[2 * v.tiles + tile] = all[0]; v.part[3 * v.tiles + tile] = all[1]; }
    return;
  }
  int at = v.part[2 * v.tiles + tile] + before[0];   // (M3 turned the tile's count into the kept runs of earlier tiles)
#pragma unroll
  for (int q = 0; q < kSortItems; q++) {
    const long r = r0 + q;
    if (r >= R) break;
    voxel[r] = ((kept >> q) & 1) ? at++ : -1;
  }
}
__global__ void MOT_SORT_BOUNDS(kSortBlock) voxel_merge_kept_kernel(SceneVoxelBuffers v, int rank) {
  __shared__ int s_part[kSortWaves * 2];
  if (rank) vm_kept_body<true>(v, s_part); else vm_kept_body<false>(v, s_part);
}

// ------------------------------------------------------------------------------------------ M7 (mot_index_voxel_maps_dev)
// The merge without the centroid: behind M6's ranks, per kept run below the capacity the run's key ITSELF — the sorted key at the run's start, not re-derived from a
// centroid — and W again, saturated. M5's cut (a run of at most short_max inputs by its thread, the longer ones of a wave's 64 runs by the wave); W is a sum of
// integers, so neither the cut nor the order shows. A kernel of its own: M5 keeps its registers and its LDS (tools/kernel_resources.py).
__global__ void MOT_SORT_BOUNDS(kSortBlock)
voxel_merge_index_kernel(VoxelMergeMaps m, SceneVoxelBuffers v, unsigned long long* __restrict__ keys, int* __restrict__ counts, long capacity) {
  __shared__ int s_pre[kVoxelMergeMaps + 1];
  __shared__ long long s_w[kSortWaves][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = sv_play(v);
  int R = v.plan[kSvRuns]; R = R < 0 ? 0 : (R > n ? n : R);
  int valid = n - v.plan[kSvOutsideN]; valid = valid < 0 ? 0 : (valid > n ? n : valid);   // the sorted positions that hold a cell
  vm_prefix_from_plan(v, n, s_pre);
  const int* __restrict__ start = reinterpret_cast<const int*>(v.key[kSvSorted ^ 1]);
  const int* __restrict__ voxel = start + v.cap;
  const unsigned long long* __restrict__ sorted = v.key[kSvSorted];
  const unsigned* __restrict__ src = v.val[kSvSorted];
  const int short_max = m.short_max < 0 ? 0 : (m.short_max > 64 ? 64 : m.short_max);
  for (long base = (long)blockIdx.x * kSortBlock; base < R; base += (long)gridDim.x * kSortBlock) {   // (uniform over the workgroup)
    const long r = base + tid;
    int s = 0, e = 0, at = 0;
    if (r < R) {
      s = start[r]; e = r + 1 < R ? start[r + 1] : valid;
      s = s < 0 ? 0 : s; e = e > valid ? valid : e;
      at = voxel[r];
      if (at < 0 || at >= capacity) e = s;   // (a sparse run, or no room: nothing to do)
    }
    const int len = e - s;
    if (len > 0 && len <= short_max) {   // the thread's own run
      long long W = 0;
      for (int p = s; p < e; p++) {
        float4 q;
        if (vm_input(m, s_pre, src[p], n, &q)) W += __float_as_int(q.w);
      }
      keys[at] = sorted[s]; counts[at] = vm_stored(W);
    }
    unsigned long long longs = __ballot(len > short_max);
    while (longs) {   // the wave's long runs, one after another (uniform over the wave)
      const int l = __ffsll(longs) - 1;
      longs &= longs - 1;
      const int sl = __shfl(s, l), el = __shfl(e, l), atl = __shfl(at, l);
      long long w = 0;
      for (long p = (long)sl + lane; p < el; p += 64) {
        float4 q;
        if (vm_input(m, s_pre, src[p], n, &q)) w += __float_as_int(q.w);
      }
      s_w[wave][lane] = w;
      MOT_WAVE_SYNC();
      if (lane == 0) {
        long long W = 0;
        for (int k = 0; k < 64; k++) W += s_w[wave][k];
        keys[atl] = sorted[sl]; counts[atl] = vm_stored(W);
      }
      MOT_WAVE_SYNC();   // (s_w is read: the next round may write it)
    }
  }
}

// ------------------------------------------------------------------------------------------ host
static unsigned vm_blocks(int cap) {
  const long blocks = ((long)cap + kSortBlock - 1) / kSortBlock;
  return (unsigned)(blocks < 1 ? 1 : (blocks > kVmBlocks ? kVmBlocks : blocks));
}
void mot_launch_voxel_merge_count(const VoxelMergeMaps& m, const SceneVoxelBuffers& v, const SceneVoxelArgs& a, long out_capacity, mot_voxel_merge_header* header, hipStream_t stream) {
  hipLaunchKernelGGL(voxel_merge_key_kernel, dim3(vm_blocks(v.cap)), dim3(kSortBlock), 0, stream, m, v, a);
  SortBuffers s;
  s.key[0] = v.key[0]; s.key[1] = v.key[1]; s.val[0] = v.val[0]; s.val[1] = v.val[1]; s.table = v.table; s.totals = v.totals; s.n = v.plan + kSvPlay; s.cap = v.cap;
  (void)mot_sort_launch(s, kSceneVoxelKeyBits, stream);
  hipLaunchKernelGGL(voxel_merge_heads_kernel, dim3(v.tiles), dim3(kSortBlock), 0, stream, v);
  hipLaunchKernelGGL(voxel_merge_scan_kernel, dim3(1), dim3(kSortBlock), 0, stream, v, 0, out_capacity, header);
  hipLaunchKernelGGL(voxel_merge_runs_kernel, dim3(v.tiles), dim3(kSortBlock), 0, stream, v);
  hipLaunchKernelGGL(voxel_merge_reduce_kernel, dim3(vm_blocks(v.cap)), dim3(kSortBlock), 0, stream, m, v, a.min_points, 0, (mot_model_voxel*)nullptr, 0L);
  hipLaunchKernelGGL(voxel_merge_kept_kernel, dim3(v.tiles), dim3(kSortBlock), 0, stream, v, 0);
  hipLaunchKernelGGL(voxel_merge_scan_kernel, dim3(1), dim3(kSortBlock), 0, stream, v, 1, out_capacity, header);
  hipLaunchKernelGGL(voxel_merge_kept_kernel, dim3(v.tiles), dim3(kSortBlock), 0, stream, v, 1);
}
void mot_launch_voxel_merge_write(const VoxelMergeMaps& m, const SceneVoxelBuffers& v, int min_points, mot_model_voxel* out, long out_capacity, hipStream_t stream) {
  if (!out || out_capacity <= 0) return;
  hipLaunchKernelGGL(voxel_merge_reduce_kernel, dim3(vm_blocks(v.cap)), dim3(kSortBlock), 0, stream, m, v, min_points, 1, out, out_capacity);
}
void mot_launch_voxel_merge_index(const VoxelMergeMaps& m, const SceneVoxelBuffers& v, unsigned long long* keys, int* counts, long capacity, hipStream_t stream) {
  if (!keys || !counts || capacity <= 0) return;
  hipLaunchKernelGGL(voxel_merge_index_kernel, dim3(vm_blocks(v.cap)), dim3(kSortBlock), 0, stream, m, v, keys, counts, capacity);
}
