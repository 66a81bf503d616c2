// mot_voxel_runs.h — what the two users of the global voxel lattice share on the device (HIP, wave64; product code): scene_voxels_seq.hip (a drive's records thinned
// to voxels) and voxel_merge.hip (voxel maps merged into one). THE cell rule (sv_key of mot_voxel_cell.h: include/mot.h, CELL OF A RECORD — one device function, so that a voxel is the
// same piece of the world whichever call made it), the ints of the plan, and the run heads of a sorted key array, counted per tile and turned into the run table.
// Both users lay their scratch out as a SceneVoxelBuffers (mot_internal.h): key[kSvSorted] holds the sorted keys, the other key buffer the run table ([cap] starts,
// then [cap] voxel places), part[0] / part[1] the tiles' run heads and all-ones keys, plan[kSvPlay] the elements in play. The kernels stay with their users.
#ifndef MOT_VOXEL_RUNS_H_
#define MOT_VOXEL_RUNS_H_
#include "mot_internal.h"
#include "mot_sort.h"
#include "mot_voxel_cell.h"   // sv_key, kSvOutside: THE cell rule (shared with the map's reader, map_judge.hip)

constexpr int kSvSorted = ((kSceneVoxelKeyBits + kSortDigitBits - 1) / kSortDigitBits) & 1;   // the buffer mot_sort_launch leaves the result in
enum { kSvRecords = 0, kSvPlay = 1, kSvRuns = 2, kSvOutsideN = 3, kSvVoxels = 4 };   // the plan's ints

__device__ __forceinline__ int sv_play(const SceneVoxelBuffers& v) { return sort_count(v.plan + kSvPlay, v.cap); }

// thread t owns sorted positions base + 8 t .. base + 8 t + 7 of the tile: bit q of the result = position q is a run head; *outs: its all-ones keys
__device__ __forceinline__ unsigned sv_heads(const unsigned long long* __restrict__ key, long base, int n, int tid, int* outs) {
  const long p0 = base + (long)tid * kSortItems;
  unsigned heads = 0;
  *outs = 0;
  unsigned long long prev = (p0 > 0 && p0 < n) ? key[p0 - 1] : 0;
#pragma unroll
  for (int q = 0; q < kSortItems; q++) {
    const long p = p0 + q;
    if (p >= n) break;
    const unsigned long long k = key[p];
    if (k == kSvOutside) ++*outs;
    else if (p == 0 || k != prev) heads |= 1u << q;
    prev = k;
  }
  return heads;
}
// kWrite = false: the tile's run heads and all-ones keys into part[0] / part[1]; true (behind the scan that turned part[0] into the runs of earlier tiles): run r
// starts at start[r]. s_part: kSortWaves * 2 ints
template <bool kWrite>
__device__ __forceinline__ void sv_heads_body(const SceneVoxelBuffers& v, int* s_part) {
  const int tid = threadIdx.x, tile = blockIdx.x;
  const int n = sv_play(v);
  const long base = (long)tile * kSortTile;
  if (base >= n || tile >= v.tiles) return;   // (uniform over the workgroup)
  int outs;
  const unsigned heads = sv_heads(v.key[kSvSorted], base, n, tid, &outs);
  const int cnt[2] = {(int)__popc(heads), outs};
  int before[2], all[2];
  block_scan_excl_i32<kSortWaves, 2>(cnt, s_part, before, all);
  if (!kWrite) {
    if (tid == 0) { v.part[tile] = all[0]; v.part[v.tiles + tile] = all[1]; }
    return;
  }
  int* __restrict__ start = reinterpret_cast<int*>(v.key[kSvSorted ^ 1]);   // the run table: [cap] starts, then [cap] voxel places
  int r = v.part[tile] + before[0];   // (the scan turned the tile's count into the runs of earlier tiles)
  for (unsigned m = heads; m; m &= m - 1) {
    if (r >= 0 && r < n) start[r] = (int)(base + (long)tid * kSortItems + (__ffs(m) - 1));
    r++;
  }
}
#endif  // MOT_VOXEL_RUNS_H_
