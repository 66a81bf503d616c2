// mot_voxel_cell.h — THE cell rule of the global voxel lattice (include/mot.h, CELL OF A RECORD), one device function for everybody who speaks of a cell: the makers
// of a map (scene_voxels_seq.hip, voxel_merge.hip, through mot_voxel_runs.h) and its reader (map_judge.hip) — so that a voxel is the same piece of the world whichever
// call made it and whichever call asks for it. Product code (HIP).
#ifndef MOT_VOXEL_CELL_H_
#define MOT_VOXEL_CELL_H_
#include "mot_internal.h"

constexpr unsigned long long kSvOutside = ~0ull;

// the cell of a record (include/mot.h, CELL OF A RECORD): the all-ones key when it takes no part
__device__ __forceinline__ unsigned long long sv_key(const float4& q, const SceneVoxelArgs& a) {
  const float lim = 3.4028234663852886e38f;
  if (!(fabsf(q.x) <= lim && fabsf(q.y) <= lim && fabsf(q.z) <= lim)) return kSvOutside;   // (NaN fails the compare)
  const float tx = q.x * a.inv_x, ty = q.y * a.inv_y, tz = q.z * a.inv_z;
  if (!(tx >= -1048576.f && tx < 1048576.f && ty >= -1048576.f && ty < 1048576.f && tz >= -2048.f && tz < 2048.f)) return kSvOutside;
  const int ix = (int)floorf(tx), iy = (int)floorf(ty), iz = (int)floorf(tz);
  return ((unsigned long long)(unsigned)(iz + 2048) << 42) | ((unsigned long long)(unsigned)(iy + 1048576) << 21) | (unsigned long long)(unsigned)(ix + 1048576);
}
#endif  // MOT_VOXEL_CELL_H_
