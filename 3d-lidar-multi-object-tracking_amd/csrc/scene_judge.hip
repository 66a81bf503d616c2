// scene_judge.hip — a frame's points judged against the rolling static-scene grid, on gfx950. Product code (HIP, wave64).
//
// scene_grid.hip fills the grid; the kernels here ask it a question about the live frame (include/mot.h, "a frame's points judged against the scene grid"): every
// elevated point of a fused step gets one of five classes — UNKNOWN, MOVING, TRAIL, NEW, KNOWN — and the points are partitioned by class, in input order, into the
// caller's block. The grid is only READ. The reference has no such output (scene_grid.hip's header).
//
//   J1  scene_judge_classify_kernel  grid (ceil(N_e / 2048), B), 256 threads, 8 points a thread — the geometry of scene_splat_kernel. The kernel names slot b, its own
//                                    grid, the live kind rule (SceneKindLive) and block kb of the caller's; the rest is sj_classify_body. Per point the 12-byte point (16 in
//                                    the float4 layout), the 4-byte id, for an owned point the two dependent gathers id -> track slot -> is_static, the transform
//                                    and cell test of scene_point_cell (mot_scene_splat.h: the cell is bit for bit the one the point would be counted in) and ONE
//                                    8-byte load of the cell's {static_hits, dynamic_hits}; neighbouring lanes mostly share a cell, so the loads coalesce by
//                                    themselves. The 64-bit trail test, then the class as one byte to the library's scratch (and to the caller's class block), and
//                                    the chunk's five counts — wave ballots on the three class bits, merged through LDS — as plain stores to the chunk's row
//   J2  scene_judge_scan_kernel      one workgroup per slot: per class an exclusive scan of the chunks' counts (block_scan_excl_i32 of mot_wave.h), the mask applied,
//                                    the segment table, and where every chunk's first record of every class goes
//   J3  scene_judge_scatter_kernel   the grid of J1, sj_scatter_body<false>: class byte in, rank inside the 64-point tile by ballots on the class bits, the 32 tiles of a chunk chained
//                                    through a small LDS table (five serial scans of 32 entries), the point and the global transform on request, one 16-byte store
//                                    per selected record below the caller's stride. Only the points of selected classes are loaded
//
// The cell of a point is gathered ONCE per call (J3 reads J1's byte). No global atomics, no workgroup waits on another, every count and every place is a sum of
// integers over a fixed set: the output does not depend on the order in which workgroups or waves run.
// INDEX SAFETY. Point, id and class loads stay below min(count, cap) of the slot; the storage index is masked (scene_point_cell); an id outside [0, E) or a
// track slot outside [0, T) is not followed (the point then counts as dynamic, as in the splat kernel); chunk rows are indexed below the slot's chunk capacity; a
// record is stored only below min(point_stride, selected records), a class byte only below class_stride.
// Resources (tools/kernel_resources.py): no scratch; LDS 80 bytes (J1), 48 (J2), 1280 (J3); 58 / 16 / 101 VGPRs (profiles/scene_bodies.md: 68 before J1's body was shared). Cost: profiles/scene_judge.md.
// The class rule, the ballots, the scan over chunks, the tile chain, the record store and the BODIES of J1 and J3 live in mot_scene_judge.h: scene_judge_seq.hip (a recorded
// drive judged against slot 0's grid) runs the same text, so that the last frame of a drive gets these kernels' bytes. J1 and J3 here only say what is the live form's own.
#include "mot_scene_judge.h"   // (and, through it, mot_scene_splat.h: the frame's points, the kind rules, the per-point step)

// ------------------------------------------------------------------------------------------ J1
__global__ void MOT_SG_BOUNDS(kSceneBlock)
scene_judge_classify_kernel(SceneGridBuffers g, SceneSplatInput in, SceneJudgeBuffers j, int b0, const EgoTf* __restrict__ tf, uint8_t* __restrict__ classes, long class_stride) {
  __shared__ int s_cnt[kSjWaves][MOT_SCENE_CLASSES];
  const int kb = blockIdx.y, b = b0 + kb;   // slot b against its own grid; block kb of the caller's
  sj_classify_body(g, in, j, b, b, tf + kb, SceneKindLive(in, b), classes ? classes + (long)kb * class_stride : nullptr, class_stride, s_cnt);
}

// ------------------------------------------------------------------------------------------ J2
// rows[chunk][c] (counts) -> rows[chunk][5 + c]: the place of the chunk's first record of class c — the records of the selected classes below c, then the class's
// points of earlier chunks (whatever for a class outside the mask: nobody reads it). Chunks tid, tid + 256, ... per thread; every lane takes part in every scan.
__global__ void MOT_SG_BOUNDS(kSceneBlock)
scene_judge_scan_kernel(SceneSplatInput in, SceneJudgeBuffers j, int b0, mot_scene_segment* __restrict__ segments) {
  __shared__ int s_part[kSjWaves];
  __shared__ int s_total[MOT_SCENE_CLASSES];
  sj_scan_body(in, j, b0 + blockIdx.x, segments + (long)blockIdx.x * MOT_SCENE_CLASSES, s_part, s_total);
}

// ------------------------------------------------------------------------------------------ J3
__global__ void MOT_SG_BOUNDS(kSceneBlock)
scene_judge_scatter_kernel(SceneSplatInput in, SceneJudgeBuffers j, int b0, const EgoTf* __restrict__ tf, mot_track_point* __restrict__ points, long point_stride) {
  __shared__ int s_cnt[kSjTiles][MOT_SCENE_CLASSES];   // points of (tile, class)
  __shared__ int s_at[kSjTiles][MOT_SCENE_CLASSES];    // where the tile's first record of the class goes
  const int kb = blockIdx.y;
  sj_scatter_body<false>(in, j, b0 + kb, nullptr, tf ? tf + kb : nullptr, points + (long)kb * point_stride, point_stride, s_cnt, s_at);
}

// ------------------------------------------------------------------------------------------ host
void mot_launch_scene_judge(const SceneGridBuffers& g, const SceneSplatInput& in, const SceneJudgeBuffers& j, int first, int batch, int max_n, const EgoTf* tf, int global,
                            mot_track_point* points, long point_stride, mot_scene_segment* segments, uint8_t* classes, long class_stride, hipStream_t stream) {
  const dim3 grid(mot_launch_chunks(max_n, kSceneChunk, j.max_chunks), batch);
  hipLaunchKernelGGL(scene_judge_classify_kernel, grid, dim3(kSceneBlock), 0, stream, g, in, j, first, tf, classes, class_stride);
  hipLaunchKernelGGL(scene_judge_scan_kernel, dim3(batch), dim3(kSceneBlock), 0, stream, in, j, first, segments);
  if (j.class_mask && points && point_stride > 0)
    hipLaunchKernelGGL(scene_judge_scatter_kernel, grid, dim3(kSceneBlock), 0, stream, in, j, first, global ? tf : nullptr, points, point_stride);
}
