// scene_judge_seq.hip — a recorded drive's points judged against the grid the drive left, on gfx950. Product code (HIP, wave64).
//
// scene_judge.hip judges the live frame of every slot against that slot's grid; the kernels here judge ALL frames of the latest mot_sequence_products_dev(MOT_SEQ_SCENE)
// call (slot k = frame k of stream 0) against slot 0's grid AS IT STANDS, i.e. with hindsight, and pack the records class-major over the whole drive into ONE block of
// the caller's: the KNOWN points of all frames are one contiguous run — the static map (include/mot.h, "a drive's points judged against its grid"). The grid is only READ.
//
//   S1  scene_judge_seq_classify_kernel  grid (ceil(N_e / 2048), frames), chunk index fastest, 256 threads, 8 points a thread — scene_judge_classify_kernel's geometry, and
//                                        its body: sj_classify_body (mot_scene_judge.h). The kernel hands in what differs: the kind of an owned point is ONE 4-byte gather
//                                        from frame k's row of the captured bit table (SceneKindRecorded: flagged static as step k left it), the matrix and the class
//                                        block are frame k's, and the window, its validity and the cells (ONE 8-byte gather of the two counters) are slot 0's
//   S2  scene_judge_seq_scan_kernel      one workgroup per frame: per class the exclusive scan over the frame's chunks (sj_scan_chunks, scene_judge_scan_kernel's) and the
//                                        frame's five totals
//   S3  scene_judge_seq_bases_kernel     ONE workgroup: per class a scan over the frames, 256 frames a round (block_scan_excl_i32), the carry in a register; classes ascending, so
//                                        the start of a class's run is known when its turn comes. Every (frame, class) gets its drive-wide base; both tables are written
//   S4  scene_judge_seq_scatter_kernel   the grid of S1, sj_scatter_body<true>: class byte in, rank inside the 64-point tile by ballots, the chunk's 32 tiles chained through the
//                                        32 x 5 LDS table from (drive-wide base + the chunk's place inside the frame), one 16-byte store per selected record below the capacity
//
// Four launches whatever `frames` is (three for the counts alone). No global atomics, no workgroup waits on another, every count and place is a sum of integers over a
// fixed set: the output does not depend on the order in which workgroups or waves run.
// INDEX SAFETY. Point, id and class loads stay below min(count, cap) of the frame's slot; the storage index is masked (scene_point_cell); an id outside
// [0, E) is not looked up (dynamic); chunk rows are indexed below the chunk capacity; every per-frame table ([frames][5] totals, the matrices, the bit rows) is indexed
// below frames <= max_batch; a record is stored only below the caller's capacity, a class byte only below class_stride. Places are int32: the host refuses
// frames * max_points beyond 2^31 - 1.
// Resources (tools/kernel_resources.py): profiles/scene_judge_sequence.md.
#include "mot_scene_judge.h"

// ------------------------------------------------------------------------------------------ S1
__global__ void MOT_SG_BOUNDS(kSceneBlock)
scene_judge_seq_classify_kernel(SceneGridBuffers g, SceneSplatInput in, SceneJudgeBuffers j, SceneSeqBuffers s, const EgoTf* __restrict__ tf, uint8_t* __restrict__ classes,
                                long class_stride) {
  __shared__ int s_cnt[kSjWaves][MOT_SCENE_CLASSES];
  const int k = blockIdx.y;   // frame k lives in slot k; grid, header and validity are slot 0's
  sj_classify_body(g, in, j, 0, k, tf + k, SceneKindRecorded(in, s, k), classes ? classes + (long)k * class_stride : nullptr, class_stride, s_cnt);
}

// ------------------------------------------------------------------------------------------ S2
// rows[chunk][5 + c]: the class's points in the frame's earlier chunks; totals[k][c]: the frame's points of class c (S3 turns it into the drive-wide base in place)
__global__ void MOT_SG_BOUNDS(kSceneBlock)
scene_judge_seq_scan_kernel(SceneSplatInput in, SceneJudgeBuffers j, int* __restrict__ totals) {
  __shared__ int s_part[kSjWaves];
  __shared__ int s_total[MOT_SCENE_CLASSES];
  const int k = blockIdx.x, tid = threadIdx.x;
  sj_scan_chunks(j.rows + (long)k * j.max_chunks * kSceneJudgeRow, sj_chunks(in, j, k), s_part, s_total, tid);
  __syncthreads();
  if (tid < MOT_SCENE_CLASSES) totals[k * MOT_SCENE_CLASSES + tid] = s_total[tid];
}

// ------------------------------------------------------------------------------------------ S3
// bases[k][c]: in the frame's count, out where frame k's first record of class c goes in the drive's block — the runs of the selected classes below c, then the class's
// points of earlier frames (for a class outside the mask the place inside an imaginary run from 0: nobody reads it). Frames tid, tid + 256, ... per thread
__global__ void MOT_SG_BOUNDS(kSceneBlock)
scene_judge_seq_bases_kernel(SceneJudgeBuffers j, int* __restrict__ bases, int frames, mot_scene_segment* __restrict__ segments, mot_scene_segment* __restrict__ totals) {
  __shared__ int s_part[kSjWaves];
  const int tid = threadIdx.x;
  int run = 0;   // the records of the selected classes below c
  for (int c = 0; c < MOT_SCENE_CLASSES; c++) {
    const bool picked = (j.class_mask >> c) & 1;
    const int start = picked ? run : 0;
    int carry = 0;   // the class's points in the frames of earlier rounds
    for (int k0 = 0; k0 < frames; k0 += kSceneBlock) {   // (uniform)
      const int k = k0 + tid;
      const int v = k < frames ? bases[k * MOT_SCENE_CLASSES + c] : 0;
      int total;
      const int first = start + carry + block_scan_excl_i32<kSjWaves>(v, s_part, total);
      carry += total;
      __syncthreads();   // (s_part is written again in the next round)
      if (k < frames) {
        bases[k * MOT_SCENE_CLASSES + c] = first;
        int* o = reinterpret_cast<int*>(segments + (long)k * MOT_SCENE_CLASSES + c);
        o[0] = picked ? first : -1; o[1] = v;
      }
    }
    if (tid == 0) {
      int* o = reinterpret_cast<int*>(totals + c);
      o[0] = picked ? start : -1; o[1] = carry;
    }
    if (picked) run += carry;
  }
}

// ------------------------------------------------------------------------------------------ S4
__global__ void MOT_SG_BOUNDS(kSceneBlock)
scene_judge_seq_scatter_kernel(SceneSplatInput in, SceneJudgeBuffers j, const int* __restrict__ bases, const EgoTf* __restrict__ tf, mot_track_point* __restrict__ out,
                               long capacity) {
  __shared__ int s_cnt[kSjTiles][MOT_SCENE_CLASSES];   // points of (tile, class)
  __shared__ int s_at[kSjTiles][MOT_SCENE_CLASSES];    // where the tile's first record of the class goes
  const int k = blockIdx.y;
  sj_scatter_body<true>(in, j, k, bases + k * MOT_SCENE_CLASSES, tf ? tf + k : nullptr, out, capacity, s_cnt, s_at);
}

// ------------------------------------------------------------------------------------------ host
void mot_launch_scene_judge_seq_count(const SceneGridBuffers& g, const SceneSplatInput& in, const SceneJudgeBuffers& j, const SceneSeqBuffers& s, int* bases, int frames, int max_n,
                                      const EgoTf* tf, mot_scene_segment* segments, mot_scene_segment* totals, uint8_t* classes, long class_stride, hipStream_t stream) {
  hipLaunchKernelGGL(scene_judge_seq_classify_kernel, dim3(mot_launch_chunks(max_n, kSceneChunk, j.max_chunks), frames), dim3(kSceneBlock), 0, stream, g, in, j, s, tf, classes, class_stride);
  hipLaunchKernelGGL(scene_judge_seq_scan_kernel, dim3(frames), dim3(kSceneBlock), 0, stream, in, j, bases);
  hipLaunchKernelGGL(scene_judge_seq_bases_kernel, dim3(1), dim3(kSceneBlock), 0, stream, j, bases, frames, segments, totals);
}
void mot_launch_scene_judge_seq_scatter(const SceneSplatInput& in, const SceneJudgeBuffers& j, const int* bases, int frames, int max_n, const EgoTf* tf, int global,
                                        mot_track_point* points, long capacity, hipStream_t stream) {
  if (!j.class_mask || !points || capacity <= 0) return;
  hipLaunchKernelGGL(scene_judge_seq_scatter_kernel, dim3(mot_launch_chunks(max_n, kSceneChunk, j.max_chunks), frames), dim3(kSceneBlock), 0, stream, in, j, bases, global ? tf : nullptr, points, capacity);
}
