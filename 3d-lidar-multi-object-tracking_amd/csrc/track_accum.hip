// track_accum.hip — every track's points accumulated over frames, on gfx950. Product code (HIP, wave64).
//
// track_points.hip partitions ONE frame's elevated points by owning track. Here the segments of a step are appended to device-resident accumulators instead: per
// TRACK SLOT of a stream (the tracker's bounded set of objects alive at once: TrackBuffers::slot_of maps an id to its slot, a slot freed by a dead track is handed
// to the next birth) one row {track_id, first_step, last_step, obs_total, total}, a ring of K points {x, y, z, step} in the tracker's global frame, and a ring of O
// observations — the track's mot_track record as the contributing step left it. The reference has no such output.
//
//   P0, P1  track_points.hip's table and count kernels, as they are (mot_launch_track_point_counts): the distinct owners and each chunk's points per key
//   A2  track_accum_plan_kernel     one workgroup per frame, one thread per segment: id -> row (slot_of), the row reset when it held another id, then
//                                   plan[segment] = {row, ring position of the first kept point}, the row's new totals, the observation; and each chunk's count of
//                                   the segment turned into (rank of the chunk's first point within the segment) - skip, skip = max(0, n - K): a frame that brings
//                                   more than K points of a track keeps the last K
//   A3  track_accum_scatter_kernel  1024-point chunks: tp_place_chunk (mot_track_place.h — P3's in-order placement) with the ring as the sink: place p >= 0 goes to
//                                   ring[(at + p) & (K - 1)] in one 16-byte store, p < 0 is a skipped point
//   --  track_accum_clear_kernel    rows back to empty (the setter, the resets, mot_stream_load); not part of an accumulate call
//
// Distinct ids of one stream have distinct slots, so one thread per segment owns its row: no atomics. Nothing depends on the order in which workgroups or waves
// run. Every index is checked or masked where it is used: an id outside [0, E) or a slot outside [0, T) drops the segment in A2, A3 tests the row again and masks
// the ring position, so garbage in an id row or the slot map cannot produce an address outside the three tables.
// Bytes per owned point: P1 4 read (id); A3 4 (id) + 12 (point) read, 16 written — the export's 36, nothing staged; per segment 32 (row) read and written, 48
// (observation) + 8 (plan) written, 144 (mot_track) read; per (chunk, segment) 3 x 4 as in the export.
// Resources (tools/kernel_resources.py): A3 16 464 bytes of LDS a workgroup — the very arrays of P3 — and 8 waves per SIMD, as P3; A2 no LDS, 8 waves per SIMD.
#include "mot_track_place.h"

static_assert(sizeof(mot_accum_row) == 32 && sizeof(mot_accum_point) == 16 && sizeof(mot_accum_obs) == 48 && sizeof(TrackAccumPlan) == 8, "include/mot.h documents the sizes");

// ------------------------------------------------------------------------------------------ A2
__global__ void MOT_TP_BOUNDS(kTpBlock)
track_accum_plan_kernel(TrackPointBuffers t, TrackAccumBuffers a, int b0) {
  const int kb = blockIdx.x, b = b0 + kb, tid = threadIdx.x;
  const int chunks = tp_chunks(t, b);
  const int R = tp_segments(t, b);
  const int step = a.steps[kb];
  int* __restrict__ rows = t.rows + (long)b * t.max_chunks * kTrackPointKeys;
  for (int key = tid; key < R; key += kTpBlock) {   // (consecutive threads read consecutive words of a chunk's row)
    int sum = 0;
    for (int ch = 0; ch < chunks; ch++) sum += rows[(long)ch * kTrackPointKeys + key];
    const int skip = sum > a.K ? sum - a.K : 0;
    int run = -skip;
    for (int ch = 0; ch < chunks; ch++) {
      const int v = rows[(long)ch * kTrackPointKeys + key];
      rows[(long)ch * kTrackPointKeys + key] = run;
      run += v;
    }
    const int id = t.seg_id[(long)b * kMaxBoxesPerFrame + key];
    const int r = (id >= 0 && id < a.E) ? a.slot_of[(long)b * a.E + id] : -1;
    TrackAccumPlan pl = {-1, 0};
    if (r >= 0 && r < a.T) {   // (the tracker's invariant: the owner of a box of this step still has its slot)
      const long at = (long)b * a.T + r;
      mot_accum_row row = a.rows[at];
      if (row.track_id != id) { row.track_id = id; row.first_step = step; row.obs_total = 0; row.total = 0; }   // the slot went to another track: its points go
      pl.row = r;
      pl.at = (int)((row.total + (unsigned long long)skip) & (unsigned long long)(a.K - 1));
      if (a.O > 0) {
        const mot_track* __restrict__ tr = a.out + at;
        mot_accum_obs o;
        o.step = step; o.count = sum; o.n_boxes = t.seg_boxes[(long)b * kMaxBoxesPerFrame + key]; o.track_manage = tr->track_manage;
        o.px = tr->px; o.py = tr->py; o.is_static = tr->is_static; o.lifetime = tr->lifetime;
        o.v = tr->v; o.yaw = tr->yaw;
        a.obs[at * a.O + (row.obs_total & (a.O - 1))] = o;
        row.obs_total++;
      }
      row.total += (unsigned long long)sum;
      row.last_step = step;
      row.reserved = 0;
      a.rows[at] = row;
    }
    a.plan[(long)b * kMaxBoxesPerFrame + key] = pl;
  }
}

// ------------------------------------------------------------------------------------------ A3
struct TaRingSink {
  const TrackAccumPlan* __restrict__ plan;   // the frame's
  mot_accum_point* __restrict__ rings;       // the frame's [T][K]
  int T, K, step;
  __device__ __forceinline__ bool takes(int, long p) const { return p >= 0; }
  __device__ __forceinline__ void put(int key, long p, float4 o, long) const {
    const TrackAccumPlan pl = plan[key];   // (key < R <= kMaxBoxesPerFrame: tp_place_chunk hands no other key over without the rest flag)
    if (pl.row < 0 || pl.row >= T) return;
    o.w = __int_as_float(step);
    *reinterpret_cast<float4*>(rings + (long)pl.row * K + ((pl.at + p) & (long)(K - 1))) = o;
  }
};
__global__ void MOT_TP_BOUNDS(kTpBlock)
track_accum_scatter_kernel(TrackPointBuffers t, TrackAccumBuffers a, int b0, const EgoTf* __restrict__ tf) {
  MOT_TP_PLACE_LDS(s);
  const int kb = blockIdx.y, b = b0 + kb;
  const TaRingSink sink = {a.plan + (long)b * kMaxBoxesPerFrame, a.points + (long)b * a.T * a.K, a.T, a.K, a.steps[kb]};
  tp_place_chunk(t, b, kb, 0, tf, s, sink);
}

// ------------------------------------------------------------------------------------------ rows back to empty
__global__ void MOT_TP_BOUNDS(kTpBlock)
track_accum_clear_kernel(mot_accum_row* __restrict__ rows, long first, long n) {
  const long i = (long)blockIdx.x * kTpBlock + threadIdx.x;
  if (i >= n) return;
  mot_accum_row e;
  e.track_id = -1; e.first_step = 0; e.last_step = 0; e.obs_total = 0; e.total = 0; e.reserved = 0;
  rows[first + i] = e;
}

// ------------------------------------------------------------------------------------------ host
void mot_launch_track_accum(const TrackPointBuffers& t, const TrackAccumBuffers& a, int first, int batch, int max_n, const EgoTf* tf, hipStream_t stream) {
  const int chunks = mot_launch_chunks(max_n, kTrackPointChunk, t.max_chunks);
  mot_launch_track_point_counts(t, first, batch, max_n, stream);
  hipLaunchKernelGGL(track_accum_plan_kernel, dim3(batch), dim3(kTpBlock), 0, stream, t, a, first);
  hipLaunchKernelGGL(track_accum_scatter_kernel, dim3(chunks, batch), dim3(kTpBlock), 0, stream, t, a, first, tf);
}
void mot_launch_track_accum_clear(mot_accum_row* rows, long first, long n, hipStream_t stream) {
  if (n <= 0) return;
  hipLaunchKernelGGL(track_accum_clear_kernel, dim3((unsigned)((n + kTpBlock - 1) / kTpBlock)), dim3(kTpBlock), 0, stream, rows, first, n);
}
