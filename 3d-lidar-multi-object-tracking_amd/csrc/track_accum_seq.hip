// track_accum_seq.hip — the per-track accumulators (track_accum.hip) fed by SEQUENCE MODE, on gfx950. Product code (HIP, wave64).
//
// mot_sequence_accumulate_dev: the frames of one recorded drive go through the tracker chained on the device (slot k = frame k, the track state in stream 0),
// and all of them are appended to stream 0's accumulators in the same call. What track_accum_plan_kernel reads for ONE frame right after its step — the id ->
// slot map and the mot_track records — is gone a step later, so it is captured inside the chain; the rest runs once, behind the last step, over all frames.
//
//   S0  track_accum_capture_kernel       one launch per step, right behind it: for every box of the step's owner row the slot of the owning id (slot_of) and
//                                        that slot's mot_track fields of mot_accum_obs, as the step left them -> cap[frame][box]
//   P0, P1  track_points.hip's table and count kernels over all frames (mot_launch_track_point_counts), as they are
//   S1  track_accum_seq_segments_kernel  one workgroup per frame, one thread per segment: the chunks' counts of the segment turned into the rank of each chunk's
//                                        first point within the segment, the segment's points, a box that carries its id and through it the captured slot
//   S2  track_accum_seq_plan_kernel      ONE workgroup walks the frames in order, one thread per segment: the row rule of track_accum_plan_kernel (restart when
//                                        the row holds another id, total, obs_total, first_step / last_step) on stream 0's rows; keeps per (frame, segment) the
//                                        sequence numbers t0 / u of its first point / its observation within the track's incarnation. A workgroup barrier
//                                        between frames hands the rows of frame k to frame k + 1 (one workgroup = one CU: the barrier's release / acquire at
//                                        workgroup scope is all a hand-off inside a workgroup needs)
//   S3  track_accum_seq_finish_kernel    one workgroup per frame, against the FINAL rows: a segment contributes only if its id is the row's final id; its
//                                        observation u is logged when u >= obs_total - O; lo = the first point of the segment that is still among the row's last K
//   S4  track_accum_seq_scatter_kernel   1024-point chunks of all frames: tp_place_chunk with a ring sink — point j of a segment goes to ring[(t0 + j) & (K - 1)]
//                                        of stream 0's row for j >= lo, with frame k's matrix and stamp
//
// The hazard the one-frame code does not have: frames of one call meet in a ring (many frames bring more than K points of a track between them; a slot goes to
// a new track in the middle of the call). S3's rule makes every ring and log position the target of at most one record of the call: ids are never reused within
// a stream, so the segments of a row's final id are one incarnation, its points carry the distinct numbers t0 + j, and only the last K of them (the last O
// observations) are written — K (O) consecutive numbers, distinct modulo K (O). This is track_accum_plan_kernel's skip = max(0, n - K) over several frames, and
// the kept part of the rings is what appending frame by frame leaves; positions outside a row's kept range are undefined, as after a restart. Nothing depends on
// the order in which workgroups run, no atomics: distinct ids of a stream have distinct slots.
// Every index is checked or masked where it is used: an id outside [0, E) or a slot outside [0, T) drops the segment in S0 / S1, S3 and S4 test the row again,
// ring and log positions are masked.
// Bytes: per box and step 4 (owner) + 4 (slot_of) + 144 (mot_track) read, 40 written; per segment 32 (row) read and written twice, 32 (plan) written, 40 + 48 for
// the observation; per owned point 36 as in track_accum.hip.
// Resources (tools/kernel_resources.py, gfx950): S0 22 VGPRs, no LDS; S1 18 VGPRs, 4 096 bytes of LDS; S2 26 VGPRs, no LDS; S3 32 VGPRs, no LDS; S4 46 VGPRs,
// 16 464 bytes of LDS (the arrays of track_points.hip's P3, as track_accum_scatter_kernel). 8 waves per SIMD each, no scratch memory.
#include "mot_track_place.h"

static_assert(sizeof(TrackAccumCapture) == 40 && sizeof(TrackAccumSeqSeg) == 32, "mot_internal.h documents the sizes");

// ------------------------------------------------------------------------------------------ S0
__global__ void MOT_TP_BOUNDS(kTpBlock)
track_accum_capture_kernel(const int* __restrict__ counts, const int* __restrict__ owner, TrackAccumBuffers a, TrackAccumCapture* __restrict__ cap, int k) {
  const int M = mot_owner_boxes(counts, k);
  for (int i = threadIdx.x; i < M; i += kTpBlock) {
    const int id = owner[(long)k * kMaxBoxesPerFrame + i];
    const int r = (id >= 0 && id < a.E) ? a.slot_of[id] : -1;   // (stream 0's map and records)
    TrackAccumCapture e;
    e.slot = -1; e.track_manage = 0; e.is_static = 0; e.lifetime = 0; e.px = 0.f; e.py = 0.f; e.v = 0.0; e.yaw = 0.0;
    if (r >= 0 && r < a.T) {
      const mot_track* __restrict__ tr = a.out + r;
      e.slot = r; e.track_manage = tr->track_manage; e.is_static = tr->is_static; e.lifetime = tr->lifetime;
      e.px = tr->px; e.py = tr->py; e.v = tr->v; e.yaw = tr->yaw;
    }
    cap[(long)k * kMaxBoxesPerFrame + i] = e;
  }
}

// ------------------------------------------------------------------------------------------ S1
__global__ void MOT_TP_BOUNDS(kTpBlock)
track_accum_seq_segments_kernel(TrackPointBuffers t, TrackAccumSeqBuffers s, int T) {
  __shared__ int s_own[kMaxBoxesPerFrame];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int M = mot_owner_boxes(t.counts, b);
  for (int i = tid; i < M; i += kTpBlock) s_own[i] = t.owner[(long)b * kMaxBoxesPerFrame + i];
  __syncthreads();
  const int chunks = tp_chunks(t, b);
  const int R = tp_segments(t, b);
  int* __restrict__ rows = t.rows + (long)b * t.max_chunks * kTrackPointKeys;
  for (int key = tid; key < R; key += kTpBlock) {
    int run = 0;
    for (int ch = 0; ch < chunks; ch++) {
      const int v = rows[(long)ch * kTrackPointKeys + key];
      rows[(long)ch * kTrackPointKeys + key] = run;
      run += v;
    }
    const int id = t.seg_id[(long)b * kMaxBoxesPerFrame + key];
    int box = -1;
    for (int i = 0; i < M && box < 0; i++) box = s_own[i] == id ? i : -1;   // (the table kernel took the id from this row)
    int r = box >= 0 ? s.cap[(long)b * kMaxBoxesPerFrame + box].slot : -1;
    if (r < 0 || r >= T) r = -1;
    TrackAccumSeqSeg g;
    g.id = id; g.row = r; g.count = run; g.box = box; g.t0 = 0; g.u = 0; g.lo = 0x7fffffff;
    s.seg[(long)b * kMaxBoxesPerFrame + key] = g;
  }
}

// ------------------------------------------------------------------------------------------ S2
__global__ void MOT_TP_BOUNDS(kTpBlock)
track_accum_seq_plan_kernel(TrackPointBuffers t, TrackAccumBuffers a, TrackAccumSeqBuffers s, int frames) {
  const int tid = threadIdx.x;
  for (int k = 0; k < frames; k++) {
    const int R = tp_segments(t, k), step = s.step0 + k;
    for (int key = tid; key < R; key += kTpBlock) {   // (distinct ids of a frame have distinct rows: a thread owns its row for the frame)
      TrackAccumSeqSeg* __restrict__ g = s.seg + (long)k * kMaxBoxesPerFrame + key;
      const int r = g->row;
      if (r < 0 || r >= a.T) continue;
      mot_accum_row row = a.rows[r];
      if (row.track_id != g->id) { row.track_id = g->id; row.first_step = step; row.obs_total = 0; row.total = 0; }   // the slot went to another track
      g->t0 = row.total; g->u = row.obs_total;
      if (a.O > 0) row.obs_total++;
      row.total += (unsigned long long)g->count;
      row.last_step = step;
      row.reserved = 0;
      a.rows[r] = row;
    }
    __syncthreads();   // frame k's rows, before any thread reads them for frame k + 1
  }
}

// ------------------------------------------------------------------------------------------ S3
__global__ void MOT_TP_BOUNDS(kTpBlock)
track_accum_seq_finish_kernel(TrackPointBuffers t, TrackAccumBuffers a, TrackAccumSeqBuffers s) {
  const int b = blockIdx.x, step = s.step0 + b;
  const int R = tp_segments(t, b);
  for (int key = threadIdx.x; key < R; key += kTpBlock) {
    TrackAccumSeqSeg* __restrict__ g = s.seg + (long)b * kMaxBoxesPerFrame + key;
    const int r = g->row, box = g->box;
    if (r < 0 || r >= a.T || box < 0 || box >= kMaxBoxesPerFrame) continue;   // (lo stays "none")
    const mot_accum_row row = a.rows[r];
    if (row.track_id != g->id) continue;   // the slot went to another track later in the call: this one's points are gone
    const unsigned long long t0 = g->t0, first = row.total > (unsigned long long)a.K ? row.total - (unsigned long long)a.K : 0ull;
    g->lo = first > t0 ? (first - t0 < 0x7fffffffull ? (int)(first - t0) : 0x7fffffff) : 0;
    if (a.O > 0 && (long)g->u >= (long)row.obs_total - (long)a.O) {
      const TrackAccumCapture e = s.cap[(long)b * kMaxBoxesPerFrame + box];
      mot_accum_obs o;
      o.step = step; o.count = g->count; o.n_boxes = t.seg_boxes[(long)b * kMaxBoxesPerFrame + key]; o.track_manage = e.track_manage;
      o.px = e.px; o.py = e.py; o.is_static = e.is_static; o.lifetime = e.lifetime;
      o.v = e.v; o.yaw = e.yaw;
      a.obs[(long)r * a.O + (g->u & (a.O - 1))] = o;
    }
  }
}

// ------------------------------------------------------------------------------------------ S4
struct TaSeqRingSink {
  const TrackAccumSeqSeg* __restrict__ seg;   // the frame's
  mot_accum_point* __restrict__ rings;        // stream 0's [T][K]
  int T, K, step;
  __device__ __forceinline__ bool takes(int key, long p) const { return p >= (long)seg[key].lo; }   // (key < R <= kMaxBoxesPerFrame: no rest segment here)
  __device__ __forceinline__ void put(int key, long p, float4 o, long) const {
    const int r = seg[key].row;
    if (r < 0 || r >= T) return;
    o.w = __int_as_float(step);
    *reinterpret_cast<float4*>(rings + (long)r * K + (long)((seg[key].t0 + (unsigned long long)p) & (unsigned long long)(K - 1))) = o;
  }
};
__global__ void MOT_TP_BOUNDS(kTpBlock)
track_accum_seq_scatter_kernel(TrackPointBuffers t, TrackAccumBuffers a, TrackAccumSeqBuffers s, const EgoTf* __restrict__ tf) {
  MOT_TP_PLACE_LDS(l);
  const int b = blockIdx.y;
  const TaSeqRingSink sink = {s.seg + (long)b * kMaxBoxesPerFrame, a.points, a.T, a.K, s.step0 + b};
  tp_place_chunk(t, b, b, 0, tf, l, sink);
}

// ------------------------------------------------------------------------------------------ host
void mot_launch_track_accum_capture(const int* counts, const int* owner, const TrackAccumBuffers& a, TrackAccumCapture* cap, int frame, hipStream_t stream) {
  hipLaunchKernelGGL(track_accum_capture_kernel, dim3(1), dim3(kTpBlock), 0, stream, counts, owner, a, cap, frame);
}
void mot_launch_track_accum_sequence(const TrackPointBuffers& t, const TrackAccumBuffers& a, const TrackAccumSeqBuffers& s, int frames, int max_n, const EgoTf* tf,
                                     hipStream_t stream) {
  const int chunks = mot_launch_chunks(max_n, kTrackPointChunk, t.max_chunks);
  mot_launch_track_point_counts(t, 0, frames, max_n, stream);
  hipLaunchKernelGGL(track_accum_seq_segments_kernel, dim3(frames), dim3(kTpBlock), 0, stream, t, s, a.T);
  hipLaunchKernelGGL(track_accum_seq_plan_kernel, dim3(1), dim3(kTpBlock), 0, stream, t, a, s, frames);
  hipLaunchKernelGGL(track_accum_seq_finish_kernel, dim3(frames), dim3(kTpBlock), 0, stream, t, a, s);
  hipLaunchKernelGGL(track_accum_seq_scatter_kernel, dim3(chunks, frames), dim3(kTpBlock), 0, stream, t, a, s, tf);
}
