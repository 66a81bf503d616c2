// track_models.hip — object-centred track models from the per-track accumulators, on gfx950. Product code (HIP, wave64).
//
// track_accum.hip keeps, per TRACK SLOT of a stream, a ring of K points in the tracker's global frame and a ring of O observations (the track's pose at every
// contributing step). Here the two are joined on the device: every point that still has its pose in the log is re-centred on the object (and, with
// MOT_MODEL_AXES, turned into the object's axes), the models of a stream are packed back to back into the caller's block, and every model gets its extent.
// The reference has no such output. Both kernels only READ the accumulators.
//
//   M1  track_models_plan_kernel       one workgroup per stream, threads over the T rows (256 at a time, a running base between the rounds): the row, the step of
//                                      the oldest logged observation, a binary search of the unrolled ring for the first point of that step or later (steps never
//                                      decrease along the unrolled ring) -> count; a workgroup exclusive scan (block_scan_excl_i32, mot_wave.h) -> first;
//                                      the 48-byte headers (extent 0) and the stream's two counts
//   M2  track_models_transform_kernel  one workgroup of ONE WAVE per (row, stream) — a model is a few hundred to a few thousand records, and a stream has many: the
//                                      parallelism is across models; rows without a model leave at once. The log, {step, px, py, c, s}, goes to LDS in tiles of 64
//                                      observations, one per lane (c, s: cos / sin of the yaw in double, rounded once to fp32, once per observation); the log ascends
//                                      in step, so a tile covers a contiguous range of the model's records, found by one more binary search of the ring (only logs
//                                      longer than a tile pay it). The records stream through in tiles of 128 (kTrackModelTile): two 16-byte loads in flight per
//                                      lane, a branch-free lower bound over the tile's steps in LDS (neighbouring points share a step: broadcast reads), one
//                                      16-byte store. The extent: every lane keeps min / max of the ORDER-PRESERVING INTEGER IMAGE of its finite records'
//                                      coordinates, then six DPP wave reductions, and lane 0 writes the six floats. Integer min / max: no float atomics, no
//                                      dependence on the order of anything.
//
// x' = x - px, y' = y - py in fp32 (bit-exact); with MOT_MODEL_AXES x' = c*dx + s*dy, y' = c*dy - s*dx, left to right, -ffp-contract=off (build.py), no fast-math
// intrinsic. z and step keep the ring's bits.
// Every index is checked or masked where it is used: ring and log positions are masked with K - 1 / O - 1, row and stream come from the grid, the header M2 reads
// back from the caller's block is clamped to what the row holds (count <= kept, first >= 0), and a record is stored only below point_stride. Garbage in a row, a
// ring or a log cannot produce an address outside the three tables or the caller's point_stride records.
// Bytes per record: 16 read, 16 written (M1 adds ~4 log2 K bytes per row). Per observation 48 read.
// Resources (tools/kernel_resources.py): M1 28 VGPRs, 32 bytes of LDS, 8 waves per SIMD; M2 74 VGPRs, 1 280 bytes of LDS, 6 waves per SIMD — the double-precision
// sincos sets M2's register count, not the streaming loop (held to 8 waves per SIMD it spills 48 bytes a lane: not taken); no scratch in either.
#include "mot_internal.h"
#include "mot_wave.h"
#include "mot_track_model.h"

#ifndef MOT_HIPEMU
#define MOT_TM_BOUNDS(n) __launch_bounds__(n)
#else
#define MOT_TM_BOUNDS(n)
#endif

constexpr int kTmPlanBlock = 256, kTmPlanWaves = kTmPlanBlock / 64;
constexpr int kTmBlock = 64, kTmItems = kTrackModelTile / kTmBlock;   // M2: one wave
static_assert(kTmBlock == 64 && kTrackModelTile % kTmBlock == 0 && kTmObsTile <= kTmBlock, "tile geometry");
static_assert(sizeof(mot_track_model) == 48 && sizeof(mot_accum_point) == 16, "include/mot.h documents the sizes");

// (tm_ring, tm_search, tm_image / tm_float / tm_finite, the log tile and tm_record, the per-record transform: mot_track_model.h, shared with track_voxels.hip)

// ------------------------------------------------------------------------------------------ M1
__global__ void MOT_TM_BOUNDS(kTmPlanBlock)
track_models_plan_kernel(TrackModelBuffers a, int b0, int flags, mot_track_model* __restrict__ models, int* __restrict__ counts) {
  __shared__ int s_tot[kTmPlanWaves * 2];
  const int kb = blockIdx.x, b = b0 + kb, tid = threadIdx.x;
  const bool current = (flags & MOT_MODEL_CURRENT) != 0;
  const int latest = current ? a.latest[b] : 0;
  int base_records = 0, base_models = 0;
  for (int r0 = 0; r0 < a.T; r0 += kTmPlanBlock) {   // (the same rounds for every thread: the scan below is a collective)
    const int r = r0 + tid;
    mot_track_model m;
    m.track_id = -1; m.first = 0; m.count = 0; m.n_obs = 0; m.first_step = 0; m.last_step = 0;
    m.min_x = m.min_y = m.min_z = m.max_x = m.max_y = m.max_z = 0.f;
    if (r < a.T) {
      const long at = (long)b * a.T + r;
      const mot_accum_row row = a.rows[at];
      const TmRing g = tm_ring(row, a.K, a.O);
      if (row.track_id >= 0 && g.n_obs > 0 && (!current || row.last_step == latest)) {
        const int oldest = a.obs[at * a.O + g.obs0].step;
        m.track_id = row.track_id; m.n_obs = g.n_obs; m.first_step = oldest; m.last_step = row.last_step;
        m.count = g.kept - tm_search<false>(a.points + at * a.K, g.ring0, a.K, 0, g.kept, oldest);
      }
    }
    // the records before this row's and, under the same barrier, the round's models (block_scan_excl_i32; only the total of the second is used)
    const int v[2] = {m.count, m.track_id >= 0 ? 1 : 0};
    int before[2], all[2];
    block_scan_excl_i32<kTmPlanWaves, 2>(v, s_tot, before, all);
    if (m.track_id >= 0) m.first = base_records + before[0];
    if (r < a.T) models[(long)kb * a.T + r] = m;
    base_records += all[0]; base_models += all[1];
    __syncthreads();   // (the totals are read: the next round may write them)
  }
  if (tid == 0) { counts[2 * kb] = base_models; counts[2 * kb + 1] = base_records; }
}

// ------------------------------------------------------------------------------------------ M2
__global__ void MOT_TM_BOUNDS(kTmBlock)
track_models_transform_kernel(TrackModelBuffers a, int b0, int flags, mot_accum_point* __restrict__ points, long point_stride, mot_track_model* __restrict__ models) {
  __shared__ TmObsTile s_obs;
  const int r = blockIdx.x, kb = blockIdx.y, b = b0 + kb, tid = threadIdx.x;
  mot_track_model* __restrict__ mp = models + (long)kb * a.T + r;
  // M1's header of this row (the whole workgroup reads the same words: every exit below is taken by all of it)
  int count = mp->count;
  const long first = mp->first;
  if (mp->track_id < 0 || count <= 0 || first < 0) return;
  const long at = (long)b * a.T + r;
  const mot_accum_row row = a.rows[at];
  const TmRing g = tm_ring(row, a.K, a.O);
  if (g.n_obs <= 0) return;
  if (count > g.kept) count = g.kept;
  const int u0 = g.kept - count;   // the model is the suffix [u0, kept) of the unrolled ring
  const mot_accum_point* __restrict__ ring = a.points + at * a.K;
  const mot_accum_obs* __restrict__ log = a.obs + at * a.O;
  mot_accum_point* __restrict__ out = points + (long)kb * point_stride;
  const bool axes = (flags & MOT_MODEL_AXES) != 0;
  int lo_x = 0x7fffffff, lo_y = 0x7fffffff, lo_z = 0x7fffffff, hi_x = (int)0x80000000, hi_y = (int)0x80000000, hi_z = (int)0x80000000;
  int pos = 0;   // records [0, pos) of the model are done
  for (int t0 = 0; t0 < g.n_obs; t0 += kTmObsTile) {
    const int nt = g.n_obs - t0 < kTmObsTile ? g.n_obs - t0 : kTmObsTile;
    __syncthreads();   // (the previous tile is read)
    if (tid < nt) tm_load_obs(s_obs, tid, log[(g.obs0 + t0 + tid) & (a.O - 1)], axes);
    __syncthreads();
    // the tile's records: up to the last one of the tile's last step (the last tile takes what is left)
    int end = count;
    if (t0 + nt < g.n_obs) end = tm_search<true>(ring, g.ring0, a.K, u0 + pos, u0 + count, s_obs.step[nt - 1]) - u0;
    for (int i0 = pos; i0 < end; i0 += kTrackModelTile) {
      float4 p[kTmItems];
#pragma unroll
      for (int k = 0; k < kTmItems; k++) {
        const int i = i0 + k * kTmBlock + tid;
        if (i < end) p[k] = *reinterpret_cast<const float4*>(ring + ((g.ring0 + u0 + i) & (a.K - 1)));
      }
#pragma unroll
      for (int k = 0; k < kTmItems; k++) {
        const int i = i0 + k * kTmBlock + tid;
        if (i >= end) continue;
        const float4 q = tm_record(s_obs, nt, p[k], axes);
        if (first + i < point_stride) *reinterpret_cast<float4*>(out + first + i) = q;
        if (tm_finite(q.x) && tm_finite(q.y) && tm_finite(q.z)) {
          const int ix = tm_image(q.x), iy = tm_image(q.y), iz = tm_image(q.z);
          lo_x = ix < lo_x ? ix : lo_x; hi_x = ix > hi_x ? ix : hi_x;
          lo_y = iy < lo_y ? iy : lo_y; hi_y = iy > hi_y ? iy : hi_y;
          lo_z = iz < lo_z ? iz : lo_z; hi_z = iz > hi_z ? iz : hi_z;
        }
      }
    }
    pos = end;
  }
  lo_x = wave_reduce_i32(lo_x, OpMinI()); lo_y = wave_reduce_i32(lo_y, OpMinI()); lo_z = wave_reduce_i32(lo_z, OpMinI());
  hi_x = wave_reduce_i32(hi_x, OpMaxI()); hi_y = wave_reduce_i32(hi_y, OpMaxI()); hi_z = wave_reduce_i32(hi_z, OpMaxI());
  if (tid == 0) {
    const bool any = lo_x <= hi_x;   // (a finite record sets all six)
    mp->min_x = any ? tm_float(lo_x) : 0.f; mp->min_y = any ? tm_float(lo_y) : 0.f; mp->min_z = any ? tm_float(lo_z) : 0.f;
    mp->max_x = any ? tm_float(hi_x) : 0.f; mp->max_y = any ? tm_float(hi_y) : 0.f; mp->max_z = any ? tm_float(hi_z) : 0.f;
  }
}

// ------------------------------------------------------------------------------------------ host
void mot_launch_track_models_plan(const TrackModelBuffers& a, int first, int batch, int flags, mot_track_model* models, int* counts, hipStream_t stream) {
  hipLaunchKernelGGL(track_models_plan_kernel, dim3(batch), dim3(kTmPlanBlock), 0, stream, a, first, flags, models, counts);
}
void mot_launch_track_models_transform(const TrackModelBuffers& a, int first, int batch, int flags, mot_accum_point* points, long point_stride, mot_track_model* models,
                                       hipStream_t stream) {
  hipLaunchKernelGGL(track_models_transform_kernel, dim3(a.T, batch), dim3(kTmBlock), 0, stream, a, first, flags, points, point_stride, models);
}
