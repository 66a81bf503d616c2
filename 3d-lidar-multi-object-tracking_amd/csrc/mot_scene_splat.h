// mot_scene_splat.h — what the splat kernels of scene_grid.hip (one step per slot) and scene_grid_seq.hip (a recorded drive in one launch) share: the window a matrix
// asks for, a frame's points as every scene kernel loads them, the KIND of an owned point (one rule per form), THE per-point step (transform, cell test, storage
// index), the wave's merged adds and scene_splat_body, the ONE body of both splat kernels. One definition, so that a drive taken in one call bins the very bits the
// frame-by-frame route bins (include/mot.h, rolling static-scene grid). Product code.
#ifndef MOT_SCENE_SPLAT_H_
#define MOT_SCENE_SPLAT_H_
#include "mot_internal.h"
#include "mot_wave.h"

#ifndef MOT_HIPEMU
#define MOT_SG_BOUNDS(n) __launch_bounds__(n)
#else
#define MOT_SG_BOUNDS(n)
#endif
#ifndef MOT_SCENE_MERGE
#define MOT_SCENE_MERGE 1
#endif
#ifndef MOT_SCENE_RUN
#define MOT_SCENE_RUN 64   // lanes a run may span: 16 (a DPP row) or 64 (profiles/scene_grid.md has both)
#endif
static_assert(MOT_SCENE_RUN == 16 || MOT_SCENE_RUN == 64, "runs end at multiples of 16 or of 64 lanes");

constexpr int kSceneBlock = 256, kSceneItems = kSceneChunk / kSceneBlock;
static_assert(kSceneChunk % kSceneBlock == 0, "every thread takes the same number of points");

constexpr float kSceneLimit = 1073741824.f;   // 2^30

// the window a matrix asks for: false when either product is not finite or is >= 2^30 in magnitude (NaN fails both compares)
__device__ __forceinline__ bool scene_window(const EgoTf& m, float inv, int W, int* oi, int* oj) {
  const float a = m.m[3] * inv, c = m.m[7] * inv;
  if (!(fabsf(a) < kSceneLimit) || !(fabsf(c) < kSceneLimit)) return false;
  *oi = (int)floorf(a) - W / 2;
  *oj = (int)floorf(c) - W / 2;
  return true;
}

// ---- a frame's points: slot `slot` of the elevated cloud, as the splat, classify and scatter kernels of both forms see them
// the clamped count (never beyond the slot: the counts are the device's)
__device__ __forceinline__ int scene_count(const SceneSplatInput& in, int slot) {
  const int n = in.counts[slot * kCountsStride + kCntElev];
  return n < 0 ? 0 : (n < (int)in.cap ? n : (int)in.cap);
}
// id[] / q[] of a thread's kSceneItems points of the chunk from `base`; a lane beyond n holds id -1 and a zero point
__device__ __forceinline__ void scene_load_points(const SceneSplatInput& in, int slot, long base, int n, int tid, int (&id)[kSceneItems], float4 (&q)[kSceneItems]) {
  const int* __restrict__ ids = in.ids + (long)slot * in.cap;
  const float4* __restrict__ cloud = in.elevated + (long)slot * in.cap;
#pragma unroll
  for (int k = 0; k < kSceneItems; k++) {
    const long i = base + k * kSceneBlock + tid;
    id[k] = -1;
    q[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n) { id[k] = ids[i]; q[k] = mot_load_xyz(cloud, i, in.elevated_packed); }
  }
}

// ---- the grid's KIND rule for an OWNED point (id >= 0; a point without owner is static): is its owner something other than a track flagged static? An id or a
// track slot that is out of range is not followed and counts as dynamic. Splat and classify of a form ask the same struct.
// live: slot b's map id -> track slot -> is_static as the step left it (two dependent gathers)
struct SceneKindLive {
  const int* __restrict__ slot_of; const mot_track* __restrict__ out; int E, T;
  __device__ __forceinline__ SceneKindLive(const SceneSplatInput& in, int b) : slot_of(in.slot_of + (long)b * in.E), out(in.out + (long)b * in.T), E(in.E), T(in.T) {}
  __device__ __forceinline__ int dynamic(int id) const {
    if (id >= E) return 1;
    const int r = slot_of[id];
    return (r >= 0 && r < T) ? out[r].is_static == 0 : 1;
  }
};
// recorded: bit `id` of frame k's row of the table scene_seq_capture_kernel filled behind step k (one gather; a slot outside [0, T) set no bit)
struct SceneKindRecorded {
  const unsigned* __restrict__ flagged; int E;
  __device__ __forceinline__ SceneKindRecorded(const SceneSplatInput& in, const SceneSeqBuffers& s, int k) : flagged(s.is_static + (long)k * s.words), E(in.E) {}
  __device__ __forceinline__ int dynamic(int id) const { return id >= E ? 1 : ((flagged[id >> 5] >> (id & 31)) & 1u) == 0u; }
};

// global cells [lo_i, hi_i) x [lo_j, hi_j) whose adds count: a step's window, or what is left of it once the later windows of a drive are known (may be empty)
struct SceneRect { int lo_i, hi_i, lo_j, hi_j; };

// THE per-point step: sensor -> global, the finite and 2^30 tests, the cell. Returns the cell's storage index when the point takes part (`take`: the point exists and its
// step has a valid window), -1 otherwise; *gz is the point's global z either way.
// fp32, left to right; the build has -ffp-contract=off (mot_track_place.h's sensor -> global step: the very bits the MOT_FRAME_GLOBAL export writes)
__device__ __forceinline__ int scene_point_cell(const EgoTf& m, const float4& q, float inv, bool take, const SceneRect& r, int W, float* gz_out) {
  const float gx = m.m[0] * q.x + m.m[1] * q.y + m.m[2] * q.z + m.m[3];
  const float gy = m.m[4] * q.x + m.m[5] * q.y + m.m[6] * q.z + m.m[7];
  const float gz = m.m[8] * q.x + m.m[9] * q.y + m.m[10] * q.z + m.m[11];
  *gz_out = gz;
  const float tx = gx * inv, ty = gy * inv;
  bool inside = take && (gx - gx == 0.f) && (gy - gy == 0.f) && (gz - gz == 0.f) && fabsf(tx) < kSceneLimit && fabsf(ty) < kSceneLimit;
  int gi = 0, gj = 0;
  if (inside) {
    gi = (int)floorf(tx); gj = (int)floorf(ty);   // exact: |t| < 2^30; origins lie within 2^30 + W / 2, so no compare below overflows
    inside = gi >= r.lo_i && gi < r.hi_i && gj >= r.lo_j && gj < r.hi_j;
  }
  return inside ? (gj & (W - 1)) * W + (gi & (W - 1)) : -1;
}

// What a wave's 64 points add: key = (storage index << 1) | kind, -1: nothing. EVERY lane of the wave calls this (no divergent exit before it). ONE lane per run of
// neighbouring lanes with the same key adds the run's length and its largest z. kSeenMax: several steps meet in one launch, so last_seen is an integer maximum
// (stamps are positive, 0 is "never"); otherwise every writer of the launch stores the same value.
template <bool kSeenMax>
__device__ __forceinline__ void scene_add_wave(SceneCell* __restrict__ cells, int key, float gz, int stamp, int lane) {
  const unsigned zkey = (unsigned)mot_float_key(gz) ^ 0x80000000u;
#if MOT_SCENE_MERGE
  // the lane before me, then the heads of the runs
  const int before = __shfl_up(key, 1, 64);
  const bool head = (lane & (MOT_SCENE_RUN - 1)) == 0 || before != key;
  const unsigned long long heads = __ballot(head);
  const unsigned long long above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
  int end = above ? __ffsll(above) - 1 : 64;   // first lane of the next run
  const int row_end = (lane | (MOT_SCENE_RUN - 1)) + 1;
  if (end > row_end) end = row_end;
  unsigned zmax = zkey;
#pragma unroll
  for (int d = 1; d < MOT_SCENE_RUN; d <<= 1) {   // lane l holds the maximum over [l, min(end, l + 2 d))
    const unsigned o = __shfl_down(zmax, d, 64);
    if (lane + d < end && o > zmax) zmax = o;
  }
  const unsigned count = (unsigned)(end - lane);
  const bool writer = head && key >= 0;
#else
  const unsigned zmax = zkey, count = 1u;
  const bool writer = key >= 0;
#endif
  if (writer) {
    SceneCell* __restrict__ c = cells + (key >> 1);
    if (key & 1) atomicAdd(&c->dynamic_hits, count);
    else { atomicAdd(&c->static_hits, count); atomicMax(&c->zkey, zmax); }
    if (kSeenMax) atomicMax(&c->last_seen, stamp);
    else c->last_seen = stamp;
  }
}

// the step's three counters into its header: one add per wave and counter
__device__ __forceinline__ void scene_count_wave(mot_scene_header* __restrict__ hdr, int n_static, int n_dynamic, int n_outside, int lane) {
  n_static = wave_sum_i32(n_static); n_dynamic = wave_sum_i32(n_dynamic); n_outside = wave_sum_i32(n_outside);
  if (lane == 0) {
    if (n_static) atomicAdd(&hdr->n_static, (unsigned)n_static);
    if (n_dynamic) atomicAdd(&hdr->n_dynamic, (unsigned)n_dynamic);
    if (n_outside) atomicAdd(&hdr->n_outside, (unsigned)n_outside);
  }
}

// THE splat body: chunk blockIdx.x of frame `slot` into `cells`. What the two kernels decide for themselves and hand in:
//   live (scene_splat_kernel)          rect = the slot's window from its header, ok = prev[b].ok (and workgroup (0, b) moves prev[b]'s origin on, in the kernel);
//                                      kSeenMax = false: last_seen is stored plainly; count = true: the counters are always added; cells and header are slot b's
//   recorded (scene_seq_splat_kernel)  rect = R[k], ok = s.win[k + 1].ok (a frame that is not the last has left, in the kernel, when nothing of it survives);
//                                      kSeenMax = true: last_seen by atomicMax; count = the frame is the last one; cells and header are slot 0's
// The kind is asked only of a point that is `inside`: no gather for a point that adds nothing (the classify body asks every valid point: MOVING needs no cell).
// No exit on max_chunks here (the judge's bodies have one): the launch's grid is the chunk count. Every lane of a wave reaches every scene_add_wave.
template <bool kSeenMax, class Kind>
__device__ __forceinline__ void scene_splat_body(const SceneSplatInput& in, int slot, const EgoTf* __restrict__ tf, float inv, bool window_ok, const SceneRect& rect, int W,
                                                 const Kind& kind, SceneCell* __restrict__ cells, int stamp, mot_scene_header* __restrict__ hdr, bool count) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int n = scene_count(in, slot);
  const long base = (long)blockIdx.x * kSceneChunk;
  if (base >= n) return;   // (uniform over the workgroup)
  const EgoTf m = *tf;
  int id[kSceneItems];
  float4 q[kSceneItems];
  scene_load_points(in, slot, base, n, tid, id, q);
  int n_static = 0, n_dynamic = 0, n_outside = 0;
#pragma unroll
  for (int k = 0; k < kSceneItems; k++) {
    const long i = base + k * kSceneBlock + tid;
    const bool valid = i < n;
    float gz;
    const int at = scene_point_cell(m, q[k], inv, valid && window_ok, rect, W, &gz);
    const bool inside = at >= 0;
    const int dynamic = (inside && id[k] >= 0) ? kind.dynamic(id[k]) : 0;
    n_static += inside && !dynamic; n_dynamic += inside && dynamic; n_outside += valid && !inside;
    // what the point adds to: (storage index, kind), -1: nothing
    scene_add_wave<kSeenMax>(cells, inside ? ((at << 1) | dynamic) : -1, gz, stamp, lane);
  }
  if (count) scene_count_wave(hdr, n_static, n_dynamic, n_outside, lane);   // (uniform over the launch's row of workgroups)
}
#endif
