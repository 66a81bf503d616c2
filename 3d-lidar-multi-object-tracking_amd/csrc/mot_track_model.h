// mot_track_model.h — device helpers the kernels of track_models.hip and track_voxels.hip share: how a row's two rings are read, and THE per-record transform of the
// object-centred models (include/mot.h, RECORD). One definition, so that the voxel models bin the very bits the raw export writes. Product code.
#ifndef MOT_TRACK_MODEL_H_
#define MOT_TRACK_MODEL_H_
#include "mot_internal.h"

constexpr int kTmObsTile = 64;   // observations in LDS at a time (a power of two: the lower bound halves it)
static_assert((kTmObsTile & (kTmObsTile - 1)) == 0, "the lower bound of tm_record halves the tile");

// what a row says of its two rings, every number inside the tables whatever the row holds
struct TmRing { int kept, ring0, n_obs, obs0; };
__device__ __forceinline__ TmRing tm_ring(const mot_accum_row& row, int K, int O) {
  TmRing g;
  g.kept = row.total < (unsigned long long)K ? (int)row.total : K;
  g.ring0 = row.total > (unsigned long long)K ? (int)(row.total & (unsigned long long)(K - 1)) : 0;
  g.n_obs = row.obs_total < 0 ? 0 : (row.obs_total < O ? row.obs_total : O);
  g.obs0 = row.obs_total > O ? (row.obs_total & (O - 1)) : 0;
  return g;
}
// first unrolled position in [lo, hi) whose step is not below / is above `step` (hi when none)
template <bool kAbove>
__device__ __forceinline__ int tm_search(const mot_accum_point* __restrict__ ring, int ring0, int K, int lo, int hi, int step) {
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    const int s = ring[(ring0 + mid) & (K - 1)].step;
    if (kAbove ? s <= step : s < step) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// order-preserving integer image of a float (a < b as floats <=> image(a) < image(b) as ints; -0.0 sits right below +0.0)
__device__ __forceinline__ int tm_image(float v) { const int i = __float_as_int(v); return i ^ ((i >> 31) & 0x7fffffff); }
__device__ __forceinline__ float tm_float(int i) { return __int_as_float(i ^ ((i >> 31) & 0x7fffffff)); }
__device__ __forceinline__ bool tm_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// a tile of the log in LDS: {step, px, py, c, s} of up to kTmObsTile consecutive observations (c, s: cos / sin of the yaw in double, rounded once to fp32, once
// per observation; written with MOT_MODEL_AXES only)
struct TmObsTile { int step[kTmObsTile]; float px[kTmObsTile], py[kTmObsTile], c[kTmObsTile], s[kTmObsTile]; };
__device__ __forceinline__ void tm_load_obs(TmObsTile& t, int k, const mot_accum_obs& o, bool axes) {
  t.step[k] = o.step; t.px[k] = o.px; t.py[k] = o.py;
  if (axes) { double sn, cs; sincos(o.yaw, &sn, &cs); t.c[k] = (float)cs; t.s[k] = (float)sn; }   // (one argument reduction for both: 8 VGPRs less than cos + sin)
}
// THE record of a model: ring point p = {x, y, z, step bits} against the tile's nt observations (ascending in step) -> {x', y', z, step bits}. The point's own
// observation is the last one of the tile whose step is not above the point's (a branch-free lower bound; neighbouring points share a step: broadcast reads);
// dx, dy one fp32 subtraction each, the rotation left to right, -ffp-contract=off (build.py), no fast-math intrinsic.
__device__ __forceinline__ float4 tm_record(const TmObsTile& t, int nt, float4 p, bool axes) {
  const int step = __float_as_int(p.w);
  int j = 0;
#pragma unroll
  for (int h = kTmObsTile / 2; h >= 1; h >>= 1)
    if (j + h < nt && t.step[j + h] <= step) j += h;
  const float dx = p.x - t.px[j], dy = p.y - t.py[j];
  float4 q = p;
  if (axes) {
    const float c = t.c[j], s = t.s[j];
    q.x = c * dx + s * dy;
    q.y = c * dy - s * dx;
  } else {
    q.x = dx; q.y = dy;
  }
  return q;
}
#endif  // MOT_TRACK_MODEL_H_
