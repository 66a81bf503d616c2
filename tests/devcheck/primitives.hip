// primitives.hip — the small pure device functions of the product, driven directly. TEST INFRASTRUCTURE: a library of its own
// (tests/devcheck/libmot_primitives.so for gfx950, libmot_primitives_emu.so for the host; built by tests/devcheck/build_primitives.py),
// like sweep.hip. It includes the product's headers, so it runs the very functions the kernels inline:
//   mot_prim_wave     every primitive of mot_wave.h, per lane, nothing folded on the device (DPP body on gfx950, __shfl body on the host)
//   mot_prim_block_scan   block_scan_excl_i32 of mot_wave.h, one workgroup of 128 / 256 / 512 / 1024 threads per case, as the call sites use it (rounds, carry, barrier)
//   mot_prim_math     mot_atanf, mot_atan2f, mot_polar_cell_exact, mot_polar_bin_exact, mot_cart_cell of mot_math.h / mot_internal.h
//   mot_prim_det5 / mot_prim_inv2 / mot_prim_wrap_pi   the tracker's scalar fp64 helpers of mot_track_prep.h
//   mot_prim_box_fp64 the fp64 library calls of the box stage (box.hip, cluster_rect kernels: sqrt, atan2, cos, sin, each rounded to float)
// Every entry point is synchronous on the null stream, takes HOST pointers, and returns 0, 1 (bad argument) or 3 (a HIP call failed).
// The cases and their references are in tests/primitive_cases.py.
#include <string.h>

#include "mot_internal.h"
#include "mot_wave.h"
#include "mot_track_prep.h"

#ifndef MOT_HIPEMU
#define MOT_LAUNCH_BOUNDS(n) __launch_bounds__(n)
#else
#define MOT_LAUNCH_BOUNDS(n)
#endif

#ifdef MOT_HIPEMU
__attribute__((used)) __shared__ int hipemu_lds_anchor;   // the emulator's launcher clears the "mot_lds" section: it has to exist in every library built against it
#endif

// ------------------------------------------------------------------------------------------------------------------ wave and row primitives
// One 256-thread workgroup (four waves, sixteen rows) per case; every lane is active (mot_wave.h's contract).
struct PrimWaveIn {
  int id_min, id_max;            // the identities handed to wave_reduce_i32_id (no value of vi lies beyond them)
  int bcast_lane, fill;          // wave_bcast_i32's source lane; row_prev_i32 / row_next_i32's fill
  int vi[256];
  unsigned long long vu[256];
  double vd[256][8];             // row_sum_f64 sums vd[.][0]; row_sum8_f64 takes all eight
};
struct PrimWaveOut {
  int rmin[256], rmax[256], rmin_id[256], rmax_id[256], scan[256], sum[256], bcast[256], prev[256], next[256], idx8[256];
  unsigned long long umin[256], umax[256], uor[256], row_or[256];
  double row_sum[256], row_sum8[256];
};

__global__ void MOT_LAUNCH_BOUNDS(256)
prim_wave_kernel(const PrimWaveIn* __restrict__ in, PrimWaveOut* __restrict__ out) {
  const PrimWaveIn& c = in[blockIdx.x];
  PrimWaveOut& o = out[blockIdx.x];
  const int t = threadIdx.x;
  const int vi = c.vi[t];
  const unsigned long long vu = c.vu[t];
  double vd[8];
#pragma unroll
  for (int j = 0; j < 8; j++) vd[j] = c.vd[t][j];
  const int id_min = c.id_min, id_max = c.id_max, fill = c.fill;
  const int lane = wave_uniform_i32(c.bcast_lane);
  o.rmin[t] = wave_reduce_i32(vi, OpMinI());
  o.rmax[t] = wave_reduce_i32(vi, OpMaxI());
  o.rmin_id[t] = wave_reduce_i32_id(vi, OpMinI(), id_min);
  o.rmax_id[t] = wave_reduce_i32_id(vi, OpMaxI(), id_max);
  o.scan[t] = wave_scan_incl_i32(vi);
  o.sum[t] = wave_sum_i32(vi);
  o.bcast[t] = wave_bcast_i32(vi, lane);
  o.prev[t] = row_prev_i32(vi, fill);
  o.next[t] = row_next_i32(vi, fill);
  o.idx8[t] = row_sum8_index(t & 15);
  o.umin[t] = wave_reduce_u64(vu, OpMinU64());
  o.umax[t] = wave_reduce_u64(vu, OpMaxU64());
  o.uor[t] = wave_reduce_u64(vu, OpOrU64());
  o.row_or[t] = row_or_u64(vu);
  o.row_sum[t] = row_sum_f64(vd[0]);
  o.row_sum8[t] = row_sum8_f64(vd);
}

template <typename T>
static bool prim_upload(T** d, const void* src, size_t bytes) {
  *d = nullptr;
  if (hipMalloc((void**)d, bytes ? bytes : 8) != hipSuccess) return false;
  return !src || !bytes || hipMemcpy(*d, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
}
static int prim_finish(bool ok, void* dst, const void* d_src, size_t bytes) {   // synchronise, copy the result back
  ok = ok && hipDeviceSynchronize() == hipSuccess;
  if (ok && bytes) ok = hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost) == hipSuccess;
  return ok ? 0 : 3;
}

extern "C" int mot_prim_wave(const void* cases_in, int n_cases, void* cases_out) {
  if (!cases_in || !cases_out || n_cases < 0) return 1;
  PrimWaveIn* d_in; PrimWaveOut* d_out;
  bool ok = prim_upload(&d_in, cases_in, (size_t)n_cases * sizeof(PrimWaveIn));
  ok = prim_upload(&d_out, nullptr, (size_t)n_cases * sizeof(PrimWaveOut)) && ok;
  if (ok && n_cases) hipLaunchKernelGGL(prim_wave_kernel, dim3((unsigned)n_cases), dim3(256), 0, 0, d_in, d_out);
  const int rc = prim_finish(ok, cases_out, d_out, (size_t)n_cases * sizeof(PrimWaveOut));
  (void)hipFree(d_in); (void)hipFree(d_out);
  return rc;
}
extern "C" int mot_prim_wave_sizes(int* in_bytes, int* out_bytes) { *in_bytes = (int)sizeof(PrimWaveIn); *out_bytes = (int)sizeof(PrimWaveOut); return 0; }

// ------------------------------------------------------------------------------------------------------------------ the exact fp32 math
constexpr int kPrimPerThread = 64;   // elements per thread (strided), so that the host build starts few fibers

// out: five planes of n words — bits of mot_atanf(x), bits of mot_atan2f(y, x), mot_polar_cell_exact, mot_polar_bin_exact, and the
// Cartesian cell packed as sweep.hip packs it (xI * MOT_MAX_GRID + yI, -1 outside)
__global__ void MOT_LAUNCH_BOUNDS(256)
prim_math_kernel(MotDevParams p, const float* __restrict__ x, const float* __restrict__ y, long n, int* __restrict__ out) {
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float xv = x[i], yv = y[i];
    out[i] = mot_f2i(mot_atanf(xv));
    out[n + i] = mot_f2i(mot_atan2f(yv, xv));
    out[2 * n + i] = mot_polar_cell_exact(p, xv, yv);
    out[3 * n + i] = mot_polar_bin_exact(p, xv, yv);
    int xI, yI;
    out[4 * n + i] = mot_cart_cell(p, xv, yv, &xI, &yI) ? xI * MOT_MAX_GRID + yI : -1;
  }
}

static unsigned prim_blocks(long n) { const long b = (n + 256L * kPrimPerThread - 1) / (256L * kPrimPerThread); return (unsigned)(b < 1 ? 1 : b); }

// dev_params: a context's MotDevParams (mot_debug_dev_params, mot_debug_api.h)
extern "C" int mot_prim_math(const void* dev_params, const float* x, const float* y, long n, int* out5n) {
  if (!dev_params || !x || !y || !out5n || n < 0 || n > (1L << 26)) return 1;
  MotDevParams p;
  memcpy(&p, dev_params, sizeof p);
  float *dx, *dy; int* d_out;
  bool ok = prim_upload(&dx, x, (size_t)n * 4);
  ok = prim_upload(&dy, y, (size_t)n * 4) && ok;
  ok = prim_upload(&d_out, nullptr, (size_t)n * 20) && ok;
  if (ok && n) hipLaunchKernelGGL(prim_math_kernel, dim3(prim_blocks(n)), dim3(256), 0, 0, p, dx, dy, n, d_out);
  const int rc = prim_finish(ok, out5n, d_out, (size_t)n * 20);
  (void)hipFree(dx); (void)hipFree(dy); (void)hipFree(d_out);
  return rc;
}

// ------------------------------------------------------------------------------------------------------------------ the tracker's scalar helpers
__global__ void MOT_LAUNCH_BOUNDS(256)
prim_det5_kernel(const double* __restrict__ m, long n, double* __restrict__ out) {
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) out[i] = det5(m + i * 25);
}
__global__ void MOT_LAUNCH_BOUNDS(256)
prim_inv2_kernel(const double* __restrict__ m, long n, double* __restrict__ out) {   // out: n x 5 — the inverse, then det2
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    double o[4];
    inv2(m + i * 4, o);
    for (int k = 0; k < 4; k++) out[i * 5 + k] = o[k];
    out[i * 5 + 4] = det2(m + i * 4);
  }
}
__global__ void MOT_LAUNCH_BOUNDS(256)
prim_wrap_pi_kernel(const double* __restrict__ a, long n, double* __restrict__ out) {
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) out[i] = wrap_pi(a[i]);
}

// which: 0 det5 (in n x 25, out n), 1 inv2 + det2 (in n x 4, out n x 5), 2 wrap_pi (in n, out n)
static int prim_scalar(int which, const double* in, long n, double* out) {
  static const int kIn[3] = {25, 4, 1}, kOut[3] = {1, 5, 1};
  if (!in || !out || n < 0 || n > (1L << 24)) return 1;
  double *d_in, *d_out;
  bool ok = prim_upload(&d_in, in, (size_t)n * kIn[which] * 8);
  ok = prim_upload(&d_out, nullptr, (size_t)n * kOut[which] * 8) && ok;
  if (ok && n) {
    if (which == 0) hipLaunchKernelGGL(prim_det5_kernel, dim3(prim_blocks(n)), dim3(256), 0, 0, d_in, n, d_out);
    else if (which == 1) hipLaunchKernelGGL(prim_inv2_kernel, dim3(prim_blocks(n)), dim3(256), 0, 0, d_in, n, d_out);
    else hipLaunchKernelGGL(prim_wrap_pi_kernel, dim3(prim_blocks(n)), dim3(256), 0, 0, d_in, n, d_out);
  }
  const int rc = prim_finish(ok, out, d_out, (size_t)n * kOut[which] * 8);
  (void)hipFree(d_in); (void)hipFree(d_out);
  return rc;
}
extern "C" int mot_prim_det5(const double* m25, long n, double* out) { return prim_scalar(0, m25, n, out); }
extern "C" int mot_prim_inv2(const double* m4, long n, double* out5) { return prim_scalar(1, m4, n, out5); }
extern "C" int mot_prim_wrap_pi(const double* a, long n, double* out) { return prim_scalar(2, a, n, out); }

// ------------------------------------------------------------------------------------------------------------------ the box stage's fp64 calls
// The expression chains of box.hip's rectangle epilogue (cluster_rect kernels: "cv::minAreaRect" / "RotatedRect::points"), as they stand there.
// mode 0: the two-point hull branch — (a, b) = (s_hx[1] - s_hx[0], s_hy[1] - s_hy[0]), float differences of pixel indices;
// mode 1: the rotating-calipers branch — (a, b) = (o2, o3), a unit direction times a width. out: four planes of n floats — width, angle in
// radians, cos, sin.
__global__ void MOT_LAUNCH_BOUNDS(256)
prim_box_fp64_kernel(const float* __restrict__ a, const float* __restrict__ b, long n, int mode, float* __restrict__ out) {
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    float w, angle;
    if (mode == 0) {
      double dx = a[i], dy = b[i];
      w = (float)sqrt(dx * dx + dy * dy);
      angle = (float)atan2(dy, dx);
    } else {
      const float o2 = a[i], o3 = b[i];
      w = (float)sqrt((double)o2 * o2 + (double)o3 * o3);
      angle = (float)atan2((double)o3, (double)o2);
    }
    out[i] = w;
    out[n + i] = angle;
    angle = (float)(angle * 180 / 3.1415926535897932384626433832795);
    // RotatedRect::points
    double _angle = angle * 3.1415926535897932384626433832795 / 180.;
    out[2 * n + i] = (float)cos(_angle);
    out[3 * n + i] = (float)sin(_angle);
  }
}

extern "C" int mot_prim_box_fp64(const float* a, const float* b, long n, int mode, float* out4n) {
  if (!a || !b || !out4n || n < 0 || n > (1L << 26) || mode < 0 || mode > 1) return 1;
  float *da, *db, *d_out;
  bool ok = prim_upload(&da, a, (size_t)n * 4);
  ok = prim_upload(&db, b, (size_t)n * 4) && ok;
  ok = prim_upload(&d_out, nullptr, (size_t)n * 16) && ok;
  if (ok && n) hipLaunchKernelGGL(prim_box_fp64_kernel, dim3(prim_blocks(n)), dim3(256), 0, 0, da, db, n, mode, d_out);
  const int rc = prim_finish(ok, out4n, d_out, (size_t)n * 16);
  (void)hipFree(da); (void)hipFree(db); (void)hipFree(d_out);
  return rc;
}

// ------------------------------------------------------------------------------------------------------------------ the workgroup scan
// block_scan_excl_i32 of mot_wave.h as its call sites use it: one workgroup of WAVES * 64 threads per case, `rounds` rounds chained through a carry, an LDS
// array of exactly WAVES * N words, and the caller's barrier before the words are written again. v and excl: [case][round][thread][N]; totals: [case][round][N].
template <int WAVES, int N>
__global__ void MOT_LAUNCH_BOUNDS(WAVES * 64)
prim_block_scan_kernel(const int* __restrict__ v, int rounds, int* __restrict__ excl, int* __restrict__ totals) {
  __shared__ int s_tot[WAVES * N];
  const int t = threadIdx.x;
  int carry[N];
#pragma unroll
  for (int c = 0; c < N; c++) carry[c] = 0;
  for (int r = 0; r < rounds; r++) {   // (uniform)
    const long row = (long)blockIdx.x * rounds + r, at = (row * (WAVES * 64) + t) * N;
    int in[N], before[N], all[N];
#pragma unroll
    for (int c = 0; c < N; c++) in[c] = v[at + c];
    if constexpr (N == 1) before[0] = block_scan_excl_i32<WAVES>(in[0], s_tot, all[0]);   // (the single-value wrapper, as most call sites)
    else block_scan_excl_i32<WAVES, N>(in, s_tot, before, all);
#pragma unroll
    for (int c = 0; c < N; c++) {
      excl[at + c] = carry[c] + before[c];
      if (t == 0) totals[row * N + c] = all[c];
      carry[c] += all[c];
    }
    __syncthreads();   // (s_tot is written again in the next round)
  }
}

template <int WAVES>
static void prim_block_scan_launch(int n_cases, int n, int rounds, const int* v, int* excl, int* totals) {
  if (n == 1) hipLaunchKernelGGL((prim_block_scan_kernel<WAVES, 1>), dim3((unsigned)n_cases), dim3(WAVES * 64), 0, 0, v, rounds, excl, totals);
  else hipLaunchKernelGGL((prim_block_scan_kernel<WAVES, 2>), dim3((unsigned)n_cases), dim3(WAVES * 64), 0, 0, v, rounds, excl, totals);
}

// waves in {2, 4, 8, 16} (the block sizes of the product's call sites), n in {1, 2} components, rounds in {1, 3}
extern "C" int mot_prim_block_scan(const int* v, int n_cases, int waves, int n, int rounds, int* excl, int* totals) {
  if (!v || !excl || !totals || n_cases < 0 || n_cases > 4096 || (waves != 2 && waves != 4 && waves != 8 && waves != 16) || (n != 1 && n != 2) || (rounds != 1 && rounds != 3)) return 1;
  const size_t words = (size_t)n_cases * rounds * waves * 64 * n, tot_words = (size_t)n_cases * rounds * n;
  int *d_v, *d_excl, *d_tot;
  bool ok = prim_upload(&d_v, v, words * 4);
  ok = prim_upload(&d_excl, nullptr, words * 4) && ok;
  ok = prim_upload(&d_tot, nullptr, tot_words * 4) && ok;
  if (ok && n_cases) {
    switch (waves) {
      case 2: prim_block_scan_launch<2>(n_cases, n, rounds, d_v, d_excl, d_tot); break;
      case 4: prim_block_scan_launch<4>(n_cases, n, rounds, d_v, d_excl, d_tot); break;
      case 8: prim_block_scan_launch<8>(n_cases, n, rounds, d_v, d_excl, d_tot); break;
      default: prim_block_scan_launch<16>(n_cases, n, rounds, d_v, d_excl, d_tot); break;
    }
  }
  int rc = prim_finish(ok, excl, d_excl, words * 4);
  if (rc == 0 && tot_words && hipMemcpy(totals, d_tot, tot_words * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = 3;
  (void)hipFree(d_v); (void)hipFree(d_excl); (void)hipFree(d_tot);
  return rc;
}
