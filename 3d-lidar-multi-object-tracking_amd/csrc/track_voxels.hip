// track_voxels.hip — voxel-thinned object models from the per-track accumulators, on gfx950. Product code (HIP, wave64).
//
// track_models.hip gives every track's accumulated points in the object's frame: the raw ring, the same surface scanned step after step. Here the same records — the
// same rows, the same transform (tm_record, mot_track_model.h) — are reduced to ONE RECORD PER OCCUPIED VOXEL of a lattice anchored at the track's position: the
// centroid of the cell's records and their number, in ascending (i_z, i_y, i_x), packed per stream. The kernels only READ the accumulators.
//
// A model is at most K <= 4096 records and one workgroup owns it, so the sort that groups the records by cell runs in LDS. The models are SORTED TWICE, once to
// count and once to write, instead of staging every model's voxels in library memory until the stream's packing is known: a staging block would have to hold the
// worst case, batch x T x K records — the size of the rings themselves, 2 GB in the shape of profiles/track_voxels.md — where the second sort costs LDS traffic
// alone and a call for the headers never runs it. The library's scratch is 96 bytes per row.
//
//   V0  track_models_plan_kernel (track_models.hip) into library scratch: every row's raw first / count, the rows that give a model
//   V1  track_voxels_count_kernel   one workgroup of 512 per (row, stream), rows without a model leave at once. The model's records stream through tm_record exactly as
//                                   in the raw export (the log in LDS in tiles of 64 observations); a record with three finite coordinates and a cell on the lattice
//                                   puts (key << 13 | record index) into LDS, key = (i_z + 512) << 22 | (i_y + 1024) << 11 | (i_x + 1024), every other record all ones
//                                   (it sorts behind every cell and is counted in n_outside). A bitonic network over the next power of two at or above the model's
//                                   count (64 at least) sorts the 64-bit entries, its three innermost merge distances in registers: a small model does not pay for 4096. The entries are distinct (the index), so the
//                                   sorted order is unique. Every thread then owns 8 consecutive sorted positions: it marks the run heads (a cell differs from its
//                                   predecessor's), and a run's length is what is left of it in the head's chunk plus the LEADING parts of the chunks behind, walked
//                                   chunk by chunk up to the next head — 8 + 511 steps at the most, never 4096. Heads whose run holds min_points records are voxels,
//                                   the others n_sparse; the raw extent as in the raw export (integer min / max). -> 48 bytes of result per row
//   V2  track_voxels_pack_kernel    one workgroup per stream, threads over the T rows as the plan kernel: exclusive scan of the rows' voxel counts (block_scan_excl_i32) -> first, the 64-byte
//                                   headers, the stream's two counts
//   V3  track_voxels_write_kernel   V1's sort again (the same entries, hence the same order), for the models with a voxel below voxel_stride; not launched without a
//                                   voxel block. The inverse permutation (16 bits per record) goes beside the entries, the records stream through tm_record a second
//                                   time and land in LDS AT THEIR SORTED POSITION, over the entries they no longer need. Every thread sums the leading part of its chunk
//                                   in fp64; a head's sums are its own chunk's records in sorted order plus the leading sums of the chunks behind, in order: linear
//                                   work when every record falls in one voxel, a fixed order of additions whatever runs where. (float)(sum / count), count, stored
//                                   only below voxel_stride.
//
// No floating-point atomics, no workgroup waits on another: the order between the four launches is the only synchronisation. Two calls give identical bytes.
// Every index is checked or masked where it is used: ring and log positions are masked with K - 1 / O - 1, a count read back from memory is clamped to what the row
// holds and to the 4096 entries of LDS, sorted positions come from the entries of this workgroup alone (index < count), the headers V3 reads back from the caller's
// block only decide WHETHER a voxel is stored (below the header's count and below voxel_stride). Garbage in a row, a ring, a log or a header cannot produce an
// address outside the tables, the scratch or the caller's voxel_stride records.
// Resources (tools/kernel_resources.py): V1 60 VGPRs, 35 360 bytes of LDS, 8 waves per SIMD; V2 46 VGPRs, 64 bytes, 8 waves per SIMD; V3 80 VGPRs, 64 032 bytes of LDS,
// 4 waves per SIMD (two workgroups per CU: LDS, not registers, sets it); no scratch in any.
#include "mot_internal.h"
#include "mot_wave.h"
#include "mot_track_model.h"

#ifndef MOT_HIPEMU
#define MOT_TV_BOUNDS(n) __launch_bounds__(n)
#else
#define MOT_TV_BOUNDS(n)
#endif

constexpr int kTvBlock = 512, kTvWaves = kTvBlock / 64;
constexpr int kTvMaxK = MOT_MODEL_VOXEL_MAX_K;     // entries of LDS: the longest model
constexpr int kTvChunk = kTvMaxK / kTvBlock;       // consecutive sorted positions a thread owns
constexpr int kTvIndexBits = 13;
constexpr unsigned long long kTvOutside = ~0ull;   // (a cell's entry is below 2^45)
static_assert(kTvChunk == 8 && kTvMaxK <= (1 << kTvIndexBits) && kTvMaxK <= 65536, "a chunk is the eight entries tv_sort_local holds in registers; positions are 16 bits, the index 13");
static_assert(sizeof(mot_track_voxel_model) == 64 && sizeof(mot_model_voxel) == 16 && sizeof(TrackVoxelResult) == 48, "include/mot.h documents the sizes");

// the cell of a record (include/mot.h, CELL): false when it takes no part
__device__ __forceinline__ bool tv_key(const float4& q, const TrackVoxelArgs& v, unsigned* key) {
  if (!(tm_finite(q.x) && tm_finite(q.y) && tm_finite(q.z))) return false;
  const float tx = q.x * v.inv_x, ty = q.y * v.inv_y, tz = q.z * v.inv_z;
  if (!(tx >= -1024.f && tx < 1024.f && ty >= -1024.f && ty < 1024.f && tz >= -512.f && tz < 512.f)) return false;
  const int ix = (int)floorf(tx), iy = (int)floorf(ty), iz = (int)floorf(tz);
  *key = ((unsigned)(iz + 512) << 22) | ((unsigned)(iy + 1024) << 11) | (unsigned)(ix + 1024);
  return true;
}

// the model's records through the raw export's transform, f(i, q) for record i = 0 .. count - 1 (each exactly once, by some thread). A collective of the workgroup.
template <typename F>
__device__ __forceinline__ void tv_stream(const TrackModelBuffers& a, long at, const TmRing& g, int count, bool axes, TmObsTile& s_obs, F f) {
  const int tid = threadIdx.x;
  const int u0 = g.kept - count;   // the model is the suffix [u0, kept) of the unrolled ring
  const mot_accum_point* __restrict__ ring = a.points + at * a.K;
  const mot_accum_obs* __restrict__ log = a.obs + at * a.O;
  int pos = 0;
  for (int t0 = 0; t0 < g.n_obs; t0 += kTmObsTile) {
    const int nt = g.n_obs - t0 < kTmObsTile ? g.n_obs - t0 : kTmObsTile;
    __syncthreads();   // (the previous tile is read)
    if (tid < nt) tm_load_obs(s_obs, tid, log[(g.obs0 + t0 + tid) & (a.O - 1)], axes);
    __syncthreads();
    int end = count;
    if (t0 + nt < g.n_obs) end = tm_search<true>(ring, g.ring0, a.K, u0 + pos, u0 + count, s_obs.step[nt - 1]) - u0;
    for (int i = pos + tid; i < end; i += kTvBlock)
      f(i, tm_record(s_obs, nt, *reinterpret_cast<const float4*>(ring + ((g.ring0 + u0 + i) & (a.K - 1))), axes));
    pos = end;
  }
}

// ascending bitonic network over s[0, n2), n2 a power of two >= 64. The merge steps at distances 4, 2, 1 — and the whole of the first three levels — run in
// registers, a thread on eight consecutive entries: 45 trips through LDS for 4096 entries where the plain network takes 78. A collective of the workgroup; ends
// behind a barrier.
__device__ __forceinline__ void tv_ce(unsigned long long& x, unsigned long long& y, bool up) {
  const bool sw = (x > y) == up;
  const unsigned long long lo = sw ? y : x, hi = sw ? x : y;
  x = lo; y = hi;
}
template <bool kFirst>
__device__ __forceinline__ void tv_sort_local(unsigned long long* s, int n2, int k) {
  for (int t = threadIdx.x; t < (n2 >> 3); t += kTvBlock) {
    const int base = t << 3;
    unsigned long long e[8];
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = s[base + i];
    if (kFirst) {   // levels 2 and 4: the direction of a pair is a matter of its place in the eight
#pragma unroll
      for (int kk = 2; kk <= 4; kk <<= 1)
#pragma unroll
        for (int j = kk >> 1; j > 0; j >>= 1)
#pragma unroll
          for (int i = 0; i < 8; i++)
            if (!(i & j)) tv_ce(e[i], e[i | j], (i & kk) == 0);
    }
    const bool up = (base & k) == 0;   // (k >= 8: one direction for the eight)
#pragma unroll
    for (int j = 4; j > 0; j >>= 1)
#pragma unroll
      for (int i = 0; i < 8; i++)
        if (!(i & j)) tv_ce(e[i], e[i | j], up);
#pragma unroll
    for (int i = 0; i < 8; i++) s[base + i] = e[i];
  }
  __syncthreads();
}
__device__ __forceinline__ void tv_sort(unsigned long long* s, int n2) {
  const int tid = threadIdx.x;
  __syncthreads();
  tv_sort_local<true>(s, n2, 8);
  for (int k = 16; k <= n2; k <<= 1) {
    for (int j = k >> 1; j >= 8; j >>= 1) {
      for (int t = tid; t < (n2 >> 1); t += kTvBlock) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const unsigned long long x = s[i], y = s[l];
        if ((x > y) == ((i & k) == 0)) { s[i] = y; s[l] = x; }
      }
      __syncthreads();
    }
    tv_sort_local<false>(s, n2, k);
  }
}

// what a thread knows of its chunk of sorted positions [c0, c0 + len) (len 0: the chunk lies behind the valid entries)
struct TvChunk { int c0, len; unsigned heads; };
__device__ __forceinline__ TvChunk tv_heads(const unsigned long long* s_ent, int n_valid) {
  TvChunk c;
  c.c0 = (int)threadIdx.x * kTvChunk;
  c.len = n_valid - c.c0 < kTvChunk ? n_valid - c.c0 : kTvChunk;
  if (c.len < 0) c.len = 0;
  c.heads = 0;
  unsigned long long prev = c.c0 > 0 && c.len > 0 ? s_ent[c.c0 - 1] >> kTvIndexBits : 0;
  for (int q = 0; q < c.len; q++) {
    const unsigned long long key = s_ent[c.c0 + q] >> kTvIndexBits;
    if (c.c0 + q == 0 || key != prev) c.heads |= 1u << q;
    prev = key;
  }
  return c;
}
// records of the run whose head is position q of the chunk; *spill: chunks behind the head's that the run reaches into (their leading parts belong to it)
__device__ __forceinline__ int tv_run(const TvChunk& c, int q, const unsigned short* s_heads, int n_valid, int* own, int* spill) {
  const unsigned later = c.heads >> (q + 1);
  *spill = 0;
  if (later) { *own = __ffs(later); return *own; }
  *own = c.len - q;
  int len = *own;
  for (int k = (int)threadIdx.x + 1; k * kTvChunk < n_valid; k++) {
    const unsigned h = s_heads[k];
    const int klen = n_valid - k * kTvChunk < kTvChunk ? n_valid - k * kTvChunk : kTvChunk;
    ++*spill;
    if (h) { len += __ffs(h) - 1; break; }
    len += klen;
  }
  return len;
}

// the small LDS of V1 and V3: the log tile, every chunk's head mask, the wave totals
struct TvShared { TmObsTile obs; unsigned short heads[kTvBlock]; int tot[kTvWaves][9]; };
// V1 and V3 are one body: the entries, the sort and the runs must be the same in both
template <bool kWrite>
__device__ __forceinline__ void tv_model(const TrackModelBuffers& a, int b0, int flags, const TrackVoxelArgs& v, const mot_track_model* __restrict__ plan,
                                         TrackVoxelResult* __restrict__ res, mot_model_voxel* __restrict__ voxels, long voxel_stride,
                                         const mot_track_voxel_model* __restrict__ models, TvShared& sh, unsigned long long* s_ent, float* s_xyz, unsigned short* s_pos,
                                         double* s_lead) {
  TmObsTile& s_obs = sh.obs;
  unsigned short* s_heads = sh.heads;
  int (*s_tot)[9] = sh.tot;
  const int r = blockIdx.x, kb = blockIdx.y, b = b0 + kb, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the plan's header of this row (the whole workgroup reads the same words: every exit below is taken by all of it)
  const mot_track_model pm = plan[(long)kb * a.T + r];
  if (pm.track_id < 0) return;
  int n_write = 0;
  long first = 0;
  if (kWrite) {
    const mot_track_voxel_model* h = models + (long)kb * a.T + r;
    n_write = h->count; first = h->first;
    if (h->track_id < 0 || n_write <= 0 || first < 0 || first >= voxel_stride) return;
  }
  const long at = (long)b * a.T + r;
  const mot_accum_row row = a.rows[at];
  const TmRing g = tm_ring(row, a.K, a.O);
  int count = pm.count;
  if (count > g.kept) count = g.kept;
  if (count > kTvMaxK) count = kTvMaxK;
  if (g.n_obs <= 0) count = 0;
  if (count <= 0) {   // a logged observation and no record: a model without voxels
    if (!kWrite && tid == 0) {
      TrackVoxelResult z = {};
      res[(long)kb * a.T + r] = z;
    }
    return;
  }
  const bool axes = (flags & MOT_MODEL_AXES) != 0;
  int n2 = 64;
  while (n2 < count) n2 <<= 1;
  for (int i = count + tid; i < n2; i += kTvBlock) s_ent[i] = kTvOutside;
  int n_out = 0;
  int lo_x = 0x7fffffff, lo_y = 0x7fffffff, lo_z = 0x7fffffff, hi_x = (int)0x80000000, hi_y = (int)0x80000000, hi_z = (int)0x80000000;
  tv_stream(a, at, g, count, axes, s_obs, [&](int i, const float4& q) {
    unsigned key;
    const bool in = tv_key(q, v, &key);
    s_ent[i] = in ? ((unsigned long long)key << kTvIndexBits) | (unsigned)i : kTvOutside;
    n_out += in ? 0 : 1;
    if (!kWrite && tm_finite(q.x) && tm_finite(q.y) && tm_finite(q.z)) {
      const int ix = tm_image(q.x), iy = tm_image(q.y), iz = tm_image(q.z);
      lo_x = ix < lo_x ? ix : lo_x; hi_x = ix > hi_x ? ix : hi_x;
      lo_y = iy < lo_y ? iy : lo_y; hi_y = iy > hi_y ? iy : hi_y;
      lo_z = iz < lo_z ? iz : lo_z; hi_z = iz > hi_z ? iz : hi_z;
    }
  });
  tv_sort(s_ent, n2);
  // the records that take part are the first n_valid sorted entries
  n_out = wave_sum_i32(n_out);
  if (lane == 0) s_tot[wave][0] = n_out;
  __syncthreads();
  int n_outside = 0;
#pragma unroll
  for (int w = 0; w < kTvWaves; w++) n_outside += s_tot[w][0];
  const int n_valid = count - n_outside;
  const TvChunk c = tv_heads(s_ent, n_valid);
  s_heads[tid] = (unsigned short)c.heads;
  if (kWrite)
    for (int q = 0; q < c.len; q++) s_pos[(int)(s_ent[c.c0 + q] & ((1u << kTvIndexBits) - 1)) & (kTvMaxK - 1)] = (unsigned short)(c.c0 + q);
  __syncthreads();   // (the heads of the chunks behind; the totals above are read)
  int kept = 0, sparse = 0;
  for (unsigned m = c.heads; m; m &= m - 1) {
    int own, spill;
    const int len = tv_run(c, __ffs(m) - 1, s_heads, n_valid, &own, &spill);
    if (len >= v.min_points) kept++; else sparse++;
  }
  if (!kWrite) {
    kept = wave_sum_i32(kept); sparse = wave_sum_i32(sparse);
    lo_x = wave_reduce_i32(lo_x, OpMinI()); lo_y = wave_reduce_i32(lo_y, OpMinI()); lo_z = wave_reduce_i32(lo_z, OpMinI());
    hi_x = wave_reduce_i32(hi_x, OpMaxI()); hi_y = wave_reduce_i32(hi_y, OpMaxI()); hi_z = wave_reduce_i32(hi_z, OpMaxI());
    if (lane == 0) {
      int* t = s_tot[wave];
      t[1] = kept; t[2] = sparse; t[3] = lo_x; t[4] = lo_y; t[5] = lo_z; t[6] = hi_x; t[7] = hi_y; t[8] = hi_z;
    }
    __syncthreads();
    if (tid == 0) {
      TrackVoxelResult o = {};
      for (int w = 0; w < kTvWaves; w++) {
        const int* t = s_tot[w];
        o.n_voxels += t[1]; o.n_sparse += t[2];
        if (w == 0 || t[3] < lo_x) lo_x = t[3];
        if (w == 0 || t[4] < lo_y) lo_y = t[4];
        if (w == 0 || t[5] < lo_z) lo_z = t[5];
        if (w == 0 || t[6] > hi_x) hi_x = t[6];
        if (w == 0 || t[7] > hi_y) hi_y = t[7];
        if (w == 0 || t[8] > hi_z) hi_z = t[8];
      }
      o.n_outside = n_outside; o.n_records = count;
      if (lo_x <= hi_x) {   // (a finite record sets all six)
        o.min_x = tm_float(lo_x); o.min_y = tm_float(lo_y); o.min_z = tm_float(lo_z);
        o.max_x = tm_float(hi_x); o.max_y = tm_float(hi_y); o.max_z = tm_float(hi_z);
      }
      res[(long)kb * a.T + r] = o;
    }
    return;
  }
  // ---- V3 only: the voxel number of this thread's first head, the records at their sorted position, the sums
  // block_scan_excl_i32 parks its wave totals in the first kTvWaves words of the table: V3 writes nothing there but the column of n_outside, and
  // that one was read before the barrier above. (Behind its barrier every entry has been read as well: the coordinates take their place)
  int voxel = block_scan_excl_i32<kTvWaves>(kept, &s_tot[0][0]);
  tv_stream(a, at, g, count, axes, s_obs, [&](int i, const float4& q) {
    unsigned key;
    if (!tv_key(q, v, &key)) return;
    const int p = s_pos[i] < n_valid ? s_pos[i] : 0;   // (i < count <= kTvMaxK; a valid record's position was written above)
    s_xyz[3 * p] = q.x; s_xyz[3 * p + 1] = q.y; s_xyz[3 * p + 2] = q.z;
  });
  __syncthreads();   // (the positions are read: the leading sums take their place)
  {
    const int lead = c.heads ? __ffs(c.heads) - 1 : c.len;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int q = 0; q < lead; q++) { sx += (double)s_xyz[3 * (c.c0 + q)]; sy += (double)s_xyz[3 * (c.c0 + q) + 1]; sz += (double)s_xyz[3 * (c.c0 + q) + 2]; }
    s_lead[3 * tid] = sx; s_lead[3 * tid + 1] = sy; s_lead[3 * tid + 2] = sz;
  }
  __syncthreads();
  mot_model_voxel* __restrict__ out = voxels + (long)kb * voxel_stride;
  for (unsigned m = c.heads; m; m &= m - 1) {
    const int q = __ffs(m) - 1;
    int own, spill;
    const int len = tv_run(c, q, s_heads, n_valid, &own, &spill);
    if (len < v.min_points) continue;
    const int k = voxel++;
    if (k >= n_write || first + k >= voxel_stride) continue;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int e = 0; e < own; e++) { sx += (double)s_xyz[3 * (c.c0 + q + e)]; sy += (double)s_xyz[3 * (c.c0 + q + e) + 1]; sz += (double)s_xyz[3 * (c.c0 + q + e) + 2]; }
    for (int e = 1; e <= spill; e++) { sx += s_lead[3 * (tid + e)]; sy += s_lead[3 * (tid + e) + 1]; sz += s_lead[3 * (tid + e) + 2]; }   // (tid + spill < kTvBlock: those chunks hold valid entries)
    mot_model_voxel o;
    o.x = (float)(sx / (double)len); o.y = (float)(sy / (double)len); o.z = (float)(sz / (double)len); o.count = len;
    out[first + k] = o;
  }
}

// ------------------------------------------------------------------------------------------ V1
__global__ void MOT_TV_BOUNDS(kTvBlock)
track_voxels_count_kernel(TrackModelBuffers a, int b0, int flags, TrackVoxelArgs v, const mot_track_model* __restrict__ plan, TrackVoxelResult* __restrict__ res) {
  __shared__ unsigned long long s_ent[kTvMaxK];
  __shared__ TvShared sh;
  tv_model<false>(a, b0, flags, v, plan, res, nullptr, 0, nullptr, sh, s_ent, nullptr, nullptr, nullptr);
}

// ------------------------------------------------------------------------------------------ V2
__global__ void MOT_TV_BOUNDS(kTvBlock)
track_voxels_pack_kernel(int T, int K, const mot_track_model* __restrict__ plan, const TrackVoxelResult* __restrict__ res, mot_track_voxel_model* __restrict__ models,
                         int* __restrict__ counts) {
  __shared__ int s_tot[kTvWaves * 2];
  const int kb = blockIdx.x, tid = threadIdx.x;
  int base_voxels = 0, base_models = 0;
  for (int r0 = 0; r0 < T; r0 += kTvBlock) {   // (the same rounds for every thread: the scan below is a collective)
    const int r = r0 + tid;
    mot_track_voxel_model m = {};
    m.track_id = -1;
    if (r < T) {
      const mot_track_model pm = plan[(long)kb * T + r];
      if (pm.track_id >= 0) {
        const TrackVoxelResult o = res[(long)kb * T + r];
        m.track_id = pm.track_id; m.n_obs = pm.n_obs; m.first_step = pm.first_step; m.last_step = pm.last_step;
        m.count = o.n_voxels < 0 ? 0 : (o.n_voxels > K ? K : o.n_voxels);
        m.min_x = o.min_x; m.min_y = o.min_y; m.min_z = o.min_z; m.max_x = o.max_x; m.max_y = o.max_y; m.max_z = o.max_z;
        m.n_records = pm.count; m.n_outside = o.n_outside; m.n_sparse = o.n_sparse;
      }
    }
    // the voxels before this row's and, under the same barrier, the round's models (block_scan_excl_i32; only the total of the second is used)
    const int v[2] = {m.count, m.track_id >= 0 ? 1 : 0};
    int before[2], all[2];
    block_scan_excl_i32<kTvWaves, 2>(v, s_tot, before, all);
    if (m.track_id >= 0) m.first = base_voxels + before[0];
    if (r < T) models[(long)kb * T + r] = m;
    base_voxels += all[0]; base_models += all[1];
    __syncthreads();   // (the totals are read: the next round may write them)
  }
  if (tid == 0) { counts[2 * kb] = base_models; counts[2 * kb + 1] = base_voxels; }
}

// ------------------------------------------------------------------------------------------ V3
__global__ void MOT_TV_BOUNDS(kTvBlock)
track_voxels_write_kernel(TrackModelBuffers a, int b0, int flags, TrackVoxelArgs v, const mot_track_model* __restrict__ plan, mot_model_voxel* __restrict__ voxels,
                          long voxel_stride, const mot_track_voxel_model* __restrict__ models) {
  // the entries while they are sorted, then the records' coordinates at their sorted position; the inverse permutation, then every chunk's leading sums
  __shared__ unsigned char s_big[kTvMaxK * 12] __attribute__((aligned(16)));
  __shared__ unsigned char s_aux[kTvBlock * 3 * 8] __attribute__((aligned(16)));
  static_assert(kTvMaxK * 12 >= kTvMaxK * 8 && kTvBlock * 3 * 8 >= kTvMaxK * 2, "what shares the two blocks fits them");
  __shared__ TvShared sh;
  tv_model<true>(a, b0, flags, v, plan, nullptr, voxels, voxel_stride, models, sh, reinterpret_cast<unsigned long long*>(s_big), reinterpret_cast<float*>(s_big),
                 reinterpret_cast<unsigned short*>(s_aux), reinterpret_cast<double*>(s_aux));
}

// ------------------------------------------------------------------------------------------ host
void mot_launch_track_voxels_count(const TrackModelBuffers& a, int first, int batch, int flags, const TrackVoxelArgs& v, const mot_track_model* plan, TrackVoxelResult* res,
                                   mot_track_voxel_model* models, int* counts, hipStream_t stream) {
  hipLaunchKernelGGL(track_voxels_count_kernel, dim3(a.T, batch), dim3(kTvBlock), 0, stream, a, first, flags, v, plan, res);
  hipLaunchKernelGGL(track_voxels_pack_kernel, dim3(batch), dim3(kTvBlock), 0, stream, a.T, a.K, plan, res, models, counts);
}
void mot_launch_track_voxels_write(const TrackModelBuffers& a, int first, int batch, int flags, const TrackVoxelArgs& v, const mot_track_model* plan, mot_model_voxel* voxels,
                                   long voxel_stride, const mot_track_voxel_model* models, hipStream_t stream) {
  hipLaunchKernelGGL(track_voxels_write_kernel, dim3(a.T, batch), dim3(kTvBlock), 0, stream, a, first, flags, v, plan, voxels, voxel_stride, models);
}
