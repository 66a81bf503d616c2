// mot_sort.h — a device-wide STABLE radix sort of 64-bit keys with a 32-bit payload, least significant digit first, on gfx950 (HIP, wave64). Product code; a primitive
// beside mot_wave.h: it knows keys, payloads and a count, nothing of what they stand for.
//
// One pass per 8-bit digit, three launches a pass, over tiles of kSortTile = 2048 elements (256 threads, 8 elements a thread):
//   P1  radix_sort_hist_kernel     one workgroup per tile: the tile's elements per digit value (an LDS table, integer adds) -> table[digit][tile]
//   P2  radix_sort_scan_kernel     one workgroup per digit VALUE (256): the exclusive scan of its row over the tiles, 256 tiles a round (block_scan_excl_i32), the carry in
//                                  a register -> table[digit][tile] = the digit's elements in earlier tiles, totals[digit]
//   P3  radix_sort_scatter_kernel  one workgroup per tile: the exclusive scan of the 256 totals (every workgroup repeats it: 256 ints) gives where a digit value starts;
//                                  wave w owns elements [512 w, 512 w + 512) of the tile, 64 at a time in position order. The lanes that hold the same digit value find
//                                  each other with eight ballots; a lane's place is (the value's start) + (earlier tiles) + (earlier waves of the tile) + (earlier
//                                  rounds of the wave, a per-wave LDS counter its first lane of the value advances) + (earlier lanes, a popcount). Equal digits keep
//                                  their order: the pass is stable, and so is the sort.
// The element count is read ON THE DEVICE (*n, clamped to [0, cap]); the launches are sized by cap, the capacity of the buffers, and a workgroup whose tile lies behind
// the count leaves at once: the number of launches depends on the key width alone, never on the data. No global atomics, no workgroup waits on another (no decoupled
// look-back): the order between the launches is the only synchronisation, and every place is a sum of integers over a fixed set — the output does not depend on how
// workgroups or waves are scheduled. INDEX SAFETY: every load is below min(*n, cap); a place outside [0, min(*n, cap)) is not stored (there is none while the table is
// this pass's own); positions are int32 (cap <= 2^31 - 1).
// Keys and payloads ping-pong between two buffers each: 24 bytes per element of capacity, and 4 bytes per (digit value, tile) for the table.
// tests/sort_cases.py holds the sort to np.argsort(kind="stable") (tests/devcheck/sort.hip). The kernels are DEFINED here with internal linkage (static): every
// translation unit that includes the header gets its own.
#ifndef MOT_SORT_H_
#define MOT_SORT_H_
#include "mot_wave.h"   // block_scan_excl_i32, MOT_WAVE_SYNC: the only header this one needs

#ifndef MOT_HIPEMU
#define MOT_SORT_BOUNDS(n) __launch_bounds__(n)
#else
#define MOT_SORT_BOUNDS(n)
#endif

constexpr int kSortBlock = 256, kSortWaves = kSortBlock / 64, kSortItems = 8;
constexpr int kSortTile = kSortBlock * kSortItems;           // elements per workgroup (tests/sort_cases.py and tests/scene_voxel_seq_cases.py mirror it)
constexpr int kSortDigitBits = 8, kSortBins = 1 << kSortDigitBits;
static_assert(kSortBins == kSortBlock, "thread d owns digit value d in the three kernels");

struct SortPass {
  const unsigned long long* key_in; const unsigned* val_in;
  unsigned long long* key_out; unsigned* val_out;
  int* table;     // [kSortBins][tiles]
  int* totals;    // [kSortBins]
  const int* n;   // on the device: the elements in play
  int cap, tiles; // capacity of the four buffers; tiles = mot_sort_tiles(cap), the workgroups of P1 and P3
  int shift;      // the pass's digit: bits [shift, shift + 8) of the key
};
inline int mot_sort_tiles(long cap) { const long t = (cap + kSortTile - 1) / kSortTile; return t < 1 ? 1 : (int)t; }
// the elements in play: *n clamped to what the buffers hold
__device__ __forceinline__ int sort_count(const int* n, int cap) { const int v = *n; return v < 0 ? 0 : (v > cap ? cap : v); }

// P1. s_hist: kSortBins ints. Every thread of a workgroup that passes the exit reaches both barriers
__device__ __forceinline__ void sort_hist_body(const SortPass& p, int* s_hist) {
  const int tid = threadIdx.x, tile = blockIdx.x;
  const int n = sort_count(p.n, p.cap);
  const long base = (long)tile * kSortTile;
  if (base >= n || tile >= p.tiles) return;   // (uniform over the workgroup)
  s_hist[tid] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kSortItems; k++) {
    const long i = base + k * kSortBlock + tid;
    if (i < n) atomicAdd(&s_hist[(int)((p.key_in[i] >> p.shift) & (kSortBins - 1))], 1);   // (LDS, integers: the sum does not depend on the order)
  }
  __syncthreads();
  p.table[(long)tid * p.tiles + tile] = s_hist[tid];
}

// P2. s_part: kSortWaves ints
__device__ __forceinline__ void sort_scan_body(const SortPass& p, int* s_part) {
  const int tid = threadIdx.x, d = blockIdx.x;
  const int n = sort_count(p.n, p.cap);
  int live = (int)(((long)n + kSortTile - 1) / kSortTile);   // the tiles that hold an element: the rows P1 wrote
  if (live > p.tiles) live = p.tiles;
  int* __restrict__ row = p.table + (long)d * p.tiles;
  int carry = 0;   // the digit value's elements in the tiles of earlier rounds
  for (int t0 = 0; t0 < live; t0 += kSortBlock) {   // (uniform)
    const int t = t0 + tid;
    const int v = t < live ? row[t] : 0;
    int total;
    const int first = carry + block_scan_excl_i32<kSortWaves>(v, s_part, total);
    carry += total;
    __syncthreads();   // (s_part is written again in the next round)
    if (t < live) row[t] = first;
  }
  if (tid == 0) p.totals[d] = carry;
}

// P3. s_at: [kSortWaves][kSortBins] ints, s_part: kSortWaves ints
__device__ __forceinline__ void sort_scatter_body(const SortPass& p, int (*s_at)[kSortBins], int* s_part) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x;
  const int n = sort_count(p.n, p.cap);
  const long base = (long)tile * kSortTile;
  if (base >= n || tile >= p.tiles) return;   // (uniform over the workgroup)
  const int start = block_scan_excl_i32<kSortWaves>(p.totals[tid], s_part);   // where digit value tid starts in the output
#pragma unroll
  for (int w = 0; w < kSortWaves; w++) s_at[w][tid] = 0;
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned long long key[kSortItems];
  unsigned val[kSortItems];
  int off[kSortItems];   // the element's place among those of its digit value in this wave
#pragma unroll
  for (int k = 0; k < kSortItems; k++) {
    const long i = base + (long)wave * (64 * kSortItems) + k * 64 + lane;
    const bool valid = i < n;
    key[k] = valid ? p.key_in[i] : ~0ull;
    val[k] = valid ? p.val_in[i] : 0u;
    const int digit = (int)((key[k] >> p.shift) & (kSortBins - 1));
    unsigned long long same = __ballot(valid);   // the lanes that hold this lane's digit value
#pragma unroll
    for (int b = 0; b < kSortDigitBits; b++) {
      const unsigned long long has = __ballot((digit >> b) & 1);
      same &= ((digit >> b) & 1) ? has : ~has;
    }
    const int rank = __popcll(same & below);
    const int before = valid ? s_at[wave][digit] : 0;   // the value's elements in the wave's earlier rounds
    MOT_WAVE_SYNC();   // (every lane has read the counter)
    if (valid && rank == 0) s_at[wave][digit] = before + __popcll(same);
    MOT_WAVE_SYNC();   // (... and the next round reads what this one left)
    off[k] = before + rank;
  }
  __syncthreads();
  {   // thread d: s_at[w][d] from wave w's count of value d to where its first such element goes
    int run = start + p.table[(long)tid * p.tiles + tile];
#pragma unroll
    for (int w = 0; w < kSortWaves; w++) { const int c = s_at[w][tid]; s_at[w][tid] = run; run += c; }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kSortItems; k++) {
    const long i = base + (long)wave * (64 * kSortItems) + k * 64 + lane;
    if (i >= n) continue;
    const int dst = s_at[wave][(int)((key[k] >> p.shift) & (kSortBins - 1))] + off[k];
    if (dst < 0 || dst >= n) continue;   // never a store outside the elements in play
    p.key_out[dst] = key[k]; p.val_out[dst] = val[k];
  }
}

static __global__ void MOT_SORT_BOUNDS(kSortBlock) radix_sort_hist_kernel(SortPass p) {
  __shared__ int s_hist[kSortBins];
  sort_hist_body(p, s_hist);
}
static __global__ void MOT_SORT_BOUNDS(kSortBlock) radix_sort_scan_kernel(SortPass p) {
  __shared__ int s_part[kSortWaves];
  sort_scan_body(p, s_part);
}
static __global__ void MOT_SORT_BOUNDS(kSortBlock) radix_sort_scatter_kernel(SortPass p) {
  __shared__ int s_at[kSortWaves][kSortBins];
  __shared__ int s_part[kSortWaves];
  sort_scatter_body(p, s_at, s_part);
}

// the buffers of a sort: key[0] / val[0] hold the input, table kSortBins * mot_sort_tiles(cap) ints, totals kSortBins ints
struct SortBuffers {
  unsigned long long* key[2]; unsigned* val[2];
  int* table; int* totals;
  const int* n; int cap;
};
// bits [0, key_bits) of the keys decide the order (the bits above are carried along): ceil(key_bits / 8) passes of three launches. Returns which of the two buffers
// holds the result (passes & 1)
inline int mot_sort_launch(const SortBuffers& b, int key_bits, hipStream_t stream) {
  const int passes = (key_bits + kSortDigitBits - 1) / kSortDigitBits;
  SortPass p;
  p.table = b.table; p.totals = b.totals; p.n = b.n; p.cap = b.cap; p.tiles = mot_sort_tiles(b.cap);
  for (int k = 0; k < passes; k++) {
    p.key_in = b.key[k & 1]; p.val_in = b.val[k & 1]; p.key_out = b.key[(k + 1) & 1]; p.val_out = b.val[(k + 1) & 1]; p.shift = k * kSortDigitBits;
    hipLaunchKernelGGL(radix_sort_hist_kernel, dim3(p.tiles), dim3(kSortBlock), 0, stream, p);
    hipLaunchKernelGGL(radix_sort_scan_kernel, dim3(kSortBins), dim3(kSortBlock), 0, stream, p);
    hipLaunchKernelGGL(radix_sort_scatter_kernel, dim3(p.tiles), dim3(kSortBlock), 0, stream, p);
  }
  return passes & 1;
}
#endif  // MOT_SORT_H_
