// regroup.hip — MOT_ORDER_ANY: every frame's elevated points put into cluster order before the box stage. Product code (HIP, wave64).
//
// The reference's boxFitting first copies the cloud into one vector per cluster (getClusteredPoints, box_fitting.cpp:46-72), so it takes a
// cloud in any point order. box.hip copies nothing: it describes a cluster by its (tile, cluster) groups, which is compact only while a
// cluster's points are neighbours in memory. For clouds in no order (merged sensors, voxel / KD-tree filtered clouds, non-repetitive
// scanners) the kernels here make them neighbours: a STABLE sort of the frame's elevated points by cluster label, and a copy of the points
// (and their cells) in that order, on which the box stage then runs unchanged. Everything order-dependent the box stage computes — a
// cluster's first point, the "first occurrence wins" slope extrema, the k-th point of the L-shape draws, the float centroid sums of the
// markers — depends on the order INSIDE a cluster only, and a stable sort keeps that order.
//
//   R1  regroup_label_kernel     N_e pts -> 16-bit key of every point (its label, 0 .. 4096; 0 = no cluster) + per-point labels in input order
//                                           on request + the chunk's histogram of the key's low 7 bits
//   R2  regroup_scan_kernel      one workgroup per frame: the histograms -> where each chunk's points of each digit go (digit-major)
//       regroup_scatter0_kernel  stable scatter by the low digit: {input index, high digit} of every point, 4 bytes
//       regroup_hist1_kernel     histogram of the high 6 bits per chunk of that sequence; regroup_scan_kernel again
//   R3  regroup_gather_kernel    stable scatter by the high digit, carrying the point: 12 bytes (+ 2 of the cell) read through the index,
//                                written at the point's place in the copy
//
// Unlabelled points (key 0) are KEPT, in front of the copy: the box stage runs on all N_e points with the frame's own count, its label
// kernel finds no cluster in those leading tiles and skips them.
// Stability: a point's place is (points of smaller digits) + (points of its digit in earlier chunks) + (points of its digit earlier in its
// chunk). The last term is exact and free of atomics: a chunk is 32 tiles of 64 consecutive points, one wave per tile at a time; within a
// tile the lanes holding a digit are found by ballots on the digit's bits (rank = lower lanes among them), and the tile's count per digit
// goes into an LDS table [tile][digit] whose prefix over the tiles one thread per digit forms. Nothing depends on scheduling.
// Bytes per elevated point (fused path): R1 2 (cell) + 2 (grid, cached) read, 2 written; scatter0 2 + 4; hist1 4; R3 4 + 12 + 2 read through
// the index, 12 + 2 written: 28 read + 20 written = 48 bytes, against the 12 + 2 + 4 (pixel) the label kernel moves.
#include "mot_internal.h"
#include "mot_wave.h"

#ifndef MOT_HIPEMU
#define MOT_RG_BOUNDS(n) __launch_bounds__(n)
#else
#define MOT_RG_BOUNDS(n)
#endif

constexpr int kRgBlock = 256, kRgItems = 8;
constexpr int kRgChunk = kRgBlock * kRgItems;    // 2048 points: the label kernel's chunk, so c.max_wg counts these chunks too
constexpr int kRgTiles = kRgChunk / 64;
constexpr int kRgBits0 = 7, kRgBits1 = 6;        // 13 bits: keys 0 .. 4096
constexpr int kRgIdxBits = 21;                   // frames of up to 2^21 - 1 points (kMaxPointsPerFrame)
constexpr unsigned kRgIdxMask = (1u << kRgIdxBits) - 1u;
static_assert((1 << kRgBits0) <= kRegroupDigits && (1 << kRgBits1) <= kRegroupDigits, "histogram row too short");
static_assert((1 << (kRgBits0 + kRgBits1)) > kMaxClusters, "two digits must hold every key");
static_assert(kRgIdxBits + kRgBits1 <= 32 && kMaxPointsPerFrame <= (int)kRgIdxMask, "index | high digit in 32 bits");
static_assert(kRgBlock >= kRegroupDigits && kRgChunk <= 65535, "one thread per digit; chunk prefixes in 16 bits");

// the frame's elevated points as every kernel here sees them (never beyond the slot: the count is the device's)
__device__ __forceinline__ int rg_count(const ClusterBuffers& c, int b) {
  const int n = c.counts[b * kCountsStride + kCntElev];
  return n < 0 ? 0 : (n < (int)c.cap ? n : (int)c.cap);
}

// ------------------------------------------------------------------------------------------ R1
__global__ void MOT_RG_BOUNDS(kRgBlock)
regroup_label_kernel(MotDevParams p, ClusterBuffers c, RegroupBuffers r) {
  __shared__ int s_hist[kRegroupDigits];
  const int b = blockIdx.y;
  const int n = rg_count(c, b);
  const long base = (long)blockIdx.x * kRgChunk;
  if (base >= n || (int)blockIdx.x >= c.max_wg) return;
  if (threadIdx.x < kRegroupDigits) s_hist[threadIdx.x] = 0;
  __syncthreads();
  const int num_cluster = c.counts[b * kCountsStride + kCntClusters];
  unsigned short* __restrict__ key = r.key + (long)b * c.cap;
  int* __restrict__ label = r.label ? r.label + (long)b * c.cap : nullptr;
#pragma unroll
  for (int k = 0; k < kRgItems; k++) {
    const long i = base + k * kRgBlock + threadIdx.x;
    if (i < n) {
      int lab = mot_point_label(p, c, b, i, num_cluster);
      if (label) label[i] = lab;
      if (lab > kMaxClusters) lab = 0;   // no statistics slot in the box stage either: box_finalize_kernel raises the capacity flag
      key[i] = (unsigned short)lab;
      atomicAdd(&s_hist[lab & ((1 << kRgBits0) - 1)], 1);
    }
  }
  __syncthreads();
  if (threadIdx.x < kRegroupDigits) r.hist[((long)b * c.max_wg + blockIdx.x) * kRegroupDigits + threadIdx.x] = s_hist[threadIdx.x];
}

// ------------------------------------------------------------------------------------------ R2
// hist[chunk][digit] (counts) -> the place of the chunk's first point of that digit: all points of smaller digits, then the digit's points
// of earlier chunks. One thread per digit walks the chunks (consecutive threads read consecutive words).
__global__ void MOT_RG_BOUNDS(kRegroupDigits)
regroup_scan_kernel(ClusterBuffers c, RegroupBuffers r) {
  __shared__ int s_part[kRegroupDigits / 64];
  const int b = blockIdx.x, d = threadIdx.x;
  const int n = rg_count(c, b);
  int chunks = (n + kRgChunk - 1) / kRgChunk;
  if (chunks > c.max_wg) chunks = c.max_wg;
  int* __restrict__ h = r.hist + (long)b * c.max_wg * kRegroupDigits;
  int sum = 0;
  for (int ch = 0; ch < chunks; ch++) sum += h[ch * kRegroupDigits + d];
  int run = block_scan_excl_i32<kRegroupDigits / 64>(sum, s_part);   // all points of smaller digits
  for (int ch = 0; ch < chunks; ch++) {
    const int v = h[ch * kRegroupDigits + d];
    h[ch * kRegroupDigits + d] = run;
    run += v;
  }
}

__global__ void MOT_RG_BOUNDS(kRgBlock)
regroup_hist1_kernel(ClusterBuffers c, RegroupBuffers r) {
  __shared__ int s_hist[kRegroupDigits];
  const int b = blockIdx.y;
  const int n = rg_count(c, b);
  const long base = (long)blockIdx.x * kRgChunk;
  if (base >= n || (int)blockIdx.x >= c.max_wg) return;
  if (threadIdx.x < kRegroupDigits) s_hist[threadIdx.x] = 0;
  __syncthreads();
  const unsigned* __restrict__ tmp = r.tmp + (long)b * c.cap;
#pragma unroll
  for (int k = 0; k < kRgItems; k++) {
    const long i = base + k * kRgBlock + threadIdx.x;
    if (i < n) atomicAdd(&s_hist[(tmp[i] >> kRgIdxBits) & ((1u << kRgBits1) - 1u)], 1);
  }
  __syncthreads();
  if (threadIdx.x < kRegroupDigits) r.hist[((long)b * c.max_wg + blockIdx.x) * kRegroupDigits + threadIdx.x] = s_hist[threadIdx.x];
}

// ------------------------------------------------------------------------------------------ stable scatter of one chunk
// PASS 0: by the key's low digit, writes {input index | high digit}. PASS 1: by the high digit, writes the point and its cell.
template <int PASS>
static __device__ __forceinline__ void regroup_scatter_body(const ClusterBuffers& c, const RegroupBuffers& r) {
  constexpr int kBits = PASS == 0 ? kRgBits0 : kRgBits1, kDigits = 1 << kBits;
  __shared__ unsigned short s_cnt[kRgTiles][kRegroupDigits];   // points of (tile, digit), then the digit's points in the chunk's earlier tiles
  __shared__ int s_goff[kRegroupDigits];                       // where the chunk's points of a digit start (scan kernel)
  const int b = blockIdx.y;
  const int n = rg_count(c, b);
  const long base = (long)blockIdx.x * kRgChunk;
  if (base >= n || (int)blockIdx.x >= c.max_wg) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < kRgTiles * kRegroupDigits / 2; i += kRgBlock) reinterpret_cast<unsigned*>(&s_cnt[0][0])[i] = 0u;
  unsigned dig[kRgItems], pay[kRgItems];
#pragma unroll
  for (int k = 0; k < kRgItems; k++) {
    const long i = base + k * kRgBlock + threadIdx.x;
    dig[k] = 0u; pay[k] = 0u;
    if (i < n) {
      if (PASS == 0) {
        const unsigned key = r.key[(long)b * c.cap + i];
        dig[k] = key & (unsigned)(kDigits - 1);
        pay[k] = (unsigned)i | ((key >> kRgBits0) << kRgIdxBits);
      } else {
        const unsigned v = r.tmp[(long)b * c.cap + i];
        dig[k] = (v >> kRgIdxBits) & (unsigned)(kDigits - 1);
        pay[k] = v & kRgIdxMask;
      }
    }
  }
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  int rank[kRgItems];
#pragma unroll
  for (int k = 0; k < kRgItems; k++) {
    const long i = base + k * kRgBlock + threadIdx.x;
    const int tile = k * (kRgBlock / 64) + wave;   // of the chunk: points 64 * tile .. 64 * tile + 63, in index order
    unsigned long long same = __ballot(i < n);     // the lanes of this tile that hold my digit
#pragma unroll
    for (int bit = 0; bit < kBits; bit++) {
      const unsigned long long set = __ballot((dig[k] >> bit) & 1u);
      same &= ((dig[k] >> bit) & 1u) ? set : ~set;
    }
    rank[k] = __popcll(same & below);
    if (i < n && rank[k] == 0) s_cnt[tile][dig[k]] = (unsigned short)__popcll(same);   // the lowest lane of each digit present
  }
  __syncthreads();
  if (threadIdx.x < kDigits) {
    int run = 0;
#pragma unroll
    for (int t = 0; t < kRgTiles; t++) { const int v = s_cnt[t][threadIdx.x]; s_cnt[t][threadIdx.x] = (unsigned short)run; run += v; }
    s_goff[threadIdx.x] = r.hist[((long)b * c.max_wg + blockIdx.x) * kRegroupDigits + threadIdx.x];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kRgItems; k++) {
    const long i = base + k * kRgBlock + threadIdx.x;
    if (i >= n) continue;
    const int tile = k * (kRgBlock / 64) + wave;
    const unsigned dst = (unsigned)(s_goff[dig[k]] + (int)s_cnt[tile][dig[k]] + rank[k]);
    if (dst >= (unsigned)n) continue;   // (cannot happen while the histograms are this frame's; never a store outside the slot)
    if (PASS == 0) {
      r.tmp[(long)b * c.cap + dst] = pay[k];
    } else {
      const long src = (long)pay[k];
      if (src >= n) continue;
      const float4 q = mot_load_xyz(c.elevated + (long)b * c.cap, src, c.elevated_packed);
      PackedXyz o; o.x = q.x; o.y = q.y; o.z = q.z;
      reinterpret_cast<PackedXyz*>(r.xyz + (long)b * c.cap)[dst] = o;
      if (c.ecell) r.cell[(long)b * c.cap + dst] = c.ecell[(long)b * c.cap + src];
    }
  }
}
__global__ void MOT_RG_BOUNDS(kRgBlock)
regroup_scatter0_kernel(ClusterBuffers c, RegroupBuffers r) { regroup_scatter_body<0>(c, r); }
// ------------------------------------------------------------------------------------------ R3
__global__ void MOT_RG_BOUNDS(kRgBlock)
regroup_gather_kernel(ClusterBuffers c, RegroupBuffers r) { regroup_scatter_body<1>(c, r); }

// ------------------------------------------------------------------------------------------ host
void mot_launch_regroup(int which, const MotDevParams& p, const ClusterBuffers& src, const RegroupBuffers& r, int batch, int max_n, hipStream_t stream) {
  int chunks = (max_n + kRgChunk - 1) / kRgChunk;
  if (chunks < 1) chunks = 1;
  if (chunks > src.max_wg) chunks = src.max_wg;
  const dim3 grid(chunks, batch);
  if (which == 0 || which < 0) hipLaunchKernelGGL(regroup_label_kernel, grid, dim3(kRgBlock), 0, stream, p, src, r);
  if (which == 1 || which < 0) {
    hipLaunchKernelGGL(regroup_scan_kernel, dim3(batch), dim3(kRegroupDigits), 0, stream, src, r);
    hipLaunchKernelGGL(regroup_scatter0_kernel, grid, dim3(kRgBlock), 0, stream, src, r);
    hipLaunchKernelGGL(regroup_hist1_kernel, grid, dim3(kRgBlock), 0, stream, src, r);
    hipLaunchKernelGGL(regroup_scan_kernel, dim3(batch), dim3(kRegroupDigits), 0, stream, src, r);
  }
  if (which == 2 || which < 0) hipLaunchKernelGGL(regroup_gather_kernel, grid, dim3(kRgBlock), 0, stream, src, r);
}
